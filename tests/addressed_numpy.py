"""numpy statement of the addressed frame buffer of mvf_frames_addressed_resample_u8 (include/mvfnet_hip.h): frames of any size laid into
one flat byte buffer, each plane at its own offset and row pitch, and the (n, 5) int32 address rows (o0, p0, o1, o2, p1) that say where:
  packed  pixel (y, x) at o0 + y p0 + 3 x;
  I420    luma at o0 + y p0 + x, U at o1 + (y >> 1) p1 + (x >> 1), V at o2 + (y >> 1) p1 + (x >> 1);
  NV12    luma as I420, U at o1 + (y >> 1) p1 + 2 (x >> 1), V one byte after it.
`pack` builds such a buffer byte by byte from these formulas, `unpack` reads it back the same way.

TEST INFRASTRUCTURE ONLY -- never imported by mvfnet_amd."""
import numpy as np

PACKED, I420, NV12 = 0, 1, 2


def _planes(frame, format):
    """One frame -> its planes as 2-D byte images: packed (h, 3 w); I420 Y, U, V; NV12 Y and the interleaved (ch, 2 cw) U, V plane."""
    if format == PACKED:
        f = np.asarray(frame)
        assert f.ndim == 3 and f.shape[2] == 3 and f.dtype == np.uint8
        return [f.reshape(f.shape[0], -1)]
    y, u, v = (np.asarray(p) for p in frame)
    assert y.ndim == 2 and u.shape == v.shape == ((y.shape[0] + 1) // 2, (y.shape[1] + 1) // 2)
    if format == I420:
        return [y, u, v]
    return [y, np.stack((u, v), axis=-1).reshape(u.shape[0], -1)]


def pack(frames_or_planes, format, pitches=None, gaps=0, fill_seed=None):
    """frames_or_planes: a list of frames -- packed: (h, w, 3) uint8 arrays; I420 / NV12: (Y (h, w), U, V (ceil(h / 2), ceil(w / 2))) -- of
    ANY sizes.  pitches: per frame (p0, p1) in bytes (p1 ignored for packed; None = the row bytes); gaps: bytes left free in front of
    EVERY plane (an int, or one int per frame).  -> (bytes (total,) uint8, addr (n, 5) int32).  The bytes no plane owns (gaps, pitch
    padding) are zero, or random with `fill_seed`: nothing may depend on them."""
    n = len(frames_or_planes)
    gaps = [int(gaps)] * n if np.isscalar(gaps) else [int(g) for g in gaps]
    addr = np.zeros((n, 5), dtype=np.int64)
    todo, at = [], 0
    for i, frame in enumerate(frames_or_planes):
        planes = _planes(frame, format)
        p0 = planes[0].shape[1] if pitches is None else int(pitches[i][0])
        p1 = 0 if format == PACKED else (planes[1].shape[1] if pitches is None else int(pitches[i][1]))
        for k, pl in enumerate(planes):
            pitch = p0 if k == 0 else p1
            assert pitch >= pl.shape[1]
            at += gaps[i]
            todo.append((at, pitch, pl))
            addr[i, (0, 2, 3)[k]] = at
            at += (pl.shape[0] - 1) * pitch + pl.shape[1]          # the plane's last row is not padded: the buffer may end with its last byte
        addr[i, 1], addr[i, 4] = p0, p1
    buf = np.zeros(at, dtype=np.uint8) if fill_seed is None else np.random.RandomState(fill_seed).randint(0, 256, size=at).astype(np.uint8)
    for at0, pitch, pl in todo:
        for y in range(pl.shape[0]):
            buf[at0 + y * pitch:at0 + y * pitch + pl.shape[1]] = pl[y]
    assert at < (1 << 31)
    return buf, addr.astype(np.int32)


def unpack(buf, addr, sizes, format):
    """The inverse of pack: bytes + (n, 5) address rows + the frames' [(h, w)] -> the list of frames (packed (h, w, 3)) or (Y, U, V) planes."""
    buf, addr = np.asarray(buf).reshape(-1), np.asarray(addr, dtype=np.int64)

    def plane(o, p, rows, nbytes, step=1, first=0):
        idx = o + np.arange(rows)[:, None] * p + first + np.arange(nbytes)[None, :] * step
        return buf[idx]
    out = []
    for (o0, p0, o1, o2, p1), (h, w) in zip(addr, sizes):
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if format == PACKED:
            out.append(plane(o0, p0, h, 3 * w).reshape(h, w, 3))
        elif format == I420:
            out.append((plane(o0, p0, h, w), plane(o1, p1, ch, cw), plane(o2, p1, ch, cw)))
        else:
            out.append((plane(o0, p0, h, w), plane(o1, p1, ch, cw, 2, 0), plane(o1, p1, ch, cw, 2, 1)))
    return out
