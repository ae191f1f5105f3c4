"""CPU: RandomErasing (mvfnet_amd/erasing.py) -- the tables it draws, their validator, the config plumbing through Recognizer2D --, the numpy restatement of
the kernel's generator (erase_numpy.py) against the Random123 known answers, and the export behind it (mvf_stem_erase): declared, bound, and refusing bad
by-value arguments before anything is launched (no GPU is needed to be refused)."""
import ctypes as C
import math

import numpy as np
import pytest

import erase_numpy as EN
from mvfnet_amd import erasing as ER

H = W = 224
DRAWS, BATCH, T = 250, 8, 2             # 2000 clips per configuration


# ------------------------------------------------------------------------------------------------ the generator's restatement
def test_philox4x32_10_reproduces_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join("%08x" % int(w) for w in EN.philox4x32_10(counter, key)) == want
    # vectorised: two counters under one key in one call give what each gives alone
    w = EN.philox4x32_10((np.array([0, 5]), np.array([0, 7]), 0, 0), (0, 0))
    one = EN.philox4x32_10((5, 7, 0, 0), (0, 0))
    assert " ".join("%08x" % int(c[0]) for c in w) == kat[0][2] and [int(c[1]) for c in w] == [int(c) for c in one]


def test_restated_normals_have_mean_0_and_variance_1():
    """10^6 restated normals (fp64): |mean| <= 5 / sqrt(N) and |var - 1| <= 5 sqrt(2 / N), the standard errors of the two estimates; |n| < 5.77."""
    n = EN.plane_noise(4, 289, 289, (0x1234ABCD, 0x0BADF00D))           # 4 * 289 * 289 * 3 = 1 002 252 values
    N = n.size
    assert N >= 10 ** 6
    mean, var = float(n.mean()), float(n.var())
    print("N = %d: mean %.3g (5 se = %.3g), var - 1 = %.3g (5 se = %.3g), max |n| = %.3f" % (N, mean, 5 / math.sqrt(N), var - 1, 5 * math.sqrt(2.0 / N), np.abs(n).max()))
    assert abs(mean) <= 5.0 / math.sqrt(N) and abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    assert np.abs(n).max() <= math.sqrt(48 * math.log(2)) < 5.77
    # the three channels are three different streams, and another key or plane gives other values
    assert abs(float(np.corrcoef(n[..., 0].ravel(), n[..., 2].ravel())[0, 1])) < 5.0 / math.sqrt(N / 3)
    assert not np.array_equal(n[0], n[1]) and not np.array_equal(n[:1], EN.plane_noise(1, 289, 289, (0x1234ABCD, 0x0BADF00E)))
    # the worst input of the logarithm: w0 = 0 -> u1 = 2^-24 -> r = sqrt(48 ln 2)
    worst = EN.normals((np.array([0]), np.array([0]), np.array([0xFFFFFFFF]), np.array([0])))
    assert worst[0, 0] == pytest.approx(math.sqrt(48 * math.log(2))) and worst[0, 1] == 0.0 and worst[0, 2] == pytest.approx(0.0, abs=1e-3)


# ------------------------------------------------------------------------------------------------ the tables
def _draws(seed=11, **kw):
    er = ER.RandomErasing(seed=seed, **kw)
    return er, [er.draw(BATCH, T, H, W) for _ in range(DRAWS)]


@pytest.mark.parametrize("cfg", [dict(), dict(probability=0.6, mode="rand", min_count=1, max_count=3), dict(probability=0.5, mode="const", cube=False, max_area=0.2, min_aspect=0.5, max_aspect=1.5)],
                         ids=["defaults", "rand_upto3", "const_per_frame"])
def test_table_statistics(cfg):
    er, draws = _draws(**cfg)
    mb = er.max_count
    mode_want = {"pixel": 2, "rand": 1, "const": 1}[er.mode]
    erased = decisions = 0
    keys, repeats_over_frames, differs_over_frames, counts = set(), 0, 0, set()
    for boxes, fill, key in draws:
        assert boxes.dtype == np.int32 and boxes.shape == (BATCH * T, mb, 5) and fill.dtype == np.float32 and fill.shape == (BATCH * T, mb, 4)
        assert key.dtype == np.uint32 and key.shape == (2,)
        ER.check_erase_table(boxes, fill, key, BATCH * T, H, W)
        keys.add(tuple(key.tolist()))
        bx, fl = boxes.reshape(BATCH, T, mb, 5), fill.reshape(BATCH, T, mb, 4)
        for i in range(BATCH):
            same = np.array_equal(bx[i, 0], bx[i, 1]) and np.array_equal(fl[i, 0], fl[i, 1])
            used0 = int((bx[i, 0, :, 4] != 0).sum())
            if er.cube:
                assert same
                decisions += 1
                erased += used0 > 0
            else:
                decisions += T
                erased += int(((bx[i, :, :, 4] != 0).sum(1) > 0).sum())
                differs_over_frames += (not same)
            repeats_over_frames += same and used0 > 0
        for p in range(BATCH * T):
            used = boxes[p, :, 4] != 0
            assert used[:int(used.sum())].all()                       # slots are filled from the front
            counts.add(int(used.sum()))
            assert (fill[p, ~used] == 0).all() and (boxes[p, ~used] == 0).all() and (fill[p, :, 3] == 0).all()
            for y0, x0, y1, x1, mode in boxes[p, used]:
                bh, bw = int(y1 - y0), int(x1 - x0)
                assert mode == mode_want and 0 <= y0 and y1 <= H and 0 <= x0 and x1 <= W and 0 < bh < H and 0 < bw < W
                # bh = round(sqrt(area * aspect)), bw = round(sqrt(area / aspect)): each side within 1/2 of its real value, so
                #   (bh - .5)(bw - .5) <= area <= (bh + .5)(bw + .5)  and  (bh - .5) / (bw + .5) <= aspect <= (bh + .5) / (bw - .5)
                a_lo, a_hi = er.min_area * H * W / er.max_count, er.max_area * H * W / er.min_count
                assert (bh - .5) * (bw - .5) <= a_hi * (1 + 1e-9) and (bh + .5) * (bw + .5) >= a_lo * (1 - 1e-9), (bh, bw)
                assert (bh - .5) / (bw + .5) <= er.max_aspect * (1 + 1e-9) and (bh + .5) / (bw - .5) >= er.min_aspect * (1 - 1e-9), (bh, bw)
            if er.mode == "const":
                assert (fill[p] == 0).all()
            if er.mode == "rand" and used.any():
                assert (fill[p, used, :3] != 0).all() and len(set(fill[p, used, 0].tolist())) == int(used.sum())          # one colour per box
    frac, sd = erased / decisions, math.sqrt(er.probability * (1 - er.probability) / decisions)
    print("erased %d of %d decisions: %.4f (probability %.2f, 4 sd = %.4f); box counts seen %s" % (erased, decisions, frac, er.probability, 4 * sd, sorted(counts)))
    assert abs(frac - er.probability) <= 4 * sd
    assert len(keys) == DRAWS                                        # a fresh key every step
    assert counts == set(range(0, mb + 1))
    if er.cube:
        assert repeats_over_frames > 0 and differs_over_frames == 0
    else:
        assert differs_over_frames > 0
    # the same seed gives the same tables, another seed other tables
    _, again = _draws(**cfg)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(draws[:20], again[:20]))
    _, other = _draws(seed=12, **cfg)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(draws[:20], other[:20]))


def test_a_box_that_cannot_fit_is_not_drawn():
    """bw < w and bh < h or no box: on a 2 x 2 image with area 1/3 .. 1 every attempt of aspect 1 gives a side of 1 or 2; only 1 x 1 boxes are accepted."""
    er = ER.RandomErasing(probability=1.0, mode="const", min_area=1.0 / 3, max_area=1.0, min_aspect=1.0, max_aspect=1.0, seed=1)
    sides = set()
    for _ in range(50):
        boxes, _, _ = er.draw(4, 1, 2, 2)
        for y0, x0, y1, x1, mode in boxes[:, 0]:
            if mode:
                sides.add((int(y1 - y0), int(x1 - x0)))
    assert sides == {(1, 1)}


def _table(planes=3, h=8, w=10):
    boxes = np.zeros((planes, 2, 5), dtype=np.int32)
    boxes[0, 0], boxes[1, 0], boxes[1, 1] = (0, 0, 4, 5, 1), (2, 3, 8, 10, 2), (0, 0, 0, 0, 1)
    fill = np.zeros((planes, 2, 4), dtype=np.float32)
    fill[0, 0, :3] = (0.5, -1.0, 2.0)
    return boxes, fill, np.array([7, 9], dtype=np.uint32)


def test_check_erase_table_rejects_each_single_violation():
    planes, h, w = 3, 8, 10
    boxes, fill, key = _table()
    ER.check_erase_table(boxes, fill, key, planes, h, w)
    for idx, v in [((0, 0, 0), -1), ((0, 0, 0), 5), ((0, 0, 2), 9), ((1, 0, 1), -1), ((1, 0, 1), 11), ((1, 0, 3), 11), ((1, 0, 3), 2), ((2, 1, 0), 1),
                   ((0, 0, 4), 3), ((2, 1, 4), -1)]:
        b = boxes.copy()
        b[idx] = v
        with pytest.raises(ValueError):
            ER.check_erase_table(b, fill, key, planes, h, w)
    for v in (float("nan"), float("inf"), -float("inf")):
        f = fill.copy()
        f[2, 1, 3] = v                                              # also in the ignored word and in an unused slot: the table is refused, not interpreted
        with pytest.raises(ValueError):
            ER.check_erase_table(boxes, f, key, planes, h, w)
    wide = np.zeros((planes, 9, 5), dtype=np.int32)
    for b, f, k in [(boxes.astype(np.int64), fill, key), (boxes, fill.astype(np.float64), key), (boxes, fill, key.astype(np.int32)), (boxes, fill, key.astype(np.int64)),
                    (boxes[:2], fill, key), (boxes, fill[:2], key), (boxes[:, :, :4], fill, key), (boxes, fill[:, :, :3], key), (boxes, fill[:, :1], key),
                    (boxes.reshape(6, 5), fill, key), (boxes, fill, key[:1]), (boxes, fill, np.zeros((1, 2), dtype=np.uint32)),
                    (wide, np.zeros((planes, 9, 4), dtype=np.float32), key), (boxes[:, :0], fill[:, :0], key)]:
        with pytest.raises(ValueError):
            ER.check_erase_table(b, f, k, planes, h, w)
    with pytest.raises(ValueError):
        ER.check_erase_table(boxes, fill, key, planes + 1, h, w)
    with pytest.raises(ValueError):
        ER.check_erase_table(boxes, fill, key, planes, h, w - 1)      # plane 1's x1 = 10 > 9
    with pytest.raises(ValueError):
        ER.check_erase_table(boxes, fill, key, planes, h - 1, w)


def test_build_erasing_by_type_name():
    e = ER.build_erasing(dict(type="RandomErasing", probability=0.5, mode="rand", max_count=2, seed=4))
    assert isinstance(e, ER.RandomErasing) and e.probability == 0.5 and e.mode == "rand" and (e.min_count, e.max_count, e.max_boxes) == (1, 2, 2)
    d = ER.build_erasing(dict(type="RandomErasing"))
    assert (d.probability, d.mode, d.min_area, d.max_area, d.min_aspect, d.max_count, d.cube) == (0.25, "pixel", 0.02, 1.0 / 3.0, 0.3, 1, True)
    assert d.max_aspect == pytest.approx(1 / 0.3)
    assert ER.build_erasing(None) is None and ER.build_erasing(e) is e
    with pytest.raises(NotImplementedError, match="GridMask"):
        ER.build_erasing(dict(type="GridMask"))
    for bad in (dict(probability=0.2), "RandomErasing", dict(type="RandomErasing", prob=0.2), dict(type="RandomErasing", probability=1.5),
                dict(type="RandomErasing", probability=-0.1), dict(type="RandomErasing", probability="0.2"), dict(type="RandomErasing", mode="noise"),
                dict(type="RandomErasing", max_count=9), dict(type="RandomErasing", min_count=0), dict(type="RandomErasing", min_count=3, max_count=2),
                dict(type="RandomErasing", min_area=0.5, max_area=0.2), dict(type="RandomErasing", min_area=0.0), dict(type="RandomErasing", min_aspect=0.0),
                dict(type="RandomErasing", min_aspect=2.0), dict(type="RandomErasing", min_aspect=0.5, max_aspect=0.4), dict(type="RandomErasing", max_count=2.5),
                dict(type="RandomErasing", max_area=float("nan"))):
        with pytest.raises(ValueError):
            ER.build_erasing(bad)
    ex = ER.ExplicitErasing(*_table())
    boxes, fill, key = ex.draw(3, 1, 8, 10)
    assert boxes.dtype == np.int32 and fill.dtype == np.float32 and key.dtype == np.uint32 and np.array_equal(boxes, _table()[0]) and ex.max_boxes == 2


def test_recognizer_reads_train_cfg_erasing():
    import mvfnet_amd

    def model(train_cfg=None):
        return mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, num_classes=10), train_cfg, dict(average_clips=None))
    m = model(dict(erasing=dict(type="RandomErasing", probability=0.25, mode="pixel", seed=1), blending=dict(type="MixupBlending", alpha=0.2)))
    assert isinstance(m.erasing, ER.RandomErasing) and m.erasing.mode == "pixel" and m.blending is not None
    assert model().erasing is None and model(dict()).erasing is None and model(dict(blending=dict(type="MixupBlending"))).erasing is None

    class _Eng(object):
        blending = erasing = label_smooth_eps = "unset"
    eng = _Eng()
    m._set_soft_options(eng, True)
    assert eng.erasing is m.erasing and eng.blending is m.blending
    m._set_soft_options(eng, False)                                # eval mode: it does not reach the engine
    assert eng.erasing is None
    m._train_engine = eng                                          # an engine driven through train_step follows the model's mode
    assert m.train() is m and eng.erasing is m.erasing
    m.eval()
    assert eng.erasing is None
    m.train()
    assert eng.erasing is m.erasing
    del m._train_engine
    with pytest.raises(NotImplementedError):
        model(dict(erasing=dict(type="NoSuchErasing")))
    with pytest.raises(ValueError):
        model(dict(erasing=dict(type="RandomErasing", max_count=9)))


def test_engine_surface():
    from mvfnet_amd.train_engine import TrainEngine
    # instance state named in the plan key, not a public scalar class attribute (those are plan-key switches of their own)
    assert "erasing" not in vars(TrainEngine)


# ------------------------------------------------------------------------------------------------ the export
def test_the_export_is_declared_and_bound():
    from mvfnet_amd import _lib
    vp, i32 = C.c_void_p, C.c_int
    assert "mvf_stem_erase" in _lib.declared_symbols()
    fn = _lib.lib.mvf_stem_erase
    assert fn.restype is C.c_int and list(fn.argtypes) == [vp, i32, i32, i32, i32, vp, i32, vp, vp, i32, vp]
    # a launch plan passes at most 40 integer-class and 4 float words per call (csrc/launch_plan.hip): every argument is an integer or a pointer
    assert C.c_float not in fn.argtypes and len(fn.argtypes) <= 40
    assert _lib.lib.mvf_abi_version() == 2
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvfnet_hip.h")).read()
    assert "Philox4x32-10" in hdr and "(x, y, p, 0)" in hdr and "#define MVF_ABI_VERSION 2" in hdr


def test_bad_arguments_are_refused_before_any_launch():
    """Host addresses that are never read: every call below must return from its argument checks."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    EINVAL, ESHAPE = -1, -2
    host = (C.c_char * 4096)()
    a = C.addressof(host)
    a += (-a) % 16
    bx, fl, ky = a + 1024, a + 2048, a + 3072

    def call(xp=a, planes=1, hp=4, wp=4, pad=1, boxes=bx, max_boxes=1, fill=fl, key=ky, dtype=0):
        return lib.mvf_stem_erase(xp, planes, hp, wp, pad, boxes, max_boxes, fill, key, dtype, None)
    for kw in (dict(xp=None), dict(boxes=None), dict(fill=None), dict(key=None)):
        assert call(**kw) == EINVAL and b"NULL" in lib.mvf_last_error(), kw
    for dtype in (2, 7, -1):
        assert call(dtype=dtype) == EINVAL and b"dtype" in lib.mvf_last_error()
    for mb in (0, 9, -1):
        assert call(max_boxes=mb) == EINVAL and b"max_boxes" in lib.mvf_last_error()
    assert call(hp=4, pad=3) == EINVAL and call(hp=8, wp=5, pad=3) == EINVAL                        # 2 * pad > hp, 2 * pad > wp
    for kw in (dict(planes=0), dict(planes=-2), dict(hp=0), dict(wp=-1), dict(pad=-1)):
        assert call(**kw) == EINVAL, kw
    assert call(hp=3, wp=3, dtype=1) == ESHAPE and b"16-byte units" in lib.mvf_last_error()         # 9 bf16 pixels
    assert call(xp=a + 8) == EINVAL and b"aligned" in lib.mvf_last_error()
    assert call(xp=a + 4, dtype=1) == EINVAL and b"aligned" in lib.mvf_last_error()
    for kw in (dict(boxes=bx + 2), dict(fill=fl + 1), dict(key=ky + 2)):
        assert call(**kw) == EINVAL and b"aligned" in lib.mvf_last_error(), kw
    assert call(hp=1 << 16, wp=1 << 16) == ESHAPE and b"too large" in lib.mvf_last_error()           # 2^32 pixels per plane: beyond int
    assert call(hp=1 << 16, wp=1 << 16, dtype=1) == ESHAPE
