"""CPU: RandAugment (mvfnet_amd/randaug.py) -- the numpy restatement of the kernel's arithmetic (randaug_numpy.py) against Pillow's recorded outputs
(tests/golden/randaug_cases.npz) and against Pillow itself where it is installed, bit for bit; the tables draw() makes, their validator, the config plumbing
through Recognizer2D; and the export behind it (mvf_frames_randaug_u8): declared, bound as declared, and refusing bad arguments before anything is launched."""
import ctypes as C
import importlib.util
import os
import random
import re

import numpy as np
import pytest

import randaug_numpy as RN
from mvfnet_amd import randaug as RA

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "randaug_cases.npz")


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_randaug_golden", os.path.join(HERE, "golden", "make_randaug_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _restated(rgb, name, arg, fill, order):
    """The restatement on an RGB image stored in `order`, returned as RGB."""
    h, w = rgb.shape[:2]
    src = np.ascontiguousarray(rgb if order == 1 else rgb[..., ::-1])
    got = RN.apply_row(src, RA.op_row(name, arg, h, w, fill, order), order)
    return got if order == 1 else got[..., ::-1]


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_the_restatement_equals_the_recorded_pillow_outputs_bit_for_bit():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    fill = tuple(int(v) for v in z["fill"])
    names = [str(n) for n in z["names"]]
    kinds = set()
    for k, (name, arg, i) in enumerate(zip(names, z["args"], z["image"])):
        img, want = z["img_%d" % i], z["out_%d" % k]
        kinds.add(int(RA.op_row(name, arg, img.shape[0], img.shape[1], fill)[0]))
        for order in (1, 0):
            got = _restated(img, name, float(arg), fill, order)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (k, name, float(arg), img.shape, order, int((got != want).sum()))
    assert kinds == set(range(12))                                  # every op kind
    # what the issue lists: blend factors on both sides of 1, thresh 0 and 256, bits 0, a constant channel, three rotations, two shears, two translations
    args = {n: sorted(float(a) for m, a in zip(names, z["args"]) if m == n) for n in set(names)}
    assert min(args["Brightness"]) < 1 < max(args["Brightness"]) and {0.0, 256.0} <= set(args["Solarize"]) and 0.0 in args["Posterize"]
    assert len(set(args["Rotate"])) >= 3 and names.count("ShearX") + names.count("ShearY") >= 2 and names.count("TranslateXRel") + names.count("TranslateYRel") >= 2
    assert (z["img_2"][..., 1] == z["img_2"][0, 0, 1]).all()


def test_equalize_on_the_37x53_image_needs_the_255_clamp():
    img = np.load(GOLDEN)["img_0"]
    assert img.shape == (37, 53, 3)
    for c in range(3):
        h = np.bincount(img[..., c].reshape(-1), minlength=256).astype(np.int64)
        nz = h[h > 0]
        step = int(nz.sum() - nz[-1]) // 255
        acc = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
        assert step > 0 and (acc // step).max() > 255 and RN.equalize_lut(img[..., c]).max() == 255


def test_the_restatement_equals_pillow_directly():
    pytest.importorskip("PIL")
    g = _golden_module()
    rng = np.random.RandomState(5)
    fill = (124, 116, 104)
    for h, w in ((37, 53), (64, 48), (5, 9), (3, 3), (1, 4)):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        img[: h // 2, :, 2] //= 3                                    # an uneven histogram
        cases = [("Invert", 0), ("AutoContrast", 0), ("Equalize", 0), ("Posterize", int(rng.randint(0, 9))), ("Solarize", int(rng.randint(0, 257))),
                 ("SolarizeAdd", int(rng.randint(0, 111))), ("Rotate", float(rng.uniform(-30, 30))), ("Rotate", 0.0), ("ShearX", float(rng.uniform(-.3, .3))),
                 ("ShearY", float(rng.uniform(-.3, .3))), ("TranslateXRel", float(rng.uniform(-.45, .45))), ("TranslateYRel", float(rng.uniform(-.45, .45)))]
        cases += [(n, float(f)) for n in ("Brightness", "Contrast", "Color", "Sharpness") for f in np.round(rng.uniform(0.1, 1.9, 3), 3)]
        for name, arg in cases:
            want = g.pil_op(img, name, arg, fill)
            for order in (1, 0):
                got = _restated(img, name, arg, fill, order)
                assert np.array_equal(got, want), (name, arg, (h, w), order, int((got != want).sum()))


def test_layers_run_in_order_on_each_frames_own_image_and_leave_the_padding():
    rng = np.random.RandomState(1)
    fr = rng.randint(0, 256, (4, 6, 8, 3)).astype(np.uint8)
    sizes = np.array([[6, 8], [6, 8], [4, 5], [4, 5]])
    table = np.stack([np.stack([RA.op_row("Invert", 0, 6, 8), RA.op_row("Solarize", 100, 6, 8)]),
                      np.stack([RA.op_row("AutoContrast", 0, 4, 5), RA.op_row("Identity", 0, 4, 5)])])
    out = RN.apply_layers(fr, table, 2, sizes)
    inv = 255 - fr[0].astype(int)
    assert np.array_equal(out[0], np.where(inv < 100, inv, 255 - inv))
    assert np.array_equal(out[2, :4, :5], RN.apply_row(fr[2, :4, :5], table[1, 0])) and not np.array_equal(out[2, :4, :5], fr[2, :4, :5])
    assert np.array_equal(out[2, 4:], fr[2, 4:]) and np.array_equal(out[2, :, 5:], fr[2, :, 5:])


# ------------------------------------------------------------------------------------------------ the draw
def test_the_config_string():
    assert RA.parse_config("rand-m7-n4-mstd0.5-inc1") == dict(magnitude=7, num_layers=4, magnitude_std=0.5, increasing=True)
    assert RA.parse_config("rand-m9-mstd101-mmax20-p0.3-inc0") == dict(magnitude=9, magnitude_std=101.0, magnitude_max=20, prob=0.3, increasing=False)
    a = RA.RandAugment("rand-m7-n4-mstd0.5-inc1")
    assert (a.num_layers, a.magnitude, a.magnitude_std, a.increasing, a.prob, a.magnitude_max) == (4, 7.0, 0.5, True, 0.5, 10.0)
    assert a.ops == RA.RAND_INCREASING_TRANSFORMS and len(a.ops) == 15 and len(RA.RAND_TRANSFORMS) == 15
    assert RA.RandAugment("rand-m5-n2").ops == RA.RAND_INCREASING_TRANSFORMS and RA.RandAugment("rand-m5-n2", increasing=False).ops == RA.RAND_TRANSFORMS
    for bad in ("augmix-m5", "rand-w0", "rand-q3", "rand-n9", "rand-n0"):
        with pytest.raises(ValueError):
            RA.RandAugment(bad)
    with pytest.raises(ValueError, match="bilinear"):
        RA.RandAugment(interpolation="bicubic")
    with pytest.raises(ValueError, match="Cutout.*built"):
        RA.RandAugment(ops=["Invert", "Cutout"])
    for kw in (dict(num_layers=0), dict(num_layers=9), dict(num_layers=2.5), dict(prob=1.5), dict(prob=-0.1), dict(magnitude="7"), dict(fill=(1, 2)),
               dict(fill=(0, 0, 256)), dict(ops=[]), dict(magnitude=float("nan"))):
        with pytest.raises(ValueError):
            RA.RandAugment(**kw)


def test_level_functions_at_magnitude_0_7_and_10(monkeypatch):
    inc, plain = RA.RandAugment(increasing=True), RA.RandAugment(increasing=False)
    for sign, draw in ((1.0, 0.0), (-1.0, 0.75)):                   # random.random() > 0.5 negates
        monkeypatch.setattr(random, "random", lambda: draw)
        for m, L in ((0, 0.0), (7, 0.7), (10, 1.0)):
            assert inc.level("Rotate", m) == sign * (L * 30.0)
            assert inc.level("ShearX", m) == sign * (L * 0.3) and inc.level("ShearY", m) == sign * (L * 0.3)
            assert inc.level("TranslateXRel", m) == sign * (L * 0.45) and inc.level("TranslateYRel", m) == sign * (L * 0.45)
            for n in ("Color", "Contrast", "Brightness", "Sharpness"):
                assert inc.level(n + "Increasing", m) == max(0.1, 1.0 + sign * (L * 0.9))
                assert plain.level(n, m) == L * 1.8 + 0.1
            assert inc.level("PosterizeIncreasing", m) == 4 - int(L * 4) and plain.level("Posterize", m) == int(L * 4)
            assert inc.level("SolarizeIncreasing", m) == 256 - min(256, int(L * 256)) and plain.level("Solarize", m) == min(256, int(L * 256))
            assert inc.level("SolarizeAdd", m) == min(110, int(L * 110))
            for n in ("AutoContrast", "Equalize", "Invert"):
                assert inc.level(n, m) is None
    monkeypatch.setattr(random, "random", lambda: 0.0)
    assert inc.level("PosterizeIncreasing", 10) == 0 and inc.level("SolarizeIncreasing", 10) == 0 and inc.level("SolarizeIncreasing", 0) == 256
    assert inc.level("BrightnessIncreasing", 0) == 1.0 and inc.level("SolarizeAdd", 20) == 110 and inc.level("PosterizeIncreasing", 7) == 2
    monkeypatch.setattr(random, "random", lambda: 0.75)
    assert inc.level("ColorIncreasing", 10) == pytest.approx(0.1) and inc.level("ColorIncreasing", 20) == 0.1       # the floor of the enhance factors


def test_op_rows():
    r = RA.op_row("PosterizeIncreasing", 0, 8, 8)
    assert r.dtype == np.int32 and r.shape == (16,) and (r[0], r[1]) == (RA.K_POSTERIZE, 0)                    # bits 0: a black frame
    assert RA.op_row("Posterize", 3, 8, 8)[1] == 0xE0 and RA.op_row("Posterize", 8, 8, 8)[0] == RA.K_IDENTITY
    assert tuple(RA.op_row("SolarizeAdd", 60, 8, 8)[:3]) == (RA.K_SOLARIZE_ADD, 128, 60) and RA.op_row("Solarize", 300, 8, 8)[1] == 256
    assert RA.op_row("ContrastIncreasing", 1.5, 8, 8)[1:2].view(np.float32)[0] == np.float32(1.5)
    co = lambda row: tuple(np.ascontiguousarray(row[1:13]).view(np.float64))   # noqa: E731
    assert co(RA.op_row("ShearX", 0.2, 8, 8)) == (1, 0.2, 0, 0, 1, 0) and co(RA.op_row("ShearY", -0.2, 8, 8)) == (1, 0, 0, -0.2, 1, 0)
    assert co(RA.op_row("TranslateXRel", 0.25, 10, 20)) == (1, 0, 5.0, 0, 1, 0) and co(RA.op_row("TranslateYRel", -0.5, 10, 20)) == (1, 0, 0, 0, 1, -5.0)
    assert co(RA.op_row("Rotate", 0.0, 10, 20)) == (1, 0, 0, 0, 1, 0) and co(RA.op_row("Rotate", 360.0, 10, 20)) == (1, 0, 0, 0, 1, 0)
    a, b, c, d, e, f = co(RA.op_row("Rotate", 90.0, 10, 20))
    assert (a, b, d, e) == (0.0, -1.0, 1.0, 0.0) and (c, f) == (15.0, -5.0)                                    # cos / sin rounded to 15 decimals
    assert RA.op_row("Rotate", 5, 8, 8, fill=(1, 2, 3), order=1)[13] == 0x030201 and RA.op_row("Rotate", 5, 8, 8, fill=(1, 2, 3), order=0)[13] == 0x010203
    assert (RA.op_row("Rotate", 5, 8, 8)[14:] == 0).all()
    with pytest.raises(ValueError, match="built"):
        RA.op_row("Cutout", 1, 8, 8)
    with pytest.raises(ValueError):
        RA.op_row("Invert", 0, 8, 8, order=2)


def test_draw_follows_the_stated_order_of_draws():
    aug = RA.RandAugment("rand-m7-n4-mstd0.5-inc1")
    batch, t, h, w = 6, 2, 40, 56
    np.random.seed(11)
    random.seed(12)
    table, mask = aug.draw(batch, t, (h, w), order=0)
    assert table.dtype == np.int32 and table.shape == (batch, 4, 16)
    RA.check_randaug_table(table, batch, 4)
    np.random.seed(11)
    random.seed(12)
    want = np.zeros_like(table)
    for i in range(batch):
        names = np.random.choice(aug.ops, 4)
        for k, name in enumerate(str(n) for n in names):
            if random.random() > 0.5:
                continue
            m = max(0.0, min(random.gauss(7, 0.5), 10.0))
            want[i, k] = RA.op_row(name, aug.level(name, m), h, w, aug.fill, 0)
    assert np.array_equal(table, want) and len(set(table[:, :, 0].reshape(-1).tolist())) > 4
    assert mask == RA.stats_mask(table) == sum(1 << k for k in range(4) if np.isin(table[:, k, 0], (5, 6, 8)).any())
    # uniform magnitudes, prob 1 (no skip draw), the plain list
    uni = RA.RandAugment("rand-m9-n2-mstd100-inc0-p1.0")
    np.random.seed(3)
    random.seed(4)
    tab2, _ = uni.draw(3, 1, (8, 8))
    np.random.seed(3)
    random.seed(4)
    for i in range(3):
        for k, name in enumerate(str(n) for n in np.random.choice(uni.ops, 2)):
            m = random.uniform(0, 9)
            assert np.array_equal(tab2[i, k], RA.op_row(name, uni.level(name, m), 8, 8, uni.fill, 0))
    assert (tab2[:, :, 0] != 0).any()


def test_the_statistics_mask_and_the_sizes():
    t = np.zeros((2, 3, 16), dtype=np.int32)
    assert RA.stats_mask(t) == 0
    t[0, 0, 0], t[1, 2, 0] = RA.K_EQUALIZE, RA.K_CONTRAST
    assert RA.stats_mask(t) == 0b101
    t[1, 1, 0] = RA.K_AUTOCONTRAST
    assert RA.stats_mask(t) == 0b111
    t[:, :, 0] = RA.K_COLOR
    assert RA.stats_mask(t) == 0
    ex = RA.ExplicitAugment(t)
    tab, mask = ex.draw(2, 4, (8, 8))
    assert tab.dtype == np.int32 and np.array_equal(tab, t) and mask == 0
    # per-frame sizes: Rotate / Translate use the clip's size; a clip whose frames differ is refused for them, not for the others
    rot = RA.RandAugment(num_layers=1, prob=1.0, ops=["Rotate"])
    sizes = np.array([[10, 20], [10, 20], [30, 16], [30, 16]])
    tab, _ = rot.draw(2, 2, sizes)
    co = np.ascontiguousarray(tab[:, 0, 1:13]).view(np.float64)
    for i, (h, w) in enumerate(((10, 20), (30, 16))):
        a, b, c = co[i, :3]
        assert a * (w / 2.0) + b * (h / 2.0) + c == pytest.approx(w / 2.0, abs=1e-9)                            # the centre maps to itself
    with pytest.raises(ValueError, match="differ in size"):
        rot.draw(2, 2, np.array([[10, 20], [10, 21], [30, 16], [30, 16]]))
    RA.RandAugment(num_layers=1, prob=1.0, ops=["ShearX", "Invert"]).draw(2, 2, np.array([[10, 20], [10, 21], [30, 16], [30, 16]]))


def test_check_randaug_table_rejects_each_single_violation():
    good = np.stack([np.stack([RA.op_row("Rotate", 10, 8, 8), RA.op_row("Posterize", 2, 8, 8)]), np.stack([RA.op_row("Color", 1.5, 8, 8), RA.op_row("SolarizeAdd", 9, 8, 8)])])
    RA.check_randaug_table(good, 2)
    RA.check_randaug_table(good, 2, 2)
    nan32, nan64 = np.array([np.nan], dtype=np.float32).view(np.int32)[0], np.array([np.nan]).view(np.int32)
    for idx, v in [((0, 0, 0), 12), ((0, 0, 0), -1), ((0, 0, 14), 1), ((1, 1, 15), 7), ((0, 1, 1), 256), ((0, 1, 1), -1), ((1, 1, 1), 257), ((1, 1, 2), 256),
                   ((1, 1, 2), -1), ((1, 0, 1), nan32), ((0, 0, 13), 1 << 24), ((0, 0, 13), -1)]:
        bad = good.copy()
        bad[idx] = v
        with pytest.raises(ValueError):
            RA.check_randaug_table(bad, 2)
    bad = good.copy()
    bad[0, 0, 5:7] = nan64
    with pytest.raises(ValueError, match="affine"):
        RA.check_randaug_table(bad, 2)
    for tab, batch, layers in [(good.astype(np.int64), 2, None), (good[:1], 2, None), (good[:, :, :15], 2, None), (good.reshape(4, 16), 4, None),
                               (good, 2, 3), (good[:, :0], 2, None), (np.zeros((2, 9, 16), dtype=np.int32), 2, None), (good, 3, None)]:
        with pytest.raises(ValueError):
            RA.check_randaug_table(tab, batch, layers)


def test_build_randaug_by_type_name():
    a = RA.build_randaug(dict(type="RandAugment", config="rand-m7-n4-mstd0.5-inc1"))
    assert isinstance(a, RA.RandAugment) and a.num_layers == 4 and a.fill == (124, 116, 104) and a.translate_pct == 0.45
    assert RA.build_randaug(None) is None and RA.build_randaug(a) is a
    with pytest.raises(NotImplementedError, match="AutoAugment"):
        RA.build_randaug(dict(type="AutoAugment"))
    for bad in (dict(config="rand-m7"), "RandAugment", dict(type="RandAugment", layers=2), dict(type="RandAugment", interpolation="bicubic"),
                dict(type="RandAugment", config="rand-z1"), dict(type="RandAugment", ops=["Blur"])):
        with pytest.raises(ValueError):
            RA.build_randaug(bad)


def test_recognizer_reads_train_cfg_randaug():
    import mvfnet_amd

    def model(train_cfg=None):
        return mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, num_classes=10), train_cfg, dict(average_clips=None))
    m = model(dict(randaug=dict(type="RandAugment", config="rand-m7-n4-mstd0.5-inc1")))
    assert isinstance(m.randaug, RA.RandAugment) and m.erasing is None and m.blending is None
    assert model().randaug is None and model(dict(erasing=dict(type="RandomErasing"))).randaug is None

    class _Eng(object):
        blending = erasing = randaug = label_smooth_eps = "unset"
    eng = _Eng()
    m._set_soft_options(eng, True)
    assert eng.randaug is m.randaug
    m._set_soft_options(eng, False)                                # eval mode: it does not reach the engine
    assert eng.randaug is None
    m._train_engine = eng
    assert m.train() is m and eng.randaug is m.randaug
    m.eval()
    assert eng.randaug is None
    del m._train_engine
    with pytest.raises(NotImplementedError):
        model(dict(randaug=dict(type="AugMix")))
    with pytest.raises(ValueError):
        model(dict(randaug=dict(type="RandAugment", interpolation="bicubic")))
    from mvfnet_amd.train_engine import TrainEngine
    assert "randaug" not in vars(TrainEngine)                      # instance state, not a plan-key switch


# ------------------------------------------------------------------------------------------------ the export
_CTYPES = {"const unsigned char*": C.c_void_p, "unsigned char*": C.c_void_p, "const int*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int,
           "unsigned": C.c_uint, "long long": C.c_longlong}


def test_the_header_declaration_matches_the_bound_argtypes():
    from mvfnet_amd import _lib
    assert "mvf_frames_randaug_u8" in _lib.declared_symbols()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mvfnet_hip.h")).read()
    m = re.search(r"\bint mvf_frames_randaug_u8\(([^)]*)\);", hdr)
    assert m is not None
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [p.split()[-1] for p in params]
    assert names == ["frames_hwc", "n", "hs", "ws", "t", "order", "sizes", "table", "layers", "stats_layers", "out", "tmp", "workspace", "workspace_bytes", "stream"]
    types = [_CTYPES[p[:p.rindex(" ")]] for p in params]
    fn = _lib.lib.mvf_frames_randaug_u8
    assert fn.restype is C.c_int and list(fn.argtypes) == types
    assert _lib.lib.mvf_abi_version() == 2 and "#define MVF_ABI_VERSION 2" in hdr
    assert "#define MVF_RANDAUG_WS_PER_FRAME (3 * 256 + 16)" in hdr and RA.WS_PER_FRAME == 3 * 256 + 16
    for text in ("(2 acc + 13) / 26", "19595", "measured there, not guaranteed", "bicubic"):
        assert text in hdr, text


def test_bad_arguments_are_refused_before_any_launch():
    """Host addresses that are never read: every call below must return from its argument checks."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    EINVAL, ESHAPE = -1, -2
    host = (C.c_char * 8192)()
    a = C.addressof(host)
    a += (-a) % 16
    fr, out, tmp, tab, sz, ws = a, a + 1024, a + 2048, a + 3072, a + 4096, a + 5120

    def call(frames=fr, n=2, hs=4, ws_=5, t=2, order=0, sizes=sz, table=tab, layers=2, stats=0, out=out, tmp=tmp, workspace=ws, wsb=2 * RA.WS_PER_FRAME):
        return lib.mvf_frames_randaug_u8(frames, n, hs, ws_, t, order, sizes, table, layers, stats, out, tmp, workspace, wsb, None)
    for kw in (dict(frames=None), dict(table=None), dict(out=None), dict(tmp=None), dict(workspace=None)):
        assert call(**kw) == EINVAL and b"NULL" in lib.mvf_last_error(), kw
    for kw in (dict(n=0), dict(n=-2), dict(hs=0), dict(ws_=-1), dict(t=0)):
        assert call(**kw) == EINVAL, kw
    assert call(n=3) == EINVAL and b"multiple" in lib.mvf_last_error()
    for order in (2, -1):
        assert call(order=order) == EINVAL and b"order" in lib.mvf_last_error()
    for layers in (0, 9, -1):
        assert call(layers=layers) == EINVAL and b"layers" in lib.mvf_last_error()
    assert call(stats=0b100) == EINVAL and b"stats_layers" in lib.mvf_last_error()
    assert call(layers=8, stats=0x100) == EINVAL
    for kw in (dict(out=tmp), dict(out=fr), dict(tmp=fr)):
        assert call(**kw) == EINVAL and b"three buffers" in lib.mvf_last_error(), kw
    for kw in (dict(frames=fr + 1), dict(out=out + 2), dict(tmp=tmp + 3), dict(table=tab + 2), dict(sizes=sz + 1), dict(workspace=ws + 2)):
        assert call(**kw) == EINVAL and b"aligned" in lib.mvf_last_error(), kw
    assert call(wsb=2 * RA.WS_PER_FRAME - 1) == EINVAL and b"workspace" in lib.mvf_last_error()
    assert call(wsb=0) == EINVAL and call(wsb=-5) == EINVAL
    assert call(hs=1 << 15, ws_=1 << 15) == ESHAPE and b"too large" in lib.mvf_last_error()
    assert call(n=1 << 22, t=1, hs=1024, ws_=1024, wsb=1 << 40) == ESHAPE and b"workgroups" in lib.mvf_last_error()
