"""CPU: batch blending (mvfnet_amd/blending.py) -- the tables Mixup / CutMix draw, their validator, the config plumbing through Recognizer2D and TSNClsHead --
and the four exports behind it (mvf_stem_blend, mvf_soft_targets, mvf_ce_loss_soft, mvf_head_train_fwd_soft): declared, bound, and refusing bad by-value
arguments before anything is launched (no GPU is needed to be refused)."""
import ctypes as C

import numpy as np
import pytest

from blend_numpy import soft_targets_ref
from mvfnet_amd import blending as BL

NEW = ("mvf_stem_blend", "mvf_soft_targets", "mvf_ce_loss_soft", "mvf_head_train_fwd_soft")
SHAPES = [(1, 7, 9), (5, 64, 48), (12, 224, 224)]
DRAWS = 200


def test_the_new_exports_are_declared_and_bound():
    from mvfnet_amd import _lib
    declared = _lib.declared_symbols()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    want = {"mvf_stem_blend": [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp],
            "mvf_soft_targets": [vp, vp, vp, i32, i32, f32, vp, vp],
            "mvf_ce_loss_soft": [vp, vp, i32, i32, vp, vp, vp, vp],
            "mvf_head_train_fwd_soft": [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]}
    for name in NEW:
        assert name in declared
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
        # a launch plan passes at most 40 integer-class and 4 float words per call (csrc/launch_plan.hip)
        assert sum(t is not f32 for t in fn.argtypes) <= 40 and sum(t is f32 for t in fn.argtypes) <= 4
    assert _lib.lib.mvf_abi_version() == 2


def test_bad_arguments_are_refused_before_any_launch():
    """Host addresses that are never read: every call below must return from its argument checks."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_char * 4096)()
    a = C.addressof(host)
    a += (-a) % 16
    assert lib.mvf_stem_blend(a, 1, 1, 4, 4, 1, a + 2048, a + 3072, a, 0, None) == -1 and b"overlap" in lib.mvf_last_error()          # out == xp
    assert lib.mvf_stem_blend(a, 1, 1, 4, 4, 1, a + 2048, a + 3072, a + 16, 1, None) == -1 and b"overlap" in lib.mvf_last_error()     # overlapping ranges
    for clips in (0, -3):
        assert lib.mvf_stem_blend(a, clips, 1, 4, 4, 1, a + 2048, a + 3072, a + 1024, 0, None) == -1
        assert lib.mvf_soft_targets(a, None, None, clips, 4, 0.0, a + 1024, None) == -1
        assert lib.mvf_ce_loss_soft(a, a + 512, clips, 4, None, a + 1024, a + 2048, None) == -1
        assert lib.mvf_head_train_fwd_soft(a, clips, 1, 1, 4, a, a, 4, a, None, a, a, a, a, a, 0, None) == -1
    for classes in (0, -1):
        assert lib.mvf_soft_targets(a, None, None, 2, classes, 0.0, a + 1024, None) == -1
        assert lib.mvf_ce_loss_soft(a, a + 512, 2, classes, None, a + 1024, a + 2048, None) == -1
        assert lib.mvf_head_train_fwd_soft(a, 2, 1, 1, 4, a, a, classes, a, None, a, a, a, a, a, 0, None) == -1
    for eps in (-0.1, 1.0, 1.5, float("nan")):
        assert lib.mvf_soft_targets(a, None, None, 2, 4, eps, a + 1024, None) == -1 and b"eps" in lib.mvf_last_error()
    assert lib.mvf_stem_blend(a, 1, 1, 3, 3, 1, a + 2048, a + 3072, a + 1024, 1, None) == -2      # 9 bf16 pixels: not a whole number of 16-byte units
    assert lib.mvf_stem_blend(a, 1, 1, 4, 4, 1, a + 2048, a + 3072, a + 1024, 7, None) == -1      # dtype
    assert lib.mvf_stem_blend(None, 1, 1, 4, 4, 1, a + 2048, a + 3072, a + 1024, 0, None) == -1
    assert lib.mvf_head_train_fwd_soft(a, 2, 1, 1, 1 << 20, a, a, 4, a, None, a, a, a, a, a, 0, None) == -5      # c beyond the LDS buffer: before the first launch


def _draws(cls, shape, seed=11, alpha=0.2):          # mmaction's default alpha
    bl = cls(alpha, seed=seed)
    return [bl.draw(*shape) for _ in range(DRAWS)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cls", [BL.MixupBlending, BL.CutmixBlending], ids=["mixup", "cutmix"])
def test_draw_properties(cls, shape):
    b, h, w = shape
    draws = _draws(cls, shape)
    again = _draws(cls, shape)
    empty = 0
    for (rows, wts), (rows2, wts2) in zip(draws, again):
        assert rows.dtype == np.int32 and rows.shape == (b, 5) and wts.dtype == np.float32 and wts.shape == (b, 2)
        assert np.array_equal(rows, rows2) and np.array_equal(wts, wts2)                 # the same seed gives the same tables
        BL.check_blend_rows(rows, wts, b, h, w)
        assert sorted(rows[:, 0].tolist()) == list(range(b))                              # one permutation per batch
        y0, x0, y1, x1 = (rows[:, k] for k in range(1, 5))
        assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= h).all() and (0 <= x0).all() and (x0 <= x1).all() and (x1 <= w).all()
        assert (rows[:, 1:] == rows[0, 1:]).all() and (wts == wts[0]).all()               # one lambda and one box per batch, as mmaction draws them
        area = (y1 - y0).astype(np.int64) * (x1 - x0)
        empty += int((area == 0).all())
        if cls is BL.MixupBlending:
            assert (area == 0).all() and np.array_equal(wts[:, 0], wts[:, 1]) and 0.0 <= wts[0, 0] <= 1.0
        else:
            assert (wts[:, 0] == 1.0).all()
            assert np.array_equal(wts[:, 1], (1.0 - area.astype(np.float64) / float(h * w)).astype(np.float32))
    assert empty > 0                                                                      # empty boxes occur (always for Mixup)
    # lambda is drawn per batch, not once (continuous for Mixup; CutMix's label weight takes the few values a small image's box areas allow)
    assert len(set(float(d[1][0, 1]) for d in draws)) > (DRAWS // 4 if cls is BL.MixupBlending else 3)
    other = _draws(cls, shape, seed=12)
    assert any(not np.array_equal(d[1], o[1]) for d, o in zip(draws, other))
    if b > 2:
        assert len(set(tuple(d[0][:, 0].tolist()) for d in draws)) > 1


def test_cutmix_box_follows_the_stated_recipe():
    """r = sqrt(1 - lambda), cw = int(w * r), ch = int(h * r), centre uniform in the image, clipped: re-derived from the same generator stream."""
    b, h, w = 5, 64, 48
    bl, rng = BL.CutmixBlending(0.7, seed=3), np.random.default_rng(3)
    for _ in range(50):
        rows, wts = bl.draw(b, h, w)
        lam = float(rng.beta(0.7, 0.7))
        perm = rng.permutation(b)
        r = np.sqrt(1.0 - lam)
        cw, ch = int(w * r), int(h * r)
        cx, cy = int(rng.integers(w)), int(rng.integers(h))
        box = (max(cy - ch // 2, 0), max(cx - cw // 2, 0), min(cy + ch // 2, h), min(cx + cw // 2, w))
        assert np.array_equal(rows[:, 0], perm) and (rows[:, 1:] == np.array(box)).all()


def _table(b=3, h=8, w=10):
    rows = np.array([[1, 0, 0, 4, 5], [2, 2, 3, 8, 10], [0, 0, 0, 0, 0]], dtype=np.int32)
    wts = np.array([[1.0, 0.75], [0.5, 0.5], [0.0, 1.0]], dtype=np.float32)
    return rows, wts


def test_check_blend_rows_rejects_each_single_violation():
    b, h, w = 3, 8, 10
    rows, wts = _table()
    BL.check_blend_rows(rows, wts, b, h, w)
    bad_rows = [(0, 0, -1), (0, 0, 3), (1, 1, -1), (1, 1, 9), (1, 3, 1), (1, 3, 9), (1, 2, -1), (1, 2, 11), (1, 4, 2), (1, 4, 11), (2, 1, 1), (2, 2, 1)]
    for i, k, v in bad_rows:
        r = rows.copy()
        r[i, k] = v
        with pytest.raises(ValueError):
            BL.check_blend_rows(r, wts, b, h, w)
    for i, k, v in [(0, 0, 1.5), (0, 0, -0.1), (1, 1, 1.0001), (2, 1, float("nan")), (2, 0, float("inf"))]:
        q = wts.copy()
        q[i, k] = v
        with pytest.raises(ValueError):
            BL.check_blend_rows(rows, q, b, h, w)
    for r, q in [(rows.astype(np.int64), wts), (rows, wts.astype(np.float64)), (rows[:2], wts), (rows, wts[:2]), (rows[:, :4], wts), (rows, wts[:, :1])]:
        with pytest.raises(ValueError):
            BL.check_blend_rows(r, q, b, h, w)
    with pytest.raises(ValueError):
        BL.check_blend_rows(rows, wts, b + 1, h, w)
    with pytest.raises(ValueError):
        BL.check_blend_rows(rows, wts, b, h, w - 1)              # row 1's x1 = 10 > 9


def test_build_blending_by_type_name():
    m = BL.build_blending(dict(type="MixupBlending", alpha=0.2, seed=4))
    c = BL.build_blending(dict(type="CutmixBlending", alpha=1.0))
    assert isinstance(m, BL.MixupBlending) and m.alpha == 0.2 and isinstance(c, BL.CutmixBlending) and c.alpha == 1.0
    assert BL.build_blending(None) is None and BL.build_blending(m) is m
    assert isinstance(BL.build_blending(dict(type="MixupBlending", num_classes=101)), BL.MixupBlending)      # mmaction's configs carry it
    with pytest.raises(NotImplementedError, match="ManifoldMixup"):
        BL.build_blending(dict(type="ManifoldMixup", alpha=0.2))
    for bad in (dict(alpha=0.2), dict(type="MixupBlending", alpha=0.0), dict(type="MixupBlending", alpha=-1), dict(type="CutmixBlending", alpha="0.2"),
                dict(type="MixupBlending", alpha=0.2, beta=1), "MixupBlending"):
        with pytest.raises(ValueError):
            BL.build_blending(bad)
    ex = BL.ExplicitBlending(*_table())
    rows, wts = ex.draw(3, 8, 10)
    assert rows.dtype == np.int32 and wts.dtype == np.float32 and np.array_equal(rows, _table()[0])


def _model(train_cfg=None, **head):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=10)
    cfg["cls_head"].update(head)
    return mvfnet_amd.build_recognizer(cfg, train_cfg, dict(average_clips=None))


def test_recognizer_reads_train_cfg_blending_and_the_heads_eps():
    m = _model(dict(blending=dict(type="CutmixBlending", alpha=0.3, seed=1)), label_smooth_eps=0.1)
    assert isinstance(m.blending, BL.CutmixBlending) and m.blending.alpha == 0.3
    assert m.cls_head.label_smooth_eps == 0.1
    plain = _model()
    assert plain.blending is None and plain.cls_head.label_smooth_eps == 0.0 and _model(dict()).blending is None

    class _Eng(object):
        blending, label_smooth_eps = "unset", "unset"
    eng = _Eng()
    m._set_soft_options(eng, True)
    assert eng.blending is m.blending and eng.label_smooth_eps == pytest.approx(0.1)
    m._set_soft_options(eng, False)                                # eval mode: neither reaches the engine
    assert eng.blending is None and eng.label_smooth_eps == 0.0
    m._train_engine = eng                                          # an engine driven through train_step follows the model's mode
    assert m.train() is m and eng.blending is m.blending and eng.label_smooth_eps == pytest.approx(0.1)
    m.eval()
    assert eng.blending is None and eng.label_smooth_eps == 0.0 and not m.training
    m.train()
    assert eng.blending is m.blending
    del m._train_engine
    with pytest.raises(NotImplementedError):
        _model(dict(blending=dict(type="NoSuchBlending")))
    with pytest.raises(ValueError):
        _model(dict(blending=dict(type="MixupBlending", alpha=0)))


@pytest.mark.parametrize("bad", [-0.1, 1.0, 2, "0.1", None, True])
def test_head_refuses_a_bad_label_smooth_eps(bad):
    from mvfnet_amd.heads.tsn_clshead import TSNClsHead
    with pytest.raises(ValueError, match="label_smooth_eps"):
        TSNClsHead(in_channels=8, num_classes=4, label_smooth_eps=bad)
    assert TSNClsHead(in_channels=8, num_classes=4, label_smooth_eps=0.2).label_smooth_eps == 0.2


def test_engine_surface():
    from mvfnet_amd.train_engine import TrainEngine
    # blending and eps are instance state named in the plan key, not public scalar class attributes (those are plan-key switches of their own)
    assert "blending" not in vars(TrainEngine) and "label_smooth_eps" not in vars(TrainEngine)


def test_numpy_scalars_are_numbers():
    from mvfnet_amd.heads.tsn_clshead import TSNClsHead
    assert BL.MixupBlending(np.float32(0.5)).alpha == 0.5 and BL.CutmixBlending(np.array(2)[()]).alpha == 2.0
    assert TSNClsHead(in_channels=8, num_classes=4, label_smooth_eps=np.float32(0.25)).label_smooth_eps == 0.25
    with pytest.raises(ValueError):
        BL.MixupBlending(np.bool_(True))


def test_numpy_restatement_of_the_targets():
    rows, wts = _table()
    labels = np.array([2, 2, 0])
    t = soft_targets_ref(labels, rows, wts, 4, 0.0, np.float32)
    assert t.dtype == np.float32 and t[0, 2] == np.float32(0.75) + np.float32(0.25) and t[1].tolist() == [0.5, 0, 0.5, 0] and t[2].tolist() == [1, 0, 0, 0]
    s = soft_targets_ref(labels, rows, wts, 4, 0.1)
    assert np.allclose(s.sum(1), 1.0) and np.allclose(s[2], [0.925, 0.025, 0.025, 0.025])
    assert np.array_equal(soft_targets_ref(labels, None, None, 4, 0.0), np.eye(4)[labels])
