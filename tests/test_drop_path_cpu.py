"""CPU: the drop-path schedule and draw (mvfnet_amd/droppath.py), its configuration, the fp64 restatement (tests/droppath_ref.py) against the oracle, and the
declarations and argument checks of the two exports of csrc/drop_path.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import droppath_ref as DR
from cases import BLOCK_CASES
from helpers import rel_err
from mvfnet_amd import droppath as DP
from mvfnet_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ schedule and draw
def test_the_linear_schedule():
    d = DP.DropPath(0.2)
    p = d.rates(16)
    assert p[0] == 0.0 and p[-1] == pytest.approx(0.2) and np.allclose(p, 0.2 * np.arange(16) / 15.0, rtol=0, atol=1e-15)
    assert d.drops(16) == (False,) + (True,) * 15
    assert DP.DropPath(0.05).rates(1).tolist() == [0.0] and DP.DropPath(0.05).drops(1) == (False,)
    assert DP.DropPath(0.0).drops(4) == (False,) * 4
    with pytest.raises(ValueError):
        d.rates(0)


CASES = [dict(unit="clip", scale_by_keep=True), dict(unit="frame", scale_by_keep=True), dict(unit="clip", scale_by_keep=False),
         dict(unit="frame", scale_by_keep=False)]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "%s_%s" % (kw["unit"], "scaled" if kw["scale_by_keep"] else "plain"))
def test_the_draw(kw):
    L, b, t, rate = 5, 6, 4, 0.4
    d = DP.DropPath(rate, seed=11, **kw)
    p = d.rates(L)
    tabs = [d.draw(L, b, t) for _ in range(40)]
    for s in tabs:
        assert s.shape == (L, b * t) and s.dtype == np.float32 and s.flags["C_CONTIGUOUS"]
        DP.check_drop_table(s, L, b * t)
        assert (s[0] == 1.0).all()                                  # block 0 never drops
        for i in range(L):
            keep = np.float32(1.0 / (1.0 - p[i])) if kw["scale_by_keep"] else np.float32(1.0)
            assert set(np.unique(s[i]).tolist()) <= {0.0, float(keep)}, (i, np.unique(s[i]))
    allt = np.stack(tabs).reshape(40, L, b, t)
    if kw["unit"] == "clip":
        assert (allt == allt[..., :1]).all()                        # the T frames of a clip share the draw
    else:
        assert (allt != allt[..., :1]).any()                        # per frame they do not
    again = DP.DropPath(rate, seed=11, **kw)
    assert all(np.array_equal(a, again.draw(L, b, t)) for a in tabs)            # the same seed: the same tables
    assert not np.array_equal(DP.DropPath(rate, seed=12, **kw).draw(L, b, t), tabs[0])


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "%s_%s" % (kw["unit"], "scaled" if kw["scale_by_keep"] else "plain"))
def test_the_keep_share_over_20000_draws(kw):
    L, b, t = 4, 500, 2
    d = DP.DropPath(0.3, seed=5, **kw)
    p = d.rates(L)
    per = b if kw["unit"] == "clip" else b * t
    steps = 20000 // per
    n = steps * per
    kept = np.zeros(L)
    for _ in range(steps):
        s = d.draw(L, b, t)
        units = s[:, ::t] if kw["unit"] == "clip" else s
        kept += (units > 0).sum(axis=1)
    for i in range(L):
        sigma = np.sqrt(p[i] * (1.0 - p[i]) / n)
        assert abs(kept[i] / n - (1.0 - p[i])) <= 4.0 * sigma, (i, kept[i] / n, 1.0 - p[i], sigma)


def test_the_refusals():
    for bad in (dict(type="DropPath", rate=1.0), dict(type="DropPath", rate=-0.1), dict(type="DropPath", rate=float("nan")), dict(type="DropPath", rate=True),
                dict(type="DropPath", rate="0.1"), dict(type="DropPath", rate=0.1, unit="video"), dict(type="DropPath", rate=0.1, mode="row"),
                dict(type="DropPath"), dict(type="DropBlock", rate=0.1), dict(rate=0.1), "DropPath"):
        with pytest.raises(ValueError):
            DP.build_drop_path(bad)
    d = DP.build_drop_path(dict(type="DropPath", rate=0.05))
    assert isinstance(d, DP.DropPath) and d.rate == 0.05 and d.unit == "clip" and d.scale_by_keep is True
    d = DP.build_drop_path(dict(type="DropPath", rate=0.1, unit="frame", scale_by_keep=False, seed=3))
    assert (d.unit, d.scale_by_keep, d.seed) == ("frame", False, 3)
    assert DP.build_drop_path(None) is None and DP.build_drop_path(d) is d
    ok = np.ones((3, 8), dtype=np.float32)
    assert DP.check_drop_table(ok, 3, 8) is not None
    for bad in (ok.astype(np.float64), ok[:2], ok[:, :7], ok.reshape(-1)):
        with pytest.raises(ValueError):
            DP.check_drop_table(bad, 3, 8)
    for v in (-0.5, float("nan"), float("inf")):
        t = ok.copy()
        t[1, 3] = v
        with pytest.raises(ValueError):
            DP.check_drop_table(t, 3, 8)
    e = DP.ExplicitDropPath(ok * 2)
    with pytest.raises(ValueError, match="row 0"):
        e.draw(3, 2, 4)
    e.table = ok
    assert np.array_equal(e.draw(3, 2, 4), ok) and e.drops(3) == (False, True, True)


def test_recognizer_reads_train_cfg_drop_path():
    import mvfnet_amd

    def model(train_cfg=None):
        return mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, num_classes=10), train_cfg, dict(average_clips=None))
    m = model(dict(drop_path=dict(type="DropPath", rate=0.05)))
    assert isinstance(m.drop_path, DP.DropPath) and m.drop_path.rate == 0.05 and m.blending is None
    assert model().drop_path is None

    class _Eng(object):
        blending = erasing = randaug = distill = drop_path = label_smooth_eps = "unset"
    eng = _Eng()
    m._set_soft_options(eng, True)
    assert eng.drop_path is m.drop_path
    m._set_soft_options(eng, False)                                 # eval mode: it does not reach the engine
    assert eng.drop_path is None
    m._train_engine = eng
    assert m.train() is m and eng.drop_path is m.drop_path
    m.eval()
    assert eng.drop_path is None
    del m._train_engine
    with pytest.raises(ValueError):
        model(dict(drop_path=dict(type="DropPath", rate=1.5)))
    from mvfnet_amd.train_engine import TrainEngine
    assert TrainEngine.drop_path is None                            # the class default: None is no plan-key switch


# ------------------------------------------------------------------------------------------------ the restatement against the oracle
def _block_sd(name, Cin, planes, stride):
    from test_oracle_golden import _block_sd as sd32
    return {k: (v.detach().double().requires_grad_(v.requires_grad) if v.dtype == torch.float32 else v) for k, v in sd32(name, Cin, planes, stride).items()}


@pytest.mark.parametrize("name", sorted(BLOCK_CASES))
def test_the_restatement_with_unit_scale_is_the_oracles_bottleneck(name):
    """l3_like is a plain block, l3_first a downsample block (stride 2)."""
    from oracle import net_torch
    N, T, Cin, planes, H, W, stride = BLOCK_CASES[name]
    assert (name == "l3_first") == (stride != 1 or Cin != planes * 4)
    mvf = dict(mode="THW", share=False, use_hs=True)
    x0 = torch.from_numpy(synth.synth_tensor("block_x/" + name, (N * T, Cin, H, W))).double()
    res = []
    for fn, kw in ((net_torch.bottleneck, {}), (DR.bottleneck, dict(scale=torch.ones(N * T, dtype=torch.float64))), (DR.bottleneck, dict(scale=None))):
        sd = _block_sd(name, Cin, planes, stride)
        x = x0.clone().requires_grad_(True)
        nb = {}
        y = fn(x, sd, "", stride, T, mvf, True, nb, **kw)
        y.backward(torch.from_numpy(synth.synth_tensor("block_dy/" + name, tuple(y.shape))).double())
        res.append((y.detach().numpy(), x.grad.numpy(), {k: t.grad.numpy() for k, t in sd.items() if t.requires_grad}, {k: t.numpy() for k, t in nb.items()}))
    ref = res[0]
    for got in res[1:]:
        assert rel_err(got[0], ref[0]) < 1e-12 and rel_err(got[1], ref[1]) < 1e-12
        assert sorted(got[2]) == sorted(ref[2]) and sorted(got[3]) == sorted(ref[3])
        for k in ref[2]:
            assert rel_err(got[2][k], ref[2][k]) < 1e-12, k
        for k in ref[3]:
            assert rel_err(got[3][k], ref[3][k]) < 1e-12, k


def test_the_restatement_drops_a_clip_of_a_plain_block():
    """s = 0 on clip 1: its output rows are relu(x), and the branch receives no gradient from them."""
    name = "l3_like"
    N, T, Cin, planes, H, W, stride = BLOCK_CASES[name]
    sd = _block_sd(name, Cin, planes, stride)
    x = torch.from_numpy(synth.synth_tensor("block_x/" + name, (N * T, Cin, H, W))).double().requires_grad_(True)
    s = torch.tensor([2.0] * T + [0.0] * T, dtype=torch.float64)
    y = DR.bottleneck(x, sd, "", stride, T, dict(mode="THW", share=False, use_hs=True), True, {}, scale=s)
    assert torch.equal(y[T:], torch.relu(x[T:]).detach())
    y1 = DR.bottleneck(x, sd, "", stride, T, dict(mode="THW", share=False, use_hs=True), True, {}, scale=None)
    assert not torch.equal(y[:T], y1[:T])


def test_the_kernel_restatements():
    rng = np.random.default_rng(3)
    m, c, rpi = 6, 8, 3
    z, r, g = rng.standard_normal((m, c)), rng.standard_normal((m, c)), rng.standard_normal((m, c))
    sc, sh = rng.standard_normal(c), rng.standard_normal(c)
    from bn_pool_ref import bn_apply, bn_mask
    one = DR.apply_bits_rowscale(z, sc, sh, r, [1.0, 1.0], rpi, act=1)
    ref = bn_apply(z, sc, sh, r=r, act=1)
    assert np.array_equal(one["out"], ref["out"]) and np.array_equal(one["bits"], ref["bits"]) and np.array_equal(one["A"], ref["A"])
    o = DR.apply_bits_rowscale(z, sc, sh, r, [0.0, 2.5], rpi, rscale=sc, rshift=sh, act=1)
    assert np.array_equal(o["out"][:3], np.maximum(r[:3] * sc + sh, 0.0))
    assert np.allclose(o["out"][3:], np.maximum(2.5 * (z[3:] * sc + sh) + r[3:] * sc + sh, 0.0), rtol=0, atol=1e-14)
    gm, a = DR.gate_rowscale(g, ref["bits"], [1.0, 1.0], rpi)
    assert np.array_equal(gm, bn_mask(g, z, ref["bits"], 4)[0])
    gm, a = DR.gate_rowscale(g, ref["bits"], [0.0, 2.5], rpi)
    assert not gm[:3].any() and np.array_equal(gm[3:], np.where(ref["out"][3:] > 0, 2.5 * g[3:], 0.0)) and np.array_equal(a[3:], np.abs(2.5 * g[3:]))


# ------------------------------------------------------------------------------------------------ the exports
_CTYPES = {"const void*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "const unsigned char*": C.c_void_p, "unsigned char*": C.c_void_p,
           "int": C.c_int, "long": C.c_long}
_NAMES = {
    "mvf_bn_apply_bits_rowscale": ["z", "m", "c", "scale", "shift", "residual", "rscale", "rshift", "row_scale", "rows_per_image", "act", "out", "sign_bits", "dtype",
                                   "stream"],
    "mvf_gate_rowscale": ["g", "g_pitch", "sign_bits", "row_scale", "rows_per_image", "m", "c", "gm_out", "dtype", "stream"],
}


@pytest.mark.parametrize("fn_name", sorted(_NAMES))
def test_the_header_declaration_matches_the_bound_argtypes(fn_name):
    from mvfnet_amd import _lib
    assert fn_name in _lib.declared_symbols() and fn_name not in _lib.QUERIES
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mvfnet_hip.h")).read()
    m = re.search(r"\bint %s\(([^)]*)\);" % fn_name, hdr)
    assert m is not None
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1] for p in params] == _NAMES[fn_name]
    types = [_CTYPES[p[:p.rindex(" ")]] for p in params]
    fn = getattr(_lib.lib, fn_name)
    assert fn.restype is C.c_int and list(fn.argtypes) == types
    assert all(t in (C.c_void_p, C.c_int, C.c_long) for t in types)            # pointers and ints only: a launch plan can carry the call
    assert _lib.lib.mvf_abi_version() == 2 and "#define MVF_ABI_VERSION 2" in hdr and len(_lib.BN_ENTRIES) == 14
    for text in ("v   = s * u", "16 bytes, row_scale 4 bytes", "bit for bit"):
        assert text in hdr, text


def test_bad_arguments_are_refused_before_any_launch():
    """Host addresses that are never read: every call below must return from its argument checks."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    EINVAL = -1
    host = (C.c_char * 8192)()
    a = C.addressof(host)
    a += (-a) % 16
    z, r, out, bits, sc, sh, tab = a, a + 1024, a + 2048, a + 3072, a + 4096, a + 4608, a + 5120

    def apply(z=z, m=6, c=8, scale=sc, shift=sh, residual=r, rscale=None, rshift=None, row_scale=tab, rpi=3, act=1, out=out, bits=bits, dtype=1):
        return lib.mvf_bn_apply_bits_rowscale(z, m, c, scale, shift, residual, rscale, rshift, row_scale, rpi, act, out, bits, dtype, None)

    def gate(g=z, pitch=8, bits=bits, row_scale=tab, rpi=3, m=6, c=8, gm=out, dtype=1):
        return lib.mvf_gate_rowscale(g, pitch, bits, row_scale, rpi, m, c, gm, dtype, None)
    for kw in (dict(z=None), dict(scale=None), dict(shift=None), dict(residual=None), dict(row_scale=None), dict(out=None), dict(bits=None)):
        assert apply(**kw) == EINVAL and b"NULL" in lib.mvf_last_error(), kw
    for kw in (dict(g=None), dict(bits=None), dict(row_scale=None), dict(gm=None)):
        assert gate(**kw) == EINVAL and b"NULL" in lib.mvf_last_error(), kw
    for call in (apply, gate):
        for kw in (dict(rpi=0), dict(rpi=-3), dict(rpi=4), dict(m=7)):
            assert call(**kw) == EINVAL and b"rows_per_image" in lib.mvf_last_error(), (call.__name__, kw)
        for kw in (dict(c=6), dict(c=0), dict(m=0), dict(m=-6)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
        for dtype in (2, -1):
            assert call(dtype=dtype) == EINVAL and b"dtype" in lib.mvf_last_error()
        assert call(row_scale=tab + 2) == EINVAL and b"aligned" in lib.mvf_last_error()
    for act in (2, 3, -1):
        assert apply(act=act) == EINVAL and b"act" in lib.mvf_last_error()
    assert apply(rscale=sc) == EINVAL and apply(rshift=sh) == EINVAL
    for kw in (dict(z=z + 8), dict(residual=r + 4), dict(out=out + 2), dict(scale=sc + 4), dict(shift=sh + 8), dict(rscale=sc + 4, rshift=sh)):
        assert apply(**kw) == EINVAL and b"aligned" in lib.mvf_last_error(), kw
    for kw in (dict(g=z + 8), dict(gm=out + 4)):
        assert gate(**kw) == EINVAL and b"aligned" in lib.mvf_last_error(), kw
    for pitch in (4, 7, 10):
        assert gate(pitch=pitch) == EINVAL and b"g_pitch" in lib.mvf_last_error()
