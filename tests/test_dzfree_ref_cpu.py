"""CPU: proof of the fp64 reference tests/dzfree_ref.py against torch FLOAT64 autograd of relu(bn3(conv3(a2)) + identity) (Bottleneck.forward's tail, bn3 in
training mode, no rounding anywhere), bound 1e-10 relative -- and every condition on the inputs of tests/test_dzfree_kernels_gpu.py (tests/dzfree_cases.py)
that the GPU module relies on: the exactness of the four lattice families in fp32 (every intermediate an fp32 number, every sum below 2^24 units, the bf16
splits of A2 exact and their low terms in use), the conditioning of the offset family, the layout of the partial rows.  The GPU tests make no exclusions, so
there is no cap on them to check."""
import numpy as np
import pytest
import torch

import dzfree_cases as K
import dzfree_ref as R
from helpers import rel_err

pytestmark = pytest.mark.cpu
TOL = 1e-10
EPS, MOM = K.EPS, K.MOMENTUM


def _close(got, want, what):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    e = rel_err(np.asarray(got), want)
    assert e < TOL, "%s: rel_err %.3g" % (what, e)


def _autograd(m, c, k, seed, zero_row=None):
    """The tail of a bottleneck under torch float64 autograd; m = 1 writes BatchNorm2d's formulas out (torch refuses one value per channel in training mode:
    biased variance 0, the unbiased divisor stays 1)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((c, k)) * np.sqrt(2.0 / k)
    if zero_row is not None:
        w[zero_row] = 0.0
    d = dict(m=m, c=c, k=k, w=w, a2=np.maximum(rng.standard_normal((m, k)), 0.0) + 0.25, identity=rng.standard_normal((m, c)), g=rng.standard_normal((m, c)),
             gamma=(rng.random(c) + 0.5) * np.where(np.arange(c) % 3 == 1, -1.0, 1.0), beta=rng.standard_normal(c) * 0.3, rm=rng.standard_normal(c) * 0.1,
             rv=rng.random(c) + 0.5)
    conv3 = torch.nn.Conv2d(k, c, 1, bias=False).double()
    bn3 = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        conv3.weight.copy_(torch.tensor(w).view(c, k, 1, 1))
        bn3.weight.copy_(torch.tensor(d["gamma"]))
        bn3.bias.copy_(torch.tensor(d["beta"]))
        bn3.running_mean.copy_(torch.tensor(d["rm"]))
        bn3.running_var.copy_(torch.tensor(d["rv"]))
    a2 = torch.tensor(d["a2"]).view(m, k, 1, 1).requires_grad_(True)
    z3 = conv3(a2)
    if m == 1:
        mean, var = z3.mean(0, keepdim=True), z3.var(0, unbiased=False, keepdim=True)
        y = (z3 - mean) / torch.sqrt(var + EPS) * bn3.weight.view(1, c, 1, 1) + bn3.bias.view(1, c, 1, 1)
        d["rm_new"] = ((1 - MOM) * bn3.running_mean + MOM * mean.detach().view(c)).numpy()
        d["rv_new"] = ((1 - MOM) * bn3.running_var + MOM * var.detach().view(c)).numpy()
    else:
        y = bn3(z3)
        d["rm_new"], d["rv_new"] = bn3.running_mean.numpy().copy(), bn3.running_var.numpy().copy()
    out = torch.relu(y + torch.tensor(d["identity"]).view(m, c, 1, 1))
    out.backward(torch.tensor(d["g"]).view(m, c, 1, 1))
    d["gm"] = d["g"] * (out.detach().view(m, c).numpy() > 0)
    z = z3.detach().view(m, c).numpy()
    d["mean"], d["var"] = z.mean(axis=0), z.var(axis=0)
    d["invstd"] = 1.0 / np.sqrt(d["var"] + EPS)
    d["da2"], d["dw"] = a2.grad.view(m, k).numpy(), conv3.weight.grad.view(c, k).numpy()
    d["dgamma"], d["dbeta"] = bn3.weight.grad.numpy(), bn3.bias.grad.numpy()
    return d


CASES = [(37, 32, 8, None), (300, 24, 12, None), (1, 16, 8, None), (37, 20, 8, 3), (300, 8, 16, 5)]


@pytest.mark.parametrize("m,c,k,zero_row", CASES, ids=str)
def test_reference_equals_float64_autograd(m, c, k, zero_row):
    d = _autograd(m, c, k, 11 * m + c + k, zero_row)
    # sums: the partial rows cut from gm at arbitrary row boundaries, with and without a split
    for c_split, rows_lo, rows_hi in ((0, 0, min(m, 7)), (c, min(m, 5), 0), (c // 3, min(m, 6), min(m, 3)), (c - 1, 1, min(m, 9))):
        lo, hi = K.partial_rows(d["gm"], c, c_split, rows_lo, rows_hi, seed=c_split + rows_hi, f32=lambda x: x)
        assert (lo is None) == (c_split == 0) and (hi is None) == (c_split == c)
        s = R.sums(d["gm"].T @ d["a2"], d["w"], d["mean"], d["invstd"], lo, rows_lo, c_split, hi, rows_hi)
        _close(s["dbeta"], d["dbeta"], "dbeta")
        _close(s["dgamma"], d["dgamma"], "dgamma")
    # prep: the data gradient as one product over the concatenated operand
    p = R.prep(d["w"].T, d["gamma"], d["mean"], d["invstd"], d["dgamma"], d["dbeta"], m)
    da2 = np.concatenate([d["gm"], d["a2"]], axis=1) @ p["bd"].T + p["bias"]
    if m == 1:
        # one row: dz3 = a (gm - dbeta - 0) = 0 identically; on the scale of the terms that cancel
        assert np.abs(d["da2"]).max() == 0.0 and np.abs(da2).max() <= 1e-12 * np.abs(p["bd"]).max() * max(np.abs(d["gm"]).max(), 1.0)
    else:
        _close(da2, d["da2"], "da2")
    # wgrad_fix
    f = R.wgrad_fix(d["gm"].T @ d["a2"], d["w"], d["a2"].T @ d["a2"], d["a2"].mean(axis=0), d["gamma"], d["mean"], d["invstd"], d["dgamma"], d["dbeta"], m)
    if m == 1:
        assert np.abs(d["dw"]).max() == 0.0 and np.abs(f["dw"]).max() <= 1e-12 * f["A"].max()
    else:
        _close(f["dw"], d["dw"], "dW")
    assert (f["A"] >= np.abs(f["dw"]) * (1 - 1e-12)).all()
    # gram_stats
    for rm, rv in ((d["rm"], d["rv"]), (None, None), (d["rm"], None), (None, d["rv"])):
        st = R.gram_stats(d["a2"].T @ d["a2"], d["a2"].mean(axis=0), d["w"], m, d["gamma"], d["beta"], EPS, MOM, rm, rv)
        _close(st["mean"], d["mean"], "mean")
        assert np.abs(st["var"] - d["var"]).max() <= TOL * st["A_var"].max()
        if m > 1:
            _close(st["invstd"], d["invstd"], "invstd")
            _close(st["scale"], d["gamma"] * d["invstd"], "scale")
            _close(st["shift"], d["beta"] - d["mean"] * d["gamma"] * d["invstd"], "shift")
        assert ("running_mean" in st) == (rm is not None) and ("running_var" in st) == (rv is not None)
        if rm is not None:
            _close(st["running_mean"], d["rm_new"], "running_mean")
        if rv is not None:
            _close(st["running_var"], d["rv_new"], "running_var")
    if zero_row is not None:
        st = R.gram_stats(d["a2"].T @ d["a2"], d["a2"].mean(axis=0), d["w"], m, d["gamma"], d["beta"], EPS, MOM)
        assert st["mean"][zero_row] == 0.0 and st["var"][zero_row] == 0.0 and st["A_var"][zero_row] == 0.0 and st["invstd"][zero_row] == 1.0 / np.sqrt(EPS)
        assert not p["bd"][:, zero_row].any()
    if m == 1:
        st = R.gram_stats(d["a2"].T @ d["a2"], d["a2"].mean(axis=0), d["w"], m, d["gamma"], d["beta"], EPS, 1.0, d["rm"], d["rv"])
        assert np.abs(st["var"]).max() <= 1e-13 * st["A_var"].max() and np.abs(st["running_var"]).max() <= 1e-13 * st["A_var"].max()


# ---------------------------------------------------------------------------------------------------------------- conditions on the GPU module's inputs
def _fp32(x, what):
    assert np.array_equal(np.asarray(x, dtype=np.float32).astype(np.float64), x), "%s is not exact in fp32" % what


def _units(abs_sum, q, what):
    """Every term a multiple of 2^-q and the sum of the absolute values below 2^24 of them: the sum is exact in fp32 in ANY order, fused or not."""
    u = np.asarray(abs_sum) * 2.0 ** q
    assert np.array_equal(u, np.round(u)) and u.max() < 2.0 ** 24, "%s: not a sum of < 2^24 units of 2^-%d (max %.3g)" % (what, q, u.max())


def _split_exact(x, terms):
    """The kernel's hi (/ mid) / lo bf16 split represents x exactly; returns the terms."""
    out, r = [], np.asarray(x, dtype=np.float64)
    for _ in range(terms):
        t = R.round_bf16(r)
        out.append(t)
        r = r - t
    assert not r.any(), "the %d-term bf16 split loses bits" % terms
    return out


def test_lattice_prep_is_exact_in_fp32():
    o = K.lattice_prep()
    assert (o["c"], o["k"]) == (768, 96) and o["c"] // 4 // 64 == 3                     # three trips per wave: the steady state of the register prefetch
    a, d0, kx = R.coefficients(o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"])
    e, t = a * kx, a * (d0 - kx * o["mean"])
    for x, what in ((1.0 / o["m"], "1 / m"), (a, "a"), (d0, "d0"), (o["invstd"] * o["dgamma"], "invstd dgamma"), (kx, "kx"), (kx * o["mean"], "kx mean"), (e, "e"), (t, "t")):
        _fp32(x, what)
    for v in (a, e):
        assert len(np.unique(v)) > 4                                                  # they vary per channel: a wrong channel index shows
    ew = e[:, None] * o["w"]
    assert np.array_equal(R.round_bf16(ew), ew) and np.array_equal(R.round_bf16(a[:, None] * o["w"]), a[:, None] * o["w"])     # the scaled operands are bf16 numbers
    p = R.prep(o["wd"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"])
    assert np.array_equal(np.round(ew * 64), ew * 64) and np.array_equal(np.round(o["w"] * 2), o["w"] * 2)      # every term of G is a multiple of 2^-7
    _units(p["A_G"], 7, "G")
    _units(p["A_bias"], 8, "bias")
    _units(np.abs(t[:, None] * o["w"]), 8, "a term of the bias")
    for x, what in ((p["bias"], "bias"), (p["bd"][:, o["c"]:], "G")):
        _fp32(x, what)
    # G is symmetric and its blocks differ: a block stored at the transposed or a shifted place shows
    g = p["bd"][:, o["c"]:]
    assert np.array_equal(g, g.T) and len({g[i:i + 32, j:j + 32].tobytes() for i in range(0, 96, 32) for j in range(0, 96, 32)}) == 9
    assert (R.round_bf16(g) != g).mean() > 0.5                                         # ... and most entries are rounded on output (from an exact sum: one result)


def test_lattice_wgrad_is_exact_in_fp32():
    o = K.lattice_wgrad()
    assert (o["c"], o["k"]) == (64, 192)                                                # three trips of 64 contraction indices
    a, d0, kx = (v[:, None] for v in R.coefficients(o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"]))
    assert np.array_equal(o["gram"], o["gram"].T)
    hi, lo = _split_exact(o["gram"], 2)
    assert (lo != 0).mean() > 0.25                                                      # the `lo` matrix instruction carries weight
    f = R.wgrad_fix(o["q"], o["w"], o["gram"], o["a_mean"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"])
    _units(np.abs(o["w"]) @ np.abs(hi) + np.abs(o["w"]) @ np.abs(lo), 1, "W A2 over both terms")
    sa, mu = o["m"] * o["a_mean"][None, :], o["mean"][:, None]
    wa = o["w"] @ o["gram"]
    inner = o["q"] - d0 * sa - kx * (wa - mu * sa)
    for x, what in ((wa, "W A2"), (mu * sa, "mean sa"), (wa - mu * sa, "W A2 - mean sa"), (kx * (wa - mu * sa), "kx (..)"), (d0 * sa, "d0 sa"), (o["q"] - d0 * sa, "Q - d0 sa"),
                    (inner, "the bracket"), (a * inner, "dW"), (f["dw"], "the reference's dW")):
        _fp32(x, what)
    _units(f["A"] / np.abs(a), 4, "the bracket")
    assert np.array_equal(f["dw"], a * inner)


def test_lattice_sums_is_exact_in_fp32():
    o = K.lattice_sums()
    assert o["c_split"] % 4 and o["rows_lo"] < 64 <= o["rows_hi"]
    s = R.sums(o["q"], o["w"], o["mean"], o["invstd"], o["part_lo"], o["rows_lo"], o["c_split"], o["part_hi"], o["rows_hi"])
    _units(np.abs(o["w"] * o["q"]).sum(axis=1), 1, "W . Q")
    _units(s["A_dbeta"], 0, "dbeta")
    _units(s["A_dgamma"] / o["invstd"], 3, "dot - mean dbeta")
    for x, what in ((s["dbeta"], "dbeta"), (o["mean"] * s["dbeta"], "mean dbeta"), (s["dgamma"], "dgamma")):
        _fp32(x, what)
    assert np.isnan(o["part_lo"][:, :, 1]).all() and np.isnan(o["part_hi"][:, :, 1]).all() and np.isnan(o["part_hi"][:o["c_split"]]).all()
    assert o["part_lo"].shape[0] == o["c_split"]


@pytest.mark.parametrize("m", K.LATTICE_GRAM_ROWS)
def test_lattice_gram_is_exact_in_fp32(m):
    o = K.lattice_gram(m)
    assert (o["c"], o["k"]) == (96, 32) and o["momentum"] == 0.5                         # three waves of a four-wave workgroup; 1 / m and the momentum dyadic
    assert (m <= K.GRAM_F64_MAX_ROWS) == (m == 2) and 2.0 ** round(np.log2(m)) == m       # one case on each side of the library's few-rows switch
    gc = o["gram"] / o["m"] - np.outer(o["a_mean"], o["a_mean"])
    for x, what in ((o["gram"], "A2"), (o["gram"] / o["m"], "A2 / m"), (np.outer(o["a_mean"], o["a_mean"]), "abar abar^T"), (gc, "Gc")):
        _fp32(x, what)
    hi, mid, lo = _split_exact(gc, 3)
    assert (mid != 0).sum() >= o["k"] and (lo != 0).sum() >= 4                         # both lower terms of the three-term split are in use
    assert (2 * np.abs(np.diag(gc)) > np.abs(gc).sum(axis=1)).all()                     # strictly diagonally dominant: positive definite
    aw = np.abs(o["w"])
    _units(((aw @ np.abs(gc)) * aw).sum(axis=1), 3, "W Gc W^T")
    _units(aw @ np.abs(o["a_mean"]), 1, "W abar")
    st = R.gram_stats(o["gram"], o["a_mean"], o["w"], o["m"], o["gamma"], o["beta"], K.EPS, o["momentum"], o["running_mean"], o["running_var"])
    for q in ("mean", "var", "running_mean"):
        _fp32(st[q], q)
    for x, what in ((o["momentum"] * o["running_var"], "running_var / 2"), (o["momentum"] * st["var"], "var / 2")):
        _fp32(x, what)
    rv = K.lattice_running_var(o, st["var"])
    if m == 2:
        _fp32(st["running_var"], "running_var")
        assert np.array_equal(rv, st["running_var"])                                    # m / (m - 1) = 2: the fp32 statement IS the exact value
    else:
        assert np.abs(rv - st["running_var"]).max() <= 2.0 ** -22 * np.abs(st["running_var"]).max()
    z = o["zero_row"]
    assert st["var"][z] == 0 and st["mean"][z] == 0 and (np.delete(st["var"], z) > 0).all()
    assert len(np.unique(st["var"])) > o["c"] // 2


# ---------------------------------------------------------------------------------------------------------------- the seeded families
def test_offset_family_is_ill_conditioned_and_the_zero_row_is_zero():
    for c, k in K.GRAM_SHAPES:
        o = K.triple(1568, c, k, "offset3")
        ratio = np.abs(o["a2"].mean(axis=0)) / o["a2"].std(axis=0)
        assert 4.0 < np.median(ratio) < 8.0, (c, k, np.median(ratio))
        z = K.triple(37, c, k, "zero_row")
        assert not z["w"][z["zero_row"]].any() and np.abs(z["w"]).sum(axis=1).astype(bool).sum() == c - 1


def test_operands_are_rounded_once_and_partial_rows_follow_the_header_layout():
    o = K.triple(K.SUMS_M, 64, 12)
    for q in ("w", "a2", "gm"):
        assert np.array_equal(R.round_bf16(o[q]), o[q])
    for q in ("mean", "invstd", "gamma", "dgamma", "dbeta", "gram", "a_mean", "q"):
        _fp32(o[q], q)
    assert np.array_equal(o["wd"], o["w"].T)
    for rows_lo, rows_hi in K.SUMS_ROWS:
        lo, hi = K.partial_rows(o["gm"], 64, 6, rows_lo, rows_hi, seed=1)
        assert lo.shape == (6, rows_lo, 2) and hi.shape == (64, rows_hi, 2)
        assert np.isnan(lo[:, :, 1]).all() and np.isnan(hi[:, :, 1]).all() and np.isnan(hi[:6]).all() and np.isfinite(hi[6:, :, 0]).all()
        s, _ = R.column_sums(lo, rows_lo, 6, hi, rows_hi, 64)
        assert np.abs(s - o["gm"].sum(axis=0)).max() < 1e-5
    assert K.partial_rows(o["gm"], 64, 0, 0, 3, seed=1)[0] is None and K.partial_rows(o["gm"], 64, 64, 3, 0, seed=1)[1] is None
    fz = K.frozen(o)
    p = R.prep(fz["wd"], fz["gamma"], fz["mean"], fz["invstd"], fz["dgamma"], fz["dbeta"], fz["m"])
    assert not p["bd"][:, 64:].any() and not p["bias"].any() and not p["A_G"].any()
    assert all(K.FLOOR <= K.bound(q) <= cap for q, cap in K.CAPS.items())
