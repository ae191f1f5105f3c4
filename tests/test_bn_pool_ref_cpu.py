"""CPU: proof of the fp64 reference tests/bn_pool_ref.py against torch in FLOAT64 (F.batch_norm forward, running statistics and autograd, for ReLU,
hard-swish, the residual and the sum of two BatchNorms; F.max_pool2d(F.relu(.), 3, 2, 1, return_indices=True) for y, the argmax byte and the gradient), bound
1e-12 relative -- and every condition on the inputs of tests/test_bn_pool_kernels_gpu.py (tests/bn_pool_cases.py) that the GPU module relies on: the share of
undecided elements of every case, the exactness of the lattice family, the conditioning of the statistics cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_pool_cases as K
import bn_pool_ref as R
from helpers import rel_err

pytestmark = pytest.mark.cpu
TOL = 1e-12
EPS, MOM = K.EPS, K.MOMENTUM


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def _close(got, want, what):
    e = rel_err(np.asarray(got), want.detach().numpy() if isinstance(want, torch.Tensor) else want)
    assert e < TOL, "%s: rel_err %.3g" % (what, e)


def _data(m, c, seed):
    rng = np.random.default_rng(seed)
    d = dict(z=rng.standard_normal((m, c)) * 2 + rng.standard_normal(c) * 3, zb=rng.standard_normal((m, c)) + rng.standard_normal(c),
             r=rng.standard_normal((m, c)), g=rng.standard_normal((m, c)), gamma=rng.random(c) + 0.5, beta=rng.standard_normal(c), gamma_b=-(rng.random(c) + 0.5),
             beta_b=rng.standard_normal(c), rm=rng.standard_normal(c) * 0.1, rv=rng.random(c) + 0.5)
    return d


@pytest.mark.parametrize("m,c", [(1, 4), (37, 12), (300, 8)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_batchnorm_forward_running_statistics_and_autograd(m, c, act):
    d = _data(m, c, 5 * m + c + act)
    z, gamma, beta = _t(d["z"], True), _t(d["gamma"], True), _t(d["beta"], True)
    rm, rv = _t(d["rm"]), _t(d["rv"])
    if m == 1:      # torch refuses one value per channel in training mode: the same formulas written out (biased var = 0, the unbiased divisor stays 1)
        mean, var = z.mean(0), z.var(0, unbiased=False)
        bn = (z - mean) / torch.sqrt(var + EPS) * gamma + beta
        rm, rv = (1 - MOM) * rm + MOM * mean.detach(), (1 - MOM) * rv + MOM * var.detach()
    else:
        bn = F.batch_norm(z, rm, rv, gamma, beta, True, MOM, EPS)
    y = bn if act == 0 else (F.relu(bn) if act == 1 else F.hardswish(bn))
    y.backward(_t(d["g"]))
    st = R.bn_stats(d["z"], d["gamma"], d["beta"], EPS, MOM, d["rm"], d["rv"])
    _close(st["mean"], _t(d["z"]).mean(0), "mean")
    _close(st["invstd"], 1 / torch.sqrt(_t(d["z"]).var(0, unbiased=False) + EPS), "invstd")
    _close(st["running_mean"], rm, "running_mean")
    _close(st["running_var"], rv, "running_var")
    ap = R.bn_apply(d["z"], st["scale"], st["shift"], act=act)
    _close(ap["out"], y, "out")
    _close(ap["colmeans"], y.mean(0), "column means")
    assert np.array_equal(R.unpack_bits(ap["bits"], c), y.detach().numpy() > 0)
    modes = {0: (0,), 1: (2, 1, 4), 2: (3,)}[act]
    for mode in modes:
        operand = ap["out"] if mode == 1 else (ap["bits"] if mode == 4 else None)
        bw = R.bn_bwd(d["g"], d["z"], operand, mode, d["gamma"], st["mean"], st["invstd"], st["scale"], st["shift"])
        _close(bw["dz"], z.grad, "dz mode %d" % mode)
        _close(bw["dgamma"], gamma.grad, "dgamma mode %d" % mode)
        _close(bw["dbeta"], beta.grad, "dbeta mode %d" % mode)
        # the sums given from outside reproduce the same dz
        _close(R.bn_bwd(d["g"], d["z"], operand, mode, d["gamma"], st["mean"], st["invstd"], st["scale"], st["shift"], bw["dgamma"], bw["dbeta"])["dz"], z.grad, "dz")
        assert (bw["A_dz"] >= np.abs(bw["dz"]) * (1 - 1e-12)).all() and (bw["A_gm"] >= np.abs(bw["gm"]) * (1 - 1e-12)).all()
    # shifted sums, any K, both partial layouts
    for k in (np.zeros(c), d["rm"], d["z"].mean(0) + 0.3):
        rows = np.array_split(np.arange(m), min(m, 5))
        part = np.stack([np.stack([(d["z"][r] - k).sum(0), ((d["z"][r] - k) ** 2).sum(0)], axis=-1) for r in rows])        # [rows][C][2]
        for layout, p in (("rm", part), ("cm", part.transpose(1, 0, 2).copy())):
            s1, s2 = R.finalize(p, layout)
            st2 = R.bn_stats_from_sums(s1, s2, m, k, d["gamma"], d["beta"], EPS, MOM, d["rm"], d["rv"])
            for q in ("mean", "scale", "shift", "running_mean", "running_var"):
                assert rel_err(st2[q], st[q]) < 1e-9, q                                  # (cancellation in s2 / M - d^2: not a 1e-12 quantity)


@pytest.mark.parametrize("m,c", [(37, 12), (300, 8)])
@pytest.mark.parametrize("act", [1, 2])
def test_residual_and_two_batchnorm_sum(m, c, act):
    d = _data(m, c, 11 * m + c)
    fa = F.relu if act == 1 else F.hardswish
    # identity residual
    z, gamma, beta, r = _t(d["z"], True), _t(d["gamma"], True), _t(d["beta"], True), _t(d["r"], True)
    y = fa(F.batch_norm(z, None, None, gamma, beta, True, MOM, EPS) + r)
    y.backward(_t(d["g"]))
    st = R.bn_stats(d["z"], d["gamma"], d["beta"], EPS, MOM)
    assert st["running_mean"] is None and st["running_var"] is None
    ap = R.bn_apply(d["z"], st["scale"], st["shift"], r=d["r"], act=act)
    _close(ap["out"], y, "out")
    if act == 1:
        for mode, operand in ((1, ap["out"]), (4, ap["bits"])):
            bw = R.bn_bwd(d["g"], d["z"], operand, mode, d["gamma"], st["mean"], st["invstd"])
            _close(bw["dz"], z.grad, "dz")
            _close(bw["gm"], r.grad, "gm = the skip connection's gradient")
            _close(bw["dgamma"], gamma.grad, "dgamma")
            _close(bw["dbeta"], beta.grad, "dbeta")
    # the downsample block: act(bn_a(z_a) + bn_b(z_b))
    za, zb = _t(d["z"], True), _t(d["zb"], True)
    ga_, ba_, gb_, bb_ = _t(d["gamma"], True), _t(d["beta"], True), _t(d["gamma_b"], True), _t(d["beta_b"], True)
    y = fa(F.batch_norm(za, None, None, ga_, ba_, True, MOM, EPS) + F.batch_norm(zb, None, None, gb_, bb_, True, MOM, EPS))
    y.backward(_t(d["g"]))
    sb = R.bn_stats(d["zb"], d["gamma_b"], d["beta_b"], EPS, MOM)
    ap = R.bn_apply(d["z"], st["scale"], st["shift"], r=d["zb"], rscale=sb["scale"], rshift=sb["shift"], act=act)
    _close(ap["out"], y, "out of the pair")
    assert (ap["A"] >= np.abs(ap["out"]) * (1 - 1e-12)).all()
    if act == 1:
        a, b = R.bn_bwd_pair(d["g"], d["z"], d["zb"], ap["bits"], d["gamma"], st["mean"], st["invstd"], d["gamma_b"], sb["mean"], sb["invstd"])
        for res, zt, gt, bt in ((a, za, ga_, ba_), (b, zb, gb_, bb_)):
            _close(res["dz"], zt.grad, "pair dz")
            _close(res["dgamma"], gt.grad, "pair dgamma")
            _close(res["dbeta"], bt.grad, "pair dbeta")
        a2, b2 = R.bn_bwd_pair(d["g"], d["z"], d["zb"], ap["bits"], d["gamma"], st["mean"], st["invstd"], d["gamma_b"], sb["mean"], sb["invstd"],
                               (a["dgamma"], a["dbeta"]), (b["dgamma"], b["dbeta"]))
        _close(a2["dz"], za.grad, "pair dz from given sums")
        _close(b2["dz"], zb.grad, "pair dz from given sums")


def _argmax_from_flat(idx, w):
    """torch's flat input index ih * w + iw per pooled element [n][c][ho][wo] -> the window position dy * 3 + dx, NHWC."""
    idx = idx.numpy()
    n, c, ho, wo = idx.shape
    ih, iw = idx // w, idx % w
    oh, ow = np.arange(ho)[None, None, :, None], np.arange(wo)[None, None, None, :]
    dy, dx = ih - (2 * oh - 1), iw - (2 * ow - 1)
    assert ((dy >= 0) & (dy < 3) & (dx >= 0) & (dx < 3)).all()
    return (dy * 3 + dx).transpose(0, 2, 3, 1).astype(np.uint8)


@pytest.mark.parametrize("family", ["lattice", "random"])
@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=str)
def test_maxpool_over_relu_batchnorm(shape, family):
    n, h, w, c = shape
    o = K.pool_case(shape, "f32", family)
    z = _t(o["z"].transpose(0, 3, 1, 2), True)
    u = z * _t(o["scale"]).view(1, c, 1, 1) + _t(o["shift"]).view(1, c, 1, 1)
    y, idx = F.max_pool2d(F.relu(u), 3, 2, 1, return_indices=True)
    g = _t(o["g"].transpose(0, 3, 1, 2))
    a = F.relu(u).detach().requires_grad_(True)                   # the pool alone: ga
    F.max_pool2d(a, 3, 2, 1).backward(g)
    fw = R.maxpool_bn_relu_fwd(o["z"], o["scale"], o["shift"])
    _close(fw["y"], y.permute(0, 2, 3, 1), "y")
    assert np.array_equal(fw["argmax"], _argmax_from_flat(idx, w)), "argmax byte"
    bw = R.maxpool_bn_relu_bwd(fw["argmax"], o["g"], h, w)
    _close(bw["ga"], a.grad.permute(0, 2, 3, 1), "ga")
    assert (bw["A_ga"] >= np.abs(bw["ga"]) * (1 - 1e-12)).all()
    if family == "lattice":
        assert (fw["y"][..., c - 1] == 0).all() and (fw["argmax"][0, 0, 0, c - 1] == 4), "the all-zero channel: first in-image tap of the corner window"
    # pool(relu(bn(z))) with batch statistics, autograd through everything
    m = n * h * w
    gamma, beta = _t(o["gamma"], True), _t(np.linspace(-0.5, 0.5, c), True)
    z2 = _t(o["z"].transpose(0, 3, 1, 2), True)
    if m == 1:
        mean, var = z2.mean((0, 2, 3), keepdim=True), z2.var((0, 2, 3), unbiased=False, keepdim=True)
        bn = (z2 - mean) / torch.sqrt(var + EPS) * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    else:
        bn = F.batch_norm(z2, None, None, gamma, beta, True, MOM, EPS)
    y2 = F.max_pool2d(F.relu(bn), 3, 2, 1)
    y2.backward(g)
    st = R.bn_stats(o["z"].reshape(-1, c), o["gamma"], np.linspace(-0.5, 0.5, c), EPS, MOM)
    fw2 = R.maxpool_bn_relu_fwd(o["z"], st["scale"], st["shift"])
    _close(fw2["y"], y2.permute(0, 2, 3, 1), "y of pool(relu(bn(z)))")
    b2 = R.maxpool_bn_relu_bwd(fw2["argmax"], o["g"], h, w, o["z"], o["gamma"], st["mean"], st["invstd"], st["scale"], st["shift"])["bn"]
    _close(b2["dz"].reshape(n, h, w, c), z2.grad.permute(0, 2, 3, 1), "dz")
    _close(b2["dgamma"], gamma.grad, "dgamma")
    _close(b2["dbeta"], beta.grad, "dbeta")


def test_bf16_rounding_is_round_to_nearest_even():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096), [1.00390625, 1.01171875, -1.00390625, 0.0, 3.0, 255.5, 2.0 ** -130]])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(R.round_bf16(x), want)
    assert np.array_equal(R.round_storage(x, "f32"), x.astype(np.float32).astype(np.float64))


def test_hard_swish_gradient_at_the_kinks_follows_autograd():
    u = _t([-3.0, 3.0, -3.5, 3.5, 0.0, -1.0, 2.999], True)
    F.hardswish(u).sum().backward()
    got = R.hswish_grad(u.detach().numpy())
    assert np.array_equal(got[:4], u.grad.numpy()[:4]) and np.abs(got - u.grad.numpy()).max() < 1e-15


# ---------------------------------------------------------------------------------------------------------------- the GPU module's input conditions
def _share(und):
    return float(und.mean())


@pytest.mark.parametrize("m,c,dtypes", K.MATRICES, ids=lambda v: str(v))
def test_matrix_cases_have_almost_no_undecided_elements(m, c, dtypes):
    for dtype in dtypes:
        o = K.matrix_case(m, c, dtype)
        assert np.array_equal(R.round_storage(o["z"], dtype), o["z"]) and np.array_equal(R.round_storage(o["gwide"], dtype), o["gwide"])
        shares = []
        for act in (0, 1, 2):
            shares.append(_share(R.bn_apply(o["z"], o["scale"], o["shift"], act=act)["undecided"]))
            shares.append(_share(R.bn_apply(o["z"], o["scale"], o["shift"], r=o["r"], act=act)["undecided"]))
            shares.append(_share(R.bn_apply(o["z"], o["scale"], o["shift"], r=o["r"], rscale=o["rscale"], rshift=o["rshift"], act=act)["undecided"]))
        shares.append(_share(R.bn_apply(o["z"], o["scale"], o["shift"], r=o["zb"], rscale=o["scale_b"], rshift=o["shift_b"], act=1)["undecided"]))
        for mode in (2, 3):
            shares.append(_share(R.bn_mask(o["gwide"][:, :c], o["z"], None, mode, o["scale"], o["shift"])[2]))
        assert max(shares) <= K.UNDECIDED_SHARE, (dtype, shares)
        if m * c < 1.0 / K.UNDECIDED_SHARE:
            assert max(shares) == 0.0


@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=str)
def test_pool_cases_lattice_is_exact_and_random_has_almost_no_undecided_elements(shape):
    n, h, w, c = shape
    for dtype in K.DTYPES:
        o = K.pool_case(shape, dtype, "lattice")
        fw = R.maxpool_bn_relu_fwd(o["z"], o["scale"], o["shift"])
        bw = R.maxpool_bn_relu_bwd(fw["argmax"], o["g"], h, w, o["z"], o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"])
        # every operand, every intermediate of either order of evaluation (product, then sum) and every result is a bf16 number: nothing rounds
        for what in (o["z"], o["g"], o["scale"], o["shift"], o["z"] * o["scale"], fw["u"], fw["y"], bw["ga"], bw["A_ga"], bw["bn"]["gm"], bw["bn"]["xhat"]):
            assert np.array_equal(R.round_bf16(what), what)
        # the sums: multiples of 1/16 below 2^24 / 16 in absolute value however they are ordered
        assert bw["bn"]["abs_dbeta"].max() < 2 ** 20 and (np.abs(bw["bn"]["gm"] * bw["bn"]["xhat"]).sum(axis=0) < 2 ** 20).all()
        assert np.array_equal(np.round(bw["bn"]["gm"] * bw["bn"]["xhat"] * 16), bw["bn"]["gm"] * bw["bn"]["xhat"] * 16)
        assert (fw["u"][fw["undecided"]] == 0).all(), "a lattice activation within 2^-20 of zero that is not zero"
        # ties among the positive maxima, and windows of zeros only
        win_ties = 0
        for k in range(9):
            dy, dx = divmod(k, 3)
            pad = np.full((n, 2 * o["ho"] + 1, 2 * o["wo"] + 1, c), -np.inf)
            pad[:, 1:h + 1, 1:w + 1] = fw["a"]
            win_ties += int(((pad[:, dy:dy + 2 * o["ho"]:2, dx:dx + 2 * o["wo"]:2] == fw["y"]) & (fw["y"] > 0) & (fw["argmax"] != k)).sum())
        if h * w > 1:
            assert win_ties > 0, "no positive tie in any window"
        assert (fw["y"][..., c - 1] == 0).all()
        o = K.pool_case(shape, dtype, "random")
        assert np.array_equal(R.round_storage(o["z"], dtype), o["z"]) and np.array_equal(R.round_storage(o["g"], dtype), o["g"])
        fw = R.maxpool_bn_relu_fwd(o["z"], o["scale"], o["shift"])
        assert _share(fw["undecided"]) <= K.UNDECIDED_SHARE
        if fw["undecided"].size < 1.0 / K.UNDECIDED_SHARE:
            assert not fw["undecided"].any()


def test_statistics_cases_are_conditioned_as_named():
    for m, c, dtypes in K.MATRICES:
        for dtype in dtypes:
            if m == 1:
                continue
            near, zero = K.stats_case(m, c, dtype, "mean30_knear"), K.stats_case(m, c, dtype, "mean30_k0")
            assert np.array_equal(near["z"], zero["z"]), "the same data with K = 0"
            sd = np.sqrt(near["ref"]["var"])
            assert (np.abs(near["ref"]["mean"] / sd) > 15).all()
            if m >= 37:
                assert (np.abs(near["ref"]["mean"] - near["running_mean"]) < 1.25 * sd + 0.5).all(), "K within about one standard deviation of the mean"
                assert near["factor"] < 6 and zero["factor"] > 200 and zero["scaled"] and not near["scaled"]
                assert K.stats_case(m, c, dtype, "mean3_k")["factor"] < 60


def test_finalize_cases_separate_the_layouts():
    for c in K.FINALIZE_CHANNELS:
        for nblk in K.FINALIZE_ROWS:
            o = K.finalize_case(c, nblk)
            assert (o["ref"]["var"] > 1.0).all()
            if nblk > 1 and c > 1:
                s1_wrong, s2_wrong = R.finalize(o["part"].reshape(nblk, c, 2), "rm")
                assert rel_err(s2_wrong, o["s2"]) > 1e-2, "a row-major reading of the channel-major partials must show"
