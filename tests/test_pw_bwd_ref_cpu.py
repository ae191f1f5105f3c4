"""CPU: what tests/test_pw_bwd_kernels_gpu.py relies on.  (1) tests/pw_bwd_ref.py with the roundings switched off equals torch float64 autograd of the
bottleneck tail -- out = relu(bn3(conv3(a2)) + identity), a2 = relu(bn2(z2)), and the downsample form relu(bn3(.) + bn_d(conv_d(x))) -- to 1e-12.  (2) The
gate margins and the 1 % allowance conditions hold for every case of tests/pw_bwd_cases.py, for those very inputs.  (3) The launch-plan ports reproduce
hand-computed splits.  (4) The comparison functions the GPU module asserts with reject the ways these kernels can go wrong: a row taken from the next chunk,
two 16-byte channel units of a row swapped, the gate bit of the neighbouring channel, the ragged tail's rows included in a sum, a split boundary moved by
64 rows, the remainder row dropped."""
import numpy as np
import pytest
import torch

import conv_epilogue_ref as E
import pw_bwd_cases as K
import pw_bwd_ref as R
from helpers import policy_set, rel_err

EPS = K.EPS


# ------------------------------------------------------------------------------------------------ (1) the reference against autograd
def _bn(z, gamma, beta):
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    return (z - mean) * invstd * gamma + beta, mean, invstd


def _leaf(t):
    return t.clone().double().requires_grad_(True)


def _tail(m, downsample, seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)          # noqa: E731
    t = dict(z2=_leaf(rn(m, 64) * 1.2 + 0.1), g2=_leaf(torch.rand(64, generator=gen, dtype=torch.float64) + 0.5), b2=_leaf(rn(64) * 0.3),
             w3=_leaf(rn(256, 64) * 0.17), g3=_leaf(torch.rand(256, generator=gen, dtype=torch.float64) + 0.5), b3=_leaf(rn(256) * 0.3))
    y2, t["mean2"], t["invstd2"] = _bn(t["z2"], t["g2"], t["b2"])
    a2 = torch.relu(y2)
    a2.retain_grad()
    z3 = a2 @ t["w3"].t()
    z3.retain_grad()
    y3, t["mean3"], t["invstd3"] = _bn(z3, t["g3"], t["b3"])
    if downsample:
        t.update(x=_leaf(rn(m, 64)), wd=_leaf(rn(256, 64) * 0.17), gd=_leaf(torch.rand(256, generator=gen, dtype=torch.float64) + 0.5), bd=_leaf(rn(256) * 0.3))
        zd = t["x"] @ t["wd"].t()
        zd.retain_grad()
        yd, t["meand"], t["invstdd"] = _bn(zd, t["gd"], t["bd"])
        t["zd"] = zd
        out = torch.relu(y3 + yd)
    else:
        t["identity"] = rn(m, 256)
        out = torch.relu(y3 + t["identity"])
    t["G"] = rn(m, 256)
    (out * t["G"]).sum().backward()
    t.update(a2=a2, z3=z3, out=out)
    return t


def _n(t):
    return t.detach().numpy()


def _close(a, b, what):
    assert rel_err(a, b) < 1e-12, (what, rel_err(a, b))


@pytest.mark.parametrize("m", [37, 209])
def test_reference_equals_autograd_of_the_plain_block(m):
    t = _tail(m, False, m)
    bits = E.pack_bits(_n(t["out"]) > 0)
    a2, w, g = _n(t["a2"]), _n(t["w3"]), _n(t["G"])
    mean, invstd = _n(t["mean3"]), _n(t["invstd3"])
    s = R.conv_bnbwd_sums(a2, w, g, bits, mean, invstd, rounding=False)
    _close(s["v1"].sum(0), _n(t["b3"].grad), "dbeta3")
    _close(s["v2"].sum(0), _n(t["g3"].grad), "dgamma3")
    assert not s["und_z"].any() and not s["allow2"].any()
    scale2 = _n(t["g2"]) * _n(t["invstd2"])
    shift2 = _n(t["b2"]) - _n(t["mean2"]) * scale2
    r = R.conv1x1_bwd_fused(a2, w, g, bits, _n(t["g3"]), mean, invstd, s["v2"].sum(0), s["v1"].sum(0), _n(t["z2"]), _n(t["mean2"]), _n(t["invstd2"]), scale2, shift2,
                            rounding=False)
    _close(r["dz"], _n(t["z3"].grad), "dz3")
    _close(r["dx"], _n(t["a2"].grad), "da2")
    _close(R.wgrad(r["dz"], a2)[0], _n(t["w3"].grad), "dW3")
    _close(r["v1"].sum(0), _n(t["b2"].grad), "dbeta2")
    _close(r["v2"].sum(0), _n(t["g2"].grad), "dgamma2")
    assert not r["allow_dx"].any() and not r["u_dz"].any()
    # per-split slabs add up to dW; partial rows add up to the sums
    bounds = K.split_bounds(m, 128)
    _close(sum(R.wgrad(r["dz"], a2, be)[0] for be in bounds), _n(t["w3"].grad), "the slabs' sum")
    _close(R.rows_sum(r["v2"], bounds).sum(1), _n(t["g2"].grad), "the partial rows' sum")
    # the statistics pass: sum (z - K), sum (z - K)^2 -> mean and biased variance
    kk = mean + 0.05
    st = R.conv_stats(a2, w, kk, rounding=False)
    d = st["v1"].sum(0) / m
    _close(kk + d, mean, "mean from the shifted sums")
    _close(1.0 / np.sqrt(st["v2"].sum(0) / m - d * d + EPS), invstd, "invstd from the shifted sums")
    # bn2's backward apply + conv2's weight gradient (mask mode 2) on the autograd da2
    x1 = np.random.default_rng(m).standard_normal((m, 256))
    b = R.bn_bwd_apply_wgrad(_n(t["a2"].grad), _n(t["z2"]), None, 2, _n(t["g2"]), _n(t["mean2"]), _n(t["invstd2"]), scale2, shift2, _n(t["g2"].grad), _n(t["b2"].grad),
                             rounding=False)
    _close(b["dz"], _n(t["z2"].grad), "dz2")
    _close(R.wgrad(b["dz"], x1)[0], _n(t["z2"].grad).T @ x1, "dW2")


@pytest.mark.parametrize("m", [37, 209])
def test_reference_equals_autograd_of_the_downsample_block(m):
    t = _tail(m, True, m + 1)
    bits = E.pack_bits(_n(t["out"]) > 0)
    a2, x, g = _n(t["a2"]), _n(t["x"]), _n(t["G"])
    sa = R.conv_bnbwd_sums(a2, _n(t["w3"]), g, bits, _n(t["mean3"]), _n(t["invstd3"]), rounding=False)
    sb = R.conv_bnbwd_sums(x, _n(t["wd"]), g, bits, _n(t["meand"]), _n(t["invstdd"]), rounding=False)
    _close(sa["v2"].sum(0), _n(t["g3"].grad), "dgamma3")
    _close(sb["v2"].sum(0), _n(t["gd"].grad), "dgamma_d")
    _close(sb["v1"].sum(0), _n(t["bd"].grad), "dbeta_d")
    ra, rb_ = R.bn_bwd_pair_wgrad(g, _n(t["z3"]), _n(t["zd"]), bits, _n(t["g3"]), _n(t["mean3"]), _n(t["invstd3"]), _n(t["gd"]), _n(t["meand"]), _n(t["invstdd"]),
                                  rounding=False)
    _close(ra["dgamma"], _n(t["g3"].grad), "pair dgamma3")
    _close(rb_["dbeta"], _n(t["bd"].grad), "pair dbeta_d")
    _close(ra["dz"], _n(t["z3"].grad), "dz3")
    _close(rb_["dz"], _n(t["zd"].grad), "dz_d")
    _close(R.wgrad(ra["dz"], a2)[0], _n(t["w3"].grad), "dW3")
    _close(R.wgrad(rb_["dz"], x)[0], _n(t["wd"].grad), "dW_d")
    # the one-pass form of conv3's backward gives the same dz3 / da2 from the final sums
    r = R.conv1x1_bwd_fused(a2, _n(t["w3"]), g, bits, _n(t["g3"]), _n(t["mean3"]), _n(t["invstd3"]), _n(t["g3"].grad), _n(t["b3"].grad), rounding=False)
    _close(r["dz"], _n(t["z3"].grad), "dz3 (fused)")
    _close(r["dx"], _n(t["a2"].grad), "da2 (fused)")


def test_rounding_points():
    """rounding=True rounds z3, dz3 and dx to bf16 and nothing else."""
    o, r = K.conv_case(209), K.fused_ref(209)
    for k_ in ("z3", "dz", "dx"):
        assert np.array_equal(E.rnd(r[k_], "bf16"), r[k_]), k_
    assert np.array_equal(r["z3"], E.rnd(o["acc"], "bf16")) and np.array_equal(r["dx"], E.rnd(r["dz"] @ o["w"], "bf16"))
    gap = R.midpoint_gap(np.array([1.0 + 2.0 ** -8 - 1e-6, 1.0 - 2.0 ** -9 + 1e-6, 0.3]), E.rnd(np.array([1.0 + 2.0 ** -8 - 1e-6, 1.0 - 2.0 ** -9 + 1e-6, 0.3]), "bf16"))
    assert abs(gap[0] - 1e-6) < 1e-12 and abs(gap[1] - 1e-6) < 1e-12 and gap[2] > 1e-4          # (the spacing halves below a power of two)


# ------------------------------------------------------------------------------------------------ (2) the conditions of every case
def _share_ok(al, ref, what):
    s = K.allowance_share(al, ref)
    assert s < K.ALLOW_SHARE, (what, s)
    return s


@pytest.mark.parametrize("m,seed", sorted({(c[0], c[1]) for c in K.fused_cases() + K.pair_cases()} | {(m, 0) for m in K.LEG_ROWS}))
def test_conditions_of_the_conv_cases(m, seed):
    """Gate margin of bn2; allowances of dx, every slab, dw (fused) and of every partial row and dgamma (pair), under the default and both forced plans."""
    o, r = K.conv_case(m, seed), K.fused_ref(m, seed)
    b2 = o["bn2"]
    assert float(E.gate_margin(b2["z"], b2["scale"], b2["shift"]).min()) > K.GATE_MARGIN
    assert 0.2 < (b2["scale"][None, :] * b2["z"] + b2["shift"][None, :] > 0).mean() < 0.8
    worst = dict(dx=_share_ok(r["allow_dx"], r["dx"], "dx"), dw=_share_ok(r["u_dz"].T @ np.abs(o["a"]), R.wgrad(r["dz"], o["a"])[0], "dw"), slab=0.0, part=0.0)
    for wgs in (256, 1, 2):
        bounds = K.split_bounds(m, K.fused_plan(m, wgs=wgs)[1])
        for b, e in bounds:
            worst["slab"] = max(worst["slab"], _share_ok(r["u_dz"][b:e].T @ np.abs(o["a"][b:e]), R.wgrad(r["dz"], o["a"], (b, e))[0], "slab"))
        for s in (o["sums"], o["pair_a"], o["pair_b"]):
            worst["part"] = max(worst["part"], _share_ok(R.rows_sum(s["allow2"], bounds), R.rows_sum(s["v2"], bounds), "partial rows"))
            _share_ok(s["allow2"].sum(0), s["v2"].sum(0), "dgamma")
    print("m %d seed %d: largest allowance shares %s; undecided z3 %.3g, dz3 %.3g" % (m, seed, {k_: "%.3g" % v for k_, v in worst.items()}, o["sums"]["und_z"].mean(),
                                                                                  r["und_dz"].mean()))
    # dgamma is not noise (what the prescribed g is for): in the typical channel the sum keeps a good part of its terms' magnitudes
    for s in (o["sums"], o["pair_a"], o["pair_b"]):
        assert np.median(np.abs(s["v2"].sum(0)) / np.abs(s["v2"]).sum(0)) > 0.2


def test_conditions_of_the_gated_apply_cases():
    for mode, c, k, m, _, _ in K.bnwg_cases():
        if mode == 2:
            o = K.bnwg_case(m, c, k, mode)
            assert float(E.gate_margin(o["z"], o["scale"], o["shift"]).min()) > K.GATE_MARGIN, (c, k, m)
            assert 0.2 < (o["scale"][None, :] * o["z"] + o["shift"][None, :] > 0).mean() < 0.8


@pytest.mark.parametrize("m,n", sorted({(c[0], c[1]) for c in K.pw_sums_cases()}))
def test_conditions_of_the_pw_sums_cases(m, n):
    o = K.pw_sums_case(m, n)
    rows = K.stats_rows(m)
    for wgs in (3, 1):
        nwg = K.pw_sums_nwg(m, n, rows, 256, wgs)
        for what, r in o["ref"].items():
            a1 = r.get("allow1", np.zeros(r["v1"].shape))
            if nwg:
                blocks = K.pw_sums_blocks(m, nwg)
                assert sorted(b for bl in blocks for b in bl) == list(range((m + 31) // 32))
                _share_ok(R.blocks_sum(a1, blocks), R.blocks_sum(r["v1"], blocks), what + " s1")
                _share_ok(R.blocks_sum(r["allow2"], blocks), R.blocks_sum(r["v2"], blocks), what + " s2")
            else:
                runs = [(b, min(m, b + 128)) for b in range(0, m, 128)]
                _share_ok(R.rows_sum(a1, runs), R.rows_sum(r["v1"], runs), what + " s1")
                _share_ok(R.rows_sum(r["allow2"], runs), R.rows_sum(r["v2"], runs), what + " s2")


# ------------------------------------------------------------------------------------------------ (3) the plan ports
def test_plan_ports_reproduce_hand_computed_splits():
    with policy_set(pwbf_wgs=256, bnwg_wgs=256, pw_sums=1, pw_sums_wgs=3):
        sizes = lambda m, rows: [e - b for b, e in K.split_bounds(m, rows)]          # noqa: E731
        # the fused / pair walker: max(128, ceil64(m / 256)) rows per workgroup
        assert K.fused_plan(17) == (1, 128) and K.chunks_of(17, 128) == [1]
        assert K.fused_plan(64) == (1, 128) and K.chunks_of(64, 128) == [1]
        assert sizes(209, K.fused_plan(209)[1]) == [128, 81]
        assert K.fused_plan(465)[0] == 4 and sizes(465, 128) == [128, 128, 128, 81]
        assert K.fused_plan(3665) == (29, 128) and 29 % 8 != 0
        assert K.fused_plan(40017) == (209, 192) and sizes(40017, 192)[-1] == 81 and set(K.chunks_of(40017, 192)[:-1]) == {3}
        assert K.fused_plan(32767)[1] == 128 and K.fused_plan(32769)[1] == 192          # two chunks per workgroup for every m up to 32,768
        assert K.fused_plan(802816) == (256, 3136)
        assert K.fused_plan(100, 512, 128) == (0, 0) and K.fused_plan(100, 256, 128) == (0, 0)
        # bnbwd_wgrad: at least 256 rows per workgroup, workgroups shared among the column and k tiles
        assert K.bnwg_plan(17, 256, 64, 1, 4) == (1, 256, 1, 1) and K.bnwg_plan(64, 256, 64, 1, 4)[0] == 1
        assert K.bnwg_plan(209, 256, 64, 1, 4)[0] == 1 and K.chunks_of(209, 256) == [4] and 209 == 3 * 64 + 17
        assert sizes(465, K.bnwg_plan(465, 256, 64, 1, 4)[1]) == [256, 209]
        assert K.bnwg_plan(3665, 256, 64, 1, 4)[0] == 15
        assert K.bnwg_plan(40017, 256, 64, 1, 4)[:2] == (157, 256)
        assert K.bnwg_plan(40017, 512, 64, 1, 4) == (126, 320, 2, 1)                    # 128 workgroups per tile: ceil64(313) = 320 rows
        assert K.bnwg_plan(465, 64, 512, 1, 2)[2:] == (1, 2) and K.bnwg_plan(465, 256, 256, 1, 2)[2:] == (2, 1)
        assert K.bnwg_tile(256, 64, 1, 4) == (256, 64) and K.bnwg_tile(256, 128, 1, 4) == (256, 128) and K.bnwg_tile(64, 256, 1, 2) == (64, 256)
        assert K.bnwg_tile(128, 256, 1, 2) == (128, 256) and K.bnwg_tile(256, 256, 1, 2) == (128, 256) and K.bnwg_tile(256, 128, 2, 4) == (256, 128)
        assert K.bnwg_tile(96, 64, 1, 4) is None and K.bnwg_tile(1024, 256, 1, 2) is None and K.bnwg_tile(256, 64, 1, 2) is None
        assert K.bnwg_plan(209, 96, 64, 1, 4)[0] == 0 and K.bnwg_plan(209, 1024, 256, 1, 2)[0] == 0
        # pw_sums: 16 partial rows are the least that leave 8 workgroups
        assert K.pw_sums_nwg(2048, 256, 16, 256) == 8 and K.pw_sums_nwg(2047, 256, 16, 256) == 8 and K.pw_sums_nwg(1921, 128, 16, 256) == 8
        assert K.pw_sums_nwg(1920, 256, 15, 256) == 0
        assert K.pw_sums_nwg(2225, 256, 18, 256) == 8
        bl = K.pw_sums_blocks(2225, 8)
        assert (2225 + 31) // 32 == 70 and sorted(len([b for b in w_ if b % 4 == i]) for w_ in bl for i in range(4)).count(3) == 6 and 2225 - 69 * 32 == 17
        assert bl[0] == [0, 32, 64, 1, 33, 65, 2, 34, 66, 3, 35, 67] and bl[7] == [28, 60, 29, 61, 30, 62, 31, 63]
        assert K.pw_sums_nwg(40017, 256, 313, 256) == 152 and K.pw_sums_nwg(40017, 128, 313, 256) == 152
        assert K.pw_sums_nwg(40017, 256, 313, 256, 1) == 128
    with policy_set(pwbf_wgs=1, bnwg_wgs=1):
        assert [K.chunks_of(m, K.fused_plan(m)[1]) for m in K.LEG_ROWS] == [[1], [4], [7], [7], [8]]
        assert [K.bnwg_plan(m, 256, 64, 1, 4)[0] for m in K.LEG_ROWS] == [1] * 5 and K.bnwg_plan(465, 512, 64, 1, 4)[:2] == (1, 512)
    with policy_set(pwbf_wgs=2, bnwg_wgs=2):
        assert [e - b for b, e in K.split_bounds(401, K.fused_plan(401)[1])] == [256, 145]
        assert [e - b for b, e in K.split_bounds(465, K.bnwg_plan(465, 256, 64, 1, 4)[1])] == [256, 209]
        assert K.bnwg_plan(465, 512, 64, 1, 4)[0] == 1                                  # two column tiles share the two workgroups
    with policy_set(pw_sums=0):
        assert K.pw_sums_nwg(2048, 256, 16, 256) == 0


# ------------------------------------------------------------------------------------------------ (4) the comparisons bite
def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


M_BITE = 465


def _swap_units(a, row, u0=0, u1=1):
    b = a.copy()
    b[row, 8 * u0:8 * u0 + 8], b[row, 8 * u1:8 * u1 + 8] = a[row, 8 * u1:8 * u1 + 8], a[row, 8 * u0:8 * u0 + 8]
    return b


def _row_from_next_chunk(a, row):
    b = a.copy()
    b[row] = a[row + K.CH]
    return b


def _neighbour_bits(bits):
    """Every channel gated by the bit of channel + 1."""
    m = E.unpack_bits(bits, bits.shape[1] * 4) > 0
    return E.pack_bits(np.roll(m, -1, axis=1))


def test_comparisons_reject_a_wrong_fused_backward():
    o, r = K.conv_case(M_BITE), K.fused_ref(M_BITE)
    b2 = o["bn2"]
    ns, rows = K.fused_plan(M_BITE, wgs=256)
    bounds = K.split_bounds(M_BITE, rows)
    K.cmp_tensor("dx", r["dx"], r["dx"], 6e-3, r["allow_dx"], l2=False)
    _rejects(K.cmp_tensor, "dx", _row_from_next_chunk(r["dx"], 10), r["dx"], 6e-3, r["allow_dx"], l2=False)
    _rejects(K.cmp_tensor, "dx", _swap_units(r["dx"], 200), r["dx"], 6e-3, r["allow_dx"], l2=False)
    bad = R.conv1x1_bwd_fused(o["a"], o["w"], o["g"], _neighbour_bits(o["bits"]), o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], acc=o["acc"])
    _rejects(K.cmp_tensor, "dx", bad["dx"], r["dx"], 6e-3, r["allow_dx"], l2=False)
    # slabs: the conv input's units swapped in one row; a row from the next chunk; the split boundary moved by 64 rows; the next split's rows included
    b, e = bounds[1]
    ref, al = R.wgrad(r["dz"], o["a"], (b, e))[0], r["u_dz"][b:e].T @ np.abs(o["a"][b:e])
    K.cmp_tensor("slab", ref, ref, 2e-6, al)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], _swap_units(o["a"], b + 5), (b, e))[0], ref, 2e-6, al)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], _row_from_next_chunk(o["a"], b + 5), (b, e))[0], ref, 2e-6, al)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], o["a"], (b + 64, e + 64))[0], ref, 2e-6, al)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], o["a"], (b, e + 17))[0], ref, 2e-6, al)
    _rejects(K.cmp_tensor, "slab", R.wgrad(bad["dz"], o["a"], (b, e))[0], ref, 2e-6, al)
    # bn2's partial rows at the LOOSEST bound a measured one may take
    v1, v2 = R.gated_sums(r["dx"], b2["z"], b2["mean"], b2["invstd"], b2["scale"], b2["shift"])
    t64 = np.stack([R.rows_sum(v1, bounds), R.rows_sum(v2, bounds)], axis=2)
    lay = K.kernel_layout(t64)
    got = K.part_rows("sums_part", lay, ns)
    cap = K.CAPS["fused"]
    K.cmp_tensor("s2", got[:, :, 1], t64[:, :, 1], cap)
    moved = [(b_ + 64, min(M_BITE, e_ + 64)) for b_, e_ in bounds]
    _rejects(K.cmp_tensor, "s2", R.rows_sum(v2, moved), t64[:, :, 1], cap)
    _rejects(K.cmp_tensor, "s1", R.rows_sum(v1, moved), t64[:, :, 0], cap)
    tail = t64.copy()
    tail[:, -1, :] += 15 * np.stack([v1[-1], v2[-1]], axis=1)                           # the ragged tail's masked rows (clamped to the last row) summed
    _rejects(K.cmp_tensor, "s1", tail[:, :, 0], t64[:, :, 0], cap)
    _rejects(K.cmp_tensor, "s2", tail[:, :, 1], t64[:, :, 1], cap)
    z_sw = _swap_units(b2["z"], 300)
    _rejects(K.cmp_tensor, "s2", R.rows_sum(R.gated_sums(r["dx"], z_sw, b2["mean"], b2["invstd"], b2["scale"], b2["shift"])[1], bounds), t64[:, :, 1], cap)
    dropped = lay.copy()
    dropped[:, ns:] = 0.0
    _rejects(K.part_rows, "sums_part", dropped, ns)
    swapped = np.concatenate([lay[:, ns:], lay[:, :ns]], axis=1)
    _rejects(K.part_rows, "sums_part", swapped, ns)
    nan = lay.copy()
    nan[3, ns + 1, 1] = np.nan
    _rejects(K.part_rows, "sums_part", nan, ns)


def test_comparisons_reject_wrong_sums_on_a_recomputed_conv():
    o = K.conv_case(M_BITE)
    s = o["pair_a"]
    ns, rows = K.fused_plan(M_BITE, wgs=256)
    bounds = K.split_bounds(M_BITE, rows)
    ref2, al2 = R.rows_sum(s["v2"], bounds), R.rows_sum(s["allow2"], bounds)
    ref1 = R.rows_sum(s["v1"], bounds)
    c1, c2 = K.CAPS["pair_s1"], K.CAPS["pair_s2"]
    K.cmp_tensor("s2", K.part_rows("part", K.kernel_layout(np.stack([ref1, ref2], axis=2)), ns)[:, :, 1], ref2, c2, al2)
    for name, kw in (("a row of a2 from the next chunk", dict(a=_row_from_next_chunk(o["a"], 3))), ("two units of a2 swapped", dict(a=_swap_units(o["a"], 3))),
                     ("the neighbour's gate bit", dict(bits=_neighbour_bits(o["bits"]))), ("two units of g swapped", dict(g=_swap_units(o["g_pair"], 130, 4, 5)))):
        args = dict(a=o["a"], g=o["g_pair"], bits=o["bits"])
        args.update(kw)
        bad = R.conv_bnbwd_sums(args["a"], o["w"], args["g"], args["bits"], o["mean"], o["invstd"])
        _rejects(K.cmp_tensor, name, R.rows_sum(bad["v2"], bounds), ref2, c2, al2)
        if "a" not in kw:
            _rejects(K.cmp_tensor, name, R.rows_sum(bad["v1"], bounds), ref1, c1)
    moved = [(b + 64, min(M_BITE, e + 64)) for b, e in bounds]
    _rejects(K.cmp_tensor, "boundary", R.rows_sum(s["v2"], moved), ref2, c2, al2)
    _rejects(K.cmp_tensor, "boundary", R.rows_sum(s["v1"], moved), ref1, c1)
    # pw_sums: the ragged last block's 15 masked rows summed (clamped to the last row); a workgroup walking with the wrong stride; zero rows not zero
    m, n = 2225, 256
    p = K.pw_sums_case(m, n)
    nwg = K.pw_sums_nwg(m, n, K.stats_rows(m), 256, 3)
    blocks = K.pw_sums_blocks(m, nwg)
    cap = K.CAPS["pw_sums"]
    for what, r in p["ref"].items():
        a1 = R.blocks_sum(r.get("allow1", np.zeros(r["v1"].shape)), blocks)
        r1, r2, a2 = R.blocks_sum(r["v1"], blocks), R.blocks_sum(r["v2"], blocks), R.blocks_sum(r["allow2"], blocks)
        owner = [i for i, bl in enumerate(blocks) if 69 in bl][0]
        for ref, al, v in ((r1, a1, r["v1"]), (r2, a2, r["v2"])):
            K.cmp_tensor(what, ref, ref, cap, al)
            tail = ref.copy()
            tail[:, owner] += 15 * v[-1]
            _rejects(K.cmp_tensor, what + " tail", tail, ref, cap, al)
            wrong = R.blocks_sum(v, [[b for wave in range(4) for b in range(wg * 4 + wave, 70, 4 * nwg + 4)] for wg in range(nwg)])
            _rejects(K.cmp_tensor, what + " walk", wrong, ref, cap, al)
    lay = np.concatenate([K.kernel_layout(np.stack([r1, r2], axis=2)), np.zeros((n, K.stats_rows(m) - 2 * nwg, 2))], axis=1)
    K.part_rows("pw_sums", lay, nwg)
    lay[5, 2 * nwg, 0] = 1e-3
    _rejects(K.part_rows, "pw_sums", lay, nwg)


def test_comparisons_reject_a_wrong_apply_and_weight_gradient():
    m, c, k = M_BITE, 256, 64
    o = K.bnwg_case(m, c, k, 4)
    r = R.bn_bwd_apply_wgrad(o["g"], o["z"], o["bits"], 4, o["gamma"], o["mean"], o["invstd"], None, None, o["dgamma"], o["dbeta"])
    K.cmp_elem("dz", r["dz"], r["dz_exact"], r["A_dz"])
    _rejects(K.cmp_elem, "dz", _row_from_next_chunk(r["dz"], 7), r["dz_exact"], r["A_dz"])
    _rejects(K.cmp_elem, "dz", _swap_units(r["dz"], 7), r["dz_exact"], r["A_dz"])
    bad = R.bn_bwd_apply_wgrad(o["g"], o["z"], _neighbour_bits(o["bits"]), 4, o["gamma"], o["mean"], o["invstd"], None, None, o["dgamma"], o["dbeta"])
    _rejects(K.cmp_elem, "dz", bad["dz"], r["dz_exact"], r["A_dz"])
    _rejects(K.cmp_elem, "dz", E.rnd(r["dz"] * (1 + 2.0 ** -6), "bf16"), r["dz_exact"], r["A_dz"])          # two bf16 ulps off
    nan = r["dz"].copy()
    nan[m - 1, c - 1] = np.nan
    _rejects(K.cmp_elem, "dz", nan, r["dz_exact"], r["A_dz"])
    b, e = K.split_bounds(m, K.bnwg_plan(m, c, k, 1, 4, wgs=256)[1])[0]
    ref = R.wgrad(r["dz"], o["x"], (b, e))[0]
    K.cmp_tensor("slab", ref, ref, 2e-6)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], o["x"], (b, e + 17))[0], ref, 2e-6)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], o["x"], (b + 64, e + 64))[0], ref, 2e-6)
    _rejects(K.cmp_tensor, "slab", R.wgrad(r["dz"], _swap_units(o["x"], 9), (b, e))[0], ref, 2e-6)
    _rejects(K.cmp_tensor, "slab", R.wgrad(_row_from_next_chunk(r["dz"], 9), o["x"], (b, e))[0], ref, 2e-6)
    _rejects(K.cmp_tensor, "slab", ref * (1 + 4e-6), ref, 2e-6)
    # mask mode 2: the gate of the neighbouring channel
    o2 = K.bnwg_case(m, 64, 256, 2)
    r2 = R.bn_bwd_apply_wgrad(o2["g"], o2["z"], None, 2, o2["gamma"], o2["mean"], o2["invstd"], o2["scale"], o2["shift"], o2["dgamma"], o2["dbeta"])
    gate = (o2["scale"][None, :] * o2["z"] + o2["shift"][None, :]) > 0
    f = lambda t: t[None, :]          # noqa: E731
    wrong = f(o2["gamma"] * o2["invstd"]) * (np.where(np.roll(gate, -1, axis=1), o2["g"], 0.0) - f(o2["dbeta"]) / m - r2["xhat"] * f(o2["dgamma"]) / m)
    _rejects(K.cmp_elem, "dz", E.rnd(wrong, "bf16"), r2["dz_exact"], r2["A_dz"])
