"""CPU: tests/conv_epilogue_ref.py (the fp64 reference the GPU epilogue tests compare with) against torch autograd in double, one small shape each.
With the z3 rounding switched off and fp32 "storage" (whose rounding is far below the bounds used here) the reference must BE the calculus it documents."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_epilogue_ref as R


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def test_bit_packing_against_a_hand_written_byte():
    # channels 0..7 of one row: on, off, off, on | off, on, on, on  ->  byte 0 = 0b1001 = 9, byte 1 = 0b1110 = 14
    mask = np.array([[1, 0, 0, 1, 0, 1, 1, 1]], dtype=bool)
    assert R.pack_bits(mask).tolist() == [[9, 14]]
    assert R.unpack_bits(np.array([[9, 14]], dtype=np.uint8), 8).tolist() == [[1, 0, 0, 1, 0, 1, 1, 1]]
    # only the low four bits of a byte gate anything
    assert R.unpack_bits(np.array([[0xF0 | 2]], dtype=np.uint8), 4).tolist() == [[0, 1, 0, 0]]
    rng = np.random.default_rng(0)
    m = rng.random((37, 24)) > 0.5
    assert np.array_equal(R.unpack_bits(R.pack_bits(m), 24) > 0, m)


def test_rounding_and_ulp_of_the_storage_types():
    a = np.array([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0, 0.1])
    assert R.rnd(a, "bf16").tolist() == [1.0, 1.0 + 2.0 ** -7, -3.0, float(torch.tensor(0.1).bfloat16())]
    assert R.ulp(np.array([1.0, 1.5, 2.0, -0.75]), "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]
    assert R.ulp(np.array([1.0, -0.75]), "f32").tolist() == [2.0 ** -23, 2.0 ** -24]


def test_partial_rows_are_channel_major_per_128_rows_and_parity_classes_follow_each_other():
    n, ho, wo, c = 3, 9, 7, 4                                     # M = 189: partial 0 = rows 0..127, partial 1 = rows 128..188
    v = np.arange(n * ho * wo * c, dtype=np.float64).reshape(-1, c)
    p = R.partials(R.row_runs(n, ho, wo), v, v * v)
    assert p.shape == (c, 2, 2) and R.stats_rows(n, ho, wo) == 2
    assert p[1, 0, 0] == v[:128, 1].sum() and p[1, 1, 0] == v[128:, 1].sum() and p[3, 1, 1] == (v[128:, 3] ** 2).sum()
    # in_dil = 2: classes (0,0), (0,1), (1,0), (1,1), each (image, oh, ow) ordered, each with its own ragged last partial
    runs = R.row_runs(n, ho, wo, 2)
    assert [len(r) for r in runs] == [3 * 5 * 4, 3 * 5 * 3, 3 * 4 * 4, 3 * 4 * 3]
    assert runs[1][:4].tolist() == [1, 3, 5, 2 * wo + 1] and runs[2][0] == wo and runs[3][0] == wo + 1
    assert R.stats_rows(n, ho, wo, 2) == 4
    n2, h2 = 8, 15                                                # 8 * 8 * 8 = 512 rows in class (0,0): four partials, then (0,1) with 448
    assert R.stats_rows(n2, h2, h2, 2) == 4 + 4 + 4 + 4 and len(R.row_runs(n2, h2, h2, 2)[3]) == 8 * 7 * 7
    p2 = R.partials(R.row_runs(n, ho, wo, 2), v, v)
    assert p2.shape == (c, 4, 2) and p2[0, 1, 0] == v[runs[1], 0].sum()


def test_strided_data_gradient_equals_conv_transpose2d():
    rng = np.random.default_rng(1)
    for (n, h, w, ci, co, k, s, p) in [(2, 13, 11, 8, 12, 3, 2, 1), (1, 14, 12, 8, 4, 3, 2, 1), (2, 15, 15, 8, 8, 1, 2, 0), (2, 6, 5, 4, 8, 3, 1, 1)]:
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        dz = rng.standard_normal((n, ho, wo, co))
        wt = rng.standard_normal((co, ci, k, k))
        oph, opw = h - ((ho - 1) * s - 2 * p + k), w - ((wo - 1) * s - 2 * p + k)
        want = F.conv_transpose2d(_t(dz).permute(0, 3, 1, 2), _t(wt), stride=s, padding=p, output_padding=(oph, opw)).permute(0, 2, 3, 1).reshape(-1, ci).numpy()
        got = R.conv(dz, R.pack_dgrad(wt), stride=1, pad=k - 1 - p, in_dil=s if s > 1 else 1, ho=h, wo=w)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
        assert R.out_size(ho, k, 1, k - 1 - p, s) >= h


def test_forward_conv_equals_torch_on_the_packed_weights():
    rng = np.random.default_rng(2)
    x, wt = rng.standard_normal((2, 7, 9, 8)), rng.standard_normal((12, 8, 3, 3))
    want = F.conv2d(_t(x).permute(0, 3, 1, 2), _t(wt), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, 12).numpy()
    got = R.conv(x, wt.transpose(0, 2, 3, 1), stride=2, pad=1)
    assert np.abs(got - want).max() < 1e-12
    z, part = R.fwd_stats(x, wt.transpose(0, 2, 3, 1), "f32", shift=np.full(12, 0.25), stride=2, pad=1)
    assert np.abs(part[:, :, 0].sum(1) - (z - 0.25).sum(0)).max() < 1e-12 and np.abs(part[:, :, 1].sum(1) - ((z - 0.25) ** 2).sum(0)).max() < 1e-12


def test_modes_9_and_10_equal_autograd_of_relu_bn_conv_plus_identity():
    rng = np.random.default_rng(3)
    n, h, w, cin, cout, eps = 3, 6, 6, 8, 12, 1e-5
    x, wt = rng.standard_normal((n, h, w, cin)), rng.standard_normal((cout, cin, 1, 1)) * 0.3
    gamma, beta = rng.random(cout) + 0.5, rng.standard_normal(cout) * 0.3
    ident, gout = rng.standard_normal((n * h * w, cout)), rng.standard_normal((n * h * w, cout))
    z3 = F.conv2d(_t(x).permute(0, 3, 1, 2), _t(wt)).permute(0, 2, 3, 1).reshape(-1, cout).requires_grad_(True)
    gt, bt = _t(gamma).requires_grad_(True), _t(beta).requires_grad_(True)
    out = F.relu(F.batch_norm(z3, None, None, gt, bt, training=True, eps=eps) + _t(ident))
    (out * _t(gout)).sum().backward()
    mean = z3.detach().mean(0).numpy()
    invstd = 1.0 / np.sqrt(z3.detach().var(0, unbiased=False).numpy() + eps)
    wp = wt.transpose(0, 2, 3, 1)
    # the forward the sign bits come from: the BatchNorm-apply epilogue with the folded coefficients
    scale = gamma * invstd
    ap = R.fwd_bnapply(x, wp, "f32", scale, beta - mean * scale, ident, round_z3=False)
    assert np.abs(ap["out"] - out.detach().numpy()).max() < 1e-6          # (fp32 "storage")
    assert np.array_equal(R.unpack_bits(ap["bits"], cout) > 0, out.detach().numpy() > 0)
    s = R.fwd_bnbwd(x, wp, "f32", gout, ap["bits"], mean, invstd, round_z3=False)["sums"]
    dbeta, dgamma = s[:, :, 0].sum(1), s[:, :, 1].sum(1)
    assert np.abs(dbeta - bt.grad.numpy()).max() < 1e-10 and np.abs(dgamma - gt.grad.numpy()).max() < 1e-10
    r = R.fwd_bnbwd(x, wp, "f32", gout, ap["bits"], mean, invstd, gamma, dgamma, dbeta, round_z3=False)
    assert np.abs(r["dz_exact"] - z3.grad.numpy()).max() < 1e-10
    # a downsample branch's BatchNorm on the residual operand
    rs, rb = rng.random(cout) + 0.5, rng.standard_normal(cout)
    ap2 = R.fwd_bnapply(x, wp, "f32", scale, beta - mean * scale, ident, rs, rb, round_z3=False)
    assert np.abs(ap2["t"] - (scale * z3.detach().numpy() + (beta - mean * scale) + rs * ident + rb)).max() < 1e-12
    # the ulp probe moves z3 by exactly one storage ulp
    r1 = R.fwd_bnbwd(x, wp, "bf16", gout, ap["bits"], mean, invstd, z3_ulps=1)
    r0 = R.fwd_bnbwd(x, wp, "bf16", gout, ap["bits"], mean, invstd)
    assert np.array_equal(r1["z3"] - r0["z3"], R.ulp(r0["z3"], "bf16")) and np.array_equal(R.rnd(r0["z3"], "bf16"), r0["z3"])


def test_epilogue_6_sums_equal_autograd_of_relu_bn():
    rng = np.random.default_rng(4)
    n, h, w, cf, ci, eps = 2, 7, 5, 8, 12, 1e-5                   # forward conv ci -> cf (3x3, stride 1); its data gradient maps dz [.., cf] to [.., ci]
    dz, wt = rng.standard_normal((n, h, w, cf)), rng.standard_normal((cf, ci, 3, 3)) * 0.2
    z = rng.standard_normal((n * h * w, ci))                      # the pre-activation of the ReLU(BN(.)) whose output the forward conv read
    gamma, beta = rng.random(ci) + 0.5, rng.standard_normal(ci) * 0.3
    zt, gt, bt = _t(z).requires_grad_(True), _t(gamma).requires_grad_(True), _t(beta).requires_grad_(True)
    a = F.relu(F.batch_norm(zt, None, None, gt, bt, training=True, eps=eps))
    mean, invstd = z.mean(0), 1.0 / np.sqrt(z.var(0) + eps)
    scale = gamma * invstd
    y, part = R.dgrad_bnsums(dz, R.pack_dgrad(wt), "f32", z, mean, invstd, scale, beta - mean * scale, stride=1, pad=1)
    want_y = F.conv_transpose2d(_t(dz).permute(0, 3, 1, 2), _t(wt), padding=1).permute(0, 2, 3, 1).reshape(-1, ci).numpy()
    assert np.abs(y - want_y).max() < 1e-5
    (a * _t(y)).sum().backward()                                  # y (as stored) is the gradient arriving at a
    assert np.abs(part[:, :, 0].sum(1) - bt.grad.numpy()).max() < 1e-10 and np.abs(part[:, :, 1].sum(1) - gt.grad.numpy()).max() < 1e-10
    assert R.gate_margin(z, scale, beta - mean * scale).shape == z.shape


def test_residual_gates_and_res_c0():
    rng = np.random.default_rng(5)
    n, h, w, cin, cout, c0 = 1, 3, 3, 4, 16, 8
    x, wp = rng.standard_normal((n, h, w, cin)), rng.standard_normal((cout, 1, 1, cin))
    res = rng.standard_normal((n * h * w, cout))
    rb, og = rng.integers(0, 16, (n * h * w, cout // 4)).astype(np.uint8), rng.integers(0, 16, (n * h * w, cout // 4)).astype(np.uint8)
    acc = R.conv(x, wp)
    y, part = R.fwd_resmask(x, wp, "f32", res, rb, og, res_c0=c0, colsums=True)
    m_r, m_o = R.unpack_bits(rb, cout), R.unpack_bits(og, cout)
    want = acc.copy()
    want[:, c0:] = (acc[:, c0:] + res[:, c0:] * m_r[:, c0:]) * m_o[:, c0:]       # below res_c0: no residual, no output gate
    assert np.abs(y - want).max() < 1e-6
    assert np.abs(part[:, 0, 0] - y.sum(0)).max() < 1e-12 and np.abs(part[:, 0, 1] - (y * y).sum(0)).max() < 1e-12
    y0 = R.fwd_resmask(x, wp, "f32", res, None, None, res_c0=0)
    assert np.abs(y0 - (acc + res)).max() < 1e-6
