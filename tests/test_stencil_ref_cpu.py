"""CPU: tests/stencil_ref.py (the fp64 reference tests/test_stencil_variants_gpu.py compares the MVF stencil and tap-gradient kernels with) against
oracle/mvf_numpy.py -- the restatement of the reference module that tests/test_oracle_golden.py pins to the golden vectors -- over every MVF golden case
with a slice (modes T / TH / THW, shared taps, T = 1, H = W = 1), and its addend / gate terms against explicit masked arithmetic.
Bound 1e-12: both sides sum the same fp64 products, in another order."""
import numpy as np
import pytest

import stencil_ref as R
from cases import MVF_CASES
from helpers import rel_err
from oracle import mvf_numpy as O

CASES = [c for c in MVF_CASES if int(c[3] * c[6])]
MODE_BITS = {"T": 1, "TH": 3, "THW": 7}
assert {c[7] for c in CASES} == {"T", "TH", "THW"} and any(c[8] for c in CASES) and any(c[2] == 1 for c in CASES) and any(c[4] == c[5] == 1 for c in CASES)


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1, a.shape[1])


def _setup(case):
    name, N, T, C, H, W, alpha, mode, share, use_hs, planes = case
    cs = int(C * alpha)
    rng = np.random.default_rng(len(name) + N * T * C * H * W)
    x = rng.standard_normal((N * T, C, H, W))
    wt, wh, ww = (rng.uniform(-1, 1, (cs, 3)) for _ in range(3))
    d = R.Desc(N * T, H, W, T, cs, MODE_BITS[mode])
    # the kernels' view of shared taps: one tap pointer three times
    taps = (wt, wt, wt) if share else (wt, wh if mode in ("TH", "THW") else None, ww if mode == "THW" else None)
    return x, d, (wt, wh, ww), taps, rng


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_plain_stencil_and_its_transpose_equal_the_oracle(case):
    name, N, T, C, H, W, alpha, mode, share, use_hs, planes = case
    x, d, (wt, wh, ww), taps, rng = _setup(case)
    out, cache, _ = O.mvf_forward(x, T, d.cs, wt, wh, ww, mode=mode, share=share, use_hs=False)
    y, A = R.stencil(_nhwc(x), d, *taps)
    assert y.shape == A.shape == (d.nt * H * W, d.cs)
    assert rel_err(y, _nhwc(out)[:, :d.cs]) < 1e-12
    assert (A >= np.abs(y) - 1e-12).all()
    yabs, _ = R.stencil(np.abs(_nhwc(x)), d, *[None if t is None else np.abs(t) for t in taps])
    assert rel_err(A, yabs) < 1e-12
    # the data gradient of the views = the stencil with reversed taps (flip = 1) on the gradient
    g = rng.standard_normal(x.shape)
    r = O.mvf_backward(g, cache)
    dx, _ = R.stencil(_nhwc(g), d, *taps, flip=1)
    assert rel_err(dx, _nhwc(r["dx"])[:, :d.cs]) < 1e-12
    # tap gradients; with shared taps the oracle sums the three views into dwt
    dwt, dwh, dww = R.tapgrad(_nhwc(x), _nhwc(g), d)
    if share:
        assert rel_err(dwt + dwh + dww, r["dwt"]) < 1e-12
    else:
        assert rel_err(dwt, r["dwt"]) < 1e-12
        for got, ref, bit in ((dwh, r["dwh"], R.VIEW_H), (dww, r["dww"], R.VIEW_W)):
            assert rel_err(got, ref) < 1e-12
            if not d.mode & bit:
                assert not got.any()
    # the centre tap is the same sum in every present view
    for got, bit in ((dwh, R.VIEW_H), (dww, R.VIEW_W)):
        if d.mode & bit:
            assert (got[:, 1] == dwt[:, 1]).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_scale_shift_hard_swish_form_equals_the_oracle_with_eval_mode_batchnorm(case):
    name, N, T, C, H, W, alpha, mode, share, use_hs, planes = case
    x, d, (wt, wh, ww), taps, rng = _setup(case)
    gamma, beta, mean = rng.uniform(0.5, 1.5, d.cs), rng.standard_normal(d.cs), rng.standard_normal(d.cs)
    var = rng.uniform(0.5, 2.0, d.cs)
    out, _, _ = O.mvf_forward(x, T, d.cs, wt, wh, ww, mode=mode, share=share, use_hs=True, gamma=gamma, beta=beta, running_mean=mean, running_var=var,
                              training=False)
    scale = gamma / np.sqrt(var + O.EPS)
    shift = beta - mean * scale
    y, A = R.stencil(_nhwc(x), d, *taps, scale=scale, shift=shift)
    assert rel_err(y, _nhwc(out)[:, :d.cs]) < 1e-12
    assert (A >= np.abs(y) - 1e-12).all()               # |hswish(u)| <= |u| <= |scale| A_v + |shift|


def test_addend_and_gates_equal_explicit_masked_arithmetic():
    d = R.Desc(8, 3, 5, 4, 8, 7)
    m = d.nt * d.h * d.w
    rng = np.random.default_rng(5)
    x = rng.standard_normal((m, 12))
    taps = [rng.uniform(-1, 1, (d.cs, 3)) for _ in range(3)]
    add = rng.standard_normal((m, 16))
    abits = rng.integers(0, 256, (m, 4), dtype=np.uint8)          # pitch 16 / 4
    gbits = rng.integers(0, 256, (m, 3), dtype=np.uint8)          # pitch 12 / 4
    plain, A0 = R.stencil(x, d, *taps, flip=1)
    on_a = np.zeros((m, d.cs))
    on_g = np.zeros((m, d.cs))
    for p in range(m):
        for c in range(d.cs):
            on_a[p, c] = (int(abits[p, c // 4]) >> (c % 4)) & 1
            on_g[p, c] = (int(gbits[p, c // 4]) >> (c % 4)) & 1
    assert 0.3 < on_a.mean() < 0.7 and 0.3 < on_g.mean() < 0.7
    assert (R.unpack_bits(abits, d.cs) == on_a).all()
    y, A = R.stencil(x, d, *taps, flip=1, addend=add, addend_c=16)
    assert np.array_equal(y, plain + add[:, :8]) and np.array_equal(A, A0 + np.abs(add[:, :8]))
    y, A = R.stencil(x, d, *taps, flip=1, addend=add, addend_c=16, addend_bits=abits)
    assert np.array_equal(y, plain + add[:, :8] * on_a) and np.array_equal(A, A0 + np.abs(add[:, :8]) * on_a)
    y, A = R.stencil(x, d, *taps, flip=1, addend=add, addend_c=16, addend_bits=abits, out_gate_bits=gbits)
    assert np.array_equal(y, (plain + add[:, :8] * on_a) * on_g) and np.array_equal(A, (A0 + np.abs(add[:, :8]) * on_a) * on_g)
    y, _ = R.stencil(x, d, *taps, out_gate_bits=gbits)
    assert np.array_equal(y, R.stencil(x, d, *taps)[0] * on_g)
    with pytest.raises(AssertionError):
        R.stencil(x, d, *taps, addend_bits=abits)                # bits without an addend


def test_statistics_are_the_shifted_sums():
    rng = np.random.default_rng(9)
    y = rng.standard_normal((37, 5))
    K = rng.standard_normal(5)
    s1, s2 = R.stats(y, K)
    for c in range(5):
        assert abs(s1[c] - sum(y[p, c] - K[c] for p in range(37))) < 1e-12
        assert abs(s2[c] - sum((y[p, c] - K[c]) ** 2 for p in range(37))) < 1e-12
    s1, s2 = R.stats(y)
    assert rel_err(s1, y.sum(0)) < 1e-12 and rel_err(s2, (y * y).sum(0)) < 1e-12
