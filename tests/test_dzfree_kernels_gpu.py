"""GPU: each of the four glue kernels of csrc/bn_dzfree.hip ALONE, through the C ABI, against the independent fp64 reference tests/dzfree_ref.py (proved against
torch float64 autograd in tests/test_dzfree_ref_cpu.py) -- mvf_bn_bwd_dzfree_prep, mvf_bn_bwd_dzfree_wgrad, mvf_bn_bwd_dzfree_sums and mvf_bn_train_stats_gram
at the smallest shapes that reach each of their code paths (tests/dzfree_cases.py says which).  No producer kernel runs: A2, a_mean, Q, the partial column
sums, dgamma and dbeta are made on the host in fp64 and rounded once.  Only mvf_pack_conv_weight_dgrad is called, and its output must equal the host's W^T.

Conventions (those of test_bn_pool_kernels_gpu.py): every output is exactly sized, NaN before the call, with a 4 KiB canary behind it that must come back
unchanged; every element must have been written; m is passed as given, m = 1 included.

Bounds, per element, from the arithmetic (U = 2^-24; A = the sum of the absolute values of the terms of the element's expression, from the reference):
  prep, scaling part  bd[k][c'] = bf16(fl(fl(gamma invstd) wd)): |got - ref| <= 2^-8 |ref| AND the bits of a numpy float32 restatement
  prep, G part        2^-8 |ref| + (2^-8 + C U) A: one bf16 rounding of each scaled operand, fp32 accumulation over C channels, one output rounding
  prep, bias          8 U A ceil(C / 512)
  wgrad               8 U A + 2^-16 |a kx| sum_j |W[c][j] A2[j][k]| (the two-term bf16 split of A2 keeps 16 bits); the reference is fed the kernel's inputs
  sums                dbeta 8 U sum |part|, dgamma 8 U A
  gram_stats          save_mean 8 U A; the variance read back as 1 / invstd^2 - eps, and running_var: 8 U A_var (A_var = sum_jk |W_cj| (|A2_jk| / m +
                      |abar_j abar_k|) |W_ck| carries the conditioning of the uncentred form; running_var adds its own term |(1 - momentum) running_var| and
                      the factors momentum m / (m - 1)); scale to 4 U of gamma x the kernel's own invstd, shift to 4 U (|beta| + |mean scale|) from the
                      kernel's own mean and scale; a zero weight row: mean 0, variance 0 exactly (running_var at momentum 1 is 0), invstd = 1 / sqrt(eps)
  lattice families    dyadic inputs (exactness proved on the CPU): every output equals the reference EXACTLY (signed zeros equal); bd through its one bf16
                      rounding of the exact sum
  composed (host)     [gm | a2] bd_gpu^T + bias_gpu against dz3 W, and the corrected dW_gpu against dz3^T a2, in fp64, bounded by the elementwise bounds
                      propagated through the product (+ U A for the fp32 rounding of Q, A2 and a_mean on the way in)
  reduced quantities  the rel_l2 of every 32 x 32 block of G and of each output vector against fp64: dzfree_cases.bound (4 x the largest measured figure,
                      profiles/dzfree_errors.txt; MVF_DZFREE_ERRORS=file dumps them, tools/dzfree_errors_table.py)
No element is excluded anywhere."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import dzfree_cases as K
import dzfree_ref as R
from helpers import rel_err, rel_l2

pytestmark = pytest.mark.gpu

ERRORS_ENV = "MVF_DZFREE_ERRORS"          # a file: one JSON line per measured reduced quantity (tooling: profiles/dzfree_errors.txt)
CANARY = 4096
U = 2.0 ** -24
EINVAL, ESHAPE, EUNSUPPORTED = -1, -2, -5
BF = torch.bfloat16


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class _Out(object):
    """An exactly-sized buffer of NaN (every byte 0xFF) with a canary behind it; `t` is the tensor the kernel writes."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape)) * (2 if dtype == BF else 4)
        self.raw = torch.empty(n + CANARY, dtype=torch.uint8, device="cuda")
        self.raw[:n] = 0xFF
        self.raw[n:] = 0xA5
        self.t = self.raw[:n].view(dtype).view(shape)
        self.n = n
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64)).to(dtype))

    def check(self, what=""):
        torch.cuda.synchronize()
        assert bool((self.raw[self.n:] == 0xA5).all()), "%s: written past the end of an exactly-sized output" % what

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw[:self.n] == 0xFF).all())


def _bf(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(BF).cuda()


def _f(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float().cuda()


def _np(t):
    return t.double().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _elem(case, what, got, ref, tol):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s %s: %d of %d elements are not finite (never written?)" % (case, what, int((~np.isfinite(got)).sum()), got.size)
    tol = np.broadcast_to(tol, ref.shape)
    bad = np.abs(got - ref) > tol
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.abs(got - ref) / np.maximum(tol, 1e-300), 0)), got.shape)
        raise AssertionError("%s %s: %d of %d elements beyond the bound; worst at %s: got %.9g, ref %.9g, bound %.3g" % (case, what, int(bad.sum()), got.size, i, got[i], ref[i],
                                                                                                                   tol[i]))


def _exact(case, what, got, ref):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), (case, what)
    bad = got != ref                                                            # (-0.0 == 0.0)
    if bad.any():
        i = np.unravel_index(np.argmax(bad), got.shape)
        raise AssertionError("%s %s: %d of %d elements differ from the exact result; first at %s: got %.9g, exact %.9g" % (case, what, int(bad.sum()), got.size, i, got[i], ref[i]))


def _reduced(case, q, got, ref, late=None):
    """rel_l2 (and rel_err, for the table) of a reduced quantity against the fp64 reference: printed, dumped, asserted <= dzfree_cases.bound(q).  late: a list
    that takes the message of a miss instead, for a caller that asserts it empty after ALL its checks have run."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), "%s %s: not finite" % (case, q)
    l2, e, b = rel_l2(got, ref), rel_err(got, ref), K.bound(q)
    if os.environ.get(ERRORS_ENV):
        with open(os.environ[ERRORS_ENV], "a") as f_:
            f_.write(json.dumps(dict(case=case, quantity=q, rel_l2=l2, rel_err=e, bound=b)) + "\n")
    print("%s %s: rel_l2 %.3g rel_err %.3g (bound %.3g)" % (case, q, l2, e, b))
    msg = "%s %s: rel_l2 %.3g against fp64, bound %.3g" % (case, q, l2, b)
    if late is not None and l2 > b:
        late.append(msg)
        return
    assert l2 <= b, msg


def _bn(o):
    return [_f(o[q]) for q in ("gamma", "mean", "invstd", "dgamma", "dbeta")]


# ------------------------------------------------------------------------------------------------ mvf_bn_bwd_dzfree_prep
def _run_prep(o, case):
    lib = _lib()
    c, k, m = o["c"], o["k"], o["m"]
    # the operand: the library's data-gradient pack of the fp32 weights IS the host's W^T
    w32, wd_lib = _f(o["w"]), torch.empty(k, c, device="cuda", dtype=BF)
    assert lib.mvf_pack_conv_weight_dgrad(P(w32), c, k, 1, 1, P(wd_lib), 1, None) == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(wd_lib), K.bf16_bits(o["wd"])), "%s: mvf_pack_conv_weight_dgrad is not the transpose of the bf16 weights" % case
    wd = _bf(o["wd"])
    bd, bias = _Out((k, c + k), BF), _Out((k,))
    par = _bn(o)
    rc = lib.mvf_bn_bwd_dzfree_prep(P(wd), c, k, *[P(t) for t in par], m, P(bd.t), P(bias.t), 1, None)
    assert rc == 0, "%s: %d %s" % (case, rc, lib.mvf_last_error())
    bd.check(case)
    bias.check(case)
    got = _np(bd.t)
    assert np.isfinite(got).all(), "%s: %d elements of bd were never written" % (case, int((~np.isfinite(got)).sum()))
    return got, _bits(bd.t), _np(bias.t)


def _prep_bounds(o, ref):
    c = o["c"]
    tol_scale = 2.0 ** -8 * np.abs(ref["bd"][:, :c])
    tol_g = 2.0 ** -8 * np.abs(ref["bd"][:, c:]) + (2.0 ** -8 + c * U) * ref["A_G"]
    tol_bias = 8 * U * ref["A_bias"] * math.ceil(c / 512.0)
    return tol_scale, tol_g, tol_bias


def _check_prep(o, case, composed=True):
    c, k, m = o["c"], o["k"], o["m"]
    got, bits, bias = _run_prep(o, case)
    ref = R.prep(o["wd"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], m)
    tol_scale, tol_g, tol_bias = _prep_bounds(o, ref)
    _elem(case, "bd, scaling part", got[:, :c], ref["bd"][:, :c], tol_scale)
    want_bits = K.scaling_restatement(o)
    assert np.array_equal(bits[:, :c], want_bits), "%s: %d of %d bf16 patterns of the scaling part differ from bf16(fl(fl(gamma invstd) wd))" % (
        case, int((bits[:, :c] != want_bits).sum()), want_bits.size)
    _elem(case, "bd, G part", got[:, c:], ref["bd"][:, c:], tol_g)
    _elem(case, "bias", bias, ref["bias"], tol_bias)
    if ref["A_G"].any():
        for j0 in range(0, k, 32):
            for k0 in range(0, k, 32):
                _reduced("%s block(%d,%d)" % (case, k0 // 32, j0 // 32), "G_block", got[k0:k0 + 32, c + j0:c + j0 + 32], ref["bd"][k0:k0 + 32, c + j0:c + j0 + 32])
        _reduced(case, "bias", bias, ref["bias"])
    if composed:
        x = np.concatenate([o["gm"], o["a2"]], axis=1)
        da, want = x @ got.T + bias, o["dz3"] @ o["w"]
        tol = np.abs(x) @ np.concatenate([tol_scale, tol_g], axis=1).T + tol_bias + 1e-13 * (np.abs(x) @ np.abs(ref["bd"]).T + np.abs(ref["bias"]))
        _elem(case, "[gm | a2] bd^T + bias against dz3 W", da, want, tol)
    return got, bits, bias, ref


def _prep_params():
    return [pytest.param(c, k, m, id="c%d_k%d_m%d" % (c, k, m)) for c, k in K.PREP_SHAPES for m in K.PREP_ROWS.get((c, k), (37,))]


@pytest.mark.parametrize("c,k,m", _prep_params())
def test_prep_operand_and_bias(c, k, m):
    """[a.W ; -G] and the bias per element, the G blocks in rel_l2, and the data gradient they stand for -- from one trip per wave to the 64 KiB LDS bound."""
    _check_prep(K.triple(m, c, k), "prep_c%d_k%d_m%d" % (c, k, m))


def test_prep_with_frozen_statistics():
    """dgamma = dbeta = 0 (the engine passes them for a BatchNorm with frozen statistics): G and the bias are zero, of either sign, bd[:, :c] is a.W."""
    o = K.frozen(K.triple(37, 512, 64))
    got, bits, bias, _ = _check_prep(o, "prep_frozen_c512_k64")
    assert not got[:, 512:].any() and not bias.any()
    assert np.array_equal(bits[:, :512], K.scaling_restatement(o))


def test_prep_lattice_is_exact():
    """Dyadic inputs (three trips, nine blocks): all of bd -- through its single bf16 rounding of the exact sum -- and the bias bit for bit: every fragment
    index, block placement and the wave-quarter sum."""
    o = K.lattice_prep()
    got, bits, bias = _run_prep(o, "prep_lattice")
    ref = R.prep(o["wd"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"])
    _exact("prep_lattice", "bd", got, R.round_bf16(ref["bd"]))
    _exact("prep_lattice", "bias", bias, ref["bias"])


# ------------------------------------------------------------------------------------------------ mvf_bn_bwd_dzfree_wgrad
def _run_wgrad(o, case):
    lib = _lib()
    c, k, m = o["c"], o["k"], o["m"]
    dw = _Out((c, k), init=o["q"])
    w, gram, am = _bf(o["w"]), _f(o["gram"]), _f(o["a_mean"])
    par = _bn(o)
    rc = lib.mvf_bn_bwd_dzfree_wgrad(P(dw.t), P(w), P(gram), P(am), *[P(t) for t in par], m, c, k, 1, None)
    assert rc == 0, "%s: %d %s" % (case, rc, lib.mvf_last_error())
    dw.check(case)
    return _np(dw.t)


def _check_wgrad(o, case):
    got = _run_wgrad(o, case)
    ref = R.wgrad_fix(o["q"], o["w"], o["gram"], o["a_mean"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"])
    tol = 8 * U * ref["A"] + 2.0 ** -16 * ref["split"]
    _elem(case, "dW", got, ref["dw"], tol)
    if o["m"] > 1:                                    # (one row: dz3 = 0 identically, dW is the rounding of a complete cancellation -- the elementwise bound is the statement)
        _reduced(case, "dw", got, ref["dw"])
    _elem(case, "dW against dz3^T a2", got, o["dz3"].T @ o["a2"], tol + U * ref["A"])
    return got, ref


def _wgrad_params():
    return [pytest.param(c, k, m, id="c%d_k%d_m%d" % (c, k, m)) for c, k in K.WGRAD_SHAPES for m in K.WGRAD_ROWS.get((c, k), (37,))]


@pytest.mark.parametrize("c,k,m", _wgrad_params())
def test_wgrad_correction(c, k, m):
    """Q -> dW in place, per element and against dz3^T a2: idle waves, a ragged last workgroup, one and three trips."""
    _check_wgrad(K.triple(m, c, k), "wgrad_c%d_k%d_m%d" % (c, k, m))


def test_wgrad_with_frozen_statistics():
    """dgamma = dbeta = 0: the correction is a . Q, one fp32 product per element -- the bits."""
    o = K.frozen(K.triple(37, 96, 64))
    got, _ = _check_wgrad(o, "wgrad_frozen_c96_k64")
    a = np.float32(o["gamma"]) * np.float32(o["invstd"])
    _exact("wgrad_frozen_c96_k64", "dW = a . Q", got, (a[:, None] * np.float32(o["q"])).astype(np.float64))


def test_wgrad_lattice_is_exact():
    """Dyadic inputs, A2 of 11 bits (hi + lo), three trips: the corrected dW bit for bit."""
    o = K.lattice_wgrad()
    got = _run_wgrad(o, "wgrad_lattice")
    ref = R.wgrad_fix(o["q"], o["w"], o["gram"], o["a_mean"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], o["m"])
    _exact("wgrad_lattice", "dW", got, ref["dw"])


# ------------------------------------------------------------------------------------------------ mvf_bn_bwd_dzfree_sums
def _run_sums(o, lo, rows_lo, c_split, hi, rows_hi, case):
    lib = _lib()
    c, k = o["c"], o["k"]
    dg, db = _Out((c,)), _Out((c,))
    q, w, mean, invstd, plo, phi = _f(o["q"]), _bf(o["w"]), _f(o["mean"]), _f(o["invstd"]), _f(lo), _f(hi)
    assert plo is None or plo.shape == (c_split, rows_lo, 2)
    rc = lib.mvf_bn_bwd_dzfree_sums(P(q), P(w), c, k, P(mean), P(invstd), P(plo), rows_lo, c_split, P(phi), rows_hi, P(dg.t), P(db.t), 1, None)
    assert rc == 0, "%s: %d %s" % (case, rc, lib.mvf_last_error())
    dg.check(case)
    db.check(case)
    return _np(dg.t), _np(db.t)


@pytest.mark.parametrize("k", K.SUMS_K)
@pytest.mark.parametrize("c", K.SUMS_C)
def test_sums_from_q_and_partial_rows(c, k):
    """dgamma / dbeta per channel for every split (none, all, inside a 4-channel workgroup) and row-count pair; element [..][1] of the partial rows and the
    channels of part_hi below the split are NaN: a kernel that reads them says so."""
    o = K.triple(K.SUMS_M, c, k)
    for c_split in K.splits(c):
        for rows_lo, rows_hi in K.SUMS_ROWS:
            case = "sums_c%d_k%d_split%d_rows%d_%d" % (c, k, c_split, rows_lo, rows_hi)
            lo, hi = K.partial_rows(o["gm"], c, c_split, rows_lo, rows_hi, seed=c + k + c_split + rows_lo)
            dg, db = _run_sums(o, lo, rows_lo, c_split, hi, rows_hi, case)
            ref = R.sums(o["q"], o["w"], o["mean"], o["invstd"], lo, rows_lo, c_split, hi, rows_hi)
            _elem(case, "dbeta", db, ref["dbeta"], 8 * U * ref["A_dbeta"])
            _elem(case, "dgamma", dg, ref["dgamma"], 8 * U * ref["A_dgamma"])
            _reduced(case, "dbeta", db, ref["dbeta"])
            _reduced(case, "dgamma", dg, ref["dgamma"])


def test_sums_lattice_is_exact():
    o = K.lattice_sums()
    dg, db = _run_sums(o, o["part_lo"], o["rows_lo"], o["c_split"], o["part_hi"], o["rows_hi"], "sums_lattice")
    ref = R.sums(o["q"], o["w"], o["mean"], o["invstd"], o["part_lo"], o["rows_lo"], o["c_split"], o["part_hi"], o["rows_hi"])
    _exact("sums_lattice", "dbeta", db, ref["dbeta"])
    _exact("sums_lattice", "dgamma", dg, ref["dgamma"])


# ------------------------------------------------------------------------------------------------ mvf_bn_train_stats_gram
RUNNING = (("both", True, True, K.MOMENTUM), ("none", False, False, K.MOMENTUM), ("mean_only", True, False, K.MOMENTUM), ("var_only", False, True, K.MOMENTUM),
           ("both_momentum1", True, True, 1.0))


def _run_gram(o, with_rm, with_rv, momentum, case, eps=K.EPS):
    lib = _lib()
    c, k, m = o["c"], o["k"], o["m"]
    outs = [_Out((c,)) for _ in range(4)]
    rm = _Out((c,), init=o["running_mean"]) if with_rm else None
    rv = _Out((c,), init=o["running_var"]) if with_rv else None
    gram, am, w, gamma, beta = _f(o["gram"]), _f(o["a_mean"]), _bf(o["w"]), _f(o["gamma"]), _f(o["beta"])
    rc = lib.mvf_bn_train_stats_gram(P(gram), P(am), P(w), m, c, k, P(gamma), P(beta), C.c_float(eps), C.c_float(momentum), P(rm.t if rm else None), P(rv.t if rv else None),
                                     *[P(t.t) for t in outs], 1, None)
    assert rc == 0, "%s: %d %s" % (case, rc, lib.mvf_last_error())
    for t in outs + [t for t in (rm, rv) if t is not None]:
        t.check(case)
    res = dict(zip(("mean", "invstd", "scale", "shift"), (_np(t.t) for t in outs)))
    res["running_mean"], res["running_var"] = (_np(rm.t) if rm else None), (_np(rv.t) if rv else None)
    for q, v in res.items():
        assert v is None or np.isfinite(v).all(), "%s %s: not finite (never written?)" % (case, q)
    return res


def _check_gram(o, case, running=RUNNING):
    eps = K.EPS
    zr = o.get("zero_row")
    keep = np.ones(o["c"], dtype=bool)
    if zr is not None:
        keep[zr] = False
    late = []
    for tag, with_rm, with_rv, momentum in running:
        cs = "%s_%s" % (case, tag)
        got = _run_gram(o, with_rm, with_rv, momentum, cs)
        ref = R.gram_stats(o["gram"], o["a_mean"], o["w"], o["m"], o["gamma"], o["beta"], eps, momentum, o["running_mean"] if with_rm else None,
                           o["running_var"] if with_rv else None)
        _elem(cs, "save_mean", got["mean"], ref["mean"], 8 * U * ref["A_mean"])
        var = 1.0 / got["invstd"] ** 2 - float(np.float32(eps))
        _elem(cs, "variance (1 / invstd^2 - eps)", var[keep], ref["var"][keep], 8 * U * ref["A_var"][keep])
        sc = o["gamma"] * got["invstd"]
        _elem(cs, "scale from the kernel's invstd", got["scale"], sc, 4 * U * np.abs(sc))
        _elem(cs, "shift from the kernel's mean and scale", got["shift"], o["beta"] - got["mean"] * got["scale"], 4 * U * (np.abs(o["beta"]) + np.abs(got["mean"] * got["scale"])))
        if with_rm:
            _elem(cs, "running_mean", got["running_mean"], ref["running_mean"], 8 * U * ref["A_running_mean"])
        if with_rv:
            _elem(cs, "running_var", got["running_var"], ref["running_var"], 8 * U * ref["A_running_var"])
        if zr is not None:
            inv0 = 1.0 / np.sqrt(float(np.float32(eps)))
            assert got["mean"][zr] == 0.0 and abs(got["invstd"][zr] - inv0) <= 2 * U * inv0, (cs, got["mean"][zr], got["invstd"][zr])
            if with_rv and momentum == 1.0:
                assert got["running_var"][zr] == 0.0, (cs, got["running_var"][zr])                       # the variance of a zero row is zero EXACTLY
            if with_rm and momentum == 1.0:
                assert got["running_mean"][zr] == 0.0
        if o["m"] == 1 and with_rv and momentum == 1.0:
            assert not got["running_var"].any(), "%s: one row has no variance" % cs
        for q in ("mean", "invstd", "scale", "shift"):
            _reduced(cs, "gram_" + q, got[q], ref[q], late)
        if with_rm:
            _reduced(cs, "gram_running_mean", got["running_mean"], ref["running_mean"], late)
        if with_rv and ref["running_var"].any():
            _reduced(cs, "gram_running_var", got["running_var"], ref["running_var"], late)
    assert not late, "every elementwise bound holds; the reduced quantities miss theirs:\n" + "\n".join(late)


def _gram_params():
    rows = {"plain": K.GRAM_ROWS, "zero_row": (1, 17, 37), "offset3": (17, 37, 1568)}
    return [pytest.param(c, k, m, fam, id="c%d_k%d_m%d-%s" % (c, k, m, fam)) for fam in K.GRAM_FAMILIES for c, k in K.GRAM_SHAPES for m in rows[fam]]


@pytest.mark.parametrize("c,k,m,family", _gram_params())
def test_gram_statistics(c, k, m, family):
    """The six outputs for running statistics given, NULL and half given, at momentum 0.1 and 1; a zero weight row; a2 = relu(N(0, 1)) + 3,
    whose |mean| / std of about 5 the uncentred Gram form has to cancel.

    Up to dzfree_cases.GRAM_F64_MAX_ROWS rows the library takes its fp64 kernel (m = 1, 2, 16 here; 17 is the first row count of the matrix-core kernel).  This
    test is why that kernel exists: with two rows Gc = d d^T / 4 has rank one and var_c = (W[c] . d)^2 / 4 is a chi-square(1) variable over the channels -- of 96+
    channels some have a variance of 1e-5 .. 2e-7 (median 0.14), 1e6 times below A_var, and invstd = (var + eps)^-1/2 multiplies the fp32 error of the sum by that
    ratio.  Under the matrix-core kernel alone every elementwise bound held at m = 2, but the rel_l2 of invstd / scale / shift measured 1.6e-4 .. 5.9e-4 against the
    2e-5 bound (plain numpy float32 on the same inputs: 6e-5 .. 2e-3)."""
    _check_gram(K.triple(m, c, k, family), "gram_%s_c%d_k%d_m%d" % (family, c, k, m))


@pytest.mark.parametrize("m", K.LATTICE_GRAM_ROWS)
def test_gram_lattice_is_exact(m):
    """Dyadic inputs, Gc of up to 20 bits (hi + mid + lo), a ragged workgroup, momentum 1/2, on both sides of the few-rows switch (m = 2: the fp64 kernel; m = 32:
    the matrix-core kernel): save_mean and running_mean bit for bit; running_var bit for bit the fp32 statement of it from the EXACT variance
    (dzfree_cases.lattice_running_var: exact at m = 2, where the variance itself follows bit for bit; one rounding of var m / (m - 1) and one of the sum at 32)."""
    o = K.lattice_gram(m)
    case = "gram_lattice_m%d" % m
    got = _run_gram(o, True, True, o["momentum"], case)
    ref = R.gram_stats(o["gram"], o["a_mean"], o["w"], o["m"], o["gamma"], o["beta"], K.EPS, o["momentum"], o["running_mean"], o["running_var"])
    _exact(case, "save_mean", got["mean"], ref["mean"])
    _exact(case, "running_mean", got["running_mean"], ref["running_mean"])
    _exact(case, "running_var", got["running_var"], K.lattice_running_var(o, ref["var"]))
    if m == 2:
        var = (got["running_var"] - (1 - o["momentum"]) * o["running_var"]) / (o["momentum"] * o["m"] / (o["m"] - 1.0))
        _exact(case, "variance", var, ref["var"])
    _check_gram(o, case, running=(("both", True, True, o["momentum"]),))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    """Two of the refusals of tests/test_abi_cpu.py again, with real device buffers: the code comes back and no output byte has changed."""
    lib = _lib()
    o = K.triple(37, 256, 32)
    wd = _bf(o["wd"])
    par = _bn(o)
    bd, bias = _Out((32, 192 + 32), BF), _Out((32,))
    rc = lib.mvf_bn_bwd_dzfree_prep(P(wd), 192, 32, *[P(t) for t in par], 37, P(bd.t), P(bias.t), 1, None)          # c = 192: a multiple of 64, not of 256
    assert rc == ESHAPE and b"bn_bwd_dzfree_prep" in lib.mvf_last_error(), (rc, lib.mvf_last_error())
    assert bd.untouched() and bias.untouched()
    s = K.triple(K.SUMS_M, 64, 12)
    lo, hi = K.partial_rows(s["gm"], 64, 6, 3, 5, seed=2)
    dg, db = _Out((64,)), _Out((64,))
    q, w, mean, invstd, phi = _f(s["q"]), _bf(s["w"]), _f(s["mean"]), _f(s["invstd"]), _f(hi)
    rc = lib.mvf_bn_bwd_dzfree_sums(P(q), P(w), 64, 12, P(mean), P(invstd), None, 3, 6, P(phi), 5, P(dg.t), P(db.t), 1, None)     # a split without part_lo
    assert rc == EINVAL and b"bn_bwd_dzfree_sums" in lib.mvf_last_error(), (rc, lib.mvf_last_error())
    assert dg.untouched() and db.untouched()
    for t in (bd, bias, dg, db):
        t.check("refusals")
