"""Drop path (stochastic depth) on the device: the two kernels of csrc/drop_path.hip against the fp64 restatement (tests/droppath_ref.py), bottleneck blocks
through BlockTrainer against the torch-fp64 bottleneck with the per-image scale on the branch, and the train engine (table upload, launch plans, accumulation,
eval / precise_bn, and an engine that never sets drop_path).  Reference semantics: timm drop_path(x, p, training, scale_by_keep) after bn3 of
Bottleneck.forward (codes/models/backbones/resnet.py:208-244)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_pool_ref as R
import droppath_ref as DR
from helpers import golden, rel_err, rel_l2
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(6, 4, 3), (5 * 49, 256, 49), (8 * 49, 512, 49), (7, 2048, 1), (4 * 196, 1024, 196)]        # (m, c, rows_per_image)
VALUES = [0.0, 1.0, float(np.float32(1.0 / 0.9)), 0.37, 2.5]
DTYPES = ["f32", "bf16"]


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """A kernel fault surfaces at the next synchronisation: nothing more of this module is launched behind one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault behind a drop-path test: %s" % e, returncode=3)


def _params():
    return [pytest.param(m, c, rpi, dt, id="m%d_c%d_r%d_%s" % (m, c, rpi, dt)) for m, c, rpi in SHAPES for dt in DTYPES]


def _tt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _dt(dtype):
    return 0 if dtype == "f32" else 1


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(_tt(dtype)).cuda()


def _f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return t.double().cpu().numpy()


def _raw(t):
    """The tensor's bits (a comparison that tells -0 from +0 and never meets NaN != NaN)."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _elem(case, what, got, ref, a, dtype, skip=None):
    """The bound of tests/test_bn_pool_kernels_gpu.py::_elem: 8 * 2^-24 * A, plus 2^-8 |ref| for bf16 storage."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s %s: %d of %d elements are not finite (never written?)" % (case, what, int((~np.isfinite(got)).sum()), got.size)
    tol = 8.0 * 2.0 ** -24 * a + (2.0 ** -8 * np.abs(ref) if dtype == "bf16" else 0.0)
    bad = np.abs(got - ref) > tol
    if skip is not None:
        bad &= ~skip
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.abs(got - ref) / np.maximum(tol, 1e-300), 0)), got.shape)
        raise AssertionError("%s %s %s: %d of %d elements beyond the bound; worst at %s: got %.9g, ref %.9g, bound %.3g" % (case, what, dtype, int(bad.sum()), got.size, i,
                                                                                                                      got[i], ref[i], tol[i]))


@functools.lru_cache(maxsize=None)
def _operands(m, c, rpi, dtype):
    """z, r, g rounded to the storage type (fp64 numpy), fp32 coefficients, a table that cycles through VALUES, random sign bits."""
    rng = np.random.default_rng(1000 * c + m)
    o = dict(m=m, c=c, rpi=rpi, n=m // rpi)
    for k in ("z", "r", "g"):
        o[k] = R.round_storage(rng.standard_normal((m, c)) * 1.5, dtype)
    for k in ("scale", "shift", "rscale", "rshift"):
        o[k] = (rng.standard_normal(c) * (0.3 if "shift" in k else 1.0) + (1.0 if "scale" in k else 0.0)).astype(np.float32).astype(np.float64)
    o["table"] = np.array([VALUES[(i + c // 4) % len(VALUES)] for i in range(o["n"])], dtype=np.float32)
    o["bits"] = R.pack_bits(rng.random((m, c)) < 0.6)
    return o


def _run_apply(o, dtype, act, res, table):
    from mvfnet_amd import _lib
    m, c = o["m"], o["c"]
    z, r = _dev(o["z"], dtype), _dev(o["r"], dtype)
    sc, sh = _f32(o["scale"]), _f32(o["shift"])
    rs, rb = (_f32(o["rscale"]), _f32(o["rshift"])) if res == "affine" else (None, None)
    tab = _f32(table)
    out = torch.full((m, c), float("nan"), dtype=_tt(dtype), device="cuda")
    bits = torch.full((m, c // 4), 0xEE, dtype=torch.uint8, device="cuda")
    rc = _lib.lib.mvf_bn_apply_bits_rowscale(P(z), m, c, P(sc), P(sh), P(r), P(rs), P(rb), P(tab), o["rpi"], act, P(out), P(bits), _dt(dtype), None)
    assert rc == 0, _lib.lib.mvf_last_error()
    torch.cuda.synchronize()
    return out, bits, (z, r, sc, sh, rs, rb)


def _run_gate(o, dtype, pitch, table):
    from mvfnet_amd import _lib
    m, c = o["m"], o["c"]
    gbuf = torch.full((m, pitch), float("nan"), dtype=_tt(dtype), device="cuda")
    gbuf[:, :c] = _dev(o["g"], dtype)
    bits = torch.from_numpy(o["bits"]).cuda()
    tab = _f32(table)
    gm = torch.full((m, c), float("nan"), dtype=_tt(dtype), device="cuda")
    rc = _lib.lib.mvf_gate_rowscale(P(gbuf), pitch, P(bits), P(tab), o["rpi"], m, c, P(gm), _dt(dtype), None)
    assert rc == 0, _lib.lib.mvf_last_error()
    torch.cuda.synchronize()
    return gm, gbuf, bits


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("m,c,rpi,dtype", _params())
def test_apply_rowscale_against_the_restatement(m, c, rpi, dtype):
    """Plain and affine residual x act 0 / 1, a table of 0, 1, fp32(1 / 0.9), 0.37 and 2.5, outputs pre-filled with NaN / 0xEE."""
    o = _operands(m, c, rpi, dtype)
    for res in ("plain", "affine"):
        for act in (0, 1):
            case = "apply m%d c%d rpi%d %s %s act%d" % (m, c, rpi, dtype, res, act)
            kw = dict(rscale=o["rscale"], rshift=o["rshift"]) if res == "affine" else {}
            ref = DR.apply_bits_rowscale(o["z"], o["scale"], o["shift"], o["r"], o["table"], rpi, act=act, **kw)
            out, bits, _ = _run_apply(o, dtype, act, res, o["table"])
            got = _np(out)
            _elem(case, "out", got, ref["out"], ref["A"], dtype)
            gb = bits.cpu().numpy()
            assert np.array_equal(gb, R.pack_bits(got > 0)), "%s: the sign bits are not those of the stored output" % case
            und = ref["undecided"]
            assert und.mean() < 1e-3, (case, float(und.mean()))
            assert np.array_equal(R.unpack_bits(gb, c)[~und], (ref["out"] > 0)[~und]), "%s: sign bits against the reference" % case


@pytest.mark.parametrize("m,c,rpi,dtype", _params())
def test_gate_rowscale_against_the_restatement(m, c, rpi, dtype):
    o = _operands(m, c, rpi, dtype)
    for pitch in (c, c + 8):
        ref, a = DR.gate_rowscale(o["g"], o["bits"], o["table"], rpi)
        gm, _, _ = _run_gate(o, dtype, pitch, o["table"])
        _elem("gate m%d c%d rpi%d %s pitch%d" % (m, c, rpi, dtype, pitch), "gm", _np(gm), ref, a, dtype)
        assert np.array_equal(_np(gm) != 0, ref != 0)


@pytest.mark.parametrize("m,c,rpi,dtype", _params())
def test_unit_scale_is_bn_apply_bits_bit_for_bit(m, c, rpi, dtype):
    from mvfnet_amd import _lib
    o = _operands(m, c, rpi, dtype)
    ones = np.ones(o["n"], dtype=np.float32)
    for res in ("plain", "affine"):
        for act in (0, 1):
            out, bits, (z, r, sc, sh, rs, rb) = _run_apply(o, dtype, act, res, ones)
            out0 = torch.full_like(out, float("nan"))
            bits0 = torch.full_like(bits, 0xEE)
            rc = _lib.lib.mvf_bn_apply_bits(P(z), m, c, P(sc), P(sh), P(r), P(rs), P(rb), act, P(out0), P(bits0), _dt(dtype), None)
            assert rc == 0, _lib.lib.mvf_last_error()
            torch.cuda.synchronize()
            assert torch.equal(_raw(out), _raw(out0)), (res, act)
            assert torch.equal(bits, bits0), (res, act)


@pytest.mark.parametrize("m,c,rpi,dtype", _params())
def test_unit_scale_gate_is_bn_bwd_reduce_mode_4_bit_for_bit(m, c, rpi, dtype):
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = _operands(m, c, rpi, dtype)
    ones = np.ones(o["n"], dtype=np.float32)
    for pitch in (c, c + 8):
        gm, gbuf, bits = _run_gate(o, dtype, pitch, ones)
        z = _dev(o["z"], dtype)
        mean, invstd = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        dgamma, dbeta = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        nb = lib.mvf_bn_workspace_bytes(m, c)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        gm0 = torch.full_like(gm, float("nan"))
        rc = lib.mvf_bn_bwd_reduce(P(gbuf), pitch, P(z), P(bits), m, c, P(mean), P(invstd), None, None, 4, P(gm0), P(dgamma), P(dbeta), P(ws), nb, _dt(dtype), None)
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert torch.equal(_raw(gm), _raw(gm0)), pitch


@pytest.mark.parametrize("m,c,rpi,dtype", _params())
def test_zero_scale_is_the_residual_exactly(m, c, rpi, dtype):
    """s = 0 and a finite z: out = act(res), whatever the branch holds -- the plain residual as stored, the affine one as mvf_bn_apply_bits forms it."""
    from mvfnet_amd import _lib
    o = _operands(m, c, rpi, dtype)
    zeros = np.zeros(o["n"], dtype=np.float32)
    for act in (0, 1):
        out, bits, (z, r, sc, sh, rs, rb) = _run_apply(o, dtype, act, "plain", zeros)
        assert torch.equal(out, torch.relu(r) if act else r), act
        out, bits, (z, r, sc, sh, rs, rb) = _run_apply(o, dtype, act, "affine", zeros)
        res = torch.full_like(out, float("nan"))
        rc = _lib.lib.mvf_bn_apply_bits(P(r), m, c, P(rs), P(rb), None, None, None, act, P(res), None, _dt(dtype), None)
        assert rc == 0, _lib.lib.mvf_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, res), act
        assert np.array_equal(bits.cpu().numpy(), R.pack_bits(_np(out) > 0))


def test_refusals_leave_the_outputs_untouched():
    from mvfnet_amd import _lib
    lib = _lib.lib
    m, c, rpi = 6, 8, 3
    z = torch.randn(m, c, device="cuda").bfloat16()
    big = torch.randn(m, c + 8, device="cuda").bfloat16()
    sc = torch.ones(c + 4, device="cuda")
    tab = torch.ones(4, device="cuda")
    out = torch.full((m * c + 16,), float("nan"), dtype=torch.bfloat16, device="cuda")
    bits = torch.full((m, c // 4), 0xEE, dtype=torch.uint8, device="cuda")

    def apply(z_=z, m_=m, c_=c, scale=sc, shift=sc, residual=z, rscale=None, rshift=None, row_scale=tab, rpi_=rpi, act=1, out_=out, bits_=bits, dtype=1):
        return lib.mvf_bn_apply_bits_rowscale(P(z_), m_, c_, P(scale), P(shift), P(residual), P(rscale), P(rshift), P(row_scale), rpi_, act, P(out_), P(bits_), dtype, None)

    def gate(g=big, pitch=c + 8, bits_=bits, row_scale=tab, rpi_=rpi, m_=m, c_=c, gm=out, dtype=1):
        return lib.mvf_gate_rowscale(P(g), pitch, P(bits_), P(row_scale), rpi_, m_, c_, P(gm), dtype, None)
    cases = [apply(z_=None), apply(scale=None), apply(shift=None), apply(residual=None), apply(row_scale=None), apply(out_=None), apply(bits_=None), apply(rpi_=0),
             apply(rpi_=4), apply(m_=7), apply(c_=6), apply(dtype=2), apply(act=2), apply(act=-1), apply(rscale=sc), apply(out_=out[1:]), apply(z_=z.view(-1)[4:]),
             apply(scale=sc[1:]), apply(row_scale=tab.view(torch.uint8)[2:]),
             gate(g=None), gate(bits_=None), gate(row_scale=None), gate(gm=None), gate(rpi_=0), gate(rpi_=-1), gate(rpi_=5), gate(c_=6), gate(pitch=4), gate(pitch=10),
             gate(dtype=3), gate(gm=out[2:]), gate(g=big.view(-1)[4:])]
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in cases), cases
    assert bool(torch.isnan(out.float()).all()) and bool((bits == 0xEE).all()), "a refused call wrote an output"
    assert apply() == 0 and gate(gm=out) == 0                                   # the calls themselves are good ones
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ blocks through BlockTrainer
T = 4
#                name: (cin, planes, H, stride, mvf)
BLOCKS = {
    "plain_64": (256, 64, 14, 1, False),
    "plain_64_mvf": (256, 64, 14, 1, True),
    "plain_256": (1024, 256, 7, 1, False),             # (the default takes the dz3-free path here)
    "down_s1": (64, 64, 14, 1, False),
    "down_s2": (256, 128, 14, 2, False),
}
KEEP = float(np.float32(1.0 / 0.8))
TABLES = {"clip1_dropped": [KEEP] * T + [0.0] * T, "mixed": [KEEP, 0.0, KEEP, KEEP, 0.0, KEEP, KEEP, 0.0]}
MVF_KW = dict(mode="THW", share=False, use_hs=True)


def _block(name):
    from mvfnet_amd.backbones.resnet import Bottleneck
    from mvfnet_amd.modules import MVF
    cin, planes, hw, stride, mvf = BLOCKS[name]
    torch.manual_seed(sorted(BLOCKS).index(name))
    down = None
    if stride != 1 or cin != planes * 4:
        down = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    blk = Bottleneck(cin, planes, stride, 1, down)
    if mvf:
        blk.conv1 = MVF(blk.conv1, T, cin, 0.125, True, False, "THW")
    for m_ in blk.modules():
        if isinstance(m_, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m_.weight.uniform_(0.5, 1.5)
                m_.bias.normal_(0.0, 0.2)
                m_.running_mean.normal_(0.0, 0.1)
                m_.running_var.uniform_(0.5, 1.5)
    return blk


def _inputs(name):
    cin, planes, hw, stride, mvf = BLOCKS[name]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2 * T, cin, hw, hw, generator=g).relu_().bfloat16().float()           # a block input is a ReLU output; exact in either storage type
    ho = (hw - 1) // stride + 1
    dy = torch.randn(2 * T, planes * 4, ho, ho, generator=g).bfloat16().float()
    return x, dy


@functools.lru_cache(maxsize=None)
def _reference(name, table):
    """The torch-fp64 bottleneck with the scale on the branch (table: a key of TABLES, or None = every scale 1): y, dx, every parameter gradient."""
    cin, planes, hw, stride, mvf = BLOCKS[name]
    blk = _block(name)
    sd = {k: (v.detach().double().requires_grad_(k in dict(blk.named_parameters())) if v.is_floating_point() else v.detach().clone()) for k, v in blk.state_dict().items()}
    x, dy = _inputs(name)
    x = x.double().requires_grad_(True)
    s = None if table is None else torch.tensor(TABLES[table], dtype=torch.float32).double()
    y = DR.bottleneck(x, sd, "", stride, T, MVF_KW if mvf else None, True, {}, scale=s)
    y.backward(dy.double())
    return y.detach().numpy(), x.grad.numpy(), {k: t.grad.numpy() for k, t in sd.items() if torch.is_tensor(t) and t.requires_grad}


def _run_block(name, dtype, table):
    """A fresh block through BlockTrainer; table: a key of TABLES or None (drop path off).  Returns trainer, block, y, dx (NCHW, storage type)."""
    from mvfnet_amd.train_engine import BlockTrainer
    blk = _block(name).cuda().train()
    tr = BlockTrainer(blk, dtype=dtype)
    x, dy = _inputs(name)
    if table is not None:
        tr.set_drop_scale(torch.tensor(TABLES[table], dtype=torch.float32, device="cuda"))
    y = tr.forward(x.cuda())
    state = dict(fuse_apply=tr.blk.fuse_apply(tr), z3_free=tr.blk.z3_free(tr, y.shape[0] * y.shape[2] * y.shape[3]), dzfree=tr.blk.dzfree(tr, y.shape[0] * y.shape[2] * y.shape[3]),
                 gram_fwd=tr.blk.gram_fwd(tr, y.shape[0] * y.shape[2] * y.shape[3]), q_z3_free=tr.blk.q_z3_free(tr, y.shape[0] * y.shape[2] * y.shape[3]),
                 gated=tr.blk.wants_gated_gradient(tr), z3_stored=tr.blk.saved["z3"] is not None)
    y = y.contiguous().clone()
    dx = tr.backward(dy.cuda()).contiguous().clone()
    torch.cuda.synchronize()
    return tr, blk, y, dx, state


def _errors(name, tr, blk, y, dx, ref, err):
    ry, rdx, rgrads = ref
    e = dict(y=err(_np(y), ry), dx=err(_np(dx), rdx))
    for pn, p in blk.named_parameters():
        e["grad/" + pn] = err(_np(tr.grad_of(p)), rgrads[pn])
    return e


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_fp32_against_the_fp64_restatement(name, table):
    cin, planes, hw, stride, mvf = BLOCKS[name]
    tr, blk, y, dx, state = _run_block(name, torch.float32, table)
    assert state == dict(fuse_apply=False, z3_free=False, dzfree=False, gram_fwd=False, q_z3_free=False, gated=None, z3_stored=True), state
    x, _ = _inputs(name)
    if name.startswith("plain") and table == "clip1_dropped":
        assert torch.equal(_raw(y[T:]), _raw(torch.relu(x.cuda())[T:])), "the dropped clip's output rows are not relu(x)"
    e = _errors(name, tr, blk, y, dx, _reference(name, table), rel_err)
    print("drop path block %s %s fp32: y %.3g dx %.3g worst grad %.3g" % (name, table, e["y"], e["dx"], max(v for k, v in e.items() if k.startswith("grad/"))))
    assert e["y"] < 1e-5, e
    assert e["dx"] < 1e-4, e
    for k, v in e.items():
        if k.startswith("grad/"):
            assert v < 2e-4, (k, v)
    tr2, blk2, y2, dx2, _ = _run_block(name, torch.float32, table)              # two runs: identical bits
    assert torch.equal(_raw(y), _raw(y2)) and torch.equal(_raw(dx), _raw(dx2))
    assert torch.equal(_raw(tr.flat_grads), _raw(tr2.flat_grads))


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_bf16_error_against_the_unchanged_path(name, table):
    """bf16 storage has no rounding-point emulation of the new line, so the error is bounded against the parent path: E_on <= 2 E_off + 1e-3 in rel_l2, E_off the
    error of the same block on the same inputs with drop path OFF against the s = 1 restatement (unchanged code), measured here.  The tables keep at least one of
    the two clips: the signal norm then falls by at most about sqrt(2) while the rounding noise does not -- the factor 2."""
    tr0, blk0, y0, dx0, state0 = _run_block(name, torch.bfloat16, None)
    if name == "plain_256":
        assert state0["dzfree"] is True                                          # what the block takes without drop path
    e_off = _errors(name, tr0, blk0, y0, dx0, _reference(name, None), rel_l2)
    tr, blk, y, dx, state = _run_block(name, torch.bfloat16, table)
    assert state == dict(fuse_apply=False, z3_free=False, dzfree=False, gram_fwd=False, q_z3_free=False, gated=None, z3_stored=True), state
    x, _ = _inputs(name)
    if name.startswith("plain") and table == "clip1_dropped":
        assert torch.equal(_raw(y[T:]), _raw(torch.relu(x.cuda().bfloat16())[T:])), "the dropped clip's output rows are not relu(x)"
    e_on = _errors(name, tr, blk, y, dx, _reference(name, table), rel_l2)
    for k in sorted(e_on):
        print("drop path block %s %s bf16 %s: E_on %.3g E_off %.3g" % (name, table, k, e_on[k], e_off[k]))
    for k in sorted(e_on):
        assert e_on[k] <= 2.0 * e_off[k] + 1e-3, (k, e_on[k], e_off[k])
    tr2, blk2, y2, dx2, _ = _run_block(name, torch.bfloat16, table)
    assert torch.equal(_raw(y), _raw(y2)) and torch.equal(_raw(dx), _raw(dx2)) and torch.equal(_raw(tr.flat_grads), _raw(tr2.flat_grads))


def test_block_trainer_hook_sets_and_clears():
    tr, blk, y, dx, state = _run_block("plain_64", torch.bfloat16, "mixed")
    assert tr.blk.drop is not None
    tr.set_drop_scale(None)
    assert tr.blk.drop is None and tr.blk.fuse_apply(tr) is True
    with pytest.raises(ValueError):
        tr.set_drop_scale(torch.ones(8, device="cuda", dtype=torch.float64))
    tr.set_drop_scale(torch.ones(5, device="cuda"))
    with pytest.raises(ValueError, match="per image"):
        tr.forward(_inputs("plain_64")[0].cuda())


# ------------------------------------------------------------------------------------------------ the engine
N_BLOCKS = 16
NEW_CALLS = ("mvf_bn_apply_bits_rowscale", "mvf_gate_rowscale")


def _model(dropout=0.0, train_cfg=None):
    import mvfnet_amd
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, T, dropout_ratio=dropout), train_cfg, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().train()


def _small_batch(seed=3, b=2):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(b, T, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (b, 1), device="cuda", generator=gen)


def _recorded(eng, fn):
    """The names of the library calls `fn` makes through the engine."""
    from mvfnet_amd import launch_plan
    with launch_plan.recording(eng) as rec:
        fn()
    torch.cuda.synchronize()
    return [op[2] for op in rec.ops]


def test_engine_unit_table_meets_the_golden_first_step():
    """An all-ones table: every block from 1 on runs the new kernels, and the first step is the reference's (tests/golden/net_cases.npz, the bounds of
    test_c1_train_two_steps_vs_reference_golden)."""
    from mvfnet_amd.droppath import ExplicitDropPath
    g = golden("net_cases.npz")
    m = _model()
    eng = m.train_engine()
    eng.drop_path = ExplicitDropPath(np.ones((N_BLOCKS, 2 * T), dtype=np.float32))
    imgs = torch.from_numpy(synth.synth_clip_batch(2, T, 224, 224)).cuda()
    labels = torch.from_numpy(synth.synth_labels(2)).cuda()
    out = {}

    def step():
        out["loss"] = eng.forward(imgs, labels)
        eng.backward()
    names = _recorded(eng, step)
    assert len(eng.blocks) == N_BLOCKS and eng.blocks[0].drop is None and all(b.drop is not None for b in eng.blocks[1:])
    assert names.count(NEW_CALLS[0]) == N_BLOCKS - 1 and names.count(NEW_CALLS[1]) == N_BLOCKS - 1
    norm = eng.step()
    loss = float(out["loss"])
    print("drop path engine, unit table: loss %.8g (golden %.8g) norm %.8g (golden %.8g)" % (loss, float(g["c1/train/loss/0"]), float(norm[0]), float(g["c1/train/total_norm/0"])))
    assert abs(loss - float(g["c1/train/loss/0"])) < 2e-5 * float(g["c1/train/loss/0"])
    assert abs(float(norm[0]) - float(g["c1/train/total_norm/0"])) < 2e-3 * float(g["c1/train/total_norm/0"])


def test_engine_row_i_of_the_table_reaches_block_i():
    """Clip 1 dropped everywhere: every plain block's output rows of clip 1 are relu of its input rows, bit for bit.  Then one block alone."""
    from mvfnet_amd.droppath import ExplicitDropPath
    m = _model()
    eng = m.train_engine(dtype=torch.bfloat16)
    eng.keep_io = True
    imgs, labels = _small_batch()
    table = np.ones((N_BLOCKS, 2 * T), dtype=np.float32)
    table[1:, T:] = 0.0
    eng.drop_path = ExplicitDropPath(table)

    def dropped(blk):
        io = blk.io
        rows = io["ho"] * io["wo"] * T
        return torch.equal(_raw(io["out"][rows:]), _raw(torch.relu(io["x"])[rows:]))
    eng.forward(imgs, labels)
    eng.backward()
    torch.cuda.synchronize()
    plain = [i for i, b in enumerate(eng.blocks) if b.cd is None]
    assert len(plain) == 12 and all(dropped(eng.blocks[i]) for i in plain)
    table = np.ones((N_BLOCKS, 2 * T), dtype=np.float32)
    table[5, T:] = 0.0                                                           # block 5 alone
    eng.drop_path.table = table
    eng.forward(imgs, labels)
    eng.backward()
    torch.cuda.synchronize()
    assert [i for i in plain if dropped(eng.blocks[i])] == [5]


def _train(use_plan, steps, accumulate=False):
    from mvfnet_amd.droppath import DropPath
    torch.manual_seed(7)
    m = _model(dropout=0.5)
    eng = m.train_engine(dtype=torch.bfloat16)
    eng.use_plan = use_plan
    eng.drop_path = DropPath(0.3, seed=5)                                        # a fresh table every step, the same sequence in both runs
    batches = [_small_batch(seed=s_) for s_ in (3, 4, 5)]
    losses = []
    for i in range(steps):
        imgs, labels = batches[i % 3]
        losses.append(eng.train_step(imgs.clone(), labels.clone()).clone())
    torch.cuda.synchronize()
    return eng, torch.cat(losses), eng.flat_params.clone(), [b.clone() for b in m.buffers()]


def test_engine_replayed_steps_equal_eager_steps_bit_for_bit():
    """Two eager steps, two recordings, then three steps replayed from the plan, each with its own table, against the same seven steps eager."""
    eng_p, loss_p, par_p, buf_p = _train(True, 7)
    eng_e, loss_e, par_e, buf_e = _train(False, 7)
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["eager"] == eng_p.plan_warmup and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    names = st[0]["plan"].names
    assert names.count(NEW_CALLS[0]) == N_BLOCKS - 1 and names.count(NEW_CALLS[1]) == N_BLOCKS - 1
    assert not getattr(eng_e, "_plans", None)
    assert torch.equal(loss_p, loss_e), (loss_p, loss_e)
    assert torch.equal(par_p, par_e)
    for a, b in zip(buf_p, buf_e):
        assert torch.equal(a, b)
    assert len(set(loss_p.tolist())) == 7


def test_engine_draws_per_micro_step_and_not_in_eval_or_precise_bn():
    from mvfnet_amd.droppath import DropPath

    class Counting(DropPath):
        draws = 0

        def draw(self, n_blocks, b, t):
            self.draws += 1
            return DropPath.draw(self, n_blocks, b, t)
    dp = Counting(0.2, seed=1)
    m = _model(train_cfg=dict(drop_path=dp))
    assert m.drop_path is dp
    eng = m.train_engine(dtype=torch.bfloat16)
    assert eng.drop_path is dp
    imgs, labels = _small_batch()
    # an eval-mode forward: bit-identical with and without the config (the same untrained weights on both sides)
    m.eval()
    assert eng.drop_path is None
    loss_eval = m(imgs, labels)["loss_cls"].detach().clone()
    scores = m(imgs, None, return_loss=False, return_numpy=False).clone()
    m0 = _model().eval()
    m0.train_engine(dtype=torch.bfloat16)
    loss0 = m0(imgs, labels)["loss_cls"].detach().clone()
    scores0 = m0(imgs, None, return_loss=False, return_numpy=False).clone()
    torch.cuda.synchronize()
    assert dp.draws == 0 and torch.equal(loss_eval, loss0) and torch.equal(scores, scores0)
    del m0
    m.train()
    assert eng.drop_path is dp
    eng.accumulate_step(imgs, labels)
    eng.accumulate_step(imgs, labels)
    assert dp.draws == 2
    eng.apply_accumulated()
    assert dp.draws == 2
    # precise_bn: no draw, none of the new calls, and the object is back afterwards
    names = _recorded(eng, lambda: eng.precise_bn([(imgs, labels)], num_iters=1))
    assert dp.draws == 2 and not any(n in names for n in NEW_CALLS) and "mvf_bn_apply_bits" in names
    assert eng.drop_path is dp
    names = _recorded(eng, lambda: (eng.forward(imgs, labels), eng.backward()))
    assert dp.draws == 3 and names.count(NEW_CALLS[0]) == N_BLOCKS - 1
    m.eval()                                                                     # back in eval mode: no draw, none of the new calls
    names = _recorded(eng, lambda: m(imgs, labels))
    assert dp.draws == 3 and not any(n in names for n in NEW_CALLS) and all(b.drop is None for b in eng.blocks)


def test_engine_without_drop_path_is_the_untouched_engine():
    """drop_path never set, and set and cleared again: the recorded call list of a step and the plan key equal those of an engine that never saw it."""
    from mvfnet_amd.droppath import DropPath
    imgs, labels = _small_batch()

    def step_names(eng):
        return _recorded(eng, lambda: (eng.forward(imgs, labels), eng.backward()))
    m_a = _model()
    a = m_a.train_engine(dtype=torch.bfloat16)
    names_a = step_names(a)
    key_a = a._plan_key(imgs, labels)
    assert not any(n in names_a for n in NEW_CALLS) and "drop_path" not in a._switch_names and not any(isinstance(k, tuple) and k and k[0] == "drop_path" for k in key_a)
    m_b = _model()
    b = m_b.train_engine(dtype=torch.bfloat16)
    assert step_names(b) == names_a and b._plan_key(imgs, labels) == key_a
    b.drop_path = DropPath(0.2, seed=2)
    key_on = b._plan_key(imgs, labels)
    assert key_on[:len(key_a)] == key_a and key_on[len(key_a):] == (("drop_path", (False,) + (True,) * (N_BLOCKS - 1), "clip", True),)
    b.drop_path = DropPath(0.2, unit="frame", scale_by_keep=False)
    assert b._plan_key(imgs, labels)[-1] == ("drop_path", (False,) + (True,) * (N_BLOCKS - 1), "frame", False)
    names_on = step_names(b)
    assert names_on.count(NEW_CALLS[0]) == N_BLOCKS - 1 and all(blk.drop is not None for blk in b.blocks[1:])
    b.drop_path = None
    assert b._plan_key(imgs, labels) == key_a
    assert step_names(b) == names_a and all(blk.drop is None for blk in b.blocks)
    assert "drop_path_table" in {k[0] for k in b._bufs} and "drop_path_table" not in {k[0] for k in a._bufs}
