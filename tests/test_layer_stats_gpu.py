"""GPU: per-parameter training statistics and skipped-step diagnosis -- mvf_flat_segment_stats / mvf_bn_stats_nonfinite (csrc/layer_stats.hip) against the
fp64 restatement in numpy (tests/layer_stats_numpy.py), and the engine layer above them (TrainEngine.enable_layer_stats, measure_layer_stats, layer_stats,
last_skip).

Bounds.  Counts and absmax: exactly equal.  sumsq: relative (n_s + 4) * 2^-52 for a segment of n_s elements -- the squares of floats are exact in double, only
the order of at most n_s non-negative additions differs, plus the two roundings of the difference mode; derived, not measured.  The engine's clip norm
(norm_out[0], fp32 partial sums) against the fp64 figures: 1e-5 relative, what tests/test_head_optimizer_gpu.py grants it against fp64."""
import numpy as np
import pytest
import torch

import layer_stats_numpy as ln
from helpers import library_names
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

CHUNK = 4096
# 8192 ends on a chunk boundary, so 4097 STARTS on one (and reaches one element into chunk 3); 1, 3, 64, 64 share chunk 3 with that element and with the head
# of 8193, which spans chunks 3, 4 and 5; 20000 runs to the ragged end of the range
LENGTHS = (8192, 4097, 1, 3, 64, 64, 8193, 20000)
FIRST = [int(v) for v in np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])]
N = int(sum(LENGTHS))
PATTERN = 0x5A


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib


def _values(n, seed):
    """A mix of magnitudes 1e-30, 1, 1e19 with random mantissas and signs, and signed zeros."""
    rng = np.random.RandomState(seed)
    mag = np.array([1e-30, 1.0, 1e19, 0.0], np.float64)[rng.randint(0, 4, n)]
    return (mag * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _device(x, offset):
    """x on the device, `offset` elements into an allocation of its own: 4-byte aligned only, as the engine's flat_*[off:] views."""
    buf = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
    v = buf[offset:offset + x.size]
    v.copy_(torch.from_numpy(x))
    return v


def _run(x, y, first, guard=None, step=None, out=None):
    """One call on device tensors; returns the records as a numpy structured array (a fresh, pattern-filled out unless one is given)."""
    lib = _lib()
    n, nseg = x.numel(), len(first)
    tab = torch.tensor(first, dtype=torch.int64).cuda()
    ws = torch.empty(lib.mvf_flat_stats_workspace_bytes(n, nseg), dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.full((nseg * 32,), PATTERN, dtype=torch.uint8, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    rc = lib.mvf_flat_segment_stats(P(x), P(y), n, P(tab), nseg, P(out), P(guard), P(step), P(ws), ws.numel(), None)
    assert rc == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(ln.FLAT_STATS_DTYPE)


# ------------------------------------------------------------------------------------------------ 1. against numpy fp64
@pytest.mark.parametrize("offset", [0, 1, 3], ids=lambda o: "off%d" % o)
def test_flat_segment_stats_match_the_fp64_restatement(offset):
    assert FIRST[1] % CHUNK == 0 and FIRST[6] // CHUNK + 2 == (FIRST[7] - 1) // CHUNK and len({f // CHUNK for f in FIRST[2:7]}) == 1
    x, y = _values(N, 1), _values(N, 2)
    y[::7] = x[::7]                                   # exact zeros in the difference
    xd, yd = _device(x, offset), _device(y, offset)
    n_s = ln.lengths(FIRST, N)
    got = _run(xd, None, FIRST)
    ln.assert_stats(got, ln.flat_segment_stats(x, None, FIRST), n_s, "x")
    assert got["absmax"].max() > 1e18 and got["sumsq"].max() > 1e36 and got["n_nan"].sum() == 0 and got["n_inf"].sum() == 0
    again = _run(xd, None, FIRST)
    assert got.tobytes() == again.tobytes()           # bit-identical from run to run
    # the difference mode on the same table; and with y aligned differently from x (the scalar path)
    diff = _run(xd, yd, FIRST)
    ln.assert_stats(diff, ln.flat_segment_stats(x, y, FIRST), n_s, "x - y")
    assert diff.tobytes() == _run(xd, yd, FIRST).tobytes()
    skew = _run(xd, _device(y, (offset + 1) % 4), FIRST)
    ln.assert_stats(skew, ln.flat_segment_stats(x, y, FIRST), n_s, "x - y, skewed")
    zero = _run(xd, xd.clone(), FIRST)
    assert not zero["sumsq"].any() and not zero["absmax"].any() and not zero["n_nan"].any() and not zero["n_inf"].any()


@pytest.mark.parametrize("n,nseg", [(1, 1), (5000, 1), (300, 300), (4100, 4100), (8192, 2)], ids=lambda v: str(v))
def test_flat_segment_stats_edge_tables(n, nseg):
    x = _values(n, 10 + n)
    first = [0] if nseg == 1 else ([0, 4096] if nseg == 2 else list(range(n)))
    for offset in (0, 1):
        got = _run(_device(x, offset), None, first)
        ln.assert_stats(got, ln.flat_segment_stats(x, None, first), ln.lengths(first, n), (n, nseg, offset))


# ------------------------------------------------------------------------------------------------ 2. non-finite values
def test_non_finite_values_are_counted_where_they_are_and_nowhere_else():
    x = _values(N, 3)
    clean = _run(_device(x, 1), None, FIRST)
    bad = x.copy()
    nan, inf = np.float32("nan"), np.float32("inf")
    plant = {FIRST[1]: nan, FIRST[2] - 1: -inf,                # first and last element of segment 1 (its first sits on a chunk boundary)
             FIRST[6]: inf, FIRST[7] - 1: nan,                 # first and last element of segment 6
             CHUNK - 1: inf, CHUNK: -inf,                      # both sides of a chunk boundary inside segment 0
             FIRST[7] + 5000: nan}
    for i, v in plant.items():
        bad[i] = v
    got = _run(_device(bad, 1), None, FIRST)
    ref = ln.flat_segment_stats(bad, None, FIRST)
    ln.assert_stats(got, ref, ln.lengths(FIRST, N), "planted")
    assert got["n_nan"].tolist() == [0, 1, 0, 0, 0, 0, 1, 1] and got["n_inf"].tolist() == [2, 1, 0, 0, 0, 0, 1, 0]
    for k in (2, 3, 4, 5):                                     # neighbours: the bits of the clean run
        assert got[k].tobytes() == clean[k].tobytes(), k
    big = [0, 1, 6, 7]
    assert (got["sumsq"][big] > 0).all() and (got["sumsq"][big] <= clean["sumsq"][big]).all()      # the finite elements are still summed
    # difference mode: inf - inf is a NaN, finite - inf an inf
    y = x.copy()
    y[CHUNK - 1] = inf
    y[FIRST[6]] = -inf
    y[7] = inf
    diff = _run(_device(bad, 3), _device(y, 3), FIRST)
    ln.assert_stats(diff, ln.flat_segment_stats(bad, y, FIRST), ln.lengths(FIRST, N), "planted, x - y")
    assert diff["n_nan"].tolist() == [1, 1, 0, 0, 0, 0, 1, 1] and diff["n_inf"].tolist() == [2, 1, 0, 0, 0, 0, 1, 0]
    # a segment without one finite element
    lone = np.array([1.0, np.nan, np.inf, 2.0], np.float32)
    got = _run(_device(lone, 0), None, [0, 1, 3])
    assert got["sumsq"].tolist() == [1.0, 0.0, 4.0] and got["absmax"].tolist() == [1.0, 0.0, 2.0] and got["n_nan"].tolist() == [0, 1, 0]


# ------------------------------------------------------------------------------------------------ 3. predication
def test_flat_segment_stats_store_nothing_while_the_guard_word_is_clear():
    x = _values(N, 4)
    xd = _device(x, 1)
    ref = ln.flat_segment_stats(x, None, FIRST)
    for flag in (0, 1):
        guard = torch.tensor([flag, 5, 2, 77], dtype=torch.int32, device="cuda")
        out = torch.full((len(FIRST) * 32 + 64,), PATTERN, dtype=torch.uint8, device="cuda")          # a band behind the records
        step = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        before_out, before_step = out.clone(), step.clone()
        got = _run(xd, None, FIRST, guard=guard, step=step[1:2], out=out)
        assert guard.tolist() == [flag, 5, 2, 77]
        assert torch.equal(out[len(FIRST) * 32:], before_out[len(FIRST) * 32:]) and step[0] == before_step[0] and step[2] == before_step[2]
        if flag == 0:
            assert torch.equal(out, before_out) and torch.equal(step, before_step)
        else:
            ln.assert_stats(got[:len(FIRST)], ref, ln.lengths(FIRST, N), "guarded")
            assert int(step[1]) == 77
    # a guard without step_out
    guard = torch.tensor([1, 0, 0, 9], dtype=torch.int32, device="cuda")
    ln.assert_stats(_run(xd, None, FIRST, guard=guard), ref, ln.lengths(FIRST, N), "guard only")


STAT_LENGTHS = (1, 3, 256, 257, 1000)


def _stat_table(seed):
    """A table of a few segments inside one arena with gaps between them; returns (arena, table tensor, per-segment slices)."""
    rng = np.random.RandomState(seed)
    arena = torch.from_numpy(rng.standard_normal(4096).astype(np.float32)).cuda()
    rows, slices, first, at = [], [], 0, 5
    for length in STAT_LENGTHS:
        rows.append((arena.data_ptr() + 4 * at, first))
        slices.append(slice(at, at + length))
        first += length
        at += length + 11
    tab = torch.from_numpy(np.array(rows, dtype=ln.STAT_DTYPE).view(np.uint8)).cuda()
    return arena, tab, slices, first


def test_bn_stats_nonfinite_counts_and_predication():
    lib = _lib()
    arena, tab, slices, n = _stat_table(5)
    nan, inf = float("nan"), float("inf")
    arena[slices[0].start] = nan                                   # the segment of length 1
    arena[slices[2].start], arena[slices[2].stop - 1], arena[slices[2].start + 64] = inf, -inf, nan
    arena[slices[4].stop - 1] = nan
    arena[slices[1].stop], arena[slices[3].start - 1] = nan, inf   # in the gaps: nobody's
    want = ln.bn_stats_nonfinite([arena[s].cpu().numpy() for s in slices])
    assert want.tolist() == [1, 0, 3, 0, 1]
    for flag in (None, 0, 1):
        guard = None if flag is None else torch.tensor([flag, 1, 1, 4], dtype=torch.int32, device="cuda")
        counts = torch.full((len(STAT_LENGTHS) + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        before = counts.clone()
        rc = lib.mvf_bn_stats_nonfinite(tab.data_ptr(), len(STAT_LENGTHS), n, counts[1:].data_ptr(), None if guard is None else guard.data_ptr(), None)
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert counts[0] == before[0] and counts[-1] == before[-1]
        if flag == 0:
            assert torch.equal(counts, before)
        else:
            assert counts[1:-1].tolist() == want.tolist(), flag


# ------------------------------------------------------------------------------------------------ engines
LR = 0.01


def _model():
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().train()


def _batch(seed, clips=2):
    return (torch.from_numpy(synth.synth_clip_batch(clips, 4, 64, 64, seed=seed)).cuda(), torch.from_numpy(synth.synth_labels(clips, seed=seed)).cuda())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _expected_rows(m, grad_of, before, scale):
    """The restatement per parameter from tensors read back around the step: {name: (grad stats, weight stats, update stats)} with one segment each."""
    out = {}
    for name, p in m.named_parameters():
        g, w0, w1 = grad_of[name], before[name], p.detach().cpu().numpy().reshape(-1)
        out[name] = (ln.flat_segment_stats(g, None, [0])[0], ln.flat_segment_stats(w0, None, [0])[0], ln.flat_segment_stats(w1, w0, [0])[0])
    return out


def _check_measured(m, eng, fig, grad_of, before, scale):
    assert list(fig["params"]) == [n for n, _ in m.named_parameters()]
    assert fig["grad_scale"] == scale and fig["step"] == eng.steps
    want = _expected_rows(m, grad_of, before, scale)
    trained_sumsq = 0.0
    for name, p in m.named_parameters():
        row, (g, w, u), bound = fig["params"][name], want[name], float(ln.sumsq_bound(p.numel()))
        # norms are square roots of sums within `bound` of each other: half the relative error, and one rounding of the root and of the scale each
        for key, ref in (("grad_norm", np.sqrt(g["sumsq"]) * scale), ("weight_norm", np.sqrt(w["sumsq"])), ("update_norm", np.sqrt(u["sumsq"]))):
            assert abs(row[key] - ref) <= (bound + 4 * ln.EPS) * ref, (name, key, row[key], ref)
        assert row["grad_absmax"] == float(g["absmax"]) * scale, name
        assert (row["grad_nan"], row["grad_inf"], row["weight_nonfinite"], row["update_nonfinite"]) == (0, 0, 0, 0), name
        assert row["trained"] == p.requires_grad, name
        if row["weight_norm"] > 0:
            assert abs(row["update_ratio"] - row["update_norm"] / row["weight_norm"]) <= 4 * ln.EPS * row["update_ratio"], name
        if row["trained"]:
            trained_sumsq += (row["grad_norm"] / scale) ** 2
    assert any(r["update_norm"] > 0 for r in fig["params"].values())
    norm = float(eng.norm_out[0])
    assert abs(np.sqrt(trained_sumsq) * scale - norm) <= 1e-5 * norm, (np.sqrt(trained_sumsq) * scale, norm)


@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
def test_a_measured_step_gives_the_restatement_of_gradient_weight_and_update(optimizer):
    m = _model()
    eng = m.train_engine(dtype=torch.bfloat16, optimizer=optimizer, lr=LR)
    eng.enable_layer_stats(on_skip=False)
    assert eng.layer_stats() is None
    imgs, labels = _batch(200)
    eng.train_step(imgs.clone(), labels.clone(), lr=LR)          # an unmeasured step first: the measured one is not the engine's first
    assert eng.layer_stats() is None
    eng.measure_layer_stats()
    eng.forward(imgs, labels)
    eng.backward()
    torch.cuda.synchronize()
    grad_of = {n: eng.grad_of(p).detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()}
    before = {n: p.detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()}
    eng.step(lr=LR)
    fig = eng.layer_stats()
    _check_measured(m, eng, fig, grad_of, before, 1.0)
    eng.train_step(imgs.clone(), labels.clone(), lr=LR)          # not armed: the figures stay those of the measured step
    assert eng.layer_stats()["step"] == fig["step"] == 2


def test_a_measured_accumulated_step_sees_the_mean_gradient():
    m = _model()
    eng = m.train_engine(dtype=torch.bfloat16, lr=LR)
    eng.enable_layer_stats(on_skip=False)
    eng.measure_layer_stats()
    for seed in (210, 211):
        imgs, labels = _batch(seed)
        eng.accumulate_step(imgs, labels)
    torch.cuda.synchronize()
    grad_of = {n: eng.acc_grad_of(p).detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()}
    before = {n: p.detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()}
    eng.apply_accumulated(lr=LR)
    _check_measured(m, eng, eng.layer_stats(), grad_of, before, 0.5)


def _state(m, eng):
    torch.cuda.synchronize()
    return [_bits(t.detach()).clone() for t in [eng.flat_params, eng.flat_mom] + list(m.buffers())]


def test_three_steps_with_everything_enabled_leave_the_bits_of_a_twin_without():
    (ma, mb) = _model(), _model()
    ea, eb = ma.train_engine(dtype=torch.bfloat16, lr=LR), mb.train_engine(dtype=torch.bfloat16, lr=LR)
    ea.enable_step_guard()
    eb.enable_step_guard()
    ea.enable_layer_stats(on_skip=True)
    for i in range(3):
        imgs, labels = _batch(220 + i)
        ea.measure_layer_stats()
        la, lb = ea.train_step(imgs.clone(), labels.clone(), lr=LR), eb.train_step(imgs.clone(), labels.clone(), lr=LR)
        sa, sb = _state(ma, ea), _state(mb, eb)
        assert len(sa) == len(sb) and all(torch.equal(a, b) for a, b in zip(sa, sb)), i
        assert torch.equal(_bits(la), _bits(lb)), i
        assert ea.layer_stats()["step"] == i + 1
    assert ea.last_skip() is None and eb._lstats is None
    assert ea.guard_state() == eb.guard_state() == dict(skipped_last=False, skipped=0, consecutive=0, steps=3)


def _mid_parameter(m):
    names = [n for n, _ in m.named_parameters()]
    name = [n for n in names if "layer2" in n and n.endswith("conv2.weight")][0]
    return name, dict(m.named_parameters())[name]


def test_last_skip_names_where_the_step_went_wrong():
    m = _model()
    eng = m.train_engine(dtype=torch.bfloat16, lr=LR)
    with pytest.raises(RuntimeError, match="enable_step_guard"):
        eng.enable_layer_stats(on_skip=True)
    with pytest.raises(RuntimeError, match="enable_layer_stats"):
        eng.last_skip()
    eng.enable_step_guard()
    eng.enable_layer_stats(on_skip=True)
    imgs, labels = _batch(230)
    eng.train_step(imgs.clone(), labels.clone(), lr=LR)
    assert eng.last_skip() is None                                # a good step leaves no record
    # 1. one NaN input pixel: the forward, at the stem's BatchNorm; the statistics go back to the snapshot behind the scan
    stats_before = [_bits(b.detach()).clone() for b in m.buffers()]
    bad = imgs.clone()
    bad[0, 1, 2, 17, 29] = float("nan")
    eng.train_step(bad, labels.clone(), lr=LR)
    rec = eng.last_skip()
    stem = {id(mod): n for n, mod in m.named_modules()}[id(eng.stem_bn.mod)]
    assert (rec["step"], rec["kind"], rec["where"]) == (2, "forward", stem), rec
    assert rec["detail"]["batchnorms_hit"] >= 1 and set(rec["detail"]["statistics"]) <= {stem + ".running_mean", stem + ".running_var"}
    # (how far the NaN travels behind the stem is the network's business: a ReLU taken as fmaxf(x, 0) stops it)
    assert all(torch.equal(a, _bits(b.detach())) for a, b in zip(stats_before, m.buffers()))
    assert eng.guard_state() == dict(skipped_last=True, skipped=1, consecutive=1, steps=2)
    # 2. one NaN in one element of a mid-network parameter's gradient, between backward() and step()
    name, p = _mid_parameter(m)
    eng.forward(imgs, labels)
    eng.backward()
    eng.grad_of(p).view(-1)[p.numel() // 2] = float("nan")
    eng.step(lr=LR)
    rec = eng.last_skip()
    assert (rec["step"], rec["kind"], rec["where"]) == (3, "backward", name), rec
    assert (rec["detail"]["n_nan"], rec["detail"]["n_inf"], rec["detail"]["parameters_hit"]) == (1, 0, 1)
    # 3. one finite 1e30 there: the sum of squares leaves fp32
    eng.forward(imgs, labels)
    eng.backward()
    eng.grad_of(p).view(-1)[p.numel() // 2] = 1e30
    eng.step(lr=LR)
    rec = eng.last_skip()
    assert (rec["step"], rec["kind"], rec["where"]) == (4, "norm_overflow", name), rec
    assert rec["detail"]["absmax"] == float(np.float32(1e30))
    assert eng.guard_state()["skipped"] == 3
    # 4. the record survives a following good step
    eng.train_step(imgs.clone(), labels.clone(), lr=LR)
    assert eng.guard_state() == dict(skipped_last=False, skipped=3, consecutive=0, steps=5)
    assert eng.last_skip() == rec
    assert all(bool(torch.isfinite(t).all()) for t in (eng.flat_params, eng.flat_mom))


def test_an_engine_that_never_enables_the_option_calls_none_of_the_new_entry_points():
    new = {"mvf_flat_segment_stats", "mvf_flat_stats_workspace_bytes", "mvf_bn_stats_nonfinite"}
    m = _model()
    eng = m.train_engine(lr=LR)
    eng.enable_step_guard()
    imgs, labels = _batch(240)

    def one_step():
        with library_names(eng) as names:
            eng.train_step(imgs.clone(), labels.clone(), lr=LR)
        return names
    assert not new & set(one_step()) and eng._lstats is None
    eng.enable_layer_stats(on_skip=True)
    eng.train_step(imgs.clone(), labels.clone(), lr=LR)
    names = [n for n in one_step() if n in new or n == "mvf_bn_stats_restore"]
    assert names == ["mvf_flat_segment_stats", "mvf_bn_stats_nonfinite", "mvf_bn_stats_restore"], names          # the scan BEFORE the restore
    eng.disable_layer_stats()
    assert not new & set(one_step())
    with pytest.raises(RuntimeError, match="enable_layer_stats"):
        eng.measure_layer_stats()
