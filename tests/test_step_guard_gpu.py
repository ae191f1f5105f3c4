"""GPU: the non-finite step guard -- mvf_sgd_step_guarded (csrc/optim.hip), mvf_bn_stats_snapshot / mvf_bn_stats_restore (csrc/precise_bn.hip) and the
engine / runner / checkpoint layers above them (TrainEngine.enable_step_guard, guard_state, Runner(nonfinite_guard=...)).

Everything is compared as bit patterns (int32 / int64 views) unless a test says otherwise: the guard adds no arithmetic, so there is no tolerance to state.
With the flag clear the guarded step IS the plain step; with the flag set nothing is stored; after a skipped step the model, the optimizer state and the
average are what they were before it."""
import numpy as np
import pytest
import torch

from helpers import library_names
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 5000, 262147, 1048579]          # the last: past one sweep of the update kernel's capped grid (4096 x 256 threads)
LR, MOM, WD, MAX_NORM, EMA_M = 0.01, 0.9, 1e-4, 40.0, 0.25
BAND = -123.25
SEG_DTYPE = np.dtype([("first", "<i8"), ("lr_mult", "<f4"), ("decay_mult", "<f4")])      # mvf_sgd_segment_t
STAT_DTYPE = np.dtype([("ptr", "<u8"), ("first", "<i8")])                                # mvf_stat_segment_t
# starts inside and on the edges of a workgroup's 256-element run, two excluded segments (lr_mult < 0); cut to the segments that start below n
SEGMENTS = ((0, 1.0, 1.0), (7, 2.0, 0.0), (256, -1.0, 0.0), (257, 1.0, 0.0), (1000, 0.5, 0.5), (1001, -1.0, 1.0), (70000, 1.0, 1.0), (262146, 2.0, 0.0))


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib


def _bits(t):
    return t.view(torch.int32) if t.is_floating_point() else t


def _segments(n):
    segs = [s for s in SEGMENTS if s[0] < n]
    firsts = [s[0] for s in segs] + [n]
    excl = torch.from_numpy(np.repeat(np.array([s[1] < 0 for s in segs]), np.diff(firsts))).cuda()
    return segs, torch.from_numpy(np.array(segs, dtype=SEG_DTYPE).view(np.uint8)).cuda(), excl


class _Operands(object):
    """params / momentum / ema / grads of n elements, each one element into an allocation of its own (4-byte aligned only, as the engine's flat_*[off:]) with a
    guard band on either side; the initial values are kept for rewinding."""

    def __init__(self, n, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.n = n
        self.init = [torch.randn(n, generator=gen, device="cuda") for _ in range(3)]
        self.full = [torch.full((n + 2,), BAND, device="cuda") for _ in range(4)]
        self.p, self.b, self.e, self.g = [f[1:n + 1] for f in self.full]
        self.norm = torch.zeros(2, device="cuda")
        self.guard = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(_lib().mvf_sgd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        g = torch.randn(n, generator=gen, device="cuda")
        self.g0 = g * (100.0 / float(g.double().norm()))          # norm 100 against max_norm 40: the step clips
        self.rewind()

    def rewind(self):
        for dst, src in zip((self.p, self.b, self.e), self.init):
            dst.copy_(src)
        self.g.copy_(self.g0)
        self.norm.fill_(float("nan"))
        self.guard.zero_()

    def state(self):
        return [_bits(f).clone() for f in self.full[:3]]          # whole allocations: the bands too

    def plain(self, tab, nseg, nesterov, ema, first):
        lib, P = _lib(), (lambda t: t.data_ptr())
        head = (P(self.p), P(self.g), P(self.b), self.n, 1.0, MAX_NORM, LR, MOM, WD, first)
        tail = (P(self.norm), P(self.ws), self.ws.numel(), None)
        avg = (P(self.e), EMA_M) if ema else ()
        if tab is None:
            f = lib.mvf_sgd_nesterov_step_ema if ema else lib.mvf_sgd_nesterov_step
            rc = f(*(head + avg + tail))
        else:
            f = lib.mvf_sgd_step_segments_ema if ema else lib.mvf_sgd_step_segments
            rc = f(*(head + (nesterov, P(tab), nseg) + avg + tail))
        assert rc == 0, lib.mvf_last_error()

    def guarded(self, tab, nseg, nesterov, ema, first):
        lib, P = _lib(), (lambda t: t.data_ptr())
        rc = lib.mvf_sgd_step_guarded(P(self.p), P(self.g), P(self.b), self.n, 1.0, MAX_NORM, LR, MOM, WD, first, nesterov, None if tab is None else P(tab), nseg,
                                      P(self.e) if ema else None, EMA_M, P(self.guard), P(self.norm), P(self.ws), self.ws.numel(), None)
        assert rc == 0, lib.mvf_last_error()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. finite gradients: the guarded step IS the plain step
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "n%d" % n)
def test_finite_gradients_give_the_bits_of_the_four_plain_entry_points(n):
    ops = _Operands(n, 11 + n)
    segs, tab, _ = _segments(n)
    for form in ("flat", "segments"):
        t, ns = (None, 0) if form == "flat" else (tab, len(segs))
        for nesterov in (0, 1):
            for ema in (False, True):
                for first in (0, 1):
                    what = (form, nesterov, ema, first)
                    ops.rewind()
                    before = ops.state()
                    ops.plain(t, ns, nesterov, ema, first)
                    want, want_norm = ops.state(), _bits(ops.norm).clone()
                    ops.rewind()
                    ops.guarded(t, ns, nesterov, ema, first)          # (the flat form ignores `nesterov`: both values must give mvf_sgd_nesterov_step)
                    assert _same(ops.state(), want), what
                    assert torch.equal(_bits(ops.norm), want_norm), what
                    assert ops.guard.tolist() == [0, 0, 0, 1], what
                    assert not torch.equal(want[0], before[0]) and not torch.equal(want[1], before[1]), what          # the step did move something
                    assert torch.equal(want[2], before[2]) != ema, what
                    assert float(ops.norm[1]) < 1.0, what                      # ... and it clipped
    assert bool((ops.full[3][0] == BAND) & (ops.full[3][-1] == BAND))


# ------------------------------------------------------------------------------------------------ 2. one non-finite value: nothing is stored
def _positions(n):
    pos = {0, n - 1, (n - 1) // 256 * 256 + ((n - 1) % 256) // 2}          # element 0, the last, one inside the last partial block
    if n > 1048577:
        pos.add(1048577)                                                    # one past element 1048576: the second sweep of the update kernel
    return sorted(pos)


@pytest.mark.parametrize("n", SIZES, ids=lambda n: "n%d" % n)
def test_one_non_finite_gradient_value_skips_the_step_and_stores_nothing(n):
    ops = _Operands(n, 23 + n)
    segs, tab, excl = _segments(n)
    before = ops.state()
    cases = [(v, k) for v in (float("nan"), float("inf"), float("-inf"), 3e19) for k in _positions(n)]
    for form in ("flat", "segments"):
        t, ns = (None, 0) if form == "flat" else (tab, len(segs))
        for value, k in cases:
            if form == "segments" and bool(excl[k]):
                continue                                   # (inside an excluded segment the value does not enter the norm: test 3)
            for ema in (True, False):
                what = (form, value, k, ema)
                ops.guard.zero_()
                ops.norm.zero_()
                ops.g[k] = value
                ops.guarded(t, ns, 1, ema, 0)
                ops.g[k] = ops.g0[k]
                assert ops.guard.tolist() == [1, 1, 1, 1], what
                assert not bool(torch.isfinite(ops.norm[0])), what          # the honest value: nan, or inf where the sum of squares left fp32
                assert _same(ops.state(), before), what
    # every gradient finite and 3e19: each square is beyond fp32 already
    ops.guard.zero_()
    ops.g.fill_(3e19)
    ops.guarded(None, 0, 1, True, 1)
    assert ops.guard.tolist() == [1, 1, 1, 1] and bool(torch.isinf(ops.norm[0])) and _same(ops.state(), before)


# ------------------------------------------------------------------------------------------------ 3. excluded segments stay outside the decision
@pytest.mark.parametrize("n", [5000, 262147], ids=lambda n: "n%d" % n)
def test_a_nan_inside_an_excluded_segment_is_not_skipped(n):
    ops = _Operands(n, 31 + n)
    segs, tab, excl = _segments(n)
    where = torch.nonzero(excl).reshape(-1)
    assert where.numel() >= 2
    for ema in (False, True):
        for nesterov in (0, 1):
            ops.rewind()
            ops.g[where] = float("nan")
            before = ops.state()
            ops.plain(tab, len(segs), nesterov, ema, 0)
            want, want_norm = ops.state(), _bits(ops.norm).clone()
            ops.rewind()
            ops.g[where] = float("nan")
            ops.guarded(tab, len(segs), nesterov, ema, 0)
            assert ops.guard.tolist() == [0, 0, 0, 1]
            assert _same(ops.state(), want) and torch.equal(_bits(ops.norm), want_norm)
            assert bool(torch.isfinite(ops.norm).all()) and not torch.equal(want[0], before[0])
            assert bool(torch.isfinite(ops.p).all())


# ------------------------------------------------------------------------------------------------ 4. the counters
def test_counter_sequence_good_bad_bad_good():
    n = 5000
    ops = _Operands(n, 41)
    flags, states = [], []
    for bad in (False, True, True, False):
        ops.g.copy_(ops.g0)
        if bad:
            ops.g[n // 2] = float("nan")
        prev = ops.state()
        ops.guarded(None, 0, 1, True, 0)
        flags.append(ops.guard.tolist())
        states.append(_same(ops.state(), prev))
    assert flags == [[0, 0, 0, 1], [1, 1, 1, 2], [1, 2, 2, 3], [0, 2, 0, 4]]
    assert states == [False, True, True, False]


# ------------------------------------------------------------------------------------------------ 5. snapshot and conditional restore
SEG_WORDS = (1, 3, 256, 257, 1000)
NAN_BITS = (0x7fc12345, 0xffc00001 - (1 << 32), 0x7f800001, -(1 << 31))          # NaN payloads (quiet, negative, signalling) and -0.0, as int32


def _random_words(k, gen):
    w = torch.randint(-(1 << 31), (1 << 31) - 1, (k,), generator=gen, dtype=torch.int64).to(torch.int32)
    w[:min(k, len(NAN_BITS))] = torch.tensor(NAN_BITS[:min(k, len(NAN_BITS))], dtype=torch.int32)
    return w


@pytest.mark.parametrize("ncount", [3, 70])
def test_snapshot_then_restore_moves_words_only_when_the_flag_is_set(ncount):
    lib = _lib()
    gen = torch.Generator().manual_seed(50 + ncount)
    n = sum(SEG_WORDS)
    # one arena of 32-bit words: every segment starts at an ODD word offset, 5 words of band in front of each and behind the last
    starts, off = [], 5
    for k in SEG_WORDS:
        off += 1 - off % 2
        starts.append(off)
        off += k + 5
    arena = _random_words(off, gen).cuda()
    firsts = np.concatenate([[0], np.cumsum(SEG_WORDS)[:-1]])
    table = np.zeros(len(SEG_WORDS), STAT_DTYPE)
    table["ptr"], table["first"] = [arena.data_ptr() + 4 * s for s in starts], firsts
    tab = torch.from_numpy(table.view(np.uint8)).cuda()
    inside = torch.zeros(off, dtype=torch.bool)
    for s, k in zip(starts, SEG_WORDS):
        inside[s:s + k] = True
    inside = inside.cuda()
    flat_full = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    flat = flat_full[3:3 + n]                            # an odd offset too
    cnt_full = torch.randint(-(1 << 62), 1 << 62, (ncount + 4,), generator=gen, dtype=torch.int64).cuda()
    cpy_full = torch.full((ncount + 4,), -5, dtype=torch.int64, device="cuda")
    cnt, cpy = cnt_full[2:2 + ncount], cpy_full[2:2 + ncount]
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    P = lambda t: t.data_ptr()       # noqa: E731
    # the table's content is validated once, by an exchange call (a gather into a scratch array)
    scratch = torch.zeros(n, dtype=torch.float32, device="cuda")
    assert lib.mvf_bn_stats_exchange(P(tab), len(SEG_WORDS), n, P(scratch), 0, None) == 0, lib.mvf_last_error()
    arena0, cnt0 = arena.clone(), cnt_full.clone()
    assert lib.mvf_bn_stats_snapshot(P(tab), len(SEG_WORDS), n, P(flat), P(cnt), ncount, P(cpy), None) == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(arena, arena0) and torch.equal(cnt_full, cnt0)                                   # the sources are only read
    assert torch.equal(flat, arena0[inside]) and torch.equal(flat, scratch.view(torch.int32))           # segment order = arena order here
    assert bool((flat_full[:3] == 77).all()) and bool((flat_full[3 + n:] == 77).all())
    assert torch.equal(cpy, cnt0[2:2 + ncount]) and bool((cpy_full[:2] == -5).all()) and bool((cpy_full[2 + ncount:] == -5).all())
    snap_flat, snap_cpy = flat_full.clone(), cpy_full.clone()
    # the step moves everything: segments, bands and counters
    arena1, cnt1 = _random_words(off, gen).cuda().flip(0).contiguous(), cnt0 + 1
    for flag, total in ((0, 9), (1, 9), (7, 0)):
        arena.copy_(arena1)
        cnt_full.copy_(cnt1)
        guard.copy_(torch.tensor([flag, total, 2, 5], dtype=torch.int32))
        assert lib.mvf_bn_stats_restore(P(tab), len(SEG_WORDS), n, P(flat), P(cnt), ncount, P(cpy), P(guard), None) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert torch.equal(flat_full, snap_flat) and torch.equal(cpy_full, snap_cpy) and guard.tolist() == [flag, total, 2, 5]
        assert torch.equal(arena[~inside], arena1[~inside]), flag                                       # bands: never
        assert torch.equal(cnt_full[:2], cnt1[:2]) and torch.equal(cnt_full[2 + ncount:], cnt1[2 + ncount:]), flag
        if flag == 0:
            assert torch.equal(arena, arena1) and torch.equal(cnt_full, cnt1)                           # nothing is stored anywhere
        else:
            assert torch.equal(arena[inside], arena0[inside]) and torch.equal(cnt, cnt0[2:2 + ncount]), flag
    # the statistics alone
    arena.copy_(arena1)
    assert lib.mvf_bn_stats_restore(P(tab), len(SEG_WORDS), n, P(flat), None, 0, None, P(guard), None) == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(arena[inside], arena0[inside]) and torch.equal(arena[~inside], arena1[~inside])


# ------------------------------------------------------------------------------------------------ engines
def _model(dropout=0.0, **backbone):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=dropout)
    cfg["backbone"].update(backbone)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().train()


def _batch(seed, clips=2):
    return (torch.from_numpy(synth.synth_clip_batch(clips, 4, 64, 64, seed=seed)).cuda(), torch.from_numpy(synth.synth_labels(clips, seed=seed)).cuda())


def _poisoned(seed, value):
    imgs, labels = _batch(seed)
    imgs[0, 1, 2, 17, 29] = value
    return imgs, labels


def _engine(dtype, guard):
    m = _model()
    eng = m.train_engine(dtype=dtype)
    eng.enable_ema(momentum=EMA_M, warmup_steps=0)
    if guard:
        eng.enable_step_guard()
    return m, eng


def _state(m, eng):
    """Bit patterns of everything a step may move: parameters, momentum, the average, every buffer (running statistics and num_batches_tracked)."""
    torch.cuda.synchronize()
    return [_bits(t.detach()).clone() for t in [eng.flat_params, eng.flat_mom, eng.flat_ema] + list(m.buffers())]


def _values(m, eng):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in [eng.flat_params, eng.flat_mom, eng.flat_ema] + list(m.buffers())]


def _all_finite(m, eng):
    return all(bool(torch.isfinite(t).all()) for t in [eng.flat_params, eng.flat_mom, eng.flat_ema] + [b for b in m.buffers() if b.is_floating_point()])


def _run(eng, batches):
    return [eng.train_step(imgs.clone(), labels.clone(), lr=LR) for imgs, labels in batches]


DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
_CONTROL = {}


def _control(dtype):
    """The engine that never met a bad batch: g1, g2, guard off.  Computed once per dtype, read by every variant of the invariant test."""
    if dtype not in _CONTROL:
        m, eng = _engine(dtype, guard=False)
        initial = _state(m, eng)
        losses = _run(eng, [_batch(110), _batch(111)])
        _CONTROL[dtype] = dict(initial=initial, state=_state(m, eng), values=_values(m, eng), losses=[_bits(l).clone() for l in losses], steps=eng.steps)
    return _CONTROL[dtype]


# ------------------------------------------------------------------------------------------------ 6. the guard does not perturb training
@DTYPES
def test_three_finite_steps_are_bit_equal_with_the_guard_on_and_off(dtype):
    (ma, ea), (mb, eb) = _engine(dtype, guard=True), _engine(dtype, guard=False)
    assert _same(_state(ma, ea), _state(mb, eb))
    for i in range(3):
        imgs, labels = _batch(100 + i)
        la, lb = ea.train_step(imgs.clone(), labels.clone(), lr=LR), eb.train_step(imgs.clone(), labels.clone(), lr=LR)
        assert _same(_state(ma, ea), _state(mb, eb)), i
        assert torch.equal(_bits(la), _bits(lb)) and bool(torch.isfinite(la).all()), i
    assert ea.guard_state() == dict(skipped_last=False, skipped=0, consecutive=0, steps=3)
    assert eb._guard is None and ea.steps == eb.steps == 3


# ------------------------------------------------------------------------------------------------ 7. the invariant
@DTYPES
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_skipped_step_leaves_the_run_as_if_the_batch_had_never_been_drawn(dtype, value):
    """Engine A: g1, bad, g2 with the guard on.  The control: g1, g2.  Without the guard the bad step writes NaN into every parameter, every momentum element, the
    average and every running statistic -- this test cannot pass there."""
    ctl = _control(dtype)
    m, eng = _engine(dtype, guard=True)
    assert _same(_state(m, eng), ctl["initial"])
    l1, = _run(eng, [_batch(110)])
    after_g1 = _state(m, eng)
    _run(eng, [_poisoned(110, value)])
    assert _same(_state(m, eng), after_g1)                      # parameters, momentum, average, statistics, counters: the bits of before the step
    st = eng.guard_state()
    assert st == dict(skipped_last=True, skipped=1, consecutive=1, steps=2), st
    assert not bool(torch.isfinite(eng.norm_out[0]))            # honestly reported
    l2, = _run(eng, [_batch(111)])
    assert _same(_state(m, eng), ctl["state"])
    assert torch.equal(_bits(l1), ctl["losses"][0]) and torch.equal(_bits(l2), ctl["losses"][1])
    st = eng.guard_state()
    assert st == dict(skipped_last=False, skipped=1, consecutive=0, steps=3), st
    assert eng.steps == 3 and ctl["steps"] == 2 and eng.ema_updates == 3          # the host counts attempted steps
    assert _all_finite(m, eng)


@DTYPES
def test_a_skipped_very_first_step_is_harmless(dtype):
    """bad, g1, g2 against g1, g2: the first real update runs as a later step on a zero momentum buffer, momentum * 0 + d against d -- equal VALUES, the sign
    of a zero may differ."""
    ctl = _control(dtype)
    m, eng = _engine(dtype, guard=True)
    _run(eng, [_poisoned(110, float("nan"))])
    assert _same(_state(m, eng), ctl["initial"])
    _run(eng, [_batch(110), _batch(111)])
    got = _values(m, eng)
    assert len(got) == len(ctl["values"]) and all(torch.equal(a, b) for a, b in zip(got, ctl["values"]))
    assert eng.guard_state() == dict(skipped_last=False, skipped=1, consecutive=0, steps=3)


def test_a_skipped_step_under_a_live_launch_plan():
    """Enough steps that forward + backward replay from a launch plan: the snapshot is taken in front of the replay, never inside a recording."""
    good = [_batch(120 + i) for i in range(6)]
    (ma, ea), (mb, eb) = _engine(torch.bfloat16, guard=True), _engine(torch.bfloat16, guard=False)
    _run(ea, good[:5])
    _run(eb, good[:5])
    assert any(st["plan"] is not None for st in ea._plans.values()) and any(st["plan"] is not None for st in eb._plans.values())
    assert _same(_state(ma, ea), _state(mb, eb))
    before = _state(ma, ea)
    _run(ea, [_poisoned(125, float("nan"))])
    assert _same(_state(ma, ea), before)
    la, = _run(ea, good[5:])
    lb, = _run(eb, good[5:])
    assert _same(_state(ma, ea), _state(mb, eb)) and torch.equal(_bits(la), _bits(lb))
    assert ea.guard_state() == dict(skipped_last=False, skipped=1, consecutive=0, steps=7)


# ------------------------------------------------------------------------------------------------ 8. accumulation
@DTYPES
def test_one_poisoned_micro_batch_drops_the_whole_group(dtype):
    (ma, ea), (mb, eb) = _engine(dtype, guard=True), _engine(dtype, guard=False)
    first, second = [_batch(130 + i) for i in range(3)], [_batch(140 + i) for i in range(3)]
    for eng in (ea, eb):                                     # a clean group on both: the bad group is not the first optimizer step
        eng.train_step_accumulated([(i.clone(), l.clone()) for i, l in first], lr=LR)
    before = _state(ma, ea)
    assert _same(before, _state(mb, eb))
    bad = [_batch(150), _poisoned(151, float("nan")), _batch(152)]
    ea.train_step_accumulated(bad, lr=LR)
    assert _same(_state(ma, ea), before)                     # the statistics are those of before the group's FIRST micro-step
    assert ea.guard_state() == dict(skipped_last=True, skipped=1, consecutive=1, steps=2)
    la = ea.train_step_accumulated([(i.clone(), l.clone()) for i, l in second], lr=LR)
    lb = eb.train_step_accumulated([(i.clone(), l.clone()) for i, l in second], lr=LR)
    assert _same(_state(ma, ea), _state(mb, eb)) and torch.equal(_bits(la), _bits(lb))
    assert not _same(_state(ma, ea), before)
    assert ea.guard_state() == dict(skipped_last=False, skipped=1, consecutive=0, steps=3)


# ------------------------------------------------------------------------------------------------ 9. runner, checkpoint
def _loader(batches):
    return [dict(img_group=i, label=l) for i, l in batches]


def test_runner_stops_after_max_consecutive_skips_with_the_model_intact(tmp_path):
    from mvfnet_amd.runner import Runner
    lines = []
    m = _model()
    run = Runner(m, work_dir=str(tmp_path), lr=LR, log_interval=1, logger=lines.append, ema=dict(momentum=EMA_M), nonfinite_guard=dict(max_consecutive=2))
    eng = run.engine
    initial = _state(m, eng)
    try:
        run.train_epoch(_loader([_poisoned(160 + i, float("nan")) for i in range(4)]))
        raised = None
    except FloatingPointError as e:
        # on entry to the handler: nothing has been poisoned
        raised = str(e)
        assert _all_finite(m, eng) and _same(_state(m, eng), initial)
    assert raised is not None and "2 consecutive" in raised and "iter 1 and iter 2" in raised, raised
    assert run.iter == 2 and run.epoch == 0
    assert len(lines) == 1 and lines[0].endswith("skipped 1"), lines


def test_runner_logs_the_count_and_checkpoints_carry_it(tmp_path):
    import os
    from mvfnet_amd.runner import Runner
    lines = []
    m = _model()
    run = Runner(m, work_dir=str(tmp_path), lr=LR, log_interval=1, logger=lines.append, nonfinite_guard={})
    assert run.nonfinite_guard == dict(max_consecutive=100)
    run.train_epoch(_loader([_batch(170), _batch(171)]))
    assert len(lines) == 2 and all(line.endswith("skipped 0") for line in lines), lines
    run.train_epoch(_loader([_poisoned(172, float("inf")), _batch(173)]))
    assert lines[2].endswith("skipped 1") and lines[3].endswith("skipped 1"), lines
    path = run.save_checkpoint()
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert (ckpt["meta"]["epoch"], ckpt["meta"]["iter"], ckpt["meta"]["skipped_steps"]) == (2, 4, 1)
    m2 = _model()
    run2 = Runner(m2, work_dir=str(tmp_path), lr=LR, logger=lines.append, nonfinite_guard=dict(max_consecutive=5))
    assert run2.engine.guard_state()["skipped"] == 0
    run2.resume(path)
    assert run2.engine.guard_state() == dict(skipped_last=False, skipped=1, consecutive=0, steps=0) and run2.iter == 4
    # a checkpoint without the entry loads as before, and a runner without the guard writes the meta it always wrote
    del ckpt["meta"]["skipped_steps"]
    bare = os.path.join(str(tmp_path), "bare.pth")
    torch.save(ckpt, bare)
    m3 = _model()
    run3 = Runner(m3, work_dir=str(tmp_path), lr=LR, logger=lines.append, nonfinite_guard={})
    run3.resume(bare)
    assert run3.engine.guard_state()["skipped"] == 0 and run3.iter == 4
    run4 = Runner(m3, work_dir=str(tmp_path), lr=LR, logger=lines.append)
    run4.engine.disable_step_guard()
    run4.resume(path)
    run4.epoch = 7
    meta = torch.load(run4.save_checkpoint(), map_location="cpu", weights_only=False)["meta"]
    assert (meta["epoch"], meta["iter"]) == (7, 4) and "skipped_steps" not in meta


# ------------------------------------------------------------------------------------------------ 10. never enabled
NEW_ENTRY_POINTS = {"mvf_sgd_step_guarded", "mvf_bn_stats_snapshot", "mvf_bn_stats_restore"}


def _names_of_one_step(eng, imgs, labels):
    with library_names(eng) as names:
        eng.forward(imgs, labels)
        eng.backward()
        eng.step()
    return names


def test_an_engine_that_never_enables_the_guard_calls_none_of_the_new_entry_points():
    m = _model()
    eng = m.train_engine()
    imgs, labels = _batch(180)
    optimizer = lambda names: [n for n in names if "sgd" in n and "workspace" not in n]          # noqa: E731
    for nesterov, ema, want in ((True, False, "mvf_sgd_nesterov_step"), (False, False, "mvf_sgd_step_segments"), (True, True, "mvf_sgd_nesterov_step_ema"),
                                (False, True, "mvf_sgd_step_segments_ema")):
        eng.nesterov = nesterov
        if ema and eng.flat_ema is None:
            eng.enable_ema(momentum=EMA_M)
        names = _names_of_one_step(eng, imgs, labels)
        assert optimizer(names) == [want] and not NEW_ENTRY_POINTS & set(names), (nesterov, ema)
    assert eng._guard is None
    with pytest.raises(RuntimeError, match="enable_step_guard"):
        eng.guard_state()
    # and with the guard on, the same four paths take the one guarded entry point, between a snapshot and a restore
    eng.enable_step_guard()
    eng.train_step(imgs, labels)                     # (the first snapshot validates the table with an exchange call)
    for nesterov in (True, False):
        eng.nesterov = nesterov
        names = _names_of_one_step(eng, imgs, labels)
        assert optimizer(names) == ["mvf_sgd_step_guarded"], nesterov
        mine = [n for n in names if n in NEW_ENTRY_POINTS]
        assert mine == ["mvf_bn_stats_snapshot", "mvf_sgd_step_guarded", "mvf_bn_stats_restore"], names
        assert "mvf_bn_stats_exchange" not in names
    eng.disable_step_guard()
    names = _names_of_one_step(eng, imgs, labels)
    assert optimizer(names) == ["mvf_sgd_step_segments_ema"] and not NEW_ENTRY_POINTS & set(names)
    torch.cuda.synchronize()
    assert _all_finite(m, eng)
