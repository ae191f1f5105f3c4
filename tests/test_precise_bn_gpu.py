"""GPU: precise BatchNorm -- mvf_bn_stats_accumulate / _finalize / _exchange (csrc/precise_bn.hip) over hand-built segment tables, and the engine / checkpoint /
runner layers above them (TrainEngine.precise_bn, averaged_weights with calibrated statistics, ema['bn_stats'], Runner.resume).

Every comparison is bit for bit, and that is derived, not measured: the kernels add fp32 values converted to fp64 in call order, divide once in fp64 and round
once to fp32 -- the operations of numpy's np.float32(sum(np.float64(x)) / np.float64(k)) in the same order under IEEE arithmetic; the exchange moves 32-bit
words.  The engine tests compare against a twin whose BatchNorm modules carry momentum 1.0 and which runs the existing forward: the forward is bit-reproducible
from run to run, so the calibrated statistics are the fp64-ordered mean of the twin's snapshots exactly."""
import os

import numpy as np
import pytest
import torch

from helpers import library_names
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

SEG_DTYPE = np.dtype([("ptr", "<u8"), ("first", "<i8")])      # mvf_stat_segment_t
LENGTHS = [1, 3, 64, 255, 256, 257, 2048]                     # boundaries inside a workgroup's 256 elements, a length-1 segment, one longer than a workgroup
GUARD = 3                                                     # NaN words before and after every segment (segments are then 4-byte aligned only)
GUARD_BITS = 0x7FC0BEEF
NEW_ENTRY_POINTS = ("mvf_bn_stats_accumulate", "mvf_bn_stats_finalize", "mvf_bn_stats_exchange")


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Segments(object):
    """Segments of the given lengths inside ONE device allocation, each between GUARD NaN words, and the device table over them."""

    def __init__(self, lengths):
        self.lengths = list(lengths)
        self.n = int(sum(lengths))
        self.starts, pos = [], 0
        for k in lengths:
            self.starts.append(pos + GUARD)
            pos += k + 2 * GUARD
        self.host = np.full(pos, GUARD_BITS, np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.float32).copy()).cuda()
        firsts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        rows = np.array([(self.dev.data_ptr() + 4 * s, f) for s, f in zip(self.starts, firsts)], dtype=SEG_DTYPE)
        self.table = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
        self.nseg = len(lengths)

    def upload(self, flat_values):
        """Write the flat fp32 values (length n) into the segments."""
        v = _bits(flat_values)
        pos = 0
        for s, k in zip(self.starts, self.lengths):
            self.host[s:s + k] = v[pos:pos + k]
            pos += k
        self.dev.copy_(torch.from_numpy(self.host.view(np.float32).copy()))

    def download(self):
        """-> (flat values as uint32 bits, True when every guard word is untouched)"""
        got = _bits(self.dev.cpu().numpy())
        mask = np.ones(got.size, bool)
        parts = []
        for s, k in zip(self.starts, self.lengths):
            parts.append(got[s:s + k])
            mask[s:s + k] = False
        return np.concatenate(parts), bool((got[mask] == GUARD_BITS).all())


def _guarded_flat(n, dtype):
    """A flat device array of n elements between GUARD NaN elements -> (whole tensor, pointer of element 0 of the payload)."""
    t = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    return t, t.data_ptr() + GUARD * t.element_size()


def _values(n, seed):
    """fp32 values with denormals, magnitudes near 1e30 of both signs, exact zeros and -0.0 mixed into normal ones."""
    rng = np.random.RandomState(seed)
    v = rng.standard_normal(n).astype(np.float32)
    special = np.array([1e-40, -3e-42, 1.4e-45, 9.7e29, -9.9e29, 1e30, 0.0, -0.0, 1.0, -1e-38], np.float32)
    pick = rng.rand(n) < 0.4
    v[pick] = special[rng.randint(0, special.size, int(pick.sum()))]
    return v


def _check_accumulate_finalize(lengths, ks=(1, 2, 7)):
    lib = _lib()
    seg = _Segments(lengths)
    n = seg.n
    for k in ks:
        what = "lengths %s k=%d" % (lengths if len(lengths) < 9 else "(%d segments)" % len(lengths), k)
        acc_t, acc = _guarded_flat(n, torch.float64)
        acc_t[GUARD:GUARD + n] = 0.0
        ref = np.zeros(n, np.float64)
        for j in range(k):
            x = _values(n, 1000 * k + 10 * j + n % 97)
            seg.upload(x)
            assert lib.mvf_bn_stats_accumulate(seg.table.data_ptr(), seg.nseg, n, acc, None) == 0, lib.mvf_last_error()
            torch.cuda.synchronize()
            ref = ref + x.astype(np.float64)
        got_acc = acc_t.cpu().numpy()
        assert np.array_equal(got_acc[GUARD:GUARD + n].view(np.uint64), ref.view(np.uint64)), "fp64 sums, " + what
        assert np.isnan(got_acc[:GUARD]).all() and np.isnan(got_acc[GUARD + n:]).all(), "accumulator guards, " + what
        want = (ref / np.float64(k)).astype(np.float32)
        last, clean = seg.download()
        assert clean and np.array_equal(last, _bits(x)), "accumulate wrote the segments, " + what
        # a flat destination: the segments keep the last batch's values
        dst_t, dst = _guarded_flat(n, torch.float32)
        assert lib.mvf_bn_stats_finalize(seg.table.data_ptr(), seg.nseg, n, acc, k, dst, None) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        got = dst_t.cpu().numpy()
        assert np.array_equal(_bits(got[GUARD:GUARD + n]), _bits(want)), "finalize into a flat array, " + what
        assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + n:]).all(), "flat guards, " + what
        last, clean = seg.download()
        assert clean and np.array_equal(last, _bits(x)), what
        # NULL: through the table
        assert lib.mvf_bn_stats_finalize(seg.table.data_ptr(), seg.nseg, n, acc, k, None, None) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        got, clean = seg.download()
        assert np.array_equal(got, _bits(want)), "finalize through the table, " + what
        assert clean, "segment guards, " + what
        assert np.array_equal(acc_t.cpu().numpy()[GUARD:GUARD + n].view(np.uint64), ref.view(np.uint64)), "finalize wrote the accumulator, " + what


# ------------------------------------------------------------------------------------------------ 1. accumulate + finalize
def test_accumulate_and_finalize_equal_numpy_fp64_mean_bit_for_bit():
    _check_accumulate_finalize(LENGTHS)


def test_single_segment_of_length_one():
    _check_accumulate_finalize([1])


def test_many_workgroups_and_many_segments():
    """~600 workgroups (no grid-stride loop: one thread per element, the grid is ceil(n / 256)) over 150 segments of mixed lengths: every step of the binary
    search is taken."""
    rng = np.random.RandomState(5)
    _check_accumulate_finalize([int(k) for k in rng.randint(1, 2048, 150)], ks=(2,))


# ------------------------------------------------------------------------------------------------ 2. exchange
def _payloads(n, seed):
    rng = np.random.RandomState(seed)
    v = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0xFF800001, 0x80000000, 0x00000000, 0x00000001, 0x7F800000], np.uint32)      # NaN payloads, sNaN, -0.0, ...
    v[:min(n, special.size)] = special[:min(n, special.size)]
    return rng.permutation(v)


@pytest.mark.parametrize("lengths", [LENGTHS, [1]], ids=["seven_segments", "one_element"])
def test_exchange_modes_move_every_bit(lengths):
    lib = _lib()
    seg = _Segments(lengths)
    n = seg.n
    a, b = _payloads(n, 11), _payloads(n, 12)
    flat_t, flat = _guarded_flat(n, torch.float32)

    def run(mode):
        assert lib.mvf_bn_stats_exchange(seg.table.data_ptr(), seg.nseg, n, flat, mode, None) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        fl = flat_t.cpu().numpy()
        got_seg, clean = seg.download()
        assert clean and np.isnan(fl[:GUARD]).all() and np.isnan(fl[GUARD + n:]).all(), mode
        return got_seg, _bits(fl)[GUARD:GUARD + n]
    seg.upload(a.view(np.float32))
    s, f = run(0)                                    # gather
    assert np.array_equal(s, a) and np.array_equal(f, a)
    flat_t.view(torch.int32)[GUARD:GUARD + n] = torch.from_numpy(b.view(np.int32).copy()).cuda()
    s, f = run(1)                                    # scatter
    assert np.array_equal(s, b) and np.array_equal(f, b)
    seg.upload(a.view(np.float32))
    s, f = run(2)                                    # swap
    assert np.array_equal(s, b) and np.array_equal(f, a)
    s, f = run(2)
    assert np.array_equal(s, a) and np.array_equal(f, b)


# ------------------------------------------------------------------------------------------------ 3. argument checks on device tables
def test_bad_device_tables_are_refused_before_any_launch():
    lib, err = _lib(), _lib().mvf_last_error
    seg = _Segments([4, 8, 16])
    x = _values(seg.n, 3)
    seg.upload(x)
    acc = torch.zeros(seg.n, dtype=torch.float64, device="cuda")
    flat = torch.full((seg.n,), 7.0, device="cuda")
    base = seg.dev.data_ptr()
    p = [base + 4 * s for s in seg.starts]

    def table(rows):
        return torch.from_numpy(np.array(rows, dtype=SEG_DTYPE).view(np.uint8).copy()).cuda()
    bad = [(table([(p[0], 1), (p[1], 4), (p[2], 12)]), b"not at 0"), (table([(p[0], 0), (p[1], 12), (p[2], 4)]), b"ascend"),
           (table([(p[0], 0), (p[1], 4), (p[2], 4)]), b"ascend"), (table([(p[0], 0), (p[1], 4), (p[2], 28)]), b"ascend"),
           (table([(p[0], 0), (0, 4), (p[2], 12)]), b"NULL or misaligned"), (table([(p[0], 0), (p[1] + 2, 4), (p[2], 12)]), b"NULL or misaligned")]
    for t, msg in bad:
        assert lib.mvf_bn_stats_accumulate(t.data_ptr(), 3, seg.n, acc.data_ptr(), None) == -1 and msg in err(), msg
        assert lib.mvf_bn_stats_finalize(t.data_ptr(), 3, seg.n, acc.data_ptr(), 2, None, None) == -1 and msg in err(), msg
        assert lib.mvf_bn_stats_finalize(t.data_ptr(), 3, seg.n, acc.data_ptr(), 2, flat.data_ptr(), None) == -1 and msg in err(), msg
        for mode in (0, 1, 2):
            assert lib.mvf_bn_stats_exchange(t.data_ptr(), 3, seg.n, flat.data_ptr(), mode, None) == -1 and msg in err(), msg
    good = seg.table.data_ptr()
    assert lib.mvf_bn_stats_accumulate(None, 3, seg.n, acc.data_ptr(), None) == -1
    assert lib.mvf_bn_stats_accumulate(good, 0, seg.n, acc.data_ptr(), None) == -1
    assert lib.mvf_bn_stats_accumulate(good, 3, 0, acc.data_ptr(), None) == -1
    assert lib.mvf_bn_stats_accumulate(good, 3, seg.n, None, None) == -1
    assert lib.mvf_bn_stats_finalize(good, 3, seg.n, acc.data_ptr(), 0, None, None) == -1 and b"count" in err()
    assert lib.mvf_bn_stats_exchange(good, 3, seg.n, None, 0, None) == -1
    assert lib.mvf_bn_stats_exchange(good, 3, seg.n, flat.data_ptr(), 3, None) == -1 and b"mode" in err()
    assert lib.mvf_bn_stats_exchange(good, 3, seg.n, p[1], 2, None) == -1 and b"overlaps" in err()
    torch.cuda.synchronize()
    got, clean = seg.download()
    assert clean and np.array_equal(got, _bits(x)) and bool((acc == 0).all()) and bool((flat == 7.0).all())


# ------------------------------------------------------------------------------------------------ engines
def _model(momentum=None, **backbone):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0)
    cfg["backbone"].update(backbone)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    if momentum is not None:
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.momentum = momentum
    return m.cuda().train()


_BATCHES = {}


def _batch(seed):
    if seed not in _BATCHES:
        _BATCHES[seed] = (torch.from_numpy(synth.synth_clip_batch(2, 4, 64, 64, seed=seed)).cuda(), torch.from_numpy(synth.synth_labels(2, seed=seed)).cuda())
    return _BATCHES[seed]


CALIB = (200, 201, 202)


def _stats(m, training_only=True):
    """{state_dict key: clone} of the running statistics of the BatchNorm modules (in training mode)."""
    out = {}
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and (mod.training or not training_only):
            out[name + ".running_mean"] = mod.running_mean.detach().clone()
            out[name + ".running_var"] = mod.running_var.detach().clone()
    return out


def _twin_snapshots(m, eng, seeds):
    """The existing forward on a model whose BatchNorm modules carry momentum 1.0: the running statistics after each batch ARE that batch's statistics."""
    snaps = []
    for s in seeds:
        eng.forward(*_batch(s))
        torch.cuda.synchronize()
        snaps.append({k: v.cpu().numpy() for k, v in _stats(m).items()})
    return snaps


def _mean_of(snaps):
    out = {}
    for k in snaps[0]:
        acc = np.zeros(snaps[0][k].shape, np.float64)
        for s in snaps:
            acc = acc + s[k].astype(np.float64)
        out[k] = (acc / np.float64(len(snaps))).astype(np.float32)
    return out


def _equal_bits(stats, want):
    return sorted(stats) == sorted(want) and all(np.array_equal(_bits(stats[k].cpu().numpy()), _bits(want[k])) for k in want)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _names_during(eng, call):
    with library_names(eng) as names:
        try:
            out = call()
        except Exception as e:          # noqa: BLE001 -- handed back to the caller beside the names
            out = e
    return names, out


def _new(names):
    return [n for n in names if n in NEW_ENTRY_POINTS]


def _launching(names):
    """Without the three new entry points and the size / plan queries (some are answered once per engine or per descriptor and cached)."""
    return sorted(n for n in names if n not in NEW_ENTRY_POINTS and not n.endswith(("_bytes", "_rows", "_splits", "_wgs")))


_RUNS = {}


def _live_run(dtype):
    """Model A (momentum 1.0 modules, the existing forward, three batches) against model B (default momentum, precise_bn over the same batches), then one
    train_step on B and on a model C whose statistics were set to the expected values by hand."""
    if dtype in _RUNS:
        return _RUNS[dtype]
    r = {}
    ma = _model(momentum=1.0)
    ea = ma.train_engine(dtype=dtype)
    snaps = _twin_snapshots(ma, ea, CALIB)
    r["forward_names"], _ = _names_during(ea, lambda: ea.forward(*_batch(CALIB[0])))
    del ma, ea
    mb = _model()
    eb = mb.train_engine(dtype=dtype)
    init = {k: v.clone() for k, v in mb.state_dict().items()}
    p0, mom0, nbt0 = eb.flat_params.clone(), eb.flat_mom.clone(), eb._nbt_flat.clone()
    pulled = []

    def feed(seeds):
        for s in seeds:
            pulled.append(s)
            yield _batch(s)
    rng0 = torch.cuda.get_rng_state()
    r["names"], r["used"] = _names_during(eb, lambda: eb.precise_bn(feed(CALIB), num_iters=3))
    torch.cuda.synchronize()
    r["rng_untouched"] = torch.equal(rng0, torch.cuda.get_rng_state())
    want = _mean_of(snaps)
    r["calibrated"] = _equal_bits(_stats(mb), want)
    r["moved"] = not any(torch.equal(v, init[k]) for k, v in _stats(mb).items())
    r["untouched"] = (_same_bits(eb.flat_params, p0) and _same_bits(eb.flat_mom, mom0) and _same_bits(eb._nbt_flat, nbt0)
                      and all(_same_bits(v, init[k]) for k, v in mb.state_dict().items() if k.endswith("num_batches_tracked")))
    r["momentum_restored"] = all(b.momentum == 0.1 for b in eb._all_bns()) and all(
        mod.momentum == 0.1 for mod in mb.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm))
    r["no_plans"] = not getattr(eb, "_plans", None) and eb.saved is None
    # the step after it: equal to the same step from statistics set by hand
    mc = _model()
    ec = mc.train_engine(dtype=dtype)
    with torch.no_grad():
        for name, mod in mc.named_modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.running_mean.copy_(torch.from_numpy(want[name + ".running_mean"]))
                mod.running_var.copy_(torch.from_numpy(want[name + ".running_var"]))
    imgs, labels = _batch(210)
    lb, lc = eb.train_step(imgs.clone(), labels.clone(), lr=0.01), ec.train_step(imgs.clone(), labels.clone(), lr=0.01)
    torch.cuda.synchronize()
    r["step_equal"] = (_same_bits(lb, lc) and _same_bits(eb.flat_params, ec.flat_params) and _same_bits(eb.flat_mom, ec.flat_mom)
                       and all(_same_bits(a, b) for a, b in zip(mb.buffers(), mc.buffers())))
    r["step_moved"] = not torch.equal(eb.flat_params, p0)
    del mc, ec
    # num_iters = 2 of a three-batch iterable, from the initial statistics again
    mb.load_state_dict(init, strict=True)
    del pulled[:]
    r["used2"] = eb.precise_bn(feed(CALIB), num_iters=2)
    torch.cuda.synchronize()
    r["pulled2"] = list(pulled)
    r["calibrated2"] = _equal_bits(_stats(mb), _mean_of(snaps[:2]))
    # an iterable that ends early: what came is used
    mb.load_state_dict(init, strict=True)
    r["used_short"] = eb.precise_bn(feed(CALIB[:1]), num_iters=200)
    torch.cuda.synchronize()
    r["calibrated_short"] = _equal_bits(_stats(mb), _mean_of(snaps[:1]))
    _RUNS[dtype] = r
    return r


DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


# ------------------------------------------------------------------------------------------------ 4. the twin run
@DTYPES
def test_precise_bn_equals_the_fp64_mean_of_a_momentum_one_twin(dtype):
    r = _live_run(dtype)
    assert r["used"] == 3
    assert r["calibrated"] and r["moved"]
    assert r["untouched"] and r["momentum_restored"] and r["no_plans"] and r["rng_untouched"]
    assert r["step_equal"] and r["step_moved"]


@DTYPES
def test_num_iters_bounds_what_is_consumed_and_a_short_iterable_is_used_as_it_came(dtype):
    r = _live_run(dtype)
    assert r["used2"] == 2 and r["pulled2"] == list(CALIB[:2]) and r["calibrated2"]
    assert r["used_short"] == 1 and r["calibrated_short"]


@DTYPES
def test_calibration_adds_one_launch_per_batch_and_one_finalize(dtype):
    r = _live_run(dtype)
    assert _new(r["names"]) == ["mvf_bn_stats_exchange"] + ["mvf_bn_stats_accumulate"] * 3 + ["mvf_bn_stats_finalize"]      # (the gather of the pre-call copy)
    # and nothing else beyond three forwards
    assert not _new(r["forward_names"])
    assert len(_launching(r["forward_names"])) > 100 and _launching(r["names"]) == _launching(r["forward_names"] * 3)


# ------------------------------------------------------------------------------------------------ 5. refusals, and a batch that raises
def test_refusals_leave_everything_as_it_was():
    m = _model()
    eng = m.train_engine()
    good = [_batch(s) for s in CALIB]
    before = {k: v.clone() for k, v in m.state_dict().items()}

    def unchanged():
        torch.cuda.synchronize()
        return all(_same_bits(v, before[k]) for k, v in m.state_dict().items()) and all(b.momentum == 0.1 for b in eng._all_bns())
    names, out = _names_during(eng, lambda: eng.precise_bn(iter(()), num_iters=3))
    assert isinstance(out, ValueError) and "no batch" in str(out) and unchanged()
    assert _new(names) == ["mvf_bn_stats_exchange"] * 2          # the pre-call copy, and its way back
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="num_iters"):
            eng.precise_bn(good, num_iters=bad)
    with pytest.raises(ValueError, match="weights"):
        eng.precise_bn(good, weights="both")
    with pytest.raises(RuntimeError, match="enable_ema"):
        eng.precise_bn(good, weights="ema")
    # a batch that raises midway (a host tensor: the forward refuses it) after one good batch has overwritten the statistics
    names, out = _names_during(eng, lambda: eng.precise_bn([good[0], (good[1][0].cpu(), good[1][1]), good[2]], num_iters=3))
    assert isinstance(out, RuntimeError) and "GPU input" in str(out)
    assert _new(names) == ["mvf_bn_stats_exchange", "mvf_bn_stats_accumulate", "mvf_bn_stats_exchange"]
    assert unchanged()
    # non-finite statistics on entry
    with torch.no_grad():
        m.backbone.layer2[1].bn2.running_var[5] = float("inf")
    names, out = _names_during(eng, lambda: eng.precise_bn(good, num_iters=3))
    assert isinstance(out, RuntimeError) and "non-finite" in str(out) and "layer2.1.bn2.running_var" in str(out)
    assert _new(names) == ["mvf_bn_stats_exchange"] and not any("conv" in n for n in names)
    with torch.no_grad():
        m.backbone.layer2[1].bn2.running_var[5] = before["backbone.layer2.1.bn2.running_var"][5]
    assert unchanged()
    # micro-steps pending in the accumulator
    eng.accumulate_step(*good[0])
    pending = {k: v.clone() for k, v in m.state_dict().items()}
    names, out = _names_during(eng, lambda: eng.precise_bn(good, num_iters=3))
    assert isinstance(out, RuntimeError) and "pending" in str(out) and not names
    assert all(_same_bits(v, pending[k]) for k, v in m.state_dict().items())
    eng.apply_accumulated(lr=0.01)
    assert eng.precise_bn(good, num_iters=1) == 1


# ------------------------------------------------------------------------------------------------ 6. frozen BatchNorms
def test_frozen_stage_statistics_stay_and_the_others_are_calibrated():
    ma = _model(momentum=1.0, frozen_stages=1)
    snaps = _twin_snapshots(ma, ma.train_engine(), CALIB[:2])
    del ma
    m = _model(frozen_stages=1)
    eng = m.train_engine()
    before = _stats(m, training_only=False)
    frozen = sorted(set(before) - set(_stats(m)))
    assert any(k.startswith("backbone.bn1.") for k in frozen) and any(k.startswith("backbone.layer1.") for k in frozen)
    assert not any(k.startswith("backbone.layer2.") for k in frozen) and 0 < len(frozen) < len(before)
    nbt = eng._nbt_flat.clone()
    assert eng.precise_bn([_batch(s) for s in CALIB[:2]]) == 2
    torch.cuda.synchronize()
    after = _stats(m, training_only=False)
    assert all(_same_bits(after[k], before[k]) for k in frozen)
    assert _equal_bits({k: v for k, v in after.items() if k not in frozen}, _mean_of(snaps))
    assert _same_bits(eng._nbt_flat, nbt)
    tab = eng._stat_table([b for b in eng._all_bns() if not b.frozen])
    assert sorted(tab.keys) == sorted(set(before) - set(frozen)) and tab is eng._stat_table([b for b in eng._all_bns() if not b.frozen])      # built once


def test_norm_eval_backbone_has_nothing_to_calibrate():
    m = _model(norm_eval=True, norm_frozen=True)
    eng = m.train_engine()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert not _stats(m)                             # every BatchNorm is in eval mode
    names, used = _names_during(eng, lambda: eng.precise_bn([_batch(CALIB[0])], num_iters=5))
    torch.cuda.synchronize()
    assert used == 0 and not names
    assert all(_same_bits(v, before[k]) for k, v in m.state_dict().items())


# ------------------------------------------------------------------------------------------------ 7. the averaged weights' own statistics
_EMA_RUNS = {}


def _ema_run(dtype):
    if dtype in _EMA_RUNS:
        return _EMA_RUNS[dtype]
    r = {}
    m = _model()
    eng = m.train_engine(dtype=dtype)
    eng.enable_ema(momentum=0.25, warmup_steps=1)
    for i in range(2):
        eng.train_step(*[t.clone() for t in _batch(220 + i)], lr=0.01)
    torch.cuda.synchronize()
    live = {k: v.clone() for k, v in m.state_dict().items()}
    p0, e0, mom0 = eng.flat_params.clone(), eng.flat_ema.clone(), eng.flat_mom.clone()
    r["ema_differs"] = not torch.equal(p0, e0)
    # before any calibration: the block pairs the averaged parameters with the LIVE statistics and calls none of the new entry points
    def block():
        with eng.averaged_weights():
            return {k: v.clone() for k, v in _stats(m).items()}
    names, inside = _names_during(eng, block)
    r["uncalibrated_block"] = (not _new(names) and names.count("mvf_ema_swap") == 2 and eng.flat_ema_stats is None
                               and all(_same_bits(v, live[k]) for k, v in inside.items()) and "bn_stats" not in eng.ema_state_dict())
    # the twin: the averaged parameters and the live statistics in a model whose BatchNorm modules carry momentum 1.0
    mt = _model(momentum=1.0)
    et = mt.train_engine(dtype=dtype)
    mt.load_state_dict(live, strict=True)
    et.flat_params.copy_(e0)
    want = _mean_of(_twin_snapshots(mt, et, CALIB))
    del mt, et
    r["names"], r["used"] = _names_during(eng, lambda: eng.precise_bn([_batch(s) for s in CALIB], num_iters=3, weights="ema"))
    torch.cuda.synchronize()

    def live_again():
        return (_same_bits(eng.flat_params, p0) and _same_bits(eng.flat_ema, e0) and _same_bits(eng.flat_mom, mom0)
                and all(_same_bits(v, live[k]) for k, v in m.state_dict().items()))
    r["live_untouched"] = live_again()
    stats0 = eng.flat_ema_stats.clone()
    names, inside = _names_during(eng, block)
    torch.cuda.synchronize()
    r["block_names"] = _new(names)
    r["inside_is_twin"] = _equal_bits(inside, want)
    r["inside_differs_from_live"] = not any(torch.equal(v, live[k]) for k, v in inside.items())
    r["restored"] = live_again() and _same_bits(eng.flat_ema_stats, stats0)
    entry = eng.ema_state_dict()
    r["entry_is_twin"] = _equal_bits(entry["bn_stats"], want) and all(v.device.type == "cpu" and v.dtype == torch.float32 for v in entry["bn_stats"].values())
    r.update(model=m, engine=eng, want=want, live=live, entry=entry)
    _EMA_RUNS[dtype] = r
    return r


@DTYPES
def test_ema_calibration_leaves_the_live_model_alone_and_the_block_sees_the_twins_statistics(dtype):
    r = _ema_run(dtype)
    assert r["ema_differs"] and r["uncalibrated_block"]
    assert r["used"] == 3 and r["live_untouched"]
    assert _new(r["names"]) == ["mvf_bn_stats_exchange"] + ["mvf_bn_stats_accumulate"] * 3 + ["mvf_bn_stats_finalize", "mvf_bn_stats_exchange"]
    assert r["names"].count("mvf_ema_swap") == 2
    assert r["block_names"] == ["mvf_bn_stats_exchange"] * 2          # entry and exit
    assert r["inside_is_twin"] and r["inside_differs_from_live"] and r["restored"]
    assert r["entry_is_twin"]


def test_checkpoints_carry_the_calibrated_statistics_and_resume_restores_them(tmp_path):
    from mvfnet_amd import checkpoint
    from mvfnet_amd.runner import Runner
    r = _ema_run(torch.float32)
    m, eng, want = r["model"], r["engine"], r["want"]
    path = checkpoint.save_checkpoint(m, os.path.join(str(tmp_path), "epoch_1.pth"), optimizer=eng.optimizer_state_dict(), meta=dict(epoch=1, iter=2),
                                      ema=eng.ema_state_dict())
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert all(_same_bits(v, r["live"][k].cpu()) for k, v in ckpt["state_dict"].items())          # state_dict stays the live model
    avg = checkpoint.averaged_state_dict(ckpt)
    with eng.averaged_weights():
        inside = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert list(avg) == list(inside) and all(_same_bits(avg[k], inside[k]) for k in avg)
    # resume into a fresh model
    m2 = _model()
    run2 = Runner(m2, work_dir=str(tmp_path), lr=0.01, ema=dict(momentum=0.25, warmup_steps=1), logger=None)
    assert run2.engine.flat_ema_stats is None
    run2.resume(path)
    eng2 = run2.engine
    assert _same_bits(eng2.flat_ema, eng.flat_ema) and _equal_bits(eng2.ema_state_dict()["bn_stats"], want)
    with eng2.averaged_weights():
        assert _equal_bits(_stats(m2), want)
    torch.cuda.synchronize()
    assert all(_same_bits(v, r["live"][k]) for k, v in m2.state_dict().items())
    # an entry without the statistics (an older checkpoint) loads as before and drops the ones the engine held
    del ckpt["ema"]["bn_stats"]
    old = os.path.join(str(tmp_path), "old.pth")
    torch.save(ckpt, old)
    run2.resume(old)
    assert eng2.flat_ema_stats is None and "bn_stats" not in eng2.ema_state_dict() and _same_bits(eng2.flat_ema, eng.flat_ema)
    # what does not fit is refused
    entry = eng.ema_state_dict()
    entry["bn_stats"]["backbone.nowhere.running_mean"] = torch.zeros(4)
    with pytest.raises(ValueError, match="backbone.nowhere.running_mean"):
        eng2.load_ema_state_dict(entry)
    entry = eng.ema_state_dict()
    del entry["bn_stats"]["backbone.bn1.running_var"]
    with pytest.raises(ValueError, match="backbone.bn1.running_var"):
        eng2.load_ema_state_dict(entry)
    # reset_ema / disable_ema drop them
    eng2.load_ema_state_dict(eng.ema_state_dict())
    assert eng2.flat_ema_stats is not None
    eng2.reset_ema()
    assert eng2.flat_ema_stats is None
    eng2.load_ema_state_dict(eng.ema_state_dict())
    eng2.disable_ema()
    assert eng2.flat_ema_stats is None and eng2.flat_ema is None


def test_an_engine_that_never_calibrates_calls_none_of_the_entry_points():
    m = _model()
    eng = m.train_engine()
    eng.enable_ema(momentum=0.25)

    def work():
        eng.train_step(*[t.clone() for t in _batch(230)], lr=0.01)
        eng.accumulate_step(*_batch(231))
        eng.apply_accumulated(lr=0.01)
        with eng.averaged_weights():
            m.state_dict()
        eng.ema_state_dict()
    names, out = _names_during(eng, work)
    torch.cuda.synchronize()
    assert out is None and not _new(names) and eng.flat_ema_stats is None and not getattr(eng, "_stat_tables", None)
