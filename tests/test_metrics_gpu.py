"""GPU: device-side accuracy -- mvf_metrics_update (csrc/metrics.hip), metrics.DeviceMetrics, runner.device_test / the evaluation hooks' on_device path, and
the train engine's accuracy window (TrainEngine.enable_train_accuracy, Runner(train_accuracy=...)).

Everything is compared as integers against the numpy restatement of the rules (tests/metrics_numpy.py): the kernel only compares scores and adds integers,
so there is no tolerance to state."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_numpy as mn
from helpers import NamesOf, library_names
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

SENT = -0x5A5A5A5A5A5A5A5B          # guard-band value of the int64 state
SENT32 = -0x5A5A5A5B                # ... and of the int32 record arrays
BAND = 4


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib


class _Call(object):
    """Device operands of mvf_metrics_update with a 4-word guard band in front of and behind the state and behind each record array."""

    def __init__(self, classes, with_confusion, max_rows):
        self.classes, self.conf = classes, with_confusion
        self.words = mn.state_words(classes, with_confusion)
        assert _lib().mvf_metrics_state_words(classes, int(with_confusion)) == self.words
        self.full = torch.full((self.words + 2 * BAND,), SENT, dtype=torch.int64, device="cuda")
        self.state = self.full[BAND:BAND + self.words]
        self.state.zero_()
        self.rank_full = torch.full((max_rows + BAND,), SENT32, dtype=torch.int32, device="cuda")
        self.pred_full = torch.full((max_rows + BAND,), SENT32, dtype=torch.int32, device="cuda")
        self.max_rows = max_rows

    def update(self, scores, labels, ks, record=True, offset=0):
        rows = scores.shape[0]
        assert scores.is_contiguous() and labels.is_contiguous() and offset + rows <= self.max_rows
        k = (C.c_int * len(ks))(*ks)
        rc = _lib().mvf_metrics_update(scores.data_ptr(), rows, self.classes, labels.data_ptr(), k, len(ks), self.state.data_ptr(), int(self.conf),
                                       self.rank_full.data_ptr() + 4 * offset if record else None, self.pred_full.data_ptr() + 4 * offset if record else None,
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib().mvf_last_error()

    def host(self):
        torch.cuda.synchronize()
        return self.state.cpu().numpy()

    def bands_intact(self, recorded):
        full = self.full.cpu().numpy()
        r, p = self.rank_full.cpu().numpy(), self.pred_full.cpu().numpy()
        return (bool((full[:BAND] == SENT).all()) and bool((full[BAND + self.words:] == SENT).all())
                and bool((r[recorded:] == SENT32).all()) and bool((p[recorded:] == SENT32).all()))


def _scores(rows, classes, seed, decimals=1):
    """fp32 normals rounded to one decimal: ties are common, at the top and at the label."""
    return np.round(np.random.RandomState(seed).standard_normal((rows, classes)), decimals).astype(np.float32)


def _labels(rows, classes, seed):
    y = np.random.RandomState(seed + 1).randint(0, classes, size=rows).astype(np.int64)
    y[0] = 0
    y[-1] = classes - 1
    return y


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("classes", [1, 2, 63, 64, 65, 400, 1000])
@pytest.mark.parametrize("rows", [1, 3, 32, 257])
def test_kernel_state_equals_the_restatement_word_for_word(classes, rows):
    s, y = _scores(rows, classes, 1000 * classes + rows), _labels(rows, classes, classes + rows)
    pre = mn.rows_ref(s, y)
    assert (pre[2] == 0).all()
    sd, yd = _cuda(s), _cuda(y)
    eight = (1, 2, 3, 5, 7, 10, classes, classes + 5)
    for ks in ((1,), (1, 5), eight):
        for conf in (False, True):
            want, rank, pred = mn.metrics_ref(s, y, ks, conf, rows=pre)
            for record in (False, True):
                op = _Call(classes, conf, rows)
                op.update(sd, yd, ks, record=record)
                got = op.host()
                assert np.array_equal(got, want), (ks, conf, record, got[:16], want[:16])
                assert op.bands_intact(rows if record else 0), (ks, conf, record)
                if record:
                    assert np.array_equal(op.rank_full[:rows].cpu().numpy(), rank) and np.array_equal(op.pred_full[:rows].cpu().numpy(), pred), (ks, conf)
    assert want[mn.HITS + 6] == rows and want[mn.HITS + 7] == rows                 # k >= classes always hits
    assert int(np.trace(want[mn.HEADER:].reshape(classes, classes))) == want[mn.HITS]


# ------------------------------------------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("classes", [5, 70, 400])
def test_ties_go_to_the_lower_class_index(classes):
    rng = np.random.RandomState(7 + classes)
    rows = 96
    s = rng.randint(0, 4, size=(rows, classes)).astype(np.float32) * np.float32(0.5)          # four distinct values
    s[0:8] = np.float32(1.25)                                                                  # all-equal rows
    s[8] = -np.inf
    s[9] = np.inf
    for r in range(10, 20):                                                                    # rows with -inf / +inf entries among ordinary ones
        s[r, rng.randint(0, classes, size=max(1, classes // 3))] = -np.inf if r % 2 else np.inf
    y = rng.randint(0, classes, size=rows).astype(np.int64)
    y[0], y[1], y[8], y[9] = 0, classes - 1, classes - 1, classes // 2
    ks = (1, 2, 5, classes)
    want, rank, pred = mn.metrics_ref(s, y, ks, True)
    assert rank[0] == 0 and rank[1] == classes - 1 and rank[8] == classes - 1 and pred[1] == 0 and pred[8] == 0 and pred[9] == 0
    op = _Call(classes, True, rows)
    op.update(_cuda(s), _cuda(y), ks)
    got = op.host()
    assert np.array_equal(got, want)
    assert np.array_equal(op.rank_full[:rows].cpu().numpy(), rank) and np.array_equal(op.pred_full[:rows].cpu().numpy(), pred)
    assert got[mn.HITS] == int(np.trace(got[mn.HEADER:].reshape(classes, classes)))          # hits(k = 1) == trace(confusion), on the device result
    assert 0 < got[mn.HITS] < rows and got[mn.HITS + 3] == rows and got[:3].tolist() == [rows, 0, 0]
    assert op.bands_intact(rows)


# ------------------------------------------------------------------------------------------------ 3. bad rows
@pytest.mark.parametrize("classes", [3, 65, 400])
def test_bad_labels_and_nan_rows_move_only_their_counters(classes):
    s = _scores(8, classes, 31 + classes)
    y = np.array([-1, classes, 1 << 40, 1, classes - 1, 0, -(1 << 40), classes - 1], dtype=np.int64)
    s[3, 1] = np.nan                      # at the label
    s[4, 0] = np.nan                      # elsewhere
    s[5, classes - 1] = np.nan            # the row's last score (the ragged tail of the last pass)
    s[6, :] = np.nan                      # a bad label on a NaN row: the label wins
    s[7, classes - 1] = -np.nan           # a negative NaN at the label
    for conf in (False, True):
        op = _Call(classes, conf, 8)
        op.update(_cuda(s), _cuda(y), (1, 5))
        got = op.host()
        assert got[:3].tolist() == [8, 4, 4] and not got[3:].any(), got[:16]          # only words 0..2 move
        assert (op.rank_full[:8].cpu().numpy() == -1).all() and (op.pred_full[:8].cpu().numpy() == -1).all()
        assert op.bands_intact(8)
        assert np.array_equal(got, mn.metrics_ref(s, y, (1, 5), conf)[0])
    # mixed with valid rows, on top of an existing state
    s2, y2 = np.concatenate([s, _scores(20, classes, 5)]), np.concatenate([y, _labels(20, classes, 6)])
    op = _Call(classes, True, 28)
    op.update(_cuda(s2), _cuda(y2), (1, 5))
    op.update(_cuda(s2), _cuda(y2), (1, 5), record=False)
    once, rank, pred = mn.metrics_ref(s2, y2, (1, 5), True)
    assert np.array_equal(op.host(), 2 * once) and once[:3].tolist() == [28, 4, 4]
    assert np.array_equal(op.rank_full[:28].cpu().numpy(), rank) and np.array_equal(op.pred_full[:28].cpu().numpy(), pred) and op.bands_intact(28)


# ------------------------------------------------------------------------------------------------ 4. accumulation, DeviceMetrics
def test_chunking_does_not_change_the_state_and_reset_gives_zeros():
    from mvfnet_amd.metrics import DeviceMetrics
    classes, rows = 65, 257
    s, y = _scores(rows, classes, 77), _labels(rows, classes, 78)
    s[100, 3] = np.nan
    y[200] = classes
    sd, yd = _cuda(s), _cuda(y)
    want, rank, pred = mn.metrics_ref(s, y, (1, 5, 64), True)
    states = []
    for chunks in ([rows], [1] * rows, [1, 3, 64, 100, 89]):
        m = DeviceMetrics(classes, k=(1, 5, 64), record=rows)
        i = 0
        for c in chunks:
            m.update(sd[i:i + c], yd[i:i + c] if c % 2 else yd[i:i + c].reshape(c, 1))          # (rows,) and (rows, 1) labels
            i += c
        assert i == rows and m.recorded == rows
        states.append(m.state.cpu().numpy())
        r, p = m.records()
        assert np.array_equal(r.cpu().numpy(), rank) and np.array_equal(p.cpu().numpy(), pred)
        with pytest.raises(RuntimeError, match="do not fit record=257"):
            m.update(sd[:1], yd[:1])
    assert all(np.array_equal(st, want) for st in states)
    with pytest.raises(ValueError, match=r"1 of 257 rows have a label outside \[0, 65\) and 1 hold a NaN"):
        m.compute()
    fig = m.compute(strict=False)
    assert fig["count"] == rows and fig["invalid"] == 1 and fig["nan_rows"] == 1
    assert fig["top1"] == want[mn.HITS] / rows and fig["top5"] == want[mn.HITS + 1] / rows and fig["top64"] == want[mn.HITS + 2] / rows
    assert np.array_equal(fig["confusion"], want[mn.HEADER:].reshape(classes, classes))
    ok = mn.rows_ref(s, y)[2] == 0
    from mvfnet_amd.evaluation import mean_class_accuracy
    assert fig["mean_class_acc"] == pytest.approx(float(mean_class_accuracy(np.eye(classes)[pred[ok]], y[ok])), abs=1e-15)
    m.reset()
    assert not m.state.cpu().numpy().any() and m.recorded == 0 and m.compute()["count"] == 0
    m.update(sd[:3], yd[:3])                                   # the record starts again at offset 0
    assert np.array_equal(m.records()[0].cpu().numpy(), rank[:3])
    with pytest.raises(ValueError, match="scores must be"):
        m.update(sd[:, :64], yd)
    with pytest.raises(ValueError, match="labels must be"):
        m.update(sd, yd.to(torch.int32))
    with pytest.raises(ValueError, match="labels must be"):
        m.update(sd, yd[:5])


# ------------------------------------------------------------------------------------------------ 5. evaluation without readbacks
def _model(test_cfg=None, dropout=0.0):
    import mvfnet_amd
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=dropout), None, test_cfg if test_cfg is not None else dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda()


class _SyncSpy(object):
    """Counts the calls that read back or wait for the device while it is active."""
    TARGETS = ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"), (torch.cuda, "synchronize"),
               (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize"))

    def __enter__(self):
        self.calls, self._saved = [], []
        for owner, name in self.TARGETS:
            real = getattr(owner, name)
            self._saved.append((owner, name, real))

            def spy(*a, _real=real, _name=name, **kw):
                self.calls.append(_name)
                return _real(*a, **kw)
            setattr(owner, name, spy)
        return self

    def __exit__(self, *a):
        for owner, name, real in self._saved:
            setattr(owner, name, real)


_EVAL = {}


def _eval_fixture():
    """One model, 12 synthetic videos of two 4-frame clips at 64 x 64; computed once, read by the tests below."""
    if not _EVAL:
        _EVAL["model"] = _model(dict(average_clips="prob")).eval()
        _EVAL["videos"] = [dict(img_group=torch.from_numpy(synth.synth_clip_batch(1, 8, 64, 64, seed=300 + i)).cuda()) for i in range(12)]
    return _EVAL["model"], _EVAL["videos"]


@pytest.mark.parametrize("average_clips", ["prob", "score"])
def test_device_test_counts_what_the_host_path_computes(average_clips):
    from mvfnet_amd.evaluation import mean_class_accuracy, top_k_accuracy
    from mvfnet_amd.metrics import DeviceMetrics
    from mvfnet_amd.runner import device_test, single_gpu_test
    model, videos = _eval_fixture()
    model.test_cfg = dict(average_clips=average_clips)
    rows = np.stack([np.asarray(r).reshape(-1) for r in single_gpu_test(model, videos)])
    assert rows.shape == (12, 400) and np.isfinite(rows).all()
    order = np.sort(rows, axis=1)[:, ::-1]
    assert (order[:, 0] > order[:, 1]).all() and (order[:, 4] > order[:, 5]).all()          # no tie at the top-1 / top-5 boundary of any host row
    # labels: video i's label is the class ranked i % 7 in its host row -- hits and misses at both k
    labels = [int(np.argsort(-rows[i], kind="stable")[i % 7]) for i in range(12)]
    want = top_k_accuracy(list(rows), labels, k=(1, 5))
    assert [round(float(a) * 12) for a in want] == [2, 10]
    metrics = DeviceMetrics(400, k=(1, 5), record=12)
    lab_dev = torch.tensor(labels, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")          # a synchronising torch call inside the pass raises
        strict_mode = True
    except Exception:
        strict_mode = False
    try:
        with _SyncSpy() as spy:
            out = device_test(model, videos, lab_dev, metrics)
    finally:
        if strict_mode:
            torch.cuda.set_sync_debug_mode("default")
    assert out is metrics and spy.calls == [], spy.calls                                    # nothing in the pass reads back or waits
    with _SyncSpy() as spy:
        fig = metrics.compute()
    assert spy.calls.count("cpu") == 1                                                       # the one read
    assert fig["count"] == 12 and fig["invalid"] == 0 and fig["nan_rows"] == 0
    assert fig["top1"] * 12 == 2 and fig["top5"] * 12 == 10
    assert fig["top1"] == float(want[0]) and fig["top5"] == float(want[1])
    assert fig["mean_class_acc"] == pytest.approx(float(mean_class_accuracy(rows, np.asarray(labels, dtype=np.int64))), abs=1e-15)
    rank, pred = (t.cpu().numpy() for t in metrics.records())
    assert rank.tolist() == [i % 7 for i in range(12)] and np.array_equal(pred, np.argmax(rows, axis=1))
    # labels as a list are uploaded once by device_test itself; the same counts
    again = DeviceMetrics(400, k=(1, 5))
    device_test(model, videos, labels, again)
    assert np.array_equal(again.state.cpu().numpy(), metrics.state.cpu().numpy())
    with pytest.raises(ValueError, match="there are 11 labels"):
        device_test(model, videos, labels[:11], DeviceMetrics(400))


def test_hooks_on_device_return_the_host_hooks_figures():
    from mvfnet_amd.evaluation import DistEvalTopKAccuracyHook, EvalTopKAccuracyHook
    from mvfnet_amd.runner import single_gpu_test
    model, videos = _eval_fixture()
    model.test_cfg = dict(average_clips="prob")
    rows = np.stack([np.asarray(r).reshape(-1) for r in single_gpu_test(model, videos)])
    labels = [int(np.argsort(-rows[i], kind="stable")[i % 7]) for i in range(12)]

    class _Runner(object):
        epoch = 1

    runner = _Runner()
    runner.model = model
    host = EvalTopKAccuracyHook(videos, labels, k=(1, 5), mean_class=True).after_train_epoch(runner)
    dev = EvalTopKAccuracyHook(videos, labels, k=(1, 5), on_device=True, mean_class=True).after_train_epoch(runner)
    assert set(host) == set(dev) == {"top1 acc", "top5 acc", "mean_class acc", "epoch"}
    assert host["top1 acc"] == dev["top1 acc"] == 2 / 12 and host["top5 acc"] == dev["top5 acc"] == 10 / 12
    assert dev["mean_class acc"] == pytest.approx(host["mean_class acc"], abs=1e-15)
    assert set(EvalTopKAccuracyHook(videos, labels, k=(1, 5), on_device=True).after_train_epoch(runner)) == {"top1 acc", "top5 acc", "epoch"}

    class _Dataset(object):
        video_infos = [dict(label=y) for y in labels]

        def __len__(self):
            return len(videos)

        def __getitem__(self, i):
            return dict(img_group=videos[i]["img_group"][0])

    out = DistEvalTopKAccuracyHook(_Dataset(), k=(1, 5), dist=False, on_device=True).after_train_epoch(runner)
    assert out["top1 acc"] == 2 / 12 and out["top5 acc"] == 10 / 12
    assert not model.training
    # several rows per video: refused before the first forward
    model.test_cfg = dict(average_clips=None)
    calls = []
    handle = model.register_forward_pre_hook(lambda *a: calls.append(1))
    try:
        with pytest.raises(ValueError, match="average_clips"):
            EvalTopKAccuracyHook(videos, labels, on_device=True).after_train_epoch(runner)
    finally:
        handle.remove()
        model.test_cfg = dict(average_clips="prob")
    assert calls == []


# ------------------------------------------------------------------------------------------------ 6. training accuracy
LR, KS = 0.01, (1, 5, 50, 200)
_TRAIN = {}


def _batch(seed, clips=2):
    return (torch.from_numpy(synth.synth_clip_batch(clips, 4, 64, 64, seed=seed)).cuda(), torch.from_numpy(synth.synth_labels(clips, seed=seed)).cuda())


def _step_scores(eng, b):
    """The engine's persistent (B, classes) score buffer: what the step's head wrote, eager or replayed."""
    return eng.buf("scores", (b, eng.num_classes), torch.float32)


def _train_run(use_plan):
    """8 train steps of the 2-clip bf16 engine with the window on; the score buffer and the labels are cloned after every step.  Once per policy."""
    if use_plan not in _TRAIN:
        m = _model().train()
        eng = m.train_engine(dtype=torch.bfloat16)
        if not use_plan:
            eng.use_plan = False
        eng.enable_train_accuracy(k=KS)
        kept = []
        for i in range(8):
            imgs, labels = _batch(400 + i % 3)
            eng.train_step(imgs.clone(), labels.clone(), lr=LR)
            kept.append((_step_scores(eng, 2).clone(), labels.clone()))
        replayed = any(st["plan"] is not None for st in getattr(eng, "_plans", {}).values())
        fig = eng.train_accuracy()
        _TRAIN[use_plan] = dict(model=m, eng=eng, fig=fig, after=eng.train_accuracy(), replayed=replayed,
                                scores=torch.cat([s for s, _ in kept]).cpu().numpy(), labels=torch.cat([l.reshape(-1) for _, l in kept]).cpu().numpy())
    return _TRAIN[use_plan]


@pytest.mark.parametrize("use_plan", [True, False], ids=["plan", "plan0"])
def test_train_accuracy_counts_every_step_eager_or_replayed(use_plan):
    run = _train_run(use_plan)
    assert run["replayed"] == use_plan                       # with plans on, the steps from the fifth on are replays
    assert run["scores"].shape == (16, 400) and np.isfinite(run["scores"]).all()
    want = mn.metrics_ref(run["scores"], run["labels"], KS, False)[0]
    fig = run["fig"]
    assert set(fig) == {"count", "top1", "top5", "top50", "top200", "invalid", "nan_rows"}
    assert fig["count"] == 16 and fig["invalid"] == 0 and fig["nan_rows"] == 0
    assert [round(fig["top%d" % k] * 16) for k in KS] == want[mn.HITS:mn.HITS + 4].tolist()
    assert all(fig["top%d" % k] == want[mn.HITS + i] / 16 for i, k in enumerate(KS))
    assert 0 < want[mn.HITS + 3] < 16 or want[mn.HITS + 2] > 0, want[:16]          # the figures are not all trivial
    after = run["after"]                                     # the read emptied the window
    assert after["count"] == 0 and np.isnan(after["top1"])


def test_plan_and_eager_runs_count_the_same():
    a, b = _train_run(True), _train_run(False)
    assert np.array_equal(a["scores"], b["scores"]) and a["fig"] == b["fig"]


def test_micro_steps_count_their_rows_and_blended_steps_count_none():
    from mvfnet_amd.blending import MixupBlending
    run = _train_run(False)
    eng = run["eng"]
    assert eng.train_accuracy()["count"] == 0
    kept = []
    for seed in (410, 411):
        imgs, labels = _batch(seed)
        eng.accumulate_step(imgs, labels)
        kept.append((_step_scores(eng, 2).clone(), labels.reshape(-1).clone()))
    eng.apply_accumulated(lr=LR)
    fig = eng.train_accuracy()
    want = mn.metrics_ref(torch.cat([s for s, _ in kept]).cpu().numpy(), torch.cat([l for _, l in kept]).cpu().numpy(), KS, False)[0]
    assert fig["count"] == 4 and [round(fig["top%d" % k] * 4) for k in KS] == want[mn.HITS:mn.HITS + 4].tolist()
    # label smoothing over integer labels is counted; a step under Mixup is not, and neither is a soft label matrix
    eng.label_smooth_eps = 0.1
    eng.train_step(*_batch(412), lr=LR)
    assert eng.train_accuracy()["count"] == 2
    eng.label_smooth_eps = 0.0
    eng.blending = MixupBlending(alpha=0.8, seed=5)
    eng.train_step(*_batch(413), lr=LR)
    eng.blending = None
    assert eng.train_accuracy()["count"] == 0
    imgs, _ = _batch(414)
    eng.train_step(imgs, torch.full((2, 400), 1.0 / 400, device="cuda"), lr=LR)
    fig = eng.train_accuracy()
    assert fig["count"] == 0 and np.isnan(fig["top1"])
    eng.disable_train_accuracy()
    with pytest.raises(RuntimeError, match="enable_train_accuracy"):
        eng.train_accuracy()
    torch.cuda.synchronize()


def _calls_of_one_step(eng, imgs, labels):
    """(library calls the engine made, entry points looked up on the package's library object) during one eager train_step."""
    import mvfnet_amd._lib as L
    from mvfnet_amd import launch_plan

    class _Names(launch_plan.Recorder):
        """RecordingLib's recorder, reduced to the names of the calls (the optimizer's calls are not plan material: their arguments need not be recordable)."""

        def call(self, name, fn, args):
            self.ops.append(name)
    rec, names = _Names(), []
    real_l = L.lib
    L.lib = NamesOf(real_l, names)
    try:
        with library_names(eng, lib=launch_plan.RecordingLib(rec, type(eng).lib)):
            eng.train_step(imgs, labels, lr=LR)
    finally:
        L.lib = real_l
    return list(rec.ops), names


def test_an_engine_that_never_enables_it_allocates_and_launches_nothing_more():
    m = _model().train()
    eng = m.train_engine(dtype=torch.bfloat16)
    eng.use_plan = False
    imgs, labels = _batch(420)
    for _ in range(2):
        eng.train_step(imgs, labels, lr=LR)
    off, names_off = _calls_of_one_step(eng, imgs, labels)
    assert "_train_acc" not in eng.__dict__ and eng._train_acc is None                     # no state attribute, nothing allocated
    assert "mvf_metrics_update" not in names_off and "mvf_metrics_update" not in off
    eng.enable_train_accuracy()
    assert eng._train_acc.state.numel() == 16                                              # no confusion matrix
    on, names_on = _calls_of_one_step(eng, imgs, labels)
    assert on == off and len(off) > 100                                                    # the engine's own sequence is what it was ...
    assert names_on.count("mvf_metrics_update") == 1                                       # ... plus the one launch behind it
    eng.disable_train_accuracy()
    again, names_again = _calls_of_one_step(eng, imgs, labels)
    assert again == off and "mvf_metrics_update" not in names_again
    torch.cuda.synchronize()


def test_runner_logs_the_training_accuracy():
    from mvfnet_amd.runner import Runner
    lines = []
    m = _model().train()
    run = Runner(m, lr=LR, log_interval=2, logger=lines.append, train_accuracy=dict(k=(1, 5)), nonfinite_guard={}, warmup=None)
    run.train_epoch([dict(img_group=i, label=l) for i, l in (_batch(430 + j) for j in range(4))])
    assert len(lines) == 2
    import re
    for line in lines:
        mt = re.search(r"grad_norm \S+ top1 (\d\.\d{4}) top5 (\d\.\d{4}) skipped 0$", line)
        assert mt, line
        assert float(mt.group(1)) * 4 in (0.0, 1.0, 2.0, 3.0, 4.0) and float(mt.group(1)) <= float(mt.group(2))          # four rows per window
