"""GPU: sample-wise AP, precision / recall / F1 counts and the best-F1 thresholds on the device -- mvf_multilabel_sample_ap / mvf_multilabel_prf /
mvf_multilabel_best_f1 (csrc/multilabel_f1.hip), DeviceMultiLabelMetrics.compute(sample_ap=, threshold=, thresholds=, best_f1=) and EvalMeanAPHook's new
figures.

Every integer output -- counts, positives, best_tp, best_n -- and the bits of best_threshold are compared exactly against the numpy restatement
(tests/multilabel_f1_numpy.py).  The fp64 sample APs are sums of at most 400 ratios in [0, 1], the kernel's in another order than numpy's: the suite's
AP_BOUND, 1e-12 (400 * 2^-53 = 4.4e-14 at the very worst)."""
import numpy as np
import pytest
import torch

import multilabel_f1_numpy as fn
import multilabel_numpy as mn
from mvfnet_amd import synth
from test_multilabel_gpu import AP_BOUND

pytestmark = pytest.mark.gpu

BASE_KEYS = {"mAP", "ap", "positives", "classes_with_positives", "rows", "nan_rows", "overflow"}
SAMPLE_KEYS = {"sample_mAP", "sample_ap", "rows_with_positives"}
PRF_KEYS = {"counts", "precision", "recall", "f1", "micro_precision", "micro_recall", "micro_f1", "macro_f1"}
BEST_KEYS = {"best_f1", "best_threshold", "macro_best_f1"}


def _case(rows, classes, kind, density, seed=0):
    gen = np.random.default_rng(seed * 7919 + rows * 31 + classes)
    if kind == "quant":
        s = (gen.integers(0, 8, (rows, classes)) / 8.0).astype(np.float32)      # 8 levels: heavy ties
    elif kind == "equal":
        s = np.full((rows, classes), 0.25, dtype=np.float32)
    else:
        s = gen.standard_normal((rows, classes)).astype(np.float32)
    if kind == "inf":
        s[gen.random((rows, classes)) < 0.1] = np.inf
        s[gen.random((rows, classes)) < 0.1] = -np.inf
    y = (gen.random((rows, classes)) < density).astype(np.uint8)
    if kind == "nan":
        bad = gen.permutation(rows)[:max(1, rows // 7)]
        s[bad, gen.integers(0, classes, bad.size)] = np.nan
    return s, y


def _metrics(classes, capacity):
    from mvfnet_amd.metrics import DeviceMultiLabelMetrics
    return DeviceMultiLabelMetrics(classes, capacity)


def _feed(m, s, y, block=None):
    block = block or len(s)
    for i in range(0, len(s), block):
        m.update(torch.from_numpy(s[i:i + block]).cuda(), torch.from_numpy(y[i:i + block]).cuda())
    return m


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _check(m, s, y, threshold=0.25, thresholds=None):
    """compute() with every option against the restatements.  -> the figures and the worst relative sample-AP error."""
    kw = dict(thresholds=thresholds) if thresholds is not None else dict(threshold=threshold)
    fig = m.compute(sample_ap=True, best_f1=True, **kw)
    assert set(fig) == BASE_KEYS | SAMPLE_KEYS | PRF_KEYS | BEST_KEYS
    n = len(s)
    # sample AP: the positives exactly, the fp64 sums within the bound
    ref = fn.sample_ap(s, y)
    assert fig["sample_ap"].shape == (n,) and fig["sample_ap"].dtype == np.float64
    have = ref["positives"] > 0
    assert np.array_equal(np.isnan(fig["sample_ap"]), ~have) and fig["rows_with_positives"] == ref["rows_with_positives"]
    err = float(np.max(np.abs(fig["sample_ap"][have] - ref["ap"][have]) / ref["ap"][have])) if have.any() else 0.0
    assert err <= AP_BOUND, err
    assert abs(fig["sample_mAP"] - ref["sample_mAP"]) <= AP_BOUND * ref["sample_mAP"] if have.any() else np.isnan(fig["sample_mAP"])
    # counts: exactly; the ratios are the conventions applied to them
    counts = fn.prf_counts(s, y, **kw)
    assert fig["counts"].dtype == np.int64 and np.array_equal(fig["counts"], counts)
    figs = fn.prf_figures(counts)
    assert all(np.array_equal(fig[k], figs[k]) for k in ("precision", "recall", "f1"))
    assert all(_same(fig[k], figs[k]) for k in ("micro_precision", "micro_recall", "micro_f1", "macro_f1"))
    # best F1: the integers, and the threshold's bits
    best = fn.best_f1(s, y)
    assert np.array_equal(fig["best_threshold"].view(np.uint32), best["best_threshold"].view(np.uint32)) and fig["best_threshold"].dtype == np.float32
    assert np.array_equal(fig["best_f1"], best["best_f1"], equal_nan=True) and _same(fig["macro_best_f1"], best["macro_best_f1"])
    return fig, err


def _raw(m, s, y):
    """The kernels' own integer outputs (sample positives, best_tp, best_n) against the restatement, past compute()'s packaging."""
    from mvfnet_amd import _lib
    m.compute()
    tp, nn, _ = m.pairs()
    dev, k, cap = m.device, m.num_classes, m.capacity
    st = torch.cuda.current_stream().cuda_stream
    s_ap, s_pos = torch.full((cap,), 7.0, dtype=torch.float64, device=dev), torch.full((cap,), 7, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.mvf_multilabel_sample_ap(m.rec_scores.data_ptr(), m.rec_labels.data_ptr(), cap, k, m.state.data_ptr(), s_ap.data_ptr(), s_pos.data_ptr(), st))
    positives = torch.from_numpy(mn.average_precision(s, y)["positives"]).to(dev)
    btp, bn = torch.full((k,), 7, dtype=torch.int32, device=dev), torch.full((k,), 7, dtype=torch.int32, device=dev)
    bth = torch.zeros(k, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib.mvf_multilabel_best_f1(m.rec_scores.data_ptr(), tp.data_ptr(), nn.data_ptr(), positives.data_ptr(), cap, k, m.state.data_ptr(),
                                               btp.data_ptr(), bn.data_ptr(), bth.data_ptr(), st))
    torch.cuda.synchronize()
    ref, best = fn.sample_ap(s, y), fn.best_f1(s, y)
    n = len(s)
    assert np.array_equal(s_pos.cpu().numpy()[:n], ref["positives"]) and (s_pos.cpu().numpy()[n:] == 0).all() and np.isnan(s_ap.cpu().numpy()[n:]).all()
    assert np.array_equal(btp.cpu().numpy(), best["best_tp"]) and np.array_equal(bn.cpu().numpy(), best["best_n"])


@pytest.mark.parametrize("kind", ["gauss", "quant", "equal", "inf", "nan"])
@pytest.mark.parametrize("classes", [1, 3, 64, 65, 157])
def test_figures_equal_the_restatement(classes, kind):
    """Capacities on both sides of the 64-row workgroup and of mvf_multilabel_ap's 256-row tile, records full and part full; classes on both sides of the
    64-class LDS tile and of the wavefront; label densities from none to all."""
    worst = 0.0
    per_class = np.linspace(-0.5, 1.0, classes).astype(np.float32)
    for capacity, rows in ((1, 1), (255, 255), (255, 100), (256, 256), (257, 257), (257, 65), (600, 600), (600, 320)):
        for density in ((0.0, 0.04, 0.5, 1.0) if capacity in (257, 600) and rows == capacity else (0.04, 0.5)):
            s, y = _case(rows, classes, kind, density)
            m = _feed(_metrics(classes, capacity), s, y)
            fig, err = _check(m, s, y, thresholds=per_class if density == 0.5 else None)
            worst = max(worst, err)
            if density == 0.5:
                _raw(m, s, y)
                again = m.compute(sample_ap=True, best_f1=True, threshold=0.25)         # bit-identical from run to run
                assert np.array_equal(again["sample_ap"], fig["sample_ap"], equal_nan=True) and _same(again["sample_mAP"], fig["sample_mAP"])
    print("classes=%d %s: worst relative sample-AP error %.3g (bound %g)" % (classes, kind, worst, AP_BOUND))


def test_defaults_return_todays_keys_and_each_option_adds_its_own():
    s, y = _case(100, 7, "quant", 0.3)
    m = _feed(_metrics(7, 128), s, y)
    plain = m.compute()
    assert set(plain) == BASE_KEYS and set(m.compute(strict=True)) == BASE_KEYS
    assert set(m.compute(sample_ap=True)) == BASE_KEYS | SAMPLE_KEYS
    assert set(m.compute(threshold=0.5)) == BASE_KEYS | PRF_KEYS and set(m.compute(thresholds=[0.5] * 7)) == BASE_KEYS | PRF_KEYS
    assert set(m.compute(best_f1=True)) == BASE_KEYS | BEST_KEYS
    full = m.compute(sample_ap=True, threshold=0.5, best_f1=True)
    assert all(np.array_equal(full[k], plain[k], equal_nan=True) for k in BASE_KEYS)           # the options change nothing of what was there
    for kw in (dict(threshold=0.5, thresholds=[0.5] * 7), dict(threshold=float("nan")), dict(thresholds=[0.5] * 6), dict(thresholds=[float("nan")] * 7),
               dict(threshold="0.5")):
        with pytest.raises(ValueError, match="threshold"):
            m.compute(**kw)
    # an empty record
    m.reset()
    fig = m.compute(sample_ap=True, threshold=0.5, best_f1=True)
    assert fig["sample_ap"].shape == (0,) and np.isnan(fig["sample_mAP"]) and fig["rows_with_positives"] == 0 and not fig["counts"].any()
    assert np.isnan(fig["best_threshold"]).all() and np.isnan(fig["macro_best_f1"]) and np.isnan(fig["macro_f1"]) and fig["micro_f1"] == 0.0


def test_appending_in_blocks_and_merged_records_equal_the_whole():
    s, y = _case(600, 65, "nan", 0.1, seed=2)
    whole = _feed(_metrics(65, 600), s, y)
    fig, _ = _check(whole, s, y)
    for block in (7, 250):
        got = _feed(_metrics(65, 600), s, y, block).compute(sample_ap=True, threshold=0.25, best_f1=True)
        assert all(np.array_equal(got[k], fig[k], equal_nan=True) for k in fig)
    # all_gather()'s merge: two records of different fill, concatenated with their NaN padding -- the slots of the second start at 320
    a, b = _feed(_metrics(65, 320), s[:290], y[:290]), _feed(_metrics(65, 320), s[290:], y[290:])
    m = _metrics(65, 1)
    m.merge([(a.rec_scores, a.rec_labels, a.state), (b.rec_scores, b.rec_labels, b.state)])
    got = m.compute(sample_ap=True, threshold=0.25, best_f1=True)
    assert m.capacity == 640 and got["sample_ap"].shape == (640,)
    for k in ("counts", "precision", "recall", "f1", "best_f1", "rows_with_positives"):
        assert np.array_equal(got[k], fig[k], equal_nan=True), k
    assert np.array_equal(got["best_threshold"].view(np.uint32), fig["best_threshold"].view(np.uint32))
    placed = np.full(640, np.nan)
    placed[:290], placed[320:320 + 310] = fig["sample_ap"][:290], fig["sample_ap"][290:]
    assert np.array_equal(got["sample_ap"], placed, equal_nan=True)       # a row's AP depends on the row alone: the same bits, at its slot
    assert abs(got["sample_mAP"] - fig["sample_mAP"]) <= AP_BOUND * fig["sample_mAP"]


# ------------------------------------------------------------------------------------------------ the hook
CLASSES = 10


def _model(average_clips):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=CLASSES, dropout_ratio=0.0)
    cfg["cls_head"]["loss_cls"] = dict(type="AsymmetricLossMultiLabel")
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=average_clips))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().eval()


def test_the_hook_agrees_between_the_host_and_the_device_path():
    from mvfnet_amd.evaluation import EvalMeanAPHook, mmit_mean_average_precision, precision_recall_f1
    from mvfnet_amd.runner import single_gpu_test
    model = _model("sigmoid")
    videos = [dict(img_group=torch.from_numpy(synth.synth_clip_batch(1, 8, 32, 32, seed=300 + i)).cuda()) for i in range(8)]
    rows = np.stack([np.asarray(r).reshape(-1) for r in single_gpu_test(model, videos)])
    labels = np.random.default_rng(1).random((8, CLASSES)) < 0.4
    labels[:, 3] = False
    labels[5] = False
    thr = float(np.median(rows))

    class _Runner(object):
        epoch = 1
    runner = _Runner()
    runner.model = model
    plain_h = EvalMeanAPHook(videos, labels).after_train_epoch(runner)
    plain_d = EvalMeanAPHook(videos, labels, on_device=True).after_train_epoch(runner)
    assert set(plain_h) == {"mAP", "epoch"} and set(plain_d) == {"mAP", "epoch"}
    host = EvalMeanAPHook(videos, labels, sample_map=True, f1_threshold=thr).after_train_epoch(runner)
    dev = EvalMeanAPHook(videos, labels, on_device=True, sample_map=True, f1_threshold=thr).after_train_epoch(runner)
    assert set(host) == set(dev) == {"mAP", "sample mAP", "micro F1", "macro F1", "epoch"}
    assert set(EvalMeanAPHook(videos, labels, sample_map=True).after_train_epoch(runner)) == {"mAP", "sample mAP", "epoch"}
    assert set(EvalMeanAPHook(videos, labels, on_device=True, f1_threshold=thr).after_train_epoch(runner)) == {"mAP", "micro F1", "macro F1", "epoch"}
    want = mmit_mean_average_precision(rows, labels)
    prf = precision_recall_f1(rows, labels, threshold=thr)
    assert 0.0 < prf["micro_f1"] < 1.0 and host["mAP"] == plain_h["mAP"] and dev["mAP"] == plain_d["mAP"]
    assert abs(host["sample mAP"] - want) <= AP_BOUND * want and abs(dev["sample mAP"] - want) <= AP_BOUND * want
    # counts are integers: the F1 figures are the same numbers on either path
    assert (host["micro F1"], host["macro F1"]) == (prf["micro_f1"], prf["macro_f1"]) == (dev["micro F1"], dev["macro F1"])
