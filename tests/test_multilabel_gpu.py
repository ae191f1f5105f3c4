"""GPU: multi-label evaluation on the device -- mvf_multilabel_record / mvf_multilabel_ap (csrc/multilabel_metrics.hip), metrics.DeviceMultiLabelMetrics,
runner.device_test with a label matrix and evaluation.EvalMeanAPHook(on_device=True).

The pair counts (TP_i, N_i) and the positives are integers: compared exactly against the numpy restatement (tests/multilabel_numpy.py).  ap and mAP are fp64
sums of at most 1000 ratios in [0, 1], the kernel's in another order than numpy's: 1e-12 relative (1000 * 2^-53 = 1.1e-13 at the very worst)."""
import numpy as np
import pytest
import torch

import multilabel_numpy as mn
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

AP_BOUND = 1e-12


def _case(rows, classes, kind, seed=0, density=0.3):
    gen = np.random.default_rng(seed * 7919 + rows * 31 + classes)
    if kind == "ties":
        s = gen.integers(-2, 3, (rows, classes)).astype(np.float32)          # five distinct values: heavy ties
    else:
        s = gen.standard_normal((rows, classes)).astype(np.float32)
    return s, (gen.random((rows, classes)) < density).astype(np.uint8)


def _metrics(classes, capacity):
    from mvfnet_amd.metrics import DeviceMultiLabelMetrics
    return DeviceMultiLabelMetrics(classes, capacity)


def _feed(m, s, y, block=None):
    block = block or len(s)
    for i in range(0, len(s), block):
        m.update(torch.from_numpy(s[i:i + block]).cuda(), torch.from_numpy(y[i:i + block]).cuda())
    return m


def _check(m, s, y, slots=None):
    """compute() and the pair arrays against the restatement.  slots: rows that took a slot (default: all of s)."""
    fig = m.compute()
    ref = mn.average_precision(s, y)
    tp, nn, used = m.pairs()
    n = len(s) if slots is None else slots
    assert used == n
    assert np.array_equal(tp[:, :n].cpu().numpy(), ref["tp"]) and np.array_equal(nn[:, :n].cpu().numpy(), ref["nn"])
    assert np.array_equal(fig["positives"], ref["positives"]) and fig["positives"].dtype == np.int64
    assert (fig["rows"], fig["nan_rows"], fig["overflow"], fig["classes_with_positives"]) == (ref["rows"], ref["nan_rows"], 0, ref["classes_with_positives"])
    have = ref["positives"] > 0
    assert np.array_equal(np.isnan(fig["ap"]), ~have)
    err = float(np.max(np.abs(fig["ap"][have] - ref["ap"][have]) / ref["ap"][have])) if have.any() else 0.0
    assert err <= AP_BOUND, err
    if have.any():
        assert abs(fig["mAP"] - ref["mAP"]) <= AP_BOUND * ref["mAP"]
    else:
        assert np.isnan(fig["mAP"])
    return fig, err


@pytest.mark.parametrize("kind", ["ties", "gauss"])
@pytest.mark.parametrize("classes", [1, 3, 157])
def test_pairs_and_ap_equal_the_restatement(classes, kind):
    """Rows on both sides of the wavefront (64) and of the kernel's 256-row workgroup / 256-entry LDS tile; 1000 rows: four tiles, the last one partial."""
    worst = 0.0
    for rows in (1, 63, 64, 65, 257, 1000):
        s, y = _case(rows, classes, kind)
        m = _feed(_metrics(classes, rows + (rows % 3)), s, y)               # capacity == rows and capacity > rows
        fig, err = _check(m, s, y)
        worst = max(worst, err)
        again = m.compute()                                                # bit-identical from run to run
        assert np.array_equal(again["ap"], fig["ap"], equal_nan=True) and np.array_equal(again["mAP"], fig["mAP"], equal_nan=True)
    print("classes=%d %s: worst relative AP error %.3g (bound %g)" % (classes, kind, worst, AP_BOUND))


def test_appending_in_blocks_equals_one_update():
    s, y = _case(1000, 5, "ties", seed=2)
    whole = _feed(_metrics(5, 1000), s, y)
    fig, _ = _check(whole, s, y)
    for block in (1, 7, 250):
        part = _feed(_metrics(5, 1000), s, y, block)
        assert torch.equal(part.rec_scores, whole.rec_scores) and torch.equal(part.rec_labels, whole.rec_labels) and torch.equal(part.state, whole.state)
        got = part.compute()
        assert np.array_equal(got["ap"], fig["ap"]) and got["mAP"] == fig["mAP"] and np.array_equal(got["positives"], fig["positives"])
    # bool labels are the uint8 ones; reset() starts a new pass in the same record
    whole.reset()
    assert whole.compute()["rows"] == 0 and np.isnan(whole.compute()["mAP"])
    whole.update(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda().bool())
    assert np.array_equal(whole.compute()["ap"], fig["ap"])


def test_a_nan_row_is_excluded_and_counted_and_inf_is_a_value():
    s, y = _case(300, 4, "gauss", seed=4)
    s[::9, 0], s[1::11, 0], s[::5, 2] = np.inf, -np.inf, -np.inf
    s[7, 1] = s[200, 3] = s[299, 0] = np.nan
    y[7] = 1
    m = _feed(_metrics(4, 320), s, y, block=64)
    fig, _ = _check(m, s, y)
    assert (fig["rows"], fig["nan_rows"]) == (297, 3)
    ok = mn.valid_rows(s)
    alone = _feed(_metrics(4, 320), s[ok], y[ok]).compute()
    # the same integer ratios; the lanes of the fp64 sum take other rows once three slots are gone
    assert np.abs(alone["ap"] - fig["ap"]).max() <= AP_BOUND and np.array_equal(alone["positives"], fig["positives"])


def test_overflow_is_counted_and_compute_raises():
    s, y = _case(100, 3, "gauss", seed=5)
    m = _feed(_metrics(3, 90), s, y, block=40)                              # 40 + 40 + 10 of the last 20
    with pytest.raises(RuntimeError, match="10 of 100 rows did not fit"):
        m.compute()
    fig = m.compute(strict=False)
    assert (fig["overflow"], fig["rows"]) == (10, 90)
    ref = mn.average_precision(s[:90], y[:90])
    assert np.array_equal(fig["positives"], ref["positives"]) and np.nanmax(np.abs(fig["ap"] - ref["ap"])) <= AP_BOUND
    m.update(torch.from_numpy(s[:5]).cuda(), torch.from_numpy(y[:5]).cuda())       # a full record takes nothing more
    assert m.compute(strict=False)["overflow"] == 15 and np.array_equal(m.compute(strict=False)["ap"], fig["ap"])


def test_a_class_without_positives_is_nan_and_left_out_of_the_mean():
    s, y = _case(65, 6, "ties", seed=6)
    y[:, 2], y[:, 4], y[:, 5] = 0, 0, 1
    fig, _ = _check(_feed(_metrics(6, 65), s, y), s, y)
    assert np.isnan(fig["ap"][[2, 4]]).all() and fig["ap"][5] == 1.0 and fig["classes_with_positives"] == 4
    assert abs(fig["mAP"] - np.mean(fig["ap"][[0, 1, 3, 5]])) <= AP_BOUND
    none, _ = _check(_feed(_metrics(6, 65), s, np.zeros_like(y)), s, np.zeros_like(y))
    assert np.isnan(none["mAP"]) and none["classes_with_positives"] == 0


def test_merged_records_equal_one_record_and_update_refusals():
    """all_gather()'s merge, without a process group: two ranks' records of different fill, concatenated with their NaN padding."""
    from mvfnet_amd.metrics import DeviceMultiLabelMetrics
    s, y = _case(257, 7, "ties", seed=8)
    s[100, 3] = np.nan
    a, b = _feed(_metrics(7, 160), s[:150], y[:150]), _feed(_metrics(7, 160), s[150:], y[150:])
    m = _metrics(7, 1)
    m.merge([(a.rec_scores, a.rec_labels, a.state), (b.rec_scores, b.rec_labels, b.state)])
    fig = m.compute()
    ref = mn.average_precision(s, y)
    assert m.capacity == 320 and (fig["rows"], fig["nan_rows"]) == (256, 1) and np.array_equal(fig["positives"], ref["positives"])
    assert np.nanmax(np.abs(fig["ap"] - ref["ap"]) / ref["ap"]) <= AP_BOUND and abs(fig["mAP"] - ref["mAP"]) <= AP_BOUND
    m.all_gather()                                                          # no process group: nothing happens
    assert m.capacity == 320
    m = DeviceMultiLabelMetrics(7, 10)
    sc, lb = torch.zeros(2, 7, device="cuda"), torch.zeros(2, 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="device tensors required"):
        m.update(sc.cpu(), lb.cpu())
    for bad_s, bad_l in ((sc.double(), lb), (sc[:, :6], lb[:, :6]), (sc, lb.long()), (sc, lb[:1]), (sc.t().contiguous().t(), lb)):
        with pytest.raises(ValueError):
            m.update(bad_s, bad_l)
    assert m.compute()["rows"] == 0


# ------------------------------------------------------------------------------------------------ evaluation passes
CLASSES = 10


def _model(average_clips):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=CLASSES, dropout_ratio=0.0)
    cfg["cls_head"]["loss_cls"] = dict(type="BCELossWithLogits")
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=average_clips))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().eval()


def test_device_test_and_the_hook_equal_the_host_path():
    from mvfnet_amd.evaluation import EvalMeanAPHook, mean_average_precision
    from mvfnet_amd.metrics import DeviceMetrics, DeviceMultiLabelMetrics
    from mvfnet_amd.runner import device_test, single_gpu_test
    import bce_numpy as bn
    model = _model("sigmoid")
    videos = [dict(img_group=torch.from_numpy(synth.synth_clip_batch(1, 8, 32, 32, seed=300 + i)).cuda()) for i in range(8)]
    rows = np.stack([np.asarray(r).reshape(-1) for r in single_gpu_test(model, videos)])
    assert rows.shape == (8, CLASSES) and np.isfinite(rows).all() and (rows >= 0).all() and (rows <= 1).all()
    # 'sigmoid' averaging is the mean over the video's two clips of sigmoid(score)
    model.test_cfg = dict(average_clips=None)
    raw = np.asarray(single_gpu_test(model, videos[:1])[0])
    model.test_cfg = dict(average_clips="sigmoid")
    assert raw.shape == (2, CLASSES) and np.abs(rows[:1] - bn.average_clip_sigmoid(raw)).max() <= 1e-5
    gen = np.random.default_rng(1)
    labels = gen.random((8, CLASSES)) < 0.4
    labels[:, 3] = False
    want = mean_average_precision(rows, labels)
    metrics = DeviceMultiLabelMetrics(CLASSES, capacity=8)
    assert device_test(model, videos, labels, metrics) is metrics
    fig = metrics.compute()
    assert fig["rows"] == 8 and np.isnan(fig["ap"][3]) and abs(fig["mAP"] - want) <= AP_BOUND * want, (fig["mAP"], want)
    again = DeviceMultiLabelMetrics(CLASSES, capacity=8)                    # labels already on the device, as uint8
    device_test(model, videos, torch.from_numpy(labels.astype(np.uint8)).cuda(), again)
    assert torch.equal(again.rec_scores, metrics.rec_scores) and torch.equal(again.rec_labels, metrics.rec_labels)
    with pytest.raises(ValueError, match="label matrix"):
        device_test(model, videos, labels[:, :4], DeviceMultiLabelMetrics(CLASSES, capacity=8))
    with pytest.raises(ValueError, match="there are 7 labels"):
        device_test(model, videos, labels[:7], DeviceMultiLabelMetrics(CLASSES, capacity=8))
    with pytest.raises(ValueError, match="one integer label per video"):     # a DeviceMetrics behaves and raises as it did
        device_test(model, videos, [[0, 1]] * 7 + [[2]], DeviceMetrics(CLASSES))

    class _Runner(object):
        epoch = 1
    runner = _Runner()
    runner.model = model
    host = EvalMeanAPHook(videos, labels).after_train_epoch(runner)
    dev = EvalMeanAPHook(videos, labels, on_device=True).after_train_epoch(runner)
    assert set(host) == {"mAP", "epoch"} and abs(host["mAP"] - want) <= AP_BOUND * want and abs(dev["mAP"] - want) <= AP_BOUND * want
    model.test_cfg = dict(average_clips=None)
    with pytest.raises(ValueError, match="average_clips"):
        EvalMeanAPHook(videos, labels, on_device=True).after_train_epoch(runner)
