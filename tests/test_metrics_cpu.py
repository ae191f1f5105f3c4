"""CPU: the host side of the device-side accuracy -- the numpy restatement of the kernel's rules (tests/metrics_numpy.py) against evaluation.top_k_accuracy /
mean_class_accuracy, its tie / NaN / bad-label rules on hand-written rows, the C ABI of mvf_metrics_update / mvf_metrics_state_words (symbols, signatures and
the argument checks, which return their status from host pointers before any launch), check_train_accuracy, the Runner's log line with a stub engine, and
the arithmetic of DeviceMetrics.compute() on a state array filled on the host."""
import ctypes as C

import numpy as np
import pytest

import metrics_numpy as mn

EINVAL, ESHAPE = -1, -2


# ------------------------------------------------------------------------------------------------ the restatement against the host functions
@pytest.mark.parametrize("classes,rows", [(1000, 300), (400, 257), (101, 64), (12, 200)])
def test_restatement_equals_the_host_functions_on_tie_free_rows(classes, rows):
    from mvfnet_amd.evaluation import mean_class_accuracy, top_k_accuracy
    scores, labels, ranks = mn.permutation_rows(rows, classes, seed=classes + rows)
    assert all(len(np.unique(r)) == classes for r in scores)                       # distinct by construction
    ks = (1, 3, 5, 9)                                                              # ranks are drawn from 0..9: no k covers them all
    state, rank, pred = mn.metrics_ref(scores, labels, ks, True)
    assert np.array_equal(rank, ranks) and np.array_equal(pred, np.argmax(scores, axis=1))
    want = [int(np.count_nonzero(ranks < k)) for k in ks]
    assert all(0 < w < rows for w in want), want                                   # every rate strictly between 0 and 1
    host = top_k_accuracy(list(scores), [int(v) for v in labels], k=ks)
    assert [int(state[mn.HITS + i]) for i in range(len(ks))] == want
    assert [round(float(a) * rows) for a in host] == want and all(abs(float(a) * rows - w) < 1e-9 for a, w in zip(host, want))
    assert state[0] == rows and state[1] == 0 and state[2] == 0 and not state[3:8].any() and not state[mn.HITS + len(ks):mn.HEADER].any()
    cf = state[mn.HEADER:].reshape(classes, classes)
    assert int(np.trace(cf)) == want[0] and int(cf.sum()) == rows
    from mvfnet_amd.metrics import mean_class_from_confusion
    assert mean_class_from_confusion(cf) == pytest.approx(float(mean_class_accuracy(scores, labels)), rel=0, abs=1e-15)
    assert 0.0 < mean_class_from_confusion(cf) < 1.0


def test_tie_rule_of_the_restatement():
    s = np.array([[1.0, 2.0, 2.0, 2.0, 0.0],      # label 2: one equal score at a lower index -> rank 1; pred = 1
                  [1.0, 2.0, 2.0, 2.0, 0.0],      # label 1: first of the equals -> rank 0
                  [3.0, 3.0, 3.0, 3.0, 3.0],      # all equal, label 4 -> rank 4, pred 0
                  [3.0, 3.0, 3.0, 3.0, 3.0],      # all equal, label 0 -> rank 0
                  [-np.inf, np.inf, 0.0, np.inf, -np.inf],      # label 3: +inf at index 1 ties and is lower -> rank 1; pred 1
                  [-np.inf, -np.inf, -np.inf, -np.inf, -np.inf]], dtype=np.float32)      # label 2 -> rank 2, pred 0
    y = np.array([2, 1, 4, 0, 3, 2])
    state, rank, pred = mn.metrics_ref(s, y, (1, 2, 5), True)
    assert rank.tolist() == [1, 0, 4, 0, 1, 2] and pred.tolist() == [1, 1, 0, 0, 1, 0]
    assert state[:3].tolist() == [6, 0, 0] and state[mn.HITS:mn.HITS + 3].tolist() == [2, 4, 6]
    cf = state[mn.HEADER:].reshape(5, 5)
    assert int(np.trace(cf)) == 2 and cf[2, 1] == 1 and cf[1, 1] == 1 and cf[4, 0] == 1 and cf[0, 0] == 1 and cf[3, 1] == 1 and cf[2, 0] == 1
    # k >= classes always hits on a valid row
    assert mn.metrics_ref(s, y, (5, 9), False)[0][mn.HITS:mn.HITS + 2].tolist() == [6, 6]


def test_nan_and_bad_label_rules_of_the_restatement():
    s = np.array([[0.0, 1.0, 2.0], [0.0, np.nan, 2.0], [np.nan, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [np.nan, 1.0, 2.0]], dtype=np.float32)
    y = np.array([2, 1, 2, -1, 3, 1 << 40])       # valid, NaN at the label, NaN elsewhere, three bad labels (the last one on a NaN row: the label wins)
    state, rank, pred = mn.metrics_ref(s, y, (1, 3), True)
    assert state[:3].tolist() == [6, 3, 2] and state[mn.HITS:mn.HITS + 2].tolist() == [1, 1]
    assert rank.tolist() == [0, -1, -1, -1, -1, -1] and pred.tolist() == [2, -1, -1, -1, -1, -1]
    cf = state[mn.HEADER:].reshape(3, 3)
    assert int(cf.sum()) == 1 and cf[2, 2] == 1
    # accumulation onto an existing state
    again, _, _ = mn.metrics_ref(s, y, (1, 3), True, state=state)
    assert np.array_equal(again, 2 * state)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_typed():
    from mvfnet_amd import _lib
    declared = _lib.declared_symbols()
    for name, nargs in (("mvf_metrics_state_words", 2), ("mvf_metrics_update", 11)):
        assert name in declared
        fn = getattr(_lib.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert _lib.lib.mvf_metrics_update.restype is C.c_int and _lib.lib.mvf_metrics_state_words.restype is C.c_size_t
    assert _lib.lib.mvf_abi_version() == 2         # additions only
    assert (_lib.METRICS_HITS, _lib.METRICS_MAX_K, _lib.METRICS_CONFUSION) == (mn.HITS, mn.MAX_K, mn.HEADER)


def test_state_words():
    from mvfnet_amd import _lib
    words = _lib.lib.mvf_metrics_state_words
    assert words(400, 0) == 16 and words(400, 1) == 16 + 160000 and words(1, 1) == 17 and words(1, 0) == 16
    assert words(46340, 1) == 16 + 46340 * 46340 and words(46341, 1) == 0 and words(46341, 0) == 16
    assert words(0, 0) == 0 and words(-3, 1) == 0
    for classes, conf in ((400, 0), (400, 1), (7, 1)):
        assert words(classes, conf) == mn.state_words(classes, conf)


def test_argument_failures_return_their_status_before_any_launch():
    """Host arrays stand in for the device operands: every refusal comes back on a machine without a GPU and nothing is dereferenced or written."""
    from mvfnet_amd import _lib
    lib, err = _lib.lib, _lib.lib.mvf_last_error
    f = (C.c_float * 64)()
    lab = (C.c_longlong * 8)()
    state = (C.c_longlong * 64)()
    rec = (C.c_int * 16)()
    P = lambda a, off=0: C.cast(a, C.c_void_p).value + off      # noqa: E731
    ks = (C.c_int * 8)(1, 5, 2, 3, 4, 6, 7, 8)

    def call(scores=P(f), rows=4, classes=5, labels=P(lab), k=ks, nk=2, st=P(state), conf=1, rank=P(rec), pred=P(rec, 32)):
        return lib.mvf_metrics_update(scores, rows, classes, labels, k, nk, st, conf, rank, pred, None)
    for name in ("scores", "labels", "st", "k"):
        assert call(**{name: None}) == EINVAL and b"NULL" in err(), name
    for classes in (0, -1):
        assert call(classes=classes) == ESHAPE and b"classes" in err()
    assert call(rows=-1) == ESHAPE and b"rows" in err()
    for nk in (0, -1, 9):
        assert call(nk=nk) == ESHAPE and b"nk" in err()
    for bad in ((0, 5), (1, 0), (1, -2)):
        assert call(k=(C.c_int * 2)(*bad)) == ESHAPE and b"ks[" in err(), bad
    assert call(k=(C.c_int * 8)(1, 2, 3, 4, 5, 6, 7, 0), nk=8) == ESHAPE and b"ks[7]" in err()
    assert call(k=(C.c_int * 8)(1, 2, 3, 4, 5, 6, 7, 0), nk=7, rows=0) == 0          # the eighth entry is not part of the call
    assert call(classes=46341, rows=0) == ESHAPE and b"confusion" in err()           # refused with rows == 0 as well: checks come first
    assert call(classes=46341, rows=0, conf=0) == 0
    assert call(st=P(state, 4)) == EINVAL and b"misaligned" in err()
    assert call(labels=P(lab, 4)) == EINVAL and call(scores=P(f, 2)) == EINVAL and call(rank=P(rec, 2)) == EINVAL and call(pred=P(rec, 1)) == EINVAL
    # rows == 0: MVF_OK without a launch, with and without the record arrays
    assert call(rows=0) == 0 and call(rows=0, rank=None, pred=None) == 0 and call(rows=0, nk=8) == 0
    assert not any(state) and not any(rec) and not any(lab) and not any(f)
    assert lib.mvf_abi_version() == 2


# ------------------------------------------------------------------------------------------------ configuration
def test_check_train_accuracy():
    from mvfnet_amd.metrics import check_train_accuracy
    from mvfnet_amd.runner import Config
    assert check_train_accuracy(None) is None
    assert check_train_accuracy({}) == dict(k=(1, 5))
    assert check_train_accuracy(dict(k=(1,))) == dict(k=(1,))
    assert check_train_accuracy(dict(k=[1, 3, 5])) == dict(k=(1, 3, 5))
    assert check_train_accuracy(Config(k=(2, 4))) == dict(k=(2, 4))
    out = check_train_accuracy(dict(k=(np.int64(1), np.int32(5))))
    assert out == dict(k=(1, 5)) and all(type(v) is int for v in out["k"])
    assert check_train_accuracy(dict(k=3)) == dict(k=(3,))
    for bad in ((), (0,), (1, -5), (1, 2.0), (True,), "15", None, tuple(range(1, 10)), True):
        with pytest.raises(ValueError, match="k must be"):
            check_train_accuracy(dict(k=bad))
    with pytest.raises(ValueError, match="unknown key 'topk'"):
        check_train_accuracy(dict(topk=(1, 5)))
    for bad in (True, (1, 5), "on"):
        with pytest.raises(ValueError, match="train_accuracy must be"):
            check_train_accuracy(bad)


def test_runner_and_train_network_refuse_a_bad_config_before_anything_is_built():
    from mvfnet_amd.runner import Runner, train_network

    class Untouched(object):
        def __getattr__(self, name):
            raise AssertionError("the model was touched (%s)" % name)
    with pytest.raises(ValueError, match="unknown key"):
        Runner(Untouched(), train_accuracy=dict(top=5))
    with pytest.raises(ValueError, match="k must be"):
        Runner(Untouched(), train_accuracy=dict(k=(0,)))
    with pytest.raises(ValueError, match="k must be"):
        train_network(Untouched(), [], dict(train_accuracy=dict(k=()), optimizer=dict(type="SGD", lr=0.01)))
    with pytest.raises(ValueError, match="train_accuracy must be"):
        train_network(Untouched(), [], dict(train_accuracy=True, optimizer=dict(type="SGD", lr=0.01)))


# ------------------------------------------------------------------------------------------------ the log line
class _Engine(object):
    flat_ema, max_norm, initial_lr = None, None, None
    norm_out = [1.5]
    accumulated_loss = 0.75

    def __init__(self):
        self.calls, self.enabled = [], None

    def train_step(self, imgs, labels, lr=None):
        self.calls.append("step")
        return 0.25

    def accumulate_step(self, imgs, labels):
        self.calls.append("micro")

    def apply_accumulated(self, lr=None):
        self.calls.append("apply")


class _AccEngine(_Engine):
    def enable_train_accuracy(self, k=(1, 5)):
        self.enabled = tuple(k)

    def train_accuracy(self):
        self.calls.append("read")
        return dict(count=4, top1=0.25, top5=0.5, top3=0.375, invalid=0, nan_rows=0)

    def enable_step_guard(self):
        pass

    def guard_state(self):
        return dict(skipped_last=False, skipped=2, consecutive=0, steps=3)


class _Model(object):
    def __init__(self, eng):
        self.eng = eng

    def train_engine(self, **opt):
        return self.eng

    def train(self, mode=True):
        return self


BATCH = dict(img_group="x", label="y")


def test_log_line_is_unchanged_with_the_option_off():
    """The stub engine has none of the option's methods: a Runner that was not given train_accuracy must not miss them, and the line is what it was."""
    from mvfnet_amd.runner import Runner
    lines, eng = [], _Engine()
    run = Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None)
    assert run.train_accuracy is None
    run.train_epoch([BATCH])
    assert lines == ["Epoch [1] iter 1 lr 0.01000 loss_cls 0.2500 grad_norm 1.500"]
    lines2, eng2 = [], _Engine()
    run2 = Runner(_Model(eng2), logger=lines2.append, log_interval=1, lr=0.01, warmup=None, accumulate=2)
    run2.train_epoch([BATCH, BATCH])
    assert lines2 == ["Epoch [1] iter 1 lr 0.01000 loss_cls 0.7500 grad_norm 1.500"]


def test_log_line_carries_the_two_figures_after_grad_norm_and_before_the_guard_note():
    from mvfnet_amd.runner import Runner
    lines, eng = [], _AccEngine()
    run = Runner(_Model(eng), logger=lines.append, log_interval=2, lr=0.01, warmup=None, train_accuracy={})
    assert run.train_accuracy == dict(k=(1, 5)) and eng.enabled == (1, 5)
    run.train_epoch([BATCH] * 4)
    assert lines == ["Epoch [1] iter %d lr 0.01000 loss_cls 0.2500 grad_norm 1.500 top1 0.2500 top5 0.5000" % i for i in (2, 4)]
    assert eng.calls == ["step", "step", "read", "step", "step", "read"]          # read at the log interval only
    # with the guard's note behind it, other k, and under accumulation
    lines, eng = [], _AccEngine()
    run = Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None, train_accuracy=dict(k=(1, 3)), nonfinite_guard={}, accumulate=2)
    assert eng.enabled == (1, 3)
    run.train_epoch([BATCH] * 3)
    assert lines == ["Epoch [1] iter %d lr 0.01000 loss_cls 0.7500 grad_norm 1.500 top1 0.2500 top3 0.3750 skipped 2" % i for i in (1, 2)]
    assert eng.calls == ["micro", "micro", "apply", "read", "micro", "apply", "read"]


# ------------------------------------------------------------------------------------------------ compute()
def _filled(classes, k, cf, hits, rows=None, invalid=0, nan_rows=0):
    import torch
    from mvfnet_amd.metrics import DeviceMetrics
    m = DeviceMetrics(classes, k=k, confusion=cf is not None, device="cpu")
    st = np.zeros(m.state.numel(), np.int64)
    st[0] = (int(np.sum(cf)) if rows is None else rows) + invalid + nan_rows
    st[1], st[2] = invalid, nan_rows
    st[8:8 + len(hits)] = hits
    if cf is not None:
        st[16:] = np.asarray(cf).reshape(-1)
    m.state.copy_(torch.from_numpy(st))
    return m


def test_compute_arithmetic_on_a_state_filled_on_the_host():
    from mvfnet_amd.evaluation import mean_class_accuracy
    # class 0: 3 of 4 right; class 1: 0 of 2; class 2 never a label but predicted twice (contributes 0); class 3 occurs nowhere (left out)
    cf = np.array([[3, 0, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    m = _filled(4, (1, 2), cf, hits=(3, 5))
    out = m.compute()
    assert set(out) == {"count", "top1", "top2", "mean_class_acc", "confusion", "invalid", "nan_rows"}
    assert out["count"] == 6 and out["top1"] == 3 / 6 and out["top2"] == 5 / 6 and out["invalid"] == 0 and out["nan_rows"] == 0
    assert out["mean_class_acc"] == pytest.approx((0.75 + 0.0 + 0.0) / 3, abs=1e-15)
    assert out["confusion"].dtype == np.int64 and np.array_equal(out["confusion"], cf)
    # the same figure from evaluation.mean_class_accuracy on rows that realise this matrix
    pred = np.array([0, 0, 0, 2, 0, 2])
    labels = np.array([0, 0, 0, 0, 1, 1])
    assert out["mean_class_acc"] == pytest.approx(float(mean_class_accuracy(np.eye(4)[pred], labels)), abs=1e-15)
    # strict mode names the counts; strict=False counts the bad rows as misses
    bad = _filled(4, (1, 2), cf, hits=(3, 5), invalid=2, nan_rows=1)
    with pytest.raises(ValueError, match=r"2 of 9 rows have a label outside \[0, 4\) and 1 hold a NaN"):
        bad.compute()
    with pytest.raises(ValueError):
        _filled(4, (1,), cf, hits=(3,), nan_rows=1).compute(strict=True)
    out = bad.compute(strict=False)
    assert out["count"] == 9 and out["top1"] == 3 / 9 and out["invalid"] == 2 and out["nan_rows"] == 1
    # without the matrix, and an empty window
    out = _filled(400, (1, 5), None, hits=(1, 2), rows=4).compute()
    assert out["top1"] == 0.25 and out["top5"] == 0.5 and out["mean_class_acc"] is None and out["confusion"] is None
    empty = _filled(4, (1,), np.zeros((4, 4), int), hits=(0,)).compute()
    assert empty["count"] == 0 and np.isnan(empty["top1"]) and np.isnan(empty["mean_class_acc"])


def test_device_metrics_refuses_bad_arguments_and_host_tensors():
    import torch
    from mvfnet_amd.metrics import DeviceMetrics
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="num_classes"):
            DeviceMetrics(bad, device="cpu")
    with pytest.raises(ValueError, match="k must be"):
        DeviceMetrics(4, k=(), device="cpu")
    with pytest.raises(ValueError, match="record"):
        DeviceMetrics(4, record=-1, device="cpu")
    with pytest.raises(ValueError, match="confusion=False"):
        DeviceMetrics(46341, device="cpu")
    m = DeviceMetrics(4, device="cpu")
    with pytest.raises(RuntimeError, match="device tensors"):
        m.update(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="record=0"):
        m.records()
    m.all_reduce()                                   # no process group: nothing happens
    assert m.compute()["count"] == 0
