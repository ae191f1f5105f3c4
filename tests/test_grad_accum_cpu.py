"""CPU: the step boundary of gradient accumulation in the runner (Runner(accumulate=k), cfg.optimizer_config.accumulate) with an engine that only records its
calls, and the declaration of the new export.  k loader batches make one optimizer step; `iter`, the warm-up and the log interval count optimizer steps (what
they mean in the reference at 8 x 12 clips per step, codes/core/train.py:159-252); the epoch's trailing group is applied with its real count."""
import ctypes

import pytest
import torch

from mvfnet_amd import runner as R


class _Engine(object):
    def __init__(self):
        self.calls, self.accumulated_count, self.norm_out = [], 0, [1.5]
        self.accumulated_loss = None

    def accumulate_step(self, imgs, labels):
        self.calls.append(("micro", int(imgs[0, 0])))
        self.accumulated_count += 1
        return torch.tensor([0.5])

    def apply_accumulated(self, lr=None):
        if self.accumulated_count == 0:
            raise RuntimeError("nothing has been accumulated")
        self.calls.append(("apply", lr, self.accumulated_count))
        self.accumulated_loss = torch.tensor([0.25 * self.accumulated_count])
        self.accumulated_count = 0
        return self.norm_out

    def train_step(self, imgs, labels, lr=None):
        self.calls.append(("train_step", lr))
        return torch.tensor([0.75])


class _Optimizer(object):
    def __init__(self, lr=0.01):
        self.engine, self.param_groups = _Engine(), [dict(lr=lr)]


class _Model(object):
    def train(self):
        return self

    def cuda(self):
        return self


def _batches(n):
    return [dict(img_group=torch.full((2, 3), float(i)), label=torch.tensor([i, i])) for i in range(n)]


SCHEDULE = dict(lr_steps=(90, 130), warmup="linear", warmup_iters=4, warmup_ratio=0.1)


def _expected(calls_per_group, lr=0.01):
    want, first = [], 0
    for step, c in enumerate(calls_per_group):
        want += [("micro", first + j) for j in range(c)]
        want.append(("apply", R.step_lr(lr, 0, step, (90, 130), 0.1, "linear", 4, 0.1), c))
        first += c
    return want


def test_runner_groups_seven_batches_into_three_optimizer_steps():
    opt, logs = _Optimizer(), []
    run = R.Runner(_Model(), optimizer=opt, max_norm=40.0, ckpt_interval=0, log_interval=1, logger=logs.append, accumulate=3, **SCHEDULE)
    run.run(_batches(7), 1)
    assert opt.engine.calls == _expected([3, 3, 1])                   # 3 + 3 + 1 micro-steps, the lr of optimizer step 0, 1, 2, the last group's count 1
    lrs = [c[1] for c in opt.engine.calls if c[0] == "apply"]
    assert lrs[0] < lrs[1] < lrs[2] < 0.01                            # the warm-up advances per optimizer step
    assert run.iter == 3 and run.epoch == 1 and opt.engine.accumulated_count == 0
    assert len(logs) == 3 and "iter 3 " in logs[2] and "loss_cls 0.2500" in logs[2] and "loss_cls 0.7500" in logs[0]      # the line reports accumulated_loss
    run.run(_batches(7), 2)                                           # nothing carries over the epoch boundary
    assert run.iter == 6 and [c[2] for c in opt.engine.calls if c[0] == "apply"] == [3, 3, 1, 3, 3, 1]


def test_a_group_that_ends_with_the_epoch_is_applied_once():
    opt = _Optimizer()
    run = R.Runner(_Model(), optimizer=opt, max_norm=None, ckpt_interval=0, log_interval=0, accumulate=3, **SCHEDULE)
    run.run(_batches(6), 1)
    assert [c[2] for c in opt.engine.calls if c[0] == "apply"] == [3, 3] and run.iter == 2


def test_accumulate_one_is_the_train_step_path():
    opt = _Optimizer()
    run = R.Runner(_Model(), optimizer=opt, max_norm=None, ckpt_interval=0, log_interval=0, **SCHEDULE)
    assert run.accumulate == 1
    run.run(_batches(4), 1)
    assert opt.engine.calls == [("train_step", R.step_lr(0.01, 0, i, (90, 130), 0.1, "linear", 4, 0.1)) for i in range(4)] and run.iter == 4


def _train_network(monkeypatch, accumulate, n=7):
    opt = _Optimizer()
    monkeypatch.setattr(R, "build_optimizer", lambda model, cfg, dtype=None: opt)
    monkeypatch.setattr(R, "DevicePrefetcher", lambda loader: loader)
    ocfg = dict(grad_clip=dict(max_norm=40, norm_type=2))
    if accumulate is not None:
        ocfg["accumulate"] = accumulate
    cfg = R.Config(optimizer=dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True), optimizer_config=ocfg,
                   lr_config=dict(policy="step", step=[90, 130], warmup="linear", warmup_iters=4, warmup_ratio=0.1),
                   checkpoint_config=dict(interval=0), log_config=dict(interval=0), total_epochs=1, work_dir=None,
                   data=dict(videos_per_gpu=1, workers_per_gpu=0), resume_from=None, load_from=None)
    return R.train_network(_Model(), _batches(n), cfg, logger=lambda s: None), opt


def test_train_network_reads_optimizer_config_accumulate(monkeypatch):
    run, opt = _train_network(monkeypatch, 3)
    assert run.accumulate == 3 and run.iter == 3 and opt.engine.calls == _expected([3, 3, 1])
    run, opt = _train_network(monkeypatch, None)                      # the default: 1 = train_step only
    assert run.accumulate == 1 and run.iter == 7 and [c[0] for c in opt.engine.calls] == ["train_step"] * 7


@pytest.mark.parametrize("bad", [0, -1, 2.5, "3", None, True])
def test_accumulate_must_be_an_integer_of_at_least_one(monkeypatch, bad):
    with pytest.raises(ValueError, match="accumulate"):
        R.Runner(_Model(), optimizer=_Optimizer(), accumulate=bad)
    built = []
    monkeypatch.setattr(R, "build_optimizer", lambda *a, **kw: built.append(1))
    cfg = R.Config(optimizer=dict(type="SGD", lr=0.01), optimizer_config=dict(accumulate=bad), total_epochs=1)
    with pytest.raises(ValueError, match="accumulate"):
        R.train_network(_Model(), _batches(2), cfg)
    assert not built                                                  # refused before anything is built


def test_the_accumulate_export_is_declared():
    from mvfnet_amd import _lib
    assert "mvf_grad_accumulate" in _lib.declared_symbols()
    fn = _lib.lib.mvf_grad_accumulate
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    assert fn(None, None, 0, 1, None) == 0                            # n = 0: no launch, no GPU needed
    assert fn(None, None, 3, 1, None) != 0 and b"NULL" in _lib.lib.mvf_last_error()
    assert fn(None, None, -1, 0, None) != 0 and b"negative" in _lib.lib.mvf_last_error()


def test_engine_surface_of_the_accumulation_exists():
    from mvfnet_amd.train_engine import TrainEngine
    for name in ("accumulate_step", "apply_accumulated", "train_step_accumulated", "acc_grad_of", "accumulated_loss"):
        assert hasattr(TrainEngine, name)
    # a public scalar class attribute would become a launch-plan key switch: the count must not be one (micro-steps share train_step's plans)
    assert "accumulated_count" not in vars(TrainEngine) and TrainEngine.flat_acc is None
