"""[r6] Launch plans (mvfnet_amd/launch_plan.py + mvf_plan_run, csrc/launch_plan.hip): a train step replayed from a recorded launch table must be the eager
step -- same kernels, same arguments, same stream order -- so losses and parameters agree BIT FOR BIT over a run that starts eager, records twice and then replays.
Reference: one iteration of batch_processor + DistOptimizerHook.after_train_iter (codes/core/train.py:45-60, codes/core/dist_utils.py:61-67)."""
import ctypes as C
import os

import pytest
import torch

from mvfnet_amd import synth

pytestmark = pytest.mark.gpu


def _engine(dtype, use_plan, t=4, dropout=0.5, depth=50, share=False):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(depth, t, dropout_ratio=dropout)
    if share:
        cfg["module_cfg"]["share"] = True                    # one tap weight serves the three views (reference MVF.py:114-116)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r%d/" % depth + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r%d/" % depth + k]) for k in sd})
    eng = m.cuda().train().train_engine(dtype=dtype)
    eng.use_plan = use_plan
    return m, eng


def _run(dtype, use_plan, steps, batches, lrs, seed=7, **kw):
    torch.manual_seed(seed)                                  # the dropout masks
    m, eng = _engine(dtype, use_plan, **kw)
    losses = []
    for i in range(steps):
        imgs, labels = batches[i % len(batches)]
        losses.append(eng.train_step(imgs.clone(), labels.clone(), lr=lrs[i % len(lrs)]).clone())      # fresh tensors: the plan patches their addresses
    torch.cuda.synchronize()
    return eng, torch.cat(losses), eng.flat_params.clone(), [b.clone() for b in m.buffers()]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_replayed_steps_equal_eager_steps_bit_for_bit(dtype):
    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen)) for _ in range(3)]
    lrs = [0.015, 0.01, 0.02, 0.005]
    steps = 9
    eng_p, loss_p, par_p, buf_p = _run(dtype, True, steps, batches, lrs)
    eng_e, loss_e, par_e, buf_e = _run(dtype, False, steps, batches, lrs)
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["eager"] == eng_p.plan_warmup and st[0]["tries"] == 2, "no plan was accepted: %r" % [(s_["eager"], s_["tries"]) for s_ in st]
    plan = st[0]["plan"]
    assert plan.n_ops > 300 and all(len(v) >= 1 for k, v in plan.slots.items() if k != "mask" or eng_p.dropout > 0), (plan.n_ops, {k: len(v) for k, v in plan.slots.items()})
    assert not getattr(eng_e, "_plans", None)
    assert torch.equal(loss_p, loss_e), (loss_p, loss_e)
    assert torch.equal(par_p, par_e)
    for a, b in zip(buf_p, buf_e):
        assert torch.equal(a, b)
    print("launch plan %s: %d ops in %d segment(s), slots %s; %d replayed steps bit-identical to eager" %
          (dtype, plan.n_ops, len(plan.cuts), {k: len(v) for k, v in plan.slots.items()}, steps - eng_p.plan_warmup - 2))


def test_a_new_batch_shape_gets_its_own_plan_and_frozen_statistics_stay_eager():
    gen = torch.Generator(device="cuda").manual_seed(5)
    m, eng = _engine(torch.bfloat16, True, dropout=0.0)
    a = (torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen))
    b = (torch.randn(1, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (1, 1), device="cuda", generator=gen))      # the partial last batch of an epoch
    for _ in range(5):
        eng.train_step(*a)
    for _ in range(5):
        eng.train_step(*b)
    eng.train_step(*a)
    torch.cuda.synchronize()
    assert len(eng._plans) == 2 and all(s["plan"] is not None for s in eng._plans.values())
    m.backbone.bn1.eval()                                    # a BatchNorm on its running statistics: folded by torch calls every step -> no plan
    n = len(eng._plans)
    eng.train_step(*a)
    assert len(eng._plans) == n and torch.isfinite(eng.flat_params).all()


def test_a_larger_batch_replaces_storage_and_the_smaller_batchs_plan_is_recorded_again():
    """A plan holds raw pointers into the engine's persistent buffers.  When a LARGER batch arrives, TrainEngine.buf() / workspace() replace those allocations
    (one allocation per call site, sized for the largest shape seen): the plan recorded for the smaller batch must not be replayed on the freed storage.  The
    sequence small x 6 (plan accepted) -> large x 6 -> small x 6 must equal the same sequence without plans bit for bit, and the small shape must have been
    recorded a second time (reference: drop_last=False loaders and a val pass between epochs hand the runner batches of different sizes, codes/core/train.py:45-60)."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    small = (torch.randn(1, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (1, 1), device="cuda", generator=gen))
    large = (torch.randn(3, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (3, 1), device="cuda", generator=gen))
    seq = [small] * 6 + [large] * 6 + [small] * 6
    out = {}
    for use_plan in (True, False):
        torch.manual_seed(9)
        m, eng = _engine(torch.bfloat16, use_plan)
        losses, epochs, replays = [], [], 0
        for imgs, labels in seq:
            mine = lambda: [v["plan"] for k, v in getattr(eng, "_plans", {}).items() if k[0] == tuple(imgs.shape)]  # noqa: E731
            before = mine()
            losses.append(eng.train_step(imgs.clone(), labels.clone()).clone())
            epochs.append(eng._storage_epoch)
            replays += bool(before) and before[0] is not None and mine()[0] is before[0]          # this shape's plan existed and survived the step: it was replayed
        torch.cuda.synchronize()
        out[use_plan] = (torch.cat(losses), eng.flat_params.clone(), epochs, eng, replays)
    loss_p, par_p, epochs, eng_p, replays = out[True]
    assert epochs[5] == epochs[0] and epochs[6] > epochs[5] and epochs[-1] == epochs[11], epochs      # only the first large step replaced storage
    st = list(eng_p._plans.values())
    assert len(st) == 2 and all(s_["plan"] is not None and s_["plan"].storage_epoch == eng_p._storage_epoch for s_ in st), [(s_["eager"], s_["tries"]) for s_ in st]
    assert replays == 8, replays                             # steps 5-6, 11-12 and 15-18 ran from plans; step 13 dropped the stale one
    assert torch.equal(loss_p, out[False][0]), (loss_p, out[False][0])
    assert torch.equal(par_p, out[False][1])


def test_plan_with_the_gradient_exchange_cut_in_two_segments(tmp_path):
    """With a process group the tail bucket's all-reduce is issued in the middle of backward: the plan has two segments around that torch call."""
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group is already up in this process")
    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "pg"), rank=0, world_size=1)
    try:
        gen = torch.Generator(device="cuda").manual_seed(9)
        batch = (torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen))
        out = {}
        for use_plan in (True, False):
            torch.manual_seed(1)
            m, eng = _engine(torch.bfloat16, use_plan)
            eng.force_allreduce = True
            losses = [eng.train_step(batch[0].clone(), batch[1].clone()).clone() for _ in range(9)]
            torch.cuda.synchronize()
            out[use_plan] = (torch.cat(losses), eng.flat_params.clone(), eng)
        plans = [s["plan"] for s in out[True][2]._plans.values()]
        assert len(plans) == 1 and plans[0] is not None and len(plans[0].cuts) == 2 and len(plans[0].py_ops) == 1
        assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    finally:
        dist.destroy_process_group()


def test_plan_run_reports_the_failing_op():
    from mvfnet_amd import _lib as L
    lib = L.lib
    ops = (L.PlanOp * 2)()
    d = L.MvfDesc(10, 16, 4, 4, 4, 4, 7, 0, 0)                # nt = 10 is not a multiple of n_segment = 4: mvf_fwd_infer refuses it
    words = (C.c_ulonglong * 16)(C.addressof(d), 0, 0, 0, 0, 0, 0, 0, 0)
    floats = (C.c_float * 1)()
    ops[0].kind, ops[0].n_int, ops[0].fn, ops[0].word0 = 0, 9, C.cast(lib.mvf_fwd_infer, C.c_void_p).value, 0
    ops[1].kind = 7
    failed = C.c_int(-5)
    assert lib.mvf_plan_run(ops, 2, words, floats, C.byref(failed)) == -2 and failed.value == 0 and b"n_segment" in lib.mvf_last_error()
    assert lib.mvf_plan_run(C.cast(C.byref(ops, C.sizeof(L.PlanOp)), C.POINTER(L.PlanOp)), 1, words, floats, C.byref(failed)) == -1 and failed.value == 0
    assert lib.mvf_plan_run(ops, 0, words, floats, C.byref(failed)) == 0 and failed.value == -1


# ------------------------------------------------------------------------------------------------ the recording belongs to ONE engine
def _clip_batch(seed, b=2):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(b, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (b, 1), device="cuda", generator=gen)


def _record_as_the_engine_does(eng, imgs, labels, between=None):
    """TrainEngine._record_step's recorded region and Plan, with `between` run between the engine's forward and its backward."""
    from mvfnet_amd import launch_plan
    prepared = eng._step_tensors(imgs, labels)
    with launch_plan.recording(eng) as rec:
        loss = eng.forward(imgs, labels, _prepared=prepared)
        if between is not None:
            between()
        eng.backward(exchange=True)
    assert rec.unsupported is None, rec.unsupported
    lab, mask, _ = prepared
    return launch_plan.Plan(rec, dict(imgs=imgs.data_ptr(), labels=lab.data_ptr(), mask=mask.data_ptr() if mask is not None else 0, loss=loss.data_ptr()))


def test_a_recording_sees_only_its_own_engines_calls():
    """launch_plan.recording(A) shadows A's library handle and nobody else's: a second engine that trains inside the block -- between A's forward and A's backward
    too -- leaves nothing in A's recording and launches on the real library."""
    from mvfnet_amd import _lib, launch_plan
    _, eng_a = _engine(torch.bfloat16, False, dropout=0.0)
    _, eng_b = _engine(torch.bfloat16, False, dropout=0.0)
    imgs, labels = _clip_batch(21)
    for eng in (eng_a, eng_b):
        for _ in range(2):                                   # buffers and workspaces reach their final sizes
            eng.train_step(imgs.clone(), labels.clone())
    with launch_plan.recording(eng_a) as rec:
        assert isinstance(eng_a.lib, launch_plan.RecordingLib) and eng_a._rec is rec
        eng_b.train_step(imgs.clone(), labels.clone())
        assert eng_b.lib is _lib.lib and eng_b._rec is None
    assert rec.ops == []
    assert "lib" not in vars(eng_a) and eng_a.lib is _lib.lib and eng_a._rec is None
    alone = _record_as_the_engine_does(eng_a, imgs.clone(), labels.clone())
    eng_a.step()
    shared = _record_as_the_engine_does(eng_a, imgs.clone(), labels.clone(), between=lambda: eng_b.train_step(imgs.clone(), labels.clone()))
    eng_a.step()
    torch.cuda.synchronize()
    assert alone.n_ops > 300 and alone.names == shared.names and alone.signature == shared.signature
    assert "lib" not in vars(eng_a) and "lib" not in vars(eng_b)


def test_an_exception_inside_a_recording_leaves_the_engine_as_it_was():
    from mvfnet_amd import _lib, launch_plan
    _, eng = _engine(torch.float32, False, dropout=0.0)
    _, fresh = _engine(torch.float32, False, dropout=0.0)
    imgs, labels = _clip_batch(22)

    def failing_backward(exchange=False):
        raise RuntimeError("stubbed backward")
    eng.backward = failing_backward
    with pytest.raises(RuntimeError, match="stubbed backward"):
        with launch_plan.recording(eng) as rec:
            eng.forward(imgs, labels)
            eng.backward(exchange=True)
    del eng.backward
    assert len(rec.ops) > 100                                # the forward was recorded up to the failure
    assert "lib" not in vars(eng) and eng.lib is _lib.lib and "_rec" not in vars(eng) and eng._rec is None
    # the twin makes the same forward, eagerly and without a failure: same parameters (no update was made), same running means (the conv epilogues shift their
    # statistics sums by them), so the next step's loss can be compared bit for bit
    fresh.forward(imgs, labels)
    loss = eng.train_step(imgs, labels)
    want = fresh.train_step(imgs, labels)
    torch.cuda.synchronize()
    assert torch.equal(loss, want), (loss, want)
    assert torch.equal(eng.flat_grads, fresh.flat_grads)
    assert "lib" not in vars(eng)


# ------------------------------------------------------------------------------------------------ share=True: the tap gradients are summed by torch calls
def test_a_shared_mvf_weight_keeps_every_step_eager():
    """With share=True the three views' tap gradients are added by in-place torch calls inside backward (_TMvf.backward), which a plan would not replay: such a
    model never gets a plan, so nine steps with use_plan on are the nine eager steps bit for bit."""
    batches = [_clip_batch(31 + i) for i in range(3)]
    eng_p, loss_p, par_p, buf_p = _run(torch.bfloat16, True, 9, batches, [0.015, 0.01], share=True)
    eng_e, loss_e, par_e, buf_e = _run(torch.bfloat16, False, 9, batches, [0.015, 0.01], share=True)
    assert any(blk.mvf is not None and blk.mvf.share for blk in eng_p.blocks)
    assert all(s_["plan"] is None for s_ in getattr(eng_p, "_plans", {}).values()) and not getattr(eng_e, "_plans", None)
    assert torch.isfinite(loss_p).all() and torch.equal(loss_p, loss_e), (loss_p, loss_e)
    assert torch.equal(par_p, par_e)
    for a, b in zip(buf_p, buf_e):
        assert torch.equal(a, b)


def test_a_shared_mvf_weights_gradient_is_the_sum_of_the_three_views():
    """One fp32 step of a share=True model: the gradient the engine leaves for layer3.0's shared shift_conv.weight equals the sum of the three views' gradients the
    torch MVF module (modules/MVF.py, its own autograd path) computes with the same weight in each view, on the same block input and the same gradient of the MVF
    output.  Tolerance: TOL_GRAD, what tests/test_mvf_gpu.py grants the module's parameter gradients (the tap weights among them)."""
    import torch.nn as nn
    from helpers import rel_err
    from mvfnet_amd.modules import MVF
    from test_mvf_gpu import TOL_GRAD
    m, eng = _engine(torch.float32, True, dropout=0.0, share=True)
    blk = next(b_ for b_ in eng.blocks if b_.mvf is not None)
    mod = next(m_ for m_ in m.modules() if isinstance(m_, MVF))          # the same block: the first one in module order
    tm = blk.mvf
    assert tm.share and tm.wt is mod.shift_conv.weight and not hasattr(mod, "h_conv")
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    seen = {}
    orig = tm.backward

    def keeping_operands(dxp, x, y, nt, h, w, c, *a, **k):
        seen.update(x=x.clone(), dy=dxp[:, :tm.cs].clone(), nt=nt, h=h, w=w, c=c)          # dxp's slice: the gradient of the MVF output, before the stencil replaces it
        return orig(dxp, x, y, nt, h, w, c, *a, **k)
    tm.backward = keeping_operands
    imgs, labels = _clip_batch(41)
    eng.train_step(imgs, labels)
    del tm.backward
    torch.cuda.synchronize()
    assert not getattr(eng, "_plans", None)
    nt, h, w, c, cs = seen["nt"], seen["h"], seen["w"], seen["c"], tm.cs
    ref = MVF(nn.Identity(), tm.T, c, cs / float(c), use_hs=True, share=False, mode=mod.mode).cuda().train()
    assert ref.num_shift_channel == cs
    with torch.no_grad():
        for view in (ref.shift_conv, ref.h_conv, ref.w_conv):
            view.weight.copy_(before["shift_conv.weight"].reshape(view.weight.shape))
        ref.bn.weight.copy_(before["bn.weight"])
        ref.bn.bias.copy_(before["bn.bias"])
    x = seen["x"].float().view(nt, h, w, c).permute(0, 3, 1, 2).contiguous()
    y = ref(x)
    dy = torch.zeros_like(y)
    dy[:, :cs] = seen["dy"].float().view(nt, h, w, cs).permute(0, 3, 1, 2)
    y.backward(dy)
    want = sum(view.weight.grad.reshape(cs, 3) for view in (ref.shift_conv, ref.h_conv, ref.w_conv))
    t_only = ref.shift_conv.weight.grad.reshape(cs, 3)
    got = eng.grad_of(mod.shift_conv.weight).reshape(cs, 3)
    err = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print("shared tap gradient vs the three views' sum: rel err %.2e (the T view alone: %.2e)" % (err, rel_err(t_only.cpu().numpy(), want.cpu().numpy())))
    assert err < TOL_GRAD, err
    assert rel_err(t_only.cpu().numpy(), want.cpu().numpy()) > 100 * TOL_GRAD          # the H and W views do contribute: the sum is what is checked
