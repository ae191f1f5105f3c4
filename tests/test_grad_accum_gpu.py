"""GPU: gradient accumulation -- mvf_grad_accumulate (csrc/grad_accum.hip) and TrainEngine.accumulate_step / apply_accumulated: one optimizer step over k
micro-batches, each under its own BatchNorm batch statistics, is the reference's data-parallel step with the ranks run one after another (8 GPUs x 12 clips,
configs/MVFNet/K400/mvf_kinetics400_2d_rgb_r50_dense.py:121-123; per-GPU BatchNorm, gradient mean by DistOptimizerHook, codes/core/dist_utils.py:15-67).

A note on "bit for bit": the engine's BatchNorm statistics are accumulated around a shift (the running mean of the moment), so the LAST BITS of a training-mode
gradient depend on the running statistics although its value does not.  Where two passes over the same micro-batches are compared exactly, the BatchNorm
buffers are rewound in between, so that both passes see the same running statistics."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mvfnet_amd import synth

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _values(n, seed):
    """fp32 test values: normal numbers of both signs, zeros, denormals, and tiny normals whose sums and differences fall into the denormal range."""
    rng = np.random.RandomState(seed)
    v = rng.standard_normal(n).astype(np.float32)
    kind = rng.randint(0, 8, n)
    v[kind == 0] = 0.0
    v[kind == 1] = (rng.standard_normal(int((kind == 1).sum())) * 1e-40).astype(np.float32)        # denormals
    v[kind == 2] = (rng.choice([-1.0, 1.0], int((kind == 2).sum())) * 1.5e-38).astype(np.float32)   # +-1.5e-38: sums cancel to 0 or differ by denormals
    v[kind == 3] *= np.float32(1e-38)
    return v


def _launch(lib, acc, g, a_off, g_off, n, first):
    return lib.mvf_grad_accumulate(acc.data_ptr() + 4 * a_off, g.data_ptr() + 4 * g_off, n, first, None)


def _check_case(lib, n, a_off, g_off):
    """Both modes on views that start a_off / g_off elements into larger buffers; the guard elements around the views must keep their values."""
    pad = 8
    acc0, g0 = _values(n, 1000 + n), _values(n, 2000 + n)
    host_a = np.full(a_off + n + pad, 7.25, np.float32)
    host_g = np.full(g_off + n + pad, -3.5, np.float32)
    host_a[a_off:a_off + n], host_g[g_off:g_off + n] = acc0, g0
    want_sum = acc0 + g0                               # numpy float32: one correctly rounded add per element
    for first, want in ((1, g0), (0, want_sum)):
        runs = []
        for _ in range(2):                             # run to run: identical
            acc, g = torch.from_numpy(host_a).cuda(), torch.from_numpy(host_g).cuda()
            assert _launch(lib, acc, g, a_off, g_off, n, first) == 0, lib.mvf_last_error()
            torch.cuda.synchronize()
            runs.append((acc.cpu().numpy(), g.cpu().numpy()))
        (out_a, out_g), (out_a2, _) = runs
        what = "n=%d offsets (%d, %d) first=%d" % (n, a_off, g_off, first)
        assert np.array_equal(out_a[a_off:a_off + n].view(np.uint32), want.view(np.uint32)), what
        assert np.array_equal(out_a[:a_off], host_a[:a_off]) and np.array_equal(out_a[a_off + n:], host_a[a_off + n:]), "guards of acc, " + what
        assert np.array_equal(out_g.view(np.uint32), host_g.view(np.uint32)), "g was written, " + what
        assert np.array_equal(out_a.view(np.uint32), out_a2.view(np.uint32)), "two runs differ, " + what


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1024, 1025, 65543])
def test_accumulate_kernel_is_the_fp32_add_bit_for_bit_at_every_offset(n):
    from mvfnet_amd import _lib
    # the allocations are 256-byte aligned: an offset of 4 + o elements puts the view o elements past a 16-byte boundary.  Equal offsets (the engine's
    # flat_*[off:] views) and unequal ones (g's loads then take the scalar form)
    for a_off in (4, 5, 6, 7):
        for g_off in (4, 5, 6, 7):
            _check_case(_lib.lib, n, a_off, g_off)


def test_accumulate_kernel_beyond_one_sweep_of_the_grid():
    """More 16-byte vectors than 2 x (grid cap x 256 threads): the two-vectors-in-flight loop, its one-vector remainder and the scalar ends in one launch."""
    from mvfnet_amd import _lib
    n = 4 * (2 * 2048 * 256 + 300) + 3
    for a_off, g_off in ((4, 4), (5, 5), (5, 6)):
        _check_case(_lib.lib, n, a_off, g_off)


def test_accumulate_kernel_argument_checks():
    from mvfnet_amd import _lib
    lib = _lib.lib
    assert lib.mvf_grad_accumulate.restype is C.c_int
    assert lib.mvf_grad_accumulate(None, None, 0, 1, None) == 0                  # n = 0: nothing to do, nothing launched
    buf = torch.full((16,), 2.0, device="cuda")
    assert lib.mvf_grad_accumulate(buf.data_ptr(), buf.data_ptr() + 32, 0, 0, None) == 0
    for acc, g in ((None, buf.data_ptr()), (buf.data_ptr(), None), (None, None)):
        assert lib.mvf_grad_accumulate(acc, g, 4, 1, None) != 0 and b"NULL" in lib.mvf_last_error()
    assert lib.mvf_grad_accumulate(buf.data_ptr(), buf.data_ptr() + 32, -1, 1, None) != 0 and b"negative" in lib.mvf_last_error()
    assert lib.mvf_grad_accumulate(buf.data_ptr(), buf.data_ptr() + 16, 8, 0, None) != 0 and b"overlap" in lib.mvf_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 2.0).all())


# ------------------------------------------------------------------------------------------------ engines
LR_FROZEN = dict(lr=0.0, momentum=0.0, weight_decay=0.0, max_norm=None)      # the weights do not move: gradients of several passes are comparable


def _model(dropout=0.0):
    import mvfnet_amd
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=dropout), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().train()


def _batch(seed, clips=2):
    return (torch.from_numpy(synth.synth_clip_batch(clips, 4, 64, 64, seed=seed)).cuda(), torch.from_numpy(synth.synth_labels(clips, seed=seed)).cuda())


def _snapshot(m):
    return [b.detach().clone() for b in m.buffers()]


def _rewind(m, snap):
    with torch.no_grad():
        for b, s in zip(m.buffers(), snap):
            b.copy_(s)


def _micro_gradients(m, eng, batches):
    """g_i of every micro-batch from forward + backward(exchange=False), then the BatchNorm buffers rewound to where they were."""
    snap = _snapshot(m)
    out = []
    for imgs, labels in batches:
        eng.forward(imgs, labels)
        eng.backward(exchange=False)
        out.append(eng.flat_grads.cpu().numpy().copy())
    _rewind(m, snap)
    return out


def _accumulation_run(dtype):
    """Three micro-batches of 2 clips on an engine whose weights do not move: their gradients one by one, and the accumulator after 2 and after 3 micro-steps."""
    m = _model()
    eng = m.train_engine(dtype=dtype, **LR_FROZEN)
    batches = [_batch(10), _batch(11), _batch(12)]
    g = _micro_gradients(m, eng, batches)
    assert eng.flat_acc is None and eng.accumulated_count == 0          # nothing is allocated before the first accumulate_step
    accs, losses = [], []
    for imgs, labels in batches:
        losses.append(eng.accumulate_step(imgs, labels).clone())
        accs.append(eng.flat_acc.cpu().numpy().copy())
    names = [k for k, _ in m.named_parameters()]
    index = np.concatenate([np.arange(eng.grad_of(p).numel()) + eng.grad_of(p).storage_offset() for _, p in m.named_parameters()])
    view_ok = all(torch.equal(eng.acc_grad_of(p), eng.flat_acc[eng.grad_of(p).storage_offset():][:p.numel()].view(p.shape)) for p in m.parameters())
    mean_loss = eng.accumulated_loss.clone()
    count = eng.accumulated_count
    eng.apply_accumulated()
    torch.cuda.synchronize()
    return dict(g=g, accs=accs, names=names, index=index, view_ok=view_ok, losses=torch.cat(losses).cpu().numpy(), mean_loss=float(mean_loss), count=count,
                count_after=eng.accumulated_count, loss_after=float(eng.accumulated_loss))


_RUNS = {}


def _run_of(dtype):
    if dtype not in _RUNS:
        _RUNS[dtype] = _accumulation_run(dtype)
    return _RUNS[dtype]


# ------------------------------------------------------------------------------------------------ 2. acc = ((g_0 + g_1) + g_2)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_accumulator_is_the_ordered_fp32_sum_of_the_micro_batch_gradients(dtype):
    r = _run_of(dtype)
    g0, g1, g2 = r["g"]
    assert np.abs(g0).max() > 0 and not np.array_equal(g0, g1) and not np.array_equal(g1, g2)
    assert np.array_equal(r["accs"][0], g0)                            # first micro-step: a copy, whatever the accumulator held
    assert np.array_equal(r["accs"][1], g0 + g1)
    assert np.array_equal(r["accs"][2], (g0 + g1) + g2)                # arrival order
    assert r["view_ok"] and r["count"] == 3 and r["count_after"] == 0


# ------------------------------------------------------------------------------------------------ 7. the loss
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_accumulated_loss_is_the_mean_of_the_micro_batch_losses(dtype):
    r = _run_of(dtype)
    want = float(r["losses"].astype(np.float32).mean(dtype=np.float32))
    assert len(set(r["losses"].tolist())) == 3
    assert abs(r["mean_loss"] - want) <= 1e-6 * abs(want), (r["mean_loss"], want)
    assert abs(r["loss_after"] - want) <= 1e-6 * abs(want)             # after the boundary it still reports the group that was applied


# ------------------------------------------------------------------------------------------------ 3. against the oracle
def test_accumulated_gradient_against_the_cpu_oracles_per_micro_batch_gradients():
    """acc of two micro-batches against the sum of the CPU oracle's per-micro-batch gradients (each under ITS OWN batch statistics).  The bound is the triangle
    inequality over the engine-vs-oracle distances of the single micro-batches, measured here: ||acc - sum_r o_r|| <= sum_r ||g_r - o_r|| (1 + 1e-6).  And the
    comparison can fail: acc / 2 is >= 10x further from either single micro-batch's oracle gradient than from the oracle mean."""
    import mvfnet_amd
    from oracle import net_torch
    r = _run_of(torch.float32)
    idx, names = r["index"], r["names"]
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips=None))
    sd0 = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd0.items()})
    torch.set_num_threads(min(16, torch.get_num_threads()))
    oracle = []
    for s in (10, 11):
        sd = {k: torch.from_numpy(vals["r50/" + k]).clone() for k in sd0}
        leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
        imgs, labels = torch.from_numpy(synth.synth_clip_batch(2, 4, 64, 64, seed=s)), torch.from_numpy(synth.synth_labels(2, seed=s))
        net_torch.forward_train(imgs, labels, sd, 50).backward()
        oracle.append(np.concatenate([leaves[k].grad.numpy().ravel() for k in names]).astype(np.float64))
    g = [r["g"][i][idx].astype(np.float64) for i in range(2)]
    acc = r["accs"][1][idx].astype(np.float64)
    norm = lambda v: float(np.sqrt((v * v).sum()))          # noqa: E731
    d_local = [norm(g[i] - oracle[i]) for i in range(2)]
    d_acc = norm(acc - (oracle[0] + oracle[1]))
    d_mean = norm(acc / 2 - (oracle[0] + oracle[1]) / 2)
    d_wrong = [norm(acc / 2 - oracle[i]) for i in range(2)]
    print("accumulation vs oracle: ||g_r - o_r|| = %.4e / %.4e (relative %.2e / %.2e); ||acc - sum o|| = %.4e (bound %.4e); acc/2 vs oracle mean %.4e, vs a single "
          "micro-batch's %.4e / %.4e" % (d_local[0], d_local[1], d_local[0] / norm(oracle[0]), d_local[1] / norm(oracle[1]), d_acc, sum(d_local), d_mean,
                                         d_wrong[0], d_wrong[1]))
    assert d_acc <= sum(d_local) * (1 + 1e-6), (d_acc, d_local)
    assert min(d_wrong) >= 10 * d_mean, (d_wrong, d_mean)


# ------------------------------------------------------------------------------------------------ 4. the update
def test_apply_accumulated_is_clip_plus_nesterov_sgd_on_the_mean_gradient():
    """k = 2, lr > 0: parameters and momentum buffers after apply_accumulated against torch's clip_grad_norm_ + SGD(nesterov) on (g_0 + g_1) / 2 -- the bounds of
    the fused optimizer's own test (test_train_gpu.py: norm 1e-5 relative, parameters 1e-6 of their largest magnitude)."""
    from helpers import rel_err
    m = _model()
    eng = m.train_engine(dtype=torch.float32, lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=40.0)
    assert eng.nesterov
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        eng.apply_accumulated()
    batches = [_batch(10), _batch(11)]
    g0, g1 = _micro_gradients(m, eng, batches)
    p0 = eng.flat_params.cpu().clone()
    for imgs, labels in batches:
        eng.accumulate_step(imgs, labels)
    assert eng.accumulated_count == 2 and eng.steps == 0
    acc = eng.flat_acc.cpu().numpy().copy()
    norm_out = eng.apply_accumulated()
    torch.cuda.synchronize()
    assert np.array_equal(acc, g0 + g1)                          # what the optimizer ran on IS the sum of the two gradients taken above
    # The torch step runs in float64 on the fp32 mean gradient: the reference must be more exact than the 1e-5 it is compared at, and an fp32 norm of ONE flat
    # 24 M-element tensor is not (a serial fp32 sum of squares loses the many small terms behind a few large ones; torch's own use is one tensor per
    # parameter).  The fp32 figure is printed beside it.
    mean = torch.from_numpy((g0 + g1) / np.float32(2.0))
    p = torch.nn.Parameter(p0.double())
    p.grad = mean.double()
    total32 = float(torch.linalg.vector_norm(mean))
    total = float(torch.nn.utils.clip_grad_norm_([p], 40.0, norm_type=2))
    opt = torch.optim.SGD([p], lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    opt.step()
    print("apply_accumulated: norm %.6f (torch float64 %.6f; torch float32 on the flat tensor %.6f), clip coefficient %.6f (float64 %.6f)"
          % (float(norm_out[0]), total, total32, float(norm_out[1]), 40.0 / (total + 1e-6)))
    assert abs(float(norm_out[0]) - total) < 1e-5 * total
    assert not torch.equal(eng.flat_params.cpu(), p0)
    assert rel_err(eng.flat_params.cpu().numpy(), p.detach().numpy()) < 1e-6
    assert rel_err(eng.flat_mom.cpu().numpy(), opt.state[p]["momentum_buffer"].numpy()) < 1e-6
    assert eng.accumulated_count == 0 and eng.steps == 1
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        eng.apply_accumulated()


# ------------------------------------------------------------------------------------------------ 5. k = 1 is train_step
def test_one_micro_batch_per_step_gives_train_steps_parameters_bit_for_bit():
    batches = [_batch(20 + i) for i in range(3)]
    lrs = [0.015, 0.01, 0.02]
    out = {}
    for mode in ("train_step", "accumulate"):
        torch.manual_seed(5)                                    # the dropout masks
        m = _model(dropout=0.5)
        eng = m.train_engine(dtype=torch.bfloat16)
        params, losses = [], []
        for (imgs, labels), lr in zip(batches, lrs):
            if mode == "train_step":
                losses.append(eng.train_step(imgs.clone(), labels.clone(), lr=lr).clone())
            else:
                losses.append(eng.accumulate_step(imgs.clone(), labels.clone()).clone())
                eng.apply_accumulated(lr=lr)
            params.append(eng.flat_params.clone())
        torch.cuda.synchronize()
        out[mode] = (params, torch.cat(losses), eng.steps, [b.clone() for b in m.buffers()])
    assert out["train_step"][2] == out["accumulate"][2] == 3
    assert torch.equal(out["train_step"][1], out["accumulate"][1])
    for i in range(3):
        assert torch.equal(out["train_step"][0][i], out["accumulate"][0][i]), "parameters differ after step %d" % (i + 1)
    assert not torch.equal(out["train_step"][0][0], out["train_step"][0][2])
    for a, b in zip(out["train_step"][3], out["accumulate"][3]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. launch plans
def test_micro_steps_replay_train_steps_plans_and_equal_the_eager_micro_steps():
    """k = 3, three optimizer steps = nine micro-steps: two eager, two recorded, five replayed from the plan train_step would use (same key)."""
    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen)) for _ in range(3)]
    out = {}
    for use_plan in (True, False):
        m = _model()
        eng = m.train_engine(dtype=torch.bfloat16)
        if not use_plan:
            eng.use_plan = False                                # (the first engine runs the default policy)
        replays = [0]
        for step in range(3):
            if step == 2 and use_plan:                          # count what the third optimizer step replays
                plan = list(eng._plans.values())[0]["plan"]
                assert plan is not None
                run = plan.run
                plan.run = lambda *a, **kw: (replays.__setitem__(0, replays[0] + 1), run(*a, **kw))[1]
            loss = eng.train_step_accumulated([(i.clone(), l.clone()) for i, l in batches], lr=0.01)      # fresh tensors: the plan patches their addresses
        torch.cuda.synchronize()
        out[use_plan] = (eng.flat_params.clone(), loss.clone(), eng, replays[0])
    eng_p, eng_e = out[True][2], out[False][2]
    assert eng_p.use_plan is True
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["eager"] == eng_p.plan_warmup and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    assert out[True][3] == 3                                    # every micro-step of the third optimizer step ran from the plan
    assert not getattr(eng_e, "_plans", None)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert eng_p.steps == eng_e.steps == 3
    eng_p.train_step(batches[0][0].clone(), batches[0][1].clone())      # train_step's key is the micro-steps' key: no second plan
    torch.cuda.synchronize()
    assert len(eng_p._plans) == 1 and list(eng_p._plans.values())[0]["tries"] == 2


# ------------------------------------------------------------------------------------------------ 8. two ranks x two micro-batches
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_accumulate(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)                                    # gloo carrying the CUDA tensors: both ranks on one device
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _model()
    eng = m.train_engine(dtype=torch.float32, **LR_FROZEN)
    assert eng._ddp_active()
    local, tails = [], []
    for i in range(2):
        imgs, labels = _batch(10 + 2 * rank + i)               # four different micro-batches over the two ranks
        eng.accumulate_step(imgs, labels)
        tails.append(bool(eng._tail_launched))                  # no collective during a micro-step
        local.append(eng.flat_grads.clone())
    before = eng.flat_acc.clone()
    eng.apply_accumulated()
    torch.cuda.synchronize()
    mine = torch.stack(local)
    everyone = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(everyone, mine)
    total = (everyone[0][0] + everyone[0][1]) + (everyone[1][0] + everyone[1][1])
    bits = eng.flat_acc.view(torch.int32).to(torch.int64)
    chk = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=bits.device) % 8191 + 1)).sum()]).cpu()
    allc = [torch.zeros_like(chk) for _ in range(world)]
    dist.all_gather(allc, chk)
    info = dict(tails=tails, plans=len(eng.__dict__.get("_plans") or {}), local_sum_exact=bool(torch.equal(before, local[0] + local[1])),
                ranks_equal=bool(torch.equal(allc[0], allc[1])), exact=bool(torch.equal(eng.flat_acc, total)),
                rel=float((eng.flat_acc.double() - total.double()).norm() / total.double().norm()), norm=float(total.double().norm()),
                distinct=not torch.equal(everyone[0][0], everyone[1][0]), count=eng.accumulated_count, steps=eng.steps)
    torch.save(info, os.path.join(out_dir, "info_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_accumulate_locally_and_exchange_once_at_the_boundary(tmp_path):
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker_accumulate, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for r in range(2):
        i = torch.load(str(tmp_path / ("info_rank%d.pt" % r)), weights_only=False)
        print("rank %d: accumulator after the exchange vs the sum of the four local gradients: exact %s, relative %.2e (norm %.4e)" % (r, i["exact"], i["rel"], i["norm"]))
        assert i["tails"] == [False, False] and i["plans"] == 0           # no collective in a micro-step, and none replayed from a plan
        assert i["local_sum_exact"] and i["distinct"] and i["norm"] > 0
        assert i["ranks_equal"]                                            # both ranks hold the same accumulator
        assert i["exact"] or i["rel"] < 1e-6
        assert i["count"] == 0 and i["steps"] == 1
