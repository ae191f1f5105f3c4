"""GPU, world_size 2 on ONE MI355X (both ranks on cuda:0, gloo backend carrying the CUDA tensors): the TrainEngine's data-parallel
step itself -- flat gradient all-reduce / world folded into the optimizer kernel, two-bucket overlapped exchange -- with real
ranks holding different clips.  (RCCL refuses two ranks on one device; the collective semantics under test are torch.distributed's,
the same calls the nccl backend receives on a multi-GPU node.)  Reference: codes/core/dist_utils.py:15-67."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, overlap, backend="gloo"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import numpy as np
    import mvfnet_amd
    from mvfnet_amd import synth
    # gloo: both ranks on cuda:0 (a 1-GPU box); nccl (= RCCL, only when >= 2 devices are visible): one device per rank
    torch.cuda.set_device(rank if backend == "nccl" else 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    m = m.cuda().train()
    eng = m.train_engine(dtype=torch.bfloat16)
    eng.overlap_allreduce = overlap
    imgs = torch.from_numpy(synth.synth_clip_batch(2, 4, 64, 64, seed=10 + rank)).cuda()          # every rank its own clips
    labels = torch.from_numpy(synth.synth_labels(2, seed=10 + rank)).cuda()
    losses = [float(eng.train_step(imgs, labels)) for _ in range(3)]
    torch.cuda.synchronize()
    bits = eng.flat_params.view(torch.int32).to(torch.int64)
    chk = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=bits.device) % 8191 + 1)).sum()]).cpu()
    allc = [torch.zeros_like(chk) for _ in range(world)]
    dist.all_gather(allc, chk)
    g0 = eng.flat_grads[:1000].cpu().numpy().copy()
    q.put((rank, losses, [c.tolist() for c in allc], g0.tolist(), float(eng.norm_out[0])))
    dist.barrier()
    dist.destroy_process_group()


def _run(overlap, backend="gloo"):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, overlap, backend)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=280) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return out


@pytest.mark.timeout(600)
def test_two_rank_train_steps_keep_replicas_bit_identical_and_buckets_equal_flat():
    a = _run(True)           # tail bucket all-reduced during backward + head bucket after it
    b = _run(False)          # one flat all-reduce after backward
    for out in (a, b):
        (r0, l0, c0, g0, n0), (r1, l1, c1, g1, n1) = out
        assert c0[0] == c0[1] == c1[0] == c1[1]                   # both ranks hold the same parameter bits after 3 steps
        assert g0 == g1 and n0 == n1                              # ... because both applied the same summed gradient / clip norm
        assert l0 != l1                                           # different clips per rank: the losses differ
        assert all(x == x for x in l0 + l1)
    assert a[0][2][0] == b[0][2][0]                               # two-bucket overlapped exchange == single collective, bit for bit
    if torch.cuda.device_count() >= 2:
        # [r3] a multi-GPU node: the same two ranks over RCCL (one device each).  Replicas bit-identical, two buckets == one collective;
        # the summed gradient may differ from gloo's in the last bit (another reduction order), so no cross-backend bit comparison
        c = _run(True, "nccl")
        d = _run(False, "nccl")
        for out in (c, d):
            (r0, l0, c0, g0, n0), (r1, l1, c1, g1, n1) = out
            assert c0[0] == c0[1] == c1[0] == c1[1] and g0 == g1 and n0 == n1
        assert c[0][2][0] == d[0][2][0]
        assert [abs(x - y) < 1e-3 * abs(y) for x, y in zip(c[0][1], a[0][1])] == [True] * 3      # same losses as the gloo run, rank 0


# ------------------------------------------------------------------------------------------------ [r3] oracle semantics of the exchange
def _worker_oracle(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import numpy as np
    import mvfnet_amd
    from mvfnet_amd import synth
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    m = m.cuda().train()
    eng = m.train_engine(dtype=torch.float32, lr=0.0, momentum=0.0, weight_decay=0.0, max_norm=None)
    imgs = torch.from_numpy(synth.synth_clip_batch(2, 4, 64, 64, seed=10 + rank)).cuda()
    labels = torch.from_numpy(synth.synth_labels(2, seed=10 + rank)).cuda()
    eng.forward(imgs, labels)
    eng.backward(exchange=False)
    local = {k: eng.grad_of(p).cpu().numpy().copy() for k, p in m.named_parameters()}
    eng.step()                                   # all-reduce (sum) of the flat gradient; / world is folded into the (lr = 0) update
    torch.cuda.synchronize()
    summed = {k: eng.grad_of(p).cpu().numpy().copy() for k, p in m.named_parameters()}
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **{"local/" + k: v for k, v in local.items()}, **{"sum/" + k: v for k, v in summed.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_exchanged_gradient_is_the_mean_of_the_oracles_per_rank_gradients(tmp_path):
    """reference dist_utils.py:15-49 with per-GPU BatchNorm (SyncBN is commented out in the reference): the gradient a rank applies is
    sum_r grad_r / world, grad_r = the gradient of rank r's OWN clips under rank r's OWN batch statistics.  Two real ranks (fp32
    engine) with different clips: what the engine holds after the exchange, / world, against the mean of the CPU oracle's two
    per-rank gradients -- and, to make sure the comparison can fail, against either single-rank gradient."""
    import numpy as np
    from helpers import rel_l2
    import mvfnet_amd
    from mvfnet_amd import synth
    from oracle import net_torch
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker_oracle, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(2)]
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips=None))
    sd0 = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd0.items()})
    torch.set_num_threads(min(16, torch.get_num_threads()))
    oracle = []
    for r in range(2):
        sd = {k: torch.from_numpy(vals["r50/" + k]).clone() for k in sd0}
        leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
        imgs = torch.from_numpy(synth.synth_clip_batch(2, 4, 64, 64, seed=10 + r))
        labels = torch.from_numpy(synth.synth_labels(2, seed=10 + r))
        net_torch.forward_train(imgs, labels, sd, 50).backward()
        oracle.append({k: v.grad.numpy() for k, v in leaves.items()})
    names = [k for k, _ in m.named_parameters()]
    assert all(np.array_equal(got[0]["sum/" + k], got[1]["sum/" + k]) for k in names)            # both ranks hold the same summed gradient
    flat = lambda d, pre="": np.concatenate([d[pre + k].ravel() for k in names])                # noqa: E731
    mean_eng = flat(got[0], "sum/") / 2.0
    mean_orc = (flat(oracle[0]) + flat(oracle[1])) / 2.0
    # the engine's own per-rank gradients against the oracle's (the size of a legitimate fp32 difference on this 2-clip network) ...
    d_local = [rel_l2(flat(got[r], "local/"), flat(oracle[r])) for r in range(2)]
    # ... the exchanged mean, and the same mean against a SINGLE rank's gradient (must be far away)
    d_mean = rel_l2(mean_eng, mean_orc)
    d_wrong = min(rel_l2(mean_eng, flat(oracle[r])) for r in range(2))
    per = np.array([rel_l2(got[0]["sum/" + k] / 2.0, (oracle[0][k] + oracle[1][k]) / 2.0) for k in names])
    print("DDP oracle check: local grads vs oracle %.2e / %.2e; exchanged mean vs oracle mean %.2e (per parameter median %.2e max %.2e); vs a single rank's %.2e"
          % (d_local[0], d_local[1], d_mean, np.median(per), per.max(), d_wrong))
    assert np.array_equal(flat(got[0], "sum/"), flat(got[0], "local/") + flat(got[1], "local/")) or rel_l2(flat(got[0], "sum/"), flat(got[0], "local/") + flat(got[1], "local/")) < 1e-6
    # measured: each rank's own gradient is 2.06e-2 from the oracle's (fp32 summation order through 53 batch-statistics BatchNorms on 2 clips:
    # the oracle itself moves by that much between fp32 and fp64), the exchanged mean 2.06e-2, a single rank's 0.68
    assert d_mean < 1.25 * max(d_local) + 1e-3 and d_mean < 4e-2, (d_mean, d_local)
    assert np.median(per) < 4e-2 and per.max() < 8e-2, (np.median(per), per.max())
    assert d_wrong > 10 * d_mean


# ------------------------------------------------------------------------------------------------ [r4] the distributed ENTRY POINTS, executed
class _Videos(torch.utils.data.Dataset):
    """An odd number of tiny synthetic videos with the item layout the reference's datasets emit (img_group [T, 3, H, W], label [1])."""

    def __init__(self, n=5, t=4, size=64):
        from mvfnet_amd import synth
        self.items = [dict(img_group=torch.from_numpy(synth.synth_clip_batch(1, t, size, size, seed=100 + i))[0],
                           label=torch.from_numpy(synth.synth_labels(1, seed=100 + i))[0].reshape(1)) for i in range(n)]
        self.video_infos = [dict(label=int(it["label"][0])) for it in self.items]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _synth_model():
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips="prob"))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m


def _worker_entry_points(rank, world, port, work_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import numpy as np
    from mvfnet_amd.runner import Config, build_dataloader, multi_gpu_test, single_gpu_test, train_network
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ds = _Videos(5)
    m = _synth_model()
    if rank == 1:                         # rank 1 starts from DIFFERENT weights: the wrapper's broadcast must overwrite them (distributed.py:40-52)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.5)
    cfg = Config(optimizer=dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True),
                 optimizer_config=dict(grad_clip=dict(max_norm=40, norm_type=2)),
                 lr_config=dict(policy="step", step=[90, 130], warmup="linear", warmup_iters=4, warmup_ratio=0.1),
                 checkpoint_config=dict(interval=1), log_config=dict(interval=1), total_epochs=2, work_dir=work_dir,
                 data=dict(videos_per_gpu=1, workers_per_gpu=0), resume_from=None, load_from=None)
    logs = []
    run = train_network(m, ds, cfg, distributed=True, validate=False, logger=logs.append)       # reference train.py:159-212 (_dist_train)
    torch.cuda.synchronize()
    dist.barrier()
    info = dict(epoch=run.epoch, iter=run.iter, logs=len(logs))
    bits = run.engine.flat_params.view(torch.int32).to(torch.int64)
    chk = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=bits.device) % 8191 + 1)).sum()]).cpu()
    allc = [torch.zeros_like(chk) for _ in range(world)]
    dist.all_gather(allc, chk)
    info["replicas_equal"] = bool(torch.equal(allc[0], allc[1]))
    # resume on BOTH ranks from rank 0's checkpoint, one more epoch
    m2 = _synth_model()
    cfg2 = Config(dict(cfg, resume_from=os.path.join(work_dir, "latest.pth"), total_epochs=3))
    run2 = train_network(m2, ds, cfg2, distributed=True, logger=logs.append)
    torch.cuda.synchronize()
    bits = run2.engine.flat_params.view(torch.int32).to(torch.int64)
    chk = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=bits.device) % 8191 + 1)).sum()]).cpu()
    allc = [torch.zeros_like(chk) for _ in range(world)]
    dist.all_gather(allc, chk)
    info.update(epoch2=run2.epoch, iter2=run2.iter, replicas_equal2=bool(torch.equal(allc[0], allc[1])),
                finite=bool(torch.isfinite(run2.engine.flat_params).all()))
    # multi_gpu_test + collect_results on the odd-sized dataset (reference test.py:42-89, 147-185): rank 0's ordered rows == one process scoring all.
    # As test_recognizer.py does, every rank first loads rank 0's checkpoint: BatchNorm running statistics are per rank during training (no
    # SyncBN in the reference either), only the parameters are kept identical by the gradient exchange.
    from mvfnet_amd.checkpoint import load_checkpoint
    dist.barrier()
    load_checkpoint(m2, os.path.join(work_dir, "epoch_3.pth"), map_location="cpu", strict=True)
    loader = build_dataloader(ds, 1, 0, dist_mode=True, shuffle=False)
    rows = multi_gpu_test(m2, loader, size=len(ds))
    if rank == 0:
        full = single_gpu_test(m2, build_dataloader(ds, 1, 0, dist_mode=False, shuffle=False))
        info["rows"] = len(rows)
        info["max_abs_diff"] = float(max(np.abs(np.asarray(a, dtype=np.float64).reshape(-1) - np.asarray(b, dtype=np.float64).reshape(-1)).max()
                                         for a, b in zip(rows, full)))
        info["argmax_equal"] = all(int(np.argmax(a)) == int(np.argmax(b)) for a, b in zip(rows, full))
    else:
        info["rows"] = rows
    torch.save(info, os.path.join(work_dir, "info_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_dist_train_and_multi_gpu_test_entry_points_run_with_two_ranks(tmp_path):
    """reference core/train.py:159-212 (`_dist_train`) and core/test.py:42-89 / 147-185, EXECUTED with two real ranks on one MI355X
    (gloo carrying the CUDA tensors): train_network(distributed=True) for two epochs over an odd-sized dataset (DistributedSampler pads
    5 videos to 3 per rank), the wrapper's broadcast overwrites rank 1's different start, replicas stay bit-identical, rank 0 writes the
    checkpoints, both ranks resume from them for a third epoch; then multi_gpu_test + collect_results: rank 0 receives the 5 rows in
    dataset order, equal to one process scoring all five."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker_entry_points, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    i0, i1 = (torch.load(str(tmp_path / ("info_rank%d.pt" % r)), weights_only=False) for r in range(2))
    assert i0["epoch"] == i1["epoch"] == 2 and i0["iter"] == i1["iter"] == 6          # ceil(5 / 2) = 3 iterations per epoch and rank
    assert i0["logs"] > 0 and i1["logs"] == 0                                          # only rank 0 logs
    assert i0["replicas_equal"] and i0["replicas_equal2"] and i0["finite"]
    assert i0["epoch2"] == i1["epoch2"] == 3 and i0["iter2"] == i1["iter2"] == 9
    assert os.path.exists(str(tmp_path / "epoch_3.pth")) and os.path.islink(str(tmp_path / "latest.pth"))
    assert i1["rows"] is None and i0["rows"] == 5
    assert i0["argmax_equal"] and i0["max_abs_diff"] < 1e-6                            # same weights, same kernels, per-video batches


@pytest.mark.timeout(600)
def test_bench_runs_its_rccl_path_with_one_rank():
    """BENCH_FORCE_DIST=1: bench.py initialises the nccl (= RCCL) process group on this box, runs the two-bucket exchange with world = 1,
    verifies its replicas and reports how much of the all-reduce is exposed -- so RCCL initialisation and the communication-stream
    choreography execute wherever the GPU tests run."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--steps", "2", "--warmup", "1", "--clips", "8", "--full", "--no-cpu-baseline",
                        "--no-other-configs", "--no-eager-compare"], capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rep = d["replicas"]
    assert rep["backend"] == "nccl" and rep["rccl_ranks"] == 1 and rep["params_bit_identical_across_ranks"]
    assert rep["allreduce_ms"]["tail_bucket_overlapped_with_backward"] > 0 and d["value"] > 0


@pytest.mark.timeout(900)
def test_bench_multi_rank_path_with_two_ranks_on_one_gpu():
    """[r5] `bench.py --gpus 2` exactly as the driver launches it (python -m torch.distributed.run, one process per rank), rehearsed on a ONE-GPU
    box: BENCH_BACKEND=gloo puts both ranks on cuda:0 with gloo carrying the CUDA tensors (RCCL refuses two ranks per device).  Everything the
    multi-GPU run adds executes with world = 2: per-rank seeds, barrier + synchronize brackets, MAX over ranks, `rank_ms_per_step`, whole-job
    `value`, `verify_replicas` (bit-identical parameters across ranks after the timed steps) and the exposed-all-reduce triple."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--clips", "4", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=800, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["config"]["clips_per_gpu"] == 4
    rk = d["rank_ms_per_step"]
    assert len(rk["all"]) == 2 and abs(rk["max"] - d["ms_per_step"]) < 1e-2 * d["ms_per_step"]          # MAX over ranks is what is reported
    assert abs(d["value"] - 2 * 4 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]                        # whole-job clips/s over both ranks
    rep = d["replicas"]
    assert rep["backend"] == "gloo" and rep["rccl_ranks"] == 2 and rep["params_bit_identical_across_ranks"]
    assert set(rep["allreduce_ms"]) == {"tail_bucket_overlapped_with_backward", "single_collective_after_backward", "no_exchange", "exposed"}
    assert "cpu_baseline" not in d and "other_configs" not in d                                           # N = 1 only
    assert d["roofline"]["frac"] > 0
