#!/usr/bin/env python3
"""Digests of everything the classification head computes, printed as one JSON object: the four fused train-head forms + mvf_head_train_bwd, the stand-alone
losses, the inference head, the relation head and whole train steps (default, label smoothing, BCE, focal, TRN; eager, recorded and replayed).

Run once per library (MVF_LIB_PATH selects it, one process each) and compare the two outputs byte for byte: a refactor of the head must reproduce every digest.
Output buffers are prefilled with NaN; every array is a view into an allocation of its own with a margin in front and behind -- one element for arrays the kernels
address by element, 16 bytes for those they address by 8- / 16-byte vectors (feat, the dropout mask, pooled, dpool, dfeat) -- and the SHA-256 is taken over the
whole allocation, so a store outside an array changes a digest too.

    python tools/head_digest.py [--no-engine] > digest.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from mvfnet_amd import _lib as L, synth  # noqa: E402
from mvfnet_amd.heads import relation as rel  # noqa: E402

lib, check = L.lib, L.check
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
ALLOCS = {}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def view(t, vec=False):
    """`t` on the device as a view into an allocation with a NaN (0xFF for integers) margin on both sides; the allocation is remembered for sha()."""
    if t is None:
        return None
    t = t.contiguous()
    lead = max(16 // t.element_size(), 1) if vec else 1
    whole = torch.full((t.numel() + 2 * lead,), NAN if t.is_floating_point() else -1, dtype=t.dtype, device="cuda")
    v = whole[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    ALLOCS[v.data_ptr()] = whole
    return v


def out(shape, dtype=F32, vec=False):
    return view(torch.full(shape, NAN).to(dtype), vec)


def sha(**views):
    torch.cuda.synchronize()
    return {k: hashlib.sha256(ALLOCS[v.data_ptr()].view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16] for k, v in views.items() if v is not None}


# ---------------------------------------------------------------------------------------------------------------- the fused forms + backward
def fused_forms(res):
    from test_head_optimizer_gpu import HEAD_CASES, head_inputs
    focal_recipes = [(2.0, 2.0, 0.0, 0.25), (1.0, 4.0, 0.05, -1.0), (3.0, 1.5, 0.2, 0.75)]
    for name, case in HEAD_CASES.items():
        clips, T, hw, c, classes = case
        for dtype in (F32, BF16):
            for p in (0.0, 0.5):
                inp = head_inputs(case, dtype, p)
                dt = 0 if dtype == F32 else 1
                gen = torch.Generator().manual_seed(clips * 7 + classes)
                targets = view(torch.rand(clips, classes, generator=gen) ** 3)
                pw = view(torch.rand(classes, generator=gen) * 4 + 0.25)
                feat, w, b = view(inp["feat"].to(dtype), True), view(inp["w"]), view(inp["b"])
                lab, mask = view(inp["labels"]), view(inp["mask"], True)
                forms = [("hard", "mvf_head_train_fwd", lab, ()), ("soft", "mvf_head_train_fwd_soft", targets, ())]
                for pwv in (None, pw):
                    for thr in (NAN, 0.5):
                        for sc in (0, 1):
                            forms.append(("bce_pw%d_thr%s_sum%d" % (pwv is not None, thr, sc), "mvf_head_train_fwd_bce", targets, (P(pwv), C.c_float(thr), sc)))
                for i, (gp, gn, m, al) in enumerate(focal_recipes):
                    prm = L.FocalParams(gamma_pos=gp, gamma_neg=gn, margin=m, alpha=al, target_threshold=NAN, sum_classes=0)
                    forms.append(("focal%d" % i, "mvf_head_train_fwd_focal", targets, (P(pw), prm)))
                for tag, fn, tg, mid in forms:
                    pooled, scores, dsc = out((clips * T, c), vec=True), out((clips, classes)), out((clips, classes))
                    lp, lo = out((clips,)), out((1,))
                    check(getattr(lib, fn)(P(feat), clips, T, hw, c, P(w), P(b), classes, P(tg), P(mask), *mid, P(pooled), P(scores), P(dsc), P(lp), P(lo), dt, None), fn)
                    dfw, dfb, dpool, dfeat = out((classes, c)), out((classes,)), out((clips, c), vec=True), out((clips * T, hw, c), dtype, True)
                    check(lib.mvf_head_train_bwd(P(dsc), P(pooled), P(w), P(mask), clips, T, hw, c, classes, P(dfw), P(dfb), P(dpool), P(dfeat), dt, None), "bwd")
                    res["fused/%s/%s/p%g/%s" % (name, "f32" if dtype == F32 else "bf16", p, tag)] = sha(
                        pooled=pooled, scores=scores, dscores=dsc, loss_part=lp, loss=lo, dfc_w=dfw, dfc_b=dfb, dfeat=dfeat)
                ALLOCS.clear()


# ---------------------------------------------------------------------------------------------------------------- the stand-alone losses
def stand_alone(res):
    for clips in (1, 7, 65):
        for classes in (1, 257, 400):
            gen = torch.Generator().manual_seed(clips * 1009 + classes)
            s = view(torch.randn(clips, classes, generator=gen) * 6)
            z = view(torch.randn(clips, classes, generator=gen) * 6)
            tg = view(torch.rand(clips, classes, generator=gen) ** 3)
            lab = view(torch.randint(0, classes, (clips,), generator=gen))
            cw = view(torch.rand(classes, generator=gen) * 4 + 0.25)
            prm = L.FocalParams(gamma_pos=1.0, gamma_neg=4.0, margin=0.05, alpha=-1.0, target_threshold=NAN, sum_classes=0)
            calls = [("ce", lambda d, lp, lo: lib.mvf_ce_loss(P(s), P(lab), clips, classes, P(d), P(lp), P(lo), None)),
                     ("ce_soft", lambda d, lp, lo: lib.mvf_ce_loss_soft(P(s), P(tg), clips, classes, P(d), P(lp), P(lo), None)),
                     ("bce", lambda d, lp, lo: lib.mvf_bce_loss(P(s), P(tg), clips, classes, P(cw), C.c_float(NAN), 0, P(d), P(lp), P(lo), None)),
                     ("focal", lambda d, lp, lo: lib.mvf_focal_loss(P(s), P(tg), clips, classes, P(cw), prm, P(d), P(lp), P(lo), None))]
            for tag, call in calls:
                for with_d in (False, True):
                    d, lp, lo = (out((clips, classes)) if with_d else None), out((clips,)), out((1,))
                    check(call(d, lp, lo), tag)
                    res["loss/%s/n%d_k%d/dscores%d" % (tag, clips, classes, with_d)] = sha(dscores=d, loss_part=lp, loss=lo)
            for with_terms in (False, True):
                d, lp, lo = out((clips, classes)), out((clips,)), out((1,))
                check(lib.mvf_ce_loss(P(s), P(lab), clips, classes, P(d), P(lp), P(lo), None), "ce")
                terms = out((2,)) if with_terms else None
                check(lib.mvf_distill_loss(P(s), P(z), clips, classes, C.c_float(4.0), C.c_float(0.7), P(d), P(lp), P(lo), P(terms), None), "distill")
                res["loss/distill/n%d_k%d/terms%d" % (clips, classes, with_terms)] = sha(dscores=d, loss_part=lp, loss=lo, terms=terms)
            ALLOCS.clear()


# ---------------------------------------------------------------------------------------------------------------- the inference head
def inference_head(res):
    for T, hw, c, classes in ((1, 1, 4, 10), (8, 49, 2048, 400)):          # test_head_pool_fc_vs_fp64's smallest and largest case
        for dtype in (F32, BF16):
            gen = torch.Generator().manual_seed(T * hw * 4099 + c * 17 + classes)
            feat = view((torch.randn(3 * T, hw, c, generator=gen) + 0.5).to(dtype), True)
            w, b = view(torch.randn(classes, c, generator=gen) / float(np.sqrt(c))), view(torch.randn(classes, generator=gen))
            pooled, sc = out((3, c), vec=True), out((3, classes))
            check(lib.mvf_head_pool_fc(P(feat), 3, T, hw, c, P(w), P(b), classes, P(pooled), P(sc), 0 if dtype == F32 else 1, None), "head_pool_fc")
            res["infer/pool_fc/rows%d_c%d_k%d/%s" % (T * hw, c, classes, "f32" if dtype == F32 else "bf16")] = sha(pooled=pooled, scores=sc)
    for clips, classes in ((1, 10), (30, 2048)):                            # test_average_clip_vs_fp64's
        s = view(torch.randn(clips, classes, generator=torch.Generator().manual_seed(clips + classes)) * 3)
        for kind in (0, 1, 2):
            o = out((clips, classes) if kind == 0 else (classes,))
            check(lib.mvf_average_clip(P(s), clips, classes, kind, P(o), None), "average_clip")
            res["infer/average_clip/n%d_k%d/kind%d" % (clips, classes, kind)] = sha(out=o)
    for clips, classes in ((1, 1), (10, 400)):                              # test_average_clip_sigmoid_vs_fp64's
        s = view(torch.randn(clips, classes, generator=torch.Generator().manual_seed(clips * 1009 + classes)) * 6)
        o = out((classes,))
        check(lib.mvf_average_clip_sigmoid(P(s), clips, classes, P(o), None), "average_clip_sigmoid")
        res["infer/average_clip_sigmoid/n%d_k%d" % (clips, classes)] = sha(out=o)
    ALLOCS.clear()


# ---------------------------------------------------------------------------------------------------------------- the relation head
def relation_head(res):
    from test_trn_head_gpu import FDIM, _hidden, make_params
    clips, T, hw, c, classes = 3, 8, 49, 64, 174                           # test_end_to_end_on_a_random_case's
    for kind in ("TRN", "TRNmultiscale"):
        for dtype in (F32, BF16):
            gen = np.random.default_rng(17 + (kind == "TRN"))
            fc_w, fc_b, scales = make_params(kind, T, c, classes, gen)
            np.random.seed(int(gen.integers(1 << 30)))
            table = rel.draw_relation_table(kind, T).astype(np.int32)
            rows, H = int(table.shape[0]), _hidden(kind)
            up = lambda a, vec=False: view(torch.from_numpy(np.ascontiguousarray(a)), vec)  # noqa: E731
            feat = view(torch.from_numpy((gen.standard_normal((clips * T, hw, c)) + 0.5).astype(np.float32)).to(dtype), True)
            mask = up(((gen.random((clips * T, c)) >= 0.5) * 2.0).astype(np.float32), True)
            dsc = up((gen.standard_normal((clips, classes)) / clips).astype(np.float32))
            fcw, fcb, tab = up(fc_w), up(fc_b), up(table)
            par = [tuple(up(a, True) for a in sc) for sc in scales]
            grads = [tuple(out(tuple(a.shape), vec=True) for a in sc) for sc in par]
            arr = (L.TrnScale * len(par))()
            for i, (sc, g) in enumerate(zip(par, grads)):
                for j, nm in enumerate(("w1", "b1", "w2", "b2")):
                    setattr(arr[i], nm, sc[j].data_ptr())
                    setattr(arr[i], "d" + nm, g[j].data_ptr())
            fr, dt = clips * T, 0 if dtype == F32 else 1
            o = dict(pooled=out((fr, c), vec=True), f=out((fr, FDIM), vec=True), h=out((rows, clips, H), vec=True), hpart=out((L.TRN_KSPLIT_MAX, rows, clips, H), vec=True),
                     scores=out((clips, classes)), dfc_w=out((FDIM, c), vec=True), dfc_b=out((FDIM,)), dh=out((rows, clips, H), vec=True), df=out((fr, FDIM), vec=True),
                     dpool=out((fr, c), vec=True), dfeat=out((fr, hw, c), dtype, True))
            info = L.TrnLaunchInfo()
            check(lib.mvf_trn_head_fwd(P(feat), clips, T, hw, c, P(fcw), P(fcb), FDIM, arr, len(arr), H, classes, P(tab), rows, P(mask), P(o["pooled"]), P(o["f"]),
                                       P(o["h"]), P(o["hpart"]), P(o["scores"]), dt, None), "trn fwd")
            lib.mvf_trn_head_last_launch(C.byref(info))
            n_fwd = info.launches
            check(lib.mvf_trn_head_bwd(P(dsc), P(o["pooled"]), P(o["f"]), P(o["h"]), P(fcw), arr, len(arr), H, classes, P(tab), rows, P(mask), clips, T, hw, c, FDIM,
                                       P(o["dfc_w"]), P(o["dfc_b"]), P(o["dh"]), P(o["df"]), P(o["dpool"]), P(o["dfeat"]), dt, None), "trn bwd")
            lib.mvf_trn_head_last_launch(C.byref(info))
            d = sha(**{k: v for k, v in o.items() if k != "hpart"})        # (hpart: only the splits the call used are written)
            d.update(sha(**{"d%s%d" % (nm, i): g[j] for i, g in enumerate(grads) for j, nm in enumerate(("w1", "b1", "w2", "b2"))}))
            d["launches"] = [n_fwd, info.launches]
            res["trn/%s/%s" % (kind, "f32" if dtype == F32 else "bf16")] = d
            ALLOCS.clear()


# ---------------------------------------------------------------------------------------------------------------- the train engine
def engine_steps(res):
    import mvfnet_amd
    CW = [0.5 + 0.25 * (i % 5) for i in range(400)]
    configs = {"default": {}, "smoothing": dict(label_smooth_eps=0.1), "bce": dict(loss_cls=dict(type="BCELossWithLogits")),
               "focal": dict(loss_cls=dict(type="SigmoidFocalLoss", gamma=2.0, alpha=0.25, class_weight=CW)),
               "trn": dict(consensus_cfg=dict(type="TRNmultiscale", num_frames=4))}
    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen)) for _ in range(3)]
    for name, head_kw in configs.items():
        torch.manual_seed(7)                                                 # the dropout masks
        np.random.seed(11)                                                   # the relation draws
        cfg = mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.5)
        cfg["cls_head"].update(head_kw)
        m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd})
        eng = m.cuda().train().train_engine(dtype=BF16)
        eng.use_plan = True
        steps = []
        for i in range(6):                                                   # two eager, two recordings, two replays
            imgs, labels = batches[i % 3]
            loss = eng.train_step(imgs.clone(), labels.clone(), lr=0.01)
            torch.cuda.synchronize()
            steps.append([hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16] for t in (loss.reshape(1).float(), eng.flat_params)])
        plans = [s["plan"] for s in getattr(eng, "_plans", {}).values() if s["plan"] is not None]
        res["engine/" + name] = dict(steps=steps, plan_ops=[p.n_ops for p in plans], plan_names=[hashlib.sha256(" ".join(p.names).encode()).hexdigest()[:16] for p in plans],
                                     head_calls=[[n for n in p.names if "head" in n or "loss" in n or "soft_targets" in n] for p in plans])


def main():
    res = {}
    fused_forms(res)
    stand_alone(res)
    inference_head(res)
    relation_head(res)
    if "--no-engine" not in sys.argv:
        engine_steps(res)
    res["digests"] = json.dumps(res).count('": "') + sum(2 * len(v["steps"]) + len(v["plan_names"]) for k, v in res.items() if k.startswith("engine/"))
    print(json.dumps(res, sort_keys=True, indent=0))


if __name__ == "__main__":
    main()
