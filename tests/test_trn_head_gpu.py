"""GPU: the temporal-relation head -- mvf_trn_head_fwd / mvf_trn_head_bwd (csrc/trn_head.hip) stage by stage against the fp64 restatement in trn_numpy.py, end
to end on the reference's fixture cases (tests/golden/trn_cases.npz), and the train engine with a 'TRN' / 'TRNmultiscale' head.

Stage-wise bound, derived rather than measured.  Each stage's restatement is fed the DEVICE's own stored inputs of that stage, so only that stage's rounding
is in the difference.  Every output element is an fp32 sum of K products plus a bias (and, where relation rows are summed into it, R row terms); for any
summation order, with or without FMA,
    |dev - ref| <= gamma_{K + R + 2} * (sum |a_i b_i| + |bias|),   gamma_n = n u / (1 - n u), u = 2^-24
with the magnitude computed per element from abs(A) @ abs(B).  The pooled mean (hw - 1 additions, a division, the mask) gets gamma_{hw + 1}.  The ReLU gates
of the backward are exact: dh is 0 wherever the stored h is not > 0, df wherever the stored f is not > 0.  dfeat is dpool's bits (fp32) or one rounding of
them to bf16 (8 significant bits, round to nearest: 2^-8 relative)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import trn_numpy as tn
from helpers import NamesOf, library_names
from mvfnet_amd import synth
from mvfnet_amd.heads import relation as rel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32, BF16 = torch.float32, torch.bfloat16
FDIM = 256
LOSS_BOUND = 5e-5            # the average head's end-to-end loss bound (test_head_optimizer_gpu.py)
HEAD_BOUND = 5e-5            # the suite's bound for head tensors across several fp32 stages, relative to the tensor's largest magnitude


def _lib():
    from mvfnet_amd import _lib as L
    return L


def _hidden(kind):
    return 512 if kind == "TRN" else 256


def make_params(kind, T, c, classes, gen):
    """(fc_w, fc_b, scales) as float32 numpy arrays with O(1) activations."""
    n = lambda *s: gen.standard_normal(s).astype(np.float32)  # noqa: E731
    H = _hidden(kind)
    fc_w, fc_b = n(FDIM, c) / np.float32(np.sqrt(c)), n(FDIM) * np.float32(0.1)
    scales = []
    for s in ([T] if kind == "TRN" else range(T, 1, -1)):
        k = s * FDIM
        scales.append((n(H, k) / np.float32(np.sqrt(k / 2)), n(H) * np.float32(0.1), n(classes, H) / np.float32(np.sqrt(H / 2)), n(classes) * np.float32(0.1)))
    return fc_w, fc_b, scales


class Device(object):
    """One relation head on the device through the C ABI: parameters, buffers filled with NaN, the launch record after each call."""

    def __init__(self, kind, clips, T, hw, c, classes, dtype, fc_w, fc_b, scales, table, mask):
        L = _lib()
        dev = "cuda"
        self.L, self.kind, self.dims, self.dtype = L, kind, (clips, T, hw, c, classes), dtype
        self.H, self.rows = _hidden(kind), int(table.shape[0])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.fc_w, self.fc_b, self.table = up(fc_w), up(fc_b), up(table.astype(np.int32))
        self.mask = up(mask) if mask is not None else None
        self.scales = [tuple(up(a) for a in sc) for sc in scales]
        nan = float("nan")
        self.grads = [tuple(torch.full_like(a, nan) for a in sc) for sc in self.scales]
        self.arr = (L.TrnScale * len(scales))()
        for i, (sc, g) in enumerate(zip(self.scales, self.grads)):
            for j, name in enumerate(("w1", "b1", "w2", "b2")):
                setattr(self.arr[i], name, sc[j].data_ptr())
                setattr(self.arr[i], "d" + name, g[j].data_ptr())
        full = lambda *s: torch.full(s, nan, device=dev)  # noqa: E731
        fr = clips * T
        self.out = dict(pooled=full(fr, c), f=full(fr, FDIM), h=full(self.rows, clips, self.H), hpart=full(L.TRN_KSPLIT_MAX, self.rows, clips, self.H), scores=full(clips, classes), dfc_w=full(FDIM, c), dfc_b=full(FDIM),
                        dh=full(self.rows, clips, self.H), df=full(fr, FDIM), dpool=full(fr, c), dfeat=full(fr, hw, c).to(dtype))

    def P(self, t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def launches(self):
        info = self.L.TrnLaunchInfo()
        assert self.L.lib.mvf_trn_head_last_launch(C.byref(info)) == 0
        return info.entry, info.launches, info.rows

    def fwd(self, feat, table=None, rows=None):
        clips, T, hw, c, classes = self.dims
        o, P = self.out, self.P
        self.feat = feat
        self.L.check(self.L.lib.mvf_trn_head_fwd(P(feat), clips, T, hw, c, P(self.fc_w), P(self.fc_b), FDIM, self.arr, len(self.arr), self.H, classes,
                                                  P(self.table if table is None else table), self.rows if rows is None else rows, P(self.mask), P(o["pooled"]),
                                                  P(o["f"]), P(o["h"]), P(o["hpart"]), P(o["scores"]), 0 if self.dtype == F32 else 1, None), "mvf_trn_head_fwd")
        assert self.launches() == (1, 5, self.rows if rows is None else rows)          # the header's count: 5 launches, whatever the rows

    def bwd(self, dscores):
        clips, T, hw, c, classes = self.dims
        o, P = self.out, self.P
        self.L.check(self.L.lib.mvf_trn_head_bwd(P(dscores), P(o["pooled"]), P(o["f"]), P(o["h"]), P(self.fc_w), self.arr, len(self.arr), self.H, classes, P(self.table),
                                                  self.rows, P(self.mask), clips, T, hw, c, FDIM, P(o["dfc_w"]), P(o["dfc_b"]), P(o["dh"]), P(o["df"]), P(o["dpool"]),
                                                  P(o["dfeat"]), 0 if self.dtype == F32 else 1, None), "mvf_trn_head_bwd")
        assert self.launches() == (2, 7, self.rows)                                    # 7 launches, whatever the rows

    def host(self):
        torch.cuda.synchronize()
        out = {k: v.float().cpu().numpy() for k, v in self.out.items()}
        out["dscales"] = [tuple(a.cpu().numpy() for a in g) for g in self.grads]
        return out


def within(dev, ref, mag, n, what):
    """|dev - ref| <= gamma_n * magnitude, per element; prints the worst ratio of the two."""
    dev, ref, mag = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(mag, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    assert dev.shape == ref.shape and np.isfinite(dev).all(), what
    bound = (n * tn.U / (1.0 - n * tn.U)) * mag
    d = np.abs(dev - ref)
    worst = float((d / np.maximum(bound, 1e-300)).max()) if d.size else 0.0
    print("%-8s worst |dev - ref| / bound = %.3f   (max-norm rel %.3g)" % (what, worst, d.max() / max(np.abs(ref).max(), 1e-300)))
    assert (d <= bound).all(), (what, worst)


def check_stages(got, dev_in, kind, T, hw, fc_w, fc_b, scales, table, mask, dscores, dtype):
    """Every stage against its restatement on the device's own inputs of that stage."""
    clips = got["scores"].shape[0]
    H, R = _hidden(kind), table.shape[0]
    c = fc_w.shape[1]
    val, mag = tn.stage_pool(dev_in, mask)
    within(got["pooled"], val, mag, hw + 1, "pooled")
    val, mag = tn.stage_fc(got["pooled"], fc_w, fc_b)
    within(got["f"], val, mag, c + 2, "f")
    pre, mag = tn.stage_hidden(got["f"], scales, table, clips, T)
    k_r = np.array([(T - int(table[r, 0])) * FDIM for r in range(R)], dtype=np.float64).reshape(R, 1, 1)
    within(got["h"], np.maximum(pre, 0.0), mag, k_r + 2, "h")
    val, mag = tn.stage_scores(got["h"], scales, table, T)
    within(got["scores"], val, mag, R * H + R + 2, "scores")
    # backward
    for si, (dw2, mw, db2, mb) in enumerate(tn.stage_dw2(dscores, got["h"], scales, table, T)):
        nr = int((table[:, 0] == si).sum())
        within(got["dscales"][si][2], dw2, mw, nr * clips + nr + 2, "dw2[%d]" % si)
        within(got["dscales"][si][3], db2, mb, nr * clips + nr + 2, "db2[%d]" % si)
    val, mag = tn.stage_dh(dscores, got["h"], scales, table, T)
    within(got["dh"], val, mag, dscores.shape[1] + 2, "dh")
    assert (got["dh"][~(got["h"] > 0)] == 0.0).all()                       # the ReLU gate is the stored h > 0, bit for bit
    for si, (dw1, mw, db1, mb) in enumerate(tn.stage_dw1(got["dh"], got["f"], scales, table, clips, T)):
        nr = int((table[:, 0] == si).sum())
        within(got["dscales"][si][0], dw1, mw, nr * clips + nr + 2, "dw1[%d]" % si)
        within(got["dscales"][si][1], db1, mb, nr * clips + nr + 2, "db1[%d]" % si)
    val, mag, cnt = tn.stage_df(got["dh"], got["f"], scales, table, clips, T)
    n_t = np.tile((cnt * H + cnt + 2).astype(np.float64), clips).reshape(clips * T, 1)
    within(got["df"], val, mag, n_t, "df")
    assert (got["df"][~(got["f"] > 0)] == 0.0).all()
    dw, mw, db, mb = tn.stage_dfc(got["df"], got["pooled"])
    within(got["dfc_w"], dw, mw, clips * T + 2, "dfc_w")
    within(got["dfc_b"], db, mb, clips * T + 2, "dfc_b")
    val, mag = tn.stage_dpool(got["df"], fc_w, hw, mask)
    within(got["dpool"], val, mag, FDIM + 2, "dpool")
    want = np.repeat(got["dpool"][:, None, :], hw, axis=1)
    if dtype == F32:
        assert np.array_equal(got["dfeat"], want)
    else:
        assert (np.abs(got["dfeat"].astype(np.float64) - want) <= 2.0 ** -8 * np.abs(want)).all()      # bf16: 8 significant bits, round to nearest
    if mask is not None:
        dropped = mask == 0
        assert (got["pooled"][dropped] == 0.0).all() and (got["dfeat"][np.broadcast_to(dropped[:, None, :], got["dfeat"].shape)] == 0.0).all()


# (kind, clips, T, hw, c, classes, dtype, p): every value of every axis, the pairs at which a kernel takes another path (one clip: a partial 16-row tile;
# hw = 1: no pooling; one class: a quarter-filled score workgroup; 174 classes: several; T = 2 multi-scale: the one row), c = 2048 once per type at 3 clips
CASES = [
    ("TRN", 1, 2, 1, 64, 1, F32, 0.0),
    ("TRN", 3, 8, 49, 64, 5, BF16, 0.5),
    ("TRN", 3, 8, 49, 2048, 174, BF16, 0.5),
    ("TRN", 1, 8, 1, 64, 174, F32, 0.5),
    ("TRN", 3, 2, 49, 64, 5, F32, 0.0),
    ("TRNmultiscale", 1, 2, 1, 64, 5, BF16, 0.0),
    ("TRNmultiscale", 3, 3, 49, 64, 1, F32, 0.5),
    ("TRNmultiscale", 1, 3, 1, 64, 174, BF16, 0.5),
    ("TRNmultiscale", 3, 8, 49, 2048, 174, BF16, 0.5),
    ("TRNmultiscale", 1, 8, 49, 64, 5, F32, 0.0),
    ("TRNmultiscale", 3, 8, 1, 64, 1, BF16, 0.0),
    ("TRNmultiscale", 3, 2, 49, 64, 174, F32, 0.5),
]


def _id(case):
    kind, clips, T, hw, c, classes, dtype, p = case
    return "%s-n%d-t%d-hw%d-c%d-k%d-%s-%s" % (kind, clips, T, hw, c, classes, "f32" if dtype == F32 else "bf16", "mask" if p else "nomask")


def _setup(case, seed=0):
    kind, clips, T, hw, c, classes, dtype, p = case
    gen = np.random.default_rng((((clips * 31 + T) * 131 + hw) * 8191 + c * 701 + classes) * 3 + (kind == "TRN") + seed * 7919)
    fc_w, fc_b, scales = make_params(kind, T, c, classes, gen)
    feat = (gen.standard_normal((clips * T, hw, c)) + 0.5).astype(np.float32)
    feat_d = torch.from_numpy(feat).cuda().to(dtype).contiguous()
    feat = feat_d.float().cpu().numpy()                                   # the restatement takes the rounded input
    mask = None
    if p > 0:
        mask = ((gen.random((clips * T, c)) >= p) * (1.0 / (1.0 - p))).astype(np.float32)
    np.random.seed(int(gen.integers(1 << 30)))
    table = rel.draw_relation_table(kind, T)
    dscores = (gen.standard_normal((clips, classes)) / clips).astype(np.float32)
    d = Device(kind, clips, T, hw, c, classes, dtype, fc_w, fc_b, scales, table, mask)
    return d, feat, feat_d, dict(fc_w=fc_w, fc_b=fc_b, scales=scales, table=table, mask=mask, dscores=dscores)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_stage_within_its_derived_bound(case):
    kind, clips, T, hw, c, classes, dtype, p = case
    d, feat, feat_d, q = _setup(case)
    assert q["table"].shape[0] == rel.relation_rows(kind, T)
    d.fwd(feat_d)
    ds_d = torch.from_numpy(q["dscores"]).cuda()
    d.bwd(ds_d)
    got = d.host()
    check_stages(got, feat, kind, T, hw, q["fc_w"], q["fc_b"], q["scales"], q["table"], q["mask"], q["dscores"], dtype)
    # determinism: the same calls again leave the same bits everywhere
    for v in d.out.values():
        v.fill_(float("nan"))
    d.fwd(feat_d)
    d.bwd(ds_d)
    again = d.host()
    for k in got:
        if k == "hpart":
            continue                                                        # a workspace: the K splits a shape does not use stay unwritten
        if k == "dscales":
            assert all(np.array_equal(a, b) for ga, gb in zip(got[k], again[k]) for a, b in zip(ga, gb))
        else:
            assert np.array_equal(got[k], again[k]), k


def test_table_order_and_other_relations():
    """Rows of the scales below T in another order: the same sum in another order, within twice the stage bound of each other.  Other relations: more."""
    case = ("TRNmultiscale", 3, 8, 1, 64, 5, F32, 0.0)
    d, feat, feat_d, q = _setup(case)
    d.fwd(feat_d)
    got = d.host()
    _, mag = tn.stage_scores(got["h"], q["scales"], q["table"], 8)
    R, H = q["table"].shape[0], 256
    exact, _ = tn.stage_scores(got["h"], q["scales"], q["table"], 8)
    bound = tn.gamma(R * H + R + 2) * mag
    perm = np.concatenate([[0], 1 + np.random.default_rng(1).permutation(R - 1)])
    assert not np.array_equal(perm, np.arange(R))
    ptable = np.ascontiguousarray(q["table"][perm])
    rel.check_relation_table(ptable, "TRNmultiscale", 8)
    d.fwd(feat_d, table=torch.from_numpy(ptable).cuda())
    permuted = d.host()
    assert np.array_equal(permuted["h"], got["h"][perm])                   # the same relations, stored in the table's new order
    # the permuted run's scores against the fp64 sum of its own h in its own order, and against the fp64 sum of the ORIGINAL order: both within the stage
    # bound (in fp64 the two orders differ by 1e-16), so the change the permutation makes is no more than the stage bound
    val, pmag = tn.stage_scores(permuted["h"], q["scales"], ptable, 8)
    within(permuted["scores"], val, pmag, R * H + R + 2, "permuted")
    diff = np.abs(permuted["scores"].astype(np.float64) - exact)
    print("permuted rows: worst |scores - fp64 sum in the original order| / bound = %.3f" % float((diff / bound).max()))
    assert (diff <= bound).all()
    np.random.seed(12345)
    other = rel.draw_relation_table("TRNmultiscale", 8)
    assert not np.array_equal(other, q["table"])
    d.fwd(feat_d, table=torch.from_numpy(other).cuda())
    assert (np.abs(d.host()["scores"].astype(np.float64) - got["scores"]) > bound).any()


def test_a_bad_table_cannot_read_outside_a_tensor():
    """The kernels clamp the scale index and every frame index: a table check_relation_table refuses gives the scores of its clamped self."""
    case = ("TRNmultiscale", 1, 3, 1, 64, 5, F32, 0.0)
    d, feat, feat_d, q = _setup(case)
    bad = np.array([[0, 0, 1, 2], [7, 0, 99, -1], [-3, -5, 1, 2], [1, 1, 2, -1]], dtype=np.int32)
    clamped = np.array([[0, 0, 1, 2], [1, 0, 2, 0], [0, 0, 1, 2], [1, 1, 2, 0]], dtype=np.int32)
    with pytest.raises(ValueError):
        rel.check_relation_table(bad, "TRNmultiscale", 3)
    d.fwd(feat_d, table=torch.from_numpy(bad).cuda())
    a = d.host()["scores"]
    d.fwd(feat_d, table=torch.from_numpy(clamped).cuda())
    assert np.isfinite(a).all() and np.array_equal(a, d.host()["scores"])


def _end_to_end(kind, T, classes, c, feat_nhwc, fc_w, fc_b, scales, table, labels, dtype=F32):
    """Device forward + mvf_ce_loss + backward against the fp64 chain from the inputs; -> the observed max-norm relative errors."""
    clips, hw = feat_nhwc.shape[0] // T, feat_nhwc.shape[1]
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    d = Device(kind, clips, T, hw, c, classes, dtype, f32(fc_w), f32(fc_b), [tuple(f32(a) for a in sc) for sc in scales], table, None)
    feat_d = torch.from_numpy(f32(feat_nhwc)).cuda().to(dtype).contiguous()
    d.fwd(feat_d)
    L = d.L
    lab = torch.from_numpy(labels).cuda()
    dsc, part, loss = torch.empty(clips, classes, device="cuda"), torch.empty(clips, device="cuda"), torch.empty(1, device="cuda")
    L.check(L.lib.mvf_ce_loss(d.P(d.out["scores"]), d.P(lab), clips, classes, d.P(dsc), d.P(part), d.P(loss), None), "mvf_ce_loss")
    d.bwd(dsc)
    got = d.host()
    ref = tn.forward(feat_d.float().cpu().numpy(), T, fc_w, fc_b, scales, table)
    ref_loss, ref_ds = tn.ce_loss(ref["scores"], labels)
    g = tn.backward(ref_ds, ref, T, fc_w, scales, table, hw)
    e = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-300))  # noqa: E731
    errs = dict(loss=abs(float(loss) - ref_loss) / abs(ref_loss), scores=e(got["scores"], ref["scores"]), dfc_w=e(got["dfc_w"], g["dfc_w"]),
                dfc_b=e(got["dfc_b"], g["dfc_b"]), dfeat=e(got["dfeat"], g["dfeat"]))
    for name, j in (("dw1", 0), ("db1", 1), ("dw2", 2), ("db2", 3)):
        errs[name] = max(e(got["dscales"][si][j], g["dscales"][si][j]) for si in range(len(scales)))
    print("end to end %s T=%d c=%d classes=%d: " % (kind, T, c, classes) + "  ".join("%s %.3g" % kv for kv in errs.items()))
    return errs


@pytest.mark.parametrize("name", ["trn8", "ms3", "ms8c64"])
def test_end_to_end_on_the_reference_cases(name):
    """The reference's own heads (fixture): the device's scores against the REFERENCE's fp64 scores, and loss / gradients against the fp64 chain."""
    _table_from_choices, _weights = tn.table_from_choices, tn.fixture_weights
    golden = np.load(os.path.join(HERE, "golden", "trn_cases.npz"))
    kind, T, classes, cin = golden[name + "/config"].tolist()
    T, classes, cin = int(T), int(classes), int(cin)
    _, fc_w, fc_b, scales = _weights(golden, name)
    table = _table_from_choices(kind, T, golden[name + "/choices"])
    feat = golden[name + "/feat"]
    nhwc = np.ascontiguousarray(feat.transpose(0, 2, 3, 1).reshape(feat.shape[0], 4, cin))
    labels = np.arange(3, dtype=np.int64) % classes
    errs = _end_to_end(kind, T, classes, cin, nhwc, fc_w, fc_b, scales, table, labels)
    assert errs["loss"] <= LOSS_BOUND
    assert all(v <= HEAD_BOUND for v in errs.values()), errs
    # against the reference's recorded scores themselves
    d = Device(kind, 3, T, 4, cin, classes, F32, fc_w.astype(np.float32), fc_b.astype(np.float32), [tuple(a.astype(np.float32) for a in sc) for sc in scales], table, None)
    d.fwd(torch.from_numpy(nhwc).cuda())
    want = golden[name + "/scores"]
    assert np.abs(d.host()["scores"] - want).max() <= HEAD_BOUND * np.abs(want).max()


@pytest.mark.parametrize("kind", ["TRN", "TRNmultiscale"])
def test_end_to_end_on_a_random_case(kind):
    case = (kind, 3, 8, 49, 64, 174, BF16, 0.0)
    d, feat, feat_d, q = _setup(case, seed=1)
    labels = np.array([0, 173, 80], dtype=np.int64)
    errs = _end_to_end(kind, 8, 174, 64, feat, *(np.float64(q["fc_w"]), np.float64(q["fc_b"])), [tuple(np.float64(a) for a in sc) for sc in q["scales"]], q["table"],
                       labels, dtype=BF16)
    assert errs["loss"] <= LOSS_BOUND
    assert all(v <= (2.0 ** -8 if k == "dfeat" else HEAD_BOUND) for k, v in errs.items()), errs


# ------------------------------------------------------------------------------------------------ the train engine
_VALS = {}
CLASSES, T_ENG = 7, 4


def _model(kind=None, seed=0, dropout=0.0, loss_cls=None):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, T_ENG, num_classes=CLASSES, dropout_ratio=dropout)
    if kind is not None:
        cfg["cls_head"]["consensus_cfg"] = dict(type=kind, num_frames=T_ENG)
    if loss_cls is not None:
        cfg["cls_head"]["loss_cls"] = loss_cls
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    sd = m.state_dict()
    key = (kind, seed)
    if key not in _VALS:
        _VALS[key] = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()}, seed=seed)
    m.load_state_dict({k: torch.from_numpy(_VALS[key]["r50/" + k]) for k in sd})
    return m.cuda()


def _clips(b=2, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    imgs = torch.randn(b, T_ENG, 3, 32, 32, device="cuda", generator=gen)
    hot = torch.rand(b, CLASSES, device="cuda", generator=gen) < 0.3
    hot[:, 1] = True
    return imgs, hot, torch.randint(0, CLASSES, (b, 1), device="cuda", generator=gen)


def _head_arrays(m):
    """(fc_w, fc_b, scales) of the model's head as fp64 host copies (the parameters BEFORE a step)."""
    h = m.cls_head
    n = lambda p: p.detach().cpu().double().numpy().copy()  # noqa: E731
    return n(h.new_fc.weight), n(h.new_fc.bias), [(n(a.weight), n(a.bias), n(b_.weight), n(b_.bias)) for a, b_ in h.segmental_consensus.scale_layers()]


def _head_params(m):
    return {k: v.detach().clone() for k, v in m.cls_head.state_dict().items()}


@pytest.mark.parametrize("use_plan", [False, True], ids=["eager", "plans_on"])
def test_each_step_computes_with_its_own_draw(use_plan):
    """Two consecutive train_steps with different draws: the scores each step left match the restatement with that step's table (and not the other's), with launch
    plans switched on as well -- relation-head steps run eagerly (no plan is recorded), so the table cannot be frozen into one."""
    imgs, _, labels = _clips()
    m = _model("TRNmultiscale").train()
    eng = m.train_engine(dtype=BF16)
    eng.use_plan, eng.plan_warmup = use_plan, 0
    np.random.seed(78)               # (three draws that differ as SETS of relations: the same set in another order is the same sum)
    tables, scores, want = [], [], []
    for step in range(3):
        fc_w, fc_b, scales = _head_arrays(m)
        eng.train_step(imgs, labels)
        torch.cuda.synchronize()
        table = eng._relation_table[0].cpu().numpy().reshape(-1, 1 + T_ENG)
        pooled = eng._bufs[("pooled", (2 * T_ENG, 2048), F32)].cpu().numpy()
        f, _ = tn.stage_fc(pooled, fc_w, fc_b)
        want.append(lambda tb, f=f, scales=scales: tn.stage_scores(np.maximum(tn.stage_hidden(f, scales, tb, 2, T_ENG)[0], 0.0), scales, tb, T_ENG)[0])
        tables.append(table)
        scores.append(eng._bufs[("scores", (2, CLASSES), F32)].cpu().numpy().copy())
    sets = [frozenset(map(tuple, tb.tolist())) for tb in tables]
    assert tables[0].shape == (7, 5) and len(set(sets)) == 3
    for i in range(3):
        own, other = want[i](tables[i]), want[i](tables[(i + 1) % 3])
        err = np.abs(scores[i] - own).max() / np.abs(own).max()
        print("step %d: scores vs the restatement with its own table %.3g, with the next step's %.3g" % (i, err, np.abs(scores[i] - other).max() / np.abs(own).max()))
        assert err <= HEAD_BOUND < np.abs(scores[i] - other).max() / np.abs(own).max()
    assert not getattr(eng, "_plans", None)                                 # nothing was recorded
    # an explicit table replaces the draw
    eng.relations = tables[0]
    eng.train_step(imgs, labels)
    assert np.array_equal(eng._relation_table[0].cpu().numpy().reshape(-1, 1 + T_ENG), tables[0])
    with pytest.raises(ValueError, match="num_frames=4"):
        eng.train_step(torch.zeros(2, 8, 3, 32, 32, device="cuda"), labels)


def _moved(before, m):
    after = m.cls_head.state_dict()
    return {k: not torch.equal(after[k], v) for k, v in before.items()}


@pytest.mark.parametrize("kind", ["TRN", "TRNmultiscale"])
def test_the_step_composes_with_the_label_kinds(kind):
    """One train_step each with integer labels, label smoothing + Mixup, a BCE multi-hot matrix and distillation from an average-head teacher: a finite loss,
    and every new parameter moves."""
    from mvfnet_amd.blending import MixupBlending
    from mvfnet_amd.distill import KnowledgeDistillation
    imgs, hot, labels = _clips()
    np.random.seed(5)
    m = _model(kind).train()
    eng = m.train_engine(dtype=BF16, lr=0.05)
    assert eng.trn is not None and eng.trn["kind"] == kind and eng._plan_key(imgs, labels) is None
    n_head = sum(p.numel() for p in m.cls_head.parameters())
    assert eng.n_params == sum(p.numel() for p in m.parameters()) and n_head > 256 * 2048      # the relation MLPs are in the flat store
    before = _head_params(m)
    loss = eng.train_step(imgs, labels)
    assert torch.isfinite(loss).all() and all(_moved(before, m).values()), _moved(before, m)
    eng.blending, eng.label_smooth_eps = MixupBlending(alpha=0.8, seed=5), 0.1
    before = _head_params(m)
    loss = eng.train_step(imgs, labels)
    assert torch.isfinite(loss).all() and all(_moved(before, m).values())
    eng.blending, eng.label_smooth_eps = None, 0.0
    teacher = _model(None, seed=1).eval()
    eng.distill = KnowledgeDistillation(teacher, temperature=4.0, alpha=0.5)
    before = _head_params(m)
    loss = eng.train_step(imgs, labels)
    terms = eng.distill_terms()
    assert torch.isfinite(loss).all() and terms["loss_kd"] > 0.0 and all(_moved(before, m).values())
    mb = _model(kind, loss_cls=dict(type="BCELossWithLogits")).train()
    engb = mb.train_engine(dtype=BF16, lr=0.05)
    assert engb.bce is not None and engb.trn is not None
    before = _head_params(mb)
    loss = engb.train_step(imgs, hot.float())
    assert torch.isfinite(loss).all() and all(_moved(before, mb).values())
    # eval mode: the head scores through the relation path, drawing as the reference does; an explicit table fixes it
    m.eval()
    table = rel.draw_relation_table(kind, T_ENG)
    feat = m.extract_feat(imgs.reshape(-1, 3, 32, 32))
    a, b_ = m.cls_head(feat, T_ENG, relations=table), m.cls_head(feat, T_ENG, relations=table)
    assert a.shape == (2, CLASSES) and torch.isfinite(a).all() and torch.equal(a, b_)
    out = m(imgs, None, return_loss=False)
    assert out.shape == (2, CLASSES) and np.isfinite(out).all()


def test_the_engines_dropout_mask_reaches_the_relation_head():
    """With dropout the engine draws its per-frame (frames, channels) mask per step and hands it to mvf_trn_head_fwd / mvf_trn_head_bwd: the pooled features the head stored are exactly zero wherever the step's mask is, the same torch seed draws the same mask,
    another seed another mask, other scores and other gradients; a train_step moves every new parameter."""
    imgs, _, labels = _clips()
    m = _model("TRNmultiscale", dropout=0.5).train()
    eng = m.train_engine(dtype=BF16, lr=0.05)
    eng.dropout = 0.5
    np.random.seed(9)
    eng.relations = rel.draw_relation_table("TRNmultiscale", T_ENG)
    runs = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        loss = eng.forward(imgs, labels)
        mask = eng.saved["mask"]
        assert mask is not None and tuple(mask.shape) == (2 * T_ENG, 2048) and 0.3 < float((mask == 0).float().mean()) < 0.7
        pooled = eng.saved["pooled"].clone()
        assert bool((pooled[mask == 0] == 0).all())
        scores = eng.saved["scores"].clone()
        eng.backward()
        torch.cuda.synchronize()
        g = eng.flat_grads.clone()
        assert torch.isfinite(loss).all() and torch.isfinite(g).all()
        runs.append((scores, g, mask.clone()))
    assert torch.equal(runs[0][2], runs[1][2]), "the same seed draws the same mask"
    # (the scores of the two same-mask forwards are NOT compared: this 2-clip batch-statistics network does not repeat its features bit for bit from one
    # forward to the next, and amplifies the difference; that the head itself repeats its bits is test_every_stage_within_its_derived_bound's second run)
    assert not torch.equal(runs[0][2], runs[2][2]) and not torch.equal(runs[0][0], runs[2][0]) and not torch.equal(runs[0][1], runs[2][1])
    before = _head_params(m)
    assert torch.isfinite(eng.train_step(imgs, labels)).all() and all(_moved(before, m).values())


def test_the_guard_skips_a_poisoned_step():
    imgs, _, labels = _clips()
    m = _model("TRNmultiscale").train()
    eng = m.train_engine(dtype=BF16)
    eng.enable_step_guard()
    eng.train_step(imgs, labels)
    assert not eng.guard_state()["skipped_last"]
    with torch.no_grad():
        m.cls_head.new_fc.weight[3, 5] = float("nan")
    before = _head_params(m)
    eng.train_step(imgs, labels)
    st = eng.guard_state()
    assert st["skipped_last"] and st["skipped"] == 1
    after = m.cls_head.state_dict()
    for k, v in before.items():
        if k != "new_fc.weight":
            assert torch.equal(after[k], v), k                              # every relation parameter bit-equal
    assert torch.equal(torch.isnan(after["new_fc.weight"]), torch.isnan(before["new_fc.weight"]))


def test_the_default_head_steps_as_it_did():
    """A default-head engine allocates nothing of the relation head, records the plan it always did (the average head's two entry points, a 12-entry key), and
    the planned steps leave the flat parameters of the eager steps bit for bit."""
    imgs, _, labels = _clips()
    sums = {}
    for use_plan in (False, True):
        m = _model(None).train()
        eng = m.train_engine(dtype=BF16)
        eng.use_plan = use_plan
        assert eng.trn is None and eng.relations is None
        for _ in range(5):
            eng.train_step(imgs, labels)
        torch.cuda.synchronize()
        sums[use_plan] = (eng.flat_params.double().sum().item(), eng.flat_params.clone())
        assert not any(str(k[0]).startswith("trn_") or k[0] == "relation_table" for k in eng._bufs)
        if use_plan:
            plans = [s["plan"] for s in eng._plans.values()]
            assert len(plans) == 1 and plans[0] is not None and all(len(key) == 12 for key in eng._plans)
            names = list(plans[0].names)
            print("default head: plan ops %d" % plans[0].n_ops)
            assert names.count("mvf_head_train_fwd") == 1 and names.count("mvf_head_train_bwd") == 1 and not any(n.startswith("mvf_trn_") for n in names)
            # the op count against one computed here: a second, independently built default-head engine, stepped eagerly and then recorded by hand
            m2 = _model(None).train()
            eng2 = m2.train_engine(dtype=BF16)
            eng2.use_plan = False
            for _ in range(2):
                eng2.train_step(imgs, labels)
            _, rec = eng2._record_step(imgs, labels, eng2._step_tensors(imgs, labels))
            assert rec is not None and rec.n_ops == plans[0].n_ops and list(rec.names) == names
    assert sums[True][0] == sums[False][0] and torch.equal(sums[True][1], sums[False][1])


# ------------------------------------------------------------------------------------------------ the loss dispatcher (heads/loss_calls.py)
HEAD_ENTRY_POINTS = {"mvf_head_train_fwd", "mvf_head_train_fwd_soft", "mvf_head_train_fwd_bce", "mvf_head_train_fwd_focal", "mvf_trn_head_fwd", "mvf_ce_loss",
                     "mvf_ce_loss_soft", "mvf_bce_loss", "mvf_focal_loss"}
DISPATCH = {"default": (None, None, 0.0, ["mvf_head_train_fwd"]),
            "smoothing": (None, None, 0.1, ["mvf_head_train_fwd_soft"]),
            "bce": (None, dict(type="BCELossWithLogits"), 0.0, ["mvf_head_train_fwd_bce"]),
            "focal": (None, dict(type="SigmoidFocalLoss"), 0.0, ["mvf_head_train_fwd_focal"]),
            "trn": ("TRNmultiscale", None, 0.0, ["mvf_trn_head_fwd", "mvf_ce_loss"])}


@pytest.mark.parametrize("config", list(DISPATCH))
def test_the_step_looks_its_head_entry_point_up_on_the_engines_library_object(config):
    """One eager forward per head configuration with the engine's library handle (eng.lib) replaced by a names-only stand-in: the step looks up exactly the
    head entry point(s) it always called, on its own handle at call time -- which is what launch_plan.recording() relies on to record the head -- and
    heads/loss_calls.py looks nothing up through _lib.lib (replaced by a second stand-in for the duration)."""
    import mvfnet_amd._lib as L
    from mvfnet_amd.heads import loss_calls
    kind, loss_cls, eps, want = DISPATCH[config]
    imgs, hot, labels = _clips()
    np.random.seed(5)
    m = _model(kind, loss_cls=loss_cls).train()
    eng = m.train_engine(dtype=BF16)
    eng.use_plan, eng.label_smooth_eps = False, eps
    assert "lib" not in vars(loss_calls)
    on_module = []
    real_l = L.lib
    L.lib = NamesOf(real_l, on_module)
    try:
        with library_names(eng) as on_engine:
            loss = eng.forward(imgs, hot.float() if loss_cls is not None else labels)
    finally:
        L.lib = real_l
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert [n for n in on_engine if n in HEAD_ENTRY_POINTS] == want, [n for n in on_engine if n in HEAD_ENTRY_POINTS]
    assert (eps > 0.0) == ("mvf_soft_targets" in on_engine)
    assert not [n for n in on_module if n in HEAD_ENTRY_POINTS or n == "mvf_soft_targets"], on_module
