"""CPU: the temporal-relation head (TSNClsHead with consensus 'TRN' / 'TRNmultiscale') -- everything that needs no device: the module tree against the
reference's (tests/golden/trn_cases.npz, made by tests/golden/make_trn_golden.py from the reference's own classes in fp64), the relation draw after
np.random.seed(k) against the recorded np.random.choice results, the table layout and check_relation_table, every refusal, the default head's unchanged
module tree and plan key, the fp64 restatement (trn_numpy.py) against the fixture's scores and autograd gradients, and the entry points' argument checks
(from host addresses that are never read)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import trn_numpy as tn
from mvfnet_amd import synth
from mvfnet_amd.heads import TSNClsHead
from mvfnet_amd.heads import relation as rel

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "trn_cases.npz"))


def _case(golden, name):
    kind, T, classes, cin = golden[name + "/config"].tolist()
    return kind, int(T), int(classes), int(cin), int(golden[name + "/seed"])


def _head(kind, T, classes, cin, **kw):
    return TSNClsHead(spatial_size=-1, consensus_cfg=dict(type=kind, num_frames=T), dropout_ratio=0, in_channels=cin, num_classes=classes, **kw)


_weights, _table_from_choices = tn.fixture_weights, tn.table_from_choices


@pytest.mark.parametrize("name", ["trn8", "ms3", "ms8c64"])
def test_module_tree_and_state_dict_equal_the_reference(golden, name):
    kind, T, classes, cin, _ = _case(golden, name)
    head = _head(kind, T, classes, cin)
    sd = head.state_dict()
    assert list(sd.keys()) == golden[name + "/keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == golden[name + "/shapes"].tolist()
    assert tuple(head.new_fc.weight.shape) == (256, cin) and head.consensus_type == kind and head.is_relation_head
    if kind == "TRN":
        assert tuple(sd["segmental_consensus.classifier.1.weight"].shape) == (512, T * 256)
        assert tuple(sd["segmental_consensus.classifier.3.weight"].shape) == (classes, 512)
    else:
        for i, s in enumerate(range(T, 1, -1)):
            assert tuple(sd["segmental_consensus.fc_fusion_scales.%d.1.weight" % i].shape) == (256, s * 256)
            assert tuple(sd["segmental_consensus.fc_fusion_scales.%d.3.weight" % i].shape) == (classes, 256)


def test_init_weights_touches_new_fc_only():
    head = _head("TRNmultiscale", 4, 5, 32)
    before = {k: v.clone() for k, v in head.state_dict().items()}
    head.init_std = 0.5
    head.init_weights()
    for k, v in head.state_dict().items():
        if not k.startswith("new_fc."):
            assert torch.equal(v, before[k]), k            # nn.Linear's default init stays, as in the reference
    assert not torch.equal(head.new_fc.weight, before["new_fc.weight"])
    assert not head.new_fc.bias.any() and 0.3 < float(head.new_fc.weight.detach().std()) < 0.7


@pytest.mark.parametrize("name", ["trn8", "ms3", "ms8c64"])
def test_the_draw_after_a_seed_is_the_reference_draw(golden, name):
    kind, T, _, _, seed = _case(golden, name)
    want = golden[name + "/choices"]
    drawn = []
    np.random.seed(seed)
    table = rel.draw_relation_table(kind, T, choices=drawn)
    assert len(drawn) == want.shape[0] and all(np.array_equal(a, b) for a, b in zip(drawn, want))
    assert np.array_equal(table, _table_from_choices(kind, T, want)) and table.dtype == np.int32
    assert np.array_equal(rel.check_relation_table(table, kind, T), table)
    np.random.seed(seed + 1)
    if want.shape[0] > 1:
        assert not np.array_equal(rel.draw_relation_table(kind, T), table)          # numpy's global generator, once per forward


@pytest.mark.parametrize("T,rows", [(2, 1), (3, 4), (4, 7), (8, 19), (16, 43)])
def test_rows_and_layout(T, rows):
    np.random.seed(T)
    table = rel.draw_relation_table("TRNmultiscale", T)
    assert table.shape == (rows, 1 + T) and rel.relation_rows("TRNmultiscale", T) == rows and rel.relation_rows("TRN", T) == 1
    assert table[0].tolist() == [0] + list(range(T))
    assert rel.draw_relation_table("TRN", T).tolist() == [[0] + list(range(T))]
    want_scale = [0] + [i for i in range(1, T - 1) for _ in range(3)]
    assert table[:, 0].tolist() == want_scale
    for row in table.tolist():
        s = T - row[0]
        assert row[1 + s:] == [-1] * (T - s) and sorted(set(row[1:1 + s])) == row[1:1 + s] and 0 <= row[1] and row[s] < T
    rel.check_relation_table(table, "TRNmultiscale", T)


def test_check_relation_table_refusals():
    np.random.seed(5)
    T = 4
    good = rel.draw_relation_table("TRNmultiscale", T)

    def bad(edit, kind="TRNmultiscale", match="relation table"):
        t = good.copy()
        t = edit(t)
        with pytest.raises(ValueError, match=match):
            rel.check_relation_table(t, kind, T)

    def setv(r, c, v):
        def e(t):
            t[r, c] = v
            return t
        return e
    bad(lambda t: t.astype(np.int64))
    bad(lambda t: t[:, :-1])
    bad(lambda t: t.reshape(-1))
    bad(lambda t: t[:0])
    bad(setv(1, 0, 5))                        # scale index outside the head's scales
    bad(setv(1, 0, -1))
    bad(setv(0, 0, 1))                        # the first row is the T-frame relation
    bad(setv(2, 0, 0))                        # ... and only the first
    bad(setv(1, 1, T))                        # frame outside [0, T)
    bad(setv(1, 1, -1))
    bad(lambda t: np.concatenate([t[:1], t[1:2], t[1:2], t[3:]]))          # the same relation twice
    bad(setv(1, T, 0))                        # padding must be -1
    bad(lambda t: np.concatenate([t, t[-1:]]))                             # more rows than the draw makes

    def swap(t):
        t[1, 1], t[1, 2] = t[1, 2], t[1, 1]
        return t
    bad(swap)                                 # frames ascend
    bad(lambda t: t, kind="TRN")              # 'TRN' has its one row
    with pytest.raises(ValueError):
        rel.check_relation_table(good, "avg", T)
    with pytest.raises(ValueError):
        rel.check_relation_table(good, "TRNmultiscale", 5)
    # rows of scales >= 1 in another order, and a scale without a row, are tables the head runs
    rel.check_relation_table(np.concatenate([good[:1], good[1:][::-1]]), "TRNmultiscale", T)
    rel.check_relation_table(good[:4], "TRNmultiscale", T)


def test_constructor_refusals():
    for cfg in (dict(type="TRN"), dict(type="TRN", num_frames=1), dict(type="TRN", num_frames=17), dict(type="TRNmultiscale", num_frames=2.0),
                dict(type="TRN", num_frames=True), dict(type="TRN", num_frames=8, dim=1), dict(type="TRNmultiscale", num_frames=8, subsample=3)):
        with pytest.raises(ValueError):
            TSNClsHead(consensus_cfg=cfg, in_channels=32, num_classes=5)
    for kw in (dict(fcn_testing=True), dict(extract_feat=True)):
        with pytest.raises(ValueError, match="relation head"):
            TSNClsHead(consensus_cfg=dict(type="TRN", num_frames=4), in_channels=32, num_classes=5, **kw)
    with pytest.raises(NotImplementedError):
        TSNClsHead(consensus_cfg=dict(type="max", dim=1), in_channels=32, num_classes=5)
    assert TSNClsHead(consensus_cfg=dict(type="TRNmultiscale", num_frames=16), in_channels=32, num_classes=5).num_frames == 16      # 43 relations
    head = _head("TRN", 4, 5, 32).eval()
    with pytest.raises(ValueError, match="num_frames=4"):
        head(torch.zeros(6, 32, 1, 1), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(torch.zeros(8, 32, 1, 1), 4)
    with pytest.raises(ValueError, match="relations="):
        TSNClsHead(in_channels=32, num_classes=5).eval()(torch.zeros(8, 32, 1, 1), 4, relations=np.zeros((1, 5), np.int32))


def test_recognizer_refusals():
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=5)
    cfg["cls_head"]["consensus_cfg"] = dict(type="TRNmultiscale", num_frames=8)
    with pytest.raises(ValueError, match="n_segment=4"):
        mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=5)
    cfg["cls_head"]["consensus_cfg"] = dict(type="TRN", num_frames=4)
    cfg["fcn_testing"] = True
    with pytest.raises(ValueError, match="fcn_testing"):
        mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    cfg["fcn_testing"] = False
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    assert [k for k in m.state_dict() if k.startswith("cls_head.")] == ["cls_head.segmental_consensus.classifier.%d.%s" % (i, p) for i in (1, 3) for p in ("weight", "bias")] + \
        ["cls_head.new_fc.weight", "cls_head.new_fc.bias"]


def _bare_engine(monkeypatch):
    """A TrainEngine that never ran __init__ (which needs a device): only what _plan_key reads."""
    from mvfnet_amd.train_engine import TrainEngine
    eng = object.__new__(TrainEngine)
    eng.num_classes, eng.keep_io, eng.input_pipeline, eng._nbt_mods = 5, False, None, []
    eng.erasing = eng.distill = eng.blending = eng.randaug = None
    eng.label_smooth_eps, eng.dropout, eng.bce, eng.focal = 0.0, 0.5, None, None
    eng.model = torch.nn.Linear(2, 2)
    eng._ddp_active = lambda: False
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    return eng


def test_the_default_head_is_what_it_was(monkeypatch):
    head = TSNClsHead(in_channels=32, num_classes=5)
    assert list(head.state_dict().keys()) == ["new_fc.weight", "new_fc.bias"] and [n for n, _ in head.named_children()] == ["dropout", "new_fc"]
    assert head.consensus_type == "avg" and not head.is_relation_head and not hasattr(head, "segmental_consensus")
    eng = _bare_engine(monkeypatch)
    eng.use_plan = True
    imgs, labels = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 1, dtype=torch.int64)
    key = eng._plan_key(imgs, labels)
    assert len(key) == 12 and key[-3:] == (False, 0.0, False)                 # no consensus entry joins the average head's key
    assert "trn" not in eng._switch_names and "relations" not in eng._switch_names
    eng.trn = dict(kind="TRN", t=4)
    assert eng._plan_key(imgs, labels) is None                                 # relation-head steps run eagerly
    with pytest.raises(ValueError, match="num_frames=4"):
        eng._relation_refusals(torch.zeros(2, 8, 3, 8, 8))


@pytest.mark.parametrize("name", ["trn8", "ms3", "ms8c64"])
def test_the_restatement_reproduces_the_reference(golden, name):
    """Both sides are fp64 and differ only in summation order: scores to 1e-12 relative, every gradient to 1e-10."""
    kind, T, classes, cin, seed = _case(golden, name)
    vals, fc_w, fc_b, scales = _weights(golden, name)
    table = _table_from_choices(kind, T, golden[name + "/choices"])
    feat = golden[name + "/feat"].astype(np.float64)                          # (clips * T, c, 2, 2)
    nhwc = feat.transpose(0, 2, 3, 1).reshape(feat.shape[0], 4, cin)
    out = tn.forward(nhwc, T, fc_w, fc_b, scales, table)
    want = golden[name + "/scores"]
    assert np.abs(out["scores"] - want).max() <= 1e-12 * np.abs(want).max()
    g = tn.backward(golden[name + "/dscores"], out, T, fc_w, scales, table, 4)
    rel_err = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)  # noqa: E731
    dfeat = g["dfeat"].reshape(feat.shape[0], 2, 2, cin).transpose(0, 3, 1, 2)
    assert rel_err(dfeat, golden[name + "/dfeat"]) <= 1e-10
    pre = "segmental_consensus."
    stems = [pre + "classifier."] if kind == "TRN" else [pre + "fc_fusion_scales.%d." % i for i in range(T - 1)]
    mine = {"new_fc.weight": g["dfc_w"], "new_fc.bias": g["dfc_b"]}
    for s, (dw1, db1, dw2, db2) in zip(stems, g["dscales"]):
        mine.update({s + "1.weight": dw1, s + "1.bias": db1, s + "3.weight": dw2, s + "3.bias": db2})
    assert sorted(mine) == sorted(vals)
    checked = 0
    for k, v in mine.items():
        if name + "/grad/" + k in golden.files:
            assert rel_err(v, golden[name + "/grad/" + k]) <= 1e-10, k
        else:
            dot, mag, dot2 = golden[name + "/gradsum/" + k]
            probe2 = synth.synth_tensor("probe/second/" + name + "/" + k, v.shape, "normal", 1.0, 0.0, 0).astype(np.float64)
            assert abs(np.vdot(v, probe2) - dot2) <= 1e-10 * mag, k
            rows = golden[name + "/gradrows/" + k]
            assert np.abs(v[[0, v.shape[0] // 2]] - rows).max() <= 1e-10 * max(np.abs(v).max(), 1e-300), k
            probe = synth.synth_tensor("probe/" + name + "/" + k, v.shape, "normal", 1.0, 0.0, 0).astype(np.float64)
            assert abs(np.abs(v).sum() - mag) <= 1e-10 * mag and abs(np.vdot(v, probe) - dot) <= 1e-10 * mag, k
        checked += 1
    assert checked == len(vals)
    # other relations give other scores: the table is what the head computes from
    if kind == "TRNmultiscale" and T > 3:
        other = table.copy()
        np.random.seed(seed + 100)
        other = rel.draw_relation_table(kind, T)
        assert not np.array_equal(other, table)
        assert np.abs(tn.forward(nhwc, T, fc_w, fc_b, scales, other)["scores"] - want).max() > 1e-6 * np.abs(want).max()


def test_bindings_and_argument_failures_need_no_device():
    """The three exports are declared, bound and refuse bad arguments before any launch; a refused call leaves an empty launch record."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    for n in ("mvf_trn_head_fwd", "mvf_trn_head_bwd", "mvf_trn_head_last_launch"):
        assert n in _lib.declared_symbols() and hasattr(lib, n)
    assert C.sizeof(_lib.TrnScale) == 64 and C.sizeof(_lib.TrnLaunchInfo) == 20 and _lib.TRN_MAX_FRAMES == rel.MAX_FRAMES == 16
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mvfnet_hip.h")).read()
    assert "#define MVF_TRN_MAX_FRAMES 16" in hdr and "5 launches whatever" in hdr and "7 launches whatever" in hdr
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    info = _lib.TrnLaunchInfo()

    def scales(n, hole=None):
        arr = (_lib.TrnScale * n)()
        for i in range(n):
            for k, _ in _lib.TrnScale._fields_:
                setattr(arr[i], k, None if k == hole else a.value)
        return arr

    def fwd(feat=a, clips=2, t=4, hw=1, c=8, w=a, fdim=8, sc=None, ns=3, hidden=8, classes=3, table=a, rows=7, pooled=a, f=a, h=a, hpart=a, scores=a, dtype=0):
        return lib.mvf_trn_head_fwd(feat, clips, t, hw, c, w, None, fdim, sc if sc is not None else scales(max(ns, 1)), ns, hidden, classes, table, rows, None,
                                    pooled, f, h, hpart, scores, dtype, None)

    def bwd(ds=a, clips=2, t=4, hw=1, c=8, ns=3, sc=None, rows=7, dh=a, dfeat=a, dtype=0):
        return lib.mvf_trn_head_bwd(ds, a, a, a, a, sc if sc is not None else scales(max(ns, 1)), ns, 8, 3, a, rows, None, clips, t, hw, c, 8, a, a, dh, a, a,
                                    dfeat, dtype, None)
    EINVAL, ESHAPE, EUNSUPPORTED = -1, -2, -5
    for want, kw in [(EINVAL, dict(feat=None)), (EINVAL, dict(w=None)), (EINVAL, dict(table=None)), (EINVAL, dict(pooled=None)), (EINVAL, dict(f=None)),
                     (EINVAL, dict(h=None)), (EINVAL, dict(hpart=None)), (EINVAL, dict(scores=None)), (EINVAL, dict(clips=0)), (EINVAL, dict(hw=0)), (EINVAL, dict(c=0)), (EINVAL, dict(fdim=0)),
                     (EINVAL, dict(hidden=0)), (EINVAL, dict(classes=0)), (EINVAL, dict(rows=0)), (EINVAL, dict(dtype=2)), (EINVAL, dict(ns=0)), (EINVAL, dict(ns=4)),
                     (EINVAL, dict(sc=scales(3, hole="w1"))), (EUNSUPPORTED, dict(t=1)), (EUNSUPPORTED, dict(t=17, ns=1)), (ESHAPE, dict(c=6)),
                     (ESHAPE, dict(clips=20000)), (ESHAPE, dict(rows=1025))]:
        info.launches = info.rows = 99
        assert fwd(**kw) == want, (kw, lib.mvf_last_error())
        assert b"trn_head_fwd" in lib.mvf_last_error()
        assert lib.mvf_trn_head_last_launch(C.byref(info)) == 0 and (info.entry, info.launches, info.rows) == (1, 0, 0)
    for want, kw in [(EINVAL, dict(ds=None)), (EINVAL, dict(dh=None)), (EINVAL, dict(dfeat=None)), (EINVAL, dict(sc=scales(3, hole="dw2"))), (EINVAL, dict(ns=0)),
                     (EUNSUPPORTED, dict(t=1)), (ESHAPE, dict(c=6)), (ESHAPE, dict(dfeat=C.c_void_p(a.value + 4)))]:
        info.launches = 99
        assert bwd(**kw) == want, (kw, lib.mvf_last_error())
        assert lib.mvf_trn_head_last_launch(C.byref(info)) == 0 and (info.entry, info.launches) == (2, 0)
    assert lib.mvf_trn_head_last_launch(None) == EINVAL
    assert all(v == 0.0 for v in host)
