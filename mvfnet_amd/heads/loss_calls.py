"""Which loss entry point of the train head a step calls, and with which arguments: one place for TrainEngine._forward (the fused forms),
TrainEngine._trn_head_forward and TSNClsHead.loss (the stand-alone forms).

Every function takes the library handle from its caller and looks the entry point up on it at call time.  The train engine passes its own handle
(`self.lib`: the loaded library, or for the one engine inside launch_plan.recording() the RecordingLib that also records the call; tests install a
stand-in the same way), TSNClsHead.loss the loaded library.  This module therefore imports no library of its own.
"""
import ctypes as C

from .._lib import check      # (the error text comes from the loaded library; no entry point is looked up through _lib here)


def _p(t):
    return t.data_ptr() if t is not None else None


def loss_kind(bce, focal, soft):
    """(stand-alone entry point, fused entry point, the arguments between the labels and the outputs).  bce / focal: TSNClsHead.bce_settings /
    focal_settings (None = off; focal wins); soft: the labels are a (B, classes) target matrix, not integers."""
    if focal is not None:
        class_weight, prm = focal
        return "mvf_focal_loss", "mvf_head_train_fwd_focal", (_p(class_weight), prm)
    if bce is not None:
        pos_weight, thr, sum_classes = bce
        return "mvf_bce_loss", "mvf_head_train_fwd_bce", (_p(pos_weight), C.c_float(thr), sum_classes)
    if soft:
        return "mvf_ce_loss_soft", "mvf_head_train_fwd_soft", ()
    return "mvf_ce_loss", "mvf_head_train_fwd", ()


def stand_alone_loss(lib, kind, scores, targets_or_labels, b, classes, dscores, loss_part, loss, stream):
    name, _, mid = kind
    check(getattr(lib, name)(_p(scores), _p(targets_or_labels), b, classes, *mid, _p(dscores), _p(loss_part), _p(loss), stream), name)


def fused_head_loss(lib, kind, feat, b, t, hw, c, fc_w, fc_b, classes, targets_or_labels, mask, pooled, scores, dscores, loss_part, loss, dt, stream):
    _, name, mid = kind
    check(getattr(lib, name)(_p(feat), b, t, hw, c, _p(fc_w), _p(fc_b), classes, _p(targets_or_labels), _p(mask), *mid, _p(pooled), _p(scores),
                             _p(dscores), _p(loss_part), _p(loss), dt, stream), name)


def targets_for(lib, lab, rows, wts, b, classes, eps, out, stream):
    """The (b, classes) target matrix of integer labels `lab`: one-hot, smoothed by eps, blended by the step's table (rows, wts; None = no blending)."""
    check(lib.mvf_soft_targets(_p(lab), _p(rows), _p(wts), b, classes, C.c_float(eps), _p(out), stream), "mvf_soft_targets")
    return out
