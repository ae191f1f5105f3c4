"""CPU: tests/wgrad_ref.py (the fp64 reference tests/test_wgrad_families_gpu.py compares the weight-gradient kernels with) against
torch.nn.grad.conv2d_weight in fp64, and its stem view against autograd of F.conv2d(x, w, stride=2, padding=3): stride 1 and 2, k = 1 / 3 / 7, odd maps,
the split operand and pixel pitches wider than the channel count.  Bound 1e-12: both sides sum the same fp64 products, in another order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as R
from helpers import rel_err

# (n, h, w, cin, cout, k, stride, pad)
CASES = [(2, 5, 7, 8, 12, 1, 1, 0), (3, 6, 5, 4, 8, 1, 2, 0), (2, 9, 7, 8, 4, 3, 1, 1), (2, 13, 11, 4, 8, 3, 2, 1), (1, 4, 4, 12, 4, 3, 1, 1),
         (2, 17, 15, 4, 8, 7, 2, 3), (1, 9, 10, 3, 5, 7, 1, 3), (2, 8, 8, 4, 4, 3, 2, 0)]


def _torch_ref(x_nhwc, dz_nhwc, cin, cout, k, stride, pad):
    x = torch.from_numpy(x_nhwc).permute(0, 3, 1, 2).contiguous()
    dz = torch.from_numpy(dz_nhwc).permute(0, 3, 1, 2).contiguous()
    return torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dz, stride=stride, padding=pad).numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_c%d_o%d_k%d_s%d_p%d" % c)
@pytest.mark.parametrize("pitch_extra", [0, 5])
def test_reference_equals_conv2d_weight_in_fp64(case, pitch_extra):
    n, h, w, cin, cout, k, stride, pad = case
    rng = np.random.default_rng(sum(case) + pitch_extra)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xps = cin + pitch_extra
    buf = rng.standard_normal((n, h, w, xps))                    # (the columns past cin hold other values: a pitch mistake shows)
    dz = rng.standard_normal((n, ho, wo, cout))
    dw, absref = R.wgrad(dz, buf, n, h, w, cin, k, k, stride, pad, x_pix_stride=xps)
    ref = _torch_ref(buf[..., :cin].copy(), dz, cin, cout, k, stride, pad)
    assert dw.shape == ref.shape == (cout, cin, k, k)
    assert rel_err(dw, ref) < 1e-12
    assert (absref >= np.abs(dw) - 1e-12).all() and absref.shape == dw.shape
    ref_abs = _torch_ref(np.abs(buf[..., :cin]), np.abs(dz), cin, cout, k, stride, pad)
    assert rel_err(absref, ref_abs) < 1e-12


@pytest.mark.parametrize("cin,split_c,xps,x2ps", [(12, 4, 12, 4), (12, 8, 16, 11), (8, 4, 9, 7)])
def test_split_operand_reads_x2_below_split_c_and_x_at_the_same_column_above(cin, split_c, xps, x2ps):
    n, h, w, cout = 2, 5, 3, 8
    rng = np.random.default_rng(cin + split_c + xps)
    x = rng.standard_normal((n, h, w, xps))
    x2 = rng.standard_normal((n, h, w, x2ps))
    dz = rng.standard_normal((n, h, w, cout))
    dw, _ = R.wgrad(dz, x, n, h, w, cin, 1, 1, 1, 0, x_pix_stride=xps, x2=x2, split_c=split_c, x2_pix_stride=x2ps)
    full = np.concatenate([x2[..., :split_c], x[..., split_c:cin]], axis=3)
    assert rel_err(dw, _torch_ref(np.ascontiguousarray(full), dz, cin, cout, 1, 1, 0)) < 1e-12
    # ... and it is not what x alone gives
    assert rel_err(dw, _torch_ref(np.ascontiguousarray(x[..., :cin]), dz, cin, cout, 1, 1, 0)) > 1e-2


@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 10, 14), (3, 6, 12)], ids=str)
def test_stem_view_equals_autograd_of_the_7x7_stride_2_conv(shape):
    n, h, w = shape
    g = torch.Generator().manual_seed(h * 7 + w)
    x = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    ho, wo = h // 2, w // 2
    dy = torch.randn(n, 64, ho, wo, generator=g, dtype=torch.float64)
    wt = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wt, stride=2, padding=3).backward(dy)
    hp, wp = h + 6, w + 8
    rng = np.random.default_rng(n + h + w)
    xp = np.zeros((n, hp, wp, 4))
    xp[:, 3:3 + h, 3:3 + w, :3] = x.permute(0, 2, 3, 1).numpy()
    xp[:, :, :, 3] = rng.standard_normal((n, hp, wp))           # the fourth packed channel and the columns only the eighth packed tap reads are dropped
    xp[:, :, w + 6:, :] = rng.standard_normal((n, hp, 2, 4))
    dz = dy.permute(0, 2, 3, 1).contiguous().numpy()
    dw, absref = R.wgrad_stem(dz, xp, n, hp, wp)
    assert dw.shape == (64, 3, 7, 7) and absref.shape == dw.shape
    assert rel_err(dw, wt.grad.numpy()) < 1e-12


def test_pitch_smaller_than_needed_is_refused():
    with pytest.raises(AssertionError):
        R.wgrad(np.zeros((1, 2, 2, 4)), np.zeros((1, 2, 2, 4)), 1, 2, 2, 8, 1, 1, 1, 0, x_pix_stride=8)
