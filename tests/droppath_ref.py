"""fp64 reference of drop path (stochastic depth) on a bottleneck's residual branch, written from the definition -- timm's drop_path(x, p, training,
scale_by_keep) applied after bn3: out = relu(s * bn3(conv3(a2)) + identity) with one scale s per image -- and from calculus, not from the kernels of
csrc/drop_path.hip.  numpy restatements of the two kernels (with what a test needs to bound an fp32 evaluation: `A`, the sum of the absolute values of the
expression's terms, as in bn_pool_ref), and a torch bottleneck in the dtype of its inputs whose every line but the residual one is the oracle's."""
import numpy as np

from bn_pool_ref import act_fwd, pack_bits, undecided, unpack_bits


def rows_of(row_scale, rows_per_image, m):
    """The per-image table spread over the m rows: image r // rows_per_image owns row r."""
    s = np.repeat(np.asarray(row_scale, dtype=np.float64), rows_per_image)
    assert s.shape == (m,), (s.shape, m)
    return s[:, None]


def apply_bits_rowscale(z, scale, shift, r, row_scale, rows_per_image, rscale=None, rshift=None, act=0):
    """out = act(s (z scale + shift) + (r | r rscale + rshift)).  Returns a dict: out, bits (sign bits of out), res (the residual term), A, undecided."""
    z = np.asarray(z, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    s = rows_of(row_scale, rows_per_image, z.shape[0])
    u = z * scale + shift
    a_u = np.abs(z * scale) + np.abs(shift)
    if rscale is not None:
        res = r * rscale + rshift
        a_res = np.abs(r * rscale) + np.abs(rshift)
    else:
        res, a_res = r, np.abs(r)
    t = s * u + res
    a = np.abs(s) * a_u + a_res               # the terms of the sum, |s| on the branch's
    out = act_fwd(t, act)
    return dict(out=out, bits=pack_bits(out > 0), res=res, A=a, undecided=undecided(t, a, (0.0,)))


def gate_rowscale(g, bits, row_scale, rows_per_image):
    """gm = bit ? s g : 0.  Returns (gm, A)."""
    g = np.asarray(g, dtype=np.float64)
    s = rows_of(row_scale, rows_per_image, g.shape[0])
    gm = np.where(unpack_bits(bits, g.shape[1]), s * g, 0.0)
    return gm, np.abs(s * g)


def bottleneck(x, sd, prefix, stride, T=None, mvf=None, training=False, new_buffers=None, scale=None):
    """oracle.net_torch.bottleneck (resnet.py:208-244) with the per-image scale `scale` (a tensor of x.shape[0] values, or None = 1) on the residual branch,
    after bn3 and before the sum: conv, BatchNorm and MVF are the oracle's functions, the residual line is this file's.  bn3's batch statistics see every
    row, dropped ones included (BatchNorm sits in front of the drop); the downsample branch is never scaled."""
    import torch.nn.functional as F

    from oracle import net_torch as nt
    identity = x
    if mvf is not None:
        out = nt.mvf_proper(x, sd, prefix + "conv1.", T, training=training, new_buffers=new_buffers, **mvf)
        out = F.conv2d(out, sd[prefix + "conv1.net.weight"])
    else:
        out = F.conv2d(x, sd[prefix + "conv1.weight"])
    out = F.relu(nt._bn(out, sd, prefix + "bn1.", training, new_buffers))
    out = F.conv2d(out, sd[prefix + "conv2.weight"], stride=stride, padding=1)
    out = F.relu(nt._bn(out, sd, prefix + "bn2.", training, new_buffers))
    out = F.conv2d(out, sd[prefix + "conv3.weight"])
    out = nt._bn(out, sd, prefix + "bn3.", training, new_buffers)
    if (prefix + "downsample.0.weight") in sd:
        identity = F.conv2d(x, sd[prefix + "downsample.0.weight"], stride=stride)
        identity = nt._bn(identity, sd, prefix + "downsample.1.", training, new_buffers)
    if scale is not None:
        out = scale.to(out.dtype).view(-1, 1, 1, 1) * out
    return F.relu(out + identity)
