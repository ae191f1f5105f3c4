"""The one run path under FramePipeline ... Yuv420FramePipeline (preprocess.FramePipeline._run): an `out=` buffer handed to to_stem is
checked in EVERY class before the launch (a wrong one would be an out-of-bounds device write), a correct one receives the bytes of the
out=None call, and a table of a column count the class does not take is refused by name."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
PAD, WP = 3, 24                                                   # crop 16: 16 + 2 * 3 = 22 columns, rounded up to the stem's even pitch
ROWS = np.array([[20, 24, 2, 1, 16, 20, 24, 28, 3, 5, 1],         # a patch resized up, mirrored
                 [20, 24, 0, 0, 20, 24, 32, 32, 8, 16, 0]], dtype=np.int32)


def _case(name):
    """-> (pipeline, 2 frames of 20 x 24, its table)."""
    from mvfnet_amd import preprocess as P
    fr = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(2, 20, 24, 3)).astype(np.uint8)).cuda()
    if name == "FramePipeline":
        return P.FramePipeline(MEAN, STD, crop_size=16), fr, torch.tensor([[2, 3, 0], [4, 8, 1]], dtype=torch.int32)
    if name == "ResamplingFramePipeline":
        return P.ResamplingFramePipeline(MEAN, STD, crop_size=16), fr, torch.from_numpy(ROWS)
    color = P.color_identity(2)
    color[:, :9] *= np.float32(0.75)
    color[:, 9:] = np.float32([3.5, -2.25, 11.0])
    return P.JitterFramePipeline(MEAN, STD, crop_size=16), fr, torch.from_numpy(P.jitter_rows(ROWS, color))


CLASSES = ["FramePipeline", "ResamplingFramePipeline", "JitterFramePipeline"]


@pytest.mark.parametrize("name", CLASSES)
def test_to_stem_refuses_a_buffer_that_does_not_hold_the_output(name):
    pipe, fr, tab = _case(name)
    bad = {"one row too few": torch.empty(2, 21, WP, 4, device="cuda"),
           "one image too few": torch.empty(1, 22, WP, 4, device="cuda"),
           "wrong dtype": torch.empty(2, 22, WP, 4, dtype=torch.bfloat16, device="cuda"),
           "not contiguous": torch.empty(2, 22, WP, 8, device="cuda")[..., :4]}
    assert tuple(bad["not contiguous"].shape) == (2, 22, WP, 4)
    for why, buf in bad.items():
        with pytest.raises(ValueError, match="output buffer"):
            pipe.to_stem(fr, tab, PAD, WP, torch.float32, out=buf)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", CLASSES)
def test_to_stem_into_a_buffer_writes_the_bytes_of_the_allocating_call(name):
    pipe, fr, tab = _case(name)
    for dtype in (torch.float32, torch.bfloat16):
        want = pipe.to_stem(fr, tab, PAD, WP, dtype)
        assert want.shape == (2, 22, WP, 4) and want.dtype == dtype and bool((want.float() != 0).any())
        buf = torch.full((2, 22, WP, 4), -7.0, dtype=dtype, device="cuda")
        got = pipe.to_stem(fr, tab, PAD, WP, dtype, out=buf)
        assert got.data_ptr() == buf.data_ptr()
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert torch.equal(buf.view(bits), want.view(bits))


def test_a_column_count_the_class_does_not_take_is_refused():
    from mvfnet_amd import preprocess as P
    fr = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device="cuda")
    jit, gat = P.jitter_rows(ROWS), P.gather_rows(ROWS, [0, 1])
    assert jit.shape == (2, 23) and gat.shape == (2, 12) and P.gather_rows(jit, [0, 1]).shape == (2, 24)
    for cls, tab in [(P.ResamplingFramePipeline, jit), (P.ResamplingFramePipeline, gat), (P.JitterFramePipeline, P.gather_rows(jit, [0, 1]))]:
        pipe = cls(MEAN, STD, crop_size=16)
        with pytest.raises(ValueError, match="columns"):
            pipe.to_nchw(fr, torch.from_numpy(tab))
        with pytest.raises(ValueError, match="columns"):
            pipe.to_stem(fr, torch.from_numpy(tab), PAD, WP, torch.float32)
    torch.cuda.synchronize()
