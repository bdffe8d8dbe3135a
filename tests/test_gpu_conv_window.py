"""The output window of the two convolution kernels (csrc/kernels.h: channels [c0, c1) into a buffer that holds the window alone, pixels
in chunks of the launch grid) through dctfhe_conv2d_rows_window, word for word against the matching channel slice of the numpy
reference of tests/conv_ref.py.  Cout = 65 crosses the 64-channel tile of the matrix-core kernel (a tile that starts at c0 = 1 or 63
reaches past the padded weight rows) and several 16-channel tiles of the vector-ALU kernel.  Then the pixel chunking (66 049 pixels, past
the 65 535 of one launch, must SUCCEED) and the refusals of the window, by their messages."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import conv_ref

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "B Cin H W Cout KH KW stride pad dim_in deff dim_o")
WINDOWS = [(0, 1), (63, 65), (1, 64), (0, 65)]


def case(B=1, Cin=3, H=4, W=3, Cout=65, KH=3, KW=3, stride=1, pad=1, dims=(40, 40, 40)):
    return Case(B, Cin, H, W, Cout, KH, KW, stride, pad, *dims)


CASES = {
    "rows40": case(dims=(39, 39, 39)),                                           # 40 words: a full tile of 32 and a partial one
    "rows31_valu": case(dims=(30, 30, 30)),                                      # 31 words: below 32, the vector-ALU kernel
    "deff_below_width": case(dims=(64, 24, 40)),                                 # words [24, 64) of the input are garbage, [24, 40) of the output zero
    "deff_below_width_valu": case(dims=(30, 12, 20)),
    "7x7_stride2_pad3_on_9x9": case(Cin=2, H=9, W=9, KH=7, KW=7, stride=2, pad=3),
    "7x7_stride2_pad3_on_9x9_valu": case(Cin=2, H=9, W=9, KH=7, KW=7, stride=2, pad=3, dims=(7, 7, 7)),
    "batch2": case(B=2),
    "batch2_valu": case(B=2, dims=(0, 0, 0)),                                    # one word per element: the clear-mode form
}


@functools.lru_cache(maxsize=None)
def data(c):
    """input rows, weights and the reference's WHOLE output: made once per case, shared by its windows, read-only"""
    rng = np.random.default_rng(list(c))
    x = conv_ref.mixed_words(rng, (c.B, c.Cin, c.H, c.W, c.dim_in + 1))
    w = conv_ref.full_range_weights(rng, (c.Cout, c.Cin, c.KH, c.KW))
    want = conv_ref.conv2d_rows(x, c.deff, w, c.stride, c.pad, c.dim_o)
    for a in (x, w, want):
        a.flags.writeable = False
    return x, w, want


def check(got, want):
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%d of %d words differ; first (batch, channel of the window, y, x, word): %s" % (len(bad), want.size, bad[:5].tolist()))


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "c%d_%d" % w)
@pytest.mark.parametrize("c", [pytest.param(c, id=k) for k, c in CASES.items()])
def test_window_is_the_channel_slice_of_the_reference(gpu_ctx, c, win):
    x, w, want = data(c)
    c0, c1 = win
    check(gpu_ctx.conv2d_rows_window(x, c.deff, w, c.stride, c.pad, c.dim_o, c0, c1), want[:, c0:c1])


def test_whole_window_is_conv2d_rows(gpu_ctx):
    c = CASES["batch2"]
    x, w, want = data(c)
    got = gpu_ctx.conv2d_rows_window(x, c.deff, w, c.stride, c.pad, c.dim_o, 0, c.Cout)
    assert np.array_equal(got, gpu_ctx.conv2d_rows(x, c.deff, w, c.stride, c.pad, c.dim_o))
    check(got, want)


# 1x1 on 257 x 257: 66 049 output pixels, one per block of gridDim.y, are past the 65 535 of one launch.  dctfhe_conv2d_rows may refuse
# that (tests/test_gpu_conv_shapes.py::test_launch_grid_guard); the window goes out in chunks and must succeed on every device.  Rows of
# 1 word (vector-ALU kernel) and of 32 words (matrix-core kernel); two channels, the window is the second.
@pytest.mark.parametrize("dim", [0, 31])
def test_pixel_chunks(gpu_ctx, dim):
    rng = np.random.default_rng(dim)
    x, w = conv_ref.mixed_words(rng, (1, 1, 257, 257, dim + 1)), conv_ref.full_range_weights(rng, (2, 1, 1, 1))
    want = conv_ref.conv2d_rows(x, dim, w, 1, 0, dim)
    check(gpu_ctx.conv2d_rows_window(x, dim, w, 1, 0, dim, 1, 2), want[:, 1:2])
    check(gpu_ctx.conv2d_rows_window(x, dim, w, 1, 0, dim, 0, 2), want)


def test_refusals_leave_the_context_usable(gpu_ctx):
    from dctfhe._lib import DctfheError
    c = CASES["rows40"]
    x, w, want = data(c)
    with pytest.raises(DctfheError, match=r"dctfhe_conv2d_rows_window: empty output window: channels \[3, 3\)"):
        gpu_ctx.conv2d_rows_window(x, c.deff, w, 1, 1, c.dim_o, 3, 3)
    with pytest.raises(DctfheError, match=r"dctfhe_conv2d_rows_window: empty output window: channels \[5, 2\)"):
        gpu_ctx.conv2d_rows_window(x, c.deff, w, 1, 1, c.dim_o, 5, 2)
    with pytest.raises(DctfheError, match=r"dctfhe_conv2d_rows_window: output window of channels \[60, 66\) outside the 65 the weights hold"):
        gpu_ctx.conv2d_rows_window(x, c.deff, w, 1, 1, c.dim_o, 60, 66)
    with pytest.raises(DctfheError, match=r"dctfhe_conv2d_rows_window: output window of channels \[-1, 4\) outside the 65 the weights hold"):
        gpu_ctx.conv2d_rows_window(x, c.deff, w, 1, 1, c.dim_o, -1, 4)
    with pytest.raises(DctfheError, match="dctfhe_conv2d_rows_window: bad geometry"):      # the checks of dctfhe_conv2d_rows, under this name
        gpu_ctx.conv2d_rows_window(x, c.deff, w, 0, 1, c.dim_o, 0, 1)
    check(gpu_ctx.conv2d_rows_window(x, c.deff, w, 1, 1, c.dim_o, 63, 65), want[:, 63:65])
