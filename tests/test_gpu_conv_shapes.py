"""The two convolution kernels (csrc/kernels.h: k_conv2d_mfma on the matrix cores for rows of 32 words and more, k_conv2d<16> on the
vector ALU below that) ONE AT A TIME through dctfhe_conv2d_rows, word for word against the numpy reference of tests/conv_ref.py, at
the shapes where such kernels go wrong: the tail of the contraction (Cin KH KW around the step of 32), partial and multiple blocks of
output channels, row tiles that are full, half live or body only, rows stored at an effective dimension (the words between deff and
the body are GARBAGE on purpose: the kernels must not read them), non-square / strided / all-padding geometry, and the byte-limb carry
chain and i32 accumulators at the shipped depth of 512 * 9 taps with the largest weights and words.  Integer arithmetic mod 2^64:
np.array_equal everywhere.  Then the refusals of the entry point and the launch-grid guard of dev_conv2d."""
import functools
import re
from collections import namedtuple

import numpy as np
import pytest

import conv_ref

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "B Cin H W Cout KH KW stride pad dim_in deff dim_o fill")


def case(B=2, Cin=3, H=5, W=4, Cout=5, KH=3, KW=3, stride=1, pad=1, dims=(40, 40, 40), fill="mixed"):
    return Case(B, Cin, H, W, Cout, KH, KW, stride, pad, *dims, fill)


@functools.lru_cache(maxsize=None)
def data(c):
    """input rows, weights and the reference result of a case: made once, shared by the tests that use the case, read-only"""
    rng = np.random.default_rng([v for v in c[:-1]])
    shape_x, shape_w = (c.B, c.Cin, c.H, c.W, c.dim_in + 1), (c.Cout, c.Cin, c.KH, c.KW)
    if c.fill == "mixed":
        x, w = conv_ref.mixed_words(rng, shape_x), conv_ref.full_range_weights(rng, shape_w)
    else:       # the extremes: every limb product has the same sign and the largest magnitude
        wv, word = {"neg": (-128, 0x8080808080808080), "pos": (127, 0x7F7F7F7F7F7F7F7F)}[c.fill]
        x, w = np.full(shape_x, word, np.uint64), np.full(shape_w, wv, np.int8)
        x[..., c.deff:c.dim_in] = rng.integers(0, 2 ** 64, x[..., c.deff:c.dim_in].shape, dtype=np.uint64)
    want = conv_ref.conv2d_rows(x, c.deff, w, c.stride, c.pad, c.dim_o)
    for a in (x, w, want):
        a.flags.writeable = False
    return x, w, want


def run(ctx, c):
    x, w, want = data(c)
    got = ctx.conv2d_rows(x, c.deff, w, c.stride, c.pad, c.dim_o)
    assert got.shape == want.shape
    if not np.array_equal(got, want):       # where: which words, channels and pixels tells staging from tap table from epilogue
        bad = np.argwhere(got != want)
        raise AssertionError("%d of %d words differ; first (batch, channel, y, x, word): %s; words %s, channels %s" % (
            len(bad), want.size, bad[:5].tolist(), sorted(set(bad[:, 4].tolist()))[:40], sorted(set(bad[:, 1].tolist()))[:40]))
    if c.KH == c.KW == 1 and c.pad == 2:      # pixels whose only tap is padding come out zero, body included
        assert not got[:, :, :2].any() and not got[:, :, -2:].any() and not got[:, :, :, :2].any() and not got[:, :, :, -2:].any()
    return got


# the geometry list both kernels take
GEOMETRY = {
    "1x3": dict(H=4, W=6, KH=1, KW=3),
    "3x1": dict(H=6, W=4, KH=3, KW=1),
    "7x7_stride2_pad3_on_9x8": dict(Cin=2, H=9, W=8, KH=7, KW=7, stride=2, pad=3),        # the ResNet-18 224^2 stem
    "1x1_pad2": dict(H=3, W=4, KH=1, KW=1, pad=2),                                        # border pixels are pure padding
    "stride3": dict(H=8, W=7, stride=3),
    "kernel_equals_padded_input": dict(H=3, W=4, KH=5, KW=6, pad=1),                      # Ho = Wo = 1
    "tall_9x2": dict(H=9, W=2),
    "batch3": dict(B=3),
}

# ---- group 1: the matrix-core kernel (dim_o + 1 >= 32)
MFMA = {}
# contraction tail: K = Cin KH KW walks in steps of 32 through the padded tap table
MFMA.update({"K%d" % (cin * kh * kw): case(Cin=cin, KH=kh, KW=kw, pad=kh // 2) for cin, kh, kw in [(3, 3, 3), (32, 1, 1), (11, 1, 3), (8, 3, 3), (24, 2, 2)]})
# blocks of 64 output channels (blockIdx.z): one channel, one full block, one channel / two channels in the last of two / three blocks
MFMA.update({"Cout%d" % co: case(Cout=co, H=3, W=4) for co in (1, 64, 65, 130)})
# row tiles of 32 words: one tile exactly; the body alone in the second; full width; a half-live tile; body only; wider / narrower output
MFMA.update({"rows_%d_%d_%d" % d: case(dims=d) for d in [(31, 31, 31), (32, 32, 32), (96, 96, 96), (64, 40, 64), (64, 0, 40), (40, 40, 100), (100, 33, 50)]})
MFMA.update({"geom_" + k: case(**g) for k, g in GEOMETRY.items()})
# accumulator headroom at the shipped depth: 512 * 9 taps of (-128) * (-128) resp. 127 * 127 in every i32 accumulator of the centre pixel
MFMA.update({"depth4608_" + f: case(B=1, Cin=512, H=3, W=3, Cout=2, dims=(31, 31, 31), fill=f) for f in ("neg", "pos")})
assert sorted(c.Cin * c.KH * c.KW for k, c in MFMA.items() if k.startswith("K")) == [27, 32, 33, 72, 96]
assert all(c.dim_o + 1 >= 32 for c in MFMA.values())

# ---- group 2: the vector-ALU kernel (dim_o + 1 < 32), 16 output channels per block of blockIdx.z
VALU = {}
VALU.update({"dim%d" % d: case(dims=(d, d, d)) for d in (0, 7, 30)})          # dim 0: the clear-mode form, one word per element
VALU.update({"Cout%d" % co: case(Cout=co, H=3, W=4, dims=(7, 7, 7)) for co in (15, 16, 17, 33)})
VALU["rows_30_12_20"] = case(dims=(30, 12, 20))
VALU.update({"geom_" + k: case(dims=(7, 7, 7), **g) for k, g in GEOMETRY.items()})
VALU.update({"depth4608_%s_dim%d" % (f, d): case(B=1, Cin=512, H=3, W=3, Cout=2, dims=(d, d, d), fill=f) for f in ("neg", "pos") for d in (0, 7)})
assert all(c.dim_o + 1 < 32 for c in VALU.values())


def params(cases, keep=lambda c: True):
    return [pytest.param(c, id=k) for k, c in cases.items() if keep(c)]


@pytest.mark.parametrize("c", params(MFMA))
def test_matrix_core_kernel_bit_exact(gpu_ctx, c):
    run(gpu_ctx, c)


@pytest.mark.parametrize("c", params(VALU))
def test_vector_alu_kernel_bit_exact(gpu_ctx, c):
    run(gpu_ctx, c)


# ---- group 3: cross-checks
@pytest.mark.parametrize("c", [pytest.param(MFMA[k], id=k) for k in ("rows_64_40_64", "geom_7x7_stride2_pad3_on_9x8")])
def test_matrix_core_kernel_against_the_oracle_on_the_dense_form(gpu_ctx, oracle, c):
    x, w, _ = data(c)
    got = gpu_ctx.conv2d_rows(x, c.deff, w, c.stride, c.pad, c.dim_o)
    xd = conv_ref.dense(x, c.deff, c.dim_o)
    for b in range(c.B):
        assert np.array_equal(got[b], oracle.conv2d(xd[b], c.Cin, c.H, c.W, c.dim_o, w.astype(np.int32), c.stride, c.pad)), b


@pytest.mark.parametrize("c", params(MFMA, lambda c: c.dim_in == c.deff == c.dim_o))
def test_conv2d_is_conv2d_rows_at_full_width(gpu_ctx, c):
    x, w, want = data(c)
    got = gpu_ctx.conv2d(c.dim_o, x, c.B, c.Cin, c.H, c.W, w, c.stride, c.pad)
    assert np.array_equal(got, gpu_ctx.conv2d_rows(x, c.deff, w, c.stride, c.pad, c.dim_o)) and np.array_equal(got, want)


# ---- group 4: refusals, by their messages; the context works afterwards
def test_refusals_leave_the_context_usable(gpu_ctx):
    from dctfhe._lib import DctfheError
    c = case(dims=(40, 24, 40))
    x, w, want = data(c)
    with pytest.raises(DctfheError, match="dctfhe_conv2d_rows: rows of 40 mask words with effective dimension 41"):
        gpu_ctx.conv2d_rows(x, 41, w, 1, 1, 64)
    with pytest.raises(DctfheError, match=r"dctfhe_conv2d_rows: output rows of 23 mask words cannot hold the result \(24 needed\)"):
        gpu_ctx.conv2d_rows(x, 24, w, 1, 1, 23)
    with pytest.raises(DctfheError, match="dctfhe_conv2d_rows: bad geometry"):
        gpu_ctx.conv2d_rows(x, 24, w, 0, 1, 40)
    with pytest.raises(DctfheError, match="dctfhe_conv2d_rows: bad geometry"):
        gpu_ctx.conv2d_rows(x, 24, w, 1, -1, 40)
    with pytest.raises(DctfheError, match="dctfhe_conv2d_rows: kernel larger than the padded input"):
        gpu_ctx.conv2d_rows(x[:, :, :2, :2], 24, w, 1, 0, 40)
    with pytest.raises(DctfheError, match="dctfhe_conv2d: kernel larger than the padded input"):      # the old entry point keeps its own name
        gpu_ctx.conv2d(40, x[:, :, :2, :2], c.B, c.Cin, 2, 2, w, 1, 0)
    run(gpu_ctx, c)


# ---- group 5: the launch-grid guard.  One output pixel per block of gridDim.y: 257 * 257 = 66 049 pixels is past 65 535.  The library
# compares the pixel count with what the device reports (hipDeviceAttributeMaxGridDimY) and REFUSES above it; at
# or below it the launch goes ahead and must be bit-exact.  Which of the two happened depends on the device's limit alone.
@pytest.mark.parametrize("dim", [31, 0])
def test_launch_grid_guard(gpu_ctx, dim):
    from dctfhe._lib import DctfheError
    pixels = 257 * 257
    rng = np.random.default_rng(dim)
    x, w = conv_ref.mixed_words(rng, (1, 1, 257, 257, dim + 1)), conv_ref.full_range_weights(rng, (1, 1, 1, 1))
    try:
        got = gpu_ctx.conv2d_rows(x, dim, w, 1, 0, dim)
    except DctfheError as e:
        m = re.search(r"convolution: (\d+) output pixels .* launch-grid limit of (\d+)", str(e))
        assert m, str(e)
        assert int(m.group(1)) == pixels and int(m.group(2)) < pixels
        print("refused: %s" % e)
        run(gpu_ctx, case(dims=(dim, dim, dim)))       # the context still works
    else:
        print("launched: %d pixels are within the device's limit" % pixels)
        assert np.array_equal(got, conv_ref.conv2d_rows(x, dim, w, 1, 0, dim))
