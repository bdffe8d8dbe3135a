"""tests/conv_ref.py, the numpy reference the convolution kernels are compared with word for word (tests/test_gpu_conv_shapes.py), pinned
on the CPU: (a) against exact Python-integer arithmetic reduced mod 2^64 on sampled outputs, (b) against the oracle's ref_conv2d on the
dense form.  No GPU."""
import numpy as np
import pytest

import conv_ref

M64 = (1 << 64) - 1

# (batch, Cin, H, W, Cout, KH, KW, stride, pad, dim_in, deff, dim_o): a square kernel on rows narrower than stored, a 1x3 kernel with
# stride 2 into rows wider than the input, and a kernel with pad >= its extent on clear-mode rows (one word per element)
CASES = [(2, 3, 5, 4, 4, 3, 3, 1, 1, 12, 7, 9),
         (1, 2, 4, 7, 3, 1, 3, 2, 1, 5, 5, 8),
         (2, 2, 3, 3, 2, 2, 2, 1, 2, 0, 0, 0)]


def make(case):
    B, Cin, H, W, Cout, KH, KW, stride, pad, dim_in, deff, dim_o = case
    rng = np.random.default_rng(sum(case))
    x = conv_ref.mixed_words(rng, (B, Cin, H, W, dim_in + 1))
    w = conv_ref.full_range_weights(rng, (Cout, Cin, KH, KW))
    return x, w


def exact_word(x, deff, w, stride, pad, dim_o, b, co, y, xo, word):
    """one output word in Python integers: nothing here can wrap, round or overflow"""
    _, Cin, H, W, L = x.shape
    _, _, KH, KW = w.shape
    if word == dim_o:
        iw = L - 1
    elif word < deff:
        iw = word
    else:
        return 0
    acc = 0
    for ci in range(Cin):
        for ky in range(KH):
            for kx in range(KW):
                iy, ix = y * stride + ky - pad, xo * stride + kx - pad
                if 0 <= iy < H and 0 <= ix < W:
                    acc += int(w[co, ci, ky, kx]) * int(x[b, ci, iy, ix, iw])
    return acc & M64


@pytest.mark.parametrize("case", CASES)
def test_reference_equals_python_integers_on_sampled_outputs(case):
    B, Cin, H, W, Cout, KH, KW, stride, pad, dim_in, deff, dim_o = case
    x, w = make(case)
    assert {-128, 127} <= set(w.reshape(-1).tolist())
    assert {0x8080808080808080, 0xFFFFFFFFFFFFFFFF} <= set(x.reshape(-1).tolist())
    got = conv_ref.conv2d_rows(x, deff, w, stride, pad, dim_o)
    Ho, Wo = conv_ref.out_hw(H, W, KH, KW, stride, pad)
    assert got.shape == (B, Cout, Ho, Wo, dim_o + 1) and got.dtype == np.uint64
    rng = np.random.default_rng(1)
    idx = [tuple(int(rng.integers(0, n)) for n in got.shape) for _ in range(40)]
    idx += [(B - 1, Cout - 1, Ho - 1, Wo - 1, dim_o), (0, 0, 0, 0, 0), (0, 0, 0, 0, max(deff - 1, 0)), (0, 0, 0, 0, min(deff, dim_o))]
    for i in idx:
        assert int(got[i]) == exact_word(x, deff, w, stride, pad, dim_o, *i), i
    # the words between deff and the body are zero
    assert not got[..., deff:dim_o].any()


def test_reference_at_the_extremes_in_python_integers():
    """every weight -128 on words whose bytes are all 0x80, every weight 127 on bytes 0x7F: the centre pixel sums all Cin * 9 taps"""
    for wv, word in [(-128, 0x8080808080808080), (127, 0x7F7F7F7F7F7F7F7F)]:
        x = np.full((1, 16, 3, 3, 3), word, np.uint64)
        w = np.full((2, 16, 3, 3), wv, np.int8)
        got = conv_ref.conv2d_rows(x, 2, w, 1, 1, 2)
        assert int(got[0, 1, 1, 1, 2]) == (16 * 9 * wv * word) & M64 and int(got[0, 0, 0, 0, 0]) == (16 * 4 * wv * word) & M64


@pytest.mark.parametrize("case", CASES)
def test_reference_equals_the_oracle_on_the_dense_form(oracle, case):
    B, Cin, H, W, Cout, KH, KW, stride, pad, dim_in, deff, dim_o = case
    x, w = make(case)
    got = conv_ref.conv2d_rows(x, deff, w, stride, pad, dim_o)
    xd = conv_ref.dense(x, deff, dim_o)
    for b in range(B):
        assert np.array_equal(got[b], oracle.conv2d(xd[b], Cin, H, W, dim_o, w.astype(np.int32), stride, pad))
