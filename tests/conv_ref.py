"""Plain numpy reference of the convolution on ciphertext rows (include/dctfhe.h dctfhe_conv2d_rows), independent of the oracle library:
widen the stored rows to dense form (mask words from deff on are zero, the body moves to the end), pad spatially, and for each tap
add  w.astype(int64).astype(uint64) * x  in wrapping u64 arithmetic.  tests/test_conv_ref_host.py pins it against exact Python-integer
arithmetic and against oracle.conv2d; tests/test_gpu_conv_shapes.py compares the two HIP kernels with it word for word.
Also the input makers those two files share: words that stress the byte-limb carry chain and weights over the whole int8 range."""
import numpy as np

# every byte >= 0x80 (a carry out of every limb), all ones, every byte 0x7F (no carry, largest positive limbs), the top bit alone,
# alternating 0x00 / 0xFF bytes (a carry into every other limb), and zero
EDGE_WORDS = np.array([0, 0x8080808080808080, 0xFFFFFFFFFFFFFFFF, 0x7F7F7F7F7F7F7F7F, 0x8000000000000000, 0x00FF00FF00FF00FF], np.uint64)
EDGE_WEIGHTS = np.array([-128, -127, 127, 0], np.int8)


def mixed_words(rng, shape):
    """half random words, half EDGE_WORDS, each edge word forced to occur (when there is room)"""
    x = rng.integers(0, 2 ** 64, shape, dtype=np.uint64)
    pick = rng.integers(0, 2 * len(EDGE_WORDS), shape)
    x = np.where(pick < len(EDGE_WORDS), EDGE_WORDS[pick % len(EDGE_WORDS)], x)
    flat = x.reshape(-1)
    if flat.size >= len(EDGE_WORDS):
        flat[rng.choice(flat.size, len(EDGE_WORDS), replace=False)] = EDGE_WORDS
    return flat.reshape(shape)


def full_range_weights(rng, shape):
    """int8 weights over -128..127 with -128, -127, 127 and 0 forced to occur (as many of them as the shape has room for)"""
    w = rng.integers(-128, 128, shape).astype(np.int8)
    flat = w.reshape(-1)
    n = min(flat.size, len(EDGE_WEIGHTS))
    flat[rng.choice(flat.size, n, replace=False)] = EDGE_WEIGHTS[:n]
    return flat.reshape(shape)


def dense(x, deff, dim_o):
    """the ciphertexts that stored rows [..., dim + 1] stand for, widened to dim_o mask words: words from deff on are zero, body last"""
    out = np.zeros(x.shape[:-1] + (dim_o + 1,), np.uint64)
    out[..., :deff] = x[..., :deff]
    out[..., dim_o] = x[..., -1]
    return out


def out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def conv2d_rows(x, deff, weight, stride, pad, dim_o):
    """x u64 [batch, Cin, H, W, dim + 1] rows at effective dimension deff, weight int8 [Cout, Cin, KH, KW]
    -> u64 [batch, Cout, Ho, Wo, dim_o + 1]: out[b, co, y, x] = sum_{ci, ky, kx} w[co, ci, ky, kx] * in[b, ci, y s + ky - p, x s + kx - p] mod 2^64"""
    assert x.dtype == np.uint64 and weight.dtype == np.int8
    xd = dense(x, deff, dim_o)
    B, Cin, H, W, L = xd.shape
    Cout, Cin_w, KH, KW = weight.shape
    assert Cin_w == Cin
    Ho, Wo = out_hw(H, W, KH, KW, stride, pad)
    xp = np.zeros((B, Cin, H + 2 * pad, W + 2 * pad, L), np.uint64)
    xp[:, :, pad:pad + H, pad:pad + W] = xd
    wu = weight.astype(np.int64).astype(np.uint64)          # two's complement: -1 -> 2^64 - 1
    out = np.zeros((B, Cout, Ho, Wo, L), np.uint64)
    for ci in range(Cin):
        for ky in range(KH):
            for kx in range(KW):
                tap = xp[:, ci, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]      # [B, Ho, Wo, L]
                out += wu[None, :, ci, ky, kx, None, None, None] * tap[:, None]
    return out
