"""Seeded input ciphertexts and compressed evaluation keys, host side (no GPU): the block-wise mask layout the expander kernels use
(csrc/kernels.h k_seeded_expand, k_lwe_encrypt_seeded), restated in numpy on the host generator; the SeededCiphertexts wire form;
the new C entry points in the ctypes binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(3, 35))


def _lib():
    from dctfhe import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return C.CDLL(_lib.LIB_PATH)


def rng(L, key, stream, idx0, count):
    out = np.empty(count, np.uint64)
    assert L.dctfhe_rng_host(key, C.c_uint64(stream), C.c_uint64(idx0), count, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def expand_blockwise(L, key, stream, stride, dim_eff, bodies, dim, row0=0):
    """numpy twin of k_seeded_expand: one generator block (8 words) at a time, each block computed once and owned by the first row
    that needs it, its words mapped back to (row, word); words from dim_eff on are zero, the body last"""
    count = bodies.size
    out = np.zeros((count, dim + 1), np.uint64)
    written = np.zeros((count, dim_eff), np.int64)
    for c in range(count):
        base = (row0 + c) * stride
        for b in range(base >> 3, ((base + dim_eff - 1) >> 3) + 1):
            if b == base >> 3 and c > 0 and ((base - stride + dim_eff - 1) >> 3) == b:
                continue
            words = rng(L, key, stream, 8 * b, 8)
            for w in range(8):
                j, cc = 8 * b + w - base, c
                if j < 0:
                    j, cc = j + stride, c - 1
                elif j >= stride:
                    j, cc = j - stride, c + 1
                if 0 <= cc < count and j < dim_eff:
                    out[cc, j] = words[w]
                    written[cc, j] += 1
    assert np.all(written == 1)                       # every mask word exactly once
    out[:, dim] = bodies
    return out


def expand_direct(L, key, stream, D, dim_eff, bodies, dim):
    """the layout of k_lwe_encrypt: mask word j < dim_eff of ciphertext c is generator word c (D + 1) + j"""
    out = np.zeros((bodies.size, dim + 1), np.uint64)
    for c in range(bodies.size):
        out[c, :dim_eff] = rng(L, key, stream, c * (D + 1), dim_eff)
    out[:, dim] = bodies
    return out


@pytest.mark.parametrize("count,D,dim_eff,dim", [
    (1, 1024, 1024, 1024),        # one full-width row: its last block holds the body's index
    (7, 1024, 1024, 1024),        # rows 1025 words apart: every row starts inside a block its predecessor owns
    (7, 1024, 300, 320),          # compact rows with a gap: blocks of the gap are never drawn
    (5, 19, 13, 19),              # rows shorter than three blocks
    (9, 8, 8, 8),                 # the smallest stride the kernel takes
])
def test_blockwise_expander_reproduces_the_mask_layout(count, D, dim_eff, dim):
    L = _lib()
    bodies = np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    got = expand_blockwise(L, KEY, 11, D + 1, dim_eff, bodies, dim)
    assert np.array_equal(got, expand_direct(L, KEY, 11, D, dim_eff, bodies, dim))


def test_blockwise_expander_key_rows_at_an_offset():
    """bootstrap-key rows: masks kN words contiguous per row (stride = dim_eff = kN), chunks starting at row0 > 0"""
    L = _lib()
    k, N, rows, row0 = 2, 16, 6, 5
    bodies = np.zeros(rows, np.uint64)
    got = expand_blockwise(L, KEY, 64, k * N, k * N, bodies, k * N, row0=row0)
    want = rng(L, KEY, 64, row0 * k * N, rows * k * N).reshape(rows, k * N)
    assert np.array_equal(got[:, :k * N], want)


def test_seeded_ciphertexts_round_trip_and_refusals():
    from dctfhe.engine import SeededCiphertexts
    sc = SeededCiphertexts(KEY, (5 << 16) + 256, 8192, 2048, np.arange(37, dtype=np.uint64) ** 3)
    blob = sc.to_bytes()
    assert len(blob) == sc.nbytes == 32 + 32 + 37 * 8
    back = SeededCiphertexts.from_bytes(blob)
    assert (back.key, back.stream, back.D, back.input_dim) == (sc.key, sc.stream, sc.D, sc.input_dim)
    assert np.array_equal(back.bodies, sc.bodies) and back.bodies.dtype == np.uint64
    for bad in (blob[:-1], blob + b"\0" * 8, blob[:40], b"XSCT" + blob[4:], blob[:4] + b"\x02" + blob[5:]):
        with pytest.raises(ValueError):
            SeededCiphertexts.from_bytes(bad)
    with pytest.raises(ValueError):
        SeededCiphertexts(KEY[:31], 0, 8192, 2048, np.zeros(1, np.uint64))
    with pytest.raises(ValueError):
        SeededCiphertexts(KEY, 0, 1024, 2048, np.zeros(1, np.uint64))        # input_dim > D


def test_new_entry_points_are_bound_and_declared():
    from dctfhe import _lib as lib
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "dctfhe.h")).read()
    for name in ("dctfhe_encrypt_seeded", "dctfhe_expand_seeded", "dctfhe_session_upload_seeded", "dctfhe_eval_keys_export_compressed",
                 "dctfhe_eval_keys_decompress_bsk"):
        assert name in lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name


def test_configuration_takes_the_compression_switches():
    from dctfhe.quantized_module import Configuration
    c = Configuration(compress_input_ciphertexts=True, compress_evaluation_keys=True)
    assert c.compress_input_ciphertexts and c.compress_evaluation_keys
    d = Configuration()
    assert not d.compress_input_ciphertexts and not d.compress_evaluation_keys
