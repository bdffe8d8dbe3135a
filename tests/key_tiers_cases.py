"""The tiny catalogues and the blob arithmetic of the tier-selection tests (tests/test_key_tiers_host.py, tests/test_gpu_key_tiers.py),
built from the shapes of params.test_params(), which have kernels.  The byte counts restate include/dctfhe.h from the tier fields; nothing
here calls the library."""
import ctypes as C
import struct

import numpy as np

from dctfhe import params as P

HEADER = 16                       # u32 magic, u32 version, u64 total bytes; then the dctfhe_params
DEVK, DEVC = 0x4b564544, 0x43564544


def catalogue_a():
    """D = 1024, four tiers: q (t_tab's shape, own key-switch key, never bootstrapped on), t (the same shape, shares q's key: the table
    tier), b (t_bit's shape, own key: the bit tier), u (t_bit's shape, own key, unused and last)"""
    tab = dict(n=48, k=1, logN=10, l=2, beta=12, lk=5, betak=4, lwe_sigma=2.0 ** -26, glwe_sigma=2.0 ** -48)
    bit = dict(n=40, k=2, logN=8, l=2, beta=10, lk=5, betak=4, lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -48)
    tiers = [P.TierSpec("q", **tab), P.TierSpec("t", ksk_share=0, **tab), P.TierSpec("b", **bit), P.TierSpec("u", **bit)]
    return P.ParamSet(D=1024, tiers=tiers, bit_tier=2, table_tier_for_w={6: 1}, input_sigma=2.0 ** -55)


def catalogue_b():
    """D = 2048, n = 40, the two unroll-2 shapes twice: p / p2 (k, l, logN) = (1, 1, 11), d / d2 (1, 3, 11) -- the duo tier, whose Fourier key
    is permuted on export.  p and d2 own a key-switch key, d and p2 share p's."""
    pair = dict(n=40, k=1, logN=11, l=1, beta=23, lk=4, betak=4, unroll=2, lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -52)
    duo = dict(pair, l=3, beta=12)
    tiers = [P.TierSpec("p", **pair), P.TierSpec("d", ksk_share=0, **duo), P.TierSpec("p2", ksk_share=0, **pair), P.TierSpec("d2", **duo)]
    return P.ParamSet(D=2048, tiers=tiers, bit_tier=0, table_tier_for_w={4: 0}, input_sigma=2.0 ** -55)


def tiny_circuit(ps):
    from dctfhe import compile as cc, models
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    return cc.compile_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=ps), calib


def mask_of(ps, names):
    idx = {t.name: i for i, t in enumerate(ps.tiers)}
    return sum(1 << idx[n] for n in names)


def blocks(t):
    return 3 * t.n // 2 if t.unroll == 2 else t.n


def sections(ps, compressed):
    """per tier (ksk bytes, bsk bytes) of one blob form, from the tier fields"""
    out = []
    for t in ps.tiers:
        if compressed:
            ksk, bsk = ps.D * t.lk * 8, blocks(t) * (t.k + 1) * t.l * t.N * 8
        else:
            ksk, bsk = ps.D * t.lk * (t.n + 1) * 8, blocks(t) * (t.k + 1) ** 2 * t.l * (t.N // 2) * 16
        out.append((ksk if t.ksk_share < 0 else 0, bsk))
    return out


def params_bytes():
    from dctfhe._lib import Params
    return C.sizeof(Params)


def blob_bytes(ps, bsk, ksk, compressed):
    full = bsk == (1 << len(ps.tiers)) - 1 and ksk == sum(1 << i for i, t in enumerate(ps.tiers) if t.ksk_share < 0)
    n = HEADER + params_bytes() + (32 if compressed else 0) + (0 if full else 8)
    for i, (k, b) in enumerate(sections(ps, compressed)):
        n += k * ((ksk >> i) & 1) + b * ((bsk >> i) & 1)
    return n


def slice_sections(full_blob, ps, bsk, ksk, compressed):
    """the kept sections, in tier order, cut out of the blob that holds every tier"""
    full_blob = np.asarray(full_blob, np.uint8)
    at = HEADER + params_bytes() + (32 if compressed else 0)
    out = []
    for i, (k, b) in enumerate(sections(ps, compressed)):
        if (ksk >> i) & 1:
            out.append(full_blob[at:at + k])
        at += k
        if (bsk >> i) & 1:
            out.append(full_blob[at:at + b])
        at += b
    assert at == full_blob.size
    return np.concatenate(out)


def pruned_from_full(full_blob, ps, bsk, ksk, compressed):
    """the pruned blob the layout rule derives from the full one: the next version, the new total, the masks behind the header (behind the
    public generator key in the compressed form), the kept sections"""
    full_blob = np.asarray(full_blob, np.uint8)
    head = HEADER + params_bytes() + (32 if compressed else 0)
    magic, version, total = struct.unpack_from("<IIQ", full_blob[:16].tobytes())
    assert magic == (DEVC if compressed else DEVK) and version == (1 if compressed else 3) and total == full_blob.size
    body = slice_sections(full_blob, ps, bsk, ksk, compressed)
    new_total = head + 8 + body.size
    hdr = np.frombuffer(struct.pack("<IIQ", magic, version + 1, new_total), np.uint8)
    masks = np.frombuffer(struct.pack("<II", bsk, ksk), np.uint8)
    return np.concatenate([hdr, full_blob[16:head], masks, body])
