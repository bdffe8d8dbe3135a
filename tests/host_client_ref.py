"""What tests/test_host_client.py and tests/test_gpu_host_client.py share: the tiny custom parameter set of the host client's key checks,
the generator (dctfhe_rng_host), the spec streams of include/dctfhe.h restated, the layout of a compressed evaluation-key blob, and the
checks of its key-switch and bootstrap bodies against the definition.  numpy only; nothing here comes from libdctfhe_client.so."""
import ctypes as C
import struct

import numpy as np

import key_material_ref as K

U = np.uint64
NONCE = bytes(range(40, 56))
HEADER = 16                       # u32 magic, u32 version, u64 total bytes; then the dctfhe_params, then the 32-byte public generator key
CBLOB_MAGIC = 0x43564544          # 'DEVC'


def custom_tiers():
    """D = 2048, n_max = 8.  Tier 0: a k = 2 one-bit tier, key-switch gadget 2 x 4 bits (2-limb grid).  Tier 1: unroll 2 (the pair
    secret; general two-bit form k = 2, N = 1024, l = 1), gadget 5 x 4 bits (4 limbs).  Tier 2: k = 1, three levels, gadget 7 x 4 bits
    (8 limbs: the full word).  Tier 3: shares tier 0's key-switch key.  Every (logN, k, l) has a bootstrap kernel, so the device imports
    the blob.  Noise far above one unit of 2^-64 and far below every gadget term (NOT secure)."""
    t = lambda **kw: dict(dict(lwe_sigma=2.0 ** -30, glwe_sigma=2.0 ** -40, unroll=1, ksk_share=-1), **kw)
    return [t(n=6, k=2, logN=8, l=2, beta=14, lk=2, betak=4, lwe_sigma=2.0 ** -12),
            t(n=8, k=2, logN=10, l=1, beta=23, lk=5, betak=4, unroll=2, lwe_sigma=2.0 ** -26),
            t(n=8, k=1, logN=9, l=3, beta=12, lk=7, betak=4),
            t(n=6, k=1, logN=10, l=2, beta=12, lk=2, betak=4, ksk_share=0, lwe_sigma=2.0 ** -12)]


CUSTOM_D, CUSTOM_NMAX, CUSTOM_INPUT_DIM, CUSTOM_INPUT_SIGMA = 2048, 8, 517, 2.0 ** -45


def custom_params():
    from dctfhe.engine import make_params
    return make_params(CUSTOM_D, CUSTOM_NMAX, custom_tiers(), CUSTOM_INPUT_SIGMA, CUSTOM_INPUT_DIM)


def rng(key, stream, idx0, count):
    """`count` generator words (key, stream, idx0 ...): dctfhe_rng_host of libdctfhe.so, the known-answer-tested host generator"""
    from dctfhe import _lib
    out = np.empty(count, U)
    assert _lib.load().dctfhe_rng_host(bytes(key), C.c_uint64(stream), C.c_uint64(idx0), C.c_size_t(count), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _sigma_mix(sigma):
    return (struct.unpack("<Q", struct.pack("<d", float(sigma)))[0] * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)


def ring_stream(logN, l, beta, sigma):
    """the packing key's mask stream R (include/dctfhe.h); noise: R + 1"""
    return (1 << 63) | ((_sigma_mix(sigma) ^ (logN << 24 | l << 16 | beta << 8)) & 0x7FFFFFFFFFFFFFFE)


def public_stream(logN, sigma):
    """the public key's mask stream P (include/dctfhe.h); noise: P + 1"""
    return (1 << 62) | ((_sigma_mix(sigma) ^ (logN << 24)) & 0x3FFFFFFFFFFFFFFE)


def blocks_of(t):
    return 3 * t.n // 2 if t.unroll == 2 else t.n


def parse_cblob(blob, cp):
    """a compressed evaluation-key blob -> (header bytes incl. parameters, pub key bytes, [per tier (ksk bodies [D, lk] or None, bsk bodies
    [blocks, (k+1) l, N])]); asserts that the blob ends where its parameters say"""
    blob = np.ascontiguousarray(blob, np.uint8)
    psize = C.sizeof(type(cp))
    off = HEADER + psize
    head, pub = blob[:off].tobytes(), blob[off:off + 32].tobytes()
    off += 32
    tiers = []
    for ti in range(cp.n_tiers):
        t = cp.tiers[ti]
        ksk = None
        if t.ksk_share < 0:
            ksk = np.frombuffer(blob, U, cp.D * t.lk, off).reshape(cp.D, t.lk)
            off += cp.D * t.lk * 8
        rows, N = (t.k + 1) * t.l, 1 << t.logN
        bsk = np.frombuffer(blob, U, blocks_of(t) * rows * N, off).reshape(blocks_of(t), rows, N)
        off += bsk.size * 8
        tiers.append((ksk, bsk))
    assert off == blob.size, (off, blob.size)
    return head, pub, tiers


def check_header(blob, cp, pub):
    """magic, version, total bytes, the parameters byte for byte, the public generator key"""
    head, got_pub, _ = parse_cblob(blob, cp)
    magic, version, total = struct.unpack_from("<IIQ", head)
    assert (magic, version, total) == (CBLOB_MAGIC, 1, len(blob))
    assert head[HEADER:] == bytes(cp)
    assert got_pub == bytes(pub)


def ksk_masks(cp, ti, pub):
    """mask words [D lk, n] of tier ti's key-switch key: generator words (pub, 16 + 2 ti, row (n + 1) + j) on the tier's grid"""
    t = cp.tiers[ti]
    rows, grid_bits = cp.D * t.lk, 64 - 8 * K.ks_limbs(t.lk, t.betak)
    words = rng(pub, K.ksk_streams(ti)[0], 0, rows * (t.n + 1)).reshape(rows, t.n + 1)[:, :t.n]
    return words & ~U((1 << grid_bits) - 1), grid_bits


def check_ksk(cp, ti, bodies, pub, S, s):
    """every body on its grid; phase <a, s> recomputed exactly = S_i 2^(64 - betak (lev + 1)) + noise of lwe_sigma and the grid rounding"""
    t = cp.tiers[ti]
    masks, grid_bits = ksk_masks(cp, ti, pub)
    body = np.asarray(bodies, U).reshape(-1)
    assert not (body & U((1 << grid_bits) - 1)).any(), (ti, "a key-switch body off its grid")
    ph = (body - (masks * s[:t.n].astype(U)).sum(axis=1, dtype=U)).reshape(cp.D, t.lk)
    want = np.stack([S.astype(U) << U(64 - t.betak * (lev + 1)) for lev in range(t.lk)], axis=1)
    E = (ph - want).view(np.int64)
    return K.check_noise(E, t.lwe_sigma, "host key-switch key, tier %d, %d limbs" % (ti, K.ks_limbs(t.lk, t.betak)), grid_bits=grid_bits, with_kurtosis=False)


def bsk_rows(cp, ti, bodies, pub):
    """the full rows [blocks, (k+1) l, k + 1, N] of a compressed key: masks are the generator's words (pub, 64 + 2 ti, (grow k + j) N + c)"""
    t = cp.tiers[ti]
    k, N, rows, blocks = t.k, 1 << t.logN, (t.k + 1) * t.l, blocks_of(t)
    masks = rng(pub, K.bsk_streams(ti)[0], 0, blocks * rows * k * N).reshape(blocks, rows, k, N)
    return np.concatenate([masks, np.asarray(bodies, U).reshape(blocks, rows, 1, N)], axis=2)


def bsk_plaintext(cp, ti, S, s):
    """the phase every row must carry, [blocks, (k+1) l, N]: bit g at coefficient 0 for p = k, - bit g S_p (BODY FORM) for p < k"""
    t = cp.tiers[ti]
    k, l, N, blocks = t.k, t.l, 1 << t.logN, blocks_of(t)
    bits = K.pair_secret(s[:t.n]) if t.unroll == 2 else s[:t.n]
    pt = np.zeros((blocks, (k + 1) * l, N), U)
    for b in range(blocks):
        if not bits[b]:
            continue
        for r in range((k + 1) * l):
            p, lev = divmod(r, l)
            g = U(1 << (64 - t.beta * (lev + 1)))
            if p < k:
                pt[b, r] = U(0) - g * K.key_poly(S, p, N)
            else:
                pt[b, r, 0] = g
    return pt, bits


def check_bsk(cp, ti, bodies, pub, S, s):
    """every row's exact phase = the body-form gadget term + noise of glwe_sigma; the rows p < k are in body form (their phase carries
    - bit g S_p, which a standard-form body would not)"""
    t = cp.tiers[ti]
    k, N = t.k, 1 << t.logN
    rows = bsk_rows(cp, ti, bodies, pub)
    pt, bits = bsk_plaintext(cp, ti, S, s)
    assert 0 < bits.sum() < bits.size, "the test key needs both bit values"
    E = (K.glwe_phase(rows, S, k, N) - pt).view(np.int64)
    st = K.check_noise(E, t.glwe_sigma, "host bootstrap key, tier %d" % ti)
    # body form, said once more from the other side: read as standard-form rows (gadget term in the mask) the p < k rows of a set bit
    # would be off by g S_p, a thousand sigma
    b = int(np.flatnonzero(bits)[0])
    g = U(1 << (64 - t.beta))
    off = (K.glwe_phase(rows[b, 0], S, k, N)).view(np.int64)
    assert np.abs(off.astype(np.float64)).max() > 0.5 * float(g), "row p = 0 of a set bit carries no - g S_0: not in body form"
    return st


def within(a, b, step=1):
    """every |a - b| <= step as torus words (wrapping)"""
    d = (np.asarray(a, U) - np.asarray(b, U)).view(np.int64)
    return bool((np.abs(d) <= step).all())
