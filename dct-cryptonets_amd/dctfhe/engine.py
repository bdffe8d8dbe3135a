"""Object layer over the C ABI: Context, Keys, Circuit, Session (host numpy buffers in and out)."""
import ctypes as C
import hashlib
import os
import struct

import numpy as np

from . import _lib
from ._lib import KeyTiers, MarginStats, MemPlan, Params, Stats, Tier, Timing, check, ptr
from .wire import PackedCiphertexts, PackedRing, PublicInputs, SeededCiphertexts, _as_u8, seed_bytes  # noqa: F401 (re-exported)


def make_params(D, n_max, tiers, input_sigma, input_dim=0):
    """tiers: list of dicts with n,k,logN,l,beta,lk,betak,lwe_sigma,glwe_sigma[,ksk_share][,unroll]."""
    p = Params()
    p.D, p.n_max, p.n_tiers, p.input_sigma, p.input_dim = D, n_max, len(tiers), input_sigma, input_dim
    for i, t in enumerate(tiers):
        p.tiers[i] = Tier(t["n"], t["k"], t["logN"], t["l"], t["beta"], t["lk"], t["betak"], t.get("ksk_share", -1),
                          t.get("unroll", 1), 0, t["lwe_sigma"], t["glwe_sigma"])
    return p


def margin_stats_dict(m):
    """a dctfhe_margin_stats as a dict of Python ints (hist: a list of 16)"""
    return dict(op=m.op, entry=m.entry, tier=m.tier, table_bits=m.table_bits, half_box=m.half_box, max_abs=m.max_abs, count=m.count,
                sum=m.sum, sum_sq=m.sum_sq, hist=list(m.hist))


def margin_probe_host(small_key, n, logN, cts_small, table_bits, want_err=True, want_stats=True):
    """the margin audit's definition on the CPU (include/dctfhe.h dctfhe_margin_probe_host; no GPU): small ciphertexts [count, n + 1]
    under the first n bytes of small_key -> (e per ciphertext as int32 or None, statistics dict or None)"""
    L = _lib.load()
    key = np.ascontiguousarray(small_key, np.uint8)
    cts = None if cts_small is None else np.ascontiguousarray(cts_small, np.uint64)
    count = 0 if cts is None else cts.size // (max(int(n), 0) + 1)
    err = np.empty(count, np.int32) if want_err else None
    st = MarginStats() if want_stats else None
    check(L.dctfhe_margin_probe_host(ptr(key), int(n), int(logN), None if cts is None else ptr(cts), count, int(table_bits),
                                     None if err is None else ptr(err), None if st is None else C.byref(st)))
    return err, (None if st is None else margin_stats_dict(st))


def device_bytes_live():
    """bytes of device memory the library holds in this process right now (dctfhe_device_bytes_live): handles, caches, calls in flight"""
    return int(_lib.load().dctfhe_device_bytes_live())


class Context:
    def __init__(self, device=0):
        self.L = _lib.load()
        self.h = C.c_void_p()
        check(self.L.dctfhe_ctx_create(device, C.byref(self.h)))

    def set_stream(self, stream):
        """issue this context's work to `stream`: a raw HIP stream handle (int) or a torch.cuda.Stream (its .cuda_stream is taken); None, 0
        or torch's default stream (the null stream) puts the context back on its own (include/dctfhe.h dctfhe_ctx_set_stream)"""
        stream = getattr(stream, "cuda_stream", stream)
        check(self.L.dctfhe_ctx_set_stream(self.h, C.c_void_p(stream or None)))

    def synchronize(self):
        check(self.L.dctfhe_ctx_synchronize(self.h))

    def fp64_peak(self):
        v = C.c_double()
        check(self.L.dctfhe_fp64_peak(self.h, C.byref(v)))
        return v.value

    def dct_frontend(self, y, c1, c2, fs, idx, mean, std, round_coeffs=False):
        """uint8 planes y [B, fs*S, fs*S], c1/c2 [B, fs*Sc, fs*Sc] -> float32 [B, C, S, S] (include/dctfhe.h dctfhe_dct_frontend)"""
        y, c1, c2 = (np.ascontiguousarray(a, np.uint8) for a in (y, c1, c2))
        B, S, Sc = y.shape[0], y.shape[1] // fs, c1.shape[1] // fs
        ii = [np.ascontiguousarray(i, np.int32) for i in idx]
        mean, std = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(std, np.float32)
        C_ = sum(i.size for i in ii)
        assert mean.size == std.size == C_ and y.shape == (B, fs * S, fs * S) and c1.shape == c2.shape == (B, fs * Sc, fs * Sc)
        out = np.empty((B, C_, S, S), np.float32)
        check(self.L.dctfhe_dct_frontend(self.h, ptr(y), ptr(c1), ptr(c2), B, S, Sc, fs, ptr(ii[0]), ii[0].size, ptr(ii[1]), ii[1].size,
                                         ptr(ii[2]), ii[2].size, ptr(mean), ptr(std), int(bool(round_coeffs)), ptr(out)))
        return out

    def add_rows(self, a, deff_a, b, deff_b, dim_o):
        """rows [count, dim + 1] at effective dimensions deff_* -> a + b as rows [count, dim_o + 1] (include/dctfhe.h dctfhe_add_rows)"""
        a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
        out = np.empty((a.shape[0], dim_o + 1), np.uint64)
        check(self.L.dctfhe_add_rows(self.h, ptr(a), a.shape[1] - 1, deff_a, ptr(b), b.shape[1] - 1, deff_b, a.shape[0], dim_o, ptr(out)))
        return out

    def affine_rows(self, a, deff_a, inout, nwords, shift, body_add):
        a = np.ascontiguousarray(a, np.uint64)
        out = np.ascontiguousarray(inout, np.uint64).copy()
        check(self.L.dctfhe_affine_rows(self.h, ptr(a), a.shape[1] - 1, deff_a, a.shape[0], nwords, shift, C.c_uint64(body_add), out.shape[1] - 1, ptr(out)))
        return out

    def acc_rows(self, o, b, nwords):
        """o + b on the first nwords mask words and the body of rows [count, dim + 1], the other words of o as they were (dctfhe_acc_rows)"""
        out, b = np.ascontiguousarray(o, np.uint64).copy(), np.ascontiguousarray(b, np.uint64)
        if out.shape[0] != b.shape[0]:
            raise ValueError("acc_rows takes one row of b per row of o")
        check(self.L.dctfhe_acc_rows(self.h, ptr(out), out.shape[1] - 1, ptr(b), b.shape[1] - 1, out.shape[0], int(nwords)))
        return out

    def gather_rows(self, src, deff_s, row_map, dim_d):
        """rows src[row_map] of [n_src, dim + 1] at effective dimension deff_s, as rows [len(row_map), dim_d + 1] (dctfhe_gather_rows)"""
        src, m = np.ascontiguousarray(src, np.uint64), np.ascontiguousarray(row_map, np.int32)
        out = np.empty((m.size, int(dim_d) + 1), np.uint64)
        check(self.L.dctfhe_gather_rows(self.h, ptr(src), src.shape[1] - 1, int(deff_s), src.shape[0], ptr(m), m.size, int(dim_d), ptr(out)))
        return out

    def sum_pool_rows(self, x, deff, K, dim_o):
        """x [batch, C, H, W, dim + 1] -> [batch, C, H // K, W // K, dim_o + 1]"""
        x = np.ascontiguousarray(x, np.uint64)
        B, Cc, H, W, L = x.shape
        out = np.empty((B, Cc, H // K, W // K, dim_o + 1), np.uint64)
        check(self.L.dctfhe_sum_pool_rows(self.h, ptr(x), L - 1, deff, B, Cc, H, W, K, dim_o, ptr(out)))
        return out

    def max_pool_rows(self, x, deff, k, s, p, p_d, table=None, dim_o=0, keys=None, tier=0):
        """MaxPool2d(k, s, p) as the session's tree (include/dctfhe.h dctfhe_max_pool_rows).  keys given: x [batch, C, H, W, dim + 1]
        encrypted rows -> [batch, C, Ho, Wo, dim_o + 1]; keys None: the clear form, x [batch, C, H, W] words -> [batch, C, Ho, Wo]"""
        keys = getattr(keys, "eval", keys)
        x = np.ascontiguousarray(x, np.uint64)
        B, Cc, H, W = x.shape[:4]
        Ho, Wo = (max(H + 2 * p - k, 0) // max(s, 1) + 1, max(W + 2 * p - k, 0) // max(s, 1) + 1)   # the library checks the geometry
        dim_in = x.shape[4] - 1 if keys is not None else 0
        out = np.empty((B, Cc, Ho, Wo) + ((dim_o + 1,) if keys is not None else ()), np.uint64)
        tab = None if table is None else np.ascontiguousarray(table, np.int64)
        check(self.L.dctfhe_max_pool_rows(self.h, None if keys is None else keys.h, tier, ptr(x), dim_in, deff, B, Cc, H, W, k, s, p, p_d,
                                          None if tab is None else ptr(tab), dim_o, ptr(out)))
        return out

    def conv2d(self, D, cts, batch, Cin, H, W, weight, stride, pad):
        weight = np.ascontiguousarray(weight, np.int8)
        Cout, _, KH, KW = weight.shape
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        cts = np.ascontiguousarray(cts, np.uint64)
        out = np.empty((batch, Cout, Ho, Wo, D + 1), np.uint64)
        check(self.L.dctfhe_conv2d(self.h, D, ptr(cts), batch, Cin, H, W, ptr(weight), Cout, KH, KW, stride, pad, ptr(out)))
        return out

    def conv2d_rows(self, x, deff, weight, stride, pad, dim_o):
        """x [batch, Cin, H, W, dim + 1] rows at effective dimension deff, weight int8 [Cout, Cin, KH, KW] -> [batch, Cout, Ho, Wo, dim_o + 1]
        (include/dctfhe.h dctfhe_conv2d_rows: the session's convolution, matrix cores when dim_o + 1 >= 32)"""
        x, weight = np.ascontiguousarray(x, np.uint64), np.ascontiguousarray(weight, np.int8)
        B, Cin, H, W, L = x.shape
        Cout, _, KH, KW = weight.shape
        Ho, Wo = (max(H + 2 * pad - KH, 0) // max(stride, 1) + 1, max(W + 2 * pad - KW, 0) // max(stride, 1) + 1)   # the library checks the geometry
        out = np.empty((B, Cout, Ho, Wo, max(dim_o, 0) + 1), np.uint64)
        check(self.L.dctfhe_conv2d_rows(self.h, ptr(x), L - 1, deff, B, Cin, H, W, ptr(weight), Cout, KH, KW, stride, pad, dim_o, ptr(out)))
        return out

    def conv2d_rows_window(self, x, deff, weight, stride, pad, dim_o, c0, c1):
        """conv2d_rows for output channels [c0, c1) only -> [batch, c1 - c0, Ho, Wo, dim_o + 1] (include/dctfhe.h dctfhe_conv2d_rows_window:
        launched in pixel chunks, so never refused for its pixel count)"""
        x, weight = np.ascontiguousarray(x, np.uint64), np.ascontiguousarray(weight, np.int8)
        B, Cin, H, W, L = x.shape
        Cout, _, KH, KW = weight.shape
        Ho, Wo = (max(H + 2 * pad - KH, 0) // max(stride, 1) + 1, max(W + 2 * pad - KW, 0) // max(stride, 1) + 1)   # the library checks the geometry
        out = np.empty((B, max(c1 - c0, 0), Ho, Wo, max(dim_o, 0) + 1), np.uint64)
        check(self.L.dctfhe_conv2d_rows_window(self.h, ptr(x), L - 1, deff, B, Cin, H, W, ptr(weight), Cout, KH, KW, stride, pad, dim_o, c0, c1, ptr(out)))
        return out

    def expand_seeded(self, sc, dim=None):
        """SeededCiphertexts -> rows of dim mask words + body (None: sc.input_dim, the compact wire form of ClientKey.encrypt)"""
        dim = sc.input_dim if dim is None else int(dim)
        out = np.empty((sc.bodies.size, dim + 1), np.uint64)
        check(self.L.dctfhe_expand_seeded(self.h, sc.key, C.c_uint64(sc.stream), sc.D, sc.input_dim, ptr(sc.bodies), sc.bodies.size, dim, ptr(out)))
        return out

    def ring_extract(self, logN, words=None, count=None, dim=None):
        """server primitive (dctfhe_ring_extract): wire words of `count` public-key inputs (or a PublicInputs: ring_extract(pi, dim=...))
        -> LWE rows [count, dim + 1] under the first 2^logN bits of the big key; dim None: 2^logN, the tightest row"""
        if isinstance(logN, PublicInputs):
            logN, words, count = logN.logN, logN.words, len(logN)
        words = np.ascontiguousarray(words, np.uint64).reshape(-1)
        count = int(count)
        dim = (1 << int(logN)) if dim is None else int(dim)
        if 5 <= int(logN) <= 12 and words.size != PublicInputs.n_words(logN, count):
            raise ValueError(f"{words.size} words are not {count} public-key inputs in rings of {1 << logN}")
        out = np.empty((count, max(dim, 0) + 1), np.uint64)
        check(self.L.dctfhe_ring_extract(self.h, int(logN), ptr(words), count, dim, ptr(out)))
        return out

    def decompress_bsk(self, blob, tier):
        """test view: the standard-domain bootstrap key of `tier` as importing a compressed blob rebuilds it"""
        blob = _as_u8(blob)
        p = blob_params(blob)
        t = p.tiers[tier]
        blocks = 3 * t.n // 2 if t.unroll == 2 else t.n
        out = np.empty((blocks, (t.k + 1) * t.l, t.k + 1, 1 << t.logN), np.uint64)
        check(self.L.dctfhe_eval_keys_decompress_bsk(self.h, ptr(blob), blob.size, tier, ptr(out)))
        return out

    def close(self):
        if self.h:
            self.L.dctfhe_ctx_destroy(self.h)
            self.h = C.c_void_p()


def key_tiers_arg(tiers):
    """a tier selection as the library's struct: a compile.KeyTierSelection (.bsk_mask / .ksk_mask), a KeyTiers of either binding or a
    (bsk, ksk) pair of bit masks"""
    bsk, ksk = (tiers.bsk_mask, tiers.ksk_mask) if hasattr(tiers, "bsk_mask") else (tiers.bsk, tiers.ksk) if hasattr(tiers, "bsk") else tiers
    return KeyTiers(int(bsk), int(ksk))


def key_tiers_all(params):
    """every key of a parameter set (dctfhe_key_tiers_all; host-only)"""
    t = KeyTiers()
    check(_lib.load().dctfhe_key_tiers_all(C.byref(params), C.byref(t)))
    return t


def key_tiers_close(params, tiers):
    """the closed selection: the owner of the key-switch key of every tier that bootstraps is added (dctfhe_key_tiers_close; host-only).
    Refused: a bit at or beyond n_tiers, a ksk bit on a tier that shares its key-switch key."""
    t = key_tiers_arg(tiers)
    check(_lib.load().dctfhe_key_tiers_close(C.byref(params), C.byref(t)))
    return t


def key_tiers_for_circuit(blob, params):
    """the closed selection a circuit blob needs under `params` (dctfhe_key_tiers_for_circuit; host-only)"""
    blob, t = bytes(blob), KeyTiers()
    check(_lib.load().dctfhe_key_tiers_for_circuit(blob, len(blob), C.byref(params), C.byref(t)))
    return t


def key_tiers_blob_bytes(params, tiers, compressed):
    """bytes of the full-form (compressed False) or compressed evaluation-key blob under a closed selection (host-only)"""
    n = C.c_size_t()
    check(_lib.load().dctfhe_key_tiers_blob_bytes(C.byref(params), C.byref(key_tiers_arg(tiers)), int(bool(compressed)), C.byref(n)))
    return n.value


def blob_params(blob):
    """the parameters in an evaluation-key blob's header (magic, version, total_bytes, params: both the full and the compressed form)"""
    blob = _as_u8(blob)
    if blob.size < 16 + C.sizeof(Params):
        raise _lib.DctfheError("evaluation-key blob too short")
    return Params.from_buffer_copy(blob[16:16 + C.sizeof(Params)].tobytes())


def blob_key_tiers(blob):
    """(bsk mask, ksk mask) of an evaluation-key blob of any of the four kinds, read from its header alone (no library call, no check:
    dctfhe_eval_keys_import validates).  The unpruned versions hold every key of their parameters."""
    blob = _as_u8(blob)
    params = blob_params(blob)
    magic, version = struct.unpack_from("<4sI", blob[:8].tobytes())
    pruned, at = {b"DEVK": (4, 16 + C.sizeof(Params)), b"DEVC": (2, 16 + C.sizeof(Params) + 32)}.get(magic, (None, 0))
    if version == pruned:
        if blob.size < at + 8:
            raise _lib.DctfheError("evaluation-key blob too short for its tier selection")
        return struct.unpack_from("<II", blob[at:at + 8].tobytes())
    n = max(0, min(int(params.n_tiers), _lib.MAX_TIERS))
    return (1 << n) - 1, sum(1 << i for i in range(n) if params.tiers[i].ksk_share < 0)


class PackKey:
    """Server side of ring packing (dctfhe_pack_key): the client's packing key, expanded on the GPU from its seeded blob."""

    def __init__(self, ctx, blob):
        self.ctx, self.L = ctx, ctx.L
        blob = _as_u8(blob)
        self.h = C.c_void_p()
        check(self.L.dctfhe_pack_key_import(ctx.h, ptr(blob), blob.size, C.byref(self.h)))
        a, b, c, d, e = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(self.L.dctfhe_pack_key_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        self.logN, self.l, self.beta, self.n_max, self.sigma = a.value, b.value, c.value, d.value, e.value

    def export_rows(self):
        """test view: the expanded key [n_max, l, 2, N_p] (mask, body)"""
        out = np.empty((self.n_max, self.l, 2, 1 << self.logN), np.uint64)
        check(self.L.dctfhe_pack_key_export_rows(self.h, ptr(out)))
        return out

    def ring_pack(self, cts_small):
        """small ciphertexts [count, n + 1] -> PackedRing (dctfhe_ring_pack)"""
        cts = np.ascontiguousarray(cts_small, np.uint64)
        count, n = cts.shape[0], cts.shape[1] - 1
        out = np.empty(PackedRing.n_words(self.logN, count), np.uint16)
        check(self.L.dctfhe_ring_pack(self.ctx.h, self.h, ptr(cts), count, n, ptr(out)))
        return PackedRing(self.logN, count, out)

    def close(self):
        if self.h:
            self.L.dctfhe_pack_key_destroy(self.h)
            self.h = C.c_void_p()


class PublicKey:
    """Data-owner side of public-key inputs (dctfhe_public_key): the client's public key, expanded on the GPU from its seeded blob, and
    the handle's own generator key (32 bytes from the OS).  Encrypts; can decrypt nothing."""

    def __init__(self, ctx, blob):
        self.ctx, self.L = ctx, ctx.L
        blob = _as_u8(blob)
        self.h = C.c_void_p()
        check(self.L.dctfhe_public_key_import(ctx.h, ptr(blob), blob.size, C.byref(self.h)))
        a, b = C.c_int(), C.c_double()
        check(self.L.dctfhe_public_key_info(self.h, C.byref(a), C.byref(b)))
        self.logN, self.sigma = a.value, b.value

    @property
    def N(self):
        return 1 << self.logN

    def export_rows(self):
        """test view: the expanded key [2, N_e] (A, B)"""
        out = np.empty((2, self.N), np.uint64)
        check(self.L.dctfhe_public_key_export_rows(self.h, ptr(out)))
        return out

    def set_encrypt_seed(self, seed32):
        """FIX the generator key the handle drew from the OS and restart its call counter -- reproducible tests only"""
        seed32 = bytes(seed32)
        if len(seed32) != 32:
            raise ValueError("an encryption seed is exactly 32 bytes")
        check(self.L.dctfhe_public_key_set_encrypt_seed(self.h, seed32))

    def draws(self, call, count):
        """test view: what call `call` draws for `count` phases -> (u uint8 [groups N_e], e1 int64 [groups N_e], e2 int64 [count])"""
        count = int(count)
        nmask = -(-count // self.N) * self.N
        u, e1, e2 = np.empty(nmask, np.uint8), np.empty(nmask, np.int64), np.empty(max(count, 0), np.int64)
        check(self.L.dctfhe_public_key_draws(self.h, int(call), count, ptr(u), ptr(e1), ptr(e2)))
        return u, e1, e2

    def encrypt(self, phases):
        """phases (uint64, any shape, taken flat) -> PublicInputs; one step of the handle's call counter"""
        phases = np.ascontiguousarray(phases, np.uint64).reshape(-1)
        out = np.empty(PublicInputs.n_words(self.logN, phases.size), np.uint64)
        check(self.L.dctfhe_encrypt_public(self.ctx.h, self.h, ptr(phases), phases.size, ptr(out)))
        return PublicInputs(self.logN, phases.size, out)

    def close(self):
        if self.h:
            self.L.dctfhe_public_key_destroy(self.h)
            self.h = C.c_void_p()


class ClientKey:
    """Secret side (include/dctfhe.h dctfhe_client_key): encrypts, decrypts, generates evaluation keys."""

    def __init__(self, ctx, params, seed=None):
        self.ctx, self.params, self.L = ctx, params, ctx.L
        self.seed = seed_bytes(seed)
        self.h = C.c_void_p()
        check(self.L.dctfhe_client_key_create(ctx.h, C.byref(params), self.seed, C.byref(self.h)))

    @property
    def D(self):
        return self.params.D

    def tier(self, i):
        return self.params.tiers[i]

    def generate_eval_keys(self, tiers=None):
        """tiers: a tier selection (key_tiers_arg); None: every tier.  Unselected keys are not generated at all."""
        h = C.c_void_p()
        if tiers is None:
            check(self.L.dctfhe_eval_keys_generate(self.h, C.byref(h)))
        else:
            check(self.L.dctfhe_eval_keys_generate_tiers(self.h, C.byref(key_tiers_arg(tiers)), C.byref(h)))
        return EvalKeys(self.ctx, self.params, h)

    def export_secret(self):
        S = np.empty(self.params.D, np.uint8)
        s = np.empty(self.params.n_max, np.uint8)
        check(self.L.dctfhe_client_key_export_secret(self.h, ptr(S), ptr(s)))
        return S, s

    def export_bsk(self, tier):
        t = self.tier(tier)
        blocks = 3 * t.n // 2 if t.unroll == 2 else t.n        # unroll 2: the key of the pair secret
        out = np.empty((blocks, (t.k + 1) * t.l, t.k + 1, 1 << t.logN), np.uint64)
        check(self.L.dctfhe_client_key_export_bsk(self.h, tier, ptr(out)))
        return out

    def set_encrypt_counter(self, next_call):
        """position inside this handle's own encryption streams (handles already differ by their nonce: include/dctfhe.h)"""
        check(self.L.dctfhe_client_key_set_encrypt_counter(self.h, next_call))

    def set_encrypt_nonce(self, nonce16):
        """FIX the 128-bit encryption nonce the handle drew from the OS -- reproducible tests / experiments only"""
        nonce16 = bytes(nonce16)
        if len(nonce16) != 16:
            raise ValueError("an encryption nonce is exactly 16 bytes")
        check(self.L.dctfhe_client_key_set_encrypt_nonce(self.h, nonce16))

    @property
    def input_dim(self):
        """mask words of a fresh encryption (the compact row width of a circuit input)"""
        return self.params.input_dim or self.params.D

    def encrypt(self, phases, dim=None):
        """-> rows of dim mask words + body; dim None: the full-width form (D + 1 words), dim = self.input_dim: the compact wire form"""
        phases = np.ascontiguousarray(phases, np.uint64).reshape(-1)
        dim = self.D if dim is None else int(dim)
        out = np.empty((phases.size, dim + 1), np.uint64)
        check(self.L.dctfhe_encrypt_rows(self.ctx.h, self.h, ptr(phases), phases.size, dim, ptr(out)))
        return out

    def encrypt_seeded(self, phases):
        """-> SeededCiphertexts: what encrypt(phases, self.input_dim) would return at this counter, masks left to the server"""
        phases = np.ascontiguousarray(phases, np.uint64).reshape(-1)
        key, stream = C.create_string_buffer(32), C.c_uint64()
        bodies = np.empty(phases.size, np.uint64)
        check(self.L.dctfhe_encrypt_seeded(self.ctx.h, self.h, ptr(phases), phases.size, key, C.byref(stream), ptr(bodies)))
        return SeededCiphertexts(key.raw, stream.value, self.D, self.input_dim, bodies)

    def export_eval_keys_compressed(self, tiers=None):
        """the evaluation keys as a compressed blob (bodies + the public mask key; EvalKeys.from_blob reads it).
        tiers: a tier selection (key_tiers_arg); None: every tier, today's bytes"""
        sel = None if tiers is None else C.byref(key_tiers_arg(tiers))
        n = C.c_size_t()
        check(self.L.dctfhe_eval_keys_export_compressed_tiers(self.h, sel, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        check(self.L.dctfhe_eval_keys_export_compressed_tiers(self.h, sel, ptr(out), out.size, C.byref(n)))
        return out

    def decrypt(self, cts, dim=None):
        dim = self.D if dim is None else int(dim)
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, dim + 1)
        out = np.empty(cts.shape[0], np.uint64)
        check(self.L.dctfhe_decrypt_rows(self.ctx.h, self.h, ptr(cts), cts.shape[0], dim, ptr(out)))
        return out

    def decrypt_packed(self, packed):
        """PackedCiphertexts -> phases (phase16 << 48: QuantizedModule.decode_output reads them like decrypt's)"""
        out = np.empty(len(packed), np.uint64)
        check(self.L.dctfhe_decrypt_packed(self.ctx.h, self.h, packed.n, ptr(packed.rows), len(packed), ptr(out)))
        return out

    def export_pack_key(self, spec):
        """the packing key for ring-packed results as its seeded blob (dctfhe_pack_key_export); spec: params.PackSpec"""
        n = C.c_size_t()
        args = (self.h, int(spec.logN), int(spec.l), int(spec.beta), float(spec.sigma))
        check(self.L.dctfhe_pack_key_export(*args, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        check(self.L.dctfhe_pack_key_export(*args, ptr(out), out.size, C.byref(n)))
        return out

    def export_public_key(self, spec):
        """the public key of public-key inputs as its seeded blob (dctfhe_public_key_export); spec: params.PublicInputSpec"""
        n = C.c_size_t()
        args = (self.h, int(spec.logN), float(spec.sigma))
        check(self.L.dctfhe_public_key_export(*args, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        check(self.L.dctfhe_public_key_export(*args, ptr(out), out.size, C.byref(n)))
        return out

    def decrypt_ring(self, ring):
        """PackedRing -> phases (phase16 << 48), one per result"""
        out = np.empty(len(ring), np.uint64)
        check(self.L.dctfhe_decrypt_ring(self.ctx.h, self.h, ring.logN, ptr(ring.words), len(ring), ptr(out)))
        return out

    def margin_probe(self, tier, cts_small, table_bits, want_err=True, want_stats=True):
        """the margin audit's kernel on small ciphertexts [count, n + 1] of `tier`, already key-switched and mod-switched, about to meet
        a table of table_bits input bits (dctfhe_margin_probe): (signed distance from the box centre per ciphertext, in levels of 2N,
        or None; statistics dict or None)"""
        cts = np.ascontiguousarray(cts_small, np.uint64)
        n = self.tier(tier).n if 0 <= tier < self.params.n_tiers else 0      # the library refuses the rest
        count = cts.size // (n + 1)
        err = np.empty(count, np.int32) if want_err else None
        st = MarginStats() if want_stats else None
        check(self.L.dctfhe_margin_probe(self.ctx.h, self.h, int(tier), ptr(cts), count, int(table_bits), None if err is None else ptr(err),
                                         None if st is None else C.byref(st)))
        return err, (None if st is None else margin_stats_dict(st))

    def close(self):
        if self.h:
            self.L.dctfhe_client_key_destroy(self.h)
            self.h = C.c_void_p()


class EvalKeys:
    """Server side (dctfhe_eval_keys): key-switch keys + Fourier bootstrap keys; all the evaluation needs."""

    def __init__(self, ctx, params, handle):
        self.ctx, self.params, self.L, self.h = ctx, params, ctx.L, handle

    @classmethod
    def from_blob(cls, ctx, blob):
        """evaluation keys as shipped by a client, full (EvalKeys.to_blob) or compressed (ClientKey.export_eval_keys_compressed):
        the server never sees a secret"""
        blob = _as_u8(blob)
        params = blob_params(blob)
        h = C.c_void_p()
        check(ctx.L.dctfhe_eval_keys_import(ctx.h, ptr(blob), blob.size, C.byref(h)))
        return cls(ctx, params, h)

    @property
    def tiers(self):
        """the tier selection this handle holds (KeyTiers: bsk and ksk bit masks over the tier indices)"""
        t = KeyTiers()
        check(self.L.dctfhe_eval_keys_tiers(self.h, C.byref(t)))
        return t

    def to_blob(self):
        """the full-form blob; of a pruned handle, a pruned blob"""
        n = C.c_size_t()
        check(self.L.dctfhe_eval_keys_export(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        check(self.L.dctfhe_eval_keys_export(self.h, ptr(out), out.size, C.byref(n)))
        return out

    @property
    def D(self):
        return self.params.D

    def tier(self, i):
        return self.params.tiers[i]

    def export_ksk(self, tier):
        t = self.tier(tier)
        out = np.empty((self.params.D, t.lk, t.n + 1), np.uint64)
        check(self.L.dctfhe_eval_keys_export_ksk(self.h, tier, ptr(out)))
        return out

    def keyswitch(self, tier, cts, shift=0, deff=0):
        """deff > 0: the caller knows every mask word beyond deff to be zero (see dctfhe_keyswitch_prefix)"""
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, self.D + 1)
        out = np.empty((cts.shape[0], self.tier(tier).n + 1), np.uint64)
        check(self.L.dctfhe_keyswitch_prefix(self.ctx.h, self.h, tier, ptr(cts), cts.shape[0], shift, deff, ptr(out)))
        return out

    def keyswitch_pack(self, tier, cts, dim, deff=0):
        """rows of dim mask words + body -> PackedCiphertexts under tier's small key (dctfhe_keyswitch_pack); deff as in keyswitch"""
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, int(dim) + 1)
        n = self.tier(tier).n
        out = np.empty((cts.shape[0], n + 1), np.uint16)
        check(self.L.dctfhe_keyswitch_pack(self.ctx.h, self.h, tier, ptr(cts), cts.shape[0], int(dim), int(deff), ptr(out)))
        return PackedCiphertexts(n, out)

    def keyswitch_diff(self, tier, cts, ia, ib, shift=0, body_add=0, deff=0):
        """key switch of cts[ia[c]] - cts[ib[c]] (dctfhe_keyswitch_diff): small ciphertexts [len(ia), n + 1]"""
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, self.D + 1)
        ia, ib = np.ascontiguousarray(ia, np.int32), np.ascontiguousarray(ib, np.int32)
        if ia.size != cts.shape[0] or ib.size != cts.shape[0]:
            raise ValueError("keyswitch_diff takes one index pair per row")
        out = np.empty((cts.shape[0], self.tier(tier).n + 1), np.uint64)
        check(self.L.dctfhe_keyswitch_diff(self.ctx.h, self.h, tier, ptr(cts), cts.shape[0], ptr(ia), ptr(ib), shift, C.c_uint64(body_add), deff,
                                           ptr(out)))
        return out

    def modswitch_center(self, tier, cts_small):
        """centred mod switch (dctfhe_modswitch_center): the adjusted copy of small ciphertexts [count, n + 1]"""
        out = np.ascontiguousarray(cts_small, np.uint64).copy()
        check(self.L.dctfhe_modswitch_center(self.ctx.h, self.h, tier, ptr(out), out.shape[0]))
        return out

    def pbs(self, tier, cts_small, tables, w, table_idx=None):
        cts_small = np.ascontiguousarray(cts_small, np.uint64)
        tables = np.ascontiguousarray(tables, np.int64).reshape(-1, 1 << w)
        idx = None if table_idx is None else np.ascontiguousarray(table_idx, np.int32)
        out = np.empty((cts_small.shape[0], self.D + 1), np.uint64)
        check(self.L.dctfhe_pbs(self.ctx.h, self.h, tier, ptr(cts_small), cts_small.shape[0], ptr(tables), tables.shape[0], w,
                                None if idx is None else ptr(idx), ptr(out)))
        return out

    def pbs_rows(self, tier, cts_small, tables, w, rows, row0=0, table_idx=None, hw=1, nchan=1, e_offset=0, accumulate=False, body_add=0):
        """the bootstrap in the library's write-back modes (dctfhe_pbs_rows): the results of cts_small go to rows [row0, row0 + count) of a
        copy of `rows` [n_rows, dim_out + 1], stored or accumulated; the whole buffer comes back"""
        cts_small = np.ascontiguousarray(cts_small, np.uint64)
        tables = np.ascontiguousarray(tables, np.int64).reshape(-1, 1 << w)
        idx = None if table_idx is None else np.ascontiguousarray(table_idx, np.int32)
        if idx is not None and idx.size != cts_small.shape[0]:
            raise ValueError("pbs_rows takes one table index per ciphertext")
        out = np.ascontiguousarray(rows, np.uint64).copy()
        check(self.L.dctfhe_pbs_rows(self.ctx.h, self.h, tier, ptr(cts_small), cts_small.shape[0], ptr(tables), tables.shape[0], w,
                                     None if idx is None else ptr(idx), int(hw), int(nchan), C.c_size_t(int(e_offset)), ptr(out), out.shape[0], int(row0),
                                     out.shape[1] - 1, int(bool(accumulate)), C.c_uint64(int(body_add))))
        return out

    def keyswitch_sum(self, tier, rows_a, rows_b, shift=0, body_add=0, deff=0):
        """key switch of rows_a[c] + rows_b[c], rows [count, dim_a + 1] and [count, dim_b + 1] (dctfhe_keyswitch_sum)"""
        a, b = np.ascontiguousarray(rows_a, np.uint64), np.ascontiguousarray(rows_b, np.uint64)
        if a.shape[0] != b.shape[0]:
            raise ValueError("keyswitch_sum takes one row of b per row of a")
        out = np.empty((a.shape[0], self.tier(tier).n + 1), np.uint64)
        check(self.L.dctfhe_keyswitch_sum(self.ctx.h, self.h, tier, ptr(a), a.shape[1] - 1, ptr(b), b.shape[1] - 1, a.shape[0], shift,
                                          C.c_uint64(int(body_add)), deff, ptr(out)))
        return out

    def round_lut(self, bit_tier, tab_tier, cts, p, r, tables, w, table_idx=None):
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, self.D + 1)
        tables = np.ascontiguousarray(tables, np.int64).reshape(-1, 1 << w)
        idx = None if table_idx is None else np.ascontiguousarray(table_idx, np.int32)
        out = np.empty_like(cts)
        check(self.L.dctfhe_round_lut(self.ctx.h, self.h, bit_tier, tab_tier, ptr(cts), cts.shape[0], p, r, ptr(tables),
                                      tables.shape[0], w, None if idx is None else ptr(idx), ptr(out)))
        return out

    def round_lut_split(self, bit_tier, tab_tier, tab_tier2, cts, p, r, tables, w, table_idx=None):
        """parity split of a w-bit table: the half-table look-ups run on tab_tier and tab_tier2 (dctfhe_round_lut_split)"""
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, self.D + 1)
        tables = np.ascontiguousarray(tables, np.int64).reshape(-1, 1 << w)
        idx = None if table_idx is None else np.ascontiguousarray(table_idx, np.int32)
        out = np.empty_like(cts)
        check(self.L.dctfhe_round_lut_split(self.ctx.h, self.h, bit_tier, tab_tier, tab_tier2, ptr(cts), cts.shape[0], p, r, ptr(tables),
                                            tables.shape[0], w, None if idx is None else ptr(idx), ptr(out)))
        return out

    def bench_pbs(self, tier, count, reps=3):
        v = C.c_double()
        check(self.L.dctfhe_bench_pbs(self.ctx.h, self.h, tier, count, reps, C.byref(v)))
        return v.value

    def close(self):
        if self.h:
            self.L.dctfhe_eval_keys_destroy(self.h)
            self.h = C.c_void_p()


class Keys:
    """Both halves in one process (tests, benchmarks, the reference's single-machine flow homomorphic_eval.py:313-317):
    `.client` (ClientKey) and `.eval` (EvalKeys); every method is the half's own."""

    def __init__(self, ctx, params, seed=None, client=None, evalk=None, tiers=None):
        self.ctx, self.params = ctx, params
        self.client = client if client is not None else ClientKey(ctx, params, seed)
        self.eval = evalk if evalk is not None else self.client.generate_eval_keys(tiers)

    @classmethod
    def generate(cls, ctx, params, seed=None, tiers=None):
        """both halves from a seed; tiers: a tier selection for the evaluation keys (key_tiers_arg; None: every tier)"""
        return cls(ctx, params, seed=seed, tiers=tiers)

    @property
    def D(self):
        return self.params.D

    def tier(self, i):
        return self.params.tiers[i]

    def __getattr__(self, name):
        if name in ("export_secret", "export_bsk", "encrypt", "decrypt", "seed", "input_dim", "set_encrypt_nonce", "set_encrypt_counter",
                    "encrypt_seeded", "export_eval_keys_compressed", "decrypt_packed", "margin_probe", "export_pack_key", "decrypt_ring",
                    "export_public_key"):
            return getattr(self.client, name)
        if name in ("export_ksk", "keyswitch", "keyswitch_pack", "keyswitch_diff", "keyswitch_sum", "modswitch_center", "pbs", "pbs_rows", "round_lut", "round_lut_split", "bench_pbs", "to_blob", "tiers"):
            return getattr(self.eval, name)
        raise AttributeError(name)

    def close(self):
        self.eval.close()
        self.client.close()


def shard_rows(rows, parts, part):
    """(first, count) of part `part`'s rows of a tensor of `rows` rows: the library's partition rule (dctfhe_shard_rows; host-only)"""
    f, n = C.c_size_t(), C.c_size_t()
    check(_lib.load().dctfhe_shard_rows(int(rows), int(parts), int(part), C.byref(f), C.byref(n)))
    return f.value, n.value


def shard_pool(batch, C_, H, W, k, s, pad, parts, part):
    """(out_first, out_count, in_first, in_count, pairs) of part `part` of a divided max pool: its output rows, the source rows it needs
    and the pairwise maxima it runs (dctfhe_shard_pool; host-only; dctfhe.compile.shard_pool is the same rule)"""
    v = [C.c_size_t() for _ in range(5)]
    check(_lib.load().dctfhe_shard_pool(*(int(x) for x in (batch, C_, H, W, k, s, pad, parts, part)), *(C.byref(x) for x in v)))
    return tuple(x.value for x in v)


def memory_plan(blob, params=None, batch=1, budget_bytes=None):
    """The session planner on the host (dctfhe_memory_plan; no context, no GPU): the bytes a session of `batch` images allocates for
    itself, undivided and under `budget_bytes` (None: no budget), and per slab group its op range, channels and slab height.  params: a
    ctypes Params (None: a clear-mode session).  Refused, naming an op, when one channel at a time everywhere still exceeds the budget."""
    blob, m = bytes(blob), MemPlan()
    check(_lib.load().dctfhe_memory_plan(blob, len(blob), None if params is None else C.byref(params), int(batch), int(budget_bytes or 0), C.byref(m)))
    return m.record()


class Circuit:
    def __init__(self, ctx, blob):
        self.ctx, self.L = ctx, ctx.L
        self.h = C.c_void_p()
        self._blob = bytes(blob)
        check(self.L.dctfhe_circuit_load(ctx.h, self._blob, len(self._blob), C.byref(self.h)))
        a, b = C.c_int64(), C.c_int64()
        check(self.L.dctfhe_circuit_io(self.h, C.byref(a), C.byref(b)))
        self.n_in, self.n_out = a.value, b.value

    def stats(self, params):
        s = Stats()
        check(self.L.dctfhe_circuit_stats(self.h, C.byref(params), C.byref(s)))
        return s

    def close(self):
        if self.h:
            self.L.dctfhe_circuit_destroy(self.h)
            self.h = C.c_void_p()


class Session:
    """Device tensors for one (circuit, keys, batch).  keys=None: noise-free clear mode (1-word ciphertexts)."""

    def __init__(self, ctx, circuit, keys, batch):
        """keys: EvalKeys (or a Keys pair, whose evaluation half is used) -- a session never needs the secret"""
        keys = getattr(keys, "eval", keys)
        self.ctx, self.circuit, self.keys, self.batch, self.L = ctx, circuit, keys, batch, ctx.L
        self.words = (keys.D + 1) if keys is not None else 1
        self.h = C.c_void_p()
        check(self.L.dctfhe_session_create(ctx.h, circuit.h, keys.h if keys is not None else None, batch, C.byref(self.h)))

    def dims(self):
        """(input, output) effective dimensions: the compact row widths of this session's circuit (0, 0 in clear mode)"""
        a, b = C.c_int(), C.c_int()
        check(self.L.dctfhe_session_dims(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def upload(self, cts, dim=None):
        """dim None: rows of D + 1 words (1 in clear mode); else the compact wire form, rows of dim mask words + body"""
        cts = np.ascontiguousarray(cts, np.uint64)
        words = self.words if (dim is None or self.keys is None) else dim + 1
        assert cts.size == self.batch * self.circuit.n_in * words, (cts.shape, self.batch, self.circuit.n_in, words)
        if dim is None or self.keys is None:
            check(self.L.dctfhe_session_upload(self.h, ptr(cts)))
        else:
            check(self.L.dctfhe_session_upload_rows(self.h, ptr(cts), int(dim)))

    def upload_seeded(self, sc):
        """SeededCiphertexts of batch x n_in inputs: the bodies go to the device, the masks are regenerated there"""
        if self.keys is not None and sc.D != self.keys.D:
            raise ValueError(f"seeded ciphertexts under D = {sc.D}, the session's keys have D = {self.keys.D}")
        check(self.L.dctfhe_session_upload_seeded(self.h, sc.key, C.c_uint64(sc.stream), sc.input_dim, ptr(sc.bodies), sc.bodies.size))

    def upload_public(self, pi):
        """PublicInputs of batch x n_in inputs: the wire words go to the device, k_pk_extract writes the rows into the input tensor"""
        check(self.L.dctfhe_session_upload_public(self.h, pi.logN, ptr(pi.words), len(pi)))

    def set_noise(self, seed, sigma_per_op):
        """clear-mode sessions: `simulate` with the noise model (sigma per op, fraction of the torus); None switches it off"""
        if sigma_per_op is None:
            check(self.L.dctfhe_session_set_noise(self.h, 0, None, 0))
            return
        sg = np.ascontiguousarray(sigma_per_op, np.float64)
        check(self.L.dctfhe_session_set_noise(self.h, seed, ptr(sg), sg.size))

    def set_noise_split(self, sigma2_per_op):
        """the noise std at the SECOND look-up of parity-split sites (one per op, 0 elsewhere); None: the first look-up's"""
        if sigma2_per_op is None:
            check(self.L.dctfhe_session_set_noise_split(self.h, None, 0))
            return
        sg = np.ascontiguousarray(sigma2_per_op, np.float64)
        check(self.L.dctfhe_session_set_noise_split(self.h, ptr(sg), sg.size))

    def run(self, timing=False):
        t = Timing() if timing else None
        check(self.L.dctfhe_session_run(self.h, C.byref(t) if timing else None))
        return t

    # -- bounded device memory (include/dctfhe.h dctfhe_session_set_memory_budget) ---------------------------------------------------
    def set_memory_budget(self, budget_bytes):
        """plan the session's buffers under `budget_bytes` (0 / None: no budget): slab groups are walked in channel slabs, no output word
        changes.  Before the first run; never sharded, never with the margin audit; a refused budget leaves the session as it was"""
        check(self.L.dctfhe_session_set_memory_budget(self.h, int(budget_bytes or 0)))

    def set_slab_heights(self, heights):
        """plan the session at these slab heights, one per slab group (dctfhe_session_set_slab_heights): for tests and experiments"""
        h = np.ascontiguousarray(heights, np.int32)
        check(self.L.dctfhe_session_set_slab_heights(self.h, ptr(h), h.size))

    def memory_plan(self):
        """the plan in force (dctfhe_session_memory_plan): planned bytes, undivided and as planned, and the slab height per group"""
        m = MemPlan()
        check(self.L.dctfhe_session_memory_plan(self.h, C.byref(m)))
        return m.record()

    # -- sharded look-up sites (include/dctfhe.h dctfhe_session_set_shard): one image over several sessions, one per GPU ----------
    def set_shard(self, part, parts):
        """this session evaluates part `part` of `parts` of every look-up and add; (0, 1) is the plain run.  Before the first run only"""
        check(self.L.dctfhe_session_set_shard(self.h, int(part), int(parts)))

    def run_span(self, first_op, end_op, timing=False):
        """ops [first_op, end_op) in order (dctfhe_session_run_span); refused at an op that needs a whole tensor which is still sliced"""
        t = Timing() if timing else None
        check(self.L.dctfhe_session_run_span(self.h, int(first_op), int(end_op), C.byref(t) if timing else None))
        return t

    def shard_plan(self):
        """the exchange points [(after_op, tensor)] in op order (dctfhe_session_shard_plan; CompiledCircuit.shard_plan is the same list)"""
        n = C.c_int()
        check(self.L.dctfhe_session_shard_plan(self.h, None, None, 0, C.byref(n)))
        a, t = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
        check(self.L.dctfhe_session_shard_plan(self.h, ptr(a), ptr(t), n.value, C.byref(n)))
        return [(int(x), int(y)) for x, y in zip(a, t)]

    def set_shard_pool(self, on=True):
        """divide the max pools too: each computes this part's outputs from its need range of the source and leaves its destination
        sliced (dctfhe_session_set_shard_pool).  After set_shard, before the first run, never with the margin audit"""
        check(self.L.dctfhe_session_set_shard_pool(self.h, 1 if on else 0))

    def shard_plan_rows(self):
        """the exchange points with the rows this part needs of each [(after_op, tensor, first, count)]: a divided pool's need range, else
        the whole tensor (dctfhe_session_shard_plan_rows; CompiledCircuit.shard_plan(rows=True, ...) is the same list)"""
        n = C.c_int()
        check(self.L.dctfhe_session_shard_plan_rows(self.h, None, None, None, None, 0, C.byref(n)))
        a, t = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
        f, c = np.empty(n.value, np.uintp), np.empty(n.value, np.uintp)
        check(self.L.dctfhe_session_shard_plan_rows(self.h, ptr(a), ptr(t), ptr(f), ptr(c), n.value, C.byref(n)))
        return [tuple(int(x) for x in e) for e in zip(a, t, f, c)]

    def mark_rows(self, tensor, first, count):
        """rows [first, first + count) of `tensor` have been brought into this session (dctfhe_session_mark_rows)"""
        check(self.L.dctfhe_session_mark_rows(self.h, int(tensor), int(first), int(count)))

    def pool_pairs(self, op):
        """pairwise maxima the last run of max-pool op `op` sent to the bootstrap (dctfhe_session_pool_pairs)"""
        n = C.c_size_t()
        check(self.L.dctfhe_session_pool_pairs(self.h, int(op), C.byref(n)))
        return n.value

    def tensor(self, tensor):
        """(device pointer, stored row stride in 64-bit words, rows) of a tensor of the circuit (dctfhe_session_tensor)"""
        dev, L, rows = C.c_void_p(), C.c_size_t(), C.c_size_t()
        check(self.L.dctfhe_session_tensor(self.h, int(tensor), C.byref(dev), C.byref(L), C.byref(rows)))
        return dev.value, L.value, rows.value

    def mark_whole(self, tensor):
        """every part's rows of `tensor` are in place in this session (dctfhe_session_mark_whole)"""
        check(self.L.dctfhe_session_mark_whole(self.h, int(tensor)))

    def copy_rows_from(self, src, tensor, first, count):
        """rows [first, first + count) of `tensor` from session `src` (same circuit, batch and mode), device to device: the loopback
        exchange of parts that share a process (dctfhe_session_copy_rows)"""
        check(self.L.dctfhe_session_copy_rows(self.h, src.h, int(tensor), int(first), int(count)))

    def download(self, dim=None):
        if dim is None or self.keys is None:
            out = np.empty((self.batch, self.circuit.n_out, self.words), np.uint64)
            check(self.L.dctfhe_session_download(self.h, ptr(out)))
        else:
            out = np.empty((self.batch, self.circuit.n_out, dim + 1), np.uint64)
            check(self.L.dctfhe_session_download_rows(self.h, ptr(out), int(dim)))
        return out

    def set_audit(self, client):
        """margin audit (dctfhe_session_set_audit): client -- a ClientKey, or a Keys pair whose client half is used -- turns it on for the
        following runs, None turns it off.  The session keeps its own copy of the small key; it needs the SECRET, so this is a
        development and assurance tool, never a server path"""
        client = getattr(client, "client", client)
        if type(client).__name__ == "HostClientKey":
            raise _lib.DctfheError("set_audit: the margin audit reads the small key from a device ClientKey; a HostClientKey (device=\"host\") "
                                   "has none -- make the audit's key with ClientKey(ctx, params, seed) from the same seed")
        check(self.L.dctfhe_session_set_audit(self.h, None if client is None else client.h))

    def audit(self):
        """the slots of the last run (dctfhe_session_audit): a list of dicts, empty when the audit is off"""
        n = C.c_int()
        check(self.L.dctfhe_session_audit(self.h, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        out = (MarginStats * n.value)()
        check(self.L.dctfhe_session_audit(self.h, out, n.value, C.byref(n)))
        return [margin_stats_dict(m) for m in out]

    def download_packed(self, tier):
        """the outputs key-switched to `tier` and packed to 16 bits per word (dctfhe_session_download_packed): PackedCiphertexts of
        batch x n_out rows; encrypted sessions only"""
        n = self.keys.tier(tier).n if (self.keys is not None and 0 <= tier < self.keys.params.n_tiers) else 0      # the library refuses the rest
        out = np.empty((self.batch * self.circuit.n_out, n + 1), np.uint16)
        check(self.L.dctfhe_session_download_packed(self.h, int(tier), ptr(out)))
        return PackedCiphertexts(n, out)

    def download_ring(self, tier, pack_key):
        """the outputs key-switched to `tier` and ring-packed with the client's packing key (dctfhe_session_download_ring): a PackedRing
        of batch x n_out results; encrypted sessions only"""
        count = self.batch * self.circuit.n_out
        out = np.empty(PackedRing.n_words(pack_key.logN, count), np.uint16)
        check(self.L.dctfhe_session_download_ring(self.h, int(tier), pack_key.h, ptr(out)))
        return PackedRing(pack_key.logN, count, out)

    def close(self):
        if self.h:
            self.L.dctfhe_session_destroy(self.h)
            self.h = C.c_void_p()
