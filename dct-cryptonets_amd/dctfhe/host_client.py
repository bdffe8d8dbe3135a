"""The key owner and the data owner WITHOUT a GPU: HostClientKey and HostPublicKey over libdctfhe_client.so (include/dctfhe_client.h).

They offer the methods of engine.ClientKey / engine.PublicKey that dctfhe.roles and dctfhe.deploy call and return the same wire objects
(dctfhe.wire), so a role runs on either.  Blobs made here import into the GPU engine and ciphertexts made there decrypt here: secret
bits, masks and every decryption are equal word for word, a noise term may differ from the device's by one unit of 2^-64
(include/dctfhe_client.h, "The Gaussian").  Threads follow OMP_NUM_THREADS.

Not here: the full (Fourier) evaluation-key export, the standard-domain bootstrap-key view and the margin audit -- server and
development paths that stay on the GPU."""
import ctypes as C

import numpy as np

from . import _lib_client
from ._lib_client import Params, check, ptr
from .wire import PackedCiphertexts, PackedRing, PublicInputs, SeededCiphertexts, _as_u8, seed_bytes  # noqa: F401


def host_params(params):
    """a dctfhe_params of either binding (dctfhe._lib.Params has the same layout) as this binding's Params"""
    return params if isinstance(params, Params) else Params.from_buffer_copy(bytes(params))


def _export(fn, *args):
    """the size-query convention: buf == NULL, then the caller's buffer"""
    n = C.c_size_t()
    check(fn(*args, None, 0, C.byref(n)))
    out = np.empty(n.value, np.uint8)
    check(fn(*args, ptr(out), out.size, C.byref(n)))
    return out


class HostPublicKey:
    """Data-owner side of public-key inputs on the host (dctfhe_host_public_key): encrypts; can decrypt nothing."""

    def __init__(self, blob):
        self.L = _lib_client.load()
        blob = _as_u8(blob)
        self.h = C.c_void_p()
        check(self.L.dctfhe_host_public_key_import(ptr(blob), blob.size, C.byref(self.h)))
        a, b = C.c_int(), C.c_double()
        check(self.L.dctfhe_host_public_key_info(self.h, C.byref(a), C.byref(b)))
        self.logN, self.sigma = a.value, b.value

    @property
    def N(self):
        return 1 << self.logN

    def set_encrypt_seed(self, seed32):
        """FIX the generator key the handle drew from the OS and restart its call counter -- reproducible tests only"""
        seed32 = bytes(seed32)
        if len(seed32) != 32:
            raise ValueError("an encryption seed is exactly 32 bytes")
        check(self.L.dctfhe_host_public_key_set_encrypt_seed(self.h, seed32))

    def draws(self, call, count):
        """test view: what call `call` draws for `count` phases -> (u uint8 [groups N_e], e1 int64 [groups N_e], e2 int64 [count])"""
        count = int(count)
        nmask = -(-count // self.N) * self.N
        u, e1, e2 = np.empty(nmask, np.uint8), np.empty(nmask, np.int64), np.empty(max(count, 0), np.int64)
        check(self.L.dctfhe_host_public_key_draws(self.h, int(call), count, ptr(u), ptr(e1), ptr(e2)))
        return u, e1, e2

    def encrypt(self, phases):
        """phases (uint64, any shape, taken flat) -> PublicInputs; one step of the handle's call counter"""
        phases = np.ascontiguousarray(phases, np.uint64).reshape(-1)
        out = np.empty(PublicInputs.n_words(self.logN, phases.size), np.uint64)
        check(self.L.dctfhe_host_encrypt_public(self.h, ptr(phases), phases.size, ptr(out)))
        return PublicInputs(self.logN, phases.size, out)

    def close(self):
        if self.h:
            self.L.dctfhe_host_public_key_destroy(self.h)
            self.h = C.c_void_p()


class HostClientKey:
    """Secret side on the host (dctfhe_host_client_key): encrypts, decrypts, exports the compressed evaluation keys."""

    def __init__(self, params, seed=None):
        self.L = _lib_client.load()
        self.params = host_params(params)
        self.seed = seed_bytes(seed)
        self.h = C.c_void_p()
        check(self.L.dctfhe_host_client_key_create(C.byref(self.params), self.seed, C.byref(self.h)))

    @property
    def D(self):
        return self.params.D

    def tier(self, i):
        return self.params.tiers[i]

    @property
    def input_dim(self):
        """mask words of a fresh encryption (the compact row width of a circuit input)"""
        return self.params.input_dim or self.params.D

    def export_secret(self):
        S = np.empty(self.params.D, np.uint8)
        s = np.empty(self.params.n_max, np.uint8)
        check(self.L.dctfhe_host_client_key_export_secret(self.h, ptr(S), ptr(s)))
        return S, s

    def public_keys(self):
        """test view: (the public generator key the blobs carry, the public encryption key of encrypt_seeded), 32 bytes each"""
        a, b = C.create_string_buffer(32), C.create_string_buffer(32)
        check(self.L.dctfhe_host_client_key_public_keys(self.h, a, b))
        return a.raw, b.raw

    def set_encrypt_counter(self, next_call):
        check(self.L.dctfhe_host_client_key_set_encrypt_counter(self.h, next_call))

    def set_encrypt_nonce(self, nonce16):
        """FIX the 128-bit encryption nonce the handle drew from the OS -- reproducible tests / experiments only"""
        nonce16 = bytes(nonce16)
        if len(nonce16) != 16:
            raise ValueError("an encryption nonce is exactly 16 bytes")
        check(self.L.dctfhe_host_client_key_set_encrypt_nonce(self.h, nonce16))

    def encrypt(self, phases, dim=None):
        """-> rows of dim mask words + body; dim None: the full-width form (D + 1 words), dim = self.input_dim: the compact wire form"""
        phases = np.ascontiguousarray(phases, np.uint64).reshape(-1)
        dim = self.D if dim is None else int(dim)
        out = np.empty((phases.size, max(dim, 0) + 1), np.uint64)
        check(self.L.dctfhe_host_encrypt_rows(self.h, ptr(phases), phases.size, dim, ptr(out)))
        return out

    def encrypt_seeded(self, phases):
        """-> SeededCiphertexts: what encrypt(phases, self.input_dim) would return at this counter, masks left to the server"""
        phases = np.ascontiguousarray(phases, np.uint64).reshape(-1)
        key, stream = C.create_string_buffer(32), C.c_uint64()
        bodies = np.empty(phases.size, np.uint64)
        check(self.L.dctfhe_host_encrypt_seeded(self.h, ptr(phases), phases.size, key, C.byref(stream), ptr(bodies)))
        return SeededCiphertexts(key.raw, stream.value, self.D, self.input_dim, bodies)

    def decrypt(self, cts, dim=None):
        dim = self.D if dim is None else int(dim)
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, dim + 1)
        out = np.empty(cts.shape[0], np.uint64)
        check(self.L.dctfhe_host_decrypt_rows(self.h, ptr(cts), cts.shape[0], dim, ptr(out)))
        return out

    def decrypt_packed(self, packed):
        """PackedCiphertexts -> phases (phase16 << 48)"""
        out = np.empty(len(packed), np.uint64)
        check(self.L.dctfhe_host_decrypt_packed(self.h, packed.n, ptr(packed.rows), len(packed), ptr(out)))
        return out

    def decrypt_ring(self, ring):
        """PackedRing -> phases (phase16 << 48), one per result"""
        out = np.empty(len(ring), np.uint64)
        check(self.L.dctfhe_host_decrypt_ring(self.h, ring.logN, ptr(ring.words), len(ring), ptr(out)))
        return out

    def export_eval_keys_compressed(self, tiers=None):
        """the evaluation keys as a compressed blob (bodies + the public mask key; engine.EvalKeys.from_blob reads it on the server).
        tiers: a tier selection -- a compile.KeyTierSelection, a KeyTiers of either binding or a (bsk mask, ksk mask) pair; None: every
        tier.  The library closes it."""
        if tiers is None:
            return _export(self.L.dctfhe_host_eval_keys_export_compressed, self.h)
        bsk, ksk = (tiers.bsk_mask, tiers.ksk_mask) if hasattr(tiers, "bsk_mask") else (tiers.bsk, tiers.ksk) if hasattr(tiers, "bsk") else tiers
        return _export(self.L.dctfhe_host_eval_keys_export_compressed_tiers, self.h, C.byref(_lib_client.KeyTiers(int(bsk), int(ksk))))

    def export_pack_key(self, spec):
        """the packing key for ring-packed results as its seeded blob; spec: params.PackSpec"""
        return _export(self.L.dctfhe_host_pack_key_export, self.h, int(spec.logN), int(spec.l), int(spec.beta), float(spec.sigma))

    def export_public_key(self, spec):
        """the public key of public-key inputs as its seeded blob; spec: params.PublicInputSpec"""
        return _export(self.L.dctfhe_host_public_key_export, self.h, int(spec.logN), float(spec.sigma))

    def generate_eval_keys(self):
        raise _lib_client.DctfheHostError("the full (Fourier) evaluation keys are made on the GPU: the host client exports the compressed form "
                                          "(export_eval_keys_compressed), which the server transforms on import")

    def close(self):
        if self.h:
            self.L.dctfhe_host_client_key_destroy(self.h)
            self.h = C.c_void_p()
