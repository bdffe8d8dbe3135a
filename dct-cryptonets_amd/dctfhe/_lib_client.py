"""ctypes binding of libdctfhe_client.so (include/dctfhe_client.h): the key owner's and the data owner's side on the host.

The library is built in-tree by __graft_entry__.build() with the host compiler (no HIP, no device code) and lives at
dct-cryptonets_amd/libdctfhe_client.so.  This module imports neither dctfhe._lib nor torch: a client needs no GPU stack.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libdctfhe_client.so")
MAX_TIERS = 12


class Tier(C.Structure):
    """dctfhe_tier (include/dctfhe.h); the layout of dctfhe._lib.Tier"""
    _fields_ = [("n", C.c_int32), ("k", C.c_int32), ("logN", C.c_int32), ("l", C.c_int32), ("beta", C.c_int32),
                ("lk", C.c_int32), ("betak", C.c_int32), ("ksk_share", C.c_int32),
                ("unroll", C.c_int32), ("reserved", C.c_int32),
                ("lwe_sigma", C.c_double), ("glwe_sigma", C.c_double)]


class Params(C.Structure):
    """dctfhe_params (include/dctfhe.h); the layout of dctfhe._lib.Params"""
    _fields_ = [("D", C.c_int32), ("n_max", C.c_int32), ("n_tiers", C.c_int32), ("input_dim", C.c_int32),
                ("input_sigma", C.c_double), ("tiers", Tier * MAX_TIERS)]


class KeyTiers(C.Structure):
    """dctfhe_key_tiers (include/dctfhe.h); the layout of dctfhe._lib.KeyTiers"""
    _fields_ = [("bsk", C.c_uint32), ("ksk", C.c_uint32)]


EXPORTS = [
    "dctfhe_host_last_error", "dctfhe_host_version", "dctfhe_host_threads",
    "dctfhe_host_client_key_create", "dctfhe_host_client_key_destroy", "dctfhe_host_client_key_export_secret",
    "dctfhe_host_client_key_set_encrypt_counter", "dctfhe_host_client_key_set_encrypt_nonce", "dctfhe_host_client_key_public_keys",
    "dctfhe_host_encrypt_rows", "dctfhe_host_encrypt_seeded", "dctfhe_host_decrypt_rows", "dctfhe_host_decrypt_packed", "dctfhe_host_decrypt_ring",
    "dctfhe_host_eval_keys_export_compressed", "dctfhe_host_eval_keys_export_compressed_tiers", "dctfhe_host_pack_key_export", "dctfhe_host_public_key_export",
    "dctfhe_host_public_key_import", "dctfhe_host_public_key_destroy", "dctfhe_host_public_key_info", "dctfhe_host_public_key_set_encrypt_seed",
    "dctfhe_host_public_key_draws", "dctfhe_host_encrypt_public",
]

_lib = None


class DctfheHostError(RuntimeError):
    pass


def load():
    """Load libdctfhe_client.so; raises if it has not been built"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DctfheHostError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (host compiler, -fopenmp)")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32, sz = C.c_void_p, C.c_uint64, C.c_int, C.c_size_t
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.dctfhe_host_last_error.restype = C.c_char_p
    L.dctfhe_host_client_key_create.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.dctfhe_host_client_key_destroy.argtypes = [vp]
    L.dctfhe_host_client_key_export_secret.argtypes = [vp, vp, vp]
    L.dctfhe_host_client_key_set_encrypt_counter.argtypes = [vp, u64]
    L.dctfhe_host_client_key_set_encrypt_nonce.argtypes = [vp, C.c_char_p]
    L.dctfhe_host_client_key_public_keys.argtypes = [vp, vp, vp]
    L.dctfhe_host_encrypt_rows.argtypes = [vp, vp, sz, i32, vp]
    L.dctfhe_host_encrypt_seeded.argtypes = [vp, vp, sz, vp, C.POINTER(u64), vp]
    L.dctfhe_host_decrypt_rows.argtypes = [vp, vp, sz, i32, vp]
    L.dctfhe_host_decrypt_packed.argtypes = [vp, i32, vp, sz, vp]
    L.dctfhe_host_decrypt_ring.argtypes = [vp, i32, vp, sz, vp]
    L.dctfhe_host_eval_keys_export_compressed.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.dctfhe_host_eval_keys_export_compressed_tiers.argtypes = [vp, C.POINTER(KeyTiers), vp, sz, C.POINTER(sz)]
    L.dctfhe_host_pack_key_export.argtypes = [vp, i32, i32, i32, C.c_double, vp, sz, C.POINTER(sz)]
    L.dctfhe_host_public_key_export.argtypes = [vp, i32, C.c_double, vp, sz, C.POINTER(sz)]
    L.dctfhe_host_public_key_import.argtypes = [vp, sz, C.POINTER(vp)]
    L.dctfhe_host_public_key_destroy.argtypes = [vp]
    L.dctfhe_host_public_key_info.argtypes = [vp, pi, pd]
    L.dctfhe_host_public_key_set_encrypt_seed.argtypes = [vp, C.c_char_p]
    L.dctfhe_host_public_key_draws.argtypes = [vp, u64, sz, vp, vp, vp]
    L.dctfhe_host_encrypt_public.argtypes = [vp, vp, sz, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise DctfheHostError(load().dctfhe_host_last_error().decode())


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
