"""ctypes binding of libdctfhe.so (include/dctfhe.h).

The library is built in-tree by __graft_entry__.build() (hipcc --offload-arch=gfx950) and lives at
dct-cryptonets_amd/libdctfhe.so.  There is no fallback: if the library is missing, or no HIP
device is visible, every operation raises.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libdctfhe.so")
MAX_TIERS = 12


class Tier(C.Structure):
    _fields_ = [("n", C.c_int32), ("k", C.c_int32), ("logN", C.c_int32), ("l", C.c_int32), ("beta", C.c_int32),
                ("lk", C.c_int32), ("betak", C.c_int32), ("ksk_share", C.c_int32),
                ("unroll", C.c_int32), ("reserved", C.c_int32),
                ("lwe_sigma", C.c_double), ("glwe_sigma", C.c_double)]


class Params(C.Structure):
    _fields_ = [("D", C.c_int32), ("n_max", C.c_int32), ("n_tiers", C.c_int32), ("input_dim", C.c_int32),
                ("input_sigma", C.c_double), ("tiers", Tier * MAX_TIERS)]


class Stats(C.Structure):
    _fields_ = [("pbs_count", C.c_int64 * MAX_TIERS), ("ks_count", C.c_int64 * MAX_TIERS), ("conv_macs", C.c_int64),
                ("lut_sites", C.c_int64), ("bit_steps", C.c_int64), ("bytes_algorithmic", C.c_double),
                ("key_bytes_per_pass", C.c_double), ("flops_f64", C.c_double), ("max_bit_width", C.c_int32),
                ("n_ops", C.c_int32)]


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("pbs_ms", C.c_double * MAX_TIERS), ("ks_ms", C.c_double),
                ("linear_ms", C.c_double), ("pbs_launches", C.c_int64 * MAX_TIERS), ("pbs_cts", C.c_int64 * MAX_TIERS)]


MARGIN_BINS = 16


class MarginStats(C.Structure):
    """dctfhe_margin_stats: one slot of the margin audit (include/dctfhe.h)"""
    _fields_ = [("op", C.c_int32), ("entry", C.c_int32), ("tier", C.c_int32), ("table_bits", C.c_int32), ("half_box", C.c_int32),
                ("max_abs", C.c_int32), ("count", C.c_int64), ("sum", C.c_int64), ("sum_sq", C.c_uint64), ("hist", C.c_int64 * MARGIN_BINS)]


class KeyTiers(C.Structure):
    """dctfhe_key_tiers: which tiers' bootstrap keys (bsk) and own key-switch keys (ksk) a set of evaluation keys holds (include/dctfhe.h)"""
    _fields_ = [("bsk", C.c_uint32), ("ksk", C.c_uint32)]

    def __eq__(self, other):
        return isinstance(other, KeyTiers) and (self.bsk, self.ksk) == (other.bsk, other.ksk)

    def __hash__(self):
        return hash((int(self.bsk), int(self.ksk)))

    def __repr__(self):
        return "KeyTiers(bsk=0x%x, ksk=0x%x)" % (self.bsk, self.ksk)


MAX_SLAB_GROUPS = 64


class MemPlan(C.Structure):
    """dctfhe_mem_plan: planned session bytes and the slab height per slab group (include/dctfhe.h)"""
    _fields_ = [("bytes_undivided", C.c_uint64), ("bytes_planned", C.c_uint64), ("budget_bytes", C.c_uint64),
                ("bytes_buffers", C.c_uint64), ("bytes_maps", C.c_uint64), ("bytes_scratch", C.c_uint64),
                ("n_groups", C.c_int32), ("reserved", C.c_int32),
                ("first_op", C.c_int32 * MAX_SLAB_GROUPS), ("end_op", C.c_int32 * MAX_SLAB_GROUPS),
                ("channels", C.c_int32 * MAX_SLAB_GROUPS), ("slab", C.c_int32 * MAX_SLAB_GROUPS)]

    def record(self):
        return dict(bytes_undivided=int(self.bytes_undivided), bytes_planned=int(self.bytes_planned), budget_bytes=int(self.budget_bytes),
                    bytes_buffers=int(self.bytes_buffers), bytes_maps=int(self.bytes_maps), bytes_scratch=int(self.bytes_scratch),
                    groups=[dict(first_op=int(self.first_op[g]), end_op=int(self.end_op[g]), channels=int(self.channels[g]), slab=int(self.slab[g]))
                            for g in range(self.n_groups)])


EXPORTS = [
    "dctfhe_last_error", "dctfhe_version", "dctfhe_ctx_create", "dctfhe_ctx_destroy", "dctfhe_ctx_set_stream",
    "dctfhe_ctx_synchronize", "dctfhe_keygen", "dctfhe_client_key_create", "dctfhe_client_key_destroy", "dctfhe_eval_keys_generate",
    "dctfhe_eval_keys_destroy", "dctfhe_eval_keys_export", "dctfhe_eval_keys_import", "dctfhe_client_key_export_secret",
    "dctfhe_eval_keys_export_ksk", "dctfhe_client_key_export_bsk", "dctfhe_rng_host", "dctfhe_rng_device", "dctfhe_client_key_set_encrypt_counter", "dctfhe_client_key_set_encrypt_nonce", "dctfhe_encrypt", "dctfhe_decrypt", "dctfhe_encrypt_rows", "dctfhe_decrypt_rows", "dctfhe_keyswitch", "dctfhe_keyswitch_prefix", "dctfhe_session_set_noise",
    "dctfhe_pbs", "dctfhe_modswitch_center", "dctfhe_round_lut", "dctfhe_conv2d", "dctfhe_conv2d_rows", "dctfhe_add_rows", "dctfhe_affine_rows", "dctfhe_sum_pool_rows", "dctfhe_circuit_load", "dctfhe_circuit_destroy", "dctfhe_params_check", "dctfhe_circuit_validate", "dctfhe_dct_frontend",
    "dctfhe_circuit_stats", "dctfhe_circuit_io", "dctfhe_session_create", "dctfhe_session_destroy",
    "dctfhe_session_upload", "dctfhe_session_run", "dctfhe_session_download", "dctfhe_session_upload_rows", "dctfhe_session_download_rows", "dctfhe_session_dims", "dctfhe_fp64_peak", "dctfhe_bench_pbs",
    "dctfhe_encrypt_seeded", "dctfhe_expand_seeded", "dctfhe_session_upload_seeded", "dctfhe_eval_keys_export_compressed",
    "dctfhe_eval_keys_decompress_bsk", "dctfhe_keyswitch_diff", "dctfhe_max_pool_rows",
    "dctfhe_round_lut_split", "dctfhe_session_set_noise_split",
    "dctfhe_session_download_packed", "dctfhe_keyswitch_pack", "dctfhe_decrypt_packed",
    "dctfhe_margin_probe_host", "dctfhe_margin_probe", "dctfhe_session_set_audit", "dctfhe_session_audit",
    "dctfhe_device_bytes_live",
    "dctfhe_pack_key_export", "dctfhe_pack_key_import", "dctfhe_pack_key_destroy", "dctfhe_pack_key_info", "dctfhe_pack_key_export_rows",
    "dctfhe_ring_words", "dctfhe_ring_pack", "dctfhe_session_download_ring", "dctfhe_decrypt_ring",
    "dctfhe_public_key_export", "dctfhe_public_key_import", "dctfhe_public_key_destroy", "dctfhe_public_key_info", "dctfhe_public_key_export_rows",
    "dctfhe_public_key_set_encrypt_seed", "dctfhe_public_key_draws", "dctfhe_public_words", "dctfhe_encrypt_public", "dctfhe_ring_extract",
    "dctfhe_session_upload_public",
    "dctfhe_shard_rows", "dctfhe_session_set_shard", "dctfhe_session_run_span", "dctfhe_session_shard_plan", "dctfhe_session_tensor",
    "dctfhe_session_mark_whole", "dctfhe_session_copy_rows",
    "dctfhe_shard_pool", "dctfhe_session_set_shard_pool", "dctfhe_session_mark_rows", "dctfhe_session_shard_plan_rows", "dctfhe_session_pool_pairs",
    "dctfhe_conv2d_rows_window", "dctfhe_memory_plan", "dctfhe_session_set_memory_budget", "dctfhe_session_memory_plan", "dctfhe_session_set_slab_heights",
    "dctfhe_pbs_rows", "dctfhe_keyswitch_sum", "dctfhe_acc_rows", "dctfhe_gather_rows",
    "dctfhe_key_tiers_all", "dctfhe_key_tiers_close", "dctfhe_key_tiers_for_circuit", "dctfhe_key_tiers_blob_bytes",
    "dctfhe_eval_keys_generate_tiers", "dctfhe_eval_keys_export_compressed_tiers", "dctfhe_eval_keys_tiers",
]

_lib = None


class DctfheError(RuntimeError):
    pass


def load():
    """Load libdctfhe.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DctfheError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); this engine has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32, sz = C.c_void_p, C.c_uint64, C.c_int, C.c_size_t
    L.dctfhe_last_error.restype = C.c_char_p
    L.dctfhe_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.dctfhe_ctx_destroy.argtypes = [vp]
    L.dctfhe_ctx_set_stream.argtypes = [vp, vp]
    L.dctfhe_ctx_synchronize.argtypes = [vp]
    L.dctfhe_keygen.argtypes = [vp, C.POINTER(Params), C.c_char_p, C.POINTER(vp), C.POINTER(vp)]
    L.dctfhe_client_key_create.argtypes = [vp, C.POINTER(Params), C.c_char_p, C.POINTER(vp)]
    L.dctfhe_client_key_destroy.argtypes = [vp]
    L.dctfhe_eval_keys_generate.argtypes = [vp, C.POINTER(vp)]
    L.dctfhe_eval_keys_destroy.argtypes = [vp]
    L.dctfhe_eval_keys_export.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.dctfhe_eval_keys_import.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.dctfhe_client_key_export_secret.argtypes = [vp, vp, vp]
    L.dctfhe_eval_keys_export_ksk.argtypes = [vp, i32, vp]
    L.dctfhe_client_key_export_bsk.argtypes = [vp, i32, vp]
    L.dctfhe_rng_host.argtypes = [C.c_char_p, u64, u64, sz, vp]
    L.dctfhe_rng_device.argtypes = [vp, C.c_char_p, u64, u64, sz, vp]
    L.dctfhe_client_key_set_encrypt_counter.argtypes = [vp, u64]
    L.dctfhe_client_key_set_encrypt_nonce.argtypes = [vp, C.c_char_p]
    L.dctfhe_encrypt.argtypes = [vp, vp, vp, sz, vp]
    L.dctfhe_decrypt.argtypes = [vp, vp, vp, sz, vp]
    L.dctfhe_encrypt_rows.argtypes = [vp, vp, vp, sz, i32, vp]
    L.dctfhe_decrypt_rows.argtypes = [vp, vp, vp, sz, i32, vp]
    L.dctfhe_keyswitch.argtypes = [vp, vp, i32, vp, sz, i32, vp]
    L.dctfhe_session_set_noise.argtypes = [vp, C.c_uint64, vp, i32]
    L.dctfhe_keyswitch_prefix.argtypes = [vp, vp, i32, vp, sz, i32, i32, vp]
    L.dctfhe_modswitch_center.argtypes = [vp, vp, i32, vp, sz]
    L.dctfhe_pbs.argtypes = [vp, vp, i32, vp, sz, vp, i32, i32, vp, vp]
    L.dctfhe_round_lut.argtypes = [vp, vp, i32, i32, vp, sz, i32, i32, vp, i32, i32, vp, vp]
    L.dctfhe_round_lut_split.argtypes = [vp, vp, i32, i32, i32, vp, sz, i32, i32, vp, i32, i32, vp, vp]
    L.dctfhe_session_set_noise_split.argtypes = [vp, vp, i32]
    L.dctfhe_conv2d.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp]
    L.dctfhe_conv2d_rows.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, vp]
    L.dctfhe_conv2d_rows_window.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.dctfhe_add_rows.argtypes = [vp, vp, i32, i32, vp, i32, i32, sz, i32, vp]
    L.dctfhe_affine_rows.argtypes = [vp, vp, i32, i32, sz, i32, i32, u64, i32, vp]
    L.dctfhe_sum_pool_rows.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.dctfhe_dct_frontend.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp]
    L.dctfhe_params_check.argtypes = [C.POINTER(Params)]
    L.dctfhe_circuit_validate.argtypes = [vp, sz]
    L.dctfhe_circuit_load.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.dctfhe_circuit_destroy.argtypes = [vp]
    L.dctfhe_circuit_stats.argtypes = [vp, C.POINTER(Params), C.POINTER(Stats)]
    L.dctfhe_circuit_io.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dctfhe_session_create.argtypes = [vp, vp, vp, i32, C.POINTER(vp)]
    L.dctfhe_session_destroy.argtypes = [vp]
    L.dctfhe_session_upload.argtypes = [vp, vp]
    L.dctfhe_session_run.argtypes = [vp, C.POINTER(Timing)]
    L.dctfhe_session_download.argtypes = [vp, vp]
    L.dctfhe_session_upload_rows.argtypes = [vp, vp, i32]
    L.dctfhe_session_download_rows.argtypes = [vp, vp, i32]
    L.dctfhe_session_dims.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dctfhe_fp64_peak.argtypes = [vp, C.POINTER(C.c_double)]
    L.dctfhe_bench_pbs.argtypes = [vp, vp, i32, sz, i32, C.POINTER(C.c_double)]
    L.dctfhe_encrypt_seeded.argtypes = [vp, vp, vp, sz, vp, C.POINTER(u64), vp]
    L.dctfhe_expand_seeded.argtypes = [vp, C.c_char_p, u64, i32, i32, vp, sz, i32, vp]
    L.dctfhe_session_upload_seeded.argtypes = [vp, C.c_char_p, u64, i32, vp, sz]
    L.dctfhe_eval_keys_export_compressed.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.dctfhe_eval_keys_decompress_bsk.argtypes = [vp, vp, sz, i32, vp]
    L.dctfhe_keyswitch_diff.argtypes = [vp, vp, i32, vp, sz, vp, vp, i32, u64, i32, vp]
    L.dctfhe_pbs_rows.argtypes = [vp, vp, i32, vp, sz, vp, i32, i32, vp, i32, i32, sz, vp, sz, sz, i32, i32, u64]
    L.dctfhe_keyswitch_sum.argtypes = [vp, vp, i32, vp, i32, vp, i32, sz, i32, u64, i32, vp]
    L.dctfhe_acc_rows.argtypes = [vp, vp, i32, vp, i32, sz, i32]
    L.dctfhe_gather_rows.argtypes = [vp, vp, i32, i32, sz, vp, sz, i32, vp]
    L.dctfhe_max_pool_rows.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp]
    L.dctfhe_session_download_packed.argtypes = [vp, i32, vp]
    L.dctfhe_keyswitch_pack.argtypes = [vp, vp, i32, vp, sz, i32, i32, vp]
    L.dctfhe_decrypt_packed.argtypes = [vp, vp, i32, vp, sz, vp]
    L.dctfhe_margin_probe_host.argtypes = [vp, i32, i32, vp, sz, i32, vp, C.POINTER(MarginStats)]
    L.dctfhe_margin_probe.argtypes = [vp, vp, i32, vp, sz, i32, vp, C.POINTER(MarginStats)]
    L.dctfhe_session_set_audit.argtypes = [vp, vp]
    L.dctfhe_session_audit.argtypes = [vp, C.POINTER(MarginStats), i32, C.POINTER(C.c_int)]
    L.dctfhe_device_bytes_live.argtypes = []
    L.dctfhe_device_bytes_live.restype = sz
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.dctfhe_pack_key_export.argtypes = [vp, i32, i32, i32, C.c_double, vp, sz, C.POINTER(sz)]
    L.dctfhe_pack_key_import.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.dctfhe_pack_key_destroy.argtypes = [vp]
    L.dctfhe_pack_key_info.argtypes = [vp, pi, pi, pi, pi, pd]
    L.dctfhe_pack_key_export_rows.argtypes = [vp, vp]
    L.dctfhe_ring_words.argtypes = [i32, sz]
    L.dctfhe_ring_words.restype = sz
    L.dctfhe_ring_pack.argtypes = [vp, vp, vp, sz, i32, vp]
    L.dctfhe_session_download_ring.argtypes = [vp, i32, vp, vp]
    L.dctfhe_decrypt_ring.argtypes = [vp, vp, i32, vp, sz, vp]
    L.dctfhe_public_key_export.argtypes = [vp, i32, C.c_double, vp, sz, C.POINTER(sz)]
    L.dctfhe_public_key_import.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.dctfhe_public_key_destroy.argtypes = [vp]
    L.dctfhe_public_key_info.argtypes = [vp, pi, pd]
    L.dctfhe_public_key_export_rows.argtypes = [vp, vp]
    L.dctfhe_public_key_set_encrypt_seed.argtypes = [vp, C.c_char_p]
    L.dctfhe_public_key_draws.argtypes = [vp, C.c_uint64, sz, vp, vp, vp]
    L.dctfhe_public_words.argtypes = [i32, sz]
    L.dctfhe_public_words.restype = sz
    L.dctfhe_encrypt_public.argtypes = [vp, vp, vp, sz, vp]
    L.dctfhe_ring_extract.argtypes = [vp, i32, vp, sz, i32, vp]
    L.dctfhe_session_upload_public.argtypes = [vp, i32, vp, sz]
    L.dctfhe_shard_rows.argtypes = [sz, i32, i32, C.POINTER(sz), C.POINTER(sz)]
    L.dctfhe_session_set_shard.argtypes = [vp, i32, i32]
    L.dctfhe_session_run_span.argtypes = [vp, i32, i32, C.POINTER(Timing)]
    L.dctfhe_session_shard_plan.argtypes = [vp, vp, vp, i32, pi]
    L.dctfhe_session_tensor.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.dctfhe_session_mark_whole.argtypes = [vp, i32]
    L.dctfhe_session_copy_rows.argtypes = [vp, vp, i32, sz, sz]
    L.dctfhe_shard_pool.argtypes = [i32] * 9 + [C.POINTER(sz)] * 5
    L.dctfhe_session_set_shard_pool.argtypes = [vp, i32]
    L.dctfhe_session_mark_rows.argtypes = [vp, i32, sz, sz]
    L.dctfhe_session_shard_plan_rows.argtypes = [vp, vp, vp, vp, vp, i32, pi]
    L.dctfhe_session_pool_pairs.argtypes = [vp, i32, C.POINTER(sz)]
    L.dctfhe_memory_plan.argtypes = [vp, sz, C.POINTER(Params), i32, sz, C.POINTER(MemPlan)]
    L.dctfhe_session_set_memory_budget.argtypes = [vp, sz]
    L.dctfhe_session_memory_plan.argtypes = [vp, C.POINTER(MemPlan)]
    L.dctfhe_session_set_slab_heights.argtypes = [vp, vp, i32]
    pk = C.POINTER(KeyTiers)
    L.dctfhe_key_tiers_all.argtypes = [C.POINTER(Params), pk]
    L.dctfhe_key_tiers_close.argtypes = [C.POINTER(Params), pk]
    L.dctfhe_key_tiers_for_circuit.argtypes = [vp, sz, C.POINTER(Params), pk]
    L.dctfhe_key_tiers_blob_bytes.argtypes = [C.POINTER(Params), pk, i32, C.POINTER(sz)]
    L.dctfhe_eval_keys_generate_tiers.argtypes = [vp, pk, C.POINTER(vp)]
    L.dctfhe_eval_keys_export_compressed_tiers.argtypes = [vp, pk, vp, sz, C.POINTER(sz)]
    L.dctfhe_eval_keys_tiers.argtypes = [vp, pk]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise DctfheError(load().dctfhe_last_error().decode())


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
