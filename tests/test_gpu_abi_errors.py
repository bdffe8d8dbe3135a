"""One negative case per C-ABI entry point on the device: bad arguments come back as an error code and
a message, nothing crashes, and the handle is usable afterwards (the early returns release what they had allocated)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kit(gpu_ctx):
    from dctfhe import compile as cc, models, params as P
    from dctfhe.engine import Circuit, Keys
    ps = P.test_params()
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=2)
    calib = np.random.default_rng(0).normal(0, 1, (16, 4, 6, 6))
    compiled = cc.compile_model(models.tiny_resnet_q(), calib, param_set=ps)
    circ = Circuit(gpu_ctx, compiled.blob)
    yield gpu_ctx, keys, circ, compiled, ps
    circ.close()
    keys.close()


def _fails(L, rc, needle):
    assert rc != 0
    msg = L.dctfhe_last_error().decode()
    assert needle in msg, msg


def test_context_and_keygen_errors(kit):
    ctx, keys, circ, compiled, ps = kit
    L = ctx.L
    h = C.c_void_p()
    _fails(L, L.dctfhe_ctx_create(99, C.byref(h)), "out of range")
    from dctfhe import params as P
    bad = P.to_c_params(ps)
    bad.tiers[0].l = 7
    c, e = C.c_void_p(), C.c_void_p()
    _fails(L, L.dctfhe_keygen(ctx.h, C.byref(bad), bytes(32), C.byref(c), C.byref(e)), "bad bootstrap gadget")
    _fails(L, L.dctfhe_client_key_create(ctx.h, C.byref(bad), bytes(32), C.byref(c)), "bad bootstrap gadget")
    _fails(L, L.dctfhe_client_key_create(ctx.h, C.byref(P.to_c_params(ps)), None, C.byref(c)), "null")
    _fails(L, L.dctfhe_eval_keys_generate(None, C.byref(e)), "null")
    n = C.c_size_t()
    small = np.zeros(64, np.uint8)
    _fails(L, L.dctfhe_eval_keys_export(keys.eval.h, small.ctypes.data_as(C.c_void_p), small.size, C.byref(n)), "needed")
    _fails(L, L.dctfhe_eval_keys_import(ctx.h, small.ctypes.data_as(C.c_void_p), small.size, C.byref(e)), "too short")
    _fails(L, L.dctfhe_client_key_set_encrypt_counter(keys.client.h, 1 << 60), "out of range")


def test_primitive_errors(kit):
    ctx, keys, circ, compiled, ps = kit
    L = ctx.L
    D = keys.D
    cts = keys.encrypt(np.arange(3, dtype=np.uint64) << np.uint64(58))
    out_small = np.zeros((3, 64), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _fails(L, L.dctfhe_keyswitch(ctx.h, keys.eval.h, 5, p(cts), 3, 0, p(out_small)), "tier out of range")
    _fails(L, L.dctfhe_keyswitch_prefix(ctx.h, keys.eval.h, 0, p(cts), 3, 0, D + 4, p(out_small)), "deff out of range")
    _fails(L, L.dctfhe_keyswitch(ctx.h, keys.eval.h, 0, p(cts), 3, 64, p(out_small)), "shift out of range")
    tab = np.zeros(1 << 12, np.int64)
    small = np.zeros((3, ps.tiers[0].n + 1), np.uint64)
    big = np.zeros((3, D + 1), np.uint64)
    _fails(L, L.dctfhe_pbs(ctx.h, keys.eval.h, 0, p(small), 3, p(tab), 1, 12, None, p(big)), "does not fit")
    _fails(L, L.dctfhe_pbs(ctx.h, keys.eval.h, -1, p(small), 3, p(tab), 1, 4, None, p(big)), "tier out of range")
    idx = np.array([0, 3, 0], np.int32)
    _fails(L, L.dctfhe_pbs(ctx.h, keys.eval.h, 0, p(small), 3, p(tab), 2, 4, p(idx), p(big)), "table_idx[1]")
    _fails(L, L.dctfhe_round_lut(ctx.h, keys.eval.h, 1, 0, p(cts), 3, 8, 2, p(tab), 1, 5, None, p(big)), "w must equal p - r")
    _fails(L, L.dctfhe_round_lut(ctx.h, keys.eval.h, 9, 0, p(cts), 3, 8, 2, p(tab), 1, 6, None, p(big)), "tier out of range")
    _fails(L, L.dctfhe_round_lut(ctx.h, keys.eval.h, 1, 0, p(cts), 3, 70, 2, p(tab), 1, 68, None, p(big)), "p <= 62")
    w = np.zeros((2, 2, 3, 3), np.int8)
    x = np.zeros((1, 2, 2, 2, 5), np.uint64)
    _fails(L, L.dctfhe_conv2d(ctx.h, 4, p(x), 1, 2, 2, 2, p(w), 2, 3, 3, 1, 0, p(x)), "kernel larger")
    _fails(L, L.dctfhe_conv2d(ctx.h, 4, p(x), 1, 2, 2, 2, p(w), 2, 3, 3, 0, 1, p(x)), "bad geometry")
    # the seams of a look-up site: dctfhe_pbs_rows refuses each of its bad arguments by message, the other three one each
    rows_io = np.zeros((4, D + 1), np.uint64)
    pbs_rows = lambda count=3, ntab=2, w=4, ix=None, hw=1, nchan=1, n_rows=4, row0=1, dim_out=D, tier=0: L.dctfhe_pbs_rows(
        ctx.h, keys.eval.h, tier, p(small), count, p(tab), ntab, w, ix, hw, nchan, 0, p(rows_io), n_rows, row0, dim_out, 1, 5)
    _fails(L, pbs_rows(row0=2), "outside the 4 rows")
    _fails(L, pbs_rows(hw=0), "hw = 0")
    _fails(L, pbs_rows(nchan=0), "per-channel tables")
    _fails(L, pbs_rows(nchan=3), "per-channel tables")
    _fails(L, pbs_rows(ix=p(idx)), "table_idx[1]")
    _fails(L, pbs_rows(ntab=1, w=12), "does not fit")
    ring = ps.tiers[0].k << ps.tiers[0].logN
    _fails(L, pbs_rows(dim_out=ring - 1), "cannot hold a ring")
    _fails(L, pbs_rows(tier=7), "tier out of range")
    assert not rows_io.any()
    _fails(L, L.dctfhe_keyswitch_sum(ctx.h, keys.eval.h, 0, p(cts), D, p(cts), D, 3, 0, 0, D + 1, p(out_small)), "deff out of range")
    _fails(L, L.dctfhe_keyswitch_sum(ctx.h, keys.eval.h, 0, p(cts), D + 1, p(cts), D, 3, 0, 0, 0, p(out_small)), "the key has")
    _fails(L, L.dctfhe_acc_rows(ctx.h, p(big), D, p(cts), D, 3, D + 1), "do not fit")
    gmap = np.array([0, 3, 1], np.int32)
    _fails(L, L.dctfhe_gather_rows(ctx.h, p(cts), D, D, 3, p(gmap), 3, D, p(big)), "map[1] = 3 out of range")
    # the handles still work after all that
    assert np.array_equal((keys.decrypt(cts) + np.uint64(1 << 56)) >> np.uint64(57), (np.arange(3, dtype=np.uint64) << np.uint64(1)))


def test_circuit_and_session_errors(kit):
    ctx, keys, circ, compiled, ps = kit
    L = ctx.L
    h = C.c_void_p()
    blob = bytearray(compiled.blob)
    _fails(L, L.dctfhe_circuit_load(ctx.h, bytes(blob[:40]), 40, C.byref(h)), "truncated")
    blob[0] ^= 1
    _fails(L, L.dctfhe_circuit_load(ctx.h, bytes(blob), len(blob), C.byref(h)), "magic")
    _fails(L, L.dctfhe_session_create(ctx.h, circ.h, keys.eval.h, 0, C.byref(h)), "batch must be")
    # a circuit that names a tier these keys lack
    from dctfhe import params as P
    from dctfhe.engine import Keys, Session
    one_tier = P.to_c_params(ps)
    one_tier.n_tiers = 1
    one_tier.n_max = one_tier.tiers[0].n
    k1 = Keys(ctx, one_tier, seed=3)
    try:
        _fails(L, L.dctfhe_session_create(ctx.h, circ.h, k1.eval.h, 1, C.byref(h)), "names a tier the keys lack")
    finally:
        k1.close()
    # the effective-dimension guard at upload: ciphertexts with a non-zero tail when the circuit was compiled for a key prefix
    sess = Session(ctx, circ, keys, 1)
    try:
        assert L.dctfhe_session_set_noise(sess.h, 1, None, 0) != 0 and "clear-mode" in L.dctfhe_last_error().decode()
    finally:
        sess.close()
    clear = Session(ctx, circ, None, 1)
    try:
        sg = np.zeros(3, np.float64)
        _fails(L, L.dctfhe_session_set_noise(clear.h, 1, sg.ctypes.data_as(C.c_void_p), 3), "one sigma per op")
    finally:
        clear.close()


def test_handles_of_another_context_are_refused(kit):
    """keys and sessions belong to the context they were made on (include/dctfhe.h): a call that names another context is refused before
    it allocates, copies or launches anything.  tests/test_gpu_contexts_streams.py has the case per entry point; here the ABI's answer."""
    from dctfhe.engine import Context, Session, device_bytes_live
    ctx, keys, circ, compiled, ps = kit
    L = ctx.L
    D = keys.D
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cts = keys.encrypt(np.arange(3, dtype=np.uint64) << np.uint64(58))
    small = np.zeros((3, ps.tiers[0].n + 1), np.uint64)
    big = np.zeros((3, D + 1), np.uint64)
    ph = np.zeros(3, np.uint64)
    tab = np.zeros(16, np.int64)
    h = C.c_void_p()
    other = Context(0)
    sess = Session(ctx, circ, keys, 1)
    try:
        held = device_bytes_live()
        _fails(L, L.dctfhe_encrypt(other.h, keys.client.h, p(ph), 3, p(big)), "context")
        _fails(L, L.dctfhe_decrypt(other.h, keys.client.h, p(cts), 3, p(ph)), "context")
        _fails(L, L.dctfhe_keyswitch(other.h, keys.eval.h, 0, p(cts), 3, 0, p(small)), "context")
        _fails(L, L.dctfhe_modswitch_center(other.h, keys.eval.h, 0, p(small), 3), "context")
        _fails(L, L.dctfhe_pbs(other.h, keys.eval.h, 0, p(small), 3, p(tab), 1, 4, None, p(big)), "context")
        _fails(L, L.dctfhe_round_lut(other.h, keys.eval.h, 1, 0, p(cts), 3, 8, 4, p(tab), 1, 4, None, p(big)), "context")
        _fails(L, L.dctfhe_keyswitch_pack(other.h, keys.eval.h, 0, p(cts), 3, D, 0, p(small)), "context")
        _fails(L, L.dctfhe_margin_probe(other.h, keys.client.h, 0, p(small), 3, 4, None, None), "context")
        _fails(L, L.dctfhe_session_create(other.h, circ.h, keys.eval.h, 1, C.byref(h)), "context")
        assert h.value is None and not big.any() and not small.any() and not ph.any()
        assert device_bytes_live() == held
        # a client key of another context at the margin audit; the session's own is accepted
        from dctfhe import params as P
        from dctfhe.engine import ClientKey
        k2 = ClientKey(other, P.to_c_params(ps), seed=2)
        try:
            _fails(L, L.dctfhe_session_set_audit(sess.h, k2.h), "context")
            sess.set_audit(keys)
            sess.set_audit(None)
        finally:
            k2.close()
        # a circuit is bound to its device, not to a context: a clear-mode session of the other context takes it
        clear = Session(other, circ, None, 1)
        clear.close()
        assert device_bytes_live() == held
        # the handles still work after all that
        assert np.array_equal((keys.decrypt(cts) + np.uint64(1 << 56)) >> np.uint64(57), (np.arange(3, dtype=np.uint64) << np.uint64(1)))
    finally:
        sess.close()
        other.close()

