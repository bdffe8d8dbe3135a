"""Which context and which stream the work runs on (include/dctfhe.h, "WHAT A HANDLE IS BOUND TO" and dctfhe_ctx_set_stream).

Everything runs on device 0 in one process; the second and third context are this module's own.  A handle of another context is refused
by every entry point that takes a context and a key handle; a circuit is shared by the contexts of its device; a sharded loopback crosses
two contexts; every primitive gives the same words on a caller's (non-blocking) stream as on the context's own; the library's work is
ordered after what the caller had enqueued on that stream; dctfhe_ctx_synchronize waits for the stream that is set; two host threads with a
context each run side by side.  All comparisons are word for word: nothing on the server side is random, and the client side is pinned by
a fixed nonce and counter (tests/test_gpu_pbs_matrix.py step (c): a bootstrap's words do not depend on the launch)."""
import ctypes as C
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch      # before anything loads libdctfhe.so: the process then has one HIP runtime, torch's (tensor_view shares device memory with it)

from test_gpu_primitives import D_SMALL, TIERS_SMALL
from test_gpu_shard import drive

pytestmark = pytest.mark.gpu

U = np.uint64
N_CT = 37
NONCE = bytes(range(16))
# The delay of the ordering tests: a chain of DELAY_N x DELAY_N float32 matmuls on the side stream.  Measured on an MI355X
# (profiles/streams_contexts.json): DELAY_CHAIN_MIN products are the shortest chain at which the control still reads the stale input in
# clear and in encrypted mode; four times that is shipped, because queueing time varies from run to run.
DELAY_N = 4096
DELAY_CHAIN_MIN = 2
DELAY_CHAIN = 4 * DELAY_CHAIN_MIN


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def live():
    from dctfhe.engine import device_bytes_live
    return device_bytes_live()


@pytest.fixture(scope="module")
def ctxs():
    """contexts A and B on device 0: the second and third of this process next to the suite's gpu_ctx"""
    from dctfhe.engine import Context
    a, b = Context(0), Context(0)
    yield a, b
    b.close()
    a.close()


@pytest.fixture(scope="module")
def prim(ctxs):
    """the D = 1024 tiers of tests/test_gpu_primitives.py on context A, with a packing key and a public key, and one set of operands"""
    from dctfhe import params as P
    from dctfhe.engine import Keys, PackKey, PublicKey, make_params
    a, _ = ctxs
    keys = Keys(a, make_params(D_SMALL, 40, TIERS_SMALL, 2.0 ** -50), seed=7)
    keys.set_encrypt_nonce(NONCE)
    pack = PackKey(a, keys.export_pack_key(P.PackSpec(logN=8, l=1, beta=16, sigma=2.0 ** -48)))
    pub = PublicKey(a, keys.export_public_key(P.PublicInputSpec(logN=8, sigma=2.0 ** -48)))
    rng = np.random.default_rng(2026)
    D, n = D_SMALL, TIERS_SMALL[0]["n"]
    e = SimpleNamespace(ctx=a, keys=keys, pack=pack, pub=pub, D=D, n=n)
    e.phases = rng.integers(0, 16, N_CT).astype(U) << U(59)
    keys.set_encrypt_counter(5)
    e.cts = keys.encrypt(e.phases)
    e.rows = rng.integers(0, 2 ** 64, (N_CT, D + 1), dtype=U)
    e.rows_b = rng.integers(0, 2 ** 64, (N_CT, 257), dtype=U)
    e.small = rng.integers(0, 2 ** 64, (N_CT, n + 1), dtype=U)
    e.small_bit = rng.integers(0, 2 ** 64, (N_CT, TIERS_SMALL[1]["n"] + 1), dtype=U)
    e.tab4 = rng.integers(0, 16, (2, 16)).astype(np.int64) << 58
    e.tab7 = (2 * rng.integers(0, 8, (2, 128))).astype(np.int64) << 57      # every pair sum even: a parity split takes it
    e.idx = (np.arange(N_CT) % 2).astype(np.int32)
    e.ia = rng.integers(0, N_CT, N_CT).astype(np.int32)
    e.ib = rng.integers(0, N_CT, N_CT).astype(np.int32)
    e.rows_io = rng.integers(0, 2 ** 64, (N_CT + 3, 513), dtype=U)           # rows of the table tier's ring, k N = 512
    e.packed = rng.integers(0, 2 ** 16, (N_CT, n + 1)).astype(np.uint16)
    e.ring = rng.integers(0, 2 ** 16, int(a.L.dctfhe_ring_words(8, N_CT))).astype(np.uint16)
    e.pool_in = rng.integers(0, 2 ** 64, (1, 2, 4, 4, D + 1), dtype=U)
    e.pool_tab = (np.maximum(np.arange(16) - 8, 0).astype(U) << U(59)).view(np.int64)
    e.conv_in = rng.integers(0, 2 ** 64, (2, 3, 5, 5, 97), dtype=U)
    e.conv_w = rng.integers(-7, 8, (5, 3, 3, 3)).astype(np.int8)
    e.gmap = rng.integers(0, N_CT, 50).astype(np.int32)
    yield e
    pub.close()
    pack.close()
    keys.close()


@pytest.fixture(scope="module")
def trunk(ctxs):
    yield from make_trunk(*ctxs)


def make_trunk(a, b):
    """the tiny trunk, batch 2: ONE circuit handle (loaded on A), the test catalogue's keys from one seed on A and on B, one seeded
    input, and the all-on-A outputs and stored input rows of the real and of the all-zero input, clear and encrypted (computed once)"""
    from dctfhe import models, params as P
    from dctfhe.engine import Circuit, Keys, Session
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from dctfhe.sharding import tensor_view
    calib = np.random.default_rng(0).normal(0, 1, (16, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params())
    t = SimpleNamespace(qm=qm, batch=2, plan=qm.compiled.shard_plan(), n_ops=len(qm.compiled.ops), t_in=qm.compiled.input_tensor)
    t.phases = qm.encode_input(qm.quantize_input(calib[:2]))
    t.circuit = Circuit(a, qm.compiled.blob)
    t.cparams = P.to_c_params(P.test_params())
    t.keys_a, t.keys_b = Keys(a, t.cparams, seed=3), Keys(b, t.cparams, seed=3)
    t.keys_a.set_encrypt_nonce(NONCE)
    t.seeded = t.keys_a.encrypt_seeded(t.phases.reshape(-1))
    t.dev = torch.device("cuda:0")
    t.out, t.zero_out, t.real_rows, t.zero_host = {}, {}, {}, {}
    for mode in ("clear", "encrypted"):
        keys = t.keys_a if mode == "encrypted" else None
        s = Session(a, t.circuit, keys, t.batch)
        if keys is None:
            s.upload(t.phases)
        else:
            s.upload_seeded(t.seeded)
            t.in_dim, t.out_dim = s.dims()
        t.real_rows[mode] = tensor_view(s, t.t_in, t.dev).clone()
        torch.cuda.synchronize()
        s.run()
        t.out[mode] = download(t, s)
        t.zero_host[mode] = np.zeros((t.phases.size, t.in_dim + 1) if keys is not None else t.phases.shape, U)
        upload_zero(t, s, mode)
        s.run()
        t.zero_out[mode] = download(t, s)
        s.close()
        assert (t.out[mode] != t.zero_out[mode]).any()      # the two inputs can be told apart by their outputs
        for v in (t.out[mode], t.zero_out[mode]):
            v.setflags(write=False)
    # the delay of the ordering tests, warmed up so that no library start-up is part of it
    t.mm = torch.full((DELAY_N, DELAY_N), 1.0 / DELAY_N, device=t.dev)
    t.mm_out = torch.empty_like(t.mm)
    torch.matmul(t.mm, t.mm, out=t.mm_out)
    torch.cuda.synchronize()
    yield t
    del t.real_rows, t.mm, t.mm_out
    t.keys_b.close()
    t.keys_a.close()
    t.circuit.close()
    qm.close()


def download(t, s):
    return s.download(t.out_dim) if s.keys is not None else s.download()


def upload_zero(t, s, mode):
    if mode == "encrypted":
        s.upload(t.zero_host[mode], t.in_dim)
    else:
        s.upload(t.zero_host[mode])


# ------------------------------------------------------------------------------------------ 1. foreign handles are refused
def _fresh(shape, dtype=U):
    """an output buffer pre-filled with a pattern: a refused call must leave it as it is"""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xA5
    return a


def _bytes_of(obj):
    """a ctypes object's memory as a numpy view"""
    return np.frombuffer(obj, np.uint8)


def _primitive_cases():
    """name -> f(L, e, ctx_handle) -> (call, output buffers).  The handles are e's (context A); the call goes to ctx_handle."""
    D = D_SMALL

    def encrypt_rows(L, e, c):
        out = _fresh((N_CT, D + 1))
        return (lambda: L.dctfhe_encrypt_rows(c, e.keys.client.h, p(e.phases), N_CT, D, p(out))), [out]

    def decrypt_rows(L, e, c):
        out = _fresh(N_CT)
        return (lambda: L.dctfhe_decrypt_rows(c, e.keys.client.h, p(e.cts), N_CT, D, p(out))), [out]

    def encrypt_seeded(L, e, c):
        key, stream, bodies = C.create_string_buffer(b"\xa5" * 32, 32), C.c_uint64(0xA5A5), _fresh(N_CT)
        return (lambda: L.dctfhe_encrypt_seeded(c, e.keys.client.h, p(e.phases), N_CT, key, C.byref(stream), p(bodies))), [_bytes_of(key), _bytes_of(stream), bodies]

    def decrypt_packed(L, e, c):
        out = _fresh(N_CT)
        return (lambda: L.dctfhe_decrypt_packed(c, e.keys.client.h, e.n, p(e.packed), N_CT, p(out))), [out]

    def decrypt_ring(L, e, c):
        out = _fresh(N_CT)
        return (lambda: L.dctfhe_decrypt_ring(c, e.keys.client.h, 8, p(e.ring), N_CT, p(out))), [out]

    def margin_probe(L, e, c):
        from dctfhe._lib import MarginStats
        err, st = _fresh(N_CT, np.int32), MarginStats()
        _bytes_of(st)[...] = 0xA5
        return (lambda: L.dctfhe_margin_probe(c, e.keys.client.h, 0, p(e.small), N_CT, 4, p(err), C.byref(st))), [err, _bytes_of(st)]

    def keyswitch(L, e, c):
        out = _fresh((N_CT, e.n + 1))
        return (lambda: L.dctfhe_keyswitch(c, e.keys.eval.h, 0, p(e.cts), N_CT, 2, p(out))), [out]

    def keyswitch_prefix(L, e, c):
        out = _fresh((N_CT, e.n + 1))
        return (lambda: L.dctfhe_keyswitch_prefix(c, e.keys.eval.h, 0, p(e.cts), N_CT, 2, 0, p(out))), [out]

    def keyswitch_diff(L, e, c):
        out = _fresh((N_CT, e.n + 1))
        return (lambda: L.dctfhe_keyswitch_diff(c, e.keys.eval.h, 0, p(e.rows), N_CT, p(e.ia), p(e.ib), 1, 1 << 62, 0, p(out))), [out]

    def keyswitch_sum(L, e, c):
        out = _fresh((N_CT, e.n + 1))
        return (lambda: L.dctfhe_keyswitch_sum(c, e.keys.eval.h, 0, p(e.rows), D, p(e.rows_b), 256, N_CT, 1, 5, 0, p(out))), [out]

    def keyswitch_pack(L, e, c):
        out = _fresh((N_CT, e.n + 1), np.uint16)
        return (lambda: L.dctfhe_keyswitch_pack(c, e.keys.eval.h, 0, p(e.rows), N_CT, D, 0, p(out))), [out]

    def modswitch_center(L, e, c):
        io = e.small.copy()
        return (lambda: L.dctfhe_modswitch_center(c, e.keys.eval.h, 0, p(io), N_CT)), [io]

    def pbs(L, e, c):
        out = _fresh((N_CT, D + 1))
        return (lambda: L.dctfhe_pbs(c, e.keys.eval.h, 0, p(e.small), N_CT, p(e.tab4), 2, 4, p(e.idx), p(out))), [out]

    def pbs_rows(L, e, c):
        io = e.rows_io.copy()
        return (lambda: L.dctfhe_pbs_rows(c, e.keys.eval.h, 0, p(e.small), N_CT, p(e.tab4), 2, 4, None, 3, 2, 1, p(io), io.shape[0], 2, 512, 1, 7)), [io]

    def round_lut(L, e, c):
        out = _fresh((N_CT, D + 1))
        return (lambda: L.dctfhe_round_lut(c, e.keys.eval.h, 1, 0, p(e.cts), N_CT, 7, 3, p(e.tab4), 2, 4, p(e.idx), p(out))), [out]

    def round_lut_split(L, e, c):
        out = _fresh((N_CT, D + 1))
        return (lambda: L.dctfhe_round_lut_split(c, e.keys.eval.h, 1, 0, 2, p(e.cts), N_CT, 9, 2, p(e.tab7), 2, 7, p(e.idx), p(out))), [out]

    def max_pool_rows(L, e, c):
        out = _fresh((1, 2, 2, 2, D + 1))
        return (lambda: L.dctfhe_max_pool_rows(c, e.keys.eval.h, 0, p(e.pool_in), D, D, 1, 2, 4, 4, 2, 2, 0, 4, p(e.pool_tab), D, p(out))), [out]

    def bench_pbs(L, e, c):
        ms = C.c_double(-1.0)
        return (lambda: L.dctfhe_bench_pbs(c, e.keys.eval.h, 0, 8, 1, C.byref(ms))), [_bytes_of(ms)]

    return {f.__name__: f for f in (encrypt_rows, decrypt_rows, encrypt_seeded, decrypt_packed, decrypt_ring, margin_probe, keyswitch, keyswitch_prefix,
                                    keyswitch_diff, keyswitch_sum, keyswitch_pack, modswitch_center, pbs, pbs_rows, round_lut, round_lut_split,
                                    max_pool_rows, bench_pbs)}


PRIMITIVE_CASES = _primitive_cases()


def _refused_then_accepted(L, make, foreign, own, needle="context", after=None):
    """the call with a foreign context is refused by a message that holds `needle` and leaves its outputs and the device-memory count as
    they were; the same call with matching handles succeeds; the count is back where it was before the pair"""
    held = live()
    call, outs = make(foreign)
    before = [o.copy() for o in outs]
    rc = call()
    msg = L.dctfhe_last_error().decode()
    assert rc != 0, "a handle of another context was accepted"
    assert needle in msg, msg
    for o, b in zip(outs, before):
        assert np.array_equal(o, b), "a refused call wrote to its output"
    assert live() == held
    call, outs = make(own)
    rc = call()
    assert rc == 0, L.dctfhe_last_error().decode()
    if after:
        after()
    assert live() == held
    return outs


@pytest.mark.parametrize("name", sorted(PRIMITIVE_CASES))
def test_foreign_key_handle_refused(ctxs, prim, name):
    """keys of context A, the call made on context B: refused; on A: accepted"""
    a, b = ctxs
    case = PRIMITIVE_CASES[name]
    _refused_then_accepted(a.L, lambda c: case(a.L, prim, c), b.h, a.h)


def test_foreign_keys_refused_by_session_create(ctxs, trunk):
    a, b = ctxs
    L, h = a.L, C.c_void_p()
    make = lambda c: ((lambda: L.dctfhe_session_create(c, trunk.circuit.h, trunk.keys_a.eval.h, trunk.batch, C.byref(h))), [_bytes_of(h)])
    _refused_then_accepted(L, make, b.h, a.h, after=lambda: L.dctfhe_session_destroy(h))


def test_foreign_client_key_refused_by_set_audit(ctxs, trunk):
    """a session of A and the client key made on B from the same seed: the parameters match, the context does not"""
    from dctfhe.engine import Session
    a, b = ctxs
    L = a.L
    s = Session(a, trunk.circuit, trunk.keys_a, trunk.batch)
    try:
        make = lambda client: ((lambda: L.dctfhe_session_set_audit(s.h, client)), [])
        _refused_then_accepted(L, make, trunk.keys_b.client.h, trunk.keys_a.client.h, after=lambda: s.set_audit(None))
        assert s.audit() == []
        s.upload_seeded(trunk.seeded)      # the session is usable after the refusal
        s.run()
        assert np.array_equal(download(trunk, s), trunk.out["encrypted"])
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 2. one circuit, two contexts
@pytest.mark.parametrize("mode", ["clear", "encrypted"])
def test_circuit_shared_by_contexts_of_one_device(ctxs, trunk, mode):
    """the circuit of A under a session of B with B's keys (the same key material: one seed): the all-on-A output, word for word"""
    from dctfhe.engine import Session
    _, b = ctxs
    s = Session(b, trunk.circuit, trunk.keys_b if mode == "encrypted" else None, trunk.batch)
    try:
        if mode == "encrypted":
            s.upload_seeded(trunk.seeded)
        else:
            s.upload(trunk.phases)
        s.run()
        assert np.array_equal(download(trunk, s), trunk.out[mode])
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 3. sharded loopback across contexts
@pytest.mark.parametrize("mode", ["clear", "encrypted"])
def test_sharded_loopback_across_contexts(ctxs, trunk, mode):
    """P = 2, part 0 on A and part 1 on B, own keys each, one circuit; tests/test_gpu_shard.py's drive: every exchange point copies rows from
    A's session to B's and from B's to A's, so dctfhe_session_copy_rows takes its cross-stream branch (event on the source's stream,
    wait on the destination's) in both directions.  A run is synchronous, so a missing wait would lose a race only by accident: this
    executes and checks the branch, it does not prove the wait."""
    from dctfhe.engine import Session
    a, b = ctxs
    enc = mode == "encrypted"
    sessions = [Session(a, trunk.circuit, trunk.keys_a if enc else None, trunk.batch), Session(b, trunk.circuit, trunk.keys_b if enc else None, trunk.batch)]
    try:
        for part, s in enumerate(sessions):
            s.set_shard(part, 2)
            if enc:
                s.upload_seeded(trunk.seeded)
            else:
                s.upload(trunk.phases)
        drive(sessions, trunk.plan, trunk.n_ops)
        for part, s in enumerate(sessions):
            assert np.array_equal(download(trunk, s), trunk.out[mode]), f"part {part}"
    finally:
        for s in sessions:
            s.close()


# ------------------------------------------------------------------------------------------ 4. primitives on a caller's stream
def _all_primitives(e):
    """every primitive once, on whatever stream e.ctx is set to -> name -> words"""
    k, ctx, D = e.keys, e.ctx, e.D
    r = {}
    k.set_encrypt_nonce(NONCE)
    k.set_encrypt_counter(5)
    r["encrypt"] = k.encrypt(e.phases)
    r["decrypt"] = k.decrypt(e.cts)
    k.set_encrypt_counter(5)
    sc = k.encrypt_seeded(e.phases)
    r["encrypt_seeded"] = np.concatenate([np.frombuffer(sc.key, np.uint8).astype(U), np.array([sc.stream], U), sc.bodies])
    r["keyswitch"] = k.keyswitch(0, e.cts, shift=2)
    r["keyswitch_bit_tier"] = k.keyswitch(1, e.cts)
    r["keyswitch_sum"] = k.keyswitch_sum(0, e.rows, e.rows_b, shift=1, body_add=5)
    r["keyswitch_diff"] = k.keyswitch_diff(0, e.rows, e.ia, e.ib, shift=1, body_add=1 << 62)
    r["modswitch_center"] = k.modswitch_center(0, e.small)
    r["pbs"] = k.pbs(0, e.small, e.tab4, 4, e.idx)
    r["pbs_bit_tier"] = k.pbs(1, e.small_bit, e.tab4[:1, :8].copy(), 3)
    r["pbs_rows_store"] = k.pbs_rows(0, e.small, e.tab4, 4, e.rows_io, row0=2, hw=3, nchan=2, e_offset=1, body_add=7)
    r["pbs_rows_accumulate"] = k.pbs_rows(0, e.small, e.tab4, 4, e.rows_io, row0=2, table_idx=e.idx, accumulate=True, body_add=7)
    r["round_lut"] = k.round_lut(1, 0, e.cts, 7, 3, e.tab4, 4, e.idx)
    r["round_lut_split"] = k.round_lut_split(1, 0, 2, e.cts, 9, 2, e.tab7, 7, e.idx)
    r["conv2d_rows_valu"] = ctx.conv2d_rows(e.conv_in[..., :17], 16, e.conv_w, 1, 1, 16)          # dim_o + 1 = 17 < 32: the integer-VALU kernel
    r["conv2d_rows_mfma"] = ctx.conv2d_rows(e.conv_in, 96, e.conv_w, 2, 1, 96)                    # dim_o + 1 = 97 >= 32: the matrix cores
    r["add_rows"] = ctx.add_rows(e.rows[:, :97], 96, e.rows_b[:, :65], 64, 128)
    r["affine_rows"] = ctx.affine_rows(e.rows[:, :97], 96, e.rows[:, :129], 64, 3, 11)
    r["acc_rows"] = ctx.acc_rows(e.rows[:, :129], e.rows_b[:, :97], 80)
    r["gather_rows"] = ctx.gather_rows(e.rows[:, :97], 64, e.gmap, 80)
    r["sum_pool_rows"] = ctx.sum_pool_rows(e.conv_in, 96, 2, 96)
    r["max_pool_rows"] = ctx.max_pool_rows(e.pool_in, D, 2, 2, 0, 4, e.pool_tab, D, keys=k, tier=0)
    r["max_pool_rows_clear"] = ctx.max_pool_rows(e.pool_in[..., 0], 0, 3, 2, 1, 4)
    r["keyswitch_pack"] = k.keyswitch_pack(0, e.rows, D).rows
    r["ring_pack"] = e.pack.ring_pack(e.small).words
    e.pub.set_encrypt_seed(bytes(range(32)))
    pi = e.pub.encrypt(e.phases)
    r["encrypt_public"] = pi.words
    r["ring_extract"] = ctx.ring_extract(pi, dim=300)
    err, st = k.margin_probe(0, e.small, 4)
    r["margin_probe"] = np.concatenate([err.astype(np.int64), np.array([st["max_abs"], st["count"], st["sum"], st["sum_sq"]] + st["hist"], np.int64)])
    return r


def test_primitives_on_a_callers_stream(ctxs, prim):
    """Every primitive on a non-blocking torch stream, bit for bit what it gives on the context's own stream, and once more after
    set_stream(None).  The caller's stream carries nothing else here: this pins the words; the ordering is test_library_work_is_ordered's."""
    a, _ = ctxs
    own = _all_primitives(prim)
    held = live()      # after the first pass: what the keys cache on first use is theirs to keep
    side = torch.cuda.Stream(torch.device("cuda:0"))
    assert side.cuda_stream != 0
    try:
        a.set_stream(side.cuda_stream)
        on_side = _all_primitives(prim)
        a.set_stream(side)                  # the same stream as a torch object
        assert np.array_equal(prim.keys.keyswitch(0, prim.cts, shift=2), own["keyswitch"])
    finally:
        a.set_stream(None)
    back = _all_primitives(prim)
    assert set(own) == set(on_side) == set(back)
    for name, want in own.items():
        assert want.size and np.array_equal(on_side[name], want), f"{name} on the caller's stream"
        assert np.array_equal(back[name], want), f"{name} after set_stream(None)"
    assert (own["pbs_rows_store"] != own["pbs_rows_accumulate"]).any() and (own["conv2d_rows_mfma"] != 0).any()
    assert live() == held


# ------------------------------------------------------------------------------------------ 5. ordered after the caller's work
def delayed_run(t, ctx, mode, chain, side, on_side, create_first):
    """A session whose real input arrives LATE on the stream `side`: a normal upload of zeros, then on `side` a chain of `chain` matmuls,
    the device-to-device copy of the real rows into the session's input tensor and an event; then run and download with no host
    synchronisation in between.  on_side: the context is set to `side` (before or after the session is created); otherwise it stays on
    its own stream and the run races the copy.  -> (the side stream was still busy when the host reached the library, the event had
    completed when the download returned, the output words)"""
    from dctfhe.engine import Session
    from dctfhe.sharding import tensor_view
    keys = (t.keys_a if ctx is t.keys_a.ctx else t.keys_b) if mode == "encrypted" else None
    s = None
    try:
        if on_side and not create_first:
            ctx.set_stream(side)
        s = Session(ctx, t.circuit, keys, t.batch)
        if on_side and create_first:
            ctx.set_stream(side)
        upload_zero(t, s, mode)
        view = tensor_view(s, t.t_in, t.dev)
        assert view.shape == t.real_rows[mode].shape
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(chain):
                torch.matmul(t.mm, t.mm, out=t.mm_out)
            view.copy_(t.real_rows[mode], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        busy = not ev.query()
        s.run()
        out = download(t, s)
        done = ev.query()
        return busy, done, out
    finally:
        side.synchronize()      # the late copy has landed before the session's memory is freed
        ctx.set_stream(None)
        if s is not None:
            s.close()


def control_stream(t, ctx, mode, chain=DELAY_CHAIN, tries=8):
    """The control: the identical sequence with the context left on its OWN stream.  Nothing orders the run after the side stream, so
    it must read the stale (all-zero, in-bounds) input: a data race on purpose, not a fault.  -> the side stream on which it did.
    One thing besides a short delay lets the unordered run see the real rows: the device serves a process's streams from a few hardware
    queues (4 here), and two streams that share one run in submission order whatever the delay.  Measured: about one new torch stream
    in four is ordered with the context's own in this way, at every chain length up to 16 (profiles/streams_contexts.json).  On such a
    stream a stray launch on the context's own stream could not be seen either, so the probe does not use it: the control is repeated
    on the next new stream.  When no stream of `tries` reads stale the probe means nothing: inconclusive, and a failure."""
    reads = []
    for _ in range(tries):
        side = torch.cuda.Stream(t.dev)
        busy, _, out = delayed_run(t, ctx, mode, chain, side, False, True)
        assert busy, "the side stream had drained before the host reached the library (longer delay?)"
        if np.array_equal(out, t.zero_out[mode]):
            return side
        reads.append("real" if np.array_equal(out, t.out[mode]) else "part of each")
    pytest.fail(f"inconclusive: the unordered control never read the stale input on {tries} streams ({reads}); DELAY_CHAIN = {chain} needs to be longer here")


@pytest.mark.parametrize("create_first", [True, False], ids=["session-before-set_stream", "session-after-set_stream"])
@pytest.mark.parametrize("mode", ["clear", "encrypted"])
def test_library_work_is_ordered_after_the_callers(ctxs, trunk, mode, create_first):
    """The context on the caller's non-blocking stream: the run must see the rows that the caller's delayed copy writes, i.e. every copy,
    fill and kernel of the run is ordered after it on that stream.  A launch that went to another stream (the context's own, the stream
    of a handle of another context, the null stream) would read the zeros instead and change output words.  A session follows its
    context's stream at call time, so it does not matter whether it was created before or after set_stream.
    First the control on the same side stream (control_stream): with the context on its own stream the outputs are those of the ZERO
    input, so the delay is long enough and the two streams are not ordered by the hardware.
    Delay, measured on an MI355X: one 4096^2 float32 matmul takes 0.95 ms.  The control reads stale from a chain of 1 in clear mode;
    in encrypted mode a chain of 1 lets the copy land while the first convolution reads (part of each input), a chain of 2 reads
    stale: DELAY_CHAIN_MIN = 2, and 4 x 2 = 8 products (7.6 ms) are shipped."""
    a, _ = ctxs
    side = control_stream(trunk, a, mode)
    busy, done, out = delayed_run(trunk, a, mode, DELAY_CHAIN, side, True, create_first)
    assert busy, "the side stream had drained before the host reached the library: the probe shows nothing (longer delay?)"
    assert np.array_equal(out, trunk.out[mode]), "the run did not wait for the caller's work on its stream"
    assert not np.array_equal(out, trunk.zero_out[mode])
    assert done, "the run returned before the caller's work on the stream it was set to had completed"


# ------------------------------------------------------------------------------------------ 6. synchronize waits for the stream that is set
def test_ctx_synchronize_waits_for_the_set_stream(ctxs, trunk):
    a, _ = ctxs
    side = torch.cuda.Stream(trunk.dev)
    try:
        a.set_stream(side)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(DELAY_CHAIN):
                torch.matmul(trunk.mm, trunk.mm, out=trunk.mm_out)
            ev = torch.cuda.Event()
            ev.record(side)
        assert not ev.query()
        a.synchronize()
        assert ev.query()
    finally:
        side.synchronize()
        a.set_stream(None)


# ------------------------------------------------------------------------------------------ 7. two host threads, two contexts
def test_two_host_threads_two_contexts(trunk):
    """One context per host thread (include/dctfhe.h): each thread makes its own context, keys (one seed), circuit and session and runs
    the trunk encrypted three times while the other does the same (ctypes releases the GIL during a call).  Every output is the
    single-threaded one.  In the middle thread 1 leaves a refusal of its own in dctfhe_last_error(), thread 0 then provokes another (a
    tier out of range), and thread 1 still reads its own."""
    from dctfhe.engine import Circuit, Context, Keys, Session
    L = trunk.circuit.L
    WAIT = 120.0
    own_set, other_failed = threading.Event(), threading.Event()
    result = [dict(outs=[], error=None, msgs=None) for _ in range(2)]

    def work(me):
        res = result[me]
        ctx = keys = circ = sess = None
        try:
            ctx = Context(0)
            keys = Keys(ctx, trunk.cparams, seed=3)
            circ = Circuit(ctx, trunk.qm.compiled.blob)
            sess = Session(ctx, circ, keys, trunk.batch)
            sess.upload_seeded(trunk.seeded)
            small = np.zeros((1, 64), U)
            cts = np.zeros((1, keys.D + 1), U)
            for run in range(3):
                sess.run()
                res["outs"].append(sess.download(trunk.out_dim))
                if run != 0:
                    continue
                if me == 1:
                    assert L.dctfhe_keyswitch_prefix(ctx.h, keys.eval.h, 0, p(cts), 1, 0, keys.D + 9, p(small)) != 0
                    mine = L.dctfhe_last_error().decode()
                    own_set.set()
                    if not other_failed.wait(WAIT):
                        raise TimeoutError("thread 0 never provoked its refusal")
                    res["msgs"] = (mine, L.dctfhe_last_error().decode())
                else:
                    if not own_set.wait(WAIT):
                        raise TimeoutError("thread 1 never left its own message")
                    assert L.dctfhe_keyswitch(ctx.h, keys.eval.h, 99, p(cts), 1, 0, p(small)) != 0
                    res["msgs"] = (L.dctfhe_last_error().decode(),)
                    other_failed.set()
        except BaseException as e:      # noqa: BLE001 -- reported by the test's own thread
            res["error"] = e
            own_set.set()
            other_failed.set()
        finally:
            for h in (sess, circ, keys, ctx):
                if h is not None:
                    h.close()

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    t0 = time.monotonic()
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, 2 * WAIT - (time.monotonic() - t0)))
    if any(th.is_alive() for th in threads):
        pytest.fail("a worker thread has not returned")
    for me, res in enumerate(result):
        if res["error"] is not None:
            raise res["error"]
        assert len(res["outs"]) == 3
        for run, out in enumerate(res["outs"]):
            assert np.array_equal(out, trunk.out["encrypted"]), f"thread {me}, run {run}"
    assert "tier out of range" in result[0]["msgs"][0]
    mine, after = result[1]["msgs"]
    assert "deff out of range" in mine and after == mine
