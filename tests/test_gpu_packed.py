"""Packed result ciphertexts on the GPU (include/dctfhe.h dctfhe_keyswitch_pack, dctfhe_session_download_packed, dctfhe_decrypt_packed;
DESIGN.md section 3.6): the pack primitive bit for bit against the existing key switch + the numpy rounding (tests/packed_ref.py), packed
decryption against its numpy twin, the noise a packed result carries against the compiler's price, a session's packed download, the
QuantizedModule switch across a client / server split, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import packed_ref

pytestmark = pytest.mark.gpu


def _cent(x):
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


def _param_set(name):
    from dctfhe import params as P
    return P.test_params() if name == "test" else P.default_params()


@pytest.fixture(scope="module")
def keysets(gpu_ctx):
    """one key pair per catalogue, made on first use and shared by the tests of this module"""
    from dctfhe import params as P
    from dctfhe.engine import Keys
    made = {}

    def get(name):
        if name not in made:
            ps = _param_set(name)
            made[name] = (ps, Keys(gpu_ctx, P.to_c_params(ps), seed=5))
        return made[name]
    yield get
    for _, k in made.values():
        k.close()


def full_width(cts, D):
    """compact rows [count, dim + 1] -> full-width rows [count, D + 1]: zeros from dim on, the body last"""
    out = np.zeros((cts.shape[0], D + 1), np.uint64)
    out[:, :cts.shape[1] - 1] = cts[:, :-1]
    out[:, D] = cts[:, -1]
    return out


def _oracle(qm, q):
    from oracle import circuit_ref
    out, ov = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not ov
    return qm.decode_output(out)


# ------------------------------------------------------------------------------------------ 1. the primitive, bit for bit
def _check_pack(keys, tier, count, dim, deff, seed):
    rng = np.random.default_rng(seed)
    cts = rng.integers(0, 1 << 64, (count, dim + 1), dtype=np.uint64)
    if deff:
        cts[:, deff:dim] = 0                                       # the contract of deff: the caller knows these to be zero
    got = keys.keyswitch_pack(tier, cts, dim, deff)
    n = keys.tier(tier).n
    assert got.n == n and got.rows.shape == (count, n + 1) and got.rows.dtype == np.uint16
    want = packed_ref.pack16(keys.keyswitch(tier, full_width(cts, keys.D), 0, deff or dim))
    assert np.array_equal(got.rows, want), (count, dim, deff)


# counts: 1, a partial tile, one past the 128-row matrix-core tile, one past the 16384-ciphertext scratch chunk
@pytest.mark.parametrize("count", [1, 7, 129, 16385])
@pytest.mark.parametrize("dim,deff", [(1024, 1024), (1024, 256), (256, 0)])
def test_keyswitch_pack_small_rings(keysets, count, dim, deff):
    _, keys = keysets("test")
    _check_pack(keys, 0, count, dim, deff, seed=count + dim + deff)


@pytest.mark.parametrize("dim,deff", [(8192, 0), (2048, 2048)])
def test_keyswitch_pack_default_tier(keysets, dim, deff):
    _, keys = keysets("default")
    _check_pack(keys, 0, 3, dim, deff, seed=dim)


@pytest.mark.parametrize("pname", ["test", "default"])
def test_rounding_edges_through_the_pack(keysets, pname):
    """trivial ciphertexts (zero mask): the key switch hands the body through, so the pack's rounding is seen word for word"""
    _, keys = keysets(pname)
    bodies = np.array([0x00007FFFFFFFFFFF, 0x0000800000000000, 0xFFFF800000000000, 0xFFFF7FFFFFFFFFFF], np.uint64)
    cts = np.zeros((4, keys.D + 1), np.uint64)
    cts[:, keys.D] = bodies
    n = keys.tier(0).n
    small = keys.keyswitch(0, cts)                                  # first through the existing primitive ...
    assert np.array_equal(small[:, n], bodies) and not small[:, :n].any()
    got = keys.keyswitch_pack(0, cts, keys.D).rows                  # ... then through the pack
    assert got[:, n].tolist() == [0x0000, 0x0001, 0x0000, 0xFFFF]   # down, tie up, carry out of the top wraps to 0, no carry
    assert not got[:, :n].any()
    assert np.array_equal(got, packed_ref.pack16(small))


# ------------------------------------------------------------------------------------------ 2. packed decryption
@pytest.mark.parametrize("pname,n,count", [("test", 1, 1), ("test", 47, 5), ("test", 48, 1000), ("default", 800, 3)])
def test_decrypt_packed_equals_reference(keysets, pname, n, count):
    from dctfhe.engine import PackedCiphertexts
    _, keys = keysets(pname)
    _, s = keys.export_secret()
    rows = np.random.default_rng(n * 1000 + count).integers(0, 1 << 16, (count, n + 1), dtype=np.uint16)
    if count >= 5:
        rows[0], rows[1] = 0xFFFF, 0                               # the largest sum of the row, and none
    got = keys.decrypt_packed(PackedCiphertexts(n, rows))
    assert got.dtype == np.uint64 and np.array_equal(got, packed_ref.decrypt_packed(rows, s, n))


# ------------------------------------------------------------------------------------------ 3. noise
@pytest.mark.parametrize("pname,dim", [("test", 1024), ("default", 2048)])
def test_packed_noise_matches_model(keysets, pname, dim):
    """what key switch + 16-bit rounding add to a fresh ciphertext, against the compiler's price var_keyswitch(deff, t) + var_round16(n)
    (the fresh encryption's own noise, 2^-55 / 2^-51.6, is far below both).  The band is the key-switch calibration's, 0.7 .. 1.3 x the
    model (tests/test_gpu_noise.py), here held on the variance itself -- the tighter reading, which implies the band on sigma."""
    from dctfhe import params as P
    ps, keys = keysets(pname)
    t = ps.tiers[0]
    phase = np.uint64(0x2B5D3A9C17E4F681)
    phases = np.full(4096, phase, np.uint64)
    cts = keys.encrypt(phases, dim)
    packed = keys.keyswitch_pack(0, cts, dim, dim)
    err = _cent(keys.decrypt_packed(packed) - phase)
    model = P.var_keyswitch(dim, t) + P.var_round16(t.n)
    print(f"{pname}: packed noise var 2^{math.log2(err.var()):.2f} (mean {err.mean():.2e}), model 2^{math.log2(model):.2f} "
          f"(key switch 2^{math.log2(P.var_keyswitch(dim, t)):.2f}, rounding 2^{math.log2(P.var_round16(t.n)):.2f}), ratio {err.var() / model:.3f}")
    assert 0.7 * model < err.var() < 1.3 * model, (pname, err.var(), model)


# ------------------------------------------------------------------------------------------ 4. sessions
def _tiny(ps, configuration=None):
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=ps, configuration=configuration)
    return qm, calib


def test_session_download_packed_small_rings():
    from dctfhe import params as P
    qm, calib = _tiny(P.test_params())
    try:
        qm.fhe_circuit.keygen(seed=4)
        keys = qm._keys
        q = qm.quantize_input(calib[:3])
        oc = qm.output_compaction()
        sess = qm._session("execute", 3)
        in_dim, out_dim = sess.dims()
        sess.upload(keys.encrypt(qm.encode_input(q).reshape(-1), in_dim), in_dim)
        sess.run()
        packed = sess.download_packed(oc.tier)
        full = sess.download().reshape(-1, keys.D + 1)
        assert len(packed) == 3 * qm._circuit.n_out and packed.n == oc.n
        assert np.array_equal(packed.rows, packed_ref.pack16(keys.keyswitch(oc.tier, full, 0, out_dim)))       # row for row
        got = qm.decode_output(keys.decrypt_packed(packed).reshape(3, -1))
        assert np.array_equal(got, _oracle(qm, q))
        assert np.array_equal(qm.decrypt_result(packed), got) and np.array_equal(qm.decrypt_result(full), got)
    finally:
        qm.close()


def test_session_download_packed_default_catalogue():
    from dctfhe import params as P
    qm, calib = _tiny(P.default_params())
    try:
        qm.fhe_circuit.keygen(seed=4)
        keys = qm._keys
        q = qm.quantize_input(calib[:1])
        oc = qm.output_compaction()
        assert (oc.name, oc.n) == ("T6", 800)
        sess = qm._session("execute", 1)
        in_dim, _ = sess.dims()
        sess.upload(keys.encrypt(qm.encode_input(q).reshape(-1), in_dim), in_dim)
        sess.run()
        packed = sess.download_packed(oc.tier)
        assert packed.rows.shape == (qm._circuit.n_out, 801)
        assert np.array_equal(qm.decode_output(keys.decrypt_packed(packed).reshape(1, -1)), _oracle(qm, q))
    finally:
        qm.close()


# ------------------------------------------------------------------------------------------ 5. facade, client / server split
def test_facade_and_split_with_all_three_switches():
    from dctfhe import params as P
    from dctfhe.engine import PackedCiphertexts
    from dctfhe.quantized_module import Configuration, QuantizedModule
    cfg = Configuration(compress_input_ciphertexts=True, compress_evaluation_keys=True, compress_output_ciphertexts=True)
    client, calib = _tiny(P.test_params(), cfg)
    server = QuantizedModule(client.compiled, configuration=cfg)         # key-less: evaluation keys arrive as a blob
    try:
        client.fhe_circuit.keygen(seed=8)
        B = 3
        q = client.quantize_input(calib[:B])
        want = _oracle(client, q)
        n, n_out = client.output_compaction().n, client.compiled.n_out()
        # the client alone, through the switches
        assert np.array_equal(client.forward_quantized(q, "execute"), want)
        assert client.last_io["output_bytes"] == 2 * (n + 1) * B * n_out
        # client -> server -> client: compressed keys, seeded inputs and packed results, all as bytes
        server.fhe_circuit.load_evaluation_keys(client.fhe_circuit.export_evaluation_keys())
        sc = client._keys.encrypt_seeded(client.encode_input(q).reshape(-1))
        out = server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B)
        assert isinstance(out, PackedCiphertexts) and out.n == n and len(out) == B * n_out
        assert np.array_equal(client.decrypt_result(out.to_bytes()), want)
        # packed=False overrides the configuration: full-width rows as before
        rows = server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B, packed=False)
        assert rows.shape == (B * n_out, client._keys.D + 1) and np.array_equal(client.decrypt_result(rows), want)
        with pytest.raises(RuntimeError, match="client key"):
            server.decrypt_result(out)
    finally:
        server.close()
        client.close()


# ------------------------------------------------------------------------------------------ 6. refusals
def _fails(L, rc, needle):
    assert rc != 0
    msg = L.dctfhe_last_error().decode()
    assert needle in msg, msg


def test_refusals(gpu_ctx, keysets):
    from dctfhe import compile as cc, models
    from dctfhe.engine import Circuit, Session
    ps, keys = keysets("test")
    L, D, n, nt = gpu_ctx.L, keys.D, ps.tiers[0].n, len(ps.tiers)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    compiled = cc.compile_model(models.tiny_resnet_q(), np.random.default_rng(0).normal(0, 1, (16, 4, 6, 6)), param_set=ps)
    circ = Circuit(gpu_ctx, compiled.blob)
    clear, sess = Session(gpu_ctx, circ, None, 1), Session(gpu_ctx, circ, keys, 1)
    try:
        rows = np.zeros((circ.n_out, ps.n_max + 1), np.uint16)
        _fails(L, L.dctfhe_session_download_packed(clear.h, 0, p(rows)), "clear-mode")
        _fails(L, L.dctfhe_session_download_packed(sess.h, -1, p(rows)), "out of range")
        _fails(L, L.dctfhe_session_download_packed(sess.h, nt, p(rows)), "out of range")
        _fails(L, L.dctfhe_session_download_packed(None, 0, p(rows)), "null")
        _fails(L, L.dctfhe_session_download_packed(sess.h, 0, None), "null")
        cts = np.zeros((2, D + 2), np.uint64)
        out = np.zeros((2, n + 1), np.uint16)
        _fails(L, L.dctfhe_keyswitch_pack(None, keys.eval.h, 0, p(cts), 2, D, 0, p(out)), "null")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, None, 0, p(cts), 2, D, 0, p(out)), "null")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, 0, None, 2, D, 0, p(out)), "null")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, 0, p(cts), 2, D, 0, None), "null")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, -1, p(cts), 2, D, 0, p(out)), "out of range")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, nt, p(cts), 2, D, 0, p(out)), "out of range")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, 0, p(cts), 2, D + 1, 0, p(out)), "the key has")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, 0, p(cts), 2, 0, 0, p(out)), "the key has")
        _fails(L, L.dctfhe_keyswitch_pack(gpu_ctx.h, keys.eval.h, 0, p(cts), 2, 256, 257, p(out)), "effective dimension")
        ph = np.zeros(2, np.uint64)
        prow = np.zeros((2, ps.n_max + 2), np.uint16)
        _fails(L, L.dctfhe_decrypt_packed(None, keys.client.h, n, p(prow), 2, p(ph)), "null")
        _fails(L, L.dctfhe_decrypt_packed(gpu_ctx.h, None, n, p(prow), 2, p(ph)), "null")
        _fails(L, L.dctfhe_decrypt_packed(gpu_ctx.h, keys.client.h, n, None, 2, p(ph)), "null")
        _fails(L, L.dctfhe_decrypt_packed(gpu_ctx.h, keys.client.h, n, p(prow), 2, None), "null")
        _fails(L, L.dctfhe_decrypt_packed(gpu_ctx.h, keys.client.h, 0, p(prow), 2, p(ph)), "the small key has")
        _fails(L, L.dctfhe_decrypt_packed(gpu_ctx.h, keys.client.h, ps.n_max + 1, p(prow), 2, p(ph)), "the small key has")
        # the Python layer turns them into DctfheError, and the handles still work after all that
        from dctfhe._lib import DctfheError
        with pytest.raises(DctfheError, match="clear-mode"):
            clear.download_packed(0)
        with pytest.raises(DctfheError, match="out of range"):
            sess.download_packed(nt)
        ok = keys.keyswitch_pack(0, np.zeros((1, D + 1), np.uint64), D)
        assert not ok.rows.any() and keys.decrypt_packed(ok).tolist() == [0]
    finally:
        sess.close()
        clear.close()
        circ.close()
