"""Ring-packed result ciphertexts on the GPU (include/dctfhe.h dctfhe_pack_key_export / _import, dctfhe_ring_pack, dctfhe_session_download_ring,
dctfhe_decrypt_ring): the pack bit for bit against the numpy reference (tests/ring_ref.py) on the server's expanded key,
the packing key's masks, phases and noise, the noise a ring-packed result carries against the compiler's price, the client's decryption, a
session's ring download, the QuantizedModule switch across a client / server split, and the refusals."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import ring_ref

pytestmark = pytest.mark.gpu
U = np.uint64


def _cent(x):
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


def ring_stream(logN, l, beta, sigma):
    """the generator stream of a spec's masks, as include/dctfhe.h documents it (noise: + 1)"""
    bits, = struct.unpack("<Q", struct.pack("<d", sigma))
    return (1 << 63) | (((bits * 0x9E3779B97F4A7C15 % (1 << 64)) ^ (logN << 24 | l << 16 | beta << 8)) & 0x7FFFFFFFFFFFFFFE)


@pytest.fixture(scope="module")
def keysets(gpu_ctx):
    """one key pair per catalogue, made on first use and shared by the tests of this module"""
    from dctfhe import params as P
    from dctfhe.engine import Keys
    made = {}

    def get(name):
        if name not in made:
            ps = P.test_params() if name == "test" else P.default_params()
            made[name] = (ps, Keys(gpu_ctx, P.to_c_params(ps), seed=5))
        return made[name]
    yield get
    for _, k in made.values():
        k.close()


@pytest.fixture(scope="module")
def packkeys(gpu_ctx, keysets):
    """(spec, blob, imported PackKey, its expanded rows [n_max, l, 2, N]) per (catalogue, logN, l, beta), made once"""
    from dctfhe import params as P
    from dctfhe.engine import PackKey
    made = {}

    def get(name, logN, l, beta):
        k = (name, logN, l, beta)
        if k not in made:
            spec = P.PackSpec(logN=logN, l=l, beta=beta, sigma=2.0 ** -48 if name == "test" else None)
            blob = keysets(name)[1].export_pack_key(spec)
            pk = PackKey(gpu_ctx, blob)
            made[k] = (spec, blob, pk, pk.export_rows())
        return made[k]
    yield get
    for _, _, pk, _ in made.values():
        pk.close()


def _oracle(qm, q):
    from oracle import circuit_ref
    out, ov = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not ov
    return qm.decode_output(out)


def _want(small, rows, spec):
    return ring_ref.pack16(ring_ref.pack(small, rows, spec.l, spec.beta), small.shape[0])


# ------------------------------------------------------------------------------------------ 1. the primitive, bit for bit
# counts: one result, two, one short of a ring, a full ring, one past it, two rings and a partial third
@pytest.mark.parametrize("l,beta", [(1, 16), (2, 8), (3, 5)])
@pytest.mark.parametrize("n", [1, 47, 48])
@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 519])
def test_ring_pack_test_ring(packkeys, count, n, l, beta):
    spec, _, pk, rows = packkeys("test", 8, l, beta)
    small = np.random.default_rng(1000 * count + 10 * n + l).integers(0, 1 << 64, (count, n + 1), dtype=U)
    got = pk.ring_pack(small)
    assert (got.logN, got.count) == (8, count) and got.words.dtype == np.uint16 and got.words.size == spec.words(count)
    assert np.array_equal(got.words, _want(small, rows, spec)), (count, n, l, beta)


def test_ring_pack_ring_of_1024(packkeys):
    spec, _, pk, rows = packkeys("test", 10, 1, 16)
    small = np.random.default_rng(10).integers(0, 1 << 64, (1031, 49), dtype=U)
    assert np.array_equal(pk.ring_pack(small).words, _want(small, rows, spec))


# n = 8 with 2051 results: every sign wrap of a full ring of 2048 and a second group
@pytest.mark.parametrize("n,count", [(800, 3), (800, 70), (8, 2051)])
def test_ring_pack_default_spec(packkeys, n, count):
    spec, _, pk, rows = packkeys("default", 11, 1, 16)
    assert rows.shape == (800, 1, 2, 2048)
    small = np.random.default_rng(n + count).integers(0, 1 << 64, (count, n + 1), dtype=U)
    got = pk.ring_pack(small)
    assert got.words.size == spec.words(count)
    assert np.array_equal(got.words, _want(small, rows, spec)), (n, count)


@pytest.mark.parametrize("pname,logN", [("test", 8), ("default", 11)])
def test_rounding_edges_through_the_pack(packkeys, pname, logN):
    """a zero mask hands the body through, so the pack's rounding is seen word for word"""
    spec, _, pk, rows = packkeys(pname, logN, 1, 16)
    n = rows.shape[0]
    small = np.zeros((4, n + 1), U)
    small[:, n] = np.array([0x00007FFFFFFFFFFF, 0x0000800000000000, 0xFFFF800000000000, 0xFFFF7FFFFFFFFFFF], U)
    got = pk.ring_pack(small).words
    assert got[spec.N:].tolist() == [0x0000, 0x0001, 0x0000, 0xFFFF]    # down, tie up, carry out of the top wraps to 0, no carry
    assert not got[:spec.N].any()
    assert np.array_equal(got, _want(small, rows, spec))


@pytest.mark.parametrize("l,beta", [(1, 16), (2, 8), (3, 5)])
def test_digit_edges_through_the_pack(packkeys, l, beta):
    """mask words at the digit -B/2, along the carry chain and at the dropped top carry"""
    spec, _, pk, rows = packkeys("test", 8, l, beta)
    edges = np.array([0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0xFFFF800000000000, 0xFFFFFFFFFFFFFFFF, 0x7FFF800000000000, 0x0000800000000000,
                      0xF800000000000000, 0xFBFFFFFFFFFFFFFF], U)
    small = np.zeros((edges.size + 1, 49), U)
    for i, e in enumerate(edges):
        small[i, i % 48] = e
        small[i, 47 - i] += e >> U(i)
    small[-1, :48] = np.resize(edges, 48)
    small[:, 48] = np.arange(small.shape[0], dtype=U) << U(50)
    d = ring_ref.decompose(edges[:3], l, beta)
    assert d[0, 0] == -(1 << (beta - 1)) and d[1, 0] == -(1 << (beta - 1)) and not d[2].any()
    assert np.array_equal(pk.ring_pack(small).words, _want(small, rows, spec))


# ------------------------------------------------------------------------------------------ 2. the key
@pytest.mark.parametrize("l,beta", [(1, 16), (2, 8)])
def test_pack_key_masks_phases_and_noise(gpu_ctx, keysets, packkeys, l, beta):
    ps, keys = keysets("test")
    spec, blob, pk, rows = packkeys("test", 8, l, beta)
    N, n_max = spec.N, ps.n_max
    # the blob: header, the public generator key, the bodies
    magic, version, logN, l_, beta_, nm, sigma, total = struct.unpack_from("<4sIiiiidQ", blob.tobytes())
    assert (magic, version, logN, l_, beta_, nm, sigma, total) == (b"DRPK", 1, 8, l, beta, n_max, spec.sigma, blob.size)
    assert blob.size == 40 + 32 + 8 * n_max * l * N and (pk.logN, pk.l, pk.beta, pk.n_max, pk.sigma) == (8, l, beta, n_max, spec.sigma)
    bodies = np.frombuffer(blob.tobytes(), "<u8", n_max * l * N, 72).reshape(n_max, l, N)
    assert rows.shape == (n_max, l, 2, N) and np.array_equal(rows[:, :, 1], bodies)
    # masks: generator word (pub, R, r N + c) of the public key the blob carries
    draws = np.empty(n_max * l * N, U)
    assert gpu_ctx.L.dctfhe_rng_device(gpu_ctx.h, blob[40:72].tobytes(), C.c_uint64(ring_stream(8, l, beta, spec.sigma)), 0, draws.size,
                                       draws.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(rows[:, :, 0].reshape(-1), draws)
    # phases under Z = the first N bits of the big key: s_j g at coefficient 0, noise everywhere
    S, s = keys.export_secret()
    A, B = rows[:, :, 0], rows[:, :, 1].copy()
    for c in np.flatnonzero(S[:N]):
        B -= ring_ref.negashift(A, int(c))
    for lev in range(l):
        B[:, lev, 0] -= s[:n_max].astype(U) << U(64 - beta * (lev + 1))
    noise = _cent(B)
    assert np.abs(noise).max() < 6.5 * spec.sigma
    var = float((noise ** 2).mean())
    print(f"packing key ({l} x {beta} bits): noise var 2^{math.log2(var):.2f} over {noise.size} coefficients, sigma_p^2 2^{2 * math.log2(spec.sigma):.2f}, "
          f"ratio {var / spec.sigma ** 2:.3f}")
    assert 0.7 * spec.sigma ** 2 < var < 1.3 * spec.sigma ** 2


def test_two_sigmas_of_one_client_key_share_no_draw(gpu_ctx, keysets, packkeys):
    """the Gaussian draw scales with sigma_p, so sigma_p is part of the stream id: a second export at another sigma_p has other masks,
    and the difference of the bodies is not a multiple of one noise polynomial"""
    from dctfhe import params as P
    _, keys = keysets("test")
    _, blob, _, rows = packkeys("test", 8, 1, 16)
    other = keys.export_pack_key(P.PackSpec(logN=8, l=1, beta=16, sigma=2.0 ** -40))
    assert ring_stream(8, 1, 16, 2.0 ** -40) != ring_stream(8, 1, 16, 2.0 ** -48)
    draws = np.empty(256, U)
    assert gpu_ctx.L.dctfhe_rng_device(gpu_ctx.h, other[40:72].tobytes(), C.c_uint64(ring_stream(8, 1, 16, 2.0 ** -40)), 0, 256,
                                       draws.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(blob[40:72], other[40:72]) and not np.array_equal(draws, rows[0, 0, 0])
    b0, b1 = (np.frombuffer(x.tobytes(), "<u8", 256, 72) for x in (blob, other))
    assert np.abs(_cent(b1 - b0)).mean() > 0.1                       # other masks: the difference is uniform on the torus, not sigma-sized


# ------------------------------------------------------------------------------------------ 3. noise
@pytest.mark.parametrize("pname,logN,calls", [("test", 8, 256), ("default", 11, 128)])
def test_ring_noise_matches_model(keysets, packkeys, pname, logN, calls):
    """what the ring pack adds to noise-free small ciphertexts of one constant phase, against var_ring_pack(n, spec, 64).  One pack is not
    a sample -- its slots share the mask's rounding errors through shifts of one key -- so the variance is taken over independent packs of
    64 slots.  Band: 0.7 .. 1.3 x the model, as for the packed rows."""
    from dctfhe import params as P
    ps, keys = keysets(pname)
    spec, _, pk, _ = packkeys(pname, logN, 1, 16)
    n, m = ps.tiers[0].n, 64
    _, s = keys.export_secret()
    sk = s[:n].astype(U)
    phase = U(0x2B5D3A9C17E4F681)
    rng = np.random.default_rng(logN)
    errs = []
    for _ in range(calls):
        small = rng.integers(0, 1 << 64, (m, n + 1), dtype=U)
        small[:, n] = (small[:, :n] * sk).sum(axis=1, dtype=U) + phase
        errs.append(_cent(keys.decrypt_ring(pk.ring_pack(small)) - phase))
    err = np.concatenate(errs)
    model = P.var_ring_pack(n, spec, m)
    var = float((err ** 2).mean())
    print(f"{pname}: ring-pack noise var 2^{math.log2(var):.2f} (mean {err.mean():.2e}) over {calls} packs of {m}, model 2^{math.log2(model):.2f}, "
          f"ratio {var / model:.3f}")
    assert 0.7 * model < var < 1.3 * model, (pname, var, model)


# ------------------------------------------------------------------------------------------ 4. the client
@pytest.mark.parametrize("pname,logN,count", [("test", 8, 1), ("test", 8, 256), ("test", 8, 257), ("default", 11, 70)])
def test_decrypt_ring_equals_reference(keysets, pname, logN, count):
    from dctfhe.engine import PackedRing
    _, keys = keysets(pname)
    S, _ = keys.export_secret()
    words = np.random.default_rng(logN * 1000 + count).integers(0, 1 << 16, PackedRing.n_words(logN, count), dtype=np.uint16)
    got = keys.decrypt_ring(PackedRing(logN, count, words))
    assert got.dtype == U and np.array_equal(got, ring_ref.decrypt16(words, S, logN, count))


def test_decrypt_ring_of_all_ones(keysets):
    from dctfhe.engine import PackedRing
    _, keys = keysets("test")
    S, _ = keys.export_secret()
    words = np.full(512, 0xFFFF, np.uint16)
    got = keys.decrypt_ring(PackedRing(8, 256, words))
    assert np.array_equal(got, ring_ref.decrypt16(words, S, 8, 256))


# ------------------------------------------------------------------------------------------ 5. sessions
def _tiny(ps, configuration=None):
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=ps, configuration=configuration)
    return qm, calib


def test_session_download_ring_small_rings():
    from dctfhe import params as P
    from dctfhe.quantized_module import Configuration
    qm, calib = _tiny(P.test_params(), Configuration(result_packing_spec=P.test_pack_spec()))
    try:
        qm.fhe_circuit.keygen(seed=4)
        keys = qm._keys
        qm.fhe_circuit.load_result_packing_key(qm.fhe_circuit.export_result_packing_key())
        q = qm.quantize_input(calib[:3])
        oc = qm.output_compaction("ring")
        sess = qm._session("execute", 3)
        in_dim, out_dim = sess.dims()
        sess.upload(keys.encrypt(qm.encode_input(q).reshape(-1), in_dim), in_dim)
        sess.run()
        ring = sess.download_ring(oc.tier, qm._pack_key)
        full = sess.download().reshape(-1, keys.D + 1)
        count = 3 * qm._circuit.n_out
        assert len(ring) == count and ring.logN == 8 and ring.words.size == oc.spec.words(count) and 2 * ring.words.size == oc.bytes_per_batch(3)
        small = keys.keyswitch(oc.tier, full, 0, out_dim)
        assert np.array_equal(ring.words, _want(small, qm._pack_key.export_rows(), oc.spec))              # word for word
        got = qm.decode_output(keys.decrypt_ring(ring).reshape(3, -1))
        assert np.array_equal(got, _oracle(qm, q))
        rows = sess.download_packed(qm.output_compaction().tier)
        assert np.array_equal(qm.decrypt_result(ring), got) and np.array_equal(qm.decrypt_result(ring.to_bytes()), got)
        assert np.array_equal(qm.decrypt_result(full), got) and np.array_equal(qm.decrypt_result(rows), got)
    finally:
        qm.close()


def test_session_download_ring_default_catalogue():
    from dctfhe import params as P
    qm, calib = _tiny(P.default_params())
    try:
        qm.fhe_circuit.keygen(seed=4)
        keys = qm._keys
        blob = qm.fhe_circuit.export_result_packing_key()
        assert blob.size == 72 + 8 * 800 * 2048
        qm.fhe_circuit.load_result_packing_key(blob)
        q = qm.quantize_input(calib[:1])
        oc = qm.output_compaction("ring")
        assert (oc.name, oc.n, oc.spec.logN) == ("T6", 800, 11)
        sess = qm._session("execute", 1)
        in_dim, _ = sess.dims()
        sess.upload(keys.encrypt(qm.encode_input(q).reshape(-1), in_dim), in_dim)
        sess.run()
        ring = sess.download_ring(oc.tier, qm._pack_key)
        assert ring.words.size == 2048 + qm._circuit.n_out
        assert np.array_equal(qm.decode_output(keys.decrypt_ring(ring).reshape(1, -1)), _oracle(qm, q))
    finally:
        qm.close()


# ------------------------------------------------------------------------------------------ 6. facade, client / server split
def test_facade_and_split_with_all_three_switches():
    from dctfhe import params as P
    from dctfhe.engine import PackedRing
    from dctfhe.quantized_module import Configuration, QuantizedModule
    cfg = Configuration(compress_input_ciphertexts=True, compress_evaluation_keys=True, compress_output_ciphertexts="ring",
                        result_packing_spec=P.test_pack_spec())
    client, calib = _tiny(P.test_params(), cfg)
    server = QuantizedModule(client.compiled, configuration=cfg)         # key-less: both keys arrive as blobs
    try:
        client.fhe_circuit.keygen(seed=8)
        B = 3
        q = client.quantize_input(calib[:B])
        want = _oracle(client, q)
        n_out = client.compiled.n_out()
        sc = client._keys.encrypt_seeded(client.encode_input(q).reshape(-1))
        server.fhe_circuit.load_evaluation_keys(client.fhe_circuit.export_evaluation_keys())
        with pytest.raises(RuntimeError, match="packing key"):           # "ring" without the packing key
            server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B)
        with pytest.raises(RuntimeError, match="packing key"):
            client.forward_quantized(q, "execute")
        pk_blob = client.fhe_circuit.export_result_packing_key()
        server.fhe_circuit.load_result_packing_key(pk_blob)
        out = server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B)
        assert isinstance(out, PackedRing) and len(out) == B * n_out and out.nbytes == 20 + 2 * (256 + B * n_out)
        assert np.array_equal(client.decrypt_result(out.to_bytes()), want)
        # packed="rows" / False override the configuration
        rows = server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B, packed="rows")
        assert np.array_equal(client.decrypt_result(rows.to_bytes()), want)
        full = server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B, packed=False)
        assert full.shape == (B * n_out, client._keys.D + 1) and np.array_equal(client.decrypt_result(full), want)
        with pytest.raises(RuntimeError, match="client key"):
            server.decrypt_result(out)
        with pytest.raises(RuntimeError, match="made by the client"):
            server.fhe_circuit.export_result_packing_key()
        # a key noisier than the priced spec is refused; so is a packing key imported on another context
        server.fhe_circuit.load_result_packing_key(client._keys.export_pack_key(P.PackSpec(logN=8, l=1, beta=16, sigma=2.0 ** -40)))
        with pytest.raises(RuntimeError, match="noisier"):
            server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), B)
        server.fhe_circuit.load_result_packing_key(pk_blob)
        # the client alone, through the switches, with its own key loaded back
        client.fhe_circuit.load_result_packing_key(pk_blob)
        assert np.array_equal(client.forward_quantized(q, "execute"), want)
        assert client.last_io["output_bytes"] == 2 * (256 + B * n_out)
    finally:
        server.close()
        client.close()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(gpu_ctx, keysets, packkeys):
    from dctfhe import compile as cc, models
    from dctfhe._lib import DctfheError
    from dctfhe.engine import Circuit, PackKey, Session, device_bytes_live
    ps, keys = keysets("test")
    spec, blob, pk, _ = packkeys("test", 8, 1, 16)
    L, n_max = gpu_ctx.L, ps.n_max
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    compiled = cc.compile_model(models.tiny_resnet_q(), np.random.default_rng(0).normal(0, 1, (16, 4, 6, 6)), param_set=ps)
    circ = Circuit(gpu_ctx, compiled.blob)
    clear, sess = Session(gpu_ctx, circ, None, 1), Session(gpu_ctx, circ, keys, 1)
    live = device_bytes_live()

    def fails(rc, needle):
        assert rc != 0
        msg = L.dctfhe_last_error().decode()
        assert needle in msg, msg
        assert device_bytes_live() == live, msg
    try:
        size, buf = C.c_size_t(), np.zeros(1 << 20, np.uint8)
        fails(L.dctfhe_pack_key_export(keys.client.h, 11, 1, 16, 2.0 ** -48, None, 0, C.byref(size)), "N_p = 2048 > D = 1024")
        fails(L.dctfhe_pack_key_export(keys.client.h, 8, 4, 16, 2.0 ** -48, None, 0, C.byref(size)), "exceeds 63")
        fails(L.dctfhe_pack_key_export(keys.client.h, 8, 1, 33, 2.0 ** -48, None, 0, C.byref(size)), "bits")
        fails(L.dctfhe_pack_key_export(keys.client.h, 4, 1, 16, 2.0 ** -48, None, 0, C.byref(size)), "outside")
        fails(L.dctfhe_pack_key_export(keys.client.h, 8, 1, 16, 2.0 ** -48, p(buf), 100, C.byref(size)), "needed")
        fails(L.dctfhe_pack_key_export(None, 8, 1, 16, 2.0 ** -48, None, 0, C.byref(size)), "null")
        # a blob of the wrong magic, version or length
        h = C.c_void_p()
        for bad, needle in [(b"XRPK" + blob.tobytes()[4:], "magic"), (blob.tobytes()[:4] + b"\x02" + blob.tobytes()[5:], "version"),
                            (blob.tobytes()[:-8], "length"), (blob.tobytes() + bytes(8), "length"), (blob.tobytes()[:40], "too short")]:
            arr = np.frombuffer(bad, np.uint8)
            fails(L.dctfhe_pack_key_import(gpu_ctx.h, p(arr), arr.size, C.byref(h)), needle)
            with pytest.raises(DctfheError, match=needle):
                PackKey(gpu_ctx, bad)
        fails(L.dctfhe_pack_key_import(gpu_ctx.h, None, 0, C.byref(h)), "null")
        # the primitive: n beyond the key's n_max, n = 0
        out = np.zeros(1024, np.uint16)
        small = np.zeros((2, n_max + 2), U)
        fails(L.dctfhe_ring_pack(gpu_ctx.h, pk.h, p(small), 2, n_max + 1, p(out)), "n_max = %d" % n_max)
        fails(L.dctfhe_ring_pack(gpu_ctx.h, pk.h, p(small), 2, 0, p(out)), "n_max")
        fails(L.dctfhe_ring_pack(gpu_ctx.h, None, p(small), 2, n_max, p(out)), "null")
        fails(L.dctfhe_ring_pack(gpu_ctx.h, pk.h, None, 2, n_max, p(out)), "null")
        # sessions
        fails(L.dctfhe_session_download_ring(clear.h, 0, pk.h, p(out)), "clear-mode")
        fails(L.dctfhe_session_download_ring(sess.h, len(ps.tiers), pk.h, p(out)), "out of range")
        fails(L.dctfhe_session_download_ring(sess.h, 0, None, p(out)), "null")
        from dctfhe.engine import Context
        ctx2 = Context(0)
        try:
            pk2 = PackKey(ctx2, blob)
            held = device_bytes_live()
            assert L.dctfhe_session_download_ring(sess.h, 0, pk2.h, p(out)) != 0 and "share one context" in L.dctfhe_last_error().decode()
            assert L.dctfhe_ring_pack(gpu_ctx.h, pk2.h, p(small), 2, n_max, p(out)) != 0 and "another context" in L.dctfhe_last_error().decode()
            assert device_bytes_live() == held
            pk2.close()
        finally:
            ctx2.close()
        assert device_bytes_live() == live
        # the client
        ph = np.zeros(2, U)
        fails(L.dctfhe_decrypt_ring(gpu_ctx.h, keys.client.h, 11, p(out), 2, p(ph)), "N_p = 2048 > D = 1024")
        fails(L.dctfhe_decrypt_ring(gpu_ctx.h, keys.client.h, 8, None, 2, p(ph)), "null")
        with pytest.raises(DctfheError, match="clear-mode"):
            clear.download_ring(0, pk)
        # the handles still work after all that
        ok = pk.ring_pack(np.zeros((1, n_max + 1), U))
        assert not ok.words.any() and keys.decrypt_ring(ok).tolist() == [0]
        assert device_bytes_live() == live
    finally:
        sess.close()
        clear.close()
        circ.close()
