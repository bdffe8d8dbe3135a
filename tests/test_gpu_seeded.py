"""Seeded input ciphertexts and compressed evaluation keys on the GPU (include/dctfhe.h dctfhe_encrypt_seeded, dctfhe_session_upload_seeded,
dctfhe_eval_keys_export_compressed): seeded encryption expands to exactly what dctfhe_encrypt_rows draws, a session fed seeded inputs
holds what upload_rows would store, compressed keys import to the same key-switch keys and to bootstrap keys of the same phases, and the
QuantizedModule switches (Configuration(compress_input_ciphertexts=True, compress_evaluation_keys=True)) evaluate to the integer circuit."""
import ctypes as C

import numpy as np
import pytest

from test_seeded_host import expand_blockwise

pytestmark = pytest.mark.gpu

NONCE = bytes(range(40, 56))


def _params(name):
    from dctfhe import params as P
    return P.to_c_params(P.test_params() if name == "test" else P.default_params())


def _oracle(qm, q):
    from oracle import circuit_ref
    out, ov = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not ov
    return qm.decode_output(out)


def _pair(ctx, cp, counter):
    """two handles of one seed with the same fixed nonce, both at `counter`: they draw the same masks and noise"""
    from dctfhe.engine import ClientKey
    a, b = ClientKey(ctx, cp, 9), ClientKey(ctx, cp, 9)
    for h in (a, b):
        h.set_encrypt_nonce(NONCE)
        h.set_encrypt_counter(counter)
    return a, b


# ------------------------------------------------------------------------------------------ 1. seeded encryption
@pytest.mark.parametrize("pname", ["test", "default"])
def test_seeded_encryption_expands_to_encrypt_rows(gpu_ctx, pname):
    cp = _params(pname)
    a, b = _pair(gpu_ctx, cp, 3)
    try:
        dim = a.input_dim
        for count in (1, 7, 1000, 100_003):
            ph = np.arange(count, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
            sc = a.encrypt_seeded(ph)
            want = b.encrypt(ph, dim)
            assert sc.D == cp.D and sc.input_dim == dim and len(sc) == count
            got = gpu_ctx.expand_seeded(sc)
            assert np.array_equal(got, want), count
            if count == 7:         # the device expander == its host twin, and a wider row puts zeros past input_dim
                assert np.array_equal(got, expand_blockwise(gpu_ctx.L, sc.key, sc.stream, cp.D + 1, dim, sc.bodies, dim))
                wide = gpu_ctx.expand_seeded(sc, cp.D)
                assert np.array_equal(wide[:, :dim], got[:, :dim]) and not wide[:, dim:cp.D].any() and np.array_equal(wide[:, -1], got[:, -1])
            err = (a.decrypt(got, dim) - ph).view(np.int64)
            assert np.abs(err).max() < 2 ** 52, count         # phases back up to the encryption noise
            del got, want
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 2. + 3. sessions
@pytest.fixture(scope="module")
def tiny():
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params())
    yield qm, calib[:3]
    qm.close()


@pytest.fixture(scope="module")
def r20():
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from dctfhe.synthetic import synthetic_dct_batch
    qm = compile_brevitas_qat_model(models.ResNet20QAT(bit_width=4, in_channels=24, img_size=16), synthetic_dct_batch(100, seed=7), n_bits=5,
                                    rounding_threshold_bits=6, p_error=0.01)
    yield qm, synthetic_dct_batch(1, seed=42)
    qm.close()


@pytest.mark.parametrize("which", ["tiny", "r20"])
def test_upload_seeded_equals_upload_rows(which, request):
    qm, x = request.getfixturevalue(which)
    qm.fhe_circuit.keygen(seed=4, force=True)
    keys = qm._keys
    keys.client.set_encrypt_nonce(NONCE)
    q = qm.quantize_input(x)
    phases = qm.encode_input(q).reshape(-1)
    sess = qm._session("execute", q.shape[0])
    in_dim, out_dim = sess.dims()
    keys.client.set_encrypt_counter(11)
    sc = keys.client.encrypt_seeded(phases)
    sess.upload_seeded(sc)
    sess.run()
    got = sess.download(out_dim)
    keys.client.set_encrypt_counter(11)
    sess.upload(keys.client.encrypt(phases, in_dim), in_dim)
    sess.run()
    want = sess.download(out_dim)
    assert np.array_equal(got, want)
    dec = qm.decode_output(keys.client.decrypt(got.reshape(-1, out_dim + 1), out_dim).reshape(q.shape[0], -1))
    assert np.array_equal(dec, _oracle(qm, q))


def test_upload_seeded_refusals(tiny):
    from dctfhe._lib import DctfheError
    from dctfhe.engine import SeededCiphertexts
    qm, x = tiny
    qm.fhe_circuit.keygen(seed=4)
    q = qm.quantize_input(x)
    phases = qm.encode_input(q).reshape(-1)
    sess = qm._session("execute", q.shape[0])
    in_dim = sess.dims()[0]
    sc = qm._keys.client.encrypt_seeded(phases)
    with pytest.raises(DctfheError, match="clear-mode"):
        qm._session("clear", q.shape[0]).upload_seeded(sc)
    with pytest.raises(DctfheError, match="batch x n_in"):
        sess.upload_seeded(SeededCiphertexts(sc.key, sc.stream, sc.D, sc.input_dim, sc.bodies[:-1]))
    wide = SeededCiphertexts(sc.key, sc.stream, sc.D, sc.input_dim, sc.bodies)
    wide.input_dim = in_dim + 1                     # past the input's effective dimension (here also past D: the C check is the one tested)
    with pytest.raises(DctfheError, match="mask words per input"):
        sess.upload_seeded(wide)
    L = qm._ctx.L
    b = sc.bodies.ctypes.data_as(C.c_void_p)
    assert L.dctfhe_session_upload_seeded(None, sc.key, 0, in_dim, b, len(sc)) != 0
    assert L.dctfhe_session_upload_seeded(sess.h, None, 0, in_dim, b, len(sc)) != 0
    assert L.dctfhe_session_upload_seeded(sess.h, sc.key, 0, in_dim, None, len(sc)) != 0
    assert L.dctfhe_encrypt_seeded(qm._ctx.h, qm._keys.client.h, b, len(sc), None, None, b) != 0
    assert L.dctfhe_expand_seeded(qm._ctx.h, sc.key, 0, sc.D, sc.D + 1, b, 1, sc.D, b) != 0          # dim_eff > D


# ------------------------------------------------------------------------------------------ 4. compressed keys
def _negacyclic_phase(rows, S, k, N):
    """body - sum_j a_j * S_j (mod X^N + 1) of GLWE rows [R][k+1][N] under the binary key S [k*N] (numpy, u64 wrap)"""
    ph = rows[:, k, :].copy()
    for j in range(k):
        a = rows[:, j, :]
        for m in np.flatnonzero(S[j * N:(j + 1) * N]):
            ph[:, m:] -= a[:, :N - m]
            ph[:, :m] += a[:, N - m:]          # X^N = -1
    return ph


@pytest.mark.parametrize("pname", ["test", "default"])
def test_compressed_keys(gpu_ctx, pname):
    from dctfhe.engine import ClientKey, EvalKeys, blob_params
    cp = _params(pname)
    client = ClientKey(gpu_ctx, cp, 21)
    full = client.generate_eval_keys()
    blob = client.export_eval_keys_compressed()
    imported = EvalKeys.from_blob(gpu_ctx, blob)
    try:
        # size: header + params, pub, own key-switch bodies, standard-domain bootstrap bodies
        want = 16 + C.sizeof(type(cp)) + 32
        for ti in range(cp.n_tiers):
            t = cp.tiers[ti]
            blocks = 3 * t.n // 2 if t.unroll == 2 else t.n
            want += (cp.D * t.lk * 8 if t.ksk_share < 0 else 0) + blocks * (t.k + 1) * t.l * (1 << t.logN) * 8
        assert blob.size == want
        n_full = C.c_size_t()
        assert gpu_ctx.L.dctfhe_eval_keys_export(full.h, None, 0, C.byref(n_full)) == 0
        if pname == "default":
            assert blob.size <= 0.27 * n_full.value, (blob.size, n_full.value)
        assert bytes(blob_params(blob)) == bytes(cp)
        S, _ = client.export_secret()
        rng = np.random.default_rng(1)
        for ti in range(cp.n_tiers):
            t = cp.tiers[ti]
            if t.ksk_share < 0:
                assert np.array_equal(imported.export_ksk(ti), full.export_ksk(ti)), ti
            N, k, l = 1 << t.logN, t.k, t.l
            dec = gpu_ctx.decompress_bsk(blob, ti)
            std = client.export_bsk(ti)
            p_is_k = np.arange((k + 1) * l) // l == k
            assert np.array_equal(dec[:, p_is_k], std[:, p_is_k]), ti              # gadget term in the body: bit for bit
            blocks = dec.shape[0]
            sel = np.arange(blocks) if pname == "test" else rng.choice(blocks, 2, replace=False)
            d = dec[sel][:, ~p_is_k].reshape(-1, k + 1, N)
            s = std[sel][:, ~p_is_k].reshape(-1, k + 1, N)
            assert np.array_equal(_negacyclic_phase(d, S, k, N), _negacyclic_phase(s, S, k, N)), ti     # body form: same phase
            del dec, std
    finally:
        imported.close()
        full.close()
        client.close()


# ------------------------------------------------------------------------------------------ 5. client / server modules
@pytest.mark.parametrize("which", ["tiny", "r20"])
def test_server_module_on_compressed_keys_and_seeded_inputs(which, request):
    from dctfhe.quantized_module import Configuration, QuantizedModule
    qm0, x = request.getfixturevalue(which)
    cfg = Configuration(compress_input_ciphertexts=True, compress_evaluation_keys=True)
    client = QuantizedModule(qm0.compiled, configuration=cfg)
    server = QuantizedModule(qm0.compiled)
    try:
        client.fhe_circuit.keygen(seed=8)
        q = client.quantize_input(x)
        want = _oracle(client, q)
        # the client alone, through the switches
        assert np.array_equal(client.forward_quantized(q, "execute"), want)
        assert client.last_io["upload_bytes"] == 8 * q.shape[0] * client._circuit.n_in
        # client -> server: compressed keys (the default under this configuration), seeded inputs as bytes
        blob = client.fhe_circuit.export_evaluation_keys()
        assert blob[:4].tobytes() == b"DEVC"
        server.fhe_circuit.load_evaluation_keys(blob)
        sc = client._keys.encrypt_seeded(client.encode_input(q).reshape(-1))
        out = server.fhe_circuit.evaluate_encrypted(sc.to_bytes(), q.shape[0])
        got = client.decode_output(client._keys.decrypt(out).reshape(q.shape[0], -1))
        assert np.array_equal(got, want)
        assert client.export_evaluation_keys(compressed=False)[:4].tobytes() == b"DEVK"
    finally:
        server.close()
        client.close()
