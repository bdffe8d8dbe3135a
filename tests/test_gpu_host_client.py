"""The host client library against the GPU engine (include/dctfhe_client.h): with equal seed, nonce and counter the host and the device
write the same masks, the same generator keys, streams, headers and lengths, and noise terms within one unit of 2^-64 (a key-switch
body within one step of its grid); what the device encrypts or packs the host decrypts word for word; a host client, a device server and
a host data owner run the tiny trunk of smoke() to the outputs of the integer circuit.  Tiny parameters: test_params() and the custom set
of tests/host_client_ref.py, at most 64 ciphertexts."""
import ctypes as C

import numpy as np
import pytest

import host_client_ref as H
import key_material_ref as K

pytestmark = pytest.mark.gpu

U = np.uint64
COUNT = 61


def _sets():
    from dctfhe import params as P
    return {"test_params": P.to_c_params(P.test_params()), "custom": H.custom_params()}


@pytest.fixture(scope="module", params=["test_params", "custom"])
def pair(request, gpu_ctx):
    """(parameters, host key, device key) of one seed, nonce fixed on both"""
    from dctfhe.engine import ClientKey
    from dctfhe.host_client import HostClientKey
    cp = _sets()[request.param]
    host, dev = HostClientKey(cp, seed=17), ClientKey(gpu_ctx, cp, seed=17)
    host.set_encrypt_nonce(H.NONCE)
    dev.set_encrypt_nonce(H.NONCE)
    yield cp, host, dev
    host.close()
    dev.close()


def _step(a, b):
    """largest wrapping |a - b| over two word arrays"""
    return int(np.abs((np.asarray(a, U) - np.asarray(b, U)).view(np.int64)).max(initial=0))


# ------------------------------------------------------------------------------------------ 1. encryption
def test_same_secret_and_generator_keys(pair):
    cp, host, dev = pair
    for a, b in zip(host.export_secret(), dev.export_secret()):
        assert np.array_equal(a, b)


def test_encryptions_share_masks_and_bodies_within_one_unit(pair):
    cp, host, dev = pair
    ph = np.random.default_rng(2).integers(0, 2 ** 64, COUNT, dtype=U)
    for dim in (host.input_dim, cp.D):
        for k in (host, dev):
            k.set_encrypt_counter(3)
        a, b = host.encrypt(ph, dim), dev.encrypt(ph, dim)
        assert a.shape == b.shape == (COUNT, dim + 1)
        assert np.array_equal(a[:, :dim], b[:, :dim]), "masks differ"
        step = _step(a[:, dim], b[:, dim])
        print("encrypt dim %d: largest |host - device| body %d, %d of %d differ" % (dim, step, int((a[:, dim] != b[:, dim]).sum()), COUNT))
        assert step <= 1
    for k in (host, dev):
        k.set_encrypt_counter(3)
    sa, sb = host.encrypt_seeded(ph), dev.encrypt_seeded(ph)
    assert sa.key == sb.key and sa.stream == sb.stream and (sa.D, sa.input_dim) == (sb.D, sb.input_dim)
    assert _step(sa.bodies, sb.bodies) <= 1
    assert np.array_equal(sa.bodies, a[:, cp.D]), "the host's seeded bodies are not its rows' bodies"
    # the noise itself differs from zero: the comparison is of noisy bodies, not of noise-free ones
    assert (host.decrypt(a) != ph).any()


# ------------------------------------------------------------------------------------------ 2. decryption
def test_host_decrypts_what_the_device_made_word_for_word(pair, gpu_ctx):
    """rows at dim = input_dim and dim = D under both parameter sets; packed rows of every tier and a ring-packed group under
    test_params(), whose key-switch shapes are the ones the device's own tests and smoke() run (the custom set's small keys of 6 and 8
    bits are key-material cases: the device key switch is not held to such widths anywhere, and this file is not the place to start)"""
    from dctfhe.engine import PackKey
    from dctfhe import params as P
    cp, host, dev = pair
    ph = np.random.default_rng(4).integers(0, 2 ** 64, COUNT, dtype=U)
    for dim in (host.input_dim, cp.D):
        rows = dev.encrypt(ph, dim)
        assert np.array_equal(host.decrypt(rows, dim), dev.decrypt(rows, dim))
    if cp.D != P.test_params().D:
        return
    ek = dev.generate_eval_keys()
    pk = None
    try:
        full = dev.encrypt(ph, cp.D)
        for tier in range(cp.n_tiers):
            packed = ek.keyswitch_pack(tier, full, cp.D)
            assert packed.n == cp.tiers[tier].n and len(packed) == COUNT
            assert np.array_equal(host.decrypt_packed(packed), dev.decrypt_packed(packed))
        spec = P.test_pack_spec()                              # rings of 256: 61 results are one partial group
        pk = PackKey(gpu_ctx, dev.export_pack_key(spec))
        ring = pk.ring_pack(ek.keyswitch(0, full))
        assert len(ring) == COUNT and ring.words.size == spec.N + COUNT
        got = host.decrypt_ring(ring)
        assert np.array_equal(got, dev.decrypt_ring(ring))
        # ... and they are the phases that went in, to the packing noise and the 16-bit rounding
        err = (got - ph).view(np.int64).astype(np.float64) / 2.0 ** 64
        assert np.abs(err).max() < 2.0 ** -10, np.abs(err).max()
    finally:
        if pk is not None:
            pk.close()
        ek.close()


# ------------------------------------------------------------------------------------------ 3. compressed keys
def test_compressed_blobs_agree_up_to_the_gaussian_unit(pair):
    cp, host, dev = pair
    a, b = host.export_eval_keys_compressed(), dev.export_eval_keys_compressed()
    assert a.size == b.size
    ha, pa, ta = H.parse_cblob(a, cp)
    hb, pb, tb = H.parse_cblob(b, cp)
    assert ha == hb and pa == pb, "header, parameters or mask key differ"
    H.check_header(a, cp, pa)
    for ti in range(cp.n_tiers):
        t = cp.tiers[ti]
        (ka, ba), (kb, bb) = ta[ti], tb[ti]
        assert (ka is None) == (kb is None) == (t.ksk_share >= 0)
        if ka is not None:
            grid = 1 << (64 - 8 * K.ks_limbs(t.lk, t.betak))
            step = _step(ka, kb)
            print("tier %d key-switch bodies: largest |host - device| %d grid steps, %d of %d differ" % (ti, step // grid, int((ka != kb).sum()), ka.size))
            assert step <= grid and not (ka & U(grid - 1)).any()
        step = _step(ba, bb)
        print("tier %d bootstrap bodies: largest |host - device| %d, %d of %d differ" % (ti, step, int((ba != bb).sum()), ba.size))
        assert step <= 1
    # the packing key and the public key, the same way
    from dctfhe import params as P
    for x, y, hdr in ((host.export_pack_key(P.test_pack_spec()), dev.export_pack_key(P.test_pack_spec()), 72),
                      (host.export_public_key(P.test_public_input_spec()), dev.export_public_key(P.test_public_input_spec()), 64)):
        assert x.size == y.size and np.array_equal(x[:hdr], y[:hdr])
        assert _step(np.frombuffer(x, U, offset=hdr), np.frombuffer(y, U, offset=hdr)) <= 1


# ------------------------------------------------------------------------------------------ 4 / 5. three roles
@pytest.fixture(scope="module")
def roles3(tmp_path_factory):
    """the tiny trunk of smoke() saved as a deployment; a host client with its keys, a device server that loaded them"""
    from dctfhe import deploy, models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    from oracle import circuit_ref
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params(),
                                    configuration=Configuration(public_input_spec=P.test_public_input_spec(), result_packing_spec=P.test_pack_spec()))
    cpath, spath = deploy.save(qm, str(tmp_path_factory.mktemp("host_roles_gpu")))
    qm.close()
    client, server = deploy.Client(cpath, device="host"), deploy.Server(spath, device=0)
    client.keygen(seed=3)
    server.load_evaluation_keys(client.export_evaluation_keys(compressed=True))
    server.load_result_packing_key(client.export_result_packing_key())
    x = calib[:2]
    ref, overflow = circuit_ref.run_clear(server.spec.blob, deploy.roles.encode_input(client.spec, client.quantize(x)))
    assert not overflow
    want = deploy.roles.decode_output(client.spec, ref)
    yield dict(client=client, server=server, cpath=cpath, x=x, want=want)
    server.close()
    client.close()


def test_key_check_made_and_verified_on_the_host_answered_on_the_device(roles3):
    from dctfhe import deploy
    client, server = roles3["client"], roles3["server"]
    assert client._ctx is None
    check = client.make_key_check()
    answer = server.answer_key_check(check)
    client.verify_key_check(answer)
    other = deploy.Client(roles3["cpath"], device="host")
    try:
        other.keygen(seed=4)
        with pytest.raises(deploy.KeyCheckError, match=r"key check failed on tier \d+"):
            other.verify_key_check(answer)
    finally:
        other.close()


@pytest.mark.parametrize("form,packed", [("seeded", None), ("rows", "rows"), ("seeded", "ring")])
def test_host_client_device_server_outputs_equal_the_integer_circuit(roles3, form, packed):
    client, server = roles3["client"], roles3["server"]
    response = server.evaluate(client.encrypt(roles3["x"], form=form), packed=packed)
    got = client.decrypt(response)
    assert client._ctx is None
    assert np.array_equal(got, roles3["want"]), (got, roles3["want"])


def test_host_data_owner_inputs_and_draws(roles3, gpu_ctx):
    from dctfhe import deploy
    from dctfhe.engine import PublicKey
    client, server, x = roles3["client"], roles3["server"], roles3["x"]
    blob = client.export_public_key()
    owner = deploy.DataOwner(roles3["cpath"], device="host")
    dev_pk = PublicKey(gpu_ctx, blob)
    try:
        owner.load_public_key(blob)
        request = owner.encrypt(x)
        assert owner._ctx is None
        got = client.decrypt(server.evaluate(request))          # Server.evaluate uploads a DPIN payload with Session.upload_public
        assert np.array_equal(got, roles3["want"]), (got, roles3["want"])
        seed = bytes(range(60, 92))
        host_pk = owner._public_key
        host_pk.set_encrypt_seed(seed)
        dev_pk.set_encrypt_seed(seed)
        count = 64
        ph = np.random.default_rng(6).integers(0, 2 ** 64, count, dtype=U)
        (u_h, e1_h, e2_h), (u_d, e1_d, e2_d) = host_pk.draws(0, count), dev_pk.draws(0, count)
        assert np.array_equal(u_h, u_d), "the u draws differ"
        assert _step(e1_h.view(U), e1_d.view(U)) <= 1 and _step(e2_h.view(U), e2_d.view(U)) <= 1
        a, b = host_pk.encrypt(ph), dev_pk.encrypt(ph)
        assert a.logN == b.logN and len(a) == len(b) == count and a.words.size == b.words.size
        # A u + e1 and B u + e2 + phase with equal u: the words differ by the noise terms' unit alone
        assert _step(a.words, b.words) <= 1
    finally:
        dev_pk.close()
        owner.close()
