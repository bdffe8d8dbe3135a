"""Evaluation keys sized to the circuit, on the GPU (include/dctfhe.h TIER SELECTIONS): the kept keys of a pruned
set are word for word those of the full set from the same seed, pruned blobs of both forms are the kept sections of the unpruned ones and
import again, a circuit under pruned keys produces the output ciphertext words of the run under full keys, every call that needs an absent
key is refused by name before it touches device memory, the dropped Fourier keys are really not resident, the roles run from a pruned
bundle with a client on the host, and the two-bit tiers bootstrap when kept and are refused when dropped.

Catalogues (tests/key_tiers_cases.py): A = q, t, b, u on test_params()'s shapes -- the tiny trunk reads bsk {t, b} and ksk {q, b}: a dropped
bootstrap key whose key-switch key stays (q), a dropped tier in front (q) and at the end (u).  B = the two unroll-2 shapes, each twice.

On the compressed round trip: a compressed blob ships the bootstrap-key rows whose gadget term sits in a mask polynomial (p < k) in BODY FORM
-- the same phase and noise draw, another ciphertext (include/dctfhe.h dctfhe_eval_keys_export_compressed) -- so the Fourier key an import
rebuilds from it never equalled the generated one in those rows, pruned or not.  What is exact, and asserted: the import of the pruned
compressed blob equals, section for section, the import of the unpruned compressed blob; its key-switch keys and its rows p = k equal the
generated handle's word for word; and a full-form blob imports and exports as the identity."""
import os
import subprocess
import sys

import numpy as np
import pytest

import key_tiers_cases as KT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "deploy_worker.py")
LIMIT_S = 120
U = np.uint64


def _all(ps):
    return (1 << len(ps.tiers)) - 1, sum(1 << i for i, t in enumerate(ps.tiers) if t.ksk_share < 0)


@pytest.fixture(scope="module")
def A(gpu_ctx):
    """catalogue A: the compiled tiny trunk, its selection, one client key, the full and the pruned handle and their four blobs"""
    from dctfhe import params as P
    from dctfhe.engine import Circuit, ClientKey
    ps = KT.catalogue_a()
    c, calib = KT.tiny_circuit(ps)
    sel = c.key_tiers()
    assert (sel.bsk_mask, sel.ksk_mask) == (0b0110, 0b0101)
    cp = P.to_c_params(ps)
    client = ClientKey(gpu_ctx, cp, seed=5)
    full, pruned = client.generate_eval_keys(), client.generate_eval_keys(sel)
    circuit = Circuit(gpu_ctx, c.blob)
    a = dict(ps=ps, cp=cp, c=c, calib=calib, sel=sel, client=client, full=full, pruned=pruned, circuit=circuit, full_blob=full.to_blob(),
             pruned_blob=pruned.to_blob(), cfull=client.export_eval_keys_compressed(), cpruned=client.export_eval_keys_compressed(sel))
    yield a
    for h in (circuit, pruned, full, client):
        h.close()


def _refused(fn, *needles):
    """fn raises, its message holds every needle, and the library's live device bytes are what they were"""
    from dctfhe._lib import DctfheError
    from dctfhe.engine import device_bytes_live
    live = device_bytes_live()
    with pytest.raises(DctfheError) as e:
        fn()
    for n in needles:
        assert n in str(e.value), (n, str(e.value))
    assert device_bytes_live() == live, "a refused call changed the device memory the library holds"


# ------------------------------------------------------------------------------------------ 1. key material
def test_kept_keys_are_the_full_sets_word_for_word(A):
    from dctfhe._lib import KeyTiers
    ps, sel, full, pruned = A["ps"], A["sel"], A["full"], A["pruned"]
    assert pruned.tiers == KeyTiers(sel.bsk_mask, sel.ksk_mask) and full.tiers == KeyTiers(*_all(ps))
    for ti, t in enumerate(ps.tiers):
        if (sel.ksk_mask >> ti) & 1:
            assert np.array_equal(pruned.export_ksk(ti), full.export_ksk(ti)), ("key-switch key", t.name)
    # a sharing tier reads its owner's key through either handle
    assert np.array_equal(pruned.export_ksk(1), full.export_ksk(0))
    # every kept Fourier key (and key-switch key) as the full-form export holds it, and the layout rule: version 4, masks, kept sections
    assert A["full_blob"].size == KT.blob_bytes(ps, *_all(ps), False)
    assert A["pruned_blob"].size == KT.blob_bytes(ps, sel.bsk_mask, sel.ksk_mask, False)
    assert np.array_equal(A["pruned_blob"], KT.pruned_from_full(A["full_blob"], ps, sel.bsk_mask, sel.ksk_mask, False))
    assert np.array_equal(A["cpruned"], KT.pruned_from_full(A["cfull"], ps, sel.bsk_mask, sel.ksk_mask, True))
    # everything selected: the calls of before, byte for byte
    again = A["client"].generate_eval_keys(_all(ps))
    try:
        assert np.array_equal(again.to_blob(), A["full_blob"])
    finally:
        again.close()
    assert np.array_equal(A["client"].export_eval_keys_compressed(_all(ps)), A["cfull"])


def test_host_and_gpu_pruned_exports_agree_as_the_full_ones_do(A):
    """the host library's noise draw may differ from the device's by one unit of 2^-64 (include/dctfhe_client.h; tests/test_gpu_host_client.py
    bounds it on the full blobs): the pruned blobs have header, public key and masks byte for byte in common, and differ word for word
    exactly as the full ones do in the kept sections"""
    from dctfhe.host_client import HostClientKey
    ps, sel = A["ps"], A["sel"]
    hk = HostClientKey(A["cp"], seed=5)
    try:
        hp, hf = hk.export_eval_keys_compressed(sel), hk.export_eval_keys_compressed()
    finally:
        hk.close()
    head = KT.HEADER + KT.params_bytes() + 32 + 8
    assert hp.size == A["cpruned"].size and np.array_equal(hp[:head], A["cpruned"][:head])
    d = (hp[head:].view(U) - A["cpruned"][head:].view(U)).view(np.int64)
    df = (hf[head - 8:].view(U) - A["cfull"][head - 8:].view(U)).view(np.int64)
    assert np.array_equal(d, KT.slice_sections(np.concatenate([hf[:head - 8], df.view(np.uint8)]), ps, sel.bsk_mask, sel.ksk_mask, True).view(np.int64))


# ------------------------------------------------------------------------------------------ 2. round trips
def _fourier_rows_p_eq_k(blob, ps, bsk, ksk, ti):
    """the polynomials of the rows p = k of tier ti's Fourier key in a full-form blob under (bsk, ksk): [blocks, l, k + 1, N] doubles"""
    pruned = (bsk, ksk) != _all(ps)
    at = KT.HEADER + KT.params_bytes() + (8 if pruned else 0)
    for i, (kb, bb) in enumerate(KT.sections(ps, False)):
        at += kb * ((ksk >> i) & 1)
        if i == ti:
            t = ps.tiers[ti]
            sec = np.asarray(blob[at:at + bb]).view(np.float64).reshape(KT.blocks(t), t.k + 1, t.l, t.k + 1, t.N)
            return sec[:, t.k]
        at += bb * ((bsk >> i) & 1)


def test_pruned_blobs_import_and_export_again(A, gpu_ctx):
    from dctfhe._lib import KeyTiers
    from dctfhe.engine import EvalKeys
    ps, sel = A["ps"], A["sel"]
    b, k = sel.bsk_mask, sel.ksk_mask
    # full form: the identity
    again = EvalKeys.from_blob(gpu_ctx, A["pruned_blob"])
    try:
        assert again.tiers == KeyTiers(b, k)
        assert np.array_equal(again.to_blob(), A["pruned_blob"])
    finally:
        again.close()
    # compressed form: the pruned import is the unpruned import, section for section (see the module docstring)
    ip, iff = EvalKeys.from_blob(gpu_ctx, A["cpruned"]), EvalKeys.from_blob(gpu_ctx, A["cfull"])
    try:
        assert ip.tiers == KeyTiers(b, k) and iff.tiers == KeyTiers(*_all(ps))
        got = ip.to_blob()
        assert np.array_equal(got, KT.pruned_from_full(iff.to_blob(), ps, b, k, False))
        # ... and against the directly generated pruned handle: key-switch keys and the rows p = k word for word
        for ti in range(len(ps.tiers)):
            if (k >> ti) & 1:
                assert np.array_equal(ip.export_ksk(ti), A["pruned"].export_ksk(ti)), ti
            if (b >> ti) & 1:
                assert np.array_equal(_fourier_rows_p_eq_k(got, ps, b, k, ti), _fourier_rows_p_eq_k(A["pruned_blob"], ps, b, k, ti)), ti
    finally:
        ip.close()
        iff.close()
    # the test view of a compressed blob honours the new offsets and refuses an absent tier
    for ti in (1, 2):
        assert np.array_equal(gpu_ctx.decompress_bsk(A["cpruned"], ti), gpu_ctx.decompress_bsk(A["cfull"], ti)), ti
    _refused(lambda: gpu_ctx.decompress_bsk(A["cpruned"], 0), "no bootstrap key of tier 0")
    _refused(lambda: gpu_ctx.decompress_bsk(A["cpruned"], 3), "no bootstrap key of tier 3")


def test_host_librarys_pruned_blob_imports_and_answers_the_key_check(A, tmp_path):
    from dctfhe import deploy
    qm = _module(A["ps"])
    deploy.save(qm, str(tmp_path), key_tiers="circuit")
    client, server = deploy.Client(str(tmp_path / deploy.CLIENT_FILE), device="host"), deploy.Server(str(tmp_path / deploy.SERVER_FILE))
    try:
        client.keygen(seed=5)
        blob = client.export_evaluation_keys()
        assert blob.size == A["cpruned"].size
        server.load_evaluation_keys(blob)
        check = client.make_key_check()
        client.verify_key_check(server.answer_key_check(check))
        # a check that asks for a tier the keys lack is refused by name
        full_client = deploy.Client(_saved_full(A["ps"], tmp_path), device="host")
        try:
            full_client.keygen(seed=5)
            with pytest.raises(ValueError, match=r"hold no bootstrap key of tier 0 \(q\)"):
                server.answer_key_check(full_client.make_key_check())
        finally:
            full_client.close()
    finally:
        server.close()
        client.close()


def _module(ps, **cfg):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    return compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=ps,
                                      configuration=Configuration(public_input_spec=P.test_public_input_spec(), result_packing_spec=P.test_pack_spec(), **cfg))


def _saved_full(ps, tmp_path):
    from dctfhe import deploy
    d = tmp_path / "full_bundle"
    if not d.exists():
        deploy.save(_module(ps), str(d))
    return str(d / deploy.CLIENT_FILE)


# ------------------------------------------------------------------------------------------ 3. determinism
def test_pruned_keys_produce_the_output_words_of_full_keys(A, gpu_ctx):
    from dctfhe import compile as cc, roles
    from dctfhe.engine import Session
    from oracle import circuit_ref
    c, client = A["c"], A["client"]
    q = roles.quantize_input(c, A["calib"][:2])
    phases = roles.encode_input(c, q)
    client.set_encrypt_nonce(bytes(range(16)))
    client.set_encrypt_counter(3)
    dim = client.input_dim
    cts = client.encrypt(phases.reshape(-1), dim)
    rows = {}
    packed = {}
    oc = cc.output_compaction(c).tier
    for name in ("full", "pruned"):
        sess = Session(gpu_ctx, A["circuit"], A[name], 2)
        try:
            sess.upload(cts, dim)
            sess.run()
            rows[name] = sess.download(sess.dims()[1])
            if (A["sel"].ksk_mask >> oc) & 1 or name == "full":
                packed[name] = sess.download_packed(oc).rows
        finally:
            sess.close()
    assert np.array_equal(rows["pruned"], rows["full"]), "the output ciphertext words depend on which unused keys are resident"
    if "pruned" in packed:
        assert np.array_equal(packed["pruned"], packed["full"])
    out_dim = rows["full"].shape[-1] - 1
    got = roles.decode_output(c, client.decrypt(rows["pruned"].reshape(-1, out_dim + 1), out_dim).reshape(2, -1))
    ref, overflow = circuit_ref.run_clear(c.blob, phases)
    assert not overflow and np.array_equal(got, roles.decode_output(c, ref))


# ------------------------------------------------------------------------------------------ 4. refusals
def test_calls_that_need_an_absent_key_are_refused_by_name(A, gpu_ctx):
    from dctfhe.engine import Session
    from dctfhe.deploy import key_check_table
    client, full, pruned, D = A["client"], A["full"], A["pruned"], A["ps"].D
    # session_create: keys that hold q's key-switch key and lack t's bootstrap key; keys that lack q's key-switch key
    no_t, no_q = client.generate_eval_keys((0b0100, 0b0001)), client.generate_eval_keys((0b0100, 0))
    try:
        assert (no_t.tiers.bsk, no_t.tiers.ksk) == (0b0100, 0b0101) and (no_q.tiers.bsk, no_q.tiers.ksk) == (0b0100, 0b0100)
        _refused(lambda: Session(gpu_ctx, A["circuit"], no_t, 1), "dctfhe_session_create: op ", "bootstraps on tier 1", "hold no bootstrap key of tier 1")
        _refused(lambda: Session(gpu_ctx, A["circuit"], no_q, 1), "dctfhe_session_create: op ", "key-switches with tier 0", "hold no key-switch key of tier 0")
    finally:
        no_t.close()
        no_q.close()
    # the primitives
    cts = client.encrypt(np.arange(5, dtype=U) << U(58))
    _refused(lambda: pruned.keyswitch(3, cts), "dctfhe_keyswitch", "no key-switch key of tier 3")
    _refused(lambda: pruned.keyswitch_pack(3, cts, D), "dctfhe_keyswitch_pack", "no key-switch key of tier 3")
    _refused(lambda: pruned.export_ksk(3), "no key-switch key of tier 3")
    small_q = pruned.keyswitch(0, cts)                          # q's key-switch key stayed: the switch runs, and is the full keys' switch
    assert np.array_equal(small_q, full.keyswitch(0, cts)) and np.array_equal(pruned.keyswitch(1, cts), small_q)
    _refused(lambda: pruned.pbs(0, small_q, key_check_table(4), 4), "dctfhe_pbs", "no bootstrap key of tier 0")
    _refused(lambda: pruned.pbs(3, full.keyswitch(3, cts), key_check_table(4), 4), "dctfhe_pbs", "no bootstrap key of tier 3")
    _refused(lambda: pruned.modswitch_center(0, small_q), "dctfhe_modswitch_center", "no bootstrap key of tier 0")
    _refused(lambda: pruned.bench_pbs(3, 4, 1), "dctfhe_bench_pbs", "no bootstrap key of tier 3")
    _refused(lambda: pruned.round_lut(2, 0, cts, 6, 2, key_check_table(4), 4), "dctfhe_round_lut", "no bootstrap key of tier 0")
    _refused(lambda: pruned.round_lut(3, 1, cts, 6, 2, key_check_table(4), 4), "dctfhe_round_lut", "no bootstrap key of tier 3")
    # a kept tier still bootstraps, to the words of the full keys
    small_t = pruned.modswitch_center(1, small_q.copy())
    assert np.array_equal(pruned.pbs(1, small_t, key_check_table(4), 4), full.pbs(1, small_t, key_check_table(4), 4))
    # a packed download on a tier whose key is absent
    sess = Session(gpu_ctx, A["circuit"], pruned, 1)
    try:
        _refused(lambda: sess.download_packed(3), "dctfhe_session_download_packed", "no key-switch key of tier 3")
    finally:
        sess.close()


@pytest.mark.parametrize("form", ["compressed", "full"])
def test_blobs_with_a_bad_selection_are_refused_before_anything_is_sized(A, gpu_ctx, form):
    import struct
    from dctfhe.engine import EvalKeys
    blob = A["cpruned"] if form == "compressed" else A["pruned_blob"]
    at = KT.HEADER + KT.params_bytes() + (32 if form == "compressed" else 0)
    assert struct.unpack_from("<II", blob[at:at + 8].tobytes()) == (0b0110, 0b0101)

    def patched(bsk, ksk):
        b = blob.copy()
        b[at:at + 8] = np.frombuffer(struct.pack("<II", bsk, ksk), np.uint8)
        return b
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, patched(0b0110, 0b0100)), "not closed: tier 1 bootstraps, the key-switch key of tier 0 is not selected")
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, patched(0b10110, 0b0101)), "at or beyond n_tiers = 4")
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, patched(0b0110, 0b0111)), "key-switch key of tier 1, which has none of its own")
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, patched(0b1111, 0b1101)), "selects every tier is written in the unpruned version")
    # a closed selection that is not this blob's: the size disagrees with the mask
    want = KT.blob_bytes(A["ps"], 0b0100, 0b0100, form == "compressed")
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, patched(0b0100, 0b0100)), f"blob is {blob.size} bytes, its parameters and tier selection need {want}")
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, blob[:-4096]), f"blob is {blob.size - 4096} bytes, its parameters and tier selection need {blob.size}")
    _refused(lambda: EvalKeys.from_blob(gpu_ctx, blob[:at + 4]), "too short for its tier selection")


# ------------------------------------------------------------------------------------------ 5. memory
def test_dropped_fourier_keys_are_not_resident(A):
    from dctfhe.engine import device_bytes_live
    ps, sel, client = A["ps"], A["sel"], A["client"]
    dropped = sum(b for i, (_, b) in enumerate(KT.sections(ps, False)) if not (sel.bsk_mask >> i) & 1)
    assert dropped == sum(KT.blocks(t) * (t.k + 1) ** 2 * t.l * (t.N // 2) * 16 for t in (ps.tiers[0], ps.tiers[3]))
    live0 = device_bytes_live()
    pruned = client.generate_eval_keys(sel)
    live1 = device_bytes_live()
    full = client.generate_eval_keys()
    live2 = device_bytes_live()
    full.close()
    pruned.close()
    assert device_bytes_live() == live0
    print(f"resident keys: full {live2 - live1} bytes, pruned {live1 - live0} bytes, dropped Fourier keys {dropped} bytes")
    assert (live2 - live1) - (live1 - live0) >= dropped


# ------------------------------------------------------------------------------------------ 6. roles
def _role(*argv):
    """one role in a fresh interpreter (tests/deploy_worker.py), as tests/test_gpu_deploy.py runs them"""
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, WORKER] + [str(a) for a in argv]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S + 30)
    assert r.returncode == 0, (argv[0], r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ROLE OK {argv[0]}" in r.stdout, r.stdout[-2000:]


def test_host_client_and_server_from_a_pruned_bundle_through_files(A, tmp_path):
    from dctfhe import deploy
    ps, sel = A["ps"], A["sel"]
    f = lambda name: str(tmp_path / name)
    qm = _module(ps, evaluation_key_tiers="circuit")
    try:
        deploy.save(qm, str(tmp_path), key_tiers="circuit")
        x = A["calib"][:2]
        want = qm.forward_quantized(qm.quantize_input(x), "disable")
    finally:
        qm.close()
    np.save(f("x.npy"), x)
    _role("keygen", "--device", "host", "--client", f("client.dctfhe"), "--key", f("client.key"), "--seed", 8, "--eval-keys", f("eval.keys"))
    assert os.path.getsize(f("eval.keys")) == KT.blob_bytes(ps, sel.bsk_mask, sel.ksk_mask, True)
    assert open(f("eval.keys"), "rb").read(8) == b"DEVC\x02\x00\x00\x00"
    _role("key-check", "make", "--device", "host", "--client", f("client.dctfhe"), "--key", f("client.key"), "--out", f("check.q"))
    _role("key-check", "answer", "--server", f("server.dctfhe"), "--eval-keys", f("eval.keys"), "--input", f("check.q"), "--out", f("check.a"))
    _role("key-check", "verify", "--device", "host", "--client", f("client.dctfhe"), "--key", f("client.key"), "--input", f("check.a"))
    _role("encrypt", "--device", "host", "--client", f("client.dctfhe"), "--key", f("client.key"), "--input", f("x.npy"), "--out", f("x.req"))
    _role("evaluate", "--server", f("server.dctfhe"), "--eval-keys", f("eval.keys"), "--request", f("x.req"), "--out", f("x.rsp"))
    _role("decrypt", "--device", "host", "--client", f("client.dctfhe"), "--key", f("client.key"), "--response", f("x.rsp"), "--out", f("out.npy"))
    assert np.array_equal(np.load(f("out.npy")), want)


def test_servers_check_coverage_not_equality(A, tmp_path):
    """a server with a FULL bundle takes pruned keys that cover its circuit and refuses, naming the tier, keys that really lack one; a
    packed form whose key-switch key is absent is refused before anything is uploaded"""
    from dctfhe import deploy
    from dctfhe.engine import device_bytes_live
    ps, sel, client = A["ps"], A["sel"], A["client"]
    qm = _module(ps)
    deploy.save(qm, str(tmp_path))
    server, cl = deploy.Server(str(tmp_path / deploy.SERVER_FILE)), deploy.Client(str(tmp_path / deploy.CLIENT_FILE))
    try:
        server.load_evaluation_keys(A["cpruned"])
        assert (server._keys.tiers.bsk, server._keys.tiers.ksk) == (sel.bsk_mask, sel.ksk_mask)
        live = device_bytes_live()
        with pytest.raises(ValueError, match=r"do not cover this bundle's circuit: they lack the bootstrap key of t, key-switch key of q"):
            server.load_evaluation_keys(client.export_eval_keys_compressed((0b0100, 0)))
        assert device_bytes_live() == live and server._keys is not None, "the refused keys replaced the ones in place"
        cl.keygen(seed=5)
        req = cl.encrypt(A["calib"][:1])
        tier = server.spec.output_compaction("rows").tier
        if (sel.ksk_mask >> tier) & 1:
            assert cl.decrypt(server.evaluate(req, packed="rows")).shape == (1, qm.compiled.n_out())
        else:
            live = device_bytes_live()
            with pytest.raises(ValueError, match=rf"key-switch key of tier {tier} \({ps.tiers[tier].name}\)"):
                server.evaluate(req, packed="rows")
            assert device_bytes_live() == live
        want = qm.forward_quantized(qm.quantize_input(A["calib"][:1]), "disable")
        assert np.array_equal(cl.decrypt(server.evaluate(req)), want)
    finally:
        cl.close()
        server.close()
        qm.close()


def test_quantized_module_under_circuit_tiers(A):
    """Configuration(evaluation_key_tiers="circuit"): keygen makes the selection, both exports ship it, a server module loads it and
    refuses keys that do not cover its circuit"""
    ps, sel = A["ps"], A["sel"]
    owner, server = _module(ps, evaluation_key_tiers="circuit"), _module(ps, evaluation_key_tiers="circuit")
    try:
        owner.fhe_circuit.keygen(seed=5)
        assert (owner._keys.eval.tiers.bsk, owner._keys.eval.tiers.ksk) == (sel.bsk_mask, sel.ksk_mask)
        assert np.array_equal(owner.export_evaluation_keys(compressed=True), A["cpruned"])
        assert np.array_equal(owner.export_evaluation_keys(compressed=False), A["pruned_blob"])
        q = owner.quantize_input(A["calib"][:1])
        assert np.array_equal(owner.forward_quantized(q, "execute"), owner.forward_quantized(q, "disable"))
        server.load_evaluation_keys(A["cpruned"])
        server.load_evaluation_keys(A["cfull"])                  # more than the circuit needs is fine
        with pytest.raises(ValueError, match="do not cover this circuit: they lack the bootstrap key of t, key-switch key of q"):
            server.load_evaluation_keys(A["client"].export_eval_keys_compressed((0b0100, 0)))
    finally:
        owner.close()
        server.close()


# ------------------------------------------------------------------------------------------ 7. the two-bit tiers, kept and dropped
@pytest.mark.parametrize("kept", [0b1001, 0b0110], ids=["p-d2-kept", "d-p2-kept"])
def test_two_bit_tiers_bootstrap_when_kept_and_are_refused_when_dropped(gpu_ctx, kept):
    """catalogue B: a 4-bit identity table through key switch, centred mod switch and bootstrap on every kept tier; the decrypted entries
    within half the spacing of the table's entries (2^-8 of the torus; the key check's own bound).  The Fourier key of d / d2 is permuted
    on export: its pruned full-form blob is the kept sections of the unpruned one all the same."""
    from dctfhe import params as P
    from dctfhe.deploy import key_check_table
    from dctfhe.engine import ClientKey, EvalKeys
    ps = KT.catalogue_b()
    cp = P.to_c_params(ps)
    client = ClientKey(gpu_ctx, cp, seed=6)
    keys = full = again = None
    try:
        keys, full = client.generate_eval_keys((kept, 0)), client.generate_eval_keys()
        ksk = keys.tiers.ksk
        assert (keys.tiers.bsk, ksk) == (kept, {0b1001: 0b1001, 0b0110: 0b0001}[kept])
        blob = keys.to_blob()
        assert np.array_equal(blob, KT.pruned_from_full(full.to_blob(), ps, kept, ksk, False))
        again = EvalKeys.from_blob(gpu_ctx, blob)
        assert np.array_equal(again.to_blob(), blob), "import + export of a pruned blob with a permuted tier is not the identity"
        w, table = 4, key_check_table(4)
        msgs = np.arange(1 << w, dtype=U)
        cts = client.encrypt(msgs << U(63 - w))
        for ti, t in enumerate(ps.tiers):
            if (kept >> ti) & 1:
                small = keys.modswitch_center(ti, keys.keyswitch(ti, cts))
                out = keys.pbs(ti, small, table, w)
                assert np.array_equal(out, full.pbs(ti, small, table, w)), (t.name, "pruned and full keys bootstrap to other words")
                assert np.array_equal(out, again.pbs(ti, small, table, w)), (t.name, "the imported pruned keys bootstrap to other words")
                err = np.abs((client.decrypt(out) - table.astype(U)).astype(np.int64).astype(np.float64)) / 2.0 ** 64
                print(f"tier {t.name}: largest error 2^{np.log2(max(err.max(), 2.0 ** -64)):.1f} of the torus")
                assert (err < 2.0 ** -8).all(), (t.name, err.max())
            else:
                small = full.modswitch_center(ti, full.keyswitch(ti, cts))
                _refused(lambda: keys.pbs(ti, small, table, w), "dctfhe_pbs", f"no bootstrap key of tier {ti}")
    finally:
        for h in (again, full, keys, client):
            if h is not None:
                h.close()
