"""Deployment bundles on the host (dctfhe/deploy.py; no GPU): save -> load reproduces every field of client.dctfhe
and server.dctfhe bit for bit, the client file holds no weights and no tables whatever the depth of the circuit, the loader refuses
pickles, foreign or truncated files and envelopes, a digest mismatch names both digests, and QuantizedModule keeps its surface."""
import dataclasses
import hashlib
import io
import json
import os
import stat
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the two client files of this module (no classifier) measure 2 093 bytes each; twice that
CLIENT_SPEC_MAX_BYTES = 4186


def _module(width, **cfg):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    return compile_brevitas_qat_model(models.tiny_resnet_q(width=width), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params(),
                                      configuration=Configuration(public_input_spec=P.test_public_input_spec(),
                                                                  result_packing_spec=P.test_pack_spec(), **cfg))


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """the tiny trunk at two depths under one catalogue (test_params), each saved once: {name: (module, client path, server path)}"""
    from dctfhe import deploy
    out = {}
    for name, width in (("shallow", (6, 8)), ("deep", (6, 6, 8))):
        qm = _module(width)
        out[name] = (qm,) + deploy.save(qm, str(tmp_path_factory.mktemp(name)))
    return out


def _canon(node):
    """a tree with floats as their IEEE-754 bytes and arrays as (dtype, shape, bytes): equality is bit for bit"""
    if isinstance(node, dict):
        return {str(k): _canon(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_canon(v) for v in node]
    if isinstance(node, (bytes, bytearray)):
        node = np.frombuffer(bytes(node), np.uint8)
    if isinstance(node, np.ndarray):
        return ("array", node.dtype.str.lstrip("<|="), node.shape, node.tobytes())
    if isinstance(node, (float, np.floating)):
        return ("f64", struct.pack("<d", float(node)))
    if isinstance(node, (np.integer,)):
        return int(node)
    return node


# ------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("name", ["shallow", "deep"])
def test_save_then_load_reproduces_every_field(saved, name):
    from dctfhe import compile as cc, deploy, params as P
    qm, cpath, spath = saved[name]
    want_client, want_server = deploy.bundle_trees(qm)
    got_client, got_server = deploy.read_container(cpath, "client"), deploy.read_container(spath, "server")
    assert _canon(got_client) == _canon(want_client)
    assert _canon(got_server) == _canon(want_server)
    assert set(got_client) <= set(deploy.CLIENT_KEYS) and set(got_server) == set(deploy.SERVER_KEYS)
    c = qm.compiled
    srv, cli = deploy.load_server_bundle(spath), deploy.load_client_spec(cpath)
    assert srv.blob == c.blob
    assert srv.digest == cli.digest == hashlib.sha256(c.blob).digest()
    for s in (srv, cli):
        assert s.param_set == c.param_set                                   # dataclass equality: every TierSpec field, floats exact
        assert P.to_c_params(s.param_set).input_sigma == P.to_c_params(c.param_set).input_sigma
        tin = c.tensors[c.input_tensor]
        assert s.input_shape == (tin.C, tin.H, tin.W) and s.n_in() == c.n_in() and s.n_out() == c.n_out()
        for f in ("in_scale", "in_bits", "e_in", "e_out", "out_scale", "out_bits"):
            assert _canon(getattr(s, f)) == _canon(getattr(c, f)), f
        assert s.dims() == (tin.deff or c.param_set.D, c.tensors[c.output_tensor].deff or c.param_set.D)
        assert _canon(vars(s.output_compaction("rows"))) == _canon(dataclasses.asdict(cc.output_compaction(c)))
        ring, want_ring = s.output_compaction("ring"), cc.output_compaction(c, form="ring", spec=P.test_pack_spec())
        assert ring.spec == want_ring.spec and isinstance(ring.spec, P.PackSpec)
        assert _canon(dict(vars(ring), spec=None)) == _canon(dict(dataclasses.asdict(want_ring), spec=None))
        plan, want_plan = s.public_input_plan(), cc.public_input_plan(c, P.test_public_input_spec())
        assert plan.spec == want_plan.spec and isinstance(plan.spec, P.PublicInputSpec)
        assert _canon(dict(vars(plan), spec=None)) == _canon(dict(dataclasses.asdict(want_plan), spec=None))
    assert _canon(srv.simulation_sigmas) == _canon([float(v) for v in c.simulation_sigmas()])
    assert _canon(srv.simulation_sigmas_split) == _canon([float(v) for v in c.simulation_sigmas_split()])
    assert cli.classifier is None


def test_floats_survive_bit_for_bit_and_classifier_is_optional(tmp_path):
    from dctfhe import deploy
    awkward = [0.1, 1.0 / 3.0, 2.0 ** -1074, 1.7976931348623157e308, -0.0, float("inf")]
    tree = dict(a=awkward, b=dict(c=np.float64(2.0 ** -55), d=[1, "x", None, True]), e=np.arange(5, dtype=np.int32))
    p = str(tmp_path / "t.dctfhe")
    deploy.write_container(p, "client", tree)
    assert _canon(deploy.read_container(p, "client")) == _canon(tree)
    qm = _module((6, 8))
    w, b = np.random.default_rng(2).normal(0, 1, (10, qm.compiled.n_out())), np.arange(10.0)
    cpath, _ = deploy.save(qm, str(tmp_path / "with_cls"), classifier=(w, b))
    spec = deploy.load_client_spec(cpath)
    assert spec.tree["has_classifier"] is True and np.array_equal(spec.classifier[0], w) and np.array_equal(spec.classifier[1], b)
    with pytest.raises(ValueError, match="classifier of shape"):
        deploy.save(qm, str(tmp_path / "bad_cls"), classifier=(w[:, :-1], b))


def test_a_refused_record_travels_as_its_text(tmp_path):
    """where the compiler refuses a form at save time the file carries the refusal, and the role raises it where pricing in place would"""
    from dctfhe import compile as cc, deploy, models, params as P
    from dctfhe.quantized_module import Configuration, QuantizedModule
    ps = P.test_params()
    for t in ps.tiers:
        t.lwe_sigma = 2.0 ** -9
    compiled = cc.compile_model(models.tiny_resnet_q(), np.random.default_rng(0).normal(0, 1, (16, 4, 6, 6)), param_set=ps)
    qm = QuantizedModule(compiled, configuration=Configuration(result_packing_spec=P.test_pack_spec(), public_input_spec=P.test_public_input_spec()))
    with pytest.raises(ValueError, match="p_fail") as e:
        qm.output_compaction("rows")
    cpath, spath = deploy.save(qm, str(tmp_path))
    for spec in (deploy.load_client_spec(cpath), deploy.load_server_bundle(spath)):
        with pytest.raises(ValueError) as got:
            spec.output_compaction("rows")
        assert str(got.value) == str(e.value)


# ------------------------------------------------------------------------------------------ weight-freeness
def test_client_spec_holds_no_weights(saved):
    from dctfhe import deploy
    from dctfhe._lib import MAX_TIERS
    from dctfhe.params import TierSpec
    assert deploy.CLIENT_KEYS == ("digest", "boundary", "param_set", "output_compaction", "public_input_plan", "has_classifier", "classifier_w",
                                  "classifier_b")
    cap = MAX_TIERS * len(dataclasses.fields(TierSpec))
    sizes, headers = {}, {}
    for name, (qm, cpath, _) in saved.items():
        raw = open(cpath, "rb").read()
        magic, version, hlen, total = struct.unpack_from("<8sIIQ", raw)
        assert (magic, version, total) == (b"DCTFHEDP", 1, len(raw))
        header = json.loads(raw[24:24 + hlen])
        assert set(header["tree"]) <= set(deploy.CLIENT_KEYS) and header["kind"] == "client"
        at = 24 + hlen
        for e in header["arrays"]:
            a = np.load(io.BytesIO(raw[at:at + e["nbytes"]]), allow_pickle=False)
            at += e["nbytes"]
            assert a.size <= cap, (name, e["name"], a.size)
        assert at == len(raw)
        sizes[name], headers[name] = len(raw), header
        print(f"client.dctfhe of the {name} trunk: {len(raw)} bytes; {len(qm.compiled.blob)} bytes of circuit blob stay with the server")
        assert len(raw) < CLIENT_SPEC_MAX_BYTES
        assert len(qm.compiled.blob) > 4 * len(raw)                      # the server's file is where the weights and tables are
    # two depths under one catalogue: the same keys, the same arrays of the same length, the same ParamSet -- only digest, scales,
    # shapes and priced records may differ
    a, b = headers["shallow"], headers["deep"]
    assert [e["name"] for e in a["arrays"]] == [e["name"] for e in b["arrays"]]
    assert [e["nbytes"] for e in a["arrays"]] == [e["nbytes"] for e in b["arrays"]]
    assert a["tree"]["param_set"] == b["tree"]["param_set"]
    assert set(a["tree"]) == set(b["tree"])
    assert abs(sizes["shallow"] - sizes["deep"]) < 64                     # digits of the JSON numbers, nothing that grows with depth
    ta, tb = (deploy.read_container(saved[n][1], "client") for n in ("shallow", "deep"))
    assert _canon(ta["param_set"]) == _canon(tb["param_set"])
    assert ta["digest"].tobytes() != tb["digest"].tobytes()
    assert len(saved["deep"][0].compiled.blob) > len(saved["shallow"][0].compiled.blob)


# ------------------------------------------------------------------------------------------ safety
def test_loader_refuses_pickles_and_foreign_or_truncated_files(saved, tmp_path):
    from dctfhe import deploy
    _, cpath, spath = saved["shallow"]
    raw = open(cpath, "rb").read()

    def refused(blob, text, kind="client", loader=deploy.load_client_spec):
        p = str(tmp_path / "bad.dctfhe")
        with open(p, "wb") as f:
            f.write(blob)
        with pytest.raises(ValueError, match=text):
            loader(p)
    refused(b"XCTFHEDP" + raw[8:], "wrong magic")
    refused(raw[:8] + struct.pack("<I", 2) + raw[12:], "unknown format version 2")
    refused(raw[:-1], "truncated file")
    refused(raw[:10], "truncated file")
    refused(raw + b"\0", "truncated file")
    refused(open(spath, "rb").read(), "a 'server' file where a 'client' file is expected")
    # a file whose array could only be read by unpickling: an object array in the classifier's place
    _, version, hlen, _ = struct.unpack_from("<8sIIQ", raw)
    header = json.loads(raw[24:24 + hlen])
    buf = io.BytesIO()
    np.save(buf, np.array([{"weights": 1}], dtype=object), allow_pickle=True)
    header["tree"]["has_classifier"], header["tree"]["classifier_w"], header["tree"]["classifier_b"] = True, {"$array": "evil"}, {"$array": "evil"}
    header["arrays"].append(dict(name="evil", nbytes=len(buf.getvalue())))
    hj = json.dumps(header, sort_keys=True).encode()
    body = raw[24 + hlen:] + buf.getvalue()
    refused(struct.pack("<8sIIQ", b"DCTFHEDP", 1, len(hj), 24 + len(hj) + len(body)) + hj + body, "needs allow_pickle=True, which this loader refuses")
    # a field outside the whitelist
    header = json.loads(raw[24:24 + hlen])
    header["tree"]["conv1_weight"] = [1, 2, 3]
    hj = json.dumps(header, sort_keys=True).encode()
    refused(struct.pack("<8sIIQ", b"DCTFHEDP", 1, len(hj), 24 + len(hj) + len(raw) - 24 - hlen) + hj + raw[24 + hlen:], "unexpected or missing fields")
    # a server bundle whose blob is not the one its digest names
    sraw = bytearray(open(spath, "rb").read())
    at = bytes(sraw).find(saved["shallow"][0].compiled.blob[:64])
    assert at > 0
    sraw[at + 100] ^= 1
    refused(bytes(sraw), "is not the digest the file states", loader=deploy.load_server_bundle)
    with pytest.raises(ValueError, match="object arrays are not stored"):
        deploy.write_container(str(tmp_path / "x"), "client", dict(a=np.array([object()], dtype=object)))


def test_envelopes_refuse_magic_version_truncation_and_digest(saved):
    from dctfhe import deploy
    d0, d1 = (deploy.load_client_spec(saved[n][1]).digest for n in ("shallow", "deep"))
    payload = deploy.rows_to_bytes(np.arange(10, dtype=np.uint64).reshape(2, 5), 4)
    req, rsp = deploy.pack_request(d0, 3, payload), deploy.pack_response(d0, 3, deploy.FORM_ROWS, payload)
    assert req[:4] == b"DREQ" and rsp[:4] == b"DRSP" and req[8:40] == d0 and req[44:] == payload and rsp[48:] == payload
    assert deploy.unpack_request(req, d0) == (3, payload) and deploy.unpack_response(rsp, d0) == (3, deploy.FORM_ROWS, payload)
    for blob, unpack, tag in ((req, deploy.unpack_request, "DREQ"), (rsp, deploy.unpack_response, "DRSP")):
        with pytest.raises(ValueError, match=f"truncated {tag} envelope"):
            unpack(blob[:20], d0)
        with pytest.raises(ValueError, match=f"truncated {tag} envelope"):
            unpack(b"", d0)
        with pytest.raises(ValueError, match="wrong magic"):
            unpack(b"XXXX" + blob[4:], d0)
        with pytest.raises(ValueError, match=f"unknown {tag} version 7"):
            unpack(blob[:4] + struct.pack("<I", 7) + blob[8:], d0)
        with pytest.raises(ValueError, match="digest mismatch") as e:
            unpack(blob, d1)
        assert d0.hex() in str(e.value) and d1.hex() in str(e.value)              # the message names the two digests
    # a truncated payload inside a whole envelope
    rows, dim = deploy.rows_from_bytes(payload)
    assert dim == 4 and rows.shape == (2, 5)
    with pytest.raises(ValueError, match="truncated ciphertext rows"):
        deploy.rows_from_bytes(payload[:-8])
    with pytest.raises(ValueError, match="truncated ciphertext rows"):
        deploy.rows_from_bytes(payload[:6])


def test_roles_refuse_on_the_host_before_any_device_object(saved, tmp_path):
    """Server.evaluate and Client.decrypt check envelope and digest first: no context, circuit or key exists when they refuse"""
    from dctfhe import deploy
    from dctfhe.engine import SeededCiphertexts
    server, client = deploy.Server(saved["shallow"][2]), deploy.Client(saved["shallow"][1])
    deep = deploy.load_client_spec(saved["deep"][1])
    sc = SeededCiphertexts(bytes(32), 1, 1024, 1024, np.zeros(144, np.uint64)).to_bytes()
    with pytest.raises(ValueError, match="digest mismatch") as e:
        server.evaluate(deploy.pack_request(deep.digest, 1, sc))
    assert server.spec.digest.hex() in str(e.value) and deep.digest.hex() in str(e.value)
    with pytest.raises(ValueError, match="truncated DREQ envelope"):
        server.evaluate(deploy.pack_request(server.spec.digest, 1, sc)[:30])
    with pytest.raises(ValueError, match="seeded-ciphertext blob of"):
        server.evaluate(deploy.pack_request(server.spec.digest, 1, sc[:-8]))
    with pytest.raises(ValueError, match="for batch 2 x 144 inputs"):
        server.evaluate(deploy.pack_request(server.spec.digest, 2, sc))
    with pytest.raises(ValueError, match="unknown magic"):
        server.evaluate(deploy.pack_request(server.spec.digest, 1, b"????" + sc[4:]))
    with pytest.raises(RuntimeError, match="needs the client's evaluation keys"):
        server.evaluate(deploy.pack_request(server.spec.digest, 1, sc))
    rows = deploy.rows_to_bytes(np.zeros((8, 5), np.uint64), 4)
    with pytest.raises(ValueError, match="digest mismatch") as e:
        client.decrypt(deploy.pack_response(deep.digest, 1, deploy.FORM_ROWS, rows))
    assert client.spec.digest.hex() in str(e.value) and deep.digest.hex() in str(e.value)
    with pytest.raises(ValueError, match="truncated DRSP envelope"):
        client.decrypt(deploy.pack_response(client.spec.digest, 1, deploy.FORM_ROWS, rows)[:40])
    with pytest.raises(ValueError, match="packed-ciphertext blob"):
        client.decrypt(deploy.pack_response(client.spec.digest, 1, deploy.FORM_PACKED, rows[:-3]))
    with pytest.raises(ValueError, match="inputs of shape"):
        client.quantize(np.zeros((1, 4, 6, 5)))
    assert server._ctx is None and server._circuit is None and client._ctx is None and client._key is None
    # the key file: the seed, bound to the digest, mode 0600; another circuit's key file is refused before a key is made
    seed = bytes(range(32))
    client._key = types.SimpleNamespace(seed=seed, close=lambda: None)
    kpath = str(tmp_path / "client.key")
    client.save_key(kpath)
    assert stat.S_IMODE(os.stat(kpath).st_mode) == 0o600
    raw = open(kpath, "rb").read()
    assert raw == b"DKEY" + struct.pack("<I", 1) + client.spec.digest + seed
    other = deploy.Client(saved["deep"][1])
    with pytest.raises(ValueError, match="digest mismatch"):
        other.load_key(kpath)
    with open(kpath, "wb") as f:
        f.write(raw[:-1])
    with pytest.raises(ValueError, match="truncated key file"):
        other.load_key(kpath)
    assert other._ctx is None and other._key is None


def test_key_check_places_messages_at_each_tiers_precision():
    from dctfhe import deploy, params as P
    assert deploy.key_check_bits(P.test_params()) == [6, 0]
    ps = P.default_params()
    bits = deploy.key_check_bits(ps)
    by_name = {t.name: w for t, w in zip(ps.tiers, bits)}
    assert by_name == {"T6": 6, "T4r": 4, "T4": 4, "B": 0, "T6a": 6, "Ba": 0, "T4r2": 4, "T5a": 5, "Ba2": 0}
    assert deploy.key_check_bits(P.default_params_5bit())[9] == 5
    for w in range(0, 8):
        m = deploy.key_check_messages(w)
        assert m.size == 4 and m.max() < max(2, 1 << w)
        t = deploy.key_check_table(w)
        assert t.size == (1 << w) if w else t.tolist() == [1 << 57]
    assert sorted(set(deploy.key_check_messages(0).tolist())) == [0, 1]           # a one-bit tier gets both signs
    assert sorted(set(deploy.key_check_messages(6).tolist())) == [0, 31, 32, 63]


# ------------------------------------------------------------------------------------------ no behaviour change
def test_quantized_module_surface_still_resolves(saved):
    from dctfhe import compile as cc, quantized_module as qmod, roles
    qm = saved["shallow"][0]
    for name in ("compiled", "configuration", "device", "verbose", "fhe_circuit", "last_timing", "last_io", "sim_seed", "output_compaction",
                 "export_result_packing_key", "load_result_packing_key", "public_input_plan", "export_public_key", "load_public_key",
                 "encrypt_public", "export_evaluation_keys", "load_evaluation_keys", "evaluate_encrypted", "statistics", "quantize_input",
                 "encode_input", "decode_output", "decrypt_result", "dequantize_output", "forward", "forward_quantized", "audit_quantized",
                 "audit", "close"):
        assert hasattr(qm, name), name
    for name in ("keygen", "export_evaluation_keys", "load_evaluation_keys", "evaluate_encrypted", "export_result_packing_key",
                 "load_result_packing_key", "export_public_key", "load_public_key", "encrypt_public", "statistics", "mlir", "graph"):
        assert hasattr(type(qm.fhe_circuit), name) or hasattr(qm.fhe_circuit, name), name
    for name in ("Configuration", "MarginReport", "FHECircuit", "QuantizedModule", "compile_brevitas_qat_model", "compile_torch_model", "_output_form"):
        assert hasattr(qmod, name), name
    assert cc.act_quant is roles.act_quant
    # the boundary functions compute what they computed: against their definitions, on the module and on the loaded spec alike
    from dctfhe import deploy
    spec = deploy.load_client_spec(saved["shallow"][1])
    x = np.random.default_rng(5).normal(0, 1, (2, 4, 6, 6))
    c = qm.compiled
    q = np.clip(np.rint(x / c.in_scale), -(2 ** (c.in_bits - 1)), 2 ** (c.in_bits - 1) - 1).astype(np.int64)
    assert np.array_equal(qm.quantize_input(x), q) and np.array_equal(roles.quantize_input(spec, x), q)
    ph = (q.astype(np.uint64) << np.uint64(c.e_in)).reshape(2, -1)
    assert np.array_equal(qm.encode_input(q), ph) and np.array_equal(roles.encode_input(spec, q), ph)
    vals = np.arange(-(1 << (c.out_bits - 1)), 1 << (c.out_bits - 1), dtype=np.int64).reshape(2, -1)     # every value an output takes
    noisy = (vals.astype(np.uint64) << np.uint64(c.e_out)) + np.uint64((1 << (c.e_out - 1)) - 1)
    assert np.array_equal(qm.decode_output(noisy), vals) and np.array_equal(roles.decode_output(spec, noisy), vals)
    assert np.array_equal(qm.dequantize_output(vals), vals * c.out_scale) and np.array_equal(roles.dequantize_output(spec, vals), vals * c.out_scale)
    with pytest.raises(ValueError, match="compress_output_ciphertexts"):
        qmod.Configuration(compress_output_ciphertexts="zip")


def test_roles_import_neither_the_compiler_nor_torch():
    """a client, a data owner or a server process: importing dctfhe.deploy pulls in neither dctfhe.compile nor torch"""
    code = ("import sys, dctfhe.deploy; bad = [m for m in ('torch', 'dctfhe.compile', 'dctfhe.models', 'dctfhe.quantized_module') if m in sys.modules]; "
            "print(bad); sys.exit(1 if bad else 0)")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "dct-cryptonets_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])


def test_save_command_writes_both_files_without_a_gpu(tmp_path):
    """python -m dctfhe.deploy save, in process: the tiny model on the test catalogue, classifier included"""
    from dctfhe import deploy
    assert deploy.main(["save", "--model", "tiny", "--test_params", "--calib_batch_size", "16", "--out", str(tmp_path)]) == 0
    cli, srv = deploy.load_client_spec(str(tmp_path / "client.dctfhe")), deploy.load_server_bundle(str(tmp_path / "server.dctfhe"))
    assert cli.digest == srv.digest == hashlib.sha256(srv.blob).digest() and cli.input_shape == (4, 6, 6)
    assert cli.classifier[0].shape == (10, cli.n_out()) and cli.output_compaction("ring").spec.logN == 8
    with pytest.raises(SystemExit, match="key-check answer needs --server, --eval-keys"):
        deploy.main(["key-check", "answer", "--input", "a", "--out", "b"])
