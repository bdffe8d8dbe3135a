"""Deployment bundles on the GPU (dctfhe/deploy.py): client, data owner and server as separate processes that share
nothing but files (tests/deploy_worker.py runs the command line, one role per process, each under its own time limit, one at a time), with
public-key inputs and ring-packed results, with seeded inputs and 16-bit rows, and the key check; then, in this process, the key check
against another key set, a truncated key blob, and the digest refusal before any upload."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "deploy_worker.py")
LIMIT_S = 120


def _role(*argv):
    """one role in a fresh interpreter; return code 0 is asserted before the caller starts the next one"""
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, WORKER] + [str(a) for a in argv]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S + 30)
    assert r.returncode == 0, (argv[0], r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ROLE OK {argv[0]}" in r.stdout, r.stdout[-2000:]


def _module(width):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(width=width), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params(),
                                    configuration=Configuration(public_input_spec=P.test_public_input_spec(), result_packing_spec=P.test_pack_spec()))
    return qm, calib


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    """save() once, the expected integers of two images from forward(fhe="disable"), and child 1: the client makes and exports its keys"""
    from dctfhe import deploy
    d = tmp_path_factory.mktemp("deploy")
    f = lambda name: str(d / name)
    qm, calib = _module((6, 8))
    try:
        deploy.save(qm, str(d))
        x = calib[:2]
        want = qm.forward_quantized(qm.quantize_input(x), "disable")
        assert np.array_equal(qm.forward(x, fhe="disable"), qm.dequantize_output(want))
    finally:
        qm.close()
    np.save(f("x.npy"), x)
    np.save(f("expected.npy"), want)
    _role("keygen", "--client", f("client.dctfhe"), "--key", f("client.key"), "--seed", 8, "--eval-keys", f("eval.keys"), "--public-key", f("public.key"),
          "--packing-key", f("packing.key"))
    assert os.stat(f("client.key")).st_mode & 0o777 == 0o600 and os.path.getsize(f("client.key")) == 72
    assert open(f("eval.keys"), "rb").read(4) == b"DEVC"                         # the compressed form
    return f


def test_three_parties_four_processes_files_only(deployment):
    f = deployment
    _role("owner-encrypt", "--client", f("client.dctfhe"), "--public-key", f("public.key"), "--input", f("x.npy"), "--out", f("owner.req"))
    _role("evaluate", "--server", f("server.dctfhe"), "--eval-keys", f("eval.keys"), "--packing-key", f("packing.key"), "--request", f("owner.req"),
          "--packed", "ring", "--out", f("ring.rsp"))
    _role("decrypt", "--client", f("client.dctfhe"), "--key", f("client.key"), "--response", f("ring.rsp"), "--out", f("ring_out.npy"))
    req, rsp = open(f("owner.req"), "rb").read(), open(f("ring.rsp"), "rb").read()
    assert req[:4] == b"DREQ" and req[44:48] == b"DPIN" and rsp[:4] == b"DRSP" and rsp[48:52] == b"DRCT" and req[8:40] == rsp[8:40]
    got, want = np.load(f("ring_out.npy")), np.load(f("expected.npy"))
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("form,packed,magics", [("seeded", "rows", (b"DSCT", b"DPCT")), ("rows", "none", (b"DROW", b"DROW"))])
def test_secret_key_inputs_and_row_results(deployment, form, packed, magics):
    f = deployment
    _role("encrypt", "--client", f("client.dctfhe"), "--key", f("client.key"), "--input", f("x.npy"), "--form", form, "--out", f(form + ".req"))
    _role("evaluate", "--server", f("server.dctfhe"), "--eval-keys", f("eval.keys"), "--request", f(form + ".req"), "--packed", packed,
          "--out", f(form + ".rsp"))
    _role("decrypt", "--client", f("client.dctfhe"), "--key", f("client.key"), "--response", f(form + ".rsp"), "--out", f(form + "_out.npy"))
    assert open(f(form + ".req"), "rb").read()[44:48] == magics[0] and open(f(form + ".rsp"), "rb").read()[48:52] == magics[1]
    assert np.array_equal(np.load(f(form + "_out.npy")), np.load(f("expected.npy")))


def test_key_check_passes_with_matching_keys(deployment):
    f = deployment
    _role("key-check", "make", "--client", f("client.dctfhe"), "--key", f("client.key"), "--out", f("check.q"))
    _role("key-check", "answer", "--server", f("server.dctfhe"), "--eval-keys", f("eval.keys"), "--input", f("check.q"), "--out", f("check.a"))
    _role("key-check", "verify", "--client", f("client.dctfhe"), "--key", f("client.key"), "--input", f("check.a"))
    assert open(f("check.q"), "rb").read(4) == b"DKCQ" and open(f("check.a"), "rb").read(4) == b"DKCA"


def test_key_check_names_the_tier_and_truncated_keys_are_refused(deployment):
    """evaluation keys of a second key set: every bootstrap decrypts to noise under the first client's secret; a blob that lost its last
    4 096 bytes: the library's length check"""
    from dctfhe import deploy
    from dctfhe._lib import DctfheError
    f = deployment
    mine, other, server = deploy.Client(f("client.dctfhe")), deploy.Client(f("client.dctfhe")), deploy.Server(f("server.dctfhe"))
    try:
        mine.load_key(f("client.key"))
        other.keygen(seed=9)
        full = mine.export_evaluation_keys(compressed=False)
        assert np.array_equal(mine.export_evaluation_keys(), np.frombuffer(open(f("eval.keys"), "rb").read(), np.uint8))     # the seed is the key
        check = mine.make_key_check()
        server.load_evaluation_keys(full)
        mine.verify_key_check(server.answer_key_check(check))                     # the full blob form passes as the compressed one did
        server.load_evaluation_keys(other.export_evaluation_keys())
        with pytest.raises(deploy.KeyCheckError, match=r"key check failed on tier \d+ \(\w+\)"):
            mine.verify_key_check(server.answer_key_check(check))
        other.verify_key_check(server.answer_key_check(other.make_key_check()))   # ... and they are the other client's keys
        for blob in (full, mine.export_evaluation_keys()):
            with pytest.raises(DctfheError, match=rf"evaluation-key blob is {blob.size - 4096} bytes, its parameters need {blob.size}"):
                server.load_evaluation_keys(blob[:-4096])
    finally:
        for r in (server, other, mine):
            r.close()


def test_server_refuses_another_circuits_request_before_any_upload(deployment, tmp_path):
    from dctfhe import deploy
    from dctfhe.engine import device_bytes_live
    f = deployment
    deep, calib = _module((6, 6, 8))
    deploy.save(deep, str(tmp_path))
    theirs, server = deploy.Client(str(tmp_path / "client.dctfhe")), deploy.Server(f("server.dctfhe"))
    try:
        theirs.keygen(seed=8)
        request = theirs.encrypt(calib[:1])
        server.load_evaluation_keys(open(f("eval.keys"), "rb").read())
        live = device_bytes_live()
        with pytest.raises(ValueError, match="digest mismatch") as e:
            server.evaluate(request)
        assert device_bytes_live() == live
        assert theirs.spec.digest.hex() in str(e.value) and server.spec.digest.hex() in str(e.value)
        assert server._sessions == {} and server._circuit is None                 # nothing was created for it
        with pytest.raises(ValueError, match="truncated DREQ envelope"):
            server.evaluate(request[:43])
        assert device_bytes_live() == live
    finally:
        server.close()
        theirs.close()
