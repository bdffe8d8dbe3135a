"""Public-key inputs, host side (no GPU): the numpy reference (tests/public_ref.py) encrypts, extracts and decrypts consistently and its
error is exactly E u + e2 - e1 Z, the PublicInputs wire form, PublicInputSpec and its variance, the compiler's price and refusal
(dctfhe.compile.public_input_plan), the Configuration switch, the binding of the entry points, and the CLI flag."""
import ctypes as C
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest

import public_ref
from ring_ref import negashift
from test_cli_flags import REFERENCE_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64


def _compile(ps):
    from dctfhe import compile as cc, models
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    return cc.compile_model(models.tiny_resnet_q(), calib, rounding_threshold_bits=6, n_bits=5, param_set=ps)


def _gauss(rng, sigma, n):
    return np.rint(rng.normal(0, sigma, n) * 2.0 ** 64).astype(np.int64)


def numpy_public_key(rng, Z, sigma):
    """([2, N] rows (A, A Z + E), E signed)"""
    N = Z.size
    A = rng.integers(0, 1 << 64, N, dtype=U)
    E = _gauss(rng, sigma, N)
    return np.stack([A, public_ref.negamul_binary(A, Z) + E.view(U)]), E


# ------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("logN,count,dim", [(5, 1, 32), (5, 33, 40), (8, 256, 256), (8, 300, 293)])
def test_reference_is_self_consistent_and_its_error_is_exact(logN, count, dim):
    rng = np.random.default_rng(100 * logN + count)
    N, sigma = 1 << logN, 2.0 ** -40
    groups, nmask = -(-count // N), -(-count // N) * N
    S = rng.integers(0, 2, dim).astype(np.uint8)                     # the big key's first dim bits; the ring key is its first N
    Z = S[:N]
    rows, E = numpy_public_key(rng, Z, sigma)
    u = rng.integers(0, 2, nmask).astype(np.uint8)
    e1, e2 = _gauss(rng, sigma, nmask), _gauss(rng, sigma, count)
    phases = rng.integers(0, 1 << 64, count, dtype=U)
    words = public_ref.encrypt(rows, u, e1, e2, phases)
    assert words.dtype == U and words.size == groups * N + count
    lwe = public_ref.extract(words, logN, count, dim)
    assert lwe.shape == (count, dim + 1) and not lwe[:, N:dim].any()
    got = public_ref.lwe_phase(lwe, S)
    assert np.array_equal(got, public_ref.decrypt(words, Z, logN, count))
    # message + error, the error exactly E u + e2 - e1 Z per group
    want = np.empty(count, U)
    for g in range(groups):
        m = min(N, count - g * N)
        ug = u[g * N:(g + 1) * N]
        err = public_ref.negamul_binary(E.view(U), ug) - public_ref.negamul_binary(e1[g * N:(g + 1) * N].view(U), Z)
        want[g * N:g * N + m] = phases[g * N:g * N + m] + err[:m] + e2[g * N:g * N + m].view(U)
    assert np.array_equal(got, want)
    # slot 0, slot N - 1 and a middle slot, written out: the mask of slot i is C_a read backwards from i, negated past the wrap
    A, B = words[:N], words[N:N + min(N, count)]
    for i in sorted({0, min(N, count) - 1, min(N, count) // 2}):
        a = [int(A[i - j]) if j <= i else -int(A[N + i - j]) % 2 ** 64 for j in range(N)]          # Python integers: no wrap to think about
        assert lwe[i, :N].tolist() == a and lwe[i, dim] == B[i]
        assert (int(B[i]) - sum(x for x, z in zip(a, Z) if z)) % 2 ** 64 == int(got[i])
    if count >= N:
        assert np.array_equal(lwe[0, 1:N], U(0) - A[:0:-1]) and lwe[0, 0] == A[0]              # slot 0: every word past the first wraps
        assert np.array_equal(lwe[N - 1, :N], A[::-1])                                        # slot N - 1: no wrap at all
    err = (got - phases).astype(np.int64).astype(np.float64) / 2.0 ** 64
    assert 0 < np.abs(err).max() < 8.0 * math.sqrt((N + 1)) * sigma


def test_reference_negashift_is_the_products_building_block():
    K = np.arange(1, 9, dtype=U)
    u = np.array([0, 1, 0, 0, 0, 0, 0, 1], np.uint8)
    assert np.array_equal(public_ref.negamul_binary(K, u), negashift(K, 1) + negashift(K, 7))
    assert int(public_ref.negamul_binary(K, u)[0]) == (-int(K[7]) - int(K[1])) % 2 ** 64       # c = 0 < i: both terms wrapped


# ------------------------------------------------------------------------------------------ wire object
def test_public_inputs_round_trip_and_refusals():
    from dctfhe.engine import PublicInputs
    words = np.random.default_rng(3).integers(0, 1 << 64, PublicInputs.n_words(8, 300), dtype=U)
    pi = PublicInputs(8, 300, words)
    blob = pi.to_bytes()
    assert blob[:4] == b"DPIN" and len(blob) == 20 + 8 * (512 + 300) == pi.nbytes and len(pi) == 300
    back = PublicInputs.from_bytes(blob)
    assert (back.logN, back.count) == (8, 300) and np.array_equal(back.words, words) and back.words.dtype == U
    assert PublicInputs.n_words(11, 6144) * 8 == 98304 and PublicInputs.n_words(8, 257) == 769 and PublicInputs.n_words(5, 32) == 64
    for bad, needle in [(b"XPIN" + blob[4:], "magic"), (blob[:4] + b"\x02" + blob[5:], "version"), (blob[:-8], "header says"),
                        (blob + bytes(8), "header says"), (blob[:10], "too short"),
                        (blob[:8] + (13).to_bytes(4, "little") + blob[12:], "header says")]:
        with pytest.raises(ValueError, match=needle):
            PublicInputs.from_bytes(bad)
    with pytest.raises(ValueError, match="logN"):
        PublicInputs(4, 1, np.zeros(17, U))
    with pytest.raises(ValueError, match="words"):
        PublicInputs(8, 300, words[:-1])
    with pytest.raises(ValueError, match="count"):
        PublicInputs(8, -1, np.zeros(0, U))


# ------------------------------------------------------------------------------------------ spec and variance
def test_public_input_spec_bounds_and_defaults():
    from dctfhe import params as P
    d = P.PublicInputSpec()
    assert (d.logN, d.N, d.sigma) == (11, 2048, P.sigma_min(2048))
    assert P.PublicInputSpec(sigma=0.0).sigma == 0.0 and P.PublicInputSpec(5, 2.0 ** -30).N == 32 and P.PublicInputSpec(12).N == 4096
    with pytest.raises(ValueError, match="noise"):
        P.PublicInputSpec(5)                                          # sigma_min(32) > 1: a ring that small takes an explicit (test) sigma
    for logN in (4, 13, 0, -1):
        with pytest.raises(ValueError, match="logN"):
            P.PublicInputSpec(logN)
    with pytest.raises(ValueError, match="noise"):
        P.PublicInputSpec(8, 1.0)
    assert d.words(6144) == 3 * 2048 + 6144 and d.groups(2049) == 2 and d.words(1) == 2049
    spec = P.default_public_input_spec(P.default_params())            # input_dim 2048: the ring fits exactly
    assert (spec.logN, spec.sigma) == (11, P.sigma_min(2048))
    assert P.default_public_input_spec().logN == 11
    with pytest.raises(ValueError, match="N_e = 2048 > 1024"):
        P.default_public_input_spec(P.test_params())                  # D = 1024, no input_dim
    ps = P.default_params()
    ps.input_dim = 512
    with pytest.raises(ValueError, match="N_e = 2048 > 512"):
        P.default_public_input_spec(ps)
    with pytest.raises(ValueError, match="N_e = 1024 > 512"):
        P.PublicInputSpec(10).check(ps)
    assert P.PublicInputSpec(9).check(ps).N == 512
    t = P.test_public_input_spec()
    assert (t.logN, t.sigma) == (8, 2.0 ** -48) and t.check(P.test_params()) is t
    # stand-alone: no ParamSet field carries it
    assert not any("public" in f for f in P.ParamSet.__dataclass_fields__)


def test_var_public_input_restates_the_formula():
    from dctfhe import params as P
    spec = P.PublicInputSpec()
    assert P.var_public_input(spec) == 2049 * P.sigma_min(2048) ** 2
    assert P.var_public_input(P.test_public_input_spec()) == 257 * 2.0 ** -96
    assert -46.5 < 0.5 * math.log2(P.var_public_input(spec)) < -45.5      # sigma ~ 2^-46, far below the stem's key switch
    assert P.var_public_input(P.PublicInputSpec(8, 0.0)) == 0.0


# ------------------------------------------------------------------------------------------ compiler
def test_public_input_plan_tiny_model_and_blob_untouched():
    from dctfhe import compile as cc, params as P
    circ = _compile(P.test_params())
    blob, report = circ.blob, circ.report()
    pfails = [getattr(o, "pfail", None) for o in circ.ops]
    var_in, fails = circ.tensors[circ.input_tensor].var, circ.expected_failures_per_image
    spec = P.test_public_input_spec()
    plan = cc.public_input_plan(circ, spec)
    assert plan.spec is spec and plan.var == P.var_public_input(spec) == 257 * 2.0 ** -96
    assert plan.inputs_per_image == circ.n_in() == 144 and plan.bytes_per_image == 8 * (256 + 144)
    assert plan.bytes_per_batch(3) == 8 * (512 + 432)
    sites = [i for i, o in enumerate(circ.ops) if o.type in (cc.OP_LUT, cc.OP_MAXPOOL)]
    assert plan.worst_site in sites and plan.worst_pfail <= circ.param_set.p_budget and plan.worst_pfail >= plan.worst_pfail_fresh > 0
    assert plan.worst_note == circ.ops[plan.worst_site].note
    # nothing of it touched the circuit
    assert circ.blob == blob and circ.report() == report
    assert [getattr(o, "pfail", None) for o in circ.ops] == pfails
    assert circ.tensors[circ.input_tensor].var == var_in and circ.expected_failures_per_image == fails
    with pytest.raises(ValueError, match="N_e = 2048 > 1024"):
        cc.public_input_plan(circ)                                    # the default ring of 2048 is no prefix of a 1024-bit key
    with pytest.raises(ValueError, match="leave the budget") as e:
        cc.public_input_plan(circ, P.PublicInputSpec(8, 2.0 ** -12))
    assert "p_fail" in str(e.value) and "N_e = 256" in str(e.value)
    assert circ.blob == blob and circ.report() == report


def test_public_input_plan_resnet20():
    from dctfhe import compile as cc, models, params as P
    from dctfhe.synthetic import synthetic_dct_batch
    circ = cc.compile_model(models.ResNet20QAT(4, 24, 16), synthetic_dct_batch(16, seed=7))
    blob, report = circ.blob, circ.report()
    plan = cc.public_input_plan(circ)
    assert (plan.spec.logN, plan.spec.sigma) == (11, P.sigma_min(2048)) and plan.var == 2049 * P.sigma_min(2048) ** 2
    assert plan.inputs_per_image == 6144 and plan.bytes_per_image == 98304 == 16 * 6144        # three full groups
    assert plan.worst_pfail <= circ.param_set.p_budget
    # the stem's key switch dwarfs 2^-46: the worst site is what it was with fresh inputs, to the last digits
    assert plan.worst_pfail == pytest.approx(circ.worst_site_failure, rel=1e-6)
    with pytest.raises(ValueError, match="leave the budget") as e:
        cc.public_input_plan(circ, P.PublicInputSpec(11, 2.0 ** -8))
    assert "op 1" in str(e.value) and "2^-8.0" in str(e.value)
    assert circ.blob == blob and circ.report() == report


# ------------------------------------------------------------------------------------------ facade
def test_configuration_switch_and_mutual_exclusion():
    from dctfhe import params as P
    from dctfhe.quantized_module import Configuration
    c = Configuration()
    assert c.public_key_inputs is False and c.public_input_spec is None
    spec = P.test_public_input_spec()
    c = Configuration(public_key_inputs=True, public_input_spec=spec, compress_output_ciphertexts="ring")
    assert c.public_key_inputs is True and c.public_input_spec is spec and c.compress_output_ciphertexts == "ring"
    with pytest.raises(ValueError, match="exclude each other"):
        Configuration(public_key_inputs=True, compress_input_ciphertexts=True)
    assert Configuration(compress_input_ciphertexts=True).compress_input_ciphertexts is True       # alone it is what it was


def test_module_prices_before_anything_is_encrypted():
    """a spec that leaves the budget is refused by the facade without a device: export_public_key, load_public_key and evaluate_encrypted
    consult public_input_plan first"""
    from dctfhe import params as P
    from dctfhe.engine import PublicInputs
    from dctfhe.quantized_module import Configuration, QuantizedModule
    circ = _compile(P.test_params())
    qm = QuantizedModule(circ, configuration=Configuration(public_key_inputs=True, public_input_spec=P.PublicInputSpec(8, 2.0 ** -12)))
    with pytest.raises(ValueError, match="leave the budget"):
        qm.fhe_circuit.export_public_key()
    with pytest.raises(ValueError, match="leave the budget"):
        qm.fhe_circuit.load_public_key(b"")
    with pytest.raises(ValueError, match="leave the budget"):
        qm.fhe_circuit.evaluate_encrypted(PublicInputs(8, 144, np.zeros(400, U)).to_bytes(), 1)
    ok = QuantizedModule(circ, configuration=Configuration(public_input_spec=P.test_public_input_spec()))
    assert ok.public_input_plan().bytes_per_image == 3200
    with pytest.raises(RuntimeError, match="load_public_key"):
        ok.fhe_circuit.encrypt_public(np.zeros((1, 4, 6, 6)))


# ------------------------------------------------------------------------------------------ library, host-only entry point
def test_public_entry_points_are_bound_and_public_words_counts():
    from dctfhe import _lib as lib, params as P
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dctfhe.h")).read()
    for name in ("dctfhe_public_key_export", "dctfhe_public_key_import", "dctfhe_public_key_destroy", "dctfhe_public_key_info",
                 "dctfhe_public_key_export_rows", "dctfhe_public_key_set_encrypt_seed", "dctfhe_public_key_draws", "dctfhe_public_words",
                 "dctfhe_encrypt_public", "dctfhe_ring_extract", "dctfhe_session_upload_public"):
        assert name in lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    L.dctfhe_public_words.restype, L.dctfhe_public_words.argtypes = C.c_size_t, [C.c_int, C.c_size_t]
    for logN in (5, 8, 11, 12):
        spec = P.PublicInputSpec(logN, 0.0)
        for count in (0, 1, spec.N - 1, spec.N, spec.N + 1, 2 * spec.N + 7, 150528):
            assert L.dctfhe_public_words(logN, count) == spec.words(count), (logN, count)
    assert L.dctfhe_public_words(11, 6144) * 8 == 98304 and L.dctfhe_public_words(8, 144) == 400


def test_build_records_no_scratch_for_the_public_input_kernels():
    from dctfhe import _lib as lib
    path = os.path.join(ROOT, "dct-cryptonets_amd", "build_resources.txt")
    if not os.path.exists(lib.LIB_PATH) or not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    rows = [ln.split() for ln in open(path) if "k_pk_encrypt" in ln or "k_pk_extract" in ln]
    assert len(rows) == 2, rows
    for r in rows:
        assert int(r[3]) == 0, r                                   # scratch bytes per lane


# ------------------------------------------------------------------------------------------ CLI mirror
def test_cli_flag_parses_and_reference_defaults_stay(monkeypatch):
    from dctfhe.quantized_module import Configuration
    spec = importlib.util.spec_from_file_location("he_cli_public", os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py"])
    ns = vars(mod.parse_args())
    assert ns["public_key_inputs"] is False and ns["compress_outputs"] == "none"
    for k, v in REFERENCE_FLAGS.items():
        assert k in ns and ns[k] == v, (k, ns.get(k), v)
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--public_key_inputs", "--fhe_mode", "execute"])
    ns = vars(mod.parse_args())
    assert ns["public_key_inputs"] is True and ns["fhe_mode"] == "execute"
    assert Configuration(public_key_inputs=ns["public_key_inputs"]).public_key_inputs is True
    for k, v in REFERENCE_FLAGS.items():
        if k != "fhe_mode":
            assert ns[k] == v, (k, ns[k], v)
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--public_key_inputs", "yes"])
    with pytest.raises(SystemExit):
        mod.parse_args()
