"""Exact 5-bit trunks on the GPU: the four-level refresh bootstrap pbs_kernel<11, 1, 4, 8> (tier T5r of dctfhe/params.py
default_params_5bit) decrypts every 5-bit message, agrees with the CPU oracle, leaves the output noise the catalogue was priced with,
survives full and compressed evaluation-key export / import, and carries whole 5-bit trunks to the integer circuit's outputs."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measurements (sigma, per-image timings) are printed; DCTFHE_MEASURE_DIR, when set, also receives them as JSON files
OUT = os.environ.get("DCTFHE_MEASURE_DIR")


def _record(fname, obj):
    print(fname, json.dumps(obj))
    if OUT:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, fname), "w") as f:
            json.dump(obj, f)


def _cent(x):
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


def _small_set(names):
    """the named tiers of the 5-bit catalogue on a D = 2048 big key (every one of them has k N <= 2048); ksk_share re-indexed"""
    import dataclasses
    from dctfhe import params as P
    full = P.default_params_5bit()
    idx = {t.name: i for i, t in enumerate(full.tiers)}
    tiers = []
    for nm in names:
        t = full.tiers[idx[nm]]
        share = names.index(full.tiers[t.ksk_share].name) if t.ksk_share >= 0 else -1
        tiers.append(dataclasses.replace(t, ksk_share=share))
    return P.ParamSet(D=2048, tiers=tiers, bit_tier=0, table_tier_for_w={5: len(tiers) - 1})


@pytest.fixture(scope="module")
def t5r_keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    ps = _small_set(["T5r"])
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=31)
    yield ps, keys
    keys.close()


def test_t5r_identity_all_messages_and_oracle(t5r_keys, oracle):
    """1301 ciphertexts (more than one round of 2-ciphertext workgroups over every CU, and an odd tail): each of the 32 messages of a 5-bit
    identity comes back; the first 8 decrypt to the oracle's values with noise of the oracle's size"""
    ps, keys = t5r_keys
    t = ps.tiers[0]
    N, w, count = t.N, 5, 1301
    msgs = np.arange(count, dtype=np.uint64) % np.uint64(1 << w)
    cts = keys.encrypt(msgs << np.uint64(63 - w))
    small = keys.keyswitch(0, cts)
    table = np.arange(1 << w, dtype=np.int64) << (63 - w - 2)
    out = keys.pbs(0, small, table, w)
    dec = lambda ph: ((ph + (np.uint64(1) << np.uint64(63 - w - 3))) >> np.uint64(63 - w - 2)) & np.uint64((1 << (w + 2)) - 1)
    S, _ = keys.export_secret()
    ph_dev = keys.decrypt(out)
    assert np.array_equal(dec(ph_dev), msgs), np.flatnonzero(dec(ph_dev) != msgs)[:10]
    assert not out[:, t.k * N: ps.D].any()
    bsk = keys.export_bsk(0)
    ref = oracle.pbs(small[:8], oracle.bsk_to_fourier(bsk), bsk, t.k, N, t.l, t.beta, table, w, None, ps.D)
    ph_ref = oracle.lwe_phase(S, ps.D, ref)
    assert np.array_equal(dec(ph_ref), dec(ph_dev[:8])) and np.array_equal(dec(ph_ref), msgs[:8])
    want = table.astype(np.uint64)[msgs[:8].astype(np.int64)]
    err_dev, err_ref = np.abs(_cent(ph_dev[:8] - want)), np.abs(_cent(ph_ref - want))
    assert err_dev.max() < max(4 * err_ref.max(), 2.0 ** -30), (err_dev.max(), err_ref.max())


def test_t5r_output_noise_matches_model(t5r_keys):
    """the l = 4 term of var_pbs_out is an extrapolation of the one-, two- and three-level tiers' calibration: measured sigma within
    [0.5x, 1.6x] of the model (the same window as tests/test_gpu_noise.py)"""
    from dctfhe import params as P
    ps, keys = t5r_keys
    t = ps.tiers[0]
    rng = np.random.default_rng(0)
    msgs = rng.integers(0, 8, 4096).astype(np.uint64)
    out = keys.pbs(0, keys.keyswitch(0, keys.encrypt(msgs << np.uint64(60))), np.arange(8, dtype=np.int64) << 57, 3)
    err = _cent(keys.decrypt(out) - (msgs << np.uint64(57)))
    assert np.abs(err).max() < 2.0 ** -9
    measured, model = err.std(), math.sqrt(P.var_pbs_out(t, P.default_params_5bit().fft_noise_c))
    _record("bw5_t5r_sigma.json", {"tier": "T5r", "log2_sigma_measured": math.log2(measured), "log2_sigma_model": math.log2(model)})
    assert 0.5 * model < measured < 1.6 * model, (math.log2(measured), math.log2(model))


def test_new_tiers_full_and_compressed_key_round_trip(gpu_ctx):
    """the new tiers (B on the longer key, Ba owning the n = 560 key-switch key Ba2 shares, T5r with 8 rows per key bit and its mask row in
    body form) through dctfhe_eval_keys_export (DEVK) and dctfhe_eval_keys_export_compressed (DEVC).  Full keys give bootstraps identical
    to the generated ones, word for word.  Compressed keys ship the rows whose gadget term sits in a mask polynomial in body form (same
    phase, other masks: DESIGN.md 3.5), so their bootstraps decrypt to the same values with noise of the same size, not to the same words."""
    from dctfhe import params as P
    from dctfhe.engine import ClientKey, EvalKeys
    ps = _small_set(["B", "Ba", "Ba2", "T5r"])
    cp = P.to_c_params(ps)
    client = ClientKey(gpu_ctx, cp, 17)
    gen = client.generate_eval_keys()
    full = EvalKeys.from_blob(gpu_ctx, gen.to_blob())
    comp_blob = client.export_eval_keys_compressed()
    assert comp_blob[:4].tobytes() == b"DEVC"
    comp = EvalKeys.from_blob(gpu_ctx, comp_blob)
    try:
        rng = np.random.default_rng(3)
        for ti, t in enumerate(ps.tiers):
            w = 5 if t.name == "T5r" else 0
            msgs = rng.integers(0, 1 << w, 96).astype(np.uint64) if w else rng.integers(0, 2, 96).astype(np.uint64)
            cts = client.encrypt(msgs << np.uint64(63 - w))
            table = (np.arange(1 << w, dtype=np.int64) << (63 - w - 2)) if w else np.array([1 << 57], np.int64)
            small = gen.keyswitch(ti, cts)
            assert np.array_equal(full.keyswitch(ti, cts), small) and np.array_equal(comp.keyswitch(ti, cts), small), t.name
            ref = gen.pbs(ti, small, table, w)
            assert np.array_equal(full.pbs(ti, small, table, w), ref), t.name
            want = (table[msgs.astype(np.int64)] if w else np.where(msgs == 0, np.int64(1 << 57), np.int64(-(1 << 57)))).astype(np.uint64)
            err_ref = np.abs(_cent(client.decrypt(ref) - want))
            err_comp = np.abs(_cent(client.decrypt(comp.pbs(ti, small, table, w)) - want))
            assert err_ref.max() < 2.0 ** -(w + 4) and err_comp.max() < 2.0 ** -(w + 4), t.name          # every value decrypts right
            assert err_comp.max() < 4 * err_ref.max() + 2.0 ** -40, (t.name, err_comp.max(), err_ref.max())
    finally:
        comp.close()
        full.close()
        gen.close()
        client.close()


def _oracle(qm, q):
    from oracle import circuit_ref
    out, ov = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not ov
    return qm.decode_output(out)


@pytest.mark.parametrize("name", ["r20_24_16", "r18_3_32"])
def test_5bit_trunk_one_image_bit_exact(name):
    """one encrypted image of a 5-bit trunk on the default (5-bit exact) catalogue equals the integer circuit on every output"""
    import warnings
    import bench
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    factory, in_ch, img, make_batch, _ = bench.CONFIGS[name]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        qm = compile_brevitas_qat_model(getattr(models, factory)(bit_width=5, in_channels=in_ch, img_size=img, seed=0), make_batch(100, 7),
                                        n_bits=5, rounding_threshold_bits=6)
    try:
        assert not [str(x.message) for x in caught if "exact-evaluation budget" in str(x.message)]      # the 5-bit catalogue holds
        assert "T5r" in [t.name for t in qm.compiled.param_set.tiers] and qm.compiled.worst_site_failure <= 1e-12
        q = qm.quantize_input(make_batch(1, 42))
        want = _oracle(qm, q)
        qm.fhe_circuit.keygen(seed=5)
        got = qm.forward_quantized(q, "execute")
        _record(f"bw5_{name}_execute.json", dict(qm.last_timing, images=1, pbs_per_image=qm.compiled.pbs_counts(),
                                                 worst_site=qm.compiled.worst_site_failure))
        assert np.array_equal(got, want), np.argwhere(got != want)
    finally:
        qm.close()


def test_cli_bit_width_5_execute():
    """the homomorphic_eval.py mirror with --bit_width 5 (no new flags): compiles on the 5-bit catalogue without a budget warning, runs one
    encrypted image, and its encrypted accuracy equals the unencrypted one"""
    import re
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"), "--dataset", "cifar10", "--model", "ResNet20qat",
           "--dct_status", "--channels", "24", "--filter_size", "4", "--image_size_dct", "16", "--bit_width", "5", "--fhe_mode", "execute",
           "--calib_batch_size", "32", "--test_batch_size", "1", "--test_subset", "1", "--rounding_threshold_bits", "6", "--n_bits", "5",
           "--p_error", "0.01"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(os.environ.get("TMPDIR", "/tmp")))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "exceeds the exact-evaluation budget" not in out.stderr, out.stderr[-2000:]
    for needle in ("Time for FHE compilation", "it works in FHE!!", "Keygen time:", "Time per inference in FHE", "Done"):
        assert needle in out.stdout, out.stdout
    accs = re.findall(r"\[Test\] Top-1 Acc: ([0-9.]+)% \| Top-5 Acc: ([0-9.]+)%", out.stdout)
    assert len(accs) == 2 and accs[0] == accs[1], out.stdout
