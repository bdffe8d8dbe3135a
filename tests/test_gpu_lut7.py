"""Exact 7-bit tables on the GPU: the parity split -- one more one-bit step, the parity bootstrapped into the padding
bit, two 6-bit look-ups S[t'] + (-1)^b0 Dt[t'] -- as a primitive on the full-size tiers, its output noise against the compiler's figure,
whole circuits compiled with rounding_threshold_bits=7 against the frozen integer interpreter, and `simulate` sampling both look-ups."""
import json
import math
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DCTFHE_MEASURE_DIR")      # measurements are printed; when set, they are also written there as JSON
E_OUT = 56                                       # output encoding of the primitive's tables: 7-bit signed values, spacing 2^-8


def _record(fname, obj):
    print(fname, json.dumps(obj))
    if OUT:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, fname), "w") as f:
            json.dump(obj, f)


def _cent(x):
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


@pytest.fixture(scope="module")
def full_keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    ps = P.default_params()
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=41)
    yield ps, keys
    keys.close()


def _tables(rng, signed, ntab=4):
    """per-channel random tables of 128 entries, odd ones among them; signed: both signs"""
    lo, hi = (-64, 64) if signed else (0, 64)
    vals = rng.integers(lo, hi, (ntab, 128), dtype=np.int64)
    vals[:, ::5] |= 1
    return vals


@pytest.mark.parametrize("second", ["T6a", "T6"])
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("p,r", [(7, 0), (11, 4)])
def test_primitive_every_message(full_keys, p, r, signed, second):
    """dctfhe_round_lut (w = 7 splits inside, both look-ups on T6a) and dctfhe_round_lut_split (second look-up on the quiet twin T6) on
    the default catalogue: every one of the 2^p messages, 8 fresh encryptions each, decrypts to T[(m + 2^(r-1)) >> r] -- zero mismatches
    (the model puts each look-up below 1e-12).  Signed: the index is value + 2^(p-1) (the offset a circuit puts into the body) and the
    tables hold both signs.  The top 2^(r-1) messages round up into the padding bit: index 128 is -T[0], the negacyclic rule of every
    table bootstrap (tests/test_gpu_primitives.py test_pbs_negacyclic_rule), which both half look-ups follow."""
    ps, keys = full_keys
    names = [t.name for t in ps.tiers]
    rng = np.random.default_rng(100 * p + 10 * signed + (second == "T6"))
    vals = _tables(rng, signed)
    tables = vals << E_OUT
    idx_msgs = np.repeat(np.arange(1 << p, dtype=np.uint64), 8)              # offset-binary index of the accumulator value
    tab_idx = (np.arange(idx_msgs.size) % vals.shape[0]).astype(np.int32)
    if signed:      # value v = idx - 2^(p-1), encoded v << (63 - p), + 2^62 on the body: the same phase as idx << (63 - p)
        v = idx_msgs.astype(np.int64) - (1 << (p - 1))
        phases = (v.astype(np.uint64) << np.uint64(63 - p)) + (np.uint64(1) << np.uint64(62))
    else:
        phases = idx_msgs << np.uint64(63 - p)
    assert np.array_equal(phases, idx_msgs << np.uint64(63 - p))
    t = (idx_msgs + np.uint64((1 << (r - 1)) if r else 0)) >> np.uint64(r)
    want = np.where(t < 128, vals[tab_idx, np.minimum(t, 127).astype(np.int64)], -vals[tab_idx, 0])
    tier, bit = names.index("T6a"), ps.bit_tier
    wrong = 0
    for c0 in range(0, phases.size, 8192):
        sl = slice(c0, c0 + 8192)
        cts = keys.encrypt(phases[sl])
        if second == "T6a":
            out = keys.round_lut(bit, tier, cts, p, r, tables, 7, tab_idx[sl])
        else:
            out = keys.round_lut_split(bit, tier, names.index("T6"), cts, p, r, tables, 7, tab_idx[sl])
        got = np.round(_cent(keys.decrypt(out)) * 2.0 ** (64 - E_OUT)).astype(np.int64)
        wrong += int((got != want[sl]).sum())
    print(f"round_lut w=7 p={p} r={r} signed={signed} second={second}: {phases.size} ciphertexts, {wrong} mismatches")
    assert wrong == 0


@pytest.mark.parametrize("second", ["T6a", "T6"])
def test_split_site_output_noise_matches_model(full_keys, second):
    """what a split site leaves on its output is the sum of two bootstrap outputs: measured sigma within the band of
    tests/test_gpu_noise.py, [0.5x, 1.6x], of the compiler's figure sqrt(var_pbs_out(T6a) + var_pbs_out(second tier))"""
    from dctfhe import params as P
    ps, keys = full_keys
    names = [t.name for t in ps.tiers]
    rng = np.random.default_rng(5)
    vals = _tables(rng, True, ntab=1)
    msgs = rng.integers(0, 128, 4096).astype(np.uint64)
    cts = keys.encrypt(msgs << np.uint64(56))
    out = keys.round_lut_split(ps.bit_tier, names.index("T6a"), names.index(second), cts, 7, 0, vals << E_OUT, 7)
    want = (vals[0, msgs.astype(np.int64)] << E_OUT).astype(np.uint64)
    err = _cent(keys.decrypt(out) - want)
    assert np.abs(err).max() < 2.0 ** -9, "wrong outputs"
    model = math.sqrt(P.var_pbs_out(ps.tiers[names.index("T6a")], ps.fft_noise_c) + P.var_pbs_out(ps.tiers[names.index(second)], ps.fft_noise_c))
    measured = float(err.std())
    _record(f"lut7_split_sigma_{second}.json", {"tiers": "T6a+" + second, "log2_sigma_measured": math.log2(measured), "log2_sigma_model": math.log2(model)})
    assert 0.5 * model < measured < 1.6 * model, (math.log2(measured), math.log2(model))


def _oracle(qm, q):
    from oracle import circuit_ref
    out, ov = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not ov
    return qm.decode_output(out)


def _engine_counts(qm):
    st = qm.statistics()
    names = [t.name for t in qm.compiled.param_set.tiers]
    return {names[i]: int(st.pbs_count[i]) for i in range(len(names)) if st.pbs_count[i]}


def test_tiny_circuit_seven_bits():
    """the tiny ResNet of tests/test_gpu_circuit.py at rounding_threshold_bits=7 on the small rings: clear, simulate and encrypted runs
    equal the integer interpreter; a session run twice on one upload decrypts to the same outputs; the engine counts the bootstraps the
    compiler counts"""
    from dctfhe import compile as cc, models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    rng = np.random.default_rng(0)
    calib = rng.normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=7, param_set=P.test_params())
    try:
        sites = [o for o in qm.compiled.ops if o.type == cc.OP_LUT and cc.is_split(o)]
        assert sites
        assert _engine_counts(qm) == qm.compiled.pbs_counts()
        q = qm.quantize_input(calib[:6])
        want = _oracle(qm, q)
        assert np.array_equal(qm.forward_quantized(q, "disable"), want)
        assert np.array_equal(qm.forward_quantized(q, "simulate"), want)
        qm.fhe_circuit.keygen(seed=5)
        assert np.array_equal(qm.forward_quantized(q, "execute"), want)
        for B in (1, 3):                                                   # batches that do not fill a workgroup
            qb = qm.quantize_input(calib[10:10 + B])
            assert np.array_equal(qm.forward_quantized(qb, "execute"), _oracle(qm, qb))
        q3 = qm.quantize_input(calib[20:23])
        want3 = _oracle(qm, q3)
        sess = qm._session("execute", 3)
        sess.upload(qm._keys.encrypt(qm.encode_input(q3).reshape(-1)))
        for _ in range(2):
            sess.run()
            out = sess.download().reshape(-1, qm._keys.D + 1)
            assert np.array_equal(qm.decode_output(qm._keys.decrypt(out).reshape(3, -1)), want3)
    finally:
        qm.close()


def test_resnet20_5bit_seven_bits_bit_exact():
    """the reference's ImageNet setting on the full-size ResNet-20 24x16^2: bit_width=5, rounding_threshold_bits=7, default (5-bit exact)
    catalogue.  One encrypted image: all 64 outputs equal the integer interpreter's and so does the label; clear mode and simulate equal
    it too; a second run of the session on the same upload decrypts to the same outputs."""
    import warnings
    import bench
    from dctfhe import compile as cc, models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    factory, in_ch, img, make_batch, _ = bench.CONFIGS["r20_24_16"]
    model = getattr(models, factory)(bit_width=5, in_channels=in_ch, img_size=img, seed=0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        qm = compile_brevitas_qat_model(model, make_batch(100, 7), n_bits=5, rounding_threshold_bits=7)
    try:
        assert not [str(x.message) for x in caught if "exact-evaluation budget" in str(x.message)]
        c = qm.compiled
        assert c.worst_site_failure <= 1e-12 and sum(1 for o in c.ops if o.type == cc.OP_LUT and cc.is_split(o)) >= 20
        assert {o.ip[9] for o in c.ops if o.type == cc.OP_LUT and cc.is_split(o)} == {cc.LUT_SPLIT, cc.LUT_SPLIT_QUIET}
        assert _engine_counts(qm) == c.pbs_counts()
        q = qm.quantize_input(make_batch(1, 42))
        want = _oracle(qm, q)
        assert want.shape == (1, 64)
        assert np.array_equal(qm.forward_quantized(q, "disable"), want)
        assert np.array_equal(qm.forward_quantized(q, "simulate"), want)
        qm.fhe_circuit.keygen(seed=5)
        got = qm.forward_quantized(q, "execute")
        _record("lut7_r20_24_16_bw5_rtb7_execute.json", dict(qm.last_timing, images=1, pbs_per_image=c.pbs_counts(), worst_site=c.worst_site_failure))
        assert np.array_equal(got, want), np.argwhere(got != want)
        label = lambda o: int(np.argmax(o[0] * c.out_scale @ model.classifier_w.T + model.classifier_b))
        assert label(got) == label(want)
        sess = qm._session("execute", 1)          # the session forward_quantized used: its input is still resident
        sess.run()
        out_dim = sess.dims()[1]
        again = qm.decode_output(qm._keys.decrypt(sess.download(out_dim).reshape(-1, out_dim + 1), out_dim).reshape(1, -1))
        assert np.array_equal(again, want)
    finally:
        qm.close()


def _one_site_blob(table, n, mode):
    """a circuit of one look-up record: p = w = 7, no rounding, one table, [1, 1, n] elements"""
    head = struct.pack("<IIiiiiii", 0x46544344, 1, 2, 1, 0, 1, 7, 0)
    tens = struct.pack("<iiii", 1, 1, n, 0) * 2
    ip = [7, 0, 7, 0, 0, 1, 1, -1, 1, mode, 0, -1]
    off = len(head) + len(tens) + 96
    rec = struct.pack("<iiii12i2qqq", 4, 0, 0, 1, *ip, 0, 0, off, 128 * 8)
    return head + tens + rec + np.ascontiguousarray(table, np.int64).tobytes()


def test_simulate_samples_both_lookups(gpu_ctx):
    """`simulate` on a split site draws the noise at BOTH look-ups.  One-record circuit, 2^18 inputs, sigma handed in through
    dctfhe_session_set_noise: with sigma = 2^-8 / 3 each look-up leaves its half-box (2^-8: the boxes of a 6-bit table) with probability
    p1 = p_fail(2^-8, sigma^2) = erfc(3 / sqrt 2) = 2.70e-3 and then reads a neighbouring entry of S or Dt, which differs from the right
    one in these tables; the output deviates when either does: rate 1 - (1 - p1)^2 = 5.39e-3 -- a single sampled look-up would give
    2.70e-3, outside the band.  Asserted with a 3-sigma binomial band.  With the second look-up's own sigma (set_noise_split) the rate is
    1 - (1 - p1)(1 - p2).  sigma = 0 on the site: no deviation at all."""
    from dctfhe import params as P
    from dctfhe.engine import Circuit, Session
    rng = np.random.default_rng(9)
    n = 1 << 18
    # S and Dt strictly increasing and wider than each other's steps: a neighbour always differs and two failures cannot cancel
    s_half = np.cumsum(rng.integers(1, 4, 64)) * 1000
    d_half = np.cumsum(rng.integers(1, 4, 64))
    table = np.empty(128, np.int64)
    table[0::2], table[1::2] = s_half + d_half, s_half - d_half
    table <<= 20
    t = rng.integers(0, 128, n).astype(np.uint64)
    ph = (t << np.uint64(56)).reshape(1, n)
    circ = Circuit(gpu_ctx, _one_site_blob(table, n, 2))
    sess = Session(gpu_ctx, circ, None, 1)
    try:
        def run(sigma, sigma2=None, seed=1):
            sess.set_noise(seed, [sigma])
            sess.set_noise_split(None if sigma2 is None else [sigma2])
            sess.upload(ph)
            sess.run()
            return sess.download().reshape(-1).view(np.int64)
        want = table[t.astype(np.int64)]
        assert np.array_equal(run(0.0), want)                                       # noise-free: the plain 128-entry read
        sigma = 2.0 ** -8 / 3.0
        p1 = P.p_fail(2.0 ** -8, sigma ** 2)
        for sigma2, seed in ((None, 1), (2.0 ** -8 / 3.5, 2)):
            p2 = p1 if sigma2 is None else P.p_fail(2.0 ** -8, sigma2 ** 2)
            rate = 1.0 - (1.0 - p1) * (1.0 - p2)
            dev = int((run(sigma, sigma2, seed) != want).sum())
            band = 3.0 * math.sqrt(n * rate * (1.0 - rate))
            print(f"simulate split: {dev} deviations of {n}, expected {n * rate:.0f} +- {band:.0f} (one look-up alone: {n * p1:.0f})")
            assert abs(dev - n * rate) <= band, (dev, n * rate, band)
            assert abs(dev - n * p1) > band                                         # not the rate of a single sampled look-up
        assert not np.array_equal(run(sigma, None, 3), run(sigma, None, 4))         # fresh draws per seed
    finally:
        sess.close()
        circ.close()


def test_simulate_deviates_at_split_sites_only():
    """whole circuit (tiny ResNet, rounding_threshold_bits=7): sigmas inflated at the split sites only -> simulate leaves clear mode;
    inflated nowhere (the compiler's own figures on these rings, or zeros) -> it does not; the facade hands the split sites' second
    sigma to the engine"""
    from dctfhe import _lib, compile as cc, models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    rng = np.random.default_rng(0)
    calib = rng.normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=7, param_set=P.test_params())
    try:
        c = qm.compiled
        split = [i for i, o in enumerate(c.ops) if o.type == cc.OP_LUT and cc.is_split(o)]
        s2 = c.simulation_sigmas_split()
        assert split and all(s2[i] > c.ops[i].sim_sigma > 0 for i in split) and all(s2[i] == 0 for i in range(len(c.ops)) if i not in split)
        q = qm.quantize_input(calib[:16])
        clear = qm.forward_quantized(q, "disable")
        sess = qm._session("clear", 16)

        def run(sig, seed):
            sess.set_noise(seed, sig)
            sess.set_noise_split(None)
            sess.upload(qm.encode_input(q))
            sess.run()
            return qm.decode_output(sess.download().reshape(16, -1))
        # sigma = half-box / 2.5: each look-up of a split site reads a neighbouring entry with probability erfc(2.5 / sqrt 2) = 1.2 %.
        # A wrong entry may push a later accumulator out of its calibrated range, which the clear engine reports instead of wrapping
        # as an encrypted run would: that, too, is a deviation that only sampled noise can cause
        inflated = [2.0 ** -8 / 2.5 if i in split else 0.0 for i in range(len(c.ops))]
        try:
            deviates = not np.array_equal(run(inflated, 1), clear)
        except _lib.DctfheError as e:
            assert "left its padded range" in str(e)
            deviates = True
        assert deviates
        assert np.array_equal(run([0.0] * len(c.ops), 2), clear)
        others = [0.0 if i in split else s for i, s in enumerate(c.simulation_sigmas())]
        assert np.array_equal(run(others, 3), clear)
    finally:
        qm.close()


def test_cli_seven_bits_simulate():
    """homomorphic_eval.py with the reference's ImageNet rounding setting (--rounding_threshold_bits 7 --bit_width 5) runs; at the exact
    tiers the simulated accuracy equals the unencrypted one"""
    import re
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"), "--dataset", "cifar10", "--model", "ResNet20qat",
           "--dct_status", "--channels", "24", "--filter_size", "4", "--image_size_dct", "16", "--bit_width", "5", "--fhe_mode", "simulate",
           "--calib_batch_size", "32", "--test_batch_size", "2", "--test_subset", "4", "--rounding_threshold_bits", "7", "--n_bits", "5",
           "--p_error", "0.01"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(os.environ.get("TMPDIR", "/tmp")))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "exceeds the exact-evaluation budget" not in out.stderr, out.stderr[-2000:]
    for needle in ("Time for FHE compilation", "it works in FHE!!", "Encrypted Reliability Analysis Results", "Done"):
        assert needle in out.stdout, out.stdout
    plain = re.search(r"Unencrypted top1 acc: (.*)", out.stdout).group(1)
    enc = re.search(r"Encrypted top1 acc: (.*)", out.stdout).group(1)
    assert plain == enc
