"""Margin audit on the GPU (include/dctfhe.h): k_margin_probe against its host twin bit for bit; the definition pinned
to the shipped bootstrap kernels on trivial ciphertexts at every level; the session's slots against the compiler's margin_model() on the
tiny trunks; and the model check itself -- measured sigma at the point of decision against the figure _estimate_noise priced."""
import ctypes as C
import math

import numpy as np
import pytest

import margin_ref

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 5, 257, 4099)      # a partial block, one block, two, several, and a tail of the grid-stride loop (the grid is capped at 1024)


def _oracle_out(qm, q):
    from oracle import circuit_ref
    out, ov = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not ov
    return qm.decode_output(out)


def _sigma(slot, logN):
    return math.sqrt(slot["sum_sq"] / slot["count"]) / (2 << logN)


# ------------------------------------------------------------------------------------------ the primitive
@pytest.fixture(scope="module")
def probe_keys(gpu_ctx):
    """the tiny rings (n = 48 at logN 10; n = 40, k = 2 at logN 8: both below one wave) and a set of its own with n = 200"""
    from dctfhe import params as P
    from dctfhe.engine import Keys, make_params
    ps = P.test_params()
    tiny = Keys(gpu_ctx, P.to_c_params(ps), seed=11)
    wide = Keys(gpu_ctx, make_params(1024, 200, [dict(n=200, k=1, logN=9, l=2, beta=12, lk=4, betak=4, lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -45)],
                                     2.0 ** -50), seed=13)
    yield {"tiny": tiny, "wide": wide}
    tiny.close()
    wide.close()


@pytest.mark.parametrize("which,tier,w", [("tiny", 0, 3), ("tiny", 0, 6), ("tiny", 1, 0), ("tiny", 1, 2), ("wide", 0, 4)])
def test_probe_equals_host_twin(probe_keys, which, tier, w):
    from dctfhe.engine import margin_probe_host
    keys = probe_keys[which]
    t = keys.tier(tier)
    rng = np.random.default_rng(17 + 10 * tier + w)
    msgs = rng.integers(0, 1 << w, max(COUNTS)).astype(np.uint64) if w else rng.integers(0, 2, max(COUNTS)).astype(np.uint64)
    small = keys.modswitch_center(tier, keys.keyswitch(tier, keys.encrypt(msgs << np.uint64(63 - w))))
    _, s = keys.export_secret()
    for count in COUNTS:
        rows = small[:count]
        want_err, want = margin_probe_host(s, t.n, t.logN, rows, w)
        assert np.array_equal(want_err, margin_ref.errors(s, t.n, t.logN, rows, w))
        want["tier"] = tier
        err, st = keys.margin_probe(tier, rows, w)
        assert np.array_equal(err, want_err), (count, np.flatnonzero(err != want_err)[:8])
        assert st == want, (count, st, want)
        err_only, no_stats = keys.margin_probe(tier, rows, w, want_stats=False)              # stats == NULL
        assert no_stats is None and np.array_equal(err_only, want_err)
        assert keys.margin_probe(tier, rows, w, want_err=False) == (None, want)              # err == NULL
    # fresh encryptions of box centres: the distance IS the noise, far inside the half-box
    assert st["max_abs"] < st["half_box"] and st["sum_sq"] > 0
    # ... and random words (every level, the ones that round up to 2N too) through the kernel's whole range
    wild = rng.integers(0, 2 ** 64, (257, t.n + 1), dtype=np.uint64)
    wild[::3, t.n] = np.uint64(2 ** 64 - 1)
    wild[::5, ::3] = np.uint64(2 ** 64 - 1) << np.uint64(62 - t.logN)
    err, st = keys.margin_probe(tier, wild, w)
    assert np.array_equal(err, margin_ref.errors(s, t.n, t.logN, wild, w))
    assert st == margin_ref.stats(err, t.logN, w, tier=tier)


@pytest.mark.parametrize("tier,w", [(0, 3), (0, 6), (1, 0)])
def test_grid_pinned_to_the_shipped_bootstrap(probe_keys, tier, w):
    """trivial small ciphertexts at all 2N body levels through dctfhe_pbs with distinct table entries and through the probe: the
    bootstrap's decrypted entry changes between two consecutive levels exactly where e steps from h - 1 to -h"""
    keys = probe_keys["tiny"]
    t = keys.tier(tier)
    two_n = 2 << t.logN
    h = 1 << (t.logN - w - 1)
    rows = margin_ref.trivial_rows(t.n, t.logN, np.arange(two_n))
    table = (np.arange(1 << w, dtype=np.int64) + 1) << np.int64(56)           # distinct, and distinct from their negations
    out = keys.decrypt(keys.pbs(tier, rows, table, w))
    entry = np.round(out.astype(np.int64).astype(np.float64) / 2.0 ** 56).astype(np.int64)
    assert set(np.abs(entry)) == set(range(1, (1 << w) + 1))
    err, st = keys.margin_probe(tier, rows, w)
    assert np.all(err[np.arange(two_n) % (2 * h) == 0] == 0)
    nxt = np.roll(np.arange(two_n), -1)                                       # the wrap 2N - 1 -> 0 included
    changes = np.flatnonzero(entry != entry[nxt])
    drops = np.flatnonzero((err == h - 1) & (err[nxt] == -h))
    assert np.array_equal(np.flatnonzero(err[nxt] != err + 1), drops)         # e climbs by one level everywhere else
    # (the box around level N reads -T[0] from both sides of the negacyclic seam: one box like the others)
    assert np.array_equal(changes, drops)
    assert st["count"] == two_n and st["max_abs"] == h


# ------------------------------------------------------------------------------------------ sessions
def _tiny_qm(kind):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    if kind == "pool":         # tests/test_gpu_maxpool.py's pooled trunk
        calib = np.random.default_rng(3).normal(0, 1, (24, 4, 9, 9))
        return compile_brevitas_qat_model(models.tiny_resnet_q(img_size=9, pool1=(3, 2, 1)), calib[:20], n_bits=5, rounding_threshold_bits=6,
                                          param_set=P.test_params()), calib
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    return compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=7 if kind == "split" else 6,
                                      param_set=P.test_params()), calib


def _check_slots(qm, slots, batch, assert_model, label):
    """the slot list against margin_model() and dctfhe_circuit_stats; the ratios measured / modelled are printed, and asserted at 1.3x
    from above where assert_model says so"""
    ps = qm.compiled.param_set
    model = qm.compiled.margin_model()
    key = lambda r: (r["op"], r["entry"], r["tier"], r["table_bits"])
    assert [key(s) for s in slots] == [key(m) for m in model]
    per_tier = {}
    for s, m in zip(slots, model):
        assert s["count"] == m["elements"] * batch, (s, m)
        assert s["half_box"] == 1 << (ps.tiers[s["tier"]].logN - s["table_bits"] - 1)
        assert sum(s["hist"]) == s["count"] and s["max_abs"] < s["half_box"] and s["sum_sq"] > 0, s
        per_tier[s["tier"]] = per_tier.get(s["tier"], 0) + s["count"]
    st = qm.statistics()
    assert per_tier == {i: st.ks_count[i] * batch for i in range(len(ps.tiers)) if st.ks_count[i]}
    ratios = [(m["op"], m["kind"], m["tier_name"], s["count"], round(_sigma(s, ps.tiers[s["tier"]].logN) / m["sigma"], 3)) for s, m in zip(slots, model)]
    print(f"margin audit {label}: (op, kind, tier, count, measured / modelled sigma)", ratios)
    if assert_model:
        over = [r for r in ratios if r[3] >= 256 and r[4] > 1.3]
        assert not over, over
    return ratios


def test_session_tiny_trunk():
    from dctfhe.engine import MarginStats
    qm, calib = _tiny_qm("exact")
    try:
        qm.fhe_circuit.keygen(seed=5)
        q = qm.quantize_input(calib[:2])
        want = _oracle_out(qm, q)
        off = qm.forward_quantized(q, "execute")
        on, report = qm.audit_quantized(q)
        assert np.array_equal(off, want) and np.array_equal(on, want)
        assert report.worst() is not None and report.worst()["z"] == min(r["z"] for r in report.rows) and "narrowest decision" in report.text()
        assert all(r["note"] == qm.compiled.ops[r["op"]].note for r in report.rows)
        # the session by hand: slots, a second run, and off again
        sess = qm._session("execute", 2)
        L, n = sess.L, C.c_int(-1)
        assert sess.audit() == []                                             # audit_quantized turned it off again
        sess.set_audit(qm._keys)
        sess.upload(qm._keys.encrypt(qm.encode_input(q).reshape(-1)))
        sess.run()
        slots = sess.audit()
        _check_slots(qm, slots, 2, True, "tiny trunk, tiny rings")
        assert len(report.rows) == len(slots) and [r["count"] for r in report.rows] == [s["count"] for s in slots]
        out1 = sess.download()
        sess.run()
        again = sess.audit()
        assert [s["count"] for s in again] == [s["count"] for s in slots]     # zeroed at every run, not doubled
        assert again == slots                                                 # same input, same integer statistics
        assert np.array_equal(sess.download(), out1)
        assert L.dctfhe_session_audit(sess.h, None, 0, C.byref(n)) == 0 and n.value == len(slots)
        one = (MarginStats * 1)()
        assert L.dctfhe_session_audit(sess.h, one, 1, C.byref(n)) != 0 and "room for 1 slots" in L.dctfhe_last_error().decode()
        sess.set_audit(None)
        sess.run()
        assert np.array_equal(sess.download(), out1)
        assert L.dctfhe_session_audit(sess.h, None, 0, C.byref(n)) == 0 and n.value == 0 and sess.audit() == []
        assert np.array_equal(qm.decode_output(qm._keys.decrypt(out1.reshape(-1, qm._keys.D + 1)).reshape(2, -1)), want)
    finally:
        qm.close()


@pytest.mark.parametrize("kind", ["split", "pool"])
def test_session_other_circuits(kind):
    from dctfhe import compile as cc
    qm, calib = _tiny_qm(kind)
    try:
        qm.fhe_circuit.keygen(seed=5)
        q = qm.quantize_input(calib[20:22])
        out, report = qm.audit_quantized(q)
        assert np.array_equal(out, _oracle_out(qm, q))
        _check_slots(qm, report.rows, 2, True, f"{kind} trunk, tiny rings")      # a report row keeps its slot's fields
        kinds = [r["kind"] for r in report.rows]
        if kind == "split":
            sites = [i for i, o in enumerate(qm.compiled.ops) if o.type == cc.OP_LUT and cc.is_split(o)]
            assert sites and kinds.count("second") == len(sites)
            for i in sites:          # steps, second, table -- and nothing for the parity bootstrap
                o = qm.compiled.ops[i]
                mine = [r for r in report.rows if r["op"] == i]
                assert [r["kind"] for r in mine] == [f"step {k}" for k in range(o.r + 1)] + ["second", "table"]
                assert mine[-2]["tier"] == cc.second_tier(qm.compiled.param_set, o) and mine[-2]["table_bits"] == o.w - 1
        else:
            (pool,) = [o for o in qm.compiled.ops if o.type == cc.OP_MAXPOOL]
            (row,) = [r for r in report.rows if r["kind"] == "pool"]
            assert row["count"] == pool.n_max * 2 and row["table_bits"] == pool.ip[5]
    finally:
        qm.close()


def test_slot_accumulates_over_chunks():
    """a site larger than the session's look-up chunk (16 384 ciphertexts): its slot is the sum over both chunks"""
    qm, calib = _tiny_qm("exact")
    try:
        biggest = max(m["elements"] for m in qm.compiled.margin_model())
        batch = 16384 // biggest + 1
        assert biggest * (batch - 1) <= 16384 < biggest * batch
        qm.fhe_circuit.keygen(seed=5)
        q = np.concatenate([qm.quantize_input(calib)] * (batch // calib.shape[0] + 1))[:batch]
        out, report = qm.audit_quantized(q)
        assert np.array_equal(out, _oracle_out(qm, q))
        assert [r["count"] for r in report.rows] == [m["elements"] * batch for m in qm.compiled.margin_model()]
        assert max(r["count"] for r in report.rows) > 16384 and all(r["max_abs"] < r["half_box"] for r in report.rows)
    finally:
        qm.close()


# ------------------------------------------------------------------------------------------ the model check
def test_model_holds_on_the_default_catalogue():
    """One key generation on the default catalogue.  Primitive: 4 096 fresh ciphertexts, key-switched and centred on T6a (w = 6) and Ba2
    (w = 0): the probe's sigma within [0.7x, 1.3x] -- the band tests/test_gpu_noise.py applies to the key switch -- of
    sqrt(input_sigma^2 + var_keyswitch + var_modswitch).  Then the tiny trunk compiled on this catalogue: every slot with at least 256
    decisions measures at most 1.3x its margin_model() sigma (the model bounds the convolution gain from above, and above is the
    direction that threatens exactness).  Two images: with one, no site of the tiny trunk (216 elements at most) reaches 256."""
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6)
    try:
        ps = qm.compiled.param_set
        assert [t.name for t in ps.tiers] == [t.name for t in P.default_params().tiers]
        qm.fhe_circuit.keygen(seed=7)
        keys = qm._keys
        names = [t.name for t in ps.tiers]
        rng = np.random.default_rng(4)
        deff = ps.input_dim or ps.D
        for name, w in (("T6a", 6), ("Ba2", 0)):
            ti = names.index(name)
            t = ps.tiers[ti]
            msgs = rng.integers(0, 1 << w, 4096).astype(np.uint64) if w else rng.integers(0, 2, 4096).astype(np.uint64)
            small = keys.modswitch_center(ti, keys.keyswitch(ti, keys.encrypt(msgs << np.uint64(63 - w)), deff=deff))
            _, st = keys.margin_probe(ti, small, w, want_err=False)
            measured = _sigma(st, t.logN)
            model = math.sqrt(ps.input_sigma ** 2 + P.var_keyswitch(deff, t) + P.var_modswitch(t))
            print(f"margin probe {name}: log2 sigma measured {math.log2(measured):.2f}, model {math.log2(model):.2f}, ratio {measured / model:.3f}, "
                  f"max|e| / half_box {st['max_abs'] / st['half_box']:.3f}")
            assert st["count"] == 4096 and st["max_abs"] < st["half_box"]
            assert 0.7 * model < measured < 1.3 * model, (name, measured, model)
        q = qm.quantize_input(calib[:2])
        out, report = qm.audit_quantized(q)
        assert np.array_equal(out, _oracle_out(qm, q))
        print(report.text())
        assert any(r["count"] >= 256 for r in report.rows)
        over = [(r["op"], r["kind"], r["tier_name"], r["count"], r["ratio"]) for r in report.rows if r["count"] >= 256 and r["ratio"] > 1.3]
        assert not over, over
        assert all(r["max_abs"] < r["half_box"] for r in report.rows)
    finally:
        qm.close()
