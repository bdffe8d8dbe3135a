"""Margin audit, the CPU side: dctfhe_margin_probe_host -- the definition of the audit's statistic (include/dctfhe.h, DESIGN.md section
6) -- against its numpy statement in tests/margin_ref.py, exactly; and CompiledCircuit.margin_model(), the compiler's figure for every
slot the engine reports, against the ops it was recorded from.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import margin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from dctfhe import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _rows(rng, count, n, logN):
    """random 64-bit words; in the rows from the third on, a body and some mask words whose level rounds up to 2N (top bits all ones)"""
    rows = rng.integers(0, 2 ** 64, (count, n + 1), dtype=np.uint64)
    top = np.uint64(2 ** 64 - 1) << np.uint64(62 - logN)            # at least logN + 2 leading ones: level 2N
    rows[2::3, n] = top | rng.integers(0, 2 ** 20, rows[2::3, n].shape, dtype=np.uint64)
    rows[2::5, ::7] = top
    return rows


@pytest.mark.parametrize("logN", [8, 10, 13])
@pytest.mark.parametrize("n", [1, 40, 63, 64, 65, 200])
def test_host_probe_equals_numpy(L, n, logN):
    from dctfhe.engine import margin_probe_host
    rng = np.random.default_rng(1000 * logN + n)
    key = rng.integers(0, 2, n + 7).astype(np.uint8)                  # longer than n: only the first n bytes count
    for w in (0, 3, logN - 1):
        for count in (1, 5, 257):
            rows = _rows(rng, count, n, logN)
            if count >= 3:
                assert (margin_ref.levels(rows[2, n], logN) == 2 << logN)
            want = margin_ref.errors(key, n, logN, rows, w)
            err, st = margin_probe_host(key, n, logN, rows, w)
            assert err.dtype == np.int32 and np.array_equal(err, want), (n, logN, w, count)
            assert st == margin_ref.stats(want, logN, w), (n, logN, w, count)
            h = 1 << (logN - w - 1)
            assert want.min() >= -h and want.max() < h and sum(st["hist"]) == count
            # either output alone
            assert np.array_equal(margin_probe_host(key, n, logN, rows, w, want_stats=False)[0], want)
            assert margin_probe_host(key, n, logN, rows, w, want_err=False) == (None, st)


@pytest.mark.parametrize("w", [0, 3, 6])
@pytest.mark.parametrize("logN", [8, 10])
def test_trivial_rows_walk_the_boxes(L, logN, w):
    """zero mask, the body on each of the 2N levels: e is 0 at the centres (multiples of G = 2^(logN - w)), climbs to h - 1 and steps to
    -h exactly between two boxes"""
    from dctfhe.engine import margin_probe_host
    n, two_n = 5, 2 << logN
    G = 1 << (logN - w)
    h = G // 2
    lv = np.arange(two_n)
    err, st = margin_probe_host(np.ones(n, np.uint8), n, logN, margin_ref.trivial_rows(n, logN, lv), w)
    assert np.array_equal(err, margin_ref.errors(np.ones(n, np.uint8), n, logN, margin_ref.trivial_rows(n, logN, lv), w))
    assert np.array_equal(err, (lv + h) % G - h)
    assert np.all(err[lv % G == 0] == 0)
    drops = np.flatnonzero(np.diff(err) != 1)
    assert np.array_equal(drops, np.arange(h - 1, two_n - 1, G)) and np.all(err[drops] == h - 1) and np.all(err[drops + 1] == -h)
    assert st["count"] == two_n and st["max_abs"] == h and st["half_box"] == h and st["sum"] == -(two_n // G) * h
    assert st["hist"][15] >= two_n // G                                   # |e| = h lands in the last bin, not past it


def test_host_probe_refusals(L):
    from dctfhe._lib import ptr
    key = np.ones(8, np.uint8)
    rows = np.zeros((2, 9), np.uint64)
    err = np.zeros(2, np.int32)

    def fails(rc, needle):
        assert rc != 0
        assert needle in L.dctfhe_last_error().decode(), L.dctfhe_last_error().decode()

    fails(L.dctfhe_margin_probe_host(ptr(key), 8, 10, ptr(rows), 2, 10, ptr(err), None), "leaves no box")
    fails(L.dctfhe_margin_probe_host(ptr(key), 8, 10, ptr(rows), 2, 11, ptr(err), None), "leaves no box")
    fails(L.dctfhe_margin_probe_host(ptr(key), 8, 10, ptr(rows), 2, -1, ptr(err), None), "leaves no box")
    fails(L.dctfhe_margin_probe_host(ptr(key), 0, 10, ptr(rows), 2, 3, ptr(err), None), "0 mask words")
    fails(L.dctfhe_margin_probe_host(ptr(key), 8, 10, None, 2, 3, ptr(err), None), "null")
    fails(L.dctfhe_margin_probe_host(None, 8, 10, ptr(rows), 2, 3, ptr(err), None), "null")
    assert L.dctfhe_margin_probe_host(ptr(key), 8, 10, None, 0, 3, None, None) == 0      # nothing to probe is not an error
    assert L.dctfhe_margin_probe_host(ptr(key), 8, 10, ptr(rows), 2, 9, ptr(err), None) == 0 and not err.any()


# ------------------------------------------------------------------------------------------ the compiler's side
def _circuits():
    from dctfhe import compile as cc, models, params as P
    rng = np.random.default_rng(0)
    yield "tiny", cc.compile_model(models.tiny_resnet_q(), rng.normal(0, 1, (32, 4, 6, 6)), rounding_threshold_bits=6, n_bits=5,
                                   param_set=P.test_params())
    # the parity-split recipe of tests/test_lut7_host.py
    yield "split", cc.compile_model(models.tiny_resnet_q(), np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6)), rounding_threshold_bits=7,
                                    param_set=P.test_params())
    yield "pool", cc.compile_model(models.tiny_resnet_q(pool1=(3, 2, 1)), np.random.default_rng(3).normal(0, 1, (20, 4, 6, 6)), n_bits=5,
                                   param_set=P.test_params())


@pytest.mark.parametrize("which", ["tiny", "split", "pool"])
def test_margin_model_lists_every_decision(which):
    from dctfhe import compile as cc, params as P
    c = dict(_circuits())[which]
    ps = c.param_set
    blob, report = c.blob, c.report()
    mm = c.margin_model()
    assert c.blob == blob and c.report() == report and c.margin_model() == mm      # a pure view
    names = [t.name for t in ps.tiers]
    per_tier, by_op = {}, {}
    for m in mm:
        by_op.setdefault(m["op"], []).append(m)
        per_tier[m["tier_name"]] = per_tier.get(m["tier_name"], 0) + m["elements"]
        assert m["tier_name"] == names[m["tier"]] and m["sigma"] > 0 and m["note"] == c.ops[m["op"]].note
        assert ps.tiers[m["tier"]].logN - m["table_bits"] >= 1
    assert list(by_op) == [i for i, o in enumerate(c.ops) if o.type in (cc.OP_LUT, cc.OP_MAXPOOL)]      # circuit order, every site
    parity = {}
    for i, o in enumerate(c.ops):
        if o.type == cc.OP_MAXPOOL:
            (m,) = by_op[i]
            assert (m["kind"], m["tier"], m["table_bits"], m["elements"], m["entry"]) == ("pool", o.ip[4], o.ip[5], o.n_max, 0)
            assert m["sigma"] >= o.sim_sigma                      # the worst level, not the last
        elif o.type == cc.OP_LUT:
            s = c.tensors[o.src0]
            n = s.C * s.H * s.W
            want = [(f"step {k}", cc.step_tier(o, k), 0) for k in range(cc.chain_steps(o))]
            if cc.is_split(o):
                want.append(("second", cc.second_tier(ps, o), o.w - 1))
                nm = names[cc.step_tier(o, o.r)]
                parity[nm] = parity.get(nm, 0) + n
            want.append(("table", o.ip[4], o.w - 1 if cc.is_split(o) else o.w))
            assert [(m["kind"], m["tier"], m["table_bits"]) for m in by_op[i]] == want
            assert [m["entry"] for m in by_op[i]] == list(range(len(want))) and all(m["elements"] == n for m in by_op[i])
            # the figures are the ones the site was priced with
            assert by_op[i][-1]["sigma"] == o.sim_sigma
            if cc.is_split(o):
                assert by_op[i][-2]["sigma"] == o.sim_sigma2
            half = lambda m: 2.0 ** -(m["table_bits"] + 2)
            assert abs(sum(P.p_fail(half(m), m["sigma"] ** 2) for m in by_op[i]) - o.pfail) <= 1e-9 * o.pfail + 1e-300
    # every bootstrap but the parity ones has a key switch of its own, hence a slot
    counts = c.pbs_counts()
    assert per_tier == {k: v - parity.get(k, 0) for k, v in counts.items() if v - parity.get(k, 0)}
    if which == "split":
        assert parity and any(m["kind"] == "second" for m in mm)
    if which == "pool":
        assert sum(m["kind"] == "pool" for m in mm) == 1


def test_exports_and_struct_layout(L):
    from dctfhe import _lib
    assert C.sizeof(_lib.MarginStats) == 6 * 4 + 3 * 8 + 16 * 8
    for name in ("dctfhe_margin_probe_host", "dctfhe_margin_probe", "dctfhe_session_set_audit", "dctfhe_session_audit"):
        assert name in _lib.EXPORTS and hasattr(L, name)
