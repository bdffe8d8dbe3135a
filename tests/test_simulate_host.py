"""The numpy twin of `simulate` (tests/simulate_ref.py) held to the definition and to the noise model, on the host (no GPU): with every
sigma at 0 it is the noise-free interpreter; its draws have the model's moments and flip a 6-bit box at the closed-form rate; the guard
that the device comparison (tests/test_gpu_simulate.py) stands on is measured against long double, and no draw of a committed
(case, seed) lies inside it; no two noisy passes of any op and run share a generator stream."""
import json
import math
import os

import numpy as np
import pytest

import simulate_cases as SC
import simulate_ref as R
from oracle import circuit_ref

U = np.uint64
OUT = os.environ.get("DCTFHE_MEASURE_DIR")      # measurements are printed; when set, they are also written there as JSON
_MEASURED = {}


def _record(fname, obj):
    if OUT:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, fname), "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)


def _tiny(kind):
    from dctfhe import compile as cc, models, params as P
    if kind == "pooled":
        import test_maxpool_host
        c, calib = test_maxpool_host._pooled((3, 2, 1), 9)
    else:
        calib = np.random.default_rng(0).normal(0, 1, (24, 4, 6, 6))
        c = cc.compile_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=7 if kind == "split" else 6, param_set=P.test_params())
    q = cc.act_quant(calib[:4], c.in_scale, True, c.in_bits)
    return c, (q.astype(np.int64).astype(np.uint64) << U(c.e_in)).reshape(4, -1)


@pytest.mark.parametrize("kind", ["resnet", "pooled", "split"])
def test_sigma_zero_is_the_clear_circuit(kind):
    """every tensor and the overflow flag; sigmas absent, and zeros with the noise switched on at one levelled op's slot only"""
    from dctfhe import compile as cc
    c, ph = _tiny(kind)
    if kind == "split":
        assert any(o.type == cc.OP_LUT and cc.is_split(o) for o in c.ops)
    if kind == "pooled":
        assert any(o.type == cc.OP_MAXPOOL for o in c.ops)
    want, flag = circuit_ref.run_clear(c.blob, ph, all_tensors=True)
    for sig in (None, [0.0] * len(c.ops)):
        got, ov = R.run_simulate(c.blob, ph, 5, sig, sig, run=3, all_tensors=True)
        assert ov == flag and not ov
        assert sorted(got) == sorted(want) and all(np.array_equal(got[t], want[t]) for t in want)
    out, ov = R.run_simulate(c.blob, ph, 5, None)
    assert np.array_equal(out, circuit_ref.run_clear(c.blob, ph)[0])


@pytest.mark.parametrize("prw,mode", [((8, 2, 6), 0), ((7, 3, 4), 1), ((7, 0, 7), 2)])
def test_sigma_zero_one_site_with_overflow(prw, mode):
    """messages under the padding bit and beyond it: the interpreter's outputs and its flag"""
    shift, body_add = SC.SITES[prw]
    rng = np.random.default_rng(1)
    tables = rng.integers(-(1 << 62), 1 << 62, (1, 1 << prw[2]), dtype=np.int64) << 1
    blob = R.chain_blob((1, 1, SC.N_SITE), [R.lut_record(*prw, shift, mode, tables, body_add)])
    for inside in (True, False):
        ph = SC.site_inputs(prw[0], prw[1], shift, body_add, rng, inside)
        want, flag = circuit_ref.run_clear(blob, ph)
        got, ov = R.run_simulate(blob, ph, 1, [0.0])
        assert flag == (not inside) and ov == flag and np.array_equal(got, want)


@pytest.mark.parametrize("sigma", [2.0 ** -30, 2.0 ** -8])
def test_draws_have_the_models_moments(sigma):
    """2^18 draws: rint of a Gaussian of std sigma 2^64 has variance (sigma 2^64)^2 + 1/12; the mean within 4 standard errors of 0, the
    sample variance within 4 of its own (sqrt(2 / n) of it)"""
    n = 1 << 18
    d = R.gauss(11, 77, np.arange(n), sigma).astype(np.float64)
    var = (sigma * 2.0 ** 64) ** 2 + 1.0 / 12.0
    print(f"sigma 2^{math.log2(sigma):.0f}: mean / std {d.mean() / math.sqrt(var):+.2e}, variance / model {d.var() / var:.5f}")
    assert abs(d.mean()) <= 4.0 * math.sqrt(var / n)
    assert abs(d.var() - var) <= 4.0 * var * math.sqrt(2.0 / n)
    assert np.array_equal(R.gauss(11, 77, np.arange(100), 0.0), np.zeros(100, np.int64))
    assert not np.array_equal(d[:64], R.gauss(11, 78, np.arange(64), sigma)) and not np.array_equal(d[:64], R.gauss(12, 77, np.arange(64), sigma))


def test_flip_rate_of_an_exact_site():
    """one exact 6-bit site, sigma a third of its half-box 2^-8: an element reads a neighbouring entry with probability
    p_fail(2^-8, sigma^2) = erfc(3 / sqrt 2); 2^18 elements, 3-sigma binomial band.  The entries are pairwise distinct."""
    from dctfhe import params as P
    n, rng = 1 << 18, np.random.default_rng(2)
    table = rng.permutation(64).astype(np.int64).reshape(1, 64) << 50
    x = (rng.integers(0, 64, (1, 1, 1, n)).astype(np.uint64)) << U(57)
    sigma = 2.0 ** -8 / 3.0
    y, ov = R.lut_site(x, 6, 0, 6, 0, 0, 0, table.view(np.uint64), 3, R.lut_stream(0, 0), sigma)
    quiet, _ = R.lut_site(x, 6, 0, 6, 0, 0, 0, table.view(np.uint64), 3, R.lut_stream(0, 0), 0.0)
    rate = P.p_fail(2.0 ** -8, sigma ** 2)
    dev, band = int((y != quiet).sum()), 3.0 * math.sqrt(n * rate * (1.0 - rate))
    print(f"twin, exact 6-bit site: {dev} flips of {n}, expected {n * rate:.0f} +- {band:.0f}")
    assert not ov and abs(dev - n * rate) <= band


def test_reduced_draw_is_the_identity_below_half():
    """x - rint(x) changes nothing while |g sigma| < 1/2: the draws of key material and encryptions (sigma <= 2^-20) are what they were"""
    idx = np.arange(1 << 14)
    g = R._normal(4, 9, idx, np.float64)
    for sigma in (2.0 ** -20, 2.0 ** -4, 0.05):
        assert (np.abs(g * sigma) < 0.5).all()
        assert np.array_equal(R.gauss(4, 9, idx, sigma), np.rint(g * sigma * 2.0 ** 64).astype(np.int64))
    with pytest.raises(AssertionError, match="half the torus"):
        R.gauss(4, 9, np.arange(1 << 17), 0.125)


@pytest.mark.parametrize("name", list(SC.BUILDERS))
def test_guard_and_near_edge(name):
    """per committed (case, seed): the largest |float64 draw - long-double draw| over the draws the case uses, the guard G = 256 times
    that (at least 2^16 units of 2^-64), and NO element whose noisy position lies within G of a box edge or of the sign flip -- the
    condition under which the device comparison is exact equality.  (A case that fails here gets another seed in simulate_cases.SEEDS.)"""
    case = SC.get(name)
    runs, trace = case.twin()
    diff = R.draw_difference(case.seed, trace)
    G = R.guard(case.seed, trace)
    close = R.near_edge(trace, G)
    _MEASURED[name] = dict(seed=case.seed, draws=trace.draws(), max_draw_difference=diff, guard=G, near_edge=len(close),
                           sigmas=sorted({r["sigma"] for r in trace.records}))
    print(name, _MEASURED[name])
    _record("simulate_twin.json", dict(unit="2^-64 of the torus", guard_margin=R.GUARD_MARGIN, guard_min=R.GUARD_MIN, cases=_MEASURED))
    assert G >= R.GUARD_MIN and G == max(R.GUARD_MIN, R.GUARD_MARGIN * diff)
    assert close == [], close[:5]
    if case.inside is not None:
        assert [ov for _, ov in runs] == [not i for i in case.inside]
    wraps = sum(int((np.abs(R._normal(case.seed, r["stream"], r["idx"], np.float64) * r["sigma"]) >= 0.5).sum()) for r in trace.records)
    assert (wraps > 0) == (name == SC.WRAP_CASE), wraps      # the twin asserts |g sigma| < 1/2 everywhere else


def test_noise_bites_where_it_should():
    """the cases at 2^-4 and 1/32 move words, the ones at 2^-40 move none: the quiet pools equal the signed maximum"""
    for name in SC.BUILDERS:
        case = SC.get(name)
        if not (name.startswith("pool-") or name.startswith("site-")) or case.allow_wrap:
            continue
        (vals, _), = [case.twin()[0][0]]
        clear = circuit_ref.run_clear(case.blob, case.runs[0], all_tensors=True)[0]
        out = max(vals)
        # (a site's on-grid half: off the grid an approximate site rounds m + f + 1/2, the clear circuit m, whatever the noise)
        on_grid = slice(0, SC.N_SITE // 2) if name.startswith("site-") else slice(None)
        moved = int((vals[out].reshape(-1)[on_grid] != clear[out].reshape(-1)[on_grid]).sum())
        if name.endswith("-quiet") or 2.0 ** -40 in case.sigmas:
            assert moved == 0, (name, moved)
        elif case.sigmas[0] >= 1.0 / 32 and "1x9" not in name and "9x1" not in name:
            assert moved > 0, name


def test_streams_are_pairwise_distinct():
    """look-up ops, pool row passes and pool column passes for runs R < 16, over the ops of the longest circuit the suite compiles (the
    ResNet-20 trunk of bench.py: 88 ops) -- and over every slot the 12-bit op field of the stream id has, which that circuit must fit
    in; none meets a key-material stream"""
    import bench
    from dctfhe import compile as cc, models
    factory, in_ch, img, make_batch, _ = bench.CONFIGS["r20_24_16"]
    c = cc.compile_model(getattr(models, factory)(in_channels=in_ch, img_size=img), make_batch(8, 7))
    n_ops = 1 << 12
    assert 80 <= len(c.ops) <= n_ops
    ids = [R.lut_stream(run, i) for run in range(16) for i in range(n_ops)]
    ids += [s for run in range(16) for i in range(n_ops) for s in R.pool_streams(run, i)]
    assert len(set(ids)) == len(ids)
    assert min(ids) > (1 << 20)      # STREAM_* of csrc/kernels.h end at 256 + the encryption counter
