"""One case per bootstrap kernel launch_pbs (csrc/dctfhe.hip) can dispatch: the 17 PBS_CASES, the paired two-bit kernels at
N = 2048 / 4096 / 8192 and the two general two-bit forms -- 22 pbs_kernel instantiations, each with its own ciphertexts per workgroup,
LDS layout, twist source and L2 warm-up.  Every case takes a short key (n = 40, D = k N, key noise far below the transform error) and
checks
  (a) a sweep of the rotation amount on the level grid (no input noise: every table width is legal) against the oracle's test vector,
      for the narrowest, a middle and the widest table, three tables picked per ciphertext, odd counts (partial last workgroups);
  (b) 65 noisy ciphertexts against the oracle's bootstrap of the same inputs under the same key: decoded values, the rms of the
      difference and the largest error;
  (c) that a ciphertext's result does not depend on its place in a launch: shuffled and alone, bit for bit the rows of (b).
On the first 37 inputs of (b), through dctfhe_pbs_rows, the write-back modes in which the library itself launches these kernels (the one-bit
steps, the parity bootstrap, a max pool's maxima, the chunks and shards of a site); exact, resting on (c):
  (d) store mode: the rows of (b); and into rows of D + 3 mask words between two guard rows, over garbage, with a body offset: the ring's
      words and the body as in (b) plus the offset, zeros between the ring and the body, the guard rows untouched;
  (e) accumulate mode at both widths, once and again on its own output: added on the ring's words and the body (the offset each time), the
      words in between and the guard rows untouched -- the padded groups of the partial last workgroup accumulate nowhere; and, not
      through store mode, onto fresh encryptions of known phases: every phase is the sum, within the model's bound plus six input sigmas;
  (f) per-channel tables, table ((e_offset + c) / hw) % nchan, at an offset below and one beyond 2^32, against the explicit index.
The bounds are the project's noise model at these shapes (tests/pbs_matrix_ref.py); nothing is taken from the kernels under test.
The model was calibrated at n = 560 .. 856 (tests/test_gpu_noise.py); the measured ratios are printed and, with DCTFHE_MEASURE_DIR set,
written to pbs_matrix.json (profiles/pbs_matrix.json is such a run)."""
import json
import math
import os
import re

import numpy as np
import pytest

import pbs_matrix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DCTFHE_MEASURE_DIR")

# (logN, k, l, unroll, beta).  beta: the shipped value where a catalogue of dctfhe/params.py has the shape (Ba / Ba2 / T4 23; T5a / T6a 22;
# B 14; F5 / F6 16; T4r / T4r2 12; T6 11; T5r 10); otherwise that of the nearest shipped shape with the same k and l (N = 4096 three
# levels takes T6's 11: the transform error grows with N^2 B^2).
PBS_MATRIX = [
    pytest.param(8, 2, 2, 1, 14, id="N256-k2-l2-u1"),
    pytest.param(9, 1, 2, 1, 16, id="N512-k1-l2-u1"),
    pytest.param(9, 1, 3, 1, 12, id="N512-k1-l3-u1"),
    pytest.param(10, 1, 1, 1, 23, id="N1024-k1-l1-u1"),
    pytest.param(10, 1, 2, 1, 16, id="N1024-k1-l2-u1"),
    pytest.param(10, 2, 1, 1, 23, id="N1024-k2-l1-u1"),
    pytest.param(10, 2, 2, 1, 14, id="N1024-k2-l2-u1"),
    pytest.param(11, 1, 1, 1, 23, id="N2048-k1-l1-u1"),
    pytest.param(11, 1, 2, 1, 16, id="N2048-k1-l2-u1"),
    pytest.param(11, 1, 3, 1, 12, id="N2048-k1-l3-u1"),
    pytest.param(11, 1, 4, 1, 10, id="N2048-k1-l4-u1"),
    pytest.param(12, 1, 1, 1, 22, id="N4096-k1-l1-u1"),
    pytest.param(12, 1, 2, 1, 16, id="N4096-k1-l2-u1"),
    pytest.param(12, 1, 3, 1, 11, id="N4096-k1-l3-u1"),
    pytest.param(13, 1, 1, 1, 22, id="N8192-k1-l1-u1"),
    pytest.param(13, 1, 2, 1, 16, id="N8192-k1-l2-u1"),
    pytest.param(13, 1, 3, 1, 11, id="N8192-k1-l3-u1"),
    pytest.param(11, 1, 1, 2, 23, id="N2048-k1-l1-u2"),
    pytest.param(12, 1, 1, 2, 22, id="N4096-k1-l1-u2"),
    pytest.param(13, 1, 1, 2, 22, id="N8192-k1-l1-u2"),
    pytest.param(11, 1, 3, 2, 12, id="N2048-k1-l3-u2"),
    pytest.param(10, 2, 1, 2, 23, id="N1024-k2-l1-u2"),
]
# the same kernels on a big key twice the ring: the mask words beyond k N must come back zero
PBS_WIDE = [pytest.param(9, 1, 2, 1, 16, id="N512-k1-l2-u1-D1024")]

N_SMALL, HOST_BYTES = 40, 128 << 20
MEASURED = {}


def _tier(logN, k, l, unroll, beta):
    glwe = 2.0 ** (-62 if logN >= 12 else -52)
    return dict(n=N_SMALL, k=k, logN=logN, l=l, beta=beta, lk=4, betak=4, lwe_sigma=2.0 ** -24, glwe_sigma=glwe, unroll=unroll)


def _dec(ph):
    """4-bit signed entries at 2^57: the entry and its negation, mod 128"""
    return ((ph + (np.uint64(1) << np.uint64(56))) >> np.uint64(57)) & np.uint64(127)


def _rms(x):
    return math.sqrt(float(np.mean(np.square(x))))


def _pbs_odd_slices(keys, small, tables, w, idx, D):
    """keys.pbs in launches of an odd number of ciphertexts (a partial last workgroup whatever the kernel packs per workgroup), none
    with an output buffer beyond ~128 MB"""
    cap = max(1, HOST_BYTES // ((D + 1) * 8))
    cap -= 1 - (cap & 1)
    outs = []
    for c0 in range(0, small.shape[0], cap):
        sm, ix = small[c0:c0 + cap], idx[c0:c0 + cap]
        pad = 1 - (sm.shape[0] & 1)
        if pad:
            sm, ix = np.concatenate([sm, sm[:1]]), np.concatenate([ix, ix[:1]])
        out = keys.pbs(0, sm, tables, w, ix)
        outs.append(out[:out.shape[0] - pad])
    return np.concatenate(outs)


# (d) .. (f): 37 ciphertexts leave a partial last workgroup whether a kernel packs 2, 4, 8 or 16 ciphertexts per workgroup
WB_COUNT, WB_BODY_ADD = 37, 0x9E3779B97F4A7C15


def _written(pre, dv, kN, D, body_add, reps):
    """what rows [1, 1 + len(dv)) of the buffer `pre` must hold after the bootstraps whose store-mode rows are dv (D + 1 words) were stored
    (reps = 0) or accumulated reps times with body_add on the body; every other row as it was"""
    want = pre.copy()
    rows = want[1:1 + dv.shape[0]]
    if reps == 0:
        rows[:, :kN] = dv[:, :kN]
        rows[:, kN:-1] = 0
        rows[:, -1] = dv[:, D] + np.uint64(body_add)
    for _ in range(reps):
        rows[:, :kN] += dv[:, :kN]
        rows[:, -1] += dv[:, D] + np.uint64(body_add)
    return want


def _same_rows(got, want, kN, what):
    """word for word, named by part: the guard rows, the ring's mask words, the words between the ring and the body, the body"""
    assert got.shape == want.shape, what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[-1], want[-1]), (what, "a row outside the launch was written")
    assert np.array_equal(got[:, :kN], want[:, :kN]), (what, "mask words of the ring", np.flatnonzero((got[:, :kN] != want[:, :kN]).any(axis=1)))
    assert np.array_equal(got[:, kN:-1], want[:, kN:-1]), (what, "words between the ring and the body", np.flatnonzero((got[:, kN:-1] != want[:, kN:-1]).any(axis=1)))
    assert np.array_equal(got[:, -1], want[:, -1]), (what, "body", np.flatnonzero(got[:, -1] != want[:, -1]))


# ------------------------------------------------------------------------------------------ host: the list is complete
def test_matrix_lists_every_instantiation():
    """the literal list above == what the PBS_CASES / PBS_MB_CASES text of csrc/dctfhe.hip and the two general two-bit forms yield (a new
    instantiation cannot be added without a case), and dctfhe_params_check accepts every entry as this module builds it"""
    import ctypes as C
    from dctfhe import _lib
    from dctfhe.engine import make_params
    src = open(os.path.join(ROOT, "dct-cryptonets_amd", "csrc", "dctfhe.hip")).read()
    body = lambda name: re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)\n" % name, src).group(1)
    want = {(int(a), int(b), int(c), 1) for a, b, c, _ in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", body("PBS_CASES"))}
    assert len(want) == 17
    mb = {(int(a), 1, 1, 2) for a in re.findall(r"X\((\d+)\)", body("PBS_MB_CASES"))}
    assert len(mb) == 3
    general = {(int(a), int(b), int(c), 2) for a, b, c in
               re.findall(r"t\.logN == (\d+) && t\.k == (\d+) && t\.l == (\d+) && t\.unroll == 2\) return launch_pbs_as", src)}
    assert general == {(11, 1, 3, 2), (10, 2, 1, 2)}
    listed = [tuple(p.values[:4]) for p in PBS_MATRIX]
    assert len(listed) == len(set(listed)) == 22 and set(listed) == want | mb | general
    L = _lib.load()
    for p in PBS_MATRIX + PBS_WIDE:
        logN, k, l, unroll, beta = p.values
        for D in (k << logN, 2 * (k << logN)):
            cp = make_params(D, N_SMALL, [_tier(logN, k, l, unroll, beta)], 2.0 ** -50)
            assert L.dctfhe_params_check(C.byref(cp)) == 0, (p.id, L.dctfhe_last_error().decode())


# ------------------------------------------------------------------------------------------ GPU: one case per kernel
def _run_case(gpu_ctx, oracle, logN, k, l, unroll, beta, D, name):
    from dctfhe.engine import Keys, make_params
    N, n = 1 << logN, N_SMALL
    tier = _tier(logN, k, l, unroll, beta)
    model = R.tier_spec(n, k, logN, l, beta, unroll, tier["glwe_sigma"])
    sigma, bound_max, bound_diff = R.sigma_model(model), R.max_bound(model), R.diff_bound(model)
    rec = dict(D=D, beta=beta, log2_sigma_model=math.log2(sigma), max_bound_over_sigma=bound_max / sigma)
    input_sigma = 2.0 ** (-62 if logN >= 12 else -50)
    keys = Keys(gpu_ctx, make_params(D, n, [tier], input_sigma), seed=41 + logN)
    try:
        S, s = keys.export_secret()
        s = s[:n].copy()
        rng = np.random.default_rng(1000 * logN + 100 * k + 10 * l + unroll)
        w_mid = min(6, logN - 5)

        # (a) the rotation sweep
        for w in (0, w_mid, logN - 1):
            levels = R.sweep_levels(logN, w, rng)
            idx = (np.arange(levels.size) % 3).astype(np.int32)
            tables = rng.integers(-8, 8, (3, 1 << w)).astype(np.int64) << 57
            out = _pbs_odd_slices(keys, R.level_grid_cts(s, logN, levels, rng), tables, w, idx, D)
            assert not out[:, k * N: D].any(), (name, w, "mask words beyond the ring")
            ph = oracle.lwe_phase(S, D, out)
            want = R.level_grid_expected(oracle, tables, idx, w, N, levels)
            bad = np.flatnonzero(_dec(ph) != _dec(want))
            err = np.abs(R.cent(ph - want)).max()
            rec["sweep_w%d" % w] = dict(levels=int(levels.size), max_err_over_sigma=err / sigma)
            print(name, "sweep w=%d: %d levels, max error %.2f sigma_model (bound %.1f)" % (w, levels.size, err / sigma, bound_max / sigma))
            assert bad.size == 0, (name, w, "levels that decode wrong", levels[bad][:16], _dec(ph)[bad][:16], _dec(want)[bad][:16])
            assert err < bound_max, (name, w, err, bound_max)

        # (b) noisy inputs against the oracle
        w, count = w_mid, 65
        msgs = (np.arange(count, dtype=np.uint64) * np.uint64(63)) % np.uint64(2 << w)      # every message of both halves where 2^(w+1) <= 65,
        idx = (np.arange(count) % 3).astype(np.int32)                                        # else 65 distinct ones spread over both
        tables = rng.integers(-8, 8, (3, 1 << w)).astype(np.int64) << 57
        small = oracle.lwe_encrypt(s, n, msgs << np.uint64(63 - w), 2.0 ** -30, seed=17 + logN)
        dev = keys.pbs(0, small, tables, w, idx)
        assert not dev[:, k * N: D].any(), (name, "mask words beyond the ring")
        want = R.message_expected(tables, idx, w, msgs)
        ph_dev = oracle.lwe_phase(S, D, dev)
        assert np.array_equal(_dec(ph_dev), _dec(want)), (name, np.flatnonzero(_dec(ph_dev) != _dec(want)))
        bsk = keys.export_bsk(0)
        refs = {}
        if unroll == 1:
            refs["f64"] = oracle.pbs(small, oracle.bsk_to_fourier(bsk), None, k, N, l, beta, tables, w, idx, D)
            if logN <= 11:
                refs["exact"] = oracle.pbs(small[:8], None, bsk, k, N, l, beta, tables, w, idx[:8], D, exact=True)
        else:
            refs["exact_two_bit"] = oracle.pbs_mb2(small[:8], bsk, k, N, l, beta, tables, w, idx[:8], D)
        err_dev = np.abs(R.cent(ph_dev - want))
        rec["noisy_max_err_over_sigma"] = err_dev.max() / sigma
        for kind, ref in refs.items():
            m = ref.shape[0]
            ph_ref = oracle.lwe_phase(S, D, ref)
            assert np.array_equal(_dec(ph_ref), _dec(want[:m])), (name, kind, "the oracle itself decodes wrong")
            rms, err_ref = _rms(R.cent(ph_dev[:m] - ph_ref)), np.abs(R.cent(ph_ref - want[:m]))
            rec["rms_diff_over_bound_" + kind] = rms / bound_diff
            print(name, "device - %s oracle on %d: rms %.3f of the bound; max error device %.2f / oracle %.2f sigma_model"
                  % (kind, m, rms / bound_diff, err_dev[:m].max() / sigma, err_ref.max() / sigma))
            assert rms < bound_diff, (name, kind, rms, bound_diff)
            assert err_dev[:m].max() < max(4 * err_ref.max(), bound_max), (name, kind, err_dev[:m].max(), err_ref.max(), bound_max)

        # (c) the same inputs in another order, and alone
        perm = rng.permutation(count)
        assert np.array_equal(keys.pbs(0, small[perm], tables, w, idx[perm]), dev[perm]), (name, "a result depends on its place in the launch")
        for c in (0, count - 1):
            assert np.array_equal(keys.pbs(0, small[c:c + 1], tables, w, idx[c:c + 1]), dev[c:c + 1]), (name, c, "a batch of one differs")

        # (d) .. (f): the write-back modes, on the first 37 inputs of (b).  By (c) their store-mode rows are dev[:37] whatever the launch.
        m, kN = WB_COUNT, k * N
        sm, ix, dv = small[:m], idx[:m], dev[:m]
        garbage = lambda dim: rng.integers(0, 2 ** 64, (m + 2, dim + 1), dtype=np.uint64)      # a guard row either side of the launched rows
        wide = dict(row0=1, table_idx=ix, body_add=WB_BODY_ADD)

        # (d) store mode
        assert np.array_equal(keys.pbs_rows(0, sm, tables, w, garbage(D)[:m], table_idx=ix), dv), (name, "store mode through pbs_rows differs from pbs")
        pre = garbage(D + 3)
        _same_rows(keys.pbs_rows(0, sm, tables, w, pre, **wide), _written(pre, dv, kN, D, WB_BODY_ADD, 0), kN, (name, "store, rows of D + 3 mask words"))
        rec["step_d"] = True

        # (e) accumulate mode, once and again on its own output
        for dim in (D, D + 3):
            pre = garbage(dim)
            once = keys.pbs_rows(0, sm, tables, w, pre, accumulate=True, **wide)
            _same_rows(once, _written(pre, dv, kN, D, WB_BODY_ADD, 1), kN, (name, "accumulate, rows of %d mask words" % dim))
            twice = keys.pbs_rows(0, sm, tables, w, once, accumulate=True, **wide)
            _same_rows(twice, _written(pre, dv, kN, D, WB_BODY_ADD, 2), kN, (name, "accumulate twice, rows of %d mask words" % dim))
        # ... and against the reference, not through store mode: onto fresh encryptions of known phases
        pre_ph = rng.integers(0, 2 ** 64, m, dtype=np.uint64)
        acc = keys.pbs_rows(0, sm, tables, w, keys.encrypt(pre_ph), table_idx=ix, accumulate=True, body_add=WB_BODY_ADD)
        want_ph = pre_ph + R.message_expected(tables, ix, w, msgs[:m]) + np.uint64(WB_BODY_ADD)
        err = np.abs(R.cent(oracle.lwe_phase(S, D, acc) - want_ph)).max()
        print(name, "accumulate onto encryptions: max error %.2f sigma_model" % (err / sigma))
        assert err < bound_max + 6 * input_sigma, (name, "accumulate onto encryptions", err, bound_max, input_sigma)
        rec["step_e"] = True

        # (f) per-channel tables: element e_offset + c of a tensor with hw elements per channel, nchan channels
        hw, nchan = 5, 3
        for e_offset in (7, (1 << 33) + 4):
            chan = np.array([((e_offset + c) // hw) % nchan for c in range(m)], np.int32)         # Python integers
            if e_offset >> 32:            # an offset cut to 32 bits picks other tables
                assert any(((e_offset % (1 << 32) + c) // hw) % nchan != chan[c] for c in range(m))
            by_rule = keys.pbs_rows(0, sm, tables, w, garbage(D)[:m], hw=hw, nchan=nchan, e_offset=e_offset)
            by_index = keys.pbs_rows(0, sm, tables, w, garbage(D)[:m], table_idx=chan)
            assert np.array_equal(by_rule, by_index), (name, "per-channel tables at e_offset", e_offset, np.flatnonzero((by_rule != by_index).any(axis=1)))
        one = keys.pbs_rows(0, sm, tables, w, garbage(D)[:m], hw=hw, nchan=1, e_offset=7)
        assert np.array_equal(one, keys.pbs_rows(0, sm, tables, w, garbage(D)[:m], table_idx=np.zeros(m, np.int32))), (name, "nchan = 1 must take table 0")
        rec["step_f"] = True
    finally:
        keys.close()
        MEASURED[name] = rec
        print("pbs_matrix.json", json.dumps({name: rec}))
        if OUT:
            os.makedirs(OUT, exist_ok=True)
            with open(os.path.join(OUT, "pbs_matrix.json"), "w") as f:
                json.dump(MEASURED, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("logN,k,l,unroll,beta", PBS_MATRIX)
def test_pbs_kernel(gpu_ctx, oracle, request, logN, k, l, unroll, beta):
    _run_case(gpu_ctx, oracle, logN, k, l, unroll, beta, k << logN, request.node.callspec.id)


@pytest.mark.gpu
@pytest.mark.parametrize("logN,k,l,unroll,beta", PBS_WIDE)
def test_pbs_kernel_big_key_wider_than_the_ring(gpu_ctx, oracle, request, logN, k, l, unroll, beta):
    _run_case(gpu_ctx, oracle, logN, k, l, unroll, beta, 2 * (k << logN), request.node.callspec.id)
