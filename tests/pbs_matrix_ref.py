"""What tests/test_gpu_pbs_matrix.py and tests/test_oracle_tfhe.py share: small ciphertexts on the level grid of a ring (their mod switch
is exact, so the blind rotation turns by a known amount), what such a bootstrap must decrypt to, which levels a sweep visits, and the
bounds params.var_pbs_out gives for one tier.  No GPU, no kernel output: everything here comes from the scheme's definition, the oracle's
test vector (ref_build_testvector) and the project's noise model."""
import dataclasses
import math

import numpy as np

FFT_WINDOW = 1.6          # upper edge of the calibration window of the f64-FFT term (tests/test_gpu_noise.py: [0.5x, 1.6x] of the model)


def cent(x):
    """torus words -> centred fractions in [-1/2, 1/2)"""
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


def level_grid_cts(s, logN, levels, rng):
    """Noise-free small ciphertexts under the key bits s whose words all sit on the 2N-level grid: mask words u_i << (63 - logN) with
    random u_i in [0, 2N), body (sum_i u_i s_i + t) << (63 - logN).  Rounding to 2N levels changes nothing, so the blind rotation turns
    the test vector by exactly t = levels[c]."""
    levels = np.asarray(levels)
    n, sh = s.size, np.uint64(63 - logN)
    u = rng.integers(0, 2 << logN, (levels.size, n), dtype=np.uint64)
    cts = np.empty((levels.size, n + 1), np.uint64)
    cts[:, :n] = u << sh
    cts[:, n] = ((u * s.astype(np.uint64)).sum(axis=1, dtype=np.uint64) + levels.astype(np.uint64)) << sh
    return cts


def level_grid_expected(oracle, tables, table_idx, w, N, levels):
    """the phase a bootstrap rotated by t must leave: coefficient 0 of X^-t tv, i.e. tv[t] for t < N and -tv[t - N] above, with the
    oracle's own test vector of table table_idx[c]"""
    levels = np.asarray(levels).astype(np.int64)
    tvs = np.stack([oracle.build_testvector(tb, w, N) for tb in np.asarray(tables, np.int64).reshape(-1, 1 << w)])
    v = tvs[np.asarray(table_idx, np.int64), levels % N]
    return np.where(levels >= N, np.uint64(0) - v, v)


def message_expected(tables, table_idx, w, msgs):
    """the same rule on box centres: message m < 2^w looks up table[m], m + 2^w its negation"""
    tables = np.asarray(tables, np.int64).reshape(-1, 1 << w).astype(np.uint64)
    msgs = np.asarray(msgs).astype(np.int64)
    v = tables[np.asarray(table_idx, np.int64), msgs % (1 << w)]
    return np.where(msgs >= (1 << w), np.uint64(0) - v, v)


def sweep_levels(logN, w, rng, target=2048):
    """The rotation amounts a sweep visits.  Rings up to N = 2048: all 2N.  Larger rings: about `target` of them -- every level within 3
    of each box edge of the first and last 8 boxes (the test vector changes value at m box - box/2), the 32 levels at either end of
    [0, 2N), the 64 around N where the sign flips, and a random remainder."""
    N = 1 << logN
    if logN <= 11:
        return np.arange(2 * N, dtype=np.int64)
    box, nbox = N >> w, 2 << w
    picked = [np.arange(0, 32), np.arange(2 * N - 32, 2 * N), np.arange(N - 32, N + 32)]
    for m in sorted(set(range(min(9, nbox))) | set(range(max(0, nbox - 8), nbox))):
        picked.append((m * box - (box >> 1) + np.arange(-3, 4)) % (2 * N))
    fixed = np.unique(np.concatenate(picked))
    rest = np.setdiff1d(np.arange(2 * N), fixed)
    extra = rng.choice(rest, max(0, target - fixed.size), replace=False)
    return np.concatenate([fixed, np.sort(extra)]).astype(np.int64)


def tier_spec(n, k, logN, l, beta, unroll, glwe_sigma, lk=4, betak=4, lwe_sigma=2.0 ** -24):
    from dctfhe import params as P
    return P.TierSpec("m", n=n, k=k, logN=logN, l=l, beta=beta, lk=lk, betak=betak, unroll=unroll, lwe_sigma=lwe_sigma, glwe_sigma=glwe_sigma)


def sigma_model(t):
    """sigma of a bootstrap's output under the model the compiler budgets with"""
    from dctfhe import params as P
    return math.sqrt(P.var_pbs_out(t))


def max_bound(t):
    """a maximum over the samples of one test: 6 sigma, at the upper edge of the model's calibration window"""
    return 6.0 * FFT_WINDOW * sigma_model(t)


def diff_bound(t):
    """rms of (f64 bootstrap - another bootstrap of the same inputs and keys): the key noise is common to both, what differs is the
    transform error and the digits it flips -- the fft and dec terms of var_pbs_out (the model with the key noise taken out), once per
    side that runs the f64 transform, hence sqrt(2)"""
    from dctfhe import params as P
    return math.sqrt(2.0) * FFT_WINDOW * math.sqrt(P.var_pbs_out(dataclasses.replace(t, glwe_sigma=2.0 ** -200)))
