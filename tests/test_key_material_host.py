"""tests/key_material_ref.py against independent definitions, without a GPU: the long-double transform against exact evaluation, the
position rule as a bijection for every bootstrap instantiation, the exact negacyclic phase against schoolbook big-integer arithmetic, the
bands against numpy's own Gaussian, and the host emulation of key_poly_to_fourier (the thread program of k_bsk_fourier, compiled for the
CPU) against the reference through the documented layout of the evaluation-key blob."""
import math
import os
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

import key_material_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64


# ------------------------------------------------------------------------------------------ the transform against exact evaluation
_PI_DEC = Decimal("3.14159265358979323846264338327950288419716939937510582097494459")


def _cos_sin_dec(r, den):
    """(cos, sin) of pi r / den for integers 0 <= r < 2 den: the Taylor series in 70-digit decimal arithmetic (|x| < 2 pi: the largest
    term is below 100, so about 65 digits survive)"""
    x = _PI_DEC * r / den
    c = s = Decimal(0)
    term, n = Decimal(1), 0
    while abs(term) > Decimal(10) ** -68:
        if n % 2 == 0:
            c += term if n % 4 == 0 else -term
        else:
            s += term if n % 4 == 1 else -term
        n += 1
        term = term * x / n
    return c, s


def _dec(v):
    """a long double as a Decimal, exactly: its 64-bit mantissa is the sum of two doubles"""
    hi = float(v)
    return Decimal(hi) + Decimal(float(v - np.longdouble(hi)))


def _exact_spectrum(poly, N):
    """sum_n x_n zeta_k^n with the exponent n (1 - 4k) reduced mod 2N in integers, Python-int coefficients, decimal cos / sin"""
    getcontext().prec = 70
    table = [_cos_sin_dec(r, N) for r in range(2 * N)]
    out = []
    for k in range(N // 2):
        re_, im_ = Decimal(0), Decimal(0)
        for n, x in enumerate(poly):
            c, s = table[(n * (1 - 4 * k)) % (2 * N)]
            re_ += int(x) * c
            im_ += int(x) * s
        out.append((re_, im_))
    return out


@pytest.mark.parametrize("N", [16, 64])
def test_long_double_spectrum_matches_exact_evaluation(N):
    rng = np.random.default_rng(N)
    polys = np.stack([rng.integers(-2 ** 63, 2 ** 63, N, dtype=np.int64),                    # a mask polynomial
                      rng.integers(-2 ** 24, 2 ** 24, N, dtype=np.int64),                    # a noise polynomial
                      np.where(np.arange(N) == 0, np.int64(1) << np.int64(40), 0).astype(np.int64)])     # a gadget term
    polys[0, :3] = [-2 ** 63, 2 ** 63 - 1, -1]
    got = K.negacyclic_spectrum(polys, N)
    eps = float(np.finfo(np.longdouble).eps)
    worst = 0.0
    for q in range(polys.shape[0]):
        want = _exact_spectrum(polys[q], N)
        l1 = float(np.abs(polys[q].astype(np.longdouble)).sum())
        for k, (re_, im_) in enumerate(want):
            d = math.hypot(float(_dec(got[q, k].real) - re_), float(_dec(got[q, k].imag) - im_))
            worst = max(worst, d / (eps * l1))
    print("N %d: worst |long double - exact| = %.2f eps sum|x_n|" % (N, worst))
    # each of the log2 M butterfly passes and the twist multiplies by a twiddle good to ~1 eps and rounds once: a first-order bound of
    # (log2 N + 2) sqrt(2) eps on every term's weight, i.e. on sum |x_n|; a double-precision transform would sit near 2048 eps
    assert worst < math.sqrt(2.0) * (math.log2(N) + 2)


def test_f64_yardstick_is_the_same_transform():
    N = 64
    x = np.random.default_rng(1).integers(-2 ** 63, 2 ** 63, (2, N), dtype=np.int64)
    ld, f64 = K.negacyclic_spectrum(x, N), K.f64_spectrum(x, N)
    rel = np.abs(f64.astype(np.clongdouble) - ld).max() / np.abs(ld).max()
    assert 1e-19 < rel < 1e-14, rel                   # equal up to double precision, and not the same computation


# ------------------------------------------------------------------------------------------ the position rule
def test_spectrum_positions_is_a_bijection_for_every_instantiation():
    cases, mb = K.pbs_cases()
    seen = set()
    for logN, k, l, P in cases + [(lg, 1, 1, 8) for lg in mb]:
        if (logN, P) in seen:
            continue
        seen.add((logN, P))
        M = 1 << (logN - 1)
        for f in (K.spectrum_positions(logN, P), K.entry_frequencies(logN, P)):
            assert f.shape == (M,) and np.array_equal(np.sort(f), np.arange(M)), (logN, P)
    assert {(8, 8), (9, 16), (9, 8), (13, 8)} <= seen
    # two geometries by hand.  M = 128, P = 8: radices 8, 8, 2, weights 16, 2, 1 -> p = 16 a + 2 b + c holds k = a + 8 b + 64 c
    f = K.spectrum_positions(8, 8)
    assert f[16 * 3 + 2 * 5 + 1] == 3 + 8 * 5 + 64 * 1
    # M = 256, P = 16: radices 16, 16 -> p = 16 a + b holds k = a + 16 b
    f = K.spectrum_positions(9, 16)
    assert f[16 * 7 + 9] == 7 + 16 * 9
    # blob entry j T + t <-> position P t + j
    assert K.entry_frequencies(9, 16)[5 * 16 + 3] == K.spectrum_positions(9, 16)[16 * 3 + 5]


# ------------------------------------------------------------------------------------------ exact phases
def _schoolbook(a, s, N):
    """a S in Z[X] / (X^N + 1) mod 2^64 with Python integers"""
    out = [0] * N
    for i, ai in enumerate(a):
        for m, sm in enumerate(s):
            if sm:
                if i + m < N:
                    out[i + m] += int(ai)
                else:
                    out[i + m - N] -= int(ai)
    return np.array([v % 2 ** 64 for v in out], dtype=object).astype(U)


@pytest.mark.parametrize("k,N", [(1, 32), (2, 16)])
def test_glwe_phase_returns_the_noise_of_a_row_built_from_it(k, N):
    rng = np.random.default_rng(10 * k + N)
    S = rng.integers(0, 2, k * N).astype(np.uint8)
    S[0], S[N - 1] = 1, 1                                # the wrap-around with its sign, and no shift at all
    E = rng.integers(-2 ** 20, 2 ** 20, (3, N), dtype=np.int64)
    rows = rng.integers(0, 2 ** 64, (3, k + 1, N), dtype=U)
    for r in range(3):
        body = E[r].view(U).copy()
        for j in range(k):
            body += _schoolbook(rows[r, j], S[j * N:(j + 1) * N], N)
        rows[r, k] = body
    got = K.glwe_phase(rows, S, k, N)
    assert np.array_equal(got.view(np.int64), E)
    assert np.array_equal(K.glwe_phase(rows[1], S, k, N), got[1])            # a single row, no leading axis


def test_pair_secret_and_limbs():
    s = np.array([0, 0, 1, 0, 0, 1, 1, 1], np.uint8)
    assert K.pair_secret(s).tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert [K.ks_limbs(5, 2), K.ks_limbs(9, 2), K.ks_limbs(4, 4), K.ks_limbs(9, 4)] == [2, 4, 4, 8]
    assert K.bsk_mask_index(3, 2, 2, 2, 256) == (3 * 6 + 2) * 2 * 256 and K.bsk_streams(1) == (66, 67) and K.ksk_streams(2) == (20, 21)


# ------------------------------------------------------------------------------------------ the bands
def test_bands_accept_a_rounded_gaussian_and_refuse_the_planted_errors():
    rng = np.random.default_rng(5)
    n = 30 * 256                                         # the smallest sample the GPU module judges
    for sigma in (2.0 ** -40, 2.0 ** -62):
        std = sigma * 2.0 ** 64
        good = np.rint(rng.normal(0, std, n)).astype(np.int64)
        st = K.check_noise(good, sigma, "gaussian")
        assert st["n"] == n
        half = np.rint(rng.normal(0, std / 2, n)).astype(np.int64)
        flat = np.rint(rng.uniform(-math.sqrt(3) * std, math.sqrt(3) * std, n)).astype(np.int64)     # equal variance, another shape
        for bad in (half, flat, good + np.int64(max(1, round(std / 4))), np.zeros(n, np.int64)):
            with pytest.raises(AssertionError):
                K.check_noise(bad, sigma, "planted")
    K.check_noise(np.zeros(n, np.int64), 0.0, "sigma 0")
    with pytest.raises(AssertionError):
        K.check_noise(good, 0.0, "sigma 0 with noise")
    # at sigma 2^-62 the rounding is part of the model: without the 1/12 the same draws sit 0.5 % higher -- visible at n = 2^22
    big = np.rint(rng.normal(0, 4.0, 1 << 22)).astype(np.int64)
    assert abs(K.noise_stats(big, K.noise_var_model(2.0 ** -62))["var_ratio"] - 1) < 5 * math.sqrt(2 / big.size)
    assert K.noise_stats(big, 16.0)["var_ratio"] - 1 > 5 * math.sqrt(2 / big.size)
    # a key-switch-key body: the draw, then the rounding to the grid
    grid_bits = 48
    body = (np.rint(rng.normal(0, 2.0 ** 51, 2560)).astype(np.int64) + (1 << 47)) >> 48 << 48
    K.check_noise(body, 2.0 ** -13, "grid", grid_bits=grid_bits, with_kurtosis=False)
    # shared draws show as correlation
    E = np.rint(rng.normal(0, 2.0 ** 24, (6, 256))).astype(np.int64)
    assert K.max_abs_corr(E) < K.corr_band(256)
    E[4] = E[1]
    assert K.max_abs_corr(E) > 0.99


# ------------------------------------------------------------------------------------------ the thread program, compiled for the host
@pytest.fixture(scope="module")
def key_fourier(tmp_path_factory):
    """tests/emul/key_fourier.cpp built with the g++ line of tests/emul/Makefile (it needs no oracle library), outside the source tree"""
    exe = str(tmp_path_factory.mktemp("emul") / "key_fourier")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "emul", "key_fourier.cpp"), "-lm"])
    return exe


def _test_polys(N, rng):
    """what a key holds: uniform mask polynomials, a noise polynomial, a body with the gadget term, the extremes"""
    polys = rng.integers(0, 2 ** 64, (4, N), dtype=U)
    polys[1] = rng.integers(-2 ** 24, 2 ** 24, N, dtype=np.int64).view(U)
    polys[2, 0] += U(1) << U(53)
    polys[3, :4] = [2 ** 63, 2 ** 63 - 1, 2 ** 64 - 1, 0]
    return polys


@pytest.mark.parametrize("logN,P", [(9, 16), (11, 8), (8, 8)])
def test_emulated_key_poly_to_fourier_matches_the_long_double_reference(key_fourier, tmp_path, logN, P):
    """the position rule and the scaling as include/dctfhe.h documents them, and the accuracy bar of the GPU test on the same thread
    program compiled for the host: rms error within 3x, largest within 4x of numpy's own double-precision transform"""
    N, M = 1 << logN, 1 << (logN - 1)
    polys = _test_polys(N, np.random.default_rng(logN))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    polys.tofile(src)
    subprocess.check_call([key_fourier, str(logN), str(P), src, dst], timeout=120)
    dev = np.fromfile(dst, np.complex128).reshape(4, M)
    ref, yard = K.fourier_key_reference(polys, logN, P)
    rms, mx, rel = K.error_ratios(dev, ref, yard)
    print("host thread program logN %d P %d: rms ratio %.2f, max ratio %.2f, yardstick %.2e relative rms" % (logN, P, rms, mx, rel))
    assert rel < 1e-15                                                # the yardstick itself is a double-precision transform
    assert rms <= 3.0 and mx <= 4.0, (rms, mx)
    # a wrong position rule is not a small error: every other permutation of the entries is off by the size of the spectrum
    wrong, _ = K.fourier_key_reference(polys, logN, P)
    wrong = wrong[..., np.roll(np.arange(M), 1)]
    assert np.abs(dev.astype(np.clongdouble) - wrong).max() > 1e-3 * np.abs(ref).max()
