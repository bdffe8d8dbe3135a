"""What tests/test_gpu_key_material.py and tests/test_key_material_host.py share: the definitions the key material is held to, restated
in numpy from include/dctfhe.h (generator streams next to dctfhe_client_key_export_bsk, Fourier-key layout next to
dctfhe_eval_keys_export).  No GPU, no kernel output, nothing imported from the kernels.

  glwe_phase            exact negacyclic body - sum_j a_j S_j mod 2^64, by shift-and-add over the set bits of S
  negacyclic_spectrum   evaluations at e^{i pi (1 - 4k) / N} in long double (twisted radix-2 transform, long-double cos / sin)
  spectrum_positions    in-place position -> frequency of the mixed-radix forward transform; entry_frequencies: blob entry -> frequency
  *_band, noise_var_model   acceptance bands of sample statistics, DERIVED (5 standard deviations of the estimator), not measured
"""
import math
import os
import re

import numpy as np

U = np.uint64
LD = np.longdouble
CLD = np.clongdouble

STREAM_KSK, STREAM_BSK = 16, 64          # + 2 tier: masks from the public generator key; + 2 tier + 1: noise from the secret one


def pbs_cases():
    """(logN, k, l, P) of every PBS_CASES entry and the logN of every PBS_MB_CASES entry, parsed from the source text the way
    test_gpu_pbs_matrix.py::test_matrix_lists_every_instantiation does (the only thing taken from the kernels' side: which shapes exist
    and how many points per thread each transform keeps)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "dct-cryptonets_amd", "csrc", "dctfhe.hip")).read()
    body = lambda name: re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)\n" % name, src).group(1)
    cases = [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", body("PBS_CASES"))]
    mb = [int(a) for a in re.findall(r"X\((\d+)\)", body("PBS_MB_CASES"))]
    assert len(cases) == len(set(c[:3] for c in cases)) == 17 and len(mb) == 3
    return cases, mb


# ------------------------------------------------------------------------------------------ streams and indices
def ksk_streams(tier):
    return STREAM_KSK + 2 * tier, STREAM_KSK + 2 * tier + 1


def bsk_streams(tier):
    return STREAM_BSK + 2 * tier, STREAM_BSK + 2 * tier + 1


def bsk_grow(block, r, k, l):
    """global row id of row r = p l + lev of key block `block`"""
    return block * (k + 1) * l + r


def bsk_mask_index(block, r, k, l, N):
    """generator index of mask word (j = 0, c = 0) of that row; its k N mask words follow contiguously: (grow k + j) N + c"""
    return bsk_grow(block, r, k, l) * k * N


def ks_limbs(lk, betak):
    """bytes a key-switch-key word keeps: 2 / 4 / 8 for lk betak + 6 <= 16 / <= 32 / more"""
    bits = lk * betak + 6
    return 2 if bits <= 16 else 4 if bits <= 32 else 8


def pair_secret(s):
    """the 3 n / 2 bits an unroll-2 key encrypts: per pair (a, b) the products a (1 - b), (1 - a) b, a b"""
    s = np.asarray(s, np.uint8)
    a, b = s[0::2], s[1::2]
    return np.stack([a & (1 - b), (1 - a) & b, a & b], axis=1).reshape(-1).astype(np.uint8)


# ------------------------------------------------------------------------------------------ exact ring arithmetic
def glwe_phase(rows, S, k, N):
    """rows [..., k + 1, N] u64 (k mask polynomials, then the body), S: at least k N key bits (S_j = S[j N : (j + 1) N]).
    Returns body - sum_j a_j S_j in Z_{2^64}[X] / (X^N + 1), [..., N] u64.
    Method: exact shift-and-add.  X^m a is the window [N - m, 2 N - m) of (-a | a); one subtraction per set bit of S_j, all in wrapping
    u64 arithmetic -- no floating point, no transform."""
    rows = np.asarray(rows, U)
    assert rows.shape[-2:] == (k + 1, N), rows.shape
    S = np.asarray(S, np.uint8)
    out = rows[..., k, :].copy()
    for j in range(k):
        a = rows[..., j, :]
        ext = np.concatenate([U(0) - a, a], axis=-1)
        for m in np.flatnonzero(S[j * N:(j + 1) * N]):
            out -= ext[..., N - m:2 * N - m]
    return out


def key_poly(S, p, N):
    """S_p as a polynomial with u64 coefficients"""
    return np.asarray(S[p * N:(p + 1) * N], np.uint8).astype(U)


def centred(x):
    """torus words -> signed integers in [-2^63, 2^63)"""
    return np.ascontiguousarray(x, U).view(np.int64)


# ------------------------------------------------------------------------------------------ long-double transform
def _require_long_double():
    nm = np.finfo(LD).nmant
    assert nm >= 63, ("np.longdouble has a %d-bit mantissa on this host; the reference transform needs the 64-bit x87 format (x86-64) -- "
                      "a double-precision reference cannot judge a double-precision kernel" % nm)


_PI = None


def _pi():
    global _PI
    if _PI is None:
        _PI = LD("3.14159265358979323846264338327950288419716939937510")
    return _PI


def _cis(num, den):
    """e^{i pi num / den} for integer arrays num (reduced exactly mod 2 den) in long double"""
    r = np.asarray(num, np.int64) % (2 * den)
    a = _pi() * r.astype(LD) / LD(den)
    out = np.empty(r.shape, CLD)
    out.real, out.imag = np.cos(a), np.sin(a)
    return out


def negacyclic_spectrum(polys_i64, N):
    """polys [..., N] of signed 64-bit coefficients -> [..., M = N / 2] complex long doubles, entry k the polynomial evaluated at
    zeta_k = e^{i pi (1 - 4k) / N}: with zeta_k^M = i, sum_n (x_n + i x_{n+M}) e^{i pi n / N} e^{-2 pi i n k / M} -- the fold and twist,
    then a forward DFT of size M, here radix-2 decimation in time with every twiddle straight from long-double cos / sin."""
    _require_long_double()
    x = np.asarray(polys_i64)
    assert x.dtype == np.int64 and x.shape[-1] == N and N >= 4 and N & (N - 1) == 0
    M = N // 2
    z = np.empty(x.shape[:-1] + (M,), CLD)
    z.real, z.imag = x[..., :M].astype(LD), x[..., M:].astype(LD)
    z *= _cis(np.arange(M), N)
    # bit-reversal, then log2 M butterfly passes
    bits = M.bit_length() - 1
    rev = np.zeros(M, np.int64)
    for b in range(bits):
        rev |= ((np.arange(M) >> b) & 1) << (bits - 1 - b)
    z = z[..., rev]
    h = 1
    while h < M:
        w = _cis(-np.arange(h), h)                     # e^{-2 pi i m / (2h)}
        z = z.reshape(x.shape[:-1] + (M // (2 * h), 2, h))
        t = z[..., 1, :] * w
        z = np.concatenate([z[..., 0, :] + t, z[..., 0, :] - t], axis=-1)      # [.., M / 2h, 2h]
        h *= 2
    return z.reshape(x.shape[:-1] + (M,))


def f64_spectrum(polys_i64, N):
    """the double-precision yardstick: the same evaluations from np.fft.fft of the f64-converted, f64-twisted fold"""
    x = np.asarray(polys_i64)
    M = N // 2
    z = (x[..., :M].astype(np.float64) + 1j * x[..., M:].astype(np.float64)) * np.exp(1j * np.pi * np.arange(M) / N)
    return np.fft.fft(z, axis=-1)


def spectrum_positions(logN, P):
    """frequency k of in-place position p < M after the forward transform: M = R_0 ... R_{s-1}, every pass of radix P but the last,
    which has M / P^(s-1); position digit i has weight W_i = prod_{j > i} R_j and holds frequency digit k_i of weight R_0 ... R_{i-1}."""
    M = 1 << (logN - 1)
    logp = P.bit_length() - 1
    assert 1 << logp == P
    s = -(-(logN - 1) // logp)
    R = [P] * (s - 1) + [M // P ** (s - 1)]
    assert all(r >= 1 for r in R) and math.prod(R) == M
    p = np.arange(M)
    k, fw = np.zeros(M, np.int64), 1
    for i in range(s):
        W = math.prod(R[i + 1:])
        k += ((p // W) % R[i]) * fw
        fw *= R[i]
    return k


def entry_frequencies(logN, P):
    """frequency of entry e of a polynomial's M complex values in the evaluation-key blob: entry j T + t holds position P t + j"""
    M = 1 << (logN - 1)
    T = M // P
    e = np.arange(M)
    return spectrum_positions(logN, P)[P * (e % T) + e // T]


def fourier_key_reference(polys_u64, logN, P):
    """what the blob must hold for these standard-domain polynomials [..., N] u64: (long-double reference, f64 yardstick), both
    [..., M] in blob entry order and scaled by 2^-64 / M"""
    N = 1 << logN
    x = np.asarray(polys_u64, U).view(np.int64)
    k = entry_frequencies(logN, P)
    scale = LD(2.0) ** -64 / LD(N // 2)
    return negacyclic_spectrum(x, N)[..., k] * scale, f64_spectrum(x, N)[..., k] * (2.0 ** -64 / (N // 2))


def error_ratios(dev_c128, ref_cld, yard_c128):
    """(rms ratio, max ratio, relative rms of the yardstick) of |device - reference| over |f64 yardstick - reference|"""
    err = np.abs(np.asarray(dev_c128).astype(CLD) - ref_cld).astype(np.float64)
    yard = np.abs(np.asarray(yard_c128).astype(CLD) - ref_cld).astype(np.float64)
    rms = lambda v: math.sqrt(float(np.mean(np.square(v))))
    return rms(err) / rms(yard), float(err.max() / yard.max()), rms(yard) / rms(np.abs(ref_cld).astype(np.float64))


# ------------------------------------------------------------------------------------------ bands
def noise_var_model(sigma, grid_bits=0):
    """variance, in units of 2^-64, of a Gaussian draw of std sigma (fraction of the torus) rounded to the nearest integer:
    (sigma 2^64)^2 + 1/12.  A key-switch-key body is then rounded to the 2^-(8 limbs) grid: grid_bits = 64 - 8 limbs adds 2^(2 grid_bits) / 12."""
    v = (sigma * 2.0 ** 64) ** 2 + 1.0 / 12.0
    if grid_bits:
        v += 4.0 ** grid_bits / 12.0
    return v


def var_band(n):
    """sample variance of n Gaussian draws over the true one: 1 +- 5 sqrt(2 / n)"""
    d = 5.0 * math.sqrt(2.0 / n)
    return 1.0 - d, 1.0 + d


def kurt_band(n):
    """excess kurtosis of n Gaussian draws: +- 5 sqrt(24 / n)"""
    return 5.0 * math.sqrt(24.0 / n)


def mean_band(std, n):
    """mean of n draws of standard deviation std: +- 5 std / sqrt(n)"""
    return 5.0 * std / math.sqrt(n)


def corr_band(n):
    """sample correlation of two independent sequences of n draws: +- 5 / sqrt(n)"""
    return 5.0 / math.sqrt(n)


def noise_stats(E, var_model):
    """E: signed integer noise (any shape) -> dict(n, var_ratio, mean, kurt, max_abs): variance about zero over the model, excess kurtosis
    about zero, all in f64"""
    e = np.asarray(E).reshape(-1)
    assert e.dtype == np.int64
    f = e.astype(np.float64)                 # rounds beyond 2^53: one part in 2^53 of a value, nothing to a second moment
    m2 = float(np.mean(f * f))
    m4 = float(np.mean((f * f) ** 2))
    return dict(n=int(e.size), var_ratio=m2 / var_model, mean=float(f.mean()), kurt=(m4 / (m2 * m2) - 3.0) if m2 > 0 else 0.0,
                max_abs=float(np.abs(f).max(initial=0.0)))


def check_noise(E, sigma, what, grid_bits=0, with_kurtosis=True):
    """asserts the bands on a sample of noise terms and returns noise_stats.  sigma = 0: E must be identically zero (no grid)."""
    if sigma == 0.0 and not grid_bits:
        assert not np.asarray(E).any(), (what, "noise at sigma = 0")
        return dict(n=int(np.asarray(E).size), var_ratio=1.0, mean=0.0, kurt=0.0, max_abs=0.0)
    vm = noise_var_model(sigma, grid_bits)
    st = noise_stats(E, vm)
    lo, hi = var_band(st["n"])
    std = math.sqrt(vm)
    print("%s: n %d, var / model %.4f (band %.4f .. %.4f), mean %.3g (band %.3g), excess kurtosis %.3f (band %.3f), max %.2f sigma"
          % (what, st["n"], st["var_ratio"], lo, hi, st["mean"], mean_band(std, st["n"]), st["kurt"], kurt_band(st["n"]), st["max_abs"] / std))
    assert lo < st["var_ratio"] < hi, (what, "variance", st)
    assert abs(st["mean"]) < mean_band(std, st["n"]), (what, "mean", st)
    if with_kurtosis:
        assert abs(st["kurt"]) < kurt_band(st["n"]), (what, "kurtosis", st)
    if not grid_bits:
        assert st["max_abs"] < 6.5 * sigma * 2.0 ** 64, (what, "maximum", st)
    return st


def max_abs_corr(E):
    """E [rows, N] signed noise -> the largest |sample correlation| between two distinct rows (about zero: the draws are centred)"""
    f = np.asarray(E).astype(np.float64)
    nrm = np.sqrt((f * f).sum(axis=1))
    assert (nrm > 0).all()
    c = (f / nrm[:, None]) @ (f / nrm[:, None]).T
    np.fill_diagonal(c, 0.0)
    return float(np.abs(c).max())
