"""Plain references for dctfhe_dct_frontend (k_dct_frontend), written from the definitions and sharing nothing with the product:
the orthonormal blockwise DCT-II in a chosen precision, the 2x bilinear up-sampling of a coefficient grid (half-pixel centres, edge
clamp) in exact integers and in floating point, and the error bounds the device tests hold the float path to."""
import numpy as np


def dct_basis(fs, dtype=np.longdouble):
    """T[u, j] = sqrt(1/fs) for u = 0, sqrt(2/fs) cos(pi (2j+1) u / (2 fs)) otherwise"""
    j = np.arange(fs, dtype=dtype)
    u = np.arange(fs, dtype=dtype)[:, None]
    pi = np.arccos(dtype(-1))
    T = np.sqrt(dtype(2) / dtype(fs)) * np.cos(pi * (2 * j + 1) * u / dtype(2 * fs))
    T[0, :] = np.sqrt(dtype(1) / dtype(fs))
    return T


def block_dct(planes, fs, dtype=np.longdouble):
    """uint8 [B, fs*S, fs*S] -> [B, fs*fs, S, S]: coefficient u*fs+v of block (by, bx) is sum_ij T[u,i] (p - 128) T[v,j]"""
    B, side, _ = planes.shape
    S = side // fs
    T = dct_basis(fs, dtype)
    blk = (planes.astype(np.int64) - 128).astype(dtype).reshape(B, S, fs, S, fs)                # [b, by, i, bx, j]
    return np.einsum("ui,byixj,vj->buvyx", T, blk, T).reshape(B, fs * fs, S, S)


def _taps(S):
    """2x up-sampling, half-pixel centres: output o reads source (o + 0.5) / 2 - 0.5 = o/2 - 1/4: three quarters of the nearer cell
    o // 2 and one quarter of its neighbour on the side o leans to, clamped at the border"""
    o = np.arange(S)
    near = o // 2
    far = np.clip(np.where(o % 2 == 0, near - 1, near + 1), 0, S // 2 - 1)
    return near, far


def upsample2_numerator(grid):
    """integer [..., Sc, Sc] -> integer [..., 2 Sc, 2 Sc]: sixteen times the bilinear value, weights 9, 3, 3, 1"""
    g = np.asarray(grid).astype(np.int64)
    near, far = _taps(2 * g.shape[-1])
    rows_n, rows_f = g[..., near, :], g[..., far, :]
    return 9 * rows_n[..., near] + 3 * rows_n[..., far] + 3 * rows_f[..., near] + rows_f[..., far]


def round_sixteenths_half_even(num):
    """num / 16 rounded to the nearest integer, ties to even, on integers"""
    q, r = np.divmod(num, 16)
    return q + ((r > 8) | ((r == 8) & (q % 2 == 1)))


def upsample2_int(grid):
    return round_sixteenths_half_even(upsample2_numerator(grid))


def upsample2_float(grid):
    """the same rule in the array's own floating-point type"""
    g = np.asarray(grid)
    near, far = _taps(2 * g.shape[-1])
    rows_n, rows_f = g[..., near, :], g[..., far, :]
    return (9 * rows_n[..., near] + 3 * rows_n[..., far] + 3 * rows_f[..., near] + rows_f[..., far]) / g.dtype.type(16)


def float_reference(y, c1, c2, fs, idx, dtype=np.longdouble):
    """what dctfhe_dct_frontend computes before its normalisation, round_coeffs off: [B, n0+n1+n2, S, S] in `dtype`"""
    S = y.shape[1] // fs
    parts = []
    for planes, ix in zip((y, c1, c2), idx):
        d = block_dct(planes, fs, dtype)
        if d.shape[-1] != S:
            assert 2 * d.shape[-1] == S
            d = upsample2_float(d)
        parts.append(d[:, np.asarray(ix, np.int64)])
    return np.concatenate(parts, axis=1)


def assert_unit_stats_bound(out, ref, what=""):
    """mean 0, std 1: the kernel's last step is one rounding of its f64 value to f32.  It accumulates at most fs^2 + 4 <= 68 f64
    terms of magnitude <= 1024, so the f64 value is within 8e-12 ~ 2^-37 of the definition; where that error straddles an f32
    rounding boundary the result is the neighbouring float, one ulp off.  Hence |out - f32(ref)| <= spacing(f32(ref)) + 2^-36."""
    r32 = np.asarray(ref).astype(np.float32)
    err = np.abs(out.astype(np.float64) - r32.astype(np.float64))
    bound = np.spacing(np.abs(r32)).astype(np.float64) + 2.0 ** -36
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: max |out - f32(ref)| = {err.max():.3e}; worst excess over the bound {float((err - bound)[worst]):.3e} at {worst}")
    assert (err <= bound).all(), (what, worst, float(out[worst]), float(r32[worst]))


def normalised_bound(r_abs, mean, std):
    """bound on |out - r| for out = fl32(fl32(fl32(v') - m) / s) against r = (v - m) / s, with u = 2^-24 the f32 unit round-off and
    |v' - v| <= 2^-37 the kernel's f64 error (see assert_unit_stats_bound):
        a = fl32(v')      |a - v|       <= 2^-37 + u |v|
        d = fl32(a - m)   |d - (v - m)| <= |a - v| + u |v - m|
        q = fl32(d / s)   |q - r|       <= |d - (v - m)| / s + u |r|
    and with |v - m| = |r| s, |v| <= |r| s + |m|:   |q - r| <= 2^-37 / s + u (3 |r| + |m| / s).
    The second-order terms (u times an error) are covered by the factor 1 + 2^-20; 2^-149 allows for a subnormal quotient."""
    u = 2.0 ** -24
    m = np.abs(np.asarray(mean, np.float64))[:, None, None]
    s = np.abs(np.asarray(std, np.float64))[:, None, None]
    return (2.0 ** -37 / s + u * (3.0 * np.asarray(r_abs, np.float64) + m / s)) * (1.0 + 2.0 ** -20) + 2.0 ** -149


def assert_normalised_bound(out, ref, mean, std, what=""):
    """out [B, C, S, S] float32 from the device with statistics mean / std (as float32) against ref = the un-normalised definition"""
    m32, s32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    dt = np.asarray(ref).dtype.type
    r = (ref - m32.astype(dt)[:, None, None]) / s32.astype(dt)[:, None, None]
    err = np.abs(out.astype(dt) - r).astype(np.float64)
    bound = normalised_bound(np.abs(r).astype(np.float64), m32, s32)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"{what}: max err / bound = {float((err / bound)[worst]):.3f} at {worst} (|r| = {float(abs(r[worst])):.4g})")
    assert (err <= bound).all(), (what, worst, float(out[worst]), float(r[worst]))
