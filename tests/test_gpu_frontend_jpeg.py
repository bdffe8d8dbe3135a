"""k_dct_frontend against libjpeg and against its definition.
  * round_coeffs path (block size 8): the quantised coefficients libjpeg wrote into the JPEG files of tests/golden/jpeg_golden.npz
    (tools/make_jpeg_goldens.py; read from the npz only), the chroma grids up-sampled by an all-integer statement of the bilinear rule
    with ties to even -- equality, no tolerance.
  * plane slots, images, coefficient indices and statistics: every output channel from the right place.
  * float path: the orthonormal DCT-II and the up-sampling in np.longdouble, to a bound derived from the number formats
    (tests/frontend_ref.py), at grids that are no power of two, with both borders clamping, and past the launch's 16384 x 256 threads
    so that the grid-stride loop takes its second trip."""
import os

import numpy as np
import pytest

import frontend_ref as R

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "jpeg_golden.npz"))
RGB = [str(n) for n in G["rgb_names"]]
GRAY = [str(n) for n in G["gray_names"]]
ALL64 = np.arange(64, dtype=np.int32)
NONE = np.zeros(0, np.int32)


# ------------------------------------------------------------------------------------------ integer path == libjpeg
@pytest.mark.parametrize("name", GRAY)
def test_integer_dct_equals_libjpeg_gray(gpu_ctx, name):
    plane, coef = G[f"gray_{name}_plane"], G[f"gray_{name}_coef"]
    S = min(plane.shape) // 8
    p = plane[None, :8 * S, :8 * S]
    out = gpu_ctx.dct_frontend(p, p, p, 8, (ALL64, NONE, NONE), np.zeros(64), np.ones(64), round_coeffs=True)
    want = coef[:S, :S].transpose(2, 0, 1)[None].astype(np.float32)
    assert out.shape == want.shape == (1, 64, S, S)
    assert np.array_equal(out, want), f"{int((out != want).sum())} of {want.size} coefficients differ from libjpeg's"


def _colour_case(name):
    """planes of the square crop (host colour conversion + down-sampler, pinned in tests/test_jpeg_pin_host.py) and libjpeg's
    coefficients for it: the crop starts at the origin, so blocks and the down-sampler's column phase are those of the whole image"""
    from dctfhe import frontend
    img = G[f"rgb_{name}_img"]
    side = min(img.shape[:2])
    S, Sc = side // 8, side // 16
    y, cb, cr = frontend.jpeg_planes_u8(img[:side, :side])
    gy, gcb, gcr = (G[f"rgb_{name}_{t}"].astype(np.int64) for t in ("y", "cb", "cr"))
    return (y[None], cb[None], cr[None]), gy[:S, :S].transpose(2, 0, 1), gcb[:Sc, :Sc].transpose(2, 0, 1), gcr[:Sc, :Sc].transpose(2, 0, 1)


@pytest.mark.parametrize("name", RGB)
def test_integer_path_equals_libjpeg_colour(gpu_ctx, name):
    (y, cb, cr), gy, gcb, gcr = _colour_case(name)
    S = gy.shape[-1]
    assert not np.array_equal(cb, cr) or name == "dc_ties"
    out = gpu_ctx.dct_frontend(y, cb, cr, 8, (ALL64, ALL64, ALL64), np.zeros(192), np.ones(192), round_coeffs=True)
    want = np.concatenate([gy, R.upsample2_int(gcb), R.upsample2_int(gcr)])[None]         # integers from libjpeg's coefficients on
    assert out.shape == want.shape == (1, 192, S, S)
    assert np.array_equal(out, want.astype(np.float32)), f"{int((out != want).sum())} of {want.size} values differ"


def test_colour_expectations_hold_upsampling_ties():
    """the expectation above must hold values exactly between two integers (numerator = 8 mod 16), with an even and with an odd
    integer below: that is where half-to-even differs from half-up, half-down and half-away-from-zero"""
    below = []
    for name in RGB:
        _, _, gcb, gcr = _colour_case(name)
        for g in (gcb, gcr):
            num = R.upsample2_numerator(g)
            below.append((num // 16)[num % 16 == 8])
    below = np.concatenate(below)
    assert (below % 2 == 0).sum() >= 10 and (below % 2 == 1).sum() >= 10
    assert (below < 0).any() and (below >= 0).any()


# ------------------------------------------------------------------------------------------ slots, images, indices, statistics
INDEX_CASES = {
    "no_luma": ([], [5, 0], [63]),
    "no_slot1": ([0, 63], [], [1, 8]),
    "no_slot2": ([7], [56, 9], []),
    "repeated": ([3, 3, 10], [2, 2], [2]),
    "descending": ([63, 40, 8, 1, 0], [9, 1], [17, 16, 0]),
    "ends_in_last": ([0, 1, 63], [0, 63], [62, 63]),
}


@pytest.fixture(scope="module")
def plumbing_planes():
    """batch 3, a different plane per image and per slot, for S = 6 / Sc = 3 and S = 5 / Sc = 5; the quantised coefficients of every
    plane from the host restatement (equal to libjpeg: tests/test_jpeg_pin_host.py)"""
    from dctfhe import frontend
    rng = np.random.default_rng(77)
    out = {}
    for S, Sc in ((6, 3), (5, 5)):
        planes = [rng.integers(0, 256, (3, 8 * n, 8 * n), dtype=np.uint8) for n in (S, Sc, Sc)]
        coefs = [np.stack([frontend.jpeg_quantised_dct(p).transpose(2, 0, 1) for p in pl]) for pl in planes]      # [3, 64, n, n]
        out[S] = (planes, coefs)
    return out


@pytest.mark.parametrize("S", [6, 5])
@pytest.mark.parametrize("case", list(INDEX_CASES))
def test_every_channel_comes_from_its_plane_image_and_coefficient(gpu_ctx, plumbing_planes, S, case):
    planes, coefs = plumbing_planes[S]
    idx = INDEX_CASES[case]
    C = sum(map(len, idx))
    # statistics that name their channel and keep the arithmetic exact: integer means, power-of-two deviations
    mean = np.arange(C, dtype=np.float32) * 3 - 4
    std = np.array([0.5, 1.0, 2.0, 4.0], np.float32)[np.arange(C) % 4]
    out = gpu_ctx.dct_frontend(planes[0], planes[1], planes[2], 8, idx, mean, std, round_coeffs=True)
    want = []
    for slot in range(3):
        g = coefs[slot][:, np.asarray(idx[slot], np.int64)]
        want.append(g if g.shape[-1] == S else R.upsample2_int(g))
    want = (np.concatenate(want, axis=1).astype(np.float64) - mean[:, None, None]) / std[:, None, None]
    assert out.shape == want.shape == (3, C, S, S)
    assert np.array_equal(out, want.astype(np.float32))
    assert np.array_equal(want.astype(np.float32), want)                                  # the expectation is exact in f32


def test_plumbing_planes_tell_slots_and_images_apart(plumbing_planes):
    """a wrong slot, image or coefficient must change the expectation: the planes' coefficient grids all differ"""
    for S, (planes, coefs) in plumbing_planes.items():
        grids = [coefs[slot][b, k] for slot in range(3) for b in range(3) for k in (0, 1, 2, 8, 9, 62, 63)]
        grids = [g if g.shape[-1] == S else R.upsample2_int(g) for g in grids]
        for i in range(len(grids)):
            for j in range(i):
                assert not np.array_equal(grids[i], grids[j])


# ------------------------------------------------------------------------------------------ float path against the definition
def _float_planes(fs, n, seed):
    """[3, fs*n, fs*n]: noise, a constant plane, a 0/255 checkerboard (cells of one pixel; `seed` picks phase and constant)"""
    rng = np.random.default_rng(seed)
    side = fs * n
    noise = rng.integers(0, 256, (side, side), dtype=np.uint8)
    const = np.full((side, side), (0, 255, 131, 77)[seed % 4], np.uint8)
    yy, xx = np.indices((side, side))
    checker = (((yy + xx + seed) % 2) * 255).astype(np.uint8)
    order = [(noise, const, checker), (checker, noise, const), (const, checker, noise)][seed % 3]
    return np.stack(order)


@pytest.fixture(scope="module")
def float_cases():
    """planes and the np.longdouble reference, computed once per (block size, grids)"""
    out = {}
    for fs in (4, 8):
        allc = np.arange(fs * fs, dtype=np.int32)
        for S, Sc in ((6, 3), (5, 5)):
            y, c1, c2 = _float_planes(fs, S, 0), _float_planes(fs, Sc, 1), _float_planes(fs, Sc, 2)
            out[fs, S] = (y, c1, c2, (allc, allc, allc), R.float_reference(y, c1, c2, fs, (allc, allc, allc)))
    return out


@pytest.mark.parametrize("S", [6, 5])
@pytest.mark.parametrize("fs", [4, 8])
def test_float_path_unit_statistics(gpu_ctx, float_cases, fs, S):
    y, c1, c2, idx, ref = float_cases[fs, S]
    C = 3 * fs * fs
    out = gpu_ctx.dct_frontend(y, c1, c2, fs, idx, np.zeros(C), np.ones(C))
    assert out.shape == ref.shape == (3, C, S, S)
    # constant planes: every AC term of the definition is zero (the longdouble sum leaves < 2^-50), so the absolute floor is tested
    for planes, lo in ((y, 0), (c1, fs * fs), (c2, 2 * fs * fs)):
        for b in range(3):
            if planes[b].min() == planes[b].max():
                assert np.abs(ref[b, lo + 1:lo + fs * fs]).max() < 2.0 ** -50
                assert np.abs(ref[b, lo] - fs * (int(planes[b, 0, 0]) - 128)).max() < 2.0 ** -50
    R.assert_unit_stats_bound(out, ref, f"fs={fs} S={S}")


@pytest.mark.parametrize("S", [6, 5])
@pytest.mark.parametrize("fs", [4, 8])
def test_float_path_shipped_statistics(gpu_ctx, float_cases, fs, S):
    """(x - mean) / std with the statistics table the package ships: the bound of frontend_ref.normalised_bound"""
    from dctfhe import frontend
    y, c1, c2, idx, ref = float_cases[fs, S]
    mean, std = frontend.load_stats()
    if fs == 4:                                                                           # 48 channels: the table's entries for them
        sel = frontend.normalize_indices(48)
        mean, std = mean[sel], std[sel]
    mean, std = mean.astype(np.float32), std.astype(np.float32)
    assert mean.size == 3 * fs * fs and (std > 0).all()
    out = gpu_ctx.dct_frontend(y, c1, c2, fs, idx, mean, std)
    R.assert_normalised_bound(out, ref, mean, std, f"fs={fs} S={S} shipped statistics")


def test_second_grid_stride_trip(gpu_ctx):
    """config #5's shape at batch 8 with block size 4: 8 x 48 x 112 x 112 = 4 816 896 outputs, more than the 16384 x 256 = 4 194 304
    threads a launch is capped at, so the last 622 592 outputs (most of image 7) are written on the loop's second trip"""
    fs, B, S, Sc = 4, 8, 112, 56
    rng = np.random.default_rng(112)
    y = rng.integers(0, 256, (B, fs * S, fs * S), dtype=np.uint8)
    c1 = rng.integers(0, 256, (B, fs * Sc, fs * Sc), dtype=np.uint8)
    c2 = rng.integers(0, 256, (B, fs * Sc, fs * Sc), dtype=np.uint8)
    allc = np.arange(16, dtype=np.int32)
    out = gpu_ctx.dct_frontend(y, c1, c2, fs, (allc, allc, allc), np.zeros(48), np.ones(48))
    assert out.size > 16384 * 256
    # f64 reference: its own error (a few 2^-53 x 16 terms x 1024) is far below the 2^-37 the bound already grants the kernel
    ref = R.float_reference(y, c1, c2, fs, (allc, allc, allc), dtype=np.float64)
    assert out.shape == ref.shape == (B, 48, S, S)
    tail = out.reshape(-1)[16384 * 256:]
    assert np.abs(tail).max() > 100                                                       # the second trip wrote coefficients, not nothing
    R.assert_unit_stats_bound(out, ref, "second trip")
