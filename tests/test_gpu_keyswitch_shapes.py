"""The key switch (csrc/kernels.h k_ks_decompose, k_ks_mfma) bit for bit against oracle.keyswitch on the tile edges the shipped path
crosses and tests/test_gpu_primitives.py (n <= 40, two column blocks) does not:
  * the shipped gadget shapes on a small big key: an XCD strip wider than one column block (cpx = ceil(column blocks / 8) > 1, with the
    early return of the workgroups past the last column block), the two-limb epilogue, two row blocks of which the second holds two rows;
  * a trailing half K-step: rows used R = deff lk = 64 (mod 128), where the staging of the last step reads zeros for its upper half;
  * the grid-stride loop of k_ks_decompose (its grid is capped at 65 536 workgroups of 256 words), for plain rows and for the row
    differences of a max pool (ks_src_diff) and for the row sums of a parity-split site (ks_src_sum);
  * the summed source (ks_src_sum, dctfhe_keyswitch_sum) at the shipped gadget shapes: two row strides, the second row set narrower
    than the first (a word of b at or beyond its width counts as zero), bodies whose sum wraps, and the prefix path at effective
    dimensions on either side of b's width."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D_SHAPES = 1024
# (n, lk, betak) -> byte limbs per key word (dctfhe.hip ks_limbs), 128-wide column blocks of limbs (n + 1), blocks per XCD strip
SHAPES = [
    dict(n=560, lk=5, betak=2, limbs=2, ncb=9, cpx=2),      # one-bit tiers B / Ba / Ba2
    dict(n=800, lk=9, betak=2, limbs=4, ncb=26, cpx=4),     # table tiers T6 / T6a / T5a
    dict(n=864, lk=6, betak=3, limbs=4, ncb=28, cpx=4),     # the p_error catalogue
]
SHAPE_IDS = ["n%d-lk%d-b%d" % (s["n"], s["lk"], s["betak"]) for s in SHAPES]


def _cent(x):
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


@pytest.fixture(scope="module")
def shape_keys(gpu_ctx):
    """one big key of 1024 bits, one tier per shipped gadget shape on a cheap ring"""
    from dctfhe.engine import Keys, make_params
    tiers = [dict(n=s["n"], k=1, logN=9, l=2, beta=12, lk=s["lk"], betak=s["betak"], lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -45) for s in SHAPES]
    k = Keys(gpu_ctx, make_params(D_SHAPES, max(s["n"] for s in SHAPES), tiers, 2.0 ** -50), seed=37)
    yield k
    k.close()


@pytest.fixture(scope="module")
def shape_inputs(shape_keys):
    """130 encryptions of 4-bit messages, and a copy with random top bytes in the mask words (every digit value occurs, the top ones too)"""
    rng = np.random.default_rng(6)
    phases = rng.integers(0, 16, 130).astype(np.uint64) << np.uint64(59)
    cts = shape_keys.encrypt(phases)
    wild = cts.copy()
    wild[:, :D_SHAPES] |= rng.integers(0, 2 ** 64, (130, D_SHAPES), dtype=np.uint64) & np.uint64(0xFF00000000000000)
    return phases, cts, wild


@pytest.mark.parametrize("tier", range(len(SHAPES)), ids=SHAPE_IDS)
def test_shipped_gadget_shapes_bit_exact(shape_keys, shape_inputs, oracle, tier):
    from dctfhe import params as P
    sh = SHAPES[tier]
    spec = P.TierSpec("s", n=sh["n"], k=1, logN=9, l=2, beta=12, lk=sh["lk"], betak=sh["betak"], lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -45)
    ncol_pad = -(-P.ks_limbs(spec) * (sh["n"] + 1) // 128) * 128
    assert (P.ks_limbs(spec), ncol_pad // 128, (ncol_pad // 128 + 7) // 8) == (sh["limbs"], sh["ncb"], sh["cpx"])   # the geometry this case is about
    phases, cts, wild = shape_inputs
    ksk = shape_keys.export_ksk(tier)
    assert ksk.shape == (D_SHAPES, sh["lk"], sh["n"] + 1)
    for shift in (0, 3):
        ref = oracle.keyswitch(wild << np.uint64(shift), ksk, sh["betak"])
        for count in (130, 1):            # 130: two row blocks, the second with two rows
            dev = shape_keys.keyswitch(tier, wild[:count], shift=shift)
            assert np.array_equal(dev, ref[:count]), (SHAPE_IDS[tier], shift, count, np.argwhere(dev != ref[:count])[:8])
    # the key is a key-switch key of the small secret: the message survives, with the noise the model prices for this gadget
    _, s = shape_keys.export_secret()
    small = shape_keys.keyswitch(tier, cts)
    assert np.array_equal(small, oracle.keyswitch(cts, ksk, sh["betak"]))
    err = np.abs(_cent(oracle.lwe_phase(s[: sh["n"]].copy(), sh["n"], small) - phases))
    sigma = math.sqrt(P.var_keyswitch(D_SHAPES, spec) + 2.0 ** -100)
    print(SHAPE_IDS[tier], "log2 of the largest error after the key switch %.2f, of the model's sigma %.2f" % (math.log2(err.max()), math.log2(sigma)))
    assert 6 * sigma < 2.0 ** -4            # (the five-level base-4 gadget of the one-bit tiers truncates at 2^-10: sigma 2^-7.3 at D = 1024)
    assert err.max() < 6 * sigma, (err.max(), sigma)


@pytest.mark.parametrize("tier,deff", [(0, 192), (1, 64), (1, 192)], ids=["lk5-deff192", "lk9-deff64", "lk9-deff192"])
def test_trailing_half_k_step_bit_exact(shape_keys, oracle, tier, deff):
    """R = deff lk = 64 (mod 128): the last K-step of k_ks_mfma has live rows in its lower half only.  Inputs are zero beyond deff, so the
    prefix call, the full-width call and the oracle give the same words."""
    sh = SHAPES[tier]
    assert (deff * sh["lk"]) % 128 == 64
    rng = np.random.default_rng(8 + deff)
    cts = rng.integers(0, 2 ** 64, (130, D_SHAPES + 1), dtype=np.uint64)
    cts[:, deff:D_SHAPES] = 0
    ref = oracle.keyswitch(cts << np.uint64(1), shape_keys.export_ksk(tier), sh["betak"])
    pref = shape_keys.keyswitch(tier, cts, shift=1, deff=deff)
    full = shape_keys.keyswitch(tier, cts, shift=1)
    assert np.array_equal(pref, ref), np.argwhere(pref != ref)[:8]
    assert np.array_equal(full, ref), np.argwhere(full != ref)[:8]


# ------------------------------------------------------------------------------------------ the summed source
def _dense(r, dim, D):
    """the ciphertexts that rows of dim mask words + body stand for, at D mask words: the words a row lacks are zero"""
    out = np.zeros((r.shape[0], D + 1), np.uint64)
    out[:, :dim] = r[:, :dim]
    out[:, D] = r[:, -1]
    return out


def _sum_reference(oracle, a, dim_a, b, dim_b, shift, body_add, ksk, betak):
    D = ksk.shape[0]
    host = (_dense(a, dim_a, D) + _dense(b, dim_b, D)) << np.uint64(shift)
    host[:, D] += np.uint64(body_add)
    return oracle.keyswitch(host, ksk, betak)


# (dim_b, deff, the first zero mask word of a): equal strides; b narrower, without and with the prefix path ending at b's width; a prefix
# that ends inside b's width (576 lk is a multiple of 64 for every lk, so each shape takes the cached column sums of 576 lk key rows)
SUM_CASES = [(1024, 0, 1024), (512, 0, 1024), (512, 512, 512), (640, 576, 576)]
SUM_BODY_ADD = (1 << 64) - (1 << 62)          # the -2^62 of the parity bootstrap


@pytest.fixture(scope="module")
def sum_inputs(shape_inputs):
    """two row sets from the wild rows (every digit value, the carry chains), the second in another order; every other pair of bodies wraps"""
    _, _, wild = shape_inputs
    a, b = wild.copy(), wild[::-1].copy()
    a[0::2, -1] |= np.uint64(1 << 63)
    b[0::2, -1] |= np.uint64(1 << 63)
    assert ((a[:, -1] + b[:, -1]) < a[:, -1]).sum() >= 65 and ((a[:, -1] + b[:, -1]) >= a[:, -1]).any()
    return a, b


@pytest.mark.parametrize("dim_b,deff,zero_from", SUM_CASES, ids=["db%d-deff%d" % c[:2] for c in SUM_CASES])
@pytest.mark.parametrize("tier", range(len(SHAPES)), ids=SHAPE_IDS)
def test_summed_source_bit_exact(shape_keys, sum_inputs, oracle, tier, dim_b, deff, zero_from):
    """dctfhe_keyswitch_sum == the oracle's key switch of ((a + b) << shift) + body_add made on the host"""
    sh = SHAPES[tier]
    assert deff == 0 or (deff * sh["lk"]) % 64 == 0         # else the library falls back to the full width: not the path this case is about
    a, b = sum_inputs
    a = a.copy()
    a[:, zero_from:D_SHAPES] = 0
    b = np.ascontiguousarray(np.concatenate([b[:, :dim_b], b[:, -1:]], axis=1))
    b[:, min(zero_from, dim_b):dim_b] = 0                   # the caller's promise covers the sum: nothing beyond deff in either
    assert deff == 0 or not (_dense(a, D_SHAPES, D_SHAPES) + _dense(b, dim_b, D_SHAPES))[:, deff:D_SHAPES].any()
    ksk = shape_keys.export_ksk(tier)
    for shift in (0, 3):
        ref = _sum_reference(oracle, a, D_SHAPES, b, dim_b, shift, SUM_BODY_ADD, ksk, sh["betak"])
        dev = shape_keys.keyswitch_sum(tier, a, b, shift=shift, body_add=SUM_BODY_ADD, deff=deff)
        assert np.array_equal(dev, ref), (SHAPE_IDS[tier], dim_b, deff, shift, np.argwhere(dev != ref)[:8])


@pytest.mark.parametrize("tier", range(len(SHAPES)), ids=SHAPE_IDS)
def test_summed_source_with_a_zero_second_operand_is_the_plain_key_switch(shape_keys, sum_inputs, tier):
    a, _ = sum_inputs
    narrow = a.copy()
    narrow[:, 512:D_SHAPES] = 0
    for rows, deff in ((a, 0), (narrow, 512)):
        for shift in (0, 3):
            got = shape_keys.keyswitch_sum(tier, rows, np.zeros((rows.shape[0], 512 + 1), np.uint64), shift=shift, deff=deff)
            assert np.array_equal(got, shape_keys.keyswitch(tier, rows, shift=shift, deff=deff)), (SHAPE_IDS[tier], deff, shift)


# ------------------------------------------------------------------------------------------ grid-stride decompose
D_BIG, ROWS_BIG = 8192, 2112          # 2112 x 8192 words > 65 536 x 256: the decompose grid walks its loop twice (the seam is at row 2048)


@pytest.fixture(scope="module")
def big(gpu_ctx):
    from dctfhe.engine import Keys, make_params
    assert ROWS_BIG * D_BIG > 65536 * 256
    tier = dict(n=40, k=1, logN=9, l=2, beta=12, lk=4, betak=4, lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -45)
    k = Keys(gpu_ctx, make_params(D_BIG, 40, [tier], 2.0 ** -50), seed=39)
    rows = np.random.default_rng(9).integers(0, 2 ** 64, (ROWS_BIG, D_BIG + 1), dtype=np.uint64)
    yield k, rows, k.export_ksk(0)
    k.close()


# the first rows, the rows either side of the seam of the grid-stride loop, the last rows: 64 in all
SAMPLE = np.concatenate([np.arange(0, 16), np.arange(2032, 2064), np.arange(ROWS_BIG - 16, ROWS_BIG)])


def test_decompose_grid_stride_rows(big, oracle):
    keys, rows, ksk = big
    whole = keys.keyswitch(0, rows, shift=2)
    for c0 in range(0, ROWS_BIG, 64):
        part = keys.keyswitch(0, rows[c0:c0 + 64], shift=2)
        assert np.array_equal(whole[c0:c0 + 64], part), (c0, np.argwhere(whole[c0:c0 + 64] != part)[:8])
    assert np.array_equal(whole[SAMPLE], oracle.keyswitch(rows[SAMPLE] << np.uint64(2), ksk, 4))


def test_decompose_grid_stride_row_differences(big, oracle):
    """ks_src_diff through the same loop: index pairs that reach across the seam in both directions"""
    keys, rows, ksk = big
    rng = np.random.default_rng(10)
    ia = np.arange(ROWS_BIG, dtype=np.int32)
    ib = ((ia + 1024 + rng.integers(0, 64, ROWS_BIG)) % ROWS_BIG).astype(np.int32)       # rows 988 .. 2047 pair with rows past the seam, and back
    assert ((ia < 2048) & (ib >= 2048)).any() and ((ia >= 2048) & (ib < 2048)).any()
    body_add = 1 << 62
    dev = keys.keyswitch_diff(0, rows, ia, ib, shift=1, body_add=body_add)
    diff = rows[ia] - rows[ib]
    host = diff << np.uint64(1)
    host[:, D_BIG] += np.uint64(body_add)
    ref = oracle.keyswitch(host, ksk, 4)              # the oracle on the differences made on the host, all rows
    assert np.array_equal(dev, ref), np.unique(np.argwhere(dev != ref)[:, 0])[:16]


ROWS_SUM, DIM_SUM_A, DIM_SUM_B, DEFF_SUM = 70000, 320, 128, 256     # 70 000 x 256 words > 65 536 x 256: the seam is at row 65 536


def test_decompose_grid_stride_row_sums(big, oracle):
    """ks_src_sum through the same loop, at a narrow effective dimension: rows of 320 and 128 mask words, the first 256 switched"""
    keys, _, ksk = big
    assert ROWS_SUM * DEFF_SUM > 65536 * 256 and (DEFF_SUM * 4) % 64 == 0
    rng = np.random.default_rng(11)
    a = rng.integers(0, 2 ** 64, (ROWS_SUM, DIM_SUM_A + 1), dtype=np.uint64)
    a[:, DEFF_SUM:DIM_SUM_A] = 0
    b = rng.integers(0, 2 ** 64, (ROWS_SUM, DIM_SUM_B + 1), dtype=np.uint64)
    body_add = 1 << 62
    whole = keys.keyswitch_sum(0, a, b, shift=1, body_add=body_add, deff=DEFF_SUM)
    half = ROWS_SUM // 2                  # each half stays under the grid cap: no loop
    assert half * DEFF_SUM <= 65536 * 256
    for c0 in (0, half):
        part = keys.keyswitch_sum(0, a[c0:c0 + half], b[c0:c0 + half], shift=1, body_add=body_add, deff=DEFF_SUM)
        assert np.array_equal(whole[c0:c0 + half], part), (c0, np.unique(np.argwhere(whole[c0:c0 + half] != part)[:, 0])[:16])
    sample = np.concatenate([np.arange(0, 16), np.arange(65536 - 16, 65536 + 16), np.arange(ROWS_SUM - 16, ROWS_SUM)])
    ref = _sum_reference(oracle, a[sample], DIM_SUM_A, b[sample], DIM_SUM_B, 1, body_add, ksk, 4)
    assert np.array_equal(whole[sample], ref), np.unique(np.argwhere(whole[sample] != ref)[:, 0])[:16]
