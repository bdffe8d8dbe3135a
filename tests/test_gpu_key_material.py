"""Key material against its definition (include/dctfhe.h, "Generator streams of the key material" and the Fourier-key layout):

  2. bootstrap keys: every inspected row, in the standard form (export_bsk) and in the decompressed body form (decompress_bsk of the
     compressed blob), has the generator's words as masks, decrypts under the exported secret to bit 2^(64 - beta (lev + 1)) at
     coefficient 0 of polynomial p plus a noise polynomial E; E is Gaussian at glwe_sigma (variance, mean, kurtosis, maximum), differs
     from row to row, from tier to tier and across the 64 MB staging chunks key generation works in, and is the same in both forms;
  3. fresh encryptions, the sampler and the key-switch-key noise, the same way;
  4. the Fourier form of the bootstrap key -- what every bootstrap multiplies with -- against a long-double transform of the exported
     standard key, one case per transform geometry the library instantiates, judged against numpy's own double-precision transform.

Everything the tests expect is restated in tests/key_material_ref.py from the header; nothing is imported from the kernels.  The bands
are derived (5 standard deviations of each estimator), not measured.  Measured figures are printed and, with DCTFHE_MEASURE_DIR set,
written to key_material.json (profiles/key_material.json is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import key_material_ref as K

pytestmark = pytest.mark.gpu

U = np.uint64
OUT = os.environ.get("DCTFHE_MEASURE_DIR")
MEASURED = {"fourier": {}, "noise": {}}
NONCE = bytes(range(100, 116))


def _record(kind, name, rec):
    MEASURED[kind][name] = rec
    print("key_material.json", json.dumps({kind: {name: rec}}))
    if OUT:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "key_material.json"), "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _draws(ctx, key, stream, idx0, count):
    """`count` words of the generator at (key, stream, idx0 ...), from the device"""
    out = np.empty(count, U)
    assert ctx.L.dctfhe_rng_device(ctx.h, bytes(key), C.c_uint64(stream), C.c_uint64(idx0), C.c_size_t(count), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _blob_pub(blob):
    """the public generator key a compressed evaluation-key blob carries after its parameters"""
    from dctfhe import _lib
    off = 16 + C.sizeof(_lib.Params)
    return blob[off:off + 32].tobytes()


def _tier(logN, k, l, beta, n, unroll=1, glwe_sigma=2.0 ** -40, lk=2, betak=4, lwe_sigma=2.0 ** -20):
    return dict(n=n, k=k, logN=logN, l=l, beta=beta, lk=lk, betak=betak, lwe_sigma=lwe_sigma, glwe_sigma=glwe_sigma, unroll=unroll)


def _blocks(t):
    return 3 * t["n"] // 2 if t["unroll"] == 2 else t["n"]


def _key_bits(oracle, s, t):
    """the bit each key block encrypts: the small key's, or the pair secret's for unroll 2"""
    s = s[:t["n"]].copy()
    if t["unroll"] != 2:
        return s
    bits = oracle.pair_secret(s)
    assert np.array_equal(bits, K.pair_secret(s))
    return bits


# ------------------------------------------------------------------------------------------ 2. bootstrap keys
def _inspect(ctx, ti, t, S, bits, pub, std, dec, picks, name):
    """the rows `picks` = [(block, r)] of a key in both forms: masks, phases, the same noise in both forms.
    Returns (E [rows, N] int64, the rows' mask draws [rows, k, N])."""
    k, l, beta, N = t["k"], t["l"], t["beta"], 1 << t["logN"]
    mask_stream, _ = K.bsk_streams(ti)
    rows_std = np.stack([std[b, r] for b, r in picks])
    rows_dec = np.stack([dec[b, r] for b, r in picks])
    draws = np.stack([_draws(ctx, pub, mask_stream, K.bsk_mask_index(b, r, k, l, N), k * N).reshape(k, N) for b, r in picks])
    want_std = draws.copy()
    pt = np.zeros((len(picks), N), U)                   # the expected plaintext, in phase terms
    for x, (b, r) in enumerate(picks):
        p, lev = divmod(r, l)
        g = U(1 << (64 - beta * (lev + 1)))
        if bits[b]:
            if p < k:                                   # the gadget term sits in mask polynomial p: - bit g S_p in the phase
                want_std[x, p, :1] += g
                pt[x] = U(0) - g * K.key_poly(S, p, N)
            else:
                pt[x, :1] = g
    assert np.array_equal(rows_std[:, :k], want_std), (name, "standard form: masks are not the generator's words (+ bit g at coefficient 0 of polynomial p)")
    assert np.array_equal(rows_dec[:, :k], draws), (name, "body form: masks are not the generator's words")
    E_std = (K.glwe_phase(rows_std, S, k, N) - pt).view(np.int64)
    E_dec = (K.glwe_phase(rows_dec, S, k, N) - pt).view(np.int64)
    assert np.array_equal(E_std, E_dec), (name, "the two forms of a row carry different noise")
    for x, (b, r) in enumerate(picks):
        if r // l == k:
            assert np.array_equal(rows_std[x], rows_dec[x]), (name, b, r, "a p = k row does not decompress bit for bit")
    return E_std, draws


def _no_shared_draws(E, draws, sigma, name):
    """no two rows share a mask polynomial, and their noise polynomials are uncorrelated"""
    N = E.shape[1]
    polys = draws.reshape(-1, N)
    assert len({m.tobytes() for m in polys}) == polys.shape[0], (name, "two rows share a mask polynomial")
    if sigma > 0:
        c = K.max_abs_corr(E)
        print("%s: largest |corr| between two of %d noise polynomials %.3f (band %.3f)" % (name, E.shape[0], c, K.corr_band(N)))
        assert c < K.corr_band(N), (name, "noise shared between rows", c)
        return c
    return 0.0


BSK_CASES = [
    # logN, k, l, beta, n, unroll, glwe_sigma
    pytest.param(8, 2, 2, 14, 5, 1, 2.0 ** -40, id="N256-k2-l2"),              # two mask polynomials, the gadget term inside one
    pytest.param(9, 1, 3, 12, 6, 1, 2.0 ** -40, id="N512-k1-l3"),
    pytest.param(11, 1, 4, 10, 6, 1, 2.0 ** -40, id="N2048-k1-l4"),
    pytest.param(10, 2, 1, 23, 6, 2, 2.0 ** -40, id="N1024-k2-l1-u2"),         # the pair secret with k = 2
    pytest.param(11, 1, 3, 12, 6, 2, 2.0 ** -40, id="N2048-k1-l3-u2"),
    pytest.param(12, 1, 1, 22, 6, 2, 2.0 ** -40, id="N4096-k1-l1-u2"),
    pytest.param(9, 1, 3, 12, 6, 1, 2.0 ** -62, id="N512-k1-l3-sigma62"),      # 4 units of 2^-64: the 1/12 of the rounding counts
    pytest.param(8, 2, 2, 14, 5, 1, 0.0, id="N256-k2-l2-sigma0"),
]


@pytest.mark.parametrize("logN,k,l,beta,n,unroll,sigma", BSK_CASES)
def test_bootstrap_key_rows_are_encryptions_of_the_key_bits(gpu_ctx, oracle, request, logN, k, l, beta, n, unroll, sigma):
    from dctfhe.engine import ClientKey, make_params
    name, N = request.node.callspec.id, 1 << logN
    t = _tier(logN, k, l, beta, n, unroll, sigma)
    ck = ClientKey(gpu_ctx, make_params(k * N, n, [t], 2.0 ** -50), seed=300 + logN + k + l)
    try:
        S, s = ck.export_secret()
        bits = _key_bits(oracle, s, t)
        assert bits.size == _blocks(t) and 0 < bits.sum() < bits.size, (name, "the test key needs both bit values")
        blob = ck.export_eval_keys_compressed()
        std, dec = ck.export_bsk(0), gpu_ctx.decompress_bsk(blob, 0)
        picks = [(b, r) for b in range(_blocks(t)) for r in range((k + 1) * l)]                      # every row of the short key
        E, draws = _inspect(gpu_ctx, 0, t, S, bits, _blob_pub(blob), std, dec, picks, name)
        st = K.check_noise(E, sigma, name)
        st["max_corr"] = _no_shared_draws(E, draws, sigma, name)
        _record("noise", "bsk-" + name, st)
    finally:
        ck.close()


def test_two_tiers_of_one_shape_share_no_draw(gpu_ctx, oracle):
    """the tier index is part of the stream id: the keys of two identical tiers have other masks and independent noise"""
    from dctfhe.engine import ClientKey, make_params
    t = _tier(8, 2, 2, 14, 5)
    N, rows = 256, 6
    ck = ClientKey(gpu_ctx, make_params(512, 5, [t, dict(t)], 2.0 ** -50), seed=77)
    try:
        S, s = ck.export_secret()
        bits = _key_bits(oracle, s, t)
        blob = ck.export_eval_keys_compressed()
        picks = [(b, r) for b in range(5) for r in range(rows)]
        got = [_inspect(gpu_ctx, ti, t, S, bits, _blob_pub(blob), ck.export_bsk(ti), gpu_ctx.decompress_bsk(blob, ti), picks, "tier %d" % ti)
               for ti in (0, 1)]
        E = np.concatenate([got[0][0], got[1][0]])
        draws = np.concatenate([got[0][1], got[1][1]])
        K.check_noise(E, t["glwe_sigma"], "two tiers")
        _no_shared_draws(E, draws, t["glwe_sigma"], "two tiers")
        assert K.bsk_streams(0) != K.bsk_streams(1)
    finally:
        ck.close()


def test_bootstrap_key_across_the_staging_chunks(gpu_ctx, oracle):
    """Key generation stages the standard-domain key in a 64 MB buffer, a whole number of key blocks per pass.  N = 8192, k = 1, l = 3:
    a block is (k + 1) l = 6 rows; in standard form (2 polynomials per row) 6 * 2 * 8192 * 8 = 786 432 bytes, 85 blocks per pass
    (85.3 fit); in body form (1 polynomial per row) 393 216 bytes, 170 blocks per pass.  A key of n = 172 blocks crosses both: the rows
    on either side of blocks 85 and 170 must come from the global row index -- a pass that restarted its indices would hand out the
    first pass's masks and noise a second time, and the difference of two such rows is noise-free.
    Inspected: blocks 0, 84 | 85, 86, 169 | 170, 171, a row with p < k and a row with p = k of each -- in the standard form, the
    decompressed body form, and (the path that stages the standard form in chunks) the Fourier key of generate_eval_keys against the
    long-double transform of the exported standard rows."""
    from dctfhe.engine import Keys, make_params
    logN, k, l, beta, n = 13, 1, 3, 11, 172
    N, M = 1 << logN, 1 << (logN - 1)
    staging = 64 << 20
    chunk_std, chunk_body = staging // ((k + 1) * l * (k + 1) * N * 8), staging // ((k + 1) * l * N * 8)
    assert (chunk_std, chunk_body) == (85, 170) and chunk_std < chunk_body < n
    t = _tier(logN, k, l, beta, n, lk=1, betak=4)
    cp = make_params(k * N, n, [t], 2.0 ** -50)
    keys = Keys(gpu_ctx, cp, seed=13)
    try:
        S, s = keys.export_secret()
        bits = _key_bits(oracle, s, t)
        blocks = [0, 84, 85, 86, 169, 170, 171]
        assert 0 < bits[blocks].sum() < len(blocks), "the inspected blocks need both bit values"
        picks = [(b, r) for b in blocks for r in (1, 5)]                    # r = 1: p = 0 < k, level 1; r = 5: p = k, level 2
        blob_c = keys.export_eval_keys_compressed()
        std, dec = keys.export_bsk(0), gpu_ctx.decompress_bsk(blob_c, 0)
        E, draws = _inspect(gpu_ctx, 0, t, S, bits, _blob_pub(blob_c), std, dec, picks, "chunks")
        st = K.check_noise(E, t["glwe_sigma"], "chunks")
        st["max_corr"] = _no_shared_draws(E, draws, t["glwe_sigma"], "chunks")
        del dec, blob_c
        # the Fourier key of the same rows: generated chunk by chunk from the standard form
        fk, _ = _fourier_key(keys.to_blob(), cp, 0)
        P = {c[:3]: c[3] for c in K.pbs_cases()[0]}[(logN, k, l)]
        q = np.array([(b * (k + 1) * l + r) * (k + 1) + j for b, r in picks for j in range(k + 1)])
        polys = np.stack([std[b, r, j] for b, r in picks for j in range(k + 1)])
        ref, yard = K.fourier_key_reference(polys, logN, P)
        rms, mx, rel = K.error_ratios(fk[q], ref, yard)
        print("chunks: Fourier key of the inspected rows: rms ratio %.2f, max ratio %.2f" % (rms, mx))
        st.update(fourier_rms_ratio=rms, fourier_max_ratio=mx)
        _record("noise", "bsk-chunks-N8192-k1-l3-n172", st)
        assert rms <= 3.0 and mx <= 4.0, (rms, mx)
    finally:
        keys.close()


# ------------------------------------------------------------------------------------------ 3. fresh encryptions, sampler, key-switch keys
def _client(ctx, input_dim, input_sigma, seed=21):
    from dctfhe.engine import ClientKey, make_params
    ck = ClientKey(ctx, make_params(512, 40, [_tier(8, 2, 2, 14, 40)], input_sigma, input_dim), seed=seed)
    ck.set_encrypt_nonce(NONCE)
    return ck


def _host_phase(rows, S):
    """body - <a, S> of rows [count, dim + 1] under the first dim key bits, in numpy"""
    dim = rows.shape[1] - 1
    return rows[:, dim] - (rows[:, :dim] * S[:dim].astype(U)).sum(axis=1, dtype=U)


def _encrypt_at(ck, counter, ph, dim):
    ck.set_encrypt_counter(counter)
    return ck.encrypt(ph, dim)


def _mask_source(ck, counter):
    """(mask key, stream) of the encryption call at `counter`: what the seeded form of that call ships"""
    ck.set_encrypt_counter(counter)
    sc = ck.encrypt_seeded(np.zeros(1, U))
    return sc.key, sc.stream


@pytest.mark.parametrize("input_dim", [16, 0])
def test_fresh_encryptions_masks_phases_and_noise(gpu_ctx, input_dim):
    D, sigma = 512, 2.0 ** -20
    ck = _client(gpu_ctx, input_dim, sigma)
    try:
        S, _ = ck.export_secret()
        dim = ck.input_dim
        assert dim == (input_dim or D)
        count = 65536 if dim == 16 else 4096               # compact rows of 17 words; full rows of 513
        ph = np.random.default_rng(3).integers(0, 2 ** 64, count, dtype=U)
        rows = _encrypt_at(ck, 5, ph, dim)
        E = (_host_phase(rows, S) - ph).view(np.int64)
        st = K.check_noise(E, sigma, "encrypt input_dim %d" % input_dim)
        # masks: generator word (mask key, stream, c (D + 1) + j) -- the first 4096 rows and the last
        key, stream = _mask_source(ck, 5)
        head = _draws(gpu_ctx, key, stream, 0, 4096 * (D + 1)).reshape(4096, D + 1)
        assert np.array_equal(rows[:4096, :dim], head[:, :dim])
        assert np.array_equal(rows[-1, :dim], _draws(gpu_ctx, key, stream, (count - 1) * (D + 1), dim))
        # the full-width form of the same call: the same ciphertexts, zeros from dim_eff on
        full = _encrypt_at(ck, 5, ph[:4096], None)
        assert full.shape == (4096, D + 1) and np.array_equal(full[:, :dim], rows[:4096, :dim]) and np.array_equal(full[:, D], rows[:4096, dim])
        assert not full[:, dim:D].any()
        # a second call: other masks, independent noise
        rows2 = _encrypt_at(ck, 6, ph, dim)
        E2 = (_host_phase(rows2, S) - ph).view(np.int64)
        K.check_noise(E2, sigma, "encrypt input_dim %d, second call" % input_dim)
        assert not np.any(rows2[:, :dim] == rows[:, :dim])
        c = K.max_abs_corr(np.stack([E, E2]))
        assert c < K.corr_band(count), ("two calls share noise", c)
        st["corr_two_calls"] = c
        _record("noise", "encrypt-input_dim%d" % input_dim, st)
    finally:
        ck.close()


def test_fresh_encryptions_at_the_edge_sigmas(gpu_ctx):
    """sigma 2^-62 is 4 units of 2^-64: the draw's rounding to an integer is a fortieth of the variance; sigma 0: no noise at all"""
    count = 65536
    ph = np.random.default_rng(4).integers(0, 2 ** 64, count, dtype=U)
    ck = _client(gpu_ctx, 16, 2.0 ** -62)
    try:
        S, _ = ck.export_secret()
        E = (_host_phase(_encrypt_at(ck, 1, ph, 16), S) - ph).view(np.int64)
        _record("noise", "encrypt-sigma62", K.check_noise(E, 2.0 ** -62, "encrypt sigma 2^-62"))
    finally:
        ck.close()
    ck = _client(gpu_ctx, 16, 0.0)
    try:
        S, _ = ck.export_secret()
        rows = _encrypt_at(ck, 1, ph, 16)
        assert np.array_equal(rows[:, 16], (rows[:, :16] * S[:16].astype(U)).sum(axis=1, dtype=U) + ph)
    finally:
        ck.close()


def test_seeded_form_at_a_mask_width_that_is_no_multiple_of_eight(gpu_ctx):
    """test_gpu_seeded.py::test_seeded_encryption_expands_to_encrypt_rows holds encrypt_seeded + expand_seeded to encrypt word for word
    at input_dim 1024 (D 1024) and 2048 (D 8192), counts up to 100 003: rows D + 1 generator words apart, so the eight-word generator
    blocks straddle rows there.  Both widths are multiples of 8; here the width whose last block is partial: 13 of D = 512."""
    ph = np.random.default_rng(6).integers(0, 2 ** 64, 1001, dtype=U)
    a, b = _client(gpu_ctx, 13, 2.0 ** -20), _client(gpu_ctx, 13, 2.0 ** -20)
    try:
        a.set_encrypt_counter(9)
        sc = a.encrypt_seeded(ph)
        want = _encrypt_at(b, 9, ph, 13)
        assert sc.input_dim == 13 and np.array_equal(gpu_ctx.expand_seeded(sc), want)
        wide = gpu_ctx.expand_seeded(sc, 512)
        assert np.array_equal(wide[:, :13], want[:, :13]) and not wide[:, 13:512].any() and np.array_equal(wide[:, 512], want[:, 13])
        S, _ = a.export_secret()
        K.check_noise((_host_phase(want, S) - ph).view(np.int64), 2.0 ** -20, "seeded, 13 mask words", with_kurtosis=False)
    finally:
        a.close()
        b.close()


def test_key_switch_key_noise(gpu_ctx):
    """every row of a key-switch key: masks on the 2^-(8 limbs) grid from the generator, S_i 2^(64 - betak (lev + 1)) plus noise of
    variance lwe_sigma^2 + grid^2 / 12 (the draw, then the rounding of the body to the grid) under the small key.  One tier with 2 limbs
    (5 levels of base 4, as the one-bit tiers ship), one with 4 (9 levels)."""
    from dctfhe.engine import Keys, make_params
    D, n = 512, 40
    tiers = [_tier(8, 2, 2, 14, n, lk=5, betak=2, lwe_sigma=2.0 ** -13), _tier(8, 2, 2, 14, n, lk=9, betak=2, lwe_sigma=2.0 ** -24)]
    keys = Keys(gpu_ctx, make_params(D, n, tiers, 2.0 ** -50), seed=31)
    try:
        S, s = keys.export_secret()
        pub = _blob_pub(keys.export_eval_keys_compressed())
        seen = set()
        for ti, t in enumerate(tiers):
            lk, betak, limbs = t["lk"], t["betak"], K.ks_limbs(t["lk"], t["betak"])
            seen.add(limbs)
            grid_bits = 64 - 8 * limbs
            ksk = keys.export_ksk(ti)
            assert ksk.shape == (D, lk, n + 1)
            rows = ksk.reshape(D * lk, n + 1)
            masks = _draws(gpu_ctx, pub, K.ksk_streams(ti)[0], 0, D * lk * (n + 1)).reshape(D * lk, n + 1)[:, :n]
            assert np.array_equal(rows[:, :n], masks & ~U((1 << grid_bits) - 1)), (ti, "masks are not the generator's words on the grid")
            assert not (rows[:, n] & U((1 << grid_bits) - 1)).any(), (ti, "a body off the grid")
            ph = _host_phase(rows, s[:n]).reshape(D, lk)
            want = np.stack([S.astype(U) << U(64 - betak * (lev + 1)) for lev in range(lk)], axis=1)
            E = (ph - want).view(np.int64)
            st = K.check_noise(E, t["lwe_sigma"], "key-switch key, %d limbs" % limbs, grid_bits=grid_bits, with_kurtosis=False)
            _record("noise", "ksk-%dlimbs" % limbs, st)
        assert seen == {2, 4}
    finally:
        keys.close()


# ------------------------------------------------------------------------------------------ 4. Fourier keys
def _fourier_key(blob, cp, ti):
    """the Fourier bootstrap key of tier ti inside an evaluation-key blob, [npoly, M] complex, and the offset at which it ends"""
    from dctfhe import _lib
    off = 16 + C.sizeof(_lib.Params)
    for i in range(cp.n_tiers):
        t = cp.tiers[i]
        if t.ksk_share < 0:
            off += cp.D * t.lk * (t.n + 1) * 8
        npoly = (3 * t.n // 2 if t.unroll == 2 else t.n) * (t.k + 1) * t.l * (t.k + 1)
        M = 1 << (t.logN - 1)
        if i == ti:
            return np.frombuffer(blob, np.complex128, npoly * M, off).reshape(npoly, M), off + npoly * M * 16
        off += npoly * M * 16
    raise IndexError(ti)


def _fourier_cases():
    cases, mb = K.pbs_cases()
    P_of = {c[:3]: c[3] for c in cases}
    out = [pytest.param(logN, k, l, P, 1, id="N%d-k%d-l%d-P%d" % (1 << logN, k, l, P)) for logN, k, l, P in cases]
    out += [pytest.param(lg, 1, 1, P_of[(lg, 1, 1)], 2, id="N%d-k1-l1-P%d-u2" % (1 << lg, P_of[(lg, 1, 1)])) for lg in mb]
    # the two general two-bit forms: their keys go through the transform of their (logN, k, l)
    out += [pytest.param(11, 1, 3, P_of[(11, 1, 3)], 2, id="N2048-k1-l3-P8-u2"), pytest.param(10, 2, 1, P_of[(10, 2, 1)], 2, id="N1024-k2-l1-P8-u2")]
    return out


FOURIER_BETA = {1: 22, 2: 16, 3: 11, 4: 10}


@pytest.mark.parametrize("logN,k,l,P,unroll", _fourier_cases())
def test_fourier_key_against_long_double_transform(gpu_ctx, request, logN, k, l, P, unroll):
    """Every polynomial (N <= 2048) or 16 of them with the first and the last (larger N): |device - reference| against
    |numpy f64 - reference|, rms within 3x and maximum within 4x.  The thread program compiled for the host measures rms ratios of
    1.2 - 1.7 and maximum ratios of 1.1 - 2.0 (tests/test_key_material_host.py); the factors are about twice that, and a
    single-precision constant anywhere in the transform is off by about 10^8 (one twiddle pass rounded through float: ratios of
    3.6e8 - 8.2e8).  Measured on an MI355X: 1.17 - 1.55 and 1.09 - 1.84 over the 22 cases (profiles/key_material.json).
    Keys of 3 blocks (n = 3; unroll 2: n = 2).  k_bsk_fourier transforms GROUPS polynomials per workgroup and clamps the last
    workgroup's spare groups to the last polynomial; (k + 1)^2 l * 3 polynomials are no multiple of GROUPS -- so the clamp runs -- at
    N = 256 k 2 l 2 (54 of 8), N = 512 k 1 l 3 (36 of 8) and N = 1024 k 2 l 1 (27 of 4).  The other shapes cannot take it: with k = 1
    the count 4 l n is a multiple of their GROUPS (8, 4 or 2) for every n, N = 1024 k 2 l 2 has 18 n of 2, and from N = 4096 on a
    workgroup holds one polynomial."""
    from dctfhe.engine import EvalKeys, Keys, make_params
    name, N, M = request.node.callspec.id, 1 << logN, 1 << (logN - 1)
    n = 2 if unroll == 2 else 3
    t = _tier(logN, k, l, FOURIER_BETA[l], n, unroll, lk=1, betak=4)
    cp = make_params(k * N, n, [t], 2.0 ** -50)
    keys = Keys(gpu_ctx, cp, seed=500 + logN)
    try:
        blob = keys.to_blob()
        fk, end = _fourier_key(blob, cp, 0)
        npoly = 3 * (k + 1) * l * (k + 1)
        assert fk.shape == (npoly, M) and end == blob.size, (name, "the blob's bootstrap key is not exactly blocks (k+1) l (k+1) polynomials")
        std = keys.export_bsk(0).reshape(npoly, N)
        if logN <= 11:
            q = np.arange(npoly)
        else:
            rest = np.random.default_rng(logN).choice(np.arange(1, npoly - 1), min(14, npoly - 2), replace=False)
            q = np.concatenate([[0], np.sort(rest), [npoly - 1]])
        ref, yard = K.fourier_key_reference(std[q], logN, P)
        rms, mx, rel = K.error_ratios(fk[q], ref, yard)
        print("%s: %d polynomials, rms ratio %.2f, max ratio %.2f, yardstick %.2e relative rms" % (name, q.size, rms, mx, rel))
        _record("fourier", name, dict(polys=int(q.size), rms_ratio=rms, max_ratio=mx, yardstick_rel_rms=rel))
        assert rel < 1e-15, (name, "the yardstick is no double-precision transform", rel)
        assert rms <= 3.0, (name, "rms error over numpy's f64 transform", rms)
        assert mx <= 4.0, (name, "largest error over numpy's f64 transform", mx)
        # importing the blob and exporting it again changes nothing
        again = EvalKeys.from_blob(gpu_ctx, blob)
        try:
            assert np.array_equal(again.to_blob(), blob), (name, "import + export is not the identity")
        finally:
            again.close()
    finally:
        keys.close()
