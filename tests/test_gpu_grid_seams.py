"""The streaming kernels past their first grid-stride trip.  Every element-wise kernel of the levelled and clear-mode paths loops under a
launch capped at 16384 blocks of 256 threads (`ew_grid()`, `launch_expand()` in csrc/dctfhe.hip): one trip covers T = 4 194 304 work items,
and production tensors take many (one ResNet-20 tensor: 8).  The stand-alone tests of these kernels stay far below T, so the words a
kernel writes from its second trip on were checked only by the end-to-end runs.  Here each kernel runs ONE AT A TIME on the smallest shape
that crosses T at a production row stride (513, 1025 or 2049 words, all odd), with T strictly inside a row and a partial last trip; the
shapes and their work counts are tests/grid_seam_cases.py, which tests/test_grid_seams_host.py holds to the source and to these rules.
Every test recomputes its work counts from the arrays (or the session's strides) it really uses and asserts the rules before it launches.

Integer arithmetic throughout: whole outputs, np.array_equal, no tolerance.  References: numpy uint64 wrap-around arithmetic, the numpy
interpreter oracle/circuit_ref.py, the host generator dctfhe_rng_host, and the host twins of `simulate`, the ring pack and the
public-key draws.  A failure names the first wrong flat index and the trip (index // T) it belongs to."""
import ctypes as C

import numpy as np
import pytest

import grid_seam_cases as G

pytestmark = pytest.mark.gpu
U = np.uint64
T = G.T


# ------------------------------------------------------------------------------------------ helpers
def same(got, want, what, item=None):
    """whole-array equality; item: flat output index -> the kernel's work item, where the two differ (the trip is item // T)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    g, w = got.reshape(-1), want.reshape(-1)
    bad = np.flatnonzero(g != w)
    first = int(bad[0])
    it = first if item is None else int(item(first))
    raise AssertionError(f"{what}: {bad.size} of {w.size} words differ; first at flat index {first} (work item {it}, trip {it // T}): "
                         f"device {int(g[first]):#x}, reference {int(w[first]):#x}; last at {int(bad[-1])}")


def check(case, kernel, W, group, trips=2, which=0):
    """the rules on the work count this test computed itself, and the table's entry for it"""
    listed = [l for l in case.loops() if l.kernel == kernel][which]
    l = G.Loop(kernel, W, group, trips, listed.whole_blocks, listed.on_boundary)
    l.check()
    assert (l.W, l.group, l.trips) == (listed.W, listed.group, listed.trips), (case.name, kernel, l.W, listed.W)


def rows(rng, count, dim):
    """random rows of dim mask words + body; what lies between a row's effective dimension and its body is GARBAGE on purpose: the
    kernels must not read it"""
    return rng.integers(0, 2 ** 64, (count, dim + 1), dtype=U)


def dense(r, deff, dim_o):
    """the ciphertext a stored row stands for, widened to dim_o mask words: words from deff on are zero"""
    out = np.zeros((r.shape[0], dim_o + 1), U)
    out[:, :deff] = r[:, :deff]
    out[:, dim_o] = r[:, -1]
    return out


def rng_words(L, key, stream, first, count):
    """generator words [first, first + count) of (key, stream) from the host generator, in 8 slices on 8 threads (the generator is
    counter-based and the call holds no interpreter lock: 33 M words take 4 s on one thread)"""
    from concurrent.futures import ThreadPoolExecutor
    out = np.empty(count, U)
    cuts = [count * i // 64 * 8 for i in range(8)] + [count]           # slices start on a generator block of 8 words

    def fill(i):
        lo, hi = cuts[i], cuts[i + 1]
        return hi == lo or L.dctfhe_rng_host(key, C.c_uint64(stream), C.c_uint64(first + lo), C.c_size_t(hi - lo), out[lo:hi].ctypes.data_as(C.c_void_p)) == 0
    with ThreadPoolExecutor(8) as pool:
        assert all(pool.map(fill, range(8)))
    return out


_hip = None


def read_rows(sess, tensor):
    """the stored words of a session's tensor [rows, stride], copied from the pointer dctfhe_session_tensor hands out with the HIP runtime
    the library itself has loaded (the engine's uploads and runs are synchronous: the words are there)"""
    global _hip
    if _hip is None:
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        assert paths, "the HIP runtime is not loaded"
        _hip = C.CDLL(paths[0])
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    dev, stride, n = sess.tensor(tensor)
    assert dev and stride >= 1
    out = np.empty((n, stride), U)
    assert _hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev), out.nbytes, 2) == 0      # 2: device to host
    return out


def flagged(call):
    """run `call`; -> did the clear engine report a message outside its padded range (the outputs are computed all the same)"""
    from dctfhe._lib import DctfheError
    try:
        call()
        return False
    except DctfheError as e:
        assert "left its padded range" in str(e), str(e)
        return True


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    k = Keys(gpu_ctx, P.to_c_params(P.test_params()), seed=3)
    yield k
    k.close()


# ------------------------------------------------------------------------------------------ 1. stand-alone primitives
@pytest.mark.parametrize("name,trips", [("add-2-trips", 2), ("add-3-trips", 3)])
def test_add_rows(gpu_ctx, name, trips):
    case = G.get(name)
    s = case.shape
    rng = np.random.default_rng(s.rows)
    a, b = rows(rng, s.rows, s.dim_a), rows(rng, s.rows, s.dim_b)
    check(case, "k_add", a.shape[0] * (s.dim_o + 1), s.dim_o + 1, trips)
    got = gpu_ctx.add_rows(a, s.deff_a, b, s.deff_b, s.dim_o)
    want = dense(a, s.deff_a, s.dim_o)
    want += dense(b, s.deff_b, s.dim_o)
    same(got, want, name)


def _touched_item(Lo, nwords):
    """flat index of an output of k_affine / k_acc_rows -> its work item (a word the kernel must leave alone: the row's first item)"""
    def f(i):
        r, w = divmod(i, Lo)
        return r * (nwords + 1) + (w if w < nwords else nwords if w == Lo - 1 else 0)
    return f


def test_affine_rows(gpu_ctx):
    """first nwords mask words = a << shift (zero from deff on), body = (body << shift) + an odd offset; the output starts as garbage and
    the words between nwords and the body must still be that garbage"""
    case = G.get("affine")
    s = case.shape
    rng = np.random.default_rng(11)
    a, before = rows(rng, s.rows, s.dim_a), rows(rng, s.rows, s.dim_o)
    add = int(rng.integers(0, 2 ** 63)) * 2 + 1
    check(case, "k_affine", a.shape[0] * (s.nwords + 1), s.nwords + 1)
    got = gpu_ctx.affine_rows(a, s.deff_a, before, s.nwords, s.shift, add)
    want = before.copy()
    want[:, :s.nwords] = dense(a, s.deff_a, s.dim_o)[:, :s.nwords] << U(s.shift)
    want[:, s.dim_o] = (a[:, -1] << U(s.shift)) + U(add)
    same(got, want, "affine", _touched_item(s.dim_o + 1, s.nwords))
    same(got[:, s.nwords:s.dim_o], before[:, s.nwords:s.dim_o], "affine: the words it must leave alone")


def test_acc_rows(gpu_ctx):
    """o[:, :nwords] += b[:, :nwords], body += body (each at its own stride); o starts as garbage and its other words stay"""
    case = G.get("acc")
    s = case.shape
    rng = np.random.default_rng(12)
    o, b = rows(rng, s.rows, s.dim_o), rows(rng, s.rows, s.dim_b)
    check(case, "k_acc_rows", o.shape[0] * (s.nwords + 1), s.nwords + 1)
    got = gpu_ctx.acc_rows(o, b, s.nwords)
    want = o.copy()
    want[:, :s.nwords] += b[:, :s.nwords]
    want[:, s.dim_o] += b[:, s.dim_b]
    same(got, want, "acc", _touched_item(s.dim_o + 1, s.nwords))
    same(got[:, s.nwords:s.dim_o], o[:, s.nwords:s.dim_o], "acc: the words it must leave alone")


def test_gather_rows(gpu_ctx):
    case = G.get("gather")
    s = case.shape
    rng = np.random.default_rng(13)
    src = rows(rng, s.n_src, s.dim_s)
    row_map = rng.integers(0, s.n_src, s.count).astype(np.int32)
    row_map[:5] = [0, s.n_src - 1, 7, 7, 0]                  # both ends and repeats ...
    row_map[-3:] = [s.n_src - 1, 0, 7]                       # ... and again beyond the seam
    assert np.unique(row_map).size < s.count and row_map.min() == 0 and row_map.max() == s.n_src - 1
    check(case, "k_pool_gather", row_map.size * (s.dim_d + 1), s.dim_d + 1)
    got = gpu_ctx.gather_rows(src, s.deff_s, row_map, s.dim_d)
    same(got, dense(src[row_map], s.deff_s, s.dim_d), "gather")


def test_sum_pool_rows(gpu_ctx):
    case = G.get("sum-pool")
    s = case.shape
    rng = np.random.default_rng(14)
    x = rng.integers(0, 2 ** 64, (s.B, s.C, s.H, s.W, s.dim_in + 1), dtype=U)
    Ho, Wo = s.H // s.K, s.W // s.K
    check(case, "k_sum_pool", s.B * s.C * Ho * Wo * (s.dim_o + 1), s.dim_o + 1)
    got = gpu_ctx.sum_pool_rows(x, s.deff_in, s.K, s.dim_o)
    want = np.zeros((s.B, s.C, Ho, Wo, s.dim_o + 1), U)
    for ky in range(s.K):
        for kx in range(s.K):
            tap = x[:, :, ky:Ho * s.K:s.K, kx:Wo * s.K:s.K]
            want[..., :s.deff_in] += tap[..., :s.deff_in]
            want[..., s.dim_o] += tap[..., -1]
    same(got, want, "sum pool")


@pytest.mark.parametrize("name", ["expand-mask-loop", "expand-tail-loop"])
def test_expand_seeded(gpu_ctx, name):
    """against dctfhe_rng_host at the stream and stride include/dctfhe.h documents: mask word j < dim_eff of row c is generator word
    c (D + 1) + j, zeros up to the body, then the body.  The mask-loop case writes some 270 MB and its reference is as large: the only
    case of that size, both freed before the next test"""
    from dctfhe.engine import SeededCiphertexts
    case = G.get(name)
    s = case.shape
    rng = np.random.default_rng(s.rows)
    key, stream = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), 0x5EED0000 + s.dim_eff
    bodies = rng.integers(0, 2 ** 64, s.rows, dtype=U)
    sc = SeededCiphertexts(key, stream, s.D, s.dim_eff, bodies)
    bpr, tail = (s.dim_eff + 7) // 8 + 1, s.dim + 1 - s.dim_eff
    if name == "expand-mask-loop":
        check(case, "k_seeded_expand", len(sc) * bpr, bpr)
        assert len(sc) * tail < T                                      # ... the tail loop of this case stays inside one trip
    else:
        check(case, "k_seeded_expand", len(sc) * tail, tail)
        assert len(sc) * bpr < T
    got = gpu_ctx.expand_seeded(sc, s.dim)
    stride = s.D + 1
    want = rng_words(gpu_ctx.L, key, stream, 0, s.rows * stride).reshape(s.rows, stride)      # stride = dim + 1 here: the rows themselves
    assert s.dim == s.D
    want[:, s.dim_eff:s.dim] = 0
    want[:, s.dim] = bodies
    try:
        # (mask loop: the item of the generator block that holds word i, counted in the row the word belongs to; a block two rows share
        # is computed by the earlier row's item)
        same(got, want, name, (lambda i: (i // stride) * bpr + (i >> 3) - ((i // stride * stride) >> 3)) if name == "expand-mask-loop" else
             (lambda i: (i // stride) * tail + max(i % stride - s.dim_eff, 0)))
    finally:
        del got, want


# ------------------------------------------------------------------------------------------ 2. clear mode: one word per element
def _lut_inputs(s, rng):
    """words that stay in range under shift 3, an odd body offset below 2^61 and the rounding term; per-channel tables with even pair sums"""
    n = s.C * s.H * s.W
    x = rng.integers(0, 2 ** 59, (1, n), dtype=U)
    tables = rng.integers(-2 ** 62, 2 ** 62, (s.C, 1 << s.w), dtype=np.int64) * 2
    body_add = int(rng.integers(0, 2 ** 60)) * 2 + 1
    return x, tables, 3, body_add


@pytest.mark.parametrize("mode", [G.LUT_EXACT, G.LUT_APPROX, G.LUT_SPLIT], ids=["exact", "approximate", "split"])
def test_lut_clear(gpu_ctx, mode):
    """one OP_LUT on 3 x 1200 x 1201 with a table per channel (T lies in channel 2): the whole download against circuit_ref.run_clear,
    overflow flag included -- once in range, once with ONE out-of-range element beyond T.  A parity-split record reads the whole table
    when no noise is on, like the other two modes"""
    from dctfhe.engine import Circuit, Session
    from oracle import circuit_ref
    case = G.get("lut-clear")
    s = case.shape
    x, tables, shift, body_add = _lut_inputs(s, np.random.default_rng(20 + mode))
    blob = G.lut_blob((s.C, s.H, s.W), s.p, s.r, s.w, shift, body_add, mode, tables)
    assert gpu_ctx.L.dctfhe_circuit_validate(blob, C.c_size_t(len(blob))) == 0
    assert circuit_ref.parse_blob(blob)["ops"][0]["ip"][9] == mode
    circ = Circuit(gpu_ctx, blob)
    sess = Session(gpu_ctx, circ, None, 1)
    try:
        dev, stride, n = sess.tensor(1)
        check(case, "k_lut_clear", n * stride, s.H * s.W)
        assert stride == 1 and T // (s.H * s.W) == s.C - 1
        sess.upload(x)
        want, ov = circuit_ref.run_clear(blob, x)
        assert not ov and flagged(sess.run) is False
        same(sess.download().reshape(1, -1), want, f"look-up mode {mode}")
        x2 = x.copy()
        x2[0, T + 12345] = U(1 << 60)                            # (x << 3) reaches bit 63: the only element out of range, in trip 1
        sess.upload(x2)
        want, ov = circuit_ref.run_clear(blob, x2)
        assert ov and flagged(sess.run) is True, "an out-of-range element beyond the first trip did not raise the overflow flag"
        same(sess.download().reshape(1, -1), want, f"look-up mode {mode}, one element out of range")
        assert flagged(sess.run) is True and flagged(lambda: (sess.upload(x), sess.run())) is False      # the flag is per run
    finally:
        sess.close()
        circ.close()


def test_lut_clear_with_noise(gpu_ctx):
    """`simulate` on the parity-split record (two draws per element, numbered 2 g and 2 g + 1, two sigmas, the half tables of channel
    (g / hw) % nchan) against the host twin tests/simulate_ref.py, word for word.  The twin needs 10 s on the host for all 8.6 M draws,
    and its long-double guard pass several times that, so it runs on three ranges of elements only -- the first 65 536,
    [T - 65 536, T + 65 536) and the last 65 536 -- and the other elements of this run are not compared (the noise-free runs above
    compare every element).  The host condition of the exact comparison (no noisy position within the guard of a box edge) is asserted
    for these ranges first"""
    import simulate_ref as R
    from dctfhe.engine import Circuit, Session
    case = G.get("lut-clear")
    s = case.shape
    x, tables, shift, body_add = _lut_inputs(s, np.random.default_rng(29))
    blob = G.lut_blob((s.C, s.H, s.W), s.p, s.r, s.w, shift, body_add, G.LUT_SPLIT, tables)
    seed, sigma, sigma2 = 0x5EA35EA3D00D, 2.0 ** -7, 2.0 ** -6      # half-box of a 3-bit half table: 2^-5, so draws do cross box edges
    n = x.size
    ranges = [(0, 65536), (T - 65536, T + 65536), (n - 65536, n)]
    trace = R.Trace()
    wants = []
    for lo, hi in ranges:
        g = np.arange(lo, hi, dtype=U)
        y, ov = R.lut_elements(x[0, lo:hi], g, s.H * s.W, s.p, s.r, s.w, shift, body_add, G.LUT_SPLIT, tables.view(U), seed, R.lut_stream(0, 0),
                               sigma, sigma2, trace, 0)
        assert not ov
        wants.append(y)
    Gd = R.guard(seed, trace)
    assert R.near_edge(trace, Gd) == [], Gd
    circ = Circuit(gpu_ctx, blob)
    sess = Session(gpu_ctx, circ, None, 1)
    try:
        check(case, "k_lut_clear", sess.tensor(1)[2], s.H * s.W)
        sess.set_noise(seed, [sigma])
        sess.set_noise_split([sigma2])
        sess.upload(x)
        assert flagged(sess.run) is False
        got = sess.download().reshape(-1)
    finally:
        sess.close()
        circ.close()
    from oracle import circuit_ref
    quiet = circuit_ref.run_clear(blob, x)[0].reshape(-1)
    moved = 0
    for (lo, hi), y in zip(ranges, wants):
        same(got[lo:hi], y, f"simulate, elements [{lo}, {hi})", lambda i, lo=lo: lo + i)
        moved += int((y != quiet[lo:hi]).sum())
    assert moved > 1000, "the noise moved next to no look-up: the comparison above says little"


@pytest.mark.parametrize("name", ["maxpool-clear-2-1-0", "maxpool-clear-3-2-1"])
def test_maxpool_clear(gpu_ctx, name):
    """dctfhe_max_pool_rows with keys = NULL: the signed-word maximum over the in-range taps, a row pass then a column pass, against
    circuit_ref.max_pool_words.  (2, 1, 0): both passes cross T.  (3, 2, 1): the row pass does, with padding taps at both borders"""
    from oracle import circuit_ref
    case = G.get(name)
    s = case.shape
    x = np.random.default_rng(s.C).integers(0, 2 ** 64, (1, s.C, s.H, s.W), dtype=U)
    Ho, Wo = (s.H + 2 * s.p - s.k) // s.s + 1, (s.W + 2 * s.p - s.k) // s.s + 1
    check(case, "k_maxpool_clear", x.shape[0] * s.C * s.H * Wo, Wo)
    if s.column_pass_crosses:
        check(case, "k_maxpool_clear", x.shape[0] * s.C * Ho * Wo, Ho * Wo, which=1)
    got = gpu_ctx.max_pool_rows(x, 0, s.k, s.s, s.p, 4)
    same(got, circuit_ref.max_pool_words(x, s.k, s.s, s.p), name)


# ------------------------------------------------------------------------------------------ 3. a levelled circuit in an encrypted session
@pytest.fixture(scope="module")
def levelled(gpu_ctx, keys):
    """y = x + x, then a sum pool of window 1, on 57 images of 4 x 6 x 6 stored at 512 mask words: (case, circuit, compact host rows)"""
    from dctfhe.engine import Circuit
    case = G.get("session-levelled")
    s = case.shape
    blob = G.levelled_blob((s.C, s.H, s.W), s.deff)
    assert gpu_ctx.L.dctfhe_circuit_validate(blob, C.c_size_t(len(blob))) == 0
    circ = Circuit(gpu_ctx, blob)
    n = s.batch * s.C * s.H * s.W
    host = np.random.default_rng(31).integers(0, 2 ** 64, (n, s.dim + 1), dtype=U)
    host[:, s.deff:s.dim] = 0                                    # the compact wire form: nothing beyond the effective dimension
    host.setflags(write=False)
    yield case, circ, host
    circ.close()


def _session_counts(case, sess):
    """the work counts of the session's launches from its own strides (dctfhe_session_tensor), held to the rules"""
    s = case.shape
    (_, L0, n0), (_, L1, n1), (_, L2, n2) = (sess.tensor(t) for t in range(3))
    assert (L0, L1, L2) == (s.stride,) * 3 and (n0, n1, n2) == (G.SESSION_ROWS,) * 3 and n0 * L0 == 4210704
    check(case, "k_tail_nonzero", n0 * (s.dim - (L0 - 1)), s.dim - (L0 - 1))
    check(case, "k_restride", n0 * L0, L0)                             # upload
    check(case, "k_restride", n2 * (s.dim + 1), s.dim + 1, trips=3, which=1)      # download
    check(case, "k_add", n1 * L1, L1)
    check(case, "k_sum_pool", n2 * L2, L2)
    return n0, L0


def test_session_levelled_run(gpu_ctx, keys, levelled):
    """upload in the compact form (dim = 1024 onto rows stored at 513 words), run, download at dim = 1024; the stored tensors are read
    behind every step.  k_restride both ways (the download in three trips), and the session's own launches of k_add and k_sum_pool"""
    from dctfhe.engine import Session
    case, circ, host = levelled
    s = case.shape
    sess = Session(gpu_ctx, circ, keys, s.batch)
    try:
        n, L = _session_counts(case, sess)
        assert sess.dims() == (s.deff, s.deff)
        sess.upload(host, dim=s.dim)
        stored = np.concatenate([host[:, :s.deff], host[:, s.dim:]], axis=1)
        same(read_rows(sess, 0), stored, "upload (k_restride to the stored stride)")
        sess.run()
        same(read_rows(sess, 0), stored, "the input after the run")
        same(read_rows(sess, 1), stored + stored, "x + x (k_add in the session)")
        same(read_rows(sess, 2), stored + stored, "sum pool of window 1 (k_sum_pool in the session)")
        want = np.zeros((n, s.dim + 1), U)
        want[:, :s.deff] = host[:, :s.deff] + host[:, :s.deff]
        want[:, s.dim] = host[:, s.dim] + host[:, s.dim]
        same(sess.download(s.dim).reshape(n, s.dim + 1), want, "download (k_restride to host rows)")
    finally:
        sess.close()


@pytest.mark.parametrize("row", ["first", "last", None])
def test_session_upload_guard(gpu_ctx, keys, levelled, row):
    """k_tail_nonzero lets the upload drop the mask words beyond the effective dimension: ONE non-zero word there must refuse the upload,
    in the first row and in the last, whose work items lie beyond T; a clean upload succeeds.  (Error returns: nothing faults)"""
    from dctfhe._lib import DctfheError
    from dctfhe.engine import Session
    case, circ, host = levelled
    s = case.shape
    sess = Session(gpu_ctx, circ, keys, s.batch)
    try:
        n, L = _session_counts(case, sess)
        tail = s.dim - s.deff
        bad = host.copy()
        if row is None:
            sess.upload(bad, dim=s.dim)
            return
        r, w = (0, s.deff + 3) if row == "first" else (n - 1, s.dim - 1)
        item = r * tail + (w - s.deff)
        assert (item < T) == (row == "first") and (row == "first" or item == n * tail - 1)
        bad[r, w] = 1
        with pytest.raises(DctfheError, match="non-zero mask words beyond"):
            sess.upload(bad, dim=s.dim)
        sess.upload(host, dim=s.dim)                                  # the flag does not stick
    finally:
        sess.close()


# ------------------------------------------------------------------------------------------ 4. ring pack and public-key draws
def test_ring_digits(gpu_ctx, keys):
    """dctfhe_ring_pack on the test ring (N = 256, n = 48, one level) with 87 600 small ciphertexts: 343 groups in one launch, the last
    partial.  tests/ring_ref.py on group 0, on group 341 (it holds digit items T - 1 and T) and on the last group, 342: every digit
    written beyond the first trip belongs to one of the last two.  ring_ref has no reference of a group's body term alone, so groups
    1 .. 340 are NOT compared (the pack itself is compared group by group in tests/test_gpu_ring.py)"""
    import ring_ref
    from dctfhe import params as P
    from dctfhe.engine import PackKey
    case = G.get("ring-digits")
    s = case.shape
    spec = P.PackSpec(logN=s.logN, l=s.l, beta=s.beta, sigma=2.0 ** -48)
    N = spec.N
    pk = PackKey(gpu_ctx, keys.export_pack_key(spec))
    try:
        key_rows = pk.export_rows()
        assert key_rows.shape == (s.n, s.l, 2, N) and (pk.l, pk.beta) == (s.l, s.beta)
        small = np.random.default_rng(41).integers(0, 2 ** 64, (s.count, s.n + 1), dtype=U)
        groups = -(-small.shape[0] // N)
        per_launch = max(1, min(groups, 4096, (64 << 20) // (s.n * pk.l * N * 4)))      # dev_ring_pack's batch of groups
        assert per_launch == groups, "the groups no longer fit one launch of k_ring_digits: each launch would stay under T"
        check(case, "k_ring_digits", groups * s.n * N, s.n * N)
        assert small.shape[0] % N != 0
        got = pk.ring_pack(small).words
        assert got.size == spec.words(s.count)
        seam = [(T - 1) // (s.n * N), T // (s.n * N)]
        assert seam == [341, 341] and groups == 343
        for g in sorted({0, *seam, groups - 1}):
            part = small[g * N:(g + 1) * N]
            want = ring_ref.pack16(ring_ref.pack(part, key_rows, s.l, s.beta), part.shape[0])
            same(got[2 * g * N:2 * g * N + want.size], want, f"ring pack, group {g} (digit items from {g * s.n * N})")
        assert 2 * (groups - 1) * N + want.size == got.size
    finally:
        pk.close()


def test_pk_draws(gpu_ctx, keys):
    """dctfhe_public_key_draws for 4 200 000 phases on the test ring against tests/public_ref.py draws(): the first 4096 draws,
    [T - 4096, T + 4096) and the last 4096 of u, e1 (nmask = 4 200 192 of them) and e2 (count)"""
    import public_ref
    from dctfhe import params as P
    from dctfhe.engine import PublicKey
    case = G.get("pk-draws")
    s = case.shape
    spec = P.test_public_input_spec()
    assert spec.logN == s.logN
    pk = PublicKey(gpu_ctx, keys.export_public_key(spec))
    try:
        seed32, call = bytes(range(7, 39)), 2
        pk.set_encrypt_seed(seed32)
        nmask = -(-s.count // spec.N) * spec.N
        check(case, "k_pk_draws", nmask, spec.N)
        assert s.count % spec.N != 0 and T + 4096 < s.count
        u, e1, e2 = pk.draws(call, s.count)
        assert (u.size, e1.size, e2.size) == (nmask, nmask, s.count)
        for lo, hi in [(0, 4096), (T - 4096, T + 4096), (nmask - 4096, nmask)]:
            assert public_ref.draws_near_a_tie(seed32, call, lo, hi - lo, spec.sigma) == []
            wu, w1, w2 = public_ref.draws(seed32, call, lo, hi - lo, spec.sigma)
            same(u[lo:hi], wu, f"u [{lo}, {hi})", lambda i, lo=lo: lo + i)
            same(e1[lo:hi], w1, f"e1 [{lo}, {hi})", lambda i, lo=lo: lo + i)
            top = min(hi, s.count)
            same(e2[lo:top], w2[:top - lo], f"e2 [{lo}, {top})", lambda i, lo=lo: lo + i)
        lo = s.count - 4096                                           # e2 ends at count, inside the last block
        same(e2[lo:], public_ref.draws(seed32, call, lo, 4096, spec.sigma)[2], f"e2 [{lo}, {s.count})", lambda i: lo + i)
        assert public_ref.draws_near_a_tie(seed32, call, lo, 4096, spec.sigma) == []
        assert 0.4 < u.mean() < 0.6 and e1.any() and e2.any()
    finally:
        pk.close()
