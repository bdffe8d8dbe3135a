"""`simulate` on the device against its numpy twin (tests/simulate_ref.py), WORD FOR WORD: one-site circuits in all
four look-up modes, per-channel tables, the two passes of a max pool, whole circuits run twice and span by span, sharded and slab-divided
sessions -- every element, none left out.  Each case first asserts on the host that no draw of its seed lies within the guard of a box
edge (tests/test_simulate_host.py measures that guard), so a last-bit difference between the device's libm and numpy's cannot show.
Then: `simulate` and the encrypted run agree with the closed form of an approximate-rounding site and of a parity split."""
import ctypes as C
import math

import numpy as np
import pytest

import simulate_cases as SC
import simulate_ref as R

pytestmark = pytest.mark.gpu
U = np.uint64
E_OUT = 56


# ------------------------------------------------------------------------------------------ helpers
_hip = None


def read_tensor(sess, tensor):
    """the words of a clear-mode session's tensor, copied from the pointer dctfhe_session_tensor hands out with the HIP runtime the
    library itself has loaded (the engine's runs are synchronous: the words are there)"""
    global _hip
    if _hip is None:
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        assert paths, "the HIP runtime is not loaded"
        _hip = C.CDLL(paths[0])
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    dev, row_words, rows = sess.tensor(tensor)
    assert row_words == 1 and dev
    out = np.empty(rows, np.uint64)
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


def host_condition(case):
    """the condition the exact comparison stands on: no noisy position within the guard of an edge"""
    runs, trace = case.twin()
    G = R.guard(case.seed, trace)
    close = R.near_edge(trace, G)
    assert close == [], (case.name, G, close[:5])
    return runs


def clear_session(ctx, circ, case, batch):
    from dctfhe.engine import Session
    s = Session(ctx, circ, None, batch)
    s.set_noise(case.seed, case.sigmas)
    s.set_noise_split(case.sigmas2)
    return s


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, first at {bad[:5].tolist()}: device {got[bad[:3]].tolist()} twin {want[bad[:3]].tolist()}"


# ------------------------------------------------------------------------------------------ every committed case
@pytest.mark.parametrize("name", list(SC.BUILDERS))
def test_device_equals_twin(gpu_ctx, name):
    """one session, run once per input of the case: pass j equals the twin's run j (outputs and overflow flag), so the run counter moves
    the stream.  A circuit of several ops, on a second session: pass 0 op by op through run_span, each op's destination read right
    behind it and compared (a span that stops early does not advance the counter), then one whole run: the twin's run 1."""
    from dctfhe.engine import Circuit
    case = SC.get(name)
    runs = host_condition(case)
    c = R.circuit_ref.parse_blob(case.blob)
    batch, n_ops, out_t = case.runs[0].shape[0], len(c["ops"]), c["output"]
    circ = Circuit(gpu_ctx, case.blob)
    sess = clear_session(gpu_ctx, circ, case, batch)
    try:
        for j, ph in enumerate(case.runs):
            sess.upload(ph)
            ov = flagged(sess.run)
            assert ov == runs[j][1], f"{name} run {j}: overflow flag {ov}, twin {runs[j][1]}"
            same(sess.download(), runs[j][0][out_t], f"{name} run {j}")
    finally:
        sess.close()
    if n_ops > 1:
        sess = clear_session(gpu_ctx, circ, case, batch)
        try:
            sess.upload(case.runs[0])
            ov = False
            for i, o in enumerate(c["ops"]):
                ov |= flagged(lambda: sess.run_span(i, i + 1))
                same(read_tensor(sess, o["dst"]), runs[0][0][o["dst"]], f"{name} op {i} (tensor {o['dst']})")
            assert ov == runs[0][1]
            same(sess.download(), runs[0][0][out_t], f"{name} spans")
            if len(case.runs) > 1:
                sess.upload(case.runs[1])
                assert flagged(sess.run) == runs[1][1]
                same(sess.download(), runs[1][0][out_t], f"{name} run 1 behind the spans")
        finally:
            sess.close()
    circ.close()


@pytest.mark.parametrize("geom", list(SC.POOLS))
def test_quiet_pool_is_the_signed_maximum(gpu_ctx, geom):
    """sigma = 2^-40 moves no relu entry: the fold m += relu(x - m) over the taps is the signed maximum, the sigma = 0 output"""
    from dctfhe.engine import Circuit, Session
    case = SC.get(f"pool-{geom}-quiet")
    want, _ = R.circuit_ref.run_clear(case.blob, case.runs[0])
    circ = Circuit(gpu_ctx, case.blob)
    try:
        for noise in (True, False):
            sess = clear_session(gpu_ctx, circ, case, 2) if noise else Session(gpu_ctx, circ, None, 2)
            try:
                sess.upload(case.runs[0])
                sess.run()
                same(sess.download(), want, f"{geom} noise={noise}")
            finally:
                sess.close()
    finally:
        circ.close()


# ------------------------------------------------------------------------------------------ divided runs, against the twin itself
def _drive(c, sessions, batch, end_op):
    """all parts span by span through the compiler's plan with row ranges; at each point every session takes the rows of its need range
    from the parts that own them (tests/test_gpu_shard_pool.py drive)"""
    from dctfhe.compile import shard_rows
    P, first = len(sessions), 0
    plans = [c.shard_plan(rows=True, part=p, parts=P, batch=batch) for p in range(P)]
    flag = False
    for i, (after_op, tensor, _, _) in enumerate(plans[0]):
        if after_op + 1 > end_op:
            break
        for s in sessions:
            flag |= flagged(lambda: s.run_span(first, after_op + 1))
        first = after_op + 1
        rows = sessions[0].tensor(tensor)[2]
        own = [shard_rows(rows, P, p) for p in range(P)]
        for q, dst in enumerate(sessions):
            nf, nn = plans[q][i][2:4]
            for p in range(P):
                lo, hi = max(own[p][0], nf), min(own[p][0] + own[p][1], nf + nn)
                if p != q and hi > lo:
                    dst.copy_rows_from(sessions[p], tensor, lo, hi - lo)
            if (nf, nn) == (0, rows):
                dst.mark_whole(tensor)
            else:
                dst.mark_rows(tensor, nf, nn)
    for s in sessions:
        flag |= flagged(lambda: s.run_span(first, end_op))
    return flag


@pytest.mark.parametrize("name", ["trunk-pooled_trunk", "trunk-pooled_trunk-noisy-pool"])
def test_sharded_parts_equal_the_twin(gpu_ctx, name):
    """three parts with the pools divided.  Stopped behind the pool, every part's own rows of the pool's output are the twin's (with
    1/32 of the torus on the pool its relu entries move, so equal rows mean equal draws); run to the end, every part downloads the
    twin's outputs and the next whole pass is the twin's run 1"""
    from dctfhe import compile as cc
    from dctfhe.engine import Circuit
    case = SC.get(name)
    runs = host_condition(case)
    c, _ = SC.compiled_trunk("pooled_trunk")
    (pool_op,) = [i for i, o in enumerate(c.ops) if o.type == cc.OP_MAXPOOL]
    pool_dst, parts = c.ops[pool_op].dst, 3
    circ = Circuit(gpu_ctx, case.blob)

    def make():
        out = []
        for p in range(parts):
            s = clear_session(gpu_ctx, circ, case, SC.BATCH)
            s.set_shard(p, parts)
            s.set_shard_pool(True)
            s.upload(case.runs[0])
            out.append(s)
        return out
    sessions = make()
    try:
        _drive(c, sessions, SC.BATCH, pool_op + 1)
        want = runs[0][0][pool_dst].reshape(-1)
        for p, s in enumerate(sessions):
            f, n = cc.shard_rows(want.size, parts, p)
            same(read_tensor(s, pool_dst)[f:f + n], want[f:f + n], f"{name}: pool rows of part {p}")
    finally:
        for s in sessions:
            s.close()
    sessions = make()
    try:
        for j in range(2):
            if j:
                for s in sessions:
                    s.upload(case.runs[1])
            assert _drive(c, sessions, SC.BATCH, len(c.ops)) == runs[j][1]
            for p, s in enumerate(sessions):
                same(s.download(), runs[j][0][c.output_tensor], f"{name}: part {p}, run {j}")
    finally:
        for s in sessions:
            s.close()
        circ.close()


@pytest.mark.parametrize("name", ["trunk-pooled_trunk", "trunk-pooled_trunk-noisy-pool"])
def test_slab_divided_run_equals_the_twin(gpu_ctx, name):
    """every slab group one channel at a time (dctfhe_session_set_slab_heights): a slab's elements keep their numbers in the whole
    tensor, and with them their draws"""
    from dctfhe.engine import Circuit
    case = SC.get(name)
    runs = host_condition(case)
    circ = Circuit(gpu_ctx, case.blob)
    sess = clear_session(gpu_ctx, circ, case, SC.BATCH)
    try:
        sess.upload(case.runs[0])
        groups = sess.memory_plan()["groups"]
        assert groups and any(g["channels"] > 1 for g in groups)
        sess.set_slab_heights([1] * len(groups))
        for j in range(2):
            if j:
                sess.upload(case.runs[1])
            assert flagged(sess.run) == runs[j][1]
            same(sess.download(), runs[j][0][R.circuit_ref.parse_blob(case.blob)["output"]], f"{name} in slabs, run {j}")
    finally:
        sess.close()
        circ.close()


# ------------------------------------------------------------------------------------------ simulate and the encrypted run
def _params(quiet_twin=False):
    """the small rings of params.test_params(); quiet_twin: the table tier as tier 2, sharing the key-switch key of tier 0 (its twin),
    which is what a LUT_SPLIT_QUIET site runs its second look-up on"""
    import copy
    from dctfhe import params as P
    ps = P.test_params()
    if quiet_twin:
        t = copy.copy(ps.tiers[0])
        t.name, t.ksk_share = "t2", 0
        ps.tiers.append(t)
    return ps


@pytest.fixture(scope="module")
def small_keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    made = {}

    def get(quiet_twin=False):
        if quiet_twin not in made:
            ps = _params(quiet_twin)
            made[quiet_twin] = (ps, Keys(gpu_ctx, P.to_c_params(ps), seed=20261020))
        return made[quiet_twin]
    yield get
    for _, k in made.values():
        k.close()


def _three_ways(ctx, keys, blob, phases, seed):
    """-> (simulate at sigma 2^-40: output words, overflow flag; execute: decrypted output words)"""
    from dctfhe.engine import Circuit, Session
    circ = Circuit(ctx, blob)
    sim = Session(ctx, circ, None, 1)
    enc = Session(ctx, circ, keys, 1)
    try:
        sim.set_noise(seed, [2.0 ** -40])
        sim.upload(phases.reshape(1, -1))
        ov = flagged(sim.run)
        enc.upload(keys.encrypt(phases.reshape(-1)))
        enc.run()
        dec = keys.decrypt(enc.download().reshape(-1, keys.D + 1))
        return sim.download().reshape(-1), ov, dec.reshape(-1)
    finally:
        sim.close()
        enc.close()
        circ.close()


def _decode(words):
    """decrypted words -> the integers at 2^E_OUT they are closest to"""
    return np.round(words.astype(np.int64).astype(np.float64) / 2.0 ** E_OUT).astype(np.int64)


def test_approximate_site_simulate_execute_and_closed_form(gpu_ctx, small_keys):
    """One approximate-rounding record under the small rings.  On-grid messages m read entry floor((m + 2^(r-1)) / 2^r), off-grid inputs
    m + f entry floor((m + f + 1/2 + 2^(r-1)) / 2^r), negated from index 2^w on (the padding bit).  The closed form, `simulate` at
    sigma 2^-40 and the decrypted encrypted run are equal at EVERY input.
    Condition: every input lies at least 8 decision sigmas from the nearest box edge.  The decision sigma is the model's
    (params.var_keyswitch + var_modswitch on the fresh input: what CompiledCircuit.margin_model prices a table with); p is the largest
    precision whose on-grid half unit 2^-(p+2) satisfies it, and the fractions are those of sixteenths that do for every m."""
    from dctfhe import params as P
    ps, keys = small_keys()
    tt = ps.tiers[0]
    sigma = math.sqrt(ps.input_sigma ** 2 + P.var_keyswitch(ps.D, tt) + P.var_modswitch(tt))
    p = int(math.floor(-math.log2(8.0 * sigma))) - 2
    r = 2
    w = p - r
    print(f"decision sigma 2^{math.log2(sigma):.2f}; p = {p}: half unit 2^-{p + 2} = {2.0 ** -(p + 2) / sigma:.1f} sigma; p + 1 would give {2.0 ** -(p + 3) / sigma:.1f}")
    assert 2.0 ** -(p + 2) >= 8.0 * sigma > 2.0 ** -(p + 3) and w >= 2
    unit = 2.0 ** -(p + 1)                                   # one message step, as a fraction of the torus
    # m + f + 1/2 against the integers: every residue of m mod 2^r occurs, so the nearest edge is frac(f + 1/2)'s distance to 0 or 1
    dist = lambda f: min((f + 0.5) % 1.0, 1.0 - (f + 0.5) % 1.0) * unit
    fracs = [j / 16.0 for j in range(-7, 8) if dist(j / 16.0) >= 8.0 * sigma]
    print("fractions", fracs, "nearest edge in sigmas", [round(dist(f) / sigma, 1) for f in fracs])
    assert 0.0 in fracs and len([f for f in fracs if f]) >= 3
    rng = np.random.default_rng(4)
    vals = rng.permutation(np.arange(1, (1 << w) + 1)) * rng.choice([-1, 1], 1 << w)
    m = np.repeat(np.arange(1 << (p + 1), dtype=np.int64), len(fracs))
    f16 = np.tile(np.array([int(f * 16) for f in fracs], np.int64), 1 << (p + 1))
    assert 256 <= m.size <= 512
    phases = ((m * 16 + f16).astype(np.uint64) << U(63 - p - 4))            # (m + f) 2^(63-p) mod 2^64
    t = ((m * 16 + f16 + 8 + (16 << (r - 1))) >> (4 + r)) % (1 << (w + 1))   # floor((m + f + 1/2 + 2^(r-1)) / 2^r) on the 2^(p+1) ring
    want = np.where(t < (1 << w), vals[t % (1 << w)], -vals[t % (1 << w)])
    on = f16 == 0
    assert np.array_equal(t[on], ((m[on] + (1 << (r - 1))) >> r) % (1 << (w + 1)))
    blob = R.chain_blob((1, 1, m.size), [R.lut_record(p, r, w, 0, 1, (vals << E_OUT).reshape(1, -1), 0)], max_bit_width=p)
    sim, ov, dec = _three_ways(gpu_ctx, keys, blob, phases, 31)
    assert ov                                                                 # half of the inputs carry the padding bit
    same(sim, (want << E_OUT).astype(np.uint64), "simulate against the closed form")
    got = _decode(dec)
    assert np.abs(dec.astype(np.int64) - (got << E_OUT)).max() < (1 << (E_OUT - 3)), "decrypted outputs far from the grid"
    same(got, want, "execute against the closed form")


@pytest.mark.parametrize("mode", [2, 3])
def test_split_site_simulate_execute_and_table(gpu_ctx, small_keys, mode):
    """a parity split at every 7-bit message, twice: `simulate` at 2^-40 (its path through S / Dt and the sign of the second look-up)
    equals the decrypted encrypted run equals T[t]"""
    ps, keys = small_keys(quiet_twin=mode == 3)
    rng = np.random.default_rng(6 + mode)
    vals = rng.integers(-64, 64, 128)
    vals[::5] |= 1
    t = np.tile(np.arange(128, dtype=np.uint64), 2)
    rec = R.lut_record(7, 0, 7, 0, mode, (vals << E_OUT).reshape(1, -1), 0)
    if mode == 3:
        rec["ip"][4] = 2                                                       # the table tier whose twin is tier 0
    blob = R.chain_blob((1, 1, t.size), [rec])
    sim, ov, dec = _three_ways(gpu_ctx, keys, blob, t << U(56), 32 + mode)
    want = vals[t.astype(np.int64)]
    assert not ov
    same(sim, (want << E_OUT).astype(np.uint64), f"mode {mode}: simulate against the table")
    same(_decode(dec), want, f"mode {mode}: execute against the table")
