"""compile_model(pool_policy="exact") on the GPU: the quiet pool tier T6p (N = 8192, two levels of 15 bits, one-bit rotation, n = 832)
against the noise model that chose it; the max pool's tree on that tier at p_d = 6; and the ImageNet setting of the 5-bit RGB trunk, small
(tests/pool_policy_cases.py): encrypted, clear and simulated runs against the integer circuit, the bootstraps per tier, the margin audit
of the pool's decisions, the same output words under a memory budget and divided over two parts, and a deployment's key check."""
import math

import numpy as np
import pytest

import pool_policy_cases as cases
from oracle import circuit_ref as mref

pytestmark = pytest.mark.gpu


def _cent(x):
    return x.astype(np.int64).astype(np.float64) / 2.0 ** 64


# ------------------------------------------------------------------------------------------ the tier alone
@pytest.fixture(scope="module")
def tier_keys(gpu_ctx):
    """[T6p, B] of the 11-tier catalogue, inputs under the first 2048 key bits as every client's"""
    from dctfhe import params as P
    from dctfhe.engine import Keys
    full = P.default_params_5bit_pool()
    ps = P.ParamSet(D=8192, tiers=[full.tiers[10], full.tiers[3]], bit_tier=1, table_tier_for_w={6: 0}, input_dim=2048)
    assert ps.tiers[0].name == "T6p" and ps.tiers[1].name == "B"
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=3)
    yield ps, keys
    keys.close()


def test_output_noise_matches_model(tier_keys):
    """as tests/test_gpu_noise.py: 1024 ciphertexts through the key switch and a 3-bit identity look-up, sigma within [0.5x, 1.6x]"""
    from dctfhe import params as P
    ps, keys = tier_keys
    t = ps.tiers[0]
    msgs = np.random.default_rng(0).integers(0, 8, 1024).astype(np.uint64)
    cts = keys.encrypt(msgs << np.uint64(60))
    out = keys.pbs(0, keys.keyswitch(0, cts), np.arange(8, dtype=np.int64) << 57, 3)
    err = _cent(keys.decrypt(out) - (msgs << np.uint64(57)))
    assert np.abs(err).max() < 2.0 ** -9, "wrong outputs"
    measured, model = err.std(), math.sqrt(P.var_pbs_out(t, ps.fft_noise_c))
    print(f"T6p sigma_out log2 (measured, model): {math.log2(measured):.2f}, {math.log2(model):.2f}")
    assert 0.5 * model < measured < 1.6 * model, (math.log2(measured), math.log2(model))


def test_keyswitch_noise_matches_model(tier_keys, oracle):
    from dctfhe import params as P
    ps, keys = tier_keys
    t = ps.tiers[0]
    _, s = keys.export_secret()
    msgs = np.random.default_rng(1).integers(0, 16, 4096).astype(np.uint64) << np.uint64(59)
    small = keys.keyswitch(0, keys.encrypt(msgs))
    err = _cent(oracle.lwe_phase(s[:t.n].copy(), t.n, small) - msgs)
    measured, model = err.std(), math.sqrt(P.var_keyswitch(ps.input_dim, t) + ps.input_sigma ** 2)
    print(f"T6p sigma after key switch log2 (measured, model): {math.log2(measured):.2f}, {math.log2(model):.2f}")
    assert 0.7 * model < measured < 1.3 * model, (math.log2(measured), math.log2(model))


@pytest.mark.parametrize("pool,H,W", [((3, 2, 1), 7, 9), ((2, 2, 0), 8, 9), ((3, 1, 1), 6, 5)])
def test_max_pool_rows_on_the_quiet_tier(gpu_ctx, tier_keys, pool, H, W):
    """5-bit values under the 64-entry relu table at e = 57, ring 8192, inputs at 2048 mask words: single-tap windows ((2, 2, 0) on 9
    columns drops one, (3, 2, 1) starts with two taps), odd sizes, the late pairing; the extremes of the difference forced"""
    import torch
    import torch.nn.functional as F
    _, keys = tier_keys
    k, s, p = pool
    p_d, e, dim_in, ring = 6, 57, 2048, 8192
    v = np.random.default_rng(k * 100 + H).integers(0, 32, (2, 3, H, W))
    v[0, 0, 0, :2] = (0, 31)           # d = -31 and, in the next window or pass, +31
    v[0, 1, 0, :2] = (31, 0)
    v[0, 2, :2, 0] = (0, 31)
    v[1, 0] = 17                       # equal pairs: d = 0
    v[1, 1] = 31                       # an all-31 window
    v[1, 2, 1::2] = 0
    table = (np.maximum(np.arange(64) - 32, 0).astype(np.uint64) << np.uint64(e)).view(np.int64)
    want = F.max_pool2d(torch.from_numpy(v.astype(np.float64)), k, s, p).numpy().astype(np.int64)
    ph = v.astype(np.uint64) << np.uint64(e)
    words = mref.max_pool_words(ph, k, s, p)
    assert np.array_equal(words.view(np.int64) >> e, want)
    cts = keys.encrypt(ph.reshape(-1), dim_in).reshape(2, 3, H, W, dim_in + 1)
    out = gpu_ctx.max_pool_rows(cts, dim_in, k, s, p, p_d, table, ring, keys=keys, tier=0)
    dec = keys.decrypt(out.reshape(-1, ring + 1), ring).reshape(want.shape)
    got = ((dec + (np.uint64(1) << np.uint64(e - 1))) >> np.uint64(e)).astype(np.int64)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert np.array_equal(got.astype(np.uint64) << np.uint64(e), words)
    # the noise the tree leaves on a maximum is the tier's output noise, a few times over: far inside half a unit of e
    assert np.abs(_cent(dec - words)).max() < 2.0 ** -(63 - e + 6)


# ------------------------------------------------------------------------------------------ the ImageNet setting, small
class Crop:
    """the circuit of tests/pool_policy_cases.py with keys, one image in the seeded wire form, and the plain encrypted run's output rows:
    computed once, never modified"""

    def __init__(self):
        from dctfhe.engine import Session
        self.qm, self.x = cases.crop_module()
        qm = self.qm
        self.c = qm.compiled
        self.pool_index, self.pool = cases.pool_op(self.c)
        qm.fhe_circuit.keygen(seed=5)
        self.q = qm.quantize_input(self.x[12:14])
        ref, overflow = mref.run_clear(self.c.blob, qm.encode_input(self.q))
        assert not overflow
        self.want = qm.decode_output(ref)
        self.ctx, self.circuit, self.keys = qm._context(), qm._circuit, qm._keys
        self.seeded = self.keys.encrypt_seeded(qm.encode_input(self.q[:1]).reshape(-1))
        sess = Session(self.ctx, self.circuit, self.keys, 1)
        try:
            sess.upload_seeded(self.seeded)
            self.timing = sess.run(timing=True)
            self.out_dim = sess.dims()[1]
            self.rows = sess.download(self.out_dim)
            self.rows.setflags(write=False)
        finally:
            sess.close()

    def decode(self, rows):
        return self.qm.decode_output(self.keys.decrypt(rows.reshape(-1, self.out_dim + 1), self.out_dim).reshape(rows.shape[0], -1))


@pytest.fixture(scope="module")
def crop():
    c = Crop()
    yield c
    c.qm.close()


def test_crop_encrypted_clear_and_simulated_equal_the_integer_circuit(crop):
    c, qm = crop.c, crop.qm
    names = [t.name for t in c.param_set.tiers]
    assert names[crop.pool.pool.tier] == "T6p" and len(names) == 11 and c.worst_site_failure <= 1e-12
    assert crop.want.shape == (2, 64) and len(np.unique(crop.want)) > 4
    assert np.array_equal(qm.forward_quantized(crop.q, "disable"), crop.want)
    got = crop.decode(crop.rows)
    assert np.array_equal(got, crop.want[:1]), np.argwhere(got != crop.want[:1])
    counts = c.pbs_counts()
    assert {names[i]: crop.timing.pbs_cts[i] for i in range(len(names)) if crop.timing.pbs_cts[i]} == counts
    assert counts["T6p"] == cases.CROP_POOL_PAIRS
    print("bootstraps per tier:", counts, "ms per tier:", {names[i]: round(crop.timing.pbs_ms[i], 1) for i in range(len(names)) if crop.timing.pbs_cts[i]})
    assert np.array_equal(qm.forward_quantized(crop.q, "simulate"), crop.want)


def test_margin_audit_of_the_pool(crop):
    """two images: 46 080 pool decisions.  The bound on measured / modelled sigma is the one tests/test_gpu_margin.py holds its rows to
    (1.3x from above); the half-box in measured sigmas is held to the model's own ratio under the same bound"""
    out, report = crop.qm.audit(crop.x[12:14])
    assert np.array_equal(out, crop.qm.dequantize_output(crop.want))
    (row,) = [r for r in report.rows if r["kind"] == "pool"]
    (model,) = [m for m in crop.c.margin_model() if m["kind"] == "pool"]
    assert row["tier_name"] == "T6p" and row["table_bits"] == 6 and row["count"] == 2 * crop.pool.n_max == 46080
    z_model = 2.0 ** -(6 + 2) / model["sigma"]
    print(f"pool decisions: measured sigma 2^{math.log2(row['sigma_measured']):.2f}, model 2^{math.log2(model['sigma']):.2f}, ratio {row['ratio']:.3f}; "
          f"half-box = {row['z']:.2f} measured sigma, {z_model:.2f} modelled; largest |e| / half-box {row['max_over_half_box']:.3f}")
    assert row["ratio"] <= 1.3
    assert row["z"] >= z_model / 1.3
    assert row["max_abs"] < row["half_box"]
    over = [(r["op"], r["kind"], r["tier_name"], r["count"], round(r["ratio"], 3)) for r in report.rows if r["count"] >= 256 and r["ratio"] > 1.3]
    assert not over, over


def test_same_words_under_a_memory_budget(crop):
    """a budget one byte below the undivided plan: the stem group (convolution, look-ups, the pool) runs in channel slabs"""
    from dctfhe.engine import Session
    whole = crop.c.memory_plan(batch=1)
    budget = whole["bytes_planned"] - 1
    sess = Session(crop.ctx, crop.circuit, crop.keys, 1)
    try:
        sess.upload_seeded(crop.seeded)
        sess.set_memory_budget(budget)
        plan = sess.memory_plan()
        stem = [g for g in plan["groups"] if g["first_op"] <= crop.pool_index < g["end_op"]]
        assert stem and stem[0]["slab"] < stem[0]["channels"] and plan["bytes_planned"] <= budget, plan
        sess.run()
        assert np.array_equal(sess.download(crop.out_dim), crop.rows)
    finally:
        sess.close()


def test_same_words_divided_over_two_parts(crop):
    """set_shard + set_shard_pool, both parts in this process, driven span by span through the plan with row ranges as
    tests/test_gpu_shard_pool.py drives its cases: each part runs its own pairwise maxima on T6p and ends with the plain run's words"""
    from dctfhe import engine, sharding
    from dctfhe.compile import shard_rows
    from dctfhe.engine import Session
    c, P = crop.c, 2
    src = c.tensors[crop.pool.src0]
    sessions = [Session(crop.ctx, crop.circuit, crop.keys, 1) for _ in range(P)]
    try:
        for p, s in enumerate(sessions):
            s.set_shard(p, P)
            s.set_shard_pool(True)
            s.upload_seeded(crop.seeded)
        plans = [c.shard_plan(rows=True, part=p, parts=P, batch=1) for p in range(P)]
        first = 0
        for p, s in enumerate(sessions):
            assert s.shard_plan_rows() == plans[p]
        for i, (after_op, tensor, _, _) in enumerate(plans[0]):
            for s in sessions:
                s.run_span(first, after_op + 1)
            first = after_op + 1
            rows = sessions[0].tensor(tensor)[2]
            own = [shard_rows(rows, P, p) for p in range(P)]
            need = [tuple(pl[i][2:4]) for pl in plans]
            for q, dst in enumerate(sessions):
                for p, f, n in sharding.needed_from(own, need, q):
                    dst.copy_rows_from(sessions[p], tensor, f, n)
                if need[q] == (0, rows):
                    dst.mark_whole(tensor)
                else:
                    dst.mark_rows(tensor, *need[q])
        for s in sessions:
            s.run_span(first, len(c.ops))
        for p, s in enumerate(sessions):
            assert np.array_equal(s.download(crop.out_dim), crop.rows), f"part {p}"
            pairs = s.pool_pairs(crop.pool_index)
            assert pairs == engine.shard_pool(1, src.C, src.H, src.W, 3, 2, 1, P, p)[4] and 0 < pairs < crop.pool.n_max
    finally:
        for s in sessions:
            s.close()


def test_deployment_key_check_covers_the_pool_tier(crop, tmp_path):
    """save with the policy on, Server and Client in this process: the key check bootstraps its known messages on all 11 tiers; evaluation
    keys whose T6p bootstrap key lost its second half (the last bytes of the blob, zeros in their place) fail it on that tier by name; a
    blob cut short is refused by its length"""
    from dctfhe import deploy
    from dctfhe._lib import DctfheError
    client_path, server_path = deploy.save(crop.qm, str(tmp_path))
    client, server = deploy.Client(client_path), deploy.Server(server_path)
    try:
        client.keygen(seed=9)
        ps = client.spec.param_set
        bits = deploy.key_check_bits(ps)
        assert len(ps.tiers) == 11 and ps.tiers[10].name == "T6p" and len(bits) == 11 and bits[10] == 6
        check = client.make_key_check()
        server.load_evaluation_keys(client.export_evaluation_keys())
        client.verify_key_check(server.answer_key_check(check))
        full = client.export_evaluation_keys(compressed=False)
        t = ps.tiers[10]
        half = t.n * t.l * (t.k + 1) * (t.k + 1) * (t.N // 2) * 16 // 2          # bytes of half its Fourier key: the blob ends with it
        with pytest.raises(DctfheError, match=rf"evaluation-key blob is {full.size - 4096} bytes, its parameters need {full.size}"):
            server.load_evaluation_keys(full[:-4096])
        full[-half:] = 0
        server.load_evaluation_keys(full)
        with pytest.raises(deploy.KeyCheckError, match=r"key check failed on tier 10 \(T6p\)"):
            client.verify_key_check(server.answer_key_check(check))
    finally:
        for r in (server, client):
            r.close()
