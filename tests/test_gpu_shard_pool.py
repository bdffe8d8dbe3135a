"""Divided max pools on one GPU: P sessions of one pooled circuit in one process, each part `p` of `P` with
set_shard + set_shard_pool, driven span by span through the plan with row ranges, the loopback copy between them.  The pool's tree is driven
by host-built index maps and nothing on the server side is random, so EVERY part must end with the unsharded run's output ciphertexts word
for word -- and in clear mode and `simulate` with the unsharded run's words and noise draws -- while it reads only its need range of the
pool's source and runs only its own pairwise maxima."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shard_pool_worker.py")
LIMIT_S = 240

PATTERN = 0x5A5A5A5A5A5A5A5A      # what the rows outside a part's need range are overwritten with (an int64 bit pattern)

GEOMS = {"k3s2-9": (9, (3, 2, 1)), "k2s2-6": (6, (2, 2, 1)), "k7s4-11": (11, (7, 4, 1))}


def _compile(img, pool1, batch):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (20, 4, img, img))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(img_size=img, pool1=pool1), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params())
    return qm, qm.encode_input(qm.quantize_input(calib[:batch]))


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    k = Keys(gpu_ctx, P.to_c_params(P.test_params()), seed=3)
    yield k
    k.close()


class Case:
    """one pooled circuit, one input of `batch` images; encrypted (keys given): the unsharded reference rows, computed once, never modified"""

    def __init__(self, ctx, keys, geom, batch=1):
        from dctfhe import compile as cc
        from dctfhe.engine import Circuit, Session
        self.ctx, self.keys, self.batch = ctx, keys, batch
        self.qm, self.phases = _compile(*GEOMS[geom], batch)
        c = self.qm.compiled
        self.circuit = Circuit(ctx, c.blob)
        self.n_ops = len(c.ops)
        (self.pool_op,) = [i for i, o in enumerate(c.ops) if o.type == cc.OP_MAXPOOL]
        o, src = c.ops[self.pool_op], c.tensors[c.ops[self.pool_op].src0]
        self.pool_src, self.pool_dst = o.src0, o.dst
        self.pool_args = (batch, src.C, src.H, src.W, o.pool.k, o.pool.stride, o.pool.pad)
        self.undivided_pairs = batch * sum(mult * sum(levels) for mult, levels in cc.pool_geometry(src.C, src.H, src.W, o.pool.k, o.pool.stride, o.pool.pad))
        self.ref_session = None
        if keys is not None:
            self.seeded = keys.encrypt_seeded(self.phases.reshape(-1))
            ref = Session(ctx, self.circuit, keys, batch)
            ref.upload_seeded(self.seeded)
            ref.run()
            self.out_dim = ref.dims()[1]
            self.ref_rows = ref.download(self.out_dim)
            self.ref_rows.setflags(write=False)
            self.ref_session = ref

    def plans(self, P):
        return [self.qm.compiled.shard_plan(rows=True, part=p, parts=P, batch=self.batch) for p in range(P)]

    def close(self):
        if self.ref_session is not None:
            self.ref_session.close()
        self.circuit.close()


@pytest.fixture(scope="module")
def cases(gpu_ctx, keys):
    made = {}

    def get(geom, batch=1, encrypted=True):
        key = (geom, batch, encrypted)
        if key not in made:
            made[key] = Case(gpu_ctx, keys if encrypted else None, geom, batch)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _view(session, tensor):
    import torch
    from dctfhe import sharding
    return sharding.tensor_view(session, tensor, torch.device("cuda", 0))


def drive(case, sessions, poison=False, end_op=None):
    """all parts span by span through the plans with row ranges; at each point every session takes, from the parts that own them, the rows
    of its range (copy_rows_from) and says so: mark_whole for a whole tensor, mark_rows for a need range.  poison: once every part has
    its rows of the pool's source, each overwrites the rows of that tensor outside its need range"""
    import torch
    from dctfhe import sharding
    from dctfhe.compile import shard_rows
    P, first = len(sessions), 0
    end_op = case.n_ops if end_op is None else end_op
    plans = case.plans(P)
    for p, s in enumerate(sessions):
        assert s.shard_plan_rows() == plans[p]      # the engine's plan is the compiler's
    for i, (after_op, tensor, _, _) in enumerate(plans[0]):
        if after_op + 1 > end_op:
            break
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
        if poison and tensor == case.pool_src:
            torch.cuda.synchronize()
            for q, s in enumerate(sessions):
                v = _view(s, tensor)
                v[:need[q][0]] = PATTERN
                v[need[q][0] + need[q][1]:] = PATTERN
            torch.cuda.synchronize()
    for s in sessions:
        s.run_span(first, end_op)


def make_sessions(case, P, pool=True, noise=None):
    from dctfhe.engine import Session
    sessions = [Session(case.ctx, case.circuit, case.keys, case.batch) for _ in range(P)]
    for p, s in enumerate(sessions):
        s.set_shard(p, P)
        if pool:
            s.set_shard_pool(True)
        if case.keys is not None:
            s.upload_seeded(case.seeded)
        else:
            if noise is not None:
                s.set_noise(noise[0], noise[1])
                s.set_noise_split(noise[2])
            s.upload(case.phases)
    return sessions


def close_all(sessions):
    for s in sessions:
        s.close()


def _oracle(case):
    from oracle import circuit_ref
    want, overflow = circuit_ref.run_clear(case.qm.compiled.blob, case.phases)
    assert not overflow
    return want


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("geom", ["k3s2-9", "k2s2-6"])
def test_encrypted_word_for_word_and_pairs(cases, geom, P):
    """9 x 9 under (3, 2, 1): two-tap windows at both ends, odd size; P = 5 slices mid-channel, so parts share halo intermediates.
    6 x 6 under (2, 2, 1): single-tap windows, so the last level is no identity and a part ends in the extra gather.
    The pool-pair counter of every part is dctfhe_shard_pool's figure; at P = 2 each is strictly below the undivided count."""
    from dctfhe import engine
    case = cases(geom)
    sessions = make_sessions(case, P)
    try:
        drive(case, sessions)
        want = case.qm.decode_output(_oracle(case))
        for p, s in enumerate(sessions):
            rows = s.download(case.out_dim)
            assert np.array_equal(rows, case.ref_rows), f"part {p} of {P}"
            got = case.keys.decrypt(rows.reshape(-1, case.out_dim + 1), case.out_dim).reshape(case.batch, -1)
            assert np.array_equal(case.qm.decode_output(got), want), f"part {p} of {P}"
            pairs = s.pool_pairs(case.pool_op)
            print(f"{geom} part {p} of {P}: {pairs} pairwise maxima, undivided {case.undivided_pairs}")
            assert pairs == engine.shard_pool(*case.pool_args, P, p)[4]
            if P == 2:
                assert 0 < pairs < case.undivided_pairs
    finally:
        close_all(sessions)


def test_set_shard_alone_runs_the_whole_pool(cases):
    """today's behaviour, pinned: without set_shard_pool every part runs every pairwise maximum, as the unsharded session does"""
    case = cases("k3s2-9")
    assert case.ref_session.pool_pairs(case.pool_op) == case.undivided_pairs
    assert case.undivided_pairs == case.qm.compiled.ops[case.pool_op].pool.n_max * case.batch
    plan = case.qm.compiled.shard_plan()
    sessions = make_sessions(case, 2, pool=False)
    try:
        from dctfhe.compile import shard_rows
        first = 0
        assert sessions[0].shard_plan() == plan
        assert sessions[0].shard_plan_rows() == [(a, t, 0, sessions[0].tensor(t)[2]) for a, t in plan]
        for after_op, tensor in plan:
            for s in sessions:
                s.run_span(first, after_op + 1)
            first = after_op + 1
            rows = sessions[0].tensor(tensor)[2]
            for q, dst in enumerate(sessions):
                dst.copy_rows_from(sessions[1 - q], tensor, *shard_rows(rows, 2, 1 - q))
                dst.mark_whole(tensor)
        for s in sessions:
            s.run_span(first, case.n_ops)
        for s in sessions:
            assert s.pool_pairs(case.pool_op) == case.undivided_pairs
            assert np.array_equal(s.download(case.out_dim), case.ref_rows)
    finally:
        close_all(sessions)


def _worker(mode):
    """tests/shard_pool_worker.py in a fresh interpreter under its own time limit: the cases that wrap a session's memory as a torch tensor
    (torch must initialise the GPU before the library does, which a test process that already holds a context cannot offer)"""
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, WORKER, "--mode", mode], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    return json.loads(line[len("RESULT "):])


def test_only_the_need_range_is_read():
    """P = 3, encrypted, both geometries: every row of the pool's source outside a part's need range is overwritten before the pool runs
    (drive(poison=True) in the worker), and every part still ends with the unsharded run's rows"""
    res = _worker("poison")
    assert sorted((x["geom"], x["part"]) for x in res) == [(g, p) for g in ("k2s2-6", "k3s2-9") for p in range(3)]
    for x in res:
        print(x)
        assert x["tensor"] == x["pool_src"] and 0 < x["rows_overwritten"] < x["rows"], x
        assert x["equal"], x


def test_unmarked_need_range_is_refused(cases):
    """a status code naming op, tensor and rows -- and the session goes on once the rows are there"""
    from dctfhe._lib import DctfheError
    from dctfhe.compile import shard_rows
    from dctfhe.engine import device_bytes_live
    case = cases("k3s2-9")
    sessions = make_sessions(case, 5)
    try:
        plans = case.plans(5)
        after_op, tensor, f, n = plans[1][0]
        assert tensor == case.pool_src and after_op + 1 == case.pool_op
        for s in sessions:
            s.run_span(0, case.pool_op)
        live = device_bytes_live()
        own = shard_rows(sessions[1].tensor(tensor)[2], 5, 1)
        assert f < own[0] and f + n > own[0] + own[1]      # part 1 needs rows on both sides of its own
        with pytest.raises(DctfheError, match=rf"op {case.pool_op} \(max pool\) reads rows {f} \.\. {f + n} of tensor {tensor}, and part 1 of 5 lacks rows {f} \.\. {own[0]}"):
            sessions[1].run_span(case.pool_op, case.pool_op + 1)
        sessions[1].mark_rows(tensor, f, own[0] - f)      # the rows before its own only: the rows behind are still missing
        with pytest.raises(DctfheError, match=rf"tensor {tensor}, and part 1 of 5 lacks rows {own[0] + own[1]} \.\. {f + n}"):
            sessions[1].run_span(case.pool_op, case.pool_op + 1)
        with pytest.raises(DctfheError, match="dctfhe_session_mark_rows: rows"):
            sessions[1].mark_rows(tensor, 0, 10 ** 9)
        assert device_bytes_live() == live
    finally:
        close_all(sessions)
    # the same sessions' work from the start, rows brought in: fine
    sessions = make_sessions(case, 5)
    try:
        drive(case, sessions)
        assert np.array_equal(sessions[1].download(case.out_dim), case.ref_rows)
    finally:
        close_all(sessions)


def _clear_outputs(case, P, noise=None, end_op=None, tensor=None):
    """clear-mode sessions; P = 0: the unsharded run.  -> per part the downloaded outputs, or (end_op given) the rows of `tensor`"""
    from dctfhe.engine import Session
    if P == 0:
        sessions = [Session(case.ctx, case.circuit, None, case.batch)]
        if noise is not None:
            sessions[0].set_noise(noise[0], noise[1])
            sessions[0].set_noise_split(noise[2])
        sessions[0].upload(case.phases)
    else:
        sessions = make_sessions(case, P, noise=noise)
    try:
        if P == 0:
            sessions[0].run_span(0, case.n_ops if end_op is None else end_op)
        else:
            drive(case, sessions, end_op=end_op)
        if end_op is None:
            return [s.download() for s in sessions]
        return [_view(s, tensor).cpu().numpy().copy() for s in sessions]
    finally:
        close_all(sessions)


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_clear_mode_equals_unsharded(cases, geom, P):
    """11 x 11 under (7, 4, 1): three levels per pass, and an input row no window reads"""
    case = cases(geom, encrypted=False)
    ref = _clear_outputs(case, 0)[0]
    assert np.array_equal(ref.reshape(case.batch, -1), _oracle(case).reshape(case.batch, -1))
    for p, out in enumerate(_clear_outputs(case, P)):
        assert np.array_equal(out, ref), f"part {p} of {P}"


def test_clear_mode_batch_two(cases):
    """two images at P = 3: 2 x 150 outputs in ranges of 100, the middle one across the image boundary"""
    case = cases("k3s2-9", batch=2, encrypted=False)
    ref = _clear_outputs(case, 0)[0]
    assert np.array_equal(ref.reshape(2, -1), _oracle(case).reshape(2, -1))
    for p, out in enumerate(_clear_outputs(case, 3)):
        assert np.array_equal(out, ref), f"part {p} of 3"


def test_simulate_draws_the_unsharded_pool_noise():
    """`simulate` with a fixed seed: the noise of a pairwise maximum is drawn by the number of its output in the whole pass, whichever
    part computes it.  The model's sigma is far too small to move a relu table entry, so the pool gets a sigma of 1/32 of the torus (the
    half-box of its 5-bit table is 1/128) and the run stops behind the pool, where each part's rows of the pool's output are compared
    with the unsharded session's (in the worker: the rows are read through the tensor's pointer) -- a look-up behind the pool could
    leave its padded range on such maxima.  All three geometries, P = 2, 3, 5."""
    res = _worker("simulate")
    assert sorted((x["geom"], x["parts"], x["part"]) for x in res) == sorted((g, P, p) for g in GEOMS for P in (2, 3, 5) for p in range(P))
    for x in res:
        assert x["words_moved_by_noise"] > 0, x      # the noise bites: equal rows mean equal draws
        assert x["equal"], x
    print({g: [x["words_moved_by_noise"] for x in res if x["geom"] == g][0] for g in GEOMS}, "pool output words moved by the noise")


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_simulate_whole_circuit(cases, geom, P):
    """the whole circuit with the model's sigmas and, as tests/test_gpu_shard.py does, an eighth of the torus on the last look-up: the
    downloaded outputs of every part equal the unsharded run's"""
    from dctfhe import compile as cc
    case = cases(geom, encrypted=False)
    c = case.qm.compiled
    sig, sig2 = list(c.simulation_sigmas()), list(c.simulation_sigmas_split())
    last = max(i for i, o in enumerate(c.ops) if o.type == cc.OP_LUT)
    sig[last] = 0.125
    ref = _clear_outputs(case, 0, (7, sig, sig2))[0]
    quiet = _clear_outputs(case, 0, None)[0]
    assert (ref != quiet).any()
    for p, out in enumerate(_clear_outputs(case, P, (7, sig, sig2))):
        assert np.array_equal(out, ref), f"part {p} of {P}"


def test_refusals(cases, keys):
    from dctfhe._lib import DctfheError
    from dctfhe.engine import Session, device_bytes_live
    case = cases("k3s2-9")
    fresh, audited, sharded = (Session(case.ctx, case.circuit, keys, 1) for _ in range(3))
    try:
        audited.set_audit(keys)
        audited.set_shard(0, 1)
        sharded.set_shard(1, 2)
        sharded.set_shard_pool(True)
        live = device_bytes_live()
        with pytest.raises(DctfheError, match="not sharded: call dctfhe_session_set_shard first"):
            fresh.set_shard_pool(True)
        assert device_bytes_live() == live
        with pytest.raises(DctfheError, match="dctfhe_session_set_shard_pool: the session has run"):
            case.ref_session.set_shard_pool(True)
        assert device_bytes_live() == live
        with pytest.raises(DctfheError, match="dctfhe_session_set_shard_pool: the margin audit is on"):
            audited.set_shard_pool(True)
        assert device_bytes_live() == live
        with pytest.raises(DctfheError, match="turn that off first"):
            sharded.set_shard(0, 2)
        with pytest.raises(DctfheError, match="is not a max pool"):
            sharded.pool_pairs(0)
        assert device_bytes_live() == live
        audited.set_audit(None)
        live = device_bytes_live()
        # off plans the whole op's level buffers again, never less than the part's; on again gives the part's plan back
        sharded.set_shard_pool(False)
        assert device_bytes_live() >= live
        sharded.set_shard_pool(True)
        assert device_bytes_live() == live
    finally:
        for s in (fresh, audited, sharded):
            s.close()
