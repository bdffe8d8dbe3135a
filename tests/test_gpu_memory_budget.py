"""Sessions under a device-memory budget (include/dctfhe.h dctfhe_session_set_memory_budget): a convolution and the
look-ups / max pools behind it run in channel slabs.  On the tiny trunks (stem of 6 channels; no pool, MaxPool(3, 2, 1), MaxPool(2, 2, 0)),
batch 2, at budgets taken from the planner's own figures -- the plan whose stem runs in slabs of 4 + 2 channels and the smallest plan it
finds (MaxPool(3, 2, 1): the stem one channel at a time and the later groups, a convolution and a look-up each, in slabs of 3 + 3 and
7 + 1; MaxPool(2, 2, 0): the stem in slabs of 3 + 3): the output ciphertexts equal the unbudgeted session's WORD FOR WORD (encrypted, clear and `simulate`), the
session holds exactly the planned bytes, and every refusal is refused by its message and leaves the session usable."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import circuit_ref as mref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 2
TRUNKS = {"plain6": (None, 6, 6), "pool321": ((3, 2, 1), 9, 6), "pool220": ((2, 2, 0), 8, 6), "pool321_rtb7": ((3, 2, 1), 9, 7)}


def live():
    from dctfhe.engine import device_bytes_live
    return device_bytes_live()


def _plans(compiled, params, batch):
    """the planner's plans from the undivided one down to the smallest, each found with the bytes of the one before minus one as budget"""
    from dctfhe._lib import DctfheError
    out = [compiled.memory_plan(params=params, batch=batch)]
    while True:
        try:
            out.append(compiled.memory_plan(params=params, batch=batch, budget_bytes=out[-1]["bytes_planned"] - 1))
        except DctfheError as e:      # the planner's refusal ends the descent; anything else is an error
            assert "memory budget of %d bytes: the smallest plan" % (out[-1]["bytes_planned"] - 1) in str(e), str(e)
            return out


class Trunk:
    def __init__(self, ctx, keys, ps, name):
        from dctfhe import compile as cc, models
        from dctfhe.engine import Circuit
        pool, img, rtb = TRUNKS[name]
        calib = np.random.default_rng(3).normal(0, 1, (24, 4, img, img))
        self.compiled = cc.compile_model(models.tiny_resnet_q(img_size=img, pool1=pool), calib[:20], rounding_threshold_bits=rtb, param_set=ps)
        q = cc.act_quant(np.asarray(calib[20:20 + BATCH], np.float64), self.compiled.in_scale, True, self.compiled.in_bits)
        self.phases = (q.astype(np.int64).astype(np.uint64) << np.uint64(self.compiled.e_in)).reshape(-1)
        self.circ = Circuit(ctx, self.compiled.blob)
        self.cts = keys.encrypt(self.phases)
        self.want, overflow = mref.run_clear(self.compiled.blob, self.phases.reshape(BATCH, -1))
        assert not overflow
        self.plans = {True: _plans(self.compiled, None, BATCH), False: _plans(self.compiled, False, BATCH)}      # encrypted / clear
        self._ref = {}

    def budgets(self, encrypted):
        """(bytes of the plan whose stem runs in slabs of 4 + 2, bytes of the smallest plan the planner finds)"""
        plans = self.plans[encrypted]
        four = [p for p in plans if p["groups"][0]["slab"] == 4]
        assert four and plans[-1]["groups"][0]["slab"] <= 4
        return four[0]["bytes_planned"], plans[-1]["bytes_planned"]

    def reference(self, ctx, keys, mode):
        """the unbudgeted session's output words: computed once per mode, shared, read-only"""
        if mode not in self._ref:
            self._ref[mode] = run(ctx, self, keys, mode, None)[0]
            self._ref[mode].flags.writeable = False
        return self._ref[mode]


def run(ctx, trunk, keys, mode, budget, heights=None):
    """-> (output words, bytes the session held); heights: slab heights set by hand instead of a budget"""
    from dctfhe.engine import Session
    before = live()
    sess = Session(ctx, trunk.circ, keys if mode == "execute" else None, BATCH)
    try:
        sess.upload(trunk.cts if mode == "execute" else trunk.phases)       # before the budget: an uploaded input stays where it is
        if budget is not None:
            sess.set_memory_budget(budget)
        if heights is not None:
            sess.set_slab_heights(heights)
            plan = sess.memory_plan()
            assert [g["slab"] for g in plan["groups"]] == list(heights) and live() - before == plan["bytes_planned"]
        if mode == "simulate":
            sess.set_noise(77, trunk.compiled.simulation_sigmas())
            sess.set_noise_split(trunk.compiled.simulation_sigmas_split())
        held = live() - before
        sess.run()
        assert live() - before == held, "the run grew the session"
        return sess.download(), held
    finally:
        sess.close()


@pytest.fixture(scope="module")
def env(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    ps = P.test_params()
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=5)
    trunks = {}

    def get(name):
        if name not in trunks:
            trunks[name] = Trunk(gpu_ctx, keys, ps, name)
            run(gpu_ctx, trunks[name], keys, "execute", None)      # the circuit's convolution packs are made with its first encrypted session
        return trunks[name]
    yield gpu_ctx, keys, get
    for t in trunks.values():
        t.circ.close()
    keys.close()


@pytest.mark.parametrize("which", [0, 1], ids=["slabs_4_2", "smallest_plan"])
@pytest.mark.parametrize("mode", ["execute", "disable", "simulate"])
@pytest.mark.parametrize("name", ["pool321", "pool220"])
def test_budgeted_outputs_equal_the_unbudgeted_word_for_word(env, name, mode, which):
    ctx, keys, get = env
    trunk = get(name)
    encrypted = mode == "execute"
    budget = trunk.budgets(encrypted)[which]
    ref = trunk.reference(ctx, keys, mode)
    got, held = run(ctx, trunk, keys, mode, budget)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert held <= budget
    if mode == "disable":
        assert np.array_equal(got.reshape(trunk.want.shape), trunk.want)
    if mode == "execute":       # decrypted and rounded to the output's exponent: the integer circuit
        e = trunk.compiled.e_out
        dec = keys.decrypt(got.reshape(-1, got.shape[-1]))
        val = ((dec + (np.uint64(1) << np.uint64(e - 1))) >> np.uint64(e)) << np.uint64(e)
        assert np.array_equal(val.reshape(trunk.want.shape), trunk.want)


@pytest.mark.parametrize("mode", ["execute", "disable", "simulate"])
def test_trunk_without_a_pool(env, mode):
    """img_size = 6, no pool: the first block's tensors are as large as the stem's and reuse the buffers it frees, so no cut lowers the
    session's bytes and the planner refuses every budget under the undivided plan (tests/test_memory_plan_host.py); the session says the
    same, stays as it was, and runs.  Its groups run in slabs all the same at heights set by hand (dctfhe_session_set_slab_heights),
    word for word what the undivided session computes."""
    from dctfhe._lib import DctfheError
    from dctfhe.engine import Session
    ctx, keys, get = env
    trunk = get("plain6")
    encrypted = mode == "execute"
    plans = trunk.plans[encrypted]
    assert len(plans) == 1
    ref = trunk.reference(ctx, keys, mode)
    got, held = run(ctx, trunk, keys, mode, plans[0]["bytes_planned"])      # a budget the undivided plan meets: the undivided plan
    assert np.array_equal(got, ref) and held == plans[0]["bytes_planned"]
    # ... so its slabs run at heights set by hand: the stem in slabs of 4 + 2, then every group one channel at a time
    channels = [g["channels"] for g in plans[0]["groups"]]
    assert channels[0] == 6
    for heights in ([4] + channels[1:], [1] * len(channels)):
        got, _ = run(ctx, trunk, keys, mode, None, heights)
        assert np.array_equal(got, ref), (heights, np.argwhere(got != ref)[:5])
    if mode != "simulate":
        before = live()
        sess = Session(ctx, trunk.circ, keys if encrypted else None, BATCH)
        try:
            sess.upload(trunk.cts if encrypted else trunk.phases)
            held = live() - before
            with pytest.raises(DctfheError, match="memory budget of %d bytes: the smallest plan" % (plans[0]["bytes_planned"] - 1)):
                sess.set_memory_budget(plans[0]["bytes_planned"] - 1)
            assert live() - before == held
            sess.run()
            assert np.array_equal(sess.download(), ref)
        finally:
            sess.close()
    if mode == "disable":
        assert np.array_equal(ref.reshape(trunk.want.shape), trunk.want)


def test_parity_split_site_inside_a_group(env):
    ctx, keys, get = env
    trunk = get("pool321_rtb7")
    inner = [i for g in trunk.plans[True][0]["groups"] for i in range(g["first_op"], g["end_op"])]
    assert any(trunk.compiled.ops[i].type == 4 and trunk.compiled.ops[i].lut.split() for i in inner), "no parity-split site inside a slab group"
    ref = trunk.reference(ctx, keys, "execute")
    for budget in sorted(set(trunk.budgets(True))):
        got, held = run(ctx, trunk, keys, "execute", budget)
        assert np.array_equal(got, ref) and held <= budget


@pytest.mark.parametrize("name", ["plain6", "pool321"])
@pytest.mark.parametrize("encrypted", [True, False], ids=["encrypted", "clear"])
def test_the_session_holds_the_planned_bytes(env, name, encrypted):
    from dctfhe.engine import Session
    ctx, keys, get = env
    trunk = get(name)
    plans = trunk.plans[encrypted]
    mode = "execute" if encrypted else "disable"
    _, unbudgeted = run(ctx, trunk, keys, mode, None)
    assert unbudgeted == plans[0]["bytes_undivided"] == plans[0]["bytes_planned"]
    for plan in plans[1:]:
        _, held = run(ctx, trunk, keys, mode, plan["bytes_planned"])
        assert held == plan["bytes_planned"] < unbudgeted, plan
    # the getter: the plan in force
    sess = Session(ctx, trunk.circ, keys if encrypted else None, BATCH)
    try:
        assert sess.memory_plan()["groups"] == plans[0]["groups"] and sess.memory_plan()["budget_bytes"] == 0
        sess.set_memory_budget(plans[-1]["bytes_planned"])
        m = sess.memory_plan()
        assert m["groups"] == plans[-1]["groups"] and m["bytes_planned"] == plans[-1]["bytes_planned"] and m["bytes_undivided"] == plans[0]["bytes_planned"]
    finally:
        sess.close()


def test_refusals_by_message_leave_the_session_usable(env):
    from dctfhe._lib import DctfheError
    from dctfhe.engine import Session
    ctx, keys, get = env
    trunk = get("pool321")
    ref = trunk.reference(ctx, keys, "execute")
    four, smallest = trunk.budgets(True)
    before = live()
    sess = Session(ctx, trunk.circ, keys, BATCH)
    try:
        sess.upload(trunk.cts)
        held = live() - before
        # one byte under the smallest plan: refused, naming the op; nothing moved; the session runs
        with pytest.raises(DctfheError, match=r"memory budget of %d bytes: the smallest plan .* needs %d bytes; .* destination of op \d+" % (smallest - 1, smallest)):
            sess.set_memory_budget(smallest - 1)
        assert live() - before == held
        # the audit is on: refused; off again: accepted
        sess.set_audit(keys)
        with pytest.raises(DctfheError, match="dctfhe_session_set_memory_budget: the margin audit is on"):
            sess.set_memory_budget(four)
        sess.set_audit(None)
        assert live() - before == held
        sess.set_memory_budget(four)
        with pytest.raises(DctfheError, match="dctfhe_session_set_audit: the session has a memory budget"):
            sess.set_audit(keys)
        with pytest.raises(DctfheError, match="dctfhe_session_set_shard: the session has a memory budget"):
            sess.set_shard(0, 2)
        # a span that cuts the divided stem group (ops [0, end))
        g = sess.memory_plan()["groups"][0]
        assert g["first_op"] == 0 and g["end_op"] >= 3 and g["slab"] == 4
        with pytest.raises(DctfheError, match=r"dctfhe_session_run_span: ops \[0, 1\) cut the slab group of ops \[0, %d\)" % g["end_op"]):
            sess.run_span(0, 1)
        with pytest.raises(DctfheError, match=r"dctfhe_session_run_span: ops \[2, %d\) cut the slab group" % len(trunk.compiled.ops)):
            sess.run_span(2, len(trunk.compiled.ops))
        sess.run_span(0, g["end_op"])                       # the whole group, then the rest
        sess.run_span(g["end_op"], len(trunk.compiled.ops))
        assert np.array_equal(sess.download(), ref)
        with pytest.raises(DctfheError, match="dctfhe_session_set_memory_budget: the session has run"):
            sess.set_memory_budget(smallest)
        sess.run()
        assert np.array_equal(sess.download(), ref)
    finally:
        sess.close()
    sharded = Session(ctx, trunk.circ, keys, BATCH)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(DctfheError, match="dctfhe_session_set_memory_budget: the session is part 0 of 2"):
            sharded.set_memory_budget(four)
    finally:
        sharded.close()
    assert live() == before


def test_configuration_budget_equals_the_plain_module():
    from dctfhe import models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    calib = np.random.default_rng(3).normal(0, 1, (24, 4, 9, 9))

    def module(configuration):
        return compile_brevitas_qat_model(models.tiny_resnet_q(img_size=9, pool1=(3, 2, 1)), calib[:20], n_bits=5, rounding_threshold_bits=6,
                                          param_set=P.test_params(), configuration=configuration)
    plain = module(None)
    smallest = _plans(plain.compiled, None, BATCH)[-1]["bytes_planned"]
    budgeted = module(Configuration(device_memory_budget_gb=(smallest + 4096) / 1e9))      # (a few bytes of room: GB are a float)
    try:
        plain.fhe_circuit.keygen(seed=5)
        budgeted.fhe_circuit.keygen(seed=5)
        x = calib[20:20 + BATCH]
        want = plain.forward(x, fhe="execute")
        assert np.array_equal(budgeted.forward(x, fhe="execute"), want)
        assert np.array_equal(budgeted.forward(x, fhe="disable"), want)
        plan = budgeted._session("execute", BATCH).memory_plan()
        assert plan["bytes_planned"] == smallest <= plan["budget_bytes"] < smallest + 8192 and plan["groups"][0]["slab"] < plan["groups"][0]["channels"]
        text = budgeted.compiled.report(memory_budget_bytes=budgeted.configuration.device_memory_budget_bytes, batch=BATCH)
        assert "device memory budget" in text and "planned %d bytes" % smallest in text and "device memory budget" not in plain.compiled.report()
    finally:
        plain.close()
        budgeted.close()


def test_cli_flag_is_accepted():
    env_ = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "dct-cryptonets_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    # the default model (ResNet-18 on 3 x 32 x 32), clear mode: a budget of 1 GB is far above what its session needs
    cmd = [sys.executable, os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"), "--fhe_mode", "disable", "--calib_batch_size", "8",
           "--device_memory_budget_gb", "1", "--verbose", ""]
    r = subprocess.run(cmd, env=env_, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Running ENCRYPTED test inference in DISABLE mode" in r.stdout and "Done" in r.stdout
    r = subprocess.run(cmd + ["--shard_image"], env=env_, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "exclude each other" in r.stderr
