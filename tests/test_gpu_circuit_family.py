"""The circuit family (tests/circuit_family.py) on the device: for every topology of the list the clear-mode run and the encrypted run
equal the numpy interpreter element for element (the approximate-rounding case within the bound test_approximate_rounding_small_rings
holds the miniature to), the engine counts the bootstraps the compiler counts, and a second pass over one upload, a sharded loopback
of two and of three parts, a run in channel slabs and the packed download paths give what the plain session gives: for the divided runs
the same ciphertext WORDS.  A pass takes milliseconds on these rings, so every case takes every path -- among them the pooled, the
zero-block, the three-stage and the parity-split ones that tests/test_circuit_family_host.py singles out (DIVIDED, TWICE, PACKED).
One key set per case; the interpreter's outputs are computed once per case and shared.  Every test prints its wall time."""
import time

import numpy as np
import pytest

import circuit_family as F
import packed_ref
import ring_ref
from test_circuit_family_host import REFUSAL, UNDIVIDABLE

pytestmark = pytest.mark.gpu

KEY_SEED = 20261021


class Module:
    """one case's QuantizedModule with its keys, the fresh inputs as integers and what the interpreter makes of them"""

    def __init__(self, name):
        from dctfhe import params as P
        from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
        self.name, self.case = name, F.BY_NAME[name]
        kw = dict(self.case.kw)
        rtb, method = kw.pop("rounding_threshold_bits"), kw.pop("rounding_method", "exact")
        self.qm = compile_brevitas_qat_model(self.case.model(), self.case.calib(), param_set=P.test_params(),
                                             rounding_threshold_bits=rtb if method == "exact" else {"n_bits": rtb, "method": method},
                                             configuration=Configuration(result_packing_spec=P.test_pack_spec()), **kw)
        try:
            assert self.qm.compiled.blob == F.compiled(name).blob          # the circuit the host tests vouch for
            self.q = self.qm.quantize_input(self.case.fresh_inputs())
            self.want, overflow = F.interpreter(name)
            assert not overflow
            self.qm.fhe_circuit.keygen(seed=KEY_SEED + F.NAMES.index(name))
        except BaseException:
            self.qm.close()
            raise

    keys = property(lambda s: s.qm._keys)

    def cts(self, sess, batch=F.BATCH):
        """the fresh inputs encrypted in the session's compact wire form -> (rows, row width)"""
        in_dim = sess.dims()[0]
        return self.keys.encrypt(self.qm.encode_input(self.q[:batch]).reshape(-1), in_dim), in_dim

    def session(self, batch=F.BATCH):
        from dctfhe.engine import Session
        return Session(self.qm._ctx, self.qm._circuit, self.keys, batch)

    def decoded(self, rows, dim, batch=F.BATCH):
        return self.qm.decode_output(self.keys.decrypt(rows.reshape(-1, dim + 1), dim).reshape(batch, -1))

    def check(self, got, batch=F.BATCH):
        """exact cases: element for element; the approximate one: more than half the outputs equal, none more than 4 units off"""
        want = self.want[:batch]
        assert got.shape == want.shape == (batch, self.qm.compiled.n_out())
        if self.case.exact:
            assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        else:
            diff = np.abs(got - want)
            print("%s: exact outputs %.1f%%, max |diff| %d" % (self.name, 100.0 * (diff == 0).mean(), diff.max()))
            assert (diff == 0).mean() > 0.5 and diff.max() <= 4


@pytest.fixture(scope="module")
def modules():
    """name -> Module, made on first use and shared by the tests of this file"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Module(name)
        return made[name]
    yield get
    for m in made.values():
        m.qm.close()


@pytest.fixture
def fam(modules, name):
    return modules(name)


def every(names):
    return pytest.mark.parametrize("name", list(names))


class clock:
    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t0 = time.time()

    def __exit__(self, *exc):
        print("%s: %.2f s" % (self.what, time.time() - self.t0))


@every(F.NAMES)
def test_clear_mode_equals_the_interpreter(fam):
    """noise-free on the device: every case bit for bit, the approximate one too (rounding is exact without noise)"""
    with clock(fam.name + " clear, batch %d" % F.BATCH):
        got = fam.qm.forward_quantized(fam.q, "disable")
    assert got.shape == fam.want.shape and np.array_equal(got, fam.want), np.argwhere(got != fam.want)[:5]


@every(F.NAMES)
@pytest.mark.parametrize("batch", [1, F.BATCH])
def test_encrypted_equals_the_interpreter(fam, batch):
    with clock(fam.name + " encrypted, batch %d" % batch):
        got = fam.qm.forward_quantized(fam.q[:batch], "execute")
    fam.check(got, batch)


@every(F.NAMES)
def test_engine_counts_the_compilers_bootstraps(fam):
    c = fam.qm.compiled
    names = [t.name for t in c.param_set.tiers]
    st = fam.qm.fhe_circuit.statistics
    got = {nm: int(n) for nm, n in zip(names, list(st.pbs_count)) if n}
    print(fam.name, "bootstraps / image", got)
    assert got == c.pbs_counts() and not any(list(st.pbs_count)[len(names):])
    assert st.n_ops == len(c.ops) and st.max_bit_width == c.max_bit_width
    assert st.lut_sites == sum(c.tensors[o.src0].C * c.tensors[o.src0].H * c.tensors[o.src0].W for o in c.ops if o.type == 4)


@every(F.NAMES)
def test_two_passes_over_one_upload(fam):
    """upload once, run twice: the second pass finds the first's leftovers in every buffer and the input where it was"""
    sess = fam.session()
    try:
        cts, in_dim = fam.cts(sess)
        out_dim = sess.dims()[1]
        sess.upload(cts, in_dim)
        with clock(fam.name + " two passes, batch %d" % F.BATCH):
            for _ in range(2):
                sess.run()
                fam.check(fam.decoded(sess.download(out_dim), out_dim))
    finally:
        sess.close()


def _plain_rows(fam):
    """(input rows, their width, the plain session's output rows at full width) of one upload"""
    sess = fam.session()
    try:
        cts, in_dim = fam.cts(sess)
        sess.upload(cts, in_dim)
        sess.run()
        rows = sess.download()
    finally:
        sess.close()
    rows.setflags(write=False)
    fam.check(fam.decoded(rows, fam.keys.D))
    return cts, in_dim, rows


@every(F.NAMES)
@pytest.mark.parametrize("n_parts", [2, 3])
def test_sharded_loopback_word_for_word(fam, n_parts):
    """sessions of one circuit, each one part of every look-up and add, driven span by span through the exchange plan: nothing on
    the server is random, so every part ends with the plain session's ciphertext words"""
    from test_gpu_shard import drive
    c = fam.qm.compiled
    cts, in_dim, ref = _plain_rows(fam)
    parts = [fam.session() for _ in range(n_parts)]
    try:
        assert parts[0].shard_plan() == c.shard_plan()
        for p, s in enumerate(parts):
            s.set_shard(p, n_parts)
            s.upload(cts, in_dim)
        with clock(fam.name + " %d-part loopback, batch %d" % (n_parts, F.BATCH)):
            drive(parts, c.shard_plan(), len(c.ops))
        for p, s in enumerate(parts):
            got = s.download()
            assert np.array_equal(got, ref), (p, np.argwhere(got != ref)[:5])
    finally:
        for s in parts:
            s.close()


@every(F.NAMES)
@pytest.mark.parametrize("n_parts", [2, 3])
def test_engine_row_plans_equal_the_compilers(fam, n_parts):
    """with the max pools divided too, every part's exchange plan with its row ranges (a divided pool's need range) is the list the
    compiler gives; nothing runs"""
    c = fam.qm.compiled
    for part in range(n_parts):
        sess = fam.session()
        try:
            sess.set_shard(part, n_parts)
            sess.set_shard_pool(True)
            assert sess.shard_plan_rows() == c.shard_plan(rows=True, part=part, parts=n_parts, batch=F.BATCH)
        finally:
            sess.close()


def _slab_run(fam, cts, in_dim, budget=None, heights=None):
    from dctfhe.engine import device_bytes_live
    before = device_bytes_live()
    sess = fam.session()
    try:
        sess.upload(cts, in_dim)
        if budget is not None:
            sess.set_memory_budget(budget)
        else:
            sess.set_slab_heights(heights)
        plan = sess.memory_plan()
        assert any(g["slab"] < g["channels"] for g in plan["groups"]), plan
        held = device_bytes_live() - before
        assert held == plan["bytes_planned"] and (budget is None or held <= budget)
        sess.run()
        assert device_bytes_live() - before == held, "the run grew the session"
        return sess.download(), plan
    finally:
        sess.close()


@every(F.NAMES)
def test_channel_slabs_word_for_word(fam):
    """under the first budget below the undivided plan and under the smallest plan the planner finds; a case no budget divides (its
    refusal is the documented one) runs at slab heights set by hand, half the channels and one channel at a time"""
    from dctfhe._lib import DctfheError
    c = fam.qm.compiled
    cts, in_dim, ref = _plain_rows(fam)
    free = c.memory_plan(batch=F.BATCH)
    if fam.name in UNDIVIDABLE[True]:
        sess = fam.session()
        try:
            with pytest.raises(DctfheError, match=REFUSAL % (free["bytes_undivided"] - 1)):
                sess.set_memory_budget(free["bytes_undivided"] - 1)
        finally:
            sess.close()
        channels = [g["channels"] for g in free["groups"]]
        settings = [dict(heights=[max(1, (ch + 1) // 2) for ch in channels]), dict(heights=[1] * len(channels))]
    else:
        plans = [free]
        while True:
            try:
                plans.append(c.memory_plan(batch=F.BATCH, budget_bytes=plans[-1]["bytes_planned"] - 1))
            except DctfheError as e:
                assert REFUSAL % (plans[-1]["bytes_planned"] - 1) in str(e), str(e)
                break
        settings = [dict(budget=b) for b in sorted({plans[1]["bytes_planned"], plans[-1]["bytes_planned"]}, reverse=True)]
    for kw in settings:
        with clock("%s slabs %r, batch %d" % (fam.name, kw, F.BATCH)):
            got, plan = _slab_run(fam, cts, in_dim, **kw)
        print(fam.name, "slab heights", [(g["slab"], g["channels"]) for g in plan["groups"]])
        assert np.array_equal(got, ref), (kw, np.argwhere(got != ref)[:5])


@every(F.NAMES)
def test_packed_and_ring_packed_downloads(fam):
    """the outputs key-switched and packed to 16-bit rows, and ring-packed (zero-blocks: 459 results, a full ring of 256 and a partial
    one; the others: one partial ring): row for row / word for word what the numpy restatements make of the plain download, and the interpreter's outputs once decrypted"""
    qm, keys = fam.qm, fam.keys
    qm.fhe_circuit.load_result_packing_key(qm.fhe_circuit.export_result_packing_key())
    rows_oc, ring_oc = qm.output_compaction(), qm.output_compaction("ring")
    sess = fam.session()
    try:
        cts, in_dim = fam.cts(sess)
        out_dim = sess.dims()[1]
        sess.upload(cts, in_dim)
        with clock(fam.name + " run + packed + ring downloads, batch %d" % F.BATCH):
            sess.run()
            packed = sess.download_packed(rows_oc.tier)
            ring = sess.download_ring(ring_oc.tier, qm._pack_key)
        full = sess.download().reshape(-1, keys.D + 1)
    finally:
        sess.close()
    count = F.BATCH * qm.compiled.n_out()
    assert len(packed) == count and packed.n == rows_oc.n
    assert np.array_equal(packed.rows, packed_ref.pack16(keys.keyswitch(rows_oc.tier, full, 0, out_dim)))
    fam.check(qm.decode_output(keys.decrypt_packed(packed).reshape(F.BATCH, -1)))
    assert len(ring) == count and ring.logN == ring_oc.spec.logN and ring.words.size == ring_oc.spec.words(count)
    small = keys.keyswitch(ring_oc.tier, full, 0, out_dim)
    want = ring_ref.pack16(ring_ref.pack(small, qm._pack_key.export_rows(), ring_oc.spec.l, ring_oc.spec.beta), count)
    assert np.array_equal(ring.words, want)
    fam.check(qm.decode_output(keys.decrypt_ring(ring).reshape(F.BATCH, -1)))
    fam.check(qm.decrypt_result(ring.to_bytes()))
    fam.check(qm.decrypt_result(packed))

