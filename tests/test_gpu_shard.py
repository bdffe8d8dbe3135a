"""Sharded look-up sites on one GPU: P sessions of one circuit in one process, each part `p` of `P`, driven span by
span through the exchange plan with the loopback copy between them.  Nothing on the server side is random, so EVERY part must end with the
unsharded run's output ciphertexts word for word -- and in clear mode and `simulate` with the unsharded run's words and noise draws."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTB_APPROX = {"n_bits": 6, "method": "approximate"}


def _compile(rtb=6, img=6, n=48, batch=2, **model_kw):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (n, 4, img, img))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(img_size=img, **model_kw), calib, n_bits=5, rounding_threshold_bits=rtb, param_set=P.test_params())
    q = qm.quantize_input(calib[:batch])
    return qm, qm.encode_input(q)


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    k = Keys(gpu_ctx, P.to_c_params(P.test_params()), seed=3)
    yield k
    k.close()


class Case:
    """one circuit, one seeded input of `batch` images, the unsharded reference rows (computed once, never modified)"""

    def __init__(self, ctx, keys, batch=2, **kw):
        from dctfhe.engine import Circuit, Session
        self.ctx, self.keys, self.batch = ctx, keys, batch
        self.qm, self.phases = _compile(batch=batch, **kw)
        self.circuit = Circuit(ctx, self.qm.compiled.blob)
        self.plan, self.n_ops = self.qm.compiled.shard_plan(), len(self.qm.compiled.ops)
        self.seeded = keys.encrypt_seeded(self.phases.reshape(-1))
        ref = Session(ctx, self.circuit, keys, batch)
        ref.upload_seeded(self.seeded)
        ref.run()
        self.out_dim = ref.dims()[1]
        self.ref_rows = ref.download(self.out_dim)
        self.ref_rows.setflags(write=False)
        self.ref_session = ref

    def close(self):
        self.ref_session.close()
        self.circuit.close()


def drive(sessions, plan, n_ops):
    """all parts span by span; at each exchange point every session takes the other parts' rows (copy_rows_from) and is told so"""
    from dctfhe.compile import shard_rows
    P, first = len(sessions), 0
    for after_op, tensor in plan:
        for s in sessions:
            s.run_span(first, after_op + 1)
        first = after_op + 1
        rows = sessions[0].tensor(tensor)[2]
        for q, dst in enumerate(sessions):
            for p, src in enumerate(sessions):
                if p != q:
                    dst.copy_rows_from(src, tensor, *shard_rows(rows, P, p))
            dst.mark_whole(tensor)
    for s in sessions:
        s.run_span(first, n_ops)


def sharded_rows(case, P):
    from dctfhe.engine import Session
    sessions = [Session(case.ctx, case.circuit, case.keys, case.batch) for _ in range(P)]
    try:
        assert sessions[0].shard_plan() == case.plan      # the engine's plan is the compiler's
        for p, s in enumerate(sessions):
            s.set_shard(p, P)
            s.upload_seeded(case.seeded)
        drive(sessions, case.plan, case.n_ops)
        return [s.download(case.out_dim) for s in sessions]
    finally:
        for s in sessions:
            s.close()


@pytest.fixture(scope="module")
def tiny(gpu_ctx, keys):
    """two images: sites of 432 and 144 rows, 16 output rows"""
    c = Case(gpu_ctx, keys)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny1(gpu_ctx, keys):
    """one image: sites of 216 (hw = 36) and 72 (hw = 9) rows and 8 output rows (tests/test_shard_host.py checks the shapes)"""
    c = Case(gpu_ctx, keys, batch=1)
    yield c
    c.close()


CASES = [(2, 2), (2, 5), (2, 16), (1, 5), (1, 16)]      # (images, parts)


@pytest.mark.parametrize("batch,P", CASES)
def test_encrypted_word_for_word(tiny, tiny1, batch, P):
    """Two images: 432 = 2 x 87 + 3 x 86 at P = 5, slices start mid-channel.  One image: 216 = 44 + 4 x 43 and 8 = 2 + 2 + 2 + 1 + 1 at
    P = 5; empty parts at the output site at P = 16."""
    from oracle import circuit_ref
    tiny = tiny if batch == 2 else tiny1
    outs = sharded_rows(tiny, P)
    for p, rows in enumerate(outs):
        assert np.array_equal(rows, tiny.ref_rows), f"part {p} of {P}"
    want, overflow = circuit_ref.run_clear(tiny.qm.compiled.blob, tiny.phases)
    assert not overflow
    got = tiny.keys.decrypt(outs[-1].reshape(-1, tiny.out_dim + 1), tiny.out_dim).reshape(batch, -1)
    assert np.array_equal(tiny.qm.decode_output(got), tiny.qm.decode_output(want))


def _clear_outputs(gpu_ctx, case, P, noise):
    """clear-mode sessions (keys = None), P = 0: the unsharded run(); noise: (seed, sigma per op, sigma2 per op) or None"""
    from dctfhe.engine import Session
    sessions = [Session(gpu_ctx, case.circuit, None, case.batch) for _ in range(max(P, 1))]
    try:
        for p, s in enumerate(sessions):
            if P:
                s.set_shard(p, P)
            if noise is not None:
                s.set_noise(noise[0], noise[1])
                s.set_noise_split(noise[2])
            s.upload(case.phases)
        if P:
            drive(sessions, case.plan, case.n_ops)
        else:
            sessions[0].run()
        return [s.download() for s in sessions]
    finally:
        for s in sessions:
            s.close()


@pytest.mark.parametrize("batch,P", CASES)
def test_clear_mode_equals_unsharded(gpu_ctx, tiny, tiny1, batch, P):
    """the per-channel table of an element goes by its number in the whole tensor (k_lut_clear's element offset)"""
    tiny = tiny if batch == 2 else tiny1
    ref = _clear_outputs(gpu_ctx, tiny, 0, None)[0]
    for p, out in enumerate(_clear_outputs(gpu_ctx, tiny, P, None)):
        assert np.array_equal(out, ref), f"part {p} of {P}"


@pytest.mark.parametrize("batch,P", CASES)
def test_simulate_draws_the_unsharded_noise(gpu_ctx, tiny, tiny1, batch, P):
    """`simulate` with a fixed seed: the noise of element e is draw e of the op's stream whichever part looks it up.  The model's sigmas
    are far too small to move an exact tier's output, so the LAST look-up (the output rows; nothing downstream can overflow) gets a
    sigma of an eighth of the torus -- many boxes wide (a half-box of 2^-(w + 2) moved nothing: neighbouring entries of the output
    quantiser's table are mostly equal) -- so that most look-ups land on a far entry"""
    from dctfhe import compile as cc
    tiny = tiny if batch == 2 else tiny1
    c = tiny.qm.compiled
    sig, sig2 = list(c.simulation_sigmas()), list(c.simulation_sigmas_split())
    last = max(i for i, o in enumerate(c.ops) if o.type == cc.OP_LUT)
    assert c.ops[last].dst == c.output_tensor and not c.ops[last].lut.split()
    sig[last] = 0.125
    noise = (20261019, sig, sig2)
    ref = _clear_outputs(gpu_ctx, tiny, 0, noise)[0]
    quiet = _clear_outputs(gpu_ctx, tiny, 0, None)[0]
    print("simulate: output words moved by the noise:", int((ref != quiet).sum()), "of", ref.size)
    assert (ref != quiet).any()      # the noise bites: equal outputs below mean equal draws
    for p, out in enumerate(_clear_outputs(gpu_ctx, tiny, P, noise)):
        assert np.array_equal(out, ref), f"part {p} of {P}"


@pytest.mark.parametrize("kw", [dict(rtb=7), dict(rtb=RTB_APPROX), dict(img=9, n=20, pool1=(3, 2, 1))], ids=["parity-split", "approximate", "pooled"])
def test_variants_word_for_word(gpu_ctx, keys, kw):
    """P = 3.  rounding_threshold_bits=7: parity-split sites (the parity rows, k_acc_rows and the KS_SUM key switch are indexed by the
    launch, the half tables by the element).  Approximate rounding: no chain, the key switch reads the source tensor's slice directly.
    Pooled trunk: the stem's max pool reads an exchanged tensor and runs in full on every part."""
    from dctfhe import compile as cc
    case = Case(gpu_ctx, keys, **kw)
    try:
        ops = case.qm.compiled.ops
        if kw.get("rtb") == 7:
            assert any(o.type == cc.OP_LUT and o.lut.split() for o in ops)
        elif kw.get("rtb") is RTB_APPROX:
            assert any(o.type == cc.OP_LUT and o.lut.approx() and o.lut.r > 0 for o in ops)
        else:
            assert any(o.type == cc.OP_MAXPOOL for o in ops)
        for p, rows in enumerate(sharded_rows(case, 3)):
            assert np.array_equal(rows, case.ref_rows), f"part {p} of 3"
    finally:
        case.close()


def test_refusals(gpu_ctx, tiny):
    from dctfhe._lib import DctfheError
    from dctfhe.engine import Session
    mk = lambda batch=2: Session(gpu_ctx, tiny.circuit, tiny.keys, batch)
    s, other, one = mk(), mk(), mk(1)
    try:
        for bad in ((2, 2), (-1, 2), (0, 0), (0, 65)):
            with pytest.raises(DctfheError, match="dctfhe_shard_rows"):
                s.set_shard(*bad)
        s.set_shard(0, 2)
        s.upload_seeded(tiny.seeded)
        first_conv_behind_a_lookup = tiny.plan[0]
        msg = rf"op \d+ needs tensor {first_conv_behind_a_lookup[1]} whole"
        with pytest.raises(DctfheError, match=msg):
            s.run()                                   # run() is run_span over the whole circuit: refused at the first such op
        with pytest.raises(DctfheError, match=msg):
            s.run_span(0, tiny.n_ops)
        with pytest.raises(DctfheError, match="has run"):
            s.set_shard(1, 2)
        with pytest.raises(DctfheError, match="unsharded"):
            s.set_audit(tiny.keys)
        # the spans in order, every tensor declared whole except the output: each download refuses
        first = 0
        for after_op, tensor in tiny.plan:
            s.run_span(first, after_op + 1)
            first = after_op + 1
            if tensor != tiny.qm.compiled.output_tensor:
                s.mark_whole(tensor)
        s.run_span(first, tiny.n_ops)
        with pytest.raises(DctfheError, match=r"output tensor \d+ holds only the rows of part 0 of 2"):
            s.download(tiny.out_dim)
        with pytest.raises(DctfheError, match="holds only the rows"):
            s.download_packed(0)
        # an audited session cannot be sharded, and says why
        other.set_audit(tiny.keys)
        with pytest.raises(DctfheError, match="stays unsharded"):
            other.set_shard(0, 2)
        other.set_audit(None)
        with pytest.raises(DctfheError, match="batch"):
            one.copy_rows_from(other, tiny.plan[0][1], 0, 1)
        with pytest.raises(DctfheError, match="rows"):
            other.copy_rows_from(s, tiny.plan[0][1], 0, 10 ** 9)
        with pytest.raises(DctfheError, match="has run"):
            tiny.ref_session.set_shard(0, 2)
    finally:
        for x in (s, other, one):
            x.close()
