"""dctfhe_circuit_stats against the compiler's own account of each site: every look-up mode and hand-over slot of an op record reaches
the engine's decode (csrc/circuit.h) and its enumeration of a site's bootstraps.  Loads blobs and reads their statistics only: no key
generation, no bootstrap.  The expected values come from CompiledCircuit.ops through compile.step_tier / chain_steps / is_split /
second_tier, never from the engine."""
import functools

import numpy as np
import pytest

from dctfhe import compile as cc, models, params as P
from dctfhe.engine import Circuit
from dctfhe.synthetic import synthetic_dct_batch

pytestmark = pytest.mark.gpu


def _tiny(**kw):
    return cc.compile_model(models.tiny_resnet_q(), np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6)), param_set=P.test_params(), **kw)


def _pooled():      # the smallest max-pool model of tests/test_maxpool_host.py
    calib = np.random.default_rng(1).normal(0, 1, (24, 4, 6, 6))
    return cc.compile_model(models.tiny_resnet_q(img_size=6, pool1=(3, 1, 1), bit_width=4), calib, n_bits=5, param_set=P.test_params())


def _resnet20(bit_width=4, **kw):
    return cc.compile_model(models.ResNet20QAT(bit_width, 24, 16), synthetic_dct_batch(24, seed=7), **kw)


CASES = {
    "tiny_exact6": lambda: _tiny(rounding_threshold_bits=6),
    "tiny_approx6": lambda: _tiny(rounding_threshold_bits=6, rounding_method="approximate"),
    "tiny_split7": lambda: _tiny(rounding_threshold_bits=7),
    "tiny_maxpool": _pooled,
    "resnet20_handovers": _resnet20,
    "resnet20_split7": lambda: _resnet20(n_bits=5, rounding_threshold_bits=7),
    # the quiet twin is a tier of the 5-bit catalogue: only the 5-bit network puts second look-ups on it
    "resnet20_5bit_split7_quiet": lambda: _resnet20(5, n_bits=5, rounding_threshold_bits=7),
}


@functools.lru_cache(maxsize=None)
def compiled(case):      # each circuit is compiled once and shared
    return CASES[case]()


def expected_stats(c):
    """what the engine must count per image, from the compiled ops alone; also the parity and hand-over terms on their own"""
    ps = c.param_set
    names = [t.name for t in ps.tiers]
    pbs = [0] * len(names)
    for nm, n in c.pbs_counts().items():
        pbs[names.index(nm)] += n
    parity = [0] * len(names)
    lut_sites = bit_steps = handed_over = 0
    for o in c.ops:
        if o.type != cc.OP_LUT:
            continue
        s = c.tensors[o.src0]
        n = s.C * s.H * s.W
        steps = 0 if o.ip[9] == cc.LUT_APPROX else cc.chain_steps(o)
        lut_sites += n
        bit_steps += n * steps
        handed_over += n * sum(1 for i in range(steps) if cc.step_tier(o, i) != o.ip[5])
        if cc.is_split(o):      # the parity bootstrap reuses the last step's small ciphertext: no key switch of its own
            parity[cc.step_tier(o, o.r)] += n
    ks = [a - b for a, b in zip(pbs, parity)]
    return dict(pbs=pbs, ks=ks, lut_sites=lut_sites, bit_steps=bit_steps), sum(parity), handed_over


@pytest.mark.parametrize("case", list(CASES))
def test_stats_match_the_compiled_ops(gpu_ctx, case):
    c = compiled(case)
    want, parity, handed_over = expected_stats(c)
    modes = {o.ip[9] for o in c.ops if o.type == cc.OP_LUT}
    if case == "tiny_approx6":
        assert cc.LUT_APPROX in modes and want["bit_steps"] == 0
    if case == "tiny_split7":
        assert cc.LUT_SPLIT in modes and parity > 0
    if case == "tiny_maxpool":
        assert any(o.type == cc.OP_MAXPOOL for o in c.ops)
    if case == "resnet20_handovers":      # B -> Ba -> Ba2: both hand-over slots of a record are live
        assert handed_over > 0 and any(o.ip[7] >= 0 and o.ip[8] < o.r for o in c.ops if o.type == cc.OP_LUT)
        assert any(o.ip[11] >= 0 for o in c.ops if o.type == cc.OP_LUT)
    if case == "resnet20_split7":
        assert cc.LUT_SPLIT in modes and parity > 0 and handed_over > 0
    if case == "resnet20_5bit_split7_quiet":
        assert cc.LUT_SPLIT in modes and cc.LUT_SPLIT_QUIET in modes and parity > 0 and handed_over > 0
    circ = Circuit(gpu_ctx, c.blob)
    try:
        st = circ.stats(P.to_c_params(c.param_set))
    finally:
        circ.close()
    nt = len(c.param_set.tiers)
    got = dict(pbs=list(st.pbs_count)[:nt], ks=list(st.ks_count)[:nt], lut_sites=st.lut_sites, bit_steps=st.bit_steps)
    print(case, "want", want, "got", got, "parity", parity, "handed over", handed_over)
    assert got == want
    assert not any(list(st.pbs_count)[nt:]) and not any(list(st.ks_count)[nt:])
    assert st.n_ops == len(c.ops) and st.max_bit_width == c.max_bit_width
