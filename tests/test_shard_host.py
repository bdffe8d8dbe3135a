"""Sharded look-up sites, the host side: the partition rule -- the library's dctfhe_shard_rows, which needs no GPU,
against its Python mirror and against brute force -- the compiler's exchange plan on three circuits, and the promise that the switch
changes nothing a circuit is compiled to.  No GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("circuit_digests", os.path.join(ROOT, "tools", "circuit_digests.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

ROWS = (0, 1, 7, 8, 216)
PARTS = (1, 2, 3, 5, 16, 64)


def _brute(rows, parts):
    """deal the rows out one at a time, round robin: the sizes of the rule; the parts then take consecutive rows in order"""
    sizes = [0] * parts
    for i in range(rows):
        sizes[i % parts] += 1
    out, first = [], 0
    for n in sizes:
        out.append((first, n))
        first += n
    return out


@pytest.fixture(scope="module")
def lib_shard_rows():
    from dctfhe import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return engine.shard_rows


@pytest.mark.parametrize("parts", PARTS)
def test_shard_rows_rule(lib_shard_rows, parts):
    from dctfhe import compile as cc
    for rows in ROWS:
        want = _brute(rows, parts)
        got = [cc.shard_rows(rows, parts, p) for p in range(parts)]
        assert got == want, (rows, parts)
        assert [lib_shard_rows(rows, parts, p) for p in range(parts)] == want, (rows, parts)
        # the ranges tile [0, rows) in order, sizes differ by at most one, the larger ones first
        assert got[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:])) and got[-1][0] + got[-1][1] == rows
        sizes = [n for _, n in got]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


@pytest.mark.parametrize("parts,part", [(0, 0), (-1, 0), (65, 0), (2, 2), (2, -1), (64, 64), (1, 1)])
def test_shard_rows_refusals(lib_shard_rows, parts, part):
    from dctfhe import compile as cc
    from dctfhe._lib import DctfheError
    with pytest.raises(ValueError):
        cc.shard_rows(216, parts, part)
    with pytest.raises(DctfheError, match="dctfhe_shard_rows"):
        lib_shard_rows(216, parts, part)


def _check_plan(c):
    from dctfhe import compile as cc
    plan = c.shard_plan()
    whole_readers = (cc.OP_CONV, cc.OP_SUMPOOL, cc.OP_MAXPOOL)
    sliced_writers = (cc.OP_LUT, cc.OP_ADD)
    writer = {o.dst: i for i, o in enumerate(c.ops)}
    sliced = {o.dst for o in c.ops if o.type in sliced_writers}
    read_whole = {o.src0 for o in c.ops if o.type in whole_readers} | {c.output_tensor}
    read_sliced_only = ({o.src0 for o in c.ops if o.type in sliced_writers} | {o.src1 for o in c.ops if o.type == cc.OP_ADD}) - read_whole
    tensors = [t for _, t in plan]
    # every tensor a convolution or pool reads, and the output, exactly once (those an element-wise op wrote: the others are whole anyway)
    assert sorted(tensors) == sorted(read_whole & sliced)
    assert len(set(tensors)) == len(tensors)
    assert not set(tensors) & read_sliced_only
    # in op order, each right after the op that writes the tensor
    assert [a for a, _ in plan] == sorted(a for a, _ in plan)
    assert all(a == writer[t] for a, t in plan)
    return plan


def test_plan_tiny_trunk():
    from dctfhe import compile as cc
    c = tool.compile_case(dict(id="tiny-rtb6", tiny=dict(), rtb=6, seed=0, n=48, img=6))
    plan = _check_plan(c)
    assert c.output_tensor in [t for _, t in plan]
    # the residual sums feed look-ups only: they never travel
    adds = {o.dst for o in c.ops if o.type == cc.OP_ADD}
    assert adds and not adds & {t for _, t in plan}


def test_tiny_trunk_shapes():
    """what tests/test_gpu_shard.py relies on: per image, sites of 216 rows (hw = 36) and 72 rows (hw = 9) and 8 output rows; per-channel
    tables (a slice that starts mid-channel needs its element offset); the last look-up writes the output; and the variants hold what
    they are run for -- parity-split sites, approximate sites that round, a max pool"""
    import numpy as np
    from dctfhe import compile as cc, models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model

    def circuit(rtb=6, img=6, n=48, **kw):
        calib = np.random.default_rng(0).normal(0, 1, (n, 4, img, img))
        return compile_brevitas_qat_model(models.tiny_resnet_q(img_size=img, **kw), calib, n_bits=5, rounding_threshold_bits=rtb, param_set=P.test_params()).compiled
    c = circuit()
    luts = [o for o in c.ops if o.type == cc.OP_LUT]
    sites = {(c.tensors[o.src0].C * c.tensors[o.src0].H * c.tensors[o.src0].W, c.tensors[o.src0].H * c.tensors[o.src0].W) for o in luts}
    assert {(216, 36), (72, 9)} <= sites and c.n_out() == 8
    assert any(o.lut.ntab > 1 for o in luts)
    assert luts[-1].dst == c.output_tensor and not luts[-1].lut.split() and c.ops[-1] is luts[-1]
    assert any(o.type == cc.OP_LUT and o.lut.split() for o in circuit(rtb=7).ops)
    assert any(o.type == cc.OP_LUT and o.lut.approx() and o.lut.r > 0 for o in circuit(rtb={"n_bits": 6, "method": "approximate"}).ops)
    assert any(o.type == cc.OP_MAXPOOL for o in circuit(img=9, n=20, pool1=(3, 2, 1)).ops)


def test_plan_pooled_trunk():
    from dctfhe import compile as cc
    c = tool.compile_case(dict(id="tiny-pool-rtb6", tiny=dict(pool1=[3, 2, 1]), rtb=6, seed=0, n=20, img=9))
    plan = _check_plan(c)
    pools = [o for o in c.ops if o.type == cc.OP_MAXPOOL]
    assert len(pools) == 1 and pools[0].src0 in [t for _, t in plan]        # the stem's look-up output reaches the max pool whole
    assert pools[0].dst not in [t for _, t in plan]                         # ... and the pool's own output is computed whole on every part


def test_plan_resnet20():
    c = tool.compile_case(tool.CASES[0])
    assert tool.CASES[0]["id"] == "r20_24_16-bw4-rtb6"
    plan = _check_plan(c)
    assert 15 <= len(plan) <= 30        # about two dozen exchanges: one per convolution input behind a look-up, the pool's, the output


def test_switch_changes_no_compiled_byte():
    """Configuration(shard_image=True) is a run-time switch: blob, report and every other digest equal the recorded ones"""
    import numpy as np
    from dctfhe import models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    with open(tool.FIXTURE) as f:
        golden = {r["case"]["id"]: r for r in json.load(f)}
    for cid, kw, n, img in (("tiny-rtb6", {}, 48, 6), ("tiny-pool-rtb6", dict(pool1=(3, 2, 1)), 20, 9)):
        calib = np.random.default_rng(0).normal(0, 1, (n, 4, img, img))
        mods = [compile_brevitas_qat_model(models.tiny_resnet_q(img_size=img, **kw), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params(),
                                           configuration=cfg) for cfg in (Configuration(shard_image=True), Configuration())]
        assert mods[0].configuration.shard_image and not mods[1].configuration.shard_image
        for m in mods:
            assert tool.digests(m.compiled) == {k: golden[cid][k] for k in tool.DIGESTS}, cid
