"""The session planner on the host (include/dctfhe.h dctfhe_memory_plan): no context, no GPU.  Slab groups of the
tiny trunks (a convolution and the look-ups / max pools behind it; an add, a second reader or the circuit output ends a group), the
undivided plan with no budget and with a roomy one, a descent of budgets (every plan fits its budget, heights only go down), determinism,
and the refusal below the smallest plan.  Planned bytes are NOT monotone in the slab height in general (the trunk without a pool shows
it).  The full-size trunks (3x448^2, 3x1024^2) are left to tools/memory_plan.py: compiling them does not fit a host test."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OP_CONV, OP_ADD, OP_SUMPOOL, OP_LUT, OP_MAXPOOL = 1, 2, 3, 4, 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    from dctfhe import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _compiled(pool, img, rtb=6):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(3).normal(0, 1, (20, 4, img, img))
    return compile_brevitas_qat_model(models.tiny_resnet_q(img_size=img, pool1=pool), calib, n_bits=5, rounding_threshold_bits=rtb,
                                      param_set=P.test_params()).compiled


@pytest.fixture(scope="module")
def plain():
    return _compiled(None, 6)


@pytest.fixture(scope="module")
def pooled():
    return _compiled((3, 2, 1), 9)


def _groups_by_definition(cc):
    """the group rule restated on the compiled ops: conv, then LUT / MAXPOOL ops that read exactly the previous destination, which
    nothing else reads (the circuit output counts as a reader)"""
    readers = {}
    for o in cc.ops:
        readers[o.src0] = readers.get(o.src0, 0) + 1
        if o.type == OP_ADD:
            readers[o.src1] = readers.get(o.src1, 0) + 1
    readers[cc.output_tensor] = readers.get(cc.output_tensor, 0) + 1
    out, i = [], 0
    while i < len(cc.ops):
        if cc.ops[i].type != OP_CONV:
            i += 1
            continue
        j = i + 1
        while j < len(cc.ops) and cc.ops[j].type in (OP_LUT, OP_MAXPOOL) and cc.ops[j].src0 == cc.ops[j - 1].dst and readers[cc.ops[j - 1].dst] == 1:
            j += 1
        if j - i >= 2:
            out.append((i, j, cc.ops[i].conv.Cout))
        i = j
    return out


@pytest.mark.parametrize("which", ["plain", "pooled"])
def test_groups_follow_the_rule(request, which):
    cc = request.getfixturevalue(which)
    m = cc.memory_plan(batch=2)
    got = [(g["first_op"], g["end_op"], g["channels"]) for g in m["groups"]]
    assert got == _groups_by_definition(cc) and got
    assert all(g["slab"] == g["channels"] for g in m["groups"])
    types = [o.type for o in cc.ops]
    for first, end, _ in got:
        assert types[first] == OP_CONV and all(t in (OP_LUT, OP_MAXPOOL) for t in types[first + 1:end])
    # the stem: conv -> look-up (-> max pool -> look-up on the pooled trunk) is one group from op 0, 6 channels
    assert got[0][0] == 0 and got[0][2] == 6
    if which == "pooled":
        assert OP_MAXPOOL in types[got[0][0]:got[0][1]]
    # the residual block: an ADD reads the look-up behind a block's second convolution together with the shortcut, so no group holds an
    # ADD, and the tensor an ADD reads is never inside a group (it is a group's LAST destination, written whole, or no group's at all)
    inner = {cc.ops[i].dst for first, end, _ in got for i in range(first, end - 1)}
    adds = [o for o in cc.ops if o.type == OP_ADD]
    assert adds and all(o.src0 not in inner and o.src1 not in inner for o in adds)
    assert cc.output_tensor not in inner


def test_no_budget_and_a_roomy_budget_give_the_undivided_plan(pooled):
    free = pooled.memory_plan(batch=2)
    assert free["bytes_planned"] == free["bytes_undivided"] > 0 and free["budget_bytes"] == 0
    assert free["bytes_planned"] == free["bytes_buffers"] + free["bytes_maps"] + free["bytes_scratch"]
    for budget in (free["bytes_undivided"], free["bytes_undivided"] + 1, 10 * free["bytes_undivided"]):
        m = pooled.memory_plan(batch=2, budget_bytes=budget)
        assert m["groups"] == free["groups"] and m["bytes_planned"] == free["bytes_undivided"] and m["budget_bytes"] == budget


def test_descent_of_budgets_each_plan_fits_and_heights_only_go_down(pooled):
    from dctfhe._lib import DctfheError
    free = pooled.memory_plan(batch=2)
    seen, budget = [free], free["bytes_undivided"] - 1
    for _ in range(64):      # walk down: every plan's bytes minus one is the next budget
        try:
            m = pooled.memory_plan(batch=2, budget_bytes=budget)
        except DctfheError as e:
            last_error = str(e)
            break
        assert m["bytes_planned"] <= budget and m["bytes_undivided"] == free["bytes_undivided"]
        assert all(1 <= g["slab"] <= g["channels"] for g in m["groups"])
        # a tighter budget never raises a height (the descent is one path), and the breakdown adds up
        assert all(a["slab"] >= b["slab"] for a, b in zip(seen[-1]["groups"], m["groups"]))
        assert m["bytes_planned"] == m["bytes_buffers"] + m["bytes_maps"] + m["bytes_scratch"]
        seen.append(m)
        budget = m["bytes_planned"] - 1
    else:
        raise AssertionError("the planner never refused")
    assert len(seen) >= 3
    # the refusal names an op and the bytes of the smallest plan
    m = re.search(r"memory budget of (\d+) bytes: the smallest plan .* needs (\d+) bytes; .* destination of op (\d+)", last_error)
    assert m, last_error
    assert int(m.group(1)) == budget and int(m.group(2)) == seen[-1]["bytes_planned"] and 0 <= int(m.group(3)) < len(pooled.ops)
    # the first cut lands in the group that holds the largest inner tensor: the stem
    first_cut = seen[1]["groups"]
    assert first_cut[0]["slab"] < first_cut[0]["channels"]


def test_twice_the_same_record_and_clear_mode(pooled):
    a = pooled.memory_plan(batch=2)
    assert a == pooled.memory_plan(batch=2)
    under = pooled.memory_plan(batch=2, budget_bytes=a["bytes_undivided"] - 1)
    assert under == pooled.memory_plan(batch=2, budget_bytes=a["bytes_undivided"] - 1)
    assert under["bytes_planned"] < a["bytes_undivided"]
    clear = pooled.memory_plan(params=False, batch=2)       # one word per element, no scratch, no maps
    assert clear["groups"] == a["groups"] and 0 < clear["bytes_planned"] < a["bytes_planned"] and clear["bytes_maps"] == 0
    assert pooled.memory_plan(batch=4)["bytes_planned"] > a["bytes_planned"]


def test_a_trunk_whose_stem_is_not_its_largest_need_is_refused_not_divided_in_vain(plain):
    """the 6 x 6 trunk without a pool: its first block holds tensors as large as the stem's, and the buffers the stem frees are reused
    there, so no cut lowers the sum of the session's allocations -- the planner says so instead of returning a plan over the budget"""
    from dctfhe._lib import DctfheError
    a = plain.memory_plan(batch=2)
    with pytest.raises(DctfheError, match=r"memory budget of %d bytes: the smallest plan" % (a["bytes_undivided"] - 1)):
        plain.memory_plan(batch=2, budget_bytes=a["bytes_undivided"] - 1)


def test_refusals(plain):
    from dctfhe import engine
    from dctfhe._lib import DctfheError
    with pytest.raises(DctfheError, match="batch must be >= 1"):
        engine.memory_plan(plain.blob, None, 0)
    with pytest.raises(DctfheError, match="circuit blob"):
        engine.memory_plan(plain.blob[:10], None, 1)
    with pytest.raises(DctfheError, match="memory budget of 1 bytes"):
        plain.memory_plan(batch=1, budget_bytes=1)


def test_report_prints_the_plan_only_under_a_budget(plain):
    assert "device memory budget" not in plain.report()
    free = plain.memory_plan()
    text = plain.report(memory_budget_bytes=free["bytes_undivided"])
    assert "device memory budget" in text and "slab group ops [0," in text


def test_configuration_option():
    from dctfhe.quantized_module import Configuration
    assert Configuration().device_memory_budget_gb is None and Configuration().device_memory_budget_bytes is None
    assert Configuration(device_memory_budget_gb=1.5).device_memory_budget_bytes == 1_500_000_000
    with pytest.raises(ValueError, match="exclude each other"):
        Configuration(device_memory_budget_gb=1, shard_image=True)
    with pytest.raises(ValueError, match="positive"):
        Configuration(device_memory_budget_gb=0)
