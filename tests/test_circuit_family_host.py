"""The circuit family (tests/circuit_family.py) on the host, no GPU: every case compiles deterministically to a blob the library accepts
and the oracle parses; the numpy interpreter reproduces the compile-time outputs element for element and takes the fresh inputs without
overflow; the modelled failure rate allows a bit-for-bit comparison; the run can be divided (shard plans, a memory plan under a budget)
or is refused with the documented message; and the list covers the topology features it is there for -- read off the COMPILED ops and
tensors, not off the case names."""
import os

import numpy as np
import pytest

import circuit_family as F

OP_CONV, OP_ADD, OP_SUMPOOL, OP_LUT, OP_MAXPOOL = 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def L():
    from dctfhe import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize("name", F.NAMES)
def test_compiles_twice_to_one_blob_the_library_accepts(L, name):
    from dctfhe import compile as cc
    from oracle import circuit_ref
    case, c = F.BY_NAME[name], F.compiled(name)
    again = cc.compile_model(case.model(), case.calib(), **case.compile_kw())
    assert again.blob == c.blob and np.array_equal(again.calib_out, c.calib_out)
    assert L.dctfhe_circuit_validate(c.blob, len(c.blob)) == 0, L.dctfhe_last_error().decode()
    parsed = circuit_ref.parse_blob(c.blob)
    assert len(parsed["ops"]) == len(c.ops) and len(parsed["tensors"]) == len(c.tensors)
    assert (parsed["input"], parsed["output"]) == (c.input_tensor, c.output_tensor)
    for po, o in zip(parsed["ops"], c.ops):
        assert po["type"] == o.type and po["dst"] == o.dst and list(po["ip"]) == [int(x) for x in o.ip]
    assert [tuple(t) for t in parsed["tensors"]] == [(t.C, t.H, t.W) for t in c.tensors]


@pytest.mark.parametrize("name", F.NAMES)
def test_interpreter_equals_the_compile_time_outputs(name):
    """the calibration batch through the numpy interpreter: no overflow, and calib_out element for element"""
    c = F.compiled(name)
    vals, overflow = F.interpreter(name, "calib")
    assert not overflow
    assert vals.shape == c.calib_out.shape == (F.N_CALIB, c.n_out())
    assert np.array_equal(vals, c.calib_out), np.argwhere(vals != c.calib_out)[:5]
    lo, hi = -(1 << (c.out_bits - 1)), (1 << (c.out_bits - 1)) - 1
    assert vals.min() >= lo and vals.max() <= hi and len(np.unique(vals)) > 3


@pytest.mark.parametrize("name", F.NAMES)
def test_fresh_inputs_stay_inside_every_table(name):
    """the rows a case names as fresh are not calibration rows, differ from one another, and the integer circuit takes them without
    leaving a padded range: the device is compared with the interpreter on exactly these"""
    case, c = F.BY_NAME[name], F.compiled(name)
    assert len(set(case.fresh)) == F.BATCH and min(case.fresh) >= F.N_CALIB
    vals, overflow = F.interpreter(name, "fresh")
    assert not overflow and vals.shape == (F.BATCH, c.n_out())
    q, _ = F.quantise(c, case.fresh_inputs())
    assert len({x.tobytes() for x in q}) == F.BATCH
    assert len(np.unique(vals)) > 2                                # not a constant output: a wrong layout would show


@pytest.mark.parametrize("name", F.NAMES)
def test_failure_bound_allows_a_bit_exact_comparison(name):
    case, c = F.BY_NAME[name], F.compiled(name)
    print(f"{name}: {len(c.ops)} ops, {sum(c.pbs_counts().values())} bootstraps / image {c.pbs_counts()}, expected failures / image "
          f"{c.expected_failures_per_image:.2e}, boundary flips / image {c.expected_boundary_flips_per_image:.2e}")
    assert c.rounding_method == ("exact" if case.exact else "approximate")
    if case.exact:
        assert c.expected_failures_per_image * F.BATCH <= F.BOUND, c.expected_failures_per_image
        assert c.expected_boundary_flips_per_image == 0.0
    else:
        assert c.expected_boundary_flips_per_image > 0.0


def _check_shard_plan(c):
    """the exchange plan against its definition: every sliced tensor a whole-reading op (or the download) reads travels once, right
    after the op that writes it; a tensor that element-wise ops alone read never travels"""
    plan = c.shard_plan()
    writer = {o.dst: i for i, o in enumerate(c.ops)}
    sliced = {o.dst for o in c.ops if o.type in (OP_LUT, OP_ADD)}
    read_whole = {o.src0 for o in c.ops if o.type in (OP_CONV, OP_SUMPOOL, OP_MAXPOOL)} | {c.output_tensor}
    assert sorted(t for _, t in plan) == sorted(read_whole & sliced)
    assert [a for a, _ in plan] == sorted(a for a, _ in plan) and all(a == writer[t] for a, t in plan)
    return plan


@pytest.mark.parametrize("name", F.NAMES)
def test_shard_plans_for_two_and_three_parts(name):
    from dctfhe import compile as cc
    c = F.compiled(name)
    plan = _check_shard_plan(c)
    assert plan and plan[-1] == (len(c.ops) - 1, c.output_tensor)
    pools = {o.src0: o for o in c.ops if o.type == OP_MAXPOOL}
    for parts in (2, 3):
        seen = {}
        for part in range(parts):
            rows = c.shard_plan(rows=True, part=part, parts=parts, batch=F.BATCH)
            assert [(a, t) for a, t, _, _ in rows] == plan                     # dividing the pools moves no exchange point here
            for a, t, first, count in rows:
                T = c.tensors[t]
                total = F.BATCH * T.C * T.H * T.W
                assert 0 <= first and first + count <= total
                if t in pools:      # a divided pool's source: the part's need range, by the rule
                    S = pools[t].pool
                    assert (first, count) == cc.shard_pool(F.BATCH, T.C, T.H, T.W, S.k, S.stride, S.pad, parts, part)[2:4]
                    seen.setdefault(t, []).append((first, count))
                else:
                    assert (first, count) == (0, total)
        for t, ranges in seen.items():      # between them the parts read every row a window reads: at most a dropped border is left out
            T = c.tensors[t]
            covered = np.zeros(F.BATCH * T.C * T.H * T.W, bool)
            for first, count in ranges:
                covered[first:first + count] = True
            S = pools[t].pool
            read = np.zeros((T.H, T.W), bool)
            for yo in range((T.H + 2 * S.pad - S.k) // S.stride + 1):
                for xo in range((T.W + 2 * S.pad - S.k) // S.stride + 1):
                    y0, x0 = max(0, yo * S.stride - S.pad), max(0, xo * S.stride - S.pad)
                    read[y0:yo * S.stride - S.pad + S.k, x0:xo * S.stride - S.pad + S.k] = True
            assert covered.reshape(-1, T.H, T.W)[:, read].all()


REFUSAL = "memory budget of %d bytes: the smallest plan"
# the cases whose session no budget under the undivided plan fits, by kind of session (True: encrypted)
UNDIVIDABLE = {True: ("three-stage", "rtb5-n4-bw3"),
               False: ("signed-stem-s2", "three-stage", "pool311", "rtb5-n4-bw3")}


@pytest.mark.parametrize("name", F.NAMES)
@pytest.mark.parametrize("encrypted", [True, False], ids=["encrypted", "clear"])
def test_memory_plan_under_a_budget_or_the_documented_refusal(L, name, encrypted):
    from dctfhe._lib import DctfheError
    c = F.compiled(name)
    params = None if encrypted else False
    free = c.memory_plan(params=params, batch=F.BATCH)
    assert free["bytes_planned"] == free["bytes_undivided"] > 0 and all(g["slab"] == g["channels"] for g in free["groups"])
    convs = [i for i, o in enumerate(c.ops) if o.type == OP_CONV]
    assert free["groups"] and all(g["first_op"] in convs and g["channels"] == c.ops[g["first_op"]].conv.Cout for g in free["groups"])
    budget = free["bytes_undivided"] - 1
    try:
        m = c.memory_plan(params=params, batch=F.BATCH, budget_bytes=budget)
    except DctfheError as e:
        # no cut lowers the session's bytes (a later tensor is as large as the stem's and reuses its buffers): refused by the message;
        # the device test runs such a case in slabs at heights set by hand
        assert REFUSAL % budget in str(e), str(e)
        assert name in UNDIVIDABLE[encrypted], name
        return
    assert name not in UNDIVIDABLE[encrypted], name
    assert m["bytes_planned"] <= budget and m["bytes_undivided"] == free["bytes_undivided"]
    assert m["bytes_planned"] == m["bytes_buffers"] + m["bytes_maps"] + m["bytes_scratch"]
    assert [(g["first_op"], g["end_op"], g["channels"]) for g in m["groups"]] == [(g["first_op"], g["end_op"], g["channels"]) for g in free["groups"]]
    assert all(1 <= g["slab"] <= g["channels"] for g in m["groups"]) and any(g["slab"] < g["channels"] for g in m["groups"])


# ------------------------------------------------------------------------------------------ what the list is there for
# tests/test_gpu_circuit_family.py takes every case through every path; these are the kinds of case each path must find on the list
DIVIDED = ("three-stage", "stem5-pool220", "signed-stem-s2")      # sharded and in slabs: three stages, a pooled one, a parity-split one
TWICE = ("pool311", "zero-blocks")                                # twice on one upload: a pooled one, the one without blocks
PACKED = ("zero-blocks", "three-stage")                           # packed and ring-packed: more than one ring of results, and less


def _features(c):
    """what a compiled circuit shows of its topology, from ops and tensors alone"""
    from dctfhe import compile as cc
    T, ops = c.tensors, c.ops
    convs = [o for o in ops if o.type == OP_CONV]
    luts = [o for o in ops if o.type == OP_LUT]
    adds = [o for o in ops if o.type == OP_ADD]
    pools = [o for o in ops if o.type == OP_MAXPOOL]
    (sump,) = [o for o in ops if o.type == OP_SUMPOOL]
    writer = {o.dst: o for o in ops}
    stem = ops[0]
    assert stem.type == OP_CONV and stem.src0 == c.input_tensor and ops[1].type == OP_LUT and ops[1].src0 == stem.dst
    f = dict(stem_k=stem.conv.KH, stem_stride=stem.conv.stride, stem_pad=stem.conv.pad, stem_in=T[stem.src0].H,
             stem_signed_table=bool(ops[1].table_values.min() < 0), in_ch=T[c.input_tensor].C,
             pool=(pools[0].pool.k, pools[0].pool.stride, pools[0].pool.pad) if pools else None, pool_in=T[pools[0].src0].H if pools else None,
             blocks=len(adds), channels={T[o.src0].C for o in convs} | {o.conv.Cout for o in convs})
    # per block, in order: the stride of its first 3x3 convolution, and its shortcut -- "identity" (a look-up that reads what the block's
    # first convolution reads) or the (kernel, stride, input size) of the convolution behind the add's second operand
    blocks = []
    for a in adds:
        v = writer[a.src1]
        assert v.type == OP_LUT
        feeder = writer.get(v.src0)
        if feeder is not None and feeder.type == OP_CONV and feeder.conv.KH == 1 and (feeder is not stem):
            sc = ("conv1x1", feeder.conv.stride, T[feeder.src0].H)
            block_in = feeder.src0
        else:
            sc, block_in = "identity", v.src0
        first = [o for o in convs if o.src0 == block_in and o.conv.KH == 3]
        assert len(first) == 1
        blocks.append((first[0].conv.stride, sc))
    f["block_strides"] = [b[0] for b in blocks]
    f["shortcuts"] = [b[1] for b in blocks]
    s = T[sump.src0]
    f["sum_k"], f["sum_in"], f["sum_out"] = sump.sum_k, s.H, T[sump.dst].H
    f["modes"] = {o.lut.mode for o in luts}
    f["max_w"] = max(o.lut.w for o in luts)
    f["rounds"] = any(o.lut.r > 0 for o in luts)
    return f


def test_the_list_covers_the_features_it_is_there_for():
    from dctfhe import compile as cc
    cs = {n: F.compiled(n) for n in F.NAMES}
    fs = {n: _features(c) for n, c in cs.items()}
    every = list(fs.values())
    assert 8 <= len(every) <= 12
    for n, c in cs.items():
        ps = c.param_set
        assert (ps.D, [(t.name, t.k, t.N) for t in ps.tiers]) == (1024, [("t", 1, 1024), ("b", 2, 256)]), n
    # stem
    assert {3, 5, 7} <= {f["stem_k"] for f in every}
    assert any(f["stem_stride"] == 2 and f["stem_pad"] > 0 and f["stem_in"] % 2 == 1 for f in every)
    assert any(f["stem_signed_table"] for f in every) and any(not f["stem_signed_table"] for f in every)
    assert all(f["pool"] is None for f in every if f["stem_signed_table"])
    # stem max pool; (3, 2, 1) on an input size no other test of the suite pools (9 x 9 and 7 x 6 there)
    assert {None, (2, 2, 0), (3, 1, 1), (3, 2, 1)} <= {f["pool"] for f in every}
    assert any(f["pool"] == (3, 2, 1) and f["pool_in"] not in (6, 7, 9) for f in every)
    # blocks
    assert {0, 1, 3} <= {f["blocks"] for f in every}
    assert any(f["blocks"] == 3 and f["block_strides"].count(2) == 2 for f in every)
    assert any(f["blocks"] and f["block_strides"][0] == 2 for f in every)
    assert any("identity" in f["shortcuts"] and any(s != "identity" for s in f["shortcuts"]) for f in every)
    strided = [s for f in every for s in f["shortcuts"] if s != "identity" and s[1] == 2]
    assert any(s[2] % 2 == 0 for s in strided) and any(s[2] % 2 == 1 for s in strided)
    # final sum pool
    assert any(f["sum_k"] == 1 for f in every)
    assert any(f["sum_k"] == f["sum_in"] > 1 for f in every)
    assert any(f["sum_in"] % f["sum_k"] and f["sum_out"] * f["sum_k"] < f["sum_in"] for f in every)
    assert any(f["sum_out"] >= 2 for f in every)
    assert any(c.n_out() > c.tensors[c.output_tensor].C for c in cs.values())
    # rounding
    assert {5, 6, 7} <= {c.rounding_threshold_bits for c in cs.values()}
    for c, f in zip(cs.values(), every):
        assert f["max_w"] <= c.rounding_threshold_bits and (cc.LUT_SPLIT in f["modes"]) == (f["max_w"] == 7)
    assert any(f["max_w"] == 7 for f in every) and any(f["max_w"] == 5 for f in every)
    approx = [n for n, c in cs.items() if c.rounding_method == "approximate"]
    assert len(approx) == 1 and cc.LUT_APPROX in fs[approx[0]]["modes"] and set(cs[approx[0]].pbs_counts()) == {"t"}
    assert all(f["rounds"] for f in every)
    assert {4, 5} <= {c.n_bits for c in cs.values()} and {3, 4} <= {c.in_bits for c in cs.values()}
    # channel counts
    assert any(f["in_ch"] == 1 for f in every)
    assert any(o.type == OP_CONV and max(o.conv.Cout, c.tensors[o.src0].C) > 16 and (o.conv.KH == 1 or i == 0)
               for c in cs.values() for i, o in enumerate(c.ops))
    # one parity-split site takes more bootstraps per batch than the session's look-up scratch holds, and not a multiple of it; every
    # other case stays under it (so the chunk loop's first and later passes are both compared)
    sites = {n: max(F.BATCH * c.tensors[o.src0].C * c.tensors[o.src0].H * c.tensors[o.src0].W for o in c.ops if o.type == OP_LUT) for n, c in cs.items()}
    chunked = [n for n, m in sites.items() if m > F.SCRATCH_CHUNK]
    assert len(chunked) == 1 and sites[chunked[0]] % F.SCRATCH_CHUNK and cc.LUT_SPLIT in fs[chunked[0]]["modes"]
    # the cases the device tests single out hold what they are singled out for
    assert fs[DIVIDED[0]]["blocks"] == 3 and fs[DIVIDED[1]]["pool"] is not None and cc.LUT_SPLIT in fs[DIVIDED[2]]["modes"]
    assert fs[TWICE[0]]["pool"] is not None and fs[TWICE[1]]["blocks"] == 0
    # packed results stay inside the budget on both forms, and one of the two fills more than one ring of the test spec
    from dctfhe import params as P
    spec = P.test_pack_spec()
    for n in cs:
        assert cc.output_compaction(cs[n]).pfail <= 1e-12 and cc.output_compaction(cs[n], "ring", spec).pfail <= 1e-12
    assert any(spec.N < F.BATCH * cs[n].n_out() < 2 * spec.N for n in PACKED) and any(F.BATCH * cs[n].n_out() < spec.N for n in PACKED)
