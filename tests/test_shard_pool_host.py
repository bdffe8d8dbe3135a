"""Divided max pools, the host side: the partition rule of one pool -- the library's dctfhe_shard_pool, which needs
no GPU, against its Python mirror and against a brute-force enumeration of windows -- the plan with row ranges on the pooled tiny trunk, and
the switch.  No GPU.

Pair counts.  A window of m in-range taps costs m - 1 pairwise maxima however the tree pairs them.  The brute force enumerates, per part,
the set of row-pass results (b, c, y, xo) under the column windows of its outputs; `useful` is the cost of the distinct intermediates and
of all outputs, `halo` what intermediates claimed by more than one part cost again.  The parts' counts must sum to useful + halo exactly.
One part of one is the undivided op as it runs today, and today's row pass also computes intermediates that NO window reads (input rows
below the last window: 11 x 11 under (7, 4, 1) leaves row 10 unread); the divided rule computes only what is read, so for P >= 2 "the
total" the sum is held against is `useful`, which equals today's count wherever every row is read (all geometries here but that one)."""
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = [((3, 2, 1), 9, 9), ((3, 2, 1), 10, 7), ((2, 2, 1), 6, 6), ((7, 4, 1), 11, 11), ((3, 2, 1), 1, 5)]      # (k, s, pad), H, W
PARTS = (1, 2, 3, 5, 64)


@pytest.fixture(scope="module")
def lib_shard_pool():
    from dctfhe import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return engine.shard_pool


def _taps(n_in, k, s, pad, o):
    return [o * s - pad + j for j in range(k) if 0 <= o * s - pad + j < n_in]


class Brute:
    """every window of the pool, one output at a time"""

    def __init__(self, batch, C, H, W, k, s, pad):
        self.dims, self.geo = (batch, C, H, W), (k, s, pad)
        self.Ho, self.Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        self.outputs = list(itertools.product(range(batch * C), range(self.Ho), range(self.Wo)))      # flat [B][C][Ho][Wo] order

    def mids_of(self, out):
        bc, yo, xo = out
        return [(bc, y, xo) for y in _taps(self.dims[2], *self.geo, yo)]

    def taps_of_mid(self, mid):
        bc, y, xo = mid
        H, W = self.dims[2:]
        return [(bc * H + y) * W + x for x in _taps(W, *self.geo, xo)]

    def part(self, first, count):
        """(set of intermediates, sorted source rows read, pairs) of the outputs [first, first + count)"""
        outs = self.outputs[first:first + count]
        mids = {m for o in outs for m in self.mids_of(o)}
        rows = sorted({r for m in mids for r in self.taps_of_mid(m)})
        pairs = sum(len(self.mids_of(o)) - 1 for o in outs) + sum(len(self.taps_of_mid(m)) - 1 for m in mids)
        return mids, rows, pairs

    def undivided_pairs(self):
        """today's tree: every row-pass result of every input row, read or not"""
        B, C, H, W = self.dims
        row = sum(len(_taps(W, *self.geo, xo)) - 1 for xo in range(self.Wo))
        col = sum(len(_taps(H, *self.geo, yo)) - 1 for yo in range(self.Ho))
        return B * C * (H * row + self.Wo * col)


@pytest.mark.parametrize("geo,H,W", GEOMETRIES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("batch,C", [(1, 1), (2, 1), (1, 6), (2, 6)])
def test_shard_pool_rule(lib_shard_pool, geo, H, W, batch, C):
    from dctfhe import compile as cc
    k, s, pad = geo
    b = Brute(batch, C, H, W, k, s, pad)
    n_out, n_in = len(b.outputs), batch * C * H * W
    all_mids, _, useful = b.part(0, n_out)
    today = b.undivided_pairs()
    # today's count is the compiler's (pool_geometry: pairs per level and multiplicity, per image)
    assert today == batch * sum(mult * sum(levels) for mult, levels in cc.pool_geometry(C, H, W, k, s, pad))
    dead = today - useful
    assert dead >= 0 and (dead > 0) == ((H, W, geo) == (11, 11, (7, 4, 1)))
    for P in PARTS:
        got = [cc.shard_pool(batch, C, H, W, k, s, pad, P, p) for p in range(P)]
        assert [lib_shard_pool(batch, C, H, W, k, s, pad, P, p) for p in range(P)] == got, (P, "library against its mirror")
        # the output ranges are shard_rows' and tile the outputs exactly
        assert [g[:2] for g in got] == [cc.shard_rows(n_out, P, p) for p in range(P)]
        assert got[0][0] == 0 and got[-1][0] + got[-1][1] == n_out and all(a[0] + a[1] == c[0] for a, c in zip(got, got[1:]))
        if P == 1:
            assert got[0] == (0, n_out, 0, n_in, today)
            continue
        total, halo, claimed = 0, 0, {}
        for p, (o0, on, i0, icnt, pairs) in enumerate(got):
            mids, rows, want_pairs = b.part(o0, on)
            if on == 0:
                assert (icnt, pairs) == (0, 0), (P, p)
                continue
            # every tap of every owned window lies in the need range, and the range is the smallest that does
            assert (i0, i0 + icnt) == (rows[0], rows[-1] + 1), (P, p)
            assert 0 <= i0 and i0 + icnt <= n_in
            assert pairs == want_pairs, (P, p)
            total += pairs
            for m in mids:
                halo += (len(b.taps_of_mid(m)) - 1) if m in claimed else 0
                claimed[m] = p
        assert set(claimed) == all_mids
        assert total >= useful, P
        assert total == useful + halo, P      # an equality against the enumeration: nothing but the halo is computed twice
        if dead == 0:
            assert total >= today
    if n_out < 64:
        assert any(g[1] == 0 for g in [cc.shard_pool(batch, C, H, W, k, s, pad, 64, p) for p in range(64)])


def test_shard_pool_single_tap_and_levels():
    """what the geometries are there for: (2, 2, 1) on 6 x 6 has single-tap windows, (7, 4, 1) on 11 x 11 three levels"""
    from dctfhe import compile as cc
    assert 1 in cc.pool_taps(6, 2, 2, 1) and 2 in cc.pool_taps(6, 2, 2, 1)
    assert len(cc.pool_level_pairs(cc.pool_taps(11, 7, 4, 1))) == 3
    assert set(cc.pool_taps(9, 3, 2, 1)) == {2, 3} and cc.pool_taps(9, 3, 2, 1)[0] == cc.pool_taps(9, 3, 2, 1)[-1] == 2


@pytest.mark.parametrize("args", [(1, 1, 9, 9, 3, 2, 1, 0, 0), (1, 1, 9, 9, 3, 2, 1, 65, 0), (1, 1, 9, 9, 3, 2, 1, 2, 2), (1, 1, 9, 9, 3, 2, 1, 2, -1)])
def test_shard_pool_refusals(lib_shard_pool, args):
    from dctfhe import compile as cc
    from dctfhe._lib import DctfheError
    with pytest.raises(ValueError):
        cc.shard_pool(*args)
    with pytest.raises(DctfheError, match="dctfhe_shard_rows"):
        lib_shard_pool(*args)


def test_shard_pool_refuses_bad_geometry(lib_shard_pool):
    from dctfhe._lib import DctfheError
    for bad in ((1, 1, 9, 9, 3, 2, 2, 2, 0), (1, 1, 9, 9, 0, 2, 0, 2, 0), (1, 1, 1, 1, 5, 1, 1, 2, 0), (0, 1, 9, 9, 3, 2, 1, 2, 0)):
        with pytest.raises(DctfheError, match="dctfhe_shard_pool: bad geometry"):
            lib_shard_pool(*bad)


@pytest.fixture(scope="module")
def pooled():
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (20, 4, 9, 9))
    return compile_brevitas_qat_model(models.tiny_resnet_q(img_size=9, pool1=(3, 2, 1)), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params()).compiled


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("parts", [2, 3, 5])
def test_ranged_plan_pooled_trunk(pooled, parts, batch):
    from dctfhe import compile as cc
    c = pooled
    plain = c.shard_plan()
    (pool_i, pool), = [(i, o) for i, o in enumerate(c.ops) if o.type == cc.OP_MAXPOOL]
    src = c.tensors[pool.src0]
    for part in range(parts):
        ranged = c.shard_plan(rows=True, part=part, parts=parts, batch=batch)
        assert [(a, t) for a, t, _, _ in ranged] == plain      # the same entries as shard_plan()
        for a, t, first, count in ranged:
            T = c.tensors[t]
            if t == pool.src0:
                assert a < pool_i
                assert (first, count) == cc.shard_pool(batch, src.C, src.H, src.W, pool.pool.k, pool.pool.stride, pool.pool.pad, parts, part)[2:4]
                assert count < batch * T.C * T.H * T.W      # 9 x 9 in parts: no part needs the whole stem tensor
            else:
                assert (first, count) == (0, batch * T.C * T.H * T.W)
    # rows=True for one part of one: every entry whole
    assert all((f, n) == (0, c.tensors[t].C * c.tensors[t].H * c.tensors[t].W) for _, t, f, n in c.shard_plan(rows=True))


def test_needed_from_is_the_overlap_with_other_owners():
    """the ranged exchange: a rank receives exactly its need range less its own rows, from the ranks that own them"""
    from dctfhe import compile as cc, sharding
    for parts in (2, 3, 5):
        rows = 4 * 9 * 9
        own = [cc.shard_rows(rows, parts, p) for p in range(parts)]
        need = [cc.shard_pool(1, 4, 9, 9, 3, 2, 1, parts, p)[2:4] for p in range(parts)]
        for q in range(parts):
            got = set()
            for p, first, count in sharding.needed_from(own, need, q):
                assert p != q and count > 0 and own[p][0] <= first and first + count <= own[p][0] + own[p][1]
                got |= set(range(first, first + count))
            want = set(range(need[q][0], need[q][0] + need[q][1])) - set(range(own[q][0], own[q][0] + own[q][1]))
            assert got == want


def test_configuration_switch():
    from dctfhe.quantized_module import Configuration
    with pytest.raises(ValueError, match="shard_image"):
        Configuration(shard_pool=True)
    cfg = Configuration(shard_image=True, shard_pool=True)
    assert cfg.shard_image and cfg.shard_pool
    assert not Configuration(shard_image=True).shard_pool and not Configuration().shard_pool


def test_new_symbols_declared_and_bound(lib_shard_pool):
    from dctfhe import _lib
    hdr = open(os.path.join(ROOT, "include", "dctfhe.h")).read()
    declared = set(re.findall(r"\b(dctfhe_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.load()
    for name in ("dctfhe_shard_pool", "dctfhe_session_set_shard_pool", "dctfhe_session_mark_rows", "dctfhe_session_shard_plan_rows",
                 "dctfhe_session_pool_pairs"):
        assert name in declared and name in _lib.EXPORTS and getattr(L, name).argtypes, name


def test_cli_flag():
    src = open(os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py")).read()
    assert '"--shard_pool"' in src and "shard_pool=params.shard_pool" in src


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exchange_worker(rank, world, port, own, need, out_dir):
    import sys
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "dct-cryptonets_amd"))
    from dctfhe.sharding import exchange_need_rows
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rows = sum(n for _, n in own)
    t = torch.full((rows, 3), -1, dtype=torch.int64)      # a rank holds its own rows (row r = r, r + 1000, r + 2000); -1: not here
    f, n = own[rank]
    t[f:f + n] = torch.arange(f, f + n)[:, None] + torch.tensor([0, 1000, 2000])
    got = exchange_need_rows(t, own, need, world)
    torch.save({"t": t, "bytes": got}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_need_rows_on_gloo(tmp_path):
    """three gloo ranks on the CPU: each ends with its own rows and the rows of its need range that the others own -- nothing else --
    and counts the bytes it received; uneven ranges, a need range inside one's own rows, and a rank that needs nothing"""
    import torch
    import torch.multiprocessing as mp
    own = [(0, 7), (7, 6), (13, 6)]
    need = [(0, 9), (9, 2), (0, 0)]      # rank 0: two rows of rank 1's; rank 1: within its own; rank 2: an empty part of the pool
    mp.spawn(_exchange_worker, args=(3, _free_port(), own, need, str(tmp_path)), nprocs=3, join=True)
    for rank in range(3):
        got = torch.load(str(tmp_path / f"rank{rank}.pt"), weights_only=True)
        held = set(range(own[rank][0], sum(own[rank]))) | set(range(need[rank][0], sum(need[rank])))
        for r in range(19):
            want = [r, r + 1000, r + 2000] if r in held else [-1, -1, -1]
            assert got["t"][r].tolist() == want, (rank, r)
        assert got["bytes"] == 8 * 3 * len(held - set(range(own[rank][0], sum(own[rank])))), rank
