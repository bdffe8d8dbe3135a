"""Image sharding for multi-GPU evaluation.

Each image is an independent circuit evaluation under the same keys (the reference loops samples one at a
time inside forward(), homomorphic_eval.py:70), so a batch shards by image: rank r of G takes images
r, r+G, r+2G, ...  Keys and circuit are regenerated per rank from the seed; the only exchange on the data
path is one all_gather of the decrypted-side logits (RCCL on GPUs, gloo in the CPU tests).

Sharding ONE image: the look-up sites of an image are element-wise, so `parts` sessions each evaluate their rows of
every look-up and add (dctfhe.engine.Session.set_shard) and exchange rows only where a convolution, a pool or the download reads a whole
tensor (CompiledCircuit.shard_plan).  exchange_rows is that exchange, broadcast_bytes ships rank 0's input blob, run_sharded walks the plan.
With the max pools divided too (Configuration(shard_pool=True)) run_sharded_rows walks the plan with row ranges:
exchange_need_rows sends a rank only the rows of its need range that other ranks own.

Every collective bench.py issues lives here, so that the CPU tests (gloo, world size 2) and the one-rank RCCL smoke test
(tests/test_gpu_rccl_smoke.py: `nccl` backend on cuda:0) run the very calls the 8-GPU job makes."""
import torch
import torch.distributed as dist


def shard_indices(n_images, rank, world):
    return list(range(rank, n_images, world))


def gather_in_image_order(local, world):
    """local: [B_local, F] tensor, same B_local on every rank -> [B_local*world, F] in global image order"""
    if world == 1 and not (dist.is_available() and dist.is_initialized()):
        return local
    parts = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(parts, local.contiguous())
    return torch.stack(parts, dim=1).reshape(local.shape[0] * world, *local.shape[1:])


def _live(world):
    return world > 1 or (dist.is_available() and dist.is_initialized())


def broadcast_seed(seed32, world, dev):
    """rank 0's 32 key-seed bytes to every rank (keys are regenerated from them on each GPU: no key traffic)"""
    t = torch.tensor(list(seed32), dtype=torch.uint8)
    if _live(world):
        t = t.to(dev)
        dist.broadcast(t, 0)
        t = t.cpu()
    return bytes(t.tolist())


def agree_min(values, world, dev):
    """element-wise minimum over ranks of a list of ints (the pass plan every rank must share)"""
    if not _live(world):
        return [int(v) for v in values]
    t = torch.tensor([int(v) for v in values], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return [int(v) for v in t.tolist()]


def max_over_ranks(x, world, dev):
    """the slowest rank's elapsed time"""
    if not _live(world):
        return float(x)
    t = torch.tensor([float(x)], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def all_true(flag, world, dev):
    if not _live(world):
        return bool(flag)
    t = torch.tensor([1.0 if flag else 0.0], device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item() > 0.5)


def barrier(world):
    if _live(world):
        dist.barrier()


def _collective_device(dev):
    """where a collective's tensors live: the GPU under RCCL, host memory under gloo"""
    return torch.device("cpu") if dist.get_backend() == "gloo" else dev


def broadcast_bytes(data, world, dev, src=0):
    """rank `src`'s bytes to every rank (the seeded or public-key input blob of a sharded image: kilobytes, never the rows)"""
    if not _live(world):
        return bytes(data)
    cdev = _collective_device(dev)
    mine = dist.get_rank() == src
    n = torch.tensor([len(data) if mine else 0], dtype=torch.int64, device=cdev)
    dist.broadcast(n, src)
    if mine:
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cdev)
    else:
        t = torch.empty(int(n.item()), dtype=torch.uint8, device=cdev)
    dist.broadcast(t, src)
    return bytes(t.cpu().numpy().tobytes())


class _DeviceRows:
    """rows of 64-bit words in device memory, as torch.as_tensor reads them without a copy"""

    def __init__(self, dev_ptr, rows, row_words):
        self.__cuda_array_interface__ = dict(shape=(int(rows), int(row_words)), typestr="<i8", data=(int(dev_ptr), False), version=2, strides=None)


def tensor_view(session, tensor, dev):
    """a session's tensor [rows, row_words] as an int64 torch tensor on `dev` over the session's own memory (Session.tensor)"""
    dev_ptr, row_words, rows = session.tensor(tensor)
    return torch.as_tensor(_DeviceRows(dev_ptr, rows, row_words), device=dev)


def exchange_rows(tensor_view, ranges, world):
    """Every part's rows of one tensor into every rank's copy: one broadcast per part of that part's row range ranges[p] = (first, count),
    straight from and into `tensor_view` (rows are contiguous).  Uneven ranges need no padding and an empty one no call; under gloo the
    rows are staged through host memory.  Returns the bytes this rank sent or received.  The engine's run is synchronous, so the rows are
    there when this is called; it returns once they are in place."""
    if len(ranges) != world:
        raise ValueError(f"exchange_rows: {len(ranges)} row ranges for {world} ranks")
    if not _live(world):
        return 0
    rank, staged, moved = dist.get_rank(), dist.get_backend() == "gloo", 0
    for p, (first, count) in enumerate(ranges):
        if count == 0:
            continue
        rows = tensor_view[first:first + count]
        if staged:
            buf = rows.cpu() if rank == p else torch.empty(rows.shape, dtype=rows.dtype)
            dist.broadcast(buf, p)
            if rank != p:
                rows.copy_(buf)
        else:
            dist.broadcast(rows, p)
        if world > 1:
            moved += rows.numel() * 8
    if tensor_view.is_cuda:
        torch.cuda.synchronize(tensor_view.device)
    return moved


def run_sharded(session, plan, n_ops, shard_rows, world, dev, timing=False):
    """A sharded session's pass over the circuit: run_span up to each exchange point of `plan` [(after_op, tensor)], exchange_rows,
    mark_whole; then the rest.  -> (timings of the spans, bytes exchanged)"""
    timings, moved, first = [], 0, 0
    for after_op, tensor in plan:
        if after_op + 1 > first:
            timings.append(session.run_span(first, after_op + 1, timing))
            first = after_op + 1
        view = tensor_view(session, tensor, dev)
        moved += exchange_rows(view, [shard_rows(view.shape[0], world, p) for p in range(world)], world)
        session.mark_whole(tensor)
    if first < n_ops:
        timings.append(session.run_span(first, n_ops, timing))
    return timings, moved


def _overlap(a, b):
    """(first, count) of the rows two ranges (first, count) share"""
    lo, hi = max(a[0], b[0]), min(a[0] + a[1], b[0] + b[1])
    return (lo, hi - lo) if hi > lo else (lo, 0)


def needed_from(own, need, rank):
    """what `rank` receives at a ranged exchange point: [(source rank, first, count)], the rows of its need range that other ranks own.
    own[p], need[p]: the (first, count) part p wrote and part p needs.  Host-only."""
    return [(p, *_overlap(own[p], need[rank])) for p in range(len(own)) if p != rank and _overlap(own[p], need[rank])[1]]


def exchange_need_rows(tensor_view, own, need, world):
    """A ranged exchange point: every rank receives, from each rank that owns some, the rows of its need range -- point to point, one
    transfer per (owner, reader) pair with rows in common, straight from and into `tensor_view`.  Uneven and empty ranges need no padding;
    under gloo the rows are staged through host memory.  Returns the bytes this rank received."""
    if len(own) != world or len(need) != world:
        raise ValueError(f"exchange_need_rows: {len(own)} own and {len(need)} need ranges for {world} ranks")
    if not _live(world):
        return 0
    rank, staged = dist.get_rank(), dist.get_backend() == "gloo"
    ops, landing, received = [], [], 0
    for q in range(world):
        for p, first, count in needed_from(own, need, q):
            rows = tensor_view[first:first + count]
            if rank == p:
                ops.append(dist.P2POp(dist.isend, rows.cpu() if staged else rows, q))
            elif rank == q:
                buf = torch.empty(rows.shape, dtype=rows.dtype) if staged else rows
                ops.append(dist.P2POp(dist.irecv, buf, p))
                landing.append((rows, buf))
                received += rows.numel() * 8
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    for rows, buf in landing:
        if staged:
            rows.copy_(buf)
    if tensor_view.is_cuda:
        torch.cuda.synchronize(tensor_view.device)
    return received


def run_sharded_rows(session, plans, n_ops, shard_rows, rank, world, dev, timing=False):
    """run_sharded with the max pools divided: plans[p] is part p's plan with row ranges [(after_op, tensor, first, count)]
    (CompiledCircuit.shard_plan(rows=True, part=p, ...); the entries agree between the parts, the ranges differ).  An entry whose range is
    the whole tensor for every part is the broadcast exchange and mark_whole; any other sends each rank its need range and ends in
    mark_rows.  -> (timings of the spans, bytes exchanged)"""
    timings, moved, first = [], 0, 0
    for i, (after_op, tensor, _, _) in enumerate(plans[rank]):
        if after_op + 1 > first:
            timings.append(session.run_span(first, after_op + 1, timing))
            first = after_op + 1
        view = tensor_view(session, tensor, dev)
        rows = view.shape[0]
        own = [shard_rows(rows, world, p) for p in range(world)]
        need = [tuple(plans[p][i][2:4]) for p in range(world)]
        if all(n == (0, rows) for n in need):
            moved += exchange_rows(view, own, world)
            session.mark_whole(tensor)
        else:
            moved += exchange_need_rows(view, own, need, world)
            session.mark_rows(tensor, *need[rank])
    if first < n_ops:
        timings.append(session.run_span(first, n_ops, timing))
    return timings, moved
