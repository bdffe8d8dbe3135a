"""Writes profiles/shard_r20.json: the COMPUTE side of sharding one ResNet-20 24x16^2 image over P GPUs, measured on
ONE GPU by running the P parts in turn in one process (loopback copies stand in for the exchange, and are not timed).  Per P in --parts:
every part's time over its spans (HIP events around dctfhe_session_run_span), the slowest part -- the projected compute latency --, the
sum over parts against the P = 1 time -- what under-filled launches cost --, the bytes each exchange moves, and the outputs of every
part against the integer circuit.  The exchange itself and any run on more than one GPU are NOT measured here.

    python tools/shard_profile.py [--parts 1,2,4,8] [--reps 2] [--out profiles/shard_r20.json] [--parent-run FILE]
    python tools/shard_profile.py --plain-run-only --out FILE      # dctfhe_session_run alone: runs on a checkout without the sharding calls
    python tools/shard_profile.py --model r18_crop96 --shard-pool both --reps 1 --out profiles/shard_pool_r18_crop96.json
--parent-run: the --plain-run-only record of the parent commit on the same box, quoted beside this tree's figures.
--model: r20 (the default), r18_crop96 (the 64_3_224 weights, all four stages, on the 96x96 crop of profiles/maxpool_crop96_kernel_stats.txt)
or r18_224 (the whole 3x224^2 image).  --shard-pool off | on | both: the stem max pool whole on every part (set_shard alone), divided
(set_shard_pool, DESIGN.md section 8.1: the plan with row ranges, each part receives its need range), or both in turn in one visit; an
entry then says which, and holds the pairwise maxima every part's pool ran and the bytes every part receives.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_r20.json"))
    ap.add_argument("--plain-run-only", action="store_true")
    ap.add_argument("--parent-run", default=None)
    ap.add_argument("--model", default="r20", choices=["r20", "r18_crop96", "r18_224"])
    ap.add_argument("--shard-pool", default="off", choices=["off", "on", "both"])
    args = ap.parse_args()
    import bench
    from dctfhe import compile as cc, models
    from dctfhe.engine import Session
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from oracle import circuit_ref
    if args.model == "r20":
        # the benchmark's workload: its model, calibration batch, catalogue and key seed
        factory, in_ch, img, make_batch, _ = bench.CONFIGS["r20_24_16"]
        model = getattr(models, factory)(bit_width=4, in_channels=in_ch, img_size=img, seed=0)
        calib, image = make_batch(100, 7), make_batch(1, 42)
        label = "ResNet-20 24x16^2, default_params(), one image (bench.py's r20_24_16)"
    else:
        # the RGB ResNet-18 trunk with the stem MaxPool2d (64_3_224), as tests/test_gpu_maxpool.py runs it: synthetic images, 12 to calibrate
        from dctfhe import frontend, synthetic
        tf = frontend.rgb_eval_transform(224)
        x = np.stack([tf(im) for im in synthetic.synthetic_images(13, 7)]).astype(np.float32)
        model = models.ResNet18QAT(bit_width=4, in_channels=3, img_size=224)
        label = "ResNet-18 3x224^2 RGB (64_3_224), default_params(), one image"
        if args.model == "r18_crop96":
            x, model = x[:, :, 64:160, 64:160], models.trunk_prefix(model, n_blocks=8, avgpool_kernel=3)
            label = "ResNet-18 3x224^2 RGB weights (64_3_224), all four stages, 96x96 crop (avgpool 3), default_params(), one image"
        calib, image = x[:12], x[12:13]
    qm = compile_brevitas_qat_model(model, calib, n_bits=5, rounding_threshold_bits=6, p_error=0.01)
    rec = dict(model=label, reps=args.reps)
    try:
        qm.fhe_circuit.keygen(seed=bench.KEY_SEED)
        keys, c = qm._keys, qm.compiled
        q = qm.quantize_input(image)
        phases = qm.encode_input(q)
        ref, overflow = circuit_ref.run_clear(c.blob, phases)
        want = qm.decode_output(ref)
        seeded = keys.encrypt_seeded(phases.reshape(-1))

        def outputs(sess):
            out_dim = sess.dims()[1]
            return qm.decode_output(keys.decrypt(sess.download(out_dim).reshape(-1, out_dim + 1), out_dim).reshape(1, -1))

        # dctfhe_session_run, the unsharded path: one warm-up pass, then the repetitions
        sess = Session(qm._context(), qm._circuit, keys, 1)
        sess.upload_seeded(seeded)
        sess.run()
        runs = [sess.run(timing=True).total_ms for _ in range(args.reps)]
        rec["plain_run"] = dict(total_ms=runs, min_ms=min(runs), equals_integer_circuit=bool(not overflow and np.array_equal(outputs(sess), want)))
        sess.close()
        print(json.dumps(rec["plain_run"]), flush=True)
        if not args.plain_run_only:
            from dctfhe.compile import shard_rows
            n_ops = len(c.ops)
            pools = [i for i, o in enumerate(c.ops) if o.type == cc.OP_MAXPOOL]
            rec["exchanges"] = len(c.shard_plan())
            rec["by_parts"] = []
            settings = {"off": [False], "on": [True], "both": [False, True]}[args.shard_pool]
            for P, divided in [(int(x), d) for x in args.parts.split(",") for d in settings]:
                if divided and P == 1 and len(settings) == 2:
                    continue      # one part of one is the undivided op: the same run as with the switch off
                sessions = [Session(qm._context(), qm._circuit, keys, 1) for _ in range(P)]
                try:
                    for p, s in enumerate(sessions):
                        s.set_shard(p, P)
                        if divided:
                            s.set_shard_pool(True)
                        s.upload_seeded(seeded)
                    # per part the plan with the rows it needs of each exchanged tensor: whole tensors unless a divided pool reads them
                    plans = [s.shard_plan_rows() for s in sessions]
                    assert plans == [c.shard_plan(rows=True, part=p, parts=P if divided else 1) for p in range(P)]
                    geometry = [sessions[0].tensor(t) for _, t, _, _ in plans[0]]
                    received = [0] * P
                    per_exchange = []
                    for i, ((a, t, _, _), (_, L, rows)) in enumerate(zip(plans[0], geometry)):
                        own = [shard_rows(rows, P, p) for p in range(P)]
                        got = [sum(min(f + n, own[p][0] + own[p][1]) - max(f, own[p][0]) for p in range(P)
                                   if p != qi and min(f + n, own[p][0] + own[p][1]) > max(f, own[p][0])) for qi, (_, _, f, n) in enumerate(pl[i] for pl in plans)]
                        for qi in range(P):
                            received[qi] += 8 * L * got[qi]
                        per_exchange.append(dict(after_op=a, tensor=t, rows=rows, row_bytes=8 * L, tensor_bytes=8 * L * rows,
                                                 largest_part_bytes=8 * L * own[0][1], rows_needed_per_part=[pl[i][3] for pl in plans],
                                                 bytes_received_per_part=[8 * L * g for g in got]))
                    passes = []
                    for _ in range(args.reps):
                        ms, first = [0.0] * P, 0
                        for i, (after_op, tensor) in enumerate([(a, t) for a, t, _, _ in plans[0]] + [(n_ops - 1, None)]):
                            for p, s in enumerate(sessions):
                                ms[p] += s.run_span(first, after_op + 1, timing=True).total_ms
                            first = after_op + 1
                            if tensor is None:
                                break
                            rows = sessions[0].tensor(tensor)[2]
                            for qi, dst in enumerate(sessions):
                                f, n = plans[qi][i][2:4]
                                for p, src in enumerate(sessions):
                                    lo, hi = max(f, shard_rows(rows, P, p)[0]), min(f + n, sum(shard_rows(rows, P, p)))
                                    if p != qi and hi > lo:
                                        dst.copy_rows_from(src, tensor, lo, hi - lo)
                                if (f, n) == (0, rows):
                                    dst.mark_whole(tensor)
                                else:
                                    dst.mark_rows(tensor, f, n)
                        passes.append(ms)
                    best = min(passes, key=max)
                    exact = all(np.array_equal(outputs(s), want) for s in sessions)
                    total = sum(e["tensor_bytes"] for e in per_exchange)
                    entry = dict(parts=P, shard_pool=divided, part_ms=passes, slowest_part_ms=max(best), sum_of_parts_ms=sum(best),
                                 every_part_equals_integer_circuit=bool(exact), tensor_bytes_exchanged=total,
                                 bytes_received_per_part=received if pools else total - sum(e["largest_part_bytes"] for e in per_exchange),
                                 pool_pairs_per_part=[[s.pool_pairs(i) for i in pools] for s in sessions] if pools else None,
                                 exchanges=per_exchange if P == 2 else [e for e in per_exchange if e["rows_needed_per_part"] != [e["rows"]] * P] or None)
                    rec["by_parts"].append(entry)
                    print(json.dumps({k: v for k, v in entry.items() if k != "exchanges"}), flush=True)
                finally:
                    for s in sessions:
                        s.close()
            one = next((e for e in rec["by_parts"] if e["parts"] == 1), None)
            for e in rec["by_parts"]:      # the divided pool against the same parts with the switch off
                off = next((x for x in rec["by_parts"] if x["parts"] == e["parts"] and not x["shard_pool"]), None)
                if e["shard_pool"] and off:
                    e["slowest_part_over_undivided"] = e["slowest_part_ms"] / off["slowest_part_ms"]
            for e in rec["by_parts"]:
                if one:
                    e["sum_of_parts_over_one_part"] = e["sum_of_parts_ms"] / one["sum_of_parts_ms"]
                    e["compute_speedup_projected"] = one["slowest_part_ms"] / e["slowest_part_ms"]
            if one:
                rec["one_part_through_run_span_vs_plain_run"] = one["slowest_part_ms"] / rec["plain_run"]["min_ms"]
            if args.parent_run:
                with open(args.parent_run) as f:
                    rec["parent_commit_plain_run"] = json.load(f)["plain_run"]
                if one:
                    rec["one_part_through_run_span_vs_parent_run"] = one["slowest_part_ms"] / rec["parent_commit_plain_run"]["min_ms"]
            rec["not_measured"] = "the exchange between GPUs (RCCL broadcasts) and any run on more than one GPU; the loopback copies are outside the timed spans"
    finally:
        qm.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
