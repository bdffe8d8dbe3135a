"""Writes profiles/shard_r20.json: the COMPUTE side of sharding one ResNet-20 24x16^2 image over P GPUs, measured on
ONE GPU by running the P parts in turn in one process (loopback copies stand in for the exchange, and are not timed).  Per P in --parts:
every part's time over its spans (HIP events around dctfhe_session_run_span), the slowest part -- the projected compute latency --, the
sum over parts against the P = 1 time -- what under-filled launches cost --, the bytes each exchange moves, and the outputs of every
part against the integer circuit.  The exchange itself and any run on more than one GPU are NOT measured here.

    python tools/shard_profile.py [--parts 1,2,4,8] [--reps 2] [--out profiles/shard_r20.json] [--parent-run FILE]
    python tools/shard_profile.py --plain-run-only --out FILE      # dctfhe_session_run alone: runs on a checkout without the sharding calls
--parent-run: the --plain-run-only record of the parent commit on the same box, quoted beside this tree's figures.
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
    args = ap.parse_args()
    import bench
    from dctfhe import models
    from dctfhe.engine import Session
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from oracle import circuit_ref
    # the benchmark's workload: its model, calibration batch, catalogue and key seed
    factory, in_ch, img, make_batch, _ = bench.CONFIGS["r20_24_16"]
    model = getattr(models, factory)(bit_width=4, in_channels=in_ch, img_size=img, seed=0)
    qm = compile_brevitas_qat_model(model, make_batch(100, 7), n_bits=5, rounding_threshold_bits=6, p_error=0.01)
    rec = dict(model="ResNet-20 24x16^2, default_params(), one image (bench.py's r20_24_16)", reps=args.reps)
    try:
        qm.fhe_circuit.keygen(seed=bench.KEY_SEED)
        keys, c = qm._keys, qm.compiled
        q = qm.quantize_input(make_batch(1, 42))
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
            plan, n_ops = c.shard_plan(), len(c.ops)
            rec["exchanges"] = len(plan)
            rec["by_parts"] = []
            for P in [int(x) for x in args.parts.split(",")]:
                sessions = [Session(qm._context(), qm._circuit, keys, 1) for _ in range(P)]
                try:
                    for p, s in enumerate(sessions):
                        s.set_shard(p, P)
                        s.upload_seeded(seeded)
                    geometry = [sessions[0].tensor(t) for _, t in plan]
                    per_exchange = [dict(after_op=a, tensor=t, rows=rows, row_bytes=8 * L, tensor_bytes=8 * L * rows,
                                         largest_part_bytes=8 * L * shard_rows(rows, P, 0)[1])
                                    for (a, t), (_, L, rows) in zip(plan, geometry)]
                    passes = []
                    for _ in range(args.reps):
                        ms, first = [0.0] * P, 0
                        for after_op, tensor in plan + [(n_ops - 1, None)]:
                            for p, s in enumerate(sessions):
                                ms[p] += s.run_span(first, after_op + 1, timing=True).total_ms
                            first = after_op + 1
                            if tensor is None:
                                break
                            rows = sessions[0].tensor(tensor)[2]
                            for qi, dst in enumerate(sessions):
                                for p, src in enumerate(sessions):
                                    if p != qi:
                                        dst.copy_rows_from(src, tensor, *shard_rows(rows, P, p))
                                dst.mark_whole(tensor)
                        passes.append(ms)
                    best = min(passes, key=max)
                    exact = all(np.array_equal(outputs(s), want) for s in sessions)
                    total = sum(e["tensor_bytes"] for e in per_exchange)
                    entry = dict(parts=P, part_ms=passes, slowest_part_ms=max(best), sum_of_parts_ms=sum(best), every_part_equals_integer_circuit=bool(exact),
                                 tensor_bytes_exchanged=total, bytes_received_per_part=total - sum(e["largest_part_bytes"] for e in per_exchange),
                                 exchanges=per_exchange if P == 2 else None)
                    rec["by_parts"].append(entry)
                    print(json.dumps({k: v for k, v in entry.items() if k != "exchanges"}), flush=True)
                finally:
                    for s in sessions:
                        s.close()
            one = next((e for e in rec["by_parts"] if e["parts"] == 1), None)
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
