"""Writes profiles/ring_outputs_r20.json: the three ways a ResNet-20 24x16^2 result travels back -- full rows, 16-bit rows, ring-packed --
measured in ONE process on one key set: bytes, download time and decryption time for one image and for a batch of eight, plus the
packing key's size and generation time.  Times are wall-clock around the synchronous calls, one warm-up call
and then `--reps` repetitions (median and minimum reported).

    python tools/ring_outputs_profile.py [--reps 5] [--batches 1,8] [--out profiles/ring_outputs_r20.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, reps):
    fn()                                   # warm-up: first-launch costs, scratch allocations
    ts, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return out, dict(median_ms=1e3 * statistics.median(ts), min_ms=1e3 * min(ts), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_outputs_r20.json"))
    args = ap.parse_args()
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from dctfhe.synthetic import synthetic_dct_batch
    from oracle import circuit_ref
    qm = compile_brevitas_qat_model(models.ResNet20QAT(4, 24, 16), synthetic_dct_batch(16, seed=7))
    rec = dict(model="ResNet-20 24x16^2, default_params()", results_per_image=qm.compiled.n_out(), batches=[])
    try:
        t = time.perf_counter()
        qm.fhe_circuit.keygen(seed=11)
        rec["keygen_s"] = time.perf_counter() - t
        keys = qm._keys
        rows_oc, ring_oc = qm.output_compaction(), qm.output_compaction("ring")
        t = time.perf_counter()
        blob = qm.fhe_circuit.export_result_packing_key()
        gen_s = time.perf_counter() - t
        t = time.perf_counter()
        qm.fhe_circuit.load_result_packing_key(blob)
        spec = ring_oc.spec
        rec["packing_key"] = dict(bytes=int(blob.size), generate_and_export_s=gen_s, import_s=time.perf_counter() - t, logN=spec.logN, levels=spec.l,
                                  base_bits=spec.beta, log2_sigma=float(np.log2(spec.sigma)), n_max=int(keys.params.n_max))
        rec["tier"] = dict(name=ring_oc.name, n=ring_oc.n, pfail_rows=rows_oc.pfail, pfail_ring=ring_oc.pfail,
                           log2_var_rows=float(np.log2(rows_oc.var)), log2_var_ring=float(np.log2(ring_oc.var)))
        # the primitive on a FULL group of random small ciphertexts (host call: 13 MB up, the pack, 8 KB down)
        small = np.random.default_rng(1).integers(0, 1 << 64, (spec.N, ring_oc.n + 1), dtype=np.uint64)
        _, rec["full_group_ring_pack"] = timed(lambda: qm._pack_key.ring_pack(small), args.reps)
        rec["full_group_ring_pack"].update(results=spec.N, n=ring_oc.n, mac_u64=2 * spec.N * spec.N * ring_oc.n * spec.l)
        for B in [int(b) for b in args.batches.split(",")]:
            q = qm.quantize_input(synthetic_dct_batch(B, seed=100 + B))
            ref, overflow = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
            want = qm.decode_output(ref)
            sess = qm._session("execute", B)
            in_dim, out_dim = sess.dims()
            sess.upload(keys.encrypt(qm.encode_input(q).reshape(-1), in_dim), in_dim)
            t = time.perf_counter()
            sess.run()
            run_s = time.perf_counter() - t
            forms = {}
            full, forms["full_rows"] = timed(lambda: sess.download(out_dim).reshape(-1, out_dim + 1), args.reps)
            rows, forms["rows16"] = timed(lambda: sess.download_packed(rows_oc.tier), args.reps)
            ring, forms["ring"] = timed(lambda: sess.download_ring(ring_oc.tier, qm._pack_key), args.reps)
            dec = {}
            dec["full_rows"], d0 = timed(lambda: keys.decrypt(full, out_dim), args.reps)
            dec["rows16"], d1 = timed(lambda: keys.decrypt_packed(rows), args.reps)
            dec["ring"], d2 = timed(lambda: keys.decrypt_ring(ring), args.reps)
            nbytes = dict(full_rows=int(full.nbytes), rows16=int(rows.rows.nbytes), ring=int(ring.words.nbytes))
            entry = dict(batch=B, results=B * qm.compiled.n_out(), run_s=run_s, overflow=bool(overflow))
            for name, dt in (("full_rows", d0), ("rows16", d1), ("ring", d2)):
                got = qm.decode_output(dec[name].reshape(B, -1))
                entry[name] = dict(bytes=nbytes[name], download=forms[name], decrypt=dt, equals_integer_circuit=bool(np.array_equal(got, want)))
            rec["batches"].append(entry)
            print(json.dumps(entry))
    finally:
        qm.close()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
