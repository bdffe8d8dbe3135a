"""Writes profiles/public_inputs_r20.json: the three ways a ResNet-20 24x16^2 input travels in -- compact rows, seeded, public-key --
measured in ONE process on one key set: bytes, encryption time and upload time for one image and for a batch of eight, every form run
through the circuit and decoded against the integer circuit.  Times are wall-clock around the synchronous calls,
one warm-up call and then `--reps` repetitions (median and minimum reported).  The comparable of the public-key upload (k_pk_extract) is
the seeded upload (k_seeded_expand) of the same build: both write the same input tensor.

    python tools/public_inputs_profile.py [--reps 5] [--batches 1,8] [--out profiles/public_inputs_r20.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "public_inputs_r20.json"))
    args = ap.parse_args()
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from dctfhe.synthetic import synthetic_dct_batch
    from oracle import circuit_ref
    qm = compile_brevitas_qat_model(models.ResNet20QAT(4, 24, 16), synthetic_dct_batch(16, seed=7))
    rec = dict(model="ResNet-20 24x16^2, default_params()", inputs_per_image=qm.compiled.n_in(), batches=[])
    try:
        t = time.perf_counter()
        qm.fhe_circuit.keygen(seed=11)
        rec["keygen_s"] = time.perf_counter() - t
        keys = qm._keys
        plan = qm.public_input_plan()
        t = time.perf_counter()
        blob = qm.fhe_circuit.export_public_key()
        gen_s = time.perf_counter() - t
        t = time.perf_counter()
        qm.fhe_circuit.load_public_key(blob)
        pk = qm._public_key
        rec["public_key"] = dict(bytes=int(blob.size), generate_and_export_s=gen_s, import_s=time.perf_counter() - t, logN=plan.spec.logN,
                                 log2_sigma=float(np.log2(plan.spec.sigma)))
        rec["plan"] = dict(log2_var_public_input=float(np.log2(plan.var)), log2_var_fresh=float(2 * np.log2(qm.compiled.param_set.input_sigma)),
                           worst_site=plan.worst_site, worst_note=plan.worst_note, worst_pfail=plan.worst_pfail,
                           worst_pfail_fresh=plan.worst_pfail_fresh, bytes_per_image=plan.bytes_per_image)
        for B in [int(b) for b in args.batches.split(",")]:
            q = qm.quantize_input(synthetic_dct_batch(B, seed=100 + B))
            ref, overflow = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
            want = qm.decode_output(ref)
            phases = qm.encode_input(q).reshape(-1)
            sess = qm._session("execute", B)
            in_dim, out_dim = sess.dims()
            enc, up = {}, {}
            rows, enc["rows"] = timed(lambda: keys.encrypt(phases, in_dim), args.reps)
            seeded, enc["seeded"] = timed(lambda: keys.encrypt_seeded(phases), args.reps)
            public, enc["public"] = timed(lambda: pk.encrypt(phases), args.reps)
            uploads = dict(rows=lambda: sess.upload(rows, in_dim), seeded=lambda: sess.upload_seeded(seeded), public=lambda: sess.upload_public(public))
            nbytes = dict(rows=int(rows.nbytes), seeded=int(seeded.bodies.nbytes), public=int(public.words.nbytes))
            tensor_bytes = B * qm.compiled.n_in() * (in_dim + 1) * 8
            entry = dict(batch=B, inputs=B * qm.compiled.n_in(), overflow=bool(overflow), input_tensor_bytes_at_least=tensor_bytes)
            for name in ("rows", "seeded", "public"):
                _, up[name] = timed(uploads[name], args.reps)          # the last upload of this form stays in the tensor
                t = time.perf_counter()
                sess.run()
                run_s = time.perf_counter() - t
                got = qm.decode_output(keys.decrypt(sess.download(out_dim).reshape(-1, out_dim + 1), out_dim).reshape(B, -1))
                entry[name] = dict(bytes=nbytes[name], encrypt=enc[name], upload=up[name], run_s=run_s,
                                   equals_integer_circuit=bool(np.array_equal(got, want)))
                print(json.dumps({name: entry[name], "batch": B}))
            rec["batches"].append(entry)
    finally:
        qm.close()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
