"""Writes profiles/key_tiers.json: evaluation keys sized to the circuit (include/dctfhe.h TIER SELECTIONS) against
the keys of the whole catalogue, for the three ResNet-20 24x16^2 circuits of the catalogues.  Per circuit and selection: the bytes of both
blob forms by the formula (dctfhe_key_tiers_blob_bytes) and as exported, the seconds of the host library's compressed export at this
machine's thread count, the seconds of its import on the GPU, dctfhe_device_bytes_live with the keys resident, and the seconds of the
full-form export of the imported handle.  One machine, one run: figures, not thresholds.

    python tools/key_tiers_profile.py --out profiles/key_tiers.json [--no-gpu]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CIRCUITS = [
    ("ResNet-20 24x16^2, 4 / 6 bits, default_params() (the benchmark circuit)", dict(bit_width=4, n_bits=5, rounding_threshold_bits=6)),
    ("ResNet-20 24x16^2, 5 / 6 bits, default_params_5bit()", dict(bit_width=5, n_bits=5, rounding_threshold_bits=6)),
    ("ResNet-20 24x16^2, 5 / 7 bits, default_params_5bit()", dict(bit_width=5, n_bits=5, rounding_threshold_bits=7)),
]


def _timed(fn, *a):
    t0 = time.perf_counter()
    out = fn(*a)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--no-gpu", action="store_true", help="formula bytes and host export only")
    a = ap.parse_args()
    from dctfhe import _lib_client, compile as cc, engine, models, params as P
    from dctfhe.host_client import HostClientKey
    from dctfhe.synthetic import synthetic_dct_batch
    rec = dict(threads=_lib_client.load().dctfhe_host_threads(), omp_num_threads=os.environ.get("OMP_NUM_THREADS"), note="one machine, one run", circuits=[])
    ctx = None if a.no_gpu else engine.Context(0)
    for label, kw in CIRCUITS:
        kw = dict(kw)
        c = cc.compile_model(models.ResNet20QAT(kw.pop("bit_width"), 24, 16), synthetic_dct_batch(24, seed=7), **kw)
        ps, cp = c.param_set, P.to_c_params(c.param_set)
        sel = c.key_tiers()
        report = c.key_report()
        r = dict(circuit=label, tiers=[t.name for t in ps.tiers], bootstraps_on=sorted(sel.bsk), key_switch_owners=sorted(sel.ksk),
                 never_bootstraps_on=[t.name for t in ps.tiers if t.name not in sel.bsk], bsk_mask=sel.bsk_mask, ksk_mask=sel.ksk_mask,
                 per_tier=report["tiers"], keys={})
        host = HostClientKey(cp, 5)
        for name, s in (("all", None), ("circuit", sel)):
            kt = engine.key_tiers_all(cp) if s is None else s
            k = dict(formula_compressed_bytes=engine.key_tiers_blob_bytes(cp, kt, True), formula_full_bytes=engine.key_tiers_blob_bytes(cp, kt, False))
            blob, k["host_export_compressed_s"] = _timed(host.export_eval_keys_compressed, s)
            k["compressed_blob_bytes"] = int(blob.size)
            if ctx is not None:
                base = engine.device_bytes_live()
                keys, k["device_import_s"] = _timed(engine.EvalKeys.from_blob, ctx, blob)
                try:
                    k["device_bytes_live_keys_resident"] = engine.device_bytes_live() - base
                    full, k["device_export_full_s"] = _timed(keys.to_blob)
                    k["full_blob_bytes"] = int(full.size)
                    del full
                finally:
                    keys.close()
            del blob
            r["keys"][name] = k
            print(label, name, json.dumps(k), flush=True)
        host.close()
        rec["circuits"].append(r)
    if ctx is not None:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
