"""Wall times of the host client library (include/dctfhe_client.h) on this machine's CPUs, and whether what it makes serves on the GPU:
per catalogue the compressed evaluation-key export (seconds, bytes), its import on the device and the key check of dctfhe.deploy
(made and verified on the host, answered on the device); the seeded encryption of one ResNet-20 input (6 144 values); the decryption of
one ring-packed response.  One machine, one run: figures, not thresholds.

    python tools/host_client_profile.py --out profiles/host_client.json [--no-gpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

U = np.uint64


def _timed(fn, *a):
    t0 = time.perf_counter()
    out = fn(*a)
    return out, time.perf_counter() - t0


def key_check(ps, host, keys):
    """dctfhe.deploy's key check by hand (no bundle at hand for a bare catalogue): per tier a few encryptions of known messages made on
    the host, key switch -> centred mod switch -> identity-table bootstrap on the device, decrypted and compared on the host"""
    from dctfhe import deploy
    dim, D, worst = host.input_dim, host.D, 0.0
    for ti, w in enumerate(deploy.key_check_bits(ps)):
        msgs = deploy.key_check_messages(w)
        rows = host.encrypt(msgs << U(63 - w), dim)
        full = np.zeros((rows.shape[0], D + 1), U)
        full[:, :dim], full[:, D] = rows[:, :dim], rows[:, dim]
        table = deploy.key_check_table(w)
        out = keys.pbs(ti, keys.modswitch_center(ti, keys.keyswitch(ti, full, 0, dim)), table, w)
        want = (table[msgs.astype(np.int64)] if w else np.where(msgs == 0, table[0], -table[0])).astype(U)
        err = np.abs((host.decrypt(out) - want).astype(np.int64).astype(np.float64)) / 2.0 ** 64
        tol = 2.0 ** -(max(w, 5) + 4)
        if not (err < tol).all():
            return False, "tier %d (%s): error 2^%.1f, allowed 2^%.0f" % (ti, ps.tiers[ti].name, np.log2(err.max()), np.log2(tol))
        worst = max(worst, float(err.max() / tol))
    return True, "largest error %.3g of its tolerance" % worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--no-gpu", action="store_true", help="host timings only")
    a = ap.parse_args()
    from dctfhe import _lib_client, params as P
    from dctfhe.host_client import HostClientKey
    from dctfhe.wire import PackedRing
    rec = dict(threads=_lib_client.load().dctfhe_host_threads(), omp_num_threads=os.environ.get("OMP_NUM_THREADS"), note="one machine, one run", catalogues={})
    ctx = None
    if not a.no_gpu:
        from dctfhe.engine import Context, EvalKeys
        ctx = Context(0)
    for name, ps in (("default_params", P.default_params()), ("default_params_5bit_pool", P.default_params_5bit_pool())):
        host, t_key = _timed(HostClientKey, P.to_c_params(ps), 5)
        blob, t_exp = _timed(host.export_eval_keys_compressed)
        r = dict(tiers=len(ps.tiers), client_key_create_s=t_key, export_evaluation_keys_compressed_s=t_exp, blob_bytes=int(blob.size))
        if name == "default_params":
            phases = np.random.default_rng(0).integers(0, 2 ** 64, 6144, dtype=U)
            sc, t_enc = _timed(host.encrypt_seeded, phases)
            r.update(encrypt_seeded_6144_s=t_enc, encrypt_seeded_bytes=sc.nbytes)
            _, t_rows = _timed(host.encrypt, phases, host.input_dim)
            r.update(encrypt_rows_6144_s=t_rows)
            ring = PackedRing(11, 64, np.random.default_rng(1).integers(0, 1 << 16, PackedRing.n_words(11, 64), dtype=np.uint16))
            _, t_dec = _timed(host.decrypt_ring, ring)
            r.update(decrypt_ring_64_results_logN11_s=t_dec, decrypt_ring_note="random words: the time does not depend on them")
            spec = P.default_pack_spec(ps)
            pk, t_pk = _timed(host.export_pack_key, spec)
            r.update(export_pack_key_s=t_pk, pack_key_bytes=int(pk.size))
            pub, t_pub = _timed(host.export_public_key, P.default_public_input_spec(ps))
            r.update(export_public_key_s=t_pub, public_key_bytes=int(pub.size))
        if ctx is not None:
            keys, t_imp = _timed(EvalKeys.from_blob, ctx, blob)
            try:
                ok, text = key_check(ps, host, keys)
            finally:
                keys.close()
            r.update(device_import_s=t_imp, device_key_check_passes=ok, device_key_check=text)
        del blob
        host.close()
        rec["catalogues"][name] = r
        print(name, json.dumps(r), flush=True)
    if ctx is not None:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
