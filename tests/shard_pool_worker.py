"""The cases of tests/test_gpu_shard_pool.py that touch a session's device memory through torch (dctfhe.sharding.tensor_view), run as a fresh
interpreter in which torch initialises the GPU before the library does -- the order of every process that uses both (tests/shard_rank_worker.py).
Prints one JSON line.
--mode poison: P = 3, encrypted; once every part holds its need range of the pool's source, each overwrites every other row of that tensor
with a fixed pattern through the pointer dctfhe_session_tensor hands out; the outputs must still be the unsharded run's.
--mode simulate: clear mode with a fixed noise seed and a sigma of 1/32 of the torus on the pool (the half-box of its 5-bit table is 1/128;
the model's sigma moves no relu entry), stopped behind the pool: each part's rows of the pool's output against the unsharded session's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["poison", "simulate"], required=True)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    import test_gpu_shard_pool as T
    from dctfhe import params as P
    from dctfhe.compile import shard_rows
    from dctfhe.engine import Context, Keys
    ctx = Context(0)
    keys = Keys(ctx, P.to_c_params(P.test_params()), seed=3) if a.mode == "poison" else None
    res = []
    try:
        if a.mode == "poison":
            for geom in ("k3s2-9", "k2s2-6"):
                case = T.Case(ctx, keys, geom)
                sessions = T.make_sessions(case, 3)
                try:
                    T.drive(case, sessions, poison=True)
                    rows = sessions[0].tensor(case.pool_src)[2]
                    for p, s in enumerate(sessions):
                        need = case.plans(3)[p][0]
                        res.append(dict(geom=geom, part=p, tensor=need[1], pool_src=case.pool_src, rows=rows, rows_overwritten=rows - need[3],
                                        equal=bool(np.array_equal(s.download(case.out_dim), case.ref_rows))))
                finally:
                    T.close_all(sessions)
                    case.close()
        else:
            for geom in T.GEOMS:
                case = T.Case(ctx, None, geom)
                c = case.qm.compiled
                sig, sig2 = list(c.simulation_sigmas()), list(c.simulation_sigmas_split())
                sig[case.pool_op] = 1.0 / 32
                noise, end = (20261019, sig, sig2), case.pool_op + 1
                ref = T._clear_outputs(case, 0, noise, end, case.pool_dst)[0]
                quiet = T._clear_outputs(case, 0, None, end, case.pool_dst)[0]
                for parts in (2, 3, 5):
                    for p, rows in enumerate(T._clear_outputs(case, parts, noise, end, case.pool_dst)):
                        f, n = shard_rows(ref.shape[0], parts, p)
                        res.append(dict(geom=geom, parts=parts, part=p, words_moved_by_noise=int((ref != quiet).sum()), words=int(ref.size),
                                        equal=bool(np.array_equal(rows[f:f + n], ref[f:f + n]))))
                case.close()
    finally:
        if keys is not None:
            keys.close()
        ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
