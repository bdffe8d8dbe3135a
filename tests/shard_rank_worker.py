"""One rank of tests/test_gpu_shard_ranks.py, run as a fresh interpreter: joins a torch.distributed group, evaluates the tiny trunk with
Configuration(shard_image=True) and prints one JSON line.  --mode forward: the sharded forward() of a rank of a gloo group.  --mode
loopback: world size 1 on the nccl backend -- forward() (the plain path there) against a sharded pass driven through
dctfhe.sharding.run_sharded, whose exchange_rows broadcasts the session's own device memory."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["forward", "loopback"], required=True)
    ap.add_argument("--backend", choices=["gloo", "nccl"], required=True)
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    a = ap.parse_args()
    from dctfhe import compile as cc, models, params as P, sharding
    from dctfhe.engine import Session
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    from oracle import circuit_ref
    torch.cuda.set_device(0)
    dist.init_process_group(a.backend, init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank, world_size=a.world)
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=P.test_params(),
                                    configuration=Configuration(shard_image=True))
    res = dict(rank=a.rank, world=a.world, backend=dist.get_backend())
    try:
        qm.fhe_circuit.keygen(seed=3)
        x = calib[:2]
        q = qm.quantize_input(x)
        ref, overflow = circuit_ref.run_clear(qm.compiled.blob, qm.encode_input(q))
        assert not overflow
        res["want"] = qm.dequantize_output(qm.decode_output(ref)).tolist()
        res["out"] = qm.forward(x, fhe="execute").tolist()
        res["io"] = {k: v for k, v in qm.last_io.items() if k in ("shard", "exchanged_bytes", "upload_bytes")}
        if a.mode == "loopback":
            dev = torch.device("cuda", 0)
            sess = Session(qm._context(), qm._circuit, qm._keys, 2)
            try:
                sess.set_shard(0, 1)
                sess.upload_seeded(qm._keys.encrypt_seeded(qm.encode_input(q).reshape(-1)))
                plan = qm.compiled.shard_plan()
                view = sharding.tensor_view(sess, plan[0][1], dev)
                ptr, row_words, rows = sess.tensor(plan[0][1])
                res["view"] = dict(same_memory=view.data_ptr() == ptr, shape=list(view.shape), want_shape=[rows, row_words], device=str(view.device))
                sharding.run_sharded(sess, plan, len(qm.compiled.ops), cc.shard_rows, 1, dev)
                out_dim = sess.dims()[1]
                ph = qm._keys.decrypt(sess.download(out_dim).reshape(-1, out_dim + 1), out_dim).reshape(2, -1)
                res["sharded_pass"] = qm.dequantize_output(qm.decode_output(ph)).tolist()
            finally:
                sess.close()
        dist.barrier()
    finally:
        qm.close()
    print("RESULT " + json.dumps(res), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
