"""Configuration(shard_image=True) between processes.  Two ranks of a gloo group share GPU 0 -- fresh interpreters
(tests/shard_rank_worker.py), each under its own time limit: rank 0 encrypts and broadcasts the seeded blob, both walk the exchange plan
with host-staged broadcasts, both decrypt the integer circuit's outputs.  One rank on the nccl backend: the same exchange on device
memory.  (Two RCCL ranks on one device are refused by RCCL and would prove nothing.)"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shard_rank_worker.py")
LIMIT_S = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _start(mode, backend, rank, world, port):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, WORKER, "--mode", mode, "--backend", backend, "--rank", str(rank), "--world", str(world),
           "--port", str(port)]
    return subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _result(proc):
    out, err = proc.communicate()
    assert proc.returncode == 0, (proc.returncode, out[-2000:], err[-4000:])
    lines = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0][len("RESULT "):])


def test_two_ranks_on_gloo():
    port = _free_port()
    procs = [_start("forward", "gloo", r, 2, port) for r in range(2)]
    res = [_result(p) for p in procs]
    for r, x in enumerate(res):
        assert x["rank"] == r and x["world"] == 2 and x["backend"] == "gloo"
        assert x["io"]["shard"] == [r, 2] and x["io"]["exchanged_bytes"] > 0
        assert x["out"] == x["want"], r                     # each rank decrypts its own whole copy: the integer circuit's outputs
    assert res[0]["out"] == res[1]["out"]
    assert res[0]["io"]["exchanged_bytes"] == res[1]["io"]["exchanged_bytes"]


def test_one_rank_on_rccl():
    x = _result(_start("loopback", "nccl", 0, 1, _free_port()))
    assert x["backend"] == "nccl"
    assert "shard" not in x["io"]                           # world size 1: forward() takes the plain path
    assert x["out"] == x["want"]
    assert x["view"]["same_memory"] and x["view"]["shape"] == x["view"]["want_shape"] and x["view"]["device"] == "cuda:0"
    assert x["sharded_pass"] == x["out"]                    # the exchange over RCCL, on the session's own memory
