"""ResNet-18 96x96 crop (the workload of profiles/maxpool_crop96_kernel_stats.txt): one encrypted pass unbudgeted, one under a budget that
divides the stem group at least in two; times, live bytes, equality of the output ciphertexts and with the integer circuit.
Writes profiles/memory_budget_slab_cost.json (or --out).      python tools/memory_budget_profile.py [--out FILE]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dct-cryptonets_amd")]
import numpy as np
import bench
from dctfhe import frontend, models, synthetic
from dctfhe.engine import Session, device_bytes_live
from dctfhe.quantized_module import compile_brevitas_qat_model
from oracle import circuit_ref
tf = frontend.rgb_eval_transform(224)
x = np.stack([tf(im) for im in synthetic.synthetic_images(13, 7)]).astype(np.float32)
model = models.trunk_prefix(models.ResNet18QAT(bit_width=4, in_channels=3, img_size=224), n_blocks=8, avgpool_kernel=3)
x = x[:, :, 64:160, 64:160]
qm = compile_brevitas_qat_model(model, x[:12], n_bits=5, rounding_threshold_bits=6, p_error=0.01)
qm.fhe_circuit.keygen(seed=bench.KEY_SEED)
keys, c = qm._keys, qm.compiled
phases = qm.encode_input(qm.quantize_input(x[12:13]))
ref, overflow = circuit_ref.run_clear(c.blob, phases)
want = qm.decode_output(ref)
seeded = keys.encrypt_seeded(phases.reshape(-1))
free = c.memory_plan(batch=1)
# a budget that divides the stem group at least in two: walk the planner down until the stem's slab is at most half its channels
plan = free
while plan["groups"][0]["slab"] * 2 > plan["groups"][0]["channels"]:
    plan = c.memory_plan(batch=1, budget_bytes=plan["bytes_planned"] - 1)
rec = dict(workload="ResNet-18 3x224^2 RGB weights, all four stages, 96x96 crop, default_params(), one image, encrypted", plans=dict(undivided=free, budgeted=plan), runs=[])
outs = []
for name, budget in (("unbudgeted", None), ("budgeted", plan["bytes_planned"])):
    before = device_bytes_live()
    sess = Session(qm._context(), qm._circuit, keys, 1)
    if budget:
        sess.set_memory_budget(budget)
    sess.upload_seeded(seeded)
    held = device_bytes_live() - before
    t = time.time()
    tm = sess.run(timing=True)
    wall = time.time() - t
    od = sess.dims()[1]
    cts = sess.download(od)
    outs.append(cts)
    got = qm.decode_output(keys.decrypt(cts.reshape(-1, od + 1), od).reshape(1, -1))
    rec["runs"].append(dict(side=name, budget_bytes=budget, session_bytes_live=held, run_ms=tm.total_ms, wall_s=wall, linear_ms=tm.linear_ms, ks_ms=tm.ks_ms,
                            equals_integer_circuit=bool(np.array_equal(got, want)), slabs=[g["slab"] for g in sess.memory_plan()["groups"]]))
    sess.close()
    print(json.dumps(rec["runs"][-1]), flush=True)
rec["output_ciphertexts_equal_word_for_word"] = bool(np.array_equal(outs[0], outs[1]))
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "memory_budget_slab_cost.json")
json.dump(rec, open(out, "w"), indent=1)
print("equal:", rec["output_ciphertexts_equal_word_for_word"])
qm.close()
