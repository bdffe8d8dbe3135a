"""Writes profiles/memory_plan.json: what the session planner (include/dctfhe.h dctfhe_memory_plan) plans for the
RGB ResNet-18 trunks -- the bytes a session allocates for itself, undivided and under a budget, and the slab height of every slab group.
PLAN ARITHMETIC ONLY: it runs on the CPU, allocates nothing on a device and runs no circuit; nothing here says a trunk was evaluated.

    python tools/memory_plan.py [--sizes 224,448,1024] [--batch3 224] [--budget-gb 200] [--out profiles/memory_plan.json]

Per image size: the 64_3_<size> trunk (models.ResNet18QAT, 4 bits, default_params()) compiled on two synthetic calibration images, then
the planner at batch 1; for --batch3 sizes also at batch 3.  A budget the smallest plan exceeds is recorded with the planner's refusal.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="224,448,1024")
    ap.add_argument("--batch3", default="224")
    ap.add_argument("--budget-gb", type=float, default=200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memory_plan.json"))
    args = ap.parse_args()
    from dctfhe import frontend, models, synthetic
    from dctfhe.quantized_module import compile_brevitas_qat_model
    budget = int(args.budget_gb * 1e9)
    batch3 = {int(s) for s in args.batch3.split(",") if s}
    rec = dict(what="dctfhe_memory_plan on the 64_3_<size> ResNet-18 trunks: plan arithmetic on the CPU, nothing was run", budget_bytes=budget, trunks=[])
    for size in [int(s) for s in args.sizes.split(",") if s]:
        tf = frontend.rgb_eval_transform(size)
        calib = np.stack([tf(im) for im in synthetic.synthetic_images(2, 7)]).astype(np.float32)
        t = time.time()
        compiled = compile_brevitas_qat_model(models.ResNet18QAT(bit_width=4, in_channels=3, img_size=size), calib, n_bits=5, rounding_threshold_bits=6,
                                              p_error=0.01).compiled
        compile_s = time.time() - t
        for batch in [1] + ([3] if size in batch3 else []):
            entry = dict(trunk="64_3_%d" % size, batch=batch, compile_seconds=round(compile_s, 1))
            t = time.time()
            free = compiled.memory_plan(batch=batch)
            entry.update(bytes_undivided=free["bytes_undivided"], undivided_fits_budget=free["bytes_undivided"] <= budget)
            try:
                m = compiled.memory_plan(batch=batch, budget_bytes=budget)
                entry.update(bytes_planned=m["bytes_planned"], fits_budget=True, groups=[g for g in m["groups"] if g["slab"] < g["channels"]],
                             n_groups=len(m["groups"]))
            except Exception as e:      # the planner's refusal, in its words
                entry.update(fits_budget=False, refusal=str(e))
            entry["plan_seconds"] = round(time.time() - t, 1)
            rec["trunks"].append(entry)
            print(json.dumps(entry), flush=True)
            with open(args.out, "w") as f:      # after every entry: the large trunks take minutes
                json.dump(rec, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
