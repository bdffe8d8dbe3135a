"""Digests of what the circuit compiler makes of a fixed set of models: tests/golden/compiled_circuit_digests.json, which
tests/test_compile_digests.py holds dctfhe/compile.py to.  The cases cover the four look-up modes, both hand-overs of the one-bit
steps and a max pool.  Per case the sha256 of: the blob, report(), pbs_counts(), margin_model() and the simulation sigmas with the
expected failures per image (repr of the floats: one ulp moves a digest).  CPU only.
usage: python tools/circuit_digests.py            -> rewrites the fixture from the checked-out compiler
       python tools/circuit_digests.py --check    -> compares, exit status 1 on a difference"""
import argparse
import hashlib
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "dct-cryptonets_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "compiled_circuit_digests.json")
DIGESTS = ("blob", "report", "pbs_counts", "margin_model", "sigmas")

# bench configurations: calibration make_batch(100, 7), seed-0 model, n_bits=5, the catalogue compile_model picks itself
# tiny trunks: models.tiny_resnet_q on params.test_params(), calibration default_rng(seed).normal(0, 1, (n, 4, img, img))
CASES = [
    dict(id="r20_24_16-bw4-rtb6", config="r20_24_16", bit_width=4, rtb=6),
    dict(id="r20_24_16-bw5-rtb6", config="r20_24_16", bit_width=5, rtb=6),
    dict(id="r20_24_16-bw4-rtb7", config="r20_24_16", bit_width=4, rtb=7),
    dict(id="r20_24_16-bw5-rtb7", config="r20_24_16", bit_width=5, rtb=7),
    dict(id="r20_24_16-bw4-approx", config="r20_24_16", bit_width=4, rtb=6, kw=dict(rounding_method="approximate")),
    dict(id="r20_24_16-bw4-p_error-approx", config="r20_24_16", bit_width=4, rtb=6,
         kw=dict(p_error=0.01, tier_policy="p_error", rounding_method="approximate")),
    dict(id="r20_3_32-bw4-rtb6", config="r20_3_32", bit_width=4, rtb=6),
    dict(id="r18_3_32-bw4-rtb6", config="r18_3_32", bit_width=4, rtb=6),
    dict(id="tiny-rtb6", tiny=dict(), rtb=6, seed=0, n=48, img=6),
    dict(id="tiny-rtb7", tiny=dict(), rtb=7, seed=0, n=48, img=6),
    dict(id="tiny-pool-rtb6", tiny=dict(pool1=[3, 2, 1]), rtb=6, seed=0, n=20, img=9),
]


def compile_case(case):
    import bench
    from dctfhe import compile as cc, models, params as P
    kw = dict(case.get("kw", {}))
    if "tiny" in case:
        pool1 = case["tiny"].get("pool1")
        model = models.tiny_resnet_q(img_size=case["img"], pool1=tuple(pool1) if pool1 else None)
        calib = np.random.default_rng(case["seed"]).normal(0, 1, (case["n"], 4, case["img"], case["img"]))
        kw["param_set"] = P.test_params()
    else:
        factory, in_ch, img, make_batch, _ = bench.CONFIGS[case["config"]]
        calib = make_batch(100, 7)
        model = getattr(models, factory)(bit_width=case["bit_width"], in_channels=in_ch, img_size=img, seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cc.compile_model(model, calib, rounding_threshold_bits=case["rtb"], n_bits=5, **kw)


def digests(c):
    texts = dict(blob=c.blob, report=c.report(), pbs_counts=json.dumps(c.pbs_counts(), sort_keys=True), margin_model=repr(c.margin_model()),
                 sigmas=repr((c.simulation_sigmas(), c.simulation_sigmas_split(), c.expected_failures_per_image)))
    return {k: hashlib.sha256(v if isinstance(v, bytes) else v.encode()).hexdigest() for k, v in texts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    rows = []
    for case in CASES:
        rows.append(dict(case=case, **digests(compile_case(case))))
        print(case["id"], rows[-1]["blob"], flush=True)
    if args.check:
        with open(FIXTURE) as f:
            want = json.load(f)
        bad = [(r["case"]["id"], k) for r, w in zip(rows, want) for k in DIGESTS if r[k] != w[k]] + ([("rows", len(rows))] if len(rows) != len(want) else [])
        print("differences:", bad)
        return 1 if bad else 0
    with open(FIXTURE, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
