"""Noise-model search for the small-key lengths of the exact-evaluation catalogue (dctfhe/params.py::default_params): per group of
tiers that share a key-switch key, the smallest n (steps of 8) that keeps the worst look-up site of the benchmark circuits at the
budget.  The circuits are compiled once (calibration is the slow part); each candidate only re-runs the encoding / tier assignment
and the noise pricing (dctfhe/compile.py::_price).  CPU only.
usage: python tools/param_search.py [--configs r20_24_16,r20_3_32,r18_3_32]   -> the table profiles/r03_param_search.log holds
       python tools/param_search.py --bit-width 5 --configs r20_24_16,r20_3_32,r18_3_32,r18_48_112
           -> the 5-bit catalogue (params.default_params_5bit: its new tiers only), profiles/bw5_param_search.log
       python tools/param_search.py --pool
           -> the quiet pool tier T6p of params.default_params_5bit_pool on the pooled 5-bit trunks (ResNet-18 3x128^2 and 3x224^2,
              rounding_threshold_bits 6 and 7, pool_policy "exact"), profiles/bw5_pool_param_search.log"""
import argparse
import copy
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dct-cryptonets_amd"))
import numpy as np  # noqa: E402

from dctfhe import compile as cc, models, params as P  # noqa: E402

GROUPS = {"table808": ["T6", "T6a", "T5a"], "refresh": ["T4r", "T4r2"], "rescale": ["T4"], "bit": ["B", "Ba", "Ba2"]}
# the 5-bit catalogue keeps the 4-bit tiers as they are; searched: the bit tier of the first rounding steps and the 5-bit refresh
GROUPS_BY_WIDTH = {4: GROUPS, 5: {"bit": ["B"], "refresh5": ["T5r"]}}


def circuits(names, bit_width=4):
    import bench
    out = {}
    for name in names:
        factory, in_ch, img, make_batch, _ = bench.CONFIGS[name]
        t0 = time.time()
        calib = make_batch(16 if name == "r18_48_112" else 100, 7)
        model = getattr(models, factory)(bit_width=bit_width, in_channels=in_ch, img_size=img, seed=0)
        out[name] = cc.compile_model(model, calib, rounding_threshold_bits=6, n_bits=5, p_error=0.01, param_set=P.params_for_bit_width(bit_width))
        print(f"# compiled {name} in {time.time() - t0:.0f} s: worst site {out[name].worst_site_failure:.2e}, expected failures / image "
              f"{out[name].expected_failures_per_image:.2e}", flush=True)
    return out


def with_n(ps, changes, bit_width=4):
    tiers = [dataclasses.replace(t, n=changes.get(t.name, t.n), lwe_sigma=0.0) if t.name in changes else t for t in ps.tiers]
    ref = P.params_for_bit_width(bit_width)
    return dataclasses.replace(ps, tiers=tiers, table_tier_for_w=dict(ref.table_tier_for_w),
                               table_tier_fallback_for_w=dict(ref.table_tier_fallback_for_w))


def price(circs, ps):
    worst, fails, counts = 0.0, {}, {}
    for name, c in circs.items():
        c2 = copy.copy(c)
        c2.tensors = [copy.copy(t) for t in c.tensors]
        c2.ops = [dataclasses.replace(o, lut=copy.copy(o.lut), pool=copy.copy(o.pool)) for o in c.ops]     # the sites pricing writes to
        c2.param_set = copy.deepcopy(ps)
        cc._price(c2)
        worst = max(worst, c2.worst_site_failure)
        fails[name] = c2.expected_failures_per_image
        counts[name] = c2.pbs_counts()
    return worst, fails, counts


def pool_search(budget):
    """T6p's small-key length: the smallest multiple of 8 at which the moved pool and every other site of the pooled 5-bit trunks stay
    within `budget`.  The circuits are compiled once on the shipped catalogue; each candidate prices them again (compile._settle)."""
    base = P.default_params_5bit_pool()
    ti = base.pool_tier_fallback_for_w[6]
    circs = {}
    for img in (128, 224):
        for rtb in (6, 7):
            calib = np.random.default_rng(0).normal(0, 1, (2, 3, img, img))
            c = cc.compile_model(models.ResNet18QAT(bit_width=5, in_channels=3, img_size=img), calib, rounding_threshold_bits=rtb,
                                 param_set=P.default_params_5bit_pool(), pool_policy="exact")
            circs[f"r18_3_{img}_rtb{rtb}"] = c
            pool = next(o for o in c.ops if o.type == cc.OP_MAXPOOL)
            print(f"# compiled r18_3_{img} rtb {rtb}: pool on {c.param_set.tiers[pool.pool.tier].name}, {pool.n_max} pairwise maxima, p_fail "
                  f"{pool.pfail:.2e}; worst site {c.worst_site_failure:.2e}, expected failures / image {c.expected_failures_per_image:.2e}", flush=True)
    t0 = base.tiers[ti]
    print(f"# catalogue as shipped: {t0.name} n={t0.n} k={t0.k} N={t0.N} l={t0.l} beta={t0.beta} lk={t0.lk} betak={t0.betak}")
    print("# per candidate n, the worst over the four circuits: the pool, the look-up that reads it, every site, expected failures per image")
    rows = []
    for n in range(t0.n + 32, t0.n - 41, -8):
        ps = copy.deepcopy(base)
        ps.tiers[ti] = dataclasses.replace(t0, n=n, lwe_sigma=0.0)
        w_pool = w_reader = w_all = 0.0
        fails = {}
        for name, c in circs.items():
            c2 = copy.copy(c)
            c2.tensors = [copy.copy(t) for t in c.tensors]
            c2.ops = [dataclasses.replace(o, lut=copy.copy(o.lut), pool=copy.copy(o.pool)) for o in c.ops]
            c2.param_set = copy.deepcopy(ps)
            cc._settle(c2)
            pool = next(o for o in c2.ops if o.type == cc.OP_MAXPOOL)
            reader = next(o for o in c2.ops if o.type == cc.OP_LUT and o.src0 == pool.dst)
            w_pool, w_reader, w_all = max(w_pool, pool.pfail), max(w_reader, reader.pfail), max(w_all, c2.worst_site_failure)
            fails[name] = c2.expected_failures_per_image
        rows.append((n, w_all))
        print(f"T6p n={n:4d}: pool {w_pool:.2e}  reader {w_reader:.2e}  worst site {w_all:.2e}  expected failures / image "
              + ", ".join(f"{k} {v:.2e}" for k, v in fails.items()), flush=True)
    ok = [n for n, w in rows if w <= budget]
    print(f"# smallest n (steps of 8) with every site <= {budget:.0e}:", min(ok) if ok else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="r20_24_16,r20_3_32,r18_3_32")
    ap.add_argument("--budget", type=float, default=1e-12)
    ap.add_argument("--bit-width", type=int, default=4, choices=sorted(GROUPS_BY_WIDTH))
    ap.add_argument("--pool", action="store_true", help="search the quiet pool tier of the pooled 5-bit trunks instead")
    args = ap.parse_args()
    if args.pool:
        return pool_search(args.budget)
    bw = args.bit_width
    circs = circuits(args.configs.split(","), bw)
    base = P.params_for_bit_width(bw)
    w0, f0, c0 = price(circs, base)
    print(f"# catalogue as shipped: worst site {w0:.2e}; tiers " + ", ".join(f"{t.name} n={t.n}" for t in base.tiers))
    print("# pbs per image:", {k: v for k, v in c0.items()})
    best = {}
    groups = GROUPS_BY_WIDTH[bw]
    for gname, names in groups.items():
        n0 = next(t.n for t in base.tiers if t.name == names[0])
        row = []
        for n in range(n0 + 16, n0 - (49 if bw == 4 else 97), -8):
            w, f, c = price(circs, with_n(base, {nm: n for nm in names}, bw))
            moved = {k: {t: v.get(t, 0) for t in ("B", "Ba", "Ba2", "T4r", "T4r2")} for k, v in c.items()}
            row.append((n, w))
            print(f"{gname:9s} n={n:4d}: worst site {w:.2e}" + ("" if moved == {k: {t: v.get(t, 0) for t in ('B', 'Ba', 'Ba2', 'T4r', 'T4r2')} for k, v in c0.items()} else
                                                                  "   (tier assignment changed: " + str({k: v for k, v in moved.items()}) + ")"), flush=True)
        ok = [n for n, w in row if w <= args.budget]
        best[gname] = min(ok) if ok else n0
    print("# smallest n within the budget, one group at a time:", best)
    allc = {nm: best[g] for g, names in groups.items() for nm in names}
    w, f, c = price(circs, with_n(base, allc, bw))
    print(f"# all groups at once: worst site {w:.2e}, expected failures per image {f}, pbs per image {c}")


if __name__ == "__main__":
    main()
