"""The committed (case, seed) list that tests/test_simulate_host.py checks on the host (guard, near_edge emptiness) and
tests/test_gpu_simulate.py runs on the device: circuits, inputs, sigmas and seeds of every comparison of `simulate` with its numpy twin
(tests/simulate_ref.py).  A case is built on demand and its twin result is computed once and shared, read-only."""
import functools

import numpy as np

import simulate_ref as R

U = np.uint64
N_SITE = 4096                                  # elements of a one-site case


class Case:
    """blob; runs: the input phases [B, n_in] of consecutive passes of ONE session (pass j is the twin's run j); sigmas / sigmas2 per op;
    allow_wrap: the one case whose draws may reach half the torus.  inside: per run, must the overflow flag stay clear"""

    def __init__(self, name, blob, runs, seed, sigmas, sigmas2=None, allow_wrap=False, inside=None, info=None):
        self.name, self.blob, self.runs, self.seed, self.sigmas, self.sigmas2 = name, blob, runs, seed, list(sigmas), None if sigmas2 is None else list(sigmas2)
        self.allow_wrap, self.inside, self.info = allow_wrap, inside, info or {}
        self._twin = None

    def twin(self):
        """-> (per run (tensors by id, overflow flag), the trace of every noisy look-up)"""
        if self._twin is None:
            trace, out = R.Trace(self.allow_wrap), []
            for j, ph in enumerate(self.runs):
                vals, ov = R.run_simulate(self.blob, ph, self.seed, self.sigmas, self.sigmas2, run=j, all_tensors=True, trace=trace)
                for v in vals.values():
                    v.setflags(write=False)
                out.append((vals, ov))
            self._twin = (out, trace)
        return self._twin


# ------------------------------------------------------------------------------------------ one-site circuits
SITES = {(6, 0, 6): (0, 0), (8, 2, 6): (3, 1 << 62), (7, 3, 4): (1, 3 << 56), (7, 0, 7): (2, 1 << 62)}      # (p, r, w) -> shift, body offset


def site_sigmas(w, split):
    """2^-4: the wrap across the padding bit is taken often; 2^-(w+2) / 3: rare flips (a split looks up w - 1 bits: a third of THEIR
    half-box too); 2^-40: the noisy path without flips"""
    return [2.0 ** -4, 2.0 ** -(w + 2) / 3.0] + ([2.0 ** -(w + 1) / 3.0] if split else []) + [2.0 ** -40]


def site_inputs(p, r, shift, body_add, rng, inside, n=N_SITE):
    """n inputs x with (x << shift) + body_add = every message with every value of its low r bits, cyclically; the second half of them
    with random bits below the unit.  inside: the messages that stay under the padding bit once the site has added half of what it rounds
    away; else every (p + 1)-bit value, so half of them with the padding bit set"""
    top = (1 << p) - ((1 << (r - 1)) if r else 0) if inside else 1 << (p + 1)
    v = np.resize(np.arange(top, dtype=np.uint64), n) << U(63 - p)
    v[n // 2:] += rng.integers(0, 1 << (63 - p), n - n // 2, dtype=np.uint64)
    return ((v - U(body_add)) >> U(shift)).reshape(1, n)


def _site_case(name, seed, p, r, w, mode, sigma, sigma2=None, n=N_SITE, allow_wrap=False):
    rng = np.random.default_rng(seed)
    shift, body_add = SITES[(p, r, w)]
    tables = rng.integers(-(1 << 62), 1 << 62, (1, 1 << w), dtype=np.int64) << 1          # even: a parity split halves their sums
    blob = R.chain_blob((1, 1, n), [R.lut_record(p, r, w, shift, mode, tables, body_add)])
    runs = [site_inputs(p, r, shift, body_add, rng, True, n), site_inputs(p, r, shift, body_add, rng, False, n)]
    return Case(name, blob, runs, seed, [sigma], None if sigma2 is None else [sigma2], allow_wrap=allow_wrap, inside=[True, False])


def _per_channel_case(name, seed, p, w, mode, sigma):
    """[2, 3, 5, 7] with one table per channel: hw = 35, so the channel boundaries fall inside wavefronts"""
    rng = np.random.default_rng(seed)
    tables = rng.integers(-(1 << 62), 1 << 62, (3, 1 << w), dtype=np.int64) << 1
    blob = R.chain_blob((3, 5, 7), [R.lut_record(p, 0, w, 0, mode, tables, 0)])
    runs = [rng.integers(0, 1 << p, (2, 105), dtype=np.uint64) << U(63 - p) for _ in range(2)]
    return Case(name, blob, runs, seed, [sigma], inside=[True, True])


# ------------------------------------------------------------------------------------------ max pools
POOLS = {"k3s2p1-9x9": ((3, 2, 1), 9, 9), "k3s2p1-7x6": ((3, 2, 1), 7, 6), "k2s2p0-6x6": ((2, 2, 0), 6, 6), "k3s1p1-5x5": ((3, 1, 1), 5, 5),
         "k3s2p1-1x9": ((3, 2, 1), 1, 9), "k3s2p1-9x1": ((3, 2, 1), 9, 1)}      # the last two: the row pass alone, the column pass alone
POOL_E, POOL_PD = 56, 5      # 4-bit values at 2^56, signed 5-bit differences: the compiler's stem pool


def relu_table():
    return np.maximum(np.arange(1 << POOL_PD) - (1 << (POOL_PD - 1)), 0).astype(np.int64) << POOL_E


def _pool_case(name, seed, geom, sigma):
    (k, s, pad), H, W = POOLS[geom]
    rng = np.random.default_rng(seed)
    blob = R.chain_blob((2, H, W), [R.pool_record(k, s, pad, POOL_PD, relu_table(), shift=63 - POOL_PD - POOL_E, body_add=1 << 62)])
    runs = [rng.integers(0, 16, (2, 2 * H * W), dtype=np.uint64) << U(POOL_E) for _ in range(2)]
    return Case(name, blob, runs, seed, [sigma], info=dict(geom=(k, s, pad)))


def _lut_pool_case(name, seed):
    """two records: a noisy 6-bit look-up (values 0 .. 15 out) feeding a noisy pool, so that the pool's streams meet a look-up's"""
    (k, s, pad), H, W = POOLS["k3s2p1-7x6"]
    rng = np.random.default_rng(seed)
    tables = rng.integers(0, 16, (2, 64), dtype=np.int64) << POOL_E
    blob = R.chain_blob((2, H, W), [R.lut_record(6, 0, 6, 0, 0, tables, 0),
                                    R.pool_record(k, s, pad, POOL_PD, relu_table(), shift=63 - POOL_PD - POOL_E, body_add=1 << 62)])
    runs = [rng.integers(0, 64, (2, 2 * H * W), dtype=np.uint64) << U(57) for _ in range(2)]
    return Case(name, blob, runs, seed, [2.0 ** -8 / 3.0, 1.0 / 32])


# ------------------------------------------------------------------------------------------ whole circuits
TRUNKS = {"resnet_exact": dict(), "resnet_approx_p_error": dict(rounding_method="approximate", p_error=0.01, tier_policy="p_error", param_set=None),
          "resnet_rtb7": dict(rounding_threshold_bits=7), "pooled_trunk": dict(img=9, pool1=(3, 2, 1))}
BATCH = 2


@functools.lru_cache(maxsize=None)
def compiled_trunk(which):
    from dctfhe import compile as cc, models, params as P
    kw = dict(TRUNKS[which])
    img, pool1 = kw.pop("img", 6), kw.pop("pool1", None)
    kw.setdefault("param_set", P.test_params())
    calib = np.random.default_rng(3).normal(0, 1, (24, 4, img, img))
    c = cc.compile_model(models.tiny_resnet_q(img_size=img, pool1=pool1), calib[:20], n_bits=5, **kw)
    q = [cc.act_quant(np.asarray(calib[20 + BATCH * j:20 + BATCH * (j + 1)], np.float64), c.in_scale, True, c.in_bits) for j in range(2)]
    return c, [(x.astype(np.int64).astype(np.uint64) << U(c.e_in)).reshape(BATCH, -1) for x in q]


def trunk_sigmas(c, last=2.0 ** -4, pool=None):
    """the compiler's figures with the last look-up raised (the model's own move nothing on the exact tiers); pool: the max pool's too"""
    from dctfhe import compile as cc
    sig, sig2 = list(c.simulation_sigmas()), list(c.simulation_sigmas_split())
    sig[max(i for i, o in enumerate(c.ops) if o.type == cc.OP_LUT)] = last
    if pool is not None:
        for i, o in enumerate(c.ops):
            if o.type == cc.OP_MAXPOOL:
                sig[i] = pool
    return sig, sig2


def _trunk_case(name, seed, which, last=2.0 ** -4, pool=None):
    c, phases = compiled_trunk(which)
    sig, sig2 = trunk_sigmas(c, last, pool)
    return Case(name, c.blob, phases, seed, sig, sig2, info=dict(trunk=which))


# ------------------------------------------------------------------------------------------ the list
def _all():
    out, seed = {}, 20261020

    def add(name, fn, *a, **kw):
        nonlocal seed
        seed += 1
        out[name] = functools.partial(fn, name, SEEDS.get(name, seed), *a, **kw)

    for (p, r, w) in ((6, 0, 6), (8, 2, 6), (7, 3, 4)):
        for mode in (0, 1):
            for j, sg in enumerate(site_sigmas(w, False)):
                add(f"site-p{p}r{r}w{w}-mode{mode}-s{j}", _site_case, p, r, w, mode, sg)
    for mode in (2, 3):
        for j, sg in enumerate(site_sigmas(7, True)):
            add(f"site-p7r0w7-mode{mode}-s{j}", _site_case, 7, 0, 7, mode, sg)
            add(f"site-p7r0w7-mode{mode}-s{j}-second", _site_case, 7, 0, 7, mode, sg, sg / 2)
    add("channels-exact", _per_channel_case, 6, 6, 0, 2.0 ** -4)
    add("channels-split", _per_channel_case, 7, 7, 2, 2.0 ** -4)
    for geom in POOLS:
        add(f"pool-{geom}-noisy", _pool_case, geom, 1.0 / 32)
        add(f"pool-{geom}-quiet", _pool_case, geom, 2.0 ** -40)
    add("lut-then-pool", _lut_pool_case)
    for which in TRUNKS:
        add(f"trunk-{which}", _trunk_case, which)
    # 1/32 of the torus on the pool (the half-box of its 5-bit table is 1/128) moves relu entries; a look-up behind it may then leave its
    # padded range, which the twin flags as the device does
    add("trunk-pooled_trunk-noisy-pool", _trunk_case, "pooled_trunk", pool=1.0 / 32)
    # the reduced draw: at an eighth of the torus |g sigma| reaches 1/2 once in 16 000 draws, so 2^17 elements per run
    add(WRAP_CASE, _site_case, 8, 2, 6, 0, 0.125, n=1 << 17, allow_wrap=True)
    return out


WRAP_CASE = "site-p8r2w6-mode0-eighth"


SEEDS = {}      # name -> seed, where the default one left a draw inside the guard of an edge (tests/test_simulate_host.py says so)
BUILDERS = _all()


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()
