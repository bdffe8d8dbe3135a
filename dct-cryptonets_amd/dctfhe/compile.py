"""Circuit compiler: float model + calibration batch -> integer circuit for the HIP engine.

Stands in for what `compile_brevitas_qat_model(model.module.feature, calib_data, rounding_threshold_bits,
n_bits, p_error, ...)` does inside Concrete-ML (reference call site homomorphic_eval.py:276-285): import the
quantised graph, fuse every float sub-graph between two integer linear ops into a per-channel table, give
each accumulator a bit-width from the calibration set, and round accumulators to `rounding_threshold_bits`
before their table (exact method, homomorphic_eval.py:279).  Brevitas/Concrete-ML are not available, so
the quantisers are restated here (per-tensor scales from the calibration batch; weights `bit_width`-bit
narrow range as reference models/backbone.py:217-223; activations as :224-227) and the circuit this
produces is the specification the engine and the oracle are both held to.

Circuit semantics (all integers):
  CONV / ADD / SUMPOOL   exact integer arithmetic on message values
  LUT(p, r, w, signed)   idx = m + (2^(p-1) if signed else 0);  t = (idx + 2^(r-1) * [r>0]) >> r;  y = table[channel][t]
  MAXPOOL(k, s, p)       max over the window's in-range taps (torch's -inf padding, floor mode), evaluated as separable
                         row / column passes of pairwise max(a, b) = b + relu(a - b): one signed p_d-bit table per pair
Encodings: a tensor with exponent e holds  phase = value * 2^e  (mod 2^64); a LUT shifts its input up to
e = 63 - p first, so that t sits in the top w+1 bits with the padding bit clear.

A table of 7 input bits is evaluated by a PARITY SPLIT on the 6-bit tiers: one more one-bit step takes the
low bit b0 of t = 2 t' + b0 off the working ciphertext, a second sign bootstrap of the same small ciphertext puts b0 into the
padding bit of a copy, and two 6-bit look-ups give  S[t'] + (-1)^b0 Dt[t'] = T[t]  with  S = (T[2j] + T[2j+1]) / 2,
Dt = T[2j] - S  (split_tables).  The blob keeps one LUT record with w = 7 and the 128-entry tables; the site's mode says how it runs.

Every op carries the typed site of its kind (ConvSite, LutSite, PoolSite: the names and rules of csrc/circuit.h, which decodes what
this module writes).  Which slot of a blob record holds which field is known to _encode_record alone.
"""
import copy
import math
import struct
from dataclasses import dataclass, replace

import numpy as np
import torch
import torch.nn.functional as F

from . import params as P
from .params import KeyTierSelection, key_blob_bytes, key_section_bytes, ksk_owner  # noqa: F401 (tier selections: defined beside the tiers, used here)

OP_CONV, OP_ADD, OP_SUMPOOL, OP_LUT = 1, 2, 3, 4
OP_MAXPOOL = 5            # not 9: the ABI tests use 9 as the unknown type
MAGIC = 0x46544344
# LutSite.mode: how the site is evaluated
LUT_EXACT, LUT_APPROX = 0, 1
LUT_SPLIT = 2             # parity split, both look-ups on the site's table tier
LUT_SPLIT_QUIET = 3       # parity split, the second look-up on the quiet twin: the tier whose key-switch key the table tier shares (ksk_share)


def split_tables(enc):
    """encoded tables [ntab, 2^w] (uint64 / int64 words as the blob stores them) -> (S, Dt) [ntab, 2^(w-1)] uint64 with
    S[j] + Dt[j] = T[2j] and S[j] - Dt[j] = T[2j+1] (mod 2^64): S = ((T[2j] + T[2j+1]) mod 2^64) >> 1, Dt = T[2j] - S.  The engine
    derives the same pair at dctfhe_circuit_load.  An odd sum has no half: ValueError (the consumer's exponent must be >= 1)."""
    t = np.ascontiguousarray(enc).view(np.uint64).reshape(-1, np.asarray(enc).shape[-1])
    with np.errstate(over="ignore"):
        sm = t[:, 0::2] + t[:, 1::2]
        if (sm & np.uint64(1)).any():
            raise ValueError("parity split: a pair of table entries has an odd sum (the table's output exponent must be >= 1)")
        s_ = sm >> np.uint64(1)
        return s_, t[:, 0::2] - s_


# ------------------------------------------------------------------------------------------ quantisers
def weight_quant(w, bits):
    """per-tensor, narrow range (reference backbone.py:217-223: Int8WeightPerTensorFloat, narrow_range=True)"""
    qmax = 2 ** (bits - 1) - 1
    s = float(np.abs(w).max()) / qmax
    if s == 0.0:
        s = 1.0
    return np.clip(np.rint(w / s), -qmax, qmax).astype(np.int64), s


def act_scale(x, signed, bits):
    m = float(np.abs(x).max()) if signed else float(max(x.max(), 0.0))
    if m == 0.0:
        m = 1.0
    return m / ((2 ** (bits - 1) - 1) if signed else (2 ** bits - 1))


from .roles import act_quant          # noqa: E402,F401  (the boundary quantiser: a client needs it without the compiler)


def max_pool_int(q, k, s, p):
    """integer max over the in-range taps of every k x k window (stride s, padding p, floor mode)"""
    B, C, H, W = q.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    lo = np.iinfo(np.int64).min
    qp = np.full((B, C, H + 2 * p, W + 2 * p), lo, np.int64)
    qp[:, :, p:p + H, p:p + W] = q
    out = np.full((B, C, Ho, Wo), lo, np.int64)
    for i in range(k):
        for j in range(k):
            out = np.maximum(out, qp[:, :, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s])
    return out


def pool_taps(n_in, k, s, p):
    """in-range taps of every output of a 1-D pass"""
    n_out = (n_in + 2 * p - k) // s + 1
    return [sum(1 for j in range(k) if 0 <= o * s - p + j < n_in) for o in range(n_out)]


def pool_level_pairs(taps):
    """pairwise maxima per tree level of one 1-D pass.  Late pairing: at level l of L = ceil(log2 max taps), an output with m
    candidates combines max(0, m - 2^(L-l-1)) pairs and carries the rest, so every output reaches one candidate at the last level
    and an output with two taps pairs there (csrc/dctfhe.hip pool_schedule is the same rule)."""
    nmax = max(taps)
    L = (nmax - 1).bit_length()
    m, out = list(taps), []
    for lev in range(L):
        cap = 1 << (L - lev - 1)
        pr = [max(0, x - cap) for x in m]
        out.append(sum(pr))
        m = [x - y for x, y in zip(m, pr)]
    return out


def pool_geometry(C, H, W, k, s, p):
    """[(multiplicity, pairs per level)] of the row pass then the column pass: pairs per image"""
    Wo = (W + 2 * p - k) // s + 1
    return [(C * H, pool_level_pairs(pool_taps(W, k, s, p))), (C * Wo, pool_level_pairs(pool_taps(H, k, s, p)))]


def conv_int(q, w, stride, pad):
    """exact integer convolution (values stay far below 2^53, so float64 is exact)"""
    out = F.conv2d(torch.from_numpy(q.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), stride=stride, padding=pad)
    return np.rint(out.numpy()).astype(np.int64)


def _bn_apply(bn, x):
    sh = (1, -1, 1, 1)
    return bn.gamma.reshape(sh) * (x - bn.mean.reshape(sh)) / np.sqrt(bn.var.reshape(sh) + bn.eps) + bn.beta.reshape(sh)


def _bn_calibrate(bn, x):
    if bn.mean is None:
        bn.mean = x.mean(axis=(0, 2, 3))
        bn.var = x.var(axis=(0, 2, 3))


# ------------------------------------------------------------------------------------------ circuit objects
@dataclass
class TensorInfo:
    C: int
    H: int
    W: int
    e: int = None            # encoding exponent
    lo: int = 0
    hi: int = 0              # guaranteed (tables) or calibrated (accumulators) value range
    var: float = 0.0         # noise variance estimate (torus^2)
    deff: int = 0            # mask words beyond this index are zero (nested keys: a bootstrap output of ring k*N has a zero tail)


@dataclass
class ConvSite:
    Cout: int
    KH: int
    KW: int
    stride: int
    pad: int


@dataclass
class LutSite:
    """one look-up: p-bit accumulator, r bits rounded away, w = p - r table bits (csrc/circuit.h LutSite and StepTiers hold the same rules)"""
    p: int
    r: int
    w: int
    signed: bool
    ntab: int                 # tables: 1, or one per channel
    body_add: int             # added to the shifted body: 2^62 puts a signed value's index at m + 2^(p-1)
    shift: int = 0            # from the input's encoding up to 63 - p
    mode: int = LUT_EXACT
    tab_tier: int = -1
    bit_tier: int = -1        # one-bit step i runs here ...
    coarse: int = -1          # ... from step coarse_from on, on the one-level twin ...
    coarse_from: int = 0
    coarse2: int = -1         # ... and from step coarse2_from on, on the two-bit-rotation twin (< 0: no hand-over)
    coarse2_from: int = 0

    def split(self): return self.mode in (LUT_SPLIT, LUT_SPLIT_QUIET)
    def approx(self): return self.mode == LUT_APPROX
    def table_bits(self): return self.w - 1 if self.split() else self.w

    def n_steps(self):
        """one-bit steps: the r rounding steps, plus the step that takes the parity bit off a split site; none when the table rounds"""
        return 0 if self.approx() else self.r + (1 if self.split() else 0)

    def step_tier(self, i):
        if self.coarse2 >= 0 and i >= self.coarse2_from:
            return self.coarse2
        return self.coarse if (self.coarse >= 0 and i >= self.coarse_from) else self.bit_tier

    def tier2(self, ps):
        """tier of a split's second look-up"""
        return ps.tiers[self.tab_tier].ksk_share if self.mode == LUT_SPLIT_QUIET else self.tab_tier


@dataclass
class PoolSite:
    k: int
    stride: int
    pad: int
    p_d: int                  # bits of the signed difference of two operands: the relu table's input
    body_add: int
    pool_geom: list           # [(multiplicity, pairs per level)] per pass (pool_geometry)
    n_max: int                # pairwise maxima per image
    levels: int               # tree levels of both passes
    shift: int = 0            # of the differences, up to 63 - p_d
    tier: int = -1            # of the relu table
    quiet: bool = False       # moved to the catalogue's quiet pool tier (ParamSet.pool_tier_fallback_for_w; pool_policy "exact")


@dataclass
class OpInfo:
    type: int
    src0: int
    src1: int
    dst: int
    conv: ConvSite = None             # the site of the op's type (OP_ADD has none; OP_SUMPOOL: its window sum_k)
    lut: LutSite = None
    pool: PoolSite = None
    sum_k: int = 0
    deff_in: int = 0                  # effective dimension of what the op reads (mask words beyond it are zero)
    payload: np.ndarray = None
    table_values: np.ndarray = None   # [ntab, 2^w] integer outputs (before encoding)
    nu2: float = 1.0
    note: str = ""
    pfail: float = 0.0
    sim_sigma: float = 0.0            # modelled noise std at the input of the site's table bootstrap (fraction of the torus)
    sim_sigma2: float = 0.0           # parity-split sites: the same at the second look-up (one more bit-tier output on its input)
    margin: list = None               # margin audit: the variance _estimate_noise priced every bootstrap with a key switch of its own at

    # what a look-up reads, for either kind of table site (a max pool looks its p_d-bit differences up unrounded)
    p = property(lambda o: o.lut.p if o.lut else o.pool.p_d if o.pool else 0)
    r = property(lambda o: o.lut.r if o.lut else 0)
    w = property(lambda o: o.lut.w if o.lut else o.pool.p_d if o.pool else 0)
    signed = property(lambda o: o.lut.signed if o.lut else o.pool is not None)
    n_max = property(lambda o: o.pool.n_max)
    # the blob record, for readers that count in slots (bench.py, the tests): encoded on demand, never written
    ip = property(lambda o: _encode_record(o)[0])
    lp = property(lambda o: _encode_record(o)[1])


def for_each_bootstrap(o, ps):
    """The bootstraps one element of op `o` takes, in execution order (csrc/circuit.h for_each_bootstrap): (kind, tier, table_bits,
    own_keyswitch).  Look-up: the one-bit steps; for a split the parity bootstrap, on the last step's small ciphertext, and the second
    look-up; the table.  Max pool: one relu bootstrap per pairwise maximum.  Nothing for the levelled ops."""
    if o.type == OP_LUT:
        L, n = o.lut, o.lut.n_steps()
        for i in range(n):
            yield f"step {i}", L.step_tier(i), 0, True
        if L.split():
            yield "parity", L.step_tier(n - 1), 0, False
            yield "second", L.tier2(ps), L.w - 1, True
        yield "table", L.tab_tier, L.table_bits(), True
    elif o.type == OP_MAXPOOL:
        yield "pool", o.pool.tier, o.pool.p_d, True


@dataclass
class CompiledCircuit:
    tensors: list
    ops: list
    input_tensor: int
    output_tensor: int
    in_scale: float
    in_bits: int
    out_scale: float
    out_bits: int
    max_bit_width: int
    param_set: object
    rounding_threshold_bits: int
    n_bits: int
    blob: bytes = b""
    expected_failures_per_image: float = 0.0
    rounding_method: str = "exact"
    expected_boundary_flips_per_image: float = 0.0    # approximate rounding only
    tier_policy: str = "exact"
    pool_policy: str = "coarse"
    calib_out: np.ndarray = None                      # the compile-time integer forward: outputs [B, n_out] on the calibration batch

    @property
    def e_in(self):
        return self.tensors[self.input_tensor].e

    @property
    def e_out(self):
        return self.tensors[self.output_tensor].e

    def n_in(self):
        t = self.tensors[self.input_tensor]
        return t.C * t.H * t.W

    def n_out(self):
        t = self.tensors[self.output_tensor]
        return t.C * t.H * t.W

    @property
    def worst_site_failure(self):
        """largest modelled failure probability per element over the look-up sites (a max pool: per pairwise maximum)"""
        return max((o.pfail for o in self.ops if o.type in (OP_LUT, OP_MAXPOOL)), default=0.0)

    def simulation_sigmas(self):
        """per op, the noise std `simulate` injects at the look-up (0 for the levelled ops)"""
        return [o.sim_sigma if o.type in (OP_LUT, OP_MAXPOOL) else 0.0 for o in self.ops]

    def simulation_sigmas_split(self):
        """per op, the noise std `simulate` injects at the SECOND look-up of a parity-split site (0 elsewhere)"""
        return [o.sim_sigma2 if (o.type == OP_LUT and o.lut.split()) else 0.0 for o in self.ops]

    def margin_model(self):
        """One record per slot of the margin audit (include/dctfhe.h dctfhe_session_audit), in the same enumeration: per look-up op its
        one-bit steps, for a parity split the second look-up, then the table; one record per max pool (its worst tree level).  The
        parity bootstrap has no key switch of its own and no record.  sigma (fraction of the torus) is the very figure _estimate_noise
        put into p_fail for that decision.  elements: decisions per image."""
        ps, out = self.param_set, []
        for i, o in enumerate(self.ops):
            boots = [b for b in for_each_bootstrap(o, ps) if b[3]]
            for e, ((kind, tier, bits, _), var) in enumerate(zip(boots, o.margin or [])):
                out.append(dict(op=i, entry=e, kind=kind, tier=tier, tier_name=ps.tiers[tier].name, table_bits=bits, elements=self._decisions(o),
                                sigma=math.sqrt(var), note=o.note))
        return out

    def _decisions(self, o):
        """bootstraps per image and entry of for_each_bootstrap"""
        s = self.tensors[o.src0]
        return o.pool.n_max if o.type == OP_MAXPOOL else s.C * s.H * s.W

    def pbs_counts(self):
        """{tier name: programmable bootstraps per image} -- table lookups on the site's table tier, rounding steps
        on the bit tier (steps below coarse_from) or the one-level bit tier (steps from coarse_from on)."""
        ps, out = self.param_set, {}
        for o in self.ops:
            boots = list(for_each_bootstrap(o, ps))
            for _, tier, _, _ in boots[-1:] + boots[:-1]:      # a site's table first: the order in which the tier names appear
                nm = ps.tiers[tier].name
                out[nm] = out.get(nm, 0) + self._decisions(o)
        return out

    def key_tiers(self, output=None, spec=None):
        """The evaluation keys this circuit reads, as a closed tier selection (include/dctfhe.h TIER SELECTIONS; the library's
        dctfhe_key_tiers_for_circuit computes the same from the blob): the bootstrap key of every tier an op bootstraps on and the
        key-switch key at the end of that tier's share chain.  output "rows" / "ring": plus the key-switch key of the tier that
        output_compaction(self, output, spec) picks, so that packed results under the pruned keys are those under the full set."""
        ps = self.param_set
        bsk = ksk = 0
        for o in self.ops:
            if o.type not in (OP_LUT, OP_MAXPOOL) or self._decisions(o) <= 0:
                continue
            for _, tier, _, _ in for_each_bootstrap(o, ps):
                bsk |= 1 << tier
                ksk |= 1 << ksk_owner(ps, tier)
        if output is not None:
            ksk |= 1 << output_compaction(self, output, spec).tier
        return KeyTierSelection.from_masks(ps, bsk, ksk)

    def key_report(self, output=None, spec=None):
        """Per tier: which of its keys key_tiers(output, spec) keeps and the bytes of each in the two blob forms (full: the Fourier
        bootstrap key and the whole key-switch key; compressed: their bodies), with the totals of the blobs for every tier and for the
        selection (header, public generator key and masks included: the figures of dctfhe_key_tiers_blob_bytes)."""
        ps, sel = self.param_set, self.key_tiers(output, spec)
        tiers = []
        for i, t in enumerate(ps.tiers):
            b = key_section_bytes(ps, t)
            tiers.append(dict(tier=i, name=t.name, bsk=t.name in sel.bsk, ksk=t.name in sel.ksk, ksk_owner=ps.tiers[ksk_owner(ps, i)].name,
                              bootstraps_per_image=self.pbs_counts().get(t.name, 0), **b))
        every = KeyTierSelection.all(ps)
        return dict(tiers=tiers, selection=dict(bsk=sorted(sel.bsk), ksk=sorted(sel.ksk), bsk_mask=sel.bsk_mask, ksk_mask=sel.ksk_mask),
                    all=dict(full_bytes=key_blob_bytes(ps, every, False), compressed_bytes=key_blob_bytes(ps, every, True)),
                    selected=dict(full_bytes=key_blob_bytes(ps, sel, False), compressed_bytes=key_blob_bytes(ps, sel, True)))

    def shard_plan(self, rows=False, part=0, parts=1, batch=1):
        """The exchange points of a run whose look-up sites are sharded over several GPUs (include/dctfhe.h dctfhe_session_shard_plan, the
        same list): [(after_op, tensor)] in op order.  Look-ups and adds run on a part's rows and leave their output sliced; convolutions,
        pools and the download read whole tensors -- so every sliced tensor one of them reads is exchanged once, right after the op that
        writes it.  A tensor read by adds and look-ups only never travels.  The plan depends on the circuit alone.

        rows=True: the plan of a run whose max pools are divided too (Configuration(shard_pool=True); dctfhe_session_shard_plan_rows of
        a session with dctfhe_session_set_shard_pool on), for part `part` of `parts` and `batch` images: [(after_op, tensor, first,
        count)].  A divided pool leaves its destination sliced and needs only its need range of the source (shard_pool); every other
        entry carries (0, rows of the tensor).  A tensor that a pool and another whole-needing op read travels whole."""
        state, writer, plan = [2] * len(self.tensors), {}, []      # 0: sliced, 1: a pool's need range is there, 2: whole

        def need(t, reader):
            if state[t] == 0:
                plan.append([writer[t], t, reader])
            elif state[t] == 1:
                for e in plan:
                    if e[0] == writer[t] and e[1] == t:
                        e[2] = -1
                reader = -1
            state[t] = max(state[t], 2 if reader < 0 else 1)
        for i, o in enumerate(self.ops):
            if o.type in (OP_LUT, OP_ADD):
                state[o.dst], writer[o.dst] = 0, i
                continue
            part_only = rows and parts > 1 and o.type == OP_MAXPOOL
            need(o.src0, i if part_only else -1)
            state[o.dst], writer[o.dst] = (0 if part_only else 2), i
        need(self.output_tensor, -1)
        plan.sort(key=lambda e: (e[0], e[1]))
        if not rows:
            return [(a, t) for a, t, _ in plan]
        out = []
        for a, t, reader in plan:
            T = self.tensors[t]
            if reader < 0:
                out.append((a, t, 0, batch * T.C * T.H * T.W))
            else:
                S = self.ops[reader].pool
                out.append((a, t) + shard_pool(batch, T.C, T.H, T.W, S.k, S.stride, S.pad, parts, part)[2:4])
        return out

    def memory_plan(self, params=None, batch=1, budget_bytes=None):
        """The session planner's record for this circuit (include/dctfhe.h dctfhe_memory_plan -- the library's planner, not a restatement):
        {bytes_undivided, bytes_planned, budget_bytes, ..., groups: [{first_op, end_op, channels, slab}]}.  params: a parameter set
        (default: the circuit's own), or False for a clear-mode session.  Host only: no GPU."""
        from .engine import memory_plan
        ps = self.param_set if params is None else params
        cp = None if ps is False else (ps if hasattr(ps, "_fields_") else P.to_c_params(ps))
        return memory_plan(self.blob, cp, batch, budget_bytes)

    def report(self, memory_budget_bytes=None, batch=1):
        """Text dump standing in for `fhe_circuit.mlir` (reference homomorphic_eval.py:309-311).  memory_budget_bytes: also the planned
        session bytes and slab heights under that budget (memory_plan)."""
        names = {OP_CONV: "conv2d", OP_ADD: "add", OP_SUMPOOL: "sum_pool", OP_LUT: "round_lut", OP_MAXPOOL: "max_pool2d"}
        ps = self.param_set
        lines = [f"// dctfhe circuit: {len(self.ops)} ops, max accumulator bit-width {self.max_bit_width}, D={ps.D}"]
        for i, t in enumerate(ps.tiers):
            lines.append(f"// tier {i} {t.name}: n={t.n} k={t.k} N={t.N} l={t.l} beta={t.beta} lk={t.lk} betak={t.betak} "
                         f"sigma_lwe=2^{math.log2(t.lwe_sigma):.1f} sigma_glwe=2^{math.log2(t.glwe_sigma):.1f}")
        for i, o in enumerate(self.ops):
            s, d = self.tensors[o.src0], self.tensors[o.dst]
            head = f"%{o.dst} = {names[o.type]}(%{o.src0}" + (f", %{o.src1}" if o.type == OP_ADD else "") + ")"
            if o.type == OP_CONV:
                head += f" {{cout={o.conv.Cout}, k={o.conv.KH}x{o.conv.KW}, stride={o.conv.stride}, pad={o.conv.pad}, nu2={o.nu2:.0f}}}"
            elif o.type == OP_SUMPOOL:
                head += f" {{k={o.sum_k}}}"
            elif o.type == OP_MAXPOOL:
                S = o.pool
                head = (f"%{o.dst} = max_pool2d(%{o.src0}, {S.k}, {S.stride}, {S.pad}) {{p_d={S.p_d}, shift={S.shift}, "
                        f"tier={ps.tiers[S.tier].name}, levels={S.levels}, pairwise_max={S.n_max}, p_fail/max={o.pfail:.1e}}}  // {o.note}")
            elif o.type == OP_LUT:
                L, nst, tab = o.lut, o.lut.n_steps(), ps.tiers[o.lut.tab_tier].name
                head += (f" {{p={L.p}, lsbs_removed={L.r}, table_bits={L.w}, signed={int(L.signed)}, shift={L.shift}, "
                         f"tier={tab}" + (", rounding=approximate" if L.approx() else "") +
                         (f", parity_split={tab}+{ps.tiers[L.tier2(ps)].name}, steps={L.r}+1" if L.split() else "") +
                         (f", bit_tier={ps.tiers[L.bit_tier].name}" if nst else "") +
                         (f", steps>={L.coarse_from}:{ps.tiers[L.coarse].name}" if (nst and L.coarse >= 0 and L.coarse_from < nst) else "") +
                         (f", steps>={L.coarse2_from}:{ps.tiers[L.coarse2].name}" if (nst and L.coarse2 >= 0 and L.coarse2_from < nst) else "") +
                         f", tables={L.ntab}, p_fail/elt={o.pfail:.1e}}}  // {o.note}")
            lines.append(f"{head} : [{s.C}x{s.H}x{s.W}] -> [{d.C}x{d.H}x{d.W}] e={d.e}")
        lines.append(f"// expected table failures per image (noise model): {self.expected_failures_per_image:.2e}")
        if self.rounding_method == "approximate":
            lines.append(f"// approximate rounding: expected boundary flips per image: {self.expected_boundary_flips_per_image:.2e}")
        if memory_budget_bytes:
            m = self.memory_plan(batch=batch, budget_bytes=memory_budget_bytes)
            lines.append(f"// device memory budget {memory_budget_bytes} bytes, batch {batch}: planned {m['bytes_planned']} bytes (undivided {m['bytes_undivided']})")
            for g in m["groups"]:
                lines.append(f"//   slab group ops [{g['first_op']}, {g['end_op']}): {g['slab']} of {g['channels']} channels at a time")
        return "\n".join(lines)


def shard_rows(rows, parts, part):
    """(first, count) of the rows part `part` of `parts` owns in a tensor of `rows` rows (include/dctfhe.h dctfhe_shard_rows, the same
    rule): q = rows // parts, r = rows % parts; part p owns q + (p < r) consecutive rows from p q + min(p, r).  Empty parts are legal."""
    rows, parts, part = int(rows), int(parts), int(part)
    if rows < 0 or not 1 <= parts <= 64 or not 0 <= part < parts:
        raise ValueError(f"shard_rows: part {part} of {parts} (1 .. 64 parts) of {rows} rows")
    q, r = divmod(rows, parts)
    return part * q + min(part, r), q + (1 if part < r else 0)


def shard_pool(batch, C, H, W, k, s, pad, parts, part):
    """Part `part` of `parts` of a divided max pool over [batch][C][H][W] (include/dctfhe.h dctfhe_shard_pool, the same rule) ->
    (out_first, out_count, in_first, in_count, pairs).  The part owns the output rows shard_rows gives it over the flat [B][C][Ho][Wo]
    order.  Its intermediates are the row-pass results (b, c, y, xo) under the column windows of these outputs; the need range is the
    smallest contiguous range of source rows holding every tap of theirs; pairs counts a pairwise maximum per tap but the first of every
    intermediate and every output -- late pairing (pool_level_pairs) spends exactly taps - 1 on a window however it pairs.  An empty part
    needs nothing; parts = 1 is the undivided op, which computes every row-pass result, read by a window or not."""
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    n_out = batch * C * Ho * Wo
    o0, on = shard_rows(n_out, parts, part)
    tw, th = np.array(pool_taps(W, k, s, pad), np.int64), np.array(pool_taps(H, k, s, pad), np.int64)
    if parts == 1:
        return 0, n_out, 0, batch * C * H * W, int(batch * C * (H * (tw - 1).sum() + Wo * (th - 1).sum()))
    if on == 0:
        return o0, 0, 0, 0, 0
    e = np.arange(o0, o0 + on, dtype=np.int64)
    xo, yo, bc = e % Wo, (e // Wo) % Ho, e // (Wo * Ho)
    y = yo[:, None] * s - pad + np.arange(k)[None, :]
    mids = np.unique(((bc[:, None] * H + y) * Wo + xo[:, None])[(y >= 0) & (y < H)])
    pairs = int((th[yo] - 1).sum() + (tw[mids % Wo] - 1).sum())
    first = (mids[0] // Wo) * W + max(0, (mids[0] % Wo) * s - pad)
    last = (mids[-1] // Wo) * W + min(W - 1, (mids[-1] % Wo) * s - pad + k - 1)
    return o0, on, int(first), int(last - first + 1), pairs


@dataclass
class OutputCompaction:
    """how a circuit's results travel packed (include/dctfhe.h dctfhe_session_download_packed): key-switched to `tier`, 16 bits per word"""
    tier: int
    name: str
    n: int
    bytes_per_ciphertext: int      # 2 (n + 1)
    var: float                     # what the key switch and the 16-bit rounding add (torus^2)
    pfail: float                   # per result, against the decode margin 2^-(out_bits + 3)


@dataclass
class RingCompaction:
    """how a circuit's results travel ring-packed (include/dctfhe.h dctfhe_session_download_ring): key-switched to `tier`, then up to
    spec.N of them in one GLWE ciphertext of 16-bit words"""
    tier: int
    name: str
    n: int
    spec: object                   # params.PackSpec
    var: float                     # what the key switch and the ring pack (full group) add (torus^2)
    pfail: float                   # per result, against the decode margin 2^-(out_bits + 3)
    results_per_image: int

    def bytes_per_batch(self, batch=1):
        return 2 * self.spec.words(batch * self.results_per_image)


def _ring_compaction(circ, spec):
    ps, out = circ.param_set, circ.tensors[circ.output_tensor]
    spec = spec if spec is not None else P.default_pack_spec(ps)
    if spec.N > ps.D:
        raise ValueError(f"ring packing: the ring key is a prefix of the big key, N_p = {spec.N} > D = {ps.D}")
    deff = out.deff or ps.D
    var, ti = min((P.var_keyswitch(deff, t) + P.var_ring_pack(t.n, spec), i) for i, t in enumerate(ps.tiers) if t.ksk_share < 0)
    t = ps.tiers[ti]
    margin = 2.0 ** -(circ.out_bits + 3)
    pfail = P.p_fail(margin, out.var + var)
    budget = getattr(ps, "p_budget", 1e-12)
    if pfail > budget:
        raise ValueError(f"ring-packed results leave the budget: best tier {t.name} (n = {t.n}) adds sigma 2^{0.5 * math.log2(var):.1f} (ring pack alone "
                         f"2^{0.5 * math.log2(P.var_ring_pack(t.n, spec)):.1f}) to an output of sigma 2^{0.5 * math.log2(max(out.var, 2.0 ** -128)):.1f} at "
                         f"effective dimension {deff}; margin 2^-{circ.out_bits + 3}, p_fail {pfail:.1e} per result > {budget:.1e}")
    return RingCompaction(tier=ti, name=t.name, n=t.n, spec=spec, var=var, pfail=pfail, results_per_image=circ.n_out())


def output_compaction(circ, form="rows", spec=None):
    """The tier whose key-switch key packs this circuit's results: among the tiers that own one (ksk_share < 0), the least
    var_keyswitch(deff_out, t) + var_round16(t.n).  Raises ValueError when a packed result would leave the catalogue's failure budget.
    form="ring": the same choice with var_ring_pack(t.n, spec) in place of the row rounding (spec: a params.PackSpec, default
    params.default_pack_spec) -> RingCompaction."""
    if form == "ring":
        return _ring_compaction(circ, spec)
    if form != "rows":
        raise ValueError(f"output compaction form {form!r} (rows or ring)")
    ps, out = circ.param_set, circ.tensors[circ.output_tensor]
    deff = out.deff or ps.D
    var, ti = min((P.var_keyswitch(deff, t) + P.var_round16(t.n), i) for i, t in enumerate(ps.tiers) if t.ksk_share < 0)
    t = ps.tiers[ti]
    margin = 2.0 ** -(circ.out_bits + 3)
    pfail = P.p_fail(margin, out.var + var)
    budget = getattr(ps, "p_budget", 1e-12)
    if pfail > budget:
        raise ValueError(f"packed results leave the budget: best tier {t.name} (n = {t.n}) adds sigma 2^{0.5 * math.log2(var):.1f} to an output of "
                         f"sigma 2^{0.5 * math.log2(max(out.var, 2.0 ** -128)):.1f} at effective dimension {deff}; margin 2^-{circ.out_bits + 3}, "
                         f"p_fail {pfail:.1e} per result > {budget:.1e}")
    return OutputCompaction(tier=ti, name=t.name, n=t.n, bytes_per_ciphertext=2 * (t.n + 1), var=var, pfail=pfail)


# the site's own rules, for callers that hold a look-up op
@dataclass
class PublicInputPlan:
    """what public-key inputs (include/dctfhe.h dctfhe_encrypt_public) cost a circuit: the variance an extracted input carries in place
    of a fresh encryption's, and the circuit priced again with it -- hand-over steps and tiers as compiled"""
    spec: object                   # params.PublicInputSpec
    var: float                     # params.var_public_input(spec) (torus^2)
    worst_site: int                # op index of the look-up site with the largest p_fail per element (-1: the circuit has none)
    worst_note: str
    worst_pfail: float
    worst_pfail_fresh: float       # the same site with fresh secret-key inputs
    expected_failures_per_image: float
    inputs_per_image: int
    bytes_per_image: int           # wire words of ONE image's inputs, 8 bytes each (a batch shares groups: bytes_per_batch)

    def bytes_per_batch(self, batch=1):
        return 8 * self.spec.words(batch * self.inputs_per_image)


def public_input_plan(circ, spec=None):
    """Prices `circ` with its input tensor's variance replaced by params.var_public_input(spec) (spec: a params.PublicInputSpec, default
    params.default_public_input_spec) on a COPY: circ, its blob and report() stay as they are.  Raises ValueError, with the numbers, when
    the ring does not fit the circuit's inputs or when a site that met p_budget with fresh inputs no longer does."""
    ps = circ.param_set
    spec = spec if spec is not None else P.default_public_input_spec(ps)
    spec.check(ps)
    var = P.var_public_input(spec)
    c = copy.copy(circ)
    c.tensors = [copy.copy(t) for t in circ.tensors]
    c.ops = [copy.copy(o) for o in circ.ops]
    _estimate_noise(c, input_var=var, settle=False)
    budget = getattr(ps, "p_budget", 1e-12)
    sites = [(o.pfail, i) for i, o in enumerate(c.ops) if o.type in (OP_LUT, OP_MAXPOOL)]
    lost = [(pf, i) for pf, i in sites if pf > budget and circ.ops[i].pfail <= budget]
    if lost:
        pf, i = max(lost)
        raise ValueError(f"public-key inputs leave the budget: an extracted input has sigma 2^{0.5 * math.log2(var):.1f} (N_e = {spec.N}, key and "
                         f"encryptor noise 2^{math.log2(spec.sigma):.1f}) against 2^{math.log2(ps.input_sigma):.1f} fresh; {len(lost)} site(s) "
                         f"leave p_budget, the worst op {i} ({circ.ops[i].note}): p_fail {pf:.1e} per element > {budget:.1e} "
                         f"(fresh inputs: {circ.ops[i].pfail:.1e})")
    pf, i = max(sites) if sites else (0.0, -1)
    return PublicInputPlan(spec=spec, var=var, worst_site=i, worst_note=circ.ops[i].note if i >= 0 else "", worst_pfail=pf,
                           worst_pfail_fresh=circ.ops[i].pfail if i >= 0 else 0.0, expected_failures_per_image=c.expected_failures_per_image,
                           inputs_per_image=circ.n_in(), bytes_per_image=8 * spec.words(circ.n_in()))


def step_tier(o, i): return o.lut.step_tier(i)
def is_split(o): return o.lut.split()
def chain_steps(o): return o.lut.n_steps()
def second_tier(ps, o): return o.lut.tier2(ps)


class _Act:
    """integer activation during compilation: calibration values, scale, circuit tensor id, guaranteed range"""

    def __init__(self, q, scale, tid, lo, hi):
        self.q, self.scale, self.tid, self.lo, self.hi = q, scale, tid, lo, hi


def _acc_precision(lo, hi, rtb, margin):
    """smallest (p, r, signed) whose padded range holds [lo, hi] (widened by margin) after rounding"""
    lo = int(math.floor(lo * (1 + margin))) if lo < 0 else int(lo)
    hi = int(math.ceil(hi * (1 + margin)))
    signed = lo < 0
    for p in range(1, 40):
        r = max(0, p - rtb)
        half = (1 << (r - 1)) if r > 0 else 0
        if signed:
            ok = -(1 << (p - 1)) <= lo and hi + half <= (1 << (p - 1)) - 1
        else:
            ok = hi + half <= (1 << p) - 1
        if ok:
            return p, r, signed
    raise ValueError("accumulator range too wide")


def lut_index(m, p, r, signed):
    idx = m + ((1 << (p - 1)) if signed else 0)
    if r > 0:
        idx = (idx + (1 << (r - 1))) >> r
    return idx


def lut_centers(p, r, w, signed):
    """accumulator value each table entry stands for"""
    return (np.arange(1 << w, dtype=np.int64) << r) - ((1 << (p - 1)) if signed else 0)


class _Builder:
    def __init__(self, ps, rtb, margin):
        self.ps, self.rtb, self.margin = ps, rtb, margin
        self.tensors, self.ops = [], []
        self.max_bits = 0

    def tensor(self, C, H, W, lo, hi):
        self.tensors.append(TensorInfo(C, H, W, None, lo, hi))
        return len(self.tensors) - 1

    def conv(self, a, layer, bits):
        wq, sw = weight_quant(layer.weight, bits)
        acc = conv_int(a.q, wq, layer.stride, layer.pad)
        Cout, _, KH, KW = wq.shape
        tid = self.tensor(Cout, acc.shape[2], acc.shape[3], int(acc.min()), int(acc.max()))
        op = OpInfo(OP_CONV, a.tid, -1, tid, conv=ConvSite(Cout, KH, KW, layer.stride, layer.pad), payload=wq.astype(np.int8))
        op.nu2 = float((wq.astype(np.float64) ** 2).sum(axis=(1, 2, 3)).max())
        self.ops.append(op)
        return _Act(acc, a.scale * sw, tid, int(acc.min()), int(acc.max()))

    def add(self, a, b):
        q = a.q + b.q
        tid = self.tensor(*q.shape[1:], a.lo + b.lo, a.hi + b.hi)
        self.ops.append(OpInfo(OP_ADD, a.tid, b.tid, tid))
        return _Act(q, a.scale, tid, a.lo + b.lo, a.hi + b.hi)

    def sum_pool(self, a, K):
        B, C, H, W = a.q.shape
        Ho, Wo = H // K, W // K     # floor mode drops the border (reference backbone.py:276 nn.AvgPool2d)
        q = a.q[:, :, :Ho * K, :Wo * K].reshape(B, C, Ho, K, Wo, K).sum(axis=(3, 5))
        tid = self.tensor(C, Ho, Wo, a.lo * K * K, a.hi * K * K)
        self.ops.append(OpInfo(OP_SUMPOOL, a.tid, -1, tid, sum_k=K))
        return _Act(q, a.scale, tid, a.lo * K * K, a.hi * K * K)

    def max_pool(self, a, k, s, p, note):
        """stem MaxPool2d(k, s, p) on the integers of a table's output (guaranteed range [lo, hi])"""
        q = max_pool_int(a.q, k, s, p)
        _, C, H, W = a.q.shape
        tid = self.tensor(C, q.shape[2], q.shape[3], a.lo, a.hi)
        p_d = max(1, (a.hi - a.lo).bit_length()) + 1               # the signed difference of two operands
        geom = pool_geometry(C, H, W, k, s, p)
        site = PoolSite(k, s, p, p_d, body_add=1 << 62,            # signed body offset: index = d + 2^(p_d - 1)
                        pool_geom=geom, n_max=sum(m * sum(pl) for m, pl in geom), levels=sum(len(pl) for _, pl in geom))
        centres = lut_centers(p_d, 0, p_d, True)
        self.ops.append(OpInfo(OP_MAXPOOL, a.tid, -1, tid, pool=site, note=note,
                               table_values=np.maximum(centres, 0).reshape(1, -1)))     # relu(d): max(a, b) = b + relu(a - b)
        return _Act(q, a.scale, tid, a.lo, a.hi)

    def lut_to_conv(self, a, fn, per_channel, rounding, out_scale, note):
        """table site whose output feeds a convolution; wide sites are split into a cheap noisy look-up followed by an
        identity 'refresh' bootstrap on a small ring (ParamSet.refresh_min_w)"""
        y = self.lut(a, fn, per_channel, rounding, out_scale, note)
        if self.ps.refresh_min_w is not None and self.ops[-1].lut.w >= self.ps.refresh_min_w:
            y = self.lut(y, lambda vals: vals, False, False, out_scale, note + " (refresh)")
        return y

    def lut(self, a, fn, per_channel, rounding, out_scale, note):
        """fn(values[ntab or 1, n]) -> integer outputs; values are message values of `a` (ints).
        rounding=True: `a` is an accumulator, calibrated range + rounding to rtb bits;
        rounding=False: `a` has a guaranteed range, table covers it exactly."""
        C = a.q.shape[1]
        if rounding:
            p, r, signed = _acc_precision(int(a.q.min()), int(a.q.max()), self.rtb, self.margin)
        else:
            p, r, signed = _acc_precision(a.lo, a.hi, 64, 0.0)
        w = p - r
        self.max_bits = max(self.max_bits, p)
        centers = lut_centers(p, r, w, signed)
        ntab = C if per_channel else 1
        vals = np.broadcast_to(centers[None, :], (ntab, centers.size))
        table = np.asarray(fn(vals), dtype=np.int64).reshape(ntab, 1 << w)
        idx = lut_index(a.q, p, r, signed)
        if idx.min() < 0 or idx.max() >= (1 << w):
            raise ValueError(f"{note}: calibration values leave the table range")
        ch = np.arange(C).reshape(1, C, 1, 1) if per_channel else np.zeros((1, 1, 1, 1), np.int64)
        q = table[np.broadcast_to(ch, idx.shape), idx]
        lo, hi = int(table.min()), int(table.max())
        tid = self.tensor(*a.q.shape[1:], lo, hi)
        site = LutSite(p, r, w, signed, ntab, body_add=(1 << 62) if signed else 0)
        self.ops.append(OpInfo(OP_LUT, a.tid, -1, tid, lut=site, table_values=table, note=note))
        return _Act(q, out_scale, tid, lo, hi)


def compile_model(model, calib, rounding_threshold_bits=6, n_bits=5, param_set=None, range_margin=0.05, p_error=None,
                  rounding_method="exact", tier_policy="exact", pool_policy="coarse"):
    """-> CompiledCircuit.  calib: float [B, C, H, W] calibration inputs (reference: first training batch,
    homomorphic_eval.py:258-261).
    tier_policy "exact" (default): the exact-evaluation catalogue of dctfhe/params.py for the model's bit width
    (params_for_bit_width: its own for 5-bit trunks, default_params() otherwise) whatever p_error says (the
    reference hands p_error = 0.01 to Concrete's optimiser, homomorphic_eval.py:282; here outputs then equal the integer
    circuit and the modelled failure estimate is reported).  tier_policy "p_error": the cheaper catalogue whose look-ups
    fail with probability <= p_error each -- stochastic outputs, like the reference's.
    rounding_method "approximate" (README.md:95-114 of the reference, rounding_threshold_bits={"n_bits":..,"method":
    "approximate"}): no one-bit rounding steps, the table bootstrap rounds; inputs next to a rounding boundary may land on
    the neighbouring table entry.
    pool_policy "coarse" (default): a max pool's relu table runs on the coarse tier of its width, whatever its price.  "exact": a pool
    that leaves the budget on that tier, or pushes the look-up that reads it out, moves to the catalogue's quiet pool tier
    (ParamSet.pool_tier_fallback_for_w), all its tree levels together.  Without a param_set the catalogue gains that tier
    (params.default_params_5bit_pool) only for a circuit that moves a pool: every other circuit compiles to the blob, the parameters and
    the evaluation keys of the default policy."""
    if pool_policy not in ("coarse", "exact"):
        raise ValueError(f"pool_policy {pool_policy!r}")
    if pool_policy == "exact" and tier_policy == "p_error":
        raise ValueError("pool_policy 'exact' needs tier_policy='exact': the p_error catalogue has no quiet pool tier (its look-ups "
                         "may each fail with probability p_error anyway)")
    if rounding_method not in ("exact", "approximate"):
        raise ValueError(f"rounding_method {rounding_method!r}")
    if tier_policy not in ("exact", "p_error"):
        raise ValueError(f"tier_policy {tier_policy!r}")
    own_catalogue = param_set is None
    if param_set is None:
        param_set = (P.params_for_p_error(p_error if p_error is not None else 0.01) if tier_policy == "p_error"
                     else P.params_for_bit_width(model.bit_width))
    ps = param_set
    calib = np.asarray(calib, dtype=np.float64)
    bits = model.bit_width
    bld = _Builder(ps, rounding_threshold_bits, range_margin)
    sgn_lo, sgn_hi = -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
    uq_hi = 2 ** bits - 1
    learned = getattr(model, "act_scales", None) or {}

    def scale_of(key, x, signed):
        """the quantiser's learned scale when the checkpoint carried one (dctfhe.checkpoint), else from the calibration batch"""
        s = learned.get(key)
        return float(s) if s else act_scale(x, signed, bits)

    # quant_inp (client side, in the clear; reference backbone.py:231,241)
    s_in = scale_of("quant_inp", calib, True)
    q0 = act_quant(calib, s_in, True, bits)
    t_in = bld.tensor(*q0.shape[1:], sgn_lo, sgn_hi)
    a = _Act(q0, s_in, t_in, sgn_lo, sgn_hi)

    # stem: conv1 -> bn1 -> [QuantReLU] -> quant_out  (backbone.py:232-261), one fused per-channel table
    acc = bld.conv(a, model.conv1, bits)
    real = acc.q * acc.scale
    _bn_calibrate(model.bn1, real)
    h = _bn_apply(model.bn1, real)
    pool1 = getattr(model, "pool1", None)
    if pool1 and not model.relu1:
        raise ValueError("the stem MaxPool2d follows the stem QuantReLU (reference backbone.py:248-259)")
    if model.relu1:
        s_r = scale_of("stem_relu", np.maximum(h, 0), False)
        hq = act_quant(np.maximum(h, 0), s_r, False, bits) * s_r
    else:
        s_r, hq = None, h
    if pool1:
        hq = max_pool_int(np.rint(hq / s_r).astype(np.int64), *pool1) * s_r
    s_q0 = scale_of("stem_quant_out", hq, True)

    def chan_fn(bn, s_acc, post):
        def fn(vals):
            x = _bn_apply(bn, (vals * s_acc)[None, :, :, None])   # vals [C, n] -> [1, C, n, 1]
            return post(x)[0, :, :, 0]
        return fn

    def stem_post(x):
        if s_r is not None:
            x = act_quant(np.maximum(x, 0), s_r, False, bits) * s_r
        return act_quant(x, s_q0, True, bits)

    if pool1:
        # three sites: bn1 + QuantReLU (u-bit on s_r), the max pool on those integers, quant_out.  The first runs split + refreshed
        # (lut_to_conv) so that the 3x-larger-than-the-pool-output stem tensor is stored at the refresh ring
        r0 = bld.lut_to_conv(acc, chan_fn(model.bn1, acc.scale, lambda x: act_quant(np.maximum(x, 0), s_r, False, bits)), True, True, s_r,
                             "stem: bn1+relu")
        mp = bld.max_pool(r0, *pool1, "stem: pool1")
        a = bld.lut_to_conv(mp, lambda vals: act_quant(vals * s_r, s_q0, True, bits), False, False, s_q0, "stem: pool1 -> quant_out")
    else:
        a = bld.lut_to_conv(acc, chan_fn(model.bn1, acc.scale, stem_post), True, True, s_q0, "stem: bn1+relu+quant_out")

    for bi, blk in enumerate(model.blocks):
        # C1 -> BN1 -> relu1 (u4)                                            backbone.py:94-96
        acc1 = bld.conv(a, blk.C1, bits)
        real1 = acc1.q * acc1.scale
        _bn_calibrate(blk.BN1, real1)
        h1 = np.maximum(_bn_apply(blk.BN1, real1), 0)
        s_r1 = scale_of(("block", bi, "relu1"), h1, False)
        r1 = bld.lut_to_conv(acc1, chan_fn(blk.BN1, acc1.scale, lambda x, s=s_r1: act_quant(np.maximum(x, 0), s, False, bits)), True, True, s_r1,
                     f"block{bi}: BN1+relu1")
        # C2 -> BN2 -> quant_out (s4)                                        backbone.py:97-99
        acc2 = bld.conv(r1, blk.C2, bits)
        real2 = acc2.q * acc2.scale
        _bn_calibrate(blk.BN2, real2)
        g2 = _bn_apply(blk.BN2, real2)
        s_qo = scale_of(("block", bi, "quant_out"), g2, True)
        main_hi, main_lo = sgn_hi * s_qo, sgn_lo * s_qo
        # shortcut                                                           backbone.py:100
        if blk.shortcut is None:
            sc_lo, sc_hi = a.lo * a.scale, a.hi * a.scale
            accs = None
        else:
            accs = bld.conv(a, blk.shortcut, bits)
            reals = accs.q * accs.scale
            _bn_calibrate(blk.BNshortcut, reals)
            gs = _bn_apply(blk.BNshortcut, reals)
            s_qs = scale_of(("block", bi, "BNquant_out"), gs, True)
            sc_lo, sc_hi = sgn_lo * s_qs, sgn_hi * s_qs
        # common integer scale of the residual sum: n_bits signed, guaranteed by construction
        zmax, zmin = 2 ** (n_bits - 1) - 1, -(2 ** (n_bits - 1))
        s_c = max(main_hi + sc_hi, -(main_lo + sc_lo)) / zmax
        while (np.rint(main_hi / s_c) + np.rint(sc_hi / s_c) > zmax) or (np.rint(main_lo / s_c) + np.rint(sc_lo / s_c) < zmin):
            s_c *= 1.01
        u = bld.lut(acc2, chan_fn(blk.BN2, acc2.scale, lambda x, s=s_qo, c=s_c: np.rint(act_quant(x, s, True, bits) * s / c).astype(np.int64)),
                    True, True, s_c, f"block{bi}: BN2+quant_out+rescale")
        if accs is None:
            v = bld.lut(a, lambda vals, s=a.scale, c=s_c: np.rint(vals * s / c).astype(np.int64), False, False, s_c, f"block{bi}: rescale shortcut")
        else:
            v = bld.lut(accs, chan_fn(blk.BNshortcut, accs.scale, lambda x, s=s_qs, c=s_c: np.rint(act_quant(x, s, True, bits) * s / c).astype(np.int64)),
                        True, True, s_c, f"block{bi}: BNshortcut+BNquant_out+rescale")
        z = bld.add(u, v)                                                    # backbone.py:102
        zr = np.maximum(z.q * s_c, 0)
        s_r2 = scale_of(("block", bi, "relu2"), zr, False)
        a = bld.lut_to_conv(z, lambda vals, c=s_c, s=s_r2: act_quant(np.maximum(vals * c, 0), s, False, bits), False, False, s_r2, f"block{bi}: relu2")

    # AvgPool2d(k) as a window sum, then QuantIdentity (s4)                  backbone.py:276-278
    K = model.avgpool_kernel
    pooled = bld.sum_pool(a, K)
    realp = pooled.q * pooled.scale / (K * K)
    s_f = scale_of("final", realp, True)
    out = bld.lut(pooled, lambda vals, s=pooled.scale / (K * K), f=s_f: act_quant(vals * s, f, True, bits), False, True, s_f, "avgpool+QuantIdentity")

    circ = CompiledCircuit(tensors=bld.tensors, ops=bld.ops, input_tensor=t_in, output_tensor=out.tid, in_scale=s_in, in_bits=bits,
                           out_scale=s_f, out_bits=bits, max_bit_width=bld.max_bits, param_set=ps,
                           rounding_threshold_bits=rounding_threshold_bits, n_bits=n_bits, rounding_method=rounding_method,
                           tier_policy=tier_policy, pool_policy=pool_policy, calib_out=out.q.reshape(out.q.shape[0], -1))
    _settle(circ)
    if pool_policy == "exact":
        budget = getattr(ps, "p_budget", 1e-12)
        if own_catalogue and _pools_over_budget(circ, budget):
            # the circuit needs a quiet pool tier: the same catalogue with it appended (the other indices unchanged), priced from scratch
            quiet = P.params_for_bit_width(model.bit_width, pool_policy="exact")
            if quiet.pool_tier_fallback_for_w:
                ps = circ.param_set = quiet
                _settle(circ)
        # like the quiet twin of a parity split (_settle): a pool moves where it, or the look-up that reads its noisier output, leaves the
        # budget; every tree level with it (level 1 alone on the coarse tier would leave level 2 near 1e-11)
        while ps.pool_tier_fallback_for_w:
            move = [o for o in _pools_over_budget(circ, budget) if not o.pool.quiet and o.pool.p_d in ps.pool_tier_fallback_for_w]
            if not move:
                break
            for o in move:
                o.pool.quiet = True
            _settle(circ)
    if own_catalogue and tier_policy == "exact" and circ.worst_site_failure > 1e-10:
        import warnings
        warnings.warn(f"dctfhe: a look-up site exceeds the exact-evaluation budget (p_fail/element {circ.worst_site_failure:.1e}); "
                      "outputs may differ from the integer circuit -- see CompiledCircuit.report()")
    circ.blob = _serialize(circ)
    return circ


def _pools_over_budget(circ, budget):
    """the max pools whose worst pairwise maximum, or whose reading look-up, fails more often than `budget`"""
    reader = {o.src0: o for o in circ.ops if o.type == OP_LUT}
    return [o for o in circ.ops if o.type == OP_MAXPOOL and max(o.pfail, reader[o.dst].pfail if o.dst in reader else 0.0) > budget]


def _settle(circ):
    """encodings, tiers and prices (_price), then the quiet twins of the parity splits"""
    ps = circ.param_set
    _price(circ)
    # parity-split sites: both look-ups on the site's (one-level) table tier where the budget holds; where the site's consumer -- the
    # refresh that reads the sum of two bootstrap outputs -- leaves it, the second look-up moves to the quiet twin, site by site
    budget = getattr(ps, "p_budget", 1e-12)
    while True:
        reader = {o.src0: o for o in circ.ops if o.type == OP_LUT}
        move = [o for o in circ.ops if o.type == OP_LUT and o.lut.mode == LUT_SPLIT and ps.tiers[o.lut.tab_tier].ksk_share >= 0
                and max(o.pfail, reader[o.dst].pfail if o.dst in reader else 0.0) > budget]
        if not move:
            break
        for o in move:
            o.lut.mode = LUT_SPLIT_QUIET
        _estimate_noise(circ)


# ------------------------------------------------------------------------------------------ encodings
def _price(circ):
    """encodings and tiers, then the noise budget; a catalogue whose faster, noisier tiers (two-bit refresh) take a site out of the
    budget falls back to their quiet twins, once, and is priced again"""
    ps = circ.param_set
    _assign_encodings(circ)
    _estimate_noise(circ)
    if getattr(ps, "table_tier_fallback_for_w", None) and circ.worst_site_failure > ps.p_budget:
        ps.table_tier_for_w = {**ps.table_tier_for_w, **ps.table_tier_fallback_for_w}
        ps.table_tier_fallback_for_w = None
        _assign_encodings(circ)
        _estimate_noise(circ)


def _encode_tables(o, e):
    enc = (o.table_values.astype(object) * (1 << e)) % (1 << 64)
    return np.array(enc, dtype=np.uint64).view(np.int64)


def _assign_encodings(circ):
    T, ops, ps = circ.tensors, circ.ops, circ.param_set
    req = [None] * len(T)
    req[circ.output_tensor] = 63 - (circ.out_bits + 1)          # signed out_bits value + padding
    for o in reversed(ops):
        if o.type == OP_LUT:
            need = 63 - o.lut.p
        elif o.type == OP_MAXPOOL:               # the output shares the input's encoding; the difference needs p_d bits
            need = 63 - o.pool.p_d if req[o.dst] is None else min(req[o.dst], 63 - o.pool.p_d)
        else:
            need = req[o.dst]
        for s in ([o.src0, o.src1] if o.type == OP_ADD else [o.src0]):
            req[s] = need if req[s] is None else min(req[s], need)
    T[circ.input_tensor].e = req[circ.input_tensor]
    T[circ.input_tensor].deff = ps.input_dim or ps.D
    # a table whose output is only ever added (or decrypted) tolerates a noisier, cheaper tier
    amplified = [False] * len(T)
    for o in ops:
        if o.type in (OP_CONV, OP_SUMPOOL, OP_MAXPOOL):     # a max pool subtracts two inputs and adds bootstrap outputs to one
            amplified[o.src0] = True
    for o in reversed(ops):          # an add passes the requirement of its result on to its operands
        if o.type == OP_ADD and amplified[o.dst]:
            amplified[o.src0] = amplified[o.src1] = True
    for o in ops:
        o.deff_in = max(T[o.src0].deff, T[o.src1].deff) if o.type == OP_ADD else T[o.src0].deff
        if o.type == OP_LUT:
            L = o.lut
            T[o.dst].e = req[o.dst]
            L.shift = (63 - L.p) - T[o.src0].e
            assert L.shift >= 0
            # a table one bit wider than the catalogue's widest (7 bits on the shipped ones) runs as a parity split: two look-ups of
            # w - 1 bits on the tier a (w - 1)-bit site takes
            coarse, split = not amplified[o.dst], False
            try:
                tier = ps.tier_for_width(L.w, coarse=coarse)
            except ValueError:
                try:
                    tier = ps.tier_for_width(L.w - 1, coarse=coarse)
                except ValueError:
                    raise ValueError(f"{o.note}: no tier for a table of {L.w} input bits: the parity split reaches one bit beyond the catalogue's "
                                     f"widest tables, more would need a larger ring (N = 16384 for 8 bits: DESIGN.md section 9)") from None
                split = True
                if circ.rounding_method == "approximate":
                    raise ValueError(f"{o.note}: a table of {L.w} input bits needs the exact method: the parity split takes the table's low bit "
                                     f"with a step of the one-bit rounding chain, which approximate rounding does not run")
                if circ.tier_policy == "p_error":
                    raise ValueError(f"{o.note}: a table of {L.w} input bits needs tier_policy='exact': the p_error catalogue has no tier with "
                                     f"the 2^-{L.w + 1} half-box both look-ups of a parity split need")
            if (L.w - 1 if split else L.w) > ps.tiers[tier].logN - 1:
                raise ValueError("table wider than the ring")
            L.tab_tier, L.bit_tier = tier, ps.bit_tier if (L.r > 0 or split) else -1
            # no hand-over yet: _estimate_noise finds the steps from which the coarser bit tiers will do
            L.coarse, L.coarse_from, L.coarse2 = (ps.bit_tier_coarse if ps.bit_tier_coarse is not None else -1), L.r + int(split), -1
            if split:      # keeps a choice of the quiet second tier made by compile_model across a re-assignment
                L.mode = L.mode if L.split() else LUT_SPLIT
            else:
                L.mode = LUT_APPROX if (circ.rounding_method == "approximate" and L.r > 0) else LUT_EXACT
            T[o.dst].deff = ps.tiers[tier].k << ps.tiers[tier].logN
            if split and ps.tiers[tier].ksk_share >= 0:      # the second look-up may move to the quiet twin: room for its ring too
                q = ps.tiers[ps.tiers[tier].ksk_share]
                T[o.dst].deff = max(T[o.dst].deff, q.k << q.logN)
            o.payload = _encode_tables(o, T[o.dst].e)
            if split:
                split_tables(o.payload)       # refuses a table whose pairs have no exact half (e = 0 with an odd sum)
        elif o.type == OP_MAXPOOL:
            S = o.pool
            T[o.dst].e = T[o.src0].e
            S.shift = (63 - S.p_d) - T[o.src0].e
            assert S.shift >= 0
            S.tier = ps.pool_tier_fallback_for_w[S.p_d] if S.quiet else ps.tier_for_width(S.p_d, coarse=not amplified[o.dst])
            if S.p_d > ps.tiers[S.tier].logN - 1:
                raise ValueError("max-pool difference table wider than the ring")
            # the pairwise maxima accumulate a bootstrap output into the first kN words of a copy of `b`
            T[o.dst].deff = max(T[o.src0].deff, ps.tiers[S.tier].k << ps.tiers[S.tier].logN)
            o.payload = _encode_tables(o, T[o.dst].e)
        else:
            T[o.dst].e = T[o.src0].e
            T[o.dst].deff = o.deff_in
            if o.type == OP_ADD:
                assert T[o.src1].e == T[o.src0].e, "residual operands must share an encoding"


# ------------------------------------------------------------------------------------------ noise budget
def _estimate_noise(circ, input_var=None, settle=True):
    """input_var: the input tensor's variance (default: a fresh secret-key encryption's).  settle=False prices the hand-over steps the
    sites already have instead of choosing them again (public_input_plan: the blob is what it is)"""
    ps, T = circ.param_set, circ.tensors
    T[circ.input_tensor].var = ps.input_sigma ** 2 if input_var is None else input_var
    total, flips = 0.0, 0.0
    for o in circ.ops:
        s = T[o.src0]
        if o.type == OP_CONV:
            T[o.dst].var = o.nu2 * s.var
        elif o.type == OP_ADD:
            T[o.dst].var = s.var + T[o.src1].var
        elif o.type == OP_SUMPOOL:
            T[o.dst].var = o.sum_k ** 2 * s.var
        elif o.type == OP_MAXPOOL:
            for fail in _price_max_pool(ps, o, s, T[o.dst]):       # one by one: the sum keeps its order
                total += fail
        else:
            fail, flip = _price_lut(ps, o, s, T[o.dst], settle)
            total += fail
            flips += flip
    circ.expected_failures_per_image = total
    circ.expected_boundary_flips_per_image = flips


def _price_max_pool(ps, o, s, d):
    """-> expected failures per image, one term per tree level.  Every level: the difference of two candidates (variance var(a) + var(b),
    bounded by twice the level's worst), key-switched over the level's effective dimension, mod-switched, one signed p_d-bit table;
    b + relu(a - b) adds one bootstrap output to b.  The column pass starts from the row pass's output."""
    S = o.pool
    tt = ps.tiers[S.tier]
    ring = tt.k << tt.logN
    v, d_in, worst, v_tab, v_worst, fails = s.var, s.deff or ps.D, 0.0, 0.0, 0.0, []
    for mult, pairs in S.pool_geom:
        for npair in pairs:
            v_tab = 2.0 * v * 4.0 ** S.shift + P.var_keyswitch(d_in, tt) + P.var_modswitch(tt)
            pf = P.p_fail(2.0 ** -(S.p_d + 2), v_tab)
            worst, v_worst = max(worst, pf), max(v_worst, v_tab)
            fails.append(pf * mult * npair)
            v += P.var_pbs_out(tt, ps.fft_noise_c)
            d_in = max(d_in, ring)
    o.pfail = worst
    o.margin = [v_worst]
    o.sim_sigma = math.sqrt(v_tab)
    d.var = v
    return fails


def _price_lut(ps, o, s, d, settle=True):
    """-> (expected failures, expected boundary flips) per image; settles the site's hand-over steps (LutSite.coarse_from, coarse2,
    coarse2_from) unless settle is False: then the site is priced as it stands"""
    L = o.lut
    n_elt = s.C * s.H * s.W
    tt = ps.tiers[L.tab_tier]
    v_in0 = s.var * 4.0 ** L.shift
    d_in = s.deff or ps.D                                     # the key switch only sums over the non-zero mask words
    v_tab_in = P.var_keyswitch(d_in, tt) + P.var_modswitch(tt)
    # parity split: r + 1 one-bit steps, two look-ups of w - 1 bits; the second one's input carries the parity bootstrap's
    # output (tier of the last step) on top of the chain's, its key switch and mod switch are its own tier's
    split, R_, W_ = L.split(), L.n_steps(), L.table_bits()
    t2 = ps.tiers[L.tier2(ps)] if split else None
    v_tab2_in = (P.var_keyswitch(d_in, t2) + P.var_modswitch(t2)) if split else 0.0
    c2 = getattr(ps, "bit_tier_coarse2", None)

    def handed_over(cf, cf2=None):
        """the site with its hand-overs at steps cf (one-level twin) and cf2 (two-bit-rotation twin; None: not at all)"""
        return replace(L, coarse_from=cf, coarse2=-1 if cf2 is None else c2, coarse2_from=cf2 or 0)

    def site_pfail(C):
        """candidate site C -> (failure probability per element, the variance at every decision that has a key switch of its own, in
        for_each_bootstrap's order)"""
        pf_, v_, step, var = 0.0, v_in0, None, []
        # an approximate site has no steps: the low r bits ride along; a failure is noise beyond the table's half-box.  (The two inputs
        # next to a rounding boundary, 2 of 2^r, sit half an input unit from it and take the neighbouring entry far more often: the
        # method's own inexactness, reported apart as boundary flips.  Its variance is listed for completeness: the audit refuses the site.)
        for i in range(R_):
            step = ps.tiers[C.step_tier(i)]
            # the tier that runs the step key-switches to its own small key (own length, own noise) and mod-switches on its ring
            v_bit_in = P.var_keyswitch(max(d_in, step.k << step.logN), step) + P.var_modswitch(step)
            v_step = 4.0 ** (L.p - i) * v_ + v_bit_in
            pf_ += P.p_fail(0.25, v_step)
            var.append(v_step)
            v_ += P.var_pbs_out(step, ps.fft_noise_c)
        v_second = (v_ + P.var_pbs_out(step, ps.fft_noise_c) + v_tab2_in) if split else 0.0
        second = P.p_fail(2.0 ** -(W_ + 2), v_second) if split else 0.0
        return pf_ + P.p_fail(2.0 ** -(W_ + 2), v_ + v_tab_in) + second, var + ([v_second] if split else []) + [v_ + v_tab_in]

    chosen = handed_over(R_) if settle else L
    pf = site_pfail(chosen)[0]
    if settle and R_ > 0 and L.coarse >= 0:
        # earliest step from which the one-level bit tier keeps the site within 2x of its all-precise failure rate
        budget = max(2.0 * pf, getattr(ps, "p_budget", 1e-12))
        cf = R_
        while cf > 0 and site_pfail(handed_over(cf - 1))[0] <= budget:
            cf -= 1
        chosen = handed_over(cf)
        if c2 is not None:      # ... and, inside that budget, the earliest step from which the two-bit-rotation tier will do
            cf2 = R_
            while cf2 > cf and site_pfail(handed_over(cf, cf2 - 1))[0] <= budget:
                cf2 -= 1
            if cf2 < R_:
                chosen = handed_over(cf, cf2)
        L = o.lut = chosen
    o.pfail, o.margin = site_pfail(chosen)
    # what `simulate` injects: the priced noise at the table, on top of what the one-bit steps left, and at a split's second look-up
    o.sim_sigma = math.sqrt(o.margin[-1])
    o.sim_sigma2 = math.sqrt(o.margin[-2]) if split else 0.0
    d.var = P.var_pbs_out(tt, ps.fft_noise_c) + (P.var_pbs_out(t2, ps.fft_noise_c) if split else 0.0)
    flip = (2.0 / 2 ** L.r) * P.p_fail(2.0 ** -(L.p + 2), v_in0 + v_tab_in) * n_elt if L.approx() else 0.0
    return o.pfail * n_elt, flip


# ------------------------------------------------------------------------------------------ blob
# The op record (struct Op of csrc/circuit.h, whose parse_circuit is the decoder): type, src0, src1, dst, ip[12], lp[2], payload range.
#   every op    ip[10] = effective dimension of what the op reads
#   OP_CONV     ip[0..4] = Cout, KH, KW, stride, pad
#   OP_SUMPOOL  ip[0] = window K
#   OP_LUT      ip[0..3] = p, r, w, shift; ip[4] = table tier; ip[5] = bit tier; ip[6] = tables; ip[7], ip[8] = one-level twin of the bit
#               tier and the step it takes over from; ip[9] = mode; ip[11] = two-bit-rotation twin << 8 | its step; lp[0] = body offset
#   OP_MAXPOOL  ip[0..2] = k, stride, pad; ip[3] = shift; ip[4] = tier of the relu table; ip[5] = p_d; ip[6] = 1 table; lp[0] = body offset
# A tier slot < 0 (ip[11]: the whole slot -1): no such hand-over.  lp words travel as signed 64-bit; src1 of a one-input op as 0.
def _encode_record(o):
    """-> (ip[12], lp[2]) of op `o`: the one place that knows which slot holds which field"""
    ip, body_add = [0] * 12, 0
    if o.type == OP_CONV:
        ip[:5] = [o.conv.Cout, o.conv.KH, o.conv.KW, o.conv.stride, o.conv.pad]
    elif o.type == OP_SUMPOOL:
        ip[0] = o.sum_k
    elif o.type == OP_LUT:
        L, body_add = o.lut, o.lut.body_add
        ip[:10] = [L.p, L.r, L.w, L.shift, L.tab_tier, L.bit_tier, L.ntab, L.coarse, L.coarse_from, L.mode]
        ip[11] = (L.coarse2 << 8 | L.coarse2_from) if L.coarse2 >= 0 else -1
    elif o.type == OP_MAXPOOL:
        S, body_add = o.pool, o.pool.body_add
        ip[:7] = [S.k, S.stride, S.pad, S.shift, S.tier, S.p_d, 1]
    ip[10] = o.deff_in
    return [int(x) for x in ip], [body_add - (1 << 64) if body_add >= (1 << 63) else body_add, 0]


def _serialize(circ):
    nT, nO = len(circ.tensors), len(circ.ops)
    head = struct.pack("<IIiiiiii", MAGIC, 1, nT, nO, circ.input_tensor, circ.output_tensor, circ.max_bit_width, 0)
    tens = b"".join(struct.pack("<iiii", t.C, t.H, t.W, 0) for t in circ.tensors)
    off = len(head) + len(tens) + nO * 96
    payloads, recs = [], []
    for o in circ.ops:
        pl = b"" if o.payload is None else np.ascontiguousarray(o.payload).tobytes()
        pad = (-len(pl)) % 16
        ip, lp = _encode_record(o)
        recs.append(struct.pack("<iiii12i2qqq", o.type, o.src0, max(o.src1, 0), o.dst, *ip, *lp, off if pl else 0, len(pl)))
        payloads.append(pl + b"\0" * pad)
        off += len(pl) + pad
    return head + tens + b"".join(recs) + b"".join(payloads)
