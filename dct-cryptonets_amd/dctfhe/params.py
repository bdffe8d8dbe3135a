"""Parameter tiers and the noise model that justifies them.

The reference hands `p_error` to Concrete's optimizer (homomorphic_eval.py:282, run_homomorphic_eval.sh:26)
and never sees the parameters it picks.  This build owns them: a static catalogue of tiers plus the
textbook TFHE variance formulas (Chillotti et al. 2020, section 4; all variances in torus^2 units),
used by the compiler to price every table site and to refuse a circuit whose failure budget is blown.

Security: binary keys; the minimal noise for ~128-bit security is taken from the linear fit
    log2 sigma_min(d) = -0.02641 * d + 2.49          (floor 2^-62)
through the tfhe-rs 128-bit parameter sets (d = 742, 864, 2048) -- background knowledge, not a
security proof; the catalogue never goes below it.
"""
import math
from dataclasses import dataclass, field, asdict


def sigma_min(d):
    return 2.0 ** max(-62.0, -0.02641 * d + 2.49)


@dataclass
class TierSpec:
    name: str
    n: int
    k: int
    logN: int
    l: int
    beta: int
    lk: int
    betak: int
    ksk_share: int = -1
    unroll: int = 1            # key bits per blind-rotate iteration (2: two-bit rotation, csrc/pbs_core.h; k = 1, l = 1 only)
    lwe_sigma: float = 0.0
    glwe_sigma: float = 0.0

    def __post_init__(self):
        if self.lwe_sigma == 0.0:
            self.lwe_sigma = sigma_min(self.n)
        if self.glwe_sigma == 0.0:
            self.glwe_sigma = sigma_min(self.k << self.logN)

    @property
    def N(self):
        return 1 << self.logN

    def as_dict(self):
        d = asdict(self)
        d.pop("name")
        return d


@dataclass
class ParamSet:
    """D: big LWE dimension (master key); tiers by role."""
    D: int
    tiers: list
    bit_tier: int                      # index of the one-bit (rounding) tier
    table_tier_for_w: dict             # table input width w -> tier index (outputs that feed a convolution / pooling)
    coarse_tier_for_w: dict = None     # same, for tables whose output only feeds an add or the circuit output (noisier is fine)
    table_tier_fallback_for_w: dict = None   # quieter (slower) tiers the compiler falls back to when a site leaves the budget
    pool_tier_fallback_for_w: dict = None    # p_d -> the quieter tier a max pool moves to when it or its reader leaves the budget (pool_policy "exact")
    bit_tier_coarse: int = None        # one-level twin of the bit tier for the last rounding steps of a site
    bit_tier_coarse2: int = None       # a still cheaper (noisier) twin for the steps after those
    refresh_min_w: int = None          # tables this wide that feed a convolution are split: coarse look-up + small-ring refresh
    p_budget: float = 1e-12            # failure probability a single look-up site may spend on cheaper rounding steps
    input_sigma: float = 0.0
    input_dim: int = 0                 # fresh encryptions mask only this prefix of the big key (0 = D); sets input_sigma's dimension
    fft_noise_c: float = 2.0           # empirical constant of the f64-FFT error term (tests/test_gpu_noise.py)

    def __post_init__(self):
        if self.input_sigma == 0.0:
            self.input_sigma = sigma_min(self.input_dim or self.D)

    @property
    def n_max(self):
        return max(t.n for t in self.tiers)

    def tier_for_width(self, w, coarse=False):
        table = self.coarse_tier_for_w if (coarse and self.coarse_tier_for_w) else self.table_tier_for_w
        for ww in sorted(table):
            if w <= ww:
                return table[ww]
        raise ValueError(f"no tier for a table of {w} input bits")


# ------------------------------------------------------------------------------------------ tier selections
def ksk_owner(ps, tier):
    """the tier whose key-switch key `tier` switches with: the end of its share chain"""
    while ps.tiers[tier].ksk_share >= 0:
        tier = ps.tiers[tier].ksk_share
    return tier


@dataclass(frozen=True)
class KeyTierSelection:
    """A tier selection of one ParamSet by name and as the library's bit masks (include/dctfhe.h dctfhe_key_tiers): bsk, the tiers whose
    bootstrap key is present; ksk, the tiers whose OWN key-switch key is present (a tier that shares has none)."""
    bsk: frozenset
    ksk: frozenset
    bsk_mask: int
    ksk_mask: int

    @classmethod
    def from_masks(cls, ps, bsk_mask, ksk_mask):
        names = lambda m: frozenset(t.name for i, t in enumerate(ps.tiers) if (m >> i) & 1)
        if (bsk_mask | ksk_mask) >> len(ps.tiers):
            raise ValueError(f"tier selection names a tier at or beyond the {len(ps.tiers)} tiers of the parameter set")
        return cls(names(bsk_mask), names(ksk_mask), int(bsk_mask), int(ksk_mask))

    @classmethod
    def all(cls, ps):
        return cls.from_masks(ps, (1 << len(ps.tiers)) - 1, sum(1 << i for i, t in enumerate(ps.tiers) if t.ksk_share < 0))

    def is_all(self, ps):
        return self == KeyTierSelection.all(ps)

    def covers(self, other):
        return not (other.bsk_mask & ~self.bsk_mask) and not (other.ksk_mask & ~self.ksk_mask)

    def missing(self, other):
        """what `other` asks for and this selection lacks, as text (for refusals)"""
        parts = [f"bootstrap key of {n}" for n in sorted(other.bsk - self.bsk)] + [f"key-switch key of {n}" for n in sorted(other.ksk - self.ksk)]
        return ", ".join(parts)


EVAL_BLOB_HEADER = 16 + 24 + 56 * 12      # u32 magic, u32 version, u64 total bytes, the dctfhe_params (12 tier slots)


def key_section_bytes(ps, t):
    """bytes of one tier's sections in the two evaluation-key blob forms (include/dctfhe.h): the Fourier bootstrap key and the whole
    key-switch key; the compressed form's standard-domain bodies"""
    blocks = 3 * t.n // 2 if t.unroll == 2 else t.n
    own = t.ksk_share < 0
    return dict(bsk_full_bytes=blocks * (t.k + 1) ** 2 * t.l * (t.N // 2) * 16, bsk_compressed_bytes=blocks * (t.k + 1) * t.l * t.N * 8,
                ksk_full_bytes=ps.D * t.lk * (t.n + 1) * 8 if own else 0, ksk_compressed_bytes=ps.D * t.lk * 8 if own else 0)


def key_blob_bytes(ps, sel, compressed):
    """bytes of an evaluation-key blob under a closed selection: header (+ the 32-byte public generator key in the compressed form), the
    two masks unless everything is selected, the kept sections (dctfhe_key_tiers_blob_bytes is the library's figure)"""
    n = EVAL_BLOB_HEADER + (32 if compressed else 0) + (0 if sel.is_all(ps) else 8)
    form = "compressed" if compressed else "full"
    for i, t in enumerate(ps.tiers):
        b = key_section_bytes(ps, t)
        n += b[f"ksk_{form}_bytes"] * ((sel.ksk_mask >> i) & 1) + b[f"bsk_{form}_bytes"] * ((sel.bsk_mask >> i) & 1)
    return n


# ------------------------------------------------------------------------------------------ variances
def ks_limbs(t):
    """byte limbs kept per key-switch-key word (csrc/dctfhe.hip ks_limbs): the key lives on the 2^-(8 limbs) torus grid"""
    bits = t.lk * t.betak + 6
    return 2 if bits <= 16 else 4 if bits <= 32 else 8


def var_keyswitch(D_eff, t):
    B = 2.0 ** t.betak
    row = t.lwe_sigma ** 2 + 2.0 ** (-16 * ks_limbs(t)) / 12.0          # the key's body is rounded to its grid: 2^-32 (2^-16 on the one-bit tiers)
    return D_eff * t.lk * ((B * B + 2) / 12.0) * row + (D_eff / 2.0) * 2.0 ** (-2 * t.betak * t.lk) / 12.0


def var_modswitch(t, centred=True):
    """rounding every word of the small ciphertext to 2N levels: sum_i s_i e_i + e_b with e uniform on +-1/(4N).  The engine's mod
    switch is CENTRED (csrc/kernels.h k_ms_center, oracle ref_ms_center): half the sum of the known remainders e_i comes off the body,
    leaving sum_i (s_i - 1/2) e_i -- n/4 units instead of the n/2 of the plain form (binary key, half the bits set)."""
    return ((t.n / 4.0 if centred else t.n / 2.0) + 1.0) / (48.0 * t.N ** 2)


def var_pbs_out(t, fft_c=2.0):
    B = 2.0 ** t.beta
    kN = t.k * t.N
    ext = t.l * (t.k + 1) * t.N * ((B * B + 2) / 12.0) * t.glwe_sigma ** 2 + (kN / 2.0 + 1.0) * 2.0 ** (-2 * t.beta * t.l) / 12.0
    # f64 FFT rounding of the external product, measured on the GPU (tools/noise_probe.py) and on the CPU oracle
    # against the exact schoolbook product (tests/emul): per CMUX  c * (k+1) l N^2 B^2/12 * 2^-106, c ~ 2.
    fft = fft_c * (t.k + 1) * t.l * float(t.N) ** 2 * (B * B / 12.0) * 2.0 ** -106
    if getattr(t, "unroll", 1) == 2:
        # two-bit rotation, per PAIR: three products scaled by (X^e - 1) (variance x2) -> key and FFT noise 6 units instead
        # of 2; the single decomposition error enters through (X^e - 1) b_w, one of the three b_w set with probability
        # 3/4 -> 1.5 units where the one-bit chain has 2 x 1/2 (the formula above counts a unit per CMUX, twice the truth)
        key = t.l * (t.k + 1) * t.N * ((B * B + 2) / 12.0) * t.glwe_sigma ** 2
        dec = (kN / 2.0 + 1.0) * 2.0 ** (-2 * t.beta * t.l) / 12.0
        return (t.n / 2.0) * (6.0 * key + 3.0 * dec + 6.0 * fft)
    return t.n * (ext + fft)


def var_round16(n):
    """packed results (csrc/kernels.h k_pack16): every word of a small ciphertext rounded to the 2^-16 torus grid.  The phase keeps
    sum_i s_i e_i + e_b with e uniform on +-2^-17: n/2 + 1 units of 2^-32 / 12 (binary key, half the bits set; plain rounding)."""
    return (n / 2.0 + 1.0) * 2.0 ** -32 / 12.0


@dataclass
class PackSpec:
    """ring packing of result ciphertexts (include/dctfhe.h dctfhe_pack_key_export): ring N_p = 2^logN whose key is the first N_p bits of the
    big key, l gadget levels of beta bits, key-row noise sigma.  Stands alone: no ParamSet field, nothing of it is serialised into a circuit."""
    logN: int = 11
    l: int = 1
    beta: int = 16
    sigma: float = None            # None: sigma_min(N_p); 0.0 is a noise-free key (tests only)

    def __post_init__(self):
        if self.sigma is None:
            self.sigma = sigma_min(1 << self.logN)

    @property
    def N(self):
        return 1 << self.logN

    def groups(self, count):
        return -(-int(count) // self.N)

    def words(self, count):
        """16-bit words of `count` ring-packed results: per group N mask words, then one body word per result"""
        return self.groups(count) * self.N + int(count)


def default_pack_spec(ps=None):
    """N_p = 2048, one level of 16 bits: with results rounded to 16 bits anyway a second level buys nothing, and the key stays 13 MB.
    ps given: raises ValueError where its big key is shorter than the ring (the ring key is a prefix of it)"""
    spec = PackSpec(logN=11, l=1, beta=16)
    if ps is not None and spec.N > ps.D:
        raise ValueError(f"ring packing: the ring key is a prefix of the big key, N_p = {spec.N} > D = {ps.D}; pass a PackSpec with a smaller ring")
    return spec


def test_pack_spec():
    """for test_params() (D = 1024): a ring of 256, noise far below every margin (NOT secure, like the catalogue it goes with)"""
    return PackSpec(logN=8, l=1, beta=16, sigma=2.0 ** -48)


def var_ring_pack(n, spec, m=None):
    """what ring packing adds to a small ciphertext of n mask words in a group of m results (default: a full ring): the key rows' noise
    through m n l digits, the decomposition's rounding of the n mask words against a binary key, and the 16-bit rounding of the N_p mask
    coefficients and the body against the ring key (half its bits set)"""
    m = spec.N if m is None else m
    B = 2.0 ** spec.beta
    return (m * n * spec.l * ((B * B + 2) / 12.0) * spec.sigma ** 2 + (n / 2.0) * 2.0 ** (-2 * spec.beta * spec.l) / 12.0
            + (spec.N / 2.0 + 1.0) * 2.0 ** -32 / 12.0)


@dataclass
class PublicInputSpec:
    """public-key inputs (include/dctfhe.h dctfhe_public_key_export): ring N_e = 2^logN whose key is the first N_e bits of the big key, noise
    sigma of the key row and of the encryptor's own draws.  Stands alone: no ParamSet field, nothing of it is serialised into a circuit."""
    logN: int = 11
    sigma: float = None            # None: sigma_min(N_e) (below 1 from N_e = 128 on); 0.0 is noise-free (tests only)

    def __post_init__(self):
        if not 5 <= int(self.logN) <= 12:
            raise ValueError(f"public-key inputs need 5 <= logN <= 12 (got {self.logN})")
        if self.sigma is None:
            self.sigma = sigma_min(1 << self.logN)
        if not 0.0 <= self.sigma < 1.0:
            raise ValueError(f"public-key inputs: noise std {self.sigma} outside [0, 1)")

    @property
    def N(self):
        return 1 << self.logN

    def groups(self, count):
        return -(-int(count) // self.N)

    def words(self, count):
        """64-bit words of `count` public-key inputs: per group N mask words, then one body word per input"""
        return self.groups(count) * self.N + int(count)

    def check(self, ps):
        """raises ValueError where the ring does not fit what an input of `ps` masks (input_dim, or D)"""
        dim = ps.input_dim or ps.D
        if self.N > dim:
            raise ValueError(f"public-key inputs: the ring key is a prefix of what an input masks, N_e = {self.N} > {dim}; "
                             f"pass a PublicInputSpec with a smaller ring")
        return self


def default_public_input_spec(ps=None):
    """N_e = 2048 at sigma_min(2048): a full group costs 16 bytes per input.  ps given: raises ValueError where its inputs mask fewer
    than 2048 words (input_dim, or D)"""
    spec = PublicInputSpec(logN=11)
    return spec.check(ps) if ps is not None else spec


def test_public_input_spec():
    """for test_params() (D = 1024): a ring of 256, noise far below every margin (NOT secure, like the catalogue it goes with)"""
    return PublicInputSpec(logN=8, sigma=2.0 ** -48)


def var_public_input(spec):
    """the noise of an extracted public-key input: E u (N_e/2 units of sigma^2: u uniform binary), e1 Z (N_e/2: binary key, half the bits
    set) and e2 (one unit)"""
    return (spec.N + 1) * spec.sigma ** 2


def p_fail(margin, var):
    """two-sided Gaussian tail beyond `margin`"""
    if var <= 0:
        return 0.0
    return math.erfc(margin / math.sqrt(2.0 * var))


# ------------------------------------------------------------------------------------------ catalogue
def default_params():
    """Exact-evaluation set: every table site fails with probability < 1e-12 under the model above.

    Small-key lengths: n = 800 for the 5/6-bit table tiers, 760 / 720 for the 4-bit ones and 560 for the one-bit tiers are the
    smallest (in steps of 8) that keep every site of the benchmark circuits under that budget (tools/param_search.py ->
    profiles/r03_param_search.log; round 3's centred mod switch bought the last 8 bits of each table tier) with base-4 key-switch gadgets
    (below) and a key switch that sums only over the effective dimension of its input (2048 for everything downstream of a
    refresh or of the client, who encrypts under the first 2048 key bits: input_dim); the blind rotation is linear in n.

    T6 (6-bit tables after a rounded accumulator) needs N = 8192: its mod-switch noise must stay 6.4
    sigma inside a 2^-8 half-box.  T5a/T4 serve the 5-bit residual-sum tables and the 4-bit rescale
    tables.  Outputs that feed convolutions (2-norm ~2^6.7) into p-bit accumulators must stay near 2^-23:
    the f64 FFT error (~ N^2 B^2) forces small digits, hence three levels (T6, T4r, T4r2).
    B is the one-bit tier of the rounding chain: margin 1/4, so a small ring, but two levels because its
    output is subtracted from a p-bit accumulator."""
    # Key-switch gadget of the table tiers: base 4, nine levels (betak = 2, lk = 9) instead of base 8, six levels: the key-switch noise
    # lk (B^2 + 2) / 12 sigma^2 drops from 33 to 13.5 units (0.64 bit of sigma), which buys 24 small-key bits per tier -- 808 / 768 / 728
    # instead of 832 / 792 / 752, 3 % of every table bootstrap -- for 1.5x the work of their key switches (0.16 us of 5-25 us per
    # ciphertext).  The one-bit tiers (half-box 1/4) take base 4 at the SAME depth, five levels: only the top 10 bits of a mask word are
    # switched, the truncation (sigma 2^-6.8) stays below the key noise (2^-5.4), the gadget factor drops from 27.5 to 7.5 -- which buys
    # 24 key bits (560 instead of 584) and lets the two-bit-rotation tier Ba2 take every step Ba used to run (ResNet-20, ResNet-18 3x32^2).
    t6 = TierSpec("T6", n=800, k=1, logN=13, l=3, beta=11, lk=9, betak=2)
    # T4 / T4r look up 4-bit values (half-box 2^-6, four times the 6-bit tiers'): they afford a shorter small key -- and the
    # blind rotation is linear in n -- at the price of key-switch keys of their own (prefixes of the same small key, noise of
    # their own dimension).  752 / 792 are the smallest (steps of 8) that keep every site of the benchmark circuits at the
    # worst-site level of the 832-bit tiers (tools: the search behind profiles/r02_param_search.log).
    t4 = TierSpec("T4", n=720, k=1, logN=11, l=1, beta=23, lk=9, betak=2, unroll=2)
    b = TierSpec("B", n=560, k=2, logN=10, l=2, beta=14, lk=5, betak=2)
    # T6a: same ring and input margin as T6, one level: its output (sigma ~2^-13) only ever meets the 2^-7 half-box
    # of the residual-sum table, never a convolution.  Half the transforms of T6 for half of the 6-bit sites.
    t6a = TierSpec("T6a", n=800, k=1, logN=13, l=1, beta=22, lk=9, betak=2, ksk_share=0, unroll=2)
    # Ba: one-level bit tier.  The output of rounding step i is amplified by 2^(p-j) only in the later steps j > i,
    # so the later steps of a chain tolerate sigma ~2^-15; the compiler picks, per
    # site, the first step from which Ba is safe.
    ba = TierSpec("Ba", n=560, k=2, logN=10, l=1, beta=23, lk=5, betak=2, ksk_share=3)
    # T4r: small ring, three levels: turns the noisy 4-bit output of a T6a look-up into a convolution-grade ciphertext
    # (sigma ~2^-25).  T6a + T4r costs ~0.7x of one T6 bootstrap.
    t4r = TierSpec("T4r", n=760, k=1, logN=11, l=3, beta=12, lk=9, betak=2)
    # T4r2: the same refresh with two key bits per iteration (general form of the two-bit rotation, csrc/pbs_core.h): 10 %
    # fewer milliseconds per launch, output 0.7 bit noisier (three external products per pair).  The compiler takes it when every
    # site of the circuit stays inside the budget with it (the ResNet-20 circuits do) and falls back to T4r otherwise (two
    # sites of ResNet-18 3x32^2 would sit at 3.8e-12): ParamSet.table_tier_fallback_for_w.  Shares T4r's key-switch key.
    t4r2 = TierSpec("T4r2", n=760, k=1, logN=11, l=3, beta=12, lk=9, betak=2, ksk_share=1, unroll=2)
    # T5a: one-level twin of the three-level 5-bit tier; the 5-bit residual-sum table is split the same way (T5a + T4r)
    t5a = TierSpec("T5a", n=800, k=1, logN=12, l=1, beta=22, lk=9, betak=2, ksk_share=0, unroll=2)
    # (a table of 5 or 6 input bits that feeds a convolution without the split would run on T6; with refresh_min_w = 5 none does)
    # Ba2: the one-level bit tier on the general two-bit rotation: 49.7 ms per launch of 16 384 against 63.6 (profiles/r02_exp_ablations.log),
    # output 0.5 bit noisier (2^-14.5): the compiler gives it the steps of a chain that can take that (78 % of them), Ba the ones before.
    ba2 = TierSpec("Ba2", n=560, k=2, logN=10, l=1, beta=23, lk=5, betak=2, ksk_share=3, unroll=2)
    return ParamSet(D=8192, tiers=[t6, t4r, t4, b, t6a, ba, t4r2, t5a, ba2], bit_tier=3, table_tier_for_w={4: 6, 6: 0},
                    table_tier_fallback_for_w={4: 1}, coarse_tier_for_w={4: 2, 5: 7, 6: 4}, bit_tier_coarse=5, bit_tier_coarse2=8, refresh_min_w=5,
                    input_dim=2048)


def params_for_bit_width(bit_width, pool_policy="coarse"):
    """Exact-evaluation catalogue for circuits of `bit_width`-bit weights and activations: the 5-bit one below for 5, default_params()
    for every other width (that catalogue, its blob and its evaluation keys are what every 4-bit circuit depends on).
    pool_policy "exact": the catalogue a circuit takes whose max pool has to move to a quiet tier -- default_params_5bit_pool() for 5
    bits; no other width has such a tier (their pools sit far inside the budget: 1.5e-21 on T5a at 4 bits)."""
    if bit_width == 5:
        return default_params_5bit_pool() if pool_policy == "exact" else default_params_5bit()
    return default_params()


def default_params_5bit():
    """Exact-evaluation set for 5-bit trunks: default_params() plus a 5-bit refresh tier and a longer key for the first rounding steps.

    Two things break the exact budget when default_params() prices a 5-bit circuit (tools/param_search.py --bit-width 5 ->
    profiles/bw5_param_search.log):
      * the 5-bit activations that feed a convolution would be refreshed on T6 (N = 8192), so every tensor downstream would have
        effective dimension 8192 instead of 2048 and every key switch four times the noise.  T5r refreshes them on N = 2048.  It has
        four levels of 10 bits: the f64 FFT error grows as N^2 B^2 per level, and 4 x 10 bits of gadget at B = 2^10 leave a
        quarter of the variance of 3 x 12 at B = 2^12 -- what a 3x3x512 convolution of its outputs into a 14-bit accumulator needs
        (ResNet-18: the convolution of refresh outputs and the key switch of the first rounding step each sat at 2^-5.3 of a 1/4
        margin).
      * the rounding steps before the one-level twins take over (B) key-switch to a longer small key: its own key-switch noise was
        the other half of that first-step failure.  Ba / Ba2 keep n = 560 and therefore a key-switch key of their own (ksk_share
        needs the same shape).
    Every 4-bit tier of default_params() stays as it is (same indices), so a 5-bit blob runs on the same engine code paths."""
    ps = default_params()
    t = ps.tiers
    # B: the bit tier of the first rounding steps, longer small key
    t[3] = TierSpec("B", n=576, k=2, logN=10, l=2, beta=14, lk=5, betak=2)
    # Ba / Ba2: the one-level bit tiers keep n = 560 -- Ba owns the key-switch key Ba2 shares
    t[5] = TierSpec("Ba", n=560, k=2, logN=10, l=1, beta=23, lk=5, betak=2)
    t[8] = TierSpec("Ba2", n=560, k=2, logN=10, l=1, beta=23, lk=5, betak=2, ksk_share=5, unroll=2)
    # T5r: refresh of 5-bit tables that feed a convolution, four levels (csrc/pbs_core.h pack_digits: beta <= 10)
    t.append(TierSpec("T5r", n=856, k=1, logN=11, l=4, beta=10, lk=9, betak=2))
    ps.table_tier_for_w = {4: 6, 5: 9, 6: 0}
    return ps


def default_params_5bit_pool():
    """default_params_5bit() plus T6p at index 10, the quiet tier of the stem max pool (compile_model(pool_policy="exact")); indices 0-9
    are default_params_5bit()'s.

    At 5 bits the pool's difference table has p_d = 6 and runs on T6a (one level, output sigma ~2^-12.4).  From the second tree level
    on a candidate carries a T6a output and its key switch sums over 8192 mask words instead of 2048: sigma ~2^-10.2 against a 2^-8
    half-box, 5.7e-5 per pairwise maximum.  T6p is T6a's ring with two levels of 15 bits and the one-bit rotation: output sigma
    ~2^-20.2, six transforms per key bit where T6 has eight.  A longer key on one level does not help (n = 864: the pool at 8.7e-11, its
    reader behind it at 2.4e-10).  n = 832 is the smallest multiple of 8 at which the pool and every other site of ResNet-18 3x128^2 and
    3x224^2 stay under 1e-12 at rounding_threshold_bits 6 and 7 (tools/param_search.py --pool -> profiles/bw5_pool_param_search.log); it
    differs from T6's 800, so T6p owns its key-switch key."""
    ps = default_params_5bit()
    ps.tiers.append(TierSpec("T6p", n=832, k=1, logN=13, l=2, beta=15, lk=9, betak=2))
    ps.pool_tier_fallback_for_w = {6: 10}
    return ps


def params_for_p_error(p_error=0.01):
    """Catalogue for tier_policy "p_error" (SURVEY 8f-4): every look-up may fail with probability ~p_error, the regime the
    reference runs in (run_homomorphic_eval.sh:26).  z = 2.6 sigma inside the half-box instead of 7, so a 6-bit table fits
    N = 4096 and a 5-bit one N = 2048; outputs that feed a convolution only have to keep the *next* look-up inside its
    half-box (sigma ~2^-16 after the 2^6.7 amplification), which two levels with 16-bit digits give (sigma ~2^-21) -- no
    refresh bootstraps.  Meant for approximate rounding; with exact rounding the one-bit tiers B / Ba serve as before."""
    if not (1e-6 <= p_error <= 0.05):
        raise ValueError("tier_policy 'p_error' is meant for 1e-6 <= p_error <= 0.05; use the exact catalogue below that")
    f6 = TierSpec("F6", n=864, k=1, logN=12, l=2, beta=16, lk=6, betak=3)
    f5 = TierSpec("F5", n=864, k=1, logN=11, l=2, beta=16, lk=6, betak=3, ksk_share=0)
    t4 = TierSpec("T4", n=864, k=1, logN=11, l=1, beta=23, lk=6, betak=3, ksk_share=0, unroll=2)
    b = TierSpec("B", n=660, k=2, logN=10, l=2, beta=14, lk=5, betak=3)
    t5a = TierSpec("T5a", n=864, k=1, logN=12, l=1, beta=22, lk=6, betak=3, ksk_share=0, unroll=2)
    ba = TierSpec("Ba", n=660, k=2, logN=10, l=1, beta=23, lk=5, betak=3, ksk_share=3)
    return ParamSet(D=8192, tiers=[f6, f5, t4, b, t5a, ba], bit_tier=3, table_tier_for_w={4: 1, 5: 1, 6: 0},
                    coarse_tier_for_w={4: 2, 5: 2, 6: 4}, bit_tier_coarse=5, p_budget=p_error / 4.0, input_dim=2048)


def test_params():
    """Tiny rings for CPU-oracle-sized parity tests (NOT secure: dimensions far below the curve)."""
    t_tab = TierSpec("t", n=48, k=1, logN=10, l=2, beta=12, lk=5, betak=4, lwe_sigma=2.0 ** -26, glwe_sigma=2.0 ** -48)
    t_bit = TierSpec("b", n=40, k=2, logN=8, l=2, beta=10, lk=5, betak=4, lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -48)
    return ParamSet(D=1024, tiers=[t_tab, t_bit], bit_tier=1, table_tier_for_w={6: 0}, input_sigma=2.0 ** -55)


def to_c_params(ps):
    from .engine import make_params
    return make_params(ps.D, ps.n_max, [t.as_dict() for t in ps.tiers], ps.input_sigma, ps.input_dim)
