// circuit.h -- the compiled-circuit blob on the host: its wire structs, the one decode of an op record into a typed site, the enumeration
// of a site's bootstraps and the per-image statistics.  No HIP type, no device memory; whoever includes it declares `int fail(fmt, ...)`
// first.  A new op type or look-up mode is added HERE: a slot in the comment below, a member of its site struct filled by parse_circuit
// and, if it bootstraps, an entry in for_each_bootstrap -- the key check, row layout and scheduler of dctfhe.hip read nothing else.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dctfhe.h"

// ---- wire format (version 1): BlobHeader, n_tensors TensorShape, n_ops Op, then the payloads the records point at
struct BlobHeader { uint32_t magic, version; int32_t n_tensors, n_ops, input_tensor, output_tensor, max_bit_width, reserved; };
struct TensorShape { int32_t C, H, W, pad; size_t elems() const { return (size_t)C * H * W; } };
enum { OP_CONV = 1, OP_ADD = 2, OP_SUMPOOL = 3, OP_LUT = 4, OP_MAXPOOL = 5 };
// Slots per op type (dctfhe/compile.py writes them; ip[10] of every record: effective dimension of the tensor the op reads):
//   OP_CONV     ip[0..4] = Cout, KH, KW, stride, pad; payload: int8 weights [Cout][Cin][KH][KW]
//   OP_ADD      src0 + src1
//   OP_SUMPOOL  ip[0] = window K (stride K)
//   OP_LUT      ip[0..3] = p, r, w, shift; ip[4] = table tier; ip[5] = bit tier; ip[6] = tables (1 or one per channel); ip[9] = mode (LUT_*);
//               one-bit step i runs on ip[5], from step ip[8] on its one-level twin ip[7], from step ip[11] & 255 on the two-bit-rotation
//               twin ip[11] >> 8 (ip[7] / ip[11] < 0: no hand-over; the compiler proves each one safe, dctfhe/compile.py::step_tier is the
//               same rule); lp[0] = body offset; payload: int64 tables [ntab][2^w] (a split record keeps the whole tables)
//   OP_MAXPOOL  ip[0..2] = k, stride, pad; ip[3] = shift of the differences to 63 - p_d; ip[4] = tier of the relu table; ip[5] = p_d;
//               ip[6] = 1 table; lp[0] = body offset of the differences; payload: 2^p_d int64 entries
struct Op {
  int32_t type, src0, src1, dst;
  int32_t ip[12];
  int64_t lp[2];
  int64_t payload_off, payload_len;
};
// look-up modes: exact rounding; approximate rounding (no one-bit steps); parity split of a w-bit table (7 on the shipped catalogues) into
// two (w-1)-bit look-ups, both on the table tier or the second on the tier whose key-switch key the table tier shares (its quiet twin)
enum { LUT_EXACT = 0, LUT_APPROX = 1, LUT_SPLIT = 2, LUT_SPLIT_QUIET = 3 };

// ---- the decoded sites
struct ConvSite { int Cout, Cin, H, W, KH, KW, stride, pad; };
struct PoolSite { int k, stride, pad, shift, tier, p_d, deff_in; uint64_t body_add; };
struct StepTiers {      // tier of one-bit step i of a look-up site
  int bit = -1, coarse = -1, coarse_from = 1 << 30, coarse2 = -1, coarse2_from = 1 << 30;
  int at(int i) const { return (coarse2 >= 0 && i >= coarse2_from) ? coarse2 : (coarse >= 0 && i >= coarse_from) ? coarse : bit; }
};
struct LutSite {
  int p = 0, r = 0, w = 0, shift = 0, ntab = 1, mode = LUT_EXACT, deff_in = 0, tab_tier = -1;
  int tier2_named = -1;   // dctfhe_round_lut_split names its second tier outright; a circuit's record leaves it to the mode
  uint64_t body_add = 0;
  StepTiers steps;
  bool split() const { return mode == LUT_SPLIT || mode == LUT_SPLIT_QUIET; }
  bool approx() const { return mode == LUT_APPROX; }
  // one-bit steps: the r rounding steps, and for a split the one that takes the table index's low bit off the working ciphertext
  int n_steps() const { return approx() ? 0 : r + (split() ? 1 : 0); }
  int table_bits() const { return split() ? w - 1 : w; }
  // tier of a split's second look-up (-1: no split, or a quiet twin that cannot be named)
  int tier2(const dctfhe_params& P) const {
    if (mode == LUT_SPLIT) return tier2_named >= 0 ? tier2_named : tab_tier;
    return (mode == LUT_SPLIT_QUIET && tab_tier >= 0 && tab_tier < P.n_tiers) ? P.tiers[tab_tier].ksk_share : -1;
  }
  // what the site adds to the shifted body before it rounds.  Exact: half of what the r steps remove.  Approximate (the low bits stay, the
  // half-box rotation of the test vector rounds): half an input unit, so that the two inputs next to a rounding boundary are equally far
  uint64_t round_add() const { return body_add + (r == 0 ? 0 : approx() ? (1ULL << (62 - p)) : (1ULL << (63 - p + r - 1))); }
};
// one op of a circuit: the record's tensors and payload range, and the decoded site of its type (sum_k: the window of OP_SUMPOOL)
struct SiteOp {
  int type = 0, src0 = 0, src1 = 0, dst = 0, deff_in = 0, sum_k = 0;
  int64_t payload_off = 0, payload_len = 0;
  ConvSite conv{};
  PoolSite pool{};
  LutSite lut;
  std::vector<int64_t> halves;   // split look-up: [S | Dt] of split_tables_host, until dctfhe_circuit_load has uploaded them
};
// A slab group: an OP_CONV at `first` and the maximal run of OP_LUT / OP_MAXPOOL behind it, ops [first, end), in
// which every op reads exactly the destination of the op before it and nothing else reads that destination.  The destinations of ops
// [first, end - 1) are TRANSIENT: a session under a memory budget holds S channels of one image of them at a time; the last destination
// is written whole.  Only groups with a transient tensor (end - first >= 2) are listed.
struct SlabGroup { int first = 0, end = 0, channels = 0; };
struct CircuitPlan {
  std::vector<TensorShape> tensors; std::vector<SiteOp> ops; int input_tensor = 0, output_tensor = 0, max_bit_width = 0;
  std::vector<SlabGroup> groups;
};
static void decode_slab_groups(CircuitPlan* c) {
  const int n = (int)c->ops.size();
  std::vector<int> readers(c->tensors.size(), 0), writers(c->tensors.size(), 0);
  for (const SiteOp& o : c->ops) {
    readers[o.src0]++;
    if (o.type == OP_ADD) readers[o.src1]++;
    writers[o.dst]++;
  }
  readers[c->output_tensor]++;      // the download reads it
  readers[c->input_tensor]++;       // ... and the input stays resident
  c->groups.clear();
  for (int i = 0; i < n; i++) {
    if (c->ops[i].type != OP_CONV) continue;
    int j = i + 1;
    while (j < n && (c->ops[j].type == OP_LUT || c->ops[j].type == OP_MAXPOOL) && c->ops[j].src0 == c->ops[j - 1].dst && readers[c->ops[j - 1].dst] == 1 &&
           writers[c->ops[j - 1].dst] == 1 && c->ops[j].dst != c->ops[j].src0)
      j++;
    if (j - i >= 2) c->groups.push_back(SlabGroup{i, j, c->ops[i].conv.Cout});
    i = j - 1;
  }
}

// The bootstraps one element of a site takes, in execution order: f(tier, table_bits, has_own_keyswitch).  The only place that knows them.
// Look-up: the one-bit steps; for a split the parity bootstrap (on the last step's small ciphertext) and the second look-up; the table.
// Max pool: one relu bootstrap per pairwise maximum.  Any op: those of its site, none for the levelled ops.
template <class F> static void for_each_bootstrap(const LutSite& L, const dctfhe_params& P, F f) {
  const int n = L.n_steps();
  for (int i = 0; i < n; i++) f(L.steps.at(i), 0, true);
  if (L.split()) { f(L.steps.at(n - 1), 0, false); f(L.tier2(P), L.w - 1, true); }
  f(L.tab_tier, L.table_bits(), true);
}
template <class F> static void for_each_bootstrap(const PoolSite& S, const dctfhe_params&, F f) { f(S.tier, S.p_d, true); }
template <class F> static void for_each_bootstrap(const SiteOp& o, const dctfhe_params& P, F f) {
  if (o.type == OP_LUT) for_each_bootstrap(o.lut, P, f);
  if (o.type == OP_MAXPOOL) for_each_bootstrap(o.pool, P, f);
}

// Parity split of tables [ntab][2^w] (t = 2 t' + b0): S[j] = ((T[2j] + T[2j+1]) mod 2^64) >> 1, Dt[j] = T[2j] - S[j], so that
// S + Dt = T[2j] and S - Dt = T[2j+1] (mod 2^64) whatever the top bit of S.  out = [S: ntab << (w-1)][Dt: the same].  An odd sum has no
// half: -1 (the compiler keeps the output exponent of a split site >= 1).
static int split_tables_host(const int64_t* T, size_t ntab, int w, std::vector<int64_t>* out) {
  const size_t half = (size_t)1 << (w - 1), n = ntab * half;
  out->resize(2 * n);
  for (size_t i = 0; i < n; i++) {
    const uint64_t a = (uint64_t)T[2 * i], b = (uint64_t)T[2 * i + 1], sum = a + b;
    if (sum & 1) return -1;
    (*out)[i] = (int64_t)(sum >> 1);
    (*out)[n + i] = (int64_t)(a - (sum >> 1));
  }
  return 0;
}

static int pool_out_size(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }
// pairwise maxima of one image: every output of a pass costs its in-range taps minus one
static int64_t pool_pairs(int C, int H, int W, int k, int s, int p) {
  auto pass = [&](int n) {
    int64_t t = 0;
    for (int o = 0; o < pool_out_size(n, k, s, p); o++)
      for (int j = 0; j < k; j++) t += (o * s - p + j >= 0 && o * s - p + j < n) ? 1 : 0;
    return t - pool_out_size(n, k, s, p);
  };
  return (int64_t)C * H * pass(W) + (int64_t)C * pool_out_size(W, k, s, p) * pass(H);
}

// parse + validate a circuit blob on the host (no GPU): header, tensor table, op records, payload ranges, per-op shapes; every record is
// decoded into its site in the same pass, and nothing after it reads Op::ip / Op::lp
static int parse_circuit(const void* blob, size_t size, CircuitPlan* c) {
  if (!blob) return fail("null circuit blob");
  if (size < sizeof(BlobHeader)) return fail("circuit blob too short");
  BlobHeader h;
  memcpy(&h, blob, sizeof h);
  if (h.magic != 0x46544344u /* 'DCTF' */ || h.version != 1) return fail("bad circuit blob magic/version");
  if (h.n_tensors < 1 || h.n_ops < 0 || h.n_tensors > (1 << 20) || h.n_ops > (1 << 20)) return fail("circuit blob: bad tensor/op count");
  const size_t need = sizeof h + (size_t)h.n_tensors * sizeof(TensorShape) + (size_t)h.n_ops * sizeof(Op);
  if (size < need) return fail("circuit blob truncated");
  auto bad_t = [&](int t) { return t < 0 || t >= h.n_tensors; };
  if (bad_t(h.input_tensor) || bad_t(h.output_tensor)) return fail("circuit blob: input/output tensor id out of range");
  c->tensors.resize(h.n_tensors);
  c->ops.assign(h.n_ops, SiteOp{});
  const char* p = (const char*)blob + sizeof h;
  memcpy(c->tensors.data(), p, (size_t)h.n_tensors * sizeof(TensorShape));
  p += (size_t)h.n_tensors * sizeof(TensorShape);
  c->input_tensor = h.input_tensor; c->output_tensor = h.output_tensor; c->max_bit_width = h.max_bit_width;
  for (const TensorShape& t : c->tensors)
    if (t.C < 1 || t.H < 1 || t.W < 1) return fail("circuit blob: empty tensor shape");
  for (int i = 0; i < h.n_ops; i++) {
    Op o;
    memcpy(&o, p + (size_t)i * sizeof(Op), sizeof o);
    if (o.type < OP_CONV || o.type > OP_MAXPOOL) return fail("op %d: unknown type %d", i, o.type);
    if (bad_t(o.src0) || bad_t(o.dst) || (o.type == OP_ADD && bad_t(o.src1))) return fail("op %d: tensor id out of range", i);
    if (o.payload_len < 0 || (o.payload_len > 0 && (o.payload_off < (int64_t)need || (size_t)o.payload_off + (size_t)o.payload_len > size)))
      return fail("op %d: payload out of range", i);
    SiteOp& site = c->ops[i];
    site.type = o.type; site.src0 = o.src0; site.src1 = o.src1; site.dst = o.dst; site.deff_in = o.ip[10];
    site.payload_off = o.payload_off; site.payload_len = o.payload_len;
    const TensorShape& a = c->tensors[o.src0];
    const TensorShape& d = c->tensors[o.dst];
    switch (o.type) {
      case OP_CONV: {
        const int Cout = o.ip[0], KH = o.ip[1], KW = o.ip[2], st = o.ip[3], pad = o.ip[4];
        if (Cout < 1 || KH < 1 || KW < 1 || st < 1 || pad < 0 || a.H + 2 * pad < KH || a.W + 2 * pad < KW) return fail("op %d: bad convolution geometry", i);
        if (d.C != Cout || d.H != (a.H + 2 * pad - KH) / st + 1 || d.W != (a.W + 2 * pad - KW) / st + 1) return fail("op %d: convolution output shape mismatch", i);
        if (o.payload_len != (int64_t)Cout * a.C * KH * KW) return fail("op %d: weight payload of %lld bytes, expected %lld", i, (long long)o.payload_len, (long long)Cout * a.C * KH * KW);
        site.conv = ConvSite{Cout, a.C, a.H, a.W, KH, KW, st, pad};
        break;
      }
      case OP_ADD: {
        const TensorShape& b2 = c->tensors[o.src1];
        if (a.C != b2.C || a.H != b2.H || a.W != b2.W || a.C != d.C || a.H != d.H || a.W != d.W) return fail("op %d: add operands differ in shape", i);
        break;
      }
      case OP_SUMPOOL: {
        const int K = site.sum_k = o.ip[0];
        if (K < 1 || d.C != a.C || d.H != a.H / K || d.W != a.W / K || d.H < 1 || d.W < 1) return fail("op %d: bad pooling geometry", i);
        break;
      }
      case OP_LUT: {
        LutSite& L = site.lut;
        L.p = o.ip[0]; L.r = o.ip[1]; L.w = o.ip[2]; L.shift = o.ip[3]; L.tab_tier = o.ip[4]; L.ntab = o.ip[6]; L.mode = o.ip[9];
        L.deff_in = o.ip[10]; L.body_add = (uint64_t)o.lp[0];
        L.steps.bit = o.ip[5]; L.steps.coarse = o.ip[7]; L.steps.coarse_from = o.ip[8];
        if (o.ip[11] >= 0) { L.steps.coarse2 = o.ip[11] >> 8; L.steps.coarse2_from = o.ip[11] & 255; }
        if (L.p < 1 || L.p > 62 || L.r < 0 || L.r >= L.p || L.w != L.p - L.r || L.shift < 0 || L.shift > 63)
          return fail("op %d: bad look-up precision (p=%d r=%d w=%d shift=%d)", i, L.p, L.r, L.w, L.shift);
        if (L.ntab != 1 && L.ntab != a.C) return fail("op %d: %d tables for %d channels", i, L.ntab, a.C);
        if (o.payload_len != ((int64_t)L.ntab << L.w) * 8) return fail("op %d: table payload of %lld bytes, expected %lld", i, (long long)o.payload_len, (long long)(((int64_t)L.ntab << L.w) * 8));
        if (a.C != d.C || a.H != d.H || a.W != d.W) return fail("op %d: look-up changes the shape", i);
        if (L.mode < LUT_EXACT || L.mode > LUT_SPLIT_QUIET) return fail("op %d: unknown look-up mode %d (0 exact, 1 approximate, 2 / 3 parity split)", i, L.mode);
        if (L.split()) {
          if (L.w < 2 || L.w > 16) return fail("op %d: a parity split needs a table of 2 to 16 input bits, not %d", i, L.w);
          if (L.steps.bit < 0) return fail("op %d: a parity split needs a bit tier", i);
          std::vector<int64_t> tmp((size_t)L.ntab << L.w);
          memcpy(tmp.data(), (const char*)blob + o.payload_off, (size_t)o.payload_len);
          if (split_tables_host(tmp.data(), (size_t)L.ntab, L.w, &site.halves)) return fail("op %d: parity split of a table whose entry pairs have an odd sum", i);
        }
        break;
      }
      case OP_MAXPOOL: {
        const PoolSite S = site.pool = PoolSite{o.ip[0], o.ip[1], o.ip[2], o.ip[3], o.ip[4], o.ip[5], o.ip[10], (uint64_t)o.lp[0]};
        if (S.k < 1 || S.k > 32 || S.stride < 1 || S.pad < 0 || 2 * S.pad > S.k || a.H + 2 * S.pad < S.k || a.W + 2 * S.pad < S.k)
          return fail("op %d: bad max-pool geometry (k=%d s=%d p=%d: need 1 <= k <= 32, s >= 1, 0 <= p <= k/2, window inside the padded input)", i, S.k, S.stride, S.pad);
        if (d.C != a.C) return fail("op %d: max pool changes the channel count (%d -> %d)", i, a.C, d.C);
        if (d.H != pool_out_size(a.H, S.k, S.stride, S.pad) || d.W != pool_out_size(a.W, S.k, S.stride, S.pad)) return fail("op %d: max-pool output shape mismatch", i);
        if (S.p_d < 2 || S.p_d > 16 || S.shift < 0 || S.p_d + S.shift > 63) return fail("op %d: bad max-pool difference precision (p_d=%d shift=%d)", i, S.p_d, S.shift);
        if (S.tier < 0 || S.tier >= DCTFHE_MAX_TIERS) return fail("op %d: max-pool tier %d out of range", i, S.tier);
        if (o.payload_len != ((int64_t)1 << S.p_d) * 8) return fail("op %d: max-pool table payload of %lld bytes, expected %lld", i, (long long)o.payload_len, (long long)(((int64_t)1 << S.p_d) * 8));
        break;
      }
    }
  }
  decode_slab_groups(c);
  return 0;
}

// per-image counts of a circuit under a parameter set (dctfhe_circuit_stats); a tier the parameters lack counts nothing
static int circuit_stats(const CircuitPlan& c, const dctfhe_params& P, dctfhe_stats* s) {
  memset(s, 0, sizeof *s);
  s->max_bit_width = c.max_bit_width;
  s->n_ops = (int)c.ops.size();
  const double Lb = (P.D + 1) * 8.0;
  auto tier_flops = [&](const dctfhe_tier& t) {
    const double N = (double)(1 << t.logN), M = N / 2;
    const double fft = 5.0 * M * std::log2(M);
    if (t.unroll == 2)   // per PAIR of key bits: the same transforms, three key blocks folded with their monomials (22 + 8 flops per
                         // point and key polynomial), the monomials themselves (18 per point)
      return (t.n / 2) * ((t.k + 1) * t.l * fft + (t.k + 1) * fft + (double)(t.k + 1) * (t.k + 1) * t.l * M * 30.0 + M * 18.0);
    return t.n * ((t.k + 1) * t.l * fft + (t.k + 1) * fft + (double)(t.k + 1) * (t.k + 1) * t.l * M * 8.0);
  };
  auto key_bytes = [&](const dctfhe_tier& t) {
    const double N = (double)(1 << t.logN);
    return (double)(t.unroll == 2 ? 3 * t.n / 2 : t.n) * t.l * (t.k + 1) * (t.k + 1) * N * 8.0 + (double)P.D * t.lk * (t.n + 1) * 8.0;
  };
  for (const SiteOp& o : c.ops) {
    const TensorShape& a = c.tensors[o.src0];
    const double ein = (double)a.elems(), eout = (double)c.tensors[o.dst].elems();
    double n = ein;      // bootstraps per entry of for_each_bootstrap
    switch (o.type) {
      case OP_CONV:
        s->conv_macs += (int64_t)(eout * o.conv.Cin * o.conv.KH * o.conv.KW);
        s->bytes_algorithmic += (ein + eout) * Lb;
        break;
      case OP_ADD: s->bytes_algorithmic += 3 * eout * Lb; break;
      case OP_SUMPOOL: s->bytes_algorithmic += (ein + eout) * Lb; break;
      case OP_LUT:
        s->lut_sites += (int64_t)ein;
        s->bit_steps += (int64_t)(ein * o.lut.n_steps());
        // the work rows once per bootstrap with a key switch of its own; a split: the parity rows and the second look-up's
        s->bytes_algorithmic += 2 * ein * Lb * (1 + o.lut.n_steps()) + (o.lut.split() ? 4 * ein * Lb : 0);
        break;
      case OP_MAXPOOL:
        n = (double)pool_pairs(a.C, a.H, a.W, o.pool.k, o.pool.stride, o.pool.pad);
        s->bytes_algorithmic += (ein + 3 * n) * Lb;     // gathers, and two rows read per difference
        break;
    }
    // a bootstrap that reuses another's small ciphertext has no key switch and streams no further key
    for_each_bootstrap(o, P, [&](int tier, int, bool own_ks) {
      if (tier < 0 || tier >= P.n_tiers) return;
      s->pbs_count[tier] += (int64_t)n;
      s->flops_f64 += n * tier_flops(P.tiers[tier]);
      if (own_ks) { s->ks_count[tier] += (int64_t)n; s->key_bytes_per_pass += key_bytes(P.tiers[tier]); }
    });
  }
  return 0;
}
