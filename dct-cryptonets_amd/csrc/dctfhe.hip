// dctfhe.hip -- host side of libdctfhe.so: contexts, key generation, the layer scheduler that walks a
// compiled circuit and issues batched HIP launches, and the C ABI of include/dctfhe.h.
// gfx950 only.  No CPU fallback anywhere: every entry point needs a live HIP device.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dctfhe.h"
#include "kernels.h"

using namespace dctfhe;

// ------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return fail("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)
#define CHK(x)              \
  do {                      \
    int r_ = (x);           \
    if (r_ != 0) return r_; \
  } while (0)

#include "circuit.h"   // the blob's wire structs, parse_circuit and the decoded sites: host-only, needs `fail`

extern "C" const char* dctfhe_last_error(void) { return g_err.c_str(); }
extern "C" int dctfhe_version(void) { return 1; }

// ------------------------------------------------------------------------------------------ structs
struct dctfhe_ctx {
  int device = 0;
  hipStream_t stream = nullptr, own = nullptr;
  hipDeviceProp_t prop;
  int max_grid_y = 0, max_grid_z = 0;      // hipDeviceAttributeMaxGridDimY / Z: what a launch grid may hold (dev_conv2d)
  ~dctfhe_ctx() { if (own) hipStreamDestroy(own); }
};

// The two owners: every piece of device memory and every event of the library is held by one of them, and nothing else frees any.
// g_dev_bytes: the bytes all live DevBufs were allocated with (dctfhe_device_bytes_live)
static std::atomic<size_t> g_dev_bytes{0};
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) { hipFree(p); g_dev_bytes -= bytes; }
    p = nullptr; bytes = 0;
  }
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipMalloc(&p, n ? n : 1);
    if (e != hipSuccess) { p = nullptr; return e; }
    bytes = n; g_dev_bytes += n;
    return e;
  }
  hipError_t upload(const void* host, size_t n) {      // alloc + blocking copy of a host operand
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemcpy(p, host, n, hipMemcpyHostToDevice);
  }
  hipError_t download(void* host, size_t n, hipStream_t st) const {      // what `st` computed into the first n bytes, to the host
    const hipError_t e = hipStreamSynchronize(st);
    return e != hipSuccess ? e : hipMemcpy(host, p, n, hipMemcpyDeviceToHost);
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept {
    if (this != &o) { reset(); e = o.e; o.e = nullptr; }
    return *this;
  }
  ~DevEvent() { reset(); }
  void reset() {
    if (e) hipEventDestroy(e);
    e = nullptr;
  }
  hipError_t create() { reset(); return hipEventCreate(&e); }
};
extern "C" size_t dctfhe_device_bytes_live(void) { return g_dev_bytes.load(); }

// a key-switch key and everything derived from it: made by the tier that owns it, read through TierKeys::ks by every tier that shares it
struct KskKey {
  DevBuf ksk;                    // u64 [D][lk][n+1]
  DevBuf colsum;                 // u64 [n+1], over all D*lk rows
  std::map<int, DevBuf> colsum_eff;   // ... over the first Deff*lk rows, filled on the first key switch at that Deff
  DevBuf kskT;                   // signed byte limbs, [limbs(n+1) padded to 128][D*lk], for the MFMA key switch (empty: integer-VALU GEMM)
  int ncol_pad = 0;
  int limbs = 8;                 // byte limbs kept per key word (ks_limbs): the key lives on the 2^-(8 limbs) torus grid
};
struct TierKeys {
  dctfhe_tier t{};
  KskKey* ks = nullptr;          // dctfhe_eval_keys::ksk[this tier], or [t.ksk_share]
  DevBuf bsk;                    // cplx [n][rows][k+1][P][T]; unroll 2: [3n/2 blocks] for the pair secret
  DevBuf wtab;                   // cplx, unroll 2: e^{i pi m/N}, m < 2N, then e^{2 pi i k/8}, k < 8
  DevBuf tw;                     // cplx
  bool mfma() const { return ks->kskT.p != nullptr; }
};

// CLIENT side: everything secret.  The whole handle is a function of (params, 32-byte seed): persist the seed to persist it.
struct dctfhe_client_key {
  dctfhe_ctx* ctx = nullptr;
  dctfhe_params p{};
  uint8_t seed[32] = {};
  rng_key sec{}, pub{};          // ChaCha20 keys: secret (key bits, noise) and public (masks)
  // ENCRYPTION randomness is per HANDLE, not per seed: its two generator keys are derived from the seed AND a 128-bit nonce drawn from
  // the OS when the handle is created.  (Key material stays a pure function of the seed.  Before, a client that re-created its key from
  // the persisted seed -- or a second process holding the seed -- re-drew the very masks and noise of earlier ciphertexts: ct1 - ct2 =
  // (0, m1 - m2).  ADVICE r2.)
  uint8_t nonce[16] = {};
  rng_key enc_sec{}, enc_pub{};
  DevBuf d_S, d_s;               // key bits, one byte each
  DevBuf d_spair[DCTFHE_MAX_TIERS];          // unroll 2: derived secret (s1(1-s2), (1-s1)s2, s1 s2) per pair
  uint64_t enc_calls = 0;        // every dctfhe_encrypt call draws from fresh streams
  const uint8_t* S() const { return d_S.as<uint8_t>(); }
  const uint8_t* s() const { return d_s.as<uint8_t>(); }
  ~dctfhe_client_key() { if (ctx) hipSetDevice(ctx->device); }      // ... before the members free themselves
};

// SERVER side: evaluation keys only (key-switch keys, Fourier bootstrap keys); nothing here depends on the secret at run time.
struct dctfhe_eval_keys {
  dctfhe_ctx* ctx = nullptr;
  dctfhe_params p{};
  KskKey ksk[DCTFHE_MAX_TIERS];  // per tier with a key-switch key of its own (ksk_share < 0)
  TierKeys tiers[DCTFHE_MAX_TIERS];
  dctfhe_key_tiers sel{};        // which tiers' keys are held (closed; key_tiers_full: every one).  An absent key has no allocation at all
  DevBuf d_dummy;                // D+1 words, sink of padded bootstrap groups
  ~dctfhe_eval_keys() { if (ctx) hipSetDevice(ctx->device); }
};
using dctfhe_keys = dctfhe_eval_keys;   // the server-side code below says K for the evaluation keys

// What a handle is bound to (include/dctfhe.h): keys and sessions to the CONTEXT they were made on -- the device code launches on the
// handle's context's stream while the entry point copies and synchronises on the caller's, and nothing orders two contexts' streams --
// a circuit to its DEVICE.  Every entry point that is given a context and a handle calls this before it allocates, copies or launches.
static int bound_to(const char* who, const dctfhe_ctx* ctx, const dctfhe_ctx* made_on, const char* what) {
  if (ctx != made_on) return fail("%s: the %s belongs to another context than the one the call names", who, what);
  return 0;
}

// a convolution's weights as the i8 MFMA kernel wants them: [Cout padded to 64][K padded to 32] K-contiguous, and per k the
// input plane offset and the tap displacement (kernels.h k_conv2d_mfma)
struct ConvPack {
  int8_t* d_w = nullptr;
  conv_tap* d_taps = nullptr;
  int kpad = 0;
};
static void conv_pack_sizes(int Cout, int Cin, int KH, int KW, size_t* wbytes, size_t* tbytes, int* kpad) {
  const int K = Cin * KH * KW;
  *kpad = (K + 31) / 32 * 32;
  *wbytes = ((size_t)((Cout + 63) / 64 * 64) * *kpad + 255) / 256 * 256;
  *tbytes = ((size_t)*kpad * sizeof(conv_tap) + 255) / 256 * 256;
}
// fills host images of the packed weights / tap table (sizes from conv_pack_sizes)
static void pack_conv_host(const int8_t* w, int Cout, int Cin, int H, int W, int KH, int KW, int pad, int kpad, int8_t* wp, conv_tap* tp) {
  const int K = Cin * KH * KW;
  for (int co = 0; co < Cout; co++) memcpy(wp + (size_t)co * kpad, w + (size_t)co * K, (size_t)K);
  for (int k = 0; k < kpad; k++) {
    if (k >= K) { tp[k] = conv_tap{-1, 0, 0}; continue; }
    const int ci = k / (KH * KW), r = k % (KH * KW);
    tp[k] = conv_tap{ci * H * W, (int16_t)(r / KW - pad), (int16_t)(r % KW - pad)};
  }
}
// every pack of a circuit (or the single one of the dctfhe_conv2d primitive) lives in ONE device allocation
static int build_conv_packs(const std::vector<const int8_t*>& w, const std::vector<ConvSite>& g, DevBuf* slab, std::vector<ConvPack>* out) {
  size_t total = 0;
  std::vector<size_t> off_w(w.size()), off_t(w.size());
  out->assign(w.size(), ConvPack{});
  for (size_t i = 0; i < w.size(); i++) {
    if (!w[i]) continue;
    size_t wb, tb;
    conv_pack_sizes(g[i].Cout, g[i].Cin, g[i].KH, g[i].KW, &wb, &tb, &(*out)[i].kpad);
    off_w[i] = total; total += wb;
    off_t[i] = total; total += tb;
  }
  if (!total) return 0;
  std::vector<char> host(total, 0);
  for (size_t i = 0; i < w.size(); i++)
    if (w[i]) pack_conv_host(w[i], g[i].Cout, g[i].Cin, g[i].H, g[i].W, g[i].KH, g[i].KW, g[i].pad, (*out)[i].kpad, (int8_t*)&host[off_w[i]], (conv_tap*)&host[off_t[i]]);
  HIPCHK(slab->upload(host.data(), total));
  for (size_t i = 0; i < w.size(); i++)
    if (w[i]) { (*out)[i].d_w = slab->as<int8_t>() + off_w[i]; (*out)[i].d_taps = (conv_tap*)(slab->as<char>() + off_t[i]); }
  return 0;
}

struct dctfhe_circuit : CircuitPlan {      // tensors, ops (one decoded SiteOp per record), input / output tensor
  dctfhe_ctx* ctx = nullptr;
  int device = 0;                // a circuit belongs to a device, not to a context: its payload is uploaded once and read-only afterwards
  std::vector<DevBuf> d_payload; // per op, device copy of its payload (weights / tables)
  std::vector<DevBuf> d_split;   // per op: the half tables [S | Dt] of a parity-split look-up, each i64 [ntab][2^(w-1)] (empty for other ops)
  std::vector<ConvPack> conv;    // per op: the matrix-core form of a convolution's weights (empty for other ops)
  DevBuf conv_slab;              // ... all of them in one allocation, made when the first encrypted session is created
  std::vector<std::vector<int8_t>> conv_w;          // host copies of the convolution weights until then
  ~dctfhe_circuit() { if (ctx) hipSetDevice(device); }
};

// ---- max pool (OP_MAXPOOL): separable passes, rows then columns; each pass a log-depth tree of pairwise maxima
// max(a, b) = b + relu(a - b) over the window's in-range taps.  Late pairing: a pass of L = ceil(log2 max taps) levels; at level l an
// output with m candidates combines its first 2 * max(0, m - 2^(L-l-1)) candidates pairwise (a = the even one, b = the odd one) and
// carries the rest, so every output reaches one candidate at the last level (dctfhe/compile.py pool_level_pairs is the same rule).  A
// level writes its output rows as [pair results in output order][carried candidates in output order]: the gather copies each pair's b
// (and each carried row) there, and the difference bootstraps accumulate into the first `pairs` rows -- one contiguous batch.
struct PoolLevel {
  int src, dst;            // 0: the op's input, 1 / 2: level buffers A / B, 3: the op's output
  size_t n_dst, pairs;     // rows written; the first `pairs` of them take a bootstrap
  size_t g_off, a_off, b_off;   // int32 offsets into PoolPlan::maps: gather map [n_dst], ia / ib [pairs] (rows of the source)
};
struct PoolPlan {
  std::vector<PoolLevel> lv;
  size_t rows_buf[2] = {0, 0};  // rows of level buffers A and B
  size_t pairs_per_batch = 0;
  // the output rows the plan computes (all of them unless the pool is divided), the smallest range of source rows that holds every tap
  // it reads, and the range of row-pass results [B*C*H][Wo] that holds its intermediates (the clear-mode `mid` buffer)
  size_t out_first = 0, out_count = 0, in_first = 0, in_count = 0, mid_first = 0, mid_count = 0;
  DevBuf maps;
};
// range == nullptr: the whole op, every row-pass result computed.  range = {first, count}: a divided pool's part (dctfhe_shard_pool) -- the
// output rows [first, first + count) of [B][C][Ho][Wo], and of the row pass only the results (b, c, y, xo) that the column pass of one of
// these outputs reads.  An output (and an intermediate) has the candidates and the level count of the whole op, so it goes through the very
// pairings of the undivided tree.  Map entries into the op's input are global rows; level buffers are numbered from 0 for the part; the last
// level (or the extra gather) writes output row out_first + i.  Host only: `maps` is what PoolPlan::maps holds on the device.
static int pool_plan_host(int batch, int C, int H, int W, int k, int s, int p, const size_t* range, PoolPlan* P, std::vector<int32_t>* maps_out) {
  const int Ho = pool_out_size(H, k, s, p), Wo = pool_out_size(W, k, s, p);
  if ((double)batch * C * H * W >= 2147483647.0) return fail("max pool: %d x %d x %d x %d rows exceed the int32 index maps", batch, C, H, W);
  const size_t n_out = (size_t)batch * C * Ho * Wo, n_mid = (size_t)batch * C * H * Wo;
  const size_t o0 = range ? range[0] : 0, on = range ? range[1] : n_out;
  if (o0 > n_out || on > n_out - o0) return fail("max pool: output rows %zu .. %zu of %zu", o0, o0 + on, n_out);
  P->out_first = o0; P->out_count = on;
  std::vector<int32_t>& maps = *maps_out;
  std::vector<std::vector<int32_t>> cand;      // per output of the current pass: its candidates' rows in the current source buffer
  int cur = 0;                                 // buffer the candidates live in
  int next_buf = 1;
  // one 1-D pass [outer][n_in][inner] -> [outer][n_out][inner] for the outputs `ids` (ascending numbers in the whole pass output);
  // row_of(element of the pass input) -> its row in buffer `cur`
  auto run_pass = [&](const std::vector<size_t>& ids, int n_in, int inner, int n_out1, auto&& row_of) {
    const size_t nout = ids.size();
    cand.assign(nout, {});
    int mmax = 1;                              // over the whole pass, not the part: the level count is the undivided tree's
    for (int o = 0; o < n_out1; o++) {
      int m = 0;
      for (int j = 0; j < k; j++) m += (o * s - p + j >= 0 && o * s - p + j < n_in) ? 1 : 0;
      mmax = std::max(mmax, m);
    }
    for (size_t q = 0; q < nout; q++) {
      const size_t e = ids[q];
      const int i = (int)(e % inner), o = (int)((e / inner) % n_out1);
      const size_t ou = e / ((size_t)inner * n_out1);
      for (int j = 0; j < k; j++) {
        const int x = o * s - p + j;
        if (x >= 0 && x < n_in) cand[q].push_back(row_of((ou * n_in + x) * inner + i));
      }
    }
    int L = 0;
    while ((1 << L) < mmax) L++;
    for (int lev = 0; lev < L; lev++) {
      const int cap = 1 << (L - lev - 1);
      PoolLevel pl{cur, next_buf, 0, 0, maps.size(), 0, 0};
      std::vector<int32_t> g, ia, ib, carried_src;
      std::vector<std::pair<size_t, int>> carried;     // (output, index into its candidates)
      std::vector<std::vector<int32_t>> nc(nout);
      for (size_t e = 0; e < nout; e++) {
        const int m = (int)cand[e].size(), pr = m > cap ? m - cap : 0;
        for (int q = 0; q < pr; q++) {
          nc[e].push_back((int32_t)g.size());
          g.push_back(cand[e][2 * q + 1]);
          ia.push_back(cand[e][2 * q]);
          ib.push_back(cand[e][2 * q + 1]);
        }
        for (int q = 2 * pr; q < m; q++) carried.push_back({e, cand[e][q]});
      }
      pl.pairs = g.size();
      for (auto& c : carried) { nc[c.first].push_back((int32_t)g.size()); g.push_back(c.second); }
      pl.n_dst = g.size();
      maps.insert(maps.end(), g.begin(), g.end());
      pl.a_off = maps.size(); maps.insert(maps.end(), ia.begin(), ia.end());
      pl.b_off = maps.size(); maps.insert(maps.end(), ib.begin(), ib.end());
      P->lv.push_back(pl);
      cand.swap(nc);
      cur = next_buf;
      next_buf = 3 - next_buf;
    }
  };
  // the row-pass results to compute: all of them, or those under the windows of the part's outputs
  auto col_taps = [&](size_t e, auto&& f) {
    const size_t xo = e % Wo, yo = (e / Wo) % Ho, bc = e / ((size_t)Wo * Ho);
    for (int j = 0; j < k; j++) {
      const int y = (int)yo * s - p + j;
      if (y >= 0 && y < H) f((bc * H + (size_t)y) * Wo + xo);
    }
  };
  std::vector<size_t> mids, outs(on);
  for (size_t q = 0; q < on; q++) outs[q] = o0 + q;
  if (!range) {
    mids.resize(n_mid);
    for (size_t m = 0; m < n_mid; m++) mids[m] = m;
  } else if (on) {
    size_t lo = n_mid, hi = 0;
    for (size_t e : outs) col_taps(e, [&](size_t m) { lo = std::min(lo, m); hi = std::max(hi, m); });
    std::vector<char> read(hi - lo + 1, 0);
    for (size_t e : outs) col_taps(e, [&](size_t m) { read[m - lo] = 1; });
    for (size_t m = lo; m <= hi; m++) if (read[m - lo]) mids.push_back(m);
  }
  if (!mids.empty()) { P->mid_first = mids.front(); P->mid_count = mids.back() - mids.front() + 1; }
  // row pass: [B*C*H][W] -> [B*C*H][Wo], on the op's input in place
  size_t in_lo = (size_t)-1, in_hi = 0;
  run_pass(mids, W, 1, Wo, [&](size_t r) { in_lo = std::min(in_lo, r); in_hi = std::max(in_hi, r); return (int32_t)r; });
  if (!mids.empty()) { P->in_first = in_lo; P->in_count = in_hi - in_lo + 1; }
  std::vector<int32_t> mid_row(P->mid_count, -1);      // row-pass result -> its row in buffer `cur`
  for (size_t q = 0; q < mids.size(); q++) mid_row[mids[q] - P->mid_first] = cand[q][0];
  // column pass on the row pass's output: [B*C][H][Wo] -> [B*C][Ho][Wo]
  run_pass(outs, H, Wo, Ho, [&](size_t m) { return mid_row[m - P->mid_first]; });
  // the op's output is in output order: the last level already wrote it so when every output ended on its own row; else one more gather
  bool identity = !P->lv.empty();
  for (size_t e = 0; e < cand.size() && identity; e++) identity = cand[e][0] == (int32_t)e;
  if (identity) {
    P->lv.back().dst = 3;
  } else {
    PoolLevel pl{cur, 3, cand.size(), 0, maps.size(), 0, 0};
    for (size_t e = 0; e < cand.size(); e++) maps.push_back(cand[e][0]);
    pl.a_off = pl.b_off = maps.size();
    P->lv.push_back(pl);
  }
  P->rows_buf[0] = P->rows_buf[1] = 0;
  for (const PoolLevel& l : P->lv)
    if (l.dst == 1 || l.dst == 2) P->rows_buf[l.dst - 1] = std::max(P->rows_buf[l.dst - 1], l.n_dst);
  for (const PoolLevel& l : P->lv) P->pairs_per_batch += l.pairs;
  // the gather and the key switch read through the maps unchecked: every entry is a row of the op's input, or a row the level before wrote
  size_t written[3] = {(size_t)batch * C * H * W, 0, 0};
  for (const PoolLevel& l : P->lv) {
    auto outside = [&](size_t off, size_t n) {
      for (size_t q = 0; q < n; q++)
        if (maps[off + q] < 0 || (size_t)maps[off + q] >= written[l.src]) return true;
      return false;
    };
    if (outside(l.g_off, l.n_dst) || outside(l.a_off, l.pairs) || outside(l.b_off, l.pairs)) return fail("max pool: an index map entry outside its source buffer");
    if (l.dst < 3) written[l.dst] = l.n_dst;
  }
  return 0;
}
static int pool_plan(int batch, int C, int H, int W, int k, int s, int p, const size_t* range, PoolPlan* P) {
  std::vector<int32_t> maps;
  CHK(pool_plan_host(batch, C, H, W, k, s, p, range, P, &maps));
  HIPCHK(P->maps.alloc(maps.size() * 4));
  if (!maps.empty()) HIPCHK(hipMemcpy(P->maps.p, maps.data(), maps.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

// key-switch digits and bodies, small ciphertexts and the 64 single-entry tables 2^j of the one-bit steps, for `chunk` ciphertexts at a time
struct LutScratch {
  DevBuf d_digits, d_bodies, d_small, d_bit_tables;
  size_t chunk = 0;
  uint8_t* digits() const { return d_digits.as<uint8_t>(); }
  uint64_t* bodies() const { return d_bodies.as<uint64_t>(); }
  uint64_t* small() const { return d_small.as<uint64_t>(); }
  const int64_t* bit_tables() const { return d_bit_tables.as<int64_t>(); }
};

struct dctfhe_session {
  dctfhe_ctx* ctx = nullptr;
  dctfhe_circuit* circ = nullptr;
  dctfhe_keys* keys = nullptr;  // nullptr: clear mode (D = 0)
  int batch = 0;
  int D = 0;
  std::vector<uint64_t*> d_tensor;
  std::vector<DevBuf> owned;        // the planner's allocations; d_tensor and pool_buf point into them
  std::vector<size_t> tensor_words;
  // encrypted tensors are stored at their effective dimension: row stride t_L[t] words = t_L[t]-1 mask words + the body;
  // t_deff[t] <= t_L[t]-1 is how many leading mask words may be non-zero.  Clear mode: one word per element.
  std::vector<size_t> t_L, t_deff;
  LutScratch lut;                   // scratch for LUT sites
  DevBuf d_overflow;                // one int
  // `simulate`: per-op noise (fraction of the torus) injected by the clear look-up kernel; empty = noise-free
  std::vector<double> sim_sigma;
  std::vector<double> sim_sigma2;   // parity-split sites: the second look-up's (0 or absent: the first one's)
  uint64_t sim_seed = 0, sim_run = 0;
  // timing: events are created once and reused by every run; bootstraps per tier and image are fixed by the circuit
  std::vector<DevEvent> ev_pool;
  int64_t pbs_per_image[DCTFHE_MAX_TIERS] = {};
  // per op: the tree of a max pool (index maps in device memory) and its two level buffers (planner-owned, reused after the op)
  std::vector<std::unique_ptr<PoolPlan>> pool;
  std::vector<std::array<uint64_t*, 2>> pool_buf;
  // margin audit (dctfhe_session_set_audit): off unless d_audit_key is set.  The session's own copy of the small key, one slot per
  // (op, bootstrap with a key switch of its own) on the device, their fixed fields, each op's first slot, and the last run's slots
  DevBuf d_audit_key, d_audit;      // bytes of the small key; margin_slot per slot
  std::vector<dctfhe_margin_stats> audit_slots, audit_last;
  std::vector<int> audit_first;
  // sharded look-up sites (dctfhe_session_set_shard): this session is part `part` of `parts`; whole[t] = 0: only this part's rows of
  // tensor t are valid.  (0, 1), the default: every tensor is whole at all times
  int part = 0, parts = 1;
  bool has_run = false;
  std::vector<char> whole;
  // divided max pools (dctfhe_session_set_shard_pool): a pool computes the part's output rows and reads only its need range of the source,
  // so a sliced tensor may hold more valid rows than the part's own: marked[t], the ranges (first, end) dctfhe_session_mark_rows declared
  bool shard_set = false, shard_pool = false;
  std::vector<std::vector<std::pair<size_t, size_t>>> marked;
  std::vector<size_t> pool_pairs_run;   // per op: pairwise maxima its last run sent to the bootstrap (max pools; 0 elsewhere)
  // memory budget (dctfhe_session_set_memory_budget): slab[g] = channels of slab group g that exist at a time; divided_group[op] = the op's
  // group when it is divided, else -1; pool_last[op]: the tree of the shorter last slab of a max pool in a divided group
  std::vector<int> slab, divided_group;
  std::vector<std::unique_ptr<PoolPlan>> pool_last;
  size_t budget_bytes = 0, planned_bytes = 0, undivided_bytes = 0;
  std::vector<int> circ_heights() const { std::vector<int> h; for (const SlabGroup& G : circ->groups) h.push_back(G.channels); return h; }      // the undivided heights
  void wipe_audit_key() {      // the secret does not outlive the audit: cleared on the context's stream, and done before the buffer is freed
    if (!d_audit_key.p) return;
    hipMemsetAsync(d_audit_key.p, 0, d_audit_key.bytes, ctx->stream);
    hipStreamSynchronize(ctx->stream);
  }
  void audit_off() {
    wipe_audit_key();
    d_audit_key.reset(); d_audit.reset();
    audit_slots.clear(); audit_last.clear(); audit_first.clear();
  }
  ~dctfhe_session() {
    if (ctx) hipSetDevice(ctx->device);
    wipe_audit_key();
  }
};

// ------------------------------------------------------------------------------------------ kernel dispatch
// (logN, k, l, points per thread).  8 points per thread keep the register arrays under 256 VGPRs, i.e. 2 waves
// per SIMD (measured 1.6x over 16 points per thread at 1 wave per SIMD); GROUPS packs ciphertexts up to 256
// threads per workgroup, so that two workgroups share a CU (N = 8192 needs all 512 threads for one ciphertext).
#define PBS_CASES(X)                                                                                 \
  X(8, 2, 2, 8) X(9, 1, 2, 16) X(9, 1, 3, 8) X(10, 1, 1, 8) X(10, 1, 2, 8) X(10, 2, 1, 8) X(10, 2, 2, 8)  \
  X(11, 1, 1, 8) X(11, 1, 2, 8) X(11, 1, 3, 8) X(12, 1, 1, 8) X(12, 1, 2, 8) X(12, 1, 3, 8)           \
  X(13, 1, 1, 8) X(13, 1, 2, 8) X(13, 1, 3, 8) X(11, 1, 4, 8)

// two-bit blind rotation (tier.unroll == 2): k = 1, one level
#define PBS_MB_CASES(X) X(11) X(12) X(13)

template <int LOGN, int K_, int L_, int P>
constexpr int groups_for() {
  using G = pbs_geom<LOGN, K_, L_, P>;
  constexpr int by_lds = (160 * 1024 - G::TW_BYTES) / G::GROUP_BYTES;
  int g = G::T >= 256 ? 1 : 256 / G::T;   // two 256-thread workgroups per CU beat one of 512 (+10..20%, profiles/r01_exp_wg.log)
  while (g > 1 && g > by_lds) g >>= 1;
  // ... and when two such workgroups do not fit the LDS together (both mask polynomials of a k = 2, l = 2 tier live there),
  // smaller workgroups keep the CU at two waves per SIMD
  while (g > 1 && 2 * (G::TW_BYTES + g * G::GROUP_BYTES) > 160 * 1024) g >>= 1;
  return g;
}

// The duo tier: the general two-bit form at N = 2048, k = 1, three levels (T4r2) runs two ciphertexts per group of M / 4 threads
// (pbs_kernel_duo), so its transforms -- the bootstrap's and the key's -- keep P = 4 points per thread and the device holds its
// Fourier key in the P = 4 order.  The evaluation-key blob keeps the one documented order (include/dctfhe.h: P = 8 for this shape):
// export and import permute the entries of each polynomial, frequency for frequency.
static bool tier_duo(const dctfhe_tier& t) { return t.logN == 11 && t.k == 1 && t.l == 3 && t.unroll == 2; }
constexpr int DUO_LOGN = 11, DUO_P = 4, DUO_BLOB_P = 8, DUO_M = 1 << (DUO_LOGN - 1);
// blob entry (j T + t of the P = 8 transform) -> device entry (of the P = 4 transform) that holds the same frequency
static const std::vector<uint16_t>& duo_entry_map() {
  static const std::vector<uint16_t> map = [] {
    std::vector<uint16_t> by_freq(DUO_M), m(DUO_M);
    constexpr int T4 = DUO_M / DUO_P, T8 = DUO_M / DUO_BLOB_P;
    for (int e = 0; e < DUO_M; e++) by_freq[spectrum_freq<DUO_LOGN - 1, DUO_P>(DUO_P * (e % T4) + e / T4)] = (uint16_t)e;
    for (int e = 0; e < DUO_M; e++) m[e] = by_freq[spectrum_freq<DUO_LOGN - 1, DUO_BLOB_P>(DUO_BLOB_P * (e % T8) + e / T8)];
    return m;
  }();
  return map;
}
// npoly polynomials of M entries: blob order -> device order (to_device) or back; src and dst must not overlap
static void duo_permute(const cplx* src, cplx* dst, size_t npoly, bool to_device) {
  const std::vector<uint16_t>& m = duo_entry_map();
  for (size_t q = 0; q < npoly; q++) {
    const cplx* a = src + q * DUO_M;
    cplx* b = dst + q * DUO_M;
    if (to_device) for (int e = 0; e < DUO_M; e++) b[m[e]] = a[e];
    else           for (int e = 0; e < DUO_M; e++) b[e] = a[m[e]];
  }
}

static int tier_ppt(const dctfhe_tier& t) {
#define X(LN, K_, L_, P_) if (t.logN == LN && t.k == K_ && t.l == L_) return P_;
  PBS_CASES(X)
#undef X
  return 0;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the function on the CURRENT device: once per (call site, device), not once
// per process (a process with contexts on two GPUs would have failed on the second at every launch above 64 KB of LDS)
#define SET_LDS_ATTR(kernel, bytes)                                                                  \
  do {                                                                                               \
    static std::atomic<uint64_t> done_mask{0};      /* contexts of several host threads launch through one call site */ \
    int dev_ = 0;                                                                                    \
    HIPCHK(hipGetDevice(&dev_));                                                                     \
    if (dev_ < 0 || dev_ >= 64 || !((done_mask.load() >> dev_) & 1)) {                               \
      HIPCHK(hipFuncSetAttribute((const void*)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
      if (dev_ >= 0 && dev_ < 64) done_mask.fetch_or(1ull << dev_);                                  \
    }                                                                                                \
  } while (0)

// one bootstrap kernel, GR ciphertexts per workgroup
template <int LN, int K, int L, int P, int GR, int MB = 0>
static int launch_pbs_as(const pbs_launch& a, hipStream_t st) {
  const size_t lds = pbs_lds_bytes<LN, K, L, P, MB>(GR);
  SET_LDS_ATTR((pbs_kernel<LN, K, L, P, GR, MB>), lds);
  const unsigned grid = (unsigned)((a.count + GR - 1) / GR);
  hipLaunchKernelGGL((pbs_kernel<LN, K, L, P, GR, MB>), dim3(grid), dim3(pbs_geom<LN, K, L, P, MB>::T * GR), lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// the duo form: DUOS groups of two ciphertexts per workgroup
template <int LN, int K, int L, int P, int DUOS>
static int launch_pbs_as_duo(const pbs_launch& a, hipStream_t st) {
  const size_t lds = pbs_duo_lds_bytes<LN, K, L, P>(DUOS);
  static_assert(pbs_duo_lds_bytes<LN, K, L, P>(DUOS) <= 160 * 1024, "LDS of one CU");
  SET_LDS_ATTR((pbs_kernel_duo<LN, K, L, P, DUOS>), lds);
  const unsigned grid = (unsigned)((a.count + 2 * DUOS - 1) / (2 * DUOS));
  hipLaunchKernelGGL((pbs_kernel_duo<LN, K, L, P, DUOS>), dim3(grid), dim3(pbs_geom<LN, K, L, P, 1>::T * DUOS), lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

static int launch_pbs(const dctfhe_tier& t, const pbs_launch& a, hipStream_t st) {
  if (a.count == 0) return 0;
  // the kernel's L2 warm-up contract (pbs_core.h): callers pad the key by PBS_PF_DIST iterations (eval_alloc does)
  if (a.pf_parts != 0 && a.pf_parts < 8) return fail("bootstrap launch: pf_parts must be 0 or >= 8 (got %d)", a.pf_parts);
  if (!a.bsk || !a.tw || !a.cts_small || !a.out || !a.dummy || (t.unroll == 2 && !a.wtab)) return fail("bootstrap launch: null operand");
  if (a.w < 0 || a.w > t.logN - 1) return fail("bootstrap launch: table of 2^%d entries does not fit N = 2^%d", a.w, t.logN);
#define X(LN, K_, L_, P_) \
  if (t.logN == LN && t.k == K_ && t.l == L_ && t.unroll == 1) return launch_pbs_as<LN, K_, L_, P_, groups_for<LN, K_, L_, P_>()>(a, st);
  PBS_CASES(X)
#undef X
  // N = 4096: two ciphertexts per 512-thread workgroup share their key lines (28.5 vs 30.8 ms)
#define X(LN) \
  if (t.logN == LN && t.k == 1 && t.l == 1 && t.unroll == 2) return launch_pbs_as<LN, 1, 1, 8, (LN == 12 ? 2 : groups_for<LN, 1, 1, 8>()), 1>(a, st);
  PBS_MB_CASES(X)
#undef X
  // the general form of the two-bit rotation (one polynomial at a time, monomial factors rebuilt per gadget row), four
  // ciphertexts per 512-thread workgroup so that they share their key lines: 74.2 ms per 4096 against 82.3 for the one-bit
  // chain of the same tier (profiles/r02_exp_ablations.log); its output is 0.7 bit noisier, so the compiler only uses it
  // where the circuit's budget allows (dctfhe/params.py T4r2).  As two duos: every loaded key value is folded into two
  // ciphertexts (pbs_core.h pbs_thread_duo; profiles/t4r2_duo_ab.json).  pbs_kernel<11, 1, 3, 8, 4, 1>, the form it replaces,
  // still builds in tools/exp_pbs.hip.
  static_assert(DUO_LOGN == 11 && DUO_P == 4, "tier_duo names this kernel's shape");
  if (t.logN == 11 && t.k == 1 && t.l == 3 && t.unroll == 2) return launch_pbs_as_duo<11, 1, 3, 4, 2>(a, st);
  // general two-bit rotation for the one-level bit tier (Ba2): one wave per ciphertext, four per workgroup
  if (t.logN == 10 && t.k == 2 && t.l == 1 && t.unroll == 2) return launch_pbs_as<10, 2, 1, 8, 4, 1>(a, st);
  return fail("no bootstrap kernel instantiated for logN=%d k=%d l=%d unroll=%d", t.logN, t.k, t.l, t.unroll);
}

static int make_twiddles(const dctfhe_tier& t, std::vector<cplx>& tw) {
  if (tier_duo(t)) {
    tw.resize(fft_geom<DUO_LOGN - 1, DUO_P>::TW_ELEMS);
    fill_twiddles<DUO_LOGN - 1, DUO_P>(tw.data());
    return 0;
  }
#define X(LN, K_, L_, P_)                                        \
  if (t.logN == LN && t.k == K_ && t.l == L_) {                  \
    tw.resize(fft_geom<LN - 1, P_>::TW_ELEMS);                   \
    fill_twiddles<LN - 1, P_>(tw.data());                        \
    return 0;                                                    \
  }
  PBS_CASES(X)
#undef X
  return fail("no bootstrap kernel instantiated for logN=%d k=%d l=%d", t.logN, t.k, t.l);
}

static int launch_bsk_fourier(const dctfhe_tier& t, const uint64_t* polys, size_t npoly, const cplx* tw, cplx* out, hipStream_t st) {
  if (tier_duo(t)) {      // straight into the device order of the duo kernel: one polynomial per workgroup of M / 4 threads
    using F = fft_geom<DUO_LOGN - 1, DUO_P>;
    const size_t lds = (size_t)F::TW_ELEMS * 16 + (size_t)F::EXCH_ELEMS * 16;
    SET_LDS_ATTR((k_bsk_fourier<DUO_LOGN, DUO_P, 1>), lds);
    hipLaunchKernelGGL((k_bsk_fourier<DUO_LOGN, DUO_P, 1>), dim3((unsigned)npoly), dim3(F::T), lds, st, polys, npoly, tw, out);
    HIPCHK(hipGetLastError());
    return 0;
  }
#define X(LN, K_, L_, P_)                                                                            \
  if (t.logN == LN && t.k == K_ && t.l == L_) {                                                      \
    using F = fft_geom<LN - 1, P_>;                                                                  \
    constexpr int GR = groups_for<LN, K_, L_, P_>();                                                 \
    const size_t lds = (size_t)F::TW_ELEMS * 16 + (size_t)GR * F::EXCH_ELEMS * 16;                   \
    SET_LDS_ATTR((k_bsk_fourier<LN, P_, GR>), lds);                                                  \
    const unsigned grid = (unsigned)((npoly + GR - 1) / GR);                                         \
    hipLaunchKernelGGL((k_bsk_fourier<LN, P_, GR>), dim3(grid), dim3(F::T * GR), lds, st, polys, npoly, tw, out); \
    HIPCHK(hipGetLastError());                                                                       \
    return 0;                                                                                        \
  }
  PBS_CASES(X)
#undef X
  return fail("no bootstrap kernel instantiated for logN=%d k=%d l=%d", t.logN, t.k, t.l);
}

// ------------------------------------------------------------------------------------------ context
extern "C" int dctfhe_ctx_create(int device_id, dctfhe_ctx** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail("dctfhe: no HIP device visible -- this engine has no CPU path");
  if (device_id < 0 || device_id >= ndev) return fail("dctfhe: device %d out of range (%d visible)", device_id, ndev);
  HIPCHK(hipSetDevice(device_id));
  std::unique_ptr<dctfhe_ctx> c(new dctfhe_ctx);
  c->device = device_id;
  HIPCHK(hipGetDeviceProperties(&c->prop, device_id));
  HIPCHK(hipDeviceGetAttribute(&c->max_grid_y, hipDeviceAttributeMaxGridDimY, device_id));
  HIPCHK(hipDeviceGetAttribute(&c->max_grid_z, hipDeviceAttributeMaxGridDimZ, device_id));
  HIPCHK(hipStreamCreate(&c->own));
  c->stream = c->own;
  *out = c.release();
  return 0;
}
extern "C" int dctfhe_ctx_destroy(dctfhe_ctx* c) {
  if (!c) return 0;
  hipSetDevice(c->device);
  delete c;
  return 0;
}
extern "C" int dctfhe_ctx_set_stream(dctfhe_ctx* c, void* s) {
  c->stream = s ? (hipStream_t)s : c->own;
  return 0;
}
extern "C" int dctfhe_ctx_synchronize(dctfhe_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------ keygen
static int check_params(const dctfhe_params* p) {
  // this is the only gate in front of an untrusted evaluation-key blob (dctfhe_eval_keys_import): every field gets both bounds, and
  // the caps keep every size computed from them (eval_blob_size, key allocations) far inside size_t
  if (p->n_tiers < 1 || p->n_tiers > DCTFHE_MAX_TIERS) return fail("n_tiers out of range");
  if (p->D < 4 || p->D % 4 || p->D > (1 << 16)) return fail("D must be a positive multiple of 4, at most 65536");
  if (p->n_max < 1 || p->n_max > (1 << 13)) return fail("n_max out of range (1 .. 8192)");
  if (p->input_dim < 0 || p->input_dim > p->D) return fail("input_dim out of range");
  if (!(p->input_sigma >= 0.0) || p->input_sigma > 1.0) return fail("input_sigma out of range");
  for (int i = 0; i < p->n_tiers; i++) {
    const dctfhe_tier& t = p->tiers[i];
    if (t.n < 1 || t.n > p->n_max) return fail("tier %d: n out of range", i);
    if (t.k < 1 || t.k > 2 || t.logN < 8 || t.logN > 13) return fail("tier %d: k or logN out of range", i);
    if ((t.k << t.logN) > p->D) return fail("tier %d: k*N exceeds D", i);
    if (t.l * t.beta > 63 || t.l < 1 || t.l > 4 || t.beta < 1 || (t.l >= 2 && t.beta > 16) || (t.l == 1 && t.beta > 28))
      return fail("tier %d: bad bootstrap gadget (l <= 4; beta <= 16 when l >= 2, <= 28 when l == 1: 32-bit accumulators)", i);
    // four levels: one kernel shape (tier T5r); its deferred digits of levels 1..3 share one 32-bit word in 10-bit fields
    // (pbs_core.h pack_digits)
    if (t.l == 4 && !(t.k == 1 && t.logN == 11 && t.beta <= 10))
      return fail("tier %d: bad bootstrap gadget (four levels only with k = 1, N = 2048, beta <= 10)", i);
    if (t.unroll != 1 && t.unroll != 2) return fail("tier %d: unroll must be 1 or 2", i);
    if (t.unroll == 2) {
      const bool paired = t.k == 1 && t.l == 1 && t.logN >= 11;                                        // pair-interleaved kernels
      const bool general = (t.k == 1 && t.l == 3 && t.logN == 11) || (t.k == 2 && t.l == 1 && t.logN == 10);   // general form
      if (!(paired || general) || (t.n & 1))
        return fail("tier %d: unroll 2 needs n even and (k, l, N) = (1, 1, >= 2048), (1, 3, 2048) or (2, 1, 1024)", i);
    }
    if (t.k < 1 || t.k > 2 || t.logN < 8 || t.logN > 13) return fail("tier %d: k or logN out of range", i);
    if (t.lk < 1 || t.lk > 63 || t.betak < 1 || t.betak > 8 || t.lk * t.betak > 63) return fail("tier %d: bad key-switch gadget (1 <= betak <= 8, lk >= 1, lk * betak <= 63)", i);
    if (!(t.lwe_sigma >= 0.0) || t.lwe_sigma > 1.0 || !(t.glwe_sigma >= 0.0) || t.glwe_sigma > 1.0) return fail("tier %d: noise parameter out of range", i);
    if (t.reserved != 0) return fail("tier %d: reserved must be 0", i);
    if (!tier_ppt(t)) return fail("tier %d: no kernel for logN=%d k=%d l=%d", i, t.logN, t.k, t.l);
    if (t.ksk_share >= i) return fail("tier %d: ksk_share must name an earlier tier", i);
    if (t.ksk_share >= 0) {
      const dctfhe_tier& o = p->tiers[t.ksk_share];
      if (o.n != t.n || o.lk != t.lk || o.betak != t.betak) return fail("tier %d: shared key-switch key has another shape", i);
    }
  }
  return 0;
}

// host-only validators: usable (and tested) without a GPU
extern "C" int dctfhe_params_check(const dctfhe_params* params) {
  if (!params) return fail("null parameters");
  return check_params(params);
}

// ---- client key -----------------------------------------------------------------------------------
static rng_key key_from_bytes(const uint8_t* b) {
  rng_key k;
  for (int i = 0; i < 8; i++) k.k[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
  return k;
}

// (seed, nonce) -> the generator keys of dctfhe_encrypt: a key-derivation key that only the seed determines (one ChaCha20 block of the
// secret generator key at a stream of its own), one block of THAT at (stream, counter) = the nonce for the noise key, and the mask key one
// block of the noise key -- the same secret -> public step as for the key material.
static void derive_encrypt_keys(dctfhe_client_key* C) {
  uint32_t o[16];
  rng_key kdf;
  chacha20_block(C->sec, STREAM_ENCKDF, 0, o);
  for (int i = 0; i < 8; i++) kdf.k[i] = o[i];
  uint64_t n0 = 0, n1 = 0;
  for (int i = 0; i < 8; i++) { n0 |= (uint64_t)C->nonce[i] << (8 * i); n1 |= (uint64_t)C->nonce[8 + i] << (8 * i); }
  chacha20_block(kdf, n0, n1, o);
  for (int i = 0; i < 8; i++) C->enc_sec.k[i] = o[i];
  chacha20_block(C->enc_sec, STREAM_PUBKEY, 0, o);
  for (int i = 0; i < 8; i++) C->enc_pub.k[i] = o[i];
}

extern "C" int dctfhe_client_key_create(dctfhe_ctx* ctx, const dctfhe_params* params, const uint8_t* seed32, dctfhe_client_key** out) {
  if (!ctx || !params || !seed32 || !out) return fail("dctfhe_client_key_create: null argument");
  CHK(check_params(params));
  HIPCHK(hipSetDevice(ctx->device));
  std::unique_ptr<dctfhe_client_key> C(new dctfhe_client_key);
  C->ctx = ctx; C->p = *params;
  memcpy(C->seed, seed32, 32);
  C->sec = key_from_bytes(seed32);
  {  // the public (mask) key is one ChaCha20 block of the secret one: knowing it says nothing about the secret key
    uint32_t o[16];
    chacha20_block(C->sec, STREAM_PUBKEY, 0, o);
    for (int i = 0; i < 8; i++) C->pub.k[i] = o[i];
  }
  {  // per-handle encryption nonce from the OS
    size_t got = 0;
    while (got < sizeof C->nonce) {
      const ssize_t r = getrandom(C->nonce + got, sizeof C->nonce - got, 0);
      if (r <= 0) return fail("dctfhe_client_key_create: the OS gave no random bytes for the encryption nonce (getrandom)");
      got += (size_t)r;
    }
    derive_encrypt_keys(C.get());
  }
  hipStream_t st = ctx->stream;
  const int D = params->D;
  HIPCHK(C->d_S.alloc(D));
  HIPCHK(C->d_s.alloc(params->n_max));
  hipLaunchKernelGGL(k_gen_bits, dim3((D + 255) / 256), dim3(256), 0, st, C->sec, (uint64_t)STREAM_BIGKEY, C->d_S.as<uint8_t>(), D);
  hipLaunchKernelGGL(k_gen_bits, dim3((params->n_max + 255) / 256), dim3(256), 0, st, C->sec, (uint64_t)STREAM_SMALLKEY, C->d_s.as<uint8_t>(), params->n_max);
  HIPCHK(hipGetLastError());
  for (int ti = 0; ti < params->n_tiers; ti++) {
    const dctfhe_tier& t = params->tiers[ti];
    if (t.unroll != 2) continue;
    HIPCHK(C->d_spair[ti].alloc((size_t)(3 * t.n / 2)));
    hipLaunchKernelGGL(k_pair_secret, dim3((t.n / 2 + 255) / 256), dim3(256), 0, st, C->s(), t.n, C->d_spair[ti].as<uint8_t>());
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));
  *out = C.release();
  return 0;
}
extern "C" int dctfhe_client_key_destroy(dctfhe_client_key* C) { delete C; return 0; }

// standard-domain bootstrap key blocks [i0, i0+ni) of tier `tier` (regenerated from the client's streams whenever needed)
static int gen_bsk_std_chunk(dctfhe_client_key* C, int tier, int i0, int ni, uint64_t* d_out) {
  const dctfhe_tier& t = C->p.tiers[tier];
  const int N = 1 << t.logN, rows = (t.k + 1) * t.l;
  SET_LDS_ATTR(k_bsk_gen_std, 8192 * 8);
  // unroll 2: the "secret" is the pair secret of 3n/2 bits, i0/ni count its blocks
  const uint8_t* bits = t.unroll == 2 ? C->d_spair[tier].as<uint8_t>() : C->s();
  hipLaunchKernelGGL(k_bsk_gen_std, dim3((unsigned)(ni * rows)), dim3(256), (size_t)N * 8, C->ctx->stream, bits, C->S(), i0, t.k, N,
                     t.l, t.beta, t.glwe_sigma, C->pub, C->sec, (uint64_t)(STREAM_BSK_MASK + 2 * tier), d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

// Precision of a key-switch key: the torus grid its words live on, 2^-(8 limbs) (client_shared.h ks_limbs: the host client rounds its
// key-switch bodies to the same grid)
static int ks_limbs(const dctfhe_tier& t) { return dctfhe::ks_limbs(t.lk, t.betak); }

// ---- evaluation keys ------------------------------------------------------------------------------
static size_t tier_bsk_blocks(const dctfhe_tier& t) { return (size_t)(t.unroll == 2 ? 3 * t.n / 2 : t.n); }
static size_t tier_bsk_elems(const dctfhe_tier& t) {   // complex values of the Fourier key, without the warm-up padding
  return tier_bsk_blocks(t) * (size_t)(t.k + 1) * t.l * (t.k + 1) * ((size_t)1 << (t.logN - 1));
}
static size_t tier_ksk_words(const dctfhe_params& p, const dctfhe_tier& t) { return (size_t)p.D * t.lk * (t.n + 1); }
// standard domain: a block is (k+1) l rows of k mask polynomials and a body polynomial; the compressed forms keep the bodies only
static size_t tier_bsk_body_words(const dctfhe_tier& t) { return tier_bsk_blocks(t) * (size_t)(t.k + 1) * t.l << t.logN; }
// blocks per pass through a 64 MB staging buffer that holds `polys` polynomials per row
static int tier_bsk_chunk(const dctfhe_tier& t, int polys) {
  const size_t block_bytes = ((size_t)(t.k + 1) * t.l * polys << t.logN) * 8;
  return std::max(1, (int)std::min(tier_bsk_blocks(t), ((size_t)64 << 20) / block_bytes));
}

// ---- tier selections (include/dctfhe.h "TIER SELECTIONS"): host only ---------------------------------------
// the tier whose key-switch key `tier` switches with: the end of its share chain
static int ksk_owner(const dctfhe_params& p, int tier) {
  while (p.tiers[tier].ksk_share >= 0) tier = p.tiers[tier].ksk_share;
  return tier;
}
static dctfhe_key_tiers key_tiers_full(const dctfhe_params& p) {
  dctfhe_key_tiers s{0, 0};
  for (int ti = 0; ti < p.n_tiers; ti++) {
    s.bsk |= 1u << ti;
    if (p.tiers[ti].ksk_share < 0) s.ksk |= 1u << ti;
  }
  return s;
}
static bool key_tiers_is_full(const dctfhe_params& p, const dctfhe_key_tiers& s) {
  const dctfhe_key_tiers f = key_tiers_full(p);
  return s.bsk == f.bsk && s.ksk == f.ksk;
}
static bool has_bsk(const dctfhe_key_tiers& s, int tier) { return (s.bsk >> tier) & 1u; }
static bool has_ksk(const dctfhe_key_tiers& s, int tier) { return (s.ksk >> tier) & 1u; }
// what a selection must satisfy before anything is sized by it; `closed`: also that no owner is missing (what a blob must carry)
static int key_tiers_check(const char* who, const dctfhe_params& p, const dctfhe_key_tiers& s, bool closed) {
  const uint32_t beyond = p.n_tiers >= 32 ? 0u : ~0u << p.n_tiers;
  if ((s.bsk | s.ksk) & beyond) return fail("%s: the tier selection names a tier at or beyond n_tiers = %d (bsk 0x%x, ksk 0x%x)", who, p.n_tiers, s.bsk, s.ksk);
  for (int ti = 0; ti < p.n_tiers; ti++) {
    if (has_ksk(s, ti) && p.tiers[ti].ksk_share >= 0)
      return fail("%s: the tier selection asks for a key-switch key of tier %d, which has none of its own (it shares tier %d's)", who, ti, p.tiers[ti].ksk_share);
    if (closed && has_bsk(s, ti) && !has_ksk(s, ksk_owner(p, ti)))
      return fail("%s: the tier selection is not closed: tier %d bootstraps, the key-switch key of tier %d is not selected", who, ti, ksk_owner(p, ti));
  }
  return 0;
}
extern "C" int dctfhe_key_tiers_all(const dctfhe_params* params, dctfhe_key_tiers* out) {
  if (!params || !out) return fail("dctfhe_key_tiers_all: null argument");
  CHK(check_params(params));
  *out = key_tiers_full(*params);
  return 0;
}
extern "C" int dctfhe_key_tiers_close(const dctfhe_params* params, dctfhe_key_tiers* io) {
  if (!params || !io) return fail("dctfhe_key_tiers_close: null argument");
  CHK(check_params(params));
  CHK(key_tiers_check("dctfhe_key_tiers_close", *params, *io, false));
  for (int ti = 0; ti < params->n_tiers; ti++)
    if (has_bsk(*io, ti)) io->ksk |= 1u << ksk_owner(*params, ti);
  return 0;
}
// The closed selection a circuit needs, and for the refusals an op that needs each key (-1: none does).  One enumeration, that of
// circuit_stats: a tier is selected exactly when its count there is positive.
struct CircuitKeyUse { dctfhe_key_tiers sel{0, 0}; int bsk_op[DCTFHE_MAX_TIERS], ksk_op[DCTFHE_MAX_TIERS]; };
static void circuit_key_use(const CircuitPlan& c, const dctfhe_params& P, CircuitKeyUse* u) {
  for (int i = 0; i < DCTFHE_MAX_TIERS; i++) u->bsk_op[i] = u->ksk_op[i] = -1;
  u->sel = dctfhe_key_tiers{0, 0};
  for (size_t i = 0; i < c.ops.size(); i++) {
    const SiteOp& o = c.ops[i];
    if (o.type == OP_MAXPOOL) {
      const TensorShape& a = c.tensors[o.src0];
      if (pool_pairs(a.C, a.H, a.W, o.pool.k, o.pool.stride, o.pool.pad) <= 0) continue;
    }
    for_each_bootstrap(o, P, [&](int tier, int, bool own_ks) {
      if (tier < 0 || tier >= P.n_tiers) return;
      if (!has_bsk(u->sel, tier)) { u->sel.bsk |= 1u << tier; u->bsk_op[tier] = (int)i; }
      const int owner = ksk_owner(P, tier);
      if (own_ks && !has_ksk(u->sel, owner)) { u->sel.ksk |= 1u << owner; u->ksk_op[owner] = (int)i; }
    });
  }
  // closing: a bootstrap that reuses another's small ciphertext still belongs to a tier that a closed selection gives a key-switch key
  for (int ti = 0; ti < P.n_tiers; ti++)
    if (has_bsk(u->sel, ti) && !has_ksk(u->sel, ksk_owner(P, ti))) { u->sel.ksk |= 1u << ksk_owner(P, ti); u->ksk_op[ksk_owner(P, ti)] = u->bsk_op[ti]; }
}
static int circuit_check_tiers(const CircuitPlan& circ, const dctfhe_params& P);
extern "C" int dctfhe_key_tiers_for_circuit(const void* blob, size_t size, const dctfhe_params* params, dctfhe_key_tiers* out) {
  if (!blob || !params || !out) return fail("dctfhe_key_tiers_for_circuit: null argument");
  CHK(check_params(params));
  CircuitPlan c;
  CHK(parse_circuit(blob, size, &c));
  CHK(circuit_check_tiers(c, *params));
  CircuitKeyUse u;
  circuit_key_use(c, *params, &u);
  *out = u.sel;
  return 0;
}
// bytes of the two blob forms under a selection: the header (and the public generator key), the two masks unless everything is selected,
// then the kept sections.  The caller has checked the selection.
static size_t eval_blob_size(const dctfhe_params& p, const dctfhe_key_tiers& s);
static size_t eval_cblob_size(const dctfhe_params& p, const dctfhe_key_tiers& s);
extern "C" int dctfhe_key_tiers_blob_bytes(const dctfhe_params* params, const dctfhe_key_tiers* tiers, int compressed, size_t* out) {
  if (!params || !tiers || !out) return fail("dctfhe_key_tiers_blob_bytes: null argument");
  CHK(check_params(params));
  CHK(key_tiers_check("dctfhe_key_tiers_blob_bytes", *params, *tiers, true));
  *out = compressed ? eval_cblob_size(*params, *tiers) : eval_blob_size(*params, *tiers);
  return 0;
}
// The one refusal of a call that needs a key the handle does not hold (like bound_to: before any allocation, copy or launch).
// need_bsk: the bootstrap key of `tier`; need_ksk: the key-switch key `tier` switches with.
static int keys_hold(const char* who, const dctfhe_eval_keys* K, int tier, bool need_bsk, bool need_ksk) {
  if (need_bsk && !has_bsk(K->sel, tier)) return fail("%s: the evaluation keys hold no bootstrap key of tier %d (tier selection bsk 0x%x, ksk 0x%x)", who, tier, K->sel.bsk, K->sel.ksk);
  if (need_ksk && !has_ksk(K->sel, ksk_owner(K->p, tier))) {
    const int owner = ksk_owner(K->p, tier);
    if (owner == tier) return fail("%s: the evaluation keys hold no key-switch key of tier %d (tier selection bsk 0x%x, ksk 0x%x)", who, tier, K->sel.bsk, K->sel.ksk);
    return fail("%s: the evaluation keys hold no key-switch key of tier %d, which tier %d switches with (tier selection bsk 0x%x, ksk 0x%x)", who, owner, tier, K->sel.bsk, K->sel.ksk);
  }
  return 0;
}

// allocate every array of the selected evaluation keys and fill what depends on the parameters only (twiddles, root tables)
static int eval_alloc(dctfhe_ctx* ctx, const dctfhe_params* params, const dctfhe_key_tiers& sel, std::unique_ptr<dctfhe_eval_keys>& E) {
  CHK(check_params(params));
  CHK(key_tiers_check("evaluation keys", *params, sel, true));
  HIPCHK(hipSetDevice(ctx->device));
  E.reset(new dctfhe_eval_keys);
  E->ctx = ctx; E->p = *params; E->sel = sel;
  hipStream_t st = ctx->stream;
  const int D = params->D;
  HIPCHK(E->d_dummy.alloc((size_t)(D + 1) * 8));
  for (int ti = 0; ti < params->n_tiers; ti++) {
    const dctfhe_tier& t = params->tiers[ti];
    TierKeys& tk = E->tiers[ti];
    tk.t = t;
    if (t.ksk_share >= 0) {
      tk.ks = E->tiers[t.ksk_share].ks;
    } else if (!has_ksk(sel, ti)) {
      tk.ks = &E->ksk[ti];      // stays empty: keys_hold refuses every call that would read it
    } else {
      KskKey& ks = E->ksk[ti];
      tk.ks = &ks;
      ks.limbs = ks_limbs(t);
      const size_t rows = (size_t)D * t.lk;
      HIPCHK(ks.ksk.alloc(rows * (t.n + 1) * 8));
      HIPCHK(ks.colsum.alloc((size_t)(t.n + 1) * 8));
      // the i8 MFMA key switch reads digits as SIGNED bytes: offset digits in [0, 2^betak) need betak <= 7;
      // wider gadgets and shapes the tiling does not cover go to the integer-VALU GEMM
      if (rows % 64 == 0 && rows <= (1u << 17) && t.betak <= 7) {
        ks.ncol_pad = ((ks.limbs * (t.n + 1) + 127) / 128) * 128;
        HIPCHK(ks.kskT.alloc((size_t)ks.ncol_pad * rows));
      }
    }
    if (!has_bsk(sel, ti)) continue;      // no twiddles, no root table, no key
    std::vector<cplx> tw;
    CHK(make_twiddles(t, tw));
    HIPCHK(tk.tw.alloc(tw.size() * sizeof(cplx)));
    HIPCHK(hipMemcpyAsync(tk.tw.p, tw.data(), tw.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    const int N = 1 << t.logN, M = N / 2;
    if (t.unroll == 2) {
      std::vector<cplx> wt((size_t)2 * N + 8);
      const long double PI = 3.141592653589793238462643383279502884L;
      for (int m = 0; m < 2 * N; m++) { const long double a = PI * m / N; wt[m] = cmk((double)cosl(a), (double)sinl(a)); }
      for (int m = 0; m < 8; m++) wt[(size_t)2 * N + m] = root64(8 * m);
      // the root table is gathered from at random by every thread of the two-bit kernels, every iteration: give it an allocation that
      // maps with one large page (a 262 KB allocation lands wherever the sub-allocator has room, and the N = 8192 bootstrap measured
      // 0 / +4 / +5 / +11 % at table addresses that were 256 / 64 / 128 / 32 KB-aligned: profiles/r02_exp_ablations.log)
      const size_t wt_bytes = (((wt.size() * sizeof(cplx)) + (2u << 20) - 1) >> 21) << 21;
      HIPCHK(tk.wtab.alloc(wt_bytes));
      HIPCHK(hipMemcpyAsync(tk.wtab.p, wt.data(), wt.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    // PBS_PF_DIST iterations' worth of extra (zero) key blocks: the L2 warm-up of the last iterations reads past the key
    // (launch_pbs checks this contract: pbs_core.h, "L2 warm-up geometry")
    const size_t per_block = (size_t)(t.k + 1) * t.l * (t.k + 1) * M;
    const size_t pad = (size_t)PBS_PF_DIST * (t.unroll == 2 ? 3 : 1) * per_block;
    HIPCHK(tk.bsk.alloc((tier_bsk_elems(t) + pad) * sizeof(cplx)));
    HIPCHK(hipMemsetAsync(tk.bsk.as<cplx>() + tier_bsk_elems(t), 0, pad * sizeof(cplx), st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// what is derived from the key-switch keys once they are in place: column sums and the signed byte limbs
static int eval_finish(dctfhe_eval_keys* E) {
  hipStream_t st = E->ctx->stream;
  for (int ti = 0; ti < E->p.n_tiers; ti++) {
    const dctfhe_tier& t = E->p.tiers[ti];
    if (t.ksk_share >= 0 || !has_ksk(E->sel, ti)) continue;
    KskKey& ks = E->ksk[ti];
    const size_t rows = (size_t)E->p.D * t.lk;
    hipLaunchKernelGGL(k_ksk_colsum, dim3((t.n + 256) / 256), dim3(256), 0, st, ks.ksk.as<uint64_t>(), (int)rows, t.n, ks.colsum.as<uint64_t>());
    if (ks.kskT.p) {
      // the limb form keeps the top tk.limbs bytes of every word: make sure nothing sits below them (an imported key must be on the grid)
      DevBuf flag;
      HIPCHK(flag.alloc(sizeof(int)));
      HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(int), st));
      hipLaunchKernelGGL(k_ksk_off_grid, dim3(2048), dim3(256), 0, st, ks.ksk.as<uint64_t>(), rows * (size_t)(t.n + 1), ks.limbs, flag.as<int>());
      int bad = 0;
      HIPCHK(hipMemcpyAsync(&bad, flag.p, sizeof bad, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (bad) return fail("tier %d: key-switch key words off the 2^-%d torus grid (a key made by another build?)", ti, 8 * ks.limbs);
      hipLaunchKernelGGL(k_ksk_to_limbs, dim3(4096), dim3(256), 0, st, ks.ksk.as<uint64_t>(), (int)rows, t.n, ks.limbs, ks.ncol_pad, ks.kskT.as<int8_t>());
    }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// a selection given by the caller: in range, no key-switch bit on a sharing tier, then closed
static int closed_selection(const char* who, const dctfhe_params& p, const dctfhe_key_tiers* tiers, dctfhe_key_tiers* sel) {
  if (!tiers) { *sel = key_tiers_full(p); return 0; }
  *sel = *tiers;
  CHK(key_tiers_check(who, p, *sel, false));
  for (int ti = 0; ti < p.n_tiers; ti++)
    if (has_bsk(*sel, ti)) sel->ksk |= 1u << ksk_owner(p, ti);
  return 0;
}
extern "C" int dctfhe_eval_keys_generate_tiers(dctfhe_client_key* C, const dctfhe_key_tiers* tiers, dctfhe_eval_keys** out) {
  if (!C || !out) return fail("dctfhe_eval_keys_generate: null argument");
  dctfhe_key_tiers sel;
  CHK(closed_selection("dctfhe_eval_keys_generate_tiers", C->p, tiers, &sel));
  std::unique_ptr<dctfhe_eval_keys> E;
  CHK(eval_alloc(C->ctx, &C->p, sel, E));
  hipStream_t st = C->ctx->stream;
  const int D = C->p.D;
  for (int ti = 0; ti < C->p.n_tiers; ti++) {
    const dctfhe_tier& t = C->p.tiers[ti];
    TierKeys& tk = E->tiers[ti];
    if (t.ksk_share < 0 && has_ksk(sel, ti)) {
      hipLaunchKernelGGL(k_ksk_gen, dim3((unsigned)((size_t)D * t.lk)), dim3(256), 0, st, C->S(), C->s(), t.n, t.lk, t.betak, ks_limbs(t), t.lwe_sigma, C->pub, C->sec,
                         (uint64_t)(STREAM_KSK + 2 * ti), tk.ks->ksk.as<uint64_t>());
      HIPCHK(hipGetLastError());
    }
    if (!has_bsk(sel, ti)) continue;
    const int N = 1 << t.logN, M = N / 2;
    const size_t per_bit_polys = (size_t)(t.k + 1) * t.l * (t.k + 1);
    const int blocks = (int)tier_bsk_blocks(t), chunk = tier_bsk_chunk(t, t.k + 1);
    DevBuf d_std;
    HIPCHK(d_std.alloc((size_t)chunk * per_bit_polys * N * 8));
    for (int i0 = 0; i0 < blocks; i0 += chunk) {
      const int ni = std::min(chunk, blocks - i0);
      CHK(gen_bsk_std_chunk(C, ti, i0, ni, d_std.as<uint64_t>()));
      CHK(launch_bsk_fourier(t, d_std.as<uint64_t>(), (size_t)ni * per_bit_polys, tk.tw.as<cplx>(), tk.bsk.as<cplx>() + (size_t)i0 * per_bit_polys * M, st));
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  CHK(eval_finish(E.get()));
  *out = E.release();
  return 0;
}
extern "C" int dctfhe_eval_keys_generate(dctfhe_client_key* C, dctfhe_eval_keys** out) { return dctfhe_eval_keys_generate_tiers(C, nullptr, out); }
extern "C" int dctfhe_eval_keys_tiers(dctfhe_eval_keys* E, dctfhe_key_tiers* out) {
  if (!E || !out) return fail("dctfhe_eval_keys_tiers: null argument");
  *out = E->sel;
  return 0;
}

extern "C" int dctfhe_keygen(dctfhe_ctx* ctx, const dctfhe_params* params, const uint8_t* seed32, dctfhe_client_key** client, dctfhe_eval_keys** eval) {
  if (!client || !eval) return fail("dctfhe_keygen: null output");
  dctfhe_client_key* C = nullptr;
  CHK(dctfhe_client_key_create(ctx, params, seed32, &C));
  dctfhe_eval_keys* E = nullptr;
  if (dctfhe_eval_keys_generate(C, &E)) { delete C; return -1; }
  *client = C; *eval = E;
  return 0;
}
extern "C" int dctfhe_eval_keys_destroy(dctfhe_eval_keys* E) { delete E; return 0; }

// ---- evaluation-key persistence: header + params, then per tier its own key-switch key (u64) and its Fourier bootstrap key
// version 2: the Fourier bootstrap keys carry 2^-64 / M (accumulator updates in units of the whole torus, fft_core.h); version 1 carried 1 / M
// version 3: the key-switch keys live on the 2^-(8 ks_limbs) torus grid (version-2 keys used all 64 bits and would lose their low bytes)
static constexpr uint32_t EVAL_BLOB_VERSION = 3;
struct EvalBlobHeader { uint32_t magic, version; uint64_t total_bytes; dctfhe_params params; };
// A PRUNED blob (a tier selection that is not everything) is the next version of its form: the two masks (u32 bsk, u32 ksk) follow the
// header -- in the compressed form the public generator key -- and then come the kept sections in tier order.  Everything selected writes
// the version above, byte for byte what it was.
static constexpr uint32_t EVAL_BLOB_VERSION_PRUNED = 4;
static size_t eval_blob_size(const dctfhe_params& p, const dctfhe_key_tiers& s) {
  size_t n = sizeof(EvalBlobHeader) + (key_tiers_is_full(p, s) ? 0 : sizeof(dctfhe_key_tiers));
  for (int ti = 0; ti < p.n_tiers; ti++) {
    const dctfhe_tier& t = p.tiers[ti];
    if (has_ksk(s, ti)) n += tier_ksk_words(p, t) * 8;
    if (has_bsk(s, ti)) n += tier_bsk_elems(t) * sizeof(cplx);
  }
  return n;
}
// the masks of a blob of either form whose header names `pruned_version`: read and checked before anything is sized by them
static int blob_selection(const char* what, const EvalBlobHeader& h, uint32_t pruned_version, const void* masks_at, size_t bytes_left, dctfhe_key_tiers* sel) {
  if (h.version != pruned_version) { *sel = key_tiers_full(h.params); return 0; }
  if (bytes_left < sizeof *sel) return fail("%s too short for its tier selection", what);
  memcpy(sel, masks_at, sizeof *sel);
  CHK(key_tiers_check(what, h.params, *sel, true));
  if (key_tiers_is_full(h.params, *sel)) return fail("%s: a blob that selects every tier is written in the unpruned version", what);
  return 0;
}
extern "C" int dctfhe_eval_keys_export(dctfhe_eval_keys* E, void* buf, size_t capacity, size_t* size) {
  if (!E || !size) return fail("dctfhe_eval_keys_export: null argument");
  const size_t need = eval_blob_size(E->p, E->sel);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_eval_keys_export: buffer of %zu bytes, %zu needed", capacity, need);
  HIPCHK(hipSetDevice(E->ctx->device));
  HIPCHK(hipStreamSynchronize(E->ctx->stream));
  const bool full = key_tiers_is_full(E->p, E->sel);
  EvalBlobHeader h{};
  h.magic = 0x4b564544u /* 'DEVK' */; h.version = full ? EVAL_BLOB_VERSION : EVAL_BLOB_VERSION_PRUNED; h.total_bytes = need; h.params = E->p;
  char* q = (char*)buf;
  memcpy(q, &h, sizeof h); q += sizeof h;
  if (!full) { memcpy(q, &E->sel, sizeof E->sel); q += sizeof E->sel; }
  for (int ti = 0; ti < E->p.n_tiers; ti++) {
    const dctfhe_tier& t = E->p.tiers[ti];
    if (has_ksk(E->sel, ti)) {
      HIPCHK(hipMemcpy(q, E->ksk[ti].ksk.p, tier_ksk_words(E->p, t) * 8, hipMemcpyDeviceToHost));
      q += tier_ksk_words(E->p, t) * 8;
    }
    if (!has_bsk(E->sel, ti)) continue;
    if (tier_duo(t)) {      // device order -> the blob's order
      std::vector<cplx> dev(tier_bsk_elems(t));
      HIPCHK(hipMemcpy(dev.data(), E->tiers[ti].bsk.p, dev.size() * sizeof(cplx), hipMemcpyDeviceToHost));
      duo_permute(dev.data(), (cplx*)q, dev.size() / DUO_M, false);
    } else {
      HIPCHK(hipMemcpy(q, E->tiers[ti].bsk.p, tier_bsk_elems(t) * sizeof(cplx), hipMemcpyDeviceToHost));
    }
    q += tier_bsk_elems(t) * sizeof(cplx);
  }
  return 0;
}
// ---- compressed evaluation keys: every mask word is a draw of the client's PUBLIC generator key `pub` (one ChaCha20 block of the secret
// key, like enc_pub for the inputs), so the blob carries `pub` and the bodies only, and the importer regenerates the masks on the GPU.
// Layout: EvalBlobHeader (magic 'DEVC', version 1), pub[32], then per tier: its own key-switch key's D*lk bodies (u64, on the
// 2^-(8 limbs) grid), its bootstrap key's standard-domain body polynomials [blocks][(k+1)l][N] (u64).  Bootstrap-key rows whose gadget
// term sits in a mask polynomial (p < k) are shipped in body form (k_bsk_gen_bodies): they decompress to the same phase, not the same
// words.  Key-switch keys and the rows with p = k decompress bit for bit.
static constexpr uint32_t EVAL_CBLOB_MAGIC = 0x43564544u /* 'DEVC' */, EVAL_CBLOB_VERSION = 1;
static constexpr uint32_t EVAL_CBLOB_VERSION_PRUNED = 2;      // the masks follow pub[32]
static size_t eval_cblob_size(const dctfhe_params& p, const dctfhe_key_tiers& s) {
  size_t n = sizeof(EvalBlobHeader) + 32 + (key_tiers_is_full(p, s) ? 0 : sizeof(dctfhe_key_tiers));
  for (int ti = 0; ti < p.n_tiers; ti++) {
    const dctfhe_tier& t = p.tiers[ti];
    if (has_ksk(s, ti)) n += (size_t)p.D * t.lk * 8;
    if (has_bsk(s, ti)) n += tier_bsk_body_words(t) * 8;
  }
  return n;
}
static void key_to_bytes(const rng_key& k, uint8_t* b) {
  for (int i = 0; i < 8; i++) for (int x = 0; x < 4; x++) b[4 * i + x] = (uint8_t)(k.k[i] >> (8 * x));
}
static uint64_t ksk_grid_mask(const dctfhe_tier& t) {
  const int drop = 64 - 8 * ks_limbs(t);
  return drop ? ~0ULL << drop : ~0ULL;
}
// rows [count][L] from device bodies (k_seeded_expand); checks the geometry the kernel relies on
static int launch_expand(const rng_key& key, uint64_t stream, uint64_t row0, uint64_t stride, int dim_eff, uint64_t and_mask, const uint64_t* d_bodies,
                         int nb, size_t count, size_t L, uint64_t* d_out, hipStream_t st) {
  if (stride < 8 || dim_eff < 1 || (uint64_t)dim_eff > stride || L < (size_t)nb || (size_t)dim_eff > L - nb)
    return fail("seeded expansion: rows %llu generator words apart, %d mask words, %d body words, stride %zu", (unsigned long long)stride, dim_eff, nb, L);
  if (count == 0) return 0;
  const size_t work = std::max(count * ((size_t)(dim_eff + 7) / 8 + 1), count * (L - dim_eff));
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, 16384));
  hipLaunchKernelGGL(k_seeded_expand, dim3(grid), dim3(256), 0, st, key, stream, row0, stride, dim_eff, and_mask, d_bodies, nb, count, L, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int dctfhe_eval_keys_export_compressed_tiers(dctfhe_client_key* C, const dctfhe_key_tiers* tiers, void* buf, size_t capacity, size_t* size) {
  if (!C || !size) return fail("dctfhe_eval_keys_export_compressed: null argument");
  const dctfhe_params& P = C->p;
  dctfhe_key_tiers sel;
  CHK(closed_selection("dctfhe_eval_keys_export_compressed_tiers", P, tiers, &sel));
  const size_t need = eval_cblob_size(P, sel);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_eval_keys_export_compressed: buffer of %zu bytes, %zu needed", capacity, need);
  HIPCHK(hipSetDevice(C->ctx->device));
  hipStream_t st = C->ctx->stream;
  const bool full = key_tiers_is_full(P, sel);
  EvalBlobHeader h{};
  h.magic = EVAL_CBLOB_MAGIC; h.version = full ? EVAL_CBLOB_VERSION : EVAL_CBLOB_VERSION_PRUNED; h.total_bytes = need; h.params = P;
  char* q = (char*)buf;
  memcpy(q, &h, sizeof h); q += sizeof h;
  key_to_bytes(C->pub, (uint8_t*)q); q += 32;
  if (!full) { memcpy(q, &sel, sizeof sel); q += sizeof sel; }
  for (int ti = 0; ti < P.n_tiers; ti++) {
    const dctfhe_tier& t = P.tiers[ti];
    if (has_ksk(sel, ti)) {     // the generated key itself (k_ksk_gen), of which only the body column leaves the device
      const size_t rows = (size_t)P.D * t.lk;
      DevBuf d_ksk;
      HIPCHK(d_ksk.alloc(rows * (t.n + 1) * 8));
      hipLaunchKernelGGL(k_ksk_gen, dim3((unsigned)rows), dim3(256), 0, st, C->S(), C->s(), t.n, t.lk, t.betak, ks_limbs(t), t.lwe_sigma, C->pub, C->sec,
                         (uint64_t)(STREAM_KSK + 2 * ti), d_ksk.as<uint64_t>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy2D(q, 8, d_ksk.as<uint64_t>() + t.n, (size_t)(t.n + 1) * 8, 8, rows, hipMemcpyDeviceToHost));
      q += rows * 8;
    }
    if (!has_bsk(sel, ti)) continue;
    const int N = 1 << t.logN, rows = (t.k + 1) * t.l;
    const int blocks = (int)tier_bsk_blocks(t), chunk = tier_bsk_chunk(t, 1);
    const uint8_t* bits = t.unroll == 2 ? C->d_spair[ti].as<uint8_t>() : C->s();
    DevBuf d_b;
    HIPCHK(d_b.alloc((size_t)chunk * rows * N * 8));
    SET_LDS_ATTR(k_bsk_gen_bodies, 8192 * 8);
    for (int i0 = 0; i0 < blocks; i0 += chunk) {
      const int ni = std::min(chunk, blocks - i0);
      hipLaunchKernelGGL(k_bsk_gen_bodies, dim3((unsigned)(ni * rows)), dim3(256), (size_t)N * 8, st, bits, C->S(), i0, t.k, N, t.l, t.beta, t.glwe_sigma,
                         C->pub, C->sec, (uint64_t)(STREAM_BSK_MASK + 2 * ti), d_b.as<uint64_t>());
      HIPCHK(hipGetLastError());
      const size_t bytes = (size_t)ni * rows * N * 8;
      HIPCHK(d_b.download(q, bytes, st));
      q += bytes;
    }
  }
  return 0;
}
extern "C" int dctfhe_eval_keys_export_compressed(dctfhe_client_key* C, void* buf, size_t capacity, size_t* size) {
  return dctfhe_eval_keys_export_compressed_tiers(C, nullptr, buf, capacity, size);
}

// a compressed blob's header, pub key and tier selection, checked against its size; *sections: where the first kept section begins
static int parse_cblob(const void* buf, size_t size, EvalBlobHeader* h, rng_key* pub, dctfhe_key_tiers* sel, const char** sections) {
  if (size < sizeof(EvalBlobHeader) + 32) return fail("compressed evaluation-key blob too short");
  memcpy(h, buf, sizeof *h);
  if (h->magic != EVAL_CBLOB_MAGIC || (h->version != EVAL_CBLOB_VERSION && h->version != EVAL_CBLOB_VERSION_PRUNED))
    return fail("bad compressed evaluation-key blob magic/version");
  CHK(check_params(&h->params));
  const size_t head = sizeof *h + 32;
  CHK(blob_selection("compressed evaluation-key blob", *h, EVAL_CBLOB_VERSION_PRUNED, (const char*)buf + head, size - head, sel));
  if (h->total_bytes != size || eval_cblob_size(h->params, *sel) != size)
    return fail(h->version == EVAL_CBLOB_VERSION_PRUNED ? "compressed evaluation-key blob is %zu bytes, its parameters and tier selection need %zu"
                                                        : "compressed evaluation-key blob is %zu bytes, its parameters need %zu", size, eval_cblob_size(h->params, *sel));
  *pub = key_from_bytes((const uint8_t*)buf + sizeof *h);
  *sections = (const char*)buf + head + (h->version == EVAL_CBLOB_VERSION_PRUNED ? sizeof *sel : 0);
  return 0;
}
// standard-domain bootstrap-key blocks [i0, i0 + ni) of tier ti from their host bodies: masks regenerated, bodies copied in
static int expand_bsk_chunk(const rng_key& pub, int ti, const dctfhe_tier& t, int i0, int ni, const uint64_t* h_bodies, uint64_t* d_bodies,
                            uint64_t* d_std, hipStream_t st) {
  const size_t N = (size_t)1 << t.logN, rows = (size_t)(t.k + 1) * t.l, nrow = (size_t)ni * rows;
  HIPCHK(hipMemcpyAsync(d_bodies, h_bodies, nrow * N * 8, hipMemcpyHostToDevice, st));
  CHK(launch_expand(pub, (uint64_t)(STREAM_BSK_MASK + 2 * ti), (uint64_t)i0 * rows, (uint64_t)t.k * N, t.k * (int)N, ~0ULL, d_bodies, (int)N, nrow,
                    (t.k + 1) * N, d_std, st));
  return 0;
}
static int import_compressed(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_eval_keys** out) {
  EvalBlobHeader h;
  rng_key pub;
  dctfhe_key_tiers sel;
  const char* q = nullptr;
  CHK(parse_cblob(buf, size, &h, &pub, &sel, &q));
  std::unique_ptr<dctfhe_eval_keys> E;
  CHK(eval_alloc(ctx, &h.params, sel, E));
  hipStream_t st = ctx->stream;
  for (int ti = 0; ti < h.params.n_tiers; ti++) {
    const dctfhe_tier& t = h.params.tiers[ti];
    TierKeys& tk = E->tiers[ti];
    if (has_ksk(sel, ti)) {
      const size_t rows = (size_t)h.params.D * t.lk;
      DevBuf d_b;
      HIPCHK(d_b.alloc(rows * 8));
      HIPCHK(hipMemcpyAsync(d_b.p, q, rows * 8, hipMemcpyHostToDevice, st));
      CHK(launch_expand(pub, (uint64_t)(STREAM_KSK + 2 * ti), 0, (uint64_t)t.n + 1, t.n, ksk_grid_mask(t), d_b.as<uint64_t>(), 1, rows, (size_t)t.n + 1,
                        tk.ks->ksk.as<uint64_t>(), st));
      HIPCHK(hipStreamSynchronize(st));
      q += rows * 8;
    }
    if (!has_bsk(sel, ti)) continue;
    const int N = 1 << t.logN, M = N / 2, rows = (t.k + 1) * t.l;
    const size_t per_bit_polys = (size_t)rows * (t.k + 1);
    const int blocks = (int)tier_bsk_blocks(t), chunk = tier_bsk_chunk(t, t.k + 1);
    DevBuf d_std, d_b;
    HIPCHK(d_std.alloc((size_t)chunk * per_bit_polys * N * 8));
    HIPCHK(d_b.alloc((size_t)chunk * rows * N * 8));
    for (int i0 = 0; i0 < blocks; i0 += chunk) {
      const int ni = std::min(chunk, blocks - i0);
      CHK(expand_bsk_chunk(pub, ti, t, i0, ni, (const uint64_t*)q, d_b.as<uint64_t>(), d_std.as<uint64_t>(), st));
      CHK(launch_bsk_fourier(t, d_std.as<uint64_t>(), (size_t)ni * per_bit_polys, tk.tw.as<cplx>(), tk.bsk.as<cplx>() + (size_t)i0 * per_bit_polys * M, st));
      HIPCHK(hipStreamSynchronize(st));      // the next chunk's copy reuses d_b and d_std
      q += (size_t)ni * rows * N * 8;
    }
  }
  CHK(eval_finish(E.get()));
  *out = E.release();
  return 0;
}
// test view: the standard-domain bootstrap key of one tier as dctfhe_eval_keys_import rebuilds it from a compressed blob
extern "C" int dctfhe_eval_keys_decompress_bsk(dctfhe_ctx* ctx, const void* buf, size_t size, int tier, uint64_t* out) {
  if (!ctx || !buf || !out) return fail("dctfhe_eval_keys_decompress_bsk: null argument");
  EvalBlobHeader h;
  rng_key pub;
  dctfhe_key_tiers sel;
  const char* q = nullptr;
  CHK(parse_cblob(buf, size, &h, &pub, &sel, &q));
  if (tier < 0 || tier >= h.params.n_tiers) return fail("tier out of range");
  if (!has_bsk(sel, tier)) return fail("dctfhe_eval_keys_decompress_bsk: the blob holds no bootstrap key of tier %d (tier selection bsk 0x%x, ksk 0x%x)", tier, sel.bsk, sel.ksk);
  for (int ti = 0; ti < tier; ti++) {
    const dctfhe_tier& t = h.params.tiers[ti];
    if (has_ksk(sel, ti)) q += (size_t)h.params.D * t.lk * 8;
    if (has_bsk(sel, ti)) q += tier_bsk_body_words(t) * 8;
  }
  const dctfhe_tier& t = h.params.tiers[tier];
  if (has_ksk(sel, tier)) q += (size_t)h.params.D * t.lk * 8;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t body_bytes = tier_bsk_body_words(t) * 8;
  DevBuf d_b, d_std;
  HIPCHK(d_b.alloc(body_bytes));
  HIPCHK(d_std.alloc(body_bytes * (t.k + 1)));
  CHK(expand_bsk_chunk(pub, tier, t, 0, (int)tier_bsk_blocks(t), (const uint64_t*)q, d_b.as<uint64_t>(), d_std.as<uint64_t>(), ctx->stream));
  HIPCHK(d_std.download(out, body_bytes * (t.k + 1), ctx->stream));
  return 0;
}

extern "C" int dctfhe_eval_keys_import(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_eval_keys** out) {
  if (!ctx || !buf || !out) return fail("dctfhe_eval_keys_import: null argument");
  if (size < sizeof(EvalBlobHeader)) return fail("evaluation-key blob too short");
  EvalBlobHeader h;
  memcpy(&h, buf, sizeof h);
  if (h.magic == EVAL_CBLOB_MAGIC) return import_compressed(ctx, buf, size, out);
  if (h.magic != 0x4b564544u || (h.version != EVAL_BLOB_VERSION && h.version != EVAL_BLOB_VERSION_PRUNED)) return fail("bad evaluation-key blob magic/version");
  CHK(check_params(&h.params));
  dctfhe_key_tiers sel;
  CHK(blob_selection("evaluation-key blob", h, EVAL_BLOB_VERSION_PRUNED, (const char*)buf + sizeof h, size - sizeof h, &sel));
  if (h.total_bytes != size || eval_blob_size(h.params, sel) != size)
    return fail(h.version == EVAL_BLOB_VERSION_PRUNED ? "evaluation-key blob is %zu bytes, its parameters and tier selection need %zu"
                                                      : "evaluation-key blob is %zu bytes, its parameters need %zu", size, eval_blob_size(h.params, sel));
  std::unique_ptr<dctfhe_eval_keys> E;
  CHK(eval_alloc(ctx, &h.params, sel, E));
  const char* q = (const char*)buf + sizeof h + (h.version == EVAL_BLOB_VERSION_PRUNED ? sizeof sel : 0);
  for (int ti = 0; ti < h.params.n_tiers; ti++) {
    const dctfhe_tier& t = h.params.tiers[ti];
    if (has_ksk(sel, ti)) {
      HIPCHK(hipMemcpy(E->ksk[ti].ksk.p, q, tier_ksk_words(h.params, t) * 8, hipMemcpyHostToDevice));
      q += tier_ksk_words(h.params, t) * 8;
    }
    if (!has_bsk(sel, ti)) continue;
    if (tier_duo(t)) {      // the blob's order -> device order
      std::vector<cplx> dev(tier_bsk_elems(t));
      duo_permute((const cplx*)q, dev.data(), dev.size() / DUO_M, true);
      HIPCHK(hipMemcpy(E->tiers[ti].bsk.p, dev.data(), dev.size() * sizeof(cplx), hipMemcpyHostToDevice));
    } else {
      HIPCHK(hipMemcpy(E->tiers[ti].bsk.p, q, tier_bsk_elems(t) * sizeof(cplx), hipMemcpyHostToDevice));
    }
    q += tier_bsk_elems(t) * sizeof(cplx);
  }
  CHK(eval_finish(E.get()));
  *out = E.release();
  return 0;
}

// ---- test / client views ---------------------------------------------------------------------------
extern "C" int dctfhe_client_key_export_secret(dctfhe_client_key* C, uint8_t* big_key, uint8_t* small_key) {
  HIPCHK(hipSetDevice(C->ctx->device));
  HIPCHK(hipMemcpy(big_key, C->S(), C->p.D, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(small_key, C->s(), C->p.n_max, hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int dctfhe_eval_keys_export_ksk(dctfhe_eval_keys* K, int tier, uint64_t* out) {
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_eval_keys_export_ksk", K, tier, false, true));
  const dctfhe_tier& t = K->p.tiers[tier];
  HIPCHK(hipSetDevice(K->ctx->device));
  HIPCHK(hipMemcpy(out, K->tiers[tier].ks->ksk.p, (size_t)K->p.D * t.lk * (t.n + 1) * 8, hipMemcpyDeviceToHost));
  return 0;
}
// the standard-domain bootstrap key, regenerated from the client's streams (what dctfhe_eval_keys_generate transformed)
extern "C" int dctfhe_client_key_export_bsk(dctfhe_client_key* C, int tier, uint64_t* out) {
  if (tier < 0 || tier >= C->p.n_tiers) return fail("tier out of range");
  const dctfhe_tier& t = C->p.tiers[tier];
  HIPCHK(hipSetDevice(C->ctx->device));
  const size_t words = tier_bsk_body_words(t) * (t.k + 1);
  DevBuf d;
  HIPCHK(d.alloc(words * 8));
  CHK(gen_bsk_std_chunk(C, tier, 0, (int)tier_bsk_blocks(t), d.as<uint64_t>()));     // unroll 2: the key of the pair secret
  HIPCHK(d.download(out, words * 8, C->ctx->stream));
  return 0;
}

// CSPRNG views: `count` outputs of (key, stream, idx0..) -- on the host (no GPU needed: known-answer tests) and on the device
extern "C" int dctfhe_rng_host(const uint8_t* key32, uint64_t stream, uint64_t idx0, size_t count, uint64_t* out) {
  const rng_key k = key_from_bytes(key32);
  for (size_t i = 0; i < count; i++) out[i] = rnd64(k, stream, idx0 + i);
  return 0;
}
extern "C" int dctfhe_rng_device(dctfhe_ctx* ctx, const uint8_t* key32, uint64_t stream, uint64_t idx0, size_t count, uint64_t* out) {
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf d;
  HIPCHK(d.alloc(count * 8));
  hipLaunchKernelGGL(k_rng_fill, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, key_from_bytes(key32), stream, idx0, d.as<uint64_t>(), count);
  HIPCHK(hipGetLastError());
  HIPCHK(d.download(out, count * 8, ctx->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------ client ops
// rows of `dim` mask words + body, input_dim <= dim <= D
extern "C" int dctfhe_encrypt_rows(dctfhe_ctx* ctx, dctfhe_client_key* C, const uint64_t* phases, size_t count, int dim, uint64_t* cts) {
  if (!ctx || !C || (count && (!phases || !cts))) return fail("dctfhe_encrypt: null argument");
  CHK(bound_to("dctfhe_encrypt", ctx, C->ctx, "client key"));
  const int D = C->p.D, dim_eff = C->p.input_dim > 0 ? C->p.input_dim : D;
  if (dim < dim_eff || dim > D) return fail("dctfhe_encrypt: rows of %d mask words; these parameters mask %d and the key has %d", dim, dim_eff, D);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)dim + 1;
  DevBuf d_ph, d_ct;
  HIPCHK(d_ph.alloc(count * 8));
  HIPCHK(d_ct.alloc(count * L * 8));
  HIPCHK(hipMemcpyAsync(d_ph.p, phases, count * 8, hipMemcpyHostToDevice, ctx->stream));
  // fresh streams per call: a (mask, noise) pair is never drawn twice under one handle; handles differ by their nonce
  const uint64_t stream = (uint64_t)STREAM_ENC + ((++C->enc_calls) << 16);
  hipLaunchKernelGGL(k_lwe_encrypt, dim3((unsigned)count), dim3(256), 0, ctx->stream, C->S(), D, dim, dim_eff, d_ph.as<uint64_t>(),
                     C->p.input_sigma, C->enc_pub, C->enc_sec, stream, d_ct.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(cts, d_ct.p, count * L * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}
extern "C" int dctfhe_encrypt(dctfhe_ctx* ctx, dctfhe_client_key* C, const uint64_t* phases, size_t count, uint64_t* cts) {
  if (!C) return fail("dctfhe_encrypt: null argument");
  return dctfhe_encrypt_rows(ctx, C, phases, count, C->p.D, cts);
}
// a handle's position in its own encryption streams (the streams themselves differ from handle to handle by the nonce)
extern "C" int dctfhe_client_key_set_encrypt_counter(dctfhe_client_key* C, uint64_t next_call) {
  if (!C) return fail("null client key");
  if (next_call >= (1ULL << 47)) return fail("encrypt counter out of range");
  C->enc_calls = next_call;
  return 0;
}
// reproducible experiments and tests only: fix the nonce (and with it every mask and noise value dctfhe_encrypt will draw)
extern "C" int dctfhe_client_key_set_encrypt_nonce(dctfhe_client_key* C, const uint8_t* nonce16) {
  if (!C || !nonce16) return fail("dctfhe_client_key_set_encrypt_nonce: null argument");
  memcpy(C->nonce, nonce16, sizeof C->nonce);
  derive_encrypt_keys(C);
  return 0;
}
extern "C" int dctfhe_decrypt_rows(dctfhe_ctx* ctx, dctfhe_client_key* C, const uint64_t* cts, size_t count, int dim, uint64_t* phases) {
  if (!ctx || !C || (count && (!phases || !cts))) return fail("dctfhe_decrypt: null argument");
  CHK(bound_to("dctfhe_decrypt", ctx, C->ctx, "client key"));
  if (dim < 0 || dim > C->p.D) return fail("dctfhe_decrypt: rows of %d mask words, the key has %d", dim, C->p.D);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)dim + 1;
  DevBuf d_ph, d_ct;
  HIPCHK(d_ph.alloc(count * 8));
  HIPCHK(d_ct.alloc(count * L * 8));
  HIPCHK(hipMemcpyAsync(d_ct.p, cts, count * L * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_lwe_phase, dim3((unsigned)count), dim3(256), 0, ctx->stream, C->S(), dim, d_ct.as<uint64_t>(), d_ph.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(phases, d_ph.p, count * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}
extern "C" int dctfhe_decrypt(dctfhe_ctx* ctx, dctfhe_client_key* C, const uint64_t* cts, size_t count, uint64_t* phases) {
  if (!C) return fail("dctfhe_decrypt: null argument");
  return dctfhe_decrypt_rows(ctx, C, cts, count, C->p.D, phases);
}
// packed results (dctfhe_keyswitch_pack, dctfhe_session_download_packed): rows of n + 1 u16 under the first n bits of the small key
extern "C" int dctfhe_decrypt_packed(dctfhe_ctx* ctx, dctfhe_client_key* C, int n, const uint16_t* rows, size_t count, uint64_t* phases) {
  if (!ctx || !C || (count && (!rows || !phases))) return fail("dctfhe_decrypt_packed: null argument");
  CHK(bound_to("dctfhe_decrypt_packed", ctx, C->ctx, "client key"));
  if (n < 1 || n > C->p.n_max) return fail("dctfhe_decrypt_packed: rows of %d mask words, the small key has %d", n, C->p.n_max);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t bytes = count * (size_t)(n + 1) * sizeof(uint16_t);
  DevBuf d_ph, d_rows;
  HIPCHK(d_ph.alloc(count * 8));
  HIPCHK(d_rows.alloc(bytes));
  HIPCHK(hipMemcpyAsync(d_rows.p, rows, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_phase16, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ctx->stream, C->s(), n, d_rows.as<uint16_t>(), count, d_ph.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(phases, d_ph.p, count * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ---- seeded input ciphertexts: the mask of ciphertext c is the draw (enc_pub, stream, c (D + 1) + j), j < input_dim, and enc_pub is one
// ChaCha20 block of the handle's secret encryption key -- the client ships (enc_pub, stream, bodies), the server regenerates the masks
extern "C" int dctfhe_encrypt_seeded(dctfhe_ctx* ctx, dctfhe_client_key* C, const uint64_t* phases, size_t count, uint8_t* mask_key,
                                     uint64_t* stream_out, uint64_t* bodies) {
  if (!ctx || !C || !mask_key || !stream_out || (count && (!phases || !bodies))) return fail("dctfhe_encrypt_seeded: null argument");
  CHK(bound_to("dctfhe_encrypt_seeded", ctx, C->ctx, "client key"));
  const int D = C->p.D, dim_eff = C->p.input_dim > 0 ? C->p.input_dim : D;
  key_to_bytes(C->enc_pub, mask_key);
  if (count == 0) { *stream_out = 0; return 0; }    // nothing drawn: the counter stays, as in dctfhe_encrypt_rows
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf d_ph, d_b;
  HIPCHK(d_ph.alloc(count * 8));
  HIPCHK(d_b.alloc(count * 8));
  HIPCHK(hipMemcpyAsync(d_ph.p, phases, count * 8, hipMemcpyHostToDevice, ctx->stream));
  const uint64_t stream = (uint64_t)STREAM_ENC + ((++C->enc_calls) << 16);      // the step dctfhe_encrypt_rows takes
  hipLaunchKernelGGL(k_lwe_encrypt_seeded, dim3((unsigned)count), dim3(256), 0, ctx->stream, C->S(), D, dim_eff, d_ph.as<uint64_t>(), C->p.input_sigma,
                     C->enc_pub, C->enc_sec, stream, d_b.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(bodies, d_b.p, count * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *stream_out = stream;
  return 0;
}
extern "C" int dctfhe_expand_seeded(dctfhe_ctx* ctx, const uint8_t* mask_key, uint64_t stream, int D, int dim_eff, const uint64_t* bodies, size_t count,
                                    int dim, uint64_t* rows) {
  if (!ctx || !mask_key || (count && (!bodies || !rows))) return fail("dctfhe_expand_seeded: null argument");
  if (D < 8 || dim_eff < 1 || dim_eff > D || dim < dim_eff || dim > D)
    return fail("dctfhe_expand_seeded: D = %d, %d mask words per ciphertext, rows of %d (need 1 <= dim_eff <= dim <= D, D >= 8)", D, dim_eff, dim);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)dim + 1;
  DevBuf d_b, d_r;
  HIPCHK(d_b.alloc(count * 8));
  HIPCHK(d_r.alloc(count * L * 8));
  HIPCHK(hipMemcpyAsync(d_b.p, bodies, count * 8, hipMemcpyHostToDevice, ctx->stream));
  CHK(launch_expand(key_from_bytes(mask_key), stream, 0, (uint64_t)D + 1, dim_eff, ~0ULL, d_b.as<uint64_t>(), 1, count, L, d_r.as<uint64_t>(), ctx->stream));
  HIPCHK(hipMemcpyAsync(rows, d_r.p, count * L * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------ device-level building blocks
struct Timers {
  hipStream_t st;
  bool on;
  std::vector<DevEvent>* pool;       // owned by the session (or by nobody: primitives pass on = false)
  struct Span { hipEvent_t a, b; int cat; };
  std::vector<Span> spans;
  size_t used = 0;
  hipEvent_t take() {
    if (used == pool->size()) { pool->emplace_back(); pool->back().create(); }
    return (*pool)[used++].e;
  }
  int begin(int cat) {
    if (!on) return -1;
    Span s; s.cat = cat;
    s.a = take(); s.b = take();
    hipEventRecord(s.a, st);
    spans.push_back(s);
    return (int)spans.size() - 1;
  }
  void end(int h) { if (h >= 0) hipEventRecord(spans[h].b, st); }
};
enum { CAT_LINEAR = 100, CAT_KS = 101 };  // 0..7: bootstrap of tier i

// The ciphertexts a key switch reads: rows of L words (body at L-1), shifted left by `shift` with body_add on the body, on the fly.
// deff: mask words beyond it are known to be zero in every input (0 or >= D: no such knowledge).  The key switch then
// runs on the first deff rows of the key only -- the same result bit for bit, deff/D of the work.
// Ciphertext c is row c (KS_ROWS), row ia[c] - row ib[c] (KS_DIFF: the pairwise maxima of a max pool) or row c + row c of `rows_b`, rows
// of Lb words (KS_SUM: the second look-up of a parity-split site): kernels.h ks_src_*.
enum KsSource { KS_ROWS, KS_DIFF, KS_SUM };
struct KsInput {
  const uint64_t* rows = nullptr; size_t L = 0; int deff = 0, shift = 0; uint64_t body_add = 0;
  KsSource source = KS_ROWS;
  const int32_t *ia = nullptr, *ib = nullptr;
  const uint64_t* rows_b = nullptr; size_t Lb = 0;
};
// key switch of `count` ciphertexts into small ciphertexts of tier `tier` (sc.small; sc.digits and sc.bodies in between)
static int dev_keyswitch(dctfhe_keys* K, int tier, const KsInput& in, size_t count, const LutScratch& sc, Timers* tm) {
  const dctfhe_tier& t = K->p.tiers[tier];
  KskKey& ks = *K->tiers[tier].ks;
  const uint64_t* ksk = ks.ksk.as<uint64_t>();
  const int8_t* kskT = ks.kskT.as<int8_t>();
  const int D = K->p.D, deff = in.deff;
  const size_t L = in.L;                         // row stride of the input ciphertexts (body at L-1)
  const int Dmax = (int)std::min<size_t>(L - 1, (size_t)D);
  hipStream_t st = K->ctx->stream;
  int De = (deff > 0 && deff < Dmax && kskT && (deff * t.lk) % 64 == 0) ? deff : Dmax;
  if (!kskT && De != D) return fail("key switch: the integer-VALU path needs full-width rows");
  if (kskT && (De * t.lk) % 64 != 0) return fail("key switch: %d rows x %d levels is not a multiple of 64", De, t.lk);
  const uint64_t* colsum = ks.colsum.as<uint64_t>();
  if (De < D) {
    auto it = ks.colsum_eff.find(De);
    if (it == ks.colsum_eff.end()) {      // filled here, entered into the cache only once the fill is under way without an error
      DevBuf cs;
      HIPCHK(cs.alloc((size_t)(t.n + 1) * 8));
      hipLaunchKernelGGL(k_ksk_colsum, dim3((t.n + 256) / 256), dim3(256), 0, st, ksk, De * t.lk, t.n, cs.as<uint64_t>());
      HIPCHK(hipGetLastError());
      it = ks.colsum_eff.emplace(De, std::move(cs)).first;
    }
    colsum = it->second.as<uint64_t>();
  }
  const int h = tm ? tm->begin(CAT_KS) : -1;
  const size_t total = count * (size_t)De;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
#define KS_DECOMPOSE(SRC, ...) \
  hipLaunchKernelGGL(k_ks_decompose<SRC>, dim3(grid), dim3(256), 0, st, SRC{__VA_ARGS__}, count, De, in.shift, in.body_add, t.lk, t.betak, sc.digits(), sc.bodies())
  switch (in.source) {
    case KS_ROWS: KS_DECOMPOSE(ks_src_rows, in.rows, L); break;
    case KS_DIFF: KS_DECOMPOSE(ks_src_diff, in.rows, L, in.ia, in.ib); break;
    case KS_SUM:  KS_DECOMPOSE(ks_src_sum, in.rows, L, in.rows_b, in.Lb, in.Lb - 1); break;
  }
#undef KS_DECOMPOSE
  if (kskT) {   // matrix-core path: i8 digits x signed byte limbs of the key
    const unsigned ncb = (unsigned)(ks.ncol_pad / 128), nrb = (unsigned)((count + 127) / 128), cpx = (ncb + 7) / 8;
#define KS_LAUNCH(LB)                                                                                                                      \
    hipLaunchKernelGGL(k_ks_mfma<LB>, dim3(8 * cpx * nrb), dim3(256), 0, st, sc.digits(), sc.bodies(), count, De * t.lk, kskT, D * t.lk, ks.ncol_pad, \
                       colsum, t.n, t.betak, sc.small())
    if (ks.limbs == 2) KS_LAUNCH(2); else if (ks.limbs == 4) KS_LAUNCH(4); else KS_LAUNCH(8);
#undef KS_LAUNCH
  } else {           // shapes the MFMA tiling does not cover (D*lk not a multiple of 64, betak = 8): integer VALU GEMM
    constexpr int CT = 16;
    dim3 g2((t.n + 1 + 255) / 256, (unsigned)((count + CT - 1) / CT));
    hipLaunchKernelGGL(k_ks_gemm<CT>, g2, dim3(256), 0, st, sc.digits(), sc.bodies(), count, D * t.lk, ksk, colsum, t.n, t.betak, sc.small());
  }
  HIPCHK(hipGetLastError());
  if (tm) tm->end(h);
  return 0;
}

// centred mod switch on `count` small ciphertexts of tier `tier`, in place (kernels.h k_ms_center); part of the key-switch span of the timers
static int dev_ms_center(dctfhe_keys* K, int tier, uint64_t* d_small, size_t count, Timers* tm) {
  if (count == 0) return 0;
  const dctfhe_tier& t = K->p.tiers[tier];
  const int h = tm ? tm->begin(CAT_KS) : -1;
  hipLaunchKernelGGL(k_ms_center, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, K->ctx->stream, d_small, count, t.n, t.logN);
  HIPCHK(hipGetLastError());
  if (tm) tm->end(h);
  return 0;
}

// What a bootstrap looks up: tables of 2^w entries; ciphertext c takes table idx[c] (idx: optional), or, of `nchan` per-channel tables,
// the one of element e_offset + c of a tensor with hw elements per channel.  The defaults mean one table.
struct PbsLut { const int64_t* tables = nullptr; int w = 0; const int32_t* idx = nullptr; int hw = 1, nchan = 1; size_t e_offset = 0; };
// Where its result goes: rows of L words, stored or added to what the rows hold, body_add on the body.
// sink: L words for the padded groups of the last workgroup, which redo the last ciphertext in store mode (kernels.h pbs_kernel); nullptr: the
// keys' own D + 1 words, which rows of at most D + 1 words fit.
struct PbsOut { uint64_t* rows = nullptr; size_t L = 0; bool accumulate = false; uint64_t body_add = 0; uint64_t* sink = nullptr; };
static int dev_pbs(dctfhe_keys* K, int tier, const uint64_t* d_small, size_t count, const PbsLut& lut, const PbsOut& out, Timers* tm) {
  const dctfhe_tier& t = K->p.tiers[tier];
  pbs_launch a;
  a.cts_small = d_small; a.count = count; a.n = t.n; a.beta = t.beta;
  a.bsk = K->tiers[tier].bsk.as<cplx>(); a.tw = K->tiers[tier].tw.as<cplx>(); a.wtab = K->tiers[tier].wtab.as<cplx>();
  a.tables = lut.tables; a.w = lut.w; a.table_idx = lut.idx; a.hw = lut.hw; a.nchan = lut.nchan; a.e_offset = lut.e_offset;
  const int ring = t.k << t.logN;
  if (out.L < (size_t)ring + 1) return fail("bootstrap output rows of %zu words cannot hold a ring of %d", out.L, ring);
  if (out.L > (size_t)K->p.D + 1 && !out.sink) return fail("bootstrap output rows of %zu words exceed the sink of the padded groups (%d words)", out.L, K->p.D + 1);
  a.out = out.rows; a.D_out = (int)out.L - 1; a.accumulate = out.accumulate; a.body_add = out.body_add; a.dummy = out.sink ? out.sink : K->d_dummy.as<uint64_t>(); a.bsk_wrap = 0;
  // L2 warm-up: each workgroup touches 1/pf_parts of the next key blocks; the paired two-bit kernel at N = 2048 measures 3 % better
  // without (profiles/r02_exp_ablations.log: 22.5 vs 23.2 ms), every other barrier-coupled kernel better with (T4r 82.4 vs 86.3, T5a 25.7
  // vs 26.6).  The parts are dealt by blockIdx / 8, i.e. per XCD: with one 512-thread workgroup per CU an XCD holds 32 of them, and 32
  // parts -- every line touched once per XCD instead of twice -- is worth 4 % on the N = 8192 kernel (288 vs 300 ms per 12 288; 24, 40,
  // 48, 64 parts: 302, 318, 325, 330), nothing at N = 4096 (143.4 vs 144.0) and N = 2048 three levels (180.9 vs 181.1).
  a.pf_parts = (t.unroll == 2 && t.logN == 11 && t.l == 1) ? 0 : t.logN >= 13 ? 32 : 16;
  const int h = tm ? tm->begin(tier) : -1;
  CHK(launch_pbs(t, a, K->ctx->stream));
  if (tm) tm->end(h);
  return 0;
}
// margin audit: where a probe of the switched small ciphertexts goes -- the secret small key (device bytes) and the slot of the site's
// FIRST bootstrap with a key switch of its own; dev_round_lut / dev_max_pool pass the slot of the one they launch to dev_ks_pbs
struct MarginProbe {
  const uint8_t* key = nullptr; margin_slot* slot = nullptr;
  MarginProbe at(int entry) const { return MarginProbe{key, slot + entry}; }
};
static unsigned margin_grid(size_t count) { return (unsigned)std::max<size_t>(1, std::min<size_t>((count + 3) / 4, 1024)); }
// the probe kernel on `count` small ciphertexts of `tier` about to meet a table of w input bits; outside every Timers span
static int dev_margin_probe(hipStream_t st, const dctfhe_tier& t, const uint8_t* d_key, const uint64_t* d_small, size_t count, int w, int32_t* d_err,
                            margin_slot* d_slot) {
  if (count == 0) return 0;
  if (w < 0 || t.logN - w < 1) return fail("margin probe: a table of %d input bits leaves no box on a ring of 2^%d", w, t.logN);
  hipLaunchKernelGGL(k_margin_probe, dim3(margin_grid(count)), dim3(256), 0, st, d_key, d_small, count, t.n, t.logN, w, d_err, d_slot);
  HIPCHK(hipGetLastError());
  return 0;
}
// key switch of `in` to tier `tier`, centred mod switch, bootstrap: what every look-up with a key switch of its own runs on a chunk.
// probe (the margin audit; nullptr everywhere else): the switched small ciphertexts are measured on the way
static int dev_ks_pbs(dctfhe_keys* K, int tier, const KsInput& in, size_t count, const PbsLut& lut, const PbsOut& out, const LutScratch& sc, Timers* tm,
                      const MarginProbe* probe = nullptr) {
  CHK(dev_keyswitch(K, tier, in, count, sc, tm));
  CHK(dev_ms_center(K, tier, sc.small(), count, tm));
  if (probe) CHK(dev_margin_probe(K->ctx->stream, K->p.tiers[tier], probe->key, sc.small(), count, lut.w, nullptr, probe->slot));
  return dev_pbs(K, tier, sc.small(), count, lut, out, tm);
}

// Both kernels put one output pixel per block of gridDim.y and one block of output channels per block of gridDim.z: a launch beyond what
// the device reports for either is refused here, by its numbers, instead of surfacing as a launch error
static int conv_grid_ok(const dctfhe_ctx* cx, size_t pixels, size_t blocks) {
  if (pixels > (size_t)cx->max_grid_y)
    return fail("convolution: %zu output pixels (batch x Ho x Wo) exceed the device's launch-grid limit of %d: run it in smaller batches", pixels, cx->max_grid_y);
  if (blocks > (size_t)cx->max_grid_z)
    return fail("convolution: %zu blocks of output channels exceed the device's launch-grid limit of %d", blocks, cx->max_grid_z);
  return 0;
}
// The output window: channels [c0, c1) of the Cout the weights hold, into a buffer laid out [batch][c1 - c0][Ho][Wo] (kernels.h).  The whole
// output (window == nullptr) goes out in one launch and is refused past the grid limit, as it always was; a window is launched in chunks
// of at most max_grid_y pixels, with the first pixel of each passed to the kernel, and is never refused for its pixel count.
struct ConvWindow { int c0, c1; };
static int dev_conv2d(const dctfhe_ctx* cx, const uint64_t* in, int batch, int Cin, int H, int W, size_t Lin, size_t deff, const int8_t* d_w, const ConvPack* pk, int Cout,
                      int KH, int KW, int stride, int pad, uint64_t* out, size_t Lout, const ConvWindow* window = nullptr) {
  hipStream_t st = cx->stream;
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  const size_t pixels = (size_t)batch * Ho * Wo;
  const int c0 = window ? window->c0 : 0, c1 = window ? window->c1 : Cout;
  if (c0 < 0 || c0 >= c1 || c1 > Cout) return fail("convolution: output window of channels [%d, %d) of %d", c0, c1, Cout);
  const bool mfma = pk && pk->d_w && Lout >= 32;
  // clear mode (one word per element): u64 wrap MACs on the vector ALU.
  // 16 output channels per thread: 32 / 64 (fewer re-reads of the input) measured 1.45x / 3.5x SLOWER -- their per-tap weights no
  // longer fit the scalar registers (profiles/r02_exp_ablations.log)
  constexpr int COT = 16;
  const size_t blocks = (size_t)(c1 - c0 + (mfma ? 63 : COT - 1)) / (mfma ? 64 : COT);
  // a window's chunk: what the device's grid holds, and no more than the 65 535 every device takes (so that the chunked path is the same
  // code on a device that reports more)
  const size_t chunk = window ? std::min<size_t>((size_t)std::max(cx->max_grid_y, 1), 65535) : std::max<size_t>(pixels, 1);
  CHK(conv_grid_ok(cx, std::min(pixels, chunk), blocks));
  if (pixels > (size_t)INT32_MAX) return fail("convolution: %zu output pixels (batch x Ho x Wo) do not fit a 32-bit pixel number", pixels);
  for (size_t pix0 = 0; pix0 < pixels; pix0 += chunk) {
    const size_t np = std::min(pixels - pix0, chunk);
    if (mfma) {
      // ciphertext rows: the contraction over (ci, ky, kx) on the matrix cores, input words split into signed byte limbs on the fly
      dim3 grid((unsigned)((Lout + 31) / 32), (unsigned)np, (unsigned)blocks);
      hipLaunchKernelGGL(k_conv2d_mfma, grid, dim3(256), 0, st, in, H, W, Lin, deff, pk->d_w, pk->d_taps, pk->kpad, Cin * H * W, c0, c1, (int)pix0, stride, Ho, Wo, Lout, out);
    } else {
      dim3 grid((unsigned)((Lout + 255) / 256), (unsigned)np, (unsigned)blocks);
      hipLaunchKernelGGL(k_conv2d<COT>, grid, dim3(256), 0, st, in, Cin, H, W, Lin, deff, d_w, c0, c1, (int)pix0, KH, KW, stride, pad, Ho, Wo, Lout, out);
    }
    HIPCHK(hipGetLastError());
  }
  return 0;
}

static unsigned ew_grid(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 16384)); }

// The rows a look-up site works on.  With one-bit steps: in place on `work` (rows of Lw words, already shifted / offset; the first `deff`
// mask words may be non-zero).  Without: nothing modifies the input, so the key switch reads `src` (rows of Ls words) directly with the
// site's shift and body offset applied on the fly, and the table bootstrap writes `work` -- no copy of the tensor at all.  A split needs
// `par` too, rows of Lp words for the parity bootstrap's output and then the second look-up's (Lw - 1, Lp - 1 >= the rings of both), and
// the half tables tab_s / tab_d in place of `tables`.  idx: optional table index per ciphertext.
struct LutRows {
  const uint64_t* src = nullptr;
  uint64_t *work = nullptr, *par = nullptr;
  size_t Ls = 0, Lw = 0, Lp = 0;
  const int64_t *tables = nullptr, *tab_s = nullptr, *tab_d = nullptr;
  const int32_t* idx = nullptr;
};
static size_t ring_of(const dctfhe_params& P, int tier);
static size_t ring_of(const dctfhe_keys* K, int tier) { return ring_of(K->p, tier); }
// probe: the margin audit's slots of this site in for_each_bootstrap order -- steps, a split's second look-up, the table
// e0: the rows are a slice that starts at element e0 of the tensor (a sharded session): the per-channel tables go by e0 + c.  Everything
// else under a site is indexed by the launch: the scratch, and the parity rows `par`, which hold one chunk at a time
static int dev_round_lut(dctfhe_keys* K, const LutSite& L, const LutRows& b, size_t count, int hw, const LutScratch& sc, Timers* tm, int deff,
                         const MarginProbe* probe = nullptr, size_t e0 = 0) {
  const bool split = L.split();
  const int p = L.p, steps = L.n_steps(), nchan = L.ntab, tab_tier = L.tab_tier, tier2 = L.tier2(K->p);
  const size_t Lw = b.Lw, ring2 = split ? ring_of(K, tier2) : 0;
  if (split) {
    if (L.w < 2 || !b.par || !b.tab_s || !b.tab_d) return fail("parity split: needs a table of at least 2 input bits, a parity buffer and the half tables");
    if (Lw < ring2 + 1 || b.Lp < ring2 + 1) return fail("parity split: rows of %zu / %zu words cannot hold the second look-up's ring of %zu", Lw, b.Lp, ring2);
  }
  for (size_t c0 = 0; c0 < count; c0 += sc.chunk) {
    const size_t cn = std::min(sc.chunk, count - c0);
    uint64_t* w0 = b.work + c0 * Lw;
    KsInput work;            // the working rows as they stand
    work.rows = w0; work.L = Lw; work.deff = deff;
    PbsLut tab;              // the site's table look-up
    tab.tables = split ? b.tab_s : b.tables; tab.w = L.table_bits(); tab.idx = b.idx ? b.idx + c0 : nullptr; tab.hw = hw; tab.nchan = nchan; tab.e_offset = e0 + c0;
    for (int i = 0; i < steps; i++) {
      const int vlog = 62 - p + i;
      KsInput in = work; in.shift = p - i;
      PbsOut bit{w0, Lw}; bit.accumulate = true; bit.body_add = (uint64_t)0 - (1ULL << vlog);
      const MarginProbe pr = probe ? probe->at(i) : MarginProbe{};
      CHK(dev_ks_pbs(K, L.steps.at(i), in, cn, PbsLut{sc.bit_tables() + vlog}, bit, sc, tm, probe ? &pr : nullptr));
    }
    if (split) {
      // t = 2 t' + b0 sits under the padding bit once the r rounding steps are done.  The last step was one more of them, on b0: it left
      // t' as a (w-1)-bit message in w0.  The same small ciphertext, bootstrapped with 2^62 and body offset -2^62, gives b0 * 2^63 (par).
      // Second look-up first, while w0 still holds t': key switch of w0 + par (b0 in the padding bit, never materialised), table Dt
      // -> (-1)^b0 Dt[t'] into par; then the first look-up S[t'] into w0 as for any site, and the sum.
      PbsOut par{b.par, b.Lp}; par.body_add = (uint64_t)0 - (1ULL << 62);
      CHK(dev_pbs(K, L.steps.at(steps - 1), sc.small(), cn, PbsLut{sc.bit_tables() + 62}, par, tm));
      KsInput sum = work; sum.source = KS_SUM; sum.rows_b = b.par; sum.Lb = b.Lp;
      PbsLut tab2 = tab; tab2.tables = b.tab_d;
      const MarginProbe pr = probe ? probe->at(steps) : MarginProbe{};
      CHK(dev_ks_pbs(K, tier2, sum, cn, tab2, PbsOut{b.par, b.Lp}, sc, tm, probe ? &pr : nullptr));
    }
    if (steps == 0) { work.rows = b.src + c0 * b.Ls; work.L = b.Ls; work.shift = L.shift; work.body_add = L.round_add(); }   // nothing modified the input
    const MarginProbe pr = probe ? probe->at(steps + (split ? 1 : 0)) : MarginProbe{};
    CHK(dev_ks_pbs(K, tab_tier, work, cn, tab, PbsOut{w0, Lw}, sc, tm, probe ? &pr : nullptr));
    if (split) {
      const int h = tm ? tm->begin(CAT_LINEAR) : -1;
      hipLaunchKernelGGL(k_acc_rows, dim3(ew_grid(cn * (ring2 + 1))), dim3(256), 0, K->ctx->stream, w0, Lw, b.par, b.Lp, cn, ring2);
      HIPCHK(hipGetLastError());
      if (tm) tm->end(h);
    }
  }
  return 0;
}
// the mask words a rounding chain touches: its input's, and the rings of the bit tiers whose outputs it accumulates (the step entries)
static int round_chain_deff(const dctfhe_params& P, int src_deff, const LutSite& L);
static int round_chain_deff(const dctfhe_keys* K, int src_deff, const LutSite& L) { return round_chain_deff(K->p, src_deff, L); }

// can the key switch of `tier` run on the first deff rows of its key only?  (matrix-core path, whole 64-row steps; otherwise it walks the
// whole stored row and every word of it has to be meaningful)
static bool ks_narrows(const dctfhe_keys* K, int tier, int deff) {
  return K->tiers[tier].mfma() && ((size_t)deff * (size_t)K->p.tiers[tier].lk) % 64 == 0;
}

static int alloc_lut_scratch(dctfhe_keys* K, size_t chunk, LutScratch* sc) {
  int lkmax = 1, nmax = 1;
  for (int i = 0; i < K->p.n_tiers; i++) { lkmax = std::max(lkmax, K->p.tiers[i].lk); nmax = std::max(nmax, K->p.tiers[i].n); }
  sc->chunk = chunk;
  HIPCHK(sc->d_digits.alloc(chunk * (size_t)K->p.D * lkmax));
  HIPCHK(sc->d_bodies.alloc(chunk * 8));
  HIPCHK(sc->d_small.alloc(chunk * (size_t)(nmax + 1) * 8));
  int64_t bt[64];
  for (int j = 0; j < 64; j++) bt[j] = (int64_t)(1ULL << j);
  HIPCHK(sc->d_bit_tables.upload(bt, sizeof bt));
  return 0;
}

// the levels of a max-pool plan on device rows.  Input rows of stride Ls (first ds mask words meaningful); level buffers and output rows of
// stride Lo, of which the first `dout` = max(ds, ring of the tier) mask words may be non-zero.  Each level: the gather, then per chunk the
// key switch of the differences (KS_DIFF), the centred mod switch and the relu bootstrap accumulated into the gathered b rows.
// d_out is the op's whole output tensor: the plan writes its rows from P.out_first on.  launched: the pairwise maxima sent to the bootstrap.
static int dev_max_pool(dctfhe_keys* K, const PoolSite& S, const PoolPlan& P, const uint64_t* d_in, size_t Ls, size_t ds, uint64_t* const bufs[2],
                        uint64_t* d_out, size_t Lo, size_t dout, const int64_t* d_table, const LutScratch& sc, Timers* tm,
                        const MarginProbe* probe = nullptr, size_t* launched = nullptr) {
  hipStream_t st = K->ctx->stream;
  const int tier = S.tier;
  if (launched) *launched = 0;
  const int32_t* maps = P.maps.as<int32_t>();
  for (const PoolLevel& l : P.lv) {
    const uint64_t* src = l.src == 0 ? d_in : bufs[l.src - 1];
    const size_t L_src = l.src == 0 ? Ls : Lo, d_src = l.src == 0 ? ds : dout;
    uint64_t* dst = l.dst == 3 ? d_out + P.out_first * Lo : bufs[l.dst - 1];
    const int h = tm ? tm->begin(CAT_LINEAR) : -1;
    hipLaunchKernelGGL(k_pool_gather, dim3(ew_grid(l.n_dst * Lo)), dim3(256), 0, st, src, L_src, d_src, maps + l.g_off, dst, Lo, l.n_dst);
    HIPCHK(hipGetLastError());
    if (tm) tm->end(h);
    for (size_t c0 = 0; c0 < l.pairs; c0 += sc.chunk) {
      const size_t cn = std::min(sc.chunk, l.pairs - c0);
      KsInput diff;
      diff.rows = src; diff.L = L_src; diff.deff = (int)d_src; diff.shift = S.shift; diff.body_add = S.body_add;
      diff.source = KS_DIFF; diff.ia = maps + l.a_off + c0; diff.ib = maps + l.b_off + c0;
      PbsOut acc{dst + c0 * Lo, Lo}; acc.accumulate = true;
      CHK(dev_ks_pbs(K, tier, diff, cn, PbsLut{d_table, S.p_d}, acc, sc, tm, probe));
      if (launched) *launched += cn;
    }
  }
  return 0;
}
// clear mode: row pass into `mid`, column pass into out.  `mid` holds the row-pass results [mid_first, mid_first + mid_count) of
// [B*C*H][Wo] and the column pass computes the outputs [out_first, out_first + out_count) of [B*C][Ho][Wo]: everything for the whole op, a
// part's intermediates and outputs for a divided pool.  The caller guarantees that the range of intermediates covers every tap of these
// outputs (PoolPlan), so the column pass never indexes outside `mid`; the row pass reads `in` within the tensor, in bounds for any range.
static int clear_max_pool(hipStream_t st, const uint64_t* in, uint64_t* mid, uint64_t* out, int batch, int C, int H, int W, int k, int s, int p,
                          int shift, uint64_t body_add, int p_d, const int64_t* d_table, double sigma, uint64_t seed, uint64_t stream,
                          size_t mid_first, size_t mid_count, size_t out_first, size_t out_count, size_t in_base = 0, size_t out_base = 0) {
  // in_base / out_base: the elements of the op's input / output that `in` / `out` point at (0: the whole tensors; a slab of a divided
  // group: the slab's first element, so that every output keeps its number in the whole op, and with it its noise)
  const int Ho = pool_out_size(H, k, s, p), Wo = pool_out_size(W, k, s, p);
  const rng_key key{{(uint32_t)seed, (uint32_t)(seed >> 32), 0x73696d75u, 0, 0, 0, 0, 0}};
  if (mid_first + mid_count > (size_t)batch * C * H * Wo || out_first + out_count > (size_t)batch * C * Ho * Wo)
    return fail("max pool (clear): intermediates %zu .. %zu or outputs %zu .. %zu outside the op", mid_first, mid_first + mid_count, out_first, out_first + out_count);
  if (out_count == 0) return 0;
  hipLaunchKernelGGL(k_maxpool_clear, dim3(ew_grid(mid_count)), dim3(256), 0, st, in, mid, mid_first, mid_count, in_base, mid_first, W, 1, Wo, k, s, p, shift,
                     body_add, p_d, d_table, sigma, key, stream);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_maxpool_clear, dim3(ew_grid(out_count)), dim3(256), 0, st, mid, out, out_first, out_count, mid_first, out_base, H, Wo, Ho, k, s, p, shift,
                     body_add, p_d, d_table, sigma, key, stream + 1);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------ primitives on host buffers
extern "C" int dctfhe_keyswitch_prefix(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* cts, size_t count, int shift, int deff,
                                       uint64_t* cts_small) {
  if (!ctx || !K) return fail("dctfhe_keyswitch: null handle");
  CHK(bound_to("dctfhe_keyswitch", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_keyswitch", K, tier, false, true));
  if (deff < 0 || deff > K->p.D) return fail("deff out of range");
  if (shift < 0 || shift > 63) return fail("shift out of range");
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const dctfhe_tier& t = K->p.tiers[tier];
  const size_t L = (size_t)K->p.D + 1;
  DevBuf d_in;
  HIPCHK(d_in.upload(cts, count * L * 8));
  LutScratch sc;
  CHK(alloc_lut_scratch(K, count, &sc));
  KsInput in;
  in.rows = d_in.as<uint64_t>(); in.L = L; in.deff = deff; in.shift = shift;
  CHK(dev_keyswitch(K, tier, in, count, sc, nullptr));
  HIPCHK(sc.d_small.download(cts_small, count * (size_t)(t.n + 1) * 8, ctx->stream));
  return 0;
}
extern "C" int dctfhe_keyswitch(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* cts, size_t count, int shift, uint64_t* cts_small) {
  return dctfhe_keyswitch_prefix(ctx, K, tier, cts, count, shift, 0, cts_small);
}

// Packed results: `count` device rows of stride L words (the first deff mask words may be non-zero) key-switched
// to `tier` at shift 0 and rounded to 16-bit rows [count][n + 1] in HOST memory, sc.chunk ciphertexts at a time.  The packed chunk goes
// through a device buffer of its own: a chunk of odd-length rows need not end on the 8-byte boundary k_pack16 stores at.
static int dev_keyswitch_pack(dctfhe_keys* K, int tier, const uint64_t* d_rows, size_t L, int deff, size_t count, const LutScratch& sc, uint16_t* rows) {
  const size_t n1 = (size_t)K->p.tiers[tier].n + 1;
  hipStream_t st = K->ctx->stream;
  DevBuf d_pack;
  HIPCHK(d_pack.alloc(std::min(sc.chunk, count) * n1 * sizeof(uint16_t)));
  for (size_t c0 = 0; c0 < count; c0 += sc.chunk) {
    const size_t cn = std::min(sc.chunk, count - c0), words = cn * n1;
    KsInput in;
    in.rows = d_rows + c0 * L; in.L = L; in.deff = deff;
    CHK(dev_keyswitch(K, tier, in, cn, sc, nullptr));
    hipLaunchKernelGGL(k_pack16, dim3(ew_grid(words / 4)), dim3(256), 0, st, sc.small(), words, d_pack.as<uint16_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rows + c0 * n1, d_pack.p, words * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int dctfhe_keyswitch_pack(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* cts, size_t count, int dim, int deff,
                                     uint16_t* rows) {
  if (!ctx || !K || (count && (!cts || !rows))) return fail("dctfhe_keyswitch_pack: null argument");
  CHK(bound_to("dctfhe_keyswitch_pack", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("dctfhe_keyswitch_pack: tier %d out of range (%d tiers)", tier, K->p.n_tiers);
  CHK(keys_hold("dctfhe_keyswitch_pack", K, tier, false, true));
  if (dim < 1 || dim > K->p.D) return fail("dctfhe_keyswitch_pack: rows of %d mask words, the key has %d", dim, K->p.D);
  if (deff < 0 || deff > dim) return fail("dctfhe_keyswitch_pack: effective dimension %d outside [0, dim = %d]", deff, dim);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)dim + 1;
  DevBuf d_in;
  HIPCHK(d_in.upload(cts, count * L * 8));
  LutScratch sc;
  CHK(alloc_lut_scratch(K, std::min<size_t>(count, 16384), &sc));
  return dev_keyswitch_pack(K, tier, d_in.as<uint64_t>(), L, deff ? deff : dim, count, sc, rows);
}

// ---- ring-packed results (kernels.h k_ring_*): the packing key and the pack on small ciphertexts -------------
// Wire form of the key (seeded only): PackBlobHeader, the client's 32-byte public generator key, then the n_max * l * N body words.
static constexpr uint32_t PACK_BLOB_MAGIC = 0x4b505244u /* 'DRPK' */, PACK_BLOB_VERSION = 1;
struct PackBlobHeader { uint32_t magic, version; int32_t logN, l, beta, n_max; double sigma; uint64_t total_bytes; };
// the generator stream of a spec's masks (noise: + 1): a stream of its own per (logN, l, beta, sigma) -- sigma included, because the
// Gaussian draw scales with it: two exports of one client key at different sigma on ONE stream would differ by E (1 - sigma2 / sigma1)
// and give E away.  Bit 63 is set (every other stream id of these generator keys is below 2^17), bit 0 clear (the noise stream is + 1); the 62 bits between are
// the IEEE-754 bits of sigma times an odd constant (a bijection mod 2^64) xor the gadget: distinct specs meet with probability 2^-61.
static uint64_t ring_stream(int logN, int l, int beta, double sigma) {
  uint64_t sb;
  memcpy(&sb, &sigma, 8);
  const uint64_t mix = (sb * 0x9E3779B97F4A7C15ULL) ^ (((uint64_t)logN << 24) | ((uint64_t)l << 16) | ((uint64_t)beta << 8));
  return (1ULL << 63) | (mix & 0x7FFFFFFFFFFFFFFEULL);
}
static int check_pack_spec(const char* who, int logN, int l, int beta, int n_max, double sigma, int D) {
  if (logN < 5 || logN > 12) return fail("%s: ring 2^%d outside 2^5 .. 2^12", who, logN);
  if (D > 0 && (1 << logN) > D) return fail("%s: the ring key is a prefix of the big key: N_p = %d > D = %d", who, 1 << logN, D);
  if (l < 1 || beta < 1 || beta > 32) return fail("%s: %d levels of %d bits (levels >= 1, 1 <= bits <= 32)", who, l, beta);
  if (l * beta > 63) return fail("%s: gadget of %d x %d bits exceeds 63", who, l, beta);
  if (n_max < 1) return fail("%s: a small key of %d bits", who, n_max);
  if (!(sigma >= 0.0) || sigma >= 1.0) return fail("%s: noise std %g outside [0, 1)", who, sigma);
  return 0;
}
static size_t pack_blob_size(int logN, int l, int n_max) { return sizeof(PackBlobHeader) + 32 + ((size_t)n_max * l << logN) * 8; }

struct dctfhe_pack_key {
  dctfhe_ctx* ctx = nullptr;
  int logN = 0, l = 0, beta = 0, n_max = 0;
  double sigma = 0;
  DevBuf key;                    // u64 [n_max][l][2][N]
  ~dctfhe_pack_key() { if (ctx) hipSetDevice(ctx->device); }
};

extern "C" int dctfhe_pack_key_export(dctfhe_client_key* C, int logN, int l, int beta, double sigma, void* buf, size_t capacity, size_t* size) {
  if (!C || !size) return fail("dctfhe_pack_key_export: null argument");
  CHK(check_pack_spec("dctfhe_pack_key_export", logN, l, beta, C->p.n_max, sigma, C->p.D));
  const size_t need = pack_blob_size(logN, l, C->p.n_max);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_pack_key_export: buffer of %zu bytes, %zu needed", capacity, need);
  HIPCHK(hipSetDevice(C->ctx->device));
  const int N = 1 << logN, rows = C->p.n_max * l;
  PackBlobHeader h{};
  h.magic = PACK_BLOB_MAGIC; h.version = PACK_BLOB_VERSION; h.logN = logN; h.l = l; h.beta = beta; h.n_max = C->p.n_max; h.sigma = sigma;
  h.total_bytes = need;
  char* q = (char*)buf;
  memcpy(q, &h, sizeof h); q += sizeof h;
  key_to_bytes(C->pub, (uint8_t*)q); q += 32;
  DevBuf d_b;
  HIPCHK(d_b.alloc((size_t)rows * N * 8));
  hipLaunchKernelGGL(k_ring_key_gen, dim3((unsigned)rows), dim3(256), (size_t)N * 8, C->ctx->stream, C->s(), C->S(), N, l, beta, sigma, C->pub, C->sec,
                     ring_stream(logN, l, beta, sigma), d_b.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(d_b.download(q, (size_t)rows * N * 8, C->ctx->stream));
  return 0;
}
extern "C" int dctfhe_pack_key_import(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_pack_key** out) {
  if (!ctx || !buf || !out) return fail("dctfhe_pack_key_import: null argument");
  if (size < sizeof(PackBlobHeader) + 32) return fail("dctfhe_pack_key_import: packing-key blob too short (%zu bytes)", size);
  PackBlobHeader h;
  memcpy(&h, buf, sizeof h);
  if (h.magic != PACK_BLOB_MAGIC) return fail("dctfhe_pack_key_import: not a packing-key blob (magic)");
  if (h.version != PACK_BLOB_VERSION) return fail("dctfhe_pack_key_import: packing-key blob version %u, this library reads %u", h.version, PACK_BLOB_VERSION);
  CHK(check_pack_spec("dctfhe_pack_key_import", h.logN, h.l, h.beta, h.n_max, h.sigma, 0));
  if (h.total_bytes != size || pack_blob_size(h.logN, h.l, h.n_max) != size)
    return fail("dctfhe_pack_key_import: packing-key blob of %zu bytes, its header needs %zu (length)", size, pack_blob_size(h.logN, h.l, h.n_max));
  HIPCHK(hipSetDevice(ctx->device));
  std::unique_ptr<dctfhe_pack_key> K(new dctfhe_pack_key);
  K->ctx = ctx; K->logN = h.logN; K->l = h.l; K->beta = h.beta; K->n_max = h.n_max; K->sigma = h.sigma;
  const size_t N = (size_t)1 << h.logN, rows = (size_t)h.n_max * h.l;
  const rng_key pub = key_from_bytes((const uint8_t*)buf + sizeof h);
  DevBuf d_b;
  HIPCHK(d_b.upload((const char*)buf + sizeof h + 32, rows * N * 8));
  HIPCHK(K->key.alloc(rows * 2 * N * 8));
  CHK(launch_expand(pub, ring_stream(h.logN, h.l, h.beta, h.sigma), 0, N, (int)N, ~0ULL, d_b.as<uint64_t>(), (int)N, rows, 2 * N, K->key.as<uint64_t>(), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *out = K.release();
  return 0;
}
extern "C" int dctfhe_pack_key_destroy(dctfhe_pack_key* K) { delete K; return 0; }
extern "C" int dctfhe_pack_key_info(dctfhe_pack_key* K, int* logN, int* l, int* beta, int* n_max, double* sigma) {
  if (!K) return fail("dctfhe_pack_key_info: null argument");
  if (logN) *logN = K->logN;
  if (l) *l = K->l;
  if (beta) *beta = K->beta;
  if (n_max) *n_max = K->n_max;
  if (sigma) *sigma = K->sigma;
  return 0;
}
// test view: the expanded key [n_max][l][2][N]
extern "C" int dctfhe_pack_key_export_rows(dctfhe_pack_key* K, uint64_t* out) {
  if (!K || !out) return fail("dctfhe_pack_key_export_rows: null argument");
  HIPCHK(hipSetDevice(K->ctx->device));
  HIPCHK(K->key.download(out, K->key.bytes, K->ctx->stream));
  return 0;
}
extern "C" size_t dctfhe_ring_words(int logN, size_t count) {
  if (logN < 0 || logN > 30) return 0;
  return (((count + ((size_t)1 << logN) - 1) >> logN) << logN) + count;
}

// `count` device small ciphertexts (rows of n + 1 words) -> their ring-packed wire words in HOST memory, as many whole groups at a time
// as 64 MB of transposed digits hold
static int dev_ring_pack(dctfhe_pack_key* K, const uint64_t* d_small, size_t count, int n, uint16_t* out) {
  hipStream_t st = K->ctx->stream;
  const size_t N = (size_t)1 << K->logN, groups = (count + N - 1) / N, dig_per_group = (size_t)n * K->l * N;
  const size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(groups, 4096), ((size_t)64 << 20) / (dig_per_group * 4)));
  DevBuf d_dig, d_out;
  HIPCHK(d_dig.alloc(G * dig_per_group * 4));
  HIPCHK(d_out.alloc(G * 2 * N * sizeof(uint16_t)));
  const size_t lds = N * 8 + N * 4;
  for (size_t g0 = 0; g0 < groups; g0 += G) {
    const size_t gn = std::min(G, groups - g0), cn = std::min(count - g0 * N, gn * N);
    const uint64_t* src = d_small + g0 * N * (size_t)(n + 1);
    hipLaunchKernelGGL(k_ring_digits, dim3(ew_grid(gn * (size_t)n * N)), dim3(256), 0, st, src, cn, n, K->logN, K->l, K->beta, d_dig.as<int32_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ring_pack, dim3((unsigned)(gn * 2 * (N / RING_TILE))), dim3(256), lds, st, d_dig.as<int32_t>(), src, cn, n, K->logN, K->l,
                       K->key.as<uint64_t>(), d_out.as<uint16_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out + g0 * 2 * N, d_out.p, dctfhe_ring_words(K->logN, cn) * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int dctfhe_ring_pack(dctfhe_ctx* ctx, dctfhe_pack_key* K, const uint64_t* cts_small, size_t count, int n, uint16_t* out) {
  if (!ctx || !K || (count && (!cts_small || !out))) return fail("dctfhe_ring_pack: null argument");
  if (K->ctx != ctx) return fail("dctfhe_ring_pack: the packing key was imported on another context");
  if (n < 1 || n > K->n_max) return fail("dctfhe_ring_pack: small ciphertexts of %d mask words, the packing key covers n_max = %d", n, K->n_max);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf d_small;
  HIPCHK(d_small.upload(cts_small, count * (size_t)(n + 1) * 8));
  return dev_ring_pack(K, d_small.as<uint64_t>(), count, n, out);
}
// CLIENT: phases of ring-packed results under the first 2^logN bits of the big key
extern "C" int dctfhe_decrypt_ring(dctfhe_ctx* ctx, dctfhe_client_key* C, int logN, const uint16_t* words, size_t count, uint64_t* phases) {
  if (!ctx || !C || (count && (!words || !phases))) return fail("dctfhe_decrypt_ring: null argument");
  CHK(bound_to("dctfhe_decrypt_ring", ctx, C->ctx, "client key"));
  if (logN < 5 || logN > 12) return fail("dctfhe_decrypt_ring: ring 2^%d outside 2^5 .. 2^12", logN);
  if ((1 << logN) > C->p.D) return fail("dctfhe_decrypt_ring: the ring key is a prefix of the big key: N_p = %d > D = %d", 1 << logN, C->p.D);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t N = (size_t)1 << logN, groups = (count + N - 1) / N, bytes = dctfhe_ring_words(logN, count) * sizeof(uint16_t);
  DevBuf d_w, d_ph;
  HIPCHK(d_w.alloc(bytes));
  HIPCHK(d_ph.alloc(count * 8));
  HIPCHK(hipMemcpyAsync(d_w.p, words, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_ring_phase16, dim3((unsigned)(groups * ((N + 255) / 256))), dim3(256), N * 3, ctx->stream, C->S(), logN, d_w.as<uint16_t>(), count,
                     d_ph.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(phases, d_ph.p, count * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ---- public-key inputs (kernels.h k_pk_*): the key, the encryptor without a secret, the extraction
// Wire form of the key (seeded only): PubBlobHeader, the client's 32-byte public generator key, then the N_e body words.
static constexpr uint32_t PUB_BLOB_MAGIC = 0x4b425044u /* 'DPBK' */, PUB_BLOB_VERSION = 1;
struct PubBlobHeader { uint32_t magic, version; int32_t logN, reserved; double sigma; uint64_t total_bytes; };
// the generator stream of the key's mask (noise: + 1), a stream of its own per (logN, sigma) for the reason given at ring_stream.  Bit 62
// is set and bit 63 clear: the packing-key streams have bit 63 set and every other id of these generator keys is below 2^17.
static uint64_t public_key_stream(int logN, double sigma) {
  uint64_t sb;
  memcpy(&sb, &sigma, 8);
  const uint64_t mix = (sb * 0x9E3779B97F4A7C15ULL) ^ ((uint64_t)logN << 24);
  return (1ULL << 62) | (mix & 0x3FFFFFFFFFFFFFFEULL);
}
static int check_public_spec(const char* who, int logN, double sigma, int dim) {
  if (logN < 5 || logN > 12) return fail("%s: ring 2^%d outside 2^5 .. 2^12", who, logN);
  if (dim > 0 && (1 << logN) > dim) return fail("%s: the ring key is a prefix of what an input masks: N_e = %d > %d", who, 1 << logN, dim);
  if (!(sigma >= 0.0) || sigma >= 1.0) return fail("%s: noise std %g outside [0, 1)", who, sigma);
  return 0;
}
static size_t pub_blob_size(int logN) { return sizeof(PubBlobHeader) + 32 + ((size_t)8 << logN); }

struct dctfhe_public_key {
  dctfhe_ctx* ctx = nullptr;
  int logN = 0;
  double sigma = 0;
  DevBuf key;                    // u64 [2][N_e]: A, B
  rng_key enc{};                 // the encryptor's own generator key (32 bytes from the OS at import)
  uint64_t calls = 0;            // call c draws from streams 3 c (u), 3 c + 1 (e1), 3 c + 2 (e2)
  ~dctfhe_public_key() { if (ctx) hipSetDevice(ctx->device); }
};
static constexpr uint64_t PUB_MAX_CALLS = 1ULL << 62;      // 3 c + 2 stays inside 64 bits

extern "C" int dctfhe_public_key_export(dctfhe_client_key* C, int logN, double sigma, void* buf, size_t capacity, size_t* size) {
  if (!C || !size) return fail("dctfhe_public_key_export: null argument");
  CHK(check_public_spec("dctfhe_public_key_export", logN, sigma, C->p.input_dim > 0 ? C->p.input_dim : C->p.D));
  const size_t need = pub_blob_size(logN);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_public_key_export: buffer of %zu bytes, %zu needed", capacity, need);
  HIPCHK(hipSetDevice(C->ctx->device));
  const int N = 1 << logN;
  PubBlobHeader h{};
  h.magic = PUB_BLOB_MAGIC; h.version = PUB_BLOB_VERSION; h.logN = logN; h.sigma = sigma; h.total_bytes = need;
  char* q = (char*)buf;
  memcpy(q, &h, sizeof h); q += sizeof h;
  key_to_bytes(C->pub, (uint8_t*)q); q += 32;
  DevBuf d_b;
  HIPCHK(d_b.alloc((size_t)N * 8));
  hipLaunchKernelGGL(k_pk_gen, dim3(1), dim3(256), (size_t)N * 8, C->ctx->stream, C->S(), N, sigma, C->pub, C->sec, public_key_stream(logN, sigma), d_b.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(d_b.download(q, (size_t)N * 8, C->ctx->stream));
  return 0;
}
extern "C" int dctfhe_public_key_import(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_public_key** out) {
  if (!ctx || !buf || !out) return fail("dctfhe_public_key_import: null argument");
  if (size < sizeof(PubBlobHeader) + 32) return fail("dctfhe_public_key_import: public-key blob too short (%zu bytes)", size);
  PubBlobHeader h;
  memcpy(&h, buf, sizeof h);
  if (h.magic != PUB_BLOB_MAGIC) return fail("dctfhe_public_key_import: not a public-key blob (magic)");
  if (h.version != PUB_BLOB_VERSION) return fail("dctfhe_public_key_import: public-key blob version %u, this library reads %u", h.version, PUB_BLOB_VERSION);
  CHK(check_public_spec("dctfhe_public_key_import", h.logN, h.sigma, 0));
  if (h.total_bytes != size || pub_blob_size(h.logN) != size)
    return fail("dctfhe_public_key_import: public-key blob of %zu bytes, its header needs %zu (length)", size, pub_blob_size(h.logN));
  HIPCHK(hipSetDevice(ctx->device));
  std::unique_ptr<dctfhe_public_key> K(new dctfhe_public_key);
  K->ctx = ctx; K->logN = h.logN; K->sigma = h.sigma;
  {  // the encryptor's generator key from the OS: two handles, even of one blob, never share a draw
    uint8_t raw[32];
    size_t got = 0;
    while (got < sizeof raw) {
      const ssize_t r = getrandom(raw + got, sizeof raw - got, 0);
      if (r <= 0) return fail("dctfhe_public_key_import: the OS gave no random bytes for the encryption key (getrandom)");
      got += (size_t)r;
    }
    K->enc = key_from_bytes(raw);
  }
  const size_t N = (size_t)1 << h.logN;
  DevBuf d_b;
  HIPCHK(d_b.upload((const char*)buf + sizeof h + 32, N * 8));
  HIPCHK(K->key.alloc(2 * N * 8));
  CHK(launch_expand(key_from_bytes((const uint8_t*)buf + sizeof h), public_key_stream(h.logN, h.sigma), 0, N, (int)N, ~0ULL, d_b.as<uint64_t>(), (int)N, 1, 2 * N,
                    K->key.as<uint64_t>(), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *out = K.release();
  return 0;
}
extern "C" int dctfhe_public_key_destroy(dctfhe_public_key* K) { delete K; return 0; }
extern "C" int dctfhe_public_key_info(dctfhe_public_key* K, int* logN, double* sigma) {
  if (!K) return fail("dctfhe_public_key_info: null argument");
  if (logN) *logN = K->logN;
  if (sigma) *sigma = K->sigma;
  return 0;
}
// test view: the expanded key [2][N_e] (A then B)
extern "C" int dctfhe_public_key_export_rows(dctfhe_public_key* K, uint64_t* out) {
  if (!K || !out) return fail("dctfhe_public_key_export_rows: null argument");
  HIPCHK(hipSetDevice(K->ctx->device));
  HIPCHK(K->key.download(out, K->key.bytes, K->ctx->stream));
  return 0;
}
// reproducible tests only: fix the encryptor's generator key and restart its call counter
extern "C" int dctfhe_public_key_set_encrypt_seed(dctfhe_public_key* K, const uint8_t* seed32) {
  if (!K || !seed32) return fail("dctfhe_public_key_set_encrypt_seed: null argument");
  K->enc = key_from_bytes(seed32);
  K->calls = 0;
  return 0;
}
extern "C" size_t dctfhe_public_words(int logN, size_t count) { return dctfhe_ring_words(logN, count); }

// the draws of call `call` for `count` phases, on the device: u i32 [groups N_e], e1 i64 [groups N_e], e2 i64 [count]
static int dev_public_draws(dctfhe_public_key* K, uint64_t call, size_t count, DevBuf* u, DevBuf* e1, DevBuf* e2) {
  const size_t N = (size_t)1 << K->logN, nmask = (count + N - 1) / N * N;
  HIPCHK(u->alloc(nmask * 4));
  HIPCHK(e1->alloc(nmask * 8));
  HIPCHK(e2->alloc(count * 8));
  hipLaunchKernelGGL(k_pk_draws, dim3(ew_grid(nmask)), dim3(256), 0, K->ctx->stream, K->enc, 3 * call, nmask, count, K->sigma, u->as<int32_t>(), e1->as<int64_t>(),
                     e2->as<int64_t>());
  HIPCHK(hipGetLastError());
  return 0;
}
// test view: what call `call` of dctfhe_encrypt_public draws for `count` phases -- u one byte per bit [groups N_e], e1 [groups N_e], e2 [count]
extern "C" int dctfhe_public_key_draws(dctfhe_public_key* K, uint64_t call, size_t count, uint8_t* u, int64_t* e1, int64_t* e2) {
  if (!K || !u || !e1 || !e2) return fail("dctfhe_public_key_draws: null argument");
  if (count == 0) return fail("dctfhe_public_key_draws: no phases (count == 0)");
  if (call >= PUB_MAX_CALLS) return fail("dctfhe_public_key_draws: call counter out of range");
  HIPCHK(hipSetDevice(K->ctx->device));
  const size_t N = (size_t)1 << K->logN, nmask = (count + N - 1) / N * N;
  DevBuf d_u, d_e1, d_e2;
  CHK(dev_public_draws(K, call, count, &d_u, &d_e1, &d_e2));
  std::vector<int32_t> u32(nmask);
  HIPCHK(d_u.download(u32.data(), nmask * 4, K->ctx->stream));
  for (size_t x = 0; x < nmask; x++) u[x] = (uint8_t)u32[x];
  HIPCHK(d_e1.download(e1, nmask * 8, K->ctx->stream));
  HIPCHK(d_e2.download(e2, count * 8, K->ctx->stream));
  return 0;
}
// ENCRYPTOR: `count` phases -> dctfhe_public_words(logN, count) wire words; one step of the handle's call counter
extern "C" int dctfhe_encrypt_public(dctfhe_ctx* ctx, dctfhe_public_key* K, const uint64_t* phases, size_t count, uint64_t* words_out) {
  if (!ctx || !K || !phases || !words_out) return fail("dctfhe_encrypt_public: null argument");
  if (K->ctx != ctx) return fail("dctfhe_encrypt_public: the public key was imported on another context");
  if (count == 0) return fail("dctfhe_encrypt_public: no phases (count == 0)");
  if (K->calls >= PUB_MAX_CALLS) return fail("dctfhe_encrypt_public: this handle's call counter is exhausted");
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)1 << K->logN, groups = (count + N - 1) / N, nwords = dctfhe_ring_words(K->logN, count);
  DevBuf d_ph, d_u, d_e1, d_e2, d_out;
  HIPCHK(d_ph.alloc(count * 8));
  HIPCHK(d_out.alloc(nwords * 8));
  HIPCHK(hipMemcpyAsync(d_ph.p, phases, count * 8, hipMemcpyHostToDevice, st));
  CHK(dev_public_draws(K, K->calls++, count, &d_u, &d_e1, &d_e2));      // the counter moves even if a later step fails: a draw is never reused
  hipLaunchKernelGGL(k_pk_encrypt, dim3((unsigned)(groups * 2 * (N / RING_TILE))), dim3(256), N * 8 + N * 4, st, d_u.as<int32_t>(), d_e1.as<int64_t>(),
                     d_e2.as<int64_t>(), d_ph.as<uint64_t>(), count, K->logN, K->key.as<uint64_t>(), d_out.as<uint64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(words_out, d_out.p, nwords * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
// device wire words -> rows at stride L (body at word L - 1) starting at d_rows
static int launch_ring_extract(int logN, const uint64_t* d_words, size_t count, size_t L, uint64_t* d_rows, hipStream_t st) {
  const size_t N = (size_t)1 << logN, groups = (count + N - 1) / N;
  hipLaunchKernelGGL(k_pk_extract, dim3((unsigned)(groups * (N / EXTRACT_TILE))), dim3(256), N * 8, st, d_words, count, logN, L, d_rows);
  HIPCHK(hipGetLastError());
  return 0;
}
static constexpr size_t PUB_MAX_COUNT = (size_t)1 << 30;      // keeps groups x tiles inside a 32-bit grid
// SERVER, the primitive on host buffers: wire words of `count` public-key inputs -> LWE rows of dim mask words + body
extern "C" int dctfhe_ring_extract(dctfhe_ctx* ctx, int logN, const uint64_t* words, size_t count, int dim, uint64_t* rows_out) {
  if (!ctx || !words || !rows_out) return fail("dctfhe_ring_extract: null argument");
  if (logN < 5 || logN > 12) return fail("dctfhe_ring_extract: ring 2^%d outside 2^5 .. 2^12", logN);
  if (count == 0 || count > PUB_MAX_COUNT) return fail("dctfhe_ring_extract: %zu inputs (1 .. 2^30)", count);
  if (dim < (1 << logN) || dim > (1 << 20)) return fail("dctfhe_ring_extract: rows of %d mask words, a slot of this ring fills N_e = %d (N_e <= dim <= 2^20)", dim, 1 << logN);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)dim + 1, nwords = dctfhe_ring_words(logN, count);
  DevBuf d_w, d_r;
  HIPCHK(d_w.alloc(nwords * 8));
  HIPCHK(d_r.alloc(count * L * 8));
  HIPCHK(hipMemcpyAsync(d_w.p, words, nwords * 8, hipMemcpyHostToDevice, ctx->stream));
  CHK(launch_ring_extract(logN, d_w.as<uint64_t>(), count, L, d_r.as<uint64_t>(), ctx->stream));
  HIPCHK(hipMemcpyAsync(rows_out, d_r.p, count * L * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// the centred mod switch on host buffers (the scheduler applies it between every key switch and its bootstrap)
extern "C" int dctfhe_modswitch_center(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, uint64_t* cts_small, size_t count) {
  if (!ctx || !K || (count && !cts_small)) return fail("dctfhe_modswitch_center: null argument");
  CHK(bound_to("dctfhe_modswitch_center", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_modswitch_center", K, tier, true, false));      // it rounds to the levels of this tier's bootstrap
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t bytes = count * (size_t)(K->p.tiers[tier].n + 1) * 8;
  DevBuf d;
  HIPCHK(d.upload(cts_small, bytes));
  CHK(dev_ms_center(K, tier, d.as<uint64_t>(), count, nullptr));
  HIPCHK(d.download(cts_small, bytes, ctx->stream));
  return 0;
}

extern "C" int dctfhe_pbs(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* cts_small, size_t count, const int64_t* tables, int ntab,
                          int w, const int32_t* table_idx, uint64_t* cts_out) {
  if (!ctx || !K) return fail("dctfhe_pbs: null handle");
  CHK(bound_to("dctfhe_pbs", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_pbs", K, tier, true, false));
  if (ntab < 1 || w < 0) return fail("dctfhe_pbs: need at least one table and w >= 0");
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const dctfhe_tier& t = K->p.tiers[tier];
  if (w > t.logN - 1) return fail("table of 2^%d entries does not fit N = 2^%d", w, t.logN);
  if (table_idx)
    for (size_t i = 0; i < count; i++)
      if (table_idx[i] < 0 || table_idx[i] >= ntab) return fail("table_idx[%zu] = %d out of range (%d tables)", i, table_idx[i], ntab);
  const size_t L = (size_t)K->p.D + 1;
  DevBuf d_small, d_out, d_tab, d_idx;
  HIPCHK(d_small.upload(cts_small, count * (size_t)(t.n + 1) * 8));
  HIPCHK(d_out.alloc(count * L * 8));
  HIPCHK(d_tab.upload(tables, ((size_t)ntab << w) * 8));
  if (table_idx) HIPCHK(d_idx.upload(table_idx, count * 4));
  PbsLut lut;
  lut.tables = d_tab.as<int64_t>(); lut.w = w; lut.idx = d_idx.as<int32_t>();
  CHK(dev_pbs(K, tier, d_small.as<uint64_t>(), count, lut, PbsOut{d_out.as<uint64_t>(), L}, nullptr));
  HIPCHK(d_out.download(cts_out, count * L * 8, ctx->stream));
  return 0;
}

// tab_tier2 >= 0: parity split (dev_round_lut) -- the table's low bit goes through one more one-bit step on bit_tier, the two half-table
// look-ups run on tab_tier and tab_tier2
extern "C" int dctfhe_round_lut_split(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int bit_tier, int tab_tier, int tab_tier2, const uint64_t* cts, size_t count,
                                      int p, int r, const int64_t* tables, int ntab, int w, const int32_t* table_idx, uint64_t* cts_out) {
  if (!ctx || !K) return fail("dctfhe_round_lut: null handle");
  CHK(bound_to("dctfhe_round_lut", ctx, K->ctx, "evaluation keys"));
  const bool split = tab_tier2 >= 0;
  if (tab_tier < 0 || tab_tier >= K->p.n_tiers || tab_tier2 >= K->p.n_tiers || ((r > 0 || split) && (bit_tier < 0 || bit_tier >= K->p.n_tiers)))
    return fail("tier out of range");
  CHK(keys_hold("dctfhe_round_lut", K, tab_tier, true, true));
  if (split) CHK(keys_hold("dctfhe_round_lut", K, tab_tier2, true, true));
  if (r > 0 || split) CHK(keys_hold("dctfhe_round_lut", K, bit_tier, true, true));
  if (p < 1 || p > 62 || r < 0 || r >= p) return fail("need 1 <= p <= 62 and 0 <= r < p");
  if (w != p - r) return fail("w must equal p - r");
  if (split && w < 2) return fail("a parity split needs a table of at least 2 input bits");
  const int wl = split ? w - 1 : w;      // input bits of the look-ups that run
  if (wl > K->p.tiers[tab_tier].logN - 1) return fail("table of 2^%d entries does not fit tier %d", wl, tab_tier);
  if (split && wl > K->p.tiers[tab_tier2].logN - 1) return fail("table of 2^%d entries does not fit tier %d", wl, tab_tier2);
  if (ntab < 1) return fail("need at least one table");
  if (!tables) return fail("dctfhe_round_lut: null tables");
  std::vector<int64_t> halves;
  if (split && split_tables_host(tables, (size_t)ntab, w, &halves)) return fail("parity split of a table whose entry pairs have an odd sum");
  if (count == 0) return 0;
  if (table_idx)
    for (size_t i = 0; i < count; i++)
      if (table_idx[i] < 0 || table_idx[i] >= ntab) return fail("table_idx[%zu] = %d out of range (%d tables)", i, table_idx[i], ntab);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)K->p.D + 1;
  DevBuf d_work, d_tab, d_idx, d_par;
  HIPCHK(d_work.upload(cts, count * L * 8));
  HIPCHK(d_tab.upload(split ? halves.data() : tables, ((size_t)ntab << w) * 8));
  if (table_idx) HIPCHK(d_idx.upload(table_idx, count * 4));
  LutScratch sc;
  CHK(alloc_lut_scratch(K, std::min<size_t>(count, 4096), &sc));
  // the site a record of this look-up would decode to (rows arrive shifted and offset; without an index every ciphertext takes table 0)
  LutSite site;
  site.p = p; site.r = r; site.w = w; site.ntab = table_idx ? ntab : 1; site.tab_tier = tab_tier; site.steps.bit = bit_tier;
  LutRows rows;
  rows.src = rows.work = d_work.as<uint64_t>(); rows.Ls = rows.Lw = L;
  rows.tables = d_tab.as<int64_t>(); rows.idx = d_idx.as<int32_t>();
  if (split) {
    HIPCHK(d_par.alloc(sc.chunk * L * 8));
    site.mode = LUT_SPLIT; site.tier2_named = tab_tier2;
    rows.par = d_par.as<uint64_t>(); rows.Lp = L;
    rows.tab_s = d_tab.as<int64_t>(); rows.tab_d = d_tab.as<int64_t>() + ((size_t)ntab << (w - 1));
  }
  if (r > 0) {
    hipLaunchKernelGGL(k_affine, dim3(ew_grid(count * L)), dim3(256), 0, ctx->stream, d_work.as<uint64_t>(), L, L - 1, d_work.as<uint64_t>(), L, count, L - 1, 0,
                       1ULL << (63 - p + r - 1));
    HIPCHK(hipGetLastError());
  }
  CHK(dev_round_lut(K, site, rows, count, 1, sc, nullptr, 0));
  HIPCHK(d_work.download(cts_out, count * L * 8, ctx->stream));
  return 0;
}
// A table of 7 input bits is split inside (both look-ups on tab_tier): at the half-box of a 6-bit table instead of half of it
extern "C" int dctfhe_round_lut(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int bit_tier, int tab_tier, const uint64_t* cts, size_t count, int p, int r,
                                const int64_t* tables, int ntab, int w, const int32_t* table_idx, uint64_t* cts_out) {
  return dctfhe_round_lut_split(ctx, K, bit_tier, tab_tier, w == 7 ? tab_tier : -1, cts, count, p, r, tables, ntab, w, table_idx, cts_out);
}

// K1 one kernel at a time on host buffers, on rows at an effective dimension (the storage form of a session's tensors; see the K2 entry
// points below): the same dev_conv2d and the same ConvPack as the session, so the matrix-core kernel runs exactly when it would there
static int rows_ok(const char* what, int dim, int deff) {
  if (dim < 0 || deff < 0 || deff > dim || dim > (1 << 16)) return fail("%s: rows of %d mask words with effective dimension %d", what, dim, deff);
  return 0;
}
static int conv2d_rows(const char* what, dctfhe_ctx* ctx, const uint64_t* in, int dim_in, int deff_in, int batch, int Cin, int H, int W, const int8_t* weight,
                       int Cout, int KH, int KW, int stride, int pad, int dim_o, uint64_t* out, const ConvWindow* window = nullptr) {
  if (!ctx) return fail("%s: null context", what);
  if (!in || !weight || !out) return fail("%s: null argument", what);
  if (dim_in < 0 || dim_o < 0 || batch < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0) return fail("%s: bad geometry", what);
  if (H + 2 * pad < KH || W + 2 * pad < KW) return fail("%s: kernel larger than the padded input", what);
  CHK(rows_ok(what, dim_in, deff_in));
  if (dim_o < deff_in || dim_o > (1 << 16)) return fail("%s: output rows of %d mask words cannot hold the result (%d needed)", what, dim_o, deff_in);
  if (window && window->c0 >= window->c1) return fail("%s: empty output window: channels [%d, %d)", what, window->c0, window->c1);
  if (window && (window->c0 < 0 || window->c1 > Cout)) return fail("%s: output window of channels [%d, %d) outside the %d the weights hold", what, window->c0, window->c1, Cout);
  const int Cwin = window ? window->c1 - window->c0 : Cout;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t Li = (size_t)dim_in + 1, Lo = (size_t)dim_o + 1;
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  const size_t nin = (size_t)batch * Cin * H * W * Li, nout = (size_t)batch * Cwin * Ho * Wo * Lo, nw = (size_t)Cout * Cin * KH * KW;
  DevBuf d_in, d_out, d_w;
  HIPCHK(d_in.upload(in, nin * 8));
  HIPCHK(d_out.alloc(nout * 8));
  HIPCHK(d_w.upload(weight, nw));
  DevBuf slab;
  std::vector<ConvPack> pk;
  CHK(build_conv_packs({weight}, {ConvSite{Cout, Cin, H, W, KH, KW, stride, pad}}, &slab, &pk));
  CHK(dev_conv2d(ctx, d_in.as<uint64_t>(), batch, Cin, H, W, Li, (size_t)deff_in, d_w.as<int8_t>(), &pk[0], Cout, KH, KW, stride, pad, d_out.as<uint64_t>(), Lo,
                 window));
  HIPCHK(d_out.download(out, nout * 8, ctx->stream));
  return 0;
}
extern "C" int dctfhe_conv2d_rows(dctfhe_ctx* ctx, const uint64_t* in, int dim_in, int deff_in, int batch, int Cin, int H, int W, const int8_t* weight, int Cout,
                                  int KH, int KW, int stride, int pad, int dim_o, uint64_t* out) {
  return conv2d_rows("dctfhe_conv2d_rows", ctx, in, dim_in, deff_in, batch, Cin, H, W, weight, Cout, KH, KW, stride, pad, dim_o, out);
}
// output channels [c0, c1) only: out is [batch][c1 - c0][Ho][Wo] rows, launched in pixel chunks (dev_conv2d), so no pixel count is refused
extern "C" int dctfhe_conv2d_rows_window(dctfhe_ctx* ctx, const uint64_t* in, int dim_in, int deff_in, int batch, int Cin, int H, int W, const int8_t* weight,
                                         int Cout, int KH, int KW, int stride, int pad, int dim_o, int c0, int c1, uint64_t* out) {
  const ConvWindow window{c0, c1};
  return conv2d_rows("dctfhe_conv2d_rows_window", ctx, in, dim_in, deff_in, batch, Cin, H, W, weight, Cout, KH, KW, stride, pad, dim_o, out, &window);
}
// full-width rows: dim_in = deff_in = dim_o = D (under its own name, so that its messages read as they always did)
extern "C" int dctfhe_conv2d(dctfhe_ctx* ctx, int D, const uint64_t* in, int batch, int Cin, int H, int W, const int8_t* weight, int Cout,
                             int KH, int KW, int stride, int pad, uint64_t* out) {
  return conv2d_rows("dctfhe_conv2d", ctx, in, D, D, batch, Cin, H, W, weight, Cout, KH, KW, stride, pad, D, out);
}

// ---- K2 (residual add, rounding offset / shift, window-sum pooling) one kernel at a time on host buffers.  Rows of `dim` mask words +
// body of which the first `deff` may be non-zero -- the storage form of the session's tensors, so that the kernels are checked at mixed
// effective dimensions outside a circuit (reference backbone.py:102 torch.add, :276 AvgPool2d).
extern "C" int dctfhe_add_rows(dctfhe_ctx* ctx, const uint64_t* a, int dim_a, int deff_a, const uint64_t* b, int dim_b, int deff_b, size_t count, int dim_o,
                               uint64_t* out) {
  if (!ctx || !a || !b || !out) return fail("dctfhe_add_rows: null argument");
  CHK(rows_ok("dctfhe_add_rows (a)", dim_a, deff_a));
  CHK(rows_ok("dctfhe_add_rows (b)", dim_b, deff_b));
  if (dim_o < std::max(deff_a, deff_b) || dim_o > (1 << 16)) return fail("dctfhe_add_rows: output rows of %d mask words cannot hold the sum (%d needed)", dim_o, std::max(deff_a, deff_b));
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t La = (size_t)dim_a + 1, Lb = (size_t)dim_b + 1, Lo = (size_t)dim_o + 1;
  DevBuf da, db, d_o;
  HIPCHK(da.upload(a, count * La * 8)); HIPCHK(db.upload(b, count * Lb * 8)); HIPCHK(d_o.alloc(count * Lo * 8));
  hipLaunchKernelGGL(k_add, dim3(ew_grid(count * Lo)), dim3(256), 0, ctx->stream, da.as<uint64_t>(), La, (size_t)deff_a, db.as<uint64_t>(), Lb, (size_t)deff_b,
                     d_o.as<uint64_t>(), Lo, count);
  HIPCHK(hipGetLastError());
  HIPCHK(d_o.download(out, count * Lo * 8, ctx->stream));
  return 0;
}
// inout: rows of dim_o + 1 words; the kernel writes the first nwords mask words (a << shift; zero from deff_a on) and the body
// ((body << shift) + body_add) and leaves the words in between as they were (what the rounding chain relies on: dctfhe_session_run)
extern "C" int dctfhe_affine_rows(dctfhe_ctx* ctx, const uint64_t* a, int dim_a, int deff_a, size_t count, int nwords, int shift, uint64_t body_add, int dim_o,
                                  uint64_t* inout) {
  if (!ctx || !a || !inout) return fail("dctfhe_affine_rows: null argument");
  CHK(rows_ok("dctfhe_affine_rows", dim_a, deff_a));
  if (dim_o < 0 || dim_o > (1 << 16) || nwords < 0 || nwords > dim_o || shift < 0 || shift > 63) return fail("dctfhe_affine_rows: bad output geometry (nwords <= dim_o, 0 <= shift <= 63)");
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t La = (size_t)dim_a + 1, Lo = (size_t)dim_o + 1;
  DevBuf da, d_o;
  HIPCHK(da.upload(a, count * La * 8)); HIPCHK(d_o.upload(inout, count * Lo * 8));
  hipLaunchKernelGGL(k_affine, dim3(ew_grid(count * ((size_t)nwords + 1))), dim3(256), 0, ctx->stream, da.as<uint64_t>(), La, (size_t)deff_a, d_o.as<uint64_t>(), Lo, count,
                     (size_t)nwords, shift, body_add);
  HIPCHK(hipGetLastError());
  HIPCHK(d_o.download(inout, count * Lo * 8, ctx->stream));
  return 0;
}
// in [batch][C][H][W] rows -> out [batch][C][H/K][W/K] rows: window sums with floor semantics (border rows / columns dropped)
extern "C" int dctfhe_sum_pool_rows(dctfhe_ctx* ctx, const uint64_t* in, int dim_in, int deff_in, int batch, int C, int H, int W, int K, int dim_o, uint64_t* out) {
  if (!ctx || !in || !out) return fail("dctfhe_sum_pool_rows: null argument");
  CHK(rows_ok("dctfhe_sum_pool_rows", dim_in, deff_in));
  if (batch < 1 || C < 1 || H < 1 || W < 1 || K < 1 || H / K < 1 || W / K < 1) return fail("dctfhe_sum_pool_rows: bad geometry");
  if (dim_o < deff_in || dim_o > (1 << 16)) return fail("dctfhe_sum_pool_rows: output rows of %d mask words cannot hold the sums (%d needed)", dim_o, deff_in);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t Li = (size_t)dim_in + 1, Lo = (size_t)dim_o + 1;
  const int Ho = H / K, Wo = W / K;
  const size_t nin = (size_t)batch * C * H * W * Li, nout = (size_t)batch * C * Ho * Wo * Lo;
  DevBuf di, d_o;
  HIPCHK(di.upload(in, nin * 8)); HIPCHK(d_o.alloc(nout * 8));
  hipLaunchKernelGGL(k_sum_pool, dim3(ew_grid(nout)), dim3(256), 0, ctx->stream, di.as<uint64_t>(), C, H, W, Li, (size_t)deff_in, K, Ho, Wo, d_o.as<uint64_t>(), Lo, nout);
  HIPCHK(hipGetLastError());
  HIPCHK(d_o.download(out, nout * 8, ctx->stream));
  return 0;
}

// key switch of the differences cts[ia[c]] - cts[ib[c]] (c < count; rows of D + 1 words, of which the first deff mask words may be
// non-zero), each shifted left by `shift` with body_add on the body: what a max pool's pairwise maxima feed their relu bootstrap
extern "C" int dctfhe_keyswitch_diff(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* cts, size_t count, const int32_t* ia,
                                     const int32_t* ib, int shift, uint64_t body_add, int deff, uint64_t* cts_small) {
  if (!ctx || !K || (count && (!cts || !ia || !ib || !cts_small))) return fail("dctfhe_keyswitch_diff: null argument");
  CHK(bound_to("dctfhe_keyswitch_diff", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_keyswitch_diff", K, tier, false, true));
  if (deff < 0 || deff > K->p.D) return fail("deff out of range");
  if (shift < 0 || shift > 63) return fail("shift out of range");
  for (size_t c = 0; c < count; c++)
    if (ia[c] < 0 || (size_t)ia[c] >= count || ib[c] < 0 || (size_t)ib[c] >= count)
      return fail("dctfhe_keyswitch_diff: index %zu (%d, %d) out of range (%zu rows)", c, ia[c], ib[c], count);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const dctfhe_tier& t = K->p.tiers[tier];
  const size_t L = (size_t)K->p.D + 1;
  DevBuf d_in, d_ia, d_ib;
  HIPCHK(d_in.upload(cts, count * L * 8));
  HIPCHK(d_ia.upload(ia, count * 4));
  HIPCHK(d_ib.upload(ib, count * 4));
  LutScratch sc;
  CHK(alloc_lut_scratch(K, count, &sc));
  KsInput in;
  in.rows = d_in.as<uint64_t>(); in.L = L; in.deff = deff; in.shift = shift; in.body_add = body_add;
  in.source = KS_DIFF; in.ia = d_ia.as<int32_t>(); in.ib = d_ib.as<int32_t>();
  CHK(dev_keyswitch(K, tier, in, count, sc, nullptr));
  HIPCHK(sc.d_small.download(cts_small, count * (size_t)(t.n + 1) * 8, ctx->stream));
  return 0;
}

// ---- the seams of a look-up site one launch at a time on host buffers (include/dctfhe.h): the bootstrap in the write-back modes that
// dev_round_lut / dev_max_pool launch it in, the key switch of a row sum, and the two streaming kernels of a split site and a max pool.
extern "C" int dctfhe_pbs_rows(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* cts_small, size_t count, const int64_t* tables, int ntab, int w,
                               const int32_t* table_idx, int hw, int nchan, size_t e_offset, uint64_t* rows_io, size_t n_rows, size_t row0, int dim_out,
                               int accumulate, uint64_t body_add) {
  if (!ctx || !K) return fail("dctfhe_pbs_rows: null handle");
  CHK(bound_to("dctfhe_pbs_rows", ctx, K->ctx, "evaluation keys"));
  if (!tables || !rows_io || (count && !cts_small)) return fail("dctfhe_pbs_rows: null argument");
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_pbs_rows", K, tier, true, false));
  if (ntab < 1 || w < 0) return fail("dctfhe_pbs_rows: need at least one table and w >= 0");
  if (hw < 1) return fail("dctfhe_pbs_rows: hw = %d elements per channel (at least 1)", hw);
  if (nchan < 1 || nchan > ntab) return fail("dctfhe_pbs_rows: %d per-channel tables of the %d given (1 <= nchan <= ntab)", nchan, ntab);
  if (row0 > n_rows || count > n_rows - row0) return fail("dctfhe_pbs_rows: rows [%zu, %zu) outside the %zu rows of the buffer", row0, row0 + count, n_rows);
  if (dim_out < 1 || dim_out > (1 << 16)) return fail("dctfhe_pbs_rows: rows of %d mask words (1 .. 2^16)", dim_out);
  const dctfhe_tier& t = K->p.tiers[tier];
  if (w > t.logN - 1) return fail("table of 2^%d entries does not fit N = 2^%d", w, t.logN);
  if (table_idx)
    for (size_t i = 0; i < count; i++)
      if (table_idx[i] < 0 || table_idx[i] >= ntab) return fail("table_idx[%zu] = %d out of range (%d tables)", i, table_idx[i], ntab);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t L = (size_t)dim_out + 1;
  DevBuf d_small, d_rows, d_tab, d_idx, d_sink;
  HIPCHK(d_small.upload(cts_small, count * (size_t)(t.n + 1) * 8));
  HIPCHK(d_rows.upload(rows_io, n_rows * L * 8));
  HIPCHK(d_tab.upload(tables, ((size_t)ntab << w) * 8));
  if (table_idx) HIPCHK(d_idx.upload(table_idx, count * 4));
  HIPCHK(d_sink.alloc(L * 8));
  PbsLut lut;
  lut.tables = d_tab.as<int64_t>(); lut.w = w; lut.idx = d_idx.as<int32_t>(); lut.hw = hw; lut.nchan = nchan; lut.e_offset = e_offset;
  PbsOut out{d_rows.as<uint64_t>() + row0 * L, L, accumulate != 0, body_add, d_sink.as<uint64_t>()};
  CHK(dev_pbs(K, tier, d_small.as<uint64_t>(), count, lut, out, nullptr));
  HIPCHK(d_rows.download(rows_io, n_rows * L * 8, ctx->stream));
  return 0;
}

// key switch of rows_a[c] + rows_b[c] (rows of dim_a + 1 and dim_b + 1 words; a word of b at or beyond dim_b counts as zero), shifted left
// by `shift`, body_add on the body: what the second look-up of a parity-split site reads (dev_round_lut); deff as dctfhe_keyswitch_prefix
extern "C" int dctfhe_keyswitch_sum(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* rows_a, int dim_a, const uint64_t* rows_b, int dim_b,
                                    size_t count, int shift, uint64_t body_add, int deff, uint64_t* cts_small) {
  if (!ctx || !K || (count && (!rows_a || !rows_b || !cts_small))) return fail("dctfhe_keyswitch_sum: null argument");
  CHK(bound_to("dctfhe_keyswitch_sum", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_keyswitch_sum", K, tier, false, true));
  if (dim_a < 1 || dim_a > K->p.D) return fail("dctfhe_keyswitch_sum: rows of %d mask words, the key has %d", dim_a, K->p.D);
  if (dim_b < 0 || dim_b > (1 << 16)) return fail("dctfhe_keyswitch_sum: second rows of %d mask words (0 .. 2^16)", dim_b);
  if (deff < 0 || deff > dim_a) return fail("deff out of range");
  if (shift < 0 || shift > 63) return fail("shift out of range");
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const dctfhe_tier& t = K->p.tiers[tier];
  const size_t La = (size_t)dim_a + 1, Lb = (size_t)dim_b + 1;
  DevBuf d_a, d_b;
  HIPCHK(d_a.upload(rows_a, count * La * 8));
  HIPCHK(d_b.upload(rows_b, count * Lb * 8));
  LutScratch sc;      // what dev_keyswitch uses of it, sized by the rows: digits of dim_a words per ciphertext
  sc.chunk = count;
  HIPCHK(sc.d_digits.alloc(count * (size_t)dim_a * t.lk));
  HIPCHK(sc.d_bodies.alloc(count * 8));
  HIPCHK(sc.d_small.alloc(count * (size_t)(t.n + 1) * 8));
  KsInput in;
  in.rows = d_a.as<uint64_t>(); in.L = La; in.deff = deff; in.shift = shift; in.body_add = body_add;
  in.source = KS_SUM; in.rows_b = d_b.as<uint64_t>(); in.Lb = Lb;
  CHK(dev_keyswitch(K, tier, in, count, sc, nullptr));
  HIPCHK(sc.d_small.download(cts_small, count * (size_t)(t.n + 1) * 8, ctx->stream));
  return 0;
}

// o += b on the first nwords mask words and the body (k_acc_rows): the sum of the two look-ups of a parity-split site
extern "C" int dctfhe_acc_rows(dctfhe_ctx* ctx, uint64_t* o_io, int dim_o, const uint64_t* b, int dim_b, size_t count, int nwords) {
  if (!ctx || !o_io || !b) return fail("dctfhe_acc_rows: null argument");
  if (dim_o < 0 || dim_o > (1 << 16) || dim_b < 0 || dim_b > (1 << 16)) return fail("dctfhe_acc_rows: rows of %d and %d mask words (0 .. 2^16)", dim_o, dim_b);
  if (nwords < 0 || nwords > std::min(dim_o, dim_b)) return fail("dctfhe_acc_rows: %d words do not fit rows of %d and %d mask words", nwords, dim_o, dim_b);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t Lo = (size_t)dim_o + 1, Lb = (size_t)dim_b + 1;
  DevBuf d_o, d_b;
  HIPCHK(d_o.upload(o_io, count * Lo * 8)); HIPCHK(d_b.upload(b, count * Lb * 8));
  hipLaunchKernelGGL(k_acc_rows, dim3(ew_grid(count * ((size_t)nwords + 1))), dim3(256), 0, ctx->stream, d_o.as<uint64_t>(), Lo, d_b.as<uint64_t>(), Lb, count,
                     (size_t)nwords);
  HIPCHK(hipGetLastError());
  HIPCHK(d_o.download(o_io, count * Lo * 8, ctx->stream));
  return 0;
}

// dst[r] = src[map[r]] at another row stride (k_pool_gather, one tree level of a max pool): mask words from deff_s on are written as zeros
extern "C" int dctfhe_gather_rows(dctfhe_ctx* ctx, const uint64_t* src, int dim_s, int deff_s, size_t n_src, const int32_t* map, size_t count, int dim_d,
                                  uint64_t* dst) {
  if (!ctx || !src || (count && (!map || !dst))) return fail("dctfhe_gather_rows: null argument");
  CHK(rows_ok("dctfhe_gather_rows", dim_s, deff_s));
  if (dim_d < deff_s || dim_d > (1 << 16)) return fail("dctfhe_gather_rows: output rows of %d mask words cannot hold the source's %d", dim_d, deff_s);
  if (n_src < 1 || n_src > (size_t)INT32_MAX) return fail("dctfhe_gather_rows: %zu source rows (1 .. 2^31 - 1)", n_src);
  for (size_t r = 0; r < count; r++)
    if (map[r] < 0 || (size_t)map[r] >= n_src) return fail("dctfhe_gather_rows: map[%zu] = %d out of range (%zu source rows)", r, map[r], n_src);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t Ls = (size_t)dim_s + 1, Ld = (size_t)dim_d + 1;
  DevBuf d_s, d_m, d_d;
  HIPCHK(d_s.upload(src, n_src * Ls * 8)); HIPCHK(d_m.upload(map, count * 4)); HIPCHK(d_d.alloc(count * Ld * 8));
  hipLaunchKernelGGL(k_pool_gather, dim3(ew_grid(count * Ld)), dim3(256), 0, ctx->stream, d_s.as<uint64_t>(), Ls, (size_t)deff_s, d_m.as<int32_t>(), d_d.as<uint64_t>(), Ld,
                     count);
  HIPCHK(hipGetLastError());
  HIPCHK(d_d.download(dst, count * Ld * 8, ctx->stream));
  return 0;
}

// MaxPool2d(k, s, p) on [batch][C][H][W] rows -> [batch][C][Ho][Wo] rows of dim_o + 1 words, with the session's tree (dev_max_pool).
// Inputs hold value * 2^(63 - p_d) (shift 0, signed body offset 2^62 on the differences); table: the 2^p_d entries of relu on the signed
// differences, at the same encoding.  keys == NULL: the clear form on one word per element (dim_in, deff_in, dim_o ignored; table unused).
extern "C" int dctfhe_max_pool_rows(dctfhe_ctx* ctx, dctfhe_eval_keys* K, int tier, const uint64_t* in, int dim_in, int deff_in, int batch, int C,
                                    int H, int W, int k, int s, int p, int p_d, const int64_t* table, int dim_o, uint64_t* out) {
  if (!ctx || !in || !out) return fail("dctfhe_max_pool_rows: null argument");
  if (K) CHK(bound_to("dctfhe_max_pool_rows", ctx, K->ctx, "evaluation keys"));
  if (batch < 1 || C < 1 || H < 1 || W < 1 || k < 1 || k > 32 || s < 1 || p < 0 || 2 * p > k || H + 2 * p < k || W + 2 * p < k)
    return fail("dctfhe_max_pool_rows: bad geometry (1 <= k <= 32, s >= 1, 0 <= p <= k/2, window inside the padded input)");
  if (p_d < 2 || p_d > 16) return fail("dctfhe_max_pool_rows: p_d %d out of range", p_d);
  const int Ho = pool_out_size(H, k, s, p), Wo = pool_out_size(W, k, s, p);
  const size_t nin = (size_t)batch * C * H * W, nout = (size_t)batch * C * Ho * Wo;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (!K) {
    DevBuf di, dm, d_o;
    HIPCHK(di.upload(in, nin * 8)); HIPCHK(dm.alloc((size_t)batch * C * H * Wo * 8)); HIPCHK(d_o.alloc(nout * 8));
    CHK(clear_max_pool(st, di.as<uint64_t>(), dm.as<uint64_t>(), d_o.as<uint64_t>(), batch, C, H, W, k, s, p, 0, 1ULL << 62, p_d, nullptr, 0.0, 0, 0, 0,
                          (size_t)batch * C * H * Wo, 0, nout));
    HIPCHK(d_o.download(out, nout * 8, st));
    return 0;
  }
  if (!table) return fail("dctfhe_max_pool_rows: null table");
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_max_pool_rows", K, tier, true, true));
  const dctfhe_tier& t = K->p.tiers[tier];
  if (p_d > t.logN - 1) return fail("dctfhe_max_pool_rows: table of 2^%d entries does not fit tier %d", p_d, tier);
  CHK(rows_ok("dctfhe_max_pool_rows", dim_in, deff_in));
  if (dim_in > K->p.D) return fail("dctfhe_max_pool_rows: rows of %d mask words, the key has %d", dim_in, K->p.D);
  const int ring = t.k << t.logN, dout = std::max(deff_in, ring);
  if (dim_o < dout || dim_o > K->p.D) return fail("dctfhe_max_pool_rows: output rows of %d mask words cannot hold the maxima (%d needed, at most D)", dim_o, dout);
  if (!ks_narrows(K, tier, deff_in) || !ks_narrows(K, tier, dout)) {
    if (dim_in != K->p.D || dim_o != K->p.D) return fail("dctfhe_max_pool_rows: this tier's key switch needs full-width rows (dim_in = dim_o = D)");
  }
  const size_t Li = (size_t)dim_in + 1, Lo = (size_t)dim_o + 1;
  PoolPlan P;
  CHK(pool_plan(batch, C, H, W, k, s, p, nullptr, &P));
  DevBuf di, d_o, ba, bb, d_tab;
  HIPCHK(di.upload(in, nin * Li * 8)); HIPCHK(d_o.alloc(nout * Lo * 8));
  HIPCHK(ba.alloc(P.rows_buf[0] * Lo * 8)); HIPCHK(bb.alloc(P.rows_buf[1] * Lo * 8));
  HIPCHK(d_tab.upload(table, ((size_t)1 << p_d) * 8));
  LutScratch sc;
  CHK(alloc_lut_scratch(K, std::min<size_t>(std::max<size_t>(P.pairs_per_batch, 1), 4096), &sc));
  uint64_t* const bufs[2] = {ba.as<uint64_t>(), bb.as<uint64_t>()};
  const PoolSite site{k, s, p, 0, tier, p_d, deff_in, 1ULL << 62};
  CHK(dev_max_pool(K, site, P, di.as<uint64_t>(), Li, (size_t)deff_in, bufs, d_o.as<uint64_t>(), Lo, (size_t)dout, d_tab.as<int64_t>(), sc, nullptr));
  HIPCHK(d_o.download(out, nout * Lo * 8, st));
  return 0;
}

// ------------------------------------------------------------------------------------------ K10 front-end
extern "C" int dctfhe_dct_frontend(dctfhe_ctx* ctx, const uint8_t* y, const uint8_t* c1, const uint8_t* c2, int batch, int S, int Sc, int fs,
                                   const int32_t* idx_y, int ny, const int32_t* idx_c1, int n1, const int32_t* idx_c2, int n2,
                                   const float* mean, const float* stdv, int round_coeffs, float* out) {
  if (!ctx || !y || !c1 || !c2 || !mean || !stdv || !out) return fail("dctfhe_dct_frontend: null argument");
  if (batch < 1 || S < 1 || (Sc != S && 2 * Sc != S) || (fs != 4 && fs != 8)) return fail("dctfhe_dct_frontend: bad geometry (block size 4 or 8; chroma grid S or S/2)");
  if (ny < 0 || n1 < 0 || n2 < 0 || ny + n1 + n2 < 1) return fail("dctfhe_dct_frontend: no coefficients selected");
  const int32_t* idx[3] = {idx_y, idx_c1, idx_c2};
  const int n[3] = {ny, n1, n2};
  for (int p = 0; p < 3; p++)
    for (int i = 0; i < n[p]; i++)
      if (!idx[p] || idx[p][i] < 0 || idx[p][i] >= fs * fs) return fail("dctfhe_dct_frontend: coefficient index out of range");
  HIPCHK(hipSetDevice(ctx->device));
  const int C = ny + n1 + n2;
  const size_t by = (size_t)batch * S * fs * S * fs, bc = (size_t)batch * Sc * fs * Sc * fs, nout = (size_t)batch * C * S * S;
  DevBuf d_y, d_c1, d_c2, d_idx, d_ms, d_out;
  HIPCHK(d_y.upload(y, by)); HIPCHK(d_c1.upload(c1, bc)); HIPCHK(d_c2.upload(c2, bc));
  HIPCHK(d_idx.alloc((size_t)C * 4)); HIPCHK(d_ms.alloc((size_t)C * 8)); HIPCHK(d_out.alloc(nout * 4));
  dct_args a;
  a.plane[0] = d_y.as<uint8_t>(); a.plane[1] = d_c1.as<uint8_t>(); a.plane[2] = d_c2.as<uint8_t>();
  a.S = S; a.Sc = Sc; a.fs = fs; a.round_coeffs = round_coeffs; a.batch = batch;
  int off = 0;
  for (int p = 0; p < 3; p++) {
    a.n[p] = n[p];
    a.idx[p] = d_idx.as<int32_t>() + off;
    if (n[p]) HIPCHK(hipMemcpy(d_idx.as<int32_t>() + off, idx[p], (size_t)n[p] * 4, hipMemcpyHostToDevice));
    off += n[p];
  }
  HIPCHK(hipMemcpy(d_ms.p, mean, (size_t)C * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_ms.as<float>() + C, stdv, (size_t)C * 4, hipMemcpyHostToDevice));
  a.mean = d_ms.as<float>(); a.stdv = d_ms.as<float>() + C; a.out = d_out.as<float>();
  hipLaunchKernelGGL(k_dct_frontend, dim3(ew_grid(nout)), dim3(256), 0, ctx->stream, a);
  HIPCHK(hipGetLastError());
  HIPCHK(d_out.download(out, nout * 4, ctx->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------ circuit
extern "C" int dctfhe_circuit_validate(const void* blob, size_t size) {
  CircuitPlan c;
  return parse_circuit(blob, size, &c);
}

extern "C" int dctfhe_circuit_load(dctfhe_ctx* ctx, const void* blob, size_t size, dctfhe_circuit** out) {
  if (!ctx || !out) return fail("dctfhe_circuit_load: null argument");
  std::unique_ptr<dctfhe_circuit> c(new dctfhe_circuit);
  CHK(parse_circuit(blob, size, c.get()));
  HIPCHK(hipSetDevice(ctx->device));
  c->ctx = ctx; c->device = ctx->device;
  c->d_payload.resize(c->ops.size());
  c->d_split.resize(c->ops.size());
  c->conv.assign(c->ops.size(), ConvPack{});
  c->conv_w.resize(c->ops.size());
  for (size_t i = 0; i < c->ops.size(); i++) {
    SiteOp& o = c->ops[i];
    const char* payload = (const char*)blob + o.payload_off;
    if (o.payload_len > 0) HIPCHK(c->d_payload[i].upload(payload, (size_t)o.payload_len));
    if (!o.halves.empty()) {      // the half tables of a parity split (parse_circuit made them), once per circuit
      HIPCHK(c->d_split[i].upload(o.halves.data(), o.halves.size() * 8));
      std::vector<int64_t>().swap(o.halves);
    }
    if (o.type == OP_CONV) c->conv_w[i].assign((const int8_t*)payload, (const int8_t*)payload + o.payload_len);
  }
  *out = c.release();
  return 0;
}
extern "C" int dctfhe_circuit_destroy(dctfhe_circuit* c) { delete c; return 0; }
extern "C" int dctfhe_circuit_io(dctfhe_circuit* c, int64_t* n_in, int64_t* n_out) {
  *n_in = (int64_t)c->tensors[c->input_tensor].elems();
  *n_out = (int64_t)c->tensors[c->output_tensor].elems();
  return 0;
}

extern "C" int dctfhe_circuit_stats(dctfhe_circuit* c, const dctfhe_params* P, dctfhe_stats* s) { return circuit_stats(*c, *P, s); }

// ------------------------------------------------------------------------------------------ session
// 1. every tier the circuit bootstraps on exists in the keys, and its tables fit that tier's ring
static int circuit_check_tiers(const CircuitPlan& circ, const dctfhe_params& P) {
  auto lacks = [&](int t) { return t < 0 || t >= P.n_tiers; };
  for (size_t i = 0; i < circ.ops.size(); i++) {
    const SiteOp& o = circ.ops[i];
    const LutSite& L = o.lut;
    const bool pool = o.type == OP_MAXPOOL;
    if (o.type == OP_LUT) {
      if (lacks(L.tab_tier) || (L.n_steps() > 0 && lacks(L.steps.bit))) return fail("op %zu names a tier the keys lack", i);
      if (L.mode == LUT_SPLIT_QUIET && lacks(L.tier2(P))) return fail("op %zu: parity split on the quiet twin, but tier %d shares no key-switch key", i, L.tab_tier);
    }
    int err = 0;
    for_each_bootstrap(o, P, [&](int t, int bits, bool) {
      if (err) return;
      if (lacks(t)) err = fail(pool ? "op %zu names a tier the keys lack" : "op %zu names a coarse bit tier the keys lack", i);
      else if (bits > P.tiers[t].logN - 1) err = fail("op %zu: %stable of 2^%d entries does not fit tier %d", i, pool ? "max-pool " : "", bits, t);
    });
    CHK(err);
  }
  return 0;
}

// 2. the matrix-core form of the convolution weights, once per circuit and only for encrypted evaluation (clear mode runs the VALU
// kernel), in one allocation
static int session_conv_packs(dctfhe_session* s) {
  dctfhe_circuit* circ = s->circ;
  std::vector<const int8_t*> cw;
  std::vector<ConvSite> cg;
  for (size_t i = 0; i < circ->ops.size(); i++) {
    cw.push_back(circ->conv_w[i].empty() ? nullptr : circ->conv_w[i].data());
    cg.push_back(circ->ops[i].conv);
  }
  return circ->conv_slab.p ? 0 : build_conv_packs(cw, cg, &circ->conv_slab, &circ->conv);
}

// 3. row layout per tensor.  Encrypted: a tensor is stored at its effective dimension -- the compiler's `deff_in` of the consuming op
// (mask words beyond it are zero in every ciphertext of the tensor); the output of a look-up is as wide as its table tier's ring, or as
// the rounding chain that works in place on it.  75 % of a ResNet tensor used to be stored, written and streamed zeros.
// From the parameters alone (P == nullptr: clear mode, one word per element), so that dctfhe_memory_plan needs no keys.
static size_t ring_of(const dctfhe_params& P, int tier) { return (size_t)P.tiers[tier].k << P.tiers[tier].logN; }
static int round_chain_deff(const dctfhe_params& P, int src_deff, const LutSite& L) {
  int d = src_deff, left = L.n_steps();
  for_each_bootstrap(L, P, [&](int tier, int, bool) { if (left-- > 0 && tier >= 0) d = std::max(d, (int)ring_of(P, tier)); });
  return d;
}
// does the key switch of `tier` run on the matrix cores?  The rule dctfhe_eval_keys follows when it builds a key's byte-limb form
static bool tier_ks_mfma(const dctfhe_params& P, int tier) {
  const dctfhe_tier& t = P.tiers[tier];
  const size_t rows = (size_t)P.D * t.lk;
  return rows % 64 == 0 && rows <= (1u << 17) && t.betak <= 7;
}
static int plan_row_layout(const CircuitPlan& circ, const dctfhe_params* P, std::vector<size_t>* t_L, std::vector<size_t>* t_deff) {
  const int nt = (int)circ.tensors.size();
  t_L->assign(nt, 1);
  t_deff->assign(nt, 0);
  if (!P) return 0;
  const size_t D = (size_t)P->D;
  // (the matrix-core key switch walks the key in steps of 64 rows: an effective dimension it cannot take is kept at full width)
  // ... and the integer-VALU key switch (betak = 8, or a key the matrix-core tiling does not cover) walks whole rows of D words: a
  // circuit that uses such a tier keeps every tensor at full width
  bool all_mfma = true;
  for (const SiteOp& o : circ.ops)
    for_each_bootstrap(o, *P, [&](int t, int, bool) { all_mfma = all_mfma && t >= 0 && t < P->n_tiers && tier_ks_mfma(*P, t); });
  auto clampd = [&](int d) { return (size_t)((all_mfma && d > 0 && (size_t)d < D && d % 64 == 0) ? d : D); };
  std::vector<char> known(nt, 0);
  auto set = [&](int t, size_t deff, size_t width) { (*t_deff)[t] = deff; (*t_L)[t] = (all_mfma ? std::max(deff, width) : D) + 1; known[t] = 1; };
  for (const SiteOp& o : circ.ops)
    if (o.src0 == circ.input_tensor) { set(circ.input_tensor, clampd(o.deff_in), 0); break; }
  if (!known[circ.input_tensor]) set(circ.input_tensor, D, 0);
  for (size_t i = 0; i < circ.ops.size(); i++) {
    const SiteOp& o = circ.ops[i];
    if (!known[o.src0] || (o.type == OP_ADD && !known[o.src1])) return fail("op %zu reads a tensor no earlier op wrote", i);
    if (o.type == OP_LUT) {
      const LutSite& L = o.lut;
      size_t ring = ring_of(*P, L.tab_tier);
      if (L.split()) ring = std::max(ring, ring_of(*P, L.tier2(*P)));      // the sum of both look-ups: as wide as the wider ring
      if (clampd(L.deff_in) < (*t_deff)[o.src0]) return fail("op %zu: look-up compiled for effective dimension %d, its input has %zu", i, L.deff_in, (*t_deff)[o.src0]);
      const size_t chain = L.n_steps() > 0 ? (size_t)round_chain_deff(*P, (int)clampd(L.deff_in), L) : 0;
      set(o.dst, ring, chain);
    } else if (o.type == OP_MAXPOOL) {      // the relu bootstraps accumulate into the first kN words of copies of the input
      set(o.dst, std::max((*t_deff)[o.src0], ring_of(*P, o.pool.tier)), 0);
    } else if (o.type == OP_ADD) {
      set(o.dst, std::max((*t_deff)[o.src0], (*t_deff)[o.src1]), 0);
    } else {
      set(o.dst, (*t_deff)[o.src0], 0);
    }
  }
  return 0;
}

// 4. device buffers, in two passes.  The SIZING pass (plan_session, host only: no allocation, no device) walks the ops once: tensor
// liveness -- a buffer goes back to the free list after its last reader, and a freed buffer of sufficient size is reused -- plus, per op,
// a max pool's level buffers and index maps and a parity split's second work buffer, and the look-up scratch.  It lists the allocations
// in the order they are made.  The ALLOCATION pass (session_allocate) makes exactly those.
// Memory budget: slab[g] channels of ONE image of every transient tensor of slab group g exist at a time, so a
// transient tensor, the level buffers, the maps and the parity buffer of an op inside a divided group are sized for the tallest slab.
// slab[g] = the group's channel count: the undivided group, byte for byte what runs without a budget.
struct PoolCut { size_t parts = 1, part = 0; bool on = false; };      // a divided max pool of a sharded session (dctfhe_session_set_shard_pool)
struct SlabPool { int channels = 0; std::unique_ptr<PoolPlan> plan; std::vector<int32_t> maps; };
// What a max pool's tree costs: rows of level buffers A / B, int32 map entries, the largest batch of pairwise maxima of a level, and the
// clear mode's row-pass results.  Every channel of every image goes through the same tree, and a level lists its rows output by output,
// so each figure is that of ONE channel times the channels: a divided group is sized from the one-channel tree, whatever its slab
// height, and its real trees are built once, for the heights in force (plan_session with trees = true checks them against this).
struct PoolSize {
  size_t rows_buf[2] = {0, 0}, maps = 0, max_pairs = 0, mid_count = 0;
  PoolSize times(size_t c) const { PoolSize r; r.rows_buf[0] = rows_buf[0] * c; r.rows_buf[1] = rows_buf[1] * c; r.maps = maps * c; r.max_pairs = max_pairs * c; r.mid_count = mid_count * c; return r; }
  bool operator==(const PoolSize& o) const { return rows_buf[0] == o.rows_buf[0] && rows_buf[1] == o.rows_buf[1] && maps == o.maps && max_pairs == o.max_pairs && mid_count == o.mid_count; }
};
static PoolSize pool_size_of(const PoolPlan& P, size_t maps) {
  PoolSize r;
  r.rows_buf[0] = P.rows_buf[0]; r.rows_buf[1] = P.rows_buf[1]; r.maps = maps; r.mid_count = P.mid_count;
  for (const PoolLevel& l : P.lv) r.max_pairs = std::max(r.max_pairs, l.pairs);
  return r;
}
// what one descent of the planner keeps between its steps: per max pool the one-channel figures and the tree of the undivided op
struct PoolCache { std::map<int, PoolSize> unit; std::map<int, std::shared_ptr<SlabPool>> whole; };
struct SessionPlan {
  std::vector<size_t> t_L, t_deff, tensor_words;      // tensor_words: what the tensor's buffer holds (a slab of it if transient)
  std::vector<size_t> alloc_bytes;                    // the allocations, in order; [0] is the input tensor's
  std::vector<int> alloc_pool_op;                     // the max pool whose level buffer made the allocation (-1: anything else)
  std::vector<int> tensor_alloc;                      // per tensor: its allocation (-1: no op touches it)
  std::vector<std::array<int, 2>> op_alloc;           // per op: level buffers A / B of a max pool, or [0] the parity work buffer
  std::vector<std::array<std::shared_ptr<SlabPool>, 2>> pool;   // per max pool: the op's tree, or in a divided group (trees = true) a full slab's and the last, shorter slab's
  std::vector<int> slab;                              // per slab group: S
  std::vector<int> divided_group;                     // per op: its group when that group is divided, else -1
  size_t scratch_chunk = 0, bytes_buffers = 0, bytes_maps = 0, bytes_scratch = 0, bytes_flag = sizeof(int);
  size_t largest_transient = 0;                       // bytes, over the transient tensors of groups that can still be lowered
  int largest_transient_group = -1;
  size_t total() const { return bytes_buffers + bytes_maps + bytes_scratch + bytes_flag; }
};
static size_t lut_scratch_bytes(const dctfhe_params& P, size_t chunk) {
  int lkmax = 1, nmax = 1;
  for (int i = 0; i < P.n_tiers; i++) { lkmax = std::max(lkmax, P.tiers[i].lk); nmax = std::max(nmax, P.tiers[i].n); }
  return chunk * (size_t)P.D * lkmax + chunk * 8 + chunk * (size_t)(nmax + 1) * 8 + 64 * sizeof(int64_t);
}
static int plan_session(const CircuitPlan& circ, const dctfhe_params* P, int batch, const PoolCut& cut, const std::vector<int>& slab, SessionPlan* out,
                        PoolCache* cache, bool trees) {
  SessionPlan& sp = *out;
  const bool keys = P != nullptr;
  const int nt = (int)circ.tensors.size(), nops = (int)circ.ops.size();
  if (slab.size() != circ.groups.size()) return fail("memory plan: %zu slab heights for %zu slab groups", slab.size(), circ.groups.size());
  CHK(plan_row_layout(circ, P, &sp.t_L, &sp.t_deff));
  sp.slab = slab;
  sp.divided_group.assign(nops, -1);
  std::vector<int> transient(nt, 0);      // per tensor: channels of it that exist at a time (0: all, of every image)
  for (size_t g = 0; g < circ.groups.size(); g++) {
    const SlabGroup& G = circ.groups[g];
    if (slab[g] < 1 || slab[g] > G.channels) return fail("memory plan: slab height %d of a group of %d channels (ops %d .. %d)", slab[g], G.channels, G.first, G.end);
    if (slab[g] == G.channels) continue;
    for (int i = G.first; i < G.end; i++) sp.divided_group[i] = (int)g;
    for (int i = G.first; i < G.end - 1; i++) transient[circ.ops[i].dst] = slab[g];
  }
  std::vector<int> last_use(nt, -1);
  for (int i = 0; i < nops; i++) {
    const SiteOp& o = circ.ops[i];
    last_use[o.src0] = i;
    if (o.type == OP_ADD) last_use[o.src1] = i;
  }
  for (size_t g = 0; g < circ.groups.size(); g++)      // every slab of a divided group reads the convolution's source
    if (slab[g] < circ.groups[g].channels) {
      int& lu = last_use[circ.ops[circ.groups[g].first].src0];
      lu = std::max(lu, circ.groups[g].end - 1);
    }
  last_use[circ.output_tensor] = 1 << 30;
  // the input stays resident too: dctfhe_session_run may be called again without a fresh upload (bench.py does)
  last_use[circ.input_tensor] = 1 << 30;
  sp.tensor_words.assign(nt, 0);
  for (int t = 0; t < nt; t++) {
    const TensorShape& T = circ.tensors[t];
    sp.tensor_words[t] = (transient[t] ? (size_t)transient[t] * T.H * T.W : (size_t)batch * T.elems()) * sp.t_L[t];
  }
  sp.alloc_bytes.clear(); sp.alloc_pool_op.clear();
  sp.tensor_alloc.assign(nt, -1);
  sp.op_alloc.assign(nops, {-1, -1});
  sp.pool.clear(); sp.pool.resize(nops);
  std::vector<int> freelist;      // allocations
  auto get = [&](size_t words, int pool_op) {
    int best = -1;
    for (int i = 0; i < (int)freelist.size(); i++)
      if (sp.alloc_bytes[freelist[i]] >= words * 8 && (best < 0 || sp.alloc_bytes[freelist[i]] < sp.alloc_bytes[freelist[best]])) best = i;
    if (best >= 0) { const int a = freelist[best]; freelist.erase(freelist.begin() + best); return a; }
    sp.alloc_bytes.push_back(words * 8);
    sp.alloc_pool_op.push_back(pool_op);
    return (int)sp.alloc_bytes.size() - 1;
  };
  auto alloc_t = [&](int t) { if (sp.tensor_alloc[t] < 0) sp.tensor_alloc[t] = get(sp.tensor_words[t], -1); };
  alloc_t(circ.input_tensor);
  size_t maxe = 1;      // the largest batch of bootstraps: the look-up scratch's chunk
  sp.bytes_maps = 0;
  for (int i = 0; i < nops; i++) {
    const SiteOp& o = circ.ops[i];
    const TensorShape& a = circ.tensors[o.src0];
    const int g = sp.divided_group[i];
    // elements of the op's input per launch: every image's, or one slab's
    const size_t elems_in = g >= 0 ? (size_t)slab[g] * a.H * a.W : (size_t)batch * a.elems();
    // A divided group runs once per slab, so what outlives a slab must not share a buffer with what a slab rewrites: the group's last
    // destination is allocated before any of its transient tensors and level buffers exist (it cannot take one they free), and the
    // convolution's source is held to the end of the group (below).  Within a slab the ops run in circuit order, as undivided.
    if (g >= 0 && i == circ.groups[g].first) alloc_t(circ.ops[circ.groups[g].end - 1].dst);
    alloc_t(o.dst);
    if (o.type == OP_MAXPOOL) {
      // the tree's level buffers (encrypted) or the row pass's output (clear); of a divided pool, this part's; of a divided group, a slab's
      const PoolSite& S = o.pool;
      size_t words[2] = {0, 0}, range[2] = {0, 0};
      if (cut.on) CHK(dctfhe_shard_rows((size_t)batch * circ.tensors[o.dst].elems(), (int)cut.parts, (int)cut.part, &range[0], &range[1]));
      const int heights[2] = {g >= 0 ? slab[g] : a.C, g >= 0 ? a.C % slab[g] : 0};
      PoolSize size;      // of the tallest tree
      if (g < 0) {        // the whole op: its tree, built once per descent
        std::shared_ptr<SlabPool>& sl = cache->whole[i];
        if (!sl) {
          sl.reset(new SlabPool);
          sl->channels = a.C;
          sl->plan.reset(new PoolPlan);
          CHK(pool_plan_host(batch, a.C, a.H, a.W, S.k, S.stride, S.pad, cut.on ? range : nullptr, sl->plan.get(), &sl->maps));
        }
        sp.pool[i][0] = sl;
        size = pool_size_of(*sl->plan, sl->maps.size());
      } else {
        if (!cache->unit.count(i)) {
          PoolPlan one;
          std::vector<int32_t> maps;
          CHK(pool_plan_host(1, 1, a.H, a.W, S.k, S.stride, S.pad, nullptr, &one, &maps));
          cache->unit[i] = pool_size_of(one, maps.size());
        }
        size = cache->unit[i].times((size_t)heights[0]);
        if (keys) sp.bytes_maps += cache->unit[i].maps * (size_t)heights[1] * 4;      // the shorter last slab's maps (counted again below: the full slab's)
        for (int v = 0; v < 2 && trees && keys; v++) {      // (clear mode runs a slab from its element numbers: no tree)
          if (!heights[v]) continue;
          std::shared_ptr<SlabPool> sl(new SlabPool);
          sl->channels = heights[v];
          sl->plan.reset(new PoolPlan);
          CHK(pool_plan_host(1, heights[v], a.H, a.W, S.k, S.stride, S.pad, nullptr, sl->plan.get(), &sl->maps));
          if (!(pool_size_of(*sl->plan, sl->maps.size()) == cache->unit[i].times((size_t)heights[v])))
            return fail("op %d: the max-pool tree of %d channels is not %d times the one-channel tree", i, heights[v], heights[v]);
          sp.pool[i][v] = sl;
        }
      }
      if (keys) {
        sp.bytes_maps += size.maps * 4;
        for (int b = 0; b < 2; b++) words[b] = size.rows_buf[b] * sp.t_L[o.dst];
        maxe = std::max(maxe, size.max_pairs);
      } else {
        words[0] = size.mid_count;
      }
      for (int b = 0; b < 2; b++)
        if (words[b]) sp.op_alloc[i][b] = get(words[b], i);
    }
    if (o.type == OP_LUT) maxe = std::max(maxe, elems_in);
    if (o.type == OP_LUT && keys && o.lut.split()) {
      // the second work buffer of a parity-split site: the parity bootstrap's output, then the second look-up's; chunk-sized (the
      // look-up scratch's chunk is at most 16384)
      sp.op_alloc[i][0] = get(std::min<size_t>(elems_in, 16384) * sp.t_L[o.dst], -1);
    }
    for (int b : sp.op_alloc[i]) if (b >= 0) freelist.push_back(b);      // held for this op only: back to the free list after it
    auto release = [&](int t) { if (last_use[t] == i && t != o.dst && sp.tensor_alloc[t] >= 0) freelist.push_back(sp.tensor_alloc[t]); };
    release(o.src0);
    if (o.type == OP_ADD && o.src1 != o.src0) release(o.src1);
    if (g >= 0 && i == circ.groups[g].end - 1) release(circ.ops[circ.groups[g].first].src0);
  }
  sp.bytes_buffers = 0;
  for (size_t b : sp.alloc_bytes) sp.bytes_buffers += b;
  sp.scratch_chunk = std::min<size_t>(maxe, 16384);
  sp.bytes_scratch = keys ? lut_scratch_bytes(*P, sp.scratch_chunk) : 0;
  // where the next cut goes: the group with the largest transient tensor among those that can still be lowered
  sp.largest_transient = 0; sp.largest_transient_group = -1;
  for (size_t g = 0; g < circ.groups.size(); g++) {
    if (slab[g] <= 1) continue;
    for (int i = circ.groups[g].first; i < circ.groups[g].end - 1; i++) {
      const TensorShape& T = circ.tensors[circ.ops[i].dst];
      const size_t bytes = (slab[g] == circ.groups[g].channels ? (size_t)batch * T.elems() : (size_t)slab[g] * T.H * T.W) * sp.t_L[circ.ops[i].dst] * 8;
      if (bytes > sp.largest_transient) { sp.largest_transient = bytes; sp.largest_transient_group = (int)g; }
    }
  }
  return 0;
}
// The planner's choice: start undivided; while the plan exceeds the budget, lower by one channel the slab height of the group that holds the
// largest transient tensor.  budget 0: no budget, the undivided plan.  Refused when height 1 everywhere still does not fit.
static int plan_under_budget(const CircuitPlan& circ, const dctfhe_params* P, int batch, size_t budget, SessionPlan* out, size_t* undivided_bytes) {
  std::vector<int> slab;
  for (const SlabGroup& G : circ.groups) slab.push_back(G.channels);
  PoolCache cache;      // a step of the descent builds no tree: the undivided ops keep theirs, a divided group is sized from one channel
  CHK(plan_session(circ, P, batch, PoolCut{}, slab, out, &cache, false));
  if (undivided_bytes) *undivided_bytes = out->total();
  size_t smallest = out->total();
  while (budget && out->total() > budget) {
    const int g = out->largest_transient_group;
    if (g < 0) {
      int worst = 0;      // the op whose destination is the largest tensor left
      size_t big = 0;
      for (int i = 0; i < (int)circ.ops.size(); i++)
        if (out->tensor_words[circ.ops[i].dst] * 8 >= big) { big = out->tensor_words[circ.ops[i].dst] * 8; worst = i; }
      return fail("memory budget of %zu bytes: the smallest plan (down to one channel of every slab group at a time) needs %zu bytes; the largest tensor left, %zu bytes, is the destination of op %d",
                  budget, smallest, big, worst);
    }
    slab[g]--;
    CHK(plan_session(circ, P, batch, PoolCut{}, slab, out, &cache, false));
    smallest = std::min(smallest, out->total());
  }
  return 0;
}

// the allocation pass: what the plan lists, in its order.  A second plan (dctfhe_session_set_shard_pool, dctfhe_session_set_memory_budget,
// before the first run) keeps the input's buffer, the first allocation: it may be uploaded already
static int session_allocate(dctfhe_session* s, SessionPlan&& sp, bool keep_scratch) {
  const dctfhe_circuit* circ = s->circ;
  const bool keys = s->keys != nullptr;
  const int nt = (int)circ->tensors.size(), nops = (int)circ->ops.size();
  if (!s->owned.empty()) {
    if (s->owned[0].bytes != sp.alloc_bytes[0]) return fail("session plan: the input's buffer changed its size");
    s->owned.erase(s->owned.begin() + 1, s->owned.end());
  }
  s->pool.clear(); s->pool.resize(nops);
  s->pool_last.clear(); s->pool_last.resize(nops);
  keep_scratch = keep_scratch && s->lut.chunk > 0;
  if (!keep_scratch) s->lut = LutScratch{};
  for (size_t a = s->owned.size(); a < sp.alloc_bytes.size(); a++) {
    if (sp.alloc_pool_op[a] >= 0) {
      size_t fr = 0, tot = 0;
      hipMemGetInfo(&fr, &tot);
      if (sp.alloc_bytes[a] > fr)
        return fail("op %d: the max pool's level buffer needs %.1f GB, %.1f GB of device memory are free (batch %d too large for one device)", sp.alloc_pool_op[a],
                    sp.alloc_bytes[a] * 1e-9, fr * 1e-9, s->batch);
    }
    DevBuf b;
    HIPCHK(b.alloc(sp.alloc_bytes[a]));
    s->owned.push_back(std::move(b));
  }
  s->t_L = sp.t_L; s->t_deff = sp.t_deff; s->tensor_words = sp.tensor_words;
  s->d_tensor.assign(nt, nullptr);
  for (int t = 0; t < nt; t++) if (sp.tensor_alloc[t] >= 0) s->d_tensor[t] = s->owned[sp.tensor_alloc[t]].as<uint64_t>();
  s->pool_buf.assign(nops, {nullptr, nullptr});
  for (int i = 0; i < nops; i++) {
    for (int b = 0; b < 2; b++) if (sp.op_alloc[i][b] >= 0) s->pool_buf[i][b] = s->owned[sp.op_alloc[i][b]].as<uint64_t>();
    for (int v = 0; v < 2; v++) {
      if (!sp.pool[i][v] || !sp.pool[i][v]->plan) continue;
      SlabPool& sl = *sp.pool[i][v];
      if (keys) {
        HIPCHK(sl.plan->maps.alloc(sl.maps.size() * 4));
        if (!sl.maps.empty()) HIPCHK(hipMemcpy(sl.plan->maps.p, sl.maps.data(), sl.maps.size() * 4, hipMemcpyHostToDevice));
      }
      (v == 0 ? s->pool[i] : s->pool_last[i]) = std::move(sl.plan);
    }
  }
  s->slab = sp.slab; s->divided_group = sp.divided_group;
  s->planned_bytes = sp.total();
  if (!s->budget_bytes) s->undivided_bytes = sp.total();
  // 5. the look-up scratch: one chunk as large as the largest batch of bootstraps, at most 16384
  return keys && !keep_scratch ? alloc_lut_scratch(s->keys, sp.scratch_chunk, &s->lut) : 0;
}
static int session_plan_buffers(dctfhe_session* s, const std::vector<int>* slab = nullptr, bool keep_scratch = false) {
  const dctfhe_circuit* circ = s->circ;
  const dctfhe_params* P = s->keys ? &s->keys->p : nullptr;
  if (P)      // the layout follows the parameters' rule for the matrix-core key switch: the keys were built by the same one
    for (const SiteOp& o : circ->ops) {
      bool same = true;
      for_each_bootstrap(o, *P, [&](int t, int, bool) { same = same && s->keys->tiers[t].mfma() == tier_ks_mfma(*P, t); });
      if (!same) return fail("session plan: the keys' key-switch form differs from the parameters' rule");
    }
  std::vector<int> undivided;
  for (const SlabGroup& G : circ->groups) undivided.push_back(G.channels);
  SessionPlan sp;
  PoolCut cut;
  cut.on = s->shard_pool; cut.parts = (size_t)s->parts; cut.part = (size_t)s->part;
  PoolCache cache;
  CHK(plan_session(*circ, P, s->batch, cut, slab ? *slab : undivided, &sp, &cache, true));
  return session_allocate(s, std::move(sp), keep_scratch);
}

// ---- memory budget (include/dctfhe.h): the planner from a blob and parameters alone, the session's switch, its getter
static int fill_mem_plan(const CircuitPlan& circ, const SessionPlan& sp, size_t undivided, size_t budget, dctfhe_mem_plan* out) {
  if (circ.groups.size() > DCTFHE_MAX_SLAB_GROUPS) return fail("memory plan: %zu slab groups, the record holds %d", circ.groups.size(), DCTFHE_MAX_SLAB_GROUPS);
  memset(out, 0, sizeof *out);
  out->bytes_undivided = undivided; out->bytes_planned = sp.total(); out->budget_bytes = budget;
  out->bytes_buffers = sp.bytes_buffers; out->bytes_maps = sp.bytes_maps; out->bytes_scratch = sp.bytes_scratch + sp.bytes_flag;
  out->n_groups = (int)circ.groups.size();
  for (size_t g = 0; g < circ.groups.size(); g++) {
    out->first_op[g] = circ.groups[g].first; out->end_op[g] = circ.groups[g].end; out->channels[g] = circ.groups[g].channels; out->slab[g] = sp.slab[g];
  }
  return 0;
}
extern "C" int dctfhe_memory_plan(const void* blob, size_t size, const dctfhe_params* params, int batch, size_t budget_bytes, dctfhe_mem_plan* out) {
  if (!out) return fail("dctfhe_memory_plan: null argument");
  if (batch < 1) return fail("dctfhe_memory_plan: batch must be >= 1");
  CircuitPlan circ;
  CHK(parse_circuit(blob, size, &circ));
  if (params) { CHK(dctfhe_params_check(params)); CHK(circuit_check_tiers(circ, *params)); }
  SessionPlan sp;
  size_t undivided = 0;
  CHK(plan_under_budget(circ, params, batch, budget_bytes, &sp, &undivided));
  return fill_mem_plan(circ, sp, undivided, budget_bytes, out);
}
static int budget_allowed(const dctfhe_session* s, const char* who) {
  if (!s) return fail("%s: null session", who);
  if (s->has_run) return fail("%s: the session has run; set the budget before its first run", who);
  if (s->parts > 1 || s->shard_pool) return fail("%s: the session is part %d of %d of a sharded run, and a budgeted session stays unsharded", who, s->part, s->parts);
  if (s->d_audit_key.p) return fail("%s: the margin audit is on, and it runs undivided: turn it off first", who);
  return 0;
}
// re-plan a session that has not run at these slab heights, with the trees of its divided pools, and allocate.  budget: what the session
// records as its budget (nullptr: exactly the plan's bytes, 0 at the undivided heights); expect: the bytes the sizing pass promised (0:
// none).  A refusal here has touched nothing.
static int session_replan(dctfhe_session* s, const char* who, const std::vector<int>& heights, size_t undivided, const size_t* budget, size_t expect) {
  HIPCHK(hipSetDevice(s->ctx->device));
  SessionPlan sp;
  PoolCache cache;
  CHK(plan_session(*s->circ, s->keys ? &s->keys->p : nullptr, s->batch, PoolCut{}, heights, &sp, &cache, true));
  if (expect && sp.total() != expect) return fail("%s: the plan with its trees needs %zu bytes, the sizing pass said %zu", who, sp.total(), expect);
  s->undivided_bytes = undivided;
  s->budget_bytes = budget ? *budget : heights == s->circ_heights() ? 0 : sp.total();
  return session_allocate(s, std::move(sp), false);
}
// the plan at slab heights given by hand, one per slab group: what the planner would pick under SOME budget is its business; this is how a
// test or an experiment runs a group at a height of its choosing.  It counts as a budget of exactly the plan's bytes.
extern "C" int dctfhe_session_set_slab_heights(dctfhe_session* s, const int32_t* slab, int n_groups) {
  CHK(budget_allowed(s, "dctfhe_session_set_slab_heights"));
  if (!slab || n_groups != (int)s->circ->groups.size()) return fail("dctfhe_session_set_slab_heights: %d heights for a circuit of %zu slab groups", n_groups, s->circ->groups.size());
  SessionPlan whole;
  PoolCache cache;
  CHK(plan_session(*s->circ, s->keys ? &s->keys->p : nullptr, s->batch, PoolCut{}, s->circ_heights(), &whole, &cache, false));
  return session_replan(s, "dctfhe_session_set_slab_heights", std::vector<int>(slab, slab + n_groups), whole.total(), nullptr, 0);
}
extern "C" int dctfhe_session_set_memory_budget(dctfhe_session* s, size_t bytes) {
  CHK(budget_allowed(s, "dctfhe_session_set_memory_budget"));
  SessionPlan sp;
  size_t undivided = 0;
  CHK(plan_under_budget(*s->circ, s->keys ? &s->keys->p : nullptr, s->batch, bytes, &sp, &undivided));      // refused: nothing was touched
  return session_replan(s, "dctfhe_session_set_memory_budget", sp.slab, undivided, &bytes, sp.total());
}
extern "C" int dctfhe_session_memory_plan(dctfhe_session* s, dctfhe_mem_plan* out) {
  if (!s || !out) return fail("dctfhe_session_memory_plan: null argument");
  SessionPlan sp;      // the heights in force; the byte figures are the session's own
  sp.slab = s->slab;
  CHK(fill_mem_plan(*s->circ, sp, s->undivided_bytes, s->budget_bytes, out));
  out->bytes_planned = s->planned_bytes;
  out->bytes_buffers = out->bytes_maps = out->bytes_scratch = 0;
  return 0;
}

extern "C" int dctfhe_session_create(dctfhe_ctx* ctx, dctfhe_circuit* circ, dctfhe_keys* keys, int batch, dctfhe_session** out) {
  if (!ctx || !circ || !out) return fail("dctfhe_session_create: null argument");
  if (batch < 1) return fail("batch must be >= 1");
  if (keys) CHK(bound_to("dctfhe_session_create", ctx, keys->ctx, "evaluation keys"));
  if (circ->device != ctx->device) return fail("dctfhe_session_create: the circuit was loaded on device %d, the context runs on device %d", circ->device, ctx->device);
  HIPCHK(hipSetDevice(ctx->device));
  std::unique_ptr<dctfhe_session> s(new dctfhe_session);
  s->ctx = ctx; s->circ = circ; s->keys = keys; s->batch = batch;
  s->D = keys ? keys->p.D : 0;
  if (keys) CHK(circuit_check_tiers(*circ, keys->p));
  if (keys) {      // every key the circuit reads is held: the first missing tier, and an op that needs it
    CircuitKeyUse u;
    circuit_key_use(*circ, keys->p, &u);
    for (int ti = 0; ti < keys->p.n_tiers; ti++) {
      if (has_bsk(u.sel, ti) && !has_bsk(keys->sel, ti))
        return fail("dctfhe_session_create: op %d bootstraps on tier %d, and the evaluation keys hold no bootstrap key of tier %d (tier selection bsk 0x%x, ksk 0x%x; the circuit needs bsk 0x%x, ksk 0x%x)",
                    u.bsk_op[ti], ti, ti, keys->sel.bsk, keys->sel.ksk, u.sel.bsk, u.sel.ksk);
      if (has_ksk(u.sel, ti) && !has_ksk(keys->sel, ti))
        return fail("dctfhe_session_create: op %d key-switches with tier %d, and the evaluation keys hold no key-switch key of tier %d (tier selection bsk 0x%x, ksk 0x%x; the circuit needs bsk 0x%x, ksk 0x%x)",
                    u.ksk_op[ti], ti, ti, keys->sel.bsk, keys->sel.ksk, u.sel.bsk, u.sel.ksk);
    }
  }
  if (keys) CHK(session_conv_packs(s.get()));
  CHK(session_plan_buffers(s.get()));
  HIPCHK(s->d_overflow.alloc(sizeof(int)));
  HIPCHK(hipMemsetAsync(s->d_overflow.p, 0, sizeof(int), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));      // the first run may come on another stream (dctfhe_ctx_set_stream)
  s->whole.assign(circ->tensors.size(), 1);
  s->marked.assign(circ->tensors.size(), {});
  s->pool_pairs_run.assign(circ->ops.size(), 0);
  if (keys) {
    dctfhe_stats stt;
    circuit_stats(*circ, keys->p, &stt);
    for (int i = 0; i < DCTFHE_MAX_TIERS; i++) s->pbs_per_image[i] = stt.pbs_count[i];
  }
  *out = s.release();
  return 0;
}

extern "C" int dctfhe_session_destroy(dctfhe_session* s) { delete s; return 0; }

// host rows of `dim` mask words + body (dim = D: the full-width form; smaller: the compact wire form of dctfhe_encrypt_rows)
extern "C" int dctfhe_session_upload_rows(dctfhe_session* s, const uint64_t* cts_in, int dim) {
  if (!s || !cts_in) return fail("dctfhe_session_upload: null argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  const int t = s->circ->input_tensor;
  hipStream_t st = s->ctx->stream;
  if (!s->keys) {      // clear mode: one word per element, stored as given
    HIPCHK(hipMemcpyAsync(s->d_tensor[t], cts_in, s->tensor_words[t] * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    s->whole[t] = 1;
    return 0;
  }
  if (dim < 1 || dim > s->D) return fail("dctfhe_session_upload: rows of %d mask words, the key has %d", dim, s->D);
  // the tensor is stored at its effective dimension.  The circuit was compiled for inputs that are zero beyond it (client
  // encryption on a key prefix, dctfhe_params.input_dim): the key switch and the convolutions never look at that tail, so make
  // sure it really is empty before dropping it
  const size_t Lh = (size_t)dim + 1, Ls = s->t_L[t], deff = s->t_deff[t];
  const size_t count = s->tensor_words[t] / Ls;
  DevBuf tmp;
  HIPCHK(tmp.alloc(count * Lh * 8));
  HIPCHK(hipMemcpyAsync(tmp.p, cts_in, count * Lh * 8, hipMemcpyHostToDevice, st));
  if (deff < (size_t)dim) {
    HIPCHK(hipMemsetAsync(s->d_overflow.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_tail_nonzero, dim3(ew_grid(count * ((size_t)dim - deff))), dim3(256), 0, st, tmp.as<uint64_t>(), count, dim, (int)deff, s->d_overflow.as<int>());
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, s->d_overflow.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return fail("input ciphertexts have non-zero mask words beyond %zu: encrypt them with these parameters (input_dim)", deff);
  }
  hipLaunchKernelGGL(k_restride, dim3(ew_grid(count * Ls)), dim3(256), 0, st, tmp.as<uint64_t>(), Lh, s->d_tensor[t], Ls, count, std::min(deff, (size_t)dim));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  s->whole[t] = 1;
  return 0;
}
// seeded inputs: only the bodies cross PCIe (8 bytes per ciphertext); the masks are written straight into the input tensor
extern "C" int dctfhe_session_upload_seeded(dctfhe_session* s, const uint8_t* mask_key, uint64_t stream, int dim_eff, const uint64_t* bodies,
                                            size_t count) {
  if (!s || !mask_key || !bodies) return fail("dctfhe_session_upload_seeded: null argument");
  if (!s->keys) return fail("dctfhe_session_upload_seeded: a clear-mode session takes phases (dctfhe_session_upload), not ciphertexts");
  HIPCHK(hipSetDevice(s->ctx->device));
  const int t = s->circ->input_tensor;
  hipStream_t st = s->ctx->stream;
  const size_t Ls = s->t_L[t], deff = s->t_deff[t], n = s->tensor_words[t] / Ls;
  if (count != n) return fail("dctfhe_session_upload_seeded: %zu ciphertexts, the session takes batch x n_in = %zu", count, n);
  // the same rule as upload_rows' tail check: the circuit reads only the first deff mask words
  if (dim_eff < 1 || (size_t)dim_eff > deff) return fail("dctfhe_session_upload_seeded: %d mask words per input; this circuit's input keeps %zu", dim_eff, deff);
  DevBuf d_b;
  HIPCHK(d_b.alloc(count * 8));
  HIPCHK(hipMemcpyAsync(d_b.p, bodies, count * 8, hipMemcpyHostToDevice, st));
  CHK(launch_expand(key_from_bytes(mask_key), stream, 0, (uint64_t)s->D + 1, dim_eff, ~0ULL, d_b.as<uint64_t>(), 1, count, Ls, s->d_tensor[t], st));
  HIPCHK(hipStreamSynchronize(st));
  s->whole[t] = 1;
  return 0;
}
// public-key inputs: the wire words cross PCIe (16 bytes per input in full groups), k_pk_extract writes the rows straight into the input tensor
extern "C" int dctfhe_session_upload_public(dctfhe_session* s, int logN, const uint64_t* words, size_t count) {
  if (!s || !words) return fail("dctfhe_session_upload_public: null argument");
  if (!s->keys) return fail("dctfhe_session_upload_public: a clear-mode session takes phases (dctfhe_session_upload), not ciphertexts");
  if (logN < 5 || logN > 12) return fail("dctfhe_session_upload_public: ring 2^%d outside 2^5 .. 2^12", logN);
  const int t = s->circ->input_tensor;
  const size_t Ls = s->t_L[t], deff = s->t_deff[t], n = s->tensor_words[t] / Ls;
  if (count == 0) return fail("dctfhe_session_upload_public: no inputs (count == 0)");
  if (count != n) return fail("dctfhe_session_upload_public: %zu inputs, the session takes batch x n_in = %zu", count, n);
  // the rule of upload_seeded: the circuit reads only the first deff mask words (and Ls > deff holds them and the body)
  if (((size_t)1 << logN) > deff) return fail("dctfhe_session_upload_public: a slot fills N_e = %d mask words; this circuit's input keeps %zu", 1 << logN, deff);
  HIPCHK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  const size_t nwords = dctfhe_ring_words(logN, count);
  DevBuf d_w;
  HIPCHK(d_w.alloc(nwords * 8));
  HIPCHK(hipMemcpyAsync(d_w.p, words, nwords * 8, hipMemcpyHostToDevice, st));
  CHK(launch_ring_extract(logN, d_w.as<uint64_t>(), count, Ls, s->d_tensor[t], st));
  HIPCHK(hipStreamSynchronize(st));
  s->whole[t] = 1;
  return 0;
}
extern "C" int dctfhe_session_upload(dctfhe_session* s, const uint64_t* cts_in) {
  if (!s) return fail("dctfhe_session_upload: null argument");
  return dctfhe_session_upload_rows(s, cts_in, s->D);
}
// mask words a compact row of the session's input / output needs (what upload_rows / download_rows accept as `dim` at least / at most
// usefully); clear-mode sessions report 0
extern "C" int dctfhe_session_dims(dctfhe_session* s, int* in_dim, int* out_dim) {
  if (!s || !in_dim || !out_dim) return fail("dctfhe_session_dims: null argument");
  *in_dim = s->keys ? (int)s->t_deff[s->circ->input_tensor] : 0;
  *out_dim = s->keys ? (int)s->t_deff[s->circ->output_tensor] : 0;
  return 0;
}
extern "C" int dctfhe_session_set_noise(dctfhe_session* s, uint64_t seed, const double* sigma_per_op, int n_ops) {
  if (s->keys) return fail("noise simulation is a clear-mode feature: create the session without keys");
  if (n_ops != 0 && n_ops != (int)s->circ->ops.size()) return fail("expected one sigma per op (%zu), got %d", s->circ->ops.size(), n_ops);
  s->sim_sigma.assign(sigma_per_op, sigma_per_op + n_ops);
  s->sim_seed = seed;
  return 0;
}

extern "C" int dctfhe_session_set_noise_split(dctfhe_session* s, const double* sigma2_per_op, int n_ops) {
  if (!s) return fail("dctfhe_session_set_noise_split: null session");
  if (s->keys) return fail("noise simulation is a clear-mode feature: create the session without keys");
  if (n_ops != 0 && n_ops != (int)s->circ->ops.size()) return fail("expected one sigma per op (%zu), got %d", s->circ->ops.size(), n_ops);
  s->sim_sigma2.assign(sigma2_per_op, sigma2_per_op + n_ops);
  return 0;
}

// a sharded session: every download reads the whole output tensor
static int output_whole(const dctfhe_session* s, const char* who) {
  const int t = s->circ->output_tensor;
  if (!s->whole[t])
    return fail("%s: output tensor %d holds only the rows of part %d of %d: exchange the other parts' rows and call dctfhe_session_mark_whole first", who, t, s->part,
                s->parts);
  return 0;
}
extern "C" int dctfhe_session_download_rows(dctfhe_session* s, uint64_t* cts_out, int dim) {
  if (!s || !cts_out) return fail("dctfhe_session_download: null argument");
  CHK(output_whole(s, "dctfhe_session_download"));
  HIPCHK(hipSetDevice(s->ctx->device));
  const int t = s->circ->output_tensor;
  hipStream_t st = s->ctx->stream;
  if (!s->keys) {
    HIPCHK(hipMemcpyAsync(cts_out, s->d_tensor[t], s->tensor_words[t] * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  if (dim < (int)s->t_deff[t] || dim > s->D) return fail("dctfhe_session_download: rows of %d mask words; the output needs %zu and the key has %d", dim, s->t_deff[t], s->D);
  const size_t Lh = (size_t)dim + 1, Ls = s->t_L[t];
  const size_t count = s->tensor_words[t] / Ls;
  DevBuf tmp;      // to host rows of dim + 1 words, zero beyond the effective dimension
  HIPCHK(tmp.alloc(count * Lh * 8));
  hipLaunchKernelGGL(k_restride, dim3(ew_grid(count * Lh)), dim3(256), 0, st, s->d_tensor[t], Ls, tmp.as<uint64_t>(), Lh, count, s->t_deff[t]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(cts_out, tmp.p, count * Lh * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int dctfhe_session_download(dctfhe_session* s, uint64_t* cts_out) {
  if (!s) return fail("dctfhe_session_download: null argument");
  return dctfhe_session_download_rows(s, cts_out, s->D);
}
// the outputs as packed rows: key-switched to `tier` straight from the output tensor (its stored stride and effective dimension) with the
// session's look-up scratch, at download time -- dctfhe_session_run and its timing do not know about it
extern "C" int dctfhe_session_download_packed(dctfhe_session* s, int tier, uint16_t* rows) {
  if (!s || !rows) return fail("dctfhe_session_download_packed: null argument");
  if (!s->keys) return fail("dctfhe_session_download_packed: a clear-mode session holds phases, not ciphertexts (dctfhe_session_download)");
  if (tier < 0 || tier >= s->keys->p.n_tiers) return fail("dctfhe_session_download_packed: tier %d out of range (%d tiers)", tier, s->keys->p.n_tiers);
  CHK(keys_hold("dctfhe_session_download_packed", s->keys, tier, false, true));
  CHK(output_whole(s, "dctfhe_session_download_packed"));
  HIPCHK(hipSetDevice(s->ctx->device));
  const int t = s->circ->output_tensor;
  const size_t Ls = s->t_L[t];
  return dev_keyswitch_pack(s->keys, tier, s->d_tensor[t], Ls, (int)s->t_deff[t], s->tensor_words[t] / Ls, s->lut, rows);
}
// the outputs ring-packed: key-switched to `tier` chunk by chunk like the packed rows above, collected as small ciphertexts on the device,
// then packed group by group with the client's packing key -- at download time, outside dctfhe_session_run and its timing
extern "C" int dctfhe_session_download_ring(dctfhe_session* s, int tier, dctfhe_pack_key* K, uint16_t* out) {
  if (!s || !K || !out) return fail("dctfhe_session_download_ring: null argument");
  if (!s->keys) return fail("dctfhe_session_download_ring: a clear-mode session holds phases, not ciphertexts (dctfhe_session_download)");
  if (K->ctx != s->ctx || s->keys->ctx != s->ctx) return fail("dctfhe_session_download_ring: session, evaluation keys and packing key must share one context");
  if (tier < 0 || tier >= s->keys->p.n_tiers) return fail("dctfhe_session_download_ring: tier %d out of range (%d tiers)", tier, s->keys->p.n_tiers);
  CHK(keys_hold("dctfhe_session_download_ring", s->keys, tier, false, true));
  const int n = s->keys->p.tiers[tier].n;
  if (n > K->n_max) return fail("dctfhe_session_download_ring: tier %d has n = %d, the packing key covers n_max = %d", tier, n, K->n_max);
  if ((1 << K->logN) > s->keys->p.D) return fail("dctfhe_session_download_ring: the ring key is a prefix of the big key: N_p = %d > D = %d", 1 << K->logN, s->keys->p.D);
  CHK(output_whole(s, "dctfhe_session_download_ring"));
  HIPCHK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  const int t = s->circ->output_tensor;
  const size_t Ls = s->t_L[t], count = s->tensor_words[t] / Ls, n1 = (size_t)n + 1;
  DevBuf d_small;
  HIPCHK(d_small.alloc(count * n1 * 8));
  for (size_t c0 = 0; c0 < count; c0 += s->lut.chunk) {
    const size_t cn = std::min(s->lut.chunk, count - c0);
    KsInput in;
    in.rows = s->d_tensor[t] + c0 * Ls; in.L = Ls; in.deff = (int)s->t_deff[t];
    CHK(dev_keyswitch(s->keys, tier, in, cn, s->lut, nullptr));
    HIPCHK(hipMemcpyAsync(d_small.as<uint64_t>() + c0 * n1, s->lut.small(), cn * n1 * 8, hipMemcpyDeviceToDevice, st));
  }
  return dev_ring_pack(K, d_small.as<uint64_t>(), count, n, out);
}

// ---- margin audit (include/dctfhe.h): the slots are those of for_each_bootstrap, the kernel k_margin_probe
static_assert(sizeof(margin_slot) == sizeof(dctfhe_margin_stats) && offsetof(margin_slot, max_abs) == offsetof(dctfhe_margin_stats, max_abs) &&
              offsetof(margin_slot, count) == offsetof(dctfhe_margin_stats, count) && offsetof(margin_slot, sum_sq) == offsetof(dctfhe_margin_stats, sum_sq) &&
              offsetof(margin_slot, hist) == offsetof(dctfhe_margin_stats, hist) && DCTFHE_MARGIN_BINS == 16, "k_margin_probe accumulates into dctfhe_margin_stats");
static dctfhe_margin_stats margin_header(int op, int entry, int tier, int logN, int w) {
  dctfhe_margin_stats m;
  memset(&m, 0, sizeof m);
  m.op = op; m.entry = entry; m.tier = tier; m.table_bits = w; m.half_box = 1 << (logN - w - 1);
  return m;
}
// the run's accumulated fields under the slots' fixed ones
static int session_audit_collect(dctfhe_session* s) {
  s->audit_last = s->audit_slots;
  if (s->audit_slots.empty()) return 0;
  std::vector<dctfhe_margin_stats> dev(s->audit_slots.size());
  HIPCHK(hipMemcpy(dev.data(), s->d_audit.p, dev.size() * sizeof(dctfhe_margin_stats), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < dev.size(); i++) {
    dctfhe_margin_stats& m = s->audit_last[i];
    m.max_abs = dev[i].max_abs; m.count = dev[i].count; m.sum = dev[i].sum; m.sum_sq = dev[i].sum_sq;
    memcpy(m.hist, dev[i].hist, sizeof m.hist);
  }
  return 0;
}
extern "C" int dctfhe_session_set_audit(dctfhe_session* s, dctfhe_client_key* C) {
  if (!s) return fail("dctfhe_session_set_audit: null session");
  HIPCHK(hipSetDevice(s->ctx->device));
  if (!C) { s->audit_off(); return 0; }
  if (!s->keys) return fail("dctfhe_session_set_audit: a clear-mode session holds phases, not ciphertexts: there is no decision noise to measure");
  if (s->parts > 1) return fail("dctfhe_session_set_audit: this session is part %d of %d; the margin audit stays unsharded", s->part, s->parts);
  if (s->budget_bytes) return fail("dctfhe_session_set_audit: the session has a memory budget (%zu bytes); the margin audit runs undivided", s->budget_bytes);
  const dctfhe_params &P = s->keys->p, &Q = C->p;
  CHK(bound_to("dctfhe_session_set_audit", s->ctx, C->ctx, "client key"));
  if (P.D != Q.D || P.n_max != Q.n_max || P.n_tiers != Q.n_tiers)
    return fail("dctfhe_session_set_audit: the client key (D = %d, n_max = %d, %d tiers) is of another parameter set than the session's keys (D = %d, n_max = %d, %d tiers)",
                Q.D, Q.n_max, Q.n_tiers, P.D, P.n_max, P.n_tiers);
  for (int t = 0; t < P.n_tiers; t++)
    if (P.tiers[t].n != Q.tiers[t].n || P.tiers[t].k != Q.tiers[t].k || P.tiers[t].logN != Q.tiers[t].logN)
      return fail("dctfhe_session_set_audit: tier %d of the client key (n = %d, k = %d, logN = %d) differs from the session's (n = %d, k = %d, logN = %d)", t,
                  Q.tiers[t].n, Q.tiers[t].k, Q.tiers[t].logN, P.tiers[t].n, P.tiers[t].k, P.tiers[t].logN);
  std::vector<dctfhe_margin_stats> slots;
  std::vector<int> first;
  for (size_t i = 0; i < s->circ->ops.size(); i++) {
    const SiteOp& o = s->circ->ops[i];
    if (o.type == OP_LUT && o.lut.approx())
      return fail("dctfhe_session_set_audit: op %zu rounds approximately: the low bits ride along into its look-up, the distance from the box centre is not noise", i);
    first.push_back((int)slots.size());
    int entry = 0, err = 0;
    for_each_bootstrap(o, P, [&](int tier, int bits, bool own_ks) {
      if (!own_ks || err) return;
      if (P.tiers[tier].logN - bits < 1) { err = fail("dctfhe_session_set_audit: op %zu: a table of %d input bits leaves no box on tier %d", i, bits, tier); return; }
      slots.push_back(margin_header((int)i, entry++, tier, P.tiers[tier].logN, bits));
    });
    CHK(err);
  }
  s->audit_off();
  // the new key copy and slot array are built in locals and enter the session together: a step that fails leaves the audit off.  The
  // key is copied last, so that no error path frees a copy of the secret unwiped
  DevBuf key, slot;
  HIPCHK(key.alloc((size_t)P.n_max));
  HIPCHK(slot.alloc(std::max<size_t>(1, slots.size()) * sizeof(margin_slot)));
  hipStream_t st = s->ctx->stream;
  HIPCHK(hipMemsetAsync(slot.p, 0, slot.bytes, st));
  hipError_t e = hipMemcpyAsync(key.p, C->s(), key.bytes, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    hipMemsetAsync(key.p, 0, key.bytes, st);
    hipStreamSynchronize(st);
    return fail("dctfhe_session_set_audit: copy of the small key -> %s", hipGetErrorString(e));
  }
  s->d_audit_key = std::move(key); s->d_audit = std::move(slot);
  s->audit_slots = slots; s->audit_last = slots; s->audit_first = first;
  return 0;
}
extern "C" int dctfhe_session_audit(dctfhe_session* s, dctfhe_margin_stats* out, int capacity, int* n_slots) {
  if (!s || !n_slots) return fail("dctfhe_session_audit: null argument");
  const int n = s->d_audit_key.p ? (int)s->audit_last.size() : 0;
  *n_slots = n;
  if (!out) return 0;
  if (capacity < n) return fail("dctfhe_session_audit: room for %d slots, the circuit has %d", capacity, n);
  if (n) memcpy(out, s->audit_last.data(), (size_t)n * sizeof(dctfhe_margin_stats));
  return 0;
}

// ---- sharded look-up sites (include/dctfhe.h): the partition rule, the exchange plan, and what moves rows between the parts
extern "C" int dctfhe_shard_rows(size_t rows, int parts, int part, size_t* first, size_t* count) {
  if (!first || !count) return fail("dctfhe_shard_rows: null argument");
  if (parts < 1 || parts > 64) return fail("dctfhe_shard_rows: %d parts (1 .. 64)", parts);
  if (part < 0 || part >= parts) return fail("dctfhe_shard_rows: part %d of %d", part, parts);
  const size_t q = rows / (size_t)parts, r = rows % (size_t)parts, p = (size_t)part;
  *first = p * q + std::min(p, r);
  *count = q + (p < r ? 1 : 0);
  return 0;
}
static bool op_runs_sliced(const SiteOp& o) { return o.type == OP_LUT || o.type == OP_ADD; }
extern "C" int dctfhe_session_set_shard(dctfhe_session* s, int part, int parts) {
  if (!s) return fail("dctfhe_session_set_shard: null session");
  size_t f, n;
  CHK(dctfhe_shard_rows(0, parts, part, &f, &n));
  if (s->has_run) return fail("dctfhe_session_set_shard: the session has run; shard it before its first run");
  if (s->d_audit_key.p && parts > 1) return fail("dctfhe_session_set_shard: the margin audit is on, and it stays unsharded: turn it off first");
  if (s->budget_bytes && parts > 1) return fail("dctfhe_session_set_shard: the session has a memory budget (%zu bytes), and a budgeted session stays unsharded", s->budget_bytes);
  if (s->shard_pool) return fail("dctfhe_session_set_shard: the max pools are divided for part %d of %d: turn that off first (dctfhe_session_set_shard_pool)", s->part, s->parts);
  s->part = part; s->parts = parts; s->shard_set = true;
  return 0;
}
// ---- divided max pools: the partition rule of one pool, the switch, the rows a part holds, the plan with row ranges
static bool pool_geometry_ok(int batch, int C, int H, int W, int k, int s, int p) {
  return batch >= 1 && C >= 1 && H >= 1 && W >= 1 && k >= 1 && k <= 32 && s >= 1 && p >= 0 && 2 * p <= k && H + 2 * p >= k && W + 2 * p >= k;
}
extern "C" int dctfhe_shard_pool(int batch, int C, int H, int W, int k, int s, int pad, int parts, int part, size_t* out_first, size_t* out_count,
                                 size_t* in_first, size_t* in_count, size_t* pairs) {
  if (!out_first || !out_count || !in_first || !in_count || !pairs) return fail("dctfhe_shard_pool: null argument");
  if (!pool_geometry_ok(batch, C, H, W, k, s, pad))
    return fail("dctfhe_shard_pool: bad geometry (1 <= k <= 32, s >= 1, 0 <= p <= k/2, window inside the padded input)");
  const size_t n_out = (size_t)batch * C * pool_out_size(H, k, s, pad) * pool_out_size(W, k, s, pad);
  size_t range[2];
  CHK(dctfhe_shard_rows(n_out, parts, part, &range[0], &range[1]));
  PoolPlan P;
  std::vector<int32_t> maps;
  CHK(pool_plan_host(batch, C, H, W, k, s, pad, parts > 1 ? range : nullptr, &P, &maps));      // one part: the undivided op as it runs today
  *out_first = range[0]; *out_count = range[1];
  *in_first = parts > 1 ? P.in_first : 0; *in_count = parts > 1 ? P.in_count : (size_t)batch * C * H * W;
  *pairs = P.pairs_per_batch;
  return 0;
}
extern "C" int dctfhe_session_set_shard_pool(dctfhe_session* s, int on) {
  if (!s) return fail("dctfhe_session_set_shard_pool: null session");
  if (s->has_run) return fail("dctfhe_session_set_shard_pool: the session has run; divide its max pools before its first run");
  if (s->d_audit_key.p) return fail("dctfhe_session_set_shard_pool: the margin audit is on, and it stays unsharded: turn it off first");
  if (!s->shard_set) return fail("dctfhe_session_set_shard_pool: the session is not sharded: call dctfhe_session_set_shard first");
  const bool want = on != 0 && s->parts > 1;      // one part of one: the undivided op
  if (want == s->shard_pool) return 0;
  HIPCHK(hipSetDevice(s->ctx->device));
  s->shard_pool = want;
  return session_plan_buffers(s, nullptr, true);      // the pools' trees and level buffers for this part (or the whole op again); the input's buffer and the look-up scratch stay
}
// the first rows of [first, first + count) of tensor t that this session does not hold: neither its own part's nor marked.  false: none
static bool rows_missing(const dctfhe_session* s, int t, size_t first, size_t count, size_t* g0, size_t* g1) {
  if (s->whole[t] || count == 0) return false;
  std::vector<std::pair<size_t, size_t>> have = s->marked[t];
  size_t f = 0, n = 0;
  dctfhe_shard_rows((size_t)s->batch * s->circ->tensors[t].elems(), s->parts, s->part, &f, &n);
  have.push_back({f, f + n});
  std::sort(have.begin(), have.end());
  size_t pos = first;
  const size_t end = first + count;
  for (const auto& iv : have) {
    if (pos >= end) break;
    if (iv.first > pos) { *g0 = pos; *g1 = std::min(iv.first, end); return true; }
    pos = std::max(pos, iv.second);
  }
  if (pos < end) { *g0 = pos; *g1 = end; return true; }
  return false;
}
extern "C" int dctfhe_session_pool_pairs(dctfhe_session* s, int op, size_t* pairs) {
  if (!s || !pairs) return fail("dctfhe_session_pool_pairs: null argument");
  if (op < 0 || op >= (int)s->circ->ops.size() || s->circ->ops[op].type != OP_MAXPOOL) return fail("dctfhe_session_pool_pairs: op %d is not a max pool", op);
  *pairs = s->pool_pairs_run[op];
  return 0;
}
// the exchange points of a circuit: (op after which, tensor) per sliced tensor that a whole-needing op or the download reads.  divided:
// a max pool runs on its part's outputs, leaves its destination sliced and needs only a range of its source: reader = that pool's op
// (-1: the whole tensor is needed).  A tensor that a pool and later a whole-needing op read travels whole, once.
struct ShardEntry { int after_op, tensor, reader; };
static void shard_plan_of(const CircuitPlan& c, bool divided, std::vector<ShardEntry>* plan) {
  std::vector<char> state(c.tensors.size(), 2);      // 0: sliced, 1: a pool's need range is there, 2: whole
  std::vector<int> writer(c.tensors.size(), -1);
  auto need = [&](int t, int reader) {
    if (state[t] == 0) plan->push_back({writer[t], t, reader});
    else if (state[t] == 1) {      // a second reader of a ranged tensor: it travels whole
      for (ShardEntry& e : *plan) if (e.tensor == t && e.after_op == writer[t]) e.reader = -1;
      reader = -1;
    }
    state[t] = std::max<char>(state[t], reader < 0 ? 2 : 1);
  };
  for (int i = 0; i < (int)c.ops.size(); i++) {
    const SiteOp& o = c.ops[i];
    if (op_runs_sliced(o)) { state[o.dst] = 0; writer[o.dst] = i; continue; }
    const bool part_only = divided && o.type == OP_MAXPOOL;
    need(o.src0, part_only ? i : -1);
    state[o.dst] = part_only ? 0 : 2;
    writer[o.dst] = i;
  }
  need(c.output_tensor, -1);
  std::sort(plan->begin(), plan->end(), [](const ShardEntry& a, const ShardEntry& b) { return std::make_pair(a.after_op, a.tensor) < std::make_pair(b.after_op, b.tensor); });
}
extern "C" int dctfhe_session_shard_plan(dctfhe_session* s, int32_t* after_op, int32_t* tensor, int capacity, int* n) {
  if (!s || !n) return fail("dctfhe_session_shard_plan: null argument");
  std::vector<ShardEntry> plan;
  shard_plan_of(*s->circ, s->shard_pool, &plan);
  *n = (int)plan.size();
  if (!after_op || !tensor) return 0;
  if (capacity < *n) return fail("dctfhe_session_shard_plan: room for %d entries, the circuit has %d", capacity, *n);
  for (int i = 0; i < *n; i++) { after_op[i] = plan[i].after_op; tensor[i] = plan[i].tensor; }
  return 0;
}
extern "C" int dctfhe_session_shard_plan_rows(dctfhe_session* s, int32_t* after_op, int32_t* tensor, size_t* first, size_t* count, int capacity, int* n) {
  if (!s || !n) return fail("dctfhe_session_shard_plan_rows: null argument");
  std::vector<ShardEntry> plan;
  shard_plan_of(*s->circ, s->shard_pool, &plan);
  *n = (int)plan.size();
  if (!after_op || !tensor || !first || !count) return 0;
  if (capacity < *n) return fail("dctfhe_session_shard_plan_rows: room for %d entries, the circuit has %d", capacity, *n);
  for (int i = 0; i < *n; i++) {
    const ShardEntry& e = plan[i];
    after_op[i] = e.after_op; tensor[i] = e.tensor;
    first[i] = e.reader < 0 ? 0 : s->pool[e.reader]->in_first;
    count[i] = e.reader < 0 ? (size_t)s->batch * s->circ->tensors[e.tensor].elems() : s->pool[e.reader]->in_count;
  }
  return 0;
}
static int tensor_ok(const dctfhe_session* s, int t, const char* who) {
  if (t < 0 || t >= (int)s->circ->tensors.size()) return fail("%s: tensor %d out of range (%zu tensors)", who, t, s->circ->tensors.size());
  if (!s->d_tensor[t]) return fail("%s: tensor %d has no storage (no op of the circuit touches it)", who, t);
  return 0;
}
extern "C" int dctfhe_session_tensor(dctfhe_session* s, int tensor, void** dev, size_t* row_words, size_t* rows) {
  if (!s || !dev || !row_words || !rows) return fail("dctfhe_session_tensor: null argument");
  CHK(tensor_ok(s, tensor, "dctfhe_session_tensor"));
  *dev = s->d_tensor[tensor]; *row_words = s->t_L[tensor]; *rows = s->tensor_words[tensor] / s->t_L[tensor];
  return 0;
}
extern "C" int dctfhe_session_mark_whole(dctfhe_session* s, int tensor) {
  if (!s) return fail("dctfhe_session_mark_whole: null session");
  CHK(tensor_ok(s, tensor, "dctfhe_session_mark_whole"));
  s->whole[tensor] = 1;
  return 0;
}
extern "C" int dctfhe_session_mark_rows(dctfhe_session* s, int tensor, size_t first, size_t count) {
  if (!s) return fail("dctfhe_session_mark_rows: null session");
  CHK(tensor_ok(s, tensor, "dctfhe_session_mark_rows"));
  const size_t rows = s->tensor_words[tensor] / s->t_L[tensor];
  if (first > rows || count > rows - first) return fail("dctfhe_session_mark_rows: rows %zu .. %zu of a tensor of %zu", first, first + count, rows);
  if (s->whole[tensor] || count == 0) return 0;
  s->marked[tensor].push_back({first, first + count});
  size_t g0, g1;
  if (!rows_missing(s, tensor, 0, rows, &g0, &g1)) { s->whole[tensor] = 1; s->marked[tensor].clear(); }
  return 0;
}
extern "C" int dctfhe_session_copy_rows(dctfhe_session* dst, dctfhe_session* src, int tensor, size_t first, size_t count) {
  if (!dst || !src) return fail("dctfhe_session_copy_rows: null session");
  if (dst->circ != src->circ) return fail("dctfhe_session_copy_rows: the sessions run different circuits");
  if (dst->batch != src->batch) return fail("dctfhe_session_copy_rows: the sessions differ in batch (%d and %d)", dst->batch, src->batch);
  CHK(tensor_ok(dst, tensor, "dctfhe_session_copy_rows"));
  CHK(tensor_ok(src, tensor, "dctfhe_session_copy_rows"));
  const size_t L = dst->t_L[tensor], rows = dst->tensor_words[tensor] / L;
  if ((dst->keys == nullptr) != (src->keys == nullptr) || src->t_L[tensor] != L)
    return fail("dctfhe_session_copy_rows: the sessions store tensor %d differently (rows of %zu and %zu words)", tensor, L, src->t_L[tensor]);
  if (dst->ctx->device != src->ctx->device) return fail("dctfhe_session_copy_rows: the sessions live on devices %d and %d", dst->ctx->device, src->ctx->device);
  if (first > rows || count > rows - first) return fail("dctfhe_session_copy_rows: rows %zu .. %zu of a tensor of %zu", first, first + count, rows);
  if (count == 0 || dst == src) return 0;
  HIPCHK(hipSetDevice(dst->ctx->device));
  if (src->ctx->stream != dst->ctx->stream) {      // after src's work: its runs are synchronous, an event covers whatever else its stream holds
    DevEvent e;
    HIPCHK(e.create());
    HIPCHK(hipEventRecord(e.e, src->ctx->stream));
    HIPCHK(hipStreamWaitEvent(dst->ctx->stream, e.e, 0));
    HIPCHK(hipMemcpyAsync(dst->d_tensor[tensor] + first * L, src->d_tensor[tensor] + first * L, count * L * 8, hipMemcpyDeviceToDevice, dst->ctx->stream));
    HIPCHK(hipStreamSynchronize(dst->ctx->stream));      // the event dies with this scope
    return 0;
  }
  HIPCHK(hipMemcpyAsync(dst->d_tensor[tensor] + first * L, src->d_tensor[tensor] + first * L, count * L * 8, hipMemcpyDeviceToDevice, dst->ctx->stream));
  return 0;
}

// ops [first_op, end_op) of the circuit on the session's part: look-ups and adds on its rows, everything else in full
static int session_run_ops(dctfhe_session* s, int first_op, int end_op, dctfhe_timing* timing) {
  HIPCHK(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  dctfhe_circuit* c = s->circ;
  dctfhe_keys* K = s->keys;
  const int B = s->batch;
  const bool sharded = s->parts > 1;
  s->has_run = true;
  Timers tm{st, timing != nullptr, &s->ev_pool, {}};
  const hipEvent_t e0 = tm.take(), e1 = tm.take();
  HIPCHK(hipEventRecord(e0, st));
  if (timing) memset(timing, 0, sizeof *timing);
  const LutScratch& sc = s->lut;
  const bool audit = s->d_audit_key.p != nullptr;
  if (audit && first_op == 0 && !s->audit_slots.empty())      // every run starts from zeroed slots
    HIPCHK(hipMemsetAsync(s->d_audit.p, 0, s->audit_slots.size() * sizeof(margin_slot), st));
  // one op on the rows it is given.  src / dst point at the first row read / written; r0 is that row's number in the WHOLE tensor (tables
  // per channel and `simulate` noise go by it), rn the rows.  A convolution: conv_batch images from src, output window `window`.  A max
  // pool: the tree `plan` (its maps count from src), or in clear mode the element bases of src and dst.
  struct OpCall { const uint64_t* src; uint64_t* dst; size_t r0, rn; int conv_batch; const ConvWindow* window; const PoolPlan* plan; size_t in_base, out_base; };
  auto run_op = [&](size_t i, const OpCall& call) -> int {
    const SiteOp& o = c->ops[i];
    const MarginProbe probe_i = audit ? MarginProbe{s->d_audit_key.as<uint8_t>(), s->d_audit.as<margin_slot>() + s->audit_first[i]} : MarginProbe{};
    const MarginProbe* probe = audit ? &probe_i : nullptr;
    const TensorShape& a = c->tensors[o.src0];
    const TensorShape& d = c->tensors[o.dst];
    const uint64_t* src = call.src;
    uint64_t* dst = call.dst;
    const size_t r0 = call.r0, rn = call.rn;
    const size_t Ls = s->t_L[o.src0], Ld = s->t_L[o.dst], ds = s->t_deff[o.src0];
    const double sg = i < s->sim_sigma.size() ? s->sim_sigma[i] : 0.0;      // clear mode: the noise `simulate` injects at this op
    switch (o.type) {
      case OP_CONV: {
        const int h = tm.begin(CAT_LINEAR);
        CHK(dev_conv2d(s->ctx, src, call.conv_batch, a.C, a.H, a.W, Ls, ds, c->d_payload[i].as<int8_t>(), &c->conv[i], o.conv.Cout, o.conv.KH, o.conv.KW, o.conv.stride,
                       o.conv.pad, dst, Ld, call.window));
        tm.end(h);
        break;
      }
      case OP_ADD: {
        const int h = tm.begin(CAT_LINEAR);
        const size_t Lb = s->t_L[o.src1];
        hipLaunchKernelGGL(k_add, dim3(ew_grid(rn * Ld)), dim3(256), 0, st, src, Ls, ds, s->d_tensor[o.src1] + r0 * Lb, Lb, s->t_deff[o.src1], dst, Ld, rn);
        HIPCHK(hipGetLastError());
        tm.end(h);
        break;
      }
      case OP_SUMPOOL: {
        const int h = tm.begin(CAT_LINEAR);
        const size_t tw = s->tensor_words[o.dst];
        hipLaunchKernelGGL(k_sum_pool, dim3(ew_grid(tw)), dim3(256), 0, st, src, a.C, a.H, a.W, Ls, ds, o.sum_k, d.H, d.W, dst, Ld, tw);
        HIPCHK(hipGetLastError());
        tm.end(h);
        break;
      }
      case OP_LUT: {
        const LutSite& L = o.lut;
        const size_t E = rn;
        const int hw = a.H * a.W;
        // (src / dst: the slice; r0 goes along wherever the element's number in the tensor is meant)
        const int64_t* halves = c->d_split[i].as<int64_t>();      // [S | Dt] of a parity split, else nullptr
        const int64_t* half_d = halves ? halves + ((size_t)L.ntab << (L.w - 1)) : nullptr;
        if (!K) {
          const double sg2 = (i < s->sim_sigma2.size() && s->sim_sigma2[i] > 0) ? s->sim_sigma2[i] : sg;
          hipLaunchKernelGGL(k_lut_clear, dim3(ew_grid(E)), dim3(256), 0, st, src, dst, E, L.shift, L.body_add, L.p, L.r, L.w, c->d_payload[i].as<int64_t>(),
                             hw, L.ntab, s->d_overflow.as<int>(), sg, rng_key{{(uint32_t)s->sim_seed, (uint32_t)(s->sim_seed >> 32), 0x73696d75u, 0, 0, 0, 0, 0}},
                             (uint64_t)(0x51D0000 + (s->sim_run << 12) + i), (int)L.approx(), (int)L.split(), sg2, halves, half_d, r0);
          HIPCHK(hipGetLastError());
        } else {
          // the one-bit steps clear the low bits in place on a shifted copy of the input (+ LutSite::round_add).  Approximate rounding (the
          // reference README's {"method": "approximate"}): no steps, and without steps nothing is copied: the key switch reads the input.
          int deff = (int)ds;
          if (L.n_steps() > 0) {
            deff = round_chain_deff(K, (int)ds, L);
            // the work row: the first deff mask words and the body.  What lies between deff and the end of the row is left alone when
            // every key switch of the site narrows to deff (the table bootstrap that ends the site rewrites the row); a key switch
            // that cannot narrow reads the whole row, so those words are zeroed (they used to be whatever the recycled
            // buffer held)
            bool narrow = true;
            for_each_bootstrap(L, K->p, [&](int tier, int, bool) { narrow = narrow && ks_narrows(K, tier, deff); });
            const size_t fill = narrow ? (size_t)deff : Ld - 1;
            const int h = tm.begin(CAT_LINEAR);
            hipLaunchKernelGGL(k_affine, dim3(ew_grid(E * (fill + 1))), dim3(256), 0, st, src, Ls, ds, dst, Ld, E, fill, L.shift, L.round_add());
            HIPCHK(hipGetLastError());
            tm.end(h);
          }
          LutRows rows;
          rows.src = src; rows.Ls = Ls; rows.work = dst; rows.Lw = Ld; rows.par = s->pool_buf[i][0]; rows.Lp = Ld;
          rows.tables = c->d_payload[i].as<int64_t>(); rows.tab_s = halves; rows.tab_d = half_d;
          CHK(dev_round_lut(K, L, rows, E, hw, sc, &tm, deff, probe, r0));
        }
        break;
      }
      case OP_MAXPOOL: {
        const PoolSite& S = o.pool;
        const PoolPlan& pp = *call.plan;
        if (!K) {
          const int h = tm.begin(CAT_LINEAR);
          CHK(clear_max_pool(st, src, s->pool_buf[i][0], dst, B, a.C, a.H, a.W, S.k, S.stride, S.pad, S.shift, S.body_add, S.p_d, c->d_payload[i].as<int64_t>(), sg,
                             s->sim_seed, (1ULL << 40) | ((uint64_t)(0x51D0000 + (s->sim_run << 12) + i) << 1), pp.mid_first, pp.mid_count, pp.out_first, pp.out_count,
                             call.in_base, call.out_base));
          tm.end(h);
        } else {
          size_t launched = 0;
          uint64_t* const bufs[2] = {s->pool_buf[i][0], s->pool_buf[i][1]};
          CHK(dev_max_pool(K, S, pp, src, Ls, ds, bufs, dst, Ld, s->t_deff[o.dst], c->d_payload[i].as<int64_t>(), sc, &tm, probe, &launched));
          s->pool_pairs_run[i] += launched;
        }
        break;
      }
      default: return fail("op %zu: unknown type %d", i, o.type);
    }
    return 0;
  };
  for (size_t i = (size_t)first_op; i < (size_t)end_op; i++) {
    const SiteOp& o = c->ops[i];
    if (s->divided_group[i] >= 0) {
      // a divided slab group (memory budget): per image and per slab of S channels, the windowed convolution into the slab's buffer, then
      // every op behind it on the slab's rows; the last op writes its rows into the whole destination at their place.  All channels of a
      // slab are whole, so a max pool has no halo.  (dctfhe_session_run_span admits whole groups only; never sharded, never audited.)
      const SlabGroup& G = c->groups[s->divided_group[i]];
      const int S = s->slab[s->divided_group[i]];
      for (int j = G.first; j < G.end; j++) { s->whole[c->ops[j].dst] = 1; s->marked[c->ops[j].dst].clear(); s->pool_pairs_run[j] = 0; }
      const TensorShape& in_t = c->tensors[o.src0];
      for (int b = 0; b < B; b++)
        for (int c0 = 0; c0 < G.channels; c0 += S) {
          const int c1 = std::min(c0 + S, G.channels);
          const ConvWindow window{c0, c1};
          for (int j = G.first; j < G.end; j++) {
            const SiteOp& oj = c->ops[j];
            const TensorShape& a = c->tensors[oj.src0];
            const TensorShape& d = c->tensors[oj.dst];
            const bool last = j == G.end - 1;
            // the slab's first row in the whole source / destination; a transient buffer holds the slab from its row 0
            const size_t in_row = ((size_t)b * G.channels + c0) * a.H * a.W, out_row = ((size_t)b * G.channels + c0) * d.H * d.W;
            OpCall call{};
            call.src = j == G.first ? s->d_tensor[oj.src0] + (size_t)b * in_t.elems() * s->t_L[oj.src0] : s->d_tensor[oj.src0];
            call.dst = s->d_tensor[oj.dst] + (last ? out_row * s->t_L[oj.dst] : 0);
            call.r0 = out_row; call.rn = (size_t)(c1 - c0) * d.H * d.W;
            call.conv_batch = 1; call.window = &window;
            PoolPlan clear_range;      // clear mode: the slab's intermediates and outputs by their numbers in the whole op
            if (oj.type == OP_MAXPOOL) {
              call.plan = (c1 - c0 == S ? s->pool[j] : s->pool_last[j]).get();
              if (!K) {
                clear_range.mid_first = ((size_t)b * G.channels + c0) * a.H * d.W; clear_range.mid_count = (size_t)(c1 - c0) * a.H * d.W;
                clear_range.out_first = out_row; clear_range.out_count = call.rn;
                call.plan = &clear_range;
                call.in_base = in_row; call.out_base = last ? 0 : out_row;
                call.dst = s->d_tensor[oj.dst];      // ... the kernel places the rows itself
              }
            }
            CHK(run_op((size_t)j, call));
          }
        }
      i = (size_t)G.end - 1;
      continue;
    }
    // this part's rows of an element-wise op (all of them in an unsharded session); any other op reads whole tensors
    size_t r0 = 0, rn = (size_t)B * c->tensors[o.dst].elems();
    if (op_runs_sliced(o)) {
      CHK(dctfhe_shard_rows(rn, s->parts, s->part, &r0, &rn));
      s->whole[o.dst] = !sharded;
      s->marked[o.dst].clear();
    } else if (o.type == OP_MAXPOOL && s->shard_pool) {      // a divided pool: the part's outputs, from the need range of its source
      const PoolPlan& pp = *s->pool[i];
      size_t g0 = 0, g1 = 0;
      if (rows_missing(s, o.src0, pp.in_first, pp.in_count, &g0, &g1))
        return fail("op %zu (max pool) reads rows %zu .. %zu of tensor %d, and part %d of %d lacks rows %zu .. %zu: bring them in and call dctfhe_session_mark_rows first",
                    i, pp.in_first, pp.in_first + pp.in_count, o.src0, s->part, s->parts, g0, g1);
      r0 = pp.out_first; rn = pp.out_count;
      s->whole[o.dst] = 0;
      s->marked[o.dst].clear();
    } else {
      if (!s->whole[o.src0])
        return fail("op %zu needs tensor %d whole, and it holds only the rows of part %d of %d: exchange the other parts' rows and call dctfhe_session_mark_whole first",
                    i, o.src0, s->part, s->parts);
      s->whole[o.dst] = 1;
      s->marked[o.dst].clear();
    }
    s->pool_pairs_run[i] = 0;
    if (rn == 0) continue;      // an empty part of a small tensor
    OpCall call{};
    const bool sliced = o.type == OP_LUT || o.type == OP_ADD;      // their pointers are the slice's; every other op is given the whole tensors
    call.src = s->d_tensor[o.src0] + (sliced ? r0 * s->t_L[o.src0] : 0);
    call.dst = s->d_tensor[o.dst] + (sliced ? r0 * s->t_L[o.dst] : 0);
    call.r0 = r0; call.rn = rn; call.conv_batch = B; call.plan = s->pool[i].get();
    CHK(run_op(i, call));
  }
  if (end_op == (int)c->ops.size() && first_op < end_op) s->sim_run++;      // `simulate` draws afresh in every pass over the circuit (its last op ends one)
  HIPCHK(hipEventRecord(e1, st));
  HIPCHK(hipEventSynchronize(e1));
  if (timing) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    timing->total_ms = ms;
    for (auto& sp : tm.spans) {
      float t = 0;
      hipEventElapsedTime(&t, sp.a, sp.b);
      if (sp.cat == CAT_LINEAR) timing->linear_ms += t;
      else if (sp.cat == CAT_KS) timing->ks_ms += t;
      else if (sp.cat >= 0 && sp.cat < DCTFHE_MAX_TIERS) { timing->pbs_ms[sp.cat] += t; timing->pbs_launches[sp.cat]++; }
    }
    for (int i = 0; i < DCTFHE_MAX_TIERS; i++) timing->pbs_cts[i] = s->pbs_per_image[i] * B;
  }
  if (audit) CHK(session_audit_collect(s));
  if (!K) {
    int ov = 0;
    HIPCHK(hipMemcpy(&ov, s->d_overflow.p, sizeof ov, hipMemcpyDeviceToHost));
    if (ov) {      // cleared on the run's stream and done before the caller is told: the next run starts from a clean flag on whatever stream it comes
      HIPCHK(hipMemsetAsync(s->d_overflow.p, 0, sizeof(int), st));
      HIPCHK(hipStreamSynchronize(st));
      return fail("clear run: a message left its padded range (calibration too tight)");
    }
  }
  return 0;
}
extern "C" int dctfhe_session_run_span(dctfhe_session* s, int first_op, int end_op, dctfhe_timing* timing) {
  if (!s) return fail("dctfhe_session_run_span: null session");
  const int n = (int)s->circ->ops.size();
  if (first_op < 0 || end_op < first_op || end_op > n) return fail("dctfhe_session_run_span: ops [%d, %d) of a circuit of %d", first_op, end_op, n);
  for (size_t g = 0; g < s->circ->groups.size(); g++) {      // a divided slab group runs slab by slab, all its ops per slab: whole or not at all
    const SlabGroup& G = s->circ->groups[g];
    if (s->slab[g] < G.channels && first_op < end_op && ((first_op > G.first && first_op < G.end) || (end_op > G.first && end_op < G.end)))
      return fail("dctfhe_session_run_span: ops [%d, %d) cut the slab group of ops [%d, %d), which the memory budget divides into slabs of %d channels: a span holds it whole or not at all",
                  first_op, end_op, G.first, G.end, s->slab[g]);
  }
  return session_run_ops(s, first_op, end_op, timing);
}
extern "C" int dctfhe_session_run(dctfhe_session* s, dctfhe_timing* timing) { return session_run_ops(s, 0, (int)s->circ->ops.size(), timing); }

// ------------------------------------------------------------------------------------------ probes
// ---- margin audit, the primitives (include/dctfhe.h): the definition on the host, and the session's kernel on host rows
static void margin_accumulate(dctfhe_margin_stats* m, int32_t e) {
  const int32_t a = e < 0 ? -e : e;
  m->count++; m->sum += e; m->sum_sq += (uint64_t)((int64_t)e * e);
  m->max_abs = std::max(m->max_abs, a);
  m->hist[margin_bin(e, m->half_box)]++;
}
extern "C" int dctfhe_margin_probe_host(const uint8_t* small_key, int n, int logN, const uint64_t* cts_small, size_t count, int table_bits, int32_t* err,
                                        dctfhe_margin_stats* stats) {
  if (n < 1) return fail("dctfhe_margin_probe_host: small ciphertexts of %d mask words", n);
  if (logN < 1 || logN > 31) return fail("dctfhe_margin_probe_host: ring of 2^%d", logN);
  if (table_bits < 0 || logN - table_bits < 1) return fail("dctfhe_margin_probe_host: a table of %d input bits leaves no box on a ring of 2^%d (need 0 <= table_bits < logN)", table_bits, logN);
  if (!small_key || (count && !cts_small)) return fail("dctfhe_margin_probe_host: null argument");
  if (stats) *stats = margin_header(-1, -1, -1, logN, table_bits);
  for (size_t c = 0; c < count; c++) {
    const uint64_t* ct = cts_small + c * (size_t)(n + 1);
    uint32_t acc = 0;
    for (int i = 0; i < n; i++)
      if (small_key[i]) acc += margin_level(ct[i], logN);
    const int32_t e = margin_error(margin_level(ct[n], logN) - acc, logN, table_bits);
    if (err) err[c] = e;
    if (stats) margin_accumulate(stats, e);
  }
  return 0;
}
extern "C" int dctfhe_margin_probe(dctfhe_ctx* ctx, dctfhe_client_key* C, int tier, const uint64_t* cts_small, size_t count, int table_bits, int32_t* err,
                                   dctfhe_margin_stats* stats) {
  if (!ctx || !C || (count && !cts_small)) return fail("dctfhe_margin_probe: null argument");
  CHK(bound_to("dctfhe_margin_probe", ctx, C->ctx, "client key"));
  if (tier < 0 || tier >= C->p.n_tiers) return fail("dctfhe_margin_probe: tier %d out of range (%d tiers)", tier, C->p.n_tiers);
  const dctfhe_tier& t = C->p.tiers[tier];
  if (table_bits < 0 || t.logN - table_bits < 1)
    return fail("dctfhe_margin_probe: a table of %d input bits leaves no box on a ring of 2^%d (need 0 <= table_bits < logN)", table_bits, t.logN);
  if (stats) *stats = margin_header(-1, -1, tier, t.logN, table_bits);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t bytes = count * (size_t)(t.n + 1) * 8;
  DevBuf d_ct, d_err, d_slot;
  HIPCHK(d_ct.alloc(bytes));
  HIPCHK(hipMemcpyAsync(d_ct.p, cts_small, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (err) HIPCHK(d_err.alloc(count * 4));
  if (stats) { HIPCHK(d_slot.alloc(sizeof(margin_slot))); HIPCHK(hipMemsetAsync(d_slot.p, 0, sizeof(margin_slot), ctx->stream)); }
  CHK(dev_margin_probe(ctx->stream, t, C->s(), d_ct.as<uint64_t>(), count, table_bits, err ? d_err.as<int32_t>() : nullptr, stats ? d_slot.as<margin_slot>() : nullptr));
  if (err) HIPCHK(hipMemcpyAsync(err, d_err.p, count * 4, hipMemcpyDeviceToHost, ctx->stream));
  dctfhe_margin_stats dev;
  if (stats) HIPCHK(hipMemcpyAsync(&dev, d_slot.p, sizeof dev, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (stats) {
    stats->max_abs = dev.max_abs; stats->count = dev.count; stats->sum = dev.sum; stats->sum_sq = dev.sum_sq;
    memcpy(stats->hist, dev.hist, sizeof dev.hist);
  }
  return 0;
}

extern "C" int dctfhe_fp64_peak(dctfhe_ctx* ctx, double* tflops) {
  HIPCHK(hipSetDevice(ctx->device));
  const int blocks = ctx->prop.multiProcessorCount * 8, threads = 256, iters = 1 << 14;
  DevBuf d;
  HIPCHK(d.alloc((size_t)blocks * threads * 8));
  DevEvent a, b;
  HIPCHK(a.create()); HIPCHK(b.create());
  hipLaunchKernelGGL(k_fp64_peak, dim3(blocks), dim3(threads), 0, ctx->stream, d.as<double>(), iters);
  hipEventRecord(a.e, ctx->stream);
  for (int r = 0; r < 4; r++) hipLaunchKernelGGL(k_fp64_peak, dim3(blocks), dim3(threads), 0, ctx->stream, d.as<double>(), iters);
  hipEventRecord(b.e, ctx->stream);
  HIPCHK(hipEventSynchronize(b.e));
  float ms = 0;
  hipEventElapsedTime(&ms, a.e, b.e);
  *tflops = 4.0 * blocks * threads * (double)iters * 8 * 2 / (ms * 1e-3) / 1e12;
  return 0;
}

extern "C" int dctfhe_bench_pbs(dctfhe_ctx* ctx, dctfhe_keys* K, int tier, size_t count, int reps, double* ms_per_launch) {
  if (!ctx || !K || !ms_per_launch) return fail("dctfhe_bench_pbs: null argument");
  CHK(bound_to("dctfhe_bench_pbs", ctx, K->ctx, "evaluation keys"));
  if (tier < 0 || tier >= K->p.n_tiers) return fail("tier out of range");
  CHK(keys_hold("dctfhe_bench_pbs", K, tier, true, false));
  HIPCHK(hipSetDevice(ctx->device));
  const dctfhe_tier& t = K->p.tiers[tier];
  const size_t L = (size_t)K->p.D + 1;
  std::vector<uint64_t> h(count * (size_t)(t.n + 1));
  uint64_t stt = 12345;
  for (auto& v : h) { stt = stt * 6364136223846793005ULL + 1442695040888963407ULL; v = stt; }
  int64_t tab[16];
  for (int i = 0; i < 16; i++) tab[i] = (int64_t)i << 58;
  DevBuf d_small, d_out, d_tab;
  HIPCHK(d_small.upload(h.data(), h.size() * 8));
  HIPCHK(d_out.alloc(count * L * 8));
  HIPCHK(d_tab.upload(tab, sizeof tab));
  DevEvent a, b;
  HIPCHK(a.create()); HIPCHK(b.create());
  const PbsLut lut{d_tab.as<int64_t>(), 4};
  const PbsOut out{d_out.as<uint64_t>(), L};
  CHK(dev_pbs(K, tier, d_small.as<uint64_t>(), count, lut, out, nullptr));
  hipEventRecord(a.e, ctx->stream);
  for (int r = 0; r < reps; r++) CHK(dev_pbs(K, tier, d_small.as<uint64_t>(), count, lut, out, nullptr));
  hipEventRecord(b.e, ctx->stream);
  HIPCHK(hipEventSynchronize(b.e));
  float ms = 0;
  hipEventElapsedTime(&ms, a.e, b.e);
  *ms_per_launch = ms / reps;
  return 0;
}
