// client_host.cpp -- libdctfhe_client.so: the key owner's and the data owner's side of the engine on the host (include/dctfhe_client.h).
// Plain C++17 + OpenMP, no HIP.  The generator, the stream ids, the key-switch grid and the arithmetic of a noise draw come from
// client_shared.h, the header the device kernels include; what is restated here are the LOOPS of kernels.h (k_lwe_encrypt, k_ksk_gen,
// k_bsk_gen_bodies, k_pair_secret, k_ring_key_gen, k_pk_gen, k_pk_draws, k_pk_encrypt, k_phase16, k_ring_phase16) and the blob
// layouts of dctfhe.hip, each named where it stands.  Every output word is a function of its index alone, so no result depends on the
// number of threads.
#include <omp.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/dctfhe_client.h"
#include "client_shared.h"

using namespace dctfhe;

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
#define CHK(x)              \
  do {                      \
    int r_ = (x);           \
    if (r_ != 0) return r_; \
  } while (0)
// no exception crosses the C boundary: the bodies below only allocate, and a failed allocation is an error like any other
template <class F>
static int guarded(const char* who, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail("%s: out of host memory", who);
  }
}

extern "C" const char* dctfhe_host_last_error(void) { return g_err.c_str(); }
extern "C" int dctfhe_host_version(void) { return 1; }
extern "C" int dctfhe_host_threads(void) { return omp_get_max_threads(); }

// ------------------------------------------------------------------------------------------ generator
static rng_key key_from_bytes(const uint8_t* b) {
  rng_key k;
  for (int i = 0; i < 8; i++) k.k[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
  return k;
}
static void key_to_bytes(const rng_key& k, uint8_t* b) {
  for (int i = 0; i < 8; i++) for (int x = 0; x < 4; x++) b[4 * i + x] = (uint8_t)(k.k[i] >> (8 * x));
}
static rng_key key_from_block(const rng_key& key, uint64_t stream, uint64_t block) {
  uint32_t o[16];
  rng_key r;
  chacha20_block(key, stream, block, o);
  for (int i = 0; i < 8; i++) r.k[i] = o[i];
  return r;
}
// out[i] = rnd64(key, stream, idx0 + i) & and_mask, i < count: every ChaCha block computed once (idx0 need not start a block)
static void gen_words(const rng_key& key, uint64_t stream, uint64_t idx0, size_t count, uint64_t and_mask, uint64_t* out) {
  if (count == 0) return;
  const uint64_t last = idx0 + (count - 1);
  for (uint64_t b = idx0 >> 3; b <= (last >> 3); b++) {
    uint32_t o[16];
    chacha20_block(key, stream, b, o);
    for (int w = 0; w < 8; w++) {
      const uint64_t idx = 8 * b + w;
      if (idx >= idx0 && idx <= last) out[idx - idx0] = ((uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32)) & and_mask;
    }
    if (b == UINT64_MAX >> 3) break;
  }
}
// the Gaussian draw of index idx (kernels.h gauss_torus): words 2 idx and 2 idx + 1 share a block
static int64_t gauss_torus(const rng_key& key, uint64_t stream, uint64_t idx, double sigma) {
  if (sigma <= 0.0) return 0;
  uint32_t o[16];
  chacha20_block(key, stream, idx >> 2, o);
  const int w = (int)((2 * idx) & 7);
  return gauss_torus_words((uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32), (uint64_t)o[2 * w + 2] | ((uint64_t)o[2 * w + 3] << 32), sigma);
}
// out[i] = gauss_torus(key, stream, idx0 + i, sigma), i < count: a block holds four draws
static void gen_gauss(const rng_key& key, uint64_t stream, uint64_t idx0, size_t count, double sigma, int64_t* out) {
  if (sigma <= 0.0) { for (size_t i = 0; i < count; i++) out[i] = 0; return; }
  size_t i = 0;
  while (i < count) {
    const uint64_t idx = idx0 + i;
    uint32_t o[16];
    chacha20_block(key, stream, idx >> 2, o);
    for (int q = (int)(idx & 3); q < 4 && i < count; q++, i++)
      out[i] = gauss_torus_words((uint64_t)o[4 * q] | ((uint64_t)o[4 * q + 1] << 32), (uint64_t)o[4 * q + 2] | ((uint64_t)o[4 * q + 3] << 32), sigma);
  }
}
static int os_random(void* dst, size_t n) {
  size_t got = 0;
  while (got < n) {
    const ssize_t r = getrandom((char*)dst + got, n - got, 0);
    if (r <= 0) return -1;
    got += (size_t)r;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ parameters
// dctfhe.hip check_params without its kernel-shape question (include/dctfhe_client.h)
static int check_params(const dctfhe_params* p) {
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
    if (t.l == 4 && !(t.k == 1 && t.logN == 11 && t.beta <= 10))
      return fail("tier %d: bad bootstrap gadget (four levels only with k = 1, N = 2048, beta <= 10)", i);
    if (t.unroll != 1 && t.unroll != 2) return fail("tier %d: unroll must be 1 or 2", i);
    if (t.unroll == 2) {
      const bool paired = t.k == 1 && t.l == 1 && t.logN >= 11;
      const bool general = (t.k == 1 && t.l == 3 && t.logN == 11) || (t.k == 2 && t.l == 1 && t.logN == 10);
      if (!(paired || general) || (t.n & 1))
        return fail("tier %d: unroll 2 needs n even and (k, l, N) = (1, 1, >= 2048), (1, 3, 2048) or (2, 1, 1024)", i);
    }
    if (t.lk < 1 || t.lk > 63 || t.betak < 1 || t.betak > 8 || t.lk * t.betak > 63) return fail("tier %d: bad key-switch gadget (1 <= betak <= 8, lk >= 1, lk * betak <= 63)", i);
    if (!(t.lwe_sigma >= 0.0) || t.lwe_sigma > 1.0 || !(t.glwe_sigma >= 0.0) || t.glwe_sigma > 1.0) return fail("tier %d: noise parameter out of range", i);
    if (t.reserved != 0) return fail("tier %d: reserved must be 0", i);
    if (t.ksk_share >= i) return fail("tier %d: ksk_share must name an earlier tier", i);
    if (t.ksk_share >= 0) {
      const dctfhe_tier& o = p->tiers[t.ksk_share];
      if (o.n != t.n || o.lk != t.lk || o.betak != t.betak) return fail("tier %d: shared key-switch key has another shape", i);
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ client key
struct dctfhe_host_client_key {
  dctfhe_params p{};
  uint8_t seed[32] = {};
  rng_key sec{}, pub{};              // secret (key bits, noise) and public (masks) generator keys
  uint8_t nonce[16] = {};            // per-handle encryption nonce (dctfhe.h: ENCRYPTION RANDOMNESS IS PER HANDLE)
  rng_key enc_sec{}, enc_pub{};
  std::vector<uint8_t> S, s;         // key bits, one byte each
  std::vector<uint8_t> spair[DCTFHE_MAX_TIERS];      // unroll 2: the pair secret (k_pair_secret)
  uint64_t enc_calls = 0;
  ~dctfhe_host_client_key() {
    auto wipe = [](std::vector<uint8_t>& v) { if (!v.empty()) explicit_bzero(v.data(), v.size()); };
    wipe(S); wipe(s);
    for (auto& v : spair) wipe(v);
    explicit_bzero(seed, sizeof seed); explicit_bzero(&sec, sizeof sec); explicit_bzero(&enc_sec, sizeof enc_sec);
  }
};

// dctfhe.hip derive_encrypt_keys
static void derive_encrypt_keys(dctfhe_host_client_key* C) {
  const rng_key kdf = key_from_block(C->sec, STREAM_ENCKDF, 0);
  uint64_t n0 = 0, n1 = 0;
  for (int i = 0; i < 8; i++) { n0 |= (uint64_t)C->nonce[i] << (8 * i); n1 |= (uint64_t)C->nonce[8 + i] << (8 * i); }
  C->enc_sec = key_from_block(kdf, n0, n1);
  C->enc_pub = key_from_block(C->enc_sec, STREAM_PUBKEY, 0);
}
// k_gen_bits
static void gen_bits(const rng_key& key, uint64_t stream, std::vector<uint8_t>& out, size_t len) {
  std::vector<uint64_t> w(len);
  gen_words(key, stream, 0, len, ~0ULL, w.data());
  out.resize(len);
  for (size_t i = 0; i < len; i++) out[i] = (uint8_t)(w[i] >> 63);
  if (len) explicit_bzero(w.data(), len * 8);
}

extern "C" int dctfhe_host_client_key_create(const dctfhe_params* params, const uint8_t* seed32, dctfhe_host_client_key** out) {
  if (!params || !seed32 || !out) return fail("dctfhe_host_client_key_create: null argument");
  CHK(check_params(params));
  return guarded("dctfhe_host_client_key_create", [&]() -> int {
    std::unique_ptr<dctfhe_host_client_key> C(new dctfhe_host_client_key);
    C->p = *params;
    memcpy(C->seed, seed32, 32);
    C->sec = key_from_bytes(seed32);
    C->pub = key_from_block(C->sec, STREAM_PUBKEY, 0);
    if (os_random(C->nonce, sizeof C->nonce)) return fail("dctfhe_host_client_key_create: the OS gave no random bytes for the encryption nonce (getrandom)");
    derive_encrypt_keys(C.get());
    gen_bits(C->sec, STREAM_BIGKEY, C->S, (size_t)params->D);
    gen_bits(C->sec, STREAM_SMALLKEY, C->s, (size_t)params->n_max);
    for (int ti = 0; ti < params->n_tiers; ti++) {
      const dctfhe_tier& t = params->tiers[ti];
      if (t.unroll != 2) continue;
      std::vector<uint8_t>& o = C->spair[ti];
      o.assign((size_t)(3 * t.n / 2), 0);
      for (int i = 0; 2 * i + 1 < t.n; i++) {
        const uint8_t a = C->s[2 * i], b = C->s[2 * i + 1];
        o[3 * i] = a && !b; o[3 * i + 1] = !a && b; o[3 * i + 2] = a && b;
      }
    }
    *out = C.release();
    return 0;
  });
}
extern "C" int dctfhe_host_client_key_destroy(dctfhe_host_client_key* C) { delete C; return 0; }
extern "C" int dctfhe_host_client_key_export_secret(dctfhe_host_client_key* C, uint8_t* big_key, uint8_t* small_key) {
  if (!C || !big_key || !small_key) return fail("dctfhe_host_client_key_export_secret: null argument");
  memcpy(big_key, C->S.data(), C->S.size());
  memcpy(small_key, C->s.data(), C->s.size());
  return 0;
}
extern "C" int dctfhe_host_client_key_set_encrypt_counter(dctfhe_host_client_key* C, uint64_t next_call) {
  if (!C) return fail("null client key");
  if (next_call >= (1ULL << 47)) return fail("encrypt counter out of range");
  C->enc_calls = next_call;
  return 0;
}
extern "C" int dctfhe_host_client_key_set_encrypt_nonce(dctfhe_host_client_key* C, const uint8_t* nonce16) {
  if (!C || !nonce16) return fail("dctfhe_host_client_key_set_encrypt_nonce: null argument");
  memcpy(C->nonce, nonce16, sizeof C->nonce);
  derive_encrypt_keys(C);
  return 0;
}
extern "C" int dctfhe_host_client_key_public_keys(dctfhe_host_client_key* C, uint8_t* pub, uint8_t* enc_pub) {
  if (!C) return fail("dctfhe_host_client_key_public_keys: null argument");
  if (pub) key_to_bytes(C->pub, pub);
  if (enc_pub) key_to_bytes(C->enc_pub, enc_pub);
  return 0;
}

// ------------------------------------------------------------------------------------------ encrypt / decrypt
// k_lwe_encrypt (cts != NULL: rows of dim mask words + body) and k_lwe_encrypt_seeded (cts == NULL: bodies only), one call counter step
static int encrypt_impl(dctfhe_host_client_key* C, const uint64_t* phases, size_t count, int dim, uint64_t* cts, uint64_t* bodies, uint64_t* stream_out) {
  const int D = C->p.D, dim_eff = C->p.input_dim > 0 ? C->p.input_dim : D;
  const int nthr = omp_get_max_threads();
  std::vector<uint64_t> scratch((size_t)nthr * dim_eff);
  const uint64_t stream = (uint64_t)STREAM_ENC + ((++C->enc_calls) << 16);
  const uint8_t* S = C->S.data();
  const double sigma = C->p.input_sigma;
#pragma omp parallel for schedule(static)
  for (int64_t c = 0; c < (int64_t)count; c++) {
    uint64_t* a = cts ? cts + (size_t)c * (dim + 1) : scratch.data() + (size_t)omp_get_thread_num() * dim_eff;
    gen_words(C->enc_pub, stream, (uint64_t)c * (uint64_t)(D + 1), (size_t)dim_eff, ~0ULL, a);
    uint64_t sum = 0;
    for (int j = 0; j < dim_eff; j++) sum += S[j] ? a[j] : 0;
    const uint64_t b = sum + phases[c] + (uint64_t)gauss_torus(C->enc_sec, stream + 1, (uint64_t)c, sigma);
    if (cts) {
      for (int j = dim_eff; j < dim; j++) a[j] = 0;
      a[dim] = b;
    } else {
      bodies[c] = b;
    }
  }
  if (stream_out) *stream_out = stream;
  return 0;
}
extern "C" int dctfhe_host_encrypt_rows(dctfhe_host_client_key* C, const uint64_t* phases, size_t count, int dim, uint64_t* cts) {
  if (!C || (count && (!phases || !cts))) return fail("dctfhe_host_encrypt_rows: null argument");
  const int D = C->p.D, dim_eff = C->p.input_dim > 0 ? C->p.input_dim : D;
  if (dim < dim_eff || dim > D) return fail("dctfhe_host_encrypt_rows: rows of %d mask words; these parameters mask %d and the key has %d", dim, dim_eff, D);
  if (count == 0) return 0;
  return guarded("dctfhe_host_encrypt_rows", [&]() -> int { return encrypt_impl(C, phases, count, dim, cts, nullptr, nullptr); });
}
extern "C" int dctfhe_host_encrypt_seeded(dctfhe_host_client_key* C, const uint64_t* phases, size_t count, uint8_t* mask_key, uint64_t* stream_out,
                                          uint64_t* bodies) {
  if (!C || !mask_key || !stream_out || (count && (!phases || !bodies))) return fail("dctfhe_host_encrypt_seeded: null argument");
  key_to_bytes(C->enc_pub, mask_key);
  if (count == 0) { *stream_out = 0; return 0; }      // nothing drawn: the counter stays, as in dctfhe_host_encrypt_rows
  return guarded("dctfhe_host_encrypt_seeded", [&]() -> int { return encrypt_impl(C, phases, count, 0, nullptr, bodies, stream_out); });
}
// k_lwe_phase
extern "C" int dctfhe_host_decrypt_rows(dctfhe_host_client_key* C, const uint64_t* cts, size_t count, int dim, uint64_t* phases) {
  if (!C || (count && (!phases || !cts))) return fail("dctfhe_host_decrypt_rows: null argument");
  if (dim < 0 || dim > C->p.D) return fail("dctfhe_host_decrypt_rows: rows of %d mask words, the key has %d", dim, C->p.D);
  const uint8_t* S = C->S.data();
#pragma omp parallel for schedule(static)
  for (int64_t c = 0; c < (int64_t)count; c++) {
    const uint64_t* ct = cts + (size_t)c * (dim + 1);
    uint64_t sum = 0;
    for (int j = 0; j < dim; j++) sum += S[j] ? ct[j] : 0;
    phases[c] = ct[dim] - sum;
  }
  return 0;
}
// k_phase16
extern "C" int dctfhe_host_decrypt_packed(dctfhe_host_client_key* C, int n, const uint16_t* rows, size_t count, uint64_t* phases) {
  if (!C || (count && (!rows || !phases))) return fail("dctfhe_host_decrypt_packed: null argument");
  if (n < 1 || n > C->p.n_max) return fail("dctfhe_host_decrypt_packed: rows of %d mask words, the small key has %d", n, C->p.n_max);
  const uint8_t* s = C->s.data();
#pragma omp parallel for schedule(static)
  for (int64_t c = 0; c < (int64_t)count; c++) {
    const uint16_t* row = rows + (size_t)c * (n + 1);
    uint32_t part = 0;
    for (int j = 0; j < n; j++) part += s[j] ? row[j] : 0u;
    phases[c] = (uint64_t)(((uint32_t)row[n] - part) & 0xFFFFu) << 48;
  }
  return 0;
}
// k_ring_phase16
extern "C" int dctfhe_host_decrypt_ring(dctfhe_host_client_key* C, int logN, const uint16_t* words, size_t count, uint64_t* phases) {
  if (!C || (count && (!words || !phases))) return fail("dctfhe_host_decrypt_ring: null argument");
  if (logN < 5 || logN > 12) return fail("dctfhe_host_decrypt_ring: ring 2^%d outside 2^5 .. 2^12", logN);
  if ((1 << logN) > C->p.D) return fail("dctfhe_host_decrypt_ring: the ring key is a prefix of the big key: N_p = %d > D = %d", 1 << logN, C->p.D);
  const int N = 1 << logN;
  const uint8_t* Z = C->S.data();
#pragma omp parallel for schedule(static)
  for (int64_t x = 0; x < (int64_t)count; x++) {
    const size_t g = (size_t)x >> logN;
    const int i = (int)((size_t)x & (size_t)(N - 1));
    const uint16_t* grp = words + g * 2 * (size_t)N;
    uint32_t part = 0;
    for (int c = 0; c < N; c++) {
      if (!Z[c]) continue;
      const uint32_t a = grp[(i - c) & (N - 1)];
      part += c <= i ? a : 0u - a;
    }
    phases[x] = (uint64_t)(((uint32_t)grp[N + i] - part) & 0xFFFFu) << 48;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ GLWE rows
// positions of the set bits of key[0 .. N)
static std::vector<int> ones_of(const uint8_t* key, int N) {
  std::vector<int> o;
  for (int c = 0; c < N; c++) if (key[c]) o.push_back(c);
  return o;
}
// B += A * Z (negacyclic, mod 2^64), Z binary with its set bits at ones[]: shift and add
static void negacyclic_acc(uint64_t* __restrict__ B, const uint64_t* __restrict__ A, const int* ones, size_t n_ones, int N) {
  for (size_t q = 0; q < n_ones; q++) {
    const int m = ones[q];
    const uint64_t* lo = A + (N - m);
    for (int c = 0; c < m; c++) B[c] -= lo[c];
    uint64_t* hi = B + m;
    for (int c = 0; c < N - m; c++) hi[c] += A[c];
  }
}
// kernels.h bsk_row_zero: the noise draw into B, then per mask polynomial j < k the draw into A and B += A * S_j.  ones[j]: the set bits
// of S_j.  grow: the global row id.
static void glwe_row_zero(const std::vector<int>* ones, uint64_t grow, int k, int N, double sigma, const rng_key& pub, const rng_key& sec, uint64_t stream,
                          uint64_t* A, uint64_t* B) {
  gen_gauss(sec, stream + 1, grow * (uint64_t)N, (size_t)N, sigma, reinterpret_cast<int64_t*>(B));
  for (int j = 0; j < k; j++) {
    gen_words(pub, stream, (grow * (uint64_t)k + j) * (uint64_t)N, (size_t)N, ~0ULL, A);
    negacyclic_acc(B, A, ones[j].data(), ones[j].size(), N);
  }
}

// ------------------------------------------------------------------------------------------ compressed evaluation keys
struct EvalBlobHeader { uint32_t magic, version; uint64_t total_bytes; dctfhe_params params; };
static constexpr uint32_t EVAL_CBLOB_MAGIC = 0x43564544u /* 'DEVC' */, EVAL_CBLOB_VERSION = 1;
static size_t tier_bsk_blocks(const dctfhe_tier& t) { return (size_t)(t.unroll == 2 ? 3 * t.n / 2 : t.n); }
static size_t tier_bsk_body_words(const dctfhe_tier& t) { return tier_bsk_blocks(t) * (size_t)(t.k + 1) * t.l << t.logN; }
// tier selections (include/dctfhe.h TIER SELECTIONS): the rules of dctfhe.hip closed_selection / eval_cblob_size, restated for the host
static constexpr uint32_t EVAL_CBLOB_VERSION_PRUNED = 2;      // the masks follow pub[32]
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
static int closed_selection(const char* who, const dctfhe_params& p, const dctfhe_key_tiers* tiers, dctfhe_key_tiers* sel) {
  if (!tiers) { *sel = key_tiers_full(p); return 0; }
  *sel = *tiers;
  if ((sel->bsk | sel->ksk) & (~0u << p.n_tiers))
    return fail("%s: the tier selection names a tier at or beyond n_tiers = %d (bsk 0x%x, ksk 0x%x)", who, p.n_tiers, sel->bsk, sel->ksk);
  for (int ti = 0; ti < p.n_tiers; ti++) {
    if (((sel->ksk >> ti) & 1u) && p.tiers[ti].ksk_share >= 0)
      return fail("%s: the tier selection asks for a key-switch key of tier %d, which has none of its own (it shares tier %d's)", who, ti, p.tiers[ti].ksk_share);
    if ((sel->bsk >> ti) & 1u) sel->ksk |= 1u << ksk_owner(p, ti);
  }
  return 0;
}
static size_t eval_cblob_size(const dctfhe_params& p, const dctfhe_key_tiers& s) {
  const dctfhe_key_tiers f = key_tiers_full(p);
  size_t n = sizeof(EvalBlobHeader) + 32 + ((s.bsk == f.bsk && s.ksk == f.ksk) ? 0 : sizeof(dctfhe_key_tiers));
  for (int ti = 0; ti < p.n_tiers; ti++) {
    const dctfhe_tier& t = p.tiers[ti];
    if ((s.ksk >> ti) & 1u) n += (size_t)p.D * t.lk * 8;
    if ((s.bsk >> ti) & 1u) n += tier_bsk_body_words(t) * 8;
  }
  return n;
}

extern "C" int dctfhe_host_eval_keys_export_compressed_tiers(dctfhe_host_client_key* C, const dctfhe_key_tiers* tiers, void* buf, size_t capacity, size_t* size) {
  if (!C || !size) return fail("dctfhe_host_eval_keys_export_compressed: null argument");
  const dctfhe_params& P = C->p;
  dctfhe_key_tiers sel;
  if (closed_selection("dctfhe_host_eval_keys_export_compressed_tiers", P, tiers, &sel)) return -1;
  const dctfhe_key_tiers all = key_tiers_full(P);
  const bool full = sel.bsk == all.bsk && sel.ksk == all.ksk;
  const size_t need = eval_cblob_size(P, sel);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_host_eval_keys_export_compressed: buffer of %zu bytes, %zu needed", capacity, need);
  return guarded("dctfhe_host_eval_keys_export_compressed", [&]() -> int {
    EvalBlobHeader h{};
    h.magic = EVAL_CBLOB_MAGIC; h.version = full ? EVAL_CBLOB_VERSION : EVAL_CBLOB_VERSION_PRUNED; h.total_bytes = need; h.params = P;
    char* q = (char*)buf;
    memcpy(q, &h, sizeof h); q += sizeof h;
    key_to_bytes(C->pub, (uint8_t*)q); q += 32;
    if (!full) { memcpy(q, &sel, sizeof sel); q += sizeof sel; }
    const int nthr = omp_get_max_threads();
    const uint8_t *S = C->S.data(), *s = C->s.data();
    for (int ti = 0; ti < P.n_tiers; ti++) {
      const dctfhe_tier& t = P.tiers[ti];
      if ((sel.ksk >> ti) & 1u) {      // k_ksk_gen, the body column: row = i lk + lev
        const int64_t rows = (int64_t)P.D * t.lk;
        const int n = t.n, drop = 64 - 8 * ks_limbs(t.lk, t.betak);
        const uint64_t mask = drop ? ~0ULL << drop : ~0ULL, half = drop ? 1ULL << (drop - 1) : 0;
        const uint64_t stream = (uint64_t)(STREAM_KSK + 2 * ti);
        std::vector<uint64_t> scratch((size_t)nthr * n);
        uint64_t* dst = reinterpret_cast<uint64_t*>(q);      // offsets are multiples of 8 from a caller buffer: written through memcpy below
#pragma omp parallel for schedule(static)
        for (int64_t row = 0; row < rows; row++) {
          uint64_t* a = scratch.data() + (size_t)omp_get_thread_num() * n;
          gen_words(C->pub, stream, (uint64_t)row * (uint64_t)(n + 1), (size_t)n, mask, a);
          uint64_t b = 0;
          for (int j = 0; j < n; j++) b += s[j] ? a[j] : 0;
          b += (uint64_t)gauss_torus(C->sec, stream + 1, (uint64_t)row, t.lwe_sigma);
          const int i = (int)(row / t.lk), lev = (int)(row % t.lk);
          if (S[i]) b += 1ULL << (64 - t.betak * (lev + 1));
          b = (b + half) & mask;
          memcpy(reinterpret_cast<char*>(dst) + (size_t)row * 8, &b, 8);
        }
        q += (size_t)rows * 8;
      }
      if (!((sel.bsk >> ti) & 1u)) continue;
      // k_bsk_gen_bodies: global row grow = block (k + 1) l + r, bodies [blocks (k + 1) l][N]
      const int N = 1 << t.logN, k = t.k, rows = (k + 1) * t.l;
      const int64_t nrow = (int64_t)tier_bsk_blocks(t) * rows;
      const uint8_t* bits = t.unroll == 2 ? C->spair[ti].data() : s;
      std::vector<int> ones[2];
      for (int j = 0; j < k; j++) ones[j] = ones_of(S + (size_t)j * N, N);
      std::vector<uint64_t> scratch((size_t)nthr * 2 * N);
      const uint64_t stream = (uint64_t)(STREAM_BSK_MASK + 2 * ti);
      char* base = q;
#pragma omp parallel for schedule(dynamic, 1)
      for (int64_t grow = 0; grow < nrow; grow++) {
        uint64_t* A = scratch.data() + (size_t)omp_get_thread_num() * 2 * N;
        uint64_t* B = A + N;
        glwe_row_zero(ones, (uint64_t)grow, k, N, t.glwe_sigma, C->pub, C->sec, stream, A, B);
        const int i = (int)(grow / rows), r = (int)(grow % rows);
        if (bits[i]) {
          const int p = r / t.l, lev = r % t.l;
          const uint64_t g = 1ULL << (64 - t.beta * (lev + 1));
          if (p == k) {
            B[0] += g;
          } else {      // BODY FORM: the gadget term of mask polynomial p moves into the body as - s_i g S_p
            const uint8_t* Sp = S + (size_t)p * N;
            for (int c = 0; c < N; c++) B[c] -= Sp[c] ? g : 0;
          }
        }
        memcpy(base + (size_t)grow * N * 8, B, (size_t)N * 8);
      }
      q += (size_t)nrow * N * 8;
      explicit_bzero(scratch.data(), scratch.size() * 8);
    }
    return 0;
  });
}
extern "C" int dctfhe_host_eval_keys_export_compressed(dctfhe_host_client_key* C, void* buf, size_t capacity, size_t* size) {
  return dctfhe_host_eval_keys_export_compressed_tiers(C, nullptr, buf, capacity, size);
}

// ------------------------------------------------------------------------------------------ packing key (ring-packed results)
static constexpr uint32_t PACK_BLOB_MAGIC = 0x4b505244u /* 'DRPK' */, PACK_BLOB_VERSION = 1;
struct PackBlobHeader { uint32_t magic, version; int32_t logN, l, beta, n_max; double sigma; uint64_t total_bytes; };
// dctfhe.hip ring_stream: the stream R of dctfhe.h
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

// k_ring_key_gen: row r = j l + lev
extern "C" int dctfhe_host_pack_key_export(dctfhe_host_client_key* C, int logN, int l, int beta, double sigma, void* buf, size_t capacity, size_t* size) {
  if (!C || !size) return fail("dctfhe_host_pack_key_export: null argument");
  CHK(check_pack_spec("dctfhe_host_pack_key_export", logN, l, beta, C->p.n_max, sigma, C->p.D));
  const size_t need = pack_blob_size(logN, l, C->p.n_max);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_host_pack_key_export: buffer of %zu bytes, %zu needed", capacity, need);
  return guarded("dctfhe_host_pack_key_export", [&]() -> int {
    const int N = 1 << logN;
    const int64_t rows = (int64_t)C->p.n_max * l;
    PackBlobHeader h{};
    h.magic = PACK_BLOB_MAGIC; h.version = PACK_BLOB_VERSION; h.logN = logN; h.l = l; h.beta = beta; h.n_max = C->p.n_max; h.sigma = sigma;
    h.total_bytes = need;
    char* q = (char*)buf;
    memcpy(q, &h, sizeof h); q += sizeof h;
    key_to_bytes(C->pub, (uint8_t*)q); q += 32;
    const std::vector<int> ones = ones_of(C->S.data(), N);
    std::vector<uint64_t> scratch((size_t)omp_get_max_threads() * 2 * N);
    const uint64_t stream = ring_stream(logN, l, beta, sigma);
    const uint8_t* s = C->s.data();
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t r = 0; r < rows; r++) {
      uint64_t* A = scratch.data() + (size_t)omp_get_thread_num() * 2 * N;
      uint64_t* B = A + N;
      glwe_row_zero(&ones, (uint64_t)r, 1, N, sigma, C->pub, C->sec, stream, A, B);
      const int j = (int)(r / l), lev = (int)(r % l);
      if (s[j]) B[0] += 1ULL << (64 - beta * (lev + 1));
      memcpy(q + (size_t)r * N * 8, B, (size_t)N * 8);
    }
    explicit_bzero(scratch.data(), scratch.size() * 8);
    return 0;
  });
}

// ------------------------------------------------------------------------------------------ public-key inputs
static constexpr uint32_t PUB_BLOB_MAGIC = 0x4b425044u /* 'DPBK' */, PUB_BLOB_VERSION = 1;
struct PubBlobHeader { uint32_t magic, version; int32_t logN, reserved; double sigma; uint64_t total_bytes; };
// dctfhe.hip public_key_stream: the stream P of dctfhe.h
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

// k_pk_gen: row 0 of a k = 1 key without a message
extern "C" int dctfhe_host_public_key_export(dctfhe_host_client_key* C, int logN, double sigma, void* buf, size_t capacity, size_t* size) {
  if (!C || !size) return fail("dctfhe_host_public_key_export: null argument");
  CHK(check_public_spec("dctfhe_host_public_key_export", logN, sigma, C->p.input_dim > 0 ? C->p.input_dim : C->p.D));
  const size_t need = pub_blob_size(logN);
  *size = need;
  if (!buf) return 0;                       // size query
  if (capacity < need) return fail("dctfhe_host_public_key_export: buffer of %zu bytes, %zu needed", capacity, need);
  return guarded("dctfhe_host_public_key_export", [&]() -> int {
    const int N = 1 << logN;
    PubBlobHeader h{};
    h.magic = PUB_BLOB_MAGIC; h.version = PUB_BLOB_VERSION; h.logN = logN; h.sigma = sigma; h.total_bytes = need;
    char* q = (char*)buf;
    memcpy(q, &h, sizeof h); q += sizeof h;
    key_to_bytes(C->pub, (uint8_t*)q); q += 32;
    const std::vector<int> ones = ones_of(C->S.data(), N);
    std::vector<uint64_t> AB((size_t)2 * N);
    glwe_row_zero(&ones, 0, 1, N, sigma, C->pub, C->sec, public_key_stream(logN, sigma), AB.data(), AB.data() + N);
    memcpy(q, AB.data() + N, (size_t)N * 8);
    explicit_bzero(AB.data(), AB.size() * 8);
    return 0;
  });
}

struct dctfhe_host_public_key {
  int logN = 0;
  double sigma = 0;
  std::vector<uint64_t> key;     // [2][N_e]: A, B
  rng_key enc{};                 // the encryptor's own generator key (32 bytes from the OS at import)
  uint64_t calls = 0;            // call c draws from streams 3 c (u), 3 c + 1 (e1), 3 c + 2 (e2)
};
static constexpr uint64_t PUB_MAX_CALLS = 1ULL << 62;      // 3 c + 2 stays inside 64 bits

extern "C" int dctfhe_host_public_key_import(const void* buf, size_t size, dctfhe_host_public_key** out) {
  if (!buf || !out) return fail("dctfhe_host_public_key_import: null argument");
  if (size < sizeof(PubBlobHeader) + 32) return fail("dctfhe_host_public_key_import: public-key blob too short (%zu bytes)", size);
  PubBlobHeader h;
  memcpy(&h, buf, sizeof h);
  if (h.magic != PUB_BLOB_MAGIC) return fail("dctfhe_host_public_key_import: not a public-key blob (magic)");
  if (h.version != PUB_BLOB_VERSION) return fail("dctfhe_host_public_key_import: public-key blob version %u, this library reads %u", h.version, PUB_BLOB_VERSION);
  CHK(check_public_spec("dctfhe_host_public_key_import", h.logN, h.sigma, 0));
  if (h.total_bytes != size || pub_blob_size(h.logN) != size)
    return fail("dctfhe_host_public_key_import: public-key blob of %zu bytes, its header needs %zu (length)", size, pub_blob_size(h.logN));
  return guarded("dctfhe_host_public_key_import", [&]() -> int {
    std::unique_ptr<dctfhe_host_public_key> K(new dctfhe_host_public_key);
    K->logN = h.logN; K->sigma = h.sigma;
    uint8_t raw[32];
    if (os_random(raw, sizeof raw)) return fail("dctfhe_host_public_key_import: the OS gave no random bytes for the encryption key (getrandom)");
    K->enc = key_from_bytes(raw);
    const size_t N = (size_t)1 << h.logN;
    K->key.resize(2 * N);
    gen_words(key_from_bytes((const uint8_t*)buf + sizeof h), public_key_stream(h.logN, h.sigma), 0, N, ~0ULL, K->key.data());
    memcpy(K->key.data() + N, (const char*)buf + sizeof h + 32, N * 8);
    *out = K.release();
    return 0;
  });
}
extern "C" int dctfhe_host_public_key_destroy(dctfhe_host_public_key* K) {
  if (K) explicit_bzero(&K->enc, sizeof K->enc);
  delete K;
  return 0;
}
extern "C" int dctfhe_host_public_key_info(dctfhe_host_public_key* K, int* logN, double* sigma) {
  if (!K) return fail("dctfhe_host_public_key_info: null argument");
  if (logN) *logN = K->logN;
  if (sigma) *sigma = K->sigma;
  return 0;
}
extern "C" int dctfhe_host_public_key_set_encrypt_seed(dctfhe_host_public_key* K, const uint8_t* seed32) {
  if (!K || !seed32) return fail("dctfhe_host_public_key_set_encrypt_seed: null argument");
  K->enc = key_from_bytes(seed32);
  K->calls = 0;
  return 0;
}
// k_pk_draws, per group of N_e indices: u one byte per bit, e1 for x < groups N_e, e2 for x < count
static void public_draws(const dctfhe_host_public_key* K, uint64_t call, size_t count, uint8_t* u, int64_t* e1, int64_t* e2) {
  const size_t N = (size_t)1 << K->logN, groups = (count + N - 1) / N;
#pragma omp parallel for schedule(static)
  for (int64_t g = 0; g < (int64_t)groups; g++) {
    const size_t x0 = (size_t)g * N, m = std::min(N, count - x0);
    uint64_t w[8];
    for (size_t c = 0; c < N; c += 8) {      // N is a multiple of 8: a group starts a block
      gen_words(K->enc, 3 * call, x0 + c, 8, ~0ULL, w);
      for (int i = 0; i < 8; i++) u[x0 + c + i] = (uint8_t)(w[i] >> 63);
    }
    gen_gauss(K->enc, 3 * call + 1, x0, N, K->sigma, e1 + x0);
    gen_gauss(K->enc, 3 * call + 2, x0, m, K->sigma, e2 + x0);
  }
}
extern "C" int dctfhe_host_public_key_draws(dctfhe_host_public_key* K, uint64_t call, size_t count, uint8_t* u, int64_t* e1, int64_t* e2) {
  if (!K || !u || !e1 || !e2) return fail("dctfhe_host_public_key_draws: null argument");
  if (count == 0) return fail("dctfhe_host_public_key_draws: no phases (count == 0)");
  if (call >= PUB_MAX_CALLS) return fail("dctfhe_host_public_key_draws: call counter out of range");
  public_draws(K, call, count, u, e1, e2);
  return 0;
}
// k_pk_encrypt: C_a = A u + e1, C_b[i] = (B u)[i] + e2[i] + phase_i (i < m); per group its N_e mask words, then its first m body words
extern "C" int dctfhe_host_encrypt_public(dctfhe_host_public_key* K, const uint64_t* phases, size_t count, uint64_t* words_out) {
  if (!K || !phases || !words_out) return fail("dctfhe_host_encrypt_public: null argument");
  if (count == 0) return fail("dctfhe_host_encrypt_public: no phases (count == 0)");
  if (K->calls >= PUB_MAX_CALLS) return fail("dctfhe_host_encrypt_public: this handle's call counter is exhausted");
  const uint64_t call = K->calls++;      // the counter moves even if a later step fails: a draw is never reused
  return guarded("dctfhe_host_encrypt_public", [&]() -> int {
    const size_t N = (size_t)1 << K->logN, groups = (count + N - 1) / N, nmask = groups * N;
    std::vector<uint8_t> u(nmask);
    std::vector<int64_t> e1(nmask), e2(count);
    std::vector<uint64_t> body(nmask);
    std::vector<std::vector<int>> ones(groups);
    public_draws(K, call, count, u.data(), e1.data(), e2.data());
    for (size_t g = 0; g < groups; g++) ones[g] = ones_of(u.data() + g * N, (int)N);
    const uint64_t *A = K->key.data(), *B = A + N;
#pragma omp parallel for schedule(static)
    for (int64_t g = 0; g < (int64_t)groups; g++) {
      const size_t x0 = (size_t)g * N, m = std::min(N, count - x0);
      uint64_t* grp = words_out + (size_t)g * 2 * N;
      uint64_t* cb = body.data() + x0;
      for (size_t c = 0; c < N; c++) { grp[c] = (uint64_t)e1[x0 + c]; cb[c] = 0; }
      negacyclic_acc(grp, A, ones[g].data(), ones[g].size(), (int)N);
      negacyclic_acc(cb, B, ones[g].data(), ones[g].size(), (int)N);
      for (size_t i = 0; i < m; i++) grp[N + i] = cb[i] + (uint64_t)e2[x0 + i] + phases[x0 + i];
    }
    explicit_bzero(u.data(), u.size());
    explicit_bzero(e1.data(), e1.size() * 8);
    explicit_bzero(e2.data(), e2.size() * 8);
    return 0;
  });
}
