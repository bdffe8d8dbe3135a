// kernels.h -- gfx950 kernels of the homomorphic-evaluation engine.
//   K1 conv2d / K2 add, sum-pool, affine      ciphertext streaming, u64 wrap arithmetic (HBM bound)
//   K3 key switch = decompose + integer GEMM  (ks_decompose, ks_gemm)
//   K4+K5+K6 programmable bootstrap           (pbs_kernel: mod-switch, blind rotate, sample extract)
//   K9 keygen / encrypt / decrypt             client side, off the timed path
// Semantics: oracle/tfhe_ref.h (the CPU restatement these are checked against).
#pragma once
#include <hip/hip_runtime.h>
#include "pbs_core.h"
#include "client_shared.h"

namespace dctfhe {

// ------------------------------------------------------------------------------------------ rng
// The generator (ChaCha20 block, rnd64), the stream ids, ks_limbs and the arithmetic of a Gaussian draw live in client_shared.h: the host
// client library (client_host.cpp) draws the same words from the same definitions.
__device__ __forceinline__ int64_t gauss_torus(const rng_key& key, uint64_t stream, uint64_t idx, double sigma) {
  if (sigma <= 0.0) return 0;
  return gauss_torus_words(rnd64(key, stream, 2 * idx), rnd64(key, stream, 2 * idx + 1), sigma);
}

__global__ void k_gen_bits(rng_key key, uint64_t stream, uint8_t* out, int len) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) out[i] = (uint8_t)(rnd64(key, stream, (uint64_t)i) >> 63);
}
__global__ void k_rng_fill(rng_key key, uint64_t stream, uint64_t idx0, uint64_t* out, size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = rnd64(key, stream, idx0 + i);
}

__device__ __forceinline__ uint64_t block_reduce_add(uint64_t v, uint64_t* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv] = v;
  __syncthreads();
  uint64_t s = 0;
  if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); i++) s += red[i];
  return s;  // valid in thread 0
}

// ------------------------------------------------------------------------------------------ client
// one block per ciphertext: a random on [0,dim_eff), b = <a,S> + phase + e
// Rows of `dim` mask words + the body (dim = D: the full-width form; dim < D: the compact wire form -- every mask word from dim_eff on
// is zero anyway).  The draws are indexed as in the full-width form, so both forms of one call hold the same ciphertexts.
__global__ void k_lwe_encrypt(const uint8_t* __restrict__ S, int D, int dim, int dim_eff, const uint64_t* __restrict__ phases,
                              double sigma, rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ cts) {
  __shared__ uint64_t red[16];
  const size_t c = blockIdx.x;
  uint64_t* ct = cts + c * (size_t)(dim + 1);
  uint64_t part = 0;
  for (int j = threadIdx.x; j < dim; j += blockDim.x) {
    const uint64_t a = (j < dim_eff) ? rnd64(pub, stream, c * (uint64_t)(D + 1) + j) : 0;
    ct[j] = a;
    if (S[j]) part += a;
  }
  const uint64_t s = block_reduce_add(part, red);
  if (threadIdx.x == 0) ct[dim] = s + phases[c] + (uint64_t)gauss_torus(sec, stream + 1, c, sigma);
}

// ---- seeded (compressed) forms: the client ships bodies only, the server regenerates the masks from the public key -------------
// rnd64 computes a whole ChaCha20 block for one word; these kernels compute each block once and use all eight of its words.  Rows lie
// `stride` generator indices apart (D + 1 for an LWE ciphertext), so a block may straddle two rows: each block index is mapped back to
// (row, word) and words from dim_eff on (the gap of a compact row, the body's index) are skipped.

// client: the bodies of k_lwe_encrypt (the same ciphertexts, for equal keys and stream) without writing a mask word.  One workgroup per
// ciphertext; the partial block shared with the previous row is computed by both rows (one block in dim_eff / 8).
__global__ void k_lwe_encrypt_seeded(const uint8_t* __restrict__ S, int D, int dim_eff, const uint64_t* __restrict__ phases, double sigma,
                                     rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ bodies) {
  __shared__ uint64_t red[16];
  const size_t c = blockIdx.x;
  const uint64_t base = c * (uint64_t)(D + 1), b_lo = base >> 3, b_hi = (base + dim_eff - 1) >> 3;
  uint64_t part = 0;
  for (uint64_t b = b_lo + threadIdx.x; b <= b_hi; b += blockDim.x) {
    uint32_t o[16];
    chacha20_block(pub, stream, b, o);
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const int64_t j = (int64_t)(8 * b + w - base);
      if (j >= 0 && j < dim_eff && S[j]) part += (uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32);
    }
  }
  const uint64_t s = block_reduce_add(part, red);
  if (threadIdx.x == 0) bodies[c] = s + phases[c] + (uint64_t)gauss_torus(sec, stream + 1, c, sigma);
}

// server: rows [count][L] from their bodies.  Row c (generator row row0 + c) gets mask word j = rnd64(key, stream, (row0 + c) stride + j)
// & and_mask for j < dim_eff, zeros up to L - nb, and its nb body words from bodies[c][nb].  Seeded inputs: stride D + 1, nb = 1;
// key-switch keys: stride n + 1, the grid mask; bootstrap-key rows: stride kN = dim_eff, nb = N.  Needs stride >= 8 (a block touches at
// most two rows) and dim_eff <= min(stride, L - nb).  Thread = one block; a block shared by two rows belongs to the earlier one, which
// writes the later row's words too, so every block is computed once.
__global__ void k_seeded_expand(rng_key key, uint64_t stream, uint64_t row0, uint64_t stride, int dim_eff, uint64_t and_mask,
                                const uint64_t* __restrict__ bodies, int nb, size_t count, size_t L, uint64_t* __restrict__ out) {
  const size_t bpr = (size_t)(dim_eff + 7) / 8 + 1, nblk = count * bpr;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nblk; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i / bpr, k = i % bpr;
    const uint64_t base = (row0 + c) * stride, b = (base >> 3) + k;
    if (b > (base + dim_eff - 1) >> 3) continue;
    if (k == 0 && c > 0 && ((base - stride + dim_eff - 1) >> 3) == b) continue;   // the previous row's last block
    uint32_t o[16];
    chacha20_block(key, stream, b, o);
#pragma unroll
    for (int w = 0; w < 8; w++) {
      int64_t j = (int64_t)(8 * b + w - base);
      int64_t cc = (int64_t)c;
      if (j < 0) { j += (int64_t)stride; cc--; }
      else if (j >= (int64_t)stride) { j -= (int64_t)stride; cc++; }
      if (cc >= 0 && cc < (int64_t)count && j < dim_eff) out[(size_t)cc * L + j] = ((uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32)) & and_mask;
    }
  }
  const size_t tail = L - (size_t)dim_eff, ntail = count * tail;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ntail; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i / tail, w = (size_t)dim_eff + i % tail;
    out[c * L + w] = w >= L - nb ? bodies[c * nb + (w - (L - nb))] : 0;
  }
}

__global__ void k_lwe_phase(const uint8_t* __restrict__ S, int dim, const uint64_t* __restrict__ cts, uint64_t* __restrict__ phases) {
  __shared__ uint64_t red[16];
  const size_t c = blockIdx.x;
  const uint64_t* ct = cts + c * (size_t)(dim + 1);
  uint64_t part = 0;
  for (int j = threadIdx.x; j < dim; j += blockDim.x)
    if (S[j]) part += ct[j];
  const uint64_t s = block_reduce_add(part, red);
  if (threadIdx.x == 0) phases[c] = ct[dim] - s;
}

// ------------------------------------------------------------------------------------------ keygen
// key-switch key: one block per row (i, lev): LWE_s(S_i * 2^(64 - betak (lev+1)))
// The key lives on a COARSE TORUS GRID of 2^-(8 limbs): its mask words are drawn on that grid and the body is rounded to it (a rounding
// of 2^-(8 limbs) / sqrt(12), far below the row's noise sigma: dctfhe.hip ks_limbs() picks limbs >= (lk betak + 6) / 8).  A key-switch
// output only ever meets a mod switch to 2N <= 2^14 levels under a noise of 2^-5 .. 2^-11: the low 32-48 bits of a 64-bit key word
// carried nothing, and the matrix-core GEMM spent half to three quarters of its work multiplying them (round 2: 8 byte limbs per word).
__global__ void k_ksk_gen(const uint8_t* __restrict__ S, const uint8_t* __restrict__ s, int n, int lk, int betak, int limbs,
                          double sigma, rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ ksk) {
  __shared__ uint64_t red[16];
  const size_t row = blockIdx.x;
  const int i = (int)(row / lk), lev = (int)(row % lk);
  uint64_t* dst = ksk + row * (size_t)(n + 1);
  const int drop = 64 - 8 * limbs;                                   // low bits that are not stored (0 for limbs = 8)
  const uint64_t mask = drop ? ~0ULL << drop : ~0ULL, half = drop ? 1ULL << (drop - 1) : 0;
  uint64_t part = 0;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const uint64_t a = rnd64(pub, stream, row * (uint64_t)(n + 1) + j) & mask;
    dst[j] = a;
    if (s[j]) part += a;
  }
  const uint64_t sum = block_reduce_add(part, red);
  if (threadIdx.x == 0) {
    uint64_t b = sum + (uint64_t)gauss_torus(sec, stream + 1, row, sigma);
    if (S[i]) b += 1ULL << (64 - betak * (lev + 1));
    dst[n] = (b + half) & mask;
  }
}
// any key word off the 2^-(8 limbs) grid?  (an imported key must be what k_ksk_gen makes: the limb form drops the low bytes unseen)
__global__ void k_ksk_off_grid(const uint64_t* __restrict__ ksk, size_t words, int limbs, int* __restrict__ flag) {
  const uint64_t low = limbs >= 8 ? 0 : ~(~0ULL << (64 - 8 * limbs));
  int bad = 0;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < words; x += (size_t)gridDim.x * blockDim.x) bad |= (ksk[x] & low) != 0;
  if (bad) atomicOr(flag, 1);
}

// secret of the two-bit blind rotation: per pair (s1, s2) the three products s1(1-s2), (1-s1)s2, s1 s2
__global__ void k_pair_secret(const uint8_t* __restrict__ s, int n, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (2 * i + 1 >= n) return;
  const uint8_t a = s[2 * i], b = s[2 * i + 1];
  out[3 * i] = a && !b; out[3 * i + 1] = !a && b; out[3 * i + 2] = a && b;
}

// What every bootstrap-key row starts from, whichever form it is stored in: the noise draw into the body polynomial B, then per mask
// polynomial j < k the draw into LDS (A; a ChaCha block, eight words, per thread: N is a multiple of 8, so a polynomial starts a block)
// and B += A * S_j (negacyclic).  grow is the global row id: the randomness does not depend on chunking.  masks: where the k mask
// polynomials go ([k][N]), or nullptr for a row that keeps its body only.
__device__ __forceinline__ void bsk_row_zero(const uint8_t* __restrict__ S_glwe, uint64_t grow, int k, int N, double sigma, const rng_key& pub,
                                             const rng_key& sec, uint64_t stream, uint64_t* __restrict__ A, uint64_t* __restrict__ B,
                                             uint64_t* __restrict__ masks) {
  for (int c = threadIdx.x; c < N; c += blockDim.x)
    B[c] = (uint64_t)gauss_torus(sec, stream + 1, grow * (uint64_t)N + c, sigma);
  for (int j = 0; j < k; j++) {
    __syncthreads();
    const uint64_t blk0 = ((grow * (uint64_t)k + j) * (uint64_t)N) >> 3;
    for (int q = threadIdx.x; q < N / 8; q += blockDim.x) {
      uint32_t o[16];
      chacha20_block(pub, stream, blk0 + q, o);
#pragma unroll
      for (int w = 0; w < 8; w++) {
        const uint64_t a = (uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32);
        A[8 * q + w] = a;
        if (masks) masks[(size_t)j * N + 8 * q + w] = a;
      }
    }
    __syncthreads();
    const uint8_t* Sj = S_glwe + (size_t)j * N;
    for (int c = threadIdx.x; c < N; c += blockDim.x) {
      uint64_t acc = 0;
      for (int m = 0; m < N; m++) {
        if (!Sj[m]) continue;  // uniform branch
        const int src = c - m;
        acc += (src >= 0) ? A[src] : (uint64_t)0 - A[src + N];
      }
      B[c] += acc;
    }
  }
}

// bootstrap key, standard domain, rows [i0, i0+ni) x rows_per_bit: GLWE(0) + s_i * gadget.
// One block per row; the mask polynomial is parked in LDS while the body accumulates A * S.
__global__ void k_bsk_gen_std(const uint8_t* __restrict__ s_small, const uint8_t* __restrict__ S_glwe, int i0, int k, int N, int l,
                              int beta, double sigma, rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int rows = (k + 1) * l;
  const int i = i0 + (int)(blockIdx.x / rows), r = (int)(blockIdx.x % rows);
  uint64_t* row = out + (size_t)blockIdx.x * (k + 1) * N;
  bsk_row_zero(S_glwe, (uint64_t)i * rows + r, k, N, sigma, pub, sec, stream, reinterpret_cast<uint64_t*>(smem_raw), row + (size_t)k * N, row);
  __syncthreads();
  if (threadIdx.x == 0 && s_small[i]) {
    const int p = r / l, lev = r % l;
    row[(size_t)p * N] += 1ULL << (64 - beta * (lev + 1));
  }
}

// the same rows in BODY FORM, bodies only ([ni * rows][N]): the masks stay the pure draws of `pub` (k_seeded_expand rebuilds them), so
// the s_i * gadget term that k_bsk_gen_std adds to mask polynomial p < k moves into the body as - s_i g S_p (same phase, same noise
// draw); rows with p = k are k_bsk_gen_std's bodies bit for bit.  Covers the pair secret of unroll 2 like k_bsk_gen_std (s_small = the
// derived bits).  One block per row.
__global__ void k_bsk_gen_bodies(const uint8_t* __restrict__ s_small, const uint8_t* __restrict__ S_glwe, int i0, int k, int N, int l,
                                 int beta, double sigma, rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int rows = (k + 1) * l;
  const int i = i0 + (int)(blockIdx.x / rows), r = (int)(blockIdx.x % rows);
  uint64_t* B = out + (size_t)blockIdx.x * N;
  bsk_row_zero(S_glwe, (uint64_t)i * rows + r, k, N, sigma, pub, sec, stream, reinterpret_cast<uint64_t*>(smem_raw), B, nullptr);
  if (!s_small[i]) return;
  const int p = r / l, lev = r % l;
  const uint64_t g = 1ULL << (64 - beta * (lev + 1));
  if (p == k) {
    if (threadIdx.x == 0) B[0] += g;       // thread 0 owns coefficient 0 in the loops above
  } else {
    const uint8_t* Sp = S_glwe + (size_t)p * N;
    for (int c = threadIdx.x; c < N; c += blockDim.x)
      if (Sp[c]) B[c] -= g;
  }
}

// standard-domain key polynomials -> Fourier device layout; GROUPS polynomials per block
template <int LOGN, int P, int GROUPS>
__global__ void __launch_bounds__((fft_geom<LOGN - 1, P>::T * GROUPS))
k_bsk_fourier(const uint64_t* __restrict__ polys, size_t npoly, const cplx* __restrict__ tw_g, cplx* __restrict__ out) {
  using F = fft_geom<LOGN - 1, P>;
  constexpr int T = F::T, N = 1 << LOGN, M = N / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  cplx* tw = reinterpret_cast<cplx*>(smem_raw);
  cplx* exch_all = tw + F::TW_ELEMS;
  for (int x = threadIdx.x; x < F::TW_ELEMS; x += blockDim.x) tw[x] = tw_g[x];
  __syncthreads();
  const int g = threadIdx.x / T, t = threadIdx.x % T;
  size_t q = (size_t)blockIdx.x * GROUPS + g;
  if (q >= npoly) q = npoly - 1;  // redundant work keeps every thread on the barriers
  cplx* exch = exch_all + (size_t)g * F::EXCH_ELEMS;
  key_poly_to_fourier<LOGN, P>(polys + q * N, out + q * M, t, tw, exch, [] { __syncthreads(); }, [] { __builtin_amdgcn_wave_barrier(); });
}

// ------------------------------------------------------------------------------------------ K3 key switch
// Step 1: digits of (ct << shift) for every mask word, offset to unsigned: dig' = dig + B/2 in [0,B).
// Layout digits[c][i*lk + lev] (u8).  Also copies the (shifted) body.
// Only the first Deff mask words are decomposed (digits [count][Deff*lk]): the caller knows the rest to be zero (nested
// keys: a ciphertext that came out of a ring of dimension kN <= Deff has a zero tail), and a zero word contributes nothing.
// Where ciphertext c comes from is a row source: word(c, i) is its mask word i < Deff, body(c) its body.

// the ciphertexts are the rows themselves (stride L words, body at L-1)
struct ks_src_rows {
  const uint64_t* cts; size_t L;
  __device__ __forceinline__ uint64_t word(size_t c, int i) const { return cts[c * L + i]; }
  __device__ __forceinline__ uint64_t body(size_t c) const { return cts[c * L + L - 1]; }
};
// the difference of two rows, for the pairwise maxima of a max pool: ciphertext c is rows[ia[c]] - rows[ib[c]] (rows of stride L, the
// first Deff mask words meaningful) -- no difference tensor is ever written
struct ks_src_diff {
  const uint64_t* rows; size_t L; const int32_t *ia, *ib;
  __device__ __forceinline__ uint64_t word(size_t c, int i) const { return rows[(size_t)ia[c] * L + i] - rows[(size_t)ib[c] * L + i]; }
  __device__ __forceinline__ uint64_t body(size_t c) const { return rows[(size_t)ia[c] * L + L - 1] - rows[(size_t)ib[c] * L + L - 1]; }
};
// the sum of two row sets, for the second look-up of a parity-split site (7-bit tables): ciphertext c is rows_a[c] + rows_b[c] -- the
// working ciphertext (rows of stride La) plus the parity bootstrap's output (rows of stride Lb, whose db stored mask words hold a ring and
// zeros; a word beyond them counts as zero) -- so the copy with the parity in its padding bit is never written
struct ks_src_sum {
  const uint64_t* rows_a; size_t La; const uint64_t* rows_b; size_t Lb, db;
  __device__ __forceinline__ uint64_t word(size_t c, int i) const { return rows_a[c * La + i] + ((size_t)i < db ? rows_b[c * Lb + i] : 0); }
  __device__ __forceinline__ uint64_t body(size_t c) const { return rows_a[c * La + La - 1] + rows_b[c * Lb + Lb - 1]; }
};

// the lk balanced base-2^betak digits of v, rounded at 2^-(lk betak), most significant first, each offset by half a base
__device__ __forceinline__ void ks_split_digits(uint64_t v, int lk, int betak, uint8_t* __restrict__ dst) {
  const int half = 1 << (betak - 1), tot = lk * betak;
  uint64_t xx = (v + (1ULL << (63 - tot))) >> (64 - tot);
  const uint64_t B = 1ULL << betak, mask = B - 1;
  uint64_t carry = 0;
  for (int lev = lk - 1; lev >= 0; lev--) {
    uint64_t d = (xx & mask) + carry;
    xx >>= betak;
    int dv;
    if (d >= (uint64_t)half) { dv = (int)d - (int)B; carry = 1; } else { dv = (int)d; carry = 0; }
    dst[lev] = (uint8_t)(dv + half);
  }
}

// lanes run over consecutive words of a ciphertext
template <class Src>
__global__ void k_ks_decompose(Src src, size_t count, int Deff, int shift, uint64_t body_add, int lk, int betak, uint8_t* __restrict__ digits,
                               uint64_t* __restrict__ bodies) {
  const size_t total = count * (size_t)Deff;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
    const size_t c = x / Deff;
    const int i = (int)(x % Deff);
    ks_split_digits(src.word(c, i) << shift, lk, betak, digits + (c * (size_t)Deff + i) * lk);
    if (i == 0) bodies[c] = (src.body(c) << shift) + body_add;      // the affine step of a look-up without rounding steps rides along
  }
}

// Step 2: out[c][j] = body_c*[j==n] - sum_r (dig'[c][r] - B/2) * ksk[r][j]
//       = body_c*[j==n] + (B/2) * colsum[j] - sum_r dig'[c][r] * ksk[r][j],   colsum[j] = sum_r ksk[r][j].
// Block: CT ciphertexts x 256 columns; digits are wave-uniform (scalar loads), the key is read
// once per block -- coalesced 8 B per lane -- and reused for CT ciphertexts.
template <int CT>
__global__ void __launch_bounds__(256)
k_ks_gemm(const uint8_t* __restrict__ digits, const uint64_t* __restrict__ bodies, size_t count, int R /* D*lk */,
          const uint64_t* __restrict__ ksk, const uint64_t* __restrict__ colsum, int n, int betak,
          uint64_t* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const size_t c0 = (size_t)blockIdx.y * CT;
  const bool live = j <= n;
  const int jj = live ? j : n;
  uint64_t acc[CT];
#pragma unroll
  for (int c = 0; c < CT; c++) acc[c] = 0;
  const uint8_t* dbase = digits + c0 * (size_t)R;
  for (int r = 0; r < R; r += 4) {
    uint64_t kv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) kv[u] = ksk[(size_t)(r + u) * (n + 1) + jj];
#pragma unroll
    for (int c = 0; c < CT; c++) {
      const size_t cc = (c0 + c < count) ? (size_t)c : 0;
      const uint32_t d4 = *reinterpret_cast<const uint32_t*>(dbase + cc * (size_t)R + r);  // wave-uniform
#pragma unroll
      for (int u = 0; u < 4; u++) acc[c] += (uint64_t)((d4 >> (8 * u)) & 0xFF) * kv[u];
    }
  }
  if (!live) return;
  const uint64_t fix = ((uint64_t)1 << (betak - 1)) * colsum[j];
#pragma unroll
  for (int c = 0; c < CT; c++) {
    if (c0 + c >= count) break;
    out[(c0 + c) * (size_t)(n + 1) + j] = (j == n ? bodies[c0 + c] : 0) + fix - acc[c];
  }
}

// ---- key switch on the matrix cores -----------------------------------------------------------------
// out[c][j] = fix[j] - sum_r dig'[c][r] * ksk[r][j] is a GEMM with a tiny-integer left operand (digits in
// [0, 2^betak)) and a u64 right operand.  The key is re-expressed once, at keygen, as 8 signed byte limbs
// (ksk = sum_k s_k 2^(8k), s_k in [-128,127], carries propagated), stored K-contiguous per output column:
// kskT[(j*8 + k) * R + r].  Then C[c][j*8+k] = sum_r dig'[c][r] * s_k[r][j] is an i8 x i8 -> i32 GEMM for
// v_mfma_i32_32x32x32_i8 (|C| <= R * 127 * 128 < 2^31 for R <= 2^17), and out = fix - sum_k C_k << 8k (mod 2^64).
// Only the TOP `limbs` byte limbs of a key word are stored (the key sits on the 2^-(8 limbs) grid: the others are zero and carry nothing
// up): column j*limbs + k' holds limb 8 - limbs + k'.
__global__ void k_ksk_to_limbs(const uint64_t* __restrict__ ksk, int R, int n, int limbs, int ncol_pad /* limbs*(n+1) rounded up */, int8_t* __restrict__ kskT) {
  const size_t total = (size_t)R * (ncol_pad / limbs);
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
    const size_t r = x % R;
    const size_t j = x / R;
    uint64_t v = (j <= (size_t)n) ? ksk[r * (size_t)(n + 1) + j] : 0;
    v >>= 64 - 8 * limbs;                                              // (limbs = 8: a shift by 0)
    for (int k = 0; k < limbs; k++) {
      int b = (int)(v & 0xFF);
      v >>= 8;
      if (b >= 128) { b -= 256; v += 1; }
      kskT[(j * limbs + k) * (size_t)R + r] = (int8_t)b;
    }
  }
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Block: 128 ciphertexts x 128 limb columns (16 output words), K step 64, 4 waves each owning a 64 x 64 quadrant
// (2 x 2 MFMA tiles).  Both operands are K-contiguous, so a lane's 16-byte fragment is one ds_read_b128 and
// the A and B fragments of a lane cover the same 16 k's whatever order the hardware walks them in.
template <int LIMBS>        // byte limbs stored per key word: 2, 4 or 8 (the top ones)
__global__ void __launch_bounds__(256)
k_ks_mfma(const uint8_t* __restrict__ digits, const uint64_t* __restrict__ bodies, size_t count, int R /* rows used: Deff*lk */,
          const int8_t* __restrict__ kskT, int ldk /* row stride of kskT: D*lk */, int ncol_pad, const uint64_t* __restrict__ colsum /* over the R rows used */,
          int n, int betak, uint64_t* __restrict__ out) {
  constexpr int BM = 128, BN = 128, BK = 128, LD = BK + 16;    // +16 B per row: rows land on different bank groups
  constexpr int SEG = BK / 16, RPP = 256 / SEG, NU = BM / RPP;  // 16-byte segments per row, rows staged per pass, passes
  __shared__ __attribute__((aligned(16))) int8_t As[BM * LD];
  __shared__ __attribute__((aligned(16))) int8_t Bs[BN * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order (1-D grid of 8 * cpx * nrb workgroups; workgroups b and b + 8 share an XCD and its 4 MB L2): every XCD
  // owns a strip of cpx column blocks of the key and walks the ciphertext row blocks with the columns fastest, so the ~32 tiles
  // an XCD runs at a time are ~4 row blocks x its 7 column blocks -- each K-slice of the digits serves 7 tiles out of L2 and each
  // K-slice of the key 4-5.  (Round 1: x = column, y = row over all XCDs: the 83 MB limb key was re-read from HBM once per row
  // block, 10.6 GB per launch.)
  const int ncb = ncol_pad / BN, nrb = (int)((count + BM - 1) / BM), cpx = (ncb + 7) / 8;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int cb = xcd * cpx + slot % cpx, rb = slot / cpx;
  if (cb >= ncb || rb >= nrb) return;
  const size_t c0 = (size_t)rb * BM;
  const size_t col0 = (size_t)cb * BN;
  v16i acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[a][b][e] = 0;
  // staging assignment: NU x 16 B of A and NU x 16 B of B per thread per K step (K step 128: half the barriers of 64; every
  // shipped K = Deff * lk is a multiple of 128 or falls back to the remainder handling below)
  const int srow = tid / SEG, sseg = (tid % SEG) * 16;
  const uint8_t* a_src[NU];
  const int8_t* b_src[NU];
#pragma unroll
  for (int u = 0; u < NU; u++) {
    size_t c = c0 + srow + RPP * u;
    if (c >= count) c = count - 1;
    a_src[u] = digits + c * (size_t)R + sseg;
    b_src[u] = kskT + (col0 + srow + RPP * u) * (size_t)ldk + sseg;
  }
  const int fr = lane & 31, fh = (lane >> 5) * 16;
  // software pipeline: the global loads of K-step k0 + BK are issued before the matrix instructions of step k0 and land under
  // them (round 1 loaded, waited, stored, computed: every K-step exposed a global round trip)
  // R is a multiple of 64 (checked by the host); a trailing half step reads zeros for its upper 64 bytes
  const v4i zero4 = {0, 0, 0, 0};
  auto fetch = [&](int k0, v4i* ga, v4i* gb) {
    const bool live = k0 + sseg < R;
#pragma unroll
    for (int u = 0; u < NU; u++) {
      ga[u] = live ? *reinterpret_cast<const v4i*>(a_src[u] + k0) : zero4;
      gb[u] = live ? *reinterpret_cast<const v4i*>(b_src[u] + k0) : zero4;
    }
  };
  v4i ga[NU], gb[NU];
  fetch(0, ga, gb);
  for (int k0 = 0; k0 < R; k0 += BK) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NU; u++) {
      *reinterpret_cast<v4i*>(&As[(srow + RPP * u) * LD + sseg]) = ga[u];
      *reinterpret_cast<v4i*>(&Bs[(srow + RPP * u) * LD + sseg]) = gb[u];
    }
    __syncthreads();
    if (k0 + BK < R) fetch(k0 + BK, ga, gb);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      v4i fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; a++) fa[a] = *reinterpret_cast<const v4i*>(&As[(wm * 64 + a * 32 + fr) * LD + kk + fh]);
#pragma unroll
      for (int b = 0; b < 2; b++) fb[b] = *reinterpret_cast<const v4i*>(&Bs[(wn * 64 + b * 32 + fr) * LD + kk + fh]);
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
  }
  // epilogue: C tile layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); limb k' = col % LIMBS stands for 2^(8 (8 - LIMBS + k'))
  static_assert(LIMBS == 2 || LIMBS == 4 || LIMBS == 8, "limb groups are folded with lane shuffles");
  const int limb = lane & (LIMBS - 1);
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const size_t word = (col0 + wn * 64 + b * 32 + (lane & 31)) / LIMBS;     // output word j of this lane's column
#pragma unroll
      for (int e = 0; e < 16; e++) {
        uint64_t v = (uint64_t)(int64_t)acc[a][b][e] << (8 * (8 - LIMBS + limb));
        v += __shfl_xor(v, 1);
        if constexpr (LIMBS >= 4) v += __shfl_xor(v, 2);
        if constexpr (LIMBS >= 8) v += __shfl_xor(v, 4);
        const size_t c = c0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (limb == 0 && c < count && word <= (size_t)n) {
          const uint64_t fix = ((uint64_t)1 << (betak - 1)) * colsum[word] + (word == (size_t)n ? bodies[c] : 0);
          out[c * (size_t)(n + 1) + word] = fix - v;
        }
      }
    }
}

__global__ void k_ksk_colsum(const uint64_t* __restrict__ ksk, int R, int n, uint64_t* __restrict__ colsum) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  uint64_t s = 0;
  for (int r = 0; r < R; r++) s += ksk[(size_t)r * (n + 1) + j];
  colsum[j] = s;
}

// Centred mod switch (semantics: oracle/tfhe_ref.c ref_ms_center).  The bootstrap rounds every word of the small ciphertext to 2N
// levels; the evaluator knows each mask word's rounding remainder and that a key bit is 1 half of the time, so half the sum of the
// remainders comes off the body first: the mod-switch error keeps sum_i (s_i - 1/2) e_i, half the variance.  One wave per ciphertext, in
// place on the key switch's output, ~6.5 KB read per ciphertext.
__global__ void __launch_bounds__(256) k_ms_center(uint64_t* __restrict__ small, size_t count, int n, int logN) {
  const size_t c = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= count) return;
  uint64_t* ct = small + c * (size_t)(n + 1);
  const int sh = 63 - logN;
  int64_t part = 0;
  for (int i = lane; i < n; i += 64) {
    const uint64_t a = ct[i];
    const uint64_t at = ((a >> (sh - 1)) + 1) >> 1;
    part += (int64_t)(a - (at << sh));
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) ct[n] -= (uint64_t)(part >> 1);
}

// ---- packed results: key-switched ciphertexts as 16-bit rows ---------------------------------------
// A result only has to survive the decode margin 2^-(out_bits + 3), so once it is key-switched to a small key the top 16 bits of every
// word are all the client needs: word -> (word + 2^47) >> 48, round to nearest on the 2^-16 grid, a tie goes up, a carry out of the top
// wraps to 0 (the u64 sum wraps).
__device__ __forceinline__ uint64_t round16(uint64_t v) { return (v + (1ULL << 47)) >> 48; }

// small [words] u64 -> rows [words] u16.  A row has n + 1 words, odd for even n, so rows are not 4-byte aligned: lanes run over the FLAT
// array, four consecutive results each, one 8-byte store per lane; the words % 4 results at the end go out as single u16 stores.
__global__ void k_pack16(const uint64_t* __restrict__ small, size_t words, uint16_t* __restrict__ rows) {
  const size_t quads = words / 4;
  uint64_t* __restrict__ out4 = reinterpret_cast<uint64_t*>(rows);
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
    const uint64_t* p = small + 4 * q;
    out4[q] = round16(p[0]) | (round16(p[1]) << 16) | (round16(p[2]) << 32) | (round16(p[3]) << 48);
  }
  const size_t tail = 4 * quads + threadIdx.x;
  if (blockIdx.x == 0 && tail < words) rows[tail] = (uint16_t)round16(small[tail]);
}

// client: phase of a packed row under the first n bits of the small key, on the 16-bit torus: (row[n] - sum_{j<n} s_j row[j]) mod 2^16,
// returned as phase16 << 48.  One wave per row as in k_ms_center: lane-strided u16 loads, 32-bit partial sums (wrapping mod 2^32 keeps
// the low 16 bits exact), butterfly reduction.
__global__ void __launch_bounds__(256) k_phase16(const uint8_t* __restrict__ s, int n, const uint16_t* __restrict__ rows, size_t count,
                                                 uint64_t* __restrict__ phases) {
  const size_t c = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= count) return;
  const uint16_t* row = rows + c * (size_t)(n + 1);
  uint32_t part = 0;
  for (int j = lane; j < n; j += 64)
    if (s[j]) part += row[j];
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) phases[c] = (uint64_t)(((uint32_t)row[n] - part) & 0xFFFFu) << 48;
}

// ---- margin audit: how far from its box centre every bootstrap decides ------------------------------------
// The bootstrap rounds each word of a small ciphertext to the 2N levels of its ring (pbs_core.h: ((x >> msh) + 1) >> 1 with msh =
// 62 - logN, the expression k_ms_center uses) and reads the box of G = 2^(logN - w) levels its switched phase lands in; boxes are
// centred on the multiples of G (testvec_coeff: half a box of rotation).  margin_error is the signed distance, in levels, of a
// switched phase from the centre of its box: in [-h, h), h = G / 2 >= 1.  While a run is correct this is the noise of the decision.
HD uint32_t margin_level(uint64_t x, int logN) { return (uint32_t)(((x >> (62 - logN)) + 1) >> 1); }
HD int32_t margin_error(uint32_t phase_levels, int logN, int w) {
  const uint32_t G = 1u << (logN - w), h = G >> 1;
  return (int32_t)((phase_levels + h) & (G - 1)) - (int32_t)h;
}
HD int margin_bin(int32_t e, int32_t h) { const int32_t a = e < 0 ? -e : e, b = 16 * a / h; return b < 15 ? b : 15; }
// the layout of dctfhe_margin_stats (include/dctfhe.h; dctfhe.hip asserts it), with the accumulated fields as the atomics take them
struct margin_slot {
  int32_t op, entry, tier, table_bits, half_box, max_abs;
  unsigned long long count, sum, sum_sq, hist[16];
};
constexpr int MARGIN_WORDS = 3 + 16;      // count, sum, sum_sq, hist[16]: the words a block adds to a slot

// The probe: `count` small ciphertexts of n + 1 words under the first n key bytes of s (0 / 1), a table of w input bits on a ring of
// 2^logN.  One wave per ciphertext as in k_ms_center and k_phase16 -- lane-strided loads, 32-bit partial sums (the phase is taken mod
// 2N, a power of two), butterfly reduction, after which every lane holds the phase -- but a wave walks ciphertexts grid-strided and
// keeps its statistics in registers: lane b < 16 counts histogram bin b, the sums are wave-uniform.  The four waves of a block meet in
// LDS and the block issues one set of integer atomics on the slot, so the result does not depend on the order of anything.  No thread
// leaves before the barrier.  err (optional): e per ciphertext; slot (optional): the accumulated statistics.
__global__ void __launch_bounds__(256) k_margin_probe(const uint8_t* __restrict__ s, const uint64_t* __restrict__ small, size_t count, int n,
                                                      int logN, int w, int32_t* __restrict__ err, margin_slot* __restrict__ slot) {
  __shared__ unsigned long long part[4][MARGIN_WORDS];
  __shared__ int part_max[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t h = (int32_t)1 << (logN - w - 1);
  unsigned long long cnt = 0, sum = 0, sq = 0, bin_count = 0;
  int32_t mx = 0;
  for (size_t c = (size_t)blockIdx.x * 4 + wave; c < count; c += (size_t)gridDim.x * 4) {
    const uint64_t* ct = small + c * (size_t)(n + 1);
    uint32_t acc = 0;
    for (int i = lane; i < n; i += 64)
      if (s[i]) acc += margin_level(ct[i], logN);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    const int32_t e = margin_error(margin_level(ct[n], logN) - acc, logN, w);
    if (err && lane == 0) err[c] = e;
    const int32_t a = e < 0 ? -e : e;
    cnt++;
    sum += (unsigned long long)(long long)e;
    sq += (unsigned long long)((long long)e * e);
    mx = a > mx ? a : mx;
    if (lane == margin_bin(e, h)) bin_count++;
  }
  if (lane == 0) { part[wave][0] = cnt; part[wave][1] = sum; part[wave][2] = sq; part_max[wave] = mx; }
  if (lane < 16) part[wave][3 + lane] = bin_count;
  __syncthreads();
  if (!slot) return;
  if (threadIdx.x < MARGIN_WORDS) {
    const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v) atomicAdd(&slot->count + threadIdx.x, v);
  } else if (threadIdx.x == MARGIN_WORDS) {
    const int m = max(max(part_max[0], part_max[1]), max(part_max[2], part_max[3]));
    if (m) atomicMax(&slot->max_abs, m);
  }
}

// ---- ring-packed results: a batch's small ciphertexts in ONE GLWE ciphertext per N results ---------------
// Ring key Z(X) = sum_c S[c] X^c, the first N bits of the big key (k = 1, the nested-prefix rule of every tier).  The packing key has one
// GLWE row (A, B = A Z + E + s_j g_lev X^0) per small-key bit j and level lev, g_lev = 2^(64 - beta (lev + 1)); the server holds it
// expanded, [n_max][l][2][N].  A group of m <= N small ciphertexts (a_i, b_i) packs to
//     acc = (0, sum_i b_i X^i) - sum_i sum_j sum_lev dig_lev(a_ij) X^i PK[j][lev]            (negacyclic, mod 2^64)
// whose phase has result i's phase at coefficient i: the message of a key row is a constant polynomial, so nothing else lands there.

// the packing key's bodies [n_max * l][N]: row r = j l + lev is the p = k row of a k = 1 bootstrap key (bsk_row_zero: noise draw, mask
// draw into LDS, B += A Z) with the gadget term on coefficient 0.  Mask word c of row r is rnd64(pub, stream, r N + c), its noise
// gauss_torus(sec, stream + 1, r N + c): k_seeded_expand rebuilds the masks (stride N, N mask words, N body words).  One block per row.
__global__ void k_ring_key_gen(const uint8_t* __restrict__ s_small, const uint8_t* __restrict__ S_big, int N, int l, int beta, double sigma,
                               rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int j = (int)(blockIdx.x / l), lev = (int)(blockIdx.x % l);
  uint64_t* B = out + (size_t)blockIdx.x * N;
  bsk_row_zero(S_big, (uint64_t)blockIdx.x, 1, N, sigma, pub, sec, stream, reinterpret_cast<uint64_t*>(smem_raw), B, nullptr);
  if (threadIdx.x == 0 && s_small[j]) B[0] += 1ULL << (64 - beta * (lev + 1));      // thread 0 owns coefficient 0 in the loops above
}

// digits of the mask words of `count` small ciphertexts (rows of n + 1 words; groups of N = 2^logN in order), TRANSPOSED:
// dig[((g n + j) l + lev) N + i] is level lev of mask word j of result i of group g, so k_ring_pack reads a key row's digits contiguously.
// The closest-representable signed decomposition of oracle/tfhe_ref.c ref_decompose: digits in [-B/2, B/2), the top carry dropped.
// Slots of a partial last group beyond its results are left unwritten (k_ring_pack never reads them).
__global__ void k_ring_digits(const uint64_t* __restrict__ small, size_t count, int n, int logN, int l, int beta, int32_t* __restrict__ dig) {
  const size_t N = (size_t)1 << logN, groups = (count + N - 1) >> logN, total = groups * (size_t)n * N;
  const int tot = l * beta;
  const uint64_t B = 1ULL << beta, half = B >> 1, mask = B - 1;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
    const size_t i = x & (N - 1), gj = x >> logN, g = gj / n, j = gj % n, c = g * N + i;
    if (c >= count) continue;
    const uint64_t v = small[c * (size_t)(n + 1) + j];
    uint64_t q = (v + (1ULL << (63 - tot))) >> (64 - tot), carry = 0;
    for (int lev = l - 1; lev >= 0; lev--) {
      const uint64_t d = (q & mask) + carry;
      q >>= beta;
      carry = d >= half;
      dig[(gj * l + lev) * N + i] = (int32_t)(carry ? (int64_t)d - (int64_t)B : (int64_t)d);
    }
  }
}

// One workgroup per (group g, component: 0 mask / 1 body, tile of RING_TILE output coefficients).  Per key row r < n l the row's
// polynomial (the window of it the tile reads, all N u64 in a full group) and the group's digits of that row (m i32) are staged in LDS; thread (c = tile coefficient, part = slot residue)
// accumulates acc[c] -= d[i] (+-K[(c - i) mod N]) in u64 over its slots i = part, part + PARTS, ..., the sign flipped where c < i (X^N = -1).
// A half-wave reads 32 consecutive key words (conflict-free 8-byte LDS reads) and one digit (a broadcast).  Epilogue: the parts are summed
// through LDS, the body term b_c joins component 1, and the word goes out rounded as k_pack16 does: the N mask words of the group, then
// its first m body words.  Groups before the last are full, so group g starts at u16 index 2 g N.
constexpr int RING_TILE = 32, RING_PARTS = 256 / RING_TILE;
// One key row's share of a tile (k_ring_pack, k_pk_encrypt): the window [first, first + span) of the row's polynomial and the row's m
// multipliers go to LDS, then the thread (coefficient c, slot residue part) takes acc -= mul[i] (+-K[(c - i) mod N]) over its slots.
// Every thread of the workgroup calls it: two barriers.
__device__ __forceinline__ uint64_t ring_tile_row(const uint64_t* __restrict__ krow, const int32_t* __restrict__ mrow, int N, int m, int first, int span,
                                                  int c, int part, uint64_t* __restrict__ K, int32_t* __restrict__ d, uint64_t acc) {
  __syncthreads();
  for (int x = threadIdx.x; x < span; x += 256) { const int idx = (first + x) & (N - 1); K[idx] = krow[idx]; }
  for (int x = threadIdx.x; x < m; x += 256) d[x] = mrow[x];
  __syncthreads();
#pragma unroll 4
  for (int i = part; i < m; i += RING_PARTS) {
    const int64_t dd = d[i];
    acc += (uint64_t)(c >= i ? -dd : dd) * K[(c - i) & (N - 1)];
  }
  return acc;
}
// the RING_PARTS partial sums of a coefficient meet through LDS; the sum is valid in the threads of part 0
__device__ __forceinline__ uint64_t ring_tile_sum(uint64_t acc, uint64_t* __restrict__ red, int part) {
  red[threadIdx.x] = acc;
  __syncthreads();
  if (part == 0)
    for (int p = 1; p < RING_PARTS; p++) acc += red[p * RING_TILE + threadIdx.x % RING_TILE];
  return acc;
}
__global__ void __launch_bounds__(256) k_ring_pack(const int32_t* __restrict__ dig, const uint64_t* __restrict__ small, size_t count, int n,
                                                   int logN, int l, const uint64_t* __restrict__ key, uint16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ uint64_t red[256];
  const int N = 1 << logN, tiles = N / RING_TILE;
  uint64_t* K = reinterpret_cast<uint64_t*>(smem_raw);
  int32_t* d = reinterpret_cast<int32_t*>(K + N);
  const int tile = (int)(blockIdx.x % tiles), comp = (int)((blockIdx.x / tiles) & 1);
  const size_t g = blockIdx.x / (2 * (size_t)tiles);
  const size_t left = count - g * N;
  const int m = left < (size_t)N ? (int)left : N;
  const int c = tile * RING_TILE + (threadIdx.x % RING_TILE), part = threadIdx.x / RING_TILE;
  const int rows = n * l;
  // the tile's coefficients meet key words (c - i) mod N, i < m: a window of m + RING_TILE - 1 words ending at the tile's last
  // coefficient -- all a partial group has to stage (one ResNet-20 image: 95 of 2048 words per row)
  const int span = m + RING_TILE - 1 < N ? m + RING_TILE - 1 : N;
  const int first = span < N ? (tile * RING_TILE - (m - 1)) & (N - 1) : 0;
  uint64_t acc = 0;
  for (int r = 0; r < rows; r++)
    acc = ring_tile_row(key + ((size_t)r * 2 + comp) * N, dig + (g * rows + r) * (size_t)N, N, m, first, span, c, part, K, d, acc);
  acc = ring_tile_sum(acc, red, part);
  if (part != 0) return;
  uint16_t* grp = out + g * 2 * (size_t)N;
  if (comp == 0) grp[c] = (uint16_t)round16(acc);
  else if (c < m) grp[N + c] = (uint16_t)round16(acc + small[(g * N + c) * (size_t)(n + 1) + n]);
}

// client: phases of ring-packed results on the 16-bit torus, phase16_i = (B16[i] - (A16 Z)[i]) mod 2^16 (negacyclic), returned as
// phase16 << 48.  One workgroup per (group, 256 slots); the group's mask and the ring key's bits sit in LDS, each thread walks the key
// bits (a broadcast read) for its slot with 32-bit partial sums, whose low 16 bits stay exact as in k_phase16.
__global__ void __launch_bounds__(256) k_ring_phase16(const uint8_t* __restrict__ S, int logN, const uint16_t* __restrict__ words, size_t count,
                                                      uint64_t* __restrict__ phases) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = 1 << logN, tiles = (N + 255) / 256;
  uint16_t* A = reinterpret_cast<uint16_t*>(smem_raw);
  uint8_t* Z = reinterpret_cast<uint8_t*>(A + N);
  const size_t g = blockIdx.x / tiles;
  const size_t left = count - g * N;
  const int m = left < (size_t)N ? (int)left : N;
  const uint16_t* grp = words + g * 2 * (size_t)N;
  for (int x = threadIdx.x; x < N; x += 256) { A[x] = grp[x]; Z[x] = S[x]; }
  __syncthreads();
  const int i = (int)(blockIdx.x % tiles) * 256 + threadIdx.x;
  if (i >= m) return;
  uint32_t part = 0;
  for (int c = 0; c < N; c++) {
    if (!Z[c]) continue;  // uniform branch
    const uint32_t a = A[(i - c) & (N - 1)];
    part += c <= i ? a : 0u - a;
  }
  phases[g * N + i] = (uint64_t)(((uint32_t)grp[N + i] - part) & 0xFFFFu) << 48;
}

// ---- public-key inputs: up to N phases in ONE GLWE ciphertext made without the secret key -----------------
// Public key: one GLWE zero row (A, B = A Z + E) under the ring key Z of the ring-packed results above, N = 2^logN <= input_dim.  A group
// of m <= N phases encrypts to C_a = A u + e1, C_b[i] = (B u)[i] + e2[i] + phase_i (i < m) with u binary: coefficient i of C_b - C_a Z is
// phase_i + (E u + e2 - e1 Z)[i].  The server extracts slot i as an LWE row under the first N bits of the big key.

// the key's body [N]: row 0 of a k = 1 bootstrap key without a message (bsk_row_zero): mask word c is rnd64(pub, stream, c), its noise
// gauss_torus(sec, stream + 1, c); k_seeded_expand rebuilds the mask.  One block.
__global__ void k_pk_gen(const uint8_t* __restrict__ S_big, int N, double sigma, rng_key pub, rng_key sec, uint64_t stream, uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bsk_row_zero(S_big, 0, 1, N, sigma, pub, sec, stream, reinterpret_cast<uint64_t*>(smem_raw), out, nullptr);
}

// the draws of one encryption call, all from the encryptor's own generator key: u[x] the top bit of word (stream, x), e1[x] the Gaussian
// draw (stream + 1, x) for x < nmask = groups N, e2[x] the draw (stream + 2, x) for x < count <= nmask
__global__ void k_pk_draws(rng_key key, uint64_t stream, size_t nmask, size_t count, double sigma, int32_t* __restrict__ u, int64_t* __restrict__ e1,
                           int64_t* __restrict__ e2) {
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < nmask; x += (size_t)gridDim.x * blockDim.x) {
    u[x] = (int32_t)(rnd64(key, stream, x) >> 63);
    e1[x] = gauss_torus(key, stream + 1, x, sigma);
    if (x < count) e2[x] = gauss_torus(key, stream + 2, x, sigma);
  }
}

// One workgroup per (group g, component: 0 mask / 1 body, tile of RING_TILE output coefficients), the tile loop of k_ring_pack with ONE
// key row (component comp of the public key, all N words) and the group's N bits u as multipliers: ring_tile_row leaves
// -sum_{i: u_i = 1} +-K[(c - i) mod N], the sign flipped where c < i.  Epilogue: the mask takes e1, the first m body coefficients e2 and
// the phase; body tiles beyond m leave at once.  N = 32 is one tile: c < N always, and the staging loops stop at N.
// Wire words (u64): per group its N mask words, then its first m body words; groups before the last are full.
__global__ void __launch_bounds__(256) k_pk_encrypt(const int32_t* __restrict__ u, const int64_t* __restrict__ e1, const int64_t* __restrict__ e2,
                                                    const uint64_t* __restrict__ phases, size_t count, int logN, const uint64_t* __restrict__ key,
                                                    uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ uint64_t red[256];
  const int N = 1 << logN, tiles = N / RING_TILE;
  uint64_t* K = reinterpret_cast<uint64_t*>(smem_raw);
  int32_t* d = reinterpret_cast<int32_t*>(K + N);
  const int tile = (int)(blockIdx.x % tiles), comp = (int)((blockIdx.x / tiles) & 1);
  const size_t g = blockIdx.x / (2 * (size_t)tiles);
  const size_t left = count - g * N;
  const int m = left < (size_t)N ? (int)left : N;
  if (comp == 1 && tile * RING_TILE >= m) return;      // the whole workgroup: no body word of this tile travels
  const int c = tile * RING_TILE + (threadIdx.x % RING_TILE), part = threadIdx.x / RING_TILE;
  uint64_t acc = ring_tile_row(key + (size_t)comp * N, u + g * N, N, N, 0, N, c, part, K, d, 0);
  acc = ring_tile_sum(acc, red, part);
  if (part != 0) return;
  const size_t x = g * N + c;
  uint64_t* grp = out + g * 2 * (size_t)N;
  if (comp == 0) grp[c] = (uint64_t)e1[x] - acc;
  else if (c < m) grp[N + c] = (uint64_t)e2[x] + phases[x] - acc;
}

// server: slot i of a group -> the LWE row a_j = C_a[i - j] (j <= i), -C_a[N + i - j] (i < j < N), zeros up to the row's body, body
// C_b[i], written at row stride L (body at word L - 1) -- straight into a session's input tensor, or into rows of dim + 1 words.
// One workgroup per (group, tile of EXTRACT_TILE slots); the group's N mask words sit in LDS (<= 32 KB); each wave writes whole rows, its
// lanes on consecutive mask words (reads run DOWN the LDS array, conflict-free; stores are 512 contiguous bytes per wave), the body last.
constexpr int EXTRACT_TILE = 32;
__global__ void __launch_bounds__(256) k_pk_extract(const uint64_t* __restrict__ words, size_t count, int logN, size_t L, uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = 1 << logN, tiles = N / EXTRACT_TILE;
  uint64_t* A = reinterpret_cast<uint64_t*>(smem_raw);
  const int tile = (int)(blockIdx.x % tiles);
  const size_t g = blockIdx.x / tiles;
  const size_t left = count - g * N;
  const int m = left < (size_t)N ? (int)left : N;
  if (tile * EXTRACT_TILE >= m) return;                // the whole workgroup: no slot of this tile is filled
  const uint64_t* grp = words + g * 2 * (size_t)N;
  for (int x = threadIdx.x; x < N; x += 256) A[x] = grp[x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int end = (tile + 1) * EXTRACT_TILE < m ? (tile + 1) * EXTRACT_TILE : m;
  for (int i = tile * EXTRACT_TILE + wv; i < end; i += 4) {
    uint64_t* row = out + (g * N + i) * L;
    for (size_t j = lane; j + 1 < L; j += 64)
      row[j] = j < (size_t)N ? ((int)j <= i ? A[i - (int)j] : (uint64_t)0 - A[N + i - (int)j]) : 0;
    if (lane == 0) row[L - 1] = grp[N + i];
  }
}

// ------------------------------------------------------------------------------------------ K4-K6 bootstrap
struct pbs_launch {
  const uint64_t* cts_small;  // count x (n+1)
  size_t count;
  int n, beta;
  const cplx* bsk;
  const cplx* tw;             // twiddle table in global memory
  const cplx* wtab;           // two-bit kernels: e^{i pi m / N}, m < 2N
  const int64_t* tables;      // [ntab][2^w]
  int w;
  const int32_t* table_idx;   // optional explicit index per ciphertext
  int hw, nchan;              // else table = ((e_offset + e) / hw) % nchan  (nchan == 1: single table)
  size_t e_offset;
  uint64_t* out;              // count x (D_out+1)
  int D_out;
  int accumulate;
  uint64_t body_add;
  uint64_t* dummy;            // D_out+1 words: sink for the padded groups of the last workgroup
  int bsk_wrap;               // cache experiments only (0 in the library; kept for the register allocation: pbs_args)
  int pf_parts;               // 0: no L2 warm-up; else each workgroup touches 1/pf_parts of the next key rows
};

template <int LOGN, int K, int L, int P, int MB>
constexpr size_t pbs_lds_bytes(int groups) {
  using G = pbs_geom<LOGN, K, L, P, MB>;
  return (size_t)G::TW_BYTES + (size_t)groups * G::GROUP_BYTES;
}

template <int LOGN, int K, int L, int P, int GROUPS, int MB = 0>
__global__ void __launch_bounds__((pbs_geom<LOGN, K, L, P, MB>::T * GROUPS), ((P >= 16 || (pbs_geom<LOGN, K, L, P, MB>::T * GROUPS) >= 512) ? 1 : 2))
pbs_kernel(pbs_launch a) {
  using G = pbs_geom<LOGN, K, L, P, MB>;
  constexpr int T = G::T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  cplx* tw = reinterpret_cast<cplx*>(smem_raw);
  unsigned char* per_group = smem_raw + G::TW_BYTES;
  for (int x = threadIdx.x; x < G::TW_LDS_ELEMS; x += blockDim.x) tw[x] = a.tw[x];
  if constexpr (MB) {     // root tables of the two-bit rotation: lo[j] = zeta^j, hi[j] = zeta^(j << ZLO)
    cplx* zl = tw + G::TW_LDS_ELEMS;
    for (int x = threadIdx.x; x < G::ZLUT_ELEMS; x += blockDim.x) zl[x] = x < (1 << G::ZLO) ? a.wtab[x] : a.wtab[(size_t)(x - (1 << G::ZLO)) << G::ZLO];
  }
  __syncthreads();
  const int g = threadIdx.x / T, t = threadIdx.x % T;
  size_t e = (size_t)blockIdx.x * GROUPS + g;
  const bool live = e < a.count;
  if (!live) e = a.count - 1;  // padded groups redo the last ciphertext and drop the result
  unsigned char* mine = per_group + (size_t)g * G::GROUP_BYTES;
  cplx* exch = reinterpret_cast<cplx*>(mine);
  uint64_t* stage = reinterpret_cast<uint64_t*>(mine + G::STAGE_OFFSET);     // aliases the exchange buffer when G::ALIAS
  uint64_t* accl = reinterpret_cast<uint64_t*>(mine + G::SHARED_BYTES);
  uint32_t* pf_dump = nullptr;     // host emulation only
  pbs_args A;
  A.ct_small = a.cts_small + e * (size_t)(a.n + 1);
  A.n = a.n; A.beta = a.beta; A.bsk = a.bsk;
  const size_t ti = a.table_idx ? (size_t)a.table_idx[e] : (a.nchan > 1 ? ((a.e_offset + e) / (size_t)a.hw) % (size_t)a.nchan : 0);
  A.table = a.tables + (ti << a.w);
  A.w = a.w;
  // padded groups of the last workgroup redo the last ciphertext (same barrier sequence) into a sink
  A.out = live ? a.out + e * (size_t)(a.D_out + 1) : a.dummy;
  A.D_out = a.D_out;
  A.accumulate = live ? a.accumulate : 0;
  A.body_add = a.body_add;
  A.bsk_wrap = a.bsk_wrap;
  A.pf_parts = a.pf_parts;
  A.wtab = a.wtab;
  A.zlut = MB ? tw + G::TW_LDS_ELEMS : nullptr;
  if constexpr (G::TWIST_LDS) A.twist = tw + G::F::TW_TOTAL; else A.twist = a.tw + G::F::TW_TOTAL;
  A.pf_rank = (int)((blockIdx.x / 8) % (unsigned)(a.pf_parts > 0 ? a.pf_parts : 1));   // blocks b and b+8 share an XCD (round-robin dispatch; speed only)
  if constexpr (T <= 64) {
    // one ciphertext per wave (or less): every exchange and the rotation stage stay inside the wave, whose LDS
    // queue is in order -- no workgroup barrier anywhere in the loop, the waves of a workgroup run decoupled
    pbs_thread<LOGN, K, L, P, MB>(A, t, tw, stage, exch, accl, pf_dump, [] { __builtin_amdgcn_wave_barrier(); }, [] { __builtin_amdgcn_wave_barrier(); });
  } else {
    pbs_thread<LOGN, K, L, P, MB>(A, t, tw, stage, exch, accl, pf_dump, [] { __syncthreads(); }, [] { __builtin_amdgcn_wave_barrier(); });
  }
}

// The duo form of the general two-bit bootstrap (pbs_thread_duo): DUOS groups of T = M / P threads per workgroup, two ciphertexts
// each.  LDS per duo: the two exchange buffers (contiguous: fft_forward_n), then the LDS-resident accumulator polynomials of both.
template <int LOGN, int K, int L, int P>
constexpr size_t pbs_duo_lds_bytes(int duos) {
  using G = pbs_geom<LOGN, K, L, P, 1>;
  return (size_t)G::TW_BYTES + (size_t)duos * 2 * G::GROUP_BYTES;
}

template <int LOGN, int K, int L, int P, int DUOS>
__global__ void __launch_bounds__((pbs_geom<LOGN, K, L, P, 1>::T * DUOS), ((pbs_geom<LOGN, K, L, P, 1>::T * DUOS) >= 512 ? 1 : 2))
pbs_kernel_duo(pbs_launch a) {
  using G = pbs_geom<LOGN, K, L, P, 1>;
  constexpr int T = G::T;
  static_assert(T >= 64 && T % 64 == 0, "a wave holds threads of one duo only");
  static_assert(G::TWIST_LDS && G::SHARED_BYTES == G::EXCH_BYTES, "duo LDS layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  cplx* tw = reinterpret_cast<cplx*>(smem_raw);
  unsigned char* per_duo = smem_raw + G::TW_BYTES;
  for (int x = threadIdx.x; x < G::TW_LDS_ELEMS; x += blockDim.x) tw[x] = a.tw[x];
  {     // root tables of the two-bit rotation: lo[j] = zeta^j, hi[j] = zeta^(j << ZLO)
    cplx* zl = tw + G::TW_LDS_ELEMS;
    for (int x = threadIdx.x; x < G::ZLUT_ELEMS; x += blockDim.x) zl[x] = x < (1 << G::ZLO) ? a.wtab[x] : a.wtab[(size_t)(x - (1 << G::ZLO)) << G::ZLO];
  }
  __syncthreads();
  const int g = threadIdx.x / T, t = threadIdx.x % T;
  unsigned char* mine = per_duo + (size_t)g * 2 * G::GROUP_BYTES;
  cplx* exch = reinterpret_cast<cplx*>(mine);
  uint64_t* accl = reinterpret_cast<uint64_t*>(mine + 2 * G::EXCH_BYTES);
  pbs_args A2[2];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    size_t e = ((size_t)blockIdx.x * DUOS + g) * 2 + c;
    const bool live = e < a.count;
    if (!live) e = a.count - 1;  // padded slots redo the last ciphertext in store mode into the sink
    pbs_args& A = A2[c];
    A.ct_small = a.cts_small + e * (size_t)(a.n + 1);
    A.n = a.n; A.beta = a.beta; A.bsk = a.bsk;
    const size_t ti = a.table_idx ? (size_t)a.table_idx[e] : (a.nchan > 1 ? ((a.e_offset + e) / (size_t)a.hw) % (size_t)a.nchan : 0);
    A.table = a.tables + (ti << a.w);
    A.w = a.w;
    A.out = live ? a.out + e * (size_t)(a.D_out + 1) : a.dummy;
    A.D_out = a.D_out;
    A.accumulate = live ? a.accumulate : 0;
    A.body_add = a.body_add;
    A.bsk_wrap = 0;
    A.pf_parts = a.pf_parts;
    A.wtab = a.wtab;
    A.zlut = tw + G::TW_LDS_ELEMS;
    A.twist = tw + G::F::TW_TOTAL;
    A.pf_rank = (int)((blockIdx.x / 8) % (unsigned)(a.pf_parts > 0 ? a.pf_parts : 1));
  }
  pbs_thread_duo<LOGN, K, L, P>(A2, t, tw, exch, accl, nullptr, [] { __syncthreads(); }, [] { __builtin_amdgcn_wave_barrier(); });
}

// ------------------------------------------------------------------------------------------ K1 conv2d
// out[b][co][y][x][word] = sum_{ci,ky,kx} w[co][ci][ky][kx] * in[b][ci][y*s+ky-p][x*s+kx-p][word]  (mod 2^64)
// Thread = one ciphertext word of one output pixel for a tile of COT output channels; lanes run over
// words, so every load is a coalesced stream of one input ciphertext.
// Output window (both kernels): channels [c0, c1) only, written to a buffer laid out [batch][c1 - c0][Ho][Wo] (relative to the window,
// not to the whole tensor), and pixels from pix0 on, one per block of gridDim.y.  c0 = 0, c1 = Cout, pix0 = 0 is the whole output.
template <int COT>
__global__ void __launch_bounds__(256)
k_conv2d(const uint64_t* __restrict__ in, int Cin, int H, int W, size_t Lin, size_t Deff, const int8_t* __restrict__ wgt, int c0, int c1,
         int pix0, int KH, int KW, int stride, int pad, int Ho, int Wo, size_t Lout, uint64_t* __restrict__ out) {
  // tensors are stored at their effective dimension: a row is Deff mask words (everything beyond is known to be zero and is
  // not stored) then the body; thread Deff of a pixel handles the body word
  const size_t word = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int pix = pix0 + blockIdx.y;    // b*Ho*Wo + y*Wo + x
  const int co0 = c0 + blockIdx.z * COT;
  const int b = pix / (Ho * Wo), y = (pix / Wo) % Ho, x = pix % Wo;
  if (word >= Lout) return;
  const bool body = word == Lout - 1;
  uint64_t acc[COT];
#pragma unroll
  for (int c = 0; c < COT; c++) acc[c] = 0;
  if (body || word < Deff) {      // (words in [Deff, Lout-1) only exist when the output row is wider than its input: zeros)
    const size_t iw = body ? Lin - 1 : word;
    const uint64_t* inb = in + (size_t)b * Cin * H * W * Lin;
    for (int ci = 0; ci < Cin; ci++)
      for (int ky = 0; ky < KH; ky++) {
        const int iy = y * stride + ky - pad;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < KW; kx++) {
          const int ix = x * stride + kx - pad;
          if (ix < 0 || ix >= W) continue;
          const uint64_t v = inb[(((size_t)ci * H + iy) * W + ix) * Lin + iw];
#pragma unroll
          for (int c = 0; c < COT; c++) {
            const int co = co0 + c;
            const int8_t wv = (co < c1) ? wgt[(((size_t)co * Cin + ci) * KH + ky) * KW + kx] : (int8_t)0;  // uniform
            acc[c] += (uint64_t)(int64_t)wv * v;
          }
        }
      }
  }
#pragma unroll
  for (int c = 0; c < COT; c++) {
    const int co = co0 + c;
    if (co < c1) out[((((size_t)b * (c1 - c0) + (co - c0)) * Ho + y) * Wo + x) * Lout + word] = acc[c];
  }
}

// ---- convolution on the matrix cores -------------------------------------------------------------------
// out[co][word] = sum_k w[co][k] * in_k[word] (mod 2^64), k = (ci, ky, kx), is a GEMM with a tiny-integer left operand (|w| <= 127)
// and a u64 right operand.  As in the key switch the u64 operand is re-expressed as 8 signed byte limbs (carries propagated),
// here on the fly while the input tile is staged: C[co][word*8 + limb] = sum_k w[co][k] * s_limb(in_k[word]) is an i8 x i8 -> i32
// GEMM for v_mfma_i32_32x32x32_i8 (|C| <= K * 127 * 128 < 2^31 for K <= 2^17) and out = sum_limb C_limb << 8 limb.
// Workgroup = one output pixel x 32 ciphertext words x 64 output channels; K in steps of 32 (ci, ky, kx) triples; wave w owns
// columns [64 w, 64 w + 64) = 8 words x 8 limbs.  Both operands K-contiguous in LDS (one ds_read_b128 per fragment).
// The 64-channel tiles start at c0, so a tile may reach past the padded weight rows: rows at or past c1 are loaded as zeros.
struct conv_tap { int32_t offset; int16_t dy, dx; };     // per k = (ci, ky, kx): ci*H*W (pixels; < 0: padding row of K), ky - pad, kx - pad

__global__ void __launch_bounds__(256)
k_conv2d_mfma(const uint64_t* __restrict__ in, int H, int W, size_t Lin, size_t Deff, const int8_t* __restrict__ wpack /* [Cout_pad64][Kpad] */,
              const conv_tap* __restrict__ taps /* [Kpad], offset < 0: padding row */, int Kpad, int Cin_HW, int c0, int c1, int pix0, int stride,
              int Ho, int Wo, size_t Lout, uint64_t* __restrict__ out) {
  constexpr int BK = 32, LD = BK + 16;
  __shared__ __attribute__((aligned(16))) int8_t As[64 * LD];
  __shared__ __attribute__((aligned(16))) int8_t Bs[256 * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pix = pix0 + blockIdx.y;    // b*Ho*Wo + y*Wo + x
  const int b = pix / (Ho * Wo), y = (pix / Wo) % Ho, x = pix % Wo;
  const int co0 = c0 + blockIdx.z * 64;
  // staging: thread = (word w of 32, group kq of 8): 4 consecutive k for one word
  const int sw = tid & 31, kq = tid >> 5;
  const size_t wg = (size_t)blockIdx.x * 32 + sw;                    // word of the output row this thread stages
  const bool wbody = wg == Lout - 1, wlive = wbody || wg < Deff;      // (words in [Deff, Lout-1) are zero)
  const size_t iw = wbody ? Lin - 1 : wg;
  const uint64_t* inb = in + (size_t)b * Cin_HW * Lin;
  const int y0 = y * stride, x0 = x * stride;
  v16i acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[a][c][e] = 0;
  const int fr = lane & 31, fh = (lane >> 5) * 16;
  for (int k0 = 0; k0 < Kpad; k0 += BK) {
    // input words of this thread's 4 taps -> signed byte limbs, limb-major so that each limb row gets one 4-byte store
    uint32_t packed[8];
#pragma unroll
    for (int l = 0; l < 8; l++) packed[l] = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const conv_tap tp = taps[k0 + kq * 4 + u];
      const int iy = y0 + tp.dy, ix = x0 + tp.dx;
      uint64_t v = 0;
      if (wlive && tp.offset >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W)
        v = inb[((size_t)tp.offset + (size_t)(iy * W + ix)) * Lin + iw];
#pragma unroll
      for (int l = 0; l < 8; l++) {
        int byte = (int)(v & 0xFF);
        v >>= 8;
        if (byte >= 128) { byte -= 256; v += 1; }
        packed[l] |= (uint32_t)(byte & 0xFF) << (8 * u);
      }
    }
    v4i ga = {0, 0, 0, 0};
    if (tid < 128 && co0 + (tid >> 1) < c1) ga = *reinterpret_cast<const v4i*>(wpack + (size_t)(co0 + (tid >> 1)) * Kpad + k0 + (tid & 1) * 16);
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 8; l++) *reinterpret_cast<uint32_t*>(&Bs[(sw * 8 + l) * LD + kq * 4]) = packed[l];
    if (tid < 128) *reinterpret_cast<v4i*>(&As[(tid >> 1) * LD + (tid & 1) * 16]) = ga;
    __syncthreads();
    v4i fa[2], fb[2];
#pragma unroll
    for (int a = 0; a < 2; a++) fa[a] = *reinterpret_cast<const v4i*>(&As[(a * 32 + fr) * LD + fh]);
#pragma unroll
    for (int c = 0; c < 2; c++) fb[c] = *reinterpret_cast<const v4i*>(&Bs[(wave * 64 + c * 32 + fr) * LD + fh]);
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int c = 0; c < 2; c++) acc[a][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[c], acc[a][c], 0, 0, 0);
  }
  // epilogue: C tile layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); limb = col & 7, word = col >> 3
  const int limb = lane & 7;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const size_t word = (size_t)blockIdx.x * 32 + wave * 8 + c * 4 + ((lane & 31) >> 3);
#pragma unroll
      for (int e = 0; e < 16; e++) {
        uint64_t v = (uint64_t)(int64_t)acc[a][c][e] << (8 * limb);
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        const int co = co0 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (limb == 0 && co < c1 && word < Lout) out[((((size_t)b * (c1 - c0) + (co - c0)) * Ho + y) * Wo + x) * Lout + word] = v;
      }
    }
}

// any non-zero mask word in [deff, D) of `count` ciphertexts?  (guards the effective-dimension shortcut at the session input)
__global__ void k_tail_nonzero(const uint64_t* __restrict__ cts, size_t count, int D /* mask words per row */, int deff, int* __restrict__ flag) {
  const size_t tail = (size_t)(D - deff), total = count * tail;
  int bad = 0;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x)
    bad |= cts[(x / tail) * (size_t)(D + 1) + deff + (x % tail)] != 0;
  if (bad) atomicOr(flag, 1);
}

// ------------------------------------------------------------------------------------------ K2 elementwise
// Rows are stored at their effective dimension (mask words the compiler knows to be zero are not stored): a row of stride L
// holds L-1 mask words and the body at L-1.  `take(row, L, d, w)` is word w of a row whose first d mask words may be non-zero.
__device__ __forceinline__ uint64_t row_word(const uint64_t* row, size_t L, size_t d, size_t w, bool body) {
  return body ? row[L - 1] : (w < d ? row[w] : 0);
}
// o = a + b; the operands may have different effective dimensions (the result has the larger)
__global__ void k_add(const uint64_t* __restrict__ a, size_t La, size_t da, const uint64_t* __restrict__ b, size_t Lb, size_t db,
                      uint64_t* __restrict__ o, size_t Lo, size_t count) {
  const size_t total = count * Lo;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i / Lo, w = i % Lo;
    const bool body = w == Lo - 1;
    o[i] = row_word(a + c * La, La, da, w, body) + row_word(b + c * Lb, Lb, db, w, body);
  }
}
// o = (a << shift), body += body_add: the first nwords mask words and the body of every row (mask words only shifted); what
// lies between nwords and the end of an output row is left alone (the table bootstrap that ends the site rewrites the row)
__global__ void k_affine(const uint64_t* __restrict__ a, size_t La, size_t da, uint64_t* __restrict__ o, size_t Lo, size_t count, size_t nwords,
                         int shift, uint64_t body_add) {
  const size_t per = nwords + 1, total = count * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i / per, w = i % per;
    const bool body = w == nwords;
    uint64_t v = row_word(a + c * La, La, da, w, body) << shift;
    if (body) v += body_add;
    o[c * Lo + (body ? Lo - 1 : w)] = v;
  }
}
// o += b on the first nwords mask words and the body of every row (rows of stride Lo / Lb): the sum of the two look-ups of a
// parity-split site, over the ring the second one wrote
__global__ void k_acc_rows(uint64_t* __restrict__ o, size_t Lo, const uint64_t* __restrict__ b, size_t Lb, size_t count, size_t nwords) {
  const size_t per = nwords + 1, total = count * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i / per, w = i % per;
    const bool body = w == nwords;
    o[c * Lo + (body ? Lo - 1 : w)] += b[c * Lb + (body ? Lb - 1 : w)];
  }
}
// rows of stride Ls -> rows of stride Ld: the first nwords mask words and the body; the other words of the output row are zero
// (session upload: host rows of D+1 words -> stored rows; download: the reverse)
__global__ void k_restride(const uint64_t* __restrict__ src, size_t Ls, uint64_t* __restrict__ dst, size_t Ld, size_t count, size_t nwords) {
  const size_t total = count * Ld;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i / Ld, w = i % Ld;
    dst[i] = w == Ld - 1 ? src[c * Ls + Ls - 1] : (w < nwords ? src[c * Ls + w] : 0);
  }
}
// window-K sum pooling with floor semantics (reference nn.AvgPool2d(k): backbone.py:276; scale folded into the next table)
__global__ void k_sum_pool(const uint64_t* __restrict__ in, int C, int H, int W, size_t Lin, size_t din, int K, int Ho, int Wo,
                           uint64_t* __restrict__ out, size_t Lout, size_t total_words) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_words; i += (size_t)gridDim.x * blockDim.x) {
    const size_t word = i % Lout;
    const bool body = word == Lout - 1;
    size_t e = i / Lout;
    const int x = (int)(e % Wo); e /= Wo;
    const int y = (int)(e % Ho); e /= Ho;  // e = b*C + c
    uint64_t s = 0;
    for (int ky = 0; ky < K; ky++)
      for (int kx = 0; kx < K; kx++) s += row_word(in + ((e * H + (size_t)(y * K + ky)) * W + (size_t)(x * K + kx)) * Lin, Lin, din, word, body);
    out[i] = s;
  }
}

// one tree level of a max pool: row r of the level's output is a copy of source row map[r] (the `b` of a pairwise maximum, which the
// difference bootstrap then accumulates into, or a candidate carried to the next level), at the output's row stride; mask words beyond
// the source's effective dimension are written as zeros
__global__ void k_pool_gather(const uint64_t* __restrict__ src, size_t Ls, size_t ds, const int32_t* __restrict__ map, uint64_t* __restrict__ dst,
                              size_t Ld, size_t count) {
  const size_t total = count * Ld;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / Ld, w = i % Ld;
    dst[i] = row_word(src + (size_t)map[r] * Ls, Ls, ds, w, w == Ld - 1);
  }
}

// simulate: Gaussian noise of std sigma on a phase sitting at `centre`, then the bootstrap's half-box rotation and negacyclic wrap, the
// entry of `table` it lands on (the look-up of k_lut_clear and k_maxpool_clear)
__device__ __forceinline__ uint64_t noisy_lookup(uint64_t centre, int w, const int64_t* __restrict__ table, const rng_key& seed, uint64_t stream,
                                                 uint64_t idx, double sigma) {
  const uint64_t half_box = 1ULL << (62 - w);
  const uint64_t noisy = centre + (uint64_t)gauss_torus(seed, stream, idx, sigma);
  // negacyclic wrap: a value pushed across the padding bit comes back negated -- reproduce the bootstrap's behaviour
  const uint64_t pos = noisy + half_box;
  const uint64_t t = (uint64_t)table[(pos >> (63 - w)) & ((1ULL << w) - 1)];
  return (pos >> 63) ? (uint64_t)0 - t : t;
}

// clear-mode table look-up on 1-word "ciphertexts" (D = 0): same arithmetic as round_lut without noise.
// sigma > 0 (`simulate` with the noise model): Gaussian noise of that standard deviation (fraction of the torus: what the
// compiler predicts at the input of this site's table bootstrap) is added where the encrypted run has it -- after the exact
// rounding steps have cleared the low bits, or, with approximate rounding, on the raw accumulator -- and the half-box
// rotation of the test vector does the rest.
// split != 0 (parity split of a 7-bit table, t = 2 t' + b0): with sigma > 0 the noise is sampled at BOTH look-ups the encrypted run makes
// (RNG indices 2e and 2e + 1; sigma at the first, sigma2 at the second, whose input also carries the parity bootstrap's output) on the
// half tables S / Dt [ntab][2^(w-1)], the second with b0 in the padding bit, so that the negacyclic wrap returns (-1)^b0 Dt[t'];
// with sigma == 0 it is the plain 2^w-entry read.
// in / out point at the first of `count` elements of a slice that starts at element e0 of the tensor (a sharded session; 0: the whole tensor).
__global__ void k_lut_clear(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, size_t count, int shift, uint64_t body_add,
                            int p, int r, int w, const int64_t* __restrict__ tables, int hw, int nchan, int* __restrict__ overflow,
                            double sigma, rng_key seed, uint64_t stream, int approx, int split, double sigma2,
                            const int64_t* __restrict__ tab_s, const int64_t* __restrict__ tab_d, size_t e0) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x) {
    const size_t g = e0 + e;      // the element's number in the whole tensor: its channel's table and its noise draws go by it
    uint64_t v = (in[e] << shift) + body_add;
    if (r > 0 && !(approx && sigma > 0)) v += 1ULL << (63 - p + r - 1);
    if (v >> 63) atomicOr(overflow, 1);  // message left the padded range: an FHE run would wrap
    uint64_t idx = (v >> (63 - w)) & ((1ULL << w) - 1);
    if (sigma > 0 && split) {
      const size_t ti = nchan > 1 ? (g / (size_t)hw) % (size_t)nchan : 0;
      const uint64_t centre = (idx >> 1) << (64 - w);              // t' as a (w-1)-bit message under a clear padding bit
      out[e] = noisy_lookup(centre, w - 1, tab_s + (ti << (w - 1)), seed, stream, 2 * g, sigma) +
               noisy_lookup(centre + ((idx & 1) << 63), w - 1, tab_d + (ti << (w - 1)), seed, stream, 2 * g + 1, sigma2);
      continue;
    }
    if (sigma > 0) {
      // exact rounding: the value sits at the centre of its box; approximate: where its low bits put it (+ half an input unit)
      const uint64_t centre = approx && r > 0 ? v + (1ULL << (62 - p)) : (idx << (63 - w));
      const size_t ti = nchan > 1 ? (g / (size_t)hw) % (size_t)nchan : 0;
      out[e] = noisy_lookup(centre, w, tables + (ti << w), seed, stream, g, sigma);
      continue;
    }
    const size_t ti = nchan > 1 ? (g / (size_t)hw) % (size_t)nchan : 0;
    out[e] = (uint64_t)tables[(ti << w) + idx];
  }
}

// clear-mode max pool, one 1-D pass: in [outer][n_in][inner] -> out [outer][n_out][inner], one thread per output, over the window's
// in-range taps.  sigma == 0: the maximum of the words read as signed int64.  sigma > 0 (`simulate`): the taps are folded as
// m = m + relu(x - m) with the noise sampled on every difference before the relu table (`table`: 2^p_d entries, index
// ((x - m) << shift) + body_add) -- one noisy look-up per pairwise maximum, as many as the encrypted tree runs.
// The launch computes outputs [e0, e0 + count) of the pass (all of them, or a divided pool's part; consecutive lanes on consecutive
// outputs).  in points at element in0 of the pass input and out at element out0 of the pass output, so a part's `mid` buffer holds its
// intermediates only; the noise of an output is drawn by its number e in the whole pass, whichever part computes it.
__global__ void k_maxpool_clear(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, size_t e0, size_t count, size_t in0, size_t out0,
                                int n_in, int inner, int n_out, int k, int s, int p, int shift, uint64_t body_add, int p_d,
                                const int64_t* __restrict__ table, double sigma, rng_key seed, uint64_t stream) {
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (size_t)gridDim.x * blockDim.x) {
    const size_t e = e0 + t;
    const int i = (int)(e % inner);
    const int o = (int)((e / inner) % n_out);
    const size_t ou = e / ((size_t)inner * n_out);
    uint64_t m = 0;
    int taken = 0;
    for (int j = 0; j < k; j++) {
      const int x = o * s - p + j;
      if (x < 0 || x >= n_in) continue;
      const uint64_t v = in[(ou * n_in + x) * inner + i - in0];
      if (taken == 0) {
        m = v;
      } else if (sigma > 0) {
        const uint64_t d = ((v - m) << shift) + body_add;
        const uint64_t centre = ((d >> (63 - p_d)) & ((1ULL << p_d) - 1)) << (63 - p_d);
        m += noisy_lookup(centre, p_d, table, seed, stream, e * 64 + (uint64_t)taken, sigma);
      } else {
        m = (int64_t)v > (int64_t)m ? v : m;
      }
      taken++;
    }
    out[e - out0] = m;
  }
}

// ------------------------------------------------------------------------------------------ K10 DCT front-end (client side, plaintext)
// uint8 planes -> float32 [B][channels][S][S]: (pixel - 128) blockwise orthonormal DCT-II (T B T^t per fs x fs block,
// reference data/cvfunctional.py:37-57), only the coefficients SubsetDCT keeps (cvtransforms.py:117-142), the two chroma
// coefficient grids -- DCT'd at half resolution -- bilinearly up-sampled to S x S (UpScaleDCT, cvtransforms.py:56-64;
// half-pixel centres, edge clamp), channels concatenated Y | slot 1 | slot 2 (Aggregate), then (x - mean) / std in f32
// (NormalizeDCT, cvtransforms.py:152-208; mean/std already gathered by the caller with the reference's index quirk).
// One thread per output value; f64 inside like the reference's numpy path.  A few kB per image: nothing to tune.
struct dct_args {
  const uint8_t* plane[3];      // Y [B][fs*S][fs*S]; chroma slots [B][fs*Sc][fs*Sc]
  int S, Sc, fs;                // output grid, chroma grid (S or S/2), block size (4 or 8)
  int n[3];                     // kept coefficients per plane
  const int32_t* idx[3];        // their row-major indices u*fs + v
  const float *mean, *stdv;     // per output channel
  int round_coeffs;             // JPEG-domain path (block size 8): coefficients are libjpeg's quantised integers (integer islow DCT, quality-100
                                // tables) and the up-sampled planes are rounded half to even, as the int16 arrays of the reference are
  float* out;                   // [B][n0+n1+n2][S][S]
  int batch;
};

// libjpeg's accurate integer forward DCT ("islow": Loeffler-Ligtenberg-Moschytz, 13-bit constants, 2 extra bits carried out of the row
// pass; jfdctint.c [K: restated from the published algorithm; pinned to the coefficients libjpeg-turbo wrote into quality-100 JPEG files,
// tests/golden/jpeg_golden.npz, by tests/test_gpu_frontend_jpeg.py and, for the host twin, tests/test_jpeg_pin_host.py]) on one row
// or column of 8 values, in place.  TurboJPEG picks this method at quality >= 96 (reference data/cvfunctional.py:24: quality=100).
// first = 1: row pass (outputs scaled by 2^2 * sqrt(8)); first = 0: column pass (removes the 2^2; the 2-D result is 8x the DCT).
__host__ __device__ inline void jfdct_islow_1d(int32_t* d, int first) {
  constexpr int CB = 13, P1 = 2;
  constexpr int32_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
                    F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  auto descale = [](int32_t x, int n) { return (x + (1 << (n - 1))) >> n; };
  int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int sh = first ? CB - P1 : CB + P1;
  d[0] = first ? (t10 + t11) << P1 : descale(t10 + t11, P1);
  d[4] = first ? (t10 - t11) << P1 : descale(t10 - t11, P1);
  int32_t z1 = (t12 + t13) * F0_541;
  d[2] = descale(z1 + t13 * F0_765, sh);
  d[6] = descale(z1 - t12 * F1_847, sh);
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * F1_175;
  t4 *= F0_298; t5 *= F2_053; t6 *= F3_072; t7 *= F1_501;
  z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
  z3 += z5; z4 += z5;
  d[7] = descale(t4 + z1 + z3, sh);
  d[5] = descale(t5 + z2 + z4, sh);
  d[3] = descale(t6 + z2 + z3, sh);
  d[1] = descale(t7 + z1 + z4, sh);
}
// quantised coefficient (u, v) of 8x8 block (by, bx): level shift, islow DCT, division by 8 * q with q = 1 (the quality-100 tables are
// all ones), rounded half away from zero as libjpeg's quantiser does (jcdctmgr.c)
__device__ inline int32_t jpeg_islow_coeff(const uint8_t* plane, int side, int by, int bx, int u, int v) {
  int32_t col[8];
  for (int i = 0; i < 8; i++) {
    int32_t row[8];
    for (int j = 0; j < 8; j++) row[j] = (int32_t)plane[(size_t)(by * 8 + i) * side + bx * 8 + j] - 128;
    jfdct_islow_1d(row, 1);
    col[i] = row[v];
  }
  jfdct_islow_1d(col, 0);
  const int32_t c = col[u];
  return c < 0 ? -((-c + 4) >> 3) : (c + 4) >> 3;
}

__device__ __forceinline__ double dct_basis(int fs, int u, int j) {
  return u == 0 ? rsqrt((double)fs) : sqrt(2.0 / fs) * cospi((double)((2 * j + 1) * u) / (double)(2 * fs));
}
__device__ inline double dct_coeff(const uint8_t* plane, int side, int fs, int by, int bx, int u, int v, int round_coeffs) {
  if (round_coeffs && fs == 8) return (double)jpeg_islow_coeff(plane, side, by, bx, u, v);     // the JPEG-domain path: integers throughout
  double acc = 0.0;
  for (int i = 0; i < fs; i++) {
    double row = 0.0;
    for (int j = 0; j < fs; j++) row += ((double)plane[(size_t)(by * fs + i) * side + bx * fs + j] - 128.0) * dct_basis(fs, v, j);
    acc += dct_basis(fs, u, i) * row;
  }
  if (round_coeffs) acc = copysign(floor(fabs(acc) + 0.5), acc);
  return acc;
}
__global__ void k_dct_frontend(dct_args a) {
  const int C = a.n[0] + a.n[1] + a.n[2];
  const size_t total = (size_t)a.batch * C * a.S * a.S;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(x % a.S), oy = (int)((x / a.S) % a.S), c = (int)((x / ((size_t)a.S * a.S)) % C), b = (int)(x / ((size_t)a.S * a.S * C));
    const int pl = c < a.n[0] ? 0 : (c < a.n[0] + a.n[1] ? 1 : 2);
    const int k = a.idx[pl][c - (pl == 0 ? 0 : (pl == 1 ? a.n[0] : a.n[0] + a.n[1]))];
    const int u = k / a.fs, v = k % a.fs;
    const int grid = pl == 0 ? a.S : a.Sc, side = grid * a.fs;
    const uint8_t* plane = a.plane[pl] + (size_t)b * side * side;
    double val;
    if (grid == a.S) {
      val = dct_coeff(plane, side, a.fs, oy, ox, u, v, a.round_coeffs);
    } else {   // bilinear up-sampling of the coefficient grid
      const double sy = (oy + 0.5) * ((double)grid / a.S) - 0.5, sx = (ox + 0.5) * ((double)grid / a.S) - 0.5;
      const int y0 = (int)floor(sy), x0 = (int)floor(sx);
      const double fy = sy - y0, fx = sx - x0;
      const int y0c = min(max(y0, 0), grid - 1), y1c = min(max(y0 + 1, 0), grid - 1), x0c = min(max(x0, 0), grid - 1), x1c = min(max(x0 + 1, 0), grid - 1);
      const double top = dct_coeff(plane, side, a.fs, y0c, x0c, u, v, a.round_coeffs) * (1.0 - fx) + dct_coeff(plane, side, a.fs, y0c, x1c, u, v, a.round_coeffs) * fx;
      const double bot = dct_coeff(plane, side, a.fs, y1c, x0c, u, v, a.round_coeffs) * (1.0 - fx) + dct_coeff(plane, side, a.fs, y1c, x1c, u, v, a.round_coeffs) * fx;
      val = top * (1.0 - fy) + bot * fy;
      if (a.round_coeffs) val = rint(val);
    }
    a.out[x] = ((float)val - a.mean[c]) / a.stdv[c];
  }
}

// ------------------------------------------------------------------------------------------ f64 peak probe
__global__ void k_fp64_peak(double* out, int iters) {
  double a0 = threadIdx.x * 1e-9, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  const double m = 1.0000001, c = 1e-7;
  for (int i = 0; i < iters; i++) {
    a0 = __builtin_fma(a0, m, c); a1 = __builtin_fma(a1, m, c); a2 = __builtin_fma(a2, m, c); a3 = __builtin_fma(a3, m, c);
    a4 = __builtin_fma(a4, m, c); a5 = __builtin_fma(a5, m, c); a6 = __builtin_fma(a6, m, c); a7 = __builtin_fma(a7, m, c);
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}

}  // namespace dctfhe
