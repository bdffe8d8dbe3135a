// client_shared.h -- what the device kernels (kernels.h, built by hipcc for gfx950) and the host client library (client_host.cpp, plain
// C++17, no HIP) must agree on word for word: the generator, its stream ids, the key-switch grid and the arithmetic of a noise draw.
// Everything here compiles with and without hipcc; the loops around it are restated on each side (kernels.h / client_host.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DCTFHE_SHARED __host__ __device__ inline
#else
#define DCTFHE_SHARED inline
#endif

namespace dctfhe {

// ------------------------------------------------------------------------------------------ rng
// Counter-based CSPRNG: ChaCha20 (D. J. Bernstein's layout: 256-bit key, 64-bit block counter, 64-bit stream id), one 64-byte
// block = eight u64 outputs; (key, stream, index) -> 64 bits, any index in any order, so every kernel draws exactly the
// values keygen drew (the test views regenerate keys from the client handle).  Two keys per client: the SECRET key feeds the
// secret-key bits and every noise term; the PUBLIC key (one ChaCha block of the secret one) feeds the ciphertext / key masks.
// The reference's runtime (Concrete) seeds an AES-CTR generator the same way.
struct rng_key { uint32_t k[8]; };

#define DCTFHE_QR(a, b, c, d)                                   \
  a += b; d ^= a; d = (d << 16) | (d >> 16);                    \
  c += d; b ^= c; b = (b << 12) | (b >> 20);                    \
  a += b; d ^= a; d = (d << 8) | (d >> 24);                     \
  c += d; b ^= c; b = (b << 7) | (b >> 25);

// one ChaCha20 block; out[16] little-endian words
DCTFHE_SHARED void chacha20_block(const rng_key& key, uint64_t stream, uint64_t block, uint32_t* out) {
  const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                           key.k[4], key.k[5], key.k[6], key.k[7], (uint32_t)block, (uint32_t)(block >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
  uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7], x8 = in[8], x9 = in[9],
           x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
#pragma unroll
  for (int r = 0; r < 10; r++) {
    DCTFHE_QR(x0, x4, x8, x12) DCTFHE_QR(x1, x5, x9, x13) DCTFHE_QR(x2, x6, x10, x14) DCTFHE_QR(x3, x7, x11, x15)
    DCTFHE_QR(x0, x5, x10, x15) DCTFHE_QR(x1, x6, x11, x12) DCTFHE_QR(x2, x7, x8, x13) DCTFHE_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + in[0]; out[1] = x1 + in[1]; out[2] = x2 + in[2]; out[3] = x3 + in[3]; out[4] = x4 + in[4]; out[5] = x5 + in[5];
  out[6] = x6 + in[6]; out[7] = x7 + in[7]; out[8] = x8 + in[8]; out[9] = x9 + in[9]; out[10] = x10 + in[10]; out[11] = x11 + in[11];
  out[12] = x12 + in[12]; out[13] = x13 + in[13]; out[14] = x14 + in[14]; out[15] = x15 + in[15];
}
// (key, stream, index) -> 64 uniform bits: word pair (index & 7) of block (index >> 3)
DCTFHE_SHARED uint64_t rnd64(const rng_key& key, uint64_t stream, uint64_t idx) {
  uint32_t o[16];
  chacha20_block(key, stream, idx >> 3, o);
  uint64_t v = 0;
#pragma unroll
  for (int w = 0; w < 8; w++)
    if ((int)(idx & 7) == w) v = (uint64_t)o[2 * w] | ((uint64_t)o[2 * w + 1] << 32);
  return v;
}

// stream ids.  Masks are drawn from the PUBLIC key at stream s, the matching noise from the SECRET key at stream s + 1.
enum : uint64_t { STREAM_BIGKEY = 1, STREAM_SMALLKEY = 2, STREAM_PUBKEY = 3, STREAM_ENCKDF = 4, STREAM_KSK = 16, STREAM_BSK_MASK = 64, STREAM_ENC = 256 };

// Precision of a key-switch key: the torus grid its words live on, 2^-(8 limbs).  The finest gadget level sits at 2^-(lk betak) and the
// row noise (sigma_lwe >= 2^-19 on every shipped tier) at least 6 bits above the grid: limbs >= (lk betak + 6) / 8, as a power of two
// (the matrix-core epilogue folds a word's limbs with lane shuffles).  Table tiers (9 levels of base 4): 4 limbs; one-bit tiers (5
// levels): 2 limbs -- a half and a quarter of round 2's GEMM.
DCTFHE_SHARED int ks_limbs(int lk, int betak) {
  const int bits = lk * betak + 6;
  return bits <= 16 ? 2 : bits <= 32 ? 4 : 8;
}

// cos(pi x).  The device has the math library's cospi; the host reduces the argument exactly (x - 2 rint(x / 2) and the quadrant are
// exact in f64) and calls libm on |r| <= 1/4, where cos and sin lose nothing to the size of their argument.  Two implementations of one
// function: a value may differ in its last unit, and with it a noise term (include/dctfhe_client.h, "The Gaussian").
DCTFHE_SHARED double shared_cospi(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return cospi(x);
#else
  const double pi = 3.14159265358979323846;
  double r = fabs(x);
  r -= 2.0 * floor(r * 0.5);                    // [0, 2)
  if (r > 1.0) r = 2.0 - r;                     // cos(pi r) = cos(pi (2 - r)): [0, 1]
  if (r <= 0.25) return cos(pi * r);
  if (r < 0.75) return sin(pi * (0.5 - r));
  return -cos(pi * (1.0 - r));
#endif
}

// The Gaussian draw of generator words w1 = word(2 idx), w2 = word(2 idx + 1): Box-Muller, times sigma, as a torus element.  g sigma
// is reduced to [-1/2, 1/2] before it is scaled, so that the conversion is defined for every sigma (x - rint(x) is exact, and the
// identity for |x| < 1/2: every draw of the key material and of an encryption is what it was).
DCTFHE_SHARED int64_t gauss_torus_words(uint64_t w1, uint64_t w2, double sigma) {
  const double u1 = ((double)(w1 >> 11) + 1.0) * (1.0 / 9007199254740992.0);
  const double u2 = ((double)(w2 >> 11)) * (1.0 / 9007199254740992.0);
  const double g = sqrt(-2.0 * log(u1)) * shared_cospi(2.0 * u2);
  const double x = g * sigma;
  return (int64_t)rint((x - rint(x)) * 18446744073709551616.0);
}

}  // namespace dctfhe
