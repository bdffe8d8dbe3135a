// san_main.cpp -- every entry point of include/dctfhe_client.h once, at tiny parameters, in a program of its own (no Python): built
// together with csrc/client_host.cpp under -fsanitize=address,undefined by tests/test_host_client.py, which requires exit 0 and an
// empty stderr.  Buffers are exactly as large as the header says, so a word written past any of them is seen.  Also: a size query, a
// too-small buffer, a truncated public-key blob, count == 0, and the refusals that must leave their outputs alone.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dctfhe_client.h"

#define REQUIRE(x)                                                                              \
  do {                                                                                          \
    if (!(x)) {                                                                                 \
      printf("san_main: %s failed at line %d: %s\n", #x, __LINE__, dctfhe_host_last_error());  \
      return 1;                                                                                 \
    }                                                                                           \
  } while (0)

static dctfhe_tier tier(int n, int k, int logN, int l, int beta, int lk, int betak, int share, int unroll) {
  dctfhe_tier t;
  memset(&t, 0, sizeof t);
  t.n = n; t.k = k; t.logN = logN; t.l = l; t.beta = beta; t.lk = lk; t.betak = betak; t.ksk_share = share; t.unroll = unroll;
  t.lwe_sigma = 1.0 / (1 << 20); t.glwe_sigma = 1.0 / (1ULL << 40);
  return t;
}

int main() {
  // the custom set of tests/host_client_ref.py: k = 2, a pair secret, a shared key-switch key, grids of 2, 4 and 8 limbs; an input
  // width (517) that ends inside a generator block
  dctfhe_params P;
  memset(&P, 0, sizeof P);
  P.D = 2048; P.n_max = 8; P.n_tiers = 4; P.input_dim = 517; P.input_sigma = 1.0 / (1ULL << 45);
  P.tiers[0] = tier(6, 2, 8, 2, 14, 2, 4, -1, 1);
  P.tiers[1] = tier(8, 2, 10, 1, 23, 5, 4, -1, 2);
  P.tiers[2] = tier(8, 1, 9, 3, 12, 7, 4, -1, 1);
  P.tiers[3] = tier(6, 1, 10, 2, 12, 2, 4, 0, 1);
  uint8_t seed[32], nonce[16];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
  for (int i = 0; i < 16; i++) nonce[i] = (uint8_t)(7 * i);

  REQUIRE(dctfhe_host_version() == 1 && dctfhe_host_threads() >= 1);
  dctfhe_host_client_key* ck = nullptr;
  {
    dctfhe_params bad = P;
    bad.tiers[0].unroll = 2;
    REQUIRE(dctfhe_host_client_key_create(&bad, seed, &ck) != 0 && ck == nullptr && strlen(dctfhe_host_last_error()) > 0);
    REQUIRE(dctfhe_host_client_key_create(nullptr, seed, &ck) != 0);
  }
  REQUIRE(dctfhe_host_client_key_create(&P, seed, &ck) == 0 && ck);
  REQUIRE(dctfhe_host_client_key_set_encrypt_nonce(ck, nonce) == 0);
  REQUIRE(dctfhe_host_client_key_set_encrypt_counter(ck, 5) == 0);
  REQUIRE(dctfhe_host_client_key_set_encrypt_counter(ck, 1ULL << 47) != 0);
  std::vector<uint8_t> S(P.D), s(P.n_max);
  REQUIRE(dctfhe_host_client_key_export_secret(ck, S.data(), s.data()) == 0);
  uint8_t pub[32], enc_pub[32];
  REQUIRE(dctfhe_host_client_key_public_keys(ck, pub, enc_pub) == 0 && dctfhe_host_client_key_public_keys(ck, nullptr, nullptr) == 0);

  // encrypt (compact and full width), seeded, decrypt: the phases come back within the noise
  const size_t count = 9;
  std::vector<uint64_t> ph(count), back(count), bodies(count);
  for (size_t i = 0; i < count; i++) ph[i] = (uint64_t)(i + 1) << 58;
  for (int dim : {517, 2048}) {
    std::vector<uint64_t> rows(count * (size_t)(dim + 1));
    REQUIRE(dctfhe_host_client_key_set_encrypt_counter(ck, 5) == 0);
    REQUIRE(dctfhe_host_encrypt_rows(ck, ph.data(), count, dim, rows.data()) == 0);
    REQUIRE(dctfhe_host_decrypt_rows(ck, rows.data(), count, dim, back.data()) == 0);
    for (size_t i = 0; i < count; i++) REQUIRE(llabs((long long)(back[i] - ph[i])) < (1LL << 24));
    uint8_t mk[32];
    uint64_t stream = 0;
    REQUIRE(dctfhe_host_client_key_set_encrypt_counter(ck, 5) == 0);
    REQUIRE(dctfhe_host_encrypt_seeded(ck, ph.data(), count, mk, &stream, bodies.data()) == 0);
    REQUIRE(stream == 256 + (6ULL << 16) && memcmp(mk, enc_pub, 32) == 0);
    for (size_t i = 0; i < count; i++) REQUIRE(bodies[i] == rows[i * (size_t)(dim + 1) + dim]);
    REQUIRE(dctfhe_host_encrypt_rows(ck, ph.data(), count, 516, rows.data()) != 0);
    REQUIRE(dctfhe_host_encrypt_rows(ck, nullptr, 0, dim, nullptr) == 0);
    REQUIRE(dctfhe_host_encrypt_seeded(ck, nullptr, 0, mk, &stream, nullptr) == 0 && stream == 0);
  }
  REQUIRE(dctfhe_host_decrypt_rows(ck, bodies.data(), count, 0, back.data()) == 0 && back[3] == bodies[3]);
  REQUIRE(dctfhe_host_decrypt_rows(ck, bodies.data(), count, 2049, back.data()) != 0);

  // packed rows (odd row length: rows are not 4-byte aligned) and ring-packed words (a partial last group)
  {
    const int n = 6;
    std::vector<uint16_t> rows(count * (n + 1));
    for (size_t i = 0; i < rows.size(); i++) rows[i] = (uint16_t)(i * 2654435761u >> 7);
    REQUIRE(dctfhe_host_decrypt_packed(ck, n, rows.data(), count, back.data()) == 0);
    uint32_t want = rows[n];
    for (int j = 0; j < n; j++) want -= s[j] ? rows[j] : 0;
    REQUIRE(back[0] == (uint64_t)(want & 0xFFFFu) << 48);
    REQUIRE(dctfhe_host_decrypt_packed(ck, 9, rows.data(), count, back.data()) != 0);
    const int logN = 5;
    const size_t m = 32 + 7, words = 2 * 32 + m;      // two groups of N_p mask words, then one body word per result
    std::vector<uint16_t> w(words);
    std::vector<uint64_t> out(m);
    for (size_t i = 0; i < words; i++) w[i] = (uint16_t)(i * 40503u);
    REQUIRE(dctfhe_host_decrypt_ring(ck, logN, w.data(), m, out.data()) == 0);
    REQUIRE(dctfhe_host_decrypt_ring(ck, 4, w.data(), m, out.data()) != 0 && dctfhe_host_decrypt_ring(ck, 12, w.data(), m, out.data()) != 0);
  }

  // the three exports: size query, too-small buffer (nothing written), the blob itself
  size_t need = 0;
  REQUIRE(dctfhe_host_eval_keys_export_compressed(ck, nullptr, 0, &need) == 0 && need > 48);
  {
    std::vector<uint8_t> small(need - 1, 0xAB), blob(need);
    size_t n2 = 0;
    REQUIRE(dctfhe_host_eval_keys_export_compressed(ck, small.data(), small.size(), &n2) != 0 && n2 == need);
    for (uint8_t b : small) REQUIRE(b == 0xAB);
    REQUIRE(dctfhe_host_eval_keys_export_compressed(ck, blob.data(), blob.size(), &n2) == 0);
    uint64_t total;
    memcpy(&total, blob.data() + 8, 8);
    REQUIRE(total == need && memcmp(blob.data(), "DEVC", 4) == 0 && memcmp(blob.data() + 16 + sizeof(dctfhe_params), pub, 32) == 0);
  }
  {
    size_t pn = 0, n2 = 0;
    REQUIRE(dctfhe_host_pack_key_export(ck, 8, 2, 12, 1.0 / (1ULL << 40), nullptr, 0, &pn) == 0 && pn == 72 + (size_t)8 * 2 * 256 * 8);
    std::vector<uint8_t> small(pn - 8, 0xCD), blob(pn);
    REQUIRE(dctfhe_host_pack_key_export(ck, 8, 2, 12, 1.0 / (1ULL << 40), small.data(), small.size(), &n2) != 0);
    for (uint8_t b : small) REQUIRE(b == 0xCD);
    REQUIRE(dctfhe_host_pack_key_export(ck, 8, 2, 12, 1.0 / (1ULL << 40), blob.data(), blob.size(), &n2) == 0 && memcmp(blob.data(), "DRPK", 4) == 0);
    REQUIRE(dctfhe_host_pack_key_export(ck, 12, 1, 16, 0.0, nullptr, 0, &n2) != 0);      // N_p = 4096 > D
    REQUIRE(dctfhe_host_pack_key_export(ck, 8, 4, 16, 0.0, nullptr, 0, &n2) != 0);       // 64 gadget bits
  }
  size_t kn = 0;
  REQUIRE(dctfhe_host_public_key_export(ck, 8, 1.0 / (1ULL << 40), nullptr, 0, &kn) == 0 && kn == 64 + 256 * 8);
  std::vector<uint8_t> kblob(kn);
  {
    size_t n2 = 0;
    std::vector<uint8_t> small(kn - 1, 0xEF);
    REQUIRE(dctfhe_host_public_key_export(ck, 8, 1.0 / (1ULL << 40), small.data(), small.size(), &n2) != 0);
    for (uint8_t b : small) REQUIRE(b == 0xEF);
    REQUIRE(dctfhe_host_public_key_export(ck, 8, 1.0 / (1ULL << 40), kblob.data(), kblob.size(), &n2) == 0);
    REQUIRE(dctfhe_host_public_key_export(ck, 10, 0.0, nullptr, 0, &n2) != 0);          // N_e = 1024 > input_dim
  }

  // the data owner: a truncated blob, a blob cut inside its header, a wrong magic; then draws and an encryption of two groups and a bit
  dctfhe_host_public_key* pk = nullptr;
  {
    std::vector<uint8_t> cut(kblob.begin(), kblob.end() - 8), head(kblob.begin(), kblob.begin() + 20), wrong(kblob);
    wrong[0] ^= 1;
    REQUIRE(dctfhe_host_public_key_import(cut.data(), cut.size(), &pk) != 0 && pk == nullptr);
    REQUIRE(dctfhe_host_public_key_import(head.data(), head.size(), &pk) != 0 && pk == nullptr);
    REQUIRE(dctfhe_host_public_key_import(wrong.data(), wrong.size(), &pk) != 0 && pk == nullptr);
  }
  REQUIRE(dctfhe_host_public_key_import(kblob.data(), kblob.size(), &pk) == 0 && pk);
  int logN = 0;
  double sigma = -1;
  REQUIRE(dctfhe_host_public_key_info(pk, &logN, &sigma) == 0 && logN == 8 && sigma == 1.0 / (1ULL << 40));
  REQUIRE(dctfhe_host_public_key_info(pk, nullptr, nullptr) == 0);
  REQUIRE(dctfhe_host_public_key_set_encrypt_seed(pk, seed) == 0);
  {
    const size_t N = 256, m = 2 * N + 5, nmask = 3 * N;
    std::vector<uint8_t> u(nmask);
    std::vector<int64_t> e1(nmask), e2(m);
    std::vector<uint64_t> phases(m), words(nmask + m), rows_back(m);
    for (size_t i = 0; i < m; i++) phases[i] = (uint64_t)(i % 16) << 59;
    REQUIRE(dctfhe_host_public_key_draws(pk, 0, m, u.data(), e1.data(), e2.data()) == 0);
    REQUIRE(dctfhe_host_public_key_draws(pk, 0, 0, u.data(), e1.data(), e2.data()) != 0);
    REQUIRE(dctfhe_host_encrypt_public(pk, phases.data(), m, words.data()) == 0);
    REQUIRE(dctfhe_host_encrypt_public(pk, phases.data(), 0, words.data()) != 0);
    // slot 0 of every group is the LWE row (C_a[0], -C_a[N-1], ..., -C_a[1] | C_b[0]) under the first N key bits: decrypt it
    for (size_t g = 0; g < 3; g++) {
      std::vector<uint64_t> row(N + 1);
      const uint64_t* grp = words.data() + g * 2 * N;
      row[0] = grp[0];
      for (size_t j = 1; j < N; j++) row[j] = 0 - grp[N - j];
      row[N] = grp[N];
      uint64_t got = 0;
      REQUIRE(dctfhe_host_decrypt_rows(ck, row.data(), 1, (int)N, &got) == 0);
      REQUIRE(llabs((long long)(got - phases[g * N])) < (1LL << 40));
    }
  }
  REQUIRE(dctfhe_host_public_key_destroy(pk) == 0 && dctfhe_host_public_key_destroy(nullptr) == 0);
  REQUIRE(dctfhe_host_client_key_destroy(ck) == 0 && dctfhe_host_client_key_destroy(nullptr) == 0);
  printf("SAN_MAIN OK\n");
  return 0;
}
