// Host emulation of the duo form of the general two-bit blind rotation (pbs_thread_duo of dct-cryptonets_amd/csrc/pbs_core.h:
// two ciphertexts per group of T = M / 4 threads, four points per thread, the geometry of pbs_kernel_duo<11, 1, 3, 4>): the radix-4
// transform's index math, the L2 warm-up range, whole bootstraps against the exact-arithmetic definition (oracle/tfhe_ref.c
// ref_pbs_mb2_batch), the odd tail, both write-back modes and the independence of the two slots.  Reuses the cases of emul_pbs.cpp;
// built by tests/test_pbs_duo_host.py with the Makefile's g++ line.
#define main emul_pbs_main
#include "emul_pbs.cpp"
#undef main

template <int LOGN, int K, int L, int P>
struct duo_rig {
  using G = pbs_geom<LOGN, K, L, P, 1>;
  static constexpr int N = G::N, M = G::M, T = G::T;
  std::vector<cplx> tw, wtab, zlut, bsk_dev;
  std::vector<unsigned char> shared;
  std::vector<uint64_t> accl;
  std::vector<uint32_t> pfd;
  duo_rig() : tw(G::F::TW_ELEMS), wtab(2 * N + 8), shared(2 * G::EXCH_BYTES), accl((size_t)2 * G::NL * N + 1), pfd(T) {
    fill_twiddles<G::LOGM, P>(tw.data());
    for (int m = 0; m < 2 * N; m++) { const long double a = 3.141592653589793238462643383279502884L * m / N; wtab[m] = cmk((double)cosl(a), (double)sinl(a)); }
    for (int m = 0; m < 8; m++) wtab[2 * N + m] = root64(8 * m);
    for (int j = 0; j < (1 << G::ZLO); j++) zlut.push_back(wtab[j]);
    for (int j = 0; j < (1 << G::ZHI); j++) zlut.push_back(wtab[(size_t)j << G::ZLO]);
  }
  pbs_args args(const uint64_t* ct, int n_in, int beta, const int64_t* table, int w, uint64_t* out, int D_out, int accumulate, uint64_t body_add, int pf_parts = 0, int pf_rank = 0, bool two_tables = true) {
    pbs_args A;
    A.ct_small = ct; A.n = n_in; A.beta = beta; A.bsk = bsk_dev.data(); A.table = table; A.w = w; A.out = out; A.D_out = D_out;
    A.accumulate = accumulate; A.body_add = body_add; A.bsk_wrap = 0; A.wtab = wtab.data(); A.zlut = two_tables ? zlut.data() : nullptr;
    A.twist = tw.data() + G::F::TW_TOTAL; A.pf_rank = pf_rank; A.pf_parts = pf_parts;
    return A;
  }
  template <class Sync>
  void run(const pbs_args (&A2)[2], int t, Sync&& sync) {
    pbs_thread_duo<LOGN, K, L, P>(A2, t, tw.data(), reinterpret_cast<cplx*>(shared.data()), accl.data(), pfd.data(), sync, sync);
  }
};

// `count` ciphertexts in duos, the last duo padded as the kernel pads it (its second slot redoes the last ciphertext in store mode into
// a sink); then one ciphertext in slot 0 and in slot 1 of one duo, and next to two different partners
template <int LOGN, int K, int L, int P>
static int run_case_duo(int n_in, int beta, int w, double sigma_bsk, int count) {
  using G = pbs_geom<LOGN, K, L, P, 1>;
  constexpr int N = G::N, M = G::M, T = G::T;
  const int D = K * N;
  std::vector<uint8_t> S(D), s(n_in);
  ref_gen_binary_key(11, D, S.data());
  ref_gen_binary_key(12, n_in, s.data());
  const int rows = (K + 1) * L, n = 3 * n_in / 2;
  std::vector<uint8_t> skey(n);
  ref_pair_secret(s.data(), n_in, skey.data());
  std::vector<uint64_t> bsk((size_t)n * rows * (K + 1) * N);
  ref_bsk_gen(skey.data(), n, S.data(), K, N, L, beta, sigma_bsk, 13, bsk.data());
  std::vector<uint64_t> phases(count), cts((size_t)count * (n_in + 1));
  for (int c = 0; c < count; c++) phases[c] = (uint64_t)((c * 5 + 1) % (1 << w)) << (63 - w);
  ref_lwe_encrypt_batch(s.data(), n_in, n_in, phases.data(), count, 1e-9, 14, cts.data());
  std::vector<int64_t> table(1 << w);
  for (int x = 0; x < (1 << w); x++) table[x] = (int64_t)(((x * 3 + 2) % (1 << w))) << (63 - w - 1);
  std::vector<uint64_t> ref_out((size_t)count * (D + 1));
  ref_pbs_mb2_batch(cts.data(), count, n_in, bsk.data(), K, N, L, beta, table.data(), w, nullptr, D, ref_out.data());

  duo_rig<LOGN, K, L, P> rig;
  rig.bsk_dev.resize((size_t)(n + PBS_PF_DIST * G::KEY_BLOCKS) * G::BSK_ELEMS_PER_KEYBIT);
  const int DW = D + 3;
  const uint64_t body_add = 0x9E3779B97F4A7C15ULL;
  std::vector<uint64_t> emu_out((size_t)count * (D + 1), 0x1234), wide_store((size_t)count * (DW + 1)), pre((size_t)count * (DW + 1)), sink((size_t)DW + 1);
  uint64_t fill = 77;
  for (auto& v : wide_store) v = ref_splitmix64(&fill);
  for (auto& v : pre) v = ref_splitmix64(&fill);
  std::vector<uint64_t> wide_acc = pre;
  struct write_back { uint64_t* out; int D_out, accumulate; uint64_t body_add; };
  const write_back passes[3] = {{emu_out.data(), D, 0, 0}, {wide_store.data(), DW, 0, body_add}, {wide_acc.data(), DW, 1, body_add}};
  // slot independence: ciphertext 0 as (slot 0, partner 1), (slot 1, partner 1 in slot 0), (slot 0, partner 2 % count), twice itself
  std::vector<uint64_t> indep((size_t)5 * (D + 1)), other((size_t)D + 1);
  {
    std::barrier bar(T);
    auto worker = [&](int t) {
      auto sync = [&] { bar.arrive_and_wait(); };
      const size_t npoly = (size_t)n * rows * (K + 1);
      for (size_t q = 0; q < npoly; q++)
        key_poly_to_fourier<LOGN, P>(bsk.data() + q * N, rig.bsk_dev.data() + q * M, t, rig.tw.data(), reinterpret_cast<cplx*>(rig.shared.data()), sync, sync);
      sync();
      for (const write_back& wb : passes)
        for (int c0 = 0; c0 < count; c0 += 2) {
          const bool tail = c0 + 1 >= count;
          const int c1 = tail ? c0 : c0 + 1;
          const pbs_args A2[2] = {rig.args(cts.data() + (size_t)c0 * (n_in + 1), n_in, beta, table.data(), w, wb.out + (size_t)c0 * (wb.D_out + 1), wb.D_out, wb.accumulate, wb.body_add),
                                  rig.args(cts.data() + (size_t)c1 * (n_in + 1), n_in, beta, table.data(), w, tail ? sink.data() : wb.out + (size_t)c1 * (wb.D_out + 1), wb.D_out,
                                           tail ? 0 : wb.accumulate, wb.body_add)};
          rig.run(A2, t, sync);
          sync();
        }
      const int pa = count > 1 ? 1 : 0, pb = count > 2 ? 2 : 0;
      const int slots[4][2] = {{0, pa}, {pa, 0}, {0, pb}, {0, 0}};
      for (int k = 0; k < 4; k++) {
        const int mine = k == 1 ? 1 : 0;      // the slot ciphertext 0 sits in
        uint64_t* o[2];
        o[mine] = indep.data() + (size_t)k * (D + 1);
        o[1 - mine] = k == 3 ? indep.data() + (size_t)4 * (D + 1) : other.data();
        const pbs_args A2[2] = {rig.args(cts.data() + (size_t)slots[k][0] * (n_in + 1), n_in, beta, table.data(), w, o[0], D, 0, 0),
                                rig.args(cts.data() + (size_t)slots[k][1] * (n_in + 1), n_in, beta, table.data(), w, o[1], D, 0, 0)};
        rig.run(A2, t, sync);
        sync();
      }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back(worker, t);
    for (auto& x : th) x.join();
  }
  std::vector<uint64_t> ph_ref(count), ph_emu(count);
  ref_lwe_phase_batch(S.data(), D, ref_out.data(), count, ph_ref.data());
  ref_lwe_phase_batch(S.data(), D, emu_out.data(), count, ph_emu.data());
  int bad = 0;
  double maxd = 0, maxe = 0;
  for (int c = 0; c < count; c++) {
    const int m = (int)(phases[c] >> (63 - w));
    const uint64_t want = (uint64_t)table[m];
    maxd = std::fmax(maxd, std::fabs((double)(int64_t)(ph_emu[c] - ph_ref[c])) / 18446744073709551616.0);
    maxe = std::fmax(maxe, std::fabs((double)(int64_t)(ph_emu[c] - want)) / 18446744073709551616.0);
    const int got = (int)(((ph_emu[c] + (1ULL << (63 - w - 2))) >> (63 - w - 1)) & ((1 << (w + 1)) - 1));
    if (got != (int)(want >> (63 - w - 1))) bad++;
  }
  int bad_store = 0, bad_acc = 0, bad_slot = 0;
  for (int c = 0; c < count; c++) {
    const uint64_t *e = emu_out.data() + (size_t)c * (D + 1), *st = wide_store.data() + (size_t)c * (DW + 1);
    const uint64_t *ac = wide_acc.data() + (size_t)c * (DW + 1), *pr = pre.data() + (size_t)c * (DW + 1);
    for (int j = 0; j < D; j++) { bad_store += st[j] != e[j]; bad_acc += ac[j] != pr[j] + e[j]; }
    for (int j = D; j < DW; j++) { bad_store += st[j] != 0; bad_acc += ac[j] != pr[j]; }
    bad_store += st[DW] != e[D] + body_add;
    bad_acc += ac[DW] != pr[DW] + e[D] + body_add;
  }
  for (int k = 0; k < 5; k++)
    for (int j = 0; j <= D; j++) bad_slot += indep[(size_t)k * (D + 1) + j] != emu_out[j];
  std::printf("duo N=%d k=%d l=%d P=%d T=%d n=%d count=%d: wrong=%d max|emu-ref|=%.3g max|emu-ideal|=%.3g; rows of D + 3 words: store mismatches=%d accumulate mismatches=%d; "
              "slot / partner mismatches=%d\n", N, K, L, P, T, n_in, count, bad, maxd, maxe, bad_store, bad_acc, bad_slot);
  return bad || maxe > std::ldexp(1.0, -(w + 4)) || bad_store || bad_acc || bad_slot;
}

// the warm-up contract for the duo's T (pf_guard_case of emul_pbs.cpp): the key buffer ends on an inaccessible page
template <int LOGN, int K, int L, int P>
static int pf_guard_duo(int n_in, int pf_parts) {
  using G = pbs_geom<LOGN, K, L, P, 1>;
  constexpr int N = G::N, T = G::T;
  const int D = K * N;
  const size_t bytes = ((size_t)(3 * n_in / 2) + (size_t)PBS_PF_DIST * G::KEY_BLOCKS) * G::BSK_ELEMS_PER_KEYBIT * 16;
  const size_t page = 4096, span = (bytes + page - 1) / page * page;
  unsigned char* map = (unsigned char*)mmap(nullptr, span + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (map == MAP_FAILED) { std::printf("mmap failed\n"); return 1; }
  if (mprotect(map + span, page, PROT_NONE)) { std::printf("mprotect failed\n"); return 1; }
  duo_rig<LOGN, K, L, P> rig;
  std::vector<uint64_t> ct(n_in + 1, 0x0123456789abcdefULL), out((size_t)2 * (D + 1));
  std::vector<int64_t> table(16, 1LL << 58);
  const int ranks[2] = {0, pf_parts > 0 ? pf_parts - 1 : 0};
  for (int pf_rank : ranks) {
    std::barrier bar(T);
    auto worker = [&](int t) {
      auto sync = [&] { bar.arrive_and_wait(); };
      pbs_args A2[2];
      for (int c = 0; c < 2; c++) {
        A2[c] = rig.args(ct.data(), n_in, 10, table.data(), 4, out.data() + (size_t)c * (D + 1), D, 0, 0, pf_parts, pf_rank, false);
        A2[c].bsk = reinterpret_cast<cplx*>(map + (span - bytes));       // the buffer ends exactly where the guard page starts
      }
      rig.run(A2, t, sync);
    };
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back(worker, t);
    for (auto& x : th) x.join();
  }
  munmap(map, span + page);
  std::printf("warm-up range duo N=%d k=%d l=%d P=%d n=%d pf_parts=%d: inside the key + %d iterations of padding\n", N, K, L, P, n_in, pf_parts, PBS_PF_DIST);
  return 0;
}

int main() {
  int fail = 0;
  fail |= fft_case<9, 4>();
  fail |= fft_case<11, 4>();
  fail |= layout_case<9, 4>();
  fail |= layout_case<11, 4>();
  fail |= pf_guard_duo<11, 1, 3, 4>(4, 16);     // pf_parts as launched, then the other legal settings
  fail |= pf_guard_duo<11, 1, 3, 4>(4, 8);
  fail |= pf_guard_duo<11, 1, 3, 4>(4, 32);
  fail |= pf_guard_duo<11, 1, 3, 4>(2, 0);
  fail |= run_case_duo<9, 1, 3, 4>(16, 7, 4, 1e-12, 5);      // the same thread program on a smaller ring, odd tail
  fail |= run_case_duo<11, 1, 3, 4>(8, 11, 4, 1e-14, 3);     // the shipped geometry and T4r2's gadget base
  fail |= run_case_duo<11, 1, 3, 4>(4, 11, 4, 1e-14, 1);     // a lone ciphertext: both slots hold it
  std::printf(fail ? "EMUL FAIL\n" : "EMUL OK\n");
  return fail;
}
