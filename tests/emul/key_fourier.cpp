// Host emulation of key_poly_to_fourier (dct-cryptonets_amd/csrc/pbs_core.h), the thread program behind k_bsk_fourier: T std::threads
// play the T lanes of one polynomial, a std::barrier plays s_barrier, a heap array plays LDS.
//   key_fourier LOGN P in.bin out.bin     in: npoly x N u64 (standard-domain key polynomials); out: npoly x M complex doubles, the
//                                         evaluation-key blob's layout
// tests/test_key_material_host.py compares the output with a long-double transform through the documented position rule.  Test
// infrastructure only; built by that test with the g++ line of tests/emul/Makefile.
#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../dct-cryptonets_amd/csrc/pbs_core.h"

using namespace dctfhe;

template <int LOGN, int P>
static int run(const char* in_path, const char* out_path) {
  constexpr int N = 1 << LOGN, M = N / 2;
  using F = fft_geom<LOGN - 1, P>;
  constexpr int T = F::T;
  std::FILE* f = std::fopen(in_path, "rb");
  if (!f) { std::perror(in_path); return 2; }
  std::vector<uint64_t> polys;
  uint64_t buf[4096];
  for (size_t got; (got = std::fread(buf, 8, 4096, f)) > 0;) polys.insert(polys.end(), buf, buf + got);
  std::fclose(f);
  if (polys.empty() || polys.size() % N) { std::fprintf(stderr, "%zu words are not polynomials of %d\n", polys.size(), N); return 2; }
  const size_t npoly = polys.size() / N;
  std::vector<cplx> tw(F::TW_ELEMS), exch(F::EXCH_ELEMS), out(npoly * M);
  fill_twiddles<LOGN - 1, P>(tw.data());
  std::barrier bar(T);
  auto worker = [&](int t) {
    auto sync = [&] { bar.arrive_and_wait(); };
    for (size_t q = 0; q < npoly; q++) {
      key_poly_to_fourier<LOGN, P>(polys.data() + q * N, out.data() + q * M, t, tw.data(), exch.data(), sync, sync);
      sync();   // the next polynomial reuses the exchange buffer
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++) th.emplace_back(worker, t);
  for (auto& x : th) x.join();
  f = std::fopen(out_path, "wb");
  if (!f) { std::perror(out_path); return 2; }
  const size_t put = std::fwrite(out.data(), sizeof(cplx), out.size(), f);
  return std::fclose(f) != 0 || put != out.size() ? 2 : 0;
}

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: key_fourier LOGN P in.bin out.bin\n"); return 2; }
  const int logN = std::atoi(argv[1]), P = std::atoi(argv[2]);
#define CASE(LN, P_) if (logN == LN && P == P_) return run<LN, P_>(argv[3], argv[4]);
  CASE(8, 8) CASE(9, 16) CASE(9, 8) CASE(10, 8) CASE(11, 8) CASE(12, 8) CASE(13, 8)
#undef CASE
  std::fprintf(stderr, "no instantiation for logN=%d P=%d\n", logN, P);
  return 2;
}
