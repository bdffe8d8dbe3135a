// Host emulation of the four-level blind rotation pbs_kernel<11, 1, 4, 8> (tier T5r of dctfhe/params.py default_params_5bit):
// the deferred-digit packing (three 10-bit digits in one 32-bit word), the gadget decomposition against the oracle, the L2
// warm-up range, and the whole bootstrap against the CPU oracle (oracle/tfhe_ref.c ref_pbs_batch, what oracle.ref_loader.pbs
// calls).  Reuses the cases of emul_pbs.cpp; built by tests/test_bitwidth5_host.py with the Makefile's g++ line.
#define main emul_pbs_main
#include "emul_pbs.cpp"
#undef main

// every digit value a base-2^10 gadget produces, at every field of the packed word, with its neighbours set to extremes
static int pack_case() {
  int bad = 0;
  const int32_t ext[3] = {-512, 0, 511};
  for (int lev = 1; lev < 4; lev++)
    for (int v = -512; v < 512; v++)
      for (int e : ext) {
        int32_t dg[4] = {0, e, e, e};
        dg[lev] = v;
        const uint32_t pk = pack_digits<4>(dg);
        bad += unpack_digit<4, 1>(pk) != (double)dg[1];
        bad += unpack_digit<4, 2>(pk) != (double)dg[2];
        bad += unpack_digit<4, 3>(pk) != (double)dg[3];
      }
  std::printf("four-level digit packing: %d mismatches\n", bad);
  return bad != 0;
}

int main() {
  int fail = 0;
  static_assert(packed_digit_bits<4>() == 10 && packed_digit_bits<3>() == 16, "packed field widths");
  fail |= pack_case();
  const int dbad = decompose_one<4>(10) + decompose_one<4>(9);
  std::printf("four-level decompose vs oracle: %d mismatches\n", dbad);
  fail |= dbad != 0;
  fail |= pf_guard_case<11, 1, 4, 8>(3, 0, 16);
  fail |= run_case<11, 1, 4, 8>(12, 10, 5, 1e-14);     // T5r's geometry and gadget, 5-bit table
  fail |= run_case<9, 1, 4, 8>(16, 10, 4, 1e-13);      // the same thread program on a smaller ring (two waves' worth of lanes)
  std::printf(fail ? "EMUL FAIL\n" : "EMUL OK\n");
  return fail;
}
