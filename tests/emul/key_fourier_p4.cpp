// key_fourier.cpp's host emulation of key_poly_to_fourier at four points per thread: the transform behind the device's Fourier key of
// the duo tier (pbs_kernel_duo<11, 1, 3, 4>), and the same thread program on a smaller ring.  Same command line:
//   key_fourier_p4 LOGN P in.bin out.bin
// Built by tests/test_pbs_duo_host.py with the g++ line of tests/emul/Makefile.
#define main key_fourier_main
#include "key_fourier.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: key_fourier_p4 LOGN P in.bin out.bin\n"); return 2; }
  const int logN = std::atoi(argv[1]), P = std::atoi(argv[2]);
  if (logN == 9 && P == 4) return run<9, 4>(argv[3], argv[4]);
  if (logN == 11 && P == 4) return run<11, 4>(argv[3], argv[4]);
  std::fprintf(stderr, "no instantiation for logN=%d P=%d\n", logN, P);
  return 2;
}
