"""The duo form of the general two-bit bootstrap without a GPU: pbs_thread_duo and the radix-4 transform compiled for the host
(tests/emul/emul_pbs_duo.cpp) against the exact-arithmetic oracle, and key_poly_to_fourier at four points per thread -- the transform
behind the device's key of that tier -- against the long-double transform with the ratios of tests/key_material_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import key_material_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
U = np.uint64


def test_emulated_duo_bootstrap(oracle, tmp_path):
    oracle_dir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-C", oracle_dir], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "emul_pbs_duo")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-pthread", "-o", exe, os.path.join(EMUL, "emul_pbs_duo.cpp"), "-L" + oracle_dir,
                           "-ltfhe_ref", "-Wl,-rpath," + oracle_dir, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "EMUL OK" in out.stdout, out.stdout + out.stderr
    # the shipped geometry: odd tail, a lone ciphertext, both write-back modes, the two slots; the warm-up range as launched
    for count in (3, 1):
        line = [l for l in out.stdout.splitlines() if l.startswith("duo N=2048 k=1 l=3 P=4 T=256") and "count=%d:" % count in l]
        assert len(line) == 1, out.stdout
        assert "wrong=0" in line[0] and "store mismatches=0 accumulate mismatches=0; slot / partner mismatches=0" in line[0], line[0]
    assert "warm-up range duo N=2048 k=1 l=3 P=4 n=4 pf_parts=16: inside the key" in out.stdout
    assert "layout N=2048 P=4: " in out.stdout and "fft N=2048 P=4 T=256 passes=5" in out.stdout


@pytest.mark.parametrize("logN", [11, 9])
def test_emulated_key_poly_to_fourier_at_four_points_per_thread(tmp_path, logN):
    """position rule, scaling and accuracy (rms within 3x, largest within 4x of numpy's double-precision transform), as
    tests/test_key_material_host.py holds the other geometries"""
    P = 4
    exe = str(tmp_path / "key_fourier_p4")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-pthread", "-o", exe, os.path.join(EMUL, "key_fourier_p4.cpp"), "-lm"])
    N, M = 1 << logN, 1 << (logN - 1)
    rng = np.random.default_rng(400 + logN)
    polys = rng.integers(0, 2 ** 64, (4, N), dtype=U)
    polys[1] = rng.integers(-2 ** 24, 2 ** 24, N, dtype=np.int64).view(U)
    polys[2, 0] += U(1) << U(53)
    polys[3, :4] = [2 ** 63, 2 ** 63 - 1, 2 ** 64 - 1, 0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    polys.tofile(src)
    subprocess.check_call([exe, str(logN), str(P), src, dst], timeout=120)
    dev = np.fromfile(dst, np.complex128).reshape(4, M)
    ref, yard = K.fourier_key_reference(polys, logN, P)
    rms, mx, rel = K.error_ratios(dev, ref, yard)
    print("host thread program logN %d P %d: rms ratio %.2f, max ratio %.2f, yardstick %.2e relative rms" % (logN, P, rms, mx, rel))
    assert rel < 1e-15
    assert rms <= 3.0 and mx <= 4.0, (rms, mx)
    wrong = ref[..., np.roll(np.arange(M), 1)]
    assert np.abs(dev.astype(np.clongdouble) - wrong).max() > 1e-3 * np.abs(ref).max()
    # the same frequencies as the blob's P = 8 order, entry for entry of the permutation the library applies on export and import
    if logN == 11:
        f4, f8 = K.entry_frequencies(logN, 4), K.entry_frequencies(logN, 8)
        assert sorted(f4) == sorted(f8) == list(range(M))
