"""Exact 5-bit trunks (CPU side): the 5-bit catalogue (dctfhe/params.py default_params_5bit) keeps every benchmark trunk inside the exact
budget, leaves the 4-bit catalogue and its circuits byte for byte as they were, passes the library's parameter gate, and the four-level
blind rotation of its refresh tier T5r matches the CPU oracle in host emulation."""
import ctypes as C
import hashlib
import os
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# recorded from the parent commit (bench.py's calibration batches, seed-0 models, rounding_threshold_bits=6)
SHA_4BIT = {
    "r20_24_16": "230c71dca425913a0001fdb4804f71a8cb4db53ee5b81edcdf44853df8de33f9",
    "r18_3_32": "25483451507a3ca9093bc79dec4d822e8233c85380b571ab8c43110b423e6fb2",
}
SHA_DEFAULT_C_PARAMS = "055ea5c28b3529faf9f54b8f1bda6f6b43f72ff1f7f5f135834c7e3e595b2993"


def _compile(name, bit_width):
    import bench
    from dctfhe import compile as cc, models
    factory, in_ch, img, make_batch, _ = bench.CONFIGS[name]
    calib = make_batch(16 if name == "r18_48_112" else 100, 7)
    model = getattr(models, factory)(bit_width=bit_width, in_channels=in_ch, img_size=img, seed=0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c = cc.compile_model(model, calib, rounding_threshold_bits=6, n_bits=5)
    return c, [str(x.message) for x in w if "dctfhe" in str(x.message)]


@pytest.mark.parametrize("name", ["r20_24_16", "r20_3_32", "r18_3_32", "r18_48_112"])
def test_5bit_trunks_compile_exact(name):
    from dctfhe import params as P
    c, warns = _compile(name, 5)
    assert not warns, warns
    assert c.worst_site_failure <= 1e-12, c.worst_site_failure
    names = [t.name for t in c.param_set.tiers]
    assert names == [t.name for t in P.default_params_5bit().tiers]
    counts = c.pbs_counts()
    assert counts.get("T5r", 0) > 0 and "T6" not in counts          # 5-bit conv-feeding activations refresh on N = 2048
    t5r = c.param_set.tiers[names.index("T5r")]
    assert (t5r.k, t5r.N, t5r.l, t5r.beta) == (1, 2048, 4, 10)
    rep = c.report()
    assert "tier 9 T5r: n=856 k=1 N=2048 l=4 beta=10" in rep and "tier=T5r" in rep


def test_catalogue_selection():
    from dctfhe import compile as cc, models, params as P
    from dctfhe.synthetic import synthetic_dct_batch
    calib = synthetic_dct_batch(16, seed=7)
    c5 = cc.compile_model(models.ResNet20QAT(5, 24, 16), calib)
    assert [t.n for t in c5.param_set.tiers] == [t.n for t in P.default_params_5bit().tiers]
    c4 = cc.compile_model(models.ResNet20QAT(4, 24, 16), calib)
    assert [t.as_dict() for t in c4.param_set.tiers] == [t.as_dict() for t in P.default_params().tiers]
    # an explicit param_set and tier_policy="p_error" behave as before
    c5x = cc.compile_model(models.ResNet20QAT(5, 24, 16), calib, param_set=P.default_params())
    assert "T5r" not in [t.name for t in c5x.param_set.tiers]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c5p = cc.compile_model(models.ResNet20QAT(5, 24, 16), calib, p_error=0.01, tier_policy="p_error")
    assert [t.name for t in c5p.param_set.tiers] == [t.name for t in P.params_for_p_error(0.01).tiers]
    assert P.params_for_bit_width(4).tiers == P.default_params().tiers
    assert P.params_for_bit_width(6).tiers == P.default_params().tiers


def test_4bit_circuits_unchanged():
    from dctfhe import params as P
    for name, want in SHA_4BIT.items():
        c, _ = _compile(name, 4)
        assert hashlib.sha256(c.blob).hexdigest() == want, name
    cp = P.to_c_params(P.default_params())
    assert hashlib.sha256(bytes(memoryview(cp))).hexdigest() == SHA_DEFAULT_C_PARAMS


def test_5bit_catalogue_key_switch_keys():
    """the longer first-step key (B) and the n = 560 one-level bit tiers cannot share a key-switch key: Ba owns one, Ba2 shares it"""
    from dctfhe import params as P
    ps = P.default_params_5bit()
    by = {t.name: (i, t) for i, t in enumerate(ps.tiers)}
    assert by["B"][1].n > by["Ba"][1].n == by["Ba2"][1].n
    assert by["B"][1].ksk_share == -1 and by["Ba"][1].ksk_share == -1 and by["Ba2"][1].ksk_share == by["Ba"][0]
    assert by["T5r"][1].ksk_share == -1 and ps.table_tier_for_w[5] == by["T5r"][0]
    # the 4-bit tiers are the default catalogue's, at the same indices
    for i, t in enumerate(P.default_params().tiers):
        if t.name not in ("B", "Ba", "Ba2"):
            assert ps.tiers[i] == t


@pytest.fixture(scope="module")
def L():
    from dctfhe import _lib
    return _lib.load()


def test_params_check_four_levels(L):
    from dctfhe import params as P
    from dctfhe.engine import make_params
    assert L.dctfhe_params_check(C.byref(P.to_c_params(P.default_params_5bit()))) == 0, L.dctfhe_last_error().decode()

    def check(**over):
        t = dict(n=40, k=1, logN=11, l=4, beta=10, lk=4, betak=4, lwe_sigma=2.0 ** -30, glwe_sigma=2.0 ** -40)
        t.update(over)
        return L.dctfhe_params_check(C.byref(make_params(8192, 40, [t], 2.0 ** -50)))
    assert check() == 0, L.dctfhe_last_error().decode()
    for over in (dict(l=5, beta=8), dict(l=4, beta=11), dict(l=4, logN=10), dict(l=4, logN=12), dict(l=4, k=2, logN=10), dict(l=4, unroll=2)):
        assert check(**over) != 0, over
        assert "bad bootstrap gadget" in L.dctfhe_last_error().decode() or "unroll 2 needs" in L.dctfhe_last_error().decode()


def test_emulated_four_level_bootstrap(oracle):
    """pbs_thread<11, 1, 4, 8> (T5r) on the host: digit packing, decomposition, warm-up range and whole bootstraps against the oracle"""
    d = os.path.join(ROOT, "tests", "emul")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "emul_pbs_l4")
        oracle_dir = os.path.join(ROOT, "oracle")
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-pthread", "-o", exe, os.path.join(d, "emul_pbs_l4.cpp"), "-L" + oracle_dir,
                               "-ltfhe_ref", "-Wl,-rpath," + oracle_dir, "-lm"])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "EMUL OK" in out.stdout, out.stdout + out.stderr
    assert "N=2048 k=1 l=4 P=8 T=128 n=12: wrong=0" in out.stdout
