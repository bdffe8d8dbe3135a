"""The duo form of the general two-bit bootstrap (pbs_kernel_duo<11, 1, 3, 4, 2>: two ciphertexts per group of 256 threads, two groups
per workgroup; csrc/pbs_core.h pbs_thread_duo), on the shape and the short key of tests/test_gpu_pbs_matrix.py (N = 2048, k = 1, l = 3,
n = 40, beta 12, unroll 2).  Launches of 1, 2, 3, 4, 5 and 9 ciphertexts -- a lone ciphertext, a full duo, an odd tail, a full workgroup,
a workgroup plus one, two workgroups plus a tail -- in both write-back modes: every output decodes to f(m), and the rms of
device - exact-arithmetic oracle (oracle pbs_mb2 = ref_pbs_mb2_batch) stays within the bound of test_gpu_pbs_matrix.py,
sqrt(2) 1.6 sqrt(n (fft + dec)) (pbs_matrix_ref.diff_bound).  Then the two slots of a duo: one ciphertext in slot 0 and in slot 1 of one
launch gives the same words, and its words do not depend on its partner.  Nothing is taken from the kernel under test."""
import math

import numpy as np
import pytest

import pbs_matrix_ref as R

LOGN, K, L, UNROLL, BETA, N_SMALL, W = 11, 1, 3, 2, 12, 40, 5
N = D = 1 << LOGN
COUNTS = (1, 2, 3, 4, 5, 9)
BODY_ADD = 0x9E3779B97F4A7C15


def _tier():
    return dict(n=N_SMALL, k=K, logN=LOGN, l=L, beta=BETA, lk=4, betak=4, lwe_sigma=2.0 ** -24, glwe_sigma=2.0 ** -52, unroll=UNROLL)


def _dec(ph):
    """4-bit signed entries at 2^57: the entry and its negation, mod 128"""
    return ((ph + (np.uint64(1) << np.uint64(56))) >> np.uint64(57)) & np.uint64(127)


@pytest.fixture(scope="module")
def rig(gpu_ctx, oracle):
    """keys, 9 noisy inputs with a table each out of three, and the exact oracle's bootstrap of them: computed once, never written to"""
    from dctfhe.engine import Keys, make_params
    keys = Keys(gpu_ctx, make_params(D, N_SMALL, [_tier()], 2.0 ** -50), seed=77)
    try:
        S, s = keys.export_secret()
        s = s[:N_SMALL].copy()
        rng = np.random.default_rng(2048134)
        m = max(COUNTS)
        msgs = (np.arange(m, dtype=np.uint64) * np.uint64(7) + np.uint64(3)) % np.uint64(2 << W)
        idx = (np.arange(m) % 3).astype(np.int32)
        tables = rng.integers(-8, 8, (3, 1 << W)).astype(np.int64) << 57
        small = oracle.lwe_encrypt(s, N_SMALL, msgs << np.uint64(63 - W), 2.0 ** -30, seed=91)
        ref = oracle.pbs_mb2(small, keys.export_bsk(0), K, N, L, BETA, tables, W, idx, D)
        want = R.message_expected(tables, idx, W, msgs)
        ph_ref = oracle.lwe_phase(S, D, ref)
        assert np.array_equal(_dec(ph_ref), _dec(want)), "the oracle itself decodes wrong"
        for a in (small, idx, tables, want, ph_ref):
            a.setflags(write=False)
        model = R.tier_spec(N_SMALL, K, LOGN, L, BETA, UNROLL, _tier()["glwe_sigma"])
        yield dict(keys=keys, S=S, small=small, idx=idx, tables=tables, want=want, ph_ref=ph_ref, bound=R.diff_bound(model), rng=rng)
    finally:
        keys.close()


def _check(rig, oracle, ph, c, what):
    assert np.array_equal(_dec(ph), _dec(rig["want"][:c])), (what, "decodes wrong", np.flatnonzero(_dec(ph) != _dec(rig["want"][:c])))
    rms = math.sqrt(float(np.mean(np.square(R.cent(ph - rig["ph_ref"][:c])))))
    print("%s: rms(device - exact oracle) = %.3f of the bound" % (what, rms / rig["bound"]))
    assert rms < rig["bound"], (what, rms, rig["bound"])


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_store_mode(rig, oracle, count):
    keys, sm, ix = rig["keys"], rig["small"][:count], rig["idx"][:count]
    out = keys.pbs(0, sm, rig["tables"], W, ix)
    assert out.shape == (count, D + 1)
    _check(rig, oracle, oracle.lwe_phase(rig["S"], D, out), count, "store, %d" % count)
    # through the row interface over garbage, a guard row either side
    pre = rig["rng"].integers(0, 2 ** 64, (count + 2, D + 1), dtype=np.uint64)
    got = keys.pbs_rows(0, sm, rig["tables"], W, pre, row0=1, table_idx=ix, body_add=BODY_ADD)
    assert np.array_equal(got[0], pre[0]) and np.array_equal(got[-1], pre[-1]), "a row outside the launch was written"
    assert np.array_equal(got[1:-1, :D], out[:, :D]) and np.array_equal(got[1:-1, D], out[:, D] + np.uint64(BODY_ADD))


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_accumulate_mode_with_body_add(rig, oracle, count):
    keys, sm, ix = rig["keys"], rig["small"][:count], rig["idx"][:count]
    pre = rig["rng"].integers(0, 2 ** 64, (count + 2, D + 1), dtype=np.uint64)
    got = keys.pbs_rows(0, sm, rig["tables"], W, pre, row0=1, table_idx=ix, accumulate=True, body_add=BODY_ADD)
    assert np.array_equal(got[0], pre[0]) and np.array_equal(got[-1], pre[-1]), "a row outside the launch was written (the padded slots accumulate nowhere)"
    added = got[1:-1] - pre[1:-1]
    added[:, D] -= np.uint64(BODY_ADD)
    _check(rig, oracle, oracle.lwe_phase(rig["S"], D, added), count, "accumulate, %d" % count)


@pytest.mark.gpu
def test_slots_of_a_duo_are_independent(rig):
    keys, sm, ix, tb = rig["keys"], rig["small"], rig["idx"], rig["tables"]
    launch = lambda order: keys.pbs(0, sm[order], tb, W, ix[order])
    # the same ciphertext in slot 0 and slot 1 of one duo, and in both duos of a workgroup
    for order in ([0, 0], [3, 3, 3, 3], [1, 2, 2, 1, 2]):
        out = launch(order)
        for a in range(len(order)):
            for b in range(a + 1, len(order)):
                if order[a] == order[b]:
                    assert np.array_equal(out[a], out[b]), (order, a, b, "the same ciphertext in two slots of one launch gives other words")
    # one ciphertext next to two different partners, in either slot, and alone (its partner then is itself, into the sink)
    alone = launch([0])[0]
    for order, at in (([0, 1], 0), ([0, 5], 0), ([1, 0], 1), ([5, 0], 1), ([4, 7, 8, 0, 2], 3), ([4, 7, 0, 8, 2], 2)):
        assert np.array_equal(launch(order)[at], alone), (order, "a ciphertext's output depends on its partner or its slot")
