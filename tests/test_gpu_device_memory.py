"""Who holds device memory (include/dctfhe.h dctfhe_device_bytes_live): every allocation of the library belongs to one owner value, so
"a closed handle gave back everything" and "a call keeps nothing" are numbers.  Every assertion is on the counter relative to its value
at the start of the case (other modules' fixtures hold handles of their own); unlike a device-wide free-memory query it does not depend
on who else uses the card."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from test_gpu_primitives import D_SMALL, TIERS_SMALL

pytestmark = pytest.mark.gpu


def live():
    from dctfhe.engine import device_bytes_live
    return device_bytes_live()


def _compile(kind, ps):
    """the three circuits of tests/test_gpu_margin.py: exact 6-bit tables, 7-bit tables (parity-split sites with their parity buffer), and
    the pooled trunk (max-pool plan with its level buffers)"""
    from dctfhe import compile as cc, models
    if kind == "pool":
        calib = np.random.default_rng(3).normal(0, 1, (20, 4, 9, 9))
        return cc.compile_model(models.tiny_resnet_q(img_size=9, pool1=(3, 2, 1)), calib, rounding_threshold_bits=6, param_set=ps), calib
    calib = np.random.default_rng(0).normal(0, 1, (48, 4, 6, 6))
    return cc.compile_model(models.tiny_resnet_q(), calib, rounding_threshold_bits=7 if kind == "split" else 6, param_set=ps), calib


def _phases(compiled, x):
    from dctfhe import compile as cc
    q = cc.act_quant(np.asarray(x, np.float64), compiled.in_scale, True, compiled.in_bits)
    return (q.astype(np.int64).astype(np.uint64) << np.uint64(compiled.e_in)).reshape(-1)


def _small_params():
    from dctfhe.engine import make_params
    return make_params(D_SMALL, 40, TIERS_SMALL, 2.0 ** -50)


# ------------------------------------------------------------------------------------------ shared key-switch key
def test_shared_keyswitch_key_is_one_object(gpu_ctx):
    """tier 2 of the small set shares tier 0's key-switch key: one key, one column-sum cache, released once whichever half goes first"""
    from dctfhe.engine import Keys
    start = live()
    for client_first in (False, True):
        keys = Keys(gpu_ctx, _small_params(), seed=7)
        t0 = TIERS_SMALL[0]
        # at least the two key-switch keys that exist (tiers 0 and 1; u64 [D][lk][n + 1]) -- and the count is exact again after the close
        own = sum(D_SMALL * t["lk"] * (t["n"] + 1) * 8 for t in TIERS_SMALL if t.get("ksk_share", -1) < 0)
        assert live() - start > own
        if not client_first:
            held = live()
            cts = np.random.default_rng(1).integers(0, 2 ** 64, (3, D_SMALL + 1), dtype=np.uint64)
            cts[:, 512:D_SMALL] = 0
            via2 = keys.keyswitch(2, cts, deff=512)
            assert live() - held == (t0["n"] + 1) * 8           # the column sums over the first 512 key rows, made on first use ...
            via0 = keys.keyswitch(0, cts, deff=512)
            assert live() - held == (t0["n"] + 1) * 8           # ... and found by the owning tier: the cache is the key's, not the tier's
            assert np.array_equal(via0, via2) and np.array_equal(via0, keys.keyswitch(0, cts))
        first, second = (keys.client, keys.eval) if client_first else (keys.eval, keys.client)
        first.close()
        assert start < live()
        second.close()
        assert live() == start


# ------------------------------------------------------------------------------------------ session life cycle
@pytest.mark.parametrize("kind", ["exact", "split", "pool"])
def test_session_life_cycle(gpu_ctx, kind):
    from dctfhe import params as P
    from dctfhe.engine import Circuit, Keys, Session
    ps = P.test_params()
    compiled, calib = _compile(kind, ps)
    phases = _phases(compiled, calib[:1])
    start = live()
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=5)
    with_keys = live()
    circ = Circuit(gpu_ctx, compiled.blob)
    sess = Session(gpu_ctx, circ, keys, 1)
    clear = Session(gpu_ctx, circ, None, 1)

    def encrypted_round():
        sess.upload(keys.encrypt(phases))
        sess.set_audit(keys)
        sess.run()
        slots = sess.audit()
        assert slots and all(s["count"] > 0 for s in slots)
        return slots, sess.download_packed(0).rows

    slots1, rows1 = encrypted_round()
    clear.upload(phases)
    clear.run()
    after_first = live()
    slots2, rows2 = encrypted_round()                                   # a fresh audit (the old key copy and slots go), the same buffers
    assert live() == after_first, "a second run grew the session"
    assert [s["count"] for s in slots2] == [s["count"] for s in slots1] and rows2.shape == rows1.shape
    clear.run()
    assert live() == after_first
    sess.close()
    clear.close()
    circ.close()
    # what is left beyond the keys is their column-sum cache: a few arrays of n + 1 words of the tiers that own a key-switch key
    gained = live() - with_keys
    sizes = [(t.n + 1) * 8 for t in ps.tiers if t.ksk_share < 0]
    assert gained in {a * sizes[0] + b * sizes[1] for a in range(4) for b in range(4)}, (gained, sizes)
    keys.close()
    assert live() == start


# ------------------------------------------------------------------------------------------ primitives hold nothing
def test_primitives_hold_nothing(gpu_ctx):
    """every entry point that runs one kernel on host buffers, once so that lazy caches are filled, then once more: not a byte stays"""
    from dctfhe import params as P
    from dctfhe._lib import check
    from dctfhe.engine import Keys
    ps = P.test_params()
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=9)
    try:
        ctx, L, D = gpu_ctx, gpu_ctx.L, ps.D
        n0 = ps.tiers[0].n
        ph = np.arange(3, dtype=np.uint64) << np.uint64(59)
        cts = keys.encrypt(ph)
        narrow = cts.copy()
        narrow[:, 512:D] = 0
        small = np.zeros((3, n0 + 1), np.uint64)
        img = keys.encrypt(np.arange(4, dtype=np.uint64) << np.uint64(58)).reshape(1, 1, 2, 2, D + 1)
        relu = (np.maximum(np.arange(32) - 16, 0).astype(np.uint64) << np.uint64(58)).view(np.int64)
        ia, ib = np.array([0, 1, 2], np.int32), np.array([1, 2, 0], np.int32)
        plane = np.arange(64, dtype=np.uint8).reshape(1, 8, 8)
        allc, none = np.arange(16, dtype=np.int32), np.zeros(0, np.int32)
        rnd = np.zeros(3, np.uint64)
        blob = keys.export_eval_keys_compressed()
        calls = {
            "encrypt_rows": lambda: keys.encrypt(ph),
            "decrypt_rows": lambda: keys.decrypt(cts),
            "encrypt_seeded + expand_seeded": lambda: ctx.expand_seeded(keys.encrypt_seeded(ph)),
            "keyswitch_pack + decrypt_packed": lambda: keys.decrypt_packed(keys.keyswitch_pack(0, cts, D)),
            "keyswitch": lambda: keys.keyswitch(0, cts, shift=1),
            "keyswitch_prefix": lambda: keys.keyswitch(1, narrow, deff=512),
            "keyswitch_diff": lambda: keys.keyswitch_diff(0, cts, ia, ib, 0, 1 << 62),
            "modswitch_center": lambda: keys.modswitch_center(0, small),
            "pbs": lambda: keys.pbs(0, small, np.zeros((1, 16), np.int64), 4),
            "pbs_rows": lambda: keys.pbs_rows(0, small, np.zeros((2, 16), np.int64), 4, np.zeros((5, D + 4), np.uint64), row0=1, hw=2, nchan=2, accumulate=True),
            "keyswitch_sum": lambda: keys.keyswitch_sum(1, narrow, narrow[:, D - 512:], deff=512),
            "acc_rows": lambda: ctx.acc_rows(cts, narrow, 512),
            "gather_rows": lambda: ctx.gather_rows(narrow, 512, ia, D),
            "round_lut": lambda: keys.round_lut(1, 0, cts, 6, 2, np.zeros((1, 16), np.int64), 4),
            "round_lut_split": lambda: keys.round_lut_split(1, 0, 0, cts, 8, 1, np.zeros((1, 128), np.int64), 7),
            "conv2d": lambda: ctx.conv2d(D, img, 1, 1, 2, 2, np.ones((1, 1, 1, 1), np.int8), 1, 0),
            "add_rows": lambda: ctx.add_rows(cts, D, narrow, 512, D),
            "affine_rows": lambda: ctx.affine_rows(cts, D, cts, D, 1, 5),
            "sum_pool_rows": lambda: ctx.sum_pool_rows(img, D, 2, D),
            "max_pool_rows": lambda: ctx.max_pool_rows(img, D, 2, 2, 0, 5, relu, D, keys=keys, tier=0),
            "max_pool_rows, clear": lambda: ctx.max_pool_rows((np.arange(4, dtype=np.uint64) << np.uint64(58)).reshape(1, 1, 2, 2), 0, 2, 2, 0, 5),
            "rng_device": lambda: check(L.dctfhe_rng_device(ctx.h, bytes(32), 1, 0, 3, rnd.ctypes.data_as(C.c_void_p))),
            "margin_probe": lambda: keys.margin_probe(0, small, 3),
            "dct_frontend": lambda: ctx.dct_frontend(plane, plane, plane, 4, (allc, none, none), np.zeros(16), np.ones(16)),
            "export_secret": keys.export_secret,
            "export_ksk": lambda: keys.export_ksk(1),
            "export_bsk": lambda: keys.export_bsk(1),
            "eval_keys_export": keys.to_blob,
            "eval_keys_export_compressed": keys.export_eval_keys_compressed,
            "decompress_bsk": lambda: ctx.decompress_bsk(blob, 1),
            "fp64_peak": ctx.fp64_peak,
            "bench_pbs": lambda: keys.bench_pbs(0, 64, 1),
        }
        for f in calls.values():
            f()
        held = live()
        for name, f in calls.items():
            f()
            assert live() == held, name
    finally:
        keys.close()


# ------------------------------------------------------------------------------------------ refused calls hold nothing
def _fails(L, rc, needle):
    assert rc != 0
    msg = L.dctfhe_last_error().decode()
    assert needle in msg, msg


def test_refused_calls_hold_nothing(gpu_ctx):
    from dctfhe import _lib, params as P
    from dctfhe.engine import Circuit, ClientKey, EvalKeys, Keys, Session
    L = gpu_ctx.L
    ps = dataclasses.replace(P.test_params(), input_dim=512)
    compiled, calib = _compile("exact", ps)
    phases = _phases(compiled, calib[:1])
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=11)
    one_tier = P.to_c_params(ps)
    one_tier.n_tiers, one_tier.n_max = 1, one_tier.tiers[0].n
    k1 = Keys(gpu_ctx, one_tier, seed=3)
    other = P.test_params()
    other.tiers[1].n, other.tiers[0].n = 32, 56
    ck = ClientKey(gpu_ctx, P.to_c_params(other), seed=4)
    circ = Circuit(gpu_ctx, compiled.blob)
    sess = Session(gpu_ctx, circ, keys, 1)
    try:
        # an evaluation-key blob with one key-switch-key word off its torus grid: refused after every array has been allocated
        blob = keys.to_blob()
        off = blob.copy()
        off[16 + C.sizeof(_lib.Params)] ^= 1
        held = live()
        with pytest.raises(_lib.DctfheError, match="torus grid"):
            EvalKeys.from_blob(gpu_ctx, off)
        assert live() == held
        good = EvalKeys.from_blob(gpu_ctx, blob)
        assert live() > held
        good.close()
        assert live() == held
        # a full-width upload with a non-zero tail into a session compiled for a key prefix
        cts = keys.encrypt(phases)
        assert not cts[:, 512:ps.D].any()
        bad = cts.copy()
        bad[5, 700] = 1
        with pytest.raises(_lib.DctfheError, match="beyond 512"):
            sess.upload(bad)
        assert live() == held
        # a session against keys that lack a tier
        h = C.c_void_p()
        _fails(L, L.dctfhe_session_create(gpu_ctx.h, circ.h, k1.eval.h, 1, C.byref(h)), "names a tier the keys lack")
        assert live() == held
        # a client key of another parameter set, on a session whose audit is on: the audit stays on, its slots as they were
        sess.set_audit(keys)
        slots = sess.audit()
        assert slots
        held = live()
        _fails(L, L.dctfhe_session_set_audit(sess.h, ck.h), "another parameter set")
        assert live() == held and sess.audit() == slots
        # ... and the handles work afterwards
        sess.upload(cts)
        sess.run()
        ran = sess.audit()
        assert [(s["op"], s["entry"]) for s in ran] == [(s["op"], s["entry"]) for s in slots] and all(s["count"] > 0 for s in ran)
        sess.set_audit(None)
        assert sess.audit() == [] and live() < held
    finally:
        sess.close()
        circ.close()
        ck.close()
        k1.close()
        keys.close()
