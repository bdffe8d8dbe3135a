"""Margin audit: what the entry points refuse, each with its message (include/dctfhe.h); the handles work afterwards."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kit(gpu_ctx):
    from dctfhe import compile as cc, models, params as P
    from dctfhe.engine import Circuit, Keys
    ps = P.test_params()
    keys = Keys(gpu_ctx, P.to_c_params(ps), seed=2)
    calib = np.random.default_rng(0).normal(0, 1, (16, 4, 6, 6))
    exact = cc.compile_model(models.tiny_resnet_q(), calib, param_set=ps)
    approx = cc.compile_model(models.tiny_resnet_q(), calib, param_set=ps, rounding_method="approximate")
    c_exact, c_approx = Circuit(gpu_ctx, exact.blob), Circuit(gpu_ctx, approx.blob)
    yield gpu_ctx, keys, c_exact, c_approx, exact, ps
    c_exact.close()
    c_approx.close()
    keys.close()


def _fails(L, rc, needle):
    assert rc != 0
    msg = L.dctfhe_last_error().decode()
    assert needle in msg, msg


def test_probe_refusals(kit):
    from dctfhe._lib import MarginStats, ptr
    ctx, keys, _, _, _, ps = kit
    L = ctx.L
    small = np.zeros((3, ps.tiers[0].n + 1), np.uint64)
    err, st = np.zeros(3, np.int32), MarginStats()
    _fails(L, L.dctfhe_margin_probe(None, keys.client.h, 0, ptr(small), 3, 3, ptr(err), C.byref(st)), "null")
    _fails(L, L.dctfhe_margin_probe(ctx.h, None, 0, ptr(small), 3, 3, ptr(err), C.byref(st)), "null")
    _fails(L, L.dctfhe_margin_probe(ctx.h, keys.client.h, 0, None, 3, 3, ptr(err), C.byref(st)), "null")
    _fails(L, L.dctfhe_margin_probe(ctx.h, keys.client.h, 2, ptr(small), 3, 3, ptr(err), C.byref(st)), "tier 2 out of range")
    _fails(L, L.dctfhe_margin_probe(ctx.h, keys.client.h, -1, ptr(small), 3, 3, ptr(err), C.byref(st)), "out of range")
    _fails(L, L.dctfhe_margin_probe(ctx.h, keys.client.h, 0, ptr(small), 3, ps.tiers[0].logN, ptr(err), C.byref(st)), "leaves no box")
    _fails(L, L.dctfhe_margin_probe(ctx.h, keys.client.h, 1, ptr(small), 3, ps.tiers[1].logN + 1, ptr(err), C.byref(st)), "leaves no box")
    _fails(L, L.dctfhe_margin_probe(ctx.h, keys.client.h, 0, ptr(small), 3, -1, ptr(err), C.byref(st)), "leaves no box")
    # the handles still work: trivial zero rows sit on a box centre
    e, s = keys.margin_probe(0, small, 3)
    assert not e.any() and s["count"] == 3 and s["max_abs"] == 0 and s["hist"][0] == 3


def test_session_refusals(kit):
    from dctfhe import params as P
    from dctfhe._lib import MarginStats
    from dctfhe.engine import ClientKey, Session, make_params
    ctx, keys, c_exact, c_approx, compiled, ps = kit
    L = ctx.L
    n = C.c_int()
    _fails(L, L.dctfhe_session_set_audit(None, keys.client.h), "null session")
    _fails(L, L.dctfhe_session_audit(None, None, 0, C.byref(n)), "null")
    clear = Session(ctx, c_exact, None, 1)
    try:
        _fails(L, L.dctfhe_session_set_audit(clear.h, keys.client.h), "clear-mode")
    finally:
        clear.close()
    sess = Session(ctx, c_exact, keys, 1)
    try:
        _fails(L, L.dctfhe_session_audit(sess.h, None, 0, None), "null")
        # clients of other parameter sets: another small key; the same lengths with another ring on one tier
        other = P.test_params()
        other.tiers[1].n = 32
        other.tiers[0].n = 56
        shape = P.test_params()
        shape.tiers[0].logN = 9
        for bad, needle in ((other, "another parameter set"), (shape, "tier 0 of the client key")):
            ck = ClientKey(ctx, P.to_c_params(bad), seed=4)
            try:
                _fails(L, L.dctfhe_session_set_audit(sess.h, ck.h), needle)
            finally:
                ck.close()
        assert sess.audit() == []                                   # a refused call leaves the audit off
        sess.set_audit(keys)
        assert L.dctfhe_session_audit(sess.h, None, 0, C.byref(n)) == 0 and n.value == len(compiled.margin_model())
        few = (MarginStats * 2)()
        _fails(L, L.dctfhe_session_audit(sess.h, few, 2, C.byref(n)), "room for 2 slots")
        assert n.value == len(compiled.margin_model())
        # on, not yet run: the slots with their fixed fields and no decisions
        slots = sess.audit()
        assert [s["count"] for s in slots] == [0] * n.value and [s["op"] for s in slots] == [m["op"] for m in compiled.margin_model()]
        sess.set_audit(None)
        assert sess.audit() == []
    finally:
        sess.close()
    rough = Session(ctx, c_approx, keys, 1)
    try:
        _fails(L, L.dctfhe_session_set_audit(rough.h, keys.client.h), "rounds approximately")
    finally:
        rough.close()


def test_module_without_client_key(kit):
    from dctfhe.quantized_module import QuantizedModule
    ctx, keys, _, _, compiled, _ = kit
    qm = QuantizedModule(compiled)
    try:
        qm.load_evaluation_keys(keys.to_blob())
        with pytest.raises(RuntimeError, match="needs the client key"):
            qm.audit_quantized(np.zeros((1, 4, 6, 6), np.int64))
    finally:
        qm.close()
