"""compile_model(pool_policy="exact") on the host (no GPU): the stem max pool of the 5-bit RGB trunks moves to the quiet pool tier T6p of
params.default_params_5bit_pool and the circuit meets the exact-evaluation budget; the default policy, and every circuit that needs no
move, compile to what they compiled to before; the catalogue, the blob, the bundles and the command line carry the tier."""
import ctypes as C
import hashlib
import importlib.util
import os
import sys
import warnings

import numpy as np
import pytest

import pool_policy_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_BLOBS = {    # compile_model(ResNet18QAT(5, 3, img), default_rng(0).normal(0, 1, (2, 3, img, img)), rtb) on the parent commit: (img, rtb)
    (128, 6): "d1ece4d52519ddb08604b21aed033c732ba11c2d61c6ecbf2c8a6b023c0d7767",
    (128, 7): "89195119cd0a257dfd572644ebddc4668d682428cb45fdfb8ab4c579cdccb15e",
    (224, 6): "e85e69df4007965266b0bf849a92a6fc9abc28e027b07a079c33edca2a3605d4",
    (224, 7): "82c96f61aab6aed649d6e4235409e9aaa43d7d98a8ef9cc1ae7099075d24f33d",
}
N_MAX = {128: 387072, 224: 1193472}


def _compile(img, rtb, **kw):
    from dctfhe import compile as cc, models
    calib = np.random.default_rng(0).normal(0, 1, (2, 3, img, img))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c = cc.compile_model(models.ResNet18QAT(bit_width=5, in_channels=3, img_size=img), calib, rounding_threshold_bits=rtb, **kw)
    return c, [x for x in w if "budget" in str(x.message)]


@pytest.mark.parametrize("rtb", [6, 7])
@pytest.mark.parametrize("img", [128, 224])
def test_resnet18_rgb_5bit_pool_moves_to_the_quiet_tier(img, rtb):
    c, warned = _compile(img, rtb, pool_policy="exact")
    _, pool = cases.pool_op(c)
    ps = c.param_set
    assert not warned
    assert ps.tiers[pool.pool.tier].name == "T6p" and pool.pool.tier == 10 and len(ps.tiers) == 11 and ps.pool_tier_fallback_for_w == {6: 10}
    print(f"{img} rtb {rtb}: pool {pool.pfail:.2e}, worst site {c.worst_site_failure:.2e}, expected failures / image {c.expected_failures_per_image:.2e}")
    assert pool.pfail <= 1e-12 and c.worst_site_failure <= 1e-12
    assert c.expected_failures_per_image < 1e-5
    assert c.pbs_counts()["T6p"] == pool.n_max == N_MAX[img]
    assert c.tensors[pool.dst].deff == 8192
    assert pool.pool.p_d == 6 and pool.ip[4] == 10
    # what follows PoolSite.tier: the report, the audit's model, the noise `simulate` injects
    assert "tier=T6p" in c.report() and "// tier 10 T6p: n=832 k=1 N=8192 l=2 beta=15" in c.report()
    (row,) = [m for m in c.margin_model() if m["kind"] == "pool"]
    assert row["tier_name"] == "T6p" and row["table_bits"] == 6 and row["elements"] == pool.n_max
    assert c.simulation_sigmas()[cases.pool_op(c)[0]] == pool.sim_sigma <= row["sigma"]
    # the default policy: the parent's blob, the pool where it was
    d, warned = _compile(img, rtb)
    _, dpool = cases.pool_op(d)
    assert hashlib.sha256(d.blob).hexdigest() == PARENT_BLOBS[img, rtb]
    assert warned and d.param_set.tiers[dpool.pool.tier].name == "T6a" and len(d.param_set.tiers) == 10
    assert abs(dpool.pfail - 5.68e-5) < 0.01e-5 and d.pool_policy == "coarse" and c.pool_policy == "exact"
    assert hashlib.sha256(_compile(img, rtb, pool_policy="coarse")[0].blob).hexdigest() == PARENT_BLOBS[img, rtb]


def _same(make):
    from dctfhe import params as P
    a, b = make(), make(pool_policy="exact")
    assert a.blob == b.blob
    assert bytes(P.to_c_params(a.param_set)) == bytes(P.to_c_params(b.param_set))
    assert [t.name for t in a.param_set.tiers] == [t.name for t in b.param_set.tiers]
    assert not any(o.pool.quiet for o in b.ops if o.pool is not None)
    return a


def test_circuits_that_need_no_move_compile_as_before():
    from dctfhe import compile as cc, models, params as P

    def quiet(fn):
        def run(**kw):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return fn(**kw)
        return run
    c = _same(quiet(lambda **kw: cc.compile_model(models.ResNet18QAT(bit_width=4, in_channels=3, img_size=224),
                                                  np.random.default_rng(0).normal(0, 1, (2, 3, 224, 224)), **kw)))
    assert c.param_set.tiers[cases.pool_op(c)[1].pool.tier].name == "T5a" and len(c.param_set.tiers) == 9
    c = _same(quiet(lambda **kw: cc.compile_model(models.ResNet20QAT(5, 24, 16), np.random.default_rng(7).normal(0, 1, (4, 24, 16, 16)), **kw)))
    assert len(c.param_set.tiers) == 10 and not any(o.type == cc.OP_MAXPOOL for o in c.ops)
    c = _same(quiet(lambda **kw: cc.compile_model(models.tiny_resnet_q(img_size=9, pool1=(3, 2, 1)), np.random.default_rng(1).normal(0, 1, (24, 4, 9, 9)),
                                                  n_bits=5, param_set=P.test_params(), **kw)))
    assert len(c.param_set.tiers) == 2


def test_catalogue_constructors():
    from dctfhe import params as P
    import dataclasses
    same = lambda a, b: dataclasses.asdict(a) == dataclasses.asdict(b)
    pool, five = P.default_params_5bit_pool(), P.default_params_5bit()
    assert [dataclasses.asdict(t) for t in pool.tiers[:10]] == [dataclasses.asdict(t) for t in five.tiers] and len(pool.tiers) == 11
    t = pool.tiers[10]
    assert (t.name, t.k, t.logN, t.l, t.beta, t.lk, t.betak, t.ksk_share, t.unroll) == ("T6p", 1, 13, 2, 15, 9, 2, -1, 1) and t.n % 8 == 0
    assert t.lwe_sigma == P.sigma_min(t.n) and t.glwe_sigma == P.sigma_min(8192)
    assert pool.pool_tier_fallback_for_w == {6: 10} and five.pool_tier_fallback_for_w is None and P.default_params().pool_tier_fallback_for_w is None
    assert same(P.params_for_bit_width(5), five) and same(P.params_for_bit_width(4), P.default_params())
    assert same(P.params_for_bit_width(5, pool_policy="exact"), pool) and same(P.params_for_bit_width(4, pool_policy="exact"), P.default_params())
    assert dataclasses.replace(pool, tiers=pool.tiers[:10], pool_tier_fallback_for_w=None) == five


@pytest.fixture(scope="module")
def crop():
    qm, x = cases.crop_module()
    yield qm, x
    qm.close()


def test_library_accepts_catalogue_and_blob_and_the_pool_is_the_integer_pool(crop):
    from dctfhe import _lib, compile as cc, params as P
    from oracle import circuit_ref as mref
    L = _lib.load()
    assert L.dctfhe_params_check(C.byref(P.to_c_params(P.default_params_5bit_pool()))) == 0, L.dctfhe_last_error().decode()
    qm, x = crop
    c = qm.compiled
    assert L.dctfhe_circuit_validate(c.blob, len(c.blob)) == 0, L.dctfhe_last_error().decode()
    i, o = cases.pool_op(c)
    assert c.param_set.tiers[o.pool.tier].name == "T6p" and cases.blob_pool_tier(c.blob, len(c.tensors), i) == 10
    counts = c.pbs_counts()
    assert counts["T6p"] == o.n_max == cases.CROP_POOL_PAIRS
    assert c.worst_site_failure <= 1e-12
    q = qm.quantize_input(x[12:14])
    vals, overflow = mref.run_clear(c.blob, qm.encode_input(q), all_tensors=True)
    assert not overflow
    e = c.tensors[o.src0].e
    assert c.tensors[o.dst].e == e
    src, dst = vals[o.src0].view(np.int64) >> np.int64(e), vals[o.dst].view(np.int64) >> np.int64(e)
    assert src.min() >= 0 and src.max() <= 31 and len(np.unique(src)) > 8
    assert np.array_equal(dst, cc.max_pool_int(src, 3, 2, 1))
    assert o.payload.size == 64
    assert np.array_equal(o.payload.ravel().view(np.uint64), np.maximum(np.arange(64) - 32, 0).astype(np.uint64) << np.uint64(e))


def test_cli_flags(monkeypatch):
    spec = importlib.util.spec_from_file_location("he_cli_pool", os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py"])
    assert mod.parse_args().pool_policy == "coarse"
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--pool_policy", "exact", "--bit_width", "5"])
    assert mod.parse_args().pool_policy == "exact"
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--pool_policy", "quiet"])
    with pytest.raises(SystemExit):
        mod.parse_args()
    from dctfhe import deploy
    monkeypatch.setattr(sys, "argv", ["deploy", "save", "--out", "x", "--pool_policy", "exact"])
    seen = {}
    monkeypatch.setattr(deploy, "_cmd_save", lambda a: seen.update(vars(a)))
    deploy.main()
    assert seen["pool_policy"] == "exact"


def test_bundles_keep_the_tier(crop, tmp_path):
    from dctfhe import deploy
    qm, _ = crop
    c = qm.compiled
    i, o = cases.pool_op(c)
    client_path, server_path = deploy.save(qm, str(tmp_path / "exact"))
    client, server = deploy.load_client_spec(client_path), deploy.load_server_bundle(server_path)
    for spec in (client, server):
        ps = spec.param_set
        assert len(ps.tiers) == 11 and ps.tiers[10] == c.param_set.tiers[10] and ps.pool_tier_fallback_for_w == {6: 10}
        assert ps == c.param_set
    assert server.blob == c.blob and cases.blob_pool_tier(server.blob, len(c.tensors), i) == 10
    assert deploy.key_check_bits(client.param_set)[10] == 6 and len(deploy.key_check_bits(client.param_set)) == 11
    # a circuit of the default policy: the bundle's parameter tree is the one bundles carried before there was a pool tier
    coarse, _ = cases.crop_module("coarse")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            client_path, _ = deploy.save(coarse, str(tmp_path / "coarse"))
        tree = deploy.read_container(client_path, "client")
        assert "pool_tier_fallback_for_w" not in tree["param_set"] and len(tree["param_set"]["tiers"]) == 10
        old = deploy.load_client_spec(client_path).param_set
        assert old == coarse.compiled.param_set and old.pool_tier_fallback_for_w is None
    finally:
        coarse.close()


def test_exact_pool_policy_refuses_the_p_error_catalogue():
    from dctfhe import compile as cc, models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (4, 4, 6, 6))
    with pytest.raises(ValueError, match="pool_policy 'exact' needs tier_policy='exact'"):
        cc.compile_model(models.tiny_resnet_q(), calib, p_error=0.01, tier_policy="p_error", pool_policy="exact")
    with pytest.raises(ValueError, match="pool_policy 'exact' needs tier_policy='exact'"):
        compile_brevitas_qat_model(models.tiny_resnet_q(), calib, p_error=0.01, tier_policy="p_error", pool_policy="exact")
    with pytest.raises(ValueError, match="pool_policy 'quiet'"):
        cc.compile_model(models.tiny_resnet_q(), calib, pool_policy="quiet")
