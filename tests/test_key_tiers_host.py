"""Tier selections on the host (include/dctfhe.h TIER SELECTIONS; no GPU): which keys the catalogue circuits read,
the compiler's answer against the library's, the closing rule and its refusals, the blob sizes against the tier fields, the host library's
pruned export against slices of its full export, and bundles that record a selection."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import key_tiers_cases as KT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from dctfhe import _lib, _lib_client
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib_client.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def resnet20(bit_width, n_bits, rtb):
    from dctfhe import compile as cc, models
    from dctfhe.synthetic import synthetic_dct_batch
    return cc.compile_model(models.ResNet20QAT(bit_width, 24, 16), synthetic_dct_batch(24, seed=7), n_bits=n_bits, rounding_threshold_bits=rtb)


# bootstraps on / key-switch owners / never bootstraps on / MiB of compressed bootstrap-key bodies: all tiers, used tiers
CATALOGUE_CIRCUITS = [
    pytest.param((4, 5, 6), {"T6a", "T4r2", "T5a", "T4", "Ba2", "B"}, {"T6", "T4r", "T4", "B"}, {"T6", "T4r", "Ba"}, 795, 411, id="r20-4bit-rtb6"),
    pytest.param((5, 5, 6), {"T6a", "T4r2", "T5a", "T4", "T5r", "Ba2", "B"}, {"T6", "T4r", "T4", "B", "Ba", "T5r"}, {"T6", "T4r", "Ba"}, 903, 519,
                 id="r20-5bit-rtb6"),
    pytest.param((5, 5, 7), {"T6a", "T4r", "T5a", "T4", "T5r", "Ba2", "B", "T6"}, {"T6", "T4r", "T4", "B", "Ba", "T5r"}, {"T4r2", "Ba"}, 903, 783,
                 id="r20-5bit-rtb7"),
]


@pytest.mark.parametrize("model,bsk,ksk,never,mib_all,mib_used", CATALOGUE_CIRCUITS)
def test_key_tiers_of_the_catalogue_circuits(L, model, bsk, ksk, never, mib_all, mib_used):
    from dctfhe import engine, params as P
    c = resnet20(*model)
    ps, sel = c.param_set, c.key_tiers()
    names = {t.name for t in ps.tiers}
    assert sel.bsk == bsk and sel.ksk == ksk and names - sel.bsk == never
    if model[0] == 5:      # Ba never bootstraps, and its key-switch key stays: Ba2 shares it
        assert "Ba" not in sel.bsk and "Ba" in sel.ksk and ps.tiers[[t.name for t in ps.tiers].index("Ba2")].ksk_share == [t.name for t in ps.tiers].index("Ba")
    # T6 / T6a: the bootstrap key goes, the key-switch key stays
    if "T6" in never:
        assert "T6" in sel.ksk
    # ... a tier is selected exactly when the compiler counts a bootstrap on it
    assert sel.bsk == {n for n, v in c.pbs_counts().items() if v > 0}
    # the library's answer on the same blob
    cp = P.to_c_params(ps)
    k = engine.key_tiers_for_circuit(c.blob, cp)
    assert (k.bsk, k.ksk) == (sel.bsk_mask, sel.ksk_mask) == (KT.mask_of(ps, bsk), KT.mask_of(ps, ksk))
    assert engine.key_tiers_close(cp, k) == k, "the circuit's selection is closed"
    # the bootstrap-key bodies of the compressed blob, in MiB, as the catalogue's table states them
    body = [b for _, b in KT.sections(ps, True)]
    assert int(sum(body) / 2 ** 20) == mib_all
    assert int(sum(b for i, b in enumerate(body) if (sel.bsk_mask >> i) & 1) / 2 ** 20) == mib_used
    # the packed output forms pick a key-switch key the circuit already reads, or add exactly that one
    from dctfhe import compile as cc
    for form in ("rows", "ring"):
        so = c.key_tiers(form)
        assert so.bsk == sel.bsk and so.ksk == sel.ksk | {cc.output_compaction(c, form).name}
    rep = c.key_report()
    assert rep["selection"]["bsk"] == sorted(bsk) and [t["name"] for t in rep["tiers"] if not t["bsk"]] == [t.name for t in ps.tiers if t.name in never]
    for form, comp in (("full_bytes", False), ("compressed_bytes", True)):
        assert rep["all"][form] == engine.key_tiers_blob_bytes(cp, engine.key_tiers_all(cp), comp) == KT.blob_bytes(ps, *_all(ps), comp)
        assert rep["selected"][form] == engine.key_tiers_blob_bytes(cp, k, comp) == KT.blob_bytes(ps, k.bsk, k.ksk, comp)
        assert rep["selected"][form] < rep["all"][form]


def _all(ps):
    return (1 << len(ps.tiers)) - 1, sum(1 << i for i, t in enumerate(ps.tiers) if t.ksk_share < 0)


def test_tiny_circuit_on_catalogue_a_selects_t_b_and_q_b(L):
    from dctfhe import engine, params as P
    ps = KT.catalogue_a()
    c, _ = KT.tiny_circuit(ps)
    sel = c.key_tiers()
    assert sel.bsk == {"t", "b"} and sel.ksk == {"q", "b"} and (sel.bsk_mask, sel.ksk_mask) == (0b0110, 0b0101)
    k = engine.key_tiers_for_circuit(c.blob, P.to_c_params(ps))
    assert (k.bsk, k.ksk) == (0b0110, 0b0101)
    assert engine.key_tiers_all(P.to_c_params(ps)) == engine.KeyTiers(0b1111, 0b1101)
    assert not sel.is_all(ps) and P.KeyTierSelection.all(ps).covers(sel) and not sel.covers(P.KeyTierSelection.all(ps))
    # a circuit that names a tier the parameters lack is refused, not silently counted as nothing
    with pytest.raises(engine._lib.DctfheError, match="names a tier the keys lack"):
        engine.key_tiers_for_circuit(c.blob, _truncated(ps, 1))


def _truncated(ps, n_tiers):
    from dctfhe import params as P
    import copy
    q = copy.deepcopy(ps)
    q.tiers = q.tiers[:n_tiers]
    return P.to_c_params(q)


def test_closing_rule_and_its_refusals(L):
    from dctfhe import engine, params as P
    from dctfhe._lib import DctfheError, KeyTiers
    cp = P.to_c_params(KT.catalogue_a())
    # a selection that lists a sharing tier: its closure holds the owner's ksk bit
    assert engine.key_tiers_close(cp, (0b0010, 0)) == KeyTiers(0b0010, 0b0001)
    assert engine.key_tiers_close(cp, (0b1110, 0)) == KeyTiers(0b1110, 0b1101)
    assert engine.key_tiers_close(cp, (0, 0b0100)) == KeyTiers(0, 0b0100)          # a key-switch key alone is a closed selection
    assert engine.key_tiers_close(cp, (0, 0)) == KeyTiers(0, 0)
    assert engine.key_tiers_close(cp, engine.key_tiers_all(cp)) == engine.key_tiers_all(cp)
    for bad in ((0b10000, 0), (0, 0b10000), (1 << 31, 0)):
        with pytest.raises(DctfheError, match=r"at or beyond n_tiers = 4"):
            engine.key_tiers_close(cp, bad)
    with pytest.raises(DctfheError, match=r"key-switch key of tier 1, which has none of its own \(it shares tier 0's\)"):
        engine.key_tiers_close(cp, (0b0010, 0b0010))
    # the size formula takes closed selections only, and names what is missing
    with pytest.raises(DctfheError, match=r"not closed: tier 1 bootstraps, the key-switch key of tier 0 is not selected"):
        engine.key_tiers_blob_bytes(cp, (0b0010, 0), True)
    with pytest.raises(DctfheError, match=r"at or beyond n_tiers"):
        engine.key_tiers_blob_bytes(cp, (0b10000, 0b1), False)
    # a share chain ends at its last owner
    ps = KT.catalogue_a()
    ps.tiers[3].ksk_share = 2
    chain = P.to_c_params(ps)
    assert engine.key_tiers_close(chain, (0b1000, 0)) == KeyTiers(0b1000, 0b0100)
    assert P.ksk_owner(ps, 3) == 2 and P.ksk_owner(ps, 1) == 0 and P.ksk_owner(ps, 0) == 0


@pytest.mark.parametrize("catalogue", ["a", "b"])
def test_blob_bytes_follow_the_tier_fields(L, catalogue):
    from dctfhe import engine, params as P
    ps = KT.catalogue_a() if catalogue == "a" else KT.catalogue_b()
    cp = P.to_c_params(ps)
    nt = len(ps.tiers)
    seen = set()
    for bsk in range(1 << nt):
        k = engine.key_tiers_close(cp, (bsk, 0))
        for extra in (0, 1 << (nt - 1) if ps.tiers[nt - 1].ksk_share < 0 else 0):
            sel = (k.bsk, k.ksk | extra)
            if sel in seen:
                continue
            seen.add(sel)
            for comp in (False, True):
                assert engine.key_tiers_blob_bytes(cp, sel, comp) == KT.blob_bytes(ps, sel[0], sel[1], comp) == \
                    P.key_blob_bytes(ps, P.KeyTierSelection.from_masks(ps, *sel), comp), (sel, comp)
    assert len(seen) > 16


def test_host_export_full_is_todays_bytes_and_pruned_is_its_slices(L):
    from dctfhe import params as P
    from dctfhe.host_client import HostClientKey
    ps = KT.catalogue_a()
    c, _ = KT.tiny_circuit(ps)
    sel = c.key_tiers()
    ck = HostClientKey(P.to_c_params(ps), seed=5)
    try:
        full = ck.export_eval_keys_compressed()
        assert full.size == KT.blob_bytes(ps, *_all(ps), True)
        assert np.array_equal(ck.export_eval_keys_compressed(_all(ps)), full), "everything selected is not the unpruned export byte for byte"
        assert np.array_equal(ck.export_eval_keys_compressed((0b1111, 0)), full), "the closure of every bootstrap key is everything"
        pruned = ck.export_eval_keys_compressed(sel)
        assert pruned.size == KT.blob_bytes(ps, sel.bsk_mask, sel.ksk_mask, True) < full.size
        assert np.array_equal(pruned, KT.pruned_from_full(full, ps, sel.bsk_mask, sel.ksk_mask, True))
        # the library closes what it is given: t alone brings q's key-switch key
        assert np.array_equal(ck.export_eval_keys_compressed((0b0010, 0)), KT.pruned_from_full(full, ps, 0b0010, 0b0001, True))
        # the last tier alone: a dropped front
        assert np.array_equal(ck.export_eval_keys_compressed((0b1000, 0)), KT.pruned_from_full(full, ps, 0b1000, 0b1000, True))
        from dctfhe.engine import blob_key_tiers
        assert blob_key_tiers(full) == _all(ps) and blob_key_tiers(pruned) == (sel.bsk_mask, sel.ksk_mask)
        for bad, needle in (((0b10000, 0), "at or beyond n_tiers = 4"), ((0, 0b0010), "has none of its own")):
            with pytest.raises(RuntimeError, match=needle):
                ck.export_eval_keys_compressed(bad)
        # size query and a too-small buffer under a selection
        from dctfhe._lib_client import KeyTiers
        n, kt = C.c_size_t(), KeyTiers(sel.bsk_mask, sel.ksk_mask)
        assert ck.L.dctfhe_host_eval_keys_export_compressed_tiers(ck.h, C.byref(kt), None, 0, C.byref(n)) == 0 and n.value == pruned.size
        small = np.zeros(64, np.uint8)
        assert ck.L.dctfhe_host_eval_keys_export_compressed_tiers(ck.h, C.byref(kt), small.ctypes.data_as(C.c_void_p), 64, C.byref(n)) != 0 and not small.any()
    finally:
        ck.close()


def test_host_export_on_the_two_bit_catalogue(L):
    """catalogue B: the pair-secret tiers, kept and dropped"""
    from dctfhe import params as P
    from dctfhe.host_client import HostClientKey
    ps = KT.catalogue_b()
    ck = HostClientKey(P.to_c_params(ps), seed=6)
    try:
        full = ck.export_eval_keys_compressed()
        for bsk, ksk in ((0b1001, 0b1001), (0b0110, 0b0001)):
            got = ck.export_eval_keys_compressed((bsk, 0))
            assert np.array_equal(got, KT.pruned_from_full(full, ps, bsk, ksk, True)), (bsk, ksk)
    finally:
        ck.close()


# ------------------------------------------------------------------------------------------ configuration and bundles
def _module(ps, **cfg):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import Configuration, compile_brevitas_qat_model
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    return compile_brevitas_qat_model(models.tiny_resnet_q(), calib, n_bits=5, rounding_threshold_bits=6, param_set=ps,
                                      configuration=Configuration(public_input_spec=P.test_public_input_spec(), result_packing_spec=P.test_pack_spec(), **cfg))


def test_configuration_selects_all_or_the_circuits_tiers(L):
    from dctfhe.quantized_module import Configuration
    assert Configuration().evaluation_key_tiers == "all"
    with pytest.raises(ValueError, match="evaluation_key_tiers"):
        Configuration(evaluation_key_tiers="some")
    ps = KT.catalogue_a()
    assert _module(ps).key_tiers() is None
    qm = _module(ps, evaluation_key_tiers="circuit")
    assert qm.key_tiers() == qm.compiled.key_tiers()
    for form in ("rows", "ring"):
        qm = _module(ps, evaluation_key_tiers="circuit", compress_output_ciphertexts=form)
        assert qm.key_tiers() == qm.compiled.key_tiers(form, qm.configuration.result_packing_spec)
        assert qm.output_compaction(form).name in qm.key_tiers().ksk


def test_bundles_record_a_pruned_selection_and_default_files_do_not_change(L, tmp_path):
    from dctfhe import deploy, params as P
    ps = KT.catalogue_a()
    qm = _module(ps)
    d0, d1, d2 = (str(tmp_path / n) for n in ("default", "all", "circuit"))
    deploy.save(qm, d0)
    deploy.save(qm, d1, key_tiers="all")
    deploy.save(qm, d2, key_tiers="circuit")
    for name in (deploy.CLIENT_FILE, deploy.SERVER_FILE):
        raw = [open(os.path.join(d, name), "rb").read() for d in (d0, d1, d2)]
        assert raw[0] == raw[1], "save(key_tiers='all') is not the default save byte for byte"
        assert raw[2] != raw[0]
    with pytest.raises(ValueError, match="key_tiers"):
        deploy.save(qm, d2, key_tiers="used")
    sel = qm.compiled.key_tiers()
    for load, name, kind in ((deploy.load_client_spec, deploy.CLIENT_FILE, "client"), (deploy.load_server_bundle, deploy.SERVER_FILE, "server")):
        full, pruned = load(os.path.join(d0, name)), load(os.path.join(d2, name))
        assert not full.pruned and full.key_tiers == P.KeyTierSelection.all(ps), "a file without the field loads as every tier"
        assert pruned.pruned and pruned.key_tiers == sel
        assert "key_tiers" not in deploy.read_container(os.path.join(d0, name), kind)
        assert deploy.read_container(os.path.join(d2, name), kind)["key_tiers"] == dict(bsk=sel.bsk_mask, ksk=sel.ksk_mask)
        assert pruned.digest == full.digest, "the selection is not part of the circuit digest"
    # the catalogue whose every tier the circuit reads: "circuit" has nothing to record and writes the default files
    qt = _module(P.test_params())
    e0, e1 = str(tmp_path / "t_default"), str(tmp_path / "t_circuit")
    deploy.save(qt, e0)
    deploy.save(qt, e1, key_tiers="circuit")
    for name in (deploy.CLIENT_FILE, deploy.SERVER_FILE):
        assert open(os.path.join(e0, name), "rb").read() == open(os.path.join(e1, name), "rb").read()


def test_host_client_follows_the_bundles_selection(L, tmp_path):
    from dctfhe import deploy
    ps = KT.catalogue_a()
    qm = _module(ps)
    deploy.save(qm, str(tmp_path / "all"))
    deploy.save(qm, str(tmp_path / "circuit"), key_tiers="circuit")
    sel = qm.compiled.key_tiers()
    a, c = deploy.Client(str(tmp_path / "all" / deploy.CLIENT_FILE), device="host"), deploy.Client(str(tmp_path / "circuit" / deploy.CLIENT_FILE), device="host")
    try:
        a.keygen(seed=8)
        c.keygen(seed=8)
        full, pruned = a.export_evaluation_keys(), c.export_evaluation_keys()
        assert np.array_equal(pruned, KT.pruned_from_full(full, ps, sel.bsk_mask, sel.ksk_mask, True))
        # the key check covers the tiers whose bootstrap key is present, and only those
        assert [t for t, _ in a._key_check_tiers()] == [0, 1, 2, 3] and [t for t, _ in c._key_check_tiers()] == [1, 2]
        assert len(c.make_key_check()) < len(a.make_key_check())
    finally:
        a.close()
        c.close()
