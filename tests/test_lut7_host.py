"""Exact 7-bit tables (CPU side): rounding_threshold_bits=7 compiles on both exact catalogues as parity-split sites (DESIGN.md section 9:
one more one-bit step, the parity into the padding bit, two 6-bit look-ups  S[t'] + (-1)^b0 Dt[t'] = T[2 t' + b0]), every site inside
the 1e-12 budget; the blob keeps ONE record per site with the whole 128-entry tables, so the frozen numpy interpreter evaluates it
unchanged; circuits compiled with rounding_threshold_bits <= 6 stay byte for byte what they were."""
import ctypes as C
import hashlib
import importlib.util
import os
import struct
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rounding_threshold_bits=6 blobs of r20_24_16 recorded from the commit before the parity split (bench.py's calibration batch of 100,
# seed-0 model): the 4-bit value is the one tests/test_bitwidth5_host.py holds
SHA_RTB6 = {
    4: "230c71dca425913a0001fdb4804f71a8cb4db53ee5b81edcdf44853df8de33f9",
    5: "cbea42efff0b12d8308c22d49997f8688047322af07949cbdfbac3e283e78937",
}


def _compile(name, bit_width, rtb=7, n_calib=100, **kw):
    import bench
    from dctfhe import compile as cc, models
    factory, in_ch, img, make_batch, _ = bench.CONFIGS[name]
    calib = make_batch(n_calib, 7)
    model = getattr(models, factory)(bit_width=bit_width, in_channels=in_ch, img_size=img, seed=0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c = cc.compile_model(model, calib, rounding_threshold_bits=rtb, n_bits=5, **kw)
    return c, calib, [str(x.message) for x in w if "dctfhe" in str(x.message)]


def test_resnet20_5bit_compiles_at_seven_bits():
    """the reference's ImageNet setting (bit_width 5, rounding_threshold_bits 7) used to end in `no tier for a table of 7 input bits`"""
    from dctfhe import compile as cc, models
    from dctfhe.synthetic import synthetic_dct_batch
    c = cc.compile_model(models.ResNet20QAT(5, 24, 16), synthetic_dct_batch(16, seed=7), rounding_threshold_bits=7)
    sites = [o for o in c.ops if o.type == cc.OP_LUT and o.w == 7]
    assert sites and all(cc.is_split(o) for o in sites)
    assert all(not cc.is_split(o) for o in c.ops if o.type == cc.OP_LUT and o.w != 7)


@pytest.mark.parametrize("bit_width", [4, 5])
@pytest.mark.parametrize("name", ["r20_24_16", "r20_3_32", "r18_3_32"])
def test_benchmark_trunks_compile_exact_at_seven_bits(name, bit_width):
    from dctfhe import compile as cc, params as P
    c, _, warns = _compile(name, bit_width)
    assert not warns, warns
    ps = c.param_set
    names = [t.name for t in ps.tiers]
    # neither catalogue got a tier
    assert names == [t.name for t in P.params_for_bit_width(bit_width).tiers]
    sites = [o for o in c.ops if o.type == cc.OP_LUT and o.w == 7]
    assert len(sites) >= 20, len(sites)
    assert c.worst_site_failure <= 1e-12, c.worst_site_failure
    for o in sites:
        assert o.ip[9] in (cc.LUT_SPLIT, cc.LUT_SPLIT_QUIET) and o.ip[2] == 7 and o.ip[5] == ps.bit_tier
        assert names[o.ip[4]] == "T6a" and o.payload.shape == (o.ip[6], 128)      # the tier a 6-bit site takes; one record, whole tables
        assert names[cc.second_tier(ps, o)] == ("T6" if o.ip[9] == cc.LUT_SPLIT_QUIET else "T6a")
        assert c.tensors[o.dst].e >= 1
        # r + 1 one-bit steps, handed over B -> Ba -> Ba2 in order
        order = [{"B": 0, "Ba": 1, "Ba2": 2}[names[cc.step_tier(o, i)]] for i in range(cc.chain_steps(o))]
        assert len(order) == o.r + 1 and order == sorted(order)
    # bootstraps per image: the steps, the parity bootstrap and both look-ups are all counted, on the tiers that run them
    want = {}
    for o in c.ops:
        if o.type != cc.OP_LUT:
            continue
        s = c.tensors[o.src0]
        n = s.C * s.H * s.W
        tiers = [o.ip[4]] + [cc.step_tier(o, i) for i in range(cc.chain_steps(o))]
        if cc.is_split(o):
            tiers += [cc.step_tier(o, o.r), cc.second_tier(ps, o)]
        for t in tiers:
            want[names[t]] = want.get(names[t], 0) + n
    assert c.pbs_counts() == want
    rep = c.report()
    assert "parity_split=T6a+T6a" in rep or "parity_split=T6a+T6" in rep
    if bit_width == 4:      # the sum of two one-level outputs stays inside every refresh's budget: no quiet twin needed
        assert all(o.ip[9] == cc.LUT_SPLIT for o in sites) and "T6" not in c.pbs_counts()
    else:                   # a 5-bit refresh (T5r) that reads a split site needs the second look-up on T6
        quiet = [o for o in sites if o.ip[9] == cc.LUT_SPLIT_QUIET]
        assert quiet and len(quiet) < len(sites)
        readers = {o.src0: o for o in c.ops if o.type == cc.OP_LUT}
        assert all("(refresh)" in readers[o.dst].note for o in quiet)


def _split_eval(blob, phases_in):
    """the circuit with every parity-split record evaluated AS the split: S[t'] + Dt[t'] for an even index, S[t'] - Dt[t'] for an odd
    one, half tables derived from the payload as the engine derives them (independent of dctfhe.compile.split_tables)"""
    from oracle import circuit_ref as R
    c = R.parse_blob(blob)
    T = c["tensors"]
    B = phases_in.shape[0]
    vals = {c["input"]: np.ascontiguousarray(phases_in, np.uint64).reshape(B, *T[c["input"]])}
    n_split = 0
    for o in c["ops"]:
        x, ip = vals[o["src0"]], o["ip"]
        if o["type"] == R.OP_LUT and ip[9] in (2, 3):
            p, r, w, shift, _, _, ntab = ip[:7]
            t = np.frombuffer(o["payload"], np.int64).reshape(ntab, 1 << w).view(np.uint64)
            s_tab = (t[:, 0::2] + t[:, 1::2]) >> np.uint64(1)
            d_tab = t[:, 0::2] - s_tab
            v = (x << np.uint64(shift)) + np.uint64(o["lp"][0] % (1 << 64))
            if r > 0:
                v = v + (np.uint64(1) << np.uint64(63 - p + r - 1))
            idx = ((v >> np.uint64(63 - w)) & np.uint64((1 << w) - 1)).astype(np.int64)
            ch = np.broadcast_to(np.arange(x.shape[1]).reshape(1, -1, 1, 1) if ntab > 1 else np.zeros((1, 1, 1, 1), np.int64), idx.shape)
            first, second = s_tab[ch, idx >> 1], d_tab[ch, idx >> 1]
            vals[o["dst"]] = first + np.where(idx & 1, np.uint64(0) - second, second)
            n_split += 1
        else:
            vals[o["dst"]] = R.eval_op(o, x, vals)[0]
    return vals[c["output"]].reshape(B, -1), n_split


@pytest.mark.parametrize("bit_width", [4, 5])
def test_oracle_interpreter_reads_split_blobs_unchanged(bit_width):
    """oracle/circuit_ref.run_clear on a 7-bit blob == the compile-time integer forward == the split evaluated as a split"""
    from dctfhe import compile as cc
    from oracle import circuit_ref
    c, calib, _ = _compile("r20_24_16", bit_width)
    assert struct.unpack_from("<II", c.blob, 0) == (cc.MAGIC, 1)
    q = cc.act_quant(calib[:4], c.in_scale, True, c.in_bits)
    ph = (q.astype(np.int64).astype(np.uint64) << np.uint64(c.e_in)).reshape(4, -1)
    out, overflow = circuit_ref.run_clear(c.blob, ph)
    assert not overflow
    vals = (out + (np.uint64(1) << np.uint64(c.e_out - 1))).view(np.int64) >> np.int64(c.e_out)
    assert np.array_equal(vals, c.calib_out[:4])
    assert np.array_equal(out & np.uint64((1 << c.e_out) - 1), np.zeros_like(out))        # exact: nothing below the encoding
    split_out, n_split = _split_eval(c.blob, ph)
    assert n_split == sum(1 for o in c.ops if o.type == cc.OP_LUT and o.w == 7) >= 20
    assert np.array_equal(split_out, out)


def test_split_table_identity():
    """S +- Dt == T (mod 2^64) for all 128 indices: random int64 tables with odd and negative entries, e = 1 ... 20, and entries
    next to the wrap-around; e = 0 with an odd sum has no exact half and is refused"""
    from dctfhe import compile as cc
    rng = np.random.default_rng(11)
    for e in range(1, 21):
        vals = rng.integers(-(1 << 40), 1 << 40, (5, 128), dtype=np.int64) | 1       # odd entries, both signs
        vals[0, :8] = [(1 << 62) - 1, -(1 << 62), (1 << 62) - 3, -(1 << 62) + 1, -1, 1, (1 << 62) - 1, (1 << 62) - 1]
        vals[1] = rng.integers(-(1 << 63 - e), 1 << 63 - e, 128, dtype=np.int64)     # fills the word: T << e wraps, sums carry out
        enc = np.array((vals.astype(object) * (1 << e)) % (1 << 64), dtype=np.uint64)
        s_tab, d_tab = cc.split_tables(enc.view(np.int64))
        assert s_tab.shape == d_tab.shape == (5, 64) and s_tab.dtype == np.uint64
        assert np.array_equal(s_tab + d_tab, enc[:, 0::2]) and np.array_equal(s_tab - d_tab, enc[:, 1::2])
    odd = np.array([[3, 4] + [0] * 126], np.int64)                                   # e = 0: 3 + 4 is odd
    with pytest.raises(ValueError, match="odd sum"):
        cc.split_tables(odd)
    assert cc.split_tables(np.array([[3, 5] + [0] * 126], np.int64))[0][0, 0] == 4    # e = 0 with an even sum is fine


def test_six_bit_blobs_unchanged():
    for bw, want in SHA_RTB6.items():
        c, _, _ = _compile("r20_24_16", bw, rtb=6)
        assert hashlib.sha256(c.blob).hexdigest() == want, bw
        assert all(o.ip[9] == 0 for o in c.ops if o.type == 4)


def test_refusals_name_their_reason():
    from dctfhe import compile as cc, models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from dctfhe.synthetic import synthetic_dct_batch
    calib = synthetic_dct_batch(16, seed=7)
    model = lambda: models.ResNet20QAT(5, 24, 16)
    with pytest.raises(ValueError, match="no tier for a table of 8 input bits"):
        cc.compile_model(model(), calib, rounding_threshold_bits=8)
    with pytest.raises(ValueError, match="needs the exact method"):
        compile_brevitas_qat_model(model(), calib, rounding_threshold_bits={"n_bits": 7, "method": "approximate"})
    with pytest.raises(ValueError, match="needs tier_policy='exact'"):
        cc.compile_model(model(), calib, rounding_threshold_bits=7, p_error=0.01, tier_policy="p_error")
    # a 7-bit table that does not come from the rounding threshold (a guaranteed range of 7 bits) takes the same road
    with pytest.raises(ValueError, match="needs the exact method"):
        cc.compile_model(model(), calib, rounding_threshold_bits=6, n_bits=7, rounding_method="approximate")
    # a catalogue with wider tables of its own keeps serving them directly (clear evaluation of fine grids)
    wide = P.ParamSet(D=8192, tiers=[P.TierSpec("wide", n=808, k=1, logN=13, l=3, beta=11, lk=9, betak=2),
                                     P.TierSpec("B", n=560, k=2, logN=10, l=2, beta=14, lk=5, betak=2)], bit_tier=1, table_tier_for_w={12: 0}, input_dim=2048)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = cc.compile_model(model(), calib, rounding_threshold_bits=8, param_set=wide)
    assert any(o.w == 8 for o in c.ops if o.type == cc.OP_LUT) and not any(cc.is_split(o) for o in c.ops if o.type == cc.OP_LUT)


def test_validate_rejects_unknown_lookup_modes():
    from dctfhe import _lib, compile as cc, models, params as P
    L = _lib.load()
    rng = np.random.default_rng(0)
    c = cc.compile_model(models.tiny_resnet_q(), rng.normal(0, 1, (48, 4, 6, 6)), rounding_threshold_bits=7, param_set=P.test_params())
    sites = [i for i, o in enumerate(c.ops) if o.type == cc.OP_LUT and cc.is_split(o)]
    assert sites and all(c.ops[i].ip[9] == cc.LUT_SPLIT for i in sites)          # test_params has no quiet twin
    assert L.dctfhe_circuit_validate(c.blob, len(c.blob)) == 0, L.dctfhe_last_error().decode()
    off = 32 + 16 * len(c.tensors) + 96 * sites[0] + 16 + 4 * 9                 # ip[9] of that record
    assert struct.unpack_from("<i", c.blob, off)[0] == cc.LUT_SPLIT
    for mode, ok in ((3, True), (4, False), (-1, False), (255, False)):
        blob = bytearray(c.blob)
        struct.pack_into("<i", blob, off, mode)
        rc = L.dctfhe_circuit_validate(bytes(blob), len(blob))
        assert (rc == 0) == ok, (mode, L.dctfhe_last_error().decode())
        if not ok:
            assert "unknown look-up mode" in L.dctfhe_last_error().decode()
    # a split record whose table pairs have no exact half
    poff = struct.unpack_from("<q", c.blob, 32 + 16 * len(c.tensors) + 96 * sites[0] + 16 + 48 + 16)[0]
    blob = bytearray(c.blob)
    struct.pack_into("<q", blob, poff, struct.unpack_from("<q", c.blob, poff)[0] + 1)
    assert L.dctfhe_circuit_validate(bytes(blob), len(blob)) != 0 and "odd sum" in L.dctfhe_last_error().decode()


def test_cli_accepts_seven_bits(monkeypatch):
    """homomorphic_eval.py --rounding_threshold_bits 7 --bit_width 5 (the reference's ImageNet setting): parsed, and the compile
    call the CLI makes with those arguments returns a circuit with split sites"""
    spec = importlib.util.spec_from_file_location("he_cli7", os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["homomorphic_eval.py", "--model", "ResNet20qat", "--dct_status", "--channels", "24", "--filter_size", "4",
                                      "--image_size_dct", "16", "--rounding_threshold_bits", "7", "--bit_width", "5"])
    ns = mod.parse_args()
    assert ns.rounding_threshold_bits == 7 and ns.bit_width == 5 and ns.rounding_method == "exact"
    from dctfhe import compile as cc, models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    from dctfhe.synthetic import synthetic_dct_batch
    model = models.model_dict["ResNet20qat"](bit_width=ns.bit_width, in_channels=ns.channels, img_size=ns.image_size_dct, num_classes=ns.num_classes)
    qm = compile_brevitas_qat_model(model, synthetic_dct_batch(16, seed=7), rounding_threshold_bits=ns.rounding_threshold_bits, n_bits=ns.n_bits,
                                    p_error=ns.p_error, tier_policy=ns.tier_policy)
    assert any(cc.is_split(o) for o in qm.compiled.ops if o.type == cc.OP_LUT)
    assert "parity_split" in qm.compiled.report()
