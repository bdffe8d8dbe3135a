"""Packed result ciphertexts, host side (no GPU): the compiler's choice of the tier that packs a circuit's results and its refusal
(dctfhe.compile.output_compaction), the numpy reference of the format (tests/packed_ref.py), the PackedCiphertexts wire form, the
binding of the three entry points, and the facade's switch (Configuration(compress_output_ciphertexts=...)) on stub device objects."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import packed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(ps, bit_width=None):
    from dctfhe import compile as cc, models
    calib = np.random.default_rng(0).normal(0, 1, (32, 4, 6, 6))
    model = models.tiny_resnet_q() if bit_width is None else models.tiny_resnet_q(bit_width=bit_width)
    return cc.compile_model(model, calib, rounding_threshold_bits=6, n_bits=5, param_set=ps)


# ------------------------------------------------------------------------------------------ compiler
def test_var_round16():
    from dctfhe import params as P
    assert P.var_round16(800) == (800 / 2 + 1) * 2.0 ** -32 / 12
    assert P.var_round16(48) == 25 * 2.0 ** -32 / 12


@pytest.mark.parametrize("bits,name,n,nbytes", [(4, "T6", 800, 1602), (5, "T5r", 856, 1714)])
def test_output_compaction_picks_the_quietest_owning_tier(bits, name, n, nbytes):
    from dctfhe import compile as cc, params as P
    ps = P.default_params() if bits == 4 else P.default_params_5bit()
    circ = _compile(ps, None if bits == 4 else 5)
    oc = cc.output_compaction(circ)
    t = ps.tiers[oc.tier]
    assert (oc.name, oc.n, oc.bytes_per_ciphertext) == (name, n, nbytes) and (t.name, t.n, t.ksk_share) == (name, n, -1)
    assert oc.pfail < 1e-12
    # the record restates the formulas: key switch over the output's effective dimension + 16-bit rounding, against the decode margin
    out = circ.tensors[circ.output_tensor]
    assert oc.var == P.var_keyswitch(out.deff, t) + P.var_round16(t.n)
    assert oc.pfail == P.p_fail(2.0 ** -(circ.out_bits + 3), out.var + oc.var)
    for u in ps.tiers:
        if u.ksk_share < 0:
            assert oc.var <= P.var_keyswitch(out.deff, u) + P.var_round16(u.n), u.name


def test_output_compaction_small_rings_and_blob_untouched():
    from dctfhe import compile as cc, params as P
    circ = _compile(P.test_params())
    blob, report = circ.blob, circ.report()
    oc = cc.output_compaction(circ)
    assert (oc.tier, oc.n, oc.bytes_per_ciphertext) == (0, 48, 98) and oc.pfail < 1e-12
    assert circ.blob == blob and circ.report() == report          # the record is not serialised


def test_output_compaction_refuses_a_noisy_key():
    from dctfhe import compile as cc, params as P
    ps = P.test_params()
    for t in ps.tiers:
        t.lwe_sigma = 2.0 ** -9
    circ = _compile(ps)
    with pytest.raises(ValueError, match="p_fail"):
        cc.output_compaction(circ)


# ------------------------------------------------------------------------------------------ reference
def test_reference_rounding_edges():
    x = np.array([0x00007FFFFFFFFFFF, 0x0000800000000000, 0xFFFF800000000000, 0xFFFF7FFFFFFFFFFF, 0x1234800000000000], np.uint64)
    assert packed_ref.pack16(x).tolist() == [0, 1, 0, 0xFFFF, 0x1235]       # down, tie up, carry out wraps to 0, no carry


def test_reference_decrypt_of_pack_is_pack_of_decrypt_up_to_rounding():
    rng = np.random.default_rng(3)
    n, count = 48, 1000
    s = rng.integers(0, 2, n).astype(np.uint8)
    small = rng.integers(0, 1 << 64, (count, n + 1), dtype=np.uint64)
    phase = small[:, n] - (small[:, :n] * s.astype(np.uint64)).sum(axis=1, dtype=np.uint64)
    got = packed_ref.decrypt_packed(packed_ref.pack16(small), s, n)
    assert got.dtype == np.uint64 and not (got & np.uint64((1 << 48) - 1)).any()
    d = ((got >> np.uint64(48)).astype(np.int64) - packed_ref.pack16(phase).astype(np.int64) + (1 << 15)) % (1 << 16) - (1 << 15)
    assert np.abs(d).max() <= int(s.sum()) + 1, (np.abs(d).max(), int(s.sum()))
    assert np.abs(d).max() > 0                                      # the bound is not vacuous: the roundings do show


# ------------------------------------------------------------------------------------------ wire form, binding
def test_packed_ciphertexts_round_trip_and_refusals():
    from dctfhe.engine import PackedCiphertexts
    rows = (np.arange(7 * 49, dtype=np.uint32) * 40503 % 65536).astype(np.uint16).reshape(7, 49)
    pc = PackedCiphertexts(48, rows)
    blob = pc.to_bytes()
    assert len(pc) == 7 and len(blob) == pc.nbytes == 20 + 2 * 7 * 49 and blob[:4] == b"DPCT"
    back = PackedCiphertexts.from_bytes(blob)
    assert back.n == 48 and back.rows.dtype == np.uint16 and np.array_equal(back.rows, rows)
    assert np.array_equal(PackedCiphertexts.from_bytes(bytearray(blob)).rows, rows)
    for bad in (b"XPCT" + blob[4:], blob[:-1], blob[:10], blob + b"\0\0", blob[:4] + b"\x02" + blob[5:]):
        with pytest.raises(ValueError):
            PackedCiphertexts.from_bytes(bad)
    with pytest.raises(ValueError):
        PackedCiphertexts(48, rows.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        PackedCiphertexts(0, rows)


def test_packed_entry_points_are_bound_and_declared():
    from dctfhe import _lib as lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dctfhe.h")).read()
    for name in ("dctfhe_session_download_packed", "dctfhe_keyswitch_pack", "dctfhe_decrypt_packed"):
        assert name in lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name


# ------------------------------------------------------------------------------------------ facade
class _StubTiming:
    total_ms, ks_ms, linear_ms, pbs_ms = 0.0, 0.0, 0.0, [0.0]


class _StubSession:
    """stands in for engine.Session: records which download ran"""

    def __init__(self, batch, n_out, n):
        self.batch, self.n_out, self.n, self.calls = batch, n_out, n, []

    def dims(self):
        return 8, 16

    def upload(self, cts, dim=None):
        self.calls.append("upload")

    def run(self, timing=False):
        return _StubTiming()

    def download(self, dim=None):
        self.calls.append("download")
        return np.zeros((self.batch, self.n_out, dim + 1), np.uint64)

    def download_packed(self, tier):
        from dctfhe.engine import PackedCiphertexts
        self.calls.append(("download_packed", tier))
        return PackedCiphertexts(self.n, np.zeros((self.batch * self.n_out, self.n + 1), np.uint16))


class _StubKeys:
    def __init__(self):
        self.calls = []

    def encrypt(self, phases, dim):
        return np.zeros((phases.size, dim + 1), np.uint64)

    def decrypt(self, cts, dim):
        self.calls.append("decrypt")
        return np.zeros(cts.shape[0], np.uint64)

    def decrypt_packed(self, packed):
        self.calls.append("decrypt_packed")
        return np.zeros(len(packed), np.uint64)


def _stubbed_module(configuration):
    from dctfhe import params as P
    from dctfhe.quantized_module import QuantizedModule
    circ = _compile(P.test_params())
    qm = QuantizedModule(circ, configuration=configuration)
    B = 2
    sess, keys = _StubSession(B, circ.n_out(), 48), _StubKeys()
    qm._sessions[("execute", B)] = sess
    qm._keys = keys
    q = qm.quantize_input(np.random.default_rng(1).normal(0, 1, (B, 4, 6, 6)))
    return qm, sess, keys, q


def test_default_configuration_takes_the_old_download_path():
    from dctfhe.quantized_module import Configuration
    assert Configuration().compress_output_ciphertexts is False
    assert Configuration(compress_output_ciphertexts=1).compress_output_ciphertexts is True
    for cfg in (None, Configuration()):
        qm, sess, keys, q = _stubbed_module(cfg)
        out = qm.forward_quantized(q, "execute")
        assert out.shape == (2, qm.compiled.n_out())
        assert sess.calls == ["upload", "download"] and keys.calls == ["decrypt"]          # download_packed is never called
        assert qm.last_io["output_bytes"] == 8 * (16 + 1) * 2 * qm.compiled.n_out()


def test_switch_downloads_and_decrypts_packed():
    from dctfhe import compile as cc
    from dctfhe.quantized_module import Configuration
    qm, sess, keys, q = _stubbed_module(Configuration(compress_output_ciphertexts=True))
    tier = cc.output_compaction(qm.compiled).tier
    out = qm.forward_quantized(q, "execute")
    assert out.shape == (2, qm.compiled.n_out())
    assert sess.calls == ["upload", ("download_packed", tier)] and keys.calls == ["decrypt_packed"]
    assert qm.last_io["output_bytes"] == 2 * (48 + 1) * 2 * qm.compiled.n_out()


def test_switch_raises_at_first_use_when_the_compiler_refuses():
    from dctfhe import params as P
    from dctfhe.quantized_module import Configuration, QuantizedModule
    ps = P.test_params()
    for t in ps.tiers:
        t.lwe_sigma = 2.0 ** -9
    qm = QuantizedModule(_compile(ps), configuration=Configuration(compress_output_ciphertexts=True))      # constructing is fine
    sess, keys = _StubSession(2, qm.compiled.n_out(), 48), _StubKeys()
    qm._sessions[("execute", 2)] = sess
    qm._keys = keys
    q = qm.quantize_input(np.random.default_rng(1).normal(0, 1, (2, 4, 6, 6)))
    with pytest.raises(ValueError, match="p_fail"):
        qm.forward_quantized(q, "execute")
    assert sess.calls == [] and keys.calls == []                    # refused before anything was encrypted or uploaded
