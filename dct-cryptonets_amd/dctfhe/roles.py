"""What a client, a data owner and a server do at the boundary of a circuit, written against a narrow SPEC object instead of the compiler's
CompiledCircuit: quantise / encode / decode, the ring plan of packed results, the public-key check, the encrypted evaluation and the
decryption of what it returns.  QuantizedModule (one process, the compiled circuit in memory) and dctfhe.deploy (separate processes, each
started from a file) run the same functions.

The spec object: in_scale, in_bits, e_in, e_out, out_scale (numbers) and n_out() -- dctfhe.compile.CompiledCircuit has them, and so has
what dctfhe.deploy loads from client.dctfhe / server.dctfhe.  The priced records (output compaction, public-input plan) are handed in by
the caller: the compiler prices them in one place, a loaded file carries them.

Nothing here imports the compiler or torch: a client or a data owner needs neither."""
import numpy as np

from .engine import PackedCiphertexts, PackedRing, PublicInputs, SeededCiphertexts


def act_quant(x, s, signed, bits):
    lo, hi = (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if signed else (0, 2 ** bits - 1)
    return np.clip(np.rint(x / s), lo, hi).astype(np.int64)


def output_form(v):
    """a compress_output_ciphertexts / packed value -> False, True (16-bit rows) or the string ring"""
    if isinstance(v, str):
        if v not in ("none", "rows", "ring"):
            raise ValueError(f"compress_output_ciphertexts {v!r} (False, True / 'rows', or 'ring')")
        return {"none": False, "rows": True, "ring": "ring"}[v]
    return bool(v)


# -- quantisation at the boundary ----------------------------------------------------------
def quantize_input(spec, x):
    return act_quant(np.asarray(x, np.float64), spec.in_scale, True, spec.in_bits)


def encode_input(spec, q):
    return (q.astype(np.int64).astype(np.uint64) << np.uint64(spec.e_in)).reshape(q.shape[0], -1)


def decode_output(spec, phases):
    e = spec.e_out
    return (phases + (np.uint64(1) << np.uint64(e - 1))).view(np.int64) >> np.int64(e)     # signed, rounded


def dequantize_output(spec, q):
    return q.astype(np.float64) * spec.out_scale


# -- the priced records against the keys that arrive -----------------------------------------
def check_public_key(plan, pk):
    """the loaded public key `pk` against the spec the public-input plan priced; raises RuntimeError (the caller closes pk)"""
    if pk.logN != plan.spec.logN or pk.sigma > plan.spec.sigma:
        raise RuntimeError(f"the public key (logN {pk.logN}, sigma {pk.sigma:.3g}) is not covered by the spec this configuration priced "
                           f"(logN {plan.spec.logN}, sigma {plan.spec.sigma:.3g})")


def ring_plan(oc, pk):
    """(tier, packing key) of a ring-packed download: the loaded packing key `pk` (None: none loaded) against the ring compaction `oc` the
    compiler priced; refuses before anything runs"""
    if pk is None:
        raise RuntimeError('compress_output_ciphertexts="ring" needs the client\'s result packing key: '
                           "fhe_circuit.load_result_packing_key(fhe_circuit.export_result_packing_key())")
    if (pk.logN, pk.l, pk.beta) != (oc.spec.logN, oc.spec.l, oc.spec.beta) or pk.n_max < oc.n:
        raise RuntimeError(f"the loaded result packing key (logN {pk.logN}, {pk.l} x {pk.beta} bits, n_max {pk.n_max}) is not the one this "
                           f"configuration prices (logN {oc.spec.logN}, {oc.spec.l} x {oc.spec.beta} bits, n {oc.n})")
    if pk.sigma > oc.spec.sigma:
        raise RuntimeError(f"the loaded result packing key is noisier (sigma {pk.sigma:.3g}) than the spec this configuration priced "
                           f"({oc.spec.sigma:.3g}): its p_fail is not covered")
    return oc.tier, pk


# -- data-owner side -------------------------------------------------------------------------
def encrypt_public(spec, public_key, x):
    """float inputs [B, C, H, W] -> PublicInputs (quantise, encode, encrypt with the loaded public key)"""
    q = quantize_input(spec, np.asarray(x))
    return public_key.encrypt(encode_input(spec, q).reshape(-1))


# -- server side -----------------------------------------------------------------------------
def parse_inputs(cts):
    """the to_bytes() form of SeededCiphertexts or PublicInputs (told apart by the magic) -> the object; anything else as it is"""
    if isinstance(cts, (bytes, bytearray, memoryview)):
        return PublicInputs.from_bytes(cts) if bytes(cts[:4]) == PublicInputs.MAGIC else SeededCiphertexts.from_bytes(cts)
    return cts


def evaluate_encrypted(sess, keys, cts, dim=None, packed=False, tier=None, pack_key=None):
    """one encrypted pass on session `sess` (made with the evaluation keys `keys`): upload cts (rows, SeededCiphertexts or PublicInputs), run, and
    download in the form `packed` says (False: rows, full width or compact as dim says; True: PackedCiphertexts on `tier`; "ring": a
    PackedRing on `tier` with `pack_key`).  Everything priced or refused was priced or refused by the caller."""
    if isinstance(cts, SeededCiphertexts):
        sess.upload_seeded(cts)
    elif isinstance(cts, PublicInputs):
        sess.upload_public(cts)
    else:
        sess.upload(cts, dim)
    sess.run()
    if packed == "ring":
        return sess.download_ring(tier, pack_key)
    if packed:
        return sess.download_packed(tier)
    if dim is None:
        return sess.download().reshape(-1, keys.D + 1)
    out_dim = sess.dims()[1]
    return sess.download(out_dim).reshape(-1, out_dim + 1)


# -- client side -----------------------------------------------------------------------------
def decrypt_result(spec, keys, x):
    """what evaluate_encrypted returned -> decoded integers [B, F].  keys: the client key (decrypt, decrypt_packed, decrypt_ring); x:
    PackedCiphertexts or a PackedRing, or the to_bytes() form of either, or rows [B * F, dim + 1] of uint64 (full width or the compact
    wire form)"""
    if isinstance(x, (bytes, bytearray, memoryview)):
        x = PackedRing.from_bytes(x) if bytes(x[:4]) == PackedRing.MAGIC else PackedCiphertexts.from_bytes(x)
    if isinstance(x, PackedRing):
        ph = keys.decrypt_ring(x)
    elif isinstance(x, PackedCiphertexts):
        ph = keys.decrypt_packed(x)
    else:
        x = np.asarray(x)
        ph = keys.decrypt(x, x.shape[-1] - 1)
    return decode_output(spec, ph.reshape(-1, spec.n_out()))
