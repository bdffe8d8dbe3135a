"""`simulate` restated in numpy: the clear-mode circuit with the compiler's noise sampled at every look-up, draw by
draw.  TEST INFRASTRUCTURE ONLY.  It shares one thing with the product, dctfhe_rng_host for the generator words (which has known-answer
tests of its own, tests/test_abi_validation.py); the draw, the look-up, the four modes of a look-up site, the two passes of a max pool and
the stream ids are written here from the definition, on top of the noise-free interpreter oracle/circuit_ref.py for the levelled ops.

A draw is a documented function of two generator words, so a device run can be compared WORD FOR WORD -- provided no draw lands so close
to a box edge that a last-bit difference between the device's log / sqrt / cospi and numpy's could move it across.  `Trace` records every
noisy position; near_edge() lists the elements within a guard of an edge (the sign flip at 2^63 is one), guard() sizes that guard from the
distance between this twin in float64 and in long double.  A test asserts near_edge() empty for its seed and then compares exactly."""
import ctypes as C
import os
import struct

import numpy as np

from oracle import circuit_ref

U = np.uint64
STREAM0 = 0x51D0000
POOL_BIT = 1 << 40
GUARD_MIN = 1 << 16          # units of 2^-64
GUARD_MARGIN = 256           # over the measured |float64 - long double|: for a device libm that cannot be measured on the host
_PI_LD = np.longdouble("3.14159265358979323846264338327950288")
_lib_handle = None


def _lib():
    global _lib_handle
    if _lib_handle is None:
        from dctfhe import _lib
        if not os.path.exists(_lib.LIB_PATH):
            import __graft_entry__
            __graft_entry__.build()
        _lib_handle = C.CDLL(_lib.LIB_PATH)
    return _lib_handle


def sim_key(seed):
    """the generator key of a session's noise: words (seed lo, seed hi, 'simu', 0, 0, 0, 0, 0), little-endian"""
    return struct.pack("<8I", seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 0x73696D75, 0, 0, 0, 0, 0)


def words_at(seed, stream, idx, key=None):
    """generator words `idx` (any integer array) of (key of `seed`, stream); key: 32 generator-key bytes instead of a session's seed"""
    idx = np.asarray(idx, np.uint64)
    if idx.size == 0:
        return np.empty(idx.shape, np.uint64)
    lo, hi = int(idx.min()), int(idx.max())
    out = np.empty(hi - lo + 1, np.uint64)
    rc = _lib().dctfhe_rng_host(sim_key(seed) if key is None else bytes(key), C.c_uint64(stream), C.c_uint64(lo), C.c_size_t(out.size), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out[(idx - U(lo)).astype(np.int64)]


def _normal(seed, stream, idx, ft, key=None):
    """the standard normal of draw `idx` in float type `ft`: Box-Muller on words 2 idx and 2 idx + 1.  cospi(2 u2) with the argument
    reduced exactly: 2 u2 is a multiple of 2^-52 in [0, 2), and so is every difference below, so only the last cos / sin rounds"""
    idx = np.asarray(idx, np.uint64)
    w1, w2 = words_at(seed, stream, U(2) * idx, key), words_at(seed, stream, U(2) * idx + U(1), key)
    two53 = ft(9007199254740992.0)
    u1 = ((w1 >> U(11)).astype(ft) + ft(1)) / two53
    a = (w2 >> U(11)).astype(ft) / two53 * ft(2)          # [0, 2)
    a = np.where(a > 1, ft(2) - a, a)                     # cos(pi a) = cos(pi (2 - a)): [0, 1]
    neg = a > ft(0.5)
    a = np.where(neg, ft(1) - a, a)                       # cos(pi a) = -cos(pi (1 - a)): [0, 1/2]
    pi = _PI_LD if ft is np.longdouble else ft(np.pi)
    c = np.where(a <= ft(0.25), np.cos(pi * a), np.sin(pi * (ft(0.5) - a)))
    c = np.where(neg, -c, c)
    return np.sqrt(ft(-2) * np.log(u1)) * c


def gauss(seed, stream, idx, sigma, ft=np.float64, allow_wrap=False, key=None):
    """draw `idx` of `stream`: rint(x 2^64) as int64 with x = g sigma reduced to [-1/2, 1/2] by x - rint(x) (the identity unless
    |g sigma| >= 1/2, which a caller must allow by name); 0 where sigma <= 0"""
    idx = np.asarray(idx, np.uint64)
    if sigma <= 0:
        return np.zeros(idx.shape, np.int64)
    x = _normal(seed, stream, idx, ft, key) * ft(sigma)
    assert allow_wrap or (np.abs(x) < 0.5).all(), "a draw of half the torus or more: |g sigma| >= 1/2"
    x = x - np.rint(x)
    assert (np.abs(x) < 0.5).all()
    return np.rint(x * ft(18446744073709551616.0)).astype(np.int64)


def gauss_ld(seed, stream, idx, sigma, allow_wrap=False):
    """the same draw in long double: only to size the guard"""
    return gauss(seed, stream, idx, sigma, np.longdouble, allow_wrap)


class Trace:
    """every noisy look-up of a twin run: (op, stream, draw indices, sigma, table bits, positions, element numbers)"""

    def __init__(self, allow_wrap=False):
        self.records, self.allow_wrap = [], allow_wrap

    def add(self, op, stream, idx, sigma, w, pos, elem):
        self.records.append(dict(op=op, stream=stream, idx=np.asarray(idx, np.uint64).ravel(), sigma=float(sigma), w=w,
                                 pos=np.asarray(pos, np.uint64).ravel(), elem=np.asarray(elem, np.int64).ravel()))

    def draws(self):
        return sum(r["idx"].size for r in self.records)


def draw_difference(seed, trace):
    """largest |float64 draw - long-double draw|, in units of 2^-64, over the draws of `trace`"""
    worst = 0
    for r in trace.records:
        if r["idx"].size:
            d = gauss(seed, r["stream"], r["idx"], r["sigma"], allow_wrap=trace.allow_wrap) - gauss_ld(seed, r["stream"], r["idx"], r["sigma"], trace.allow_wrap)
            worst = max(worst, int(np.abs(d).max()))
    return worst


def guard(seed, trace):
    """G: GUARD_MARGIN times the measured difference, never below GUARD_MIN"""
    return max(GUARD_MIN, GUARD_MARGIN * draw_difference(seed, trace))


def near_edge(trace, G):
    """[(op, element)] whose noisy position lies within G of a multiple of 2^(63 - w): a box edge, or the sign flip at 2^63"""
    out = []
    for r in trace.records:
        box = 1 << (63 - r["w"])
        assert 2 * G < box
        d = r["pos"] & U(box - 1)
        close = (d < U(G)) | (d > U(box - G))
        out += [(r["op"], int(e)) for e in np.unique(r["elem"][close])]
    return out


def noisy_lookup(centre, w, table, draw):
    """-> (entries, positions): pos = centre + draw + 2^(62 - w); entry (pos >> (63 - w)) mod 2^w of `table` (one table, or one row per
    element), negated where bit 63 of pos is set"""
    pos = centre + draw.view(np.uint64) + U(1 << (62 - w))
    j = ((pos >> U(63 - w)) & U((1 << w) - 1)).astype(np.int64)
    t = table[j] if table.ndim == 1 else np.take_along_axis(table, j[..., None], -1)[..., 0]
    return np.where((pos >> U(63)).astype(bool), U(0) - t, t), pos


def split_tables(T):
    """T uint64 [ntab, 2^w] -> (S, Dt): S[j] = ((T[2j] + T[2j+1]) mod 2^64) >> 1, Dt[j] = T[2j] - S[j]"""
    S = (T[:, 0::2] + T[:, 1::2]) >> U(1)
    return S, T[:, 0::2] - S


def lut_stream(run, op):
    return STREAM0 + (run << 12) + op


def pool_streams(run, op):
    """(row pass, column pass)"""
    P = POOL_BIT | (lut_stream(run, op) << 1)
    return P, P + 1


def lut_site(x, p, r, w, shift, body_add, mode, tables, seed, stream, sigma, sigma2=0.0, trace=None, op=0):
    """x uint64 [B, C, H, W]; tables uint64 [ntab, 2^w] -> (outputs, overflow flag)"""
    g = np.arange(x.size, dtype=np.uint64).reshape(x.shape)
    return lut_elements(x, g, x.shape[2] * x.shape[3], p, r, w, shift, body_add, mode, tables, seed, stream, sigma, sigma2, trace, op)


def lut_elements(x, g, hw, p, r, w, shift, body_add, mode, tables, seed, stream, sigma, sigma2=0.0, trace=None, op=0):
    """the site on the words x of the elements numbered g in the whole tensor (uint64 arrays of one shape; a channel is hw elements):
    table and draws go by g, so any range of a tensor can be evaluated on its own -> (outputs, overflow flag among these elements)"""
    approx, split = mode == 1, mode in (2, 3)
    v = (x << U(shift)) + U(body_add % (1 << 64))
    if r > 0 and not (approx and sigma > 0):
        v = v + U(1 << (63 - p + r - 1))
    overflow = bool((v >> U(63)).any())
    idx = (v >> U(63 - w)) & U((1 << w) - 1)
    ntab = tables.shape[0]
    ti = ((g // U(hw)) % U(ntab)).astype(np.int64) if ntab > 1 else np.zeros(x.shape, np.int64)
    if sigma <= 0:
        return tables[ti, idx.astype(np.int64)], overflow
    aw = trace.allow_wrap if trace is not None else False
    if split:
        S, Dt = split_tables(tables)
        centre = (idx >> U(1)) << U(64 - w)
        s2 = sigma2 if sigma2 and sigma2 > 0 else sigma
        y1, pos1 = noisy_lookup(centre, w - 1, S[ti], gauss(seed, stream, U(2) * g, sigma, allow_wrap=aw))
        y2, pos2 = noisy_lookup(centre + ((idx & U(1)) << U(63)), w - 1, Dt[ti], gauss(seed, stream, U(2) * g + U(1), s2, allow_wrap=aw))
        if trace is not None:
            trace.add(op, stream, U(2) * g, sigma, w - 1, pos1, g)
            trace.add(op, stream, U(2) * g + U(1), s2, w - 1, pos2, g)
        return y1 + y2, overflow
    centre = v + U(1 << (62 - p)) if (approx and r > 0) else idx << U(63 - w)
    y, pos = noisy_lookup(centre, w, tables[ti], gauss(seed, stream, g, sigma, allow_wrap=aw))
    if trace is not None:
        trace.add(op, stream, g, sigma, w, pos, g)
    return y, overflow


def pool_pass(a, k, s, p, shift, body_add, p_d, table, seed, stream, sigma, trace=None, op=0):
    """one 1-D pass of a max pool: a uint64 [outer, n_in, inner] -> [outer, n_out, inner].  Every output folds its in-range taps in tap
    order: the first gives m = x, each later one m += noisy relu of the difference (sigma = 0: the signed-word maximum)"""
    outer, n_in, inner = a.shape
    n_out = (n_in + 2 * p - k) // s + 1
    e = np.arange(outer * n_out * inner, dtype=np.uint64).reshape(outer, n_out, inner)
    m = np.zeros((outer, n_out, inner), np.uint64)
    taken = np.zeros((outer, n_out, inner), np.uint64)
    aw = trace.allow_wrap if trace is not None else False
    for j in range(k):
        xi = np.arange(n_out) * s - p + j
        valid = np.broadcast_to(((xi >= 0) & (xi < n_in))[None, :, None], m.shape)
        v = a[:, np.clip(xi, 0, n_in - 1), :]
        first, later = valid & (taken == 0), valid & (taken > 0)
        m = np.where(first, v, m)
        if sigma > 0:
            d = ((v - m) << U(shift)) + U(body_add % (1 << 64))
            centre = ((d >> U(63 - p_d)) & U((1 << p_d) - 1)) << U(63 - p_d)
            di = (e * U(64) + taken)[later]
            y, pos = noisy_lookup(centre[later], p_d, table, gauss(seed, stream, di, sigma, allow_wrap=aw))
            m[later] += y
            if trace is not None:
                trace.add(op, stream, di, sigma, p_d, pos, e[later])
        else:
            m = np.where(later & (v.view(np.int64) > m.view(np.int64)), v, m)
        taken = taken + valid.astype(np.uint64)
    return m


def max_pool(x, k, s, p, shift, body_add, p_d, table, seed, streams, sigma, trace=None, op=0):
    """x uint64 [B, C, H, W] -> (row-pass result [B, C, H, Wo], output [B, C, Ho, Wo])"""
    B, Cc, H, W = x.shape
    mid = pool_pass(x.reshape(B * Cc * H, W, 1), k, s, p, shift, body_add, p_d, table, seed, streams[0], sigma, trace, op)
    Wo = mid.shape[1]
    out = pool_pass(mid.reshape(B * Cc, H, Wo), k, s, p, shift, body_add, p_d, table, seed, streams[1], sigma, trace, op)
    return mid.reshape(B, Cc, H, Wo), out.reshape(B, Cc, -1, Wo)


def run_simulate(blob, phases, seed, sigmas, sigmas2=None, run=0, all_tensors=False, trace=None):
    """phases uint64 [B, n_in] -> (uint64 [B, n_out], overflow flag) of pass `run` of a session with set_noise(seed, sigmas) and
    set_noise_split(sigmas2); all_tensors: the phases of every tensor, by id, instead.  trace: a Trace to fill"""
    c = circuit_ref.parse_blob(blob)
    T = c["tensors"]
    B = phases.shape[0]
    vals = {c["input"]: np.ascontiguousarray(phases, np.uint64).reshape(B, *T[c["input"]])}
    overflow = False
    for i, o in enumerate(c["ops"]):
        x, ip = vals[o["src0"]], o["ip"]
        sg = float(sigmas[i]) if sigmas is not None and i < len(sigmas) else 0.0
        if o["type"] == circuit_ref.OP_LUT:
            p, r, w, shift, ntab, mode = ip[0], ip[1], ip[2], ip[3], ip[6], ip[9]
            tables = np.frombuffer(o["payload"], np.int64).reshape(ntab, 1 << w).view(np.uint64)
            sg2 = float(sigmas2[i]) if sigmas2 is not None and i < len(sigmas2) else 0.0
            vals[o["dst"]], over = lut_site(x, p, r, w, shift, o["lp"][0], mode, tables, seed, lut_stream(run, i), sg, sg2, trace, i)
        elif o["type"] == circuit_ref.OP_MAXPOOL and sg > 0:
            table = np.frombuffer(o["payload"], np.int64).view(np.uint64)
            _, vals[o["dst"]] = max_pool(x, ip[0], ip[1], ip[2], ip[3], o["lp"][0], ip[5], table, seed, pool_streams(run, i), sg, trace, i)
            over = False
        else:
            vals[o["dst"]], over = circuit_ref.eval_op(o, x, vals)
        overflow |= over
    if all_tensors:
        return vals, overflow
    return vals[c["output"]].reshape(B, -1), overflow


# ------------------------------------------------------------------------------------------ small blobs
def lut_record(p, r, w, shift=0, mode=0, tables=None, body_add=0):
    """tables: int64 [ntab, 2^w]"""
    tables = np.ascontiguousarray(tables, np.int64).reshape(-1, 1 << w)
    return dict(type=circuit_ref.OP_LUT, ip=[p, r, w, shift, 0, 1, tables.shape[0], -1, 1, mode, 0, -1], lp=body_add, payload=tables.tobytes())


def pool_record(k, s, pad, p_d, table, shift=0, body_add=1 << 62):
    """table: 2^p_d int64 entries (the relu of the signed differences, offset-binary: body_add = 2^62 puts a zero difference mid-table)"""
    table = np.ascontiguousarray(table, np.int64).reshape(1 << p_d)
    return dict(type=circuit_ref.OP_MAXPOOL, ip=[k, s, pad, shift, 0, p_d, 1, 0, 0, 0, 0, 0], lp=body_add, payload=table.tobytes())


def chain_blob(shape, records, max_bit_width=7):
    """a circuit of one or two records in a row on an input of `shape` = (C, H, W); tensor i + 1 is record i's output"""
    shapes = [tuple(shape)]
    for rec in records:
        Cc, H, W = shapes[-1]
        if rec["type"] == circuit_ref.OP_MAXPOOL:
            k, s, pad = rec["ip"][:3]
            shapes.append((Cc, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1))
        else:
            shapes.append((Cc, H, W))
    head = struct.pack("<IIiiiiii", 0x46544344, 1, len(shapes), len(records), 0, len(records), max_bit_width, 0)
    tens = b"".join(struct.pack("<iiii", *s, 0) for s in shapes)
    off = len(head) + len(tens) + 96 * len(records)
    recs, payloads = b"", b""
    for i, rec in enumerate(records):
        lp0 = rec["lp"] - (1 << 64) if rec["lp"] >= (1 << 63) else rec["lp"]
        recs += struct.pack("<iiii12i2qqq", rec["type"], i, 0, i + 1, *rec["ip"], lp0, 0, off + len(payloads), len(rec["payload"]))
        payloads += rec["payload"] + b"\0" * ((-len(rec["payload"])) % 16)
    blob = head + tens + recs + payloads
    L = _lib()
    L.dctfhe_last_error.restype = C.c_char_p
    assert L.dctfhe_circuit_validate(blob, C.c_size_t(len(blob))) == 0, L.dctfhe_last_error().decode()
    return blob
