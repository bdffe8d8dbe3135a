"""Noise-free numpy interpreter for circuit blobs that contain max-pool ops (type 5), on the phase domain.

Test infrastructure only.  Ops 1-4 are evaluated as oracle/circuit_ref.py evaluates them (its blob parser and wrap-around convolution
are reused; the rest is restated here); op 5 follows the MaxPool2d contract: out[c, yo, xo] is the maximum of the in-range taps
in[c, yo*s - p + i, xo*s - p + j], 0 <= i, j < k, of the words read as signed int64 (floor mode, out-of-range taps ignored).
Shares no code with the product.
"""
import numpy as np

from oracle.circuit_ref import _conv_u64, parse_blob

OP_CONV, OP_ADD, OP_SUMPOOL, OP_LUT, OP_MAXPOOL = 1, 2, 3, 4, 5


def max_pool_words(x, k, s, p):
    """x uint64 [B, C, H, W] -> signed-word maximum over every k x k window"""
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xs = x.view(np.int64)
    out = np.empty((B, C, Ho, Wo), np.int64)
    for yo in range(Ho):
        ys = [y for y in range(yo * s - p, yo * s - p + k) if 0 <= y < H]
        for xo in range(Wo):
            xs_ = [xx for xx in range(xo * s - p, xo * s - p + k) if 0 <= xx < W]
            out[:, :, yo, xo] = xs[:, :, ys][:, :, :, xs_].max(axis=(2, 3))
    return out.view(np.uint64)


def run_clear(blob, phases_in, all_tensors=False):
    """phases_in: uint64 [B, n_in] -> (uint64 [B, n_out], overflow flag); all_tensors: the phases of every tensor, by id, instead"""
    c = parse_blob(blob)
    T = c["tensors"]
    B = phases_in.shape[0]
    vals = {c["input"]: np.ascontiguousarray(phases_in, np.uint64).reshape(B, *T[c["input"]])}
    overflow = False
    for o in c["ops"]:
        x = vals[o["src0"]]
        ip = o["ip"]
        if o["type"] == OP_CONV:
            Cout, KH, KW, stride, pad = ip[:5]
            y = _conv_u64(x, np.frombuffer(o["payload"], np.int8).reshape(Cout, x.shape[1], KH, KW), stride, pad)
        elif o["type"] == OP_ADD:
            y = x + vals[o["src1"]]
        elif o["type"] == OP_SUMPOOL:
            K = ip[0]
            Ho, Wo = x.shape[2] // K, x.shape[3] // K
            y = x[:, :, :Ho * K, :Wo * K].reshape(B, x.shape[1], Ho, K, Wo, K).sum(axis=(3, 5), dtype=np.uint64)
        elif o["type"] == OP_LUT:
            p, r, w, shift, _, _, ntab = ip[:7]
            tables = np.frombuffer(o["payload"], np.int64).reshape(ntab, 1 << w).view(np.uint64)
            v = (x << np.uint64(shift)) + np.uint64(o["lp"][0] % (1 << 64))
            if r > 0:
                v = v + (np.uint64(1) << np.uint64(63 - p + r - 1))
            overflow |= bool((v >> np.uint64(63)).any())
            idx = ((v >> np.uint64(63 - w)) & np.uint64((1 << w) - 1)).astype(np.int64)
            ch = np.arange(x.shape[1]).reshape(1, -1, 1, 1) if ntab > 1 else np.zeros((1, 1, 1, 1), np.int64)
            y = tables[np.broadcast_to(ch, idx.shape), idx]
        elif o["type"] == OP_MAXPOOL:
            y = max_pool_words(x, ip[0], ip[1], ip[2])
        else:
            raise ValueError("unknown op")
        vals[o["dst"]] = y
    if all_tensors:
        return vals, overflow
    return vals[c["output"]].reshape(B, -1), overflow
