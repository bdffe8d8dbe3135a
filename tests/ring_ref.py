"""numpy restatement of ring-packed results (include/dctfhe.h): the signed decomposition, the pack of small
ciphertexts with an expanded packing key, the 16-bit wire rounding and the client's decryption.  Everything mod 2^64 (uint64 wraps)."""
import numpy as np

U = np.uint64


def decompose(v, l, beta):
    """uint64 array -> int64 digits [..., l], most significant first: oracle/tfhe_ref.c ref_decompose (digits in [-B/2, B/2), the top
    carry dropped)"""
    v = np.atleast_1d(np.asarray(v, U))
    tot = l * beta
    x = (v + U(1 << (63 - tot))) >> U(64 - tot)
    B, half, mask = 1 << beta, U(1 << (beta - 1)), U((1 << beta) - 1)
    out = np.empty(v.shape + (l,), np.int64)
    carry = np.zeros(v.shape, U)
    for lev in range(l - 1, -1, -1):
        d = (x & mask) + carry
        x = x >> U(beta)
        hi = d >= half
        out[..., lev] = np.where(hi, d.astype(np.int64) - B, d.astype(np.int64))
        carry = hi.astype(U)
    return out


def negashift(v, i):
    """X^i v(X) mod X^N + 1, 0 <= i < N"""
    N = v.shape[-1]
    return v.copy() if i == 0 else np.concatenate([U(0) - v[..., N - i:], v[..., :N - i]], axis=-1)


def pack(small, key, l, beta):
    """small ciphertexts [count, n + 1] and the expanded key [n_max, l, 2, N] -> accumulators [groups, 2, N] (mask, body) of uint64:
    per group acc = (0, sum_i b_i X^i) - sum_i X^i sum_{j, lev} dig_lev(a_ij) PK[j][lev]"""
    small = np.asarray(small, U)
    count, n = small.shape[0], small.shape[1] - 1
    N = key.shape[-1]
    K = np.ascontiguousarray(key[:n], U).reshape(n * l, 2 * N)
    groups = -(-count // N)
    acc = np.zeros((groups, 2, N), U)
    dig = decompose(small[:, :n], l, beta).reshape(count, n * l).astype(U)        # two's complement: the products wrap like the signed ones
    prod = (dig @ K).reshape(count, 2, N)
    for c in range(count):
        g, i = divmod(c, N)
        acc[g] -= negashift(prod[c], i)
        acc[g, 1, i:i + 1] += small[c:c + 1, n]
    return acc


def round16(w):
    return ((np.asarray(w, U) + U(1 << 47)) >> U(48)).astype(np.uint16)


def pack16(acc, count):
    """accumulators -> the wire words: per group its N mask words, then its first m body words, rounded like k_pack16"""
    N = acc.shape[-1]
    out = []
    for g in range(acc.shape[0]):
        m = min(N, count - g * N)
        out += [round16(acc[g, 0]), round16(acc[g, 1, :m])]
    return np.concatenate(out) if out else np.zeros(0, np.uint16)


def decrypt16(words, Z, logN, count):
    """wire words -> phases (phase16 << 48) under the ring key bits Z (the first N bits of the big key)"""
    N = 1 << logN
    words = np.asarray(words, np.uint16).astype(np.int64)
    out = np.empty(count, U)
    for g in range(-(-count // N)):
        m = min(N, count - g * N)
        A, B = words[g * 2 * N:g * 2 * N + N], words[g * 2 * N + N:g * 2 * N + N + m]
        AZ = np.zeros(N, np.int64)
        for c in np.flatnonzero(np.asarray(Z[:N])):
            AZ += A if c == 0 else np.concatenate([-A[N - c:], A[:N - c]])
        out[g * N:g * N + m] = ((B - AZ[:m]) & 0xFFFF).astype(U) << U(48)
    return out
