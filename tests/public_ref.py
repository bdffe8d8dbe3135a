"""numpy restatement of public-key inputs (include/dctfhe.h): the encryptor on an expanded public key and given draws,
the server's sample extraction, and the phases a holder of the ring key reads off the wire words.  Everything mod 2^64 (uint64 wraps)."""
import numpy as np

from ring_ref import negashift

U = np.uint64


def negamul_binary(K, u):
    """K(X) u(X) mod X^N + 1, u binary: sum over the set bits of u of X^i K"""
    out = np.zeros(K.shape[-1], U)
    for i in np.flatnonzero(u):
        out += negashift(K, int(i))
    return out


def encrypt(rows, u, e1, e2, phases):
    """expanded key rows [2, N] (A, B), draws u [groups N] (0 / 1), e1 [groups N], e2 [count] (signed) and phases [count] -> the wire
    words: per group C_a = A u + e1 (N words), then C_b[i] = (B u)[i] + e2[i] + phase_i for its first m slots"""
    rows = np.asarray(rows, U)
    N = rows.shape[-1]
    phases = np.asarray(phases, U).reshape(-1)
    e1, e2 = np.asarray(e1).astype(np.int64).view(U), np.asarray(e2).astype(np.int64).view(U)
    count, out = phases.size, []
    for g in range(-(-count // N)):
        m = min(N, count - g * N)
        ug = np.asarray(u[g * N:(g + 1) * N])
        out.append(negamul_binary(rows[0], ug) + e1[g * N:(g + 1) * N])
        out.append(negamul_binary(rows[1], ug)[:m] + e2[g * N:g * N + m] + phases[g * N:g * N + m])
    return np.concatenate(out) if out else np.zeros(0, U)


def extract(words, logN, count, dim):
    """wire words -> LWE rows [count, dim + 1]: slot i of a group has a_j = C_a[i - j] (j <= i), -C_a[N + i - j] (i < j < N), zeros up to
    dim, body C_b[i]"""
    N = 1 << logN
    words = np.asarray(words, U)
    out = np.zeros((count, dim + 1), U)
    for g in range(-(-count // N)):
        m = min(N, count - g * N)
        A, B = words[g * 2 * N:g * 2 * N + N], words[g * 2 * N + N:g * 2 * N + N + m]
        for i in range(m):
            out[g * N + i, :i + 1] = A[i::-1]
            out[g * N + i, i + 1:N] = U(0) - A[:i:-1]
        out[g * N:g * N + m, dim] = B
    return out


def decrypt(words, Z, logN, count):
    """wire words -> phases: coefficient i of C_b - C_a Z under the ring key bits Z (the first N bits of the big key)"""
    N = 1 << logN
    words = np.asarray(words, U)
    out = np.empty(count, U)
    for g in range(-(-count // N)):
        m = min(N, count - g * N)
        A, B = words[g * 2 * N:g * 2 * N + N], words[g * 2 * N + N:g * 2 * N + N + m]
        out[g * N:g * N + m] = B - negamul_binary(A, np.asarray(Z[:N]))[:m]
    return out


def lwe_phase(rows, S):
    """LWE rows [count, dim + 1] under the first dim bits of S -> body - <mask, S>"""
    rows = np.asarray(rows, U)
    dim = rows.shape[1] - 1
    return rows[:, dim] - (rows[:, :dim] * np.asarray(S[:dim]).astype(U)).sum(axis=1, dtype=U)
