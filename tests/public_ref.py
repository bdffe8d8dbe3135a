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


def draws(key32, call, first, n, sigma, ft=np.float64):
    """what call `call` of an encryptor whose generator key is `key32` draws at x in [first, first + n) (include/dctfhe.h, "Randomness"):
    u[x] the top bit of generator word (key, 3 call, x), e1[x] the Gaussian draw (key, 3 call + 1, x), e2[x] the draw (key, 3 call + 2, x)
    -> (u uint8, e1 int64, e2 int64), each of n values.  A range is made on its own (`first`): the generator is counter-based.  The caller
    cuts e1 at groups N_e and e2 at count.  ft: the float type of the Gaussian (tests/simulate_ref.py gauss, the draw of the library)"""
    import simulate_ref as R
    x = np.arange(first, first + n, dtype=np.uint64)
    u = (R.words_at(None, 3 * call, x, key32) >> U(63)).astype(np.uint8)
    e1 = R.gauss(None, 3 * call + 1, x, sigma, ft, key=key32)
    e2 = R.gauss(None, 3 * call + 2, x, sigma, ft, key=key32)
    return u, e1, e2


def draws_near_a_tie(key32, call, first, n, sigma):
    """[x] in the range whose e1 or e2, before the final rounding to a torus word, lies so close to a half-integer that the last bit of
    a math library could move it: within G = 256 times the largest |float64 - long double| of the unrounded draws of the range (the
    guard of tests/simulate_ref.py, in units of 2^-64; at sigma = 2^-48 a draw is some 2^16 units and G some 2^-28 of one).  A
    word-for-word comparison with the device asserts this empty for its seed first.  For |g sigma| < 1/2 only (asserted)"""
    import simulate_ref as R
    x = np.arange(first, first + n, dtype=np.uint64)
    close = np.zeros(n, bool)
    for stream in (3 * call + 1, 3 * call + 2):
        y = [R._normal(None, stream, x, ft, key32) * ft(sigma) for ft in (np.float64, np.longdouble)]
        assert (np.abs(y[1]) < 0.5).all()
        y = [v * type(v[0])(18446744073709551616.0) for v in y]
        G = 256 * float(np.abs(y[0].astype(np.longdouble) - y[1]).max())
        assert G < 0.01, G
        frac = y[1] - np.floor(y[1])
        close |= np.asarray(np.abs(frac - np.longdouble(0.5)) < G)
    return (first + np.flatnonzero(close)).tolist()


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
