"""The margin audit's definition in numpy (include/dctfhe.h), for the tests to hold the library against.

A small ciphertext (a_0 .. a_{n-1}, b) on a ring of N = 2^logN meets a table of w input bits:
    lv(x) = ((x >> (62 - logN)) + 1) >> 1                   the bootstrap's rounding to 2N levels (2N itself wraps to 0 below)
    phi   = (lv(b) - sum_{i<n} s_i lv(a_i)) mod 2N
    G = 2^(logN - w), h = G / 2;   e = ((phi + h) mod G) - h     in [-h, h)
and the statistics are plain integer sums over the ciphertexts."""
import numpy as np

BINS = 16


def levels(words, logN):
    w = np.asarray(words, np.uint64)
    return ((w >> np.uint64(62 - logN)) + np.uint64(1)) >> np.uint64(1)


def errors(small_key, n, logN, cts_small, table_bits):
    """-> int32 e per row of cts_small [count, n + 1]"""
    cts = np.asarray(cts_small, np.uint64).reshape(-1, n + 1)
    s = np.asarray(small_key[:n], np.uint64)
    lv = levels(cts, logN)
    two_n = np.uint64(2 << logN)
    phi = (lv[:, n] + two_n * np.uint64(n + 1) - (lv[:, :n] * s[None, :]).sum(axis=1, dtype=np.uint64)) % two_n
    G = np.uint64(1 << (logN - table_bits))
    h = G >> np.uint64(1)
    return (((phi + h) % G).astype(np.int64) - np.int64(h)).astype(np.int32)


def stats(e, logN, table_bits, op=-1, entry=-1, tier=-1):
    """the dict dctfhe.engine.margin_stats_dict makes of a dctfhe_margin_stats"""
    e = np.asarray(e, np.int64)
    h = 1 << (logN - table_bits - 1)
    a = np.abs(e)
    bins = np.minimum(BINS - 1, 16 * a // h)
    return dict(op=op, entry=entry, tier=tier, table_bits=table_bits, half_box=h, max_abs=int(a.max()) if e.size else 0, count=int(e.size),
                sum=int(e.sum()), sum_sq=int((e * e).sum()), hist=[int((bins == b).sum()) for b in range(BINS)])


def trivial_rows(n, logN, levels_):
    """zero-mask small ciphertexts whose body sits exactly on the given levels of 2N"""
    rows = np.zeros((len(levels_), n + 1), np.uint64)
    rows[:, n] = np.asarray(levels_, np.uint64) << np.uint64(63 - logN)
    return rows
