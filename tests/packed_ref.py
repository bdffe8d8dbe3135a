"""numpy reference of the packed result form (include/dctfhe.h dctfhe_session_download_packed): small ciphertexts
rounded to 16 bits per word, and their decryption on the 16-bit torus."""
import numpy as np


def pack16(small):
    """u64 words -> uint16: (word + 2^47) >> 48 -- round to nearest on the 2^-16 grid, a tie goes up, a carry out of the top wraps to 0"""
    small = np.asarray(small, np.uint64)
    return ((small + np.uint64(1 << 47)) >> np.uint64(48)).astype(np.uint16)


def decrypt_packed(rows, key_bits, n):
    """rows [count, n + 1] uint16, key_bits: the small key (its first n bits are used) -> phases as phase16 << 48 (uint64)"""
    rows = np.asarray(rows, np.uint16).reshape(-1, n + 1).astype(np.uint64)
    s = np.asarray(key_bits[:n], np.uint64)
    ph16 = (rows[:, n] - (rows[:, :n] * s).sum(axis=1, dtype=np.uint64)) & np.uint64(0xFFFF)
    return ph16 << np.uint64(48)
