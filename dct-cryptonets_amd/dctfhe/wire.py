"""Wire objects of the client / data-owner / server boundary and the key seed: numpy and struct only.  No native library is loaded
here, so the GPU engine (dctfhe.engine) and the host client (dctfhe.host_client) share them."""
import hashlib
import os
import struct

import numpy as np


def seed_bytes(seed=None):
    """The 32-byte CSPRNG seed of a client key.  None: fresh from the OS (os.urandom) -- the default everywhere;
    32 bytes: used as they are (a persisted or broadcast key); int: a DETERMINISTIC seed for tests and reproducible
    experiments (SHA-256 of a label and the integer) -- guessable by construction, never for real data."""
    if seed is None:
        return os.urandom(32)
    if isinstance(seed, (bytes, bytearray)):
        if len(seed) != 32:
            raise ValueError("a key seed is exactly 32 bytes")
        return bytes(seed)
    return hashlib.sha256(b"dctfhe deterministic test seed " + str(int(seed)).encode()).digest()


def _as_u8(blob):
    return np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, np.uint8)


class SeededCiphertexts:
    """Input ciphertexts in SEEDED form (include/dctfhe.h dctfhe_encrypt_seeded): the 32-byte public mask key, the generator stream and
    one body per ciphertext.  Mask word j < input_dim of ciphertext c is generator word (key, stream, c (D + 1) + j): the server
    regenerates it (Session.upload_seeded, Context.expand_seeded).  Wire form: to_bytes / from_bytes."""

    MAGIC, VERSION = b"DSCT", 1
    _HDR = struct.Struct("<4sIQiiQ")          # magic, version, stream, D, input_dim, count; then the key (32 bytes) and count u64 bodies

    def __init__(self, key, stream, D, input_dim, bodies):
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("a mask key is exactly 32 bytes")
        D, input_dim = int(D), int(input_dim)
        if not (1 <= input_dim <= D):
            raise ValueError(f"input_dim {input_dim} outside [1, D = {D}]")
        self.key, self.stream, self.D, self.input_dim = key, int(stream), D, input_dim
        self.bodies = np.ascontiguousarray(bodies, np.uint64).reshape(-1)

    def __len__(self):
        return self.bodies.size

    @property
    def nbytes(self):
        return self._HDR.size + 32 + self.bodies.nbytes

    def to_bytes(self):
        return self._HDR.pack(self.MAGIC, self.VERSION, self.stream, self.D, self.input_dim, self.bodies.size) + self.key + self.bodies.tobytes()

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        H = cls._HDR.size
        if len(blob) < H + 32:
            raise ValueError("seeded-ciphertext blob too short")
        magic, version, stream, D, input_dim, count = cls._HDR.unpack_from(blob)
        if magic != cls.MAGIC or version != cls.VERSION:
            raise ValueError("not a seeded-ciphertext blob (magic / version)")
        if len(blob) != H + 32 + 8 * count:
            raise ValueError(f"seeded-ciphertext blob of {len(blob)} bytes, its header says {H + 32 + 8 * count}")
        return cls(blob[H:H + 32], stream, D, input_dim, np.frombuffer(blob, np.uint64, count, H + 32).copy())


class PackedCiphertexts:
    """Result ciphertexts in PACKED form (include/dctfhe.h dctfhe_session_download_packed): key-switched to a small key of n bits and
    rounded to 16 bits per word, rows [count, n + 1] of uint16.  Wire form: to_bytes / from_bytes (little-endian)."""

    MAGIC, VERSION = b"DPCT", 1
    _HDR = struct.Struct("<4sIiQ")            # magic, version, n, count; then count x (n + 1) u16

    def __init__(self, n, rows):
        n = int(n)
        if n < 1:
            raise ValueError(f"packed ciphertexts need n >= 1 (got {n})")
        rows = np.ascontiguousarray(rows, np.uint16)
        if rows.size % (n + 1):
            raise ValueError(f"{rows.size} words are not rows of n + 1 = {n + 1}")
        self.n, self.rows = n, rows.reshape(-1, n + 1)

    def __len__(self):
        return self.rows.shape[0]

    @property
    def nbytes(self):
        return self._HDR.size + self.rows.nbytes

    def to_bytes(self):
        return self._HDR.pack(self.MAGIC, self.VERSION, self.n, self.rows.shape[0]) + self.rows.astype("<u2", copy=False).tobytes()

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        H = cls._HDR.size
        if len(blob) < H:
            raise ValueError("packed-ciphertext blob too short")
        magic, version, n, count = cls._HDR.unpack_from(blob)
        if magic != cls.MAGIC or version != cls.VERSION:
            raise ValueError("not a packed-ciphertext blob (magic / version)")
        if n < 1 or len(blob) != H + 2 * count * (n + 1):
            raise ValueError(f"packed-ciphertext blob of {len(blob)} bytes, its header says n = {n}, {count} rows")
        return cls(n, np.frombuffer(blob, "<u2", count * (n + 1), H).astype(np.uint16))


class PackedRing:
    """Result ciphertexts in RING-PACKED form (include/dctfhe.h dctfhe_session_download_ring): groups of up to N_p = 2^logN results, each
    group one GLWE ciphertext of 16-bit words -- its N_p mask words, then one body word per result.  words: flat uint16, groups
    contiguous.  Wire form: to_bytes / from_bytes (little-endian)."""

    MAGIC, VERSION = b"DRCT", 1
    _HDR = struct.Struct("<4sIiQ")            # magic, version, logN, count; then groups * N_p + count u16

    def __init__(self, logN, count, words):
        logN, count = int(logN), int(count)
        if not 5 <= logN <= 12:
            raise ValueError(f"ring-packed ciphertexts need 5 <= logN <= 12 (got {logN})")
        if count < 0:
            raise ValueError(f"ring-packed ciphertexts: count {count}")
        words = np.ascontiguousarray(words, np.uint16).reshape(-1)
        if words.size != self.n_words(logN, count):
            raise ValueError(f"{words.size} words are not {count} results in rings of {1 << logN} ({self.n_words(logN, count)} words)")
        self.logN, self.count, self.words = logN, count, words

    @staticmethod
    def n_words(logN, count):
        N = 1 << logN
        return -(-count // N) * N + count

    def __len__(self):
        return self.count

    @property
    def nbytes(self):
        return self._HDR.size + self.words.nbytes

    def to_bytes(self):
        return self._HDR.pack(self.MAGIC, self.VERSION, self.logN, self.count) + self.words.astype("<u2", copy=False).tobytes()

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        H = cls._HDR.size
        if len(blob) < H:
            raise ValueError("ring-packed-ciphertext blob too short")
        magic, version, logN, count = cls._HDR.unpack_from(blob)
        if magic != cls.MAGIC or version != cls.VERSION:
            raise ValueError("not a ring-packed-ciphertext blob (magic / version)")
        if not 5 <= logN <= 12 or len(blob) != H + 2 * cls.n_words(logN, count):
            raise ValueError(f"ring-packed-ciphertext blob of {len(blob)} bytes, its header says logN = {logN}, {count} results")
        return cls(logN, count, np.frombuffer(blob, "<u2", cls.n_words(logN, count), H).astype(np.uint16))


class PublicInputs:
    """Input ciphertexts made with a PUBLIC key (include/dctfhe.h dctfhe_encrypt_public): groups of up to N_e = 2^logN inputs, each group
    one GLWE ciphertext of 64-bit words -- its N_e mask words, then one body word per input.  words: flat uint64, groups contiguous.
    Wire form: to_bytes / from_bytes (little-endian)."""

    MAGIC, VERSION = b"DPIN", 1
    _HDR = struct.Struct("<4sIiQ")            # magic, version, logN, count; then groups * N_e + count u64

    def __init__(self, logN, count, words):
        logN, count = int(logN), int(count)
        if not 5 <= logN <= 12:
            raise ValueError(f"public-key inputs need 5 <= logN <= 12 (got {logN})")
        if count < 0:
            raise ValueError(f"public-key inputs: count {count}")
        words = np.ascontiguousarray(words, np.uint64).reshape(-1)
        if words.size != self.n_words(logN, count):
            raise ValueError(f"{words.size} words are not {count} inputs in rings of {1 << logN} ({self.n_words(logN, count)} words)")
        self.logN, self.count, self.words = logN, count, words

    @staticmethod
    def n_words(logN, count):
        N = 1 << logN
        return -(-count // N) * N + count

    def __len__(self):
        return self.count

    @property
    def nbytes(self):
        return self._HDR.size + self.words.nbytes

    def to_bytes(self):
        return self._HDR.pack(self.MAGIC, self.VERSION, self.logN, self.count) + self.words.astype("<u8", copy=False).tobytes()

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        H = cls._HDR.size
        if len(blob) < H:
            raise ValueError("public-key-input blob too short")
        magic, version, logN, count = cls._HDR.unpack_from(blob)
        if magic != cls.MAGIC or version != cls.VERSION:
            raise ValueError("not a public-key-input blob (magic / version)")
        if not 5 <= logN <= 12 or len(blob) != H + 8 * cls.n_words(logN, count):
            raise ValueError(f"public-key-input blob of {len(blob)} bytes, its header says logN = {logN}, {count} inputs")
        return cls(logN, count, np.frombuffer(blob, "<u8", cls.n_words(logN, count), H).astype(np.uint64))
