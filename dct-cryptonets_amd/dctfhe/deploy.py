"""Deployment bundles: a client, a data owner and a server that each start from a FILE.

    save(q_module, directory)        once, after compilation, without a GPU: client.dctfhe (no weights, no tables) and server.dctfhe
    Client(path)                     keygen / save_key / load_key, the three key exports, encrypt, decrypt, the key check
    DataOwner(path)                  load_public_key, encrypt -- the same client.dctfhe, no secret
    Server(path)                     load_evaluation_keys, load_result_packing_key, evaluate, run_clear, answer_key_check
    python -m dctfhe.deploy ...      one role per invocation, files in and files out

The files are one container each: magic, format version, total length, a JSON header, then arrays in numpy's .npy form read with
allow_pickle=False.  Nothing in a file is imported, evaluated or unpickled.  Requests and responses travel in envelopes (DREQ / DRSP) that
carry the SHA-256 of the circuit blob: a server refuses a request of another circuit and a client a response of another circuit before
anything reaches the GPU.  The key check bootstraps a few known messages per tier before the long run.

The roles run dctfhe.roles, the functions QuantizedModule runs.  Only save() and the `save` command import the compiler; Client and
DataOwner never create a Circuit, Server never holds a ClientKey."""
import dataclasses
import hashlib
import io
import json
import os
import struct
import sys
import types

import numpy as np

from . import params as P
from . import roles
from .params import KeyTierSelection
from ._lib import MAX_TIERS, DctfheError
from .engine import (Circuit, ClientKey, Context, EvalKeys, PackKey, PackedCiphertexts, PackedRing, PublicInputs, PublicKey, SeededCiphertexts,
                     Session, blob_key_tiers, blob_params, key_tiers_for_circuit, seed_bytes)

FILE_MAGIC, FORMAT_VERSION = b"DCTFHEDP", 1
_FILE_HDR = struct.Struct("<8sIIQ")           # magic, format version, JSON header bytes, total file bytes; then the header, then the arrays
CLIENT_FILE, SERVER_FILE = "client.dctfhe", "server.dctfhe"
TIER_FIELDS = tuple(f.name for f in dataclasses.fields(P.TierSpec))
BOUNDARY_KEYS = ("input_shape", "in_scale", "in_bits", "e_in", "n_out", "e_out", "out_scale", "out_bits", "in_dim", "out_dim")
# the client spec's keys: a fixed whitelist (tests/test_deploy_host.py); nothing of the model beyond its boundary
CLIENT_KEYS = ("digest", "boundary", "param_set", "output_compaction", "public_input_plan", "has_classifier", "classifier_w", "classifier_b")
SERVER_KEYS = ("digest", "boundary", "param_set", "output_compaction", "public_input_plan", "blob", "simulation_sigmas", "simulation_sigmas_split")
# fields either file may carry and a default save() does not write.  key_tiers: dict(bsk, ksk), the bit masks of a PRUNED bundle's tier
# selection (include/dctfhe.h TIER SELECTIONS); absent: every tier, which is how files from before the field load
OPTIONAL_KEYS = ("key_tiers",)


# ------------------------------------------------------------------------------------------ container
def _flatten(node, floats, arrays, path):
    """a tree of dict / list / int / str / bool / None / float / ndarray / bytes -> its JSON form: floats move into one float64 array
    (bit for bit), ndarrays and bytes into arrays of their own"""
    if isinstance(node, dict):
        return {str(k): _flatten(v, floats, arrays, f"{path}.{k}" if path else str(k)) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_flatten(v, floats, arrays, f"{path}.{i}") for i, v in enumerate(node)]
    if isinstance(node, (bytes, bytearray)):
        node = np.frombuffer(bytes(node), np.uint8)
    if isinstance(node, np.ndarray):
        if node.dtype.hasobject:
            raise ValueError(f"{path}: object arrays are not stored")
        arrays.append((path, np.ascontiguousarray(node).astype(node.dtype.newbyteorder("<"), copy=False)))
        return {"$array": path}
    if isinstance(node, (bool, str)) or node is None:
        return node
    if isinstance(node, (int, np.integer)):
        return int(node)
    if isinstance(node, (float, np.floating)):
        floats.append(float(node))
        return {"$f64": len(floats) - 1}
    raise ValueError(f"{path}: a {type(node).__name__} is not stored")


def _unflatten(node, floats, arrays):
    if isinstance(node, dict):
        if set(node) == {"$f64"}:
            return float(floats[node["$f64"]])
        if set(node) == {"$array"}:
            return arrays[node["$array"]]
        return {k: _unflatten(v, floats, arrays) for k, v in node.items()}
    if isinstance(node, list):
        return [_unflatten(v, floats, arrays) for v in node]
    return node


def write_container(path, kind, tree):
    floats, arrays = [], []
    body = _flatten(tree, floats, arrays, "")
    arrays.insert(0, ("$f64", np.asarray(floats, "<f8")))
    chunks = []
    for _, a in arrays:
        buf = io.BytesIO()
        np.save(buf, a, allow_pickle=False)
        chunks.append(buf.getvalue())
    header = json.dumps(dict(kind=kind, tree=body, arrays=[dict(name=n, nbytes=len(c)) for (n, _), c in zip(arrays, chunks)]),
                        sort_keys=True).encode()
    total = _FILE_HDR.size + len(header) + sum(len(c) for c in chunks)
    with open(path, "wb") as f:
        f.write(_FILE_HDR.pack(FILE_MAGIC, FORMAT_VERSION, len(header), total))
        f.write(header)
        for c in chunks:
            f.write(c)


def read_container(path, kind):
    """-> the tree write_container stored.  ValueError: wrong magic, unknown version, a truncated file, another kind, or an array that
    could only be read by unpickling"""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < _FILE_HDR.size:
        raise ValueError(f"{path}: truncated file ({len(raw)} bytes, shorter than the fixed header)")
    magic, version, hlen, total = _FILE_HDR.unpack_from(raw)
    if magic != FILE_MAGIC:
        raise ValueError(f"{path}: wrong magic {magic!r} (not a dctfhe deployment file)")
    if version != FORMAT_VERSION:
        raise ValueError(f"{path}: unknown format version {version} (this build reads version {FORMAT_VERSION})")
    if total != len(raw) or _FILE_HDR.size + hlen > len(raw):
        raise ValueError(f"{path}: truncated file ({len(raw)} bytes, its header says {total})")
    try:
        header = json.loads(raw[_FILE_HDR.size:_FILE_HDR.size + hlen].decode())
        entries = [(str(e["name"]), int(e["nbytes"])) for e in header["arrays"]]
        got_kind, body = header["kind"], header["tree"]
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f"{path}: unreadable header ({e})") from None
    if got_kind != kind:
        raise ValueError(f"{path}: a {got_kind!r} file where a {kind!r} file is expected")
    at, arrays = _FILE_HDR.size + hlen, {}
    if at + sum(n for _, n in entries) != len(raw) or any(n < 0 for _, n in entries):
        raise ValueError(f"{path}: truncated file (the arrays do not fill {len(raw)} bytes)")
    for name, n in entries:
        try:
            arrays[name] = np.load(io.BytesIO(raw[at:at + n]), allow_pickle=False)
        except ValueError as e:
            if "pickle" in str(e).lower() or "object arrays" in str(e).lower():
                raise ValueError(f"{path}: array {name!r} needs allow_pickle=True, which this loader refuses ({e})") from None
            raise ValueError(f"{path}: array {name!r} is unreadable ({e})") from None
        except (EOFError, OSError) as e:
            raise ValueError(f"{path}: array {name!r} is unreadable ({e})") from None
        at += n
    return _unflatten(body, arrays.get("$f64", np.zeros(0)), arrays)


# ------------------------------------------------------------------------------------------ records <-> trees
def _params_tree(ps):
    pairs = lambda d: None if d is None else [[int(k), int(v)] for k, v in sorted(d.items())]
    out = {f.name: getattr(ps, f.name) for f in dataclasses.fields(ps) if f.name != "tiers"}
    for k in ("table_tier_for_w", "coarse_tier_for_w", "table_tier_fallback_for_w"):
        out[k] = pairs(out[k])
    # a catalogue with a quiet pool tier says so; one without keeps the tree bundles have always carried
    if out["pool_tier_fallback_for_w"] is None:
        del out["pool_tier_fallback_for_w"]
    else:
        out["pool_tier_fallback_for_w"] = pairs(out["pool_tier_fallback_for_w"])
    out["tiers"] = [{n: getattr(t, n) for n in TIER_FIELDS} for t in ps.tiers]
    return out


def _params_from_tree(t):
    t = dict(t)
    for k in ("table_tier_for_w", "coarse_tier_for_w", "table_tier_fallback_for_w", "pool_tier_fallback_for_w"):
        t[k] = None if t.get(k) is None else {int(a): int(b) for a, b in t[k]}
    t["tiers"] = [P.TierSpec(**tier) for tier in t["tiers"]]
    if len(t["tiers"]) > MAX_TIERS:
        raise ValueError(f"{len(t['tiers'])} tiers (at most {MAX_TIERS})")
    return P.ParamSet(**t)


class Record(types.SimpleNamespace):
    """a priced record as a file carries it: the fields of the compiler's dataclass (OutputCompaction, RingCompaction, PublicInputPlan)"""


def _priced(fn):
    """the record fn() prices as a tree, or {"refused": text} where the compiler refuses it"""
    try:
        return dataclasses.asdict(fn())
    except ValueError as e:
        return {"refused": str(e)}


def _record(tree, spec_cls=None):
    """tree -> Record (spec: the params dataclass again); a refusal raises the compiler's ValueError, as pricing it in place would"""
    if "refused" in tree:
        raise ValueError(tree["refused"])
    d = dict(tree)
    if spec_cls is not None:
        d["spec"] = spec_cls(**d["spec"])
    return Record(**d)


def circuit_digest(blob):
    return hashlib.sha256(bytes(blob)).digest()


def key_check_bits(ps):
    """per tier, the table precision the key check places its messages at: the widest table the catalogue gives the tier, 0 (a sign
    bootstrap) for the one-bit tiers and for a tier without a role"""
    w = [0] * len(ps.tiers)
    for table in (ps.table_tier_for_w, ps.coarse_tier_for_w, ps.table_tier_fallback_for_w, getattr(ps, "pool_tier_fallback_for_w", None)):
        for ww, ti in (table or {}).items():
            w[ti] = max(w[ti], int(ww))
    for ti in (ps.bit_tier, ps.bit_tier_coarse, ps.bit_tier_coarse2):
        if ti is not None:
            w[ti] = 0
    return w


# ------------------------------------------------------------------------------------------ save
def bundle_key_tiers(q_module, key_tiers="all"):
    """the tier selection a bundle records: None for "all"; for "circuit" CompiledCircuit.key_tiers at the output form (and packing spec)
    of the module's Configuration -- None again where that is every tier"""
    if key_tiers not in ("all", "circuit"):
        raise ValueError(f"key_tiers {key_tiers!r} (all or circuit)")
    if key_tiers == "all":
        return None
    cfg, c = q_module.configuration, q_module.compiled
    form = cfg.compress_output_ciphertexts
    sel = c.key_tiers("ring", cfg.result_packing_spec) if form == "ring" else c.key_tiers("rows" if form else None)
    return None if sel.is_all(c.param_set) else sel


def bundle_trees(q_module, classifier=None, key_tiers="all"):
    """(client tree, server tree) of a compiled module; the priced records at the specs its Configuration carries now"""
    c = q_module.compiled
    ps = c.param_set
    tin, tout = c.tensors[c.input_tensor], c.tensors[c.output_tensor]
    digest = circuit_digest(c.blob)
    boundary = dict(input_shape=[tin.C, tin.H, tin.W], in_scale=float(c.in_scale), in_bits=int(c.in_bits), e_in=int(c.e_in), n_out=int(c.n_out()),
                    e_out=int(c.e_out), out_scale=float(c.out_scale), out_bits=int(c.out_bits), in_dim=int(tin.deff or ps.D),
                    out_dim=int(tout.deff or ps.D))
    common = dict(digest=digest, boundary=boundary, param_set=_params_tree(ps),
                  output_compaction=dict(rows=_priced(lambda: q_module.output_compaction("rows")),
                                         ring=_priced(lambda: q_module.output_compaction("ring"))),
                  public_input_plan=_priced(q_module.public_input_plan))
    sel = bundle_key_tiers(q_module, key_tiers)
    if sel is not None:
        common["key_tiers"] = dict(bsk=int(sel.bsk_mask), ksk=int(sel.ksk_mask))
    client = dict(common, has_classifier=classifier is not None)
    if classifier is not None:
        w, b = classifier
        client["classifier_w"], client["classifier_b"] = np.asarray(w, np.float64), np.asarray(b, np.float64)
        if client["classifier_w"].ndim != 2 or client["classifier_w"].shape != (client["classifier_b"].size, c.n_out()):
            raise ValueError(f"classifier of shape {client['classifier_w'].shape} for {c.n_out()} features")
    server = dict(common, blob=np.frombuffer(bytes(c.blob), np.uint8), simulation_sigmas=np.asarray(c.simulation_sigmas(), np.float64),
                  simulation_sigmas_split=np.asarray(c.simulation_sigmas_split(), np.float64))
    return client, server


def save(q_module, directory, classifier=None, key_tiers="all"):
    """Writes client.dctfhe and server.dctfhe for a compiled QuantizedModule into `directory`; needs no GPU.  classifier: (w, b) of the
    clear nn.Linear the client applies to the decrypted features (optional).  key_tiers: "all" (default: the files of before) or
    "circuit": both files record the tier selection the circuit reads, and the client makes and ships only those evaluation keys.
    Returns the two paths."""
    client, server = bundle_trees(q_module, classifier, key_tiers)
    os.makedirs(directory, exist_ok=True)
    paths = os.path.join(directory, CLIENT_FILE), os.path.join(directory, SERVER_FILE)
    write_container(paths[0], "client", client)
    write_container(paths[1], "server", server)
    return paths


class Spec:
    """What a role needs of a circuit, as loaded from a file: the narrow spec object of dctfhe.roles (in_scale, in_bits, e_in, e_out,
    out_scale, n_out()), the ParamSet, the circuit digest and the priced records."""

    def __init__(self, tree, keys, path="<tree>"):
        required = {"digest", "boundary", "param_set", "output_compaction", "public_input_plan"}
        if set(tree) - set(keys) - set(OPTIONAL_KEYS) or not required <= set(tree):
            raise ValueError(f"{path}: unexpected or missing fields {sorted((set(tree) - set(keys) - set(OPTIONAL_KEYS)) | (required - set(tree)))}")
        self.tree = tree
        self.digest = bytes(np.asarray(tree["digest"], np.uint8).tobytes())
        if len(self.digest) != 32:
            raise ValueError(f"{path}: a circuit digest is 32 bytes")
        b = tree["boundary"]
        if set(b) != set(BOUNDARY_KEYS):
            raise ValueError(f"{path}: boundary fields {sorted(b)}")
        self.input_shape = tuple(int(v) for v in b["input_shape"])
        self.in_scale, self.out_scale = float(b["in_scale"]), float(b["out_scale"])
        self.in_bits, self.e_in, self.e_out, self.out_bits = int(b["in_bits"]), int(b["e_in"]), int(b["e_out"]), int(b["out_bits"])
        self._n_out, self.in_dim, self.out_dim = int(b["n_out"]), int(b["in_dim"]), int(b["out_dim"])
        self.param_set = _params_from_tree(tree["param_set"])
        self.classifier = (tree["classifier_w"], tree["classifier_b"]) if tree.get("has_classifier") else None
        # the bundle's tier selection (params.KeyTierSelection); a file without the field selects every tier
        kt = tree.get("key_tiers")
        if kt is not None and (not isinstance(kt, dict) or set(kt) != {"bsk", "ksk"}):
            raise ValueError(f"{path}: key_tiers holds the two masks bsk and ksk")
        self.key_tiers = KeyTierSelection.all(self.param_set) if kt is None else KeyTierSelection.from_masks(self.param_set, int(kt["bsk"]), int(kt["ksk"]))
        self.pruned = kt is not None

    def n_in(self):
        return int(np.prod(self.input_shape))

    def n_out(self):
        return self._n_out

    def dims(self):
        """(input, output) effective dimensions, as Session.dims() reports them for this circuit"""
        return self.in_dim, self.out_dim

    def output_compaction(self, form="rows"):
        if form not in ("rows", "ring"):
            raise ValueError(f"output compaction form {form!r} (rows or ring)")
        return _record(self.tree["output_compaction"][form], P.PackSpec if form == "ring" else None)

    def public_input_plan(self):
        return _record(self.tree["public_input_plan"], P.PublicInputSpec)

    def c_params(self):
        return P.to_c_params(self.param_set)


def load_client_spec(path):
    return Spec(read_container(path, "client"), CLIENT_KEYS, path)


def load_server_bundle(path):
    spec = Spec(read_container(path, "server"), SERVER_KEYS, path)
    spec.blob = spec.tree["blob"].astype(np.uint8).tobytes()
    if circuit_digest(spec.blob) != spec.digest:
        raise ValueError(f"{path}: the circuit blob's SHA-256 {circuit_digest(spec.blob).hex()} is not the digest the file states {spec.digest.hex()}")
    spec.simulation_sigmas = [float(v) for v in spec.tree["simulation_sigmas"]]
    spec.simulation_sigmas_split = [float(v) for v in spec.tree["simulation_sigmas_split"]]
    return spec


# ------------------------------------------------------------------------------------------ envelopes
REQ_MAGIC, RSP_MAGIC, ENVELOPE_VERSION = b"DREQ", b"DRSP", 1
_REQ = struct.Struct("<4sI32sI")              # magic, version, circuit digest, batch; then the payload
_RSP = struct.Struct("<4sI32sII")             # magic, version, circuit digest, batch, form; then the payload
FORM_ROWS, FORM_PACKED, FORM_RING = 0, 1, 2
ROWS_MAGIC = b"DROW"
_ROWS = struct.Struct("<4sIiQ")               # magic, version, dim, count; then count x (dim + 1) u64


def rows_to_bytes(rows, dim):
    rows = np.ascontiguousarray(rows, np.uint64).reshape(-1, int(dim) + 1)
    return _ROWS.pack(ROWS_MAGIC, 1, int(dim), rows.shape[0]) + rows.astype("<u8", copy=False).tobytes()


def rows_from_bytes(blob):
    """-> (rows [count, dim + 1] uint64, dim)"""
    blob = bytes(blob)
    if len(blob) < _ROWS.size:
        raise ValueError("truncated ciphertext rows (shorter than their header)")
    magic, version, dim, count = _ROWS.unpack_from(blob)
    if magic != ROWS_MAGIC or version != 1:
        raise ValueError("not ciphertext rows (magic / version)")
    if dim < 1 or len(blob) != _ROWS.size + 8 * count * (dim + 1):
        raise ValueError(f"truncated ciphertext rows: {len(blob)} bytes, the header says dim = {dim}, {count} rows")
    return np.frombuffer(blob, "<u8", count * (dim + 1), _ROWS.size).astype(np.uint64).reshape(count, dim + 1), dim


def _digest_refusal(what, got, mine, whose):
    return ValueError(f"digest mismatch: the {what} is for circuit {got.hex()}, {whose} for circuit {mine.hex()}")


def pack_request(digest, batch, payload):
    return _REQ.pack(REQ_MAGIC, ENVELOPE_VERSION, digest, int(batch)) + bytes(payload)


def unpack_request(blob, digest):
    """-> (batch, payload bytes); ValueError on a truncated envelope, wrong magic / version, or a digest that is not `digest`"""
    blob = bytes(blob)
    if len(blob) < _REQ.size + 4:
        raise ValueError(f"truncated DREQ envelope ({len(blob)} bytes)")
    magic, version, got, batch = _REQ.unpack_from(blob)
    if magic != REQ_MAGIC:
        raise ValueError(f"wrong magic {magic!r}: not a request envelope (DREQ)")
    if version != ENVELOPE_VERSION:
        raise ValueError(f"unknown DREQ version {version} (this build reads version {ENVELOPE_VERSION})")
    if got != digest:
        raise _digest_refusal("request", got, digest, "this server's bundle is")
    if batch < 1:
        raise ValueError(f"DREQ envelope: batch {batch}")
    return batch, blob[_REQ.size:]


def pack_response(digest, batch, form, payload):
    return _RSP.pack(RSP_MAGIC, ENVELOPE_VERSION, digest, int(batch), int(form)) + bytes(payload)


def unpack_response(blob, digest):
    """-> (batch, form, payload bytes); ValueError as unpack_request"""
    blob = bytes(blob)
    if len(blob) < _RSP.size + 4:
        raise ValueError(f"truncated DRSP envelope ({len(blob)} bytes)")
    magic, version, got, batch, form = _RSP.unpack_from(blob)
    if magic != RSP_MAGIC:
        raise ValueError(f"wrong magic {magic!r}: not a response envelope (DRSP)")
    if version != ENVELOPE_VERSION:
        raise ValueError(f"unknown DRSP version {version} (this build reads version {ENVELOPE_VERSION})")
    if got != digest:
        raise _digest_refusal("response", got, digest, "this client's spec is")
    if batch < 1 or form not in (FORM_ROWS, FORM_PACKED, FORM_RING):
        raise ValueError(f"DRSP envelope: batch {batch}, form {form}")
    return batch, form, blob[_RSP.size:]


# ------------------------------------------------------------------------------------------ key check
KCQ_MAGIC, KCA_MAGIC = b"DKCQ", b"DKCA"
_KC = struct.Struct("<4sI32sI")               # magic, version, circuit digest, entries; then per entry _KCE and its rows
_KCE = struct.Struct("<iiiI")                 # tier, table bits w, mask words per row, rows; then rows x (dim + 1) u64


class KeyCheckError(ValueError):
    pass


def key_check_messages(w):
    """the known messages of a tier whose tables take w bits: the ends and the middle of the range; w = 0: both signs, twice"""
    top = (1 << w) - 1
    return np.array([0, 1, 0, 1] if w == 0 else [0, top, (top + 1) // 2, top // 2], np.uint64)


def key_check_table(w):
    """the identity table of w input bits at two bits of headroom; w = 0: the sign bootstrap's one entry (+-2^57)"""
    return (np.arange(1 << w, dtype=np.int64) << np.int64(63 - w - 2)) if w else np.array([1 << 57], np.int64)


def _pack_key_check(magic, digest, entries):
    out = [_KC.pack(magic, 1, digest, len(entries))]
    for tier, w, rows in entries:
        rows = np.ascontiguousarray(rows, np.uint64)
        out.append(_KCE.pack(int(tier), int(w), rows.shape[1] - 1, rows.shape[0]) + rows.astype("<u8", copy=False).tobytes())
    return b"".join(out)


def _unpack_key_check(magic, blob, digest, whose):
    blob = bytes(blob)
    if len(blob) < _KC.size:
        raise ValueError(f"truncated key-check blob ({len(blob)} bytes)")
    m, version, got, n = _KC.unpack_from(blob)
    if m != magic or version != 1:
        raise ValueError(f"not a key-check blob {magic.decode()} (magic / version)")
    if got != digest:
        raise _digest_refusal("key check", got, digest, whose)
    at, entries = _KC.size, []
    for _ in range(n):
        if len(blob) < at + _KCE.size:
            raise ValueError("truncated key-check blob (an entry's header)")
        tier, w, dim, count = _KCE.unpack_from(blob, at)
        at += _KCE.size
        if dim < 1 or not 0 <= w <= 16 or len(blob) < at + 8 * count * (dim + 1):
            raise ValueError("truncated key-check blob (an entry's rows)")
        entries.append((tier, w, np.frombuffer(blob, "<u8", count * (dim + 1), at).astype(np.uint64).reshape(count, dim + 1)))
        at += 8 * count * (dim + 1)
    if at != len(blob):
        raise ValueError("key-check blob with trailing bytes")
    return entries


# ------------------------------------------------------------------------------------------ roles
HOST = "host"                                  # device="host": the role runs on libdctfhe_client.so, no GPU (dctfhe.host_client)
KEY_MAGIC = b"DKEY"
_KEYFILE = struct.Struct("<4sI32s32s")        # magic, version, circuit digest, the 32-byte key seed


def device_arg(v):
    """a role's device: a GPU index, or the string host (clients and data owners only)"""
    if isinstance(v, str) and v.strip().lower() == HOST:
        return HOST
    try:
        return int(v)
    except (TypeError, ValueError):
        raise ValueError(f"device {v!r}: a GPU index or 'host'") from None


class _Role:
    def __init__(self, spec, device):
        self.spec, self.device, self._ctx = spec, device_arg(device), None

    @property
    def on_host(self):
        return self.device == HOST

    def _context(self):
        if self.on_host:
            raise DctfheError("this role runs on the host: it has no GPU context (this engine has no CPU path for anything that needs one)")
        if self._ctx is None:
            self._ctx = Context(self.device)
        return self._ctx

    def _checked(self, x):
        x = np.asarray(x)
        if x.ndim != 4 or tuple(x.shape[1:]) != self.spec.input_shape:
            raise ValueError(f"inputs of shape {tuple(x.shape)}; this circuit takes [B, {', '.join(map(str, self.spec.input_shape))}]")
        return x

    def quantize(self, x):
        return roles.quantize_input(self.spec, self._checked(x))

    def dequantize(self, q):
        return roles.dequantize_output(self.spec, q)

    def classify(self, features):
        """the clear nn.Linear on dequantised features, where the file carries one"""
        if self.spec.classifier is None:
            raise RuntimeError("this file carries no classifier")
        w, b = self.spec.classifier
        return np.asarray(features, np.float64) @ w.T + b


class Client(_Role):
    """The key owner, started from client.dctfhe: makes the keys, encrypts with the secret key, decrypts results.
    device: a GPU index, or "host" -- the same role on the host library, no GPU (compressed evaluation keys only)."""

    def __init__(self, path, device=0):
        super().__init__(load_client_spec(path), device)
        self._key = None

    def _need_key(self):
        if self._key is None:
            raise RuntimeError("this client has no key yet: keygen() or load_key(path)")
        return self._key

    def keygen(self, seed=None):
        """seed as dctfhe.engine.seed_bytes: None = 32 fresh bytes from the OS, 32 bytes = a persisted seed, int = a deterministic test seed"""
        seed = seed_bytes(seed)
        if self._key is not None:
            self._key.close()
        if self.on_host:
            from .host_client import HostClientKey
            self._key = HostClientKey(self.spec.c_params(), seed)
        else:
            self._key = ClientKey(self._context(), self.spec.c_params(), seed)

    def save_key(self, path):
        """the key file: the 32-byte key seed (key material is a pure function of the parameters and the seed), bound to the circuit
        digest; mode 0600"""
        key = self._need_key()
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
        try:
            os.fchmod(fd, 0o600)
            os.write(fd, _KEYFILE.pack(KEY_MAGIC, 1, self.spec.digest, key.seed))
        finally:
            os.close(fd)

    def load_key(self, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) != _KEYFILE.size:
            raise ValueError(f"{path}: truncated key file ({len(raw)} bytes, a key file has {_KEYFILE.size})")
        magic, version, digest, seed = _KEYFILE.unpack(raw)
        if magic != KEY_MAGIC or version != 1:
            raise ValueError(f"{path}: not a key file (magic / version)")
        if digest != self.spec.digest:
            raise _digest_refusal("key file", digest, self.spec.digest, "this client's spec is")
        self.keygen(seed)

    def export_evaluation_keys(self, compressed=True):
        """the evaluation keys as a blob for the server (no secret inside): compressed (bodies + the public mask key) or full"""
        key = self._need_key()
        tiers = self.spec.key_tiers if self.spec.pruned else None      # a pruned bundle ships only its selection
        if compressed:
            return key.export_eval_keys_compressed(tiers)
        if self.on_host:
            raise ValueError('export_evaluation_keys(compressed=False): the full (Fourier) keys are made on the GPU; a client on device="host" '
                             "ships the compressed form, which the server transforms on import")
        ek = key.generate_eval_keys(tiers)
        try:
            return ek.to_blob()
        finally:
            ek.close()

    def export_public_key(self):
        return self._need_key().export_public_key(self.spec.public_input_plan().spec)

    def export_result_packing_key(self):
        return self._need_key().export_pack_key(self.spec.output_compaction("ring").spec)

    def encrypt(self, x, form="seeded"):
        """float inputs [B, C, H, W] -> a request envelope: seeded (bodies + the public mask key) or compact rows"""
        if form not in ("seeded", "rows"):
            raise ValueError(f"input form {form!r} (seeded or rows)")
        key = self._need_key()
        q = self.quantize(x)
        phases = roles.encode_input(self.spec, q).reshape(-1)
        payload = key.encrypt_seeded(phases).to_bytes() if form == "seeded" else rows_to_bytes(key.encrypt(phases, self.spec.in_dim), self.spec.in_dim)
        return pack_request(self.spec.digest, q.shape[0], payload)

    def decrypt(self, response):
        """a response envelope -> the decoded integers [B, F]; dequantize() gives the floats"""
        batch, form, payload = unpack_response(response, self.spec.digest)
        if form == FORM_ROWS:
            x, _ = rows_from_bytes(payload)
        else:
            x = PackedRing.from_bytes(payload) if form == FORM_RING else PackedCiphertexts.from_bytes(payload)
        if len(x) != batch * self.spec.n_out():
            raise ValueError(f"a response of {len(x)} results for batch {batch} x {self.spec.n_out()} outputs")
        return roles.decrypt_result(self.spec, self._need_key(), x)

    # -- key check ---------------------------------------------------------------------------
    def make_key_check(self):
        """per tier a few fresh encryptions of known messages at the tier's table precision (compact rows), for Server.answer_key_check"""
        key, dim = self._need_key(), self.spec.in_dim
        entries = [(ti, w, key.encrypt(key_check_messages(w) << np.uint64(63 - w), dim)) for ti, w in self._key_check_tiers()]
        return _pack_key_check(KCQ_MAGIC, self.spec.digest, entries)

    def _key_check_tiers(self):
        """(tier, table bits) of the key check: the tiers whose bootstrap key the bundle's selection holds (a closed selection holds their
        key-switch keys too)"""
        return [(ti, w) for ti, w in enumerate(key_check_bits(self.spec.param_set)) if (self.spec.key_tiers.bsk_mask >> ti) & 1]

    def verify_key_check(self, answer):
        """decrypts what the server bootstrapped and compares with the identity table's entries; KeyCheckError names the first tier that
        differs.  Proves that the server's keys bootstrap correctly under this client's secret; says nothing about security."""
        key, ps = self._need_key(), self.spec.param_set
        entries = _unpack_key_check(KCA_MAGIC, answer, self.spec.digest, "this client's spec is")
        asked = self._key_check_tiers()
        if [(t, w) for t, w, _ in entries] != asked:
            raise KeyCheckError(f"key check: the answer covers tiers {[(t, w) for t, w, _ in entries]}, this client asked for {asked}")
        for ti, w, rows in entries:
            msgs = key_check_messages(w)
            if rows.shape != (msgs.size, ps.D + 1):
                raise KeyCheckError(f"key check failed on tier {ti} ({ps.tiers[ti].name}): rows of shape {rows.shape}")
            table = key_check_table(w)
            want = (table[msgs.astype(np.int64)] if w else np.where(msgs == 0, table[0], -table[0])).astype(np.uint64)
            err = np.abs((key.decrypt(rows) - want).astype(np.int64).astype(np.float64)) / 2.0 ** 64
            tol = 2.0 ** -(max(w, 5) + 4)          # half the spacing of the table's entries, and no wider than 2^-9
            if not (err < tol).all():
                raise KeyCheckError(f"key check failed on tier {ti} ({ps.tiers[ti].name}): {int((err >= tol).sum())} of {msgs.size} bootstraps of a "
                                    f"{w}-bit identity miss their entry (largest error 2^{np.log2(max(err.max(), 2.0 ** -64)):.1f} of the torus, "
                                    f"allowed 2^{np.log2(tol):.0f}); these evaluation keys are not this client's")

    def close(self):
        if self._key is not None:
            self._key.close()
            self._key = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


class DataOwner(_Role):
    """A party with inputs and no secret, started from the same client.dctfhe: encrypts with the client's public key.
    device: a GPU index, or "host" -- the same role on the host library, no GPU."""

    def __init__(self, path, device=0):
        super().__init__(load_client_spec(path), device)
        self._public_key = None

    def load_public_key(self, blob):
        plan = self.spec.public_input_plan()
        if self.on_host:
            from .host_client import HostPublicKey
            pk = HostPublicKey(blob)
        else:
            pk = PublicKey(self._context(), blob)
        try:
            roles.check_public_key(plan, pk)
        except RuntimeError:
            pk.close()
            raise
        if self._public_key is not None:
            self._public_key.close()
        self._public_key = pk

    def encrypt(self, x):
        """float inputs [B, C, H, W] -> a request envelope of public-key inputs"""
        if self._public_key is None:
            raise RuntimeError("encrypt needs the client's public key: load_public_key(blob)")
        x = self._checked(x)
        return pack_request(self.spec.digest, x.shape[0], roles.encrypt_public(self.spec, self._public_key, x).to_bytes())

    def close(self):
        if self._public_key is not None:
            self._public_key.close()
            self._public_key = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


class Server(_Role):
    """The evaluator, started from server.dctfhe: holds the circuit and evaluation keys, never a secret."""

    def __init__(self, path, device=0):
        if device_arg(device) == HOST:
            raise DctfheError('Server(device="host"): circuits are evaluated on the GPU -- this engine has no CPU path for the server')
        super().__init__(load_server_bundle(path), device)
        self._circuit, self._keys, self._pack_key, self._sessions = None, None, None, {}
        self.sim_seed = 977

    def _circ(self):
        if self._circuit is None:
            self._circuit = Circuit(self._context(), self.spec.blob)
        return self._circuit

    def _drop_sessions(self, mode):
        for k in [k for k in self._sessions if k[0] == mode]:
            self._sessions.pop(k).close()

    def _session(self, mode, batch):
        if (mode, batch) not in self._sessions:
            if mode == "execute" and self._keys is None:
                raise RuntimeError("evaluate needs the client's evaluation keys: load_evaluation_keys(blob)")
            sess = Session(self._context(), self._circ(), self._keys if mode == "execute" else None, batch)
            if mode == "execute" and sess.dims() != self.spec.dims():
                got = sess.dims()
                sess.close()
                raise RuntimeError(f"the bundle states effective dimensions {self.spec.dims()}, the engine finds {got}")
            self._sessions[(mode, batch)] = sess
        return self._sessions[(mode, batch)]

    def load_evaluation_keys(self, blob):
        """either blob form, full or compressed.  ValueError where the blob's parameters are not the bundle's ParamSet; the library's own
        length check refuses a truncated blob"""
        got, want = blob_params(blob), self.spec.c_params()
        fields = lambda p: (p.D, p.n_max, p.n_tiers, p.input_dim, p.input_sigma) + tuple(
            tuple(getattr(p.tiers[i], f) for f, _ in p.tiers[i]._fields_ if f != "reserved") for i in range(max(0, min(p.n_tiers, MAX_TIERS))))
        if fields(got) != fields(want):
            raise ValueError("these evaluation keys were made for another ParamSet than this bundle's (D, tiers or noise differ): "
                             "client.dctfhe and server.dctfhe are not of one save()")
        # coverage before anything is imported: what the circuit itself reads (a full bundle refuses pruned keys only where a tier is
        # really missing); the key that packs results is checked when a packed form is asked for (evaluate)
        need = key_tiers_for_circuit(self.spec.blob, want)
        held = KeyTierSelection.from_masks(self.spec.param_set, *blob_key_tiers(blob))
        need = KeyTierSelection.from_masks(self.spec.param_set, need.bsk, need.ksk)
        if not held.covers(need):
            raise ValueError(f"these evaluation keys do not cover this bundle's circuit: they lack the {held.missing(need)}")
        keys = EvalKeys.from_blob(self._context(), blob)
        self._drop_sessions("execute")
        if self._keys is not None:
            self._keys.close()
        self._keys = keys

    def load_result_packing_key(self, blob):
        pk = PackKey(self._context(), blob)
        if self._pack_key is not None:
            self._pack_key.close()
        self._pack_key = pk

    def evaluate(self, request, packed=None):
        """a request envelope -> a response envelope.  packed: None / False / "none": compact rows; True / "rows": 16-bit rows; "ring":
        ring-packed (needs load_result_packing_key).  Envelope, digest, payload and the priced records are checked before anything is
        uploaded"""
        batch, payload = unpack_request(request, self.spec.digest)
        magic = payload[:4]
        if magic == ROWS_MAGIC:
            cts, dim = rows_from_bytes(payload)
            if dim != self.spec.in_dim:
                raise ValueError(f"input rows of {dim} mask words; this circuit's inputs keep {self.spec.in_dim}")
        elif magic in (SeededCiphertexts.MAGIC, PublicInputs.MAGIC):
            cts, dim = roles.parse_inputs(payload), self.spec.in_dim
        else:
            raise ValueError(f"a request payload of unknown magic {magic!r}")
        if len(cts) != batch * self.spec.n_in():
            raise ValueError(f"a request of {len(cts)} ciphertexts for batch {batch} x {self.spec.n_in()} inputs")
        if isinstance(cts, PublicInputs):
            self.spec.public_input_plan()          # refuses before anything runs
        packed = roles.output_form(False if packed is None else packed)
        tier, pack_key = None, None
        if packed == "ring":
            tier, pack_key = roles.ring_plan(self.spec.output_compaction("ring"), self._pack_key)
        elif packed:
            tier = self.spec.output_compaction("rows").tier
        if tier is not None and self._keys is not None and not (self._keys.tiers.ksk >> tier) & 1:
            raise ValueError(f"packed={packed!r}: results are packed with the key-switch key of tier {tier} ({self.spec.param_set.tiers[tier].name}), "
                             "which these evaluation keys do not hold (a bundle saved with key_tiers=\"circuit\" covers the output form of "
                             "the module's Configuration)")
        out = roles.evaluate_encrypted(self._session("execute", batch), self._keys, cts, dim, packed, tier, pack_key)
        if packed == "ring":
            return pack_response(self.spec.digest, batch, FORM_RING, out.to_bytes())
        if packed:
            return pack_response(self.spec.digest, batch, FORM_PACKED, out.to_bytes())
        return pack_response(self.spec.digest, batch, FORM_ROWS, rows_to_bytes(out, out.shape[1] - 1))

    def run_clear(self, q, simulate=False):
        """the integer circuit on quantised inputs q [B, C, H, W] in the clear: noise-free, or with the compiler's noise model sampled at
        every look-up (simulate) -> decoded integers [B, F]"""
        q = np.asarray(q)
        sess = self._session("clear", q.shape[0])
        if simulate:
            sess.set_noise(self.sim_seed, self.spec.simulation_sigmas)
            sess.set_noise_split(self.spec.simulation_sigmas_split)
            self.sim_seed += 1
        else:
            sess.set_noise(0, None)
        sess.upload(roles.encode_input(self.spec, q))
        sess.run()
        return roles.decode_output(self.spec, sess.download().reshape(q.shape[0], -1))

    def answer_key_check(self, blob):
        """key switch -> centred mod switch -> bootstrap with the identity table on every ciphertext of Client.make_key_check"""
        if self._keys is None:
            raise RuntimeError("the key check needs the client's evaluation keys: load_evaluation_keys(blob)")
        keys, D = self._keys, self._keys.D
        entries = _unpack_key_check(KCQ_MAGIC, blob, self.spec.digest, "this server's bundle is")
        out = []
        held = keys.tiers
        for tier, w, rows in entries:
            dim = rows.shape[1] - 1
            if 0 <= tier < keys.params.n_tiers and not (held.bsk >> tier) & 1:
                raise ValueError(f"key check: these evaluation keys hold no bootstrap key of tier {tier} ({self.spec.param_set.tiers[tier].name})")
            if not 0 <= tier < keys.params.n_tiers or dim > D or w >= keys.tier(tier).logN:
                raise ValueError(f"key check: tier {tier}, {w} table bits, rows of {dim} mask words do not fit these keys")
            full = np.zeros((rows.shape[0], D + 1), np.uint64)
            full[:, :dim], full[:, D] = rows[:, :dim], rows[:, dim]
            small = keys.modswitch_center(tier, keys.keyswitch(tier, full, 0, dim))
            out.append((tier, w, keys.pbs(tier, small, key_check_table(w), w)))
        return _pack_key_check(KCA_MAGIC, self.spec.digest, out)

    def close(self):
        for s in self._sessions.values():
            s.close()
        self._sessions = {}
        for name in ("_keys", "_pack_key", "_circuit", "_ctx"):
            h = getattr(self, name)
            if h is not None:
                h.close()
                setattr(self, name, None)


# ------------------------------------------------------------------------------------------ command line
def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _write(path, blob):
    with open(path, "wb") as f:
        f.write(blob.tobytes() if isinstance(blob, np.ndarray) else bytes(blob))


def _cmd_save(a):
    # the only command that needs the compiler (and torch); it needs no GPU
    import torch  # noqa: F401
    from . import frontend, models, synthetic
    from .quantized_module import Configuration, compile_brevitas_qat_model, compile_torch_model
    kw = {}
    if a.model == "tiny":
        model = models.tiny_resnet_q()
        calib = np.random.default_rng(a.seed + 100).normal(0, 1, (a.calib_batch_size, model.in_channels, model.img_size, model.img_size))
        compile_fn = compile_brevitas_qat_model
    else:
        if a.dct_status:
            tf, in_ch, img = frontend.dct_eval_transform(a.filter_size, a.image_size_dct, a.channels, a.dct_pattern), a.channels, a.image_size_dct
        else:
            tf, in_ch, img = frontend.rgb_eval_transform(a.image_size), 3, a.image_size
        name = a.model if a.model.endswith("qat") else a.model + "qat"
        model = models.model_dict[name](bit_width=a.bit_width, in_channels=in_ch, img_size=img, num_classes=a.num_classes)
        if a.checkpoint_path and os.path.isfile(a.checkpoint_path):
            from . import checkpoint
            checkpoint.load_checkpoint(a.checkpoint_path, model)
        else:
            print("WARNING: No checkpoint loaded. Using random weights (for testing only)")
        calib = np.stack([tf(im) for im in synthetic.synthetic_images(a.calib_batch_size, a.seed + 100)]).astype(np.float32)
        compile_fn = compile_brevitas_qat_model if "qat" in a.model.lower() else compile_torch_model
    if a.test_params:
        kw["param_set"] = P.test_params()
        cfg = Configuration(result_packing_spec=P.test_pack_spec(), public_input_spec=P.test_public_input_spec())
    else:
        cfg = Configuration()
    rtb = a.rounding_threshold_bits if a.rounding_method == "exact" else {"n_bits": a.rounding_threshold_bits, "method": "approximate"}
    qm = compile_fn(model, calib, rounding_threshold_bits=rtb, n_bits=a.n_bits, p_error=a.p_error, configuration=cfg, tier_policy=a.tier_policy,
                    pool_policy=a.pool_policy, **kw)
    cls = None if model.classifier_w is None else (model.classifier_w, model.classifier_b)
    for p in save(qm, a.out, classifier=cls, key_tiers=a.key_tiers):
        print(f"wrote {p} ({os.path.getsize(p)} bytes)")


def _cmd_keygen(a):
    c = Client(a.client, a.device)
    try:
        c.keygen(a.seed)
        c.save_key(a.key)
        if a.eval_keys:
            _write(a.eval_keys, c.export_evaluation_keys(compressed=not a.full_keys))
        if a.public_key:
            _write(a.public_key, c.export_public_key())
        if a.packing_key:
            _write(a.packing_key, c.export_result_packing_key())
    finally:
        c.close()


def _cmd_encrypt(a):
    c = Client(a.client, a.device)
    try:
        c.load_key(a.key)
        _write(a.out, c.encrypt(np.load(a.input, allow_pickle=False), form=a.form))
    finally:
        c.close()


def _cmd_owner_encrypt(a):
    o = DataOwner(a.client, a.device)
    try:
        o.load_public_key(_read(a.public_key))
        _write(a.out, o.encrypt(np.load(a.input, allow_pickle=False)))
    finally:
        o.close()


def _server(a):
    s = Server(a.server, a.device)
    try:
        s.load_evaluation_keys(_read(a.eval_keys))
    except BaseException:
        s.close()
        raise
    return s


def _cmd_evaluate(a):
    s = _server(a)
    try:
        if a.packing_key:
            s.load_result_packing_key(_read(a.packing_key))
        _write(a.out, s.evaluate(_read(a.request), packed=a.packed))
    finally:
        s.close()


def _cmd_decrypt(a):
    c = Client(a.client, a.device)
    try:
        c.load_key(a.key)
        q = c.decrypt(_read(a.response))
        with open(a.out, "wb") as f:
            np.save(f, q, allow_pickle=False)
        if a.logits:
            with open(a.logits, "wb") as f:
                np.save(f, c.classify(c.dequantize(q)), allow_pickle=False)
    finally:
        c.close()


def _cmd_key_check(a):
    need = dict(make=("client", "key", "out"), answer=("server", "eval_keys", "input", "out"), verify=("client", "key", "input"))[a.step]
    missing = [n for n in need if getattr(a, n) is None]
    if missing:
        raise SystemExit(f"key-check {a.step} needs " + ", ".join("--" + n.replace("_", "-") for n in missing))
    if a.step == "answer":
        s = _server(a)
        try:
            _write(a.out, s.answer_key_check(_read(a.input)))
        finally:
            s.close()
        return
    c = Client(a.client, a.device)
    try:
        c.load_key(a.key)
        if a.step == "make":
            _write(a.out, c.make_key_check())
        else:
            c.verify_key_check(_read(a.input))
            print("key check passed: every tier bootstraps its identity table under this client's key")
    finally:
        c.close()


def _parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dctfhe.deploy", description="dctfhe deployment bundles: one role per invocation, files in and out")
    sub = ap.add_subparsers(dest="command", required=True)

    def cmd(name, fn, help_):
        p = sub.add_parser(name, help=help_)
        p.set_defaults(fn=fn)
        p.add_argument("--device", default=0, type=device_arg,
                       help="GPU index; 'host' runs the client and owner sub-commands (keygen, encrypt, owner-encrypt, decrypt, key-check make / verify) "
                            "without a GPU")
        return p
    p = cmd("save", _cmd_save, "compile a model and write client.dctfhe and server.dctfhe (no GPU)")
    p.add_argument("--out", required=True, help="directory for the two files")
    p.add_argument("--model", default="ResNet18qat", choices=["ResNet20", "ResNet20qat", "ResNet18", "ResNet18qat", "tiny"])
    p.add_argument("--num_classes", default=10, type=int)
    p.add_argument("--dct_status", action="store_true")
    p.add_argument("--channels", default=64, type=int, choices=[3, 6, 24, 48, 64, 192])
    p.add_argument("--filter_size", default=8, type=int)
    p.add_argument("--image_size", default=32, type=int)
    p.add_argument("--image_size_dct", default=56, type=int)
    p.add_argument("--dct_pattern", default="default", choices=["default", "square", "triangle", "learned"])
    p.add_argument("--bit_width", default=4, type=int)
    p.add_argument("--checkpoint_path", type=str)
    p.add_argument("--calib_batch_size", default=64, type=int)
    p.add_argument("--rounding_threshold_bits", default=6, type=int)
    p.add_argument("--n_bits", default=5, type=int)
    p.add_argument("--p_error", default=0.01, type=float)
    p.add_argument("--rounding_method", default="exact", choices=["exact", "approximate"])
    p.add_argument("--tier_policy", default="exact", choices=["exact", "p_error"])
    p.add_argument("--pool_policy", default="coarse", choices=["coarse", "exact"])
    p.add_argument("--key_tiers", default="all", choices=["all", "circuit"],
                   help="circuit: the bundle records the tiers the circuit reads, and the client makes and ships only their evaluation keys")
    p.add_argument("--seed", default=42, type=int, help="seed of the synthetic calibration images")
    p.add_argument("--test_params", action="store_true", help="the tiny, INSECURE test catalogue (trying the flow only)")
    p = cmd("keygen", _cmd_keygen, "client: make a key, write the key file and the exports")
    p.add_argument("--client", required=True)
    p.add_argument("--key", required=True, help="key file to write (mode 0600)")
    p.add_argument("--seed", default=None, type=int, help="deterministic TEST seed; default: 32 fresh bytes from the OS")
    p.add_argument("--eval-keys", help="write the evaluation keys here")
    p.add_argument("--full-keys", action="store_true", help="the full evaluation-key blob instead of the compressed one")
    p.add_argument("--public-key", help="write the public key of public-key inputs here")
    p.add_argument("--packing-key", help="write the result packing key here")
    p = cmd("encrypt", _cmd_encrypt, "client: float inputs (.npy, [B, C, H, W]) -> a request")
    p.add_argument("--client", required=True)
    p.add_argument("--key", required=True)
    p.add_argument("--input", required=True)
    p.add_argument("--form", default="seeded", choices=["seeded", "rows"])
    p.add_argument("--out", required=True)
    p = cmd("owner-encrypt", _cmd_owner_encrypt, "data owner: float inputs (.npy) -> a request, with the public key only")
    p.add_argument("--client", required=True)
    p.add_argument("--public-key", required=True)
    p.add_argument("--input", required=True)
    p.add_argument("--out", required=True)
    p = cmd("evaluate", _cmd_evaluate, "server: a request -> a response")
    p.add_argument("--server", required=True)
    p.add_argument("--eval-keys", required=True)
    p.add_argument("--packing-key")
    p.add_argument("--request", required=True)
    p.add_argument("--packed", default="none", choices=["none", "rows", "ring"])
    p.add_argument("--out", required=True)
    p = cmd("decrypt", _cmd_decrypt, "client: a response -> the decoded integers (.npy, [B, F])")
    p.add_argument("--client", required=True)
    p.add_argument("--key", required=True)
    p.add_argument("--response", required=True)
    p.add_argument("--out", required=True)
    p.add_argument("--logits", help="also write the clear classifier's logits here (a file with a classifier)")
    p = cmd("key-check", _cmd_key_check, "make (client), answer (server), verify (client): a few bootstraps per tier before the long run")
    p.add_argument("step", choices=["make", "answer", "verify"])
    p.add_argument("--client")
    p.add_argument("--key")
    p.add_argument("--server")
    p.add_argument("--eval-keys")
    p.add_argument("--input", help="answer: the client's check; verify: the server's answer")
    p.add_argument("--out")
    return ap


def main(argv=None):
    a = _parser().parse_args(argv)
    a.fn(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
