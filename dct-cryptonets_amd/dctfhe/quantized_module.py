"""The operator surface the reference drives, re-hosted on the HIP engine.

    reference call site                                         here
    compile_brevitas_qat_model(...)  homomorphic_eval.py:276    compile_brevitas_qat_model -> QuantizedModule
    compile_torch_model(...)         homomorphic_eval.py:287    compile_torch_model (same circuit builder)
    Configuration(...)               homomorphic_eval.py:266    Configuration (progress flags kept, inert; compress_input_ciphertexts,
                                                                compress_evaluation_keys: seeded inputs / compressed evaluation keys;
                                                                compress_output_ciphertexts: packed 16-bit results, as rows
                                                                or, with "ring", up to N_p of them in one GLWE ciphertext;
                                                                public_key_inputs: inputs encrypted with a public key)
    q.fhe_circuit.graph.maximum_integer_bit_width()    :301     FHECircuit.graph.maximum_integer_bit_width()
    q.fhe_circuit.mlir                                 :311     FHECircuit.mlir  (text dump of the compiled circuit)
    q.fhe_circuit.keygen()                             :315     FHECircuit.keygen()  (keys generated on the GPU)
    q.forward(x, fhe="simulate"|"execute")             :70      QuantizedModule.forward

fhe="execute": quantise -> encrypt -> circuit on ciphertexts -> decrypt -> dequantise, all ciphertext work in
libdctfhe.so.  fhe="simulate" / "disable": the same integer circuit on plaintext phases (1-word
"ciphertexts"), also on the GPU through the same scheduler -- the noise-free circuit.  There is no CPU path.
"""
import math
import time

import numpy as np

from . import compile as cc
from . import params as P
from . import roles
from .engine import Circuit, Context, Keys, PackKey, PublicInputs, PublicKey, SeededCiphertexts, Session


class Configuration:
    """Stand-in for concrete.fhe.Configuration (reference homomorphic_eval.py:266-273)."""

    def __init__(self, show_progress=False, progress_tag=False, progress_title="", compress_input_ciphertexts=False,
                 compress_evaluation_keys=False, compress_output_ciphertexts=False, result_packing_spec=None, public_key_inputs=False,
                 public_input_spec=None, shard_image=False, shard_pool=False, device_memory_budget_gb=None, evaluation_key_tiers="all", **kwargs):
        self.show_progress, self.progress_tag, self.progress_title = show_progress, progress_tag, progress_title
        # Concrete's switches: fhe="execute" ships seeded inputs (bodies + a public mask key; include/dctfhe.h dctfhe_encrypt_seeded),
        # export_evaluation_keys() the compressed blob (dctfhe_eval_keys_export_compressed).  Both off by default.
        self.compress_input_ciphertexts = bool(compress_input_ciphertexts)
        self.compress_evaluation_keys = bool(compress_evaluation_keys)
        # dctfhe addition (like tier_policy): results come back key-switched to a small key and rounded to 16 bits per word
        # (include/dctfhe.h dctfhe_session_download_packed; the tier is dctfhe.compile.output_compaction's).  Off by default.
        # "ring": up to N_p results in one GLWE ciphertext instead (dctfhe_session_download_ring), with the packing key the client exports
        # (FHECircuit.export_result_packing_key) and the server loads; result_packing_spec: its params.PackSpec (None: the default one).
        # True (or "rows") keeps meaning the rows form; "none" is False; any other string raises ValueError (it used to count as True).
        self.compress_output_ciphertexts = _output_form(compress_output_ciphertexts)
        self.result_packing_spec = result_packing_spec
        # dctfhe addition: fhe="execute" encrypts its inputs WITHOUT the secret key, through a public key the client exports once
        # (include/dctfhe.h dctfhe_encrypt_public; FHECircuit.export_public_key / load_public_key / encrypt_public split the parties);
        # public_input_spec: its params.PublicInputSpec (None: the default one).  Off by default.  The seeded form is made with the
        # secret key, so the two switches exclude each other.
        self.public_key_inputs = bool(public_key_inputs)
        self.public_input_spec = public_input_spec
        if self.public_key_inputs and self.compress_input_ciphertexts:
            raise ValueError("public_key_inputs and compress_input_ciphertexts exclude each other: a seeded input is made with the secret key")
        # dctfhe addition: under an initialised torch.distributed group of more than one rank, fhe="execute" spreads every image over the
        # ranks' GPUs -- each evaluates its rows of the look-up sites, rows are exchanged where a convolution, a pool or the download
        # reads a whole tensor (include/dctfhe.h dctfhe_session_set_shard).  Every rank calls forward with the same
        # x and holds the same keys (keygen(seed=...) or load_evaluation_keys).  Off by default; one rank, or no group: the plain path.
        self.shard_image = bool(shard_image)
        # ... and with shard_pool the max pools are divided too: a rank computes its own pool outputs and receives only the rows of the
        # pool's source under its windows (dctfhe_session_set_shard_pool).  It refines shard_image and needs it.
        self.shard_pool = bool(shard_pool)
        if self.shard_pool and not self.shard_image:
            raise ValueError("shard_pool divides the max pools of a sharded image: it needs shard_image=True")
        # dctfhe addition: every session the module creates plans its buffers under this many GB (10^9 bytes) of device memory: a
        # convolution and the look-ups / max pools behind it run in channel slabs, and no output word changes (DESIGN.md section 4.2;
        # include/dctfhe.h dctfhe_session_set_memory_budget).  None: no budget.  A budgeted session stays unsharded.
        self.device_memory_budget_gb = None if device_memory_budget_gb is None else float(device_memory_budget_gb)
        if self.device_memory_budget_gb is not None and self.device_memory_budget_gb <= 0:
            raise ValueError("device_memory_budget_gb must be positive (None: no budget)")
        if self.device_memory_budget_gb is not None and self.shard_image:
            raise ValueError("device_memory_budget_gb and shard_image exclude each other: a budgeted session stays unsharded")
        # dctfhe addition: "circuit" makes, exports and loads only the evaluation keys the compiled circuit reads (include/dctfhe.h TIER
        # SELECTIONS; CompiledCircuit.key_tiers), plus the key-switch key that packs the results in the form compress_output_ciphertexts
        # names.  "all" (default): every tier of the catalogue, the keys and blobs of before.  No output word depends on the choice.
        if evaluation_key_tiers not in ("all", "circuit"):
            raise ValueError(f"evaluation_key_tiers {evaluation_key_tiers!r} (all or circuit)")
        self.evaluation_key_tiers = evaluation_key_tiers
        self.extra = kwargs

    @property
    def device_memory_budget_bytes(self):
        return None if self.device_memory_budget_gb is None else int(self.device_memory_budget_gb * 1e9)


_output_form = roles.output_form


class MarginReport:
    """What a margin audit measured (QuantizedModule.audit), slot by slot beside the compiler's model (CompiledCircuit.margin_model).
    rows: one dict per slot -- op, entry, kind, tier, tier_name, table_bits, note, the slot's count, sum, sum_sq, half_box and max_abs
    (levels of the tier's 2N), mean (levels), sigma_measured = sqrt(sum_sq / count) / 2N and sigma_model (fractions of the torus), ratio = measured / model,
    max_over_half_box = max_abs / half_box, z = the half-box in measured sigmas, hist (16 bins of 16 |e| / half_box).
    It validates the variance model at every decision of this run; it does not observe a 1e-13 tail."""

    def __init__(self, rows):
        self.rows = rows

    @classmethod
    def from_slots(cls, slots, model, params):
        if [(m["op"], m["entry"], m["tier"], m["table_bits"]) for m in model] != [(s["op"], s["entry"], s["tier"], s["table_bits"]) for s in slots]:
            raise RuntimeError("margin audit: the engine's slots are not the compiler's margin_model()")
        rows = []
        for s, m in zip(slots, model):
            two_n = 2.0 * (1 << params.tiers[s["tier"]].logN)
            cnt = s["count"]
            sig = math.sqrt(s["sum_sq"] / cnt) / two_n if cnt else float("nan")
            rows.append(dict(op=s["op"], entry=s["entry"], kind=m["kind"], tier=s["tier"], tier_name=m["tier_name"], table_bits=s["table_bits"],
                             note=m["note"], count=cnt, half_box=s["half_box"], max_abs=s["max_abs"], sum=s["sum"], sum_sq=s["sum_sq"], mean=(s["sum"] / cnt if cnt else float("nan")),
                             sigma_measured=sig, sigma_model=m["sigma"], ratio=sig / m["sigma"] if cnt else float("nan"),
                             max_over_half_box=s["max_abs"] / s["half_box"],
                             z=(s["half_box"] / two_n / sig) if (cnt and sig > 0) else float("inf"), hist=list(s["hist"])))
        return cls(rows)

    def worst(self):
        """the slot whose half-box is the fewest measured sigmas wide (None for a circuit without look-ups)"""
        probed = [r for r in self.rows if r["count"]]
        return min(probed, key=lambda r: r["z"]) if probed else None

    def text(self):
        lines = ["// margin audit: sigma at the point of decision, measured against the compiler's model (fractions of the torus, log2)"]
        for r in self.rows:
            lg = lambda v: f"{math.log2(v):7.2f}" if (v == v and v > 0) else "    n/a"
            lines.append(f"op {r['op']:3d}.{r['entry']} {r['kind']:<7} tier={r['tier_name']:<5} bits={r['table_bits']} count={r['count']:8d} "
                         f"measured=2^{lg(r['sigma_measured'])} model=2^{lg(r['sigma_model'])} ratio={r['ratio']:.2f} "
                         f"max|e|/half_box={r['max_over_half_box']:.3f} z={r['z']:.1f}  // {r['note']}")
        w = self.worst()
        if w is not None:
            lines.append(f"// narrowest decision: op {w['op']}.{w['entry']} ({w['kind']}, {w['note']}): half-box = {w['z']:.1f} measured sigma, "
                         f"largest ratio measured / model {max(r['ratio'] for r in self.rows if r['count']):.2f}")
        return "\n".join(lines)


class _Graph:
    def __init__(self, circ):
        self._c = circ

    def maximum_integer_bit_width(self):
        return self._c.max_bit_width


class FHECircuit:
    def __init__(self, owner):
        self._o = owner
        self.graph = _Graph(owner.compiled)

    @property
    def mlir(self):
        return self._o.compiled.report()

    def keygen(self, seed=None, force=False):
        """reference homomorphic_eval.py:315.  seed: None = 32 fresh bytes from the OS (the default); 32 bytes = a persisted /
        broadcast key seed; int = deterministic test seed (dctfhe.engine.seed_bytes)."""
        self._o._keygen(seed, force)

    # -- client / server split: the owner's methods (QuantizedModule) -----------------------------------------------
    def export_evaluation_keys(self, compressed=None):
        return self._o.export_evaluation_keys(compressed)

    def load_evaluation_keys(self, blob):
        return self._o.load_evaluation_keys(blob)

    def evaluate_encrypted(self, cts, batch, dim=None, packed=None):
        return self._o.evaluate_encrypted(cts, batch, dim, packed)

    def export_result_packing_key(self):
        return self._o.export_result_packing_key()

    def load_result_packing_key(self, blob):
        return self._o.load_result_packing_key(blob)

    def export_public_key(self):
        return self._o.export_public_key()

    def load_public_key(self, blob):
        return self._o.load_public_key(blob)

    def encrypt_public(self, x):
        return self._o.encrypt_public(x)

    @property
    def statistics(self):
        """Concrete's `fhe_circuit.statistics` is a property; here the engine's dctfhe_stats of the compiled circuit"""
        return self._o.statistics()


class QuantizedModule:
    def __init__(self, compiled, device=0, verbose=False, classifier=None, configuration=None):
        self.compiled = compiled
        self.configuration = configuration if configuration is not None else Configuration()
        self.device = device
        self.verbose = verbose
        self._ctx = None
        self._circuit = None
        self._keys = None
        self._sessions = {}
        self.fhe_circuit = FHECircuit(self)
        self.last_timing = None
        self.last_io = None
        self.sim_seed = 977
        self._compaction = None
        self._ring_compaction = None
        self._pack_key = None
        self._public_plan = None
        self._public_key = None
        self._public_key_of = None         # the key set forward(fhe="execute") made its own public key for

    # -- lazy device objects -------------------------------------------------------------
    def _context(self):
        if self._ctx is None:
            self._ctx = Context(self.device)
            self._circuit = Circuit(self._ctx, self.compiled.blob)
        return self._ctx

    def _keygen(self, seed, force=False):
        ctx = self._context()
        if self._keys is not None and not force:
            return
        if self._keys is not None:
            for k in [k for k in self._sessions if k[0] == "execute"]:
                self._sessions.pop(k).close()
            self._keys.close()
        self._keys = Keys(ctx, P.to_c_params(self.compiled.param_set), seed, tiers=self.key_tiers())

    def key_tiers(self):
        """the tier selection of this module's evaluation keys: None (every tier) under Configuration(evaluation_key_tiers="all"), under
        "circuit" CompiledCircuit.key_tiers for the configuration's output form"""
        if self.configuration.evaluation_key_tiers != "circuit":
            return None
        form = self.configuration.compress_output_ciphertexts
        if form == "ring":
            return self.compiled.key_tiers("ring", self.configuration.result_packing_spec)
        return self.compiled.key_tiers("rows" if form else None)

    def _session(self, mode, batch):
        key = (mode, batch)
        if key not in self._sessions:
            ctx = self._context()
            if mode == "execute" and self._keys is None:
                self._keygen(None)
            sess = Session(ctx, self._circuit, self._keys if mode == "execute" else None, batch)
            if self.configuration.device_memory_budget_bytes:
                try:
                    sess.set_memory_budget(self.configuration.device_memory_budget_bytes)
                except Exception:
                    sess.close()
                    raise
            self._sessions[key] = sess
        return self._sessions[key]

    def _shard_group(self):
        """(rank, world) when Configuration(shard_image=True) meets an initialised torch.distributed group of more than one rank"""
        if not self.configuration.shard_image:
            return None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
            return None
        return dist.get_rank(), dist.get_world_size()

    def _shard_session(self, batch, rank, world):
        """this rank's part of an image-sharded encrypted run: a session of its own, sharded before its first run"""
        if self._keys is None or not hasattr(self._keys, "decrypt"):
            raise RuntimeError("shard_image: every rank needs the same client key before forward(): fhe_circuit.keygen(seed=...) with one seed on all ranks")
        key = ("execute", ("shard", batch, rank, world))
        if key not in self._sessions:
            sess = Session(self._context(), self._circuit, self._keys, batch)
            sess.set_shard(rank, world)
            if self.configuration.shard_pool:
                sess.set_shard_pool(True)
            self._sessions[key] = sess
        return self._sessions[key]

    def output_compaction(self, form="rows"):
        """the tier packed results are key-switched to (dctfhe.compile.output_compaction; form "rows" or "ring"); raises ValueError where
        packing would leave the catalogue's failure budget"""
        if form == "ring":
            if self._ring_compaction is None:
                self._ring_compaction = cc.output_compaction(self.compiled, form="ring", spec=self.configuration.result_packing_spec)
            return self._ring_compaction
        if self._compaction is None:
            self._compaction = cc.output_compaction(self.compiled)
        return self._compaction

    def export_result_packing_key(self):
        """client side: the packing key of ring-packed results as a blob to ship to the server once (no secret inside; 13 MB at the default
        spec).  The spec is the one output_compaction("ring") priced"""
        if self._keys is None:
            self._keygen(None)
        if not isinstance(self._keys, Keys):
            raise RuntimeError("the result packing key is made by the client (its secret key); this module holds evaluation keys only")
        return self._keys.client.export_pack_key(self.output_compaction("ring").spec)

    def load_result_packing_key(self, blob):
        """server side (or a single process, with its own export): the packing key `compress_output_ciphertexts="ring"` packs with"""
        ctx = self._context()
        if self._pack_key is not None:
            self._pack_key.close()
        self._pack_key = PackKey(ctx, blob)

    def public_input_plan(self):
        """what public-key inputs cost this circuit (dctfhe.compile.public_input_plan with Configuration.public_input_spec); raises
        ValueError where a site would leave the catalogue's failure budget"""
        if self._public_plan is None:
            self._public_plan = cc.public_input_plan(self.compiled, self.configuration.public_input_spec)
        return self._public_plan

    def export_public_key(self):
        """client side: the public key of public-key inputs as a blob to hand to data owners (no secret inside; 16 KB at the default
        spec).  The spec is the one public_input_plan() priced"""
        spec = self.public_input_plan().spec
        if self._keys is None:
            if self._public_key is not None:      # a data owner's module: a fresh key set here would be an unrelated one
                raise RuntimeError("the public key is made by the client (its secret key); this module holds a loaded public key only")
            self._keygen(None)
        if not isinstance(self._keys, Keys):
            raise RuntimeError("the public key is made by the client (its secret key); this module holds evaluation keys only")
        return self._keys.client.export_public_key(spec)

    def load_public_key(self, blob):
        """data-owner side: the client's public key; this module can then run `encrypt_public` and needs neither the client key nor
        evaluation keys for it"""
        plan = self.public_input_plan()
        ctx = self._context()
        pk = PublicKey(ctx, blob)
        try:
            roles.check_public_key(plan, pk)
        except RuntimeError:
            pk.close()
            raise
        if self._public_key is not None:
            self._public_key.close()
        self._public_key, self._public_key_of = pk, None

    def encrypt_public(self, x):
        """data-owner side: float inputs [B, C, H, W] -> PublicInputs (quantise, encode, encrypt with the loaded public key)"""
        if self._public_key is None:
            raise RuntimeError("encrypt_public needs the client's public key: fhe_circuit.load_public_key(blob)")
        return roles.encrypt_public(self.compiled, self._public_key, x)

    def _own_public_key(self):
        """forward(fhe="execute") under Configuration(public_key_inputs=True): this module's own public key, made once per key set"""
        if self._public_key is None or self._public_key_of is not self._keys:
            self.load_public_key(self.export_public_key())
            self._public_key_of = self._keys
        return self._public_key

    def _ring_plan(self):
        """(tier, packing key) of a ring-packed download; refuses before anything runs"""
        return roles.ring_plan(self.output_compaction("ring"), self._pack_key)

    # -- client / server split (reference homomorphic_eval.py:313-317 keeps both halves in one process) ------------
    def export_evaluation_keys(self, compressed=None):
        """client side: the evaluation keys as a flat uint8 blob to ship to the server (no secret inside).  compressed (default:
        Configuration.compress_evaluation_keys): bodies + the public mask key, about a quarter of the size; needs the client key"""
        if self._keys is None:
            self._keygen(None)
        if compressed is None:
            compressed = self.configuration.compress_evaluation_keys
        if compressed:
            if not isinstance(self._keys, Keys):
                raise RuntimeError("compressed evaluation keys are made by the client (its secret key); this module holds evaluation keys only")
            return self._keys.client.export_eval_keys_compressed(self.key_tiers())
        return self._keys.eval.to_blob()      # the handle's own selection (keygen made it with key_tiers())

    def load_evaluation_keys(self, blob):
        """server side: evaluate with keys a client generated elsewhere (either blob form: full or compressed); this module can
        then run `evaluate_encrypted` but can neither encrypt nor decrypt"""
        from .engine import EvalKeys, blob_key_tiers
        need = self.key_tiers()
        if need is not None:      # refuse before anything is imported
            held = cc.KeyTierSelection.from_masks(self.compiled.param_set, *blob_key_tiers(blob))
            if not held.covers(need):
                raise ValueError(f"the evaluation keys do not cover this circuit: they lack the {held.missing(need)}")
        ctx = self._context()
        for k in [k for k in self._sessions if k[0] == "execute"]:
            self._sessions.pop(k).close()
        if self._keys is not None:
            self._keys.close()
        self._keys = EvalKeys.from_blob(ctx, blob)

    def evaluate_encrypted(self, cts, batch, dim=None, packed=None):
        """server side: input ciphertexts [batch * n_in, D+1] -> output ciphertexts [batch * n_out, D+1]; dim: the compact wire
        form instead -- input rows of dim mask words + body, output rows of Session.dims()[1] mask words + body.  cts may also be
        SeededCiphertexts (or their to_bytes() form): the masks are regenerated on the GPU; dim then only selects the output form.
        PublicInputs (or their to_bytes() form, told from seeded bytes by the magic): the rows are extracted on the GPU, likewise.
        packed (default: Configuration.compress_output_ciphertexts): True / "rows": the outputs as PackedCiphertexts instead, "ring": as
        a PackedRing (needs load_result_packing_key), whatever dim says"""
        cts = roles.parse_inputs(cts)
        if isinstance(cts, PublicInputs):
            self.public_input_plan()          # refuses before anything runs
        packed = self.configuration.compress_output_ciphertexts if packed is None else _output_form(packed)
        pack_key = None
        if packed == "ring":
            tier, pack_key = self._ring_plan()
        else:
            tier = self.output_compaction().tier if packed else None
        return roles.evaluate_encrypted(self._session("execute", batch), self._keys, cts, dim, packed, tier, pack_key)

    def statistics(self):
        self._context()
        return self._circuit.stats(P.to_c_params(self.compiled.param_set))

    # -- quantisation at the boundary ----------------------------------------------------
    def quantize_input(self, x):
        return roles.quantize_input(self.compiled, x)

    def encode_input(self, q):
        return roles.encode_input(self.compiled, q)

    def decode_output(self, phases):
        return roles.decode_output(self.compiled, phases)

    def decrypt_result(self, x):
        """client side: what evaluate_encrypted returned -> decoded integers [B, F].  x: PackedCiphertexts or a PackedRing, or the
        to_bytes() form of either, or rows [B * F, dim + 1] of uint64 (full width or the compact wire form)"""
        if self._keys is None or not hasattr(self._keys, "decrypt"):
            raise RuntimeError("decrypting needs the client key (fhe_circuit.keygen); this module holds evaluation keys only")
        return roles.decrypt_result(self.compiled, self._keys, x)

    def dequantize_output(self, q):
        return roles.dequantize_output(self.compiled, q)

    # -- the reference's entry point -----------------------------------------------------
    def forward(self, x, fhe="disable"):
        """x: float [B, C, H, W] -> float [B, F]  (reference homomorphic_eval.py:70)."""
        if fhe not in ("disable", "simulate", "execute"):
            raise ValueError(f"fhe mode {fhe!r}")
        x = np.asarray(x)
        q = self.quantize_input(x)
        out_q = self.forward_quantized(q, fhe)
        return self.dequantize_output(out_q)

    def forward_quantized(self, q, fhe="disable"):
        phases = self.encode_input(q)
        B = q.shape[0]
        mode = "execute" if fhe == "execute" else "clear"
        shard = self._shard_group() if mode == "execute" else None
        sess = self._session(mode, B) if shard is None else self._shard_session(B, *shard)
        if mode == "clear":
            # "simulate" = the integer circuit with the compiler's noise model sampled at every look-up (reference: Concrete's
            # simulation, homomorphic_eval.py:333-347); "disable" = noise-free.  At the exact tiers the two coincide.
            if fhe == "simulate":
                sess.set_noise(self.sim_seed, self.compiled.simulation_sigmas())
                sess.set_noise_split(self.compiled.simulation_sigmas_split())
                self.sim_seed += 1
            else:
                sess.set_noise(0, None)
        t0 = time.time()
        if mode == "execute":
            # ciphertexts travel in the compact wire form: a fresh encryption masks input_dim words, an output the ring of the last
            # table tier -- not the D words of the master key (include/dctfhe.h dctfhe_encrypt_rows)
            # Configuration(compress_input_ciphertexts=True): only the bodies travel (seeded form), the GPU regenerates the masks
            in_dim, out_dim = sess.dims()
            seeded = self.configuration.compress_input_ciphertexts
            # Configuration(compress_output_ciphertexts=True): results come back packed (refused here, before anything is encrypted,
            # where the compiler's price for it leaves the budget)
            form = self.configuration.compress_output_ciphertexts
            if form == "ring":
                pack_tier, pack_key = self._ring_plan()
            else:
                pack_tier = self.output_compaction().tier if form else None
            # Configuration(public_key_inputs=True): encrypted without the secret key, extracted on the GPU (priced first, like the above)
            public = self._own_public_key() if self.configuration.public_key_inputs else None
            t1 = time.time()
            if shard is not None:
                # an image over the ranks' GPUs: rank 0 encrypts -- in the seeded form, or with the public key -- and its blob travels
                # (kilobytes; a handle's encryption randomness is its own, so the ranks must not each encrypt); every rank expands it whole
                import torch
                from . import sharding
                dev, seeded = torch.device("cuda", self.device), public is None
                blob = b""
                if shard[0] == 0:
                    blob = (public.encrypt(phases.reshape(-1)) if public is not None else self._keys.encrypt_seeded(phases.reshape(-1))).to_bytes()
                blob = sharding.broadcast_bytes(blob, shard[1], dev)
                cts = PublicInputs.from_bytes(blob) if public is not None else SeededCiphertexts.from_bytes(blob)
            elif public is not None:
                cts = public.encrypt(phases.reshape(-1))
            else:
                cts = self._keys.encrypt_seeded(phases.reshape(-1)) if seeded else self._keys.encrypt(phases.reshape(-1), in_dim)
            t2 = time.time()
            if public is not None:
                sess.upload_public(cts)
            elif seeded:
                sess.upload_seeded(cts)
            else:
                sess.upload(cts, in_dim)
            t3 = time.time()
            if shard is not None:
                # run_span to each exchange point of the compiler's plan, the rows of that tensor between the ranks, mark_whole; the
                # output is whole on every rank at the end, so each downloads and decrypts its own copy
                # (shard_pool: the plan with row ranges -- a rank receives its need range of a divided pool's source, then mark_rows)
                if self.configuration.shard_pool:
                    plans = [self.compiled.shard_plan(rows=True, part=p, parts=shard[1], batch=B) for p in range(shard[1])]
                    spans, moved = sharding.run_sharded_rows(sess, plans, len(self.compiled.ops), cc.shard_rows, shard[0], shard[1], dev, timing=True)
                else:
                    spans, moved = sharding.run_sharded(sess, self.compiled.shard_plan(), len(self.compiled.ops), cc.shard_rows, shard[1], dev, timing=True)
                timing = _sum_timings(spans)
            else:
                timing = sess.run(timing=True)
            t4 = time.time()
            if pack_tier is None:
                out = sess.download(out_dim).reshape(-1, out_dim + 1)
                t5 = time.time()
                out_ph = self._keys.decrypt(out, out_dim).reshape(B, -1)
            elif form == "ring":
                pr = sess.download_ring(pack_tier, pack_key)
                out = pr.words
                t5 = time.time()
                out_ph = self._keys.decrypt_ring(pr).reshape(B, -1)
            else:
                pk = sess.download_packed(pack_tier)
                out = pk.rows
                t5 = time.time()
                out_ph = self._keys.decrypt_packed(pk).reshape(B, -1)
            self.last_io = dict(encrypt_s=t2 - t1, upload_s=t3 - t2, run_s=t4 - t3, download_s=t5 - t4, decrypt_s=time.time() - t5,
                                input_bytes=int(cts.words.nbytes if public is not None else cts.nbytes), output_bytes=int(out.nbytes),
                                upload_bytes=int(cts.words.nbytes if public is not None else cts.bodies.nbytes if seeded else cts.nbytes))
            if shard is not None:
                self.last_io.update(shard=shard, exchanged_bytes=int(moved))
        else:
            sess.upload(phases)
            timing = sess.run(timing=True)
            out_ph = sess.download().reshape(B, -1)
        self.last_timing = dict(total_ms=timing.total_ms, pbs_ms=list(timing.pbs_ms), ks_ms=timing.ks_ms, linear_ms=timing.linear_ms,
                                wall_s=time.time() - t0)
        return self.decode_output(out_ph)

    # -- margin audit (include/dctfhe.h dctfhe_session_set_audit): a development and assurance tool ------------------
    def audit_quantized(self, q):
        """An encrypted pass over integer inputs q [B, C, H, W] with the margin audit on: (decoded outputs [B, F], MarginReport).  Every
        bootstrap decision of the run is measured with the client's secret key, so it runs where the client key is."""
        if self.configuration.shard_image:
            raise RuntimeError("the margin audit stays unsharded: audit() is refused under Configuration(shard_image=True)")
        if self._keys is not None and not hasattr(self._keys, "decrypt"):
            raise RuntimeError("the margin audit needs the client key (fhe_circuit.keygen); this module holds evaluation keys only")
        phases = self.encode_input(q)
        B = q.shape[0]
        sess = self._session("execute", B)
        in_dim, out_dim = sess.dims()
        sess.set_audit(self._keys.client)
        try:
            sess.upload(self._keys.encrypt(phases.reshape(-1), in_dim), in_dim)
            sess.run()
            slots = sess.audit()
            out = sess.download(out_dim).reshape(-1, out_dim + 1)
        finally:
            sess.set_audit(None)
        report = MarginReport.from_slots(slots, self.compiled.margin_model(), self.compiled.param_set)
        return self.decode_output(self._keys.decrypt(out, out_dim).reshape(B, -1)), report

    def audit(self, x):
        """x: float [B, C, H, W] -> (float outputs [B, F] of an encrypted pass, MarginReport)"""
        out_q, report = self.audit_quantized(self.quantize_input(np.asarray(x)))
        return self.dequantize_output(out_q), report

    def close(self):
        for s in self._sessions.values():
            s.close()
        self._sessions = {}
        if self._keys is not None:
            self._keys.close()
            self._keys = None
        if self._pack_key is not None:
            self._pack_key.close()
            self._pack_key = None
        if self._public_key is not None:
            self._public_key.close()
            self._public_key = None
        if self._circuit is not None:
            self._circuit.close()
            self._circuit = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


def _sum_timings(spans):
    """the spans of a sharded pass as one Timing: every field summed"""
    from ._lib import MAX_TIERS, Timing
    out = Timing()
    for t in spans:
        out.total_ms += t.total_ms
        out.ks_ms += t.ks_ms
        out.linear_ms += t.linear_ms
        for i in range(MAX_TIERS):
            out.pbs_ms[i] += t.pbs_ms[i]
            out.pbs_launches[i] += t.pbs_launches[i]
            out.pbs_cts[i] = t.pbs_cts[i]
    return out


def _as_numpy(t):
    if hasattr(t, "detach"):
        return t.detach().cpu().numpy()
    return np.asarray(t)


def compile_brevitas_qat_model(torch_model, torch_inputset, n_bits=5, configuration=None, rounding_threshold_bits=6, p_error=None,
                               verbose=False, device=0, param_set=None, tier_policy="exact", pool_policy="coarse", **kwargs):
    """Same keyword surface as the call at reference homomorphic_eval.py:276-285.  `torch_model` is what the reference
    passes -- the trunk `model.module.feature`, a torch.nn.Module walked by dctfhe.torch_import (duck-typed: the float
    `ResNetDCT` and, where Brevitas exists, `ResNetQDCT` import unchanged) -- or a dctfhe.models.ResNetQ description.
    `bit_width` (dctfhe addition): weight/activation width when the module does not say (`qconv_args`).
    rounding_threshold_bits: int (exact rounding) or {"n_bits": int, "method": "exact"|"approximate"} as the reference's
    README.md:95-114 suggests.  tier_policy: "exact" (default, outputs equal the integer circuit whatever p_error) or
    "p_error" (cheaper tiers whose look-ups fail with probability <= p_error; dctfhe addition).  pool_policy: "coarse" (default) or
    "exact" (a max pool that leaves the budget on its coarse tier moves to the catalogue's quiet pool tier; dctfhe addition)."""
    method = "exact"
    if isinstance(rounding_threshold_bits, dict):
        method = str(rounding_threshold_bits.get("method", "exact")).lower().split(".")[-1]      # also accepts "Exactness.APPROXIMATE"
        rtb = rounding_threshold_bits["n_bits"]
    else:
        rtb = rounding_threshold_bits
    from . import torch_import
    bit_width = kwargs.pop("bit_width", None)
    if torch_import.is_torch_module(torch_model):
        torch_model = torch_import.from_torch_module(torch_model, bit_width=bit_width or 4)
    compiled = cc.compile_model(torch_model, _as_numpy(torch_inputset), rounding_threshold_bits=rtb, n_bits=n_bits,
                                param_set=param_set, p_error=p_error, rounding_method=method, tier_policy=tier_policy,
                                pool_policy=pool_policy)
    return QuantizedModule(compiled, device=device, verbose=verbose, configuration=configuration)


def compile_torch_model(torch_model, torch_inputset, n_bits=5, configuration=None, rounding_threshold_bits=6, p_error=None,
                        verbose=False, device=0, param_set=None, tier_policy="exact", pool_policy="coarse", **kwargs):
    """PTQ twin of the above (reference homomorphic_eval.py:287-295): a float torch trunk (`ResNetDCT`), every weight and
    activation quantised to `n_bits` post-training ([K] Concrete-ML's PTQ applies n_bits to all ops) unless `bit_width`
    says otherwise; the circuit builder is the same."""
    from . import torch_import
    if torch_import.is_torch_module(torch_model):
        kwargs.setdefault("bit_width", n_bits)
    return compile_brevitas_qat_model(torch_model, torch_inputset, n_bits, configuration, rounding_threshold_bits, p_error, verbose,
                                      device, param_set, tier_policy, pool_policy, **kwargs)
