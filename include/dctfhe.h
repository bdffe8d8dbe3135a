/*
 * dctfhe.h -- C ABI of libdctfhe.so, the MI355X-native homomorphic-evaluation engine that sits
 * behind the reference's third-party boundary.
 *
 * The reference (zhiyongggggg/dct-cryptonets) is pure Python; its hot path is reached through
 * five call sites into concrete-ml / concrete-python (absent third-party wheels):
 *
 *   (R1) compile_brevitas_qat_model(feature, calib, ...)   dct-cryptonets/homomorphic_eval.py:276-285
 *        compile_torch_model(...)                          dct-cryptonets/homomorphic_eval.py:287-295
 *   (R2) q_module.fhe_circuit.graph.maximum_integer_bit_width()            homomorphic_eval.py:301
 *   (R3) q_module.fhe_circuit.keygen()                                     homomorphic_eval.py:315
 *   (R4) q_module.forward(data, fhe="simulate"|"execute")                  homomorphic_eval.py:70
 *   (R5) q_module.fhe_circuit.mlir                                         homomorphic_eval.py:311
 *
 * Nothing like a C interface exists in the reference; each entry point below names the call
 * site whose work it carries.  The Python facade that keeps the reference's names
 * (dct-cryptonets_amd/dctfhe/quantized_module.py) binds these with ctypes; INTEGRATION.md shows
 * the stub.  Conventions: opaque handles, int status (0 = OK, <0 = error, text through
 * dctfhe_last_error()), caller-allocated host buffers, no exceptions across the boundary.
 * A dctfhe_ctx is bound to one GPU and one host thread (one per rank); distinct contexts are
 * independent: each has a stream of its own, and nothing orders the streams of two contexts.
 *
 * WHAT A HANDLE IS BOUND TO.  Client keys, evaluation keys, packing keys, public keys and sessions belong to
 * the CONTEXT they were made on: their work is issued to that context's stream.  Every entry point that takes
 * a dctfhe_ctx together with such a handle refuses a handle of another context (the message says "context"),
 * dctfhe_session_create refuses evaluation keys of another context and dctfhe_session_set_audit a client key
 * of another context than the session's.  A refused call has allocated, copied and launched nothing: every
 * handle stays usable and the caller's buffers are untouched.  A CIRCUIT belongs to a DEVICE: its payload is
 * uploaded once by dctfhe_circuit_load and only read afterwards, so sessions of several contexts of that
 * device may share one circuit handle (dctfhe_session_copy_rows expects it); dctfhe_session_create refuses a
 * circuit of another device (the message says "device").  Key material is a pure function of (params, seed):
 * a second context gets the same keys from the same seed.  One context, and the handles made on it, are used
 * by one host thread at a time; two threads with a context each run side by side, and dctfhe_last_error() is
 * per thread.  Ciphertext layout, encodings and key formats: DESIGN.md section 3.
 */
#ifndef DCTFHE_H
#define DCTFHE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DCTFHE_MAX_TIERS 12

typedef struct dctfhe_ctx dctfhe_ctx;
typedef struct dctfhe_client_key dctfhe_client_key;   /* CLIENT: secret keys + the CSPRNG keys; never needed by the server */
typedef struct dctfhe_eval_keys dctfhe_eval_keys;     /* SERVER: key-switch keys + Fourier bootstrap keys (public material) */
typedef struct dctfhe_circuit dctfhe_circuit;
typedef struct dctfhe_session dctfhe_session;

/* One bootstrapping parameter tier (what concrete-optimizer picks per partition; R1 p_error). */
typedef struct {
  int32_t n;            /* small LWE dimension (prefix of the small secret key) */
  int32_t k, logN;      /* GLWE dimension, log2 polynomial size; k*N <= D (prefix of the big key) */
  int32_t l, beta;      /* bootstrap gadget: levels 1..4, base log; l*beta <= 63, beta <= 28 (l = 1), 16 (l = 2, 3), 10 (l = 4: k = 1, N = 2048 only) */
  int32_t lk, betak;    /* key-switch gadget: levels, base log */
  int32_t ksk_share;    /* >= 0: reuse the key-switch key of that (earlier) tier; -1: own key */
  int32_t unroll;       /* key bits per blind-rotate iteration: 1, or 2 (k = 1, l = 1, n even; key of 3n/2 blocks) */
  int32_t reserved;     /* must be 0 (formerly key_lds; kept so that the evaluation-key blob layout does not change) */
  double lwe_sigma;     /* noise std of key-switch-key rows (fraction of the torus) */
  double glwe_sigma;    /* noise std of bootstrap-key rows */
} dctfhe_tier;

typedef struct {
  int32_t D;            /* big LWE dimension = length of the master binary key */
  int32_t n_max;        /* length of the small binary key */
  int32_t n_tiers;
  int32_t input_dim;    /* fresh client encryptions mask only the first input_dim words (a prefix of the big key, like
                           every bootstrap output of a smaller ring); 0 = D.  input_sigma must suit that dimension. */
  double input_sigma;   /* noise std of fresh client encryptions */
  dctfhe_tier tiers[DCTFHE_MAX_TIERS];
} dctfhe_params;

typedef struct {
  int64_t pbs_count[DCTFHE_MAX_TIERS];   /* bootstraps per image, per tier */
  int64_t ks_count[DCTFHE_MAX_TIERS];    /* key switches per image, per tier */
  int64_t conv_macs;                     /* scalar ciphertext*plaintext MACs per image */
  int64_t lut_sites, bit_steps;          /* table look-ups and one-bit rounding steps per image */
  double bytes_algorithmic;              /* SURVEY 8(d) B_img without the key passes */
  double key_bytes_per_pass;             /* sum over layer steps of |BSK|+|KSK| (divide by images per batch) */
  double flops_f64;                      /* SURVEY 8(d) F_img */
  int32_t max_bit_width;                 /* R2 */
  int32_t n_ops;
} dctfhe_stats;

/* Per-run timing (milliseconds, HIP events on the context's stream). */
typedef struct {
  double total_ms;
  double pbs_ms[DCTFHE_MAX_TIERS];
  double ks_ms;
  double linear_ms;
  int64_t pbs_launches[DCTFHE_MAX_TIERS];
  int64_t pbs_cts[DCTFHE_MAX_TIERS];
} dctfhe_timing;

const char* dctfhe_last_error(void);
int dctfhe_version(void);

int dctfhe_ctx_create(int device_id, dctfhe_ctx** out);
int dctfhe_ctx_destroy(dctfhe_ctx* ctx);
/* Issue the context's work to an existing HIP stream of the context's device -- a stream the caller made, e.g. a torch.cuda.Stream()
 * (its .cuda_stream) -- instead of the context's own; NULL resets to the context's own stream.  Torch's DEFAULT stream is the null stream,
 * whose handle is NULL: passing it resets the context, it does not put the library on the null stream.
 * Guarantee: every copy, fill and kernel of a later call on this context or on a handle made on it goes to that stream (a handle follows
 * its context's stream at call time, whenever it was made), so the library's work runs after whatever the caller had enqueued on the stream
 * before the call, with no host synchronisation in between; dctfhe_ctx_synchronize waits for the stream that is set.
 * Not guaranteed: asynchrony.  Every call still returns only when its own work is done (dctfhe_session_run is synchronous), and allocating
 * or freeing device memory inside a call may wait for ALL streams of the device.  Blocking copies of host operands into buffers the call has
 * just allocated do not wait for the stream; nothing reads them before the call's own launches.  The stream must outlive its use here. */
int dctfhe_ctx_set_stream(dctfhe_ctx* ctx, void* hip_stream);
int dctfhe_ctx_synchronize(dctfhe_ctx* ctx);

/* R3 keygen() (homomorphic_eval.py:313-317).  The reference's `fhe_circuit.keygen()` makes a client key set and the
 * evaluation keys the server needs; here they are two handles so that the secret never has to reach the server.
 *
 * Randomness: a counter-mode ChaCha20 generator on the GPU keyed by the caller's 32-byte seed (draw it from the OS:
 * os.urandom / getrandom).  The secret-key bits and every noise term come from the seed's own stream; ciphertext and key
 * MASKS come from a second ChaCha20 key that is one block of the first (public: knowing it gives nothing about the seed).
 * The KEY MATERIAL of a client key is a pure function of (params, seed): persist the 32 bytes to persist it; every rank of a
 * multi-GPU job gets the same keys from the same seed (broadcast the seed, not the keys).  Encryption randomness is NOT a
 * function of the seed alone: see dctfhe_encrypt.
 * SECURITY STATUS: parameters follow a fit through published 128-bit sets (dctfhe/params.py), not an estimator run --
 * there is none in this environment; treat the "~128-bit" figure as unverified. */
int dctfhe_client_key_create(dctfhe_ctx* ctx, const dctfhe_params* params, const uint8_t seed[32], dctfhe_client_key** out);
int dctfhe_client_key_destroy(dctfhe_client_key* client);
/* client side: evaluation keys for `client`'s secret (the expensive part of keygen; runs on the GPU) */
int dctfhe_eval_keys_generate(dctfhe_client_key* client, dctfhe_eval_keys** out);
/* both at once */
int dctfhe_keygen(dctfhe_ctx* ctx, const dctfhe_params* params, const uint8_t seed[32], dctfhe_client_key** client,
                  dctfhe_eval_keys** eval);
int dctfhe_eval_keys_destroy(dctfhe_eval_keys* eval);
/* evaluation-key persistence / shipping to the server: a flat blob (header + parameters, then per tier its key-switch key
 * and its Fourier bootstrap key).  buf == NULL: only *size is written (size query).
 * Blob ('DEVK', little-endian): u32 magic, u32 version, u64 total bytes, the dctfhe_params; then per tier its own key-switch key
 * [D][lk][n+1] u64 (absent where ksk_share >= 0) and its Fourier bootstrap key: exactly blocks (k+1) l (k+1) polynomials in the order of
 * dctfhe_client_key_export_bsk (blocks = n, or 3n/2 for unroll 2; no padding), each M = N/2 complex doubles (re, im).
 * Fourier-key layout of one polynomial: the forward transform runs in place in mixed radix M = R_0 ... R_{s-1} with P = 8 or 16 points
 * per thread (16 for logN 9, l 2; 8 for every other shape), every pass of radix P and the last of radix M / P^(s-1), T = M / P threads.
 * Entry j T + t (j < P, t < T) holds in-place position p = P t + j.  Its value is the polynomial, coefficients read as SIGNED 64-bit
 * integers, evaluated at e^{i pi (1 - 4k) / N} and multiplied by 2^-64 / M, where k = spectrum_freq(p) (csrc/fft_core.h): with
 * W_i = prod_{j > i} R_j, digit (p / W_i) mod R_i of the position is frequency digit k_i of weight R_0 ... R_{i-1}.
 * (The blob's order is one rule for every shape.  On the device the general two-bit tier at logN 11, l 3 keeps its key in the order of a
 * transform with 4 points per thread; export and import permute its entries frequency for frequency.)
 * tests/key_material_ref.py restates the rule; tests/test_gpu_key_material.py holds every shape's key to a long-double transform. */
int dctfhe_eval_keys_export(dctfhe_eval_keys* eval, void* buf, size_t capacity, size_t* size);
/* import accepts both blob forms: the one above and the compressed one below (told apart by the magic). */
int dctfhe_eval_keys_import(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_eval_keys** out);
/* COMPRESSED evaluation keys (CLIENT side: the bodies need the secret).  Every key mask word is a draw of the client's public generator key
 * (one ChaCha20 block of the secret one), so the blob holds the header and parameters, that 32-byte key, then per tier the D*lk bodies of
 * its own key-switch key (u64, on the 2^-(8 limbs) grid) and the standard-domain bodies of its bootstrap key, blocks x (k+1)l x N u64
 * (blocks = n, or 3n/2 for unroll 2).  dctfhe_eval_keys_import regenerates the masks on the GPU and transforms the bootstrap key as
 * dctfhe_eval_keys_generate does.  Key-switch keys and the bootstrap-key rows whose gadget term sits in the body (p = k) decompress bit
 * for bit; the rows p < k are shipped in BODY FORM (a, b - s_i g S_p): the same phase and noise draw, another ciphertext.  About a
 * quarter of dctfhe_eval_keys_export's size for the default parameters.  buf == NULL: size query. */
int dctfhe_eval_keys_export_compressed(dctfhe_client_key* client, void* buf, size_t capacity, size_t* size);
/* test view: the standard-domain bootstrap key [blocks][(k+1)l][k+1][N] of `tier` as import rebuilds it from a compressed blob
 * (refused for a tier whose bootstrap key a pruned blob does not hold) */
int dctfhe_eval_keys_decompress_bsk(dctfhe_ctx* ctx, const void* buf, size_t size, int tier, uint64_t* out);

/* TIER SELECTIONS: evaluation keys sized to a circuit.  A catalogue is one fixed list of tiers and a compiled
 * circuit reads only some of their keys; a selection, carried BESIDE the parameters (tier indices are part of the circuit blob and of every
 * key stream id, so the parameters themselves cannot shrink), says which keys are made, exported, imported and held.
 *   bsk bit t: the bootstrap key of tier t is present.
 *   ksk bit t: the key-switch key that tier t OWNS is present.  A tier with ksk_share >= 0 owns none: it needs the ksk bit of the owner at
 *              the end of its share chain.
 * CLOSING a selection sets the owner's ksk bit for every tier whose bsk bit is set.  Refused: a bit at or beyond n_tiers, a ksk bit on a
 * tier that shares.  (A dropped bootstrap key whose key-switch key stays is the ordinary case: T6 next to T6a, which switches with T6's.)
 * Everything selected -- dctfhe_key_tiers_all, and a NULL selection wherever one is taken -- is what the library did before selections
 * existed: the same keys, the same blobs byte for byte.  The kept keys of any other selection are word for word those of the full set from
 * the same seed (a key's draws depend on its tier index and nothing else), and the server draws nothing at random, so a run under pruned
 * keys produces the output ciphertext words of the run under full keys.
 * An absent key is not generated, transformed or allocated.
 * Blobs: everything selected writes the version of each form documented above.  Any other selection writes the NEXT version of that form
 * ('DEVK' version 4, 'DEVC' version 2): the two masks (u32 bsk, u32 ksk) follow the header -- in the compressed form the public generator
 * key -- then the kept sections in tier order.  dctfhe_eval_keys_import reads all four kinds; it checks the masks before it sizes
 * anything (a closed selection within n_tiers, not everything) and the total size against them.
 * Refusals: every entry point that reads a key the handle lacks returns -1 before it allocates, copies or launches; the message names the
 * tier and says "bootstrap key" or "key-switch key".  dctfhe_session_create names the first missing tier and an op that needs it.
 * dctfhe_modswitch_center asks for the bootstrap key of its tier (it rounds to that bootstrap's levels).  dctfhe_margin_probe takes a client
 * key, which holds no selection, and dctfhe_session_set_audit a session, whose keys dctfhe_session_create has already checked.
 * all / close / for_circuit / blob_bytes run on the host without a GPU. */
typedef struct { uint32_t bsk, ksk; } dctfhe_key_tiers;
int dctfhe_key_tiers_all(const dctfhe_params* params, dctfhe_key_tiers* out);
int dctfhe_key_tiers_close(const dctfhe_params* params, dctfhe_key_tiers* io);
/* the closed selection of a circuit blob: every tier an op bootstraps on (rounding steps, table tiers, the second tier of a split site, the
 * parity bootstrap, max-pool tiers) and the owner of every key-switch key an op switches with -- exactly the tiers whose pbs_count /
 * ks_count in dctfhe_circuit_stats is positive.  Refused: a circuit that names a tier the parameters lack. */
int dctfhe_key_tiers_for_circuit(const void* blob, size_t size, const dctfhe_params* params, dctfhe_key_tiers* out);
/* bytes of dctfhe_eval_keys_export (compressed = 0) or dctfhe_eval_keys_export_compressed (!= 0) under a CLOSED selection */
int dctfhe_key_tiers_blob_bytes(const dctfhe_params* params, const dctfhe_key_tiers* tiers, int compressed, size_t* out);
/* tiers == NULL: everything.  The selection is closed first. */
int dctfhe_eval_keys_generate_tiers(dctfhe_client_key* client, const dctfhe_key_tiers* tiers, dctfhe_eval_keys** out);
int dctfhe_eval_keys_export_compressed_tiers(dctfhe_client_key* client, const dctfhe_key_tiers* tiers, void* buf, size_t capacity, size_t* size);
/* the selection a handle holds (generated or imported); dctfhe_eval_keys_export of a pruned handle writes a pruned blob */
int dctfhe_eval_keys_tiers(dctfhe_eval_keys* eval, dctfhe_key_tiers* out);

/* test / client views */
int dctfhe_client_key_export_secret(dctfhe_client_key* client, uint8_t* big_key /* D */, uint8_t* small_key /* n_max */);
/* standard-domain keys: ksk [D][lk][n+1] (public, from the evaluation keys); bsk [n][(k+1)l][k+1][N], regenerated from the
 * client's streams -- exactly what dctfhe_eval_keys_generate transformed to the Fourier domain.
 * Key-switch-key words live on the torus grid 2^-(8 limbs), limbs = 2 / 4 / 8 for lk*betak + 6 <= 16 / <= 32 / more (their low
 * 64 - 8 limbs bits are zero: masks drawn on the grid, bodies rounded to it); dctfhe_eval_keys_import refuses a key off that grid.
 *
 * Generator streams of the key material (pub: the client's PUBLIC generator key, the 32 bytes a compressed blob carries after its
 * parameters; sec: the secret one, the seed).  A mask word is a generator word (dctfhe_rng_*); a noise term is the Gaussian draw of its
 * index: generator words 2 idx and 2 idx + 1 through Box-Muller, times sigma 2^64, rounded to the nearest integer (variance
 * (sigma 2^64)^2 + 1/12 in units of 2^-64; 0 where sigma = 0).
 *   key-switch key of tier t, row = i lk + lev (i < D): mask word j < n is (pub, 16 + 2t, row (n + 1) + j) with the low 64 - 8 limbs bits
 *     cleared; noise (sec, 16 + 2t + 1, row); body = <a, s> + noise + S_i 2^(64 - betak (lev + 1)), rounded to the grid (a tie goes up).
 *   bootstrap key of tier t, global row grow = block (k + 1) l + r, r = p l + lev (p <= k, lev < l): coefficient c of mask polynomial
 *     j < k is (pub, 64 + 2t, (grow k + j) N + c); noise coefficient c is (sec, 64 + 2t + 1, grow N + c).  The row is
 *     GLWE_S(0) + bit_block 2^(64 - beta (lev + 1)) at coefficient 0 of polynomial p (a mask polynomial for p < k, the body for p = k),
 *     S_j = bits [j N, (j + 1) N) of the big key; bit = the small key's, or for unroll 2 the pair secret's: per pair (a, b) the blocks
 *     a (1 - b), (1 - a) b, a b.  The indices are global: they do not depend on how a key is generated in pieces.
 * The tier index is part of every stream id, so two tiers of one shape share no draw.  The compressed blob ships the same rows with pure
 * draws as masks (BODY FORM, see dctfhe_eval_keys_export_compressed): same noise terms, word for word. */
int dctfhe_eval_keys_export_ksk(dctfhe_eval_keys* eval, int tier, uint64_t* out);
int dctfhe_client_key_export_bsk(dctfhe_client_key* client, int tier, uint64_t* out);
/* the generator itself: `count` 64-bit outputs (key, stream, idx0 + i).  _host runs on the CPU (known-answer tests need no GPU) */
int dctfhe_rng_host(const uint8_t key[32], uint64_t stream, uint64_t idx0, size_t count, uint64_t* out);
int dctfhe_rng_device(dctfhe_ctx* ctx, const uint8_t key[32], uint64_t stream, uint64_t idx0, size_t count, uint64_t* out);
/* bytes of device memory the library holds in this process right now: the sum over every live allocation of the size it was made with
 * (handles, caches and the buffers of calls in flight).  Host-only: an atomic counter, no device needed. */
size_t dctfhe_device_bytes_live(void);

/* R4, client half: encrypt phases (already encoded) / return phases b - <a,s>.  Host buffers.  Every dctfhe_encrypt call
 * draws masks and noise from fresh generator streams (a per-handle call counter). */
int dctfhe_encrypt(dctfhe_ctx* ctx, dctfhe_client_key* client, const uint64_t* phases, size_t count,
                   uint64_t* cts /* count x (D+1) */);
int dctfhe_decrypt(dctfhe_ctx* ctx, dctfhe_client_key* client, const uint64_t* cts, size_t count, uint64_t* phases);
/* The same in the COMPACT WIRE FORM: rows of `dim` mask words + the body instead of D + 1 words.  A fresh encryption masks only
 * params.input_dim words and a circuit output only the ring of its last table tier (dctfhe_session_dims), so the host <-> device
 * and client <-> server traffic of an image shrinks by D / dim (ResNet-18 48x112^2: 39.5 GB -> 9.9 GB of input per image).
 * encrypt: input_dim <= dim <= D (words from input_dim on are zero); decrypt: dim <= D (the words a row lacks count as zero).
 * Both forms of one call hold the same ciphertexts. */
int dctfhe_encrypt_rows(dctfhe_ctx* ctx, dctfhe_client_key* client, const uint64_t* phases, size_t count, int dim,
                        uint64_t* cts /* count x (dim+1) */);
int dctfhe_decrypt_rows(dctfhe_ctx* ctx, dctfhe_client_key* client, const uint64_t* cts /* count x (dim+1) */, size_t count, int dim,
                        uint64_t* phases);
/* ENCRYPTION RANDOMNESS IS PER HANDLE.  Key material is a pure function of (params, seed) -- persist or broadcast the 32 bytes to
 * persist or share the key -- but the masks and noise of dctfhe_encrypt come from generator keys derived from the seed AND a 128-bit
 * nonce that dctfhe_client_key_create draws from the OS (getrandom), at a position given by a per-handle call counter.  Two handles
 * made from one seed (a re-created key, a second process, the ranks of a job) therefore never draw the same mask or noise.
 * set_encrypt_counter moves the position inside the handle's own streams (kept for callers that partition them); set_encrypt_nonce
 * FIXES the nonce -- reproducible experiments and tests only: handles with equal seed, nonce and counter encrypt identically. */
/* SEEDED input ciphertexts: the client keeps the masks to itself -- they are draws of the handle's public encryption key (one ChaCha20
 * block of its secret one) -- and ships the 32-byte key, the stream id and one body per ciphertext (8 bytes instead of 8 (input_dim + 1)).
 * encrypt_seeded takes one step of the call counter like dctfhe_encrypt_rows; for equal nonce and counter the expanded ciphertexts are
 * bit for bit those of dctfhe_encrypt_rows(dim = input_dim): mask word j < input_dim of ciphertext c is generator word
 * (mask_key, stream, c (D+1) + j).  expand_seeded is the server's stand-alone expander: rows of dim >= dim_eff mask words + body
 * (words from dim_eff on zero).  dctfhe_session_upload_seeded writes the masks straight into a session's input tensor. */
int dctfhe_encrypt_seeded(dctfhe_ctx* ctx, dctfhe_client_key* client, const uint64_t* phases, size_t count, uint8_t mask_key[32] /* out */,
                          uint64_t* stream /* out */, uint64_t* bodies /* count */);
int dctfhe_expand_seeded(dctfhe_ctx* ctx, const uint8_t mask_key[32], uint64_t stream, int D, int dim_eff, const uint64_t* bodies, size_t count,
                         int dim, uint64_t* rows /* count x (dim+1) */);
int dctfhe_client_key_set_encrypt_counter(dctfhe_client_key* client, uint64_t next_call);
int dctfhe_client_key_set_encrypt_nonce(dctfhe_client_key* client, const uint8_t nonce[16]);

/* R4, server half, one primitive at a time on host buffers (parity tests, integration). */
int dctfhe_keyswitch(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* cts, size_t count,
                     int shift, uint64_t* cts_small /* count x (n+1) */);
/* the same when the caller knows every input to be zero beyond mask word `deff` (nested keys: outputs of a ring of
 * dimension k*N <= deff): only the first deff rows of the key are used -- identical result, deff/D of the work */
int dctfhe_keyswitch_prefix(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* cts, size_t count,
                            int shift, int deff, uint64_t* cts_small);
/* centred mod switch, in place on small ciphertexts (count x (n+1)): half the sum of the mask words' rounding remainders comes off the
 * body, which halves the variance of the bootstrap's mod-switch error.  dctfhe_round_lut and dctfhe_session_run
 * apply it between every key switch and its bootstrap; dctfhe_keyswitch / dctfhe_pbs are the bare primitives. */
int dctfhe_modswitch_center(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, uint64_t* cts_small, size_t count);
int dctfhe_pbs(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* cts_small, size_t count,
               const int64_t* tables /* [ntab][2^w] */, int ntab, int w, const int32_t* table_idx /* may be NULL */,
               uint64_t* cts_out /* count x (D+1) */);
int dctfhe_round_lut(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int bit_tier, int tab_tier, const uint64_t* cts,
                     size_t count, int p, int r, const int64_t* tables, int ntab, int w,
                     const int32_t* table_idx, uint64_t* cts_out);
/* A table of w = 7 input bits is evaluated by a parity split: with t = 2 t' + b0 the index, one more one-bit step on
 * bit_tier takes b0 off the ciphertext, a second sign bootstrap of the same small ciphertext puts b0 into the padding bit of a copy, and
 * two 6-bit look-ups -- S[j] = (T[2j] + T[2j+1]) / 2 on tab_tier, Dt[j] = T[2j] - S[j] on tab_tier2, negated by the negacyclic rotation
 * when b0 = 1 -- sum to T[t].  Every pair T[2j] + T[2j+1] must be even.  dctfhe_round_lut splits w = 7 with tab_tier2 = tab_tier;
 * dctfhe_round_lut_split splits any w >= 2 when tab_tier2 >= 0 (and is dctfhe_round_lut without a split when tab_tier2 < 0). */
int dctfhe_round_lut_split(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int bit_tier, int tab_tier, int tab_tier2, const uint64_t* cts,
                           size_t count, int p, int r, const int64_t* tables, int ntab, int w, const int32_t* table_idx,
                           uint64_t* cts_out);
int dctfhe_conv2d(dctfhe_ctx* ctx, int D, const uint64_t* in, int batch, int Cin, int H, int W,
                  const int8_t* weight /* [Cout][Cin][KH][KW] */, int Cout, int KH, int KW, int stride, int pad,
                  uint64_t* out);

/* K2 one kernel at a time on host buffers (reference backbone.py:102 torch.add, :276 AvgPool2d, and the shift / offset that opens a
 * rounding chain): rows of `dim` mask words + body whose mask words from `deff` on count as zero -- the storage form of a session's
 * tensors, here exposed so that the streaming kernels can be checked at mixed effective dimensions outside a circuit.
 * add: out = a + b, dim_o >= max(deff_a, deff_b).  affine: the first nwords mask words of each inout row become a << shift, the body
 * (body << shift) + body_add, the words in between are LEFT AS THEY ARE.  sum_pool: KxK window sums, floor semantics (nn.AvgPool2d(K)
 * drops the border; the 1/K^2 lives in the next table). */
int dctfhe_add_rows(dctfhe_ctx* ctx, const uint64_t* a, int dim_a, int deff_a, const uint64_t* b, int dim_b, int deff_b, size_t count,
                    int dim_o, uint64_t* out);
int dctfhe_affine_rows(dctfhe_ctx* ctx, const uint64_t* a, int dim_a, int deff_a, size_t count, int nwords, int shift, uint64_t body_add,
                       int dim_o, uint64_t* inout);
int dctfhe_sum_pool_rows(dctfhe_ctx* ctx, const uint64_t* in /* [batch][C][H][W] rows */, int dim_in, int deff_in, int batch, int C, int H,
                         int W, int K, int dim_o, uint64_t* out /* [batch][C][H/K][W/K] rows */);
/* K1 on rows: dctfhe_conv2d as the session runs it, on input rows of dim_in mask words + body whose mask words from deff_in on count as
 * zero (and are not read) into output rows of dim_o >= deff_in mask words: words [deff_in, dim_o) are zero, the body is last.  The
 * matrix-core kernel is taken exactly when the session takes it (dim_o + 1 >= 32), the integer-VALU kernel otherwise.  dctfhe_conv2d is
 * this call with dim_in = deff_in = dim_o = D.  A launch whose batch x Ho x Wo output pixels (or whose output-channel blocks) exceed the
 * device's launch-grid limit is refused with a message that names both numbers. */
int dctfhe_conv2d_rows(dctfhe_ctx* ctx, const uint64_t* in /* [batch][Cin][H][W] rows of dim_in+1 */, int dim_in, int deff_in, int batch,
                       int Cin, int H, int W, const int8_t* weight /* [Cout][Cin][KH][KW] */, int Cout, int KH, int KW, int stride,
                       int pad, int dim_o, uint64_t* out /* [batch][Cout][Ho][Wo] rows of dim_o+1 */);
/* dctfhe_conv2d_rows for a window of its output: channels [c0, c1) only, 0 <= c0 < c1 <= Cout, into a buffer that holds the window and
 * nothing else.  The pixels go out in chunks of at most the device's launch-grid limit, so no pixel count is refused; c0 = 0, c1 = Cout
 * computes what dctfhe_conv2d_rows computes.  The same kernels and the same weight pack: a session under a memory budget runs its
 * convolutions through this path. */
int dctfhe_conv2d_rows_window(dctfhe_ctx* ctx, const uint64_t* in /* [batch][Cin][H][W] rows of dim_in+1 */, int dim_in, int deff_in,
                              int batch, int Cin, int H, int W, const int8_t* weight /* [Cout][Cin][KH][KW] */, int Cout, int KH, int KW,
                              int stride, int pad, int dim_o, int c0, int c1, uint64_t* out /* [batch][c1-c0][Ho][Wo] rows of dim_o+1 */);

/* ---- bounded device memory.  A slab group is a convolution and the maximal run of look-ups / max pools behind it
 * in which each op reads exactly the destination of the op before it and nothing else reads that destination.  Under a budget a session
 * holds `slab` channels of ONE image of a group's inner tensors at a time and walks the group slab by slab; the group's last destination
 * is written whole.  slab = channels: the undivided group, byte for byte what runs without a budget.  No output word depends on the cut.
 * The budget counts what a session allocates for itself: tensors, a max pool's level buffers and index maps, the parity work buffer, the
 * look-up scratch and the overflow flag -- NOT keys, circuit payloads or convolution packs.
 * dctfhe_memory_plan: host only (no context, no GPU), from a circuit blob, parameters (NULL: a clear-mode session) and batch.
 * budget_bytes = 0: no budget.  It starts undivided and, while the plan exceeds the budget, lowers by one channel the slab height of the
 * group that holds the largest inner tensor; it refuses, naming an op and the bytes of the smallest plan, when one channel at a time
 * everywhere still does not fit.
 * dctfhe_session_set_memory_budget: the same planner on a session, before its first run (an uploaded input stays where it is); refused once
 * the session has run, on a sharded session and while the margin audit is on.  A budget the planner refuses leaves the session as it
 * was: nothing is freed before the plan stands.  (An allocation that then fails on the device does not: destroy that session.)
 * dctfhe_session_run_span refuses a span that begins or ends inside a divided group.  dctfhe_session_memory_plan: the plan in force. */
#define DCTFHE_MAX_SLAB_GROUPS 64
typedef struct {
  uint64_t bytes_undivided, bytes_planned, budget_bytes;
  uint64_t bytes_buffers, bytes_maps, bytes_scratch;      /* of bytes_planned (dctfhe_memory_plan; 0 from a session) */
  int32_t n_groups, reserved;
  int32_t first_op[DCTFHE_MAX_SLAB_GROUPS], end_op[DCTFHE_MAX_SLAB_GROUPS];      /* ops [first_op, end_op) */
  int32_t channels[DCTFHE_MAX_SLAB_GROUPS], slab[DCTFHE_MAX_SLAB_GROUPS];        /* the group's channels; how many exist at a time */
} dctfhe_mem_plan;
int dctfhe_memory_plan(const void* blob, size_t size, const dctfhe_params* params, int batch, size_t budget_bytes, dctfhe_mem_plan* out);
int dctfhe_session_set_memory_budget(dctfhe_session* s, size_t bytes);
int dctfhe_session_memory_plan(dctfhe_session* s, dctfhe_mem_plan* out);
/* The plan at slab heights given by hand, one per slab group in the order of the plan record, each from 1 to the group's channels, under
 * the rules of dctfhe_session_set_memory_budget; it counts as a budget of exactly the plan's bytes.  For tests and experiments: which
 * heights fit a budget is the planner's business. */
int dctfhe_session_set_slab_heights(dctfhe_session* s, const int32_t* slab, int n_groups);

/* max pool (circuit op 5), one piece at a time on host buffers.
 * keyswitch_diff: key switch of cts[ia[c]] - cts[ib[c]] (count rows of D + 1 words and count index pairs, indices < count), shifted
 * left by `shift`, body_add on the body; deff as dctfhe_keyswitch_prefix.  Output: count small ciphertexts of `tier`.
 * max_pool_rows: MaxPool2d(k, s, p) (1 <= k <= 32, 0 <= p <= k/2, floor mode, out-of-range taps ignored) as the session runs it:
 * row pass then column pass, each a tree of pairwise maxima b + relu(a - b) with one bootstrap of the signed p_d-bit `table` (2^p_d
 * entries, relu of the centred differences) on `tier`.  Inputs carry value * 2^(63 - p_d); outputs rows of dim_o + 1 words,
 * dim_o >= max(deff_in, ring of the tier).  keys == NULL: the clear form, one word per element, the maximum of the words read as
 * signed int64 (dim_in, deff_in, dim_o, tier and table unused). */
int dctfhe_keyswitch_diff(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* cts, size_t count, const int32_t* ia,
                          const int32_t* ib, int shift, uint64_t body_add, int deff, uint64_t* out_small);
int dctfhe_max_pool_rows(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* in /* [batch][C][H][W] rows */, int dim_in,
                         int deff_in, int batch, int C, int H, int W, int k, int s, int p, int p_d, const int64_t* table, int dim_o,
                         uint64_t* out /* [batch][C][Ho][Wo] rows */);

/* The seams a look-up site is stitched from, one launch at a time on host buffers (tests).  Nothing stays on the device afterwards.
 * pbs_rows: dctfhe_pbs in the write-back modes the library itself launches.  rows_io holds n_rows rows of dim_out + 1 words (dim_out >= the
 * tier's ring k N, at most 2^16); the bootstraps of the count small ciphertexts go to rows [row0, row0 + count).  accumulate = 0: mask words
 * [0, k N) and the body are stored, words [k N, dim_out) zeroed; accumulate != 0: the result is ADDED to mask words [0, k N) and to the body,
 * the words in between are left as they are.  body_add goes on the body in both modes.  Rows outside [row0, row0 + count) come back as they
 * went in.  table_idx == NULL: ciphertext c takes table ((e_offset + c) / hw) % nchan of the first nchan tables (nchan = 1: table 0).
 * Refused: row0 + count > n_rows, hw < 1, nchan < 1, nchan > ntab, a table_idx entry outside [0, ntab), w > logN - 1, dim_out < k N.
 * keyswitch_sum: key switch of rows_a[c] + rows_b[c] (rows of dim_a + 1 and dim_b + 1 words, 1 <= dim_a <= D; a mask word of b at or beyond
 * dim_b counts as zero), shifted left by `shift`, body_add on the body: what the second look-up of a parity split reads.  deff as
 * dctfhe_keyswitch_prefix, for the SUM: 0 <= deff <= dim_a.
 * acc_rows: o += b on the first nwords mask words and on the body of every row (rows of dim_o + 1 and dim_b + 1 words, nwords <=
 * min(dim_o, dim_b)); the other words of o stay.
 * gather_rows: dst[r] = row map[r] of src (n_src rows of dim_s + 1 words whose mask words from deff_s on count as zero) as a row of
 * dim_d + 1 >= deff_s + 1 words: words [deff_s, dim_d) zero, the body last.  A map entry outside [0, n_src) is refused. */
int dctfhe_pbs_rows(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* cts_small, size_t count,
                    const int64_t* tables /* [ntab][2^w] */, int ntab, int w, const int32_t* table_idx /* may be NULL */, int hw, int nchan,
                    size_t e_offset, uint64_t* rows_io /* n_rows x (dim_out+1) */, size_t n_rows, size_t row0, int dim_out, int accumulate,
                    uint64_t body_add);
int dctfhe_keyswitch_sum(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* rows_a /* count x (dim_a+1) */, int dim_a,
                         const uint64_t* rows_b /* count x (dim_b+1) */, int dim_b, size_t count, int shift, uint64_t body_add, int deff,
                         uint64_t* cts_small /* count x (n+1) */);
int dctfhe_acc_rows(dctfhe_ctx* ctx, uint64_t* o_io /* count x (dim_o+1) */, int dim_o, const uint64_t* b /* count x (dim_b+1) */, int dim_b,
                    size_t count, int nwords);
int dctfhe_gather_rows(dctfhe_ctx* ctx, const uint64_t* src /* n_src x (dim_s+1) */, int dim_s, int deff_s, size_t n_src, const int32_t* map,
                       size_t count, int dim_d, uint64_t* dst /* count x (dim_d+1) */);

/* K10, client side, plaintext: the DCT front-end of reference data/cvfunctional.py:37-74 + data/cvtransforms.py:56-64,117-208 on
 * uint8 planes (luma [batch][fs*S][fs*S]; two chroma slots [batch][fs*Sc][fs*Sc], Sc = S/2 for the 4:2:0 paths or S):
 * blockwise orthonormal DCT-II of (pixel - 128), only the kept coefficients idx_* (row-major u*fs+v), chroma grids
 * bilinearly up-sampled to S x S, channels concatenated luma | slot 1 | slot 2, (x - mean[c]) / std[c] in f32.
 * round_coeffs != 0: the JPEG-domain (filter 8) path's integer coefficient planes.  out: float32 [batch][ny+n1+n2][S][S]. */
int dctfhe_dct_frontend(dctfhe_ctx* ctx, const uint8_t* y, const uint8_t* c1, const uint8_t* c2, int batch, int S, int Sc, int fs,
                        const int32_t* idx_y, int ny, const int32_t* idx_c1, int n1, const int32_t* idx_c2, int n2,
                        const float* mean, const float* stdv, int round_coeffs, float* out);

/* host-only validators (no GPU): parameter set / circuit blob well-formed?  0 or -1 with dctfhe_last_error() */
int dctfhe_params_check(const dctfhe_params* params);
/* Circuit op types: 1 conv2d, 2 add, 3 sum_pool, 4 look-up, 5 max pool.  Max-pool record: ip[0..2] = k, stride, padding; ip[3] = shift
 * of the differences to 63 - p_d; ip[4] = tier of the relu table; ip[5] = p_d (signed difference bits); ip[6] = 1 table; ip[10] =
 * effective dimension of the input; lp[0] = body offset of the differences (2^62); payload: 2^p_d int64 entries relu(d) * 2^e.
 * The output keeps the input's encoding e.
 * Look-up record: ip[0..3] = p, r, w, shift; ip[4] = table tier; ip[5] = bit tier; ip[6] = tables; ip[7] / ip[8], ip[11] = hand-over of the
 * one-bit steps to the cheaper bit tiers; ip[10] = effective dimension of the input; ip[9] = mode: 0 exact rounding, 1 approximate
 * rounding, 2 parity split with both look-ups on ip[4], 3 parity split with the second look-up on the tier whose key-switch key ip[4]
 * shares (its quiet twin).  A split record keeps the whole 2^w-entry tables; every other value of ip[9] is rejected. */
int dctfhe_circuit_validate(const void* blob, size_t size);

/* R1: load a compiled circuit description (built by dctfhe.compile, format in DESIGN.md section 4). */
int dctfhe_circuit_load(dctfhe_ctx* ctx, const void* blob, size_t size, dctfhe_circuit** out);
int dctfhe_circuit_destroy(dctfhe_circuit* circ);
int dctfhe_circuit_stats(dctfhe_circuit* circ, const dctfhe_params* params, dctfhe_stats* out);
int dctfhe_circuit_io(dctfhe_circuit* circ, int64_t* n_in_per_image, int64_t* n_out_per_image);

/* R4: evaluate the circuit on a batch of images.  A session owns the device tensors and needs the EVALUATION keys only. */
int dctfhe_session_create(dctfhe_ctx* ctx, dctfhe_circuit* circ, dctfhe_eval_keys* keys /* NULL: clear mode */,
                          int batch, dctfhe_session** out);
int dctfhe_session_destroy(dctfhe_session* s);
int dctfhe_session_upload(dctfhe_session* s, const uint64_t* cts_in /* batch x n_in x (D+1); clear: x 1 */);
/* compact wire form: host rows of dim mask words + body (clear-mode sessions ignore dim).  upload: any 1 <= dim <= D; words a row lacks
 * count as zero, words beyond the input's effective dimension must BE zero (checked).  download: dim >= the output's effective dimension.
 * dctfhe_session_dims reports the two effective dimensions (input: what upload keeps; output: the least download accepts). */
int dctfhe_session_upload_rows(dctfhe_session* s, const uint64_t* cts_in /* batch x n_in x (dim+1) */, int dim);
/* seeded inputs (dctfhe_encrypt_seeded): only the bodies are copied to the device; count must be batch x n_in, 1 <= dim_eff <= the input's
 * effective dimension (in_dim of dctfhe_session_dims); encrypted sessions only.  The stored input equals upload_rows of the expanded rows. */
int dctfhe_session_upload_seeded(dctfhe_session* s, const uint8_t mask_key[32], uint64_t stream, int dim_eff, const uint64_t* bodies, size_t count);
int dctfhe_session_download_rows(dctfhe_session* s, uint64_t* cts_out /* batch x n_out x (dim+1) */, int dim);
int dctfhe_session_dims(dctfhe_session* s, int* in_dim, int* out_dim);
/* synchronous.  The uploaded input stays resident: run may be called again without a fresh upload (same result). */
int dctfhe_session_run(dctfhe_session* s, dctfhe_timing* timing /* may be NULL */);
/* clear-mode sessions (keys == NULL) only: `simulate` with the noise model.  sigma_per_op[i] (fraction of the torus, 0 for
 * ops that are not look-ups) is added at the input of op i's table look-up, fresh draws every run; n_ops = 0 switches it off.
 * The definition (tests/simulate_ref.py is its numpy twin, compared word for word).  All words mod 2^64.
 *   key      the dctfhe_rng_host key of words (seed & 0xffffffff, seed >> 32, 0x73696d75, 0, 0, 0, 0, 0), little-endian
 *   draw     gauss(stream, idx, sigma) = (int64) rint(x 2^64), x = g sigma - rint(g sigma) (a torus element: exact, the identity for
 *            |g sigma| < 1/2, defined for every sigma), g = sqrt(-2 ln u1) cospi(2 u2), u1 = ((word(2 idx) >> 11) + 1) 2^-53,
 *            u2 = (word(2 idx + 1) >> 11) 2^-53; 0 where sigma <= 0
 *   look-up  noisy_lookup(centre, w, T, idx, sigma): pos = centre + gauss + 2^(62-w); entry (pos >> (63-w)) & (2^w - 1) of T, negated when
 *            bit 63 of pos is set
 *   run R    counts, from the session's creation, the passes that reached the circuit's last op (a run_span that stops early does not
 *            advance it; set_noise and uploads do not reset it)
 *   OP_LUT i stream 0x51D0000 + (R << 12) + i; element g = its number in the whole [B][C][H][W] tensor, whatever slice or slab computes
 *            it; v = (x << shift) + body_add, + 2^(63-p+r-1) when r > 0 except on an approximate site with sigma > 0; overflow when bit
 *            63 of v is set; idx = the top w bits of v under the padding bit; table (g / hw) % ntab.  sigma = 0: T[idx], never negated.
 *            Exact: centre idx << (63-w), draw g.  Approximate, r > 0: centre v + 2^(62-p), draw g.  Parity split: S[j] = ((T[2j] +
 *            T[2j+1]) mod 2^64) >> 1, Dt[j] = T[2j] - S[j], centre (idx >> 1) << (64-w); S at width w-1, draw 2g, sigma, plus Dt with
 *            (idx & 1) << 63 added to the centre, draw 2g+1, sigma2 (set_noise_split; sigma where 0 or absent)
 *   OP_MAXPOOL i  streams P = 2^40 | ((0x51D0000 + (R << 12) + i) << 1) for the row pass, P + 1 for the column pass; an output folds its
 *            in-range taps in tap order: m = x at the first, then d = ((x - m) << shift) + body_add and
 *            m += noisy_lookup(top p_d bits of d, p_d, relu table, e 64 + taken, sigma), e the output's number in the whole pass, taken
 *            the taps folded so far.  sigma = 0: the signed-word maximum */
int dctfhe_session_set_noise(dctfhe_session* s, uint64_t seed, const double* sigma_per_op, int n_ops);
/* parity-split look-ups run two table bootstraps: sigma_per_op is sampled at the first, sigma2_per_op[i] (> 0) at the second, whose input
 * also carries the parity bootstrap's output; without this call, or where the entry is 0, the second takes sigma_per_op[i] too */
int dctfhe_session_set_noise_split(dctfhe_session* s, const double* sigma2_per_op, int n_ops);
int dctfhe_session_download(dctfhe_session* s, uint64_t* cts_out /* batch x n_out x (D+1) */);

/* PACKED result ciphertexts.  A result carries a signed out_bits-bit value plus padding: its decode margin is
 * 2^-(out_bits + 3), far wider than a 64-bit word resolves.  The server therefore key-switches each result to the small key of `tier`
 * with the key-switch key it already holds (the tier's own, or the one it shares: ksk_share) -- shift 0, the sum over the first deff key
 * rows, exactly the n + 1 words dctfhe_keyswitch_prefix(tier, shift = 0, deff) returns -- and keeps the top 16 bits of every word:
 *     row[j] = (uint16_t)((small[j] + 2^47) >> 48),  j = 0 .. n
 * (round to nearest on the 2^-16 torus grid, a tie goes up, a carry out of the top wraps to 0; plain rounding, not centred).  Host form:
 * count x (n + 1) little-endian uint16_t, rows contiguous (odd row length for even n: rows are not 4-byte aligned).  2 (n + 1) bytes per
 * result instead of 8 (out_dim + 1).  Which tier keeps the result inside its margin is the compiler's call (dctfhe.compile
 * output_compaction); no new key material is involved.
 *
 * dctfhe_session_download_packed: the session's outputs in that form.  Runs at download time with the session's look-up scratch, in chunks
 * of at most 16384 ciphertexts; dctfhe_session_run and dctfhe_timing do not see it.  Encrypted sessions only. */
int dctfhe_session_download_packed(dctfhe_session* s, int tier, uint16_t* rows /* batch x n_out x (n+1) */);
/* The primitive on host rows of dim mask words + body (words from deff on count as zero; deff = 0: dim), 1 <= dim <= D, 0 <= deff <= dim,
 * with dctfhe_keyswitch_prefix's contract for deff: the caller knows every mask word from deff on to be zero. */
int dctfhe_keyswitch_pack(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, const uint64_t* cts /* count x (dim+1) */, size_t count, int dim,
                          int deff, uint16_t* rows /* count x (n+1) */);
/* CLIENT: phases of packed rows under the first n bits of the small key (n = the tier's small dimension, 1 <= n <= n_max):
 *     phase16 = (row[n] - sum_{j<n} s_j row[j]) mod 2^16,  returned as (uint64_t)phase16 << 48
 * so that whatever decodes dctfhe_decrypt's phases decodes these. */
int dctfhe_decrypt_packed(dctfhe_ctx* ctx, dctfhe_client_key* client, int n, const uint16_t* rows, size_t count, uint64_t* phases);

/* RING-PACKED result ciphertexts: up to N_p = 2^logN results travel in ONE GLWE ciphertext, 2 (N_p + m) bytes
 * for m results instead of 2 m (n + 1).  Opt-in; it needs key material of its own, the PACKING KEY, which the client makes once.
 *
 * Spec: ring size N_p = 2^logN (5 <= logN <= 12, N_p <= D), l_p gadget levels of beta_p bits (l_p >= 1, 1 <= beta_p <= 32: digits are
 * kept in 32 bits; l_p beta_p <= 63), noise std sigma_p (fraction of the torus).  dctfhe.params default_pack_spec: logN 11, one level of
 * 16 bits -- the 16-bit rounding below already costs more than the second level would save.
 * Ring key: Z(X) = sum_{c < N_p} S[c] X^c, the first N_p bits of the big key as ONE polynomial (k = 1; the nested-prefix rule of every
 * tier's GLWE key).
 * Packing key: for every small-key bit j < n_max and level lev < l_p one GLWE row (A, B), B = A Z + E + s_j 2^(64 - beta_p (lev + 1)) X^0,
 * negacyclic, mod 2^64.  With row r = j l_p + lev and the spec's generator stream
 *     R = 1 << 63 | ((bits(sigma_p) * 0x9E3779B97F4A7C15 mod 2^64) ^ (logN << 24 | l_p << 16 | beta_p << 8)) & 0x7FFFFFFFFFFFFFFE
 * (bits: the IEEE-754 double as a u64; nothing else draws from R or R + 1: every other stream id of the key-material generator keys is below 2^17, and encryptions use the per-handle keys)
 * mask word A[c] is generator word (pub, R, r N_p + c) of the client's PUBLIC generator key and E[c] the Gaussian draw
 * (sec, R + 1, r N_p + c) of the secret one, as for the bootstrap keys.  sigma_p is part of R because the Gaussian draw scales with it:
 * exports of one client key at two sigma_p never share a draw.
 * Blob (seeded form only, little-endian): u32 magic 'DRPK', u32 version 1, i32 logN, l_p, beta_p, n_max, f64 sigma_p, u64 total bytes;
 * the 32-byte public generator key; n_max l_p N_p body words B (u64).  Import regenerates every A on the GPU.  Small keys are prefixes of
 * one small key, so one packing key serves every tier: tier t uses its first n_t l_p rows.  13 MB at the default spec and n_max = 800.
 *
 * Pack (server): results are key-switched to the small key of `tier` exactly as dctfhe_keyswitch_prefix(tier, shift 0, deff) does, taken in
 * order in groups of N_p (result i of a group in slot i; the last group may hold m < N_p), and per group
 *     acc = (0, sum_i b_i X^i) - sum_i sum_{j<n} sum_lev dig_lev(a_ij) X^i PK[j][lev]
 * with dig the closest-representable signed decomposition (digits in [-B/2, B/2), the top carry dropped) and X^i the negacyclic shift.
 * A key row's message is a constant polynomial, so coefficient i of acc's phase is result i's phase and nothing else.
 * Wire form: per group the N_p mask words, then the first m body words, each (uint16_t)((w + 2^47) >> 48) as in the packed rows above;
 * groups contiguous, little-endian: dctfhe_ring_words(logN, count) = groups N_p + count words.
 * Decrypt (client): phase16_i = (B16[i] - (A16 Z)[i]) mod 2^16, negacyclic, returned as (uint64_t)phase16 << 48.
 *
 * pack_key_export: CLIENT; buf == NULL: size query.  Refused: N_p > D, l_p beta_p > 63, a spec outside the ranges above.
 * pack_key_import: SERVER; refused: a blob of the wrong magic, version or length.  pack_key_export_rows: test view of the expanded key,
 * [n_max][l_p][2][N_p] (A then B).  ring_pack: the primitive on host small ciphertexts count x (n + 1), 1 <= n <= n_max of the key.
 * session_download_ring: the session's outputs in that form; key-switched in chunks like dctfhe_session_download_packed, packed at download
 * time -- dctfhe_session_run and dctfhe_timing do not see it.  Refused: a clear-mode session, a tier whose n exceeds the key's n_max, a packing key imported on another context. */
typedef struct dctfhe_pack_key dctfhe_pack_key;       /* SERVER: the expanded packing key (public material) */
int dctfhe_pack_key_export(dctfhe_client_key* client, int logN, int l_p, int beta_p, double sigma_p, void* buf, size_t capacity, size_t* size);
int dctfhe_pack_key_import(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_pack_key** out);
int dctfhe_pack_key_destroy(dctfhe_pack_key* key);
int dctfhe_pack_key_info(dctfhe_pack_key* key, int* logN, int* l_p, int* beta_p, int* n_max, double* sigma_p /* each may be NULL */);
int dctfhe_pack_key_export_rows(dctfhe_pack_key* key, uint64_t* out /* n_max x l_p x 2 x N_p */);
size_t dctfhe_ring_words(int logN, size_t count);
int dctfhe_ring_pack(dctfhe_ctx* ctx, dctfhe_pack_key* key, const uint64_t* cts_small /* count x (n+1) */, size_t count, int n,
                     uint16_t* out /* dctfhe_ring_words */);
int dctfhe_session_download_ring(dctfhe_session* s, int tier, dctfhe_pack_key* key, uint16_t* out /* dctfhe_ring_words of batch x n_out */);
int dctfhe_decrypt_ring(dctfhe_ctx* ctx, dctfhe_client_key* client, int logN, const uint16_t* words, size_t count, uint64_t* phases);

/* PUBLIC-KEY INPUTS: a party that holds no secret encrypts up to N_e = 2^logN input phases into ONE GLWE
 * ciphertext with a compact public key; the server extracts them as LWE rows.  16 bytes per input in full groups.  Opt-in.
 *
 * Spec: ring N_e = 2^logN, 5 <= logN <= 12, N_e <= input_dim (D where input_dim is 0): the ring key Z(X) = sum_{c < N_e} S[c] X^c is
 * the first N_e bits of the big key (the ring key of the ring-packed results above), and a circuit's input tensor keeps only input_dim
 * mask words.  Noise std sigma (fraction of the torus) for the key row and for the encryptor's e1, e2.  dctfhe.params
 * default_public_input_spec: logN 11, sigma_min(2048).
 * Public key: ONE GLWE zero row (A, B), B = A Z + E, negacyclic, mod 2^64.  With the spec's generator stream
 *     P = 1 << 62 | ((bits(sigma) * 0x9E3779B97F4A7C15 mod 2^64) ^ (logN << 24)) & 0x3FFFFFFFFFFFFFFE
 * (bits: the IEEE-754 double as a u64) A[c] is generator word (pub, P, c) of the client's PUBLIC generator key and E[c] the Gaussian draw
 * (sec, P + 1, c) of the secret one.  Bit 62 set and bit 63 clear: P and P + 1 meet no packing-key stream R, R + 1 (bit 63 set) and no
 * other id of these generator keys (all below 2^17); sigma and logN are part of P for the reason given at R.
 * Blob (seeded form only, little-endian): u32 magic 'DPBK', u32 version 1, i32 logN, i32 0, f64 sigma, u64 total bytes; the 32-byte public
 * generator key; N_e body words B (u64): 16 448 bytes at logN 11.  Import regenerates A on the GPU.
 *
 * Encryption, per group of m <= N_e phases (phase i of a call: group i / N_e, slot i mod N_e): u uniform in {0,1}^N_e, e1 Gaussian(sigma)
 * on N_e coefficients, e2 on m;  C_a = A u + e1;  C_b[i] = (B u)[i] + e2[i] + phase_i, i < m.  Coefficient i of C_b - C_a Z is
 * phase_i + (E u + e2 - e1 Z)[i].
 * Wire form: per group its N_e mask words, then its first m body words, u64 little-endian, groups contiguous:
 * dctfhe_public_words(logN, count) = groups N_e + count words (the layout of the ring-packed results at full width).
 * Randomness: the encryptor holds NO client key.  public_key_import draws a 32-byte generator key from the OS (getrandom) and keeps a call
 * counter; call c = 0, 1, ... draws u[x] = the top bit of generator word (key, 3 c, x), e1[x] = the Gaussian draw (key, 3 c + 1, x) for
 * x < groups N_e (x = group N_e + coefficient) and e2[x] = the draw (key, 3 c + 2, x) for x < count: no two calls and no two handles share
 * a draw.  public_key_set_encrypt_seed fixes the key and restarts the counter -- reproducible tests only; public_key_draws regenerates
 * the draws of one call (u one byte per bit, e1, e2 signed torus words), so a reference can rebuild the ciphertext bit for bit.
 * Extraction (server): slot i of a group is the LWE row a_j = C_a[i - j] (j <= i), a_j = -C_a[N_e + i - j] (i < j < N_e), a_j = 0
 * (N_e <= j), body C_b[i], under the first N_e bits of the big key.
 *
 * public_key_export: CLIENT; buf == NULL: size query.  Refused: logN outside [5, 12], N_e > input_dim (or D), sigma outside [0, 1).
 * public_key_import: ENCRYPTOR; refused: a blob of the wrong magic, version or length.  public_key_export_rows: test view, [2][N_e].
 * encrypt_public / ring_extract / public_key_draws refuse count == 0; ring_extract needs dim >= N_e and writes count rows of dim + 1
 * words; session_upload_public writes the rows straight into the session's input tensor and refuses a clear-mode session,
 * count != batch x n_in and N_e beyond the mask words the circuit's input keeps. */
typedef struct dctfhe_public_key dctfhe_public_key;   /* ENCRYPTOR: the expanded public key and the handle's own generator key */
int dctfhe_public_key_export(dctfhe_client_key* client, int logN, double sigma, void* buf, size_t capacity, size_t* size);
int dctfhe_public_key_import(dctfhe_ctx* ctx, const void* buf, size_t size, dctfhe_public_key** out);
int dctfhe_public_key_destroy(dctfhe_public_key* key);
int dctfhe_public_key_info(dctfhe_public_key* key, int* logN, double* sigma /* each may be NULL */);
int dctfhe_public_key_export_rows(dctfhe_public_key* key, uint64_t* out /* 2 x N_e */);
int dctfhe_public_key_set_encrypt_seed(dctfhe_public_key* key, const uint8_t* seed32);
int dctfhe_public_key_draws(dctfhe_public_key* key, uint64_t call, size_t count, uint8_t* u /* groups x N_e */, int64_t* e1 /* groups x N_e */,
                            int64_t* e2 /* count */);
size_t dctfhe_public_words(int logN, size_t count);
int dctfhe_encrypt_public(dctfhe_ctx* ctx, dctfhe_public_key* key, const uint64_t* phases, size_t count, uint64_t* words_out /* dctfhe_public_words */);
int dctfhe_ring_extract(dctfhe_ctx* ctx, int logN, const uint64_t* words, size_t count, int dim, uint64_t* rows_out /* count x (dim+1) */);
int dctfhe_session_upload_public(dctfhe_session* s, int logN, const uint64_t* words, size_t count);

/* MARGIN AUDIT: the decision noise of every bootstrap that has a key switch of its own, measured in a real run.
 * A development and assurance tool: it needs the client's SECRET key, so it is never a server path.
 *
 * Take a small ciphertext (a_0 .. a_{n-1}, b) of a tier with ring N = 2^logN, key-switched and mod-switched (centred), about to be
 * bootstrapped with a table of w input bits (w = 0: a one-bit step).  With lv(x) = ((x >> (62 - logN)) + 1) >> 1, the bootstrap's own
 * rounding to 2N levels,
 *     phi = (lv(b) - sum_{i<n} s_i lv(a_i)) mod 2N          the switched phase under the first n bits of the small key
 *     G = 2^(logN - w), h = G / 2                           box width and half-box in levels; boxes are centred on the multiples of G
 *     e = ((phi + h) mod G) - h,  -h <= e < h               the signed distance from the centre of the box the bootstrap will read
 * While the run is correct, e is exactly the noise the compiler prices at that decision (dctfhe.compile margin_model).  It is an
 * integer: every statistic below is exact and does not depend on the order of summation.
 * A WRONG SECRET CANNOT BE DETECTED: the statistics then read as uniform noise (max_abs near half_box, a flat histogram). */
#define DCTFHE_MARGIN_BINS 16
typedef struct {
  int32_t op, entry;          /* circuit op; index among that op's bootstraps that have a key switch of their own (-1, -1: a primitive call) */
  int32_t tier, table_bits;   /* tier -1: the host form */
  int32_t half_box, max_abs;  /* h and the largest |e|, in levels of the tier's 2N */
  int64_t count, sum;         /* decisions probed; sum of e */
  uint64_t sum_sq;            /* sum of e^2 */
  int64_t hist[DCTFHE_MARGIN_BINS];   /* bin min(15, 16 |e| / half_box) */
} dctfhe_margin_stats;

/* no GPU (like dctfhe_rng_host): the definition, on host rows of n + 1 words.  small_key: n bytes, 0 or 1.  1 <= n, 1 <= logN <= 31,
 * 0 <= table_bits < logN.  err (count values) and stats may each be NULL. */
int dctfhe_margin_probe_host(const uint8_t* small_key, int n, int logN, const uint64_t* cts_small, size_t count,
                             int table_bits, int32_t* err, dctfhe_margin_stats* stats);
/* the session's kernel on host rows of `tier`, key bits from the client handle */
int dctfhe_margin_probe(dctfhe_ctx* ctx, dctfhe_client_key* client, int tier, const uint64_t* cts_small, size_t count,
                        int table_bits, int32_t* err, dctfhe_margin_stats* stats);
/* encrypted sessions: client != NULL turns the audit on for the following runs, NULL turns it off.  The session copies the small key's
 * n_max bytes into a device buffer of its own (cleared before it is freed, on destroy and when the audit is turned off): the client
 * handle may be destroyed afterwards.  While the audit is on, every bootstrap launch with a key switch of its own is followed by one
 * small streaming kernel over its small ciphertexts; dctfhe_timing.total_ms of such a run includes them (the per-category spans do
 * not).  Off -- the default -- a run launches exactly what it did before this call existed.
 * Refused: a clear-mode session; a client whose D, n_max, tier count or any tier's n, k, logN differ from the session's keys; a circuit
 * with an approximate-rounding site (the low bits ride along there: e is not noise). */
int dctfhe_session_set_audit(dctfhe_session* s, dctfhe_client_key* client);
/* The slots of the last run: one per (op, bootstrap with a key switch of its own), ops in circuit order, a look-up's one-bit steps,
 * then for a parity split its second look-up, then its table; a max pool has one slot over all its levels.  (The parity bootstrap
 * reuses the last step's small ciphertext: no slot.  The order is that of the enumeration, not of execution.)  The chunks of a site
 * accumulate into its slot; every dctfhe_session_run starts from zeroed slots.  out == NULL: only *n_slots is written; audit off:
 * *n_slots = 0.  capacity < *n_slots is refused. */
int dctfhe_session_audit(dctfhe_session* s, dctfhe_margin_stats* out, int capacity, int* n_slots);

/* SHARDED LOOK-UP SITES: one image over `parts` sessions, one per GPU.  Opt-in; the default (0, 1) is the plain run.
 *
 * Partition rule (every element-wise tensor; a "row" is one ciphertext of the flat [B][C][H][W] order): with q = rows / parts and
 * r = rows % parts, part p owns the q + (p < r) consecutive rows from p q + min(p, r).  Empty parts are legal (rows < parts).
 * shard_rows is host-only (no GPU); refused: parts < 1, parts > 64, part outside [0, parts).
 *
 * Every tensor of a session is WHOLE or SLICED (only this part's rows are valid).  The input is whole after an upload.  Look-ups and adds
 * run on this part's rows only, read the same rows of their sources (a whole source may feed them) and leave their destination sliced.
 * Convolutions, sum pools, max pools and every download need whole sources; they are computed in full on every part (a max pool's own
 * bootstraps included) and leave whole destinations.  Nothing on the server side is random, so a row does not depend on the launch it
 * was computed in: a sharded run reproduces the unsharded output ciphertexts word for word.
 *
 * set_shard: refused once the session has run, and while the margin audit is on (the audit stays unsharded; set_audit likewise refuses
 * a sharded session).
 * run_span: ops [first_op, end_op) in order, synchronous like dctfhe_session_run; an op that needs a whole tensor which is sliced is
 * refused with its number and the tensor's.  dctfhe_session_run is run_span over the whole circuit, for every (part, parts).
 * shard_plan: the exchange points, in op order: one entry per sliced tensor that a whole-needing op or the download reads, placed after
 * the op that writes the tensor.  It depends on the circuit only.  after_op / tensor == NULL: only *n is written; capacity < *n is refused.
 * At an entry the caller brings every part's rows of `tensor` into every session (session_tensor: the device pointer, the stored row
 * stride in words and the row count; between processes a broadcast per part) and then calls mark_whole.
 * copy_rows: rows [first, first + count) of `tensor` from src to dst, device to device, on dst's stream after src's work -- the loopback
 * that lets one process and one GPU run all parts.  Refused: sessions of different circuits, batches or modes, rows out of range. */
int dctfhe_shard_rows(size_t rows, int parts, int part, size_t* first, size_t* count);
int dctfhe_session_set_shard(dctfhe_session* s, int part, int parts);
int dctfhe_session_run_span(dctfhe_session* s, int first_op, int end_op, dctfhe_timing* timing /* may be NULL */);
int dctfhe_session_shard_plan(dctfhe_session* s, int32_t* after_op, int32_t* tensor, int capacity, int* n);
int dctfhe_session_tensor(dctfhe_session* s, int tensor, void** dev, size_t* row_words, size_t* rows);
int dctfhe_session_mark_whole(dctfhe_session* s, int tensor);
int dctfhe_session_copy_rows(dctfhe_session* dst, dctfhe_session* src, int tensor, size_t first, size_t count);

/* Divided max pools: opt-in on top of set_shard.  A pool's outputs read small windows and its tree of pairwise
 * maxima is driven by host-built index maps, so part p computes only its own outputs -- the rows dctfhe_shard_rows gives it over the flat
 * [B][C][Ho][Wo] order, the rows the look-up behind the pool then reads -- and produces the words of the undivided run.
 * shard_pool (host-only, no GPU): the partition of one pool.  (out_first, out_count): the part's output rows.  Its intermediates are the
 * row-pass results (b, c, y, xo) under the column windows of these outputs; the row pass computes only those, and a part recomputes the
 * halo it shares with a neighbour instead of receiving it.  (in_first, in_count): the smallest contiguous range of source rows [B][C][H][W]
 * that holds every tap of every owned window (a superset of the taps).  pairs: the pairwise maxima (bootstraps) the part runs; every
 * output and intermediate goes through the pairings of the undivided tree (late pairing, level count of the whole pass).  An empty part
 * has in_count = 0 and pairs = 0.  parts = 1 is the undivided op as dctfhe_session_run executes it: the whole source, every row-pass result.
 * set_shard_pool: on != 0 -> OP_MAXPOOL runs on the part's outputs and leaves its destination sliced; the pools' trees, level buffers and
 * clear-mode intermediates are planned again for the part (an uploaded input stays).  Refused without a prior set_shard, once the session
 * has run, and while the margin audit is on; set_shard is refused while it is on.  Off (the default): nothing changes.
 * mark_rows: the caller has brought rows [first, first + count) of `tensor` in.  A sliced tensor holds its own part's rows and what was
 * marked since it was written; once that is every row it is whole.  A divided pool runs when its need range is held, and run_span names
 * op, tensor and the first missing rows otherwise.  mark_whole stays as it is.
 * shard_plan_rows: the entries of shard_plan with a row range each: the need range of this session's part for a tensor that one divided
 * pool reads, (0, rows) for every other entry.  With the pools divided the entries are those of a circuit whose pools leave their
 * destination sliced (shard_plan answers likewise); without, shard_plan's with (0, rows).
 * pool_pairs: the pairwise maxima the last run of max-pool op `op` sent to the bootstrap (0 before a run, for an empty part and in clear
 * mode, which runs no bootstraps). */
int dctfhe_shard_pool(int batch, int C, int H, int W, int k, int s, int pad, int parts, int part, size_t* out_first, size_t* out_count,
                      size_t* in_first, size_t* in_count, size_t* pairs);
int dctfhe_session_set_shard_pool(dctfhe_session* s, int on);
int dctfhe_session_mark_rows(dctfhe_session* s, int tensor, size_t first, size_t count);
int dctfhe_session_shard_plan_rows(dctfhe_session* s, int32_t* after_op, int32_t* tensor, size_t* first, size_t* count, int capacity, int* n);
int dctfhe_session_pool_pairs(dctfhe_session* s, int op, size_t* pairs);

/* f64 FMA peak micro-benchmark (TFLOP/s) used to price the blind-rotate kernel in bench.py. */
int dctfhe_fp64_peak(dctfhe_ctx* ctx, double* tflops);
/* stand-alone timing of the blind-rotate kernel: count ciphertexts of tier `tier`, average ms per launch */
int dctfhe_bench_pbs(dctfhe_ctx* ctx, dctfhe_eval_keys* keys, int tier, size_t count, int reps, double* ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif
