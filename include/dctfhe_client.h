/*
 * dctfhe_client.h -- C ABI of libdctfhe_client.so: the key owner's and the data owner's side of include/dctfhe.h on the HOST.
 *
 * Plain C++17 with OpenMP: the library links neither the HIP nor the HSA runtime and holds no device code, so a client or a data owner
 * needs no GPU.  The server (circuits, sessions, evaluation-key import) stays in libdctfhe.so and has no CPU path.
 *
 * Every entry point is the twin of the dctfhe.h entry point it names (dctfhe_host_X <-> dctfhe_X) WITHOUT the context argument: same
 * parameters otherwise, same blobs, same wire forms, same generator streams and row indices (dctfhe.h, "Generator streams of the key
 * material", the packing-key stream R, the public-key stream P and the encryptor's draws).  Blobs made here import into libdctfhe.so
 * and ciphertexts made there decrypt here; the two libraries share nothing at run time.
 * Conventions as in dctfhe.h: int status (0 = OK, < 0 = error, the text through dctfhe_host_last_error(), thread-local),
 * caller-allocated buffers, buf == NULL = size query (only *size is written), opaque handles, no exceptions across the boundary.
 * Threads follow OMP_NUM_THREADS.  The result never depends on the thread count: every word is a function of its index.
 *
 * THE GAUSSIAN -- the one place where host and device may differ.
 * A noise term is rint(x 2^64), x = g sigma - rint(g sigma), g = sqrt(-2 ln u1) cospi(2 u2) (dctfhe.h: u1, u2 from generator words
 * 2 idx, 2 idx + 1).  The device evaluates log and cospi with its math library, the host with libm (cospi by an exact argument
 * reduction to |r| <= 1/4): two implementations, each within a unit or two of the last place of g.  At the largest sigma 2^64 of any
 * catalogue (about 2^45 |g|) an f64 relative error of a few 2^-52 stays under 2^-3 absolute before the final rint, so
 *     |host noise term - device noise term| <= 1        (units of 2^-64)
 * and for a key-switch body, which is rounded to the grid 2^-(8 limbs) after the noise is added, at most ONE STEP of that grid.
 * Everything without a noise term is equal word for word: secret bits, generator keys, every mask word, stream ids, headers, and every
 * decryption.  dctfhe.h's "key material is a pure function of (params, seed)" therefore holds per implementation: secret bits and
 * masks are identical everywhere, noise terms up to that unit.  Both keys are valid keys of the same secret; a server cannot tell
 * which side made a blob.
 *
 * Left out on purpose: the full (Fourier) evaluation-key export (the server transforms a compressed blob on import), the margin audit
 * with a client key, dctfhe_client_key_export_bsk, and everything that takes a context, a circuit or a session.
 * The parameter check is dctfhe_params_check's without its last question (does the ENGINE have a bootstrap kernel for a tier's
 * (logN, k, l)?): that one is the server's to answer, at dctfhe_eval_keys_import.
 */
#ifndef DCTFHE_CLIENT_H
#define DCTFHE_CLIENT_H
#include "dctfhe.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dctfhe_host_client_key dctfhe_host_client_key;   /* CLIENT: secret key bits and the generator keys, in host memory */
typedef struct dctfhe_host_public_key dctfhe_host_public_key;   /* ENCRYPTOR: the expanded public key and the handle's own generator key */

const char* dctfhe_host_last_error(void);
int dctfhe_host_version(void);
/* OpenMP threads the library will use (omp_get_max_threads: OMP_NUM_THREADS where set) */
int dctfhe_host_threads(void);

/* dctfhe_client_key_create: key bits from (seed, STREAM_BIGKEY / STREAM_SMALLKEY), the public generator key one block of the secret
 * one, a fresh 128-bit encryption nonce from the OS (getrandom). */
int dctfhe_host_client_key_create(const dctfhe_params* params, const uint8_t seed[32], dctfhe_host_client_key** out);
/* clears the secret bits and generator keys before the memory is released */
int dctfhe_host_client_key_destroy(dctfhe_host_client_key* client);
int dctfhe_host_client_key_export_secret(dctfhe_host_client_key* client, uint8_t* big_key /* D */, uint8_t* small_key /* n_max */);
int dctfhe_host_client_key_set_encrypt_counter(dctfhe_host_client_key* client, uint64_t next_call);
int dctfhe_host_client_key_set_encrypt_nonce(dctfhe_host_client_key* client, const uint8_t nonce[16]);
/* test view: the handle's public generator key (what the blobs carry) and its public encryption key (what encrypt_seeded returns) */
int dctfhe_host_client_key_public_keys(dctfhe_host_client_key* client, uint8_t pub[32] /* may be NULL */, uint8_t enc_pub[32] /* may be NULL */);

/* dctfhe_encrypt_rows / dctfhe_encrypt_seeded / dctfhe_decrypt_rows / dctfhe_decrypt_packed / dctfhe_decrypt_ring */
int dctfhe_host_encrypt_rows(dctfhe_host_client_key* client, const uint64_t* phases, size_t count, int dim, uint64_t* cts /* count x (dim+1) */);
int dctfhe_host_encrypt_seeded(dctfhe_host_client_key* client, const uint64_t* phases, size_t count, uint8_t mask_key[32] /* out */,
                               uint64_t* stream /* out */, uint64_t* bodies /* count */);
int dctfhe_host_decrypt_rows(dctfhe_host_client_key* client, const uint64_t* cts /* count x (dim+1) */, size_t count, int dim, uint64_t* phases);
int dctfhe_host_decrypt_packed(dctfhe_host_client_key* client, int n, const uint16_t* rows, size_t count, uint64_t* phases);
int dctfhe_host_decrypt_ring(dctfhe_host_client_key* client, int logN, const uint16_t* words, size_t count, uint64_t* phases);

/* dctfhe_eval_keys_export_compressed: the blob dctfhe_eval_keys_import reads (magic 'DEVC').  The heavy part: per bootstrap-key row a
 * negacyclic product of the mask polynomials with the binary GLWE key, shift-and-add over rows in parallel. */
int dctfhe_host_eval_keys_export_compressed(dctfhe_host_client_key* client, void* buf, size_t capacity, size_t* size);
/* the same under a tier selection (dctfhe.h TIER SELECTIONS; NULL: everything, the bytes of the call above): the selection is closed
 * first, a pruned blob is 'DEVC' version 2 with the two masks behind the public generator key, and only the kept sections are computed. */
int dctfhe_host_eval_keys_export_compressed_tiers(dctfhe_host_client_key* client, const dctfhe_key_tiers* tiers, void* buf, size_t capacity, size_t* size);
int dctfhe_host_pack_key_export(dctfhe_host_client_key* client, int logN, int l_p, int beta_p, double sigma_p, void* buf, size_t capacity, size_t* size);
int dctfhe_host_public_key_export(dctfhe_host_client_key* client, int logN, double sigma, void* buf, size_t capacity, size_t* size);

/* dctfhe_public_key_*: the data owner's handle, from the blob above (or dctfhe_public_key_export's) */
int dctfhe_host_public_key_import(const void* buf, size_t size, dctfhe_host_public_key** out);
int dctfhe_host_public_key_destroy(dctfhe_host_public_key* key);
int dctfhe_host_public_key_info(dctfhe_host_public_key* key, int* logN, double* sigma /* each may be NULL */);
int dctfhe_host_public_key_set_encrypt_seed(dctfhe_host_public_key* key, const uint8_t* seed32);
int dctfhe_host_public_key_draws(dctfhe_host_public_key* key, uint64_t call, size_t count, uint8_t* u /* groups x N_e */, int64_t* e1 /* groups x N_e */,
                                 int64_t* e2 /* count */);
int dctfhe_host_encrypt_public(dctfhe_host_public_key* key, const uint64_t* phases, size_t count, uint64_t* words_out /* dctfhe_public_words */);

#ifdef __cplusplus
}
#endif
#endif
