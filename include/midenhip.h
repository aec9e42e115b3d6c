/* libmidenhip — C ABI of the MI355X-native STARK proving backend for Miden VM.
 *
 * Drop-in boundary: these entry points are what a Rust FFI shim under
 * `miden_prover::prove_stark()` (reference prover/src/lib.rs:317-355) binds; see INTEGRATION.md
 * for the `extern "C"` block and the cfg-gated `prove_stark_hip`.  Conventions, following the
 * reference's own C-ABI precedent (crates/crypto/src/hash/algebraic_sponge/rescue/arch/mod.rs:12-21):
 *   - plain pointers and sizes only; all field elements are uint64_t Goldilocks values
 *     (p = 2^64 - 2^32 + 1); inputs may be non-canonical (< 2^64), outputs are canonical;
 *   - extension-field elements are 2 consecutive uint64_t [c0, c1] (x^2 = 7);
 *   - every function returns 0 on success or an MH_ERR_* code; mh_last_error(ctx) gives the
 *     message; no exception or panic crosses the boundary;
 *   - the caller owns host buffers; the library owns device buffers until the matching *_free;
 *   - one ctx per proving thread, calls on one ctx are blocking and not re-entrant.
 */
#ifndef MIDENHIP_H
#define MIDENHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_OK 0
#define MH_ERR_INVALID 1
#define MH_ERR_HIP 2
#define MH_ERR_OOM 3
#define MH_ERR_INTERNAL 4
#define MH_ERR_COMM 5      /* a collective of a sharded proof failed or did not complete within $MH_COMM_TIMEOUT_S (default 120 s) */

typedef struct mh_ctx mh_ctx;
typedef struct mh_trace mh_trace; /* device-resident trace matrix (column-major) */
typedef struct mh_tree mh_tree;   /* device-resident LMCS tree + its LDE matrices */
typedef struct mh_air mh_air;     /* an AIR: constraint DAG compiled for the device interpreter */
typedef struct mh_proof mh_proof; /* host-resident proof: transcript fields + commitments */

/* ---- context ------------------------------------------------------------------------------ */
int mh_ctx_create(int device_id, mh_ctx** out);
void mh_ctx_destroy(mh_ctx* ctx);
/* Release the device buffers the context keeps pooled between proofs (freed automatically on OOM and at destroy). */
int mh_ctx_trim(mh_ctx* ctx);
/* Device memory as a long-lived service sees it: out[0] = bytes cached in the context's buffer pool (returned by mh_ctx_trim),
 * out[1] = bytes of twiddle / coset tables the context keeps, out[2] = free and out[3] = total bytes of the device (hipMemGetInfo). */
int mh_ctx_mem_stats(mh_ctx* ctx, uint64_t out[4]);
const char* mh_last_error(const mh_ctx* ctx);
int mh_device_count(void);

/* Kernel profiler: HIP events recorded on the ctx's private stream around each kernel class.
 * mh_prof_get returns accumulated milliseconds, attributed algorithmic bytes and launch count. */
int mh_prof_enable(mh_ctx* ctx, int on);
/* Restrict the profiler to ONE kernel class (e.g. "lmcs_leaf_absorb"); NULL or "" = every class and span again.  An event
 * record is a barrier packet on the stream: recording every class costs a 2^20-row proof ~0.5 ms (a proof has ~130 scopes),
 * one class ~10 us. */
int mh_prof_filter(mh_ctx* ctx, const char* name);
int mh_prof_reset(mh_ctx* ctx);
int mh_prof_get(mh_ctx* ctx, const char* name, double* ms, double* bytes, long* count);
/* writes up to cap bytes of a '\n'-separated "name ms bytes count" listing */
int mh_prof_dump(mh_ctx* ctx, char* buf, size_t cap);

/* ---- unit-parity entry points --------------------------------------------------------------- */
/* Poseidon2 permutation (replaces Poseidon2Permutation256::permute_mut,
 * crates/crypto/src/hash/algebraic_sponge/poseidon2/mod.rs:340,380-386) on n states of 12 felts,
 * host array-of-states layout [n][12], in place. */
int mh_poseidon2_permute(mh_ctx* ctx, uint64_t* states, size_t n);
/* Measurement aid: permutations per second of the same device permutation with the state held in
 * registers (no memory traffic) = the VALU ceiling bench.py reports hash kernels against. */
int mh_poseidon2_register_rate(mh_ctx* ctx, double* perms_per_second);

/* Coset LDE of a host row-major matrix (replaces Radix2DitParallel::coset_lde_batch as called at
 * crates/lifted-stark/src/prover/commit.rs:173): `out` receives the (n<<added_bits) x width
 * row-major matrix in the REFERENCE's storage order (physical row r = evaluation at
 * shift * w^bitrev(r)), for parity checks. */
int mh_coset_lde_batch(mh_ctx* ctx, const uint64_t* rowmajor, int log_n, size_t width, int added_bits,
                       uint64_t shift, uint64_t* out);

/* ---- device-resident traces ----------------------------------------------------------------- */
/* Upload a host row-major RowMajorMatrix<Felt> (values, width) of height 2^log_n: one H2D copy +
 * an on-device transpose to column-major; canonicalises felts. */
int mh_trace_upload(mh_ctx* ctx, const uint64_t* rowmajor, int log_n, size_t width, mh_trace** out);
/* The same without blocking: returns as soon as the copy is enqueued.  The DMA and the transpose run on the context's COPY
 * stream, under whatever the compute stream is doing; every consumer of the trace (mh_prove, mh_session_*, mh_commit_traces,
 * mh_lookup_build_aux, mh_trace_download) orders itself after the upload on the GPU, no host wait.  Start the uploads of all
 * the matrices of a statement in proof order (ascending height, ties by instance index), then call mh_prove: the LDE and the leaf
 * sponges of matrix k run while matrices k+1.. are still on the PCIe link; only the first matrix's copy is exposed.  `rowmajor`
 * should be page-locked (mh_host_alloc) -- pageable memory makes the copy synchronous -- and must stay valid and unmodified
 * until the proof has been made (or mh_trace_wait has returned).  Reference: prover/src/lib.rs:317-355 hands over host
 * RowMajorMatrix values. */
int mh_trace_upload_async(mh_ctx* ctx, const uint64_t* rowmajor, int log_n, size_t width, mh_trace** out);
/* The same for a COLUMN-major host matrix, colmajor[c * 2^log_n + r] (a trace builder that writes columns: SURVEY 8(f) #4).
 * Every column is one contiguous copy and there is no transpose, so ONE matrix pipelines too: the columns go up in groups of
 * eight, and the LDE of a group starts when that group has landed -- the exposed part of the upload is the first group.  (A
 * row-major matrix cannot be split like this: its column windows move at 16-36 GB/s.)  Same lifetime rules as above. */
int mh_trace_upload_cols_async(mh_ctx* ctx, const uint64_t* colmajor, int log_n, size_t width, mh_trace** out);
/* Blocks until the upload of `t` has landed (the host buffer may be reused) and releases its landing buffer. */
int mh_trace_wait(mh_ctx* ctx, mh_trace* t);
/* The same for a row-major matrix that is already in device memory (a GPU trace generator): no PCIe traffic. */
int mh_trace_from_device(mh_ctx* ctx, const uint64_t* device_rowmajor, int log_n, size_t width, mh_trace** out);
void mh_trace_free(mh_trace* t);
/* Page-locked host memory (hipHostMalloc): a trace built in it uploads by direct DMA at PCIe line rate; any
 * other host pointer works too, staged by the runtime (several times slower).  NULL on failure. */
void* mh_host_alloc(size_t bytes);
void mh_host_free(void* p);

/* ---- commitments (K1-K3) -------------------------------------------------------------------- */
/* The commitment scheme's hasher (the reference's StarkConfig::Lmcs, air/src/config.rs:212-305).  MH_LMCS_POSEIDON2 (default):
 * StatefulSponge leaves + TruncatedPermutation nodes.  MH_LMCS_BLAKE3: the Blake3_256 configuration's LMCS (config.rs:275-289,
 * ProvingOptions::default()): leaf = chain over the matrices of blake3(state || row felts as 8 LE bytes each) from a zero
 * state (crates/stateful-hasher/src/chaining.rs:32-50, alignment 1), node = blake3(left || right); a digest travels as
 * four uint64_t = its 32 bytes little-endian.  MH_LMCS_KECCAK: the Keccak configuration's LMCS (config.rs:307-353): the
 * overwrite-mode sponge over 64-bit lanes with Keccak-f[1600] (25 lanes, 17 felts as canonical u64 per permutation, digest =
 * lanes 0..3; alignment 17), node = one permutation over left || right in a zero state.  MH_LMCS_RPO / MH_LMCS_RPX: the
 * other two ALGEBRAIC configurations (config.rs:224-245): the Poseidon2 LMCS and duplex challenger with the Rescue Prime
 * permutations (crates/crypto/src/hash/algebraic_sponge/rescue/).
 * The setting is the context's StarkConfig: it applies to everything the context commits, opens and proves -- mh_commit_traces,
 * mh_commit_traces_sharded, mh_tree_open, mh_prove / mh_prove_sharded and the staged session.  The row alignment follows the
 * hasher (lmcs.alignment(): the sponge's rate, 8 or 17; 1 for the chaining hasher: OOD blocks and opened rows are then
 * unpadded), the FRI leaves use it, and so does the challenger of the one-shot prover: the duplex sponge over the configuration's
 * permutation (Poseidon2, RPO, RPX) or, for Blake3 and Keccak, the library's restatement of p3's SerializingChallenger64 over a
 * HashChallenger (external code with no in-tree mirror: a shim that wants p3's own keeps the transcript on the host and drives
 * mh_session_*, which never sees a challenger).  mh_verify / mh_verify_ex are the Poseidon2 configuration; mh_verify_lmcs takes
 * the id.  mh_grind is the duplex sponge's PoW search (algebraic configurations). */
#define MH_LMCS_POSEIDON2 0
#define MH_LMCS_BLAKE3 1
#define MH_LMCS_KECCAK 2
#define MH_LMCS_RPO 3
#define MH_LMCS_RPX 4
int mh_ctx_set_lmcs(mh_ctx* ctx, int lmcs);
int mh_ctx_get_lmcs(const mh_ctx* ctx);
/* Hiding LMCS: salted leaves (the reference's HidingLmcsConfig, crates/lifted-stark/src/lmcs/hiding_config.rs: LiftedMerkleTree with
 * SALT_ELEMS > 0).  With salt_elems = n > 0 every tree the context commits from now on absorbs, after its last matrix, one more matrix
 * of n columns and tree height (lifted_tree.rs:233-245), and every opened leaf hints its n raw salt felts, unpadded, after its aligned
 * rows (lmcs/proof.rs:108-121).  It changes mh_commit_traces, mh_tree_open, mh_prove, mh_prove_host and the staged mh_session_* path;
 * every tree of a proof is salted -- preprocessed (if committed on this context with the same setting), main, aux, quotient, each FRI
 * round -- as the reference's prover uses one Lmcs for all of them.  Such a proof verifies with mh_verify_hiding; mh_verify,
 * mh_verify_ex and mh_verify_lmcs are the non-hiding configurations.  salt_elems = 0 (the default) is the plain LMCS: same bytes, same
 * kernels as a context that never called this.
 * The salt is a PRF of the seed and is never stored: the salt row of PHYSICAL (bit-reversed, lifted_tree.rs:300-306) leaf row i of
 * the t-th salted tree committed on the context since this call (t = 0, 1, ...; mh_tree_salt_index) is lanes 0 .. n-1 of one Poseidon2
 * permutation of   [i, t, 0x53414c54, 0, 0, 0, 0, 0, seed0, seed1, seed2, seed3]   (seed words reduced mod p; the key sits in the
 * capacity lanes), whichever hash function the LMCS uses.  The leaf kernels derive it in registers; mh_tree_open and
 * mh_tree_download_salt regenerate the rows they need.  The same seed therefore reproduces the same trees and proofs.
 * SECURITY: the seed is the only secret.  It must be unpredictable and FRESH for every proof -- a seed used twice, or one a verifier
 * can guess, hides nothing.  seed = NULL draws it from the operating system (getrandom) and is the right choice outside tests.
 * Hiding commitments are ONE ingredient of a zero-knowledge prover: the reference randomises neither the trace nor the quotient, Miden's
 * own configurations use the non-hiding LMCS, and this library builds what the reference has and no more -- a proof made with salt on
 * is NOT zero-knowledge.
 * Not covered (MH_ERR_INVALID and a message while salt is on): mh_shard_*, mh_commit_traces_sharded, mh_prove_sharded and sharded
 * sessions, mh_prove_miden*, mh_prove_precompile*, mh_check_* (the statement entries pin the reference's non-hiding configurations). */
#define MH_MAX_SALT_ELEMS 8
int mh_ctx_set_salt(mh_ctx* ctx, int salt_elems /* 0 = off (default) .. 8 */, const uint64_t seed[4] /* NULL: OS entropy (getrandom) */);
int mh_ctx_get_salt(const mh_ctx* ctx);
/* blake3(data) (host only; unit-parity entry point, like mh_poseidon2_permute) */
void mh_blake3(const uint8_t* data, size_t n, uint8_t out32[32]);

/* commit_traces (crates/lifted-stark/src/prover/commit.rs:142-180): per trace (proof order =
 * ascending height) coset-LDE by 2^log_blowup on the canonical shift of ITS lde order, then the
 * aligned LMCS tree (Lmcs::build_aligned_tree, lmcs/config.rs:125-137).  root = 4 felts.
 * The tree keeps its LDEs: mh_pcs_open / mh_pcs_begin open one or several such trees at 1..4 out-of-domain points and prove the
 * evaluations (the polynomial commitment scheme on its own, no AIR), mh_pcs_verify checks them. */
int mh_commit_traces(mh_ctx* ctx, int n_traces, mh_trace* const* traces, int log_blowup, mh_tree** out,
                     uint64_t root[4]);
/* mh_commit_traces' root on the CPU: HOST ONLY (no context, no HIP call), for verifiers and setup.  The root of an AIR's preprocessed
 * matrices is part of the statement a verifier checks (the preprocessed_root of mh_verify*): a verifier box has no GPU and derives it
 * here from the matrices it knows, instead of being told it by the prover.  No prover entry calls this; proving has no CPU path.
 * rowmajor[i]: matrix i, row-major, 2^log_heights[i] rows of widths[i] cells (any uint64_t, reduced mod p as every upload path does),
 * in proof order = ascending height.  root = exactly what mh_commit_traces returns for the same matrices in the same order on a
 * context set to `lmcs` (MH_LMCS_*) with salt off, byte-hash roots packed as by mh_tree_root.  Uses up to 16 threads.
 * MH_ERR_INVALID + a reason in err (may be NULL): a null pointer, n_mats < 1, a zero width, log_blowup outside 0..8,
 * log_heights[i] + log_blowup > 32, descending heights, an unknown lmcs. */
int mh_commit_host(int lmcs, int n_mats, const uint64_t* const* rowmajor, const uint8_t* log_heights, const size_t* widths,
                   int log_blowup, uint64_t root[4], char* err, size_t err_cap);
void mh_tree_free(mh_tree* t);
int mh_tree_root(const mh_tree* t, uint64_t root[4]);
int mh_tree_log_height(const mh_tree* t);

/* LmcsTree::prove_batch (lmcs/lifted_tree.rs:155-180): for sorted, de-duplicated domain indices
 * (this call sorts/dedups), the opened rows of every matrix padded to `alignment`, then the
 * missing sibling digests bottom-up, left-to-right.  fields/commits must hold
 * n_idx * (sum(aligned widths) + mh_tree_salt_elems(t)) and n_idx * depth * 4 felts at most: a salted tree (mh_ctx_set_salt) hints
 * each leaf's raw salt felts after its rows. */
int mh_tree_open(mh_ctx* ctx, const mh_tree* t, const uint64_t* indices, size_t n_idx, size_t alignment,
                 uint64_t* fields, size_t* n_fields, uint64_t* commits, size_t* n_commit_felts);

/* Parity/debug: download matrix `mat` of the tree in the reference's storage order
 * (row-major, bit-reversed rows). */
int mh_tree_download_lde(mh_ctx* ctx, const mh_tree* t, int mat, uint64_t* out_rowmajor_bitrev);
/* Parity/debug: download all digest layers, leaf layer (domain order) first: (2H-1)*4 felts. */
int mh_tree_download_layers(mh_ctx* ctx, const mh_tree* t, uint64_t* out);
/* Hiding LMCS (mh_ctx_set_salt): the salt width the tree was committed with (0: not salted) and its number t in the salt PRF. */
int mh_tree_salt_elems(const mh_tree* t);
uint64_t mh_tree_salt_index(const mh_tree* t);
/* Parity/debug: the tree's salt matrix, regenerated: [2^log_height][salt_elems], PHYSICAL (bit-reversed) row order like
 * mh_tree_download_lde (lifted_tree.rs:300-306) -- the matrix that, appended to the tree's LDEs, gives its leaves.  It IS the secret
 * the commitment hides behind.  MH_ERR_INVALID for an unsalted tree. */
int mh_tree_download_salt(mh_ctx* ctx, const mh_tree* t, uint64_t* out);

/* ---- coset-sharded commitment across the GPUs of a node (one process + one ctx per GPU) -------- */
/* The LDE is stored coset-major, so rank k of `world` (a power of two <= 2^log_blowup) owns cosets
 * [k*B/world, (k+1)*B/world) of every column: it runs the (replicated) inverse NTT, the forward NTT
 * of ITS cosets only and the leaf sponges of its leaves.  The Merkle tree is indexed in domain order
 * (crates/lifted-stark/src/lmcs/lifted_tree.rs:247-258), i.e. by rows first, so one all-to-all of
 * leaf digests follows (done by the host layer with RCCL / torch.distributed, see
 * miden-vm_amd/sharding.py): rank d receives rows [d*N/world, (d+1)*N/world) of every coset, laid
 * out [B][N/world] digests, builds that subtree, and the `world` subroots (all-gathered, 32 B each)
 * are combined on the host.  The result equals mh_commit_traces' root on one GPU. */
typedef struct mh_shard mh_shard;
int mh_shard_commit_leaves(mh_ctx* ctx, int n_traces, mh_trace* const* traces, int log_blowup, int rank, int world,
                           mh_shard** out);
void mh_shard_free(mh_shard* s);
/* DEVICE pointer to this rank's leaf digests, [cosets_local][N] x 4 felts (coset-major). */
uint64_t* mh_shard_leaf_digests(mh_shard* s, size_t* n_digests);
/* digests_device: DEVICE pointer to the exchanged digests [B][N/world] x 4 felts. */
int mh_shard_build_subtree(mh_ctx* ctx, mh_shard* s, const uint64_t* digests_device, uint64_t subroot[4]);
/* Host only (no GPU needed): Merkle root over `world` subroots given in rank order, Poseidon2 nodes ... */
int mh_merkle_cap_root(const uint64_t* subroots, int world, uint64_t root[4]);
/* ... and under any LMCS hasher (MH_LMCS_*): the one the context of mh_shard_commit_leaves / mh_shard_build_subtree was set to. */
int mh_merkle_cap_root_lmcs(int lmcs, const uint64_t* subroots, int world, uint64_t root[4]);

/* ---- AIRs as data: the constraint DAG blob "MHDAG001" ------------------------------------------ */
/* The Rust side captures `air.eval` once on a symbolic builder (the route of
 * crates/ace-codegen/src/pipeline.rs:71-123) and ships a flat u64 blob:
 *   [0] magic 0x4d48444147303031  [1] main_width  [2] aux_width (EF columns)  [3] num_randomness
 *   [4] num_aux_values  [5] num_public_values  [6] n_periodic  [7] log_quotient_degree
 *   [8] n_nodes  [9] n_constraints  [10] preprocessed_width  [11] reserved
 *   n_periodic x { len, values[len] }            periodic columns (power-of-two lengths)
 *   n_nodes x { op | a << 8 | b << 36, const }   ops: 0 CONST(const) 1 MAIN(a=col,b=row offset)
 *        2 AUX(a=EF col,b=row) 3 PUBLIC(a) 4 PERIODIC(a) 5 IS_FIRST 6 IS_LAST 7 IS_TRANSITION
 *        8 RANDOMNESS(a) 9 AUX_VALUE(a) 10 ADD(a,b) 11 SUB(a,b) 12 MUL(a,b) 13 NEG(a) 14 PREPROCESSED(a=col,b=row);
 *        a, b < node id for the four gates
 *   n_constraints x node id                      in emission order (constraint k folds with alpha^(K-1-k))
 * miden-vm_amd/dag.py is the reference exporter used by tests and bench. */
int mh_air_load(mh_ctx* ctx, const uint64_t* blob, size_t n_words, mh_air** out);
void mh_air_free(mh_air* air);
int mh_air_log_quotient_degree(const mh_air* air);
/* Number of specialised kernels the DAG was compiled into (hiprtc at load time, code objects cached on disk
 * under $MH_JIT_CACHE_DIR or ~/.cache/midenhip); 0 = small DAG, evaluated by the generic interpreter kernel.
 * MH_JIT=0 / MH_JIT=1 in the environment force either path (both are bit-identical). */
int mh_air_compiled_chunks(const mh_air* air);
/* Offline precompilation, host only (no GPU, no context): compiles the chunk kernels of a constraint-DAG blob or of a lookup program
 * ("MHLKP001") for gfx950 into the cache directory ($MH_JIT_CACHE_DIR, else ~/.cache/midenhip), where a later mh_air_load /
 * mh_lookup_load finds them -- a prover service ships the directory and never runs hiprtc on the request path (measured for the
 * chiplets AIR: 5.7 s cold, 3 ms from the cache).  *n_chunks = kernels of the program (0: small DAG, interpreted). */
int mh_jit_precompile(const uint64_t* blob, size_t n_words, int* n_chunks);
/* Largest VGPR count over those kernels (their occupancy is 512 / VGPRs waves per SIMD); 0 when nothing was compiled. */
int mh_air_compiled_max_vgprs(const mh_air* air);
/* Preprocessed columns (fixed circuit data committed once at setup: crates/lifted-stark/src/preprocessed.rs; blob word
 * [10] = preprocessed width, DAG op 14 PREPROCESSED(a = col, b = row offset)).  Setup = mh_commit_traces of the
 * preprocessed matrices of the AIRs that declare some, in PROOF order (ascending height, ties by instance index), with
 * the proving blowup; its root is observed by the caller right after the protocol parameters and before the statement
 * (prover/mod.rs:282-286), i.e. it belongs in `pre_observe`.  Each such AIR is then pointed at its matrix of that tree;
 * proofs open the tree first (`[preprocessed?, main, aux, quotient]`).  The tree must outlive the proofs. */
int mh_air_attach_preprocessed(mh_air* air, const mh_tree* tree, int matrix_index, const mh_trace* raw);
/* tree = NULL detaches.  `raw` = the uploaded preprocessed matrix itself (trace domain); only needed when a lookup
 * program attached to the same AIR reads preprocessed columns (table lookups), NULL otherwise. */

/* ---- LogUp aux trace on the device -------------------------------------------------------------------------
 * Replaces `build_logup_aux_trace` (air/src/lookup/aux_builder.rs:49-96) for an AIR whose bus messages are
 * exported as a lookup program: the "MHLKP001" blob = the constraint-DAG blob's header (w[2] = number of aux EF
 * columns, w[4] = w[5] = w[7] = 0, w[9] ignored, w[10] = preprocessed width), periodic tables and node list (ops CONST,
 * MAIN, PREPROCESSED, PERIODIC, RANDOMNESS, ADD, SUB, MUL, NEG), followed per aux column by: count, then `count` pairs (multiplicity node id,
 * denominator node id).  Semantics (aux_builder.rs:202-258): f_c(r) = sum_j m_j(r) / d_j(r) over the fractions
 * of column c with m_j(r) != 0;  aux[r][c >= 1] = f_c(r);  aux[r][0] = sum_{r' < r} sum_c f_c(r');  the one
 * aux value = the sum over all rows (`committed_finals`).  A zero denominator is MH_ERR_INVALID.
 * Optional tail, REGISTER columns behind the w[2] LogUp columns (precompiles-prover/src/tests/aux_register.rs; the extension-field
 * accumulators of precompiles-prover/src/uint/store_mul/mod.rs:118-121, which that AIR's `build_aux_trace` computes on the CPU):
 * count, then per register: keep node id (0xFFFFFFFF = the constant 1), build node id, n_terms <= 8, n_terms pairs (another register,
 * coefficient node id; no cycles).  Semantics: r_k[0] = 0,  r_k[i + 1] = keep(i) r_k[i] + sum_j coeff_j(i) r_j[i] + build(i);  aux
 * column w[2] + k = r_k.  Registers stay out of the running sum and of the aux value; the AIR's own constraints tie them down.
 * `mh_air_attach_lookup` makes mh_prove / mh_session_commit_aux build that instance's aux trace on the device
 * (its `mh_aux_builder` callback is not called); the lookup must outlive the AIR's proofs. */
typedef struct mh_lookup mh_lookup;
int mh_lookup_load(mh_ctx* ctx, const uint64_t* blob, size_t n_words, mh_lookup** out);
void mh_lookup_free(mh_lookup* l);
int mh_air_attach_lookup(mh_air* air, const mh_lookup* l); /* l = NULL detaches */
/* Stand-alone: aux trace (device resident, 2 * (LogUp columns + registers) base columns) + accumulator final of `main_trace`. */
int mh_lookup_build_aux(mh_ctx* ctx, const mh_lookup* l, const mh_trace* main_trace, const mh_trace* preprocessed /* or NULL */,
                        const uint64_t* randomness, size_t n_randomness, mh_trace** aux_out, uint64_t acc_final[2]);
/* Copy a device trace back as a row-major [2^log_n][width] matrix (tests). */
int mh_trace_download(mh_ctx* ctx, const mh_trace* t, uint64_t* rowmajor_out);

/* ---- the whole proof: miden_prover::prove_stark (prover/src/lib.rs:317-355) -> ------------------ */
/* ProverInstance::prove (crates/lifted-stark/src/prover/mod.rs:230-578).                           */
typedef struct mh_pcs_params { /* PcsParams::new argument order regrouped (pcs/params.rs:52-96) */
  int log_blowup, log_folding_arity, log_final_degree, folding_pow_bits, deep_pow_bits, num_queries, query_pow_bits;
} mh_pcs_params;

/* LiftedAir::build_aux_trace (crates/lifted-air/src/air.rs): called once per AIR instance, in
 * instance order, after the main commitment.  randomness = 2*max_num_randomness felts; the callee
 * fills the flattened EF aux trace (rows x 2*aux_width, row-major) and 2*num_aux_values felts.
 * A non-zero return aborts the proof (this is also where Statement::eval_external failures go).
 * NULL = every aux trace and aux value is zero (DummyMidenAir), generated on the device. */
typedef int (*mh_aux_builder)(void* user, int instance_idx, const uint64_t* randomness, uint64_t* aux_out,
                              uint64_t* aux_values_out);

/* airs / traces in INSTANCE order.  challenger_state = the 12-felt sponge state of the prototype
 * challenger (air/src/config.rs:255-273: RELATION_DIGEST in state[8..12]); pre_observe = every felt
 * observed before observe_shape (protocol parameters, air/src/config.rs:188-198, then
 * Statement::observe).  The transcript, PoW witnesses (smallest valid witness) and query openings
 * are produced inside; the result is the reference's StarkProofData. */
int mh_prove(mh_ctx* ctx, const mh_pcs_params* params, int n_airs, mh_air* const* airs, mh_trace* const* traces,
             const uint64_t* public_values, size_t n_public_values, const uint64_t challenger_state[12],
             const uint64_t* pre_observe, size_t n_pre_observe, mh_aux_builder aux_builder, void* user, mh_proof** out);
/* The shape of prove_stark itself (prover/src/lib.rs:317-355): HOST row-major matrices in (instance order; page-locked memory from
 * mh_host_alloc for full overlap), proof out.  The library starts every upload at once in proof order and proves: matrix k + 1 is on
 * the PCIe link while matrix k is extended and hashed.  Equivalent to mh_trace_upload_async x n, mh_prove, mh_trace_free x n. */
int mh_prove_host(mh_ctx* ctx, const mh_pcs_params* params, int n_airs, mh_air* const* airs, const uint64_t* const* traces_rowmajor,
                  const int* log_heights, const uint64_t* public_values, size_t n_public_values, const uint64_t challenger_state[12],
                  const uint64_t* pre_observe, size_t n_pre_observe, mh_aux_builder aux_builder, void* user, mh_proof** out);
/* One proof sharded over `world` GPUs (one process + one ctx per GPU, all ranks call this with the same
 * arguments and traces; every rank returns the same proof).  The coset-major layout makes every pass over
 * LDE-sized data local to a rank's cosets; what crosses ranks goes through these three collectives on
 * DEVICE buffers (implemented by the host layer over RCCL, see miden-vm_amd/sharding.py):
 *   all_to_all  (leaf digests of every commitment, 32 B per leaf),
 *   all_gather  (subtree roots; quotient-chunk coefficients; a FRI layer once it has fewer rows per
 *                coset than ranks),
 *   all_reduce_sum_u64 (query openings: every value is contributed by exactly one rank).
 * Each callback returns 0 on success; unless `stream_ordered` is set the library synchronises its stream before calling
 * and expects the collective to be complete on return.  world must be a power of two <= 2^log_blowup and <= the shortest trace.
 * Any mix of per-AIR quotient degrees is accepted (an AIR's native quotient chunks are gathered with all_gather and upsampled on
 * every rank), and world may exceed the number of quotient chunks D: chunk t then lives on rank t * world / D, the other ranks
 * idle through constraint evaluation (if D < B only world * D / B ranks hold quotient-coset rows). */
typedef struct mh_comm {
  int rank, world;
  void* user;
  int (*all_to_all)(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_peer);
  int (*all_gather)(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_rank);
  int (*all_reduce_sum_u64)(void* user, uint64_t* buf_dev, size_t n);
  /* 0: host-synchronous callbacks (the contract above: stream synchronised before the call, complete on return);
   * 1: the callbacks ENQUEUE on the ctx's stream and return at once (mh_comm_create_rccl): no host synchronisation. */
  int stream_ordered;
} mh_comm;
/* The trace of a sharded proof: every rank uploads only its 1/world of the ROWS (a contiguous slice of the row-major host matrix)
 * over its own PCIe link, the slices are all-gathered over the communicator and each rank transposes the whole.  Collective: every
 * rank calls it with the same shape; `rowmajor` must be readable by every rank (threads of one process, or a shared mapping), a
 * rank reads only its slice.  The result is an ordinary mh_trace (the full matrix on every rank: the inverse NTT needs all rows). */
int mh_trace_upload_sharded(mh_ctx* ctx, const mh_comm* comm, const uint64_t* rowmajor, int log_n, size_t width, mh_trace** out);
/* ---- the communicator inside the library: RCCL over xGMI ------------------------------------------------------
 * One process + one ctx per GPU.  Rank 0 calls mh_rccl_unique_id and hands the 128 bytes to every rank (by whatever
 * started the ranks); every rank calls mh_comm_create_rccl with its ctx (ncclCommInitRank: collective, blocks until all
 * `world` ranks arrive).  The returned mh_comm runs the three collectives as RCCL calls on the ctx's own stream and on the
 * library's own device buffers (leaf-digest all-to-all = grouped ncclSend/ncclRecv, ncclAllGather, ncclAllReduce(sum, u64)).
 * RCCL is opened lazily from $MH_RCCL_LIB, $ROCM_PATH/lib/librccl.so.1 or /opt/rocm/lib/librccl.so.1.
 * mh_comm_selftest moves known patterns through all three collectives of ANY mh_comm and checks them (every rank calls it). */
#define MH_RCCL_ID_BYTES 128
int mh_rccl_unique_id(uint8_t id[MH_RCCL_ID_BYTES]);
int mh_comm_create_rccl(mh_ctx* ctx, const uint8_t id[MH_RCCL_ID_BYTES], int rank, int world, mh_comm** out);
void mh_comm_destroy(mh_comm* comm); /* communicators made by mh_comm_create_rccl or mh_comm_create_local */
/* The same collectives between the contexts of ONE process (one thread + one ctx per rank; ranks on different GPUs use peer
 * copies over xGMI, ranks sharing a GPU plain device copies): create one fabric, then every rank's thread calls
 * mh_comm_create_local (collective: returns when all `world` ranks have joined).  Stream ordered like the RCCL communicator.
 * No RCCL, no launcher: the shape for a host that drives all GPUs of a node from one process. */
typedef struct mh_local_fabric mh_local_fabric;
mh_local_fabric* mh_local_fabric_create(int world);
void mh_local_fabric_destroy(mh_local_fabric* f); /* after every rank's communicator has been destroyed */
int mh_comm_create_local(mh_ctx* ctx, mh_local_fabric* f, int rank, mh_comm** out);
/* Marks the fabric dead and wakes every rank waiting in a collective (they return an error).  Call it from a rank's error path
 * -- a failed session step, a rank that will never reach the next collective -- so that its peers do not block for ever.  A failed
 * mh_comm_create_local and a failed collective do this themselves.  Sticky: create a new fabric to continue. */
void mh_local_fabric_abort(mh_local_fabric* f);
int mh_comm_selftest(mh_ctx* ctx, const mh_comm* comm);
/* mh_commit_traces for one rank of a sharded prover (every rank calls it with the same traces): the setup commitment
 * of preprocessed matrices for mh_prove_sharded / sharded sessions.  Same root as mh_commit_traces. */
int mh_commit_traces_sharded(mh_ctx* ctx, const mh_comm* comm, int n_traces, mh_trace* const* traces, int log_blowup,
                             mh_tree** out, uint64_t root[4]);
int mh_prove_sharded(mh_ctx* ctx, const mh_comm* comm, const mh_pcs_params* params, int n_airs, mh_air* const* airs,
                     mh_trace* const* traces, const uint64_t* public_values, size_t n_public_values,
                     const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe,
                     mh_aux_builder aux_builder, void* user, mh_proof** out);
/* ---- staged proof session: the caller owns the Fiat-Shamir transcript ------------------------------
 * The same device stages `mh_prove` runs, one entry point per step of ProverInstance::prove
 * (crates/lifted-stark/src/prover/mod.rs:230-578), for a host that keeps p3's DuplexChallenger /
 * ProverTranscript itself: every call takes the challenges the transcript sampled and returns what the
 * transcript must observe next.  Calls out of protocol order return MH_ERR_INVALID.  EF values are
 * (c0, c1) pairs of canonical felts.  `comm` NULL (or world 1) = single GPU; otherwise every rank makes the
 * same calls with the same challenges (as in mh_prove_sharded).  The session BORROWS the airs and traces:
 * they must outlive it.
 *
 *   begin                    channel.observe(n_airs, log heights...)               order.rs:154-163
 *   commit_main   -> root    channel.send_commitment(root)                         mod.rs:300-318
 *   commit_aux(randomness[num_randomness]) -> root, aux values (proof order)       mod.rs:330-412
 *   commit_quotient(alpha, beta) -> root                                           mod.rs:420-560
 *   ood_point_ok(z) / ood(z) -> evals[2][ood_width] (row z, then row z*w_H)        pcs/prover.rs:70-136
 *   [grind deep_pow_bits]  deep(alpha_deep, beta_deep)                             deep/prover.rs:147-193
 *   num_fri_rounds x { fri_commit -> root, [grind folding_pow_bits], fri_fold(beta) }   fri/prover.rs:113-205
 *   fri_final -> final_poly_len coefficients, descending degree                    fri/prover.rs:212-239
 *   [grind query_pow_bits]  open(indices) -> hinted felts + digests, transcript order   pcs/prover.rs:138-195 */
typedef struct mh_session mh_session;
typedef struct mh_session_shape_t {
  int log_lde_height;    /* query indices are sampled with this many bits */
  size_t num_randomness; /* EF challenges to sample after the main commitment (max over the AIRs) */
  size_t num_aux_values; /* EF aux values sent after the aux commitment (all instances, proof order) */
  size_t ood_width;      /* EF evaluations per OOD point: every committed matrix, each padded to 8 columns */
  int num_fri_rounds;
  size_t final_poly_len; /* EF coefficients of the final polynomial */
} mh_session_shape_t;
int mh_session_begin(mh_ctx* ctx, const mh_comm* comm, const mh_pcs_params* params, int n_airs, mh_air* const* airs,
                     mh_trace* const* traces, const uint64_t* public_values, size_t n_public_values, mh_session** out);
void mh_session_free(mh_session* s);
int mh_session_shape(const mh_session* s, mh_session_shape_t* out);
int mh_session_commit_main(mh_session* s, uint64_t root[4]);
int mh_session_commit_aux(mh_session* s, const uint64_t* randomness, mh_aux_builder aux_builder, void* user,
                          uint64_t root[4], uint64_t* aux_values_out);
int mh_session_commit_quotient(mh_session* s, const uint64_t alpha[2], const uint64_t beta[2], uint64_t root[4]);
int mh_session_ood_point_ok(const mh_session* s, const uint64_t z[2]); /* 1 = acceptable, 0 = resample */
int mh_session_ood(mh_session* s, const uint64_t z[2], uint64_t* evals_out);
int mh_session_deep(mh_session* s, const uint64_t alpha[2], const uint64_t beta[2]);
int mh_session_fri_commit(mh_session* s, uint64_t root[4]);
int mh_session_fri_fold(mh_session* s, const uint64_t beta[2]);
int mh_session_fri_final(mh_session* s, uint64_t* coeffs_out);
/* The result holds only the hints: mh_proof_fields / mh_proof_commitments = what ProverTranscript::hint_* receives. */
int mh_session_open(mh_session* s, const uint64_t* indices, size_t n_indices, mh_proof** out);
/* GrindingChallenger::grind on the device: `state` = the sponge state, `pending` = felts observed since the
 * last permutation (< 8).  Returns the smallest witness; the caller replays check_witness on its challenger. */
int mh_grind(mh_ctx* ctx, const uint64_t state[12], const uint64_t* pending, size_t n_pending, int bits, uint64_t* witness);
/* The same search for the byte challengers of the Blake3 / Keccak configurations (context set accordingly): `input` = the hash
 * challenger's input buffer as it stands before the witness is observed (the chaining value of the last flush followed by every
 * byte observed since); returns the smallest felt w such that, after observing w as 8 little-endian bytes, the u64 built from the
 * LAST eight digest bytes (last byte lowest: HashChallenger pops from the end) has `bits` low zero bits.  The caller replays
 * check_witness on its own challenger. */
int mh_grind_bytes(mh_ctx* ctx, const uint8_t* input, size_t n_input, int bits, uint64_t* witness);
/* ---- the polynomial commitment scheme on its own: open committed trees at N points ---------------------------------
 * pcs::open_with_channel (crates/lifted-stark/src/pcs/prover.rs:34-101) and pcs::verify_aligned (pcs/verifier.rs:72-174) for ANY
 * committed LMCS trees (mh_commit_traces; a session's own through mh_session_trees) and ANY 1 <= N <= MH_PCS_MAX_POINTS out-of-domain
 * points -- the shape of pcs/tests.rs and benches/pcs.rs, and of a p3-style Pcs::open over this backend.  mh_prove runs the same
 * protocol welded to the STARK (trees [preprocessed?, main, aux, quotient], points (z, z * w_N)).
 * Semantics (pcs/deep/interpolate.rs:87-204, pcs/deep/prover.rs:115-315): with N_max the tallest matrix height over all trees, a matrix
 * of height n = N_max / L is evaluated at z_j^L (its lifted polynomial f(X^L) at z_j); a point's evaluations are the matrices of all
 * trees in order, each zero-padded to the LMCS alignment (8; 1 under Blake3; 17 under Keccak) -- `ood_width` EF values; column i of
 * that flat aligned order carries alpha^(ood_width - 1 - i), point j carries beta^j:
 *   Q(x) = sum_j beta^j (f_red(z_j) - f_red(x)) / (z_j - x),   f_red = sum_i alpha^(ood_width - 1 - i) f_i.
 * Duplicate points are legal.  The FRI rounds, grinding and the query phase are those of mh_prove; a tree shorter than the tallest is
 * virtually lifted in the query phase (its indices fold by their low bits, lmcs/tree_indices.rs:72-84).
 * Preconditions, MH_ERR_INVALID with a message otherwise and before anything is launched (pcs/deep/prover.rs:68-79, :133-138):
 * n_trees >= 1; every tree was committed on this context under its current LMCS hasher and salt width with
 * log_blowup == params->log_blowup; at least one tree at the maximum height; 1 <= n_points <= MH_PCS_MAX_POINTS; every point nonzero,
 * outside the trace domain H of the tallest matrix and outside the LDE coset gK (mh_pcs_point_ok; domain.rs:539-553).  Single GPU
 * only: a tree from mh_commit_traces_sharded (world > 1) is refused.  Salted trees (mh_ctx_set_salt) are accepted; the FRI round trees
 * then take the context's salt as in mh_prove.  The trees are BORROWED: they must outlive the mh_pcs.
 * BINDING THE ROOTS IS THE CALLER'S JOB (pcs/tests.rs:69-72 observes them before opening): neither mh_pcs_open nor mh_pcs_verify
 * puts the roots into the transcript.  Passing each root's four words in `pre_observe`, to both, binds them under all five
 * configurations (a byte configuration's words go in as the digest's 32 raw bytes).
 *
 * Staged (the caller owns the transcript; calls out of order return MH_ERR_INVALID, as in the session):
 *   begin(trees, points)     checks the preconditions
 *   evals -> [n_points][ood_width] EF    per point in order: channel.send_algebra_slice     pcs/deep/prover.rs:88-113
 *   [grind deep_pow_bits]  deep(alpha, beta)                                                deep/prover.rs:147-193
 *   num_fri_rounds x { fri_commit -> root, [grind folding_pow_bits], fri_fold(beta) }       fri/prover.rs:113-205
 *   fri_final -> final_poly_len coefficients, descending degree                             fri/prover.rs:212-239
 *   [grind query_pow_bits]  query(indices) -> hints: every input tree in order, then every FRI round   pcs/prover.rs:138-195 */
#define MH_PCS_MAX_POINTS 4
typedef struct mh_pcs mh_pcs;
typedef struct mh_pcs_shape_t {
  int log_lde_height;    /* of the tallest tree: query indices are sampled with this many bits */
  int n_points;
  size_t ood_width;      /* EF evaluations per point: every matrix of every tree, each padded to the LMCS alignment */
  int num_fri_rounds;
  size_t final_poly_len; /* EF coefficients of the final polynomial */
} mh_pcs_shape_t;
/* Host only.  1 = z may be opened at when the tallest committed matrix has 2^log_max_trace_height rows, 0 = not (or bad arguments). */
int mh_pcs_point_ok(int log_max_trace_height, int log_blowup, const uint64_t z[2]);
int mh_pcs_begin(mh_ctx* ctx, const mh_pcs_params* params, int n_trees, const mh_tree* const* trees, int n_points,
                 const uint64_t* points /* [n_points][2] */, mh_pcs** out);
void mh_pcs_free(mh_pcs* p);
int mh_pcs_shape(const mh_pcs* p, mh_pcs_shape_t* out);
int mh_pcs_evals(mh_pcs* p, uint64_t* evals_out /* [n_points][ood_width][2], transcript order */);
int mh_pcs_deep(mh_pcs* p, const uint64_t alpha[2], const uint64_t beta[2]);
/* Parity/debug: the DEEP layer Q, [2^log_lde_height][2] in DOMAIN order (index i <-> x = g * w_K^i); valid between deep and the
 * first fold. */
int mh_pcs_download_deep(mh_pcs* p, uint64_t* out);
int mh_pcs_fri_commit(mh_pcs* p, uint64_t root[4]);
int mh_pcs_fri_fold(mh_pcs* p, const uint64_t beta[2]);
int mh_pcs_fri_final(mh_pcs* p, uint64_t* coeffs_out);
/* The result holds only the hints, like mh_session_open. */
int mh_pcs_query(mh_pcs* p, const uint64_t* indices, size_t n_indices, mh_proof** out);
/* One shot with the library's transcript (all five configurations, like mh_prove), exactly open_with_channel's:
 *   for each point j in order: send_algebra_slice(point j's aligned evaluations);  grind deep_pow_bits;  sample alpha, then beta;
 *   per FRI round: send the commitment, grind folding_pow_bits, sample beta;  the final polynomial (descending degree);
 *   grind query_pow_bits;  num_queries x sample_bits(log_lde_height);  hint every input tree's batch opening in tree order, then every
 *   FRI round's;  finalize.
 * mh_proof_fields / mh_proof_commitments are the transcript, mh_proof_digest its digest; mh_proof_log_trace_heights lists the trees'
 * log heights (tallest matrix of each). */
int mh_pcs_open(mh_ctx* ctx, const mh_pcs_params* params, int n_trees, const mh_tree* const* trees, int n_points, const uint64_t* points,
                const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe, mh_proof** out);
/* verify_aligned.  Host only: no GPU, no ctx.  roots: [n_trees][4]; log_tree_heights[t]: log2 of the rows of tree t's tallest matrix
 * (its depth is that + params->log_blowup); n_mats[t] matrices per tree, whose UNPADDED widths follow each other in `widths`, all trees
 * flat; salt_elems: the salt width the trees were committed with (0: the plain LMCS).  MH_OK + the transcript digest + (evals_out not
 * NULL) the evaluations with the alignment padding dropped, [n_points][sum of the widths][2]; or MH_ERR_INVALID with the reason in
 * `err`: a malformed or truncated stream, trailing data, a non-canonical felt, a point on H or gK, n_points or n_trees out of range,
 * an opening that does not match its root, a DEEP / FRI inconsistency. */
int mh_pcs_verify(int lmcs, int salt_elems, const mh_pcs_params* params, int n_trees, const uint64_t* roots,
                  const uint8_t* log_tree_heights, const int* n_mats, const size_t* widths, int n_points, const uint64_t* points,
                  const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe, const uint64_t* fields,
                  size_t n_fields, const uint64_t* commitments, size_t n_commitments, uint64_t* evals_out, uint64_t digest[4], char* err,
                  size_t err_cap);
/* The session's input trees in group order [preprocessed?, main, aux, quotient] (prover/mod.rs:552-560), BORROWED until
 * mh_session_free (the preprocessed tree: until its owner frees it); valid once the quotient is committed.  *n_trees = their number;
 * MH_ERR_INVALID if cap is smaller. */
int mh_session_trees(const mh_session* s, const mh_tree** out, int cap, int* n_trees);

/* ---- verifier (host only: no GPU, no ctx) ---------------------------------------------------------------------
 * Replays a proof against the AIRs' constraint-DAG blobs: crates/lifted-stark/src/verifier/mod.rs (flow, constraint
 * identity), pcs/verifier.rs + lmcs/config.rs:172-211 (openings), pcs/deep/verifier.rs, pcs/fri/verifier.rs.
 * Inputs mirror mh_prove: AIR blobs and log heights in INSTANCE order, the same challenger state / pre-observed
 * felts, and the proof's two streams (mh_proof_fields / mh_proof_commitments).  MH_OK + the transcript digest, or
 * MH_ERR_INVALID with the reason in `err`. */
int mh_verify(const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs, const size_t* air_blob_words,
              const uint8_t* log_trace_heights, const uint64_t* public_values, size_t n_public_values,
              const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe,
              const uint64_t* fields, size_t n_fields, const uint64_t* commitments, size_t n_commitments,
              const uint64_t* preprocessed_root /* [4]: the setup commitment, NULL if no AIR has preprocessed columns */,
              uint64_t digest[4], char* err, size_t err_cap);
/* Statement::eval_external (crates/lifted-air/src/statement.rs:94-108; MultiAir::eval_external, crates/lifted-air/src/air.rs:247-287):
 * the statement's cross-AIR assertions, checked by the reference verifier as its step 11 (crates/lifted-stark/src/verifier/mod.rs:
 * 488-501, ExternalAssertionFailed) and by its prover before the aux commitment is used (prover/mod.rs:383-399).  The AIRs of this
 * library are data (constraint DAGs); a statement-level hook is code, so it is a callback: it receives the shared challenges
 * (n_randomness EF values), every instance's committed aux values and the log heights, all in INSTANCE order, writes one EF value
 * (c0, c1) per assertion into assertions_out (room for `cap`) and returns their number, or a negative value for the reference's
 * ReductionError.  mh_verify_ex rejects the proof unless every value is zero.  mh_verify == mh_verify_ex(external = NULL) verifies a
 * statement WITHOUT cross-AIR assertions (the default MultiAir): a caller whose statement has some -- every LogUp / bus statement,
 * e.g. Miden's "sum of the committed finals plus boundary corrections = 0" (air/src/lib.rs:854-1000) -- MUST use mh_verify_ex;
 * with mh_verify the bus balance is unchecked.  On the proving side the same check belongs in the `mh_aux_builder` callback /
 * after mh_session_commit_aux, which hand the aux values to the caller for exactly this purpose. */
typedef int (*mh_external_assertions)(void* user, const uint64_t* randomness, size_t n_randomness, const uint64_t* const* aux_values,
                                      const size_t* n_aux_values, const uint8_t* log_trace_heights, int n_airs, uint64_t* assertions_out,
                                      size_t cap);
int mh_verify_ex(const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs, const size_t* air_blob_words,
                 const uint8_t* log_trace_heights, const uint64_t* public_values, size_t n_public_values,
                 const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe, const uint64_t* fields,
                 size_t n_fields, const uint64_t* commitments, size_t n_commitments, const uint64_t* preprocessed_root,
                 mh_external_assertions external, void* external_user, uint64_t digest[4], char* err, size_t err_cap);
/* mh_verify_ex under any of the five configurations: lmcs = MH_LMCS_* (prover/src/lib.rs:246-300 dispatches the same five). */
int mh_verify_lmcs(int lmcs, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs, const size_t* air_blob_words,
                   const uint8_t* log_trace_heights, const uint64_t* public_values, size_t n_public_values,
                   const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe, const uint64_t* fields,
                   size_t n_fields, const uint64_t* commitments, size_t n_commitments, const uint64_t* preprocessed_root,
                   mh_external_assertions external, void* external_user, uint64_t digest[4], char* err, size_t err_cap);
/* mh_verify_lmcs for a proof made under a hiding LMCS (mh_ctx_set_salt, salt_elems = 0 .. MH_MAX_SALT_ELEMS): every opened leaf of every
 * tree -- preprocessed, main, aux, quotient, each FRI round -- is read as `rows + salt` and the salt is absorbed last
 * (lmcs/proof.rs:108-137).  preprocessed_root is the root of the SALTED setup tree.  salt_elems = 0 is mh_verify_lmcs. */
int mh_verify_hiding(int lmcs, int salt_elems, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs,
                     const size_t* air_blob_words, const uint8_t* log_trace_heights, const uint64_t* public_values, size_t n_public_values,
                     const uint64_t challenger_state[12], const uint64_t* pre_observe, size_t n_pre_observe, const uint64_t* fields,
                     size_t n_fields, const uint64_t* commitments, size_t n_commitments, const uint64_t* preprocessed_root,
                     mh_external_assertions external, void* external_user, uint64_t digest[4], char* err, size_t err_cap);
/* A ready-made mh_external_assertions: one assertion, the sum over the instances of their aux value 0 (the LogUp accumulator
 * final, `committed_finals` of air/src/lookup/aux_builder.rs) -- the balance of a bus statement with no boundary corrections. */
int mh_external_logup_balance(void* user, const uint64_t* randomness, size_t n_randomness, const uint64_t* const* aux_values,
                              const size_t* n_aux_values, const uint8_t* log_trace_heights, int n_airs, uint64_t* assertions_out,
                              size_t cap);
/* A ready-made mh_external_assertions for the second client: `ChipletMultiAir::eval_external` of the precompile prover's session
 * (precompiles-prover/src/session/prove.rs:243-256) = the sum of the committed sigmas + `fixed_boundary_correction` (:205-216), the
 * verifier's consumes of the session's fixed environment (session/fixed.rs: the VM-owned curve group's `EcGroup` tuple, the five fixed
 * uints' `UintVal` tuples).  Every AIR must expose exactly one aux value (its sigma): any other shape returns -1.  `user` is unused.
 * `mh_external_precompile_session_ec_only` is the reduced form for statements that leave the uint store out (the EcGroup part of the
 * correction only) -- a callback of its own name so that the real statement cannot be weakened by a flag passed by mistake. */
int mh_external_precompile_session(void* user, const uint64_t* randomness, size_t n_randomness, const uint64_t* const* aux_values,
                                   const size_t* n_aux_values, const uint8_t* log_trace_heights, int n_airs, uint64_t* assertions_out,
                                   size_t cap);
int mh_external_precompile_session_ec_only(void* user, const uint64_t* randomness, size_t n_randomness, const uint64_t* const* aux_values,
                                           const size_t* n_aux_values, const uint8_t* log_trace_heights, int n_airs,
                                           uint64_t* assertions_out, size_t cap);

/* ---- LMCS openings checked on their own, and the batch verifier --------------------------------------------------------------------
 * mh_lmcs_verify is the counterpart of mh_tree_open (the reference's Lmcs::open_batch, lmcs/config.rs:172-211): HOST ONLY, no context.
 * An opening = the root, the tree's log height (= depth: log2 of its leaves, the LDE height), the UNALIGNED widths of its matrices in
 * commitment order, the row alignment the opening was made with, the opened indices (any order, duplicates allowed, as mh_tree_open
 * takes them) and the two streams exactly as mh_tree_open wrote them.  salt_elems = mh_tree_salt_elems of the tree.
 * MH_OK, or MH_ERR_INVALID + a reason in err (may be NULL): a stream too short or with trailing data, a non-canonical felt (under the
 * byte-hash configurations a digest word is not a felt and is not checked), an index outside the tree, an unknown lmcs, salt outside
 * 0..MH_MAX_SALT_ELEMS, no index, more than 4096 matrices, a width or alignment above 2^20, or "Merkle root mismatch". */
typedef struct mh_lmcs_opening {
  uint64_t root[4];
  int log_height;
  int n_mats;
  const size_t* widths; /* [n_mats], unaligned */
  size_t alignment;     /* 8 / 17 (Keccak) / 1 (Blake3) for a proof's trees; whatever mh_tree_open was given otherwise */
  const uint64_t* indices;
  size_t n_indices;
  const uint64_t* fields; /* per sorted unique index: every matrix's aligned row, then the salt */
  size_t n_fields;
  const uint64_t* commitments; /* the sibling digests that cannot be derived, bottom-up, left to right; 4 words each */
  size_t n_commit_felts;
} mh_lmcs_opening;
int mh_lmcs_verify(int lmcs, int salt_elems, const mh_lmcs_opening* o, char* err, size_t err_cap);
/* The same for n openings on the DEVICE: every leaf of every opening is hashed by one kernel (one lane per leaf, leaves of one shape
 * per wave), every path by a second one (one workgroup per opening, the levels in LDS) -- a constant number of launches per batch,
 * one read-back.  ok[i] = 1 iff mh_lmcs_verify accepts items[i]; an opening the host checks refuse (lengths, indices, felts) gets 0
 * without reaching the device.  Device memory per pass is bounded by the environment variable MH_VERIFY_BATCH_BYTES (default 256 MB):
 * a larger batch runs as consecutive chunks.  Call-level failures only in the return value: null arguments, a HIP error, and
 * MH_ERR_INVALID for an opening of more than 1024 distinct leaves or a matrix wider than 32764 cells (the kernels' bounds: use the
 * host call for those); the reason is mh_last_error's.  n = 0 is MH_OK. */
int mh_lmcs_verify_batch(mh_ctx* ctx, int lmcs, int salt_elems, size_t n, const mh_lmcs_opening* items, int* ok);

/* ---- an opening read back as a Merkle witness (the reference's BatchProofView / MerkleWitness, lmcs/proof.rs:42-80) -----------------
 * What the verifier of an opening derives on its way to the root, kept: for depth = log_height and the k DISTINCT opened indices
 * i_0 < ... < i_{k-1}, three arrays of 4-word digests, packed as mh_tree_root packs them:
 *   leaf_digests[k][4]      the hash of opened leaf q (its aligned rows, then its salt), ascending index order;
 *   paths[k][depth][4]      paths[q][l] = the digest of node (i_q >> l) ^ 1 on level l above the leaves, bottom to top
 *                           (MerkleWitness::path(i_q)): a streamed sibling where the proof carries one, otherwise a leaf digest or a
 *                           derived node of the same opening;
 *   nodes[n_nodes][4]       every derived parent, level by level from the leaves' parents up, ascending position within a level;
 *                           node j of level l is the j-th distinct value of i >> (l + 1); the last entry is the root.
 * depth 0: k = 1, no path element, no node, leaf_digests[0] is the root.
 * mh_lmcs_witness_size: shape only (k and n_nodes) from log_height and the indices, which may come in any order and with duplicates;
 * it refuses what mh_lmcs_verify's index checks refuse, with the same reason.
 * mh_lmcs_witness: HOST ONLY.  MH_OK exactly when mh_lmcs_verify accepts the same arguments; otherwise its code and its reason, and
 * nothing is written to the buffers.  `nodes` may be NULL; a NULL leaf_digests or paths (depth > 0) is refused. */
int mh_lmcs_witness_size(const mh_lmcs_opening* o, size_t* n_leaves, size_t* n_nodes, char* err, size_t err_cap);
int mh_lmcs_witness(int lmcs, int salt_elems, const mh_lmcs_opening* o, uint64_t* leaf_digests, uint64_t* paths, uint64_t* nodes /* or NULL */,
                    char* err, size_t err_cap);
/* The same for n openings on the DEVICE, in mh_lmcs_verify_batch's passes: the leaf kernel's digests are kept, and a witness form of
 * the path kernel stores every parent and copies every path element while it walks the levels.  One read-back per pass, in the final
 * layout.  outs[i] = the caller's buffers for items[i], sized by mh_lmcs_witness_size (nodes may be NULL).  ok[i] = 1 iff
 * mh_lmcs_witness accepts items[i] and then outs[i] holds what it writes; for ok[i] = 0 the item's buffers are untouched.  Call-level
 * refusals, kernel bounds and MH_VERIFY_BATCH_BYTES as mh_lmcs_verify_batch. */
typedef struct mh_lmcs_witness_out {
  uint64_t* leaf_digests;
  uint64_t* paths;
  uint64_t* nodes; /* or NULL */
} mh_lmcs_witness_out;
int mh_lmcs_witness_batch(mh_ctx* ctx, int lmcs, int salt_elems, size_t n, const mh_lmcs_opening* items, const mh_lmcs_witness_out* outs, int* ok);

/* mh_verify_hiding for MANY proofs of one statement shape: the AIR list, the parameters, the challenger state and the external
 * assertions are the batch's, an item carries what differs per proof.  For a node that sits beside the provers and accepts many
 * proofs before it aggregates them; a verifier box without a GPU keeps mh_verify*.  Each item is replayed on the host (transcript,
 * constraint identity, DEEP and FRI algebra, proof of work: up to 16 threads, so `external` is called from several threads at once,
 * each call with its item's external_user) while its LMCS openings are only recorded; then ONE device pass hashes every recorded
 * opening of every item (the two kernels of mh_lmcs_verify_batch).  A replay that fails keeps the openings it recorded before the
 * failure, because they come earlier in the proof: a damaged opened row fails its tree's root in mh_verify_hiding, and fails the
 * algebra behind the opening only here, where the hashing is postponed.
 * Verdict: results[i].code = MH_OK iff the replay succeeded and all openings verified, else MH_ERR_INVALID; accept / reject equals
 * mh_verify_hiding's on the same item in every case, and an accepted item's digest is its digest.  The REASON: a failed opening
 * reads "proof rejected: Merkle root mismatch (<tree>)" with <tree> = "committed tree t of n" in the order [preprocessed?, main,
 * aux, quotient] or "FRI round r tree", the first failed one of the item; otherwise the replay's reason stands.  It is
 * mh_verify_hiding's reason (plus the tree) except for a proof with more than one defect, where an opening recorded before the
 * replay's failure wins even if mh_verify_hiding meets another defect first.  An item with more than 1024 distinct query indices is rejected with
 * a reason (the path kernel's bound).  The return value is for call-level failures only (null arguments, malformed AIR blobs, a HIP
 * error); n_items = 0 is MH_OK.  When to prefer the host call: measured on the Miden statement of a 2^16-row program (DESIGN.md
 * section 3j), a single proof gains 0.3 ms of 1.7 under Poseidon2 and nothing under Blake3 (0.37 against 0.39 ms); from 8 proofs on
 * the batch is 3 to 20 times faster per proof, under Blake3 through the replay threads rather than the device.
 * Not there yet: batch forms of mh_verify_precompile and mh_pcs_verify (they go through the same recorded openings), sharded contexts. */
typedef struct mh_verify_item {
  const uint8_t* log_trace_heights; /* [n_airs], instance order */
  const uint64_t* public_values;
  size_t n_public_values;
  const uint64_t* pre_observe;
  size_t n_pre_observe;
  const uint64_t* fields;
  size_t n_fields;
  const uint64_t* commitments;
  size_t n_commitments;              /* digests */
  const uint64_t* preprocessed_root; /* [4] or NULL */
  void* external_user;
} mh_verify_item;
typedef struct mh_verify_result {
  int code; /* MH_OK or MH_ERR_INVALID */
  uint64_t digest[4];
  char reason[216]; /* "" when accepted */
} mh_verify_result;
int mh_verify_batch(mh_ctx* ctx, int lmcs, int salt_elems, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs,
                    const size_t* air_blob_words, const uint64_t challenger_state[12], mh_external_assertions external, size_t n_items,
                    const mh_verify_item* items, mh_verify_result* results);
/* mh_verify_batch that also hands back what it derived: verdicts, digests and reasons are exactly mh_verify_batch's, and *out
 * receives a set (free it with mh_witness_set_free) that holds, for every ACCEPTED item, one witness (mh_lmcs_witness*) per LMCS
 * opening of the proof, in proof order: the committed trees [preprocessed?, main, aux, quotient], then FRI round 0, 1, ...  A rejected
 * item carries none.  This is what a recursive verifier's advice needs per tree: a leaf hash and a Merkle path per query, the inner
 * nodes, and the opened rows behind every leaf hash.  Every pointer of a view points into memory the set owns, `rows` included (a
 * copy of the proof's field stream: the set outlives the caller's buffers).  On a call-level failure *out is NULL. */
typedef struct mh_witness_set mh_witness_set;
typedef struct mh_witness_tree {
  int kind;  /* 0: a committed tree, 1: an FRI round tree */
  int which; /* which tree of that kind */
  int depth;
  size_t n_leaves, n_nodes, row_len; /* row_len: felts per opened leaf (every matrix's aligned row, then the salt) */
  uint64_t root[4];
  const uint64_t* indices;      /* [n_leaves], ascending */
  const uint64_t* rows;         /* [n_leaves][row_len] */
  const uint64_t* leaf_digests; /* [n_leaves][4] */
  const uint64_t* paths;        /* [n_leaves][depth][4] */
  const uint64_t* nodes;        /* [n_nodes][4] */
} mh_witness_tree;
int mh_verify_batch_witness(mh_ctx* ctx, int lmcs, int salt_elems, const mh_pcs_params* params, int n_airs, const uint64_t* const* air_blobs,
                            const size_t* air_blob_words, const uint64_t challenger_state[12], mh_external_assertions external, size_t n_items,
                            const mh_verify_item* items, mh_verify_result* results, mh_witness_set** out);
size_t mh_witness_set_trees(const mh_witness_set* set, size_t item); /* 0 for a rejected item or an item out of range */
int mh_witness_set_tree(const mh_witness_set* set, size_t item, size_t t, mh_witness_tree* view);
void mh_witness_set_free(mh_witness_set* set);

/* ---- the precompile prover's session: SessionTraces::prove_stark's own shape (precompiles-prover/src/session/prove.rs:295-330, 385-416)
 * Twelve main traces + the transcript root in, proof out -- the statement layer `ChipletMultiAir` adds to the proof system, in the
 * library (csrc/precompile.cpp) so that a C caller restates nothing:
 *   - the twelve AIRs of `ChipletAir::all()` (session/prove.rs:111-126: ChunkNode, Poseidon2, KeccakRound, BytePairLut, KeccakSponge,
 *     TranscriptEval, UintStoreMul, UintAdd, EcGroups, EcPointStore, EcGroupAdd, EcMsm) with their lookup programs, embedded as the
 *     blobs of miden-vm_amd/blobs/precompile; every aux column (LogUp sums and UintStoreMul's three registers) is built on the device;
 *   - BytePairLutAir's preprocessed 2^16 x 4 table (primitives/byte_pair_lut.rs:262-277), generated by mh_precompile_load and
 *     committed once per hash function, on first use (the reference's session/preprocessed_cache.rs);
 *   - `precompile_pcs_params()` (stark_config.rs:60-71), the placeholder relation digest 0^4 (session/prove.rs:40), the transcript
 *     prefix `observe_protocol_params` | preprocessed commitment | len(air_inputs) = 4, the root, 0, 0 (the default `MultiAir::observe`,
 *     crates/lifted-air/src/air.rs:307-324);
 *   - `ChipletMultiAir::eval_external` = mh_external_precompile_session.
 * mains_rowmajor[i]: AIR i's main trace, row-major, height 2^log_heights[i], width as the AIR declares (42, 32, 68, 3, 67, 39, 44,
 * 30, 6, 14, 21, 38), canonical felts; index 3 (BytePairLut) has 2^16 rows.  public_root: the transcript root (`air_inputs`).
 * hash_fn = MH_LMCS_*. */
#define MH_PRECOMPILE_NUM_AIRS 12
#define MH_PRECOMPILE_PRE_OBSERVE_FELTS 19 /* 8 protocol parameters + 4 (preprocessed commitment) + 1 + 4 + 2 (statement framing) */
typedef struct mh_precompile mh_precompile; /* the twelve AIRs loaded on a context, lookups attached, the byte-pair table uploaded */
void mh_precompile_pcs_params(mh_pcs_params* out);
int mh_precompile_load(mh_ctx* ctx, mh_precompile** out);
void mh_precompile_free(mh_precompile* s);
/* the embedded blobs, for a caller that drives the generic entry points itself: lookup = 0 the constraint DAG, 1 the lookup program */
int mh_precompile_air_blob(int which, int lookup, const uint64_t** words_out, size_t* n_words);
/* the setup commitment of the byte-pair table under hash_fn, made on the device (on first use, then cached in `s`) */
int mh_precompile_preprocessed_root(mh_precompile* s, int hash_fn, uint64_t root[4]);
/* the same root derived on the HOST from the table itself (mh_commit_host at mh_precompile_pcs_params().log_blowup; the reference's
 * session/preprocessed_cache.rs): no context, no GPU.  Derived once per hash function and process (0.3 - 7 s by hasher), then kept; safe to
 * call from several threads.  This is the verifier's copy of the verifying key: mh_verify_precompile pins it. */
int mh_precompile_setup_root(int hash_fn, uint64_t root[4]);
int mh_precompile_pre_observe(const mh_pcs_params* p, const uint64_t preprocessed_root[4], const uint64_t public_root[4],
                              uint64_t out[MH_PRECOMPILE_PRE_OBSERVE_FELTS]);
int mh_prove_precompile(mh_ctx* ctx, mh_precompile* s, int hash_fn, const uint64_t* const mains_rowmajor[MH_PRECOMPILE_NUM_AIRS],
                        const int log_heights[MH_PRECOMPILE_NUM_AIRS], const uint64_t public_root[4], mh_proof** out);
/* the same over device-resident traces, in `ChipletAir::all()` order */
int mh_prove_precompile_traces(mh_ctx* ctx, mh_precompile* s, int hash_fn, mh_trace* const traces[MH_PRECOMPILE_NUM_AIRS],
                               const uint64_t public_root[4], mh_proof** out);
/* `verify_stark` (session/prove.rs:365-383, 386-425): StarkProofData bytes -> MH_OK + the transcript digest, or MH_ERR_INVALID + reason.
 * Host only (no context, no GPU).  The setup commitment of the byte-pair table is part of the statement and the verifier derives it
 * itself (mh_precompile_setup_root, as the reference's verifier recomputes it from the table): preprocessed_root = NULL is the normal
 * call.  A non-NULL preprocessed_root is CHECKED against the derived root before any proof byte is read; one that differs -- a root
 * forwarded from a prover who committed another table -- is MH_ERR_INVALID with a reason that names the setup commitment. */
int mh_verify_precompile(int hash_fn, const uint64_t preprocessed_root[4] /* or NULL */, const uint64_t public_root[4], const uint8_t* proof_bytes,
                         size_t n_bytes, uint64_t digest[4], char* err, size_t err_cap);

/* ---- the Miden VM statement: prove_stark's own shape (prover/src/lib.rs:317-355) --------------------------------------------------
 * Three matrices + 32 public values + aux inputs in, proof out -- the statement layer the reference's `MidenMultiAir` adds to the
 * proof system, in the library (csrc/miden.cpp) so that a C caller restates nothing:
 *   - the three AIRs [CoreAir, ChipletsAir, Poseidon2PermutationAir] (air/src/lib.rs:560-650) with their LogUp lookup programs, embedded
 *     as the blobs of miden-vm_amd/blobs (all eight aux columns are built on the device);
 *   - `MidenMultiAir::observe` (air/src/lib.rs:805-849): [kernel_H | program_hash] [deferred_root | 0^4] [stack inputs 16] [stack
 *     outputs 16], kernel_H = hash_kernel_digests (:946-961) = Poseidon2 hash_elements of the kernel-digest felts;
 *   - `MidenMultiAir::eval_external` (:854-933): the three committed LogUp finals + the boundary corrections (block-hash seed,
 *     deferred-root log, one KernelRomInit per kernel digest) must vanish -- mh_verify_miden checks it, no proof of this statement
 *     verifies without it;
 *   - pcs_params() and RELATION_DIGEST of air/src/config.rs:54-67, 93-98; hash_fn = MH_LMCS_* as `prove_miden_vm_execution_trace`
 *     dispatches on ProvingOptions::hash_fn (prover/src/lib.rs:246-300).
 * public_values: stack inputs (16) ++ stack outputs (16).  aux_inputs: program hash (4) | deferred root (4) | kernel procedure
 * digests (4 each, at most 255).  Matrices row-major, heights 2^log_*, widths 51 / 22 / 16, canonical felts. */
#define MH_MIDEN_NUM_PUBLIC_VALUES 32
#define MH_MIDEN_PRE_OBSERVE_FELTS 56 /* 8 protocol parameters + the 48-felt statement schedule */
typedef struct mh_miden mh_miden; /* the three AIRs loaded on a context, lookups attached */
int mh_miden_load(mh_ctx* ctx, mh_miden** out);
void mh_miden_free(mh_miden* m);
int mh_prove_miden(mh_ctx* ctx, const mh_miden* m, int hash_fn, const uint64_t* core_rowmajor, int log_core,
                   const uint64_t* chiplets_rowmajor, int log_chiplets, const uint64_t* poseidon2_rowmajor, int log_poseidon2,
                   const uint64_t* public_values /* [32] */, const uint64_t* aux_inputs, size_t n_aux_inputs, mh_proof** out);
/* the same over device-resident traces (mh_trace_upload* / mh_trace_from_device), instance order core, chiplets, poseidon2 */
int mh_prove_miden_traces(mh_ctx* ctx, const mh_miden* m, int hash_fn, mh_trace* const traces[3], const uint64_t* public_values,
                          const uint64_t* aux_inputs, size_t n_aux_inputs, mh_proof** out);
/* verifier/src/lib.rs:320-330 for this statement: StarkProofData bytes -> MH_OK + the transcript digest, or MH_ERR_INVALID + reason.
 * Host only (no context, no GPU). */
int mh_verify_miden(int hash_fn, const uint64_t* public_values /* [32] */, const uint64_t* aux_inputs, size_t n_aux_inputs,
                    const uint8_t* proof_bytes, size_t n_bytes, uint64_t digest[4], char* err, size_t err_cap);
/* mh_verify_miden for n proofs through mh_verify_batch: per proof the arguments of mh_verify_miden; results[i] as mh_verify_batch
 * fills them (accept / reject and digest = mh_verify_miden's).  Malformed bytes or inputs reject that item alone. */
typedef struct mh_miden_verify_item {
  const uint64_t* public_values; /* [32] */
  const uint64_t* aux_inputs;
  size_t n_aux_inputs;
  const uint8_t* proof_bytes;
  size_t n_bytes;
} mh_miden_verify_item;
int mh_verify_miden_batch(mh_ctx* ctx, int hash_fn, size_t n, const mh_miden_verify_item* items, mh_verify_result* results);
/* the same through mh_verify_batch_witness: set item i = proof i (none for an item rejected before or in the batch) */
int mh_verify_miden_batch_witness(mh_ctx* ctx, int hash_fn, size_t n, const mh_miden_verify_item* items, mh_verify_result* results,
                                  mh_witness_set** out);
/* the pieces, for a caller that drives mh_prove / mh_session_* / mh_verify_ex itself */
void mh_miden_pcs_params(mh_pcs_params* out);
void mh_miden_challenger_state(uint64_t state[12]);
int mh_miden_hash_kernel_digests(const uint64_t* kernel_felts, size_t n_felts, uint64_t out[4]);
int mh_miden_pre_observe(const mh_pcs_params* params, const uint64_t* public_values, const uint64_t* aux_inputs, size_t n_aux_inputs,
                         uint64_t out[MH_MIDEN_PRE_OBSERVE_FELTS]);
/* randomness = (alpha, beta) as 4 felts; aux_values[i] = the i-th AIR's committed values (2 felts each); out = the one assertion */
int mh_miden_eval_external(const uint64_t randomness[4], const uint64_t* aux_inputs, size_t n_aux_inputs,
                           const uint64_t* const* aux_values, const size_t* n_aux_values, int n_airs, uint64_t out[2]);
int mh_miden_air_blob(int which /* 0 core, 1 chiplets, 2 poseidon2 */, const uint64_t** words_out, size_t* n_words);

void mh_proof_free(mh_proof* p);
size_t mh_proof_num_fields(const mh_proof* p);
size_t mh_proof_num_commitments(const mh_proof* p);
const uint64_t* mh_proof_fields(const mh_proof* p);       /* TranscriptData::fields */
const uint64_t* mh_proof_commitments(const mh_proof* p);  /* TranscriptData::commitments, 4 felts each.  Either pointer may be NULL when its
                                                             count is 0 (mh_session_open of openings that need no sibling) */
const uint64_t* mh_proof_digest(const mh_proof* p);       /* StarkOutput::digest, 4 felts */
size_t mh_proof_num_traces(const mh_proof* p);
const uint8_t* mh_proof_log_trace_heights(const mh_proof* p);
/* Serialise StarkProofData; returns the byte length needed (writes only if cap is large enough). */
size_t mh_proof_serialize(const mh_proof* p, uint8_t* out, size_t cap);
/* The inverse: StarkProofData bytes -> proof (what verifier/src/lib.rs:320-330 does first; 64 MiB limit).  MH_ERR_INVALID on
 * truncated input, trailing bytes, oversized length prefixes or non-canonical field elements.  The digest is not part of
 * StarkProofData and comes back zeroed (mh_verify recomputes it). */
int mh_proof_deserialize(const uint8_t* bytes, size_t len, mh_proof** out);

/* ---- constraint checker: ExecutionTrace::check_constraints / SessionTraces::check (crates/lifted-stark/src/debug.rs) ---------------
 * Evaluates every constraint of an AIR on every row of a trace, on the device, and reports which constraints fail where -- a debugging
 * tool for witness generators, not part of any proof (no Fiat-Shamir transcript; the statement entries derive debug challenges).
 * Two stages (csrc/check.hip): the screen folds every constraint with a fresh random alpha per call and flags the rows where the fold does
 * not vanish (a failing row escapes with probability <= K / p^2); the exact stage then evaluates each constraint on those rows with the
 * reference's debug selectors (is_first = [r == 0], is_last = [r == n-1], is_transition = [r != n-1], next row = (r + 1) mod n).
 * MH_CHECK_EXACT skips the screen and evaluates every constraint on every row.
 * MH_OK: every constraint and every external assertion vanishes.  MH_ERR_UNSATISFIED: they do not; mh_last_error names the first entry.
 * *n_entries = the number of entries, even when it exceeds cap; the first cap are written, ordered by (instance, first_row,
 * constraint), external assertions last. */
#define MH_ERR_UNSATISFIED 6 /* mh_check_*: the trace does not satisfy the statement; the entries say where */
#define MH_CHECK_EXACT 1     /* flags: evaluate every constraint on every row (no fold screen) */
typedef struct mh_check_entry {
  int32_t instance;    /* AIR instance in the statement's instance order; -1: an external (cross-AIR) assertion */
  uint32_t constraint; /* constraint index in the DAG (= the reference's emission order); external: assertion index */
  uint64_t rows;       /* rows on which it does not vanish (external: 1) */
  uint64_t first_row;  /* the smallest such row (external: 0) */
  uint64_t value[2];   /* its value there, EF (c1 = 0 for a base-field constraint) */
} mh_check_entry;
/* One AIR over one trace (instance 0 in the entries).  aux: the aux trace (2 * aux_width base columns, as mh_lookup_build_aux makes it),
 * required when the AIR has aux columns; preprocessed: the raw preprocessed matrix, or NULL for the one attached to the AIR.
 * randomness / aux_values: EF pairs, at least as many as the AIR reads.  failing_rows: NULL, or room for 2^log_n + 1 words:
 * [0] = the number m of rows on which some constraint fails, [1..m] = those rows, ascending. */
int mh_check_constraints(mh_ctx* ctx, const mh_air* air, const mh_trace* main_trace, const mh_trace* aux /* or NULL */,
                         const mh_trace* preprocessed /* or NULL */, const uint64_t* public_values, size_t n_public,
                         const uint64_t* randomness /* EF pairs */, size_t n_randomness, const uint64_t* aux_values /* EF pairs */,
                         size_t n_aux_values, int flags, mh_check_entry* out, size_t cap, size_t* n_entries, uint64_t* failing_rows);
/* Test and diagnostic entry, like mh_pcs_download_deep: the screen's fold itself, with the caller's alpha instead of a fresh random one.
 * out [2^log_n][2] receives F(r) = sum_k alpha^(K-1-k) C_k(r) as canonical EF pairs, one per row, computed by the AIR's own constraint
 * program (compiled chunks or interpreter, whichever mh_air_load chose) on the trace domain with the screen's selector values:
 * is_first = [r == 0], is_last = [r == n-1], is_transition = w_n^r - w_n^-1 (zero on the last row only; w_n the generator of the trace
 * domain), next row = (r + 1) mod n.  Arguments and their checks as mh_check_constraints. */
int mh_constraint_fold(mh_ctx* ctx, const mh_air* air, const mh_trace* main_trace, const mh_trace* aux /* or NULL */,
                       const mh_trace* preprocessed /* or NULL */, const uint64_t* public_values, size_t n_public,
                       const uint64_t* randomness /* EF pairs */, size_t n_randomness, const uint64_t* aux_values /* EF pairs */,
                       size_t n_aux_values, const uint64_t alpha[2], uint64_t* out);
/* The statements: the arguments of the provers without hash_fn.  Aux columns are built on the device by the attached lookup programs with
 * debug challenges: a Poseidon2 duplex challenger started from the statement's challenger state observes the pre-observe schedule
 * (mh_miden_pre_observe; mh_precompile_pre_observe with 0^4 for the preprocessed commitment), the number of AIRs and their log heights
 * in instance order, then samples the lookup challenges -- the transcript order of a proof up to the main commitment, which it omits.
 * Then the statement's eval_external and every instance are checked. */
int mh_check_miden(mh_ctx* ctx, const mh_miden* m, const uint64_t* core_rowmajor, int log_core, const uint64_t* chiplets_rowmajor,
                   int log_chiplets, const uint64_t* poseidon2_rowmajor, int log_poseidon2, const uint64_t* public_values /* [32] */,
                   const uint64_t* aux_inputs, size_t n_aux_inputs, int flags, mh_check_entry* out, size_t cap, size_t* n_entries);
int mh_check_miden_traces(mh_ctx* ctx, const mh_miden* m, mh_trace* const traces[3], const uint64_t* public_values,
                          const uint64_t* aux_inputs, size_t n_aux_inputs, int flags, mh_check_entry* out, size_t cap, size_t* n_entries);
int mh_check_precompile(mh_ctx* ctx, mh_precompile* s, const uint64_t* const mains_rowmajor[MH_PRECOMPILE_NUM_AIRS],
                        const int log_heights[MH_PRECOMPILE_NUM_AIRS], const uint64_t public_root[4], int flags, mh_check_entry* out,
                        size_t cap, size_t* n_entries);
int mh_check_precompile_traces(mh_ctx* ctx, mh_precompile* s, mh_trace* const traces[MH_PRECOMPILE_NUM_AIRS], const uint64_t public_root[4],
                               int flags, mh_check_entry* out, size_t cap, size_t* n_entries);

/* ---- bus balance: unmatched LogUp messages (air/src/lookup/debug/trace/mod.rs:44-95,161-189 check_trace_balance / BalanceReport /
 * Unmatched / PushRecord; folded over a whole statement as precompiles-prover/src/tests/bus_balance.rs:25-108 does) -----------------
 * Every constraint of every AIR holds on a trace whose buses do not balance; mh_check_* then reports one external entry and nothing
 * else.  mh_check_balance* says WHICH messages are unmatched: it nets the multiplicities of all live pushes (canonical multiplicity
 * != 0) of all instances plus the statement's boundary pushes per encoded denominator, and reports every denominator whose net
 * multiplicity is not zero, with the pushes (instance, row, column, fraction, multiplicity) that landed on it.  Device stage:
 * csrc/balance.hip, over the planes the lookup programs write (the aux traces are not built).
 * Two stages: the screen sums m / d over all pushes and returns MH_OK when the sum is zero (unbalanced buses escape with probability
 * about #pushes / p^2 over the challenges); otherwise, or under MH_CHECK_EXACT, the exact stage nets the pushes in an open-addressing
 * table in device memory (load factor <= 1/2, 64-bit atomics only) and assembles the report.
 * MH_OK: balanced.  MH_ERR_UNSATISFIED: not; mh_last_error names the first entry.  A live push whose denominator is zero is
 * MH_ERR_INVALID.  *n_entries / *n_pushes = the exact totals, even when they exceed the caps; the first entry_cap / push_cap are written.
 * Entries ascend by (denom[0], denom[1]); the push list holds the pushes of entry 0, then of entry 1, ..., each entry's pushes by
 * (instance, row, column, fraction) with the boundary pushes (instance -1) last.  Two calls on the same input return the same bytes.
 * At most 2^22 pushes are collected: when the entries' pushes are more, the entries come back complete (`pushes` exact) but with
 * first_push = MH_BALANCE_NO_PUSHES and nothing is written to the push list; *n_pushes is still the exact total.
 * Not in scope: PushRecord::msg_repr (the lookup blob does not carry payloads), MutualExclusionViolation (it does not carry groups),
 * collect_column_oracle_folds. */
#define MH_BALANCE_NO_PUSHES UINT64_MAX /* mh_balance_entry.first_push: the push list was not collected (internal bound) */
typedef struct mh_balance_entry {   /* reference: Unmatched */
  uint64_t denom[2];       /* canonical encoded denominator */
  uint64_t net[2];         /* net signed multiplicity mod p (c1 = 0 for base-field multiplicities) */
  uint64_t pushes;         /* live pushes that landed on it, exact */
  uint64_t first_push;     /* index of its first push in the push list (entry order, then push order) */
} mh_balance_entry;
typedef struct mh_balance_push {    /* reference: PushRecord without msg_repr */
  int32_t instance;        /* -1: a boundary push of the statement */
  uint32_t column;         /* LogUp column of the lookup program (boundary: 0) */
  uint32_t fraction;       /* index within the column, program order (boundary: index in the statement's boundary list) */
  uint64_t row;
  uint64_t multiplicity[2];
} mh_balance_push;
/* Any set of lookup programs over their traces.  preprocessed: NULL, or per instance the raw preprocessed matrix (NULL where the
 * program reads none).  randomness: EF pairs, at least as many as every program reads.  Boundary pushes: boundary_denoms = n_boundary
 * EF pairs, boundary_signs = +1 / -1 each (the statement holds when sum_pushes m / d + sum_boundary sign / denom = 0). */
int mh_check_balance(mh_ctx* ctx, int n, const mh_lookup* const* lookups, const mh_trace* const* traces,
                     const mh_trace* const* preprocessed /* or NULL */, const uint64_t* randomness /* EF pairs */, size_t n_randomness,
                     const uint64_t* boundary_denoms /* EF pairs */, const int32_t* boundary_signs, size_t n_boundary, int flags,
                     mh_balance_entry* entries, size_t entry_cap, size_t* n_entries, mh_balance_push* pushes, size_t push_cap,
                     size_t* n_pushes);
/* The statements: the arguments and the debug challenges of mh_check_miden* / mh_check_precompile*.  Boundary pushes: the block-hash
 * seed, the two deferred-root terms and one KernelRomInit per kernel digest (MidenMultiAir::eval_external); the fixed EcGroup / UintVal
 * consumes of the session (`session_stack_residual`).  No state of mh_miden / mh_precompile is touched. */
int mh_check_balance_miden(mh_ctx* ctx, const mh_miden* m, const uint64_t* core_rowmajor, int log_core, const uint64_t* chiplets_rowmajor,
                           int log_chiplets, const uint64_t* poseidon2_rowmajor, int log_poseidon2, const uint64_t* public_values /* [32] */,
                           const uint64_t* aux_inputs, size_t n_aux_inputs, int flags, mh_balance_entry* entries, size_t entry_cap,
                           size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);
int mh_check_balance_miden_traces(mh_ctx* ctx, const mh_miden* m, mh_trace* const traces[3], const uint64_t* public_values,
                                  const uint64_t* aux_inputs, size_t n_aux_inputs, int flags, mh_balance_entry* entries, size_t entry_cap,
                                  size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);
int mh_check_balance_precompile(mh_ctx* ctx, mh_precompile* s, const uint64_t* const mains_rowmajor[MH_PRECOMPILE_NUM_AIRS],
                                const int log_heights[MH_PRECOMPILE_NUM_AIRS], const uint64_t public_root[4], int flags,
                                mh_balance_entry* entries, size_t entry_cap, size_t* n_entries, mh_balance_push* pushes, size_t push_cap,
                                size_t* n_pushes);
int mh_check_balance_precompile_traces(mh_ctx* ctx, mh_precompile* s, mh_trace* const traces[MH_PRECOMPILE_NUM_AIRS],
                                       const uint64_t public_root[4], int flags, mh_balance_entry* entries, size_t entry_cap,
                                       size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);

/* ---- multiplicity columns: the provider side of a table-style LogUp bus, counted on the device ---------------------------------------
 * Replaces the host-side ledgers the reference keeps next to its trace generators (precompiles-prover byte_pair_lut.rs:134-226,
 * uint/add/trace.rs:37-103 UintAddRequires, RangeChecker::emit_table_rows).  A multiplicity cell is the value that makes its key's net
 * zero; the lookup programs say who pushes what.  Inputs as mh_check_balance, plus the SLOTS: the fractions whose multiplicity is
 * affine in a main-trace column, m(r) = a(r) + b(r) * trace[r][main_column].  Device stage: csrc/multiplicity.hip.
 *   probe    every program of an instance with declared columns is evaluated on a scratch copy of its trace with all declared columns
 *            0 and again with all 1: a = m at 0, b = (m at 1) - (m at 0), key = d.  The declaration is checked numerically and
 *            refused (MH_ERR_INVALID, mh_last_error names instance / column / fraction) when a slot's denominator differs between
 *            the two evaluations, when a slot's b is not a base-field value, when a fraction that is no slot differs between them (an
 *            undeclared reader of a declared column), when a slot indexes outside its program or trace, when two slots name the same
 *            (instance, lookup_column, fraction), or when a live push has a zero denominator.  A refused call leaves the traces as
 *            they were.
 *   net      one table for the statement: every push with a != 0 (other fractions: their m), every boundary push, and every slot
 *            push with b(r) != 0 -- a provider candidate, also when its a is 0.  Per key: net = sum of a mod p; owner = the candidate
 *            with the lowest push id (instance base + row * K + fraction, the numbering of mh_check_balance).
 *   resolve  per cell (instance, declared column, row): the first slot of that column in declaration order with b(r) != 0 decides.
 *            Its push owns its key: the cell becomes -net[0] / b(r) mod p, canonical.  It does not: 0.  No such slot on the row: the
 *            cell keeps its value.  *n_written = the cells written.
 *   verify   the exact stage of mh_check_balance over the filled traces; entries / pushes / totals / caps / ordering are that call's.
 * MH_OK: every bus balances.  MH_ERR_UNSATISFIED: not (a looked-up value no provider row carries; a cell shared by fractions that
 * disagree, such as a multiplicity constant over a cycle of rows; a gated provider nobody covers): the report says where, and the
 * traces stay filled as far as they could be.  n_slots == 0 is mh_check_balance with MH_CHECK_EXACT.  Two calls on the same inputs
 * leave the same bytes in the traces and return the same report.
 * The traces are filled IN PLACE in their device storage: fill before the trace is committed or proved (a tree committed earlier
 * does not follow).  The call orders itself after a pending mh_trace_upload_async and runs on the context's stream.
 * Not in scope: multiplicities coupled across rows, sharded contexts, host matrices (upload, fill, mh_trace_download). */
typedef struct mh_mult_slot {   /* fraction `fraction` of LogUp column `lookup_column` of instance `instance` has a multiplicity that
                                   is affine in main-trace column `main_column` */
  int32_t instance;
  uint32_t lookup_column, fraction;   /* as in mh_balance_push */
  uint32_t main_column;
} mh_mult_slot;
int mh_fill_multiplicities(mh_ctx* ctx, int n, const mh_lookup* const* lookups, mh_trace* const* traces,
                           const mh_trace* const* preprocessed /* or NULL */, const uint64_t* randomness /* EF pairs */, size_t n_randomness,
                           const uint64_t* boundary_denoms /* EF pairs */, const int32_t* boundary_signs, size_t n_boundary,
                           const mh_mult_slot* slots, size_t n_slots, uint64_t* n_written, mh_balance_entry* entries, size_t entry_cap,
                           size_t* n_entries, mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);
/* The statements: challenges, boundary pushes and instance numbering of mh_check_balance_*_traces.  No state of mh_miden /
 * mh_precompile is touched. */
int mh_fill_multiplicities_miden_traces(mh_ctx* ctx, const mh_miden* m, mh_trace* const traces[3], const uint64_t* public_values,
                                        const uint64_t* aux_inputs, size_t n_aux_inputs, const mh_mult_slot* slots, size_t n_slots,
                                        uint64_t* n_written, mh_balance_entry* entries, size_t entry_cap, size_t* n_entries,
                                        mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);
int mh_fill_multiplicities_precompile_traces(mh_ctx* ctx, mh_precompile* s, mh_trace* const traces[MH_PRECOMPILE_NUM_AIRS],
                                             const uint64_t public_root[4], const mh_mult_slot* slots, size_t n_slots, uint64_t* n_written,
                                             mh_balance_entry* entries, size_t entry_cap, size_t* n_entries, mh_balance_push* pushes,
                                             size_t push_cap, size_t* n_pushes);

/* ---- the Poseidon2 permutation trace of the Miden statement, built on the device -------------------------------------------------------
 * The third main trace of the statement (16 columns: witnesses[3] | state[12] | perm_id) holds no information of its own:
 * fill_poseidon2_permutation_trace (processor/src/trace/chiplets/hasher/trace.rs:361-408) derives it from a list of (input state,
 * multiplicity) requests, one 16-row cycle each, then zero-state zero-multiplicity padding cycles with consecutive ids; and the list is
 * what record_perm_request (hasher/mod.rs:469-480) collects from the hasher controller's input rows of the chiplets trace.  Device
 * stage: csrc/p2_trace.hip.  Every cell written is canonical.  The result is an ordinary mh_trace of this context: traces[2] of
 * mh_prove_miden_traces, mh_check_miden_traces, mh_check_balance_miden_traces and mh_fill_multiplicities_miden_traces.
 *   from a list      cycle c < k: states[c], multiplicities[c], both reduced mod p.
 *   from chiplets    a controller input row has column 0 = 0 (the hasher's chiplet selector) and column 1 = 1 (controller s0); memory
 *                    rows (1, 1, ..) and controller padding rows (0, 0, 1, 0) are not.  Its request id is column 20 (perm_id), its state
 *                    columns 4..15.  k = the largest id + 1; cycle c's state is that of the LOWEST input row with id c, its multiplicity
 *                    the number of input rows with id c.
 * (k + 1) * 16 <= 2^log_n is required (one padding cycle at least, as in the reference); log_n lies in 6..32, or is -1:
 * max(6, ceil log2((k + 1) * 16)).  k == 0 gives all padding.
 * A null pointer, a chiplets trace that is not 22 wide or belongs to another context and a log_n out of range are refused before any
 * launch.  A DEFECT of the input is found on the device: *out = NULL, MH_ERR_INVALID, `info` filled, mh_last_error names kind and row.
 * Kinds, reported in this order, always the lowest row / id of the kind:
 *   1  the perm_id of an input row lies beyond the id table (N/2 + 1 entries for N chiplets rows); defect_row = the row.  n_requests
 *      is then a partial value: the largest id + 1 over the input rows whose id lies inside the table
 *   3  an input row carries another state than the lowest input row of its id; defect_row = the row
 *   2  an id below k that no input row requests; defect_row = the id
 *   4  (k + 1) * 16 > 2^log_n; defect_row = the lowest id without a cycle of its own, 2^log_n / 16 - 1
 * The context stays usable.  The call orders itself after a pending mh_trace_upload_async / _cols_async of the chiplets trace, waits
 * once for five words of the scan and returns with the trace's kernel enqueued: any later call on the context may use *out at once.
 * Two calls on the same input leave the same bytes.
 * Not in scope: the precompile prover's Poseidon2Air (another AIR, with cube registers), sharded contexts, and deriving the chiplets
 * trace itself. */
typedef struct mh_p2_trace_info {
  uint64_t n_requests;     /* k: distinct permutation requests = cycles that carry one */
  uint64_t n_input_rows;   /* controller input rows read (0 for the host-list entry) */
  int32_t  log_n;          /* height of the trace built */
  int32_t  defect;         /* 0 none, 1 id out of range, 2 id gap, 3 conflicting states for one id, 4 too many requests for log_n */
  uint64_t defect_row;     /* lowest chiplets row (kinds 1, 3) or lowest id (kinds 2, 4) */
} mh_p2_trace_info;
/* fill_poseidon2_permutation_trace from a host request list: states [k][12], multiplicities [k] (any uint64_t, reduced mod p) */
int mh_poseidon2_trace_build(mh_ctx* ctx, const uint64_t* states, const uint64_t* multiplicities, size_t k,
                             int log_n /* -1: max(6, ceil log2((k + 1) * 16)) */, mh_trace** out, mh_p2_trace_info* info /* may be NULL */);
/* the same, the requests read from a device-resident chiplets trace (width 22) */
int mh_miden_poseidon2_trace(mh_ctx* ctx, const mh_trace* chiplets, int log_n /* -1 as above */, mh_trace** out,
                             mh_p2_trace_info* info /* may be NULL */);

/* ---- the range-check table, laid on the device from the statement's lookups ------------------------------------------------------------
 * mh_fill_multiplicities counts how often each table row is looked up; this call also lays the table.  From traces whose value column
 * and multiplicity column hold anything at all it writes both, as RangeChecker::write_range_into_core does (processor/src/trace/range/
 * mod.rs:82-204): the 16-bit values any push of the statement looks up, 0 and 65535 always, ascending, gaps bridged by rows 3^k apart
 * (k <= 7, get_num_bridge_rows / write_rows), a trailing (0, 65535) row, the table in the LAST rows_needed rows and zeros above it.
 * The rule is the reference's and is fixed.  Device stage: csrc/range_table.hip.
 *   probe    the declaring instance's program on a scratch copy of its trace with the value column 0, then 1.  The slot's denominator
 *            must be d0 + g * cell with d0, g the same on every row and g != 0, its multiplicity the same in both, and no other
 *            fraction may differ between the two: otherwise MH_ERR_INVALID, mh_last_error names the first offending fraction.
 *   mark     every push of the statement with a non-zero multiplicity (boundary pushes included, the slot's own left out) whose
 *            (d - d0) / g is a base-field value below 2^16 is a lookup of that value.  Pushes of other buses fail this decode because
 *            the challenges are extension-field values; the verify stage reports whatever would slip through.
 *   rows     rows_needed = sum over the present values of 1 + get_num_bridge_rows(gap) + 1.  rows_needed > 2^log_n of the declaring
 *            trace: MH_ERR_INVALID with `info` filled, so the caller can size the trace and call again.
 *   emit     both columns: zeros in rows [0, n - rows_needed), the table below; multiplicity cells 0.
 *   fill     mh_fill_multiplicities with the one slot (instance, lookup_column, fraction, mult_column): *n_written, the report, MH_OK /
 *            MH_ERR_UNSATISFIED are that call's.  The count of value 0 is kept on the table's first row, as the reference does.
 * A refused call (MH_ERR_INVALID) has written nothing.  A looked-up value of 2^16 or more, or one outside the base field, cannot be
 * decoded: it gets no row and comes back as an unmatched push in the report (MH_ERR_UNSATISFIED).  Two calls on the same inputs leave
 * the same bytes.  Lifetime and ordering are those of mh_fill_multiplicities: in place, after a pending mh_trace_upload_async, on the
 * context's stream, before the trace is committed or proved.
 * Not in scope: sharded contexts, host matrices, rules other than the 16-bit / 3^k table, deriving the memory rows' own range limbs
 * (the chiplets trace has to carry them: they are what the memory rows push). */
typedef struct mh_range_slot {   /* fraction `fraction` of LogUp column `lookup_column` of instance `instance` is the table's provider:
                                    its denominator encodes main-trace column `value_column`, its multiplicity is affine in `mult_column` */
  int32_t instance;
  uint32_t lookup_column, fraction;   /* as in mh_balance_push */
  uint32_t value_column, mult_column;
} mh_range_slot;
typedef struct mh_range_table_info {
  uint64_t n_values;         /* distinct values in the table (0 and 65535 included) */
  uint64_t rows_needed;      /* value rows + bridge rows + the trailing row */
  uint64_t rows_available;   /* height of the declaring instance's trace */
} mh_range_table_info;
int mh_fill_range_table(mh_ctx* ctx, int n, const mh_lookup* const* lookups, mh_trace* const* traces,
                        const mh_trace* const* preprocessed /* or NULL */, const uint64_t* randomness /* EF pairs */, size_t n_randomness,
                        const uint64_t* boundary_denoms /* EF pairs */, const int32_t* boundary_signs, size_t n_boundary,
                        const mh_range_slot* slot, mh_range_table_info* info /* may be NULL */, uint64_t* n_written,
                        mh_balance_entry* entries, size_t entry_cap, size_t* n_entries, mh_balance_push* pushes, size_t push_cap,
                        size_t* n_pushes);
/* The Miden statement: the slot is the core trace's range table (instance 0, LogUp column 0 fraction 14, value column 50,
 * multiplicity column 49); challenges and boundary pushes of mh_check_balance_miden_traces. */
int mh_fill_range_table_miden_traces(mh_ctx* ctx, const mh_miden* m, mh_trace* const traces[3], const uint64_t* public_values,
                                     const uint64_t* aux_inputs, size_t n_aux_inputs, mh_range_table_info* info /* may be NULL */,
                                     uint64_t* n_written, mh_balance_entry* entries, size_t entry_cap, size_t* n_entries,
                                     mh_balance_push* pushes, size_t push_cap, size_t* n_pushes);

/* ---- the memory chiplet's trace section, built on the device from an access list -------------------------------------------------------
 * The memory section of the chiplets trace is the one chiplet section that is not row-local: Memory::fill_trace (processor/src/trace/
 * chiplets/memory/mod.rs:308-406, segment.rs) walks the accesses sorted by (context, word, clock), carries every word through its
 * accesses, takes a delta against the previous row and inverts it.  Here the caller hands over the accesses in program order, 48 bytes
 * each, and the device writes the 17 cells per access.  Device stage: csrc/memory_section.hip.  Every cell written is canonical.
 *   row order   by (ctx, addr >> 2, clk); ties keep arrival order (a stable sort).
 *   columns     rw (1 = read), ew (1 = word access), ctx, word_addr (addr & ~3), idx0, idx1 (the bits of addr & 3; 0 for a word
 *               access), clk, v0..v3 (the word AFTER the access; a word nobody wrote is four zeros), d0, d1 (16-bit halves of the
 *               delta), d_inv (its field inverse, 0 for delta 0), f_scw (1 when ctx and word equal the previous row's), w0, w1 (halves
 *               of word_addr / 4).
 *   delta       ctx difference when the context changed, else word_addr difference when the word changed, else clk difference.  Row 0
 *               has delta 1 and f_scw 1: the reference starts from (ctx, word, clk - 1), for clk = 0 too.
 * PRECONDITION: within one (ctx, word) the clocks do not decrease in arrival order (a processor emits accesses in clock order).  Then
 * this is Memory::fill_trace cell for cell.  A list that breaks it is sorted by the rule above all the same.
 * A DEFECT of the list: MH_ERR_INVALID, `info` filled, nothing written (*out = NULL), mh_last_error names kind and access; the context
 * stays usable.  Kind 4 is decided on the host before anything else, kinds 1 and 2 in the first kernel (the lowest arrival index of
 * either), kind 3 after the sort (the lowest arrival index):
 *   1  kind > 3
 *   2  a word access whose addr is not a multiple of 4 (UnalignedWordAccess)
 *   3  two accesses of one (ctx, word) in one cycle of which the later is a write, or the earlier is a write (IllegalMemoryAccess);
 *      defect_index = the later access
 *   4  the section does not fit: n > 2^log_n, or start_row + n > the chiplets trace's height; defect_index = the first access
 *      without a row
 * n == 0 is MH_OK and writes no row.  n > 2^24, a null pointer, a chiplets trace that is not 22 wide or belongs to another context are
 * refused before any launch.  `accesses` is a host pointer and may be reused when the call returns.  The call orders itself after a
 * pending mh_trace_upload_async of the chiplets trace, waits twice (five words that fix the sort's digit plan and carry kinds 1 and 2;
 * three words with kind 3 and the counts) and returns with the rows kernel enqueued on the context's stream; `row_of`, when asked for,
 * costs a third wait.  Two calls on one input leave the same bytes and name the same defect.
 * Not in scope: sharded contexts, device-resident access lists, the other four chiplet sections (of them bitwise, ACE and kernel ROM
 * have no device builder; the hasher controller's is mh_hasher_section_build below), lists whose clocks run against arrival order
 * beyond the order rule stated above, and n > 2^24. */
typedef struct mh_mem_access {      /* 48 bytes */
  uint32_t ctx, addr, clk, kind;    /* kind: bit 0 = read, bit 1 = word access; addr is the ELEMENT address */
  uint64_t value[4];                /* element write: value[0]; word write: value[0..3]; reads ignore it.  Any uint64_t, reduced mod p */
} mh_mem_access;
typedef struct mh_mem_section_info {
  uint64_t n_rows;        /* rows written = n (0 when the call was refused) */
  uint64_t n_words;       /* distinct (ctx, word) pairs */
  uint64_t n_contexts;    /* distinct contexts */
  int32_t  log_n;         /* height of the trace written to */
  int32_t  defect;        /* 0, or the kind above */
  uint64_t defect_index;  /* arrival index of the lowest offending access */
} mh_mem_section_info;
/* a trace of width 17 (MemoryCols + w0, w1), the section in rows [0, n), zeros below; log_n = -1: max(6, ceil log2 n) */
int mh_memory_section_build(mh_ctx* ctx, const mh_mem_access* accesses, size_t n, int log_n, mh_trace** out,
                            uint32_t* row_of /* [n] or NULL: the section row access i landed on */, mh_mem_section_info* info /* may be NULL */);
/* the same rows written in place into a device-resident chiplets trace (width 22) at rows [start_row, start_row + n):
 * columns 0..2 = 1, 1, 0 (the memory chiplet's selectors), columns 3..19 = the 17 cells; columns 20 and 21 are not touched */
int mh_miden_memory_section(mh_ctx* ctx, mh_trace* chiplets, uint64_t start_row, const mh_mem_access* accesses, size_t n,
                            uint32_t* row_of, mh_mem_section_info* info);
/* rows of one tile of the word-carry scan (a property of the build; tests place their sizes around it) */
uint32_t mh_memory_section_tile(void);

/* ---- the hasher controller's trace section, built on the device from an op list --------------------------------------------------------
 * The hasher controller is the first and largest chiplet section, and the one whose content is computed: every second row is a
 * Poseidon2 output.  Hasher (processor/src/trace/chiplets/hasher/mod.rs:131-480, trace.rs:91-139) appends two rows per permutation
 * and numbers the distinct pre-states in order of first appearance (record_perm_request).  Here the caller hands over the hash
 * operations in program order, 24 bytes each plus their operands, and the device computes the permutations and writes the 20 cells per
 * row.  Device stage: csrc/hasher_section.hip.  Every cell written is canonical.  With mh_miden_poseidon2_trace the third main trace
 * follows from the same rows, so no permutation is computed on the host.
 *   columns     sel[3] | state[12] | node_index | mrupdate_id | is_boundary | direction_bit | perm_id
 *   rows        per permutation an input row (the op's selectors, the pre-state) and an output row (RETURN_HASH (0,0,0) or RETURN_STATE
 *               (0,0,1), the post-state); both carry the permutation's perm_id and the mrupdate_id in effect.
 *   permute           1 permutation, LINEAR_HASH (1,0,0) / RETURN_STATE, boundary 1 / 1
 *   control block     state h1 | h2 | 0, domain, 0, 0; RETURN_HASH; boundary 1 / 1
 *   basic block       a permutation per 8-felt batch: the rate is overwritten, the capacity kept (zero before the first); RETURN_STATE
 *                     on all outputs but the last; boundary on the first input row and the last output row only
 *   merkle verify     per level the state root | sibling, or sibling | root when the index's bit is 1, capacity zero; selectors MP_VERIFY
 *                     (1,0,1); input row: the index and its lowest bit; output row: index >> 1 and the next level's bit (0 on the last
 *                     level); boundary on level 0's input row and the last level's output row; RETURN_HASH on the last level only
 *   merkle update     mrupdate_id += 1 first, then the old value's leg (MR_UPDATE_OLD (1,1,0)) and the new value's (MR_UPDATE_NEW (1,1,1))
 *   perm_id     k for the k-th distinct pre-state in order of first appearance; distinct as canonical field elements (x and x + p are
 *               one state); a repeat gets the first one's id.  n_requests is their number.
 *   padding     to a multiple of 8 rows with selectors (0,1,0), all other cells 0 and mrupdate_id = the final counter
 *   addr        of an op = the 1-based row of its first row
 * A memoised replay of a block hash (replay_memoized_trace, mod.rs:404-431) appends the same rows under the current mrupdate_id and
 * registers the same requests: for this interface it is simply the operation listed again.
 * A DEFECT of the list: MH_ERR_INVALID, `info` filled, nothing written (*out = NULL), mh_last_error names kind and op; the context stays
 * usable.  Every op is tested for kinds 1, 2, 3, 4 in this order and carries the first it has; the call reports the LOWEST op index that
 * carries any of them -- the op at which the reference would stop -- so for each kind the lowest index with it when no earlier op is
 * defective.  Kind 5 is reported only for a list without the others; it is known after the row-offset scan, before any row is written:
 *   1  kind > 4
 *   2  count out of range: a basic block with 0 batches, a Merkle depth of 0 or above 64 ("path is empty")
 *   3  a Merkle index that is not below p, or with index >> depth != 0 for depth < 64 ("invalid index for the path")
 *   4  operands that do not lie inside felts[0, n_felts)
 *   5  the section does not fit: n_rows > 2^log_n, or n_rows above the chiplets trace's height; defect_index = the first op without its
 *      rows (n_ops when only the padding lacks room)
 * n_ops == 0 is MH_OK with zero rows.  A null pointer, a trace of the wrong width or of another context, log_n out of range and more than
 * 2^24 permutations are refused without a defect number and before anything is written.  The permutation count of a list with n_ops <=
 * 2^24 is known from the first kernels' read-back; it is tested before the defects and before any further launch, and every op counts
 * with what its kind and count say (0 for defects 1 and 2).
 * `ops`, `felts` and `results` are host pointers and may be reused when the call returns.  The call orders itself after a pending
 * mh_trace_upload_async of the chiplets trace, runs on the context's stream and waits twice: for six words with the defects and the
 * sizes, and for n_requests, which is part of `info` and known only when the chains have been walked.  It returns with the rows kernel
 * enqueued; `results`, when asked for, costs a third wait.  Two calls on one input leave the same bytes and name the same defect.
 * Not in scope: sharded contexts, device-resident op lists, the bitwise, ACE and kernel-ROM sections, deriving the op list from a program
 * (the decoder's job), and the precompile prover's Poseidon2Air. */
typedef struct mh_hash_op {     /* 24 bytes */
  uint32_t kind;    /* 0 permute, 1 control block, 2 basic block, 3 merkle verify, 4 merkle update */
  uint32_t count;   /* basic block: batches (>= 1); merkle: depth 1..64; otherwise ignored */
  uint64_t index;   /* merkle: node index; control block: the domain felt; otherwise ignored */
  uint64_t payload; /* offset, in felts, of this op's operands in `felts` */
} mh_hash_op;
/* operands: permute 12 (the state) | control block 8 (h1, h2) | basic block 8*count | merkle verify 4 + 4*depth (value, siblings from the
   leaf up) | merkle update 8 + 4*depth (old value, new value, siblings).  Any uint64_t, reduced mod p. */
typedef struct mh_hash_result { uint64_t addr; uint64_t state[12]; uint64_t old_root[4]; } mh_hash_result;
/* addr = 1-based row of the op's first row; state = the op's last post-state (digest = state[0..3]; merkle update: of the NEW leg);
   old_root = the old leg's root for a merkle update, zeros otherwise */
typedef struct mh_hasher_section_info {
  uint64_t n_rows;          /* controller rows incl. padding to a multiple of 8 (0 when refused) */
  uint64_t n_permutations;  /* input rows */
  uint64_t n_requests;      /* distinct pre-states = the k of mh_p2_trace_info */
  uint64_t mrupdate_id;     /* final counter */
  int32_t log_n, defect; uint64_t defect_index;
} mh_hasher_section_info;
/* a trace of width 20, the section in rows [0, n_rows), zeros below; log_n = -1: max(6, ceil log2 n_rows) */
int mh_hasher_section_build(mh_ctx* ctx, const mh_hash_op* ops, size_t n_ops, const uint64_t* felts, size_t n_felts, int log_n,
                            mh_trace** out /* width 20 */, mh_hash_result* results /* [n_ops] or NULL */, mh_hasher_section_info* info /* may be NULL */);
/* the same rows written in place into rows [0, n_rows) of a device-resident chiplets trace (width 22; the hasher is always the first
 * section): column 0 = 0, columns 1..20 = the 20 cells; column 21 (chip_clk) and every row from n_rows on are not touched */
int mh_miden_hasher_section(mh_ctx* ctx, mh_trace* chiplets /* width 22 */, const mh_hash_op* ops, size_t n_ops, const uint64_t* felts,
                            size_t n_felts, mh_hash_result* results, mh_hasher_section_info* info);
/* ops (plan) and permutations (perm_id ranks) of one scan tile (a property of the build; tests place their sizes around it) */
uint32_t mh_hasher_section_tile(void);

/* ---- the bitwise, ACE and kernel-ROM sections, and the whole chiplets trace, built on the device --------------------------------------
 * The three chiplet sections the two builders above leave out, and one entry that takes the five lists of an executed program and
 * returns the finished device-resident chiplets trace: no chiplets cell is uploaded.  Device stages: csrc/bitwise_section.hip,
 * csrc/ace_section.hip, csrc/kernel_rom_section.hip, csrc/chiplets_build.hip.  Every cell written is canonical, every cell has one
 * writer, and two calls on one input leave the same bytes and name the same defect.  All list pointers are host pointers and may be
 * reused when a call returns.  A DEFECT of a list: MH_ERR_INVALID, `info` filled, nothing written (*out = NULL), mh_last_error names
 * kind and index; the context stays usable.  A null pointer, a chiplets trace that is not 22 wide or belongs to another context and a
 * log_n outside 6..32 (other than -1) are refused without a defect number.  Each builder has a standalone form (a trace of the section's
 * own width, the section in rows [0, n_rows), zeros below; log_n = -1: max(6, ceil log2 n_rows)) and an in-place form that writes rows
 * [start_row, start_row + n_rows) of a width-22 chiplets trace: the section's selector prefix and its payload columns, nothing else.
 *
 * BITWISE (processor/src/trace/chiplets/bitwise/mod.rs): 13 columns, 8 rows per operation.  Row i = 0..7 with off = 28 - 4i holds
 *   op | a >> off | b >> off | the four low bits of a >> off, LSB first | those of b >> off | prev | result
 * where result = prev << 4 | the row's result nibble and prev is the result of the row before (0 on row 0).  In place: columns 0, 1 =
 * 1, 0 and columns 2..14.  Defects, in this order:
 *   1  op > 1; defect_index = the lowest such op.  Decided by one pass over the list on the host before any launch.
 *   2  the section does not fit: 8 n_ops > 2^log_n or beyond the chiplets trace's height; defect_index = the first op without its rows.
 * More than 2^24 rows are refused before any launch.  One kernel, no wait; `results` (a AND b / a XOR b per op), when asked for, is
 * written by the same kernel and costs one wait.
 *
 * ACE (ace/{mod,trace,instruction}.rs, execution/operations/eval_circuit.rs:54-118): 16 columns.  One evaluation has n_read =
 * num_vars / 2 READ rows and num_eval EVAL rows and nw = 2 n_read + num_eval wires whose ids descend from nw - 1 in insertion order.
 *   READ row i   s_start = (i == 0) | 0 | ctx | ptr + 4i | clk | 0 | id0 = nw-1-2i | v0 (word[0], word[1]) | id1 = id0 - 1 | v1 (word[2],
 *                word[3]) | num_eval - 1 | 0 | m1 | m0
 *   EVAL row k   0 | 1 | ctx | ptr + 4 n_read + k | clk | eval_op (p-1 sub, 0 mul, 1 add) | id0 = num_eval-1-k | v0 | id_l | v_l | id_r |
 *                v_r | m0
 * An instruction is id_l | id_r << 30 | op << 60 of the canonical felt (op 0 sub, 1 mul, 2 add); m of a wire is the number of times any
 * gate of the evaluation names it (id_l == id_r counts twice); products are in F_p[x]/(x^2 - 7); the last wire must be zero.  The
 * operands of evaluation e lie at felts[payload ..]: 2 num_vars felts (the n_read words as read from memory), then num_eval instruction
 * felts.  Evaluations are listed in clock order, which is the reference's row order.  In place: columns 0..3 = 1, 1, 1, 0 and columns
 * 4..19.  Every evaluation is tested for kinds 1, 2, 3, 4 in this order and carries the first it has; the call reports the LOWEST
 * evaluation that carries any of them, then kind 5, then kind 6 for the lowest evaluation with it:
 *   1  num_vars zero or odd, num_eval zero or not a multiple of 4, or more than 2^30 - 1 wires
 *   2  clk not above the previous evaluation's
 *   3  operands that do not lie inside felts[0, n_felts), or ptr + 2 num_vars + num_eval beyond the 32-bit address space
 *   4  a gate whose opcode is above 2 or that names a wire not yet inserted (the gate itself included); defect_gate = the lowest such
 *      gate of that evaluation
 *   5  the section does not fit; defect_index = the first evaluation without its rows
 *   6  the circuit does not evaluate to zero.  Known only after evaluation: the rows kernel is enqueued after that read-back.
 * More than 2^24 rows (by the headers as they stand) are refused before any launch.  The call waits twice: for the words with kinds
 * 1..5 and the sizes, and for kind 6 and n_rounds; it returns with the rows kernel enqueued.
 * Evaluation: a wave takes one evaluation and walks its gates 64 at a time, a lane a gate.  In a round every gate whose operands lie
 * before the window or belong to a finished lane of the window computes; finished values pass between lanes inside the wave.  n_rounds
 * is the total of rounds over all windows of all evaluations, a function of the circuits alone: a chain of N gates of which each
 * reads the one before costs N, N gates that read only READ wires cost ceil(N / 64).
 *
 * KERNEL ROM (kernel_rom/mod.rs): 5 columns m | h0..h3, one row per DISTINCT declared procedure digest (declared duplicates collapse,
 * as the reference's map does), sorted by the 32 canonical little-endian bytes of the four felts compared lexicographically -- not
 * numeric order: 0x0100 sorts before 0x0001.  m = the number of calls of that digest.  Digests are any uint64_t, reduced mod p.  In
 * place: columns 0..4 = 1, 1, 1, 1, 0 and columns 5..9.  n_procs > 255 is refused without a defect number.  Defects, in this order:
 *   1  a call of an undeclared digest (SyscallTargetNotInKernel); defect_index = the lowest such call
 *   2  the section does not fit; defect_index = the first row without room
 * One wait (the row count and kind 1); `digests` (the rows' digests in trace order: what the caller puts into aux_inputs[8..]), when
 * asked for, costs a second.
 *
 * FRAME and WHOLE TRACE (trace/chiplets/mod.rs:58-73, 134-173, 213-310).  Width 22; trace_len = hasher rows (a multiple of 8) + 8 *
 * bitwise ops + memory accesses + ACE rows + kernel rows + 1: one padding row is mandatory.
 *   section     selector prefix    payload columns
 *   hasher      s0 = 0             1..20
 *   bitwise     (1,0)              2..14
 *   memory      (1,1,0)            3..19
 *   ACE         (1,1,1,0)          4..19
 *   kernel ROM  (1,1,1,1,0)        5..9
 *   padding     (1,1,1,1,1)        zero payload
 * Column 21 is row + 1 on every row; every cell no section owns is 0.  mh_miden_chiplets_frame writes column 21 on all rows and, from
 * padding_start on, ones in columns 0..4 and zeros in columns 5..20; it touches nothing else and does not wait.
 * mh_miden_chiplets_build allocates the trace on the device (log_n = -1: max(6, ceil log2 trace_len)), zero-fills it, runs the five
 * in-place builders in trace order at the starts it computes and writes the frame; no matrix is uploaded.  The sizes are known before
 * the allocation: the hasher's, bitwise, memory and ACE rows from the lists' headers as they stand (a defective op counts with what
 * its kind and count say, 0 for an unknown kind), the kernel rows from a first run of the kernel-ROM sort (one wait, skipped for
 * fewer than two procedures).  trace_len > 2^log_n is a defect of its own (defect_section 5, defect 1, defect_index = trace_len),
 * reported before anything is allocated.  Otherwise a defect in any list frees the trace (*out = NULL) and the report names the first
 * defective section in trace order (defect_section 0 hasher .. 4 kernel ROM; defect and defect_index as that section's builder gives
 * them; the section's own info holds the rest).  An empty list is legal and takes no rows.  Everything is ordered on the context's
 * stream, and the call waits up to 8 times: 1 for the kernel row count, 2 in the hasher builder, 0 in the bitwise builder, 2 in the
 * memory builder, 2 in the ACE builder, 1 in the kernel-ROM builder; it returns with the frame kernel enqueued.
 * Not in scope: sharded contexts, device-resident lists, deriving the lists from a program, emitting the memory accesses an evaluation
 * makes (the caller's memory list already holds them), and the precompile prover's chiplets. */
typedef struct mh_bitwise_op { uint32_t op, a, b; } mh_bitwise_op;   /* 12 bytes; op 0 AND, 1 XOR */
typedef struct mh_bitwise_section_info {
  uint64_t n_rows;        /* 8 n_ops (0 when refused) */
  int32_t log_n, defect; uint64_t defect_index;
} mh_bitwise_section_info;
int mh_bitwise_section_build(mh_ctx* ctx, const mh_bitwise_op* ops, size_t n_ops, int log_n, mh_trace** out /* width 13 */,
                             uint32_t* results /* [n_ops] or NULL */, mh_bitwise_section_info* info /* may be NULL */);
int mh_miden_bitwise_section(mh_ctx* ctx, mh_trace* chiplets /* width 22 */, uint64_t start_row, const mh_bitwise_op* ops, size_t n_ops,
                             uint32_t* results, mh_bitwise_section_info* info);

typedef struct mh_ace_eval {       /* 32 bytes */
  uint32_t ctx, ptr, clk, num_vars, num_eval, reserved;
  uint64_t payload;                /* offset, in felts, of this evaluation's operands in `felts` */
} mh_ace_eval;
typedef struct mh_ace_section_info {
  uint64_t n_rows;        /* READ + EVAL rows (0 when refused) */
  uint64_t n_wires, n_gates;
  uint64_t n_rounds;      /* see "Evaluation" above; 0 until the circuits have been evaluated */
  int32_t log_n, defect;
  uint64_t defect_index;  /* the evaluation */
  uint64_t defect_gate;   /* kind 4: the gate; otherwise 0 */
} mh_ace_section_info;
int mh_ace_section_build(mh_ctx* ctx, const mh_ace_eval* evals, size_t n_evals, const uint64_t* felts, size_t n_felts, int log_n,
                         mh_trace** out /* width 16 */, mh_ace_section_info* info /* may be NULL */);
int mh_miden_ace_section(mh_ctx* ctx, mh_trace* chiplets /* width 22 */, uint64_t start_row, const mh_ace_eval* evals, size_t n_evals,
                         const uint64_t* felts, size_t n_felts, mh_ace_section_info* info);
/* evaluations of one tile of the plan's scan (a property of the build; tests place their sizes around it) */
uint32_t mh_ace_section_tile(void);

typedef struct mh_kernel_rom_section_info {
  uint64_t n_rows;        /* distinct declared digests (0 when refused) */
  uint64_t n_calls;
  int32_t log_n, defect; uint64_t defect_index;
} mh_kernel_rom_section_info;
int mh_kernel_rom_section_build(mh_ctx* ctx, const uint64_t* procs /* [n_procs][4] */, size_t n_procs, const uint64_t* calls /* [n_calls][4] */,
                                size_t n_calls, int log_n, mh_trace** out /* width 5 */, uint64_t* digests /* [n_procs][4] or NULL: the first
                                n_rows entries are written, in trace order */, mh_kernel_rom_section_info* info /* may be NULL */);
int mh_miden_kernel_rom_section(mh_ctx* ctx, mh_trace* chiplets /* width 22 */, uint64_t start_row, const uint64_t* procs, size_t n_procs,
                                const uint64_t* calls, size_t n_calls, uint64_t* digests, mh_kernel_rom_section_info* info);

typedef struct mh_chiplets_lists {
  const mh_hash_op* hash_ops; size_t n_hash_ops; const uint64_t* hash_felts; size_t n_hash_felts;
  const mh_bitwise_op* bitwise_ops; size_t n_bitwise_ops;
  const mh_mem_access* mem_accesses; size_t n_mem_accesses;
  const mh_ace_eval* ace_evals; size_t n_ace_evals; const uint64_t* ace_felts; size_t n_ace_felts;
  const uint64_t* kernel_procs; size_t n_kernel_procs; const uint64_t* kernel_calls; size_t n_kernel_calls;
} mh_chiplets_lists;
typedef struct mh_chiplets_info {
  uint64_t start[5];        /* first row of the hasher, bitwise, memory, ACE and kernel-ROM sections */
  uint64_t padding_start, trace_len;   /* trace_len = padding_start + 1 */
  int32_t log_n;
  int32_t defect_section;   /* -1, or 0 hasher .. 4 kernel ROM, 5 the frame (trace_len > 2^log_n) */
  int32_t defect, reserved;
  uint64_t defect_index;
  mh_hasher_section_info hasher;
  mh_bitwise_section_info bitwise;
  mh_mem_section_info memory;
  mh_ace_section_info ace;
  mh_kernel_rom_section_info kernel_rom;
} mh_chiplets_info;
int mh_miden_chiplets_build(mh_ctx* ctx, const mh_chiplets_lists* lists, int log_n, mh_trace** out /* width 22 */,
                            mh_chiplets_info* info /* may be NULL */);
int mh_miden_chiplets_frame(mh_ctx* ctx, mh_trace* chiplets /* width 22 */, uint64_t padding_start);

/* ---- the precompile prover's Keccak round and sponge traces, built on the device from messages ----
 * mh_keccak_traces_build takes the bytes a session hashes and returns the main traces of KeccakRoundAir (68 columns, index 2 of
 * mh_prove_precompile_traces) and KeccakSpongeAir (67 columns, index 4), device-resident: neither crosses PCIe.
 * mh_keccak_round_trace_build is the stand-alone form for callers that hold the permutation inputs.  Device stage:
 * csrc/keccak_traces.hip.  The rule is the reference's (hash/keccak/round/mod.rs:725-806 generate_trace_from_states_inner,
 * hash/keccak/sponge/trace.rs:176-262 SpongeRequires, :388-585 generate_trace) and is fixed; the 128-slot round programme
 * (round/program.rs slots()) and the 24 round constants live in the library.
 *   messages  message i is bytes[offset .. offset + len); chunk_head = the base of its chunk-tape segment, in chunks of four lanes
 *             (ChunkRequires::require gives it).  Keccak-256: rate 136, pad10*1 with 0x01 / 0x80; len / 136 + 1 blocks, one
 *             permutation and 32 sponge rows a block, in message order.
 *   heights   round: max(2, next_pow2(ceil(max(n_perms, 1) / 2) * 3200)) -- no permutation lays one inactive cycle; sponge:
 *             max(32, next_pow2(32 n_perms)).  log_* = -1 takes these; a larger one pads by the generators' rule (round: zero rows, ip
 *             running on in both lanes; sponge: seq_id running on, bytes_left falling by 8 per rate slot modulo p, chunk_ptr held); a
 *             smaller one is refused with the heights needed in `info`.
 *   refusals  before any trace is allocated or written, MH_ERR_INVALID, *round_out / *sponge_out untouched, `info` filled:
 *             defect_kind 1 offset + len past n_bytes; 2 4 chunk_head + the message's lanes (4 max(1, ceil(len / 32))) not below
 *             2^32; 3 more than 2^24 rows in either trace; 4 a NULL pointer where one is required (defect_index 0); 5 / 6 log_round /
 *             log_sponge below the height needed (defect_index = the rows needed).  defect_index = the message, for kinds 1..3 the lowest.
 *   results   digests[i] = the 32-byte Keccak-256 digest of message i; outputs[n] = Keccak-f[1600] of states[n].  Asking for either
 *             makes the call wait for the stream; without them the call returns with the kernels enqueued on the context's stream.
 * The byte-pair table's three multiplicity columns are not counted here: mh_fill_multiplicities_precompile_traces does that.
 * Every cell is written by one lane; a second call leaves the same bytes.
 * Not in scope: the chunk / node, Poseidon2, transcript, uint and EC chiplets' traces; device-resident message bytes; sharded runs. */
typedef struct mh_keccak_msg { uint64_t offset, len, chunk_head; } mh_keccak_msg;
typedef struct mh_keccak_traces_info {
  uint64_t n_perms;             /* blocks = permutations over all messages */
  uint64_t sponge_rows;         /* 32 n_perms: the sponge's active rows */
  uint64_t round_rows_needed;   /* the least height of the round trace */
  uint64_t sponge_rows_needed;  /* the least height of the sponge trace */
  int32_t defect_kind;          /* 0 none */
  uint64_t defect_index;
} mh_keccak_traces_info;
/* Host only: the round programme, (op, shift, back_a, back_b, dst_mult) per slot; op 0 NOP, 1 XOR, 2 ANDNOT, 3 ROL, 4 XORROL. */
int mh_keccak_round_program(int32_t* out /* [128 * 5] */);
/* Host only: the level of each slot in the device schedule, -1 for a NOP slot.  Level 0 reads only the previous round's outputs, RC
 * or the input; any other slot lies one above the highest same-round slot it reads.  10 levels of 5 5 5 5 5 5 25 25 25 1 slots. */
int mh_keccak_round_levels(int32_t* out /* [128] */);
int mh_keccak_round_trace_build(mh_ctx* ctx, const uint64_t* states /* [n_perms][25] */, size_t n_perms, int log_n /* -1: least */,
                                mh_trace** out /* width 68 */, uint64_t* outputs /* [n_perms][25] or NULL */);
int mh_keccak_traces_build(mh_ctx* ctx, const uint8_t* bytes, size_t n_bytes, const mh_keccak_msg* msgs, size_t n_msgs, int log_round,
                           int log_sponge /* -1: least */, mh_trace** round_out /* width 68 */, mh_trace** sponge_out /* width 67 */,
                           uint8_t* digests /* [n_msgs][32] or NULL */, mh_keccak_traces_info* info /* may be NULL */);

/* ---- the precompile prover's Poseidon2 chiplet trace, built on the device from the absorption ledger ----
 * mh_poseidon2_chiplet_trace_build takes the ledger of Poseidon2Requires -- every absorption's capacity, block count and the two
 * multiplicities, the rate blocks in absorption order -- and returns the main trace of Poseidon2Air (32 columns, index 1 of
 * mh_prove_precompile_traces, mh_check_precompile_traces and mh_fill_multiplicities_precompile_traces), device-resident.  Device
 * stage: csrc/poseidon2_chiplet.hip; the planner (mh_poseidon2_chiplet_plan, host only): csrc/poseidon2_chiplet_plan.cpp.  The rule is
 * the reference's (transcript/poseidon2/trace.rs:217-420 generate_trace / write_cycle) and is fixed.
 *   columns   perm_seq_id 0, in_mult 1, out_mult 2, is_absorb 3, state 4..15, witnesses 16..18, cube registers 19..31.
 *   layout    absorption i lies on cycles start_i .. start_i + n_blocks_i - 1 (16 rows a cycle), start_i = the n_blocks before it.
 *             perm_seq_id = the cycle on its 16 rows, padding included; every other cell of a padding cycle is 0.  in_mult and out_mult
 *             (mod p) stand on all rows of the absorption's cycles, is_absorb = 1 on every cycle but its first.
 *   state     cycle k of an absorption starts from (first half of block k, second half, cap) for k = 0, else the capacity is the previous
 *             cycle's output 8..11.  The digest is the last cycle's output 0..3.  Felts and multiplicities are any uint64_t, reduced mod p.
 *   rows      0: the input, the 12 cubes of M_E state + ARK_EXT_INITIAL[0]; 1..3: before external rounds 1..3 with their cubes; 4..10:
 *             before three internal rounds, the three S-box outputs in the witnesses, the cubes of s0 + ARK_INT in registers 0..2; 11:
 *             before internal round 21, its output in witness 0, the 12 cubes of the first terminal round in registers 0..11, the cube of
 *             the internal S-box input in register 12; 12..14: terminal rounds 1..3; 15: the output, no cube.  All else 0.
 *   refs      refs[c][h] = -1: half h of block c is the literal blocks[c][4 h .. 4 h + 3]; otherwise the index of an EARLIER absorption
 *             whose digest is that half (the literal is not read): the node and transcript absorptions hash digests, and no permutation
 *             runs on the host.  level = 0 without a reference, else one above the highest level referenced; the device runs level
 *             by level.  refs = NULL: all literal.
 *   heights   max(16, next_pow2(16 n_cycles)): no padding cycle is required.  log_n = -1 takes it; a larger one pads; a smaller one
 *             is refused.
 *   refusals  before anything is allocated, MH_ERR_INVALID, *out untouched, `info` filled, mh_last_error names kind and index; the
 *             lowest kind first and within it the lowest index: defect_kind 1 a NULL pointer where one is required (index 0); 2 an
 *             absorption with n_blocks = 0 (index: the absorption); 3 the n_blocks do not add up to n_cycles (index: the first absorption
 *             that runs past it, n_abs when the list ends short); 4 a reference that is neither -1 nor the index of an earlier absorption
 *             (index 2 cycle + half); 5 more than 2^20 cycles (2^24 rows; index: n_cycles); 6 log_n below the height needed (index:
 *             the rows needed; the build entry only).
 *   results   digests[i] = the digest of absorption i, outputs[c] = the permutation output of cycle c.  Asking for either makes the
 *             call wait for the stream; without them it returns with the kernels enqueued on the context's stream.
 * Every cell is written by one lane, no atomics; a second call leaves the same bytes.
 * Not in scope: interning absorptions and counting in_mult / out_mult (the host ledger does both without hashing); the chunk / node,
 * transcript, uint and EC chiplets' traces; device-resident inputs; sharded contexts; more than 2^24 rows. */
typedef struct mh_p2c_absorption { uint64_t cap[4]; uint64_t n_blocks, in_mult, out_mult; } mh_p2c_absorption; /* 56 bytes */
typedef struct mh_p2c_info {
  uint64_t n_absorptions, n_cycles;
  uint64_t n_levels;      /* 0 without an absorption */
  uint64_t rows_needed;   /* the least height */
  int32_t log_n;          /* the height taken (plan: the least) */
  int32_t defect_kind;    /* 0 none */
  uint64_t defect_index;
} mh_p2c_info;
/* Host only: validation, the start cycle and the level of every absorption. */
int mh_poseidon2_chiplet_plan(const mh_p2c_absorption* abs, size_t n_abs, const int64_t* refs /* [n_cycles][2] or NULL */, size_t n_cycles,
                              uint64_t* start /* [n_abs] or NULL */, uint32_t* level /* [n_abs] or NULL */, mh_p2c_info* info);
int mh_poseidon2_chiplet_trace_build(mh_ctx* ctx, const mh_p2c_absorption* abs, size_t n_abs, const uint64_t* blocks /* [n_cycles][8] */,
                                     const int64_t* refs /* [n_cycles][2] or NULL */, size_t n_cycles, int log_n /* -1: least */,
                                     mh_trace** out /* width 32 */, uint64_t* digests /* [n_abs][4] or NULL */,
                                     uint64_t* outputs /* [n_cycles][12] or NULL */, mh_p2c_info* info /* may be NULL */);

/* ---- the precompile prover's UintStoreMul and UintAdd traces, built on the device from the ledgers ----
 * mh_uint_traces_build takes the uint store (values at pointers, each under a bound row), the multiply-accumulate relations
 * kappa_a a b +- kappa_c c = r (mod bound + 1) and the additions a + b = c (mod bound + 1), all over store pointers, and returns the main
 * traces of UintStoreMulAir (44 columns, index 6) and UintAddAir (30 columns, index 7 of mh_prove_precompile_traces,
 * mh_check_precompile_traces and mh_fill_multiplicities_precompile_traces), device-resident.  Device stage: csrc/uint_traces.hip; the
 * planner (mh_uint_traces_plan, host only): csrc/uint_traces_plan.cpp.  The rule is the reference's (uint/trace.rs:273-386,
 * uint/mul/trace.rs:90-180 and 278-384, uint/store_mul/trace.rs:43-72, uint/add/trace.rs:104-215) and is fixed.
 *   rows      mh_uint_row: ptr, bound_ptr, the value in eight 32-bit limbs (least first), and the reads of the row from OUTSIDE these two
 *             chiplets (val_reads over UintVal, limb_reads over UintLimbs: the verifier's boundary reads, the MSM and eval chiplets).
 *             In strictly ascending ptr order -- the order of the trace; a bound row is its own bound_ptr.
 *   store     columns 0..17, four rows per stored value: 0 the low eight 16-bit limbs of the value; 1 the high eight, the UintVal
 *             multiplicity in cell 8 and the UintLimbs multiplicity in cell 9; 2 the sixteen 16-bit limbs of bound - value; 3 the bound's
 *             32-bit limbs 0..3 in cells 0..3 and 4..7 in cells 8..11, the carries of value + (bound - value) out of 32-bit limbs 0..3 in
 *             cells 4..7 and 4..6 in cells 12..14, the gap next_ptr - ptr - 1 in cell 15; ptr 16, bound_ptr 17 on all four.
 *             UintVal multiplicity = val_reads + the c, r of every multiply relation + the a, b, c, bound of every addition + one per
 *             row whose bound_ptr this is (+ 1 on a padding block); UintLimbs = limb_reads + the a, b, bound of every multiply
 *             relation; both mod p.  Padding blocks: ptr = last ptr + 1 + k, its own bound, value 0.
 *   multiply  columns 18..43, eight rows per relation (a, b, bound, quotient, r, carries, carries, c): sixteen 16-bit limbs of a, b and
 *             the bound; the 17 16-bit limbs of q = (kappa_a a b +- kappa_c c) div (bound + 1) (0 on a subtractive underflow, where
 *             `borrow` <= 2 moduli are added back); the 32-bit limbs of r and c; the 31 carries of the synthetic division of the
 *             identity's coefficient polynomial by X - 2^16, each + 2^31 and split in two 16-bit halves over the 62 free cells; on the c
 *             row mult mod p, c_ptr, kappa_c, is_sub, +-kappa_c in cells 8..12; a_ptr, b_ptr, r_ptr, bound_ptr, kappa_a, 1, borrow in
 *             columns 37..43 on all eight.  All-zero blocks after the relations.
 *   adder     two rows per relation: a | b limbs, carries gamma_0..3 (carry of a + b minus carry of c + k (bound + 1), mod p), b
 *             absent, w, w S (nz: w = 1 / S, S the sum of b's limbs), b present; c | bound limbs, gamma_4..6, 0, k, c present, mult mod p,
 *             c absent; a_ptr, b_ptr, c_ptr, bound_ptr, 1, nz in columns 24..29 on both.  Pointer 0 in b or c: absent, value 0.
 *   heights   multiplier half next_pow2(8 max(1, n_mul)); store 4 max(1, next_pow2(n_store), multiplier rows / 4): the 44-column
 *             trace has the store's height.  Adder next_pow2(2 max(1, n_add)).  log_usm / log_add = -1 takes them; a larger one pads
 *             (store: padding blocks; multiplier, adder: zero blocks); a smaller one is refused.
 *   refusals  MH_ERR_INVALID, the out pointers untouched, no trace allocated, `info` filled, mh_last_error names section (0 store, 1
 *             multiply, 2 add), kind, index and operand; the lowest kind first, within it the multiply section before the add section
 *             and the lowest index.  Found by the planner: 1 a NULL pointer where a count is nonzero; 2 more than 2^24 rows in either
 *             trace, or padding pointers reaching 2^32; 3 log_usm / log_add below the height needed (index: the rows needed); 4 a store
 *             ptr that is 0 or not above the one before; 5 a gap to the next ptr >= 2^16 (index: the row before the gap); 6 a bound_ptr
 *             that is not stored; 7 a value above its bound's.  Found by the device's witness pass, through one packed 64-bit minimum
 *             read back once before any trace cell is written: 8 a relation's pointer that is not stored (operand: multiply a 0, b 1,
 *             c 2, r 3, bound 4; add a 0, b 1, c 2, bound 3; 0 is allowed for an addition's b and c only); 9 a kappa >= 2^16 (operand 0
 *             kappa_a, 1 kappa_c); 10 r is not the canonical remainder, or the exact-division self-check of the carry chain failed; for
 *             an addition a + b != c + k (bound + 1) for both k in {0, 1}; 11 a quotient >= 2^272; 12 a subtractive underflow beyond two
 *             moduli; 13 a carry outside the +-2^31 window; 14 nz with b = 0.
 *             Kind 10 for an addition is STRICTER than the reference's generator on purpose: that one asks only (a + b) mod (bound + 1)
 *             = c, accepts 25 + 30 = 0 (mod 11) when the operands live under a foreign, larger bound, and lays a block no k in {0, 1}
 *             satisfies.
 * Every cell of both traces is written by the call; a second call leaves the same bytes.  The byte-pair table's Range16 column is not
 * counted here: mh_fill_multiplicities* does that from the lookup programs.
 * Not in scope: interning and deduplicating values and relations, and computing r (sequential, the host ledger's); sorting the store;
 * the EC point store, group add, MSM and transcript-eval traces; device-resident inputs; sharded contexts; more than 2^24 rows. */
typedef struct mh_uint_row { uint32_t ptr, bound_ptr; uint32_t value[8]; uint32_t val_reads, limb_reads; } mh_uint_row;          /* 48 bytes */
typedef struct mh_uint_mul_op { uint32_t a, b, c, r, bound, kappa_a, kappa_c, is_sub; uint64_t mult; } mh_uint_mul_op;           /* 40 bytes */
typedef struct mh_uint_add_op { uint32_t a, b, c, bound, nz, reserved; uint64_t mult; } mh_uint_add_op;                          /* 32 bytes */
typedef struct mh_uint_traces_info {
  uint64_t n_store, n_mul, n_add;
  uint64_t usm_rows_needed, usm_rows;   /* the least height of the 44-column trace, and the one taken */
  uint64_t add_rows_needed, add_rows;
  int32_t defect_section;               /* 0 store, 1 multiply, 2 add */
  int32_t defect_kind;                  /* 0 none */
  uint64_t defect_index;
  int32_t defect_operand;
  int32_t reserved;
} mh_uint_traces_info;
/* Host only: kinds 1..7, the heights, and for every store row the index of its bound's row. */
int mh_uint_traces_plan(const mh_uint_row* rows, size_t n_store, const mh_uint_mul_op* muls, size_t n_mul, const mh_uint_add_op* adds,
                        size_t n_add, int log_usm, int log_add /* -1: least */, uint32_t* bound_index /* [n_store] or NULL */,
                        mh_uint_traces_info* info);
int mh_uint_traces_build(mh_ctx* ctx, const mh_uint_row* rows, size_t n_store, const mh_uint_mul_op* muls, size_t n_mul,
                         const mh_uint_add_op* adds, size_t n_add, int log_usm, int log_add /* -1: least */,
                         mh_trace** usm_out /* width 44 */, mh_trace** add_out /* width 30 */, mh_uint_traces_info* info /* may be NULL */);

/* ---- the precompile prover's EcGroups, EcPointStore, EcGroupAdd and EcMsm traces, built on the device from the ledgers ----
 * mh_ec_traces_build takes the group table, the point store, the recorded additions and the MSM expressions with their term rows, all
 * as pointer lists (no coordinate limb enters these traces), and returns the main traces of EcGroupsAir (6 columns, index 8),
 * EcPointStoreAir (14, index 9), EcGroupAddAir (21, index 10) and EcMsmAir (38, index 11 of mh_prove_precompile_traces,
 * mh_check_precompile_traces and mh_fill_multiplicities_precompile_traces), device-resident.  Device stage: csrc/ec_traces.hip (row
 * bodies: csrc/ec_traces_rows.cuh); the planner (mh_ec_traces_plan, host only): csrc/ec_traces_plan.cpp.  The rule is the reference's
 * (ec/trace.rs:347-411, ec/add/trace.rs:146-251, ec/msm/trace.rs:390-500) and is fixed.
 *   groups    mh_ec_group, row i is group pointer i + 1: the uint pointers of a, b, the base-field bound and the scalar bound (the bound
 *             itself where the group has no other).  Trace row: ptr, a_ptr, b_ptr, bound_ptr, sbound_ptr, mult.  Pads run the pointer
 *             chain on, the other cells 0.
 *   points    mh_ec_point, row i is point pointer i + 1: group, x_ptr, y_ptr, the membership trio's u_ptr, w_ptr, and kind 0 member,
 *             1 point at infinity (all four pointers 0), 2 closure-certified (u, w 0).  Trace row: ptr, group, the group's a, b, bound,
 *             sbound, x, y, u, w, is_pai, ECPOINT_MULT, 1, is_cert.  Pads all zero.
 *   add       mh_ec_add_op: group, the point pointers p, q, r, kind 0 pai_p, 1 pai_q, 2 pai_both, 3 cancel, 4 double, 5 generic, mints
 *             (r is minted by this addition: double / generic only), t = slope_aux, lambda, t, y3, e, x3 (uint pointers, 0 in the dead
 *             cases) and mult, the relation's multiplicity (the host's: relations are deduplicated there).  Four rows per addition, cells
 *             0..2: t[0..2] | t[3..5] | r, sbound, group | mult mod p, p, q; columns 3..20 on all four: px, py, qx, qy (the operands'
 *             x_ptr, y_ptr; 0 for the point at infinity), the group's a, b, bound, the five case flags, 1, mints, and for mints
 *             r - p - 1 and r - q - 1 in 16-bit halves.  All-zero blocks after the additions.
 *   msm       mh_msm_expr, expression k is pointer k + 1: kind 0 intro, 1 combine, 2 neg; group; val (the value point); a_expr, b_expr
 *             (operands: earlier expressions; 0 where the kind has none); n_rows; neg_minted; ext_mult; claim_mult.  mh_msm_term: the
 *             expressions' (base, scalar) rows, concatenated in expression order, bases strictly ascending within an expression.  One
 *             trace row per term; the other 36 cells are derived: a combine row with base B has i, j = the lower bounds of B in the
 *             operands' term lists, take_a / take_b / take_both by which of them hold B, base_a, s_a, base_b, s_b the operands' terms at
 *             the cursors (0 on a side not taken); a neg row has i = idx and the operand's row; val_a, val_b the operands' val; neg_x,
 *             neg_ya val_a's coordinates and neg_yr val's y on a neg's boundary row; the 16-bit halves of expr - a_expr - 1 and
 *             expr - b_expr - 1 on boundary rows.  Pads: expr_ptr = n_exprs + 1, idx counting from 0.
 *   demand    computed on the device, all mod p.  Group mult = ext_reads + one per point of the group + one per cancel / double / generic
 *             addition + one per combine / neg expression.  ECPOINT_MULT = ext_reads + p and q of every addition + r of every cancel /
 *             double / generic addition + val_a and val of every neg expression.  Expression mult = ext_mult + one per use as a_expr or
 *             b_expr (combine(a, a) uses a twice).  ext_reads / ext_mult are the reads from OUTSIDE these four chiplets (the verifier's
 *             boundary read of the fixed groups, the eval chip's point_on_group / pai_on_group / resolve reads, EcRequire.neg's read of
 *             the point at infinity): any 64-bit word, reduced mod p here.  The intro rows' read of the literal 1 is a val_reads of
 *             mh_uint_row (above); the Range16 reads of the ordering limbs are mh_fill_multiplicities*'s, as in the uint build.
 *   heights   groups, points: max(2, next_pow2(n)); add: next_pow2(4 max(1, n_add)); msm: max(2, next_pow2(n_terms)).  log_* = -1
 *             takes them; a larger one pads; a smaller one is refused.
 *   refusals  MH_ERR_INVALID, the out pointers untouched, no trace allocated, `info` filled, mh_last_error names section (0 groups,
 *             1 points, 2 add, 3 msm), kind, index and operand; the lowest kind first, within it the lowest section, then the lowest
 *             index; a later kind is only looked for once the earlier ones are absent.  Found by the planner: 1 a NULL list where a count
 *             is nonzero (section 3: operand 0 exprs, 1 terms); 2 more than 2^24 rows in a trace (index: the count) or a log_* above 24
 *             (index: the log); 3 a log_* below the height needed (index: the rows needed); 4 a point's group that is 0 or above
 *             n_groups; 5 a point kind outside 0..2 (operand 0), a point at infinity with a nonzero x, y, u or w (operand 1..4), a
 *             certified point with a nonzero u or w (operand 3, 4); 6 an expression kind outside 0..2 (operand 0), n_rows = 0 or an
 *             intro with n_rows != 1 (operand 1), the n_rows not summing to n_terms (index n_exprs, operand 2); 7 an operand that is 0
 *             or not an earlier expression, or nonzero where the kind has none (operand 0 a_expr, 1 b_expr).  Found by the device's
 *             checking pass, through one packed 64-bit minimum read back once before any trace is allocated: 8 an addition's p, q, r or
 *             group (operand 0..3), or an expression's val or group (operand 0, 1), that is 0 or out of range; 9 an addition kind
 *             outside 0..5 (operand 0), mints outside {0, 1} or on a kind other than double / generic (operand 1); 10 p, q or r of an
 *             addition stored under another group than the op's (operand 0..2), or an expression whose group is not its val's (operand
 *             0), its a_expr's (1) or its b_expr's (2); 11 an addition whose kind disagrees with which of p, q are points at infinity;
 *             12 mints with r <= p (operand 0), r <= q (1) or an r that is not a certified row (2); 13 a term row whose base is not above
 *             the one before it in its expression (index: the term row); 14 (index: the term row) a combine row whose base neither
 *             operand holds (operand 0), a merge that skips an operand's term -- this row's cursors advanced by its takes are not the
 *             next row's, the first row's are not 0, 0, or the last row does not end at both lists' lengths (operand 1) --, a neg whose
 *             rows are not its operand's bases one for one (operand 2); 15 an intro whose val is not its base.  Sections 0..2 index
 *             their record, section 3 the expression (kinds 6..8, 10, 15) or the term row (13, 14).
 *             The recorders (EcRequire.add, EcMsmRequires of the reference's ec/require.rs and ec/msm/require.rs) can produce none of
 *             these: every check here is of a pointer, a kind or an order, none of a value -- equal values need not be equal pointers
 *             (pinned uints exist).
 * Every cell of all four traces is written by the call, padding included; the counters and the minimum are scratch the call clears
 * itself; a second call leaves the same bytes.
 * Not in scope: interning, deduplication and the 256-bit arithmetic of the group law (the host recorder's and the uint build's); the
 * TranscriptEval and ChunkNode traces; device-resident inputs; sharded contexts; more than 2^24 rows. */
typedef struct mh_ec_group { uint32_t a_ptr, b_ptr, bound_ptr, sbound_ptr; uint64_t ext_reads; } mh_ec_group;                      /* 24 bytes */
typedef struct mh_ec_point { uint32_t group, x_ptr, y_ptr, u_ptr, w_ptr, kind; uint64_t ext_reads; } mh_ec_point;                  /* 32 bytes */
typedef struct mh_ec_add_op { uint32_t group, p, q, r, kind, mints; uint32_t t[6]; uint64_t mult; } mh_ec_add_op;                  /* 56 bytes */
typedef struct mh_msm_expr { uint32_t kind, group, val, a_expr, b_expr, n_rows, neg_minted, reserved; uint64_t ext_mult, claim_mult; } mh_msm_expr; /* 48 bytes */
typedef struct mh_msm_term { uint32_t base, scalar; } mh_msm_term;                                                                 /* 8 bytes */
typedef struct mh_ec_traces_info {
  uint64_t n_groups, n_points, n_add, n_exprs, n_terms;
  uint64_t groups_rows_needed, groups_rows;   /* the least height, and the one taken */
  uint64_t points_rows_needed, points_rows;
  uint64_t add_rows_needed, add_rows;
  uint64_t msm_rows_needed, msm_rows;
  int32_t defect_section;                     /* 0 groups, 1 points, 2 add, 3 msm */
  int32_t defect_kind;                        /* 0 none */
  uint64_t defect_index;
  int32_t defect_operand;
  int32_t reserved;
} mh_ec_traces_info;                          /* 128 bytes */
/* Host only: kinds 1..7, the heights, and every expression's first term row. */
int mh_ec_traces_plan(const mh_ec_group* groups, size_t n_groups, const mh_ec_point* points, size_t n_points, const mh_ec_add_op* adds,
                      size_t n_add, const mh_msm_expr* exprs, size_t n_exprs, const mh_msm_term* terms, size_t n_terms, int log_groups,
                      int log_points, int log_add, int log_msm /* -1: least */, uint32_t* row_start /* [n_exprs] or NULL */,
                      mh_ec_traces_info* info);
int mh_ec_traces_build(mh_ctx* ctx, const mh_ec_group* groups, size_t n_groups, const mh_ec_point* points, size_t n_points,
                       const mh_ec_add_op* adds, size_t n_add, const mh_msm_expr* exprs, size_t n_exprs, const mh_msm_term* terms,
                       size_t n_terms, int log_groups, int log_points, int log_add, int log_msm /* -1: least */,
                       mh_trace** groups_out /* width 6 */, mh_trace** points_out /* width 14 */, mh_trace** add_out /* width 21 */,
                       mh_trace** msm_out /* width 38 */, mh_ec_traces_info* info /* may be NULL */);

/* ---- the precompile prover's ChunkNode and TranscriptEval traces, built on the device from the ledgers and the Poseidon2 trace ----
 * mh_chunk_node_trace_build returns the main trace of ChunkNodeAir (42 columns, index 0 of mh_prove_precompile_traces,
 * mh_check_precompile_traces and mh_fill_multiplicities_precompile_traces), mh_transcript_eval_trace_build that of TranscriptEvalAir (39
 * columns, index 5), device-resident.  Both read their digests from `p2`, the device-resident Poseidon2 chiplet trace (width 32) that
 * mh_poseidon2_chiplet_trace_build returned on the same context: "the digest on cycle c" is its cells (row 16 c + 15, columns 4..7), read
 * on the context's stream behind the kernels that wrote them.  No permutation runs on the host and no digest is copied there.  Device
 * stage: csrc/transcript_traces.hip (row bodies: csrc/transcript_traces_rows.cuh); the planners (mh_chunk_node_plan,
 * mh_transcript_eval_plan, host only): csrc/transcript_traces_plan.cpp.  The rule is the reference's (hash/chunk/trace.rs:133-175,
 * hash/keccak/node/trace.rs:52-113, hash/chunk_node/trace.rs:24-45, transcript/eval/trace.rs:895-1155) and is fixed.
 *
 * ChunkNode.  One mh_kn_record per distinct hashed input, in ledger order (KeccakNodeRequires.records, 1:1 with ChunkRequires.records):
 * the message is bytes[offset .. offset + len), digests[i] its Keccak-256 digest (as mh_keccak_traces_build returns them), chunk_head
 * the first row of its chunk chain, sponge_head its first sponge row, perm_chunks the first cycle of the chain's absorption,
 * perm_digest_chunks / perm_keccak the one-block absorptions of the digest and of the node, out_mult the node's readers.
 *   chunk     columns 0..11.  n_chunks = max(1, ceil(len / 32)); row chunk_head + c = row, perm_chunks + c, 1, c == 0, and the eight
 *             little-endian u32 felts of message bytes 32 c .. 32 c + 31, zero-padded.  Dead rows: row, next_perm, 0, ..., next_perm
 *             running on from the LAST record's perm_chunks + n_chunks (from 0 without records).
 *   node      columns 12..41.  Row i = 1, sponge_head, len / 136 + 1, chunk_head, n_chunks, perm_chunks, len, perm_digest_chunks,
 *             perm_keccak, the digest as eight little-endian u32 felts, the digests on cycles perm_chunks + n_chunks - 1,
 *             perm_digest_chunks and perm_keccak, out_mult mod p.  Rows below are zero.
 *   height    max(2, next_pow2(n), next_pow2(total chunks)).  log_n = -1 takes it; a larger one pads; a smaller one is refused.
 *   refusals  MH_ERR_INVALID, *out untouched, nothing allocated, `info` filled, mh_last_error names kind, index and operand; the lowest
 *             kind first, within it the lowest index.  The planner's: 1 a NULL pointer where one is required (operand 0 bytes, 1 digests,
 *             2 records, 3 p2 -- or a p2 of another context or width --, 4 out); 2 offset + len past n_bytes (index: the record); 3 a
 *             chunk_head that is not the running sum of n_chunks; 4 a sponge_head that is not a multiple of 32; 5 a cycle at or beyond
 *             the cycles of p2 (operand 0 the chain's last, 1 perm_digest_chunks, 2 perm_keccak); 6 more than 2^24 rows (index: the
 *             rows) or a log_n above 24 (index: the log); 7 log_n below the height needed (index: the rows needed).  The device's, one
 *             packed 64-bit minimum read back once before the trace is allocated: 8 a chain that is not one absorption of p2 --
 *             is_absorb (column 3) is not 0 on cycle perm_chunks (operand 0) or not 1 on one of the n_chunks - 1 cycles behind it
 *             (operand 1); 9 a digest cycle that does not end an absorption -- is_absorb is not 0 on the cycle behind it, where there is
 *             one, or the cycle is padding (all zero) -- (operand 0 the chain's last cycle, 1 perm_digest_chunks, 2 perm_keccak).
 *
 * TranscriptEval.  The transcript DAG as mh_te_node records in recording order (children before parents), the MSM claims' term rows
 * (mh_te_term: the node indices of base and scalar) and a pool of 256-bit literals, limbs[n_lit][8] little-endian u32.
 *   kinds     0 ZERO, 1 AND, 2 UINT_LEAF, 3 UINT_PIN, 4 UINT_OP (op 1 add, 2 sub, 3 mul, 4 is), 5 EC_CREATE, 6 EC_PAI, 7 EC_OP (op 1 add,
 *             2 sub, 3 is), 8 EC_MSM.  Truthy: ZERO, AND, UINT_PIN and the two `is`; uint values: UINT_LEAF and the other UINT_OPs; EC
 *             values: EC_CREATE, EC_PAI, the other EC_OPs, EC_MSM.
 *   fields    lhs, rhs: the operands -- a node index below the record's own, or (AND only) -1 - c: an external True binding, the digest
 *             on cycle c of p2 (a Keccak claim's h_keccak).  A leaf's or pin's lhs indexes the literal pool (lo = limbs 0..3, hi = 4..7);
 *             an MSM's lhs, rhs are term_start, n_terms.  perm: the node's own first cycle (ignored for ZERO).  ptr: the stored uint /
 *             point the node stands for (an op's result, 0 for `is`; an MSM's value point).  bound_ptr: the modulus row of a uint node,
 *             of a created point's coordinates, an MSM's scalar bound.  group: EC_CREATE, EC_PAI, EC_OP (0 for `is`), EC_MSM.  expr: the
 *             MSM chiplet's expression.  Fields a kind does not name are ignored.
 *   derived   h = the digest on cycle perm (MSM row idx: perm + idx; ZERO: zeros).  The lhs / rhs hashes = the operand's h (an MSM
 *             operand's: the digest on its last cycle).  a_ptr, b_ptr (an MSM row's base_ptr, scalar_ptr) = the operands' ptr.  out_mult
 *             of a value node = its readers, counted on the device: uses as an operand of UINT_OP / EC_CREATE / EC_OP and as an MSM
 *             term, a == b counting twice.  out_mult of the root is 0, of every other truthy node 1.  Tag arguments and flags as the
 *             reference lays them.
 *   rows      row 0 the root; then every other non-ZERO node in list order, an MSM on n_terms rows (head / last flags, msm_idx, ptr and
 *             out_mult on the last row only); then ONE merged ZERO row whose out_mult is the number of ZERO nodes other than the root,
 *             if there are any; then zero rows.  height = max(2, next_pow2(active rows)).
 *   refusals  as above.  The planner's: 1 a NULL pointer (operand 0 nodes, 1 terms, 2 limbs, 3 p2, 4 out); 2 an unknown kind (operand
 *             0) or an op outside the kind's range (operand 1); 3 a source that is out of range or not below the own index (operand 0
 *             lhs, 1 rhs; a negative source anywhere but under an AND; a literal index >= n_lit: operand 0; an MSM with term_start +
 *             n_terms past the term rows: operand 0, with n_terms = 0: operand 1), or a term node that is (index: the term row, operand 2
 *             base, 3 scalar); 4 a root index out of range or a root that is not of a truthy kind (index: the root); 5 a cycle at or
 *             beyond the cycles of p2 (operand 0 the node's own, an MSM's last; 1 an external lhs; 2 an external rhs); 6 more than 2^24
 *             rows (or 2^25 nodes) or a log_n above 24; 7 log_n too small (index: the rows needed).  The device's checking pass: 8 an operand of the
 *             wrong class -- a value under an AND, a truthy or EC node under a uint op or a create, a uint node under an EC op (operand 0
 *             lhs, 1 rhs), as an MSM base or an EC node as an MSM scalar (index: the term row, operand 2 base, 3 scalar); 9 operands
 *             under different moduli: an operand's bound_ptr of a UINT_OP / EC_CREATE against the record's (operand 0 lhs, 1 rhs), an
 *             MSM scalar's against the record's (index: the term row, operand 3); 10 an `is` over distinct pointers; 11 a truthy node
 *             that is never read (operand 0: a stray unasserted claim) or read twice (operand 1: Truthy consumed twice), or the root
 *             read at all (operand 2); 12 a value node nobody reads; 13 a perm that is not a one-block absorption of p2 (operand 0 it
 *             continues one, 1 it does not end there); 14 an MSM span that is not one absorption of n_terms blocks (operand 0 its first
 *             cycle continues one; 1 a later cycle does not, index: the term row; 2 it does not end on its last); 15 an external cycle
 *             that does not end an absorption (operand 0 lhs, 1 rhs).
 *   result    root_felts (may be NULL): the four felts of row 0's h, the statement's public input -- the call's one read-back besides
 *             the minimum.
 * No VALUE is checked: that a cycle's capacity and rate are the node's tag and operands is the AIR's bus, which mh_check_balance* finds.
 * Every cell of both traces is written by one lane, padding included; the counters and the minimum are scratch the calls clear
 * themselves; a second call leaves the same bytes.
 * Not in scope: recording the transcript (deduplication, interning: the host's); counting the Poseidon2 in_mult / out_mult; chunk
 * chains laid by anything but a Keccak node; device-resident input lists; sharded contexts; more than 2^24 rows. */
typedef struct mh_kn_record { uint64_t offset, len, chunk_head, sponge_head, perm_chunks, perm_digest_chunks, perm_keccak, out_mult; } mh_kn_record; /* 64 bytes */
typedef struct mh_chunk_node_info {
  uint64_t n_records, n_chunks, p2_cycles;
  uint64_t rows_needed, rows;   /* the least height, and the one taken */
  int32_t defect_kind;          /* 0 none */
  int32_t defect_operand;
  uint64_t defect_index;
} mh_chunk_node_info;           /* 56 bytes */
typedef struct mh_te_node { uint32_t kind, op; int64_t lhs, rhs; uint64_t perm, ptr, bound_ptr, group, expr; } mh_te_node;            /* 64 bytes */
typedef struct mh_te_term { uint32_t base_node, scalar_node; } mh_te_term;                                                          /* 8 bytes */
typedef struct mh_transcript_eval_info {
  uint64_t n_nodes, n_terms, n_lit, p2_cycles;
  uint64_t active_rows, n_zero; /* the rows that are not padding; the ZERO nodes other than the root */
  uint64_t rows_needed, rows;
  int32_t defect_kind;
  int32_t defect_operand;
  uint64_t defect_index;
} mh_transcript_eval_info;      /* 80 bytes */
/* Host only: kinds 1..7 (no pointer but `records` is read through) and the height. */
int mh_chunk_node_plan(const uint8_t* bytes, size_t n_bytes, const uint8_t* digests, const mh_kn_record* records, size_t n,
                       uint64_t p2_cycles, int log_n /* -1: least */, mh_chunk_node_info* info);
int mh_chunk_node_trace_build(mh_ctx* ctx, const mh_trace* p2 /* width 32 */, const uint8_t* bytes, size_t n_bytes,
                              const uint8_t* digests /* [n][32] */, const mh_kn_record* records, size_t n, int log_n /* -1: least */,
                              mh_trace** out /* width 42 */, mh_chunk_node_info* info /* may be NULL */);
/* Host only: kinds 1..7, the height and every node's first row (`limbs` is not read through). */
int mh_transcript_eval_plan(const mh_te_node* nodes, size_t n_nodes, const mh_te_term* terms, size_t n_terms, const uint32_t* limbs,
                            size_t n_lit, uint64_t root, uint64_t p2_cycles, int log_n /* -1: least */,
                            uint32_t* row_start /* [n_nodes] or NULL */, mh_transcript_eval_info* info);
int mh_transcript_eval_trace_build(mh_ctx* ctx, const mh_trace* p2 /* width 32 */, const mh_te_node* nodes, size_t n_nodes,
                                   const mh_te_term* terms, size_t n_terms, const uint32_t* limbs /* [n_lit][8] */, size_t n_lit,
                                   uint64_t root, int log_n /* -1: least */, mh_trace** out /* width 39 */,
                                   uint64_t* root_felts /* [4] or NULL */, mh_transcript_eval_info* info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MIDENHIP_H */
