/*
 * dagpu.h -- C ABI of the MI355X-native celestia-app data-availability hot path.
 *
 * Library: celestia-app_amd/libdagpu.so (hipcc --offload-arch=gfx950).
 * Plain pointers and sizes only; the caller owns every buffer and nothing is
 * retained after a call returns.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repo root).  The Go
 * (cgo) binding a maintainer would add on the reference side is in
 * INTEGRATION.md.
 *
 * Layouts
 *   share      512 bytes (appconsts.ShareSize, pkg/appconsts/global_consts.go:29)
 *   ODS        k*k shares, row-major                     (k*k*512 B)
 *   EDS        (2k)*(2k) shares, row-major, Q0|Q1 / Q2|Q3 ((2k)^2*512 B)
 *   root       90 bytes = minNs(29) | maxNs(29) | sha256(32)
 *   row_roots  2k roots, col_roots 2k roots, dah 32 bytes
 *   batches    squares packed back to back in each array (mixed-k batches:
 *              square i starts after the bytes of squares 0..i-1)
 *
 * Errors: functions return 0 or a negative dagpu_status; batch calls also
 * fill a per-square status array.  dagpu_last_error() gives the message of the
 * calling thread's last failure on that context (errno-like; a thread that has
 * not failed on it gets the context's most recent message), same wording as
 * the reference where one exists.
 * Threading: a context is thread-safe.  Host-memory calls are serialised on
 * it; device-resident (*_device) calls take no lock and may be issued from
 * several threads at once, each on its own stream with its own buffers.
 */
#ifndef DAGPU_H
#define DAGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAGPU_SHARE_SIZE 512
#define DAGPU_NAMESPACE_SIZE 29
#define DAGPU_ROOT_SIZE 90
#define DAGPU_HASH_SIZE 32

typedef enum dagpu_status {
  DAGPU_OK = 0,
  DAGPU_ERR_NOT_POW2 = -1,       /* pkg/da/data_availability_header.go:67-69 */
  DAGPU_ERR_NOT_SQUARE = -2,     /* rsmt2d newDataSquare: "number of chunks must be a square number" */
  DAGPU_ERR_SHARE_SIZE = -3,     /* shares not all 512 B / shard not a multiple of 64 */
  DAGPU_ERR_PUSH_ORDER = -4,     /* nmt ErrInvalidPushOrder (Q0 namespaces unsorted) */
  DAGPU_ERR_TOO_FEW_SHARDS = -5, /* reedsolomon ErrTooFewShards */
  DAGPU_ERR_UNREPAIRABLE = -6,   /* rsmt2d ErrUnrepairableDataSquare */
  DAGPU_ERR_BYZANTINE = -7,      /* rsmt2d ErrByzantineData */
  DAGPU_ERR_BAD_ROOTS = -8,      /* rsmt2d "bad root input" */
  DAGPU_ERR_ARG = -9,
  DAGPU_ERR_DEVICE = -10,        /* HIP runtime failure */
  DAGPU_ERR_UNSUPPORTED = -11,   /* e.g. k above what this build implements */
  DAGPU_ERR_PROOF = -12,         /* a proof does not verify against the given root */
  DAGPU_ERR_SQUARE = -13         /* square construction rejected the txs (pkg/square errors) */
} dagpu_status;

typedef struct dagpu_ctx dagpu_ctx;

/* Library version (major*10000 + minor*100 + patch). */
int dagpu_version(void);

/* Widest square one GPU serves: DAGPU_MAX_SQUARE_WIDTH (the split square
 * goes to DAGPU_MAX_SPLIT_WIDTH over >= 8 GPUs, codec vectors to
 * DAGPU_MAX_CODEC_WIDTH).  pkg/da ExtendShares (data_availability_header.go:65-75)
 * checks only that the share count is a power of two, and rsmt2d's LeoRSCodec
 * reports MaxChunks() = 32768 * 32768 (Leopard GF(2^16): 65536 shards); the EDS
 * of k = 8192 is 128 GiB, which fits one MI355X's 288 GB of HBM, and k = 16384
 * (512 GiB) does not, so every square entry point returns DAGPU_ERR_UNSUPPORTED
 * above it. */
#define DAGPU_MAX_SQUARE_WIDTH 8192
uint32_t dagpu_max_square_width(void);

/* Widest codec vector (k data shards) dagpu_encode / dagpu_decode serve:
 * Leopard GF(2^16)'s limit, k + k = 65536 shards (klauspost/reedsolomon
 * leopardFF16 New: dataShards + parityShards <= 65536).  A cgo
 * LeoRSCodec.MaxChunks() over this library returns the square of it, as
 * rsmt2d's own (32768 * 32768).  DAGPU_ERR_UNSUPPORTED above it. */
#define DAGPU_MAX_CODEC_WIDTH 32768
uint32_t dagpu_max_codec_width(void);

/* Open a context on HIP device `device` (one context per GPU per process). */
int dagpu_init(int device, dagpu_ctx** out);
void dagpu_destroy(dagpu_ctx* ctx);
const char* dagpu_last_error(dagpu_ctx* ctx);  /* NULL: this thread's last context-free call */

/* Replaces da.ExtendShares + da.NewDataAvailabilityHeader + dah.Hash()
 * (pkg/da/data_availability_header.go:65-75, :44-63, :92-108) for one square.
 * shares: n_shares * share_size bytes (host).  eds_out may be NULL (roots/DAH
 * only, the device-resident default).  Errors as ExtendShares: n_shares not a
 * power of two -> DAGPU_ERR_NOT_POW2; not a square -> DAGPU_ERR_NOT_SQUARE;
 * unsorted Q0 namespaces -> DAGPU_ERR_PUSH_ORDER (NewDataAvailabilityHeader). */
int dagpu_extend_shares(dagpu_ctx* ctx, const uint8_t* shares, size_t n_shares,
                        size_t share_size, uint8_t* eds_out, uint8_t* row_roots,
                        uint8_t* col_roots, uint8_t* dah);

/* Batched host-memory form (app/extend_block.go:14-22 block replay; mixed k).
 * k[i] = original square width of square i.  status[i] gets a dagpu_status.
 * Returns DAGPU_OK if every square succeeded, else the first failing status.
 * A run of equal k larger than ~128 MiB of ODS is pipelined: chunk c goes up
 * on a copy stream while chunk c-1 is extended.  Host->device copies run at
 * PCIe speed only from page-locked memory: allocate `ods` with
 * dagpu_host_alloc or pin it with dagpu_host_register. */
int dagpu_extend_batch(dagpu_ctx* ctx, const uint8_t* ods, const uint32_t* k, size_t n,
                       uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots,
                       uint8_t* dah, int32_t* status);

/* Page-locked host memory for dagpu_extend_batch inputs (hipHostMalloc /
 * hipHostRegister).  dagpu_host_alloc returns NULL on failure. */
void* dagpu_host_alloc(size_t bytes);
void dagpu_host_free(void* p);
int dagpu_host_register(void* p, size_t bytes);
int dagpu_host_unregister(void* p);

/* Device-resident batch, one k for all n squares; every pointer is device
 * memory; work is enqueued on `stream` (hipStream_t, NULL = default stream) and
 * the call returns without synchronising.  d_ods may be NULL when Q0 is already
 * in place inside d_eds.  d_status: n int32 bitmasks (0 = OK, 1 = push order).
 * d_workspace: dagpu_workspace_size(k, n) bytes.  Every output (EDS, roots,
 * DAHs, status) is complete only when `stream` reaches the end of the call's
 * work: a large batch is hashed in slices, and the DAHs of all squares, the
 * first ones included, are written by the call's last launch. */
size_t dagpu_workspace_size(uint32_t k, size_t n);
int dagpu_extend_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_ods,
                              uint8_t* d_eds, uint8_t* d_row_roots, uint8_t* d_col_roots,
                              uint8_t* d_dah, int32_t* d_status, void* d_workspace,
                              void* stream);

/* Device-resident stages (for profiling and for callers that already hold an
 * EDS on the device): RS extension only, and NMT roots + DAH only. */
int dagpu_extend_rs_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_ods,
                           uint8_t* d_eds, void* stream);
int dagpu_roots_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_eds,
                       uint8_t* d_row_roots, uint8_t* d_col_roots, uint8_t* d_dah,
                       int32_t* d_status, void* d_workspace, void* stream);

/* Replaces NewDataAvailabilityHeader(eds) for an EDS already in host memory
 * (rsmt2d RowRoots/ColRoots + Hash). */
int dagpu_roots(dagpu_ctx* ctx, uint32_t k, const uint8_t* eds, uint8_t* row_roots,
                uint8_t* col_roots, uint8_t* dah);

/* rsmt2d.Codec (LeoRSCodec, pkg/appconsts/global_consts.go:92) Encode over many
 * vectors: data = nvec * k shards of shard_size bytes (contiguous per vector),
 * parity = nvec * k shards.  shard_size must be a multiple of 64. */
int dagpu_encode(dagpu_ctx* ctx, uint32_t k, size_t nvec, size_t shard_size,
                 const uint8_t* data, uint8_t* parity);

/* rsmt2d.Codec Decode (klauspost Reconstruct via Leopard GF(2^8)): shards =
 * nvec * 2k shards of shard_size bytes, present = nvec * 2k flags (non-zero =
 * shard present).  Missing shards are rebuilt in place.  Needs >= k present
 * per vector (DAGPU_ERR_TOO_FEW_SHARDS otherwise). */
int dagpu_decode(dagpu_ctx* ctx, uint32_t k, size_t nvec, size_t shard_size,
                 uint8_t* shards, const uint8_t* present);

/* rsmt2d ExtendedDataSquare.Repair for one square in host memory: eds is
 * (2k)^2 * 512 bytes with present[(2k)^2] flags; missing cells are filled in
 * place and every row/column root is re-verified against row_roots/col_roots
 * (DAGPU_ERR_BYZANTINE on mismatch, DAGPU_ERR_UNREPAIRABLE if the crossword
 * cannot be solved, DAGPU_ERR_BAD_ROOTS if a complete axis disagrees up front). */
int dagpu_repair(dagpu_ctx* ctx, uint32_t k, uint8_t* eds, uint8_t* present,
                 const uint8_t* row_roots, const uint8_t* col_roots);

/* dagpu_repair plus the failing axis, for rsmt2d's ErrByzantineData{Axis,
 * Index, Shares} (the input of celestia-node's bad-encoding fraud proof) and
 * its "bad root input: <axis> <i> ..." error.  byz (4 int32, may be NULL) =
 * {axis (0 row, 1 col), index, rebuilt axis, rebuilt index}, all -1 when the
 * status is neither DAGPU_ERR_BYZANTINE nor DAGPU_ERR_BAD_ROOTS.
 *   - prerepairSanityCheck failures: the first in the order i = 0..2k-1 x
 *     {row root, col root, row parity, col parity} (upstream runs these checks
 *     concurrently and returns whichever fails first in time); rebuilt = axis.
 *   - solveCrossword failures: the first failing attempt in rsmt2d's
 *     sequential order (each pass: row i, then column i).  Either the rebuilt
 *     axis' own root differs (axis = rebuilt axis) or an orthogonal axis it
 *     completed does (axis = that orthogonal axis; rebuilt = the row/column
 *     whose rebuild completed it, whose shares rsmt2d v0.11.0 attaches).
 * On DAGPU_ERR_BYZANTINE, present[] is left as rsmt2d leaves the square: the
 * cells filled by the attempts before the failing one (their bytes in eds are
 * the committed ones); ErrByzantineData.Shares = the cells of the rebuilt axis
 * with present[] set.  A prerepairSanityCheck failure (DAGPU_ERR_BAD_ROOTS, or
 * DAGPU_ERR_BYZANTINE from the check) returns before rsmt2d's crossword:
 * present[] is the input's.  The bytes of cells whose present[] flag is 0 are
 * unspecified (rsmt2d holds nil there).  Replaces ExtendedDataSquare.Repair
 * (rsmt2d v0.11.0). */
int dagpu_repair_ex(dagpu_ctx* ctx, uint32_t k, uint8_t* eds, uint8_t* present,
                    const uint8_t* row_roots, const uint8_t* col_roots, int32_t* byz);

/* Device-resident batched Repair: n squares of width k (device pointers),
 * d_present = n * (2k)^2 flags (updated in place), expected roots as produced by
 * dagpu_extend_batch_device.  d_status gets one dagpu_status per square.
 * d_workspace: dagpu_repair_workspace_size(k, n) bytes.  Enqueued on `stream`;
 * the call reads the round counters on the host once per crossword round (and
 * once more when deferred axes need their codeword check), so it returns when
 * its last command is queued.  Axes whose data
 * half is complete are re-encoded instead of decoded, and axes whose parity
 * half is complete are rebuilt by the inverse transform (same bytes);
 * DAGPU_REPAIR_FILL=0 in the environment selects the plain decoder schedule.
 * The _ex form also writes d_byz (n * 4 int32, device memory, as byz of
 * dagpu_repair_ex); a square whose crossword fails is then re-run in rsmt2d's
 * sequential order on the device to name its axis (synchronises `stream`).
 * Without d_byz the crossword's failing axis is not resolved and the cells of
 * a square with a failure are left as the batched crossword filled them. */
size_t dagpu_repair_workspace_size(uint32_t k, size_t n);
int dagpu_repair_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds,
                              uint8_t* d_present, const uint8_t* d_row_roots,
                              const uint8_t* d_col_roots, int32_t* d_status,
                              void* d_workspace, void* stream);
int dagpu_repair_batch_device_ex(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds,
                                 uint8_t* d_present, const uint8_t* d_row_roots,
                                 const uint8_t* d_col_roots, int32_t* d_status, int32_t* d_byz,
                                 void* d_workspace, void* stream);

/* dagpu_repair_batch_device split in two: dagpu_repair_start returns at once
 * (*handle names the repair); a library worker thread makes the crossword's
 * host decisions and queues its kernels on a stream of its own, forked from
 * `stream` at the call (work already queued there runs first).
 * dagpu_repair_join(ctx, handle, stream2) waits until the worker has queued
 * its last command and makes stream2 wait for the repair; it returns the
 * repair's call status (per-square results in d_status).  Repairs started back
 * to back (slices of a batch, squares of several blocks) run side by side; a
 * context serves 64 started, not yet joined repairs.  Buffer lifetime: d_eds,
 * d_present, d_status and d_workspace (and the roots) must stay valid until
 * stream2 -- the stream passed to dagpu_repair_join -- has passed the repair.
 * Free or reuse them only in stream2's order (work queued on stream2 after the
 * join, or after hipStreamSynchronize(stream2)); an allocator that frees in
 * another stream's order must first make that stream wait for stream2 (the
 * Python wrapper calls record_stream(stream2) on each buffer).  Joins from several
 * host threads wait side by side (the slot table is locked only to claim a
 * slot); a failed repair's message is re-raised on the joining thread
 * (dagpu_last_error), and a worker that cannot be started returns
 * DAGPU_ERR_DEVICE with no slot taken. */
int dagpu_repair_start(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds, uint8_t* d_present,
                       const uint8_t* d_row_roots, const uint8_t* d_col_roots, int32_t* d_status,
                       void* d_workspace, void* stream, uint64_t* handle);
int dagpu_repair_join(dagpu_ctx* ctx, uint64_t handle, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream around each
 * kernel the pipeline enqueues (for bench.py's roofline; off by default).
 * Kernel ids: 0 RS row pass, 1 RS column pass, 2 NMT leaves, 3 NMT trees,
 * 4 DAH, 5 decode, 6 Repair fill encode.  dagpu_profile_read synchronises the recorded events and
 * returns, per kernel id, the summed milliseconds and launch count since the
 * last reset (arrays of DAGPU_PROFILE_KERNELS entries). */
#define DAGPU_PROFILE_KERNELS 7
int dagpu_profile_enable(dagpu_ctx* ctx, int on);
int dagpu_profile_read(dagpu_ctx* ctx, double* total_ms, uint64_t* launches, int reset);

/* Stage timeline of the last host-path extend call (dagpu_extend_shares /
 * one-chunk dagpu_extend_batch) when dagpu_profile_enable(ctx, 2) is on:
 * ms[i] = milliseconds from the call's first enqueue to stage i (HIP events on
 * the compute stream, and on the copy stream for the EDS halves), -1 when the
 * stage did not run.  For diagnosing single-call latency. */
#define DAGPU_STAGES 10
#define DAGPU_STAGE_START 0      /* before the ODS upload */
#define DAGPU_STAGE_UPLOADED 1
#define DAGPU_STAGE_ROWS 2       /* RS row pass done */
#define DAGPU_STAGE_COLS 3       /* RS column pass done */
#define DAGPU_STAGE_LEAVES 4
#define DAGPU_STAGE_TREES 5
#define DAGPU_STAGE_DAH 6
#define DAGPU_STAGE_RESULTS 7    /* roots + DAH + status downloaded */
#define DAGPU_STAGE_EDS_TOP 8    /* [Q0|Q1] halves downloaded (copy stream) */
#define DAGPU_STAGE_EDS_BOTTOM 9 /* [Q2|Q3] halves downloaded (copy stream) */
int dagpu_profile_stages(dagpu_ctx* ctx, float* ms);

/* Schedule of the last Repair on this context (diagnostics; a started repair's
 * schedule becomes "the last" at its join, so started repairs in flight never
 * mix their counters): out[0] crossword
 * rounds that rebuilt something, out[1] vectors re-encoded from a complete data
 * half (fill), out[2] vectors rebuilt from a complete parity half (reverse
 * fill), out[3] vectors planned for the decoder, out[4] decodes deferred to the
 * other axis.  All zero with DAGPU_REPAIR_FILL=0 except out[0]. */
#define DAGPU_REPAIR_STATS 5
int dagpu_repair_stats(dagpu_ctx* ctx, int64_t* out);

/* RFC-6962 root of rowRoots || colRoots (DataAvailabilityHeader.Hash,
 * pkg/da/data_availability_header.go:92-108), computed on the host side of the
 * boundary for small inputs (w = number of row roots; w == 0 gives the
 * empty-tree hash SHA256("")). */
int dagpu_dah_hash(const uint8_t* row_roots, const uint8_t* col_roots, size_t w,
                   uint8_t* out32);

/* ---- Generic trees (batched; host buffers in, host buffers out) ---------- */

/* Leaf prefix modes of dagpu_nmt_roots (what is hashed for a push of `d`):
 *   NONE   0x00 | d            d is nmt namespaced data (ns = d[0:29])
 *   SELF   0x00 | d[0:29] | d  (wrapper Q0 cell; blob commitment leaf)
 *   PARITY 0x00 | 0xFF*29 | d  (wrapper cell outside Q0)
 *   FLAGS  per-push SELF / PARITY byte in prefix_flags */
#define DAGPU_PREFIX_NONE 0
#define DAGPU_PREFIX_SELF 1
#define DAGPU_PREFIX_PARITY 2
#define DAGPU_PREFIX_FLAGS 3

/* Roots of many namespaced Merkle trees: nmt.New(sha256.New(),
 * NamespaceIDSize(29), IgnoreMaxNamespace(ignore_max_ns)) followed by Push of
 * every leaf and Root() (nmt v0.20.0; hasher mirror
 * test/util/malicious/hasher.go:161-309).  Tree t has leaf_counts[t] pushes,
 * packed tree after tree in `leaves`, leaf_len bytes each.  roots: ntrees * 90
 * B (an empty tree gives 0^29 | 0^29 | SHA256("")).  status[t] (optional):
 * DAGPU_ERR_PUSH_ORDER when a pushed namespace is below its predecessor's
 * (ErrInvalidPushOrder); the call then returns that status. */
int dagpu_nmt_roots(dagpu_ctx* ctx, size_t ntrees, const uint32_t* leaf_counts,
                    const uint8_t* leaves, size_t leaf_len, int prefix_mode,
                    const uint8_t* prefix_flags, int ignore_max_ns, uint8_t* roots,
                    int32_t* status);

/* rsmt2d.Tree drop-in for wrapper.NewConstructor(squareSize)
 * (pkg/wrapper/nmt_wrapper.go:73-124): tree t is the
 * ErasuredNamespacedMerkleTree of axis index axis_index[t] after
 * leaf_counts[t] Push calls of share_len-byte shares (packed in `shares`);
 * returns every Root().  Same errors: square_size 0, pushes past 2*squareSize,
 * shares shorter than 29 B, namespace push order. */
int dagpu_wrapper_roots(dagpu_ctx* ctx, uint64_t square_size, size_t ntrees,
                        const uint32_t* axis_index, const uint32_t* leaf_counts,
                        const uint8_t* shares, size_t share_len, uint8_t* roots,
                        int32_t* status);

/* merkle.HashFromByteSlices (celestia-core v0.34 crypto/merkle, RFC-6962) for
 * many lists: list t has counts[t] items of item_len bytes (packed); out32 gets
 * ntrees 32-B roots (an empty list gives SHA256("")). */
int dagpu_merkle_roots(dagpu_ctx* ctx, size_t ntrees, const uint32_t* counts,
                       const uint8_t* items, size_t item_len, uint8_t* out32);

/* Every node of ONE RFC-6962 tree (merkle.ProofsFromByteSlices, celestia-core
 * crypto/merkle; pkg/proof/proof.go:87): the n leaf hashes, then each level
 * (ceil-halving, an odd last node promoted unchanged) up to the root, 32 B each.
 * *n_nodes: in = capacity of out32 in nodes, out = nodes written (or needed). */
int dagpu_merkle_levels(dagpu_ctx* ctx, size_t n, const uint8_t* items, size_t item_len,
                        uint8_t* out32, size_t* n_nodes);

/* Proof verification on the host (light-client side of pkg/proof):
 * nmt Proof.VerifyInclusion (nmt v0.20.0, IgnoreMaxNamespace, used by
 * celestia-core ShareProof.VerifyProof): n leaves of leaf_len bytes each, given
 * WITHOUT the namespace the tree prepends, proven at [start, end) by nnodes
 * 90-B nodes against a 90-B root.  crypto/merkle Proof.Verify: leaf bytes,
 * index/total and naunts 32-B aunts (leaf to root) against a 32-B root.
 * DAGPU_OK = valid, DAGPU_ERR_PROOF = does not verify, DAGPU_ERR_ARG = malformed. */
int dagpu_nmt_verify_inclusion(const uint8_t* ns29, const uint8_t* leaves, size_t n, size_t leaf_len,
                               int64_t start, int64_t end, const uint8_t* nodes, size_t nnodes,
                               const uint8_t* root90);
int dagpu_merkle_verify(const uint8_t* root32, const uint8_t* leaf, size_t leaf_len, int64_t index,
                        int64_t total, const uint8_t* aunts, size_t naunts);

/* ---- Many proofs verified in one call, hashed on the GPU ----------------
 * nmt Proof.VerifyInclusion and crypto/merkle Proof.Verify for a batch: what
 * celestia-core ShareProof.Validate / RowProof.Validate do row by row, and what
 * the reference's x/blobstream/client/verify.go:216-227 (VerifyShares) asks of
 * them, for every proof of a list at once.  The specification is the two host
 * verifiers above: status[i] is exactly what dagpu_nmt_verify_inclusion /
 * dagpu_merkle_verify returns for proof i (DAGPU_OK or DAGPU_ERR_PROOF; proof
 * byte order as there, "parity unpinned").
 *
 * A proof is one fixed record of int64 in HOST memory (both call forms);
 * offsets count leaves / nodes / aunts, and ranges of different proofs may
 * overlap in every buffer:
 *   nmt     desc[8i..]  = { start, end, n_leaves, leaf_off, n_nodes, node_off,
 *                           ns_index, root_index }
 *           leaves leaf_off .. leaf_off + n_leaves (leaf_len bytes each, WITHOUT
 *           the namespace), nodes node_off .. (90 B each), namespace ns_index
 *           of `namespaces` (29 B each), root root_index of `roots` (90 B each).
 *   merkle  desc[6i..]  = { index, total, n_aunts, aunt_off, leaf_index,
 *                           root_index }
 *           leaf leaf_index of `leaves` (leaf_len bytes each), aunts aunt_off ..
 *           (32 B each, leaf to root), root root_index of `roots32`.
 * Every descriptor is checked before anything is launched: an offset or index
 * outside the stated totals (or negative, or n_nodes > INT32_MAX) fails the
 * whole call with DAGPU_ERR_ARG and leaves `status` untouched.  A range the
 * host verifier rejects (start < 0, start >= end, n_leaves != end - start; also
 * end > 2^62, where the host verifier does not terminate) gives that proof
 * DAGPU_ERR_PROOF and does not fail the call.  The call returns DAGPU_OK when
 * it ran, whatever the per-proof results.
 *
 * dagpu_nmt_verify_batch: every buffer in host memory.
 * dagpu_nmt_verify_batch_device: bulk data and `d_status` (n int32) in device
 * memory; d_workspace (16-B aligned) of dagpu_nmt_verify_workspace_size(n, m)
 * bytes, m >= the sum of desc[i].n_leaves.  The call returns when the
 * descriptors are uploaded (it waits for `stream` up to that copy, and `desc`
 * may be freed); the kernels are enqueued only.  With leaf_len == 512,
 * d_leaves may be an extended square itself (cell (r, c) = leaf r * 2k + c):
 * samples of a resident square are verified without a copy.
 * dagpu_merkle_verify_batch: host memory; leaf_hashes (n x 32 B, optional) are
 * the proofs' own LeafHash fields, a mismatch with leafHash(leaf) gives
 * DAGPU_ERR_PROOF as in Proof.Verify. */
#define DAGPU_NMT_DESC_WORDS 8
#define DAGPU_MERKLE_DESC_WORDS 6
int dagpu_nmt_verify_batch(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* namespaces,
                           size_t n_ns, const uint8_t* leaves, size_t n_leaves, size_t leaf_len,
                           const uint8_t* nodes, size_t n_nodes, const uint8_t* roots, size_t n_roots,
                           int32_t* status);
size_t dagpu_nmt_verify_workspace_size(size_t n, size_t n_leaves);
int dagpu_nmt_verify_batch_device(dagpu_ctx* ctx, size_t n, const int64_t* desc,
                                  const uint8_t* d_namespaces, size_t n_ns, const uint8_t* d_leaves,
                                  size_t n_leaves, size_t leaf_len, const uint8_t* d_nodes, size_t n_nodes,
                                  const uint8_t* d_roots, size_t n_roots, int32_t* d_status,
                                  void* d_workspace, void* stream);
int dagpu_merkle_verify_batch(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* leaves,
                              size_t n_leaves, size_t leaf_len, const uint8_t* leaf_hashes,
                              const uint8_t* aunts, size_t n_aunts, const uint8_t* roots32, size_t n_roots,
                              int32_t* status);

/* inclusion.SubTreeWidth (pkg/inclusion/blob_share_commitment_rules.go:85-101). */
int dagpu_subtree_width(uint64_t share_count, uint32_t subtree_root_threshold);

/* inclusion.CreateCommitment (pkg/inclusion/commitment.go:19-75) for blobs
 * already split into shares (shares.SplitBlobs): blob b has namespace
 * namespaces[b*29..] and share_counts[b] 512-B shares (packed in `shares`).
 * Subtree widths from subtree_root_threshold (appconsts
 * DefaultSubtreeRootThreshold = 64); commitments: nblobs * 32 B. */
int dagpu_blob_commitments(dagpu_ctx* ctx, size_t nblobs, const uint8_t* namespaces,
                           const uint32_t* share_counts, const uint8_t* shares,
                           uint32_t subtree_root_threshold, uint8_t* commitments);

/* ---- One oversized square split over P GPUs (configs[4] stress) ---------
 * Same result as dagpu_extend_batch_device on the whole square; rank g of P
 * (P a power of two <= k) owns Q0 rows [g*k/P, (g+1)*k/P) and EDS columns
 * [g*2k/P, (g+1)*2k/P).  The caller runs the collectives (RCCL over xGMI)
 * between the steps; all pointers are device memory on `stream`:
 *   1 dagpu_split_rows_device   d_ods_rows (k/P rows of k shares) -> d_send:
 *                               P blocks of (k/P) x (2k/P) shares, block h for
 *                               rank h; zeroes then sets *d_status (push order)
 *   2 all-to-all of d_send      rank h receives the P blocks in rank order =
 *                               rows 0..k-1 of its slab (2k rows x 2k/P shares)
 *   3 dagpu_split_cols_device   fills slab rows k..2k-1, writes the slab's
 *                               2k/P column roots (90 B) and 2k row-subtree
 *                               records (96 B: minNs[32] maxNs[32] digest[32])
 *   4 all-gather row-subtree records (P x 2k x 96 B, rank order) and column
 *     roots (2k x 90 B, column order); max-reduce the status words
 *   5 dagpu_split_finish_device row roots (2k x 90 B) and the DAH (32 B)
 * Every step only enqueues on `stream` (nothing is read from host memory):
 * synchronise it before reading the results.  With P = 1 the one
 * send block is rows 0..k-1 of the slab: pass the slab itself as d_send and
 * skip step 2 (the encoder then writes [Q0 | Q1] in place).
 * d_workspace: dagpu_split_workspace_size(k, P) bytes (0 = invalid k / P).
 * Widths: every k up to DAGPU_MAX_SQUARE_WIDTH, and k = DAGPU_MAX_SPLIT_WIDTH
 * (16384: a 512 GiB EDS, beyond one GPU) over P >= 8 parts -- per rank a 64 GiB
 * column slab plus ~70 GiB of staging and forest records at P = 8;
 * DAGPU_ERR_UNSUPPORTED (workspace size 0) for fewer parts or wider squares. */
#define DAGPU_MAX_SPLIT_WIDTH 16384
size_t dagpu_split_workspace_size(uint32_t k, uint32_t parts);
int dagpu_split_rows_device(dagpu_ctx* ctx, uint32_t k, uint32_t parts, uint32_t part,
                            const uint8_t* d_ods_rows, uint8_t* d_send, int32_t* d_status,
                            void* d_workspace, void* stream);
int dagpu_split_cols_device(dagpu_ctx* ctx, uint32_t k, uint32_t parts, uint32_t part,
                            uint8_t* d_slab, uint8_t* d_col_roots, uint8_t* d_row_sub,
                            int32_t* d_status, void* d_workspace, void* stream);
int dagpu_split_finish_device(dagpu_ctx* ctx, uint32_t k, uint32_t parts,
                              const uint8_t* d_row_sub_all, const uint8_t* d_col_roots_all,
                              uint8_t* d_row_roots, uint8_t* d_dah, void* d_workspace,
                              void* stream);

/* ---- Row-tree inner nodes (nmt.NodeVisitor / inclusion.EDSSubTreeRootCacher,
 * pkg/inclusion/nmt_caching.go:81-128; share commitments from the EDS,
 * get_commit.go:12-30) ------------------------------------------------------
 * dagpu_row_nodes_device hashes every node of every row NMT of one EDS (device
 * memory) into d_nodes (dagpu_row_nodes_size(k) bytes): 96-B records minNs[32]
 * maxNs[32] digest[32]; level L (0 = leaves, log2(2k) = root) is packed after
 * level L-1, row-major, so node (row, L, p) is record
 * sum_{l<L} 2k*(2k>>l) + row*(2k>>L) + p.  Synchronises `stream`.
 * dagpu_row_nodes_gather_device reads n (row, depth, position) uint32 triples
 * (depth 0 = root) and writes n packed 90-B nodes. */
size_t dagpu_row_nodes_size(uint32_t k);
size_t dagpu_row_nodes_workspace_size(uint32_t k);
int dagpu_row_nodes_device(dagpu_ctx* ctx, uint32_t k, const uint8_t* d_eds, uint8_t* d_nodes,
                           void* d_workspace, void* stream);
int dagpu_row_nodes_gather_device(dagpu_ctx* ctx, uint32_t k, const uint8_t* d_nodes, size_t n,
                                  const uint32_t* d_requests, uint8_t* d_out, void* stream);

/* ---- Column-tree inner nodes ----------------------------------------------
 * The DAH commits to the column roots as well as the row roots, and rsmt2d /
 * celestia-node samples and the shares of a bad-encoding fraud proof are
 * proven against a column root.  The leaf node of cell (r, c) is the same in
 * row tree r and in column tree c (the wrapper's namespace prefix depends only
 * on Q0 membership), so level 0 of the row store above is level 0 of the column
 * trees too: leaf r of column c is record r*2k + c, and no leaf is hashed twice.
 * dagpu_col_nodes_device hashes levels 1 .. log2(2k) of every column tree from
 * d_row_nodes (a store filled by dagpu_row_nodes_device) into d_col_inner
 * (dagpu_col_nodes_size(k) = dagpu_row_nodes_size(k) - (2k)^2*96 bytes), the
 * same 96-B records: node (col, L, p), L >= 1, is record
 * sum_{1<=l<L} 2k*(2k>>l) + col*(2k>>L) + p; the level-log2(2k) nodes are the
 * column roots.  Both stores 16-B aligned.  Unlike the row call it only
 * ENQUEUES on `stream` and does not synchronise (nothing is uploaded);
 * d_workspace (dagpu_col_nodes_workspace_size(k) bytes) is reserved. */
size_t dagpu_col_nodes_size(uint32_t k);
size_t dagpu_col_nodes_workspace_size(uint32_t k);
int dagpu_col_nodes_device(dagpu_ctx* ctx, uint32_t k, const uint8_t* d_row_nodes, uint8_t* d_col_inner,
                           void* d_workspace, void* stream);

/* ---- Many nmt range proofs produced in one call ---------------------------
 * nmt ProveRange(start, end) on row or column trees of one resident square
 * (what pkg/proof/proof.go:87-150 asks of the wrapper tree row by row), for a
 * whole list of requests, written in the layout dagpu_nmt_verify_batch_device
 * takes: produce -> verify or produce -> ship needs no host step.  Nothing is
 * hashed: a proof is a selection of nodes of the two stores above.
 *
 * A request is one fixed record of int64 in HOST memory:
 *   req[4i..] = { axis (0 row, 1 column), index, start, end }
 * The nodes of [start, end) in a tree of 2k = 2^m leaves are the roots of the
 * maximal subtrees disjoint from the range, left to right (nmt
 * buildRangeProof): for each set bit b of start from high to low the node at
 * depth m-b, position (start>>b)-1; then for each zero bit b of end-1 from
 * b = 0 up the node at depth m-b, position ((end-1)>>b)+1;
 * popcount(start) + m - popcount(end-1) nodes, none for [0, 2k).
 *
 * Outputs, proof after proof in request order with no gaps:
 *   d_nodes_out   packed 90-B nodes (2-B aligned), nodes_cap = capacity in nodes
 *   d_ns_out      optional, n x 29 B: the min-namespace of the range's FIRST
 *                 leaf (share[0:29] inside Q0, 0xFF x 29 elsewhere)
 *   d_shares_out  optional, the proven cells, 512 B each (16-B aligned, as
 *                 d_eds), shares_cap = capacity in cells; d_eds is read only
 *                 for these and may be NULL when d_shares_out is NULL
 *   desc_out      optional, HOST, n x DAGPU_NMT_DESC_WORDS: { start, end,
 *                 n_leaves = end-start, leaf_off, n_nodes, node_off,
 *                 ns_index = i, root_index = axis*2k + index }, i.e. leaves in
 *                 d_shares_out, namespaces in d_ns_out and a roots table
 *                 row_roots || col_roots (4k x 90 B).  A single-cell row sample
 *                 may instead point leaf_off at the EDS itself
 *                 (index*2k + start), as the verifier allows.
 *   *n_nodes_total (optional) the nodes written.
 * Namespaces: VerifyInclusion prepends ONE namespace to every leaf of a proof,
 * so a range that spans several namespaces gets a correct proof that no single
 * namespace verifies; the reference's ParseNamespace (pkg/proof/querier.go)
 * rejects such ranges before proving, and callers should do the same.
 *
 * Every request is checked before anything is launched: axis not 0 / 1, index
 * outside [0, 2k), not 0 <= start < end <= 2k, an axis-1 request with
 * d_col_inner == NULL, more nodes than nodes_cap or (with d_shares_out) more
 * cells than shares_cap fails the whole call with DAGPU_ERR_ARG and leaves
 * every output, desc_out and *n_nodes_total included, untouched.
 *
 * Stream contract as dagpu_nmt_verify_batch_device: d_workspace (16-B aligned)
 * of dagpu_nmt_prove_workspace_size(n) bytes; the call returns when requests
 * and offsets are uploaded (it waits for `stream` up to that copy, and `req`
 * may be freed); the kernels are enqueued only, and a verify call on the same
 * stream may follow with no synchronisation. */
#define DAGPU_PROVE_REQ_WORDS 4
size_t dagpu_nmt_prove_workspace_size(size_t n);
int dagpu_nmt_prove_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n, const int64_t* req,
                                 const uint8_t* d_eds, const uint8_t* d_row_nodes,
                                 const uint8_t* d_col_inner, uint8_t* d_nodes_out, size_t nodes_cap,
                                 uint8_t* d_ns_out, uint8_t* d_shares_out, size_t shares_cap,
                                 int64_t* desc_out, size_t* n_nodes_total, void* d_workspace,
                                 void* stream);

/* ---- Share proofs to the data root from a whole batch of squares ----------
 * A ShareProof (pkg/proof/proof.go:58-165) is the nmt range proof of each
 * touched row under its row root (lines 127-140) plus a RowProof: the merkle
 * proof of each of those row roots under DataAvailabilityHeader.Hash, from
 * merkle.ProofsFromByteSlices over rowRoots || colRoots (lines 84-91; consumer
 * x/blobstream/client/verify.go).  The reference recomputes the EDS and every
 * tree per query; here one store holds them for all n squares of a batch.
 *
 * dagpu_proof_store_device fills d_store (dagpu_proof_store_size(k, n, ..)
 * bytes, 16-B aligned) from n extended squares in device memory, square i at
 * d_eds + i * square_stride (a multiple of 16 B, at least (2k)^2 * 512).  Three
 * regions, square-major, starts 256-B aligned:
 *   row store  offset 0, dagpu_row_nodes_size(k) bytes per square: byte for
 *              byte what dagpu_row_nodes_device writes for that EDS
 *   col store  offset *col_off, dagpu_col_nodes_size(k) bytes per square: byte
 *              for byte what dagpu_col_nodes_device writes
 *   DAH tree   offset *dah_off, (8k - 1) * 32 B per square: the RFC-6962 tree
 *              over rowRoots || colRoots (4k leaves, a power of two, so no node
 *              is promoted); level 0 = the 4k leaf hashes SHA256(0x00 | root90),
 *              level L packed after level L - 1, so node (L, p) is digest
 *              8k - (8k >> L) + p and the last digest is the data root
 * so dagpu_nmt_prove_batch_device, dagpu_nmt_namespace_* and
 * dagpu_row_nodes_gather_device work unchanged on the slices of square i.
 * The call only ENQUEUES on `stream`: the shapes are uniform, nothing is
 * uploaded and nothing is synchronised.  The number of launches does not depend
 * on n: one leaf pass over all n (2k)^2 cells, level L of the row AND column
 * trees of all squares in one launch (log2(2k) launches), each DAH level of all
 * squares in one launch (log2(4k) + 1).  No push-order check: the squares were
 * extended, and their status words say what that found.  d_workspace
 * (dagpu_proof_store_workspace_size(k, n) bytes) is reserved.  Sizes are 0 for
 * an invalid k or n = 0.
 *
 * dagpu_nmt_prove_squares_device is dagpu_nmt_prove_batch_device across the
 * squares of such a store, with one more request word,
 *   req[5i..] = { square, axis, index, start, end }     (HOST)
 * the same node rule and output order, the same d_ns_out / d_shares_out
 * semantics (cells read from d_eds + square * square_stride) and the same
 * stream contract (the call returns when the requests are uploaded; the
 * kernels are only enqueued; d_workspace 16-B aligned,
 * dagpu_nmt_prove_squares_workspace_size(n_req) bytes).  Per request i it
 * also emits the merkle half:
 *   d_axis_roots_out  i x 90 B (2-B aligned): the root of the proven tree, from
 *                     the store's top level
 *   d_leaf_hash_out   i x 32 B (16-B aligned): that root's leaf hash in the DAH tree
 *   d_aunts_out       log2(4k) x 32 B at i * log2(4k) (16-B aligned): the aunts
 *                     of leaf axis*2k + index, leaf to root, in the order of
 *                     merkle.ProofsFromByteSlices: at level L node (L, (leaf >> L) ^ 1)
 *   desc_out          HOST, n_req x DAGPU_NMT_DESC_WORDS as the single-square
 *                     call with ns_index = i and root_index = i: the roots
 *                     table of a following dagpu_nmt_verify_batch_device is
 *                     d_axis_roots_out itself
 *   mdesc_out         HOST, n_req x DAGPU_MERKLE_DESC_WORDS: { index =
 *                     axis*2k + index, total = 4k, n_aunts = log2(4k), aunt_off
 *                     = i * log2(4k), leaf_index = i, root_index = square }:
 *                     leaves are d_axis_roots_out (leaf_len 90), roots the n_sq
 *                     data roots (32 B each)
 * Each of the three merkle outputs and each descriptor array may be NULL.
 * Nothing is hashed.  A square outside [0, n_sq), axis not 0 / 1, index outside
 * [0, 2k), not 0 <= start < end <= 2k, more nodes than nodes_cap or (with
 * d_shares_out) more cells than shares_cap fails the whole call with
 * DAGPU_ERR_ARG before anything is launched; every output, the host
 * descriptors and *n_nodes_total stay untouched.
 *
 * dagpu_share_proof_requests is NewShareInclusionProof's row split
 * (pkg/proof/proof.go:63-67, 127-140) as host arithmetic, context-free:
 * sreq[3i..] = { square, start, end }, a range of row-major ODS share indexes,
 * 0 <= start < end <= k^2, becomes one 5-word request per touched row (axis 0,
 * index = row): the first from start % k, the last to (end-1) % k inclusive,
 * the rows between [0, k).  span_out (n + 1) holds the prefix sums of rows per
 * range, *n_req the total.  An invalid range or square, or more rows than
 * `cap`, gives DAGPU_ERR_ARG and writes nothing. */
#define DAGPU_PROVE_SQ_REQ_WORDS 5
size_t dagpu_proof_store_size(uint32_t k, size_t n, size_t* col_off, size_t* dah_off);
size_t dagpu_proof_store_workspace_size(uint32_t k, size_t n);
int dagpu_proof_store_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_eds,
                             size_t square_stride, uint8_t* d_store, void* d_workspace, void* stream);
size_t dagpu_nmt_prove_squares_workspace_size(size_t n_req);
int dagpu_nmt_prove_squares_device(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_req,
                                   const int64_t* req, const uint8_t* d_eds, size_t square_stride,
                                   const uint8_t* d_store, uint8_t* d_nodes_out, size_t nodes_cap,
                                   uint8_t* d_ns_out, uint8_t* d_shares_out, size_t shares_cap,
                                   uint8_t* d_axis_roots_out, uint8_t* d_leaf_hash_out,
                                   uint8_t* d_aunts_out, int64_t* desc_out, int64_t* mdesc_out,
                                   size_t* n_nodes_total, void* d_workspace, void* stream);
int dagpu_share_proof_requests(uint32_t k, size_t n_sq, size_t n, const int64_t* sreq,
                               int64_t* req_out, size_t cap, int64_t* span_out, size_t* n_req);

/* ---- Namespace proofs: ProveNamespace / VerifyNamespace -------------------
 * "Every share of namespace N in this square, with a proof that nothing was
 * left out": nmt ProveNamespace, Proof.VerifyNamespace and absence proofs (what
 * celestia-node's GetSharesByNamespace serves per row).  nmt is not part of the
 * reference tree (it only calls ProveRange, pkg/proof/proof.go:140): like
 * VerifyInclusion above, the rules are recalled from nmt v0.20.0 and are
 * "parity unpinned".  THIS BLOCK IS THEIR SPECIFICATION.
 *
 * Namespaces are 29 bytes compared bytewise, IgnoreMaxNamespace is on, nodes
 * are 90 B (min | max | digest).  Leaves are given WITHOUT the namespace the
 * tree prepends, as for dagpu_nmt_verify_inclusion; a leaf is hashed as
 * 0x00 | nid | leaf.
 *
 * ProveNamespace(tree, nid) on one full tree of 2k leaves with root R:
 *   1 nid < R.min or R.max < nid: the EMPTY proof, start = end = 0, no nodes,
 *     no leaf hash.  R.max is the stored one: in rows < k it ignores the parity
 *     leaves, so the parity namespace is outside those rows and is the whole
 *     row in rows >= k.
 *   2 leaves with ns == nid exist (contiguous, [s, e)): the PRESENCE proof,
 *     range [s, e) with the ProveRange(s, e) nodes, no leaf hash.
 *   3 otherwise the ABSENCE proof: s = the first leaf with ns > nid, range
 *     [s, s+1) with the ProveRange(s, s+1) nodes, and leafHash = the 90-B leaf
 *     node of s.  No leaf data is carried.
 *
 * VerifyNamespace(proof, nid, leaves, root):
 *   1 empty form (start == end, no nodes, no leaf hash): valid iff there are no
 *     leaves and nid < root.min or root.max < nid.
 *   2 else start < 0, start >= end or end > 2^62 fail the proof.
 *   3 absence (a leaf hash is given): invalid with any leaves, with
 *     end - start != 1, or unless nid < leafHash.min; the one leaf node of the
 *     fold is leafHash itself.
 *   4 presence: invalid unless n_leaves == end - start; leaf nodes are
 *     nid | nid | SHA256(0x00 | nid | leaf).
 *   5 the fold of dagpu_nmt_verify_inclusion, unchanged (same code).
 *   6 completeness: every proof node consumed for a subtree left of the range
 *     must have max < nid, every one consumed right of it (the leftover nodes
 *     folded on the right included) nid < min.
 * dagpu_nmt_verify_namespace is the host verifier (leaf_hash90 NULL unless
 * absence); return codes as dagpu_nmt_verify_inclusion.
 *
 * Batched on the GPU: dagpu_nmt_verify_namespace_batch (host buffers) and
 * dagpu_nmt_verify_namespace_batch_device mirror the two inclusion calls with
 * 9-word descriptors: words 0-7 as DAGPU_NMT_DESC_WORDS, word 8 =
 * leaf_hash_index into `leaf_hashes` (90 B each), -1 = none.  The descriptor
 * checks are the same plus that index (< -1 or >= n_leaf_hashes):
 * DAGPU_ERR_ARG, status untouched.  Proofs that rules 2-4 reject from the
 * descriptor alone get DAGPU_ERR_PROOF with no device work; status[i] equals
 * what dagpu_nmt_verify_namespace returns for proof i.  Stream and workspace
 * contract as dagpu_nmt_verify_batch_device, with
 * dagpu_nmt_verify_namespace_workspace_size(n, m), m >= the sum of n_leaves;
 * d_leaves may be a resident EDS.
 *
 * From a resident square, ROW trees only (column trees are out of scope: a
 * namespace is contiguous along rows of Q0 and that is what nodes serve):
 * dagpu_nmt_namespace_ranges_device classifies n_q namespaces (HOST, 29 B
 * each) against every row tree of the row store d_row_nodes
 * (dagpu_row_nodes_device; root records in its top level, leaf namespaces in
 * level 0): ranges_out (HOST) gets n_q x 2k x { kind, start, end } int32, kind
 * DAGPU_NS_OUTSIDE / PRESENT / ABSENT (start = end = 0 outside); counts_out[4]
 * = { proofs with kind != 0, absence proofs, proof nodes, proven cells }.  It
 * synchronises `stream` once, for the read-back.
 * dagpu_nmt_prove_namespace_batch_device searches the same way, lays the
 * proofs with kind != 0 out in (query, row) order and enqueues: their nodes
 * (d_nodes_out, 90 B each, 2-B aligned), the proven shares of presence proofs
 * (d_shares_out, 512 B each, 16-B aligned; d_eds is the square), the absence
 * proofs' leaf hashes (d_leaf_hashes_out, level-0 nodes packed 90 B, 2-B
 * aligned) and d_ns_out = the n_q query namespaces.  On the HOST it writes one
 * 9-word descriptor per proof (desc_out: ns_index = query, root_index = row
 * into a row-roots table, n_leaves = 0 and leaf_hash_index = running count for
 * absence) and pairs_out, { query, row } int32 per proof: the layout
 * dagpu_nmt_verify_namespace_batch_device takes, and that call may follow on
 * the same stream with no synchronisation.  Capacities are arguments
 * (proofs_cap, nodes_cap, shares_cap, leaf_hashes_cap); when one is too small
 * the call returns DAGPU_ERR_ARG, counts_out holds what is needed and every
 * other output is untouched.  n_q = 0 is DAGPU_OK: counts_out = 0, nothing
 * else written.  d_workspace (16-B aligned) of
 * dagpu_nmt_namespace_workspace_size(k, n_q) bytes serves both calls. */
#define DAGPU_NMT_NS_DESC_WORDS 9
#define DAGPU_NS_OUTSIDE 0
#define DAGPU_NS_PRESENT 1
#define DAGPU_NS_ABSENT 2
int dagpu_nmt_verify_namespace(const uint8_t* ns29, const uint8_t* leaves, size_t n, size_t leaf_len,
                               int64_t start, int64_t end, const uint8_t* nodes, size_t nnodes,
                               const uint8_t* leaf_hash90, const uint8_t* root90);
int dagpu_nmt_verify_namespace_batch(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* namespaces,
                                     size_t n_ns, const uint8_t* leaves, size_t n_leaves, size_t leaf_len,
                                     const uint8_t* nodes, size_t n_nodes, const uint8_t* leaf_hashes,
                                     size_t n_leaf_hashes, const uint8_t* roots, size_t n_roots,
                                     int32_t* status);
size_t dagpu_nmt_verify_namespace_workspace_size(size_t n, size_t n_leaves);
int dagpu_nmt_verify_namespace_batch_device(dagpu_ctx* ctx, size_t n, const int64_t* desc,
                                            const uint8_t* d_namespaces, size_t n_ns, const uint8_t* d_leaves,
                                            size_t n_leaves, size_t leaf_len, const uint8_t* d_nodes,
                                            size_t n_nodes, const uint8_t* d_leaf_hashes, size_t n_leaf_hashes,
                                            const uint8_t* d_roots, size_t n_roots, int32_t* d_status,
                                            void* d_workspace, void* stream);
size_t dagpu_nmt_namespace_workspace_size(uint32_t k, size_t n_q);
int dagpu_nmt_namespace_ranges_device(dagpu_ctx* ctx, uint32_t k, size_t n_q, const uint8_t* namespaces,
                                      const uint8_t* d_row_nodes, int32_t* ranges_out, int64_t* counts_out,
                                      void* d_workspace, void* stream);
int dagpu_nmt_prove_namespace_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n_q, const uint8_t* namespaces,
                                           const uint8_t* d_eds, const uint8_t* d_row_nodes,
                                           uint8_t* d_nodes_out, size_t nodes_cap, uint8_t* d_ns_out,
                                           uint8_t* d_shares_out, size_t shares_cap,
                                           uint8_t* d_leaf_hashes_out, size_t leaf_hashes_cap,
                                           int64_t* desc_out, int32_t* pairs_out, size_t proofs_cap,
                                           int64_t* counts_out, void* d_workspace, void* stream);

/* ---- Namespace proofs across the squares of a batch proof store -----------
 * dagpu_nmt_prove_namespace_squares_device is
 * dagpu_nmt_prove_namespace_batch_device for all n_sq squares of a
 * dagpu_proof_store_device store in one call, with the merkle half to the data
 * root that dagpu_nmt_prove_squares_device emits.  The rules are exactly those
 * of the block above (row trees only, all 2k rows of every square; nothing new
 * is recalled from nmt, parity stays unpinned as stated there), and the
 * single-square call is the specification: the proof of (query, square, row)
 * is byte for byte what it emits for (query, row) on the slices of that square.
 *
 * One search runs over every (query, square, row); the hits are counted,
 * ordered and laid out on the device, and the emit, share-gather and merkle
 * kernels read their tables from there.  Proofs with kind != 0 are listed in
 * (query, square, row) order, ascending.  counts_out[4] (HOST) = { proofs,
 * absence proofs, proof nodes, proven cells } over the whole batch.
 *   namespaces        HOST, n_q x 29 B
 *   d_eds             square i at d_eds + i * square_stride (16-B aligned both;
 *                     square_stride >= (2k)^2 * 512)
 *   d_store           the batch proof store of the n_sq squares (16-B aligned)
 *   d_nodes_out, d_shares_out, d_leaf_hashes_out, d_ns_out
 *                     as in the single-square call: the proofs' nodes (90 B each,
 *                     2-B aligned), the cells of presence proofs (512 B each,
 *                     16-B aligned), the level-0 nodes of absence proofs (90 B,
 *                     2-B aligned) and the n_q query namespaces (29 B each)
 *   d_axis_roots_out  i x 90 B (2-B aligned): the row root of proof i
 *   d_dah_leaf_hash_out  i x 32 B (16-B aligned): its leaf hash in the DAH tree
 *   d_aunts_out       log2(4k) x 32 B at i * log2(4k) (16-B aligned): the aunts
 *                     of leaf `row` of 4k, leaf to root
 *                     -- each of the three may be NULL, as in
 *                     dagpu_nmt_prove_squares_device
 *   desc_out          HOST, DAGPU_NMT_NS_DESC_WORDS per proof: ns_index = query,
 *                     root_index = i (the roots table of a following
 *                     dagpu_nmt_verify_namespace_batch_device is
 *                     d_axis_roots_out itself), n_leaves = 0 and
 *                     leaf_hash_index = running absence count for an absence
 *                     proof, -1 otherwise
 *   mdesc_out         HOST, may be NULL: DAGPU_MERKLE_DESC_WORDS per proof,
 *                     { row, 4k, log2(4k), i * log2(4k), i, square }: leaves are
 *                     d_axis_roots_out (leaf_len 90), roots the n_sq data roots
 *   hits_out          HOST, DAGPU_NS_HIT_WORDS int32 per proof:
 *                     { query, square, row, kind, start, end }
 * A dagpu_nmt_verify_namespace_batch_device and a dagpu_merkle_verify_batch
 * may follow with no synchronisation beyond what the call itself did.
 *
 * dagpu_nmt_namespace_squares_count_device runs the search and the count
 * alone: counts_out as above and, when per_out (HOST, n_q x n_sq int32, query
 * major) is not NULL, the proofs of every (query, square): which squares hold
 * a namespace.
 *
 * Cost: the number of launches depends on neither n_sq nor n_q.  The proof
 * call synchronises `stream` at most twice (after the count, to size the
 * outputs against the capacities; after the hit records are read back and
 * before the emit kernels are enqueued), the count call once.  Nothing but the
 * padded query namespaces is uploaded.  Host work and PCIe traffic are
 * O(n_q + proofs), for per_out O(n_q * n_sq), never O(n_q * n_sq * 2k).  What
 * comes back from the device, the four totals and every hit record, is
 * re-checked on the host before anything is sized or emitted from it; a
 * violation returns DAGPU_ERR_DEVICE.  The tables the emit kernels read are
 * written on the device by the same lanes as the hit records and are not read
 * back: the re-check does not cover them.
 *
 * d_workspace (16-B aligned): dagpu_nmt_namespace_squares_workspace_size(k,
 * n_sq, n_q, proofs_cap) bytes, proofs_cap = 0 for the count call: 4 B per
 * (query, square, row), 32 B per 256 of them, and 48 B per proof of
 * proofs_cap.  The size is 0 for an invalid k, n_sq = 0 or a count that
 * overflows (n_q * n_sq * 2k must stay below 2^31 - 256).
 *
 * DAGPU_ERR_ARG before any launch: an invalid k, n_sq = 0, a null or
 * misaligned buffer, a square_stride smaller than a square, a (query, square,
 * row) count or a size that overflows.  When a capacity (proofs_cap,
 * leaf_hashes_cap, nodes_cap, shares_cap) is too small the call returns
 * DAGPU_ERR_ARG, counts_out holds the need and every other output, the host
 * arrays included, is untouched.  n_q = 0 is DAGPU_OK: counts_out = 0, nothing
 * else written.  A batch in which nothing hits is DAGPU_OK with zero counts;
 * only d_ns_out is written. */
#define DAGPU_NS_HIT_WORDS 6
size_t dagpu_nmt_namespace_squares_workspace_size(uint32_t k, size_t n_sq, size_t n_q, size_t proofs_cap);
int dagpu_nmt_namespace_squares_count_device(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_q,
                                             const uint8_t* namespaces, const uint8_t* d_store,
                                             int64_t* counts_out, int32_t* per_out, void* d_workspace,
                                             void* stream);
int dagpu_nmt_prove_namespace_squares_device(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_q,
                                             const uint8_t* namespaces, const uint8_t* d_eds,
                                             size_t square_stride, const uint8_t* d_store,
                                             uint8_t* d_nodes_out, size_t nodes_cap, uint8_t* d_ns_out,
                                             uint8_t* d_shares_out, size_t shares_cap,
                                             uint8_t* d_leaf_hashes_out, size_t leaf_hashes_cap,
                                             uint8_t* d_axis_roots_out, uint8_t* d_dah_leaf_hash_out,
                                             uint8_t* d_aunts_out, int64_t* desc_out, int64_t* mdesc_out,
                                             int32_t* hits_out, size_t proofs_cap, int64_t* counts_out,
                                             void* d_workspace, void* stream);

/* ---- Square construction (host; pkg/square, app version 1) ---------------
 * square.Construct (pkg/square/square.go:22-63, builder.go): ntx txs packed
 * back to back in `txs` (tx_lens[i] bytes each; blob txs in the BlobTx proto
 * wire format, pkg/blob/blob.go:56-90) -> the original data square, k*k
 * 512-B shares row-major, in ods_out (ods_cap bytes; k*k*512 needed, k <=
 * max_square_size; *square_size = k is set even when ods_out is too small,
 * which returns DAGPU_ERR_ARG).  Every tx must fit and normal txs must come
 * before blob txs, else DAGPU_ERR_SQUARE with the reference's message
 * ("not enough space to append tx at index 3", ...).  max_square_size =
 * SquareSizeUpperBound (128) and subtree_root_threshold = 64 for app v1.
 * The ODS goes straight into dagpu_extend_shares / the device batch API.
 * ctx may be NULL (then no message is kept).  No device work.
 * A single tx of 4 GiB or more is refused (DAGPU_ERR_SQUARE, "tx at index i
 * has 4 GiB or more"), here and in dagpu_square_build / dagpu_square_plan: the
 * BlobTx parser shared with the device planner (csrc/square_plan.hpp) walks a
 * tx with 32-bit offsets. */
int dagpu_square_construct(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                           uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* ods_out,
                           size_t ods_cap, uint32_t* square_size);
/* square.Build: txs that do not fit are skipped (kept[i] = 0), normal txs may
 * follow blob txs; the reference returns the kept normal txs, then the kept
 * blob txs, in input order within each group. */
int dagpu_square_build(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                       uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* ods_out,
                       size_t ods_cap, uint32_t* square_size, uint8_t* kept);

/* ---- Square construction on the device: plan on the host, write in HBM ----
 * The entry of block replay is txs, not an ODS (app/extend_block.go:14-22:
 * square.Construct, then da.ExtendShares; app/prepare_proposal.go:87-107 and
 * app/process_proposal.go:135-161 start from txs too).  These calls split
 * square.Construct / square.Build (pkg/square/square.go:22-63, builder.go
 * Export, WriteSquare) into the layout, decided on the host, and the writing
 * of the k*k shares (pkg/shares/split_compact_shares.go, split_sparse_shares.go,
 * padding.go), done by one function per share that the host executor and the
 * kernel share (csrc/square_write.hpp).
 *
 * dagpu_square_plan: the arguments, checks, return codes and messages of
 * dagpu_square_construct (kept == NULL) or dagpu_square_build (kept != NULL,
 * filled as there), but the result is a plan: a relocatable blob of tables
 * with no pointers, whose source references are offsets into `txs`.  It copies
 * no payload byte.  *plan_bytes and *square_size are set even when plan_out
 * (plan_cap bytes, 4-B aligned) is too small, which returns DAGPU_ERR_ARG.
 * DAGPU_ERR_UNSUPPORTED for txs of 2 GiB or more, or a square wider than 1024.
 * Thread-safe: blocks of a batch may be planned on several threads.
 *
 * dagpu_square_plan_check: every offset and range of a plan against its own
 * size and src_bytes of txs, the runs covering shares 0 .. k*k-1 once and in
 * order, and the order of the tables the writer searches; DAGPU_ERR_ARG on any
 * violation (message: dagpu_last_error(NULL)).  The writers trust a plan only
 * after it: both run it first.  The one exception is
 * dagpu_square_construct_device (below), whose writer takes plans the device
 * planner has just made in device memory and trusts them on the planner's
 * own bounds.
 *
 * dagpu_square_plan_write_host: the square of a plan and its txs, row r at
 * ods_out + r * row_pitch (row_pitch >= k*512; bytes between rows untouched). */
int dagpu_square_plan(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                      uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* kept, uint8_t* plan_out,
                      size_t plan_cap, size_t* plan_bytes, uint32_t* square_size);
int dagpu_square_plan_check(const uint8_t* plan, size_t plan_bytes, size_t src_bytes);
int dagpu_square_plan_write_host(const uint8_t* plan, size_t plan_bytes, const uint8_t* txs, size_t src_bytes,
                                 uint8_t* ods_out, size_t row_pitch);
/* n planned squares of one width k written in HBM by one kernel (one wave per
 * share).  plans[i] / plan_bytes[i] (HOST) is block i's plan, its packed txs
 * lie at d_src + src_offs[i] (src_offs: n + 1 HOST offsets, ascending, the last
 * <= src_bytes, the size of d_src); square i goes to d_ods + i * square_stride
 * with rows row_pitch bytes apart: row_pitch = k*512 and square_stride =
 * k*k*512 is the packed ODS batch, row_pitch = 2k*512 and square_stride =
 * 4k*k*512 writes Q0 of an EDS batch in place, the zero-copy input of
 * dagpu_extend_batch_device (d_ods = NULL).  d_ods, square_stride and row_pitch
 * are multiples of 16; bytes outside each square's k x (k*512) window are not
 * touched.  Every plan is checked (dagpu_square_plan_check) and must have width
 * k, else DAGPU_ERR_ARG (the message names the block) and nothing is enqueued.
 * d_workspace (16-B aligned, dagpu_square_write_workspace_size(n, sum of
 * plan_bytes) bytes) receives the plans and must stay valid until the kernel
 * has run; with NULL the library allocates it and the call also waits for the
 * kernel.  The call returns after the upload of the plans has left host
 * memory (plans, plan_bytes and src_offs may be freed at once) and, with a
 * workspace, before the kernel has run: it is enqueued on `stream`. */
size_t dagpu_square_write_workspace_size(size_t n, size_t plan_bytes_total);
int dagpu_square_write_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* const* plans,
                              const size_t* plan_bytes, const uint8_t* d_src, const size_t* src_offs,
                              size_t src_bytes, uint8_t* d_ods, size_t square_stride, size_t row_pitch,
                              void* d_workspace, void* stream);

/* ---- Square plans made on the device: raw txs to plans with no host pass ---
 * dagpu_square_plan (kept == NULL, square.Construct) for n blocks at once, on
 * the device: the packed txs of the blocks are in HBM (d_src, src_offs[n + 1]
 * HOST offsets as in dagpu_square_write_device, each block below 2 GiB), ntx[n]
 * (HOST) is each block's tx count and tx_lens (HOST) the lengths of all blocks'
 * txs back to back; every block's lengths must add up to its src_offs span.
 * The library uploads the lengths in one copy, then two kernels run on
 * `stream` (csrc/square_plan.hip; arithmetic csrc/square_plan.hpp, shared with
 * dagpu_square_plan): one lane per tx classifies it (blob.UnmarshalBlobTx),
 * one workgroup per block replays Construct's append loop as a scan, sorts
 * the blobs, walks NextShareIndex, sizes the PFB stream and emits the plan.
 * max_square_size: a power of two <= 128, else DAGPU_ERR_UNSUPPORTED;
 * square.Build (kept != NULL) is not offered.  Outputs, all DEVICE, 16-B
 * aligned:
 *   d_plans    the plan arena, plans_cap bytes.  Block i's plan is byte for
 *              byte what dagpu_square_plan returns for it, at a 16-B aligned
 *              offset the device chooses (one atomic add per block: the order
 *              of the plans in the arena is not fixed).
 *   d_records  n records of 32 bytes { uint64 plan_off, uint64 src_off,
 *              uint32 plan_bytes, k, status, nblob }: where the plan lies, the
 *              square width found, the status below.  plan_bytes = 0 for a
 *              rejected block: it gets no plan.
 *   d_status   n uint32: 0, or kind | index << 8, nonzero exactly for the
 *              blocks dagpu_square_plan rejects, the first error in its order:
 *                DAGPU_PLAN_NO_SPACE_TX / _NO_SPACE_BLOB_TX / _TX_AFTER_BLOB_TX
 *                    with the tx index of the reference's message
 *                DAGPU_PLAN_LAYOUT    any error of Export / WriteSquare, with
 *                    the index of the blob in namespace order where there is one
 *                DAGPU_PLAN_TOO_MANY_BLOBS  more than max_square_size^2 blobs
 *                    (an empty blob fails Export, any other costs a share)
 *                DAGPU_PLAN_ARENA     plans_cap is below the bound
 * The message of a rejected block is dagpu_square_plan's on that block.
 * Bounds: a block of t txs has a plan of at most 216 + 41 t + 51 m^2 bytes
 * (m = max_square_size: 2 segments and 1 unit per tx, 48 B per blob, 5 B of
 * delimiter per tx, 21 B of IndexWrapper head and tail per PFB, 3 B per share
 * index); dagpu_square_plan_device_arena_size(n, ntx_total, m) is the sum over
 * the blocks.  dagpu_square_plan_device_workspace_size(n, ntx_total, m) =
 * 16 + 32 n + 64 ntx_total + n * (32 KiB + 64 m^2) bytes: 64 B per tx of
 * tables, 64 B per possible blob, the sorted order.  For 256 full blocks
 * (4,000 txs each, m = 128) that is 0.34 GB of workspace and 0.26 GB of arena;
 * the plans themselves take 0.2 MB per block.  d_workspace (16-B aligned) must
 * stay valid until the kernels have run; with NULL the library allocates it
 * and waits.  Checked before anything is enqueued: null pointers, alignment,
 * ascending src_offs, the tx_lens sums, the 2 GiB and 2^24 txs per block.
 * Every kernel read of d_src stays inside the tx it parses: a length field
 * that points past its tx rejects the tx as a blob tx, it is not followed.
 *
 * dagpu_square_construct_device: the same, then the squares of width k written
 * as dagpu_square_write_device writes them (d_ods, square_stride, row_pitch),
 * from the device's records with no host synchronisation between.  A block
 * with a nonzero status, or whose width is not k (its status becomes
 * DAGPU_PLAN_WIDTH | found width << 8), is skipped: not a byte of its square's
 * window is touched.  The writers above trust a plan only after
 * dagpu_square_plan_check; this one trusts the plans the planner has just made
 * in device memory the caller has not touched, on the bounds above.
 *
 * dagpu_square_plan_emulate_host: the same arguments and outputs in HOST
 * memory, the kernels' algorithm run as host loops (256 lanes per phase, the
 * same scan chunks and sorting network); plans lie in block order.  For tests
 * and for planning without a device.  No context. */
#define DAGPU_PLAN_NO_SPACE_TX 1
#define DAGPU_PLAN_NO_SPACE_BLOB_TX 2
#define DAGPU_PLAN_TX_AFTER_BLOB_TX 3
#define DAGPU_PLAN_LAYOUT 4
#define DAGPU_PLAN_TOO_MANY_BLOBS 5
#define DAGPU_PLAN_WIDTH 6
#define DAGPU_PLAN_ARENA 7
#define DAGPU_PLAN_RECORD_BYTES 32
size_t dagpu_square_plan_device_workspace_size(size_t n, size_t ntx_total, uint32_t max_square_size);
size_t dagpu_square_plan_device_arena_size(size_t n, size_t ntx_total, uint32_t max_square_size);
int dagpu_square_plan_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs, size_t src_bytes,
                             const uint32_t* ntx, const uint64_t* tx_lens, uint32_t max_square_size,
                             uint32_t subtree_root_threshold, uint8_t* d_plans, size_t plans_cap, void* d_records,
                             uint32_t* d_status, void* d_workspace, void* stream);
int dagpu_square_construct_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_src, const size_t* src_offs,
                                  size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                                  uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* d_plans,
                                  size_t plans_cap, void* d_records, uint8_t* d_ods, size_t square_stride,
                                  size_t row_pitch, uint32_t* d_status, void* d_workspace, void* stream);
int dagpu_square_plan_emulate_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes,
                                   const uint32_t* ntx, const uint64_t* tx_lens, uint32_t max_square_size,
                                   uint32_t subtree_root_threshold, uint8_t* plans, size_t plans_cap, void* records,
                                   uint32_t* status);

/* ---- Share commitments from squares resident in HBM ----------------------
 * ProcessProposal recomputes every blob's share commitment and compares it
 * with the one its MsgPayForBlobs declares (x/blob/types/blob_tx.go:91-100,
 * called at app/process_proposal.go:120) before it builds the square.  With
 * the squares written in HBM (dagpu_square_write_device) the commitments of
 * every blob of every block of a batch come from those bytes in one enqueue:
 * inclusion.CreateCommitment (pkg/inclusion/commitment.go:19-75) depends on
 * the blob's shares alone.
 *
 * dagpu_square_plan_blobs: the blob table of a plan, 4 uint32 per blob
 * {first_share, share_count, data_off, data_len} in plan order (ascending
 * first_share; the plan sorts blobs by namespace, so this is not tx order).
 * data_off is the offset of the blob's data in the block's packed txs: a
 * caller that parsed the BlobTxs ties a plan blob back to (tx, blob index)
 * with it, and so to the commitment the PFB declares.  Runs
 * dagpu_square_plan_check first (DAGPU_ERR_ARG, message dagpu_last_error(NULL));
 * needs no context and no device.  *nblob is set even when cap (in blobs) is
 * too small, which returns DAGPU_ERR_ARG.
 *
 * dagpu_blob_commitments_device: n squares of width k addressed as in
 * dagpu_square_write_device (square i at d_squares + i * square_stride, rows
 * row_pitch apart: the packed ODS batch or Q0 inside an EDS batch), and nblobs
 * HOST records of three int64 {square, first_share, share_count}: blob b is
 * shares [first, first + count) of that square in row-major order over the
 * k x k ODS.  For each, with w = SubTreeWidth(count, subtree_root_threshold)
 * (blob_share_commitment_rules.go:85-101) and the split of
 * MerkleMountainRangeSizes(count, w) (commitment.go:85-107): the nmt root of
 * each subtree, leaf j = 0x00 | share[0:29] | share (namespace | share for a
 * range that is one blob, commitment.go:53-63), nodes by nmt HashNode with
 * IgnoreMaxNamespace; then merkle.HashFromByteSlices of the 90-B roots
 * (commitment.go:73) into d_commitments[b*32..].
 * d_status[b] (int32): 0, or the OR of
 *   DAGPU_COMMIT_MISMATCH    d_expected != NULL and the 32 bytes differ from
 *                            d_expected[b*32..] (the comparison of
 *                            blob_tx.go:96-99)
 *   DAGPU_COMMIT_PUSH_ORDER  inside some subtree a leaf's namespace is below
 *                            its predecessor's (nmt ErrInvalidPushOrder); the
 *                            commitment bytes of such a blob are unspecified.
 *                            Ranges of <= threshold shares have one-leaf
 *                            subtrees and never set it, as in nmt.
 * d_square_status (n int32, may be NULL) is zeroed on the stream and receives
 * the OR of the statuses of each square's blobs: one read of n words tells
 * which blocks to reject.
 * Checked on the host before anything is enqueued: k a power of two (<= 1024,
 * else DAGPU_ERR_UNSUPPORTED), threshold > 0, row_pitch >= k*512, d_squares,
 * square_stride and row_pitch multiples of 16, and for every record
 * 0 <= square < n, count >= 1, 0 <= first, first + count <= k*k; a refusal
 * returns DAGPU_ERR_ARG and its message names the blob.  nblobs == 0 is valid
 * and only zeroes d_square_status.
 * d_workspace (16-B aligned, dagpu_blob_commitments_workspace_size(k, nblobs,
 * sum of share counts) bytes) must stay valid until the kernels have run; the
 * call returns once the tables have left host memory, with three kernels
 * enqueued on `stream`.  With NULL the library allocates it and waits. */
#define DAGPU_COMMIT_MISMATCH 1
#define DAGPU_COMMIT_PUSH_ORDER 2
size_t dagpu_blob_commitments_workspace_size(uint32_t k, size_t nblobs, size_t nshares_total);
int dagpu_blob_commitments_device(dagpu_ctx* ctx, uint32_t k, size_t n, size_t nblobs,
                                  const int64_t* blobs /* HOST, 3 per blob */, const uint8_t* d_squares,
                                  size_t square_stride, size_t row_pitch, uint32_t subtree_root_threshold,
                                  uint8_t* d_commitments, const uint8_t* d_expected /* may be NULL */,
                                  int32_t* d_status, int32_t* d_square_status /* may be NULL */,
                                  void* d_workspace, void* stream);
int dagpu_square_plan_blobs(const uint8_t* plan, size_t plan_bytes, uint32_t* out, size_t cap, size_t* nblob);

/* ---- ValidateBlobTx on the device: PFB decode and the stateless rules ------
 * The other half of what ProcessProposal does per tx before it builds the
 * square (app/process_proposal.go:60-77, :120): the rules of ValidateBlobTx
 * (x/blob/types/blob_tx.go:36-103) short of the comparison of the commitments
 * (blob_tx.go:92-100), which dagpu_blob_commitments_device makes against the
 * table of declared commitments this call fills.  One function per tx
 * (csrc/blobtx_check.hpp, shared by the kernels of csrc/blobtx_check.hip and
 * the host executor) returns a word kind | index << 8, the first failure in
 * the reference's order:
 *   a BlobTx (blob.UnmarshalBlobTx, pkg/blob/blob.go:56-90):
 *   DECODE         the inner tx does not decode (blob_tx.go:37-40).  The SDK's
 *                  TxDecoder is not in the reference: the rule is the project's
 *                  walker (Tx 1 body -> TxBody 1 messages -> Any {1 type_url,
 *                  2 value}; a malformed buffer or a wrong wire type on one of
 *                  those four fields); the SDK's stricter rejections are not
 *                  restated.
 *   MULTIPLE_MSGS  message count != 1 (blob_tx.go:44-47); index = the count,
 *                  capped at 2^24 - 1
 *   NO_PFB         type_url is not /celestia.blob.v1.MsgPayForBlobs (:49-52)
 *   PFB_DECODE     the message value is malformed, or a wrong wire type on its
 *                  fields 1, 2, 3, 4 or 8 (repeated uint32 packed or not)
 *   MsgPayForBlobs.ValidateBasic (x/blob/types/payforblob.go:95-148):
 *   NO_NAMESPACES, NO_SHARE_VERSIONS, NO_BLOB_SIZES, NO_SHARE_COMMITMENTS
 *                  (:96-110), MISMATCHED_COUNTS (:112-117)
 *   INVALID_NAMESPACE (namespace.From, :120-123), RESERVED_NAMESPACE
 *                  (IsReserved, :184; pkg/namespace/namespace.go:108-118),
 *                  INVALID_NAMESPACE_VERSION (:188); index = the namespace
 *   UNSUPPORTED_SHARE_VERSION (:130-134); index = the share version
 *   BAD_SIGNER     sdk.AccAddressFromBech32 with the prefix "celestia"
 *                  (:136-139): BIP-173 bech32, the 5 -> 8 bit regrouping without
 *                  padding, 1 to 255 bytes.  The SDK is not vendored in the
 *                  reference: recalled, parity unpinned beyond the addresses
 *                  the reference's files contain.
 *   BAD_COMMITMENT_LENGTH (:141-145); index = the commitment
 *   ValidateBlobs (payforblob.go:211-239), index = the blob:
 *   BLOB_NAMESPACE_VERSION_TOO_LARGE (:217), BLOB_INVALID_NAMESPACE (:220),
 *   BLOB_RESERVED_NAMESPACE, BLOB_INVALID_NAMESPACE_VERSION (:224),
 *   ZERO_BLOB_SIZE (:229), BLOB_UNSUPPORTED_SHARE_VERSION (:233)
 *   SIZE_MISMATCH  blob_tx.go:69; index = the first blob whose len(data) is not
 *                  blob_sizes[i], or the smaller count when the counts differ
 *   NAMESPACE_MISMATCH  blob_tx.go:73-89; index = the lowest such blob
 *   any other tx (process_proposal.go:60-77): 0 when it does not decode,
 *   NON_BLOB_TX_HAS_PFB (:72-76) with index = the first message whose type_url
 *   is the PFB url, else 0.
 *
 * dagpu_blob_tx_check: the word of one tx in host memory; never reads a byte
 * at or past n.  n is below 2 GiB, the bound of a block's txs; a longer buffer
 * is not walked and gives 0.
 *
 * dagpu_blob_tx_validate_device: the txs of n blocks as
 * dagpu_square_plan_device takes them (d_src, HOST src_offs[n + 1], src_bytes,
 * HOST ntx[n], HOST tx_lens) with its request checks and messages, the plan
 * arena and records it left in HBM (d_plans, plans_cap, d_records), and HOST
 * blob_base[n + 1]: block i's plan blobs own rows [blob_base[i],
 * blob_base[i + 1]) of the expected table, block by block in plan order (the
 * order of dagpu_square_plan_blobs; a block without a plan owns no rows).
 * blob_base == NULL ties nothing: d_plans, d_records and d_expected are then
 * not read.  Outputs, all DEVICE:
 *   d_tx_status     one word per tx of the batch, in batch order
 *   d_block_status  two words per block, 8-B aligned: {index in the block of
 *                   its lowest failing tx, or 0xFFFFFFFF; that tx's word, or 0}
 *   d_expected      32 bytes per row: the commitment the blob's MsgPayForBlobs
 *                   declares, found through the plan blob's data_off; zeros
 *                   for a row whose tx failed before its commitment lengths
 *                   were checked, or that ties to no blob.  Every row is written.
 * Three kernels on `stream`: one lane per tx, one per block, one per row.
 * Checked before anything is enqueued (DAGPU_ERR_ARG and a message): null
 * pointers, alignment, blob_base starting at 0 and ascending, and the planner's
 * checks of src_offs / ntx / tx_lens.  d_workspace (16-B aligned,
 * dagpu_blob_tx_validate_workspace_size(n, ntx_total, blob_base[n]) = 48 n +
 * 32 ntx_total + 32 bytes at most) must stay valid until the kernels have run;
 * the call returns once its tables have left host memory.  With NULL the
 * library allocates it and waits.
 *
 * dagpu_blob_tx_validate_host: the same arguments and outputs in HOST memory,
 * the same per-tx and per-row functions run as loops.  No context, no device. */
#define DAGPU_BLOBTX_OK 0
#define DAGPU_BLOBTX_DECODE 1
#define DAGPU_BLOBTX_MULTIPLE_MSGS 2
#define DAGPU_BLOBTX_NO_PFB 3
#define DAGPU_BLOBTX_PFB_DECODE 4
#define DAGPU_BLOBTX_NO_NAMESPACES 5
#define DAGPU_BLOBTX_NO_SHARE_VERSIONS 6
#define DAGPU_BLOBTX_NO_BLOB_SIZES 7
#define DAGPU_BLOBTX_NO_SHARE_COMMITMENTS 8
#define DAGPU_BLOBTX_MISMATCHED_COUNTS 9
#define DAGPU_BLOBTX_INVALID_NAMESPACE 10
#define DAGPU_BLOBTX_RESERVED_NAMESPACE 11
#define DAGPU_BLOBTX_INVALID_NAMESPACE_VERSION 12
#define DAGPU_BLOBTX_UNSUPPORTED_SHARE_VERSION 13
#define DAGPU_BLOBTX_BAD_SIGNER 14
#define DAGPU_BLOBTX_BAD_COMMITMENT_LENGTH 15
#define DAGPU_BLOBTX_BLOB_NAMESPACE_VERSION_TOO_LARGE 16
#define DAGPU_BLOBTX_BLOB_INVALID_NAMESPACE 17
#define DAGPU_BLOBTX_BLOB_RESERVED_NAMESPACE 18
#define DAGPU_BLOBTX_BLOB_INVALID_NAMESPACE_VERSION 19
#define DAGPU_BLOBTX_ZERO_BLOB_SIZE 20
#define DAGPU_BLOBTX_BLOB_UNSUPPORTED_SHARE_VERSION 21
#define DAGPU_BLOBTX_SIZE_MISMATCH 22
#define DAGPU_BLOBTX_NAMESPACE_MISMATCH 23
#define DAGPU_BLOBTX_NON_BLOB_TX_HAS_PFB 24
uint32_t dagpu_blob_tx_check(const uint8_t* tx, size_t n);
size_t dagpu_blob_tx_validate_workspace_size(size_t n, size_t ntx_total, size_t nblobs_total);
int dagpu_blob_tx_validate_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs,
                                  size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                                  const uint8_t* d_plans, size_t plans_cap, const void* d_records,
                                  const uint64_t* blob_base /* HOST, n + 1, may be NULL */, uint32_t* d_tx_status,
                                  uint32_t* d_block_status, uint8_t* d_expected, void* d_workspace, void* stream);
int dagpu_blob_tx_validate_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes,
                                const uint32_t* ntx, const uint64_t* tx_lens, const uint8_t* plans, size_t plans_cap,
                                const void* records, const uint64_t* blob_base, uint32_t* tx_status,
                                uint32_t* block_status, uint8_t* expected);

/* ---- ProcessProposal on the device: raw txs to verdicts in one read ---------
 * The commitment check laid out where the plans lie, and the verdict of the
 * data-parallel part of ProcessProposal (app/process_proposal.go:53-164) per
 * block.  Arithmetic in csrc/commit_plan.hpp, shared by the kernels and the
 * host executors.
 *
 * dagpu_commit_plan_device / dagpu_commit_plan_host: from the plan arena and
 * SpRecord[n] dagpu_square_plan_device left (d_plans, plans_cap, d_records) to
 * the tables dagpu_blob_commitments_device's kernels read, for the batch's
 * width k and subtree_root_threshold, with no download:
 *   d_tables    the image commit_layout builds from the same blobs, word for
 *               word: blob[nblobs]{square, first_share} | share_pre[nblobs + 1]
 *               | sub_pre[nblobs + 1] | sub[nsub]{blob, first leaf, size} |
 *               work[nwork]; blocks in order, a block's blobs in plan order
 *   d_counts    8 words {nblobs, nshares, nsub, nwork, max_subtrees, 0, 0, 0}
 *   d_blob_base n + 1 uint64: block i owns rows [blob_base[i], blob_base[i + 1])
 * A block contributes nothing when its record has a status, no plan
 * (plan_bytes == 0) or another width than k, when an offset of its record or
 * plan header passes plan_bytes or plans_cap (nothing outside is read), or when
 * its blobs do not fit k * k shares.  Capacities need no read:
 *   shares, rows, subtrees and blobs <= n * k * k;  work items <= n * k * k / 2;
 *   d_tables holds dagpu_commit_plan_table_words(k, n) = 7.5 n k^2 + 2 words.
 * k a power of two <= 1024 (else DAGPU_ERR_UNSUPPORTED), threshold > 0,
 * n * k * k < 2^31, n < 2^24; d_plans, d_records, d_tables, d_counts 16-B and
 * d_blob_base 8-B aligned.  Three kernels on `stream`, no copy and no wait with
 * a workspace (dagpu_commit_plan_workspace_size(k, n) bytes, 16-B aligned);
 * with NULL the library allocates it and waits.  The host executor runs the
 * same functions as loops over host memory; no context, no device.
 *
 * dagpu_proposal_check_device: the request as dagpu_blob_tx_validate_device
 * takes it (with its checks and messages) and the squares
 * dagpu_square_construct_device wrote (d_squares, square_stride, row_pitch as
 * in dagpu_blob_commitments_device).  Enqueues the per-tx rules (d_tx_status,
 * d_block_status as there), the layout above, the tie of every row to its
 * declared commitment and the three commitment kernels in their counted forms
 * (grids of min(capacity, a fixed multiple of the CU count) workgroups striding
 * over the counts the layout left in d_counts).  Outputs, all DEVICE, sized by capacity
 * cap = n * k * k:
 *   d_expected, d_commitments  cap x 32 B; rows [0, blob_base[n]) are written
 *   d_blob_status   cap int32, DAGPU_COMMIT_* per row, zeroed up to cap first
 *   d_row_tx        cap x 2 uint32: the block-local index of the tx that owns
 *                   the row's blob and the blob's index inside that tx, or
 *                   0xFFFFFFFF twice for a row that does not tie
 *   d_square_status n int32, the OR over each block's rows, zeroed first
 *   d_counts (8 words), d_blob_base (n + 1 uint64) as above
 * No device-to-host copy; the call returns once its tables have left the
 * context's page-locked staging.  d_workspace:
 * dagpu_proposal_check_workspace_size(k, n, ntx_total) bytes, 16-B aligned,
 * valid until the kernels have run; NULL: the library allocates and waits.
 *
 * dagpu_proposal_verdict_device / _host: four uint32 per block {code, tx, word,
 * aux} from the records, the check's outputs, extend's per-square status and
 * data roots (d_extend_status, d_dah; may be NULL) and two HOST arrays that may
 * be NULL: data_hashes (n x 32) and square_sizes (n uint32), uploaded on
 * `stream` through the context's page-locked staging.  The first code that
 * applies, in the reference's order:
 *   NON_BLOB_TX_HAS_PFB (:75) / INVALID_BLOB_TX (:120)  the lowest failing tx of
 *       the loop fails a stateless rule; tx, word = its DAGPU_BLOBTX_* word
 *   CALCULATE_COMMITMENT / INVALID_SHARE_COMMITMENT (:120, blob_tx.go:91-100)
 *       the lowest failing tx fails on a commitment (DAGPU_COMMIT_PUSH_ORDER /
 *       _MISMATCH); tx, aux = the blob's index in the tx.  The tx reported is
 *       the lowest over both rule sets; a tx that fails both ways reports the
 *       stateless word, as ValidateBlobTx does; within a tx the lowest blob,
 *       its push-order fault before its mismatch.
 *   CONSTRUCT_FAILED (:135-139)  the planner rejected the block; word = its
 *       status.  No square was written for such a block, so a commitment
 *       mismatch in it cannot be seen: its code is its lowest stateless failure
 *       if it has one, else this one.  It is rejected either way.
 *   SQUARE_SIZE_DIFFERS (:142-145)  square_sizes given and != the block's
 *       width; aux = the computed width
 *   NOT_JUDGED  the block's width is not k: no square was written, nothing was
 *       compared; the caller sends the block to a batch of its width.  Never
 *       an accept.
 *   EXTEND_FAILED (:147-157), DATA_ROOT_DIFFERS (:161-164), ACCEPT.
 * Two kernels: one lane per row with a status folds its key into its block's
 * word (64-bit atomic min), one lane per block writes the record.  d_workspace:
 * dagpu_proposal_verdict_workspace_size(k, n, ntx_total) bytes.  Refusals of
 * all three calls (null pointers, misalignment, k, threshold, pitch) return
 * DAGPU_ERR_ARG / DAGPU_ERR_UNSUPPORTED with a message before anything is
 * enqueued; no output byte is touched. */
#define DAGPU_VERDICT_ACCEPT 0
#define DAGPU_VERDICT_NON_BLOB_TX_HAS_PFB 1
#define DAGPU_VERDICT_INVALID_BLOB_TX 2
#define DAGPU_VERDICT_CALCULATE_COMMITMENT 3
#define DAGPU_VERDICT_INVALID_SHARE_COMMITMENT 4
#define DAGPU_VERDICT_CONSTRUCT_FAILED 5
#define DAGPU_VERDICT_SQUARE_SIZE_DIFFERS 6
#define DAGPU_VERDICT_NOT_JUDGED 7
#define DAGPU_VERDICT_EXTEND_FAILED 8
#define DAGPU_VERDICT_DATA_ROOT_DIFFERS 9
size_t dagpu_commit_plan_table_words(uint32_t k, size_t n);
size_t dagpu_commit_plan_workspace_size(uint32_t k, size_t n);
int dagpu_commit_plan_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_plans, size_t plans_cap,
                             const void* d_records, uint32_t subtree_root_threshold, uint32_t* d_tables,
                             uint32_t* d_counts, uint64_t* d_blob_base, void* d_workspace, void* stream);
int dagpu_commit_plan_host(uint32_t k, size_t n, const uint8_t* plans, size_t plans_cap, const void* records,
                           uint32_t subtree_root_threshold, uint32_t* tables, uint32_t* counts, uint64_t* blob_base);
size_t dagpu_proposal_check_workspace_size(uint32_t k, size_t n, size_t ntx_total);
int dagpu_proposal_check_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_src, const size_t* src_offs,
                                size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                                const uint8_t* d_plans, size_t plans_cap, const void* d_records,
                                const uint8_t* d_squares, size_t square_stride, size_t row_pitch,
                                uint32_t subtree_root_threshold, uint32_t* d_tx_status, uint32_t* d_block_status,
                                uint8_t* d_expected, uint8_t* d_commitments, int32_t* d_blob_status,
                                uint32_t* d_row_tx, int32_t* d_square_status, uint32_t* d_counts,
                                uint64_t* d_blob_base, void* d_workspace, void* stream);
size_t dagpu_proposal_verdict_workspace_size(uint32_t k, size_t n, size_t ntx_total);
int dagpu_proposal_verdict_device(dagpu_ctx* ctx, uint32_t k, size_t n, const void* d_records,
                                  const uint32_t* d_block_status, const int32_t* d_blob_status,
                                  const uint32_t* d_row_tx, const uint64_t* d_blob_base,
                                  const int32_t* d_extend_status /* may be NULL */,
                                  const uint8_t* d_dah /* may be NULL */,
                                  const uint8_t* data_hashes /* HOST, may be NULL */,
                                  const uint32_t* square_sizes /* HOST, may be NULL */, uint32_t* d_verdicts,
                                  void* d_workspace, void* stream);
int dagpu_proposal_verdict_host(uint32_t k, size_t n, const void* records, const uint32_t* block_status,
                                const int32_t* blob_status, const uint32_t* row_tx, const uint64_t* blob_base,
                                const int32_t* extend_status, const uint8_t* dah, const uint8_t* data_hashes,
                                const uint32_t* square_sizes, uint32_t* verdicts);

/* ---- Tx signatures: batched secp256k1 ECDSA, SIGN_MODE_DIRECT ---------------
 * The stateless half of the SigVerificationDecorator (app/ante/ante.go:55,
 * reached from app/process_proposal.go:103 and :126): one secp256k1 ECDSA
 * verification over SHA-256(SignDoc) per tx, as cosmos-sdk v0.46
 * crypto/keys/secp256k1 PubKey.VerifySignature makes it.  The stateful inputs
 * (account numbers, stored public keys) come in as tables; the sequence
 * comparison, the account lookup, the key-to-address check, fees and gas stay
 * with the caller, who gets the signer records for them.  Arithmetic in
 * csrc/secp256k1.hpp and csrc/tx_sig.hpp, shared by the kernels
 * (csrc/tx_sig.hip) and the host executors (csrc/tx_sig_host.cpp).
 *
 * A status word is kind | index << 8.  0 is DAGPU_SIG_OK.  Not judged (the
 * caller's host path decides these; none is a rejection):
 *   TX_UNDECODABLE      the walk Tx -> AuthInfo -> SignerInfo -> Any / ModeInfo
 *                       fails, the body's messages included
 *                       (process_proposal.go:60-66 skips such a tx).  The walker
 *                       is this project's (unknown fields skipped, the last of
 *                       a field wins); the SDK's stricter canonical-encoding
 *                       rejections are not restated.
 *   UNSUPPORTED_SIGNERS signer_infos or signatures count != 1; index = the
 *                       signer_infos count, capped at 2^24 - 1
 *   UNSUPPORTED_MODE    not Single {SIGN_MODE_DIRECT}; index = the mode, 0 for
 *                       Multi or none
 *   UNSUPPORTED_PUBKEY_TYPE  a public_key whose type_url is not
 *                       /cosmos.crypto.secp256k1.PubKey
 *   NO_PUBKEY           none in the tx and none in the table
 * Rejecting, checked in this order (the reference reports every one of them as
 * ErrUnauthorized, so the order is this project's own):
 *   BAD_PUBKEY          key length != 33, prefix not 0x02 / 0x03, x >= p, or
 *                       x^3 + 7 not a square
 *   BAD_LENGTH          signature length != 64; index = the length, capped
 *   OUT_OF_RANGE        r = 0, r >= n or s = 0
 *   HIGH_S              s > n / 2 (malleable)
 *   MISMATCH            with z = SHA-256(sign bytes), w = 1 / s mod n:
 *                       R = (z w) G + (r w) Q is infinity, or R.x mod n != r
 *
 * dagpu_secp256k1_verify_device / _host: the generic batch: n digests (32 B
 * each), signatures (64 B, big-endian r | s) and compressed keys (33 B); one
 * word per item, 0 or BAD_PUBKEY, OUT_OF_RANGE, HIGH_S, MISMATCH.  One kernel
 * on `stream`, one lane per item, no copy and no wait.
 *
 * dagpu_secp256k1_g_table: the 15 affine multiples 1 G .. 15 G the
 * verification adds by 4-bit window, 64 bytes each (big-endian x | y): the
 * committed constants (recompute = 0), or computed by the library's own point
 * arithmetic (recompute = 1); the tests compare both with the Python mirror.
 *
 * dagpu_tx_signers_device / _host: the request as dagpu_blob_tx_validate_device
 * takes it (d_src, HOST src_offs[n + 1], src_bytes, HOST ntx[n], HOST tx_lens)
 * with its request checks and messages.  d_signers (8-B aligned), 48 bytes per
 * tx of the batch: {pubkey[33], kind u8, pad[6], sequence u64 little-endian}:
 * the key the tx carries (zeros when it carries none of 33 bytes), the kind
 * the walk alone gives (no table: NO_PUBKEY says the tx carries no key; kinds
 * up to BAD_LENGTH), and the sequence it declares (0 for TX_UNDECODABLE and
 * UNSUPPORTED_SIGNERS).  A BlobTx is unwrapped to its inner tx first.
 *
 * dagpu_tx_sig_verify_device / _host: the same request plus chain_id (HOST
 * bytes, chain_id_len <= 64 or DAGPU_ERR_ARG), d_account_numbers (one uint64
 * per tx of the batch, 8-B aligned) and d_pubkeys (may be NULL; ntx_total x
 * 33; a row whose first byte is 0 means none; a present row is the key used,
 * whatever key the tx carries, as the account's stored key is in the
 * reference).  The sign bytes are the proto3 encoding of SignDoc {body_bytes 1,
 * auth_info_bytes 2, chain_id 3, account_number 4} with body_bytes and
 * auth_info_bytes the exact byte ranges of the tx's fields 1 and 2, a field
 * omitted when empty or 0; they are streamed into SHA-256, never materialised.
 * Outputs, all DEVICE:
 *   d_tx_status     one word per tx of the batch, in batch order
 *   d_block_status  four words per block: {index in the block of its lowest tx
 *                   with a rejecting kind, or 0xFFFFFFFF; that tx's word, or
 *                   0; the number of not-judged txs; 0}
 *   d_signers       as above
 * Three kernels on `stream`: one lane per tx (walk, hash), one lane per tx
 * (curve arithmetic; a tx whose word is final leaves at once), one per block.
 * d_workspace (16-B aligned, dagpu_tx_sig_verify_workspace_size(n, ntx_total)
 * = 44 n + 152 ntx_total + 96 bytes at most) must stay valid until the kernels
 * have run; the call returns once its tables have left host memory and does
 * not wait for the kernels.  With NULL the library allocates it and waits.
 * The host executors run the same functions as loops; no context, no device. */
#define DAGPU_SIG_OK 0
#define DAGPU_SIG_TX_UNDECODABLE 1
#define DAGPU_SIG_UNSUPPORTED_SIGNERS 2
#define DAGPU_SIG_UNSUPPORTED_MODE 3
#define DAGPU_SIG_UNSUPPORTED_PUBKEY_TYPE 4
#define DAGPU_SIG_NO_PUBKEY 5
#define DAGPU_SIG_BAD_PUBKEY 16
#define DAGPU_SIG_BAD_LENGTH 17
#define DAGPU_SIG_OUT_OF_RANGE 18
#define DAGPU_SIG_HIGH_S 19
#define DAGPU_SIG_MISMATCH 20
int dagpu_secp256k1_verify_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_digests, const uint8_t* d_sigs,
                                  const uint8_t* d_pubkeys, uint32_t* d_status, void* stream);
int dagpu_secp256k1_verify_host(size_t n, const uint8_t* digests, const uint8_t* sigs, const uint8_t* pubkeys,
                                uint32_t* status);
int dagpu_secp256k1_g_table(uint8_t* out /* 15 x 64 */, int recompute);
size_t dagpu_tx_sig_verify_workspace_size(size_t n, size_t ntx_total);
int dagpu_tx_signers_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs, size_t src_bytes,
                            const uint32_t* ntx, const uint64_t* tx_lens, uint8_t* d_signers, void* d_workspace,
                            void* stream);
int dagpu_tx_signers_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
                          const uint64_t* tx_lens, uint8_t* signers);
int dagpu_tx_sig_verify_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs,
                               size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                               const uint8_t* chain_id /* HOST */, size_t chain_id_len,
                               const uint64_t* d_account_numbers, const uint8_t* d_pubkeys /* may be NULL */,
                               uint32_t* d_tx_status, uint32_t* d_block_status, uint8_t* d_signers,
                               void* d_workspace, void* stream);
int dagpu_tx_sig_verify_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes,
                             const uint32_t* ntx, const uint64_t* tx_lens, const uint8_t* chain_id,
                             size_t chain_id_len, const uint64_t* account_numbers, const uint8_t* pubkeys,
                             uint32_t* tx_status, uint32_t* block_status, uint8_t* signers);

/* ---- Square read: txs and blobs back out of squares resident in HBM -------
 * The opposite direction of dagpu_square_write_device: square.Deconstruct
 * (pkg/square/square.go:65-155) split into a scan of the shares
 * (shares.ParseShares, pkg/shares/parse.go:42-97), a gather of the payload that
 * was asked for, and the walk over the tx streams (parseRawData,
 * pkg/shares/parse_compact_shares.go:47-66): dagpu_compact_units walks one
 * downloaded stream serially on the host; dagpu_square_units_device ("Tx
 * index" below) walks every stream of a batch where it lies, one lane per
 * share.  The arithmetic is csrc/square_read.hpp, shared by the host executor
 * and the kernels (csrc/square_read.hip).
 *
 * Squares are addressed as in dagpu_square_write_device (square i at
 * d_squares + i * square_stride, rows row_pitch apart: the packed ODS batch or
 * Q0 inside an EDS batch), with its limits, alignment checks and messages.
 *
 * dagpu_square_scan_device / dagpu_square_scan_host:
 * shares.ParseShares(shares, ignorePadding = false) of n squares of width k.
 * Of each share the first 38 bytes count (pkg/shares/shares.go:60-200): the
 * namespace (29 B), the info byte (share version << 1 | sequence start), on a
 * start share the big-endian sequence length, on a compact share (tx or PFB
 * namespace) the big-endian reserved bytes; Share.IsPadding (shares.go:115-143)
 * is "start share of sequence length 0, or the tail padding or the primary
 * reserved padding namespace"; the content is the last 474 (compact start),
 * 478 (compact continuation, sparse start) or 482 bytes of the share.  A
 * sequence is a start share and the continuation shares up to the next start
 * share; sequences never cross squares.
 * Records: sequence j of square i, in share order, at d_records[i * seq_cap +
 * j], j < min(n_sequences, seq_cap); other records are not written.  flags:
 * exactly one of DAGPU_SEQ_SPARSE / _TX / _PFB; DAGPU_SEQ_PADDING for a
 * sequence of one share that IsPadding (ShareSequence.isPadding,
 * share_sequence.go:44-52); the first share's version from bit
 * DAGPU_SEQ_VERSION_SHIFT.  reserved_bytes: the first share's, compact only.
 * payload_len: 0 for padding, sequence_len for a blob, 474 + 478 (count - 1)
 * for a compact sequence (the content of all its shares, uncut: extractRawData,
 * parse_compact_shares.go:72-86, does not cut at the sequence length either).
 * Summary, 8 int32 per square: {code, index, the lowest share whose share
 * version is not 0 or -1, n_sequences, n_blob_sequences, blob_payload_bytes,
 * compact_payload_bytes, 0}; the two byte totals are the sums over the
 * non-padding sparse / compact sequences of payload_len rounded up to 16,
 * which is what dagpu_square_read_device needs for them, and mean something
 * only when code is DAGPU_SCAN_OK.  ParseShares ignores share versions;
 * ParseBlobs and ParseTxs refuse one that is not 0 (parse_compact_shares.go:35-42,
 * parse_sparse_shares.go:37-41), so the third word tells whether they would.
 * code / index: the first error in the reference's order.
 *   pass 1, ascending share i (parse.go:51-75):
 *     DAGPU_SCAN_NAMESPACE     namespace.From rejects share i's namespace: not
 *                              version 0 with 18 zero ID bytes, nor version 255
 *                              (pkg/namespace/namespace.go:40-58, :95-113)
 *     DAGPU_SCAN_INCONSISTENT  share i is a continuation and no start share
 *                              precedes it, or its namespace differs from that
 *                              of the nearest start share before it
 *     the lowest i wins; on one share NAMESPACE comes first
 *   pass 2, if pass 1 found nothing (parse.go:77-82, share_sequence.go:54-76):
 *     DAGPU_SCAN_LENGTH        index = the first share of the lowest sequence
 *                              that is not padding and whose share count is not
 *                              CompactSharesNeeded / SparseSharesNeeded of its
 *                              sequence length (share_sequence.go:106-142)
 *   then DAGPU_SCAN_OVERFLOW   n_sequences > seq_cap; index = n_sequences
 *                              (seq_cap = k*k never overflows)
 * summary_out (HOST, may be NULL) receives a copy of the summary and makes the
 * call wait for it; without it, and with a workspace, everything is only
 * enqueued on `stream` (four launches).  d_records and d_summary are 16-B
 * aligned.  d_workspace: dagpu_square_scan_workspace_size(k, n) bytes, 16-B
 * aligned; NULL: the library allocates it and waits.  A refusal returns
 * DAGPU_ERR_ARG with a message and enqueues nothing.  The host executor
 * computes the same records and summary serially; it needs no context and no
 * device (message: dagpu_last_error(NULL)).
 *
 * dagpu_square_read_device: the payload of the sequences that were asked for.
 * Selected: the non-padding sequences, of squares whose code is DAGPU_SCAN_OK,
 * whose class is in class_mask (DAGPU_READ_BLOBS: sparse; DAGPU_READ_COMPACT:
 * tx and PFB) and whose namespace is one of the n_ns HOST namespaces (29 B
 * each; NULL / 0: every namespace).  In (square, share) order, selected
 * sequence m has d_selected[m] = its index into the record table, and
 * d_offsets[m] = its 16-B aligned offset into d_payload, the sum of the
 * earlier ones' payload_len rounded up to 16.  d_totals = {n_selected,
 * payload_bytes (that sum over all of them), overflow}.  A sequence whose
 * payload would end past payload_cap is not gathered and sets overflow = 1; the
 * others are.  A blob yields its sequence_len bytes (478 of its first share,
 * 482 of each continuation, the last one cut), a compact sequence the content
 * of all its shares.  Bytes between payloads and past them are not written.
 * d_selected and d_offsets hold n * seq_cap entries, d_totals 3.  d_workspace:
 * dagpu_square_read_workspace_size(k, n, seq_cap, n_ns) bytes, 16-B aligned; with
 * it the call is enqueued on `stream` (four launches) and returns once the
 * namespace list has left host memory; with NULL the library allocates it and
 * waits.
 *
 * dagpu_compact_units: parseRawData over a compact sequence's payload: the
 * units (txs, or wrapped PFBs) from the first share's reserved bytes on.
 * first_unit is that reserved value, a byte index into the first share: 0
 * gives no units (Share.RawDataUsingReserved), 38 .. 511 starts at payload
 * byte first_unit - 38, anything else is DAGPU_ERR_ARG.  Each unit is a
 * uvarint length read as ParseDelimiter does (pkg/shares/utils.go:92-117: a
 * 10-byte zero-padded window, skipping the value's canonical length) and that
 * many bytes; the walk stops at a length of 0 or one longer than what is left.
 * out_off[i] / out_len[i]: unit i's bytes in `stream`.  *n is set even when cap
 * is too small, which returns DAGPU_ERR_ARG; a varint that overflows 64 bits
 * is DAGPU_ERR_SQUARE with the reference's message.  No context, no device. */
#define DAGPU_SCAN_OK 0
#define DAGPU_SCAN_NAMESPACE 1
#define DAGPU_SCAN_INCONSISTENT 2
#define DAGPU_SCAN_LENGTH 3
#define DAGPU_SCAN_OVERFLOW 4
#define DAGPU_SCAN_SUMMARY_WORDS 8
#define DAGPU_SEQ_SPARSE 1
#define DAGPU_SEQ_TX 2
#define DAGPU_SEQ_PFB 4
#define DAGPU_SEQ_PADDING 8
#define DAGPU_SEQ_VERSION_SHIFT 8
#define DAGPU_READ_BLOBS 1
#define DAGPU_READ_COMPACT 2
typedef struct dagpu_seq_record {
  uint8_t ns[32]; /* 29 bytes, zero padded */
  uint32_t first_share, share_count, sequence_len, flags, reserved_bytes, payload_len;
  uint32_t pad[2];
} dagpu_seq_record; /* 64 bytes */
size_t dagpu_square_scan_workspace_size(uint32_t k, size_t n);
int dagpu_square_scan_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares, size_t square_stride,
                             size_t row_pitch, uint32_t seq_cap, dagpu_seq_record* d_records, int32_t* d_summary,
                             int32_t* summary_out /* HOST, may be NULL */, void* d_workspace, void* stream);
int dagpu_square_scan_host(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride, size_t row_pitch,
                           uint32_t seq_cap, dagpu_seq_record* records, int32_t* summary);
size_t dagpu_square_read_workspace_size(uint32_t k, size_t n, uint32_t seq_cap, size_t n_ns);
int dagpu_square_read_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares, size_t square_stride,
                             size_t row_pitch, uint32_t seq_cap, const dagpu_seq_record* d_records,
                             const int32_t* d_summary, const uint8_t* namespaces /* HOST, may be NULL */, size_t n_ns,
                             uint32_t class_mask, uint32_t* d_selected, uint64_t* d_offsets, uint64_t* d_totals,
                             uint8_t* d_payload, size_t payload_cap, void* d_workspace, void* stream);
int dagpu_compact_units(const uint8_t* stream, size_t len, uint32_t first_unit, uint64_t* out_off, uint64_t* out_len,
                        size_t cap, size_t* n);

/* ---- Tx index: where unit i of a block lies in a resident square ----------
 * A unit is what parseRawData yields: a tx in the tx namespace, a wrapped PFB
 * (IndexWrapper) in the PFB namespace.  Block tx order is every unit of the tx
 * namespace's sequences in share order, then every unit of the PFB
 * namespace's: the index Builder.FindTxShareRange (pkg/square/builder.go:268-317)
 * and NewTxInclusionProof (pkg/proof/proof.go:23-45) take.  The arithmetic is
 * csrc/square_units.hpp, shared by the host executor, the host loop that
 * emulates the kernels and the kernels (csrc/square_units.hip); the argument
 * why one lane per share finds what the serial walk finds stands there.
 *
 * dagpu_square_units_device: over the squares, records and summary of
 * dagpu_square_scan_device (same addressing, same seq_cap), unit j of square i
 * at d_units[i * unit_cap + j], j < min(n_units, unit_cap):
 *   start_share, end_share  row-major ODS share indexes, end exclusive: the
 *                           share that holds the first byte of the unit's
 *                           length delimiter, and 1 + the share that holds its
 *                           last data byte (FindTxShareRange of a square the
 *                           Builder made)
 *   seq                     the unit's sequence in the square's record table
 *   flags                   DAGPU_SEQ_TX or DAGPU_SEQ_PFB
 *   offset, len             the unit's data bytes in its sequence's payload
 *                           (what dagpu_square_read_device gathers for it), as
 *                           dagpu_compact_units reports out_off / out_len
 * Unit summary, 8 int32 per square: {code, index, n_units, n_tx_units,
 * n_pfb_units, the sum of len rounded up to 16, 0, 0}:
 *   DAGPU_UNITS_OK        the table is bit for bit the serial walk's
 *                         (dagpu_square_units_host)
 *   DAGPU_UNITS_SCAN      the square's scan code is not DAGPU_SCAN_OK; nothing
 *                         is produced
 *   DAGPU_UNITS_HOST      the device could not establish that its walk equals
 *                         the serial one, or the serial walk would report an
 *                         error; index = the lowest share where this showed.
 *                         The table is not to be used: run the host executor
 *                         on that square
 *   DAGPU_UNITS_OVERFLOW  n_units > unit_cap; index = n_units, the first
 *                         unit_cap records are written
 * and words 2 .. 5 are 0 unless the code is OK or OVERFLOW.  No square the
 * Builder made takes the HOST code.  unit_summary_out (HOST, may be NULL)
 * receives a copy of the summary and makes the call wait for it; without it,
 * and with a workspace, the call only enqueues four launches on `stream`.
 * d_units and d_unit_summary are 16-B aligned.  d_workspace:
 * dagpu_square_units_workspace_size(k, n) bytes, 16-B aligned; NULL: the
 * library allocates it and waits.
 *
 * dagpu_square_units_host: the host executor, authoritative: the serial walk
 * (dagpu_compact_units) over each non-padding compact sequence of host squares
 * and their host records and summary.  Never DAGPU_UNITS_HOST.  The first
 * square with a sequence the serial walk refuses ends the call: a varint that
 * overflows 64 bits is DAGPU_ERR_SQUARE, a first reserved value outside {0,
 * 38 .. 511} DAGPU_ERR_ARG, with dagpu_compact_units' messages; that square's
 * summary is zeroed, the squares before it are complete.  No context, no device.
 * dagpu_square_units_emulate_host: the kernels' algorithm as a host loop over
 * all shares, the same per-lane functions: the same table and summary as
 * dagpu_square_units_device, DAGPU_UNITS_HOST included.  For tests and for
 * checking a square without a device.
 *
 * dagpu_square_read_units_device: the data bytes of selected units.  pairs:
 * m HOST pairs {square, unit index} of uint32.  Unit pairs[t] goes to d_payload
 * at d_offsets[t], a multiple of 16: the sum over the earlier pairs of len
 * rounded up to 16.  d_totals = {m, payload_bytes, flags}: flags bit 0
 * (overflow) when a unit would end past payload_cap, which is then not
 * gathered, the others are; bit 1 (DAGPU_READ_UNITS_INVALID) when a pair's
 * square is >= n or not DAGPU_UNITS_OK, or its index is not below n_units and
 * unit_cap.  The summary lives on the device, so such a pair is not refused up
 * front: it yields length 0.  Nothing outside a unit's len bytes is written.
 * d_offsets holds m entries, d_totals 3.  d_workspace:
 * dagpu_square_read_units_workspace_size(m) bytes, 16-B aligned; with it the
 * call is enqueued on `stream` (two launches, no host round trip between the
 * table and the gather) and returns once the pairs have left host memory; with
 * NULL the library allocates it and waits. */
#define DAGPU_UNITS_OK 0
#define DAGPU_UNITS_SCAN 1
#define DAGPU_UNITS_HOST 2
#define DAGPU_UNITS_OVERFLOW 3
#define DAGPU_UNITS_SUMMARY_WORDS 8
#define DAGPU_READ_UNITS_INVALID 2
typedef struct dagpu_unit_record {
  uint32_t start_share, end_share, seq, flags;
  uint64_t offset, len;
} dagpu_unit_record; /* 32 bytes */
size_t dagpu_square_units_workspace_size(uint32_t k, size_t n);
int dagpu_square_units_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares, size_t square_stride,
                              size_t row_pitch, uint32_t seq_cap, const dagpu_seq_record* d_records,
                              const int32_t* d_summary, uint32_t unit_cap, dagpu_unit_record* d_units,
                              int32_t* d_unit_summary, int32_t* unit_summary_out /* HOST, may be NULL */,
                              void* d_workspace, void* stream);
int dagpu_square_units_host(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride, size_t row_pitch,
                            uint32_t seq_cap, const dagpu_seq_record* records, const int32_t* summary,
                            uint32_t unit_cap, dagpu_unit_record* units, int32_t* unit_summary);
int dagpu_square_units_emulate_host(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride,
                                    size_t row_pitch, uint32_t seq_cap, const dagpu_seq_record* records,
                                    const int32_t* summary, uint32_t unit_cap, dagpu_unit_record* units,
                                    int32_t* unit_summary);
size_t dagpu_square_read_units_workspace_size(size_t m);
int dagpu_square_read_units_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares,
                                   size_t square_stride, size_t row_pitch, uint32_t seq_cap,
                                   const dagpu_seq_record* d_records, uint32_t unit_cap,
                                   const dagpu_unit_record* d_units, const int32_t* d_unit_summary,
                                   const uint32_t* pairs /* HOST, 2 per unit */, size_t m, uint64_t* d_offsets,
                                   uint64_t* d_totals, uint8_t* d_payload, size_t payload_cap, void* d_workspace,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
