/*
 * torrent_verify.h -- C ABI of the MI355X piece-verification engine (libtorrent_verify.so).
 *
 * The reference (rclarey/torrent, TypeScript for Deno) has no verify function and no FFI:
 * its only per-piece SHA-1 is `crypto.subtle.digest("SHA-1", content)` inside
 * tools/make_torrent.ts:28-31.  This ABI is what a Deno `Deno.dlopen` binding of the new
 * verify path (ts/verify.ts) binds.  Each entry point names the reference
 * interface whose data it consumes or replaces.
 *
 * Conventions
 *   - Only fixed-width integers and plain pointers cross the boundary.
 *   - Every function returns TV_OK (0) or a negative TV_ERR_*; the message is available from
 *     tv_last_error().  (The TS/Python host turns a negative status into a thrown Error, like
 *     piece.ts:21-65; unreadable data is NOT an error: it yields a 0 bit, like Storage.get
 *     returning null, storage.ts:50-65.)
 *   - One tv_ctx drives one GPU (one process or host thread per GPU).  Calls on one ctx are
 *     serialised by an internal mutex; different ctxs are independent.
 *   - The caller owns every host pointer and keeps it valid for the duration of the call.
 *     The library owns its HIP streams, events, pinned staging buffers and device memory.
 *   - Piece indices are GLOBAL torrent piece indices; a ctx holds the shard
 *     [shard_first, shard_first + shard_count) resident in HBM.
 *   - Bitfields are MSB-first, piece i -> byte i>>3, mask 0x80>>(i&7), spare bits 0
 *     (reference torrent.ts:53,60 and :147-149).
 */
#ifndef TORRENT_VERIFY_H
#define TORRENT_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TV_ABI_VERSION 1

#define TV_OK 0
#define TV_ERR_ARG (-1)     /* invalid argument / geometry */
#define TV_ERR_HIP (-2)     /* HIP runtime failure (message has the hipError string) */
#define TV_ERR_STATE (-3)   /* call out of order (e.g. verify before set_layout) */
#define TV_ERR_NOMEM (-4)   /* device or pinned host allocation failed */
#define TV_ERR_IO (-5)      /* tv_stage_file: file missing, unreadable or shorter than the read
                               (the reference's fsStorage.get -> null, storage.ts:163-171) */

typedef struct tv_ctx tv_ctx;

/* ABI version of the loaded library (== TV_ABI_VERSION). */
int tv_abi_version(void);

/* Number of visible HIP devices. */
int tv_device_count(int *count);

/* Host CPUs this process may use, as the library sees them (no HIP call, no context): the cgroup CPU quota
 * (cpu.max, v2; cpu.cfs_quota_us / cfs_period_us, v1) when one is set, else OMP_NUM_THREADS when set (a stated
 * share), else the affinity mask; never more than the affinity mask, at least 1.  Hosts divide it among the shards
 * of a call (TV_OPT_FILE_THREADS per context), as torrent_amd/_cpu.py cpu_share does. */
int tv_cpu_share(uint32_t *cores);

/* Create a context bound to HIP device `device`. */
int tv_create(tv_ctx **out, int device);

/* Release every resource of the context.  NULL is a no-op. */
void tv_destroy(tv_ctx *ctx);

/* Copy the last error message of `ctx` (or of the calling thread when ctx == NULL) into buf.
 * Returns the full message length. */
int tv_last_error(const tv_ctx *ctx, char *buf, size_t n);

/*
 * Geometry of the torrent and of this ctx's shard; allocates the resident payload.
 *
 * Device budget.  The payload (shard_count padded pieces) is allocated whole when it fits
 * TV_OPT_RESIDENT_BUDGET (default: the GPU's free memory at this call less a margin).  A larger shard gets a
 * WINDOWED layout instead, so no shard fails for its size: the allocation holds two buffers (one when the
 * budget holds only one) of W pieces (TV_COUNTER_WINDOW_PIECES), staging fills window k's buffer, and when
 * staging reaches window k + 1 the library hashes window k (kernels into the shard's digest rows) while k + 1
 * stages into the other buffer.  tv_verify / tv_hash end the pass (the open window is hashed, windows never
 * staged get zero digests: bit 0) and compare / return the whole shard.  Rules of a windowed layout: staging
 * (tv_stage, tv_stage_file, tv_fill_synthetic) must ascend window by window -- bytes of a window already
 * hashed this pass are TV_ERR_STATE; tv_stage_files sorts its segments itself; tv_read reads the open window
 * only; tv_verify_list is TV_ERR_STATE; repeated tv_verify / tv_hash reuse the pass's digests, and staging
 * after them starts a new pass.  TV_COUNTER_PAYLOAD_BYTES <= the budget (unless one piece exceeds it).
 * Slot pool.  With TV_OPT_LIST_SLOTS = K the payload holds K piece slots instead of the shard (incremental
 * verify: only the pieces awaiting verification need device memory).  A piece takes a free slot when its
 * first byte is staged and keeps it until tv_verify_list lists it; staging a piece when all K slots are
 * taken is TV_ERR_STATE.  tv_verify / tv_hash / tv_fill_synthetic are TV_ERR_STATE on a slot pool.
 *
 *   total_length : InfoDict.length (metainfo.ts:21,40 / :125 sum of file lengths)
 *   piece_length : InfoDict.pieceLength (metainfo.ts:14)
 *   n_pieces     : InfoDict.pieces.length, the DIGEST count (metainfo.ts:16,111);
 *                  piece i has length piece.ts:16-19 and linear offset i*piece_length
 *                  (torrent.ts:165,186)
 *   shard_first, shard_count : pieces resident on this device; shard_first % 8 == 0 so the
 *                  bitfield slice is whole bytes; any shard_first when shard_count == 0
 * Device and pinned allocations are kept and reused when the new geometry fits them (a run of
 * single-piece layouts allocates once).
 * Replaces: the per-piece Storage.get(i*pieceLength, pieceLength(i)) walk (storage.ts:50-65).
 */
int tv_set_layout(tv_ctx *ctx, uint64_t total_length, uint64_t piece_length, uint64_t n_pieces,
                  uint64_t shard_first, uint64_t shard_count);

/*
 * Expected digests: the raw `info.pieces` byte string (pieces_len bytes; NOT 20*n_pieces when
 * the string is ragged).  Slice i is bytes [20i, 20i+20) as partition(info.pieces, 20)
 * makes it (metainfo.ts:111, _bytes.ts:92-99); a slice shorter than 20 bytes never matches.
 */
int tv_set_digests(tv_ctx *ctx, const uint8_t *pieces, uint64_t pieces_len);

/*
 * Copy `len` payload bytes at LINEAR torrent offset `linear_offset` (the concatenation of the
 * files in info.files order, storage.ts:89-137) into the resident payload.  Bytes outside the
 * shard are ignored.  The copy goes through the library's pinned staging ring and is complete
 * when the call returns.  Pageable memory is copied into the ring by TV_OPT_FILE_THREADS threads; a
 * page-locked source (tv_host_alloc / tv_host_register) is DMA'd directly.  Replaces: fsStorage.get
 * reads feeding Storage.get (storage.ts:150-172).
 */
int tv_stage(tv_ctx *ctx, uint64_t linear_offset, const uint8_t *src, uint64_t len);

/*
 * n tv_stage calls in one: buffer k (srcs[k], lens[k] bytes) holds LINEAR bytes [linear_offsets[k],
 * linear_offsets[k] + lens[k]).  The same clipping, windows (ascending, as consecutive tv_stage calls) and mark
 * clearing apply, in order k = 0 .. n-1; every copy is complete when the call returns.  For a host that holds a
 * batch of pieces as separate buffers (one Storage.get result per piece, storage.ts:50-65): the library packs
 * the buffers shorter than 16 MiB into its pinned ring slots (many per slot) on its own threads, one DMA per
 * run of adjacent bytes, on both staging lanes when they fill two slots of a whole-shard layout, so the caller
 * does no gather copy.  Replaces: a batch of Storage.get results (storage.ts:50-65), one per piece, as
 * verifyPieces collects them; or a multi-file payload's files (10,000 of them stage at ~51 GB/s).
 */
int tv_stage_many(tv_ctx *ctx, uint64_t n, const uint64_t *linear_offsets, const uint8_t *const *srcs,
                  const uint64_t *lens);

/*
 * Stage `len` bytes of the file at `path` (a NUL-terminated path), starting at byte `file_offset`,
 * as LINEAR torrent bytes [linear_offset, linear_offset + len).  This is one file segment of
 * Storage.get's mapping (storage.ts:89-137: path, offset in the file, length) read the way
 * fsStorage.get reads it (storage.ts:150-172: open, seek, read).  The bytes are read by parallel preads
 * (TV_OPT_FILE_THREADS threads, 1-4 MiB requests) into the library's pinned ring, one 64 MiB slot at a time,
 * and DMA'd from the slot to HBM while the next slot is read (53 GB/s end to end from a warm page cache on
 * an MI355X host whose PCIe H2D copy runs at 57.6; profiles/r05).  A part whose bytes are mostly not in the
 * page cache is read with O_DIRECT (faster than buffered reads at disk rates; a filesystem that refuses it
 * is read buffered).  Bytes outside the shard are skipped.  A missing, unopenable or short file (or a read error
 * part-way) returns TV_ERR_IO, and the library marks the pieces Storage.get would return null for
 * (storage.ts:50-65 reads piece by piece): from the piece holding the first byte the file cannot supply
 * to the segment's end.  The whole pieces before that byte are staged and stay readable.  Marked pieces
 * are reported 0 by tv_verify and tv_verify_list until the next tv_set_layout; the host marks nothing.  Unlike
 * fsStorage.get (which opens with create: true, storage.ts:28-32,158) a missing file is never created.
 * The file is opened as fsStorage.get opens it (read + write, storage.ts:28-32,158): a file this process
 * may not write returns TV_ERR_IO, as Deno.open fails there.  len == 0 reads nothing but still checks the
 * open: TV_ERR_IO when fsStorage.get's open would fail (a directory, a missing parent directory, no
 * permission); a missing file in a writable directory succeeds (fsStorage.get would create it; this call
 * creates nothing).
 */
int tv_stage_file(tv_ctx *ctx, const char *path, uint64_t file_offset, uint64_t linear_offset, uint64_t len);

/*
 * Stage MANY file segments in one call: a shard's whole Storage.get mapping (storage.ts:89-137), each
 * segment read as fsStorage.get reads it (storage.ts:150-172).  Segment k is `lens[k]` bytes of file
 * `paths[k]` from byte `file_offsets[k]`, staged as LINEAR bytes [linear_offsets[k], +lens[k]).
 *   - Segments of >= TV_OPT_FILE_DIRECT_MIN bytes (default 32 MiB) take the tv_stage_file path, cut into
 *     256 MiB units dealt to two staging lanes (a helper thread with its own copy stream and pinned ring,
 *     and the calling thread; the TV_OPT_FILE_THREADS readers shared between them), which DMA side by side.
 *   - Shorter ones are packed into the pinned ring's 64 MiB slots. TV_OPT_FILE_THREADS threads read
 *     them (open, pread, close; default 16), and each run of linear-contiguous segments is one DMA.
 *     A slot's DMA overlaps the reads of the next slot. This is the many-small-files case: a
 *     10,000-file torrent is one call, not 10,000.
 * status_out[k] = TV_OK, or TV_ERR_IO when the file is missing, unreadable, not writable or shorter than
 * the segment.  As for tv_stage_file, the library itself marks the pieces Storage.get would return null
 * for (from the piece holding the first unreadable byte to the segment's end; the whole pieces before it
 * are staged), tv_verify reports them 0 until the next tv_set_layout, and the status is informational: a
 * host that cleared every piece a failed segment touches would lose a short file's readable pieces.
 *   - Zero-length segments belong in the list: Storage.get's walk emits them for a file that ends where a
 *     piece starts and for a zero-length file inside a piece (storage.ts:109-110), and fsStorage.get still
 *     opens them (storage.ts:158).  Such a segment reads nothing; its status is TV_ERR_IO exactly when that
 *     open would fail (tv_stage_file, len == 0), and nothing is created.  Its piece, linear_offsets[k] /
 *     piece_length, is then marked unreadable.
 * The call itself returns TV_OK unless an argument or HIP error occurs; the first I/O failure's message is
 * kept for tv_last_error.  Bytes outside the shard are skipped.
 */
int tv_stage_files(tv_ctx *ctx, uint64_t n, const char *const *paths, const uint64_t *file_offsets,
                   const uint64_t *linear_offsets, const uint64_t *lens, int32_t *status_out);

/*
 * Stage the shard's bytes from the torrent's FILE TABLE in one call: the library makes Storage.get's walk
 * (storage.ts:89-137) itself.  File k holds `lengths[k]` bytes and is found at the k-th of the n NUL-terminated
 * paths packed back to back in `paths` (`paths_bytes` bytes in all): [dir, ...info.files[k].path] joined, or
 * [dir, info.name] for a single-file torrent (n = 1).  Files are in info.files order, so file k starts at the sum
 * of the lengths before it.  Every segment of the walk that meets the shard is staged as tv_stage_files stages
 * it, the zero-length segments fsStorage.get still opens included (storage.ts:109-110,158).  status_out[k] (n
 * entries, one per FILE) = TV_ERR_IO when a segment of file k failed, else TV_OK; as for tv_stage_files the
 * library marks the unreadable pieces itself and the status is informational.  A host thus passes its file table
 * (which it may keep across calls) and does no per-file work per call.  TV_ERR_ARG when `paths` holds fewer than
 * n NUL-terminated paths or the lengths overflow 64-bit offsets.
 */
int tv_stage_file_table(tv_ctx *ctx, uint64_t n, const uint64_t *lengths, const char *paths, uint64_t paths_bytes,
                        int32_t *status_out);

/* The inverse of tv_stage: copy `len` resident bytes at LINEAR offset `linear_offset` to host
 * `dst` (HBM as the piece store serving block requests, torrent.ts:164-167 Storage.get).  Bytes
 * outside the shard are left untouched in dst. */
int tv_read(tv_ctx *ctx, uint64_t linear_offset, uint8_t *dst, uint64_t len);

/* Fill the resident shard with the synthetic payload of `seed` (benchmarks / GPU tests):
 * byte at linear offset o = byte (o & 7) of splitmix64(seed, o >> 3), little-endian. */
int tv_fill_synthetic(tv_ctx *ctx, uint64_t seed);

/*
 * Verify every resident piece of the shard (HBM-resident path).
 *   avail_bits : optional (NULL = all readable) shard-relative MSB-first bitfield, ceil(shard_count/8)
 *                bytes; a clear bit forces 0 (Storage.get -> null: missing / short file).
 *   bitfield_out : ceil(shard_count/8) bytes, shard-relative; bit j = piece shard_first + j.
 * Piece i's bit is 1 iff its bytes are readable AND SHA-1(bytes) == info.pieces[i].
 */
int tv_verify(tv_ctx *ctx, const uint8_t *avail_bits, uint8_t *bitfield_out);

/*
 * Verify a LIST of resident pieces (incremental verify on piece completion, SURVEY 8f row f1: the
 * piece-message handler torrent.ts:183-193 is where a completed piece is checked).  pieces[k] are
 * GLOBAL piece indices inside this ctx's shard (any order, duplicates allowed); ok_out[k] = 1 iff
 * SHA-1 of the resident bytes of piece pieces[k] equals info.pieces[pieces[k]], else 0.  Only pieces
 * whose bytes were staged should be listed.  On a slot pool (TV_OPT_LIST_SLOTS) a listed piece without a
 * slot (never staged) is 0, and every listed piece's slot is free again when the call returns.
 * TV_ERR_STATE on a windowed layout.
 */
int tv_verify_list(tv_ctx *ctx, const uint64_t *pieces, uint64_t n, uint8_t *ok_out);

/*
 * Verify the shard from a HOST buffer (end-to-end resume check): `src` holds the
 * shard's linear bytes [shard_first*piece_length, ...) (src_len bytes; pieces extending past
 * src_len are unreadable).  Data streams host -> pinned ring -> HBM over PCIe with copy/compute
 * overlap; no resident payload is needed (set the layout with TV_OPT_RESIDENT = 0).  Device memory: two chunk
 * buffers within TV_OPT_RESIDENT_BUDGET (default 1 GiB), each a column of a window of >= 2,048 pieces, at most
 * 256 MiB; TV_OPT_STREAM_CHUNK instead gives columns of that width across the whole shard.
 */
int tv_verify_host(tv_ctx *ctx, const uint8_t *src, uint64_t src_len, const uint8_t *avail_bits,
                   uint8_t *bitfield_out);

/*
 * The resume check from the torrent's FILES through the bounded ring (SURVEY 8f row f2 under a small device
 * budget): the stream engine of tv_stream_*, with the library's own readers filling each request's rows straight
 * from the files (the file table as for tv_stage_file_table: n files of lengths[k] bytes, paths NUL-separated in
 * `paths`).  Each row's linear bytes are walked over the files as Storage.get walks them (storage.ts:98-137) and
 * read as fsStorage.get reads them; a piece is 0 exactly when fsStorage.get would return null for it (a byte in a
 * missing, unopenable or short file, a zero-length segment whose open fails, bytes past the files' end) or its
 * SHA-1 differs.  The layout is set with TV_OPT_RESIDENT = 0; device memory: two chunk buffers within
 * TV_OPT_RESIDENT_BUDGET (default 1 GiB), each a column -- a byte range of every piece of a window of >= 2,048 pieces,
 * as wide as the budget allows -- so each row is one long read and every window's SHA-1s advance with each column;
 * a shard far larger than the budget verifies at the staging rate (an explicit TV_OPT_STREAM_CHUNK instead gives
 * columns of that width across the whole shard).  Host memory: the 192 MiB ring.  status_out[k]
 * (n entries) = TV_ERR_IO when a read or open of file k failed.  Nothing is created.
 */
int tv_stream_file_table(tv_ctx *ctx, uint64_t n, const uint64_t *lengths, const char *paths, uint64_t paths_bytes,
                         const uint8_t *avail_bits, uint8_t *bitfield_out, int32_t *status_out);

/* Creation mode (make_torrent.ts:28-31, :147-173): 20-byte SHA-1 of every resident piece of the
 * shard, written to digests_out (20*shard_count bytes), in piece order. */
int tv_hash(tv_ctx *ctx, uint8_t *digests_out);

/*
 * A BATCH LAYOUT: many v1 torrents of any piece lengths resident at once, verified by ONE kernel launch.  The
 * interface it serves is the client's torrent map (client.ts: `torrents: Map<string, Torrent>`): when a client
 * starts, every torrent it holds is re-checked, and SHA-1 is serial inside a piece, so a launch per torrent costs at
 * least one piece's serial hash each while filling a sliver of the GPU.
 *
 * Torrent t has the geometry tv_set_layout(total_length[t], piece_length[t], n_pieces[t], 0, n_pieces[t]) would give
 * it (n_pieces[t] digests, which may differ from ceil(total / L); piece lengths per piece.ts:16-19; 0 pieces allowed).
 * The payload is one device allocation, a region per torrent laid out as a resident layout's rows (stride =
 * round_up(L, 64) + TV_OPT_STRIDE_PAD), every region 256-byte aligned, the usual slack after the last.  There are no
 * windows and no slot pool: a batch beyond TV_OPT_RESIDENT_BUDGET (or the automatic budget) is TV_ERR_NOMEM (the
 * message names the bytes and the budget; the context stays usable), TV_OPT_LIST_SLOTS set or TV_OPT_RESIDENT = 0 is
 * TV_ERR_STATE.  TV_ERR_ARG (naming the torrent): a geometry tv_set_layout would refuse, 2^32 - 1 pieces or more in
 * all.  Allocations are reused as tv_set_layout reuses them.  Torrent 0 is selected on return; tv_set_layout ends
 * the batch.
 */
int tv_set_batch_layout(tv_ctx *ctx, uint64_t n_torrents, const uint64_t *total_length,
                        const uint64_t *piece_length, const uint64_t *n_pieces);

/*
 * Select torrent t of the batch (one entry of client.ts's torrent map): tv_set_digests, tv_stage, tv_stage_many,
 * tv_stage_file, tv_stage_files, tv_stage_file_table, tv_read and tv_fill_synthetic then work on it unchanged,
 * linear_offset meaning ITS linear space.  A torrent's ragged-digest bits, the unreadable marks file staging left
 * and whether its digests were set survive selecting another torrent and coming back.  TV_ERR_ARG: t >= n_torrents;
 * TV_ERR_STATE: no batch layout.
 */
int tv_batch_select(tv_ctx *ctx, uint64_t torrent);

/*
 * Verify every piece of every torrent of the batch (the start-up re-check of client.ts's torrent map) in ONE
 * launch.  bitfield_out: the per-torrent MSB-first bitfields back to back, torrent t's starting at byte
 * sum over u < t of ceil(n_pieces[u] / 8); avail_bits (optional, NULL = all readable): the same shape.  A piece's bit
 * is 1 iff it is available, not marked unreadable by file staging, its digest slice is 20 bytes long and SHA-1 of its
 * resident bytes equals the slice.  TV_ERR_STATE (naming the torrent) when a torrent's digests were never set.
 * tv_last_timing, tv_last_kernel (the form that ran, 1 launch) and TV_COUNTER_LAST_WORKGROUPS report it.
 * While a batch layout is set, every other verifying or hashing call (tv_verify, tv_hash, tv_verify_list,
 * tv_verify_host, tv_stream_*, tv_v2_*, tv_hybrid_*) is TV_ERR_STATE.
 */
int tv_batch_verify(tv_ctx *ctx, const uint8_t *avail_bits, uint8_t *bitfield_out);

/*
 * BitTorrent v2 (BEP 52) pieces: SHA-256 merkle roots over 16 KiB blocks.  The reference knows v1 torrents only
 * (metainfo.ts:12-44 has no `file tree`); these calls verify and create the format current clients write by default.
 *
 * In a v2 torrent every file starts a new piece, so the layout set by tv_set_layout is the ALIGNED linear space:
 * piece p at linear offset p * piece_length, pieces numbered in file-tree order as if pad files aligned every file
 * (a zero-length file has no piece).  tv_stage*, tv_read and tv_fill_synthetic work on that space unchanged; the
 * host stages each file at its aligned offset.  piece_length must be a power of two >= TV_V2_LEAF_BYTES.
 *
 * tv_v2_set_pieces gives the piece table of the layout: n == the layout's n_pieces entries, GLOBAL (the ctx takes
 * its shard from them, as tv_set_digests does).
 *   piece_bytes[p] : valid bytes of piece p, 1 .. piece_length (a file's last piece may be short; bytes past it are
 *                    never read into a hash)
 *   tree_leaves[p] : width of piece p's merkle tree in leaves: a power of two >= ceil(piece_bytes[p] / 16 KiB) and
 *                    <= piece_length / 16 KiB.  A piece of a file longer than one piece has the full width
 *                    (its `piece layers` entry is the root of a whole piece subtree, the missing leaves zero hashes);
 *                    a file of <= piece_length bytes is one piece whose tree is only as wide as its leaves need, and
 *                    whose root is the file's `pieces root`.  The width cannot be derived from the length: the host
 *                    passes it.
 *   hashes         : 32 * n bytes, the expected root of every piece (`piece layers` entries, or `pieces root` for a
 *                    one-piece file); NULL = creation mode (tv_v2_hash only).
 * A leaf (16 KiB block, the last of a file 1 .. 16,384 bytes, not padded) hashes to SHA-256 of its bytes; a leaf
 * position past the piece's bytes is 32 zero bytes; an interior node is SHA-256(left || right).
 * TV_ERR_ARG: piece_length not a power of two or < 16 KiB, n != n_pieces, a piece_bytes / tree_leaves entry outside
 * the ranges above.  TV_ERR_STATE: before tv_set_layout, on a windowed layout or a slot pool (v2 needs the shard
 * resident), during a stream; tv_v2_verify / tv_v2_hash without a piece table (tv_v2_verify: without hashes).
 * tv_set_layout drops the table.
 *
 * tv_v2_verify: as tv_verify -- bit j = piece shard_first + j is readable (avail_bits, and not marked unreadable by
 * tv_stage_file(s)) AND its merkle root equals hashes[32 j'..], j' its global index.  tv_v2_hash: the 32-byte root of
 * every resident piece, in piece order (creation mode: a file's `piece layers` entry, or its `pieces root` when it
 * is one piece; the host reduces a longer file's layer to its `pieces root`).  tv_last_timing, tv_last_kernel
 * (kernel id 8) and TV_COUNTER_LAST_WORKGROUPS (the leaf kernel's grid) report on them.
 *
 * tv_v2_verify_list: a LIST of v2 pieces in ONE launch (incremental verify on piece completion, as tv_verify_list
 * for v1).  The entries describe themselves, so no tv_v2_set_pieces and no tv_set_digests is needed, and an
 * incremental host hands over only what its pending pieces need: entry k is GLOBAL piece pieces[k] of this ctx's
 * shard (any order, duplicates allowed) with piece_bytes[k] valid bytes, a tree of tree_leaves[k] leaves (the ranges
 * of tv_v2_set_pieces) and the expected root hashes[32 k ..]; ok_out[k] = 1 iff the merkle root of the piece's
 * resident bytes equals it.  On a whole-shard resident layout the piece's row is read; on a slot pool
 * (TV_OPT_LIST_SLOTS) its slot, with tv_verify_list's rules: a listed piece without a slot (never staged) is 0, and
 * every listed piece's slot is free again when the call returns.  Bytes past piece_bytes[k] in a row or slot (a
 * previous occupant's) are never read into a hash.  Pieces marked unreadable by tv_stage_file(s) are 0.  n == 0 is
 * TV_OK.  Each piece's tree is reduced inside one workgroup (leaf hashes and levels in on-chip memory), so the call
 * holds no node buffers: device memory is 48 bytes per listed entry (at least 1,024 entries), reused by later calls
 * of the same or a smaller n.  Piece lengths up to 1 GiB (65,536 leaves).
 * TV_ERR_ARG: NULL arguments with n > 0, a piece outside the shard, piece_length not a power of two >= 16 KiB or
 * > 1 GiB, a piece_bytes / tree_leaves entry outside the ranges above.  TV_ERR_STATE: before tv_set_layout, on a
 * windowed layout, with TV_OPT_RESIDENT = 0, during a stream.  A refused call frees no slot.  tv_last_timing,
 * tv_last_kernel (kernel id 16, one launch) and TV_COUNTER_LAST_WORKGROUPS report on it.
 */
#define TV_V2_LEAF_BYTES 16384
int tv_v2_set_pieces(tv_ctx *ctx, uint64_t n, const uint32_t *piece_bytes, const uint32_t *tree_leaves,
                     const uint8_t *hashes);
int tv_v2_verify(tv_ctx *ctx, const uint8_t *avail_bits, uint8_t *bitfield_out);
int tv_v2_hash(tv_ctx *ctx, uint8_t *roots_out);
int tv_v2_verify_list(tv_ctx *ctx, uint64_t n, const uint64_t *pieces, const uint32_t *piece_bytes,
                      const uint32_t *tree_leaves, const uint8_t *hashes /* 32*n */, uint8_t *ok_out);

/*
 * Below the piece: the leaf layer of a v2 piece, and single 16 KiB blocks against it.  A v2 piece hash is the root of
 * a merkle tree so that a block can be checked on its own: a downloader that has a piece's leaf layer (obtained from
 * a peer and proven against the piece's hash, a `hashes` message) can name the bad blocks of a failed piece and fetch
 * only those again, and check a block before its piece is complete; a seeder answers a hash request from the leaf
 * layer of a piece it holds.  The tree above the leaves (proofs, uncle hashes) is a few hundred small hashes: host
 * work, not in this library.
 *
 * Both calls take entries that describe themselves exactly as tv_v2_verify_list's do: entry k is GLOBAL piece
 * pieces[k] of this ctx's shard (any order, duplicates allowed) with piece_bytes[k] valid bytes and a tree of
 * tree_leaves[k] leaves (the ranges and error texts of tv_v2_set_pieces); no piece table and no digests are needed; on
 * a whole-shard resident layout the piece's row is read, on a slot pool (TV_OPT_LIST_SLOTS) its slot.  With
 * W = piece_length / 16 KiB, block i of a piece is its bytes [16384 i, min(16384 (i + 1), piece_bytes[k])): it holds
 * bytes when 16384 i < piece_bytes[k], and its hash is SHA-256 of those bytes (the last one 1 .. 16,384, not padded).
 * Any valid v2 piece length is accepted (no tree is held in on-chip memory, so tv_v2_verify_list's 1 GiB limit does
 * not apply).
 *
 * tv_v2_leaf_hashes: leaves_out gets 32 * n * W bytes: entry k's block i at leaves_out + (k * W + i) * 32; the
 * positions at or past ceil(piece_bytes[k] / 16 KiB), out to W, are 32 zero bytes (BEP 52's zero hashes of the padding
 * leaves inside the tree, and the positions beyond a narrower tree alike).  A listed piece that holds no slot, or that
 * tv_stage_file(s) marked unreadable, is TV_ERR_STATE naming the piece (there is nothing to hand out).
 *
 * tv_v2_check_blocks: leaf_hashes has the layout of leaves_out (32 * n * W bytes; only wanted positions are read).
 * want_bits: n rows of ceil(W / 8) bytes, MSB-first, bit i of row k = block i of entry k is wanted; NULL = every block
 * that holds bytes.  ok_bits_out has the same shape: bit i of row k is 1 iff block i is wanted, holds at least one
 * valid byte, and SHA-256 of its valid bytes equals leaf_hashes[(k * W + i) * 32 ..]; spare bits are 0.  A block that
 * is not wanted is neither read nor hashed, so a partly received piece can sit in a slot with stale bytes around its
 * staged blocks.  A piece without a slot, or marked unreadable, gives all 0 bits (tv_verify_list's rule).
 *
 * release != 0 frees the listed pieces' slots when the call returns, as tv_v2_verify_list does; release == 0 keeps
 * them (the piece may still be assembling).  A refused call changes nothing and frees no slot.  n == 0 is TV_OK.
 * TV_ERR_ARG: NULL arrays with n > 0 (want_bits may be NULL), a piece outside the shard, piece_length not a power of
 * two >= 16 KiB, a piece_bytes / tree_leaves entry outside its range, more than TV_V2_BLOCKS_MAX blocks to hash, and
 * for tv_v2_leaf_hashes also n * W > TV_V2_BLOCKS_MAX.  TV_ERR_STATE: before tv_set_layout, on a windowed layout, with
 * TV_OPT_RESIDENT = 0, during a stream.  Each call is ONE launch, one lane per block to hash; device memory is at most
 * 48 bytes per such block (at least 1,024 of them), reused by later calls that fit.  tv_last_timing, tv_last_kernel
 * (kernel id 64, one launch) and TV_COUNTER_LAST_WORKGROUPS (ceil(blocks / 256)) report on it.
 */
#define TV_V2_BLOCKS_MAX (1ull << 22)
int tv_v2_leaf_hashes(tv_ctx *ctx, uint64_t n, const uint64_t *pieces, const uint32_t *piece_bytes,
                      const uint32_t *tree_leaves, uint8_t *leaves_out, int release);
int tv_v2_check_blocks(tv_ctx *ctx, uint64_t n, const uint64_t *pieces, const uint32_t *piece_bytes,
                       const uint32_t *tree_leaves, const uint8_t *leaf_hashes, const uint8_t *want_bits,
                       uint8_t *ok_bits_out, int release);

/*
 * Hybrid torrents: one info dict with both descriptions of one payload (BEP 52's upgrade path; what current clients
 * write by default): the v1 `files` / `pieces` with BEP 47 pad files (`attr` containing `p`) after every file that
 * does not end a piece, and the v2 `file tree` / `piece layers`.  A client must check BOTH hash sets: a torrent whose
 * two descriptions disagree can feed different payloads to v1 and v2 peers, and BEP 52 tells clients to refuse it.  The
 * reference knows neither pad files nor v2 (metainfo.ts:12-44).
 *
 * With the pads every file starts a piece, so the v1 linear space IS the aligned space of the v2 calls: one
 * tv_set_layout (total_length = the v1 length, pads included), one staging of each file at its aligned offset, then
 * tv_v2_set_pieces (the v2 piece table; with hashes for a verify) and, for a verify, tv_set_digests (the v1 `pieces`
 * string).  v1 piece i is the piece_bytes[i] file bytes of v2 piece i followed by the pad file's zeros out to
 * v1_len(i) = min(piece_length, total_length - i * piece_length): every piece has v1_len = piece_length except
 * possibly the last.  Pad ranges are DEFINED as zeros, as clients treat pad files: both calls first zero
 * [piece_bytes[i], v1_len(i)) of every resident row that has such a range (one kernel launch over the shard's tail
 * pieces, at most one per file; none when no piece has one), whatever was staged there, so a host never stages, reads
 * or looks for a pad file, and tv_read returns zeros there afterwards.  Then the SHA-1 launch of tv_verify / tv_hash
 * and the launches of tv_v2_verify / tv_v2_hash run over the same resident bytes.
 *
 * tv_hybrid_verify: bit j of v1_bits_out = piece shard_first + j is readable (avail_bits, and not marked unreadable by
 * tv_stage_file(s)) AND SHA-1 of its v1_len bytes equals its `pieces` slice, as tv_verify; of v2_bits_out = readable
 * AND its merkle root equals its hash, as tv_v2_verify; bitfield_out = v1 AND v2.  v1_bits_out and v2_bits_out may be
 * NULL; a host that passes them can name the pieces where the descriptions disagree (v1 != v2).  All three are
 * ceil(shard_count / 8) bytes, spare bits 0.
 * tv_hybrid_hash (creation mode): the 20-byte SHA-1 of every resident v1 piece (pad zeros included) and the 32-byte
 * merkle root of every resident v2 piece, in piece order, from one staging.
 * TV_ERR_STATE: before tv_set_layout, on a windowed layout or a slot pool, with TV_OPT_RESIDENT = 0, during a stream,
 * without a piece table; tv_hybrid_verify without digests or without v2 hashes.  TV_ERR_ARG: NULL outputs with a
 * non-empty shard (bitfield_out; digests_out or roots_out), a piece_bytes[i] > v1_len(i) (the layout is not the v1
 * space of the table), piece_length > 2 GiB.  A refused call changes nothing.  shard_count == 0 is TV_OK.
 * tv_last_kernel reports kernel id 128 and the launches used (the pad launch when there is one, the SHA-1 launch, the
 * v2 launches); tv_last_timing's kernel_ms spans from the pad kernel's start to the last hash kernel's end.  Device
 * memory beyond the layout's and the piece table's: 16 bytes per tail piece (at least 1,024 of them) and, for a verify,
 * a second bitfield and availability (2 x 8 bytes per 64 pieces), allocated by the first call that needs them, counted
 * in TV_COUNTER_DEVICE_BYTES / _ALLOCS and reused by later calls they fit.  tv_verify, tv_hash and the tv_v2_* calls on
 * the same ctx keep their own answers (tv_verify then hashes the zeroed pads, as a v1 client reading pad files would).
 * A shard that does not fit the device budget streams instead (tv_hybrid_stream_begin, below).
 *
 * tv_hybrid_verify_list: a LIST of completed pieces of a hybrid torrent, both hashes from one staging (incremental
 * verify on piece completion, SURVEY 8f row f1, as tv_verify_list for v1 and tv_v2_verify_list for v2).  The layout is
 * the v1 space (total_length with the pads) and tv_set_digests holds the v1 `pieces` string; the entries describe their
 * v2 side themselves exactly as tv_v2_verify_list's do (no tv_v2_set_pieces is needed; a table that has been set is
 * left alone).  On a whole-shard resident layout the piece's row is read, on a slot pool (TV_OPT_LIST_SLOTS) its slot.
 * Entry k is GLOBAL piece pieces[k] (any order, duplicates allowed) with v1_len = min(piece_length, total_length -
 * pieces[k] * piece_length).  The call first DEFINES the bytes [piece_bytes[k], v1_len) of the entry's row or slot as
 * zeros, whatever a previous occupant or a fill left there (a host never stages a pad).  v1_ok_out[k] = 1 iff SHA-1 of
 * the v1_len bytes equals the piece's `pieces` slice (a ragged or short slice never matches, as tv_verify_list);
 * v2_ok_out[k] = 1 iff the merkle root of the first piece_bytes[k] bytes under a tree of tree_leaves[k] leaves equals
 * hashes[32 k ..]; ok_out[k] = v1 AND v2.  v1_ok_out and v2_ok_out may be NULL.  A listed piece without a slot (never
 * staged), or marked unreadable by tv_stage_file(s), is 0 in all three.  release != 0 frees every listed piece's slot
 * when the call returns, as the other list calls do; release == 0 keeps them (the host may follow a failed piece with
 * tv_v2_check_blocks; tv_read then shows the zeros).  A refused call changes nothing: it stores no zero and frees no
 * slot.  n == 0 is TV_OK.
 * TV_ERR_STATE, in this order: before tv_set_layout, before tv_set_digests, on a windowed layout, with TV_OPT_RESIDENT
 * = 0, during a stream.  TV_ERR_ARG: NULL pieces, piece_bytes, tree_leaves, hashes or ok_out with n > 0, a piece
 * outside the shard, piece_length not a power of two >= 16 KiB or > 1 GiB (the v2 list kernel's limit), a piece_bytes /
 * tree_leaves entry outside tv_v2_set_pieces' ranges (its texts), a piece_bytes[k] > v1_len (tv_hybrid_verify's text).
 * Every launch goes onto the compute stream before the call's one wait: the list pad launch (one launch over entries x
 * chunks, each entry's range derived on the device from its row, its piece_bytes and its piece with the layout; only
 * when some launched entry has a pad range), the SHA-1 list launch (tv_verify_list's kernel choice and launch order),
 * the v2 list launch.  tv_last_kernel reports kernel id 512 and 2 launches, 3 with the pad launch, 0 when no listed
 * piece held a slot; tv_last_timing's kernel_ms spans from the first launch's start to the last one's end;
 * TV_COUNTER_LAST_WORKGROUPS is the v2 list launch's grid.  Device memory beyond the two list calls' buffers: 8 bytes
 * per listed entry (at least 1,024 entries), counted in TV_COUNTER_DEVICE_BYTES / _ALLOCS and reused by later calls
 * that fit.
 */
int tv_hybrid_verify(tv_ctx *ctx, const uint8_t *avail_bits, uint8_t *v1_bits_out, uint8_t *v2_bits_out,
                     uint8_t *bitfield_out);
int tv_hybrid_hash(tv_ctx *ctx, uint8_t *digests_out /* 20*shard_count */, uint8_t *roots_out /* 32*shard_count */);
int tv_hybrid_verify_list(tv_ctx *ctx, uint64_t n, const uint64_t *pieces, const uint32_t *piece_bytes,
                          const uint32_t *tree_leaves, const uint8_t *hashes /* 32*n */, uint8_t *v1_ok_out,
                          uint8_t *v2_ok_out, uint8_t *ok_out, int release);

/*
 * Streamed verify through a BOUNDED pinned ring (end-to-end resume check, SURVEY 8d cfg5: the
 * resume flow Client.add -> Storage -> bitfield -> sendBitfield, client.ts:53-67, torrent.ts:56-60,101).
 * No resident payload and no whole-shard host buffer are needed: the library hands out requests in the
 * order its kernels consume them, the caller (a Storage.get reader, a file reader, a generator) fills
 * each request's pinned staging slot, and the library DMAs it to HBM over PCIe while the kernels hash the
 * previous column.  Host memory in flight is the ring (TV_STREAM_RING_SLOTS x TV_STREAM_SLOT_BYTES).
 *
 *   tv_stream_begin(ctx, avail)          avail: optional shard-relative MSB-first bits (NULL = all)
 *   loop: tv_stream_next(ctx, &req)      req.rows == 0 -> every byte has been requested
 *         fill req.slot (row q at req.slot + q*req.width) and tv_stream_commit(ctx, &req),
 *         or tv_stream_commit_from(ctx, &req, src, src_pitch) to copy the rows from caller memory
 *   tv_stream_end(ctx, bitfield_out)     ceil(shard_count/8) bytes, as tv_verify
 *
 * A request covers `rows` consecutive pieces starting at GLOBAL piece `piece`, and bytes
 * [offset, offset + width) of each (piece-relative; every request of one column has the same offset; with
 * TV_OPT_STREAM_ROWS the offset is 0 and the width the piece length).
 * Row q holds the LINEAR bytes [(piece+q)*piece_length + offset, ...) of length
 * row_bytes(q) = min(width, piece_len(piece+q) - offset), which is `width` for every row except
 * the short last piece's (0 past its end; piece.ts:16-19).  One request is outstanding at a time.  A piece whose bytes cannot be read
 * (Storage.get -> null, storage.ts:50-65) is reported with tv_stream_unreadable and gets bit 0.
 * Calls that use the resident payload fail with TV_ERR_STATE while a stream is active;
 * tv_set_layout / tv_set_digests / tv_stream_abort end it.  Replaces: the per-piece
 * Storage.get + digest loop (storage.ts:50-65, make_torrent.ts:28-31) of a resume check.
 */
#define TV_STREAM_RING_SLOTS 3
#define TV_STREAM_SLOT_BYTES (64ull << 20)
typedef struct tv_stream_req {
    uint64_t piece;   /* GLOBAL index of row 0's piece */
    uint64_t rows;    /* pieces in this request; 0 = the stream is complete */
    uint64_t offset;  /* byte offset inside each piece (the column) */
    uint64_t width;   /* row pitch in `slot`; row q holds tv_row_bytes(q) <= width valid bytes */
    uint8_t *slot;    /* library-owned page-locked staging memory, rows * width bytes */
    uint64_t seq;     /* request number (tv_stream_commit checks it) */
} tv_stream_req;
int tv_stream_begin(tv_ctx *ctx, const uint8_t *avail_bits);
int tv_stream_next(tv_ctx *ctx, tv_stream_req *req);
int tv_stream_commit(tv_ctx *ctx, const tv_stream_req *req);
/* Rows from caller memory: row q at src + q*src_pitch (row_bytes(q) bytes).  A page-locked src
 * (tv_host_alloc / tv_host_register) is DMA'd directly and must stay unmodified until tv_stream_end /
 * tv_stream_abort returns; pageable memory is copied into the request's slot before the call returns. */
int tv_stream_commit_from(tv_ctx *ctx, const tv_stream_req *req, const uint8_t *src, uint64_t src_pitch);
/* Piece `piece` (GLOBAL, inside the shard) is unreadable: its bit will be 0. */
int tv_stream_unreadable(tv_ctx *ctx, uint64_t piece);
int tv_stream_end(tv_ctx *ctx, uint8_t *bitfield_out);
/* Drop an active stream (a reader failed part-way); the ctx is usable again.  No-op when idle. */
int tv_stream_abort(tv_ctx *ctx);
/* Benchmarks / tests: fill the outstanding request's slot with the synthetic payload of `seed` (the
 * bytes tv_fill_synthetic writes), generated on the host by TV_OPT_FILE_THREADS threads. */
int tv_stream_fill_synthetic(tv_ctx *ctx, const tv_stream_req *req, uint64_t seed);

/*
 * Streamed BitTorrent v2 verify through the same bounded ring: a v2 torrent larger than the device budget, or on a
 * GPU shared with other work, checked without a resident shard.
 *
 * tv_v2_stream_begin starts a stream whose units are hashed as v2 pieces.  It carries the piece table itself (as
 * tv_v2_verify_list's entries do): n == the layout's n_pieces GLOBAL entries with tv_v2_set_pieces' ranges and error
 * texts, `hashes` required (32 * n bytes); the ctx copies its shard's part, so the arrays are the caller's again when
 * the call returns.  It needs a layout (the ALIGNED linear space, as for the other v2 calls), but neither
 * tv_set_digests nor tv_v2_set_pieces, works with TV_OPT_RESIDENT 0 or 1, and leaves a table set with
 * tv_v2_set_pieces alone.  After it tv_stream_next / _commit / _commit_from / _unreadable / _fill_synthetic / _end /
 * _abort work as after tv_stream_begin, with one difference in the requests: row q holds
 * min(width, piece_bytes[piece + q] - offset) valid bytes, 0 when that piece ends before the column (every file ends
 * a piece, so any row may be short; a row of 0 bytes is neither filled nor copied).
 *
 * Geometry: a column is C bytes of every piece of a window of wn pieces; C is a power of two, 16 KiB <= C <=
 * min(piece_length, 64 MiB), wn a multiple of 64 or the whole shard.  TV_OPT_STREAM_CHUNK = X > 0: C = the largest
 * power of two <= min(max(X, 16 KiB), min(piece_length, 64 MiB)), one window across the shard.  Otherwise, under
 * TV_OPT_RESIDENT_BUDGET (1 GiB when unset) for the two chunk buffers: whole pieces (C = min(piece_length, 64 MiB))
 * when 64 of them fit, else C halved until 64 rows fit; then as many pieces per window as fit.  TV_OPT_STREAM_ROWS has
 * no effect.  A column of a piece is a whole aligned subtree of its merkle tree, so one kernel launch per column
 * reduces it to one node per piece and nothing is carried from column to column; a window's last column is followed by
 * log2(piece_length / C) level launches and one finish launch.  Device memory beyond the two chunk buffers: 44 bytes
 * per shard piece and at most 48 bytes x wn x (piece_length / C) of nodes, reused by a later stream they fit
 * (TV_COUNTER_DEVICE_BYTES / _ALLOCS count them).  tv_last_kernel reports kernel id 32 and the launches used;
 * tv_last_timing and TV_COUNTER_LAST_WORKGROUPS report as for a v1 stream.
 * TV_ERR_STATE: before tv_set_layout, while a stream is active.  TV_ERR_ARG: piece_length not a power of two >= 16 KiB,
 * n != n_pieces, a piece_bytes / tree_leaves entry outside its range, NULL arrays with n > 0.
 *
 * tv_v2_stream_file_table is that stream with the library's own readers as the producer, as tv_stream_file_table:
 * the piece table as above and the file table (n_files files of lengths[k] bytes, paths NUL-separated in `paths`, in
 * file-tree order).  File k starts at its ALIGNED offset: start[k + 1] = round_up(start[k] + lengths[k],
 * piece_length); a zero-length file takes no space.  TV_ERR_ARG when the files' piece count differs from n_pieces or
 * a piece's bytes differ from what its file holds of it.  A v2 piece lies in exactly one file: it is unreadable
 * (bit 0) exactly when that file is missing, unopenable under TV_OPT_OPEN_RW, or shorter than the piece's offset in
 * it + piece_bytes (the zero-length-segment open rule of v1 does not apply).  status_out[k] (n_files entries) =
 * TV_ERR_IO when a read or open of file k failed.  Nothing is created.
 */
int tv_v2_stream_begin(tv_ctx *ctx, uint64_t n, const uint32_t *piece_bytes, const uint32_t *tree_leaves,
                       const uint8_t *hashes /* 32*n */, const uint8_t *avail_bits);
int tv_v2_stream_file_table(tv_ctx *ctx, uint64_t n_pieces, const uint32_t *piece_bytes, const uint32_t *tree_leaves,
                            const uint8_t *hashes, uint64_t n_files, const uint64_t *lengths, const char *paths,
                            uint64_t paths_bytes, const uint8_t *avail_bits, uint8_t *bitfield_out, int32_t *status_out);

/*
 * Streamed hybrid verify through the same bounded ring: BOTH hash sets of a hybrid torrent from one pass over its
 * bytes, without a resident shard (a torrent larger than the device budget, or a GPU shared with other work; two
 * separate streams would move every byte over PCIe or off the disks twice).
 *
 * tv_hybrid_stream_begin is tv_v2_stream_begin (the GLOBAL piece table carried by the call, `hashes` required, the
 * same ranges and error texts) over a layout that is the v1 space of the table (total_length with the pads, as for
 * tv_hybrid_verify) and after tv_set_digests (the v1 `pieces` string), as tv_stream_begin needs it.  It works with
 * TV_OPT_RESIDENT 0 or 1 and leaves a table set with tv_v2_set_pieces alone.  The requests follow the v2 row rule (row
 * q holds min(width, piece_bytes[piece + q] - offset) FILE bytes; an empty row is neither filled nor copied): pad ranges
 * are DEFINED as zeros and never cross PCIe.  When a unit's last request is committed the compute stream runs, over the
 * unit's chunk buffer: a column pad launch that zeroes the part of [piece_bytes, v1_len) inside the column in every row
 * that has one (each row's range derived on the device from the stream's piece table and the layout; no launch for a
 * unit without one, so a one-file torrent with no tail pays nothing), the SHA-1 column launch of a v1 stream, and the v2
 * column launch; after a window's last column the v2 level launches and the finish launch.  tv_stream_next / _commit /
 * _commit_from / _unreadable / _fill_synthetic / _abort work unchanged.  tv_stream_end returns v1 AND v2;
 * tv_hybrid_stream_end returns all three bitfields (v1_bits_out and v2_bits_out may be NULL; ceil(shard_count / 8)
 * bytes each, spare bits 0; an unreadable or unavailable piece is 0 in all three) and is TV_ERR_STATE on a stream that
 * is not a hybrid one, which then stays active.
 *
 * Geometry: C a power of two, 16 KiB <= C <= min(piece_length, 64 MiB), wn a multiple of 64 or the whole shard, as
 * for a v2 stream.  TV_OPT_STREAM_CHUNK = X > 0: tv_v2_stream_begin's rule, one window across the shard.  Otherwise,
 * under TV_OPT_RESIDENT_BUDGET (1 GiB when unset): each chunk buffer takes at most min(budget / 2, 256 MiB), and a
 * window holds at least min(shard_count, 2,048) pieces where the budget allows (SHA-1 is serial per piece: a window of
 * a few hundred whole pieces hashes slower than it stages): C starts at min(piece_length, 64 MiB) and is halved while
 * that many rows do not fit, down to 16 KiB; then wn = the largest multiple of 64 whose rows fit, at least 64.
 * TV_OPT_STREAM_ROWS has no effect.  Device memory beyond a v2 stream's: the second bitfield (16 bytes per 64 pieces,
 * shared with tv_hybrid_verify), counted in TV_COUNTER_DEVICE_BYTES / _ALLOCS and reused by a later stream it fits.
 * tv_last_kernel reports kernel id 256 and the launches used: per unit 2, plus 1 where the pad kernel ran, and per
 * window log2(piece_length / C) + 1.  tv_last_timing and TV_COUNTER_LAST_WORKGROUPS report as for the other streams.
 * TV_ERR_STATE: before tv_set_layout, before tv_set_digests, while a stream is active.  TV_ERR_ARG: as
 * tv_v2_stream_begin, and a piece_bytes[i] > v1_len(i) for a shard piece (tv_hybrid_verify's text), piece_length > 2 GiB.
 * A refused begin leaves no stream.
 *
 * tv_hybrid_stream_file_table is that stream with the library's own readers as the producer: tv_v2_stream_file_table's
 * arguments, checks, open rules (TV_OPT_OPEN_RW) and per-file status over the REAL files in file-tree order, each at
 * its aligned offset.  Pad files are not in the table: they are never opened or looked for.
 */
int tv_hybrid_stream_begin(tv_ctx *ctx, uint64_t n, const uint32_t *piece_bytes, const uint32_t *tree_leaves,
                           const uint8_t *hashes /* 32*n */, const uint8_t *avail_bits);
int tv_hybrid_stream_end(tv_ctx *ctx, uint8_t *v1_bits_out, uint8_t *v2_bits_out, uint8_t *bitfield_out);
int tv_hybrid_stream_file_table(tv_ctx *ctx, uint64_t n_pieces, const uint32_t *piece_bytes, const uint32_t *tree_leaves,
                                const uint8_t *hashes, uint64_t n_files, const uint64_t *lengths, const char *paths,
                                uint64_t paths_bytes, const uint8_t *avail_bits, uint8_t *v1_bits_out,
                                uint8_t *v2_bits_out, uint8_t *bitfield_out, int32_t *status_out);

/*
 * Streamed CREATION through the same bounded ring: the hashes of a new torrent without a resident shard.  The
 * reference's only SHA-1 loop is its creator, and that creator streams: makeTorrent reads each file in pieceLength
 * parts and hashes every part as it arrives (tools/make_torrent.ts:18-113 for a directory, :147-173 for one file;
 * hashAndStore :28-31).  tv_hash / tv_v2_hash / tv_hybrid_hash need the whole shard in device memory first; these
 * calls hash it while it arrives, within the device memory of the verify stream of the same kind.
 *
 * tv_stream_hash_begin (v1 pieces, piece.ts:16-19), tv_v2_stream_hash_begin (BEP 52 merkle pieces; the GLOBAL piece
 * table as tv_v2_stream_begin takes it) and tv_hybrid_stream_hash_begin (both; the layout is the v1 space of the table,
 * as for tv_hybrid_stream_begin) start a stream that is the verify stream of its kind in every respect but its end:
 * the same geometry (TV_OPT_STREAM_CHUNK, TV_OPT_STREAM_ROWS, TV_OPT_RESIDENT_BUDGET), ring, chunk buffers, row rule
 * and launches (the hybrid column pad launch included); tv_stream_next / _commit / _commit_from / _fill_synthetic /
 * _abort serve it unchanged.  It needs no tv_set_digests, no expected roots and no availability: every piece is
 * hashed (make_torrent.ts never skips one), and tv_stream_unreadable on it is TV_ERR_STATE (the stream stays active).
 * The layout is set with TV_OPT_RESIDENT = 0 (a windowed layout is TV_ERR_STATE).  The last launch of each window
 * stores where a verify stream's compares: the SHA-1 digests, and the merkle roots in place of the expected ones, so a
 * creation stream holds no device memory beyond the verify stream's.
 *
 * tv_stream_hash_end writes what the resident calls write, in piece order: tv_hash's 20-byte digests
 * (crypto.subtle.digest("SHA-1", ...), make_torrent.ts:28-31) into digests_out and tv_v2_hash's 32-byte roots into
 * roots_out.  A v1 stream takes roots_out == NULL, a v2 stream digests_out == NULL, a hybrid stream both pointers; a
 * required pointer that is NULL is TV_ERR_ARG and the stream is aborted.  Ending before the last column aborts
 * (TV_ERR_STATE), as for tv_stream_end.  tv_stream_end or tv_hybrid_stream_end on a creation stream, and
 * tv_stream_hash_end on a verify stream, are TV_ERR_STATE and abort the stream.  A refused call writes nothing to its
 * outputs.  tv_last_timing, tv_last_kernel (the ids and launch counts of the verify streams),
 * TV_COUNTER_LAST_WORKGROUPS and TV_COUNTER_LAST_STREAM_REQUESTS report as for the verify streams.
 *
 * The *_hash_file_table calls are those streams with the library's own readers as the producer, the file table as
 * tv_stream_file_table / tv_v2_stream_file_table take it (the v2 and hybrid forms: the REAL files, each at its aligned
 * offset).  Files are opened read-only, as the creator opens its sources (Deno.open(path), make_torrent.ts:78),
 * whatever TV_OPT_OPEN_RW says, and the cold-file options apply as they do to verify.  Creation cannot skip a piece:
 * if any byte of the shard cannot be read (a missing, unopenable or short file) the call returns TV_ERR_IO with
 * status_out[k] = TV_ERR_IO for the file, the outputs untouched and the stream aborted; the ctx stays usable.
 */
int tv_stream_hash_begin(tv_ctx *ctx);
int tv_v2_stream_hash_begin(tv_ctx *ctx, uint64_t n, const uint32_t *piece_bytes, const uint32_t *tree_leaves);
int tv_hybrid_stream_hash_begin(tv_ctx *ctx, uint64_t n, const uint32_t *piece_bytes, const uint32_t *tree_leaves);
int tv_stream_hash_end(tv_ctx *ctx, uint8_t *digests_out /* 20*shard_count */, uint8_t *roots_out /* 32*shard_count */);
int tv_stream_hash_file_table(tv_ctx *ctx, uint64_t n, const uint64_t *lengths, const char *paths, uint64_t paths_bytes,
                              uint8_t *digests_out, int32_t *status_out);
int tv_v2_stream_hash_file_table(tv_ctx *ctx, uint64_t n_pieces, const uint32_t *piece_bytes, const uint32_t *tree_leaves,
                                 uint64_t n_files, const uint64_t *lengths, const char *paths, uint64_t paths_bytes,
                                 uint8_t *roots_out, int32_t *status_out);
int tv_hybrid_stream_hash_file_table(tv_ctx *ctx, uint64_t n_pieces, const uint32_t *piece_bytes,
                                     const uint32_t *tree_leaves, uint64_t n_files, const uint64_t *lengths,
                                     const char *paths, uint64_t paths_bytes, uint8_t *digests_out, uint8_t *roots_out,
                                     int32_t *status_out);

/* Page-locked host memory for tv_verify_host / tv_stage sources.  A pinned source is read by
 * DMA directly (no staging memcpy); pageable memory goes through the library's pinned ring.
 * tv_host_register pins an existing range (e.g. a caller's buffer), tv_host_unregister undoes it. */
int tv_host_alloc(uint64_t bytes, void **out);
int tv_host_free(void *ptr);
int tv_host_register(void *ptr, uint64_t bytes);
int tv_host_unregister(void *ptr);

/* Options (tv_set_option keys): what a host integrating the library sets.  (Measurement and test knobs -- kernel
 * forcing, stride padding, file-staging A/B modes, NUMA binding, probes, fault injection -- are keys of the
 * library's internal header torrent_amd/csrc/tv_options_internal.h, which only the tests and tools use.) */
#define TV_OPT_STREAM_CHUNK 3 /* tv_verify_host / tv_stream_*: bytes of each piece per streamed column across the
                                 whole shard (0, default: tv_stream_*: the widest power of two <= L whose column over
                                 the shard is <= 512 MiB; tv_verify_host / tv_stream_file_table: windows x columns
                                 within TV_OPT_RESIDENT_BUDGET, or 1 GiB) */
#define TV_OPT_FILE_DIRECT_MIN 7 /* tv_stage_files: segment length that takes the long-segment path (default 32 MiB) */
#define TV_OPT_FILE_THREADS 8    /* host threads of the context (default 16): tv_stage_file(s)' readers (shared by the
                                    two staging lanes), and the copies of pageable tv_stage sources into the pinned
                                    ring.  A host running several contexts in one process divides its CPU share
                                    among them (verify.py / verify.ts do) */
#define TV_OPT_RESIDENT 10       /* 1 (default): tv_set_layout allocates the resident payload; 0: it does not (a
                                    streamed-only ctx, tv_stream_*; the resident calls then fail with TV_ERR_STATE).
                                    Takes effect at the next tv_set_layout */
#define TV_OPT_TWIN_FILL 13      /* twin kernel with fewer workgroups than 2 per CU (resident calls, cfg4's shards at
                                    N = 4 / 8): 1 (default, auto) = add light companion workgroups up to 2 per CU
                                    that run the same instruction stream on one piece of their main workgroup on
                                    the otherwise idle SIMDs and discard the result (a CU running one twin
                                    workgroup is ~4.5 % slower per block than one running two; +2.2-3.2 %, 0.2-0.4 %
                                    more HBM reads) -- unless other processes hold >= 1 GiB of this GPU's memory
                                    (the kernel driver's per-process accounting): on a GPU shared with other work
                                    the companions would take CUs it may be using; 0 = the real grid only, always.
                                    Bitfields are the same either way.  tv_verify_list adds them only to a list of
                                    >= 32 x CUs pieces */
#define TV_OPT_RESIDENT_BUDGET 16 /* bytes of device memory the resident payload may take (0, default: the GPU's free
                                     memory at tv_set_layout less 4 GiB and 64 B per piece).  A shard larger than it
                                     gets a windowed layout (tv_set_layout).  Takes effect at the next tv_set_layout */
#define TV_OPT_LIST_SLOTS 17      /* K > 0: tv_set_layout allocates a pool of K piece slots instead of the shard (see
                                     tv_set_layout; incremental verify, tv_verify_list).  0 (default) = off.  Takes
                                     effect at the next tv_set_layout */
#define TV_OPT_OPEN_RW 18         /* how tv_stage_file(s) open files: 1 (default) = read + write, as fsStorage.get
                                     opens every segment (storage.ts:28-32,158; an unwritable file reads as null);
                                     0 = read-only, as make_torrent.ts:78 opens its sources (creation mode from files
                                     the process may not write).  Zero-length segments' open check follows it */
#define TV_OPT_STREAM_ROWS 19     /* tv_stream_* request rows: 0 (default) = columns of TV_OPT_STREAM_CHUNK bytes of
                                     every shard piece (one launch per column over the whole shard); 1 = whole
                                     pieces (when a piece fits one ring slot), in windows of up to 4 GiB of pieces
                                     per chunk buffer (a multiple of 64 pieces; TV_OPT_RESIDENT_BUDGET / 2 if set
                                     and smaller), one launch per window: one Storage.get per piece for a reader
                                     that opens a file per call (fsStorage.get, storage.ts:149-172).  Set it
                                     before tv_stream_begin (TV_ERR_STATE during a stream) */
#define TV_OPT_CLOCK_PROBE 20     /* 1: verify / hash launches (resident, windows, stream units) record the shader clock
                                     they ran at (workgroup 0 reads the shader and 100 MHz real-time counters at its
                                     start and end; TV_COUNTER_LAST_CLOCK_KHZ).  0 (default) = off */
int tv_set_option(tv_ctx *ctx, int key, int64_t value);
int tv_get_option(tv_ctx *ctx, int key, int64_t *value);

/* Timing of the last tv_verify / tv_hash / tv_verify_host call, from HIP events recorded on the
 * library's compute stream: kernel_ms = the verify kernel(s) only; total_ms = whole call. */
int tv_last_timing(tv_ctx *ctx, double *kernel_ms, double *total_ms);

/* Kernel chosen for the last call (1 lane, 2 split, 4 twin; 8 = the v2 SHA-256 merkle kernels, 16 = the v2 list
 * kernel, 32 = a v2 stream's column kernel, 64 = the v2 block kernel, 128 = a hybrid call's pad + SHA-1 + v2 launches,
 * 256 = a hybrid stream's, 512 = a hybrid list call's pad + SHA-1 list + v2 list launches) and launches it used. */
int tv_last_kernel(tv_ctx *ctx, int *kernel, int *launches);

/* Resource counters of a ctx (tv_get_counter keys): how often tv_set_layout and the calls after it had to
 * allocate device memory, and what the ctx holds now.  A run of small layouts on a ctx (verify_piece, list
 * flushes) must not reallocate, and a small call must not evict a bulk call's payload; these make both
 * observable.  No reference counterpart (the reference holds no device memory). */
#define TV_COUNTER_PAYLOAD_ALLOCS 1 /* resident payload allocations since tv_create */
#define TV_COUNTER_DEVICE_ALLOCS 2  /* device allocations of every kind since tv_create */
#define TV_COUNTER_PAYLOAD_BYTES 3  /* bytes of the resident payload allocation held now (0: none) */
#define TV_COUNTER_DEVICE_BYTES 4   /* bytes of device memory held now */
#define TV_COUNTER_LAST_WORKGROUPS 5 /* workgroups of the last verify / hash / list launch (companion
                                        workgroups of TV_OPT_TWIN_FILL included) */
#define TV_COUNTER_NUMA_NODE 6       /* the GPU's NUMA node (sysfs numa_node of its PCI function); UINT64_MAX if
                                        unknown */
#define TV_COUNTER_RING_NODE 7       /* the NUMA node holding the first pinned ring slot's first page; UINT64_MAX
                                        if the ring is not allocated yet or the node is unknown */
#define TV_COUNTER_WINDOW_PIECES 8   /* pieces per window of a windowed layout (0: the shard is resident whole) */
#define TV_COUNTER_WINDOWS 9         /* windows hashed by the current (or last) pass of a windowed layout */
#define TV_COUNTER_BUDGET 10         /* the device budget the last tv_set_layout applied, bytes (0: no resident payload
                                        or a slot pool) */
#define TV_COUNTER_SLOTS_USED 11     /* slots of a slot pool holding a staged piece not yet listed */
#define TV_COUNTER_LAST_CLOCK_KHZ 12 /* TV_OPT_CLOCK_PROBE: the shader clock of the last probed launch's workgroup 0, kHz
                                        (shader-counter ticks / 100 MHz real-time ticks over its life); 0 = none.
                                        Waits for the ctx's queued kernels */
int tv_get_counter(tv_ctx *ctx, int key, uint64_t *value);

/* Block until all work queued by the ctx is complete. */
int tv_synchronize(tv_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* TORRENT_VERIFY_H */
