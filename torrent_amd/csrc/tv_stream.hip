// tv_stream.hip -- the streamed verify engine (tv_stream_*; tv_verify_host runs on it): a bounded pinned ring
// between the caller's bytes and two device chunk buffers, one kernel launch per column / window of pieces.
// tv_v2_stream_begin / tv_v2_stream_file_table run BitTorrent v2 pieces through the same engine: one column-kernel
// launch per unit and the window's top tree after its last column.  tv_hybrid_stream_begin /
// tv_hybrid_stream_file_table run both hash sets of a hybrid torrent over each unit's chunk buffer: the column pad
// kernel, the SHA-1 column launch, the v2 column launch.  tv_stream_hash_begin and its v2 and hybrid forms run each kind
// in creation mode (StreamState::hash): the same units and launches, the last ones storing the hashes, which
// tv_stream_hash_end hands out.
//
// The kinds share one row rule (stream_row_bytes), one geometry setter (set_geometry), one commit path
// (stream_commit_locked over tv_plan.h for_row_copies) and one unit dispatch (unit_launch); the library's own reader
// (stream_files_locked) is shard_is_cold, FdCache, tv_plan.h walk_row_files and read_segment.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cassert>
#include <cerrno>
#include <cstring>
#include <memory>

#include "tv_ctx.h"
#include "tv_fileio.h"

namespace tvi {

// ---- streamed verify (tv_stream_*; tv_verify_host runs on it too) ------------------------------------
//
// Column `col` carries bytes [col*C, col*C + C) of every shard piece.  Its rows arrive as requests of up to
// one ring slot (64 MiB) each, filled by the caller, and are DMA'd from the slot into device chunk buffer
// unit & 1 (row pitch C + 256; a unit is one column of one window of pieces).  When a unit's last request is
// committed, its launch set (unit_launch) hashes it on the compute stream while the next unit's requests fill the
// other buffer: for v1 pieces one SHA-1 launch (chaining values persist in d_state; the last column pads, compares
// and writes the bitfield).  Host memory in flight: the ring.

// A stream call with no stream begun: TV_ERR_STATE and `text` (a batch layout, where none can begin: its own text).
static int no_stream(tv_ctx* c, const char* text) {
    return c->batch_on ? batch_refused(c) : fail(c, TV_ERR_STATE, "%s", text);
}

// The row rule of the begun stream: the piece's valid bytes inside the column, 0 when the piece ends before it.  A v1
// piece has piece_len bytes (piece.ts:16-19: only the torrent's last piece is short); a v2 or hybrid piece has its
// table's (st.v2_bytes), so any row may be short or empty: every file ends a piece.
uint64_t stream_row_bytes(const tv_ctx* c, uint64_t piece, uint64_t offset, uint64_t width) {
    const uint64_t plen = c->st.v2 ? c->st.v2_bytes[piece - c->first] : piece_len(c, piece);
    return plen > offset ? std::min(width, plen - offset) : 0;
}

// Drop an active stream: give its lent slot back and let the queued copies and kernels drain.
void stream_abort_locked(tv_ctx* c) {
    StreamState& st = c->st;
    if (!st.active) return;
    if (st.outstanding && st.slot >= 0) (void)release_slot(c, st.slot, 0);
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    st = StreamState{};
}

// Row mode (TV_OPT_STREAM_ROWS): each request row is a whole piece (one Storage.get per piece), which needs a
// piece to fit one ring slot.
bool stream_rows(const tv_ctx* c) { return c->stream_rows && c->L <= kRingSlotBytes; }

// Row mode's window: whole pieces per chunk buffer, a multiple of 64 (bitfield words of their own), at most
// kRowWindowBytes per buffer (TV_OPT_RESIDENT_BUDGET / 2 if smaller), the shard when it fits.
constexpr uint64_t kRowWindowBytes = 4ull << 30;
uint64_t stream_row_window(const tv_ctx* c) {
    const uint64_t pitch = (c->L + 63) / 64 * 64 + 256;
    uint64_t bytes = kRowWindowBytes;
    if (c->budget_opt) bytes = std::min<uint64_t>(bytes, c->budget_opt / 2);
    const uint64_t w = std::max<uint64_t>(64, bytes / pitch / 64 * 64);
    return std::min<uint64_t>(w, c->count);
}

// Column width: TV_OPT_STREAM_CHUNK, or ~512 MiB columns (64 KiB .. L); a multiple of 64, at most one slot.
uint64_t stream_column(const tv_ctx* c) {
    uint64_t C = c->stream_chunk;
    if (!C) {
        C = 64ull << 10;
        while (C * 2 <= c->L && C * 2 * c->count <= (512ull << 20)) C *= 2;
    }
    C = std::min<uint64_t>((C / 64) * 64, ((c->L + 63) / 64) * 64);
    return std::max<uint64_t>(64, std::min<uint64_t>(C, kRingSlotBytes));
}

// Bytes of each of the two device chunk buffers a stream over the current geometry needs.
uint64_t stream_chunk_need(const tv_ctx* c) {
    if (!c->count) return 0;
    if (stream_rows(c)) return ((c->L + 63) / 64 * 64 + 256) * stream_row_window(c) + kSlack;
    return (stream_column(c) + 256) * c->count + kSlack;
}

// The geometry of a stream under a device budget: tv_plan.h stream_geometry (its rationale there).
void budget_geometry(const tv_ctx* c, uint64_t budget, uint64_t min_win, uint64_t* col, uint64_t* win) {
    stream_geometry(c->L, c->count, budget, min_win, kRingSlotBytes, kSlack, col, win);
}

// What both begin calls start with: a fresh state holding the availability bits (a creation stream, `hash`, has none:
// every piece is hashed).  false = the shard is empty and the stream is active already: there is nothing to hash, the
// first tv_stream_next reports completion.
static bool begin_state(tv_ctx* c, const uint8_t* avail_bits, bool hash = false) {
    StreamState& st = c->st;
    st = StreamState{};
    st.hash = hash;
    st.av.assign((c->count + 7) / 8, 0xFF);
    if (avail_bits && !hash) memcpy(st.av.data(), avail_bits, st.av.size());
    st.active = c->count == 0;
    return !st.active;
}

// The two chunk buffers of `need` bytes each; both go before either is replaced.
static int grow_chunks(tv_ctx* c, uint64_t need) {
    if (buf_fits(c->d_chunk[0], need, true) && buf_fits(c->d_chunk[1], need, true)) return TV_OK;
    for (DevBuf& b : c->d_chunk) free_buf(b);
    for (DevBuf& b : c->d_chunk) {
        const int rc = grow_buf(c, b, need, true, need);
        if (rc) return rc;
    }
    return TV_OK;
}

// ... and end with: the call's first event, the bitfield words cleared, both chunk buffers free to be written.
static int begin_done(tv_ctx* c) {
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    TV_HIP(c, hipMemsetAsync(c->d_out, 0, c->bit_words * 8, c->stream));  // fail closed, as tv_verify
    TV_HIP(c, hipEventRecord(c->done_ev[0], c->stream));
    TV_HIP(c, hipEventRecord(c->done_ev[1], c->stream));
    c->st.active = true;
    return TV_OK;
}

// The units of a stream of columns of C bytes over windows of wn pieces, and the rows of a request (req_bytes, or one
// ring slot).  A v2 or hybrid stream's C divides L.
static void set_geometry(tv_ctx* c, uint64_t C, uint64_t wn, uint64_t req_bytes) {
    StreamState& st = c->st;
    st.C = C;
    st.wn = wn;
    st.row_pitch = C + 256;  // (tail over-read slack per row)
    st.ncol = (c->L + C - 1) / C;
    st.nwin = (c->count + wn - 1) / wn;
    st.nunits = st.nwin * st.ncol;
    st.rows_per_req = std::max<uint64_t>(1, (req_bytes ? std::min<uint64_t>(req_bytes, kRingSlotBytes) : kRingSlotBytes) / C);
}

// (The begin functions share begin_state, set_geometry, grow_chunks and begin_done; the HIP calls between them stay per
// kind: a v2 begin synchronises the compute stream before it replaces buffers and after its table copy, v1 never.)
int stream_begin_locked(tv_ctx* c, const uint8_t* avail_bits, uint64_t col_override = 0, uint64_t win_override = 0,
                        uint64_t req_bytes = 0, bool hash = false) {
    if (!begin_state(c, avail_bits, hash)) return TV_OK;
    if (stream_rows(c))  // whole pieces per row, windows of stream_row_window pieces
        set_geometry(c, (c->L + 63) / 64 * 64, stream_row_window(c), req_bytes);
    else                 // columns across the whole shard (or across windows of win_override pieces)
        set_geometry(c, col_override ? col_override : stream_column(c),
                     win_override ? std::min(win_override, c->count) : c->count, req_bytes);
    const int rc = grow_chunks(c, c->st.row_pitch * c->st.wn + kSlack);
    return rc ? rc : begin_done(c);
}

// A BitTorrent v2 stream (tv_v2_stream_begin): the same ring, requests and chunk buffers, the units hashed as merkle
// pieces.  A column of C = c x 16 KiB bytes of a piece is a whole aligned subtree of its tree, so the column kernel
// reduces it to one node in the window's partial-node buffer and NOTHING is carried between columns (the v1 columns
// carry each piece's SHA-1 chaining value in d_state); the window's last column is followed by the top tree over the
// L / C nodes of each piece: log2(L / C) level launches and the finish launch, on a table derived for the window.
// The geometry: tv_plan.h v2_stream_geometry.  The caller has checked the state and the table (v2_check_table).
//
// hybrid (tv_hybrid_stream_begin): the same stream under tv_plan.h hybrid_stream_geometry, whose units are also hashed
// as v1 pieces (unit_launch): the SHA-1 column launches use the state of a v1 stream (the digests, d_state,
// d_base_avail; bits into d_out), the v2 launches write a second bitfield, the first half of d_hy_bits (its sizing
// rule: bit_words), cleared here so it fails closed.  The caller has also checked the digests and piece_bytes <= v1_len.
//
// hash (tv_v2_stream_hash_begin, tv_hybrid_stream_hash_begin): the same stream without expected roots (`hashes` is not
// read): the hash rows of the table stay zero until the windows' finish launches write the roots there.
int v2_stream_begin_locked(tv_ctx* c, const uint32_t* piece_bytes, const uint32_t* tree_leaves, const uint8_t* hashes,
                           const uint8_t* avail_bits, uint64_t req_bytes = 0, bool hybrid = false, bool hash = false) {
    StreamState& st = c->st;
    const bool hashes_any = begin_state(c, avail_bits, hash);
    st.v2 = true;
    st.hybrid = hybrid;
    st.kernel = hybrid ? TV_KERNEL_HYBRID_STREAM : TV_KERNEL_V2_STREAM;
    if (!hashes_any) return TV_OK;
    uint64_t C = 0, wn = 0;
    (hybrid ? hybrid_stream_geometry : v2_stream_geometry)(c->L, c->count, c->budget_opt ? c->budget_opt : (1ull << 30),
                                                           c->stream_chunk, kSlack, &C, &wn);
    assert(C && c->L % C == 0);   // (both powers of two, C <= L: set_geometry's rounded-up column count is exact)
    set_geometry(c, C, wn, req_bytes);
    while ((kV2Leaf << st.v2_logc) < C) st.v2_logc++;
    while ((1ull << st.v2_logn) < st.ncol) st.v2_logn++;
    TV_HIP(c, hipStreamSynchronize(c->stream));   // (nothing queued still reads the buffers replaced below)
    // (whole-piece columns run no level: the finish launch reads the column nodes themselves, level buffer A alone)
    const uint64_t need_tab = v2s_tab_words(c->count), need_nodes = st.ncol > 1 ? v2_node_words(wn, st.ncol) : 8 * wn;
    int rc = grow_chunks(c, st.row_pitch * wn + kSlack);
    if (!rc) rc = grow_buf(c, c->d_v2s_tab, need_tab, true, need_tab);
    if (!rc) rc = grow_buf(c, c->d_v2s_nodes, need_nodes, true, need_nodes);
    if (!rc && hybrid) rc = grow_buf(c, c->d_hy_bits, c->bit_words, false, c->bit_words);
    if (rc) return rc;
    // the shard's rows: bytes, leaves, the width of each piece's top tree over its column nodes, and the expected root
    // words (big-endian values), SoA [8][pieces of the window] window after window: a window's launches see a table
    // of their own at piece j0 (expected words at 8 * j0)
    std::vector<uint32_t> tab(need_tab, 0);
    st.v2_bytes.resize(c->count);
    for (uint64_t j = 0; j < c->count; j++) {
        const uint64_t i = c->first + j, j0 = j / wn * wn, wcount = std::min(wn, c->count - j0);
        st.v2_bytes[j] = tab[j] = piece_bytes[i];
        tab[c->count + j] = tree_leaves[i];
        tab[2 * c->count + j] = std::max<uint32_t>(1, tree_leaves[i] >> st.v2_logc);
        if (!hash) digest_pack(hashes + 32 * i, 8, tab.data() + v2s_hash_base(c->count, j0), wcount, j - j0);
    }
    TV_HIP(c, hipMemcpyAsync(c->d_v2s_tab.ptr, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    TV_HIP(c, hipStreamSynchronize(c->stream));   // (tab is the call's own)
    if (hybrid) TV_HIP(c, hipMemsetAsync(c->d_hy_bits.ptr, 0, c->bit_words * 8, c->stream));
    return begin_done(c);
}

// ---- a completed unit's launches (unit_launch), on the compute stream after col_ev; each counts st.launches ----------
// A v2 unit's column kernel on the chunk buffer: the only v2 launch that reads it.
static int v2_column_launch(tv_ctx* c, int buf, uint64_t j0, uint64_t wcount) {
    StreamState& st = c->st;
    uint32_t* tab = c->d_v2s_tab.get<uint32_t>();
    TvV2Col k{};
    k.data = c->d_chunk[buf].get<uint8_t>();
    k.stride = st.row_pitch;
    k.n = (uint32_t)wcount;
    k.logc = st.v2_logc;
    k.logn = st.v2_logn;
    k.col = (uint32_t)(st.unit % st.ncol);
    k.piece_bytes = tab + j0;
    k.tree_leaves = tab + c->count + j0;
    k.nodes = c->d_v2s_nodes.get<uint32_t>();
    k.clock = c->clock_probe ? c->d_clock : nullptr;
    TV_HIP(c, tv_v2_launch_column(k, c->stream, &c->last_workgroups));
    st.launches++;
    return TV_OK;
}

// After a v2 window's last column, its top tree over the column nodes (one level launch per doubling of the columns,
// none when a column is a whole piece) and the finish launch into the window's bitfield words (a creation stream: the
// roots into the window's hash rows of the table, [8][wcount] at its base).
static int v2_top_launch(tv_ctx* c, uint64_t j0, uint64_t wcount) {
    StreamState& st = c->st;
    uint32_t* tab = c->d_v2s_tab.get<uint32_t>();
    TvV2 p{};
    p.n = (uint32_t)wcount;
    p.logW = st.v2_logn;
    p.piece_bytes = tab + j0;
    p.tree_leaves = tab + 2 * c->count + j0;
    p.nodes_a = c->d_v2s_nodes.get<uint32_t>();
    p.nodes_b = p.nodes_a + v2s_nodes_b_base(wcount, st.ncol);
    if (st.hash) p.roots = tab + v2s_hash_base(c->count, j0);
    else p.expect = tab + v2s_hash_base(c->count, j0);
    // (availability: st.av, applied at the end with the unreadable pieces; a hybrid stream's v2 bits: d_hy_bits)
    p.out64 = (st.hybrid ? c->d_hy_bits.get<uint64_t>() : c->d_out) + j0 / 64;
    p.out_words = (uint32_t)((wcount + 63) / 64);
    for (uint32_t l = 0; l < st.v2_logn; l++) {
        TV_HIP(c, tv_v2_launch_level(p, l, st.v2_logn, c->stream));
        st.launches++;
    }
    TV_HIP(c, tv_v2_launch_finish(p, st.hash, c->stream));
    st.launches++;
    return TV_OK;
}

// A completed unit's SHA-1 column launch: the window's pieces (the shard's digest / state rows from j0; bitfield words
// from j0 / 64: a window of a multi-window stream is a multiple of 64 pieces) over bytes [offset, offset + C) of each,
// the chaining values carried in d_state; the window's last column pads, compares and writes the bits (a creation
// stream: stores the digests in the shard's d_hash rows from j0, window_launch's out_digests [5][count], and is given
// neither digests nor availability).
static int v1_unit_launch(tv_ctx* c, int buf, uint64_t j0, uint64_t wcount, uint64_t offset) {
    StreamState& st = c->st;
    const bool last = st.unit % st.ncol + 1 == st.ncol;
    TvPieces p = window_launch(c, j0, wcount, c->d_chunk[buf].get<uint8_t>());
    p.stride = st.row_pitch;
    p.avail64 = c->d_base_avail + j0 / 64;
    p.out64 = c->d_out + j0 / 64;
    p.data_off = offset;
    p.blk_begin = offset / 64;
    p.blk_end = last ? UINT64_MAX : (offset + st.C) / 64;
    p.finalize = last ? 1 : 0;
    if (st.hash) {
        p.digests = nullptr;
        p.avail64 = nullptr;
        p.out64 = nullptr;
    }
    const int kernel = choose_kernel_n(c, wcount, p.n_main < p.n);
    if (!st.v2) st.kernel = kernel;   // (tv_last_kernel: a hybrid stream reports its own id)
    p.lane_pairs = lane_pairs_for(c, p.n);
    TV_HIP(c, tv_launch_verify(p, kernel, st.hash, c->stream, c->split_pairs, &c->last_workgroups));
    st.launches++;
    return TV_OK;
}

// A hybrid unit's column pad launch, when a row of the unit has a pad range inside the column (the host knows both
// tables: a unit without one pays nothing).
static int hybrid_pad_launch(tv_ctx* c, int buf, uint64_t j0, uint64_t wcount, uint64_t offset) {
    StreamState& st = c->st;
    uint64_t chunks = 0;   // the most a row's range has
    for (uint64_t q = 0; q < wcount; q++) {
        uint64_t b, e;
        hybrid_col_range(st.v2_bytes[j0 + q], hybrid_v1_len(c->total, c->L, c->first + j0 + q), offset, st.C, &b, &e);
        chunks = std::max(chunks, hybrid_col_chunks(b, e));
    }
    if (!chunks) return TV_OK;
    TV_HIP(c, hybrid_col_pad_launch(c, c->d_chunk[buf].get<uint8_t>(), st.row_pitch, c->d_v2s_tab.get<uint32_t>() + j0,
                                    c->first + j0, offset, st.C, wcount, chunks, c->stream));
    st.launches++;
    return TV_OK;
}

// The launch set of the completed unit in chunk buffer `buf` (pieces [j0, j0 + wcount) of the shard, column bytes from
// `offset`).  v1: the SHA-1 column launch.  v2: the column kernel, then the window's top tree.  hybrid: the pad launch,
// the SHA-1 column launch, then the v2 set.  done_ev[buf] follows the last launch that reads the buffer.
static int unit_launch(tv_ctx* c, int buf, uint64_t j0, uint64_t wcount, uint64_t offset) {
    StreamState& st = c->st;
    int rc = st.hybrid ? hybrid_pad_launch(c, buf, j0, wcount, offset) : TV_OK;
    if (!rc && (st.hybrid || !st.v2)) rc = v1_unit_launch(c, buf, j0, wcount, offset);
    if (!rc && st.v2) rc = v2_column_launch(c, buf, j0, wcount);
    if (rc) return rc;
    TV_HIP(c, hipEventRecord(c->done_ev[buf], c->stream));
    return st.v2 && st.unit % st.ncol + 1 == st.ncol ? v2_top_launch(c, j0, wcount) : TV_OK;
}

int stream_next_locked(tv_ctx* c, tv_stream_req* req) {
    StreamState& st = c->st;
    if (!st.active) return no_stream(c, "tv_stream_begin has not been called");
    if (st.outstanding)
        return fail(c, TV_ERR_STATE, "request %llu is still outstanding (commit it first)", (unsigned long long)st.req.seq);
    *req = tv_stream_req{};
    if (st.unit >= st.nunits) return TV_OK;  // rows == 0: every byte has been requested
    const int buf = (int)(st.unit & 1);
    const uint64_t j0 = st.unit / st.ncol * st.wn, wcount = std::min(st.wn, c->count - j0);
    // the first copy into chunk buffer `buf` waits for the kernel that last read it
    if (st.row == 0) TV_HIP(c, hipStreamWaitEvent(c->copy_stream, c->done_ev[buf], 0));
    int rc = take_slot(c, &st.slot, 0);
    if (rc) return rc;
    req->piece = c->first + j0 + st.row;
    req->rows = std::min<uint64_t>(st.rows_per_req, wcount - st.row);
    req->offset = st.unit % st.ncol * st.C;
    req->width = std::min<uint64_t>(st.C, c->L - req->offset);
    req->slot = c->ring[st.slot];
    req->seq = ++st.seq;
    st.req = *req;
    st.outstanding = true;
    return TV_OK;
}

// Queue the outstanding request's rows [0, rows_copy) (the others are unreadable and not copied).  Source:
// the request's slot (src == nullptr), or caller memory at src (row q at src + q*pitch), DMA'd directly when
// page-locked and gathered into the slot by the lane-0 pool otherwise.  One body for every kind of stream.
int stream_commit_locked(tv_ctx* c, const tv_stream_req* req, const uint8_t* src, uint64_t pitch, bool pinned,
                         uint64_t rows_copy) {
    StreamState& st = c->st;
    if (!st.active) return no_stream(c, "tv_stream_begin has not been called");
    if (!st.outstanding) return fail(c, TV_ERR_STATE, "no outstanding request (call tv_stream_next)");
    if (!req || req->seq != st.req.seq || req->piece != st.req.piece || req->rows != st.req.rows)
        return fail(c, TV_ERR_ARG, "the request does not match outstanding request %llu", (unsigned long long)st.req.seq);
    const tv_stream_req r = st.req;
    const int buf = (int)(st.unit & 1);
    const uint64_t j0 = st.unit / st.ncol * st.wn, wcount = std::min(st.wn, c->count - j0);
    uint8_t* dst = c->d_chunk[buf].get<uint8_t>() + st.row * st.row_pitch;
    uint8_t* slot = c->ring[st.slot];
    const uint64_t n = std::min(rows_copy, r.rows);
    const auto bytes = [&](uint64_t q) { return stream_row_bytes(c, r.piece + q, r.offset, r.width); };
    const uint8_t* from = slot;
    uint64_t from_pitch = r.width;
    if (src && pinned) {
        from = src;
        from_pitch = pitch;
    } else if (src) {   // each row's valid bytes into the slot, ~4 MiB of rows per task
        const uint64_t per = std::max<uint64_t>(1, (4ull << 20) / r.width);
        c->pool[0].run(c->file_threads, (n + per - 1) / per, [&](uint64_t t) {
            for (uint64_t q = t * per; q < std::min(n, (t + 1) * per); q++)
                if (const uint64_t nb = bytes(q)) tv_copy_host(slot + q * r.width, src + q * pitch, nb);
        });
    }
    // a run of full rows is one 2D copy, a short row a copy of its own, an empty row none (v1: a run, then the tail)
    int rc = for_row_copies(n, r.width, bytes, [&](uint64_t q, uint64_t rows, uint64_t nb) -> int {
        if (nb == r.width)
            TV_HIP(c, hipMemcpy2DAsync(dst + q * st.row_pitch, st.row_pitch, from + q * from_pitch, from_pitch, r.width,
                                       rows, hipMemcpyHostToDevice, c->copy_stream));
        else
            TV_HIP(c, hipMemcpyAsync(dst + q * st.row_pitch, from + q * from_pitch, nb, hipMemcpyHostToDevice,
                                     c->copy_stream));
        return TV_OK;
    });
    if (rc) return rc;
    st.outstanding = false;
    const int s = st.slot;
    st.slot = -1;
    rc = release_slot(c, s, 0);  // its event follows the copies just queued
    if (rc) return rc;
    st.row += r.rows;
    if (st.row < wcount) return TV_OK;
    // the unit is complete: hash it while the caller fills the next one
    TV_HIP(c, hipEventRecord(c->col_ev[buf], c->copy_stream));
    TV_HIP(c, hipStreamWaitEvent(c->stream, c->col_ev[buf], 0));
    if (!st.k0) {
        TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
        st.k0 = true;
    }
    rc = unit_launch(c, buf, j0, wcount, r.offset);
    if (rc) return rc;
    st.unit++;
    st.row = 0;
    return TV_OK;
}

// v1_out / v2_out (optional; tv_hybrid_stream_end): a hybrid stream's own two bitfields; bitfield_out is their AND.
int stream_end_locked(tv_ctx* c, uint8_t* bitfield_out, uint8_t* v1_out = nullptr, uint8_t* v2_out = nullptr) {
    StreamState& st = c->st;
    if (!st.active) return no_stream(c, "tv_stream_begin has not been called");
    if (st.hash) {
        stream_abort_locked(c);
        return fail(c, TV_ERR_STATE, "the active stream is a creation stream (it ends with tv_stream_hash_end); aborted");
    }
    if (st.outstanding || st.unit < st.nunits) {
        const unsigned long long done = st.unit, all = st.nunits;
        stream_abort_locked(c);
        return fail(c, TV_ERR_STATE, "stream ended before its last column (%llu of %llu hashed); aborted", done, all);
    }
    if (c->count) {
        if (!bitfield_out) {
            stream_abort_locked(c);
            return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
        }
        TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
        const size_t wbytes = c->bit_words * 8;
        int rc = TV_OK;
        if (st.hybrid) {   // the v2 bits ride behind the v1 bits in h_bits (read_bits waits for both copies)
            rc = ensure_hbits(c, 2 * wbytes);
            if (!rc && hipMemcpyAsync(c->h_bits + wbytes, c->d_hy_bits.ptr, wbytes, hipMemcpyDeviceToHost, c->stream))
                rc = fail(c, TV_ERR_HIP, "tv_stream_end: the copy of the v2 bitfield failed");
        }
        if (!rc) rc = read_bits(c, bitfield_out);
        if (rc) {
            stream_abort_locked(c);
            return rc;
        }
        for (size_t k = 0; k < st.av.size(); k++) {
            bitfield_out[k] &= st.av[k];  // unreadable pieces: bit 0 (in every bitfield of a hybrid stream)
            if (!st.hybrid) continue;
            const uint8_t b2 = c->h_bits[wbytes + k] & st.av[k];   // (spare bits: 0 in the v1 bits, so in the AND)
            if (v1_out) v1_out[k] = bitfield_out[k];
            if (v2_out) v2_out[k] = k + 1 == st.av.size() && c->count % 8 ? b2 & (uint8_t)(0xFF00u >> (c->count % 8)) : b2;
            bitfield_out[k] &= b2;
        }
        c->last_kernel = st.kernel;
        c->last_launches = st.launches;   // (a v1 stream: one per unit)
        rc = finish_timing(c);
        c->last_stream_requests = st.seq;   // (TV_COUNTER_LAST_STREAM_REQUESTS: completed streams only)
        st = StreamState{};
        return rc;
    }
    c->last_stream_requests = st.seq;   // (an empty shard: 0)
    st = StreamState{};
    return TV_OK;
}

// The end of a creation stream (tv_stream_hash_end): what the resident calls hand back -- tv_hash's digests out of
// d_hash (a v1 or hybrid stream), tv_v2_hash's roots out of the table's hash rows (a v2 or hybrid stream), through the
// digest codec, in piece order.  Every refusal comes before the first byte is written.
int stream_hash_end_locked(tv_ctx* c, uint8_t* digests_out, uint8_t* roots_out) {
    StreamState& st = c->st;
    if (!st.active) return no_stream(c, "tv_stream_hash_begin has not been called");
    if (!st.hash) {
        stream_abort_locked(c);
        return fail(c, TV_ERR_STATE, "the active stream is a verify stream (it ends with tv_stream_end); aborted");
    }
    if (st.outstanding || st.unit < st.nunits) {
        const unsigned long long done = st.unit, all = st.nunits;
        stream_abort_locked(c);
        return fail(c, TV_ERR_STATE, "stream ended before its last column (%llu of %llu hashed); aborted", done, all);
    }
    const bool v1 = !st.v2 || st.hybrid, v2 = st.v2;
    if (c->count && ((v1 && !digests_out) || (v2 && !roots_out))) {
        stream_abort_locked(c);
        return fail(c, TV_ERR_ARG, "%s is NULL", v1 && !digests_out ? "digests_out" : "roots_out");
    }
    if (!c->count) {
        c->last_stream_requests = st.seq;   // (an empty shard: 0)
        st = StreamState{};
        return TV_OK;
    }
    std::vector<uint32_t> soa1(v1 ? 5 * c->count : 0), soa2(v2 ? v2s_hash_words(c->count) : 0);
    int rc;
    {
        DrainGuard drain(c);  // declared after the vectors: their copies end before they go, also on error paths
        rc = [&]() -> int {
            TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
            if (v1)
                TV_HIP(c, hipMemcpyAsync(soa1.data(), c->d_hash, soa1.size() * 4, hipMemcpyDeviceToHost, c->stream));
            if (v2)
                TV_HIP(c, hipMemcpyAsync(soa2.data(), c->d_v2s_tab.get<uint32_t>() + v2s_hash_base(c->count, 0),
                                         soa2.size() * 4, hipMemcpyDeviceToHost, c->stream));
            TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
            TV_HIP(c, hipEventSynchronize(c->ev_call1));
            return TV_OK;
        }();
    }
    if (rc) {
        stream_abort_locked(c);
        return rc;
    }
    for (uint64_t j = 0; j < c->count; j++) {
        if (v1) digest_unpack(soa1.data(), c->count, j, 5, digests_out + 20 * j);
        if (v2) {   // the window's own [8][wcount] rows
            const uint64_t j0 = j / st.wn * st.wn, wcount = std::min(st.wn, c->count - j0);
            digest_unpack(soa2.data() + v2s_hash_word(c->count, st.wn, j0, 0), wcount, j - j0, 8, roots_out + 32 * j);
        }
    }
    c->last_kernel = st.kernel;
    c->last_launches = st.launches;
    rc = finish_timing(c);
    c->last_stream_requests = st.seq;
    st = StreamState{};
    return rc;
}

// Public stream calls: a HIP failure leaves the stream unusable, so it is aborted (the ctx stays usable).
int stream_result(tv_ctx* c, int rc) {
    if (rc == TV_ERR_HIP || rc == TV_ERR_NOMEM) stream_abort_locked(c);
    return rc;
}

// ---- the library's own readers as the producer (tv_stream_file_table and its v2 and hybrid forms), in parts ----------
// File k's bytes are the LINEAR bytes [start[k], start[k] + lengths[k]) (v1: the files back to back; v2: every file at
// the next piece boundary, tv_plan.h v2_file_starts).

// Whether the shard's files are mostly not in the page cache (TV_OPT_FILE_ODIRECT): up to 16 of the files holding
// >= 1 MiB of its bytes, evenly spread, each sampled as the staging path samples a unit (64 pages), weighted by
// bytes.  A cold shard is read in longer rows (fewer pieces per window) by more readers: O_DIRECT reads wait on
// the disk, which wants long requests and many in flight (profiles/r06/window_bench_cold_cols*.jsonl).
static bool shard_is_cold(const tv_ctx* c, uint64_t n, const uint64_t* lengths, const std::vector<const char*>& path,
                          const std::vector<uint64_t>& start) {
    if (!c->file_odirect) return false;
    uint64_t lo, hi;
    shard_bytes(c, /*clamp_total=*/true, &lo, &hi);
    std::vector<uint64_t> big;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t a = std::max(lo, start[k]), b = std::min(hi, start[k] + lengths[k]);
        if (b > a && b - a >= (1u << 20) && path[k][0]) big.push_back(k);
    }
    double hit = 0, all = 0;
    const size_t m = std::min<size_t>(16, big.size());
    for (size_t q = 0; q < m; q++) {
        const uint64_t k = big[q * big.size() / m];
        const uint64_t a = std::max(lo, start[k]), b = std::min(hi, start[k] + lengths[k]);
        // (nonblocking: a FIFO in the table must not hang the sample; only regular files are sampled)
        const int fd = open(path[k], O_RDONLY | O_NONBLOCK | O_CLOEXEC);
        if (fd < 0) continue;
        struct stat sb;
        const double f = fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) ? cached_fraction(fd, a - start[k], b - a) : -1;
        close(fd);
        if (f < 0) continue;
        hit += f * (double)(b - a);
        all += (double)(b - a);
    }
    return all > 0 && hit < 0.5 * all;
}

// The call's open files: the first kCachedFds opened stay open until the end (a one- or few-file torrent opens each
// once); past that a reader opens and closes the file around its read (as fsStorage.get does per call), so a
// 10,000-file torrent never runs into the descriptor limit.  -2: the open failed.  A cached file whose pages are mostly
// not in the page cache at its open (64 sampled pages, TV_OPT_FILE_ODIRECT) is also opened O_DIRECT: its rows are read
// past the page cache (dfds; -1 none, and a file whose O_DIRECT read the filesystem refuses reads buffered from then
// on: no_direct).
struct FdCache {
    static constexpr int kCachedFds = 256;
    const tv_ctx* c;
    const uint64_t* lengths;
    const std::vector<const char*>& path;
    std::vector<int> fds, dfds;
    std::unique_ptr<std::atomic<bool>[]> no_direct;
    int cached = 0;
    std::mutex mu;
    const bool rw;   // TV_OPT_OPEN_RW; a creation call's readers always open read-only (make_torrent.ts:78)
    FdCache(const tv_ctx* c, uint64_t n, const uint64_t* lengths, const std::vector<const char*>& path, bool read_only)
        : c(c), lengths(lengths), path(path), fds(n, -1), dfds(n, -1), no_direct(new std::atomic<bool>[n ? n : 1]()),
          rw(c->open_rw && !read_only) {}
    ~FdCache() {
        for (int x : fds)
            if (x >= 0) close(x);
        for (int x : dfds)
            if (x >= 0) close(x);
    }
    // (under mu) file k's cached descriptor, -2, or -1 = not opened yet; *dfd: its O_DIRECT one while in use
    int cached_fd(uint64_t k, int* dfd) const {
        if (dfds[k] >= 0 && !no_direct[k].load(std::memory_order_relaxed)) *dfd = dfds[k];
        return fds[k];
    }
    // -> a descriptor of file k, and whether the caller closes it after its read (*dfd as above, or -1)
    int fd_of(uint64_t k, bool* own, int* dfd) {
        *own = false;
        *dfd = -1;
        {
            std::lock_guard<std::mutex> fg(mu);
            if (fds[k] != -1) return cached_fd(k, dfd);
        }
        int e = 0;
        const int d = path[k][0] ? open_file(path[k], rw, &e) : -1;
        std::lock_guard<std::mutex> fg(mu);
        if (fds[k] != -1) {   // another reader opened it meanwhile
            if (d >= 0) close(d);
            return cached_fd(k, dfd);
        }
        if (d < 0) {
            if (e != EMFILE && e != ENFILE) fds[k] = -2;   // (out of descriptors: not the file's failure, but unread)
            return -1;
        }
        if (cached < kCachedFds) {
            cached++;
            fds[k] = d;
            if (c->file_odirect && lengths[k] >= (1u << 20)) {
                if (is_cold(cached_fraction(d, 0, lengths[k]))) dfds[k] = open_direct(path[k], rw);
                if (dfds[k] >= 0) *dfd = dfds[k];
            }
            return d;
        }
        *own = true;
        return d;
    }
};

// `len` bytes of file k from byte `fo` into dst (a ring slot): O_DIRECT first where the file has such a descriptor, the
// rest buffered.  -> the bytes read (< len: missing, unopenable or short, as fsStorage.get's read).
static uint64_t read_segment(tv_ctx* c, FdCache& files, uint64_t k, uint64_t fo, uint8_t* dst, uint64_t len) {
    bool own = false;
    int dfd = -1;
    const int fd = files.fd_of(k, &own, &dfd);
    uint64_t o = 0;
    if (dfd >= 0) {
        const int64_t got = c->file_odirect == 2 ? -EINVAL   // (fault injection: O_DIRECT reads refused)
                                                 : read_direct(dfd, fo, dst, len);
        if (got >= 0) {
            o = (uint64_t)got;
            c->file_ns[TV_FILE_BYTES_ODIRECT].fetch_add(o, std::memory_order_relaxed);
        } else {
            // an O_DIRECT read the filesystem refuses is not the file's failure: this file reads buffered from here
            // on, this segment included (counted, first errno kept, as the staging path's fallback)
            files.no_direct[k].store(true, std::memory_order_relaxed);
            odirect_refused(c, (int)-got);
        }
    }
    if (fd >= 0 && o < len) {   // (a failed read's bytes so far still count as read)
        uint64_t in = 0;
        read_at(fd, dst + o, fo + o, len - o, len - o, &in);
        o += in;
    }
    if (own) close(fd);
    c->file_ns[TV_FILE_BYTES_READ].fetch_add(o, std::memory_order_relaxed);
    return o;
}

// The reader loop: begin(cold) starts the stream (its geometry and availability are the caller's) once the shard's files
// are known to be mostly in the page cache or not.  The lane-0 pool fills each request's ring slot: a row's bytes
// (stream_row_bytes) are walked over the file table (tv_plan.h walk_row_files) and read segment by segment; a row that
// a missing, unopenable or short file cannot fill makes its piece unreadable and the file's status TV_ERR_IO.  end():
// the stream's end call, which hands the results out.  hash: a creation call -- the files are opened read-only, and a
// row that cannot be filled ends the call (creation cannot skip a piece): TV_ERR_IO after the statuses are set, the
// stream aborted, end() never called.
int stream_files_locked(tv_ctx* c, uint64_t n, const uint64_t* lengths, const std::vector<const char*>& path,
                        const std::vector<uint64_t>& start, const std::function<int(bool)>& begin,
                        int32_t* status_out, const std::function<int()>& end, bool hash = false) {
    const bool cold = shard_is_cold(c, n, lengths, path, start);
    FdCache files(c, n, lengths, path, hash);
    const int readers = cold ? (c->stream_cold_readers ? c->stream_cold_readers : 2 * c->file_threads) : c->file_threads;
    DrainGuard drain(c);  // (the ring's copies and the column kernels are done when the call returns)
    int rc = begin(cold);
    if (rc) {
        stream_abort_locked(c);
        return rc;
    }
    std::vector<std::atomic<int32_t>> file_err(n);
    for (auto& e : file_err) e.store(TV_OK);
    bool unread = false;   // a row could not be filled
    for (;;) {
        tv_stream_req req;
        rc = stream_next_locked(c, &req);
        if (rc || !req.rows) break;
        uint8_t* slot = c->ring[c->st.slot];
        std::vector<uint8_t> row_bad(req.rows, 0);
        c->pool[0].run(readers, req.rows, [&](uint64_t q) {
            const uint64_t i = req.piece + q, j = i - c->first;
            const uint64_t nb = stream_row_bytes(c, i, req.offset, req.width);
            if (!nb || !get_bit(c->st.av.data(), j)) return;
            const uint64_t a = i * c->L + req.offset;   // the row's linear bytes: [a, a + nb)
            uint8_t* out = slot + q * req.width;
            const RowWalk w = walk_row_files(start.data(), lengths, n, a, a + nb,
                                             [&](uint64_t k, uint64_t fo, uint64_t at, uint64_t len) {
                if (read_segment(c, files, k, fo, out + at, len) == len) return true;
                file_err[k].store(TV_ERR_IO);   // missing, unopenable or short: the piece is null, as fsStorage.get's
                return false;
            });
            // (kRowGap: a row reaching into the gap after a file, its table and files disagree; no file's status)
            if (w != kRowWalked) row_bad[q] = 1;
        });
        for (uint64_t q = 0; q < req.rows; q++)
            if (row_bad[q]) {
                clear_bit(c->st.av.data(), req.piece + q - c->first);
                unread = true;
            }
        if (hash && unread) break;   // (the lent slot goes back with the abort)
        rc = stream_commit_locked(c, &req, nullptr, 0, true, req.rows);
        if (rc) break;
    }
    for (uint64_t k = 0; k < n; k++)
        if (file_err[k].load() != TV_OK) status_out[k] = TV_ERR_IO;
    if (rc) {
        stream_abort_locked(c);
        return rc;
    }
    if (hash && unread) {
        stream_abort_locked(c);
        return fail(c, TV_ERR_IO, "a file is missing, unopenable or shorter than its declared length (status_out); "
                                  "nothing was hashed out");
    }
    return end();
}

// What tv_v2_stream_begin and tv_hybrid_stream_begin (and their file-table forms) check before anything changes: the
// layout, the GLOBAL piece table and its hashes; a hybrid stream also needs the digests (TV_ERR_STATE) and a layout that
// is the v1 space of the table: piece_bytes <= v1_len for every shard piece (tv_hybrid_verify's rule and text).
// hash: the creation forms (tv_v2_stream_hash_begin, tv_hybrid_stream_hash_begin) need neither digests nor hashes.
int v2_stream_check(tv_ctx* c, bool hybrid, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                    const uint8_t* hashes, bool hash = false) {
    const char* what = hybrid ? (hash ? "tv_hybrid_stream_hash_begin" : "tv_hybrid_stream_begin") : "tv_v2_stream_begin";
    int rc = require_layout(c, hybrid && !hash);
    if (rc) return rc;
    rc = v2_check_table(c, n, piece_bytes, tree_leaves);
    if (rc) return rc;
    if (n && !hashes && !hash) return fail(c, TV_ERR_ARG, "NULL argument");
    if (hash && c->win)
        return fail(c, TV_ERR_STATE, "a creation stream needs a layout without windows (TV_OPT_RESIDENT = 0)");
    if (!hybrid) return TV_OK;
    if (c->L > kHybridMaxL)
        return fail(c, TV_ERR_ARG, "%s takes piece lengths up to %llu bytes (the layout has %llu)", what,
                    (unsigned long long)kHybridMaxL, (unsigned long long)c->L);
    for (uint64_t i = c->first; i < c->first + c->count; i++)
        if (piece_bytes[i] > hybrid_v1_len(c->total, c->L, i))
            return fail(c, TV_ERR_ARG, "%s: piece_bytes[%llu] = %llu exceeds the piece's v1 length %llu (total_length "
                                       "%llu): the layout is not the v1 space of these pieces", what,
                        (unsigned long long)i, (unsigned long long)piece_bytes[i],
                        (unsigned long long)hybrid_v1_len(c->total, c->L, i), (unsigned long long)c->total);
    return TV_OK;
}

int v2_stream_begin_call(tv_ctx* c, bool hybrid, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                         const uint8_t* hashes, const uint8_t* avail_bits, bool hash = false) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = v2_stream_check(c, hybrid, n, piece_bytes, tree_leaves, hashes, hash);
    if (rc) return rc;
    TV_HIP(c, hipSetDevice(c->device));
    rc = v2_stream_begin_locked(c, piece_bytes, tree_leaves, hashes, avail_bits, 0, hybrid, hash);
    if (rc) c->st = StreamState{};   // (a failed begin leaves no stream, v2 or other)
    return rc;
}

// tv_v2_stream_file_table / tv_hybrid_stream_file_table: tv_stream_file_table's reader loop over the ALIGNED file table
// (every file starts a piece), the rows ending with their piece's bytes.  A v2 piece lies in one file, so it is
// unreadable exactly when that file cannot supply its bytes; there are no zero-length segments to open, and a hybrid
// torrent's pad files are not in the table: they are never opened or looked for.  hash: the creation forms
// (tv_v2_stream_hash_file_table, tv_hybrid_stream_hash_file_table): the same table checks, no hashes and no
// availability, the outputs tv_stream_hash_end's.
int v2_stream_files_call(tv_ctx* c, bool hybrid, uint64_t n_pieces, const uint32_t* piece_bytes,
                         const uint32_t* tree_leaves, const uint8_t* hashes, uint64_t n, const uint64_t* lengths,
                         const char* paths, uint64_t paths_bytes, const uint8_t* avail_bits, uint8_t* v1_out,
                         uint8_t* v2_out, uint8_t* bitfield_out, int32_t* status_out, bool hash = false,
                         uint8_t* digests_out = nullptr, uint8_t* roots_out = nullptr) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = v2_stream_check(c, hybrid, n_pieces, piece_bytes, tree_leaves, hashes, hash);
    if (rc) return rc;
    if (!hash && !bitfield_out && c->count) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    if (hash && c->count && (!roots_out || (hybrid && !digests_out)))
        return fail(c, TV_ERR_ARG, "%s is NULL", !roots_out ? "roots_out" : "digests_out");
    if (n && (!lengths || !paths || !status_out)) return fail(c, TV_ERR_ARG, "NULL argument");
    std::vector<const char*> path(n);
    const uint64_t np = parse_path_table(n, paths, paths_bytes, path.data());
    if (np < n) return path_error(c, np, paths_bytes, n);
    std::vector<uint64_t> start;   // file k's linear bytes: [start[k], start[k] + lengths[k])
    uint64_t bad = 0;
    if (!v2_file_starts(n, lengths, c->L, &start, &bad))
        return fail(c, TV_ERR_ARG, "file %llu: the lengths overflow 64-bit offsets", (unsigned long long)bad);
    if (start[n] / c->L != n_pieces)
        return fail(c, TV_ERR_ARG, "the files hold %llu pieces, the piece table %llu", (unsigned long long)(start[n] / c->L),
                    (unsigned long long)n_pieces);
    // every piece's bytes are its file's (so a row never reaches past its file into the gap before the next one)
    for (uint64_t k = 0; k < n; k++)
        for (uint64_t p = start[k] / c->L, o = 0; o < lengths[k]; p++, o += c->L)
            if (piece_bytes[p] != std::min<uint64_t>(c->L, lengths[k] - o))
                return fail(c, TV_ERR_ARG, "piece_bytes[%llu] = %llu, but file %llu holds %llu bytes of that piece",
                            (unsigned long long)p, (unsigned long long)piece_bytes[p], (unsigned long long)k,
                            (unsigned long long)std::min<uint64_t>(c->L, lengths[k] - o));
    for (uint64_t k = 0; k < n; k++) status_out[k] = TV_OK;
    if (!c->count) return TV_OK;
    TV_HIP(c, hipSetDevice(c->device));
    rc = stream_files_locked(c, n, lengths, path, start, [&](bool cold) {
        return v2_stream_begin_locked(c, piece_bytes, tree_leaves, hashes, avail_bits, cold ? c->stream_cold_req : 0, hybrid,
                                      hash);
    }, status_out, [&] {
        return hash ? stream_hash_end_locked(c, digests_out, roots_out) : stream_end_locked(c, bitfield_out, v1_out, v2_out);
    }, hash);
    if (rc && !c->st.active) c->st = StreamState{};
    return rc;
}

}  // namespace tvi

using namespace tvi;

extern "C" {

// End-to-end verification from a host buffer holding the whole shard (tv_verify_host): the stream engine
// with the caller's buffer as the producer.  Each request's rows are one 2D DMA straight from a page-locked
// source (src pitch L) or are gathered into the request's ring slot first.  Rows past src_len are not
// copied; their pieces are unreadable.
int tv_verify_host(tv_ctx* c, const uint8_t* src, uint64_t src_len, const uint8_t* avail_bits,
                   uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, true);
    if (rc) return rc;
    if (!bitfield_out && c->count) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    if (!src && src_len) return fail(c, TV_ERR_ARG, "src is NULL");
    if (!c->count) return TV_OK;
    TV_HIP(c, hipSetDevice(c->device));
    // pieces whose bytes extend past src_len are unreadable
    std::vector<uint8_t> av((c->count + 7) / 8, 0);
    for (uint64_t j = 0; j < c->count; j++) {
        const uint64_t end = j * c->L + piece_len(c, c->first + j);
        if (end <= src_len && (!avail_bits || get_bit(avail_bits, j))) set_bit(av.data(), j);
    }
    const bool pinned = is_pinned(src);
    uint64_t col = 0, win = 0;   // windows x columns within the device budget (or 1 GiB), unless a width is set
    if (!c->stream_chunk && !stream_rows(c))
        budget_geometry(c, c->budget_opt ? c->budget_opt : (1ull << 30), 2048, &col, &win);
    DrainGuard drain(c);  // no DMA reads the caller's buffer after the call returns, also on error paths
    rc = stream_begin_locked(c, av.data(), col, win);
    if (rc) {
        stream_abort_locked(c);
        return rc;
    }
    for (;;) {
        tv_stream_req req;
        rc = stream_next_locked(c, &req);
        if (rc || !req.rows) break;
        // rows wholly inside src: a prefix of the request (its rows ascend in linear offset)
        const uint64_t base = (req.piece - c->first) * c->L + req.offset;
        uint64_t k = 0;
        while (k < req.rows && base + k * c->L + stream_row_bytes(c, req.piece + k, req.offset, req.width) <= src_len) k++;
        rc = stream_commit_locked(c, &req, k ? src + base : nullptr, c->L, pinned, k);
        if (rc) break;
    }
    if (rc) {
        stream_abort_locked(c);
        return rc;
    }
    return stream_end_locked(c, bitfield_out);
}

// The resume check from FILES through the bounded ring (tv_stream_file_table): the stream engine with the library's
// own readers as the producer.  Each request's rows (bytes [offset, offset + width) of consecutive pieces: a column
// across the shard) are read by the lane-0 pool straight from the files into the request's ring slot, each row's
// linear range walked over the file table as Storage.get walks it (storage.ts:98-137); the kernels hash one column
// while the next is read.  Device memory: two columns (TV_OPT_STREAM_CHUNK bytes of every shard piece), so a shard
// verifies under a small device budget with every piece's SHA-1 advancing at once, where windows of whole pieces
// pay one piece's serial SHA-1 per window.  A piece is unreadable exactly when fsStorage.get would return null
// for it: a byte of it in a missing, unopenable or too-short file, a zero-length segment of its walk whose open
// fails (storage.ts:109-110,158), or bytes past the files' end.  Files are opened as fsStorage.get opens them
// (TV_OPT_OPEN_RW), kept open for the call, never created.
//
// hash (tv_stream_hash_file_table): the creation stream over the same readers.  No digests, no availability; the files
// are opened read-only (make_torrent.ts:78), and a byte of the shard that cannot be read ends the call with TV_ERR_IO.
static int v1_stream_files_call(tv_ctx* c, uint64_t n, const uint64_t* lengths, const char* paths, uint64_t paths_bytes,
                                const uint8_t* avail_bits, uint8_t* bitfield_out, int32_t* status_out, bool hash,
                                uint8_t* digests_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, !hash);
    if (rc) return rc;
    if (!hash && !bitfield_out && c->count) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    if (hash && !digests_out && c->count) return fail(c, TV_ERR_ARG, "digests_out is NULL");
    if (hash && c->win)
        return fail(c, TV_ERR_STATE, "a creation stream needs a layout without windows (TV_OPT_RESIDENT = 0)");
    if (n && (!lengths || !paths || !status_out)) return fail(c, TV_ERR_ARG, "NULL argument");
    std::vector<const char*> path(n);
    std::vector<uint64_t> start(n + 1, 0);   // file k's linear bytes: [start[k], start[k + 1])
    const uint64_t np = parse_path_table(n, paths, paths_bytes, path.data());
    for (uint64_t k = 0; k < n; k++) {
        if (k == np) return path_error(c, np, paths_bytes, n);
        if (lengths[k] > UINT64_MAX - start[k])
            return fail(c, TV_ERR_ARG, "file %llu: the lengths overflow 64-bit offsets", (unsigned long long)k);
        start[k + 1] = start[k] + lengths[k];
        status_out[k] = TV_OK;
    }
    if (!c->count) return TV_OK;
    TV_HIP(c, hipSetDevice(c->device));
    uint64_t lo, hi;
    shard_bytes(c, /*clamp_total=*/true, &lo, &hi);
    // availability before any read: the caller's bits, pieces past the files' end, and the pieces whose walk has a
    // zero-length segment whose open fails (the same segments tv_stage_file_table checks)
    std::vector<uint8_t> av((c->count + 7) / 8, 0);
    for (uint64_t j = 0; j < c->count; j++) {
        const uint64_t i = c->first + j, end = i * c->L + piece_len(c, i);
        if (end <= std::min(c->total, start[n]) && (!avail_bits || get_bit(avail_bits, j))) set_bit(av.data(), j);
    }
    {
        std::vector<TableSeg> segs;
        uint64_t bad = 0, reached = 0;
        if (!walk_file_table(n, lengths, lo, hi, c->L, &segs, &bad, &reached))
            return fail(c, TV_ERR_ARG, "file %llu: the lengths overflow 64-bit offsets", (unsigned long long)bad);
        for (const TableSeg& sg : segs) {
            if (sg.len || sg.linear < lo || sg.linear >= hi) continue;
            if (fs_openable(path[sg.file], c->open_rw && !hash)) {
                status_out[sg.file] = TV_ERR_IO;
                clear_bit(av.data(), sg.linear / c->L - c->first);
            }
        }
    }
    if (hash)   // creation cannot skip a piece: the files end before the shard does, or a zero-length file does not open
        for (uint64_t j = 0; j < c->count; j++)
            if (!get_bit(av.data(), j))
                return fail(c, TV_ERR_IO, "piece %llu cannot be read: the files end before it does, or a zero-length "
                                          "file of its range cannot be opened", (unsigned long long)(c->first + j));
    // Geometry: windows x columns within the budget (TV_OPT_RESIDENT_BUDGET, or 1 GiB); a cold shard's windows are
    // 512 pieces (rows 4 x longer; ~44 GB/s of hashing, above what the disk gives).  An explicit TV_OPT_STREAM_CHUNK
    // keeps the engine's columns across the whole shard.
    return stream_files_locked(c, n, lengths, path, start, [&](bool cold) {
        uint64_t col = 0, win = 0;
        if (!c->stream_chunk) {
            const uint64_t min_win = cold ? (c->stream_cold_window ? c->stream_cold_window : 512) : 2048;
            budget_geometry(c, c->budget_opt ? c->budget_opt : (1ull << 30), min_win, &col, &win);
        }
        return stream_begin_locked(c, av.data(), col, win, cold ? c->stream_cold_req : 0, hash);
    }, status_out, [&] {
        return hash ? stream_hash_end_locked(c, digests_out, nullptr) : stream_end_locked(c, bitfield_out);
    }, hash);
}

int tv_stream_file_table(tv_ctx* c, uint64_t n, const uint64_t* lengths, const char* paths, uint64_t paths_bytes,
                         const uint8_t* avail_bits, uint8_t* bitfield_out, int32_t* status_out) {
    return v1_stream_files_call(c, n, lengths, paths, paths_bytes, avail_bits, bitfield_out, status_out, false, nullptr);
}

int tv_stream_hash_file_table(tv_ctx* c, uint64_t n, const uint64_t* lengths, const char* paths, uint64_t paths_bytes,
                              uint8_t* digests_out, int32_t* status_out) {
    return v1_stream_files_call(c, n, lengths, paths, paths_bytes, nullptr, nullptr, status_out, true, digests_out);
}

// Creation streams (tv_stream_hash_begin and its v2 and hybrid forms): the verify stream of the same kind -- its
// geometry, ring, requests and launches -- whose last launches store what the resident creation calls compute
// (make_torrent.ts:18-113,147-173 is the reference's streaming creator).  They need no digests, no expected roots and
// no availability; tv_stream_hash_end hands the hashes out.
int tv_stream_hash_begin(tv_ctx* c) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, false);
    if (rc) return rc;
    if (c->win) return fail(c, TV_ERR_STATE, "a creation stream needs a layout without windows (TV_OPT_RESIDENT = 0)");
    TV_HIP(c, hipSetDevice(c->device));
    return stream_result(c, stream_begin_locked(c, nullptr, 0, 0, 0, true));
}

int tv_v2_stream_hash_begin(tv_ctx* c, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves) {
    return v2_stream_begin_call(c, false, n, piece_bytes, tree_leaves, nullptr, nullptr, true);
}

int tv_hybrid_stream_hash_begin(tv_ctx* c, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves) {
    return v2_stream_begin_call(c, true, n, piece_bytes, tree_leaves, nullptr, nullptr, true);
}

int tv_stream_hash_end(tv_ctx* c, uint8_t* digests_out, uint8_t* roots_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    TV_HIP(c, hipSetDevice(c->device));
    return stream_hash_end_locked(c, digests_out, roots_out);
}

int tv_v2_stream_hash_file_table(tv_ctx* c, uint64_t n_pieces, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                                 uint64_t n, const uint64_t* lengths, const char* paths, uint64_t paths_bytes,
                                 uint8_t* roots_out, int32_t* status_out) {
    return v2_stream_files_call(c, false, n_pieces, piece_bytes, tree_leaves, nullptr, n, lengths, paths, paths_bytes,
                                nullptr, nullptr, nullptr, nullptr, status_out, true, nullptr, roots_out);
}

int tv_hybrid_stream_hash_file_table(tv_ctx* c, uint64_t n_pieces, const uint32_t* piece_bytes,
                                     const uint32_t* tree_leaves, uint64_t n, const uint64_t* lengths, const char* paths,
                                     uint64_t paths_bytes, uint8_t* digests_out, uint8_t* roots_out, int32_t* status_out) {
    return v2_stream_files_call(c, true, n_pieces, piece_bytes, tree_leaves, nullptr, n, lengths, paths, paths_bytes,
                                nullptr, nullptr, nullptr, nullptr, status_out, true, digests_out, roots_out);
}

int tv_stream_begin(tv_ctx* c, const uint8_t* avail_bits) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, true);
    if (rc) return rc;
    TV_HIP(c, hipSetDevice(c->device));
    return stream_result(c, stream_begin_locked(c, avail_bits));
}

int tv_v2_stream_begin(tv_ctx* c, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                       const uint8_t* hashes, const uint8_t* avail_bits) {
    return v2_stream_begin_call(c, false, n, piece_bytes, tree_leaves, hashes, avail_bits);
}

int tv_hybrid_stream_begin(tv_ctx* c, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                           const uint8_t* hashes, const uint8_t* avail_bits) {
    return v2_stream_begin_call(c, true, n, piece_bytes, tree_leaves, hashes, avail_bits);
}

int tv_v2_stream_file_table(tv_ctx* c, uint64_t n_pieces, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                            const uint8_t* hashes, uint64_t n, const uint64_t* lengths, const char* paths,
                            uint64_t paths_bytes, const uint8_t* avail_bits, uint8_t* bitfield_out,
                            int32_t* status_out) {
    return v2_stream_files_call(c, false, n_pieces, piece_bytes, tree_leaves, hashes, n, lengths, paths, paths_bytes,
                                avail_bits, nullptr, nullptr, bitfield_out, status_out);
}

int tv_hybrid_stream_file_table(tv_ctx* c, uint64_t n_pieces, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                                const uint8_t* hashes, uint64_t n, const uint64_t* lengths, const char* paths,
                                uint64_t paths_bytes, const uint8_t* avail_bits, uint8_t* v1_bits_out,
                                uint8_t* v2_bits_out, uint8_t* bitfield_out, int32_t* status_out) {
    return v2_stream_files_call(c, true, n_pieces, piece_bytes, tree_leaves, hashes, n, lengths, paths, paths_bytes,
                                avail_bits, v1_bits_out, v2_bits_out, bitfield_out, status_out);
}

int tv_stream_next(tv_ctx* c, tv_stream_req* req) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    if (!req) return fail(c, TV_ERR_ARG, "req is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    TV_HIP(c, hipSetDevice(c->device));
    return stream_result(c, stream_next_locked(c, req));
}

int tv_stream_commit(tv_ctx* c, const tv_stream_req* req) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    TV_HIP(c, hipSetDevice(c->device));
    return stream_result(c, stream_commit_locked(c, req, nullptr, 0, true, req ? req->rows : 0));
}

int tv_stream_commit_from(tv_ctx* c, const tv_stream_req* req, const uint8_t* src, uint64_t src_pitch) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    if (!src) return fail(c, TV_ERR_ARG, "src is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    if (req && req->rows > 1 && src_pitch < req->width)
        return fail(c, TV_ERR_ARG, "src_pitch %llu is shorter than the row width %llu", (unsigned long long)src_pitch,
                    (unsigned long long)req->width);
    TV_HIP(c, hipSetDevice(c->device));
    return stream_result(c, stream_commit_locked(c, req, src, src_pitch, is_pinned(src), req ? req->rows : 0));
}

int tv_stream_unreadable(tv_ctx* c, uint64_t piece) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->st.active) return no_stream(c, "tv_stream_begin has not been called");
    if (c->st.hash)   // (the stream stays active: tv_stream_abort gives it up)
        return fail(c, TV_ERR_STATE, "tv_stream_unreadable: a creation stream cannot skip a piece");
    if (piece < c->first || piece >= c->first + c->count)
        return fail(c, TV_ERR_ARG, "piece %llu is not in this context's shard", (unsigned long long)piece);
    clear_bit(c->st.av.data(), piece - c->first);
    return TV_OK;
}

int tv_stream_end(tv_ctx* c, uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    TV_HIP(c, hipSetDevice(c->device));
    return stream_end_locked(c, bitfield_out);
}

int tv_hybrid_stream_end(tv_ctx* c, uint8_t* v1_bits_out, uint8_t* v2_bits_out, uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    if (c->st.active && !c->st.hybrid && !c->st.hash)   // (the stream stays active: tv_stream_end ends it; a creation
                                                         // stream is refused and aborted by stream_end_locked)
        return fail(c, TV_ERR_STATE, "tv_hybrid_stream_end: the active stream is not a hybrid stream");
    TV_HIP(c, hipSetDevice(c->device));
    return stream_end_locked(c, bitfield_out, v1_bits_out, v2_bits_out);
}

int tv_stream_abort(tv_ctx* c) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    TV_HIP(c, hipSetDevice(c->device));
    stream_abort_locked(c);
    return TV_OK;
}

int tv_stream_fill_synthetic(tv_ctx* c, const tv_stream_req* req, uint64_t seed) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    const StreamState& st = c->st;
    if (!st.active || !st.outstanding) return no_stream(c, "no outstanding request (call tv_stream_next)");
    if (!req || req->seq != st.req.seq) return fail(c, TV_ERR_ARG, "the request does not match the outstanding one");
    const tv_stream_req r = st.req;
    uint8_t* slot = c->ring[st.slot];
    c->pool[0].run(c->file_threads, r.rows, [&](uint64_t q) {
        const uint64_t i = r.piece + q;
        tv_synth_fill_host(seed, i * c->L + r.offset, stream_row_bytes(c, i, r.offset, r.width), slot + q * r.width);
    });
    return TV_OK;
}

}  // extern "C"
