// tv_hybrid.hip -- hybrid torrents (BEP 52 with the v1 keys, BEP 47 pad files): both descriptions of one payload
// checked, or created, from ONE staging (tv_hybrid_verify, tv_hybrid_hash).  In a hybrid torrent every file starts a
// piece, so the v1 linear space is the aligned space of the layout: v1 piece i is v2 piece i's piece_bytes[i] file bytes
// followed by the pad file's zeros out to v1_len(i).  tv_hybrid_pad_kernel writes those zeros into the resident rows
// (one launch over the shard's tail table, tv_plan.h hybrid_tails); then the SHA-1 launch of tv_verify / tv_hash and
// the launch set of tv_v2_verify / tv_v2_hash run over the same rows.  A hybrid STREAM (tv_stream.hip) zeroes the pad
// ranges of each unit's chunk buffer with tv_hybrid_col_pad_kernel instead.  tv_hybrid_verify_list checks completed
// pieces on a slot pool (or a resident shard): tv_hybrid_list_pad_kernel over the listed rows, then the launch parts of
// tv_verify_list and tv_v2_verify_list (tv_ctx.h V1List / V2List), one wait.
#include <cstring>

#include "tv_ctx.h"

using namespace tvi;

// ------------------------------------------------------------------------------------------
// pad kernel: workgroup g zeroes chunk g of the launch (tv_plan.h: chunk k of tail entry e is the bytes of the row's
// [begin, end) inside [a0 + k * kHybridChunk, a0 + (k + 1) * kHybridChunk), a0 = begin & ~15).  The entry of a chunk is
// found by a search over the entries' chunk0 (ascending; at most log2(n) + 1 steps, the same in every lane).  Byte
// stores up to the first 16-byte aligned ADDRESS (whatever the stride makes of the row base), uint4 stores from there,
// byte stores for what is left before `end`: nothing below begin, nothing at or past end.
// ------------------------------------------------------------------------------------------
namespace {

struct TvHybridPad {
    uint8_t* data;
    uint64_t stride;
    const HybridTail* tails;
    uint32_t n;        // entries
    uint32_t chunks;   // workgroups
    uint32_t rows;     // rows of the payload (a tail outside them is skipped: never a store out of bounds)
    uint32_t L;        // no tail ends past it
};

__global__ __launch_bounds__(256) void tv_hybrid_pad_kernel(TvHybridPad p) {
    const uint32_t g = blockIdx.x;
    if (g >= p.chunks || p.n == 0) return;
    const HybridTail t = p.tails[hybrid_chunk_entry(p.tails, p.n, g)];
    uint64_t b, e;
    if (t.row >= p.rows || t.end > p.L || !hybrid_chunk_range(t, g, &b, &e)) return;
    const uint64_t row = reinterpret_cast<uint64_t>(p.data) + (uint64_t)t.row * p.stride;
    const uint64_t pb = row + b, pe = row + e;
    uint64_t va, ve;
    hybrid_split(pb, pe, &va, &ve);
    const uint32_t tid = threadIdx.x;
    if (pb + tid < va) *reinterpret_cast<uint8_t*>(pb + tid) = 0;   // (at most 15 bytes)
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t q = va + 16ull * tid; q < ve; q += 16ull * 256) *reinterpret_cast<uint4*>(q) = z;
    if (ve + tid < pe) *reinterpret_cast<uint8_t*>(ve + tid) = 0;   // (at most 15 bytes)
}

hipError_t launch_pad(const TvHybridPad& p, hipStream_t s) {
    if (p.n == 0 || p.chunks == 0) return hipSuccess;
    if (p.chunks > 0x7FFFFFFFu) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(tv_hybrid_pad_kernel, dim3(p.chunks), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// column pad kernel (a hybrid stream's unit: window rows [j0, j0 + rows) x column [offset, offset + C) of a chunk buffer
// of row pitch C + 256).  Workgroup (x = row, y = chunk) derives the row's range itself -- its piece bytes from the
// stream's piece table on the device, its v1 length from the layout (tv_plan.h hybrid_col_chunk) -- so a unit needs no
// table of its own and no copy.  A row with an empty range, and a chunk outside it, return at once.  The stores are the
// pad kernel's: bytes, uint4 from the first 16-byte aligned address, bytes; nothing below b, nothing at or past e
// (e <= C < the pitch), nothing in a row outside the unit.
// ------------------------------------------------------------------------------------------
struct TvHybridColPad {
    uint8_t* data;
    uint64_t pitch;
    const uint32_t* piece_bytes;   // of the unit's rows (the stream's table from piece j0 on)
    uint64_t total, L;             // the layout: v1_len(i) = min(L, total - i * L)
    uint64_t piece0;               // GLOBAL piece of row 0
    uint64_t offset, C;            // the column
    uint32_t rows;
};

__global__ __launch_bounds__(256) void tv_hybrid_col_pad_kernel(TvHybridColPad p) {
    const uint32_t r = blockIdx.x;
    if (r >= p.rows) return;
    uint64_t b, e;
    if (!hybrid_col_chunk(p.piece_bytes[r], p.total, p.L, p.piece0 + r, p.offset, p.C, blockIdx.y, &b, &e)) return;
    const uint64_t row = reinterpret_cast<uint64_t>(p.data) + (uint64_t)r * p.pitch;
    const uint64_t pb = row + b, pe = row + e;
    uint64_t va, ve;
    hybrid_split(pb, pe, &va, &ve);
    const uint32_t tid = threadIdx.x;
    if (pb + tid < va) *reinterpret_cast<uint8_t*>(pb + tid) = 0;   // (at most 15 bytes)
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t q = va + 16ull * tid; q < ve; q += 16ull * 256) *reinterpret_cast<uint4*>(q) = z;
    if (ve + tid < pe) *reinterpret_cast<uint8_t*>(ve + tid) = 0;   // (at most 15 bytes)
}

// ------------------------------------------------------------------------------------------
// list pad kernel (tv_hybrid_verify_list: m launched entries, each a whole piece in a payload row or a slot).  Workgroup
// (x = entry, y = chunk) derives the entry's range itself -- its row and piece bytes from the v2 list table the call
// uploads anyway, its v1 length from its GLOBAL piece and the layout (tv_plan.h hybrid_list_chunk: the column rule with
// offset 0 and C = L) -- so the call builds and copies no tail table.  An entry with an empty range, and a chunk outside
// it, return at once.  The stores are the pad kernel's: bytes, uint4 from the first 16-byte aligned address, bytes;
// nothing below piece_bytes, nothing at or past v1_len (<= L <= the stride), nothing in a row outside the payload.  A
// piece listed twice is stored twice, with the same zeros.
// ------------------------------------------------------------------------------------------
struct TvHybridListPad {
    uint8_t* data;
    uint64_t stride;
    const uint32_t* rows;          // [m] payload row (or slot) of entry e
    const uint32_t* piece_bytes;   // [m]
    const uint64_t* pieces;        // [m] GLOBAL piece
    uint64_t total, L;             // the layout: v1_len(i) = min(L, total - i * L)
    uint32_t m;
    uint32_t nrows;                // rows of the payload (an entry outside them is skipped: never a store out of bounds)
};

__global__ __launch_bounds__(256) void tv_hybrid_list_pad_kernel(TvHybridListPad p) {
    const uint32_t en = blockIdx.x;
    if (en >= p.m) return;
    const uint32_t r = p.rows[en];
    uint64_t b, e;
    if (r >= p.nrows || !hybrid_list_chunk(p.piece_bytes[en], p.total, p.L, p.pieces[en], blockIdx.y, &b, &e)) return;
    const uint64_t row = reinterpret_cast<uint64_t>(p.data) + (uint64_t)r * p.stride;
    const uint64_t pb = row + b, pe = row + e;
    uint64_t va, ve;
    hybrid_split(pb, pe, &va, &ve);
    const uint32_t tid = threadIdx.x;
    if (pb + tid < va) *reinterpret_cast<uint8_t*>(pb + tid) = 0;   // (at most 15 bytes)
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t q = va + 16ull * tid; q < ve; q += 16ull * 256) *reinterpret_cast<uint4*>(q) = z;
    if (ve + tid < pe) *reinterpret_cast<uint8_t*>(ve + tid) = 0;   // (at most 15 bytes)
}

// `chunks` = the most chunks an entry's range has (0 = no entry has one: nothing is launched).
hipError_t launch_list_pad(const TvHybridListPad& p, uint64_t chunks, hipStream_t s) {
    if (p.m == 0 || chunks == 0) return hipSuccess;
    if (p.m > 0x7FFFFFFFu || chunks > 65535 || p.L > p.stride) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(tv_hybrid_list_pad_kernel, dim3(p.m, (uint32_t)chunks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace

namespace tvi {

// The column pad launch of one unit of a hybrid stream (tv_stream.hip): `chunks` = the most chunks a row's range has
// (the caller knows both tables; 0 = no row has a range: nothing is launched).
hipError_t hybrid_col_pad_launch(const tv_ctx* c, uint8_t* data, uint64_t pitch, const uint32_t* piece_bytes,
                                 uint64_t piece0, uint64_t offset, uint64_t C, uint64_t rows, uint64_t chunks,
                                 hipStream_t s) {
    if (rows == 0 || chunks == 0) return hipSuccess;
    if (rows > 0xFFFFFFull || chunks > 65535 || C + 256 != pitch) return hipErrorInvalidConfiguration;
    TvHybridColPad p{data, pitch, piece_bytes, c->total, c->L, piece0, offset, C, (uint32_t)rows};
    hipLaunchKernelGGL(tv_hybrid_col_pad_kernel, dim3((uint32_t)rows, (uint32_t)chunks), dim3(256), 0, s, p);
    return hipGetLastError();
}

// TV_OPT_HYBRID_PAD_PROBE (tools/hybrid_bench.py): zero the tails of the last hybrid call's table once more, timed on
// the compute stream: mode 1 = the pad kernel's one launch, mode 2 = one hipMemsetAsync per tail (what a host holding
// the rows would do without the kernel).  The time is TV_COUNTER_HYBRID_PAD_NS.
int hybrid_pad_probe(tv_ctx* c, int mode) {
    const int rc = v2_require(c, "TV_OPT_HYBRID_PAD_PROBE");
    if (rc) return rc;
    if (!c->hy_valid) return fail(c, TV_ERR_STATE, "TV_OPT_HYBRID_PAD_PROBE follows a hybrid call on this piece table");
    TV_HIP(c, hipSetDevice(c->device));
    TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
    if (mode == 1) {
        TvHybridPad pad{c->d_payload, c->stride, c->d_hy_tails.get<HybridTail>(), c->hy_n, c->hy_chunks,
                        (uint32_t)c->count, (uint32_t)c->L};
        TV_HIP(c, launch_pad(pad, c->stream));
    } else {
        for (const HybridTail& t : c->hy_tails_host)
            TV_HIP(c, hipMemsetAsync(c->d_payload + (uint64_t)t.row * c->stride + t.begin, 0, t.end - t.begin, c->stream));
    }
    TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
    TV_HIP(c, hipEventSynchronize(c->ev_k1));
    float ms = 0.f;
    TV_HIP(c, hipEventElapsedTime(&ms, c->ev_k0, c->ev_k1));
    c->hy_probe_ns = (uint64_t)((double)ms * 1e6);
    return TV_OK;
}

void hybrid_on_layout(tv_ctx* c) {
    c->hy_valid = false;
    c->hy_n = c->hy_chunks = 0;
    c->hy_tails_host.clear();
    c->v2_tab_bytes.clear();
    // (the rules of the list buffers and of the bit words: kept while not far larger than the new shard needs)
    if (c->d_hy_tails.cap > std::max<uint64_t>(1024, 2 * c->count)) free_buf(c->d_hy_tails);
    if (!reuse_fits(c->bit_words, c->d_hy_bits.cap)) free_buf(c->d_hy_bits);
    if (c->d_hy_list.cap > std::max<uint64_t>(1024, 2 * c->count)) free_buf(c->d_hy_list);
}

}  // namespace tvi

namespace {

// The state both calls need, in the order the header lists it; nothing is changed before the last check passes.
int hybrid_require(tv_ctx* c, const char* what, bool verify) {
    int rc = v2_require(c, what);
    if (rc) return rc;
    if (!c->v2_set) return fail(c, TV_ERR_STATE, "%s: tv_v2_set_pieces has not been called for this layout", what);
    if (verify && !c->digests_set) return fail(c, TV_ERR_STATE, "%s: tv_set_digests has not been called", what);
    if (verify && !c->v2_hashes)
        return fail(c, TV_ERR_STATE, "%s: the piece table has no expected hashes (creation mode)", what);
    return TV_OK;
}

// The shard's tail table on the device (built once per piece table) and, for a verify, the second bitfield.
int hybrid_prepare(tv_ctx* c, const char* what, bool verify) {
    std::vector<HybridTail> tails;
    uint64_t chunks = 0, bad = 0;
    if (!c->hy_valid) {
        if (c->v2_tab_bytes.size() != c->count) return fail(c, TV_ERR_STATE, "%s: no piece table", what);
        if (!hybrid_tails(c->total, c->L, c->first, c->count, c->v2_tab_bytes.data(), &tails, &chunks, &bad)) {
            if (bad == UINT64_MAX)
                return fail(c, TV_ERR_ARG, "%s takes piece lengths up to %llu bytes (the layout has %llu)", what,
                            (unsigned long long)kHybridMaxL, (unsigned long long)c->L);
            return fail(c, TV_ERR_ARG, "%s: piece_bytes[%llu] = %llu exceeds the piece's v1 length %llu (total_length "
                                       "%llu): the layout is not the v1 space of these pieces", what,
                        (unsigned long long)(c->first + bad), (unsigned long long)c->v2_tab_bytes[bad],
                        (unsigned long long)hybrid_v1_len(c->total, c->L, c->first + bad), (unsigned long long)c->total);
        }
        if (chunks > 0x7FFFFFFFull) return fail(c, TV_ERR_ARG, "%s: too many pad chunks", what);
    }
    TV_HIP(c, hipSetDevice(c->device));
    if (verify && !buf_fits(c->d_hy_bits, c->bit_words, false)) {
        TV_HIP(c, hipStreamSynchronize(c->stream));
        const int rc = grow_buf(c, c->d_hy_bits, c->bit_words, false, c->bit_words);
        if (rc) return rc;
    }
    if (c->hy_valid) return TV_OK;
    if (!tails.empty()) {
        TV_HIP(c, hipStreamSynchronize(c->stream));   // (a pad launch of the last table may still read the buffer)
        const int rc = grow_buf(c, c->d_hy_tails, tails.size(), false, std::max<uint64_t>(tails.size(), 1024));
        if (rc) return rc;
        TV_HIP(c, hipMemcpyAsync(c->d_hy_tails.ptr, tails.data(), tails.size() * sizeof(HybridTail),
                                 hipMemcpyHostToDevice, c->stream));
        TV_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->hy_n = (uint32_t)tails.size();
    c->hy_chunks = (uint32_t)chunks;
    c->hy_tails_host.swap(tails);
    c->hy_valid = true;
    return TV_OK;
}

// Pad kernel, SHA-1 launch, v2 launch set, one after the other on the compute stream; ev_k0 .. ev_k1 bracket them.  (The
// v2 launches on a second stream beside the SHA-1 launch were measured and not kept: DESIGN.md section 4.)
int hybrid_run(tv_ctx* c, const TvPieces& p1, TvV2& p2, bool hash) {
    TvHybridPad pad{};
    pad.data = c->d_payload;
    pad.stride = c->stride;
    pad.tails = c->d_hy_tails.get<HybridTail>();
    pad.n = c->hy_n;
    pad.chunks = c->hy_chunks;
    pad.rows = (uint32_t)c->count;
    pad.L = (uint32_t)c->L;
    const int kernel = choose_kernel(c);
    TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
    TV_HIP(c, launch_pad(pad, c->stream));   // (a shard with no tail launches nothing)
    int rc = launch_resident(c, p1, kernel, hash);
    if (rc) return rc;
    rc = v2_launch(c, p2, hash);
    if (rc) return rc;
    TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
    c->last_kernel = TV_KERNEL_HYBRID;
    c->last_launches = (c->hy_n ? 1 : 0) + 1 + 2 + (int)c->v2_maxlog;
    return TV_OK;
}

}  // namespace

extern "C" {

int tv_hybrid_verify(tv_ctx* c, const uint8_t* avail_bits, uint8_t* v1_bits_out, uint8_t* v2_bits_out,
                     uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = hybrid_require(c, "tv_hybrid_verify", true);
    if (rc) return rc;
    if (!c->count) return TV_OK;
    if (!bitfield_out) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    rc = hybrid_prepare(c, "tv_hybrid_verify", true);
    if (rc) return rc;
    const size_t wbytes = c->bit_words * 8, nbytes = (c->count + 7) / 8;
    rc = ensure_hbits(c, 2 * wbytes);
    if (rc) return rc;
    std::vector<uint8_t> av2(wbytes);
    DrainGuard drain(c);   // declared after av2: its H2D copy ends before it goes, also on error paths
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    // v1: base & caller & readable (d_avail or d_base_avail); v2: caller & readable, in the second half of d_hy_bits
    const uint64_t* av1 = nullptr;
    rc = launch_avail(c, avail_bits, &av1);
    if (rc) return rc;
    uint64_t* out2 = c->d_hy_bits.get<uint64_t>();
    uint64_t* d_av2 = out2 + c->d_hy_bits.cap;
    TvV2 p2 = v2_launch_args(c);
    p2.out64 = out2;
    if (v2_avail_bits(c, avail_bits, av2.data())) {
        TV_HIP(c, hipMemcpyAsync(d_av2, av2.data(), wbytes, hipMemcpyHostToDevice, c->stream));
        p2.avail64 = d_av2;
    }
    TvPieces p1 = resident_launch(c);
    p1.avail64 = av1;
    // fail closed: a piece a launch does not write reads as 0, never as a stale 1
    TV_HIP(c, hipMemsetAsync(c->d_out, 0, wbytes, c->stream));
    TV_HIP(c, hipMemsetAsync(out2, 0, wbytes, c->stream));
    rc = hybrid_run(c, p1, p2, false);
    if (rc) return rc;
    TV_HIP(c, hipMemcpyAsync(c->h_bits, c->d_out, wbytes, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipMemcpyAsync(c->h_bits + wbytes, out2, wbytes, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
    TV_HIP(c, hipEventSynchronize(c->ev_call1));
    const uint8_t spare = c->count % 8 ? (uint8_t)(0xFF00u >> (c->count % 8)) : 0xFF;   // spare bits 0
    for (size_t k = 0; k < nbytes; k++) {
        const uint8_t m = k + 1 == nbytes ? spare : 0xFF;
        const uint8_t b1 = c->h_bits[k] & m, b2 = c->h_bits[wbytes + k] & m;
        if (v1_bits_out) v1_bits_out[k] = b1;
        if (v2_bits_out) v2_bits_out[k] = b2;
        bitfield_out[k] = b1 & b2;
    }
    return finish_timing(c);
}

int tv_hybrid_hash(tv_ctx* c, uint8_t* digests_out, uint8_t* roots_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = hybrid_require(c, "tv_hybrid_hash", false);
    if (rc) return rc;
    if (!c->count) return TV_OK;
    if (!digests_out || !roots_out) return fail(c, TV_ERR_ARG, "NULL argument");
    rc = hybrid_prepare(c, "tv_hybrid_hash", false);
    if (rc) return rc;
    std::vector<uint32_t> soa1(5 * c->count), soa2(8 * c->count);
    DrainGuard drain(c);   // declared after the vectors: drains before they are freed, also on error paths
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    TvPieces p1 = resident_launch(c);
    p1.avail64 = nullptr;
    TvV2 p2 = v2_launch_args(c);
    rc = hybrid_run(c, p1, p2, true);
    if (rc) return rc;
    TV_HIP(c, hipMemcpyAsync(soa1.data(), c->d_hash, soa1.size() * 4, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipMemcpyAsync(soa2.data(), p2.roots, soa2.size() * 4, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
    TV_HIP(c, hipEventSynchronize(c->ev_call1));
    for (uint64_t j = 0; j < c->count; j++) {
        digest_unpack(soa1.data(), c->count, j, 5, digests_out + 20 * j);
        digest_unpack(soa2.data(), c->count, j, 8, roots_out + 32 * j);
    }
    return finish_timing(c);
}

// The check of completed pieces of a hybrid torrent: tv_verify_list's and tv_v2_verify_list's launch
// parts (tv_ctx.h V1List / V2List) over the same rows or slots, after the list pad launch; one wait.
int tv_hybrid_verify_list(tv_ctx* c, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                          const uint32_t* tree_leaves, const uint8_t* hashes, uint8_t* v1_ok_out, uint8_t* v2_ok_out,
                          uint8_t* ok_out, int release) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    // the state, in the order the header lists it
    if (!c->has_layout) return fail(c, TV_ERR_STATE, "tv_set_layout has not been called");
    if (c->batch_on) return batch_refused(c);
    if (!c->digests_set) return fail(c, TV_ERR_STATE, "tv_set_digests has not been called");
    if (c->win)
        return fail(c, TV_ERR_STATE, "tv_hybrid_verify_list needs the shard resident or a slot pool (TV_OPT_LIST_SLOTS); "
                                     "this layout is windowed (the shard exceeds the device budget)");
    if (c->count && !c->d_payload)
        return fail(c, TV_ERR_STATE, "no resident payload (the layout was set with TV_OPT_RESIDENT = 0): use tv_stream_*");
    if (c->st.active) return fail(c, TV_ERR_STATE, "a stream is active (finish it with tv_stream_end or tv_stream_abort)");
    if (n == 0) return TV_OK;
    if (!pieces || !piece_bytes || !tree_leaves || !hashes || !ok_out) return fail(c, TV_ERR_ARG, "NULL argument");
    // every entry is checked before anything is stored, launched or freed: a refused call changes nothing
    int rc = v2_list_check(c, "tv_hybrid_verify_list", n, pieces, piece_bytes, tree_leaves);
    if (rc) return rc;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t v1 = hybrid_v1_len(c->total, c->L, pieces[k]);
        if (piece_bytes[k] > v1)
            return fail(c, TV_ERR_ARG, "tv_hybrid_verify_list: piece_bytes[%llu] = %llu exceeds the piece's v1 length "
                                       "%llu (total_length %llu): the layout is not the v1 space of these pieces",
                        (unsigned long long)k, (unsigned long long)piece_bytes[k], (unsigned long long)v1,
                        (unsigned long long)c->total);
    }
    std::vector<uint8_t> ok1(n, 0), ok2(n, 0);
    V1List l1;
    V2List l2;
    rc = v1_list_plan(c, n, pieces, ok1.data(), &l1);
    if (rc) return rc;
    v2_list_plan(c, n, pieces, piece_bytes, tree_leaves, hashes, ok2.data(), &l2);
    // the pad launch reads the v2 table's rows and bytes; it needs each launched entry's GLOBAL piece beside them
    const uint64_t m = l2.m;
    std::vector<uint64_t> global(m);
    uint64_t chunks = 0;
    for (uint64_t e = 0; e < m; e++) {
        const uint64_t k = l2.origin[e];
        global[e] = pieces[k];
        chunks = std::max(chunks, hybrid_list_chunks(piece_bytes[k], c->total, c->L, pieces[k]));
    }
    TV_HIP(c, hipSetDevice(c->device));
    if (m) {
        DrainGuard drain(c);  // after the host vectors: their H2D / D2H copies end before they go
        rc = v1_list_reserve(c, l1);
        if (!rc) rc = v2_list_reserve(c, l2);
        if (!rc) rc = grow_buf(c, c->d_hy_list, m, false, std::max<uint64_t>(m, 1024));
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
        rc = v1_list_upload(c, l1);
        if (!rc) rc = v2_list_upload(c, l2);
        if (rc) return rc;
        TV_HIP(c, hipMemcpyAsync(c->d_hy_list.ptr, global.data(), m * 8, hipMemcpyHostToDevice, c->stream));
        TvHybridListPad pad{};
        pad.data = c->d_payload;
        pad.stride = c->stride;
        pad.rows = c->d_v2_list.get<uint32_t>();
        pad.piece_bytes = pad.rows + m;
        pad.pieces = c->d_hy_list.get<uint64_t>();
        pad.total = c->total;
        pad.L = c->L;
        pad.m = (uint32_t)m;
        pad.nrows = (uint32_t)(c->slots ? c->slots : c->count);
        int kernel = 0;
        TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
        TV_HIP(c, launch_list_pad(pad, chunks, c->stream));   // (a list with no pad range launches nothing)
        rc = v1_list_launch(c, l1, &kernel);
        if (!rc) rc = v2_list_launch(c, l2);   // (last: TV_COUNTER_LAST_WORKGROUPS is its grid)
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
        rc = v1_list_download(c, l1);
        if (!rc) rc = v2_list_download(c, l2);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
        TV_HIP(c, hipEventSynchronize(c->ev_call1));
    } else {
        c->last_workgroups = 0;
    }
    v1_list_scatter(l1, ok1.data());
    v2_list_scatter(l2, ok2.data());
    list_zero_unread(c, n, pieces, ok1.data());
    list_zero_unread(c, n, pieces, ok2.data());
    for (uint64_t k = 0; k < n; k++) {
        if (v1_ok_out) v1_ok_out[k] = ok1[k];
        if (v2_ok_out) v2_ok_out[k] = ok2[k];
        ok_out[k] = ok1[k] & ok2[k];
    }
    if (release) list_release(c, n, pieces);
    rc = list_finish(c, TV_KERNEL_HYBRID_LIST, m);
    c->last_launches = m ? 2 + (chunks ? 1 : 0) : 0;
    return rc;
}

}  // extern "C"
