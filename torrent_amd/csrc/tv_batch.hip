// tv_batch.hip -- the batch layout (tv_set_batch_layout, tv_batch_select, tv_batch_verify): many v1 torrents of any
// piece lengths resident at once and verified by ONE launch, for a client that holds a map of torrents (client.ts:
// `torrents: Map<string, Torrent>`) and re-checks all of them when it starts.
//
// The payload is one allocation with a region per torrent, each laid out as a resident single-torrent layout (rows of
// stride = round_up(L, 64) + pad), 256-byte aligned.  The context's geometry fields (total, L, P, count, stride,
// region) and per-torrent state (digest_ok, file_bad, digests_set) are the SELECTED torrent's, so piece_dst / piece_src
// and the clip helpers, and with them every staging call, work on it unchanged; tv_batch_select swaps them with the
// copies in tv_ctx::batch.  The digest table is [5][N] over all N pieces, torrent t's columns from col0.
// tv_batch_verify plans on the host (tv_plan.h batch_plan: launch order, groups, each group's block ranges), uploads
// one {offset, length, digest column} per launch position and one record per group, launches the BATCH instantiation
// of the chosen kernel form and scatters the out bytes into the per-torrent bitfields, applying availability, the
// unreadable marks and the base bits (a 20-byte digest slice, a piece inside the torrent) there.
#include <cstring>

#include "tv_ctx.h"

using namespace tvi;

namespace tvi {

int batch_refused(tv_ctx* c) {
    return fail(c, TV_ERR_STATE, "a batch layout is set (tv_set_batch_layout): its torrents verify with tv_batch_verify "
                                 "only; tv_set_layout returns the context to one torrent");
}

void batch_end(tv_ctx* c) {
    c->batch_on = false;
    c->batch.clear();
    c->batch_cur = c->batch_pieces = 0;
    c->region = 0;
    free_buf(c->d_batch);
    free_buf(c->d_batch_geom);
}

// The selected torrent's state back into its record / a record's into the context.
static void batch_save(tv_ctx* c) {
    BatchTorrent& b = c->batch[c->batch_cur];
    b.digests_set = c->digests_set;
    b.any_file_bad = c->any_file_bad;
    b.digest_ok.swap(c->digest_ok);
    b.file_bad.swap(c->file_bad);
}

static void batch_load(tv_ctx* c, uint64_t t) {
    BatchTorrent& b = c->batch[t];
    c->batch_cur = t;
    c->total = b.total;
    c->L = b.L;
    c->P = c->count = b.count;
    c->first = 0;
    c->stride = b.stride;
    c->region = b.region;
    c->digests_set = b.digests_set;
    c->any_file_bad = b.any_file_bad;
    c->digest_ok.swap(b.digest_ok);
    c->file_bad.swap(b.file_bad);
}

int batch_put_digests(tv_ctx* c, const uint32_t* soa) {
    if (!c->count) return TV_OK;
    const BatchTorrent& b = c->batch[c->batch_cur];
    TV_HIP(c, hipSetDevice(c->device));
    TV_HIP(c, hipMemcpy2DAsync(c->d_digests + b.col0, c->batch_pieces * 4, soa, c->count * 4, c->count * 4, 5,
                               hipMemcpyHostToDevice, c->stream));
    TV_HIP(c, hipStreamSynchronize(c->stream));
    return TV_OK;
}

}  // namespace tvi

extern "C" {

int tv_set_batch_layout(tv_ctx* c, uint64_t n_torrents, const uint64_t* total_length, const uint64_t* piece_length,
                        const uint64_t* n_pieces) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    if (!n_torrents) return fail(c, TV_ERR_ARG, "n_torrents must be > 0");
    if (!total_length || !piece_length || !n_pieces) return fail(c, TV_ERR_ARG, "NULL argument");
    if (c->list_slots_opt)
        return fail(c, TV_ERR_STATE, "tv_set_batch_layout: a batch has no slot pool (TV_OPT_LIST_SLOTS is set)");
    if (!c->resident)
        return fail(c, TV_ERR_STATE, "tv_set_batch_layout: a batch is resident (TV_OPT_RESIDENT is 0)");
    // every torrent's geometry by tv_set_layout's rules, its region and its columns
    std::vector<BatchTorrent> bt(n_torrents);
    uint64_t bytes = 0, pieces = 0, bits = 0;
    for (uint64_t t = 0; t < n_torrents; t++) {
        const uint64_t L = piece_length[t], n = n_pieces[t];
        if (L == 0) return fail(c, TV_ERR_ARG, "torrent %llu: piece_length must be > 0", (unsigned long long)t);
        if (L > (1ull << 36)) return fail(c, TV_ERR_ARG, "torrent %llu: piece_length must be <= 64 GiB", (unsigned long long)t);
        const uint64_t stride = ((L + 63) / 64) * 64 + c->pad;
        if (n >= 0xFFFFFFFFull || n >= UINT64_MAX / 20 || n >= UINT64_MAX / L - 1 ||
            (n && n > (UINT64_MAX - kSlack - 256 - bytes) / stride))
            return fail(c, TV_ERR_ARG, "torrent %llu: geometry overflows 64-bit offsets or is larger than a layout may "
                                       "be (%llu pieces of %llu bytes)", (unsigned long long)t, (unsigned long long)n,
                        (unsigned long long)L);
        pieces += n;
        if (pieces >= 0xFFFFFFFFull)
            return fail(c, TV_ERR_ARG, "torrent %llu: the batch would hold %llu pieces (at most 2^32 - 2)",
                        (unsigned long long)t, (unsigned long long)pieces);
        BatchTorrent& b = bt[t];
        b.total = total_length[t];
        b.L = L;
        b.count = n;
        b.stride = stride;
        b.region = bytes;
        b.col0 = pieces - n;
        b.bit0 = bits;
        b.digest_ok.assign((n + 7) / 8 + 8, 0);
        b.file_bad.assign((n + 7) / 8 + 8, 0);
        bytes = (bytes + n * stride + 255) / 256 * 256;   // (every region starts 256-byte aligned)
        bits += (n + 7) / 8;
    }
    const uint64_t need = pieces ? bytes + kSlack : 0;
    TV_HIP(c, hipSetDevice(c->device));
    // the device budget, as tv_set_layout computes it; a batch has no windows, so beyond it there is nothing to fall
    // back to (checked before anything changes: the context stays as it was)
    uint64_t budget = c->budget_opt;
    if (need && !budget) {
        size_t fr = 0, tot = 0;
        TV_HIP(c, hipMemGetInfo(&fr, &tot));
        const uint64_t avail = (uint64_t)fr + c->cap_payload + c->d_chunk[0].bytes() + c->d_chunk[1].bytes();
        const uint64_t margin = (4ull << 30) + 64 * pieces;
        budget = avail > margin ? avail - margin : 0;
    }
    if (need > budget)
        return fail(c, TV_ERR_NOMEM, "the batch needs %llu bytes of device memory, the budget is %llu "
                                     "(TV_OPT_RESIDENT_BUDGET; a batch has no windows: set smaller batches)",
                    (unsigned long long)need, (unsigned long long)budget);
    stream_abort_locked(c);
    TV_HIP(c, hipStreamSynchronize(c->stream));
    TV_HIP(c, hipStreamSynchronize(c->copy_stream));
    TV_HIP(c, hipStreamSynchronize(c->copy_stream2));
    {
        const int rc = win_sync_streams(c);
        if (rc) return rc;
    }
    // the state tv_set_layout resets: no windows, no slots, no v2 table, nothing marked
    c->has_layout = false;
    batch_end(c);
    c->digests_set = false;
    c->any_file_bad = c->any_unhashed = false;
    c->win = false;
    c->win_n = 0;
    c->win_bufs = 0;
    c->win_nhs = 1;
    c->win_buf_bytes = 0;
    c->win_cur = UINT64_MAX;
    c->win_buf = 1;
    c->win_valid = 0;
    c->win_done = c->win_timing = false;
    c->win_launched = c->win_passes = 0;
    c->slots = 0;
    c->slot_of.clear();
    c->slot_free.clear();
    c->budget = budget;
    c->total = c->P = c->first = c->count = 0;   // (what v2_on_layout / hybrid_on_layout size by: a batch holds no v2 memory)
    c->L = 1;
    c->bit_words = 0;
    c->unhashed.assign(8, 0);
    // tv_set_layout's reuse rule for the payload and the per-piece tables
    if (!need || !reuse_fits(need, c->cap_payload) || c->cap_payload > budget) free_payload(c);
    if (!reuse_fits(pieces, c->cap_count)) free_per_piece(c);
    for (DevBuf& b : c->d_chunk) free_buf(b);
    if (c->d_list.cap > std::max<uint64_t>(1024, 2 * pieces)) {
        free_buf(c->d_list);
        free_buf(c->d_list_out);
    }
    v2_on_layout(c);
    hybrid_on_layout(c);
    if (need && !c->d_payload) {
        const hipError_t e = hipMalloc((void**)&c->d_payload, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            c->d_payload = nullptr;
            return fail(c, e == hipErrorOutOfMemory ? TV_ERR_NOMEM : TV_ERR_HIP,
                        "hipMalloc(%llu) of the batch payload (budget %llu): %s", (unsigned long long)need,
                        (unsigned long long)budget, hipGetErrorString(e));
        }
        c->cap_payload = need;
        c->n_payload_allocs++;
        c->n_device_allocs++;
    }
    if (pieces && !c->d_digests) {
        TV_HIP(c, hipMalloc((void**)&c->d_digests, 5 * pieces * sizeof(uint32_t)));
        TV_HIP(c, hipMalloc((void**)&c->d_state, 5 * pieces * sizeof(uint32_t)));
        TV_HIP(c, hipMalloc((void**)&c->d_hash, 5 * pieces * sizeof(uint32_t)));
        c->cap_count = pieces;
        c->n_device_allocs += 3;
    }
    if (need) {   // the tail over-read slack past the last region reads zeros
        TV_HIP(c, hipMemsetAsync(c->d_payload + bytes, 0, kSlack, c->stream));
        TV_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->batch.swap(bt);
    c->batch_pieces = pieces;
    c->batch_on = true;
    batch_load(c, 0);
    c->has_layout = true;
    return TV_OK;
}

int tv_batch_select(tv_ctx* c, uint64_t torrent) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->has_layout || !c->batch_on) return fail(c, TV_ERR_STATE, "tv_set_batch_layout has not been called");
    if (torrent >= c->batch.size())
        return fail(c, TV_ERR_ARG, "torrent %llu is not in the batch of %llu torrents", (unsigned long long)torrent,
                    (unsigned long long)c->batch.size());
    batch_save(c);
    batch_load(c, torrent);
    return TV_OK;
}

int tv_batch_verify(tv_ctx* c, const uint8_t* avail_bits, uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->has_layout || !c->batch_on) return fail(c, TV_ERR_STATE, "tv_set_batch_layout has not been called");
    // the selected torrent's state joins the others' for the call and comes back on every exit
    batch_save(c);
    struct Reload {
        tv_ctx* c;
        ~Reload() { batch_load(c, c->batch_cur); }
    } reload{c};
    const uint64_t N = c->batch_pieces;
    uint64_t out_bytes = 0;
    for (uint64_t t = 0; t < c->batch.size(); t++) {
        const BatchTorrent& b = c->batch[t];
        if (b.count && !b.digests_set)
            return fail(c, TV_ERR_STATE, "torrent %llu: tv_set_digests has not been called (tv_batch_select it first)",
                        (unsigned long long)t);
        out_bytes += (b.count + 7) / 8;
    }
    if (!bitfield_out && N) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    if (N == 0) return list_finish(c, 0, 0);
    // every piece of the batch in (torrent, piece) order: its length, bytes, digest column and bit
    std::vector<uint64_t> lens(N), offs(N), bit(N);
    std::vector<uint8_t> allowed(N);
    {
        uint64_t e = 0;
        for (const BatchTorrent& b : c->batch)
            for (uint64_t j = 0; j < b.count; j++, e++) {
                const uint64_t len = (j == b.count - 1 && b.total % b.L) ? b.total % b.L : b.L;   // piece.ts:16-19
                lens[e] = len;
                offs[e] = b.region + j * b.stride;
                bit[e] = b.bit0 * 8 + j;
                // the base bits (a whole digest slice, the piece inside the torrent), the caller's, file staging's marks
                allowed[e] = get_bit(b.digest_ok.data(), j) && j * b.L + len <= b.total &&
                             !(b.any_file_bad && get_bit(b.file_bad.data(), j)) &&
                             (!avail_bits || get_bit(avail_bits, bit[e]));
            }
    }
    // the kernel form, as for a list (v1_list_launch): a forced one, else twin while the entries fit 64 x CUs, split up
    // to 16,384, lane beyond; no companion workgroups
    const int kernel = (c->kernel_opt == TV_KERNEL_LANE || c->kernel_opt == TV_KERNEL_SPLIT ||
                        c->kernel_opt == TV_KERNEL_TWIN)
                           ? c->kernel_opt
                           : (N <= 64 * (uint64_t)c->cus ? TV_KERNEL_TWIN : (N <= 256 * 64 ? TV_KERNEL_SPLIT : TV_KERNEL_LANE));
    std::vector<uint32_t> launch;
    std::vector<int64_t> origin;
    std::vector<BatchGroup> groups;
    batch_plan(N, lens.data(), tv_batch_span(kernel), &launch, &origin, &groups);
    const uint64_t m = launch.size();
    if (m >= 0xFFFFFFFFull) return fail(c, TV_ERR_ARG, "the batch launch would hold %llu positions", (unsigned long long)m);
    std::vector<uint64_t> h_off(2 * m);   // offsets, then lengths
    std::vector<uint32_t> h_col(m);
    std::vector<TvBatchGeom> h_geom(groups.size());
    for (uint64_t t = 0; t < m; t++) {
        h_off[t] = offs[launch[t]];
        h_off[m + t] = lens[launch[t]];
        h_col[t] = launch[t];   // (entry e's digest is column e of the [5][N] table: col0 + j)
    }
    for (uint64_t q = 0; q < groups.size(); q++) h_geom[q] = {groups[q].fast_end, groups[q].end, groups[q].nb_min, 0};
    std::vector<uint8_t> ok(m, 0);
    TV_HIP(c, hipSetDevice(c->device));
    DrainGuard drain(c);   // after the host vectors: their H2D / D2H copies end before they go
    int rc = grow_buf(c, c->d_batch, m, false, std::max<uint64_t>(m, 1024));
    if (!rc) rc = grow_buf(c, c->d_batch_geom, groups.size(), false, std::max<uint64_t>(groups.size(), 64));
    if (!rc) rc = grow_buf(c, c->d_list_out, m, false, std::max<uint64_t>(m, 1024));
    if (rc) return rc;
    const uint64_t cap = c->d_batch.cap;
    uint64_t* d_off = c->d_batch.get<uint64_t>();
    uint64_t* d_len = d_off + cap;
    uint32_t* d_col = reinterpret_cast<uint32_t*>(d_len + cap);
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    TV_HIP(c, hipMemcpyAsync(d_off, h_off.data(), m * 8, hipMemcpyHostToDevice, c->stream));
    TV_HIP(c, hipMemcpyAsync(d_len, h_off.data() + m, m * 8, hipMemcpyHostToDevice, c->stream));
    TV_HIP(c, hipMemcpyAsync(d_col, h_col.data(), m * 4, hipMemcpyHostToDevice, c->stream));
    TV_HIP(c, hipMemcpyAsync(c->d_batch_geom.ptr, h_geom.data(), h_geom.size() * sizeof(TvBatchGeom),
                             hipMemcpyHostToDevice, c->stream));
    TvPieces p{};
    p.data = c->d_payload;
    p.n = p.n_main = (uint32_t)m;
    p.last_idx = 0xFFFFFFFFu;
    p.blk_begin = 0;
    p.blk_end = UINT64_MAX;
    p.finalize = 1;
    p.dcount = (uint32_t)N;
    p.digests = c->d_digests;
    p.out_bytes = c->d_list_out.get<uint8_t>();
    p.b_off = d_off;
    p.b_len = d_len;
    p.b_col = d_col;
    p.b_geom = c->d_batch_geom.get<TvBatchGeom>();
    TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
    TV_HIP(c, tv_launch_verify_batch(p, kernel, c->stream, &c->last_workgroups));
    TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
    TV_HIP(c, hipMemcpyAsync(ok.data(), c->d_list_out.ptr, m, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
    TV_HIP(c, hipEventSynchronize(c->ev_call1));
    memset(bitfield_out, 0, out_bytes);
    for (uint64_t t = 0; t < m; t++)
        if (origin[t] >= 0 && ok[t] && allowed[origin[t]]) set_bit(bitfield_out, bit[origin[t]]);
    return list_finish(c, kernel, m);
}

}  // extern "C"
