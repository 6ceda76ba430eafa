// tv_v2.hip -- BitTorrent v2 (BEP 52): the piece table of a layout (tv_v2_set_pieces) and the SHA-256 merkle verify
// and hash calls over the resident shard (tv_v2_verify, tv_v2_hash): one leaf launch, one launch per tree level, one
// finish launch (tv_v2_kernels.hip); and the list verify of self-describing entries over a resident shard or a slot
// pool (tv_v2_verify_list): one launch, the trees in LDS; and the calls below the piece (tv_v2_leaf_hashes,
// tv_v2_check_blocks): the listed entries' 16 KiB blocks, one lane each, in one launch.
#include <cstring>

#include "tv_ctx.h"

using namespace tvi;

namespace tvi {

static bool v2_piece_length_ok(uint64_t L) { return L >= TV_V2_LEAF_BYTES && (L & (L - 1)) == 0; }

// Words of the two level buffers for `count` pieces of W leaves: A [8][count x W], B [8][count x max(W/2, 1)].
uint64_t v2_node_words(uint64_t count, uint64_t W) { return 8 * count * (W + (W > 1 ? W / 2 : 1)); }

void v2_on_layout(tv_ctx* c) {
    c->v2_set = c->v2_hashes = false;
    if (c->d_v2_list.cap > std::max<uint64_t>(1024, 2 * c->count)) free_buf(c->d_v2_list);   // (as tv_verify_list's buffers)
    // the block calls' items: kept while the new shard could list that many blocks (the same rule, in blocks)
    if (c->d_v2_blk.cap > std::max<uint64_t>(1024, 2 * c->count * std::max<uint64_t>(1, c->L / TV_V2_LEAF_BYTES)))
        free_buf(c->d_v2_blk);
    // a v2 stream's table and nodes: kept for a layout a v2 stream could run on and whose table they fit
    if (!(v2_piece_length_ok(c->L) && c->count && reuse_fits(11 * c->count, c->d_v2s_tab.cap))) {
        free_buf(c->d_v2s_tab);
        free_buf(c->d_v2s_nodes);
    }
    // keep what a v2 table of the new geometry would reuse; anything else goes (a v1 layout holds no v2 memory)
    const bool v2 = v2_piece_length_ok(c->L) && c->count && !c->win && !c->slots;
    if (!v2 || !reuse_fits(c->count, c->d_v2_tab.cap) ||
        !reuse_fits(v2_node_words(c->count, c->L / TV_V2_LEAF_BYTES), c->d_v2_nodes.cap)) {
        free_buf(c->d_v2_tab);
        free_buf(c->d_v2_nodes);
    }
}

int v2_check_entry(tv_ctx* c, uint64_t k, uint64_t b, uint64_t w) {
    const uint64_t W = c->L / TV_V2_LEAF_BYTES;
    if (b == 0 || b > c->L)
        return fail(c, TV_ERR_ARG, "piece_bytes[%llu] = %llu is outside 1 .. %llu", (unsigned long long)k,
                    (unsigned long long)b, (unsigned long long)c->L);
    if (w == 0 || (w & (w - 1)) || w < (b + TV_V2_LEAF_BYTES - 1) / TV_V2_LEAF_BYTES || w > W)
        return fail(c, TV_ERR_ARG, "tree_leaves[%llu] = %llu is not a power of two in %llu .. %llu",
                    (unsigned long long)k, (unsigned long long)w,
                    (unsigned long long)((b + TV_V2_LEAF_BYTES - 1) / TV_V2_LEAF_BYTES), (unsigned long long)W);
    return TV_OK;
}

int v2_check_table(tv_ctx* c, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves) {
    if (!v2_piece_length_ok(c->L))
        return fail(c, TV_ERR_ARG, "a v2 piece length is a power of two >= %d (the layout has %llu)", TV_V2_LEAF_BYTES,
                    (unsigned long long)c->L);
    if (n != c->P)
        return fail(c, TV_ERR_ARG, "the piece table has %llu entries, the layout %llu pieces", (unsigned long long)n,
                    (unsigned long long)c->P);
    if (n && (!piece_bytes || !tree_leaves)) return fail(c, TV_ERR_ARG, "NULL argument");
    for (uint64_t p = 0; p < n; p++) {
        const int rc = v2_check_entry(c, p, piece_bytes[p], tree_leaves[p]);
        if (rc) return rc;
    }
    return TV_OK;
}

// The calls' common state checks (in the order the header lists them).
int v2_require(tv_ctx* c, const char* what) {
    const int rc = require_layout(c, false, true);
    if (rc) return rc;
    if (c->win)
        return fail(c, TV_ERR_STATE, "%s needs the shard resident; this layout is windowed (the shard exceeds the "
                                     "device budget)", what);
    if (c->slots) return fail(c, TV_ERR_STATE, "%s needs the shard resident; this layout is a slot pool (TV_OPT_LIST_SLOTS)", what);
    return TV_OK;
}

TvV2 v2_launch_args(tv_ctx* c) {
    TvV2 p{};
    const uint64_t W = 1ull << c->v2_logW;
    p.data = c->d_payload;
    p.stride = c->stride;
    p.n = (uint32_t)c->count;
    p.logW = c->v2_logW;
    // piece-major needs a full wave of pieces; below that (and by default) leaf-linear
    const int want = c->v2_map_opt ? c->v2_map_opt : TV_V2_MAP_LEAF;
    p.map = (want == TV_V2_MAP_PIECE && c->count >= 64) ? TV_V2_MAP_PIECE : TV_V2_MAP_LEAF;
    uint32_t* tab = c->d_v2_tab.get<uint32_t>();
    const uint64_t cap = c->d_v2_tab.cap;
    p.piece_bytes = tab;
    p.tree_leaves = tab + cap;
    p.expect = tab + 2 * cap;     // [8][count] packed at the row length `count` (<= cap)
    p.roots = tab + 10 * cap;
    p.nodes_a = c->d_v2_nodes.get<uint32_t>();
    p.nodes_b = p.nodes_a + 8 * c->count * W;
    p.out64 = c->d_out;
    p.clock = c->clock_probe ? c->d_clock : nullptr;
    return p;
}

// leaf kernel, tree levels, finish
int v2_launch(tv_ctx* c, TvV2& p, bool hash) {
    TV_HIP(c, tv_v2_launch_leaves(p, c->stream, &c->last_workgroups));
    for (uint32_t l = 0; l < c->v2_maxlog; l++) TV_HIP(c, tv_v2_launch_level(p, l, c->v2_maxlog, c->stream));
    TV_HIP(c, tv_v2_launch_finish(p, hash, c->stream));
    c->v2_last_map = (int)p.map;
    return TV_OK;
}

}  // namespace tvi

namespace {

// the launch set of tv_v2_verify / tv_v2_hash on the compute stream; ev_k0 .. ev_k1 bracket it
int v2_run(tv_ctx* c, TvV2& p, bool hash) {
    TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
    const int rc = v2_launch(c, p, hash);
    if (rc) return rc;
    TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
    c->last_kernel = TV_KERNEL_V2;
    c->last_launches = 2 + (int)c->v2_maxlog;
    return TV_OK;
}

// The entries of a list call (tv_v2_verify_list, tv_v2_leaf_hashes, tv_v2_check_blocks) against the layout: GLOBAL
// pieces of this shard with tv_v2_set_pieces' ranges and texts.
int v2_check_entries(tv_ctx* c, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                     const uint32_t* tree_leaves) {
    for (uint64_t k = 0; k < n; k++) {
        int rc = list_in_shard(c, pieces[k]);
        if (!rc) rc = v2_check_entry(c, k, piece_bytes[k], tree_leaves[k]);
        if (rc) return rc;
    }
    return TV_OK;
}

// tv_v2_leaf_hashes (check = false: `out` = leaves_out) and tv_v2_check_blocks (check = true: `out` = ok_bits_out).
// One tv_v2_block_kernel launch over the items v2_block_items (tv_plan.h) makes of the entries.
int v2_blocks_call(tv_ctx* c, const char* what, bool check, uint64_t n, const uint64_t* pieces,
                   const uint32_t* piece_bytes, const uint32_t* tree_leaves, const uint8_t* leaf_hashes,
                   const uint8_t* want_bits, uint8_t* out, int release) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, false, true);
    if (rc) return rc;
    if (c->win)
        return fail(c, TV_ERR_STATE, "%s needs the shard resident or a slot pool (TV_OPT_LIST_SLOTS); this layout is "
                                     "windowed (the shard exceeds the device budget)", what);
    if (n == 0) return TV_OK;
    if (!pieces || !piece_bytes || !tree_leaves || !out || (check && !leaf_hashes))
        return fail(c, TV_ERR_ARG, "NULL argument");
    if (n >= 0xFFFFFF00ull) return fail(c, TV_ERR_ARG, "list too long");
    if (!v2_piece_length_ok(c->L))
        return fail(c, TV_ERR_ARG, "a v2 piece length is a power of two >= %d (the layout has %llu)", TV_V2_LEAF_BYTES,
                    (unsigned long long)c->L);
    const uint64_t W = c->L / TV_V2_LEAF_BYTES;
    // everything is checked before anything is launched or freed: a refused call changes nothing
    rc = v2_check_entries(c, n, pieces, piece_bytes, tree_leaves);
    if (rc) return rc;
    if (!check && (W > TV_V2_BLOCKS_MAX || n > TV_V2_BLOCKS_MAX / W))
        return fail(c, TV_ERR_ARG, "%s: %llu entries of %llu leaf positions exceed TV_V2_BLOCKS_MAX (%llu)", what,
                    (unsigned long long)n, (unsigned long long)W, (unsigned long long)TV_V2_BLOCKS_MAX);
    // entries with nothing to hash: in a slot pool a piece that holds no slot (never staged), anywhere a piece file
    // staging could not read
    std::vector<uint8_t> skip(n, 0);
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t j = pieces[k] - c->first;
        const bool no_slot = !list_held(c, j);
        const bool unread = c->any_file_bad && get_bit(c->file_bad.data(), j);
        if (!no_slot && !unread) continue;
        if (!check)
            return fail(c, TV_ERR_STATE, no_slot ? "%s: piece %llu holds no slot (it was never staged, or was listed since)"
                                                 : "%s: piece %llu was marked unreadable by tv_stage_file(s)",
                        what, (unsigned long long)pieces[k]);
        skip[k] = 1;
    }
    std::vector<V2BlockItem> items;
    if (!v2_block_items(n, piece_bytes, W, check ? want_bits : nullptr, skip.data(), TV_V2_BLOCKS_MAX, &items))
        return fail(c, TV_ERR_ARG, "%s: more than TV_V2_BLOCKS_MAX (%llu) blocks to hash", what,
                    (unsigned long long)TV_V2_BLOCKS_MAX);
    const uint64_t m = items.size(), words = (m + 63) / 64;
    std::vector<uint32_t> tab((check ? 11 : 3) * m);   // rows, leaves, lens, expected leaf words [8][m] (big-endian values)
    for (uint64_t t = 0; t < m; t++) {
        const uint64_t k = items[t].entry, j = pieces[k] - c->first;
        tab[t] = list_row(c, j);
        tab[m + t] = items[t].leaf;
        tab[2 * m + t] = items[t].len;
        if (check) digest_pack(leaf_hashes + (k * W + items[t].leaf) * 32, 8, tab.data() + 3 * m, m, t);
    }
    std::vector<uint64_t> ballots(check ? words : 0);
    std::vector<uint32_t> soa(check ? 0 : 8 * m);
    TV_HIP(c, hipSetDevice(c->device));
    if (m) {
        DrainGuard drain(c);  // after the host vectors: their H2D / D2H copies end before they go
        // a check's ballot words (one bit per item), then 11 table words per item: within 48 bytes per item
        rc = grow_buf(c, c->d_v2_blk, m, false, std::max<uint64_t>(m, 1024));
        if (rc) return rc;
        uint64_t* d_out = c->d_v2_blk.get<uint64_t>();
        uint32_t* d = c->d_v2_blk.get<uint32_t>() + 2 * words;
        TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
        TV_HIP(c, hipMemcpyAsync(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
        // fail closed: an item the launch does not write reads as a mismatch
        if (check) TV_HIP(c, hipMemsetAsync(d_out, 0, words * 8, c->stream));
        TvV2Blocks p{};
        p.data = c->d_payload;
        p.stride = c->stride;
        p.m = (uint32_t)m;
        p.rows = d;
        p.leaves = d + m;
        p.lens = d + 2 * m;
        p.expect = d + 3 * m;
        p.hashes = d + 3 * m;
        p.out64 = d_out;
        TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
        TV_HIP(c, tv_v2_launch_blocks(p, check, c->stream, &c->last_workgroups));
        TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
        if (check) TV_HIP(c, hipMemcpyAsync(ballots.data(), d_out, words * 8, hipMemcpyDeviceToHost, c->stream));
        else TV_HIP(c, hipMemcpyAsync(soa.data(), p.hashes, soa.size() * 4, hipMemcpyDeviceToHost, c->stream));
        TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
        TV_HIP(c, hipEventSynchronize(c->ev_call1));
    } else {
        c->last_workgroups = 0;
    }
    if (check) {
        v2_block_scatter(n, W, items, ballots.data(), out);
    } else {
        memset(out, 0, n * W * 32);   // positions past a piece's bytes: zero hashes, out to W
        for (uint64_t t = 0; t < m; t++)
            digest_unpack(soa.data(), m, t, 8, out + ((uint64_t)items[t].entry * W + items[t].leaf) * 32);
    }
    if (release) list_release(c, n, pieces);
    return list_finish(c, TV_KERNEL_V2_BLOCKS, m);
}

}  // namespace

namespace tvi {

// ---- the launch parts of tv_v2_verify_list (tv_ctx.h: V2List), shared with tv_hybrid_verify_list ------------------------

int v2_list_check(tv_ctx* c, const char* what, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                  const uint32_t* tree_leaves) {
    if (n >= 0xFFFFFF00ull) return fail(c, TV_ERR_ARG, "list too long");
    if (!v2_piece_length_ok(c->L))
        return fail(c, TV_ERR_ARG, "a v2 piece length is a power of two >= %d (the layout has %llu)", TV_V2_LEAF_BYTES,
                    (unsigned long long)c->L);
    if (c->L / TV_V2_LEAF_BYTES > (1ull << TV_V2_LIST_MAX_LOGW))
        return fail(c, TV_ERR_ARG, "%s takes pieces of up to %llu bytes (the layout has %llu)", what,
                    (unsigned long long)TV_V2_LEAF_BYTES << TV_V2_LIST_MAX_LOGW, (unsigned long long)c->L);
    return v2_check_entries(c, n, pieces, piece_bytes, tree_leaves);
}

// The entries launched: every listed piece, or, in a slot pool, the listed pieces that hold a slot (the others were
// never staged: 0).  origin[e] = the entry's index in the caller's arrays.
void v2_list_plan(tv_ctx* c, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                  const uint32_t* tree_leaves, const uint8_t* hashes, uint8_t* ok_out, V2List* l) {
    l->origin.clear();
    l->origin.reserve(n);
    for (uint64_t k = 0; k < n; k++) {
        if (list_held(c, pieces[k] - c->first)) l->origin.push_back(k);
        else ok_out[k] = 0;
    }
    const uint64_t m = l->m = l->origin.size();
    l->tab.assign(11 * m, 0);
    for (uint64_t e = 0; e < m; e++) {
        const uint64_t k = l->origin[e], j = pieces[k] - c->first;
        l->tab[e] = list_row(c, j);
        l->tab[m + e] = piece_bytes[k];
        l->tab[2 * m + e] = tree_leaves[k];
        digest_pack(hashes + 32 * k, 8, l->tab.data() + 3 * m, m, e);
    }
    l->ok.assign(m, 0);
}

// (11 table words and 4 out bytes per entry)
int v2_list_reserve(tv_ctx* c, const V2List& l) {
    return grow_buf(c, c->d_v2_list, l.m, false, std::max<uint64_t>(l.m, 1024));
}

static uint8_t* v2_list_out(const tv_ctx* c) {
    return reinterpret_cast<uint8_t*>(c->d_v2_list.get<uint32_t>() + 11 * c->d_v2_list.cap);
}

int v2_list_upload(tv_ctx* c, const V2List& l) {
    TV_HIP(c, hipMemcpyAsync(c->d_v2_list.ptr, l.tab.data(), l.tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    // fail closed: an entry the launch does not write reads as 0
    TV_HIP(c, hipMemsetAsync(v2_list_out(c), 0, l.m, c->stream));
    return TV_OK;
}

int v2_list_launch(tv_ctx* c, const V2List& l) {
    const uint64_t m = l.m, W = c->L / TV_V2_LEAF_BYTES;
    uint32_t* d = c->d_v2_list.get<uint32_t>();
    TvV2List p{};
    p.data = c->d_payload;
    p.stride = c->stride;
    p.m = (uint32_t)m;
    while ((1ull << p.logW) < W) p.logW++;
    p.rows = d;
    p.bytes = d + m;
    p.widths = d + 2 * m;
    p.expect = d + 3 * m;
    p.out_bytes = v2_list_out(c);
    TV_HIP(c, tv_v2_launch_list(p, c->stream, &c->last_workgroups));
    return TV_OK;
}

int v2_list_download(tv_ctx* c, V2List& l) {
    TV_HIP(c, hipMemcpyAsync(l.ok.data(), v2_list_out(c), l.m, hipMemcpyDeviceToHost, c->stream));
    return TV_OK;
}

void v2_list_scatter(const V2List& l, uint8_t* ok_out) {
    for (uint64_t e = 0; e < l.m; e++) ok_out[l.origin[e]] = l.ok[e];
}

}  // namespace tvi

extern "C" {

int tv_v2_set_pieces(tv_ctx* c, uint64_t n, const uint32_t* piece_bytes, const uint32_t* tree_leaves,
                     const uint8_t* hashes) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = v2_require(c, "tv_v2_set_pieces");
    if (rc) return rc;
    c->v2_set = c->v2_hashes = false;
    c->hy_valid = false;
    rc = v2_check_table(c, n, piece_bytes, tree_leaves);
    if (rc) return rc;
    c->v2_tab_bytes.assign(piece_bytes + (c->count ? c->first : 0), piece_bytes + (c->count ? c->first + c->count : 0));
    const uint64_t W = c->L / TV_V2_LEAF_BYTES;
    uint32_t logW = 0;
    while ((1ull << logW) < W) logW++;
    c->v2_logW = logW;
    c->v2_maxlog = 0;
    if (!c->count) {
        c->v2_set = true;
        c->v2_hashes = hashes != nullptr;
        return TV_OK;
    }
    TV_HIP(c, hipSetDevice(c->device));
    TV_HIP(c, hipStreamSynchronize(c->stream));   // (a v2 call of the last table may still read the buffers)
    const uint64_t need_nodes = v2_node_words(c->count, W);
    rc = grow_buf(c, c->d_v2_tab, c->count, true, c->count);
    if (!rc) rc = grow_buf(c, c->d_v2_nodes, need_nodes, true, need_nodes);
    if (rc) return rc;
    // the shard's rows: bytes, leaves, expected root words (big-endian values, SoA)
    const uint64_t cap = c->d_v2_tab.cap;
    std::vector<uint32_t> tab(10 * cap, 0);
    uint32_t maxw = 1;
    for (uint64_t j = 0; j < c->count; j++) {
        const uint64_t i = c->first + j;
        tab[j] = piece_bytes[i];
        tab[cap + j] = tree_leaves[i];
        maxw = std::max(maxw, tree_leaves[i]);
        if (hashes) digest_pack(hashes + 32 * i, 8, tab.data() + 2 * cap, c->count, j);
    }
    while ((1u << c->v2_maxlog) < maxw) c->v2_maxlog++;
    TV_HIP(c, hipMemcpyAsync(c->d_v2_tab.ptr, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    TV_HIP(c, hipStreamSynchronize(c->stream));
    c->v2_set = true;
    c->v2_hashes = hashes != nullptr;
    return TV_OK;
}

int tv_v2_verify(tv_ctx* c, const uint8_t* avail_bits, uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = v2_require(c, "tv_v2_verify");
    if (rc) return rc;
    if (!c->v2_set) return fail(c, TV_ERR_STATE, "tv_v2_set_pieces has not been called for this layout");
    if (!c->v2_hashes) return fail(c, TV_ERR_STATE, "tv_v2_verify: the piece table has no expected hashes (creation mode)");
    if (!bitfield_out && c->count) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    if (!c->count) return TV_OK;
    TV_HIP(c, hipSetDevice(c->device));
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    TvV2 p = v2_launch_args(c);
    rc = launch_avail(c, avail_bits, &p.avail64, false);
    if (rc) return rc;
    rc = v2_run(c, p, false);   // (the finish kernel writes every word of d_out)
    if (rc) return rc;
    rc = read_bits(c, bitfield_out);
    if (rc) return rc;
    return finish_timing(c);
}

int tv_v2_hash(tv_ctx* c, uint8_t* roots_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = v2_require(c, "tv_v2_hash");
    if (rc) return rc;
    if (!c->v2_set) return fail(c, TV_ERR_STATE, "tv_v2_set_pieces has not been called for this layout");
    if (!roots_out && c->count) return fail(c, TV_ERR_ARG, "roots_out is NULL");
    if (!c->count) return TV_OK;
    TV_HIP(c, hipSetDevice(c->device));
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    TvV2 p = v2_launch_args(c);
    rc = v2_run(c, p, true);
    if (rc) return rc;
    std::vector<uint32_t> soa(8 * c->count);
    DrainGuard drain(c);  // declared after soa: drains before soa is freed, also on error paths
    TV_HIP(c, hipMemcpyAsync(soa.data(), p.roots, soa.size() * 4, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
    TV_HIP(c, hipEventSynchronize(c->ev_call1));
    for (uint64_t j = 0; j < c->count; j++) digest_unpack(soa.data(), c->count, j, 8, roots_out + 32 * j);
    return finish_timing(c);
}

int tv_v2_verify_list(tv_ctx* c, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                      const uint32_t* tree_leaves, const uint8_t* hashes, uint8_t* ok_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, false, true);
    if (rc) return rc;
    if (c->win)
        return fail(c, TV_ERR_STATE, "tv_v2_verify_list needs the shard resident or a slot pool (TV_OPT_LIST_SLOTS); "
                                     "this layout is windowed (the shard exceeds the device budget)");
    if (n == 0) return TV_OK;
    if (!pieces || !piece_bytes || !tree_leaves || !hashes || !ok_out) return fail(c, TV_ERR_ARG, "NULL argument");
    // every entry is checked before anything is launched or freed: a refused call changes nothing
    rc = v2_list_check(c, "tv_v2_verify_list", n, pieces, piece_bytes, tree_leaves);
    if (rc) return rc;
    V2List l;
    v2_list_plan(c, n, pieces, piece_bytes, tree_leaves, hashes, ok_out, &l);
    TV_HIP(c, hipSetDevice(c->device));
    if (l.m) {
        DrainGuard drain(c);  // after the host vectors: their H2D / D2H copies end before they go
        rc = v2_list_reserve(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
        rc = v2_list_upload(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
        rc = v2_list_launch(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
        rc = v2_list_download(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
        TV_HIP(c, hipEventSynchronize(c->ev_call1));
    } else {
        c->last_workgroups = 0;
    }
    v2_list_scatter(l, ok_out);
    list_zero_unread(c, n, pieces, ok_out);
    list_release(c, n, pieces);
    return list_finish(c, TV_KERNEL_V2_LIST, l.m);
}

int tv_v2_leaf_hashes(tv_ctx* c, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                      const uint32_t* tree_leaves, uint8_t* leaves_out, int release) {
    return v2_blocks_call(c, "tv_v2_leaf_hashes", false, n, pieces, piece_bytes, tree_leaves, nullptr, nullptr,
                          leaves_out, release);
}

int tv_v2_check_blocks(tv_ctx* c, uint64_t n, const uint64_t* pieces, const uint32_t* piece_bytes,
                       const uint32_t* tree_leaves, const uint8_t* leaf_hashes, const uint8_t* want_bits,
                       uint8_t* ok_bits_out, int release) {
    return v2_blocks_call(c, "tv_v2_check_blocks", true, n, pieces, piece_bytes, tree_leaves, leaf_hashes, want_bits,
                          ok_bits_out, release);
}

}  // extern "C"
