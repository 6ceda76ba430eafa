// tv_verify.hip -- the verify and hash calls (tv_verify, tv_verify_list, tv_hash): one launch over the resident
// shard, a list of resident / slotted pieces, or the compare that ends a windowed pass.
#include <cstring>

#include "tv_ctx.h"

using namespace tvi;

namespace tvi {

// ---- the launch parts of tv_verify_list (tv_ctx.h: V1List), shared with tv_hybrid_verify_list ---------------------------

// The entries launched: every listed piece, or, in a slot pool, the listed pieces that hold a slot (the others were
// never staged: 0), in tv_plan.h list_plan's order (a short last piece in waves of its own).
int v1_list_plan(tv_ctx* c, uint64_t n, const uint64_t* pieces, uint8_t* ok_out, V1List* l) {
    std::vector<uint32_t> local(n);
    for (uint64_t k = 0; k < n; k++) {
        const int rc = list_in_shard(c, pieces[k]);
        if (rc) return rc;
        local[k] = (uint32_t)(pieces[k] - c->first);
    }
    std::vector<uint8_t> held(c->slots ? n : 0);
    for (uint64_t k = 0; k < held.size(); k++) {
        held[k] = list_held(c, local[k]);
        if (!held[k]) ok_out[k] = 0;
    }
    const bool short_last = c->first + c->count == c->P && piece_len(c, c->P - 1) != c->L;
    list_plan(n, local.data(), c->slots ? held.data() : nullptr, short_last ? c->count - 1 : UINT64_MAX, &l->launch,
              &l->origin);
    l->m = l->launch.size();
    if (c->slots)  // the rows: each entry's slot (the kernels read piece launch[j]'s bytes from slot rows[j])
        for (uint64_t j = 0; j < l->m; j++) l->launch.push_back(list_row(c, l->launch[j]));
    l->ok.assign(l->m, 0);
    return TV_OK;
}

int v1_list_reserve(tv_ctx* c, const V1List& l) {
    int rc = grow_buf(c, c->d_list, l.m, false, std::max<uint64_t>(l.m, 1024));
    if (!rc) rc = grow_buf(c, c->d_list_out, l.m, false, std::max<uint64_t>(l.m, 1024));
    return rc;
}

int v1_list_upload(tv_ctx* c, const V1List& l) {
    TV_HIP(c, hipMemcpyAsync(c->d_list.ptr, l.launch.data(), l.launch.size() * 4, hipMemcpyHostToDevice, c->stream));
    return TV_OK;
}

int v1_list_launch(tv_ctx* c, const V1List& l, int* kernel_out) {
    const uint64_t m = l.m;
    uint32_t* d_list = c->d_list.get<uint32_t>();
    TvPieces p = resident_launch(c);
    p.n = (uint32_t)m;
    p.n_main = (uint32_t)m;
    p.idx = d_list;
    p.rows = c->slots ? d_list + m : nullptr;
    p.clock = nullptr;
    p.out_bytes = c->d_list_out.get<uint8_t>();
    // twin (two lanes per piece) while its 2-wave workgroups fit two per CU, then split (rounds + helper pair,
    // ~30 % shorter serial stream per block than lane) while one pair per CU suffices, like choose_kernel;
    // the lane list kernel for longer lists
    const int kernel = (c->kernel_opt == TV_KERNEL_LANE || c->kernel_opt == TV_KERNEL_SPLIT ||
                        c->kernel_opt == TV_KERNEL_TWIN)
                           ? c->kernel_opt
                           : (m <= 64 * (uint64_t)c->cus ? TV_KERNEL_TWIN : (m <= 256 * 64 ? TV_KERNEL_SPLIT : TV_KERNEL_LANE));
    // Companions (as resident launches) only for a list that gives every CU a workgroup: a shorter one would
    // fill 2 x CUs workgroups with copies re-hashing the same few pieces (a 1-piece flush: 512 copies) for a
    // ~4 % shorter flush (r03 latency: tools/latency_probe.py)
    const uint64_t list_wgs = (m + 31) / 32;
    if (kernel == TV_KERNEL_TWIN && (c->twin_fill == 2 || ((c->twin_fill == 1 || c->twin_fill == 3) &&
                                                            list_wgs >= (uint64_t)c->cus && companions_on(c)))) {
        p.fill_to = 2u * (uint32_t)c->cus;
        p.fill_all = c->fill_all ? 1u : 0u;
    }
    TV_HIP(c, tv_launch_verify_list(p, kernel, c->stream, &c->last_workgroups));
    *kernel_out = kernel;
    return TV_OK;
}

int v1_list_download(tv_ctx* c, V1List& l) {
    TV_HIP(c, hipMemcpyAsync(l.ok.data(), c->d_list_out.ptr, l.m, hipMemcpyDeviceToHost, c->stream));
    return TV_OK;
}

void v1_list_scatter(const V1List& l, uint8_t* ok_out) {
    for (uint64_t i = 0; i < l.m; i++)
        if (l.origin[i] >= 0) ok_out[l.origin[i]] = l.ok[i];
}

}  // namespace tvi

extern "C" {

int tv_verify(tv_ctx* c, const uint8_t* avail_bits, uint8_t* bitfield_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, true, true);
    if (rc) return rc;
    if (!bitfield_out && c->count) return fail(c, TV_ERR_ARG, "bitfield_out is NULL");
    if (!c->count) return TV_OK;
    if (c->slots) return fail(c, TV_ERR_STATE, "tv_verify: a slot pool (TV_OPT_LIST_SLOTS) verifies with tv_verify_list");
    TV_HIP(c, hipSetDevice(c->device));
    const uint64_t* av = nullptr;
    if (c->win) {
        // windowed: end the pass (its windows hashed into d_hash as they filled), then compare the whole shard
        rc = win_finalize(c);
        if (!rc) rc = launch_avail(c, avail_bits, &av);
        if (rc) return rc;
        TV_HIP(c, tv_launch_compare(c->d_hash, c->d_digests, (uint32_t)c->count, (uint32_t)c->count, av, c->d_out,
                                    c->stream));
        rc = read_bits(c, bitfield_out);
        if (rc) return rc;
        c->last_launches = (int)c->win_launched;
        return finish_timing(c);
    }
    TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
    rc = launch_avail(c, avail_bits, &av);
    if (rc) return rc;
    const int kernel = choose_kernel(c);
    TvPieces p = resident_launch(c);
    p.avail64 = av;
    // fail closed: a piece the launch does not write reads as 0, never as a stale 1
    TV_HIP(c, hipMemsetAsync(c->d_out, 0, c->bit_words * 8, c->stream));
    TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
    rc = launch_resident(c, p, kernel, false);
    if (rc) return rc;
    TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
    rc = read_bits(c, bitfield_out);
    if (rc) return rc;
    c->last_kernel = kernel;
    c->last_launches = 1;
    return finish_timing(c);
}

int tv_verify_list(tv_ctx* c, const uint64_t* pieces, uint64_t n, uint8_t* ok_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, true, true);
    if (rc) return rc;
    if (n == 0) return TV_OK;
    if (!pieces || !ok_out) return fail(c, TV_ERR_ARG, "NULL argument");
    if (n >= 0xFFFFFFFFull) return fail(c, TV_ERR_ARG, "list too long");
    if (c->win)
        return fail(c, TV_ERR_STATE, "tv_verify_list needs the shard resident or a slot pool (TV_OPT_LIST_SLOTS); "
                                     "this layout is windowed (the shard exceeds the device budget)");
    V1List l;
    rc = v1_list_plan(c, n, pieces, ok_out, &l);
    if (rc) return rc;
    TV_HIP(c, hipSetDevice(c->device));
    int kernel = 0;
    if (l.m) {
        DrainGuard drain(c);  // after the host vectors: their H2D / D2H copies end before they go
        rc = v1_list_reserve(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
        rc = v1_list_upload(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
        rc = v1_list_launch(c, l, &kernel);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
        rc = v1_list_download(c, l);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
        TV_HIP(c, hipEventSynchronize(c->ev_call1));
    }
    v1_list_scatter(l, ok_out);
    list_zero_unread(c, n, pieces, ok_out);   // (recover_segment's marks)
    list_release(c, n, pieces);
    return list_finish(c, kernel, l.m);
}

int tv_hash(tv_ctx* c, uint8_t* digests_out) {
    if (!c) return fail(nullptr, TV_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> g(c->mu);
    int rc = require_layout(c, false, true);
    if (rc) return rc;
    if (!digests_out && c->count) return fail(c, TV_ERR_ARG, "digests_out is NULL");
    if (!c->count) return TV_OK;
    if (c->slots) return fail(c, TV_ERR_STATE, "tv_hash: a slot pool (TV_OPT_LIST_SLOTS) holds no shard");
    TV_HIP(c, hipSetDevice(c->device));
    int kernel = 0;
    if (c->win) {
        rc = win_finalize(c);  // windowed: the windows were hashed into d_hash as they filled
        if (rc) return rc;
        kernel = c->last_kernel;
    } else {
        TV_HIP(c, hipEventRecord(c->ev_call0, c->stream));
        kernel = choose_kernel(c);
        TvPieces p = resident_launch(c);
        p.avail64 = nullptr;
        TV_HIP(c, hipEventRecord(c->ev_k0, c->stream));
        rc = launch_resident(c, p, kernel, true);
        if (rc) return rc;
        TV_HIP(c, hipEventRecord(c->ev_k1, c->stream));
    }
    std::vector<uint32_t> soa(5 * c->count);
    DrainGuard drain(c);  // declared after soa: drains before soa is freed, also on error paths
    TV_HIP(c, hipMemcpyAsync(soa.data(), c->d_hash, soa.size() * 4, hipMemcpyDeviceToHost, c->stream));
    TV_HIP(c, hipEventRecord(c->ev_call1, c->stream));
    TV_HIP(c, hipEventSynchronize(c->ev_call1));
    for (uint64_t j = 0; j < c->count; j++) digest_unpack(soa.data(), c->count, j, 5, digests_out + 20 * j);
    c->last_kernel = kernel;
    c->last_launches = c->win ? (int)c->win_launched : 1;
    return finish_timing(c);
}

}  // extern "C"
