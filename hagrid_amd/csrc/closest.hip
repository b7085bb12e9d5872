// closest.hip -- nearest-surface queries: for every point of a batch the nearest triangle within its radius, the squared distance, the
// closest point, the feature that holds it and the side (include/hagrid_amd.h: hagrid_closest_points; arithmetic, semantics, the walk and
// the argument why its pruning is sound: include/hagrid/closest.h).  No counterpart in the reference.
//
// The kernel is the header's closest_query with device loads: one query per lane, one wavefront per workgroup, the XCD-aware block ->
// range map and the streaming 16-byte loads / stores of trav_multi.hip.  It walks the construction format (entries -> cells | small_cells
// -> ref_ids); the cell format is a kernel argument: ONE kernel (the product library's kernel budget, tests/test_abi.py).  The descent
// into an entry's sub-blocks keeps a stack of (node word, next child) per level in LDS, laid out [level][lane]: a lane only ever touches
// its own column, so there is nothing to synchronise, 64 lanes at one level read 64 consecutive words (no bank conflict), and no register
// array is indexed at run time (no scratch).  8 KB of LDS per wavefront: 20 wavefronts per CU by LDS, which the registers allow as well
// (DESIGN.md 4.6).  Queries are processed in buffer order: no binning, no traversal image, no hints -- each answer depends on its query alone.
//
// nearest_tris_kernel (hagrid_nearest_tris) is the same walk with the header's NearList as its accumulator: the k <= 8 nearest candidates of
// every point, sorted, after a cursor, with label pairs skipped.  The list (8 ids, 8 distances) lives in registers; the 32-byte records are made again from
// the winners' ids AFTER the walk, so q, feature and side cost no register at the walk's peak.  A kernel of its own: as a mode of closest_points_kernel the
// list would take every nearest-surface launch from 5 wavefronts per SIMD to 4.
#include "trav_common.h"
#include "wave_prims.h"

#include "hagrid/closest.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hc = hagrid::closest;

namespace {

__global__ void __launch_bounds__(64) closest_points_kernel(const DevGrid g, const float4* __restrict__ points, float4* __restrict__ results, const int n,
                                                            unsigned long long* __restrict__ counters) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < n;
    hc::Counts cnt;
    cnt.cells = 0; cnt.tris = 0; cnt.pruned = 0;
    if (live) {
        const float4 pr = nt_load4(points + id);
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        hc::Best b;
        hc::closest_query(g, st, vec3(pr.x, pr.y, pr.z), pr.w, b, cnt);
        nt_store4(results + 2 * size_t(id), b.q.x, b.q.y, b.q.z, b.d2);
        nt_store4(results + 2 * size_t(id) + 1, __int_as_float(b.id), __int_as_float(b.feature), float(b.side), 0.0f);
    }
    if (counters) add_batch_counters(counters, lane, live ? 1 : 0, cnt.cells, cnt.tris, cnt.pruned);
}

__global__ void __launch_bounds__(64) nearest_tris_kernel(const DevGrid g, const ListArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    hc::Counts cnt;
    cnt.cells = 0; cnt.tris = 0; cnt.pruned = 0;
    int full = 0;
    if (live) {
        const float4 pr = nt_load4(a.queries + id);
        const vec3 p(pr.x, pr.y, pr.z);
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        hc::NearList<HAGRID_MAX_NEAREST> list;
        float cur_d2 = -1.0f;
        int cur_id = -1;
        if (a.cursors) { const float2 c = a.cursors[id]; cur_d2 = c.x; cur_id = __float_as_int(c.y); }
        list.setup(a.k, cur_d2, cur_id, a.query_labels ? a.query_labels[id] : -1, a.tri_labels);
        hc::closest_query(g, st, p, pr.w, list, cnt);
        full = list.full() ? 1 : 0;
        const size_t base = size_t(id) * size_t(a.k);
#pragma nounroll
        for (int j = 0; j < a.k; j++) {
            int sid; float sd2;
            list.get(j, sid, sd2);
            if (a.entries) nt_store2(a.entries + base + j, sd2, __int_as_float(sid));
            if (a.records) {
                hc::Best b;
                hc::slot_record([&g](int t) { return g.tri(t); }, sid, sd2, p, b);
                nt_store4(a.records + 2 * (base + j), b.q.x, b.q.y, b.q.z, b.d2);
                nt_store4(a.records + 2 * (base + j) + 1, __int_as_float(b.id), __int_as_float(b.feature), float(b.side), 0.0f);
            }
        }
    }
    if (a.counters) add_batch_counters(a.counters, lane, live ? 1 : 0, cnt.cells, cnt.tris, cnt.pruned, full);
}

} // namespace

extern "C" int hagrid_closest_points(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, void* results, int num_points,
                                     void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (flags) HG_FAIL(ctx, HAGRID_EINVAL, "closest_points: unknown flag (flags must be 0)");
    if (num_points < 0) HG_FAIL(ctx, HAGRID_EINVAL, "closest_points: negative num_points");
    HG_TRY(check_walk_grid(ctx, "closest_points", grid));
    if (!aligned(counters, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "closest_points: the counters must be 8-byte aligned");
    if (num_points == 0) return HAGRID_OK;
    if (!tris || !points || !results) HG_FAIL(ctx, HAGRID_EINVAL, "closest_points: null triangle, point or result buffer");
    if (!aligned(tris, 16) || !aligned(points, 16) || !aligned(results, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "closest_points: triangles, points and results must be 16-byte aligned");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    DevGrid g;
    g.set(grid, tris);
    closest_points_kernel<<<grid_blocks(num_points, 64), 64, 0, ctx->stream>>>(g, static_cast<const float4*>(points), static_cast<float4*>(results), num_points,
                                                                                static_cast<unsigned long long*>(counters));
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_nearest_tris(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, int num_points, int k, const void* cursors,
                                   const void* query_labels, const void* tri_labels, void* entries, void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    return launch_lists(ctx, "nearest_tris", "point", nearest_tris_kernel, grid, tris, points, num_points, k, cursors, query_labels, tri_labels, entries, records, counters, flags);
}
