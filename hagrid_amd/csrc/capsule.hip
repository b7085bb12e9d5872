// capsule.hip -- capsule queries: for every segment of a batch the k nearest triangles within its radius, nearest first, paged (include/hagrid_amd.h:
// hagrid_segment_tris; arithmetic, semantics, the walk and the argument why its pruning is sound: include/hagrid/capsule.h).  No counterpart in
// the reference.
//
// segment_tris_kernel has nearest_tris_kernel's shape (closest.hip): one query per lane, one wavefront per workgroup, the XCD-aware block -> range map, the
// LDS stack [level][lane], streaming 16-byte loads and stores, vector stores only, counters through add_batch_counters.  The walk is capsule.h's segment_query
// with SegList (NearList and a second label) as its accumulator; the list stays (d2, id): s, q, feature and side are made again from the winners' ids AFTER
// the walk.  A kernel of its own: as a launch-uniform mode of nearest_tris_kernel it cost hagrid_nearest_tris 1.6 to 3.1 % (the allocation of the whole
// kernel: 125 VGPRs instead of 103, 133 instead of 48 scalar registers spilled into vector lanes).  Its slot in the kernel budget: frame.hip.
#include "trav_common.h"
#include "wave_prims.h"

#include "hagrid/capsule.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hc = hagrid::closest;
namespace cap = hagrid::capsule;

namespace {

struct SegmentArgs {
    const float4* __restrict__ segments;    ///< two float4 per query: a, r; b, 0
    const float2* __restrict__ cursors;
    const int* __restrict__ query_labels;   ///< two per query
    const int* __restrict__ tri_labels;
    float2* __restrict__ entries;
    float4* __restrict__ records;
    unsigned long long* __restrict__ counters;
    int n, k;
};

__global__ void __launch_bounds__(64) segment_tris_kernel(const DevGrid g, const SegmentArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    hc::Counts cnt;
    cnt.cells = 0; cnt.tris = 0; cnt.pruned = 0;
    int full = 0;
    if (live) {
        const float4 s0 = nt_load4(a.segments + 2 * size_t(id)), s1 = nt_load4(a.segments + 2 * size_t(id) + 1);
        const vec3 pa(s0.x, s0.y, s0.z), pb(s1.x, s1.y, s1.z);
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        cap::SegList<HAGRID_MAX_NEAREST> list;
        float cur_d2 = -1.0f;
        int cur_id = -1;
        if (a.cursors) { const float2 c = a.cursors[id]; cur_d2 = c.x; cur_id = __float_as_int(c.y); }
        list.setup(a.k, cur_d2, cur_id, a.query_labels ? a.query_labels[2 * size_t(id)] : -1, a.query_labels ? a.query_labels[2 * size_t(id) + 1] : -1, a.tri_labels);
        cap::segment_query(g, st, pa, pb, s0.w, list, cnt);
        full = list.full() ? 1 : 0;
        const size_t base = size_t(id) * size_t(a.k);
#pragma nounroll
        for (int j = 0; j < a.k; j++) {
            int sid; float sd2;
            list.get(j, sid, sd2);
            if (a.entries) nt_store2(a.entries + base + j, sd2, __int_as_float(sid));
            if (a.records) {
                cap::SegRecord o;
                cap::slot_record([&g](int t) { return g.tri(t); }, sid, sd2, pa, pb, o);
                nt_store4(a.records + 2 * (base + j), o.q.x, o.q.y, o.q.z, o.d2);
                nt_store4(a.records + 2 * (base + j) + 1, __int_as_float(o.id), __int_as_float(o.feature), float(o.side), o.s);
            }
        }
    }
    if (a.counters) add_batch_counters(a.counters, lane, live ? 1 : 0, cnt.cells, cnt.tris, cnt.pruned, full);
}

} // namespace

extern "C" int hagrid_segment_tris(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* segments, int num_segments, int k, const void* cursors,
                                   const void* query_labels, const void* tri_labels, void* entries, void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (flags) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: unknown flag (flags must be 0)");
    if (num_segments < 0) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: negative num_segments");
    if (k < 1 || k > HAGRID_MAX_NEAREST) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: k must be 1 .. HAGRID_MAX_NEAREST");
    if (!grid) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: null grid");
    if (!grid->entries || (!grid->cells && !grid->small_cells)) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: the walk reads the construction format (grid released for traversal, or incomplete)");
    if (!grid->ref_ids) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: incomplete grid");
    if (grid->shift < 0 || grid->shift > 15 || grid->dims[0] <= 0 || grid->dims[1] <= 0 || grid->dims[2] <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: bad shift or dims");
    if (!aligned(counters, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: the counters must be 8-byte aligned");
    if ((query_labels != nullptr) != (tri_labels != nullptr)) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: query_labels and tri_labels are given together or not at all");
    if (int64_t(num_segments) * int64_t(k) > int64_t(INT32_MAX)) HG_FAIL(ctx, HAGRID_ERANGE, "segment_tris: num_segments * k beyond 2^31 - 1");
    if (num_segments == 0) return HAGRID_OK;
    if (!tris || !segments) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: null triangle or segment buffer");
    if (!entries && !records) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: entries and records are both null");
    if (!aligned(tris, 16) || !aligned(segments, 16) || !aligned(records, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: triangles, segments and records must be 16-byte aligned");
    if (!aligned(entries, 8) || !aligned(cursors, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: entries and cursors must be 8-byte aligned");
    if (!aligned(query_labels, 4) || !aligned(tri_labels, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "segment_tris: the labels must be 4-byte aligned");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    DevGrid g;
    g.set(grid, tris);
    SegmentArgs a;
    a.segments = static_cast<const float4*>(segments); a.cursors = static_cast<const float2*>(cursors);
    a.query_labels = static_cast<const int*>(query_labels); a.tri_labels = static_cast<const int*>(tri_labels);
    a.entries = static_cast<float2*>(entries); a.records = static_cast<float4*>(records); a.counters = static_cast<unsigned long long*>(counters);
    a.n = num_segments; a.k = k;
    segment_tris_kernel<<<grid_blocks(num_segments, 64), 64, 0, ctx->stream>>>(g, a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}
