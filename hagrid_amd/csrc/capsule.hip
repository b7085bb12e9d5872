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

__global__ void __launch_bounds__(64) segment_tris_kernel(const DevGrid g, const ListArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    hc::Counts cnt;
    cnt.cells = 0; cnt.tris = 0; cnt.pruned = 0;
    int full = 0;
    if (live) {
        const float4 s0 = nt_load4(a.queries + 2 * size_t(id)), s1 = nt_load4(a.queries + 2 * size_t(id) + 1);
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
    return launch_lists(ctx, "segment_tris", "segment", segment_tris_kernel, grid, tris, segments, num_segments, k, cursors, query_labels, tri_labels, entries, records, counters, flags);
}
