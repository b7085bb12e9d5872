// overlap_lists.hip -- overlap lists: EVERY triangle that meets each box, contact query or oriented box, ascending by id, in CSR form, without paging
// (include/hagrid_amd.h: hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs; the list type and the duplicate model: include/hagrid/overlap.h, RefList;
// DESIGN.md 4.18).  No counterpart in the reference.
//
// This is stage 1 of the protocol of the ball lists (ball_lists.hip): count -> scan -> fill, then hagrid_unique_lists -> scan -> hagrid_compact_lists, which
// are reused as they are -- a reference is stored as the 8-byte entry {+0.0f, id}, so the second stage's order (d2, id) is the order by id.  Both scans are the
// caller's and so is every buffer: no entry point here asks for memory.
//
// overlap_refs_kernel is the header's overlap_query, textually the walk of the k-list kernels (overlap.hip), with RefList as its list: one query per lane, one
// wavefront per workgroup, the XCD-aware block -> range map, the LDS stack [level][lane], streaming loads of the records and one streaming 8-byte store per
// reference while the query's room lasts.  A lane keeps no id: the address of its first slot, its room and its count.  Boxes, contact queries and oriented
// boxes, count mode and fill mode, Cell and SmallCell grids: launch-uniform arguments of ONE kernel (the product library's kernel budget, tests/test_abi.py) --
// without the eight ids of the k-list the three shapes fit one register budget, which the k-list kernels do not (overlap.hip).
#include "overlap_dev.h"
#include "wave_prims.h"

#include "hagrid/crossings.h"
#include "hagrid/unique_lists.h"

#include <string>

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hc = hagrid::closest;
namespace ho = hagrid::overlap;
namespace hb = hagrid::obb;
namespace hl = hagrid::lists;

namespace {

struct RefsArgs {
    const float4* __restrict__ boxes;           // one of the three is given: 32-byte box records,
    const float4* __restrict__ queries;         // 48-byte Tri records (the contact form),
    const float4* __restrict__ obbs;            // 64-byte oriented-box records
    const int* __restrict__ first;              // contact form: `first` per query, may be null
    const int* __restrict__ query_labels;       // contact form: three per query; oriented boxes: one per query; both label arrays given or both null
    const int* __restrict__ tri_labels;
    const long long* __restrict__ offsets;      // null: count mode
    int* __restrict__ counts;                   // may be null in fill mode
    float2* __restrict__ entries;
    long long capacity;
    unsigned long long* __restrict__ counters;
    int n;
};

// RefList's store: the query's first slot is made before the walk and carried through it (two registers); the distance word of the entry is +0.0f
struct RefStore {
    float2* slots;
    __device__ __forceinline__ void operator()(int position, int id) const { nt_store2(slots + position, 0.0f, __int_as_float(id)); }
};
typedef ho::RefList<RefStore> Refs;

// the range of query i: crossings.h's slot_range in its CSR form -- the room rule is hagrid_list_crossings', word for word
__device__ __forceinline__ void hx_range(const RefsArgs& a, int i, long long& first, long long& room) { hagrid::crossings::slot_range(a.offsets, 0, a.capacity, i, first, room); }

// boxes and contact queries: the filter is launch-uniform, as in overlap_boxes_kernel
__device__ __forceinline__ void walk_box(const OverlapGrid& g, LdsStack& st, const RefsArgs& a, int id, Refs& list, ho::Counts& cnt) {
    vec3 lo, hi;
    int first = 0;
    bool active = true;
    DevFilter filter;
    filter.on = a.queries != nullptr;
    filter.f.q.queries = a.queries; filter.f.q.labels = a.query_labels; filter.f.q.tri_labels = a.tri_labels;
    filter.f.q.i = id;
    if (a.queries) {
        active = ho::query_box(filter.f.q.tri(), g.c.eps, lo, hi);
        if (a.first) first = __builtin_nontemporal_load(a.first + id);
    } else {
        const float4 b0 = nt_load4(a.boxes + 2 * size_t(id)), b1 = nt_load4(a.boxes + 2 * size_t(id) + 1);
        lo = vec3(b0.x, b0.y, b0.z); hi = vec3(b1.x, b1.y, b1.z);
        first = __float_as_int(b0.w);
    }
    list.init(first);
    if (active) ho::overlap_query(g, st, lo, hi, false, list, cnt, filter);
}

// oriented boxes: ObbFilter plus FacePrune, as in obb_tris_kernel
__device__ __forceinline__ void walk_obb(const OverlapGrid& g, LdsStack& st, const RefsArgs& a, int id, Refs& list, ho::Counts& cnt) {
    vec3 lo, hi;
    hb::ObbFilter<DevObb> filter;
    filter.q.obbs = a.obbs; filter.q.labels = a.query_labels; filter.q.tri_labels = a.tri_labels; filter.q.i = id;
    hb::FacePrune<DevObb> prune;
    bool active;
    int first;
    {
        const float4 r0 = nt_load4(a.obbs + 4 * size_t(id)), r1 = nt_load4(a.obbs + 4 * size_t(id) + 1), r2 = nt_load4(a.obbs + 4 * size_t(id) + 2),
                     r3 = nt_load4(a.obbs + 4 * size_t(id) + 3);
        hb::Obb b;
        b.c = vec3(r0.x, r0.y, r0.z); b.u = vec3(r1.x, r1.y, r1.z); b.v = vec3(r2.x, r2.y, r2.z); b.w = vec3(r3.x, r3.y, r3.z);
        first = __float_as_int(r0.w);
        active = hb::obb_box(b, g.c.eps, lo, hi);
        prune.set(filter.q, b, g.c.eps, true);
    }
    list.init(first);
    if (active) ho::overlap_query(g, st, lo, hi, false, list, cnt, filter, prune);
}

__global__ void __launch_bounds__(64) overlap_refs_kernel(const OverlapGrid g, const RefsArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    ho::Counts cnt;
    cnt.cells = 0; cnt.sats = 0; cnt.pruned = 0;
    int written = 0, is_short = 0;
    if (live) {
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        long long first = 0, room = 0;
        if (a.offsets) hx_range(a, id, first, room);
        Refs list;
        list.store.slots = a.entries + first;
        list.room = int(room < 0x7fffffffLL ? room : 0x7fffffffLL);
        if (a.obbs) walk_obb(g, st, a, id, list, cnt);
        else walk_box(g, st, a, id, list, cnt);
        const int refs = list.count;
        if (a.counts) __builtin_nontemporal_store(refs, a.counts + id);
        if (a.offsets) {            // the slots the references left over get the empty entry
            written = refs < list.room ? refs : list.room;
            is_short = refs > list.room ? 1 : 0;
            int again = id;
            HAGRID_MADE_HERE(again);         // the range once more, from the query's number (as crossings.hip)
            hx_range(a, again, first, room);
            const hl::Entry none = hl::empty_entry();
            for (long long s = written; s < room; s++) nt_store2(a.entries + first + s, none.d2, __int_as_float(none.id));
        }
    }
    if (a.counters) {
        add_batch_counters(a.counters, lane, live ? 1 : 0, cnt.cells, cnt.sats, cnt.pruned);
        const unsigned long long sw = wave_sum_u64((unsigned)written), ss = wave_sum_u64((unsigned)is_short);
        if (lane == 0) { atomicAdd(a.counters + 4, sw); atomicAdd(a.counters + 5, ss); }
    }
}

// what the three entry points check and do: the refusals of the k-list query of the same shape (overlap.hip) and those of hagrid_ball_refs (ball_lists.hip)
int launch(hagrid_ctx* ctx, const char* who, const hagrid_grid* grid, const void* tris, RefsArgs a, const void* records, const void* offsets, void* counts, void* entries,
           int64_t capacity, void* counters, uint32_t flags) {
    const std::string w(who);
    if (flags) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": unknown flag (flags must be 0)").c_str());
    if (a.n < 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": negative number of queries").c_str());
    if (capacity < 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": negative capacity").c_str());
    HG_TRY(check_walk_grid(ctx, who, grid));
    if (!offsets && (entries || capacity != 0)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": count mode (offsets == NULL) takes no entries and a capacity of 0").c_str());
    if ((a.query_labels != nullptr) != (a.tri_labels != nullptr)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": query_labels and tri_labels are given together or not at all").c_str());
    if (!aligned(counters, 8) || !aligned(offsets, 8) || !aligned(entries, 8)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": counters, offsets and entries must be 8-byte aligned").c_str());
    if (!aligned(counts, 4) || !aligned(a.first, 4) || !aligned(a.query_labels, 4) || !aligned(a.tri_labels, 4))
        HG_FAIL(ctx, HAGRID_EINVAL, (w + ": counts, first and the labels must be 4-byte aligned").c_str());
    if (!aligned(tris, 16) || !aligned(records, 16)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": triangles and query records must be 16-byte aligned").c_str());
    if (a.n == 0) return HAGRID_OK;
    if (!tris || !records) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null triangle or query buffer").c_str());
    if (!offsets && !counts) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": count mode needs counts").c_str());
    if (offsets && !entries && capacity > 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null output buffer").c_str());
    HG_HIP(ctx, hipSetDevice(ctx->device));
    OverlapGrid g;
    g.set(grid, tris);
    g.clip.set(g.c.lo, g.c.hi);
    a.offsets = static_cast<const long long*>(offsets); a.counts = static_cast<int*>(counts);
    a.entries = static_cast<float2*>(entries); a.capacity = capacity;
    a.counters = static_cast<unsigned long long*>(counters);
    overlap_refs_kernel<<<grid_blocks(a.n, 64), 64, 0, ctx->stream>>>(g, a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

} // namespace

extern "C" int hagrid_box_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* boxes, int num_boxes, const void* offsets, void* counts, void* entries,
                               int64_t capacity, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    RefsArgs a = {};
    a.boxes = static_cast<const float4*>(boxes);
    a.n = num_boxes;
    return launch(ctx, "box_refs", grid, tris, a, boxes, offsets, counts, entries, capacity, counters, flags);
}

extern "C" int hagrid_tri_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* queries, int num_queries, const void* first, const void* query_labels,
                               const void* tri_labels, const void* offsets, void* counts, void* entries, int64_t capacity, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    RefsArgs a = {};
    a.queries = static_cast<const float4*>(queries);
    a.first = static_cast<const int*>(first);
    a.query_labels = static_cast<const int*>(query_labels); a.tri_labels = static_cast<const int*>(tri_labels);
    a.n = num_queries;
    return launch(ctx, "tri_refs", grid, tris, a, queries, offsets, counts, entries, capacity, counters, flags);
}

extern "C" int hagrid_obb_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* obbs, int num_obbs, const void* query_labels, const void* tri_labels,
                               const void* offsets, void* counts, void* entries, int64_t capacity, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    RefsArgs a = {};
    a.obbs = static_cast<const float4*>(obbs);
    a.query_labels = static_cast<const int*>(query_labels); a.tri_labels = static_cast<const int*>(tri_labels);
    a.n = num_obbs;
    return launch(ctx, "obb_refs", grid, tris, a, obbs, offsets, counts, entries, capacity, counters, flags);
}
