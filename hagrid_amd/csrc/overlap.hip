// overlap.hip -- box-overlap queries: for every box of a batch the k smallest ids of the triangles that meet it (include/hagrid_amd.h:
// hagrid_overlap_boxes, hagrid_overlap_lattice; the test, the list, the walk and the argument why it is sound: include/hagrid/overlap.h).
// No counterpart in the reference.
//
// The kernel is the header's overlap_query with device loads, in the shape of closest.hip: one box per lane, one wavefront per workgroup, the
// XCD-aware block -> range map, streaming 16-byte loads of the box records and streaming stores of the ids.  It walks the construction format
// (entries -> cells | small_cells -> ref_ids).  k, the cell format, ANY and "boxes from a buffer or from lattice constants" are kernel arguments,
// uniform over the launch: ONE kernel (the product library's kernel budget, tests/test_abi.py).  The id list lives in eight registers -- every loop
// over it runs over compile-time indices, k only appears in comparisons with them -- and the descent's stack of (node word, next child) per level in
// LDS, laid out [level][lane]: a lane only ever touches its own column, so there is nothing to synchronise, 64 lanes at one level read 64 consecutive
// words (no bank conflict) and no register array is indexed at run time (no scratch).  8 KB of LDS per wavefront: 20 wavefronts per CU by LDS
// (DESIGN.md 4.7).  Boxes are processed in buffer order: no binning, no traversal image, no hints -- each answer depends on its box alone.
//
// The CONTACT form (hagrid_overlap_tris) is a launch-uniform mode of the same kernel: the lane forms its box from its query's Tri record
// (overlap.h: query_box) and every triangle that has met the box passes the pair filter -- labels, surface, tri_meets of hagrid/tri_tri.h -- before the list
// takes it.  The query record is read again for every such candidate instead of being held across the walk, and the 17 axes are evaluated one at a time in
// rolled loops; the kernel is compiled for four wavefronts per SIMD (amdgpu_waves_per_eu), which the allocator meets with 128 VGPRs and no scratch.
//
// ORIENTED BOXES (hagrid_overlap_obbs, DESIGN.md 4.16, include/hagrid/obb.h) have a kernel of their own further down, obb_tris_kernel: the one above has no
// register left for a third mode.  The accessors the kernels read grid and queries through (OverlapGrid, DevQuery, DevFilter, DevObb) are overlap_dev.h's,
// shared with overlap_lists.hip.
#include "overlap_dev.h"
#include "wave_prims.h"

#include <string>

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hc = hagrid::closest;
namespace ho = hagrid::overlap;
namespace hb = hagrid::obb;

namespace {

struct OverlapArgs {
    const float4* __restrict__ boxes;        // null: the lattice form
    int* __restrict__ ids;
    int* __restrict__ counts;                // may be null
    unsigned long long* __restrict__ counters;   // may be null
    const float4* __restrict__ queries;      // not null: the contact form -- Tri records ask, `boxes` is null
    const int* __restrict__ first;           // contact form: `first` per query, may be null
    const int* __restrict__ query_labels;    // contact form: three labels per query and per scene triangle, both given or both null
    const int* __restrict__ tri_labels;
    int n, k, any;
    float ox, oy, oz, sx, sy, sz;            // lattice: origin, voxel size
    int nx, ny;                              // lattice: voxels along x and y (x fastest)
};

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) overlap_boxes_kernel(const OverlapGrid g, const OverlapArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    ho::Counts cnt;
    cnt.cells = 0; cnt.sats = 0; cnt.pruned = 0;
    if (live) {
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
        } else if (a.boxes) {
            const float4 b0 = nt_load4(a.boxes + 2 * size_t(id)), b1 = nt_load4(a.boxes + 2 * size_t(id) + 1);
            lo = vec3(b0.x, b0.y, b0.z); hi = vec3(b1.x, b1.y, b1.z);
            first = __float_as_int(b0.w);
        } else {
            const int x = id % a.nx, yz = id / a.nx, y = yz % a.ny, z = yz / a.ny;
            lo = vec3(ho::lattice_face(a.ox, x, a.sx), ho::lattice_face(a.oy, y, a.sy), ho::lattice_face(a.oz, z, a.sz));
            hi = vec3(ho::lattice_face(a.ox, x + 1, a.sx), ho::lattice_face(a.oy, y + 1, a.sy), ho::lattice_face(a.oz, z + 1, a.sz));
        }
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        ho::IdList<ho::kMaxIds> list;
        list.init(a.k, first);
        if (active) ho::overlap_query(g, st, lo, hi, a.any != 0, list, cnt, filter);
        int* out = a.ids + size_t(id) * size_t(a.k);
        if (a.k == 8) {         // the base is 16-byte aligned (checked on the host): two streaming stores
            nt_store4(reinterpret_cast<float4*>(out), __int_as_float(list.id[0]), __int_as_float(list.id[1]), __int_as_float(list.id[2]), __int_as_float(list.id[3]));
            nt_store4(reinterpret_cast<float4*>(out) + 1, __int_as_float(list.id[4]), __int_as_float(list.id[5]), __int_as_float(list.id[6]), __int_as_float(list.id[7]));
        } else if (a.k == 4) {
            nt_store4(reinterpret_cast<float4*>(out), __int_as_float(list.id[0]), __int_as_float(list.id[1]), __int_as_float(list.id[2]), __int_as_float(list.id[3]));
        } else {
#pragma unroll
            for (int j = 0; j < ho::kMaxIds; j++)
                if (j < a.k) __builtin_nontemporal_store(list.id[j], out + j);
        }
        if (a.counts) __builtin_nontemporal_store(list.count(), a.counts + id);
    }
    if (a.counters) add_batch_counters(a.counters, lane, live ? 1 : 0, cnt.cells, cnt.sats, cnt.pruned);
}

// what both entry points check and do; boxes null: the lattice form (a holds its constants and n)
int launch(hagrid_ctx* ctx, const char* who, const hagrid_grid* grid, const void* tris, OverlapArgs a, void* ids, void* counts, void* counters, uint32_t flags) {
    if (flags & ~HAGRID_OVERLAP_ANY) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": unknown flag (HAGRID_OVERLAP_ANY is the only one)").c_str());
    if (a.k < 1 || a.k > HAGRID_MAX_OVERLAP_IDS) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": k must be 1 .. HAGRID_MAX_OVERLAP_IDS").c_str());
    if ((flags & HAGRID_OVERLAP_ANY) && a.k != 1) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": HAGRID_OVERLAP_ANY needs k = 1").c_str());
    HG_TRY(check_walk_grid(ctx, who, grid));
    if (!aligned(counters, 8)) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": the counters must be 8-byte aligned").c_str());
    if (!aligned(counts, 4)) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": the counts must be 4-byte aligned").c_str());
    if (a.n == 0) return HAGRID_OK;
    if (!tris || !ids) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": null triangle or id buffer").c_str());
    if (!aligned(tris, 16) || !aligned(a.boxes, 16) || !aligned(a.queries, 16)) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": triangles, boxes and queries must be 16-byte aligned").c_str());
    // k = 4 and k = 8 store their ids 16 bytes at a time, every other k one id at a time
    if (!aligned(ids, (a.k == 4 || a.k == 8) ? 16 : 4)) HG_FAIL(ctx, HAGRID_EINVAL, (std::string(who) + ": the ids must be 16-byte aligned for k = 4 and k = 8, 4-byte aligned otherwise").c_str());
    HG_HIP(ctx, hipSetDevice(ctx->device));
    OverlapGrid g;
    g.set(grid, tris);
    g.clip.set(g.c.lo, g.c.hi);
    a.ids = static_cast<int*>(ids);
    a.counts = static_cast<int*>(counts);
    a.counters = static_cast<unsigned long long*>(counters);
    a.any = (flags & HAGRID_OVERLAP_ANY) ? 1 : 0;
    overlap_boxes_kernel<<<grid_blocks(a.n, 64), 64, 0, ctx->stream>>>(g, a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

// ---- oriented boxes (hagrid_overlap_obbs; include/hagrid/obb.h) --------------------------------------------------------------------
// A kernel of its own, not a mode of the one above (that one is at its register limit), with its shape: one query per lane, one wavefront per workgroup,
// the stack in LDS, streaming loads of the records and streaming stores of the ids.  Across the walk a lane keeps its bounding box and the margin, nothing else
// of the box: the record is read again for every candidate that has met the bounding box, as the contact form reads its query, and again for every block the
// prune is asked about, which makes its three face normals anew (held across the walk they are 15 floats, and the kernel spilled: DESIGN.md 4.16).

struct ObbArgs {
    const float4* __restrict__ obbs;
    const int* __restrict__ query_labels;    // one label per query and three per scene triangle, both given or both null
    const int* __restrict__ tri_labels;
    int* __restrict__ ids;
    int* __restrict__ counts;                // may be null
    unsigned long long* __restrict__ counters;   // may be null
    int n, k, any;
};

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) obb_tris_kernel(const OverlapGrid g, const ObbArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    ho::Counts cnt;
    cnt.cells = 0; cnt.sats = 0; cnt.pruned = 0;
    if (live) {
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
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        ho::IdList<ho::kMaxIds> list;
        list.init(a.k, first);
        if (active) ho::overlap_query(g, st, lo, hi, a.any != 0, list, cnt, filter, prune);
        int* out = a.ids + size_t(id) * size_t(a.k);
        if (a.k == 8) {         // the base is 16-byte aligned (checked on the host): two streaming stores
            nt_store4(reinterpret_cast<float4*>(out), __int_as_float(list.id[0]), __int_as_float(list.id[1]), __int_as_float(list.id[2]), __int_as_float(list.id[3]));
            nt_store4(reinterpret_cast<float4*>(out) + 1, __int_as_float(list.id[4]), __int_as_float(list.id[5]), __int_as_float(list.id[6]), __int_as_float(list.id[7]));
        } else if (a.k == 4) {
            nt_store4(reinterpret_cast<float4*>(out), __int_as_float(list.id[0]), __int_as_float(list.id[1]), __int_as_float(list.id[2]), __int_as_float(list.id[3]));
        } else {
#pragma unroll
            for (int j = 0; j < ho::kMaxIds; j++)
                if (j < a.k) __builtin_nontemporal_store(list.id[j], out + j);
        }
        if (a.counts) __builtin_nontemporal_store(list.count(), a.counts + id);
    }
    if (a.counters) add_batch_counters(a.counters, lane, live ? 1 : 0, cnt.cells, cnt.sats, cnt.pruned);
}

} // namespace

extern "C" int hagrid_overlap_obbs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* obbs, int num_obbs, const void* query_labels,
                                   const void* tri_labels, int k, void* ids, void* counts, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (num_obbs < 0) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: negative num_obbs");
    if (num_obbs > 0 && !obbs) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: null box buffer");
    if ((query_labels != nullptr) != (tri_labels != nullptr)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: query_labels and tri_labels are given together or not at all");
    if (!aligned(query_labels, 4) || !aligned(tri_labels, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: the labels must be 4-byte aligned");
    if (flags & ~HAGRID_OVERLAP_ANY) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: unknown flag (HAGRID_OVERLAP_ANY is the only one)");
    if (k < 1 || k > HAGRID_MAX_OVERLAP_IDS) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: k must be 1 .. HAGRID_MAX_OVERLAP_IDS");
    if ((flags & HAGRID_OVERLAP_ANY) && k != 1) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: HAGRID_OVERLAP_ANY needs k = 1");
    HG_TRY(check_walk_grid(ctx, "overlap_obbs", grid));
    if (!aligned(counters, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: the counters must be 8-byte aligned");
    if (!aligned(counts, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: the counts must be 4-byte aligned");
    if (num_obbs == 0) return HAGRID_OK;
    if (!tris || !ids) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: null triangle or id buffer");
    if (!aligned(tris, 16) || !aligned(obbs, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: triangles and boxes must be 16-byte aligned");
    if (!aligned(ids, (k == 4 || k == 8) ? 16 : 4)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_obbs: the ids must be 16-byte aligned for k = 4 and k = 8, 4-byte aligned otherwise");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    OverlapGrid g;
    g.set(grid, tris);
    g.clip.set(g.c.lo, g.c.hi);
    ObbArgs a = {};
    a.obbs = static_cast<const float4*>(obbs);
    a.query_labels = static_cast<const int*>(query_labels);
    a.tri_labels = static_cast<const int*>(tri_labels);
    a.ids = static_cast<int*>(ids);
    a.counts = static_cast<int*>(counts);
    a.counters = static_cast<unsigned long long*>(counters);
    a.n = num_obbs; a.k = k;
    a.any = (flags & HAGRID_OVERLAP_ANY) ? 1 : 0;
    obb_tris_kernel<<<grid_blocks(num_obbs, 64), 64, 0, ctx->stream>>>(g, a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_overlap_boxes(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* boxes, int num_boxes, int k, void* ids, void* counts,
                                    void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (num_boxes < 0) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_boxes: negative num_boxes");
    if (num_boxes > 0 && !boxes) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_boxes: null box buffer");
    OverlapArgs a = {};
    a.boxes = static_cast<const float4*>(boxes);
    a.n = num_boxes; a.k = k;
    a.nx = 1; a.ny = 1;
    return launch(ctx, "overlap_boxes", grid, tris, a, ids, counts, counters, flags);
}

extern "C" int hagrid_overlap_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n, int k,
                                      void* ids, void* counts, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    int total = 0;
    HG_TRY(check_lattice(ctx, "overlap_lattice", origin, size, n, &total));
    OverlapArgs a = {};
    a.boxes = nullptr;
    a.n = total; a.k = k;
    a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
    a.sx = size[0]; a.sy = size[1]; a.sz = size[2];
    a.nx = n[0]; a.ny = n[1];
    return launch(ctx, "overlap_lattice", grid, tris, a, ids, counts, counters, flags);
}

extern "C" int hagrid_overlap_tris(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* queries, int num_queries, const void* first,
                                   const void* query_labels, const void* tri_labels, int k, void* ids, void* counts, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (num_queries < 0) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_tris: negative num_queries");
    if (num_queries > 0 && !queries) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_tris: null query buffer");
    if ((query_labels != nullptr) != (tri_labels != nullptr)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_tris: query_labels and tri_labels are given together or not at all");
    if (!aligned(first, 4) || !aligned(query_labels, 4) || !aligned(tri_labels, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "overlap_tris: first and the labels must be 4-byte aligned");
    OverlapArgs a = {};
    a.queries = static_cast<const float4*>(queries);
    a.first = static_cast<const int*>(first);
    a.query_labels = static_cast<const int*>(query_labels);
    a.tri_labels = static_cast<const int*>(tri_labels);
    a.n = num_queries; a.k = k;
    a.nx = 1; a.ny = 1;
    return launch(ctx, "overlap_tris", grid, tris, a, ids, counts, counters, flags);
}
