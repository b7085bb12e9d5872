// trav_multi.hip -- multi-hit traversal: the k nearest intersections of every ray, sorted by (t, id) (include/hagrid_amd.h:
// hagrid_traverse_grid_multi; the list and its rules: include/hagrid/multi_hit.h).  No counterpart in the reference.
//
// The walk is hagrid/cell_walk.h's over the device accessor of trav_common.h, launched like traverse_kernel_v2 (trav_plain.hip): one wavefront per
// workgroup, the XCD-aware block -> ray-range map, streaming loads / stores for rays and hits.  What is particular is the visitor:
//   * every triangle is tested against the ray's OWN [tmin, tmax) -- the window is never shrunk to the nearest hit so far;
//   * accepted intersections go into a sorted list of capacity k held in registers (HitList<KMAX>, every index a compile-time one);
//   * the ray is done when the list is full and its last entry is not beyond the exit of the current cell, or the ray left the grid.
// k and the cell format are kernel arguments (the same for every ray): ONE kernel with HAGRID_MAX_HITS slots serves every k and both
// Cell and SmallCell grids -- the product library's kernel budget (tests/test_abi.py) has room for this one and the shading kernel
// of frame.hip, not for a family of k buckets; what that costs small k is in DESIGN.md.  Rays are processed in buffer order: no ray
// binning, no tile packets, no learned tile order, no traversal image (all out of scope for this entry point); each ray's list depends on that ray alone, so it would be the same under any lane <-> ray assignment.
#include "trav_common.h"

#include "hagrid/multi_hit.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;

namespace {

constexpr int KMAX = HAGRID_MAX_HITS;

__global__ void __launch_bounds__(64) traverse_multi_kernel(const TraverseArgs a, const int k, const int small_cells) {
    const bool UVS = (a.mode & HAGRID_TRAVERSE_UVS) != 0;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
    if (id >= a.num_rays) return;

    const float4 r0 = nt_load4(a.rays + 2 * size_t(id)), r1 = nt_load4(a.rays + 2 * size_t(id) + 1);
    const RayGrid g(a, small_cells);
    const walk::RaySetup s(g.c, vec3(r0.x, r0.y, r0.z), vec3(r1.x, r1.y, r1.z), r0.w, r1.w);

    HitList<KMAX> list;
    list.init(k, s.ray.tmax);
    auto visit = [&](walk::RefList<RayGrid> refs, float texit, bool) {
        while (!refs.done()) {
            const int ref = refs.next();
            Hit h;
            if (intersect_prim_ray_uvs(g.tri(ref), s.ray, ref, h)) list.insert(h.t, ref, h.u, h.v);
        }
        return list.full() && list.last_t <= texit;
    };
    if (s.enters) walk::walk_cells(g, s, visit);

    float4* out = a.hits + size_t(id) * size_t(k);
    HAGRID_UNROLL
    for (int j = 0; j < KMAX; j++)
        if (j < k) nt_store4(out + j, __int_as_float(list.id[j]), list.t[j], UVS ? list.u[j] : 0.0f, UVS ? list.v[j] : 0.0f);
}

} // namespace

extern "C" int hagrid_traverse_grid_multi(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, void* hits,
                                          int num_rays, int k, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (k < 1 || k > HAGRID_MAX_HITS) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: k must be 1 .. HAGRID_MAX_HITS");
    if (flags & ~uint32_t(HAGRID_TRAVERSE_UVS)) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: the only flag is HAGRID_TRAVERSE_UVS (any-hit contradicts k hits)");
    if (grid && !grid->entries) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: the multi-hit walk reads the construction format (grid released for traversal)");
    if (ctx->opt_id_is_steps) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: the lists hold primitive ids (\"traverse.id_is_steps\" is 1)");
    TraverseArgs a;
    HG_TRY(make_args(ctx, grid, tris, rays, hits, num_rays, a));
    if (int64_t(num_rays) * int64_t(k) > int64_t(INT32_MAX)) HG_FAIL(ctx, HAGRID_ERANGE, "traverse_grid_multi: num_rays * k does not fit 31 bits");
    if (num_rays == 0) return HAGRID_OK;
    if (!aligned(tris, 16) || !aligned(rays, 16) || !aligned(hits, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: triangles, rays and hits must be 16-byte aligned");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    a.mode = flags;
    const int blocks = grid_blocks(num_rays, 64);
    traverse_multi_kernel<<<blocks, 64, 0, ctx->stream>>>(a, k, grid->small_cells != nullptr ? 1 : 0);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}
