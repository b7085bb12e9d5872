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
//
// hagrid_traverse_grid_filtered is a MODE of the same kernel, not a second one (the kernel budget again): a filter record per ray and a mask per
// triangle (include/hagrid/ray_filter.h) arrive as two launch-uniform pointers, either of which may be null, and any-hit as a bit of a.mode.
// The skipped triangle is refused in front of the triangle test, the masks meet only for an accepted intersection (one 4-byte gather, for those
// alone), a ray whose mask is zero does not walk, and with any-hit (k = 1) the ray is done behind the first cell that left an entry in its list.
// All of it is ONE condition in front of the insert and one term of the visitor's answer, in a copy of the walk that only a launch with a filter, masks or
// any-hit enters: woven into the one walk it cost the unfiltered launch 4 to 12 % depending on its form.
// hagrid_traverse_grid_multi launches with nulls and takes the plain copy: the lists are what they were.
#include "trav_common.h"

#include "hagrid/multi_hit.h"
#include "hagrid/ray_filter.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;

namespace {

constexpr int KMAX = HAGRID_MAX_HITS;

// The walk of one ray into its list.  FILTERED is a COPY of the walk, not a second kernel: hagrid_traverse_grid_multi takes the plain copy, whose
// instructions are those it had before the filter existed.
template <bool FILTERED>
__device__ __forceinline__ void walk_into_list(const RayGrid& g, const walk::RaySetup& s, HitList<KMAX>& list, const RayFilter f,
                                               const uint32_t* __restrict__ tri_masks, const bool any_hit) {
    auto visit = [&](walk::RefList<RayGrid> refs, float texit, bool) {
        while (!refs.done()) {
            const int ref = refs.next();
            Hit h;
            if (FILTERED) {
                if (!f.skips(ref) && intersect_prim_ray_uvs(g.tri(ref), s.ray, ref, h) && f.admits(tri_masks, ref)) list.insert(h.t, ref, h.u, h.v);
            } else {
                if (intersect_prim_ray_uvs(g.tri(ref), s.ray, ref, h)) list.insert(h.t, ref, h.u, h.v);
            }
        }
        return list.full() && ((FILTERED && any_hit) || list.last_t <= texit);
    };
    walk::walk_cells(g, s, visit);
}

// Four wavefronts per SIMD, stated: with both copies of the walk the allocator takes 133 VGPRs when left alone, which is three wavefronts; held to 128 it
// spills no vector register and uses no scratch (python tools/kernel_resources.py trav_multi).
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) traverse_multi_kernel(const TraverseArgs a, const int k, const int small_cells,
                                                                  const RayFilter* __restrict__ filters, const uint32_t* __restrict__ tri_masks) {
    const bool UVS = (a.mode & HAGRID_TRAVERSE_UVS) != 0, any_hit = (a.mode & HAGRID_TRAVERSE_ANY_HIT) != 0;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
    if (id >= a.num_rays) return;

    const float4 r0 = nt_load4(a.rays + 2 * size_t(id)), r1 = nt_load4(a.rays + 2 * size_t(id) + 1);
    const RayGrid g(a, small_cells);
    const walk::RaySetup s(g.c, vec3(r0.x, r0.y, r0.z), vec3(r1.x, r1.y, r1.z), r0.w, r1.w);

    HitList<KMAX> list;
    list.init(k, s.ray.tmax);
    if (filters || tri_masks || any_hit) {                  // launch-uniform
        const RayFilter f = RayFilter::of(filters, size_t(id));
        if (s.enters && f.walks()) walk_into_list<true>(g, s, list, f, tri_masks, any_hit);
    } else if (s.enters) {
        walk_into_list<false>(g, s, list, RayFilter(), nullptr, false);
    }

    float4* out = a.hits + size_t(id) * size_t(k);
    HAGRID_UNROLL
    for (int j = 0; j < KMAX; j++)
        if (j < k) nt_store4(out + j, __int_as_float(list.id[j]), list.t[j], UVS ? list.u[j] : 0.0f, UVS ? list.v[j] : 0.0f);
}

} // namespace

// both entry points: `who` names the caller in the messages; filters, tri_masks and HAGRID_TRAVERSE_ANY_HIT only come from the filtered one
static int launch_multi(hagrid_ctx* ctx, const char* who, const hagrid_grid* grid, const void* tris, const void* rays, const void* filters,
                        const void* tri_masks, void* hits, int num_rays, int k, uint32_t flags) {
    const std::string w(who);
    if (grid && !grid->entries) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": the multi-hit walk reads the construction format (grid released for traversal)").c_str());
    if (ctx->opt_id_is_steps) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": the lists hold primitive ids (\"traverse.id_is_steps\" is 1)").c_str());
    TraverseArgs a;
    HG_TRY(make_args(ctx, grid, tris, rays, hits, num_rays, a));
    if (int64_t(num_rays) * int64_t(k) > int64_t(INT32_MAX)) HG_FAIL(ctx, HAGRID_ERANGE, (w + ": num_rays * k does not fit 31 bits").c_str());
    if (num_rays == 0) return HAGRID_OK;
    if (!aligned(tris, 16) || !aligned(rays, 16) || !aligned(hits, 16)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": triangles, rays and hits must be 16-byte aligned").c_str());
    HG_HIP(ctx, hipSetDevice(ctx->device));
    a.mode = flags;
    const int blocks = grid_blocks(num_rays, 64);
    traverse_multi_kernel<<<blocks, 64, 0, ctx->stream>>>(a, k, grid->small_cells != nullptr ? 1 : 0, static_cast<const RayFilter*>(filters),
                                                          static_cast<const uint32_t*>(tri_masks));
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_traverse_grid_multi(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, void* hits,
                                          int num_rays, int k, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (k < 1 || k > HAGRID_MAX_HITS) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: k must be 1 .. HAGRID_MAX_HITS");
    if (flags & ~uint32_t(HAGRID_TRAVERSE_UVS)) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: the only flag is HAGRID_TRAVERSE_UVS (any-hit contradicts k hits)");
    return launch_multi(ctx, "traverse_grid_multi", grid, tris, rays, nullptr, nullptr, hits, num_rays, k, flags);
}

extern "C" int hagrid_traverse_grid_filtered(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, const void* filters,
                                             const void* tri_masks, void* hits, int num_rays, int k, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (k < 1 || k > HAGRID_MAX_HITS) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_filtered: k must be 1 .. HAGRID_MAX_HITS");
    if (flags & ~uint32_t(HAGRID_TRAVERSE_UVS | HAGRID_TRAVERSE_ANY_HIT)) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_filtered: unknown flag (HAGRID_TRAVERSE_UVS and HAGRID_TRAVERSE_ANY_HIT are the two)");
    if ((flags & HAGRID_TRAVERSE_ANY_HIT) && k != 1) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_filtered: the flag HAGRID_TRAVERSE_ANY_HIT needs k = 1");
    if (!aligned(filters, 8) || !aligned(tri_masks, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_filtered: filters must be 8-byte aligned, tri_masks 4-byte aligned");
    return launch_multi(ctx, "traverse_grid_filtered", grid, tris, rays, filters, tri_masks, hits, num_rays, k, flags);
}
