// trav_multi.hip -- multi-hit traversal: the k nearest intersections of every ray, sorted by (t, id) (include/hagrid_amd.h:
// hagrid_traverse_grid_multi; the list and its rules: include/hagrid/multi_hit.h).  No counterpart in the reference.
//
// The walk is traverse_kernel_v2's over the construction format (entries -> cells | small_cells -> ref_ids, trav_plain.hip): one
// wavefront per workgroup, the XCD-aware block -> ray-range map, the next cell's voxel-map walk and cell load issued before the
// current cell's triangle tests, streaming loads / stores for rays and hits.  What differs is what a ray keeps and when it stops:
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

// a cell of either format; a SmallCell's list ends with its sentinel, so its `end` is no bound
__device__ __forceinline__ CellBox load_cell(const void* __restrict__ cells, uint32_t index, bool small) {
    CellBox c;
    if (small) { c = load_cell_box<true>(cells, index); c.end = 0x7fffffff; }
    else       { c = load_cell_box<false>(cells, index); }
    return c;
}

__global__ void __launch_bounds__(64) traverse_multi_kernel(const TraverseArgs a, const int k, const int small_cells) {
    const bool SMALL = small_cells != 0;
    const bool UVS = (a.mode & HAGRID_TRAVERSE_UVS) != 0;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
    if (id >= a.num_rays) return;

    const float4 r0 = nt_load4(a.rays + 2 * size_t(id)), r1 = nt_load4(a.rays + 2 * size_t(id) + 1);
    const vec3 org(r0.x, r0.y, r0.z);
    vec3 dir(r1.x, r1.y, r1.z);
    const float tmin = r0.w, tmax = r1.w;
    const bool admitted = admit_ray(org, dir, tmin, tmax);          // an inadmissible ray is a miss: no cell walk
    const vec3 inv_dir(safe_rcp(dir.x), safe_rcp(dir.y), safe_rcp(dir.z));
    const vec3 walk_inv(walk_rcp(dir.x), walk_rcp(dir.y), walk_rcp(dir.z));          // for the cell walk: no exit through planes of an axis the ray does not move along
    const vec3 gmin(a.min_x, a.min_y, a.min_z), gmax(a.max_x, a.max_y, a.max_z);
    const vec3 csize(a.cs_x, a.cs_y, a.cs_z), ginv(a.inv_x, a.inv_y, a.inv_z);
    const bool px = dir.x >= 0.0f, py = dir.y >= 0.0f, pz = dir.z >= 0.0f;

    const vec3 ta = (gmin - org) * inv_dir, tb = (gmax - org) * inv_dir;
    const vec3 t0 = min(ta, tb), t1 = max(ta, tb);
    const float tstart = detail::fmax2(detail::fmax2(t0.x, detail::fmax2(t0.y, t0.z)), tmin);
    const float tend = detail::fmin2(detail::fmin2(t1.x, detail::fmin2(t1.y, t1.z)), tmax);

    HitList<KMAX> list;
    list.init(k, tmax);
    const Ray ray(org, tmin, dir, tmax);          // the window every triangle is tested against

    if (admitted && !(tstart > tend)) {
        const vec3 fv = (tstart * dir + org - gmin) * ginv;
        int vx = min(max(int(fv.x), 0), a.dims_x - 1);
        int vy = min(max(int(fv.y), 0), a.dims_y - 1);
        int vz = min(max(int(fv.z), 0), a.dims_z - 1);

        auto walk = [&](uint32_t w, int x, int y, int z) -> uint32_t {   // sub-levels of the voxel map
            int depth = 0;
            while (w & 3u) {
                const int l = int(w & 3u);
                depth += l;
                const int s = a.shift - depth, m = (1 << l) - 1;
                w = a.entries[(w >> 2) + ((x >> s) & m) + ((((y >> s) & m) + (((z >> s) & m) << l)) << l)];
            }
            return w;
        };
        auto top_index = [&](int x, int y, int z) -> int { return (x >> a.shift) + a.top_x * ((y >> a.shift) + a.top_y * (z >> a.shift)); };

        int top_idx = top_index(vx, vy, vz);
        uint32_t topw = a.entries[top_idx];
        CellBox c = load_cell(a.cells, walk(topw, vx, vy, vz) >> 2, SMALL);

        for (;;) {
            const int cx = px ? c.hx : c.lx, cy = py ? c.hy : c.ly, cz = pz ? c.hz : c.lz;
            const vec3 tcell = (vec3(float(cx), float(cy), float(cz)) * csize + gmin - org) * walk_inv;
            const float texit = detail::fmin2(tcell.x, detail::fmin2(tcell.y, tcell.z));
            const vec3 ev = (texit * dir + org - gmin) * ginv;
            const int nx = texit == tcell.x ? cx + (px ? 0 : -1) : int(ev.x);
            const int ny = texit == tcell.y ? cy + (py ? 0 : -1) : int(ev.y);
            const int nz = texit == tcell.z ? cz + (pz ? 0 : -1) : int(ev.z);
            vx = px ? max(nx, vx) : min(nx, vx);
            vy = py ? max(ny, vy) : min(ny, vy);
            vz = pz ? max(nz, vz) : min(nz, vz);
            const bool outside = (vx < 0) | (vx >= a.dims_x) | (vy < 0) | (vy >= a.dims_y) | (vz < 0) | (vz >= a.dims_z);

            // first reference of this cell and the next cell's top entry: two independent loads in flight
            const int begin = c.begin;
            const bool nonempty = begin >= 0 && begin < c.end;
            int cur = nonempty ? begin : 0;
            int ref = a.refs[cur];
            cur++;
            if (!nonempty) ref = -1;
            // (a voxel outside the grid keeps the current top-level entry; the sub-level indices are masked, so its walk stays inside that entry's blocks and is dropped)
            const int ntop = outside ? top_idx : top_index(vx, vy, vz);
            if (ntop != top_idx) { topw = a.entries[ntop]; top_idx = ntop; }
            // next cell: walk + load, overlapping the triangle tests below
            const CellBox nc = load_cell(a.cells, walk(topw, vx, vy, vz) >> 2, SMALL);

            while (ref >= 0) {
                const int next = cur < c.end ? a.refs[cur] : -1;
                cur++;
                Hit h;
                if (intersect_prim_ray_uvs(load_tri(a.tris, ref), ray, ref, h)) list.insert(h.t, ref, h.u, h.v);
                ref = next;
            }
            if ((list.full() && list.last_t <= texit) || outside) break;
            c = nc;
        }
    }

    float4* out = a.hits + size_t(id) * size_t(k);
    HAGRID_UNROLL
    for (int j = 0; j < KMAX; j++)
        if (j < k) nt_store4(out + j, __int_as_float(list.id[j]), list.t[j], UVS ? list.u[j] : 0.0f, UVS ? list.v[j] : 0.0f);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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
    if (!aligned16(tris) || !aligned16(rays) || !aligned16(hits)) HG_FAIL(ctx, HAGRID_EINVAL, "traverse_grid_multi: triangles, rays and hits must be 16-byte aligned");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    a.mode = flags;
    const int blocks = grid_blocks(num_rays, 64);
    traverse_multi_kernel<<<blocks, 64, 0, ctx->stream>>>(a, k, grid->small_cells != nullptr ? 1 : 0);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}
