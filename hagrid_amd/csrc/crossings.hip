// crossings.hip -- crossing queries: for every ray ALL the surfaces it crosses, condensed into one 16-byte record (count, first t, length inside, winding), and
// from that whether a point lies inside a closed surface (include/hagrid_amd.h: hagrid_count_crossings, hagrid_points_inside, hagrid_inside_lattice; the record,
// the page, the accumulator and the argument why nothing is lost: include/hagrid/crossings.h).  No counterpart in the reference.
//
// The kernel is the header's crossings_walk in the shape of traverse_multi_kernel (trav_multi.hip): one wavefront per workgroup, the XCD-aware block -> item
// map, the next cell's voxel-map walk and cell load issued before the current cell's triangle tests, streaming 16-byte loads and stores, the construction
// format (entries -> cells | small_cells -> ref_ids) walked in buffer order.  Like multi-hit it neither uses nor touches the traversal image, ray binning, tile
// packets, the learned order or the nearest-hit hints.  One lane per ITEM: a ray in the ray form, a point in the point and lattice forms -- the lane then walks
// its m rays one after another.  The cell format, the source (ray buffer, point buffer or lattice constants), m, the directions, the vote rule and whether
// records are stored are kernel arguments, uniform over the launch: ONE kernel (the product library's kernel budget, tests/test_abi.py).  The page (kPage
// entries of t and key, no u, v) and the accumulator live in registers: every loop over the page runs over compile-time indices.  When a page is flushed the
// SAME cell's list is tested again; `again` keeps that to one copy of the list loop.  kPage was chosen by register count alone, not by timing.
#include "trav_common.h"
#include "wave_prims.h"

#include "hagrid/crossings.h"

#include <string>

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hx = hagrid::crossings;

namespace {

constexpr int kPage = 8;

struct CrossArgs {
    const float4* __restrict__ rays;            // the ray form; null otherwise
    const float4* __restrict__ points;          // the point form; both null: the lattice form
    float4* __restrict__ records;               // may be null in the point and lattice forms
    int* __restrict__ inside;                   // null in the ray form
    unsigned long long* __restrict__ counters;  // may be null
    int n, m, winding;
    float d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z;      // the directions of the point and lattice forms
    float ox, oy, oz, sx, sy, sz;               // lattice: origin, voxel size
    int nx, ny;                                 // lattice: voxels along x and y (x fastest)
};

__device__ __forceinline__ CellBox load_cell(const void* __restrict__ cells, uint32_t index, bool small) {
    CellBox c;
    if (small) { c = load_cell_box<true>(cells, index); c.end = 0x7fffffff; }
    else       { c = load_cell_box<false>(cells, index); }
    return c;
}

__global__ void __launch_bounds__(64) crossings_kernel(const TraverseArgs a, const CrossArgs q, const int small_cells) {
    const bool SMALL = small_cells != 0;
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < q.n;
    int n_cells = 0, n_tests = 0, n_flushes = 0;
    if (live) {
        vec3 org, ray_dir(0.0f, 0.0f, 0.0f);
        float tmin = 0.0f, tmax;
        bool active = true;
        if (q.rays) {
            const float4 r0 = nt_load4(q.rays + 2 * size_t(id)), r1 = nt_load4(q.rays + 2 * size_t(id) + 1);
            org = vec3(r0.x, r0.y, r0.z); ray_dir = vec3(r1.x, r1.y, r1.z);
            tmin = r0.w; tmax = r1.w;
        } else {
            if (q.points) {
                const float4 p = nt_load4(q.points + size_t(id));
                org = vec3(p.x, p.y, p.z); tmax = p.w;
            } else {
                const int x = id % q.nx, yz = id / q.nx, y = yz % q.ny, z = yz / q.ny;
                org = vec3(hx::lattice_centre(q.ox, x, q.sx), hx::lattice_centre(q.oy, y, q.sy), hx::lattice_centre(q.oz, z, q.sz));
                tmax = __builtin_inff();
            }
            active = hx::point_active(org, tmax);
        }
        const vec3 gmin(a.min_x, a.min_y, a.min_z), gmax(a.max_x, a.max_y, a.max_z);
        const vec3 csize(a.cs_x, a.cs_y, a.cs_z), ginv(a.inv_x, a.inv_y, a.inv_z);
        int votes = 0;
#pragma unroll 1
        for (int d = 0; d < q.m; d++) {
            vec3 dir = q.rays ? ray_dir : (d == 0 ? vec3(q.d0x, q.d0y, q.d0z) : d == 1 ? vec3(q.d1x, q.d1y, q.d1z) : vec3(q.d2x, q.d2y, q.d2z));
            const bool admitted = active && admit_ray(org, dir, tmin, tmax);          // an inadmissible ray and an inactive point take no cell step
            const vec3 inv_dir(safe_rcp(dir.x), safe_rcp(dir.y), safe_rcp(dir.z));
            const vec3 walk_inv(walk_rcp(dir.x), walk_rcp(dir.y), walk_rcp(dir.z));
            const bool px = dir.x >= 0.0f, py = dir.y >= 0.0f, pz = dir.z >= 0.0f;
            const vec3 ta = (gmin - org) * inv_dir, tb = (gmax - org) * inv_dir;
            const vec3 t0 = min(ta, tb), t1 = max(ta, tb);
            const float tstart = detail::fmax2(detail::fmax2(t0.x, detail::fmax2(t0.y, t0.z)), tmin);
            const float tend = detail::fmin2(detail::fmin2(t1.x, detail::fmin2(t1.y, t1.z)), tmax);
            const Ray ray(org, tmin, dir, tmax);          // the window every triangle is tested against

            hx::Accum acc;
            acc.init(tmax);
            if (admitted && !(tstart > tend)) {
                hx::Page<kPage> page;
                page.init(kPage);
                const vec3 fv = (tstart * dir + org - gmin) * ginv;
                int vx = min(max(hx::f2i(fv.x), 0), a.dims_x - 1);
                int vy = min(max(hx::f2i(fv.y), 0), a.dims_y - 1);
                int vz = min(max(hx::f2i(fv.z), 0), a.dims_z - 1);

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
                CellBox nc = c;
                float texit = 0.0f;
                bool outside = false, again = false;

                for (;;) {
                    if (!again) {
                        n_cells++;
                        const int cx = px ? c.hx : c.lx, cy = py ? c.hy : c.ly, cz = pz ? c.hz : c.lz;
                        const vec3 tcell = (vec3(float(cx), float(cy), float(cz)) * csize + gmin - org) * walk_inv;
                        texit = detail::fmin2(tcell.x, detail::fmin2(tcell.y, tcell.z));
                        const vec3 ev = (texit * dir + org - gmin) * ginv;
                        const int nx = texit == tcell.x ? cx + (px ? 0 : -1) : hx::f2i(ev.x);
                        const int ny = texit == tcell.y ? cy + (py ? 0 : -1) : hx::f2i(ev.y);
                        const int nz = texit == tcell.z ? cz + (pz ? 0 : -1) : hx::f2i(ev.z);
                        vx = px ? max(nx, vx) : min(nx, vx);
                        vy = py ? max(ny, vy) : min(ny, vy);
                        vz = pz ? max(nz, vz) : min(nz, vz);
                        outside = (vx < 0) | (vx >= a.dims_x) | (vy < 0) | (vy >= a.dims_y) | (vz < 0) | (vz >= a.dims_z);
                    }
                    // first reference of this cell and the next cell's top entry: two independent loads in flight
                    const int begin = c.begin;
                    const bool nonempty = begin >= 0 && begin < c.end;
                    int cur = nonempty ? begin : 0;
                    int ref = a.refs[cur];
                    cur++;
                    if (!nonempty) ref = -1;
                    if (!again) {
                        // (a voxel outside the grid keeps the current top-level entry; the sub-level indices are masked, so its walk stays inside that entry's blocks and is dropped)
                        const int ntop = outside ? top_idx : top_index(vx, vy, vz);
                        if (ntop != top_idx) { topw = a.entries[ntop]; top_idx = ntop; }
                        // next cell: walk + load, overlapping the triangle tests below
                        nc = load_cell(a.cells, walk(topw, vx, vy, vz) >> 2, SMALL);
                    }
                    while (ref >= 0) {
                        const int next = cur < c.end ? a.refs[cur] : -1;
                        cur++;
                        float t; bool entering;
                        n_tests++;
                        if (hx::crosses(load_tri(a.tris, ref), ray, t, entering)) page.insert(t, (uint32_t(ref) << 1) | (entering ? 1u : 0u));
                        ref = next;
                    }
                    again = page.full() && (page.last_t <= texit || outside);
                    if (again) { page.flush(acc); n_flushes++; continue; }          // and this cell's list once more
                    if (outside) break;
                    c = nc;
                }
                if (!page.empty()) { page.flush(acc); n_flushes++; }
            }
            const Hit rec = acc.record();
            votes += hx::vote(rec, q.winding != 0);
            if (q.records) nt_store4(q.records + size_t(id) * size_t(q.m) + size_t(d), __int_as_float(rec.id), rec.t, rec.u, rec.v);
        }
        if (q.inside) __builtin_nontemporal_store(active ? (2 * votes > q.m ? 1 : 0) : -1, q.inside + id);
    }
    if (q.counters) {   // batch totals: the wavefront's sums, one vector atomic each
        const int items = wave_sum(live ? 1 : 0);
        // a lane's count fits 31 bits, 64 of them need not
        unsigned long long cells = (unsigned long long)(unsigned)n_cells, tests = (unsigned long long)(unsigned)n_tests, flushes = (unsigned long long)(unsigned)n_flushes;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            cells += (unsigned long long)__shfl_xor((long long)cells, d, 64);
            tests += (unsigned long long)__shfl_xor((long long)tests, d, 64);
            flushes += (unsigned long long)__shfl_xor((long long)flushes, d, 64);
        }
        if (lane == 0) {
            atomicAdd(q.counters + 0, (unsigned long long)items);
            atomicAdd(q.counters + 1, cells);
            atomicAdd(q.counters + 2, tests);
            atomicAdd(q.counters + 3, flushes);
        }
    }
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what the three entry points check and do; q holds the source and n
int launch(hagrid_ctx* ctx, const char* who, bool ray_form, const hagrid_grid* grid, const void* tris, CrossArgs q, const float* dirs, int num_dirs, void* inside, void* records,
           void* counters, uint32_t flags, uint32_t known_flags) {
    const std::string w(who);
    if (flags & ~known_flags) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": unknown flag").c_str());
    if (!grid) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null grid").c_str());
    if (!grid->entries || (!grid->cells && !grid->small_cells)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": the walk reads the construction format (grid released for traversal, or incomplete)").c_str());
    if (ctx->opt_id_is_steps) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": the walk tests by primitive id (\"traverse.id_is_steps\" is 1)").c_str());
    if (grid->dims[0] <= 0 || grid->dims[1] <= 0 || grid->dims[2] <= 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": bad dims").c_str());
    TraverseArgs a;
    HG_TRY(make_args(ctx, grid, nullptr, nullptr, nullptr, 0, a));
    if (!ray_form) {        // the point and lattice forms: m directions
        if (!(num_dirs == 1 || num_dirs == 3 || (num_dirs == 0 && !dirs)) || (num_dirs > 0 && !dirs)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": num_dirs must be 1 or 3 (0 with dirs == NULL: the three defaults)").c_str());
        float d[9];
        for (int i = 0; i < 9; i++) d[i] = hx::kDefaultDirs[i];
        q.m = num_dirs ? num_dirs : 3;
        for (int i = 0; i < 3 * num_dirs; i++) d[i] = dirs[i];
        for (int i = 0; i < q.m; i++) {
            vec3 dir(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
            if (!admit_ray(vec3(0.0f), dir, 0.0f, 1.0f)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": a direction must be finite and not zero").c_str());
        }
        q.d0x = d[0]; q.d0y = d[1]; q.d0z = d[2]; q.d1x = d[3]; q.d1y = d[4]; q.d1z = d[5]; q.d2x = d[6]; q.d2y = d[7]; q.d2z = d[8];
        if (int64_t(q.n) * int64_t(q.m) > int64_t(INT32_MAX)) HG_FAIL(ctx, HAGRID_ERANGE, (w + ": num_points * num_dirs does not fit 31 bits").c_str());
    }
    if (!aligned(counters, 8)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": the counters must be 8-byte aligned").c_str());
    if (!aligned(inside, 4)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": inside must be 4-byte aligned").c_str());
    if (!aligned(tris, 16) || !aligned(q.rays, 16) || !aligned(q.points, 16) || !aligned(records, 16)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": triangles, rays, points and records must be 16-byte aligned").c_str());
    if (q.n == 0) return HAGRID_OK;
    if (!tris) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null triangle buffer").c_str());
    if (ray_form ? !records : !inside) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null output buffer").c_str());
    HG_HIP(ctx, hipSetDevice(ctx->device));
    a.tris = static_cast<const float4*>(tris);
    a.num_rays = q.n;
    q.records = static_cast<float4*>(records);
    q.inside = static_cast<int*>(inside);
    q.counters = static_cast<unsigned long long*>(counters);
    q.winding = (flags & HAGRID_INSIDE_WINDING) ? 1 : 0;
    crossings_kernel<<<grid_blocks(q.n, 64), 64, 0, ctx->stream>>>(a, q, grid->small_cells != nullptr ? 1 : 0);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

} // namespace

extern "C" int hagrid_count_crossings(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, void* records, int num_rays, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (num_rays < 0) HG_FAIL(ctx, HAGRID_EINVAL, "count_crossings: negative num_rays");
    if (num_rays > 0 && !rays) HG_FAIL(ctx, HAGRID_EINVAL, "count_crossings: null ray buffer");
    CrossArgs q = {};
    q.rays = static_cast<const float4*>(rays);
    q.n = num_rays; q.m = 1; q.nx = 1; q.ny = 1;
    return launch(ctx, "count_crossings", true, grid, tris, q, nullptr, 0, nullptr, records, counters, flags, 0u);
}

extern "C" int hagrid_points_inside(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, int num_points, const float* dirs, int num_dirs, void* inside,
                                    void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (num_points < 0) HG_FAIL(ctx, HAGRID_EINVAL, "points_inside: negative num_points");
    if (num_points > 0 && !points) HG_FAIL(ctx, HAGRID_EINVAL, "points_inside: null point buffer");
    CrossArgs q = {};
    q.points = static_cast<const float4*>(points);
    q.n = num_points; q.nx = 1; q.ny = 1;
    return launch(ctx, "points_inside", false, grid, tris, q, dirs, num_dirs, inside, records, counters, flags, HAGRID_INSIDE_WINDING);
}

extern "C" int hagrid_inside_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n, const float* dirs, int num_dirs,
                                     void* inside, void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (!origin || !size || !n) HG_FAIL(ctx, HAGRID_EINVAL, "inside_lattice: null origin, size or n");
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "inside_lattice: the lattice needs at least one voxel along every axis");
    const long long plane = (long long)n[0] * n[1];                 // each factor is below 2^31: fits 62 bits
    if (plane > 0x7fffffffLL) HG_FAIL(ctx, HAGRID_EINVAL, "inside_lattice: more than 2^31 - 1 voxels");
    const long long total = plane * n[2];                           // below 2^62 now
    if (total > 0x7fffffffLL) HG_FAIL(ctx, HAGRID_EINVAL, "inside_lattice: more than 2^31 - 1 voxels");
    for (int i = 0; i < 3; i++)
        if (!(size[i] > 0.0f) || !(size[i] <= 3.4028234663852886e38f) || !(origin[i] >= -3.4028234663852886e38f && origin[i] <= 3.4028234663852886e38f))
            HG_FAIL(ctx, HAGRID_EINVAL, "inside_lattice: the voxel size must be positive and finite, the origin finite");
    CrossArgs q = {};
    q.n = int(total);
    q.ox = origin[0]; q.oy = origin[1]; q.oz = origin[2];
    q.sx = size[0]; q.sy = size[1]; q.sz = size[2];
    q.nx = n[0]; q.ny = n[1];
    return launch(ctx, "inside_lattice", false, grid, tris, q, dirs, num_dirs, inside, records, counters, flags, HAGRID_INSIDE_WINDING);
}
