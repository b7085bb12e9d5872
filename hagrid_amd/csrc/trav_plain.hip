// trav_plain.hip -- traversal of the construction format (entries -> cells -> ref_ids), for grids without a traversal image
// (virtual resolution above 65535 per axis, compressed grids deeper than six levels, "traverse.image" = 0) and for what walks that
// format by definition: the statistics entry point and the reference binary's Hit.id = step count (traverse.cu:80,93).
//
// Replaces the reference's traverse<CellT, Tri> kernel (traverse.cu:27-95) with intersect_ray_box (:14-21) and compute_voxel (:23-25).
// Results per ray are identical to the CPU oracle's (same IEEE operation sequence, contraction off).
#include "trav_common.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;

namespace {

// the accessor of the statistics kernel: every look-up starts at the top level and counts the voxel-map words it reads
struct CountingGrid : RayGrid {
    mutable unsigned n_words = 0;
    using RayGrid::RayGrid;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { n_words++; return entries[i]; }
    __device__ __forceinline__ CellRec cell_at(int x, int y, int z) const {
        return cell(walk::descend(*this, word(uint32_t(walk::top_index(c, x, y, z))), x, y, z) >> 2);
    }
};

// ONE kernel: the cell format is a kernel argument, uniform over the launch (as in trav_multi.hip and closest.hip; the product library's kernel budget,
// tests/test_abi.py); the counters are kept in registers whether or not the caller asked for them (a.steps / a.stats null, "traverse.variant" = 1).
// RaySetup, step and the descent of hagrid/cell_walk.h in a loop of its own: no load is issued early, one voxel-map walk per cell visited, so the
// step and word counts are the oracle's.
__global__ void __launch_bounds__(256) traverse_kernel(const TraverseArgs a, const int small) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= a.num_rays) return;

    const float4 r0 = a.rays[2 * size_t(id)], r1 = a.rays[2 * size_t(id) + 1];
    const CountingGrid g(a, small);
    const walk::RaySetup s(g.c, vec3(r0.x, r0.y, r0.z), vec3(r1.x, r1.y, r1.z), r0.w, r1.w);

    Hit hit(-1, s.ray.tmax, 0.0f, 0.0f);
    int steps = 0;
    unsigned n_cells = 0, n_refs = 0, n_sent = 0, n_long = 0;

    if (s.enters) {
        int vx = s.vx, vy = s.vy, vz = s.vz;
        for (;;) {
            const CellRec c = g.cell_at(vx, vy, vz);
            const walk::Step st = walk::step(g.c, s, c, vx, vy, vz);

            // the cell's triangles
            walk::RefList<CountingGrid> refs(g, c);
            while (!refs.done()) {
                const int ref = refs.next();
                intersect_prim_ray(g.tri(ref), Ray(s.ray.org, s.ray.tmin, s.ray.dir, hit.t), ref, hit);
            }
            int consumed = 0;
            if (small) {          // the words read, the sentinel among them
                if (c.begin >= 0) { consumed = refs.cur - c.begin; n_refs += unsigned(consumed - 1); n_sent++; if (consumed - 1 > 4) n_long += unsigned(consumed - 1); }
            } else {
                consumed = c.end - c.begin;
                n_refs += unsigned(consumed); if (consumed > 4) n_long += unsigned(consumed);
            }
            steps += 1 + consumed;
            n_cells++;

            if (hit.t <= st.texit || st.outside) break;
        }
    }

    a.hits[id] = make_float4(__int_as_float(a.id_is_steps ? steps : hit.id), hit.t, 0.0f, 0.0f);

    if (a.steps) a.steps[id] = steps;
    if (a.stats) {
        atomicAdd(a.stats + 0, 1ull);
        atomicAdd(a.stats + 1, (unsigned long long)s.enters);
        atomicAdd(a.stats + 2, (unsigned long long)n_cells);
        atomicAdd(a.stats + 3, (unsigned long long)g.n_words);
        atomicAdd(a.stats + 4, (unsigned long long)n_refs);
        atomicAdd(a.stats + 5, (unsigned long long)n_sent);
        atomicAdd(a.stats + 6, (unsigned long long)(hit.id >= 0));
        atomicAdd(a.stats + 7, (unsigned long long)n_long);
    }
}


// ---- v2: latency-oriented kernel ---------------------------------------------------------------------------------
// A 1M-ray batch is bound by the critical path of its longest rays (hundreds of cell steps, each a chain of
// dependent loads: top entry -> sub entry -> cell -> ref id -> triangle), not by throughput.  v2 shortens that chain:
//   * the NEXT cell's voxel-map walk and cell load are issued before the current cell's triangles are tested (the driver of hagrid/cell_walk.h, which v2
//     gave its shape), and the top-level entry is kept in a register while the ray stays inside the same top-level cell (TopWord, trav_common.h);
//   * loads are issued unconditionally with clamped addresses so that independent chains overlap instead of
//     being serialised by divergent branches;
//   * one wavefront per workgroup (a finished wave frees its slot at once) and an XCD-aware block -> ray-range map:
//     consecutive ray ranges run on the same XCD, so each of the 8 private L2s caches one band of the scene.
// Same arithmetic per ray as v1 (and the oracle): identical hits.
// a.mode (HAGRID_TRAVERSE_ANY_HIT | HAGRID_TRAVERSE_UVS) is read at run time: the barycentrics are computed with every accepted hit (two multiplies; id and t are
// the same operations either way) and stored where asked for -- one instantiation per cell format and addressing instead of four.
// v2's accessor.  NARROW: every gather is base + unsigned 32-bit byte offset, index products are 24-bit multiplies (trav_common.h).
template <bool SMALL, bool NARROW>
struct V2Grid {
    static constexpr bool small = SMALL;
    const TraverseArgs& a;
    const walk::WalkConsts c;
    mutable TopWord top;
    __device__ __forceinline__ explicit V2Grid(const TraverseArgs& a_) : a(a_), c(walk_consts(a_)) {}
    __device__ __forceinline__ CellRec cell_at(int x, int y, int z) const { return cell(walk::descend(*this, top.at(*this, top_index(x, y, z)), x, y, z) >> 2); }

    __device__ __forceinline__ int top_index(int x, int y, int z) const {
        if (NARROW) return int(uint32_t(x >> a.shift) + __umul24(uint32_t(a.top_x), uint32_t(y >> a.shift)) + __umul24(uint32_t(a.top_xy), uint32_t(z >> a.shift)));
        return walk::top_index(c, x, y, z);
    }
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return NARROW ? gather32<uint32_t>(a.entries, i << 2) : a.entries[i]; }
    __device__ __forceinline__ int ref(int i) const { return NARROW ? gather32<int>(a.refs, uint32_t(i) << 2) : a.refs[i]; }
    __device__ __forceinline__ CellRec cell(uint32_t i) const {
        if (!NARROW) return load_cell_box<SMALL>(a.cells, i);
        CellRec c;
        if (SMALL) {
            const uint4 w = gather32<uint4>(a.cells, i << 4);
            c.lx = int(w.x & 0xffffu); c.ly = int(w.x >> 16); c.lz = int(w.y & 0xffffu);
            c.hx = int(w.y >> 16); c.hy = int(w.z & 0xffffu); c.hz = int(w.z >> 16);
            c.begin = int(w.w); c.end = 0;
        } else {
            const int4 lo = gather32<int4>(a.cells, i << 5), hi = gather32<int4>(a.cells, (i << 5) + 16u);
            c.lx = lo.x; c.ly = lo.y; c.lz = lo.z; c.begin = lo.w;
            c.hx = hi.x; c.hy = hi.y; c.hz = hi.z; c.end = hi.w;
        }
        return c;
    }
    __device__ __forceinline__ Tri tri(int ref) const {
        if (!NARROW) return load_tri(a.tris, ref);
        if (HG_SOLO && __ballot(ref != __builtin_amdgcn_readfirstlane(ref)) == 0ull) return load_tri_scalar(a.tris, ref);
        // ref * 48 as two full-rate instructions (the compiler turns the shift-add back into a quarter-rate 32-bit multiply)
        uint32_t r3, o;
        asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(r3) : "v"(ref));
        asm("v_lshlrev_b32 %0, 4, %1" : "=v"(o) : "v"(r3));
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.tris) + o);
        const float4 p0 = p[0], p1 = p[1], p2 = p[2];
        return Tri(vec3(p0.x, p0.y, p0.z), p0.w, vec3(p1.x, p1.y, p1.z), p1.w, vec3(p2.x, p2.y, p2.z), p2.w);
    }
};

template <bool SMALL, int BLOCK, bool NARROW>
__global__ void __launch_bounds__(BLOCK, 8) traverse_kernel_v2(const TraverseArgs a) {
    const bool ANY = (a.mode & HAGRID_TRAVERSE_ANY_HIT) != 0, UVS = (a.mode & HAGRID_TRAVERSE_UVS) != 0;
    const int* perm = (a.perm && (!a.perm_flag || __builtin_amdgcn_readfirstlane(*a.perm_flag))) ? a.perm : nullptr;
    const int w = (BLOCK == 64 && !perm) ? tile_packet_row_len(a) : 0;
    const int b = (w && a.xcd_chunk_log2 >= 0) ? xcd_chunked(blockIdx.x, gridDim.x, a.xcd_chunk_log2) : xcd_split(blockIdx.x, gridDim.x);
    const int slot = w ? tile_packet_slot(a, w, b, threadIdx.x) : b * BLOCK + threadIdx.x;
    if (slot >= a.num_rays) return;
    const int id = perm ? perm[slot] : slot;

    const float4 r0 = nt_load4(a.rays + 2 * size_t(id)), r1 = nt_load4(a.rays + 2 * size_t(id) + 1);
    typedef V2Grid<SMALL, NARROW> G;
    const G g(a);
    const walk::RaySetup s(g.c, vec3(r0.x, r0.y, r0.z), vec3(r1.x, r1.y, r1.z), r0.w, r1.w);

    Hit hit(-1, s.ray.tmax, 0.0f, 0.0f);
    // the nearest hit: the window shrinks to it; done when it is not beyond the cell's exit (any-hit: at the first accepted intersection)
    auto visit = [&](walk::RefList<G> refs, float texit, bool) {
        while (!refs.done()) {
            const int ref = refs.next();
            const bool got = intersect_prim_ray_uvs(g.tri(ref), Ray(s.ray.org, s.ray.tmin, s.ray.dir, hit.t), ref, hit);
            if (ANY && got) break;
        }
        return (ANY && hit.id >= 0) || hit.t <= texit;
    };
    if (s.enters) walk::walk_cells(g, s, visit);
    nt_store4(a.hits + id, __int_as_float(hit.id), hit.t, UVS ? hit.u : 0.0f, UVS ? hit.v : 0.0f);
}


} // namespace

void hagrid_trav::launch_v2(hipStream_t st, int blocks, bool small, bool narrow, unsigned mode, const TraverseArgs& a0) {
    TraverseArgs a = a0;
    a.mode = mode & 3u;
    if (small) { if (narrow) traverse_kernel_v2<true, 64, true><<<blocks, 64, 0, st>>>(a); else traverse_kernel_v2<true, 64, false><<<blocks, 64, 0, st>>>(a); }
    else       { if (narrow) traverse_kernel_v2<false, 64, true><<<blocks, 64, 0, st>>>(a); else traverse_kernel_v2<false, 64, false><<<blocks, 64, 0, st>>>(a); }
}


void hagrid_trav::launch_plain(hipStream_t st, int num_rays, bool small, const TraverseArgs& a) {
    const int blocks = grid_blocks(num_rays, 256);
    traverse_kernel<<<blocks, 256, 0, st>>>(a, small ? 1 : 0);
}
