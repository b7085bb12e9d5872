// distance.hip -- the distance lattice by scatter: for every voxel centre of a lattice the nearest triangle within a band, made by the TRIANGLES -- each visits
// the voxels whose centres can lie within the band of it and takes the minimum into the voxel's 8-byte slot (include/hagrid_amd.h: hagrid_distance_lattice; the
// key, the voxel box with its margin, tasks, splat and finish: include/hagrid/distance.h).  The answers are those of hagrid_closest_points over the centres with
// r = band, bit for bit.  No counterpart in the reference.
//
// ONE kernel with a launch-uniform mode (the product library's kernel budget, tests/test_abi.py), one wavefront per workgroup in every mode:
//   size    one lane per triangle: the tasks of its voxel box into sizes[i]; the library's plain scan (build.hip: scan_plain) turns them into offsets in place;
//   splat   one wavefront per task, tasks in a grid-stride loop whose bound is read from DEVICE memory (the scan's total: the host never reads a size back).  The
//           triangle of a task is found by a binary search over the offsets (uniform over the wavefront), its box is made again (a dozen operations), and the
//           lanes take consecutive voxel numbers of the box, x fastest: one atomic instruction touches runs of consecutive 8-byte slots.  A plain load of the
//           slot first; the 64-bit atomic minimum only when the key is smaller than what was read.  When the scan's sum left 31 bits the loop runs over
//           triangles instead, each with all its runs;
//   finish  one lane per voxel: the slot unpacked into ids / d2, the winner's record made again by point_tri / tri_side.
// Vector atomics and vector stores only.  The grid's cells are not walked: the grid supplies the triangle count (the largest id it refers to), the scene box
// for the margin and the promise that the scene is admissible.
#include "trav_common.h"
#include "wave_prims.h"

#include "hagrid/distance.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hc = hagrid::closest;
namespace hd = hagrid::distance;

namespace {

enum { kSize = 0, kSplat = 1, kFinish = 2 };

struct DistArgs {
    hd::Consts c;
    const float4* __restrict__ tris;
    int num_tris, voxels, mode;
    int* sizes;                                 // size: tasks per triangle; splat: their exclusive sums
    const int* total;                           // splat: the number of tasks
    const int* too_large;                       // splat: != 0: the sum left 31 bits, take triangles
    unsigned long long* slots;                  // one key per voxel
    int* ids; float* d2; float4* records;       // finish; each may be null
    unsigned long long* counters;               // may be null
};

struct Slots {
    unsigned long long* p;
    __device__ __forceinline__ unsigned long long load(int e) const { return p[e]; }
    __device__ __forceinline__ void take_min(int e, unsigned long long key) const { atomicMin(p + e, key); }
};

__global__ void __launch_bounds__(64) distance_kernel(const DistArgs a) {
    const int lane = threadIdx.x;
    if (a.mode == kSize) {
        int boxes = 0;
        unsigned long long tasks = 0;
        for (long long base = (long long)blockIdx.x * 64; base < a.num_tris; base += (long long)gridDim.x * 64) {
            const long long i = base + lane;
            if (i < a.num_tris) {
                const int v = hd::tri_box(load_tri(a.tris, int(i)), a.c).voxels();
                const int t = hd::num_tasks(v, hd::kTaskVoxels);
                a.sizes[i] = t;
                boxes += v > 0 ? 1 : 0; tasks += (unsigned)t;
            }
        }
        if (a.counters) {
            const unsigned long long sb = wave_sum_u64((unsigned)boxes), st = wave_sum_u64(tasks);
            if (lane == 0) { atomicAdd(a.counters + 0, sb); atomicAdd(a.counters + 1, st); }
        }
    } else if (a.mode == kSplat) {
        const bool by_tri = __builtin_amdgcn_readfirstlane(*a.too_large) != 0;
        const int total = by_tri ? a.num_tris : __builtin_amdgcn_readfirstlane(*a.total);
        const Slots slots{a.slots};
        unsigned long long pairs = 0;
        for (long long t = blockIdx.x; t < total; t += gridDim.x) {
            int j = int(t), run = 0, run_end = 0x7fffffff;
            if (!by_tri) {
                const int* off = a.sizes;
                j = hd::find_task([off](int i) { return off[i]; }, a.num_tris, int(t));
                run = int(t) - off[j]; run_end = run + 1;
            }
            const Tri tri = load_tri(a.tris, j);
            const hd::Box box = hd::tri_box(tri, a.c);
            const unsigned v = unsigned(box.voxels());
            for (; run < run_end && unsigned(run) * unsigned(hd::kTaskVoxels) < v; run++) {
#pragma unroll 1
                for (int i = 0; i < hd::kTaskVoxels / 64; i++) {
                    const unsigned first = unsigned(run) * unsigned(hd::kTaskVoxels) + unsigned(i) * 64u;
                    if (first >= v) break;
                    const unsigned k = first + unsigned(lane);
                    if (k < v) {
                        vec3 p;
                        const int e = hd::box_voxel(box, a.c, int(k), p);
                        pairs += hd::splat_voxel(tri, j, p, a.c.r2, e, slots) ? 1u : 0u;
                    }
                }
            }
        }
        if (a.counters) {
            const unsigned long long sp = wave_sum_u64(pairs);
            if (lane == 0) atomicAdd(a.counters + 2, sp);
        }
    } else {
        const long long e = (long long)blockIdx.x * 64 + lane;
        int found = 0;
        if (e < a.voxels) {
            const unsigned long long key = a.slots[e];
            const vec3 p = hd::element_centre(a.c, int(e));
            found = key != hd::kEmpty ? 1 : 0;
            if (a.ids) __builtin_nontemporal_store(found ? hd::key_id(key) : -1, a.ids + e);
            if (a.d2) __builtin_nontemporal_store(found ? hd::key_d2(key) : a.c.r2, a.d2 + e);
            if (a.records) {
                const float4* tris = a.tris;
                hc::Best b;
                hd::finish_voxel([tris](int id) { return load_tri(tris, id); }, key, p, a.c.r2, b);
                nt_store4(a.records + 2 * size_t(e), b.q.x, b.q.y, b.q.z, b.d2);
                nt_store4(a.records + 2 * size_t(e) + 1, __int_as_float(b.id), __int_as_float(b.feature), float(b.side), 0.0f);
            }
        }
        if (a.counters) {
            const unsigned long long sf = wave_sum_u64((unsigned)found);
            if (lane == 0) atomicAdd(a.counters + 3, sf);
        }
    }
}

} // namespace

extern "C" int hagrid_distance_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n, float band,
                                       void* workspace, void* ids, void* d2, void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    int voxels = 0;
    HG_TRY(check_lattice(ctx, "distance_lattice", origin, size, n, &voxels));
    if (flags) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: unknown flag (flags must be 0)");
    if (!grid) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: null grid");
    if (!grid->entries || (!grid->cells && !grid->small_cells)) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: grid released for traversal, or incomplete");
    if (!grid->ref_ids) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: incomplete grid");
    if (grid->dims[0] <= 0 || grid->dims[1] <= 0 || grid->dims[2] <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: bad dims");
    if (!(band >= 0.0f) || !(band <= 3.4028234663852886e38f)) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: the band must be finite and not negative");
    if (!workspace || !aligned(workspace, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: the workspace (8 bytes per voxel) must be given and 8-byte aligned");
    if (!ids && !d2 && !records) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: at least one of ids, d2 and records must be given");
    if (!aligned(ids, 4) || !aligned(d2, 4) || !aligned(counters, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: ids and d2 must be 4-byte aligned, the counters 8-byte aligned");
    if (!tris) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: null triangle buffer");
    if (!aligned(tris, 16) || !aligned(records, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "distance_lattice: triangles and records must be 16-byte aligned");
    HG_HIP(ctx, hipSetDevice(ctx->device));

    // the triangle count: known to the host when the context holds the traversal image of this grid (hagrid_setup_traversal), else one word is read back first
    int max_ref = -1;
    HG_TRY(grid_max_ref(ctx, grid, &max_ref));
    DistArgs a = {};
    a.c = hd::make_consts(grid->bbox_min, grid->bbox_max, origin, size, n, band);
    a.tris = static_cast<const float4*>(tris);
    a.num_tris = max_ref + 1; a.voxels = voxels;
    a.slots = static_cast<unsigned long long*>(workspace);
    a.ids = static_cast<int*>(ids); a.d2 = static_cast<float*>(d2); a.records = static_cast<float4*>(records);
    a.counters = static_cast<unsigned long long*>(counters);
    hipStream_t st = ctx->stream;
    HG_HIP(ctx, hipMemsetAsync(workspace, 0xff, size_t(voxels) * 8, st));
    PoolTemps tmp(ctx);
    if (a.num_tris > 0) {
        int* tasks = ctx->dscratch + kScrDistTasks; int* too_large = ctx->dscratch + kScrDistTooLarge;      // the number of tasks; their sum left 31 bits
        a.sizes = tmp.get<int>(size_t(a.num_tris));
        if (!a.sizes) return HAGRID_ENOMEM;
        a.total = tasks; a.too_large = too_large;
        HG_HIP(ctx, hipMemsetAsync(tasks, 0, 2 * sizeof(int), st));
        const int waves = std::max(ctx->num_cus, 1) * 32;
        a.mode = kSize;
        distance_kernel<<<std::min(grid_blocks(a.num_tris, 64), waves), 64, 0, st>>>(a); HG_DBG(ctx);
        HG_TRY(scan_plain(ctx, a.sizes, a.sizes, a.num_tris, tasks, too_large));
        if (ctx->opt_distance_by_triangle) HG_HIP(ctx, hipMemsetAsync(too_large, 0x01, sizeof(int), st));      // (tests: the word a sum beyond 31 bits leaves)
        a.mode = kSplat;
        distance_kernel<<<waves, 64, 0, st>>>(a); HG_DBG(ctx);
    }
    a.mode = kFinish;
    distance_kernel<<<grid_blocks(voxels, 64), 64, 0, st>>>(a); HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}
