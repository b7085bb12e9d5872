// crossings.hip -- crossing queries: for every ray ALL the surfaces it crosses, condensed into one 16-byte record (count, first t, length inside, winding), and
// from that whether a point lies inside a closed surface (include/hagrid_amd.h: hagrid_count_crossings, hagrid_points_inside, hagrid_inside_lattice; the record,
// the page, the accumulator and the argument why nothing is lost: include/hagrid/crossings.h).  No counterpart in the reference.
//
// The kernel runs the header's crossings_walk (the walk of hagrid/cell_walk.h with the page visitor) over the device accessor of trav_common.h, launched
// like traverse_multi_kernel (trav_multi.hip): one wavefront per workgroup, the XCD-aware block -> item map, streaming 16-byte loads and stores.  Like
// multi-hit it neither uses nor touches the traversal image, ray binning, tile packets, the learned order or the nearest-hit hints.  One lane per ITEM: a
// ray in the ray form, a point in the point and lattice forms -- the lane then walks its m rays one after another.  The cell format, the source (ray
// buffer, point buffer or lattice constants), m, the directions, the vote rule and whether records are stored are kernel arguments, uniform over the
// launch: ONE kernel (the product library's kernel budget, tests/test_abi.py).  The page (kPage entries of t and key, no u, v) and the accumulator live in
// registers: every loop over the page runs over compile-time indices.  kPage was chosen by register count alone, not by timing.
//
// hagrid_list_crossings is a launch-uniform MODE of the same kernel (q.list), not a second one: the lane works out its slots once (hx::slot_range), the
// header's sink stores every folded entry with position < room as one streaming 8-byte word, and after the walk the lane fills [min(m, room), room) with the
// empty entry.  The other forms run with room 0 and a null target: the sink stores nothing and their records are the bits they were.
//
// hagrid_fill_lattice is the ROW form, a fourth source beside ray, point and lattice and again a launch-uniform mode (q.row = 1 + axis): one lane per voxel row
// of one axis, one launch per requested axis on the context's stream, x, y, z.  The lane's ray is the header's row_ray, its sink the header's RowSink over the
// emitter below: between two crossings the state is constant, so a run of voxels gets it at once.  A pass that is not the last keeps its vote in the workspace
// byte (hx::row_bits: two bits per pass), the last pass reads the byte and writes `inside`; a lane whose row ends inside goes over its row once more with
// valid = 0.  Inside one launch every voxel belongs to exactly one lane, so the launch order is the only synchronisation.  Rows along x are contiguous: there a
// run is stored four voxels at a time where the address allows (one 16-byte store of `inside`, one dword of the workspace); rows along y and z lie one x apart
// in neighbouring lanes and store element by element.
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
    unsigned long long* __restrict__ counters;  // may be null; int64[4], in the list mode int64[6]
    const long long* __restrict__ offsets;      // the list mode, CSR form: int64[n + 1]; null: the stride form
    unsigned long long* __restrict__ entries;   // the list mode: `capacity` entries of 8 bytes, t in the low word and key in the high one
    long long capacity;
    int list, stride;
    int n, m, winding;
    float d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z;      // the directions of the point and lattice forms
    float ox, oy, oz, sx, sy, sz;               // lattice: origin, voxel size
    int nx, ny;                                 // lattice: voxels along x and y (x fastest)
    int nz;                                     // the row form: voxels along z
    int row, row_pass, row_last;                // the row form: 1 + axis (0: another form); the pass (0, 1, 2) and whether it is the last
    int row_n, row_stride; float row_o, row_s;  // the row form: voxels along a row, their element stride, origin and voxel size of the axis (hx::row_of's, made on the host)
    unsigned char* __restrict__ ws;             // the row form: one byte per voxel; null when the only pass is the last
    long long rec_base;                         // the row form: the first record of this axis
};

// an entry of the list mode: t in the low word and the key in the high one
struct EntrySink {
    __device__ __forceinline__ static unsigned long long word(float t, uint32_t key) { return (unsigned long long)__float_as_uint(t) | ((unsigned long long)key << 32); }
};

// the emitter of hx::RowSink: `length` voxels from element `first` on, `stride` apart, get the row's vote (valid = 0: the row abstains).  hx::row_put says what a
// voxel gets.  Rows along x (stride 1) are always pass 0 -- x is the lowest axis --, so what their voxels get is read from nowhere and the same for the whole run:
// four voxels whose target is aligned go as one store, a 16-byte one of `inside` when x is the only axis, a dword of the workspace otherwise.
struct RowEmit {
    unsigned char* ws; int* inside;
    int pass, last, valid;
    __device__ __forceinline__ void operator()(int first, int stride, int length, int state) const {
        int e = first;
        int left = length;
        HAGRID_MADE_HERE(e);         // addresses are made here, from the index: made ahead they would be carried through the whole walk, two registers each
        if (stride == 1 && pass == 0) {
            const unsigned b = hx::row_bits(0u, 0, valid, state);
            if (last) {
                const int v = hx::row_answer(b);
#pragma clang loop unroll(disable) vectorize(disable)
                for (; left > 0 && (reinterpret_cast<uintptr_t>(inside + e) & 15u); left--, e++) inside[e] = v;
#pragma clang loop unroll(disable) vectorize(disable)
                for (; left >= 4; left -= 4, e += 4) *reinterpret_cast<int4*>(inside + e) = make_int4(v, v, v, v);
            } else {
#pragma clang loop unroll(disable) vectorize(disable)
                for (; left > 0 && (reinterpret_cast<uintptr_t>(ws + e) & 3u); left--, e++) ws[e] = (unsigned char)b;
#pragma clang loop unroll(disable) vectorize(disable)
                for (; left >= 4; left -= 4, e += 4) *reinterpret_cast<unsigned*>(ws + e) = b * 0x01010101u;
            }
        }
#pragma clang loop unroll(disable) vectorize(disable)
        for (; left > 0; left--, e += stride) hx::row_put(ws, inside, e, pass, last != 0, valid, state);
    }
};

// The one sink of the kernel: the list mode's entries or the row form's voxels, by the launch.  A lane is in one mode or the other, so what it carries through
// the walk shares three registers: the list mode keeps its first slot in the words the row form uses for base and cursor, and its room in the row form's sum.
struct Sink {
    hx::RowSink<RowEmit> row;
    unsigned long long* entries;
    int is_row;
    __device__ __forceinline__ void set_list(long long first, int room) { row.base = int(first); row.c = int(first >> 32); row.sum = room; }
    __device__ __forceinline__ int room() const { return row.sum; }
    __device__ __forceinline__ unsigned long long* slots() const { return entries + ((long long)(unsigned)row.base | ((long long)row.c << 32)); }
    __device__ __forceinline__ void operator()(int position, float t, uint32_t key) const {
        if (is_row) row(position, t, key);
        else if (position < row.sum) __builtin_nontemporal_store(EntrySink::word(t, key), slots() + position);
    }
};

} // namespace

template <>
struct hagrid::crossings::SinkTraits<Sink> {
    __device__ __forceinline__ static bool serial(const Sink& s) { return s.is_row != 0; }
};

namespace {

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) crossings_kernel(const TraverseArgs a, const CrossArgs q, const int small_cells) {
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < q.n;
    int n_cells = 0, n_tests = 0, n_flushes = 0, n_written = 0, n_short = 0, n_abstained = 0;
    if (live) {
        vec3 org, ray_dir(0.0f, 0.0f, 0.0f);
        float tmin = 0.0f, tmax;
        bool active = true;
        int row_base = 0;
        if (q.rays) {
            const float4 r0 = nt_load4(q.rays + 2 * size_t(id)), r1 = nt_load4(q.rays + 2 * size_t(id) + 1);
            org = vec3(r0.x, r0.y, r0.z); ray_dir = vec3(r1.x, r1.y, r1.z);
            tmin = r0.w; tmax = r1.w;
        } else if (q.row) {
            const int axis = q.row - 1;
            const hx::Row w = hx::row_of(axis, id, q.nx, q.ny, q.nz);
            row_base = w.base;
            org = vec3(hx::lattice_centre(q.ox, w.x, q.sx), hx::lattice_centre(q.oy, w.y, q.sy), hx::lattice_centre(q.oz, w.z, q.sz));
            ray_dir = vec3(axis == 0 ? 1.0f : 0.0f, axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f);
            tmin = -__builtin_inff(); tmax = __builtin_inff();
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

        long long first = 0, room = 0;
        if (q.list) hx::slot_range(q.offsets, q.stride, q.capacity, id, first, room);
        Sink sink;
        sink.entries = q.entries;
        sink.is_row = q.row;
        sink.row.emit = RowEmit{q.ws, q.inside, q.row_pass, q.row_last, 1};
        sink.row.init(hx::Row{0, 0, 0, q.row_n, row_base, q.row_stride}, q.row_o, q.row_s, q.winding != 0);
        if (!q.row) sink.set_list(first, int(room < 0x7fffffffLL ? room : 0x7fffffffLL));

        int votes = 0;
#pragma unroll 1
        for (int d = 0; d < q.m; d++) {
            const vec3 dir = (q.rays || q.row) ? ray_dir : (d == 0 ? vec3(q.d0x, q.d0y, q.d0z) : d == 1 ? vec3(q.d1x, q.d1y, q.d1z) : vec3(q.d2x, q.d2y, q.d2z));
            Hit rec(0, tmax, 0.0f, 0.0f);          // an inactive point takes no cell step
            if (active) {
                hx::Counts n;
                const RayGrid g(a, small_cells);
                rec = hx::crossings_walk<kPage>(g, Ray(org, tmin, dir, tmax), kPage, n, sink);
                n_cells += n.cells; n_tests += n.tests; n_flushes += n.flushes;
            }
            votes += hx::vote(rec, q.winding != 0);
            if (q.records) nt_store4(q.records + size_t(q.rec_base) + size_t(id) * size_t(q.m) + size_t(d), __int_as_float(rec.id), rec.t, rec.u, rec.v);
            if (q.list) {           // (m = 1) the slots the list left over get the empty entry
                n_written = rec.id < sink.room() ? rec.id : sink.room();
                n_short = rec.id > sink.room() ? 1 : 0;
                const unsigned long long none = EntrySink::word(tmax, 0xffffffffu);
                int again = id;
                HAGRID_MADE_HERE(again);         // the range once more, from the ray's number: neither it nor its address is carried through the walk
                hx::slot_range(q.offsets, q.stride, q.capacity, again, first, room);
                for (long long p = n_written; p < room; p++) __builtin_nontemporal_store(none, q.entries + first + p);
            }
            if (q.row) {            // (m = 1) the voxels behind the last crossing; a row that ends inside once more, as "abstains"
                HAGRID_MADE_HERE(sink.row.base);         // (as in RowEmit: nothing made from the base before the walk is carried through it)
                sink.row.finish();
                if (sink.row.state()) {
                    n_abstained = 1;
                    RowEmit abstains = sink.row.emit;
                    abstains.valid = 0;
                    abstains(sink.row.base, sink.row.stride, sink.row.n, 0);
                }
            }
        }
        if (q.inside && !q.row) __builtin_nontemporal_store(active ? (2 * votes > q.m ? 1 : 0) : -1, q.inside + id);
    }
    if (q.counters) {
        add_batch_counters(q.counters, lane, live ? 1 : 0, n_cells, n_tests, n_flushes);
        if (q.list) {               // entries written (without empty ones), rays whose list did not fit
            const unsigned long long sw = wave_sum_u64((unsigned)n_written), ss = wave_sum_u64((unsigned)n_short);
            if (lane == 0) { atomicAdd(q.counters + 4, sw); atomicAdd(q.counters + 5, ss); }
        }
        if (q.row) {                // rows that abstained
            const unsigned long long sa = wave_sum_u64((unsigned)n_abstained);
            if (lane == 0) atomicAdd(q.counters + 4, sa);
        }
    }
}

// what the four entry points check and do; q holds the source and n, in the list mode the slots as well
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
    if (!aligned(counters, 8) || !aligned(q.offsets, 8) || !aligned(q.entries, 8)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": counters, offsets and entries must be 8-byte aligned").c_str());
    if (!aligned(inside, 4)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": inside must be 4-byte aligned").c_str());
    if (!aligned(tris, 16) || !aligned(q.rays, 16) || !aligned(q.points, 16) || !aligned(records, 16)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": triangles, rays, points and records must be 16-byte aligned").c_str());
    if (q.n == 0) return HAGRID_OK;
    if (!tris) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null triangle buffer").c_str());
    if (q.list ? (!q.entries && q.capacity > 0) : ((ray_form && !q.row) ? !records : !inside)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null output buffer").c_str());
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

extern "C" int hagrid_list_crossings(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, int num_rays, const void* offsets, int stride, void* entries,
                                     int64_t capacity, void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (num_rays < 0) HG_FAIL(ctx, HAGRID_EINVAL, "list_crossings: negative num_rays");
    if (capacity < 0) HG_FAIL(ctx, HAGRID_EINVAL, "list_crossings: negative capacity");
    if (stride < 0 || (offsets != nullptr) == (stride >= 1)) HG_FAIL(ctx, HAGRID_EINVAL, "list_crossings: either offsets (CSR form, stride 0) or a stride >= 1 with offsets == NULL");
    if (num_rays > 0 && !rays) HG_FAIL(ctx, HAGRID_EINVAL, "list_crossings: null ray buffer");
    if (!offsets && int64_t(num_rays) * int64_t(stride) > capacity) HG_FAIL(ctx, HAGRID_ERANGE, "list_crossings: num_rays * stride is beyond the capacity");
    CrossArgs q = {};
    q.rays = static_cast<const float4*>(rays);
    q.n = num_rays; q.m = 1; q.nx = 1; q.ny = 1;
    q.list = 1; q.stride = stride; q.capacity = capacity;
    q.offsets = static_cast<const long long*>(offsets);
    q.entries = static_cast<unsigned long long*>(entries);
    return launch(ctx, "list_crossings", true, grid, tris, q, nullptr, 0, nullptr, records, counters, flags, 0u);
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
    int total = 0;
    HG_TRY(check_lattice(ctx, "inside_lattice", origin, size, n, &total));
    CrossArgs q = {};
    q.n = total;
    q.ox = origin[0]; q.oy = origin[1]; q.oz = origin[2];
    q.sx = size[0]; q.sy = size[1]; q.sz = size[2];
    q.nx = n[0]; q.ny = n[1];
    return launch(ctx, "inside_lattice", false, grid, tris, q, dirs, num_dirs, inside, records, counters, flags, HAGRID_INSIDE_WINDING);
}

extern "C" int hagrid_fill_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n, uint32_t axes, void* inside,
                                   void* workspace, void* records, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    int total = 0;
    HG_TRY(check_lattice(ctx, "fill_lattice", origin, size, n, &total));
    if (axes & ~7u) HG_FAIL(ctx, HAGRID_EINVAL, "fill_lattice: axes is a mask of 1 (x), 2 (y) and 4 (z)");
    if (axes == 0) axes = 7u;
    int passes = 0, last_axis = 0;
    for (int a = 0; a < 3; a++)
        if (axes & (1u << a)) { passes++; last_axis = a; }
    if (passes > 1 && !workspace) HG_FAIL(ctx, HAGRID_EINVAL, "fill_lattice: more than one axis needs the workspace (one byte per voxel)");
    CrossArgs q = {};
    q.ox = origin[0]; q.oy = origin[1]; q.oz = origin[2];
    q.sx = size[0]; q.sy = size[1]; q.sz = size[2];
    q.nx = n[0]; q.ny = n[1]; q.nz = n[2];
    q.m = 1;
    q.ws = passes > 1 ? static_cast<unsigned char*>(workspace) : nullptr;
    for (int a = 0; a < 3; a++) {
        if (!(axes & (1u << a))) continue;
        q.n = int(hx::num_rows(a, n[0], n[1], n[2]));          // rows <= voxels, which fit 31 bits
        q.row = 1 + a; q.row_last = a == last_axis ? 1 : 0;
        const hx::Row w = hx::row_of(a, 0, n[0], n[1], n[2]);
        q.row_n = w.n; q.row_stride = w.stride; q.row_o = origin[a]; q.row_s = size[a];
        HG_TRY(launch(ctx, "fill_lattice", true, grid, tris, q, nullptr, 0, inside, records, counters, flags, HAGRID_INSIDE_WINDING));
        q.rec_base += q.n;
        q.row_pass++;
    }
    return HAGRID_OK;
}
