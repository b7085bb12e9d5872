// hagrid/distance.h -- the distance lattice by SCATTER (hagrid_amd.h: hagrid_distance_lattice): for every voxel centre of a lattice the answer of
// hagrid_closest_points for the query (centre, r = band), made the other way round: every triangle visits the voxels whose centres can lie within the
// band of it and takes the minimum into each voxel's slot.  No counterpart in the reference.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same functions serve the gfx950 kernel
// (hagrid_amd/csrc/distance.hip) and host programs (tests/cpp/distance_host.cpp); hagrid_amd/scene.py (distance_lattice) states the answer in numpy:
// closest_points over lattice_centres with r = band.
//
// ---- semantics: nothing new ------------------------------------------------------------------------------------------------------------
// Voxel e = x + nx * (y + ny * z) has the centre p = (lattice_centre(o, c, s) per axis) of crossings.h.  Its answer is closest::brute_force(p, band): among
// the triangles with a surface and d2 <= band * band, d2 = point_tri's, the smallest in (d2, id); none: id -1, d2 = band * band, q = p.  point_tri,
// tri_side, the skipping of triangles whose stored normal is 0, "a NaN d2 is never accepted" and "a NaN centre gives id -1" are closest.h's.
//
// ---- the key ---------------------------------------------------------------------------------------------------------------------------
// key = (uint64(bits of d2) << 32) | uint32(id).  An accepted d2 is a sum of squares or a square over a positive number: never negative, never -0, never
// NaN (NaN fails d2 <= r2); on such floats the unsigned order of the bits is the order of the values, so the unsigned order of keys IS (d2, id).  The empty
// slot is all ones: no accepted key has those bits (d2 would be a NaN).  A minimum does not depend on the order of arrival: the lattice is deterministic,
// whatever order the tasks run in and however the hardware orders the atomics.
//
// ---- the voxel box of a triangle, and THE MARGIN ----------------------------------------------------------------------------------------
// A triangle visits a BOX of voxels [c0, c1] per axis.  Pruning only skips what cannot be accepted; acceptance is `d2 <= r2` with point_tri's d2, and
// nothing else (there is no plane test, no earlier rejection).  The rule, per axis, with [lo, hi] the triangle's extent over v0, v0 - e1, v0 + e2 (the
// vertices as point_tri forms them), M = the largest of |coordinate| over the grid box and the two lattice corners o and o + float(n) * s, and of band,
// eps = 2^-16 * M and reach = band + eps:
//       f0 = ((lo - reach) - o) / s,  f1 = ((hi + reach) - o) / s,  c0 = floor(f0) - 1,  c1 = floor(f1) + 1,  both clamped to [0, n - 1]
// (the clamps are applied to the floats, so no cast overflows; a NaN -- which finite inputs cannot produce -- counts as "no bound on this side").
// Why it is conservative IN FLOAT32.  Let P be the centre of voxel c as the kernel computes it, a float: P = o + (c + 0.5) s + d with |d| <= 2^-22 M (float(c)
// is off by at most c * 2^-24 voxels, i.e. 2^-24 of the lattice's extent <= 2 M; the product and the sum round once each, results <= 2 M).  If the pair is
// accepted, point_tri's d2 <= fl(band * band).  A computed d2 differs from the true squared distance between P and the triangle of the rounded vertices by a
// few ulp of the coordinates plus a relative 2^-20 or so (closest.h, THE MARGIN: three-term dot products, one division), so the true distance is at most
// band * (1 + 2^-20) + 2^-20 M, and the distance along one axis from P to [lo, hi] is no larger.  Hence
//       (c + 0.5) s >= lo - band - o - (2^-20 band + 2^-20 M + 2^-22 M) > lo - band - o - eps / 4.
// The computed f0 comes from three roundings of values <= 4 M (2^-24 each: 2^-21 M in all, far below eps / 4) and one division (relative 2^-24 of f0, i.e.
// 2^-24 * 4 M in coordinate units), so f0 * s <= lo - band - eps - o + eps / 4.  Together: (c + 0.5) s > f0 * s + eps / 2, so c > f0 - 0.5, and
// c >= floor(f0) - 1 holds with half a voxel and eps / 2 to spare.  The upper end is the mirror image.  The band is part of M because its relative
// error (2^-20 band) must stay inside eps when the band is larger than every coordinate.  When a lattice corner overflows, M, eps and reach are +inf and
// every box is the whole lattice: slow, not wrong (such centres are +-inf, point_tri gives them NaN or inf, nothing is accepted: id -1).
// A triangle without a surface has the EMPTY box.
//
// ---- tasks -----------------------------------------------------------------------------------------------------------------------------
// The voxels of a box are numbered k = (x - x0) + bx * ((y - y0) + by * (z - z0)), x fastest; a TASK is a run of at most T consecutive numbers, so a box
// of v voxels has ceil(v / T) tasks and one wall-sized triangle is many tasks.  sizes -> exclusive scan -> task t belongs to the triangle j with
// offsets[j] <= t < offsets[j + 1] (find_task: a binary search; triangles without tasks are never found).  Consecutive lanes take consecutive k: runs along x.
// A task count per triangle is below 2^31 / T; the scan's sum may still leave 31 bits (a million wall-sized triangles): the splat then takes TRIANGLES
// instead of tasks, each with all its runs, and the result is the same.
//
// ---- splat and finish --------------------------------------------------------------------------------------------------------------------
// splat_voxel: point_tri for one (triangle, voxel); when d2 <= r2 the key is offered to the slot: a plain read first, the atomic minimum only when the key
// is smaller than what was read.  Slots only ever decrease, so a stale read is never smaller than the slot: it can cost an atomic, never a result.
// finish_voxel: the winner's record, recomputed by point_tri and tri_side -- the 32 bytes of hagrid_closest_points.
#ifndef HAGRID_DISTANCE_H
#define HAGRID_DISTANCE_H

#include "closest.h"
#include "crossings.h"
#include "prims.h"
#include "vec.h"

namespace hagrid {
namespace distance {

constexpr int kTaskVoxels = 2048;                       ///< T of the kernel: voxels per task
constexpr unsigned long long kEmpty = ~0ull;

HOST DEVICE inline unsigned long long make_key(float d2, int id) { return ((unsigned long long)as<uint32_t>(d2) << 32) | (unsigned long long)uint32_t(id); }
HOST DEVICE inline float key_d2(unsigned long long k) { return as<float>(uint32_t(k >> 32)); }
HOST DEVICE inline int key_id(unsigned long long k) { return int(uint32_t(k)); }

/// the lattice, the band and the reach of the box rule
struct Consts {
    float ox, oy, oz, sx, sy, sz;
    int nx, ny, nz;
    float band, r2, reach;
};

HOST DEVICE inline float abs1(float v) { return v < 0.0f ? -v : v; }

/// M of THE MARGIN over one axis: the grid box, the two lattice corners
HOST DEVICE inline float axis_largest(float grid_lo, float grid_hi, float o, float s, int n) {
    const float far = o + float(n) * s;
    return max(max(abs1(grid_lo), abs1(grid_hi)), max(abs1(o), abs1(far)));
}

/// made once, on the host; band is finite and >= 0
HOST inline Consts make_consts(const float* grid_lo, const float* grid_hi, const float* origin, const float* size, const int* n, float band) {
    Consts c;
    c.ox = origin[0]; c.oy = origin[1]; c.oz = origin[2];
    c.sx = size[0]; c.sy = size[1]; c.sz = size[2];
    c.nx = n[0]; c.ny = n[1]; c.nz = n[2];
    c.band = band; c.r2 = band * band;
    float m = band;
    for (int a = 0; a < 3; a++) m = max(m, axis_largest(grid_lo[a], grid_hi[a], origin[a], size[a], n[a]));
    c.reach = band + 1.52587890625e-05f * m;            // eps = 2^-16 * M
    return c;
}

/// [c0, c1] of one axis; empty when c0 > c1
HOST DEVICE inline void axis_range(float lo, float hi, float o, float s, int n, float reach, int& c0, int& c1) {
    float f0 = ((lo - reach) - o) / s, f1 = ((hi + reach) - o) / s;
    const float top = min(float(n) + 2.0f, 2147483520.0f);         // (the largest float below 2^31: the casts below cannot overflow)
    if (!(f0 == f0)) f0 = 0.0f;                         // NaN: no bound on this side
    if (!(f1 == f1)) f1 = top;
    if (f1 < -1.0f) { c0 = 0; c1 = -1; return; }        // floor(f1) + 1 < 0
    f0 = f0 > 0.0f ? f0 : 0.0f; f0 = f0 < top ? f0 : top;
    f1 = f1 > 0.0f ? f1 : 0.0f; f1 = f1 < top ? f1 : top;
    c0 = int(f0) - 1; c0 = c0 > 0 ? c0 : 0;            // f >= 0: the cast is the floor; a box beyond the lattice keeps c0 > n - 1
    c1 = int(f1); c1 = c1 < n - 2 ? c1 + 1 : n - 1;
}

struct Box {
    int x0, y0, z0, bx, by, bz;
    HOST DEVICE int voxels() const { return bx * by * bz; }                // <= the lattice's, which fit 31 bits
};

/// the voxel box of a triangle; empty (0 voxels) for a triangle without a surface
HOST DEVICE inline Box tri_box(const Tri& tri, const Consts& c) {
    Box b;
    b.x0 = b.y0 = b.z0 = 0; b.bx = b.by = b.bz = 0;
    const vec3 n = tri.normal();
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return b;
    const vec3 v1 = tri.v0 - tri.e1, v2 = tri.v0 + tri.e2;
    const vec3 lo = min(tri.v0, min(v1, v2)), hi = max(tri.v0, max(v1, v2));
    int x1, y1, z1;
    axis_range(lo.x, hi.x, c.ox, c.sx, c.nx, c.reach, b.x0, x1);
    axis_range(lo.y, hi.y, c.oy, c.sy, c.ny, c.reach, b.y0, y1);
    axis_range(lo.z, hi.z, c.oz, c.sz, c.nz, c.reach, b.z0, z1);
    if (x1 < b.x0 || y1 < b.y0 || z1 < b.z0) return b;
    b.bx = x1 - b.x0 + 1; b.by = y1 - b.y0 + 1; b.bz = z1 - b.z0 + 1;
    return b;
}

HOST DEVICE inline int num_tasks(int voxels, int task_voxels) { return voxels / task_voxels + (voxels % task_voxels ? 1 : 0); }

/// voxel number k of a box: its element in the lattice and its centre
HOST DEVICE inline int box_voxel(const Box& b, const Consts& c, int k, vec3& p) {
    const int row = int(unsigned(k) / unsigned(b.bx)), x = b.x0 + (k - row * b.bx);
    const int lz = int(unsigned(row) / unsigned(b.by)), y = b.y0 + (row - lz * b.by), z = b.z0 + lz;
    p = vec3(crossings::lattice_centre(c.ox, x, c.sx), crossings::lattice_centre(c.oy, y, c.sy), crossings::lattice_centre(c.oz, z, c.sz));
    return x + c.nx * (y + c.ny * z);
}

/// the centre of element e of the lattice
HOST DEVICE inline vec3 element_centre(const Consts& c, int e) {
    const int x = e % c.nx, yz = e / c.nx, y = yz % c.ny, z = yz / c.ny;
    return vec3(crossings::lattice_centre(c.ox, x, c.sx), crossings::lattice_centre(c.oy, y, c.sy), crossings::lattice_centre(c.oz, z, c.sz));
}

/// the triangle of task t: the last j in [0, n) with offset(j) <= t (offsets: the exclusive sums of the sizes; t is below their total)
template <typename F>
HOST DEVICE inline int find_task(F offset, int n, int t) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (offset(mid) <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/// one (triangle, voxel): true when the pair is within the band.  S: load(e) -> key (may be stale), take_min(e, key)
template <typename S>
HOST DEVICE inline bool splat_voxel(const Tri& tri, int id, const vec3& p, float r2, int e, S& slots) {
    closest::Pair r;
    if (!closest::point_tri(tri, p, r) || !(r.d2 <= r2)) return false;
    const unsigned long long key = make_key(r.d2, id);
    if (key < slots.load(e)) slots.take_min(e, key);
    return true;
}

/// the answer of a voxel from its slot.  tri_at(j) -> Tri
template <typename F>
HOST DEVICE inline void finish_voxel(F tri_at, unsigned long long key, const vec3& p, float r2, closest::Best& b) {
    b.init(p, r2);
    if (key == kEmpty) return;
    const int id = key_id(key);
    const Tri tri = tri_at(id);
    closest::Pair r;
    closest::point_tri(tri, p, r);
    b.id = id; b.d2 = r.d2; b.q = r.q; b.feature = r.feature; b.side = closest::tri_side(tri, p, r.q);
}

} // namespace distance
} // namespace hagrid

#endif // HAGRID_DISTANCE_H
