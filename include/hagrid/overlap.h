// hagrid/overlap.h -- box-overlap queries (hagrid_amd.h: hagrid_overlap_boxes, hagrid_overlap_lattice): for an axis-aligned box, the k smallest
// ids of the triangles that meet it.  No counterpart in the reference, which answers questions about rays only.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same functions serve the gfx950
// kernel (hagrid_amd/csrc/overlap.hip) and host programs (tests/cpp/overlap_host.cpp); hagrid_amd/scene.py (overlap_pairs, overlap_boxes,
// lattice_boxes) states the same operations in numpy and gives the same bits.
//
// ---- one triangle, one box ------------------------------------------------------------------------------------------------------
// Triangle j MEETS the box [lo, hi] exactly when intersect_tri_box<true, true>(v0, e1, e2, n, lo, hi) of prims.h says so: the plane of
// the triangle against the box, the three box axes, the nine cross axes, in the expression order of that header.  As a truth value this
// is the reference's intersect_prim_cell AND the bounds check -- the test the build itself inserts triangles with, plus the box axes.
//
// ---- the query ------------------------------------------------------------------------------------------------------------------
// A box record is 32 bytes, the layout of BBox: min.xyz, int32 `first` (the pad slot after min), max.xyz, pad 0.  With
// S = {j >= first : j meets the box}, m = |S| and 1 <= k <= 8 the answer is the min(k, m) smallest ids of S, ascending, in k slots (unused
// slots -1), and count = min(m, k + 1): k + 1 says "there are more".  So the list for k is a prefix of the list for k + 1, and a caller
// pages through S by asking again with first = last id + 1.  "The k smallest ids" does not care how often a triangle is offered.
//   * ALL of S (hagrid_amd.h: hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs) comes from the same walk with a third list type, RefList,
//     which keeps nothing: every triangle that `wants` lets through and that meets the box is a REFERENCE -- counted and, while the query's room lasts,
//     handed to a store in walk order.  THE DUPLICATE MODEL: a triangle is referenced by several cells, the build inserts by the separating-axis test and
//     not by the bounding box (so no cell is the canonical owner of a triangle inside a box), and expanded cell boxes overlap -- a triangle arrives once
//     per visit of a cell that lists it, and only the cell tested last is recognised.  So R, the number of references of a query, is a property of the
//     grid and the walk; R >= m, and the set of ids among the references is exactly S.  The sorted, duplicate-free list -- the pages of the k-list
//     concatenated -- is one segmented sort away (hagrid/unique_lists.h): a reference is stored as the entry {+0.0f, id}, so that sort orders by id alone.
//   * an INACTIVE box -- a NaN bound, or min > max on an axis -- has count 0, ids -1 and takes no walk;
//   * a box with min == max is a point and gets whatever the test says;
//   * THE CLIP: the query runs over a grid, and before anything else the box is clipped to the grid box grown by eps = GridConsts::abs_margin
//     on every side (Clip: lo = fmax2(lo, grid min - eps), hi = fmin2(hi, grid max + eps)); S is defined by the test against the CLIPPED box, in
//     the brute force as in the walk.  Every triangle lies inside the grid box ((b) below), so in exact arithmetic this removes no triangle
//     from S; a box inside the grown grid box keeps its bits.  What it buys: infinite and huge bounds are legal and well defined.  Handed to
//     the test as they are they would make the box centre and half extent inf or NaN (or swallow the triangle's coordinates), the cross axes
//     would never separate, and triangles whose bounding box overlaps the box but which have no point in it would count as meeting it -- an
//     answer no walk over cells can reproduce.  A box that the clip turns inside out lies beyond the grid and meets nothing.
//   * ANY (HAGRID_OVERLAP_ANY, k = 1): the walk stops at the first triangle that meets the box; the id is SOME member of S or -1, count 0 or 1.
// The lattice form makes its boxes itself: voxel (x, y, z) of an nx * ny * nz lattice, x fastest, is lo = origin + float(c) * size,
// hi = origin + float(c + 1) * size per axis (neighbouring voxels share their faces bit for bit), first = 0.
//
// ---- the list -------------------------------------------------------------------------------------------------------------------
// IdList keeps the ids in eight compile-time slots (the HitList of multi_hit.h on ids only: every loop over compile-time indices, so the
// array lives in registers), sorted, each id once.  `more` is set when a triangle that meets the box is not in a full list (it was
// refused, or it fell off the end).  Which triangles skip the test: ids below `first` and ids already listed, always; ids above the
// last slot of a full list once `more` is set -- they can change neither the list nor the flag.
//
// ---- the walk -------------------------------------------------------------------------------------------------------------------
// overlap_query walks the construction format (entries -> cells | small_cells -> ref_ids) and returns exactly what brute_force gives
// over all triangles, both for the clipped box.  (1) The box's voxel range: both corners moved OUTWARD by eps = GridConsts::abs_margin (2^-16 of the largest
// |coordinate| of the grid box, the margin of closest.h), to voxel coordinates, clamped in float to [0, dims - 1], cast; a box that lies
// beyond a face of the grid by more than the margin ends here.  (2) The top-level cells of that range.  (3) Each one's sub-blocks,
// keeping a sub-block only if its INTEGER voxel range meets the box's: no float pruning, no ring search.  (4) The list of the cell of
// every leaf reached; the cell tested last is recognised and skipped, and testing a cell twice changes nothing.  Why it is sound:
//   (a) a cell's reference list holds every triangle that meets the cell's box (closest.h (a): the build puts a triangle into every voxel
//       it overlaps, merging unites lists, expansion grows a cell only over neighbours whose lists are subsets or whose extra triangles
//       miss the grown region);
//   (b) every triangle lies inside the grid box, so the part of a box beyond a face of the grid meets nothing (the bounds check refuses it);
//   (c) the clipped box is finite and no larger than the grid box plus the margin, so the test runs on coordinates of the scene's magnitude and
//       is the separating-axis test it is meant to be: a triangle that meets the box has a point inside it (up to rounding far below eps) and
//       inside the grid; the voxel that holds this point lies in the voxel range
//       -- the float voxel coordinate of a corner is off by a few ulp of the largest coordinate, and the build's own decision for that
//       voxel (the same test in float, the truncating casts of compute_range) by a few more: all far inside eps = 128 ulp -- and the
//       leaf of that voxel is reached, because the integer range of every sub-block above it contains the voxel; by (a) the cell of the
//       leaf lists the triangle.
// Three counts per box: cells visited, triangle / box tests evaluated, sub-blocks pruned.  A query may bring a BLOCK PRUNE of its own (NoPrune, the
// default, drops nothing; obb.h's FacePrune): it is asked of every sub-block next to the integer range, and of every top-level cell of the range.
//
// ---- contact queries (hagrid_amd.h: hagrid_overlap_tris) ----------------------------------------------------------
// A query may be a TRIANGLE A instead of a box: S = {j >= first : no label >= 0 of A is a label of j, j has a surface, j meets box(A), tri_meets(A, j)} with
// tri_meets of tri_tri.h and box(A) = A's bounding box grown by eps on every side, then clipped as every box is (query_box).  Everything above stays as it
// is: test_cell, brute_force and overlap_query take a PAIR FILTER that a triangle which meets the box must pass as well (NoFilter, the default, lets
// everything pass); TriFilter is the filter of this query, tris_query and tris_brute_force the two ends.  The walk is sound by (a) - (c) as they stand,
// because every member of S meets a box.  The second count is then of the pairs offered to tri_meets.
#ifndef HAGRID_OVERLAP_H
#define HAGRID_OVERLAP_H

#include "block_walk.h"
#include "grid.h"
#include "multi_hit.h"
#include "prims.h"
#include "tri_tri.h"
#include "vec.h"

namespace hagrid {
namespace overlap {

// GridConsts, CellRec, ArrayStack, kMaxLevels: block_walk.h, which names them in this namespace as well

constexpr int kMaxIds = 8;

struct Counts { int cells, sats, pruned; };

/// the pair: does the triangle meet the box?
HOST DEVICE inline bool meets(const Tri& tri, const vec3& lo, const vec3& hi) {
    return intersect_tri_box<true, true>(tri.v0, tri.e1, tri.e2, tri.normal(), lo, hi);
}

/// a NaN bound, or min > max on an axis
HOST DEVICE inline bool inactive(const vec3& lo, const vec3& hi) { return !(lo.x <= hi.x) || !(lo.y <= hi.y) || !(lo.z <= hi.z); }

/// the grid box grown by the absolute margin: what every query box is clipped to before the test (THE CLIP above)
struct Clip {
    vec3 lo, hi;
    HOST DEVICE void set(const vec3& grid_lo, const vec3& grid_hi) {
        const float eps = GridConsts::abs_margin(grid_lo, grid_hi);
        lo = vec3(grid_lo.x - eps, grid_lo.y - eps, grid_lo.z - eps);
        hi = vec3(grid_hi.x + eps, grid_hi.y + eps, grid_hi.z + eps);
    }
    /// false: nothing is left of the box (it was inactive, or it lies beyond the grid)
    HOST DEVICE bool apply(vec3& blo, vec3& bhi) const {
        if (inactive(blo, bhi)) return false;
        blo = vec3(detail::fmax2(blo.x, lo.x), detail::fmax2(blo.y, lo.y), detail::fmax2(blo.z, lo.z));
        bhi = vec3(detail::fmin2(bhi.x, hi.x), detail::fmin2(bhi.y, hi.y), detail::fmin2(bhi.z, hi.z));
        return !inactive(blo, bhi);
    }
};

/// voxel c of a lattice along one axis
HOST DEVICE inline float lattice_face(float origin, int c, float size) { return origin + float(c) * size; }

template <int KMAX>
struct IdList {
    int id[KMAX];
    int cap;            ///< k: slots in use, 1 .. KMAX
    int last;           ///< copy of slot cap - 1: the list is full when last >= 0
    int first;          ///< only ids >= first take part
    bool more;          ///< a triangle that meets the box is not in the (full) list

    HOST DEVICE void init(int k, int first_) {
        cap = k; last = -1; first = first_; more = false;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) id[j] = -1;
    }

    HOST DEVICE bool found() const { return id[0] >= 0; }

    /// does `ref` need the test at all?
    HOST DEVICE bool wants(int ref) const {
        if (ref < first) return false;
        if (more && last >= 0 && ref > last) return false;
        bool dup = false;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) dup = dup || id[j] == ref;
        return !dup;
    }

    /// `ref` meets the box (and wants() said yes): it sinks to its sorted place, pushing the rest one slot down; what is left over at the
    /// end -- `ref` itself or the id that fell off slot cap - 1 -- is a member of S outside the list
    HOST DEVICE void take(int ref) {
        int ci = ref;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) {
            const bool t = j < cap && (id[j] < 0 || ci < id[j]);
            const int oi = id[j];
            id[j] = t ? ci : oi;
            ci = t ? oi : ci;
        }
        if (ci >= 0) more = true;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++)
            if (j == cap - 1) last = id[j];
    }

    /// min(m, k + 1)
    HOST DEVICE int count() const {
        int c = more ? 1 : 0;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) c += (j < cap && id[j] >= 0) ? 1 : 0;
        return c;
    }
};

/// Every member of S as it arrives, duplicates included (the header: THE DUPLICATE MODEL).  STORE: store(position, id), called for the first `room`
/// references.  Never "found": a walk with this list runs to its end (there is no ANY).
template <typename STORE>
struct RefList {
    int count;          ///< references so far (R when the walk is over)
    int room;           ///< references the store takes
    int first;          ///< only ids >= first take part
    STORE store;

    HOST DEVICE void init(int first_) { first = first_; count = 0; }
    HOST DEVICE bool found() const { return false; }
    HOST DEVICE bool wants(int ref) const { return ref >= first; }
    HOST DEVICE void take(int ref) {
        if (count < room) store(count, ref);
        count++;
    }
};

/// The pair filter of a query: what a triangle that meets the box must pass as well to be a member of S.  accept(id, tri, tests) -> bool, where `tests`
/// is the query's count of tests evaluated; counts_box_tests() says whether that count is of the triangle / box tests (a filter that says no counts its
/// own).  This one lets everything pass: the box queries.
struct NoFilter {
    HOST DEVICE bool counts_box_tests() const { return true; }
    HOST DEVICE bool accept(int, const Tri&, int&) const { return true; }
};

/// The block prune of a query: drops(c, x, y, z, s) -> true leaves out the block of 2^s voxels per axis at voxel (x, y, z) -- a sub-block, or a top-level
/// cell before its word is read -- although its integer voxel range meets the box's.  This one drops nothing: the box and contact queries.  (obb.h: FacePrune)
struct NoPrune {
    HOST DEVICE bool drops(const GridConsts&, int, int, int, int) const { return false; }
};

/// the definition: every triangle, in order, against the clipped box.  tri_at(j) -> Tri.  Returns the number of tests evaluated.
template <typename F, typename L, typename P = NoFilter>
HOST DEVICE inline int brute_force(F tri_at, int num_tris, const Clip& clip, const vec3& box_lo, const vec3& box_hi, bool any, L& list, const P& filter = P()) {
    int sats = 0;
    vec3 lo = box_lo, hi = box_hi;
    if (!clip.apply(lo, hi)) return sats;
    for (int j = 0; j < num_tris; j++) {
        if (!list.wants(j)) continue;
        if (filter.counts_box_tests()) sats++;
        const Tri t = tri_at(j);
        if (meets(t, lo, hi) && filter.accept(j, t, sats)) {
            list.take(j);
            if (any) break;
        }
    }
    return sats;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------

struct VoxelRange { int lx, ly, lz, hx, hy, hz; };     ///< inclusive

/// a float voxel coordinate into [0, dmax] (NaN -> 0), then the cast
HOST DEVICE inline int clamp_cast(float f, float dmax) {
    float a = f > 0.0f ? f : 0.0f;
    a = a < dmax ? a : dmax;
    return int(a);
}

/// false: the box lies beyond a face of the grid
HOST DEVICE inline bool voxel_range(const GridConsts& c, const vec3& lo, const vec3& hi, VoxelRange& r) {
    const float lx = ((lo.x - c.eps) - c.lo.x) * c.inv.x, ly = ((lo.y - c.eps) - c.lo.y) * c.inv.y, lz = ((lo.z - c.eps) - c.lo.z) * c.inv.z;
    const float hx = ((hi.x + c.eps) - c.lo.x) * c.inv.x, hy = ((hi.y + c.eps) - c.lo.y) * c.inv.y, hz = ((hi.z + c.eps) - c.lo.z) * c.inv.z;
    const float dx = float(c.dims.x), dy = float(c.dims.y), dz = float(c.dims.z);
    if (hx < 0.0f || hy < 0.0f || hz < 0.0f || lx >= dx || ly >= dy || lz >= dz) return false;
    r.lx = clamp_cast(lx, float(c.dims.x - 1)); r.ly = clamp_cast(ly, float(c.dims.y - 1)); r.lz = clamp_cast(lz, float(c.dims.z - 1));
    r.hx = clamp_cast(hx, float(c.dims.x - 1)); r.hy = clamp_cast(hy, float(c.dims.y - 1)); r.hz = clamp_cast(hz, float(c.dims.z - 1));
    return true;
}

/// does the block of 2^s voxels per axis at (x, y, z) miss the range?
HOST DEVICE inline bool misses(const VoxelRange& r, int x, int y, int z, int s) {
    const int e = 1 << s;
    return x > r.hx || x + e <= r.lx || y > r.hy || y + e <= r.ly || z > r.hz || z + e <= r.lz;
}

/// the list of one cell.  G: c (GridConsts), clip (Clip), word(i), cell(i) -> CellRec, ref(i), tri(id)
template <typename G, typename L, typename P = NoFilter>
HOST DEVICE inline void test_cell(const G& g, const vec3& lo, const vec3& hi, bool any, uint32_t index, L& list, Counts& n, const P& filter = P()) {
    const CellRec c = g.cell(index);
    n.cells++;
    if (c.begin < 0) return;
    for (int i = c.begin; i < c.end; i++) {
        const int ref = g.ref(i);
        if (ref < 0) break;
        if (!list.wants(ref)) continue;
        if (filter.counts_box_tests()) n.sats++;
        const Tri t = g.tri(ref);
        if (meets(t, lo, hi) && filter.accept(ref, t, n.sats)) {
            list.take(ref);
            if (any) return;
        }
    }
}

/// one top-level cell of the range: descend its sub-blocks (block_walk.h) while their voxel ranges meet the box's
template <typename G, typename S, typename L, typename P = NoFilter, typename B = NoPrune>
HOST DEVICE inline void visit_top(const G& g, S& st, const vec3& lo, const vec3& hi, bool any, const VoxelRange& r, int tx, int ty, int tz, uint32_t& last_cell,
                                  L& list, Counts& n, const P& filter = P(), const B& region = B()) {
    const GridConsts& c = g.c;
    auto prune = [&](int x, int y, int z, int s) {
        const bool out = misses(r, x, y, z, s) || region.drops(c, x, y, z, s);
        if (out) n.pruned++;
        return out;
    };
    auto leaf = [&](uint32_t ci) {                      // true: ANY has its triangle
        if (ci == last_cell) return false;
        last_cell = ci;
        test_cell(g, lo, hi, any, ci, list, n, filter);
        return any && list.found();
    };
    const uint32_t top_w = g.word(uint32_t(tx + c.top.x * (ty + c.top.y * tz)));
    if (!(top_w & 3u)) leaf(top_w >> 2);
    else blocks::descend_top(g, st, top_w, tx, ty, tz, prune, leaf);
}

/// the answer for the box [lo, hi] over the grid g: equal to brute_force over all triangles (with ANY: some member of S, or none).
/// `list` arrives initialised (init(k, first)).
template <typename G, typename S, typename L, typename P = NoFilter, typename B = NoPrune>
HOST DEVICE inline void overlap_query(const G& g, S& st, const vec3& box_lo, const vec3& box_hi, bool any, L& list, Counts& n, const P& filter = P(), const B& region = B()) {
    const GridConsts& c = g.c;
    n.cells = 0; n.sats = 0; n.pruned = 0;
    vec3 lo = box_lo, hi = box_hi;
    if (!g.clip.apply(lo, hi)) return;
    VoxelRange r;
    if (!voxel_range(c, lo, hi, r)) return;
    uint32_t last_cell = 0xffffffffu;
    const int x0 = r.lx >> c.shift, x1 = r.hx >> c.shift, y0 = r.ly >> c.shift, y1 = r.hy >> c.shift, z0 = r.lz >> c.shift, z1 = r.hz >> c.shift;
    for (int z = z0; z <= z1; z++)
        for (int y = y0; y <= y1; y++)
            for (int x = x0; x <= x1; x++) {
                if (region.drops(c, x << c.shift, y << c.shift, z << c.shift, c.shift)) { n.pruned++; continue; }
                visit_top(g, st, lo, hi, any, r, x, y, z, last_cell, list, n, filter, region);
                if (any && list.found()) return;
            }
}

// ---- contact queries: a triangle asks -------------------------------------------------------------------------------------------

/// The box of a query triangle: its bounding box grown by eps (the grid's absolute margin) on every side.  false: the query is INACTIVE -- not
/// admissible (a coordinate or a derived vertex that is not finite), or without a surface (stored normal 0).
HOST DEVICE inline bool query_box(const Tri& q, float eps, vec3& lo, vec3& hi) {
    if (!tri_admissible(q) || !tri_has_surface(q)) return false;
    const BBox b = q.bbox();
    lo = vec3(b.min.x - eps, b.min.y - eps, b.min.z - eps);
    hi = vec3(b.max.x + eps, b.max.y + eps, b.max.z + eps);
    return true;
}

/// Does a label >= 0 of the query equal a label of the triangle?
HOST DEVICE inline bool labels_shared(int q0, int q1, int q2, int t0, int t1, int t2) {
    return (q0 >= 0 && (q0 == t0 || q0 == t1 || q0 == t2)) || (q1 >= 0 && (q1 == t0 || q1 == t1 || q1 == t2)) || (q2 >= 0 && (q2 == t0 || q2 == t1 || q2 == t2));
}

/// The pair filter of a contact query.  Q: tri() -> the query triangle, labelled() -> bool, label(i) -> label i of the query, tri_label(id, i) -> label i of
/// scene triangle id.  A pair that shares a label is skipped; a triangle without a surface takes no part; the rest is offered to tri_meets and counted.
template <typename Q>
struct TriFilter {
    Q q;
    HOST DEVICE bool counts_box_tests() const { return false; }
    HOST DEVICE bool accept(int id, const Tri& t, int& tests) const {
        if (q.labelled() && labels_shared(q.label(0), q.label(1), q.label(2), q.tri_label(id, 0), q.tri_label(id, 1), q.tri_label(id, 2))) return false;
        if (!tri_has_surface(t)) return false;
        tests++;
        return tri_meets(q.tri(), t);
    }
};

/// the definition of the contact query: every triangle, in order.  `eps`: the grid's absolute margin.  Returns the number of pairs offered to tri_meets.
template <typename F, typename L, typename Q>
HOST DEVICE inline int tris_brute_force(F tri_at, int num_tris, const Clip& clip, float eps, const Q& q, bool any, L& list) {
    vec3 lo, hi;
    if (!query_box(q.tri(), eps, lo, hi)) return 0;
    TriFilter<Q> f = {q};
    return brute_force(tri_at, num_tris, clip, lo, hi, any, list, f);
}

/// the contact query over the grid g: equal to tris_brute_force over all triangles.  `list` arrives initialised (init(k, first)).
template <typename G, typename S, typename L, typename Q>
HOST DEVICE inline void tris_query(const G& g, S& st, const Q& q, bool any, L& list, Counts& n) {
    n.cells = 0; n.sats = 0; n.pruned = 0;
    vec3 lo, hi;
    if (!query_box(q.tri(), g.c.eps, lo, hi)) return;
    TriFilter<Q> f = {q};
    overlap_query(g, st, lo, hi, any, list, n, f);
}

} // namespace overlap
} // namespace hagrid

#endif // HAGRID_OVERLAP_H
