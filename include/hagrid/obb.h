// hagrid/obb.h -- oriented-box queries (hagrid_amd.h: hagrid_overlap_obbs): for a rotated (or sheared) box, the k smallest ids of the triangles that meet
// it.  The id list, paging by `first`, ANY, the clip, the walk and the argument (a) - (c) why it is sound are overlap.h's; this header adds the PAIR
// (box / triangle), the pair filter that carries it through overlap.h's brute_force and overlap_query, and a block PRUNE by the box's face normals, which
// is what keeps a thin diagonal box from visiting its whole bounding box.  No counterpart in the reference, which answers questions about rays only.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same functions serve the gfx950 kernel
// (hagrid_amd/csrc/overlap.hip: obb_tris_kernel) and host programs (tests/cpp/obb_host.cpp); hagrid_amd/scene.py (obb_pairs, overlap_obbs) states the pair
// and the query in numpy and gives the same truth values.
//
// ---- the record -----------------------------------------------------------------------------------------------------------------
// 64 bytes, four float4: c.xyz and int32 `first` (the pad slot, as a box record of overlap.h carries it), then u.xyz, v.xyz, w.xyz, each with pad 0.  The
// box is {c + a u + b v + g w : |a|, |b|, |g| <= 1}.  u, v, w need be neither normalised nor orthogonal -- a sheared box is legal -- and nothing here
// divides or normalises.  A record with a component that is not finite is INACTIVE: count 0, ids -1, no walk.  A zero axis (a FLAT box, a parallelogram
// or a segment) is legal and is answered by the same 13 axes as every other box: its face normals are zero or parallel and separate less, so where the
// pair is COPLANAR (the triangle lies in the plane of the flat box) the test is CONSERVATIVE -- it may say "meet" for a pair that lies apart inside that
// plane.  The exactness statement below is for boxes with volume only.
//
// ---- the pair -------------------------------------------------------------------------------------------------------------------
// The triangle's vertices are tritri::Verts (v0, v0 - e1, v0 + e2, each rounded once), its edges their differences.  obb_meets(box, tri) is true when NO
// axis of the separating-axis test strictly separates.  The 13 axes, in this order, one at a time (none is kept):
//    1..3    cross(v, w), cross(w, u), cross(u, v)        the face normals of the box (face_normal(i))
//    4       the stored normal of the triangle
//    5..13   cross(box axis i, triangle edge j), i outer, j inner
// On an axis L the box projects to centre dot(L, c), radius (|dot(L, u)| + |dot(L, v)|) + |dot(L, w)|; the triangle to dot(L, vertex).  Separated when
// min > centre + radius or max < centre - radius.  A zero axis projects everything to 0 and separates nothing; a NaN projection (overflow) compares
// false and separates nothing.
// EXACTNESS.  With every coordinate of c, u, v, w and of the triangle's vertices a multiple of 1/2 and |coordinate| <= 16: triangle edges are multiples of
// 1/2 up to 32; face normals multiples of 1/4 up to 2 * 16 * 16 = 2^9; the stored normal a multiple of 1/4 up to 2 * 32 * 32 = 2^11; cross axes
// multiples of 1/4 up to 2 * 16 * 32 = 2^10; a projection is a multiple of 1/8 up to 3 * 2^11 * 16 < 2^17, the radius up to 3 * that, centre +- radius
// up to 4 * that < 2^19: every product and every partial sum is a multiple of 1/8 below 2^19, an integer below 2^22 < 2^24 in units of 1/8.  On such
// input the float32 predicate is the exact one (tests/golden/make_golden_obb.py pins that against rational arithmetic and another algorithm).
//
// ---- the query ------------------------------------------------------------------------------------------------------------------
// S = {j >= first : pair not skipped, triangle j has a surface, j meets aabb(box), obb_meets(box, j)}.  aabb(box) = c -+ ((|u| + |v|) + |w|) per
// component, grown by eps = GridConsts::abs_margin on every side (obb_box), then clipped as every box of overlap.h is; "meets" is overlap::meets.  As for
// the contact queries the precondition removes nothing in exact arithmetic (a shared point lies in the box, so in its bounding box, and in the grid), and
// it makes the walk sound by (a) - (c) of overlap.h as they stand, because every member of S meets an axis-aligned box.  Huge axes are legal: the
// bounding box then has infinite bounds, which the clip takes to the grid box, and projections that overflow separate nothing.
// Labels: optionally ONE int32 per query against three per scene triangle (labels_shared(q, -1, -1, ...)), both arrays or neither: a pair is SKIPPED when
// the query's label is >= 0 and is one of the triangle's three.  With body ids as labels a body's box does not see the body's own triangles.
// The second count is of the pairs offered to obb_meets.
//
// ---- the prune ------------------------------------------------------------------------------------------------------------------
// overlap.h's walk drops a sub-block whose INTEGER voxel range misses the query's.  For a thin box along the grid diagonal that range is most of the grid.
// FacePrune also drops a block that a FACE NORMAL of the box separates from the box: with L = face_normal(i) -- the very bits obb_meets uses as axes 1..3 --,
// the block [x0, x1] x [y0, y1] x [z0, z1] (face coordinates float(corner) * cell_size + lo, centre m, half extents h) projects to
// dot(L, m) +- ((|L.x| h.x + |L.y| h.y) + |L.z| h.z), the box to D +- r with D = dot(L, c), r = (|dot(L, u)| + |dot(L, v)|) + |dot(L, w)|, and
//         dropped when   |dot(L, m) - D| - block radius  >  r + eps * l1,      l1 = (|L.x| + |L.y|) + |L.z|.
// Nothing is divided and no root is taken: the gap in units of distance is the left side minus r, over |L|, and l1 >= |L|, so eps * l1 takes at least
// eps of distance off it (capsule.h, axis test (ii)).  L, D and R = r + eps * l1 are made AGAIN for every block asked about, one normal at a time, from
// the record read again: held across the walk they are 15 floats, and the walk has no such room under the kernel's 128 registers.  The
// same prune is asked of a top-level cell before its word is read.  A zero normal (a flat box) has R = 0 and 0 > 0 drops nothing; inf or NaN on either
// side compares false -- which is also how the prune is switched OFF: with eps = inf, R is inf (or NaN for a zero normal).
// THE MARGIN.  Let M be the largest |coordinate| of the grid box and u = 2^-23 M one ulp of it, so eps = 128 u.  The argument is made for queries with
// every component of c, u, v, w within 4 M (far_box below switches the float prune OFF for any other query; the integer range then prunes alone, as in
// overlap.h).  L is the computed cross product and is taken as it is: the separating-axis argument holds for ANY axis when the true projections are
// used, so only the projections carry error, and all of it is counted in units of u * l1:
//   * a dot product of L with a vector whose components are at most K M: each product rounds by at most 2^-24 K M |L_i| = K/2 u |L_i|, each of the two
//     sums by as much of l1: at most 1.5 K u l1.  D (K = 4): 6;  the three terms of r: 18, their two sums (values up to 12 M l1): 12 more;
//     adding eps * l1 to make R: 8;
//   * the block's faces are off by at most 2 u each (THE MARGIN of closest.h), so m by 2.5 u and h by 2 u per component (|m|, h <= M): dot(L, m)
//     carries 2.5 from m and 1.5 of its own, the block radius 2 and 1.5;
//   * the subtraction of D (values up to 5 M l1) 4, the subtraction of the block radius 4.
// In all under 62 u l1, and with the few u of the build's own overlap decisions under 64 u l1: HALF of the eps * l1 = 128 u l1 that is taken off.
// WHY IT IS SOUND.  The axis is one of obb_meets's own, bit for bit, and obb_meets evaluates it with projections of the same accuracy: a triangle it lets
// pass has a point p in the box (up to rounding far below eps, (c) of overlap.h) and in the grid.  On L the true projection of p lies inside the true
// interval of the box and inside that of every block that holds p's voxel, so for such a block the true left side is <= r, the computed one
// <= r + 64 u l1 < R: the block is kept, at every level above the leaf of that voxel, and by (a) the leaf's cell lists the triangle.  The integer range
// contains the voxel as before.  For components beyond 4 M the errors grow with |c| / M while eps does not: no float prune there.
#ifndef HAGRID_OBB_H
#define HAGRID_OBB_H

#include "overlap.h"

namespace hagrid {
namespace obb {

/// the box {c + a u + b v + g w : |a|, |b|, |g| <= 1}
struct Obb {
    vec3 c, u, v, w;
    /// axis i (0, 1, 2; taken mod 3 up to 5): u, v, w.  Selected value by value: a select between the members themselves would put the box into memory
    HOST DEVICE vec3 axis(int i) const {
        const bool a = i == 0 || i == 3, b = i == 1 || i == 4;
        return vec3(a ? u.x : (b ? v.x : w.x), a ? u.y : (b ? v.y : w.y), a ? u.z : (b ? v.z : w.z));
    }
    /// face normal i (0, 1, 2): cross(v, w), cross(w, u), cross(u, v)
    HOST DEVICE vec3 face_normal(int i) const { return cross(axis(i + 1), axis(i + 2)); }
};

/// the 64-byte record as it lies in memory
struct ObbRecord { float c[3]; int first; float u[3], pad_u, v[3], pad_v, w[3], pad_w; };

HOST DEVICE inline Obb from_record(const ObbRecord& r) {
    Obb b;
    b.c = vec3(r.c[0], r.c[1], r.c[2]); b.u = vec3(r.u[0], r.u[1], r.u[2]); b.v = vec3(r.v[0], r.v[1], r.v[2]); b.w = vec3(r.w[0], r.w[1], r.w[2]);
    return b;
}

HOST DEVICE inline bool finite1(float a) { return detail::fabs1(a) <= 3.4028234663852886e38f; }      // false for NaN and inf
HOST DEVICE inline bool finite3(const vec3& a) { return finite1(a.x) && finite1(a.y) && finite1(a.z); }
/// every component finite?  (else the query is INACTIVE)
HOST DEVICE inline bool admissible(const Obb& b) { return finite3(b.c) && finite3(b.u) && finite3(b.v) && finite3(b.w); }

/// does the axis strictly separate the box from the triangle?
HOST DEVICE inline bool axis_separates(const vec3& L, const Obb& b, const tritri::Verts& t) {
    using detail::fabs1;
    using detail::fmax2;
    using detail::fmin2;
    const float centre = dot(L, b.c);
    const float radius = (fabs1(dot(L, b.u)) + fabs1(dot(L, b.v))) + fabs1(dot(L, b.w));
    const float p0 = dot(L, t.v0), p1 = dot(L, t.v1), p2 = dot(L, t.v2);
    const float lo = fmin2(p0, fmin2(p1, p2)), hi = fmax2(p0, fmax2(p1, p2));
    return lo > centre + radius || hi < centre - radius;
}

/// what an axis is made from is made inside its loop iteration: no normal, edge or cross product is computed ahead of the loops and carried through them
HOST DEVICE inline void made_here(vec3& a) { HAGRID_MADE_HERE(a.x); HAGRID_MADE_HERE(a.y); HAGRID_MADE_HERE(a.z); }
HOST DEVICE inline void made_here(Obb& b) { made_here(b.u); made_here(b.v); made_here(b.w); }
HOST DEVICE inline void made_here(tritri::Verts& t) { made_here(t.v0); made_here(t.v1); made_here(t.v2); }

/// does the triangle meet the box?  (the 13 axes above)  The loops are kept as loops: a kernel that evaluates one axis at a time holds one axis in registers.
HOST DEVICE inline bool obb_meets(const Obb& b_, const Tri& tri) {
    Obb b = b_;
    tritri::Verts t(tri);
    HAGRID_NOUNROLL
    for (int i = 0; i < 3; i++) {
        if (axis_separates(b.face_normal(i), b, t)) return false;
    }
    if (axis_separates(tri.normal(), b, t)) return false;
    HAGRID_NOUNROLL
    for (int i = 0; i < 3; i++) {
        HAGRID_NOUNROLL
        for (int j = 0; j < 3; j++) {
            if (axis_separates(cross(b.axis(i), t.edge(j)), b, t)) return false;
        }
    }
    return true;
}

/// aabb(box) grown by eps (the grid's absolute margin) on every side.  false: the query is INACTIVE.
HOST DEVICE inline bool obb_box(const Obb& b, float eps, vec3& lo, vec3& hi) {
    using detail::fabs1;
    if (!admissible(b)) return false;
    const float rx = (fabs1(b.u.x) + fabs1(b.v.x)) + fabs1(b.w.x), ry = (fabs1(b.u.y) + fabs1(b.v.y)) + fabs1(b.w.y), rz = (fabs1(b.u.z) + fabs1(b.v.z)) + fabs1(b.w.z);
    lo = vec3((b.c.x - rx) - eps, (b.c.y - ry) - eps, (b.c.z - rz) - eps);
    hi = vec3((b.c.x + rx) + eps, (b.c.y + ry) + eps, (b.c.z + rz) + eps);
    return true;
}

/// The pair filter of an oriented-box query (overlap.h: NoFilter, TriFilter).  Q: box() -> Obb, labelled() -> bool, label() -> the query's one label,
/// tri_label(id, i) -> label i of scene triangle id.
template <typename Q>
struct ObbFilter {
    Q q;
    HOST DEVICE bool counts_box_tests() const { return false; }
    HOST DEVICE bool accept(int id, const Tri& t, int& tests) const {
        if (q.labelled() && overlap::labels_shared(q.label(), -1, -1, q.tri_label(id, 0), q.tri_label(id, 1), q.tri_label(id, 2))) return false;
        if (!tri_has_surface(t)) return false;
        tests++;
        return obb_meets(q.box(), t);
    }
};

/// the float prune is proved for boxes with every component within 4 M of the origin (THE MARGIN): eps = 2^-16 M
HOST DEVICE inline bool far_box(float eps, const Obb& b) {
    using detail::fabs1;
    const float lim = eps * 262144.0f;          // 4 M
    const vec3 m(detail::fmax2(detail::fmax2(fabs1(b.c.x), fabs1(b.u.x)), detail::fmax2(fabs1(b.v.x), fabs1(b.w.x))),
                 detail::fmax2(detail::fmax2(fabs1(b.c.y), fabs1(b.u.y)), detail::fmax2(fabs1(b.v.y), fabs1(b.w.y))),
                 detail::fmax2(detail::fmax2(fabs1(b.c.z), fabs1(b.u.z)), detail::fmax2(fabs1(b.v.z), fabs1(b.w.z))));
    return !(m.x <= lim && m.y <= lim && m.z <= lim);
}

/// The block prune of an oriented-box query (overlap.h: NoPrune).  Q as for ObbFilter.  It keeps NOTHING of the box across the walk (its switch is the value of eps): the record is
/// read again for every block asked about and L, D, R are made one normal at a time (the kernel's registers: DESIGN.md 4.16).
template <typename Q>
struct FacePrune {
    Q q;
    float eps;              ///< the grid's margin; +inf: OFF (the host programs' switch, or a box beyond 4 M) -- R is then inf or NaN, nothing is dropped and
                            ///< the integer range prunes alone

    HOST DEVICE void set(const Q& q_, const Obb& b, float eps_, bool use) { q = q_; eps = (use && !far_box(eps_, b)) ? eps_ : __builtin_inff(); }
    /// is the block of 2^s voxels per axis at voxel (x, y, z) separated from the box by a face normal?
    HOST DEVICE bool drops(const overlap::GridConsts& c, int x, int y, int z, int s) const {
        using detail::fabs1;
        HAGRID_MADE_HERE(x); HAGRID_MADE_HERE(y); HAGRID_MADE_HERE(z);        // nothing of a block is computed ahead of the walk's loops and carried through them
        const int e = 1 << s;
        const float x0 = float(x) * c.cell_size.x + c.lo.x, x1 = float(x + e) * c.cell_size.x + c.lo.x;
        const float y0 = float(y) * c.cell_size.y + c.lo.y, y1 = float(y + e) * c.cell_size.y + c.lo.y;
        const float z0 = float(z) * c.cell_size.z + c.lo.z, z1 = float(z + e) * c.cell_size.z + c.lo.z;
        const vec3 m((x0 + x1) * 0.5f, (y0 + y1) * 0.5f, (z0 + z1) * 0.5f), h((x1 - x0) * 0.5f, (y1 - y0) * 0.5f, (z1 - z0) * 0.5f);
        const Obb b = q.box();
        HAGRID_NOUNROLL
        for (int i = 0; i < 3; i++) {
            const vec3 L = b.face_normal(i);
            const float D = dot(L, b.c);
            const float r = (fabs1(dot(L, b.u)) + fabs1(dot(L, b.v))) + fabs1(dot(L, b.w));
            const float R = r + eps * ((fabs1(L.x) + fabs1(L.y)) + fabs1(L.z));
            const float t = dot(L, m) - D;
            const float rb = (fabs1(L.x) * h.x + fabs1(L.y) * h.y) + fabs1(L.z) * h.z;
            if (fabs1(t) - rb > R) return true;
        }
        return false;
    }
};

/// the definition of the oriented-box query: every triangle, in order.  `eps`: the grid's absolute margin.  Returns the number of pairs offered to obb_meets.
template <typename F, typename L, typename Q>
HOST DEVICE inline int obb_brute_force(F tri_at, int num_tris, const overlap::Clip& clip, float eps, const Q& q, bool any, L& list) {
    vec3 lo, hi;
    if (!obb_box(q.box(), eps, lo, hi)) return 0;
    ObbFilter<Q> f = {q};
    return overlap::brute_force(tri_at, num_tris, clip, lo, hi, any, list, f);
}

/// the oriented-box query over the grid g: equal to obb_brute_force over all triangles.  `list` arrives initialised (init(k, first)).  float_prune =
/// false leaves the face normals out of the walk: the same answer over more cells (host programs measure with it what the prune saves).
template <typename G, typename S, typename L, typename Q>
HOST DEVICE inline void obb_query(const G& g, S& st, const Q& q, bool any, L& list, overlap::Counts& n, bool float_prune = true) {
    n.cells = 0; n.sats = 0; n.pruned = 0;
    vec3 lo, hi;
    FacePrune<Q> prune;
    {
        const Obb b = q.box();
        if (!obb_box(b, g.c.eps, lo, hi)) return;
        prune.set(q, b, g.c.eps, float_prune);
    }
    ObbFilter<Q> f = {q};
    overlap::overlap_query(g, st, lo, hi, any, list, n, f, prune);
}

} // namespace obb
} // namespace hagrid

#endif // HAGRID_OBB_H
