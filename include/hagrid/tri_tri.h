// hagrid/tri_tri.h -- the triangle / triangle pair of the contact queries (hagrid_amd.h: hagrid_overlap_tris; the query, the list and the walk: overlap.h).
// No counterpart in the reference, which answers questions about rays only.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same function serves the gfx950 kernel
// (hagrid_amd/csrc/overlap.hip) and host programs (tests/cpp/overlap_tris_host.cpp); hagrid_amd/scene.py (tri_tri_pairs) states the same operations in
// numpy and gives the same truth values.
//
// ---- the pair -------------------------------------------------------------------------------------------------------------------
// The vertices of a triangle are v0, v1 = v0 - e1 and v2 = v0 + e2, each rounded once, as Tri::bbox forms them; its edges are the differences of these
// vertices, v0 - v1, v2 - v0 and v2 - v1; its normal is the stored one.  tri_meets(a, b) is true when NO axis of the separating-axis test strictly
// separates the projections p = dot(axis, vertex) of the two triangles: for every axis, minA > maxB || minB > maxA is false.  The axes are 17, taken in
// this order, one at a time (none is kept):
//    1      n_a
//    2..4   cross(n_a, ea_i)      the in-plane edge normals of a
//    5      n_b
//    6..8   cross(n_b, eb_j)      the in-plane edge normals of b
//    9..17  cross(ea_i, eb_j), i outer, j inner
// The six in-plane axes are what separates COPLANAR pairs: there the two normals are parallel, every cross(ea, eb) is parallel to them as well, and the
// other eleven axes all project both triangles to one point each.  Without them every coplanar pair in one plane "meets".
// Why the projections are those of the VERTICES, and the edges their differences: two triangles that share a vertex bit for bit project it to the same
// float on every axis, so no axis separates them there, whatever the rounding of the rest -- neighbours in a mesh are reported reliably.  (Projections
// formed from v0 and the stored edges, dot(axis, v0) - dot(axis, e1), reach a shared vertex by two routes and two roundings: on the stadium mesh that form
// called 931 of 3442 touching pairs apart.)  And everything the test reads is the 18 floats of the six vertices and the two normals.
// A zero axis (parallel edges) projects everything to 0 and separates nothing; a NaN projection (overflow) compares false and separates nothing.
// With integer coordinates |c| <= 16 every product and sum above is an integer below 2^24 (edges <= 32, normals <= 2^11, in-plane axes <= 2^17,
// projections <= 3 * 16 * 2^17), so the float32 predicate is the exact one on such input (tests/golden/make_golden_overlap_tris.py pins that against
// rational arithmetic).
#ifndef HAGRID_TRI_TRI_H
#define HAGRID_TRI_TRI_H

#include "multi_hit.h"
#include "prims.h"
#include "vec.h"

namespace hagrid {
namespace tritri {

/// the three vertices as Tri::bbox forms them
struct Verts {
    vec3 v0, v1, v2;
    HOST DEVICE explicit Verts(const Tri& t) : v0(t.v0), v1(t.v0 - t.e1), v2(t.v0 + t.e2) {}
    /// edge i (0, 1, 2): v0 - v1, v2 - v0, v2 - v1
    HOST DEVICE vec3 edge(int i) const { return i == 0 ? v0 - v1 : (i == 1 ? v2 - v0 : v2 - v1); }
};

/// does the axis strictly separate the projections of the two triangles?
HOST DEVICE inline bool axis_separates(const vec3& ax, const Verts& a, const Verts& b) {
    using detail::fmax2;
    using detail::fmin2;
    const float a0 = dot(ax, a.v0), a1 = dot(ax, a.v1), a2 = dot(ax, a.v2);
    const float b0 = dot(ax, b.v0), b1 = dot(ax, b.v1), b2 = dot(ax, b.v2);
    const float min_a = fmin2(a0, fmin2(a1, a2)), max_a = fmax2(a0, fmax2(a1, a2));
    const float min_b = fmin2(b0, fmin2(b1, b2)), max_b = fmax2(b0, fmax2(b1, b2));
    return min_a > max_b || min_b > max_a;
}

} // namespace tritri

/// do the two triangles meet?  (the 17 axes above)  The loops are kept as loops: a kernel that evaluates one axis at a time holds one axis in registers.
HOST DEVICE inline bool tri_meets(const Tri& a, const Tri& b) {
    using namespace tritri;
    const Verts va(a), vb(b);
    {
        const vec3 n = a.normal();
        if (axis_separates(n, va, vb)) return false;
        HAGRID_NOUNROLL
        for (int i = 0; i < 3; i++)
            if (axis_separates(cross(n, va.edge(i)), va, vb)) return false;
    }
    {
        const vec3 n = b.normal();
        if (axis_separates(n, va, vb)) return false;
        HAGRID_NOUNROLL
        for (int j = 0; j < 3; j++)
            if (axis_separates(cross(n, vb.edge(j)), va, vb)) return false;
    }
    HAGRID_NOUNROLL
    for (int i = 0; i < 3; i++) {
        HAGRID_NOUNROLL
        for (int j = 0; j < 3; j++)
            if (axis_separates(cross(va.edge(i), vb.edge(j)), va, vb)) return false;
    }
    return true;
}

/// has the triangle a surface?  A stored normal of (0, 0, 0) says no (closest.h; the bad-index triangles of hagrid_scene_assemble are such)
HOST DEVICE inline bool tri_has_surface(const Tri& t) { return !(t.nx == 0.0f && t.ny == 0.0f && t.nz == 0.0f); }

} // namespace hagrid

#endif // HAGRID_TRI_TRI_H
