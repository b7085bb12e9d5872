// hagrid/capsule.h -- capsule queries (hagrid_amd.h: hagrid_segment_tris): for a segment a -> b and a radius r, the k triangles nearest to the SEGMENT within
// r, nearest first, paged -- the edge-edge half of a cloth step's proximity pairs, a character's or a robot link's capsule, "does this cable clear the mesh
// by r".  It is closest.h's neighbour query (NearList, cursor, labels, THE MARGIN) with one new pair function (segment - triangle), one new lower bound
// (segment - block) and the walk that carries them.  No counterpart in the reference.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same functions serve the gfx950 kernel (the segment
// mode of nearest_tris_kernel, hagrid_amd/csrc/capsule.hip) and host programs (tests/cpp/segments_host.cpp); hagrid_amd/scene.py (segment_pairs,
// segment_tris) states the same operations in numpy and gives the same bits.
//
// ---- one segment, one triangle: seg_tri -------------------------------------------------------------------------------------------
// d = b - a.  The result is d2, the closest point q ON THE TRIANGLE, the parameter s in [0, 1] of the closest point c = a + d * s ON THE SEGMENT, and the
// feature.  A triangle whose stored normal is (0, 0, 0) has no surface and takes no part.  Six candidates, in this order; a later one replaces an earlier
// one only when its d2 is strictly smaller (so an earlier one wins a tie, and a NaN d2 replaces nothing):
//   1. the end a: point_tri(tri, a) of closest.h -- d2, q and feature 0 .. 3 as it gives them, s = 0;
//   2. the end b: point_tri(tri, b), s = 1;
//   3 .. 5. the segment against the triangle's three edges in point_tri's order (1: e = v0, u = -e1;  2: e = v1, u = v2 - v1;  3: e = v0, u = e2), the
//      clamped closest pair of two segments, feature 1, 2 or 3.  With clamp(x) = `x > 0 ? x : 0` then `x < 1 ? x : 1` (NaN -> 0, as in segment_d2):
//        A = dot(d, d).  A == 0 (a segment of no length): the candidate IS segment_d2(a, e, u), operation for operation, with s = 0.  Otherwise
//        w = a - e, E = dot(u, u), F = dot(u, w), C = dot(d, w);
//        E == 0 (an edge of no length):  t = 0, s = clamp(-C / A);
//        otherwise  B = dot(d, u), den = A * E - B * B;
//                   s = den > 0 ? clamp((B * F - C * E) / den) : 0        (parallel, or den lost to rounding: start from the end a)
//                   t = (B * s + F) / E
//                   not (t >= 0)  (negative or NaN):  t = 0, s = clamp(-C / A)
//                   else t > 1:                       t = 1, s = clamp((B - C) / A);
//        c = a + d * s, q = e + u * t, d2 = dot(c - q, c - q).  No division by zero is ever made: A and E are tested before they divide, den > 0 before
//        it does.
//   6. piercing: h_a = dot(a - v0, n), h_b = dot(b - v0, n).  When one is > 0 and the other < 0:  s = h_a / (h_a - h_b)  (the divisor's magnitude is at
//      least |h_a|, rounding being monotonic, so 0 <= s <= 1), x = a + d * s, and if x passes point_tri's three inside tests
//      (dot(cross(e1, x - v0), n) >= 0, dot(cross(x - v1, v2 - v1), n) >= 0, dot(cross(e2, x - v0), n) >= 0) and dot(n, n) > 0 the candidate is d2 = 0,
//      q = x, feature 4.
// side = tri_side(tri, c, q) with c = a + d * s.
//
// WHY SIX ARE ENOUGH (in exact arithmetic).  The distance between a point of the segment and a point of the triangle is a convex function on the product
// of two convex sets.  If its minimum is 0 the segment meets the triangle: in its interior (6), or on its boundary (3 .. 5).  If it is positive and attained
// at a pair (c, q) with c an end of the segment, 1 or 2 finds it; with q on the boundary of the triangle, 3 .. 5 find it.  What is left is c interior to the
// segment and q interior to the face: then c - q is perpendicular to both, the segment is parallel to the plane, and the pair can be slid along d at the same
// distance until c reaches an end or q the boundary -- a pair one of 1 .. 5 finds.
//
// PROMISE.  With a == b the result is point_tri(tri, a)'s d2, q and feature with s = +0, bit for bit: 2 repeats 1 and is not strictly smaller; 3 .. 5 are
// the three segment_d2 values point_tri itself took the smallest of, or beat with the face; h_a == h_b, so 6 does not apply.
//
// ---- the query --------------------------------------------------------------------------------------------------------------------
// A segment record is 32 bytes: ax, ay, az, r; bx, by, bz, 0.  r2 = r * r (+inf allowed).  r < 0 is an inactive query (every slot d2 = -1, id -1); a NaN or
// infinite coordinate or a NaN radius gives id -1, d2 = r2 everywhere: neither walks.  Candidates, cursor, order, unused slots and paging are NearList's
// (closest.h) with seg_tri's d2 in place of point_tri's.  A query carries TWO labels (an edge's two vertex indices; -1: unused): the pair is skipped when a
// label >= 0 equals one of the triangle's three.  The record of a slot is {qx, qy, qz, d2}, {id, feature, side, s}: hagrid_closest_points' record with s in
// the word that is 0 there, made again from the winner's id after the walk; an unused slot: q = a, the slot's d2, id -1, feature = side = 0, s = +0.
//
// ---- the walk: segment_query --------------------------------------------------------------------------------------------------------
// (a), (b), (c) of closest.h hold for a segment as they do for a point: a triangle's distance to the segment is at least the distance from the segment to
// any box that contains the part of the triangle in question.  From closest.h the walk takes test_cell, visit_top and face_room as they are,
// with (a, b) as the query, block_beyond below as visit_top's lower bound and the cells of a and b as its home cells.  Its own: it tests the cells that hold
// a and b (each end clamped into the grid) for a first best; the capsule (segment, sqrt(best)) stays inside the box of a's cell when BOTH ends have
// face_room (when b lies in another cell its distance to one of those faces is negative and the test fails by itself); the rings lie around the BOX of
// top-level cells the two ends span: ring 0 is that box, ring k the shell k cells around it, and the lower bound of ring k is the gap from the segment's
// bounding box to the nearest face of the cube of rings before it that still has grid behind it.
//
// THE LOWER BOUND of segment to block is the larger of two, each sound on its own because both shapes are convex (any axis on which their projections lie
// apart by g proves a distance of at least g):
//   (i)  box to box: per axis the gap between [min(a, b), max(a, b)] and the block's interval -- axis_gap with an interval in place of p -- shrunk by eps,
//        squared and summed;
//   (ii) the axes L = cross(d, e_x) = (0, d.z, -d.y), cross(d, e_y) = (-d.z, 0, d.x), cross(d, e_z) = (d.y, -d.x, 0).  L is perpendicular to d, so the
//        segment projects to the one point dot(a, L); the block with centre m and half extents h projects to dot(m, L) +- (|L.x| h.x + |L.y| h.y + |L.z| h.z).
//        The gap is g = (|dot(m - a, L)| - rad) / |L|.  Written without the division and without a root, with l1 = |L.x| + |L.y| + |L.z| >= |L|:
//            num = |dot(m - a, L)| - rad - eps * l1, clamped at 0;        beyond when  dot(L, L) >= 2^-60  and  num * num > best * (1 + 2^-10) * dot(L, L).
//        An axis with dot(L, L) below 2^-60 (a segment along a coordinate axis, or of no length, or one whose squares underflow) is LEFT OUT: nothing is
//        ever divided, and NaN or inf on the right (best = inf) fails the `>`.
// "Beyond" is either of the two being beyond: the larger of the bounds exceeds the best.  Without (ii) a long diagonal segment's box is the scene and
// nothing is pruned.
//
// THE MARGIN, extended.  (i) is THE MARGIN of closest.h word for word: the interval's ends are the ends' coordinates, exact.  (ii) has longer arithmetic.
// Let M be the largest |coordinate| of the grid box and u = 2^-23 M one ulp of it, so eps = 128 u.  The ends of a segment may lie outside the grid; the
// argument is made for |a|, |b| <= 4 M per coordinate (far_ends below switches (ii) off for any other query).  Then:
//   * the computed d~ = b - a has components up to 8 M and differs from d by at most 4 u per component (half an ulp of the result), 7 u in length.  SAT
//     holds for ANY axis if the segment's true projection is used: on L~ = cross(d~, e) the true segment projects to an interval of width
//     |dot(d - d~, L~)| <= 7 u |L~| around dot(a, L~) -- 7 u in units of g, at most 7 u l1 in units of num;
//   * m and h are half sums and half differences of face coordinates, each off by at most 2 u (THE MARGIN); m - a has components up to 5 M and is off by
//     at most 4 u per component (2 u of m, 2 u of the subtraction); each of its two products with L's non-zero components rounds by up to 2^-24 of
//     5 M |L_i| = 2.5 u |L_i|, and so does their sum: |dot(m - a, L)| is off by at most 9 u l1;
//   * rad: 2 u l1 from h, u l1 from its two products and its sum (h <= M): 3 u l1;
//   * the two subtractions that make num, of magnitudes up to 5 M l1: 2.5 u l1 each.
// In all at most 24 u l1, and with the few u of the build's own overlap decisions under 32 u l1: a quarter of the eps l1 = 128 u l1 taken off num.
// Replacing |L| by l1 >= |L| only shrinks more: eps l1 / |L| lies between eps and sqrt(2) eps in units of distance.  On the right, dot(L, L) and the
// product with best are off by a relative 2^-22 or so, inside the 2^-10 -- as long as neither has underflowed: an axis is used only when dot(L, L) >= 2^-60
// (not merely != 0: below that its two squares may be denormal and the sum carries no relative accuracy) and when the right-hand side is a normal number
// or best is exactly 0 (then the right-hand side is exactly 0 and num > 0 after the shrink is a true gap).  An underflow of num * num on the left only
// loses a prune.  For ends farther out than 4 M the errors grow with |a| / M while eps does not; (i), whose terms are differences of the ends' own
// coordinates to face coordinates and whose error is relative to the distance itself, prunes alone there under the 2^-10.
// A tie with the k-th best is never pruned: equality does not satisfy `>`.
#ifndef HAGRID_CAPSULE_H
#define HAGRID_CAPSULE_H

#include "closest.h"

namespace hagrid {
namespace capsule {

using closest::Pair; using closest::Counts; using closest::NearList; using closest::GridConsts; using closest::CellRec;
using closest::point_tri; using closest::segment_d2; using closest::tri_side; using closest::shrink; using closest::beyond; using closest::face;
using closest::test_cell; using closest::visit_top; using closest::face_room;

struct SegPair { float d2; vec3 q; float s; int feature; };

HOST DEVICE inline float clamp01(float x) { x = x > 0.0f ? x : 0.0f; return x < 1.0f ? x : 1.0f; }

/// candidate 3 .. 5: the segment a + d * s against the edge e + u * t; A = dot(d, d).  q on the edge, s on the segment
HOST DEVICE inline float seg_edge(const vec3& a, const vec3& d, float A, const vec3& e, const vec3& u, vec3& q, float& s) {
    if (A == 0.0f) { s = 0.0f; return segment_d2(a, e, u, q); }
    const vec3 w = a - e;
    const float E = dot(u, u), F = dot(u, w), C = dot(d, w);
    float t;
    if (E == 0.0f) { t = 0.0f; s = clamp01(-C / A); }
    else {
        const float B = dot(d, u);
        const float den = A * E - B * B;
        s = den > 0.0f ? clamp01((B * F - C * E) / den) : 0.0f;
        t = (B * s + F) / E;
        if (!(t >= 0.0f)) { t = 0.0f; s = clamp01(-C / A); }
        else if (t > 1.0f) { t = 1.0f; s = clamp01((B - C) / A); }
    }
    const vec3 c = a + d * s;
    q = e + u * t;
    const vec3 cq = c - q;
    return dot(cq, cq);
}

/// false: the triangle has no surface (stored normal 0) and takes no part
HOST DEVICE inline bool seg_tri(const Tri& tri, const vec3& a, const vec3& b, SegPair& r) {
    const vec3 n = tri.normal();
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return false;
    float d2 = 0.0f, s = 0.0f; vec3 q = a; int f = 0;
    HAGRID_NOUNROLL
    for (int k = 0; k < 2; k++) {               // the ends: one body of point_tri in the kernel, not two
        Pair pk;
        point_tri(tri, k ? b : a, pk);
        if (k == 0 || pk.d2 < d2) { d2 = pk.d2; q = pk.q; f = pk.feature; s = k ? 1.0f : 0.0f; }
    }
    const vec3 v0 = tri.v0, v1 = v0 - tri.e1, v2 = v0 + tri.e2;
    const vec3 u1(-tri.e1.x, -tri.e1.y, -tri.e1.z), u2 = v2 - v1;
    const vec3 d = b - a;
    const float A = dot(d, d);
    HAGRID_NOUNROLL
    for (int k = 1; k <= 3; k++) {              // rolled: the kernel's registers
        vec3 qk; float sk;
        const float dk = seg_edge(a, d, A, k == 2 ? v1 : v0, k == 1 ? u1 : (k == 2 ? u2 : tri.e2), qk, sk);
        if (dk < d2) { d2 = dk; q = qk; f = k; s = sk; }
    }
    const vec3 a0 = a - v0;
    const float ha = dot(a0, n), hb = dot(b - v0, n);
    if ((ha > 0.0f && hb < 0.0f) || (ha < 0.0f && hb > 0.0f)) {
        const float sx = ha / (ha - hb);
        const vec3 x = a + d * sx;
        const vec3 x0 = x - v0, x1 = x - v1;
        const float s1 = dot(cross(tri.e1, x0), n), s2 = dot(cross(x1, u2), n), s3 = dot(cross(tri.e2, x0), n);
        if (s1 >= 0.0f && s2 >= 0.0f && s3 >= 0.0f && dot(n, n) > 0.0f && 0.0f < d2) { d2 = 0.0f; q = x; f = 4; s = sx; }
    }
    r.d2 = d2; r.q = q; r.s = s; r.feature = f;
    return true;
}

/// NearList with the two labels of a segment query and seg_tri as its pair function
template <int KMAX>
struct SegList : NearList<KMAX> {
    int label_b;                ///< the second label; the first is NearList's
    HOST DEVICE void setup(int k, float cursor_d2, int cursor_id, int label_a_, int label_b_, const int* labels) {
        NearList<KMAX>::setup(k, cursor_d2, cursor_id, label_a_, labels);
        label_b = label_b_;
    }
    HOST DEVICE void offer(const Tri& tri, int ref, const vec3& a, const vec3& b) {
        if (this->tri_labels && (this->label >= 0 || label_b >= 0)) {
            const int* l = this->tri_labels + 3 * size_t(ref);
            const int l0 = l[0], l1 = l[1], l2 = l[2];
            if (this->label >= 0 && (l0 == this->label || l1 == this->label || l2 == this->label)) return;
            if (label_b >= 0 && (l0 == label_b || l1 == label_b || l2 == label_b)) return;
        }
        SegPair r;
        if (!seg_tri(tri, a, b, r)) return;
        this->insert(r.d2, ref);
    }
};

/// the 32-byte answer for slot (id, d2) of a list, made again by seg_tri / tri_side after the walk
struct SegRecord { vec3 q; float d2; int id, feature, side; float s; };
template <typename F>
HOST DEVICE inline void slot_record(F tri_at, int id, float d2, const vec3& a, const vec3& b, SegRecord& o) {
    o.q = a; o.d2 = d2; o.id = -1; o.feature = 0; o.side = 0; o.s = 0.0f;
    if (id < 0) return;
    const Tri tri = tri_at(id);
    SegPair r;
    seg_tri(tri, a, b, r);
    const vec3 c = a + (b - a) * r.s;
    o.q = r.q; o.d2 = r.d2; o.id = id; o.feature = r.feature; o.side = tri_side(tri, c, r.q); o.s = r.s;
}

HOST DEVICE inline bool finite1(float x) { return detail::fabs1(x) <= 3.4028234663852886e38f; }     // false for NaN and +-inf

/// is the query answered without looking at a triangle?  (inactive; a NaN or infinite coordinate; a NaN radius)
template <typename A>
HOST DEVICE inline bool trivial_query(const vec3& a, const vec3& b, float r, A& l) {
    const float r2 = r * r;
    if (r < 0.0f) { l.init(a, -1.0f); return true; }
    l.init(a, r2);
    return !(finite1(a.x) && finite1(a.y) && finite1(a.z) && finite1(b.x) && finite1(b.y) && finite1(b.z)) || !(r2 == r2);
}

/// the definition: every triangle, in order.  tri_at(j) -> Tri
template <typename F, typename A>
HOST DEVICE inline void brute_force(F tri_at, int num_tris, const vec3& a, const vec3& b, float r, A& l) {
    if (trivial_query(a, b, r, l)) return;
    for (int j = 0; j < num_tris; j++) l.offer(tri_at(j), j, a, b);
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------

/// shrunk distance from the interval [plo, phi] to the interval [lo corner, hi corner] along one axis
HOST DEVICE inline float interval_gap(float plo, float phi, int lc, int hc, float cs, float lo, float eps) {
    const float x = face(lc, cs, lo) - phi, y = plo - face(hc, cs, lo);
    return shrink(x > y ? x : y, eps);
}

/// (ii) for one axis L = (+-p, -+q) over the two coordinates u, v it lives in: mu, mv = block centre - a; hu, hv = half extents; Lu, Lv = L's components
HOST DEVICE inline bool axis_beyond(float mu, float mv, float hu, float hv, float Lu, float Lv, float eps, float best_d2) {
    const float LL = Lu * Lu + Lv * Lv;
    const float au = detail::fabs1(Lu), av = detail::fabs1(Lv);
    const float t = mu * Lu + mv * Lv;
    const float num = shrink(detail::fabs1(t) - (au * hu + av * hv), eps * (au + av));
    const float rhs = best_d2 * 1.0009765625f * LL;
    const bool exact = LL >= 8.67361737988403547e-19f, right = best_d2 == 0.0f, normal = rhs >= 1.17549435082228751e-38f;     // 2^-60; the smallest normal
    return (int(exact) & (int(right) | int(normal)) & int(num * num > rhs)) != 0;            // no branches: the kernel's registers
}

/// is the block [l, h] (integer corners) certainly farther from the segment than best_d2?  sat: (ii) is in use
HOST DEVICE inline bool block_beyond(const GridConsts& c, const vec3& a_, const vec3& b_, bool sat, int lx, int ly, int lz, int hx, int hy, int hz, float best_d2) {
    vec3 a = a_, b = b_;
    HAGRID_MADE_HERE(a.x); HAGRID_MADE_HERE(a.y); HAGRID_MADE_HERE(a.z); HAGRID_MADE_HERE(b.x); HAGRID_MADE_HERE(b.y); HAGRID_MADE_HERE(b.z);
    const float gx = interval_gap(a.x < b.x ? a.x : b.x, a.x < b.x ? b.x : a.x, lx, hx, c.cell_size.x, c.lo.x, c.eps);
    const float gy = interval_gap(a.y < b.y ? a.y : b.y, a.y < b.y ? b.y : a.y, ly, hy, c.cell_size.y, c.lo.y, c.eps);
    const float gz = interval_gap(a.z < b.z ? a.z : b.z, a.z < b.z ? b.z : a.z, lz, hz, c.cell_size.z, c.lo.z, c.eps);
    if (beyond(gx * gx + gy * gy + gz * gz, best_d2)) return true;
    if (!sat) return false;
    const float x0 = face(lx, c.cell_size.x, c.lo.x), x1 = face(hx, c.cell_size.x, c.lo.x);
    const float y0 = face(ly, c.cell_size.y, c.lo.y), y1 = face(hy, c.cell_size.y, c.lo.y);
    const float z0 = face(lz, c.cell_size.z, c.lo.z), z1 = face(hz, c.cell_size.z, c.lo.z);
    const float mx = (x0 + x1) * 0.5f - a.x, my = (y0 + y1) * 0.5f - a.y, mz = (z0 + z1) * 0.5f - a.z;
    const float hx_ = (x1 - x0) * 0.5f, hy_ = (y1 - y0) * 0.5f, hz_ = (z1 - z0) * 0.5f;
    const vec3 d = b - a;
    HAGRID_NOUNROLL
    for (int k = 0; k < 3; k++) {               // axis k lives in the coordinates u = k + 1, v = k + 2 (mod 3): L_u = d_v, L_v = -d_u.  Rolled: the kernel's registers
        const float mu = k == 0 ? my : (k == 1 ? mz : mx), mv = k == 0 ? mz : (k == 1 ? mx : my);
        const float hu = k == 0 ? hy_ : (k == 1 ? hz_ : hx_), hv = k == 0 ? hz_ : (k == 1 ? hx_ : hy_);
        const float du = k == 0 ? d.y : (k == 1 ? d.z : d.x), dv = k == 0 ? d.z : (k == 1 ? d.x : d.y);
        if (axis_beyond(mu, mv, hu, hv, dv, -du, c.eps, best_d2)) return true;
    }
    return false;
}

/// (ii) is proved for ends within 4 M of the origin (THE MARGIN, extended): eps = 2^-16 M
HOST DEVICE inline bool far_ends(const GridConsts& c, const vec3& a, const vec3& b) {
    const float lim = c.eps * 262144.0f;        // 4 M
    return !(detail::fabs1(a.x) <= lim && detail::fabs1(a.y) <= lim && detail::fabs1(a.z) <= lim &&
             detail::fabs1(b.x) <= lim && detail::fabs1(b.y) <= lim && detail::fabs1(b.z) <= lim);
}

/// the voxel of p along one axis, p clamped into the grid
HOST DEVICE inline int voxel1(float p, float lo, float inv, int dim) {
    float f = (p - lo) * inv;
    f = f > 0.0f ? f : 0.0f;
    f = f < float(dim - 1) ? f : float(dim - 1);
    return int(f);
}

/// the answer for (a, b, r) over the grid g: equal, bit for bit, to brute_force over all triangles with the same accumulator.  use_axes = false leaves (ii)
/// out of the lower bound: the same answer over more triangles (host programs measure with it what (ii) prunes)
template <typename G, typename S, typename A>
HOST DEVICE inline void segment_query(const G& g, S& st, const vec3& a, const vec3& b, float r, A& l, Counts& n, bool use_axes = true) {
    const GridConsts& c = g.c;
    n.cells = 0; n.tris = 0; n.pruned = 0;
    if (trivial_query(a, b, r, l)) return;

    // the cells of a and b, each clamped into the grid
    const int ax = voxel1(a.x, c.lo.x, c.inv.x, c.dims.x), ay = voxel1(a.y, c.lo.y, c.inv.y, c.dims.y), az = voxel1(a.z, c.lo.z, c.inv.z, c.dims.z);
    const int bx = voxel1(b.x, c.lo.x, c.inv.x, c.dims.x), by = voxel1(b.y, c.lo.y, c.inv.y, c.dims.y), bz = voxel1(b.z, c.lo.z, c.inv.z, c.dims.z);
    const uint32_t cell_a = walk::descend(g, g.word(uint32_t((ax >> c.shift) + c.top.x * ((ay >> c.shift) + c.top.y * (az >> c.shift)))), ax, ay, az) >> 2;
    const uint32_t cell_b = walk::descend(g, g.word(uint32_t((bx >> c.shift) + c.top.x * ((by >> c.shift) + c.top.y * (bz >> c.shift)))), bx, by, bz) >> 2;
    const CellRec c0 = test_cell(g, cell_a, l, n, a, b);
    if (cell_b != cell_a) test_cell(g, cell_b, l, n, a, b);

    // does the capsule (segment, sqrt(best)) stay inside the box of a's cell?  faces on the grid boundary have nothing behind them
    const float big = 3.4028234663852886e38f;
    {
        const float m = face_room(c, c0, b, face_room(c, c0, a, big));
        if (m == big) return;                           // the cell is the whole grid
        const float ms = shrink(m, c.eps);
        if (beyond(ms * ms, l.d2)) return;
    }

    // rings of top-level cells around the box of top-level cells the ends span
    const bool sat = use_axes && !far_ends(c, a, b);
    auto far_block = [&](int lx, int ly, int lz, int hx, int hy, int hz) { return block_beyond(c, a, b, sat, lx, ly, lz, hx, hy, hz, l.d2); };
    auto home = [cell_a, cell_b](uint32_t ci) { return ci == cell_a || ci == cell_b; };       // by value: by reference the kernel is allocated differently
    uint32_t last_cell = cell_a;
    for (int k = 0;; k++) {
        // the cube of rings 0 .. k, from the ends once more: only its six corners are carried through the ring, not the box and the ring's ranges beside them
        vec3 ea = a, eb = b;
        HAGRID_MADE_HERE(ea.x); HAGRID_MADE_HERE(ea.y); HAGRID_MADE_HERE(ea.z); HAGRID_MADE_HERE(eb.x); HAGRID_MADE_HERE(eb.y); HAGRID_MADE_HERE(eb.z);
        const int vax = voxel1(ea.x, c.lo.x, c.inv.x, c.dims.x), vbx = voxel1(eb.x, c.lo.x, c.inv.x, c.dims.x);
        const int vay = voxel1(ea.y, c.lo.y, c.inv.y, c.dims.y), vby = voxel1(eb.y, c.lo.y, c.inv.y, c.dims.y);
        const int vaz = voxel1(ea.z, c.lo.z, c.inv.z, c.dims.z), vbz = voxel1(eb.z, c.lo.z, c.inv.z, c.dims.z);
        const int x0 = (min(vax, vbx) >> c.shift) - k, x1 = (max(vax, vbx) >> c.shift) + k;
        const int y0 = (min(vay, vby) >> c.shift) - k, y1 = (max(vay, vby) >> c.shift) + k;
        const int z0 = (min(vaz, vbz) >> c.shift) - k, z1 = (max(vaz, vbz) >> c.shift) + k;
        // lower bound of ring k >= 1: from the segment's bounding box to the nearest face of the cube of rings 0 .. k-1 that still has grid behind it
        float m = big;
        if (x0 + 1 > 0)   m = min(m, min(ea.x, eb.x) - face((x0 + 1) << c.shift, c.cell_size.x, c.lo.x));
        if (x1 < c.top.x) m = min(m, face(x1 << c.shift, c.cell_size.x, c.lo.x) - max(ea.x, eb.x));
        if (y0 + 1 > 0)   m = min(m, min(ea.y, eb.y) - face((y0 + 1) << c.shift, c.cell_size.y, c.lo.y));
        if (y1 < c.top.y) m = min(m, face(y1 << c.shift, c.cell_size.y, c.lo.y) - max(ea.y, eb.y));
        if (z0 + 1 > 0)   m = min(m, min(ea.z, eb.z) - face((z0 + 1) << c.shift, c.cell_size.z, c.lo.z));
        if (z1 < c.top.z) m = min(m, face(z1 << c.shift, c.cell_size.z, c.lo.z) - max(ea.z, eb.z));
        if (k == 0) m = 0.0f;                           // ring 0, the box itself, is always visited
        if (m == big) break;                            // the rings have left the grid
        const float ms = shrink(m, c.eps);
        if (beyond(ms * ms, l.d2)) break;

        for (int z = max(z0, 0); z <= min(z1, c.top.z - 1); z++) {
            const bool zface = k == 0 || z == z0 || z == z1;                // ring 0: every row whole
            for (int y = max(y0, 0); y <= min(y1, c.top.y - 1); y++) {
                const bool shell = zface || y == y0 || y == y1;             // the whole row belongs to the ring, else its two ends
                for (int x = shell ? max(x0, 0) : x0; x <= (shell ? min(x1, c.top.x - 1) : x1); x += shell ? 1 : x1 - x0) {
                    if (x < 0 || x >= c.top.x) continue;
                    visit_top(g, st, far_block, home, x, y, z, last_cell, l, n, a, b);
                }
            }
        }
    }
}

} // namespace capsule
} // namespace hagrid

#endif // HAGRID_CAPSULE_H
