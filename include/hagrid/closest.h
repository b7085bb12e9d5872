// hagrid/closest.h -- nearest-surface queries (hagrid_amd.h: hagrid_closest_points): for a point p and a radius r, the triangle
// nearest to p within r, the squared distance, the closest point on it, the feature that holds it and the side of the face p is on.
// No counterpart in the reference, which answers questions about rays only.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same functions serve the gfx950
// kernel (hagrid_amd/csrc/closest.hip) and host programs (tests/cpp/closest_host.cpp); hagrid_amd/scene.py (closest_pairs,
// closest_points) states the same operations in numpy and gives the same bits.
//
// ---- one point, one triangle ----------------------------------------------------------------------------------------------------
// The Tri record holds v0, e1 = v0 - v1, e2 = v2 - v0 and n = cross(e1, e2).  With v1 = v0 - e1, v2 = v0 + e2 (what Tri::bbox uses):
//   * three segments, in this order: 1: a = v0, ab = -e1 (to v1);  2: a = v1, ab = v2 - v1;  3: a = v0, ab = e2 (to v2).  For each:
//     t = dot(p - a, ab) / dot(ab, ab), clamped to [0, 1] by `t > 0 ? t : 0` then `t < 1 ? t : 1` (NaN -> 0: a segment of no length is
//     its start), q = a + ab * t, d2 = dot(p - q, p - q).  d2_edge is the smallest, an earlier segment winning a tie (strict <);
//   * p projects inside when dot(cross(e1, p - v0), n) >= 0, dot(cross(p - v1, v2 - v1), n) >= 0, dot(cross(e2, p - v0), n) >= 0 and
//     dot(n, n) > 0.  Then with h = dot(p - v0, n) the face candidate h * h / dot(n, n) wins when it is <= d2_edge, with
//     q = p - n * (h / dot(n, n)) and feature 0;
//   * side = sign(dot(p - q, n)) as +1, -1 or 0: the sign of the FACE normal, not a robust inside / outside at edges and vertices.
// This is the plane-and-segments form.  The barycentric-region form of the textbooks (products d1*d4 - d3*d2) loses the distance
// to cancellation on meshes; this form does not (DESIGN.md 4.6 has the figures).
// A triangle whose stored normal is (0, 0, 0) has no surface and is skipped (no ray hits it either); a candidate whose d2 is NaN is
// never accepted.
//
// ---- the query ------------------------------------------------------------------------------------------------------------------
// r2 = r * r (+inf allowed).  Among all triangles j with d2_j <= r2 the answer is the smallest in the order (d2 ascending, id
// ascending).  None: id -1, d2 = r2, q = p, feature = side = 0.  r < 0 is an inactive query (id -1, d2 = -1); a NaN coordinate or a
// NaN radius gives id -1.
//
// ---- the walk -------------------------------------------------------------------------------------------------------------------
// closest_query walks the construction format (entries -> cells | small_cells -> ref_ids) and returns exactly what the definition
// above gives over all triangles; pruning only ever skips triangles that cannot win.  Why it is sound:
//   (a) a cell's reference list holds every triangle that meets the cell's box: the build puts a triangle into every voxel it
//       overlaps, merging unites lists, and expansion grows a cell only over neighbours whose lists are subsets of its own (or,
//       in the precise mode, whose extra triangles miss the grown region);
//   (b) every triangle lies inside the grid box, so nothing lies beyond a face of the grid;
//   (c) a triangle's distance to p is at least the distance from p to any box that contains the part of it in question.
// So: the walk tests the list of the cell that holds p (p clamped into the grid); if the ball (p, sqrt(best)) stays inside that
// cell's box (faces on the grid boundary do not count, by (b)) it is done.  Otherwise it visits the top-level cells in rings
// (Chebyshev distance 0, 1, 2, ... from p's top-level cell), descends each one's sub-blocks while the box of the sub-block is not
// farther than the best so far, and tests the cells of the leaves it reaches.  A ring's lower bound is the distance from p to the
// nearest face of the cube of rings before it that still lies inside the grid; when that exceeds the best so far -- which starts as
// r2, so a query that has found nothing stops at its radius -- or no such face is left, the walk is over.
//
// THE MARGIN.  Every pruning comparison has the form `lower bound > best`.  The lower bound is made of float differences between p
// and face coordinates `float(corner) * cell_size + grid_min`; each is first reduced by eps = 2^-16 * (largest |coordinate| of the
// grid box) and clamped at 0, and the comparison is lower^2 > best * (1 + 2^-10).  eps is 128 ulp of the largest coordinate: the face
// coordinate and the difference are off by at most 2 ulp of it, the build's own overlap decisions (SAT in float, truncating casts of
// compute_range) by a few more, and a triangle's computed distance differs from its true one by a few ulp of the coordinates plus a
// relative 2^-20 or so (three-term dot products, one division) -- all far inside eps on the left and 2^-10 on the right.  A triangle
// that ties with the best (same d2, smaller id) is never pruned: equality does not satisfy `>`.
//
// A cell reached through several leaves may be tested again; offering a triangle twice changes nothing.  The cell of p and the cell
// tested last are recognised and skipped.  Three counts per query: cells visited, triangles tested, sub-blocks / top-level cells pruned.
//
// ---- the k nearest (hagrid_amd.h: hagrid_nearest_tris) --------------------------------------------------------------------------
// trivial_query, brute_force, test_cell, visit_top and closest_query are templates over the ACCUMULATOR: what is offered every triangle
// (offer), what a query starts from (init) and what the pruning compares with (the field d2).  test_cell and visit_top take the QUERY as a
// trailing pack that they hand to offer unread (p here; a, b in capsule.h), and visit_top the lower bound as a callable: one of each for every query shape.  Best keeps one answer; NearList<KMAX> keeps
// the k <= KMAX smallest CANDIDATES in the order (d2 ascending, id ascending).  Triangle j is a candidate of a query when point_tri gives it
// a surface, its d2 is not NaN, d2 <= r2, the pair is not skipped by the labels (the query's label is >= 0 and equals one of the triangle's
// three) and (d2, j) sorts strictly AFTER the query's cursor.  A cursor of d2 = -1 excludes nothing (every candidate has d2 >= 0), a cursor
// with a NaN d2 excludes everything; the cursor for the next page is the last slot of a FULL list.  Unused slots: d2 = r2, id -1.
// The list's pruning field d2 is r2 until the list is full, then the d2 of its last entry -- the k-th best so far.  THE MARGIN holds with one
// more sentence: a sub-block whose shrunk lower bound is beyond that value holds nothing that enters the list, because whatever enters
// sorts before the last entry and so has d2 <= its d2; a tie with the last entry is never pruned, because equality does not satisfy `>`.
// A triangle arrives once per cell that references it: one already in the list is dropped; one that fell off the end never comes back,
// because the last entry only decreases; one of an earlier page is kept out by the cursor order.  Hence: the list for k is a prefix of
// the list for k + 1, pages concatenated are all candidates sorted, and with k = 1, no cursor and no labels the entry is (d2, id) of Best.
// The k-list has no count of the ball's content: with pruning at the k-th best the walk never sees the rest.  A full list means "ask again" -- or ask RefSink:
//
// ---- the whole ball (hagrid_amd.h: hagrid_ball_refs) ------------------------------------------------------------------------------
// RefSink is the third accumulator: its pruning field d2 is r2 and NEVER MOVES, so one walk sees every candidate (the candidate rule above without a
// cursor).  It keeps nothing: an accepted offer -- a REFERENCE -- is counted and, while the query's room lasts, handed to a store as (position, d2, id) in walk
// order.  THE MARGIN holds as it stands: every pruning comparison is `lower bound > r2 * (1 + 2^-10)` with a constant on the right, a sub-block pruned holds
// nothing within r, a triangle at exactly r2 is never pruned (equality does not satisfy `>`).  What does NOT carry over is "offering a triangle twice changes
// nothing": a triangle arrives once per visit of a cell that lists it, so R, the number of references, is a property of the grid and the walk (R >= the
// number of candidates, the set of ids among them IS the candidate set, equal ids carry equal d2 bits).  The sorted, duplicate-free list is one segmented
// sort away: hagrid/unique_lists.h.
#ifndef HAGRID_CLOSEST_H
#define HAGRID_CLOSEST_H

#include "block_walk.h"
#include "cell_walk.h"
#include "grid.h"
#include "multi_hit.h"
#include "prims.h"
#include "vec.h"

namespace hagrid {
namespace closest {

struct Pair { float d2; vec3 q; int feature; };

/// squared distance from p to the segment a + ab * t, t in [0, 1]; q = the closest point
HOST DEVICE inline float segment_d2(const vec3& p, const vec3& a, const vec3& ab, vec3& q) {
    const vec3 ap = p - a;
    float t = dot(ap, ab) / dot(ab, ab);
    t = t > 0.0f ? t : 0.0f;
    t = t < 1.0f ? t : 1.0f;
    q = a + ab * t;
    const vec3 d = p - q;
    return dot(d, d);
}

/// false: the triangle has no surface (stored normal 0) and takes no part
HOST DEVICE inline bool point_tri(const Tri& tri, const vec3& p, Pair& r) {
    const vec3 n = tri.normal();
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return false;
    const vec3 v0 = tri.v0, v1 = v0 - tri.e1, v2 = v0 + tri.e2;
    const vec3 u1(-tri.e1.x, -tri.e1.y, -tri.e1.z), u2 = v2 - v1;
    vec3 q, qk;
    float d2 = segment_d2(p, v0, u1, q);
    int f = 1;
    float dk = segment_d2(p, v1, u2, qk);
    if (dk < d2) { d2 = dk; q = qk; f = 2; }
    dk = segment_d2(p, v0, tri.e2, qk);
    if (dk < d2) { d2 = dk; q = qk; f = 3; }
    const vec3 d0 = p - v0, d1 = p - v1;
    const float nn = dot(n, n);
    const float s1 = dot(cross(tri.e1, d0), n), s2 = dot(cross(d1, u2), n), s3 = dot(cross(tri.e2, d0), n);
    if (s1 >= 0.0f && s2 >= 0.0f && s3 >= 0.0f && nn > 0.0f) {
        const float h = dot(d0, n);
        const float df = h * h / nn;
        if (df <= d2) { d2 = df; q = p - n * (h / nn); f = 0; }
    }
    r.d2 = d2; r.q = q; r.feature = f;
    return true;
}

/// +1, -1 or 0: the side of the triangle's plane (by its stored normal) p lies on, seen from the closest point q
HOST DEVICE inline int tri_side(const Tri& tri, const vec3& p, const vec3& q) {
    const float s = dot(p - q, tri.normal());
    return s > 0.0f ? 1 : (s < 0.0f ? -1 : 0);
}

struct Best {
    int id; float d2; vec3 q; int feature, side;
    HOST DEVICE void init(const vec3& p, float r2) { id = -1; d2 = r2; q = p; feature = 0; side = 0; }
    /// would (c_d2, c_id) replace the answer so far?  NaN never does.
    HOST DEVICE bool takes(float c_d2, int c_id) const { return id < 0 ? c_d2 <= d2 : (c_d2 < d2 || (c_d2 == d2 && c_id < id)); }
    HOST DEVICE void offer(const Tri& tri, int ref, const vec3& p) {
        Pair r;
        if (point_tri(tri, p, r) && takes(r.d2, ref)) { id = ref; d2 = r.d2; q = r.q; feature = r.feature; side = tri_side(tri, p, r.q); }
    }
};

/// The k <= KMAX nearest candidates of one query, sorted by (d2, id), in the style of HitList (multi_hit.h): every loop runs over compile-time
/// indices, the capacity only appears in comparisons with them, nothing is indexed at run time -- the arrays live in registers on the device.
template <int KMAX>
struct NearList {
    int id[KMAX];
    float dd[KMAX];             ///< the entries' d2; an unused slot holds r2
    int cap;                    ///< k: slots in use, 1 .. KMAX
    float d2;                   ///< what the walk prunes with: r2 until the list is full, then the d2 of slot cap - 1
    int last_id;                ///< the id of slot cap - 1: the list is full when last_id >= 0
    float cur_d2; int cur_id;   ///< the cursor: only what sorts strictly after it is a candidate
    int label;                  ///< the query's label (< 0: skips nothing)
    const int* tri_labels;      ///< three labels per triangle, or null

    /// before init: k, the cursor ((-1, -1): none) and the labels (null: none)
    HOST DEVICE void setup(int k, float cursor_d2, int cursor_id, int query_label, const int* labels) {
        cap = k; cur_d2 = cursor_d2; cur_id = cursor_id; label = query_label; tri_labels = labels;
    }
    HOST DEVICE void init(const vec3&, float r2) {
        d2 = r2; last_id = -1;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) { id[j] = -1; dd[j] = r2; }
    }
    HOST DEVICE bool full() const { return last_id >= 0; }
    /// (da, ia) sorts before (db, ib)
    HOST DEVICE static bool before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

    HOST DEVICE void offer(const Tri& tri, int ref, const vec3& p) {
        if (tri_labels && label >= 0) {
            const int* l = tri_labels + 3 * size_t(ref);
            if (l[0] == label || l[1] == label || l[2] == label) return;
        }
        Pair r;
        if (!point_tri(tri, p, r)) return;
        insert(r.d2, ref);
    }
    /// the candidate (c, ref) of a pair that the labels do not skip: the rest of the candidate rule, and its place in the list (capsule.h offers seg_tri's d2 here)
    HOST DEVICE void insert(const float c, int ref) {
        if (!(c <= d2)) return;                                                 // NaN, or beyond r2 (d2 is never above r2)
        if (!(c > cur_d2 || (c == cur_d2 && ref > cur_id))) return;             // not after the cursor (a NaN cursor: nothing is)
        if (last_id >= 0 && !before(c, ref, d2, last_id)) return;               // cannot change a full list
        bool dup = false;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) dup = dup || id[j] == ref;
        if (dup) return;
        // the new entry sinks to its sorted place, pushing the rest one slot down; what falls off slot cap - 1 is dropped
        int ci = ref; float cd = c;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) {
            const bool take = j < cap && (id[j] < 0 || before(cd, ci, dd[j], id[j]));
            const int oi = id[j]; const float od = dd[j];
            id[j] = take ? ci : oi; dd[j] = take ? cd : od;
            ci = take ? oi : ci; cd = take ? od : cd;
        }
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++)
            if (j == cap - 1) { last_id = id[j]; d2 = dd[j]; }                  // an unused slot: -1 and r2, as before
    }

    /// slot j (a run-time value) without indexing at run time
    HOST DEVICE void get(int j, int& out_id, float& out_d2) const {
        out_id = -1; out_d2 = 0.0f;
        HAGRID_UNROLL
        for (int i = 0; i < KMAX; i++)
            if (i == j) { out_id = id[i]; out_d2 = dd[i]; }
    }
};

/// Every candidate of one query, as it arrives (the header: "the whole ball").  STORE: store(position, d2, id), called for the first `room` references.
/// offer / insert are split like NearList's, so that another query shape can offer its own d2 to the same sink.
template <typename STORE>
struct RefSink {
    float d2;                   ///< what the walk prunes with: r2, for the whole walk
    int count;                  ///< references so far (R when the walk is over)
    int room;                   ///< references the store takes
    int label;                  ///< the query's label (< 0: skips nothing)
    const int* tri_labels;      ///< three labels per triangle, or null
    STORE store;

    /// before init: the room, the labels (null: none)
    HOST DEVICE void setup(int slots, int query_label, const int* labels) { room = slots; label = query_label; tri_labels = labels; }
    HOST DEVICE void init(const vec3&, float r2) { d2 = r2; count = 0; }
    HOST DEVICE void offer(const Tri& tri, int ref, const vec3& p) {
        if (tri_labels && label >= 0) {
            const int* l = tri_labels + 3 * size_t(ref);
            if (l[0] == label || l[1] == label || l[2] == label) return;
        }
        Pair r;
        if (!point_tri(tri, p, r)) return;
        insert(r.d2, ref);
    }
    /// the candidate (c, ref) of a pair that the labels do not skip
    HOST DEVICE void insert(const float c, int ref) {
        if (!(c <= d2)) return;                                                 // NaN, or beyond r2
        if (count < room) store(count, c, ref);
        count++;
    }
};

/// the 32-byte answer for slot (id, d2) of a list: q, feature and side made again by point_tri / tri_side, after the walk; an unused slot: q = p
template <typename F>
HOST DEVICE inline void slot_record(F tri_at, int id, float d2, const vec3& p, Best& b) {
    b.init(p, d2);
    if (id < 0) return;
    const Tri tri = tri_at(id);
    Pair r;
    point_tri(tri, p, r);
    b.id = id; b.d2 = r.d2; b.q = r.q; b.feature = r.feature; b.side = tri_side(tri, p, r.q);
}

/// is the query answered without looking at a triangle?  (inactive, NaN)  A: Best or NearList
template <typename A>
HOST DEVICE inline bool trivial_query(const vec3& p, float r, A& b) {
    const float r2 = r * r;
    if (r < 0.0f) { b.init(p, -1.0f); return true; }
    b.init(p, r2);
    return !(p.x == p.x) || !(p.y == p.y) || !(p.z == p.z) || !(r2 == r2);
}

/// the definition: every triangle, in order.  tri_at(j) -> Tri
template <typename F, typename A>
HOST DEVICE inline void brute_force(F tri_at, int num_tris, const vec3& p, float r, A& b) {
    if (trivial_query(p, r, b)) return;
    for (int j = 0; j < num_tris; j++) b.offer(tri_at(j), j, p);
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------

// GridConsts, CellRec (here `end` bounds the list), ArrayStack, kMaxLevels: block_walk.h, which names them in this namespace as well
struct Counts { int cells, tris, pruned; };

/// a distance reduced by the absolute margin, not below 0
HOST DEVICE inline float shrink(float d, float eps) { const float m = d - eps; return m > 0.0f ? m : 0.0f; }
/// lower bound (squared, already shrunk) certainly above the best so far?
HOST DEVICE inline bool beyond(float lower2, float best_d2) { return lower2 > best_d2 * 1.0009765625f; }   // 1 + 2^-10
/// face coordinate of an integer corner along one axis
HOST DEVICE inline float face(int corner, float cs, float lo) { return float(corner) * cs + lo; }
/// shrunk distance from p to the interval [lo corner, hi corner] along one axis
HOST DEVICE inline float axis_gap(float p, int lc, int hc, float cs, float lo, float eps) {
    const float a = face(lc, cs, lo) - p, b = p - face(hc, cs, lo);
    return shrink(a > b ? a : b, eps);
}
HOST DEVICE inline float box_lower2(const GridConsts& c, const vec3& p, int lx, int ly, int lz, int hx, int hy, int hz) {
    const float dx = axis_gap(p.x, lx, hx, c.cell_size.x, c.lo.x, c.eps), dy = axis_gap(p.y, ly, hy, c.cell_size.y, c.lo.y, c.eps), dz = axis_gap(p.z, lz, hz, c.cell_size.z, c.lo.z, c.eps);
    return dx * dx + dy * dy + dz * dz;
}

/// the list of one cell.  G: c (GridConsts), word(i), cell(i) -> CellRec, ref(i), tri(id); q...: the query as b.offer takes it
template <typename G, typename A, typename... Q>
HOST DEVICE inline CellRec test_cell(const G& g, uint32_t index, A& b, Counts& n, const Q&... q) {
    const CellRec c = g.cell(index);
    n.cells++;
    if (c.begin >= 0) {
        for (int i = c.begin; i < c.end; i++) {
            const int ref = g.ref(i);
            if (ref < 0) break;
            n.tris++;
            b.offer(g.tri(ref), ref, q...);
        }
    }
    return c;
}

/// one top-level cell: descend its sub-blocks (block_walk.h) while they are not beyond the best so far.  What differs between the queries comes as two
/// callables that capture what the query function already holds: far_block(lx, ly, lz, hx, hy, hz) -- is the block with these integer corners certainly
/// farther than b.d2? -- and home(cell): a cell tested before the rings, not to be tested again
template <typename G, typename S, typename FB, typename H, typename A, typename... Q>
HOST DEVICE inline void visit_top(const G& g, S& st, FB far_block, H home, int tx, int ty, int tz, uint32_t& last_cell, A& b, Counts& n, const Q&... q) {
    const GridConsts& c = g.c;
    auto prune = [&](int x, int y, int z, int s) {
        const bool far = far_block(x, y, z, x + (1 << s), y + (1 << s), z + (1 << s));
        if (far) n.pruned++;
        return far;
    };
    auto leaf = [&](uint32_t ci) {
        if (!home(ci) && ci != last_cell) { last_cell = ci; test_cell(g, ci, b, n, q...); }
        return false;
    };
    if (prune(tx << c.shift, ty << c.shift, tz << c.shift, c.shift)) return;       // before the word is read
    const uint32_t top_w = g.word(uint32_t(tx + c.top.x * (ty + c.top.y * tz)));
    if (!(top_w & 3u)) leaf(top_w >> 2);
    else blocks::descend_top(g, st, top_w, tx, ty, tz, prune, leaf);
}

/// smallest distance from p to the faces of cell c0's box that have grid behind them, and m; m still big: there is none
HOST DEVICE inline float face_room(const GridConsts& c, const CellRec c0, const vec3& p, float m) {    // c0 by value: by reference the kernels are allocated differently
    if (c0.lx > 0)        m = min(m, p.x - face(c0.lx, c.cell_size.x, c.lo.x));
    if (c0.hx < c.dims.x) m = min(m, face(c0.hx, c.cell_size.x, c.lo.x) - p.x);
    if (c0.ly > 0)        m = min(m, p.y - face(c0.ly, c.cell_size.y, c.lo.y));
    if (c0.hy < c.dims.y) m = min(m, face(c0.hy, c.cell_size.y, c.lo.y) - p.y);
    if (c0.lz > 0)        m = min(m, p.z - face(c0.lz, c.cell_size.z, c.lo.z));
    if (c0.hz < c.dims.z) m = min(m, face(c0.hz, c.cell_size.z, c.lo.z) - p.z);
    return m;
}

/// the answer for (p, r) over the grid g: equal, bit for bit, to brute_force over all triangles with the same accumulator (Best, NearList)
template <typename G, typename S, typename A>
HOST DEVICE inline void closest_query(const G& g, S& st, const vec3& p, float r, A& b, Counts& n) {
    const GridConsts& c = g.c;
    n.cells = 0; n.tris = 0; n.pruned = 0;
    if (trivial_query(p, r, b)) return;

    // the voxel of p, p clamped into the grid
    const vec3 f = (p - c.lo) * c.inv;
    float fx = f.x > 0.0f ? f.x : 0.0f, fy = f.y > 0.0f ? f.y : 0.0f, fz = f.z > 0.0f ? f.z : 0.0f;
    fx = fx < float(c.dims.x - 1) ? fx : float(c.dims.x - 1);
    fy = fy < float(c.dims.y - 1) ? fy : float(c.dims.y - 1);
    fz = fz < float(c.dims.z - 1) ? fz : float(c.dims.z - 1);
    const int vx = int(fx), vy = int(fy), vz = int(fz);
    const int tx = vx >> c.shift, ty = vy >> c.shift, tz = vz >> c.shift;

    // its cell
    const uint32_t first_cell = walk::descend(g, g.word(uint32_t(tx + c.top.x * (ty + c.top.y * tz))), vx, vy, vz) >> 2;
    const CellRec c0 = test_cell(g, first_cell, b, n, p);

    // does the ball (p, sqrt(best)) stay inside the cell's box?  faces on the grid boundary have nothing behind them
    {
        const float big = 3.4028234663852886e38f;
        const float m = face_room(c, c0, p, big);
        if (m == big) return;                           // the cell is the whole grid
        const float ms = shrink(m, c.eps);
        if (beyond(ms * ms, b.d2)) return;
    }

    // rings of top-level cells around (tx, ty, tz)
    auto far_block = [&](int lx, int ly, int lz, int hx, int hy, int hz) { return beyond(box_lower2(c, p, lx, ly, lz, hx, hy, hz), b.d2); };
    auto home = [first_cell](uint32_t ci) { return ci == first_cell; };
    uint32_t last_cell = first_cell;
    visit_top(g, st, far_block, home, tx, ty, tz, last_cell, b, n, p);
    for (int k = 1;; k++) {
        // lower bound of ring k: the nearest face of the cube of rings 0 .. k-1 that still has grid behind it
        const float big = 3.4028234663852886e38f;
        float m = big;
        if (tx - k + 1 > 0)   m = min(m, p.x - face((tx - k + 1) << c.shift, c.cell_size.x, c.lo.x));
        if (tx + k < c.top.x) m = min(m, face((tx + k) << c.shift, c.cell_size.x, c.lo.x) - p.x);
        if (ty - k + 1 > 0)   m = min(m, p.y - face((ty - k + 1) << c.shift, c.cell_size.y, c.lo.y));
        if (ty + k < c.top.y) m = min(m, face((ty + k) << c.shift, c.cell_size.y, c.lo.y) - p.y);
        if (tz - k + 1 > 0)   m = min(m, p.z - face((tz - k + 1) << c.shift, c.cell_size.z, c.lo.z));
        if (tz + k < c.top.z) m = min(m, face((tz + k) << c.shift, c.cell_size.z, c.lo.z) - p.z);
        if (m == big) break;                            // the rings have left the grid
        const float ms = shrink(m, c.eps);
        if (beyond(ms * ms, b.d2)) break;

        const int z0 = max(tz - k, 0), z1 = min(tz + k, c.top.z - 1);
        const int y0 = max(ty - k, 0), y1 = min(ty + k, c.top.y - 1);
        for (int z = z0; z <= z1; z++) {
            const bool zface = z == tz - k || z == tz + k;
            for (int y = y0; y <= y1; y++) {
                const bool shell = zface || y == ty - k || y == ty + k;     // the whole row belongs to the ring, else its two ends
                const int xa = shell ? max(tx - k, 0) : tx - k, xb = shell ? min(tx + k, c.top.x - 1) : tx + k;
                const int step = shell ? 1 : 2 * k;
                for (int x = xa; x <= xb; x += step) {
                    if (x < 0 || x >= c.top.x) continue;
                    visit_top(g, st, far_block, home, x, y, z, last_cell, b, n, p);
                }
            }
        }
    }
}

} // namespace closest
} // namespace hagrid

#endif // HAGRID_CLOSEST_H
