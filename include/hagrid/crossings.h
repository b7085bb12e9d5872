// hagrid/crossings.h -- crossing queries (hagrid_amd.h: hagrid_count_crossings, hagrid_list_crossings, hagrid_points_inside, hagrid_inside_lattice, hagrid_fill_lattice): ALL the
// surfaces a ray crosses, condensed into one 16-byte record or written out as a sorted list, and from that whether a point lies inside a closed surface.  No counterpart in the
// reference, which answers with the nearest hit only.
//
// Everything is float32 without contraction (-ffp-contract=off), every sum in the order written.  The same code serves the gfx950 kernel
// (hagrid_amd/csrc/crossings.hip) and host programs (tests/cpp/crossings_host.cpp); hagrid_amd/scene.py (ray_tri_pairs, ray_crossings,
// points_inside, lattice_centres) states the same operations in numpy and gives the same bits.
//
// ---- one ray, one triangle ------------------------------------------------------------------------------------------------------
// Ray i CROSSES triangle j exactly when intersect_prim_ray(tri[j], Ray(org, tmin, dir, tmax), j, h) of prims.h accepts the pair with the
// ray's OWN window -- the intersection set of multi_hit.h.  Its value is t = h.t.  Its FACING is the sign bit of det = dot(tri.normal(),
// ray.dir), the expression of prims.h: LEAVING when the bit is clear (the ray runs with the normal), ENTERING when it is set.
// An accepted pair never has det == 0 and never a NaN t:
//   * det == +-0: abs_det = 0, so both window comparisons have a product with 0 on one side: `t >= abs_det * tmin` and `abs_det * tmax > t` read t >= 0
//     and 0 > t (or a comparison with NaN for an infinite bound, which is false).  No t is both: refused.  A NaN det makes abs_det NaN and the
//     comparisons of u, v, w false: refused.
//   * h.t = t * (1 / abs_det) is NaN only if t is (fails `t >= abs_det * tmin`: refused), if abs_det is (above), or as 0 * inf: t = 0 with abs_det = 0
//     (above), or t infinite with abs_det infinite.  t = +inf fails `abs_det * tmax > t`.  That leaves t = -inf with abs_det = +inf, tmin < 0 < tmax: BOTH
//     dot(n, dir) and dot(n, v0 - org) overflowed float32, which takes a direction AND an origin some 1e19 times the scene's size.  prims.h accepts that
//     pair with a NaN t; crosses() below refuses it (t == t), so that no NaN ever enters the order.  No ray of the tests is such a ray.
// So the facing is never the sign of a zero, and (t, id) is a strict total order on the crossings of a ray.
//
// ---- the record -----------------------------------------------------------------------------------------------------------------
// 16 bytes in the layout of Hit, so the shading kernels read it as it is (GRAY / HEAT of hagrid_shade_hits over records: the crossing-count
// picture; DEPTH: the first surface).  With the m crossings of the ray sorted by (t ascending, id ascending) as c_0 .. c_{m-1}:
//   id  int32         count = m
//   t   float32       t_first = t of c_0; the bits of the ray's tmax when m = 0
//   u   float32       length: acc = +0.0f; for p = 0, 1, .. while 2p + 1 < m: acc = acc + (t_{2p+1} - t_{2p}) -- sequential, in that order.  The
//                     length of the ray inside the solid when it starts outside a closed surface; an unpaired last crossing adds nothing.
//   v   int32 bits    winding = #leaving - #entering
// A ray that admit_ray (ray.h) refuses takes no cell step, nor does an inactive ray (tmax = -1: the window is empty); both get count 0,
// t = the bits of tmax, length +0, winding 0.
//
// ---- exact counting without a list of unbounded length --------------------------------------------------------------------------
// A triangle is referenced by several cells, so counting needs exact de-duplication, and no canonical-cell rule gives it (overlap.h: the
// build inserts by the separating-axis test, expanded cell boxes overlap).  What multi_hit.h relies on does: a sorted list of bounded
// capacity that keeps each triangle once -- plus a CURSOR.
//   * A PAGE holds the P smallest crossings that sort STRICTLY AFTER the cursor (t, id).  It is HitList's structure on (t, key) only
//     (key = id * 2 + entering; no u, v): the same duplicate check, the same "the last entry only decreases" argument, every loop over
//     compile-time indices.  P <= PMAX is the same for every ray of a launch.
//   * When the page is full and its last entry is not beyond the exit of the current cell (last_t <= texit, the stop rule of trav_multi.hip) -- or
//     the ray has left the grid --, the page is FLUSHED: its entries are folded, in order, into the ACCUMULATOR (count, winding, first t, the
//     running length and the pending unpaired t, so a pair may straddle two pages), the cursor becomes the page's last entry, the page is
//     emptied, and the list of the CURRENT cell is tested again before the walk steps on.  A page that is not full when the ray leaves the
//     grid is folded and the ray is done.
//   * The cursor strictly increases at every flush, and every flush of a full page folds P distinct crossings: at most floor(m / P) such flushes
//     plus the final one, so the number of flushes is at most ceil(m / P) + 1.
// Why nothing is lost and nothing counted twice.  Counted twice: an entry is folded once, and afterwards it does not sort after the cursor,
// so the page refuses it for good.  Lost: the argument is multi-hit's, per page.  It rests on
//   (a) a cell's reference list holds every triangle that meets the cell's box (closest.h (a));
//   (b) every triangle lies inside the grid box, so a crossing lies on the part of the ray inside the grid;
//   (c) the cells the walk visits cover that part of the ray in order of t, each up to its texit;
// so when the walk is in cell C, every crossing with t <= texit(C) has been offered by C or a cell before it.  A flush happens with
// last_t <= texit(C) (or at the end of the ray, where everything has been offered).  Every crossing between the old cursor and the page's
// last entry has t <= last_t <= texit(C), was therefore offered while the page's last entry was no smaller than now, and so is in the page:
// the page IS the P smallest crossings after the old cursor, of the whole ray.  What the full page refused or dropped sorts after its last
// entry, the new cursor.  Such a crossing D is offered again if its triangle is listed by C or a later cell.  If it is listed only by
// cells before C, it lies in one of them, E, with t_D <= texit(E); it was refused or dropped by a full page whose last entry sorts
// before D, so that page had last_t <= t_D <= texit(E) while the walk was still in E or before: the flush rule fired THERE, and kept firing
// with E's list tested again, until D was folded.  So no crossing is left behind a cell the walk has stepped past.
// The record does not depend on P: crossings_brute_force over ALL triangles defines it, the walk reproduces it.
//
// ---- the list: what a sink sees ---------------------------------------------------------------------------------------------------
// Page::flush, PageVisitor, crossings_walk and crossings_brute_force take a SINK: sink(position, t, key), called once per folded entry, in the order of
// the folds, with position = acc.count before the fold.  Each crossing is folded once and none is lost (above), and a flush folds a sorted page whose every
// entry sorts after the cursor, the last entry of the page before it: so the folds of a ray, over all its flushes, run through c_0 .. c_{m-1} in (t, id)
// order.  So the sink sees the sorted list of the ray, entry p at position p, whatever P is -- and the list is a by-product of the count, not a second walk.
// The default sink (NoSink) does nothing: the record alone, as before.
//   An ENTRY of the list is 8 bytes: float t; int32 key, key = id * 2 + entering, the page's own key (id = key >> 1, entering = key & 1).  The EMPTY entry is
//   t = the bits of the ray's tmax, key = -1.
//   CSR form: offsets is int64[num_rays + 1]; ray i owns the slots [offsets[i], offsets[i+1]) of `entries`, which holds `capacity` of them.  Its ROOM is
//   offsets[i+1] - offsets[i]; the room is 0 when that difference is negative, when offsets[i] < 0 or when offsets[i+1] > capacity: such a ray writes nothing,
//   whatever the offsets say (slot_range below).  Stride form: no offsets, a stride S >= 1; ray i owns [i * S, (i + 1) * S), and capacity >= num_rays * S is
//   the caller's to check (the entry point does, on the host).
//   A ray writes its first min(m, room) entries into the first slots of its range, and the empty entry into every slot that is left when room > m.  Nothing
//   outside its range is written, and the content for room r is a prefix of the content for room r + 1.  With offsets made from the counts of
//   hagrid_count_crossings over the same rays and grid every slot is written exactly once and there is no empty entry.  A ray that is not admissible or not
//   active has m = 0 and takes no cell step: its slots, if any, get empty entries.  Truncation shows in the record: record.id = m > room.
//
// ---- points ---------------------------------------------------------------------------------------------------------------------
// A point record is 16 bytes: x, y, z, reach.  For each of m in {1, 3} directions d the ray is org = p, tmin = 0, dir = d, tmax = reach (+inf is
// allowed and the normal case).  The VOTE of d is count & 1, with HAGRID_INSIDE_WINDING it is winding != 0; inside = 1 when 2 * votes > m,
// else 0; -1 for an INACTIVE point (reach < 0, a NaN reach, a NaN or infinite coordinate), which takes no walk.  The default directions
// (kDefaultDirs) are (3, 1, 2) / sqrt 14, (-2, 4, 3) / sqrt 29, (1, -5, 2) / sqrt 30: none lies along a lattice axis or a face diagonal, so a ray
// through a vertex or an edge of an axis-aligned tessellation is not the common case, and the majority of three makes a single grazing
// ray harmless.  The answer MEANS something for closed surfaces only; a point ON the surface gets whatever the formula gives (tmin = 0
// accepts t = 0).  The lattice form uses the centre of voxel (x, y, z), x fastest: origin + (float(c) + 0.5f) * size per axis, reach +inf.
#ifndef HAGRID_CROSSINGS_H
#define HAGRID_CROSSINGS_H

#include "cell_walk.h"
#include "grid.h"
#include "multi_hit.h"
#include "prims.h"
#include "ray.h"
#include "vec.h"

#if defined(__clang__)
#define HAGRID_NO_UNROLL _Pragma("clang loop unroll(disable) vectorize(disable)")
#else
#define HAGRID_NO_UNROLL
#endif

namespace hagrid {
namespace crossings {

constexpr int kMaxPage = 8;

/// the three default directions, unit length to float32 rounding
constexpr float kDefaultDirs[9] = {0.80178373f, 0.26726124f, 0.53452248f, -0.37139068f, 0.74278135f, 0.55708601f, 0.18257419f, -0.91287093f, 0.36514837f};

/// the pair: does the ray cross the triangle; t and the facing (true: entering, the sign bit of det)
HOST DEVICE inline bool crosses(const Tri& tri, const Ray& ray, float& t, bool& entering) {
    Hit h;
    if (!intersect_prim_ray(tri, ray, 0, h) || !(h.t == h.t)) return false;
    t = h.t;
    entering = (as<uint32_t>(dot(tri.normal(), ray.dir)) & 0x80000000u) != 0;          // det of prims.h: the same expression, the same bits
    return true;
}

/// what a ray has crossed so far, in the order of (t, id)
struct Accum {
    int count, winding;
    float t_first, length, pending;
    HOST DEVICE void init(float tmax) { count = 0; winding = 0; t_first = tmax; length = 0.0f; pending = 0.0f; }
    HOST DEVICE void fold(float t, bool entering) {
        if (count == 0) t_first = t;
        if (count & 1) length = length + (t - pending);
        else pending = t;
        count++;
        winding += entering ? -1 : 1;
    }
    HOST DEVICE Hit record() const { return Hit(count, t_first, length, as<float>(winding)); }
};

/// the sink that keeps nothing: the record alone
struct NoSink {
    HOST DEVICE void operator()(int, float, uint32_t) const {}
};

/// How Page::flush hands its entries to a sink.  Default: from the unrolled loop over the page's slots, the sink's code once per slot -- right for a sink of a few
/// instructions.  A sink with loops and stores of its own (RowSink below) is called from ONE place instead, in a loop that picks slot j by selects: SERIAL.  The
/// entries, their order and the positions are the same; a kernel's sink may decide by a launch-uniform value.
template <typename S>
struct SinkTraits {
    HOST DEVICE static bool serial(const S&) { return false; }
};

/// the slots of ray i in the list forms (above): first slot and room; room 0 for a pair of offsets that is negative, decreasing or beyond the capacity
HOST DEVICE inline void slot_range(const long long* offsets, int stride, long long capacity, int i, long long& first, long long& room) {
    first = 0; room = 0;
    if (offsets) {
        const long long b = offsets[i], e = offsets[size_t(i) + 1];
        if (b >= 0 && e >= b && e <= capacity) { first = b; room = e - b; }
    } else {
        first = (long long)i * stride; room = stride;
    }
}

/// the P smallest crossings after the cursor, sorted, each triangle once.  key = id * 2 + entering (ids fit 31 bits); an empty slot has kEmpty.
template <int PMAX>
struct Page {
    static constexpr uint32_t kEmpty = 0xffffffffu;
    uint32_t key[PMAX];
    float t[PMAX];
    int cap;                                ///< P: slots in use, 1 .. PMAX
    uint32_t last_key; float last_t;        ///< copy of slot cap - 1: the page is full when last_key != kEmpty
    bool has_cursor; uint32_t cur_key; float cur_t;

    HOST DEVICE void init(int p) {
        cap = p; has_cursor = false; cur_key = 0; cur_t = 0.0f;
        clear();
    }
    HOST DEVICE void clear() {
        last_key = kEmpty; last_t = 0.0f;
        HAGRID_UNROLL
        for (int j = 0; j < PMAX; j++) { key[j] = kEmpty; t[j] = 0.0f; }
    }
    HOST DEVICE bool full() const { return last_key != kEmpty; }
    HOST DEVICE bool empty() const { return key[0] == kEmpty; }

    /// (ta, ka) sorts before (tb, kb); keys of different triangles compare like their ids
    HOST DEVICE static bool before(float ta, uint32_t ka, float tb, uint32_t kb) { return ta < tb || (ta == tb && ka < kb); }

    /// an accepted crossing; returns whether the page changed
    HOST DEVICE bool insert(float ht, uint32_t k) {
        if (has_cursor && !before(cur_t, cur_key, ht, k)) return false;             // folded already
        if (last_key != kEmpty && !before(ht, k, last_t, last_key)) return false;   // cannot change a full page
        bool dup = false;
        HAGRID_UNROLL
        for (int j = 0; j < PMAX; j++) dup = dup || key[j] == k;
        if (dup) return false;
        uint32_t ck = k; float ct = ht;
        HAGRID_UNROLL
        for (int j = 0; j < PMAX; j++) {
            const bool take = j < cap && (key[j] == kEmpty || before(ct, ck, t[j], key[j]));
            const uint32_t ok = key[j]; const float ot = t[j];
            key[j] = take ? ck : ok; t[j] = take ? ct : ot;
            ck = take ? ok : ck; ct = take ? ot : ct;
        }
        HAGRID_UNROLL
        for (int j = 0; j < PMAX; j++)
            if (j == cap - 1) { last_key = key[j]; last_t = t[j]; }
        return true;
    }

    /// fold the entries, in order, into the accumulator, each one shown to the sink first (position = the count before the fold); the cursor moves to the
    /// last of them; the page is empty afterwards
    template <typename S = NoSink>
    HOST DEVICE void flush(Accum& acc, const S& sink = S()) {
        if (SinkTraits<S>::serial(sink)) {
            HAGRID_NO_UNROLL
            for (int j = 0; j < cap; j++) {         // (a page is sorted with its empty slots last)
                uint32_t kj = key[0]; float tj = t[0];
                HAGRID_UNROLL
                for (int i = 1; i < PMAX; i++) { kj = i == j ? key[i] : kj; tj = i == j ? t[i] : tj; }
                if (kj == kEmpty) break;
                sink(acc.count, tj, kj);
                acc.fold(tj, (kj & 1u) != 0);
                has_cursor = true; cur_key = kj; cur_t = tj;
            }
            clear();
            return;
        }
        HAGRID_UNROLL
        for (int j = 0; j < PMAX; j++)
            if (j < cap && key[j] != kEmpty) {
                sink(acc.count, t[j], key[j]);
                acc.fold(t[j], (key[j] & 1u) != 0);
                has_cursor = true; cur_key = key[j]; cur_t = t[j];
            }
        clear();
    }
};

/// The definition: every triangle against the ray, a page of PMAX over ALL triangles, again and again until a page comes back not full.  tri_at(j) -> Tri.
/// No grid, no cell, no stop rule: a pass offers everything, so each page is the PMAX smallest crossings after the cursor; the record does not depend on
/// PMAX (a host program takes a large one: a ray with m crossings costs m / PMAX + 1 passes), nor does the list the sink sees.
template <int PMAX = kMaxPage, typename F, typename S = NoSink>
HOST DEVICE inline Hit crossings_brute_force(F tri_at, int num_tris, const Ray& ray_in, const S& sink = S()) {
    vec3 dir = ray_in.dir;
    const bool admitted = admit_ray(ray_in.org, dir, ray_in.tmin, ray_in.tmax);
    const Ray ray(ray_in.org, ray_in.tmin, dir, ray_in.tmax);
    Accum acc;
    acc.init(ray.tmax);
    if (!admitted) return acc.record();
    Page<PMAX> page;
    page.init(PMAX);
    for (;;) {
        for (int j = 0; j < num_tris; j++) {
            float t; bool entering;
            if (crosses(tri_at(j), ray, t, entering)) page.insert(t, (uint32_t(j) << 1) | (entering ? 1u : 0u));
        }
        const bool more = page.full();
        page.flush(acc, sink);
        if (!more) break;
    }
    return acc.record();
}

/// per-ray counts of the walk
struct Counts { int cells, tests, flushes; };

using walk::WalkConsts;
using walk::CellRec;

/// What the crossing walk does with a cell (the visitor of walk::walk_cells): every reference of the list against the ray's own window into the page; when
/// the page is full and its last entry is not beyond the cell's exit (or the ray leaves the grid) the page is flushed and the SAME list tested once more.
template <int PMAX, typename G, typename S = NoSink>
struct PageVisitor {
    const G& g; const Ray& ray; Page<PMAX>& page; Accum& acc; Counts& n; const S& sink;
    HOST DEVICE bool operator()(const walk::RefList<G>& list, float texit, bool outside) {
        n.cells++;
        for (;;) {
            walk::RefList<G> l = list;
            while (!l.done()) {
                const int ref = l.next();
                float t; bool entering;
                n.tests++;
                if (crosses(g.tri(ref), ray, t, entering)) page.insert(t, (uint32_t(ref) << 1) | (entering ? 1u : 0u));
            }
            if (!(page.full() && (page.last_t <= texit || outside))) return false;
            page.flush(acc, sink);    // and this cell's list once more
            n.flushes++;
        }
    }
};

/// The walk of cell_walk.h with pages: the record of one ray over the grid g, equal to crossings_brute_force over all triangles.
/// G: the accessor of cell_walk.h -- c (WalkConsts), small, cell_at(vx, vy, vz) -> CellRec, ref(i) -- and tri(id).  P: the page capacity.  sink: sees the sorted
/// list, entry by entry.  The kernel (crossings.hip) and the host programs tests/cpp/crossings_host.cpp and crossing_lists_host.cpp all run this function.
template <int PMAX, typename G, typename S = NoSink>
HOST DEVICE inline Hit crossings_walk(const G& g, const Ray& ray_in, int P, Counts& n, const S& sink = S()) {
    const walk::RaySetup s(g.c, ray_in.org, ray_in.dir, ray_in.tmin, ray_in.tmax);
    Accum acc;
    acc.init(ray_in.tmax);
    n.cells = 0; n.tests = 0; n.flushes = 0;
    if (!s.enters) return acc.record();

    Page<PMAX> page;
    page.init(P);
    PageVisitor<PMAX, G, S> visit{g, s.ray, page, acc, n, sink};
    walk::walk_cells(g, s, visit);
    if (!page.empty()) { page.flush(acc, sink); n.flushes++; }
    return acc.record();
}

/// an inactive point takes no walk and gets inside = -1: reach < 0 or NaN, a NaN or infinite coordinate
HOST DEVICE inline bool point_active(const vec3& p, float reach) {
    const uint32_t e = 0x7f800000u;
    const bool finite = ((as<uint32_t>(p.x) & e) != e) & ((as<uint32_t>(p.y) & e) != e) & ((as<uint32_t>(p.z) & e) != e);
    return finite && reach >= 0.0f;
}

/// the vote of one ray's record
HOST DEVICE inline int vote(const Hit& rec, bool winding) { return winding ? (as<int32_t>(rec.v) != 0 ? 1 : 0) : (rec.id & 1); }

/// the centre of voxel c of a lattice along one axis
HOST DEVICE inline float lattice_centre(float origin, int c, float size) { return origin + (float(c) + 0.5f) * size; }

// ---- the fill: one ray per voxel ROW (hagrid_fill_lattice) ------------------------------------------------------------------------
// For every requested axis a (mask bit 1 << a), every row of the lattice along a gets ONE ray: org = the centre of the row's voxel 0 (lattice_centre on all three
// axes), dir = +e_a, tmin = -inf, tmax = +inf.  Voxel c of the row lies at tc(c) = lattice_centre(o_a, c, s_a) - lattice_centre(o_a, 0, s_a) (row_tc: one
// subtraction; non-decreasing in c, since every operation is monotone in c).  The STATE BEFORE c is taken over the crossings with t < tc(c), strictly: their
// count & 1, with winding (#leaving - #entering) != 0 -- counting from -inf, so a brick that begins inside the solid is right.  The row's FINAL state is the same
// expression over all its crossings.  A row whose final state is 1 ends inside a surface that should be closed: one of its crossings was miscounted (a ray through
// an edge, a vertex), or the surface is open.  That row ABSTAINS: no vote for any of its voxels.  Otherwise its vote for voxel c is the state before c.
// inside[voxel] = combine(valid, votes): -1 when valid = 0, else 2 * votes > valid; valid = the requested axes whose row through the voxel did not abstain, votes
// = those of them that vote 1.  A row admit_ray refuses has no crossings and votes 0.
// Rows of an axis are numbered with the lower remaining axis fastest (row_of); the records of the row rays are those of crossings_walk over the row ray.
// RowSink is a sink (above): between two crossings the state is constant, so on entry (t, key) it hands the current state to every voxel with tc(c) <= t as ONE
// run, then folds the entry; finish() hands out the rest.  The sink interface is const: cursor and running sums are mutable.

/// where voxel c of a row lies on the row's ray
HOST DEVICE inline float row_tc(float origin, int c, float size) { return lattice_centre(origin, c, size) - lattice_centre(origin, 0, size); }

/// the answer for a voxel from the rows through it
HOST DEVICE inline int combine_votes(int valid, int votes) { return valid == 0 ? -1 : (2 * votes > valid ? 1 : 0); }

/// What a PASS (one requested axis; passes run one after another, numbered 0, 1, 2 in ascending axis order) does with the vote of its row for voxel e.  The
/// workspace byte keeps two bits per pass: bit 2k = the row of pass k did not abstain, bit 2k + 1 = it votes 1.  Pass 0 overwrites the byte (its content before
/// is unspecified), a later pass replaces its own two bits, the LAST pass does not write the byte: it writes inside[e] from the byte and its own vote.  A
/// row that abstains calls this again with valid = 0: its contribution is replaced, nobody else's is touched.  ws may be null when pass 0 is the last.
HOST DEVICE inline unsigned row_bits(unsigned before, int pass, int valid, int vote) {
    return (before & ~(3u << (2 * pass))) | (unsigned((valid ? 1 : 0) | ((valid && vote) ? 2 : 0)) << (2 * pass));
}
HOST DEVICE inline int row_answer(unsigned b) {
    const int valid = int(b & 1u) + int((b >> 2) & 1u) + int((b >> 4) & 1u), votes = int((b >> 1) & 1u) + int((b >> 3) & 1u) + int((b >> 5) & 1u);
    return combine_votes(valid, votes);
}
HOST DEVICE inline void row_put(unsigned char* ws, int* inside, int e, int pass, bool last, int valid, int vote) {
    const unsigned b = row_bits(pass == 0 ? 0u : ws[e], pass, valid, vote);
    if (last) inside[e] = row_answer(b);
    else ws[e] = (unsigned char)b;
}

/// row r of axis a (0, 1, 2) of an nx * ny * nz lattice: the voxel it starts at, the index of that voxel (x fastest), the element stride and the voxels along it
struct Row { int x, y, z, n, base, stride; };          // (an element index fits 31 bits: check_lattice)
HOST DEVICE inline Row row_of(int axis, int r, int nx, int ny, int nz) {
    Row w;
    if (axis == 0)      { w.x = 0; w.y = r % ny; w.z = r / ny; w.n = nx; w.stride = 1; }
    else if (axis == 1) { w.x = r % nx; w.y = 0; w.z = r / nx; w.n = ny; w.stride = nx; }
    else                { w.x = r % nx; w.y = r / nx; w.z = 0; w.n = nz; w.stride = nx * ny; }
    w.base = (w.z * ny + w.y) * nx + w.x;
    return w;
}
/// the rows along axis a
HOST DEVICE inline long long num_rows(int axis, int nx, int ny, int nz) { return axis == 0 ? (long long)ny * nz : axis == 1 ? (long long)nx * nz : (long long)nx * ny; }

/// the ray of a row: from the centre of its voxel 0 along +e_axis, the whole line
HOST DEVICE inline Ray row_ray(const Row& w, int axis, const float* origin, const float* size) {
    const float inf = as<float>(uint32_t(0x7f800000u));
    const vec3 org(lattice_centre(origin[0], w.x, size[0]), lattice_centre(origin[1], w.y, size[1]), lattice_centre(origin[2], w.z, size[2]));
    return Ray(org, -inf, vec3(axis == 0 ? 1.0f : 0.0f, axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f), inf);
}

/// The row as a consumer of the sorted crossings.  E: emit(first, stride, length, state) -- `length` voxels from element `first` on, `stride` apart, get `state`.
template <typename E>
struct RowSink {
    E emit;
    int base, stride;               ///< the row's first element and element stride
    int n; float o, s;              ///< voxels along the row; origin and voxel size of the row's axis
    bool use_winding;
    mutable int c, sum;             ///< the cursor: voxels [0, c) have their state; the crossings folded so far: their number, with winding #leaving - #entering

    HOST DEVICE void init(const Row& w, float origin, float size, bool wind) {
        base = w.base; stride = w.stride; n = w.n; o = origin; s = size; use_winding = wind; c = 0; sum = 0;
    }
    HOST DEVICE int state() const { return use_winding ? (sum != 0 ? 1 : 0) : (sum & 1); }
    HOST DEVICE void operator()(int, float t, uint32_t key) const {
        int e = c;
        HAGRID_NO_UNROLL
        while (e < n && row_tc(o, e, s) <= t) e++;
        if (e > c) { emit(base + c * stride, stride, e - c, state()); c = e; }
        sum += (use_winding && (key & 1u)) ? -1 : 1;
    }
    /// after the walk: the voxels behind the last crossing; state() is then the row's final state
    HOST DEVICE void finish() const {
        if (n > c) { emit(base + c * stride, stride, n - c, state()); c = n; }
    }
};

template <typename E>
struct SinkTraits<RowSink<E>> {
    HOST DEVICE static bool serial(const RowSink<E>&) { return true; }
};

/// The definition of one row: the brute force over ALL triangles with the row as the sink.  Returns the record of the row ray; sink.state() is the final state.
template <int PMAX = kMaxPage, typename F, typename E>
HOST DEVICE inline Hit fill_row(F tri_at, int num_tris, const Ray& row, const RowSink<E>& sink) {
    const Hit rec = crossings_brute_force<PMAX>(tri_at, num_tris, row, sink);
    sink.finish();
    return rec;
}

} // namespace crossings
} // namespace hagrid

// The C++ shim over the entry points (count_crossings, list_crossings, points_inside, inside_lattice, fill_lattice) is with its neighbours in traverse.h.

#endif // HAGRID_CROSSINGS_H
