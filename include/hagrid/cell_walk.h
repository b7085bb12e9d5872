// hagrid/cell_walk.h -- the ray walk over the construction format (entries -> cells | small_cells -> ref_ids), written once: the ray set-up, the step from
// a cell to the next voxel, the voxel-map descent and the loop around them.  Float32 without contraction (-ffp-contract=off), every operation in the order
// written; the CPU oracle (oracle/hagrid_oracle.c) states the same operations independently and is the judge.
//
// Who runs it: the nearest-hit kernel v2 and the statistics kernel (hagrid_amd/csrc/trav_plain.hip), multi-hit (trav_multi.hip), crossings (crossings.hip) --
// each over an accessor with device loads and a visitor that says what a ray keeps and when it is done -- and the host programs of tests/cpp (multi_hit_host,
// crossings_host) over accessors whose loads are plain array reads with bounds checks.  The traversal-image kernels (trav_kernels.h) walk another format.
//
// The accessor G:  c (WalkConsts), small (SmallCell lists end with their sentinel; may be a compile-time constant), cell_at(vx, vy, vz) -> the CellRec of a
//                  voxel inside the grid, ref(i) -> reference.  ref(0) is read for an empty cell and dropped.  How cell_at finds the cell is the accessor's
//                  business: the device accessors keep the top-level word while the ray stays in one top-level cell and go down with descend() below.
// The visitor V:   visit(list, texit, outside) -> the ray is done.  list is a RefList<G> over the current cell, texit the parameter at which the ray leaves
//                  that cell, outside whether the next voxel lies beyond the grid (the driver ends the ray then, whatever the visitor returns).
#ifndef HAGRID_CELL_WALK_H
#define HAGRID_CELL_WALK_H

#include "prims.h"
#include "ray.h"
#include "vec.h"

namespace hagrid {
namespace walk {

/// float -> int as the gfx950 conversion does it (v_cvt_i32_f32: truncation, saturating, NaN -> 0).  On the host a plain cast of a value that does not fit
/// is undefined (x86 gives INT_MIN), and the walk does convert such values: the voxel coordinate of an exit point far outside the grid.  Written out, so that
/// the host walk and the kernel take the same steps on every ray.
HOST DEVICE inline int f2i(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return int(f);
#else
    if (!(f == f)) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return int(f);
#endif
}

/// a cell of either format.  end: past-the-end reference.  A SmallCell's list ends with its sentinel and the ray walk does not read its `end`; closest.h and
/// overlap.h bound every list by `end`, so their loaders give a SmallCell INT_MAX there.  A SmallCell with begin < 0 is empty.
struct CellRec { int lx, ly, lz, hx, hy, hz, begin, end; };

/// setup_traversal's constants (hagrid_amd/csrc/traverse.hip make_args computes the same), from the VIRTUAL resolution dims = top-level resolution << shift.
/// blocks::GridConsts (block_walk.h) is this struct set from the top-level resolution, plus the margin of the region queries, which no ray walk reads.
struct WalkConsts {
    ivec3 top, dims;
    int shift;
    vec3 lo, hi, cell_size, inv;
    HOST DEVICE void set(const ivec3& dims_, int shift_, const vec3& lo_, const vec3& hi_) {
        dims = dims_; shift = shift_; lo = lo_; hi = hi_;
        top = ivec3(dims.x >> shift, dims.y >> shift, dims.z >> shift);
        const vec3 ext = hi - lo;
        inv = vec3(dims) / ext;
        cell_size = ext / vec3(dims);
    }
};

/// What a ray computes before its first cell.
struct RaySetup {
    Ray ray;                ///< dir as admit_ray leaves it (every zero +0): the window every triangle is tested against
    vec3 walk_inv;          ///< for the cell walk: no exit through planes of an axis the ray does not move along
    bool admitted;          ///< an inadmissible ray is a miss: no cell walk
    bool px, py, pz;
    float tstart, tend;
    bool enters;            ///< admitted and the window meets the grid box
    int vx, vy, vz;         ///< the first voxel, clamped into the grid (0 when the ray does not enter)

    HOST DEVICE RaySetup(const WalkConsts& k, const vec3& org, const vec3& dir_in, float tmin, float tmax) {
        vec3 dir = dir_in;
        admitted = admit_ray(org, dir, tmin, tmax);
        ray = Ray(org, tmin, dir, tmax);
        const vec3 inv_dir(safe_rcp(dir.x), safe_rcp(dir.y), safe_rcp(dir.z));
        walk_inv = vec3(walk_rcp(dir.x), walk_rcp(dir.y), walk_rcp(dir.z));
        px = dir.x >= 0.0f; py = dir.y >= 0.0f; pz = dir.z >= 0.0f;
        // slab test against the grid box
        const vec3 ta = (k.lo - org) * inv_dir, tb = (k.hi - org) * inv_dir;
        const vec3 t0 = min(ta, tb), t1 = max(ta, tb);
        tstart = detail::fmax2(detail::fmax2(t0.x, detail::fmax2(t0.y, t0.z)), tmin);
        tend = detail::fmin2(detail::fmin2(t1.x, detail::fmin2(t1.y, t1.z)), tmax);
        enters = admitted && !(tstart > tend);
        vx = 0; vy = 0; vz = 0;
        if (enters) {
            const vec3 fv = (tstart * dir + org - k.lo) * k.inv;
            vx = min(max(f2i(fv.x), 0), k.dims.x - 1);
            vy = min(max(f2i(fv.y), 0), k.dims.y - 1);
            vz = min(max(f2i(fv.z), 0), k.dims.z - 1);
        }
    }
};

struct Step { float texit; bool outside; };

/// From the cell c, which holds the voxel (vx, vy, vz), to the next voxel along the ray: the cell's exit plane per axis, texit, the voxel behind it -- the
/// plane's own coordinate on the axis the ray leaves through, the converted exit point on the others --, never moving backwards; outside: beyond the grid.
HOST DEVICE inline Step step(const WalkConsts& k, const RaySetup& s, const CellRec& c, int& vx, int& vy, int& vz) {
    const int cx = s.px ? c.hx : c.lx, cy = s.py ? c.hy : c.ly, cz = s.pz ? c.hz : c.lz;
    const vec3 tcell = (vec3(float(cx), float(cy), float(cz)) * k.cell_size + k.lo - s.ray.org) * s.walk_inv;
    Step r;
    r.texit = detail::fmin2(tcell.x, detail::fmin2(tcell.y, tcell.z));
    const vec3 ev = (r.texit * s.ray.dir + s.ray.org - k.lo) * k.inv;
    const int nx = r.texit == tcell.x ? cx + (s.px ? 0 : -1) : f2i(ev.x);
    const int ny = r.texit == tcell.y ? cy + (s.py ? 0 : -1) : f2i(ev.y);
    const int nz = r.texit == tcell.z ? cz + (s.pz ? 0 : -1) : f2i(ev.z);
    vx = s.px ? max(nx, vx) : min(nx, vx);
    vy = s.py ? max(ny, vy) : min(ny, vy);
    vz = s.pz ? max(nz, vz) : min(nz, vz);
    // v < 0 || v >= dims as one unsigned comparison per axis (dims > 0)
    r.outside = (uint32_t(vx) >= uint32_t(k.dims.x)) | (uint32_t(vy) >= uint32_t(k.dims.y)) | (uint32_t(vz) >= uint32_t(k.dims.z));
    return r;
}

/// index of the top-level entry of a voxel (a device accessor may compute the same number in another way)
HOST DEVICE inline int top_index(const WalkConsts& k, int x, int y, int z) { return (x >> k.shift) + k.top.x * ((y >> k.shift) + k.top.y * (z >> k.shift)); }

/// the sub-levels of the voxel map over g.word(i): from the top-level word w of the voxel (x, y, z) to its leaf word (cell index << 2)
template <typename G>
HOST DEVICE inline uint32_t descend(const G& g, uint32_t w, int x, int y, int z) {
    int depth = 0;
    while (w & 3u) {
        const int l = int(w & 3u);
        depth += l;
        const int s = g.c.shift - depth, m = (1 << l) - 1;
        w = g.word((w >> 2) + ((x >> s) & m) + ((((y >> s) & m) + (((z >> s) & m) << l)) << l));
    }
    return w;
}

/// The references of one cell, one reference ahead: the load of the next one is issued before the caller tests the current one.
/// A copy starts again where the original stands (crossings tests a cell's list several times).
template <typename G>
struct RefList {
    const G& g;
    int cur, end, ref;
    HOST DEVICE RefList(const G& g_, const CellRec& c) : g(g_), end(c.end) {
        const bool nonempty = g.small ? c.begin >= 0 : c.begin < c.end;
        cur = nonempty ? c.begin : 0;           // loaded whether or not it is used: nothing waits for the comparison
        ref = g.ref(cur);
        cur++;
        if (!nonempty) ref = -1;
    }
    HOST DEVICE bool done() const { return ref < 0; }
    /// the current reference; the list moves on
    HOST DEVICE int next() {
        const int r = ref;
        ref = g.small ? g.ref(cur) : (cur < end ? g.ref(cur) : -1);
        cur++;
        return r;
    }
};

/// The walk of one ray that enters the grid (s.enters).  The first reference of the current cell and the NEXT cell's look-up are issued before the visitor
/// tests the current cell's triangles: they do not depend on the tests, and if the ray ends in this cell they are dropped.  (On the host that order is
/// harmless.)  A voxel outside the grid has no cell and nothing is looked up for it: the ray ends behind this cell.
template <typename G, typename V>
HOST DEVICE inline void walk_cells(const G& g, const RaySetup& s, V& visit) {
    int vx = s.vx, vy = s.vy, vz = s.vz;
    CellRec c = g.cell_at(vx, vy, vz);
    for (;;) {
        const Step st = step(g.c, s, c, vx, vy, vz);
        const RefList<G> list(g, c);
        CellRec nc = c;
        if (!st.outside) nc = g.cell_at(vx, vy, vz);
        if (visit(list, st.texit, st.outside) || st.outside) break;
        c = nc;
    }
}

} // namespace walk
} // namespace hagrid

#endif // HAGRID_CELL_WALK_H
