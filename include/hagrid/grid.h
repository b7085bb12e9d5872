// hagrid/grid.h -- the irregular grid data layout (API mirror of the reference's src/grid.h).
//
//   voxel --lookup_entry--> Entry chain (voxel map) --> Cell (integer AABB on the virtual grid
//   dims << shift, plus a [begin, end) range into ref_ids) --> primitive ids.
//
// Layout contract (bytes, bit positions) is identical to the reference: Entry 4 B with log_dim in
// bits 0-1 and begin in bits 2-31 (grid.h:12-20), Cell 32 B (:23-33), SmallCell 16 B (:36-45).
#ifndef HAGRID_GRID_H
#define HAGRID_GRID_H

#include <vector>
#include "vec.h"
#include "bbox.h"

namespace hagrid {

/// Voxel map word.  log_dim == 0: leaf, begin = cell index.  log_dim = k > 0: inner node whose
/// (2^k)^3 children start at entry index begin, x fastest.
struct Entry {
    enum { LOG_DIM_BITS = 2, BEGIN_BITS = 32 - LOG_DIM_BITS };
    uint32_t log_dim : LOG_DIM_BITS;
    uint32_t begin : BEGIN_BITS;
};

struct Cell {
    ivec3 min; int begin;   ///< lower corner (virtual grid units), first reference
    ivec3 max; int end;     ///< upper corner (exclusive), past-the-end reference
    HOST DEVICE Cell() {}
    HOST DEVICE Cell(const ivec3& lo, int b, const ivec3& hi, int e) : min(lo), begin(b), max(hi), end(e) {}
};

/// Compressed cell: 16-bit corners; its reference list ends with a -1 sentinel, begin = -1 if empty.
struct SmallCell {
    usvec3 min; usvec3 max; int begin;
    HOST DEVICE SmallCell() {}
    HOST DEVICE SmallCell(const usvec3& lo, const usvec3& hi, int b) : min(lo), max(hi), begin(b) {}
};

static_assert(sizeof(Entry) == 4 && sizeof(Cell) == 32 && sizeof(SmallCell) == 16, "grid record layout");

struct Grid {
    Entry* entries;           ///< voxel map (device)
    int* ref_ids;             ///< primitive references (device)
    Cell* cells;              ///< cells (device), nullptr once compressed
    SmallCell* small_cells;   ///< compressed cells (device), nullptr unless compressed
    BBox bbox;                ///< grid bounding box (scene box enlarged by 0.1 %)
    ivec3 dims;               ///< top-level resolution
    int num_cells, num_entries, num_refs;
    int shift;                ///< log2 of the finest subdivision: virtual resolution = dims << shift
    std::vector<int> offsets; ///< cumulative entry count per voxel-map level
};

struct Range {
    int lx, ly, lz, hx, hy, hz;
    HOST DEVICE Range() {}
    HOST DEVICE Range(int lx_, int ly_, int lz_, int hx_, int hy_, int hz_) : lx(lx_), ly(ly_), lz(lz_), hx(hx_), hy(hy_), hz(hz_) {}
    HOST DEVICE int size() const { return (hx - lx + 1) * (hy - ly + 1) * (hz - lz + 1); }
};

HOST DEVICE inline Entry make_entry(uint32_t log_dim, uint32_t begin) {
    Entry e; e.log_dim = log_dim; e.begin = begin; return e;
}

/// A grid coordinate from its float image, total: a value inside int's range gives its truncation, 2^31 and beyond
/// `beyond`, -2^31 and below `below`, NaN `nan`.  The comparison is made in the float domain, so no result depends on a
/// conversion of a value outside int's range ("Admissible scenes").
HOST DEVICE inline int grid_coord(float v, int below, int beyond, int nan) {
    return v >= 2147483648.0f ? beyond : (v > -2147483648.0f ? int(v) : (v != v ? nan : below));
}

/// Inclusive range of grid cells touched by obj_bb, clamped to the grid (truncating casts).  A lower coordinate beyond
/// int's range counts as 2^30 (past every grid), an upper one below it as -2^30; a NaN covers its axis.
HOST DEVICE inline Range compute_range(const ivec3& dims, const BBox& grid_bb, const BBox& obj_bb) {
    const vec3 inv = vec3(dims) / grid_bb.extents();
    const int out = 0x40000000;
    return Range(max(grid_coord((obj_bb.min.x - grid_bb.min.x) * inv.x, 0, out, 0), 0),
                 max(grid_coord((obj_bb.min.y - grid_bb.min.y) * inv.y, 0, out, 0), 0),
                 max(grid_coord((obj_bb.min.z - grid_bb.min.z) * inv.z, 0, out, 0), 0),
                 min(grid_coord((obj_bb.max.x - grid_bb.min.x) * inv.x, -out, out, out), dims.x - 1),
                 min(grid_coord((obj_bb.max.y - grid_bb.min.y) * inv.y, -out, out, out), dims.y - 1),
                 min(grid_coord((obj_bb.max.z - grid_bb.min.z) * inv.z, -out, out, out), dims.z - 1));
}

/// One component of compute_grid_dims: max(1, int(p)) wherever that is defined, INT_MAX from 2^31 on, 1 for NaN.
HOST DEVICE inline int grid_dim(float p) {
    return p >= 2147483648.0f ? 0x7fffffff : (p >= 1.0f ? int(p) : 1);
}

/// Is Cleary's formula defined for this box?  No when density * n / volume is not finite (a flat box, a volume
/// that underflows) or a product extent * ratio is NaN or beyond int's range.
HOST DEVICE inline bool grid_dims_defined(const BBox& bb, int num_prims, float density) {
    const vec3 e = bb.extents();
    const float q = density * num_prims / (e.x * e.y * e.z);
    if (!(q - q == 0.0f)) return false;
    const float ratio = det_cbrtf(q);
    const float px = e.x * ratio, py = e.y * ratio, pz = e.z * ratio, lim = 2147483648.0f;
    return px > -lim && px < lim && py > -lim && py < lim && pz > -lim && pz < lim;
}

/// Resolution for num_prims primitives in bb at the given density (Cleary's formula);
/// the cube root is the deterministic det_cbrtf so host and device agree.  Total: see grid_dim.
HOST DEVICE inline ivec3 compute_grid_dims(const BBox& bb, int num_prims, float density) {
    const vec3 e = bb.extents();
    const float volume = e.x * e.y * e.z;
    const float ratio = det_cbrtf(density * num_prims / volume);
    return ivec3(grid_dim(e.x * ratio), grid_dim(e.y * ratio), grid_dim(e.z * ratio));
}

/// The fraction of a scene's scale below which an axis of its box is widened, the smallest scale, and the share of the added width
/// that goes below the box (widen_scene_box).
constexpr float kWidenFraction = 0.0009765625f;          // 2^-10
constexpr float kWidenMinScale = 9.5367431640625e-07f;   // 2^-20
constexpr float kWidenBelow = 0.381966f;                 // 2 - the golden ratio: no plane k / (dims << shift) of a grid comes near it

/// The box a scene gets where Cleary's formula is undefined for its own (a quad, a ground plane, coincident points):
/// every axis thinner than 2^-10 of the scene's scale is widened to that width.  The scale is the largest extent, or the
/// largest coordinate magnitude if that is larger (so that the new planes are 2^13 ulp apart at least), and 2^-20 at the
/// least (so that the volume, 2^-90 or more, is a normal number).  The added width is NOT split evenly: the resolutions
/// are even, so the centre of the box is a cell boundary at every level, and a flat scene placed there would be
/// referenced from both sides at best and, where the boundary's rounding goes against it, from neither.
HOST DEVICE inline BBox widen_scene_box(const BBox& bb) {
    const vec3 e = bb.extents();
    float s = e.x > e.y ? e.x : e.y; s = e.z > s ? e.z : s;
    const float c[6] = { bb.min.x, bb.min.y, bb.min.z, bb.max.x, bb.max.y, bb.max.z };
    for (int i = 0; i < 6; i++) { const float a = c[i] < 0 ? -c[i] : c[i]; s = a > s ? a : s; }
    s = s > kWidenMinScale ? s : kWidenMinScale;
    const float w = s * kWidenFraction;
    BBox r = bb;
    if (e.x < w) { const float below = (w - e.x) * kWidenBelow; r.min.x = bb.min.x - below; r.max.x = bb.max.x + ((w - e.x) - below); }
    if (e.y < w) { const float below = (w - e.y) * kWidenBelow; r.min.y = bb.min.y - below; r.max.y = bb.max.y + ((w - e.y) - below); }
    if (e.z < w) { const float below = (w - e.z) * kWidenBelow; r.min.z = bb.min.z - below; r.max.z = bb.max.z + ((w - e.z) - below); }
    return r;
}

/// Walks the voxel map from the top-level entry of `voxel` (virtual grid coordinates) down to a leaf
/// and returns the cell index.  dims = top-level resolution.
HOST DEVICE inline uint32_t lookup_entry(const Entry* entries, int shift, const ivec3& dims, const ivec3& voxel) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(entries);
    uint32_t w = words[(voxel.x >> shift) + dims.x * ((voxel.y >> shift) + dims.y * (voxel.z >> shift))];
    int depth = 0;
    while (w & 3u) {
        const int k = int(w & 3u);
        depth += k;
        const int s = shift - depth, m = (1 << k) - 1;
        const int cx = (voxel.x >> s) & m, cy = (voxel.y >> s) & m, cz = (voxel.z >> s) & m;
        w = words[(w >> 2) + cx + ((cy + (cz << k)) << k)];
    }
    return w >> 2;
}

/// Calls f(ref) for every reference of the cell; returns how many words of ref_ids were consumed.
template <typename F>
HOST DEVICE inline int foreach_ref(Cell cell, const int* ref_ids, F f) {
    for (int i = cell.begin; i < cell.end; i++) {
        const int ref = ref_ids[i];
        if (ref < 0) break;
        f(ref);
    }
    return cell.end - cell.begin;
}

template <typename F>
HOST DEVICE inline int foreach_ref(SmallCell cell, const int* ref_ids, F f) {
    if (cell.begin < 0) return 0;
    int i = cell.begin;
    for (;;) {
        const int ref = ref_ids[i++];
        if (ref < 0) break;
        f(ref);
    }
    return i - cell.begin;
}

} // namespace hagrid

#endif // HAGRID_GRID_H
