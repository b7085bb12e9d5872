// host_support.h -- what the host programs of tests/cpp (closest_host, overlap_host, crossings_host, multi_hit_host) share: whole files in and out, the
// parameter file, and the construction format (entries -> cells | small_cells -> ref_ids) behind an accessor that checks every index.  Test support only;
// tests/_host.py writes the files this reads.
#ifndef HAGRID_TESTS_HOST_SUPPORT_H
#define HAGRID_TESTS_HOST_SUPPORT_H

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/block_walk.h"

namespace host_support {

using namespace hagrid;

template <typename T>
std::vector<T> read_file(const char* name) {
    std::vector<T> v;
    FILE* f = fopen(name, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", name); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(size_t(bytes) / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", name); exit(2); }
    fclose(f);
    return v;
}

template <typename T>
void write_file(const char* name, const std::vector<T>& v) {
    FILE* f = fopen(name, "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) { fprintf(stderr, "cannot write %s\n", name); exit(2); }
    fclose(f);
}

/// what every walk's parameter file holds of the grid (tests/_host.py grid_header): i32 small, 3 i32 top-level dims, i32 shift, 3 f32 bbox min, 3 f32 bbox max
struct GridHeader { int small; ivec3 top; int shift; vec3 lo, hi; };

struct Params {
    std::vector<char> bytes;
    size_t pos = 0;
    template <typename T> T get() {
        T t;
        if (pos + sizeof(T) > bytes.size()) { fprintf(stderr, "parameter file too short\n"); exit(2); }
        memcpy(&t, bytes.data() + pos, sizeof(T));
        pos += sizeof(T);
        return t;
    }
    vec3 get3() { const float x = get<float>(), y = get<float>(), z = get<float>(); return vec3(x, y, z); }
    GridHeader get_grid_header() {
        GridHeader h;
        h.small = get<int32_t>();
        h.top.x = get<int32_t>(); h.top.y = get<int32_t>(); h.top.z = get<int32_t>();
        h.shift = get<int32_t>();
        h.lo = get3(); h.hi = get3();
        if (h.shift < 0 || h.shift > 15) { fprintf(stderr, "walk: bad shift\n"); exit(2); }
        return h;
    }
};

/// The `end` a SmallCell's record gets.  Its list ends with its sentinel: the ray walks (cell_walk.h) never read `end`, the region queries (block_walk.h) bound
/// every list by it.
constexpr int kEndUnread = 0, kEndUnbounded = INT_MAX;

/// The grid arrays with bounds checks: a walk that leaves them is a bug of the walk, not a crash.  Serves both accessor concepts: cell_walk.h's (c, small,
/// cell_at, ref) and block_walk.h's (c, word, cell, ref, tri).  SMALL_END: kEndUnread or kEndUnbounded.
template <int SMALL_END>
struct HostGrid {
    blocks::GridConsts c;           ///< a walk::WalkConsts as well
    bool small = false;
    std::vector<uint32_t> entries;
    std::vector<char> cells;        ///< Cell or SmallCell records
    std::vector<int32_t> refs;
    std::vector<Tri> tris;

    void load(const GridHeader& h, const char* entries_file, const char* cells_file, const char* refs_file) {
        c.set(h.top, h.shift, h.lo, h.hi);
        small = h.small != 0;
        entries = read_file<uint32_t>(entries_file); cells = read_file<char>(cells_file); refs = read_file<int32_t>(refs_file);
    }

    uint32_t word(uint32_t i) const {
        if (i >= entries.size()) { fprintf(stderr, "walk: entry index beyond the voxel map\n"); exit(2); }
        return entries[i];
    }
    walk::CellRec cell(uint32_t i) const {
        if (i >= cells.size() / (small ? sizeof(SmallCell) : sizeof(Cell))) { fprintf(stderr, "walk: cell index beyond the cells\n"); exit(2); }
        walk::CellRec r;
        if (small) {
            const SmallCell& s = reinterpret_cast<const SmallCell*>(cells.data())[i];
            r.lx = s.min.x; r.ly = s.min.y; r.lz = s.min.z; r.hx = s.max.x; r.hy = s.max.y; r.hz = s.max.z; r.begin = s.begin; r.end = SMALL_END;
        } else {
            const Cell& s = reinterpret_cast<const Cell*>(cells.data())[i];
            r.lx = s.min.x; r.ly = s.min.y; r.lz = s.min.z; r.hx = s.max.x; r.hy = s.max.y; r.hz = s.max.z; r.begin = s.begin; r.end = s.end;
        }
        return r;
    }
    walk::CellRec cell_at(int vx, int vy, int vz) const {
        return cell(walk::descend(*this, word(uint32_t(walk::top_index(c, vx, vy, vz))), vx, vy, vz) >> 2);
    }
    int ref(int i) const {
        if (i < 0 || size_t(i) >= refs.size()) { fprintf(stderr, "walk: reference index beyond ref_ids\n"); exit(2); }
        return refs[i];
    }
    const Tri& tri(int id) const {
        if (id < 0 || size_t(id) >= tris.size()) { fprintf(stderr, "walk: triangle id beyond the triangles\n"); exit(2); }
        return tris[id];
    }
};

} // namespace host_support

#endif // HAGRID_TESTS_HOST_SUPPORT_H
