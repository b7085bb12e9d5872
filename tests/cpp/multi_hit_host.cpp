// multi_hit_host -- the multi-hit walk of hagrid_amd/csrc/trav_multi.hip written for the HOST over include/hagrid/{common,prims,grid,
// multi_hit}.h (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: tests/test_multi_hit_cpu.py compares what this writes with
// the fixture tests/golden/multi_hit.npz, tests/test_multi_hit_gpu.py with what the device wrote.  The cell walk is the kernel's
// (include/hagrid/cell_walk.h) over an accessor that checks every index; the list is the HitList the kernel uses.
//
//   multi_hit_host walk   PARAMS ENTRIES CELLS REFS TRIS RAYS OUT    PARAMS: i32 small, i32 k, 3 i32 top-level dims, i32 shift, 3 f32 bbox min,
//                                                                    3 f32 bbox max, i32 num_rays;  OUT: num_rays * k Hit records (u = v = 0)
//   multi_hit_host layers PARAMS HITS OUT                            PARAMS: i32 k, f32 clip, f32 opacity, i32 n;  OUT: n pixels (shade_layers of frame.h)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/cell_walk.h"
#include "hagrid/multi_hit.h"
#include "hagrid/frame.h"

using namespace hagrid;

namespace {

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
};

// the accessor of cell_walk.h over host arrays, cell and reference indices checked
struct HostGrid {
    walk::WalkConsts c;
    bool small;
    const Entry* entries;
    const Cell* cells;
    const SmallCell* small_cells;
    const int* refs;
    size_t num_cells, num_refs;

    walk::CellRec cell_at(int vx, int vy, int vz) const {
        const uint32_t index = lookup_entry(entries, c.shift, c.top, ivec3(vx, vy, vz));
        if (index >= num_cells) { fprintf(stderr, "walk: cell index beyond the cells\n"); exit(2); }
        walk::CellRec b;
        if (small) {
            const SmallCell& s = small_cells[index];
            b.lx = s.min.x; b.ly = s.min.y; b.lz = s.min.z; b.hx = s.max.x; b.hy = s.max.y; b.hz = s.max.z; b.begin = s.begin; b.end = 0;
        } else {
            const Cell& s = cells[index];
            b.lx = s.min.x; b.ly = s.min.y; b.lz = s.min.z; b.hx = s.max.x; b.hy = s.max.y; b.hz = s.max.z; b.begin = s.begin; b.end = s.end;
        }
        return b;
    }
    int ref(int i) const {
        if (i < 0 || size_t(i) >= num_refs) { fprintf(stderr, "walk: reference index beyond ref_ids\n"); exit(2); }
        return refs[i];
    }
};

void walk_ray(const HostGrid& g, const Tri* tris, const Ray& ray_in, int k, Hit* out) {
    const walk::RaySetup s(g.c, ray_in.org, ray_in.dir, ray_in.tmin, ray_in.tmax);
    HitList<HAGRID_MAX_HITS> list;          // the kernel's list: HAGRID_MAX_HITS slots, k of them in use
    list.init(k, ray_in.tmax);
    // the cell's triangles, each against the ray's own window; done when the list is full and its last entry is not beyond the cell's exit
    auto visit = [&](walk::RefList<HostGrid> refs, float texit, bool) {
        while (!refs.done()) {
            const int ref = refs.next();
            Hit h(-1, ray_in.tmax, 0.0f, 0.0f);
            if (intersect_prim_ray(tris[ref], s.ray, ref, h)) list.insert(h.t, ref, 0.0f, 0.0f);
        }
        return list.full() && list.last_t <= texit;
    };
    if (s.enters) walk::walk_cells(g, s, visit);
    list.store(out);
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: multi_hit_host walk|layers PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "walk" && argc == 9) {
        const int small = p.get<int32_t>(), k = p.get<int32_t>();
        ivec3 top;
        top.x = p.get<int32_t>(); top.y = p.get<int32_t>(); top.z = p.get<int32_t>();
        const int shift = p.get<int32_t>();
        const vec3 lo = p.get3(), hi = p.get3();
        const int n = p.get<int32_t>();
        if (k < 1 || k > HAGRID_MAX_HITS) { fprintf(stderr, "walk: k must be 1 .. HAGRID_MAX_HITS\n"); return 2; }
        const std::vector<uint32_t> entries = read_file<uint32_t>(argv[3]);
        const std::vector<char> cells = read_file<char>(argv[4]);
        const std::vector<int32_t> refs = read_file<int32_t>(argv[5]);
        const std::vector<Tri> tris = read_file<Tri>(argv[6]);
        const std::vector<Ray> rays = read_file<Ray>(argv[7]);
        if (int(rays.size()) != n) { fprintf(stderr, "walk: the ray file does not hold num_rays records\n"); return 2; }
        HostGrid g;
        g.c.set(top << shift, shift, lo, hi);
        g.small = small != 0;
        g.entries = reinterpret_cast<const Entry*>(entries.data());
        g.cells = small ? nullptr : reinterpret_cast<const Cell*>(cells.data());
        g.small_cells = small ? reinterpret_cast<const SmallCell*>(cells.data()) : nullptr;
        g.num_cells = cells.size() / (small ? sizeof(SmallCell) : sizeof(Cell));
        g.refs = refs.data(); g.num_refs = refs.size();
        std::vector<Hit> out(size_t(n) * size_t(k));
        for (int i = 0; i < n; i++) {
            walk_ray(g, tris.data(), rays[i], k, out.data() + size_t(i) * size_t(k));
        }
        write_file(argv[8], out);
    } else if (op == "layers" && argc == 5) {
        const int k = p.get<int32_t>();
        const float clip = p.get<float>(), opacity = p.get<float>();
        const int n = p.get<int32_t>();
        const std::vector<Hit> hits = read_file<Hit>(argv[3]);
        if (k < 1 || hits.size() != size_t(n) * size_t(k)) { fprintf(stderr, "layers: the hit file does not hold n * k records\n"); return 2; }
        std::vector<uint32_t> out((size_t(n)));
        for (int i = 0; i < n; i++) out[i] = frame::shade_layers(hits.data() + size_t(i) * size_t(k), k, clip, opacity);
        write_file(argv[4], out);
    } else {
        fprintf(stderr, "multi_hit_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
