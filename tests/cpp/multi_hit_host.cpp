// multi_hit_host -- the multi-hit walk of hagrid_amd/csrc/trav_multi.hip written for the HOST over include/hagrid/{common,prims,grid,
// multi_hit}.h (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: tests/test_multi_hit_cpu.py compares what this writes with
// the fixture tests/golden/multi_hit.npz, tests/test_multi_hit_gpu.py with what the device wrote.  The cell walk is the one of
// traverse_kernel (trav_plain.hip): same voxel walk, same texit, same next-voxel rule; the list is the HitList the kernel uses.
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

struct HostGrid {
    const Entry* entries;
    const Cell* cells;
    const SmallCell* small_cells;
    const int* refs;
    size_t num_cells, num_refs;
    ivec3 top, dims;        // top-level and virtual resolution
    int shift;
    vec3 lo, hi, cell_size, inv;
};

struct Box { int lx, ly, lz, hx, hy, hz, begin, end; };

Box cell_box(const HostGrid& g, uint32_t index) {
    if (index >= g.num_cells) { fprintf(stderr, "walk: cell index beyond the cells\n"); exit(2); }
    Box b;
    if (g.small_cells) {
        const SmallCell& c = g.small_cells[index];
        b.lx = c.min.x; b.ly = c.min.y; b.lz = c.min.z; b.hx = c.max.x; b.hy = c.max.y; b.hz = c.max.z; b.begin = c.begin; b.end = 0;
    } else {
        const Cell& c = g.cells[index];
        b.lx = c.min.x; b.ly = c.min.y; b.lz = c.min.z; b.hx = c.max.x; b.hy = c.max.y; b.hz = c.max.z; b.begin = c.begin; b.end = c.end;
    }
    return b;
}

void walk_ray(const HostGrid& g, const Tri* tris, const Ray& ray_in, int k, Hit* out) {
    const vec3 org = ray_in.org;
    vec3 dir = ray_in.dir;
    const float tmin = ray_in.tmin, tmax = ray_in.tmax;
    const bool admitted = admit_ray(org, dir, tmin, tmax);          // an inadmissible ray is a miss: no cell walk
    const Ray ray(org, tmin, dir, tmax);          // the window every triangle is tested against
    const vec3 inv_dir(safe_rcp(dir.x), safe_rcp(dir.y), safe_rcp(dir.z));
    const vec3 walk_inv(walk_rcp(dir.x), walk_rcp(dir.y), walk_rcp(dir.z));
    const bool px = dir.x >= 0.0f, py = dir.y >= 0.0f, pz = dir.z >= 0.0f;

    const vec3 ta = (g.lo - org) * inv_dir, tb = (g.hi - org) * inv_dir;
    const vec3 t0 = min(ta, tb), t1 = max(ta, tb);
    const float tstart = detail::fmax2(detail::fmax2(t0.x, detail::fmax2(t0.y, t0.z)), tmin);
    const float tend = detail::fmin2(detail::fmin2(t1.x, detail::fmin2(t1.y, t1.z)), tmax);

    HitList<HAGRID_MAX_HITS> list;          // the kernel's list: HAGRID_MAX_HITS slots, k of them in use
    list.init(k, tmax);

    if (admitted && !(tstart > tend)) {
        const vec3 fv = (tstart * dir + org - g.lo) * g.inv;
        int vx = min(max(int(fv.x), 0), g.dims.x - 1);
        int vy = min(max(int(fv.y), 0), g.dims.y - 1);
        int vz = min(max(int(fv.z), 0), g.dims.z - 1);
        for (;;) {
            const Box c = cell_box(g, lookup_entry(g.entries, g.shift, g.top, ivec3(vx, vy, vz)));

            // exit plane of the cell along the ray
            const int cx = px ? c.hx : c.lx, cy = py ? c.hy : c.ly, cz = pz ? c.hz : c.lz;
            const vec3 tcell = (vec3(float(cx), float(cy), float(cz)) * g.cell_size + g.lo - org) * walk_inv;
            const float texit = detail::fmin2(tcell.x, detail::fmin2(tcell.y, tcell.z));

            // next voxel, never moving backwards
            const vec3 ev = (texit * dir + org - g.lo) * g.inv;
            const int nx = texit == tcell.x ? cx + (px ? 0 : -1) : int(ev.x);
            const int ny = texit == tcell.y ? cy + (py ? 0 : -1) : int(ev.y);
            const int nz = texit == tcell.z ? cz + (pz ? 0 : -1) : int(ev.z);
            vx = px ? max(nx, vx) : min(nx, vx);
            vy = py ? max(ny, vy) : min(ny, vy);
            vz = pz ? max(nz, vz) : min(nz, vz);

            // the cell's triangles, each against the ray's own window
            if (g.small_cells ? c.begin >= 0 : c.begin < c.end) {
                for (int cur = c.begin; g.small_cells || cur < c.end; cur++) {
                    if (size_t(cur) >= g.num_refs) { fprintf(stderr, "walk: reference index beyond ref_ids\n"); exit(2); }
                    const int ref = g.refs[cur];
                    if (ref < 0) break;
                    Hit h(-1, tmax, 0.0f, 0.0f);
                    if (intersect_prim_ray(tris[ref], ray, ref, h)) list.insert(h.t, ref, 0.0f, 0.0f);
                }
            }

            if ((list.full() && list.last_t <= texit) || vx < 0 || vx >= g.dims.x || vy < 0 || vy >= g.dims.y || vz < 0 || vz >= g.dims.z) break;
        }
    }
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
        HostGrid g;
        g.top.x = p.get<int32_t>(); g.top.y = p.get<int32_t>(); g.top.z = p.get<int32_t>();
        g.shift = p.get<int32_t>();
        g.lo = p.get3(); g.hi = p.get3();
        const int n = p.get<int32_t>();
        if (k < 1 || k > HAGRID_MAX_HITS) { fprintf(stderr, "walk: k must be 1 .. HAGRID_MAX_HITS\n"); return 2; }
        const std::vector<uint32_t> entries = read_file<uint32_t>(argv[3]);
        const std::vector<char> cells = read_file<char>(argv[4]);
        const std::vector<int32_t> refs = read_file<int32_t>(argv[5]);
        const std::vector<Tri> tris = read_file<Tri>(argv[6]);
        const std::vector<Ray> rays = read_file<Ray>(argv[7]);
        if (int(rays.size()) != n) { fprintf(stderr, "walk: the ray file does not hold num_rays records\n"); return 2; }
        g.entries = reinterpret_cast<const Entry*>(entries.data());
        g.cells = small ? nullptr : reinterpret_cast<const Cell*>(cells.data());
        g.small_cells = small ? reinterpret_cast<const SmallCell*>(cells.data()) : nullptr;
        g.num_cells = cells.size() / (small ? sizeof(SmallCell) : sizeof(Cell));
        g.refs = refs.data(); g.num_refs = refs.size();
        // setup_traversal's constants, as hagrid_amd/csrc/traverse.hip make_args computes them
        const vec3 ext = g.hi - g.lo;
        g.dims = g.top << g.shift;
        g.inv = vec3(g.dims) / ext;
        g.cell_size = ext / vec3(g.dims);
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
