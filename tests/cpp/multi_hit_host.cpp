// multi_hit_host -- the multi-hit walk of hagrid_amd/csrc/trav_multi.hip written for the HOST over include/hagrid/{common,prims,grid,
// multi_hit}.h (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: tests/test_multi_hit_cpu.py compares what this writes with
// the fixture tests/golden/multi_hit.npz, tests/test_multi_hit_gpu.py with what the device wrote.  The cell walk is the kernel's
// (include/hagrid/cell_walk.h) over an accessor that checks every index; the list is the HitList the kernel uses.
//
//   multi_hit_host walk   PARAMS ENTRIES CELLS REFS TRIS RAYS OUT    PARAMS: the grid header (host_support.h), i32 k, i32 num_rays;
//                                                                    OUT: num_rays * k Hit records (u = v = 0)
//   multi_hit_host layers PARAMS HITS OUT                            PARAMS: i32 k, f32 clip, f32 opacity, i32 n;  OUT: n pixels (shade_layers of frame.h)
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/cell_walk.h"
#include "hagrid/multi_hit.h"
#include "hagrid/frame.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;

namespace {

// the accessor of cell_walk.h over host arrays, every index checked
typedef HostGrid<kEndUnread> RayGrid;

void walk_ray(const RayGrid& g, const Ray& ray_in, int k, Hit* out) {
    const walk::RaySetup s(g.c, ray_in.org, ray_in.dir, ray_in.tmin, ray_in.tmax);
    HitList<HAGRID_MAX_HITS> list;          // the kernel's list: HAGRID_MAX_HITS slots, k of them in use
    list.init(k, ray_in.tmax);
    // the cell's triangles, each against the ray's own window; done when the list is full and its last entry is not beyond the cell's exit
    auto visit = [&](walk::RefList<RayGrid> refs, float texit, bool) {
        while (!refs.done()) {
            const int ref = refs.next();
            Hit h(-1, ray_in.tmax, 0.0f, 0.0f);
            if (intersect_prim_ray(g.tri(ref), s.ray, ref, h)) list.insert(h.t, ref, 0.0f, 0.0f);
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
        const GridHeader h = p.get_grid_header();
        const int k = p.get<int32_t>(), n = p.get<int32_t>();
        if (k < 1 || k > HAGRID_MAX_HITS) { fprintf(stderr, "walk: k must be 1 .. HAGRID_MAX_HITS\n"); return 2; }
        RayGrid g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.tris = read_file<Tri>(argv[6]);
        const std::vector<Ray> rays = read_file<Ray>(argv[7]);
        if (int(rays.size()) != n) { fprintf(stderr, "walk: the ray file does not hold num_rays records\n"); return 2; }
        std::vector<Hit> out(size_t(n) * size_t(k));
        for (int i = 0; i < n; i++) {
            walk_ray(g, rays[i], k, out.data() + size_t(i) * size_t(k));
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
