// filtered_host -- the filtered multi-hit walk of hagrid_amd/csrc/trav_multi.hip (hagrid_traverse_grid_filtered) written for the HOST over
// include/hagrid/{common,prims,grid,cell_walk,multi_hit,ray_filter}.h (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files:
// tests/test_filtered_cpu.py compares what this writes with scene.filtered_hits, tests/test_filtered_gpu.py with what the device wrote.  The cell walk is
// the kernel's over an accessor that checks every index, the list is the kernel's HitList, the filter the kernel's RayFilter -- in the kernel's order: the
// skipped triangle in front of the triangle test, the masks for an accepted intersection, a ray with mask 0 does not walk, any-hit ends behind the first cell that left an entry.
//
//   filtered_host walk PARAMS ENTRIES CELLS REFS TRIS RAYS FILTERS MASKS OUT
//       PARAMS: the grid header (host_support.h), i32 k, i32 num_rays, i32 any_hit, i32 has_filters, i32 has_masks
//       FILTERS: num_rays records (u32 mask, i32 skip), read when has_filters;  MASKS: u32 per triangle, read when has_masks
//       OUT: num_rays * k Hit records (u = v = 0)
#include <string>
#include <vector>

#include "hagrid_amd.h"          // HAGRID_MAX_HITS
#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/cell_walk.h"
#include "hagrid/multi_hit.h"
#include "hagrid/ray_filter.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;

namespace {

typedef HostGrid<kEndUnread> RayGrid;

// the triangle masks with the index checked: the kernel trusts the caller with the array's length, the test does not
struct Masks {
    std::vector<uint32_t> m;
    bool given = false;
    bool admits(const RayFilter& f, int ref) const {
        if (!given) return f.admits(nullptr, ref);
        if (ref < 0 || size_t(ref) >= m.size()) { fprintf(stderr, "walk: triangle id beyond the triangle masks\n"); exit(2); }
        return f.admits(m.data(), ref);
    }
};

void walk_ray(const RayGrid& g, const Ray& ray_in, const RayFilter& f, const Masks& masks, int k, bool any_hit, Hit* out) {
    const walk::RaySetup s(g.c, ray_in.org, ray_in.dir, ray_in.tmin, ray_in.tmax);
    HitList<HAGRID_MAX_HITS> list;
    list.init(k, ray_in.tmax);
    auto visit = [&](walk::RefList<RayGrid> refs, float texit, bool) {
        while (!refs.done()) {
            const int ref = refs.next();
            Hit h(-1, ray_in.tmax, 0.0f, 0.0f);
            if (!f.skips(ref) && intersect_prim_ray(g.tri(ref), s.ray, ref, h) && masks.admits(f, ref)) list.insert(h.t, ref, 0.0f, 0.0f);
        }
        return list.full() && (any_hit || list.last_t <= texit);
    };
    if (s.enters && f.walks()) walk::walk_cells(g, s, visit);
    list.store(out);
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 11 || std::string(argv[1]) != "walk") { fprintf(stderr, "usage: filtered_host walk PARAMS ENTRIES CELLS REFS TRIS RAYS FILTERS MASKS OUT\n"); return 2; }
    Params p;
    p.bytes = read_file<char>(argv[2]);
    const GridHeader h = p.get_grid_header();
    const int k = p.get<int32_t>(), n = p.get<int32_t>(), any_hit = p.get<int32_t>(), has_filters = p.get<int32_t>(), has_masks = p.get<int32_t>();
    if (k < 1 || k > HAGRID_MAX_HITS) { fprintf(stderr, "walk: k must be 1 .. HAGRID_MAX_HITS\n"); return 2; }
    if (any_hit && k != 1) { fprintf(stderr, "walk: any-hit needs k = 1\n"); return 2; }
    RayGrid g;
    g.load(h, argv[3], argv[4], argv[5]);
    g.tris = read_file<Tri>(argv[6]);
    const std::vector<Ray> rays = read_file<Ray>(argv[7]);
    if (int(rays.size()) != n) { fprintf(stderr, "walk: the ray file does not hold num_rays records\n"); return 2; }
    std::vector<RayFilter> filters;
    if (has_filters) {
        filters = read_file<RayFilter>(argv[8]);
        if (int(filters.size()) != n) { fprintf(stderr, "walk: the filter file does not hold num_rays records\n"); return 2; }
    }
    Masks masks;
    masks.given = has_masks != 0;
    if (masks.given) masks.m = read_file<uint32_t>(argv[9]);
    std::vector<Hit> out(size_t(n) * size_t(k));
    for (int i = 0; i < n; i++)
        walk_ray(g, rays[i], RayFilter::of(has_filters ? filters.data() : nullptr, size_t(i)), masks, k, any_hit != 0, out.data() + size_t(i) * size_t(k));
    write_file(argv[10], out);
    return 0;
}
