// crossings_host -- the crossing queries of include/hagrid/crossings.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files:
// tests/test_crossings_cpu.py compares what this writes with the fixture tests/golden/crossings.npz, tests/test_crossings_gpu.py with what the device
// wrote.  Modes: `paged`, the header's crossings_brute_force over all triangles (no grid; a page of 256); `brute`, the same definition without a page --
// every crossing that crosses() of the header accepts into a vector, sorted by (t, id), folded by the header's Accum: linear in the triangles however many a
// ray crosses (hostile rays cross thousands), and a check of the page by something that has none; and `walk`, the header's crossings_walk over a grid in the
// construction format with a page capacity chosen at run time (1 .. 8).
//
//   crossings_host brute|paged PARAMS TRIS ITEMS OUT                      PARAMS: i32 form, i32 n, i32 m, i32 winding, 9 f32 dirs, 3 f32 origin, 3 f32 size, 3 i32 lattice n
//   crossings_host walk  PARAMS ENTRIES CELLS REFS TRIS ITEMS OUT        PARAMS: the same, then the grid header (host_support.h), i32 page
// form 0: ITEMS = n rays (32 bytes), m = 1; form 1: ITEMS = n points (16 bytes: x, y, z, reach); form 2: the lattice, ITEMS is not read.
// OUT: n * m Hit-shaped records, then n int32 `inside` (forms 1 and 2; zeros for form 0), then int64[4] totals (items, cells, tests, flushes) and the int64
// largest excess of a ray's flushes over ceil(count / page) + 1 (<= 0 when the bound holds; the brute force leaves the last four at 0).
#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/crossings.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace hx = hagrid::crossings;

namespace {

// the accessor of cell_walk.h over host arrays, every index checked, and tri(id)
typedef HostGrid<kEndUnread> RayGrid;

struct Query {
    int form, n, m, winding;
    float dirs[9];
    vec3 origin, size;
    ivec3 lat;
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: crossings_host brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    const bool walk = op == "walk";
    const bool paged = op == "paged";
    if (!((walk && argc == 9) || ((op == "brute" || paged) && argc == 6))) { fprintf(stderr, "crossings_host: unknown operation or wrong number of files: %s\n", op.c_str()); return 2; }
    Params p;
    p.bytes = read_file<char>(argv[2]);
    Query q;
    q.form = p.get<int32_t>(); q.n = p.get<int32_t>(); q.m = p.get<int32_t>(); q.winding = p.get<int32_t>();
    for (int i = 0; i < 9; i++) q.dirs[i] = p.get<float>();
    q.origin = p.get3(); q.size = p.get3();
    q.lat.x = p.get<int32_t>(); q.lat.y = p.get<int32_t>(); q.lat.z = p.get<int32_t>();
    if (q.form < 0 || q.form > 2 || q.n < 0 || (q.m != 1 && q.m != 3) || (q.form == 0 && q.m != 1)) { fprintf(stderr, "crossings_host: bad form, n or m\n"); return 2; }

    RayGrid g;
    g.c.set(ivec3(1), 0, vec3(0.0f), vec3(1.0f));          // the brute force reads no grid
    int page = hx::kMaxPage;
    if (walk) {
        const GridHeader h = p.get_grid_header();
        page = p.get<int32_t>();
        if (page < 1 || page > hx::kMaxPage) { fprintf(stderr, "walk: the page capacity must be 1 .. 8\n"); return 2; }
        g.load(h, argv[3], argv[4], argv[5]);
    }
    g.tris = read_file<Tri>(argv[walk ? 6 : 3]);
    const std::vector<Tri>& tris = g.tris;
    const char* items_name = argv[walk ? 7 : 4];
    std::vector<Ray> rays;
    std::vector<float> points;
    if (q.form == 0) {
        rays = read_file<Ray>(items_name);
        if (int(rays.size()) != q.n) { fprintf(stderr, "crossings_host: the ray file does not hold n records\n"); return 2; }
    } else if (q.form == 1) {
        points = read_file<float>(items_name);
        if (points.size() != size_t(q.n) * 4) { fprintf(stderr, "crossings_host: the point file does not hold n records\n"); return 2; }
    } else if (q.n != q.lat.x * q.lat.y * q.lat.z) { fprintf(stderr, "crossings_host: n is not the number of voxels\n"); return 2; }

    std::vector<Hit> records(size_t(q.n) * size_t(q.m));
    std::vector<int32_t> inside(size_t(q.n), 0);
    int64_t totals[5] = {q.n, 0, 0, 0, std::numeric_limits<int64_t>::min()};
    const Tri* t = tris.data();
    std::vector<std::pair<float, uint32_t> > all;
    for (int i = 0; i < q.n; i++) {
        vec3 org; float tmin = 0.0f, tmax; vec3 dir0(0.0f);
        bool active = true;
        if (q.form == 0) { org = rays[i].org; tmin = rays[i].tmin; tmax = rays[i].tmax; dir0 = rays[i].dir; }
        else {
            if (q.form == 1) { org = vec3(points[4 * size_t(i)], points[4 * size_t(i) + 1], points[4 * size_t(i) + 2]); tmax = points[4 * size_t(i) + 3]; }
            else {
                const int x = i % q.lat.x, yz = i / q.lat.x, y = yz % q.lat.y, z = yz / q.lat.y;
                org = vec3(hx::lattice_centre(q.origin.x, x, q.size.x), hx::lattice_centre(q.origin.y, y, q.size.y), hx::lattice_centre(q.origin.z, z, q.size.z));
                tmax = std::numeric_limits<float>::infinity();
            }
            active = hx::point_active(org, tmax);
        }
        int votes = 0;
        for (int d = 0; d < q.m; d++) {
            const vec3 dir = q.form == 0 ? dir0 : vec3(q.dirs[3 * d], q.dirs[3 * d + 1], q.dirs[3 * d + 2]);
            const Ray ray(org, tmin, dir, tmax);
            Hit rec(0, tmax, 0.0f, 0.0f);
            if (active) {
                if (walk) {
                    hx::Counts n;
                    rec = hx::crossings_walk<hx::kMaxPage>(g, ray, page, n);
                    totals[1] += n.cells; totals[2] += n.tests; totals[3] += n.flushes;
                    const int64_t excess = int64_t(n.flushes) - ((int64_t(rec.id) + page - 1) / page + 1);
                    if (excess > totals[4]) totals[4] = excess;
                } else if (paged) {
                    rec = hx::crossings_brute_force<256>([t](int j) { return t[j]; }, int(tris.size()), ray);
                } else {
                    vec3 adir = dir;
                    hx::Accum acc;
                    acc.init(tmax);
                    if (admit_ray(org, adir, tmin, tmax)) {
                        const Ray aray(org, tmin, adir, tmax);
                        all.clear();
                        for (size_t j = 0; j < tris.size(); j++) {
                            float ht; bool entering;
                            if (hx::crosses(tris[j], aray, ht, entering)) all.push_back(std::make_pair(ht, (uint32_t(j) << 1) | (entering ? 1u : 0u)));
                        }
                        std::sort(all.begin(), all.end());          // by t, then by key = by id
                        for (size_t k = 0; k < all.size(); k++) acc.fold(all[k].first, (all[k].second & 1u) != 0);
                    }
                    rec = acc.record();
                }
            }
            votes += hx::vote(rec, q.winding != 0);
            records[size_t(i) * size_t(q.m) + size_t(d)] = rec;
        }
        if (q.form != 0) inside[i] = active ? (2 * votes > q.m ? 1 : 0) : -1;
    }
    if (totals[4] == std::numeric_limits<int64_t>::min()) totals[4] = 0;

    const char* out_name = argv[walk ? 8 : 5];
    FILE* f = fopen(out_name, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out_name); return 2; }
    bool ok = records.empty() || fwrite(records.data(), sizeof(Hit), records.size(), f) == records.size();
    ok = ok && (inside.empty() || fwrite(inside.data(), sizeof(int32_t), inside.size(), f) == inside.size());
    ok = ok && fwrite(totals, sizeof(int64_t), 5, f) == 5;
    fclose(f);
    if (!ok) { fprintf(stderr, "cannot write %s\n", out_name); return 2; }
    return 0;
}
