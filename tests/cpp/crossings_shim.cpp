// Crossing queries from C++: hagrid::count_crossings, hagrid::points_inside and hagrid::inside_lattice of include/hagrid/traverse.h over a grid built through
// the headers, compiled as plain C++ (-DHOST= -DDEVICE=) and linked with libhagrid_amd.so.  Verifies records and inside flags against crossings_brute_force of
// include/hagrid/crossings.h on the host.  usage: crossings_shim [triangles] [rays]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "hagrid/build.h"
#include "hagrid/mem_manager.h"
#include "hagrid/traverse.h"
#include "hagrid/crossings.h"

using namespace hagrid;
namespace hx = hagrid::crossings;

static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static float rnd(uint64_t seed, uint64_t i) { return float(mix(seed + (i + 1) * 0x9E3779B97F4A7C15ull) >> 40) * (1.0f / 16777216.0f); }

static bool same(const Hit& a, const Hit& b) { return memcmp(&a, &b, sizeof(Hit)) == 0; }

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 20000, nr = argc > 2 ? atoi(argv[2]) : 1000;
    std::vector<Tri> host_tris(n);
    const float s = 1.0f / cbrtf(float(n));
    for (int i = 0; i < n; i++) {
        vec3 c(rnd(1, 9 * i), rnd(1, 9 * i + 1), rnd(1, 9 * i + 2));
        vec3 a = (2.0f * vec3(rnd(1, 9 * i + 3), rnd(1, 9 * i + 4), rnd(1, 9 * i + 5)) - vec3(1.0f)) * s;
        vec3 b = (2.0f * vec3(rnd(1, 9 * i + 6), rnd(1, 9 * i + 7), rnd(1, 9 * i + 8)) - vec3(1.0f)) * s;
        vec3 v0 = c, v1 = c + a, v2 = c + b, e1 = v0 - v1, e2 = v2 - v0, nn = cross(e1, e2);
        host_tris[i] = Tri(v0, nn.x, e1, nn.y, e2, nn.z);
    }
    MemManager mem(true);
    auto tris = mem.alloc<Tri>(host_tris.size());
    mem.copy<Copy::HST_TO_DEV>(tris, host_tris.data(), host_tris.size());
    Grid grid;
    grid.entries = nullptr; grid.cells = nullptr; grid.ref_ids = nullptr; grid.small_cells = nullptr;
    build_grid(mem, tris, n, grid, 0.12f, 2.4f);
    merge_grid(mem, grid, 0.995f);
    flatten_grid(mem, grid);
    expand_grid(mem, grid, tris, 3);

    // rays from random points in the box in random directions; every fourth with a finite window
    std::vector<Ray> host_rays(nr);
    const vec3 lo = grid.bbox.min, ext = grid.bbox.extents();
    for (int i = 0; i < nr; i++) {
        const vec3 o = lo + vec3(rnd(3, 6 * i), rnd(3, 6 * i + 1), rnd(3, 6 * i + 2)) * ext;
        const vec3 d = 2.0f * vec3(rnd(3, 6 * i + 3), rnd(3, 6 * i + 4), rnd(3, 6 * i + 5)) - vec3(1.0f);
        host_rays[i] = Ray(o, i % 4 == 3 ? 0.05f : 0.0f, d, i % 4 == 3 ? 0.4f : std::numeric_limits<float>::infinity());
    }
    Ray* rays = mem.alloc<Ray>(nr);
    mem.copy<Copy::HST_TO_DEV>(rays, host_rays.data(), host_rays.size());
    const ivec3 lat(6, 5, 4);
    const int nv = lat.x * lat.y * lat.z, most = nr > nv ? nr : nv;
    Hit* records = mem.alloc<Hit>(size_t(most) * 3);
    int* inside = mem.alloc<int>(most);
    std::vector<Hit> h_rec(size_t(most) * 3);
    std::vector<int> h_in(most);
    const Tri* t = host_tris.data();
    auto tri_at = [t](int j) { return t[j]; };

    count_crossings(grid, tris, rays, records, nr);
    mem.copy<Copy::DEV_TO_HST>(h_rec.data(), records, size_t(nr));
    int bad = 0, crossed = 0, most_crossings = 0;
    for (int i = 0; i < nr; i++) {
        const Hit want = hx::crossings_brute_force(tri_at, n, host_rays[i]);
        bad += same(want, h_rec[i]) ? 0 : 1;
        crossed += h_rec[i].id > 0;
        most_crossings = h_rec[i].id > most_crossings ? h_rec[i].id : most_crossings;
    }
    printf("%d rays, %d with a crossing, at most %d, %d mismatches vs host brute force\n", nr, crossed, most_crossings, bad);

    // the ray origins as points, default directions, per-ray records; then the lattice with one direction of the caller's and the winding rule
    std::vector<float> host_pts(size_t(nr) * 4);
    for (int i = 0; i < nr; i++) {
        host_pts[4 * i] = host_rays[i].org.x; host_pts[4 * i + 1] = host_rays[i].org.y; host_pts[4 * i + 2] = host_rays[i].org.z;
        host_pts[4 * i + 3] = i % 7 == 6 ? -1.0f : std::numeric_limits<float>::infinity();
    }
    float* pts = mem.alloc<float>(host_pts.size());
    mem.copy<Copy::HST_TO_DEV>(pts, host_pts.data(), host_pts.size());
    points_inside(grid, tris, pts, nr, inside, nullptr, 0, records);
    mem.copy<Copy::DEV_TO_HST>(h_rec.data(), records, size_t(nr) * 3);
    mem.copy<Copy::DEV_TO_HST>(h_in.data(), inside, nr);
    int bad_pts = 0;
    for (int i = 0; i < nr; i++) {
        const vec3 p(host_pts[4 * i], host_pts[4 * i + 1], host_pts[4 * i + 2]);
        const float reach = host_pts[4 * i + 3];
        int votes = 0, wrong = 0;
        for (int d = 0; d < 3; d++) {
            Hit want(0, reach, 0.0f, 0.0f);
            if (hx::point_active(p, reach)) want = hx::crossings_brute_force(tri_at, n, Ray(p, 0.0f, vec3(hx::kDefaultDirs[3 * d], hx::kDefaultDirs[3 * d + 1], hx::kDefaultDirs[3 * d + 2]), reach));
            wrong += same(want, h_rec[size_t(i) * 3 + d]) ? 0 : 1;
            votes += hx::vote(want, false);
        }
        const int want_in = hx::point_active(p, reach) ? (2 * votes > 3 ? 1 : 0) : -1;
        bad_pts += (wrong || want_in != h_in[i]) ? 1 : 0;
    }
    printf("%d points, %d mismatches in the point form\n", nr, bad_pts);

    const vec3 size = ext / vec3(float(lat.x), float(lat.y), float(lat.z));
    const float dir[3] = {0.0f, -0.6f, 0.8f};
    inside_lattice(grid, tris, lo, size, lat, inside, dir, 1, nullptr, nullptr, true);
    mem.copy<Copy::DEV_TO_HST>(h_in.data(), inside, nv);
    int bad_lat = 0;
    for (int i = 0; i < nv; i++) {
        const int x = i % lat.x, y = (i / lat.x) % lat.y, z = i / (lat.x * lat.y);
        const vec3 p(hx::lattice_centre(lo.x, x, size.x), hx::lattice_centre(lo.y, y, size.y), hx::lattice_centre(lo.z, z, size.z));
        const Hit want = hx::crossings_brute_force(tri_at, n, Ray(p, 0.0f, vec3(dir[0], dir[1], dir[2]), std::numeric_limits<float>::infinity()));
        bad_lat += hx::vote(want, true) != h_in[i] ? 1 : 0;
    }
    printf("%d voxels, %d mismatches in the lattice form\n", nv, bad_lat);

    mem.free(records); mem.free(inside); mem.free(rays); mem.free(pts);
    mem.free(grid.entries); mem.free(grid.cells); mem.free(grid.ref_ids); mem.free(grid.small_cells); mem.free(tris);
    fflush(stdout);
    return bad == 0 && bad_pts == 0 && bad_lat == 0 && crossed > 0 ? 0 : 1;
}
