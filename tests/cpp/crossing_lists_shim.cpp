// Crossing lists from C++: hagrid::count_crossings, a scan on the host and hagrid::list_crossings of include/hagrid/traverse.h over a grid built through the
// headers, compiled as plain C++ (-DHOST= -DDEVICE=) and linked with libhagrid_amd.so: count, scan, fill.  Verifies every entry against
// crossings_brute_force of include/hagrid/crossings.h with a sink on the host, then the stride form with four slots per ray.
// usage: crossing_lists_shim [triangles] [rays]
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

struct Slot { float t; int32_t key; };
static bool same(const Slot& a, const Slot& b) { return memcmp(&a, &b, sizeof(Slot)) == 0; }

struct Collect {
    std::vector<Slot>* out;
    void operator()(int, float t, uint32_t key) const { Slot s; s.t = t; s.key = int32_t(key); out->push_back(s); }
};

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
    Hit* records = mem.alloc<Hit>(nr);
    std::vector<Hit> h_rec(nr);

    // count, scan, fill
    count_crossings(grid, tris, rays, records, nr);
    mem.copy<Copy::DEV_TO_HST>(h_rec.data(), records, size_t(nr));
    std::vector<int64_t> h_off(size_t(nr) + 1, 0);
    for (int i = 0; i < nr; i++) h_off[i + 1] = h_off[i] + h_rec[i].id;
    const int64_t total = h_off[nr];
    int64_t* offsets = mem.alloc<int64_t>(h_off.size());
    mem.copy<Copy::HST_TO_DEV>(offsets, h_off.data(), h_off.size());
    Slot* entries = mem.alloc<Slot>(size_t(total) + 1);
    std::vector<Slot> h_ent(size_t(total) + 1);
    memset(h_ent.data(), 0xFF, h_ent.size() * sizeof(Slot));
    mem.copy<Copy::HST_TO_DEV>(entries, h_ent.data(), h_ent.size());
    list_crossings(grid, tris, rays, nr, offsets, 0, entries, total, records);
    mem.copy<Copy::DEV_TO_HST>(h_ent.data(), entries, h_ent.size());
    mem.copy<Copy::DEV_TO_HST>(h_rec.data(), records, size_t(nr));

    const Tri* t = host_tris.data();
    auto tri_at = [t](int j) { return t[j]; };
    std::vector<std::vector<Slot> > want(nr);
    int bad = 0, longest = 0;
    for (int i = 0; i < nr; i++) {
        Collect sink; sink.out = &want[i];
        const Hit rec = hx::crossings_brute_force(tri_at, n, host_rays[i], sink);
        bool ok = memcmp(&rec, &h_rec[i], sizeof(Hit)) == 0 && int64_t(want[i].size()) == h_off[i + 1] - h_off[i];
        for (size_t p = 0; ok && p < want[i].size(); p++) ok = same(want[i][p], h_ent[size_t(h_off[i]) + p]);
        bad += ok ? 0 : 1;
        longest = int(want[i].size()) > longest ? int(want[i].size()) : longest;
    }
    Slot untouched;
    memset(&untouched, 0xFF, sizeof(Slot));
    bad += same(h_ent[size_t(total)], untouched) ? 0 : 1;          // the slot behind the capacity
    printf("%d rays, %lld crossings, the longest list %d, %d mismatches vs host brute force\n", nr, (long long)total, longest, bad);

    // the stride form: four slots per ray, empty entries (tmax, -1) behind a short list
    const int S = 4;
    Slot* fixed = mem.alloc<Slot>(size_t(nr) * S);
    list_crossings(grid, tris, rays, nr, nullptr, S, fixed, int64_t(nr) * S);
    std::vector<Slot> h_fix(size_t(nr) * S);
    mem.copy<Copy::DEV_TO_HST>(h_fix.data(), fixed, h_fix.size());
    int bad_stride = 0;
    for (int i = 0; i < nr; i++)
        for (int p = 0; p < S; p++) {
            Slot w; w.t = host_rays[i].tmax; w.key = -1;
            if (size_t(p) < want[i].size()) w = want[i][p];
            bad_stride += same(w, h_fix[size_t(i) * S + p]) ? 0 : 1;
        }
    printf("%d slots, %d mismatches in the stride form\n", nr * S, bad_stride);

    mem.free(records); mem.free(rays); mem.free(offsets); mem.free(entries); mem.free(fixed);
    mem.free(grid.entries); mem.free(grid.cells); mem.free(grid.ref_ids); mem.free(grid.small_cells); mem.free(tris);
    fflush(stdout);
    return bad == 0 && bad_stride == 0 && total > 0 && longest > S ? 0 : 1;
}
