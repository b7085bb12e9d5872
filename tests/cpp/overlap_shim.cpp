// Box-overlap queries from C++: hagrid::overlap_boxes and hagrid::overlap_lattice of include/hagrid/traverse.h over a grid built through the headers,
// compiled as plain C++ (-DHOST= -DDEVICE=) and linked with libhagrid_amd.so.  Verifies ids and counts against brute_force of include/hagrid/overlap.h
// on the host.  usage: overlap_shim [triangles] [boxes]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hagrid/build.h"
#include "hagrid/mem_manager.h"
#include "hagrid/overlap.h"
#include "hagrid/traverse.h"

using namespace hagrid;
namespace ho = hagrid::overlap;

static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static float rnd(uint64_t seed, uint64_t i) { return float(mix(seed + (i + 1) * 0x9E3779B97F4A7C15ull) >> 40) * (1.0f / 16777216.0f); }

typedef ho::IdList<ho::kMaxIds> List;

// ids and count of one box by the definition against what the device wrote
static int check(const std::vector<Tri>& tris, const ho::Clip& clip, const vec3& lo, const vec3& hi, int first, int k, bool any, const int* ids, int count) {
    List l;
    l.init(k, first);
    const Tri* t = tris.data();
    ho::brute_force([t](int j) { return t[j]; }, int(tris.size()), clip, lo, hi, false, l);
    if (any) {      // some member of S, or none
        if ((ids[0] >= 0) != l.found() || count != (l.found() ? 1 : 0)) return 1;
        vec3 clo = lo, chi = hi;
        return ids[0] >= 0 && !(ids[0] >= first && clip.apply(clo, chi) && ho::meets(tris[ids[0]], clo, chi)) ? 1 : 0;
    }
    int bad = count != l.count() ? 1 : 0;
    for (int j = 0; j < k; j++) bad += ids[j] != l.id[j] ? 1 : 0;
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 20000, nb = argc > 2 ? atoi(argv[2]) : 1000;
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

    // boxes of 1 % to 6 % of the box around random points; every fourth one asks from an id on, every eighth one has an infinite bound
    std::vector<BBox> host_boxes(nb);
    const vec3 lo = grid.bbox.min, ext = grid.bbox.extents();
    ho::Clip clip;
    clip.set(grid.bbox.min, grid.bbox.max);
    for (int i = 0; i < nb; i++) {
        const vec3 c = lo + vec3(rnd(3, 4 * i), rnd(3, 4 * i + 1), rnd(3, 4 * i + 2)) * ext;
        const vec3 h = ext * (0.005f + 0.025f * rnd(3, 4 * i + 3));
        host_boxes[i] = BBox(c - h, c + h);
        if (i % 8 == 5) {                       // every eighth box loses a bound
            const int f = (i / 8) % 6;
            float& bound = f < 3 ? (f == 0 ? host_boxes[i].min.x : f == 1 ? host_boxes[i].min.y : host_boxes[i].min.z)
                                 : (f == 3 ? host_boxes[i].max.x : f == 4 ? host_boxes[i].max.y : host_boxes[i].max.z);
            bound = f < 3 ? -INFINITY : INFINITY;
        }
        host_boxes[i].pad0 = (i % 4 == 3) ? n / 2 : 0;
        host_boxes[i].pad1 = 0;
    }
    BBox* boxes = mem.alloc<BBox>(nb);
    mem.copy<Copy::HST_TO_DEV>(boxes, host_boxes.data(), host_boxes.size());
    const ivec3 lat(9, 7, 5);
    const int nv = lat.x * lat.y * lat.z, most = nb > nv ? nb : nv;
    int* ids = mem.alloc<int>(size_t(most) * ho::kMaxIds);
    int* counts = mem.alloc<int>(most);
    std::vector<int> h_ids(size_t(most) * ho::kMaxIds), h_counts(most);

    int bad = 0, found = 0;
    const int ks[3] = {1, 3, 8};
    for (int q = 0; q < 4; q++) {
        const int k = q < 3 ? ks[q] : 1;
        const bool any = q == 3;
        overlap_boxes(grid, tris, boxes, nb, k, ids, counts, nullptr, any);
        mem.copy<Copy::DEV_TO_HST>(h_ids.data(), ids, size_t(nb) * k);
        mem.copy<Copy::DEV_TO_HST>(h_counts.data(), counts, nb);
        for (int i = 0; i < nb; i++) {
            bad += check(host_tris, clip, host_boxes[i].min, host_boxes[i].max, host_boxes[i].pad0, k, any, h_ids.data() + size_t(i) * k, h_counts[i]);
            found += h_ids[size_t(i) * k] >= 0;
        }
    }
    printf("%d boxes, %d answers with a triangle, %d mismatches vs host brute force\n", nb, found, bad);

    // the lattice form: the boxes are made on the device
    const vec3 size = ext / vec3(float(lat.x), float(lat.y), float(lat.z));
    overlap_lattice(grid, tris, lo, size, lat, 2, ids, counts);
    mem.copy<Copy::DEV_TO_HST>(h_ids.data(), ids, size_t(nv) * 2);
    mem.copy<Copy::DEV_TO_HST>(h_counts.data(), counts, nv);
    int bad_lat = 0, filled = 0;
    for (int i = 0; i < nv; i++) {
        const int x = i % lat.x, y = (i / lat.x) % lat.y, z = i / (lat.x * lat.y);
        const vec3 vlo(ho::lattice_face(lo.x, x, size.x), ho::lattice_face(lo.y, y, size.y), ho::lattice_face(lo.z, z, size.z));
        const vec3 vhi(ho::lattice_face(lo.x, x + 1, size.x), ho::lattice_face(lo.y, y + 1, size.y), ho::lattice_face(lo.z, z + 1, size.z));
        bad_lat += check(host_tris, clip, vlo, vhi, 0, 2, false, h_ids.data() + size_t(i) * 2, h_counts[i]);
        filled += h_counts[i] > 0;
    }
    printf("%d voxels, %d with a triangle, %d mismatches in the lattice form\n", nv, filled, bad_lat);

    mem.free(ids); mem.free(counts); mem.free(boxes);
    mem.free(grid.entries); mem.free(grid.cells); mem.free(grid.ref_ids); mem.free(grid.small_cells); mem.free(tris);
    fflush(stdout);
    return bad == 0 && bad_lat == 0 && found > 0 && filled > 0 ? 0 : 1;
}
