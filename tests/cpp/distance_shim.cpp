// The distance lattice from C++: hagrid::distance_lattice of include/hagrid/traverse.h over a grid built through the headers, compiled as plain C++ (-DHOST= -DDEVICE=)
// and linked with libhagrid_amd.so.  The scene is a set of closed boxes, each face split along a diagonal.  Verifies ids, d2 and the 32-byte records of the device
// against closest::brute_force of include/hagrid/closest.h over the voxel centres with r = band, bit for bit, with a band of 1.5 voxels and with a band that makes
// every triangle's voxel box the whole lattice; once more with records alone.  usage: distance_shim [boxes]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hagrid/build.h"
#include "hagrid/mem_manager.h"
#include "hagrid/traverse.h"
#include "hagrid/distance.h"

using namespace hagrid;
namespace hc = hagrid::closest;
namespace hd = hagrid::distance;

static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static float rnd(uint64_t seed, uint64_t i) { return float(mix(seed + (i + 1) * 0x9E3779B97F4A7C15ull) >> 40) * (1.0f / 16777216.0f); }

struct Box { vec3 lo, hi; };
struct Result { float qx, qy, qz, d2; int32_t id, feature; float side; int32_t zero; };

static void add_box(std::vector<Tri>& tris, const Box& b) {
    static const int quad[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 6, 7, 5}};
    for (int f = 0; f < 6; f++)
        for (int h = 0; h < 2; h++) {
            vec3 v[3];
            const int idx[3] = {quad[f][0], quad[f][h + 1], quad[f][h + 2]};
            for (int k = 0; k < 3; k++) v[k] = vec3(idx[k] & 1 ? b.hi.x : b.lo.x, idx[k] & 2 ? b.hi.y : b.lo.y, idx[k] & 4 ? b.hi.z : b.lo.z);
            const vec3 e1 = v[0] - v[1], e2 = v[2] - v[0], n = cross(e1, e2);
            tris.push_back(Tri(v[0], n.x, e1, n.y, e2, n.z));
        }
}

int main(int argc, char** argv) {
    const int nb = argc > 1 ? atoi(argv[1]) : 40;
    std::vector<Tri> host_tris;
    for (int i = 0; i < nb; i++) {
        Box b;
        b.lo = vec3(float(int(rnd(5, 6 * i) * 48)) / 16.0f, float(int(rnd(5, 6 * i + 1) * 48)) / 16.0f, float(int(rnd(5, 6 * i + 2) * 48)) / 16.0f);
        b.hi = b.lo + vec3(float(1 + int(rnd(5, 6 * i + 3) * 15)) / 16.0f, float(1 + int(rnd(5, 6 * i + 4) * 15)) / 16.0f, float(1 + int(rnd(5, 6 * i + 5) * 15)) / 16.0f);
        add_box(host_tris, b);
    }
    const int n = int(host_tris.size());
    MemManager mem(true);
    auto tris = mem.alloc<Tri>(host_tris.size());
    mem.copy<Copy::HST_TO_DEV>(tris, host_tris.data(), host_tris.size());
    Grid grid;
    grid.entries = nullptr; grid.cells = nullptr; grid.ref_ids = nullptr; grid.small_cells = nullptr;
    build_grid(mem, tris, n, grid, 0.12f, 2.4f);
    merge_grid(mem, grid, 0.995f);
    flatten_grid(mem, grid);
    expand_grid(mem, grid, tris, 3);

    const ivec3 lat(37, 19, 13);            // centres ON faces and edges among them: corners lie on multiples of 1/16
    const vec3 origin(-0.125f, -0.0625f, -0.1875f), size(0.125f, 0.25f, 0.375f);
    const int nv = lat.x * lat.y * lat.z;
    int* ids = mem.alloc<int>(nv);
    float* d2 = mem.alloc<float>(nv);
    Result* records = mem.alloc<Result>(nv);
    unsigned long long* work = mem.alloc<unsigned long long>(nv);
    std::vector<int> h_ids(nv);
    std::vector<float> h_d2(nv);
    std::vector<Result> h_rec(nv);
    const Tri* t = host_tris.data();
    auto tri_at = [t](int j) { return t[j]; };

    int bad = 0, bad_rec = 0, found = 0;
    const float bands[2] = {0.5625f, 8.0f};
    for (int k = 0; k < 3; k++) {
        const float band = bands[k % 2];
        mem.one(ids, nv); mem.one(d2, nv); mem.one(records, nv); mem.zero(work, nv);
        if (k < 2) distance_lattice(grid, tris, origin, size, lat, band, work, ids, d2, records);
        else       distance_lattice(grid, tris, origin, size, lat, band, work, nullptr, nullptr, records);
        mem.copy<Copy::DEV_TO_HST>(h_ids.data(), ids, nv);
        mem.copy<Copy::DEV_TO_HST>(h_d2.data(), d2, nv);
        mem.copy<Copy::DEV_TO_HST>(h_rec.data(), records, nv);
        for (int e = 0; e < nv; e++) {
            const vec3 p(crossings::lattice_centre(origin.x, e % lat.x, size.x), crossings::lattice_centre(origin.y, (e / lat.x) % lat.y, size.y),
                         crossings::lattice_centre(origin.z, e / (lat.x * lat.y), size.z));
            hc::Best b;
            hc::brute_force(tri_at, n, p, band, b);
            Result w;
            w.qx = b.q.x; w.qy = b.q.y; w.qz = b.q.z; w.d2 = b.d2; w.id = b.id; w.feature = b.feature; w.side = float(b.side); w.zero = 0;
            bad_rec += memcmp(&w, &h_rec[e], sizeof(Result)) != 0;
            if (k < 2) bad += h_ids[e] != b.id || memcmp(&h_d2[e], &b.d2, 4) != 0;
            else       bad += h_ids[e] != -1 || (as<uint32_t>(h_d2[e]) != 0xffffffffu);          // null outputs are not written
            found += k == 0 && b.id >= 0;
        }
    }
    printf("%d triangles, %d voxels, %d found with the narrow band, %d ids or d2 differ, %d records differ\n", n, nv, found, bad, bad_rec);

    mem.free(records); mem.free(ids); mem.free(d2); mem.free(work);
    mem.free(grid.entries); mem.free(grid.cells); mem.free(grid.ref_ids); mem.free(grid.small_cells); mem.free(tris);
    fflush(stdout);
    return bad == 0 && bad_rec == 0 && found > 0 && found < nv ? 0 : 1;
}
