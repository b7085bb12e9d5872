// The scan-line fill from C++: hagrid::fill_lattice of include/hagrid/traverse.h over a grid built through the headers, compiled as plain C++ (-DHOST= -DDEVICE=)
// and linked with libhagrid_amd.so.  The scene is a set of closed boxes, each face split along a diagonal; the lattice is laid so that no centre lies on a
// face.  Verifies the device's answers and records against fill_row of include/hagrid/crossings.h on the host, all three axes and one axis alone, and the
// answers with the winding rule against the boxes themselves.  usage: fill_lattice_shim [boxes]
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Box { vec3 lo, hi; };

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

// the emitter of the host definition: the votes of one pass into a byte per voxel, as hx::row_put keeps them
struct Emit {
    unsigned char* ws; int* inside; int pass; bool last; int valid;
    void operator()(int first, int stride, int length, int state) const {
        for (int i = 0; i < length; i++) hx::row_put(ws, inside, first + i * stride, pass, last, valid, state);
    }
};

int main(int argc, char** argv) {
    const int nb = argc > 1 ? atoi(argv[1]) : 40;
    std::vector<Tri> host_tris;
    std::vector<Box> boxes;
    for (int i = 0; i < nb; i++) {          // corners on multiples of 1/16 in [0, 4): the lattice below has its centres on odd multiples of 1/32
        Box b;
        b.lo = vec3(float(int(rnd(5, 6 * i) * 48)) / 16.0f, float(int(rnd(5, 6 * i + 1) * 48)) / 16.0f, float(int(rnd(5, 6 * i + 2) * 48)) / 16.0f);
        b.hi = b.lo + vec3(float(1 + int(rnd(5, 6 * i + 3) * 15)) / 16.0f, float(1 + int(rnd(5, 6 * i + 4) * 15)) / 16.0f, float(1 + int(rnd(5, 6 * i + 5) * 15)) / 16.0f);
        boxes.push_back(b);
        add_box(host_tris, b);
    }
    // Two more boxes fix the scene's box at [0, 65/16]^3: its middle planes, which are cell boundaries of the grid, then lie on odd multiples of 1/32, where no face
    // lies.  (Without them a face can lie exactly IN a cell boundary, and there the walk of cell_walk.h -- the ray form's as well -- is known to lose the crossing.)
    const Box first = {vec3(0.0f), vec3(0.0625f)}, last = {vec3(4.0f), vec3(4.0625f)};
    boxes.push_back(first); add_box(host_tris, first);
    boxes.push_back(last); add_box(host_tris, last);
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

    const ivec3 lat(67, 35, 21);
    const float origin[3] = {-0.125f, -0.09375f, -0.125f}, size[3] = {0.0625f, 0.125f, 0.1875f};          // centres on odd multiples of 1/32 on every axis
    const int nv = lat.x * lat.y * lat.z;
    const int rows_all = int(hx::num_rows(0, lat.x, lat.y, lat.z) + hx::num_rows(1, lat.x, lat.y, lat.z) + hx::num_rows(2, lat.x, lat.y, lat.z));
    int* inside = mem.alloc<int>(nv);
    unsigned char* work = mem.alloc<unsigned char>(nv);
    Hit* records = mem.alloc<Hit>(rows_all);
    std::vector<int> h_in(nv), want_in(nv);
    std::vector<unsigned char> want_ws(nv);
    std::vector<Hit> h_rec(rows_all), want_rec;
    const Tri* t = host_tris.data();
    auto tri_at = [t](int j) { return t[j]; };

    int bad = 0, bad_rec = 0, bad_truth = 0, filled = 0;
    const unsigned masks[2] = {7u, 2u};
    for (int k = 0; k < 2; k++) {
        const unsigned axes = masks[k];
        fill_lattice(grid, tris, vec3(origin[0], origin[1], origin[2]), vec3(size[0], size[1], size[2]), lat, inside, k == 0 ? work : nullptr, axes, true, records);
        mem.copy<Copy::DEV_TO_HST>(h_in.data(), inside, nv);
        int pass = 0, last_axis = 0;
        for (int a = 0; a < 3; a++) if (axes & (1u << a)) last_axis = a;
        want_rec.clear();
        for (int a = 0; a < 3; a++) {
            if (!(axes & (1u << a))) continue;
            const int rows = int(hx::num_rows(a, lat.x, lat.y, lat.z));
            for (int r = 0; r < rows; r++) {
                const hx::Row w = hx::row_of(a, r, lat.x, lat.y, lat.z);
                hx::RowSink<Emit> sink;
                sink.emit = Emit{want_ws.data(), want_in.data(), pass, a == last_axis, 1};
                sink.init(w, origin[a], size[a], true);
                want_rec.push_back(hx::fill_row<64>(tri_at, n, hx::row_ray(w, a, origin, size), sink));
                if (sink.state()) { sink.emit.valid = 0; sink.emit(w.base, w.stride, w.n, 0); }
            }
            pass++;
        }
        mem.copy<Copy::DEV_TO_HST>(h_rec.data(), records, want_rec.size());
        for (size_t i = 0; i < want_rec.size(); i++) bad_rec += memcmp(&want_rec[i], &h_rec[i], sizeof(Hit)) != 0;
        for (int i = 0; i < nv; i++) {
            bad += h_in[i] != want_in[i];
            const int c[3] = {i % lat.x, (i / lat.x) % lat.y, i / (lat.x * lat.y)};
            float p[3];
            for (int a = 0; a < 3; a++) p[a] = hx::lattice_centre(origin[a], c[a], size[a]);
            int truth = 0;
            for (const Box& b : boxes) truth |= (p[0] > b.lo.x && p[0] < b.hi.x && p[1] > b.lo.y && p[1] < b.hi.y && p[2] > b.lo.z && p[2] < b.hi.z) ? 1 : 0;
            // boxes may overlap: the winding number is then 2, which is inside as well
            bad_truth += h_in[i] != truth;
            filled += truth;
        }
    }
    printf("%d boxes, %d voxels, %d inside, %d mismatches vs host fill_row, %d records differ, %d mismatches vs the boxes\n", int(boxes.size()), nv, filled / 2, bad, bad_rec, bad_truth);

    mem.free(records); mem.free(inside); mem.free(work);
    mem.free(grid.entries); mem.free(grid.cells); mem.free(grid.ref_ids); mem.free(grid.small_cells); mem.free(tris);
    fflush(stdout);
    return bad == 0 && bad_rec == 0 && bad_truth == 0 && filled > 0 ? 0 : 1;
}
