// fill_lattice_host -- hagrid_fill_lattice on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: what the passes of the gfx950 kernel
// (hagrid_amd/csrc/crossings.hip, the row form) do, with the header's functions: row_of and row_ray for the row, RowSink as the sink of fill_row (mode `brute`:
// no grid, a page of 256) or of crossings_walk (mode `walk`: a grid in the construction format, a page capacity chosen at run time, 1 .. 8), row_put for every
// voxel, once more with valid = 0 along a row that ends inside.  tests/test_fill_lattice_cpu.py compares what this writes with tests/golden/fill_lattice.npz,
// tests/test_fill_lattice_gpu.py with what the device wrote.
//
//   fill_lattice_host brute PARAMS TRIS OUT                      PARAMS: 3 f32 origin, 3 f32 size, 3 i32 n, i32 axes, i32 winding
//   fill_lattice_host walk  PARAMS ENTRIES CELLS REFS TRIS OUT   PARAMS: the same, then the grid header (host_support.h), i32 page
// OUT: int32 inside per voxel (x fastest), then one Hit-shaped record per row (axis after axis, the lower remaining axis fastest), then one byte per row (1: it
// abstained), padded to a multiple of 8 bytes, then int64[5] totals (rows, cells, tests, flushes, rows that abstained; the brute force leaves cells, tests and
// flushes at 0).  A store outside the lattice, or outside the row, ends the program with status 2: the emitter checks every one.
#include <cstdint>
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

typedef HostGrid<kEndUnread> RayGrid;

// the emitter of the kernel over host arrays: a run of voxels of ONE row gets the row's vote
struct Emit {
    std::vector<unsigned char>* ws;
    std::vector<int32_t>* inside;
    long long row_base, row_stride; int row_n;      // what the row owns
    int pass; bool last; int valid;
    void operator()(int first, int stride, int length, int state) const {
        const long long k = stride > 0 ? (first - row_base) / stride : -1;
        if (stride != row_stride || first < row_base || row_base + k * stride != first || length < 0 || k + length > row_n) { fprintf(stderr, "fill_lattice_host: a store outside the row\n"); exit(2); }
        for (int i = 0; i < length; i++) {
            const long long e = (long long)first + (long long)i * stride;
            if (e < 0 || size_t(e) >= inside->size()) { fprintf(stderr, "fill_lattice_host: a store outside the lattice\n"); exit(2); }
            hx::row_put(ws->data(), inside->data(), int(e), pass, last, valid, state);
        }
    }
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: fill_lattice_host brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    const bool walk = op == "walk";
    if (!((walk && argc == 8) || (op == "brute" && argc == 5))) { fprintf(stderr, "fill_lattice_host: unknown operation or wrong number of files: %s\n", op.c_str()); return 2; }
    Params p;
    p.bytes = read_file<char>(argv[2]);
    float origin[3], size[3]; int n[3];
    for (int i = 0; i < 3; i++) origin[i] = p.get<float>();
    for (int i = 0; i < 3; i++) size[i] = p.get<float>();
    for (int i = 0; i < 3; i++) n[i] = p.get<int32_t>();
    int axes = p.get<int32_t>();
    const bool winding = p.get<int32_t>() != 0;
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0 || (long long)n[0] * n[1] * n[2] > (1 << 26) || axes < 0 || axes > 7) { fprintf(stderr, "fill_lattice_host: bad lattice or axes\n"); return 2; }
    if (axes == 0) axes = 7;

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
    const Tri* t = g.tris.data();
    const int num_tris = int(g.tris.size());

    const size_t voxels = size_t(n[0]) * size_t(n[1]) * size_t(n[2]);
    std::vector<unsigned char> ws(voxels, 0xA5);            // the workspace's content before the first pass is unspecified
    std::vector<int32_t> inside(voxels, -2);
    std::vector<Hit> records;
    std::vector<unsigned char> abstained;
    int64_t totals[5] = {0, 0, 0, 0, 0};
    int pass = 0, last_axis = 0;
    for (int a = 0; a < 3; a++) if (axes & (1 << a)) last_axis = a;
    for (int a = 0; a < 3; a++) {
        if (!(axes & (1 << a))) continue;
        const long long rows = hx::num_rows(a, n[0], n[1], n[2]);
        for (long long r = 0; r < rows; r++) {
            const hx::Row w = hx::row_of(a, int(r), n[0], n[1], n[2]);
            hx::RowSink<Emit> sink;
            sink.emit = Emit{&ws, &inside, w.base, w.stride, w.n, pass, a == last_axis, 1};
            sink.init(w, origin[a], size[a], winding);
            const Ray ray = hx::row_ray(w, a, origin, size);
            Hit rec;
            if (walk) {
                hx::Counts c;
                rec = hx::crossings_walk<hx::kMaxPage>(g, ray, page, c, sink);
                sink.finish();
                totals[1] += c.cells; totals[2] += c.tests; totals[3] += c.flushes;
            } else {
                rec = hx::fill_row<256>([t](int j) { return t[j]; }, num_tris, ray, sink);
            }
            if (sink.c != w.n) { fprintf(stderr, "fill_lattice_host: a row was not finished\n"); return 2; }
            const bool out = sink.state() != 0;
            if (out) {                                      // the row ends inside: once more along it, as "abstains"
                sink.emit.valid = 0;
                sink.emit(w.base, w.stride, w.n, 0);
            }
            records.push_back(rec);
            abstained.push_back(out ? 1 : 0);
            totals[0]++; totals[4] += out ? 1 : 0;
        }
        pass++;
    }
    while (abstained.size() % 8) abstained.push_back(0);

    const char* out_name = argv[walk ? 7 : 4];
    FILE* f = fopen(out_name, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out_name); return 2; }
    bool ok = fwrite(inside.data(), sizeof(int32_t), inside.size(), f) == inside.size();
    ok = ok && fwrite(records.data(), sizeof(Hit), records.size(), f) == records.size();
    ok = ok && fwrite(abstained.data(), 1, abstained.size(), f) == abstained.size();
    ok = ok && fwrite(totals, sizeof(int64_t), 5, f) == 5;
    fclose(f);
    if (!ok) { fprintf(stderr, "cannot write %s\n", out_name); return 2; }
    return 0;
}
