// closest_host -- include/hagrid/closest.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: the per-pair
// arithmetic, the brute-force definition and the walk over the construction format that hagrid_amd/csrc/closest.hip runs on the device.
// tests/test_closest_cpu.py compares what this writes with hagrid_amd/scene.py and the fixture tests/golden/closest.npz,
// tests/test_closest_gpu.py with what the device wrote.
//
//   closest_host pairs PARAMS TRIS POINTS OUT        PARAMS: i32 n;  triangle i against point i;  OUT: n x 8 words: i32 valid, f32 d2, 3 f32 q,
//                                                    i32 feature, i32 side, 0
//   closest_host brute PARAMS TRIS POINTS OUT        PARAMS: i32 n;  every point against all triangles;  OUT: n result records (32 bytes)
//   closest_host walk  PARAMS ENTRIES CELLS REFS TRIS POINTS OUT COUNTS
//                                                    PARAMS: i32 small, 3 i32 top-level dims, i32 shift, 3 f32 bbox min, 3 f32 bbox max, i32 n;
//                                                    OUT: n result records;  COUNTS: n x 3 i32 (cells visited, triangles tested, pruned)
// A point is 4 f32: x, y, z, r.  A result record: {f32 qx, qy, qz, d2}, {i32 id, i32 feature, f32 side, 0}.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/closest.h"

using namespace hagrid;
namespace hc = hagrid::closest;

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

struct Point { float x, y, z, r; };
struct Result { float qx, qy, qz, d2; int32_t id, feature; float side; int32_t zero; };
static_assert(sizeof(Point) == 16 && sizeof(Result) == 32, "record layout");

Result to_record(const hc::Best& b) {
    Result r;
    r.qx = b.q.x; r.qy = b.q.y; r.qz = b.q.z; r.d2 = b.d2;
    r.id = b.id; r.feature = b.feature; r.side = float(b.side); r.zero = 0;
    return r;
}

// the grid arrays with bounds checks: a walk that leaves them is a bug of the walk, not a crash
struct HostGrid {
    hc::GridConsts c;
    const uint32_t* entries; size_t num_entries;
    const Cell* cells; const SmallCell* small_cells; size_t num_cells;
    const int* refs; size_t num_refs;
    const Tri* tris; size_t num_tris;

    uint32_t word(uint32_t i) const {
        if (i >= num_entries) { fprintf(stderr, "walk: entry index beyond the voxel map\n"); exit(2); }
        return entries[i];
    }
    hc::CellRec cell(uint32_t i) const {
        if (i >= num_cells) { fprintf(stderr, "walk: cell index beyond the cells\n"); exit(2); }
        hc::CellRec r;
        if (small_cells) {
            const SmallCell& s = small_cells[i];
            r.lx = s.min.x; r.ly = s.min.y; r.lz = s.min.z; r.hx = s.max.x; r.hy = s.max.y; r.hz = s.max.z; r.begin = s.begin; r.end = INT_MAX;
        } else {
            const Cell& s = cells[i];
            r.lx = s.min.x; r.ly = s.min.y; r.lz = s.min.z; r.hx = s.max.x; r.hy = s.max.y; r.hz = s.max.z; r.begin = s.begin; r.end = s.end;
        }
        return r;
    }
    int ref(int i) const {
        if (i < 0 || size_t(i) >= num_refs) { fprintf(stderr, "walk: reference index beyond ref_ids\n"); exit(2); }
        return refs[i];
    }
    Tri tri(int id) const {
        if (id < 0 || size_t(id) >= num_tris) { fprintf(stderr, "walk: triangle id beyond the triangles\n"); exit(2); }
        return tris[id];
    }
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: closest_host pairs|brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "pairs" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Point> pts = read_file<Point>(argv[4]);
        if (int(tris.size()) != n || int(pts.size()) != n) { fprintf(stderr, "pairs: the files do not hold n records\n"); return 2; }
        std::vector<uint32_t> out(size_t(n) * 8, 0u);
        for (int i = 0; i < n; i++) {
            const vec3 pt(pts[i].x, pts[i].y, pts[i].z);
            hc::Pair r;
            uint32_t* o = out.data() + size_t(i) * 8;
            if (!hc::point_tri(tris[i], pt, r)) continue;
            o[0] = 1u; o[1] = as<uint32_t>(r.d2); o[2] = as<uint32_t>(r.q.x); o[3] = as<uint32_t>(r.q.y); o[4] = as<uint32_t>(r.q.z);
            o[5] = uint32_t(r.feature); o[6] = uint32_t(hc::tri_side(tris[i], pt, r.q));
        }
        write_file(argv[5], out);
    } else if (op == "brute" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Point> pts = read_file<Point>(argv[4]);
        if (int(pts.size()) != n) { fprintf(stderr, "brute: the point file does not hold n records\n"); return 2; }
        std::vector<Result> out((size_t(n)));
        const Tri* t = tris.data();
        for (int i = 0; i < n; i++) {
            hc::Best b;
            hc::brute_force([t](int j) { return t[j]; }, int(tris.size()), vec3(pts[i].x, pts[i].y, pts[i].z), pts[i].r, b);
            out[i] = to_record(b);
        }
        write_file(argv[5], out);
    } else if (op == "walk" && argc == 10) {
        const int small = p.get<int32_t>();
        ivec3 top;
        top.x = p.get<int32_t>(); top.y = p.get<int32_t>(); top.z = p.get<int32_t>();
        const int shift = p.get<int32_t>();
        const vec3 lo = p.get3(), hi = p.get3();
        const int n = p.get<int32_t>();
        if (shift < 0 || shift > 15) { fprintf(stderr, "walk: bad shift\n"); return 2; }
        const std::vector<uint32_t> entries = read_file<uint32_t>(argv[3]);
        const std::vector<char> cells = read_file<char>(argv[4]);
        const std::vector<int32_t> refs = read_file<int32_t>(argv[5]);
        const std::vector<Tri> tris = read_file<Tri>(argv[6]);
        const std::vector<Point> pts = read_file<Point>(argv[7]);
        if (int(pts.size()) != n) { fprintf(stderr, "walk: the point file does not hold n records\n"); return 2; }
        HostGrid g;
        g.c.set(top, shift, lo, hi);
        g.entries = entries.data(); g.num_entries = entries.size();
        g.cells = small ? nullptr : reinterpret_cast<const Cell*>(cells.data());
        g.small_cells = small ? reinterpret_cast<const SmallCell*>(cells.data()) : nullptr;
        g.num_cells = cells.size() / (small ? sizeof(SmallCell) : sizeof(Cell));
        g.refs = refs.data(); g.num_refs = refs.size();
        g.tris = tris.data(); g.num_tris = tris.size();
        std::vector<Result> out((size_t(n)));
        std::vector<int32_t> counts(size_t(n) * 3);
        hc::ArrayStack<hc::kMaxLevels> st;
        for (int i = 0; i < n; i++) {
            hc::Best b;
            hc::Counts c;
            hc::closest_query(g, st, vec3(pts[i].x, pts[i].y, pts[i].z), pts[i].r, b, c);
            out[i] = to_record(b);
            counts[size_t(i) * 3] = c.cells; counts[size_t(i) * 3 + 1] = c.tris; counts[size_t(i) * 3 + 2] = c.pruned;
        }
        write_file(argv[8], out);
        write_file(argv[9], counts);
    } else {
        fprintf(stderr, "closest_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
