// overlap_host -- include/hagrid/overlap.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: the triangle / box test,
// the brute-force definition and the walk over the construction format that hagrid_amd/csrc/overlap.hip runs on the device.
// tests/test_overlap_cpu.py compares what this writes with hagrid_amd/scene.py and the fixture tests/golden/overlap.npz,
// tests/test_overlap_gpu.py with what the device wrote.
//
//   overlap_host pairs PARAMS TRIS BOXES OUT         PARAMS: i32 n;  triangle i against box i;  OUT: n i32 (1: the triangle meets the box)
//   overlap_host brute PARAMS TRIS BOXES IDS COUNTS  PARAMS: i32 n, i32 k, i32 any, 3 f32 grid box min, 3 f32 grid box max;  every box, clipped, against all triangles;  IDS: n x k i32, COUNTS: n i32
//   overlap_host walk  PARAMS ENTRIES CELLS REFS TRIS BOXES IDS COUNTS TOTALS
//                                                    PARAMS: i32 small, 3 i32 top-level dims, i32 shift, 3 f32 bbox min, 3 f32 bbox max, i32 n, i32 k, i32 any;
//                                                    TOTALS: n x 3 i32 (cells visited, tests evaluated, sub-blocks pruned)
// A box is 32 bytes: 3 f32 min, i32 first, 3 f32 max, i32 pad.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/overlap.h"

using namespace hagrid;
namespace hc = hagrid::closest;
namespace ho = hagrid::overlap;

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

struct BoxRec { float lo[3]; int32_t first; float hi[3]; int32_t pad; };
static_assert(sizeof(BoxRec) == 32, "record layout");

typedef ho::IdList<ho::kMaxIds> List;

void to_record(const List& l, int k, int32_t* ids, int32_t& count) {
    for (int j = 0; j < k; j++) ids[j] = l.id[j];
    count = l.count();
}

// the grid arrays with bounds checks: a walk that leaves them is a bug of the walk, not a crash
struct HostGrid {
    hc::GridConsts c;
    ho::Clip clip;
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
    if (argc < 4) { fprintf(stderr, "usage: overlap_host pairs|brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "pairs" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<BoxRec> boxes = read_file<BoxRec>(argv[4]);
        if (int(tris.size()) != n || int(boxes.size()) != n) { fprintf(stderr, "pairs: the files do not hold n records\n"); return 2; }
        std::vector<int32_t> out(size_t(n), 0);
        for (int i = 0; i < n; i++) {
            const vec3 lo(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), hi(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]);
            out[i] = (!ho::inactive(lo, hi) && ho::meets(tris[i], lo, hi)) ? 1 : 0;
        }
        write_file(argv[5], out);
    } else if (op == "brute" && argc == 7) {
        const int n = p.get<int32_t>(), k = p.get<int32_t>(), any = p.get<int32_t>();
        const vec3 glo = p.get3(), ghi = p.get3();
        ho::Clip clip;
        clip.set(glo, ghi);
        if (k < 1 || k > ho::kMaxIds || (any && k != 1)) { fprintf(stderr, "brute: bad k\n"); return 2; }
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<BoxRec> boxes = read_file<BoxRec>(argv[4]);
        if (int(boxes.size()) != n) { fprintf(stderr, "brute: the box file does not hold n records\n"); return 2; }
        std::vector<int32_t> ids(size_t(n) * k), counts((size_t(n)));
        const Tri* t = tris.data();
        for (int i = 0; i < n; i++) {
            const vec3 lo(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), hi(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]);
            List l;
            l.init(k, boxes[i].first);
            ho::brute_force([t](int j) { return t[j]; }, int(tris.size()), clip, lo, hi, any != 0, l);
            to_record(l, k, ids.data() + size_t(i) * k, counts[i]);
        }
        write_file(argv[5], ids);
        write_file(argv[6], counts);
    } else if (op == "walk" && argc == 11) {
        const int small = p.get<int32_t>();
        ivec3 top;
        top.x = p.get<int32_t>(); top.y = p.get<int32_t>(); top.z = p.get<int32_t>();
        const int shift = p.get<int32_t>();
        const vec3 glo = p.get3(), ghi = p.get3();
        const int n = p.get<int32_t>(), k = p.get<int32_t>(), any = p.get<int32_t>();
        if (shift < 0 || shift > 15) { fprintf(stderr, "walk: bad shift\n"); return 2; }
        if (k < 1 || k > ho::kMaxIds || (any && k != 1)) { fprintf(stderr, "walk: bad k\n"); return 2; }
        const std::vector<uint32_t> entries = read_file<uint32_t>(argv[3]);
        const std::vector<char> cells = read_file<char>(argv[4]);
        const std::vector<int32_t> refs = read_file<int32_t>(argv[5]);
        const std::vector<Tri> tris = read_file<Tri>(argv[6]);
        const std::vector<BoxRec> boxes = read_file<BoxRec>(argv[7]);
        if (int(boxes.size()) != n) { fprintf(stderr, "walk: the box file does not hold n records\n"); return 2; }
        HostGrid g;
        g.c.set(top, shift, glo, ghi);
        g.clip.set(glo, ghi);
        g.entries = entries.data(); g.num_entries = entries.size();
        g.cells = small ? nullptr : reinterpret_cast<const Cell*>(cells.data());
        g.small_cells = small ? reinterpret_cast<const SmallCell*>(cells.data()) : nullptr;
        g.num_cells = cells.size() / (small ? sizeof(SmallCell) : sizeof(Cell));
        g.refs = refs.data(); g.num_refs = refs.size();
        g.tris = tris.data(); g.num_tris = tris.size();
        std::vector<int32_t> ids(size_t(n) * k), counts((size_t(n))), totals(size_t(n) * 3);
        hc::ArrayStack<hc::kMaxLevels> st;
        for (int i = 0; i < n; i++) {
            const vec3 lo(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), hi(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]);
            List l;
            l.init(k, boxes[i].first);
            ho::Counts c;
            ho::overlap_query(g, st, lo, hi, any != 0, l, c);
            to_record(l, k, ids.data() + size_t(i) * k, counts[i]);
            totals[size_t(i) * 3] = c.cells; totals[size_t(i) * 3 + 1] = c.sats; totals[size_t(i) * 3 + 2] = c.pruned;
        }
        write_file(argv[8], ids);
        write_file(argv[9], counts);
        write_file(argv[10], totals);
    } else {
        fprintf(stderr, "overlap_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
