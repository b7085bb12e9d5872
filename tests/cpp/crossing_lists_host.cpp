// crossing_lists_host -- hagrid_list_crossings on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: what one lane of the gfx950 kernel
// (hagrid_amd/csrc/crossings.hip, the list mode) does for its ray, with the header's functions: slot_range for the slots, crossings_brute_force (mode
// `brute`: no grid, a page of 256) or crossings_walk (mode `walk`: a grid in the construction format, a page capacity chosen at run time, 1 .. 8) with a sink
// that stores entry `position` while position < room, then the empty entry into the slots left over.  tests/test_crossing_lists_cpu.py compares what this
// writes with the fixture tests/golden/crossing_lists.npz and with scene.crossing_slots, tests/test_crossing_lists_gpu.py with what the device wrote.
//
//   crossing_lists_host brute PARAMS TRIS RAYS OFFSETS OUT                     PARAMS: i32 n, i32 stride, i64 capacity, i32 guard
//   crossing_lists_host walk  PARAMS ENTRIES CELLS REFS TRIS RAYS OFFSETS OUT  PARAMS: the same, then the grid header (host_support.h), i32 page
// OFFSETS: int64[n + 1] (the CSR form, stride 0), or an empty file with stride >= 1.  OUT: capacity + guard entries of 8 bytes (every byte 0xFF where nothing
// was written), then n Hit-shaped records, then int64[6] totals (rays, cells, tests, flushes, entries written, rays with m > room) and the int64 largest excess
// of a ray's flushes over ceil(count / page) + 1 (the brute force leaves cells, tests, flushes and the excess at 0).  A store outside the ray's own slots ends
// the program with status 2: the sink checks every one.
#include <cstdint>
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

typedef HostGrid<kEndUnread> RayGrid;

struct Slot { float t; int32_t key; };

// the sink of the kernel over a host array; [first, first + room) is all it may touch
struct ArraySink {
    std::vector<Slot>* slots;
    long long first, room;
    void put(long long position, float t, int32_t key) const {
        if (position < 0 || position >= room || first < 0 || size_t(first + position) >= slots->size()) { fprintf(stderr, "crossing_lists_host: a store outside the ray's slots\n"); exit(2); }
        Slot e; e.t = t; e.key = key;
        (*slots)[size_t(first + position)] = e;
    }
    void operator()(int position, float t, uint32_t key) const {
        if (position < room) put(position, t, int32_t(key));
    }
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: crossing_lists_host brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    const bool walk = op == "walk";
    if (!((walk && argc == 10) || (op == "brute" && argc == 7))) { fprintf(stderr, "crossing_lists_host: unknown operation or wrong number of files: %s\n", op.c_str()); return 2; }
    Params p;
    p.bytes = read_file<char>(argv[2]);
    const int n = p.get<int32_t>(), stride = p.get<int32_t>();
    const long long capacity = p.get<int64_t>();
    const int guard = p.get<int32_t>();
    if (n < 0 || stride < 0 || capacity < 0 || guard < 0) { fprintf(stderr, "crossing_lists_host: bad n, stride, capacity or guard\n"); return 2; }

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
    const std::vector<Ray> rays = read_file<Ray>(argv[walk ? 7 : 4]);
    const std::vector<long long> offsets = read_file<long long>(argv[walk ? 8 : 5]);
    if (int(rays.size()) != n) { fprintf(stderr, "crossing_lists_host: the ray file does not hold n records\n"); return 2; }
    if (offsets.empty() ? stride < 1 : (stride != 0 || offsets.size() != size_t(n) + 1)) { fprintf(stderr, "crossing_lists_host: offsets of n + 1 values, or a stride >= 1\n"); return 2; }
    if (offsets.empty() && (long long)n * stride > capacity) { fprintf(stderr, "crossing_lists_host: n * stride is beyond the capacity\n"); return 2; }

    Slot blank;
    memset(&blank, 0xFF, sizeof(blank));
    std::vector<Slot> slots(size_t(capacity) + size_t(guard), blank);
    std::vector<Hit> records(static_cast<size_t>(n));
    int64_t totals[7] = {n, 0, 0, 0, 0, 0, std::numeric_limits<int64_t>::min()};
    const Tri* t = g.tris.data();
    const int num_tris = int(g.tris.size());
    for (int i = 0; i < n; i++) {
        ArraySink sink;
        sink.slots = &slots;
        hx::slot_range(offsets.empty() ? nullptr : offsets.data(), stride, capacity, i, sink.first, sink.room);
        Hit rec;
        if (walk) {
            hx::Counts c;
            rec = hx::crossings_walk<hx::kMaxPage>(g, rays[i], page, c, sink);
            totals[1] += c.cells; totals[2] += c.tests; totals[3] += c.flushes;
            const int64_t excess = int64_t(c.flushes) - ((int64_t(rec.id) + page - 1) / page + 1);
            if (excess > totals[6]) totals[6] = excess;
        } else {
            rec = hx::crossings_brute_force<256>([t](int j) { return t[j]; }, num_tris, rays[i], sink);
        }
        const long long written = rec.id < sink.room ? rec.id : sink.room;
        for (long long s = written; s < sink.room; s++) sink.put(s, rays[i].tmax, -1);
        totals[4] += written; totals[5] += rec.id > sink.room ? 1 : 0;
        records[size_t(i)] = rec;
    }
    if (totals[6] == std::numeric_limits<int64_t>::min()) totals[6] = 0;

    const char* out_name = argv[walk ? 9 : 6];
    FILE* f = fopen(out_name, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out_name); return 2; }
    bool ok = slots.empty() || fwrite(slots.data(), sizeof(Slot), slots.size(), f) == slots.size();
    ok = ok && (records.empty() || fwrite(records.data(), sizeof(Hit), records.size(), f) == records.size());
    ok = ok && fwrite(totals, sizeof(int64_t), 7, f) == 7;
    fclose(f);
    if (!ok) { fprintf(stderr, "cannot write %s\n", out_name); return 2; }
    return 0;
}
