// ball_lists_host -- the ball lists (hagrid_amd.h: hagrid_ball_refs, hagrid_unique_lists, hagrid_compact_lists) on the HOST (g++ -ffp-contract=off -DHOST=
// -DDEVICE=), driven from files: RefSink of include/hagrid/closest.h under the brute force and under the walk that ball_refs_kernel of
// hagrid_amd/csrc/ball_lists.hip runs, and the segment operations of include/hagrid/unique_lists.h with the network that unique_lists_kernel runs.
// tests/test_ball_lists_cpu.py compares what this writes with hagrid_amd/scene.py (tris_within, unique_lists, compact_lists) and the fixture
// tests/golden/ball_lists.npz, tests/test_ball_lists_gpu.py with what the device wrote.
//
//   ball_lists_host brute   PARAMS TRIS POINTS QLABELS TLABELS OFFSETS_OUT ENTRIES_OUT
//       PARAMS: i32 n, i32 labels given.  Every query against every triangle through RefSink, then unique_segment: the lists in CSR form (i64 n + 1 offsets).
//   ball_lists_host refs    PARAMS GRID_ENTRIES CELLS REFS TRIS POINTS QLABELS TLABELS OFFSETS ENTRIES_INOUT COUNTS_OUT COUNTERS_OUT
//       PARAMS: the grid header of host_support.h, i32 n, i32 labels given, i32 fill, i64 capacity.  fill = 0: count mode (OFFSETS and ENTRIES_INOUT are not
//       read).  fill = 1: ENTRIES_INOUT holds `capacity` entries (the caller's poison) and gets what the kernel writes.  COUNTS_OUT: n x 4 i32 (R, cells
//       visited, triangles tested, pruned); COUNTERS_OUT: the six i64 totals.
//   ball_lists_host unique  PARAMS OFFSETS ENTRIES_INOUT COUNTS_OUT          PARAMS: i32 n, i64 capacity
//   ball_lists_host compact PARAMS OFFSETS ENTRIES COUNTS OUT_OFFSETS OUT_ENTRIES_INOUT          PARAMS: i32 n, i64 capacity, i64 out_capacity
// An entry: {f32 d2, i32 id}.  QLABELS n i32, TLABELS 3 i32 per triangle (not read when labels are not given).
#include <string>
#include <vector>

#include "hagrid/closest.h"
#include "hagrid/crossings.h"
#include "hagrid/unique_lists.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace hc = hagrid::closest;
namespace hl = hagrid::lists;

namespace {

struct Query { float x, y, z, r; };
static_assert(sizeof(Query) == 16 && sizeof(hl::Entry) == 8, "record layout");

struct Span {
    hl::Entry* p;
    hl::Entry get(long long i) const { return p[i]; }
    void set(long long i, const hl::Entry& e) { p[i] = e; }
};
struct PushStore {
    std::vector<hl::Entry>* v;
    void operator()(int, float d2, int id) const { hl::Entry e; e.d2 = d2; e.id = id; v->push_back(e); }
};
struct SlotStore {
    hl::Entry* slots;
    void operator()(int position, float d2, int id) const { slots[position].d2 = d2; slots[position].id = id; }
};

struct Labels {
    std::vector<int32_t> q, t;
    void load(bool given, const char* qf, const char* tf, int n, size_t num_tris) {
        if (!given) return;
        q = read_file<int32_t>(qf); t = read_file<int32_t>(tf);
        if (int(q.size()) != n || t.size() != 3 * num_tris) { fprintf(stderr, "the files do not hold n query labels or 3 labels per triangle\n"); exit(2); }
    }
    int of(int i) const { return q.empty() ? -1 : q[i]; }
    const int32_t* tris() const { return t.empty() ? nullptr : t.data(); }
};

std::vector<long long> read_offsets(const char* file, int n) {
    std::vector<long long> o = read_file<long long>(file);
    if (int(o.size()) != n + 1) { fprintf(stderr, "%s does not hold n + 1 offsets\n", file); exit(2); }
    return o;
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: ball_lists_host brute|refs|unique|compact PARAMS ...\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "brute" && argc == 9) {
        const int n = p.get<int32_t>();
        const bool labelled = p.get<int32_t>() != 0;
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Query> q = read_file<Query>(argv[4]);
        if (int(q.size()) != n) { fprintf(stderr, "the file does not hold n queries\n"); return 2; }
        Labels labels;
        labels.load(labelled, argv[5], argv[6], n, tris.size());
        std::vector<long long> offsets(size_t(n) + 1, 0);
        std::vector<hl::Entry> all, one;
        const Tri* t = tris.data();
        for (int i = 0; i < n; i++) {
            one.clear();
            hc::RefSink<PushStore> sink;
            sink.store.v = &one;
            sink.setup(INT_MAX, labels.of(i), labels.tris());
            hc::brute_force([t](int j) { return t[j]; }, int(tris.size()), vec3(q[i].x, q[i].y, q[i].z), q[i].r, sink);
            if (size_t(sink.count) != one.size()) { fprintf(stderr, "brute: count and stores differ\n"); return 2; }
            Span s{one.data()};
            const long long m = hl::unique_segment(s, (long long)one.size());
            all.insert(all.end(), one.begin(), one.begin() + m);
            offsets[size_t(i) + 1] = (long long)all.size();
        }
        write_file(argv[7], offsets);
        write_file(argv[8], all);
        return 0;
    }
    if (op == "refs" && argc == 14) {
        const GridHeader h = p.get_grid_header();
        const int n = p.get<int32_t>();
        const bool labelled = p.get<int32_t>() != 0, fill = p.get<int32_t>() != 0;
        const long long capacity = p.get<int64_t>();
        HostGrid<kEndUnbounded> g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.tris = read_file<Tri>(argv[6]);
        const std::vector<Query> q = read_file<Query>(argv[7]);
        if (int(q.size()) != n) { fprintf(stderr, "the file does not hold n queries\n"); return 2; }
        Labels labels;
        labels.load(labelled, argv[8], argv[9], n, g.tris.size());
        std::vector<long long> offsets;
        std::vector<hl::Entry> entries;
        if (fill) {
            offsets = read_offsets(argv[10], n);
            entries = read_file<hl::Entry>(argv[11]);
            if ((long long)entries.size() != capacity) { fprintf(stderr, "the file does not hold `capacity` entries\n"); return 2; }
        }
        std::vector<int32_t> counts(size_t(n) * 4);
        std::vector<int64_t> counters(6, 0);
        hc::ArrayStack<hc::kMaxLevels> st;
        for (int i = 0; i < n; i++) {
            long long first = 0, room = 0;
            if (fill) crossings::slot_range(offsets.data(), 0, capacity, i, first, room);
            hc::RefSink<SlotStore> sink;
            sink.store.slots = entries.data() + first;
            sink.setup(int(room < 0x7fffffffLL ? room : 0x7fffffffLL), labels.of(i), labels.tris());
            hc::Counts c;
            hc::closest_query(g, st, vec3(q[i].x, q[i].y, q[i].z), q[i].r, sink, c);
            const int written = sink.count < sink.room ? sink.count : sink.room;
            for (long long s = written; s < room; s++) entries[size_t(first + s)] = hl::empty_entry();
            counts[size_t(i) * 4] = sink.count; counts[size_t(i) * 4 + 1] = c.cells; counts[size_t(i) * 4 + 2] = c.tris; counts[size_t(i) * 4 + 3] = c.pruned;
            counters[0] += 1; counters[1] += c.cells; counters[2] += c.tris; counters[3] += c.pruned;
            if (fill) { counters[4] += written; counters[5] += sink.count > sink.room ? 1 : 0; }
        }
        if (fill) write_file(argv[11], entries);
        write_file(argv[12], counts);
        write_file(argv[13], counters);
        return 0;
    }
    if (op == "unique" && argc == 6) {
        const int n = p.get<int32_t>();
        const long long capacity = p.get<int64_t>();
        const std::vector<long long> offsets = read_offsets(argv[3], n);
        std::vector<hl::Entry> entries = read_file<hl::Entry>(argv[4]);
        if ((long long)entries.size() != capacity) { fprintf(stderr, "the file does not hold `capacity` entries\n"); return 2; }
        std::vector<int32_t> counts(size_t(n), 0);
        for (int i = 0; i < n; i++) {
            long long first, room;
            hl::segment_range(offsets.data(), capacity, i, first, room);
            Span s{entries.data() + first};
            counts[i] = int32_t(hl::unique_segment(s, room));
        }
        write_file(argv[4], entries);
        write_file(argv[5], counts);
        return 0;
    }
    if (op == "compact" && argc == 8) {
        const int n = p.get<int32_t>();
        const long long capacity = p.get<int64_t>(), out_capacity = p.get<int64_t>();
        const std::vector<long long> offsets = read_offsets(argv[3], n), out_offsets = read_offsets(argv[6], n);
        const std::vector<hl::Entry> entries = read_file<hl::Entry>(argv[4]);
        const std::vector<int32_t> counts = read_file<int32_t>(argv[5]);
        std::vector<hl::Entry> out = read_file<hl::Entry>(argv[7]);
        if ((long long)entries.size() != capacity || (long long)out.size() != out_capacity || int(counts.size()) != n) { fprintf(stderr, "the files do not fit the parameters\n"); return 2; }
        for (int i = 0; i < n; i++) {
            long long first, room, dfirst, droom;
            hl::segment_range(offsets.data(), capacity, i, first, room);
            hl::segment_range(out_offsets.data(), out_capacity, i, dfirst, droom);
            const long long c = hl::compact_count(counts[i], room, droom);
            for (long long s = 0; s < droom; s++) out[size_t(dfirst + s)] = s < c ? entries[size_t(first + s)] : hl::empty_entry();
        }
        write_file(argv[7], out);
        return 0;
    }
    fprintf(stderr, "ball_lists_host: unknown operation or wrong number of files: %s\n", op.c_str());
    return 2;
}
