// overlap_lists_host -- the overlap lists (hagrid_amd.h: hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs, then hagrid_unique_lists and hagrid_compact_lists) on
// the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: RefList of include/hagrid/overlap.h under the three brute forces and under the walk
// that overlap_refs_kernel of hagrid_amd/csrc/overlap_lists.hip runs, and the segment operations of include/hagrid/unique_lists.h.
// tests/test_overlap_lists_cpu.py compares what this writes with hagrid_amd/scene.py (box_lists, contact_lists, obb_lists) and the fixtures
// tests/golden/{overlap,overlap_tris,obb}.npz, tests/test_overlap_lists_gpu.py with what the device wrote.
//
//   overlap_lists_host brute PARAMS TRIS RECORDS FIRST QLABELS TLABELS OFFSETS_OUT IDS_OUT
//       PARAMS: i32 shape (0 boxes, 1 contact queries, 2 oriented boxes), i32 n, 3 f32 grid box min, 3 f32 grid box max.  Every query against every triangle
//       through RefList, then unique_segment: the lists in CSR form (i64 n + 1 offsets, i32 ids).
//   overlap_lists_host walk  PARAMS GRID_ENTRIES CELLS REFS TRIS RECORDS FIRST QLABELS TLABELS OFFSETS_INOUT ENTRIES_INOUT COUNTS_OUT TOTALS_OUT LIST_OFFSETS_OUT LIST_IDS_OUT
//       PARAMS: the grid header of host_support.h, i32 shape, i32 n, i32 given, i64 capacity.
//       given = 0: the whole protocol -- count, scan, fill, unique, scan, compact.  OFFSETS_INOUT gets the exclusive sums of the counts, ENTRIES_INOUT the
//       filled references BEFORE the sort, LIST_OFFSETS_OUT / LIST_IDS_OUT the lists.
//       given = 1: fill mode alone into the caller's ranges: OFFSETS_INOUT holds n + 1 offsets, ENTRIES_INOUT `capacity` entries (the caller's poison) and gets
//       what the kernel writes; the two list files are written empty.
//       COUNTS_OUT: n x 4 i32 (R, cells visited, tests evaluated, blocks pruned); TOTALS_OUT: the fill launch's six i64 totals.
// RECORDS: n records of 32 bytes (boxes), 48 (Tri) or 64 (oriented boxes).  FIRST: n i32 or empty (contact queries only; boxes carry it in the record).
// QLABELS: 3 n i32 (contact) or n i32 (oriented boxes), TLABELS: 3 i32 per triangle, or both empty (no labels).  An entry: {f32 d2 = +0.0, i32 id}.
#include <string>
#include <vector>

#include "hagrid/crossings.h"
#include "hagrid/obb.h"
#include "hagrid/overlap.h"
#include "hagrid/unique_lists.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace ho = hagrid::overlap;
namespace hb = hagrid::obb;
namespace hl = hagrid::lists;

namespace {

enum Shape { kBoxes = 0, kContact = 1, kObbs = 2 };

struct BoxRecord { float lo[3]; int first; float hi[3]; float pad; };
static_assert(sizeof(BoxRecord) == 32 && sizeof(Tri) == 48 && sizeof(hb::ObbRecord) == 64 && sizeof(hl::Entry) == 8, "record layout");

// the accessor of overlap.h: the grid and the clip box
struct OverlapGrid : HostGrid<kEndUnbounded> { ho::Clip clip; };

struct Span {
    hl::Entry* p;
    hl::Entry get(long long i) const { return p[i]; }
    void set(long long i, const hl::Entry& e) { p[i] = e; }
};
struct PushStore {
    std::vector<hl::Entry>* v;
    void operator()(int, int id) const { hl::Entry e; e.d2 = 0.0f; e.id = id; v->push_back(e); }
};
struct SlotStore {
    hl::Entry* slots;
    void operator()(int position, int id) const { slots[position].d2 = 0.0f; slots[position].id = id; }
};

int tri_label_at(const std::vector<int32_t>& labels, int id, int i) {
    const size_t at = 3 * size_t(id) + size_t(i);
    if (id < 0 || at >= labels.size()) { fprintf(stderr, "triangle id beyond the labels\n"); exit(2); }
    return labels[at];
}

// the query of overlap.h's TriFilter
struct TriQuery {
    const Tri* rec;
    const int32_t* labels;                  // of this query, or null
    const std::vector<int32_t>* tri_labels_;
    const Tri& tri() const { return *rec; }
    bool labelled() const { return labels != nullptr; }
    int label(int i) const { return labels[i]; }
    int tri_label(int id, int i) const { return tri_label_at(*tri_labels_, id, i); }
};

// the query of obb.h's ObbFilter
struct ObbQuery {
    const hb::ObbRecord* rec;
    const int32_t* label_;                  // of this query, or null
    const std::vector<int32_t>* tri_labels_;
    hb::Obb box() const { return hb::from_record(*rec); }
    bool labelled() const { return label_ != nullptr; }
    int label() const { return *label_; }
    int tri_label(int id, int i) const { return tri_label_at(*tri_labels_, id, i); }
};

// the batch as the files give it
struct Batch {
    int shape, n;
    std::vector<BoxRecord> boxes;
    std::vector<Tri> queries;
    std::vector<hb::ObbRecord> obbs;
    std::vector<int32_t> first, qlabels, tlabels;

    void load(int shape_, int n_, size_t num_tris, const char* records, const char* f, const char* ql, const char* tl) {
        shape = shape_; n = n_;
        size_t have = 0;
        if (shape == kBoxes) { boxes = read_file<BoxRecord>(records); have = boxes.size(); }
        else if (shape == kContact) { queries = read_file<Tri>(records); have = queries.size(); }
        else if (shape == kObbs) { obbs = read_file<hb::ObbRecord>(records); have = obbs.size(); }
        else { fprintf(stderr, "unknown shape\n"); exit(2); }
        if (have != size_t(n)) { fprintf(stderr, "the record file does not hold n records\n"); exit(2); }
        first = read_file<int32_t>(f); qlabels = read_file<int32_t>(ql); tlabels = read_file<int32_t>(tl);
        if (!first.empty() && (shape != kContact || first.size() != size_t(n))) { fprintf(stderr, "the file of firsts does not hold n values for contact queries\n"); exit(2); }
        if (qlabels.empty() != tlabels.empty()) { fprintf(stderr, "one label file without the other\n"); exit(2); }
        const size_t per_query = shape == kContact ? 3 : 1;
        if (!qlabels.empty() && (shape == kBoxes || qlabels.size() != per_query * size_t(n) || tlabels.size() != 3 * num_tris)) { fprintf(stderr, "the label files do not fit the shape\n"); exit(2); }
    }
    int first_of(int i) const { return shape == kBoxes ? boxes[i].first : (shape == kObbs ? obbs[i].first : (first.empty() ? 0 : first[i])); }
    TriQuery tri_query(int i) const {
        TriQuery q;
        q.rec = &queries[i]; q.labels = qlabels.empty() ? nullptr : qlabels.data() + 3 * size_t(i); q.tri_labels_ = &tlabels;
        return q;
    }
    ObbQuery obb_query(int i) const {
        ObbQuery q;
        q.rec = &obbs[i]; q.label_ = qlabels.empty() ? nullptr : qlabels.data() + i; q.tri_labels_ = &tlabels;
        return q;
    }

    /// the brute force of query i's shape
    template <typename L>
    void brute(const std::vector<Tri>& tris, const ho::Clip& clip, float eps, int i, L& list) const {
        const Tri* t = tris.data();
        auto tri_at = [t](int j) { return t[j]; };
        list.init(first_of(i));
        if (shape == kBoxes) ho::brute_force(tri_at, int(tris.size()), clip, vec3(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), vec3(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]), false, list);
        else if (shape == kContact) ho::tris_brute_force(tri_at, int(tris.size()), clip, eps, tri_query(i), false, list);
        else hb::obb_brute_force(tri_at, int(tris.size()), clip, eps, obb_query(i), false, list);
    }
    /// the walk of query i's shape: what overlap_refs_kernel runs
    template <typename S, typename L>
    void walk(const OverlapGrid& g, S& st, int i, L& list, ho::Counts& c) const {
        list.init(first_of(i));
        if (shape == kBoxes) ho::overlap_query(g, st, vec3(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), vec3(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]), false, list, c);
        else if (shape == kContact) ho::tris_query(g, st, tri_query(i), false, list, c);
        else hb::obb_query(g, st, obb_query(i), false, list, c);
    }
};

/// one launch of the kernel on the host: count mode (offsets null) or fill mode.  counts: n x 4, totals: six, ADDED to
void refs_launch(const OverlapGrid& g, const Batch& b, const long long* offsets, hl::Entry* entries, long long capacity, std::vector<int32_t>& counts, std::vector<int64_t>& totals) {
    ho::ArrayStack<ho::kMaxLevels> st;
    for (int i = 0; i < b.n; i++) {
        long long first = 0, room = 0;
        if (offsets) crossings::slot_range(offsets, 0, capacity, i, first, room);
        ho::RefList<SlotStore> list;
        list.store.slots = entries + first;
        list.room = int(room < 0x7fffffffLL ? room : 0x7fffffffLL);
        ho::Counts c;
        b.walk(g, st, i, list, c);
        const int written = list.count < list.room ? list.count : list.room;
        for (long long s = written; s < room; s++) entries[size_t(first + s)] = hl::empty_entry();
        counts[size_t(i) * 4] = list.count; counts[size_t(i) * 4 + 1] = c.cells; counts[size_t(i) * 4 + 2] = c.sats; counts[size_t(i) * 4 + 3] = c.pruned;
        totals[0] += 1; totals[1] += c.cells; totals[2] += c.sats; totals[3] += c.pruned;
        if (offsets) { totals[4] += written; totals[5] += list.count > list.room ? 1 : 0; }
    }
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: overlap_lists_host brute|walk PARAMS ...\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "brute" && argc == 10) {
        const int shape = p.get<int32_t>(), n = p.get<int32_t>();
        const vec3 glo = p.get3(), ghi = p.get3();
        ho::Clip clip;
        clip.set(glo, ghi);
        const float eps = ho::GridConsts::abs_margin(glo, ghi);
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        Batch batch;
        batch.load(shape, n, tris.size(), argv[4], argv[5], argv[6], argv[7]);
        std::vector<long long> offsets(size_t(n) + 1, 0);
        std::vector<int32_t> ids;
        std::vector<hl::Entry> one;
        for (int i = 0; i < n; i++) {
            one.clear();
            ho::RefList<PushStore> list;
            list.store.v = &one;
            list.room = INT_MAX;
            batch.brute(tris, clip, eps, i, list);
            if (size_t(list.count) != one.size()) { fprintf(stderr, "brute: count and stores differ\n"); return 2; }
            Span s{one.data()};
            const long long m = hl::unique_segment(s, (long long)one.size());
            if (m != (long long)one.size()) { fprintf(stderr, "brute: the brute force offered a triangle twice\n"); return 2; }
            for (long long j = 0; j < m; j++) ids.push_back(one[size_t(j)].id);
            offsets[size_t(i) + 1] = (long long)ids.size();
        }
        write_file(argv[8], offsets);
        write_file(argv[9], ids);
        return 0;
    }
    if (op == "walk" && argc == 17) {
        const GridHeader h = p.get_grid_header();
        const int shape = p.get<int32_t>(), n = p.get<int32_t>();
        const bool given = p.get<int32_t>() != 0;
        long long capacity = p.get<int64_t>();
        OverlapGrid g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.clip.set(h.lo, h.hi);
        g.tris = read_file<Tri>(argv[6]);
        Batch batch;
        batch.load(shape, n, g.tris.size(), argv[7], argv[8], argv[9], argv[10]);
        std::vector<int32_t> counts(size_t(n) * 4);
        std::vector<int64_t> totals(6, 0);
        std::vector<long long> offsets, list_offsets;
        std::vector<hl::Entry> entries;
        std::vector<int32_t> list_ids;
        if (given) {
            offsets = read_file<long long>(argv[11]);
            entries = read_file<hl::Entry>(argv[12]);
            if (int(offsets.size()) != n + 1 || (long long)entries.size() != capacity) { fprintf(stderr, "the files do not hold n + 1 offsets and `capacity` entries\n"); return 2; }
            refs_launch(g, batch, offsets.data(), entries.data(), capacity, counts, totals);
            write_file(argv[12], entries);
        } else {
            std::vector<int64_t> count_totals(6, 0);
            refs_launch(g, batch, nullptr, nullptr, 0, counts, count_totals);                      // count
            if (count_totals[4] != 0 || count_totals[5] != 0) { fprintf(stderr, "count mode wrote\n"); return 2; }
            offsets.assign(size_t(n) + 1, 0);
            for (int i = 0; i < n; i++) offsets[size_t(i) + 1] = offsets[i] + counts[size_t(i) * 4];      // scan
            capacity = offsets[n];
            hl::Entry poison;
            memset(&poison, 0xFF, sizeof poison);
            entries.assign(size_t(capacity), poison);
            std::vector<int32_t> again(size_t(n) * 4);
            refs_launch(g, batch, offsets.data(), entries.data(), capacity, again, totals);       // fill
            if (again != counts) { fprintf(stderr, "fill mode counts differ from count mode's\n"); return 2; }
            write_file(argv[11], offsets);
            write_file(argv[12], entries);                                                         // the references before the sort
            std::vector<int32_t> m(size_t(n), 0);
            for (int i = 0; i < n; i++) {                                                           // unique
                long long first, room;
                hl::segment_range(offsets.data(), capacity, i, first, room);
                Span s{entries.data() + first};
                m[i] = int32_t(hl::unique_segment(s, room));
            }
            list_offsets.assign(size_t(n) + 1, 0);
            for (int i = 0; i < n; i++) list_offsets[size_t(i) + 1] = list_offsets[i] + m[i];      // scan
            const long long out_capacity = list_offsets[n];
            list_ids.assign(size_t(out_capacity), -2);
            for (int i = 0; i < n; i++) {                                                           // compact
                long long first, room, dfirst, droom;
                hl::segment_range(offsets.data(), capacity, i, first, room);
                hl::segment_range(list_offsets.data(), out_capacity, i, dfirst, droom);
                const long long c = hl::compact_count(m[i], room, droom);
                for (long long s = 0; s < droom; s++) list_ids[size_t(dfirst + s)] = s < c ? entries[size_t(first + s)].id : hl::empty_entry().id;
            }
        }
        write_file(argv[13], counts);
        write_file(argv[14], totals);
        write_file(argv[15], list_offsets);
        write_file(argv[16], list_ids);
        return 0;
    }
    fprintf(stderr, "overlap_lists_host: unknown operation or wrong number of files: %s\n", op.c_str());
    return 2;
}
