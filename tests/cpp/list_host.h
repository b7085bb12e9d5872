// list_host.h -- what the host programs of the list queries (nearest_k_host: points, segments_host: segments) share: the batch as the files hold it and the
// brute and walk operations.  A program gives a traits type T:
//   T::Query                                     the query record as the file holds it, with a radius r
//   T::List                                      the accumulator (closest::NearList, capsule::SegList)
//   T::kLabels                                   labels per query in QLABELS;  T::kBoxOnly: PARAMS ends with i32 box_only (handed to walk)
//   T::setup(list, k, cursor_d2, cursor_id, labels, tri_labels)      labels: the query's kLabels labels, or null
//   T::brute(tri_at, num_tris, query, list)      the definition
//   T::walk(grid, stack, query, list, counts, box_only)              the walk the kernel runs
//   T::record(tri_at, id, d2, query, result)     the 32-byte record of a slot, its last word included
//   <name> brute PARAMS TRIS QUERIES CURSORS QLABELS TLABELS ENTRIES RECORDS
//   <name> walk  PARAMS GRID_ENTRIES CELLS REFS TRIS QUERIES CURSORS QLABELS TLABELS ENTRIES RECORDS COUNTS
// PARAMS: (walk: the grid header of host_support.h,) i32 n, i32 k, i32 cursors given, i32 labels given (, i32 box_only).  A cursor and an entry: {f32 d2, i32 id};
// QLABELS kLabels * n i32, TLABELS 3 i32 per triangle (files that are not given are not read).  ENTRIES: n * k entries; RECORDS: n * k records; COUNTS: n x 4
// i32 (cells visited, triangles tested, pruned, 1 = the list came back full).
#ifndef HAGRID_TESTS_LIST_HOST_H
#define HAGRID_TESTS_LIST_HOST_H

#include <string>
#include <vector>

#include "hagrid/closest.h"
#include "host_support.h"

namespace list_host {

using namespace hagrid;
using namespace host_support;
namespace hc = hagrid::closest;

constexpr int KMAX = 8;
struct Entry { float d2; int32_t id; };
struct Result { float qx, qy, qz, d2; int32_t id, feature; float side, last; };       // last: +0 for a point (the bits of the i32 0 there), s for a segment
static_assert(sizeof(Entry) == 8 && sizeof(Result) == 32, "record layout");

template <typename T>
struct Batch {
    int n, k, box_only;
    std::vector<typename T::Query> queries;
    std::vector<Entry> cursors;
    std::vector<int32_t> qlabels, tlabels;
    std::vector<Entry> entries;
    std::vector<Result> records;

    void load(Params& p, size_t num_tris, const char* query_file, const char* cursor_file, const char* ql_file, const char* tl_file) {
        n = p.get<int32_t>(); k = p.get<int32_t>();
        const bool has_cursors = p.get<int32_t>() != 0, has_labels = p.get<int32_t>() != 0;
        box_only = T::kBoxOnly ? p.get<int32_t>() : 0;
        if (k < 1 || k > KMAX) { fprintf(stderr, "k must be 1 .. %d\n", KMAX); exit(2); }
        queries = read_file<typename T::Query>(query_file);
        if (has_cursors) cursors = read_file<Entry>(cursor_file);
        if (has_labels) { qlabels = read_file<int32_t>(ql_file); tlabels = read_file<int32_t>(tl_file); }
        if (int(queries.size()) != n || (has_cursors && int(cursors.size()) != n) || (has_labels && (int(qlabels.size()) != T::kLabels * n || tlabels.size() != 3 * num_tris))) {
            fprintf(stderr, "the files do not hold n queries, n cursors, %d n query labels or 3 labels per triangle\n", int(T::kLabels)); exit(2);
        }
        entries.resize(size_t(n) * k); records.resize(size_t(n) * k);
    }
    void setup(int i, typename T::List& list) const {
        T::setup(list, k, cursors.empty() ? -1.0f : cursors[i].d2, cursors.empty() ? -1 : cursors[i].id, qlabels.empty() ? nullptr : &qlabels[T::kLabels * size_t(i)],
                 tlabels.empty() ? nullptr : tlabels.data());
    }
    template <typename F>
    void store(int i, const typename T::List& list, F tri_at) {
        for (int j = 0; j < k; j++) {
            Entry& e = entries[size_t(i) * k + j];
            list.get(j, e.id, e.d2);
            T::record(tri_at, e.id, e.d2, queries[i], records[size_t(i) * k + j]);
        }
    }
};

/// the operations brute and walk; -1: op is neither (with this number of files)
template <typename T>
int run(const std::string& op, Params& p, int argc, char** argv) {
    Batch<T> b;
    if (op == "brute" && argc == 10) {
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        b.load(p, tris.size(), argv[4], argv[5], argv[6], argv[7]);
        const Tri* t = tris.data();
        for (int i = 0; i < b.n; i++) {
            typename T::List list;
            b.setup(i, list);
            T::brute([t](int j) { return t[j]; }, int(tris.size()), b.queries[i], list);
            b.store(i, list, [t](int j) { return t[j]; });
        }
        write_file(argv[8], b.entries);
        write_file(argv[9], b.records);
        return 0;
    }
    if (op == "walk" && argc == 14) {
        const GridHeader h = p.get_grid_header();
        HostGrid<kEndUnbounded> g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.tris = read_file<Tri>(argv[6]);
        b.load(p, g.tris.size(), argv[7], argv[8], argv[9], argv[10]);
        std::vector<int32_t> counts(size_t(b.n) * 4);
        hc::ArrayStack<hc::kMaxLevels> st;
        for (int i = 0; i < b.n; i++) {
            typename T::List list;
            hc::Counts c;
            b.setup(i, list);
            T::walk(g, st, b.queries[i], list, c, b.box_only != 0);
            b.store(i, list, [&g](int j) { return g.tri(j); });
            counts[size_t(i) * 4] = c.cells; counts[size_t(i) * 4 + 1] = c.tris; counts[size_t(i) * 4 + 2] = c.pruned; counts[size_t(i) * 4 + 3] = list.full() ? 1 : 0;
        }
        write_file(argv[11], b.entries);
        write_file(argv[12], b.records);
        write_file(argv[13], counts);
        return 0;
    }
    return -1;
}

} // namespace list_host

#endif // HAGRID_TESTS_LIST_HOST_H
