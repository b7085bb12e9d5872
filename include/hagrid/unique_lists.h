// hagrid/unique_lists.h -- segments of (d2, id) entries: sort, unique, compact (hagrid_amd.h: hagrid_unique_lists, hagrid_compact_lists).  The second
// stage of the ball lists (closest.h: "the whole ball"): the walk leaves REFERENCES, one per visit of a cell that lists the triangle; this makes the sorted,
// duplicate-free list out of them.  It needs no grid and knows no query shape.  No counterpart in the reference.
//
// The same functions serve the gfx950 kernel (hagrid_amd/csrc/ball_lists.hip) and host programs (tests/cpp/ball_lists_host.cpp); hagrid_amd/scene.py
// (unique_lists, compact_lists) states the same in numpy and gives the same bits.
//
// ---- an entry ---------------------------------------------------------------------------------------------------------------------
// 8 bytes: float d2, int id -- the entry of hagrid_nearest_tris.  The EMPTY entry is (+inf, -1).  An entry is VALID when id >= 0 and d2 is not NaN.
// The order is (d2 by FLOAT comparison, id): -0.0 and +0.0 are the same distance, the id decides between them; the d2 BITS travel unchanged.
//
// ---- a segment (the room rule of hagrid_list_crossings, crossings.h slot_range) ------------------------------------------------------
// Segment i is the slots [offsets[i], offsets[i + 1]) of `capacity` slots; its room is the range's length, and 0 if that is negative or the range leaves
// [0, capacity].  Nothing outside a segment is read or written.
//
// ---- unique -----------------------------------------------------------------------------------------------------------------------
// In place: the valid entries of the segment, sorted, entries EQUAL IN ID reduced to one, stand at its front; every other slot holds EMPTY; the count is
// how many survive.  The contract: equal ids in one segment carry equal d2 bits (closest.h guarantees it: d2 is point_tri's of the same point and
// triangle).  Then equal ids are neighbours after the sort and the result does not depend on how the sort orders equal keys.
//
// ---- the sort ---------------------------------------------------------------------------------------------------------------------
// A bitonic network for ARBITRARY n in which every compare-exchange puts the smaller entry at the LOWER index (network_pair below): for k = 2, 4, 8, ...
// while k / 2 < n: one FLIP step (i against i ^ (k - 1) inside blocks of k), then steps j = k / 4, k / 8, ..., 1 (i against i ^ j).  Think of the array as
// padded to a power of two with entries larger than all others: a pad is never moved down, because the larger entry always goes up and a pad is already
// above -- so a pair whose upper index is >= n is skipped and the pad is never materialised.  The pairs of one step are disjoint: they run in any order, on
// any number of lanes, with one barrier between steps.  (n log^2 n / 4 compare-exchanges, in place, no scratch: why it serves segments of any length.)
//
// ---- compact ----------------------------------------------------------------------------------------------------------------------
// Copies the first min(counts[i], room of the source, room of the destination) entries of source segment i to destination segment i and fills the rest of
// the destination's room with EMPTY (a negative count copies nothing).
#ifndef HAGRID_UNIQUE_LISTS_H
#define HAGRID_UNIQUE_LISTS_H

#include <stdint.h>

#include "common.h"

namespace hagrid {
namespace lists {

struct Entry { float d2; int32_t id; };

HOST DEVICE inline Entry empty_entry() {
    Entry e;
    e.d2 = __builtin_inff(); e.id = -1;
    return e;
}
HOST DEVICE inline bool valid(const Entry& e) { return e.id >= 0 && e.d2 == e.d2; }
/// what the sort sees of an entry: itself when valid, else EMPTY (which sorts behind every valid entry: +inf, and -1 as the largest unsigned id)
HOST DEVICE inline Entry canonical(const Entry& e) { return valid(e) ? e : empty_entry(); }
/// a sorts strictly before b (canonical entries)
HOST DEVICE inline bool before(const Entry& a, const Entry& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && uint32_t(a.id) < uint32_t(b.id)); }

/// the room rule
HOST DEVICE inline void segment_range(const long long* offsets, long long capacity, long long i, long long& first, long long& room) {
    first = 0; room = 0;
    const long long b = offsets[i], e = offsets[i + 1];
    if (b >= 0 && e >= b && e <= capacity) { first = b; room = e - b; }
}

/// Pair t (0 <= t < P / 2, P the power of two >= n) of one step of the network: its lower and upper index.  flip: the first step of stage k (width = k);
/// otherwise the step at distance j (width = 2 j).  The pair takes part when hi < n.
HOST DEVICE inline void network_pair(long long t, long long width, bool flip, long long& lo, long long& hi) {
    const long long half = width >> 1, low = t & (half - 1);
    lo = ((t - low) << 1) | low;
    hi = flip ? (lo - low) + (width - 1 - low) : lo + half;
}

/// the whole network over n entries, one pair after another.  A: get(i) -> Entry, set(i, Entry)
template <typename A>
HOST DEVICE inline void network_sort(A& a, long long n) {
    long long P = 1;
    while (P < n) P <<= 1;
    for (long long k = 2; (k >> 1) < n; k <<= 1) {
        for (long long w = k; w >= 2; w >>= 1) {
            for (long long t = 0; t < (P >> 1); t++) {
                long long lo, hi;
                network_pair(t, w, w == k, lo, hi);
                if (hi >= n) continue;
                const Entry x = a.get(lo), y = a.get(hi);
                if (before(y, x)) { a.set(lo, y); a.set(hi, x); }
            }
        }
    }
}

/// the definition of unique over one segment of `room` slots.  A: get(i), set(i, Entry) with i relative to the segment.  Returns the count.
template <typename A>
HOST DEVICE inline long long unique_segment(A& a, long long room) {
    for (long long i = 0; i < room; i++) a.set(i, canonical(a.get(i)));
    network_sort(a, room);
    long long m = 0;
    int32_t prev = -1;
    for (long long i = 0; i < room; i++) {
        const Entry e = a.get(i);
        if (e.id < 0) break;                    // EMPTY from here on
        if (e.id != prev) { a.set(m, e); m++; }
        prev = e.id;
    }
    for (long long i = m; i < room; i++) a.set(i, empty_entry());
    return m;
}

/// how many entries compact copies for a segment
HOST DEVICE inline long long compact_count(long long count, long long src_room, long long dst_room) {
    long long c = count < src_room ? count : src_room;
    c = c < dst_room ? c : dst_room;
    return c > 0 ? c : 0;
}

} // namespace lists
} // namespace hagrid

#endif // HAGRID_UNIQUE_LISTS_H
