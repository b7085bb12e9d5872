// ball_lists.hip -- ball lists: EVERY triangle within r of each point, sorted, in CSR form, without paging (include/hagrid_amd.h: hagrid_ball_refs,
// hagrid_unique_lists, hagrid_compact_lists; the accumulator and why a constant bound keeps the walk sound: include/hagrid/closest.h, "the whole ball"; the
// segments, the sort and its network: include/hagrid/unique_lists.h).  No counterpart in the reference.
//
// The protocol is hagrid_list_crossings': count -> scan -> fill, then unique -> scan -> compact.  Both scans are the caller's and so is every buffer: no entry
// point here asks for memory.
//
// ball_refs_kernel is nearest_tris_kernel (closest.hip) with the header's RefSink as its accumulator: one query per lane, one wavefront per workgroup, the
// XCD-aware block -> range map, the LDS stack [level][lane], streaming loads and stores.  The sink prunes at r2 for the whole walk and stores every accepted
// offer -- a REFERENCE, one per visit of a cell that lists the triangle -- as one streaming 8-byte word while the query's room lasts.  Count mode and fill
// mode, Cell and SmallCell grids: launch-uniform arguments of ONE kernel (the product library's kernel budget, tests/test_abi.py).
//
// unique_lists_kernel needs no grid.  A workgroup of four wavefronts takes 64 consecutive segments; every wavefront reads all 64 ranges (one coalesced
// load) and so knows the same three classes:
//   room <= 1          the segment's own lane of wavefront 0 answers it (empty and one-entry lists dominate sparse batches);
//   room <= kSortCap   ONE wavefront sorts it in its 8 KB of LDS (the header's network, a wave barrier between steps), drops the duplicates with a ballot
//                      per 64 entries and writes the survivors and the padding back; the four wavefronts take these segments in turn;
//   room >  kSortCap   the WHOLE workgroup runs the same network in place over global memory, a workgroup barrier between steps (no scratch: why lists of
//                      any length come out right); wavefront 0 then drops the duplicates in place, 64 entries at a time, front to back.
// hagrid_compact_lists is a launch-uniform mode of the same kernel: the four wavefronts copy the segments' fronts in turn, 64 entries per step.
#include "trav_common.h"
#include "wave_prims.h"

#include "hagrid/closest.h"
#include "hagrid/crossings.h"
#include "hagrid/unique_lists.h"

using namespace hagrid;
using namespace hagrid_impl;
using namespace hagrid_trav;
namespace hc = hagrid::closest;
namespace hl = hagrid::lists;

namespace {

constexpr int kSortCap = 1024;          // entries a wavefront sorts in LDS (8 KB; four wavefronts per workgroup: 32 KB, 20 wavefronts per CU by LDS)
constexpr int kSegsPerBlock = 64;
constexpr int kUniqueBlock = 256;

struct BallArgs {
    const float4* __restrict__ queries;
    const int* __restrict__ query_labels;
    const int* __restrict__ tri_labels;
    const long long* __restrict__ offsets;      // null: count mode
    int* __restrict__ counts;                   // may be null in fill mode
    float2* __restrict__ entries;
    long long capacity;
    unsigned long long* __restrict__ counters;
    int n;
};

// RefSink's store: the query's first slot is made before the walk and carried through it (two registers)
struct RefStore {
    float2* slots;
    __device__ __forceinline__ void operator()(int position, float d2, int id) const { nt_store2(slots + position, d2, __int_as_float(id)); }
};

// the range of query i: crossings.h's slot_range in its CSR form -- the room rule is hagrid_list_crossings', word for word
__device__ __forceinline__ void hx_range(const BallArgs& a, int i, long long& first, long long& room) { hagrid::crossings::slot_range(a.offsets, 0, a.capacity, i, first, room); }

__global__ void __launch_bounds__(64) ball_refs_kernel(const DevGrid g, const BallArgs a) {
    __shared__ uint32_t s_w[hc::kMaxLevels][64], s_i[hc::kMaxLevels][64];
    const int lane = threadIdx.x;
    const int id = xcd_split(blockIdx.x, gridDim.x) * 64 + lane;
    const bool live = id < a.n;
    hc::Counts cnt;
    cnt.cells = 0; cnt.tris = 0; cnt.pruned = 0;
    int written = 0, is_short = 0;
    if (live) {
        const float4 pr = nt_load4(a.queries + id);
        const vec3 p(pr.x, pr.y, pr.z);
        LdsStack st;
        st.w_ = &s_w[0][lane]; st.i_ = &s_i[0][lane];
        long long first = 0, room = 0;
        if (a.offsets) hx_range(a, id, first, room);
        hc::RefSink<RefStore> sink;
        sink.store.slots = a.entries + first;
        sink.setup(int(room < 0x7fffffffLL ? room : 0x7fffffffLL), a.query_labels ? a.query_labels[id] : -1, a.tri_labels);
        hc::closest_query(g, st, p, pr.w, sink, cnt);
        const int refs = sink.count;
        if (a.counts) __builtin_nontemporal_store(refs, a.counts + id);
        if (a.offsets) {            // the slots the references left over get the empty entry
            written = refs < sink.room ? refs : sink.room;
            is_short = refs > sink.room ? 1 : 0;
            int again = id;
            HAGRID_MADE_HERE(again);         // the range once more, from the query's number (as crossings.hip)
            hx_range(a, again, first, room);
            const hl::Entry none = hl::empty_entry();
            for (long long s = written; s < room; s++) nt_store2(a.entries + first + s, none.d2, __int_as_float(none.id));
        }
    }
    if (a.counters) {
        add_batch_counters(a.counters, lane, live ? 1 : 0, cnt.cells, cnt.tris, cnt.pruned);
        const unsigned long long sw = wave_sum_u64((unsigned)written), ss = wave_sum_u64((unsigned)is_short);
        if (lane == 0) { atomicAdd(a.counters + 4, sw); atomicAdd(a.counters + 5, ss); }
    }
}

// ---- unique and compact --------------------------------------------------------------------------------------------------------------

struct UniqueArgs {
    const long long* __restrict__ offsets;
    float2* entries;                            // unique: sorted in place; compact: the source
    long long capacity;
    int* counts;                                // unique: out; compact: in
    const long long* __restrict__ out_offsets;  // compact only
    float2* out_entries;
    long long out_capacity;
    unsigned long long* __restrict__ counters;
    int n, compact;
};

__device__ __forceinline__ hl::Entry load_entry(const float2* p) { const float2 v = *p; hl::Entry e; e.d2 = v.x; e.id = __float_as_int(v.y); return e; }
__device__ __forceinline__ void store_entry(float2* p, const hl::Entry& e) { *p = make_float2(e.d2, __int_as_float(e.id)); }
// LDS traffic of one wavefront is served in issue order; this keeps the compiler from moving accesses across a step of the network
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ long long shfl_ll(long long v, int src) {
    const int lo = __shfl(int(v), src, 64), hi = __shfl(int(v >> 32), src, 64);
    return (long long)(unsigned)lo | ((long long)hi << 32);
}
__device__ __forceinline__ long long pow2_at_least(long long n) { long long P = 1; while (P < n) P <<= 1; return P; }

// one segment of n <= kSortCap slots by one wavefront: LDS sort, duplicates dropped on the way back.  Returns the count.
__device__ __forceinline__ int unique_in_lds(float2* s, float2* g, int n, int lane) {
    for (int i = lane; i < n; i += 64) store_entry(s + i, hl::canonical(load_entry(g + i)));
    wave_sync();
    const int P = int(pow2_at_least(n));
    for (int k = 2; (k >> 1) < n; k <<= 1) {
        for (int w = k; w >= 2; w >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                long long lo, hi;
                hl::network_pair(t, w, w == k, lo, hi);
                if (hi < n) {
                    const hl::Entry x = load_entry(s + lo), y = load_entry(s + hi);
                    if (hl::before(y, x)) { store_entry(s + lo, y); store_entry(s + hi, x); }
                }
            }
            wave_sync();
        }
    }
    int m = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const hl::Entry e = i < n ? load_entry(s + i) : hl::empty_entry();
        const int prev = (i > 0 && i < n) ? load_entry(s + i - 1).id : -1;
        const bool keep = i < n && e.id >= 0 && e.id != prev;
        const unsigned long long mask = __ballot(keep);
        if (keep) store_entry(g + m + __popcll(mask & ((1ull << lane) - 1ull)), e);
        m += __popcll(mask);
        if (__ballot(i < n && e.id >= 0) == 0ull) break;          // EMPTY from here on
    }
    const hl::Entry none = hl::empty_entry();
    for (int i = m + lane; i < n; i += 64) store_entry(g + i, none);
    return m;
}

// one segment of any length by the whole workgroup, in place over global memory.  s_ml: one LDS word.  Returns the count (in every thread).
__device__ __forceinline__ long long unique_in_place(float2* g, long long n, long long* s_ml) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (long long i = tid; i < n; i += kUniqueBlock) {
        const hl::Entry e = load_entry(g + i);
        if (!hl::valid(e)) store_entry(g + i, hl::empty_entry());
    }
    __syncthreads();
    const long long P = pow2_at_least(n);
    for (long long k = 2; (k >> 1) < n; k <<= 1) {
        for (long long w = k; w >= 2; w >>= 1) {
            for (long long t = tid; t < (P >> 1); t += kUniqueBlock) {
                long long lo, hi;
                hl::network_pair(t, w, w == k, lo, hi);
                if (lo >= n) break;                                // lo grows with t
                if (hi < n) {
                    const hl::Entry x = load_entry(g + lo), y = load_entry(g + hi);
                    if (hl::before(y, x)) { store_entry(g + lo, y); store_entry(g + hi, x); }
                }
            }
            __syncthreads();
        }
    }
    if (tid < 64) {                 // wavefront 0: the survivors move to the front, 64 entries at a time; a chunk is read whole before any of it is written
        long long m = 0;
        int carried = -1;           // the id before the chunk
        for (long long i0 = 0; i0 < n; i0 += 64) {
            const long long i = i0 + lane;
            const hl::Entry e = i < n ? load_entry(g + i) : hl::empty_entry();
            const int up = __shfl_up(e.id, 1, 64);
            const int prev = lane == 0 ? carried : up;
            carried = __shfl(e.id, 63, 64);
            const bool keep = i < n && e.id >= 0 && e.id != prev;
            const unsigned long long mask = __ballot(keep);
            if (keep) store_entry(g + m + __popcll(mask & ((1ull << lane) - 1ull)), e);
            m += __popcll(mask);
            if (__ballot(i < n && e.id >= 0) == 0ull) break;
        }
        if (lane == 0) *s_ml = m;
    }
    __syncthreads();
    const long long m = *s_ml;
    const hl::Entry none = hl::empty_entry();
    for (long long i = m + tid; i < n; i += kUniqueBlock) store_entry(g + i, none);
    __syncthreads();                // s_ml is free for the next segment
    return m;
}

__global__ void __launch_bounds__(kUniqueBlock) unique_lists_kernel(const UniqueArgs a) {
    __shared__ float2 s_e[kUniqueBlock / 64][kSortCap];
    __shared__ long long s_ml;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long seg = (long long)blockIdx.x * kSegsPerBlock + lane;        // the same in every wavefront
    const bool live = seg < a.n;
    long long first = 0, room = 0;
    if (live) hl::segment_range(a.offsets, a.capacity, seg, first, room);
    unsigned long long c1 = 0, c2 = 0, c3 = 0;      // per lane: what the counters get beside the number of segments

    if (a.compact) {
        long long dfirst = 0, droom = 0, copy = 0;
        if (live) {
            hl::segment_range(a.out_offsets, a.out_capacity, seg, dfirst, droom);
            const int cnt = a.counts[seg];
            copy = hl::compact_count(cnt, room, droom);
            if (wave == 0) { c1 = (unsigned long long)copy; c2 = cnt > copy ? 1 : 0; }
        }
        const hl::Entry none = hl::empty_entry();
        int turn = 0;
        for (unsigned long long todo = __ballot(droom > 0); todo; todo &= todo - 1ull, turn++) {
            if ((turn & 3) != wave) continue;
            const int src = __ffsll((long long)todo) - 1;
            const float2* from = a.entries + shfl_ll(first, src);
            float2* to = a.out_entries + shfl_ll(dfirst, src);
            const long long cp = shfl_ll(copy, src), dr = shfl_ll(droom, src);
            for (long long i = lane; i < dr; i += 64) {
                const hl::Entry e = i < cp ? load_entry(from + i) : none;
                nt_store2(to + i, e.d2, __int_as_float(e.id));
            }
        }
    } else {
        // room <= 1: the segment's own lane
        if (live && wave == 0) {
            int m = 0;
            if (room == 1) {
                const hl::Entry e = load_entry(a.entries + first);
                m = hl::valid(e) ? 1 : 0;
                if (!m) store_entry(a.entries + first, hl::empty_entry());
            }
            if (room <= 1) { a.counts[seg] = m; c2 = (unsigned long long)m; }
            c1 = (unsigned long long)room;
        }
        // room <= kSortCap: a wavefront each, in turn
        int turn = 0;
        for (unsigned long long todo = __ballot(room >= 2 && room <= kSortCap); todo; todo &= todo - 1ull, turn++) {
            if ((turn & 3) != wave) continue;
            const int src = __ffsll((long long)todo) - 1;
            const int m = unique_in_lds(s_e[wave], a.entries + shfl_ll(first, src), int(shfl_ll(room, src)), lane);
            if (lane == 0) { a.counts[(long long)blockIdx.x * kSegsPerBlock + src] = m; c2 += (unsigned long long)m; }
        }
        // longer: the workgroup (the mask is the same in every wavefront: the loop is uniform over the workgroup)
        for (unsigned long long todo = __ballot(room > kSortCap); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const long long m = unique_in_place(a.entries + shfl_ll(first, src), shfl_ll(room, src), &s_ml);
            if (threadIdx.x == 0) { a.counts[(long long)blockIdx.x * kSegsPerBlock + src] = int(m < 0x7fffffffLL ? m : 0x7fffffffLL); c2 += (unsigned long long)m; c3 += 1; }
        }
    }
    if (a.counters) {
        const unsigned long long s0 = wave_sum_u64(live && wave == 0 ? 1ull : 0ull), s1 = wave_sum_u64(c1), s2 = wave_sum_u64(c2), s3 = wave_sum_u64(c3);
        if (lane == 0) {
            if (s0) atomicAdd(a.counters + 0, s0);
            if (s1) atomicAdd(a.counters + 1, s1);
            if (s2) atomicAdd(a.counters + 2, s2);
            if (s3) atomicAdd(a.counters + 3, s3);
        }
    }
}

int check_segments(hagrid_ctx* ctx, const std::string& w, int num_lists, const void* offsets, const void* entries, int64_t capacity, const void* counts, const void* counters,
                   uint32_t flags) {
    if (flags) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": unknown flag (flags must be 0)").c_str());
    if (num_lists < 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": negative num_lists").c_str());
    if (capacity < 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": negative capacity").c_str());
    if (!aligned(counters, 8) || !aligned(offsets, 8) || !aligned(entries, 8)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": counters, offsets and entries must be 8-byte aligned").c_str());
    if (!aligned(counts, 4)) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": counts must be 4-byte aligned").c_str());
    if (num_lists == 0) return HAGRID_OK;
    if (!offsets || !counts) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null offsets or counts").c_str());
    if (!entries && capacity > 0) HG_FAIL(ctx, HAGRID_EINVAL, (w + ": null entries with a capacity").c_str());
    return HAGRID_OK;
}

int launch_unique(hagrid_ctx* ctx, const UniqueArgs& a) {
    HG_HIP(ctx, hipSetDevice(ctx->device));
    unique_lists_kernel<<<grid_blocks(a.n, kSegsPerBlock), kUniqueBlock, 0, ctx->stream>>>(a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

} // namespace

extern "C" int hagrid_ball_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, int num_points, const void* query_labels, const void* tri_labels,
                                const void* offsets, void* counts, void* entries, int64_t capacity, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    if (flags) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: unknown flag (flags must be 0)");
    if (num_points < 0) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: negative num_points");
    if (capacity < 0) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: negative capacity");
    HG_TRY(check_walk_grid(ctx, "ball_refs", grid));
    if (!offsets && (entries || capacity != 0)) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: count mode (offsets == NULL) takes no entries and a capacity of 0");
    if ((query_labels != nullptr) != (tri_labels != nullptr)) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: query_labels and tri_labels are given together or not at all");
    if (!aligned(counters, 8) || !aligned(offsets, 8) || !aligned(entries, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: counters, offsets and entries must be 8-byte aligned");
    if (!aligned(counts, 4) || !aligned(query_labels, 4) || !aligned(tri_labels, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: counts and labels must be 4-byte aligned");
    if (!aligned(tris, 16) || !aligned(points, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: triangles and points must be 16-byte aligned");
    if (num_points == 0) return HAGRID_OK;
    if (!tris || !points) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: null triangle or point buffer");
    if (!offsets && !counts) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: count mode needs counts");
    if (offsets && !entries && capacity > 0) HG_FAIL(ctx, HAGRID_EINVAL, "ball_refs: null output buffer");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    DevGrid g;
    g.set(grid, tris);
    BallArgs a;
    a.queries = static_cast<const float4*>(points);
    a.query_labels = static_cast<const int*>(query_labels); a.tri_labels = static_cast<const int*>(tri_labels);
    a.offsets = static_cast<const long long*>(offsets); a.counts = static_cast<int*>(counts);
    a.entries = static_cast<float2*>(entries); a.capacity = capacity;
    a.counters = static_cast<unsigned long long*>(counters);
    a.n = num_points;
    ball_refs_kernel<<<grid_blocks(num_points, 64), 64, 0, ctx->stream>>>(g, a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_unique_lists(hagrid_ctx* ctx, int num_lists, const void* offsets, void* entries, int64_t capacity, void* counts, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    HG_TRY(check_segments(ctx, "unique_lists", num_lists, offsets, entries, capacity, counts, counters, flags));
    if (num_lists == 0) return HAGRID_OK;
    UniqueArgs a = {};
    a.offsets = static_cast<const long long*>(offsets); a.entries = static_cast<float2*>(entries); a.capacity = capacity;
    a.counts = static_cast<int*>(counts); a.counters = static_cast<unsigned long long*>(counters);
    a.n = num_lists;
    return launch_unique(ctx, a);
}

extern "C" int hagrid_compact_lists(hagrid_ctx* ctx, int num_lists, const void* offsets, const void* entries, int64_t capacity, const void* counts, const void* out_offsets,
                                    void* out_entries, int64_t out_capacity, void* counters, uint32_t flags) {
    if (!ctx) return HAGRID_EINVAL;
    HG_TRY(check_segments(ctx, "compact_lists", num_lists, offsets, entries, capacity, counts, counters, flags));
    if (out_capacity < 0) HG_FAIL(ctx, HAGRID_EINVAL, "compact_lists: negative out_capacity");
    if (!aligned(out_offsets, 8) || !aligned(out_entries, 8)) HG_FAIL(ctx, HAGRID_EINVAL, "compact_lists: out_offsets and out_entries must be 8-byte aligned");
    if (num_lists == 0) return HAGRID_OK;
    if (!out_offsets) HG_FAIL(ctx, HAGRID_EINVAL, "compact_lists: null out_offsets");
    if (!out_entries && out_capacity > 0) HG_FAIL(ctx, HAGRID_EINVAL, "compact_lists: null out_entries with a capacity");
    UniqueArgs a = {};
    a.offsets = static_cast<const long long*>(offsets); a.entries = const_cast<float2*>(static_cast<const float2*>(entries)); a.capacity = capacity;
    a.counts = const_cast<int*>(static_cast<const int*>(counts));
    a.out_offsets = static_cast<const long long*>(out_offsets); a.out_entries = static_cast<float2*>(out_entries); a.out_capacity = out_capacity;
    a.counters = static_cast<unsigned long long*>(counters);
    a.n = num_lists; a.compact = 1;
    return launch_unique(ctx, a);
}
