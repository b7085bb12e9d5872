// hagrid/multi_hit.h -- the list behind multi-hit traversal (hagrid_amd.h: hagrid_traverse_grid_multi): the k nearest
// intersections of one ray, sorted.  No counterpart in the reference, which answers with the nearest hit only.
//
// An INTERSECTION of a ray with triangle j exists exactly when intersect_prim_ray(tri[j], ray, j, h) of prims.h accepts it
// with the ray's OWN tmin and tmax (the window is never shrunk: the nearest-hit walk compares t with abs_det * tmax in the
// scaled domain, so a shrunk window would change which triangles are accepted); its value is h.t.  The list holds the
// min(k, number of intersections) smallest ones in the order (t ascending, then id ascending); unused slots are what a
// miss looks like in traverse_grid: id -1, t = tmax, u = v = 0.  Consequences:
//   - the list for k is a prefix of the list for k + 1;
//   - k = 1 is NOT promised to equal traverse_grid bit for bit: that walk shrinks tmax in the scaled comparison and breaks
//     ties in t by list order, this one by id.
//
// The same struct serves the gfx950 kernel (hagrid_amd/csrc/trav_multi.hip) and a host program (tests/cpp/multi_hit_host.cpp).
// Every loop runs over compile-time indices and is fully unrolled on the device, so the arrays live in registers: a
// register array indexed at run time goes to scratch memory.  The capacity k <= KMAX is a run-time value the same for
// every ray of a launch; it only appears in comparisons with those compile-time indices.
#ifndef HAGRID_MULTI_HIT_H
#define HAGRID_MULTI_HIT_H

#include "ray.h"

#if defined(__clang__)
#define HAGRID_UNROLL _Pragma("unroll")
#define HAGRID_NOUNROLL _Pragma("nounroll")
#else
#define HAGRID_UNROLL
#define HAGRID_NOUNROLL
#endif
#if defined(__HIP_DEVICE_COMPILE__)
/// what is made from x after this line is made HERE: nothing derived from x is computed ahead of a loop and carried through it in registers
#define HAGRID_MADE_HERE(x) asm volatile("" : "+v"(x))
#else
#define HAGRID_MADE_HERE(x)
#endif

namespace hagrid {

template <int KMAX>
struct HitList {
    int id[KMAX];
    float t[KMAX], u[KMAX], v[KMAX];
    int cap;                    ///< k: slots in use, 1 .. KMAX
    int last_id; float last_t;  ///< copy of slot cap - 1: the list is full when last_id >= 0

    /// k empty slots (and KMAX - k that stay empty)
    HOST DEVICE void init(int k, float tmax) {
        cap = k; last_id = -1; last_t = tmax;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) { id[j] = -1; t[j] = tmax; u[j] = 0.0f; v[j] = 0.0f; }
    }

    HOST DEVICE bool full() const { return last_id >= 0; }

    /// (ta, ia) sorts before (tb, ib)
    HOST DEVICE static bool before(float ta, int ia, float tb, int ib) { return ta < tb || (ta == tb && ia < ib); }

    /// An accepted intersection (ht, ref).  A triangle is referenced by several cells, so it may arrive again: it is kept once.
    /// A full list takes it only if it sorts before the last entry, which is dropped; a dropped triangle never comes back,
    /// because the last entry only ever decreases.  Returns whether the list changed.
    HOST DEVICE bool insert(float ht, int ref, float hu, float hv) {
        if (last_id >= 0 && !before(ht, ref, last_t, last_id)) return false;       // cheap early-out: cannot change the list
        bool dup = false;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) dup = dup || id[j] == ref;
        if (dup) return false;
        // the new entry sinks to its sorted place, pushing the rest one slot down; what falls off slot cap - 1 is dropped
        int ci = ref; float ct = ht, cu = hu, cv = hv;
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++) {
            const bool take = j < cap && (id[j] < 0 || before(ct, ci, t[j], id[j]));
            const int oi = id[j]; const float ot = t[j], ou = u[j], ov = v[j];
            id[j] = take ? ci : oi; t[j] = take ? ct : ot; u[j] = take ? cu : ou; v[j] = take ? cv : ov;
            ci = take ? oi : ci; ct = take ? ot : ct; cu = take ? ou : cu; cv = take ? ov : cv;
        }
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++)
            if (j == cap - 1) { last_id = id[j]; last_t = t[j]; }
        return true;
    }

    /// slots 0 .. cap - 1 to out[0 .. cap - 1]
    HOST DEVICE void store(Hit* out) const {
        HAGRID_UNROLL
        for (int j = 0; j < KMAX; j++)
            if (j < cap) out[j] = Hit(id[j], t[j], u[j], v[j]);
    }
};

} // namespace hagrid

#endif // HAGRID_MULTI_HIT_H
