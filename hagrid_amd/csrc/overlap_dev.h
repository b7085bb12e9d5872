// overlap_dev.h -- the device-side accessors of the region queries (include/hagrid/overlap.h, include/hagrid/obb.h), shared by the k-list kernels of
// overlap.hip and the reference kernels of overlap_lists.hip: the grid with its clip box, and the per-lane queries the pair filters read from.
#ifndef HAGRID_AMD_OVERLAP_DEV_H
#define HAGRID_AMD_OVERLAP_DEV_H

#include "trav_common.h"

#include "hagrid/obb.h"
#include "hagrid/overlap.h"

namespace hagrid_trav {

// the accessor of overlap.h: the grid and the clip box
struct OverlapGrid : DevGrid { hagrid::overlap::Clip clip; };

// the query of overlap.h's TriFilter for one lane: the record and the labels are read again for every candidate that has met the box -- few do, the
// lines stay in the vector L1, and nothing of the query but the box is live across the walk
struct DevQuery {
    const float4* __restrict__ queries;      // the launch's arrays (uniform) and this lane's query: addresses are formed where they are used
    const int* __restrict__ labels;          // of the queries, or null
    const int* __restrict__ tri_labels;
    int i;
    __device__ __forceinline__ hagrid::Tri tri() const { return load_tri(queries, i); }
    __device__ __forceinline__ bool labelled() const { return labels != nullptr; }
    __device__ __forceinline__ int label(int j) const { return labels[3 * size_t(i) + j]; }
    __device__ __forceinline__ int tri_label(int id, int j) const { return tri_labels[3 * size_t(id) + j]; }
};

// the pair filter of the launch: nothing for boxes, TriFilter for the contact form (uniform over the launch)
struct DevFilter {
    hagrid::overlap::TriFilter<DevQuery> f;
    bool on;
    __device__ __forceinline__ bool counts_box_tests() const { return !on; }
    __device__ __forceinline__ bool accept(int id, const hagrid::Tri& t, int& tests) const { return !on || f.accept(id, t, tests); }
};

__device__ __forceinline__ hagrid::obb::Obb load_obb(const float4* __restrict__ obbs, int i) {
    using hagrid::vec3;
    const float4* p = obbs + 4 * size_t(i);
    const float4 c = p[0], u = p[1], v = p[2], w = p[3];
    hagrid::obb::Obb b;
    b.c = vec3(c.x, c.y, c.z); b.u = vec3(u.x, u.y, u.z); b.v = vec3(v.x, v.y, v.z); b.w = vec3(w.x, w.y, w.z);
    return b;
}

// the query of obb.h's ObbFilter for one lane
struct DevObb {
    const float4* __restrict__ obbs;
    const int* __restrict__ labels;          // of the queries, or null
    const int* __restrict__ tri_labels;
    int i;
    __device__ __forceinline__ hagrid::obb::Obb box() const {
        int j = i;
        HAGRID_MADE_HERE(j);                  // the record is read HERE, at every use: no load of it is moved ahead of the walk's loops and kept
        return load_obb(obbs, j);
    }
    __device__ __forceinline__ bool labelled() const { return labels != nullptr; }
    __device__ __forceinline__ int label() const { return labels[i]; }
    __device__ __forceinline__ int tri_label(int id, int j) const { return tri_labels[3 * size_t(id) + j]; }
};

} // namespace hagrid_trav

#endif // HAGRID_AMD_OVERLAP_DEV_H
