// hagrid/ray_filter.h -- which triangles take part for which ray (hagrid_amd.h: hagrid_traverse_grid_filtered): a visibility mask per
// ray against a mask per triangle, and one triangle the ray does not see at all (the one it starts on, the one it just hit).  No
// counterpart in the reference; the switch is Embree's ray mask, the visibility mask of OptiX / DXR instances and "ignore this primitive".
//
// A filter record is 8 bytes, 8-byte aligned: uint32 mask, int32 skip.  Triangle j TAKES PART for ray i exactly when
//     (mask_i & tri_masks[j]) != 0   and   j != skip_i
// where a missing filter array means mask = kRayMaskAll, skip = -1 for every ray, and a missing mask array means all ones for every
// triangle.  Any negative skip, and a skip that names no triangle, skips nothing: no reference ever equals it.  The answer of a
// filtered query is the answer of the unfiltered one over the scene with the triangles that take no part deleted, ids unchanged.
//
// The same struct serves the gfx950 kernel (hagrid_amd/csrc/trav_multi.hip) and a host program (tests/cpp/filtered_host.cpp), as
// multi_hit.h does.  The order of the two tests is the kernel's: skips() in front of the triangle test (a compare of two registers),
// admits() only for an intersection that was accepted -- those are rare, so the 4-byte gather of tri_masks[ref] is paid for them alone.
#ifndef HAGRID_RAY_FILTER_H
#define HAGRID_RAY_FILTER_H

#include "common.h"

namespace hagrid {

constexpr uint32_t kRayMaskAll = 0xFFFFFFFFu;           ///< HAGRID_RAY_MASK_ALL

struct RayFilter {
    uint32_t mask;
    int32_t skip;

    /// sees everything
    HOST DEVICE RayFilter() : mask(kRayMaskAll), skip(-1) {}
    HOST DEVICE RayFilter(uint32_t mask_, int32_t skip_) : mask(mask_), skip(skip_) {}

    /// record i of the array, or the record that sees everything when there is no array
    HOST DEVICE static RayFilter of(const RayFilter* filters, size_t i) { return filters ? filters[i] : RayFilter(); }

    /// a ray whose mask is zero sees no triangle whatever the triangles' masks are: it takes no cell step
    HOST DEVICE bool walks() const { return mask != 0u; }
    /// in front of the triangle test (references are >= 0, so a negative skip matches none)
    HOST DEVICE bool skips(int ref) const { return ref == skip; }
    /// for an accepted intersection with triangle ref; tri_masks may be null (all ones)
    HOST DEVICE bool admits(const uint32_t* tri_masks, int ref) const { return (mask & (tri_masks ? tri_masks[ref] : kRayMaskAll)) != 0u; }
};

static_assert(sizeof(RayFilter) == 8, "a filter record is 8 bytes: uint32 mask, int32 skip");

} // namespace hagrid

#endif // HAGRID_RAY_FILTER_H
