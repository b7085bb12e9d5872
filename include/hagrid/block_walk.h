// hagrid/block_walk.h -- the descent through the sub-blocks of one top-level cell of the construction format (entries -> cells | small_cells -> ref_ids),
// written once: the counterpart of cell_walk.h for the queries about a REGION.  A ray follows one voxel after another (cell_walk.h); a region query visits every
// sub-block of the voxel map that its region may reach, depth first, and leaves out the blocks its own predicate refuses.
//
// Who runs it: nearest-surface queries (closest.h: blocks not farther than the best so far) and box-overlap queries (overlap.h: blocks whose voxel range meets
// the box's), each in its kernel (hagrid_amd/csrc/closest.hip, overlap.hip) over device loads with the stack in LDS, and in the host programs of tests/cpp over
// arrays with bounds checks and an ArrayStack.  Which top-level cells a query visits, and what it does with a top-level cell that is a leaf, is the query's own.
//
// The accessor G:  c (GridConsts), word(i) -> word i of the voxel map, cell(i) -> CellRec, ref(i) -> reference, tri(id) -> Tri.  The driver reads c and word
//                  only; the rest is what the queries' leaf functions read.
// The stack S:     set(level, w, i), set_i(level, i), w(level), i(level): per level the word of the node and the index of its next child.  kMaxLevels levels.
//                  ArrayStack below on the host; the kernels keep theirs in LDS (LdsStack, hagrid_amd/csrc/trav_common.h).
#ifndef HAGRID_BLOCK_WALK_H
#define HAGRID_BLOCK_WALK_H

#include "cell_walk.h"
#include "vec.h"

namespace hagrid {
namespace blocks {

/// walk::WalkConsts set from the TOP-LEVEL resolution (the same operations on the same numbers), and the margin, which only the region queries read
struct GridConsts : walk::WalkConsts {
    float eps;              ///< the absolute margin
    HOST DEVICE void set(const ivec3& top_, int shift_, const vec3& lo_, const vec3& hi_) {
        walk::WalkConsts::set(top_ << shift_, shift_, lo_, hi_);
        eps = abs_margin(lo_, hi_);
    }
    HOST DEVICE static float abs_margin(const vec3& lo_, const vec3& hi_) {
        float m = detail::fabs1(lo_.x);
        m = max(m, detail::fabs1(lo_.y)); m = max(m, detail::fabs1(lo_.z));
        m = max(m, detail::fabs1(hi_.x)); m = max(m, detail::fabs1(hi_.y)); m = max(m, detail::fabs1(hi_.z));
        return m * 1.52587890625e-05f;      // 2^-16
    }
};
using walk::CellRec;         ///< here `end` bounds the list: INT_MAX for a SmallCell (sentinel-terminated); begin < 0: empty

/// A host-side stack for the descent (a run-time indexed array: fine on the host; the kernels keep their stack in LDS)
template <int LEVELS>
struct ArrayStack {
    uint32_t w_[LEVELS], i_[LEVELS];
    void set(int level, uint32_t w, uint32_t i) { w_[level] = w; i_[level] = i; }
    void set_i(int level, uint32_t i) { i_[level] = i; }
    uint32_t w(int level) const { return w_[level]; }
    uint32_t i(int level) const { return i_[level]; }
};
constexpr int kMaxLevels = 16;     ///< every level of the voxel map consumes at least one of the `shift` <= 15 bits

/// The sub-blocks of the top-level cell (tx, ty, tz), whose word top_w says it is no leaf (top_w & 3): depth first, the children of a node by ascending index,
/// a child's own children before its next sibling.  For every sub-block -- 2^s voxels per axis from the voxel (cx, cy, cz) -- prune(cx, cy, cz, s) is asked
/// before the block's word is read: true leaves the block out (and what is below it).  For every leaf word reached leaf(cell index) is called: true ends the
/// descent.  Returns whether a leaf ended it.  A word that is no valid voxel map (more levels than `shift` has bits, deeper than the stack) is passed over.
template <typename G, typename S, typename Prune, typename Leaf>
HOST DEVICE inline bool descend_top(const G& g, S& st, uint32_t top_w, int tx, int ty, int tz, Prune prune, Leaf leaf) {
    int rs = g.c.shift;                                 // the current node covers 2^rs voxels per axis from (ox, oy, oz)
    int ox = tx << rs, oy = ty << rs, oz = tz << rs;
    int level = 0;
    st.set(0, top_w, 0u);
    while (level >= 0) {
        const uint32_t nw = st.w(level), idx = st.i(level);
        const int l = int(nw & 3u);
        if (idx >= (1u << (3 * l))) {                   // this node is done: back to its parent
            level--;
            if (level >= 0) {
                rs += int(st.w(level) & 3u);
                const int keep = ~((1 << rs) - 1);
                ox &= keep; oy &= keep; oz &= keep;
            }
            continue;
        }
        st.set_i(level, idx + 1u);
        const int m = (1 << l) - 1, s = rs - l;
        if (s < 0) continue;                            // not a valid voxel map
        const int cx = ox + ((int(idx) & m) << s), cy = oy + (((int(idx) >> l) & m) << s), cz = oz + ((int(idx) >> (2 * l)) << s);
        if (prune(cx, cy, cz, s)) continue;
        const uint32_t cw = g.word((nw >> 2) + idx);
        if (!(cw & 3u)) {
            if (leaf(cw >> 2)) return true;
        } else if (level + 1 < kMaxLevels) {
            level++;
            st.set(level, cw, 0u);
            rs = s; ox = cx; oy = cy; oz = cz;
        }
    }
    return false;
}

} // namespace blocks

// The names these had while closest.h defined them and overlap.h borrowed them: the queries' own code and programs written against either header keep
// their spelling, whichever of the two headers they include.
namespace closest { using blocks::GridConsts; using blocks::CellRec; using blocks::ArrayStack; using blocks::kMaxLevels; }
namespace overlap { using blocks::GridConsts; using blocks::CellRec; using blocks::ArrayStack; using blocks::kMaxLevels; }
} // namespace hagrid

#endif // HAGRID_BLOCK_WALK_H
