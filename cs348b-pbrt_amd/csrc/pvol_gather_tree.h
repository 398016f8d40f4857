// pvol_gather_tree.h -- KdTree<Photon>::KdTree / recursiveBuild (core/kdtree.h:99-147) as a pure function: the node array in the
// reference's numbering from the photons' positions.  Plain C++, no HIP: pvol_gather.hip uploads what it returns, the CPU tests
// read it through pvol_gather_tree_build.
//
// Why the result does not depend on the library: CompareNode (kdtree.h:87-94) orders by (p[axis], address in the input vector),
// a strict total order, so std::nth_element's post-condition fixes the median and both sides as SETS; the sub-ranges are
// re-partitioned under their own axis, so the order inside a side never reaches the tree.
#ifndef PVOL_GATHER_TREE_H
#define PVOL_GATHER_TREE_H
#include <stdint.h>
#include <algorithm>
#include <vector>

#define PVOL_GATHER_MAX_PHOTONS (1u << 24)
#define PVOL_GATHER_MAX_DEPTH 25   // floor(log2(2^24)) + 1

// One node, 32 bytes, as the device reads it (two 16-byte loads).  A missing right child is the reference's (1 << 29) - 1,
// which `rightChild < nNodes` (kdtree.h:168) tells from a real one.
struct GatherNode {
    float p[3];            // nodeData[node].p
    float splitPos;        // leaf: 0
    uint32_t splitAxis;    // 3 = leaf
    uint32_t hasLeftChild; // the left child is node + 1
    uint32_t rightChild;
    uint32_t index;        // the photon's index in the caller's order
};
#define PVOL_GATHER_NO_CHILD ((1u << 29) - 1u)

struct GatherTreeBuilder {
    const float *p;
    std::vector<uint32_t> order;   // buildNodes: indices into the caller's arrays
    GatherNode *nodes;
    uint32_t nextFreeNode;
    int depth;

    void build(uint32_t nodeNum, uint32_t start, uint32_t end, int level) {
        depth = std::max(depth, level);
        GatherNode &N = nodes[nodeNum];
        if (start + 1 == end) {   // initLeaf
            const uint32_t i = order[start];
            N.p[0] = p[3 * (size_t)i]; N.p[1] = p[3 * (size_t)i + 1]; N.p[2] = p[3 * (size_t)i + 2];
            N.splitPos = 0.f; N.splitAxis = 3; N.hasLeftChild = 0; N.rightChild = PVOL_GATHER_NO_CHILD; N.index = i;
            return;
        }
        // the bound of the range and BBox::MaximumExtent (core/geometry.h:421-429): x only when strictly the largest, else y
        // when strictly larger than z, else z
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = p[3 * (size_t)order[start] + a];
        for (uint32_t k = start + 1; k < end; ++k)
            for (int a = 0; a < 3; ++a) {
                const float v = p[3 * (size_t)order[k] + a];
                lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v);
            }
        const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        const int axis = (dx > dy && dx > dz) ? 0 : (dy > dz ? 1 : 2);
        const uint32_t mid = (start + end) / 2;
        const float *pp = p;
        std::nth_element(order.begin() + start, order.begin() + mid, order.begin() + end, [pp, axis](uint32_t a, uint32_t b) {
            const float va = pp[3 * (size_t)a + axis], vb = pp[3 * (size_t)b + axis];
            return va == vb ? a < b : va < vb;
        });
        const uint32_t i = order[mid];
        N.p[0] = p[3 * (size_t)i]; N.p[1] = p[3 * (size_t)i + 1]; N.p[2] = p[3 * (size_t)i + 2];
        N.splitPos = N.p[axis]; N.splitAxis = (uint32_t)axis; N.hasLeftChild = 0; N.rightChild = PVOL_GATHER_NO_CHILD; N.index = i;
        if (start < mid) {
            N.hasLeftChild = 1;
            build(nextFreeNode++, start, mid, level + 1);   // always nodeNum + 1
        }
        if (mid + 1 < end) {
            const uint32_t r = nextFreeNode++;
            nodes[nodeNum].rightChild = r;
            build(r, mid + 1, end, level + 1);
        }
    }
};

// The tree over n photons (1 <= n <= 2^24, finite positions p[n][3]) into nodes[n].  Returns its depth, the number of nodes on the
// longest root-to-leaf path: the median split halves a range, so it is at most floor(log2 n) + 1 <= PVOL_GATHER_MAX_DEPTH.
static inline int gather_tree_build(const float *p, uint32_t n, GatherNode *nodes) {
    GatherTreeBuilder b;
    b.p = p; b.nodes = nodes; b.nextFreeNode = 1; b.depth = 0;
    b.order.resize(n);
    for (uint32_t i = 0; i < n; ++i) b.order[i] = i;
    b.build(0, 0, n, 1);
    return b.depth;
}
#endif
