// gather_tree_main.cpp -- the gather map's tree builder (csrc/pvol_gather_tree.h) as a stand-alone program, so that it can run
// under -fsanitize=address,undefined (test_gather_photons.py).  argv[1] points (default 100 000), a fifth of them duplicates and a
// fifth on a coarse lattice; checks what a lookup relies on: every photon in exactly one node, children inside the array, the
// left child at node + 1, the split value the node's own coordinate, the depth within its bound.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../cs348b-pbrt_amd/csrc/pvol_gather_tree.h"

int main(int argc, char **argv) {
    const uint32_t n = argc > 1 ? (uint32_t)strtoul(argv[1], 0, 10) : 100000u;
    if (n < 1 || n > PVOL_GATHER_MAX_PHOTONS) return 2;
    std::vector<float> p(3 * (size_t)n);
    uint32_t s = 12345u;
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            s = s * 1664525u + 1013904223u;
            float v = (float)(s >> 8) / 16777216.f;
            if (i % 5 == 1) v = (float)((s >> 8) & 7u) / 8.f;
            p[3 * (size_t)i + a] = v;
        }
    for (uint32_t i = 2; i < n; i += 5)
        for (int a = 0; a < 3; ++a) p[3 * (size_t)i + a] = p[3 * (size_t)(i - 2) + a];
    std::vector<GatherNode> nodes(n);
    const int depth = gather_tree_build(p.data(), n, nodes.data());
    int bound = 1;
    for (uint32_t m = n; m > 1; m >>= 1) ++bound;
    if (depth < 1 || depth > bound || depth > PVOL_GATHER_MAX_DEPTH) { printf("depth %d bound %d\n", depth, bound); return 1; }
    std::vector<unsigned char> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const GatherNode &N = nodes[i];
        if (N.index >= n || seen[N.index]++) { printf("node %u: index\n", i); return 1; }
        for (int a = 0; a < 3; ++a) if (N.p[a] != p[3 * (size_t)N.index + a]) { printf("node %u: position\n", i); return 1; }
        if (N.splitAxis > 3 || (N.hasLeftChild && i + 1 >= n) || (N.rightChild != PVOL_GATHER_NO_CHILD && (N.rightChild >= n || N.rightChild <= i))) {
            printf("node %u: children\n", i);
            return 1;
        }
        if (N.splitAxis < 3 && N.splitPos != N.p[N.splitAxis]) { printf("node %u: split\n", i); return 1; }
        if (N.splitAxis == 3 && (N.hasLeftChild || N.rightChild != PVOL_GATHER_NO_CHILD)) { printf("node %u: leaf\n", i); return 1; }
    }
    printf("ok %u points depth %d\n", n, depth);
    return 0;
}
