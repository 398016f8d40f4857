// heap_probe.cpp -- what the C++ library in use really does with the two things the gather's exactness rests on:
// the layout std::make_heap / std::pop_heap / std::push_heap leave an array in, and the node order a median-split kd-tree gets from
// std::nth_element under a strict total order.  Stand-alone; test_gather_photons.py compiles it, feeds it cases on stdin and holds
// tests/gather_ref.py against what it prints.
//
// stdin, whitespace separated:
//   H k m  then m pairs  <d2 as fp32 bit pattern> <id>     -> the k-nearest process over the sequence; prints "bits id" per slot
//   T n    then n triples of fp32 bit patterns (x y z)     -> the tree; prints "index axis hasLeft rightChild" per node
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Close {
    float d2;
    uint32_t id;
    bool operator<(const Close &o) const { return d2 == o.d2 ? id < o.id : d2 < o.d2; }
};

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static void heap_case(uint32_t k, uint32_t m) {
    std::vector<Close> buf(k);
    uint32_t found = 0;
    float md2 = from_bits(0x7f800000u);
    for (uint32_t i = 0; i < m; ++i) {
        uint32_t bits, id;
        if (scanf("%u %u", &bits, &id) != 2) return;
        Close c = {from_bits(bits), id};
        if (!(c.d2 < md2)) continue;
        if (found < k) {
            buf[found++] = c;
            if (found == k) { std::make_heap(buf.begin(), buf.end()); md2 = buf[0].d2; }
        } else {
            std::pop_heap(buf.begin(), buf.end());
            buf[k - 1] = c;
            std::push_heap(buf.begin(), buf.end());
            md2 = buf[0].d2;
        }
    }
    printf("%u", found);
    for (uint32_t i = 0; i < found; ++i) printf(" %u %u", to_bits(buf[i].d2), buf[i].id);
    printf("\n");
}

struct TreeOut { uint32_t index, axis, hasLeft, right; };
struct TreeBuild {
    std::vector<float> p;
    std::vector<uint32_t> order;
    std::vector<TreeOut> nodes;
    uint32_t nextFree;
    void build(uint32_t node, uint32_t start, uint32_t end) {
        if (start + 1 == end) { nodes[node] = TreeOut{order[start], 3u, 0u, (1u << 29) - 1u}; return; }
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = p[3 * order[start] + a];
        for (uint32_t i = start; i < end; ++i)
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[3 * order[i] + a]); hi[a] = std::max(hi[a], p[3 * order[i] + a]); }
        const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
        const int axis = (ex > ey && ex > ez) ? 0 : (ey > ez ? 1 : 2);
        const uint32_t mid = (start + end) / 2;
        const float *pp = p.data();
        std::nth_element(order.begin() + start, order.begin() + mid, order.begin() + end, [pp, axis](uint32_t a, uint32_t b) {
            return pp[3 * a + axis] == pp[3 * b + axis] ? a < b : pp[3 * a + axis] < pp[3 * b + axis];
        });
        nodes[node] = TreeOut{order[mid], (uint32_t)axis, 0u, (1u << 29) - 1u};
        if (start < mid) { nodes[node].hasLeft = 1; build(nextFree++, start, mid); }
        if (mid + 1 < end) { const uint32_t r = nextFree++; nodes[node].right = r; build(r, mid + 1, end); }
    }
};

static void tree_case(uint32_t n) {
    TreeBuild t;
    t.p.resize(3 * (size_t)n); t.order.resize(n); t.nodes.resize(n); t.nextFree = 1;
    for (size_t i = 0; i < 3 * (size_t)n; ++i) {
        uint32_t bits;
        if (scanf("%u", &bits) != 1) return;
        t.p[i] = from_bits(bits);
    }
    for (uint32_t i = 0; i < n; ++i) t.order[i] = i;
    if (n) t.build(0, 0, n);
    printf("%u", n);
    for (uint32_t i = 0; i < n; ++i) printf(" %u %u %u %u", t.nodes[i].index, t.nodes[i].axis, t.nodes[i].hasLeft, t.nodes[i].right);
    printf("\n");
}

int main() {
    char kind;
    uint32_t a, b;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'H') { if (scanf("%u %u", &a, &b) != 2) return 1; heap_case(a, b); }
        else if (kind == 'T') { if (scanf("%u", &a) != 1) return 1; tree_case(a); }
        else return 1;
    }
    return 0;
}
