// levels_check: tpt_wide_tree_levels (host/wide_bvh.cpp) under ASan + UBSan, CPU only.  Trees of
// tpt_wide_tree_build over random boxes: the level ranges partition the nodes and every inner child
// of level l lies in level l + 1, with a buffer of exactly the size asked for; then the same trees
// with links overwritten by arbitrary words, which must be refused or answered without reading
// outside the node array.  Prints "ok" and returns 0.  Built by levels_check.mk beside it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "tpt.h"

static int fail(const char* what, int n) {
    std::printf("FAILED: %s (n = %d)\n", what, n);
    return 1;
}

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> pos(-10.0f, 10.0f), ext(0.0f, 1.0f);
    const int sizes[] = {2, 3, 5, 17, 130, 2000, 20000};
    for (int n : sizes) {
        std::vector<float> box(6 * (size_t)n);
        std::vector<uint32_t> emit(n);
        for (int p = 0; p < n; ++p) {
            for (int k = 0; k < 3; ++k) {
                const float c = pos(rng), h = ext(rng);
                box[6 * p + k] = c - h;
                box[6 * p + 3 + k] = c + h;
            }
            emit[p] = rng() % 3 == 0;
        }
        std::vector<float> nodes(32 * (size_t)(n - 1));
        int32_t need = 0;
        const int32_t n4 = tpt_wide_tree_build(n, box.data(), emit.data(), nodes.data(), n - 1, &need, 2);
        if (n4 < 1 || n4 > n - 1) return fail("tpt_wide_tree_build", n);
        const int32_t lv = tpt_wide_tree_levels(nodes.data(), n4, 0, nullptr, 0);
        if (lv < 1) return fail("level count", n);
        std::vector<int32_t> begin((size_t)lv + 1, -1);   // exactly the size asked for
        if (tpt_wide_tree_levels(nodes.data(), n4, 0, begin.data(), lv + 1) != lv) return fail("second call", n);
        if (begin[0] != 0 || begin[1] != 1 || begin[lv] != n4) return fail("partition ends", n);
        for (int l = 0; l < lv; ++l) {
            if (begin[l + 1] <= begin[l]) return fail("empty level", n);
            for (int i = begin[l]; i < begin[l + 1]; ++i) {
                int32_t links[4];
                std::memcpy(links, &nodes[32 * (size_t)i + 24], sizeof links);
                for (int k = 0; k < 4; ++k) {
                    if (links[k] < 0) continue;
                    const int32_t id = links[k] & ((1 << 30) - 1);
                    if (id >= n4) continue;   // a leaf
                    if (l + 1 >= lv || id < begin[l + 1] || id >= begin[l + 2]) return fail("child outside the next level", n);
                }
            }
        }
        // with an id base: the same ranges
        std::vector<float> moved(nodes.begin(), nodes.begin() + 32 * (size_t)n4);
        const int32_t base = 1000;
        for (int i = 0; i < n4; ++i) {
            int32_t links[4];
            std::memcpy(links, &moved[32 * (size_t)i + 24], sizeof links);
            for (int k = 0; k < 4; ++k)
                if (links[k] >= 0) links[k] += (links[k] & ((1 << 30) - 1)) < n4 ? base : 2 * base;
            std::memcpy(&moved[32 * (size_t)i + 24], links, sizeof links);
        }
        std::vector<int32_t> begin2((size_t)lv + 1, -1);
        if (tpt_wide_tree_levels(moved.data(), n4, base, begin2.data(), lv + 1) != lv || begin2 != begin)
            return fail("id base", n);
        // arbitrary links: refused, or answered, but never read outside [0, n4)
        for (int round = 0; round < 50; ++round) {
            std::vector<float> bad(nodes.begin(), nodes.begin() + 32 * (size_t)n4);
            for (int e = 0; e < 1 + round % 4; ++e) {
                const int32_t word = (int32_t)rng();
                const size_t at = 32 * (size_t)(rng() % (uint32_t)n4) + 24 + rng() % 4;
                std::memcpy(&bad[at], &word, sizeof word);
            }
            std::vector<int32_t> out((size_t)lv + 8, -1);
            const int32_t got = tpt_wide_tree_levels(bad.data(), n4, 0, out.data(), lv + 8);
            if (got == 0 || got > n4) return fail("arbitrary links", n);
        }
    }
    if (tpt_wide_tree_levels(nullptr, 3, 0, nullptr, 0) != -1) return fail("null nodes", 0);
    std::printf("ok\n");
    return 0;
}
