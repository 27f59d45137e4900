// Host check of Arena (csrc/model.h): a few hundred mixed alloc / release / reset steps over a host buffer that stands for the device slab
// (nothing dereferences it), against a list of the live blocks kept here.  No GPU is touched.  Build and run (tests/test_arena_check.py does):
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/arena_check.cpp univst_amd/csrc/model.hip -o build/arena_check && build/arena_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../univst_amd/csrc/model.h"

void uv_set_error(const char*, ...) {}      // (abi.hip's, which this program does not link)

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

struct Live {
    size_t off, size;      // size as requested; the arena rounds it up to 256
};
static size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

int main() {
    const size_t SLAB = 1 << 20;
    std::vector<char> slab(SLAB);
    Arena a;
    a.base = slab.data();
    a.size = SLAB;
    a.reset();
    std::vector<Live> live;
    size_t max_end = 0, nulls = 0;
    unsigned rng = 12345;
    auto rnd = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
    auto whole = [&]() { return a.blocks.size() == 1 && a.blocks[0].free && a.blocks[0].off == 0 && a.blocks[0].size == SLAB; };
    for (int step = 0; step < 600; ++step) {
        if (live.empty() || rnd() % 3) {
            static const size_t sizes[] = {1, 255, 256, 257, 1000, 4096, 65536 + 1, 200000, 400000};
            const size_t n = sizes[rnd() % 9] + rnd() % 64;
            char* p = (char*)a.alloc(n);
            size_t largest = 0;      // first fit must succeed exactly when some free block holds the rounded size
            for (const Arena::Block& b : a.blocks)
                if (b.free) largest = std::max(largest, b.size);
            if (!p) {
                CHECK(largest < up256(n));
                ++nulls;
                continue;
            }
            const size_t off = p - a.base;
            CHECK(off % 256 == 0 && off + up256(n) <= SLAB);
            for (const Live& l : live) CHECK(off + up256(n) <= l.off || l.off + up256(l.size) <= off);      // never overlaps a live block
            live.push_back({off, n});
            max_end = std::max(max_end, off + up256(n));
        } else {
            const size_t i = rnd() % live.size();
            a.release(a.base + live[i].off);
            live.erase(live.begin() + i);
        }
        CHECK(a.high_water == max_end);
        size_t at = 0;      // the block list tiles the slab in order, and no two free blocks are neighbours
        for (size_t i = 0; i < a.blocks.size(); ++i) {
            CHECK(a.blocks[i].off == at && a.blocks[i].size > 0);
            CHECK(i == 0 || !(a.blocks[i].free && a.blocks[i - 1].free));
            at += a.blocks[i].size;
        }
        CHECK(at == SLAB);
    }
    CHECK(nulls > 0 && max_end > SLAB / 2);      // the walk did reach exhaustion
    a.release(nullptr);
    while (!live.empty()) {                      // everything released, in arbitrary order: one free block again
        const size_t i = rnd() % live.size();
        a.release(a.base + live[i].off);
        live.erase(live.begin() + i);
    }
    CHECK(whole());
    CHECK(a.alloc(SLAB + 1) == nullptr);         // exhaustion
    void* all = a.alloc(SLAB);
    CHECK(all == a.base && a.alloc(1) == nullptr && a.high_water == SLAB);
    a.reset();
    CHECK(whole() && a.high_water == SLAB);      // reset returns the blocks, the high-water mark is the handle's lifetime maximum
    printf("arena_check: ok (%zu exhausted requests, high water %zu of %zu)\n", nulls, max_end, SLAB);
    return 0;
}
