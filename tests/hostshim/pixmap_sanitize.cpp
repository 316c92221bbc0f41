// pixmap_sanitize.cpp -- TEST PROGRAM: csrc/pt_magic_div.h and csrc/pt_pixel_map.h stand-alone, so that tests/test_pixel_map.py can build it with
// -fsanitize=address,undefined and run it as a child process: pairs for small, large and power-of-two divisors, and every slot of a rect map, a
// sub-rect, a 1x1 frame, tile maps and a partition that owns nothing, both forms, against / and %.
// Prints what it saw; exit status 0 = every invariant held (the sanitizers abort on their own findings).
#include "pixmap_host.h"
#include <cstdio>
#include <vector>

using namespace pixhost;

static int check_map(const uint32_t (&d)[7])
{
    const pt::PixelMap pm = make_map(d);
    std::vector<uint32_t> slots(pm.n_slots), a((size_t)pm.n_slots * 4u), b((size_t)pm.n_slots * 4u);
    for (uint32_t i = 0; i < pm.n_slots; i++) slots[i] = i;
    map_slots(pm, pm.n_slots, slots.data(), a.data(), 0);
    map_slots(pm, pm.n_slots, slots.data(), b.data(), 1);
    if (a != b) { std::printf("the two forms disagree\n"); return 1; }
    uint64_t valid = 0;
    for (uint32_t i = 0; i < pm.n_slots; i++) {
        const uint32_t* r = &a[(size_t)i * 4u];
        if (r[2] >= pm.n_slots && d[0] == 1u) { std::printf("packed index out of range\n"); return 1; }
        if (r[3]) {
            valid++;
            if (r[0] >= d[1] || r[1] >= d[2]) { std::printf("valid pixel outside the image\n"); return 1; }
            if (d[0] == 0u && r[2] != (r[1] - d[4]) * d[5] + (r[0] - d[3])) { std::printf("rect index wrong\n"); return 1; }
        }
    }
    std::printf("mode %u %ux%u (%u %u %u %u): %u slots, %llu valid\n", d[0], d[1], d[2], d[3], d[4], d[5], d[6], pm.n_slots, (unsigned long long)valid);
    if (d[0] == 0u && valid != (uint64_t)d[5] * d[6]) { std::printf("valid count wrong\n"); return 1; }
    return 0;
}

int main()
{
    for (uint32_t d : { 1u, 2u, 3u, 7u, 129u, 240u, 256u, 4097u, 65535u, (1u << 25) - 1u, (1u << 26) - 1u, (1u << 26), 0x7FFFFFFFu }) {
        uint32_t first = 0;
        uint64_t bad = div_mismatches(d, 0u, 1u << 16, &first) + div_mismatches(d, (1u << 26) - (1u << 12), 1u << 26, &first);
        bad += div_mismatches(d, 0x7FFFFFFFu - 4096u, 0x7FFFFFFFu, &first);
        if (bad) { std::printf("d = %u: %llu quotients differ, first n = %u\n", d, (unsigned long long)bad, first); return 1; }
    }
    const uint32_t maps[][7] = { { 0, 1, 1, 0, 0, 1, 1 }, { 0, 7, 5, 0, 0, 7, 5 }, { 0, 70, 42, 0, 0, 70, 42 }, { 0, 1027, 8, 0, 0, 1027, 8 }, { 0, 64, 48, 3, 5, 21, 13 },
                                 { 1, 70, 42, 8, 0, 1, 1 }, { 1, 70, 42, 16, 1, 1, 3 }, { 1, 70, 42, 32, 2, 3, 7 }, { 1, 70, 42, 8, 2, 3, 7 }, { 1, 9, 9, 32, 1, 1, 3 } };
    for (const auto& m : maps)
        if (check_map(m)) return 1;
    std::printf("ok\n");
    return 0;
}
