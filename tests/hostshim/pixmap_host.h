// pixmap_host.h -- TEST SHIM: csrc/pt_magic_div.h and csrc/pt_pixel_map.h compiled as host C++, behind the entry points that pixmap_host.cpp
// (the library tests/test_pixel_map.py loads) and pixmap_sanitize.cpp (the stand-alone sanitizer program) share.
//   A map is described by seven words: {mode, img_w, img_h, a, b, c, d}
//     mode 0: rect (a, b, c, d) = (x, y, w, h) of an img_w x img_h image
//     mode 1: tiles of edge a owned by the partition (first, run, stride) = (b, c, d)
//   n_slots is what the host side sets: the rect's blocks * 64, or the owned tiles * a * a.
// Not part of the product; never loaded by it.
#pragma once

#include <stdint.h>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_pixel_map.h"

namespace pixhost {

// the tiles t < total with first <= t % stride < first + run
inline uint32_t owned_tiles(uint32_t total, uint32_t first, uint32_t run, uint32_t stride)
{
    uint32_t n = 0;
    for (uint32_t t = 0; t < total; t++) {
        const uint32_t r = t % stride;
        if (r >= first && r < first + run) n++;
    }
    return n;
}

inline pt::PixelMap make_map(const uint32_t* d)
{
    pt::PixelMap pm;
    if (d[0] == 0u) {
        pm = pt::pixel_map_rect(d[1], d[2], d[3], d[4], d[5], d[6]);
        pm.n_slots = (uint32_t)((uint64_t)((d[5] + 7) / 8) * ((d[6] + 7) / 8) * 64ull);
    } else {
        pm = pt::pixel_map_tiles(d[1], d[2], d[3], d[4], d[5], d[6]);
        pm.n_slots = owned_tiles(pm.tiles_total, d[4], d[5], d[6]) * d[3] * d[3];
    }
    return pm;
}

// out[4 i ..] = {px, py, out_index, valid} of slots[i]: block_origin + block_pixel (form 0) or the per-lane slot_to_pixel (form 1)
inline void map_slots(const pt::PixelMap& pm, uint32_t n, const uint32_t* slots, uint32_t* out, int form)
{
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t s = slots[i];
        const pt::PixelRef r = form == 0 ? pt::block_pixel(pt::block_origin(pm, s >> 6), s & 63u) : pt::slot_to_pixel(pm, s);
        out[4 * (size_t)i + 0] = r.px; out[4 * (size_t)i + 1] = r.py; out[4 * (size_t)i + 2] = r.out_index; out[4 * (size_t)i + 3] = r.valid ? 1u : 0u;
    }
}

// the number of n in [lo, hi) with magic_div(n, pair of d) != n / d, and the first such n
inline uint64_t div_mismatches(uint32_t d, uint32_t lo, uint32_t hi, uint32_t* first_bad)
{
    const pt::MagicDiv m = pt::make_magic_div(d);
    uint64_t bad = 0;
    for (uint32_t n = lo; n < hi; n++)
        if (pt::magic_div(n, m) != n / d) { if (bad++ == 0 && first_bad) *first_bad = n; }
    return bad;
}

}  // namespace pixhost
