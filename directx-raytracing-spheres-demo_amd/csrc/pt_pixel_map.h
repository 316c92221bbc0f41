// pt_pixel_map.h -- the slot -> pixel mapping of the primary pass and of every kernel that walks a frame's slots.  No HIP types: the
// kernels, the host side that fills the map (pt_api.hip) and the host-compiled tests (tests/hostshim/pixmap_host.cpp) share this file.
#pragma once

#include <stdint.h>

#include "pt_magic_div.h"

namespace pt {

// A slot is 64-aligned to an 8x8 pixel block so that one wave64 = one 8x8 block of pixels.
//   mode 0 (rect):  block b = slot / 64 over ceil(w/8) x ceil(h/8) blocks of the rect
//   mode 1 (tiles): tile k = slot / ts^2 is this rank's k-th tile = global tile (rank + k * world)
struct PixelMap {
    uint32_t mode;
    uint32_t img_w, img_h;        // RenderSize
    uint32_t rx, ry, rw, rh;      // rect (mode 0)
    uint32_t blocks_x;            // ceil(rw / 8) (mode 0)
    uint32_t ts, tiles_x, tiles_total;  // mode 1 (ts = 1 << ts_shift)
    // mode 1 ownership: the tiles t with first <= t % stride < first + run, in increasing t (pt_set_partition_ex);
    // the plain rank/world interleave is (first, run, stride) = (rank, 1, world)
    uint32_t first, run, stride;
    uint32_t ts_shift;
    uint32_t n_slots;
    MagicDiv div_blocks_x, div_tiles_x, div_run;  // the divisions by blocks_x, tiles_x and run (pt_magic_div.h), made with the map
};

struct PixelRef {
    uint32_t px, py;     // global pixel
    uint32_t out_index;  // index into the output float4 buffer
    bool valid;
};

// the map of a rect of the image: 8x8-pixel blocks of the rect (the caller sets n_slots)
inline PixelMap pixel_map_rect(uint32_t img_w, uint32_t img_h, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh)
{
    PixelMap pm{};
    pm.mode = 0;
    pm.img_w = img_w; pm.img_h = img_h;
    pm.rx = rx; pm.ry = ry; pm.rw = rw; pm.rh = rh;
    pm.blocks_x = (rw + 7) / 8;
    pm.div_blocks_x = make_magic_div(pm.blocks_x);
    pm.div_tiles_x = pm.div_run = make_magic_div(1u);
    return pm;
}

// the map of the tiles (edge ts, a power of two >= 8) that a partition (first, run, stride) owns (the caller sets n_slots)
inline PixelMap pixel_map_tiles(uint32_t img_w, uint32_t img_h, uint32_t ts, uint32_t first, uint32_t run, uint32_t stride)
{
    PixelMap pm{};
    pm.mode = 1;
    pm.img_w = img_w; pm.img_h = img_h;
    pm.ts = ts;
    pm.ts_shift = (uint32_t)__builtin_ctz(ts);
    pm.tiles_x = (img_w + ts - 1) / ts;
    pm.tiles_total = pm.tiles_x * ((img_h + ts - 1) / ts);
    pm.first = first; pm.run = run; pm.stride = stride;
    pm.div_blocks_x = make_magic_div(1u);
    pm.div_tiles_x = make_magic_div(pm.tiles_x);
    pm.div_run = make_magic_div(run);
    return pm;
}

// Where an 8x8 block's pixels lie.  Made from the block index alone: for a wave whose 64 slots are one block (the primary pass) every
// member is wave-uniform and the arithmetic below runs on the scalar unit, once per tile.
struct BlockOrigin {
    uint32_t px0, py0;      // global pixel of the block's lane 0
    uint32_t out0, pitch;   // its index into the output buffer, and the output's row pitch (rw, or ts inside a packed tile)
    uint32_t ext_x, ext_y;  // columns / rows of the block that lie inside the rect (the image, for an owned tile); 0 = none
};

PT_MD BlockOrigin block_origin(const PixelMap& m, uint32_t block)
{
    BlockOrigin o;
    if (m.mode == 0) {
        const uint32_t by = magic_div(block, m.div_blocks_x), bx = block - by * m.blocks_x;
        const uint32_t x0 = bx * 8u, y0 = by * 8u;
        o.px0 = m.rx + x0;
        o.py0 = m.ry + y0;
        o.out0 = y0 * m.rw + x0;
        o.pitch = m.rw;
        o.ext_x = x0 < m.rw ? m.rw - x0 : 0u;
        o.ext_y = y0 < m.rh ? m.rh - y0 : 0u;
    } else {
        // tile edge ts is a power of two >= 8 (ts_shift = log2 ts): shifts and masks only, except the tile -> (tx, ty) split
        const uint32_t bpt_shift = m.ts_shift - 3u;      // 8x8 blocks per tile row = ts / 8
        const uint32_t kb_shift = 2u * bpt_shift;        // blocks per tile = (ts / 8)^2
        const uint32_t k = block >> kb_shift, b = block & ((1u << kb_shift) - 1u);
        const uint32_t lx0 = (b & ((1u << bpt_shift) - 1u)) << 3, ly0 = (b >> bpt_shift) << 3;
        uint32_t gt;
        if (m.run == 1u) {
            gt = m.first + k * m.stride;
        } else {
            const uint32_t q = magic_div(k, m.div_run);
            gt = m.first + q * m.stride + (k - q * m.run);
        }
        const uint32_t ty = magic_div(gt, m.div_tiles_x), tx = gt - ty * m.tiles_x;
        o.px0 = (tx << m.ts_shift) + lx0;
        o.py0 = (ty << m.ts_shift) + ly0;
        o.out0 = (k << (2u * m.ts_shift)) + (ly0 << m.ts_shift) + lx0;
        o.pitch = m.ts;
        o.ext_x = (gt < m.tiles_total && o.px0 < m.img_w) ? m.img_w - o.px0 : 0u;
        o.ext_y = o.py0 < m.img_h ? m.img_h - o.py0 : 0u;
    }
    return o;
}

// the lane's pixel inside its block (lane = slot & 63)
PT_MD PixelRef block_pixel(const BlockOrigin& o, uint32_t lane)
{
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    PixelRef r;
    r.px = o.px0 + lx;
    r.py = o.py0 + ly;
    r.valid = lx < o.ext_x && ly < o.ext_y;
    r.out_index = o.out0 + ly * o.pitch + lx;
    return r;
}
PT_MD uint32_t block_out_index(const BlockOrigin& o, uint32_t lane) { return o.out0 + (lane >> 3) * o.pitch + (lane & 7u); }

// For kernels whose lanes hold slots of different blocks (queue-fed passes, the side passes): the same arithmetic per lane, each division a
// multiply-high and a shift.
PT_MD PixelRef slot_to_pixel(const PixelMap& m, uint32_t slot) { return block_pixel(block_origin(m, slot >> 6), slot & 63u); }

}  // namespace pt
