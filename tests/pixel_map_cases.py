"""The maps that tests/test_pixel_map.py (CPU) and tests/test_gpu_pixel_map.py (GPU) check, and the slot -> pixel mapping restated in plain
integers with // and %: what csrc/pt_device.h's slot_to_pixel computed before the division became a multiply-high.

A map is the seven words the shims take (tests/hostshim/pixmap_host.h):
  (0, img_w, img_h, x, y, w, h)                 a rect of the image, cut into 8x8-pixel blocks, 64 slots per block
  (1, img_w, img_h, ts, first, run, stride)     the ts x ts tiles t with first <= t % stride < first + run, ts * ts slots per tile"""
import numpy as np

MAPS = {
    "rect_1x1": (0, 1, 1, 0, 0, 1, 1),
    "rect_7x5": (0, 7, 5, 0, 0, 7, 5),
    "rect_8x8": (0, 8, 8, 0, 0, 8, 8),
    "rect_9x9": (0, 9, 9, 0, 0, 9, 9),
    "rect_70x42": (0, 70, 42, 0, 0, 70, 42),
    "rect_1027x8": (0, 1027, 8, 0, 0, 1027, 8),  # blocks_x = 129
    "subrect_64x48": (0, 64, 48, 3, 5, 21, 13),
    "rect_16384x16384": (0, 16384, 16384, 0, 0, 16384, 16384),  # 2^22 blocks: where the float-reciprocal division used to hand over
    **{f"tiles_ts{ts}_{f}_{r}_{s}": (1, 70, 42, ts, f, r, s) for ts in (8, 16, 32) for f, r, s in ((0, 1, 1), (1, 1, 3), (2, 3, 7))},
    "tiles_none_owned": (1, 9, 9, 32, 1, 1, 3),  # one tile, owned by rank 0 of 3
}


def owned_tiles(m):
    _, w, h, ts, first, run, stride = m
    total = ((w + ts - 1) // ts) * ((h + ts - 1) // ts)
    return [t for t in range(total) if first <= t % stride < first + run]


def n_slots(m):
    if m[0] == 0:
        return ((m[5] + 7) // 8) * ((m[6] + 7) // 8) * 64
    return len(owned_tiles(m)) * m[3] * m[3]


def slots_of(name):
    """every slot of the map; the giant rect is sampled: every 4099th slot and the last 4096"""
    n = n_slots(MAPS[name])
    if name == "rect_16384x16384":
        return np.ascontiguousarray(np.unique(np.concatenate([np.arange(0, n, 4099, dtype=np.int64), np.arange(n - 4096, n, dtype=np.int64)])).astype(np.uint32))
    return np.arange(n, dtype=np.uint32)


def expected(m, slots):
    """(len(slots), 4) uint32 {px, py, out_index, valid}, in uint32 arithmetic as the kernels'"""
    s = np.asarray(slots, dtype=np.int64)
    if m[0] == 0:
        _, _, _, rx, ry, rw, rh = m
        blocks_x = (rw + 7) // 8
        b, l = s // 64, s % 64
        by, bx = b // blocks_x, b % blocks_x
        x, y = bx * 8 + l % 8, by * 8 + l // 8
        valid = (x < rw) & (y < rh)
        px, py, out = rx + x, ry + y, y * rw + x
    else:
        _, img_w, img_h, ts, first, run, stride = m
        tiles_x = (img_w + ts - 1) // ts
        tiles_total = tiles_x * ((img_h + ts - 1) // ts)
        k, w = s // (ts * ts), s % (ts * ts)
        b, l = w // 64, w % 64
        bpt = ts // 8
        lx, ly = (b % bpt) * 8 + l % 8, (b // bpt) * 8 + l // 8
        q = k // run
        gt = first + q * stride + (k - q * run)
        ty, tx = gt // tiles_x, gt % tiles_x
        px, py = tx * ts + lx, ty * ts + ly
        valid = (gt < tiles_total) & (px < img_w) & (py < img_h)
        out = k * ts * ts + ly * ts + lx
    return np.stack([px % 2 ** 32, py % 2 ** 32, out % 2 ** 32, valid.astype(np.int64)], axis=1).astype(np.uint32)
