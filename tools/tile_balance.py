#!/usr/bin/env python3
"""Predict, on the CPU, how evenly the two tile maps of the 1-spp primary pass (csrc/pt_trace.h bounce_kernel) spread the C2
frame's work over its workgroups.  Host library and the host-compiled device headers only: no GPU.

Every 8x8 block of the resting C2 view (demo scene, 1920x1080) is put into one of the three classes the tile-order table sorts by, with the
product's own pyramid and region tests (tests/hostshim/beam_host.cpp, region_host.cpp over the padded leaf boxes of pt_lbvh.cpp, as
tests/test_gpu_list_walk.py computes lists):
  sky     the block's primary-beam list is empty
  region  the list is not empty and the block has a region record: its five rays land on one mirror-like sphere and the region's list fits
  walk    the list is not empty and there is no region record: the bounce-1 rays of the block walk the tree
A block costs its class's weight in wave instructions: sky and ground (region) from DESIGN.md 7 (about 175, and 1 400-2 200: 1 800); what a
tree-walking block costs has not been measured per tile, so it is a parameter, swept from 2x to 5x ground.  A workgroup's cost is the sum
over the tiles it draws; a pass is as long as its slowest workgroup, so max / mean over the workgroups is how much longer than a perfectly
balanced pass it runs (the bound ignores that a CU holds two workgroups and that a workgroup's eight waves share its tiles).

  batch map        draw w of workgroup b is wave slot w % 8 of batch b + (w / 8) * grid: eight runs of eight consecutive blocks
  interleaved map  draw w of workgroup b is tile b + grid * w

    python tools/tile_balance.py [--width 1920 --height 1080 --grid 512 --waves 8]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

F32P, U32P, U8P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
SKY, GROUND = 175.0, 1800.0      # wave instructions per tile
REFL_CAP = 21                    # kReflListCap (pt_region.h)
BEAM_CAP = 15                    # kBeamListCap (pt_beam.h)
MAX_ROUGHNESS, MIN_ROUGHNESS = 2.5e-3, 2e-3  # kReflMaxRoughness, kMinRoughness


def fp(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(F32P)


def load_shims():
    beam = C.CDLL(entry.build_beam_shim())
    beam.bm_make.argtypes = [F32P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, F32P]
    beam.bm_meets_boxes.argtypes = [F32P, C.c_uint32, F32P, U8P]
    beam.bm_meets_leaves.argtypes = [F32P, C.c_uint32, F32P, U8P]
    beam.bm_rays.argtypes = [F32P, C.c_uint32, C.c_uint32, C.c_uint32, U32P, F32P, F32P, F32P, F32P]
    region = C.CDLL(entry.build_region_shim())
    region.rg_meets_boxes.argtypes = [F32P, C.c_uint32, F32P, U8P]
    region.rg_from_rays.argtypes = [F32P, F32P, F32P, C.c_float, F32P]
    region.rg_from_rays.restype = C.c_int
    for f in (beam.bm_make, beam.bm_meets_boxes, beam.bm_meets_leaves, beam.bm_rays, region.rg_meets_boxes):
        f.restype = None
    return beam, region


def leaf_boxes(spheres):
    """the padded cubes the tree builders put around the spheres (pt_lbvh.cpp)"""
    c = np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(np.float32)
    r = spheres["r"].astype(np.float32)[:, None]
    bmin, bmax = (c - r).min(0), (c + r).max(0)
    pad = np.float32(max(np.abs(bmin).max(), np.abs(bmax).max())) * np.float32(2.0 ** -17)
    return np.ascontiguousarray(np.concatenate([c - r - pad, c + r + pad], 1), dtype=np.float32)


def block_rays(beam, cam12, w, h, bx, by):
    """the five rays of every block's pyramid (its corners in beam_corners' order, then its centre): float32 directions [n, 5, 3], origin"""
    x0, y0 = 8.0 * bx - 0.5, 8.0 * by - 0.5
    pts = np.stack([np.stack([x0, y0], 1), np.stack([x0 + 9.0, y0], 1), np.stack([x0 + 9.0, y0 + 9.0], 1), np.stack([x0, y0 + 9.0], 1),
                    np.stack([x0 + 4.5, y0 + 4.5], 1)], 1).reshape(-1, 2)
    pix = np.clip(np.floor(pts), 0, [w - 1, h - 1])  # (primary_ray is affine in pixel + jitter: the split between the two is free)
    jit = np.ascontiguousarray(pts - pix - 0.5, dtype=np.float32)
    pix = np.ascontiguousarray(pix, dtype=np.uint32)
    o, d = np.zeros((len(pix), 3), np.float32), np.zeros((len(pix), 3), np.float32)
    beam.bm_rays(fp(cam12), w, h, len(pix), pix.ctypes.data_as(U32P), fp(jit), None, fp(o), fp(d))
    return o[0].copy(), d.reshape(-1, 5, 3)


def first_hits(o, d, spheres):
    """float64 closest sphere of every ray: ids [n] (-1: a miss)"""
    c = np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(np.float64)
    r = spheres["r"].astype(np.float64)
    d = d.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    best_t, best = np.full(len(d), np.inf), np.full(len(d), -1, np.int64)
    for j in range(len(c)):
        oc = o.astype(np.float64) - c[j]
        b = d @ oc
        disc = b * b - (oc @ oc - r[j] * r[j])
        ok = disc >= 0.0
        sq = np.sqrt(np.where(ok, disc, 0.0))
        t = np.where(-b - sq > 0.0, -b - sq, -b + sq)
        ok &= (t > 0.0) & (t < best_t)
        best_t[ok], best[ok] = t[ok], j
    return best


def classify(w, h):
    """class of every block in slot (raster) order: 0 sky, 1 region, 2 walk"""
    host = dxrs_amd.load_host()
    spheres, materials, _ = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    cam = host.camera(w, h, jitter_index=0, jitter_count=8)
    cam12 = np.array([*cam.Position, *cam.RightDirection, *cam.UpDirection, *cam.ForwardDirection], np.float32)
    beam, region = load_shims()
    boxes = leaf_boxes(spheres)
    n = len(boxes)
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    by, bx = np.divmod(np.arange(nbx * nby), nbx)
    o, dirs = block_rays(beam, cam12, w, h, bx.astype(np.float64), by.astype(np.float64))
    hit = first_hits(o, dirs.reshape(-1, 3), spheres).reshape(-1, 5)
    # a material that samples the specular lobe only (lobe_weights: no diffuse albedo, no transmission), smooth enough for a region
    mirror = ((materials["Metallic"] == 1.0) | ((materials["BaseColor"][:, :3] == 0.0).all(1) & (materials["Transmission"] == 0.0))) \
        & (np.maximum(materials["Roughness"], MIN_ROUGHNESS) <= MAX_ROUGHNESS) & (materials["AlphaMode"] == 0)
    cls = np.zeros(nbx * nby, np.int64)
    g, rg, out = np.zeros(16, np.float32), np.zeros(11, np.float32), np.zeros(n, np.uint8)
    out2 = np.zeros(n, np.uint8)
    for t in range(nbx * nby):
        beam.bm_make(fp(cam12), w, h, 8 * int(bx[t]), 8 * int(by[t]), 0.0, 0.0, fp(g))
        beam.bm_meets_boxes(fp(g), n, fp(boxes), out.ctypes.data_as(U8P))
        beam.bm_meets_leaves(fp(g), n, fp(boxes), out2.ctypes.data_as(U8P))
        count = int((out & out2).sum())
        if count == 0:
            continue
        cls[t] = 2
        s = hit[t, 0]
        if count > BEAM_CAP or s < 0 or (hit[t] != s).any() or not mirror[s]:
            continue
        centre = np.array([spheres["cx"][s], spheres["cy"][s], spheres["cz"][s]], np.float32)
        if not region.rg_from_rays(fp(o), fp(np.ascontiguousarray(dirs[t])), fp(centre), C.c_float(float(spheres["r"][s])), fp(rg)):
            continue
        region.rg_meets_boxes(fp(rg), n, fp(boxes), out.ctypes.data_as(U8P))
        if 1 <= int(out.sum()) <= REFL_CAP:
            cls[t] = 1
    return cls, nbx, nby


def tiles_of(grid, waves, n_draws, interleave):
    """tile index [grid, n_draws] of draw w of workgroup b (indices past the frame's end included)"""
    b, wv = np.arange(grid)[:, None], np.arange(n_draws)[None, :]
    return b + grid * wv if interleave else (b + (wv // waves) * grid) * waves + wv % waves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, default=512, help="workgroups of the primary pass (2 per CU on 256 CUs)")
    ap.add_argument("--waves", type=int, default=8, help="waves per workgroup")
    args = ap.parse_args()
    cls, nbx, nby = classify(args.width, args.height)
    n = len(cls)
    batches = (n + args.waves - 1) // args.waves
    n_draws = (batches + args.grid - 1) // args.grid * args.waves  # seg_cap / 64
    counts = {"sky": int((cls == 0).sum()), "region": int((cls == 1).sum()), "walk": int((cls == 2).sum())}
    print(json.dumps({"width": args.width, "height": args.height, "blocks": [nbx, nby], "grid": args.grid, "draws_per_workgroup": n_draws, "classes": counts}))
    rows = np.flatnonzero((cls.reshape(nby, nbx) == 2).any(1))
    print(json.dumps({"walk_block_rows": [int(rows.min()), int(rows.max())] if len(rows) else None}))
    for name, inter in (("batch", False), ("interleaved", True)):
        t = tiles_of(args.grid, args.waves, n_draws, inter)
        inside = t < n
        walk = ((cls[np.minimum(t, n - 1)] == 2) & inside).sum(1)
        print(json.dumps({"map": name, "walk_tiles_per_workgroup": {"max": int(walk.max()), "mean": round(float(walk.mean()), 2),
                                                                     "workgroups_without": int((walk == 0).sum())}}))
    for k in (2.0, 3.0, 4.0, 5.0):
        weight = np.array([SKY, GROUND, k * GROUND])
        line = {"walk_over_ground": k}
        for name, inter in (("batch", False), ("interleaved", True)):
            t = tiles_of(args.grid, args.waves, n_draws, inter)
            cost = np.where(t < n, weight[cls[np.minimum(t, n - 1)]], 0.0).sum(1)
            line[name] = {"max_over_mean": round(float(cost.max() / cost.mean()), 3), "max": int(cost.max()), "mean": int(cost.mean())}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
