#!/usr/bin/env python3
"""Time pt_restir_di (row N10, the reservoir pass that makes the frame's direct illumination) on the C2 workload (demo scene seed 0, 8
bounces, 1 spp, a resting camera without jitter) and print one JSON line.

Per size, the median (and the 10-90 % spread) of --frames one-call-at-a-time measurements after --warmup calls, one context:
  * the pass alone at the defaults and with reuse off (EnableTemporal = EnableSpatial = 0), FrameIndex advancing, the history running:
    per launch from pt_get_profile (profiling on: launch 1 = initial + temporal under ms_traverse, launch 2 = spatial + final under
    ms_shade; event pairs around each launch, so no launch gap), their sum, and the host's wall time from the call to the end of a wait;
  * wall time, call to end of wait, of the chain pt_render_gbuffer + pt_restir_di + pt_render_with_di against pt_render with row N4's
    DI and without DI, back to back in this script.
  * row N17 (pt_restir_di_ex): in each local-light sampling mode (the library's default sizes), the pass with {1 BRDF candidate}, {the
    boiling filter at 0.2}, {both}, and the same call with the extras off, per launch and per call as above (keys restir_ex_<mode>_<config>_...;
    the presampling launches are under ms_tail and not in these figures);
  * row N22 (pt_restir_di_full; keys restir_full_<camera>_<config>_...): on the resting camera and on a travelling one (0.02 units per
    frame along x with the jitter sequence running; its G-buffer is rendered before each call, outside the timing), per launch and
    per call as above: final-visibility reuse off, at (MaxAge 0, MaxDistance 0) and at (4, 16) -- launch 2 with and without the final
    rays, launch 1 without and with the visibility word -- and Basic, Pairwise and Raytraced bias correction in both reuse passes;
    plus the share of the frame's pixels the pass wrote under each reuse setting;
Also the share of pixels that have a surface for the pass (finite depth, roughness >= 0.05) and the bytes the two launches must move
(launch 1: 20 B read per pixel (depth, NormalRoughness), without a surface 16 B written, with one 56 B more read, 100 B of record and
reservoir written and 100 B of history read; launch 2: 16 B read per pixel, with a surface 84 B more and 100 B for a neighbour, 32 B
written where DI is).
Kernel durations by name: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_restir_di.py`.

    python tools/bench_restir_di.py [--frames 200 --warmup 30 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402
from dxrs_amd.abi_types import GBUFFER_CHANNELS, RESTIR_DI_INPUTS  # noqa: E402


def summary(res, key, values):
    res[f"{key}_ms"] = round(float(np.median(values)), 4)
    res[f"{key}_spread_ms"] = round(float(np.percentile(values, 90) - np.percentile(values, 10)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    args = ap.parse_args()
    torch.cuda.init()
    host = dxrs_amd.load_host()
    spheres, mats, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    dev = torch.device("cuda", 0)
    width = dict(GBUFFER_CHANNELS)
    res = {"workload": "demo scene seed 0, 8 bounces, 1 spp, resting camera, one call at a time", "frames": args.frames}
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = dxrs_amd.Renderer(device=0)
        try:
            r.set_scene(spheres, mats, sd)
            r.set_camera(host.camera_matrices(w, h, jitter=False))
            r.set_constants(dxrs_amd.types.graphics_settings(w, h, bounces=8, spp=1))
            gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device=dev) for n in RESTIR_DI_INPUTS}
            out, dd, ds = (torch.zeros((h, w, 4), dtype=torch.float32, device=dev) for _ in range(3))
            torch.cuda.synchronize(dev)
            gptrs = {n: b.data_ptr() for n, b in gb.items()}
            bufs = dict(gptrs, Diffuse=dd.data_ptr(), Specular=ds.data_ptr())
            r.render_gbuffer_device(gptrs)
            r.synchronize()
            surface = torch.isfinite(gb["LinearDepth"][..., 0]) & (gb["NormalRoughness"][..., 3] >= 0.05)
            res[f"surface_share_{size}"] = round(float(surface.float().mean()), 4)
            # the pass alone, per launch and as a whole
            r.set_profiling(True)
            for kind, kw in (("defaults", {}), ("reuse_off", dict(temporal=False, spatial=False))):
                l1, l2, wall = [], [], []
                for k in range(args.warmup + args.frames):
                    r.profile(reset=True)
                    t0 = time.perf_counter()
                    r.restir_di_device(w, h, bufs, frame_index=k, reset_history=k == 0, **kw)
                    r.synchronize()
                    t1 = time.perf_counter()
                    p = r.profile(reset=True)
                    if k >= args.warmup:
                        l1.append(p.ms_traverse); l2.append(p.ms_shade); wall.append((t1 - t0) * 1e3)
                summary(res, f"restir_{kind}_{size}_launch1", l1)
                summary(res, f"restir_{kind}_{size}_launch2", l2)
                summary(res, f"restir_{kind}_{size}_launches", [a + b for a, b in zip(l1, l2)])
                summary(res, f"restir_{kind}_{size}_wall", wall)
            # row N17: the extras in each sampling mode, next to the same call without them
            t = dxrs_amd.types
            for mode, ls in (("uniform", None), ("power", dict(mode=t.LIGHT_SAMPLING_POWER_RIS)), ("regir", dict(mode=t.LIGHT_SAMPLING_REGIR_RIS))):
                for config, cd in (("off", dict()), ("brdf1", dict(brdf_samples=1)), ("filter", dict(boiling_filter=0.2)), ("both", dict(brdf_samples=1, boiling_filter=0.2))):
                    l1, l2, wall = [], [], []
                    for k in range(args.warmup + args.frames):
                        r.profile(reset=True)
                        t0 = time.perf_counter()
                        r.restir_di_device(w, h, bufs, frame_index=k, reset_history=k == 0, light_sampling=ls, candidates=cd)
                        r.synchronize()
                        t1 = time.perf_counter()
                        p = r.profile(reset=True)
                        if k >= args.warmup:
                            l1.append(p.ms_traverse); l2.append(p.ms_shade); wall.append((t1 - t0) * 1e3)
                    summary(res, f"restir_ex_{mode}_{config}_{size}_launch1", l1)
                    summary(res, f"restir_ex_{mode}_{config}_{size}_launch2", l2)
                    summary(res, f"restir_ex_{mode}_{config}_{size}_wall", wall)
            # row N22: final-visibility reuse and pairwise MIS, on a resting and on a travelling camera
            reuse = (("reuse_off", dict(shading={})), ("reuse_0_0", dict(shading=dict(reuse=True, max_age=0, max_distance=0.0))),
                     ("reuse_4_16", dict(shading=dict(reuse=True, max_age=4, max_distance=16.0))))
            bias = tuple((name, dict(shading={}, temporal_bias=mode, spatial_bias=mode)) for name, mode in
                         (("basic", t.RESTIR_BIAS_BASIC), ("pairwise", t.RESTIR_BIAS_PAIRWISE), ("raytraced", t.RESTIR_BIAS_RAYTRACED)))
            for camera in ("resting", "travelling"):
                for config, kw in reuse + bias:
                    l1, l2, wall, prev = [], [], [], None
                    for k in range(args.warmup + args.frames):
                        if camera == "travelling":
                            prev = host.camera_matrices(w, h, position=(0.02 * k, 0.0, -15.0), jitter_index=k, previous=prev)
                            r.set_camera(prev)
                            r.render_gbuffer_device(gptrs)
                            r.synchronize()
                        if config.startswith("reuse") and k == args.warmup + args.frames - 1:
                            dd.zero_(); ds.zero_()
                            torch.cuda.synchronize(dev)
                        r.profile(reset=True)
                        t0 = time.perf_counter()
                        r.restir_di_device(w, h, bufs, frame_index=k, reset_history=k == 0, **kw)
                        r.synchronize()
                        t1 = time.perf_counter()
                        p = r.profile(reset=True)
                        if k >= args.warmup:
                            l1.append(p.ms_traverse); l2.append(p.ms_shade); wall.append((t1 - t0) * 1e3)
                    summary(res, f"restir_full_{camera}_{config}_{size}_launch1", l1)
                    summary(res, f"restir_full_{camera}_{config}_{size}_launch2", l2)
                    summary(res, f"restir_full_{camera}_{config}_{size}_wall", wall)
                    if config.startswith("reuse"):
                        res[f"restir_full_{camera}_{config}_{size}_written_share"] = round(float((dd[..., :3].sum(-1) + ds[..., :3].sum(-1) > 0).float().mean()), 6)
            r.set_camera(host.camera_matrices(w, h, jitter=False))
            r.render_gbuffer_device(gptrs)
            r.restir_di_device(w, h, bufs, frame_index=0, reset_history=True)
            r.synchronize()
            r.set_profiling(False)
            res[f"lit_share_{size}"] = round(float((dd[..., :3].sum(-1) + ds[..., :3].sum(-1) > 0).float().mean()), 4)
            # the chain against pt_render with and without row N4's DI
            for kind in ("render", "render_n4", "chain"):
                r.set_constants(dxrs_amd.types.graphics_settings(w, h, bounces=8, spp=1, di=kind == "render_n4"))
                wall = []
                for k in range(args.warmup + args.frames):
                    t0 = time.perf_counter()
                    if kind == "chain":
                        r.render_gbuffer_device(gptrs)
                        r.restir_di_device(w, h, bufs, frame_index=k, reset_history=k == 0)
                        r.render_with_di_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr())
                    else:
                        r.render_device(out.data_ptr())
                    r.synchronize()
                    if k >= args.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                summary(res, f"{kind}_{size}_wall", wall)
            n = w * h
            ns = int(surface.sum())
            res[f"launch1_{size}_bytes"] = n * 20 + (n - ns) * 16 + ns * 256
            res[f"launch2_{size}_bytes"] = n * 16 + ns * 184 + int(res[f"lit_share_{size}"] * n) * 32
        finally:
            r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
