#!/usr/bin/env python3
"""Time pt_restir_di_sampled (row N16: Power_RIS and ReGIR local-light presampling in front of the reservoir pass, DESIGN.md spec S22)
on the C2 workload (demo scene seed 0, a resting camera without jitter) and print one JSON line.

Per size, the median (and the 10-90 % spread) of --frames one-call-at-a-time measurements after --warmup calls, one context, the
history running, FrameIndex advancing:
  * per mode (uniform = pt_restir_di, power, regir, at the defaults): launch 1 (ms_traverse) and launch 2 (ms_shade) from pt_get_profile,
    the presampling launches as one interval (ms_tail), and the host's wall time from the call to the end of a wait;
  * per stage, as differences of such intervals: pyramid = the presampling interval of Power_RIS with one tile of one entry, Power segment
    = Power_RIS at the defaults minus that, ReGIR segment = ReGIR_RIS at the defaults minus Power_RIS at the defaults;
  * the scene's emitter count, and the RMSE of one frame's DI (luminance of Diffuse + Specular, reuse off) in the three modes against
    the average of --reference-frames frames of uniform candidates (the smallest size only).

    python tools/bench_light_ris.py [--frames 200 --warmup 30 --sizes 1920x1080,3840x2160 --reference-frames 4096]"""
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
from dxrs_amd.abi_types import GBUFFER_CHANNELS, LIGHT_SAMPLING_POWER_RIS, LIGHT_SAMPLING_REGIR_RIS, RESTIR_DI_INPUTS  # noqa: E402

MODES = (("uniform", None), ("power", dict(mode=LIGHT_SAMPLING_POWER_RIS)), ("regir", dict(mode=LIGHT_SAMPLING_REGIR_RIS)))


def summary(res, key, values):
    res[f"{key}_ms"] = round(float(np.median(values)), 4)
    res[f"{key}_spread_ms"] = round(float(np.percentile(values, 90) - np.percentile(values, 10)), 4)


def timed(r, w, h, bufs, ls, frames, warmup, **kw):
    """-> per-call lists (presampling, launch 1, launch 2, wall) in ms"""
    pre, l1, l2, wall = [], [], [], []
    for k in range(warmup + frames):
        r.profile(reset=True)
        t0 = time.perf_counter()
        r.restir_di_device(w, h, bufs, frame_index=k, reset_history=k == 0, light_sampling=ls, **kw)
        r.synchronize()
        t1 = time.perf_counter()
        p = r.profile(reset=True)
        if k >= warmup:
            pre.append(p.ms_tail); l1.append(p.ms_traverse); l2.append(p.ms_shade); wall.append((t1 - t0) * 1e3)
    return pre, l1, l2, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--reference-frames", type=int, default=4096)
    args = ap.parse_args()
    torch.cuda.init()
    host = dxrs_amd.load_host()
    spheres, mats, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    dev = torch.device("cuda", 0)
    width = dict(GBUFFER_CHANNELS)
    res = {"workload": "demo scene seed 0, resting camera, one call at a time", "frames": args.frames,
           "emitters": int(((mats["EmissiveStrength"][:, None] * mats["EmissiveColor"]) > 0).any(axis=1).sum())}
    sizes = [tuple(int(v) for v in size.split("x")) for size in args.sizes.split(",")]
    for w, h in sizes:
        size = f"{w}x{h}"
        r = dxrs_amd.Renderer(device=0)
        try:
            r.set_scene(spheres, mats, sd)
            r.set_camera(host.camera_matrices(w, h, jitter=False))
            r.set_constants(dxrs_amd.types.graphics_settings(w, h, bounces=8, spp=1))
            gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device=dev) for n in RESTIR_DI_INPUTS}
            dd, ds = (torch.zeros((h, w, 4), dtype=torch.float32, device=dev) for _ in range(2))
            torch.cuda.synchronize(dev)
            gptrs = {n: b.data_ptr() for n, b in gb.items()}
            bufs = dict(gptrs, Diffuse=dd.data_ptr(), Specular=ds.data_ptr())
            r.render_gbuffer_device(gptrs)
            r.synchronize()
            r.set_profiling(True)
            stage = {}
            for name, ls in MODES:
                pre, l1, l2, wall = timed(r, w, h, bufs, ls, args.frames, args.warmup)
                stage[name] = float(np.median(pre))
                summary(res, f"{name}_{size}_presampling", pre)
                summary(res, f"{name}_{size}_launch1", l1)
                summary(res, f"{name}_{size}_launch2", l2)
                summary(res, f"{name}_{size}_wall", wall)
            pre, _, _, _ = timed(r, w, h, bufs, dict(mode=LIGHT_SAMPLING_POWER_RIS, tile_size=1, tile_count=1), args.frames, args.warmup)
            summary(res, f"stage_pyramid_{size}", pre)
            res[f"stage_power_segment_{size}_ms"] = round(stage["power"] - float(np.median(pre)), 4)
            res[f"stage_regir_segment_{size}_ms"] = round(stage["regir"] - stage["power"], 4)
            r.set_profiling(False)
            if (w, h) == min(sizes, key=lambda s: s[0] * s[1]) and args.reference_frames:
                lum = torch.tensor([0.2126, 0.7152, 0.0722, 0.0], device=dev)

                def image(k, ls):
                    dd.zero_(); ds.zero_()
                    torch.cuda.synchronize(dev)
                    r.restir_di_device(w, h, bufs, frame_index=k, reset_history=True, temporal=False, spatial=False, light_sampling=ls)
                    r.synchronize()
                    return ((dd + ds) * lum).sum(-1).double()
                mean = torch.zeros((h, w), dtype=torch.float64, device=dev)
                for k in range(args.reference_frames):
                    mean += image(100000 + k, None)
                mean /= args.reference_frames
                for name, ls in MODES:
                    err = [float(((image(k, ls) - mean) ** 2).mean().sqrt()) for k in range(16)]
                    res[f"rmse_{name}_{size}"] = round(float(np.mean(err)), 6)
                res["rmse_reference_frames"] = args.reference_frames
        finally:
            r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
