#!/usr/bin/env python3
"""Time pt_render_with_di (a frame whose direct illumination the caller supplies) against pt_render without DI and with row N4's own
DI estimate, on the C2 workload (demo scene seed 0, 8 bounces, 1 spp, jitter 0 of 8), and print one JSON line.

Per size and frame kind: the median (and the 10-90 % spread) of --frames one-frame-at-a-time timings (PtStats.ms_total: the frame's
events on its lane, the DI gather included) after --warmup frames, one context, the three kinds back to back.  The supplied DI is
random and non-negative.  Byte model of the gather in front of the frame: 32 B read + 16 B written per slot.
Kernel durations without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_render_with_di.py`.

    python tools/bench_render_with_di.py [--frames 200 --warmup 30 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402


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
    res = {"workload": "demo scene seed 0, 8 bounces, 1 spp, one frame at a time", "frames": args.frames}
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = dxrs_amd.Renderer(device=0)
        try:
            r.set_scene(spheres, mats, sd)
            r.set_camera(host.camera(w, h, jitter_index=0, jitter_count=8))
            out = torch.zeros((h, w, 4), device=dev)
            dd, ds = torch.rand((h, w, 4), device=dev), torch.rand((h, w, 4), device=dev)
            torch.cuda.synchronize(dev)
            for kind in ("render", "render_n4", "render_with_di"):
                r.set_constants(dxrs_amd.types.graphics_settings(w, h, bounces=8, spp=1, di=kind == "render_n4"))
                ms = []
                for k in range(args.warmup + args.frames):
                    if kind == "render_with_di":
                        st = r.render_with_di_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr(), want_stats=True)
                    else:
                        st = r.render_device(out.data_ptr(), want_stats=True)
                    if k >= args.warmup:
                        ms.append(st.ms_total)
                res[f"{kind}_{size}_ms"] = round(float(np.median(ms)), 4)
                res[f"{kind}_{size}_spread_ms"] = round(float(np.percentile(ms, 90) - np.percentile(ms, 10)), 4)
            res[f"gather_{size}_bytes"] = 48 * ((w + 7) // 8) * ((h + 7) // 8) * 64
        finally:
            r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
