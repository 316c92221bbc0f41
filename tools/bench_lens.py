#!/usr/bin/env python3
"""Time pt_render_lens (row N26, the thin-lens camera) with device events and print one JSON line.  The scene is C2 (demo scene seed 0,
8 bounces, a resting camera without jitter, in focus at view depth 15, where the demo's spheres are).

Per size (1920x1080 and 3840x2160) and per sample count (1 and 16 spp), in one process and alternating over --rounds rounds so that
drift hits all alike: pt_render_lens at ApertureRadius 0 and 0.05, pt_render, and pt_render_sharc with stage QUERY only over an empty
cache (the same loop without the lens, one primary ray per pixel).  Per variant: the median of all its single-call event timings, the
smallest and largest of its per-round medians (the run-to-run spread inside this process), and the rays of one frame.

    python tools/bench_lens.py [--calls 20 --warmup 5 --rounds 3 --sizes 1920x1080,3840x2160 --spp 1,16]"""
import argparse
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

QUERY = 4
FOCUS, APERTURE = 15.0, 0.05


def timings_ms(stream, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls per variant and round (a quarter of it at 16 spp)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--spp", default="1,16")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    res = {"metric": "pt_render_lens", "statistic": "median of single-call device-event timings; spread = smallest and largest per-round median", "calls_per_round": args.calls,
           "rounds": args.rounds, "focus_distance": FOCUS, "aperture": APERTURE, "sizes": {}}
    frame = [0]
    for W, H in [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")]:
        out = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        base = host.camera_matrices(W, H, jitter=False)
        k = FOCUS / float(np.sqrt(sum(float(x) ** 2 for x in base.ForwardDirection)))  # what CameraController::SetFocusDistance does
        for v in (base.RightDirection, base.UpDirection, base.ForwardDirection):
            for i in range(3):
                v[i] = v[i] * k
        cams = {0.0: copy.copy(base), APERTURE: copy.copy(base)}
        cams[APERTURE].ApertureRadius = APERTURE
        size = {}
        for spp in [int(s) for s in args.spp.split(",")]:
            calls = max(args.calls // 4, 3) if spp >= 8 else args.calls

            def next_frame():
                frame[0] += 1
                r.set_constants(t.graphics_settings(W, H, frame_index=frame[0], bounces=8, spp=spp))

            def lens():
                next_frame()
                r.render_lens_device(out.data_ptr())

            def plain():
                next_frame()
                r.render_device(out.data_ptr())

            def query():
                next_frame()
                r.render_sharc_device(out.data_ptr(), stages=QUERY, reset_history=True, capacity=1 << 16)

            # name -> (the camera's aperture, the call); pt_render and the query ignore the aperture
            variants = {"pt_render_lens_aperture_0": (0.0, lens), f"pt_render_lens_aperture_{APERTURE}": (APERTURE, lens), "pt_render": (0.0, plain),
                        "pt_render_sharc_query_empty_cache": (0.0, query)}
            samples = {name: [] for name in variants}
            for _ in range(args.rounds):
                for name, (aperture, fn) in variants.items():
                    r.set_camera(cams[aperture])
                    samples[name].append(timings_ms(stream, fn, calls, args.warmup))
            row = {}
            for name, rounds in samples.items():
                meds = [float(np.median(x)) for x in rounds]
                row[name + "_ms"] = round(float(np.median(np.concatenate(rounds))), 5)
                row[name + "_spread_ms"] = [round(min(meds), 5), round(max(meds), 5)]
            next_frame()
            r.set_camera(cams[0.0])
            row["rays_lens_aperture_0"] = int(r.render_lens_device(out.data_ptr(), want_stats=True).rays)
            row["rays_pt_render"] = int(r.render_device(out.data_ptr(), want_stats=True).rays)
            row["rays_query_empty_cache"] = int(r.render_sharc_device(out.data_ptr(), want_stats=True, stages=QUERY, reset_history=True, capacity=1 << 16).rays)
            r.set_camera(cams[APERTURE])
            row[f"rays_lens_aperture_{APERTURE}"] = int(r.render_lens_device(out.data_ptr(), want_stats=True).rays)
            size[f"{spp}spp"] = row
        res["sizes"][f"{W}x{H}"] = size
        del out
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
