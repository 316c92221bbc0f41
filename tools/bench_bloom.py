#!/usr/bin/env python3
"""Time pt_bloom (row N5) with device events and print one JSON line: ms per call at each size, launches per call, the
byte model, and the C2 frame (pt_render -> [pt_bloom ->] pt_tonemap) with and without bloom.

Byte model (fp32 RGBA, 16 B a texel; W x H input, chain level k of w_k x h_k):
  minimum  = the input read twice (chain step 1 and the merge) + the output written once + level 0 written and read once
  steps    = what the 10 launches move if every launch reads its source once and writes its destination once

    python tools/bench_bloom.py [--calls 300 --warmup 30 --frames 100 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

TEXEL = 16
LAUNCHES = 10  # 5 downsamples, 4 upsamples, the merge


def chain(w, h):
    return [(max(1, (w // 2) >> k), max(1, (h // 2) >> k)) for k in range(5)]


def byte_model(w, h):
    c = [a * b for a, b in chain(w, h)]
    full = w * h
    minimum = TEXEL * (2 * full + full + 2 * c[0])
    steps = full + c[0]                                   # step 1
    steps += sum(c[k - 1] + c[k] for k in range(1, 5))    # steps 2-5
    steps += sum(c[k + 1] + c[k] for k in range(3, -1, -1))  # steps 6-9
    steps += full + c[0] + full                           # merge
    return minimum, TEXEL * steps


def time_calls(stream, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(calls):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=100, help="C2 frames timed with and without bloom")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--strength", type=float, default=0.05)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    rng = np.random.default_rng(0)
    res = {"metric": "pt_bloom", "launches_per_call": LAUNCHES, "calls": args.calls, "sizes": {}}
    for s in args.sizes.split(","):
        w, h = map(int, s.split("x"))
        img = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (h * w, 4))).astype(np.float32)
        d_in = torch.from_numpy(img).cuda()
        d_out = torch.empty_like(d_in)
        ms = time_calls(stream, lambda: r.bloom(d_in.data_ptr(), d_out.data_ptr(), w, h, args.strength), args.calls, args.warmup)
        minimum, steps = byte_model(w, h)
        res["sizes"][s] = {"ms": round(ms, 5), "bytes_min": minimum, "bytes_steps": steps, "us_at_8TBps_min": round(minimum / 8e12 * 1e6, 2),
                           "us_at_8TBps_steps": round(steps / 8e12 * 1e6, 2), "effective_TBps_min": round(minimum / (ms * 1e-3) / 1e12, 3),
                           "effective_TBps_steps": round(steps / (ms * 1e-3) / 1e12, 3)}
    # C2: demo scene, 1920x1080, 1 spp, 8 bounces; render -> [bloom ->] tonemap (ACES + sRGB) every frame
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    w, h = 1920, 1080
    r.set_scene(spheres, materials, sd)
    r.set_camera(host.camera(w, h))
    gs = t.graphics_settings(w, h, bounces=8, spp=1)
    frame = torch.empty((w * h, 4), dtype=torch.float32, device="cuda")
    bloomed = torch.empty_like(frame)
    ldr = torch.empty(w * h, dtype=torch.int32, device="cuda")
    tm = t.tonemap_params(t.TONE_ACES_FILMIC, t.TRANSFER_SRGB, 0.0)
    counter = [0]

    def frame_fn(bloom):
        def fn():
            gs.FrameIndex = counter[0]
            counter[0] += 1
            r.set_constants(gs)
            r.render_device(frame.data_ptr())
            src = frame
            if bloom:
                r.bloom(frame.data_ptr(), bloomed.data_ptr(), w, h, args.strength)
                src = bloomed
            r.tonemap(src.data_ptr(), w * h, tm, ldr.data_ptr())
        return fn

    without = time_calls(stream, frame_fn(False), args.frames, 10)
    with_bloom = time_calls(stream, frame_fn(True), args.frames, 10)
    res["c2_frame_ms"] = {"render_tonemap": round(without, 5), "render_bloom_tonemap": round(with_bloom, 5), "bloom_share_ms": round(with_bloom - without, 5)}
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
