#!/usr/bin/env python3
"""Time pt_chromatic_aberration (row N29) with device events and print one JSON line.  The input is the C2 scene's real radiance (demo
scene seed 0, 1 spp, 8 bounces) at each size.

Per size: the median of --calls single-call event timings with the default offsets (0.003, 0.003, -0.003) and with the extreme ones
(+1/16, -1/16, +1/16); the byte model; the achieved rate against a float4 device-to-device copy of the same size (one float4 read
and one written per texel) timed the same way in the same process.  Then the post chain pt_upscale -> pt_nis_sharpen ->
[pt_chromatic_aberration] -> pt_bloom -> pt_tonemap at each output size, from a half-size frame, with and without the pass, per frame.

Byte model (what each texel loads and stores once): the colour's float4 read (16 B) and the output's float4 written (16 B) = 32 B.  Not
counted: a workgroup stages 35 x 10 scalars per channel for the 32 x 8 texels it owns, 1.37 dword loads per texel and channel, and
each lane reads its own alpha; the caches serve those.
The kernel's duration without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_chromatic_aberration.py`
(chromab_kernel).

    python tools/bench_chromatic_aberration.py [--calls 200 --warmup 30 --frames 50 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

BYTES_PER_TEXEL = 32
EXTREME_OFFSETS = (0.0625, -0.0625, 0.0625)


def median_ms(stream, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def mean_ms(stream, fn, calls, warmup):
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=50, help="frames timed through the post chain with and without the pass")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    default = tuple(t.CHROMATIC_ABERRATION_OFFSETS)
    res = {"metric": "pt_chromatic_aberration", "calls": args.calls, "statistic": "median of single-call device-event timings",
           "offsets_default": default, "offsets_extreme": EXTREME_OFFSETS, "bytes_per_texel": BYTES_PER_TEXEL, "sizes": {}, "post_chain_ms": {}}
    for W, H in [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")]:
        n = W * H
        color = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        sharp = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_camera(host.camera(W, H, jitter_index=0))
        r.set_constants(t.graphics_settings(W, H, bounces=8, spp=1))
        r.render_device(color.data_ptr())
        r.synchronize()
        p = dict(Color=color.data_ptr(), Output=out.data_ptr())
        ms = {name: median_ms(stream, lambda k=k: r.chromatic_aberration_device((W, H), p, offsets=k), args.calls, args.warmup)
              for name, k in (("default", default), ("extreme", EXTREME_OFFSETS))}
        copy_ms = median_ms(stream, lambda: out.copy_(color), args.calls, args.warmup)
        model = BYTES_PER_TEXEL * n
        rate, rate_x, copy_rate = model / (ms["default"] * 1e-3), model / (ms["extreme"] * 1e-3), model / (copy_ms * 1e-3)
        res["sizes"][f"{W}x{H}"] = {"call_ms": round(ms["default"], 5), "call_extreme_ms": round(ms["extreme"], 5), "bytes": model,
                                    "call_TBps": round(rate / 1e12, 3), "call_extreme_TBps": round(rate_x / 1e12, 3), "copy_ms": round(copy_ms, 5),
                                    "copy_TBps": round(copy_rate / 1e12, 3), "call_fraction_of_copy": round(rate / copy_rate, 3),
                                    "call_extreme_fraction_of_copy": round(rate_x / copy_rate, 3)}
        # the post chain from a half-size frame: pt_upscale -> pt_nis_sharpen -> [pt_chromatic_aberration] -> pt_bloom -> pt_tonemap
        w, h = W // 2, H // 2
        small = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
        depth = torch.zeros(h * w, dtype=torch.float32, device="cuda")
        velocity = torch.zeros((h * w, 3), dtype=torch.float32, device="cuda")
        ldr = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cam = host.camera_matrices(w, h, jitter_index=0, jitter_count=32)
        r.set_camera(cam)
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        r.render_gbuffer_device(dict(LinearDepth=depth.data_ptr(), MotionVector=velocity.data_ptr()))
        r.render_device(small.data_ptr())
        r.synchronize()
        up = dict(Color=small.data_ptr(), Depth=depth.data_ptr(), Velocity=velocity.data_ptr(), Output=color.data_ptr())
        jit = (-cam.Jitter[0], -cam.Jitter[1])
        tm = t.tonemap_params()

        def chain(fringe):
            def fn():
                r.upscale_device((w, h), (W, H), up, jitter=jit)
                r.nis_sharpen_device((W, H), dict(Color=color.data_ptr(), Output=sharp.data_ptr()), sharpness=0.5)
                src = sharp
                if fringe:
                    r.chromatic_aberration_device((W, H), dict(Color=sharp.data_ptr(), Output=out.data_ptr()))
                    src = out
                r.bloom(src.data_ptr(), src.data_ptr(), W, H, 0.05)
                r.tonemap(src.data_ptr(), n, tm, ldr.data_ptr())
            return fn

        plain = mean_ms(stream, chain(False), args.frames, 10)
        fringed = mean_ms(stream, chain(True), args.frames, 10)
        res["post_chain_ms"][f"{w}x{h}:{W}x{H}"] = {"upscale_nis_bloom_tonemap": round(plain, 5), "upscale_nis_chromab_bloom_tonemap": round(fringed, 5),
                                                    "difference": round(fringed - plain, 5)}
        del color, sharp, out, small, depth, velocity, ldr
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
