#!/usr/bin/env python3
"""Time pt_nis_sharpen (row N12, the NIS stand-in) with device events and print one JSON line.  The input is the C2 scene's real
radiance (demo scene seed 0, 1 spp, 8 bounces) at each size.

Per size: the median of --calls single-call event timings for HdrMode None and Linear; the byte model; the achieved rate against a
float4 device-to-device copy of the same size (one float4 read and one written per texel) timed the same way in the same process.
Then the post chain pt_upscale -> pt_nis_sharpen -> pt_bloom -> pt_tonemap at each output size, from a half-size frame, with and
without the pass, per frame.

Byte model (what each texel loads and stores once): the colour's float4 read (16 B) and the output's float4 written (16 B) = 32 B.  Not
counted: a workgroup stages the lumas of 36 x 12 texels for the 32 x 8 it owns, so 1.69 float4 loads are issued per texel, and each
lane reads its own colour once more; the caches serve those.
The kernel's duration without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_nis.py`
(nis_kernel<hdr mode>).

    python tools/bench_nis.py [--calls 200 --warmup 30 --frames 50 --sizes 1920x1080,3840x2160]"""
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
    ap.add_argument("--sharpness", type=float, default=0.5)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    res = {"metric": "pt_nis_sharpen", "calls": args.calls, "statistic": "median of single-call device-event timings", "sharpness": args.sharpness,
           "bytes_per_texel": BYTES_PER_TEXEL, "sizes": {}, "post_chain_ms": {}}
    for W, H in [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")]:
        n = W * H
        color = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_camera(host.camera(W, H, jitter_index=0))
        r.set_constants(t.graphics_settings(W, H, bounces=8, spp=1))
        r.render_device(color.data_ptr())
        r.synchronize()
        p = dict(Color=color.data_ptr(), Output=out.data_ptr())
        ms = {name: median_ms(stream, lambda m=mode: r.nis_sharpen_device((W, H), p, sharpness=args.sharpness, hdr_mode=m), args.calls, args.warmup)
              for name, mode in (("none", t.NIS_HDR_NONE), ("linear", t.NIS_HDR_LINEAR))}
        copy_ms = median_ms(stream, lambda: out.copy_(color), args.calls, args.warmup)
        model = BYTES_PER_TEXEL * n
        rate, copy_rate = model / (ms["none"] * 1e-3), model / (copy_ms * 1e-3)
        res["sizes"][f"{W}x{H}"] = {"call_ms": round(ms["none"], 5), "call_linear_ms": round(ms["linear"], 5), "bytes": model,
                                    "call_TBps": round(rate / 1e12, 3), "copy_ms": round(copy_ms, 5), "copy_TBps": round(copy_rate / 1e12, 3),
                                    "call_fraction_of_copy": round(rate / copy_rate, 3)}
        # the post chain from a half-size frame: pt_upscale -> [pt_nis_sharpen] -> pt_bloom -> pt_tonemap
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

        def chain(sharpen):
            def fn():
                r.upscale_device((w, h), (W, H), up, jitter=jit)
                src = color
                if sharpen:
                    r.nis_sharpen_device((W, H), p, sharpness=args.sharpness)
                    src = out
                r.bloom(src.data_ptr(), src.data_ptr(), W, H, 0.05)
                r.tonemap(src.data_ptr(), n, tm, ldr.data_ptr())
            return fn

        plain = mean_ms(stream, chain(False), args.frames, 10)
        sharpened = mean_ms(stream, chain(True), args.frames, 10)
        res["post_chain_ms"][f"{w}x{h}:{W}x{H}"] = {"upscale_bloom_tonemap": round(plain, 5), "upscale_nis_bloom_tonemap": round(sharpened, 5),
                                                    "difference": round(sharpened - plain, 5)}
        del color, out, small, depth, velocity, ldr
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
