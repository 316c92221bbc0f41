#!/usr/bin/env python3
"""Time pt_upscale (row N11, the super-resolution stand-in) with device events and print one JSON line.  Inputs are the C2 scene's real
radiance, LinearDepth and MotionVector (demo scene seed 0, 1 spp, 8 bounces, resting camera, Halton jitter) at each input size.

Per shape: the median of --calls single-call event timings of the call with its history running; the byte model; the achieved rate
against a float4 device-to-device copy of the same byte count timed the same way in the same process.  Then the chain at each output
size -- pt_render_gbuffer (LinearDepth, MotionVector) + pt_render at the input size + pt_upscale -- against pt_render at the output size,
per frame, one lane.

Byte model (what each pixel loads and stores once; the 3 x 3 taps are staged in LDS, the history's bilinear footprint is counted as
served by the caches): per input pixel the 28 B a workgroup stages (colour rgb 12, Depth 4, Velocity 12; the alpha rides in the colour's
float4 load) read; per output pixel history 16 + 4 read, history 16 + 4 and Output 16 written.  Not counted: the output's alpha, which each
lane reads again from the Color line its workgroup just staged.
The kernel's duration without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_upscale.py`
(upscale_kernel<restart>).

    python tools/bench_upscale.py [--calls 200 --warmup 30 --frames 50 --shapes 960x540:1920x1080,1920x1080:3840x2160,1280x720:1920x1080]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402


def byte_model(n_in, n_out):
    return 28 * n_in + (20 + 36) * n_out


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


def buffers(w, h, W, H):
    b = dict(Color=torch.zeros((h * w, 4), dtype=torch.float32, device="cuda"), Depth=torch.zeros(h * w, dtype=torch.float32, device="cuda"),
             Velocity=torch.zeros((h * w, 3), dtype=torch.float32, device="cuda"), Output=torch.zeros((H * W, 4), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=50, help="C2 frames timed with the chain and with pt_render alone")
    ap.add_argument("--shapes", default="960x540:1920x1080,1920x1080:3840x2160,1280x720:1920x1080")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    res = {"metric": "pt_upscale", "calls": args.calls, "statistic": "median of single-call device-event timings", "shapes": {}, "c2_frame_ms": {}}
    shapes = [tuple(tuple(map(int, s.split("x"))) for s in shape.split(":")) for shape in args.shapes.split(",")]
    for (w, h), (W, H) in shapes:
        cam = host.camera_matrices(w, h, jitter_index=0, jitter_count=32)
        r.set_camera(cam)
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        b = buffers(w, h, W, H)
        r.render_gbuffer_device(dict(LinearDepth=b["Depth"].data_ptr(), MotionVector=b["Velocity"].data_ptr()))
        r.render_device(b["Color"].data_ptr())
        r.synchronize()
        p = {k: v.data_ptr() for k, v in b.items()}
        jit = (-cam.Jitter[0], -cam.Jitter[1])
        r.upscale_device((w, h), (W, H), p, jitter=jit, reset=True)
        ms = median_ms(stream, lambda: r.upscale_device((w, h), (W, H), p, jitter=jit), args.calls, args.warmup)
        ms_reset = median_ms(stream, lambda: r.upscale_device((w, h), (W, H), p, jitter=jit, reset=True), args.calls, args.warmup)
        model = byte_model(w * h, W * H)
        src = torch.empty((model // 32, 4), dtype=torch.float32, device="cuda")  # a copy moving the same bytes: half read, half written
        dst = torch.empty_like(src)
        copy_ms = median_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup)
        rate, copy_rate = model / (ms * 1e-3), 2 * src.numel() * 4 / (copy_ms * 1e-3)
        res["shapes"][f"{w}x{h}:{W}x{H}"] = {"call_ms": round(ms, 5), "call_reset_ms": round(ms_reset, 5), "bytes": model, "call_TBps": round(rate / 1e12, 3),
                                             "copy_ms": round(copy_ms, 5), "copy_TBps": round(copy_rate / 1e12, 3),
                                             "call_fraction_of_copy": round(rate / copy_rate, 3)}
        del src, dst
        # the chain against pt_render at the output size: one lane, a new frame index and jitter per frame, resting camera
        full = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        counter = [0]

        def chain(upscale):
            def fn():
                k = counter[0]
                counter[0] += 1
                size = (w, h) if upscale else (W, H)
                c = host.camera_matrices(*size, jitter_index=k, jitter_count=32)
                r.set_camera(c)
                r.set_constants(t.graphics_settings(*size, frame_index=k, bounces=8, spp=1))
                if not upscale:
                    r.render_device(full.data_ptr())
                    return
                r.render_gbuffer_device(dict(LinearDepth=p["Depth"], MotionVector=p["Velocity"]))
                r.render_device(p["Color"])
                r.upscale_device((w, h), (W, H), p, jitter=(-c.Jitter[0], -c.Jitter[1]))
            return fn

        render = mean_ms(stream, chain(False), args.frames, 10)
        chained = mean_ms(stream, chain(True), args.frames, 10)
        res["c2_frame_ms"][f"{w}x{h}:{W}x{H}"] = {"pt_render_at_output_size": round(render, 5), "gbuffer_render_upscale": round(chained, 5),
                                                  "ratio": round(chained / render, 3)}
        del b, full
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
