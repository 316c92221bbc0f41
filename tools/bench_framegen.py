#!/usr/bin/env python3
"""Time pt_frame_gen (row N13, the DLSS-G stand-in) with device events and print one JSON line.  The inputs are two frames of the C2
scene (demo scene seed 0, 1 spp, 8 bounces) seen by a travelling camera: the second frame's tone-mapped colour, LinearDepth and
MotionVector, with the first frame as the history, so the vectors are real and the scatter has collisions and holes.

Per shape (1920x1080 and 3840x2160, each at 1:1 and from a half-size G-buffer): the median of --calls single-call event timings of a
generating call (clear + scatter + gather) and of a restart (three copies); the byte model; the achieved rate against a device-to-device
copy that moves the same number of bytes (half of them read, half written), timed the same way in the same process.  Then the post chain
[pt_upscale ->] pt_bloom -> pt_tonemap at each shape with and without pt_frame_gen behind it, per frame.

Byte model (what is loaded and stored once): per output pixel the colour and the previous colour read, the history and the output
written (16 B); per render pixel the field cleared (8 B), one 8-byte atomic, depth and vector read by the scatter (16 B), the depth's
history written (4 B), the field entry, the winner's vector and depth and one previous depth read by the gather (28 B) = 64 B.  Not
counted: the other three targets of a moving pixel's scatter, and the eight colour taps of the gather, which neighbouring lanes share
through the caches.
The two kernels' durations without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_framegen.py`
(framegen_scatter_kernel, framegen_gather_kernel; the clear is the runtime's fill kernel).

    python tools/bench_framegen.py [--calls 200 --warmup 30 --frames 50 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

BYTES_PER_OUTPUT_PIXEL, BYTES_PER_RENDER_PIXEL = 16, 64


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
    tm = t.tonemap_params()
    res = {"metric": "pt_frame_gen", "calls": args.calls, "statistic": "median of single-call device-event timings",
           "bytes_per_output_pixel": BYTES_PER_OUTPUT_PIXEL, "bytes_per_render_pixel": BYTES_PER_RENDER_PIXEL, "shapes": {}, "post_chain_ms": {}}
    for W, H in [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")]:
        N = W * H
        for w, h in ((W, H), (W // 2, H // 2)):
            n = w * h
            small = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            full = torch.zeros((N, 4), dtype=torch.float32, device="cuda") if n != N else small
            depth = torch.zeros(n, dtype=torch.float32, device="cuda")
            mv = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            ldr = torch.zeros(N, dtype=torch.int32, device="cuda")
            mid = torch.zeros(N, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            fg = dict(Color=ldr.data_ptr(), Depth=depth.data_ptr(), MotionVector=mv.data_ptr(), Output=mid.data_ptr())
            up = dict(Color=small.data_ptr(), Depth=depth.data_ptr(), Velocity=mv.data_ptr(), Output=full.data_ptr())

            def post(generate):
                if n != N:
                    r.upscale_device((w, h), (W, H), up)
                r.bloom(full.data_ptr(), full.data_ptr(), W, H, 0.05)
                r.tonemap(full.data_ptr(), N, tm, ldr.data_ptr())
                if generate:
                    r.frame_gen_device((w, h), (W, H), fg)

            # two frames of a travelling camera; the second one's buffers stay for the timed calls
            cam = None
            for f in range(2):
                cam = host.camera_matrices(w, h, position=(0.4 * f, 0.15 * f, -15.0 + 0.3 * f), look_at=(0.0, 0.0, 0.0), jitter=False, previous=cam)
                r.set_camera(cam)
                r.set_constants(t.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
                r.render_gbuffer_device(dict(LinearDepth=depth.data_ptr(), MotionVector=mv.data_ptr()))
                r.render_device(small.data_ptr())
                post(False)
                r.frame_gen_device((w, h), (W, H), fg, reset=f == 0)
            r.synchronize()
            z = depth.cpu().numpy()
            moving = float(np.abs(mv.cpu().numpy()[np.isfinite(z)][:, :2]).max(axis=1).mean()) if np.isfinite(z).any() else 0.0
            call_ms = median_ms(stream, lambda: r.frame_gen_device((w, h), (W, H), fg), args.calls, args.warmup)
            restart_ms = median_ms(stream, lambda: r.frame_gen_device((w, h), (W, H), fg, reset=True), args.calls, args.warmup)
            r.frame_gen_device((w, h), (W, H), fg)
            model = BYTES_PER_OUTPUT_PIXEL * N + BYTES_PER_RENDER_PIXEL * n
            src = torch.zeros(model // 8, dtype=torch.float32, device="cuda")
            dst = torch.zeros(model // 8, dtype=torch.float32, device="cuda")
            copy_ms = median_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup)
            rate, copy_rate = model / (call_ms * 1e-3), model / (copy_ms * 1e-3)
            plain = mean_ms(stream, lambda: post(False), args.frames, 10)
            generating = mean_ms(stream, lambda: post(True), args.frames, 10)
            key = f"{w}x{h}:{W}x{H}"
            res["shapes"][key] = {"call_ms": round(call_ms, 5), "restart_ms": round(restart_ms, 5), "bytes": model, "call_TBps": round(rate / 1e12, 3),
                                  "copy_ms": round(copy_ms, 5), "copy_TBps": round(copy_rate / 1e12, 3), "call_fraction_of_copy": round(rate / copy_rate, 3),
                                  "mean_vector_px_on_surfaces": round(moving, 3), "surface_share": round(float(np.isfinite(z).mean()), 4)}
            chain = ("upscale_" if n != N else "") + "bloom_tonemap"
            res["post_chain_ms"][key] = {chain: round(plain, 5), chain + "_framegen": round(generating, 5), "difference": round(generating - plain, 5)}
            del small, full, depth, mv, ldr, mid, src, dst
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
