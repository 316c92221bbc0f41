#!/usr/bin/env python3
"""Time pt_nrd_reblur (row N30, the ReBLUR stand-in) with device events and print one JSON line.  Inputs are the C2 scene's real
G-buffer guides and ReBLUR-packed N7 outputs (demo scene seed 0, 1 spp, 8 bounces, resting camera) at each size.

Per size, interleaved in one process (call by call, so that clocks and cache state are shared): pt_nrd_reblur, pt_nrd_denoise in ReBLUR
mode with 5 a-trous steps, pt_nrd_reblur with RESTART (no history: every lobe goes through the history fix and blurs at its largest
radius, what a frame after a cut costs) and a float4 device-to-device copy moving the byte model's bytes (half read, half written);
the median of --calls single-call event timings each; the first two CONTINUE after --warmup rounds, so their history is full (the
camera rests and the G-buffer's motion vectors are 0), with a changing FrameIndex.

Byte model per pass (what each pixel loads and stores once; the neighbour taps are counted as served by the caches):
  (a) temporal hit:  ViewZ 4 + MotionVector 12 + NormalRoughness 16 + In 2 x 16 + previous slot 5 x 16 read, work 2 x 16 + fast 2 x 16 +
                     guide 16 written = 224 B; miss: 4 read + 7 x 16 written = 116 B
  (b) fix and clamp: ViewZ 4 + work 2 x 16 + fast 2 x 16 read, slow 2 x 16 written = 100 B; miss: 4 B
  (c) blur:          ViewZ 4 + NormalRoughness 16 + slow 2 x 16 + history lengths 8 read, work 2 x 16 written = 92 B; miss: 4 B
  (d) post-blur:     ViewZ 4 + NormalRoughness 16 + work 2 x 16 + history lengths 8 read, Out 2 x 16 + slow 2 x 16 written = 124 B; miss: 4 B
History and work buffers: 2 slots x 5 float4 + 2 float4 = 192 B per pixel (pt_nrd_denoise: 200 B).
Per-pass kernel durations without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_nrd_reblur.py`
(rb_temporal_kernel, rb_fix_kernel, rb_blur_kernel<false>, rb_blur_kernel<true>).

    python tools/bench_nrd_reblur.py [--calls 200 --warmup 30 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

REBLUR = 2
GUIDES = ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "MotionVector")
BYTES_PER_PIXEL = 2 * 5 * 16 + 2 * 16


def byte_model(n, hits):
    miss = n - hits
    passes = {"temporal": 224 * hits + 116 * miss, "fix_clamp": 100 * hits + 4 * miss, "blur": 92 * hits + 4 * miss, "post_blur": 124 * hits + 4 * miss}
    return dict(passes, call=sum(passes.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
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
    res = {"metric": "pt_nrd_reblur", "calls": args.calls, "statistic": "median of single-call device-event timings, the three interleaved",
           "history_and_work_bytes_per_pixel": BYTES_PER_PIXEL, "sizes": {}}
    width = dict(t.GBUFFER_CHANNELS)
    for s in args.sizes.split(","):
        w, h = map(int, s.split("x"))
        n = w * h
        r.set_camera(host.camera_matrices(w, h, jitter=False))  # (with the matrices the G-buffer's MotionVector needs)
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        b = {k: torch.zeros((n, width[k]), dtype=torch.float32, device="cuda") for k in GUIDES}
        b.update({k: torch.zeros((n, 4), dtype=torch.float32, device="cuda") for k in ("Radiance", "NoisyDiffuse", "NoisySpecular", "OutDiffuse", "OutSpecular")})
        torch.cuda.synchronize()
        r.render_gbuffer_device({k: b[k].data_ptr() for k in GUIDES})
        r.render_denoiser_device(REBLUR, b["Radiance"].data_ptr(), {"Diffuse": b["NoisyDiffuse"].data_ptr(), "Specular": b["NoisySpecular"].data_ptr()})
        r.nrd_composition_device(REBLUR, True, w, h, dict({k: b[k].data_ptr() for k in GUIDES[:4]}, NoisyDiffuse=b["NoisyDiffuse"].data_ptr(),
                                                          NoisySpecular=b["NoisySpecular"].data_ptr()))
        r.synchronize()
        hits = int(torch.isfinite(b["LinearDepth"]).sum().item())
        p = dict(ViewZ=b["LinearDepth"].data_ptr(), MotionVector=b["MotionVector"].data_ptr(), NormalRoughness=b["NormalRoughness"].data_ptr(),
                 InDiffuse=b["NoisyDiffuse"].data_ptr(), InSpecular=b["NoisySpecular"].data_ptr(), OutDiffuse=b["OutDiffuse"].data_ptr(),
                 OutSpecular=b["OutSpecular"].data_ptr())
        model = byte_model(n, hits)
        src = torch.empty((model["call"] // 32, 4), dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        frame = [0]

        def reblur():
            r.nrd_reblur_device(w, h, p, frame_index=frame[0])
            frame[0] += 1

        fns = {"pt_nrd_reblur": reblur, "pt_nrd_denoise": lambda: r.nrd_denoise_device(REBLUR, w, h, p), "copy": lambda: dst.copy_(src)}
        r.nrd_reblur_device(w, h, p, accumulation_mode=2)
        r.nrd_denoise_device(REBLUR, w, h, p, accumulation_mode=2)
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)] for k in fns}
        for i in range(args.calls):
            for k, fn in fns.items():
                a, e = ev[k][i]
                a.record(stream)
                fn()
                e.record(stream)
        torch.cuda.synchronize()
        ms = {k: float(np.median([a.elapsed_time(e) for a, e in v])) for k, v in ev.items()}
        n_hist = float(np.median(r.nrd_reblur_history(w, h)["fast_s"][..., 3][b["LinearDepth"].reshape(h, w).isfinite().cpu().numpy()]))
        rev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
        for a, e in rev:  # (a block of its own: a RESTART among the others would empty their history)
            a.record(stream)
            r.nrd_reblur_device(w, h, p, accumulation_mode=1, frame_index=frame[0])
            e.record(stream)
        torch.cuda.synchronize()
        ms["restart"] = float(np.median([a.elapsed_time(e) for a, e in rev]))
        rate, copy_rate = model["call"] / (ms["pt_nrd_reblur"] * 1e-3), 2 * src.numel() * 4 / (ms["copy"] * 1e-3)
        res["sizes"][s] = {"hit_fraction": round(hits / n, 4), "specular_history_length_median": n_hist, "pt_nrd_reblur_ms": round(ms["pt_nrd_reblur"], 5),
                           "pt_nrd_reblur_restart_ms": round(ms["restart"], 5), "pt_nrd_denoise_reblur_mode_5_steps_ms": round(ms["pt_nrd_denoise"], 5), "copy_ms": round(ms["copy"], 5), "bytes": model,
                           "call_TBps": round(rate / 1e12, 3), "copy_TBps": round(copy_rate / 1e12, 3), "call_fraction_of_copy": round(rate / copy_rate, 3),
                           "reblur_over_denoise": round(ms["pt_nrd_reblur"] / ms["pt_nrd_denoise"], 3)}
        del src, dst, b
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
