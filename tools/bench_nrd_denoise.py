#!/usr/bin/env python3
"""Time pt_nrd_denoise (row N9, the NRD stand-in) with device events and print one JSON line.  Inputs are the C2 scene's real G-buffer
guides and packed N7 outputs (demo scene seed 0, 1 spp, 8 bounces, resting camera) at each size, for NRDReBLUR and NRDReLAX.

Per size and mode: the median of --calls single-call event timings of the whole call (CONTINUE after --warmup calls, 5 a-trous steps)
and of the same call with 1 a-trous step, whose difference gives the four steps 2..5; the byte model per pass; the achieved rate of the
whole call against a float4 device-to-device copy of the same byte count timed the same way in the same process.  Then the C2 chain
(pt_render_gbuffer + pt_render_denoiser + pack + denoise + compose, ReLAX) against pt_render, per frame, one lane.

Byte model per pass (what each pixel loads and stores once; the neighbour taps are counted as served by the caches):
  temporal hit: ViewZ 4 + MotionVector 12 + NormalRoughness 16 + In 2 x 16 + previous history 4 x 16 read, history 4 x 16 +
                hit distances 8 written = 200 B; miss: 4 read + 64 written = 68 B
  variance hit: ViewZ 4 + NormalRoughness 16 + accumulated 2 x 16 + moments 16 read, 2 x 16 written = 100 B; miss: 4 B
  a-trous hit:  ViewZ 4 + NormalRoughness 16 + 2 x 16 read, 2 x 16 written (the last step also reads 8 B of hit distance) = 84 B;
                miss: 4 B
Per-pass kernel durations without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_nrd_denoise.py`
(dn_temporal_kernel, dn_variance_kernel, dn_atrous_kernel<mode, last>).

    python tools/bench_nrd_denoise.py [--calls 200 --warmup 30 --frames 50 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402

MODES = {"ReBLUR": 2, "ReLAX": 3}
GUIDES = ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "MotionVector")


def byte_model(n, hits, iterations=5):
    temporal = 200 * hits + 68 * (n - hits)
    variance = 100 * hits + 4 * (n - hits)
    atrous = 84 * hits + 4 * (n - hits)
    return {"temporal": temporal, "variance": variance, "atrous_step": atrous,
            "call": temporal + variance + iterations * atrous + 8 * hits}


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


def buffers(t, n):
    width = dict(t.GBUFFER_CHANNELS)
    b = {k: torch.zeros((n, width[k]), dtype=torch.float32, device="cuda") for k in GUIDES}
    b.update({k: torch.zeros((n, 4), dtype=torch.float32, device="cuda") for k in ("Radiance", "NoisyDiffuse", "NoisySpecular", "OutDiffuse", "OutSpecular")})
    torch.cuda.synchronize()
    return b


def denoise_ptrs(b):
    return dict(ViewZ=b["LinearDepth"].data_ptr(), MotionVector=b["MotionVector"].data_ptr(), NormalRoughness=b["NormalRoughness"].data_ptr(),
                InDiffuse=b["NoisyDiffuse"].data_ptr(), InSpecular=b["NoisySpecular"].data_ptr(), OutDiffuse=b["OutDiffuse"].data_ptr(),
                OutSpecular=b["OutSpecular"].data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=50, help="C2 frames timed with the chain and with pt_render alone")
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
    res = {"metric": "pt_nrd_denoise", "calls": args.calls, "statistic": "median of single-call device-event timings", "sizes": {}}
    for s in args.sizes.split(","):
        w, h = map(int, s.split("x"))
        n = w * h
        r.set_camera(host.camera(w, h, jitter=False))
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        entry = {}
        for name, mode in MODES.items():
            b = buffers(t, n)
            r.render_gbuffer_device({k: b[k].data_ptr() for k in GUIDES})
            r.render_denoiser_device(mode, b["Radiance"].data_ptr(), {"Diffuse": b["NoisyDiffuse"].data_ptr(), "Specular": b["NoisySpecular"].data_ptr()})
            g = {k: b[k].data_ptr() for k in GUIDES[:4]}
            r.nrd_composition_device(mode, True, w, h, dict(g, NoisyDiffuse=b["NoisyDiffuse"].data_ptr(), NoisySpecular=b["NoisySpecular"].data_ptr()))
            r.synchronize()
            hits = int(torch.isfinite(b["LinearDepth"]).sum().item())
            p = denoise_ptrs(b)
            r.nrd_denoise_device(mode, w, h, p, accumulation_mode=2)
            ms5 = median_ms(stream, lambda: r.nrd_denoise_device(mode, w, h, p), args.calls, args.warmup)
            ms1 = median_ms(stream, lambda: r.nrd_denoise_device(mode, w, h, p, atrous_iterations=1), args.calls, args.warmup)
            model = byte_model(n, hits)
            src = torch.empty((model["call"] // 32, 4), dtype=torch.float32, device="cuda")  # a copy moving the same bytes: half read, half written
            dst = torch.empty_like(src)
            copy_ms = median_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup)
            rate, copy_rate = model["call"] / (ms5 * 1e-3), 2 * src.numel() * 4 / (copy_ms * 1e-3)
            step_ms = (ms5 - ms1) / 4
            step_rate = model["atrous_step"] / (step_ms * 1e-3) if step_ms > 0 else None
            entry[name] = {"hit_fraction": round(hits / n, 4), "call_ms": round(ms5, 5), "call_1_step_ms": round(ms1, 5),
                           "atrous_step_ms": round(step_ms, 5), "bytes": model, "call_TBps": round(rate / 1e12, 3),
                           "atrous_step_TBps": round(step_rate / 1e12, 3) if step_rate else None, "copy_ms": round(copy_ms, 5),
                           "copy_TBps": round(copy_rate / 1e12, 3), "call_fraction_of_copy": round(rate / copy_rate, 3),
                           "atrous_step_fraction_of_copy": round(step_rate / copy_rate, 3) if step_rate else None}
            del src, dst, b
        res["sizes"][s] = entry
    # the C2 chain against pt_render: 1920x1080, one lane, a new frame index per frame, resting camera
    w, h = 1920, 1080
    n = w * h
    r.set_camera(host.camera(w, h, jitter=False))
    gs = t.graphics_settings(w, h, bounces=8, spp=1)
    b = buffers(t, n)
    g = {k: b[k].data_ptr() for k in GUIDES[:4]}
    p = denoise_ptrs(b)
    counter = [0]

    def chain(full):
        def fn():
            gs.FrameIndex = counter[0]
            counter[0] += 1
            r.set_constants(gs)
            if not full:
                r.render_device(b["Radiance"].data_ptr())
                return
            r.render_gbuffer_device({k: b[k].data_ptr() for k in GUIDES})
            r.render_denoiser_device(3, b["Radiance"].data_ptr(), {"Diffuse": b["NoisyDiffuse"].data_ptr(), "Specular": b["NoisySpecular"].data_ptr()})
            r.nrd_composition_device(3, True, w, h, dict(g, NoisyDiffuse=b["NoisyDiffuse"].data_ptr(), NoisySpecular=b["NoisySpecular"].data_ptr()))
            r.nrd_denoise_device(3, w, h, p)
            r.nrd_composition_device(3, False, w, h, dict(g, DenoisedDiffuse=b["OutDiffuse"].data_ptr(), DenoisedSpecular=b["OutSpecular"].data_ptr(),
                                                          Radiance=b["Radiance"].data_ptr()))
        return fn

    render = mean_ms(stream, chain(False), args.frames, 10)
    full = mean_ms(stream, chain(True), args.frames, 10)
    res["c2_frame_ms"] = {"pt_render": round(render, 5), "gbuffer_denoiser_pack_denoise_compose": round(full, 5), "ratio": round(full / render, 3)}
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
