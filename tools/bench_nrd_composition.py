#!/usr/bin/env python3
"""Time pt_nrd_composition (row N8) with device events and print one JSON line.  Inputs are the C2 scene's real G-buffer and N7 outputs
(demo scene seed 0, 1 spp, 8 bounces, frame 0) at each size, for NRDReBLUR and NRDReLAX.

Per size and mode: the median of --calls single-call event timings after --warmup calls, for pack and for compose (pack runs in place
on its own output call after call: the bytes it moves do not change); the byte model; the achieved rate against a float4
device-to-device copy of the same byte count (read half, write half) timed the same way in the same process.  Then the C2 chain
(pt_render_gbuffer + pt_render_denoiser + pack + compose, ReBLUR) against pt_render, per frame, one lane.

Byte model (what each branch loads and stores; every pixel reads its 4 B of LinearDepth, a miss stops there):
  pack ReBLUR hit: 2 albedos 24 + NormalRoughness.w 4 + noisy 2 x 16 read + 2 x 16 written = 4 + 92 B
  pack ReLAX hit:  24 + 32 + 32 = 4 + 88 B
  compose hit:     24 + denoised 2 x 16 + radiance 16 read + 16 written = 4 + 88 B
("line" also gives the model with NormalRoughness counted whole, 16 B: its .w shares a 64 B line with three other pixels' normals.)
Kernel durations without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_nrd_composition.py`.

    python tools/bench_nrd_composition.py [--calls 300 --warmup 50 --frames 100 --sizes 1920x1080,3840x2160]"""
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


def byte_model(n, hits, mode, pack, line=False):
    if pack:
        per_hit = 24 + 64 + ((16 if line else 4) if mode == 2 else 0)
    else:
        per_hit = 24 + 32 + 32
    return 4 * n + per_hit * hits


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
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames", type=int, default=100, help="C2 frames timed with the chain and with pt_render alone")
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
    width = dict(t.GBUFFER_CHANNELS)
    res = {"metric": "pt_nrd_composition", "calls": args.calls, "statistic": "median of single-call device-event timings", "sizes": {}}
    for s in args.sizes.split(","):
        w, h = map(int, s.split("x"))
        n = w * h
        r.set_camera(host.camera(w, h))
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        entry = {}
        for name, mode in MODES.items():
            b = {k: torch.zeros((n, width[k]), dtype=torch.float32, device="cuda") for k in t.NRD_TEXTURES[:4]}
            b.update({k: torch.zeros((n, 4), dtype=torch.float32, device="cuda") for k in t.NRD_TEXTURES[4:]})
            torch.cuda.synchronize()
            r.render_gbuffer_device({k: b[k].data_ptr() for k in t.NRD_TEXTURES[:4]})
            r.render_denoiser_device(mode, b["Radiance"].data_ptr(), {"Diffuse": b["NoisyDiffuse"].data_ptr(), "Specular": b["NoisySpecular"].data_ptr()})
            r.synchronize()
            hits = int(torch.isfinite(b["LinearDepth"]).sum().item())
            b["DenoisedDiffuse"].copy_(b["NoisyDiffuse"])
            b["DenoisedSpecular"].copy_(b["NoisySpecular"])
            torch.cuda.synchronize()
            ptrs = {k: v.data_ptr() for k, v in b.items()}
            e = {"hit_fraction": round(hits / n, 4)}
            for direction, pack in (("pack", True), ("compose", False)):
                ms = median_ms(stream, lambda: r.nrd_composition_device(mode, pack, w, h, ptrs), args.calls, args.warmup)
                bytes_ = byte_model(n, hits, mode, pack)
                src = torch.empty((bytes_ // 32, 4), dtype=torch.float32, device="cuda")  # a copy moving the same bytes: half read, half written
                dst = torch.empty_like(src)
                copy_ms = median_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup)
                rate, copy_rate = bytes_ / (ms * 1e-3), 2 * src.numel() * 4 / (copy_ms * 1e-3)
                e[direction] = {"ms": round(ms, 5), "bytes": bytes_, "bytes_line": byte_model(n, hits, mode, pack, line=True),
                                "TBps": round(rate / 1e12, 3), "copy_ms": round(copy_ms, 5), "copy_TBps": round(copy_rate / 1e12, 3),
                                "fraction_of_copy": round(rate / copy_rate, 3)}
                del src, dst
            entry[name] = e
            del b
        res["sizes"][s] = entry
    # the C2 chain against pt_render: 1920x1080, one lane, a new frame index per frame
    w, h = 1920, 1080
    n = w * h
    r.set_camera(host.camera(w, h))
    gs = t.graphics_settings(w, h, bounces=8, spp=1)
    b = {k: torch.zeros((n, width[k]), dtype=torch.float32, device="cuda") for k in t.NRD_TEXTURES[:4]}
    b.update({k: torch.zeros((n, 4), dtype=torch.float32, device="cuda") for k in t.NRD_TEXTURES[4:]})
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in b.items()}
    counter = [0]

    def chain(full):
        def fn():
            gs.FrameIndex = counter[0]
            counter[0] += 1
            r.set_constants(gs)
            if not full:
                r.render_device(ptrs["Radiance"])
                return
            r.render_gbuffer_device({k: ptrs[k] for k in t.NRD_TEXTURES[:4]})
            r.render_denoiser_device(2, ptrs["Radiance"], {"Diffuse": ptrs["NoisyDiffuse"], "Specular": ptrs["NoisySpecular"]})
            r.nrd_composition_device(2, True, w, h, ptrs)
            r.nrd_composition_device(2, False, w, h, dict(ptrs, DenoisedDiffuse=ptrs["NoisyDiffuse"], DenoisedSpecular=ptrs["NoisySpecular"]))
        return fn

    render = mean_ms(stream, chain(False), args.frames, 10)
    full = mean_ms(stream, chain(True), args.frames, 10)
    res["c2_frame_ms"] = {"pt_render": round(render, 5), "gbuffer_denoiser_pack_compose": round(full, 5), "ratio": round(full / render, 3)}
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
