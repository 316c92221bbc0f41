#!/usr/bin/env python3
"""Time pt_ray_reconstruction (row N15, the DLSS-RR stand-in) with device events and print one JSON line.  Inputs are the C2 scene's
real buffers (demo scene seed 0, 1 spp, 8 bounces, Halton jitter): the G-buffer's LinearDepth, MotionVector, NormalRoughness,
DiffuseAlbedo and SpecularAlbedo and pt_render_denoiser mode 1's radiance and SpecularHitDistance at each render size.

Per shape: the median of --calls single-call event timings of the call (both launches) with its history running, and of the call with
Reset; the byte model; the achieved rate against a float4 device-to-device copy of the same byte count timed the same way in the same
process; the same call with every pixel a surface whose 25 taps all count (the resolve pass's worst case).  Then the chain this call
replaces, for the same job, in the same script: pt_nrd_composition pack -> pt_nrd_denoise -> pt_nrd_composition compose -> pt_upscale on
the ReLAX outputs of the same frame, mean per frame of the four calls queued back to back, against the mean of pt_ray_reconstruction
queued the same way.

Byte model (what each pixel loads and stores once; the 5 x 5 taps are staged in LDS, the history's bilinear footprints are counted as
served by the caches).  Prepare, per render pixel: Color 16, Depth 4, MotionVector 12, NormalRoughness 16, the albedos 24,
SpecularHitDistance 4 read, three float4 records written: 124 B.  Resolve, per render pixel: two records and MotionVector staged (44),
the virtual-motion record (16) and the albedos (24) read once: 84 B; per output pixel: history 36 read, history 36 and Output 16
written: 88 B.
The two kernels' durations without launch gaps: run this under `rocprofv3 --kernel-trace --stats -- python
tools/bench_ray_reconstruction.py` (rr_prepare_kernel, rr_resolve_kernel<restart>).

    python tools/bench_ray_reconstruction.py [--calls 200 --warmup 30 --frames 50 --shapes 960x540:1920x1080,1920x1080:3840x2160,1920x1080:1920x1080]"""
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
    return (124 + 84) * n_in + 88 * n_out


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


def buffers(t, w, h, W, H):
    n = w * h
    b = {name: torch.zeros((n, width), dtype=torch.float32, device="cuda") for name, width in t.RAY_RECONSTRUCTION_INPUTS}
    b["Output"] = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    # the NRD chain's: the packed pair, the denoised pair, the composed radiance, the upscaled frame
    b.update({k: torch.zeros((n, 4), dtype=torch.float32, device="cuda") for k in ("NoisyDiffuse", "NoisySpecular", "OutDiffuse", "OutSpecular", "Radiance")})
    b["Upscaled"] = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--frames", type=int, default=50, help="frames timed with the NRD chain and with pt_ray_reconstruction queued back to back")
    ap.add_argument("--shapes", default="960x540:1920x1080,1920x1080:3840x2160,1920x1080:1920x1080")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    res = {"metric": "pt_ray_reconstruction", "calls": args.calls, "statistic": "median of single-call device-event timings", "shapes": {}}
    shapes = [tuple(tuple(map(int, s.split("x"))) for s in shape.split(":")) for shape in args.shapes.split(",")]
    relax = t.DENOISER_NRD_RELAX
    for (w, h), (W, H) in shapes:
        prev = host.camera_matrices(w, h, position=(0.0, 0.0, -15.1), look_at=(0.0, 0.0, 0.0), jitter_index=0, jitter_count=32)
        cam = host.camera_matrices(w, h, position=(0.0, 0.0, -15.0), look_at=(0.0, 0.0, 0.0), jitter_index=1, jitter_count=32, previous=prev)
        r.set_camera(cam)
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        b = buffers(t, w, h, W, H)
        p = {k: v.data_ptr() for k, v in b.items()}
        guides = dict(LinearDepth=p["Depth"], MotionVector=p["MotionVector"], NormalRoughness=p["NormalRoughness"], DiffuseAlbedo=p["DiffuseAlbedo"],
                      SpecularAlbedo=p["SpecularAlbedo"])
        r.render_gbuffer_device(guides)
        r.render_denoiser_device(t.DENOISER_DLSS_RR, p["Color"], dict(SpecularHitDistance=p["SpecularHitDistance"]))
        r.render_gbuffer_device(guides)
        r.render_denoiser_device(relax, p["Radiance"], dict(Diffuse=p["NoisyDiffuse"], Specular=p["NoisySpecular"]))
        r.synchronize()
        hits = float(torch.isfinite(b["Depth"]).float().mean().item())
        virtual = float((b["SpecularHitDistance"] > 0).float().mean().item())
        rr = {k: p[k] for k in t.RAY_RECONSTRUCTION_TEXTURES}

        def call(reset=False):
            r.ray_reconstruction_device((w, h), (W, H), rr, cam, reset=reset)

        call(True)
        ms = median_ms(stream, call, args.calls, args.warmup)
        ms_reset = median_ms(stream, lambda: call(True), args.calls, args.warmup)
        model = byte_model(w * h, W * H)
        src = torch.empty((model // 32, 4), dtype=torch.float32, device="cuda")  # a copy moving the same bytes: half read, half written
        dst = torch.empty_like(src)
        copy_ms = median_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup)
        rate, copy_rate = model / (ms * 1e-3), 2 * src.numel() * 4 / (copy_ms * 1e-3)
        del src, dst
        # the chain the call replaces: pack -> denoise -> compose -> upscale, on the same frame's ReLAX buffers
        g = dict(LinearDepth=p["Depth"], DiffuseAlbedo=p["DiffuseAlbedo"], SpecularAlbedo=p["SpecularAlbedo"], NormalRoughness=p["NormalRoughness"])
        dn = dict(ViewZ=p["Depth"], MotionVector=p["MotionVector"], NormalRoughness=p["NormalRoughness"], InDiffuse=p["NoisyDiffuse"],
                  InSpecular=p["NoisySpecular"], OutDiffuse=p["OutDiffuse"], OutSpecular=p["OutSpecular"])
        jit = (-cam.Jitter[0], -cam.Jitter[1])

        def nrd_chain():
            r.nrd_composition_device(relax, True, w, h, dict(g, NoisyDiffuse=p["NoisyDiffuse"], NoisySpecular=p["NoisySpecular"]))
            r.nrd_denoise_device(relax, w, h, dn)
            r.nrd_composition_device(relax, False, w, h, dict(g, DenoisedDiffuse=p["OutDiffuse"], DenoisedSpecular=p["OutSpecular"], Radiance=p["Radiance"]))
            r.upscale_device((w, h), (W, H), dict(Color=p["Radiance"], Depth=p["Depth"], Velocity=p["MotionVector"], Output=p["Upscaled"]), jitter=jit)

        chain = mean_ms(stream, nrd_chain, args.frames, 10)
        ours = mean_ms(stream, call, args.frames, 10)
        # the worst case for the resolve pass: every pixel a surface whose 25 taps all pass the edge-stopping terms
        b["Depth"].fill_(10.0)
        b["NormalRoughness"].copy_(torch.tensor([0.0, 0.0, -1.0, 0.5], device="cuda").expand_as(b["NormalRoughness"]))
        call(True)
        ms_surface = median_ms(stream, call, args.calls, args.warmup)
        res["shapes"][f"{w}x{h}:{W}x{H}"] = {
            "surface_fraction": round(hits, 4), "hit_distance_fraction": round(virtual, 4), "call_ms": round(ms, 5), "call_reset_ms": round(ms_reset, 5),
            "call_all_surface_ms": round(ms_surface, 5), "all_surface_fraction_of_copy": round(model / (ms_surface * 1e-3) / copy_rate, 3),
            "bytes": model, "call_TBps": round(rate / 1e12, 3), "copy_ms": round(copy_ms, 5), "copy_TBps": round(copy_rate / 1e12, 3),
            "call_fraction_of_copy": round(rate / copy_rate, 3),
            "same_job_ms": {"pack_denoise_compose_upscale": round(chain, 5), "pt_ray_reconstruction": round(ours, 5), "ratio": round(ours / chain, 3)}}
        del b
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
