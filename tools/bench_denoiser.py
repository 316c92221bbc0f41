#!/usr/bin/env python3
"""Time pt_render_denoiser (row N7) against pt_render with device events and print one JSON line: ms per frame of C2 (demo scene,
1920x1080, 1 spp, 8 bounces), C2 with direct illumination and C3 (the same scene at 3840x2160, 16 spp) as pt_render and as each
denoiser mode (DLSS-RR, ReBLUR; ReLAX runs ReBLUR's kernels), with one lane and with three frames in flight (the caller rotating one
set of buffers per lane), and the ratio of each mode to pt_render.  The frames are submitted through the C-ABI with prebuilt
arguments (no per-frame Python objects), after a pre-warm (a freshly leased GPU is not in its running state for the first frames),
and the modes are timed in alternating rounds; the median round is reported.

    python tools/bench_denoiser.py [--frames 100 --rounds 3 --prewarm 300 --c3-frames 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402


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
    ap.add_argument("--frames", type=int, default=100, help="C2 frames timed per configuration and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prewarm", type=int, default=300, help="frames rendered before the first timed round")
    ap.add_argument("--c3-frames", type=int, default=10, help="C3 frames timed per configuration and round")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    C = dxrs_amd.binding.C
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    res = {"metric": "pt_render_denoiser", "ms_per_frame": {}}
    modes = (("render", 0), ("dlss_rr", t.DENOISER_DLSS_RR), ("nrd_reblur", t.DENOISER_NRD_REBLUR))
    configs = (("C2", 1920, 1080, 1, False, args.frames, args.prewarm), ("C2_DI", 1920, 1080, 1, True, args.frames, args.prewarm // 2),
               ("C3", 3840, 2160, 16, False, args.c3_frames, 3))
    for name, w, h, spp, di, frames, prewarm in configs:
        gs = t.graphics_settings(w, h, bounces=8, spp=spp, di=di)
        entry = {}
        for lanes in (1, 3):
            r = dxrs_amd.Renderer(stream=stream.cuda_stream, frames_in_flight=lanes)
            r.set_scene(spheres, materials, sd)
            r.set_camera(host.camera(w, h))
            lib, ctx = r._lib, r._ctx
            bufs = [{"out": torch.zeros((w * h, 4), dtype=torch.float32, device="cuda"),
                     "Diffuse": torch.zeros((w * h, 4), dtype=torch.float32, device="cuda"),
                     "Specular": torch.zeros((w * h, 4), dtype=torch.float32, device="cuda"),
                     "SpecularHitDistance": torch.zeros((w * h,), dtype=torch.float32, device="cuda")} for _ in range(lanes)]
            outs = [C.c_void_p(b["out"].data_ptr()) for b in bufs]
            dn = {mode: [C.byref(t.PtDenoiserOutputs(Denoiser=mode, Diffuse=b["Diffuse"].data_ptr(), Specular=b["Specular"].data_ptr(),
                                                     SpecularHitDistance=b["SpecularHitDistance"].data_ptr())) for b in bufs] for _, mode in modes if mode}
            gs_ref = C.byref(gs)
            torch.cuda.synchronize()
            counter = [0]

            def frame_fn(mode):
                def fn():
                    k = counter[0]
                    counter[0] += 1
                    gs.FrameIndex = k
                    lib.pt_set_constants(ctx, gs_ref)
                    if mode:
                        st = lib.pt_render_denoiser(ctx, None, outs[k % lanes], 1, dn[mode][k % lanes], None)
                    else:
                        st = lib.pt_render(ctx, None, outs[k % lanes], 1, None)
                    if st:
                        raise RuntimeError(f"render failed: {st}")
                return fn

            for label, mode in modes:
                time_calls(stream, frame_fn(mode), max(1, prewarm // len(modes)), 0)
            rounds = {label: [] for label, _ in modes}
            for _ in range(args.rounds):
                for label, mode in modes:
                    rounds[label].append(time_calls(stream, frame_fn(mode), frames, 2))
            row = {label: round(sorted(v)[len(v) // 2], 5) for label, v in rounds.items()}
            row["dlss_rr_ratio"] = round(row["dlss_rr"] / row["render"], 4)
            row["nrd_ratio"] = round(row["nrd_reblur"] / row["render"], 4)
            entry[f"{lanes}_lanes"] = row
            r.close()
        res["ms_per_frame"][name] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
