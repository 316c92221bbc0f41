#!/usr/bin/env python3
"""Time pt_render_gbuffer (row N6) with device events and print one JSON line: ms per call on the C2 scene at 1080p and 4K for
all 13 outputs and for the denoiser subset (LinearDepth, NormalRoughness, MotionVector, BaseColorMetalness); the bytes a call
stores (counted from the frame's hits and misses: a hit writes every requested channel, a miss only Position, the depths,
MotionVector and Radiance) and the store rate that achieves, beside the all-hits bound; and the C2 frame as pt_render alone and as
pt_render_gbuffer -> pt_render, with one lane and with three frames in flight, and one frame at a time (submit, wait).

    python tools/bench_gbuffer.py [--calls 200 --warmup 20 --frames 100 --sizes 1920x1080,3840x2160]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402


MISS_CHANNELS = ("Position", "LinearDepth", "NormalizedDepth", "MotionVector", "Radiance")  # what a miss writes (spec S12)


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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100, help="C2 frames timed with and without the G-buffer pass")
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
    # depth_only: the trace and one 4-byte store (what every subset pays before its stores and its material evaluation)
    subsets = {"all": [n for n, _ in t.GBUFFER_CHANNELS], "denoiser": list(t.GBUFFER_DENOISER), "depth_only": ["LinearDepth"]}
    res = {"metric": "pt_render_gbuffer", "calls": args.calls, "sizes": {}}
    for s in args.sizes.split(","):
        w, h = map(int, s.split("x"))
        r.set_camera(host.camera_matrices(w, h))
        r.set_constants(t.graphics_settings(w, h, bounces=8, spp=1))
        bufs = {n: torch.empty((w * h, t.GBUFFER_WIDTH[n]), dtype=torch.float32, device="cuda") for n in subsets["all"]}
        hits = int(np.isfinite(r.render_gbuffer(["LinearDepth"])["LinearDepth"]).sum())  # a miss writes LinearDepth = inf
        entry = {"hit_fraction": round(hits / (w * h), 4)}
        for name, chans in subsets.items():
            if name not in ("all", "denoiser") and s != "1920x1080":
                continue
            ptrs = {n: bufs[n].data_ptr() for n in chans}
            ms = time_calls(stream, lambda: r.render_gbuffer_device(ptrs), args.calls, args.warmup)
            bpp = 4 * sum(t.GBUFFER_WIDTH[n] for n in chans)  # bytes stored per pixel where every channel is written (a hit)
            bpp_miss = 4 * sum(t.GBUFFER_WIDTH[n] for n in chans if n in MISS_CHANNELS)
            stored = bpp * hits + bpp_miss * (w * h - hits)
            entry[name] = {"ms": round(ms, 5), "bytes_per_hit": bpp, "bytes_per_miss": bpp_miss, "bytes_stored": stored,
                           "store_TBps": round(stored / (ms * 1e-3) / 1e12, 3), "bytes_all_hits": bpp * w * h,
                           "us_at_8TBps_all_hits": round(bpp * w * h / 8e12 * 1e6, 2), "us_at_8TBps_stored": round(stored / 8e12 * 1e6, 2)}
        res["sizes"][s] = entry
    # C2: demo scene, 1920x1080, 1 spp, 8 bounces; [G-buffer ->] frame, the reference's order on one queue.  With frames in flight the
    # caller rotates over as many frame buffers and G-buffer sets as there are lanes.
    r.close()
    w, h = 1920, 1080
    gs = t.graphics_settings(w, h, bounces=8, spp=1)
    res["c2_frame_ms"] = {}
    for lanes in (1, 3):
        rr = dxrs_amd.Renderer(stream=stream.cuda_stream, frames_in_flight=lanes)
        rr.set_scene(spheres, materials, sd)
        rr.set_camera(host.camera_matrices(w, h))
        frames = [torch.empty((w * h, 4), dtype=torch.float32, device="cuda") for _ in range(lanes)]
        sets = [{n: torch.empty((w * h, t.GBUFFER_WIDTH[n]), dtype=torch.float32, device="cuda") for n in subsets["all"]} for _ in range(lanes)]
        ptrs = [{n: b.data_ptr() for n, b in st.items()} for st in sets]
        torch.cuda.synchronize()
        counter = [0]

        def frame_fn(gbuffer):
            def fn():
                k = counter[0]
                counter[0] += 1
                gs.FrameIndex = k
                rr.set_constants(gs)
                if gbuffer:
                    rr.render_gbuffer_device(ptrs[k % lanes])
                rr.render_device(frames[k % lanes].data_ptr())
            return fn

        alone = time_calls(stream, frame_fn(False), args.frames, 10)
        with_gb = time_calls(stream, frame_fn(True), args.frames, 10)
        entry = {"render": round(alone, 5), "gbuffer_render": round(with_gb, 5), "gbuffer_share_ms": round(with_gb - alone, 5)}
        # one frame at a time (App::Tick -> Render -> WaitForGPU): host wall time from submission to the finished frame
        def one(gbuffer):
            fn = frame_fn(gbuffer)
            walls = []
            for _ in range(30):
                t0 = time.perf_counter()
                fn()
                rr.synchronize()
                walls.append(time.perf_counter() - t0)
            return round(float(np.median(walls[5:])) * 1e3, 5)

        entry["one_frame_at_a_time"] = {"render": one(False), "gbuffer_render": one(True)}
        res["c2_frame_ms"][f"{lanes}_lanes"] = entry
        rr.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
