#!/usr/bin/env python3
"""Time pt_render_sharc (row N14, the SHARC stand-in) with device events and print one JSON line.  The scene is C2 (demo scene seed 0,
1 spp, 8 bounces, a resting camera) with the reference's SHARC settings (Capacity 1 << 22, DownscaleFactor 4, SceneScale 50,
RoughnessThreshold 0.4), after --fill whole calls that fill the cache.

Per size (1920x1080 and 3840x2160), the median of --calls single-call event timings of: the whole call (UPDATE | RESOLVE | QUERY), the
call without its query (UPDATE | RESOLVE), the update alone, the query alone, and pt_render at the same settings in the same process.
Every timed stage runs over the WARM cache: the filled cache is downloaded once and installed again (pt_sharc_upload) before each stage
is timed.  Whole calls and UPDATE | RESOLVE calls keep a cache warm by themselves; update-only and query-only calls leave the resolved
voxels as they are.  A resolve-only call is never timed: without an update in front of it every voxel ages, and MaxStaleFrames such
calls empty the cache.  A call with a single stage pays inside its event pair what the whole call pays once -- the clear of the
accumulators (update), the counters' memset, the host's enqueue gap -- so single-stage times do not add up to the call.  The stage
times are therefore derived from differences of combined calls: resolve = (UPDATE | RESOLVE) - UPDATE, query in the call = call -
(UPDATE | RESOLVE); the stand-alone times are reported beside them.  Also: the rays per frame of the call, of its query and of
pt_render.  The resolve's
bytes per second against a device-to-device copy that moves the same number of bytes; byte model of the resolve: per slot the key read
(8 B); per OCCUPIED slot two voxels read and one written (48 B) -- an empty slot's voxels are not touched.
Then the image quality on the same scene at --quality-size: the RMSE of a 1-spp pt_render_sharc frame and of a 1-spp pt_render frame
against --reference-frames accumulated pt_render frames.

pt_render_sharc_ex (row N18) per size, with the DI one pt_render_gbuffer + pt_restir_di_ex pair made for the view and DLSS-RR's output
(mode 1): the whole call and UPDATE | RESOLVE over the warm cache as above (ex_query_in_call = their difference), its surcharge over
pt_render_sharc, and beside it pt_render_with_di's surcharge over pt_render (a gather launch of 32 B per pixel); then the default
frame's chain pt_render_gbuffer -> pt_restir_di_ex -> pt_render_sharc_ex -> pt_ray_reconstruction (to 2x the size), the median wall
time from the first call to the end of the wait, next to the same chain with pt_render_with_di in the cache's place.

The anti-firefly filter (row N19, IsAntiFireflyEnabled through pt_render_sharc_ex without DI or outputs) per size, over the warm cache
as above: the whole call, UPDATE | RESOLVE and the update alone with the filter on (ff_*), the resolve as their difference and against the
same device copy, next to the filter-off figures of the same run; and the 1-spp RMSE with the filter on beside the existing pair.

    python tools/bench_sharc.py [--calls 100 --warmup 10 --fill 12 --sizes 1920x1080,3840x2160 --quality-size 480x270 --reference-frames 2048]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402
from dxrs_amd.abi_types import GBUFFER_CHANNELS, RESTIR_DI_INPUTS  # noqa: E402

UPDATE, RESOLVE, QUERY = 1, 2, 4
RESOLVE_BYTES_PER_SLOT, RESOLVE_BYTES_PER_OCCUPIED_SLOT = 8, 48


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fill", type=int, default=12, help="whole calls that fill the cache before anything is timed")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--quality-size", default="480x270")
    ap.add_argument("--reference-frames", type=int, default=2048)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    st = dict(capacity=args.capacity, downscale_factor=4, scene_scale=50.0, roughness_threshold=0.4)
    res = {"metric": "pt_render_sharc", "calls": args.calls, "statistic": "median of single-call device-event timings", "capacity": args.capacity,
           "resolve_bytes_per_slot": RESOLVE_BYTES_PER_SLOT, "resolve_bytes_per_occupied_slot": RESOLVE_BYTES_PER_OCCUPIED_SLOT, "sizes": {}}
    frame = [0]

    def next_frame(w, h):
        frame[0] += 1
        r.set_constants(t.graphics_settings(w, h, frame_index=frame[0], bounces=8, spp=1))

    for W, H in [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")]:
        out = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_camera(host.camera_matrices(W, H, jitter=False))
        for k in range(args.fill):
            next_frame(W, H)
            r.render_sharc_device(out.data_ptr(), reset_history=k == 0, **st)
        r.synchronize()
        keys, voxels = r.sharc_download(args.capacity)
        occupied = int((keys != 0).sum())

        def stage(stages):
            next_frame(W, H)
            r.render_sharc_device(out.data_ptr() if stages & QUERY else 0, stages=stages, **st)

        def plain():
            next_frame(W, H)
            r.render_device(out.data_ptr())

        def warm(fn):
            """fn timed over the filled cache: installed again first, and checked afterwards to be still as full"""
            r.sharc_upload(keys, voxels)
            ms_ = median_ms(stream, fn, args.calls, args.warmup)
            r.synchronize()
            left = int((r.sharc_download(args.capacity)[0] != 0).sum())
            assert left >= occupied * 9 // 10, f"the cache drained while a stage was timed: {left} of {occupied} slots left"
            return ms_

        ms = {name: warm(fn) for name, fn in (("call", lambda: stage(7)), ("update_resolve", lambda: stage(UPDATE | RESOLVE)), ("update_alone", lambda: stage(UPDATE)),
                                              ("query_alone", lambda: stage(QUERY)))}
        ms["pt_render"] = median_ms(stream, plain, args.calls, args.warmup)
        ms["resolve"] = ms["update_resolve"] - ms["update_alone"]

        def stage_ff(stages):
            next_frame(W, H)
            r.render_sharc_ex_device(out.data_ptr() if stages & QUERY else 0, None, None, None, 0, None, stages=stages, anti_firefly=True, **st)

        ms["ff_call"] = warm(lambda: stage_ff(7))
        ms["ff_update_resolve"] = warm(lambda: stage_ff(UPDATE | RESOLVE))
        ms["ff_update_alone"] = warm(lambda: stage_ff(UPDATE))
        ms["ff_resolve"] = ms["ff_update_resolve"] - ms["ff_update_alone"]
        ms["query_in_call"] = ms["call"] - ms["update_resolve"]
        clear = torch.zeros(args.capacity * 4, dtype=torch.int32, device="cuda")
        ms["clear"] = median_ms(stream, lambda: clear.zero_(), args.calls, args.warmup)
        model = RESOLVE_BYTES_PER_SLOT * args.capacity + RESOLVE_BYTES_PER_OCCUPIED_SLOT * occupied
        src = torch.zeros(model // 8 + 1, dtype=torch.float32, device="cuda")
        dst = torch.zeros(model // 8 + 1, dtype=torch.float32, device="cuda")
        ms["copy"] = median_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup)
        r.sharc_upload(keys, voxels)
        next_frame(W, H)
        rays_call = r.render_sharc_device(out.data_ptr(), want_stats=True, **st).rays
        rays_query = r.render_sharc_device(out.data_ptr(), want_stats=True, stages=QUERY, **st).rays
        rays_plain = r.render_device(out.data_ptr(), want_stats=True).rays
        # ---- row N18: the same frame with the DI of pt_restir_di_ex and DLSS-RR's SpecularHitDistance
        width = dict(GBUFFER_CHANNELS)
        gb = {n: torch.zeros((H * W, width[n]), dtype=torch.float32, device="cuda") for n in set(RESTIR_DI_INPUTS) | {"DiffuseAlbedo", "SpecularAlbedo"}}
        dd, ds = (torch.zeros((H * W, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        shd = torch.zeros(H * W, dtype=torch.float32, device="cuda")
        up = torch.zeros((4 * H * W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        cam = host.camera_matrices(W, H, jitter=False)
        ptrs = {n: b.data_ptr() for n, b in gb.items()}

        def make_di(reset=False):
            r.render_gbuffer_device(ptrs)
            r.restir_di_device(W, H, dict({n: ptrs[n] for n in RESTIR_DI_INPUTS}, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), frame_index=frame[0], reset_history=reset,
                               candidates=dict(brdf_samples=1, boiling_filter=0.2))

        next_frame(W, H)
        make_di(True)
        r.synchronize()

        def stage_ex(stages):
            next_frame(W, H)
            r.render_sharc_ex_device(out.data_ptr() if stages & QUERY else 0, dd.data_ptr(), ds.data_ptr(), None, 1, dict(SpecularHitDistance=shd.data_ptr()), stages=stages, **st)

        def with_di():
            next_frame(W, H)
            r.render_with_di_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, 1, dict(SpecularHitDistance=shd.data_ptr()))

        ms["ex_call"] = warm(lambda: stage_ex(7))
        ms["ex_update_resolve"] = warm(lambda: stage_ex(UPDATE | RESOLVE))
        ms["ex_query_in_call"] = ms["ex_call"] - ms["ex_update_resolve"]
        ms["ex_update_resolve_surcharge"] = ms["ex_update_resolve"] - ms["update_resolve"]
        ms["ex_query_surcharge"] = ms["ex_query_in_call"] - ms["query_in_call"]
        ms["pt_render_with_di"] = median_ms(stream, with_di, args.calls, args.warmup)
        ms["with_di_surcharge"] = ms["pt_render_with_di"] - ms["pt_render"]

        def chain(middle):
            wall = []
            for k in range(args.warmup + args.calls // 2):
                next_frame(W, H)
                t0 = time.perf_counter()
                make_di()
                middle()
                r.ray_reconstruction_device((W, H), (2 * W, 2 * H), dict(Color=out.data_ptr(), Depth=ptrs["LinearDepth"], MotionVector=ptrs["MotionVector"],
                                                                         NormalRoughness=ptrs["NormalRoughness"], DiffuseAlbedo=ptrs["DiffuseAlbedo"],
                                                                         SpecularAlbedo=ptrs["SpecularAlbedo"], SpecularHitDistance=shd.data_ptr(), Output=up.data_ptr()),
                                            cam, reset=k == 0)
                r.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(wall[args.warmup:]))

        r.sharc_upload(keys, voxels)
        ms["chain_default_frame"] = chain(lambda: r.render_sharc_ex_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, 1, dict(SpecularHitDistance=shd.data_ptr()), **st))
        ms["chain_with_di_no_cache"] = chain(lambda: r.render_with_di_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, 1, dict(SpecularHitDistance=shd.data_ptr())))
        del gb, dd, ds, shd, up
        res["sizes"][f"{W}x{H}"] = dict({k + "_ms": round(v, 5) for k, v in ms.items()}, call_over_pt_render=round(ms["call"] / ms["pt_render"], 3),
                                        rays_call=int(rays_call), rays_query=int(rays_query), rays_pt_render=int(rays_plain), occupied_slots=occupied, resolve_bytes=model,
                                        resolve_TBps=round(model / (ms["resolve"] * 1e-3) / 1e12, 3), copy_TBps=round(model / (ms["copy"] * 1e-3) / 1e12, 3),
                                        resolve_fraction_of_copy=round(ms["copy"] / ms["resolve"], 3), ff_resolve_fraction_of_copy=round(ms["copy"] / ms["ff_resolve"], 3))
        del out, clear, src, dst
    # image quality: 1 spp through the cache and without it against a converged pt_render accumulation
    W, H = map(int, args.quality_size.split("x"))
    n = W * H
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    accum = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.set_camera(host.camera_matrices(W, H, jitter=False))
    for k in range(args.reference_frames):
        r.set_constants(t.graphics_settings(W, H, frame_index=100000 + k, bounces=8, spp=1))
        r.render_device(out.data_ptr())
        r.accumulate(accum.data_ptr(), out.data_ptr(), n, k)
    r.synchronize()
    truth = accum.cpu().numpy()[:, :3].astype(np.float64)
    for k in range(args.fill):
        r.set_constants(t.graphics_settings(W, H, frame_index=k, bounces=8, spp=1))
        r.render_sharc_device(out.data_ptr(), reset_history=k == 0, **st)
    r.synchronize()
    cached = out.cpu().numpy()[:, :3].astype(np.float64)
    r.render_device(out.data_ptr())
    r.synchronize()
    plain_img = out.cpu().numpy()[:, :3].astype(np.float64)
    for k in range(args.fill):
        r.set_constants(t.graphics_settings(W, H, frame_index=k, bounces=8, spp=1))
        r.render_sharc_ex_device(out.data_ptr(), None, None, None, 0, None, reset_history=k == 0, anti_firefly=True, **st)
    r.synchronize()
    filtered = out.cpu().numpy()[:, :3].astype(np.float64)
    res["quality"] = {"size": f"{W}x{H}", "reference_frames": args.reference_frames, "rmse_pt_render_sharc_1spp": round(float(np.sqrt(((cached - truth) ** 2).mean())), 5),
                      "rmse_pt_render_sharc_ff_1spp": round(float(np.sqrt(((filtered - truth) ** 2).mean())), 5),
                      "rmse_pt_render_1spp": round(float(np.sqrt(((plain_img - truth) ** 2).mean())), 5), "mean_radiance": round(float(truth.mean()), 5)}
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
