#!/usr/bin/env python3
"""Time row N27 -- pt_render_gbuffer_packed and pt_render_from_gbuffer -- with device events and print one JSON line.  The scene is C2 (demo
scene seed 0, 8 bounces, a resting camera without jitter).

Per size (1920x1080 and 3840x2160), in one process and alternating over --rounds rounds so that drift hits all alike:
  the G-buffer pass: pt_render_gbuffer against pt_render_gbuffer_packed, with all 13 outputs and with the eight channels a frame from the
    G-buffer reads; the bytes each writes, and the time of a device-to-device copy of as many bytes (what writing them costs at the least);
  per sample count (1 and 16 spp) the frames alone -- pt_render, pt_render_from_gbuffer from float32 (Format 0) and packed (Format 1)
    buffers -- and the chains, each queued as the two calls without a wait between them, the pass writing the eight channels:
    gbuffer -> pt_render, gbuffer -> pt_render_from_gbuffer (Format 0), gbuffer_packed -> pt_render_from_gbuffer (Format 1);
    and the rays of one frame of each.
Per variant: the median of all its single-call event timings and the smallest and largest of its per-round medians (the run-to-run spread
inside this process).

    python tools/bench_gbframe.py [--calls 20 --warmup 5 --rounds 3 --sizes 1920x1080,3840x2160 --spp 1,16]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers and events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402
from dxrs_amd.abi_types import GBUFFER_CHANNELS, GBUFFER_FRAME_INPUTS, GBUFFER_PACKED  # noqa: E402

F32_BYTES = {name: 4 * width for name, width in GBUFFER_CHANNELS}
PACKED_BYTES = {name: np.dtype(dtype).itemsize * width for name, dtype, width in GBUFFER_PACKED}
ALL = [name for name, _ in GBUFFER_CHANNELS]


def timings_ms(stream, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summarise(samples):
    row = {}
    for name, rounds in samples.items():
        meds = [float(np.median(x)) for x in rounds]
        row[name + "_ms"] = round(float(np.median(np.concatenate(rounds))), 5)
        row[name + "_spread_ms"] = [round(min(meds), 5), round(max(meds), 5)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="timed calls per variant and round (a quarter of it at 16 spp)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--spp", default="1,16")
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    r.set_scene(spheres, materials, sd)
    res = {"metric": "pt_render_from_gbuffer", "statistic": "median of single-call device-event timings; spread = smallest and largest per-round median",
           "calls_per_round": args.calls, "rounds": args.rounds, "chain_channels": list(GBUFFER_FRAME_INPUTS), "sizes": {}}
    frame = [0]
    for W, H in [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")]:
        n = W * H
        out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        f32 = {name: torch.zeros(n * F32_BYTES[name], dtype=torch.uint8, device="cuda") for name in ALL}
        packed = {name: torch.zeros(n * PACKED_BYTES[name], dtype=torch.uint8, device="cuda") for name in ALL}
        torch.cuda.synchronize()
        r.set_camera(host.camera_matrices(W, H, jitter=False))

        def ptrs(bufs, names):
            return {name: bufs[name].data_ptr() for name in names}

        def next_frame(spp):
            frame[0] += 1
            r.set_constants(t.graphics_settings(W, H, frame_index=frame[0], bounces=8, spp=spp))

        # ---- the pass
        next_frame(1)
        passes = {"gbuffer_f32_all13": (lambda: r.render_gbuffer_device(ptrs(f32, ALL)), sum(F32_BYTES.values())),
                  "gbuffer_packed_all13": (lambda: r.render_gbuffer_packed_device(ptrs(packed, ALL)), sum(PACKED_BYTES.values())),
                  "gbuffer_f32_inputs8": (lambda: r.render_gbuffer_device(ptrs(f32, GBUFFER_FRAME_INPUTS)), sum(F32_BYTES[k] for k in GBUFFER_FRAME_INPUTS)),
                  "gbuffer_packed_inputs8": (lambda: r.render_gbuffer_packed_device(ptrs(packed, GBUFFER_FRAME_INPUTS)), sum(PACKED_BYTES[k] for k in GBUFFER_FRAME_INPUTS))}
        copies = {}
        for name, (_, bytes_per_pixel) in passes.items():
            src = torch.zeros(n * bytes_per_pixel, dtype=torch.uint8, device="cuda")
            copies[name] = (src, torch.empty_like(src))
        torch.cuda.synchronize()
        samples = {name: [] for name in passes}
        copy_samples = {name + "_copy": [] for name in passes}
        for _ in range(args.rounds):
            for name, (fn, _) in passes.items():
                samples[name].append(timings_ms(stream, fn, args.calls, args.warmup))
                src, dst = copies[name]
                copy_samples[name + "_copy"].append(timings_ms(stream, lambda: dst.copy_(src), args.calls, args.warmup))
        size = {"pass": summarise(samples)}
        size["pass"].update(summarise(copy_samples))
        for name, (_, bytes_per_pixel) in passes.items():
            size["pass"][name + "_bytes_per_pixel"] = bytes_per_pixel
            size["pass"][name + "_over_copy"] = round(size["pass"][name + "_ms"] / size["pass"][name + "_copy_ms"], 3)
        del copies

        # ---- the frames and the chains
        for spp in [int(s) for s in args.spp.split(",")]:
            calls = max(args.calls // 4, 3) if spp >= 8 else args.calls

            def plain():
                next_frame(spp)
                r.render_device(out.data_ptr())

            def from_f32():
                next_frame(spp)
                r.render_from_gbuffer_device(out.data_ptr(), ptrs(f32, GBUFFER_FRAME_INPUTS), 0)

            def from_packed():
                next_frame(spp)
                r.render_from_gbuffer_device(out.data_ptr(), ptrs(packed, GBUFFER_FRAME_INPUTS), 1)

            def chain_plain():
                next_frame(spp)
                r.render_gbuffer_device(ptrs(f32, GBUFFER_FRAME_INPUTS))
                r.render_device(out.data_ptr())

            def chain_f32():
                next_frame(spp)
                r.render_gbuffer_device(ptrs(f32, GBUFFER_FRAME_INPUTS))
                r.render_from_gbuffer_device(out.data_ptr(), ptrs(f32, GBUFFER_FRAME_INPUTS), 0)

            def chain_packed():
                next_frame(spp)
                r.render_gbuffer_packed_device(ptrs(packed, GBUFFER_FRAME_INPUTS))
                r.render_from_gbuffer_device(out.data_ptr(), ptrs(packed, GBUFFER_FRAME_INPUTS), 1)

            variants = {"pt_render": plain, "from_gbuffer_f32": from_f32, "from_gbuffer_packed": from_packed, "chain_gbuffer_pt_render": chain_plain,
                        "chain_gbuffer_from_gbuffer_f32": chain_f32, "chain_gbuffer_packed_from_gbuffer_packed": chain_packed}
            # (the frames alone read the G-buffer the last chain of their format left: this frame's own, the camera rests)
            chain_f32()
            chain_packed()
            samples = {name: [] for name in variants}
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    samples[name].append(timings_ms(stream, fn, calls, args.warmup))
            row = summarise(samples)
            next_frame(spp)
            row["rays_pt_render"] = int(r.render_device(out.data_ptr(), want_stats=True).rays)
            row["rays_from_gbuffer_f32"] = int(r.render_from_gbuffer_device(out.data_ptr(), ptrs(f32, GBUFFER_FRAME_INPUTS), 0, want_stats=True).rays)
            row["rays_from_gbuffer_packed"] = int(r.render_from_gbuffer_device(out.data_ptr(), ptrs(packed, GBUFFER_FRAME_INPUTS), 1, want_stats=True).rays)
            row["rays_gbuffer_pass"] = n  # one primary ray per pixel, in either form
            size[f"{spp}spp"] = row
        res["sizes"][f"{W}x{H}"] = size
        del out, f32, packed
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
