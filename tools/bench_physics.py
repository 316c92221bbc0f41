#!/usr/bin/env python3
"""Time pt_physics_step (row N23, the PhysX stand-in, DESIGN.md spec S27) and print one JSON line.

Per scene -- C2 (the demo scene's bodies) and C5 (2^20 procedural spheres and the Star) -- with the Star's constant pull on, after
--settle steps of 1/60 s so that bodies are in contact:
  step_ms         one step of 1/60 s: the mean over --calls steps queued without a report, between two device events
  contacts        the pairs in contact in one step after the timed ones
  host_step_ms    the same step through the host-compiled header (tests/hostshim/physics_host.cpp), one thread, pairs by sort-and-sweep
                  (C2 always; C5 with --host-big: minutes)
  refit_ms        pt_update_spheres + pt_refit_accel of the same spheres alone
  render_ms       the pt_render frame of the scene (1920x1080, 1 spp, 8 bounces), for scale
Per kernel: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_physics.py` (physics_*_kernel, the refit's kernels).

--loop (row N24, spec S28) times the frame loop with physics instead, two ways in one process, interleaved round by round:
  download   step -> pt_physics_download -> pt_update_spheres + pt_refit_accel -> [pt_render_gbuffer(previous pose from the host)] -> pt_render
  publish    step -> pt_physics_publish -> [pt_render_gbuffer_published] -> pt_render
per scene (C2, C5), with 1 and 3 frames in flight, without and with the G-buffer pass (MotionVector) in front of the frame.  A round is
--frames frames into three rotating device buffers and one pt_synchronize at its end, timed on the host clock (the waits of the download
loop are host time); frame_ms = round time / frames.  Reported per row and loop: the median over --rounds rounds, min and max.  C5's step
alone takes tens of milliseconds: it gets --big-frames frames and --big-rounds rounds.  Every finished row is also printed to stderr.

    python tools/bench_physics.py [--calls 100 --settle 120 --big 1048576 --host-big] [--loop --frames 30 --rounds 9]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (events only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402
import __graft_entry__ as graft  # noqa: E402


def bodies_for(t, spheres):
    """density 1, the last sphere (the Star) immovable and LARGE"""
    b = np.zeros(len(spheres), t.PHYSICS_BODY_DTYPE)
    b["InvMass"] = (1.0 / (4.0 / 3.0 * np.pi * spheres["r"].astype(np.float64) ** 3)).astype(np.float32)
    b["InvMass"][-1] = 0
    b["Flags"][-1] = t.PHYSICS_LARGE
    return b


def host_step_ms(lib, t, spheres, vel, ang, rot, bodies, settings, att, steps):
    vp = C.c_void_p
    lib.ph_host_create.restype = vp
    lib.ph_host_create.argtypes = [vp] * 5 + [C.c_uint32]
    lib.ph_host_step.argtypes = [vp, C.POINTER(t.PtPhysicsSettings), vp, C.c_uint32, C.c_float, C.c_uint32, vp]
    lib.ph_host_destroy.argtypes = [vp]
    h = lib.ph_host_create(spheres.ctypes.data, bodies.ctypes.data, vel.ctypes.data, ang.ctypes.data, rot.ctypes.data, len(spheres))
    rep = np.zeros(4, np.uint32)
    t0 = time.perf_counter()
    for _ in range(steps):
        lib.ph_host_step(h, C.byref(settings), att.ctypes.data, len(att), 1 / 60, 1, rep.ctypes.data)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    lib.ph_host_destroy(h)
    return ms, int(rep[0])


def loop_context(t, host, spheres, materials, sd, lanes, settle):
    n = len(spheres)
    r = dxrs_amd.Renderer(frames_in_flight=lanes)
    r.set_scene(spheres, materials, sd)
    r.physics_create(spheres, bodies_for(t, spheres), settings=t.physics_settings())
    r.physics_set_attractors(np.array([(n - 1, t.PHYSICS_CONSTANT, 10.0, t.PHYSICS_ALL_BODIES)], t.PHYSICS_ATTRACTOR_DTYPE))
    for _ in range(settle):
        r.physics_step(1 / 60, 1, report=False)
    W, H = 1920, 1080
    r.set_camera(host.camera_matrices(W, H))
    r.set_constants(t.graphics_settings(W, H, bounces=8, spp=1))
    outs = [torch.zeros((H * W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    mvs = [torch.zeros((H * W, 3), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    return r, outs, mvs


def loop_download(r, spheres, outs, mvs, frames, gbuffer, state):
    for k in range(frames):
        r.physics_step(1 / 60, 1, report=False)
        s, _, _, _ = r.physics_download(rotations=False, lin_vel=False, ang_vel=False)
        moved = spheres.copy()
        moved["cx"], moved["cy"], moved["cz"] = s[:, 0], s[:, 1], s[:, 2]
        r.update_spheres(moved)
        if gbuffer:
            r.render_gbuffer_device({"MotionVector": mvs[k % 3].data_ptr()}, previous_spheres=state.get("prev"))
            state["prev"] = moved
        r.render_device(outs[k % 3].data_ptr())
    r.synchronize()


def loop_publish(r, spheres, outs, mvs, frames, gbuffer, state):
    for k in range(frames):
        r.physics_step(1 / 60, 1, report=False)
        r.physics_publish()
        if gbuffer:
            r.render_gbuffer_device({"MotionVector": mvs[k % 3].data_ptr()}, previous="published")
        r.render_device(outs[k % 3].data_ptr())
    r.synchronize()


def loop_mode(args):
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    res = {"metric": "physics frame loop", "settle_steps": args.settle, "size": [1920, 1080], "rows": []}
    for name, kind, count in (("C2", dxrs_amd.host.SCENE_DEMO, 0), ("C5", dxrs_amd.host.SCENE_PROCEDURAL, args.big)):
        spheres, materials, sd = host.scene(kind, seed=0, count=count) if count else host.scene(kind, seed=0)
        sd.IsStatic = 0  # the physics is live: the G-buffer pass uses the previous pose
        frames, rounds = (args.big_frames, args.big_rounds) if count else (args.frames, args.rounds)
        for lanes in (1, 3):
            ctx = {"download": loop_context(t, host, spheres, materials, sd, lanes, args.settle), "publish": loop_context(t, host, spheres, materials, sd, lanes, args.settle)}
            fn = {"download": loop_download, "publish": loop_publish}
            for gbuffer in (False, True):
                times, state = {"download": [], "publish": []}, {"download": {}, "publish": {}}
                for which in fn:
                    fn[which](*ctx[which][:1], spheres, *ctx[which][1:], 5, gbuffer, state[which])  # warm-up: allocations, first takes
                for rnd in range(rounds):
                    for which in (("download", "publish") if rnd % 2 == 0 else ("publish", "download")):
                        r, outs, mvs = ctx[which]
                        t0 = time.perf_counter()
                        fn[which](r, spheres, outs, mvs, frames, gbuffer, state[which])
                        times[which].append((time.perf_counter() - t0) * 1e3 / frames)
                row = {"scene": name, "bodies": len(spheres), "frames_in_flight": lanes, "gbuffer": gbuffer, "frames": frames, "rounds": rounds}
                for which, v in times.items():
                    row[which] = {"frame_ms_median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            for r, _, _ in ctx.values():
                r.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--settle", type=int, default=120)
    ap.add_argument("--big", type=int, default=1 << 20)
    ap.add_argument("--host-big", action="store_true")
    ap.add_argument("--loop", action="store_true", help="time the frame loop with physics: download against publish (row N24)")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--big-frames", type=int, default=8)
    ap.add_argument("--big-rounds", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.init()
    if args.loop:
        return loop_mode(args)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    t = dxrs_amd.types
    host = dxrs_amd.load_host()
    shim = C.CDLL(graft.build_physics_shim())
    res = {"metric": "pt_physics_step", "calls": args.calls, "settle_steps": args.settle, "dt": 1 / 60, "scenes": {}}
    for name, kind, count in (("C2", dxrs_amd.host.SCENE_DEMO, 0), ("C5", dxrs_amd.host.SCENE_PROCEDURAL, args.big)):
        spheres, materials, sd = host.scene(kind, seed=0, count=count) if count else host.scene(kind, seed=0)
        n = len(spheres)
        r = dxrs_amd.Renderer(stream=stream.cuda_stream)
        r.set_scene(spheres, materials, sd)
        settings = t.physics_settings()
        bodies = bodies_for(t, spheres)
        att = np.array([(n - 1, t.PHYSICS_CONSTANT, 10.0, t.PHYSICS_ALL_BODIES)], t.PHYSICS_ATTRACTOR_DTYPE)
        r.physics_create(spheres, bodies, settings=settings)
        r.physics_set_attractors(att)
        for _ in range(args.settle):
            r.physics_step(1 / 60, 1, report=False)
        sph, rot, vel, ang = r.physics_download()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            r.physics_step(1 / 60, 1, report=False)
        b.record(stream)
        b.synchronize()
        step_ms = a.elapsed_time(b) / args.calls
        contacts = r.physics_step(1 / 60, 1).Contacts
        entry = {"bodies": n, "step_ms": round(step_ms, 4), "contacts": int(contacts)}
        if name == "C2" or args.host_big:
            ms, hc = host_step_ms(shim, t, sph, vel, ang, rot, bodies, settings, att, 20 if name == "C2" else 2)
            entry.update(host_step_ms=round(ms, 3), host_threads=1, host_contacts=hc)
        moved = spheres.copy()
        for i, k in enumerate(("cx", "cy", "cz")):
            moved[k] = sph[:, i]
        r.update_spheres(moved)
        r.synchronize()
        a.record(stream)
        for _ in range(20):
            r.update_spheres(moved)
        b.record(stream)
        b.synchronize()
        entry["refit_ms"] = round(a.elapsed_time(b) / 20, 4)
        W, H = 1920, 1080
        out = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
        r.set_camera(host.camera(W, H))
        r.set_constants(t.graphics_settings(W, H, bounces=8, spp=1))
        for _ in range(5):
            r.render_device(out.data_ptr())
        r.synchronize()
        a.record(stream)
        for _ in range(20):
            r.render_device(out.data_ptr())
        b.record(stream)
        b.synchronize()
        entry["render_ms"] = round(a.elapsed_time(b) / 20, 4)
        res["scenes"][name] = entry
        r.close()
        del out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
