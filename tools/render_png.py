#!/usr/bin/env python3
"""Render the demo scene on the GPU and write a PNG through the product's own display path: N frames of the path tracer
with jittered cameras -> pt_accumulate (running mean) [-> pt_bloom with --bloom] -> pt_tonemap (ACES filmic + sRGB, the reference's SDR default) ->
R8G8B8A8 (--nrd: one frame through the NRD path instead, row N8; --nrd-denoise: --frames frames of a resting camera through it with the
NRD stand-in, row N9; --restir-di: --frames frames of a resting camera through pt_render_gbuffer -> pt_restir_di -> pt_render_with_di,
row N10, accumulated; --upscale MODE: --frames frames of a resting camera rendered at the mode's input size with Halton jitter and
upscaled to --width x --height by pt_upscale, row N11; --nis SHARPNESS: pt_nis_sharpen, row N12, on the frame at output size, after the
upscaler when there is one and before bloom; --chromatic-aberration R G B: pt_chromatic_aberration, row N29, with the three channels'
offsets, after --nis and before bloom; --frame-gen MID.png: the frames at --time minus --dt and at --time, and the frame
pt_frame_gen, row N13, makes between them; --sharc: --frames frames of a resting camera through pt_render_sharc, row N14, the last one tone
mapped; --ray-reconstruction [MODE]: --frames frames of a resting camera rendered at the mode's input size through pt_render_gbuffer ->
pt_render_denoiser mode 1 -> pt_ray_reconstruction, row N15, to --width x --height; --sharc --restir-di --ray-reconstruction together: the
reference's default frame, pt_render_gbuffer -> pt_restir_di_ex -> pt_render_sharc_ex (row N18) -> pt_ray_reconstruction; --aperture R [--focus-distance F]: the accumulated frames through the thin-lens camera,
pt_render_lens, row N26; --from-gbuffer {float,packed}: the accumulated frames with the G-buffer's texel as every sample's primary surface,
pt_render_gbuffer[_packed] -> pt_render_from_gbuffer, row N27).  Viewer convenience; the measured output of the hot path is the fp32 HDR radiance buffer.

    python tools/render_png.py out.png [--width 1280 --height 720 --spp 8 --frames 16 --bounces 8 --time 0.0 --textures
                                        --texture-dir /path/to/Assets/Textures --bloom 0.05 --gbuffer NormalRoughness | --denoiser-output Diffuse | --nrd ReBLUR | --nrd-denoise ReLAX | --restir-di [--light-sampling regir] [--brdf-samples 1] [--boiling-filter 0.2] [--bias-correction pairwise] [--reuse-visibility [4 16]] | --upscale performance] [--nis 0.5] [--chromatic-aberration 0.003 0.003 -0.003] [--frame-gen mid.png --dt 0.1] [--sharc [--sharc-anti-firefly]] | --sharc --sharc-anti-firefly --restir-di --brdf-samples 1 --boiling-filter 0.2 --ray-reconstruction quality
                                        [--ray-reconstruction [performance]]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device buffers only)
import dxrs_amd_loader  # noqa: E402,F401
import dxrs_amd  # noqa: E402


def gbuffer_image(name, a):
    """a G-buffer channel (h, w, c) as 8-bit RGB: unit vectors and octahedral normals as 0.5 + 0.5 v, motion vectors around grey,
    colours and scalars scaled by their largest finite value; pixels the pass did not write (NaN) or infinite ones are black"""
    valid = np.isfinite(a).all(axis=-1)
    v = np.where(np.isfinite(a), a, 0.0).astype(np.float64)
    if name in ("FlatNormal", "GeometricNormal", "NormalRoughness"):
        rgb = 0.5 + 0.5 * np.concatenate([v[..., :3], np.zeros(v.shape[:2] + (max(0, 3 - v.shape[-1]),))], -1)[..., :3]
    elif name == "MotionVector":
        m = max(np.abs(v[..., :2]).max(), 1e-6)
        rgb = np.stack([0.5 + 0.5 * v[..., 0] / m, 0.5 + 0.5 * v[..., 1] / m, np.full(v.shape[:2], 0.5)], -1)
    else:
        m = max(np.abs(v[valid]).max() if valid.any() else 1.0, 1e-6)
        x = np.abs(v) / m
        rgb = np.repeat(x[..., :1], 3, -1) if v.shape[-1] < 3 else x[..., :3]
        rgb = rgb ** (1 / 2.2)
    rgb[~valid] = 0.0
    return (np.clip(rgb, 0.0, 1.0) * 255 + 0.5).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16, help="jittered frames accumulated by pt_accumulate")
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--time", type=float, default=0.0, help="simulation time of the closed-form motion")
    ap.add_argument("--physics", action="store_true", help="row N23: reach --time with pt_physics_step (steps of 1/60 s, collisions included) instead of the closed form")
    ap.add_argument("--publish", action="store_true", help="--physics: hand the simulated pose to the frame on the device (pt_physics_publish, row N24) instead of download + pt_update_spheres")
    ap.add_argument("--star-gravity", action="store_true", help="--physics: the Star's constant 10 m/s^2 pull on every body (the reference's H key)")
    ap.add_argument("--earth-gravity", action="store_true", help="--physics: the Earth's inverse-square pull on every body, not just the Moon (the G key)")
    ap.add_argument("--textures", action="store_true", help="textured Alien-Metal / Moon / Earth (procedural stand-ins)")
    ap.add_argument("--env-map", action="store_true", help="lat-long HDR environment light (MyScene.ixx:94-95; procedural stand-in) instead of the sky")
    ap.add_argument("--texture-dir", default=None, help="directory of decoded images (<stem>.ptex, e.g. tests/golden/textures = the reference's Assets/Textures): use them instead of the stand-ins")
    ap.add_argument("--operator", choices=["saturate", "reinhard", "aces"], default="aces")
    ap.add_argument("--exposure", type=float, default=0.0, help="stops")
    ap.add_argument("--bloom", type=float, default=None, metavar="STRENGTH",
                    help="pt_bloom on the accumulated radiance before tone mapping (the reference's default is 0.05); off by default")
    ap.add_argument("--gbuffer", default=None, metavar="CHANNEL", choices=[n for n, _ in dxrs_amd.types.GBUFFER_CHANNELS],
                    help="write one channel of pt_render_gbuffer (row N6) of the first frame instead of the path-traced image")
    ap.add_argument("--denoiser-output", default=None, choices=["Diffuse", "Specular", "SpecularHitDistance"],
                    help="write one output of pt_render_denoiser (row N7) of the first frame instead of the path-traced image: Diffuse / "
                         "Specular from NRDReBLUR (radiance; their hit distance is not shown), SpecularHitDistance from DLSSRayReconstruction")
    ap.add_argument("--nrd", default=None, choices=["ReBLUR", "ReLAX"],
                    help="one frame through the reference's NRD path with the identity for NRD (row N8): pt_render_gbuffer -> "
                         "pt_render_denoiser -> pack -> copy -> compose, then the tone map (no accumulation)")
    ap.add_argument("--nrd-denoise", default=None, choices=["ReBLUR", "ReLAX"],
                    help="--frames frames of a resting camera through the NRD path with pt_nrd_denoise for NRD (row N9): pt_render_gbuffer "
                         "-> pt_render_denoiser -> pack -> denoise -> compose; the last frame, tone mapped")
    ap.add_argument("--nrd-reblur", action="store_true",
                    help="the chain of --nrd-denoise ReBLUR with pt_nrd_reblur for NRD (row N30: the recurrent-blur stand-in for ReBLUR itself); "
                         "what applies to --nrd-denoise applies to it")
    ap.add_argument("--restir-di", action="store_true",
                    help="--frames frames of a resting camera whose direct illumination the reservoir pass makes (row N10): pt_render_gbuffer "
                         "-> pt_restir_di (the history running) -> pt_render_with_di, accumulated, tone mapped")
    ap.add_argument("--light-sampling", default="uniform", choices=["uniform", "power", "regir"],
                    help="with --restir-di: where the reservoir pass draws its initial candidates (row N16): uniformly from the emitter list "
                         "(pt_restir_di), from Power_RIS tiles or from the ReGIR grid (pt_restir_di_sampled at its defaults; the reference's "
                         "default is regir)")
    ap.add_argument("--brdf-samples", type=int, default=0, metavar="N",
                    help="with --restir-di: N BSDF-sampled candidates mixed into initial sampling (row N17, pt_restir_di_ex; 0 .. 8, the reference's default is 1)")
    ap.add_argument("--boiling-filter", type=float, default=None, metavar="STRENGTH",
                    help="with --restir-di: the boiling filter over the temporal result at this strength in [0, 1] (row N17; the reference's default is 0.2)")
    ap.add_argument("--bias-correction", default=None, choices=["off", "basic", "pairwise", "raytraced"],
                    help="with --restir-di: the bias correction of both reuse passes (the library's default is basic); pairwise runs through "
                         "pt_restir_di_full (row N22)")
    ap.add_argument("--reuse-visibility", nargs="*", type=float, default=None, metavar="AGE DIST",
                    help="with --restir-di: final shading reuses a sample's visibility (row N22, pt_restir_di_full) where the sample is at most "
                         "AGE frames old and DIST pixels from where it was drawn; without values 4 16, the RTXDI SDK's defaults as recollected")
    ap.add_argument("--upscale", default=None, metavar="MODE", choices=list(dxrs_amd.types.UPSCALE_MODES),
                    help="--frames frames of a resting camera rendered at the mode's input size (pt_upscale_input_size) with Halton jitter (row "
                         "N11): pt_render_gbuffer (LinearDepth, MotionVector) -> pt_render -> pt_upscale to --width x --height [-> pt_bloom with "
                         "--bloom] -> the tone map at output size; the last frame")
    ap.add_argument("--nis", type=float, default=None, metavar="SHARPNESS",
                    help="pt_nis_sharpen (row N12; the reference's default sharpness is 0.5) at output size: after pt_upscale with --upscale, "
                         "else on the accumulated radiance; before pt_bloom")
    ap.add_argument("--chromatic-aberration", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help="pt_chromatic_aberration (row N29) about the image centre with these offsets (each within +-1/16; 0.003 0.003 -0.003 are "
                         "the defaults): wherever --nis applies, after it and before pt_bloom")
    ap.add_argument("--frame-gen", default=None, metavar="MID.png",
                    help="render the scene at --time minus --dt and at --time (one frame each: pt_render_gbuffer with the earlier pose as the "
                         "previous one -> pt_render [-> pt_bloom] -> pt_tonemap) and write the frame pt_frame_gen (row N13) makes between the "
                         "two to MID.png; the frame at --time goes to the positional output")
    ap.add_argument("--sharc", action="store_true",
                    help="--frames frames of a resting camera through the radiance cache (row N14): pt_render_sharc with the reference's "
                         "SHARC settings (update at a quarter of the size, resolve, query); the last frame, tone mapped (no accumulation)")
    ap.add_argument("--sharc-anti-firefly", action="store_true",
                    help="--sharc with the cache's anti-firefly filter (row N19, IsAntiFireflyEnabled, which the reference's application sets): "
                         "the frame goes through pt_render_sharc_ex")
    ap.add_argument("--ray-reconstruction", nargs="?", const="native", default=None, metavar="MODE", choices=list(dxrs_amd.types.UPSCALE_MODES),
                    help="--frames frames of a resting camera through the reference's default denoiser path (row N15): rendered at the "
                         "mode's input size (pt_upscale_input_size; native without a mode) with Halton jitter: pt_render_gbuffer -> "
                         "pt_render_denoiser mode 1 -> pt_ray_reconstruction to --width x --height [-> pt_nis_sharpen with --nis] [-> pt_bloom "
                         "with --bloom] -> the tone map; the last frame")
    ap.add_argument("--aperture", type=float, default=None, metavar="R",
                    help="the plain path-traced frame through the thin-lens camera (row N26): pt_render_lens with ApertureRadius R, accumulated like pt_render's frames")
    ap.add_argument("--focus-distance", type=float, default=None, metavar="F",
                    help="--aperture: the view depth in focus, through CameraController::SetFocusDistance (default 15: the demo's spheres)")
    ap.add_argument("--from-gbuffer", default=None, choices=["float", "packed"],
                    help="the plain path-traced frame the way the reference runs it (row N27): each frame's G-buffer pass (float: pt_render_gbuffer, packed: "
                         "pt_render_gbuffer_packed, the reference's texture formats), then pt_render_from_gbuffer, which loads it as the primary surface of every sample")
    ap.add_argument("--dt", type=float, default=0.1, help="--frame-gen: seconds between the two rendered frames")
    args = ap.parse_args()
    if args.nrd_reblur:
        if args.nrd_denoise:
            ap.error("--nrd-reblur and --nrd-denoise are two stand-ins for the same pass: give one")
        args.nrd_denoise = "ReBLUR"
    if args.frame_gen and (args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di or args.upscale or args.nis is not None):
        ap.error("--frame-gen applies to the plain path-traced frame")
    default_frame = bool(args.sharc and args.restir_di and args.ray_reconstruction)  # the reference's default frame, rows N6 / N17 / N18 / N15
    if default_frame and (args.frame_gen or args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.upscale):
        ap.error("--sharc --restir-di --ray-reconstruction is the default frame: it takes --light-sampling, --brdf-samples, --boiling-filter, --nis and --bloom only")
    if default_frame:
        pass
    elif args.sharc and (args.frame_gen or args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di or args.upscale or args.nis is not None):
        ap.error("--sharc applies to the plain path-traced frame")
    if not default_frame and args.ray_reconstruction and (args.frame_gen or args.sharc or args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di or args.upscale):
        ap.error("--ray-reconstruction is a path of its own: it takes --nis and --bloom only")
    if args.aperture is not None and (args.frame_gen or args.sharc or args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di or args.upscale
                                      or args.ray_reconstruction):
        ap.error("--aperture applies to the plain path-traced frame")
    if args.from_gbuffer and (args.aperture is not None or args.frame_gen or args.sharc or args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di
                              or args.upscale or args.ray_reconstruction):
        ap.error("--from-gbuffer applies to the plain path-traced frame")
    if args.focus_distance is not None and args.aperture is None:
        ap.error("--focus-distance applies to --aperture")
    if args.focus_distance is not None and not args.focus_distance > 0.0:
        ap.error("--focus-distance must be positive")
    focus_distance = 15.0 if args.focus_distance is None else args.focus_distance
    if args.sharc_anti_firefly and not args.sharc:
        ap.error("--sharc-anti-firefly applies to --sharc")
    if args.light_sampling != "uniform" and not args.restir_di:
        ap.error("--light-sampling applies to --restir-di")
    if (args.brdf_samples or args.boiling_filter is not None) and not args.restir_di:
        ap.error("--brdf-samples and --boiling-filter apply to --restir-di")
    if (args.bias_correction or args.reuse_visibility is not None) and not args.restir_di:
        ap.error("--bias-correction and --reuse-visibility apply to --restir-di")
    if args.reuse_visibility is not None and len(args.reuse_visibility) not in (0, 2):
        ap.error("--reuse-visibility takes no value or AGE DIST")
    if args.nis is not None and not default_frame and (args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di):
        ap.error("--nis applies to the path-traced frame, with or without --upscale; not to --gbuffer, --denoiser-output, --nrd, --nrd-denoise or --restir-di")
    if args.chromatic_aberration is not None:
        if args.frame_gen or (args.sharc and not default_frame) or (not default_frame and (args.gbuffer or args.denoiser_output or args.nrd or args.nrd_denoise or args.restir_di)):
            ap.error("--chromatic-aberration applies where --nis does: the path-traced frame, --upscale, --ray-reconstruction and the default frame")
        if not all(abs(k) <= dxrs_amd.types.CHROMATIC_ABERRATION_MAX_OFFSET for k in args.chromatic_aberration):
            ap.error("--chromatic-aberration: each offset must be within +-1/16")
    from PIL import Image

    t = dxrs_amd.types
    # row N22: the arguments that send the reservoir pass through pt_restir_di_full
    full = {}
    if args.bias_correction:
        mode = dict(off=t.RESTIR_BIAS_OFF, basic=t.RESTIR_BIAS_BASIC, pairwise=t.RESTIR_BIAS_PAIRWISE, raytraced=t.RESTIR_BIAS_RAYTRACED)[args.bias_correction]
        full.update(temporal_bias=mode, spatial_bias=mode)
    if args.reuse_visibility is not None:
        age, dist = args.reuse_visibility or (4, 16)
        full["shading"] = dict(reuse=True, max_age=int(age), max_distance=float(dist))
    elif args.bias_correction == "pairwise":
        full["shading"] = {}
    host = dxrs_amd.load_host()
    spheres, materials, sd = host.scene(dxrs_amd.host.SCENE_DEMO, seed=0)
    if args.time and not args.physics:
        spheres = host.scene_at_time(0, args.time)
    torch.cuda.init()
    stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
    r = dxrs_amd.Renderer(stream=stream.cuda_stream)
    textured = bool(args.textures or args.texture_dir)
    if textured or args.env_map:
        # --texture-dir: decoded images (<stem>.ptex; tests/golden/textures holds the reference's own assets) through the host mirror's loader
        ts, sd_env = host.demo_textures(0, args.time, textured=textured, environment_map=args.env_map, return_scene_data=True, texture_dir=args.texture_dir)
        if args.env_map:
            sd = sd_env
    r.set_scene(spheres, materials, sd)
    if textured or args.env_map:
        r.set_textures(ts)
    if args.physics:
        # the bodies, initial velocities and forces of MyScene.ixx (heroes, the grid of oscillators, Moon, Earth, Star: host/Physics.hpp)
        nb = len(spheres)
        moon, earth, star = nb - 3, nb - 2, nb - 1
        bodies = np.zeros(nb, t.PHYSICS_BODY_DTYPE)
        bodies["InvMass"] = (1.0 / (4.0 / 3.0 * np.pi * spheres["r"].astype(np.float64) ** 3)).astype(np.float32)
        bodies["Flags"][spheres["r"] > 4 * np.median(spheres["r"])] = t.PHYSICS_LARGE
        omega = 2 * np.pi / 3.0
        bodies["Flags"][4:moon] |= t.PHYSICS_SPRING
        bodies["SpringY0"], bodies["SpringOmega2"] = 0.5, omega * omega
        lin, ang = np.zeros((nb, 3), np.float32), np.zeros((nb, 3), np.float32)
        lin[4:moon, 1] = -0.5 * omega * np.sin(-spheres["cx"][4:moon])
        gm = 4 * np.pi ** 2 * 4.0 ** 3 / 100.0
        bodies["InvMass"][earth], bodies["InvMass"][star] = 6.6743e-11 / gm, 0
        lin[moon, 2], ang[moon, 1], ang[earth, 1] = -np.sqrt(gm / 4.0), -np.sqrt(gm / 4.0) / 4.0, -2 * np.pi / 15.0
        r.physics_create(spheres, bodies, lin, ang, ts.rotations if textured else None)
        att = [(earth, t.PHYSICS_INVERSE_SQUARE, gm, t.PHYSICS_ALL_BODIES if args.earth_gravity else moon)]
        if args.star_gravity:
            att.append((star, t.PHYSICS_CONSTANT, 10.0, t.PHYSICS_ALL_BODIES))
        r.physics_set_attractors(att)
        steps, contacts = int(round(args.time * 60)), 0
        for _ in range(steps):
            contacts = r.physics_step(1 / 60, 1).Contacts
        if args.publish:
            r.physics_publish()
        else:
            sph, rot, _, _ = r.physics_download()
            spheres = spheres.copy()
            for i, k in enumerate(("cx", "cy", "cz")):
                spheres[k] = sph[:, i]
            r.update_spheres(spheres)
            if textured:
                r.update_rotations(rot)
        print(f"physics (pt_physics_step): {steps} steps of 1/60 s, {contacts} contacts in the last" + (", pose published on the device" if args.publish else ""))
    w, h, n = args.width, args.height, args.width * args.height
    gs = t.graphics_settings(w, h, bounces=args.bounces, spp=args.spp)
    if args.gbuffer:
        r.set_camera(host.camera_matrices(w, h, jitter_index=0, jitter_count=max(args.frames, 8)))
        r.set_constants(gs)
        img = gbuffer_image(args.gbuffer, r.render_gbuffer([args.gbuffer])[args.gbuffer])
        Image.fromarray(img).save(args.out)
        print(f"G-buffer {args.gbuffer} {w}x{h} -> {args.out}")
        r.close()
        return
    if args.denoiser_output:
        mode = t.DENOISER_DLSS_RR if args.denoiser_output == "SpecularHitDistance" else t.DENOISER_NRD_REBLUR
        r.set_camera(host.camera(w, h, jitter_index=0, jitter_count=max(args.frames, 8)))
        r.set_constants(gs)
        a = r.render_denoiser(mode)[1][args.denoiser_output]  # (NaN where the frame wrote nothing: black)
        img = gbuffer_image("Radiance", a[..., :3] if a.shape[-1] == 4 else a)
        Image.fromarray(img).save(args.out)
        print(f"denoiser output {args.denoiser_output} {w}x{h} -> {args.out}")
        r.close()
        return
    frame = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    accum = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ldr = torch.empty(n, dtype=torch.int32, device="cuda")
    if args.frame_gen:
        sd.IsStatic = 0
        r.set_scene(spheres, materials, sd)
        if textured or args.env_map:
            r.set_textures(ts)
        depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        velocity = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        mid = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.set_camera(host.camera_matrices(w, h, jitter=False))
        earlier = None
        for k, time in enumerate((args.time - args.dt, args.time)):
            moved = host.scene_at_time(0, time)
            r.update_spheres(moved)
            gs.FrameIndex = k
            r.set_constants(gs)
            r.render_gbuffer_device(dict(LinearDepth=depth.data_ptr(), MotionVector=velocity.data_ptr()), previous_spheres=earlier)
            r.render_device(frame.data_ptr())
            if args.bloom is not None:
                r.bloom(frame.data_ptr(), frame.data_ptr(), w, h, args.bloom)
            r.tonemap(frame.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
            generated = r.frame_gen_device((w, h), (w, h), dict(Color=ldr.data_ptr(), Depth=depth.data_ptr(), MotionVector=velocity.data_ptr(),
                                                                Output=mid.data_ptr()), reset=k == 0)
            earlier = moved
        r.synchronize()
        assert generated
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        Image.fromarray(mid.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.frame_gen)
        print(f"frame generation (pt_frame_gen) {w}x{h}: time {args.time} -> {args.out}, time {args.time - args.dt / 2} -> {args.frame_gen}")
        r.close()
        return
    if default_frame:
        # GBufferGeneration -> RTXDI -> Raytracing::Render(SHARC) -> DLSS-RR (App.cpp:1255-1268): pt_render_gbuffer -> pt_restir_di_ex ->
        # pt_render_sharc_ex with that DI and mode 1 -> pt_ray_reconstruction, every pass queued on the frame's lane or the context's stream
        iw, ih = dxrs_amd.load_hip().upscale_input_size(t.UPSCALE_MODES[args.ray_reconstruction], w, h)
        b = {name: torch.zeros((ih, iw, width), dtype=torch.float32, device="cuda") for name, width in t.RAY_RECONSTRUCTION_INPUTS}
        b["Output"] = accum
        gwidth = dict(t.GBUFFER_CHANNELS)
        gbuf = {name: torch.zeros((ih, iw, gwidth[name]), dtype=torch.float32, device="cuda") for name in t.RESTIR_DI_INPUTS if name not in ("LinearDepth", "MotionVector", "NormalRoughness")}
        dd, ds = (torch.zeros((ih, iw, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        gs = t.graphics_settings(iw, ih, bounces=args.bounces, spp=args.spp)
        ls = {"uniform": None, "power": dict(mode=t.LIGHT_SAMPLING_POWER_RIS), "regir": dict(mode=t.LIGHT_SAMPLING_REGIR_RIS)}[args.light_sampling]
        cd = dict(brdf_samples=args.brdf_samples, boiling_filter=args.boiling_filter)
        prev_cam, rays = None, 0
        for k in range(args.frames):
            gs.FrameIndex = k
            cam = host.camera_matrices(iw, ih, jitter_index=k, jitter_count=32, previous=prev_cam)
            prev_cam = cam
            r.set_camera(cam)
            r.set_constants(gs)
            ptrs = dict({name: v.data_ptr() for name, v in gbuf.items()}, LinearDepth=b["Depth"].data_ptr(), MotionVector=b["MotionVector"].data_ptr(),
                        NormalRoughness=b["NormalRoughness"].data_ptr())
            r.render_gbuffer_device(dict(ptrs, DiffuseAlbedo=b["DiffuseAlbedo"].data_ptr(), SpecularAlbedo=b["SpecularAlbedo"].data_ptr()))
            r.restir_di_device(iw, ih, dict(ptrs, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), frame_index=k, reset_history=k == 0, light_sampling=ls, candidates=cd,
                               **full)
            rays = r.render_sharc_ex_device(b["Color"].data_ptr(), dd.data_ptr(), ds.data_ptr(), None, t.DENOISER_DLSS_RR,
                                            dict(SpecularHitDistance=b["SpecularHitDistance"].data_ptr()), want_stats=True, roughness_threshold=0.4, reset_history=k == 0,
                                            anti_firefly=args.sharc_anti_firefly).rays
            r.ray_reconstruction_device((iw, ih), (w, h), {name: v.data_ptr() for name, v in b.items()}, cam, reset=k == 0)
            r.synchronize()
            for buf in (b["SpecularHitDistance"], dd, ds):  # cleared by the caller, after the calls that read them
                buf.zero_()
            torch.cuda.synchronize()
        hdr = accum
        if args.nis is not None:
            r.nis_sharpen_device((w, h), dict(Color=hdr.data_ptr(), Output=frame.data_ptr()), sharpness=args.nis)
            hdr = frame
        if args.chromatic_aberration is not None:
            src, hdr = hdr, torch.empty_like(frame)
            r.chromatic_aberration_device((w, h), dict(Color=src.data_ptr(), Output=hdr.data_ptr()), offsets=args.chromatic_aberration)
        if args.bloom is not None:
            r.bloom(hdr.data_ptr(), hdr.data_ptr(), w, h, args.bloom)
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(hdr.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        print(f"default frame (pt_render_gbuffer -> pt_restir_di_ex -> pt_render_sharc_ex -> pt_ray_reconstruction {args.ray_reconstruction}, {args.frames} frames, "
              f"{rays} rays in the last) {iw}x{ih} -> {w}x{h} -> {args.out}")
        r.close()
        return
    if args.sharc:
        r.set_camera(host.camera_matrices(w, h, jitter=False))
        rays = 0
        for k in range(args.frames):
            gs.FrameIndex = k
            r.set_constants(gs)
            if args.sharc_anti_firefly:
                rays = r.render_sharc_ex_device(frame.data_ptr(), want_stats=True, roughness_threshold=0.4, reset_history=k == 0, anti_firefly=True).rays
            else:
                rays = r.render_sharc_device(frame.data_ptr(), want_stats=True, roughness_threshold=0.4, reset_history=k == 0).rays
        hdr = frame
        if args.bloom is not None:
            r.bloom(hdr.data_ptr(), hdr.data_ptr(), w, h, args.bloom)
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(hdr.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        print(f"SHARC ({'pt_render_sharc_ex, anti-firefly filter' if args.sharc_anti_firefly else 'pt_render_sharc'}, {args.frames} frames, {rays} rays in the last) {w}x{h} -> {args.out}")
        r.close()
        return
    if args.ray_reconstruction:
        iw, ih = dxrs_amd.load_hip().upscale_input_size(t.UPSCALE_MODES[args.ray_reconstruction], w, h)
        b = {name: torch.zeros((ih, iw, width), dtype=torch.float32, device="cuda") for name, width in t.RAY_RECONSTRUCTION_INPUTS}
        b["Output"] = accum
        torch.cuda.synchronize()
        gs = t.graphics_settings(iw, ih, bounces=args.bounces, spp=args.spp)
        prev_cam = None
        for k in range(args.frames):
            gs.FrameIndex = k
            cam = host.camera_matrices(iw, ih, jitter_index=k, jitter_count=32, previous=prev_cam)
            prev_cam = cam
            r.set_camera(cam)
            r.set_constants(gs)
            r.render_gbuffer_device(dict(LinearDepth=b["Depth"].data_ptr(), MotionVector=b["MotionVector"].data_ptr(), NormalRoughness=b["NormalRoughness"].data_ptr(),
                                         DiffuseAlbedo=b["DiffuseAlbedo"].data_ptr(), SpecularAlbedo=b["SpecularAlbedo"].data_ptr()))
            r.render_denoiser_device(t.DENOISER_DLSS_RR, b["Color"].data_ptr(), dict(SpecularHitDistance=b["SpecularHitDistance"].data_ptr()))
            r.ray_reconstruction_device((iw, ih), (w, h), {name: v.data_ptr() for name, v in b.items()}, cam, reset=k == 0)
            b["SpecularHitDistance"].zero_()  # cleared by the caller, after the call that read it
        hdr = accum
        if args.nis is not None:
            r.nis_sharpen_device((w, h), dict(Color=hdr.data_ptr(), Output=frame.data_ptr()), sharpness=args.nis)
            hdr = frame
        if args.chromatic_aberration is not None:
            src, hdr = hdr, torch.empty_like(frame)
            r.chromatic_aberration_device((w, h), dict(Color=src.data_ptr(), Output=hdr.data_ptr()), offsets=args.chromatic_aberration)
        if args.bloom is not None:
            r.bloom(hdr.data_ptr(), hdr.data_ptr(), w, h, args.bloom)
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(hdr.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        print(f"ray reconstruction {args.ray_reconstruction} (pt_ray_reconstruction, {args.frames} frames) {iw}x{ih} -> {w}x{h} -> {args.out}")
        r.close()
        return
    if args.upscale:
        up = r.upscaler((w, h), mode=t.UPSCALE_MODES[args.upscale])
        iw, ih = up.input_size
        color = torch.zeros((ih, iw, 4), dtype=torch.float32, device="cuda")
        depth = torch.zeros((ih, iw), dtype=torch.float32, device="cuda")
        velocity = torch.zeros((ih, iw, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gs = t.graphics_settings(iw, ih, bounces=args.bounces, spp=args.spp)
        prev_cam = None
        for k in range(args.frames):
            gs.FrameIndex = k
            cam = host.camera_matrices(iw, ih, jitter_index=k, jitter_count=32, previous=prev_cam)
            prev_cam = cam
            r.set_camera(cam)
            r.set_constants(gs)
            r.render_gbuffer_device(dict(LinearDepth=depth.data_ptr(), MotionVector=velocity.data_ptr()))
            r.render_device(color.data_ptr())
            hdr = up(color, depth, velocity, jitter=(-cam.Jitter[0], -cam.Jitter[1]))
        if args.nis is not None:
            r.nis_sharpen_device((w, h), dict(Color=hdr.data_ptr(), Output=frame.data_ptr()), sharpness=args.nis)
            hdr = frame
        if args.chromatic_aberration is not None:
            src, hdr = hdr, torch.empty_like(frame)
            r.chromatic_aberration_device((w, h), dict(Color=src.data_ptr(), Output=hdr.data_ptr()), offsets=args.chromatic_aberration)
        if args.bloom is not None:
            r.bloom(hdr.data_ptr(), hdr.data_ptr(), w, h, args.bloom)
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(hdr.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        print(f"upscale {args.upscale} (pt_upscale, {args.frames} frames) {iw}x{ih} -> {w}x{h} -> {args.out}")
        r.close()
        return
    if args.restir_di:
        r.set_camera(host.camera_matrices(w, h, jitter=False))
        ls = {"uniform": None, "power": dict(mode=t.LIGHT_SAMPLING_POWER_RIS), "regir": dict(mode=t.LIGHT_SAMPLING_REGIR_RIS)}[args.light_sampling]
        cd = dict(brdf_samples=args.brdf_samples, boiling_filter=args.boiling_filter) if args.brdf_samples or args.boiling_filter is not None else None
        for k in range(args.frames):
            gs.FrameIndex = k
            r.set_constants(gs)
            dd, ds, _ = r.restir_di(fill=0.0, reset_history=k == 0, light_sampling=ls, candidates=cd, **full)  # (cleared outputs: a pixel without DI keeps 0)
            r.render_with_di_device(frame.data_ptr(), dd.data_ptr(), ds.data_ptr())
            r.accumulate(accum.data_ptr(), frame.data_ptr(), n, k)
            r.synchronize()
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(accum.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        entry = "pt_restir_di_full, " + args.light_sampling if "shading" in full else "pt_restir_di_ex, " + args.light_sampling if cd else ("pt_restir_di" if ls is None else "pt_restir_di_sampled, " + args.light_sampling)
        print(f"ReSTIR DI ({entry}, {args.frames} frames) {w}x{h} -> {args.out}")
        r.close()
        return
    if args.nrd_denoise:
        mode = t.DENOISER_NRD_REBLUR if args.nrd_denoise == "ReBLUR" else t.DENOISER_NRD_RELAX
        r.set_camera(host.camera(w, h, jitter=False))
        den = r.nrd_reblur_denoiser() if args.nrd_reblur else r.nrd_denoiser(mode)
        for k in range(args.frames):
            gs.FrameIndex = k
            r.set_constants(gs)
            x = r.nrd_chain(mode, denoise=den)
        composed = torch.from_numpy(x["Radiance"].reshape(n, 4)).cuda()
        torch.cuda.synchronize()
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(composed.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        print(f"NRD {args.nrd_denoise} ({'pt_nrd_reblur' if args.nrd_reblur else 'pt_nrd_denoise'}, {args.frames} frames) {w}x{h} -> {args.out}")
        r.close()
        return
    if args.nrd:
        mode = t.DENOISER_NRD_REBLUR if args.nrd == "ReBLUR" else t.DENOISER_NRD_RELAX
        r.set_camera(host.camera(w, h, jitter_index=0, jitter_count=max(args.frames, 8)))
        r.set_constants(gs)
        composed = torch.from_numpy(r.nrd_chain(mode)["Radiance"].reshape(n, 4)).cuda()
        torch.cuda.synchronize()
        op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
        r.tonemap(composed.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
        r.synchronize()
        Image.fromarray(ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)[..., :3]).save(args.out)
        print(f"NRD {args.nrd} (identity denoiser) {w}x{h} -> {args.out}")
        r.close()
        return
    gb = None
    if args.from_gbuffer:
        inputs = t.GBUFFER_FRAME_INPUTS
        size = {name: 4 * width for name, width in t.GBUFFER_CHANNELS} if args.from_gbuffer == "float" else \
            {name: np.dtype(dtype).itemsize * width for name, dtype, width in t.GBUFFER_PACKED}
        gb = {name: torch.zeros(n * size[name], dtype=torch.uint8, device="cuda") for name in inputs}
        torch.cuda.synchronize()
    for k in range(args.frames):
        gs.FrameIndex = k
        if args.aperture is not None:
            r.set_camera(host.camera_lens(w, h, args.aperture, focus_distance, jitter_index=k, jitter_count=max(args.frames, 8)))
        else:
            r.set_camera(host.camera(w, h, jitter_index=k, jitter_count=max(args.frames, 8)))
        r.set_constants(gs)
        if args.aperture is not None:
            r.render_lens_device(frame.data_ptr())
        elif gb is not None:  # (the pass and the frame that reads it are queued on one lane: no wait between them)
            ptrs = {name: b.data_ptr() for name, b in gb.items()}
            (r.render_gbuffer_device if args.from_gbuffer == "float" else r.render_gbuffer_packed_device)(ptrs)
            r.render_from_gbuffer_device(frame.data_ptr(), ptrs, 0 if args.from_gbuffer == "float" else 1)
        else:
            r.render_device(frame.data_ptr())
        r.accumulate(accum.data_ptr(), frame.data_ptr(), n, k)
    op = {"saturate": t.TONE_SATURATE, "reinhard": t.TONE_REINHARD, "aces": t.TONE_ACES_FILMIC}[args.operator]
    hdr = accum
    if args.nis is not None:
        r.nis_sharpen_device((w, h), dict(Color=accum.data_ptr(), Output=frame.data_ptr()), sharpness=args.nis)
        hdr = frame
    if args.chromatic_aberration is not None:
        src, hdr = hdr, torch.empty_like(accum)
        r.chromatic_aberration_device((w, h), dict(Color=src.data_ptr(), Output=hdr.data_ptr()), offsets=args.chromatic_aberration)
    if args.bloom is not None:
        src, hdr = hdr, torch.empty_like(accum)  # the running mean stays as it is
        r.bloom(src.data_ptr(), hdr.data_ptr(), w, h, args.bloom)
    r.tonemap(hdr.data_ptr(), n, t.tonemap_params(op, t.TRANSFER_SRGB, args.exposure), ldr.data_ptr())
    r.synchronize()
    rgba = ldr.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    Image.fromarray(rgba[..., :3]).save(args.out)
    if args.aperture is not None:  # (pt_get_totals does not count pt_render_lens)
        print(f"thin lens (pt_render_lens, aperture {args.aperture}, in focus at {focus_distance}), {args.frames} frames x {args.spp} spp -> {args.out}")
    elif gb is not None:  # (nor pt_render_from_gbuffer)
        print(f"from the {args.from_gbuffer} G-buffer (pt_render_from_gbuffer, {sum(b.numel() for b in gb.values()) // n} bytes per pixel read), {args.frames} frames x {args.spp} spp -> {args.out}")
    else:
        tot = r.totals()
        print(f"{args.frames} frames x {args.spp} spp, {tot.rays} rays -> {args.out}")
    r.close()


if __name__ == "__main__":
    main()
