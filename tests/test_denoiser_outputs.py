"""Row N7 -- the bounce loop's denoiser outputs (pt_render_denoiser: Shaders/Raytracing.hlsl:377-414; DESIGN.md spec S13).
GPU: every output bit for bit against values built in numpy float32 from the CPU oracle (res: oracle_render; isDiffuse / hd: sample 0's
events of oracle_trace_pixel) and the G-buffer's Radiance (prim), with NaN-payload sentinels where a mode writes nothing; exact
consistency with pt_render and pt_render_gbuffer where the oracle does not reach (textures, alpha, environment maps, animation, a
moving camera); DI on; frames in flight; argument errors; the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MISS = 0xFFFFFFFF
SENTINEL = np.uint32(0x7FC0DEAD).view(np.float32)  # a NaN with a payload: survives exactly where nothing is written
DLSS, REBLUR, RELAX = 1, 2, 3
SPLIT = 8  # PT_FLAG_SPLIT_KERNELS


def bits_equal(got, want, what=""):
    """bit-exact equality, NaN payloads included"""
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def setup(r, dxrs, spheres, mats, sd, cam, w, h, textures=None, **gs):
    r.set_scene(spheres, mats, sd)
    if textures is not None:
        r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(dxrs.types.graphics_settings(w, h, **gs))


def sample0(oracle, spheres, mats, sd, cam, gs, rect):
    """per pixel of rect: (primary hit, isDiffuse, hd) from the oracle's sample-0 events"""
    x0, y0, rw, rh = rect
    hit = np.zeros((rh, rw), bool)
    diffuse = np.ones((rh, rw), bool)
    hd = np.full((rh, rw), np.inf, np.float32)
    for y in range(rh):
        for x in range(rw):
            ev = oracle.trace_pixel(spheres, mats, sd, cam, gs, x0 + x, y0 + y)
            ev = ev[ev[:, 0] == 0]
            b0, b1 = ev[ev[:, 1] == 0], ev[ev[:, 1] == 1]
            hit[y, x] = b0[0, 2:3].view(np.uint32)[0] != MISS
            if len(b1):
                diffuse[y, x] = int(b0[0, 14]) == 0  # the lobe sampled at bounce 0 (0 = DiffuseReflection)
                hd[y, x] = b1[0, 3] if b1[0, 2:3].view(np.uint32)[0] != MISS else np.inf
    return hit, diffuse, hd


def expected(res, prim, hit, diffuse, hd, mode, di_d=None, di_s=None):
    """spec S13's table in numpy float32: {name: array} of out and the mode's buffers (SENTINEL where untouched)"""
    h, w = hit.shape
    zero = np.zeros((h, w, 3), np.float32)
    if mode == DLSS:
        shd = np.full((h, w, 1), SENTINEL, np.float32)
        m = hit & ~diffuse & np.isfinite(hd)
        shd[m, 0] = hd[m]
        return {"out": res, "SpecularHitDistance": shd}
    out = np.concatenate([prim, np.ones((h, w, 1), np.float32)], axis=2)
    d = res[..., :3] - prim
    ind = np.where(d > 0, d, np.float32(0)).astype(np.float32)
    di_d = zero if di_d is None else di_d
    di_s = zero if di_s is None else di_s
    dm = diffuse[..., None]
    dif = np.concatenate([di_d + np.where(dm, ind, zero), np.where(dm, hd[..., None], np.float32(0))], axis=2).astype(np.float32)
    spe = np.concatenate([di_s + np.where(dm, zero, ind), np.where(dm, np.float32(0), hd[..., None])], axis=2).astype(np.float32)
    dif[~hit] = SENTINEL
    spe[~hit] = SENTINEL
    return {"out": out, "Diffuse": dif, "Specular": spe}


def check_against_oracle(r, dxrs, oracle, spheres, mats, sd, cam, w, h, rect=None, **gs_kw):
    setup(r, dxrs, spheres, mats, sd, cam, w, h, **gs_kw)
    gs = dxrs.types.graphics_settings(w, h, **gs_kw)
    rect = rect or (0, 0, w, h)
    res, _ = oracle.render(spheres, mats, sd, cam, gs, rect=rect, threads=8)
    prim = r.render_gbuffer(["Radiance"], rect=rect)["Radiance"]
    hit, diffuse, hd = sample0(oracle, spheres, mats, sd, cam, gs, rect)
    assert hit.any()
    for mode in (DLSS, REBLUR, RELAX):
        out, bufs = r.render_denoiser(mode, rect=rect, fill=SENTINEL)
        want = expected(res, prim, hit, diffuse, hd, mode)
        bits_equal(out, want["out"], f"mode {mode}: out")
        for name, arr in bufs.items():
            bits_equal(arr, want[name], f"mode {mode}: {name}")
    img, _ = r.render(rect=rect, want_stats=False)
    bits_equal(img, res, "pt_render")  # (the oracle's radiance is the frame's)
    return hit, diffuse, hd


def transmissive(host, dxrs):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    mats = mats.copy()
    mats["Metallic"][1::2] = 0.0
    mats["Transmission"][1::2] = 1.0
    mats["Roughness"][1::2] = 0.05
    return spheres, mats, sd


ORACLE_CASES = {
    # name: (scene, w, h, rect, graphics settings)
    "c1_b8": ("small", 96, 64, None, dict(bounces=8, spp=1)),
    "c1_b0": ("small", 96, 64, None, dict(bounces=0, spp=1)),
    "c1_b1_spp3": ("small", 96, 64, None, dict(bounces=1, spp=3, frame_index=2)),
    "c1_spp3_rr_off": ("small", 64, 48, None, dict(bounces=8, spp=3, rr=False, frame_index=1)),
    "c1_high_threshold": ("small", 96, 64, None, dict(bounces=8, spp=1, threshold=0.6)),
    "c2_crop": ("demo", 1920, 1080, (928, 500, 64, 32), dict(bounces=8, spp=1, frame_index=3)),
    "c2_crop_spp3": ("demo", 1920, 1080, (1901, 1064, 19, 16), dict(bounces=8, spp=3, frame_index=5)),
    "transmissive": ("transmissive", 320, 180, (96, 64, 64, 48), dict(bounces=8, spp=1)),
}


def scene_of(kind, host, dxrs):
    if kind == "small":
        return host.scene(dxrs.host.SCENE_SMALL, seed=0)
    if kind == "demo":
        return host.scene(dxrs.host.SCENE_DEMO, seed=0)
    return transmissive(host, dxrs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_gpu_bit_exact_against_oracle(dxrs, host, oracle, renderer, case):
    kind, w, h, rect, gs = ORACLE_CASES[case]
    spheres, mats, sd = scene_of(kind, host, dxrs)
    cam = host.camera_matrices(w, h, jitter_index=gs.get("frame_index", 0))
    hit, diffuse, hd = check_against_oracle(renderer, dxrs, oracle, spheres, mats, sd, cam, w, h, rect=rect, **gs)
    if gs["bounces"] == 0:
        assert diffuse[hit].all() and np.isinf(hd).all()  # every sample ends at bounce 0
    elif case == "c1_b8" or case == "transmissive":
        assert (~diffuse & hit).any() and (diffuse & hit & np.isfinite(hd)).any(), "both lobes occur"


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [SPLIT, 0])
def test_gpu_global_memory_tree_and_split_schedule(dxrs, host, oracle, flags):
    """a 10^5-sphere tree in global memory (split schedule by default), and the LDS tree forced into the split schedule"""
    if flags:
        spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
        w, h, rect = 320, 180, (128, 64, 48, 40)
    else:
        spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=100000)
        w, h, rect = 512, 512, (224, 224, 40, 40)
    r = dxrs.Renderer(device=0, flags=flags)
    try:
        cam = host.camera_matrices(w, h, jitter_index=4)
        for spp in (1, 2):
            check_against_oracle(r, dxrs, oracle, spheres, mats, sd, cam, w, h, rect=rect, bounces=8, spp=spp, frame_index=spp)
        if not flags:
            assert not r.accel.lds_resident
    finally:
        r.close()


def consistency(r, w, h, di=False, rect=None):
    """the exact relations of spec S13 that need no oracle, for the frame the next render call renders"""
    gb = r.render_gbuffer(["Radiance", "LinearDepth"], rect=rect)
    prim = gb["Radiance"]
    hit = np.isfinite(gb["LinearDepth"][..., 0])  # the primary hits, independently of the outputs under test (a miss writes inf)
    assert hit.any()
    img, _ = r.render(rect=rect, want_stats=False)
    o1, b1 = r.render_denoiser(DLSS, rect=rect, fill=SENTINEL)
    o2, b2 = r.render_denoiser(REBLUR, rect=rect, fill=SENTINEL)
    o3, b3 = r.render_denoiser(RELAX, rect=rect, fill=SENTINEL)
    bits_equal(o1, img, "DLSS-RR out == pt_render")
    bits_equal(o2[..., :3], prim, "NRD out == G-buffer Radiance")
    bits_equal(o3, o2, "ReLAX out == ReBLUR out")
    bits_equal(b3["Diffuse"], b2["Diffuse"], "ReLAX Diffuse == ReBLUR")
    bits_equal(b3["Specular"], b2["Specular"], "ReLAX Specular == ReBLUR")
    for name in ("Diffuse", "Specular"):  # written exactly on the hits
        assert (np.isnan(b2[name]).all(axis=-1) == ~hit).all(), name
        bits_equal(b2[name][~hit], np.full(b2[name][~hit].shape, SENTINEL, np.float32), f"{name} on misses")
    shd = b1["SpecularHitDistance"][..., 0]
    written = ~np.isnan(shd)
    assert (written <= hit).all()
    bits_equal(b2["Specular"][..., 3][written], shd[written], "Specular.a == SpecularHitDistance")
    assert (b2["Diffuse"][..., 3][written] == 0).all()
    if not di:
        d = img[..., :3] - prim
        ind = np.where(d > 0, d, np.float32(0)).astype(np.float32)
        bits_equal((b2["Diffuse"][..., :3] + b2["Specular"][..., :3])[hit], ind[hit], "Diffuse + Specular == max(pt_render - prim, 0)")
    return img, prim, o2, b2, hit


@pytest.mark.gpu
def test_gpu_textured_scene_with_environment_map(dxrs, host, renderer):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    ts, sd = host.demo_textures(seed=0, time=0.0, environment_map=True, return_scene_data=True)
    w, h = 480, 270
    setup(renderer, dxrs, spheres, mats, sd, host.camera_matrices(w, h, jitter_index=2), w, h, textures=ts, bounces=8, spp=1)
    consistency(renderer, w, h)
    renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=3, bounces=6, spp=2))
    consistency(renderer, w, h, rect=(40, 24, 200, 120))
    renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_alpha_scene(dxrs, host):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    ts, sd = host.demo_textures(seed=0, time=0.0, environment_map=False, return_scene_data=True)
    mats = mats.copy()
    mats["AlphaMode"][::3] = 2  # Mask
    mats["AlphaCutoff"][::3] = 0.5
    w, h = 320, 180
    r = dxrs.Renderer(device=0)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h, jitter_index=1), w, h, textures=ts, bounces=8, spp=1)
        consistency(r, w, h)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_animation_refit_and_moving_camera(dxrs, host):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    sd.IsStatic = 0
    w, h = 320, 180
    r = dxrs.Renderer(device=0)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h), w, h, bounces=8, spp=1)
        for f in range(4):
            moved = spheres.copy()
            moved["cy"] += np.float32(0.1 * f) * np.sin(np.arange(len(spheres), dtype=np.float32))
            r.update_spheres(moved)
            # the camera moves and turns
            r.set_camera(host.camera_matrices(w, h, position=(0.3 * f, 0.0, -15.0 + 0.2 * f), look_at=(0.5 * f, 0.2 * f, 0.0), jitter_index=f))
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
            consistency(r, w, h)
    finally:
        r.close()


def check_di(r, dxrs, host, w, h):
    """DI on: the consistency relations, out + Diffuse + Specular against the pt_render frame on hits, and an all-metal scene's
    Diffuse.rgb == 0 (no diffuse lobe: no diffuse half of the DI, every first bounce specular)"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    for spp in (1, 2):
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h, jitter_index=spp), w, h, bounces=8, spp=spp, di=True, frame_index=spp)
        img, prim, o2, b2, hit = consistency(r, w, h, di=True)
        total = o2[..., :3] + b2["Diffuse"][..., :3] + b2["Specular"][..., :3]
        ref = img[..., :3]
        err = np.abs(total.astype(np.float64) - ref)[hit]
        assert (err <= np.maximum(1e-5 * np.abs(ref[hit]), 1e-7)).all(), float(err.max())
        assert (b2["Diffuse"][..., :3][hit] > 0).any() and (b2["Specular"][..., :3][hit] > 0).any()
    metal = mats.copy()
    metal["Metallic"][:] = 1.0
    setup(r, dxrs, spheres, metal, sd, host.camera_matrices(w, h), w, h, bounces=8, spp=1, di=True)
    _, _, _, b2, hit = consistency(r, w, h, di=True)
    assert (b2["Diffuse"][..., :3][hit] == 0).all()


@pytest.mark.gpu
def test_gpu_direct_illumination(dxrs, host, renderer):
    """DI made inside the fused primary pass"""
    check_di(renderer, dxrs, host, 480, 270)


@pytest.mark.gpu
def test_gpu_direct_illumination_split_schedule(dxrs, host):
    """DI made by di_kernel before the shade passes (its kSplit form in the NRD modes)"""
    r = dxrs.Renderer(device=0, flags=SPLIT)
    try:
        r.set_profiling(True)
        check_di(r, dxrs, host, 320, 180)
        assert r.profile(reset=True).shade_launches > 0  # (the split schedule ran)
    finally:
        r.close()


def knob_renderer(dxrs, knobs, **kw):
    """a context created with the PT_* knobs set (they are read once, at pt_create)"""
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        return dxrs.Renderer(device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["640x360", "1280x720"])
def test_gpu_schedules_with_a_separate_looping_pass(dxrs, host, size):
    """the forms of big frames and of frames in flight: the compacting primary pass without kFuse (its primary-cache records at spp > 1),
    then a separate looping pass -- at 1 spp, and merged at spp > 1 with the cache-mode-2 restarts whose finish takes the pixel index
    from the records.  PT_FUSE_LOOP=0 forces them at any size; 1280x720 (>= 400k slots) takes them by itself at spp > 1."""
    w, h = map(int, size.split("x"))
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    knobs = {"PT_FUSE_LOOP": "0"} if w == 640 else {}
    r = knob_renderer(dxrs, knobs, frames_in_flight=3)
    try:
        r.set_profiling(True)
        for spp in ((1, 3) if knobs else (2,)):
            setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h, jitter_index=spp), w, h, bounces=8, spp=spp, frame_index=spp)
            r.profile(reset=True)
            consistency(r, w, h)
            p = r.profile(reset=True)
            assert p.tail_launches >= 4 and p.traverse_launches >= 4, (p.tail_launches, p.traverse_launches)  # one looping pass per frame
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h), w, h, bounces=8, spp=2, di=True)
        consistency(r, w, h, di=True)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """three lanes alternate pt_render and pt_render_denoiser over rotating buffers: every frame equals the same frame rendered alone"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 640, 360
    frames = 9

    def cam_of(f):
        return host.camera_matrices(w, h, position=(0.0, 0.0, -15.0 + 0.05 * f), jitter_index=f)

    def mode_of(f):
        return (0, DLSS, REBLUR)[f % 3] if f % 2 else 0

    def fill(shape):
        return torch.from_numpy(np.full(shape, SENTINEL, np.float32)).to("cuda")

    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        r.set_scene(spheres, mats, sd)
        sets = [dict(out=fill((h, w, 4)), Diffuse=fill((h, w, 4)), Specular=fill((h, w, 4)), SpecularHitDistance=fill((h, w, 1))) for _ in range(3)]
        torch.cuda.synchronize()
        got = []
        for f in range(frames):
            r.set_camera(cam_of(f))
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
            s = sets[f % 3]
            if mode_of(f):
                r.render_denoiser_device(mode_of(f), s["out"].data_ptr(), {k: v.data_ptr() for k, v in s.items() if k != "out"})
            else:
                r.render_device(s["out"].data_ptr())
            if f % 3 == 2:
                r.synchronize()
                got += [{k: v.cpu().numpy().copy() for k, v in x.items()} for x in sets]
                for x in sets:
                    for v in x.values():
                        v.copy_(fill(tuple(v.shape)))
                torch.cuda.synchronize()
        r.synchronize()
    finally:
        r.close()
    alone = dxrs.Renderer(device=0)
    try:
        alone.set_scene(spheres, mats, sd)
        for f in range(frames):
            alone.set_camera(cam_of(f))
            alone.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
            if mode_of(f):
                out, bufs = alone.render_denoiser(mode_of(f), fill=SENTINEL)
                bits_equal(got[f]["out"], out, f"frame {f}: out")
                for k, v in bufs.items():
                    bits_equal(got[f][k], v, f"frame {f}: {k}")
            else:
                img, _ = alone.render(want_stats=False)
                bits_equal(got[f]["out"], img, f"frame {f}: pt_render")
    finally:
        alone.close()


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, host, renderer):
    from dxrs_amd.types import PtDenoiserOutputs, PtRect
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    buf = torch.zeros(64 * 64 * 4 + 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(64 * 64 * 4, dtype=torch.float32, device="cuda")
    p, o = buf.data_ptr(), C.c_void_p(out.data_ptr())
    fresh = dxrs.Renderer(device=0)
    try:
        assert lib.pt_render_denoiser(fresh._ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=1, SpecularHitDistance=p)), None) == 4  # no scene
    finally:
        fresh.close()
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    setup(renderer, dxrs, spheres, mats, sd, host.camera_matrices(64, 64), 64, 64)
    for mode in (0, 4, 99):
        assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=mode, Diffuse=p, Specular=p, SpecularHitDistance=p)), None) == 1
    assert lib.pt_render_denoiser(ctx, None, o, 1, None, None) == 1
    assert lib.pt_render_denoiser(ctx, None, None, 1, C.byref(PtDenoiserOutputs(Denoiser=1, SpecularHitDistance=p)), None) == 1
    assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=1, Diffuse=p, Specular=p)), None) == 1
    assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=1, SpecularHitDistance=p + 2)), None) == 1
    for mode in (2, 3):
        assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=mode, Diffuse=p, SpecularHitDistance=p)), None) == 1
        assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=mode, Specular=p)), None) == 1
        assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=mode, Diffuse=p + 4, Specular=p)), None) == 1
        assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(PtDenoiserOutputs(Denoiser=mode, Diffuse=p, Specular=p + 8)), None) == 1
    ok = PtDenoiserOutputs(Denoiser=2, Diffuse=p, Specular=p)
    assert lib.pt_render_denoiser(ctx, C.byref(PtRect(60, 0, 8, 8)), o, 1, C.byref(ok), None) == 1
    assert lib.pt_render_denoiser(ctx, C.byref(PtRect(0, 0, 0, 8)), o, 1, C.byref(ok), None) == 1
    gs = dxrs.types.graphics_settings(64, 64)
    gs.Denoiser = 2
    assert lib.pt_set_constants(ctx, C.byref(gs)) == 5  # the constants still refuse a denoiser: it is named per frame
    assert lib.pt_render_denoiser(ctx, None, o, 1, C.byref(ok), None) == 0  # the context still works
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """Raytracing::Render(radiance, DenoiserBuffers&) (host/Raytracing.hpp) from C++: the demo frame's outputs equal the Python path's
    wherever the mode writes, and Render(radiance) still refuses a denoiser"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_denoiser")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_denoiser.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 160, 90
    n = w * h
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera(w, h, jitter=False), w, h, bounces=8, spp=1)
        for mode in (DLSS, REBLUR, RELAX):
            outp = str(tmp_path / f"dn{mode}.f32")
            res = subprocess.run([exe, str(w), str(h), str(mode), outp], capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stdout + res.stderr
            raw = np.fromfile(outp, dtype=np.float32)
            out, bufs = r.render_denoiser(mode, fill=SENTINEL)
            bits_equal(raw[:n * 4].reshape(h, w, 4), out, f"C++ mode {mode}: out")
            at = n * 4
            for name, width in dxrs.abi_types.DENOISER_OUTPUTS[mode]:
                got = raw[at:at + n * width].reshape(h, w, width)
                at += n * width
                written = bufs[name].view(np.uint32) != SENTINEL.view(np.uint32)
                assert written.any()
                bits_equal(got[written], bufs[name][written], f"C++ mode {mode}: {name}")
    finally:
        r.close()
