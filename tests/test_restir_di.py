"""Row N10 -- a frame whose direct illumination the caller supplies (pt_render_with_di: the reference's frame with IsDIEnabled =
isReSTIRDIEnabled, Source/App.cpp:1262; DI = Diffuse.rgb + Specular.rgb, Raytracing.hlsl:160).
CPU: the C-ABI exports and rejects what it can without a GPU.
GPU: the supplied DI is consumed exactly -- out == f32(res0 + f32(Dd + Ds)) on primary hits, res0 (the same frame with D = 0) on misses --
at 1 spp and spp > 1, in the fused one-launch form, the split schedule, beam-list frames and textured scenes; fed the oracle's row-N4
estimates it reproduces the oracle's N4 frame bit for bit; in the denoiser modes the outputs follow spec S13 with the supplied halves,
also with the DI buffers aliased to the frame's own outputs."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from test_denoiser_outputs import SENTINEL, bits_equal

HERE = os.path.dirname(os.path.abspath(__file__))
DLSS, REBLUR, RELAX = 1, 2, 3
SPLIT = 8  # PT_FLAG_SPLIT_KERNELS


# ---------------------------------------------------------------------------------------------------- CPU: ABI
def test_render_with_di_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_render_with_di") and "pt_render_with_di" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtDirectLighting
    assert C.sizeof(PtDirectLighting) == 16 and PtDirectLighting.Specular.offset == 8
    buf = (C.c_float * 64)()
    di = PtDirectLighting(Diffuse=C.addressof(buf), Specular=C.addressof(buf))
    assert lib.pt_render_with_di(None, None, C.addressof(buf), 1, C.byref(di), None, None) == 1  # PT_ERR_INVALID_ARG: null context
    assert lib.pt_last_error(None) == b"null context"


# ---------------------------------------------------------------------------------------------------- GPU helpers
def setup(r, dxrs, spheres, mats, sd, cam, w, h, textures=None, **gs):
    r.set_scene(spheres, mats, sd)
    r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(dxrs.types.graphics_settings(w, h, **gs))


def random_di(rng, h, w):
    """non-negative DI with a few exact zeros and large values (.w: a distance, not read)"""
    d = rng.exponential(0.5, (h, w, 4)).astype(np.float32)
    d[rng.random((h, w)) < 0.1, :3] = 0
    d[rng.random((h, w)) < 0.01, :3] *= 1e4
    return d


def primary_hits(r, rect):
    return np.isfinite(r.render_gbuffer(["LinearDepth"], rect=rect)["LinearDepth"][..., 0])


def check_consumption(r, rng, rect, rested=False):
    """out == f32(res0 + f32(Dd + Ds)) where the primary ray hit, res0 elsewhere; res0 = the same frame with D = 0"""
    x0, y0, w, h = rect
    hit = primary_hits(r, rect)
    assert hit.any()
    zero = np.zeros((h, w, 4), np.float32)
    dd, ds = random_di(rng, h, w), random_di(rng, h, w)
    reps = 3 if rested else 1  # (the third frame of a rested view takes its primary candidates from the beam lists)
    res0 = [r.render_with_di(zero, zero, rect=rect) for _ in range(reps)][-1]
    out = [r.render_with_di(dd, ds, rect=rect) for _ in range(reps)][-1]
    want = res0.copy()
    s = (dd[..., :3] + ds[..., :3]).astype(np.float32)
    want[..., :3] = np.where(hit[..., None], (res0[..., :3] + s).astype(np.float32), res0[..., :3])
    bits_equal(out, want, "out == res0 + (Dd + Ds)")
    return res0, hit


CONSUMPTION_CASES = {
    # name: (scene, w, h, rect, graphics settings, renderer flags)
    "c1_spp1": ("small", 96, 64, None, dict(bounces=8, spp=1), 0),
    "c1_spp3": ("small", 96, 64, None, dict(bounces=6, spp=3, frame_index=2), 0),
    "c2_crop_rested": ("demo", 1920, 1080, (928, 500, 64, 32), dict(bounces=8, spp=1, frame_index=3), 0),
    "c2_crop_spp2_rested": ("demo", 1920, 1080, (900, 480, 40, 24), dict(bounces=8, spp=2, frame_index=5), 0),
    "c2_split": ("demo", 320, 180, (128, 64, 48, 40), dict(bounces=8, spp=1), SPLIT),
    "c2_split_spp2": ("demo", 320, 180, (128, 64, 48, 40), dict(bounces=8, spp=2), SPLIT),
    "textured": ("textured", 160, 96, None, dict(bounces=6, spp=1, frame_index=1), 0),
    "global_tree": ("procedural", 256, 256, (96, 96, 40, 40), dict(bounces=8, spp=1), 0),
}


def scene_of(kind, host, dxrs):
    if kind == "small":
        return host.scene(dxrs.host.SCENE_SMALL, seed=0) + (None,)
    if kind == "demo":
        return host.scene(dxrs.host.SCENE_DEMO, seed=0) + (None,)
    if kind == "procedural":
        return host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=100000) + (None,)
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    ts, sd = host.demo_textures(seed=0, time=0.0, environment_map=True, return_scene_data=True)
    return spheres, mats, sd, ts


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CONSUMPTION_CASES))
def test_gpu_with_di_consumes_the_supplied_di(dxrs, host, case):
    kind, w, h, rect, gs, flags = CONSUMPTION_CASES[case]
    spheres, mats, sd, ts = scene_of(kind, host, dxrs)
    r = dxrs.Renderer(device=0, flags=flags)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h, jitter_index=gs.get("frame_index", 0)), w, h, textures=ts, **gs)
        rng = np.random.default_rng(zlib.crc32(case.encode()))
        res0, hit = check_consumption(r, rng, rect or (0, 0, w, h), rested="rested" in case)
        # D = 0 is the frame with DI on and nothing supplied: the emission reached by a reflective first bounce is dropped (N4's gate), so
        # where the scene has emitters it differs from pt_render without DI; misses are the environment either way
        r.set_constants(dxrs.types.graphics_settings(w, h, **gs))
        plain, _ = r.render(rect, want_stats=False)
        bits_equal(res0[~hit], plain[~hit], "misses: environment")
        if kind == "procedural":
            assert not r.accel.lds_resident
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_with_di_frames_in_flight(dxrs, host):
    """three lanes, buffers rotated as the contract asks: every frame consumes its own DI"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 128, 96
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h), w, h, bounces=8, spp=1)
        import torch
        rng = np.random.default_rng(5)
        hit = primary_hits(r, None)
        dev = torch.device("cuda", 0)
        ds = [torch.from_numpy(random_di(rng, h, w)).to(dev) for _ in range(6)]
        zero = torch.zeros((h, w, 4), device=dev)
        outs = [torch.full((h, w, 4), float("nan"), device=dev) for _ in range(3)]
        torch.cuda.synchronize(dev)
        r.render_with_di_device(outs[0].data_ptr(), zero.data_ptr(), zero.data_ptr())
        r.synchronize()
        res0 = outs[0].cpu().numpy()
        got = []
        for k in range(6):
            o = outs[k % 3]
            r.render_with_di_device(o.data_ptr(), ds[k].data_ptr(), zero.data_ptr())
            if k % 3 == 2:
                r.synchronize()
                got += [x.cpu().numpy() for x in outs]
        for k in range(6):
            want = res0.copy()
            d = ds[k].cpu().numpy()
            want[..., :3] = np.where(hit[..., None], (res0[..., :3] + (d[..., :3] + np.float32(0))).astype(np.float32), res0[..., :3])
            bits_equal(got[k], want, f"frame {k}")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 3])
def test_gpu_with_di_reproduces_the_oracle_n4_frame(dxrs, host, oracle, renderer, spp):
    """fed the oracle's row-N4 estimates (Dd = est, Ds = 0), the frame is the oracle's N4 frame bit for bit"""
    from test_direct_illumination import lit_scene
    t = dxrs.types
    spheres, mats = lit_scene(dxrs, n_lights=3, glass=True)
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    w, h = 48, 32
    cam = host.camera(w, h, position=(0, 1.5, -7), jitter_index=spp)
    gs = t.graphics_settings(w, h, frame_index=7 * spp, bounces=4, spp=spp, di=True)
    ref, _ = oracle.render(spheres, mats, sd, cam, gs, threads=8)
    est = np.zeros((h, w, 4), np.float32)
    for y in range(h):
        for x in range(w):
            _, rec, _ = oracle.trace_pixel_ex(spheres, mats, sd, cam, gs, x, y)
            est[y, x, :3] = rec[7:10]
    assert (est[..., :3] > 0).any()
    renderer.set_scene(spheres, mats, sd)
    renderer.set_textures(None)
    renderer.set_camera(cam)
    renderer.set_constants(t.graphics_settings(w, h, frame_index=7 * spp, bounces=4, spp=spp, di=False))  # (IsDIEnabled is not what decides)
    out = renderer.render_with_di(est, np.zeros_like(est))
    bits_equal(out[..., :3], ref[..., :3], "pt_render_with_di(N4 estimates) == the oracle's N4 frame")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, SPLIT])
def test_gpu_with_di_denoiser_modes(dxrs, host, flags):
    """spec S13 with the supplied halves: NRD Diffuse = Dd + Diffuse(D = 0), Specular = Ds + Specular(D = 0), the rest unchanged; DLSS-RR
    out = out(D = 0) + (Dd + Ds); the same with the DI buffers aliased to the outputs"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h, rect = 320, 180, (120, 60, 56, 40)
    r = dxrs.Renderer(device=0, flags=flags)
    try:
        for spp in (1, 2):
            setup(r, dxrs, spheres, mats, sd, host.camera_matrices(w, h, jitter_index=spp), w, h, bounces=8, spp=spp, frame_index=spp)
            rng = np.random.default_rng(spp + flags)
            hit = primary_hits(r, rect)
            zero = np.zeros((rect[3], rect[2], 4), np.float32)
            dd, ds = random_di(rng, rect[3], rect[2]), random_di(rng, rect[3], rect[2])
            o0, b0 = r.render_with_di(zero, zero, rect=rect, mode=DLSS, fill=SENTINEL)
            o1, b1 = r.render_with_di(dd, ds, rect=rect, mode=DLSS, fill=SENTINEL)
            want = o0.copy()
            want[..., :3] = np.where(hit[..., None], (o0[..., :3] + (dd[..., :3] + ds[..., :3]).astype(np.float32)).astype(np.float32), o0[..., :3])
            bits_equal(o1, want, "DLSS-RR out")
            bits_equal(b1["SpecularHitDistance"], b0["SpecularHitDistance"], "DLSS-RR SpecularHitDistance")
            for mode in (REBLUR, RELAX):
                o0, b0 = r.render_with_di(zero, zero, rect=rect, mode=mode, fill=SENTINEL)
                o1, b1 = r.render_with_di(dd, ds, rect=rect, mode=mode, fill=SENTINEL)
                bits_equal(o1, o0, f"mode {mode}: out (the primary emission)")
                for name, d in (("Diffuse", dd), ("Specular", ds)):
                    want = b0[name].copy()
                    want[hit, :3] = (d[hit, :3] + b0[name][hit, :3]).astype(np.float32)
                    bits_equal(b1[name], want, f"mode {mode}: {name}")
                    assert np.isnan(b1[name][~hit]).all()
                o2, b2 = r.render_with_di(dd, ds, rect=rect, mode=mode, fill=SENTINEL, alias=True)
                bits_equal(o2, o1, f"mode {mode} aliased: out")
                for name, d in (("Diffuse", dd), ("Specular", ds)):
                    want = b1[name].copy()
                    want[~hit] = d[~hit]  # (misses are never written: the aliased buffer keeps its DI there)
                    bits_equal(b2[name], want, f"mode {mode} aliased: {name}")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_with_di_argument_errors(dxrs, host, renderer):
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    w, h = 32, 16
    setup(renderer, dxrs, spheres, mats, sd, host.camera_matrices(w, h), w, h, bounces=2, spp=1)
    dev = torch.device("cuda", 0)
    buf = torch.zeros((h * w + 1, 4), device=dev)
    out = torch.zeros((h, w, 4), device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(dxrs.PtError, match="null direct lighting"):
        renderer.render_with_di_device(out.data_ptr(), 0, buf.data_ptr())
    with pytest.raises(dxrs.PtError, match="16-byte aligned"):
        renderer.render_with_di_device(out.data_ptr(), buf.data_ptr() + 4, buf.data_ptr())
    with pytest.raises(dxrs.PtError, match="Denoiser must be"):
        renderer.render_with_di_device(out.data_ptr(), buf.data_ptr(), buf.data_ptr(), mode=4)
    with pytest.raises(dxrs.PtError, match="NRD modes need"):
        renderer.render_with_di_device(out.data_ptr(), buf.data_ptr(), buf.data_ptr(), mode=REBLUR)
    renderer.render_with_di_device(out.data_ptr(), buf.data_ptr(), buf.data_ptr())  # and the context still works
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """Raytracing::Render(radiance, DirectLighting) (host/Raytracing.hpp) from C++: a ReBLUR frame's Diffuse / Specular fed back as the next
    frame's DI give the Python path's frame bit for bit"""
    import subprocess
    import torch
    pkg = os.path.join(os.path.dirname(HERE), "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_with_di")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_with_di.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 160, 90
    outp = str(tmp_path / "with_di.f32")
    res = subprocess.run([exe, str(w), str(h), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(outp, dtype=np.float32).reshape(h, w, 4)
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0)
    try:
        setup(r, dxrs, spheres, mats, sd, host.camera(w, h, jitter=False), w, h, bounces=8, spp=1)
        dev = torch.device("cuda", 0)
        nd, ns, tmp, out = (torch.zeros((h, w, 4), device=dev) for _ in range(4))
        torch.cuda.synchronize(dev)
        r.render_denoiser_device(REBLUR, tmp.data_ptr(), {"Diffuse": nd.data_ptr(), "Specular": ns.data_ptr()})
        r.render_with_di_device(out.data_ptr(), nd.data_ptr(), ns.data_ptr())
        r.synchronize()
        got = out.cpu().numpy()
        assert (nd.cpu().numpy()[..., :3] > 0).any()
        bits_equal(raw, got, "C++ mirror == Python path")
    finally:
        r.close()
