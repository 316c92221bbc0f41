"""Row N18 -- pt_render_sharc_ex, the frame through the radiance cache with the frame's direct illumination and the denoiser outputs
(DESIGN.md spec S24).
CPU: the host-compiled header (tests/hostshim/sharc_ex_host.cpp over csrc/pt_sharc.h's _ex functions): extras off against the existing
shim; exact known answers on a black scene; the any(DI > 0) gate; the NRD modes' rule; the outputs' known answers; the guide signals'
independence of the cache; no double counting of the direct light; a sanitizer build of a stand-alone program.
GPU: extras off against pt_render_sharc; the empty cache against pt_render_denoiser and pt_render_with_di; the kernels against the host
header bit for bit; the chain gbuffer -> restir -> cache -> ray reconstruction queued and synchronised; the argument rules; the C++ mirror."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import restir_reference as rref
from test_restir_pass import cpu_gbuffer, make_scene
from test_restir_pass import shims as restir_shims  # noqa: F401  (a fixture)
from test_sharc import CAP, GH, GW, QUERY, RESOLVE, UPDATE, H, HostCache, W, c1, cache_map, defaults, gpu_content, p, same_bits, setup
from test_sharc import cpu_scene, shims  # noqa: F401  (fixtures)

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
OUTPUTS = {1: (("SpecularHitDistance", 1),), 2: (("Diffuse", 4), ("Specular", 4)), 3: (("Diffuse", 4), ("Specular", 4))}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def is_sentinel(a):
    return bits(a) == SENTINEL.view(np.uint32)


# ---------------------------------------------------------------------------------------------------- the host-compiled header
@pytest.fixture(scope="module")
def ex_lib():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_sharc_ex_shim())
    vp, u32 = C.c_void_p, C.c_uint32
    lib.sh_host_call_ex.restype = None
    lib.sh_host_call_ex.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.sh_host_texel.restype = None
    lib.sh_host_texel.argtypes = [vp, u32, u32, vp]
    lib.sh_host_trace_both.restype = None
    lib.sh_host_trace_both.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp]
    return lib


class HostCacheEx(HostCache):
    """pt_render_sharc_ex over the host-compiled header: HostCache with the DI and the denoiser outputs of a call"""

    def __init__(self, ex, lib, gbshim, spheres, mats, sd, textures=None):
        super().__init__(lib, gbshim, spheres, mats, sd, textures)
        self.ex = ex

    def call_ex(self, cam, gs, rect=None, di=None, mode=0, alias=False, **kw):
        """-> (image (h, w, 4) or None, {output: array}, rays, failed inserts).  di = (Diffuse, Specular) float32 (h, w, 4) or None; the image
        and the outputs start as the sentinel; alias (NRD modes): the outputs are the DI's own arrays (copies of them)"""
        s = defaults(**kw)
        stages = s["stages"] or 7
        w, h = gs.RenderSize[0], gs.RenderSize[1]
        rect = rect or (0, 0, w, h)
        if self.capacity != s["capacity"]:
            self.capacity, self.valid = s["capacity"], False
            self.keys = np.zeros(self.capacity, np.uint64)
            self.accum, self.resolved = np.zeros((self.capacity, 4), np.uint32), np.zeros((self.capacity, 4), np.uint32)
        if s["reset_history"] or not self.valid:
            self.keys[:] = 0
            self.accum[:] = 0
            self.resolved[:] = 0
        self.valid = True
        prm = np.array([w, h, gs.FrameIndex, gs.Bounces, gs.SamplesPerPixel, gs.IsRussianRouletteEnabled, s["capacity"], s["downscale_factor"],
                        s["accumulation_frames"], s["max_stale_frames"], int(s["visualize"]), stages, *rect], np.uint32)
        fprm = np.array([gs.ThroughputThreshold, s["scene_scale"], s["roughness_threshold"]], np.float32)
        out = np.full((rect[3], rect[2], 4), SENTINEL, np.float32)
        dd, ds = (np.ascontiguousarray(a, dtype=np.float32).copy() for a in di) if di is not None else (None, None)
        bufs = {name: np.full((rect[3], rect[2], width), SENTINEL, np.float32) for name, width in OUTPUTS.get(mode, ())}
        if alias and mode >= 2:
            bufs = {"Diffuse": dd, "Specular": ds}
        counters = np.zeros(2, np.uint64)
        self.ex.sh_host_call_ex(p(self.spheres), p(self.mats), len(self.spheres), p(self.env), p(self.texels), p(self.info), 0 if self.info is None else len(self.info),
                                p(self.maps), p(self.rot), C.addressof(cam), p(prm), p(fprm), p(self.keys), p(self.accum), p(self.resolved), p(out), p(counters),
                                p(dd), p(ds), mode, p(bufs.get("SpecularHitDistance")), p(bufs.get("Diffuse")), p(bufs.get("Specular")))
        if stages & RESOLVE:
            self.accum, self.resolved = self.resolved, self.accum
        return (out if stages & QUERY else None), bufs, int(counters[0]), int(counters[1])


def c1_cpu(dxrs, host, w, h):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    return spheres, mats, sd, host.camera_matrices(w, h, jitter=False)


def constant_di(w, h, d=(0.25, 0.5, 0.125), s=(0.125, 0.25, 0.0625)):
    """a DI whose sums have short mantissas: up to four of them add without rounding.  .w is not read: it holds a NaN"""
    dd, ds = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    dd[..., :3], ds[..., :3] = d, s
    dd[..., 3] = ds[..., 3] = np.nan
    return dd, ds


def random_di(w, h, seed, zero_fraction=0.0):
    rng = np.random.default_rng(seed)
    dd, ds = (rng.uniform(0.01, 2.0, (h, w, 4)).astype(np.float32) for _ in range(2))
    if zero_fraction:
        off = rng.random((h, w)) < zero_fraction
        dd[off, :3] = 0.0
        ds[off, :3] = 0.0
    return dd, ds


# ---------------------------------------------------------------------------------------------------- CPU 1: ABI
def test_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_render_sharc_ex") and "pt_render_sharc_ex" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtSharcSettings
    s = PtSharcSettings()
    assert lib.pt_render_sharc_ex(None, None, None, 0, C.byref(s), None, None, None) == 1  # PT_ERR_INVALID_ARG: null context


def test_update_texel_of_a_uv(ex_lib):
    """clamp(uint(u * n), 0, n - 1): the borders, both ends, values outside [0, 1) and NaN"""
    u = np.array([0.0, 0.0104, 0.0105, 0.5, 0.999999, 1.0, 1.5, -0.25, np.nan, np.inf, 1e30], np.float32)
    t = np.zeros(len(u), np.uint32)
    ex_lib.sh_host_texel(p(u), len(u), 96, p(t))
    assert list(t) == [0, 0, 1, 48, 95, 95, 95, 0, 0, 95, 95]


# ---------------------------------------------------------------------------------------------------- CPU 2: extras off
@pytest.mark.parametrize("scene", ["test", "c1"])
def test_extras_off_is_pt_render_sharc(dxrs, host, shims, ex_lib, cpu_scene, scene):
    w, h = (W, H) if scene == "test" else (24, 16)
    spheres, mats, sd, cam = cpu_scene if scene == "test" else c1_cpu(dxrs, host, w, h)
    old, new = HostCache(*shims, spheres, mats, sd), HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    for f in range(3):
        gs = dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=2 if f == 2 else 1)
        st = dict(capacity=1 << 12, reset_history=f == 0)
        want, rays, failed = old.call(cam, gs, **st)
        got, bufs, rays_ex, failed_ex = new.call_ex(cam, gs, **st)
        assert same_bits(got, want) and not bufs and (rays_ex, failed_ex) == (rays, failed)
        assert new.content() == old.content() and len(old.content()) > 20


# ---------------------------------------------------------------------------------------------------- CPU 3: a black scene
def black_scene(dxrs):
    spheres, mats, sd = make_scene(dxrs)
    mats = mats.copy()
    mats["EmissiveStrength"][:] = 0.0
    sd.EnvironmentLightColor[0] = sd.EnvironmentLightColor[1] = sd.EnvironmentLightColor[2] = 0.0
    return spheres, mats, sd


def update_paths_that_hit(lib, hc, cam, gs, st):
    """per path of the update grid, from the existing shim: does the path's own primary ray hit?"""
    s = defaults(**st)
    w, h = gs.RenderSize[0], gs.RenderSize[1]
    gw, gh = w // s["downscale_factor"], h // s["downscale_factor"]
    prm = np.array([w, h, 0, gs.Bounces, 1, 1, s["capacity"], s["downscale_factor"], 10, 64, 0, 7, 0, 0, w, h], np.uint32)
    fprm = np.array([gs.ThroughputThreshold, s["scene_scale"], s["roughness_threshold"]], np.float32)
    frames = np.array([gs.FrameIndex], np.uint32)
    keys, rgb = np.zeros(gw * gh, np.uint64), np.zeros((gw * gh, 3), np.float32)
    lib.sh_host_estimates(p(hc.spheres), p(hc.mats), len(hc.spheres), p(hc.env), C.addressof(cam), p(prm), p(fprm), p(frames), 1, p(keys), p(rgb))
    return int((keys != 0).sum())


def test_black_scene_known_answers(dxrs, host, shims, ex_lib, cpu_scene):
    spheres, mats, sd = black_scene(dxrs)
    cam = cpu_scene[3]
    hc = HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    di = constant_di(W, H)
    c = di[0][0, 0, :3] + di[1][0, 0, :3]
    gs = dxrs.types.graphics_settings(W, H, frame_index=4, bounces=6, spp=1)
    st = dict(capacity=1 << 14, downscale_factor=2)
    hits = update_paths_that_hit(shims[0], hc, cam, gs, st)
    assert 100 < hits < (W // 2) * (H // 2)
    # update on an empty cache: every path that hits adds round(c * 1024) to the voxel of its first vertex, and nothing else is positive
    _, _, _, failed = hc.call_ex(cam, gs, di=di, stages=UPDATE | RESOLVE, reset_history=True, **st)
    sums = hc.resolved[:, :3].astype(np.uint64).sum(axis=0)
    want = [hits * int(math.floor(float(np.float32(x)) * 1024.0 + 0.5)) for x in c]
    assert failed == 0 and list(sums) == want, (list(sums), want)
    assert int((hc.resolved[:, 3] & 0xFFFF).sum()) > hits, "the later vertices are inserted too, with radiance 0"
    hc.call_ex(cam, gs, stages=UPDATE | RESOLVE, reset_history=True, **st)
    assert not hc.resolved[:, :3].any(), "without DI a black scene's cache holds no radiance"
    # query over the empty cache: a hit pixel is its DI, whatever the sample count; a miss is the (black) environment
    for spp in (1, 2, 4):
        gsq = dxrs.types.graphics_settings(W, H, frame_index=4, bounces=6, spp=spp)
        plain, _, _, _ = hc.call_ex(cam, gsq, stages=QUERY, reset_history=True, **st)
        assert not plain[..., :3].any() and (plain[..., 3] == 1.0).all()
        for mode in (0, 1):
            img, bufs, _, _ = hc.call_ex(cam, gsq, di=di, mode=mode, stages=QUERY, reset_history=True, **st)
            lit = img[..., 0] != 0.0
            assert 0.3 * W * H < lit.sum() < W * H
            assert same_bits(img[lit][:, :3], np.broadcast_to(c, (int(lit.sum()), 3))) and not img[~lit][:, :3].any(), (spp, mode)


# ---------------------------------------------------------------------------------------------------- CPU 4: the gate
def test_gate_is_any_di_positive(dxrs, shims, ex_lib, cpu_scene):
    spheres, mats, sd, cam = cpu_scene
    st = dict(capacity=1 << 12, downscale_factor=1)
    zero = (np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32))
    zero[0][..., 3] = 5.0  # (.w is not read)
    one = (zero[0].copy(), zero[1].copy())
    py, px = 20, 17  # a pixel of the ground
    one[1][py, px, 1] = 0.75
    for mode in (0, 1, 2, 3):
        res = {}
        for name, di in (("none", None), ("zero", zero), ("one", one)):
            hc = HostCacheEx(ex_lib, *shims, spheres, mats, sd)
            gs = dxrs.types.graphics_settings(W, H, frame_index=2, bounces=6, spp=2)
            img, bufs, rays, failed = hc.call_ex(cam, gs, di=di, mode=mode, reset_history=True, **st)
            assert failed == 0
            res[name] = (img, bufs, rays, hc.content())
        a, b, o = res["none"], res["zero"], res["one"]
        assert same_bits(a[0], b[0]) and a[2] == b[2] and a[3] == b[3], f"mode {mode}: DI = 0 everywhere is no DI"
        assert all(same_bits(a[1][k], b[1][k]) for k in a[1])
        changed = {k for k in set(a[3]) | set(o[3]) if a[3].get(k) != o[3].get(k)}
        assert 1 <= len(changed) <= 12, f"mode {mode}: {len(changed)} voxels differ: only those the texel's update path touches may"
        diff = (bits(a[0]) != bits(o[0])).any(axis=-1)
        if mode < 2:
            assert diff[py, px] and a[0][py, px, 0] != 0.0, "the pixel's own DI"
        # (elsewhere the query may differ only through the changed voxels, which is why the cache is compared first; with the cache
        # untouched by the query's own reads, pixels differ only where a path read a changed voxel)
        off, _, _, _ = HostCacheEx(ex_lib, *shims, spheres, mats, sd).call_ex(cam, dxrs.types.graphics_settings(W, H, frame_index=2, bounces=6, spp=2), di=one, mode=mode,
                                                                               stages=QUERY, reset_history=True, **st)
        ref_off, _, _, _ = HostCacheEx(ex_lib, *shims, spheres, mats, sd).call_ex(cam, dxrs.types.graphics_settings(W, H, frame_index=2, bounces=6, spp=2), mode=mode,
                                                                                   stages=QUERY, reset_history=True, **st)
        d2 = (bits(off) != bits(ref_off)).any(axis=-1)
        assert d2.sum() == (1 if mode < 2 else 0) and (mode >= 2 or d2[py, px]), f"mode {mode}: over an empty cache only that pixel differs"


# ---------------------------------------------------------------------------------------------------- CPU 5: the NRD rule
@pytest.mark.parametrize("mode", [2, 3])
def test_nrd_query_does_not_read_di(dxrs, shims, ex_lib, cpu_scene, mode):
    spheres, mats, sd, cam = cpu_scene
    st = dict(capacity=1 << 12, downscale_factor=1)
    di = random_di(W, H, 5)
    gs = dxrs.types.graphics_settings(W, H, frame_index=1, bounces=6, spp=1)
    with_di, without = HostCacheEx(ex_lib, *shims, spheres, mats, sd), HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    with_di.call_ex(cam, gs, di=di, mode=mode, stages=UPDATE | RESOLVE, reset_history=True, **st)
    without.call_ex(cam, gs, mode=mode, stages=UPDATE | RESOLVE, reset_history=True, **st)
    assert with_di.content() != without.content(), "the update takes the DI in every mode"
    keys, voxels = with_di.keys.copy(), with_di.resolved.copy()
    a = with_di.call_ex(cam, gs, di=di, mode=mode, stages=QUERY, **st)
    without.install(keys, voxels)
    b = without.call_ex(cam, gs, mode=mode, stages=QUERY, **st)
    assert same_bits(a[0], b[0]) and all(same_bits(a[1][k], b[1][k]) for k in ("Diffuse", "Specular")) and a[2] == b[2]
    with_di.install(keys, voxels)
    c = with_di.call_ex(cam, gs, di=di, mode=mode, alias=True, stages=QUERY, **st)
    hit = ~is_sentinel(a[1]["Diffuse"][..., 0])
    assert same_bits(c[0], a[0]) and all(same_bits(c[1][k][hit], a[1][k][hit]) for k in ("Diffuse", "Specular")), "aliased outputs"
    assert same_bits(c[1]["Diffuse"][~hit], di[0][~hit]), "a miss leaves the aliased buffer its DI"


# ---------------------------------------------------------------------------------------------------- CPU 6: the outputs' known answers
def test_outputs_known_answers_bounces_0(dxrs, shims, ex_lib, cpu_scene):
    spheres, mats, sd, cam = cpu_scene
    hc = HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    gs = dxrs.types.graphics_settings(W, H, frame_index=0, bounces=0, spp=1)
    img1, b1, _, _ = hc.call_ex(cam, gs, mode=1, reset_history=True, capacity=1 << 12)
    assert is_sentinel(b1["SpecularHitDistance"]).all(), "no bounce-1 ray: nothing is written"
    img2, b2, _, _ = hc.call_ex(cam, gs, mode=2, reset_history=True, capacity=1 << 12)
    hit = ~is_sentinel(b2["Diffuse"][..., 0])
    assert 0.3 * W * H < hit.sum() < W * H
    assert not b2["Diffuse"][hit][:, :3].any() and np.isposinf(b2["Diffuse"][hit][:, 3]).all() and not b2["Specular"][hit].any()
    assert is_sentinel(b2["Specular"][~hit]).all() and same_bits(img2, img1), "out = the primary emission = the whole radiance at Bounces 0"


def test_outputs_known_answers_mirror_sphere(dxrs, host, shims, ex_lib):
    """a Metallic-1, roughness-0 sphere of radius 1 at the origin seen from (0, 0, -6), inside an emissive sphere of radius 100 around the
    origin: every lobe of the small sphere is specular and every reflected ray meets the large one; the centre ray returns along the
    axis, from (0, 0, -1) to (0, 0, -100): 99.  The small sphere's pixels are those whose primary emission (mode 2's out) is 0."""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    w, h = 25, 17
    spheres = np.zeros(2, SPHERE_DTYPE)
    spheres[0], spheres[1] = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 100.0)
    mats = default_material(2)
    mats["Metallic"][0], mats["Roughness"][0] = 1.0, 0.0
    mats["BaseColor"][:, :3] = 0.8
    mats["EmissiveStrength"][:] = 0.0
    mats["EmissiveStrength"][1], mats["EmissiveColor"][1] = 1.0, (1.0, 1.0, 1.0)
    sd = PtSceneData()
    cam = host.camera_matrices(w, h, position=(0.0, 0.0, -6.0), look_at=(0.0, 0.0, 0.0), hfov=math.radians(40), jitter=False)
    hc = HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    gs = dxrs.types.graphics_settings(w, h, frame_index=0, bounces=3, spp=1)
    img, b, _, _ = hc.call_ex(cam, gs, mode=1, reset_history=True, capacity=1 << 12)
    shd = b["SpecularHitDistance"][..., 0]
    prim, b2, _, _ = hc.call_ex(cam, gs, mode=2, reset_history=True, capacity=1 << 12)
    assert not is_sentinel(b2["Diffuse"]).any(), "every primary ray hits a sphere"
    small = prim[..., 0] == 0.0
    assert 10 < small.sum() < w * h // 2 and small[h // 2, w // 2]
    assert not is_sentinel(shd[small]).any(), "written on every pixel of the mirror: its bounce-1 ray hits the large sphere"
    centre = float(shd[h // 2, w // 2])
    print(f"centre SpecularHitDistance {centre!r}")
    assert abs(centre - 99.0) <= 99.0 * 1e-5  # (the tracer's hit tolerance: the spawn offset and fp32 roots)
    assert (shd[small] > 98.9).all() and (shd[small] < 101.0).all()
    assert not b2["Diffuse"][small].any(), "Diffuse.rgb = 0, and .w = 0: the lobe is specular"
    assert same_bits(b2["Specular"][small][:, 3], shd[small]) and (b2["Specular"][small][:, :3] > 0).all()
    big = ~small
    written = ~is_sentinel(shd[big])
    assert same_bits(shd[big][written], b2["Specular"][big][written][:, 3]) and not b2["Diffuse"][big][written][:, 3].any()
    assert (b2["Diffuse"][big][~written][:, 3] > 0).all(), "a diffuse first bounce carries its hit distance in Diffuse.w and writes no SpecularHitDistance"


# ---------------------------------------------------------------------------------------------------- the bounce-1 emission: known answers
def emitter_shell_scene(dxrs, inner):
    """a sphere of radius 1 at the origin (`inner` sets its material) inside an emissive shell of radius 100 (emission (1, 1, 1)), black
    environment: whatever leaves the inner sphere meets the emitter next"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(2, SPHERE_DTYPE)
    spheres[0], spheres[1] = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 100.0)
    mats = default_material(2)
    mats["BaseColor"][:, :3] = 0.8
    mats["EmissiveStrength"][:] = 0.0
    mats["EmissiveStrength"][1], mats["EmissiveColor"][1] = 1.0, (1.0, 1.0, 1.0)
    for k, v in inner.items():
        mats[k][0] = v
    sd = PtSceneData()
    sd.EnvironmentLightColor[0] = sd.EnvironmentLightColor[1] = sd.EnvironmentLightColor[2] = 0.0
    return spheres, mats, sd


def test_bounce_1_emission_known_answers(dxrs, host, shims, ex_lib):
    """Bounces = 1, DI = c > 0 on every texel, every primary ray on the inner sphere, whose own emission is 0.
    A mirror seen from outside: no lobe is the transmission lobe, so the emitter at bounce 1 is dropped -- the query's pixel is c exactly
    (without DI it is the reflected emitter), and the update's cache holds (paths) x round(c * 1024) per channel and nothing else.
    Glass seen from its centre: a sample that leaves through the transmission lobe meets the emitter at bounce 1 and keeps it -- the
    pixel is fl(c + the pixel without DI), bit for bit, whichever lobe the sample took (a reflected sample meets the glass again: 0) --
    and the update's cache holds the emitter's radiance beside the DI."""
    w, h = 24, 16
    di = constant_di(w, h)
    c = di[0][0, 0, :3] + di[1][0, 0, :3]
    q = [int(math.floor(float(np.float32(x)) * 1024.0 + 0.5)) for x in c]
    st = dict(capacity=1 << 12, downscale_factor=1)
    gs = dxrs.types.graphics_settings(w, h, frame_index=3, bounces=1, spp=1)
    views = {"mirror": (dict(Metallic=1.0, Roughness=0.0), host.camera_matrices(w, h, position=(0.0, 0.0, -6.0), look_at=(0.0, 0.0, 0.0), hfov=math.radians(10), jitter=False)),
             "glass": (dict(Transmission=1.0, Roughness=0.0, IOR=1.5), host.camera_matrices(w, h, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 1.0), hfov=math.radians(40), jitter=False))}
    for name, (inner, cam) in views.items():
        hc = HostCacheEx(ex_lib, *shims, *emitter_shell_scene(dxrs, inner))
        prim, b2, _, _ = hc.call_ex(cam, gs, mode=2, stages=QUERY, reset_history=True, **st)
        assert not is_sentinel(b2["Diffuse"]).any() and not prim[..., :3].any(), f"{name}: every primary ray is on the inner sphere, which emits nothing"
        for mode in (0, 1):
            plain, _, _, _ = hc.call_ex(cam, gs, mode=mode, stages=QUERY, reset_history=True, **st)
            lit, _, _, _ = hc.call_ex(cam, gs, di=di, mode=mode, stages=QUERY, reset_history=True, **st)
            if name == "mirror":
                assert (plain[..., :3] > 0).all(), "without DI the pixel is the reflected emitter"
                assert same_bits(lit[..., :3], np.broadcast_to(c, (h, w, 3))), "with DI the emitter at bounce 1 is dropped"
            else:
                through = plain[..., 0] > 0
                print(f"glass, mode {mode}: {int(through.sum())} of {w * h} samples left through the transmission lobe")
                assert through.sum() > w * h // 2 and (plain[through][:, :3] > 0.5).all()
                assert same_bits(lit[..., :3], c + plain[..., :3]), "a sample through the transmission lobe keeps the emitter at bounce 1"
        _, _, _, failed = hc.call_ex(cam, gs, di=di, stages=UPDATE | RESOLVE, reset_history=True, **st)
        sums = [int(x) for x in hc.resolved[:, :3].astype(np.uint64).sum(axis=0)]
        assert failed == 0
        if name == "mirror":
            assert sums == [w * h * x for x in q], (sums, q)
        else:
            # (a path through the transmission lobe adds the emitter's 1.0 = 1024 to the emitter's voxel, and its share to the first vertex)
            assert all(s >= w * h * x + 1024 * (w * h // 2) for s, x in zip(sums, q)), (sums, q)


def test_culled_trace_is_the_brute_force_trace(dxrs, host, ex_lib):
    """the cull in front of the host's closest-hit test drops no sphere the test would accept: 400 rays into 32,800 spheres, from outside
    the field and from inside it, give the same t and id with and without it"""
    spheres, mats, _ = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=32800)
    assert len(spheres) >= 32768
    rng = np.random.default_rng(7)
    n = 400
    xyzr = np.ascontiguousarray(spheres).view(np.float32).reshape(-1, 4)
    centres, radii = xyzr[:, :3], xyzr[:, 3]
    pick = rng.integers(0, len(spheres), n)
    o = np.zeros((n, 3), np.float32)
    o[: n // 2] = (0.0, 3.0, -15.0)
    o[n // 2:] = centres[pick[n // 2:]] + rng.normal(size=(n - n // 2, 3)) * 3.0 * radii[pick[n // 2:], None]
    target = centres[pick] + rng.normal(size=(n, 3)) * 0.6 * radii[pick, None]  # (around a sphere: hits, grazing rays and near misses)
    d = target - o
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    o = np.ascontiguousarray(o)
    tp, tc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    ip, ic = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ex_lib.sh_host_trace_both(p(np.ascontiguousarray(spheres)), p(np.ascontiguousarray(mats)), len(spheres), p(o), p(d), n, p(tp), p(ip), p(tc), p(ic))
    assert np.array_equal(ip, ic) and same_bits(tp, tc)
    hit = ip != 0xFFFFFFFF
    assert n // 4 < hit.sum() < n and len(np.unique(ip)) > n // 8, "the rays must hit, miss, and meet many different spheres"


# ---------------------------------------------------------------------------------------------------- CPU 7: the guide signals
def test_guide_signals_do_not_depend_on_the_cache(dxrs, shims, ex_lib, cpu_scene):
    spheres, mats, sd, cam = cpu_scene
    st = dict(capacity=1 << 12, downscale_factor=1, scene_scale=5.0)
    hc = HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    gs = dxrs.types.graphics_settings(W, H, frame_index=9, bounces=8, spp=2)
    empty = {m: hc.call_ex(cam, gs, mode=m, stages=QUERY, reset_history=True, **st) for m in (1, 2)}
    for f in range(4):
        hc.call_ex(cam, dxrs.types.graphics_settings(W, H, frame_index=f, bounces=8, spp=1), stages=UPDATE | RESOLVE, reset_history=f == 0, **st)
    warm = {m: hc.call_ex(cam, gs, mode=m, stages=QUERY, **st) for m in (1, 2)}
    assert warm[1][2] < empty[1][2] and not same_bits(warm[1][0], empty[1][0]), "the warm cache ends paths"
    assert same_bits(warm[1][1]["SpecularHitDistance"], empty[1][1]["SpecularHitDistance"])
    assert (~is_sentinel(warm[1][1]["SpecularHitDistance"])).sum() > 20
    for k in ("Diffuse", "Specular"):
        assert same_bits(warm[2][1][k][..., 3], empty[2][1][k][..., 3]), k
    assert not same_bits(warm[2][1]["Diffuse"][..., :3], empty[2][1]["Diffuse"][..., :3])


# ---------------------------------------------------------------------------------------------------- CPU 8: no double counting
K_FRAMES = 512


def test_direct_light_is_counted_once(dxrs, host, oracle, shims, ex_lib, restir_shims):  # noqa: F811
    """The 24 x 16 view of test_restir_pass.statistics, cache off (a query over an empty cache), DI = the quadrature of the direct light
    per surface (0 where the reservoir pass has no surface record): deterministic, so the noise is the path tracer's.  Image totals
    (luminance) of K = 512 frames at 1 spp with DI in mode 0 against the same frames without DI: the mean of the per-frame differences
    within 5 of its standard errors; the no-DI run's halves first.  Observed on the CPU: the no-DI halves (totals 106.81 / 106.53) differ by
    0.21 of their standard error; with DI 106.957, without 106.671: +0.286, 0.44 of the paired difference's standard error 0.644."""
    w, h = 24, 16
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gb, _ = cpu_gbuffer(restir_shims, oracle, cam, w, h, spheres, mats, sd)
    scene = rref.Scene(spheres, mats)
    dd, ds = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    for i in range(w * h):
        s = rref.surface(gb, i, tuple(cam.Position))
        if s is not None:
            dd[i // w, i % w, :3] = rref.quadrature(scene, s, k=8)  # (the whole estimate in Diffuse: only the sum is read)
    assert (dd[..., :3].sum(axis=-1) > 0).sum() > w * h // 3
    hc = HostCacheEx(ex_lib, *shims, spheres, mats, sd)
    lum = np.array([0.2126, 0.7152, 0.0722])
    with_di, without = np.zeros(K_FRAMES), np.zeros(K_FRAMES)
    for f in range(K_FRAMES):
        gs = dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1)
        a, _, _, _ = hc.call_ex(cam, gs, di=(dd, ds), stages=QUERY, reset_history=True, capacity=16)
        b, _, _, _ = hc.call_ex(cam, gs, stages=QUERY, reset_history=True, capacity=16)
        with_di[f], without[f] = (a[..., :3].astype(np.float64) @ lum).sum(), (b[..., :3].astype(np.float64) @ lum).sum()
    half = K_FRAMES // 2
    x, y = without[:half], without[half:]
    se_xy = math.sqrt(x.var(ddof=1) / len(x) + y.var(ddof=1) / len(y))
    print(f"no DI: halves {x.mean():.4f} / {y.mean():.4f}, difference {abs(x.mean() - y.mean()) / se_xy:.2f} standard errors")
    assert abs(x.mean() - y.mean()) <= 5 * se_xy, "the path tracer alone is not stable under the bound"
    d = with_di - without
    se = d.std(ddof=1) / math.sqrt(K_FRAMES)
    print(f"with DI {with_di.mean():.4f}, without {without.mean():.4f}: difference {d.mean():+.4f}, standard error {se:.4f} ({abs(d.mean()) / se:.2f})")
    assert abs(d.mean()) <= 5 * se
    assert with_di.std() < without.std(), "the deterministic DI replaces the noisiest term"


# ---------------------------------------------------------------------------------------------------- CPU 9: sanitizers
def test_sanitized_stand_alone_program(tmp_path):
    """update, resolve and query with a DI (zeros, a NaN, an inf, a negative texel) in the modes 0..3 and with aliased NRD outputs, three
    frames each, under ASan + UBSan, in a child process (nothing sanitised is loaded into Python)"""
    exe = str(tmp_path / "sharc_ex_sanitize")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-o", exe, "sharc_ex_sanitize.cpp"], cwd=os.path.join(HERE, "hostshim"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout


# ---------------------------------------------------------------------------------------------------- GPU
def gpu_call(r, di=None, mode=0, rect=None, alias=False, **st):
    """-> (image or None, {output: array}, rays); image and outputs start as the sentinel"""
    img, bufs, s = r.render_sharc_ex(di[0] if di is not None else None, di[1] if di is not None else None, rect=rect, mode=mode, fill=SENTINEL, alias=alias, **st)
    return img, bufs, int(s.rays)


@pytest.mark.gpu
def test_gpu_extras_off_equals_pt_render_sharc(dxrs, host, renderer):
    spheres, mats, sd, cam = c1(dxrs, host)
    runs = []
    for ex in (False, True):
        frames = []
        for f in range(3):
            gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1)
            if f == 0:
                setup(renderer, dxrs, spheres, mats, sd, cam, gs)
            renderer.set_constants(gs)
            st = defaults(reset_history=f == 0)
            if ex:
                img, bufs, rays = gpu_call(renderer, **st)
                assert not bufs
            else:
                img, s = renderer.render_sharc(**st)
                rays = int(s.rays)
            frames.append((img, rays, gpu_content(renderer)))
        runs.append(frames)
    for f in range(3):
        a, b = runs[0][f], runs[1][f]
        assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and len(a[2]) > 100, f"frame {f}"


@pytest.mark.gpu
@pytest.mark.parametrize("spp,rect", [(1, None), (3, None), (1, (5, 3, 67, 45))])
def test_gpu_empty_cache_equals_pt_render_denoiser(dxrs, host, renderer, spp, rect):
    """modes 1 / 2 / 3 without DI, and modes 2 / 3 with a DI the query must not read: out and every buffer, untouched sentinels included"""
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=3, bounces=8, spp=spp)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    rw, rh = (rect[2], rect[3]) if rect else (GW, GH)
    di = random_di(rw, rh, 11)
    for mode in (1, 2, 3):
        want, wb = renderer.render_denoiser(mode, rect=rect, fill=SENTINEL)
        for with_di in ((False, True) if mode >= 2 else (False,)):
            got, gb, _ = gpu_call(renderer, di=di if with_di else None, mode=mode, rect=rect, **defaults(stages=QUERY, reset_history=True))
            assert same_bits(got, want), (mode, with_di)
            for k in wb:
                assert same_bits(gb[k], wb[k]), (mode, with_di, k)
                assert is_sentinel(wb[k]).any() and not is_sentinel(wb[k]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 3])
def test_gpu_empty_cache_with_di_against_pt_render_with_di(dxrs, host, renderer, spp):
    """DI > 0 on every pixel, so the two gates agree.  pt_render_with_di: (sum of spp samples) * inv_spp + DI; here: the sum of spp
    (DI + sample) terms * inv_spp.  The terms are non-negative, so each differing rounding moves the result by at most 2^-23 of it:
    per sample the additions of its up to Bounces + 1 vertex terms associate differently once DI stands in front (Bounces + 2
    roundings), and the sum over the samples, the product and pt_render_with_di's final addition make 3 more."""
    import torch
    bounces = 8
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=3, bounces=bounces, spp=spp)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    di = random_di(GW, GH, 12)
    n = spp * (bounces + 2) + 3
    worst = 0.0
    for mode in (0, 1):
        res = renderer.render_with_di(di[0], di[1], mode=mode, fill=SENTINEL)
        want, wb = (res, {}) if mode == 0 else res
        dev = torch.device("cuda", 0)
        out = torch.zeros((GH, GW, 4), device=dev)
        dd, ds = (torch.from_numpy(a).to(dev) for a in di)
        shd = torch.zeros((GH, GW, 1), device=dev)
        torch.cuda.synchronize(dev)
        ws = renderer.render_with_di_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, mode, {"SpecularHitDistance": shd.data_ptr()}, want_stats=True)
        got, gb, rays = gpu_call(renderer, di=di, mode=mode, **defaults(stages=QUERY, reset_history=True))
        assert rays == int(ws.rays), (mode, rays, ws.rays)
        a, b = got[..., :3].astype(np.float64), want[..., :3].astype(np.float64)
        assert (a >= 0).all() and (b >= 0).all() and np.isfinite(a).all()
        bound = n * 2.0 ** -23 * np.maximum(a, b)
        frac = np.abs(a - b) / np.where(bound > 0, bound, 1.0)
        worst = max(worst, float(frac.max()))
        print(f"spp {spp} mode {mode}: largest |a - b| is {frac.max():.3f} of the bound (n = {n})")
        assert (np.abs(a - b) <= bound).all(), f"mode {mode}: {frac.max():.3f} of the bound"
        assert same_bits(got[..., 3], want[..., 3])
        if mode == 1:
            assert same_bits(gb["SpecularHitDistance"], wb["SpecularHitDistance"])
    print(f"spp {spp}: worst {worst:.3f} of the bound")


@pytest.mark.gpu
def test_gpu_zero_di_equals_pt_render_sharc(dxrs, host, renderer):
    spheres, mats, sd, cam = c1(dxrs, host)
    zero = (np.zeros((GH, GW, 4), np.float32), np.zeros((GH, GW, 4), np.float32))
    res = []
    for ex in (False, True):
        for f in range(2):
            gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=2)
            if f == 0:
                setup(renderer, dxrs, spheres, mats, sd, cam, gs)
            renderer.set_constants(gs)
            st = defaults(reset_history=f == 0)
            if ex:
                img, _, rays = gpu_call(renderer, di=zero, **st)
            else:
                img, s = renderer.render_sharc(**st)
                rays = int(s.rays)
        res.append((img, rays, gpu_content(renderer)))
    assert same_bits(res[0][0], res[1][0]) and res[0][1] == res[1][1] and res[0][2] == res[1][2]


def ex_frames_against_host(dxrs, r, hc, spheres, mats, sd, cams, modes=(0, 1, 2, 3), textures=None, bounces=8, zero_fraction=0.2, size=(GW, GH), **kw):
    """consecutive pt_render_sharc_ex calls with a random DI (positive, a fifth of the texels 0) against the host header, per mode: the
    cache as a map after each call, the image, the outputs and the ray count"""
    width, height = size
    for mode in modes:
        for f, cam in enumerate(cams):
            gs = dxrs.types.graphics_settings(width, height, frame_index=f, bounces=bounces, spp=2 if f == 1 else 1)
            if f == 0:
                setup(r, dxrs, spheres, mats, sd, cam, gs, textures)
            r.set_camera(cam)
            r.set_constants(gs)
            di = random_di(width, height, 100 + 10 * mode + f, zero_fraction)
            st = defaults(reset_history=f == 0, **kw)
            got, gb, rays = gpu_call(r, di=di, mode=mode, **st)
            want, wb, wrays, failed = hc.call_ex(cam, gs, di=di, mode=mode, **st)
            assert failed == 0, "the capacity must be chosen so that the host run has no failed insert"
            g, h = gpu_content(r, st["capacity"]), hc.content()
            assert set(g) == set(h), f"mode {mode} frame {f}: {len(set(g) ^ set(h))} keys differ"
            bad = [k for k in g if g[k] != h[k]]
            assert not bad, f"mode {mode} frame {f}: {len(bad)} of {len(g)} voxels differ"
            assert len(g) > 100
            assert same_bits(got, want), f"mode {mode} frame {f}: {int((bits(got) != bits(want)).any(axis=-1).sum())} pixels differ from the host header"
            for k in wb:
                assert same_bits(gb[k], wb[k]), (mode, f, k)
                assert not is_sentinel(wb[k]).all()
            assert rays == wrays, (mode, f, rays, wrays)


@pytest.mark.gpu
def test_gpu_equals_the_host_header(dxrs, host, renderer, shims, ex_lib):
    spheres, mats, sd, cam = c1(dxrs, host)
    moved = host.camera_matrices(GW, GH, position=(1.5, 0.5, -14.0), look_at=(0.0, 0.0, 0.0), previous=cam)
    ex_frames_against_host(dxrs, renderer, HostCacheEx(ex_lib, *shims, spheres, mats, sd), spheres, mats, sd, [cam, cam, moved])


@pytest.mark.gpu
def test_gpu_equals_the_host_header_scene_in_global_memory(dxrs, host, shims, ex_lib):
    spheres, mats, sd, cam = c1(dxrs, host)
    moved = host.camera_matrices(GW, GH, position=(1.5, 0.5, -14.0), look_at=(0.0, 0.0, 0.0), previous=cam)
    r = dxrs.Renderer(device=0, flags=dxrs.types.PT_FLAG_NO_LDS_SCENE)
    try:
        ex_frames_against_host(dxrs, r, HostCacheEx(ex_lib, *shims, spheres, mats, sd), spheres, mats, sd, [cam, cam, moved])
        assert not r.accel.lds_resident
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_equals_the_host_header_textured_alpha_scene(dxrs, host, renderer, shims, ex_lib):
    import golden_cases
    case = next(c for c in golden_cases.cases(dxrs, host) if c["file"].startswith("a5_alpha"))
    cam = host.camera_matrices(GW, GH, position=(0.0, 2.0, -7.0), jitter_index=1)
    moved = host.camera_matrices(GW, GH, position=(0.6, 2.3, -6.5), jitter_index=2, previous=cam)
    hc = HostCacheEx(ex_lib, *shims, case["spheres"], case["materials"], case["sd"], textures=case["textures"])
    try:
        ex_frames_against_host(dxrs, renderer, hc, case["spheres"], case["materials"], case["sd"], [cam, cam, moved], textures=case["textures"], bounces=5)
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gpu_equals_the_host_header_tree_with_32_bit_stack(dxrs, host, shims, ex_lib, mode):
    """32,800 spheres, the fewest round number whose tree (n - 1 nodes) takes the 32-bit stack (from 32767 nodes): the same comparison.
    The host's trace culls before its exact test (sharc_ex_host.h) to keep so many spheres quick."""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=32800)
    cam = host.camera_matrices(GW, GH)
    moved = host.camera_matrices(GW, GH, position=(1.5, 0.5, -14.0), look_at=(0.0, 0.0, 0.0), previous=cam)
    r = dxrs.Renderer(device=0)
    try:
        ex_frames_against_host(dxrs, r, HostCacheEx(ex_lib, *shims, spheres, mats, sd), spheres, mats, sd, [cam, cam, moved], modes=(mode,))
        assert r.accel.node_count >= 32767 and not r.accel.lds_resident
    finally:
        r.close()


def chain(dxrs, host, sync):
    """two frames of gbuffer -> restir_di_ex -> sharc_ex(DI, mode 1, the NRD outputs named as the DI buffers) -> ray reconstruction on a
    context with three lanes; sync: a device synchronise after every call"""
    import torch
    from dxrs_amd.abi_types import RESTIR_DI_INPUTS
    w, h, Wo, Ho = GW, GH, 2 * GW, 2 * GH
    spheres, mats, sd = make_scene(dxrs)
    dev = torch.device("cuda", 0)
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        width = dict(dxrs.abi_types.GBUFFER_CHANNELS)
        names = set(RESTIR_DI_INPUTS) | {"DiffuseAlbedo", "SpecularAlbedo"}
        gb = {n: torch.zeros((h, w, width[n]), device=dev) for n in names}
        dd, ds, color = (torch.zeros((h, w, 4), device=dev) for _ in range(3))
        shd = torch.zeros((h, w, 1), device=dev)
        output = torch.zeros((Ho, Wo, 4), device=dev)
        torch.cuda.synchronize(dev)
        r.set_scene(spheres, mats, sd)
        prev, results = None, []
        wait = r.synchronize if sync else (lambda: None)
        for f in range(2):
            cam = host.camera_matrices(w, h, position=(0.1 * f, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter_index=f, jitter_count=32, previous=prev)
            prev = cam
            r.set_camera(cam)
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=6, spp=1))
            ptrs = {n: b.data_ptr() for n, b in gb.items()}
            r.render_gbuffer_device(ptrs)
            wait()
            r.restir_di_device(w, h, dict({n: ptrs[n] for n in RESTIR_DI_INPUTS}, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), frame_index=f, reset_history=f == 0,
                               candidates=dict(brdf_samples=1, boiling_filter=0.2))
            wait()
            r.render_sharc_ex_device(color.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, 1,
                                     dict(SpecularHitDistance=shd.data_ptr(), Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), **defaults(reset_history=f == 0))
            wait()
            r.ray_reconstruction_device((w, h), (Wo, Ho), dict(Color=color.data_ptr(), Depth=gb["LinearDepth"].data_ptr(), MotionVector=gb["MotionVector"].data_ptr(),
                                                               NormalRoughness=gb["NormalRoughness"].data_ptr(), DiffuseAlbedo=gb["DiffuseAlbedo"].data_ptr(),
                                                               SpecularAlbedo=gb["SpecularAlbedo"].data_ptr(), SpecularHitDistance=shd.data_ptr(), Output=output.data_ptr()),
                                        cam, reset=f == 0)
            wait()
            r.synchronize()  # (the frame's results are read back, and the next frame's passes overwrite the buffers from the lane)
            results.append([t.cpu().numpy().copy() for t in (dd, ds, color, shd, output)])
            shd.zero_()
            dd.zero_()
            ds.zero_()
            torch.cuda.synchronize(dev)
        return results, cache_map(*r.sharc_download(CAP))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_default_frame_chain_queued_equals_synchronised(dxrs, host):
    queued, cq = chain(dxrs, host, False)
    synced, cs = chain(dxrs, host, True)
    assert cq == cs and len(cq) > 100
    for f in range(2):
        for name, a, b in zip(("Diffuse", "Specular", "Color", "SpecularHitDistance", "Output"), queued[f], synced[f]):
            assert same_bits(a, b), f"frame {f}: {name} differs"
        dd, ds, color, shd, output = queued[f]
        assert (dd[..., :3] > 0).any() and (shd > 0).any() and np.isfinite(output).all() and output[..., :3].max() > 0
        assert np.isfinite(color).all()


@pytest.mark.gpu
def test_gpu_argument_errors(dxrs, host, renderer):
    import torch
    from dxrs_amd.abi_types import PtDenoiserOutputs, PtDirectLighting, PtRect, PtSharcSettings
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=4, spp=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    renderer.render_sharc(**defaults(reset_history=True))
    content = gpu_content(renderer)
    dev = torch.device("cuda", 0)
    n = GW * GH
    buf = {k: torch.full((n + 1, 4), 7.0, device=dev) for k in ("out", "dd", "ds", "nd", "ns")}
    shd = torch.full((n + 1,), 7.0, device=dev)
    torch.cuda.synchronize(dev)
    lib, ctx = renderer._lib, renderer._ctx
    ptr = {k: v.data_ptr() for k, v in buf.items()}

    def call(di=None, outputs=None, rect=None, stages=7, out=ptr["out"]):
        s = PtSharcSettings(Capacity=CAP, DownscaleFactor=2, Stages=stages)
        d = PtDirectLighting(Diffuse=C.c_void_p(di[0]), Specular=C.c_void_p(di[1])) if di else None
        o = PtDenoiserOutputs(Denoiser=outputs[0], **{k: C.c_void_p(v) for k, v in outputs[1].items()}) if outputs else None
        return lib.pt_render_sharc_ex(ctx, C.byref(PtRect(*rect)) if rect else None, C.c_void_p(out), 1, C.byref(s), C.byref(d) if d else None,
                                      C.byref(o) if o else None, None)

    good_di = (ptr["dd"], ptr["ds"])
    cases = [("null DI buffer", dict(di=(0, ptr["ds"]))), ("null DI buffer", dict(di=(ptr["dd"], 0))), ("misaligned DI", dict(di=(ptr["dd"] + 4, ptr["ds"]))),
             ("misaligned DI", dict(di=(ptr["dd"], ptr["ds"] + 8))), ("mode 0 in outputs", dict(outputs=(0, {}))), ("mode 4", dict(outputs=(4, {}))),
             ("mode 1 without its buffer", dict(outputs=(1, {}))), ("mode 1 misaligned", dict(outputs=(1, dict(SpecularHitDistance=shd.data_ptr() + 2)))),
             ("mode 2 without Specular", dict(outputs=(2, dict(Diffuse=ptr["nd"])))), ("mode 3 misaligned", dict(outputs=(3, dict(Diffuse=ptr["nd"] + 4, Specular=ptr["ns"])))),
             ("Diffuse is out", dict(outputs=(2, dict(Diffuse=ptr["out"], Specular=ptr["ns"])))),
             ("Diffuse overlaps Specular", dict(outputs=(2, dict(Diffuse=ptr["nd"], Specular=ptr["nd"] + 16)))),
             ("DI is out", dict(di=(ptr["out"], ptr["ds"]))), ("DI is out", dict(di=(ptr["dd"], ptr["out"]), outputs=(2, dict(Diffuse=ptr["nd"], Specular=ptr["ns"])))),
             ("DI overlaps SpecularHitDistance", dict(di=(shd.data_ptr(), ptr["ds"]), outputs=(1, dict(SpecularHitDistance=shd.data_ptr())))),
             ("DI overlaps Diffuse without being it", dict(di=(ptr["nd"] + 16, ptr["ds"]), outputs=(3, dict(Diffuse=ptr["nd"], Specular=ptr["ns"])))),
             ("DI + UPDATE with a partial rect", dict(di=good_di, rect=(0, 0, GW, GH - 1))), ("DI + UPDATE with a partial rect", dict(di=good_di, rect=(8, 0, GW - 8, GH), stages=UPDATE)),
             ("misaligned out", dict(di=good_di, out=ptr["out"] + 4)), ("null out", dict(di=good_di, out=0))]
    for what, kw in cases:
        assert call(**kw) == 1, what
        assert lib.pt_last_error(ctx)
    renderer.synchronize()
    for k, v in buf.items():
        assert (v == 7.0).all(), f"a refused call wrote {k}"
    assert (shd == 7.0).all() and gpu_content(renderer) == content, "a refused call touched the cache"
    # what must be accepted: a QUERY-only call with a partial rect and rect-sized DI; DI with the whole frame named as the rect; the NRD
    # outputs in the DI's buffers; IsDIEnabled in the constants (ignored)
    assert call(di=good_di, rect=(8, 4, GW - 8, GH - 4), stages=QUERY) == 0
    assert call(di=good_di, rect=(0, 0, GW, GH)) == 0
    assert call(di=good_di, outputs=(2, dict(Diffuse=ptr["dd"], Specular=ptr["ds"]))) == 0
    renderer.set_constants(dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=4, spp=1, di=True))
    assert call(di=good_di, outputs=(1, dict(SpecularHitDistance=shd.data_ptr()))) == 0
    s = PtSharcSettings(Capacity=CAP, DownscaleFactor=2, Stages=QUERY)
    assert lib.pt_render_sharc(ctx, None, C.c_void_p(ptr["out"]), 1, C.byref(s), None) == 5, "pt_render_sharc keeps refusing IsDIEnabled"
    renderer.set_constants(gs)
    renderer.synchronize()
    assert (buf["out"][n:] == 7.0).all() and (buf["dd"][n:] == 7.0).all() and (shd[n:] == 7.0).all(), "nothing is written past the frame"
    want, _ = renderer.render()
    got, _, _ = gpu_call(renderer, **defaults(stages=QUERY, reset_history=True))
    assert same_bits(got, want), "the context renders a correct frame after the refusals"


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """Raytracing::Render(radiance, SHARC&, SHARCSettings, const DirectLighting*, DenoiserBuffers*) (host/Raytracing.hpp) from C++: a
    ReBLUR frame's Diffuse / Specular as the DI of two DLSS-RR frames through the cache give the binding's frame bit for bit"""
    import torch
    pkg = os.path.join(os.path.dirname(HERE), "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_sharc_ex")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_sharc_ex.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 160, 90
    outp = str(tmp_path / "sharc_ex.f32")
    res = subprocess.run([exe, str(w), str(h), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(outp, dtype=np.float32)
    radiance, shd_cpp = raw[:w * h * 4].reshape(h, w, 4), raw[w * h * 4:].reshape(h, w)
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0)
    try:
        gs = dxrs.types.graphics_settings(w, h, frame_index=0, bounces=8, spp=1)
        r.set_scene(spheres, mats, sd)
        r.set_camera(host.camera(w, h, jitter=False))
        r.set_constants(gs)
        dev = torch.device("cuda", 0)
        nd, ns, tmp, out = (torch.zeros((h, w, 4), device=dev) for _ in range(4))
        shd = torch.zeros((h, w), device=dev)
        torch.cuda.synchronize(dev)
        r.render_denoiser_device(2, tmp.data_ptr(), {"Diffuse": nd.data_ptr(), "Specular": ns.data_ptr()})
        for f in range(2):
            r.render_sharc_ex_device(out.data_ptr(), nd.data_ptr(), ns.data_ptr(), None, 1, {"SpecularHitDistance": shd.data_ptr()}, capacity=1 << 18,
                                     downscale_factor=4, scene_scale=50.0, roughness_threshold=0.4, accumulation_frames=10, max_stale_frames=64, reset_history=f == 0)
        r.synchronize()
        assert (nd.cpu().numpy()[..., :3] > 0).any() and (shd.cpu().numpy() > 0).any()
        wrote = shd.cpu().numpy() > 0  # (the C++ program's buffer is not cleared: compared where the frames write)
        assert same_bits(radiance, out.cpu().numpy()) and same_bits(shd_cpp[wrote], shd.cpu().numpy()[wrote]), "C++ mirror == Python path"
    finally:
        r.close()
