"""Row N26 -- pt_render_lens, the pure path-traced frame through the thin-lens camera (DESIGN.md spec S29).
CPU: the host-compiled header (tests/hostshim/lens_host.cpp over csrc/pt_lens.h) against the float64 restatement (lens_reference.py): the
lens rays inside a counted rounding bound, with their geometric facts; aperture 0 as pt_render's loop; the lens stream's independence of
the bounce generator; the circle of confusion of a small emitter in and out of focus; the all-miss frame; the argument rules that need no
device; a sanitizer build of a stand-alone program.
GPU: aperture 0 against pt_render bit for bit, aperture > 0 against the host-compiled header bit for bit with equal ray counts, over
the tree forms and material variants; consecutive frames, frames in flight, the argument rules, the C++ mirror."""
import copy
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lens_reference as ref
from test_restir_pass import make_scene
from test_sharc import HostCache, p, same_bits, setup

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -24  # the unit roundoff of float32


# ---------------------------------------------------------------------------------------------------- the host-compiled header
@pytest.fixture(scope="module")
def shims():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_lens_shim())
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    for name, res, args in (("lens_host_get_ray", None, [vp, vp, u32, vp]), ("lens_host_rays", None, [vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp]),
                            ("lens_host_stream", None, [u32, u32, u32, u32, vp]),
                            ("lens_host_frame", C.c_uint64, [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, f32, vp, vp]),
                            ("lens_host_primary_hits", u32, [vp, vp, u32, vp, vp])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    sh = C.CDLL(g.build_sharc_shim())
    sh.sh_host_call.restype = None
    sh.sh_host_call.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    gb = C.CDLL(g.build_gbuffer_shim())
    gb.gb_srgb_lut.restype = None
    gb.gb_srgb_lut.argtypes = [vp]
    return lib, sh, gb


def with_lens(cam, aperture, focus=None):
    """a copy of cam with ApertureRadius = aperture; focus: Right, Up and Forward rescaled together so that |Forward| = focus (what
    CameraController::SetFocusDistance does: the pinhole image does not change)"""
    c = copy.copy(cam)
    c.ApertureRadius = aperture
    if focus is not None:
        k = np.float32(focus) / np.float32(math.sqrt(sum(float(x) ** 2 for x in cam.ForwardDirection)))
        for v in (c.RightDirection, c.UpDirection, c.ForwardDirection):
            for i in range(3):
                v[i] = float(np.float32(v[i]) * k)
    return c


class HostLens:
    """pt_render_lens over the host-compiled header; the scene arrays are prepared as test_sharc.HostCache prepares them, and the
    environment map SceneData names (a lat-long texture or six cube faces of the texture table, with its transform) goes with them"""

    def __init__(self, shims, spheres, mats, sd, textures=None):
        self.lib, self.sh = shims[0], shims[1]
        self.hc = HostCache(shims[1], shims[2], spheres, mats, sd, textures)
        self.env_map = np.array([sd.EnvironmentLightTextureDescriptor, sd.IsEnvironmentLightTextureCubeMap], np.uint32)
        self.env_xf = np.array(list(sd.EnvironmentLightTransform), np.float32)

    def scene_args(self):
        hc = self.hc
        return (p(hc.spheres), p(hc.mats), len(hc.spheres), p(hc.env), p(hc.texels), p(hc.info), 0 if hc.info is None else len(hc.info), p(hc.maps), p(hc.rot),
                p(self.env_map), p(self.env_xf))

    def frame(self, cam, gs, rect=None, per_pixel=False):
        """-> (image (h, w, 4), rays[, the rays of each pixel (h, w)])"""
        w, h = gs.RenderSize[0], gs.RenderSize[1]
        rect = rect or (0, 0, w, h)
        prm = np.array([w, h, gs.FrameIndex, gs.Bounces, gs.SamplesPerPixel, gs.IsRussianRouletteEnabled, *rect], np.uint32)
        out = np.zeros((rect[3], rect[2], 4), np.float32)
        pr = np.zeros((rect[3], rect[2]), np.uint32) if per_pixel else None
        rays = self.lib.lens_host_frame(*self.scene_args(), C.addressof(cam), p(prm), gs.ThroughputThreshold, p(out), p(pr))
        return (out, int(rays), pr) if per_pixel else (out, int(rays))

    def query_off(self, cam, gs, rect=None):
        """the host sh_query_pixel with the cache off: pt_render's loop (test_sharc.py pins it to pt_render on the GPU)"""
        return self.hc.call(cam, gs, rect=rect, cache=False)[:2]

    def primary_hits(self, cam, gs, rect=None):
        w, h = gs.RenderSize[0], gs.RenderSize[1]
        prm = np.array([w, h, 0, 0, 1, 0, *(rect or (0, 0, w, h))], np.uint32)
        return int(self.lib.lens_host_primary_hits(p(self.hc.spheres), p(self.hc.mats), len(self.hc.spheres), C.addressof(cam), p(prm)))


# ---------------------------------------------------------------------------------------------------- CPU: ABI and arguments
def test_lens_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_render_lens") and "pt_render_lens" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtCamera
    assert PtCamera.ApertureRadius.offset == 76
    out = np.zeros(4, np.float32)
    assert lib.pt_render_lens(None, None, out.ctypes.data, 0, None) == 1  # PT_ERR_INVALID_ARG: null context
    assert lib.pt_render_lens(None, None, None, 1, None) == 1
    assert hasattr(dxrs.Renderer, "render_lens") and hasattr(dxrs.Renderer, "render_lens_device")


# ---------------------------------------------------------------------------------------------------- CPU: GetRay and the lens stream
def test_get_ray_and_lens_stream(shims):
    lib = shims[0]
    rng = np.random.default_rng(1)
    u1 = np.concatenate([[2.0 ** -23, 0.25, 0.5, 0.75, 1.0], rng.uniform(0, 1, 2000)]).astype(np.float32)
    u2 = np.concatenate([[2.0 ** -23, 0.5, 1.0, 1.0 - 2.0 ** -23, 0.25], rng.uniform(0, 1, 2000)]).astype(np.float32)
    xy = np.zeros((len(u1), 2), np.float32)
    lib.lens_host_get_ray(p(u1), p(u2), len(u1), p(xy))
    worst = 0.0
    for i in range(len(u1)):
        wx, wy = ref.get_ray_xy(u1[i], u2[i])
        bound = v_bound(u2[i])
        worst = max(worst, abs(xy[i, 0] - wx) / bound, abs(xy[i, 1] - wy) / bound)
        assert abs(xy[i, 0] - wx) <= bound and abs(xy[i, 1] - wy) <= bound, (u1[i], u2[i], xy[i], wx, wy)
        assert float(xy[i, 0]) ** 2 + float(xy[i, 1]) ** 2 <= 1.0 + 2.0 * bound, "the lens point lies on the unit disc"
    print(f"GetRay: largest error {worst:.3f} of its bound")
    assert (xy[u2 == 1.0] == 0.0).all(), "z = 1 is the disc's centre"
    # the distribution crowds the rim: E[r^2] = 2/3, E[x^2] = E[y^2] = 1/3 (200,000 pairs: a standard error of 7e-4 on r^2, whose variance is 4/45)
    n = 200000
    a, b = rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    big = np.zeros((n, 2), np.float32)
    lib.lens_host_get_ray(p(a), p(b), n, p(big))
    r2 = (big.astype(np.float64) ** 2).sum(axis=1)
    assert abs(r2.mean() - 2.0 / 3.0) <= 4.0 * math.sqrt(4.0 / 45.0 / n)
    assert abs((big[:, 0].astype(np.float64) ** 2).mean() - 1.0 / 3.0) <= 4.0 * math.sqrt(0.1 / n)  # Var[x^2] = E[r^4] E[cos^4] - 1/9 = (8/15)(3/8) - 1/9 < 0.1
    # the stream: seed and draws as the spec states them, and no number of it is one of the bounce generator's first draws
    for px, py, frame in ((0, 0, 0), (18, 12, 7), (1919, 1079, 123456), (65535, 65535, 0xFFFFFFFF)):
        u = np.zeros(8, np.float32)
        lib.lens_host_stream(px, py, frame, 4, p(u))
        assert [float(x) for x in u] == ref.lens_stream(px, py, frame, 4)
        assert ((u > 0) & (u <= 1)).all()


def v_bound(u2):
    """the bound on a component of GetRay(u).xy against float64.  x = 1 - z^2: the square and the difference round once each, both below 1:
    2 EPS absolute; the square root moves by at most dx / sqrt(x) and rounds once: dr = 2 EPS / r + EPS r (z = 1: x = 0 and r = 0 exactly,
    dr = 0); sincos_2pi is within 5e-7 absolute (spec S1); the product rounds once: dv = dr + 5e-7 r + EPS"""
    r = math.sqrt(max(1.0 - float(u2) ** 2, 0.0))
    dr = 0.0 if r == 0.0 else 2.0 * EPS / r + EPS * r
    return dr + 5e-7 * r + EPS


# ---------------------------------------------------------------------------------------------------- CPU: rays against float64
def norm(v):
    return math.sqrt(float(np.dot(v, v)))


def test_lens_rays_against_float64(host, shims):
    """Origin and direction inside a bound counted from the operations (EPS = 2^-24 per rounding, first order, inputs exact).  With unit
    RightN / UpN from normalize (dot: 3 roundings, sqrt 1 at half weight, rcp 1, product 1: 5 EPS a component) and |v| <= 1:
      offset   each product RightN v.x, UpN v.y: 6 EPS + dv; their sum rounds once, the scaling by A once: d_off = A (14 EPS + 2 dv)
      origin   one more rounding: d_o = d_off + EPS (|Position| + A), a component
      nx, ny   (pixel + 0.5 exact) + Jitter, InvW, their product: 3 EPS relative on u <= 1, the fma once: 7 EPS absolute
      D        two products of nx / ny (7 EPS each) with Right / Up, the fma and the sum with Forward: below 11 EPS S, S = |Right| + |Up| + |Forward|
      D - off  d_x = 12 EPS (S + A) + d_off, a component
      d        normalising a vector moved by sqrt(3) d_x a side turns it by at most that over its length; its own roundings 5 EPS:
               d_d = sqrt(3) d_x / |D - offset| + 5 EPS
    The geometric facts are checked on the header's float32 rays in float64, within the same bounds: |o - Position| <= A, o - Position
    perpendicular to ForwardN, and the ray passes the pinhole ray's point Position + D."""
    lib = shims[0]
    w, h = 19, 13
    cams = []
    for jitter_index, focus, pos, look in ((0, None, (0.0, 0.0, -15.0), None), (3, 9.0, (1.5, 2.5, -9.0), (0.0, 1.0, 0.0)), (5, 0.25, (-300.0, 40.0, 120.0), (10.0, 0.0, 3.0))):
        base = host.camera_matrices(w, h, position=pos, look_at=look, hfov=math.radians(70), jitter=jitter_index != 0, jitter_index=jitter_index)
        for aperture in (1e-3, 0.05, 1.0):
            cams.append(with_lens(base, aperture, focus))
    us = [2.0 ** -23, 0.5, 1.0, 0.3, 0.8125, 1.0 - 2.0 ** -23]
    pixels = [(0, 0), (18, 12), (9, 6), (18, 0), (0, 12), (4, 11)]
    worst_o = worst_d = worst_geo = 0.0
    for cam in cams:
        px, py, u1, u2 = (np.array(a) for a in zip(*[(x, y, a, b) for (x, y) in pixels for a in us for b in us]))
        px, py, u1, u2 = px.astype(np.uint32), py.astype(np.uint32), u1.astype(np.float32), u2.astype(np.float32)
        n = len(px)
        o, d, tt = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
        lib.lens_host_rays(C.addressof(cam), w, h, p(px), p(py), p(u1), p(u2), n, p(o), p(d), p(tt))
        A = float(cam.ApertureRadius)
        P, FN = ref.vec(cam.Position), ref.unit(ref.vec(cam.ForwardDirection))
        S = norm(ref.vec(cam.RightDirection)) + norm(ref.vec(cam.UpDirection)) + norm(ref.vec(cam.ForwardDirection))
        for i in range(n):
            want = ref.lens_ray(cam, w, h, int(px[i]), int(py[i]), u1[i], u2[i])
            dv = v_bound(u2[i])
            d_off = A * (14.0 * EPS + 2.0 * dv)
            d_o = d_off + EPS * (float(np.abs(P).max()) + A)
            d_x = 12.0 * EPS * (S + A) + d_off
            d_d = math.sqrt(3.0) * d_x / want["length"] + 5.0 * EPS
            eo, ed = np.abs(o[i] - want["o"]).max(), np.abs(d[i] - want["d"]).max()
            assert eo <= d_o and ed <= d_d, (A, px[i], py[i], u1[i], u2[i], eo, d_o, ed, d_d)
            worst_o, worst_d = max(worst_o, eo / d_o), max(worst_d, ed / d_d)
            # tmin = Near rcp(dot(ForwardN, d)): the dot moves by sqrt(3) d_d and 8 EPS of its own (ForwardN 5, three roundings); rcp and product 2 EPS
            cos = float(FN @ want["d"])
            assert abs(tt[i, 0] - want["tmin"]) <= want["tmin"] * ((math.sqrt(3.0) * d_d + 8.0 * EPS) / cos + 2.0 * EPS)
            assert tt[i, 1] == np.float32(want["tmax"]) or abs(tt[i, 1] - want["tmax"]) <= want["tmax"] * ((math.sqrt(3.0) * d_d + 8.0 * EPS) / cos + 2.0 * EPS)
            # the geometric facts, on the float32 ray itself
            of, df = o[i].astype(np.float64), d[i].astype(np.float64)
            s3 = math.sqrt(3.0)
            assert norm(of - P) <= A + s3 * d_o
            assert abs(float((of - P) @ FN)) <= s3 * d_o
            q = P + want["D"] - of
            miss = norm(q - float(q @ df) * df / float(df @ df))
            geo = s3 * d_o + norm(q) * s3 * d_d * 2.0  # (the point moves by d_o, the line turns by d_d a component and is not exactly unit: twice)
            assert miss <= geo, (A, px[i], py[i], u1[i], u2[i], miss, geo)
            worst_geo = max(worst_geo, miss / geo)
    print(f"lens_ray: origin {worst_o:.3f}, direction {worst_d:.3f}, focus point {worst_geo:.3f} of their bounds")


# ---------------------------------------------------------------------------------------------------- CPU: frames of the test scene
W, H = 19, 13


@pytest.fixture(scope="module")
def cpu_scene(dxrs, host):
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(W, H, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    return spheres, mats, sd, cam


@pytest.mark.parametrize("spp", [1, 3])
def test_aperture_zero_is_pt_render(dxrs, shims, cpu_scene, spp):
    """bit for bit against the host sh_query_pixel with the cache off; a pixel whose primary ray hits traces spp primaries where pt_render
    traces one, a pixel whose ray misses one in both"""
    spheres, mats, sd, cam = cpu_scene
    hl = HostLens(shims, spheres, mats, sd)
    for rect in (None, (5, 3, 11, 9)):
        gs = dxrs.types.graphics_settings(W, H, frame_index=5, bounces=8, spp=spp)
        want, rays_want = hl.query_off(cam, gs, rect)
        got, rays = hl.frame(with_lens(cam, 0.0), gs, rect)
        assert same_bits(got, want)
        hits = hl.primary_hits(cam, gs, rect)
        assert 0 < hits < (W * H if rect is None else rect[2] * rect[3]), "the frame must hold both hits and misses"
        assert rays == rays_want + (spp - 1) * hits, (rays, rays_want, hits)
    far = with_lens(cam, 0.0, focus=40.0)
    assert same_bits(hl.frame(far, gs)[0], hl.query_off(far, gs)[0])


def test_lens_stream_is_independent_of_the_bounce_generator(dxrs, host, shims):
    """The camera at the centre of a large diffuse emissive sphere: a chord of a sphere meets it at both ends under the same angle, so
    every vertex of a path sees the geometry of every other and the path's length is decided by the Russian-roulette draws alone.  The
    counting hook (the rays of each pixel): with the lens open they are those of aperture 0 -- the lens takes no number from the bounce
    generator and leaves its order alone -- while another FrameIndex, which moves the generator, changes them."""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(1, SPHERE_DTYPE)
    spheres[0] = (0.0, 0.0, 0.0, 50.0)
    mats = default_material(1)
    mats["BaseColor"][0, :3] = (0.8, 0.7, 0.6)
    mats["Roughness"], mats["Metallic"] = 1.0, 0.0
    mats["EmissiveColor"][0], mats["EmissiveStrength"][0] = (1.0, 0.9, 0.8), 1.0
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.0, 0.0, 0.0, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    hl = HostLens(shims, spheres, mats, sd)
    cam = host.camera_matrices(W, H, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 1.0), jitter=False)
    gs = dxrs.types.graphics_settings(W, H, frame_index=11, bounces=24, spp=2, threshold=0.0)
    img0, rays0, pp0 = hl.frame(with_lens(cam, 0.0), gs, per_pixel=True)
    img1, rays1, pp1 = hl.frame(with_lens(cam, 0.05, focus=10.0), gs, per_pixel=True)
    assert np.array_equal(pp0, pp1) and rays0 == rays1
    assert len(np.unique(pp0)) > 4 and pp0.min() >= 2, "the draws decide the lengths: the hook has something to see"
    assert not same_bits(img0, img1) and np.allclose(img0, img1, rtol=1e-3), "the same paths, seen from other lens points"
    other = dxrs.types.graphics_settings(W, H, frame_index=12, bounces=24, spp=2, threshold=0.0)
    assert not np.array_equal(hl.frame(with_lens(cam, 0.0), other, per_pixel=True)[2], pp0)


# The circle of confusion.  A point at view depth z and lateral position X is seen through the lens point `off` (lateral, in the lens
# plane) along the ray that leaves Position + off towards the in-focus point Position + D, D = (nx |Right|, ny |Up|, F): at depth z that
# ray is at lateral position (z / F) D_lat + off (1 - z / F), so the point appears where D_lat = (F / z) X - off (F / z - 1): the pinhole
# image shifted by -off (F / z - 1), in pixels by W / (2 |Right|) of that a unit (nx = D_lat.x / |Right|, a pixel is 2 / W of nx; the y
# axis has H / (2 |Up|), the same number for square pixels).  The lens frame is the pinhole frame convolved with the distribution of the
# shift; off = A (v.x, v.y) with E[v.x^2] = E[r^2] E[cos^2] = (2/3)(1/2) = 1/3, so every axis' second central moment grows by
#   (A |1 - F / z| W / (2 |Right|))^2 / 3
# and the total energy stays (no pdf weight: every sample counts alike).  The emitter is a sphere, not a plane: its visible surface lies
# in front of its centre by 2/3 of its radius on average, which moves |1 - F / z| by (2/3)(R / z)(F / z): 0.25 % at z = F / 2 with the
# radii below (0.5 % of the added moment), 0.13 % at z = 2 F, and at z = F leaves a blur of 0.003 pixels -- all below the standard errors.
F_DIST, TAN_HALF, CC_APERTURE, CC_W, CC_SPP, CC_REPEATS, CC_RHO = 10.0, 0.02, 0.04, 64, 16, 32, 3.0


def footprint(img):
    """-> (energy, second central moment along x, along y) of the frame's red channel, in pixels"""
    I = img[..., 0].astype(np.float64)
    e = I.sum()
    ys, xs = np.mgrid[0:I.shape[0], 0:I.shape[1]]
    mx, my = (I * xs).sum() / e, (I * ys).sum() / e
    return e, (I * (xs - mx) ** 2).sum() / e, (I * (ys - my) ** 2).sum() / e


@pytest.mark.parametrize("depth", [1.0, 2.0, 0.5])
def test_circle_of_confusion(dxrs, shims, depth):
    from dxrs_amd.abi_types import PtCamera
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    z = depth * F_DIST
    right = TAN_HALF * F_DIST
    radius = CC_RHO * z * TAN_HALF / (CC_W / 2.0)  # CC_RHO pixels on the screen
    spheres = np.zeros(1, SPHERE_DTYPE)
    spheres[0] = (0.0, 0.0, z, radius)
    mats = default_material(1)
    mats["BaseColor"][0, :3] = 0.0
    mats["EmissiveColor"][0], mats["EmissiveStrength"][0] = (1.0, 1.0, 1.0), 1.0
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.0, 0.0, 0.0, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    cam = PtCamera()
    cam.RightDirection[0], cam.UpDirection[1], cam.ForwardDirection[2] = right, right, F_DIST
    cam.NearDepth, cam.FarDepth = 1e-2, math.inf
    hl = HostLens(shims, spheres, mats, sd)
    # the pinhole frame, box-filtered: the mean over an 8 x 8 grid of sub-pixel jitters (a 1-spp frame alone is the mask of the pixel centres,
    # whose area is off by an eighth); the lens frames take a random jitter each, so that their expectation is that frame convolved
    gs1 = dxrs.types.graphics_settings(CC_W, CC_W, frame_index=0, bounces=0, spp=1)
    acc = np.zeros((CC_W, CC_W, 4), np.float64)
    for jy in range(8):
        for jx in range(8):
            cam.Jitter[0], cam.Jitter[1] = (jx + 0.5) / 8.0 - 0.5, (jy + 0.5) / 8.0 - 0.5
            acc += hl.frame(with_lens(cam, 0.0), gs1)[0]
    pin = footprint(acc / 64.0)
    print(f"depth {depth} F: pinhole energy {pin[0]:.4f} (pi rho^2 = {math.pi * CC_RHO ** 2:.4f}), moments {pin[1]:.4f} {pin[2]:.4f} (rho^2 / 4 + 1 / 12 = {CC_RHO ** 2 / 4.0 + 1.0 / 12.0:.4f})")
    assert abs(pin[0] - math.pi * CC_RHO ** 2) < 0.2 and all(abs(pin[a] - CC_RHO ** 2 / 4.0 - 1.0 / 12.0) < 0.1 for a in (1, 2)), "a box-filtered disc of CC_RHO pixels"
    jitters = np.random.default_rng(26).uniform(-0.5, 0.5, (CC_REPEATS, 2))
    runs = []
    for k in range(CC_REPEATS):
        cam.Jitter[0], cam.Jitter[1] = jitters[k]
        runs.append(footprint(hl.frame(with_lens(cam, CC_APERTURE), dxrs.types.graphics_settings(CC_W, CC_W, frame_index=100 + k, bounces=0, spp=CC_SPP))[0]))
    runs = np.array(runs)
    mean, se = runs.mean(axis=0), runs.std(axis=0, ddof=1) / math.sqrt(CC_REPEATS)
    added = (CC_APERTURE * abs(1.0 - F_DIST / z) * CC_W / (2.0 * right)) ** 2 / 3.0
    for axis in (1, 2):
        print(f"depth {depth} F, axis {'xy'[axis - 1]}: pinhole moment {pin[axis]:.4f}, lens {mean[axis]:.4f} +- {se[axis]:.4f}, predicted excess {added:.4f}, "
              f"deviation {(mean[axis] - pin[axis] - added) / max(se[axis], 1e-30):.2f} standard errors")
        if depth == 1.0:
            assert added == 0.0
        else:
            assert se[axis] < 0.05 * added, "the standard error is well below the effect"
        assert abs(mean[axis] - pin[axis] - added) <= 4.0 * se[axis]
    print(f"depth {depth} F: energy pinhole {pin[0]:.3f}, lens {mean[0]:.3f} +- {se[0]:.3f}")
    assert abs(mean[0] - pin[0]) <= 4.0 * se[0]


@pytest.mark.parametrize("aperture", [0.0, 0.05, 1.0])
def test_all_miss_frame_is_the_environment(dxrs, host, shims, aperture):
    """The mean of n equal floats c is c itself where n c is a float32 and n a power of two: any colour at 1 and 2 spp, colours of a few
    mantissa bits at 4 spp.  (At aperture 0 a missing pixel is the environment itself, as in pt_render, at any spp.)"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(1, SPHERE_DTYPE)
    spheres[0] = (0.0, 0.0, -100.0, 1.0)  # behind the camera
    sd = PtSceneData()
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    cam = with_lens(host.camera_matrices(W, H, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 1.0)), aperture, focus=3.0)
    for colour, spps in (((0.1, 0.7, 1.3), (1, 2) if aperture else (1, 2, 3, 5)), ((0.5, 0.25, 1.75), (1, 2, 4))):
        sd.EnvironmentLightColor[:] = (*colour, 1.0)
        hl = HostLens(shims, spheres, default_material(1), sd)
        for spp in spps:
            img, rays = hl.frame(cam, dxrs.types.graphics_settings(W, H, frame_index=3, bounces=8, spp=spp))
            assert (img == np.array([*colour, 1.0], np.float32)).all(), (colour, spp)
            assert rays == W * H * (spp if aperture else 1)


# ---------------------------------------------------------------------------------------------------- CPU: sanitizers
def test_sanitized_stand_alone_program(tmp_path):
    """the host header's frame at apertures 0 and > 0, 1x1 and ragged frames and a sub-rect, under ASan + UBSan, in a child process (nothing
    sanitised is loaded into Python)"""
    exe = str(tmp_path / "lens_sanitize")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-o", exe, "lens_sanitize.cpp"], cwd=os.path.join(HERE, "hostshim"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout


# ---------------------------------------------------------------------------------------------------- GPU
SHAPES = [(19, 13, (4, 2, 13, 9)), (1, 1, None)]


def c1(dxrs, host, w, h, **cam_kw):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    return spheres, mats, sd, host.camera_matrices(w, h, **cam_kw)


def render_lens_both(r, rect, w, h):
    """the frame through the host `out` and through a device `out`: both must hold the same bits -> (image, stats)"""
    import torch
    img, s = r.render_lens(rect)
    rw, rh = (rect[2], rect[3]) if rect else (w, h)
    dev = torch.zeros((rh, rw, 4), dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    s2 = r.render_lens_device(dev.data_ptr(), rect, want_stats=True)
    assert same_bits(dev.cpu().numpy(), img) and s2.rays == s.rays
    return img, s


def check_variant(dxrs, r, hl, spheres, mats, sd, cam, w, h, rect, textures=None, bounces=8):
    """aperture 0 against pt_render, aperture 0.05 against the host header with equal ray counts: the whole frame and `rect`, spp 1 and 3"""
    for spp in (1, 3):
        gs = dxrs.types.graphics_settings(w, h, frame_index=3, bounces=bounces, spp=spp)
        setup(r, dxrs, spheres, mats, sd, with_lens(cam, 0.0), gs, textures)
        for rc in (None, rect) if rect else (None,):
            want, _ = r.render(rc)
            got, _ = render_lens_both(r, rc, w, h)
            assert same_bits(got, want), f"aperture 0, spp {spp}, rect {rc}: {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} pixels differ from pt_render"
        open_cam = with_lens(cam, 0.05, focus=12.0)
        r.set_camera(open_cam)
        for rc in (None, rect) if rect else (None,):
            got, s = render_lens_both(r, rc, w, h)
            want, rays = hl.frame(open_cam, gs, rc)
            assert same_bits(got, want), f"aperture 0.05, spp {spp}, rect {rc}: {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} pixels differ from the host header"
            assert s.rays == rays, (spp, rc, s.rays, rays)
            assert s.pixels == got.shape[0] * got.shape[1] and s.paths == s.pixels * spp


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,rect", SHAPES)
def test_gpu_scene_in_lds(dxrs, host, renderer, shims, w, h, rect):
    spheres, mats, sd, cam = c1(dxrs, host, w, h)
    check_variant(dxrs, renderer, HostLens(shims, spheres, mats, sd), spheres, mats, sd, cam, w, h, rect)
    assert renderer.accel.lds_resident
    if (w, h) == (19, 13):
        got, _ = renderer.render_lens()
        pin, _ = renderer.render()
        assert not same_bits(got, pin), "an open lens changes the frame"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,rect", SHAPES)
def test_gpu_scene_in_global_memory(dxrs, host, shims, w, h, rect):
    r = dxrs.Renderer(device=0, flags=dxrs.types.PT_FLAG_NO_LDS_SCENE)
    try:
        spheres, mats, sd, cam = c1(dxrs, host, w, h)
        check_variant(dxrs, r, HostLens(shims, spheres, mats, sd), spheres, mats, sd, cam, w, h, rect)
        assert not r.accel.lds_resident
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "latlong"])
def test_gpu_textured_with_an_environment_map(dxrs, host, renderer, shims, kind):
    """the small scene under the rotated cube environment of golden row a18, and under the same function as a lat-long map: the textured
    instances' environment functor, fed the lens rays' own directions (a primary miss of an open lens) and the bounce rays'"""
    import golden_cases
    from dxrs_amd import textures as T
    case = next(c for c in golden_cases.cases(dxrs, host) if c["file"].startswith("a18_cube"))
    sd, ts = case["sd"], case["textures"]
    if kind == "latlong":
        ts = T.TextureSet(len(case["spheres"]))
        yy, xx = np.mgrid[0:16, 0:32]
        img = np.stack([0.6 + 0.4 * np.cos(xx * (math.pi / 16.0)), 0.3 + yy / 20.0, 0.9 + 0.5 * np.sin(xx * (math.pi / 8.0)), np.ones_like(xx, dtype=np.float64)], -1)
        sd = copy.copy(sd)
        sd.EnvironmentLightTextureDescriptor, sd.IsEnvironmentLightTextureCubeMap = ts.add_hdr_image(img.astype(np.float32)), 0
    w, h = 19, 13
    cam = host.camera_matrices(w, h, jitter_index=2)
    hl = HostLens(shims, case["spheres"], case["materials"], sd, textures=ts)
    try:
        check_variant(dxrs, renderer, hl, case["spheres"], case["materials"], sd, cam, w, h, (4, 2, 13, 9), textures=ts, bounces=5)
        gs = dxrs.types.graphics_settings(w, h, frame_index=3, bounces=5, spp=3)
        assert hl.primary_hits(cam, gs) < w * h, "some primary rays must reach the map"
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_textured_without_alpha_test(dxrs, host, renderer, shims):
    """test_sharc.py's emissive map on an emitter, nothing alpha-tested: the textured instances with the plain walk"""
    from dxrs_amd.textures import TextureSet
    spheres, mats, sd = make_scene(dxrs)
    ts = TextureSet(len(spheres))
    yy, xx = np.mgrid[0:32, 0:64]
    checker = ((xx // 4 + yy // 4) & 1).astype(np.uint8)
    glow = np.zeros((32, 64, 4), np.uint8)
    glow[..., 0], glow[..., 1], glow[..., 2], glow[..., 3] = 255, 80 + 175 * checker, 40 + 215 * checker, 255
    ts.maps[1, 1] = ts.add_image(glow)
    w, h = 19, 13
    cam = host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70))
    try:
        check_variant(dxrs, renderer, HostLens(shims, spheres, mats, sd, textures=ts), spheres, mats, sd, cam, w, h, (4, 2, 13, 9), textures=ts)
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_alpha_tested(dxrs, host, renderer, shims):
    """the alpha-tested golden scene (tests/golden_cases.py, row a5): the kTex / kAlpha instances"""
    import golden_cases
    case = next(c for c in golden_cases.cases(dxrs, host) if c["file"].startswith("a5_alpha"))
    w, h = 19, 13
    cam = host.camera_matrices(w, h, position=(0.0, 2.0, -7.0), jitter_index=1)
    hl = HostLens(shims, case["spheres"], case["materials"], case["sd"], textures=case["textures"])
    try:
        check_variant(dxrs, renderer, hl, case["spheres"], case["materials"], case["sd"], cam, w, h, (4, 2, 13, 9), textures=case["textures"], bounces=5)
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_tree_with_32_bit_stack(dxrs, host, shims):
    """40,000 spheres (test_sharc.py's scene): more than 32,767 nodes, so the instances with the 32-bit traversal stack run"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=40000)
    w, h = 19, 13
    cam = host.camera_matrices(w, h)
    r = dxrs.Renderer(device=0)
    try:
        check_variant(dxrs, r, HostLens(shims, spheres, mats, sd), spheres, mats, sd, cam, w, h, (4, 2, 13, 9))
        assert r.accel.node_count >= 32767 and not r.accel.lds_resident
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [0, 8])
def test_gpu_bounces_and_consecutive_frames(dxrs, host, renderer, shims, bounces):
    """three consecutive FrameIndex values with a moving camera, against the host header"""
    w, h = 19, 13
    spheres, mats, sd, cam = c1(dxrs, host, w, h)
    hl = HostLens(shims, spheres, mats, sd)
    cams = [cam]
    for k in (1, 2):
        cams.append(host.camera_matrices(w, h, position=(0.6 * k, 0.3 * k, -15.0 + k), look_at=(0.0, 0.0, 0.0), jitter_index=k, previous=cams[-1]))
    for f, base in enumerate(cams):
        gs = dxrs.types.graphics_settings(w, h, frame_index=f, bounces=bounces, spp=2)
        open_cam = with_lens(base, 0.1, focus=13.0)
        if f == 0:
            setup(renderer, dxrs, spheres, mats, sd, open_cam, gs)
        renderer.set_camera(open_cam)
        renderer.set_constants(gs)
        got, s = renderer.render_lens()
        want, rays = hl.frame(open_cam, gs)
        assert same_bits(got, want) and s.rays == rays, (f, s.rays, rays)
        if bounces == 0:
            assert s.rays == w * h * 2


@pytest.mark.gpu
def test_gpu_interleaved_with_frames_in_flight(dxrs, host, shims):
    """pt_render frames in flight on three lanes while pt_render_lens calls run: queued equals synchronised"""
    import torch
    w, h = 19, 13
    spheres, mats, sd, cam = c1(dxrs, host, w, h)
    hl = HostLens(shims, spheres, mats, sd)
    open_cam = with_lens(cam, 0.05, focus=12.0)
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        gs = [dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1) for f in range(3)]
        setup(r, dxrs, spheres, mats, sd, open_cam, gs[0])
        alone = []
        for f in range(3):
            r.set_constants(gs[f])
            alone.append(r.render()[0])
        dev = torch.device("cuda", 0)
        frames = [torch.zeros((h, w, 4), dtype=torch.float32, device=dev) for _ in range(3)]
        lens = [torch.zeros((h, w, 4), dtype=torch.float32, device=dev) for _ in range(3)]
        torch.cuda.synchronize(dev)
        for f in range(3):
            r.set_constants(gs[f])
            r.render_lens_device(lens[f].data_ptr())
            r.render_device(frames[f].data_ptr())
        r.synchronize()
        for f in range(3):
            want, _ = hl.frame(open_cam, gs[f])
            assert same_bits(frames[f].cpu().numpy(), alone[f]), f"frame {f}: pt_render changed"
            assert same_bits(lens[f].cpu().numpy(), want), f"frame {f}: pt_render_lens differs from the host header"
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_argument_errors(dxrs, host, renderer):
    from dxrs_amd.abi_types import PtRect
    w, h = 19, 13
    spheres, mats, sd, cam = c1(dxrs, host, w, h)
    gs = dxrs.types.graphics_settings(w, h, frame_index=0, bounces=4, spp=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    want, _ = renderer.render()
    lib, ctx = renderer._lib, renderer._ctx
    out = np.full((h, w, 4), 7.0, np.float32)
    assert lib.pt_render_lens(ctx, None, None, 0, None) == 1, "null output"
    bad = PtRect(15, 0, 10, 10)
    assert lib.pt_render_lens(ctx, C.byref(bad), out.ctypes.data, 0, None) == 1, "a rect outside RenderSize"
    for aperture in (-1e-6, -1.0, float("nan"), float("inf"), float("-inf")):
        renderer.set_camera(with_lens(cam, aperture))  # pt_set_camera accepts anything
        assert lib.pt_render_lens(ctx, None, out.ctypes.data, 0, None) == 1, aperture
        assert lib.pt_last_error(ctx)
        got, _ = renderer.render()
        assert same_bits(got, want), "pt_render ignores the field"
    renderer.set_camera(with_lens(cam, 0.05))
    renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=0, bounces=4, spp=1, di=True))
    assert lib.pt_render_lens(ctx, None, out.ctypes.data, 0, None) == 5, "IsDIEnabled"
    assert (out == 7.0).all(), "a refused call writes nothing"
    renderer.set_constants(gs)
    fresh = dxrs.Renderer(device=0)
    try:
        assert fresh._lib.pt_render_lens(fresh._ctx, None, out.ctypes.data, 0, None) == 4, "PT_ERR_STATE: no scene"
    finally:
        fresh.close()
    renderer.set_camera(with_lens(cam, 0.0))
    got, _ = renderer.render_lens()
    assert same_bits(got, want), "the context renders a correct frame after the refusals"


@pytest.mark.gpu
def test_gpu_cpp_mirror(dxrs, host, tmp_path):
    """Raytracing::RenderThinLens (tests/cpp/host_lens.cpp) against the Python binding with the camera the program used"""
    from dxrs_amd.abi_types import PtCamera
    pkg = os.path.dirname(dxrs.__file__)
    exe = str(tmp_path / "host_lens")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_lens.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 48, 27
    outp = str(tmp_path / "lens.f32")
    res = subprocess.run([exe, str(w), str(h), "0.3", "14", outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    n = w * h * 16
    lens, pinhole, plain = (raw[k * n:(k + 1) * n].view(np.float32).reshape(h, w, 4) for k in range(3))
    cam = PtCamera.from_buffer_copy(raw[3 * n:].tobytes())
    assert abs(cam.ApertureRadius - 0.3) < 1e-6 and abs(math.sqrt(sum(float(x) ** 2 for x in cam.ForwardDirection)) - 14.0) < 1e-4
    assert same_bits(pinhole, plain) and not same_bits(lens, plain)
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0)
    try:
        r.set_scene(spheres, mats, sd)
        r.set_camera(cam)
        r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=2, bounces=6, spp=2))
        got, _ = r.render_lens()
        assert same_bits(got, lens)
    finally:
        r.close()
