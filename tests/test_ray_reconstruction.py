"""Row N15 -- the ray-reconstruction stand-in (pt_ray_reconstruction: Streamline's DLSS-RR feature as
App::ProcessDLSSRayReconstruction drives it; DESIGN.md spec S21).
CPU: the product's header (csrc/pt_rr.h compiled as host C++ by tests/hostshim/rr_host.cpp) stage by stage against the float64 numpy
restatement (tests/rr_reference.py); the identities (an all-miss sequence is pt_upscale bit for bit, constant luminance under a random
albedo comes back to a few ulp); the tile bound; the virtual motion of a plane mirror against the analytic image point; the history
rules; the quality on a noisy jittered pattern against pt_upscale's header on the same inputs; ASan + UBSan over a stand-alone program.
GPU: pt_ray_reconstruction against the host-compiled header bit for bit, output and downloaded history (random sequences, a sequence
with motion, a Reset and a size change, the real chain G-buffer -> pt_render_denoiser mode 1 -> pt_ray_reconstruction, one frame at a
time and two in flight), the all-miss identity on the device, argument errors, the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rr_reference as ref
from test_upscale import HostUpscaler, jitter_of, pattern

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
SENTINEL = np.uint32(0x7FC0BEEF).view(np.float32)  # a NaN with a payload: survives exactly where nothing is written
GUARD = 64  # float4 texels either side of Output that a call must leave alone
U = 2.0 ** -24  # half an ulp of 1: the relative error of one fp32 rounding
SIZES = [((1, 1), (1, 1)), ((33, 9), (50, 14)), ((41, 29), (41, 29)), ((16, 16), (64, 64))]
TEXTURES = ("Color", "Depth", "MotionVector", "NormalRoughness", "DiffuseAlbedo", "SpecularAlbedo", "SpecularHitDistance")
# The header (fp32) against the float64 restatement, per pixel (test notes).
# Prepare.  The staged colour t = d / (1 + max d), d = min(c' / max(A, eps), 65504): A carries one rounding (the sum), the quotient one,
# the sum 1 + max d one, the second quotient one: 4 U relative, and t < 1, so 4 U absolute; PREP_T_TOL is twice that.  Normal and
# roughness are selections and clamps: exact.  The virtual motion: the NDC (3 roundings), ProjectionToView (a 3-fma chain per
# component), two quotients, two products, ViewToWorld (3 fma), X - Position (1), the normalisation (5), X + V s (2),
# PreviousWorldToProjection (3), the quotient and the fma to uv (2), the difference and the product with the size (2): about 32
# roundings, each relative to the largest term of its sum, which the cancellation in X - Position and in uv_prev - uv turns into an
# absolute error in uv of 32 U max(1, |uv_prev|), times the image's extent in pixels; VIRT_TOL doubles the count.  The weight is two
# luminances (3 roundings each), a sum, a quotient and a product: WEIGHT_TOL = 16 U.
PREP_T_TOL = 8 * U
VIRT_TOL = 64 * U
WEIGHT_TOL = 16 * U
# Resolve.  As S17 (test_upscale.py): the position p = (o + 0.5)(w / W) carries two roundings that the tap offsets inherit, and the
# kernels and the coverage have slopes of at most about W / w per input pixel, so colour and weight move by up to 1.2e-7 max(W, H):
# T_RTOL times the output's larger extent.  On top, independent of the extent: the edge-stopping terms (the depth term is a rounded
# difference times a rounded reciprocal, 3 U; the normal term a 3-term dot product scaled by 5, 20 U; the roughness term 4 U), the
# 25-tap sums (25 U), the renormalised bilinear history tap (four products, three sums, a reciprocal and a product: 10 U): T_EDGE =
# 64 U covers their sum.  The clip's bounds mean +- 1.5 sigma carry sigma's error: sigma^2 = m2 / sw - e^2 is a difference whose
# rounding, about 20 U of m2 / sw, is relative to the variance only where the variance is not small against m2 / sw; the restatement
# reports that ratio as a margin, and a pixel below RESOLVE_MARGIN (the floor of the variance) is one of those that may be left out.
T_RTOL = 3e-7
T_EDGE = 64 * U
OUT_RTOL = 2e-3       # of the frame's largest finite value: the inverse tone map amplifies by (1 + c)^2 (test_upscale.py)
RESOLVE_MARGIN = 1e-4
FLIP_SHARE = 1e-3     # the share of a case's pixels that may sit within the tolerance of a branch or floor decision


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_rr_shim())
    lib.rr_host_prepare.restype = None
    lib.rr_host_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rr_host_frame.restype = C.c_uint32
    lib.rr_host_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.rr_host_max_extent.restype = C.c_uint32
    lib.rr_host_max_extent.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.rr_host_tile_w.restype = lib.rr_host_tile_h.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def up_shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_upscale_shim())
    lib.up_host_frame.restype = None
    lib.up_host_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.up_host_frame_tiled.restype = C.c_uint32
    lib.up_host_frame_tiled.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return lib


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def make_camera(w, h, position, previous_position=None, near=0.1, far=100.0, hfov=np.pi / 2):
    """a camera at `position` looking down +z (DirectXMath row vectors): clip = [p, 1] . WorldToView . ViewToProjection, clip.w = the
    view depth; the fp32 values both the header and the restatement are given"""
    xs = 1.0 / np.tan(hfov / 2.0)
    ys = xs * w / h
    A = far / (far - near)
    proj = np.array([[xs, 0, 0, 0], [0, ys, 0, 0], [0, 0, A, 1], [0, 0, -near * A, 0]], np.float64)

    def world_to_view(p):
        m = np.eye(4)
        m[3, :3] = -np.asarray(p, np.float64)
        return m

    prev = position if previous_position is None else previous_position
    return dict(Position=c32(position), ProjectionToView=c32(np.linalg.inv(proj)).ravel(), ViewToWorld=c32(np.linalg.inv(world_to_view(position))).ravel(),
                PreviousWorldToProjection=c32(world_to_view(prev) @ proj).ravel(), xs=xs, ys=ys)


def settings_floats(cam, jitter, max_a):
    return c32(np.concatenate([[jitter[0], jitter[1], max_a or 16.0], cam["Position"], cam["ProjectionToView"], cam["ViewToWorld"],
                               cam["PreviousWorldToProjection"]]))


class HostReconstructor:
    """pt_ray_reconstruction on the host-compiled header, with the history logic of pt_api_post.hip: the first call, Reset and a change
    of either size restart; two history slots alternate, re-made when a size changes."""

    def __init__(self, shim, tiled=False):
        self.shim, self.key, self.slots, self.cur, self.restarted, self.tiled, self.rec = shim, None, None, 0, None, tiled, None

    def __call__(self, tex, cam, out_size, jitter=(0.0, 0.0), reset=False, max_a=0.0):
        tex = {k: c32(tex[k]) for k in TEXTURES}
        h, w = tex["Depth"].shape
        W, H = out_size
        restart = bool(reset) or self.key is None
        if self.key != (w, h, W, H):
            self.slots = [(np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)) for _ in range(2)]
            restart = True
        self.key = (w, h, W, H)
        prev, cur = self.slots[self.cur], self.slots[self.cur ^ 1]
        out = np.full((H, W, 4), SENTINEL, np.float32)
        self.rec = tuple(np.full((h, w, 4), SENTINEL, np.float32) for _ in range(3))
        size = np.array([w, h, W, H], np.uint32)
        fprm = settings_floats(cam, jitter, max_a)
        arrays = [tex[k] for k in TEXTURES] + [out, *self.rec, *prev, *cur]
        ptrs = (C.c_void_p * 17)(*[a.ctypes.data for a in arrays])
        assert self.shim.rr_host_frame(size.ctypes.data, fprm.ctypes.data, 1 if restart else 0, 1 if self.tiled else 0, ptrs) == 0
        self.cur ^= 1
        self.restarted = restart
        return out

    def history(self):
        """the slot the last call wrote: (hist (H, W, 4), normal (H, W, 4), z (H, W))"""
        return self.slots[self.cur]


def unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def random_scene(rng, w, h, miss=0.1):
    """what stays from frame to frame: a tilted plane with a raised block and misses, normals that lean a little (a few lean far),
    roughness in blocks, two albedos; some NaN payloads among the guides"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    depth = (5.0 + 0.02 * xs + 0.01 * ys).astype(np.float32)
    depth[h // 3:h // 2 + 1, w // 4:w // 2 + 1] -= 2.0
    depth[rng.random((h, w)) < miss] = np.inf
    n = np.concatenate([rng.normal(0.0, 0.15, (h, w, 2)), -np.ones((h, w, 1))], axis=-1)
    far = rng.random((h, w)) < 0.05
    n[far] = rng.normal(0.0, 1.0, (int(far.sum()), 3))
    rough = np.repeat(np.repeat(rng.uniform(0.0, 1.0, ((h + 3) // 4, (w + 3) // 4)) ** 2, 4, axis=0), 4, axis=1)[:h, :w]
    rough = rough + rng.uniform(-0.03, 0.03, (h, w))
    nr = np.concatenate([unit(n), rough[..., None]], axis=-1).astype(np.float32)
    nr[rng.random((h, w, 4)) < 0.004] = np.nan
    da = rng.uniform(0.02, 0.9, (h, w, 3)).astype(np.float32)
    sa = rng.uniform(0.0, 0.3, (h, w, 3)).astype(np.float32)
    da[rng.random((h, w, 3)) < 0.003] = np.nan
    da[rng.random((h, w)) < 0.01] = 0.0
    return dict(Depth=depth, NormalRoughness=nr, DiffuseAlbedo=da, SpecularAlbedo=sa)


def random_frame(rng, scene):
    """a frame over `scene`: an HDR image over six decades with fireflies, NaN, +-inf and negative channels; sub-pixel motion, a few
    pixels moving far; hit distances of which a third are 0 and a few not finite"""
    h, w = scene["Depth"].shape
    rgb = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 3))).astype(np.float32)
    for value, share in ((np.nan, 0.01), (np.inf, 0.01), (-np.inf, 0.005), (-1.5, 0.02), (6.0e4, 0.01)):
        rgb[rng.random((h, w, 3)) < share] = value
    color = np.concatenate([rgb, rng.uniform(0.0, 1.0, (h, w, 1)).astype(np.float32)], axis=-1)
    mv = rng.uniform(-0.9, 0.9, (h, w, 3)).astype(np.float32)
    mv[..., 2] *= 0.05
    mv[rng.random((h, w)) < 0.03, :2] = 40.0
    hit = rng.uniform(0.1, 20.0, (h, w)).astype(np.float32)
    hit[rng.random((h, w)) < 0.33] = 0.0
    for value, share in ((np.nan, 0.01), (np.inf, 0.01), (-1.0, 0.01)):
        hit[rng.random((h, w)) < share] = value
    return dict(scene, Color=color, MotionVector=mv, SpecularHitDistance=hit)


def travelling_camera(w, h, f):
    pos = lambda k: (0.3 + 0.05 * k, -0.2 + 0.02 * k, -1.0 + 0.03 * k)
    return make_camera(w, h, pos(f), pos(f - 1) if f else None)


def finite_max(a):
    a = np.asarray(a, np.float64)
    a = np.abs(a[np.isfinite(a)])
    return float(a.max()) if a.size else 1.0


# ------------------------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("sizes,seed", [(SIZES[0], 0), (SIZES[1], 1), (SIZES[2], 2), (SIZES[3], 3)])
def test_header_matches_numpy_restatement(shim, sizes, seed):
    """4-frame sequences; every frame of the header stage by stage against the restatement: the prepare records and the virtual motion,
    then the resolve pass fed the header's own records and previous history slot: output and every history plane"""
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(seed)
    rr = HostReconstructor(shim)
    scene = random_scene(rng, w, h, miss=0.0 if w == 1 else 0.1)
    worst = dict(t=0.0, virt=0.0, weight=0.0, ht=0.0, ha=0.0, out=0.0)
    flips = total = prep_flips = prep_total = 0
    for f in range(4):
        tex = random_frame(rng, scene)
        cam = travelling_camera(w, h, f)
        prev = None if f == 0 else tuple(a.copy() for a in rr.history())
        jit = jitter_of(f)
        out = rr(tex, cam, (W, H), jitter=jit, max_a=3.0)
        assert rr.restarted == (f == 0)
        # stage 1
        p = ref.prepare(tex, cam, jit)
        tz, nr, virt = rr.rec
        assert np.array_equal(tz[..., 3].view(np.uint32), p["tz"][..., 3].astype(np.float32).view(np.uint32))
        assert np.array_equal(nr.view(np.uint32), p["nr"].astype(np.float32).view(np.uint32))  # selections and clamps: exact
        assert np.array_equal(virt[..., 3], np.zeros((h, w), np.float32))
        err_t = np.abs(tz[..., :3] - p["tz"][..., :3]).max(axis=-1)
        assert err_t.max() <= PREP_T_TOL, err_t.max()
        with np.errstate(invalid="ignore"):
            clip = p["virtual_clip"]
            reach = np.maximum(1.0, np.nan_to_num(np.abs(clip[..., :2] / clip[..., 3:4]).max(axis=-1), nan=1.0, posinf=1.0))
        err_v = np.abs(virt[..., :2].astype(np.float64) - p["virt"][..., :2]).max(axis=-1) / (reach * max(w, h))
        err_w = np.abs(virt[..., 2] - p["virt"][..., 2])
        with np.errstate(invalid="ignore"):
            bad = ~((err_v <= VIRT_TOL) & (err_w <= WEIGHT_TOL))
        bad &= ~(np.isnan(p["virt"][..., :2]).any(axis=-1) & np.isnan(virt[..., :2]).any(axis=-1))  # a NaN vector stays a NaN vector
        flipped = bad & (p["margin"] < VIRT_TOL)
        assert not (bad & ~flipped).any(), (f, np.argwhere(bad & ~flipped)[:4].tolist(), np.nanmax(err_v), np.nanmax(err_w))
        prep_flips += int(flipped.sum())
        prep_total += bad.size
        used = p["virt"][..., 2] > 0
        if w > 1:
            assert 0.05 < used.mean() < 0.95  # pixels with and without a virtual motion
        worst.update(t=max(worst["t"], err_t.max()), virt=max(worst["virt"], np.nanmax(np.where(bad, 0.0, err_v))), weight=max(worst["weight"], err_w[~bad].max()))
        # stages 2-6, from the header's records
        want = ref.resolve(tex, dict(tz=tz, nr=nr, virt=virt[..., :3]), prev, (W, H), jit, 3.0)
        hist, hist_n, z = rr.history()
        scale = finite_max(want["out"][..., :3])
        err_ht = np.abs(hist[..., :3] - want["hist"][..., :3]).max(axis=-1)
        err_ha = np.abs(hist[..., 3] - want["hist"][..., 3]) / 3.0
        err_o = np.abs(out[..., :3] - want["out"][..., :3]).max(axis=-1) / scale
        tol = T_RTOL * max(W, H) + T_EDGE
        bad = (err_ht > tol) | (err_ha > tol) | (err_o > OUT_RTOL)
        flipped = bad & (want["margin"] < max(tol, RESOLVE_MARGIN))
        assert not (bad & ~flipped).any(), (f, np.argwhere(bad & ~flipped)[:4].tolist(), err_ht.max(), err_ha.max(), err_o.max())
        ok = ~bad
        worst.update(ht=max(worst["ht"], err_ht[ok].max()), ha=max(worst["ha"], err_ha[ok].max()), out=max(worst["out"], err_o[ok].max()))
        flips += int(flipped.sum())
        total += bad.size
        assert np.array_equal(z.view(np.uint32), want["z"].astype(np.float32).view(np.uint32))  # the depth is a selection: exact
        assert np.array_equal(hist_n.view(np.uint32), want["hist_n"].astype(np.float32).view(np.uint32))
        assert np.array_equal(out[..., 3].view(np.uint32), want["out"][..., 3].astype(np.float32).view(np.uint32))  # alpha is copied
        assert np.isfinite(out[..., :3]).all() and np.isfinite(hist).all()
        if f and w > 1:
            s = want["surface"]
            assert 0.3 < want["accepted"][s].mean() < 0.99  # both branches of the blend are taken
    print(f"{w}x{h} -> {W}x{H}: prepare t {worst['t']:.3g} virt {worst['virt']:.3g} weight {worst['weight']:.3g}; resolve t {worst['ht']:.3g} "
          f"weight {worst['ha']:.3g} out {worst['out']:.3g}; left out: prepare {prep_flips} of {prep_total}, resolve {flips} of {total}")
    assert flips <= FLIP_SHARE * total and prep_flips <= FLIP_SHARE * prep_total


@pytest.mark.parametrize("sizes", [((24, 16), (24, 16)), ((24, 16), (48, 32))])
def test_all_miss_sequence_is_pt_upscale(shim, up_shim, sizes):
    """every depth +inf: Output and the history equal pt_upscale's header bit for bit, given the same Color, Depth, Velocity, Jitter,
    Reset and MaxHistoryWeight; the guides are random and must not matter"""
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(21)
    rr, upscaler = HostReconstructor(shim, tiled=True), HostUpscaler(up_shim)
    scene = random_scene(rng, w, h)
    scene["Depth"] = np.full((h, w), np.inf, np.float32)
    for f in range(5):
        tex = random_frame(rng, scene)
        reset = f == 3
        got = rr(tex, travelling_camera(w, h, f), (W, H), jitter=jitter_of(f), reset=reset, max_a=4.0)
        want = upscaler(tex["Color"], tex["Depth"], tex["MotionVector"], (W, H), jitter=jitter_of(f), reset=reset, max_a=4.0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
        assert np.array_equal(rr.history()[0].view(np.uint32), upscaler.history()[0].view(np.uint32)), f
        assert np.array_equal(rr.history()[2].view(np.uint32), upscaler.history()[1].view(np.uint32)), f
        assert not rr.history()[1].any()
    assert rr.history()[0][..., 3].max() > 1.0  # the history was used


def test_constant_luminance_returns_the_albedo(shim):
    """Color = L (DiffuseAlbedo + SpecularAlbedo) with a random albedo texture, at 1:1: Output = L albedo from the first frame on, the
    albedo's detail unfiltered.  The bound: the demodulated d = fl(fl(L A) / A) is L (1 +- 2 U) and t = d / (1 + max d) adds two
    roundings, so the taps' t lie within 4 U of t(L); the moments about the centre keep the mean inside the taps' hull (+ 1 U for the
    sum t_c + e), the renormalised bilinear history adds 6 U, the blend's fma 1 U: t_out within 12 U (relative) of t(L).  The inverse
    t / (1 - max t) divides by 1 - t = 1 / (1 + L), whose absolute error 12 U t + U becomes relative (12 U L + U (1 + L)); with the
    quotient and the product with A: (12 + 12 L + (1 + L) + 2) U in all, and one more for comparing against fl(L A)."""
    w, h, L = 37, 23, 0.75
    bound = (12 + 12 * L + (1 + L) + 3) * U
    rng = np.random.default_rng(8)
    da = rng.uniform(0.02, 0.9, (h, w, 3)).astype(np.float32)
    sa = rng.uniform(0.0, 0.3, (h, w, 3)).astype(np.float32)
    A = (da + sa).astype(np.float32)
    color = np.concatenate([np.float32(L) * A, np.ones((h, w, 1), np.float32)], axis=-1)
    nr = np.zeros((h, w, 4), np.float32)
    nr[..., 2], nr[..., 3] = -1.0, 0.5
    tex = dict(Color=color, Depth=np.full((h, w), 4.0, np.float32), MotionVector=np.zeros((h, w, 3), np.float32), NormalRoughness=nr, DiffuseAlbedo=da,
               SpecularAlbedo=sa, SpecularHitDistance=np.zeros((h, w), np.float32))
    rr = HostReconstructor(shim)
    cam = make_camera(w, h, (0.0, 0.0, 0.0))
    want = np.float64(np.float32(L)) * A.astype(np.float64)
    worst = 0.0
    for f in range(6):
        out = rr(tex, cam, (w, h), jitter=jitter_of(f))
        worst = max(worst, float(np.abs(out[..., :3] / want - 1.0).max()))
    print(f"constant luminance: {worst / U:.2f} U against a bound of {bound / U:.1f} U")
    assert worst <= bound
    assert rr.history()[0][..., 3].min() > 2.0  # the history was blended in


@pytest.mark.parametrize("sizes", SIZES + [((1, 1), (4, 4)), ((33, 9), (129, 33)), ((255, 31), (256, 32)), ((1000, 5), (1001, 17))])
def test_workgroup_tiles_hold_every_tap(shim, sizes):
    """the kernel's staging, run on the host: per 32 x 8 block the footprint of rr_footprint in a 36 x 12 tile holds every tap of the
    block's lanes, and the frames equal the whole-image path"""
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(w + 7 * W)
    whole, tiled = HostReconstructor(shim), HostReconstructor(shim, tiled=True)
    scene = random_scene(rng, w, h)
    for f in range(2):
        tex = random_frame(rng, scene)
        cam = travelling_camera(w, h, f)
        a = whole(tex, cam, (W, H), jitter=jitter_of(f))
        b = tiled(tex, cam, (W, H), jitter=jitter_of(f))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
        for x, y in zip(whole.history(), tiled.history()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f


def test_tile_bound_over_a_sweep_of_ratios_and_at_the_largest_sizes(shim):
    """The footprint a block's taps need (rr_footprint_extent, before the kernel bounds it by the tile) stays within 36 x 12 input
    pixels: the sweep of test_upscale.py's test_footprint_bound_over_a_sweep_of_ratios.  The bound is reached."""
    tile = {32: shim.rr_host_tile_w(), 8: shim.rr_host_tile_h()}
    assert tile == {32: 36, 8: 12}
    pairs = [(n, N) for N in range(1, 161) for n in range((N + 3) // 4, N + 1)]
    for N in (255, 256, 257, 1023, 1024, 1025, 1080, 1920, 2160, 3840, 4095, 4096, 4097):
        pairs += [(n, N) for n in range((N + 3) // 4, N + 1)]
    pairs += [(n, N) for N in range(16384 - 63, 16385) for n in range(N - 63, N + 1)]
    pairs += [((N + 3) // 4, N) for N in range(16384 - 63, 16385)]
    rng = np.random.default_rng(11)
    for N in rng.integers(161, 16385, 3000):
        pairs.append((int(rng.integers((N + 3) // 4, N + 1)), int(N)))
    widest = {32: 0, 8: 0}
    for n, N in pairs:
        for block in (32, 8):
            e = shim.rr_host_max_extent(n, N, block)
            assert e <= tile[block], (n, N, block, e)
            widest[block] = max(widest[block], e)
    assert widest == tile
    # 16383 -> 16384 on one axis (the ratio closest to 1 from below): one row of blocks of each orientation through the tiled path
    for (w, h), (W, H) in (((16383, 3), (16384, 8)), ((3, 16383), (8, 16384))):
        rng = np.random.default_rng(3)
        scene = random_scene(rng, w, h)
        HostReconstructor(shim, tiled=True)(random_frame(rng, scene), make_camera(w, h, (0.0, 0.0, 0.0)), (W, H), jitter=(0.3, -0.4))


def test_virtual_motion_of_a_plane_mirror(shim):
    """A mirror in the plane z = 6 seen by a camera that has moved; behind every pixel's reflection a point at distance hit.  The
    reflected point's image Q' lies on the view ray through the mirror point X, hit beyond it, so the prepare pass's virtual position
    must be the projection of Q' through the previous camera -- here from the ray-plane intersection in float64, not through
    ProjectionToView -- within VIRT_TOL pixels per pixel of extent (the bound derived at the top of the file).  With hit distance 0
    the virtual motion is the surface motion bit for bit and its weight is 0."""
    w, h = 48, 27
    pos, prev_pos = np.array([0.4, -0.3, -2.0]), np.array([0.1, -0.2, -2.5])
    cam = make_camera(w, h, pos, prev_pos)
    jit = (0.25, -0.125)
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = (xs + 0.5 - jit[0]) / w, (ys + 0.5 - jit[1]) / h
    ray = np.stack([(2 * u - 1) / cam["xs"], (1 - 2 * v) / cam["ys"], np.ones_like(u)], axis=-1)  # view space = world orientation
    depth = np.full((h, w), 6.0 - pos[2])
    X = pos + ray * depth[..., None]
    hit = rng.uniform(0.5, 12.0, (h, w))
    image_point = X + unit(X - pos) * hit[..., None]  # the mirror image of the reflected point
    p = image_point - prev_pos
    uv_prev = np.stack([p[..., 0] * cam["xs"] / p[..., 2] * 0.5 + 0.5, p[..., 1] * cam["ys"] / p[..., 2] * -0.5 + 0.5], axis=-1)
    want = (uv_prev - np.stack([u, v], axis=-1)) * (w, h)
    nr = np.zeros((h, w, 4), np.float32)
    nr[..., 2] = -1.0  # roughness 0: f = 1
    mv = rng.uniform(-2.0, 2.0, (h, w, 3)).astype(np.float32)
    tex = dict(Color=np.ones((h, w, 4), np.float32), Depth=c32(depth), MotionVector=mv, NormalRoughness=nr, DiffuseAlbedo=np.full((h, w, 3), 0.25, np.float32),
               SpecularAlbedo=np.full((h, w, 3), 0.75, np.float32), SpecularHitDistance=c32(hit))
    rr = HostReconstructor(shim)
    rr(tex, cam, (w, h), jitter=jit)
    virt = rr.rec[2]
    reach = np.maximum(1.0, np.abs(uv_prev * 2 - 1).max(axis=-1))
    err = np.abs(virt[..., :2] - want).max(axis=-1) / (reach * max(w, h))
    print(f"plane mirror: {err.max() / U:.1f} U per pixel of extent, bound {VIRT_TOL / U:.0f} U; offsets up to {np.abs(want).max():.2f} pixels")
    assert err.max() <= VIRT_TOL
    assert np.abs(want).max() > 2.0 and np.abs(want - mv[..., :2]).max() > 1.0  # the virtual motion is not small and not the surface's
    assert np.abs(virt[..., 2] - 0.75).max() <= WEIGHT_TOL  # the specular share of the albedo's luminance, f = 1
    tex["SpecularHitDistance"] = np.zeros((h, w), np.float32)
    rr(tex, cam, (w, h), jitter=jit)
    assert np.array_equal(rr.rec[2][..., :2].view(np.uint32), mv[..., :2].view(np.uint32)) and not rr.rec[2][..., 2:].any()
    # rougher than the threshold (f = 0): no weight
    tex["SpecularHitDistance"], nr[..., 3] = c32(hit), 0.4
    rr(tex, cam, (w, h), jitter=jit)
    assert not rr.rec[2][..., 2].any()


def flat_frame(rng, w, h, depth=4.0):
    nr = np.zeros((h, w, 4), np.float32)
    nr[..., 2], nr[..., 3] = -1.0, 0.5
    return dict(Color=rng.uniform(0.1, 1.0, (h, w, 4)).astype(np.float32), Depth=np.full((h, w), depth, np.float32), MotionVector=np.zeros((h, w, 3), np.float32),
                NormalRoughness=nr, DiffuseAlbedo=np.full((h, w, 3), 0.5, np.float32), SpecularAlbedo=np.full((h, w, 3), 0.1, np.float32),
                SpecularHitDistance=np.zeros((h, w), np.float32))


def kappa_of(tex, cam, out_size, jitter=(0.0, 0.0)):
    return ref.reconstruct(tex, cam, None, out_size, jitter)["kappa"]


def test_history_weight_at_rest_and_restarts(shim):
    w, h, W, H = 16, 12, 32, 24
    rng = np.random.default_rng(4)
    cam = make_camera(w, h, (0.0, 0.0, 0.0))
    rr = HostReconstructor(shim)
    total = np.zeros((H, W))
    for f in range(12):
        tex = flat_frame(rng, w, h)
        jit = jitter_of(f)
        rr(tex, cam, (W, H), jitter=jit, max_a=2.0)
        kappa = kappa_of(tex, cam, (W, H), jit)
        total = np.minimum(total + kappa, 2.0)  # A grows by kappa per frame and stops at MaxHistoryWeight
        assert np.abs(rr.history()[0][..., 3] - total).max() <= (f + 1) * T_RTOL * max(W, H), f
    assert (total == 2.0).mean() > 0.5 and kappa.min() >= 1 / 16 and kappa.max() <= 1
    tex = flat_frame(rng, w, h)
    kappa0 = kappa_of(tex, cam, (W, H))
    rr(tex, cam, (W, H))
    assert not rr.restarted and (rr.history()[0][..., 3] > kappa0 + 0.01).all()
    rr(tex, cam, (W, H), reset=True)
    assert rr.restarted and np.abs(rr.history()[0][..., 3] - kappa0).max() <= 1e-6
    rr(tex, cam, (W, H))
    assert not rr.restarted
    for size_in, size_out in (((16, 12), (48, 36)), ((12, 9), (48, 36))):  # the output size changes, then the render size
        tex = flat_frame(rng, *size_in)
        cam = make_camera(*size_in, (0.0, 0.0, 0.0))
        rr(tex, cam, size_out)
        assert rr.restarted
        assert np.abs(rr.history()[0][..., 3] - kappa_of(tex, cam, size_out)).max() <= 1e-6
        rr(tex, cam, size_out)
        assert not rr.restarted


def test_depth_step_restarts_exactly_the_disoccluded_pixels(shim):
    """a block (depth 5) that moves 3 input pixels to the right over a background (depth 10) at 2:1: the background it uncovers --
    output columns [2 a, 2 (a + 3)) of the block's rows -- has no history, every other pixel keeps its own"""
    w, h, W, H = 40, 24, 80, 48
    a, b = 10, 20
    rng = np.random.default_rng(6)
    cam = make_camera(w, h, (0.0, 0.0, 0.0))
    rr = HostReconstructor(shim)

    def frame(a, b):
        tex = flat_frame(rng, w, h, 10.0)
        tex["Depth"][4:h - 4, a:b] = 5.0
        return tex

    rr(frame(a, b), cam, (W, H))
    prev = tuple(x.copy() for x in rr.history())
    tex = frame(a + 3, b + 3)
    tex["MotionVector"][tex["Depth"] < 6.0, 0] = -3.0  # previous - current, in input pixels
    rr(tex, cam, (W, H))
    want = ref.reconstruct(tex, cam, prev, (W, H))
    restarted = np.abs(rr.history()[0][..., 3] - want["kappa"]) <= 1e-6  # A = kappa; with history it is twice that here
    assert np.array_equal(restarted, ~want["accepted"])
    expected = np.zeros((H, W), bool)
    expected[8:2 * (h - 4), 2 * a:2 * (a + 3)] = True
    assert np.array_equal(restarted, expected)
    assert np.abs(rr.history()[0][..., 3][~restarted] - 2 * want["kappa"][~restarted]).max() <= 1e-6


def test_normal_flip_at_equal_depth_is_rejected(shim):
    w, h, W, H = 20, 12, 40, 24
    rng = np.random.default_rng(7)
    cam = make_camera(w, h, (0.0, 0.0, 0.0))
    rr = HostReconstructor(shim)
    rr(flat_frame(rng, w, h), cam, (W, H))
    tex = flat_frame(rng, w, h)
    tex["NormalRoughness"][:, w // 2:, :3] = (0.0, 0.8, -0.6)  # cos = 0.6 < 0.8 against the history's normal, the depth unchanged
    kappa = kappa_of(tex, cam, (W, H))
    rr(tex, cam, (W, H))
    a = rr.history()[0][..., 3]
    assert np.abs(a[:, W // 2:] - kappa[:, W // 2:]).max() <= 1e-6  # restarted
    assert np.abs(a[:, :W // 2] - 2 * kappa[:, :W // 2]).max() <= 1e-6  # kept
    rr(tex, cam, (W, H))
    assert np.abs(rr.history()[0][..., 3][:, W // 2:] - 2 * kappa[:, W // 2:]).max() <= 1e-6  # the new normal's history is accepted


QUALITY_IN, QUALITY_OUT = (96, 64), (192, 128)


def smooth_albedo(x, y, size):
    """an albedo texture at output-pixel coordinates: three slow waves per channel, within [0.2, 0.9]"""
    W, H = size
    return np.stack([0.55 + 0.35 * np.sin(2 * np.pi * (x / W * k + y / H * (4 - k)) + k) for k in (1, 2, 3)], axis=-1)


def test_quality_against_the_upscaler_on_noisy_input(shim, up_shim):
    """A jittered band-limited pattern (test_upscale.py's) times an albedo texture, times seeded noise uniform in [0, 2) per pixel and
    frame, at 2:1.  The yardstick is pt_upscale's header on the same Color, Depth and motion: the stand-in's RMSE against the noise-free
    truth at output resolution is below it at frame 0 and at frame 16.  Measured on the CPU: see DESIGN.md section 10, row N15."""
    (w, h), (W, H) = QUALITY_IN, QUALITY_OUT
    oy, ox = np.mgrid[0:H, 0:W]
    truth = pattern(ox + 0.5, oy + 0.5, (W, H))[..., None] * smooth_albedo(ox + 0.5, oy + 0.5, (W, H))
    iy, ix = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(16)
    cam = make_camera(w, h, (0.0, 0.0, 0.0))
    rr, upscaler = HostReconstructor(shim), HostUpscaler(up_shim)
    nr = np.zeros((h, w, 4), np.float32)
    nr[..., 2], nr[..., 3] = -1.0, 0.5
    errs = {"rr": [], "up": []}
    for f in range(17):
        jit = jitter_of(f)
        sx, sy = (ix + 0.5 - jit[0]) * 2.0, (iy + 0.5 - jit[1]) * 2.0  # point samples at i + 0.5 - Jitter
        albedo = smooth_albedo(sx, sy, (W, H))
        noise = rng.uniform(0.0, 2.0, (h, w, 1))
        color = np.concatenate([pattern(sx, sy, (W, H))[..., None] * albedo * noise, np.ones((h, w, 1))], axis=-1)
        tex = dict(Color=color, Depth=np.full((h, w), 5.0), MotionVector=np.zeros((h, w, 3)), NormalRoughness=nr, DiffuseAlbedo=0.8 * albedo,
                   SpecularAlbedo=0.2 * albedo, SpecularHitDistance=np.zeros((h, w)))
        a = rr(tex, cam, (W, H), jitter=jit)
        b = upscaler(color, tex["Depth"], tex["MotionVector"], (W, H), jitter=jit)
        errs["rr"].append(float(np.sqrt(((a[..., :3] - truth) ** 2).mean())))
        errs["up"].append(float(np.sqrt(((b[..., :3] - truth) ** 2).mean())))
    print(f"quality: frame 0 {errs['rr'][0]:.5f} against {errs['up'][0]:.5f} (ratio {errs['rr'][0] / errs['up'][0]:.4f}), "
          f"frame 16 {errs['rr'][16]:.5f} against {errs['up'][16]:.5f} (ratio {errs['rr'][16] / errs['up'][16]:.4f})")
    assert errs["rr"][0] < errs["up"][0], errs
    assert errs["rr"][16] < errs["up"][16], errs


def test_sanitizers_stand_alone(tmp_path):
    """tests/cpp/rr_sanitize.cpp under ASan + UBSan as a plain executable"""
    exe = str(tmp_path / "rr_sanitize")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    os.path.join(HERE, "cpp", "rr_sanitize.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "rr_sanitize ok" in res.stdout, res.stdout + res.stderr


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import RAY_RECONSTRUCTION_TEXTURES, PtRayReconstructionSettings, PtRayReconstructionTextures
    lib = dxrs.load_hip().lib
    S = PtRayReconstructionSettings
    assert C.sizeof(S) == 240 and C.sizeof(PtRayReconstructionTextures) == 64
    assert (S.RenderSize.offset, S.OutputSize.offset, S.Jitter.offset, S.Reset.offset, S.MaxHistoryWeight.offset, S.Position.offset,
            S.ProjectionToView.offset, S.ViewToWorld.offset, S.PreviousWorldToProjection.offset) == (0, 8, 16, 24, 28, 32, 48, 112, 176)
    assert [getattr(PtRayReconstructionTextures, n).offset for n in RAY_RECONSTRUCTION_TEXTURES] == [8 * i for i in range(8)]
    assert RAY_RECONSTRUCTION_TEXTURES == TEXTURES + ("Output",)
    s = S(RenderSize=(C.c_uint32 * 2)(32, 32), OutputSize=(C.c_uint32 * 2)(64, 64))
    assert lib.pt_ray_reconstruction(None, C.byref(s), C.byref(PtRayReconstructionTextures())) == 1
    assert lib.pt_ray_reconstruction(None, None, None) == 1
    assert lib.pt_ray_reconstruction_history(None, None, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def camera_struct(dxrs, cam, jitter=(0.0, 0.0)):
    """the PtCamera that carries make_camera's fields (PtCamera.Jitter = -Settings.Jitter)"""
    c = dxrs.types.PtCamera()
    for k in range(3):
        c.Position[k] = float(cam["Position"][k])
    c.Jitter[0], c.Jitter[1] = -jitter[0], -jitter[1]
    for index, name in ((2, "PreviousWorldToProjection"), (6, "ProjectionToView"), (7, "ViewToWorld")):
        for k in range(16):
            c.Matrices[index][k] = float(cam[name][k])
    return c


class GpuReconstructor:
    """pt_ray_reconstruction on device copies; Output starts as the sentinel and sits between two guard bands that must stay the sentinel"""

    def __init__(self, dxrs, renderer):
        self.dxrs, self.r, self.out_size = dxrs, renderer, None

    def __call__(self, tex, cam, out_size, jitter=(0.0, 0.0), reset=False, max_a=0.0):
        import torch
        W, H = out_size
        h, w = np.asarray(tex["Depth"]).shape
        d = {k: torch.from_numpy(c32(tex[k])).cuda() for k in TEXTURES}
        out = torch.from_numpy(np.full((H * W + 2 * GUARD, 4), SENTINEL, np.float32)).cuda()
        torch.cuda.synchronize()
        self.r.ray_reconstruction_device((w, h), (W, H), dict({k: v.data_ptr() for k, v in d.items()}, Output=out.data_ptr() + 16 * GUARD),
                                         camera_struct(self.dxrs, cam, jitter), jitter=jitter, reset=reset, max_history_weight=max_a)
        self.r.synchronize()
        self.out_size = (W, H)
        res = out.cpu().numpy()
        for band in (res[:GUARD], res[GUARD + H * W:]):
            assert np.array_equal(band.view(np.uint32), np.full(band.shape, SENTINEL).view(np.uint32)), "the guard band was written"
        return res[GUARD:GUARD + H * W].reshape(H, W, 4)

    def history(self):
        return self.r.ray_reconstruction_history(self.out_size)


def compare_sequence(dxrs, renderer, shim, frames, what):
    """the frames (tex, cam, out_size, jitter, reset) through the GPU and the host header -> output and history bit for bit"""
    gpu, host = GpuReconstructor(dxrs, renderer), HostReconstructor(shim)
    restarts = []
    for f, (tex, cam, out_size, jit, reset) in enumerate(frames):
        reset = True if f == 0 else reset  # (the shared context carries other tests' history)
        got = gpu(tex, cam, out_size, jitter=jit, reset=reset, max_a=3.0)
        want = host(tex, cam, out_size, jitter=jit, reset=reset, max_a=3.0)
        bits_equal(got, want, f"{what} frame {f}: Output")
        for name, a, b in zip(("history", "normal", "depth"), gpu.history(), host.history()):
            bits_equal(a, b, f"{what} frame {f}: {name}")
        assert not np.array_equal(got.view(np.uint32), np.full(got.shape, SENTINEL).view(np.uint32))
        restarts.append(host.restarted)
    return restarts


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", SIZES)
def test_gpu_bit_exact_random_sequences(dxrs, renderer, shim, sizes):
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(w + 3 * h + 5 * W)
    scene = random_scene(rng, w, h)
    frames = [(random_frame(rng, scene), travelling_camera(w, h, f), (W, H), jitter_of(f), False) for f in range(4)]
    compare_sequence(dxrs, renderer, shim, frames, f"{w}x{h} -> {W}x{H}")


@pytest.mark.gpu
def test_gpu_motion_reset_and_size_change(dxrs, renderer, shim):
    """70x20 -> 140x40 with motion; a Reset in the middle, then the output size changes, then the render size"""
    rng = np.random.default_rng(12)
    plan = [((70, 20), (140, 40), False), ((70, 20), (140, 40), False), ((70, 20), (140, 40), True), ((70, 20), (140, 40), False),
            ((70, 20), (105, 30), False), ((70, 20), (105, 30), False), ((53, 15), (105, 30), False), ((53, 15), (105, 30), False)]
    scenes, frames = {}, []
    for f, ((w, h), out_size, reset) in enumerate(plan):
        scenes.setdefault((w, h), random_scene(rng, w, h))
        frames.append((random_frame(rng, scenes[(w, h)]), travelling_camera(w, h, f), out_size, jitter_of(f), reset))
    assert compare_sequence(dxrs, renderer, shim, frames, "restart rules") == [True, False, True, False, True, False, True, False]


def chain_buffers(torch, w, h, W, H):
    widths = dict(Color=4, Depth=1, MotionVector=3, NormalRoughness=4, DiffuseAlbedo=3, SpecularAlbedo=3, SpecularHitDistance=1)
    b = {k: torch.zeros((h, w, n), dtype=torch.float32, device="cuda") for k, n in widths.items()}
    b["Output"] = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    return b


def chain_frame(dxrs, host, r, b, f, w, h, W, H, prev_cam):
    """frame f of the travelling camera: pt_render_gbuffer -> pt_render_denoiser mode 1 -> pt_ray_reconstruction, all queued.  The caller
    clears SpecularHitDistance, as the reference's host does -- after the call that read it: with frames in flight a lane's frame is
    ordered after what the stream held n_lanes - 1 render calls earlier, not after what is queued just before it"""
    cam = host.camera_matrices(w, h, position=(0.15 * f, 0.05 * f, -15.0 + 0.1 * f), look_at=(0.0, 0.0, 0.0), jitter_index=f, jitter_count=32, previous=prev_cam)
    r.set_camera(cam)
    r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
    r.render_gbuffer_device(dict(LinearDepth=b["Depth"].data_ptr(), MotionVector=b["MotionVector"].data_ptr(), NormalRoughness=b["NormalRoughness"].data_ptr(),
                                 DiffuseAlbedo=b["DiffuseAlbedo"].data_ptr(), SpecularAlbedo=b["SpecularAlbedo"].data_ptr()))
    r.render_denoiser_device(dxrs.types.DENOISER_DLSS_RR, b["Color"].data_ptr(), dict(SpecularHitDistance=b["SpecularHitDistance"].data_ptr()))
    r.ray_reconstruction_device((w, h), (W, H), {k: v.data_ptr() for k, v in b.items()}, cam, reset=f == 0)
    return cam


@pytest.mark.gpu
def test_gpu_real_chain_bit_exact(dxrs, host, shim):
    """the demo scene (C2's) at 192x108 -> 384x216, 4 frames of a travelling camera: one frame at a time against the host header fed
    the inputs the device made, then the same frames with two in flight against the first run"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h, W, H, frames = 192, 108, 384, 216, 4
    results = {}
    for lanes in (1, 2):
        tstream = torch.cuda.Stream()
        r = dxrs.Renderer(device=0, stream=tstream.cuda_stream, frames_in_flight=lanes)
        try:
            with torch.cuda.stream(tstream):
                r.set_scene(spheres, mats, sd)
                sets = [chain_buffers(torch, w, h, W, H) for _ in range(lanes)]
                hr = HostReconstructor(shim)
                outs, prev_cam = [], None
                for f in range(frames):
                    b = sets[f % lanes]
                    prev_cam = cam = chain_frame(dxrs, host, r, b, f, w, h, W, H, prev_cam)
                    if lanes == 1:
                        r.synchronize()
                        tex = {k: b[k].cpu().numpy().reshape((h, w) if b[k].shape[2] == 1 else b[k].shape) for k in TEXTURES}
                        got = b["Output"].cpu().numpy()
                        fields = dict(Position=c32(list(cam.Position)), ProjectionToView=c32(list(cam.Matrices[6])), ViewToWorld=c32(list(cam.Matrices[7])),
                                      PreviousWorldToProjection=c32(list(cam.Matrices[2])))
                        want = hr(tex, fields, (W, H), jitter=(-cam.Jitter[0], -cam.Jitter[1]))
                        bits_equal(got, want, f"chain frame {f}: Output")
                        for name, x, y in zip(("history", "normal", "depth"), r.ray_reconstruction_history((W, H)), hr.history()):
                            bits_equal(x, y, f"chain frame {f}: {name}")
                        outs.append(got.copy())
                        b["SpecularHitDistance"].zero_()
                        if f:
                            assert np.abs(tex["MotionVector"][np.isfinite(tex["Depth"])][:, :2]).max() > 0.1
                            assert (hr.rec[2][..., 2] > 0).any()  # some pixels carry a virtual motion
                    else:
                        b["SpecularHitDistance"].zero_()  # (on the context's stream: after the call above, before the set's next frame)
                        if f % lanes == lanes - 1:
                            r.synchronize()
                            outs += [sets[k]["Output"].cpu().numpy().copy() for k in range(lanes)]
                r.synchronize()
                results[lanes] = outs
                if lanes == 1:
                    assert hr.history()[0][..., 3].max() > 1.0 and np.isfinite(tex["Depth"]).mean() > 0.02
        finally:
            r.close()
    for f in range(frames):
        bits_equal(results[2][f], results[1][f], f"frame {f}: two frames in flight and one")


@pytest.mark.gpu
def test_gpu_all_miss_is_pt_upscale(dxrs, renderer):
    import torch
    w, h, W, H = 48, 20, 96, 40
    rng = np.random.default_rng(31)
    scene = random_scene(rng, w, h)
    scene["Depth"] = np.full((h, w), np.inf, np.float32)
    gpu = GpuReconstructor(dxrs, renderer)
    for f in range(3):
        tex = random_frame(rng, scene)
        jit = jitter_of(f)
        got = gpu(tex, travelling_camera(w, h, f), (W, H), jitter=jit, reset=f == 0, max_a=4.0)
        d = [torch.from_numpy(c32(tex[k])).cuda() for k in ("Color", "Depth", "MotionVector")]
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.upscale_device((w, h), (W, H), dict(Color=d[0].data_ptr(), Depth=d[1].data_ptr(), Velocity=d[2].data_ptr(), Output=out.data_ptr()),
                                jitter=jit, reset=f == 0, max_history_weight=4.0)
        renderer.synchronize()
        bits_equal(got, out.cpu().numpy(), f"all-miss frame {f}")
    assert gpu.history()[0][..., 3].max() > 1.0


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, renderer):
    from dxrs_amd.types import RAY_RECONSTRUCTION_TEXTURES, PtRayReconstructionTextures, ray_reconstruction_settings
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    w, h, W, H = 32, 16, 64, 32
    bufs = {k: torch.zeros(4 * w * 4 * h * 4 + 8, dtype=torch.float32, device="cuda") for k in RAY_RECONSTRUCTION_TEXTURES}  # (room for the 4x case)
    p = {k: b.data_ptr() for k, b in bufs.items()}
    cam = camera_struct(dxrs, make_camera(w, h, (0.0, 0.0, 0.0)))

    def call(size_in=(w, h), size_out=(W, H), jitter=(0.0, 0.0), max_a=0.0, poke=None, **over):
        s = ray_reconstruction_settings(size_in, size_out, cam, jitter, True, max_a)
        if poke:
            getattr(s, poke[0])[poke[1]] = poke[2]
        t = PtRayReconstructionTextures(**{name: C.c_void_p(over.get(name, p[name])) for name in RAY_RECONSTRUCTION_TEXTURES})
        return lib.pt_ray_reconstruction(ctx, C.byref(s), C.byref(t))

    s = ray_reconstruction_settings((w, h), (W, H), cam)
    assert lib.pt_ray_reconstruction(None, None, None) == 1
    assert lib.pt_ray_reconstruction(ctx, None, C.byref(PtRayReconstructionTextures())) == 1 and lib.pt_ray_reconstruction(ctx, C.byref(s), None) == 1
    for size_in in ((0, h), (w, 0), (16385, h), (w, 16385)):
        assert call(size_in=size_in, size_out=size_in) == 1, size_in
    for size_out in ((w - 1, H), (W, h - 1), (4 * w + 1, H), (W, 4 * h + 1), (0, 0)):
        assert call(size_out=size_out) == 1, size_out
    assert call(size_in=(8192, 1), size_out=(16385, 1)) == 1
    assert call(size_out=(w, h)) == 0 and call(size_out=(4 * w, 4 * h)) == 0
    for jitter in ((np.nan, 0.0), (0.0, np.inf), (1.5, 0.0), (0.0, -1.0001)):
        assert call(jitter=jitter) == 1, jitter
    assert call(jitter=(1.0, -1.0)) == 0
    for max_a in (np.nan, np.inf, -1.0, 0.5, 256.5):
        assert call(max_a=max_a) == 1, max_a
    assert call(max_a=1.0) == 0 and call(max_a=256.0) == 0
    for field, index in (("Position", 1), ("ProjectionToView", 0), ("ProjectionToView", 15), ("ViewToWorld", 7), ("PreviousWorldToProjection", 12)):
        for value in (np.nan, np.inf, -np.inf):
            assert call(poke=(field, index, value)) == 1, (field, index, value)
    for name in RAY_RECONSTRUCTION_TEXTURES:
        assert call(**{name: None}) == 1, name
    for name in ("Color", "NormalRoughness", "Output"):
        assert call(**{name: p[name] + 8}) == 1, name
    for name in ("Depth", "MotionVector", "DiffuseAlbedo", "SpecularAlbedo", "SpecularHitDistance"):
        assert call(**{name: p[name] + 2}) == 1, name
        assert call(**{name: p[name] + 4}) == 0, name
    for name in TEXTURES:
        assert call(Output=p[name]) == 1, name
    two = torch.zeros(2 * W * H * 4, dtype=torch.float32, device="cuda")  # Color: w * h texels, then Output: W * H texels
    assert call(Color=two.data_ptr(), Output=two.data_ptr() + 16 * (w * h - 1)) == 1
    assert call(Color=two.data_ptr(), Output=two.data_ptr() + 16 * w * h) == 0
    assert call(Depth=p["SpecularHitDistance"]) == 0  # two inputs may share a buffer
    assert call() == 0
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, shim, tmp_path):
    """dxrs::RayReconstruction (host/RayReconstruction.hpp) from C++, against pt_api.h alone: three frames of the demo scene through
    G-buffer, pt_render_denoiser mode 1 and the stand-in, tagged and evaluated as App::ProcessDLSSRayReconstruction does, equal the
    host-compiled header fed the inputs the program downloaded; a missing tag is refused"""
    exe = str(tmp_path / "host_rr")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(PKG, "host"), os.path.join(HERE, "cpp", "host_rr.cpp"),
                    "-o", exe, "-L", PKG, "-lpt_hip", f"-Wl,-rpath,{PKG}"], check=True)
    w, h, W, H, frames = 96, 54, 192, 108, 3
    outp = str(tmp_path / "rr.f32")
    res = subprocess.run([exe, str(w), str(h), str(W), str(H), str(frames), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout
    raw = np.fromfile(outp, dtype=np.float32)
    n, N = w * h, W * H
    per = 2 + 3 + 48 + 19 * n + 4 * N
    assert raw.size == frames * per
    hr = HostReconstructor(shim)
    for f in range(frames):
        x = raw[f * per:(f + 1) * per]
        jit = (float(x[0]), float(x[1]))
        cam = dict(Position=x[2:5], ProjectionToView=x[5:21], ViewToWorld=x[21:37], PreviousWorldToProjection=x[37:53])
        o, tex = 53, {}
        for name, width in (("Color", 4), ("Depth", 1), ("MotionVector", 3), ("NormalRoughness", 4), ("DiffuseAlbedo", 3), ("SpecularAlbedo", 3),
                            ("SpecularHitDistance", 1)):
            tex[name] = x[o:o + width * n].reshape((h, w) if width == 1 else (h, w, width))
            o += width * n
        bits_equal(x[o:].reshape(H, W, 4), hr(tex, cam, (W, H), jitter=jit), f"C++ frame {f}")
        assert jit != (0.0, 0.0)
    assert hr.history()[0][..., 3].max() > 1.0
