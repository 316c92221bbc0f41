"""Row N10 -- pt_restir_di, the reservoir pass that makes the DI pt_render_with_di takes (DESIGN.md spec S16).
CPU: the host-compiled header (tests/hostshim/restir_host.cpp over csrc/pt_restir.h) pass by pass against the float64 restatement
(restir_reference.py), known answers, an unbiasedness check against a quadrature of the direct-light integral, the noise ratio against
the one-candidate estimate.  GPU: pt_restir_di against the host-compiled header bit for bit over consecutive frames (so the
reservoirs the outputs derive from are covered), the history's restart rules, the chain into pt_render_with_di, argument errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import restir_reference as ref
from test_gbuffer import grid, host_pixels, linear_textures, oracle_hits

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = ("Position", "GeometricNormal", "LinearDepth", "MotionVector", "BaseColorMetalness", "NormalRoughness", "IOR", "Transmission")
WIDTH = dict(Position=4, GeometricNormal=2, LinearDepth=1, MotionVector=3, BaseColorMetalness=4, NormalRoughness=4, IOR=1, Transmission=1)
GB_COLUMNS = dict(Position=(0, 4), GeometricNormal=(6, 8), LinearDepth=(8, 9), MotionVector=(10, 13), BaseColorMetalness=(13, 17),
                  NormalRoughness=(23, 27), IOR=(27, 28), Transmission=(28, 29))  # columns of gbuffer_host.cpp's 32 floats per pixel
GB_BIT = dict(Position=1 << 0, GeometricNormal=1 << 2, LinearDepth=1 << 3, MotionVector=1 << 5, BaseColorMetalness=1 << 6, NormalRoughness=1 << 9,
              IOR=1 << 10, Transmission=1 << 11)
OFF, BASIC, PAIRWISE, RAYTRACED = 0, 1, 2, 3
SENTINEL = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]


# ---------------------------------------------------------------------------------------------------- the host-compiled header
@pytest.fixture(scope="module")
def shims():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_restir_shim())
    vp, u32 = C.c_void_p, C.c_uint32
    lib.ri_host_call.restype = None
    lib.ri_host_call.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp]
    gb = C.CDLL(g.build_gbuffer_shim())
    gb.gb_pixels.restype = None
    gb.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    gb.gb_srgb_lut.restype = None
    gb.gb_srgb_lut.argtypes = [vp]
    return lib, gb


def settings(**kw):
    """pt_restir_di's settings with its defaults applied (PtRestirDiSettings: 0 -> default)"""
    s = dict(frame_index=0, reset_history=False, initial_samples=8, temporal=True, temporal_bias=BASIC, max_history=20, spatial=True,
             spatial_bias=BASIC, spatial_samples=1, spatial_radius=32.0)
    s.update(kw)
    return s


class HostPass:
    """pt_restir_di over the host-compiled header: the two history slots and the restart rules of the entry point"""

    def __init__(self, lib, gbshim, spheres, mats, textures=None):
        self.lib, self.spheres, self.mats = lib, np.ascontiguousarray(spheres), np.ascontiguousarray(mats)
        self.texels, self.info = linear_textures(gbshim, textures)
        self.maps = self.rot = None
        if self.texels is not None:
            maps = np.zeros((len(spheres), 8), np.uint32)
            maps[:, :7] = textures.maps
            maps[:, 7] = (textures.maps != 0xFFFFFFFF).any(axis=1)
            self.maps = np.ascontiguousarray(maps)
            self.rot = np.ascontiguousarray(textures.rotations, dtype=np.float32)
        self.size, self.valid, self.cur = None, False, 0

    def slot(self, k):
        return self.slots[k]

    def call(self, gb, w, h, cam, out_d, out_s, launches=3, **kw):
        s = settings(**kw)
        n = w * h
        if self.size != (w, h):
            self.slots = [[np.zeros((n, 4), np.float32) for _ in range(4)] + [np.zeros(n, np.float32)] + [np.zeros((n, 4), np.float32) for _ in range(2)]
                          for _ in range(2)]
            self.size, self.valid = (w, h), False
        restart = s["reset_history"] or not self.valid
        cur, prev = self.cur ^ 1, self.cur
        if launches == 4:  # the spatial pass alone, over the slot the last call wrote: nothing advances
            cur, prev = self.cur, self.cur ^ 1
        prm = np.array([w, h, s["frame_index"], s["initial_samples"], int(s["temporal"]), s["temporal_bias"], s["max_history"], int(s["spatial"]),
                        s["spatial_bias"], s["spatial_samples"], 0 if restart else 1, launches], np.uint32)
        fprm = np.array([s["spatial_radius"], *cam.Position, *cam.PreviousPosition], np.float32)
        arrays = [np.ascontiguousarray(gb[name], dtype=np.float32) for name in INPUTS] + self.slots[cur] + self.slots[prev] + [out_d, out_s]
        ptrs = (C.c_void_p * 24)(*[a.ctypes.data for a in arrays])
        p = lambda a: a.ctypes.data if a is not None else None
        self.lib.ri_host_call(p(self.spheres), p(self.mats), len(self.spheres), p(self.texels), p(self.info), 0 if self.info is None else len(self.info),
                              p(self.maps), p(self.rot), p(prm), p(fprm), ptrs)
        if launches != 4:
            self.cur, self.valid = cur, True
        return self.slots[cur]

    def frame(self, gb, w, h, cam, **kw):
        out_d, out_s = (np.full((w * h, 4), SENTINEL, np.float32) for _ in range(2))
        self.call(gb, w, h, cam, out_d, out_s, **kw)
        return out_d, out_s


def reservoirs(slot):
    """the reservoir planes of a slot -> dicts, as restir_reference holds them"""
    a, c = slot[5], slot[6]
    return [dict(light=int(a[i, 0:1].view(np.uint32)[0]), u1=float(a[i, 1]), u2=float(a[i, 2]), W=float(a[i, 3]), M=float(c[i, 0]), p_hat=float(c[i, 1]),
                 age=int(c[i, 2:3].view(np.uint32)[0])) for i in range(len(a))]


# ---------------------------------------------------------------------------------------------------- the CPU scene
W, H = 48, 32
GROUND, E0, E1, E2, BLOCKER, MASKED, MIRROR = range(7)


def make_scene(dxrs, emitters=(E0, E1, E2), blockers=True):
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(7, SPHERE_DTYPE)
    spheres[GROUND] = (0.0, -1000.0, 0.0, 1000.0)
    spheres[E0] = (-3.0, 3.0, 0.5, 0.5)
    spheres[E1] = (3.0, 2.0, 1.0, 0.25)
    spheres[E2] = (0.5, 5.0, 3.0, 1.0)
    spheres[BLOCKER] = (-1.5, 1.0, 0.0, 0.8) if blockers else (-1.5, -50.0, 0.0, 0.8)
    spheres[MASKED] = (1.8, 1.2, 0.8, 0.5)
    spheres[MIRROR] = (1.2, 0.7, -1.5, 0.7)
    mats = default_material(7)
    mats["BaseColor"][:, :3] = [(0.6, 0.55, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0.7, 0.2, 0.2), (0.2, 0.7, 0.2), (0.9, 0.9, 0.9)]
    mats["Roughness"] = [0.6, 0.5, 0.5, 0.5, 0.35, 0.5, 0.02]
    mats["Metallic"] = [0.0, 0, 0, 0, 0.5, 0.0, 1.0]
    for e, colour, strength in ((E0, (1.0, 0.9, 0.8), 20.0), (E1, (1.0, 0.5, 0.2), 60.0), (E2, (0.4, 0.6, 1.0), 5.0)):
        if e in emitters:
            mats["EmissiveColor"][e] = colour
            mats["EmissiveStrength"][e] = strength
    mats["AlphaMode"][MASKED] = 1      # Mask below the cutoff: the sphere does not exist for rays, visibility rays included
    mats["BaseColor"][MASKED, 3] = 0.25
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.1, 0.1, 0.1, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    return spheres, mats, sd


def cpu_gbuffer(shims, oracle, cam, w, h, spheres, mats, sd):
    """the G-buffer pt_render_gbuffer writes (the host-compiled pt_gbuffer.h over the oracle's hits); unwritten channels hold 0"""
    px, py = grid(0, 0, w, h)
    t, ids = oracle_hits(oracle, cam, w, h, spheres, px, py, materials=mats)
    vals, mask = host_pixels(shims[1], cam, w, h, spheres, mats, sd, px, py, t, ids)
    gb = {}
    for name in INPUTS:
        a, b = GB_COLUMNS[name]
        gb[name] = np.where(((mask & GB_BIT[name]) != 0)[:, None], vals[:, a:b], 0.0).astype(np.float32)
    return gb, ids


@pytest.fixture(scope="module")
def cpu_case(dxrs, host, oracle, shims):
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(W, H, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gb, ids = cpu_gbuffer(shims, oracle, cam, W, H, spheres, mats, sd)
    assert (ids == 0xFFFFFFFF).any() and (ids == MIRROR).any() and (ids == GROUND).any() and (ids == BLOCKER).any()
    return spheres, mats, sd, cam, gb, ids


# ---------------------------------------------------------------------------------------------------- CPU: ABI
def test_restir_di_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_restir_di") and "pt_restir_di" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtRestirDiSettings, PtRestirDiTextures
    assert C.sizeof(PtRestirDiSettings) == 48 and PtRestirDiSettings.ResetHistory.offset == 12 and PtRestirDiSettings.SpatialRadius.offset == 44
    assert PtRestirDiSettings.TemporalBiasCorrection.offset == 24 and PtRestirDiSettings.EnableSpatial.offset == 32
    assert C.sizeof(PtRestirDiTextures) == 80
    s, t = PtRestirDiSettings(), PtRestirDiTextures()
    assert lib.pt_restir_di(None, C.byref(s), C.byref(t)) == 1  # PT_ERR_INVALID_ARG: null context


# ---------------------------------------------------------------------------------------------------- CPU: pass by pass
# Continuous values: a reservoir's W and p_hat and an output pixel are sums of at most 8 + 2 target-function values, each a chain of
# about 60 float32 operations (cone sample, two BSDF lobes, luminance), against their float64 values: 64 * 2^-24 per value, times 4 for the
# cancellation in (1 - cos) terms near grazing directions the BSDF's Fresnel and geometry terms amplify.
PASS_RTOL = 4 * 64 * 2.0 ** -24
# Discrete choices may differ where a float32 comparison sits within rounding of its threshold (the RIS draw against w / w_sum, the
# depth and normal tests): at most this share of the pixels, counted below.
MAX_FLIPPED_SHARE = 0.01
# a comparison of the restatement counts as near its threshold when its relative margin is below this (PASS_RTOL, the error the two
# sides of a float32 comparison can carry): only such a pixel's pick may differ, and the seeds are chosen so that few are
NEAR = 4 * 64 * 2.0 ** -24


def close(a, b):
    return abs(a - b) <= PASS_RTOL * max(abs(a), abs(b)) + 1e-12


def test_header_matches_float64_restatement_pass_by_pass(shims, cpu_case):
    spheres, mats, sd, cam, gb, ids = cpu_case
    scene = ref.Scene(spheres, mats)
    n = W * H
    cam_pos, prev_pos = tuple(cam.Position), tuple(cam.PreviousPosition)
    surf_cache = {}

    def surfaces(i, pos):
        if (i, pos) not in surf_cache:
            surf_cache[(i, pos)] = ref.surface(gb, i, pos)
        return surf_cache[(i, pos)]

    hp = HostPass(*shims, spheres, mats)
    flipped = near = 0
    # frame 0: initial sampling alone (no history, spatial off)
    slot0 = hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, frame_index=0, spatial=False)
    got0 = reservoirs(slot0)
    want0 = []
    for i in range(n):
        s = surfaces(i, cam_pos)
        margins = []
        r = ref.initial(scene, s, i % W, i // W, 0, 8, margins) if s is not None else ref.empty_reservoir()
        near0 = bool(margins) and min(margins) < NEAR
        near += near0
        want0.append(r)
        g = got0[i]
        assert (g["M"] > 0) == (s is not None), f"pixel {i}: surface validity"
        if s is None:
            continue
        if (g["light"], g["u1"], g["u2"]) != (r["light"], np.float32(r["u1"]), np.float32(r["u2"])) or (g["W"] > 0) != (r["W"] > 0):
            assert near0, f"pixel {i}: the initial pick differs away from every threshold: {g} != {r}"
            flipped += 1
            want0[i] = g  # the later frames are compared from the header's own choice
            continue
        assert g["M"] == r["M"] and close(g["W"], r["W"]) and close(g["p_hat"], r["p_hat"]), (i, g, r)
    valid = sum(1 for i in range(n) if surfaces(i, cam_pos) is not None)
    assert valid > n // 3 and sum(1 for r in want0 if r["W"] > 0) > valid // 4
    assert not any(surfaces(i, cam_pos) is not None for i in range(n) if ids[i] in (MIRROR, 0xFFFFFFFF)), "mirror-like pixels and misses have no surface"
    # frame 1: temporal (Raytraced) over frame 0's slot, then spatial (Basic, 3 neighbours) and final shading
    out_d, out_s = (np.full((n, 4), SENTINEL, np.float32) for _ in range(2))
    slot1 = hp.call(gb, W, H, cam, out_d, out_s, frame_index=1, temporal_bias=RAYTRACED, spatial_samples=3, spatial_radius=6.0)
    got1 = reservoirs(slot1)
    want1, accepted = [], 0
    for i in range(n):
        s = surfaces(i, cam_pos)
        if s is None:
            want1.append(ref.empty_reservoir())
            continue
        margins = []
        cur = ref.initial(scene, s, i % W, i // W, 1, 8, margins)
        r, acc = ref.temporal(scene, s, cur, (surfaces, want0), i % W, i // W, W, H, tuple(float(x) for x in gb["MotionVector"][i]), 1, RAYTRACED, 20, prev_pos,
                              margins)
        accepted += acc
        near1 = bool(margins) and min(margins) < NEAR
        near += near1
        g = got1[i]
        if (g["light"], g["u1"], g["u2"], g["M"]) != (r["light"], np.float32(r["u1"]), np.float32(r["u2"]), r["M"]) or (g["W"] > 0) != (r["W"] > 0):
            assert near1, f"pixel {i}: the temporal pick differs away from every threshold: {g} != {r}"
            flipped += 1
            r = g
        else:
            assert close(g["W"], r["W"]) and close(g["p_hat"], r["p_hat"]) and g["age"] == r["age"], (i, g, r)
        want1.append(r)
    assert accepted == valid, "a resting view reprojects every surface onto itself"
    # the spatial pass alone: the reservoir it hands to final shading, pick by pick
    sp_a, sp_c = (np.zeros((n, 4), np.float32) for _ in range(2))
    hp.call(gb, W, H, cam, sp_a, sp_c, launches=4, frame_index=1, temporal_bias=RAYTRACED, spatial_samples=3, spatial_radius=6.0)
    got_sp = reservoirs([None] * 5 + [sp_a, sp_c])
    written = reused = 0
    for i in range(n):
        s = surfaces(i, cam_pos)
        is_written = out_d[i, 0:1].view(np.uint32)[0] != SENTINEL.view(np.uint32)
        if s is None:
            assert not is_written and out_s[i, 0:1].view(np.uint32)[0] == SENTINEL.view(np.uint32)
            continue
        r, acc = ref.spatial(scene, s, want1[i], surfaces, want1, i % W, i // W, W, H, 1, BASIC, 3, 6.0, cam_pos)
        reused += bool(acc)
        g = got_sp[i]
        if (g["light"], g["u1"], g["u2"], g["M"]) != (r["light"], np.float32(r["u1"]), np.float32(r["u2"]), r["M"]) or (g["W"] > 0) != (r["W"] > 0):
            flipped += 1  # (a different spatial pick or neighbour set: a discrete choice, counted)
            continue
        assert close(g["W"], r["W"]) and close(g["p_hat"], r["p_hat"]) and g["age"] == r["age"], (i, g, r)
        f = ref.final(scene, s, r)   # the picks agree: every value of the pixel is held to the tolerance
        assert (f is not None) == is_written, (i, g, r)
        if f is None:
            continue
        written += 1
        for c in range(3):
            assert close(out_d[i, c], f[0][c]) and close(out_s[i, c], f[1][c]), (i, out_d[i], f)
        assert abs(out_d[i, 3] - f[2]) <= 1e-4 * f[2] and out_s[i, 3] == out_d[i, 3]
    assert written > valid // 4 and reused > valid // 4
    print(f"flipped discrete choices: {flipped} of {3 * valid} ({flipped / (3 * valid):.4f}); near a threshold in the restatement alone: {near} of {2 * valid}")
    assert near <= MAX_FLIPPED_SHARE * 2 * valid, "the seeds (FrameIndex 0 and 1) put too many of the restatement's own comparisons near their thresholds"
    assert flipped <= MAX_FLIPPED_SHARE * 3 * valid, flipped


# ---------------------------------------------------------------------------------------------------- CPU: known answers
def test_one_candidate_without_reuse_is_n4s_formula(shims, cpu_case):
    """InitialSamples = 1, no reuse: a written pixel holds Le f inv_pdf n_lights of the drawn sample"""
    spheres, mats, sd, cam, gb, ids = cpu_case
    scene = ref.Scene(spheres, mats)
    hp = HostPass(*shims, spheres, mats)
    out_d, out_s = hp.frame(gb, W, H, cam, frame_index=5, initial_samples=1, temporal=False, spatial=False)
    checked = 0
    for i in range(W * H):
        s = ref.surface(gb, i, tuple(cam.Position))
        written = out_d[i, 0:1].view(np.uint32)[0] != SENTINEL.view(np.uint32)
        if s is None:
            assert not written
            continue
        rng = ref.it.Stream(ref.it.rng_seed(i % W, i // W, 5 ^ ref.SALT_INITIAL))
        u0, u1, u2 = rng.unit(), rng.unit(), rng.unit()
        e = ref.shade(scene, s, min(int(u0 * 3), 2), u1, u2)
        lit = e["p_hat"] > 0 and ref.visible(scene, s, e)[0]
        assert written == lit, i
        if lit:
            k = e["inv_pdf"] * 3
            for c in range(3):
                assert close(out_d[i, c], e["le"][c] * e["f_d"][c] * k) and close(out_s[i, c], e["le"][c] * e["f_s"][c] * k)
            checked += 1
    assert checked > 100


def test_single_emitter_closed_form_and_occlusion(dxrs, host, oracle, shims):
    """one emitter: W after the initial pass is (sum of the candidates' p_hat) / (M p_hat_selected) -- 1 / p_hat_selected times the mean;
    with one candidate exactly 1 (n_lights = 1).  Behind the blocker the selected sample is occluded: W = 0, M kept."""
    spheres, mats, sd = make_scene(dxrs, emitters=(E0,))
    cam = host.camera_matrices(W, H, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gb, ids = cpu_gbuffer(shims, oracle, cam, W, H, spheres, mats, sd)
    scene = ref.Scene(spheres, mats)
    hp = HostPass(*shims, spheres, mats)
    n = W * H
    one = reservoirs(hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, initial_samples=1, spatial=False))
    eight = reservoirs(hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, initial_samples=8, spatial=False,
                               reset_history=True, frame_index=3))
    occluded = lit = 0
    for i in range(n):
        s = ref.surface(gb, i, tuple(cam.Position))
        if s is None:
            assert one[i]["M"] == 0 and eight[i]["M"] == 0 and eight[i]["W"] == 0
            continue
        assert one[i]["M"] == 1 and eight[i]["M"] == 8
        if one[i]["W"] > 0:
            assert abs(one[i]["W"] - 1.0) <= 2.0 ** -22
        r = eight[i]
        if r["p_hat"] > 0:
            e = ref.shade(scene, s, r["light"], r["u1"], r["u2"])
            if ref.visible(scene, s, e)[0]:
                rng = ref.it.Stream(ref.it.rng_seed(i % W, i // W, 3 ^ ref.SALT_INITIAL))
                total = 0.0
                for _ in range(8):
                    u0, u1, u2, _rnd = rng.unit(), rng.unit(), rng.unit(), rng.unit()
                    total += ref.shade(scene, s, 0, u1, u2)["p_hat"]
                assert close(r["W"], total / (8 * e["p_hat"])), (i, r)
                lit += 1
            else:
                assert r["W"] == 0.0 and r["M"] == 8
                occluded += 1
    assert lit > 100 and occluded > 5


def test_m_cap_holds_after_100_frames(shims, cpu_case):
    spheres, mats, sd, cam, gb, ids = cpu_case
    w, h = 16, 8  # a corner of the frame's buffers is a frame of its own: the pass reads nothing but its inputs
    rows = np.arange(h)[:, None] * W + np.arange(w)[None, :] + (H - h) * W + 16
    sub = {name: np.ascontiguousarray(gb[name][rows.ravel()]) for name in INPUTS}
    hp = HostPass(*shims, spheres, mats)
    for f in range(100):
        out_d, out_s = hp.frame(sub, w, h, cam, frame_index=f, initial_samples=4, max_history=5)
    res = reservoirs(hp.slot(hp.cur))
    m = np.array([r["M"] for r in res])
    assert m.max() == 4 * (1 + 5) and (m[m > 0] >= 4).all()
    assert max(r["age"] for r in res) >= 1


# ---------------------------------------------------------------------------------------------------- CPU: unbiasedness and noise
F_FRAMES, HISTORY = 160, 8   # F frames, batches of MaxHistoryLength frames


@pytest.fixture(scope="module")
def statistics(dxrs, host, oracle, shims):
    """per-frame images of DI = Diffuse.rgb + Specular.rgb (luminance) over a static 24 x 16 view, for the Raytraced configuration with
    the history running, the defaults, and the one-candidate control; and the quadrature"""
    w, h = 24, 16
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gb, ids = cpu_gbuffer(shims, oracle, cam, w, h, spheres, mats, sd)
    scene = ref.Scene(spheres, mats)
    quad = np.zeros(w * h)
    for i in range(w * h):
        s = ref.surface(gb, i, tuple(cam.Position))
        if s is not None:
            quad[i] = ref.it.lum(ref.quadrature(scene, s, k=8))
    lum = np.array([0.2126, 0.7152, 0.0722])

    def run(**kw):
        hp = HostPass(*shims, spheres, mats)
        frames = []
        for f in range(F_FRAMES):
            out_d, out_s = hp.frame(gb, w, h, cam, frame_index=f, **kw)
            img = np.where(out_d[:, :1].view(np.uint32) == SENTINEL.view(np.uint32), 0.0, (out_d[:, :3].astype(np.float64) + out_s[:, :3]))
            frames.append(img @ lum)
        return np.array(frames)
    return dict(quad=quad, raytraced=run(temporal_bias=RAYTRACED, spatial_bias=RAYTRACED, max_history=HISTORY, spatial_samples=2, spatial_radius=4.0),
                control=run(initial_samples=1, temporal=False, spatial=False), defaults=run())


def deviation(frames, quad, block):
    """(image total of mean - quadrature, its standard error from batch means over blocks of `block` frames)"""
    totals = (frames - quad[None, :]).sum(axis=1)
    batches = totals[:len(totals) // block * block].reshape(-1, block).mean(axis=1)
    return float(batches.mean()), float(batches.std(ddof=1) / math.sqrt(len(batches)))


def test_unbiased_with_raytraced_correction(statistics):
    """F = 160 frames, batches of MaxHistoryLength = 8.  Observed (image total of 384 pixels, luminance; quadrature total 17.2903):
    control deviation -0.0120 (standard error 0.1337), Raytraced deviation -0.0779 (standard error 0.0455)."""
    q = statistics["quad"]
    dev_c, se_c = deviation(statistics["control"], q, 1)
    dev_r, se_r = deviation(statistics["raytraced"], q, HISTORY)
    print(f"quadrature total {q.sum():.4f}; control dev {dev_c:+.4f} se {se_c:.4f}; raytraced dev {dev_r:+.4f} se {se_r:.4f}")
    assert abs(dev_c) <= 3 * se_c, "the control (independent one-candidate frames) fails the check itself"
    assert abs(dev_r) <= 3 * se_r


# measured on the CPU: 0.147 (single-frame RMSE against the quadrature at the defaults, frames 16..159 of a running history, over that of
# the one-candidate configuration on the same frames); the bound is halfway between it and 1
NOISE_RATIO_MEASURED = 0.147


def test_noise_ratio_against_one_candidate(statistics):
    q = statistics["quad"]
    rmse = lambda frames: math.sqrt(((frames[16:] - q[None, :]) ** 2).mean())
    ratio = rmse(statistics["defaults"]) / rmse(statistics["control"])
    print(f"RMSE ratio defaults / one candidate: {ratio:.3f}")
    assert ratio < (NOISE_RATIO_MEASURED + 1.0) / 2


# ---------------------------------------------------------------------------------------------------- GPU
def gpu_setup(r, dxrs, spheres, mats, sd, cam, w, h, textures=None, frame_index=0):
    r.set_scene(spheres, mats, sd)
    r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=frame_index, bounces=2, spp=1))


def gpu_frame(r, hp, w, h, cam, what="", **kw):
    """one pt_restir_di call (sentinel-filled outputs) against the host-compiled header fed the same G-buffer: every word bit for bit,
    unwritten pixels included"""
    dd, ds, gb = r.restir_di(fill=SENTINEL, **kw)
    gbn = {name: gb[name].cpu().numpy().reshape(w * h, -1) for name in INPUTS}
    want_d, want_s = hp.frame(gbn, w, h, cam, **kw)
    got_d, got_s = dd.cpu().numpy().reshape(-1, 4), ds.cpu().numpy().reshape(-1, 4)
    for got, want, name in ((got_d, want_d, "Diffuse"), (got_s, want_s, "Specular")):
        diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {w * h} pixels differ, first {int(np.argmax(diff))}: {got[np.argmax(diff)]} != {want[np.argmax(diff)]}"
    written = got_d[:, 0:1].view(np.uint32)[:, 0] != SENTINEL.view(np.uint32)
    return written, got_d, gbn


def demo_case(dxrs, host, w, h, **cam_kw):
    """the CPU tests' scene (a rough ground, three emitters, blockers, a mirror, sky): most pixels receive DI, unlike the demo scene's
    mirror-like ground"""
    spheres, mats, sd = make_scene(dxrs)
    return spheres, mats, sd, host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), **cam_kw)


@pytest.mark.gpu
def test_gpu_four_frames_ragged(dxrs, host, renderer, shims):
    w, h = 67, 45
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = HostPass(*shims, spheres, mats)
    lit = 0
    for f in range(4):
        written, _, _ = gpu_frame(renderer, hp, w, h, cam, f"frame {f}", frame_index=f, reset_history=f == 0, spatial_samples=3, spatial_radius=40.0)
        lit += int(written.sum())
    assert lit > 4 * w * h // 10


@pytest.mark.gpu
def test_gpu_travelling_camera(dxrs, host, renderer, shims):
    w, h = 64, 48
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    hp = HostPass(*shims, spheres, mats)
    prev = None
    renderer.set_scene(spheres, mats, sd)
    renderer.set_textures(None)
    for f in range(3):
        cam = host.camera_matrices(w, h, position=(0.4 * f, 0.1 * f, -15.0 + 0.5 * f), look_at=(0.2 * f, 0.0, 0.0), jitter_index=f, previous=prev)
        renderer.set_camera(cam)
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=2, spp=1))
        written, _, _ = gpu_frame(renderer, hp, w, h, cam, f"frame {f}", frame_index=f, reset_history=f == 0, temporal_bias=RAYTRACED)
        assert written.any(), f"frame {f}: no pixel received DI"
        if f > 0:  # reprojection was accepted for some surfaces and rejected for others: M above the initial 8 only where it was
            slot = hp.slot(hp.cur)
            m = slot[6][np.isfinite(slot[3][:, 2]), 0]
            assert (m > 8).any() and (m == 8).any(), f"frame {f}: M {np.unique(m)}"
        prev = cam


@pytest.mark.gpu
@pytest.mark.parametrize("tb,sb", [(OFF, OFF), (BASIC, RAYTRACED), (RAYTRACED, BASIC)])
def test_gpu_bias_modes(dxrs, host, renderer, shims, tb, sb):
    w, h = 64, 48
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = HostPass(*shims, spheres, mats)
    for f in range(2):
        gpu_frame(renderer, hp, w, h, cam, f"frame {f}", frame_index=f, reset_history=f == 0, temporal_bias=tb, spatial_bias=sb, spatial_samples=2)


@pytest.mark.gpu
@pytest.mark.parametrize("initial,spatial_samples,radius", [(1, 1, 0.5), (8, 4, 32.0), (32, 4, 0.5), (8, 1, 32.0)])
def test_gpu_sample_counts_and_radii(dxrs, host, renderer, shims, initial, spatial_samples, radius):
    """radius 0.5 rounds every neighbour onto the pixel itself (the API's 0 means the default radius): no spatial reuse"""
    w, h = 64, 48
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = HostPass(*shims, spheres, mats)
    for f in range(2):
        gpu_frame(renderer, hp, w, h, cam, f"frame {f}", frame_index=7 + f, reset_history=f == 0, initial_samples=initial, spatial_samples=spatial_samples,
                  spatial_radius=radius)


@pytest.mark.gpu
def test_gpu_textured_emitter_and_alpha_mapped_blocker(dxrs, host, renderer, shims):
    """the test scene with an emissive map on emitter E0 (its radiance is evaluated through EvaluateMaterial at the point a visibility
    ray reaches) and a base-colour map with holes in its alpha on the blocker under it (AlphaMode Mask: its crossings are tested)"""
    from dxrs_amd.textures import TextureSet
    w, h = 96, 64
    spheres, mats, sd = make_scene(dxrs)
    mats = mats.copy()
    mats["BaseColor"][BLOCKER, 3] = 1.0
    mats["AlphaMode"][BLOCKER] = 1
    ts = TextureSet(len(spheres))
    yy, xx = np.mgrid[0:32, 0:64]
    checker = ((xx // 4 + yy // 4) & 1).astype(np.uint8)
    glow = np.zeros((32, 64, 4), np.uint8)
    glow[..., 0], glow[..., 1], glow[..., 2], glow[..., 3] = 255, 80 + 175 * checker, 40 + 215 * checker, 255
    holes = np.full((32, 64, 4), 255, np.uint8)
    holes[..., 3] = 255 * checker
    ts.maps[E0, 1] = ts.add_image(glow)     # TEXTURE_MAP_EMISSIVE_COLOR
    ts.maps[BLOCKER, 0] = ts.add_image(holes)  # TEXTURE_MAP_BASE_COLOR
    mapped = [E0, BLOCKER]
    cam = host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h, textures=ts)
    hp = HostPass(*shims, spheres, mats, textures=ts)
    opaque = mats.copy()
    opaque["AlphaMode"][mapped[1]] = 0
    hp_opaque = HostPass(*shims, spheres, opaque, textures=ts)
    j = int(np.flatnonzero(np.flatnonzero(mats["EmissiveStrength"] * mats["EmissiveColor"].max(axis=1) > 0) == mapped[0])[0])
    from_textured = crossed = 0
    for f in range(2):
        written, got_d, gbn = gpu_frame(renderer, hp, w, h, cam, f"frame {f}", frame_index=f, reset_history=f == 0, spatial_samples=2)
        slot = hp.slot(hp.cur)
        from_textured += int((written & (slot[5][:, 0].view(np.uint32) == j) & (slot[5][:, 3] > 0)).sum())
        # the same frame with the blocker opaque: a difference means a visibility ray went through its alpha-tested crossings
        other_d, _ = hp_opaque.frame(gbn, w, h, cam, frame_index=f, reset_history=f == 0, spatial_samples=2)
        crossed += int((other_d.view(np.uint32) != got_d.view(np.uint32)).any(axis=1).sum())
    renderer.set_textures(None)
    assert from_textured > 0, "no written pixel holds a sample of the textured emitter"
    assert crossed > 0, "no visibility ray met the alpha-mapped blocker"


@pytest.mark.gpu
def test_gpu_scene_in_global_memory(dxrs, host, shims):
    w, h = 64, 48
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=100000)
    mats = mats.copy()
    big = np.argsort(spheres["r"])[-3:]
    mats["EmissiveColor"][big] = (1.0, 0.8, 0.6)
    mats["EmissiveStrength"][big] = 10.0
    cam = host.camera_matrices(w, h, jitter=False)
    r = dxrs.Renderer(device=0)
    try:
        gpu_setup(r, dxrs, spheres, mats, sd, cam, w, h)
        assert not r.accel.lds_resident
        hp = HostPass(*shims, spheres, mats)
        for f in range(2):
            written, _, _ = gpu_frame(r, hp, w, h, cam, f"frame {f}", frame_index=f, reset_history=f == 0)
            assert written.sum() > 16, f"frame {f}: the emitters light {int(written.sum())} pixels"
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_zero_emitters_writes_nothing(dxrs, host, renderer):
    w, h = 64, 48
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    mats = mats.copy()
    mats["EmissiveStrength"] = 0.0
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    dd, ds, _ = renderer.restir_di(fill=SENTINEL)
    for t in (dd, ds):
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_history_restarts_and_moved_spheres_keep_it(dxrs, host, renderer, shims):
    """The history logic has no CPU counterpart: which call restarts is decided by the entry point (pt_api.hip, which needs a device);
    the header only takes the decision as RiParams::history_valid, and a CPU test would check HostPass's Python copy of the rules
    against itself.  Here each rule is discriminated by bit parity with the library.
    ResetHistory, a size change and a new scene restart the history (the host model is told to); spheres moved by
    pt_update_spheres keep it (the host model continues) -- bit parity holds only if the library decides the same"""
    w, h = 64, 48
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = HostPass(*shims, spheres, mats)
    gpu_frame(renderer, hp, w, h, cam, "first", frame_index=0, reset_history=True)
    gpu_frame(renderer, hp, w, h, cam, "continue", frame_index=1)
    gpu_frame(renderer, hp, w, h, cam, "reset", frame_index=2, reset_history=True)
    # moved spheres: the history continues
    moved = spheres.copy()
    moved["cy"][1:] += 0.05
    renderer.update_spheres(moved)
    hp.spheres = np.ascontiguousarray(moved)
    gpu_frame(renderer, hp, w, h, cam, "moved", frame_index=3)
    # a new scene restarts
    gpu_setup(renderer, dxrs, moved, mats, sd, cam, w, h)
    hp.valid = False
    gpu_frame(renderer, hp, w, h, cam, "new scene", frame_index=4)
    gpu_frame(renderer, hp, w, h, cam, "continue 2", frame_index=5)
    # a size change restarts
    w2, h2 = 40, 24
    cam2 = host.camera_matrices(w2, h2, jitter=False)
    renderer.set_camera(cam2)
    renderer.set_constants(dxrs.types.graphics_settings(w2, h2, frame_index=6, bounces=2, spp=1))
    gpu_frame(renderer, hp, w2, h2, cam2, "resized", frame_index=6)


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True])
def test_gpu_chain_three_lanes(dxrs, host, alias):
    """pt_render_gbuffer -> pt_restir_di -> pt_render_with_di with three frames in flight, one buffer set per lane, no host wait in
    between: the frames equal, bit for bit, the same frames fed a downloaded and re-uploaded copy of the DI"""
    import torch
    w, h, frames, mode = 64, 48, 5, 3
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    from dxrs_amd.abi_types import GBUFFER_CHANNELS
    width = dict(GBUFFER_CHANNELS)

    def run(reupload):
        r = dxrs.Renderer(device=0, frames_in_flight=3)
        try:
            r.set_scene(spheres, mats, sd)
            sets = [dict(gb={n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS},
                         dd=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), ds=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                         out=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), nd=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                         ns=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")) for _ in range(3)]
            torch.cuda.synchronize()
            outs, dis = [], []
            for f in range(frames):
                s = sets[f % 3]
                r.set_camera(host.camera_matrices(w, h, jitter_index=f))
                r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=4, spp=1))
                if reupload or f >= 3:
                    r.synchronize()      # (the buffers are cleared from the host side)
                    for t in (s["dd"], s["ds"], s["nd"], s["ns"]):
                        t.zero_()
                    torch.cuda.synchronize()
                ptrs = {n: b.data_ptr() for n, b in s["gb"].items()}
                r.render_gbuffer_device(ptrs)
                dd, ds = (s["nd"], s["ns"]) if alias else (s["dd"], s["ds"])
                r.restir_di_device(w, h, dict(ptrs, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), frame_index=f, spatial_samples=2)
                if reupload:
                    r.synchronize()
                    dd2, ds2 = torch.from_numpy(dd.cpu().numpy().copy()).cuda(), torch.from_numpy(ds.cpu().numpy().copy()).cuda()
                    if alias:
                        s["nd"].copy_(dd2); s["ns"].copy_(ds2)
                        dd2, ds2 = s["nd"], s["ns"]
                    torch.cuda.synchronize()
                    dd, ds = dd2, ds2
                r.render_with_di_device(s["out"].data_ptr(), dd.data_ptr(), ds.data_ptr(), None, mode, {"Diffuse": s["nd"].data_ptr(), "Specular": s["ns"].data_ptr()})
                if reupload or f >= 2:
                    r.synchronize()
                    outs.append([s["out"].cpu().numpy().copy(), s["nd"].cpu().numpy().copy(), s["ns"].cpu().numpy().copy()])
            r.synchronize()
            return outs
        finally:
            r.close()

    free, staged = run(False), run(True)
    for k, got in enumerate(free):
        want = staged[len(staged) - len(free) + k]
        for a, b, name in zip(got, want, ("out", "Diffuse", "Specular")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"frame {k} {name}"
    assert any((g[0][..., :3] > 0).any() for g in free)


@pytest.mark.gpu
def test_gpu_argument_errors_leave_outputs_untouched(dxrs, host, renderer):
    import torch
    w, h = 64, 48
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    from dxrs_amd.abi_types import GBUFFER_CHANNELS
    width = dict(GBUFFER_CHANNELS)
    gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS}
    out = torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({n: b.data_ptr() for n, b in gb.items()})  # real surfaces: a rejected call that launched anyway would write
    renderer.synchronize()
    assert bool((torch.isfinite(gb["LinearDepth"][..., 0]) & (gb["NormalRoughness"][..., 3] >= 0.05)).any())
    good = dict({n: b.data_ptr() for n, b in gb.items()}, Diffuse=out[0].data_ptr(), Specular=out[1].data_ptr())
    lib, ctx = renderer._lib, renderer._ctx
    from dxrs_amd.abi_types import PtRestirDiSettings, PtRestirDiTextures

    def status(buffers=good, **kw):
        fields = dict(RenderSize=(C.c_uint32 * 2)(w, h))
        fields.update(kw)
        s = PtRestirDiSettings(**fields)
        t = PtRestirDiTextures(**{n: C.c_void_p(p) for n, p in buffers.items() if p})
        return lib.pt_restir_di(ctx, C.byref(s), C.byref(t))

    INVALID, UNSUPPORTED = 1, 5
    assert lib.pt_restir_di(ctx, None, None) == INVALID
    for name in good:
        assert status(dict(good, **{name: 0})) == INVALID, name
    assert status(dict(good, Position=good["Position"] + 4)) == INVALID
    assert status(dict(good, GeometricNormal=good["GeometricNormal"] + 4)) == INVALID
    assert status(dict(good, Diffuse=good["Diffuse"] + 8)) == INVALID
    assert status(dict(good, Specular=good["Diffuse"])) == INVALID                    # the outputs overlap
    assert status(dict(good, Specular=good["Diffuse"] + 16 * (w * h - 1))) == INVALID  # ... by one pixel
    assert status(dict(good, Diffuse=good["NormalRoughness"])) == INVALID              # an output over an input
    assert status(RenderSize=(C.c_uint32 * 2)(0, h)) == INVALID and status(RenderSize=(C.c_uint32 * 2)(w, 16385)) == INVALID
    assert status(InitialSamples=33) == INVALID and status(SpatialSamples=33) == INVALID
    assert status(EnableTemporal=2) == INVALID and status(EnableSpatial=2) == INVALID
    assert status(TemporalBiasCorrection=4) == INVALID and status(SpatialBiasCorrection=7) == INVALID
    assert status(TemporalBiasCorrection=PAIRWISE) == UNSUPPORTED and status(SpatialBiasCorrection=PAIRWISE) == UNSUPPORTED
    for bad in (-1.0, float("nan"), float("inf")):
        assert status(SpatialRadius=bad) == INVALID
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    assert status() == 0
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) != SENTINEL.view(np.uint32)).any()
    # PT_ERR_STATE as pt_render: no acceleration structure for the current scene
    r2 = dxrs.Renderer(device=0)
    try:
        s = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h))
        t = PtRestirDiTextures(**{n: C.c_void_p(p) for n, p in good.items()})
        assert r2._lib.pt_restir_di(r2._ctx, C.byref(s), C.byref(t)) == 4
    finally:
        r2.close()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, shims, tmp_path):
    """RTXDI (host/RTXDI.hpp) bound to pt_restir_di from C++, three frames of the demo scene: every pixel the host-compiled header
    writes from the program's own G-buffer holds the same bits, and every other pixel keeps what the buffers held before the pass (a
    frame the program rendered into them)"""
    import subprocess
    from types import SimpleNamespace
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_restir_di")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_restir_di.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h, frames = 96, 64, 3
    outp = str(tmp_path / "restir.f32")
    res = subprocess.run([exe, str(w), str(h), str(frames), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout and "pairwise" in res.stdout
    data = np.fromfile(outp, dtype=np.float32)
    n = w * h
    per_frame = 6 + n * (sum(WIDTH.values()) + 16)
    assert len(data) == frames * per_frame
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    hp = HostPass(*shims, spheres, mats)
    lit = 0
    for f in range(frames):
        d = data[f * per_frame:(f + 1) * per_frame]
        cam = SimpleNamespace(Position=d[0:3], PreviousPosition=d[3:6])
        before_d, before_s = d[6:6 + 4 * n].reshape(n, 4), d[6 + 4 * n:6 + 8 * n].reshape(n, 4)
        assert (before_d[:, 3] == 1).all() and (before_s[:, 3] == 1).all()
        at, gb = 6 + 8 * n, {}
        for name in INPUTS:
            gb[name] = d[at:at + n * WIDTH[name]].reshape(n, WIDTH[name])
            at += n * WIDTH[name]
        got_d, got_s = d[at:at + 4 * n].reshape(n, 4), d[at + 4 * n:at + 8 * n].reshape(n, 4)
        want_d, want_s = hp.frame(gb, w, h, cam, frame_index=f, reset_history=f == 0, spatial_samples=2)
        written = want_d[:, 0:1].view(np.uint32)[:, 0] != SENTINEL.view(np.uint32)
        lit += int(written.sum())
        for got, want, before, name in ((got_d, want_d, before_d, "Diffuse"), (got_s, want_s, before_s, "Specular")):
            expect = np.where(written[:, None], want, before)
            assert np.array_equal(got.view(np.uint32), expect.view(np.uint32)), f"frame {f} {name}"
    assert lit > 0
