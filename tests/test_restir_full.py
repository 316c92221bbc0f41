"""Row N22 -- pt_restir_di_full: pairwise bias correction and final-visibility reuse (DESIGN.md spec S26).
CPU: the host-compiled header paths (tests/hostshim/restir_full_host.cpp over csrc/pt_restir.h) against the float64 restatement
(restir_full_reference.py) and known answers -- the visibility word and its gate, the two exact regimes of reuse and its one-sided
property, pairwise MIS pass by pass, its known answers, unbiasedness without occluders, the stand-alone sanitizer program.
GPU: whole pt_restir_di_full calls against the host-compiled header bit for bit, outputs and both history slots."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import restir_full_reference as fref
import restir_reference as ref
from test_light_ris import CPU_POWER, CPU_REGIR, MAX_EXCLUDED, POWER, REGIR, UNIFORM, U, history_equal, quadrature_image, same_bits, sampling
from test_restir_mis import MisHostPass
from test_restir_pass import (BASIC, BLOCKER, E0, F_FRAMES, GROUND, H, HISTORY, INPUTS, OFF, PAIRWISE, PASS_RTOL, RAYTRACED, SENTINEL, W, cpu_gbuffer, deviation, gpu_setup,
                              make_scene, reservoirs, settings)

HERE = os.path.dirname(os.path.abspath(__file__))
CAM = dict(position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
LUM = np.array([0.2126, 0.7152, 0.0722])
NO_EXTRAS = dict(brdf_samples=0, boiling_filter=None)
REUSE_OFF = dict(reuse=False, max_age=0, max_distance=0.0)
SDK_DEFAULTS = dict(reuse=True, max_age=4, max_distance=16.0)  # as recollected: what host/RTXDI.hpp's ShadingSettings holds
SW, SH = 24, 16  # the small view of the frame sequences


# ---------------------------------------------------------------------------------------------------- the host-compiled headers
@pytest.fixture(scope="module")
def shims():
    """(rf, lr, ri, gb, rm): index 1 .. 3 as test_restir_mis's, so that its MisHostPass takes (rm, lr, ri, gb)"""
    import __graft_entry__ as g

    vp, u32, f32, i32 = C.c_void_p, C.c_uint32, C.c_float, C.c_int
    rf = C.CDLL(g.build_restir_full_shim())
    for name, res, args in (("rf_host_call", None, [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, f32, vp, f32, vp, f32, vp]), ("rf_host_vis_fresh", u32, []),
                            ("rf_host_vis_moved", u32, [u32, i32, i32]), ("rf_host_vis_usable", u32, [u32, u32, f32, u32, u32]),
                            ("rf_host_pairwise", None, [u32, f32, f32, f32, vp, vp])):
        getattr(rf, name).restype, getattr(rf, name).argtypes = res, args
    rm = C.CDLL(g.build_restir_mis_shim())
    rm.rm_host_call.restype, rm.rm_host_call.argtypes = None, [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, f32, vp, f32]
    lr = C.CDLL(g.build_lightris_shim())
    ri = C.CDLL(g.build_restir_shim())
    ri.ri_host_call.restype, ri.ri_host_call.argtypes = None, [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp]
    gb = C.CDLL(g.build_gbuffer_shim())
    gb.gb_pixels.restype = None
    gb.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    gb.gb_srgb_lut.restype = None
    gb.gb_srgb_lut.argtypes = [vp]
    return rf, lr, ri, gb, rm


def mis_pass(shims, spheres, mats, textures=None):
    return MisHostPass((shims[4], shims[1], shims[2], shims[3]), spheres, mats, textures)


class FullHostPass(MisHostPass):
    """pt_restir_di_full over the host-compiled header: MisHostPass's slots and restart rules, rf_host_call in place of rm_host_call;
    shading = dict(reuse, max_age, max_distance) or None.  self.rays after a call: launch 1's, the spatial pass's and final shading's
    rays, and the number of final-shading pixels written without one."""

    def __init__(self, shims, spheres, mats, textures=None):
        MisHostPass.__init__(self, (shims[0], shims[1], shims[2], shims[3]), spheres, mats, textures)
        self.rays = np.zeros(4, np.uint64)

    def call(self, gb, w, h, cam, out_d, out_s, launches=3, light_sampling=None, candidates=None, shading=None, **kw):
        s = settings(**kw)
        ls = light_sampling or sampling(UNIFORM)
        cd = dict(NO_EXTRAS, **(candidates or {}))
        sh = dict(REUSE_OFF, **(shading or {}))
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
        sprm = np.array([ls["mode"], ls["tile_size"], ls["tile_count"], ls["grid_size"], ls["lights_per_cell"], ls["build_samples"]], np.uint32)
        on = cd["boiling_filter"] is not None
        cprm = np.array([cd["brdf_samples"], int(on)], np.uint32)
        shprm = np.array([int(sh["reuse"]), sh["max_age"]], np.uint32)
        arrays = [np.ascontiguousarray(gb[name], dtype=np.float32) for name in INPUTS] + self.slots[cur] + self.slots[prev] + [out_d, out_s]
        ptrs = (C.c_void_p * 24)(*[a.ctypes.data for a in arrays])
        p = lambda a: a.ctypes.data if a is not None else None
        self.lib.rf_host_call(p(self.spheres), p(self.mats), len(self.spheres), p(self.texels), p(self.info), 0 if self.info is None else len(self.info),
                              p(self.maps), p(self.rot), p(prm), p(fprm), ptrs, p(sprm), ls["cell_size"], p(cprm), float(cd["boiling_filter"]) if on else 0.0,
                              p(shprm), float(sh["max_distance"]), p(self.rays))
        if launches != 4:
            self.cur, self.valid = cur, True
        return self.slots[cur]

    def handed(self, gb, w, h, cam, **kw):
        """the reservoirs the spatial pass of the last call handed to final shading -> (dicts, words)"""
        a, c = (np.zeros((w * h, 4), np.float32) for _ in range(2))
        self.call(gb, w, h, cam, a, c, launches=4, **kw)
        return reservoirs([None] * 5 + [a, c]), c[:, 3].copy().view(np.uint32)


def words(slot):
    return slot[6][:, 3].copy().view(np.uint32)


def written(out):
    return out[:, 0].copy().view(np.uint32) != SENTINEL.view(np.uint32)


@pytest.fixture(scope="module")
def cpu_case(dxrs, host, oracle, shims):
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(W, H, **CAM)
    gb, ids = cpu_gbuffer((shims[2], shims[3]), oracle, cam, W, H, spheres, mats, sd)
    assert (ids == GROUND).any() and (ids == BLOCKER).any()
    return spheres, mats, sd, cam, gb


def travelling(host, w, h, f, prev):
    return host.camera_matrices(w, h, position=(0.3 * f, 2.5 + 0.05 * f, -9.0 + 0.4 * f), look_at=(0.1 * f, 1.0, 0.0), hfov=math.radians(70), jitter_index=f, previous=prev)


@pytest.fixture(scope="module")
def sequences(dxrs, host, oracle, shims):
    """the 24 x 16 frame sequences among occluders: eight frames of a travelling camera and one frame of a resting one (Jitter 0), each
    (camera, G-buffer)"""
    spheres, mats, sd = make_scene(dxrs)
    moving, prev = [], None
    for f in range(8):
        cam = travelling(host, SW, SH, f, prev)
        moving.append((cam, cpu_gbuffer((shims[2], shims[3]), oracle, cam, SW, SH, spheres, mats, sd)[0]))
        prev = cam
    cam = host.camera_matrices(SW, SH, **CAM)
    resting = (cam, cpu_gbuffer((shims[2], shims[3]), oracle, cam, SW, SH, spheres, mats, sd)[0])
    return spheres, mats, moving, resting


# ---------------------------------------------------------------------------------------------------- 1. CPU: ABI
def test_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_restir_di_full") and "pt_restir_di_full" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtLightSamplingSettings, PtRestirDiCandidates, PtRestirDiSettings, PtRestirDiShading, PtRestirDiTextures
    S = PtRestirDiShading
    assert C.sizeof(S) == 16
    assert [getattr(S, f).offset for f in ("ReuseFinalVisibility", "FinalVisibilityMaxAge", "FinalVisibilityMaxDistance", "_pad")] == [0, 4, 8, 12]
    assert C.sizeof(PtRestirDiSettings) == 48 and C.sizeof(PtLightSamplingSettings) == 32 and C.sizeof(PtRestirDiCandidates) == 16 and C.sizeof(PtRestirDiTextures) == 80
    s, ls, cd, sh, t = PtRestirDiSettings(), PtLightSamplingSettings(), PtRestirDiCandidates(), S(), PtRestirDiTextures()
    INVALID = 1  # a null context, whatever else is null: what the three siblings answer
    assert lib.pt_restir_di_full(None, C.byref(s), C.byref(ls), C.byref(cd), C.byref(sh), C.byref(t)) == INVALID
    assert lib.pt_restir_di_full(None, None, None, None, None, None) == INVALID
    assert lib.pt_restir_di_ex(None, None, None, None, None) == INVALID and lib.pt_restir_di_sampled(None, None, None, None) == INVALID and lib.pt_restir_di(None, None, None) == INVALID


# ---------------------------------------------------------------------------------------------------- 2. CPU: extras off
@pytest.mark.parametrize("n_brdf", [0, 1])
@pytest.mark.parametrize("ls", [None, CPU_POWER, CPU_REGIR], ids=["uniform", "power", "regir"])
def test_extras_off_is_pt_restir_di_ex(shims, cpu_case, ls, n_brdf):
    """shading null or ReuseFinalVisibility 0 and modes 0 / 1 / 3: outputs and both history slots equal pt_restir_di_ex's header path bit
    for bit (the word included: 0), four frames with the history running"""
    spheres, mats, sd, cam, gb = cpu_case
    old, new = mis_pass(shims, spheres, mats), FullHostPass(shims, spheres, mats)
    cd = dict(brdf_samples=n_brdf, boiling_filter=0.2 if n_brdf else None)
    modes = [(OFF, RAYTRACED), (BASIC, BASIC), (RAYTRACED, OFF), (BASIC, RAYTRACED)]
    for f in range(4):
        kw = dict(frame_index=f, reset_history=f == 0, spatial_samples=2, spatial_radius=8.0, temporal_bias=modes[f][0], spatial_bias=modes[f][1], light_sampling=ls,
                  candidates=cd)
        a = old.frame(gb, W, H, cam, **kw)
        b = new.frame(gb, W, H, cam, shading=None if f & 1 else dict(reuse=False, max_age=4, max_distance=16.0), **kw)
        for x, y, name in zip(a, b, ("Diffuse", "Specular")):
            assert same_bits(x, y), f"frame {f}: {name}"
        for k in range(2):
            for x, y in zip(old.slot(k), new.slot(k)):
                assert same_bits(x, y), f"frame {f}: history slot {k}"
        assert not words(new.slot(new.cur)).any()
    assert (new.slot(new.cur)[6][:, 0] > 8 + n_brdf).any(), "the history ran"


# ---------------------------------------------------------------------------------------------------- 3. CPU: the visibility word
def test_word_arithmetic_and_gate_known_answers(shims):
    rf = shims[0]
    fresh = rf.rf_host_vis_fresh()
    assert fresh == fref.encode(fref.FRESH) == 1 | (128 << 8) | (128 << 16)
    assert rf.rf_host_vis_moved(0, 3, -4) == 0, "the word that says nothing moves to itself"
    # the header against the restatement over steps that cross the range in both directions
    for start in (fref.FRESH, (True, 120, -120), (False, 5, 5), (True, None, 3), (True, -127, 127)):
        for dx in (-300, -128, -127, -8, -1, 0, 1, 7, 127, 128, 254, 255, 300):
            for dy in (-255, -1, 0, 1, 254):
                got = rf.rf_host_vis_moved(fref.encode(start), dx, dy)
                assert got == fref.encode(fref.moved(start, dx, dy)), (start, dx, dy, hex(got))
    # sticky saturation: 127 pixels is held, one more saturates the axis, and coming back does not restore it
    a = rf.rf_host_vis_moved(fresh, 127, 0)
    assert fref.decode(a) == (True, 127, 0)
    b = rf.rf_host_vis_moved(a, 1, 0)
    assert fref.decode(b) == (True, None, 0)
    c = rf.rf_host_vis_moved(b, -100, 2)
    assert fref.decode(c) == (True, None, 2)
    usable = lambda reuse, max_age, dist, age, word: bool(rf.rf_host_vis_usable(int(reuse), max_age, dist, age, word))
    assert not usable(True, 255, 1e30, 0, c), "a saturated offset is never inside the window"
    assert usable(True, 255, 1e30, 0, a)
    # the gate: reuse off, bit clear, age at and above MaxAge, the distance at and just above MaxDistance
    at = lambda dx, dy: fref.encode((True, dx, dy))
    assert not usable(False, 4, 16.0, 0, fresh) and not usable(True, 4, 16.0, 0, fref.encode((False, 0, 0))) and not usable(True, 4, 16.0, 0, 0)
    assert usable(True, 4, 16.0, 4, fresh) and not usable(True, 4, 16.0, 5, fresh)
    assert usable(True, 0, 0.0, 0, fresh) and not usable(True, 0, 0.0, 1, fresh) and not usable(True, 0, 0.0, 0, at(1, 0))
    assert usable(True, 4, 5.0, 0, at(3, 4)) and usable(True, 4, 5.0, 0, at(-4, 3)) and not usable(True, 4, 5.0, 0, at(4, 4)) and not usable(True, 4, 5.0, 0, at(3, -5))
    assert usable(True, 4, 16.0, 0, at(16, 0)) and not usable(True, 4, 16.0, 0, at(16, 1)) and usable(True, 4, 16.0, 0, at(-11, 11)) and not usable(True, 4, 16.0, 0, at(12, -11))
    for word in (fresh, at(3, 4), at(16, 1), a, c, 0):
        for age in (0, 4, 5):
            assert usable(True, 4, 16.0, age, word) == fref.usable(True, 4, 16.0, age, fref.decode(word))


def test_word_set_by_initial_sampling_and_carried_by_temporal(shims, cpu_case):
    """launch 1 alone.  The word is FRESH exactly where the initial visibility ray succeeded (W > 0), 0 on an occluded or empty sample.
    Then over a hand-built history (every record from the real frame, reservoirs with W 1e6 in even columns and W 0 in odd ones, a known
    word and age 5) and a motion vector of one pixel: where the history's sample is selected its word arrives moved by (-1, 0) with age 6
    (a temporal hit), elsewhere the current sample keeps its own word and age 0 (a temporal miss)."""
    spheres, mats, sd, cam, gb = cpu_case
    n = W * H
    zeros = lambda: (np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32))
    hp = FullHostPass(shims, spheres, mats)
    reuse = dict(reuse=True, max_age=4, max_distance=16.0)
    slot = hp.call(gb, W, H, cam, *zeros(), launches=1, frame_index=0, spatial=False, shading=reuse)
    valid = np.isfinite(slot[3][:, 2])
    lit = slot[5][:, 3] > 0
    assert (valid & lit).sum() > 100 and (valid & ~lit).sum() > 20, "lit and occluded samples both occur"
    assert (words(slot)[valid & lit] == fref.encode(fref.FRESH)).all() and (words(slot)[valid & ~lit] == 0).all()
    # the hand-built history
    word_in = fref.encode((True, 3, -2))
    res0, res1 = slot[5], slot[6]
    res0[:, 3] = np.where(np.arange(n) % W % 2 == 0, 1e6, 0.0)
    res1[:, 2] = np.array([5], np.uint32).view(np.float32)[0]
    res1[:, 3] = np.array([word_in], np.uint32).view(np.float32)[0]
    moved_gb = dict(gb, MotionVector=np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1)))
    alone = FullHostPass(shims, spheres, mats)  # frame 1's initial samples by themselves
    cur = alone.call(moved_gb, W, H, cam, *zeros(), launches=1, frame_index=1, temporal=False, spatial=False, shading=reuse)
    out = hp.call(moved_gb, W, H, cam, *zeros(), launches=1, frame_index=1, spatial=False, shading=reuse)
    got, got_w, cur_w = reservoirs(out), words(out), words(cur)
    hits = misses = 0
    for i in np.flatnonzero(valid):
        if got[i]["age"] == 6:
            assert (i % W) % 2 == 1, "only an even column's history carries weight, and it is read from one pixel to the right"
            assert got_w[i] == fref.encode(fref.moved((True, 3, -2), -1, 0)) == fref.encode((True, 2, -2)), i
            hits += 1
        else:
            assert got[i]["age"] == 0 and got_w[i] == cur_w[i], i
            misses += 1
    assert hits > 50 and misses > 50, (hits, misses)


def raw_neighbour(px, py, k, rot, radius):
    """restir_reference.neighbour before the reflection into view"""
    rr = math.sqrt((k + 0.5) / 32.0) * radius
    a = k * ref.GOLDEN + rot
    a -= math.floor(a)
    return px + math.floor(rr * math.cos(2.0 * math.pi * a) + 0.5), py + math.floor(rr * math.sin(2.0 * math.pi * a) + 0.5)


def test_word_carried_by_the_spatial_pass(shims, cpu_case):
    """the spatial pass alone over launch 1's slot with every reservoir's age set to its pixel index + 1 and a word that depends on the
    pixel: a pick's age names the neighbour it came from, and its word is that neighbour's moved by (px - qx, py - qy), the neighbour's
    position taken after the reflection into view"""
    spheres, mats, sd, cam, gb = cpu_case
    n = W * H
    hp = FullHostPass(shims, spheres, mats)
    reuse = dict(reuse=True, max_age=4, max_distance=16.0)
    slot = hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, frame_index=0, spatial=False, shading=reuse)
    valid = np.isfinite(slot[3][:, 2])
    word_of = lambda i: (True, (i % W) % 7 - 3, (i // W) % 5 - 2)
    slot[6][:, 2] = (np.arange(n, dtype=np.uint32) + 1).view(np.float32)
    slot[6][:, 3] = np.array([fref.encode(word_of(i)) for i in range(n)], np.uint32).view(np.float32)
    kw = dict(frame_index=0, spatial_samples=4, spatial_radius=30.0, shading=reuse)
    picks = reflected = 0
    for bias in (BASIC, PAIRWISE):
        got, got_w = hp.handed(gb, W, H, cam, spatial_bias=bias, **kw)
        for i in np.flatnonzero(valid):
            px, py = i % W, i // W
            q = got[i]["age"] - 1
            if q == i:
                assert got_w[i] == fref.encode(word_of(i))
                continue
            qx, qy = q % W, q // W
            assert got_w[i] == fref.encode(fref.moved(word_of(q), px - qx, py - qy)), (bias, i, q)
            picks += 1
            rng = ref.it.Stream(ref.it.rng_seed(px, py, (0 ^ ref.SALT_SPATIAL) & 0xFFFFFFFF))
            start, rot = rng.uint() & 31, rng.unit()
            for k in range(4):
                if ref.neighbour(px, py, W, H, (start + k) & 31, rot, 30.0) == (qx, qy) and raw_neighbour(px, py, (start + k) & 31, rot, 30.0) != (qx, qy):
                    reflected += 1
    assert picks > 200 and reflected > 20, (picks, reflected)


def test_alpha_tested_emitter_is_always_traced(dxrs, host, oracle, shims):
    """one emitter, whose material is alpha-tested through a base-colour map (opaque everywhere): every final ray is cast, however
    fresh the sample; the same scene with the emitter Opaque reuses"""
    from dxrs_amd.textures import TextureSet
    spheres, mats, sd = make_scene(dxrs, emitters=(E0,))
    cam = host.camera_matrices(SW, SH, **CAM)
    gb, _ = cpu_gbuffer((shims[2], shims[3]), oracle, cam, SW, SH, spheres, mats, sd)
    ts = TextureSet(len(spheres))
    ts.maps[E0, 0] = ts.add_image(np.full((8, 8, 4), 255, np.uint8))
    reused = {}
    for mode in (0, 1):
        m = mats.copy()
        m["BaseColor"][E0] = (1.0, 1.0, 1.0, 1.0)
        m["AlphaMode"][E0] = mode
        hp = FullHostPass(shims, spheres, m, textures=ts)
        out = hp.frame(gb, SW, SH, cam, frame_index=0, reset_history=True, spatial=False, shading=dict(reuse=True, max_age=0, max_distance=0.0))
        reused[mode] = (int(hp.rays[3]), int(hp.rays[2]), int(written(out[0]).sum()))
    print(f"(pixels without a final ray, final rays, pixels written): emitter Opaque {reused[0]}, alpha-tested {reused[1]}")
    assert reused[0][0] > 20 and reused[0][0] == reused[0][2], "without spatial reuse every written pixel is the pixel's own fresh sample"
    assert reused[1][0] == 0 and reused[1][1] >= reused[1][2] > 20


# ---------------------------------------------------------------------------------------------------- 4 - 6. CPU: the regimes of reuse
def run_sequence(shims, spheres, mats, frames, shading, **kw):
    """-> per frame (Diffuse, Specular, final rays, pixels without one, handed reservoirs, handed words)"""
    hp, out = FullHostPass(shims, spheres, mats), []
    for f, (cam, gb) in enumerate(frames):
        args = dict(frame_index=f, reset_history=f == 0, spatial_samples=2, spatial_radius=6.0, shading=shading, **kw)
        d, s = hp.frame(gb, SW, SH, cam, **args)
        rays, free = int(hp.rays[2]), int(hp.rays[3])
        out.append((d, s, rays, free) + hp.handed(gb, SW, SH, cam, **args))
    return out


@pytest.fixture(scope="module")
def regimes(shims, sequences):
    spheres, mats, moving, resting = sequences
    rest = [resting] * 8
    return dict(moving_off=run_sequence(shims, spheres, mats, moving[:6], None), moving_a=run_sequence(shims, spheres, mats, moving[:6], dict(reuse=True, max_age=0, max_distance=0.0)),
                resting_off=run_sequence(shims, spheres, mats, rest, None), resting_b=run_sequence(shims, spheres, mats, rest, dict(reuse=True, max_age=255, max_distance=0.0)),
                moving_sdk=run_sequence(shims, spheres, mats, moving[:6], SDK_DEFAULTS))


def outputs_equal(a, b, what):
    for f, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x[0], y[0]) and same_bits(x[1], y[1]), f"{what}: frame {f}"


def test_exact_regime_a_travelling_camera(regimes):
    """MaxAge 0, MaxDistance 0 among occluders, six frames of a travelling camera: the reused ray is the ray initial sampling cast in
    this call, so the outputs equal reuse off bit for bit, with strictly fewer final rays"""
    off, on = regimes["moving_off"], regimes["moving_a"]
    outputs_equal(off, on, "regime A")
    rays_off, rays_on = sum(x[2] for x in off), sum(x[2] for x in on)
    print(f"regime A: final rays {rays_on} against {rays_off} with reuse off ({1 - rays_on / rays_off:.3f} saved)")
    assert sum(int(written(x[0]).sum()) for x in off) > 6 * 50 and rays_on < rays_off and sum(x[3] for x in on) == rays_off - rays_on


def test_exact_regime_b_resting_camera(regimes):
    """a resting camera (Jitter 0) over a static scene, MaxDistance 0, MaxAge 255, eight frames: a sample that stays at its pixel is
    re-aimed along the very ray that found it, so the outputs equal reuse off bit for bit; temporal picks now reuse too, so a smaller
    share of the final rays is cast than in regime A, and fewer per frame"""
    off, on = regimes["resting_off"], regimes["resting_b"]
    outputs_equal(off, on, "regime B")
    a_off, a_on = regimes["moving_off"], regimes["moving_a"]
    share_a = sum(x[2] for x in a_on) / sum(x[2] for x in a_off)
    share_b = sum(x[2] for x in on) / sum(x[2] for x in off)
    print(f"regime B: final rays {sum(x[2] for x in on)} against {sum(x[2] for x in off)} with reuse off: {share_b:.3f} of them cast, regime A {share_a:.3f}")
    assert share_b < share_a and sum(x[2] for x in on) / len(on) < sum(x[2] for x in a_on) / len(a_on)


def test_reuse_is_one_sided_at_the_sdk_defaults(shims, regimes):
    """MaxAge 4, MaxDistance 16 on the travelling camera among occluders.  Reuse never changes a reservoir: what the spatial pass hands
    to final shading is the same sample either way.  Every pixel reuse off writes holds the same bits with reuse on; every extra pixel
    holds a sample whose word passes the gate -- its traced ray was blocked, or reuse off would have written it.
    Measured on this sequence (6 frames of 24 x 16): 0.9993 of the final rays saved (1 cast against 1386: a sample with W > 0 was seen
    when it was drawn, so only age and distance keep it from the gate), 0.0180 of the written pixels leaked (25 of 1386)."""
    off, on = regimes["moving_off"], regimes["moving_sdk"]
    rf = shims[0]
    extra = total = 0
    for f, (a, b) in enumerate(zip(off, on)):
        for key in ("light", "u1", "u2", "W", "M", "p_hat", "age"):
            assert [r[key] for r in a[4]] == [r[key] for r in b[4]], f"frame {f}: reuse changed a reservoir's {key}"
        wa, wb = written(a[0]), written(b[0])
        assert not (wa & ~wb).any(), f"frame {f}: reuse dropped a pixel"
        assert same_bits(a[0][wa], b[0][wa]) and same_bits(a[1][wa], b[1][wa]), f"frame {f}"
        for i in np.flatnonzero(wb & ~wa):
            assert rf.rf_host_vis_usable(1, 4, 16.0, b[4][i]["age"], int(b[5][i])), (f, i, b[4][i], hex(int(b[5][i])))
        extra += int((wb & ~wa).sum())
        total += int(wb.sum())
    rays_off, rays_on = sum(x[2] for x in off), sum(x[2] for x in on)
    print(f"SDK defaults: {1 - rays_on / rays_off:.4f} of the final rays saved ({rays_on} against {rays_off}); {extra} of {total} written pixels leaked ({extra / total:.4f})")
    assert rays_on < rays_off


# ---------------------------------------------------------------------------------------------------- 7. CPU: pairwise against the restatement
# W = w_sum / p_sel.  The reservoirs' M, W and stored p_hat are the same float32 numbers on both sides; the re-aimed targets p_c(y_i) and
# p_i(y_c) carry test_restir_pass's PASS_RTOL each.  m_i = a / (a + b) with b in error moves by at most PASS_RTOL, so a neighbour's weight
# p_c(y_i) W_i m_i / k by 2 PASS_RTOL and 4 roundings; a canonical term c / (M_i p_i(y_c) + c) by PASS_RTOL and 3 roundings, their mean and
# the product with p_c(y_c) W_c by k + 3 more; the sum of the k + 1 weights by k roundings; the quotient by the selected target, which is
# re-aimed for a neighbour's sample, by PASS_RTOL and 1: 3 PASS_RTOL + (k + 6) U in all.
def pairwise_bound(k):
    return 3 * PASS_RTOL + (k + 6) * U


def with_words(rs, ws):
    for r, w in zip(rs, ws):
        r["vis"] = fref.decode(int(w))
    return rs


def compare_pairwise(got, got_w, want, margins, bound, what):
    """-> 1 where the pixel is left out: a decision of the restatement within the bound of its threshold and a different pick"""
    same = (got["light"], got["u1"], got["u2"], got["M"]) == (want["light"], np.float32(want["u1"]), np.float32(want["u2"]), want["M"]) and (got["W"] > 0) == (want["W"] > 0)
    if not same:
        assert margins and min(margins) <= bound, f"{what}: the pick differs away from every threshold: {got} != {want}"
        return 1
    tol = lambda a, b: abs(a - b) <= bound * max(abs(a), abs(b)) + 1e-12
    assert tol(got["W"], want["W"]) and tol(got["p_hat"], want["p_hat"]) and got["age"] == want["age"] and int(got_w) == fref.encode(want["vis"]), (what, got, want)
    return 0


PAIRWISE_FRAME = 1


def test_pairwise_temporal_against_restatement(shims, cpu_case):
    spheres, mats, sd, cam, gb = cpu_case
    scene = ref.Scene(spheres, mats)
    n, frame = W * H, PAIRWISE_FRAME
    zeros = lambda: (np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32))
    hp, alone = FullHostPass(shims, spheres, mats), FullHostPass(shims, spheres, mats)
    first = hp.call(gb, W, H, cam, *zeros(), launches=1, frame_index=frame - 1, spatial=False, temporal_bias=PAIRWISE)
    prev = with_words(reservoirs(first), words(first))
    cur_slot = alone.call(gb, W, H, cam, *zeros(), launches=1, frame_index=frame, temporal=False, spatial=False, temporal_bias=PAIRWISE, shading=dict(reuse=True))
    cur = with_words(reservoirs(cur_slot), words(cur_slot))
    out = hp.call(gb, W, H, cam, *zeros(), launches=1, frame_index=frame, spatial=False, temporal_bias=PAIRWISE)
    got, got_w = reservoirs(out), words(out)
    cam_pos, prev_pos = tuple(float(x) for x in cam.Position), tuple(float(x) for x in cam.PreviousPosition)
    cache = {}

    def surfaces(i, pos):
        if (i, pos) not in cache:
            cache[(i, pos)] = ref.surface(gb, i, pos)
        return cache[(i, pos)]
    valid = left_out = near_alone = picked = 0
    for i in range(n):
        s = surfaces(i, cam_pos)
        if s is None:
            continue
        valid += 1
        margins = []
        want, accepted = fref.temporal_pairwise(scene, s, cur[i], surfaces, prev, i % W, i // W, W, H, tuple(float(x) for x in gb["MotionVector"][i]), frame, 20, prev_pos, margins)
        assert accepted, "a resting view reprojects every surface onto itself"
        near_alone += bool(margins) and min(margins) <= pairwise_bound(1)
        left_out += compare_pairwise(got[i], got_w[i], want, margins, pairwise_bound(1), f"pixel {i}")
        picked += got[i]["age"] == 1
    print(f"temporal: {valid} surfaces, the history's sample picked at {picked}; left out {left_out}; near a threshold in the restatement alone {near_alone}")
    assert valid > n // 3 and 0 < picked < valid
    assert near_alone <= MAX_EXCLUDED * valid, "the seed puts too many of the restatement's own comparisons near their thresholds"
    assert left_out <= MAX_EXCLUDED * valid


@pytest.mark.parametrize("k", [1, 4])
def test_pairwise_spatial_against_restatement(shims, cpu_case, k):
    spheres, mats, sd, cam, gb = cpu_case
    scene = ref.Scene(spheres, mats)
    n, frame, radius = W * H, PAIRWISE_FRAME, 6.0
    hp = FullHostPass(shims, spheres, mats)
    kw = dict(spatial_samples=k, spatial_radius=radius, spatial_bias=PAIRWISE, temporal_bias=PAIRWISE)
    for f in (frame - 1, frame):
        slot = hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, frame_index=f, **kw)
    centre = with_words(reservoirs(slot), words(slot))
    got, got_w = hp.handed(gb, W, H, cam, frame_index=frame, **kw)
    cam_pos = tuple(float(x) for x in cam.Position)
    cache = {}

    def surfaces(i, pos):
        if (i, pos) not in cache:
            cache[(i, pos)] = ref.surface(gb, i, pos)
        return cache[(i, pos)]
    valid = left_out = near_alone = reused = full = 0
    for i in range(n):
        s = surfaces(i, cam_pos)
        if s is None:
            continue
        valid += 1
        margins = []
        want, accepted = fref.spatial_pairwise(scene, s, centre[i], surfaces, centre, i % W, i // W, W, H, frame, k, radius, cam_pos, margins)
        reused += bool(accepted)
        full += len(accepted) == k
        near = [m for m in margins if m <= pairwise_bound(k)]
        near_alone += bool(near)
        left_out += compare_pairwise(got[i], got_w[i], want, margins, pairwise_bound(k), f"pixel {i}")
    print(f"spatial, {k} samples: {valid} surfaces, {reused} with a neighbour, {full} with all {k}; left out {left_out}; near a threshold in the restatement alone {near_alone}")
    assert valid > n // 3 and reused > valid // 10 and full > 0
    assert near_alone <= MAX_EXCLUDED * valid, "the seed puts too many of the restatement's own comparisons near their thresholds"
    assert left_out <= MAX_EXCLUDED * valid


# ---------------------------------------------------------------------------------------------------- 8. CPU: pairwise known answers
def host_pairwise(rf, M_c, W_c, pc_yc, rows):
    nb = np.ascontiguousarray(rows, np.float32).reshape(-1, 5)
    out = np.zeros(len(nb) + 1, np.float32)
    rf.rf_host_pairwise(len(nb), M_c, W_c, pc_yc, nb.ctypes.data, out.ctypes.data)
    return out


def test_pairwise_weights_known_answers(shims):
    rf = shims[0]
    # k identical neighbours on the centre's own surface with its M: m = 1 / (k + 1) for each of the k + 1 samples
    for k in (1, 2, 4, 7):
        M, Wt, p = 8.0, 0.37, 1.9
        out = host_pairwise(rf, M, Wt, p, [(M, Wt, p, p, p)] * k)
        assert np.allclose(out, p * Wt / (k + 1), rtol=(k + 8) * U, atol=0), (k, out)
    # a neighbour facing away (p_i(y_c) = 0 and p_c(y_i) = 0): nothing from it, and the canonical weight of that pair is 1
    out = host_pairwise(rf, 8.0, 0.5, 2.0, [(16.0, 0.25, 3.0, 0.0, 0.0)])
    assert out[0] == 0.0 and out[1] == np.float32(2.0) * np.float32(0.5)
    out = host_pairwise(rf, 8.0, 0.5, 2.0, [(16.0, 0.25, 3.0, 0.0, 0.0), (8.0, 0.5, 2.0, 2.0, 2.0)])
    assert out[0] == 0.0 and abs(out[1] - 2.0 * 0.5 * (2.0 / 3.0) / 2) <= 8 * U and abs(out[2] - 2.0 * 0.5 * (1.0 + 1.0 / 3.0) / 2) <= 8 * U
    # an empty canonical reservoir's pair: both denominators can vanish; the term counts 1 and the weights stay finite
    out = host_pairwise(rf, 8.0, 0.0, 0.0, [(8.0, 0.5, 0.0, 0.0, 0.0)])
    assert out[0] == 0.0 and out[1] == 0.0
    # the header against the restatement, and the k + 1 techniques' weights sum to 1 at a common sample
    rng = np.random.default_rng(5)
    for k in (1, 3, 4):
        rows = [tuple(float(x) for x in np.float32(rng.uniform(0.1, 20.0, 5))) for _ in range(k)]
        M_c, W_c, pc = (float(np.float32(x)) for x in rng.uniform(0.5, 10.0, 3))
        out = host_pairwise(rf, M_c, W_c, pc, rows)
        want = fref.pairwise_weights(M_c, W_c, pc, rows)
        assert np.allclose(out, want, rtol=(k + 8) * U, atol=0)
        # one y seen by all: p_i(y) = rows[i][2], p_c(y) = pc; every technique's contribution p / (M p) weight M m -> sums to 1
        y = [(r[0], 1.0, r[2], pc, r[2]) for r in rows]
        w = fref.pairwise_weights(M_c, 1.0, pc, y)
        assert abs(sum(w[i] / pc for i in range(k)) + w[k] / pc - 1.0) <= 1e-12


def test_pairwise_identical_neighbours_equal_basic(shims, cpu_case):
    """every pixel given the record and the reservoir of one lit ground pixel: k identical neighbours with the centre's M weigh 1 / (k + 1)
    each, so W equals Basic's to the counted bound (Basic: Z = (k + 1) M over a sum of k + 1 equal terms); with no accepted neighbour
    (SpatialSamples whose table entries all fall on the pixel itself: radius 0) the centre is returned unchanged"""
    spheres, mats, sd, cam, gb = cpu_case
    n = W * H
    hp = FullHostPass(shims, spheres, mats)
    slot = hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, frame_index=0, spatial=False)
    lit = np.flatnonzero(np.isfinite(slot[3][:, 2]) & (slot[5][:, 3] > 0))
    src = int(lit[len(lit) // 2])
    for plane in slot:
        plane[:] = plane[src]
    centre = reservoirs(slot)[src]
    for k in (1, 4):
        kw = dict(frame_index=0, spatial_samples=k, spatial_radius=5.0)
        basic, _ = hp.handed(gb, W, H, cam, spatial_bias=BASIC, **kw)
        pair, _ = hp.handed(gb, W, H, cam, spatial_bias=PAIRWISE, **kw)
        for i in range(n):
            assert pair[i]["M"] == basic[i]["M"] and (pair[i]["light"], pair[i]["u1"], pair[i]["u2"]) == (centre["light"], centre["u1"], centre["u2"])
            if pair[i]["M"] == (k + 1) * centre["M"]:
                assert abs(pair[i]["W"] - basic[i]["W"]) <= pairwise_bound(k) * basic[i]["W"], (k, i, pair[i], basic[i])
        assert sum(1 for r in pair if r["M"] == (k + 1) * centre["M"]) > n // 2
    alone, _ = hp.handed(gb, W, H, cam, spatial_bias=PAIRWISE, frame_index=0, spatial_samples=4, spatial_radius=0.4)
    for r in alone:
        assert r == centre


# ---------------------------------------------------------------------------------------------------- 9. CPU: unbiasedness
def open_scene(dxrs):
    """a ground under two emitters of unequal power, everything else put away inside the ground.  The line through the emitters' centres
    climbs at 32 degrees, more than the 19 degrees of the cone of lines that touch both spheres, so past the upper emitter that cone never
    comes down, and past the lower one it meets the ground behind the camera (z below -8.6): no surface in view sees one emitter through
    the other.  A visibility ray starts at the spawn origin, not at the point the cone was aimed from, so a sample within about
    offset / r of the limb misses its emitter -- an occlusion of its own, which a quadrature resolves only at k near r / offset.  The
    spawn offset grows with the largest coordinate of the hit sphere (1.5e-2 on make_scene's ground of radius 1000, where the estimate
    loses 0.75 % of the light of an emitter of radius 1): a ground of radius 40 and emitters of radius 1.5 bring the band to 4e-4."""
    spheres, mats, sd = make_scene(dxrs, emitters=(E0, 2), blockers=False)
    spheres = spheres.copy()
    for i in range(len(spheres)):
        if i not in (GROUND, E0, 2):
            spheres["cy"][i] = -30.0
    spheres[GROUND] = (0.0, -40.0, 0.0, 40.0)
    spheres[E0] = (0.0, 4.0, -7.0, 1.5)
    spheres[2] = (0.0, 9.0, 1.0, 1.5)
    return spheres, mats, sd


@pytest.fixture(scope="module")
def statistics(dxrs, host, oracle, shims):
    w, h = SW, SH
    spheres, mats, sd = open_scene(dxrs)
    cam = host.camera_matrices(w, h, **CAM)
    gb, ids = cpu_gbuffer((shims[2], shims[3]), oracle, cam, w, h, spheres, mats, sd)
    scene = ref.Scene(spheres, mats)
    cam_pos = tuple(float(x) for x in cam.Position)
    quad = quadrature_image(scene, gb, w * h, cam_pos, 8)
    unoccluded = np.zeros(w * h)
    for i in range(w * h):
        s = ref.surface(gb, i, cam_pos)
        if s is None:
            continue
        total = (0.0, 0.0, 0.0)
        for j in range(len(scene.lights)):
            acc = (0.0, 0.0, 0.0)
            for a in range(8):
                for c in range(8):
                    e = ref.shade(scene, s, j, (a + 0.5) / 8, (c + 0.5) / 8)
                    if e["p_hat"] > 0.0:
                        acc = ref.it.add(acc, ref.it.scale(ref.it.mul(e["le"], ref.it.add(e["f_d"], e["f_s"])), e["inv_pdf"]))
            total = ref.it.add(total, ref.it.scale(acc, 1.0 / 64))
        unoccluded[i] = ref.it.lum(total)

    def run(**kw):
        hp = FullHostPass(shims, spheres, mats)
        frames = []
        for f in range(F_FRAMES):
            out_d, out_s = hp.frame(gb, w, h, cam, frame_index=f, **kw)
            frames.append(np.where(written(out_d)[:, None], out_d[:, :3].astype(np.float64) + out_s[:, :3], 0.0) @ LUM)
        return np.array(frames)
    reuse = dict(max_history=HISTORY, spatial_samples=2, spatial_radius=4.0)
    both = lambda mode: dict(temporal_bias=mode, spatial_bias=mode, **reuse)
    return dict(quad=quad, unoccluded=unoccluded, control=run(initial_samples=1, temporal=False, spatial=False),
                pairwise_uniform=run(**both(PAIRWISE)), pairwise_power=run(light_sampling=CPU_POWER, **both(PAIRWISE)),
                basic_uniform=run(**both(BASIC)), basic_power=run(light_sampling=CPU_POWER, **both(BASIC)))


def test_pairwise_is_unbiased_without_occluders(statistics):
    """test_unbiased_with_brdf_candidates' check -- F = 160 frames, batches of MaxHistoryLength = 8, the image total of the mean DI
    against the quadrature within 3 standard errors by batch means, next to the one-candidate control, which must pass it itself -- for
    Pairwise in both reuse passes with Uniform and Power_RIS candidates, on a scene whose quadrature with and without visibility agree
    (the targets carry no visibility: among occluders Pairwise is biased the way Basic is).  Basic on the same frames is printed.
    Measured (quadrature total 135.8195): control -0.3790 (standard error 0.3063); Pairwise Uniform -0.0128 (0.0619), Power_RIS +0.1773
    (0.1256); Basic Uniform -0.0996 (0.0726), Power_RIS +0.1750 (0.1276)."""
    q = statistics["quad"]
    assert q.sum() > 1.0 and np.allclose(q, statistics["unoccluded"], rtol=1e-12, atol=0), "the scene has an occluder"
    dev_c, se_c = deviation(statistics["control"], q, 1)
    print(f"quadrature total {q.sum():.4f}; control dev {dev_c:+.4f} se {se_c:.4f}")
    assert abs(dev_c) <= 3 * se_c, "the control (independent one-candidate frames) fails the check itself"
    for name in ("uniform", "power"):
        dev, se = deviation(statistics["pairwise_" + name], q, HISTORY)
        dev_b, se_b = deviation(statistics["basic_" + name], q, HISTORY)
        print(f"{name} candidates: Pairwise dev {dev:+.4f} se {se:.4f} ({abs(dev) / se:.2f} standard errors); Basic dev {dev_b:+.4f} se {se_b:.4f} ({abs(dev_b) / se_b:.2f})")
        assert abs(dev) <= 3 * se, name
        rmse = lambda frames: math.sqrt(((frames - q[None, :]) ** 2).mean())
        print(f"{name} candidates: single-frame RMSE against the quadrature, Pairwise {rmse(statistics['pairwise_' + name]):.5f} over Basic {rmse(statistics['basic_' + name]):.5f}: "
              f"{rmse(statistics['pairwise_' + name]) / rmse(statistics['basic_' + name]):.3f}")


# ---------------------------------------------------------------------------------------------------- 10. CPU: sanitizers
def test_header_paths_under_sanitizers(tmp_path):
    """tests/hostshim/restir_full_sanitize.cpp: spec S26's header paths under AddressSanitizer + UBSan as a stand-alone program"""
    import __graft_entry__ as g
    exe = g.build_restir_full_sanitizer(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "restir_full_sanitize ok" in res.stdout, res.stdout + res.stderr


# ---------------------------------------------------------------------------------------------------- GPU
GPU_POWER = sampling(POWER, tile_size=100, tile_count=3)
GPU_REGIR = sampling(REGIR, tile_size=100, tile_count=3, grid_size=4, lights_per_cell=70, cell_size=4.0)
MODES = dict(uniform=None, power=GPU_POWER, regir=GPU_REGIR)
BOTH_PAIRWISE = dict(temporal_bias=PAIRWISE, spatial_bias=PAIRWISE)


def gpu_full_frame(r, hp, w, h, cam, what, ls, cd, sh, **kw):
    """one pt_restir_di_full call (sentinel-filled outputs) against the host-compiled header fed the same G-buffer: every word of Diffuse
    and Specular, unwritten pixels included, and both slots of the history (pt_restir_di_history), the visibility word among them"""
    had_history = hp.valid and hp.size == (w, h)
    dd, ds, gb = r.restir_di_full(fill=SENTINEL, light_sampling=ls, candidates=cd, shading=sh, **kw)
    gbn = {name: gb[name].cpu().numpy().reshape(w * h, -1) for name in INPUTS}
    want_d, want_s = hp.frame(gbn, w, h, cam, light_sampling=ls, candidates=cd, shading=sh, **kw)
    got_d, got_s = dd.cpu().numpy().reshape(-1, 4), ds.cpu().numpy().reshape(-1, 4)
    for got, want, name in ((got_d, want_d, "Diffuse"), (got_s, want_s, "Specular")):
        diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {w * h} pixels differ, first {int(np.argmax(diff))}: {got[np.argmax(diff)]} != {want[np.argmax(diff)]}"
    history_equal(r, hp, w, h, 0, what)
    if had_history:
        history_equal(r, hp, w, h, 1, what)
    return written(got_d), got_d, got_s, gbn


def moving_frames(dxrs, host, r, w, h, frames):
    prev = None
    for f in range(frames):
        cam = travelling(host, w, h, f, prev)
        r.set_camera(cam)
        r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=2, spp=1))
        yield f, cam
        prev = cam


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_ragged_blocks(dxrs, host, renderer, shims, mode):
    """19 x 13: ragged 8x8 blocks on both axes.  Pairwise in both reuse passes, reuse at (4, 16), one BRDF candidate with the boiling
    filter, four frames of a travelling camera"""
    w, h = 19, 13
    spheres, mats, sd = make_scene(dxrs)
    renderer.set_scene(spheres, mats, sd)
    renderer.set_textures(None)
    hp = FullHostPass(shims, spheres, mats)
    free = 0
    for f, cam in moving_frames(dxrs, host, renderer, w, h, 4):
        gpu_full_frame(renderer, hp, w, h, cam, f"frame {f}", MODES[mode], dict(brdf_samples=1, boiling_filter=0.2), SDK_DEFAULTS, frame_index=f, reset_history=f == 0,
                       spatial_samples=2, spatial_radius=6.0, **BOTH_PAIRWISE)
        free += int(hp.rays[3])
    assert free > 0 and words(hp.slot(hp.cur)).any(), "some pixel was shaded without a final ray, and the history carries words"


@pytest.mark.gpu
def test_gpu_exact_regime_a(dxrs, host, renderer, shims):
    """MaxAge 0, MaxDistance 0 among occluders on a travelling camera: the device's outputs equal its own reuse-off outputs bit for bit
    (two contexts' worth of history: the sequence is run twice), and the host-compiled header's"""
    w, h = 40, 24
    spheres, mats, sd = make_scene(dxrs)
    renderer.set_scene(spheres, mats, sd)
    renderer.set_textures(None)
    runs = {}
    for name, sh in (("off", REUSE_OFF), ("a", dict(reuse=True, max_age=0, max_distance=0.0))):
        hp, outs, free = FullHostPass(shims, spheres, mats), [], 0
        for f, cam in moving_frames(dxrs, host, renderer, w, h, 3):
            _, d, s, _ = gpu_full_frame(renderer, hp, w, h, cam, f"{name}, frame {f}", None, None, sh, frame_index=f, reset_history=f == 0, spatial_samples=2, spatial_radius=6.0)
            outs.append((d, s))
            free += int(hp.rays[3])
        runs[name] = (outs, free)
    for f, (a, b) in enumerate(zip(runs["off"][0], runs["a"][0])):
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), f"frame {f}"
    assert runs["off"][1] == 0 and runs["a"][1] > 100


@pytest.mark.gpu
def test_gpu_scene_in_global_memory(dxrs, host, shims):
    """the 10^5-sphere tree in global memory (the wide walker), as test_restir_mis builds it: pairwise, reuse, a BRDF candidate, two frames"""
    w, h = 40, 24
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
        hp = FullHostPass(shims, spheres, mats)
        for f in range(2):
            lit, _, _, _ = gpu_full_frame(r, hp, w, h, cam, f"frame {f}", GPU_POWER, dict(brdf_samples=1, boiling_filter=0.2), SDK_DEFAULTS, frame_index=f, reset_history=f == 0,
                                          **BOTH_PAIRWISE)
            assert lit.sum() > 4, f"frame {f}: the emitters light {int(lit.sum())} pixels"
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_textured_emitter_and_alpha_mapped_blocker(dxrs, host, renderer, shims):
    """test_restir_mis's textured scene (an emissive map on E0, holes in the blocker's alpha), and E1 alpha-tested through a map of its
    own: its samples are always traced, the other emitters' are reused"""
    from dxrs_amd.textures import TextureSet
    w, h = 96, 64
    spheres, mats, sd = make_scene(dxrs)
    mats = mats.copy()
    mats["BaseColor"][BLOCKER, 3] = 1.0
    mats["AlphaMode"][BLOCKER] = 1
    mats["BaseColor"][2] = (1.0, 1.0, 1.0, 1.0)
    mats["AlphaMode"][2] = 1
    ts = TextureSet(len(spheres))
    yy, xx = np.mgrid[0:32, 0:64]
    checker = ((xx // 4 + yy // 4) & 1).astype(np.uint8)
    glow = np.zeros((32, 64, 4), np.uint8)
    glow[..., 0], glow[..., 1], glow[..., 2], glow[..., 3] = 255, 80 + 175 * checker, 40 + 215 * checker, 255
    holes = np.full((32, 64, 4), 255, np.uint8)
    holes[..., 3] = 255 * checker
    ts.maps[E0, 1] = ts.add_image(glow)
    ts.maps[BLOCKER, 0] = ts.add_image(holes)
    ts.maps[2, 0] = ts.add_image(np.full((8, 8, 4), 255, np.uint8))
    cam = host.camera_matrices(w, h, **CAM)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h, textures=ts)
    hp = FullHostPass(shims, spheres, mats, textures=ts)
    try:
        free = 0
        for f in range(2):
            gpu_full_frame(renderer, hp, w, h, cam, f"frame {f}", None, dict(brdf_samples=1, boiling_filter=0.2), SDK_DEFAULTS, frame_index=f, reset_history=f == 0,
                           spatial_samples=2, temporal_bias=PAIRWISE, spatial_bias=BASIC)
            free += int(hp.rays[3])
    finally:
        renderer.set_textures(None)
    assert free > 100


@pytest.mark.gpu
def test_gpu_entry_points_and_state(dxrs, host, renderer, shims):
    """extras off equals pt_restir_di_ex; the four entry points alternate on one context over one history (the three older ones write the
    word as 0); spheres moved by pt_update_spheres keep the history; a scene without emitters writes nothing"""
    w, h = 40, 24
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, **CAM)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = FullHostPass(shims, spheres, mats)
    ex = dict(brdf_samples=1, boiling_filter=0.2)

    def frame(f, what, ls, cd, sh, **kw):
        """through the binding's own choice of entry point (shading None: one of the three older ones), each against the one host model"""
        dd, ds, gb = renderer.restir_di(fill=SENTINEL, light_sampling=ls, candidates=cd, shading=sh, frame_index=f, reset_history=f == 0, spatial_samples=2, **kw)
        gbn = {name: gb[name].cpu().numpy().reshape(w * h, -1) for name in INPUTS}
        want_d, want_s = hp.frame(gbn, w, h, cam, light_sampling=ls, candidates=cd, shading=sh, frame_index=f, reset_history=f == 0, spatial_samples=2, **kw)
        assert same_bits(dd.cpu().numpy().reshape(-1, 4), want_d) and same_bits(ds.cpu().numpy().reshape(-1, 4), want_s), what
        history_equal(renderer, hp, w, h, 0, what)
        if f > 0:
            history_equal(renderer, hp, w, h, 1, what)
        return dd.cpu().numpy(), ds.cpu().numpy()
    frame(0, "pt_restir_di_full", GPU_POWER, ex, SDK_DEFAULTS, **BOTH_PAIRWISE)
    assert words(hp.slot(hp.cur)).any()
    frame(1, "pt_restir_di", None, None, None)
    assert not words(hp.slot(hp.cur)).any()
    frame(2, "pt_restir_di_full after a call that left no words", None, None, SDK_DEFAULTS, spatial_bias=PAIRWISE)
    frame(3, "pt_restir_di_sampled", GPU_REGIR, None, None)
    frame(4, "pt_restir_di_full, pairwise temporal alone", GPU_REGIR, None, {}, temporal_bias=PAIRWISE)
    frame(5, "pt_restir_di_ex", GPU_POWER, ex, None, temporal_bias=RAYTRACED)
    a = frame(6, "pt_restir_di_full, extras off", GPU_POWER, ex, {}, temporal_bias=RAYTRACED)
    # ... which is pt_restir_di_ex: the same call on the same history through the other entry point gives the same bits
    other = dxrs.Renderer(device=0)
    try:
        gpu_setup(other, dxrs, spheres, mats, sd, cam, w, h)
        outs = {}
        for name, sh in (("ex", None), ("full", dict(reuse=False, max_age=4, max_distance=16.0))):
            for f in range(2):
                dd, ds, _ = other.restir_di(fill=SENTINEL, light_sampling=GPU_POWER, candidates=ex, shading=sh, frame_index=f, reset_history=f == 0, spatial_samples=2)
            outs[name] = (dd.cpu().numpy(), ds.cpu().numpy(), other.restir_di_history(w, h, 0), other.restir_di_history(w, h, 1))
        assert same_bits(outs["ex"][0], outs["full"][0]) and same_bits(outs["ex"][1], outs["full"][1])
        for k in (2, 3):
            assert same_bits(outs["ex"][k][0], outs["full"][k][0]) and same_bits(outs["ex"][k][1], outs["full"][k][1])
    finally:
        other.close()
    # moved spheres keep the history
    moved = spheres.copy()
    moved["cy"][1:] += 0.05
    moved["cx"][E0] += 0.5
    renderer.update_spheres(moved)
    hp.spheres = np.ascontiguousarray(moved)
    frame(7, "moved", GPU_POWER, ex, SDK_DEFAULTS, **BOTH_PAIRWISE)
    frame(8, "moved, next", GPU_POWER, ex, SDK_DEFAULTS, **BOTH_PAIRWISE)
    assert (hp.slot(hp.cur)[6][:, 0] > 9).any(), "the history ran on"
    dark = mats.copy()
    dark["EmissiveStrength"] = 0.0
    gpu_setup(renderer, dxrs, spheres, dark, sd, cam, w, h)
    dd, ds, _ = renderer.restir_di_full(fill=SENTINEL, candidates=ex, light_sampling=GPU_REGIR, shading=SDK_DEFAULTS, **BOTH_PAIRWISE)
    for t in (dd, ds):
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_argument_errors_leave_outputs_and_history_untouched(dxrs, host, renderer, shims):
    import torch
    w, h = 40, 24
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, **CAM)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = FullHostPass(shims, spheres, mats)
    gpu_full_frame(renderer, hp, w, h, cam, "first", None, None, SDK_DEFAULTS, frame_index=0, reset_history=True, **BOTH_PAIRWISE)
    before = renderer.restir_di_history(w, h, 0)
    from dxrs_amd.abi_types import GBUFFER_CHANNELS, PtRestirDiCandidates, PtRestirDiSettings, PtRestirDiShading, PtRestirDiTextures
    width = dict(GBUFFER_CHANNELS)
    gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS}
    out = torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({n: b.data_ptr() for n, b in gb.items()})
    renderer.synchronize()
    lib, ctx = renderer._lib, renderer._ctx
    lib.pt_last_error.restype = C.c_char_p
    s = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h), FrameIndex=1, EnableTemporal=1, EnableSpatial=1, TemporalBiasCorrection=PAIRWISE, SpatialBiasCorrection=PAIRWISE)
    t = PtRestirDiTextures(**dict({n: C.c_void_p(b.data_ptr()) for n, b in gb.items()}, Diffuse=C.c_void_p(out[0].data_ptr()), Specular=C.c_void_p(out[1].data_ptr())))
    INVALID, UNSUPPORTED = 1, 5
    status = lambda **fields: lib.pt_restir_di_full(ctx, C.byref(s), None, None, C.byref(PtRestirDiShading(**fields)), C.byref(t))
    assert lib.pt_restir_di_full(ctx, None, None, None, None, None) == INVALID and lib.pt_restir_di_full(ctx, C.byref(s), None, None, None, None) == INVALID
    assert status(ReuseFinalVisibility=2) == INVALID and status(ReuseFinalVisibility=1, FinalVisibilityMaxAge=256) == INVALID and status(_pad=1) == INVALID
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert status(ReuseFinalVisibility=1, FinalVisibilityMaxDistance=bad) == INVALID, bad
    assert lib.pt_restir_di_full(ctx, C.byref(s), None, C.byref(PtRestirDiCandidates(BrdfSamples=9)), None, C.byref(t)) == INVALID  # the siblings' errors hold
    s_bad = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h), TemporalBiasCorrection=4)
    assert lib.pt_restir_di_full(ctx, C.byref(s_bad), None, None, None, C.byref(t)) == INVALID
    # the three older entry points keep refusing mode 2, and say where it runs
    for call in (lambda: lib.pt_restir_di(ctx, C.byref(s), C.byref(t)), lambda: lib.pt_restir_di_sampled(ctx, C.byref(s), None, C.byref(t)),
                 lambda: lib.pt_restir_di_ex(ctx, C.byref(s), None, None, C.byref(t))):
        assert call() == UNSUPPORTED and b"pt_restir_di_full" in lib.pt_last_error(ctx)
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    after = renderer.restir_di_history(w, h, 0)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]), "a rejected call touched the history"
    assert status(ReuseFinalVisibility=1, FinalVisibilityMaxAge=255, FinalVisibilityMaxDistance=0.0) == 0
    assert lib.pt_restir_di_full(ctx, C.byref(s), None, None, None, C.byref(t)) == 0  # NULL shading with mode 2
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) != SENTINEL.view(np.uint32)).any()


def chain(dxrs, host, sync):
    """the default frame's chain with the fourth entry point: three frames of gbuffer -> restir_di_full (pairwise, reuse at (4, 16), a
    BRDF candidate, the filter) -> sharc_ex(DI, mode 1, the NRD outputs named as the DI buffers) -> ray reconstruction at 96 x 64 on a
    context with three lanes; sync: a device synchronise after every call"""
    import torch
    from dxrs_amd.abi_types import RESTIR_DI_INPUTS
    from test_sharc import defaults
    w, h, Wo, Ho = 96, 64, 192, 128
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
        for f in range(3):
            cam = host.camera_matrices(w, h, position=(0.1 * f, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter_index=f, jitter_count=32, previous=prev)
            prev = cam
            r.set_camera(cam)
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=6, spp=1))
            ptrs = {n: b.data_ptr() for n, b in gb.items()}
            r.render_gbuffer_device(ptrs)
            wait()
            r.restir_di_device(w, h, dict({n: ptrs[n] for n in RESTIR_DI_INPUTS}, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), frame_index=f, reset_history=f == 0,
                               candidates=dict(brdf_samples=1, boiling_filter=0.2), shading=SDK_DEFAULTS, **BOTH_PAIRWISE)
            wait()
            r.render_sharc_ex_device(color.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, 1,
                                     dict(SpecularHitDistance=shd.data_ptr(), Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), **defaults(reset_history=f == 0, scene_scale=5.0))
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
        return results
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_default_frame_chain_queued_equals_synchronised(dxrs, host):
    queued, synced = chain(dxrs, host, False), chain(dxrs, host, True)
    for f in range(3):
        for name, a, b in zip(("Diffuse", "Specular", "Color", "SpecularHitDistance", "Output"), queued[f], synced[f]):
            assert same_bits(a, b), f"frame {f}: {name} differs"
        dd, ds, color, shd, output = queued[f]
        assert (dd[..., :3] > 0).any() and np.isfinite(output).all() and output[..., :3].max() > 0


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, shims, tmp_path):
    """RTXDI (host/RTXDI.hpp) from C++: after the SetConstants overload that takes ShadingSettings, Render() accepts Pairwise and runs
    pt_restir_di_full -- three frames of the demo scene with Pairwise in both passes and reuse at the mirror's defaults turned on give
    the host-compiled header's bits; after the old overload Pairwise still throws"""
    from types import SimpleNamespace
    from test_restir_pass import WIDTH
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_restir_full")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_restir_full.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h, frames = 96, 64, 3
    outp = str(tmp_path / "restir_full.f32")
    res = subprocess.run([exe, str(w), str(h), str(frames), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout and "pt_restir_di_full" in res.stdout
    data = np.fromfile(outp, dtype=np.float32)
    n = w * h
    per_frame = 6 + n * (sum(WIDTH.values()) + 16)
    assert len(data) == frames * per_frame
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    hp = FullHostPass(shims, spheres, mats)
    lit = 0
    for f in range(frames):
        d = data[f * per_frame:(f + 1) * per_frame]
        cam = SimpleNamespace(Position=d[0:3], PreviousPosition=d[3:6])
        before_d, before_s = d[6:6 + 4 * n].reshape(n, 4), d[6 + 4 * n:6 + 8 * n].reshape(n, 4)
        at, gb = 6 + 8 * n, {}
        for name in INPUTS:
            gb[name] = d[at:at + n * WIDTH[name]].reshape(n, WIDTH[name])
            at += n * WIDTH[name]
        got_d, got_s = d[at:at + 4 * n].reshape(n, 4), d[at + 4 * n:at + 8 * n].reshape(n, 4)
        want_d, want_s = hp.frame(gb, w, h, cam, frame_index=f, reset_history=f == 0, spatial_samples=2, shading=SDK_DEFAULTS, **BOTH_PAIRWISE)
        lit_f = written(want_d)
        lit += int(lit_f.sum())
        for got, want, before, name in ((got_d, want_d, before_d, "Diffuse"), (got_s, want_s, before_s, "Specular")):
            expect = np.where(lit_f[:, None], want, before)
            assert np.array_equal(got.view(np.uint32), expect.view(np.uint32)), f"frame {f} {name}"
    assert lit > 0
