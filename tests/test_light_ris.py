"""Row N16 -- pt_restir_di_sampled: Power_RIS and ReGIR local-light presampling in front of the reservoir pass (DESIGN.md spec S22).
CPU: the host-compiled headers (tests/hostshim/lightris_host.cpp over csrc/pt_lightris.h and csrc/pt_restir.h) against the float64
restatement (light_ris_reference.py) and known answers -- the pyramid, the Power segment, the ReGIR grid, initial sampling in the three
modes, unbiasedness against the quadrature of the direct-light integral, the noise against uniform candidates.  GPU: what the kernels
built (pt_light_ris_download) and whole calls against the host-compiled headers bit for bit, the identity of Mode 0 with pt_restir_di,
emitters that move, lanes, argument errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import light_ris_reference as lref
import restir_reference as ref
from test_restir_pass import (BASIC, GROUND, H, INPUTS, SENTINEL, W, HostPass, cpu_gbuffer, deviation, gpu_setup, make_scene, reservoirs, settings)

U = 2.0 ** -24  # unit roundoff of float32
ENTRY = np.dtype([("light", "<u4"), ("inv_pdf", "<f4")])
INVALID = 0xFFFFFFFF
UNIFORM, POWER, REGIR = 0, 1, 2
# the share of entries (or pixels) a comparison with the restatement may exclude because a discrete choice sits within rounding of
# its threshold: at most 0.1 %, for the header's choices and for the restatement's own draws alike
MAX_EXCLUDED = 0.001


def sampling(mode, **kw):
    """PtLightSamplingSettings with its defaults applied (0 -> default)"""
    s = dict(mode=mode, tile_size=1024, tile_count=128, grid_size=16, lights_per_cell=512, build_samples=8, cell_size=1.0)
    s.update(kw)
    return s


# ---------------------------------------------------------------------------------------------------- the host-compiled headers
@pytest.fixture(scope="module")
def shims():
    import __graft_entry__ as g

    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    lr = C.CDLL(g.build_lightris_shim())
    for name, res, args in (("lr_host_lights", u32, [vp, u32, vp]), ("lr_host_levels", u32, [u32]), ("lr_host_pyramid_floats", u32, [u32]),
                            ("lr_host_level_offset", u32, [u32, u32]), ("lr_host_pyramid_from_powers", None, [vp, u32, vp]),
                            ("lr_host_powers", None, [vp, vp, u32, vp]), ("lr_host_power_segment", None, [vp, u32, u32, u32, u32, vp]),
                            ("lr_host_regir_segment", None, [vp, vp, u32, vp, vp, vp, vp]), ("lr_host_volume_target", f32, [vp, vp, u32, u32, vp, f32]),
                            ("lr_host_cell_centre", None, [vp, u32, f32, u32, vp]), ("lr_host_cell_of", u32, [vp, vp, vp, u32, f32]),
                            ("lr_host_call", None, [vp, vp, u32, vp, vp, vp, vp, f32, vp, vp])):
        getattr(lr, name).restype, getattr(lr, name).argtypes = res, args
    ri = C.CDLL(g.build_restir_shim())
    ri.ri_host_call.restype = None
    ri.ri_host_call.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp]
    gb = C.CDLL(g.build_gbuffer_shim())
    gb.gb_pixels.restype = None
    gb.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    gb.gb_srgb_lut.restype = None
    gb.gb_srgb_lut.argtypes = [vp]
    return lr, ri, gb


def host_pyramid(lr, powers):
    powers = np.ascontiguousarray(powers, np.float32)
    out = np.full(lr.lr_host_pyramid_floats(len(powers)), np.nan, np.float32)
    lr.lr_host_pyramid_from_powers(powers.ctypes.data, len(powers), out.ctypes.data)
    return out


def pyramid_levels(lr, pyr, n):
    lv = lr.lr_host_levels(n)
    return [pyr[lr.lr_host_level_offset(lv, k):lr.lr_host_level_offset(lv, k) + 4 ** (lv - k)] for k in range(lv + 1)]


def host_power_segment(lr, pyr, n, tile_size, tile_count, frame):
    out = np.zeros(tile_size * tile_count, ENTRY)
    lr.lr_host_power_segment(pyr.ctypes.data, n, tile_size, tile_count, frame, out.ctypes.data)
    return out


def host_regir_segment(lr, spheres, mats, power, cam_pos, frame, s):
    spheres, mats = np.ascontiguousarray(spheres), np.ascontiguousarray(mats)
    iprm = np.array([s["grid_size"], s["lights_per_cell"], s["build_samples"], s["tile_size"], s["tile_count"], frame], np.uint32)
    fprm = np.array([s["cell_size"], *cam_pos], np.float32)
    out = np.zeros(s["grid_size"] ** 3 * s["lights_per_cell"], ENTRY)
    lr.lr_host_regir_segment(spheres.ctypes.data, mats.ctypes.data, len(spheres), power.ctypes.data, iprm.ctypes.data, fprm.ctypes.data, out.ctypes.data)
    return out


def host_structures(lr, spheres, mats, cam_pos, frame, s):
    """what one call builds: (pyramid, entries) as pt_light_ris_download returns them"""
    spheres, mats = np.ascontiguousarray(spheres), np.ascontiguousarray(mats)
    n = lr.lr_host_lights(mats.ctypes.data, len(mats), None)
    powers = np.zeros(n, np.float32)
    lr.lr_host_powers(spheres.ctypes.data, mats.ctypes.data, len(spheres), powers.ctypes.data)
    pyr = host_pyramid(lr, powers)
    power = host_power_segment(lr, pyr, n, s["tile_size"], s["tile_count"], frame)
    if s["mode"] != REGIR:
        return pyr, power
    return pyr, np.concatenate([power, host_regir_segment(lr, spheres, mats, power, cam_pos, frame, s)])


class SampledHostPass(HostPass):
    """pt_restir_di_sampled over the host-compiled headers: HostPass's history slots and restart rules, lr_host_call in place of
    ri_host_call (untextured scenes); `built` = (pyramid, entries) of the last call with a presampling mode"""

    def __init__(self, shims, spheres, mats):
        super().__init__(shims[0], shims[2], spheres, mats)
        self.built = None

    def call(self, gb, w, h, cam, out_d, out_s, launches=3, light_sampling=None, **kw):
        s = settings(**kw)
        ls = light_sampling or sampling(UNIFORM)
        n = w * h
        if self.size != (w, h):
            self.slots = [[np.zeros((n, 4), np.float32) for _ in range(4)] + [np.zeros(n, np.float32)] + [np.zeros((n, 4), np.float32) for _ in range(2)]
                          for _ in range(2)]
            self.size, self.valid = (w, h), False
        restart = s["reset_history"] or not self.valid
        cur, prev = self.cur ^ 1, self.cur
        prm = np.array([w, h, s["frame_index"], s["initial_samples"], int(s["temporal"]), s["temporal_bias"], s["max_history"], int(s["spatial"]),
                        s["spatial_bias"], s["spatial_samples"], 0 if restart else 1, launches], np.uint32)
        fprm = np.array([s["spatial_radius"], *cam.Position, *cam.PreviousPosition], np.float32)
        sprm = np.array([ls["mode"], ls["tile_size"], ls["tile_count"], ls["grid_size"], ls["lights_per_cell"], ls["build_samples"]], np.uint32)
        arrays = [np.ascontiguousarray(gb[name], dtype=np.float32) for name in INPUTS] + self.slots[cur] + self.slots[prev] + [out_d, out_s]
        ptrs = (C.c_void_p * 24)(*[a.ctypes.data for a in arrays])
        pyr = ris = None
        if ls["mode"] != UNIFORM:
            n_lights = self.lib.lr_host_lights(self.mats.ctypes.data, len(self.mats), None)
            pyr = np.zeros(self.lib.lr_host_pyramid_floats(n_lights), np.float32)
            ris = np.zeros(ls["tile_size"] * ls["tile_count"] + (ls["grid_size"] ** 3 * ls["lights_per_cell"] if ls["mode"] == REGIR else 0), ENTRY)
        p = lambda a: a.ctypes.data if a is not None else None
        self.lib.lr_host_call(p(self.spheres), p(self.mats), len(self.spheres), p(prm), p(fprm), ptrs, p(sprm), ls["cell_size"], p(pyr), p(ris))
        self.cur, self.valid = cur, True
        if pyr is not None:
            self.built = (pyr, ris)
        return self.slots[cur]


def least(margins, kind):
    """the smallest margin of one kind among light_ris_reference's (kind, margin) records"""
    return min((m for k, m in margins if k == kind), default=math.inf)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------------- CPU: ABI
def test_abi_without_gpu(dxrs):
    """Symbols, layout and the null context.  The message of each range violation needs a context, and a context needs a device: those
    are checked in test_gpu_misuse."""
    lib = dxrs.load_hip().lib
    for name in ("pt_restir_di_sampled", "pt_restir_di_history", "pt_light_ris_download"):
        assert hasattr(lib, name) and name in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtLightSamplingSettings, PtRestirDiSettings, PtRestirDiTextures
    S = PtLightSamplingSettings
    assert C.sizeof(S) == 32
    assert [getattr(S, f).offset for f in ("Mode", "TileSize", "TileCount", "ReGIRGridSize", "ReGIRLightsPerCell", "ReGIRBuildSamples", "ReGIRCellSize", "_pad")] == [
        0, 4, 8, 12, 16, 20, 24, 28]
    assert C.sizeof(PtRestirDiSettings) == 48  # pt_restir_di keeps its settings
    s, ls, t = PtRestirDiSettings(), S(), PtRestirDiTextures()
    assert lib.pt_restir_di_sampled(None, C.byref(s), C.byref(ls), C.byref(t)) == 1  # PT_ERR_INVALID_ARG: null context
    n = C.c_uint32(0)
    assert lib.pt_light_ris_download(None, None, C.byref(n), None, C.byref(n)) == 1
    assert lib.pt_restir_di_history(None, 0, None, None) == 1


def test_headers_under_sanitizers(tmp_path):
    """tests/cpp/lightris_sanitize.cpp: pt_lightris.h and pt_restir.h's initial sampling under AddressSanitizer + UBSan as a stand-alone
    program (exact-size heap arrays around every level, tile and cell; whole calls in the three modes)"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "lightris_sanitize")
    build = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(here, "cpp", "lightris_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "lightris_sanitize ok" in res.stdout, res.stdout + res.stderr


# ---------------------------------------------------------------------------------------------------- CPU: the pyramid
def spread_powers(n, seed, decades=6.5):
    """n positive float32 powers spanning `decades` decades"""
    rng = np.random.default_rng(seed)
    p = (10.0 ** (rng.random(n) * decades - 2.0)).astype(np.float32)
    if n > 1:
        p[0], p[-1] = np.float32(10.0 ** -2.0), np.float32(10.0 ** (decades - 2.0))
    return p


@pytest.mark.parametrize("n", [1, 2, 4, 5, 16, 17, 1023, 1024, 1025, 4097])
def test_pyramid(shims, n):
    lr = shims[0]
    powers = spread_powers(n, n)
    lv = lr.lr_host_levels(n)
    assert 4 ** lv >= n and (lv == 0 or 4 ** (lv - 1) < n)
    pyr = host_pyramid(lr, powers)
    assert len(pyr) == (4 ** (lv + 1) - 1) // 3 and lref.levels(n) == lv
    lev = pyramid_levels(lr, pyr, n)
    assert same_bits(lev[0][:n], powers), "leaf j holds power_j"
    assert (lev[0][n:].view(np.uint32) == 0).all(), "padding leaves are +0"
    for k in range(lv):
        q = lev[k].reshape(-1, 4)
        want = (((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]) * np.float32(0.25)  # float32 throughout: numpy does not contract or widen
        assert want.dtype == np.float32 and same_bits(lev[k + 1], want), f"level {k + 1}"
    # top * 4^Lv against the float64 sum: a path from a leaf to the top passes Lv parents of three float32 additions of non-negative
    # terms each (the multiplications by 0.25 and 4^Lv are exact): relative error at most (1 + U)^(3 Lv) - 1
    total = float(powers.astype(np.float64).sum())
    got = float(lev[lv][0]) * 4.0 ** lv
    bound = (1.0 + U) ** (3 * lv) - 1.0
    print(f"n = {n}: Lv = {lv}, top 4^Lv / sum - 1 = {got / total - 1.0:+.3e}, bound {bound:.3e}")
    assert abs(got - total) <= bound * total
    # ... and the float64 restatement's pyramid within the same bound, level by level
    want64 = lref.pyramid([float(x) for x in powers])
    for k in range(lv + 1):
        assert np.all(np.abs(lev[k].astype(np.float64) - np.array(want64[k])) <= ((1.0 + U) ** (3 * k) - 1.0) * np.array(want64[k])), f"level {k}"


def test_light_power_of_a_scene(dxrs, shims):
    """power_j = r^2 luminance(Le): four products and a three-term dot product away from float64, (1 + U)^8 - 1"""
    lr = shims[0]
    spheres, mats, sd = make_scene(dxrs)
    scene = ref.Scene(spheres, mats)
    n = lr.lr_host_lights(mats.ctypes.data, len(mats), None)
    lights = np.zeros(n, np.uint32)
    lr.lr_host_lights(mats.ctypes.data, len(mats), lights.ctypes.data)
    assert list(lights) == scene.lights and n == 3
    powers = np.zeros(n, np.float32)
    lr.lr_host_powers(spheres.ctypes.data, mats.ctypes.data, len(spheres), powers.ctypes.data)
    for j in range(n):
        want = lref.power(scene, j)
        assert want > 0 and abs(float(powers[j]) - want) <= ((1.0 + U) ** 8 - 1.0) * want


# ---------------------------------------------------------------------------------------------------- CPU: the Power segment
def test_power_segment_against_restatement(shims):
    """Unequal powers over 6.5 decades (3 162 000 : 1), n = 37 (Lv = 3), 8 tiles of 256.
    invSourcePdf power_j / sum(power) = 1: the walk's pdf is the product over Lv levels of q_k / sum, where `sum` is bitwise four times
    the stored parent, so the stored values telescope exactly to leaf / (4^Lv top); what remains is Lv divisions, Lv products (the first,
    by 1, exact), the reciprocal, and the 3 Lv additions between 4^Lv top and the true sum: (1 + U)^(5 Lv + 1) - 1.
    Against the restatement the chosen child may differ only where u = rng sum lies within rounding of a prefix sum: a float32 prefix
    differs from its float64 value by at most (3 Lv + 2) U sum, u by (3 Lv + 4) U sum, so only where |u - prefix| <= (6 Lv + 6) U sum."""
    lr = shims[0]
    n, tile_size, tile_count, frame = 37, 256, 8, 11
    powers = spread_powers(n, 7)
    assert powers.max() / powers.min() >= 1e6
    lv = lr.lr_host_levels(n)
    pyr = host_pyramid(lr, powers)
    seg = host_power_segment(lr, pyr, n, tile_size, tile_count, frame)
    total = float(powers.astype(np.float64).sum())
    assert (seg["light"] < n).all(), "an entry is a real emitter: padding leaves weigh nothing"
    bound = (1.0 + U) ** (5 * lv + 1) - 1.0
    ratio = seg["inv_pdf"].astype(np.float64) * powers[seg["light"]].astype(np.float64) / total
    print(f"max |invSourcePdf power / sum - 1| = {np.abs(ratio - 1.0).max():.3e}, bound {bound:.3e}")
    assert np.abs(ratio - 1.0).max() <= bound
    pyr64 = lref.pyramid([float(x) for x in powers])
    near_bound = (6 * lv + 6) * U
    excluded = near_alone = 0
    for t in range(tile_count):
        for s in range(tile_size):
            margins = []
            j, inv = lref.power_entry(pyr64, t, s, frame, margins)
            near = least(margins, "child") <= near_bound
            near_alone += near
            got = seg[t * tile_size + s]
            if int(got["light"]) != j:
                assert near, f"entry ({t}, {s}): leaf {got['light']} != {j} away from every boundary"
                excluded += 1
                continue
            assert abs(float(got["inv_pdf"]) - inv) <= bound * inv
    print(f"entries whose leaf differs: {excluded}; near a boundary in the restatement alone: {near_alone} of {len(seg)}")
    assert near_alone <= MAX_EXCLUDED * len(seg), "the powers and the seed put too many of the restatement's own draws near a boundary"
    assert excluded <= MAX_EXCLUDED * len(seg)


def test_power_segment_known_answers(shims):
    lr = shims[0]
    one = host_power_segment(lr, host_pyramid(lr, [3.5]), 1, 100, 3, 4)
    assert (one["light"] == 0).all() and same_bits(one["inv_pdf"], np.ones(300, np.float32)), "n = 1: every entry is {0, 1.0f}"
    for k in (1, 2, 3):  # 4^k equal powers: every quotient is exactly 1/4
        n = 4 ** k
        seg = host_power_segment(lr, host_pyramid(lr, np.full(n, 0.3, np.float32)), n, 64, 4, k)
        assert same_bits(seg["inv_pdf"], np.full(256, n, np.float32)) and len(np.unique(seg["light"])) == n
    # a zero-weight emitter is never chosen, and a pyramid of zeros yields invalid entries
    seg = host_power_segment(lr, host_pyramid(lr, [0.0, 2.0, 0.0, 1.0, 0.0]), 5, 64, 4, 0)
    assert set(np.unique(seg["light"])) == {1, 3}
    seg = host_power_segment(lr, host_pyramid(lr, [0.0, 0.0]), 2, 16, 1, 0)
    assert (seg["light"] == INVALID).all() and (seg["inv_pdf"] == 0).all()


def test_power_segment_frequencies(shims):
    """one default-size segment (128 tiles of 1024 = 131 072 entries), n = 5: each emitter's share within 5 binomial standard errors of
    power_j / sum (the bound of row N14's statistical test)"""
    lr = shims[0]
    powers = np.array([1.0, 40.0, 0.25, 8.0, 3.0], np.float32)
    seg = host_power_segment(lr, host_pyramid(lr, powers), 5, 1024, 128, 2)
    assert len(seg) == 131072 and (seg["light"] < 5).all()
    p = powers.astype(np.float64) / powers.astype(np.float64).sum()
    for j in range(5):
        share = float((seg["light"] == j).mean())
        se = math.sqrt(p[j] * (1.0 - p[j]) / len(seg))
        print(f"emitter {j}: share {share:.5f}, expected {p[j]:.5f}, {abs(share - p[j]) / se:.2f} standard errors")
        assert abs(share - p[j]) <= 5.0 * se


# ---------------------------------------------------------------------------------------------------- CPU: ReGIR
def cell_of(lr, P, xi, cam, grid, cell_size):
    a = [np.array(v, np.float32) for v in (P, xi, cam)]
    return lr.lr_host_cell_of(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, grid, cell_size)


def test_regir_cell_index_known_answers(shims):
    lr = shims[0]
    cam, mid = (1.5, -2.0, 7.25), (0.5, 0.5, 0.5)  # xi = 0.5: no jitter
    for grid, cs in ((16, 1.0), (2, 0.5), (4, 2.5)):
        h = grid // 2
        assert cell_of(lr, cam, mid, cam, grid, cs) == (h * grid + h) * grid + h, "P at the camera: cell G / 2 on each axis"
        assert lref.cell_of(cam, mid, cam, grid, cs) == (h * grid + h) * grid + h
        for axis in range(3):
            for sign in (-1.0, 1.0):
                P = list(cam)
                P[axis] += sign * (grid / 2 + 0.5) * cs  # half a cell outside the face
                assert cell_of(lr, P, mid, cam, grid, cs) == INVALID and lref.cell_of(P, mid, cam, grid, cs) is None
                P[axis] = cam[axis] + sign * (grid / 2 - 0.5) * cs  # the centre of the last cell inside it
                want = [h, h, h]
                want[axis] = grid - 1 if sign > 0 else 0
                assert cell_of(lr, P, mid, cam, grid, cs) == (want[2] * grid + want[1]) * grid + want[0]
    # an odd grid: the camera sits at the centre of the middle cell
    centre = np.zeros(3, np.float32)
    c = np.array(cam, np.float32)
    assert cell_of(lr, cam, mid, cam, 3, 1.0) == (1 * 3 + 1) * 3 + 1
    lr.lr_host_cell_centre(c.ctypes.data, 3, 2.0, 13, centre.ctypes.data)
    assert same_bits(centre, c)
    # the jitter moves a point by at most half a cell: xi = 1 carries the centre of a cell onto its upper face, into the next cell
    assert cell_of(lr, (cam[0] + 0.5, cam[1] + 0.5, cam[2] + 0.5), (1.0, 1.0, 1.0), cam, 4, 1.0) == (3 * 4 + 3) * 4 + 3


def test_regir_volume_target_against_float64(dxrs, shims):
    """about 25 float32 roundings, none of them cancelling except C - centre, whose error U |C| enters dist >= 0.75 R (dist at d = 0)
    as at most 2 U |C| / (0.75 R) after the square: bound (32 + 4 max|C| / (0.75 R)) U"""
    lr = shims[0]
    spheres, mats, sd = make_scene(dxrs)
    scene = ref.Scene(spheres, mats)
    checked = 0
    for cs in (0.1, 1.0, 2.5, 10.0):
        R = math.sqrt(3.0) * cs
        for centre in ((0.0, 0.0, 0.0), (-3.0, 3.0, 0.5), (4.5, -1.5, 12.0), (0.5, 5.0, 3.0 + 1e-3)):
            c = np.array(centre, np.float32)
            for j in range(3):
                got = lr.lr_host_volume_target(spheres.ctypes.data, mats.ctypes.data, len(spheres), j, c.ctypes.data, cs)
                want = lref.volume_target(scene, j, tuple(float(x) for x in c), float(np.float32(cs)))
                reach = max(abs(x) for x in scene.spheres[scene.lights[j]][:3] + tuple(centre))
                assert want > 0 and abs(got - want) <= (32 + 4 * reach / (0.75 * R)) * U * want, (cs, centre, j, got, want)
                checked += 1
    assert checked == 48


def regir_case(dxrs, lr, build_samples, frame):
    spheres, mats, sd = make_scene(dxrs)
    s = sampling(REGIR, tile_size=100, tile_count=3, grid_size=2, lights_per_cell=70, build_samples=build_samples, cell_size=2.5)
    cam_pos = (0.25, 2.5, -1.0)
    pyr, entries = host_structures(lr, spheres, mats, cam_pos, frame, s)
    n_power = s["tile_size"] * s["tile_count"]
    return ref.Scene(spheres, mats), s, cam_pos, entries[:n_power], entries[n_power:]


def test_regir_one_build_sample_keeps_the_tile_entrys_pdf(dxrs, shims):
    """BuildSamples = 1: w_sum = target inv, the entry's invSourcePdf = w_sum / (1 target): the tile entry's within two roundings"""
    lr = shims[0]
    scene, s, cam_pos, power, regir = regir_case(dxrs, lr, 1, 5)
    assert len(regir) == 8 * 70
    checked = excluded = 0
    for g in range(len(regir)):
        margins = []
        tile = lref.regir_tile(g, 5, s["tile_count"], margins)
        rng = lref.it.Stream(lref.it.rng_seed(g & 0xFFF, g >> 12, 5 ^ lref.SALT_REGIR))
        slot = lref.pick(rng.unit(), s["tile_size"], margins)
        if least(margins, "pick") <= U:
            excluded += 1
            continue
        src = power[tile * s["tile_size"] + slot]
        assert int(regir[g]["light"]) == int(src["light"]) != INVALID
        assert abs(float(regir[g]["inv_pdf"]) - float(src["inv_pdf"])) <= ((1.0 + U) ** 2 - 1.0) * float(src["inv_pdf"])
        checked += 1
    assert excluded <= MAX_EXCLUDED * len(regir) and checked > 500


def test_regir_segment_against_restatement(dxrs, shims):
    """8 build samples over the host-built Power segment.  A candidate's weight is the volume target (32 U, the test above, the emitters
    being within a few R) times the tile entry's invSourcePdf (taken from the float32 segment: exact) -- 34 U with the product -- and w_sum
    adds one rounding per candidate: the selection rnd w_sum <= w may differ only where |rnd w_sum - w| <= 2 (34 + 8) U w; the picks
    only where u n lies within U n of an integer.  The entry's value: w_sum / (8 target): (34 + 8 + 32 + 2) U."""
    lr = shims[0]
    frame = 9
    scene, s, cam_pos, power, regir = regir_case(dxrs, lr, 8, frame)
    tiles = [[(int(e["light"]), float(e["inv_pdf"])) for e in power[t * s["tile_size"]:(t + 1) * s["tile_size"]]] for t in range(s["tile_count"])]
    cam32 = tuple(float(np.float32(x)) for x in cam_pos)
    excluded = near_alone = valid = 0
    for g in range(len(regir)):
        margins = []
        tile = lref.regir_tile(g, frame, s["tile_count"], margins)
        j, inv = lref.regir_entry(scene, cam32, s["grid_size"], float(np.float32(s["cell_size"])), s["lights_per_cell"], s["build_samples"], tiles[tile], g, frame, margins)
        near = least(margins, "pick") <= U or least(margins, "ris") <= 2 * 42 * U
        near_alone += near
        got = regir[g]
        if int(got["light"]) != j:
            assert near, f"slot {g}: emitter {got['light']} != {j} away from every threshold"
            excluded += 1
            continue
        valid += j != INVALID
        assert abs(float(got["inv_pdf"]) - inv) <= 76 * U * inv, (g, got, inv)
    print(f"slots whose choice differs: {excluded}; near a threshold in the restatement alone: {near_alone} of {len(regir)}")
    assert valid > 500
    assert near_alone <= MAX_EXCLUDED * len(regir) and excluded <= MAX_EXCLUDED * len(regir)
    # the cells differ: a cell nearer to an emitter holds it more often
    share = lambda cell, j: float((regir[cell * 70:(cell + 1) * 70]["light"] == j).mean())
    assert len({tuple(round(share(c, j), 3) for j in range(3)) for c in range(8)}) > 1



# ---------------------------------------------------------------------------------------------------- CPU: initial sampling
CAM = dict(position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
# the grid of the CPU tests: 8^3 cells of 2.5 around the camera reach the whole scene in front of it; small tiles keep a frame cheap
CPU_POWER = sampling(POWER, tile_size=256, tile_count=16)
CPU_REGIR = sampling(REGIR, tile_size=256, tile_count=16, grid_size=8, lights_per_cell=64, cell_size=2.5)


@pytest.fixture(scope="module")
def cpu_case(dxrs, host, oracle, shims):
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(W, H, **CAM)
    gb, ids = cpu_gbuffer((shims[1], shims[2]), oracle, cam, W, H, spheres, mats, sd)
    assert (ids == GROUND).any()
    return spheres, mats, sd, cam, gb


def frames_equal(a, b, what):
    for x, y, name in zip(a, b, ("Diffuse", "Specular")):
        assert same_bits(x, y), f"{what}: {name}"


def test_uniform_through_the_new_shim_is_the_existing_pass(shims, cpu_case):
    """Mode 0 through lr_host_call (ri_pass1_px<kLrUniform>) against ri_host_call of the existing shim (ri_pass1_px as it was called
    before): outputs and both history slots, bit for bit, over three frames with the history running"""
    spheres, mats, sd, cam, gb = cpu_case
    old, new = HostPass(shims[1], shims[2], spheres, mats), SampledHostPass(shims, spheres, mats)
    for f in range(3):
        kw = dict(frame_index=f, reset_history=f == 0, spatial_samples=2, spatial_radius=8.0)
        frames_equal(old.frame(gb, W, H, cam, **kw), new.frame(gb, W, H, cam, light_sampling=sampling(UNIFORM), **kw), f"frame {f}")
        for k in range(2):
            for a, b in zip(old.slot(k), new.slot(k)):
                assert same_bits(a, b), f"frame {f}: history slot {k}"
    assert (new.slot(new.cur)[6][:, 0] > 8).any(), "the history ran"


def test_one_emitter_power_ris_is_uniform(dxrs, host, oracle, shims):
    """one emitter: every Power_RIS entry is {0, 1.0f}, the draws are the same and the source weight is 1 = n_lights"""
    from test_restir_pass import E0
    spheres, mats, sd = make_scene(dxrs, emitters=(E0,))
    cam = host.camera_matrices(W, H, **CAM)
    gb, _ = cpu_gbuffer((shims[1], shims[2]), oracle, cam, W, H, spheres, mats, sd)
    uni, pow_ = SampledHostPass(shims, spheres, mats), SampledHostPass(shims, spheres, mats)
    for f in range(2):
        kw = dict(frame_index=f, reset_history=f == 0)
        frames_equal(uni.frame(gb, W, H, cam, **kw), pow_.frame(gb, W, H, cam, light_sampling=CPU_POWER, **kw), f"frame {f}")
        for a, b in zip(uni.slot(uni.cur), pow_.slot(pow_.cur)):
            assert same_bits(a, b), f"frame {f}: history"
    assert (pow_.built[1]["light"] == 0).all() and (pow_.built[1]["inv_pdf"] == 1.0).all()


@pytest.mark.parametrize("ls", [CPU_POWER, CPU_REGIR], ids=["power", "regir"])
def test_initial_sampling_against_restatement(shims, cpu_case, ls):
    """Launch 1 alone (no history), pixel by pixel.  The restatement draws from the float32 structures the call built (their own
    checks are above), so what is compared is initial sampling itself.  A pixel's pick may differ only where a comparison of the
    restatement sits within rounding of its threshold: an index pick within U n of an integer; a cell coordinate -- five float32
    operations on magnitudes up to M = 32 divided by the cell size, plus G / 2 -- within (5 M / cs + G) U of an integer; a stream-RIS
    step, whose weight is the target function (test_restir_pass's PASS_RTOL = 256 U) times the entry's invSourcePdf, within
    2 (256 + 8 + 2) U w.  What is held exactly is what spec S22 adds: the source of each candidate, the selected (emitter, u1, u2), M
    and whether the visibility ray kept the sample.  The values of p_hat and W are ri_shade's, which S22 does not touch and
    test_restir_pass holds to its own tolerance (their float32 error depends on how grazing the sample is, not on the source).
    With 936 surfaces the 0.1 % cap allows no exclusion at all: FrameIndex 8 is chosen so that none of the restatement's own comparisons
    sits near a threshold in either mode (at FrameIndex 6 and 7 one does)."""
    spheres, mats, sd, cam, gb = cpu_case
    scene = ref.Scene(spheres, mats)
    n, frame = W * H, 8
    hp = SampledHostPass(shims, spheres, mats)
    got = reservoirs(hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, frame_index=frame, spatial=False,
                             light_sampling=ls))
    ris = [(int(e["light"]), float(e["inv_pdf"])) for e in hp.built[1]]
    cam_pos = tuple(float(x) for x in cam.Position)
    cell_bound, ris_bound = (5 * 32 / ls["cell_size"] + ls["grid_size"]) * U, 2 * 266 * U
    valid = flipped = near_alone = lit = in_cell = 0
    for i in range(n):
        s = ref.surface(gb, i, cam_pos)
        g = got[i]
        assert (g["M"] > 0) == (s is not None)
        if s is None:
            continue
        valid += 1
        margins = []
        r = lref.initial(scene, s, i % W, i // W, frame, 8, ls["mode"], ris, ls["tile_size"], ls["tile_count"], ls["grid_size"], ls["lights_per_cell"],
                         float(np.float32(ls["cell_size"])), cam_pos, margins)
        in_cell += ls["mode"] == REGIR and lref.cell_of(s["P"], (0.5, 0.5, 0.5), cam_pos, ls["grid_size"], ls["cell_size"]) is not None
        near = least(margins, "pick") <= U or least(margins, "cell") <= cell_bound or least(margins, "ris") <= ris_bound
        near_alone += near
        if (g["light"], g["u1"], g["u2"]) != (r["light"], np.float32(r["u1"]), np.float32(r["u2"])) or (g["W"] > 0) != (r["W"] > 0):
            assert near, f"pixel {i}: the pick differs away from every threshold: {g} != {r}"
            flipped += 1
            continue
        lit += r["W"] > 0
        assert g["M"] == r["M"] == 8 and (g["p_hat"] > 0) == (r["p_hat"] > 0), (i, g, r)
    print(f"{valid} surfaces, {lit} lit, {in_cell} inside the grid; flipped {flipped}; near a threshold in the restatement alone: {near_alone}")
    assert valid > n // 3 and lit > valid // 4
    if ls["mode"] == REGIR:
        assert in_cell > valid // 2
    assert near_alone <= MAX_EXCLUDED * valid, "the seed puts too many of the restatement's own comparisons near their thresholds"
    assert flipped <= MAX_EXCLUDED * valid


# ---------------------------------------------------------------------------------------------------- CPU: unbiasedness and noise
N_FRAMES, BATCH = 96, 4
LUM = np.array([0.2126, 0.7152, 0.0722])
# the fallback case: the camera pulled back and a 2^3 grid of 8-unit cells around it, so that the near part of the ground is inside
# and the far part and the emitters' surroundings fall back to the Power_RIS tile
FALLBACK_CAM = dict(position=(0.0, 3.0, -12.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
FALLBACK_REGIR = sampling(REGIR, tile_size=256, tile_count=16, grid_size=2, lights_per_cell=64, cell_size=8.0)


def di_frames(hp, gb, w, h, cam, ls, frames, first_frame=0, **kw):
    """per-frame images of the luminance of Diffuse.rgb + Specular.rgb, temporal and spatial reuse off"""
    out = []
    for f in range(frames):
        d, s = hp.frame(gb, w, h, cam, frame_index=first_frame + f, temporal=False, spatial=False, reset_history=True, light_sampling=ls, **kw)
        out.append(np.where(d[:, :1].view(np.uint32) == SENTINEL.view(np.uint32), 0.0, d[:, :3].astype(np.float64) + s[:, :3]) @ LUM)
    return np.array(out)


def quadrature_image(scene, gb, n, cam_pos, k):
    quad = np.zeros(n)
    for i in range(n):
        s = ref.surface(gb, i, cam_pos)
        if s is not None:
            quad[i] = ref.it.lum(ref.quadrature(scene, s, k=k))
    return quad


@pytest.fixture(scope="module")
def quadratures(dxrs, host, oracle, shims, cpu_case):
    """the stratified quadrature of the direct-light integral (restir_reference.quadrature, the one test_restir_pass uses) over the
    48 x 32 view and over the fallback view: computed once, shared, left unchanged"""
    spheres, mats, sd, cam, gb = cpu_case
    scene = ref.Scene(spheres, mats)
    cam2 = host.camera_matrices(W, H, **FALLBACK_CAM)
    gb2, _ = cpu_gbuffer((shims[1], shims[2]), oracle, cam2, W, H, spheres, mats, sd)
    return dict(front=(cam, gb, quadrature_image(scene, gb, W * H, tuple(float(x) for x in cam.Position), 8)),
                fallback=(cam2, gb2, quadrature_image(scene, gb2, W * H, tuple(float(x) for x in cam2.Position), 8)))


@pytest.fixture(scope="module")
def uniform_frames(shims, cpu_case, quadratures):
    """the same frames with uniform candidates (S16 as it was), per view: an unbiased estimate of the same integral"""
    spheres, mats = cpu_case[0], cpu_case[1]
    return {view: di_frames(SampledHostPass(shims, spheres, mats), gb, W, H, cam, sampling(UNIFORM), N_FRAMES, first_frame=5000)
            for view, (cam, gb, quad) in quadratures.items()}


@pytest.mark.parametrize("view,ls", [("front", CPU_POWER), ("front", CPU_REGIR), ("fallback", FALLBACK_REGIR)], ids=["power", "regir", "regir-fallback"])
def test_unbiased_without_reuse(shims, cpu_case, quadratures, uniform_frames, view, ls):
    """N = 96 frames of 48 x 32, temporal and spatial reuse off, batches of 4: the image total of the mean DI against the quadrature,
    within 5 standard errors by batch means, the standard error below 1 % of the total (which is what N was chosen for).
    Measured (quadrature total 69.13 front, 50.44 fallback): Power_RIS -0.85 (standard error 0.26), ReGIR_RIS -0.43 (0.12), ReGIR_RIS
    with 47 % of the surfaces inside the grid -0.66 (0.20).  The k = 8 quadrature carries a discretisation error of its own of about
    this size: uniform candidates deviate from it by -0.65 (0.07 over 384 frames), one uniform candidate -- plain Monte Carlo -- by -0.72
    (0.17); so a second, sharper check holds each mode against the uniform estimate of the same frames' count, the two being
    independent: within 5 standard errors of their difference."""
    spheres, mats = cpu_case[0], cpu_case[1]
    cam, gb, quad = quadratures[view]
    if view == "fallback":
        cells = cells_of_frame(shims[0], gb, cam, ls)
        print(f"surfaces inside the grid: {cells.mean():.2f}")
        assert 0.25 <= cells.mean() <= 0.75, "about half the surfaces fall outside the grid"
    frames = di_frames(SampledHostPass(shims, spheres, mats), gb, W, H, cam, ls, N_FRAMES)
    dev, se = deviation(frames, quad, BATCH)
    dev_u, se_u = deviation(uniform_frames[view], quad, BATCH)
    print(f"quadrature total {quad.sum():.4f}; deviation {dev:+.4f}, standard error {se:.4f} ({se / quad.sum():.4%} of the total); "
          f"uniform candidates: deviation {dev_u:+.4f}, standard error {se_u:.4f}")
    assert se < 0.01 * quad.sum()
    assert abs(dev) <= 5 * se
    assert abs(dev - dev_u) <= 5 * math.hypot(se, se_u)


def strong_and_dim_scene(dxrs):
    """64 emitters of equal radius over a rough ground: one strong, 63 a thousand times dimmer"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    rng = np.random.default_rng(64)
    spheres = np.zeros(65, SPHERE_DTYPE)
    spheres[0] = (0.0, -1000.0, 0.0, 1000.0)
    spheres["cx"][1:] = rng.uniform(-5.0, 5.0, 64)
    spheres["cy"][1:] = rng.uniform(1.0, 4.0, 64)
    spheres["cz"][1:] = rng.uniform(-3.0, 6.0, 64)
    spheres["r"][1:] = 0.2
    mats = default_material(65)
    mats["BaseColor"][:, :3] = 0.6
    mats["Roughness"] = 0.6
    mats["EmissiveColor"][1:] = (1.0, 0.9, 0.8)
    mats["EmissiveStrength"][1:] = 0.05
    mats["EmissiveStrength"][17] = 50.0
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.1, 0.1, 0.1, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    return spheres, mats, sd


def test_noise_below_uniform(dxrs, host, oracle, shims):
    """one strong emitter among 63 a thousand times dimmer, 8 candidates, no reuse: single-frame RMSE against the quadrature over a
    16 x 8 view and 24 frames.  Only the direction is asserted: each presampled mode is below Uniform."""
    w, h, frames = 16, 8, 24
    spheres, mats, sd = strong_and_dim_scene(dxrs)
    cam = host.camera_matrices(w, h, **CAM)
    gb, _ = cpu_gbuffer((shims[1], shims[2]), oracle, cam, w, h, spheres, mats, sd)
    quad = quadrature_image(ref.Scene(spheres, mats), gb, w * h, tuple(float(x) for x in cam.Position), 4)
    assert (quad > 0).sum() > w * h // 3
    rmse = {}
    for name, ls in (("uniform", sampling(UNIFORM)), ("power", CPU_POWER), ("regir", CPU_REGIR)):
        fr = di_frames(SampledHostPass(shims, spheres, mats), gb, w, h, cam, ls, frames)
        rmse[name] = math.sqrt(((fr - quad[None, :]) ** 2).mean())
    print(f"single-frame RMSE: {rmse}; power / uniform {rmse['power'] / rmse['uniform']:.3f}, regir / uniform {rmse['regir'] / rmse['uniform']:.3f}")
    assert rmse["power"] < rmse["uniform"] and rmse["regir"] < rmse["uniform"]


# ---------------------------------------------------------------------------------------------------- GPU
def emitter_scene(dxrs, n_lights, seed=0):
    """a rough ground under n_lights small emitters of unequal size, colour and strength (three decades)"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    rng = np.random.default_rng(seed + n_lights)
    n = n_lights + 2
    spheres = np.zeros(n, SPHERE_DTYPE)
    spheres[0] = (0.0, -1000.0, 0.0, 1000.0)
    spheres[1] = (0.0, 1.0, 0.0, 1.0)  # a rough blocker in the middle
    spheres["cx"][2:] = rng.uniform(-6.0, 6.0, n_lights)
    spheres["cy"][2:] = rng.uniform(0.5, 6.0, n_lights)
    spheres["cz"][2:] = rng.uniform(-4.0, 8.0, n_lights)
    spheres["r"][2:] = rng.uniform(0.05, 0.3, n_lights)
    mats = default_material(n)
    mats["BaseColor"][:, :3] = 0.6
    mats["Roughness"] = 0.6
    mats["EmissiveColor"][2:] = rng.uniform(0.1, 1.0, (n_lights, 3))
    mats["EmissiveStrength"][2:] = 10.0 ** rng.uniform(-1.0, 2.0, n_lights)
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.1, 0.1, 0.1, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    return spheres, mats, sd


def entries_equal(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} entries, expected {len(want)}"
    diff = (got["light"] != want["light"]) | (got["inv_pdf"].view(np.uint32) != want["inv_pdf"].view(np.uint32))
    assert not diff.any(), f"{what}: {int(diff.sum())} of {len(got)} entries differ, first {int(np.argmax(diff))}: {got[np.argmax(diff)]} != {want[np.argmax(diff)]}"


def structures_equal(r, lr, spheres, mats, cam, frame, ls, what):
    pyr, ris = r.light_ris_download()
    want_pyr, want_ris = host_structures(lr, spheres, mats, tuple(cam.Position), frame, ls)
    assert len(pyr) == len(want_pyr), f"{what}: pyramid of {len(pyr)} floats, expected {len(want_pyr)}"
    diff = pyr.view(np.uint32) != want_pyr.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {len(pyr)} pyramid floats differ, first {int(np.argmax(diff))}: {pyr[np.argmax(diff)]} != {want_pyr[np.argmax(diff)]}"
    entries_equal(ris, want_ris, what)
    return pyr, ris


STRUCTURE_CASES = [(1, sampling(POWER, tile_size=64, tile_count=4)), (5, sampling(POWER, tile_size=64, tile_count=4)),
                   (1024, sampling(POWER, tile_size=64, tile_count=4)), (1025, sampling(POWER, tile_size=64, tile_count=4)),
                   (4097, sampling(POWER, tile_size=64, tile_count=4)), (5, sampling(POWER, tile_size=100, tile_count=3)),
                   (5, sampling(REGIR, tile_size=100, tile_count=3, grid_size=2, lights_per_cell=70)),
                   (17, sampling(REGIR, tile_size=64, tile_count=4, grid_size=3, lights_per_cell=256, cell_size=2.5)), (5, sampling(REGIR))]


@pytest.mark.gpu
@pytest.mark.parametrize("n_lights,ls", STRUCTURE_CASES, ids=[f"{n}-{s['mode']}-{s['tile_size']}x{s['tile_count']}-{s['grid_size']}x{s['lights_per_cell']}" for n, s in STRUCTURE_CASES])
def test_gpu_structures_match_host(dxrs, host, renderer, shims, n_lights, ls):
    """what the three kernels built, bit for bit: one and two launches of the pyramid kernel (1024 | 1025) and a ragged second launch
    (4097), tiles that are no multiple of the wave (100), ReGIR cells that are no multiple of the workgroup (70), the defaults"""
    w, h = 16, 8
    spheres, mats, sd = emitter_scene(dxrs, n_lights)
    cam = host.camera_matrices(w, h, position=(0.3, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    renderer.restir_di(fill=SENTINEL, frame_index=3, light_sampling=ls)
    pyr, ris = structures_equal(renderer, shims[0], spheres, mats, cam, 3, ls, f"{n_lights} emitters")
    assert (ris["light"][:ls["tile_size"] * ls["tile_count"]] < n_lights).all()


def history_equal(r, hp, w, h, which, what):
    """a slot of the context's history (pt_restir_di_history) against the host model's, bit for bit: the plane that says whether a pixel
    has a surface everywhere, the rest of the record, the transmission and the reservoir wherever it has one (launch 1 writes nothing
    else for a pixel without a surface)"""
    planes, tr = r.restir_di_history(w, h, which)
    slot = hp.slot(hp.cur ^ which)  # [rec0, rec1, rec2, rec3, transmission, res0, res1]
    want = [slot[0], slot[1], slot[2], slot[3], slot[5], slot[6]]
    assert same_bits(planes[3], want[3]), f"{what}: history slot {which}: the depth plane"
    valid = np.isfinite(want[3][:, 2])
    assert valid.any()
    for k in range(6):
        diff = (planes[k][valid].view(np.uint32) != want[k][valid].view(np.uint32)).any(axis=1)
        assert not diff.any(), f"{what}: history slot {which}, plane {k}: {int(diff.sum())} of {int(valid.sum())} surfaces differ"
    assert same_bits(tr[valid], slot[4][valid]), f"{what}: history slot {which}: transmission"


def gpu_sampled_frame(r, hp, w, h, cam, what, ls, **kw):
    """one pt_restir_di_sampled call (sentinel-filled outputs) against the host-compiled headers fed the same G-buffer: every word of
    Diffuse and Specular, unwritten pixels included, both slots of the history, and the structures the call built"""
    had_history = hp.valid and hp.size == (w, h)  # (the other slot holds a call's results only from the second call on)
    dd, ds, gb = r.restir_di(fill=SENTINEL, light_sampling=ls, **kw)
    gbn = {name: gb[name].cpu().numpy().reshape(w * h, -1) for name in INPUTS}
    want_d, want_s = hp.frame(gbn, w, h, cam, light_sampling=ls, **kw)
    got_d, got_s = dd.cpu().numpy().reshape(-1, 4), ds.cpu().numpy().reshape(-1, 4)
    for got, want, name in ((got_d, want_d, "Diffuse"), (got_s, want_s, "Specular")):
        diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {w * h} pixels differ, first {int(np.argmax(diff))}: {got[np.argmax(diff)]} != {want[np.argmax(diff)]}"
    history_equal(r, hp, w, h, 0, what)
    if had_history:
        history_equal(r, hp, w, h, 1, what)
    if ls["mode"] != UNIFORM:
        pyr, ris = r.light_ris_download()
        assert same_bits(pyr, hp.built[0]), f"{what}: pyramid"
        entries_equal(ris, hp.built[1], what)
    return got_d[:, 0:1].view(np.uint32)[:, 0] != SENTINEL.view(np.uint32), gbn


def cells_of_frame(lr, gbn, cam, ls):
    """per surface pixel: inside the grid without jitter?"""
    P = gbn["Position"]
    ok = np.isfinite(gbn["LinearDepth"][:, 0]) & (gbn["NormalRoughness"][:, 3] >= 0.05)
    return np.array([cell_of(lr, P[i, :3], (0.5, 0.5, 0.5), tuple(cam.Position), ls["grid_size"], ls["cell_size"]) != INVALID for i in np.flatnonzero(ok)])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [POWER, REGIR])
def test_gpu_three_frames_travelling_camera(dxrs, host, renderer, shims, mode):
    """67 x 45: ragged for the 8 x 8 pixel blocks and for the 16 x 16 tile blocks; the history runs (temporal and spatial reuse on), so
    frame f's outputs cover the reservoirs of the frames before; the camera travels, so the grid's centre moves and some surfaces fall
    back to the Power_RIS tile"""
    w, h = 67, 45
    spheres, mats, sd = make_scene(dxrs)
    ls = sampling(mode, tile_size=128, tile_count=6, grid_size=4, lights_per_cell=96, cell_size=2.5)
    hp = SampledHostPass(shims, spheres, mats)
    renderer.set_scene(spheres, mats, sd)
    renderer.set_textures(None)
    prev, lit, inside, outside = None, 0, 0, 0
    for f in range(3):
        cam = host.camera_matrices(w, h, position=(0.4 * f, 2.5 + 0.1 * f, -9.0 + 0.5 * f), look_at=(0.2 * f, 1.0, 0.0), hfov=math.radians(70), jitter_index=f,
                                   previous=prev)
        renderer.set_camera(cam)
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=2, spp=1))
        written, gbn = gpu_sampled_frame(renderer, hp, w, h, cam, f"frame {f}", ls, frame_index=f, reset_history=f == 0, spatial_samples=3, spatial_radius=20.0)
        lit += int(written.sum())
        if mode == REGIR:
            cells = cells_of_frame(shims[0], gbn, cam, ls)
            inside, outside = inside + int(cells.sum()), outside + int((~cells).sum())
        prev = cam
    assert lit > 3 * w * h // 10
    if mode == REGIR:
        assert inside > 100 and outside > 100, (inside, outside)


@pytest.mark.gpu
def test_gpu_scene_in_global_memory_with_many_emitters(dxrs, host, shims):
    w, h = 64, 48
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=100000)
    mats = mats.copy()
    rng = np.random.default_rng(5)
    lit = np.sort(np.concatenate([np.argsort(spheres["r"])[-3:], rng.choice(len(spheres) - 3, 1500, replace=False)]))
    lit = np.unique(lit)
    mats["EmissiveColor"][lit] = (1.0, 0.8, 0.6)
    mats["EmissiveStrength"][lit] = 10.0 ** rng.uniform(-1.0, 1.5, len(lit))
    cam = host.camera_matrices(w, h, jitter=False)
    r = dxrs.Renderer(device=0)
    try:
        gpu_setup(r, dxrs, spheres, mats, sd, cam, w, h)
        assert not r.accel.lds_resident
        assert shims[0].lr_host_lights(mats.ctypes.data, len(mats), None) > 1024
        hp = SampledHostPass(shims, spheres, mats)
        ls = sampling(REGIR, tile_size=256, tile_count=8, grid_size=4, lights_per_cell=64, cell_size=10.0)
        for f in range(2):
            written, _ = gpu_sampled_frame(r, hp, w, h, cam, f"frame {f}", ls, frame_index=f, reset_history=f == 0)
            assert written.sum() > 16, f"frame {f}: the emitters light {int(written.sum())} pixels"
    finally:
        r.close()


def raw_call(r, w, h, buffers, ls, entry="pt_restir_di_sampled", **fields):
    """the entry points as C sees them: ls = a PtLightSamplingSettings, or None for a null pointer -> status"""
    from dxrs_amd.abi_types import PtRestirDiSettings, PtRestirDiTextures
    s = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h), EnableTemporal=1, EnableSpatial=1, TemporalBiasCorrection=BASIC, SpatialBiasCorrection=BASIC, **fields)
    t = PtRestirDiTextures(**{n: C.c_void_p(p) for n, p in buffers.items() if p})
    if entry == "pt_restir_di":
        return r._lib.pt_restir_di(r._ctx, C.byref(s), C.byref(t))
    return r._lib.pt_restir_di_sampled(r._ctx, C.byref(s), C.byref(ls) if ls is not None else None, C.byref(t))


@pytest.mark.gpu
def test_gpu_uniform_is_pt_restir_di(dxrs, host, renderer):
    """Mode 0 and the null pointer are pt_restir_di bit for bit -- outputs and the history slot each call wrote, so the same slots and
    restart rules -- and the two entry points may alternate on one context"""
    import torch
    from dxrs_amd.abi_types import GBUFFER_CHANNELS, PtLightSamplingSettings
    w, h, frames = 67, 45, 4
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    width = dict(GBUFFER_CHANNELS)
    gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS}
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({n: b.data_ptr() for n, b in gb.items()})
    renderer.synchronize()

    def run(pick):
        outs = []
        for f in range(frames):
            out = torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)).cuda()
            torch.cuda.synchronize()
            bufs = dict({n: b.data_ptr() for n, b in gb.items()}, Diffuse=out[0].data_ptr(), Specular=out[1].data_ptr())
            entry, ls = pick(f)
            assert raw_call(renderer, w, h, bufs, ls, entry, FrameIndex=f, ResetHistory=int(f == 0), SpatialSamples=2) == 0
            renderer.synchronize()
            planes, tr = renderer.restir_di_history(w, h, 0)
            valid = np.isfinite(planes[3][:, 2])
            outs.append(np.concatenate([out.cpu().numpy().ravel(), planes[3].ravel(), planes[:, valid].ravel(), tr[valid]]))
        return outs

    zero = PtLightSamplingSettings()  # Mode 0; the other fields are not looked at
    zero.TileSize = 99999
    want = run(lambda f: ("pt_restir_di", None))
    assert (want[-1][:2 * h * w * 4].view(np.uint32) != SENTINEL.view(np.uint32)).any()
    for name, pick in (("Mode 0", lambda f: ("pt_restir_di_sampled", zero)), ("null pointer", lambda f: ("pt_restir_di_sampled", None)),
                       ("alternating", lambda f: ("pt_restir_di", None) if f & 1 else ("pt_restir_di_sampled", zero))):
        got = run(pick)
        for f in range(frames):
            assert len(got[f]) == len(want[f]) and same_bits(got[f], want[f]), f"{name}: frame {f}"


@pytest.mark.gpu
def test_gpu_emitter_changes_are_followed(dxrs, host, renderer, shims):
    """an emitter resized and moved by pt_update_spheres is seen by the next call's pyramid and both segments (the kernels read the
    lane's own spheres); a pt_set_scene that takes the emitter count across 1024 and back reallocates and the counts follow"""
    w, h = 16, 8
    ls = sampling(REGIR, tile_size=64, tile_count=4, grid_size=2, lights_per_cell=70, cell_size=5.0)
    spheres, mats, sd = emitter_scene(dxrs, 5)
    cam = host.camera_matrices(w, h, position=(0.3, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    renderer.restir_di(fill=SENTINEL, frame_index=0, light_sampling=ls)
    pyr0, ris0 = structures_equal(renderer, shims[0], spheres, mats, cam, 0, ls, "before")
    moved = spheres.copy()
    moved["r"][3] *= 3.0
    moved["cx"][3] += 2.0
    moved["cz"][3] -= 1.5
    renderer.update_spheres(moved)
    renderer.restir_di(fill=SENTINEL, frame_index=0, light_sampling=ls)
    pyr1, ris1 = structures_equal(renderer, shims[0], moved, mats, cam, 0, ls, "moved")
    assert pyr1[1] != pyr0[1] and not same_bits(ris1["inv_pdf"], ris0["inv_pdf"]), "the same FrameIndex: only the emitter changed"
    for n_lights in (1030, 5):
        spheres, mats, sd = emitter_scene(dxrs, n_lights, seed=1)
        gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
        renderer.restir_di(fill=SENTINEL, frame_index=1, light_sampling=ls)
        pyr, _ = structures_equal(renderer, shims[0], spheres, mats, cam, 1, ls, f"{n_lights} emitters")
        assert len(pyr) == shims[0].lr_host_pyramid_floats(n_lights)


@pytest.mark.gpu
def test_gpu_three_lanes_equal_one_lane(dxrs, host):
    """pt_render_gbuffer -> pt_restir_di_sampled -> pt_render_with_di with three frames in flight, one buffer set per lane, no host
    wait in between: the frames equal, bit for bit, those of a one-lane context (consecutive calls hand the history, the pyramid and
    the RIS buffer from lane to lane)"""
    import torch
    from dxrs_amd.abi_types import GBUFFER_CHANNELS
    w, h, frames, mode = 64, 48, 5, 3
    spheres, mats, sd = make_scene(dxrs)
    width = dict(GBUFFER_CHANNELS)
    ls = sampling(REGIR, tile_size=128, tile_count=6, grid_size=4, lights_per_cell=96, cell_size=2.5)

    def run(lanes):
        r = dxrs.Renderer(device=0, frames_in_flight=lanes)
        try:
            r.set_scene(spheres, mats, sd)
            sets = [dict(gb={n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS},
                         dd=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), ds=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                         out=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), nd=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"),
                         ns=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")) for _ in range(3)]
            torch.cuda.synchronize()
            outs = []
            for f in range(frames):
                s = sets[f % 3]
                r.set_camera(host.camera_matrices(w, h, position=(0.2 * f, 2.5, -9.0 + 0.3 * f), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter_index=f))
                r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=4, spp=1))
                if f >= 3:
                    r.synchronize()      # (the buffers are read back and cleared from the host side)
                    outs.append([s[k].cpu().numpy().copy() for k in ("out", "dd", "ds")])
                    for t in (s["dd"], s["ds"], s["nd"], s["ns"]):
                        t.zero_()
                    torch.cuda.synchronize()
                ptrs = {n: b.data_ptr() for n, b in s["gb"].items()}
                r.render_gbuffer_device(ptrs)
                r.restir_di_device(w, h, dict(ptrs, Diffuse=s["dd"].data_ptr(), Specular=s["ds"].data_ptr()), frame_index=f, spatial_samples=2, light_sampling=ls)
                r.render_with_di_device(s["out"].data_ptr(), s["dd"].data_ptr(), s["ds"].data_ptr(), None, mode, {"Diffuse": s["nd"].data_ptr(), "Specular": s["ns"].data_ptr()})
            r.synchronize()
            for k in range(frames - 3, frames):  # the last three frames still sit in their buffer sets
                outs.append([sets[k % 3][name].cpu().numpy().copy() for name in ("out", "dd", "ds")])
            return outs
        finally:
            r.close()

    one, three = run(1), run(3)
    assert len(one) == len(three) == frames
    for k, (a, b) in enumerate(zip(one, three)):
        for x, y, name in zip(a, b, ("out", "Diffuse", "Specular")):
            assert same_bits(x, y), f"frame {k} {name}"
    assert any((g[1][..., :3] > 0).any() for g in three)


@pytest.mark.gpu
def test_gpu_misuse(dxrs, host, renderer):
    import torch
    from dxrs_amd.abi_types import GBUFFER_CHANNELS, PtLightSamplingSettings
    w, h = 32, 16
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    width = dict(GBUFFER_CHANNELS)
    gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS}
    out = torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({n: b.data_ptr() for n, b in gb.items()})
    renderer.synchronize()
    good = dict({n: b.data_ptr() for n, b in gb.items()}, Diffuse=out[0].data_ptr(), Specular=out[1].data_ptr())
    INVALID_ARG, STATE = 1, 4

    def message(**fields):
        status = raw_call(renderer, w, h, good, PtLightSamplingSettings(**fields))
        return status, renderer._lib.pt_last_error(renderer._ctx).decode()

    for fields, text in ((dict(Mode=3), "Mode must be"), (dict(Mode=1, TileSize=8193), "TileSize"), (dict(Mode=1, TileCount=1025), "TileCount"),
                         (dict(Mode=2, ReGIRGridSize=33), "ReGIRGridSize"), (dict(Mode=2, ReGIRLightsPerCell=1025), "ReGIRLightsPerCell"),
                         (dict(Mode=2, ReGIRBuildSamples=33), "ReGIRBuildSamples"), (dict(Mode=2, ReGIRCellSize=0.05), "ReGIRCellSize"),
                         (dict(Mode=2, ReGIRCellSize=10.5), "ReGIRCellSize"), (dict(Mode=2, ReGIRCellSize=float("nan")), "ReGIRCellSize"),
                         (dict(Mode=2, ReGIRCellSize=float("inf")), "ReGIRCellSize"), (dict(Mode=1, _pad=1), "_pad"),
                         (dict(Mode=2, ReGIRGridSize=32, ReGIRLightsPerCell=512), "2^24"), (dict(Mode=2, TileSize=8192, TileCount=1024, ReGIRGridSize=26, ReGIRLightsPerCell=512), "2^24")):
        status, msg = message(**fields)
        assert status == INVALID_ARG and text in msg and msg.startswith("pt_restir_di_sampled: "), (fields, status, msg)
    assert raw_call(renderer, w, h, dict(good, Diffuse=0), PtLightSamplingSettings(Mode=1)) == INVALID_ARG
    assert raw_call(renderer, w, h, good, PtLightSamplingSettings(Mode=1), InitialSamples=33) == INVALID_ARG
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all(), "a rejected call writes nothing"
    assert raw_call(renderer, w, h, good, PtLightSamplingSettings(Mode=2, ReGIRGridSize=2, ReGIRCellSize=10.0)) == 0
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) != SENTINEL.view(np.uint32)).any()
    # the download hook's own errors
    n_pyr, n_ris = C.c_uint32(0), C.c_uint32(0)
    lib, ctx = renderer._lib, renderer._ctx
    assert lib.pt_light_ris_download(ctx, None, None, None, C.byref(n_ris)) == INVALID_ARG
    assert lib.pt_light_ris_download(ctx, None, C.byref(n_pyr), None, C.byref(n_ris)) == 0 and n_pyr.value == 5 and n_ris.value == 1024 * 128 + 8 * 512
    small = np.zeros(4, np.float32)
    n_pyr.value = 4
    assert lib.pt_light_ris_download(ctx, small.ctypes.data, C.byref(n_pyr), None, C.byref(n_ris)) == INVALID_ARG and n_pyr.value == 5
    assert lib.pt_restir_di_history(ctx, 2, small.ctypes.data, small.ctypes.data) == INVALID_ARG
    assert lib.pt_restir_di_history(ctx, 0, None, small.ctypes.data) == INVALID_ARG
    # zero emitters: success, nothing written
    dark = mats.copy()
    dark["EmissiveStrength"] = 0.0
    gpu_setup(renderer, dxrs, spheres, dark, sd, cam, w, h)
    out.copy_(torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)))
    torch.cuda.synchronize()
    assert raw_call(renderer, w, h, good, PtLightSamplingSettings(Mode=2)) == 0
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    # before a scene is set: PT_ERR_STATE, and the hook has nothing to return
    r2 = dxrs.Renderer(device=0)
    try:
        assert raw_call(r2, w, h, good, PtLightSamplingSettings(Mode=1)) == STATE
        assert r2._lib.pt_light_ris_download(r2._ctx, None, C.byref(n_pyr), None, C.byref(n_ris)) == STATE
        assert r2._lib.pt_restir_di_history(r2._ctx, 0, small.ctypes.data, small.ctypes.data) == STATE
    finally:
        r2.close()
