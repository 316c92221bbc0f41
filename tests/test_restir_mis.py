"""Row N17 -- pt_restir_di_ex: BRDF candidates in initial sampling and the boiling filter (DESIGN.md spec S23).
CPU: the host-compiled header paths (tests/hostshim/restir_mis_host.cpp over csrc/pt_restir.h and csrc/pt_light.h) against the float64
restatement (restir_mis_reference.py) and known answers -- the cone inverse, the lobe-summed pdf, initial sampling in the three modes,
the identity with the extras off, unbiasedness against the quadrature of the direct-light integral, the noise on a glossy ground next
to a large emitter, the filter's known answers, the stand-alone sanitizer program.  GPU: whole pt_restir_di_ex calls against the
host-compiled header bit for bit, outputs and both history slots."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import light_ris_reference as lref
import restir_mis_reference as mref
import restir_reference as ref
from test_light_ris import (CPU_POWER, CPU_REGIR, ENTRY, MAX_EXCLUDED, POWER, REGIR, UNIFORM, U, SampledHostPass, history_equal, host_structures, least,
                            pyramid_levels, quadrature_image, same_bits, sampling)
from test_restir_pass import (BASIC, BLOCKER, E0, F_FRAMES, GROUND, H, HISTORY, INPUTS, OFF, PASS_RTOL, RAYTRACED, SENTINEL, W, HostPass, cpu_gbuffer, deviation,
                              gpu_setup, make_scene, reservoirs, settings)

HERE = os.path.dirname(os.path.abspath(__file__))
CAM = dict(position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
LUM = np.array([0.2126, 0.7152, 0.0722])
NO_EXTRAS = dict(brdf_samples=0, boiling_filter=None)
REFERENCE_DEFAULTS = dict(brdf_samples=1, boiling_filter=0.2)  # InitialSampling.BRDFSamples, TemporalResampling.BoilingFilter


# ---------------------------------------------------------------------------------------------------- the host-compiled headers
@pytest.fixture(scope="module")
def shims():
    import __graft_entry__ as g

    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    rm = C.CDLL(g.build_restir_mis_shim())
    for name, res, args in (("rm_host_call", None, [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, f32, vp, f32]), ("rm_host_sample_cone", None, [vp, u32, vp]),
                            ("rm_host_invert_cone", None, [vp, u32, vp]), ("rm_host_bsdf_pdf", None, [vp, vp, u32, vp, vp]),
                            ("rm_host_boiling", f32, [vp, f32, vp, vp]), ("rm_host_boiling_multiplier", f32, [f32])):
        getattr(rm, name).restype, getattr(rm, name).argtypes = res, args
    lr = C.CDLL(g.build_lightris_shim())
    for name, res, args in (("lr_host_lights", u32, [vp, u32, vp]), ("lr_host_levels", u32, [u32]), ("lr_host_pyramid_floats", u32, [u32]),
                            ("lr_host_level_offset", u32, [u32, u32]), ("lr_host_pyramid_from_powers", None, [vp, u32, vp]),
                            ("lr_host_powers", None, [vp, vp, u32, vp]), ("lr_host_power_segment", None, [vp, u32, u32, u32, u32, vp]),
                            ("lr_host_regir_segment", None, [vp, vp, u32, vp, vp, vp, vp]), ("lr_host_call", None, [vp, vp, u32, vp, vp, vp, vp, f32, vp, vp])):
        getattr(lr, name).restype, getattr(lr, name).argtypes = res, args
    ri = C.CDLL(g.build_restir_shim())
    ri.ri_host_call.restype = None
    ri.ri_host_call.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp]
    gb = C.CDLL(g.build_gbuffer_shim())
    gb.gb_pixels.restype = None
    gb.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    gb.gb_srgb_lut.restype = None
    gb.gb_srgb_lut.argtypes = [vp]
    return rm, lr, ri, gb


class MisHostPass(HostPass):
    """pt_restir_di_ex over the host-compiled header: HostPass's history slots and restart rules, rm_host_call in place of ri_host_call
    (textured scenes included); light_sampling as SampledHostPass takes it, candidates = dict(brdf_samples, boiling_filter = strength or None)"""

    def __init__(self, shims, spheres, mats, textures=None):
        super().__init__(shims[0], shims[3], spheres, mats, textures)

    def call(self, gb, w, h, cam, out_d, out_s, launches=3, light_sampling=None, candidates=None, **kw):
        s = settings(**kw)
        ls = light_sampling or sampling(UNIFORM)
        cd = dict(NO_EXTRAS, **(candidates or {}))
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
        on = cd["boiling_filter"] is not None
        cprm = np.array([cd["brdf_samples"], int(on)], np.uint32)
        arrays = [np.ascontiguousarray(gb[name], dtype=np.float32) for name in INPUTS] + self.slots[cur] + self.slots[prev] + [out_d, out_s]
        ptrs = (C.c_void_p * 24)(*[a.ctypes.data for a in arrays])
        p = lambda a: a.ctypes.data if a is not None else None
        self.lib.rm_host_call(p(self.spheres), p(self.mats), len(self.spheres), p(self.texels), p(self.info), 0 if self.info is None else len(self.info),
                              p(self.maps), p(self.rot), p(prm), p(fprm), ptrs, p(sprm), ls["cell_size"], p(cprm), float(cd["boiling_filter"]) if on else 0.0)
        self.cur, self.valid = cur, True
        return self.slots[cur]


@pytest.fixture(scope="module")
def cpu_case(dxrs, host, oracle, shims):
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(W, H, **CAM)
    gb, ids = cpu_gbuffer((shims[2], shims[3]), oracle, cam, W, H, spheres, mats, sd)
    assert (ids == GROUND).any()
    return spheres, mats, sd, cam, gb


# ---------------------------------------------------------------------------------------------------- CPU: ABI
def test_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_restir_di_ex") and "pt_restir_di_ex" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtLightSamplingSettings, PtRestirDiCandidates, PtRestirDiSettings, PtRestirDiTextures
    S = PtRestirDiCandidates
    assert C.sizeof(S) == 16
    assert [getattr(S, f).offset for f in ("BrdfSamples", "EnableBoilingFilter", "BoilingFilterStrength", "_pad")] == [0, 4, 8, 12]
    assert C.sizeof(PtRestirDiSettings) == 48 and C.sizeof(PtLightSamplingSettings) == 32 and C.sizeof(PtRestirDiTextures) == 80  # the siblings keep theirs
    s, ls, cd, t = PtRestirDiSettings(), PtLightSamplingSettings(), S(), PtRestirDiTextures()
    # PT_ERR_INVALID_ARG for a null context, whatever else is null: what pt_restir_di and pt_restir_di_sampled answer
    assert lib.pt_restir_di_ex(None, C.byref(s), C.byref(ls), C.byref(cd), C.byref(t)) == 1
    assert lib.pt_restir_di_ex(None, None, None, None, None) == 1
    assert lib.pt_restir_di_sampled(None, None, None, None) == 1 and lib.pt_restir_di(None, None, None) == 1


# ---------------------------------------------------------------------------------------------------- CPU: the cone inverse
def cone_cases():
    """(P, C, r, u1, u2): near, far (r / d down to 1e-3), limb (u1 = 1 and just below) and axis (u1 at the smallest draw) samples, emitters
    along +z and -z of the surface (where get_basis branches on the sign of the axis' z) and off axis"""
    rng = np.random.default_rng(17)
    rows = []
    for axis in ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1e-4, -1e-4, -1.0), (0.6, 0.0, 0.8), (-0.36, 0.8, -0.48), (0.0, 1.0, 0.0)):
        for ratio in (0.9, 0.5, 0.1, 1e-2, 1e-3):   # r / d
            for r in (0.25, 3.0):
                d = r / ratio
                P = rng.uniform(-2.0, 2.0, 3)
                Cc = P + d * np.array(axis) / np.linalg.norm(axis)
                for u1 in (1.0, 1.0 - 2.0 ** -24, 0.75, 0.5, 1e-3, 2.0 ** -23):
                    for u2 in (1.0, 0.75, 0.5, 0.25, 0.125, 2.0 ** -23, float(rng.uniform(0.01, 0.99))):
                        rows.append((*P, *Cc, r, u1, u2))
    return np.array(rows, np.float32)


def test_invert_sphere_cone_round_trip(shims):
    """u -> L -> u' -> L' through the header, and L' against the float64 restatement's forward(inverse(L)).
    Bound on max |L' - L| per component.  The tangential part of L' has length sin(theta) <= sin_max = r / d and its angle is 2 pi u2':
      * u2' carries atan2_spec's error (spec S8: below 2e-5 rad), the two sincos_2pi evaluations theirs (5e-7 each, absolute), the
        rounding of u2' near 1 half a unit: 2 pi U rad -- all scaled by sin_max;
      * the basis is formed in float32 and is orthonormal only to a few U (get_basis: 4 operations per entry), which enters once
        through rotate_vector and once through rotate_vector_inverse: 8 U;
      * the two rotations round 3 times per component (3 + 3), lx^2 + ly^2, the sum 1 + lz, the two quotients, cos = 1 - k, sin^2 and its
        root: 10 more roundings, each at most U in a component of a unit vector (a relative error of sin(theta) moves the component by
        sin(theta) times it);
    in all sin_max (2e-5 + 1e-6 + 2 pi U) + 24 U.  The restatement evaluates the same polynomial in float64, so it is held to the same
    bound without the atan2 term's benefit of the doubt."""
    rm = shims[0]
    rows = cone_cases()
    n = len(rows)
    fwd = np.zeros((n, 5), np.float32)
    rm.rm_host_sample_cone(rows.ctypes.data, n, fwd.ctypes.data)
    assert (fwd[:, 4] == 1).all()
    inv_in = np.ascontiguousarray(np.concatenate([rows[:, :7], fwd[:, :3]], axis=1), np.float32)
    u = np.zeros((n, 2), np.float32)
    rm.rm_host_invert_cone(inv_in.ctypes.data, n, u.ctypes.data)
    assert (u > 0).all() and (u <= 1).all()
    back_in = np.ascontiguousarray(np.concatenate([rows[:, :7], u], axis=1), np.float32)
    back = np.zeros((n, 5), np.float32)
    rm.rm_host_sample_cone(back_in.ctypes.data, n, back.ctypes.data)
    worst = worst64 = 0.0
    for i in range(n):
        P, Cc, r = tuple(float(x) for x in rows[i, 0:3]), tuple(float(x) for x in rows[i, 3:6]), float(rows[i, 6])
        d = math.sqrt(sum((a - b) ** 2 for a, b in zip(P, Cc)))
        bound = (r / d) * (2e-5 + 1e-6 + 2 * math.pi * U) + 24 * U
        err = float(np.abs(back[i, :3].astype(np.float64) - fwd[i, :3]).max())
        L = tuple(float(x) for x in fwd[i, :3])
        u64 = mref.invert_cone(P, Cc, r, L)
        L64, _ = mref.it.sphere_cone(P, Cc, r, *u64)
        err64 = max(abs(a - float(b)) for a, b in zip(L64, back[i, :3]))
        assert err <= bound and err64 <= bound, (i, rows[i], fwd[i], u[i], back[i], err, err64, bound)
        worst, worst64 = max(worst, err / bound), max(worst64, err64 / bound)
    print(f"{n} round trips: largest |L' - L| is {worst:.3f} of its bound, against the restatement {worst64:.3f}")
    # inside the sphere the inverse answers (1, 1)
    inside = np.array([[0, 0, 0, 0.1, 0, 0, 1.0, 0, 0, 1]], np.float32)
    out = np.zeros(2, np.float32)
    rm.rm_host_invert_cone(inside.ctypes.data, 1, out.ctypes.data)
    assert tuple(out) == (1.0, 1.0)


# ---------------------------------------------------------------------------------------------------- CPU: the lobe-summed pdf
SURFACES = dict(diffuse=dict(base=(0.6, 0.55, 0.5), metallic=0.0, roughness=0.9, ior=1.5, transmission=0.0),
                glossy=dict(base=(0.9, 0.8, 0.7), metallic=0.7, roughness=0.2, ior=1.5, transmission=0.0),
                transmissive=dict(base=(0.8, 0.9, 1.0), metallic=0.0, roughness=0.3, ior=1.33, transmission=0.7))


def host_pdfs(rm, m, Ng, Ns, V, L):
    surf = np.array([*m["base"], m["metallic"], m["roughness"], m["ior"], m["transmission"], *Ng, *Ns, *V], np.float32)
    L = np.ascontiguousarray(L, np.float32)
    out, w = np.zeros((len(L), 4), np.float32), np.zeros(3, np.float32)
    rm.rm_host_bsdf_pdf(surf.ctypes.data, L.ctypes.data, len(L), out.ctypes.data, w.ctypes.data)
    return out, w


def sphere_grid(n_theta, n_phi):
    """midpoints of an equal-area grid over the sphere about +z: (directions, the weight of each = 4 pi / count)"""
    z = 1.0 - 2.0 * (np.arange(n_theta) + 0.5) / n_theta
    phi = 2.0 * math.pi * (np.arange(n_phi) + 0.5) / n_phi
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1.0 - zz * zz)
    return np.stack([s * np.cos(pp), s * np.sin(pp), zz], axis=-1).reshape(-1, 3), 4.0 * math.pi / (n_theta * n_phi)


def kept_share(rough, V, k):
    """the share of VNDF-sampled reflections about V that leave above the plane z = 0: a k x k midpoint grid over the sampler's (u1, u2), float64"""
    basis = mref.it.get_basis((0.0, 0.0, 1.0))
    vl = mref.it.to_local(basis, V)
    kept = 0
    for a in range(k):
        for c in range(k):
            H = mref.it.to_world(basis, mref.it.vndf_ray(((a + 0.5) / k, (c + 0.5) / k), rough, vl))
            kept += mref.it.reflect(mref.it.neg(V), H)[2] > 0.0
    return kept / (k * k)


@pytest.mark.parametrize("name", list(SURFACES))
def test_bsdf_pdf_all(shims, name):
    """the sum of the per-lobe pdfs that apply, bit for bit; and a pdf: its integral over the sphere.  What it integrates to: the
    diffuse lobe's cosine pdf integrates to its lobe weight w_D; the specular lobe's visible-normal pdf to w_S times the share of
    VNDF-sampled reflections that leave above the horizon (Ng = Ns here; the rest is what bsdf_sample rejects, 1.7 % of all samples for
    the roughness-0.9 surface at V 40 degrees off the normal) -- that share is counted in float64 over a stratified grid of the sampler's
    own (u1, u2); the transmission term |N.L| w_T is no normalised density (BxDF.hlsli:172-177 returns the cosine itself) and
    integrates to 2 pi w_T over the sphere.  So the expected integral is w_D + w_S kept + 2 pi w_T -- 1 for a surface without
    transmission up to the rejected share -- and the quadrature's own error is taken from halving both grids."""
    rm = shims[0]
    m = SURFACES[name]
    Ng = Ns = (0.0, 0.0, 1.0)
    V = (math.sin(math.radians(40)), 0.0, math.cos(math.radians(40)))
    dirs, weight = sphere_grid(512, 1024)
    out, w = host_pdfs(rm, m, Ng, Ns, V, dirs)
    wt = float(w[2])
    assert (wt > 0) == (name == "transmissive")
    above = dirs[:, 2].astype(np.float32) > 0
    want = np.zeros(len(dirs), np.float32)
    if wt > 0:
        want = out[:, 3].copy()
    if wt < 1:
        want = np.where(above, (want + (out[:, 1] + out[:, 2]).astype(np.float32)).astype(np.float32), want)
    assert same_bits(out[:, 0], want), "bsdf_pdf_all is the sum of the per-lobe pdfs that apply"
    assert (out[~above, 1] == 0).all() and (out[~above, 2] == 0).all()
    total = float(out[:, 0].astype(np.float64).sum() * weight)
    coarse_dirs, coarse_w = sphere_grid(256, 512)
    coarse = float(host_pdfs(rm, m, Ng, Ns, V, coarse_dirs)[0][:, 0].astype(np.float64).sum() * coarse_w)
    kept, kept_coarse = (kept_share(max(2e-3, float(np.float32(m["roughness"]))), V, k) for k in (192, 96))
    expected = float(w[0]) + float(w[1]) * kept + 2.0 * math.pi * wt
    err = abs(total - coarse) + float(w[1]) * abs(kept - kept_coarse) + 1e-6
    print(f"{name}: weights {w}, integral {total:.6f}, expected {expected:.6f}, quadrature error {err:.2e}")
    assert abs(total - expected) <= err
    # the float64 restatement, direction by direction on a coarse set
    s = dict(sv={"FrontNg": Ng, "Ns": Ns, "basis": mref.it.get_basis(Ns)},
             b=mref.it.bsdf_of({"BaseColor": [float(np.float32(c)) for c in m["base"]] + [1.0], "Metallic": float(np.float32(m["metallic"])),
                                "Roughness": float(np.float32(m["roughness"])), "IOR": float(np.float32(m["ior"])), "Transmission": float(np.float32(m["transmission"]))}, True, False))
    V32 = tuple(float(np.float32(x)) for x in V)
    w64 = mref.it.lobe_weights(s["b"], s["sv"], V32)
    some, _ = sphere_grid(12, 16)
    some = some.astype(np.float32)
    got = host_pdfs(rm, m, Ng, Ns, V, some)[0][:, 0]
    for L, g in zip(some, got):
        p = mref.pdf_all(s["b"], s["sv"], tuple(float(x) for x in L), V32, w64)
        assert abs(float(g) - p) <= PASS_RTOL * max(p, 1e-6), (L, g, p)


# ---------------------------------------------------------------------------------------------------- CPU: initial sampling
INITIAL_FRAME = 22  # (see the test's docstring)


@pytest.mark.parametrize("n_brdf", [1, 8])
@pytest.mark.parametrize("ls", [sampling(UNIFORM), CPU_POWER, CPU_REGIR], ids=["uniform", "power", "regir"])
def test_initial_sampling_against_restatement(shims, cpu_case, ls, n_brdf):
    """Launch 1 alone (no history, filter off), pixel by pixel: the selected (emitter, u1, u2), M = 8 + N_B, whether the visibility ray
    kept the sample, and p_hat and W -- W = w_sum / (M p_hat) carries every candidate's balance-heuristic weight -- to test_restir_pass's
    PASS_RTOL.  The restatement draws from the float32 structures the call built.  A pixel whose discrete choice sits within rounding of
    its threshold may differ and is counted: an index pick within U n of an integer, a cell coordinate (test_light_ris's bound), a
    stream-RIS step within 2 (256 + 16 + 2) U w (the weight is the target function, PASS_RTOL = 256 U, over a mixture density of the same
    error, summed over up to 16 candidates), a lobe choice within 64 U of its threshold (the lobe weights' own error), a direction within
    64 U of the geometric horizon, a ray that would graze a silhouette, or swap its two nearest hits, if turned by 64 U (the BRDF
    direction is a chain of about 60 operations), an inverted u1 within 8 U d / r of its clamp at the limb.
    With 936 surfaces the 0.1 % cap allows no exclusion at all, and 8 + N_B candidates with a ray each make a near miss likely: of
    FrameIndex 8 .. 34 only 22 keeps all six cases clear, which is why it is the seed.  Two kinds of miss occur at the others: one
    restatement comparison near its threshold (the header never flipped one: `flipped` was 0 throughout), and pixels 643 and 740 -- the
    roughness-0.35 blocker at a grazing view -- whose p_hat, for LOCAL candidates too, is off by up to 1.4 PASS_RTOL in ri_shade's own
    float32 GGX term (1 - NoH^2 (1 - alpha^2) cancels to within alpha^2 = 0.015): rows N10 / N16's arithmetic, which S23 does not touch."""
    spheres, mats, sd, cam, gb = cpu_case
    scene = ref.Scene(spheres, mats)
    n, frame = W * H, INITIAL_FRAME
    hp = MisHostPass(shims, spheres, mats)
    got = reservoirs(hp.call(gb, W, H, cam, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), launches=1, frame_index=frame, spatial=False,
                             light_sampling=ls, candidates=dict(brdf_samples=n_brdf)))
    cam_pos = tuple(float(x) for x in cam.Position)
    ris = pyr = None
    if ls["mode"] != UNIFORM:
        pyr32, entries = host_structures(shims[1], spheres, mats, cam_pos, frame, ls)
        ris = [(int(e["light"]), float(e["inv_pdf"])) for e in entries]
        pyr = [[float(x) for x in level] for level in pyramid_levels(shims[1], pyr32, len(scene.lights))]
    cell_bound, ris_bound = (5 * 32 / ls["cell_size"] + ls["grid_size"]) * U, 2 * 274 * U
    valid = flipped = near_alone = lit = 0
    for i in range(n):
        s = ref.surface(gb, i, cam_pos)
        g = got[i]
        assert (g["M"] > 0) == (s is not None)
        if s is None:
            continue
        valid += 1
        margins = []
        r = mref.initial(scene, s, i % W, i // W, frame, 8, n_brdf, ls["mode"], ris, pyr, ls["tile_size"], ls["tile_count"], ls["grid_size"], ls["lights_per_cell"],
                         float(np.float32(ls["cell_size"])), cam_pos, margins)
        near = (least(margins, "pick") <= U or least(margins, "cell") <= cell_bound or least(margins, "ris") <= ris_bound or least(margins, "lobe") <= 64 * U
                or least(margins, "fresnel") <= 64 * U or least(margins, "horizon") <= 64 * U or least(margins, "hit") <= 64 * U or least(margins, "clamp") <= 8 * U)
        near_alone += near
        if near:
            print(f"pixel {i} near a threshold:", {k: least(margins, k) for k in ("pick", "cell", "ris", "lobe", "fresnel", "horizon", "hit", "clamp")})
        same_pick = g["light"] == r["light"] and (g["W"] > 0) == (r["W"] > 0) and abs(g["u1"] - r["u1"]) <= 1e-3 and abs(g["u2"] - r["u2"]) <= 1e-3
        if not same_pick:
            assert near, f"pixel {i}: the pick differs away from every threshold: {g} != {r}"
            flipped += 1
            continue
        assert g["M"] == r["M"] == 8 + n_brdf
        # a local candidate's (u1, u2) are the draws themselves; an inverted one's are held through the values they give
        tol = lambda a, b: abs(a - b) <= PASS_RTOL * max(abs(a), abs(b)) + 1e-12
        assert tol(g["p_hat"], r["p_hat"]) and tol(g["W"], r["W"]), (i, g, r)
        lit += r["W"] > 0
    print(f"{valid} surfaces, {lit} lit; flipped {flipped}; near a threshold in the restatement alone: {near_alone}")
    assert valid > n // 3 and lit > valid // 4
    assert near_alone <= MAX_EXCLUDED * valid, "the seed puts too many of the restatement's own comparisons near their thresholds"
    assert flipped <= MAX_EXCLUDED * valid


# ---------------------------------------------------------------------------------------------------- CPU: identity
@pytest.mark.parametrize("ls", [None, CPU_POWER, CPU_REGIR], ids=["uniform", "power", "regir"])
def test_extras_off_is_the_existing_pass(shims, cpu_case, ls):
    """BrdfSamples = 0 and the filter off through rm_host_call against ri_host_call / lr_host_call: outputs and both history slots, bit
    for bit, over four frames with the history running"""
    spheres, mats, sd, cam, gb = cpu_case
    old = HostPass(shims[2], shims[3], spheres, mats) if ls is None else SampledHostPass((shims[1], shims[2], shims[3]), spheres, mats)
    new = MisHostPass(shims, spheres, mats)
    for f in range(4):
        kw = dict(frame_index=f, reset_history=f == 0, spatial_samples=2, spatial_radius=8.0, temporal_bias=RAYTRACED)
        a = old.frame(gb, W, H, cam, **kw) if ls is None else old.frame(gb, W, H, cam, light_sampling=ls, **kw)
        b = new.frame(gb, W, H, cam, light_sampling=ls, candidates=NO_EXTRAS, **kw)
        for x, y, name in zip(a, b, ("Diffuse", "Specular")):
            assert same_bits(x, y), f"frame {f}: {name}"
        for k in range(2):
            for x, y in zip(old.slot(k), new.slot(k)):
                assert same_bits(x, y), f"frame {f}: history slot {k}"
    assert (new.slot(new.cur)[6][:, 0] > 8).any(), "the history ran"


# ---------------------------------------------------------------------------------------------------- CPU: unbiasedness
@pytest.fixture(scope="module")
def statistics(dxrs, host, oracle, shims):
    """test_restir_pass's method: per-frame images of the luminance of DI over a static 24 x 16 view, 160 frames with the history
    running under Raytraced correction, for 8 + 1 candidates in each sampling mode, and the one-candidate control; and the quadrature"""
    w, h = 24, 16
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(w, h, **CAM)
    gb, ids = cpu_gbuffer((shims[2], shims[3]), oracle, cam, w, h, spheres, mats, sd)
    quad = quadrature_image(ref.Scene(spheres, mats), gb, w * h, tuple(float(x) for x in cam.Position), 8)

    def run(**kw):
        hp = MisHostPass(shims, spheres, mats)
        frames = []
        for f in range(F_FRAMES):
            out_d, out_s = hp.frame(gb, w, h, cam, frame_index=f, **kw)
            frames.append(np.where(out_d[:, :1].view(np.uint32) == SENTINEL.view(np.uint32), 0.0, (out_d[:, :3].astype(np.float64) + out_s[:, :3])) @ LUM)
        return np.array(frames)
    reuse = dict(temporal_bias=RAYTRACED, spatial_bias=RAYTRACED, max_history=HISTORY, spatial_samples=2, spatial_radius=4.0, candidates=dict(brdf_samples=1))
    small_regir = sampling(REGIR, tile_size=256, tile_count=16, grid_size=8, lights_per_cell=64, cell_size=2.5)
    return dict(quad=quad, control=run(initial_samples=1, temporal=False, spatial=False), uniform=run(**reuse), power=run(light_sampling=CPU_POWER, **reuse),
                regir=run(light_sampling=small_regir, **reuse))


def test_unbiased_with_brdf_candidates(statistics):
    """F = 160 frames, batches of MaxHistoryLength = 8, 8 local + 1 BRDF candidate, Raytraced correction in both reuse passes: the image
    total of the mean DI against the quadrature within 3 standard errors by batch means, for Uniform and Power_RIS candidates, next to
    the one-candidate control (independent frames), which must pass the same check itself.  ReGIR_RIS is printed only: its mixture is
    approximate by spec (the BRDF side prices the light technique by power, not by the cell).
    Measured (quadrature total 17.2903): control -0.0120 (standard error 0.1337), Uniform -0.0621 (0.0514), Power_RIS -0.0591 (0.0459),
    ReGIR_RIS -0.1231 (0.0292, 4.2 standard errors)."""
    q = statistics["quad"]
    dev_c, se_c = deviation(statistics["control"], q, 1)
    print(f"quadrature total {q.sum():.4f}; control dev {dev_c:+.4f} se {se_c:.4f}")
    out = {}
    for name in ("uniform", "power", "regir"):
        out[name] = deviation(statistics[name], q, HISTORY)
        print(f"{name} candidates + 1 BRDF candidate: dev {out[name][0]:+.4f} se {out[name][1]:.4f} ({abs(out[name][0]) / out[name][1]:.2f} standard errors)")
    assert abs(dev_c) <= 3 * se_c, "the control (independent one-candidate frames) fails the check itself"
    for name in ("uniform", "power"):
        assert abs(out[name][0]) <= 3 * out[name][1], name


# ---------------------------------------------------------------------------------------------------- CPU: noise
def glossy_scene(dxrs):
    """where BSDF sampling should win: a ground of roughness 0.1 and one large emitter a little above it"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(2, SPHERE_DTYPE)
    spheres[0] = (0.0, -1000.0, 0.0, 1000.0)
    spheres[1] = (0.0, 2.6, 2.0, 2.5)
    mats = default_material(2)
    mats["BaseColor"][:, :3] = [(0.6, 0.55, 0.5), (0, 0, 0)]
    mats["Roughness"] = [0.1, 0.5]
    mats["Metallic"] = [0.8, 0.0]
    mats["EmissiveColor"][1] = (1.0, 0.9, 0.8)
    mats["EmissiveStrength"][1] = 5.0
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.1, 0.1, 0.1, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    return spheres, mats, sd


# measured on the CPU: single-frame RMSE against the quadrature of {8 local + 1 BRDF candidate} over that of {9 local candidates}, reuse
# off, 24 x 16 pixels, 48 frames; the bound is halfway between it and 1 (the rule of test_noise_ratio_against_one_candidate)
GLOSSY_NOISE_RATIO_MEASURED = 0.071


def test_noise_on_a_glossy_ground_next_to_a_large_emitter(dxrs, host, oracle, shims):
    w, h, frames = 24, 16, 48
    spheres, mats, sd = glossy_scene(dxrs)
    cam = host.camera_matrices(w, h, position=(0.0, 1.5, -7.0), look_at=(0.0, 0.5, 0.0), hfov=math.radians(60), jitter=False)
    gb, ids = cpu_gbuffer((shims[2], shims[3]), oracle, cam, w, h, spheres, mats, sd)
    quad = quadrature_image(ref.Scene(spheres, mats), gb, w * h, tuple(float(x) for x in cam.Position), 48)
    assert (quad > 0).sum() > w * h // 4

    def rmse(**kw):
        hp, out = MisHostPass(shims, spheres, mats), []
        for f in range(frames):
            d, s = hp.frame(gb, w, h, cam, frame_index=f, temporal=False, spatial=False, reset_history=True, **kw)
            out.append(np.where(d[:, :1].view(np.uint32) == SENTINEL.view(np.uint32), 0.0, d[:, :3].astype(np.float64) + s[:, :3]) @ LUM)
        return math.sqrt(((np.array(out) - quad[None, :]) ** 2).mean())
    mixed, local = rmse(initial_samples=8, candidates=dict(brdf_samples=1)), rmse(initial_samples=9)
    print(f"single-frame RMSE: 8 + 1 candidates {mixed:.5f}, 9 + 0 candidates {local:.5f}, ratio {mixed / local:.3f}")
    assert mixed / local < (GLOSSY_NOISE_RATIO_MEASURED + 1.0) / 2


# ---------------------------------------------------------------------------------------------------- CPU: the boiling filter
def host_boiling(rm, w, strength):
    w = np.ascontiguousarray(w, np.float32)
    n, flags = C.c_uint32(0), np.zeros(64, np.uint32)
    s = rm.rm_host_boiling(w.ctypes.data, strength, C.byref(n), flags.ctypes.data)
    return np.float32(s), n.value, flags.astype(bool)


def test_boiling_filter_known_answers(shims):
    rm = shims[0]
    assert rm.rm_host_boiling_multiplier(0.2) == 41.0 and rm.rm_host_boiling_multiplier(1.0) == 1.0
    assert rm.rm_host_boiling_multiplier(0.0) == np.float32(np.float32(10.0) / np.float32(1e-6)) - np.float32(9.0)  # clamped, finite
    ones = np.ones(64, np.float32)
    w = ones.copy(); w[23] = 42.0
    s, n, flags = host_boiling(rm, w, 0.2)   # mean 105 / 64 = 1.64, times 41 = 67.3 > 42
    assert (s, n) == (105.0, 64) and not flags.any()
    w[23] = 200.0
    s, n, flags = host_boiling(rm, w, 0.2)   # mean 263 / 64 = 4.11, times 41 = 168.5 < 200
    assert (s, n) == (263.0, 64) and flags.sum() == 1 and flags[23]
    # strength 1: everything above the mean of the nonzero weights
    rng = np.random.default_rng(3)
    w = rng.uniform(0.1, 5.0, 64).astype(np.float32)
    w[::5] = 0.0
    s, n, flags = host_boiling(rm, w, 1.0)
    assert n == int((w > 0).sum()) and np.array_equal(flags, w > np.float32(s / np.float32(n)))
    assert flags.any() and not flags[w == 0].any()
    # all zero: nothing changes, whatever the strength
    for strength in (0.0, 0.2, 1.0):
        s, n, flags = host_boiling(rm, np.zeros(64, np.float32), strength)
        assert (s, n) == (0.0, 0) and not flags.any()
    # lanes without a surface (weight 0) count neither in S nor in n: 10 lanes of 1 and one of 30, mean 40 / 11, not 40 / 64
    w = np.zeros(64, np.float32); w[:10] = 1.0; w[40] = 30.0
    s, n, flags = host_boiling(rm, w, 1.0)
    assert (s, n) == (40.0, 11) and flags.sum() == 1 and flags[40]
    assert host_boiling(rm, w, 0.2)[2].sum() == 0  # 30 < 41 * 40 / 11
    # the sum is the six-level butterfly, bit for bit: weights over 12 decades, whose float32 sum depends on the order
    for seed in range(8):
        w = (10.0 ** np.random.default_rng(seed).uniform(-6, 6, 64)).astype(np.float32)
        s, n, flags = host_boiling(rm, w, 0.2)
        want = mref.butterfly_sum32(w)
        assert s.view(np.uint32) == want.view(np.uint32), (seed, s, want)
        S, n64, f64 = mref.boiling(w, 0.2)
        assert n == n64 and np.array_equal(flags, f64)
    assert any(mref.butterfly_sum32(w) != np.float32(np.sum(w.astype(np.float32)[::-1], dtype=np.float32)) for w in
               [(10.0 ** np.random.default_rng(s).uniform(-6, 6, 64)).astype(np.float32) for s in range(8)]), "the order matters for these weights"


def test_boiling_filter_stops_an_over_weighted_reservoir(shims, cpu_case):
    """one history reservoir's W overwritten with a huge value: with the filter on the pixel stores M = 0 and the next frame does not
    reuse it; with the filter off it does"""
    spheres, mats, sd, cam, gb = cpu_case
    n = W * H
    results = {}
    for name, cd in (("on", dict(boiling_filter=0.2)), ("off", NO_EXTRAS)):
        hp = MisHostPass(shims, spheres, mats)
        kw = dict(spatial=False, candidates=cd)
        hp.frame(gb, W, H, cam, frame_index=0, reset_history=True, **kw)
        slot = hp.slot(hp.cur)
        lit = np.flatnonzero(np.isfinite(slot[3][:, 2]) & (slot[5][:, 3] > 0) & (slot[6][:, 1] > 0))
        # a lit pixel in the interior of an 8x8 block whose other lanes mostly hold surfaces
        px = next(int(i) for i in lit if np.isfinite(slot[3][:, 2].reshape(H, W)[(i // W) // 8 * 8:(i // W) // 8 * 8 + 8, (i % W) // 8 * 8:(i % W) // 8 * 8 + 8]).sum() > 48)
        slot[5][px, 3] = 1e9
        hp.frame(gb, W, H, cam, frame_index=1, **kw)
        after = reservoirs(hp.slot(hp.cur))[px]
        hp.frame(gb, W, H, cam, frame_index=2, **kw)
        results[name] = (after, reservoirs(hp.slot(hp.cur))[px])
    after, later = results["on"]
    assert after["M"] == 0 and after["W"] == 0, after
    assert later["M"] == 8, f"the next frame found no history at the pixel: {later}"
    after, later = results["off"]
    assert after["M"] == 16 and after["W"] > 1e3, after
    assert later["M"] == 24, later


# ---------------------------------------------------------------------------------------------------- CPU: sanitizers
def test_header_paths_under_sanitizers(tmp_path):
    """tests/cpp/restir_mis_sanitize.cpp: spec S23's header paths under AddressSanitizer + UBSan as a stand-alone program"""
    import __graft_entry__ as g
    exe = g.build_restir_mis_sanitizer(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "restir_mis_sanitize ok" in res.stdout, res.stdout + res.stderr


# ---------------------------------------------------------------------------------------------------- GPU
# small presampled structures: a call rebuilds them on both sides
GPU_POWER = sampling(POWER, tile_size=100, tile_count=3)
GPU_REGIR = sampling(REGIR, tile_size=100, tile_count=3, grid_size=4, lights_per_cell=70, cell_size=4.0)
MODES = dict(uniform=None, power=GPU_POWER, regir=GPU_REGIR)


def gpu_ex_frame(r, hp, w, h, cam, what, ls, cd, **kw):
    """one pt_restir_di_ex call (sentinel-filled outputs) against the host-compiled header fed the same G-buffer: every word of Diffuse
    and Specular, unwritten pixels included, and both slots of the history (pt_restir_di_history)"""
    had_history = hp.valid and hp.size == (w, h)
    dd, ds, gb = r.restir_di(fill=SENTINEL, light_sampling=ls, candidates=cd, **kw)
    gbn = {name: gb[name].cpu().numpy().reshape(w * h, -1) for name in INPUTS}
    want_d, want_s = hp.frame(gbn, w, h, cam, light_sampling=ls, candidates=cd, **kw)
    got_d, got_s = dd.cpu().numpy().reshape(-1, 4), ds.cpu().numpy().reshape(-1, 4)
    for got, want, name in ((got_d, want_d, "Diffuse"), (got_s, want_s, "Specular")):
        diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {w * h} pixels differ, first {int(np.argmax(diff))}: {got[np.argmax(diff)]} != {want[np.argmax(diff)]}"
    history_equal(r, hp, w, h, 0, what)
    if had_history:
        history_equal(r, hp, w, h, 1, what)
    return got_d[:, 0:1].view(np.uint32)[:, 0] != SENTINEL.view(np.uint32), got_d, gbn


def demo_case(dxrs, host, w, h, **cam_kw):
    spheres, mats, sd = make_scene(dxrs)
    return spheres, mats, sd, host.camera_matrices(w, h, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), **cam_kw)


RAGGED_CASES = [("uniform", 1, None), ("uniform", 8, 0.2), ("power", 1, 0.2), ("power", 8, 1.0), ("regir", 1, 1.0), ("regir", 8, None), ("uniform", 0, 0.2),
                ("power", 0, 1.0), ("regir", 0, 0.2)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,n_brdf,strength", RAGGED_CASES, ids=[f"{m}-{n}-{s}" for m, n, s in RAGGED_CASES])
def test_gpu_ragged_blocks(dxrs, host, renderer, shims, mode, n_brdf, strength):
    """19 x 13: ragged 8x8 blocks on both axes -- edge waves whose lanes outside the image still take part in the filter's butterfly --
    over three frames with the history running; N_B in {0, 1, 8} x the three sampling modes x the filter off, at 0.2 and at 1"""
    w, h = 19, 13
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = MisHostPass(shims, spheres, mats)
    cd = dict(brdf_samples=n_brdf, boiling_filter=strength)
    emptied = 0
    for f in range(3):
        gpu_ex_frame(renderer, hp, w, h, cam, f"frame {f}", MODES[mode], cd, frame_index=f, reset_history=f == 0, spatial_samples=2, spatial_radius=6.0)
        slot = hp.slot(hp.cur)
        emptied += int((np.isfinite(slot[3][:, 2]) & (slot[6][:, 0] == 0)).sum())
    if strength == 1.0:
        assert emptied > 0, "strength 1 empties every reservoir above its block's mean"


@pytest.mark.gpu
def test_gpu_four_frames_travelling_camera(dxrs, host, renderer, shims):
    """67 x 45 over four frames of a travelling camera with the reference's defaults (ReGIR_RIS, 8 + 1 candidates, filter 0.2) and
    Raytraced temporal correction: reprojection accepts some surfaces and rejects others"""
    w, h = 67, 45
    spheres, mats, sd = make_scene(dxrs)
    hp = MisHostPass(shims, spheres, mats)
    renderer.set_scene(spheres, mats, sd)
    renderer.set_textures(None)
    prev, lit = None, 0
    for f in range(4):
        cam = host.camera_matrices(w, h, position=(0.3 * f, 2.5 + 0.05 * f, -9.0 + 0.4 * f), look_at=(0.1 * f, 1.0, 0.0), hfov=math.radians(70), jitter_index=f, previous=prev)
        renderer.set_camera(cam)
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=2, spp=1))
        written, _, _ = gpu_ex_frame(renderer, hp, w, h, cam, f"frame {f}", GPU_REGIR, REFERENCE_DEFAULTS, frame_index=f, reset_history=f == 0, temporal_bias=RAYTRACED,
                                     spatial_samples=2)
        lit += int(written.sum())
        if f > 0:
            slot = hp.slot(hp.cur)
            m = slot[6][np.isfinite(slot[3][:, 2]), 0]
            assert (m > 9).any() and (m == 9).any(), f"frame {f}: M {np.unique(m)}"
        prev = cam
    assert lit > 4 * w * h // 10


@pytest.mark.gpu
@pytest.mark.parametrize("tb,sb", [(OFF, OFF), (BASIC, RAYTRACED), (RAYTRACED, BASIC)])
def test_gpu_bias_modes(dxrs, host, renderer, shims, tb, sb):
    w, h = 40, 24
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = MisHostPass(shims, spheres, mats)
    for f in range(2):
        gpu_ex_frame(renderer, hp, w, h, cam, f"frame {f}", GPU_POWER, REFERENCE_DEFAULTS, frame_index=f, reset_history=f == 0, temporal_bias=tb, spatial_bias=sb,
                     spatial_samples=2)


@pytest.mark.gpu
def test_gpu_textured_emitter_and_alpha_mapped_blocker(dxrs, host, renderer, shims):
    """test_restir_pass's textured scene: BRDF rays go through the alpha-tested walker (the blocker's base-colour map has holes in its
    alpha) and may find the emitter with the emissive map"""
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
    ts.maps[E0, 1] = ts.add_image(glow)
    ts.maps[BLOCKER, 0] = ts.add_image(holes)
    cam = host.camera_matrices(w, h, **CAM)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h, textures=ts)
    hp = MisHostPass(shims, spheres, mats, textures=ts)
    opaque = mats.copy()
    opaque["AlphaMode"][BLOCKER] = 0
    hp_opaque = MisHostPass(shims, spheres, opaque, textures=ts)
    cd = dict(brdf_samples=8, boiling_filter=0.2)
    crossed = 0
    try:
        for f in range(2):
            written, got_d, gbn = gpu_ex_frame(renderer, hp, w, h, cam, f"frame {f}", None, cd, frame_index=f, reset_history=f == 0, spatial_samples=2)
            # the same launch 1 with the blocker opaque: a different reservoir means a ray went through its alpha-tested crossings
            hp_opaque.frame(gbn, w, h, cam, candidates=cd, frame_index=f, reset_history=f == 0, spatial_samples=2)
            crossed += int((hp.slot(hp.cur)[5].view(np.uint32) != hp_opaque.slot(hp_opaque.cur)[5].view(np.uint32)).any(axis=1).sum())
    finally:
        renderer.set_textures(None)
    assert crossed > 0, "no ray met the alpha-mapped blocker"


@pytest.mark.gpu
def test_gpu_scene_in_global_memory(dxrs, host, shims):
    """the 10^5-sphere tree in global memory (the wide walker): BRDF rays and the filter, two frames"""
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
        hp = MisHostPass(shims, spheres, mats)
        for f in range(2):
            written, _, _ = gpu_ex_frame(r, hp, w, h, cam, f"frame {f}", GPU_POWER, REFERENCE_DEFAULTS, frame_index=f, reset_history=f == 0)
            assert written.sum() > 4, f"frame {f}: the emitters light {int(written.sum())} pixels"
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_moved_spheres_and_zero_emitters(dxrs, host, renderer, shims):
    """spheres moved by pt_update_spheres between frames keep the history and are seen by the BRDF rays, the emitter index and the
    pyramid; a scene without emitters writes nothing"""
    w, h = 40, 24
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = MisHostPass(shims, spheres, mats)
    gpu_ex_frame(renderer, hp, w, h, cam, "first", GPU_REGIR, REFERENCE_DEFAULTS, frame_index=0, reset_history=True)
    moved = spheres.copy()
    moved["cy"][1:] += 0.05
    moved["cx"][E0] += 0.5
    renderer.update_spheres(moved)
    hp.spheres = np.ascontiguousarray(moved)
    gpu_ex_frame(renderer, hp, w, h, cam, "moved", GPU_REGIR, REFERENCE_DEFAULTS, frame_index=1)
    gpu_ex_frame(renderer, hp, w, h, cam, "moved, next", GPU_REGIR, REFERENCE_DEFAULTS, frame_index=2)
    dark = mats.copy()
    dark["EmissiveStrength"] = 0.0
    gpu_setup(renderer, dxrs, spheres, dark, sd, cam, w, h)
    dd, ds, _ = renderer.restir_di(fill=SENTINEL, candidates=REFERENCE_DEFAULTS, light_sampling=GPU_REGIR)
    for t in (dd, ds):
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_extras_off_and_alternating_entry_points(dxrs, host, renderer, shims):
    """candidates NULL, or BrdfSamples 0 with the filter off: pt_restir_di_sampled's bits (and pt_restir_di's in Uniform mode); the
    three entry points alternate on one context and share the history"""
    w, h = 40, 24
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = MisHostPass(shims, spheres, mats)

    def frame(f, what, ls, cd):
        """through the binding's own choice of entry point: candidates None and light_sampling None = pt_restir_di; candidates None =
        pt_restir_di_sampled; otherwise pt_restir_di_ex -- each against the one host model"""
        dd, ds, gb = renderer.restir_di(fill=SENTINEL, light_sampling=ls, candidates=cd, frame_index=f, reset_history=f == 0, spatial_samples=2)
        gbn = {name: gb[name].cpu().numpy().reshape(w * h, -1) for name in INPUTS}
        want_d, want_s = hp.frame(gbn, w, h, cam, light_sampling=ls, candidates=cd, frame_index=f, reset_history=f == 0, spatial_samples=2)
        assert same_bits(dd.cpu().numpy().reshape(-1, 4), want_d) and same_bits(ds.cpu().numpy().reshape(-1, 4), want_s), what
        history_equal(renderer, hp, w, h, 0, what)
        if f > 0:
            history_equal(renderer, hp, w, h, 1, what)
    frame(0, "pt_restir_di", None, None)
    frame(1, "pt_restir_di_ex, extras off, Uniform", None, NO_EXTRAS)
    frame(2, "pt_restir_di_sampled", GPU_POWER, None)
    frame(3, "pt_restir_di_ex, extras off, Power_RIS", GPU_POWER, NO_EXTRAS)
    frame(4, "pt_restir_di_ex", GPU_REGIR, REFERENCE_DEFAULTS)
    frame(5, "pt_restir_di", None, None)
    frame(6, "pt_restir_di_ex, filter only", None, dict(boiling_filter=0.2))
    frame(7, "pt_restir_di_sampled", GPU_REGIR, None)
    # NULL candidates through the C-ABI itself
    import torch
    from dxrs_amd.abi_types import GBUFFER_CHANNELS, PtRestirDiSettings, PtRestirDiTextures, light_sampling_settings
    width = dict(GBUFFER_CHANNELS)
    gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS}
    outs = [torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)).cuda() for _ in range(2)]
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({n: b.data_ptr() for n, b in gb.items()})
    s = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h), FrameIndex=9, ResetHistory=1, EnableTemporal=1, EnableSpatial=1)
    ls = light_sampling_settings(mode=POWER, tile_size=100, tile_count=3)
    for k, call in enumerate((lambda t: renderer._lib.pt_restir_di_ex(renderer._ctx, C.byref(s), C.byref(ls), None, C.byref(t)),
                              lambda t: renderer._lib.pt_restir_di_sampled(renderer._ctx, C.byref(s), C.byref(ls), C.byref(t)))):
        t = PtRestirDiTextures(**dict({n: C.c_void_p(b.data_ptr()) for n, b in gb.items()}, Diffuse=C.c_void_p(outs[k][0].data_ptr()), Specular=C.c_void_p(outs[k][1].data_ptr())))
        assert call(t) == 0
        renderer.synchronize()
    assert same_bits(outs[0].cpu().numpy(), outs[1].cpu().numpy())
    assert (outs[0].cpu().numpy().view(np.uint32) != SENTINEL.view(np.uint32)).any()
    hp.valid = False


@pytest.mark.gpu
def test_gpu_argument_errors_leave_outputs_and_history_untouched(dxrs, host, renderer, shims):
    import torch
    w, h = 40, 24
    spheres, mats, sd, cam = demo_case(dxrs, host, w, h, jitter=False)
    gpu_setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    hp = MisHostPass(shims, spheres, mats)
    gpu_ex_frame(renderer, hp, w, h, cam, "first", None, REFERENCE_DEFAULTS, frame_index=0, reset_history=True)
    before = renderer.restir_di_history(w, h, 0)
    from dxrs_amd.abi_types import GBUFFER_CHANNELS, PtLightSamplingSettings, PtRestirDiCandidates, PtRestirDiSettings, PtRestirDiTextures
    width = dict(GBUFFER_CHANNELS)
    gb = {n: torch.zeros((h, w, width[n]), dtype=torch.float32, device="cuda") for n in INPUTS}
    out = torch.from_numpy(np.full((2, h, w, 4), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({n: b.data_ptr() for n, b in gb.items()})
    renderer.synchronize()
    lib, ctx = renderer._lib, renderer._ctx
    s = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h), FrameIndex=1, EnableTemporal=1, EnableSpatial=1)
    t = PtRestirDiTextures(**dict({n: C.c_void_p(b.data_ptr()) for n, b in gb.items()}, Diffuse=C.c_void_p(out[0].data_ptr()), Specular=C.c_void_p(out[1].data_ptr())))

    def status(ls=None, **fields):
        cd = PtRestirDiCandidates(**fields)
        return lib.pt_restir_di_ex(ctx, C.byref(s), C.byref(ls) if ls is not None else None, C.byref(cd), C.byref(t))
    INVALID = 1
    assert lib.pt_restir_di_ex(ctx, None, None, None, None) == INVALID and lib.pt_restir_di_ex(ctx, C.byref(s), None, None, None) == INVALID
    assert status(BrdfSamples=9) == INVALID and status(EnableBoilingFilter=2) == INVALID and status(BrdfSamples=1, _pad=1) == INVALID
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert status(EnableBoilingFilter=1, BoilingFilterStrength=bad) == INVALID, bad
    assert status(PtLightSamplingSettings(Mode=3), BrdfSamples=1) == INVALID          # the siblings' errors hold
    s_bad = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(w, h), InitialSamples=33)
    assert lib.pt_restir_di_ex(ctx, C.byref(s_bad), None, C.byref(PtRestirDiCandidates(BrdfSamples=1)), C.byref(t)) == INVALID
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    after = renderer.restir_di_history(w, h, 0)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]), "a rejected call touched the history"
    assert status(BrdfSamples=8, EnableBoilingFilter=1, BoilingFilterStrength=0.0) == 0  # strength 0 is legal (clamped to 1e-6)
    assert status(BrdfSamples=0, EnableBoilingFilter=0, BoilingFilterStrength=float("nan")) == 0  # read only when the filter is enabled
    renderer.synchronize()
    assert (out.cpu().numpy().view(np.uint32) != SENTINEL.view(np.uint32)).any()


@pytest.mark.gpu
def test_gpu_chain_three_lanes_with_the_reference_defaults(dxrs, host):
    """pt_render_gbuffer -> pt_restir_di_ex (ReGIR_RIS, 8 + 1 candidates, filter 0.2) -> pt_render_with_di with three frames in flight, one
    buffer set per lane, no host wait in between: the frames equal, bit for bit, the same frames fed a downloaded and re-uploaded copy of
    the DI"""
    import torch
    w, h, frames, mode = 64, 48, 5, 3
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    from dxrs_amd.abi_types import GBUFFER_CHANNELS
    width = dict(GBUFFER_CHANNELS)
    ls = sampling(REGIR, tile_size=256, tile_count=16, grid_size=8, lights_per_cell=64, cell_size=4.0)

    def run(reupload):
        r = dxrs.Renderer(device=0, frames_in_flight=3)
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
                r.set_camera(host.camera_matrices(w, h, jitter_index=f))
                r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=4, spp=1))
                if reupload or f >= 3:
                    r.synchronize()
                    for t in (s["dd"], s["ds"], s["nd"], s["ns"]):
                        t.zero_()
                    torch.cuda.synchronize()
                ptrs = {n: b.data_ptr() for n, b in s["gb"].items()}
                r.render_gbuffer_device(ptrs)
                dd, ds = s["dd"], s["ds"]
                r.restir_di_device(w, h, dict(ptrs, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), frame_index=f, spatial_samples=2, light_sampling=ls,
                                   candidates=REFERENCE_DEFAULTS)
                if reupload:
                    r.synchronize()
                    dd, ds = torch.from_numpy(dd.cpu().numpy().copy()).cuda(), torch.from_numpy(ds.cpu().numpy().copy()).cuda()
                    torch.cuda.synchronize()
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
def test_gpu_cpp_host_mirror(dxrs, host, shims, tmp_path):
    """RTXDI (host/RTXDI.hpp) bound to pt_restir_di_ex from C++ with the reference's BRDFSamples and BoilingFilter and Power_RIS candidates
    at the library's default sizes, three frames of the demo scene: every pixel the host-compiled header writes from the program's own
    G-buffer holds the same bits, and every other pixel keeps what the buffers held before the pass"""
    from types import SimpleNamespace
    from test_restir_pass import WIDTH
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_restir_di_ex")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_restir_di_ex.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h, frames = 96, 64, 3
    outp = str(tmp_path / "restir.f32")
    res = subprocess.run([exe, str(w), str(h), str(frames), outp, "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout and "BrdfSamples" in res.stdout
    data = np.fromfile(outp, dtype=np.float32)
    n = w * h
    per_frame = 6 + n * (sum(WIDTH.values()) + 16)
    assert len(data) == frames * per_frame
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    hp = MisHostPass(shims, spheres, mats)
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
        want_d, want_s = hp.frame(gb, w, h, cam, frame_index=f, reset_history=f == 0, spatial_samples=2, light_sampling=sampling(POWER), candidates=REFERENCE_DEFAULTS)
        written = want_d[:, 0:1].view(np.uint32)[:, 0] != SENTINEL.view(np.uint32)
        lit += int(written.sum())
        for got, want, before, name in ((got_d, want_d, before_d, "Diffuse"), (got_s, want_s, before_s, "Specular")):
            expect = np.where(written[:, None], want, before)
            assert np.array_equal(got.view(np.uint32), expect.view(np.uint32)), f"frame {f} {name}"
    assert lit > 0
