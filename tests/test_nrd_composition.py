"""Row N8 -- the NRD composition pass (pt_nrd_composition: PostProcessing::NRDComposition, Shaders/NRDComposition.hlsl, App::ProcessNRD;
DESIGN.md spec S14).
CPU: the product's header (csrc/pt_nrd.h compiled as host C++ by tests/hostshim/nrd_host.cpp) against the float64 numpy restatement
(tests/nrd_reference.py) and hand-derived known answers; the identity chain (pack, copy, compose) on the oracle's N7 outputs and the
G-buffer header, against the oracle's frame -- where its tolerance and mask coverage are chosen.
GPU: pt_nrd_composition against the host-compiled header bit for bit (random images, the real chain); the identity chain against
pt_render; frames in flight; argument errors; the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nrd_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REBLUR, RELAX = 2, 3
P_DEFAULT = np.array(ref.HIT_DISTANCE, np.float32)
SENTINEL = np.uint32(0x7FC0BEEF).view(np.float32)  # a NaN with a payload: survives exactly where nothing is written
# The identity chain reproduces the frame on the pixels of CHAIN_MASK within CHAIN_RTOL of the pixel's largest channel: pack and
# compose round the albedo quotient and product (and ReBLUR the YCoCg round trip) once each.  On the oracle's frames the largest
# error seen was 4.4e-7 (ReBLUR) / 1.1e-7 (ReLAX).
CHAIN_RTOL = 2e-6
# The C2 crop of the chain tests (demo scene, 1920x1080, frame 0, no DI): 62.5 % of its pixels hit; 14.7 % of the hits are in the mask;
# nearly all others have a zero albedo channel (metals: no diffuse albedo) -- there a lobe is zeroed, as the spec says.
C2_CROP = (720, 405, 480, 270)
C2_CROP_COVERAGE = (0.14, 0.16)


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_nrd_shim())
    vp, u32, f = C.c_void_p, C.c_uint32, C.c_float
    lib.nrd_host.restype = None
    lib.nrd_host.argtypes = [u32, C.c_int, u32] + [vp] * 10
    lib.nrd_norm_hit_dist_host.restype = f
    lib.nrd_norm_hit_dist_host.argtypes = [f, f, vp, f]
    lib.nrd_to_ycocg.restype = None
    lib.nrd_to_ycocg.argtypes = [vp, vp]
    lib.nrd_from_ycocg.restype = None
    lib.nrd_from_ycocg.argtypes = [vp, vp]
    return lib


def c32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def host_pass(shim, mode, pack, bufs, P=P_DEFAULT):
    """one pt_nrd_composition call on the host-compiled header; bufs: {NRD texture name: array}.  Returns copies of the written buffers:
    (NoisyDiffuse, NoisySpecular) for pack, Radiance for compose."""
    b = {k: c32(v).copy() for k, v in bufs.items() if v is not None}
    n = b["LinearDepth"].size
    p = lambda k: b[k].ctypes.data if k in b else None  # noqa: E731
    P = c32(P)
    shim.nrd_host(n, 1 if pack else 0, mode, P.ctypes.data, p("LinearDepth"), p("DiffuseAlbedo"), p("SpecularAlbedo"), p("NormalRoughness"),
                  p("NoisyDiffuse"), p("NoisySpecular"), p("DenoisedDiffuse"), p("DenoisedSpecular"), p("Radiance"))
    return (b["NoisyDiffuse"], b["NoisySpecular"]) if pack else b["Radiance"]


def random_inputs(rng, n, special=True):
    """{name: array (n, k)} of plausible G-buffer / lobe values plus, with `special`, the edge cases of S14"""
    depth = rng.uniform(0.1, 200.0, n).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    da = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    sa = rng.uniform(0.02, 1.0, (n, 3)).astype(np.float32)
    nr = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
    nr[:, 3] = rng.uniform(0.0, 1.0, n)
    lobes = []
    for _ in range(4):
        x = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), (n, 4))).astype(np.float32)
        x[:, 3] = rng.choice([0.0, 1.0], n) * np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n))
        x[rng.random((n, 4)) < 0.05] = 0.0
        lobes.append(x)
    rad = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (n, 4))).astype(np.float32)
    if special:
        pick = lambda p: rng.random(n) < p  # noqa: E731
        depth[pick(0.05)] = np.inf
        depth[pick(0.02)] = -np.inf
        depth[pick(0.02)] = np.nan
        depth[pick(0.02)] = 0.0
        for alb in (da, sa):
            vals = np.float32([0.0, -0.0, 1e-45, 1e-40, 1.17e-38, -0.25, 1e-30])
            m = rng.random((n, 3)) < 0.03
            alb[m] = vals[rng.integers(0, len(vals), int(m.sum()))]
        for x in lobes + [rad]:
            vals = np.float32([np.nan, np.inf, -np.inf, -1.0, 7e4, 1e30, SENTINEL])
            m = rng.random((n, 3)) < 0.02
            x[:, :3][m] = vals[rng.integers(0, len(vals), int(m.sum()))]
        for x in lobes:
            vals = np.float32([0.0, np.inf, np.nan, 1e30, 7e4, 65504.0, 1e-9, -2.0])
            m = pick(0.1)
            x[m, 3] = vals[rng.integers(0, len(vals), int(m.sum()))]
        nr[pick(0.05), 3] = 0.0
        nr[pick(0.05), 3] = 1.0
    return dict(LinearDepth=depth, DiffuseAlbedo=da, SpecularAlbedo=sa, NormalRoughness=nr, NoisyDiffuse=lobes[0], NoisySpecular=lobes[1],
                DenoisedDiffuse=lobes[2], DenoisedSpecular=lobes[3], Radiance=rad)


def assert_close(got, want, scale, rtol, what):
    """got (float32) against want (float64): NaN masks equal, |got - want| <= rtol * scale elsewhere (scale broadcast per pixel)"""
    got = got.astype(np.float64)
    with np.errstate(over="ignore"):
        want = want.astype(np.float32).astype(np.float64)  # (what overflows float32 is inf there too)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ at {np.argwhere(gn != wn)[:5].tolist()}"
    ok = ~gn
    same_inf = (got == want)
    with np.errstate(invalid="ignore"):
        err = np.where(same_inf | ~ok, 0.0, np.abs(got - want))
    bound = rtol * np.broadcast_to(scale, got.shape) + 1e-37
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{what}: {len(bad)} values off, first {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("mode", [REBLUR, RELAX])
@pytest.mark.parametrize("seed", [0, 1])
def test_header_pack_matches_numpy_restatement(shim, mode, seed):
    rng = np.random.default_rng(seed)
    x = random_inputs(rng, 20000)
    got_d, got_s = host_pass(shim, mode, True, {k: x[k] for k in ref_keys(True)})
    want_d, want_s = ref.pack(mode, x["LinearDepth"], x["DiffuseAlbedo"], x["SpecularAlbedo"], x["NormalRoughness"], x["NoisyDiffuse"],
                              x["NoisySpecular"])
    hit = np.isfinite(x["LinearDepth"])
    for got, want, src in ((got_d, want_d, x["NoisyDiffuse"]), (got_s, want_s, x["NoisySpecular"])):
        # misses: untouched, bit for bit (the NaN payloads included)
        assert np.array_equal(got[~hit].view(np.uint32), src[~hit].view(np.uint32))
        scale = np.maximum(np.abs(want[:, :3]).max(axis=1, keepdims=True), 1e-30)
        assert_close(got[hit, :3], want[hit, :3], scale[hit], 4e-7, f"mode {mode} rgb")
        assert_close(got[hit, 3:], want[hit, 3:], np.abs(want[hit, 3:]), 2e-6, f"mode {mode} hit distance")
        assert np.isfinite(got[hit]).all()
        zeroed = hit & ~np.isfinite(ref.quotient(src, x["DiffuseAlbedo"] if src is x["NoisyDiffuse"] else x["SpecularAlbedo"])).all(axis=1)
        assert zeroed.sum() > 50
        if mode == RELAX:
            assert (got[zeroed, :3] == 0).all()  # (ReBLUR: YCoCg of 0 is 0 too, checked by the restatement)
    # the edge cases were drawn
    assert (~hit).sum() > 1000 and (x["DiffuseAlbedo"] == 0).any() and np.isnan(x["NoisyDiffuse"]).any()


def ref_keys(pack):
    return ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo") + (("NormalRoughness", "NoisyDiffuse", "NoisySpecular") if pack else
                                                                 ("DenoisedDiffuse", "DenoisedSpecular", "Radiance"))


@pytest.mark.parametrize("mode", [REBLUR, RELAX])
@pytest.mark.parametrize("seed", [0, 1])
def test_header_compose_matches_numpy_restatement(shim, mode, seed):
    rng = np.random.default_rng(10 + seed)
    x = random_inputs(rng, 20000)
    if mode == REBLUR:  # denoised ReBLUR data is YCoCg: give it plausible (signed) chroma
        for k in ("DenoisedDiffuse", "DenoisedSpecular"):
            x[k][:, 1:3] *= rng.uniform(-0.5, 0.5, (len(x[k]), 2)).astype(np.float32)
    got = host_pass(shim, mode, False, {k: x[k] for k in ref_keys(False)})
    want, scale = ref.compose(mode, x["LinearDepth"], x["DiffuseAlbedo"], x["SpecularAlbedo"], x["DenoisedDiffuse"], x["DenoisedSpecular"],
                              x["Radiance"])
    hit = np.isfinite(x["LinearDepth"])
    assert np.array_equal(got[~hit].view(np.uint32), x["Radiance"][~hit].view(np.uint32))
    assert np.array_equal(got[:, 3].view(np.uint32), x["Radiance"][:, 3].view(np.uint32))  # alpha untouched
    assert_close(got[hit, :3], want[hit, :3], scale[hit], 1e-6, f"mode {mode} compose")


def test_known_answers(shim):
    P = P_DEFAULT
    # NormHitDist at the default P = {3, 0.1, 20, -25}: f = (3 + 0.1 |z|) (1 + 19 saturate(exp2(-25 r^2)))
    #   r = 1: exp2(-25) = 2.98e-8 -> f = (3 + 0.1 |z|) (1 + 5.66e-7); r = 0: f = 20 (3 + 0.1 |z|); r = 0.2: exp2(-1) = 0.5 -> f = 10.5 (...)
    cases = [(2.0, 10.0, 1.0, 2.0 / (4.0 * (1 + 19 * 2.0 ** -25))), (2.0, -10.0, 1.0, 2.0 / (4.0 * (1 + 19 * 2.0 ** -25))),
             (40.0, 10.0, 0.0, 0.5), (21.0, 0.0, 0.2, 21.0 / (3.0 * 10.5)), (5.0, 20.0, 1.0, 1.0), (0.0, 5.0, 0.5, 0.0),
             (np.inf, 5.0, 0.5, 1.0)]
    for h, z, r, want in cases:
        got = shim.nrd_norm_hit_dist_host(h, z, P.ctypes.data, r)
        assert got == pytest.approx(want, rel=2e-6, abs=0), (h, z, r)
    # YCoCg: (1, 0, 0) -> (.25, .5, -.25); (0, 1, 0) -> (.5, 0, .5); a round trip is exact on dyadic values
    out = np.empty(3, np.float32)
    for rgb, ycocg in (((1, 0, 0), (0.25, 0.5, -0.25)), ((0, 1, 0), (0.5, 0.0, 0.5)), ((0, 0, 1), (0.25, -0.5, -0.25))):
        shim.nrd_to_ycocg(np.float32(rgb).ctypes.data, out.ctypes.data)
        assert out.tolist() == list(ycocg)
    for rgb in ((1.0, 2.0, 3.0), (0.5, 0.0, 4.0), (65504.0, 1.0, 0.25)):
        a, b = np.float32(rgb), np.empty(3, np.float32)
        shim.nrd_to_ycocg(a.ctypes.data, out.ctypes.data)
        shim.nrd_from_ycocg(out.ctypes.data, b.ctypes.data)
        assert b.tolist() == a.tolist()
    shim.nrd_from_ycocg(np.float32([0.0, 1.0, 0.0]).ctypes.data, out.ctypes.data)  # r = 1, g = 0, b = -1 -> clamped
    assert out.tolist() == [1.0, 0.0, 0.0]
    shim.nrd_from_ycocg(np.float32([np.nan, 0.0, 0.0]).ctypes.data, out.ctypes.data)  # NaN -> 0, as HLSL max
    assert out.tolist() == [0.0, 0.0, 0.0]
    # ReLAX pack: rgb and hit distance clamped at 65504; a lobe with one infinite channel is black; 0 stays 0, tiny becomes 1e-6
    one = lambda v: np.float32([v])  # noqa: E731
    x = dict(LinearDepth=one(5.0), DiffuseAlbedo=np.float32([[0.5, 1.0, 0.25]]), SpecularAlbedo=np.float32([[1.0, 1.0, 1.0]]),
             NoisyDiffuse=np.float32([[4e4, 7e4, 2.0, 1e9]]), NoisySpecular=np.float32([[np.inf, 1.0, 1.0, 1e-9]]))
    d, s = host_pass(shim, RELAX, True, x)
    assert d.tolist() == [[65504.0, 65504.0, 8.0, 65504.0]]
    assert s[0, :3].tolist() == [0.0, 0.0, 0.0] and s[0, 3] == np.float32(1e-6)
    x["NoisySpecular"] = np.float32([[1.0, 1.0, 1.0, 0.0]])
    x["DiffuseAlbedo"] = np.float32([[0.5, 0.0, 0.25]])  # a zero albedo channel zeroes the whole lobe
    d, s = host_pass(shim, RELAX, True, x)
    assert d[0, :3].tolist() == [0.0, 0.0, 0.0] and s.tolist() == [[1.0, 1.0, 1.0, 0.0]]
    # compose adds the lobes times the albedo, alpha untouched
    r = host_pass(shim, RELAX, False, dict(LinearDepth=one(1.0), DiffuseAlbedo=np.float32([[0.5, 0.5, 0.5]]), SpecularAlbedo=np.float32([[1, 2, 4]]),
                                           DenoisedDiffuse=np.float32([[2, 4, 8, 9]]), DenoisedSpecular=np.float32([[1, 1, 1, 9]]),
                                           Radiance=np.float32([[0.5, 0.25, 0.125, 0.75]])))
    assert r.tolist() == [[2.5, 4.25, 8.125, 0.75]]


def chain_inputs(host, oracle, dxrs, rect, frame):
    """what the GPU chain sees, made on the CPU: the oracle's frame, its N7 outputs (the rules of tests/test_denoiser_outputs.py, buffers
    cleared to 0) and the G-buffer header's channels -> dict of (rh, rw, k) float32 arrays"""
    import __graft_entry__ as g
    from test_denoiser_outputs import expected, sample0
    from test_gbuffer import channel, grid, host_pixels, oracle_hits

    gb = C.CDLL(g.build_gbuffer_shim())
    vp, u32 = C.c_void_p, C.c_uint32
    gb.gb_pixels.restype = None
    gb.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    W, H = 1920, 1080
    cam = host.camera_matrices(W, H, jitter_index=frame)
    gs = dxrs.types.graphics_settings(W, H, bounces=8, spp=1, frame_index=frame)
    res, _ = oracle.render(spheres, mats, sd, cam, gs, rect=rect, threads=8)
    hit, diffuse, hd = sample0(oracle, spheres, mats, sd, cam, gs, rect)
    px, py = grid(*rect)
    t, ids = oracle_hits(oracle, cam, W, H, spheres, px, py)
    vals, _ = host_pixels(gb, cam, W, H, spheres, mats, sd, px, py, t, ids)
    rw, rh = rect[2], rect[3]
    out = {name: np.ascontiguousarray(channel(vals, name)).astype(np.float32).reshape(rh, rw, -1)
           for name in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "Radiance")}
    assert np.array_equal(np.isfinite(out["LinearDepth"][..., 0]), hit)
    out["Frame"] = res
    for mode in (REBLUR, RELAX):
        e = expected(res, out["Radiance"], hit, diffuse, hd, mode)
        out[mode] = dict(Emission=e["out"], NoisyDiffuse=np.where(hit[..., None], e["Diffuse"], 0).astype(np.float32),
                         NoisySpecular=np.where(hit[..., None], e["Specular"], 0).astype(np.float32))
    return out


def check_identity_chain(mode, x, got, frame, coverage=None):
    """the identity chain's Radiance `got` against the frame (all arrays (h, w, k)): within CHAIN_RTOL on the mask; a zeroed lobe where
    an albedo channel is 0; misses untouched.  -> the mask's share of the hit pixels"""
    flat = lambda a: a.reshape(-1, a.shape[-1]).astype(np.float32)  # noqa: E731
    depth, da, sa = flat(x["LinearDepth"])[:, 0], flat(x["DiffuseAlbedo"]), flat(x["SpecularAlbedo"])
    nd, ns, em, fr, got = flat(x["NoisyDiffuse"]), flat(x["NoisySpecular"]), flat(x["Emission"]), flat(frame), flat(got)
    hit = np.isfinite(depth)
    assert np.array_equal(got[~hit].view(np.uint32), em[~hit].view(np.uint32))  # misses: the emission pt_render_denoiser wrote
    assert np.array_equal(got[:, 3].view(np.uint32), em[:, 3].view(np.uint32))
    qd, qs = ref.quotient(nd, da), ref.quotient(ns, sa)
    good = [(a > 0).all(axis=1) & np.isfinite(q).all(axis=1) & (q <= 65504).all(axis=1) for a, q in ((da, qd), (sa, qs))]
    zero = [(a == 0).any(axis=1) for a in (da, sa)]
    mask = hit & good[0] & good[1] & (fr[:, :3] >= em[:, :3]).all(axis=1)
    scale = np.maximum(np.abs(fr[:, :3]).max(axis=1, keepdims=True), 1e-30)
    assert_close(got[mask, :3], fr[mask, :3].astype(np.float64), scale[mask], CHAIN_RTOL, f"mode {mode}: identity chain vs frame")
    # a lobe with a zero albedo channel contributes nothing; the other one is restored
    rule = hit & ~mask & ((good[0] | zero[0]) & (good[1] | zero[1])) & (zero[0] | zero[1])
    want = em[:, :3].astype(np.float64) + np.where(good[0][:, None], nd[:, :3], 0.0) + np.where(good[1][:, None], ns[:, :3], 0.0)
    assert_close(got[rule, :3], want[rule], np.maximum(np.abs(want[rule]).max(axis=1, keepdims=True), 1e-30), CHAIN_RTOL,
                 f"mode {mode}: zeroed lobes")
    share = mask.sum() / hit.sum()
    if coverage is not None:
        assert coverage[0] <= share <= coverage[1], share
        assert (mask | rule).sum() >= 0.99 * hit.sum()
    return share


def test_identity_chain_on_the_oracles_frame(dxrs, host, oracle, shim):
    """pack -> copy -> compose on the CPU-made inputs of the C2 crop reproduces the oracle's frame (this is where CHAIN_RTOL and
    C2_CROP_COVERAGE come from)"""
    x = chain_inputs(host, oracle, dxrs, C2_CROP, 0)
    for mode in (REBLUR, RELAX):
        y = dict(x, **x[mode])
        flat = {k: y[k].reshape(-1, y[k].shape[-1]) for k in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness",
                                                                "NoisyDiffuse", "NoisySpecular", "Emission")}
        flat["LinearDepth"] = flat["LinearDepth"][:, 0]
        pd, ps = host_pass(shim, mode, True, {k: flat[k] for k in ref_keys(True)})
        rad = host_pass(shim, mode, False, dict(LinearDepth=flat["LinearDepth"], DiffuseAlbedo=flat["DiffuseAlbedo"],
                                                SpecularAlbedo=flat["SpecularAlbedo"], DenoisedDiffuse=pd, DenoisedSpecular=ps,
                                                Radiance=flat["Emission"]))
        check_identity_chain(mode, y, rad.reshape(y["Emission"].shape), x["Frame"], C2_CROP_COVERAGE)


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import PtNrdCompositionConstants, PtNrdCompositionTextures
    lib = dxrs.load_hip().lib
    k = PtNrdCompositionConstants(RenderSize=(C.c_uint32 * 2)(64, 64), Pack=1, Denoiser=REBLUR)
    assert lib.pt_nrd_composition(None, C.byref(k), C.byref(PtNrdCompositionTextures())) == 1
    assert lib.pt_nrd_composition(None, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU

NAMES = ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "NoisyDiffuse", "NoisySpecular", "DenoisedDiffuse",
         "DenoisedSpecular", "Radiance")


def bits_equal(got, want, what=""):
    """bit-exact equality; NaN compared by mask (a NaN payload the pass computes is not part of the contract -- one it leaves alone
    is, and is checked where the pass leaves it)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ at {np.argwhere(gn != wn)[:5].tolist()}"
    g, w = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:5].tolist()}: {got[~gn][bad[:5]].tolist()} vs {want[~wn][bad[:5]].tolist()}"


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def gpu_pass(renderer, mode, pack, w, h, bufs, P=tuple(ref.HIT_DISTANCE)):
    """pt_nrd_composition on device copies of bufs -> what host_pass returns"""
    import torch
    d = {k: to_dev(v) for k, v in bufs.items() if v is not None}
    torch.cuda.synchronize()
    renderer.nrd_composition_device(mode, pack, w, h, {k: t.data_ptr() for k, t in d.items()}, P)
    renderer.synchronize()
    return (d["NoisyDiffuse"].cpu().numpy(), d["NoisySpecular"].cpu().numpy()) if pack else d["Radiance"].cpu().numpy()


def gpu_vs_host(renderer, shim, mode, pack, w, h, x, P=P_DEFAULT):
    bufs = {k: x[k] for k in ref_keys(pack)}
    if pack and mode == RELAX:
        bufs.pop("NormalRoughness")  # not read
    got = gpu_pass(renderer, mode, pack, w, h, bufs, tuple(float(v) for v in P))
    want = host_pass(shim, mode, pack, bufs, P)
    hit = np.isfinite(np.asarray(x["LinearDepth"], np.float32).ravel())
    for g, wnt, name in zip(got if pack else (got,), want if pack else (want,), ("NoisyDiffuse", "NoisySpecular") if pack else ("Radiance",)):
        g, wnt = g.reshape(-1, 4), wnt.reshape(-1, 4)
        bits_equal(g, wnt, f"mode {mode} pack {pack}: {name}")
        src = np.asarray(x[name], np.float32).reshape(-1, 4)
        assert np.array_equal(g[~hit].view(np.uint32), src[~hit].view(np.uint32)), f"{name}: a miss pixel was written"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (333, 77), (1920, 1080), (3840, 2160)])
def test_gpu_bit_exact_random_images(renderer, shim, size):
    w, h = size
    rng = np.random.default_rng(w * 7 + h)
    x = random_inputs(rng, w * h, special=True)
    for mode in (REBLUR, RELAX):
        for pack in (True, False):
            gpu_vs_host(renderer, shim, mode, pack, w, h, x)
    gpu_vs_host(renderer, shim, REBLUR, True, w, h, x, np.float32([1.0, 0.5, 4.0, -3.0]))  # a caller's own hit distance parameters


@pytest.mark.gpu
def test_gpu_pack_in_place_keeps_neighbours(renderer, shim):
    """a rect's buffers hold w * h pixels: a guard band behind them stays untouched, and the noisy buffers are rewritten in place"""
    import torch
    w, h = 333, 77
    n = w * h
    x = random_inputs(np.random.default_rng(5), n)
    d = {k: to_dev(x[k]) for k in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness")}
    guard = np.full((n + 64, 4), SENTINEL, np.float32)
    nd, ns = to_dev(guard), to_dev(guard)
    nd[:n] = to_dev(x["NoisyDiffuse"])
    ns[:n] = to_dev(x["NoisySpecular"])
    torch.cuda.synchronize()
    renderer.nrd_composition_device(REBLUR, True, w, h, dict({k: t.data_ptr() for k, t in d.items()}, NoisyDiffuse=nd.data_ptr(),
                                                              NoisySpecular=ns.data_ptr()))
    renderer.synchronize()
    want_d, want_s = host_pass(shim, REBLUR, True, {k: x[k] for k in ref_keys(True)})
    for t, want in ((nd, want_d), (ns, want_s)):
        a = t.cpu().numpy()
        bits_equal(a[:n], want)
        assert np.array_equal(a[n:].view(np.uint32), guard[n:].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c2", "c2_di", "textured"])
def test_gpu_real_chain_bit_exact(dxrs, host, renderer, shim, case):
    """the G-buffer and N7 outputs of one frame, packed and composed on the GPU, equal the host-compiled header run on the downloaded
    inputs, bit for bit"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = (1920, 1080) if case != "textured" else (480, 270)
    ts = None
    if case == "textured":
        ts, sd = host.demo_textures(seed=0, time=0.0, environment_map=True, return_scene_data=True)
    renderer.set_scene(spheres, mats, sd)
    if ts is not None:
        renderer.set_textures(ts)
    try:
        renderer.set_camera(host.camera_matrices(w, h, jitter_index=2))
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=2, bounces=8, spp=1, di=case == "c2_di"))
        for mode in (REBLUR, RELAX):
            x = renderer.nrd_chain(mode)
            flat = {k: x[k].reshape(-1, x[k].shape[-1]) for k in x}
            flat["LinearDepth"] = flat["LinearDepth"][:, 0]
            hit = np.isfinite(flat["LinearDepth"])
            assert 0.2 < hit.mean() < 1.0
            want_d, want_s = host_pass(shim, mode, True, dict((k, flat[k]) for k in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo",
                                                                                    "NormalRoughness", "NoisyDiffuse", "NoisySpecular")))
            bits_equal(flat["PackedDiffuse"], want_d, f"{case} mode {mode}: packed Diffuse")
            bits_equal(flat["PackedSpecular"], want_s, f"{case} mode {mode}: packed Specular")
            bits_equal(flat["DenoisedDiffuse"], want_d)
            want = host_pass(shim, mode, False, dict(LinearDepth=flat["LinearDepth"], DiffuseAlbedo=flat["DiffuseAlbedo"],
                                                     SpecularAlbedo=flat["SpecularAlbedo"], DenoisedDiffuse=want_d, DenoisedSpecular=want_s,
                                                     Radiance=flat["Emission"]))
            bits_equal(flat["Radiance"], want, f"{case} mode {mode}: composed radiance")
            assert (flat["Radiance"][hit, :3] != flat["Emission"][hit, :3]).any()
    finally:
        if ts is not None:
            renderer.set_textures(None)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["crop", "frame"])
def test_gpu_identity_chain_reproduces_pt_render(dxrs, host, renderer, where):
    """pack -> copy -> compose of a C2 frame (no DI) reproduces pt_render of the same frame within CHAIN_RTOL on the mask, with the
    coverage the CPU test measured on the same crop; misses unchanged, zeroed lobes where an albedo channel is 0"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 1920, 1080
    rect, frame, coverage = (C2_CROP, 0, C2_CROP_COVERAGE) if where == "crop" else ((0, 0, w, h), 5, (0.04, 0.06))
    renderer.set_scene(spheres, mats, sd)
    renderer.set_camera(host.camera_matrices(w, h, jitter_index=frame))
    renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=frame, bounces=8, spp=1))
    img, _ = renderer.render(rect=rect, want_stats=False)
    for mode in (REBLUR, RELAX):
        x = renderer.nrd_chain(mode, rect=rect)
        check_identity_chain(mode, x, x["Radiance"], img, coverage)


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """three lanes, six frames of a moving camera and animated spheres, one buffer set per lane: G-buffer -> pt_render_denoiser -> pack
    -> copy -> compose, all queued without waiting, equals the same frames run one at a time"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    sd.IsStatic = 0
    w, h = 640, 360
    frames = 6
    width = dict(dxrs.types.GBUFFER_CHANNELS)

    def frame_setup(r, f):
        moved = spheres.copy()
        moved["cy"] += np.float32(0.1 * f) * np.sin(np.arange(len(spheres), dtype=np.float32))
        r.update_spheres(moved)
        r.set_camera(host.camera_matrices(w, h, position=(0.3 * f, 0.0, -15.0 + 0.2 * f), look_at=(0.5 * f, 0.2 * f, 0.0), jitter_index=f))
        r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))

    def mode_of(f):
        return REBLUR if f % 2 == 0 else RELAX

    tstream = torch.cuda.Stream()
    r = dxrs.Renderer(device=0, stream=tstream.cuda_stream, frames_in_flight=3)
    got = []
    try:
        r.set_scene(spheres, mats, sd)
        sets = []
        for _ in range(3):
            s = {k: torch.zeros((h, w, width[k]), dtype=torch.float32, device="cuda") for k in NAMES[:4]}
            s.update({k: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for k in NAMES[4:]})
            sets.append(s)
        torch.cuda.synchronize()
        with torch.cuda.stream(tstream):
            for f in range(frames):
                frame_setup(r, f)
                s = sets[f % 3]
                r.render_gbuffer_device({k: s[k].data_ptr() for k in NAMES[:4]})
                r.render_denoiser_device(mode_of(f), s["Radiance"].data_ptr(), {"Diffuse": s["NoisyDiffuse"].data_ptr(),
                                                                               "Specular": s["NoisySpecular"].data_ptr()})
                inputs = {k: s[k].data_ptr() for k in NAMES[:4]}
                r.nrd_composition_device(mode_of(f), True, w, h, dict(inputs, NoisyDiffuse=s["NoisyDiffuse"].data_ptr(),
                                                                      NoisySpecular=s["NoisySpecular"].data_ptr()))
                s["DenoisedDiffuse"].copy_(s["NoisyDiffuse"])
                s["DenoisedSpecular"].copy_(s["NoisySpecular"])
                r.nrd_composition_device(mode_of(f), False, w, h, dict(inputs, DenoisedDiffuse=s["DenoisedDiffuse"].data_ptr(),
                                                                       DenoisedSpecular=s["DenoisedSpecular"].data_ptr(),
                                                                       Radiance=s["Radiance"].data_ptr()))
                # the set's next frame finds its noisy buffers cleared: cleared here, behind this frame's consumers (a lane waits for what
                # the caller queued after the render call n_lanes calls back, not for what it queues just before its own)
                for k in ("NoisyDiffuse", "NoisySpecular"):
                    s[k].zero_()
                if f % 3 == 2:
                    got += [{k: v.cpu().numpy().copy() for k, v in x.items()} for x in sets]
        r.synchronize()
        torch.cuda.synchronize()
    finally:
        r.close()
    alone = dxrs.Renderer(device=0)
    try:
        alone.set_scene(spheres, mats, sd)
        for f in range(frames):
            frame_setup(alone, f)
            x = alone.nrd_chain(mode_of(f))
            for k in ("LinearDepth", "DenoisedDiffuse", "DenoisedSpecular", "Radiance"):  # (written on every pixel)
                bits_equal(got[f][k], x[k], f"frame {f}: {k}")
            assert (np.isfinite(x["LinearDepth"]).mean()) > 0.2
    finally:
        alone.close()


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, renderer):
    from dxrs_amd.types import PtNrdCompositionConstants, PtNrdCompositionTextures
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    w, h = 64, 32
    n = w * h
    bufs = {k: torch.zeros(n * 4 + 8, dtype=torch.float32, device="cuda") for k in NAMES}
    p = {k: b.data_ptr() for k, b in bufs.items()}

    def call(pack=1, mode=REBLUR, size=(w, h), **over):
        k = PtNrdCompositionConstants(RenderSize=(C.c_uint32 * 2)(*size), Pack=pack, Denoiser=mode, ReBLURHitDistance=(C.c_float * 4)(*ref.HIT_DISTANCE))
        t = PtNrdCompositionTextures(**{name: C.c_void_p(over.get(name, p[name])) for name in NAMES})
        return lib.pt_nrd_composition(ctx, C.byref(k), C.byref(t))

    assert lib.pt_nrd_composition(None, None, None) == 1
    k = PtNrdCompositionConstants(RenderSize=(C.c_uint32 * 2)(w, h), Pack=1, Denoiser=REBLUR)
    assert lib.pt_nrd_composition(ctx, None, C.byref(PtNrdCompositionTextures())) == 1
    assert lib.pt_nrd_composition(ctx, C.byref(k), None) == 1
    for mode in (0, 1, 4, 99):
        assert call(mode=mode) == 1
    for size in ((0, h), (w, 0), (16385, 1), (1, 16385)):
        assert call(size=size) == 1
    # a buffer the direction needs is missing
    for name in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "NoisyDiffuse", "NoisySpecular"):
        assert call(pack=1, **{name: None}) == 1, name
    for name in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "DenoisedDiffuse", "DenoisedSpecular", "Radiance"):
        assert call(pack=0, **{name: None}) == 1, name
    # ... and what it does not use may be absent: ReLAX pack does not read NormalRoughness, pack no denoised buffer, compose no noisy one
    assert call(pack=1, mode=RELAX, NormalRoughness=None, DenoisedDiffuse=None, DenoisedSpecular=None, Radiance=None) == 0
    assert call(pack=0, NormalRoughness=None, NoisyDiffuse=None, NoisySpecular=None) == 0
    # float4 buffers must be 16-byte aligned, the others 4-byte
    for name in ("NormalRoughness", "NoisyDiffuse", "NoisySpecular"):
        assert call(pack=1, **{name: p[name] + 4}) == 1, name
    for name in ("DenoisedDiffuse", "DenoisedSpecular", "Radiance"):
        assert call(pack=0, **{name: p[name] + 8}) == 1, name
    assert call(pack=1, LinearDepth=p["LinearDepth"] + 2) == 1
    assert call(pack=1, LinearDepth=p["LinearDepth"] + 4) == 0
    # a written buffer overlapping another buffer of the call
    for name in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "DenoisedDiffuse", "DenoisedSpecular"):
        assert call(pack=0, Radiance=p[name]) == 1, name
    two = torch.zeros(2 * n * 4, dtype=torch.float32, device="cuda")  # two images back to back
    assert call(pack=0, DenoisedDiffuse=two.data_ptr(), Radiance=two.data_ptr() + 16 * (n - 1)) == 1  # (one pixel shared)
    assert call(pack=0, DenoisedDiffuse=two.data_ptr(), Radiance=two.data_ptr() + 16 * n) == 0
    assert call(pack=1, NoisySpecular=p["NoisyDiffuse"]) == 1
    assert call(pack=1, NoisyDiffuse=p["NormalRoughness"]) == 1
    assert call(pack=0, NoisyDiffuse=p["Radiance"]) == 0  # (compose does not use the noisy buffers)
    assert call() == 0  # the context still works
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """PostProcessing::NRDComposition (host/NRDComposition.hpp) from C++: the demo frame's packed buffers and composed radiance equal the
    Python path's, and a mode other than ReBLUR / ReLAX is refused"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_nrd_composition")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_nrd_composition.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 160, 90
    n = w * h
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0)
    try:
        r.set_scene(spheres, mats, sd)
        r.set_camera(host.camera(w, h, jitter=False))
        r.set_constants(dxrs.types.graphics_settings(w, h, bounces=8, spp=1))
        for mode in (REBLUR, RELAX):
            outp = str(tmp_path / f"nrd{mode}.f32")
            res = subprocess.run([exe, str(w), str(h), str(mode), outp], capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stdout + res.stderr
            assert "expected error" in res.stdout
            raw = np.fromfile(outp, dtype=np.float32).reshape(3, h, w, 4)
            x = r.nrd_chain(mode)
            hit = np.isfinite(x["LinearDepth"][..., 0])
            assert hit.any()
            bits_equal(raw[0], x["Radiance"], f"C++ mode {mode}: radiance")
            bits_equal(raw[1][hit], x["PackedDiffuse"][hit], f"C++ mode {mode}: packed Diffuse")
            bits_equal(raw[2][hit], x["PackedSpecular"][hit], f"C++ mode {mode}: packed Specular")
    finally:
        r.close()
