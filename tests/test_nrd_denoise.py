"""Row N9 -- the NRD stand-in (pt_nrd_denoise: NRD::Denoise as App::ProcessNRD drives it; DESIGN.md spec S15).
CPU: the product's header (csrc/pt_denoise.h compiled as host C++ by tests/hostshim/denoise_host.cpp) against the float64 numpy
restatement (tests/denoise_reference.py) pass by pass, and hand-derived known answers; the denoised chain on the oracle's frames
against the oracle at 256 spp -- where the quality ratios are chosen.
GPU: pt_nrd_denoise against the host-compiled header bit for bit (random images, real chains of a resting, travelling and animated
camera, 1080p, a ragged size, RESTART in a sequence); frames in flight; RenderSize changes; argument errors; the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REBLUR, RELAX = 2, 3
SENTINEL = np.uint32(0x7FC0BEEF).view(np.float32)  # a NaN with a payload: survives exactly where nothing is written
# Pass-by-pass tolerance of the header (fp32, exp2_spec) against the float64 restatement, relative to the pass's scale: each pass
# rounds a few dozen fp32 operations (~1e-6) and its edge weights are exp of arguments up to 80, whose fp32 rounding (~80 * 6e-8 =
# 5e-6 relative) and exp2_spec's error (~1e-7) pass into the weights.  Largest errors seen on these images: temporal 2.1e-5,
# variance 1.2e-6, a-trous 2.0e-7 (a-trous: outside the two pixels per check that may take the other branch).
PASS_RTOL = 3e-5
# Quality on the oracle's C2 crop (QUALITY_CROP, frames 0..15 of a resting camera, 1 spp each) against the oracle at 256 spp: RMSE of
# the composed frame over the hit pixels.  Seen on the CPU: noisy 0.1715 (frame 0); denoised 0.1232 at frame 0 (ratio 0.718) and
# 0.1188 at frame 15 (0.964 of the denoised frame 0), ReBLUR and ReLAX alike to 4 digits.  The crop's specular is mostly mirror-like
# (history cap 1, a-trous strength ~0), so frames 1..15 improve the diffuse lobe only.
QUALITY_CROP = (840, 472, 240, 136)
QUALITY_FRAMES = 16
QUALITY_RATIO_0 = 0.80   # denoised / noisy RMSE at frame 0
QUALITY_RATIO_15 = 0.99  # denoised at frame 15 / denoised at frame 0
PTRS = ("viewz", "mv", "nr", "in_d", "in_s", "out_d", "out_s", "prev_sig_d", "prev_sig_s", "prev_mom", "prev_guide", "sig_d", "sig_s", "mom",
        "guide", "hitd", "xd0", "xs0", "xd1", "xs1")


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_denoise_shim())
    lib.dn_host_pass.restype = None
    lib.dn_host_pass.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class HostDenoiser:
    """pt_nrd_denoise on the host-compiled header, with the history logic of pt_api_post.hip: the first call, and a call with another size
    or mode, restarts; two history slots alternate."""

    def __init__(self, shim):
        self.shim, self.key, self.slots, self.cur = shim, None, None, 0

    def __call__(self, mode, z, mv, nr, ind, ins, accumulation=0, max_d=0, max_s=0, iterations=0, out=None, keep=False):
        z = c32(z)
        h, w = z.shape[:2]
        restart = accumulation != 0 or self.key is None or self.key[2] != mode
        if self.key is None or self.key[:2] != (w, h):
            self.slots = [{k: np.zeros((h, w, 4), np.float32) for k in ("sig_d", "sig_s", "mom", "guide")} for _ in range(2)]
            restart = True
        self.key = (w, h, mode)
        prev, cur = self.slots[self.cur], self.slots[self.cur ^ 1]
        b = dict(viewz=z, mv=c32(mv), nr=c32(nr), in_d=c32(ind), in_s=c32(ins), hitd=np.zeros((h, w, 2), np.float32),
                 xd0=np.full((h, w, 4), np.nan, np.float32), xs0=np.full((h, w, 4), np.nan, np.float32), xd1=np.full((h, w, 4), np.nan, np.float32),
                 xs1=np.full((h, w, 4), np.nan, np.float32))
        b["out_d"], b["out_s"] = (c32(o).copy() for o in out) if out is not None else (np.full((h, w, 4), SENTINEL, np.float32) for _ in range(2))
        b.update({"prev_" + k: v for k, v in prev.items()})
        b.update(cur)
        ptrs = (C.c_void_p * len(PTRS))(*[b[k].ctypes.data for k in PTRS])
        iterations = iterations or 5
        passes = {}

        def run(p, src=0, step=0):
            prm = np.array([w, h, max_d or 30, max_s or 30, 1 if restart else 0, src, step], np.uint32)
            self.shim.dn_host_pass(p, mode, prm.ctypes.data, ptrs)

        run(0)
        if keep:
            passes["temporal"] = {k: cur[k].copy() for k in cur} | {"hitd": b["hitd"].copy()}
        run(1)
        if keep:
            passes["variance"] = (b["xd0"].copy(), b["xs0"].copy())
        for it in range(iterations):
            src = it & 1
            run(3 if it + 1 == iterations else 2, src, 1 << it)
            if keep:
                dst = ("out_d", "out_s") if it + 1 == iterations else (f"xd{1 - src}", f"xs{1 - src}")
                passes[f"atrous{it}"] = (b[dst[0]].copy(), b[dst[1]].copy())
        self.cur ^= 1
        self.restarted = restart
        if keep:
            passes["prev"] = None if restart else {k: v.copy() for k, v in prev.items()}
            return b["out_d"], b["out_s"], passes
        return b["out_d"], b["out_s"]

    def history(self):
        """the slot the last call wrote"""
        return self.slots[self.cur]


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_frame(rng, w, h, mode, miss=0.1):
    """plausible guides and packed lobes: a tilted plane with a raised block and misses, normals near the view axis, motion of up to
    1.5 pixels (a few far off), lobes over 4 decades with zero hit distances and rare fireflies"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    z = (5.0 + 0.02 * xs + 0.01 * ys).astype(np.float32)
    z[h // 3:h // 2, w // 4:w // 2] -= 2.0
    z[rng.random((h, w)) < miss] = np.inf
    nr = np.zeros((h, w, 4), np.float32)
    nr[..., :3] = unit(np.float32([0, 0, -1]) + 0.15 * rng.standard_normal((h, w, 3)).astype(np.float32))
    nr[..., 3] = rng.uniform(0.0, 1.0, (h, w))
    nr[rng.random((h, w)) < 0.1, 3] = 0.0
    mv = rng.uniform(-1.5, 1.5, (h, w, 3)).astype(np.float32)
    mv[..., 2] *= 0.05
    mv[rng.random((h, w)) < 0.03, :2] = 40.0
    lobes = []
    for _ in range(2):
        rgb = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), (h, w, 3))).astype(np.float32)
        rgb[rng.random((h, w)) < 0.02] *= 100.0
        a = rng.uniform(0.05, 30.0, (h, w)).astype(np.float32)
        a[rng.random((h, w)) < 0.2] = 0.0
        if mode == REBLUR:
            rgb = ref.to_ycocg(rgb.astype(np.float64)).astype(np.float32)
            a = np.clip(a / 30.0, 0.0, 1.0).astype(np.float32)
        lobes.append(np.concatenate([rgb, a[..., None]], axis=-1).astype(np.float32))
    return z, mv, nr, lobes[0], lobes[1]


def assert_close(got, want, scale, rtol, what, allow=0):
    """got (float32) against want (float64) on the pixels where want is not NaN: |got - want| <= rtol * scale; `allow` pixels may differ
    (a branch of the spec decided the other way in fp32)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    m = ~np.isnan(want)
    with np.errstate(invalid="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want))  # (equal infinities)
    bad = m & ~(err <= rtol * scale)
    n_bad = int(bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=-1).sum()) if bad.ndim >= 2 else int(bad.sum())
    worst = float(np.nanmax(np.where(m, err / scale, 0.0)))
    assert n_bad <= allow, f"{what}: {n_bad} pixels off (worst relative error {worst:.3g}), first {np.argwhere(bad)[:4].tolist()}"
    return worst


def neighbourhood_max(a, r):
    """max of a over the (2r + 1)^2 window of each pixel, NaN ignored"""
    out = np.where(np.isnan(a), -np.inf, a)
    res = out.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            res = np.maximum(res, ref.shift(out, dx, dy, -np.inf))
    return res


# ------------------------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("mode", [REBLUR, RELAX])
@pytest.mark.parametrize("seed", [0, 1])
def test_header_passes_match_numpy_restatement(shim, mode, seed):
    """two calls (a restart, then one with history) on a random 41 x 29 image; each pass of the header against the restatement fed the
    header's own fp32 results of the pass before"""
    rng = np.random.default_rng(seed)
    w, h = 41, 29
    d = HostDenoiser(shim)
    for call in range(2):
        z, mv, nr, ind, ins = random_frame(rng, w, h, mode)
        if call == 1:  # the same surface a little later: most of the history survives the depth and normal tests
            z = np.where(np.isfinite(z0), z0, z).astype(np.float32)
            nr = nr0
        out_d, out_s, p = d(mode, z, mv, nr, ind, ins, max_s=20, keep=True)
        z0, nr0 = z, nr
        hit = np.isfinite(z)
        t = ref.temporal(mode, z, mv, nr, ind, ins, p["prev"], 30, 20)
        got = p["temporal"]
        for k in ("sig_d", "sig_s", "mom", "guide"):
            scale = np.maximum(np.abs(t[k]).max(axis=-1, keepdims=True), 1e-3)
            assert_close(got[k], t[k], scale, PASS_RTOL, f"call {call}: temporal {k}", allow=2)
        assert_close(got["hitd"][hit], t["hitd"][hit], np.maximum(np.abs(t["hitd"][hit]), 1e-3), PASS_RTOL, f"call {call}: hit distance")
        assert (got["sig_d"][..., 3][hit] == 1).all() if call == 0 else (got["sig_d"][..., 3][hit] > 1.5).mean() > 0.5
        vd, vs = ref.variance(z, nr, got["sig_d"], got["sig_s"], got["mom"])
        for g, want, what in ((p["variance"][0], vd, "diffuse"), (p["variance"][1], vs, "specular")):
            scale = np.maximum(np.abs(want[..., :3]).max(axis=-1, keepdims=True), 1e-3)
            assert_close(g[..., :3], want[..., :3], scale, PASS_RTOL, f"call {call}: variance pass rgb {what}")
            vscale = np.maximum(neighbourhood_max(np.abs(got["mom"]).max(axis=-1), 3), 1e-3)  # the m2 it sums bounds the cancellation
            assert_close(g[..., 3], want[..., 3], vscale, PASS_RTOL, f"call {call}: variance {what}", allow=2)
        xd, xs = p["variance"]
        for it in range(5):
            want_d, want_s = ref.atrous(mode, z, nr, xd, xs, 1 << it, it == 4, got["hitd"])
            gd, gs = p[f"atrous{it}"]
            for g, want, src in ((gd, want_d, xd), (gs, want_s, xs)):
                scale = np.nanmax(np.abs(src[..., :3])) * np.ones(g.shape[:2] + (1,))
                assert_close(g[..., :3], want[..., :3], scale, PASS_RTOL, f"call {call}: a-trous step {it} rgb", allow=2)
                if it < 4:
                    vscale = np.nanmax(np.abs(src[..., 3])) * np.ones(g.shape[:2])
                    assert_close(g[..., 3], want[..., 3], vscale, PASS_RTOL, f"call {call}: a-trous step {it} variance", allow=2)
                else:
                    assert np.array_equal(g[..., 3][hit], got["hitd"][..., 0 if g is gd else 1][hit])
            xd, xs = gd, gs
        for o in (out_d, out_s):  # misses are never written
            assert np.array_equal(o[~hit].view(np.uint32), np.full(o[~hit].shape, SENTINEL).view(np.uint32))
            assert np.isfinite(o[hit]).all()


def plane(w, h, z=4.0, rough=0.3):
    nr = np.zeros((h, w, 4), np.float32)
    nr[..., 2] = -1.0
    nr[..., 3] = rough
    return np.full((h, w), z, np.float32), np.zeros((h, w, 3), np.float32), nr


def lobe(w, h, rgb, a, mode):
    c = np.float32(rgb)
    if mode == REBLUR:
        c = ref.to_ycocg(c.astype(np.float64)).astype(np.float32)
    x = np.empty((h, w, 4), np.float32)
    x[..., :3] = c
    x[..., 3] = a
    return x


@pytest.mark.parametrize("mode", [REBLUR, RELAX])
def test_constant_signal_on_a_plane_is_unchanged(shim, mode):
    w, h = 40, 24
    z, mv, nr = plane(w, h)
    d = HostDenoiser(shim)
    ind, ins = lobe(w, h, (0.5, 0.25, 2.0), 3.0 if mode == RELAX else 0.25, mode), lobe(w, h, (1.5, 0.75, 0.125), 0.5, mode)
    for f in range(4):
        od, os_ = d(mode, z, mv, nr, ind, ins)
        for o, i in ((od, ind), (os_, ins)):
            ulp = np.spacing(np.abs(i)).astype(np.float32)
            assert (np.abs(o - i) <= 2 * ulp).all(), (f, np.abs(o - i).max())


@pytest.mark.parametrize("mode", [REBLUR, RELAX])
def test_history_length_at_rest_and_specular_cap(shim, mode):
    w, h = 24, 16
    z, mv, nr = plane(w, h)
    nr[:, : w // 4, 3] = 0.0    # mirror: cap max(1, round(12 * 0)) = 1
    nr[:, w // 4: w // 2, 3] = 0.1   # round(12 * 0.2) = round(2.4) = 2
    nr[:, w // 2:, 3] = 0.6     # saturate(1.2) = 1: 12
    rng = np.random.default_rng(3)
    d = HostDenoiser(shim)
    for k in range(1, 16):
        ind, ins = (lobe(w, h, rng.uniform(0.1, 1.0, 3), 1.0 if mode == RELAX else 0.2, mode) for _ in range(2))
        d(mode, z, mv, nr, ind, ins, max_d=10, max_s=12)
        hs = d.history()
        assert (hs["sig_d"][..., 3] == min(k, 10)).all(), k
        assert (hs["sig_s"][:, : w // 4, 3] == 1).all()
        assert (hs["sig_s"][:, w // 4: w // 2, 3] == min(k, 2)).all()
        assert (hs["sig_s"][:, w // 2:, 3] == min(k, 12)).all()


def test_depth_step_restarts_exactly_the_disoccluded_pixels(shim):
    w, h = 32, 20
    z, mv, nr = plane(w, h, z=6.0)
    ind = ins = lobe(w, h, (1, 1, 1), 1.0, RELAX)
    d = HostDenoiser(shim)
    for _ in range(3):
        d(RELAX, z, mv, nr, ind, ins)
    z2 = z.copy()
    z2[5:12, 8:20] = 3.0  # an occluder moves in; the motion vector says the background is where it was
    z2[0, 0] = 6.0 * 1.04  # |6 - z| within 5 % of z: kept
    z2[0, 1] = 6.0 * 1.06  # beyond: restarted
    d(RELAX, z2, mv, nr, ind, ins)
    n = d.history()["sig_d"][..., 3]
    restarted = np.zeros((h, w), bool)
    restarted[5:12, 8:20] = True
    restarted[0, 1] = True
    assert (n[restarted] == 1).all() and (n[~restarted] == 4).all()


@pytest.mark.parametrize("mode", [REBLUR, RELAX])
def test_half_planes_do_not_bleed(shim, mode):
    w, h = 48, 24
    z, mv, nr = plane(w, h)
    z[:, : w // 2] = 1.0
    z[:, w // 2:] = 10.0
    ind = np.concatenate([lobe(w // 2, h, (0.25, 0.5, 1.0), 0.5, mode), lobe(w // 2, h, (4.0, 2.0, 1.0), 0.5, mode)], axis=1)
    ins = ind[:, ::-1].copy()
    d = HostDenoiser(shim)
    for _ in range(3):
        od, os_ = d(mode, z, mv, nr, ind, ins)
        for o, i in ((od, ind), (os_, ins)):
            assert (np.abs(o - i) <= 2 * np.spacing(np.abs(i))).all(), np.abs(o - i).max()


@pytest.mark.parametrize("accumulation", [1, 2])
def test_restart_modes_reset_history(shim, accumulation):
    w, h = 16, 12
    z, mv, nr = plane(w, h)
    ind = ins = lobe(w, h, (1, 2, 3), 1.0, RELAX)
    d = HostDenoiser(shim)
    for _ in range(5):
        d(RELAX, z, mv, nr, ind, ins)
    assert (d.history()["sig_d"][..., 3] == 5).all()
    d(RELAX, z, mv, nr, ind, ins, accumulation=accumulation)
    assert d.restarted and (d.history()["sig_d"][..., 3] == 1).all()
    d(RELAX, z, mv, nr, ind, ins)
    assert (d.history()["sig_d"][..., 3] == 2).all()
    d(REBLUR, z, mv, nr, ind, ins)  # a mode change restarts too
    assert d.restarted and (d.history()["sig_d"][..., 3] == 1).all()


def test_misses_keep_their_sentinel_and_zero_hit_distance_is_reconstructed(shim):
    w, h = 12, 10
    z, mv, nr = plane(w, h, z=5.0)
    z[0, :] = np.inf
    z[4, 4] = np.nan
    ind = lobe(w, h, (1, 1, 1), 2.0, RELAX)
    ind[6, 6, 3] = 0.0         # neighbours all 2 -> 2
    ind[8, 2:5, 3] = [4.0, 0.0, 7.0]
    ind[7:10, 3, 3] = 0.0      # (8, 3): nonzero neighbours at depth 5: 4 (left), 7 (right), 2 at (7, 2), (7, 4), (9, 2) -> mean
    z[9, 4] = 9.0              # ... but (9, 4) fails the depth test
    ins = lobe(w, h, (1, 1, 1), 0.0, RELAX)  # no specular hit distance anywhere: stays 0
    od, os_ = HostDenoiser(shim)(RELAX, z, mv, nr, ind, ins)
    miss = ~np.isfinite(z)
    for o in (od, os_):
        assert np.array_equal(o[miss].view(np.uint32), np.full(o[miss].shape, SENTINEL).view(np.uint32))
    assert od[6, 6, 3] == 2.0
    assert od[8, 3, 3] == np.float32((2.0 + 2.0 + 4.0 + 7.0 + 2.0) / 5.0)
    assert (os_[~miss, 3] == 0).all()


def chain_frames(host, oracle, dxrs, rect, frames):
    """CPU-made inputs of the C2 chain (as test_nrd_composition.chain_inputs makes them: the oracle's frame, its N7 outputs and the
    G-buffer header's channels, MotionVector included) for frames of a resting camera without jitter -> list of dicts"""
    import __graft_entry__ as g
    from test_denoiser_outputs import expected, sample0
    from test_gbuffer import channel, grid, host_pixels, oracle_hits

    gb = C.CDLL(g.build_gbuffer_shim())
    vp, u32 = C.c_void_p, C.c_uint32
    gb.gb_pixels.restype = None
    gb.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    W, H = 1920, 1080
    rw, rh = rect[2], rect[3]
    cam = host.camera_matrices(W, H, jitter=False)
    px, py = grid(*rect)
    t, ids = oracle_hits(oracle, cam, W, H, spheres, px, py)
    vals, _ = host_pixels(gb, cam, W, H, spheres, mats, sd, px, py, t, ids)
    guides = {name: np.ascontiguousarray(channel(vals, name)).astype(np.float32).reshape(rh, rw, -1)
              for name in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "Radiance", "MotionVector")}
    out = []
    for f in frames:
        gs = dxrs.types.graphics_settings(W, H, bounces=8, spp=1, frame_index=f)
        res, _ = oracle.render(spheres, mats, sd, cam, gs, rect=rect, threads=8)
        hit, diffuse, hd = sample0(oracle, spheres, mats, sd, cam, gs, rect)
        assert np.array_equal(np.isfinite(guides["LinearDepth"][..., 0]), hit)
        x = dict(guides, Frame=res)
        for mode in (REBLUR, RELAX):
            e = expected(res, guides["Radiance"], hit, diffuse, hd, mode)
            x[mode] = dict(Emission=e["out"], NoisyDiffuse=np.where(hit[..., None], e["Diffuse"], 0).astype(np.float32),
                           NoisySpecular=np.where(hit[..., None], e["Specular"], 0).astype(np.float32))
        out.append(x)
    return out


def rmse(a, b, m):
    return float(np.sqrt(((a[m][:, :3].astype(np.float64) - b[m][:, :3]) ** 2).mean()))


def test_quality_on_the_oracles_frames(dxrs, host, oracle, shim):
    """16 resting frames of the C2 crop through pack -> denoise -> compose (host-compiled headers): the composed frame is closer to
    the oracle's 256-spp frame than the noisy one at frame 0, and closer still at frame 15 (where QUALITY_RATIO_* come from)"""
    import __graft_entry__ as g
    from test_nrd_composition import host_pass
    nrd = C.CDLL(g.build_nrd_shim())
    nrd.nrd_host.restype = None
    nrd.nrd_host.argtypes = [C.c_uint32, C.c_int, C.c_uint32] + [C.c_void_p] * 10
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    W, H = 1920, 1080
    gs = dxrs.types.graphics_settings(W, H, bounces=8, spp=256, frame_index=1000)  # (its own random numbers)
    truth, _ = oracle.render(spheres, mats, sd, host.camera_matrices(W, H, jitter=False), gs, rect=QUALITY_CROP, threads=8)
    frames = chain_frames(host, oracle, dxrs, QUALITY_CROP, range(QUALITY_FRAMES))
    hit = np.isfinite(frames[0]["LinearDepth"][..., 0])
    assert 0.3 < hit.mean() < 1.0
    for mode in (REBLUR, RELAX):
        d = HostDenoiser(shim)
        errs = []
        for f, x in enumerate(frames):
            y = dict(x, **x[mode])
            flat = lambda k: y[k].reshape(-1, y[k].shape[-1])  # noqa: E731
            z = y["LinearDepth"][..., 0]
            pd, ps = host_pass(nrd, mode, True, dict(LinearDepth=z.ravel(), DiffuseAlbedo=flat("DiffuseAlbedo"), SpecularAlbedo=flat("SpecularAlbedo"),
                                                     NormalRoughness=flat("NormalRoughness"), NoisyDiffuse=flat("NoisyDiffuse"),
                                                     NoisySpecular=flat("NoisySpecular")))
            shape = y["NoisyDiffuse"].shape
            od, os_ = d(mode, z, y["MotionVector"], y["NormalRoughness"], pd.reshape(shape), ps.reshape(shape), out=(pd.reshape(shape), ps.reshape(shape)))
            base = dict(LinearDepth=z.ravel(), DiffuseAlbedo=flat("DiffuseAlbedo"), SpecularAlbedo=flat("SpecularAlbedo"), Radiance=flat("Emission"))
            rad = host_pass(nrd, mode, False, dict(base, DenoisedDiffuse=od.reshape(-1, 4), DenoisedSpecular=os_.reshape(-1, 4)))
            m = np.isfinite(z).ravel()
            errs.append(rmse(rad.reshape(-1, 4), truth.reshape(-1, 4), m))
            if f == 0:
                noisy = host_pass(nrd, mode, False, dict(base, DenoisedDiffuse=pd, DenoisedSpecular=ps))
                e_noisy = rmse(noisy.reshape(-1, 4), truth.reshape(-1, 4), m)
                assert e_noisy == pytest.approx(rmse(y["Frame"].reshape(-1, 4), truth.reshape(-1, 4), m), rel=0.05)
        print(f"mode {mode}: noisy {e_noisy:.4f} denoised frame 0 {errs[0]:.4f} frame 15 {errs[-1]:.4f}")
        assert errs[0] < QUALITY_RATIO_0 * e_noisy, (e_noisy, errs)
        assert errs[-1] < QUALITY_RATIO_15 * errs[0], (e_noisy, errs)


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import PtNrdDenoiseSettings, PtNrdDenoiseTextures
    lib = dxrs.load_hip().lib
    s = PtNrdDenoiseSettings(RenderSize=(C.c_uint32 * 2)(64, 64), Denoiser=RELAX)
    assert C.sizeof(PtNrdDenoiseSettings) == 32 and C.sizeof(PtNrdDenoiseTextures) == 64
    assert lib.pt_nrd_denoise(None, C.byref(s), C.byref(PtNrdDenoiseTextures())) == 1
    assert lib.pt_nrd_denoise(None, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU

TEX = ("ViewZ", "MotionVector", "NormalRoughness", "InDiffuse", "InSpecular")


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


class GpuDenoiser:
    """pt_nrd_denoise on device copies; outputs start as the sentinel"""

    def __init__(self, renderer):
        self.r = renderer

    def __call__(self, mode, z, mv, nr, ind, ins, accumulation=0, max_d=0, max_s=0, iterations=0):
        import torch
        h, w = np.asarray(z).shape[:2]
        d = {k: torch.from_numpy(c32(v)).cuda() for k, v in zip(TEX, (z, mv, nr, ind, ins))}
        out = [torch.from_numpy(np.full((h, w, 4), SENTINEL, np.float32)).cuda() for _ in range(2)]
        torch.cuda.synchronize()
        self.r.nrd_denoise_device(mode, w, h, dict({k: t.data_ptr() for k, t in d.items()}, OutDiffuse=out[0].data_ptr(), OutSpecular=out[1].data_ptr()),
                                  accumulation_mode=accumulation, max_diffuse_frames=max_d, max_specular_frames=max_s, atrous_iterations=iterations)
        self.r.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()


def compare_sequence(renderer, shim, frames, what, **kw):
    """the frames (mode, z, mv, nr, ind, ins, accumulation) through the GPU and the host header -> bit for bit, misses untouched"""
    gpu, host = GpuDenoiser(renderer), HostDenoiser(shim)
    for f, (mode, z, mv, nr, ind, ins, acc) in enumerate(frames):
        acc = 2 if f == 0 else acc  # (the shared context carries other tests' history)
        gd, gs = gpu(mode, z, mv, nr, ind, ins, accumulation=acc, **kw)
        hd, hs = host(mode, z, mv, nr, ind, ins, accumulation=acc, **kw)
        bits_equal(gd, hd, f"{what} frame {f}: OutDiffuse")
        bits_equal(gs, hs, f"{what} frame {f}: OutSpecular")
        miss = ~np.isfinite(np.asarray(z))
        assert np.array_equal(gd[miss].view(np.uint32), np.full(gd[miss].shape, SENTINEL).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (41, 29), (333, 197), (1920, 1080)])
@pytest.mark.parametrize("mode", [REBLUR, RELAX])
def test_gpu_bit_exact_random_images(renderer, shim, size, mode):
    w, h = size
    rng = np.random.default_rng(w + 3 * h + mode)
    frames = []
    z0 = nr0 = None
    for f in range(3):
        z, mv, nr, ind, ins = random_frame(rng, w, h, mode)
        if f:
            z, nr = np.where(np.isfinite(z0), z0, z).astype(np.float32), nr0
        z0, nr0 = z, nr
        frames.append((mode, z, mv, nr, ind, ins, 0))
    compare_sequence(renderer, shim, frames, f"{w}x{h}", max_s=20, iterations=(3 if w > 1000 else 0))


@pytest.mark.gpu
def test_gpu_restart_in_a_sequence_and_eight_iterations(renderer, shim):
    w, h = 97, 61
    rng = np.random.default_rng(7)
    z, mv, nr, ind, ins = random_frame(rng, w, h, RELAX)
    mv[:] = 0.0
    frames = [(RELAX, z, mv, nr, *random_frame(rng, w, h, RELAX)[3:], acc) for acc in (0, 0, 0, 1, 0, 2, 0)]
    compare_sequence(renderer, shim, frames, "restart", iterations=8, max_d=4)


def real_chain(dxrs, host, renderer, shim, kind, mode, n_frames=8, w=480, h=270):
    """n_frames of the C2 scene through nrd_chain with the GPU denoiser; each frame's packed buffers and guides through the host header
    in the same order -> bit for bit"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    if kind == "animated":
        sd.IsStatic = 0
    renderer.set_scene(spheres, mats, sd)
    hd = HostDenoiser(shim)
    den = renderer.nrd_denoiser(mode, rect=(0, 0, w, h))
    prev, prev_cam = spheres.copy(), None
    for f in range(n_frames):
        moved = spheres.copy()
        if kind == "animated":
            moved["cy"] += np.float32(0.05 * f) * np.sin(np.arange(len(spheres), dtype=np.float32))
            renderer.update_spheres(moved)
            den.previous_pose = (prev, None)
        pos = (0.0, 0.0, -15.0) if kind != "travelling" else (0.15 * f, 0.05 * f, -15.0 + 0.1 * f)
        cam = host.camera_matrices(w, h, position=pos, look_at=(0.0, 0.0, 0.0), jitter_index=f, previous=prev_cam)
        renderer.set_camera(cam)
        prev_cam = cam
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
        x = renderer.nrd_chain(mode, rect=(0, 0, w, h), denoise=den)
        z = x["LinearDepth"][..., 0]
        want_d, want_s = hd(mode, z, x["MotionVector"], x["NormalRoughness"], x["PackedDiffuse"], x["PackedSpecular"],
                            out=(x["PackedDiffuse"], x["PackedSpecular"]))
        bits_equal(x["DenoisedDiffuse"], want_d, f"{kind} mode {mode} frame {f}: OutDiffuse")
        bits_equal(x["DenoisedSpecular"], want_s, f"{kind} mode {mode} frame {f}: OutSpecular")
        if kind != "resting":
            assert np.abs(x["MotionVector"][np.isfinite(z)][:, :2]).max() > 0.1 or f == 0
        prev = moved
    assert hd.history()["sig_d"][..., 3].max() >= min(n_frames, 2)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["resting", "travelling", "animated"])
@pytest.mark.parametrize("mode", [REBLUR, RELAX])
def test_gpu_real_chain_bit_exact(dxrs, host, renderer, shim, kind, mode):
    real_chain(dxrs, host, renderer, shim, kind, mode)


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """three lanes and six frames of a travelling camera, G-buffer -> pt_render_denoiser -> pack -> denoise -> compose all queued
    without waiting, equal the same frames run one at a time on a one-lane context"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 320, 180
    frames = 6
    width = dict(dxrs.types.GBUFFER_CHANNELS)
    names = ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "MotionVector")

    def frame_setup(r, f):
        r.set_camera(host.camera_matrices(w, h, position=(0.2 * f, 0.0, -15.0 + 0.1 * f), look_at=(0.0, 0.0, 0.0), jitter_index=f))
        r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))

    def run(r, lanes):
        got = []
        sets = []
        for _ in range(3):  # (three buffer sets in both runs: a G-buffer channel a pixel does not write keeps the same old value)
            s = {k: torch.zeros((h, w, width[k]), dtype=torch.float32, device="cuda") for k in names}
            s.update({k: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for k in ("Noisy0", "Noisy1", "Out0", "Out1", "Radiance")})
            sets.append(s)
        torch.cuda.synchronize()
        r.set_scene(spheres, mats, sd)
        for f in range(frames):
            frame_setup(r, f)
            s = sets[f % 3]
            r.render_gbuffer_device({k: s[k].data_ptr() for k in names})
            r.render_denoiser_device(RELAX, s["Radiance"].data_ptr(), {"Diffuse": s["Noisy0"].data_ptr(), "Specular": s["Noisy1"].data_ptr()})
            inputs = {k: s[k].data_ptr() for k in names[:4]}
            r.nrd_composition_device(RELAX, True, w, h, dict(inputs, NoisyDiffuse=s["Noisy0"].data_ptr(), NoisySpecular=s["Noisy1"].data_ptr()))
            r.nrd_denoise_device(RELAX, w, h, dict(ViewZ=s["LinearDepth"].data_ptr(), MotionVector=s["MotionVector"].data_ptr(),
                                                   NormalRoughness=s["NormalRoughness"].data_ptr(), InDiffuse=s["Noisy0"].data_ptr(),
                                                   InSpecular=s["Noisy1"].data_ptr(), OutDiffuse=s["Out0"].data_ptr(), OutSpecular=s["Out1"].data_ptr()),
                                 accumulation_mode=2 if f == 0 else 0)
            r.nrd_composition_device(RELAX, False, w, h, dict(inputs, DenoisedDiffuse=s["Out0"].data_ptr(), DenoisedSpecular=s["Out1"].data_ptr(),
                                                              Radiance=s["Radiance"].data_ptr()))
            if lanes == 1 or f % 3 == 2:
                r.synchronize()
                got += [{k: v.cpu().numpy().copy() for k, v in x.items()} for x in (sets if lanes > 1 else [s])]
            for k in ("Noisy0", "Noisy1"):  # the set's next frame finds its noisy buffers cleared
                s[k].zero_()
            if lanes == 1:
                torch.cuda.synchronize()  # (cleared on torch's stream, which the one-lane context's stream knows nothing of)
        r.synchronize()
        torch.cuda.synchronize()
        return got

    tstream = torch.cuda.Stream()
    r3 = dxrs.Renderer(device=0, stream=tstream.cuda_stream, frames_in_flight=3)
    try:
        with torch.cuda.stream(tstream):
            many = run(r3, 3)
    finally:
        r3.close()
    r1 = dxrs.Renderer(device=0)
    try:
        one = run(r1, 1)
    finally:
        r1.close()
    assert len(many) == len(one) == frames
    for f in range(frames):
        for k in names + ("Out0", "Out1", "Radiance"):  # (in the order the chain makes them; the noisy buffers are cleared by now)
            bits_equal(many[f][k], one[f][k], f"frame {f}: {k}")
    assert (one[-1]["Out0"] != one[-1]["Noisy0"]).any()


@pytest.mark.gpu
def test_gpu_render_size_change_restarts(renderer, shim):
    rng = np.random.default_rng(11)
    gpu = GpuDenoiser(renderer)
    for (w, h) in ((40, 30), (40, 30), (30, 40), (30, 40)):
        z, mv, nr, ind, ins = random_frame(rng, w, h, RELAX, miss=0.0)
        mv[:] = 0.0
        gpu(RELAX, z, mv, nr, ind, ins)
    # the same two frames on a fresh host mirror (the size change restarted the history)
    rng = np.random.default_rng(11)
    host = HostDenoiser(shim)
    seq = [random_frame(rng, w, h, RELAX, miss=0.0) for (w, h) in ((40, 30), (40, 30), (30, 40), (30, 40))]
    for f, (z, mv, nr, ind, ins) in enumerate(seq):
        mv[:] = 0.0
        want = host(RELAX, z, mv, nr, ind, ins)
        assert host.restarted == (f in (0, 2))
    z, mv, nr, ind, ins = seq[-1]
    # one more frame of the same size: the GPU continues its (restarted) history exactly as the mirror does
    bits_equal(gpu(RELAX, z, mv, nr, ind, ins)[0], host(RELAX, z, mv, nr, ind, ins)[0], "after the size change")
    assert want is not None


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, renderer):
    from dxrs_amd.types import NRD_DENOISE_TEXTURES, PtNrdDenoiseSettings, PtNrdDenoiseTextures
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    w, h = 64, 32
    n = w * h
    bufs = {k: torch.zeros(n * 4 + 8, dtype=torch.float32, device="cuda") for k in NRD_DENOISE_TEXTURES}
    p = {k: b.data_ptr() for k, b in bufs.items()}

    def call(mode=RELAX, size=(w, h), acc=2, iters=0, **over):
        s = PtNrdDenoiseSettings(RenderSize=(C.c_uint32 * 2)(*size), Denoiser=mode, AccumulationMode=acc, AtrousIterations=iters)
        t = PtNrdDenoiseTextures(**{name: C.c_void_p(over.get(name, p[name])) for name in NRD_DENOISE_TEXTURES})
        return lib.pt_nrd_denoise(ctx, C.byref(s), C.byref(t))

    assert lib.pt_nrd_denoise(None, None, None) == 1
    s = PtNrdDenoiseSettings(RenderSize=(C.c_uint32 * 2)(w, h), Denoiser=RELAX)
    assert lib.pt_nrd_denoise(ctx, None, C.byref(PtNrdDenoiseTextures())) == 1
    assert lib.pt_nrd_denoise(ctx, C.byref(s), None) == 1
    for mode in (0, 1, 4, 99):
        assert call(mode=mode) == 1
    assert call(acc=3) == 1 and call(acc=99) == 1
    for size in ((0, h), (w, 0), (16385, 1), (1, 16385)):
        assert call(size=size) == 1
    assert call(iters=9) == 1 and call(iters=8) == 0
    for name in NRD_DENOISE_TEXTURES:
        if name != "BaseColorMetalness":
            assert call(**{name: None}) == 1, name
    assert call(BaseColorMetalness=None) == 0
    for name in ("NormalRoughness", "BaseColorMetalness", "InDiffuse", "InSpecular", "OutDiffuse", "OutSpecular"):
        assert call(**{name: p[name] + 8}) == 1, name
    for name in ("ViewZ", "MotionVector"):
        assert call(**{name: p[name] + 2}) == 1, name
        assert call(**{name: p[name] + 4}) == 0, name
    for name in ("ViewZ", "MotionVector", "NormalRoughness", "BaseColorMetalness", "InDiffuse", "InSpecular", "OutSpecular"):
        assert call(OutDiffuse=p[name]) == 1, name
    two = torch.zeros(2 * n * 4, dtype=torch.float32, device="cuda")
    assert call(InDiffuse=two.data_ptr(), OutSpecular=two.data_ptr() + 16 * (n - 1)) == 1
    assert call(InDiffuse=two.data_ptr(), OutSpecular=two.data_ptr() + 16 * n) == 0
    assert call(InDiffuse=p["InSpecular"]) == 0  # two inputs may share a buffer
    assert call() == 0
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """dxrs::NRD (host/NRD.hpp) from C++, against pt_api.h alone: three frames of the demo scene through pack, NRD::Denoise and
    compose equal the Python chain's, and a mode other than ReBLUR / ReLAX is refused"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_nrd_denoise")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_nrd_denoise.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h, frames = 160, 90, 3
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    for mode in (REBLUR, RELAX):
        outp = str(tmp_path / f"dn{mode}.f32")
        res = subprocess.run([exe, str(w), str(h), str(mode), str(frames), outp], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        assert "expected error" in res.stdout
        raw = np.fromfile(outp, dtype=np.float32).reshape(frames, h, w, 4)
        r = dxrs.Renderer(device=0)
        try:
            r.set_scene(spheres, mats, sd)
            for f in range(frames):
                r.set_camera(host.camera(w, h, jitter=False))
                r.set_constants(dxrs.types.graphics_settings(w, h, bounces=8, spp=1, frame_index=f))
                if f == 0:
                    den = r.nrd_denoiser(mode)
                x = r.nrd_chain(mode, denoise=den)
                bits_equal(raw[f], x["Radiance"], f"C++ mode {mode} frame {f}: radiance")
        finally:
            r.close()
