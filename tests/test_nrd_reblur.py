"""Row N30 -- the ReBLUR stand-in (pt_nrd_reblur; DESIGN.md spec S32).
CPU: the product's header (csrc/pt_reblur.h compiled as host C++ by tests/hostshim/reblur_host.cpp) against the float64 numpy
restatement (tests/reblur_reference.py) pass by pass; exact properties, the radius' and the history's behaviour, responsiveness, motion;
the denoised chain on the oracle's frames against the oracle at 256 spp and against S15's filter; a stand-alone sanitizer program.
GPU: pt_nrd_reblur against the host-compiled header bit for bit (random sequences, real chains), alternation with pt_nrd_denoise,
RenderSize changes, frames in flight, argument errors, the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as dref
import reblur_reference as ref
from test_nrd_denoise import QUALITY_CROP, QUALITY_FRAMES, SENTINEL, HostDenoiser, bits_equal, c32, chain_frames, lobe, plane, random_frame, rmse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REBLUR = 2
# Pass-by-pass tolerance of the header (fp32, exp2_spec) against the float64 restatement, relative to the pass's scale, derived as
# test_nrd_denoise.PASS_RTOL is: pass (a) rounds a few dozen fp32 operations per channel (~1e-6) and forms its bilinear weights from
# fx = x + MV.x, which rounds at the image's width (41: 4e-6, times the largest history value of the footprint over the result, a few);
# pass (b) sums up to 25 weighted taps, and its two-moment sigma cancels no worse than the centre tap allows (var >= mu^2 / 10: ~1e-6);
# passes (c) and (d) sum 9 taps whose weights are exp of arguments up to 80 (their fp32 rounding, 80 * 6e-8 = 5e-6 relative, and
# exp2_spec's ~1e-7 pass into the weights).  Largest errors seen on these images (seeds 0 and 1, three calls): temporal 1.84e-5,
# history fix and clamp 3.1e-6, blur 4.5e-7, post-blur 4.4e-7; largest share of hit pixels left out in a check 0.25 %.
PASS_RTOL = 3e-5
FRAGILE_MAX = 0.005  # the share of hit pixels a check may leave out (a condition of the issue, not a measurement)
# Quality on the oracle's C2 crop (QUALITY_CROP, frames 0..15 of a resting camera, 1 spp each) against the oracle at 256 spp: RMSE of
# the composed frame over the hit pixels.  Seen on the CPU: noisy 0.1715 (frame 0); pt_nrd_reblur 0.1203 at frame 0 (ratio 0.701) and
# 0.0783 at frame 15 (0.651 of frame 0; 0.0972 at frame 1, 0.0838 at frame 5); S15's filter in ReBLUR mode (HostDenoiser, the parent's
# pt_nrd_denoise) 0.1232 at frame 0 and 0.1188 at frame 15.  The ratios asserted are the measured ones with a 10 % margin.
QUALITY_RATIO_0 = 0.771   # denoised / noisy RMSE at frame 0
QUALITY_RATIO_15 = 0.716  # denoised at frame 15 / denoised at frame 0
PTRS = ("viewz", "mv", "nr", "in_d", "in_s", "out_d", "out_s", "prev_slow_d", "prev_slow_s", "prev_fast_d", "prev_fast_s", "prev_guide",
        "slow_d", "slow_s", "fast_d", "fast_s", "guide", "x_d", "x_s")
SLOT = ("slow_d", "slow_s", "fast_d", "fast_s", "guide")


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_reblur_shim())
    lib.rb_host_pass.restype = None
    lib.rb_host_pass.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rb_host_radius.restype = C.c_float
    lib.rb_host_radius.argtypes = [C.c_float] * 4
    lib.rb_host_spec_cap.restype = C.c_float
    lib.rb_host_spec_cap.argtypes = [C.c_uint32, C.c_float, C.c_float, C.c_float]
    return lib


@pytest.fixture(scope="module")
def dn_shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_denoise_shim())
    lib.dn_host_pass.restype = None
    lib.dn_host_pass.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


class HostReblur:
    """pt_nrd_reblur on the host-compiled header, with the history logic of pt_api_post.hip: the first call and a call with another size
    restart; two history slots alternate."""

    def __init__(self, shim):
        self.shim, self.key, self.slots, self.cur = shim, None, None, 0

    def __call__(self, z, mv, nr, ind, ins, accumulation=0, frame_index=0, max_n=0, max_fast=0, fix=0, rmin=0.0, rmax=0.0, out=None, keep=False):
        z = c32(z)
        h, w = z.shape[:2]
        restart = accumulation != 0 or self.key is None
        if self.key != (w, h):
            self.slots = [{k: np.zeros((h, w, 4), np.float32) for k in SLOT} for _ in range(2)]
            restart = True
        self.key = (w, h)
        prev, cur = self.slots[self.cur], self.slots[self.cur ^ 1]
        b = dict(viewz=z, mv=c32(mv), nr=c32(nr), in_d=c32(ind), in_s=c32(ins), x_d=np.full((h, w, 4), np.nan, np.float32),
                 x_s=np.full((h, w, 4), np.nan, np.float32))
        b["out_d"], b["out_s"] = (c32(o).copy() for o in out) if out is not None else (np.full((h, w, 4), SENTINEL, np.float32) for _ in range(2))
        b.update({"prev_" + k: v for k, v in prev.items()})
        b.update(cur)
        ptrs = (C.c_void_p * len(PTRS))(*[b[k].ctypes.data for k in PTRS])
        prm = np.array([w, h, max_n or 30, max_fast or 6, fix or 3, 1 if restart else 0, frame_index], np.uint32)
        radii = np.array([rmin or 1.0, rmax or 30.0], np.float32)
        passes = {}
        for p, (name, keys) in enumerate((("temporal", ("x_d", "x_s", "fast_d", "fast_s", "guide")), ("fix", ("slow_d", "slow_s")),
                                          ("blur", ("x_d", "x_s")), ("post", ("out_d", "out_s", "slow_d", "slow_s")))):
            self.shim.rb_host_pass(p, prm.ctypes.data, radii.ctypes.data, ptrs)
            if keep:
                passes[name] = {k: b[k].copy() for k in keys}
        self.cur ^= 1
        self.restarted = restart
        if keep:
            passes["prev"] = None if restart else {k: v.copy() for k, v in prev.items()}
            return b["out_d"], b["out_s"], passes
        return b["out_d"], b["out_s"]

    def history(self):
        """the slot the last call wrote"""
        return self.slots[self.cur]


def check(got, want, scale, what, fragile, hit):
    """got (float32) against want (float64) where want is not NaN and the pixel is not fragile: |got - want| <= PASS_RTOL * scale.
    The share of hit pixels left out is a condition: at most FRAGILE_MAX."""
    share = fragile[hit].mean() if hit.any() else 0.0
    assert share <= FRAGILE_MAX, f"{what}: the restatement leaves out {share:.4%} of the hit pixels"
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    m = ~np.isnan(want) & ~fragile[..., None]
    with np.errstate(invalid="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want)) / scale
    bad = m & ~(err <= PASS_RTOL)
    worst = float(np.max(np.where(m, err, 0.0)))
    print(f"{what}: left out {share:.4%}, worst relative error {worst:.3g}")
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels off (worst {worst:.3g}), first {np.argwhere(bad)[:4].tolist()}"
    return worst


def window_max(a, r):
    out = np.where(np.isnan(a), -np.inf, a)
    res = out.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            res = np.maximum(res, dref.shift(out, dx, dy, -np.inf))
    return res


def sequence(rng, w, h, calls, miss=0.1):
    """random_frame images of one surface (the guides of the first call stay, so most of the history survives)"""
    frames = []
    z0 = nr0 = None
    for _ in range(calls):
        z, mv, nr, ind, ins = random_frame(rng, w, h, REBLUR, miss=miss)
        if z0 is not None:
            z, nr = np.where(np.isfinite(z0), z0, z).astype(np.float32), nr0
        z0, nr0 = z, nr
        frames.append((z, mv, nr, ind, ins))
    return frames


# ------------------------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("seed", [0, 1])
def test_header_passes_match_numpy_restatement(shim, seed):
    """three calls (a restart, then two with history, so the history fix and the clamp act on mixed history lengths) on random 41 x 29
    images with misses, zero hit distances, fireflies and motion; each pass of the header against the restatement fed the header's own
    fp32 results of the pass before"""
    rng = np.random.default_rng(seed)
    w, h = 41, 29
    d = HostReblur(shim)
    fixed = 0
    for call, (z, mv, nr, ind, ins) in enumerate(sequence(rng, w, h, 3)):
        out_d, out_s, p = d(z, mv, nr, ind, ins, frame_index=5 + call, max_n=20, keep=True)
        hit = np.isfinite(z)
        t = ref.temporal(z, mv, nr, ind, ins, p["prev"], 20, 6)
        got = p["temporal"]
        for k in ("x_d", "x_s", "fast_d", "fast_s", "guide"):
            scale = np.maximum(np.abs(t[k]).max(axis=-1, keepdims=True), 1e-3)
            check(got[k], t[k], scale, f"call {call}: temporal {k}", t["fragile"], hit)
        n_d = got["fast_d"][..., 3]
        assert (n_d[hit] == 1).all() if call == 0 else (n_d[hit] > 1.5).mean() > 0.5
        fixed += int((n_d[hit] < 3).sum()) if call else 0
        fd, fs, frag = ref.fix(z, nr, got["x_d"], got["x_s"], got["fast_d"], got["fast_s"], 3)
        for g, want, k in ((p["fix"]["slow_d"], fd, "d"), (p["fix"]["slow_s"], fs, "s")):
            scale = np.maximum(window_max(np.maximum(np.abs(got["x_" + k][..., :3]).max(-1), np.abs(got["fast_" + k][..., :3]).max(-1)), 4), 1e-3)[..., None]
            check(g, want, scale, f"call {call}: history fix and clamp {k}", frag, hit)
        for post, name, src in ((False, "blur", p["fix"]), (True, "post", p["blur"])):
            sd, ss = (src["slow_d"], src["slow_s"]) if not post else (src["x_d"], src["x_s"])
            bd, bs, frag, _ = ref.blur(z, nr, sd, ss, got["fast_d"], got["fast_s"], 5 + call, post, 1.0, 30.0)
            gd, gs = (p["blur"]["x_d"], p["blur"]["x_s"]) if not post else (p["post"]["out_d"], p["post"]["out_s"])
            for g, want, s_ in ((gd, bd, sd), (gs, bs, ss)):
                scale = np.nanmax(np.abs(np.where(hit[..., None], s_, np.nan)[..., :3])) * np.ones(g.shape[:2] + (1,))
                check(g, np.where(hit[..., None], want, np.nan), scale, f"call {call}: {name}", frag, hit)
        for o in (out_d, out_s):  # misses are never written
            assert np.array_equal(o[~hit].view(np.uint32), np.full(o[~hit].shape, SENTINEL).view(np.uint32))
            assert np.isfinite(o[hit]).all()
    assert fixed > 0  # the history fix acted on a call with history


def test_constant_signal_on_a_plane_is_bit_identical(shim):
    w, h = 40, 24
    z, mv, nr = plane(w, h)
    d = HostReblur(shim)
    ind, ins = lobe(w, h, (0.5, 0.25, 2.0), 0.25, REBLUR), lobe(w, h, (1.5, 0.75, 0.125), 0.5, REBLUR)
    for f in range(5):
        od, os_, p = d(z, mv, nr, ind, ins, frame_index=f, keep=True)
        for name, keys in (("temporal", ("x_d", "x_s")), ("fix", ("slow_d", "slow_s")), ("blur", ("x_d", "x_s")), ("post", ("out_d", "out_s"))):
            for k, i in zip(keys, (ind, ins)):
                bits_equal(p[name][k], i, f"call {f}: {name} {k}")
        bits_equal(od, ind, "OutDiffuse")
        bits_equal(os_, ins, "OutSpecular")


def test_misses_keep_the_sentinel_are_never_taps_and_out_w_is_the_reconstructed_hit_distance(shim):
    w, h = 12, 10
    z, mv, nr = plane(w, h, z=5.0)
    z[0, :] = np.inf
    z[4, 4] = np.nan
    ind = lobe(w, h, (1, 1, 1), 0.5, REBLUR)
    ind[6, 6, 3] = 0.0         # neighbours all 0.5 -> 0.5
    ind[8, 2:5, 3] = [0.25, 0.0, 0.75]
    ind[7:10, 3, 3] = 0.0      # (8, 3): nonzero neighbours at depth 5: 0.25 (left), 0.75 (right), 0.5 at (7, 2), (7, 4), (9, 2) -> mean
    z[9, 4] = 9.0              # ... but (9, 4) fails the depth test
    ins = lobe(w, h, (1, 1, 1), 0.0, REBLUR)  # no specular hit distance anywhere: stays 0
    miss = ~np.isfinite(z)
    ind[miss, :3] = 1e30       # a miss's values would wreck any sum they entered
    ins[miss, :3] = -1e30
    d = HostReblur(shim)
    for f in range(3):
        od, os_ = d(z, mv, nr, ind, ins, frame_index=f)
        for o in (od, os_):
            assert np.array_equal(o[miss].view(np.uint32), np.full(o[miss].shape, SENTINEL).view(np.uint32))
            assert np.abs(o[~miss][:, :3]).max() < 10.0
        assert od[6, 6, 3] == 0.5
        assert od[8, 3, 3] == np.float32((0.5 + 0.5 + 0.25 + 0.75 + 0.5) / 5.0)
        assert (os_[~miss, 3] == 0).all()
        hs = d.history()
        assert (hs["fast_d"][miss] == 0).all() and (hs["slow_d"][miss] == 0).all()  # history reset: length 0


def test_the_history_written_is_the_output(shim):
    """recurrence: the slow history slot of a call is its Out (the signal YCoCg-encoded as Out is, and the hit distance), bit for bit"""
    rng = np.random.default_rng(5)
    d = HostReblur(shim)
    for f, (z, mv, nr, ind, ins) in enumerate(sequence(rng, 33, 21, 3)):
        od, os_ = d(z, mv, nr, ind, ins, frame_index=f)
        hit = np.isfinite(z)
        bits_equal(d.history()["slow_d"][hit], od[hit], "slow diffuse")
        bits_equal(d.history()["slow_s"][hit], os_[hit], "slow specular")


def test_half_planes_do_not_bleed(shim):
    w, h = 48, 24
    z, mv, nr = plane(w, h)
    z[:, : w // 2] = 1.0
    z[:, w // 2:] = 10.0
    ind = np.concatenate([lobe(w // 2, h, (0.25, 0.5, 1.0), 0.5, REBLUR), lobe(w // 2, h, (4.0, 2.0, 1.0), 0.5, REBLUR)], axis=1)
    ins = ind[:, ::-1].copy()
    d = HostReblur(shim)
    for f in range(3):
        od, os_ = d(z, mv, nr, ind, ins, frame_index=f)
        for o, i in ((od, ind), (os_, ins)):
            assert (np.abs(o - i) <= 2 * np.spacing(np.abs(i))).all(), np.abs(o - i).max()


def impulse(w, h, rough, a, calls, shim, **kw):
    """an impulse of Y = 64 at the centre of a flat plane, the same input `calls` times -> (last OutDiffuse Y, last OutSpecular Y)"""
    z, mv, nr = plane(w, h, rough=rough)
    ind, ins = lobe(w, h, (1, 1, 1), a, REBLUR), lobe(w, h, (1, 1, 1), a, REBLUR)
    # (the 3x3 anti-firefly would clamp a single bright pixel: the impulse is a 3 x 3 block, whose centre the response is measured around)
    for x in (ind, ins):
        x[h // 2 - 1: h // 2 + 2, w // 2 - 1: w // 2 + 2, 0] = 64.0
    d = HostReblur(shim)
    for f in range(calls):
        od, os_ = d(z, mv, nr, ind, ins, frame_index=f, **kw)
    return od[..., 0] - ind[..., 0], os_[..., 0] - ins[..., 0]


def support(delta):
    """the largest Chebyshev distance from the image centre at which the response differs from the input"""
    h, w = delta.shape
    ys, xs = np.nonzero(delta != 0)
    return 0 if len(xs) == 0 else int(max(np.abs(xs - w // 2).max(), np.abs(ys - h // 2).max()))


def test_radius_mirror_is_untouched_and_support_follows_history_and_hit_distance(shim):
    w, h = 151, 151
    # a mirror: no spatial spread at all, in any call
    for calls in (1, 3):
        dd, ds = impulse(w, h, 0.002, 0.5, calls, shim)
        assert (ds == 0).all()
        assert (dd != 0).any()
    # the response lies within the spec's radius (two passes of at most R each, + 1 for the block, + 1 for the rounding) and shrinks with n
    r1 = shim.rb_host_radius(1.0, 30.0, 1.0, 0.5)
    assert r1 == pytest.approx(30.0 * np.sqrt(0.5), rel=1e-6)
    d1, s1 = impulse(w, h, 0.6, 0.5, 1, shim)
    d20, s20 = impulse(w, h, 0.6, 0.5, 20, shim)
    for a, b in ((d1, d20), (s1, s20)):
        assert 4 < support(a) <= 2 * (r1 + 1) + 1
        assert support(b) < support(a)
    # with history: the first call's spread is part of the history, so compare the radius the header uses, and a fresh impulse after 19 calls
    r20 = shim.rb_host_radius(1.0, 30.0, 20.0, 0.5)
    assert r20 < r1 and r20 == pytest.approx(30.0 * np.sqrt(0.5 / 20.0), rel=1e-6)
    # the support grows with the normalised hit distance, in both lobes
    small = [support(x) for x in impulse(w, h, 0.6, 0.02, 1, shim)]
    large = [support(x) for x in impulse(w, h, 0.6, 0.9, 1, shim)]
    assert all(s < l for s, l in zip(small, large)), (small, large)
    # the radius' shape: within [Rmin, Rmax], not increasing in n, not decreasing in the hit distance
    ns, hs = np.arange(1, 40, dtype=np.float32), np.linspace(0, 1, 33, dtype=np.float32)
    R = np.array([[shim.rb_host_radius(2.0, 40.0, float(n), float(a)) for a in hs] for n in ns])
    assert R.min() >= 2.0 and R.max() <= 40.0 and (np.diff(R, axis=0) <= 0).all() and (np.diff(R, axis=1) >= 0).all()
    assert R[0, -1] == 40.0 and R[-1, 0] == 2.0


def test_history_length_at_rest_reaches_the_cap_for_a_mirror_too(shim, dn_shim):
    w, h = 24, 16
    z, mv, nr = plane(w, h)
    nr[:, : w // 2, 3] = 0.002  # mirror
    nr[:, w // 2:, 3] = 0.6
    rng = np.random.default_rng(3)
    d, s15 = HostReblur(shim), HostDenoiser(dn_shim)
    for k in range(1, 16):
        ind, ins = (lobe(w, h, rng.uniform(0.1, 1.0, 3), 0.2, REBLUR) for _ in range(2))
        d(z, mv, nr, ind, ins, frame_index=k, max_n=12, max_fast=4)
        s15(REBLUR, z, mv, nr, ind, ins, max_d=12, max_s=12)
        hs = d.history()
        assert (hs["fast_d"][..., 3] == min(k, 12)).all(), k
        assert (hs["fast_s"][..., 3] == min(k, 12)).all(), k  # the mirror half too
        assert (s15.history()["sig_s"][:, : w // 2, 3] == 1).all()  # S15's cap for the mirror
        assert (s15.history()["sig_s"][:, w // 2:, 3] == min(k, 12)).all()


def test_specular_cap_falls_with_motion(shim):
    cap = lambda r, m: shim.rb_host_spec_cap(30, r, m, 0.0)  # noqa: E731
    for r in (0.0, 0.002, 0.1, 0.3, 0.5, 1.0):
        c15 = max(1.0, np.floor(30 * min(r / 0.5, 1.0) + 0.5))
        caps = [cap(r, m) for m in (0.0, 0.25, 0.5, 1.0, 2.0, 8.0, 64.0, 1e6)]
        assert caps[0] == 30.0  # at rest: MaxAccumulatedFrames for every roughness
        assert all(a >= b for a, b in zip(caps, caps[1:])) and all(c >= 1.0 for c in caps)
        assert caps[-1] == c15  # far motion: S15's roughness-scaled cap
        assert shim.rb_host_spec_cap(30, r, 0.6, 0.8) == cap(r, 1.0)  # |MV.xy|
    assert cap(0.002, 1.0) == np.floor(1 + 29 / 3.0 + 0.5)
    assert shim.rb_host_spec_cap(30, 0.002, np.nan, 0.0) == 1.0 and shim.rb_host_spec_cap(30, 0.002, np.inf, 0.0) == 1.0
    # in the filter: a moving mirror's history stays short, a resting one's grows
    w, h = 16, 12
    z, mv, nr = plane(w, h, rough=0.002)
    mv[:, w // 2:, 0] = -1.0  # the right half's surface was one pixel to the left (its first column reprojects onto the resting half)
    ind = ins = lobe(w, h, (1, 2, 3), 0.3, REBLUR)
    d = HostReblur(shim)
    for _ in range(14):
        d(z, mv, nr, ind, ins)
    n = d.history()["fast_s"][..., 3]
    assert (n[:, : w // 2] == 14).all() and (n[:, w // 2:] == 11).all()


@pytest.mark.parametrize("accumulation", [1, 2])
def test_restart_modes_reset_history(shim, accumulation):
    w, h = 16, 12
    z, mv, nr = plane(w, h)
    ind = ins = lobe(w, h, (1, 2, 3), 0.3, REBLUR)
    d = HostReblur(shim)
    for _ in range(5):
        d(z, mv, nr, ind, ins)
    assert (d.history()["fast_d"][..., 3] == 5).all()
    d(z, mv, nr, ind, ins, accumulation=accumulation)
    assert d.restarted and (d.history()["fast_d"][..., 3] == 1).all() and (d.history()["fast_s"][..., 3] == 1).all()
    d(z, mv, nr, ind, ins)
    assert (d.history()["fast_d"][..., 3] == 2).all()


def test_depth_step_restarts_exactly_the_disoccluded_pixels(shim):
    w, h = 32, 20
    z, mv, nr = plane(w, h, z=6.0)
    ind = ins = lobe(w, h, (1, 1, 1), 0.3, REBLUR)
    d = HostReblur(shim)
    for _ in range(3):
        d(z, mv, nr, ind, ins)
    z2 = z.copy()
    z2[5:12, 8:20] = 3.0  # an occluder moves in; the motion vector says the background is where it was
    z2[0, 0] = 6.0 * 1.04  # |6 - z| within 5 % of z: kept
    z2[0, 1] = 6.0 * 1.06  # beyond: restarted
    d(z2, mv, nr, ind, ins)
    restarted = np.zeros((h, w), bool)
    restarted[5:12, 8:20] = True
    restarted[0, 1] = True
    for k in ("fast_d", "fast_s"):
        n = d.history()[k][..., 3]
        assert (n[restarted] == 1).all() and (n[~restarted] == 4).all()


def test_responsiveness_to_a_step(shim):
    """a noise-free constant input at rest for 40 calls, then a step: six calls later the output has covered at least 0.6 of it (the
    fast history of cap 6 covers 1 - (5/6)^6 = 0.665 and the clamp ties the slow one to it; the slow one alone: 1 - (29/30)^6 = 0.18)"""
    w, h = 20, 14
    z, mv, nr = plane(w, h)
    d = HostReblur(shim)
    lo, hi = lobe(w, h, (1, 1, 1), 0.3, REBLUR), lobe(w, h, (3, 3, 3), 0.3, REBLUR)
    for f in range(40):
        od, os_ = d(z, mv, nr, lo, lo, frame_index=f)
    bits_equal(od, lo, "settled")
    for f in range(6):
        od, os_ = d(z, mv, nr, hi, hi, frame_index=40 + f)
    for o in (od, os_):
        covered = (o[..., 0] - lo[..., 0]) / (hi[..., 0] - lo[..., 0])
        assert covered.min() >= 0.6, covered.min()
        assert covered.max() <= 0.67


def test_motion_whole_pixel_translation_gives_the_resting_result_shifted(shim):
    """a pattern that moves by (4, -4) pixels per call (a multiple of the 4 x 4 rotation pattern) with the matching motion vector: after
    8 calls the output is the resting one shifted by 28 pixels each way.  The blur is recurrent, so what the image border and the strip
    that enters the moving window change travels on with every call: per call the largest radius (MaxBlurRadius 3 here, + 1 for the
    rounding) twice, the history fix's 4 and the 4 pixels that enter; the band of 8 such reaches is left out.  Tolerance: 4 fp32
    roundings of the signal's scale (1) -- the two runs do the same arithmetic on the same numbers (the reprojection's bilinear weights
    are 1 and three zeros either way, float(x) + MV is exact), so no difference at all is expected."""
    calls, step, rmax = 8, 4, 3.0
    band = calls * (2 * (int(rmax) + 1) + 4 + step)
    w = h = 2 * band + 64
    rng = np.random.default_rng(9)
    W, H = w + step * calls, h + step * calls
    zz = np.ascontiguousarray(np.broadcast_to((5.0 + 0.01 * np.arange(W))[None, :], (H, W))).astype(np.float32)
    big_nr = np.zeros((H, W, 4), np.float32)
    big_nr[..., 2] = -1.0
    big_nr[..., 3] = 0.6  # (the cap of a specular this rough does not depend on the motion)
    x0, y0 = 0, step * (calls - 1)
    rest, move = HostReblur(shim), HostReblur(shim)
    win = lambda a, ox, oy: np.ascontiguousarray(a[oy: oy + h, ox: ox + w])  # noqa: E731
    for f in range(calls):
        lobes = [np.concatenate([rng.uniform(0.2, 1.0, (H, W, 3)), rng.uniform(0.1, 0.9, (H, W, 1))], axis=-1).astype(np.float32) for _ in range(2)]
        # resting: the window stays at (x0, y0); moving: the window slides there, so the content moves by (+step, -step) pixels per call
        fx, fy = step * (calls - 1 - f), step * f
        mv0 = np.zeros((h, w, 3), np.float32)
        mv1 = mv0.copy()
        if f:
            mv1[..., 0], mv1[..., 1] = -step, step  # previous - current position of the surface, in pixels
        r = rest(win(zz, x0, y0), mv0, win(big_nr, x0, y0), win(lobes[0], x0, y0), win(lobes[1], x0, y0), frame_index=f, rmax=rmax)
        m = move(win(zz, fx, fy), mv1, win(big_nr, fx, fy), win(lobes[0], fx, fy), win(lobes[1], fx, fy), frame_index=f, rmax=rmax)
    assert (fx, fy) == (x0, y0)
    inner = (slice(band, h - band), slice(band, w - band))
    for a, b in zip(r, m):
        assert np.abs(a[inner] - b[inner]).max() <= 4 * 2.0 ** -23, np.abs(a[inner] - b[inner]).max()
    assert (r[0][inner] != win(lobes[0], x0, y0)[inner]).any()
    assert (move.history()["fast_d"][inner][..., 3] == calls).all()


def test_quality_on_the_oracles_frames(dxrs, host, oracle, shim, dn_shim):
    """16 resting frames of the C2 crop through pack -> pt_nrd_reblur -> compose (host-compiled headers), the chain and truth of
    test_nrd_denoise.test_quality_on_the_oracles_frames: (i) the composed frame at frame 0 beats the noisy one, (ii) frame 15 beats frame
    0, (iii) frame 15 is strictly below what S15's filter in ReBLUR mode reaches at frame 15, computed here in the same run"""
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
    rb, s15 = HostReblur(shim), HostDenoiser(dn_shim)
    errs, errs15 = [], []
    for f, x in enumerate(frames):
        y = dict(x, **x[REBLUR])
        flat = lambda k: y[k].reshape(-1, y[k].shape[-1])  # noqa: E731
        z = y["LinearDepth"][..., 0]
        pd, ps = host_pass(nrd, REBLUR, True, dict(LinearDepth=z.ravel(), DiffuseAlbedo=flat("DiffuseAlbedo"), SpecularAlbedo=flat("SpecularAlbedo"),
                                                   NormalRoughness=flat("NormalRoughness"), NoisyDiffuse=flat("NoisyDiffuse"),
                                                   NoisySpecular=flat("NoisySpecular")))
        shape = y["NoisyDiffuse"].shape
        packed = (pd.reshape(shape), ps.reshape(shape))
        base = dict(LinearDepth=z.ravel(), DiffuseAlbedo=flat("DiffuseAlbedo"), SpecularAlbedo=flat("SpecularAlbedo"), Radiance=flat("Emission"))
        m = np.isfinite(z).ravel()
        od, os_ = rb(z, y["MotionVector"], y["NormalRoughness"], *packed, frame_index=f, out=packed)
        rad = host_pass(nrd, REBLUR, False, dict(base, DenoisedDiffuse=od.reshape(-1, 4), DenoisedSpecular=os_.reshape(-1, 4)))
        errs.append(rmse(rad.reshape(-1, 4), truth.reshape(-1, 4), m))
        od, os_ = s15(REBLUR, z, y["MotionVector"], y["NormalRoughness"], *packed, out=packed)
        rad = host_pass(nrd, REBLUR, False, dict(base, DenoisedDiffuse=od.reshape(-1, 4), DenoisedSpecular=os_.reshape(-1, 4)))
        errs15.append(rmse(rad.reshape(-1, 4), truth.reshape(-1, 4), m))
        if f == 0:
            noisy = host_pass(nrd, REBLUR, False, dict(base, DenoisedDiffuse=pd, DenoisedSpecular=ps))
            e_noisy = rmse(noisy.reshape(-1, 4), truth.reshape(-1, 4), m)
    hit = np.isfinite(frames[0]["LinearDepth"][..., 0])
    for k in ("fast_d", "fast_s"):  # at rest the history is full wherever there is a surface, the mirrors included
        assert (rb.history()[k][..., 3][hit] > QUALITY_FRAMES - 0.01).all(), k
    print(f"noisy {e_noisy:.4f}; pt_nrd_reblur frame 0 {errs[0]:.4f} ({errs[0] / e_noisy:.3f}) frame 15 {errs[-1]:.4f} ({errs[-1] / errs[0]:.3f}); "
          f"S15 frame 0 {errs15[0]:.4f} frame 15 {errs15[-1]:.4f}; all {[round(e, 4) for e in errs]}")
    assert errs[0] < QUALITY_RATIO_0 * e_noisy, (e_noisy, errs)
    assert errs[-1] < QUALITY_RATIO_15 * errs[0], (e_noisy, errs)
    assert errs[-1] < errs15[-1], (errs, errs15)


def test_sanitizer_program(tmp_path):
    """tests/cpp/reblur_sanitize.cpp: the header under AddressSanitizer + UBSan as a stand-alone program (guard bytes around every
    buffer; 1 x 1, 1 x 40 and 37 x 11 with the largest radius, so taps leave the image on every border)"""
    import __graft_entry__ as g
    exe = g.build_reblur_sanitizer(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "reblur_sanitize ok" in res.stdout, res.stdout + res.stderr


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import PtNrdDenoiseTextures, PtNrdReblurSettings as S, nrd_reblur_settings
    hip = dxrs.load_hip()
    lib = hip.lib
    assert C.sizeof(S) == 48 and C.sizeof(PtNrdDenoiseTextures) == 64
    assert (S.RenderSize.offset, S.AccumulationMode.offset, S.FrameIndex.offset, S.MaxAccumulatedFrames.offset, S.MaxFastAccumulatedFrames.offset,
            S.HistoryFixFrames.offset, S.MinBlurRadius.offset, S.MaxBlurRadius.offset, S._pad.offset) == (0, 8, 12, 16, 20, 24, 28, 32, 36)
    assert "pt_nrd_reblur" in dxrs.binding.API_SYMBOLS and "pt_nrd_reblur_history" in dxrs.binding.API_SYMBOLS
    assert lib.pt_nrd_reblur.argtypes[1]._type_ is S and lib.pt_nrd_reblur.argtypes[2]._type_ is PtNrdDenoiseTextures
    s = nrd_reblur_settings(64, 64, frame_index=3, max_blur_radius=12.5)
    assert (s.RenderSize[0], s.RenderSize[1], s.FrameIndex, s.MaxBlurRadius, tuple(s._pad)) == (64, 64, 3, 12.5, (0, 0, 0))
    assert lib.pt_nrd_reblur(None, C.byref(s), C.byref(PtNrdDenoiseTextures())) == 1
    assert lib.pt_nrd_reblur(None, None, None) == 1
    assert lib.pt_nrd_reblur_history(None, None, None, None, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU

TEX = ("ViewZ", "MotionVector", "NormalRoughness", "InDiffuse", "InSpecular")


class GpuReblur:
    """pt_nrd_reblur on device copies; outputs start as the sentinel"""

    def __init__(self, renderer):
        self.r = renderer

    def __call__(self, z, mv, nr, ind, ins, accumulation=0, frame_index=0, max_n=0, max_fast=0, fix=0, rmin=0.0, rmax=0.0):
        import torch
        h, w = np.asarray(z).shape[:2]
        d = {k: torch.from_numpy(c32(v)).cuda() for k, v in zip(TEX, (z, mv, nr, ind, ins))}
        out = [torch.from_numpy(np.full((h, w, 4), SENTINEL, np.float32)).cuda() for _ in range(2)]
        torch.cuda.synchronize()
        self.r.nrd_reblur_device(w, h, dict({k: t.data_ptr() for k, t in d.items()}, OutDiffuse=out[0].data_ptr(), OutSpecular=out[1].data_ptr()),
                                 accumulation_mode=accumulation, frame_index=frame_index, max_accumulated_frames=max_n, max_fast_accumulated_frames=max_fast,
                                 history_fix_frames=fix, min_blur_radius=rmin, max_blur_radius=rmax)
        self.r.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()


def compare_sequence(renderer, shim, frames, what, **kw):
    """the frames (z, mv, nr, ind, ins, accumulation, frame_index) through the GPU and the host header -> Out and the history slot bit
    for bit, misses untouched"""
    gpu, host = GpuReblur(renderer), HostReblur(shim)
    for f, (z, mv, nr, ind, ins, acc, fi) in enumerate(frames):
        acc = 2 if f == 0 else acc  # (the shared context carries other tests' history)
        gd, gs = gpu(z, mv, nr, ind, ins, accumulation=acc, frame_index=fi, **kw)
        hd, hs = host(z, mv, nr, ind, ins, accumulation=acc, frame_index=fi, **kw)
        bits_equal(gd, hd, f"{what} frame {f}: OutDiffuse")
        bits_equal(gs, hs, f"{what} frame {f}: OutSpecular")
        miss = ~np.isfinite(np.asarray(z))
        assert np.array_equal(gd[miss].view(np.uint32), np.full(gd[miss].shape, SENTINEL).view(np.uint32))
        h, w = miss.shape
        slot = renderer.nrd_reblur_history(w, h)
        for k in SLOT:
            bits_equal(slot[k], host.history()[k], f"{what} frame {f}: history {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (41, 29), (333, 197)])
def test_gpu_bit_exact_random_sequences(renderer, shim, size):
    """four calls with motion, a RESTART in the middle and a changing FrameIndex"""
    w, h = size
    rng = np.random.default_rng(w + 3 * h)
    frames = [fr + (acc, fi) for fr, acc, fi in zip(sequence(rng, w, h, 4), (0, 0, 1, 0), (7, 8, 21, 22))]
    compare_sequence(renderer, shim, frames, f"{w}x{h}", max_n=20, max_fast=5, rmax=(64.0 if w > 100 else 0.0))


def real_chain(dxrs, host, renderer, shim, kind, n_frames=8, w=480, h=270):
    """test_nrd_denoise.real_chain's recipe with pt_nrd_reblur: n_frames of the C2 scene through nrd_chain with the GPU denoiser; each
    frame's packed buffers and guides through the host header in the same order -> bit for bit"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    renderer.set_scene(spheres, mats, sd)
    hd = HostReblur(shim)
    den = renderer.nrd_reblur_denoiser(rect=(0, 0, w, h), frame_index=100)
    prev_cam = None
    for f in range(n_frames):
        pos = (0.0, 0.0, -15.0) if kind != "travelling" else (0.15 * f, 0.05 * f, -15.0 + 0.1 * f)
        cam = host.camera_matrices(w, h, position=pos, look_at=(0.0, 0.0, 0.0), jitter_index=f, previous=prev_cam)
        renderer.set_camera(cam)
        prev_cam = cam
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
        x = renderer.nrd_chain(REBLUR, rect=(0, 0, w, h), denoise=den)
        z = x["LinearDepth"][..., 0]
        want_d, want_s = hd(z, x["MotionVector"], x["NormalRoughness"], x["PackedDiffuse"], x["PackedSpecular"], frame_index=100 + f,
                            out=(x["PackedDiffuse"], x["PackedSpecular"]))
        bits_equal(x["DenoisedDiffuse"], want_d, f"{kind} frame {f}: OutDiffuse")
        bits_equal(x["DenoisedSpecular"], want_s, f"{kind} frame {f}: OutSpecular")
        if kind != "resting":
            assert np.abs(x["MotionVector"][np.isfinite(z)][:, :2]).max() > 0.1 or f == 0
    assert hd.history()["fast_d"][..., 3].max() >= min(n_frames, 2)
    assert (x["DenoisedDiffuse"] != x["PackedDiffuse"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["resting", "travelling"])
def test_gpu_real_chain_bit_exact(dxrs, host, renderer, shim, kind):
    real_chain(dxrs, host, renderer, shim, kind)


@pytest.mark.gpu
def test_gpu_alternation_with_pt_nrd_denoise_on_one_context(dxrs, renderer, shim, dn_shim):
    """pt_nrd_reblur and pt_nrd_denoise (ReBLUR mode) called in turn on one context: each call's result is what a denoiser of its own
    gives (the host mirrors, which the other GPU tests pin the kernels to bit for bit) -- neither disturbs the other's history"""
    from test_nrd_denoise import GpuDenoiser
    w, h = 61, 37
    rng = np.random.default_rng(21)
    gpu_rb, gpu_dn, host_rb, host_dn = GpuReblur(renderer), GpuDenoiser(renderer), HostReblur(shim), HostDenoiser(dn_shim)
    for f, (z, mv, nr, ind, ins) in enumerate(sequence(rng, w, h, 4)):
        acc = 2 if f == 0 else 0
        for o, want, what in zip(gpu_rb(z, mv, nr, ind, ins, accumulation=acc, frame_index=f), host_rb(z, mv, nr, ind, ins, accumulation=acc, frame_index=f),
                                 ("OutDiffuse", "OutSpecular")):
            bits_equal(o, want, f"frame {f}: pt_nrd_reblur {what}")
        for o, want, what in zip(gpu_dn(REBLUR, z, mv, nr, ind, ins, accumulation=acc), host_dn(REBLUR, z, mv, nr, ind, ins, accumulation=acc),
                                 ("OutDiffuse", "OutSpecular")):
            bits_equal(o, want, f"frame {f}: pt_nrd_denoise {what}")
    assert host_rb.history()["fast_d"][..., 3].max() > 2 and host_dn.history()["sig_d"][..., 3].max() > 2


@pytest.mark.gpu
def test_gpu_render_size_change_restarts(renderer, shim):
    rng = np.random.default_rng(11)
    gpu, host = GpuReblur(renderer), HostReblur(shim)
    for f, (w, h) in enumerate(((40, 30), (40, 30), (30, 40), (30, 40), (30, 40))):
        z, mv, nr, ind, ins = random_frame(rng, w, h, REBLUR, miss=0.0)
        mv[:] = 0.0
        acc = 2 if f == 0 else 0
        got, want = gpu(z, mv, nr, ind, ins, accumulation=acc, frame_index=f), host(z, mv, nr, ind, ins, accumulation=acc, frame_index=f)
        assert host.restarted == (f in (0, 2))
        bits_equal(got[0], want[0], f"call {f}: OutDiffuse")
        bits_equal(got[1], want[1], f"call {f}: OutSpecular")
        n = renderer.nrd_reblur_history(w, h)["fast_d"][..., 3]
        assert np.array_equal(n, host.history()["fast_d"][..., 3])
        assert n.max() == (1, 2, 1, 2, 3)[f]  # (a pixel whose random normal turned too far restarts on its own)


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """three lanes and six frames of a travelling camera, G-buffer -> pt_render_denoiser -> pack -> pt_nrd_reblur -> compose all queued
    without waiting, equal the same frames run one at a time on a one-lane context"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 320, 180
    frames = 6
    width = dict(dxrs.types.GBUFFER_CHANNELS)
    names = ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "MotionVector")

    def run(r, lanes):
        got = []
        sets = []
        for _ in range(3):
            s = {k: torch.zeros((h, w, width[k]), dtype=torch.float32, device="cuda") for k in names}
            s.update({k: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for k in ("Noisy0", "Noisy1", "Out0", "Out1", "Radiance")})
            sets.append(s)
        torch.cuda.synchronize()
        r.set_scene(spheres, mats, sd)
        for f in range(frames):
            r.set_camera(host.camera_matrices(w, h, position=(0.2 * f, 0.0, -15.0 + 0.1 * f), look_at=(0.0, 0.0, 0.0), jitter_index=f))
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
            s = sets[f % 3]
            r.render_gbuffer_device({k: s[k].data_ptr() for k in names})
            r.render_denoiser_device(REBLUR, s["Radiance"].data_ptr(), {"Diffuse": s["Noisy0"].data_ptr(), "Specular": s["Noisy1"].data_ptr()})
            inputs = {k: s[k].data_ptr() for k in names[:4]}
            r.nrd_composition_device(REBLUR, True, w, h, dict(inputs, NoisyDiffuse=s["Noisy0"].data_ptr(), NoisySpecular=s["Noisy1"].data_ptr()))
            r.nrd_reblur_device(w, h, dict(ViewZ=s["LinearDepth"].data_ptr(), MotionVector=s["MotionVector"].data_ptr(),
                                           NormalRoughness=s["NormalRoughness"].data_ptr(), InDiffuse=s["Noisy0"].data_ptr(),
                                           InSpecular=s["Noisy1"].data_ptr(), OutDiffuse=s["Out0"].data_ptr(), OutSpecular=s["Out1"].data_ptr()),
                                accumulation_mode=2 if f == 0 else 0, frame_index=f)
            r.nrd_composition_device(REBLUR, False, w, h, dict(inputs, DenoisedDiffuse=s["Out0"].data_ptr(), DenoisedSpecular=s["Out1"].data_ptr(),
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
        for k in names + ("Out0", "Out1", "Radiance"):
            bits_equal(many[f][k], one[f][k], f"frame {f}: {k}")
    assert (one[-1]["Out0"] != one[-1]["Noisy0"]).any()


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, renderer):
    from dxrs_amd.types import NRD_DENOISE_TEXTURES, PtNrdDenoiseTextures, PtNrdReblurSettings
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    lib.pt_last_error.restype = C.c_char_p
    w, h = 64, 32
    n = w * h
    bufs = {k: torch.zeros(n * 4 + 8, dtype=torch.float32, device="cuda") for k in NRD_DENOISE_TEXTURES}
    p = {k: b.data_ptr() for k, b in bufs.items()}

    def call(size=(w, h), acc=2, pad=(0, 0, 0), expect=None, settings=None, **over):
        s = PtNrdReblurSettings(RenderSize=(C.c_uint32 * 2)(*size), AccumulationMode=acc, _pad=(C.c_uint32 * 3)(*pad), **(settings or {}))
        t = PtNrdDenoiseTextures(**{name: C.c_void_p(over.get(name, p[name])) for name in NRD_DENOISE_TEXTURES})
        st = lib.pt_nrd_reblur(ctx, C.byref(s), C.byref(t))
        if expect is not None:
            assert st == 1 and expect in lib.pt_last_error(ctx).decode(), (expect, st, lib.pt_last_error(ctx))
        return st

    assert lib.pt_nrd_reblur(None, None, None) == 1
    s = PtNrdReblurSettings(RenderSize=(C.c_uint32 * 2)(w, h))
    assert lib.pt_nrd_reblur(ctx, None, C.byref(PtNrdDenoiseTextures())) == 1 and b"null pointer" in lib.pt_last_error(ctx)
    assert lib.pt_nrd_reblur(ctx, C.byref(s), None) == 1
    call(acc=3, expect="AccumulationMode")
    call(acc=99, expect="AccumulationMode")
    for size in ((0, h), (w, 0), (16385, 1), (1, 16385)):
        call(size=size, expect="RenderSize")
    call(settings=dict(MaxFastAccumulatedFrames=31), expect="MaxFastAccumulatedFrames")  # above the default 30
    call(settings=dict(MaxAccumulatedFrames=4), expect="MaxFastAccumulatedFrames")       # the default 6 above 4
    assert call(settings=dict(MaxAccumulatedFrames=4, MaxFastAccumulatedFrames=4)) == 0
    for bad in (float("nan"), float("inf"), -1.0):
        call(settings=dict(MinBlurRadius=bad), expect="MinBlurRadius")
        call(settings=dict(MaxBlurRadius=bad), expect="MaxBlurRadius")
    call(settings=dict(MinBlurRadius=31.0), expect="MinBlurRadius must be at most MaxBlurRadius")  # above the default 30
    call(settings=dict(MinBlurRadius=2.0, MaxBlurRadius=1.5), expect="MinBlurRadius must be at most MaxBlurRadius")
    call(settings=dict(MaxBlurRadius=64.5), expect="at most 64")
    assert call(settings=dict(MinBlurRadius=64.0, MaxBlurRadius=64.0)) == 0
    for k in range(3):
        call(pad=tuple(1 if j == k else 0 for j in range(3)), expect="padding")
    for name in NRD_DENOISE_TEXTURES:
        if name != "BaseColorMetalness":
            call(**{name: None}, expect=name)
    assert call(BaseColorMetalness=None) == 0
    for name in ("NormalRoughness", "BaseColorMetalness", "InDiffuse", "InSpecular", "OutDiffuse", "OutSpecular"):
        call(**{name: p[name] + 8}, expect=name)
    for name in ("ViewZ", "MotionVector"):
        call(**{name: p[name] + 2}, expect=name)
        assert call(**{name: p[name] + 4}) == 0, name
    for name in ("ViewZ", "MotionVector", "NormalRoughness", "BaseColorMetalness", "InDiffuse", "InSpecular", "OutSpecular"):
        call(OutDiffuse=p[name], expect="OutDiffuse")
    two = torch.zeros(2 * n * 4, dtype=torch.float32, device="cuda")
    assert call(InDiffuse=two.data_ptr(), OutSpecular=two.data_ptr() + 16 * (n - 1)) == 1
    assert call(InDiffuse=two.data_ptr(), OutSpecular=two.data_ptr() + 16 * n) == 0
    assert call(InDiffuse=p["InSpecular"]) == 0  # two inputs may share a buffer
    assert call() == 0
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """dxrs::NRD (host/NRD.hpp) with its ReBLUR opt-in from C++, against pt_api.h alone: three frames of the demo scene through pack,
    NRD::Denoise (-> pt_nrd_reblur) and compose equal the Python chain's"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_nrd_reblur")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_nrd_reblur.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h, frames = 160, 90, 3
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    outp = str(tmp_path / "rb.f32")
    res = subprocess.run([exe, str(w), str(h), str(frames), outp], capture_output=True, text=True, timeout=300)
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
                den = r.nrd_reblur_denoiser()
            x = r.nrd_chain(REBLUR, denoise=den)
            bits_equal(raw[f], x["Radiance"], f"C++ frame {f}: radiance")
    finally:
        r.close()
