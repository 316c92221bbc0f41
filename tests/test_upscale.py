"""Row N11 -- the super-resolution stand-in (pt_upscale: XeSS::Execute as App::ProcessXeSSSuperResolution drives it; DESIGN.md spec S17).
CPU: the product's header (csrc/pt_upscale.h compiled as host C++ by tests/hostshim/upscale_host.cpp) against the float64 numpy
restatement (tests/upscale_reference.py), the spec's properties (identity, a constant image, the history weight, disocclusion, history
leaving the frame), the quality of 32 jittered frames against an analytic pattern, pt_upscale_input_size against a table worked by hand.
GPU: pt_upscale against the host-compiled header bit for bit (random sequences with motion, the restart rules, the real half-size chain
of a resting, travelling and animated camera), frames in flight, argument errors, the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import upscale_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENTINEL = np.uint32(0x7FC0BEEF).view(np.float32)  # a NaN with a payload: survives exactly where nothing is written
GUARD = 64  # float4 texels either side of Output that a call must leave alone
# The header (fp32) against the float64 restatement.  The history's t-space colour (scale 1) and weight (scale MaxHistoryWeight): the
# position p = (o + 0.5) (w / W) carries two fp32 roundings, 1.2e-7 p at most, that the tap offsets d inherit; the Lanczos weights have a
# slope of about 1 per input pixel and the coverage one of W / w, so both move by up to 1.2e-7 max(W, H): the tolerance is T_RTOL times
# the output's larger extent.  Largest errors seen over the sequences below, per unit of that extent: colour 8.8e-8, weight 2.8e-8.
# The output, relative to the frame's largest finite value: the inverse c = t / (1 - max t) multiplies a t-space error by (1 + c)^2, and
# the frames hold +inf, sanitised to 65504, so an fp32 rounding of t (3e-8 at best) alone is 3e-8 * 65505 = 2e-3 of that scale at the
# brightest pixels.  Largest seen: 4.7e-4.
T_RTOL = 3e-7
OUT_RTOL = 2e-3
# a discrete decision of the spec may go the other way in fp32 where the float64 margin is below the tolerance; seen: 0 pixels
FLIP_SHARE = 1e-3
# Quality on the analytic pattern (QUALITY_*): RMSE against the pattern at output resolution.  Seen on the CPU: bilinear upsample of
# frame 31 alone 0.03566, upscaled frame 0 0.00983, upscaled frame 31 0.00696: ratios 0.1952 to bilinear, 0.7081 to frame 0 (the pattern
# is smooth enough for one frame's Lanczos resample to do well; the clamp to the current taps' range bounds what the history adds).
# Each bound is the ratio plus a tenth of its gap to 1.
QUALITY_IN, QUALITY_OUT, QUALITY_FRAMES = (96, 64), (192, 128), 32
QUALITY_RATIO_BILINEAR = 0.276
QUALITY_RATIO_FRAME0 = 0.738


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_upscale_shim())
    lib.up_host_frame.restype = None
    lib.up_host_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.up_host_frame_tiled.restype = C.c_uint32
    lib.up_host_frame_tiled.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.up_host_max_extent.restype = C.c_uint32
    lib.up_host_max_extent.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.up_host_tile_w.restype = lib.up_host_tile_h.restype = C.c_uint32
    lib.up_host_lanczos.restype = C.c_float
    lib.up_host_lanczos.argtypes = [C.c_float]
    return lib


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class HostUpscaler:
    """pt_upscale on the host-compiled header, with the history logic of pt_api_post.hip: the first call, Reset and a change of either size
    restart; two history slots alternate, re-made when the output size changes."""

    def __init__(self, shim, tiled=False):
        self.shim, self.key, self.slots, self.cur, self.restarted, self.tiled = shim, None, None, 0, None, tiled

    def __call__(self, color, depth, velocity, out_size, jitter=(0.0, 0.0), reset=False, max_a=0.0):
        color, depth, velocity = c32(color), c32(depth), c32(velocity)
        h, w = depth.shape[:2]
        W, H = out_size
        restart = bool(reset) or self.key is None or self.key[:2] != (w, h)
        if self.key is None or self.key[2:] != (W, H):
            self.slots = [(np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)) for _ in range(2)]
            restart = True
        self.key = (w, h, W, H)
        prev, cur = self.slots[self.cur], self.slots[self.cur ^ 1]
        out = np.full((H, W, 4), SENTINEL, np.float32)
        size = np.array([w, h, W, H], np.uint32)
        fprm = np.array([jitter[0], jitter[1], max_a or 16.0], np.float32)
        ptrs = (C.c_void_p * 8)(*[a.ctypes.data for a in (color, depth, velocity, out, prev[0], prev[1], cur[0], cur[1])])
        if self.tiled:  # the kernel's workgroup tiles: every tap must lie inside the staged footprint
            assert self.shim.up_host_frame_tiled(size.ctypes.data, fprm.ctypes.data, 1 if restart else 0, ptrs) == 0
        else:
            self.shim.up_host_frame(size.ctypes.data, fprm.ctypes.data, 1 if restart else 0, ptrs)
        self.cur ^= 1
        self.restarted = restart
        return out

    def history(self):
        """the slot the last call wrote: (hist (H, W, 4), z (H, W))"""
        return self.slots[self.cur]


def random_frame(rng, w, h, depth=None, miss=0.1):
    """an HDR image over six decades with NaN, +-inf and negative channels; a tilted plane with a raised block and misses (kept from
    frame to frame, so most of the history survives); sub-pixel motion, a few pixels moving far"""
    rgb = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 3))).astype(np.float32)
    for value, share in ((np.nan, 0.01), (np.inf, 0.01), (-np.inf, 0.005), (-1.5, 0.02)):
        rgb[rng.random((h, w, 3)) < share] = value
    color = np.concatenate([rgb, rng.uniform(0.0, 1.0, (h, w, 1)).astype(np.float32)], axis=-1)
    if depth is None:
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
        depth = (5.0 + 0.02 * xs + 0.01 * ys).astype(np.float32)
        depth[h // 3:h // 2 + 1, w // 4:w // 2 + 1] -= 2.0
        depth[rng.random((h, w)) < miss] = np.inf
    mv = rng.uniform(-0.9, 0.9, (h, w, 3)).astype(np.float32)
    mv[..., 2] *= 0.05
    mv[rng.random((h, w)) < 0.03, :2] = 40.0
    return color, depth, mv


def jitter_of(k):
    """frame k's Settings.Jitter: minus the camera's Halton (2, 3) offset in [-0.5, 0.5)"""
    return (-(ref.halton(k % 32 + 1, 2) - 0.5), -(ref.halton(k % 32 + 1, 3) - 0.5))


def finite_max(a):
    a = np.asarray(a, np.float64)
    return float(np.abs(a[np.isfinite(a)]).max())


# ------------------------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("sizes,seed", [(((41, 29), (64, 47)), 0), (((67, 45), (200, 135)), 1)])
def test_header_matches_numpy_restatement(shim, sizes, seed):
    """4-frame sequences; every frame of the header against the restatement fed the header's own previous history slot"""
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(seed)
    up = HostUpscaler(shim)
    depth = None
    worst = dict(t=0.0, a=0.0, out=0.0)
    flips = total = 0
    for f in range(4):
        color, depth, mv = random_frame(rng, w, h, depth)
        prev = None if f == 0 else tuple(a.copy() for a in up.history())
        jit = jitter_of(f)
        out = up(color, depth, mv, (W, H), jitter=jit, max_a=3.0)
        assert up.restarted == (f == 0)
        want = ref.upscale(color, depth, mv, prev, (W, H), jit, 3.0)
        hist, z = up.history()
        scale = finite_max(want["out"][..., :3])
        err_t = np.abs(hist[..., :3] - want["hist"][..., :3]).max(axis=-1)
        err_a = np.abs(hist[..., 3] - want["hist"][..., 3]) / 3.0
        err_o = np.abs(out[..., :3] - want["out"][..., :3]).max(axis=-1) / scale
        tol = T_RTOL * max(W, H)
        bad = (err_t > tol) | (err_a > tol) | (err_o > OUT_RTOL)
        flipped = bad & (want["margin"] < tol)
        assert not (bad & ~flipped).any(), (f, np.argwhere(bad & ~flipped)[:4].tolist(), err_t.max(), err_a.max(), err_o.max())
        ok = ~bad
        worst = dict(t=max(worst["t"], err_t[ok].max() / max(W, H)), a=max(worst["a"], err_a[ok].max() / max(W, H)), out=max(worst["out"], err_o[ok].max()))
        flips += int(flipped.sum())
        total += bad.size
        assert np.array_equal(z.view(np.uint32), want["z"].astype(np.float32).view(np.uint32))  # the nearest depth is a selection: exact
        assert np.array_equal(out[..., 3].view(np.uint32), want["out"][..., 3].astype(np.float32).view(np.uint32))  # alpha is copied
        assert np.isfinite(out).all()
        if f:
            assert 0.5 < want["accepted"].mean() < 0.99  # both branches of step 5 are taken
    print(f"{w}x{h} -> {W}x{H}: worst t {worst['t']:.3g} weight {worst['a']:.3g} out {worst['out']:.3g}, {flips} of {total} pixels flipped")
    assert flips <= FLIP_SHARE * total


@pytest.mark.parametrize("sizes", [((1, 1), (1, 1)), ((1, 1), (4, 4)), ((41, 29), (41, 29)), ((41, 29), (64, 47)), ((67, 45), (200, 135)),
                                   ((33, 9), (129, 33)), ((255, 31), (256, 32)), ((1000, 3), (1001, 9))])
def test_workgroup_tiles_hold_every_tap(shim, sizes):
    """the kernel's staging, run on the host: per 32 x 8 block the footprint of up_footprint in a kUpTileW x kUpTileH tile holds every
    tap of the block's lanes (native size, ragged edges, the 4x limit, ratios just above 1), and the frames equal the whole-image path"""
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(w + 7 * W)
    whole, tiled = HostUpscaler(shim), HostUpscaler(shim, tiled=True)
    depth = None
    for f in range(2):
        color, depth, mv = random_frame(rng, w, h, depth)
        a = whole(color, depth, mv, (W, H), jitter=jitter_of(f))
        b = tiled(color, depth, mv, (W, H), jitter=jitter_of(f))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
        for x, y in zip(whole.history(), tiled.history()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f


def test_tile_bound_at_the_largest_sizes(shim):
    """16383 -> 16384 on one axis (the ratio closest to 1 from below, where the fp32 product rounds coarsest): one row of blocks of each
    orientation"""
    for (w, h), (W, H) in (((16383, 2), (16384, 8)), ((2, 16383), (8, 16384))):
        color = np.ones((h, w, 4), np.float32)
        tiled = HostUpscaler(shim, tiled=True)
        tiled(color, np.full((h, w), 2.0, np.float32), np.zeros((h, w, 3), np.float32), (W, H), jitter=(0.3, -0.4))


def test_footprint_bound_over_a_sweep_of_ratios(shim):
    """The footprint a block's taps need (up_footprint_extent, before the kernel bounds it by the tile) stays within the tile of 34 x 10
    input pixels: every pair 1 <= n_in <= n_out <= 4 n_in up to 160 output pixels, every input size of the output sizes around the powers
    of two and the usual frame sizes, the 64 ratios closest to 1 at each of the 64 largest output sizes (where the fp32 product rounds
    coarsest), and random pairs.  The bound is reached, so the tile is no larger than it has to be."""
    tile = {32: shim.up_host_tile_w(), 8: shim.up_host_tile_h()}
    assert tile == {32: 34, 8: 10}
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
            e = shim.up_host_max_extent(n, N, block)
            assert e <= tile[block], (n, N, block, e)
            widest[block] = max(widest[block], e)
    assert widest == tile


def test_lanczos_polynomial(shim):
    assert shim.up_host_lanczos(0.0) == 1.0
    assert abs(shim.up_host_lanczos(1.0)) < 1e-7 and shim.up_host_lanczos(4.0) == 0.0 and shim.up_host_lanczos(9.0) == 0.0
    for x in (0.25, 0.5, 1.5, 1.9):
        want = np.sinc(x) * np.sinc(x / 2)  # FSR2's polynomial approximates the Lanczos-2 window
        assert abs(shim.up_host_lanczos(np.float32(x * x)) - want) < 0.05
        assert abs(shim.up_host_lanczos(np.float32(x * x)) - float(ref.lanczos(x * x))) < 1e-6


def test_identity_at_native_size(shim):
    """1:1, Jitter = 0, Reset: the sanitised input to rounding (relative to the image's largest value), alpha bit for bit"""
    rng = np.random.default_rng(2)
    w, h = 37, 23
    color = np.concatenate([rng.uniform(0.0, 1.0, (h, w, 3)), rng.uniform(-2.0, 2.0, (h, w, 1))], axis=-1).astype(np.float32)
    color[3, 5, 0], color[7, 2, 1], color[9, 9, 2] = np.nan, -0.25, -np.inf
    depth = np.full((h, w), 4.0, np.float32)
    out = HostUpscaler(shim)(color, depth, np.zeros((h, w, 3), np.float32), (w, h), reset=True)
    want = ref.sanitize(color[..., :3])
    assert want[3, 5, 0] == 0 and want[7, 2, 1] == 0 and want[9, 9, 2] == 0
    err = np.abs(out[..., :3] - want).max() / want.max()
    print(f"identity: {err:.3g}")
    assert err <= 1e-6
    assert np.array_equal(out[..., 3].view(np.uint32), color[..., 3].view(np.uint32))


@pytest.mark.parametrize("out_size", [(24, 16), (36, 24), (48, 32), (72, 48)])
def test_constant_image_stays_constant(shim, out_size):
    w, h = 24, 16
    color = np.empty((h, w, 4), np.float32)
    color[...] = (0.5, 0.25, 2.0, 0.75)
    depth, mv = np.full((h, w), 4.0, np.float32), np.zeros((h, w, 3), np.float32)
    up = HostUpscaler(shim)
    for f in range(8):
        out = up(color, depth, mv, out_size, jitter=jitter_of(f))
        assert np.abs(out / np.float32([0.5, 0.25, 2.0, 0.75]) - 1.0).max() <= 1e-6, f


def test_history_weight_at_rest_and_restarts(shim):
    w, h, W, H = 16, 12, 32, 24
    rng = np.random.default_rng(4)
    depth, mv = np.full((h, w), 4.0, np.float32), np.zeros((h, w, 3), np.float32)
    up = HostUpscaler(shim)
    total = np.zeros((H, W))
    for f in range(12):
        color = rng.uniform(0.1, 1.0, (h, w, 4)).astype(np.float32)
        jit = jitter_of(f)
        up(color, depth, mv, (W, H), jitter=jit, max_a=2.0)
        kappa = ref.upscale(color, depth, mv, None, (W, H), jit)["kappa"]
        total = np.minimum(total + kappa, 2.0)  # A grows by kappa per frame and stops at MaxHistoryWeight
        assert np.abs(up.history()[0][..., 3] - total).max() <= (f + 1) * T_RTOL * max(W, H), f  # (kappa's rounding: see T_RTOL)
    assert (total == 2.0).mean() > 0.5 and kappa.min() >= 1 / 16 and kappa.max() <= 1
    color = rng.uniform(0.1, 1.0, (h, w, 4)).astype(np.float32)
    kappa0 = ref.upscale(color, depth, mv, None, (W, H))["kappa"]
    up(color, depth, mv, (W, H))
    assert not up.restarted and (up.history()[0][..., 3] > kappa0 + 0.01).all()
    up(color, depth, mv, (W, H), reset=True)
    assert up.restarted and np.abs(up.history()[0][..., 3] - kappa0).max() <= 1e-6
    up(color, depth, mv, (W, H))
    assert not up.restarted
    for size_in, size_out in (((16, 12), (48, 36)), ((12, 9), (48, 36))):  # the output size changes, then the input size
        ww, hh = size_in
        args = (rng.uniform(0.1, 1.0, (hh, ww, 4)).astype(np.float32), np.full((hh, ww), 4.0, np.float32), np.zeros((hh, ww, 3), np.float32))
        up(*args, size_out)
        assert up.restarted
        assert np.abs(up.history()[0][..., 3] - ref.upscale(*args, None, size_out)["kappa"]).max() <= 1e-6
        up(*args, size_out)
        assert not up.restarted


def step_scene(w, h, a, b):
    """a foreground block (depth 5) over columns [a, b) and the middle rows of a background (depth 10)"""
    depth = np.full((h, w), 10.0, np.float32)
    depth[4:h - 4, a:b] = 5.0
    color = np.empty((h, w, 4), np.float32)
    color[...] = (0.2, 0.3, 0.4, 1.0)
    color[depth < 6.0] = (1.0, 0.8, 0.6, 1.0)
    return color, depth


def test_depth_step_restarts_exactly_the_disoccluded_pixels(shim):
    """a block that moves 3 input pixels to the right: the background it uncovers has no history, everything else keeps its own"""
    w, h, W, H = 40, 24, 80, 48
    a, b = 10, 20
    up = HostUpscaler(shim)
    c0, z0 = step_scene(w, h, a, b)
    up(c0, z0, np.zeros((h, w, 3), np.float32), (W, H))
    prev = tuple(x.copy() for x in up.history())
    c1, z1 = step_scene(w, h, a + 3, b + 3)
    mv = np.zeros((h, w, 3), np.float32)
    mv[z1 < 6.0, 0] = -3.0  # previous - current, in input pixels
    up(c1, z1, mv, (W, H))
    want = ref.upscale(c1, z1, mv, prev, (W, H))
    restarted = np.abs(up.history()[0][..., 3] - want["kappa"]) <= 1e-6  # A = kappa; with history it is twice that here
    assert np.array_equal(restarted, ~want["accepted"])
    ys, xs = np.nonzero(restarted)
    assert len(xs) >= 6 * 2 * (h - 8) - 4 * 6  # the three uncovered input columns, bar the corners the dilated depth keeps
    assert xs.min() >= 2 * a - 2 and xs.max() < 2 * (a + 3) + 2 and ys.min() >= 2 * 4 - 2 and ys.max() < 2 * (h - 4) + 2
    assert np.abs(up.history()[0][..., 3][~restarted] - 2 * want["kappa"][~restarted]).max() <= 1e-6


def test_history_leaving_the_frame_restarts_and_misses_keep_theirs(shim):
    w, h, W, H = 20, 12, 40, 24
    rng = np.random.default_rng(5)
    color = rng.uniform(0.1, 1.0, (h, w, 4)).astype(np.float32)
    depth = np.full((h, w), np.inf, np.float32)  # all misses: both depths infinite passes the depth test
    depth[:, : w // 2] = 3.0
    still = np.zeros((h, w, 3), np.float32)
    up = HostUpscaler(shim)
    up(color, depth, still, (W, H))
    kappa = ref.upscale(color, depth, still, None, (W, H))["kappa"]
    up(color, depth, still, (W, H))
    assert np.abs(up.history()[0][..., 3] - 2 * kappa).max() <= 1e-6  # hits and miss-to-miss pixels both keep their history
    mv = still.copy()
    mv[..., 0] = -4.0  # the previous position is 8 output pixels to the left: columns 0..7 come from outside the frame
    up(color, depth, mv, (W, H))
    a = up.history()[0][..., 3]
    assert np.abs(a[:, :8] - kappa[:, :8]).max() <= 1e-6
    assert (a[:, 8:W // 2 - 2] > kappa[:, 8:W // 2 - 2] + 0.01).all()
    nan_mv = still.copy()
    nan_mv[2, 3, 0] = np.nan  # q is not inside anything
    up(color, depth, nan_mv, (W, H))
    assert np.isfinite(up.history()[0]).all()


def pattern(x, y, size):
    """slanted soft edges plus a zone plate whose local frequency stays below 0.18 cycles per output pixel (the input's Nyquist rate at
    2x is 0.25), at output-pixel coordinates (x, y)"""
    W, H = size
    r2 = (x - 0.35 * W) ** 2 + (y - 0.4 * H) ** 2
    k = 0.18 / (2.0 * np.hypot(W, H))  # phase pi k r^2: frequency k r <= 0.18 over the frame
    zone = 0.5 + 0.5 * np.cos(np.pi * k * r2 * 2.0)
    edge1 = 0.5 + 0.5 * np.tanh(((x - 0.6 * W) * np.cos(0.3) + (y - 0.5 * H) * np.sin(0.3)) / 1.5)
    edge2 = 0.5 + 0.5 * np.tanh(((x - 0.2 * W) * np.sin(0.2) - (y - 0.7 * H) * np.cos(0.2)) / 1.5)
    return 0.05 + 0.5 * zone * (1.0 - 0.6 * edge1) + 0.4 * edge1 * edge2


def test_quality_of_jittered_accumulation(shim):
    (w, h), (W, H) = QUALITY_IN, QUALITY_OUT
    oy, ox = np.mgrid[0:H, 0:W]
    truth = pattern(ox + 0.5, oy + 0.5, (W, H))
    iy, ix = np.mgrid[0:h, 0:w]
    depth, mv = np.full((h, w), 5.0, np.float32), np.zeros((h, w, 3), np.float32)
    up = HostUpscaler(shim)
    errs = []
    for f in range(QUALITY_FRAMES):
        jit = jitter_of(f)
        v = pattern((ix + 0.5 - jit[0]) * 2.0, (iy + 0.5 - jit[1]) * 2.0, (W, H))  # point samples at i + 0.5 - Jitter
        color = np.stack([v, v, v, np.ones_like(v)], axis=-1).astype(np.float32)
        out = up(color, depth, mv, (W, H), jitter=jit, max_a=32.0)
        errs.append(float(np.sqrt(((out[..., 0] - truth) ** 2).mean())))
    bil = ref.bilinear_upsample(color, (W, H))[..., 0]
    e_bil = float(np.sqrt(((bil - truth) ** 2).mean()))
    print(f"quality: bilinear {e_bil:.5f} frame 0 {errs[0]:.5f} frame 31 {errs[-1]:.5f}: ratios {errs[-1] / e_bil:.4f} {errs[-1] / errs[0]:.4f}")
    assert errs[-1] < QUALITY_RATIO_BILINEAR * e_bil, (e_bil, errs)
    assert errs[-1] < QUALITY_RATIO_FRAME0 * errs[0], errs


# (mode 1..5 -> input size) per output size: w = max(1, (W * 10 + r10 / 2) / r10) with r10 = 10, 15, 17, 20, 30, by hand:
# e.g. 1920 at 17: 19208 / 17 = 1129.88 -> 1129; 1080 at 17: 10808 / 17 = 635.76 -> 635; 1280 at 30: 12815 / 30 = 427.17 -> 427
INPUT_SIZES = {
    (1280, 720): ((1280, 720), (853, 480), (753, 424), (640, 360), (427, 240)),
    (1920, 1080): ((1920, 1080), (1280, 720), (1129, 635), (960, 540), (640, 360)),
    (2560, 1440): ((2560, 1440), (1707, 960), (1506, 847), (1280, 720), (853, 480)),
    (3840, 2160): ((3840, 2160), (2560, 1440), (2259, 1271), (1920, 1080), (1280, 720)),
    (7680, 4320): ((7680, 4320), (5120, 2880), (4518, 2541), (3840, 2160), (2560, 1440)),
}
AUTO_MODE = {(1280, 720): 1, (1920, 1080): 2, (2560, 1440): 3, (3840, 2160): 4, (7680, 4320): 5}


def test_upscale_input_size(dxrs):
    hip = dxrs.load_hip()
    for out, table in INPUT_SIZES.items():
        for mode, want in enumerate(table, start=1):
            assert hip.upscale_input_size(mode, *out) == want, (out, mode)
        assert hip.upscale_input_size(0, *out) == table[AUTO_MODE[out] - 1], out
    # Auto at the edges of its pixel-count thresholds (App.cpp:1381-1394): <= is the lower mode
    for (W, H), mode in (((1280, 800), 1), ((1281, 800), 2), ((1920, 1200), 2), ((1921, 1200), 3), ((2560, 1600), 3), ((2561, 1600), 4),
                         ((3840, 2400), 4), ((3841, 2400), 5), ((1, 1), 1), ((16384, 16384), 5)):
        assert hip.upscale_input_size(0, W, H) == hip.upscale_input_size(mode, W, H), (W, H)
    assert hip.upscale_input_size(5, 1, 1) == (1, 1) and hip.upscale_input_size(5, 2, 4) == (1, 1) and hip.upscale_input_size(4, 3, 5) == (2, 3)
    lib = hip.lib
    w, h = C.c_uint32(7), C.c_uint32(7)
    for mode, W, H in ((6, 64, 64), (99, 64, 64), (1, 0, 64), (1, 64, 0)):
        assert lib.pt_upscale_input_size(mode, W, H, C.byref(w), C.byref(h)) == 1
    assert lib.pt_upscale_input_size(1, 64, 64, None, C.byref(h)) == 1 and lib.pt_upscale_input_size(1, 64, 64, C.byref(w), None) == 1
    assert (w.value, h.value) == (7, 7)


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import PtUpscaleSettings, PtUpscaleTextures
    lib = dxrs.load_hip().lib
    s = PtUpscaleSettings(InputSize=(C.c_uint32 * 2)(32, 32), OutputSize=(C.c_uint32 * 2)(64, 64))
    assert C.sizeof(PtUpscaleSettings) == 32 and C.sizeof(PtUpscaleTextures) == 32
    assert PtUpscaleSettings.Jitter.offset == 16 and PtUpscaleSettings.Reset.offset == 24 and PtUpscaleSettings.MaxHistoryWeight.offset == 28
    assert lib.pt_upscale(None, C.byref(s), C.byref(PtUpscaleTextures())) == 1
    assert lib.pt_upscale(None, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


class GpuUpscaler:
    """pt_upscale on device copies; Output starts as the sentinel and sits between two guard bands that must stay the sentinel"""

    def __init__(self, renderer):
        self.r = renderer

    def __call__(self, color, depth, velocity, out_size, jitter=(0.0, 0.0), reset=False, max_a=0.0):
        import torch
        h, w = np.asarray(depth).shape[:2]
        W, H = out_size
        d = [torch.from_numpy(c32(v)).cuda() for v in (color, depth, velocity)]
        out = torch.from_numpy(np.full((H * W + 2 * GUARD, 4), SENTINEL, np.float32)).cuda()
        torch.cuda.synchronize()
        self.r.upscale_device((w, h), (W, H), dict(Color=d[0].data_ptr(), Depth=d[1].data_ptr(), Velocity=d[2].data_ptr(),
                                                   Output=out.data_ptr() + 16 * GUARD), jitter=jitter, reset=reset, max_history_weight=max_a)
        self.r.synchronize()
        res = out.cpu().numpy()
        for band in (res[:GUARD], res[GUARD + H * W:]):
            assert np.array_equal(band.view(np.uint32), np.full(band.shape, SENTINEL).view(np.uint32)), "the guard band was written"
        return res[GUARD:GUARD + H * W].reshape(H, W, 4)


def compare_sequence(renderer, shim, frames, what):
    """the frames (color, depth, velocity, out_size, jitter, reset) through the GPU and the host header -> bit for bit"""
    gpu, host = GpuUpscaler(renderer), HostUpscaler(shim)
    for f, (color, depth, mv, out_size, jit, reset) in enumerate(frames):
        reset = True if f == 0 else reset  # (the shared context carries other tests' history)
        got = gpu(color, depth, mv, out_size, jitter=jit, reset=reset, max_a=3.0)
        want = host(color, depth, mv, out_size, jitter=jit, reset=reset, max_a=3.0)
        bits_equal(got, want, f"{what} frame {f}")
        assert not np.array_equal(got.view(np.uint32), np.full(got.shape, SENTINEL).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [((1, 1), (1, 1)), ((1, 1), (4, 4)), ((41, 29), (64, 47)), ((67, 45), (200, 135)), ((320, 180), (640, 360)),
                                   ((960, 540), (1920, 1080))])
def test_gpu_bit_exact_random_sequences(renderer, shim, sizes):
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(w + 3 * h + 5 * W)
    frames, depth = [], None
    for f in range(3 if w > 900 else 4):
        color, depth, mv = random_frame(rng, w, h, depth)
        frames.append((color, depth, mv, (W, H), jitter_of(f), False))
    compare_sequence(renderer, shim, frames, f"{w}x{h} -> {W}x{H}")


@pytest.mark.gpu
def test_gpu_restart_rules(renderer, shim):
    """Reset in the middle of a sequence, then an output-size change, then an input-size change: the GPU restarts where the host class,
    which restates pt_api_post.hip's rule, does"""
    rng = np.random.default_rng(12)
    plan = [((40, 30), (80, 60), False), ((40, 30), (80, 60), False), ((40, 30), (80, 60), True), ((40, 30), (80, 60), False),
            ((40, 30), (100, 75), False), ((40, 30), (100, 75), False), ((50, 38), (100, 75), False), ((50, 38), (100, 75), False)]
    gpu, host = GpuUpscaler(renderer), HostUpscaler(shim)
    depths, restarts = {}, []
    for f, ((w, h), out_size, reset) in enumerate(plan):
        color, depths[(w, h)], mv = random_frame(rng, w, h, depths.get((w, h)), miss=0.0)
        mv[:] = 0.0
        reset = reset or f == 0
        got = gpu(color, depths[(w, h)], mv, out_size, jitter=jitter_of(f), reset=reset)
        want = host(color, depths[(w, h)], mv, out_size, jitter=jitter_of(f), reset=reset)
        restarts.append(host.restarted)
        bits_equal(got, want, f"restart rules frame {f}")
    assert restarts == [True, False, True, False, True, False, True, False]


def real_chain(dxrs, host, renderer, shim, kind, n_frames=6, w=480, h=270, W=960, H=540):
    """n_frames of the C2 scene: half-size pt_render_gbuffer + pt_render with Halton jitter -> pt_upscale, against the host header fed
    the same device-made inputs bit for bit; then pt_bloom and pt_tonemap at output size"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    if kind == "animated":
        sd.IsStatic = 0
    renderer.set_scene(spheres, mats, sd)
    hu = HostUpscaler(shim)
    up = renderer.upscaler((W, H), mode=dxrs.types.UPSCALE_PERFORMANCE)
    assert up.input_size == (w, h)
    color = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    depth = torch.zeros((h, w, 1), dtype=torch.float32, device="cuda")
    mvb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ldr = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    prev, prev_cam = spheres.copy(), None
    for f in range(n_frames):
        moved = spheres.copy()
        previous_spheres = None
        if kind == "animated":
            moved["cy"] += np.float32(0.05 * f) * np.sin(np.arange(len(spheres), dtype=np.float32))
            renderer.update_spheres(moved)
            previous_spheres = prev
        pos = (0.0, 0.0, -15.0) if kind != "travelling" else (0.15 * f, 0.05 * f, -15.0 + 0.1 * f)
        cam = host.camera_matrices(w, h, position=pos, look_at=(0.0, 0.0, 0.0), jitter_index=f, jitter_count=32, previous=prev_cam)
        renderer.set_camera(cam)
        prev_cam = cam
        renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
        renderer.render_gbuffer_device(dict(LinearDepth=depth.data_ptr(), MotionVector=mvb.data_ptr()), previous_spheres=previous_spheres)
        renderer.render_device(color.data_ptr())
        jit = (-cam.Jitter[0], -cam.Jitter[1])
        out = up(color, depth, mvb, jitter=jit)
        renderer.synchronize()
        c, z, mv, got = color.cpu().numpy(), depth.cpu().numpy()[..., 0], mvb.cpu().numpy(), out.cpu().numpy()
        want = hu(c, z, mv, (W, H), jitter=jit)
        bits_equal(got, want, f"{kind} frame {f}")
        if kind != "resting" and f:
            assert np.abs(mv[np.isfinite(z)][:, :2]).max() > 0.1
        prev = moved
    assert abs(jit[0]) <= 0.5 and abs(jit[1]) <= 0.5 and jit != (0.0, 0.0)
    assert hu.history()[0][..., 3].max() > 1.0  # the history was used
    renderer.bloom(out.data_ptr(), out.data_ptr(), W, H, 0.1)
    renderer.tonemap(out.data_ptr(), W * H, dxrs.types.tonemap_params(), ldr.data_ptr())
    renderer.synchronize()
    assert np.isfinite(out.cpu().numpy()).all() and int(ldr.cpu().numpy().view(np.uint32).max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["resting", "travelling", "animated"])
def test_gpu_real_chain_bit_exact(dxrs, host, renderer, shim, kind):
    real_chain(dxrs, host, renderer, shim, kind)


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """three lanes and six frames of a travelling camera, G-buffer -> pt_render -> pt_upscale queued without waiting, leave the rendered
    frames bit-identical to frames rendered without pt_upscale, and the upscaled frames equal to a one-lane run's"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h, W, H = 240, 136, 480, 272
    frames = 6

    def run(r, lanes, upscale):
        sets = [dict(Color=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), Depth=torch.zeros((h, w), dtype=torch.float32, device="cuda"),
                     Velocity=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"), Output=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"))
                for _ in range(3)]
        torch.cuda.synchronize()
        r.set_scene(spheres, mats, sd)
        got = []
        for f in range(frames):
            cam = host.camera_matrices(w, h, position=(0.2 * f, 0.0, -15.0 + 0.1 * f), look_at=(0.0, 0.0, 0.0), jitter_index=f, jitter_count=32)
            r.set_camera(cam)
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
            s = sets[f % 3]
            r.render_gbuffer_device(dict(LinearDepth=s["Depth"].data_ptr(), MotionVector=s["Velocity"].data_ptr()))
            r.render_device(s["Color"].data_ptr())
            if upscale:
                r.upscale_device((w, h), (W, H), {k: v.data_ptr() for k, v in s.items()}, jitter=(-cam.Jitter[0], -cam.Jitter[1]), reset=f == 0)
            if lanes == 1 or f % 3 == 2:
                r.synchronize()
                got += [{k: v.cpu().numpy().copy() for k, v in x.items()} for x in (sets if lanes > 1 else [s])]
        r.synchronize()
        return got

    results = {}
    for name, lanes, upscale in (("many", 3, True), ("plain", 3, False), ("one", 1, True)):
        tstream = torch.cuda.Stream()
        r = dxrs.Renderer(device=0, stream=tstream.cuda_stream, frames_in_flight=lanes)
        try:
            with torch.cuda.stream(tstream):
                results[name] = run(r, lanes, upscale)
        finally:
            r.close()
    for f in range(frames):
        for k in ("Depth", "Velocity", "Color"):
            bits_equal(results["many"][f][k], results["plain"][f][k], f"frame {f}: {k} with and without pt_upscale")
        bits_equal(results["many"][f]["Output"], results["one"][f]["Output"], f"frame {f}: Output, three lanes and one")
    assert np.abs(results["one"][-1]["Output"]).max() > 0


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, renderer):
    from dxrs_amd.types import UPSCALE_TEXTURES, PtUpscaleSettings, PtUpscaleTextures
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    w, h, W, H = 32, 16, 64, 32
    bufs = {k: torch.zeros(4 * w * 4 * h * 4 + 8, dtype=torch.float32, device="cuda") for k in UPSCALE_TEXTURES}  # (room for the 4x case)
    p = {k: b.data_ptr() for k, b in bufs.items()}

    def call(size_in=(w, h), size_out=(W, H), jitter=(0.0, 0.0), max_a=0.0, **over):
        s = PtUpscaleSettings(InputSize=(C.c_uint32 * 2)(*size_in), OutputSize=(C.c_uint32 * 2)(*size_out), Jitter=(C.c_float * 2)(*jitter), Reset=1,
                              MaxHistoryWeight=max_a)
        t = PtUpscaleTextures(**{name: C.c_void_p(over.get(name, p[name])) for name in UPSCALE_TEXTURES})
        return lib.pt_upscale(ctx, C.byref(s), C.byref(t))

    s = PtUpscaleSettings(InputSize=(C.c_uint32 * 2)(w, h), OutputSize=(C.c_uint32 * 2)(W, H))
    assert lib.pt_upscale(None, None, None) == 1
    assert lib.pt_upscale(ctx, None, C.byref(PtUpscaleTextures())) == 1 and lib.pt_upscale(ctx, C.byref(s), None) == 1
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
    for name in UPSCALE_TEXTURES:
        assert call(**{name: None}) == 1, name
    for name in ("Color", "Output"):
        assert call(**{name: p[name] + 8}) == 1, name
    for name in ("Depth", "Velocity"):
        assert call(**{name: p[name] + 2}) == 1, name
        assert call(**{name: p[name] + 4}) == 0, name
    for name in ("Color", "Depth", "Velocity"):
        assert call(Output=p[name]) == 1, name
    two = torch.zeros(2 * W * H * 4, dtype=torch.float32, device="cuda")  # Color: w * h texels, then Output: W * H texels
    assert call(Color=two.data_ptr(), Output=two.data_ptr() + 16 * (w * h - 1)) == 1
    assert call(Color=two.data_ptr(), Output=two.data_ptr() + 16 * w * h) == 0
    assert call(Depth=p["Velocity"]) == 0  # two inputs may share a buffer
    assert call() == 0
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, shim, tmp_path):
    """dxrs::XeSS (host/XeSS.hpp) from C++, against pt_api.h alone: four frames of the demo scene rendered at the Performance mode's
    input size with Halton jitter, tagged and executed as App::ProcessXeSSSuperResolution does, equal the host-compiled header fed the
    inputs the program downloaded; a missing tag is refused"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_upscale")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_upscale.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    W, H, frames = 320, 180, 4
    outp = str(tmp_path / "up.f32")
    res = subprocess.run([exe, str(W), str(H), "4", str(frames), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout
    w, h = dxrs.load_hip().upscale_input_size(4, W, H)
    assert f"input {w}x{h}" in res.stdout
    raw = np.fromfile(outp, dtype=np.float32)
    per = 2 + w * h * 8 + W * H * 4
    assert raw.size == frames * per
    hu = HostUpscaler(shim)
    for f in range(frames):
        x = raw[f * per:(f + 1) * per]
        jit = (float(x[0]), float(x[1]))
        color, depth, mv = x[2:2 + w * h * 4].reshape(h, w, 4), x[2 + w * h * 4:2 + w * h * 5].reshape(h, w), x[2 + w * h * 5:2 + w * h * 8].reshape(h, w, 3)
        bits_equal(x[2 + w * h * 8:].reshape(H, W, 4), hu(color, depth, mv, (W, H), jitter=jit), f"C++ frame {f}")
        assert jit != (0.0, 0.0)
    assert hu.history()[0][..., 3].max() > 1.0
