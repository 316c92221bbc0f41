"""Row N19 -- the radiance cache's anti-firefly filter (IsAntiFireflyEnabled through pt_render_sharc_ex, DESIGN.md spec S25).
CPU: the host-compiled header (tests/hostshim/sharc_ff_host.cpp over csrc/pt_sharc.h): the resolve's clamp against known answers and a
float64 restatement of S25; the update's weight threshold on hand-built states; the filter off against the existing shim; the filter's
effect on a scene with fireflies; a sanitizer build of a stand-alone program; the ABI.
GPU: the kernels against the host header word for word with the filter on; the smallest shapes; the flag switched between calls; the
default-frame chain queued and synchronised; the argument rules; the C++ mirror."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import sharc_reference as ref
from test_restir_pass import make_scene
from test_sharc import CAP, GH, GW, QUERY, RESOLVE, UPDATE, H, W, c1, cache_map, defaults, gpu_content, p, same_bits, setup, voxel_w
from test_sharc import cpu_scene, shims  # noqa: F401  (fixtures)
from test_sharc_ex import OUTPUTS, SENTINEL, HostCacheEx, bits, c1_cpu, gpu_call, is_sentinel, random_di
from test_sharc_ex import ex_lib  # noqa: F401  (a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24  # the unit roundoff of float32
MIN_SAMPLES, MIN_FRAMES, FLOOR, WEIGHT_THRESHOLD = 8, 2, 1.0, 2.0  # S25's constants, restated
LUM32 = np.array([0.2126, 0.7152, 0.0722], np.float32)
LUM = LUM32.astype(np.float64)  # (the float32 constants exactly: the restatement differs from the header by rounding of operations only)


# ---------------------------------------------------------------------------------------------------- the host-compiled header
@pytest.fixture(scope="module")
def ff_lib():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_sharc_ff_shim())
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    for name, args in dict(sh_host_call_ff=[vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp],
                           sh_host_resolve_ff=[vp, vp, u32, u32, u32, vp, vp, vp, vp], sh_host_luminance=[vp, u32, vp],
                           sh_host_propagate=[vp, vp, u32, u32, vp, vp, vp, u32, u32, vp, vp],
                           sh_host_update_hit=[vp, vp, vp, u32, vp, f32, vp, vp, u32, vp, vp, vp, f32, u32, vp, vp]).items():
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    return lib


class HostCacheFf(HostCacheEx):
    """pt_render_sharc_ex with IsAntiFireflyEnabled over the host-compiled header: HostCacheEx with the flag of a call, and the two
    statistics the host keeps (slots the resolve clamped, walks the weight threshold stopped), summed over the calls"""

    def __init__(self, ff, ex, lib, gbshim, spheres, mats, sd, textures=None):
        super().__init__(ex, lib, gbshim, spheres, mats, sd, textures)
        self.ff = ff
        self.clamped = self.stopped = 0

    def call_ff(self, cam, gs, rect=None, di=None, mode=0, **kw):
        """-> (image (h, w, 4) or None, {output: array}, rays, failed inserts); anti_firefly among the settings"""
        s = defaults(**kw)
        stages = s["stages"] or 7
        w, h = gs.RenderSize[0], gs.RenderSize[1]
        rect = rect or (0, 0, w, h)
        if self.capacity != s["capacity"]:
            self.capacity, self.valid = s["capacity"], False
            self.keys = np.zeros(self.capacity, np.uint64)
            self.accum, self.resolved = np.zeros((self.capacity, 4), np.uint32), np.zeros((self.capacity, 4), np.uint32)
        if s["reset_history"] or not self.valid:
            self.keys[:] = 0
            self.accum[:] = 0
            self.resolved[:] = 0
        self.valid = True
        prm = np.array([w, h, gs.FrameIndex, gs.Bounces, gs.SamplesPerPixel, gs.IsRussianRouletteEnabled, s["capacity"], s["downscale_factor"],
                        s["accumulation_frames"], s["max_stale_frames"], int(s["visualize"]), stages, *rect], np.uint32)
        fprm = np.array([gs.ThroughputThreshold, s["scene_scale"], s["roughness_threshold"]], np.float32)
        out = np.full((rect[3], rect[2], 4), SENTINEL, np.float32)
        dd, ds = (np.ascontiguousarray(a, dtype=np.float32).copy() for a in di) if di is not None else (None, None)
        bufs = {name: np.full((rect[3], rect[2], width), SENTINEL, np.float32) for name, width in OUTPUTS.get(mode, ())}
        counters, ffc = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        self.ff.sh_host_call_ff(p(self.spheres), p(self.mats), len(self.spheres), p(self.env), p(self.texels), p(self.info), 0 if self.info is None else len(self.info),
                                p(self.maps), p(self.rot), C.addressof(cam), p(prm), p(fprm), p(self.keys), p(self.accum), p(self.resolved), p(out), p(counters),
                                p(dd), p(ds), mode, p(bufs.get("SpecularHitDistance")), p(bufs.get("Diffuse")), p(bufs.get("Specular")),
                                1 if s.get("anti_firefly") else 0, p(ffc))
        if stages & RESOLVE:
            self.accum, self.resolved = self.resolved, self.accum
        self.clamped += int(ffc[0])
        self.stopped += int(ffc[1])
        return (out if stages & QUERY else None), bufs, int(counters[0]), int(counters[1])


def resolve_ff(ff_lib, acc, prev, A=10, M=64):
    """-> (resolved voxels, clear, the accumulators behind the clamp, clamped) of n voxels"""
    acc, prev = np.ascontiguousarray(acc, np.uint32).reshape(-1, 4), np.ascontiguousarray(prev, np.uint32).reshape(-1, 4)
    n = len(acc)
    out, clear, ca, cl = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
    ff_lib.sh_host_resolve_ff(p(acc), p(prev), n, A, M, p(out), p(clear), p(ca), p(cl))
    return out, clear, ca, cl


def resolve_plain(lib, acc, prev, A=10, M=64):
    acc, prev = np.ascontiguousarray(acc, np.uint32).reshape(-1, 4), np.ascontiguousarray(prev, np.uint32).reshape(-1, 4)
    n = len(acc)
    out, clear = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
    lib.sh_host_resolve(p(acc), p(prev), n, A, M, p(out), p(clear))
    return out, clear


def lum64(sums, n):
    """Y of the mean of integer sums, in float64 with S25's float32 coefficients"""
    return (np.asarray(sums, np.float64) @ LUM) / (np.asarray(n, np.float64) * ref.RADIANCE_SCALE)


def random_voxels(rng, n, history):
    """n (acc, prev) pairs.  acc: sums over the whole 32-bit range (a tenth saturated or nearly), counts up to 2^20 (beyond the 16 bits of
    a resolved voxel), a fifth without samples.  history: 'none' (prev = 0), 'short' (below either minimum), 'long' (both reached)"""
    acc = np.zeros((n, 4), np.uint32)
    acc[:, :3] = (2.0 ** rng.uniform(0, 32, (n, 3))).astype(np.uint64).clip(0, 0xFFFFFFFF).astype(np.uint32)
    sat = rng.random(n) < 0.1
    acc[sat, :3] = 0xFFFFFFFF - rng.integers(0, 3, (int(sat.sum()), 3)).astype(np.uint32)
    acc[:, 3] = (2.0 ** rng.uniform(0, 20, n)).astype(np.uint32)
    acc[rng.random(n) < 0.2, 3] = 0
    prev = np.zeros((n, 4), np.uint32)
    if history != "none":
        prev[:, :3] = (2.0 ** rng.uniform(0, 32, (n, 3))).astype(np.uint64).clip(0, 0xFFFFFFFF).astype(np.uint32)
        if history == "short":
            few = rng.random(n) < 0.5  # too few samples with any frame count, or enough samples in too few frames
            samples = np.where(few, rng.integers(0, MIN_SAMPLES, n), rng.integers(MIN_SAMPLES, 65536, n))
            frames = np.where(few, rng.integers(0, 256, n), rng.integers(0, MIN_FRAMES, n))
        else:
            samples = np.where(rng.random(n) < 0.3, rng.integers(MIN_SAMPLES, 64, n), rng.integers(MIN_SAMPLES, 65536, n))
            frames = rng.integers(MIN_FRAMES, 256, n)
        prev[:, 3] = samples.astype(np.uint32) | (frames.astype(np.uint32) << 16) | (rng.integers(0, 6, n).astype(np.uint32) << 24)
    return acc, prev


# ---------------------------------------------------------------------------------------------------- CPU 1: ABI
def test_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert hasattr(lib, "pt_render_sharc_ex") and "pt_render_sharc_ex" in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtSharcSettings
    assert C.sizeof(PtSharcSettings) == 48 and PtSharcSettings.IsAntiFireflyEnabled.offset == 24 and PtSharcSettings.IsHashGridVisualizationEnabled.offset == 28
    assert PtSharcSettings.SceneScale.offset == 8 and PtSharcSettings.AccumulationFrames.offset == 16 and PtSharcSettings.ResetHistory.offset == 32
    assert PtSharcSettings.Stages.offset == 36
    s = dxrs.binding.sharc_settings(anti_firefly=True)
    assert s.IsAntiFireflyEnabled == 1
    assert lib.pt_render_sharc_ex(None, None, None, 0, C.byref(s), None, None, None) == 1  # PT_ERR_INVALID_ARG: null context


# ---------------------------------------------------------------------------------------------------- CPU 2: the resolve's clamp
@pytest.mark.parametrize("history", ["none", "short"])
def test_clamp_without_history_is_sh_resolve_slot(shims, ff_lib, history):
    rng = np.random.default_rng(19)
    acc, prev = random_voxels(rng, 4000, history)
    assert (acc[:, 3] > 65535).sum() > 100 and (acc[:, :3] >= 0xFFFFFFFD).any(axis=1).sum() > 100
    for A, M in ((10, 64), (255, 254), (1, 2)):
        got, clear, ca, cl = resolve_ff(ff_lib, acc, prev, A, M)
        want, wclear = resolve_plain(shims[0], acc, prev, A, M)
        assert np.array_equal(got, want) and np.array_equal(clear, wclear) and not cl.any() and np.array_equal(ca, acc)


def test_clamp_leaves_a_voxel_without_samples_alone(shims, ff_lib):
    """n_a = 0 over any history, a stale one included: the sums (which nothing adds to without a sample; here arbitrary) pass unchanged"""
    rng = np.random.default_rng(20)
    acc, prev = random_voxels(rng, 2000, "long")
    acc[:, 3] = 0
    got, clear, ca, cl = resolve_ff(ff_lib, acc, prev)
    want, wclear = resolve_plain(shims[0], acc, prev)
    assert np.array_equal(got, want) and np.array_equal(clear, wclear) and not cl.any() and np.array_equal(ca, acc)
    assert (got[:, 3] >> 24).max() > 0, "stale histories are among them"


@pytest.mark.parametrize("radiance", [(0.02, 0.01, 0.03), (3.0, 2.0, 1.0), (200.0, 256.0, 100.0)])
def test_steady_signal_is_never_clamped(shims, ff_lib, radiance):
    """the same mean every frame, from sample counts that change: 32 resolves, the history from the filter's own output"""
    q = np.array([ref.quantise(x) for x in radiance], np.uint64)
    prev_ff = prev_plain = np.zeros((1, 4), np.uint32)
    for f in range(32):
        n = (1, 7, 3, 40, 2)[f % 5]
        acc = np.array([[*(q * n), n]], np.uint32)
        prev_ff, _, ca, cl = resolve_ff(ff_lib, acc, prev_ff)
        prev_plain, _ = resolve_plain(shims[0], acc, prev_plain)
        assert not cl[0] and np.array_equal(ca, acc), f
        assert np.array_equal(prev_ff, prev_plain)
    n_p, f_p, _ = ref.unpack_w(int(prev_ff[0, 3]))
    assert n_p >= MIN_SAMPLES and f_p == 10, "the filter was armed"


def test_spike_is_clamped_to_k_times_the_history(shims, ff_lib):
    """A history of mean (2, 2, 2) (Y_p = 2 > the floor) and one of mean (0.25, 0.25, 0.25) (Y_p = the floor 1), n_p = 40 and 8 samples, and
    a frame of n_a samples whose mean is 1000 times the history's: the clamped accumulators' mean luminance is K Y_p, K = 5 + 5 / n_p.
    Bound.  Every operand is positive, so relative errors add to first order.  Y of a mean, per term: the sum's conversion (1
    rounding), the divisor float(n) * 1024 (1: the conversion; the product with a power of two is exact), the division (1), the product
    with the coefficient (1), up to two additions (2): 6 u, u = 2^-24.  K: a division and an addition, 2 u.  limit = K * Y_p: 6 + 2 + 1 =
    9 u.  s = limit / Y_a: 9 + 6 + 1 = 16 u.  float(sum) * s: a conversion and a product, 18 u; counted as 20 u for the second-order terms.
    Truncation takes less than 1 from each sum, less than (0.2126 + 0.7152 + 0.0722) / (1024 n_a) from Y.  So
    |Y(clamped mean) - K Y_p| <= 20 u K Y_p + 1.0001 / (1024 n_a), both sides in float64 from the integer words."""
    worst = 0.0
    for mean, n_p in (((2.0, 2.0, 2.0), 40), ((0.25, 0.25, 0.25), 8), ((3.0, 0.5, 9.0), 65535)):
        for n_a in (1, 5, 300):
            q = np.array([ref.quantise(x) for x in mean], np.uint64)
            prev = np.array([[*(q * n_p).clip(0, 0xFFFFFFFF), voxel_w(n_p, 6, 0)]], np.uint32)
            acc = np.array([[*(q * 1000 * n_a).clip(0, 0xFFFFFFFF), n_a]], np.uint32)
            got, clear, ca, cl = resolve_ff(ff_lib, acc, prev)
            assert cl[0] and not clear[0]
            y_p = max(float(lum64(prev[0, :3], n_p)), FLOOR)
            k = 5.0 + 5.0 / n_p
            y = float(lum64(ca[0, :3], n_a))
            bound = 20 * U * k * y_p + 1.0001 / (1024.0 * n_a)
            worst = max(worst, abs(y - k * y_p) / bound)
            assert abs(y - k * y_p) <= bound, (mean, n_p, n_a, y, k * y_p, bound)
            assert (ca[0, :3] <= acc[0, :3]).all() and ca[0, 3] == n_a
            want, _ = resolve_plain(shims[0], ca, prev)
            assert np.array_equal(got, want), "behind the clamp the join is sh_resolve_slot's"
            # the colour is kept: the three sums are scaled alike
            ratio = ca[0, :3].astype(np.float64) / acc[0, :3]
            assert ratio.max() - ratio.min() <= 2.0 / acc[0, :3].min() + 4 * U
    print(f"largest |Y - K Y_p| is {worst:.3f} of the bound")


def restated_clamp(acc, prev):
    """S25 (a) in float64 from the integer words -> the scaled sums as real numbers (the sums themselves where the step does not act)"""
    n_p, f_p, n_a = int(prev[3]) & 0xFFFF, (int(prev[3]) >> 16) & 0xFF, int(acc[3])
    sums = acc[:3].astype(np.float64)
    if not (n_a > 0 and n_p >= MIN_SAMPLES and f_p >= MIN_FRAMES):
        return sums, False
    y_p = max(float(lum64(prev[:3], n_p)), FLOOR)
    y_a = float(lum64(acc[:3], n_a))
    limit = (5.0 + 5.0 / n_p) * y_p
    if not y_a > limit:
        return sums, False
    return sums * (limit / y_a), True


def test_clamp_against_the_float64_restatement(shims, ff_lib):
    """Random voxels with a long history.  Per sum, against sum * min(1, K Y_p / Y_a) of the restatement: the header's factor carries 16 u
    and its product 2 more (the count of test_spike_is_clamped_to_k_times_the_history), 20 u with the second-order terms, and the
    truncation less than 1: |got - want| <= 20 u sum + 1.  Where the two disagree on Y_a > K Y_p the factor is within 16 u of 1 and the
    same bound holds, so no voxel is left out.  The guards of sh_ff_scale (a product at or above 2^32, a result above the sum) move a
    result towards the exact one."""
    rng = np.random.default_rng(21)
    acc, prev = random_voxels(rng, 6000, "long")
    # a third of them near the threshold and above it, so that the clamp acts often: acc = history's mean times a factor around K
    near = np.flatnonzero(rng.random(len(acc)) < 0.5)
    for i in near:
        n_p, n_a = int(prev[i, 3]) & 0xFFFF, max(int(acc[i, 3]) & 0xFF, 1)
        f = rng.choice([4.9, 5.0, 5.2, 5.7, 8.0, 100.0]) * max(1.0, 1.0 / max(float(lum64(prev[i, :3], n_p)), 1e-9))
        acc[i, :3] = np.clip(prev[i, :3].astype(np.float64) / n_p * n_a * f, 0, 0xFFFFFFFF).astype(np.uint32)
        acc[i, 3] = n_a
    got, clear, ca, cl = resolve_ff(ff_lib, acc, prev)
    want_join, want_clear = resolve_plain(shims[0], ca, prev)
    assert np.array_equal(got, want_join) and np.array_equal(clear, want_clear)
    assert (ca[:, :3] <= acc[:, :3]).all(), "a sum rose"
    assert np.array_equal(ca[:, 3], acc[:, 3]), "a count changed"
    plain, _ = resolve_plain(shims[0], acc, prev)
    assert np.array_equal(got[:, 3] >> 16, plain[:, 3] >> 16), "frame and stale counts are the unfiltered resolve's"
    worst, disagreements, acted = 0.0, 0, 0
    for i in range(len(acc)):
        want, clamped = restated_clamp(acc[i], prev[i])
        bound = 20 * U * acc[i, :3].astype(np.float64) + 1.0
        err = np.abs(ca[i, :3].astype(np.float64) - want)
        assert (err <= bound).all(), (i, acc[i], prev[i], ca[i], want)
        worst = max(worst, float((err / bound).max()))
        disagreements += clamped != bool(cl[i])
        acted += clamped
    print(f"{acted} of {len(acc)} voxels clamped, {disagreements} decided differently at the threshold; largest error {worst:.3f} of the bound")
    assert acted > 1000 and (len(acc) - acted) > 1000


# ---------------------------------------------------------------------------------------------------- CPU 3: the weight threshold
def lum32(c):
    c = np.asarray(c, np.float32)
    return np.float32(np.float32(LUM32[0] * c[0]) + np.float32(LUM32[1] * c[1])) + np.float32(LUM32[2] * c[2])


def propagate(ff_lib, weights, length, radiance, ff, skipped=False, T=None):
    """-> (accum (8, 4), stopped, weight[0]) after the walk over slots 1, 2, 3"""
    slots = np.array([1, 2, 3], np.uint32)
    w = np.ones((3, 3), np.float32)
    if len(weights):
        w[:len(weights)] = weights
    accum, stopped, w0 = np.zeros((8, 4), np.uint32), np.zeros(1, np.uint32), np.zeros(3, np.float32)
    ff_lib.sh_host_propagate(p(slots), p(w), length, int(skipped), p(np.asarray(T, np.float32)) if T is not None else None, p(np.asarray(radiance, np.float32)),
                             p(accum), 8, int(ff), p(stopped), p(w0))
    return accum, int(stopped[0]), w0


def q3(c):
    return [ref.quantise(float(x)) for x in np.asarray(c, np.float32)]


def test_weight_threshold_known_answers(ff_lib):
    r = np.array([1.0, 0.5, 0.25], np.float32)
    y = np.zeros(3, np.float32)
    ff_lib.sh_host_luminance(p(np.array([[1.9] * 3, [2.1] * 3, [2.0] * 3], np.float32)), 3, p(y))
    assert [float(v) for v in y] == [float(lum32([a] * 3)) for a in (1.9, 2.1, 2.0)], "Y left to right, no fma"
    assert y[0] < 2.0 < y[1]
    # one stored vertex: a weight of luminance 1.9 passes, 2.1 stops; without the filter both pass
    for wt, stops in ((1.9, False), (2.1, True), (2.0, bool(y[2] > 2.0))):
        for ff in (False, True):
            accum, stopped, _ = propagate(ff_lib, [[wt] * 3], 1, r, ff)
            want = np.zeros((8, 4), np.uint32)
            if not (ff and stops):
                want[1, :3] = q3(r * np.float32(wt))
            assert np.array_equal(accum, want) and stopped == int(ff and stops), (wt, ff)
    # a coloured weight: the luminance decides, not a component
    accum, stopped, _ = propagate(ff_lib, [[9.0, 0.1, 0.1]], 1, r, True)
    assert lum32([9.0, 0.1, 0.1]) < 2.0 and stopped == 0 and list(accum[1, :3]) == q3(r * np.float32([9.0, 0.1, 0.1]))
    accum, stopped, _ = propagate(ff_lib, [[0.1, 2.9, 0.1]], 1, r, True)
    assert lum32([0.1, 2.9, 0.1]) > 2.0 and stopped == 1 and not accum.any()
    # three vertices, weights 1.5 each: the product crosses 2 at the second vertex, which and whatever lies behind it receive nothing
    w = [[1.5] * 3] * 3
    accum, stopped, _ = propagate(ff_lib, w, 3, r, True)
    want = np.zeros((8, 4), np.uint32)
    want[1, :3] = q3(r * np.float32(1.5))
    assert np.array_equal(accum, want) and stopped == 1
    accum, stopped, _ = propagate(ff_lib, w, 3, r, False)
    want[2, :3] = q3(r * np.float32(1.5) * np.float32(1.5))
    want[3, :3] = q3(r * np.float32(1.5) * np.float32(1.5) * np.float32(1.5))
    assert np.array_equal(accum, want) and stopped == 0
    # a heavy vertex behind a light one, a light one behind a heavy one (the walk does not resume)
    accum, stopped, _ = propagate(ff_lib, [[0.5] * 3, [3.0] * 3, [0.1] * 3], 3, r, True)
    assert stopped == 0 and accum[1, :3].any() and accum[2, :3].any() and accum[3, :3].any(), "0.5, 1.5, 0.15: never above 2"
    accum, stopped, _ = propagate(ff_lib, [[3.0] * 3, [0.1] * 3, [1.0] * 3], 3, r, True)
    assert stopped == 1 and not accum.any(), "3 stops the walk although the product falls to 0.3 behind it"
    # no sample count is ever added by the walk; length 0 adds nothing; vertices beyond the length are not read
    for ff in (False, True):
        accum, stopped, _ = propagate(ff_lib, [], 0, r, ff)
        assert not accum.any() and stopped == 0
        accum, stopped, _ = propagate(ff_lib, [[1.0] * 3, [50.0] * 3, [50.0] * 3], 1, r, ff)
        assert list(accum[1]) == [*q3(r), 0] and not accum[2:].any() and stopped == 0
    # NaN and infinite weights: a NaN luminance stops nothing and quantises to 0; an infinite one stops
    accum, stopped, _ = propagate(ff_lib, [[np.nan] * 3], 1, r, True)
    assert stopped == 0 and not accum.any()
    accum, stopped, _ = propagate(ff_lib, [[np.inf] * 3], 1, r, True)
    assert stopped == 1 and not accum.any()


def test_weight_threshold_skipped_vertex(ff_lib):
    """after a vertex that found no slot, the next segment's throughput multiplies the stored weight (sh_set_throughput): 1.5 * 1.5
    crosses the threshold at the first vertex, where 1.5 alone (no skip: the throughput replaces the weight) does not"""
    r = np.array([1.0, 1.0, 1.0], np.float32)
    accum, stopped, w0 = propagate(ff_lib, [[1.5] * 3], 1, r, True, skipped=True, T=[1.5] * 3)
    assert list(w0) == [2.25] * 3 and stopped == 1 and not accum.any()
    accum, stopped, w0 = propagate(ff_lib, [[1.5] * 3], 1, r, True, skipped=False, T=[1.5] * 3)
    assert list(w0) == [1.5] * 3 and stopped == 0 and list(accum[1, :3]) == q3(r * np.float32(1.5))
    accum, stopped, w0 = propagate(ff_lib, [[1.5] * 3], 1, r, False, skipped=True, T=[1.5] * 3)
    assert stopped == 0 and list(accum[1, :3]) == q3(r * np.float32(2.25))


def test_update_hit_keeps_the_vertex_own_sample(ff_lib):
    """sh_update_hit with a stored vertex whose weight is above the threshold: the new vertex's own (emission, 1 sample) is added with and
    without the filter; the stored vertex receives the emission only without it"""
    cap = 64
    e = np.array([2.0, 1.0, 0.5], np.float32)
    res = {}
    for ff in (False, True):
        keys, accum, resolved = np.zeros(cap, np.uint64), np.zeros((cap, 4), np.uint32), np.zeros((cap, 4), np.uint32)
        w = np.ones((3, 3), np.float32)
        w[0] = 2.5
        slot, stopped = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        ff_lib.sh_host_update_hit(p(keys), p(accum), p(resolved), cap, p(np.zeros(3, np.float32)), 50.0, p(np.array([63, 0, 0], np.uint32)), p(w), 1,
                                  p(np.array([1.0, 2.0, 3.0], np.float32)), p(np.array([0.0, 1.0, 0.0], np.float32)), p(e), 0.9, int(ff), p(slot), p(stopped))
        s = int(slot[0])
        assert s != 0xFFFFFFFF and s != 63 and keys[s] != 0
        assert list(accum[s]) == [*q3(e), 1], ff
        res[ff] = (accum[63].copy(), int(stopped[0]))
    assert list(res[False][0]) == [*q3(e * np.float32(2.5)), 0] and res[False][1] == 0
    assert not res[True][0].any() and res[True][1] == 1


# ---------------------------------------------------------------------------------------------------- CPU 4: the filter off
@pytest.mark.parametrize("scene", ["test", "c1"])
def test_filter_off_is_the_existing_header(dxrs, host, shims, ex_lib, ff_lib, cpu_scene, scene):  # noqa: F811
    w, h = (W, H) if scene == "test" else (24, 16)
    spheres, mats, sd, cam = cpu_scene if scene == "test" else c1_cpu(dxrs, host, w, h)
    for with_di in (False, True):
        old, new = HostCacheEx(ex_lib, *shims, spheres, mats, sd), HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd)
        for f in range(6):
            gs = dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=2 if f == 2 else 1)
            di = random_di(w, h, 40 + f, 0.2) if with_di else None
            st = dict(capacity=1 << 12, reset_history=f == 0)
            want, wb, rays, failed = old.call_ex(cam, gs, di=di, mode=1 if with_di else 0, **st)
            got, gb, rays_ff, failed_ff = new.call_ff(cam, gs, di=di, mode=1 if with_di else 0, anti_firefly=False, **st)
            assert same_bits(got, want) and (rays_ff, failed_ff) == (rays, failed) and all(same_bits(gb[k], wb[k]) for k in wb)
            assert new.content() == old.content() and len(old.content()) > 20
        assert new.clamped == 0 and new.stopped == 0


# ---------------------------------------------------------------------------------------------------- CPU 5: the effect
def firefly_scene(dxrs):
    """a glossy ground (roughness 0.1, mostly metallic) next to one small, strong emitter above it (radius 0.1, two units up: its own voxels
    lie above the ground's), under a dim sky: a path that leaves the ground and meets the emitter brings back hundreds of times what its
    neighbours do.  A rough white sphere stands beside it: the ground's own lobes never weigh a segment above 2, a path that leaves the
    white sphere through its specular lobe does, and without such a path the weight threshold would have nothing to stop"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(3, SPHERE_DTYPE)
    spheres[0] = (0.0, -1000.0, 0.0, 1000.0)
    spheres[1] = (0.0, 2.0, 0.0, 0.1)
    spheres[2] = (1.5, 0.7, 0.5, 0.7)
    mats = default_material(3)
    mats["BaseColor"][:, :3] = [(0.6, 0.55, 0.5), (0, 0, 0), (0.9, 0.9, 0.9)]
    mats["Roughness"] = [0.1, 0.5, 0.9]
    mats["Metallic"] = [0.8, 0.0, 0.0]
    mats["EmissiveColor"][1] = (1.0, 0.9, 0.8)
    mats["EmissiveStrength"][1] = 250.0
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.05, 0.05, 0.05, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = 1
    return spheres, mats, sd


def ground_luminance(content):
    """key -> Y of the voxel's radiance, over the ground's voxels with samples (cell y of -1 or 0: the emitter's lie above)"""
    out = {}
    for k, v in content.items():
        n = v[3] & 0xFFFF
        if n and ref.unpack_key(k)["cell"][1] in (-1, 0):
            out[k] = float(lum64(v[:3], n))
    return out


def blotch_ratio(lum):
    """the largest ratio of a voxel to the median of its neighbours (same level and octant, cells at most one apart, at least 4 of them)"""
    cells = {}
    for k in lum:
        u = ref.unpack_key(k)
        cells.setdefault((u["level"], u["octant"]), {})[u["cell"]] = lum[k]
    best = 0.0
    for group in cells.values():
        for (x, y, z), v in group.items():
            nb = [group[(x + dx, y + dy, z + dz)] for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                  if (dx, dy, dz) != (0, 0, 0) and (x + dx, y + dy, z + dz) in group]
            if len(nb) >= 4 and np.median(nb) > 0:
                best = max(best, v / float(np.median(nb)))
    return best


def test_filter_lowers_the_variance_and_adds_no_energy(dxrs, host, shims, ex_lib, ff_lib):  # noqa: F811
    """24 resting frames of the 48 x 32 update grid (DownscaleFactor 1, scene scale 5: voxels of 0.8 and 1.6 units, which several paths a
    frame meet, as in test_sharc.py's content test), filter off and on.  Measured on the CPU: without the filter the largest ground voxel
    is 293 times the median of its neighbours (33 with it); 8 slots clamped and 3 walks stopped in the 24 frames; over the 279 ground
    voxels both runs hold from frame 8 on, the summed frame-to-frame variance of the luminance falls from 43.3 to 0.314 (0.7 %), the
    summed mean from 30.1 to 12.6 (42 %: the filter is biased, it removes the energy of the rare paths it clamps)."""
    frames, first = 24, 8
    spheres, mats, sd = firefly_scene(dxrs)
    cam = host.camera_matrices(W, H, position=(0.0, 1.5, -7.0), look_at=(0.0, 0.5, 0.0), hfov=math.radians(60), jitter=False)
    runs = {}
    for ff in (False, True):
        hc = HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd)
        per_frame = []
        for f in range(frames):
            gs = dxrs.types.graphics_settings(W, H, frame_index=f, bounces=8, spp=1)
            _, _, _, failed = hc.call_ff(cam, gs, stages=UPDATE | RESOLVE, reset_history=f == 0, capacity=1 << 14, downscale_factor=1, scene_scale=5.0,
                                         anti_firefly=ff)
            assert failed == 0
            if f >= first:
                per_frame.append(ground_luminance(hc.content()))
        runs[ff] = (per_frame, hc.clamped, hc.stopped)
    off, on = runs[False][0], runs[True][0]
    blotch = max(blotch_ratio(lum) for lum in off)
    print(f"filter off: the largest voxel-to-neighbour-median ratio is {blotch:.1f}")
    assert blotch >= 10.0, "the scene shows no blotch without the filter: the run shows nothing"
    print(f"filter on: {runs[True][1]} slots clamped, {runs[True][2]} walks stopped in {frames} frames")
    assert runs[False][1] == 0 and runs[False][2] == 0
    assert runs[True][1] >= 1 and runs[True][2] >= 1
    common = set.intersection(*(set(lum) for lum in off), *(set(lum) for lum in on))
    assert len(common) > 50
    a = np.array([[lum[k] for k in sorted(common)] for lum in off])
    b = np.array([[lum[k] for k in sorted(common)] for lum in on])
    var_off, var_on = float(a.var(axis=0, ddof=1).sum()), float(b.var(axis=0, ddof=1).sum())
    mean_off, mean_on = float(a.mean(axis=0).sum()), float(b.mean(axis=0).sum())
    print(f"{len(common)} voxels, frames {first}..{frames - 1}: summed variance {var_off:.4g} -> {var_on:.4g} ({var_on / var_off:.3f}), summed mean {mean_off:.4g} -> {mean_on:.4g} "
          f"({mean_on / mean_off:.3f}); blotch ratio with the filter {max(blotch_ratio(lum) for lum in on):.1f}")
    assert var_on < var_off
    assert mean_on <= mean_off


# ---------------------------------------------------------------------------------------------------- CPU 6: sanitizers
def test_sanitized_stand_alone_program(tmp_path):
    """the clamp and the weight threshold on edge voxels and weights (zeros, saturated sums, counts past 16 bits, NaN and infinities), then
    eight frames of update, resolve and query with the filter on, with and without a DI that spikes, under ASan + UBSan, in a child process
    (nothing sanitised is loaded into Python)"""
    exe = str(tmp_path / "sharc_ff_sanitize")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-o", exe, "sharc_ff_sanitize.cpp"], cwd=os.path.join(HERE, "hostshim"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout


# ---------------------------------------------------------------------------------------------------- GPU
N_FRAMES = 6
FF = dict(anti_firefly=True, scene_scale=5.0)  # (voxels of 0.8 and 1.6 units: at 48 x 32 update paths a voxel gathers the history the clamp needs)


def moving_cameras(host, position, look_at, **kw):
    """six cameras, each a few hundredths of a unit from the last: the voxels keep their keys, the paths change"""
    cams, prev = [], None
    for f in range(N_FRAMES):
        prev = host.camera_matrices(GW, GH, position=(position[0] + 0.03 * f, position[1] + 0.01 * f, position[2]), look_at=look_at, previous=prev, **kw)
        cams.append(prev)
    return cams


def spiking_di(f, seed):
    """a random DI (a fifth of the texels 0); in the last frame a block of texels holds 1000 in every channel of Diffuse"""
    di = random_di(GW, GH, seed + f, 0.2)
    if f == N_FRAMES - 1:
        di[0][GH // 4:3 * GH // 4, GW // 4:3 * GW // 4, :3] = 1000.0
    return di


def host_sequence(dxrs, hc, cams, with_di, mode, bounces=8, seed=300, flags=None, require_clamp=True, require_stop=True, **kw):
    """the six calls on the host header -> per frame (gs, di, settings, image, outputs, rays, failed, content); asserts that the sequence
    clamps a slot and stops a walk"""
    frames = []
    for f, cam in enumerate(cams):
        gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=bounces, spp=2 if f == 1 else 1)
        di = spiking_di(f, seed) if with_di else None
        st = defaults(reset_history=f == 0, **dict(FF, **kw))
        if flags is not None:
            st["anti_firefly"] = flags[f]
        want, wb, rays, failed = hc.call_ff(cam, gs, di=di, mode=mode, **st)
        frames.append((gs, di, st, want, wb, rays, failed, hc.content()))
    print(f"host: {hc.clamped} slots clamped, {hc.stopped} walks stopped, {len(frames[-1][7])} voxels")
    assert (hc.clamped >= 1 or not require_clamp) and (hc.stopped >= 1 or not require_stop), "the sequence does not exercise the filter"
    return frames


def device_equals_host(dxrs, r, frames, spheres, mats, sd, cams, mode, textures=None, min_voxels=100):
    """the same six calls on the device: keys and voxels (pt_sharc_download, as a map), image, outputs and the ray counter"""
    for f, (cam, (gs, di, st, want, wb, rays, failed, content)) in enumerate(zip(cams, frames)):
        if f == 0:
            setup(r, dxrs, spheres, mats, sd, cam, gs, textures)
        r.set_camera(cam)
        r.set_constants(gs)
        got, gb, grays = gpu_call(r, di=di, mode=mode, **st)
        g = gpu_content(r, st["capacity"])
        assert set(g) == set(content), f"mode {mode} frame {f}: {len(set(g) ^ set(content))} keys differ"
        bad = [k for k in g if g[k] != content[k]]
        assert not bad, f"mode {mode} frame {f}: {len(bad)} of {len(g)} voxels differ"
        assert len(g) > min_voxels
        assert same_bits(got, want), f"mode {mode} frame {f}: {int((bits(got) != bits(want)).any(axis=-1).sum())} pixels differ from the host header"
        for k in wb:
            assert same_bits(gb[k], wb[k]), (mode, f, k)
            assert not is_sentinel(wb[k]).all()
        assert grays == rays, (mode, f, grays, rays)
        # (the C-ABI reports the ray counter only; the failed-insert counter is held to the host's through the cache's content: the host's
        # count is 0 here, and an insert that failed on the device would leave a key out of the map compared above)
        assert failed == 0, "the capacity must be chosen so that the host run has no failed insert"


C1_VIEW = dict(position=(1.0, 5.0, -5.0), look_at=(0.0, 3.0, 0.0))  # (onto the rough white sphere: its specular lobe weighs segments above 2)


@pytest.mark.gpu
def test_gpu_equals_the_host_header_test_scene_without_di(dxrs, host, renderer, shims, ex_lib, ff_lib):  # noqa: F811
    """(scene scale 10 here: at 5 no voxel of this scene is clamped within six frames)"""
    spheres, mats, sd = make_scene(dxrs)
    cams = moving_cameras(host, (0.0, 2.5, -9.0), (0.0, 1.0, 0.0), hfov=math.radians(70))
    frames = host_sequence(dxrs, HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd), cams, False, 0, scene_scale=10.0)
    device_equals_host(dxrs, renderer, frames, spheres, mats, sd, cams, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_gpu_equals_the_host_header_c1_with_di(dxrs, host, renderer, shims, ex_lib, ff_lib, mode):  # noqa: F811
    spheres, mats, sd, _ = c1(dxrs, host)
    cams = moving_cameras(host, **C1_VIEW)
    frames = host_sequence(dxrs, HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd), cams, True, mode)
    device_equals_host(dxrs, renderer, frames, spheres, mats, sd, cams, mode)


@pytest.mark.gpu
def test_gpu_equals_the_host_header_scene_in_global_memory(dxrs, host, shims, ex_lib, ff_lib):  # noqa: F811
    spheres, mats, sd, _ = c1(dxrs, host)
    cams = moving_cameras(host, **C1_VIEW)
    frames = host_sequence(dxrs, HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd), cams, True, 1, seed=400)
    r = dxrs.Renderer(device=0, flags=dxrs.types.PT_FLAG_NO_LDS_SCENE)
    try:
        device_equals_host(dxrs, r, frames, spheres, mats, sd, cams, 1)
        assert not r.accel.lds_resident
    finally:
        r.close()


def alpha_case(dxrs, host):
    import golden_cases
    return next(c for c in golden_cases.cases(dxrs, host) if c["file"].startswith("a5_alpha"))


def rough_ground(spheres, mats):
    """the scene's largest sphere, its ground, with the test scene's ground material (a rough dielectric).  The mirror grounds of the
    golden alpha scene and of the procedural scene never weigh a segment above 2, and six frames of them stop no walk; a rough dielectric
    does it a few times (its specular lobe is chosen by the Fresnel term at the normal and weighs by the one at the half vector)"""
    mats = mats.copy()
    g = int(np.argmax(spheres["r"]))
    mats["Metallic"][g], mats["Roughness"][g] = 0.0, 0.6
    mats["BaseColor"][g, :3] = (0.6, 0.55, 0.5)
    return mats


@pytest.mark.gpu
def test_gpu_equals_the_host_header_textured_alpha_scene(dxrs, host, renderer, shims, ex_lib, ff_lib):  # noqa: F811
    """the alpha-tested golden scene (tests/golden_cases.py, row a5) on a rough ground (rough_ground), mode 2"""
    case = alpha_case(dxrs, host)
    mats = rough_ground(case["spheres"], case["materials"])
    cams = moving_cameras(host, (0.0, 2.0, -7.0), None, jitter_index=1)
    hc = HostCacheFf(ff_lib, ex_lib, *shims, case["spheres"], mats, case["sd"], textures=case["textures"])
    frames = host_sequence(dxrs, hc, cams, True, 2, bounces=5, seed=500)
    try:
        device_equals_host(dxrs, renderer, frames, case["spheres"], mats, case["sd"], cams, 2, textures=case["textures"])
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_equals_the_host_header_tree_with_32_bit_stack(dxrs, host, shims, ex_lib, ff_lib):  # noqa: F811
    """32,800 spheres (the tree takes the 32-bit stack from 32767 nodes) on a rough ground (rough_ground), mode 1; the host's trace culls
    before its exact test"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=32800)
    mats = rough_ground(spheres, mats)
    cams = moving_cameras(host, (0.0, 1.0, -5.0), (0.0, 0.5, 0.0))
    frames = host_sequence(dxrs, HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd), cams, True, 1, seed=600)
    r = dxrs.Renderer(device=0)
    try:
        device_equals_host(dxrs, r, frames, spheres, mats, sd, cams, 1)
        assert r.accel.node_count >= 32767 and not r.accel.lds_resident
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------- GPU: the smallest shapes
def small_frames(dxrs, host, r, hc, spheres, mats, sd, w, h, n, position, look_at, min_voxels, **kw):
    """n calls of a w x h frame with the filter on, device against host: the cache as a map, the image, the rays"""
    prev = None
    for f in range(n):
        cam = prev = host.camera_matrices(w, h, position=(position[0] + 0.03 * f, position[1], position[2]), look_at=look_at, hfov=math.radians(70), previous=prev)
        gs = dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1)
        if f == 0:
            setup(r, dxrs, spheres, mats, sd, cam, gs)
        r.set_camera(cam)
        r.set_constants(gs)
        st = defaults(reset_history=f == 0, **dict(FF, **kw))
        got, _, rays = gpu_call(r, **st)
        want, _, wrays, failed = hc.call_ff(cam, gs, **st)
        assert failed == 0
        g, c = gpu_content(r, st["capacity"]), hc.content()
        assert g == c and len(g) >= min_voxels, (f, len(g), len(c))
        assert same_bits(got, want) and rays == wrays, f


@pytest.mark.gpu
def test_gpu_one_path_update_grid(dxrs, host, renderer, shims, ex_lib, ff_lib):  # noqa: F811
    """a 4 x 4 frame with DownscaleFactor 4: one update path, one partial wave in every kernel"""
    spheres, mats, sd = make_scene(dxrs)
    small_frames(dxrs, host, renderer, HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd), spheres, mats, sd, 4, 4, 4, (0.0, 2.5, -9.0), (0.0, 1.0, 0.0), 1,
                 downscale_factor=4, capacity=16)


@pytest.mark.gpu
def test_gpu_ragged_frame(dxrs, host, renderer, shims, ex_lib, ff_lib):  # noqa: F811
    """19 x 13: no multiple of the 8 x 8 block in either direction; the update grid is 9 x 6"""
    spheres, mats, sd = make_scene(dxrs)
    small_frames(dxrs, host, renderer, HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd), spheres, mats, sd, 19, 13, 4, (0.0, 2.5, -9.0), (0.0, 1.0, 0.0), 20,
                 capacity=1 << 10)


@pytest.mark.gpu
def test_gpu_one_full_bucket(dxrs, host, renderer, shims, ex_lib, ff_lib):  # noqa: F811
    """Capacity 16: one bucket, one partial workgroup in the resolve.  Which keys a full bucket turns away depends on the order the
    inserts arrive in, so the bucket is filled on the host (two frames, in the host's order), installed on the device (pt_sharc_upload),
    and both go on from there: every slot holds a key, every insert of another key fails on both sides alike, the sixteen voxels gather
    samples and are clamped and resolved word for word."""
    spheres, mats, sd = make_scene(dxrs)
    hc = HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd)
    cams = moving_cameras(host, (0.0, 2.5, -9.0), (0.0, 1.0, 0.0), hfov=math.radians(70))
    st = dict(FF, capacity=16)
    failures = 0
    for f in range(2):
        gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1)
        _, _, _, failed = hc.call_ff(cams[f], gs, **defaults(reset_history=f == 0, stages=UPDATE | RESOLVE, **st))
        failures += failed
    assert failures > 100 and (hc.keys != 0).all(), "the bucket is full and inserts have failed"
    setup(renderer, dxrs, spheres, mats, sd, cams[2], dxrs.types.graphics_settings(GW, GH, frame_index=2, bounces=8, spp=1))
    renderer.sharc_upload(hc.keys, hc.resolved)
    for f in range(2, N_FRAMES):
        gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1)
        renderer.set_camera(cams[f])
        renderer.set_constants(gs)
        got, _, rays = gpu_call(renderer, **defaults(**st))
        want, _, wrays, failed = hc.call_ff(cams[f], gs, **defaults(**st))
        assert failed > 100
        assert gpu_content(renderer, 16) == hc.content() and len(hc.content()) == 16
        assert same_bits(got, want) and rays == wrays, f
    print(f"host: {hc.clamped} slots clamped, {hc.stopped} walks stopped")


# ---------------------------------------------------------------------------------------------------- GPU: the flag between calls
@pytest.mark.gpu
def test_gpu_flag_switched_between_calls(dxrs, host, renderer, shims, ex_lib, ff_lib):  # noqa: F811
    """off, on, off, on, off, on over one cache: the flag has no state of its own"""
    spheres, mats, sd, _ = c1(dxrs, host)
    cams = moving_cameras(host, **C1_VIEW)
    hc = HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd)
    frames = host_sequence(dxrs, hc, cams, True, 1, flags=(False, True, False, True, False, True), require_stop=False)
    device_equals_host(dxrs, renderer, frames, spheres, mats, sd, cams, 1)
    plain = HostCacheFf(ff_lib, ex_lib, *shims, spheres, mats, sd)
    off = host_sequence(dxrs, plain, cams, True, 1, flags=(False,) * N_FRAMES, require_stop=False, require_clamp=False)
    assert off[-1][7] != frames[-1][7], "the filter changed the cache"


# ---------------------------------------------------------------------------------------------------- GPU: the default frame
def chain(dxrs, host, sync):
    """test_sharc_ex.chain with IsAntiFireflyEnabled: three frames of gbuffer -> restir_di_ex -> sharc_ex(DI, mode 1, the NRD outputs named
    as the DI buffers, the filter on) -> ray reconstruction on a context with three lanes; sync: a device synchronise after every call"""
    import torch
    from dxrs_amd.abi_types import RESTIR_DI_INPUTS
    w, h, Wo, Ho = GW, GH, 2 * GW, 2 * GH
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
                               candidates=dict(brdf_samples=1, boiling_filter=0.2))
            wait()
            r.render_sharc_ex_device(color.data_ptr(), dd.data_ptr(), ds.data_ptr(), None, 1,
                                     dict(SpecularHitDistance=shd.data_ptr(), Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), **defaults(reset_history=f == 0, **FF))
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
        return results, cache_map(*r.sharc_download(CAP))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_default_frame_chain_queued_equals_synchronised(dxrs, host):
    queued, cq = chain(dxrs, host, False)
    synced, cs = chain(dxrs, host, True)
    assert cq == cs and len(cq) > 100
    for f in range(3):
        for name, a, b in zip(("Diffuse", "Specular", "Color", "SpecularHitDistance", "Output"), queued[f], synced[f]):
            assert same_bits(a, b), f"frame {f}: {name} differs"
        dd, ds, color, shd, output = queued[f]
        assert (dd[..., :3] > 0).any() and (shd > 0).any() and np.isfinite(output).all() and output[..., :3].max() > 0
        assert np.isfinite(color).all()


# ---------------------------------------------------------------------------------------------------- GPU: arguments
@pytest.mark.gpu
def test_gpu_argument_rules(dxrs, host, renderer):
    import torch
    from dxrs_amd.abi_types import PtDirectLighting, PtRect, PtSharcSettings
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=4, spp=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    renderer.render_sharc(**defaults(reset_history=True))
    content = gpu_content(renderer)
    dev = torch.device("cuda", 0)
    n = GW * GH
    buf = {k: torch.full((n + 1, 4), 7.0, device=dev) for k in ("out", "dd", "ds")}
    torch.cuda.synchronize(dev)
    lib, ctx = renderer._lib, renderer._ctx
    ptr = {k: v.data_ptr() for k, v in buf.items()}

    def call(di=False, rect=None, stages=7, ff=1):
        s = PtSharcSettings(Capacity=CAP, DownscaleFactor=2, Stages=stages, IsAntiFireflyEnabled=ff)
        d = PtDirectLighting(Diffuse=C.c_void_p(ptr["dd"]), Specular=C.c_void_p(ptr["ds"])) if di else None
        return lib.pt_render_sharc_ex(ctx, C.byref(PtRect(*rect)) if rect else None, C.c_void_p(ptr["out"]), 1, C.byref(s), C.byref(d) if d else None, None, None)

    # refused with the flag set: a rect outside RenderSize; a partial rect with DI and the update stage
    assert call(rect=(90, 0, 10, 10)) == 1 and lib.pt_last_error(ctx)
    assert call(di=True, rect=(0, 0, GW, GH - 1)) == 1 and lib.pt_last_error(ctx)
    s = PtSharcSettings(Capacity=CAP, DownscaleFactor=2, Stages=QUERY, IsAntiFireflyEnabled=1)
    assert lib.pt_render_sharc(ctx, None, C.c_void_p(ptr["out"]), 1, C.byref(s), None) == 5, "pt_render_sharc keeps refusing the flag"
    assert b"pt_render_sharc_ex" in lib.pt_last_error(ctx), "the message points at the entry point that accepts it"
    renderer.synchronize()
    for k, v in buf.items():
        assert (v == 7.0).all(), f"a refused call wrote {k}"
    assert gpu_content(renderer) == content, "a refused call touched the cache"
    # accepted: the flag alone, with each stage alone, with a rect for a QUERY-only call, with a DI
    assert call() == 0
    for stages in (UPDATE, RESOLVE, QUERY, UPDATE | RESOLVE):
        assert call(stages=stages) == 0, stages
    assert call(rect=(8, 4, GW - 8, GH - 4), stages=QUERY) == 0
    assert call(di=True) == 0 and call(di=True, ff=0) == 0
    renderer.synchronize()
    assert (buf["out"][n:] == 7.0).all(), "nothing is written past the frame"
    want, _ = renderer.render()
    got, _, _ = gpu_call(renderer, **defaults(stages=QUERY, reset_history=True, anti_firefly=True))
    assert same_bits(got, want), "the context renders a correct frame afterwards"


# ---------------------------------------------------------------------------------------------------- GPU: the C++ mirror
@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """Raytracing::Render(radiance, SHARC&, SHARCSettings) and its five-argument form (host/Raytracing.hpp) from C++ with the settings
    filled as App.cpp:1270-1278 fills them (IsAntiFireflyEnabled = true): four frames without DI, then two DLSS-RR frames with a ReBLUR
    frame's Diffuse / Specular as their DI, give the binding's frames bit for bit"""
    import torch
    pkg = os.path.join(os.path.dirname(HERE), "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_sharc_ff")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_sharc_ff.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 160, 90
    outp = str(tmp_path / "sharc_ff.f32")
    res = subprocess.run([exe, str(w), str(h), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(outp, dtype=np.float32)
    plain_cpp, radiance = raw[:w * h * 4].reshape(h, w, 4), raw[w * h * 4:2 * w * h * 4].reshape(h, w, 4)
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0)
    try:
        st = dict(capacity=1 << 14, downscale_factor=4, scene_scale=5.0, roughness_threshold=0.4, accumulation_frames=10, max_stale_frames=64, anti_firefly=True)
        r.set_scene(spheres, mats, sd)
        r.set_camera(host.camera(w, h, jitter=False))
        for f in range(4):
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
            plain, _, _ = r.render_sharc_ex(reset_history=f == 0, **st)
        assert same_bits(plain_cpp, plain), "C++ mirror == Python path (no DI)"
        dev = torch.device("cuda", 0)
        nd, ns, tmp, out = (torch.zeros((h, w, 4), device=dev) for _ in range(4))
        shd = torch.zeros((h, w), device=dev)
        torch.cuda.synchronize(dev)
        r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=0, bounces=8, spp=1))
        r.render_denoiser_device(2, tmp.data_ptr(), {"Diffuse": nd.data_ptr(), "Specular": ns.data_ptr()})
        for f in range(2):
            r.render_sharc_ex_device(out.data_ptr(), nd.data_ptr(), ns.data_ptr(), None, 1, {"SpecularHitDistance": shd.data_ptr()}, reset_history=f == 0, **st)
        r.synchronize()
        assert same_bits(radiance, out.cpu().numpy()), "C++ mirror == Python path (DI, DLSS-RR)"
    finally:
        r.close()
