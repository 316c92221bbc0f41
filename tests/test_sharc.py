"""Row N14 -- pt_render_sharc, the frame through the radiance cache (DESIGN.md spec S20).
CPU: the host-compiled header (tests/hostshim/sharc_host.cpp over csrc/pt_sharc.h) against the float64 restatement (sharc_reference.py):
the hash grid, the key, the hash map, quantisation and resolve, the query's validity rule; the empty cache as the identity; the cache's
content against path-traced estimates from the same header with the cache off; a sanitizer build of a stand-alone program.
GPU: the query over an empty cache against pt_render bit for bit; update, resolve and query against the host-compiled header bit for
bit over consecutive frames; eviction, overflow, the restart and argument rules, frames in flight, a textured scene."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import sharc_reference as ref
from test_gbuffer import linear_textures
from test_restir_pass import make_scene

HERE = os.path.dirname(os.path.abspath(__file__))
UPDATE, RESOLVE, QUERY = 1, 2, 4
NO_SLOT = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- the host-compiled header
@pytest.fixture(scope="module")
def shims():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_sharc_shim())
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    for name, args in dict(sh_host_level=[vp, u32, f32, vp, vp], sh_host_voxel_size=[vp, u32, f32, vp], sh_host_key=[vp, vp, vp, vp, u32, vp],
                           sh_host_key_at=[vp, f32, vp, vp, u32, vp, vp], sh_host_bucket=[vp, u32, u32, vp], sh_host_map_ops=[vp, u32, vp, vp, u32, vp],
                           sh_host_quantise=[vp, u32, vp], sh_host_add=[vp, u32, vp, u32], sh_host_resolve=[vp, vp, u32, u32, u32, vp, vp],
                           sh_host_radiance=[vp, u32, vp], sh_host_valid_hit=[vp, vp, vp, u32, vp],
                           sh_host_call=[vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
                           sh_host_estimates=[vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp]).items():
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    gb = C.CDLL(g.build_gbuffer_shim())
    gb.gb_srgb_lut.restype = None
    gb.gb_srgb_lut.argtypes = [vp]
    return lib, gb


def p(a):
    """the array's address (the returned object keeps the array alive through the call)"""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def defaults(**kw):
    """pt_render_sharc's settings as the tests use them (the library's defaults for what is not given)"""
    s = dict(capacity=1 << 16, downscale_factor=2, scene_scale=50.0, roughness_threshold=0.4, accumulation_frames=10, max_stale_frames=64,
             visualize=False, reset_history=False, stages=0)
    s.update(kw)
    return s


class HostCache:
    """pt_render_sharc over the host-compiled header: the context's three arrays and the restart rules of the entry point"""

    def __init__(self, lib, gbshim, spheres, mats, sd, textures=None):
        self.lib, self.spheres, self.mats = lib, np.ascontiguousarray(spheres), np.ascontiguousarray(mats)
        self.env = np.array(list(sd.EnvironmentLightColor), np.float32)
        self.texels, self.info = linear_textures(gbshim, textures)
        self.maps = self.rot = None
        if self.texels is not None:
            maps = np.zeros((len(spheres), 8), np.uint32)
            maps[:, :7] = textures.maps
            maps[:, 7] = (textures.maps != 0xFFFFFFFF).any(axis=1)
            self.maps = np.ascontiguousarray(maps)
            self.rot = np.ascontiguousarray(textures.rotations, dtype=np.float32)
        self.capacity, self.valid = 0, False

    def install(self, keys, voxels):
        self.capacity, self.valid = len(keys), True
        self.keys, self.resolved, self.accum = keys.copy(), voxels.copy(), np.zeros_like(voxels)

    def call(self, cam, gs, rect=None, cache=True, **kw):
        """-> (image (h, w, 4) or None, rays, failed inserts); cache=False: the header's loop with the cache off"""
        s = defaults(**kw)
        stages = s["stages"] or 7
        w, h = gs.RenderSize[0], gs.RenderSize[1]
        rect = rect or (0, 0, w, h)
        if cache:
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
                        s["accumulation_frames"], s["max_stale_frames"], int(s["visualize"]), stages if cache else QUERY, *rect], np.uint32)
        fprm = np.array([gs.ThroughputThreshold, s["scene_scale"], s["roughness_threshold"]], np.float32)
        out = np.zeros((rect[3], rect[2], 4), np.float32)
        counters = np.zeros(2, np.uint64)
        self.lib.sh_host_call(p(self.spheres), p(self.mats), len(self.spheres), p(self.env), p(self.texels), p(self.info), 0 if self.info is None else len(self.info),
                              p(self.maps), p(self.rot), C.addressof(cam), p(prm), p(fprm), p(self.keys) if cache else None, p(self.accum) if cache else None,
                              p(self.resolved) if cache else None, p(out), p(counters))
        if cache and stages & RESOLVE:
            self.accum, self.resolved = self.resolved, self.accum
        return (out if stages & QUERY or not cache else None), int(counters[0]), int(counters[1])

    def content(self):
        return cache_map(self.keys, self.resolved)


def cache_map(keys, voxels):
    """the cache as key -> voxel words; a key in two slots is an error"""
    occupied = np.flatnonzero(keys)
    assert len(np.unique(keys[occupied])) == len(occupied), "a key occupies two slots"
    assert not voxels[keys == 0].any(), "an empty slot holds a voxel"
    return {int(keys[s]): tuple(int(x) for x in voxels[s]) for s in occupied}


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- CPU: ABI
def test_sharc_abi_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    for name in ("pt_render_sharc", "pt_sharc_download", "pt_sharc_upload"):
        assert hasattr(lib, name) and name in dxrs.binding.API_SYMBOLS
    from dxrs_amd.abi_types import PtSharcSettings
    assert C.sizeof(PtSharcSettings) == 48 and PtSharcSettings.SceneScale.offset == 8 and PtSharcSettings.AccumulationFrames.offset == 16
    assert PtSharcSettings.ResetHistory.offset == 32 and PtSharcSettings.Stages.offset == 36
    s = PtSharcSettings()
    assert lib.pt_render_sharc(None, None, None, 0, C.byref(s), None) == 1  # PT_ERR_INVALID_ARG: null context
    assert lib.pt_sharc_download(None, None, None, 16) == 1 and lib.pt_sharc_upload(None, None, None, 16) == 1


# ---------------------------------------------------------------------------------------------------- CPU: the hash grid
def header_levels(lib, d2, scale=50.0):
    d2 = f32(d2)
    level, voxel = np.zeros(len(d2), np.uint32), np.zeros(len(d2), np.float32)
    lib.sh_host_level(p(d2), len(d2), scale, p(level), p(voxel))
    return level, voxel


def test_grid_level_and_voxel_size(shims):
    lib = shims[0]
    # known answers: distance d = 2^k is the first of level k + bias, the float below it the last of level k - 1 + bias
    for k in (-3, 0, 1, 5, 10):
        d = np.float32(2.0 ** k)
        below = np.nextafter(d * d, np.float32(0), dtype=np.float32)
        level, voxel = header_levels(lib, [d * d, below])
        assert list(level) == [max(k + 2, 1), max(k + 1, 1)], (k, level)
        assert voxel[0] == np.float32(2.0 ** max(k + 2, 1) / 200.0)
    # distance 0, a denormal, the smallest normal, huge, inf: the clamp at level 1 and the top of the float range
    level, voxel = header_levels(lib, [0.0, 1e-45, 2.0 ** -126, 3e38, np.inf])
    assert list(level) == [1, 1, 1, 65, 66] and voxel[0] == np.float32(2.0 / 200.0)
    # the restatement over a sweep of squared distances, and over every exponent
    rng = np.random.default_rng(1)
    d2 = np.concatenate([np.exp(rng.uniform(-40, 40, 4000)), 2.0 ** np.arange(-126, 128, dtype=np.float64)]).astype(np.float32)
    level, voxel = header_levels(lib, d2, 17.0)
    for i in range(len(d2)):
        want = ref.grid_level(float(d2[i]))
        assert level[i] == want and voxel[i] == np.float32(ref.voxel_size(want, 17.0)), (d2[i], level[i], want)
    # the clamp at level 1023 (the level is a parameter of the voxel size: no float32 distance reaches it)
    lv = np.array([1, 127, 128, 1023], np.uint32)
    vs = np.zeros(4, np.float32)
    lib.sh_host_voxel_size(p(lv), 4, 50.0, p(vs))
    assert vs[0] == np.float32(0.01) and np.isfinite(vs[1]) and np.isinf(vs[2]) and np.isinf(vs[3])
    P, N = f32([[1, 2, 3]] * 2), f32([[0, 1, 0]] * 2)
    keys = np.zeros(2, np.uint64)
    lib.sh_host_key(p(P), p(N), p(np.array([0, 5000], np.uint32)), p(f32([1.0, 1.0])), 2, p(keys))
    assert [ref.unpack_key(int(k))["level"] for k in keys] == [1, 1023]


def test_key_packing(shims):
    lib = shims[0]
    rng = np.random.default_rng(2)
    n = 3000
    P = (rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-2, 4, (n, 1))).astype(np.float32)
    N = rng.normal(size=(n, 3)).astype(np.float32)
    N[:8] = [[(-1) ** (k & 1), (-1) ** (k >> 1 & 1), (-1) ** (k >> 2 & 1)] for k in range(8)]  # all 8 octants
    P[8] = (-0.5, -1e9, 1e9)      # below and above the field's range: clamped
    P[9] = (0.0, -0.0, 1e-30)
    level = rng.integers(1, 40, n).astype(np.uint32)
    level[8] = 7  # (a voxel of 0.64)
    voxel = np.array([ref.voxel_size(int(l), 50.0) for l in level], np.float32)
    keys = np.zeros(n, np.uint64)
    lib.sh_host_key(p(P), p(N), p(level), p(voxel), n, p(keys))
    assert (keys != 0).all(), "the level field is the nonzero tag"
    near = 0
    for i in range(n):
        want = ref.key([float(x) for x in P[i]], N[i], int(level[i]), float(voxel[i]))
        if int(keys[i]) != want:
            # float32 x / voxel may round onto a cell border that float64 stays below: only there may the cells differ, by one
            q = P[i].astype(np.float64) / float(voxel[i])
            got, exp = ref.unpack_key(int(keys[i])), ref.unpack_key(want)
            assert got["level"] == exp["level"] and got["octant"] == exp["octant"]
            assert all(abs(a - b) <= 1 and (a == b or abs(qq - round(qq)) < 1e-6 * max(1.0, abs(qq))) for a, b, qq in zip(got["cell"], exp["cell"], q)), (i, got, exp)
            near += 1
    assert near <= n // 100
    u = [ref.unpack_key(int(k)) for k in keys[:10]]
    assert sorted(x["octant"] for x in u[:8]) == list(range(8))
    assert u[8]["cell"][0] == -1 and u[8]["cell"][1] == -65536 and u[8]["cell"][2] == 65535
    assert u[9]["cell"] == (0, 0, 0) or u[9]["cell"] == (0, -0, 0)
    assert all(x["level"] == int(l) for x, l in zip(u, level[:10]))
    # a point and its neighbour across a cell border, a normal flipped: different keys; the same cell: the same key
    cam = f32([0, 0, 0])
    pts = f32([[10.01, 0.3, 0.3], [10.02, 0.3, 0.3], [10.01, 0.3, 0.3], [10.01 + 0.64, 0.3, 0.3]])
    nrm = f32([[0, 1, 0], [0, 1, 0], [0, -1, 0], [0, 1, 0]])
    k4, v4 = np.zeros(4, np.uint64), np.zeros(4, np.float32)
    lib.sh_host_key_at(p(cam), 50.0, p(pts), p(nrm), 4, p(k4), p(v4))
    assert k4[0] == k4[1] and k4[0] != k4[2] and k4[0] != k4[3] and v4[0] == np.float32(2.0 ** 5 / 200.0)
    base = np.zeros(n, np.uint32)
    lib.sh_host_bucket(p(keys), n, 1 << 12, p(base))
    assert all(int(base[i]) == ref.bucket_base(int(keys[i]), 1 << 12) for i in range(n))


# ---------------------------------------------------------------------------------------------------- CPU: the hash map
def test_map_insert_find_erase(shims):
    lib = shims[0]
    rng = np.random.default_rng(3)
    capacity = 1 << 8
    pool = rng.integers(1, 1 << 63, 300, dtype=np.uint64)
    ops = rng.choice([0, 1, 1, 2], 6000).astype(np.uint32)
    key = pool[rng.integers(0, len(pool), len(ops))]
    keys = np.zeros(capacity, np.uint64)
    slot = np.zeros(len(ops), np.uint32)
    lib.sh_host_map_ops(p(keys), capacity, p(ops), p(key), len(ops), p(slot))
    m = ref.Map(capacity)
    failed = holes_used = 0
    for i in range(len(ops)):
        k = int(key[i])
        want = (m.find, m.insert, m.erase)[int(ops[i])](k)
        assert int(slot[i]) == want, (i, ops[i], slot[i], want)
        failed += ops[i] == 1 and want == NO_SLOT
    assert failed > 0 and [int(x) for x in keys] == m.keys
    occupied = keys[keys != 0]
    assert len(np.unique(occupied)) == len(occupied), "a key occupies two slots"
    # inserts that follow evictions: a hole in front of a key must not make a second copy of it
    keys[:] = 0
    same = [int(k) for k in pool if ref.bucket_base(int(k), 32) == 0][:6]
    assert len(same) >= 4
    seq_ops = np.array([1, 1, 1, 2, 1, 1, 0], np.uint32)
    seq_key = np.array([same[0], same[1], same[2], same[0], same[2], same[3], same[2]], np.uint64)
    s7 = np.zeros(7, np.uint32)
    lib.sh_host_map_ops(p(keys), 32, p(seq_ops), p(seq_key), 7, p(s7))
    assert list(s7) == [0, 1, 2, 0, 2, 0, 2] and [int(x) for x in keys[:3]] == [same[3], same[1], same[2]]


def test_full_bucket_fails_the_insert_and_nothing_else(shims):
    lib = shims[0]
    capacity = 16  # one bucket
    keys = np.zeros(capacity, np.uint64)
    ins = np.arange(1, 21, dtype=np.uint64) << np.uint64(51)
    slot = np.zeros(20, np.uint32)
    lib.sh_host_map_ops(p(keys), capacity, p(np.ones(20, np.uint32)), p(ins), 20, p(slot))
    assert list(slot[:16]) == list(range(16)) and (slot[16:] == NO_SLOT).all()
    assert list(keys) == list(ins[:16]), "a failed insert leaves the bucket as it was"
    again = np.zeros(20, np.uint32)
    lib.sh_host_map_ops(p(keys), capacity, p(np.zeros(20, np.uint32)), p(ins), 20, p(again))
    assert list(again) == list(slot)


# ---------------------------------------------------------------------------------------------------- CPU: quantisation and resolve
def test_quantisation(shims):
    lib = shims[0]
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(0, 300, 2000), 10.0 ** rng.uniform(-8, 1, 2000), [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 256.0, 257.0, 1e30, 0.5 / 1024, 0.49 / 1024,
                                                                                  1.5 / 1024]]).astype(np.float32)
    q = np.zeros(len(x), np.uint32)
    lib.sh_host_quantise(p(x), len(x), p(q))
    assert [int(v) for v in q] == [ref.quantise(float(v)) for v in x]
    assert list(q[-12:]) == [0, 0, 0, 0, 262144, 0, 262144, 262144, 262144, 1, 0, 2]
    # a contribution with a NaN, a negative and a huge component, then an ordinary one with a sample: per component, order-free
    accum = np.zeros((4, 4), np.uint32)
    lib.sh_host_add(p(accum), 2, p(f32([np.nan, -3.0, 1e9])), 0)
    lib.sh_host_add(p(accum), 2, p(f32([0.25, 0.5, 1.0])), 1)
    assert [int(v) for v in accum[2]] == [256, 512, 262144 + 1024, 1] and not accum[[0, 1, 3]].any()


def voxel_w(n, frames, stale):
    return n | (frames << 16) | (stale << 24)


def test_resolve_every_branch(shims):
    lib = shims[0]
    rng = np.random.default_rng(5)
    cases = []  # (acc, prev, accumulation_frames, max_stale_frames)
    cases.append(((1000, 2000, 3000, 4), (0, 0, 0, 0), 10, 64))                                # first frame
    cases.append(((1000, 0, 7, 3), (5000, 6000, 7000, voxel_w(20, 4, 0)), 10, 64))              # accumulation below the window
    cases.append(((1000, 0, 7, 3), (5000, 6000, 7000, voxel_w(20, 9, 0)), 10, 64))              # ... reaching it exactly
    cases.append(((1000, 0, 7, 3), (5001, 6001, 7001, voxel_w(20, 10, 0)), 10, 64))             # above: rescaled by 10 / 11
    cases.append(((0, 0, 0, 0), (5000, 6000, 7000, voxel_w(1, 10, 0)), 10, 64))                 # stale, rescaled: keeps one sample
    cases.append(((0, 0, 0, 0), (5000, 6000, 7000, voxel_w(20, 3, 5)), 10, 64))                 # stale ageing
    cases.append(((0, 0, 0, 0), (5000, 6000, 7000, voxel_w(20, 3, 1)), 10, 2))                  # stale 2 = MaxStaleFrames: kept
    cases.append(((0, 0, 0, 0), (5000, 6000, 7000, voxel_w(20, 3, 2)), 10, 2))                  # stale 3 = MaxStaleFrames + 1: evicted
    cases.append(((7, 8, 9, 1), (5000, 6000, 7000, voxel_w(20, 3, 2)), 10, 2))                  # a sample resets the age
    cases.append(((4000000000, 5, 5, 70000), (4000000000, 5, 5, voxel_w(65535, 2, 0)), 10, 64))  # sums past 32 bits, samples past 16: halved
    cases.append(((0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF), (0xFFFFFFFF, 1, 0, voxel_w(65535, 255, 0)), 255, 254))
    for _ in range(300):
        acc = tuple(int(v) for v in rng.integers(0, 1 << 22, 3)) + (int(rng.integers(0, 50)) * int(rng.integers(0, 2)),)
        prev = tuple(int(v) for v in rng.integers(0, 1 << 30, 3)) + (voxel_w(int(rng.integers(0, 3000)), int(rng.integers(0, 14)), int(rng.integers(0, 6))),)
        cases.append((acc, prev, int(rng.integers(1, 12)), int(rng.integers(1, 6))))
    seen = dict(first=0, below=0, above=0, stale=0, evicted=0, halved=0)
    for acc, prev, A, M in cases:
        out, clear = np.zeros(4, np.uint32), np.zeros(1, np.uint32)
        lib.sh_host_resolve(p(np.array(acc, np.uint32)), p(np.array(prev, np.uint32)), 1, A, M, p(out), p(clear))
        sums, n, frames, stale, want_clear = ref.resolve(acc, prev, A, M)
        assert bool(clear[0]) == want_clear, (acc, prev, A, M)
        gn, gf, gs = ref.unpack_w(int(out[3]))
        assert (gn, gf, gs) == (n, frames, stale), (acc, prev, A, M, (gn, gf, gs), (n, frames, stale))
        assert all(abs(float(out[k]) - sums[k]) <= 1.0 for k in range(3)), (acc, prev, A, M, out, sums)
        pf = ref.unpack_w(prev[3])[1]
        seen["evicted"] += want_clear
        seen["first"] += prev == (0, 0, 0, 0)
        seen["below"] += (not want_clear) and pf + 1 <= A
        seen["above"] += (not want_clear) and pf + 1 > A
        seen["stale"] += (not want_clear) and acc[3] == 0
        seen["halved"] += (not want_clear) and (acc[3] + ref.unpack_w(prev[3])[0]) * min(A, pf + 1) // (pf + 1) > 65535
    assert all(v > 0 for v in seen.values()), seen
    rgb = np.zeros(3, np.float32)
    lib.sh_host_radiance(p(np.array([2048, 1024, 512, voxel_w(4, 3, 1)], np.uint32)), 1, p(rgb))
    assert list(rgb) == [0.5, 0.25, 0.125]


def test_query_validity_rule(shims):
    lib = shims[0]
    dist = np.array([0.01, 0.1, 0.27, 0.28, 0.5, 1.0, 3.0, 10.0, 100.0], np.float32)
    rough = np.array([0.0, 0.05, 0.3, 0.5, 0.7, 0.9, 0.98, 0.99, 1.0, 1.7, 3.0], np.float32)
    d, r = (a.ravel() for a in np.meshgrid(dist, rough, indexing="ij"))
    voxel = np.full(len(d), 0.16, np.float32)
    pr = np.ascontiguousarray(r.copy())
    valid = np.zeros(len(d), np.uint32)
    lib.sh_host_valid_hit(p(np.ascontiguousarray(d)), p(voxel), p(pr), len(d), p(valid))
    assert (pr == np.minimum(r, np.float32(0.99))).all(), "previousRoughness is clamped to 0.99"
    checked = 0
    for i in range(len(d)):
        want, footprint = ref.valid_hit(float(d[i]), float(voxel[i]), float(r[i]))
        margin = min(abs(float(d[i]) / (float(voxel[i]) * math.sqrt(3.0)) - 1.0), abs(footprint / float(voxel[i]) - 1.0))
        if margin > 1e-5:  # away from both thresholds the float32 rule and the restatement must agree
            assert bool(valid[i]) == want, (d[i], r[i], footprint)
            checked += 1
    assert checked >= len(d) - 2 and valid.any() and not valid.all()
    assert not valid[r == 0].any(), "a primary hit (accumulated roughness 0) never reads the cache"
    assert valid[(d == 100.0) & (r >= 0.99)].all()


# ---------------------------------------------------------------------------------------------------- CPU: frames of the test scene
W, H = 48, 32


@pytest.fixture(scope="module")
def cpu_scene(dxrs, host):
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(W, H, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70), jitter=False)
    return spheres, mats, sd, cam


@pytest.mark.parametrize("spp", [1, 3])
def test_empty_cache_is_the_identity(dxrs, shims, cpu_scene, spp):
    spheres, mats, sd, cam = cpu_scene
    hc = HostCache(*shims, spheres, mats, sd)
    gs = dxrs.types.graphics_settings(W, H, frame_index=5, bounces=8, spp=spp)
    off, rays_off, _ = hc.call(cam, gs, cache=False)
    on, rays_on, _ = hc.call(cam, gs, stages=QUERY, reset_history=True)
    assert np.array_equal(off.view(np.uint32), on.view(np.uint32)) and rays_on == rays_off
    assert np.isfinite(off).all() and rays_off > W * H and len(np.unique(off[..., 0])) > W * H // 4


def test_three_host_frames_fill_age_and_never_duplicate(dxrs, shims, cpu_scene):
    spheres, mats, sd, cam = cpu_scene
    hc = HostCache(*shims, spheres, mats, sd)
    occupied = []
    for f in range(3):
        img, rays, failed = hc.call(cam, dxrs.types.graphics_settings(W, H, frame_index=f, bounces=8, spp=1), capacity=1 << 12, reset_history=f == 0)
        content = hc.content()
        assert failed == 0 and np.isfinite(img).all() and rays > W * H
        assert all(ref.unpack_w(v[3])[1] <= f + 1 for v in content.values())
        occupied.append(len(content))
    assert occupied[0] > 50 and occupied[2] >= occupied[0]
    assert any(ref.unpack_w(v[3])[2] > 0 for v in content.values()) and any(ref.unpack_w(v[3])[0] >= 3 for v in content.values())


# The cache's content is the path tracer's own estimate.  Scene scale 5 (voxels of 1.6 units around the camera's distance: a few hundred
# voxels, each met by several paths per frame), every path of the 48 x 32 grid (DownscaleFactor 1), K = 96 resting frames inside an
# accumulation window of 128, so that every frame counts alike.  The cache-off estimator: the update pass's own paths for 64 other frame
# indices (98304 paths), each followed to its end by sh_path_radiance and booked to the voxel of its first vertex.
K_FRAMES, EST_FRAMES, N_VOXELS = 96, 64, 8


def test_cache_content_is_the_path_traced_estimate(dxrs, shims, cpu_scene):
    lib = shims[0]
    spheres, mats, sd, cam = cpu_scene
    hc = HostCache(*shims, spheres, mats, sd)
    st = dict(capacity=1 << 12, downscale_factor=1, scene_scale=5.0, accumulation_frames=128, stages=UPDATE | RESOLVE)
    for f in range(K_FRAMES):
        _, _, failed = hc.call(cam, dxrs.types.graphics_settings(W, H, frame_index=f, bounces=8, spp=1, threshold=0.0), reset_history=f == 0, **st)
        assert failed == 0
    content = hc.content()
    gs = dxrs.types.graphics_settings(W, H, frame_index=0, bounces=16, spp=1, threshold=0.0)
    s = defaults(**st)
    prm = np.array([W, H, 0, gs.Bounces, 1, 1, s["capacity"], 1, 128, 64, 0, 7, 0, 0, W, H], np.uint32)
    fprm = np.array([0.0, s["scene_scale"], s["roughness_threshold"]], np.float32)
    frames = np.arange(1000, 1000 + EST_FRAMES, dtype=np.uint32)
    n = EST_FRAMES * W * H
    keys, rgb = np.zeros(n, np.uint64), np.zeros((n, 3), np.float32)
    lib.sh_host_estimates(p(hc.spheres), p(hc.mats), len(spheres), p(hc.env), C.addressof(cam), p(prm), p(fprm), p(frames), EST_FRAMES, p(keys), p(rgb))
    uniq, counts = np.unique(keys[keys != 0], return_counts=True)
    chosen = [int(k) for k in uniq[np.argsort(-counts)][:N_VOXELS]]
    worst = 0.0
    for k in chosen:
        x = rgb[keys == np.uint64(k)].astype(np.float64)
        half = len(x) // 2
        mean, se = x.mean(axis=0), x.std(axis=0, ddof=1) / math.sqrt(len(x))
        a, b = x[:half], x[half:]
        se_ab = np.sqrt(a.var(axis=0, ddof=1) / len(a) + b.var(axis=0, ddof=1) / len(b))
        assert (np.abs(a.mean(axis=0) - b.mean(axis=0)) <= 5 * se_ab).all(), "the cache-off estimator alone is not stable under the bound"
        assert k in content, "a voxel every frame's paths meet is missing from the cache"
        v = content[k]
        samples = ref.unpack_w(v[3])[0]
        cached = np.array(v[:3], np.float64) / (samples * ref.RADIANCE_SCALE)
        dev = np.abs(cached - mean) / se
        print(f"voxel {k:#x}: {len(x)} estimates, {samples} cached samples, cache {cached}, path traced {mean} +- {se}, deviation {dev} standard errors")
        assert samples > 200 and len(x) > 500
        worst = max(worst, float(dev.max()))
    assert worst <= 5.0, f"a voxel's radiance is {worst:.2f} standard errors from the path-traced mean"


# ---------------------------------------------------------------------------------------------------- CPU: sanitizers
def test_sanitized_stand_alone_program(tmp_path):
    """update, resolve and query of the host header for three frames, with an eviction and an overflowing bucket, under ASan + UBSan, in a
    child process (nothing sanitised is loaded into Python)"""
    exe = str(tmp_path / "sharc_sanitize")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-o", exe, "sharc_sanitize.cpp"], cwd=os.path.join(HERE, "hostshim"), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout


# ---------------------------------------------------------------------------------------------------- GPU
GW, GH, CAP = 96, 64, 1 << 16


def c1(dxrs, host, **cam_kw):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    return spheres, mats, sd, host.camera_matrices(GW, GH, **cam_kw)


def setup(r, dxrs, spheres, mats, sd, cam, gs, textures=None):
    r.set_scene(spheres, mats, sd)
    r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(gs)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def gpu_content(r, capacity=CAP):
    return cache_map(*r.sharc_download(capacity))


def check_empty_cache(dxrs, r, spheres, mats, sd, cam, spp, rect=None):
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=3, bounces=8, spp=spp)
    setup(r, dxrs, spheres, mats, sd, cam, gs)
    want, ws = r.render(rect)
    got, s = r.render_sharc(rect, **defaults(stages=QUERY, reset_history=True))
    assert same_bits(got, want), f"{int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} pixels differ from pt_render"
    assert s.rays == ws.rays, (s.rays, ws.rays)
    assert not gpu_content(r), "a query leaves the cache empty"


@pytest.mark.gpu
@pytest.mark.parametrize("spp,rect", [(1, None), (3, None), (1, (5, 3, 67, 45))])
def test_gpu_empty_cache_equals_pt_render(dxrs, host, renderer, spp, rect):
    check_empty_cache(dxrs, renderer, *c1(dxrs, host), spp, rect)


@pytest.mark.gpu
def test_gpu_empty_cache_equals_pt_render_scene_in_global_memory(dxrs, host):
    r = dxrs.Renderer(device=0, flags=dxrs.types.PT_FLAG_NO_LDS_SCENE)
    try:
        check_empty_cache(dxrs, r, *c1(dxrs, host), 1)
        assert not r.accel.lds_resident
    finally:
        r.close()


def frames_against_host(dxrs, r, hc, spheres, mats, sd, cams, textures=None, bounces=8, **kw):
    """consecutive pt_render_sharc calls against the host header: the cache as a map after each, the image and the ray count"""
    for f, cam in enumerate(cams):
        gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=bounces, spp=1)
        if f == 0:
            setup(r, dxrs, spheres, mats, sd, cam, gs, textures)
        r.set_camera(cam)
        r.set_constants(gs)
        st = defaults(reset_history=f == 0, **kw)
        got, s = r.render_sharc(**st)
        want, rays, failed = hc.call(cam, gs, **st)
        assert failed == 0, "the capacity must be chosen so that the host run has no failed insert"
        g, h = gpu_content(r, st["capacity"]), hc.content()
        assert set(g) == set(h), f"frame {f}: {len(set(g) ^ set(h))} keys differ"
        bad = [k for k in g if g[k] != h[k]]
        assert not bad, f"frame {f}: {len(bad)} of {len(g)} voxels differ, first {bad[0]:#x}: {g[bad[0]]} != {h[bad[0]]}"
        assert len(g) > 100
        assert same_bits(got, want), f"frame {f}: {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} pixels differ from the host header"
        assert s.rays == rays, (f, s.rays, rays)


@pytest.mark.gpu
def test_gpu_update_and_resolve_equal_the_host_header(dxrs, host, renderer, shims):
    spheres, mats, sd, cam = c1(dxrs, host)
    moved = host.camera_matrices(GW, GH, position=(1.5, 0.5, -14.0), look_at=(0.0, 0.0, 0.0), previous=cam)
    frames_against_host(dxrs, renderer, HostCache(*shims, spheres, mats, sd), spheres, mats, sd, [cam, cam, moved])


@pytest.mark.gpu
def test_gpu_query_over_a_warm_cache(dxrs, host, renderer, shims):
    """the host query over exactly the arrays the device holds; uploaded again, the device's frame stays what it was"""
    spheres, mats, sd = make_scene(dxrs)
    cam = host.camera_matrices(GW, GH, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70))
    hc = HostCache(*shims, spheres, mats, sd)
    for f in range(4):
        gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=2)
        if f == 0:
            setup(renderer, dxrs, spheres, mats, sd, cam, gs)
        renderer.set_constants(gs)
        renderer.render_sharc(**defaults(reset_history=f == 0, stages=UPDATE | RESOLVE))
    keys, voxels = renderer.sharc_download(CAP)
    hc.install(keys, voxels)
    got, s = renderer.render_sharc(**defaults(stages=QUERY))
    want, rays, _ = hc.call(cam, gs, stages=QUERY)
    off, rays_off, _ = hc.call(cam, gs, cache=False)
    assert same_bits(got, want) and s.rays == rays
    assert rays < rays_off and not same_bits(want, off), "the warm cache ends paths"
    renderer.sharc_upload(keys, voxels)
    again, s2 = renderer.render_sharc(**defaults(stages=QUERY))
    assert same_bits(again, got) and s2.rays == s.rays
    vis, _ = renderer.render_sharc(**defaults(stages=QUERY, visualize=True))
    wv, _, _ = hc.call(cam, gs, stages=QUERY, visualize=True)
    assert same_bits(vis, wv) and not same_bits(vis, got)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [CAP, 64])
def test_gpu_eviction(dxrs, host, renderer, capacity):
    """after the camera jumps far away the old voxels age out; at four buckets inserts fail, and only order-free invariants hold"""
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=8, spp=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    st = defaults(capacity=capacity, max_stale_frames=2)
    renderer.render_sharc(reset_history=True, **{k: v for k, v in st.items() if k != "reset_history"})
    first = set(gpu_content(renderer, capacity))
    assert first and (capacity != CAP or len(first) > 100)
    far = host.camera_matrices(GW, GH, position=(0.0, 4000.0, -12000.0), look_at=(0.0, 0.0, 0.0), previous=cam)
    renderer.set_camera(far)
    for f in range(1, 4):
        renderer.set_constants(dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1))
        img, _ = renderer.render_sharc(**st)
        now = gpu_content(renderer, capacity)  # (asserts that no key appears twice)
        assert np.isfinite(img).all() and len(now) <= capacity
        if capacity == CAP:
            assert bool(first & set(now)) == (f < 3), f"frame {f}: {len(first & set(now))} of the old keys are left"


@pytest.mark.gpu
def test_gpu_restart_rules(dxrs, host, renderer):
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=8, spp=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    fill = defaults(stages=UPDATE | RESOLVE)

    def frames_of(content):
        return max(ref.unpack_w(v[3])[1] for v in content.values())

    renderer.render_sharc(**dict(fill, reset_history=True))
    renderer.render_sharc(**fill)
    assert frames_of(gpu_content(renderer)) == 2
    renderer.render_sharc(**dict(fill, reset_history=True))
    assert frames_of(gpu_content(renderer)) == 1, "ResetHistory restarts the cache"
    renderer.render_sharc(**fill)
    renderer.set_scene(spheres, mats, sd)
    renderer.render_sharc(**fill)
    assert frames_of(gpu_content(renderer)) == 1, "pt_set_scene restarts the cache"
    renderer.render_sharc(**dict(fill, capacity=1 << 15))
    assert frames_of(gpu_content(renderer, 1 << 15)) == 1, "a capacity change restarts the cache"
    with pytest.raises(dxrs.PtError) as e:
        renderer.sharc_download(CAP)
    assert e.value.status == 1
    renderer.render_sharc(**dict(fill, capacity=1 << 15))
    assert frames_of(gpu_content(renderer, 1 << 15)) == 2


@pytest.mark.gpu
def test_gpu_argument_errors(dxrs, host, renderer):
    from dxrs_amd.abi_types import PtSharcSettings, PtStats
    spheres, mats, sd, cam = c1(dxrs, host)
    gs = dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=4, spp=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, gs)
    want, _ = renderer.render()
    lib, ctx = renderer._lib, renderer._ctx
    out = np.full((GH, GW, 4), 7.0, np.float32)
    ok = PtSharcSettings(Capacity=CAP, DownscaleFactor=2, Stages=QUERY, ResetHistory=1)
    assert lib.pt_render_sharc(ctx, None, out.ctypes.data, 0, None, None) == 1, "null settings"
    assert lib.pt_render_sharc(ctx, None, None, 0, C.byref(ok), None) == 1, "null output"
    for field, value, status in (("DownscaleFactor", 5, 1), ("SceneScale", 4.0, 1), ("SceneScale", 101.0, 1), ("SceneScale", float("nan"), 1), ("Capacity", 3 << 10, 1),
                                 ("Capacity", 8, 1), ("RoughnessThreshold", 1.5, 1), ("AccumulationFrames", 256, 1), ("MaxStaleFrames", 255, 1), ("Stages", 8, 1),
                                 ("IsAntiFireflyEnabled", 1, 5)):
        s = PtSharcSettings(Capacity=CAP, DownscaleFactor=2, Stages=QUERY, ResetHistory=1)
        setattr(s, field, value)
        assert lib.pt_render_sharc(ctx, None, out.ctypes.data, 0, C.byref(s), None) == status, (field, value)
        assert renderer._lib.pt_last_error(ctx)
    from dxrs_amd.abi_types import PtRect
    bad = PtRect(90, 0, 10, 10)
    assert lib.pt_render_sharc(ctx, C.byref(bad), out.ctypes.data, 0, C.byref(ok), None) == 1, "a rect outside RenderSize"
    renderer.set_constants(dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=4, spp=1, di=True))
    assert lib.pt_render_sharc(ctx, None, out.ctypes.data, 0, C.byref(ok), None) == 5, "IsDIEnabled"
    dn = dxrs.types.graphics_settings(GW, GH, frame_index=0, bounces=4, spp=1)
    dn.Denoiser = 2
    assert lib.pt_set_constants(ctx, C.byref(dn)) == 5, "Denoiser (refused where the constants are set)"
    assert (out == 7.0).all(), "a refused call writes nothing"
    renderer.set_constants(gs)
    got, _ = renderer.render_sharc(**defaults(stages=QUERY, reset_history=True))
    assert same_bits(got, want), "the context renders a correct frame after the refusals"


@pytest.mark.gpu
def test_gpu_interleaved_with_frames_in_flight(dxrs, host, shims):
    """pt_render frames in flight on other lanes while pt_render_sharc calls run: both results are what they are alone"""
    import torch
    spheres, mats, sd, cam = c1(dxrs, host)
    hc = HostCache(*shims, spheres, mats, sd)
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        gs = [dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1) for f in range(3)]
        setup(r, dxrs, spheres, mats, sd, cam, gs[0])
        alone = []
        for f in range(3):
            r.set_constants(gs[f])
            alone.append(r.render()[0])
        dev = torch.device("cuda", 0)
        frames = [torch.zeros((GH, GW, 4), dtype=torch.float32, device=dev) for _ in range(3)]
        cached = [torch.zeros((GH, GW, 4), dtype=torch.float32, device=dev) for _ in range(3)]
        torch.cuda.synchronize(dev)
        for f in range(3):
            r.set_constants(gs[f])
            r.render_sharc_device(cached[f].data_ptr(), **defaults(reset_history=f == 0))
            r.render_device(frames[f].data_ptr())
        r.synchronize()
        for f in range(3):
            want, _, failed = hc.call(cam, gs[f], **defaults(reset_history=f == 0))
            assert failed == 0
            assert same_bits(frames[f].cpu().numpy(), alone[f]), f"frame {f}: pt_render changed"
            assert same_bits(cached[f].cpu().numpy(), want), f"frame {f}: pt_render_sharc differs from the host header"
        g, h = gpu_content(r), hc.content()
        assert g == h
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_textured_scene(dxrs, host, renderer, shims):
    """the alpha-tested golden scene (tests/golden_cases.py, row a5): the kTex / kAlpha instances, one frame against the host header"""
    import golden_cases
    case = next(c for c in golden_cases.cases(dxrs, host) if c["file"].startswith("a5_alpha"))
    cam = host.camera_matrices(GW, GH, position=(0.0, 2.0, -7.0), jitter_index=1)
    hc = HostCache(*shims, case["spheres"], case["materials"], case["sd"], textures=case["textures"])
    try:
        frames_against_host(dxrs, renderer, hc, case["spheres"], case["materials"], case["sd"], [cam], textures=case["textures"], bounces=5)
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_textured_scene_without_alpha_test(dxrs, host, renderer, shims):
    """the test scene with an emissive map on an emitter and nothing alpha-tested: the textured instances with the plain walk (tree in LDS)"""
    from dxrs_amd.textures import TextureSet
    spheres, mats, sd = make_scene(dxrs)
    ts = TextureSet(len(spheres))
    yy, xx = np.mgrid[0:32, 0:64]
    checker = ((xx // 4 + yy // 4) & 1).astype(np.uint8)
    glow = np.zeros((32, 64, 4), np.uint8)
    glow[..., 0], glow[..., 1], glow[..., 2], glow[..., 3] = 255, 80 + 175 * checker, 40 + 215 * checker, 255
    ts.maps[1, 1] = ts.add_image(glow)  # TEXTURE_MAP_EMISSIVE_COLOR of emitter E0
    cam = host.camera_matrices(GW, GH, position=(0.0, 2.5, -9.0), look_at=(0.0, 1.0, 0.0), hfov=math.radians(70))
    try:
        frames_against_host(dxrs, renderer, HostCache(*shims, spheres, mats, sd, textures=ts), spheres, mats, sd, [cam, cam], textures=ts)
        assert renderer.accel.lds_resident
    finally:
        renderer.set_textures(None)


@pytest.mark.gpu
def test_gpu_tree_with_32_bit_stack(dxrs, host):
    """40,000 spheres: more than 32,767 nodes, so the instances with the 32-bit traversal stack run (the tree in global memory).  The
    query over an empty cache against pt_render; then whole calls, checked by what does not need the host's brute-force trace"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=40000)
    cam = host.camera_matrices(GW, GH)
    r = dxrs.Renderer(device=0)
    try:
        check_empty_cache(dxrs, r, spheres, mats, sd, cam, 1)
        assert r.accel.node_count >= 32767 and not r.accel.lds_resident
        for f in range(2):
            r.set_constants(dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1))
            img, s = r.render_sharc(**defaults(reset_history=f == 0))
            content = gpu_content(r)  # (asserts that no key appears twice)
            assert np.isfinite(img).all() and len(content) > 100 and s.rays > GW * GH
        assert max(ref.unpack_w(v[3])[1] for v in content.values()) == 2
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_the_cache_ends_paths(dxrs, host, renderer):
    """C1 with a rough ground: after 8 resting frames the query traces strictly fewer rays than pt_render does for the same frame"""
    spheres, mats, sd, cam = c1(dxrs, host)
    mats = mats.copy()
    ground = int(np.argmax(spheres["r"]))
    mats["Roughness"][ground], mats["Metallic"][ground] = 0.9, 0.0
    for f in range(8):
        gs = dxrs.types.graphics_settings(GW, GH, frame_index=f, bounces=8, spp=1)
        if f == 0:
            setup(renderer, dxrs, spheres, mats, sd, cam, gs)
        renderer.set_constants(gs)
        renderer.render_sharc(**defaults(reset_history=f == 0, stages=UPDATE | RESOLVE))
    _, plain = renderer.render()
    img, s = renderer.render_sharc(**defaults(stages=QUERY))
    assert np.isfinite(img).all() and s.rays < plain.rays, (s.rays, plain.rays)
