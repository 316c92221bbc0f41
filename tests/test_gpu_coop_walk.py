"""The cooperative tree walk of the 1-spp looping pass (csrc/pt_trace.h closest_hit_coop): a wave with at most 32 live paths
splits each ray's walk over 2, 4 or 8 lanes; with more it walks per lane.  A closest-hit query does not depend on the order of its tests, so
frames of the default context must equal, bit for bit and with equal ray counts, those of a context created with PT_COOP_WALK=0 and those
of the CPU oracle -- in the separate looping pass (PT_FUSE_LOOP=0) and in the fused form's tail (PT_FUSE_LOOP=1)."""
import os

import numpy as np
import pytest

from util import context_under as _context, count_mismatch

gpu = pytest.mark.gpu

SIZES = [(64, 40), (136, 72)]
FRAMES = (0, 1, 2)
BOUNCES = 8


@pytest.fixture(scope="module")
def contexts(dxrs):
    """(coop, fuse) -> context: the walk on (the default) / off, in the separate looping pass (fuse 0) / the fused form's tail (fuse 1)."""
    made = {}

    def get(coop, fuse):
        if (coop, fuse) not in made:
            env = {"PT_FUSE_LOOP": str(fuse)}
            if not coop:
                env["PT_COOP_WALK"] = "0"
            assert coop == 0 or "PT_COOP_WALK" not in os.environ  # (the default is what is under test)
            made[(coop, fuse)] = _context(dxrs, env)
        return made[(coop, fuse)]

    yield get
    for r in made.values():
        r.close()


def glass_scene(dxrs, rng, n=24):
    """Mostly transmissive spheres in front of the camera over a rough ground: paths that reach bounce 8."""
    s = np.zeros(n, dtype=dxrs.SPHERE_DTYPE)
    s["cx"], s["cy"], s["cz"] = rng.uniform(-3, 3, n), rng.uniform(-1.5, 2.0, n), rng.uniform(-8, 2, n)
    s["r"] = rng.uniform(0.3, 1.1, n)
    s[0] = (0.0, -501.5, 0.0, 500.0)
    m = dxrs.types.default_material(n)
    m["BaseColor"][:, :3] = rng.uniform(0.7, 1.0, (n, 3))
    m["Transmission"] = (rng.random(n) < 0.7).astype(np.float32)
    m["Roughness"] = rng.choice([0.0, 0.05, 0.4], n)
    m["Metallic"] = np.where(m["Transmission"] > 0, 0.0, rng.choice([0.0, 1.0], n))
    m["Transmission"][0], m["Metallic"][0], m["Roughness"][0] = 0.0, 0.0, 0.6
    return s, m


def _scene_and_camera(dxrs, host, name, w, h, frame):
    if name == "demo":
        return host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=frame)
    s, m = glass_scene(dxrs, np.random.default_rng(9100))
    return (s, m, host.scene(dxrs.host.SCENE_SMALL)[2]), host.camera(w, h, position=(0.0, 0.8, -14.0), look_at=(0.0, 0.0, -3.0), jitter_index=frame)


def _settings(dxrs, w, h, frame, rr, bounces=BOUNCES):
    return dxrs.types.graphics_settings(w, h, frame_index=frame, bounces=bounces, spp=1, rr=rr)


_oracle_cache = {}


def _oracle_frame(dxrs, host, oracle, name, w, h, frame, rr, rect=None):
    key = (name, w, h, frame, rr, rect)
    if key not in _oracle_cache:
        scene, cam = _scene_and_camera(dxrs, host, name, w, h, frame)
        _oracle_cache[key] = oracle.render(*scene, cam, _settings(dxrs, w, h, frame, rr), rect=rect, threads=8)
    return _oracle_cache[key]


def _render(r, scene, cam, gs, rect=None):
    r.set_scene(*scene)
    r.set_camera(cam)
    r.set_constants(gs)
    return r.render(rect)


# One 8x8 rect is one wave of the primary pass, so every path of it that goes on sits in ONE wave of the looping pass (of the fused tail): that
# wave's live paths at its traces are the rect's rays at depth 2, 3, ... (the primary pass traces depths 0 and 1 itself), which the oracle counts.
SINGLE_WAVE_RECTS = [("glass", 64, 40, (32, 16, 8, 8), True), ("demo", 64, 40, (32, 16, 8, 8), True),
                     ("glass", 136, 72, (68, 32, 8, 8), False), ("demo", 136, 72, (68, 32, 8, 8), True)]


def _live_counts(dxrs, host, oracle, name, w, h, rect, rr):
    """live paths of the rect's one looping wave at each of its traces: rays at depth d = rays(Bounces = d) - rays(Bounces = d - 1)"""
    scene, cam = _scene_and_camera(dxrs, host, name, w, h, 0)
    total = [oracle.render(*scene, cam, _settings(dxrs, w, h, 0, rr, bounces=b), rect=rect, threads=4)[1].rays for b in range(1, BOUNCES + 1)]
    return [total[k] - total[k - 1] for k in range(1, len(total))]


def test_the_cases_reach_every_group_size(dxrs, host, oracle):
    """CPU: the single-wave rects below make waves with 1, 2-8 (k = 8), 9-16 (k = 4), 17-32 (k = 2) and more than 32 (per-lane walk) live paths."""
    seen = set()
    for name, w, h, rect, rr in SINGLE_WAVE_RECTS:
        counts = _live_counts(dxrs, host, oracle, name, w, h, rect, rr)
        print(name, w, h, rect, rr, counts)
        assert counts[0] <= 64
        for n in counts:
            seen.add("0" if n == 0 else "1" if n == 1 else "2-8" if n <= 8 else "9-16" if n <= 16 else "17-32" if n <= 32 else ">32")
    assert {"1", "2-8", "9-16", "17-32", ">32"} <= seen


@gpu
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name,w,h,rect,rr", SINGLE_WAVE_RECTS)
def test_single_wave_rects(dxrs, host, oracle, contexts, name, w, h, rect, rr, fuse):
    scene, cam = _scene_and_camera(dxrs, host, name, w, h, 0)
    gs = _settings(dxrs, w, h, 0, rr)
    ref, ost = _oracle_frame(dxrs, host, oracle, name, w, h, 0, rr, rect)
    for coop in (1, 0):
        img, st = _render(contexts(coop, fuse), scene, cam, gs, rect)
        assert st.rays == ost.rays
        assert count_mismatch(img, ref) == 0


@gpu
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("rr", [True, False])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["demo", "glass"])
def test_small_frames(dxrs, host, oracle, contexts, name, w, h, rr, fuse):
    """Three consecutive frames, with and without Russian roulette: walk on = walk off = oracle."""
    for frame in FRAMES:
        scene, cam = _scene_and_camera(dxrs, host, name, w, h, frame)
        gs = _settings(dxrs, w, h, frame, rr)
        ref, ost = _oracle_frame(dxrs, host, oracle, name, w, h, frame, rr)
        img, st = _render(contexts(1, fuse), scene, cam, gs)
        img0, st0 = _render(contexts(0, fuse), scene, cam, gs)
        assert st.rays == st0.rays == ost.rays
        assert count_mismatch(img, img0) == 0
        assert count_mismatch(img, ref) == 0


def tie_scene(dxrs, kind):
    """coincident: every sphere of a glass cluster twice, the copy (higher id) with another colour.  tangent: a chain of glass spheres that
    touch each other on the view axis (the leaving and the entering crossing share one t), each also present twice."""
    if kind == "coincident":
        s, m = glass_scene(dxrs, np.random.default_rng(9200), 12)
    else:
        s = np.zeros(5, dtype=dxrs.SPHERE_DTYPE)
        s[0] = (0.0, -501.5, 0.0, 500.0)
        for k in range(4):
            s[1 + k] = (0.0, 0.0, -6.0 + 2.0 * k, 1.0)
        m = dxrs.types.default_material(5)
        m["Transmission"][1:], m["Roughness"][1:], m["Roughness"][0] = 1.0, 0.0, 0.6
        m["BaseColor"][1:, :3] = (0.9, 0.95, 1.0)
    s2, m2 = np.concatenate([s, s]), np.concatenate([m, m])
    m2["BaseColor"][len(s):, :3] = (1.0, 0.2, 0.1)
    m2["EmissiveStrength"][len(s):], m2["EmissiveColor"][len(s):, :3] = 3.0, (1.0, 0.0, 0.0)
    return s2, m2


@gpu
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("kind", ["coincident", "tangent"])
def test_ties_go_to_the_lower_id(dxrs, host, oracle, contexts, kind, fuse):
    """Equal t: the lower id, as brute force.  The copies differ in colour and emission, so a wrong id shows in the image."""
    s, m = tie_scene(dxrs, kind)
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    w, h = 65, 41  # (odd: the centre column looks straight down the axis of the tangent chain)
    cam = host.camera(w, h, position=(0.0, 0.0, -14.0), look_at=(0.0, 0.0, 0.0))
    gs = _settings(dxrs, w, h, 0, False)
    ref, ost = oracle.render(s, m, sd, cam, gs, threads=8)
    for coop in (1, 0):
        img, st = _render(contexts(coop, fuse), (s, m, sd), cam, gs)
        assert st.rays == ost.rays
        assert count_mismatch(img, ref) == 0


@gpu
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_degenerate_trees(dxrs, host, oracle, contexts, n, fuse):
    """Trees whose cut at depth 3 has leaves above it and empty slots (a single sphere has no tree at all)."""
    s, m = glass_scene(dxrs, np.random.default_rng(9300 + n), 8)
    keep = [1, 2, 3, 4, 0][:n]  # (the glass first; the ground joins at n = 5)
    s, m = s[keep].copy(), m[keep].copy()
    s["cx"], s["cz"] = np.linspace(-0.8, 0.8, n) if n > 1 else 0.0, -6.0 + 1.5 * np.arange(n)
    if n == 5:
        s[4] = (0.0, -501.5, 0.0, 500.0)
    m["Transmission"][:min(n, 4)], m["Metallic"][:min(n, 4)] = 1.0, 0.0
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    w, h = 64, 40
    cam = host.camera(w, h, position=(0.0, 0.3, -12.0), look_at=(0.0, 0.0, -3.0))
    gs = _settings(dxrs, w, h, n, False)
    ref, ost = oracle.render(s, m, sd, cam, gs, threads=8)
    assert ost.rays > oracle.render(s, m, sd, cam, _settings(dxrs, w, h, n, False, bounces=1), threads=8)[1].rays  # (paths go on past the primary pass)
    for coop in (1, 0):
        img, st = _render(contexts(coop, fuse), (s, m, sd), cam, gs)
        assert st.rays == ost.rays
        assert count_mismatch(img, ref) == 0


@gpu
@pytest.mark.parametrize("fuse", [0, 1])
def test_largest_lds_resident_scene(dxrs, host, oracle, contexts, fuse):
    """The largest scene of test_gpu_fuzz's sweep around the LDS limits that is still staged in LDS (the walk's start table shares that LDS)."""
    from test_gpu_fuzz import random_scene
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    r = contexts(1, fuse)
    for n in (820, 780, 740, 700, 680, 660, 640, 620, 600, 560, 520):
        spheres, materials = random_scene(dxrs, np.random.default_rng(9000 + n), n)
        if r.set_scene(spheres, materials, sd).lds_resident:
            break
    else:
        pytest.fail("no LDS-resident scene in the sweep")
    print(f"largest LDS-resident scene of the sweep: {n} spheres")
    w, h = 96, 64
    cam = host.camera(w, h, position=(0.3, 0.2, -12.0), jitter_index=n)
    gs = _settings(dxrs, w, h, n, True, bounces=5)
    ref, ost = oracle.render(spheres, materials, sd, cam, gs, threads=8)
    for coop in (1, 0):
        img, st = _render(contexts(coop, fuse), (spheres, materials, sd), cam, gs)
        assert st.rays == ost.rays
        assert count_mismatch(img, ref) == 0


@gpu
def test_frames_in_flight_moving_spheres_and_rebuild(dxrs, host, contexts):
    """Three frames in flight: a resting then moving camera, pt_update_spheres between frames (a refit: new boxes, same topology), then another
    scene through pt_build_accel (a new tree: the start table is made from it).  Every frame equals the PT_COOP_WALK=0 context's."""
    w, h = 136, 72
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    off = contexts(0, 0)
    r = _context(dxrs, {"PT_FUSE_LOOP": "0"}, frames_in_flight=3)
    try:
        def same(frame):
            gs = _settings(dxrs, w, h, frame, True)
            r.set_constants(gs)
            off.set_constants(gs)
            img, st = r.render()
            img = np.array(img, copy=True)
            img0, st0 = off.render()
            assert st.rays == st0.rays and count_mismatch(img, img0) == 0

        for x in (r, off):
            x.set_scene(*scene)
            x.set_camera(host.camera(w, h))
        for k in range(4):
            same(k)
        for k in range(4):
            cam = host.camera(w, h, position=(0.05 * (k + 1), 0.0, -15.0 + 0.1 * (k + 1)))
            r.set_camera(cam)
            off.set_camera(cam)
            same(4 + k)
        moved = scene[0].copy()
        for k in range(3):
            moved["cy"][1:] += 0.07
            moved["cx"][1::2] -= 0.05
            r.update_spheres(moved)
            off.update_spheres(moved)
            same(8 + k)
        s, m = glass_scene(dxrs, np.random.default_rng(9400), 30)
        for x in (r, off):
            x.set_scene(s, m, scene[2], build=False)
            x.build_accel()
            x.set_camera(host.camera(w, h, position=(0.0, 0.8, -14.0), look_at=(0.0, 0.0, -3.0)))
        for k in range(3):
            same(11 + k)
    finally:
        r.close()
