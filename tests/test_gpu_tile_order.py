"""The primary pass over a view with beam lists (csrc/pt_trace.h bounce_kernel): every workgroup draws its tiles with a non-empty
list first (PT_TILE_ORDER=0: slot order) and a tile with an empty list takes a short path (PT_SKY_FAST=0: the general one).  Neither changes a
lane's arithmetic, so every frame must equal, bit for bit and with equal ray, path and pixel totals, the frame of a context created with both
knobs off, and the CPU oracle's.  Every case renders a resting view until the lists are in use, and says so."""
import math
import os

import numpy as np
import pytest

from util import bits, count_mismatch

pytestmark = pytest.mark.gpu

OFF = {"PT_TILE_ORDER": "0", "PT_SKY_FAST": "0"}
SEPARATE = {"PT_FUSE_LOOP": "0"}                                    # the looping pass as a launch of its own
FEW_GROUPS = {"PT_FUSE_LOOP": "0", "PT_TRAVERSE_BLOCKS_PER_CU": "1"}  # ... and workgroups that visit several batches (a table of 16 and more tiles)
BOUNCES = 8
DLSS_RR = 1  # abi_types.DENOISER_DLSS_RR


def _context(dxrs, env, **kw):
    """A context created under `env` (the knobs are read once, at pt_create)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return dxrs.Renderer(device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def pair(dxrs):
    """base env -> (context with the defaults, context with both knobs off)"""
    made = {}

    def get(base=None):
        base = dict(base or {})
        key = tuple(sorted(base.items()))
        if key not in made:
            assert not any(k in os.environ for k in ("PT_TILE_ORDER", "PT_SKY_FAST", "PT_TILE_TABLE"))  # (the defaults are what is under test)
            made[key] = (_context(dxrs, base), _context(dxrs, {**base, **OFF}))
        return made[key]

    yield get
    for on, off in made.values():
        on.close()
        off.close()


def _copy(struct):
    return type(struct).from_buffer_copy(struct)


def _rested(r, scene, cam, gs, textures=None):
    """The view rendered until its primary-beam lists are in use (the third frame of a resting view) -> (image, stats of that frame)"""
    r.set_scene(*scene)
    if textures is not None:
        r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(gs)
    r.render()
    r.render()
    img, st = r.render()
    if textures is not None:
        r.set_textures(None)
    assert st.beams_used, "the resting view's lists are not in use"
    return img, st


def _same_totals(a, b):
    assert (a.rays, a.paths, a.pixels) == (b.rays, b.paths, b.pixels)


def _check(dxrs, host, oracle, contexts, scene, cam, w, h, spp=1, frame=0, textures=None):
    gs = dxrs.types.graphics_settings(w, h, frame_index=frame, bounces=BOUNCES, spp=spp)
    on, off = contexts
    img, st = _rested(on, scene, cam, gs, textures)
    img0, st0 = _rested(off, scene, cam, gs, textures)
    ref, ost = oracle.render(*scene, cam, gs, threads=8, textures=textures)
    _same_totals(st, st0)
    assert st.rays == ost.rays and st.pixels == w * h and st.paths == w * h * spp
    assert np.array_equal(bits(img), bits(img0))
    assert count_mismatch(img, ref) == 0
    return ref, ost


@pytest.mark.parametrize("base", [SEPARATE, FEW_GROUPS], ids=["one_batch", "several_batches"])
def test_separate_looping_pass(dxrs, host, oracle, pair, base):
    """640x384 (80 x 48 blocks): workgroups with sky and ground tiles, those at the horizon with both"""
    w, h = 640, 384
    _check(dxrs, host, oracle, pair(base), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=1), w, h, frame=1)


def test_fused_form(dxrs, host, oracle, pair):
    w, h = 256, 256
    _check(dxrs, host, oracle, pair(), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=2), w, h, frame=2)


@pytest.mark.parametrize("base", [None, FEW_GROUPS], ids=["fused", "separate"])
def test_ragged_size(dxrs, host, oracle, pair, base):
    """333x197: partial 8x8 blocks on two edges, so sky tiles with invalid lanes, and a last batch that is not full"""
    w, h = 333, 197
    _check(dxrs, host, oracle, pair(base), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=3), w, h, frame=3)


def _corner_rays(cam):
    f = np.array(cam.ForwardDirection[:], np.float64)
    r = np.array(cam.RightDirection[:], np.float64)
    u = np.array(cam.UpDirection[:], np.float64)
    d = np.array([f + sx * r + sy * u for sx in (-1, 1) for sy in (-1, 1)])
    return np.tile(np.array(cam.Position[:], np.float32), (4, 1)), (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)


@pytest.mark.parametrize("base", [None, FEW_GROUPS], ids=["fused", "separate"])
def test_all_sky_and_all_ground(dxrs, host, oracle, pair, base):
    """A camera pitched up so that every tile is sky (the table is all light), then one looking down at the ground sphere (all heavy)"""
    w, h = 200, 136
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    up = host.camera(w, h, position=(0.0, 30.0, -15.0), look_at=(0.0, 130.0, -5.0), hfov=math.radians(40.0))
    ref, ost = _check(dxrs, host, oracle, pair(base), scene, up, w, h)
    assert ost.rays == w * h  # no primary ray hits anything
    down = host.camera(w, h, position=(0.0, 6.0, -15.0), look_at=(0.0, -60.0, -11.0), hfov=math.radians(40.0))
    # the directions that hit a sphere form a convex cone: the four corners of the frustum hit the largest sphere, so every primary ray hits something
    ground = scene[0][[int(np.argmax(scene[0]["r"]))]]
    o, d = _corner_rays(down)
    t, ids = oracle.closest_hits(ground, o, d, use_bvh=False)
    assert (ids == 0).all() and np.isfinite(t).all()
    _check(dxrs, host, oracle, pair(base), scene, down, w, h, frame=1)


@pytest.mark.parametrize("base", [None, SEPARATE], ids=["fused", "separate"])
def test_several_samples(dxrs, host, oracle, pair, base):
    """320x200 at 4 spp: these instances keep the slot order and the general path (a primary miss also leaves the pixel's primary-hit record,
    which the looping pass reads when it regenerates a sample); what they share with the 1-spp instances -- the staging barrier, the hand-over
    that a wave without survivors skips -- is the same with the knobs on and off"""
    w, h = 320, 200
    _check(dxrs, host, oracle, pair(base), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=4), w, h, spp=4, frame=4)


def test_constant_environment_colour(dxrs, host, oracle, pair):
    """EnvironmentLightColor.a >= 0: the short path stores the colour, not the sky"""
    w, h = 256, 160
    spheres, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    sd = _copy(sd)
    sd.EnvironmentLightColor[0], sd.EnvironmentLightColor[1], sd.EnvironmentLightColor[2], sd.EnvironmentLightColor[3] = 0.7, 0.8, 1.1, 1.0
    ref, _ = _check(dxrs, host, oracle, pair(), (spheres, materials, sd), host.camera(w, h, jitter_index=5), w, h, frame=5)
    assert (bits(ref[0, :, :3]) == bits(np.array([0.7, 0.8, 1.1], np.float32))).all()  # (the top row is environment)


def test_environment_map(dxrs, host, oracle, pair):
    """A lat-long environment map: the textured instances keep the general path, and the tile order applies"""
    w, h = 256, 160
    spheres, materials, _ = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    tex, sd_env = host.demo_textures(0, 0.0, textured=False, environment_map=True, return_scene_data=True)
    _check(dxrs, host, oracle, pair(), (spheres, materials, sd_env), host.camera(w, h, jitter_index=6), w, h, frame=6, textures=tex)


def test_moving_camera(dxrs, host, oracle, pair):
    """Rest, travel, rest: frames with exact lists, frames with none (slot order, no short path) and frames with widened lists"""
    w, h = 320, 200
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    on, off = pair(SEPARATE)
    positions = [(0.0, 0.0, -15.0)] * 3 + [(0.4 * k, 0.1 * k, -15.0 + 0.5 * k) for k in range(1, 4)] + [(1.2, 0.3, -13.5)] * 3
    used = []
    for r in (on, off):
        r.set_scene(*scene)
    for k, pos in enumerate(positions):
        cam = host.camera(w, h, position=pos, jitter_index=0)
        gs = dxrs.types.graphics_settings(w, h, frame_index=k, bounces=BOUNCES, spp=1)
        frames = []
        for r in (on, off):
            r.set_camera(cam)
            r.set_constants(gs)
            img, st = r.render()
            frames.append((np.array(img, copy=True), st))
        (img, st), (img0, st0) = frames
        ref, ost = oracle.render(*scene, cam, gs, threads=8)
        _same_totals(st, st0)
        assert st.rays == ost.rays and bool(st.beams_used) == bool(st0.beams_used)
        assert np.array_equal(bits(img), bits(img0)) and count_mismatch(img, ref) == 0, k
        used.append(bool(st.beams_used))
    assert used[2] and used[-1] and not all(used), used


def test_tile_partition(dxrs, host, oracle, pair):
    """render_tiles (slot -> pixel mode 1): an interleaved share of a frame whose right and bottom tiles are padded"""
    import torch
    from dxrs_amd import tiles
    w, h = 333, 197
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera(w, h, jitter_index=7)
    gs = dxrs.types.graphics_settings(w, h, frame_index=7, bounces=BOUNCES, spp=1)
    ref, _ = oracle.render(*scene, cam, gs, threads=8)
    want = tiles.pack_range(ref, 1, 1, 3)
    got = []
    for r in pair():
        r.set_scene(*scene)
        r.set_camera(cam)
        r.set_constants(gs)
        try:
            r.set_partition(1, 3)
            assert r.tiles_count(1) == want.shape[0]
            packed = torch.full((want.shape[0] * 1024, 4), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for _ in range(3):
                st = r.render_tiles(packed.data_ptr(), want_stats=True)
            assert st.beams_used
            got.append((packed.cpu().numpy().reshape(want.shape), st))
        finally:
            r.set_partition(0, 1)
    (img, st), (img0, st0) = got
    _same_totals(st, st0)
    assert np.array_equal(bits(img), bits(img0))  # (all four channels: the padding pixels are written as zeros)
    assert np.array_equal(bits(img)[..., :3], bits(want)[..., :3])


def test_denoiser_frame(dxrs, host, oracle, pair):
    """A DLSS-RR frame of pt_render_denoiser: its radiance is pt_render's, its hit distances are the same with the knobs on and off"""
    w, h = 256, 256
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera(w, h, jitter_index=2)
    gs = dxrs.types.graphics_settings(w, h, frame_index=2, bounces=BOUNCES, spp=1)
    ref, ost = oracle.render(*scene, cam, gs, threads=8)
    got = []
    for r in pair():
        r.set_scene(*scene)
        r.set_camera(cam)
        r.set_constants(gs)
        r.render_denoiser(DLSS_RR)
        r.render_denoiser(DLSS_RR)
        r.totals(reset=True)
        out, bufs = r.render_denoiser(DLSS_RR, fill=-7.0)
        tot = r.totals(reset=True)
        assert tot.beams_used == 1
        got.append((out, bufs, tot))
    (out, bufs, tot), (out0, bufs0, tot0) = got
    _same_totals(tot, tot0)
    assert tot.rays == ost.rays
    assert np.array_equal(bits(out), bits(out0)) and count_mismatch(out, ref) == 0
    assert sorted(bufs) == sorted(bufs0)
    for name in bufs:
        assert np.array_equal(bits(bufs[name]), bits(bufs0[name])), name


def test_table_fallback(dxrs, host):
    """PT_TILE_TABLE=4: every workgroup of a 256x256 frame visits 8 tiles, more than the table may hold, and keeps the slot order"""
    w, h = 256, 256
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera(w, h, jitter_index=2)
    gs = dxrs.types.graphics_settings(w, h, frame_index=2, bounces=BOUNCES, spp=1)
    got = []
    for env in ({"PT_TILE_TABLE": "4"}, OFF):
        r = _context(dxrs, env)
        try:
            got.append(_rested(r, scene, cam, gs))
        finally:
            r.close()
    (img, st), (img0, st0) = got
    _same_totals(st, st0)
    assert np.array_equal(bits(img), bits(img0))
