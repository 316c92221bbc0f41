"""The tile map of the 1-spp primary pass behind the segmented hand-over (csrc/pt_trace.h bounce_kernel): draw w of workgroup
b is tile b + grid * w (PT_TILE_INTERLEAVE=0: the batch map, eight consecutive tiles per batch), and the order table sorts a workgroup's
tiles into three classes where the view has region records.  Which workgroup traces a tile, and when, changes no lane's arithmetic: every
path owns its pixel and its RNG stream.  So every frame here must equal, bit for bit and with equal ray, path and queue totals, the frame of
a context created with PT_TILE_INTERLEAVE=0, the frame of one created with PT_BEAMS=0 PT_REFL_BEAMS=0 (no lists: every ray traverses, the
slot order), and the CPU oracle's.

The shapes are the smallest at which the map can go wrong: 70x42 (54 tiles in 7 batches: ragged edge tiles, a last batch that is not full,
draws past the end of the frame that must still reach every barrier), 200x120 (the demo's resting view with region records, over several
frames so that the lists are in use), 1920x16 (a block row of 240 tiles, wider than the stride of its grid of 60)."""
import os

import numpy as np
import pytest

from util import bits, context_under as _context, count_mismatch

pytestmark = pytest.mark.gpu

BATCH = {"PT_TILE_INTERLEAVE": "0"}
PLAIN = {"PT_BEAMS": "0", "PT_REFL_BEAMS": "0"}
FUSED, SEPARATE = {"PT_FUSE_LOOP": "1"}, {"PT_FUSE_LOOP": "0"}
BOUNCES = 8
DLSS_RR = 1  # abi_types.DENOISER_DLSS_RR
KNOBS = ("PT_TILE_INTERLEAVE", "PT_TILE_ORDER", "PT_TILE_TABLE", "PT_SKY_FAST", "PT_BEAMS", "PT_REFL_BEAMS", "PT_FUSE_LOOP", "PT_SEG")


@pytest.fixture(scope="module")
def trio(dxrs):
    """base env (and frames in flight) -> (context with the defaults, with the batch map, without lists)"""
    made = {}

    def get(base=None, frames_in_flight=0):
        base = dict(base or {})
        key = (tuple(sorted(base.items())), frames_in_flight)
        if key not in made:
            assert not any(k in os.environ for k in KNOBS)  # (the defaults are what is under test)
            made[key] = tuple(_context(dxrs, {**base, **extra}, frames_in_flight=frames_in_flight) for extra in ({}, BATCH, PLAIN))
        return made[key]

    yield get
    for group in made.values():
        for r in group:
            r.close()


def _rested(r, scene, cam, gs, frames=3):
    """The view rendered `frames` times (its lists are in use from the third frame of a resting view)
    -> (image, stats, queue sizes, region-served waves) of the last frame"""
    r.set_scene(*scene)
    r.set_camera(cam)
    r.set_constants(gs)
    for _ in range(frames - 1):
        r.render()
    r.refl_stats(reset=True)
    img, st = r.render()
    return np.array(img, copy=True), st, r.queue_sizes() if gs.SamplesPerPixel == 1 else None, r.refl_stats(reset=True)[1]


def _check(dxrs, oracle, contexts, scene, cam, w, h, spp=1, frame=0, frames=3, di=False, expect_regions=False):
    gs = dxrs.types.graphics_settings(w, h, frame_index=frame, bounces=BOUNCES, spp=spp, di=di)
    (img, st, q, listed), (img_b, st_b, q_b, listed_b), (img_p, st_p, q_p, listed_p) = (_rested(r, scene, cam, gs, frames) for r in contexts)
    ref, ost = oracle.render(*scene, cam, gs, threads=8)
    assert st.beams_used and st_b.beams_used and not st_p.beams_used and listed_p == 0
    assert listed == listed_b and (listed > 0 or not expect_regions), (listed, listed_b)
    assert (st.rays, st.paths, st.pixels) == (st_b.rays, st_b.paths, st_b.pixels) == (st_p.rays, st_p.paths, st_p.pixels)
    assert st.rays == ost.rays and st.pixels == w * h and st.paths == w * h * spp
    assert q == q_b == q_p, (q, q_b, q_p)
    assert np.array_equal(bits(img), bits(img_b)) and np.array_equal(bits(img), bits(img_p))
    assert count_mismatch(img, ref) == 0


@pytest.mark.parametrize("base", [FUSED, SEPARATE], ids=["fused", "separate"])
@pytest.mark.parametrize("w,h,regions", [(70, 42, False), (200, 120, True), (1920, 16, False)], ids=["70x42", "200x120", "1920x16"])
def test_shapes_and_schedule_forms(dxrs, host, oracle, trio, base, w, h, regions):
    """Every shape with the looping pass fused into the primary launch and as a launch of its own; four frames of the resting view"""
    _check(dxrs, oracle, trio(base), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=1), w, h, frame=1, frames=4, expect_regions=regions)


def test_default_schedule(dxrs, host, oracle, trio):
    """No knob set at all: what a caller gets"""
    w, h = 200, 120
    _check(dxrs, oracle, trio(), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=2), w, h, frame=2, expect_regions=True)


@pytest.mark.parametrize("knob", [{"PT_TILE_TABLE": "4"}, {"PT_TILE_ORDER": "0"}], ids=["table_cap", "table_off"])
def test_slot_order_of_the_interleaved_map(dxrs, host, oracle, trio, knob):
    """PT_TILE_TABLE=4: a workgroup of a 200x120 frame visits 8 tiles, more than the table may hold, and falls back to the slot order;
    PT_TILE_ORDER=0: no table at all.  The draws then walk the interleaved map in w."""
    w, h = 200, 120
    _check(dxrs, oracle, trio({**SEPARATE, **knob}), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=3), w, h, frame=3, expect_regions=True)


@pytest.mark.parametrize("lanes", [1, 3])
def test_frames_in_flight(dxrs, host, oracle, trio, lanes):
    """Six frames of a resting view queued without waiting, on one lane (each frame behind the one before) and on three (overlapped on the
    device), in the default schedule; every frame of the three contexts is the same frame"""
    torch = pytest.importorskip("torch")
    w, h, n = 200, 120, 6
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera(w, h, jitter_index=4)
    gs = dxrs.types.graphics_settings(w, h, frame_index=4, bounces=BOUNCES, spp=1)
    ref, ost = oracle.render(*scene, cam, gs, threads=8)
    got = []
    for r in trio(None, frames_in_flight=lanes):
        r.set_scene(*scene)
        r.set_camera(cam)
        r.set_constants(gs)
        bufs = [torch.empty((h * w, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]
        r.totals(reset=True)
        for b in bufs:
            r.render_device(b.data_ptr())
        r.synchronize()
        tot = r.totals(reset=True)
        got.append(([b.cpu().numpy().reshape(h, w, 4) for b in bufs], tot, r.queue_sizes()))
    (imgs, tot, q), (imgs_b, tot_b, q_b), (imgs_p, tot_p, q_p) = got
    assert tot.beams_used > 0 and tot_b.beams_used > 0 and tot_p.beams_used == 0
    assert (tot.rays, tot.paths) == (tot_b.rays, tot_b.paths) == (tot_p.rays, tot_p.paths) and tot.rays == n * ost.rays
    assert q == q_b == q_p
    for k in range(n):
        assert np.array_equal(bits(imgs[k]), bits(imgs_b[k])) and np.array_equal(bits(imgs[k]), bits(imgs_p[k])), k
        assert count_mismatch(imgs[k], ref) == 0, k


def test_moving_camera_through_a_swap_of_share_built_lists(dxrs, host, oracle, trio):
    """Three frames in flight over a camera in steady travel (tests/test_gpu_list_walk.py): lists built in shares inside the primary passes
    and swapped in; a moving view has no region records, so the table has two classes.  The first lists are made for 32 frames, so a frame
    from the 44th on that uses lists uses a later build's."""
    torch = pytest.importorskip("torch")
    spheres, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h, n, late = 256, 144, 56, 44
    gs = dxrs.types.graphics_settings(w, h, frame_index=0, bounces=3, spp=1)
    cams = [host.camera(w, h, position=(0.004 * k, 0.0, -15.0 + 0.003 * k), jitter_index=k % 8) for k in range(n)]
    out = []
    for r in trio(SEPARATE, frames_in_flight=3):
        r.set_scene(spheres, materials, sd)
        bufs = [torch.empty((h * w, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]
        used, rays = [], []
        for lo, hi in ((0, late), (late, n)):
            r.totals(reset=True)
            for k in range(lo, hi):
                gs.FrameIndex = k
                r.set_constants(gs)
                r.set_camera(cams[k])
                r.render_device(bufs[k].data_ptr())
            r.synchronize()
            tot = r.totals(reset=True)
            used.append(int(tot.beams_used))
            rays.append((int(tot.rays), int(tot.paths)))
        out.append(([b.cpu().numpy().reshape(h, w, 4) for b in bufs], rays, used, r.queue_sizes()))
    (imgs, rays, used, q), (imgs_b, rays_b, used_b, q_b), (imgs_p, rays_p, used_p, q_p) = out
    # (when a finished build is swapped in depends on when its frames finish: the two contexts need not use lists in the same frames)
    assert used_p == [0, 0] and min(used[0], used_b[0]) > late // 2 and min(used[1], used_b[1]) > 0, (used, used_b, used_p)
    assert rays == rays_b == rays_p and q == q_b == q_p
    total = 0
    for k in range(n):
        assert np.array_equal(bits(imgs[k]), bits(imgs_b[k])) and np.array_equal(bits(imgs[k]), bits(imgs_p[k])), k
        gs.FrameIndex = k
        ref, ost = oracle.render(spheres, materials, sd, cams[k], gs, threads=8)
        assert count_mismatch(imgs[k], ref) == 0, k
        total += ost.rays
    assert total == rays[0][0] + rays[1][0]


@pytest.mark.parametrize("base", [FUSED, SEPARATE], ids=["fused", "separate"])
def test_direct_illumination_frame(dxrs, host, oracle, trio, base):
    """IsDIEnabled: the primary pass makes the direct-illumination estimate at the first shading (the kDI instances)"""
    w, h = 200, 120
    _check(dxrs, oracle, trio(base), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=5), w, h, frame=5, di=True, expect_regions=True)


def test_denoiser_frame(dxrs, host, oracle, trio):
    """A DLSS-RR frame of pt_render_denoiser (the kDn instances share the tile loop): its radiance is pt_render's, its other outputs are the
    same under both maps and without lists"""
    w, h = 200, 120
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera(w, h, jitter_index=6)
    gs = dxrs.types.graphics_settings(w, h, frame_index=6, bounces=BOUNCES, spp=1)
    ref, ost = oracle.render(*scene, cam, gs, threads=8)
    got = []
    for r in trio():
        r.set_scene(*scene)
        r.set_camera(cam)
        r.set_constants(gs)
        r.render_denoiser(DLSS_RR)
        r.render_denoiser(DLSS_RR)
        r.totals(reset=True)
        out, bufs = r.render_denoiser(DLSS_RR, fill=-7.0)
        got.append((out, bufs, r.totals(reset=True), r.queue_sizes()))
    (out, bufs, tot, q), (out_b, bufs_b, tot_b, q_b), (out_p, bufs_p, tot_p, q_p) = got
    assert tot.beams_used == 1 and tot_b.beams_used == 1 and tot_p.beams_used == 0
    assert (tot.rays, tot.paths) == (tot_b.rays, tot_b.paths) == (tot_p.rays, tot_p.paths) and tot.rays == ost.rays
    assert q == q_b == q_p
    assert np.array_equal(bits(out), bits(out_b)) and np.array_equal(bits(out), bits(out_p)) and count_mismatch(out, ref) == 0
    assert sorted(bufs) == sorted(bufs_b) == sorted(bufs_p)
    for name in bufs:
        assert np.array_equal(bits(bufs[name]), bits(bufs_b[name])) and np.array_equal(bits(bufs[name]), bits(bufs_p[name])), name


@pytest.mark.parametrize("base", [FUSED, SEPARATE], ids=["fused", "separate"])
def test_several_samples_keep_the_batch_map(dxrs, host, oracle, trio, base):
    """96x64 at 4 spp: the spp > 1 instances are compiled without the table and the interleave, whatever the switch says"""
    w, h = 96, 64
    _check(dxrs, oracle, trio(base), host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h, jitter_index=7), w, h, spp=4, frame=7)
