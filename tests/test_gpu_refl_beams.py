"""Reflection beams (DESIGN.md "Reflection beams"): the in-register first bounce of a 1-spp primary pass takes its candidates from
the block's region list when every active lane's spawned ray lies in the region.  Frames with the lists (the default) and without
them (a context created with PT_REFL_BEAMS=0) must agree bit for bit with each other and with the CPU oracle, with equal ray counts."""
import os

import numpy as np
import pytest

from util import count_mismatch, render_rested

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer_refl(renderer):
    return renderer


@pytest.fixture(scope="module")
def renderer_no_refl(dxrs):
    """A context created with PT_REFL_BEAMS=0 (the knobs are read once, at pt_create)."""
    old = os.environ.get("PT_REFL_BEAMS")
    os.environ["PT_REFL_BEAMS"] = "0"
    try:
        r = dxrs.Renderer(device=0)
    finally:
        if old is None:
            os.environ.pop("PT_REFL_BEAMS", None)
        else:
            os.environ["PT_REFL_BEAMS"] = old
    yield r
    r.close()


def _setup(r, scene, cam, gs, textures=None):
    spheres, materials, sd = scene
    r.set_scene(spheres, materials, sd)
    if textures is not None:
        r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(gs)


def _on_off(renderer_refl, renderer_no_refl, scene, cam, gs, rect=None, textures=None):
    """The rested frame with the lists and without; returns (image, stats, bounce-1 waves, waves served by a list)."""
    _setup(renderer_refl, scene, cam, gs, textures)
    renderer_refl.refl_stats(reset=True)
    renderer_refl.render(rect)
    renderer_refl.render(rect)
    renderer_refl.refl_stats(reset=True)
    img, st = renderer_refl.render(rect)  # (the view has rested: primary-beam lists and region records are in place)
    waves, listed = renderer_refl.refl_stats(reset=True)
    _setup(renderer_no_refl, scene, cam, gs, textures)
    img0, st0 = render_rested(renderer_no_refl, rect)
    assert renderer_no_refl.refl_stats(reset=True)[1] == 0
    assert st.rays == st0.rays
    assert count_mismatch(img, img0) == 0
    return img, st, waves, listed


def test_c2_serves_bounce1_waves_from_lists(dxrs, host, oracle, renderer_refl, renderer_no_refl):
    """C2 (demo scene, 1080p, 1 spp, 8 bounces): the whole frame on and off, a ground crop against the oracle, and the share of
    bounce-1 waves served by lists."""
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera(1920, 1080)
    gs = dxrs.types.graphics_settings(1920, 1080, bounces=8, spp=1)
    img, st, waves, listed = _on_off(renderer_refl, renderer_no_refl, scene, cam, gs)
    share = listed / max(waves, 1)
    print(f"C2: {listed} of {waves} bounce-1 waves served by region lists ({100 * share:.1f} %)")
    assert waves > 0 and share >= 0.1
    rect = (832, 860, 256, 128)  # ground: mirror bounces
    _setup(renderer_refl, scene, cam, gs)
    crop, cst = render_rested(renderer_refl, rect)
    ref, ost = oracle.render(*scene, cam, gs, rect=rect, threads=8)
    assert cst.rays == ost.rays
    assert count_mismatch(crop, ref) == 0
    assert count_mismatch(crop, img[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]) == 0


def test_c1(dxrs, host, oracle, renderer_refl, renderer_no_refl):
    scene = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    cam = host.camera(256, 256)
    gs = dxrs.types.graphics_settings(256, 256, bounces=4, spp=1)
    img, st, _, _ = _on_off(renderer_refl, renderer_no_refl, scene, cam, gs)
    ref, ost = oracle.render(*scene, cam, gs, threads=8)
    assert st.rays == ost.rays
    assert count_mismatch(img, ref) == 0


def mirror_scene(dxrs, rng, roughness, n=40, alpha=False):
    """A mirror ground (a huge sphere, metallic 1) under random small spheres of random materials."""
    s = np.zeros(n, dtype=dxrs.SPHERE_DTYPE)
    s["cx"], s["cy"], s["cz"] = rng.uniform(-4, 4, n), rng.uniform(-0.5, 2.5, n), rng.uniform(-4, 6, n)
    s["r"] = rng.uniform(0.1, 0.8, n)
    s[0] = (0.0, -500.5, 0.0, 500.0)
    m = dxrs.types.default_material(n)
    m["BaseColor"][:, :3] = rng.random((n, 3))
    m["Metallic"] = rng.choice([0.0, 1.0, 0.3], n)
    m["Roughness"] = rng.choice([0.0, 1e-3, 0.05, 0.5], n)
    m["Transmission"] = rng.choice([0.0, 1.0], n)
    emit = rng.random(n) < 0.2
    m["EmissiveStrength"][emit] = rng.uniform(1.0, 20.0, emit.sum())
    m["EmissiveColor"][emit] = rng.random((emit.sum(), 3))
    if alpha:
        a = rng.random(n) < 0.3
        a[0] = False
        m["AlphaMode"][a] = rng.choice([1, 2], a.sum())
        m["BaseColor"][a, 3] = rng.choice([0.0, 0.3, 0.9], a.sum())
        m["AlphaCutoff"][a] = 0.5
    m["BaseColor"][0, :3] = (0.9, 0.8, 0.7)
    m["Metallic"][0], m["Roughness"][0], m["Transmission"][0], m["EmissiveStrength"][0], m["AlphaMode"][0] = 1.0, roughness, 0.0, 0.0, 0
    return s, m


@pytest.mark.parametrize("roughness", [0.0, 1e-3, 0.05])
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("di", [False, True])
def test_mirror_scenes(dxrs, host, oracle, renderer_refl, renderer_no_refl, roughness, seed, di):
    rng = np.random.default_rng(7100 + seed)
    spheres, materials = mirror_scene(dxrs, rng, roughness, alpha=seed == 2)
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    w, h = 160, 96
    cam = host.camera(w, h, position=(0.3, 1.5, -9.0), look_at=(0.0, -0.5, 0.0), jitter_index=seed)
    gs = dxrs.types.graphics_settings(w, h, frame_index=seed * 13, bounces=4, spp=1, di=di)
    img, st, waves, listed = _on_off(renderer_refl, renderer_no_refl, (spheres, materials, sd), cam, gs)
    ref, ost = oracle.render(spheres, materials, sd, cam, gs, threads=8)
    assert st.rays == ost.rays
    assert count_mismatch(img, ref) == 0
    if roughness <= 1e-3:
        assert listed > 0  # the ground's blocks have regions


def test_textured_scene(dxrs, host, oracle, renderer_refl, renderer_no_refl):
    from test_textures import make_textured_scene
    rng = np.random.default_rng(7300)
    spheres, materials, ts = make_textured_scene(dxrs, rng, 20, 1)
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    cam = host.camera(97, 61, position=(0.0, 0.5, -12.0))
    gs = dxrs.types.graphics_settings(97, 61, bounces=4, spp=1)
    img, st, _, _ = _on_off(renderer_refl, renderer_no_refl, (spheres, materials, sd), cam, gs, textures=ts)
    ref, ost = oracle.render(spheres, materials, sd, cam, gs, threads=8, textures=ts)
    assert st.rays == ost.rays
    assert count_mismatch(img, ref) == 0
    renderer_refl.set_textures(None)
    renderer_no_refl.set_textures(None)


def test_frames_in_flight_and_moving_camera(dxrs, host, renderer_no_refl):
    """Three frames in flight over a resting then moving camera: every frame equals the PT_REFL_BEAMS=0 context's, and frames of the
    moving camera use no region (their lists come from the share builds)."""
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 640, 360
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        _setup(r, scene, host.camera(w, h), dxrs.types.graphics_settings(w, h, bounces=8, spp=1))
        _setup(renderer_no_refl, scene, host.camera(w, h), dxrs.types.graphics_settings(w, h, bounces=8, spp=1))
        outs = []
        for k in range(6):
            img, _ = r.render()
            outs.append(np.array(img, copy=True))
        waves, listed = r.refl_stats(reset=True)
        assert listed > 0
        ref, _ = renderer_no_refl.render()
        for o in outs:
            assert count_mismatch(o, ref) == 0
        for k in range(8):
            cam = host.camera(w, h, position=(0.05 * (k + 1), 0.0, -15.0 + 0.1 * (k + 1)))
            r.set_camera(cam)
            renderer_no_refl.set_camera(cam)
            img, st = r.render()
            img0, st0 = renderer_no_refl.render()
            assert st.rays == st0.rays and count_mismatch(img, img0) == 0
        assert r.refl_stats(reset=True)[1] == 0
    finally:
        r.close()
