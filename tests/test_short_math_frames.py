"""GPU: small frames against the CPU oracle, bit for bit with equal ray counts, for the shading arithmetic that uses pt_math.h's short exact
forms at the sites whose operand range is proven (tests/test_short_math.py checks the forms, tests/test_short_math_ranges.py the ranges).
64x64 and a ragged 67x45: the demo scene at 1 and 3 spp, the small scene (five of its spheres are glass), and the small scene with a sphere of
radius 1e-4 filling the view and with a ground of radius 1e4 -- the extremes for the sites that stay on the compiler's expansions (the hit
frame's normal, the sphere intersection, the half vector)."""
import numpy as np
import pytest

from util import count_mismatch, render_rested

pytestmark = pytest.mark.gpu
SIZES = [(64, 64), (67, 45)]


def check(dxrs, oracle, renderer, scene, cam, w, h, spp, bounces=8):
    spheres, materials, sd = scene
    gs = dxrs.types.graphics_settings(w, h, frame_index=3, bounces=bounces, spp=spp)
    renderer.set_scene(spheres, materials, sd)
    renderer.set_camera(cam)
    renderer.set_constants(gs)
    img, stats = render_rested(renderer)
    ref, ostats = oracle.render(spheres, materials, sd, cam, gs, threads=8)
    assert stats.rays == ostats.rays, (stats.rays, ostats.rays)
    assert count_mismatch(img, ref) == 0
    return stats


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("spp", [1, 3])
def test_demo_scene(dxrs, host, oracle, renderer, w, h, spp):
    check(dxrs, oracle, renderer, host.scene(dxrs.host.SCENE_DEMO, seed=0), host.camera(w, h), w, h, spp)


@pytest.mark.parametrize("w,h", SIZES)
def test_small_scene_with_glass(dxrs, host, oracle, renderer, w, h):
    scene = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    assert (scene[1]["Transmission"] == 1).any()
    stats = check(dxrs, oracle, renderer, scene, host.camera(w, h), w, h, 1)
    assert stats.rays > w * h + w * h // 4  # paths do go on from the spheres


@pytest.mark.parametrize("w,h", SIZES)
def test_sphere_of_radius_1e_4(dxrs, host, oracle, renderer, w, h):
    """a rough metal sphere of radius 1e-4 in free space, the camera 4e-4 from its centre: it covers a good part of the view"""
    spheres, materials, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    spheres, materials = spheres.copy(), materials.copy()
    spheres[13] = (0.0, 2.0, -5.0, 1e-4)
    materials["Metallic"][13], materials["Roughness"][13], materials["Transmission"][13] = 1.0, 0.3, 0.0
    cam = host.camera(w, h)
    for k, v in enumerate((0.0, 2.0, -5.0 - 4e-4)):
        cam.Position[k] = v
        cam.PreviousPosition[k] = v
    cam.NearDepth = 1e-5
    stats = check(dxrs, oracle, renderer, (spheres, materials, sd), cam, w, h, 1)
    assert stats.rays > w * h + w * h // 50  # the sphere is hit by primaries, whose paths go on


@pytest.mark.parametrize("w,h", SIZES)
def test_ground_of_radius_1e4(dxrs, host, oracle, renderer, w, h):
    spheres, materials, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    spheres = spheres.copy()
    assert spheres["r"][15] == 50.0
    spheres[15] = (0.0, -1e4 - 0.1, 0.0, 1e4)
    stats = check(dxrs, oracle, renderer, (spheres, materials, sd), host.camera(w, h), w, h, 1)
    assert stats.rays > w * h + w * h // 4
