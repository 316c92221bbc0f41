"""The side passes (pt_render_gbuffer, pt_restir_di_ex, pt_render_sharc_ex) at the scene sizes around the opt-in for more than the default
64 KB of LDS (csrc/pt_launch.h launch_kernel: taken from 64 KB - kStaticLdsMargin of dynamic LDS).  The frames run these sizes in
tests/test_gpu_fuzz.py (test_scene_sizes_around_the_lds_limits); the same random scenes here.  560, 640, 700 and 780 spheres all lie above
the opt-in's threshold (their trees are 12 to 15 levels deep: 59 to 79 KB with the stacks), so 520 -- 54 880 B, between 48 KB and the
threshold, where the side passes used to opt in and no longer do -- is added.
A closest-hit query does not depend on which copy of the tree is walked: the LDS-resident context and one that keeps the tree in global
memory (PT_FLAG_NO_LDS_SCENE) give the same bits."""
import numpy as np
import pytest

from test_gpu_fuzz import random_scene
from test_sharc import same_bits, setup
from test_sharc import shims  # noqa: F401  (a fixture)
from test_sharc_ex import HostCacheEx, ex_frames_against_host
from test_sharc_ex import ex_lib  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

COUNTS = (520, 560, 640, 700, 780)
W, H = 64, 48
STATIC_LDS_MARGIN = (2048 + 64 + 16) * 4  # kStaticLdsMargin (csrc/pt_launch.h)


@pytest.fixture(scope="module")
def renderer_global(dxrs):
    r = dxrs.Renderer(device=0, flags=dxrs.types.PT_FLAG_NO_LDS_SCENE)
    yield r
    r.close()


def scene_of(dxrs, host, n):
    spheres, mats = random_scene(dxrs, np.random.default_rng(9000 + n), n)
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    return spheres, mats, sd, host.camera_matrices(W, H, position=(0.3, 0.2, -12.0), jitter_index=n)


def lds_bytes(n, depth):
    """-> (scene_lds_bytes(n - 1, n) of csrc/pt_trace.h, that plus the stacks of 512 lanes: depth entries of 2 B each)"""
    scene = ((n - 1) * 4 + n) * 16 + ((n * 4 + 15) & ~15)
    return scene, scene + 512 * max(1, depth) * 2


def test_sizes_lie_on_both_sides_of_the_opt_in(dxrs, host, renderer, renderer_global):
    lds = {}
    for n in COUNTS:
        spheres, mats, sd, _ = scene_of(dxrs, host, n)
        info = renderer.set_scene(spheres, mats, sd)
        scene, total = lds_bytes(n, info.depth)
        print(f"{n} spheres: depth {info.depth}, scene {scene} B, traverse LDS {total} B, lds_resident {info.lds_resident}")
        # pt_build_accel's rule: the scene copy within 64 KB, and with the stacks within half a CU's 160 KB
        assert bool(info.lds_resident) == (scene <= 64 * 1024 and total <= 80 * 1024), n
        assert renderer_global.set_scene(spheres, mats, sd).lds_resident == 0
        if info.lds_resident:
            lds[n] = total
    assert set(lds) == set(COUNTS), "every one of these scenes is LDS-resident"
    assert any(48 * 1024 < b <= 64 * 1024 - STATIC_LDS_MARGIN for b in lds.values()), "no scene between 48 KB and the opt-in's threshold"
    assert any(b > 64 * 1024 - STATIC_LDS_MARGIN for b in lds.values()), "no scene above the opt-in's threshold"


@pytest.mark.parametrize("n", COUNTS)
def test_gbuffer_does_not_depend_on_where_the_tree_lives(dxrs, host, renderer, renderer_global, n):
    spheres, mats, sd, cam = scene_of(dxrs, host, n)
    gs = dxrs.types.graphics_settings(W, H, frame_index=n, bounces=4, spp=1)
    runs = []
    for r in (renderer, renderer_global):
        setup(r, dxrs, spheres, mats, sd, cam, gs)
        runs.append(r.render_gbuffer("all"))
    assert renderer.accel.lds_resident and not renderer_global.accel.lds_resident
    assert len(runs[0]) == 13
    for name in runs[0]:
        assert same_bits(runs[0][name], runs[1][name]), name
    depth = runs[0]["LinearDepth"]
    assert np.isfinite(depth).sum() > W * H // 10, "the view must show the scene"


@pytest.mark.parametrize("n", COUNTS)
def test_restir_di_ex_does_not_depend_on_where_the_tree_lives(dxrs, host, renderer, renderer_global, n):
    spheres, mats, sd, cam = scene_of(dxrs, host, n)
    assert ((mats["EmissiveStrength"][:, None] * mats["EmissiveColor"]) > 0).any(), "the scene needs emitters"
    runs = []
    for r in (renderer, renderer_global):
        frames = []
        for f in range(2):
            gs = dxrs.types.graphics_settings(W, H, frame_index=f, bounces=4, spp=1)
            if f == 0:
                setup(r, dxrs, spheres, mats, sd, cam, gs)
            r.set_constants(gs)
            dd, ds, _ = r.restir_di(reset_history=f == 0, candidates=dict(brdf_samples=1, boiling_filter=0.2))
            frames.append((dd.cpu().numpy(), ds.cpu().numpy()))
        runs.append(frames)
    assert renderer.accel.lds_resident and not renderer_global.accel.lds_resident
    for f in range(2):
        for k, name in enumerate(("Diffuse", "Specular")):
            assert same_bits(runs[0][f][k], runs[1][f][k]), f"frame {f}: {name}"
        assert np.nan_to_num(runs[0][f][0][..., :3]).max() > 0, f"frame {f}: no pixel is lit"


@pytest.mark.parametrize("n", COUNTS)
def test_sharc_ex_equals_the_host_header(dxrs, host, renderer, shims, ex_lib, n):  # noqa: F811
    """update, resolve and query of two frames (the second at 2 spp) with a DI and the DLSS-RR output, at flags 0"""
    spheres, mats, sd, cam = scene_of(dxrs, host, n)
    ex_frames_against_host(dxrs, renderer, HostCacheEx(ex_lib, *shims, spheres, mats, sd), spheres, mats, sd, [cam, cam], modes=(1,), size=(W, H))
    assert renderer.accel.lds_resident
