"""The GPU against the independent float64 tracer (tests/independent_tracer.py), with no oracle in between: every case of
tests/test_independent_tracer.py -- untextured, textured, environment-mapped, alpha-tested, direct illumination -- is rendered
through the C-ABI over a rect that covers its fixture pixels, and each fixture pixel's radiance is compared with the committed
trace's radiance column under the bound the CPU comparison uses for the oracle (worst relative error < 1e-2).  The textured and
DI cases are rendered once more by a context without reflection-beam lists (PT_REFL_BEAMS=0)."""
import os

import numpy as np
import pytest

import test_independent_tracer as ti

pytestmark = pytest.mark.gpu


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


def _case(dxrs, host, name):
    """(spheres, materials, sd, cam, gs, textures, fixture rows) of a case"""
    if name in ti.TEXTURED_CASES:
        c = ti.textured_case(dxrs, host, name)
        return c["spheres"], c["materials"], c["sd"], c["cam"], c["gs"], c["textures"], ti._load(name)["events"]
    kind, w, h, bounces, spp, rr, frame, _ = ti.CASES[name]
    spheres, materials, sd = ti._scene(dxrs, host, kind)
    gs = dxrs.types.graphics_settings(w, h, frame_index=frame, bounces=bounces, spp=spp, rr=rr)
    rows = np.load(os.path.join(ti.GOLD, f"independent_trace_{name}.npz"))["events"]
    return spheres, materials, sd, host.camera(w, h, jitter_index=frame), gs, None, rows


def _radiance_errors(r, case):
    spheres, materials, sd, cam, gs, textures, rows = case
    r.set_scene(spheres, materials, sd)
    r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(gs)
    x0, y0 = int(rows[:, 0].min()), int(rows[:, 1].min())
    rect = (x0, y0, int(rows[:, 0].max()) - x0 + 1, int(rows[:, 1].max()) - y0 + 1)
    img, _ = r.render(rect)
    r.set_textures(None)
    last = np.r_[rows[1:, 0] != rows[:-1, 0], True] | np.r_[rows[1:, 1] != rows[:-1, 1], True]  # each pixel's last event row
    errs = []
    for row in rows[last]:
        px, py, want = int(row[0]), int(row[1]), row[15:18]
        got = img[py - y0, px - x0, :3].astype(np.float64)
        errs.append(float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-3)))
    return np.array(errs)


@pytest.mark.parametrize("name", ti.ALL_CASES)
def test_gpu_radiance_matches_the_independent_tracer(dxrs, host, renderer, name):
    errs = _radiance_errors(renderer, _case(dxrs, host, name))
    print(f"{name}: {len(errs)} pixels, median {np.median(errs):.2e}, worst {errs.max():.2e}")
    assert errs.max() < 1e-2, (name, float(errs.max()))


@pytest.mark.parametrize("name", sorted(ti.TEXTURED_CASES))
def test_gpu_without_reflection_beams_matches_the_independent_tracer(dxrs, host, renderer_no_refl, name):
    errs = _radiance_errors(renderer_no_refl, _case(dxrs, host, name))
    print(f"{name} (PT_REFL_BEAMS=0): {len(errs)} pixels, median {np.median(errs):.2e}, worst {errs.max():.2e}")
    assert errs.max() < 1e-2, (name, float(errs.max()))
