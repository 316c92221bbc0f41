"""GPU: primary-beam lists at the edges of their bounds (csrc/pt_beam.h, csrc/pt_beam_cache.h; tests/test_primary_beams.py holds the CPU
properties).  Short trajectories of whole small frames -- the image corners are where the bounds are tightest -- over scenes with many small
spheres near block outlines, every frame bit-identical to the oracle whichever way its primaries were found, and some frames of every case
served by lists (else the case checked nothing)."""
import math
import os

import pytest

pytestmark = pytest.mark.gpu


def run(dxrs, host, oracle, r, scene, w, h, cams, min_used=1):
    """Renders cams[k] as frame k of one view; every frame against the oracle; -> which frames used lists"""
    from util import count_mismatch
    spheres, materials, sd = scene
    gs = dxrs.types.graphics_settings(w, h, frame_index=0, bounces=3, spp=1)
    r.set_scene(spheres, materials, sd)
    used = []
    for k, cam in enumerate(cams):
        gs.FrameIndex = k
        r.set_constants(gs); r.set_camera(cam)
        img, st = r.render()
        ref, ost = oracle.render(spheres, materials, sd, cam, gs, threads=8)
        assert st.rays == ost.rays and count_mismatch(img, ref) == 0, k
        used.append(bool(st.beams_used))
    assert sum(used) >= min_used, used
    return used


def yaw_look_at(position, distance, angle):
    return (position[0] + distance * math.sin(angle), position[1], position[2] + distance * math.cos(angle))


def test_narrow_lens_yawing_near_the_margin_cap(dxrs, host, oracle, renderer):
    """A 10 degree lens: one pixel is 1e-3 rad / 1.8 here, so a yaw of 2e-4 rad per frame asks for a margin of several pixels -- near the cap of 8."""
    w, h, pos = 320, 200, (0.0, 2.0, -60.0)
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cams = [host.camera(w, h, position=pos, look_at=yaw_look_at(pos, 60.0, 2e-4 * k), hfov=math.radians(10.0), jitter_index=k % 8) for k in range(14)]
    run(dxrs, host, oracle, renderer, scene, w, h, cams)


def test_wide_lens_turning_slowly(dxrs, host, oracle, renderer):
    """A lens of 150 degrees: the image corner lies 1.35 rad off the view axis, where 1 / cos^2 multiplies every turn by 20."""
    w, h, pos = 320, 200, (0.0, 1.0, -14.0)
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cams = [host.camera(w, h, position=pos, look_at=yaw_look_at(pos, 14.0, 1e-4 * k), hfov=math.radians(150.0), jitter_index=k % 8) for k in range(14)]
    run(dxrs, host, oracle, renderer, scene, w, h, cams)


def test_travelling_camera_with_slack_near_the_smallest_radius(dxrs, host, oracle, renderer):
    """A step per frame of a twentieth of the smallest radius: half a span's travel is about that radius, the cap of the slack."""
    w, h = 320, 200
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    step = 0.05 * float(scene[0]["r"].min())
    cams = [host.camera(w, h, position=(0.7 * step * k, 1.0, -14.0 + 0.7 * step * k), jitter_index=k % 8) for k in range(16)]
    run(dxrs, host, oracle, renderer, scene, w, h, cams)


@pytest.mark.parametrize("hfov_deg", [22.0, 60.0])
def test_off_axis_camera_whose_lens_shift_changes(dxrs, host, oracle, renderer, hfov_deg):
    """An off-axis (lens-shift) camera: Forward + s * Right with s changing a little every frame.  Its bases are no rotations of one another
    (beam_within reads half the shift as a turn): lists serve such frames only while the shift is paid for, and the frames of the view at rest
    after the shift has stopped."""
    w, h, pos = 320, 200, (0.0, 1.5, -40.0 if hfov_deg < 30 else -14.0)
    scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cams = []
    for k in range(16):
        cam = host.camera(w, h, position=pos, look_at=(0.0, 0.5, 0.0), hfov=math.radians(hfov_deg), jitter_index=k % 8)
        s = 2.5e-4 * min(k, 10)  # ten frames of a growing shift (0.04 pixels a frame at 22 degrees), then the view rests
        for i in range(3):
            cam.ForwardDirection[i] += s * cam.RightDirection[i]
        cams.append(cam)
    used = run(dxrs, host, oracle, renderer, scene, w, h, cams)
    assert used[-1], used  # the resting view's exact lists


def test_margin_cap_raised_by_its_knob(dxrs, host, oracle):
    """PT_BEAM_MAX_MARGIN=64 (the knob has no upper limit; 64 pixels are eight blocks) in a context of its own -- the knobs are read at
    pt_create: a yaw four times as fast as the default cap serves."""
    old = os.environ.get("PT_BEAM_MAX_MARGIN")
    os.environ["PT_BEAM_MAX_MARGIN"] = "64"
    try:
        r = dxrs.Renderer(device=0)
    finally:
        if old is None:
            os.environ.pop("PT_BEAM_MAX_MARGIN", None)
        else:
            os.environ["PT_BEAM_MAX_MARGIN"] = old
    try:
        w, h, pos = 320, 200, (0.0, 1.0, -14.0)
        scene = host.scene(dxrs.host.SCENE_DEMO, seed=0)
        cams = [host.camera(w, h, position=pos, look_at=yaw_look_at(pos, 14.0, 6e-3 * k), jitter_index=k % 8) for k in range(14)]
        run(dxrs, host, oracle, r, scene, w, h, cams)
    finally:
        r.close()
