"""GPU: the leaf, beam and region headers as hipcc compiles them for gfx950 (tests/hostshim/leaf_batch_gpu.hip: the wrapper text of
leaf_batch.h, the product's compiler flags, one thread per element) against the same wrappers compiled as host C++.
- Bit parity: every function of pt_math.h, pt_bsdf.h, pt_texture.h, pt_post.h, pt_light.h and region_contains, device == host word for
  word on 2^20 random operands plus the edge tables of tests/test_leaf_edges.py.  Two NaNs compare equal; nothing else is allowed.
- pt_region.h (atan2f, asinf, acosf, cosf from the device library) and pt_beam.h (the reciprocal-square-root instruction) are NOT the
  same arithmetic on the two sides: the properties test_refl_region.py and test_primary_beams.py prove for the host build are run on the
  device's own results, with the same float64 brute force, the same floors and zero violations allowed.
- An agreement report (printed, not asserted; DESIGN.md "Primary beams" / "Reflection beams" record a run of it)."""
import ctypes as C

import numpy as np
import pytest

import test_leaf_edges as le
import test_primary_beams as tpb
import test_refl_region as trr

pytestmark = pytest.mark.gpu
N_RANDOM = 1 << 20


@pytest.fixture(scope="module")
def hostb():
    import __graft_entry__ as g

    return le.Batch(g.build_leaf_batch_host(), "lbh_")


@pytest.fixture(scope="module")
def devb():
    import __graft_entry__ as g

    return le.Batch(g.build_leaf_batch_gpu(), "lbg_")


@pytest.fixture(scope="module")
def beam_host():
    import __graft_entry__ as g

    return C.CDLL(g.build_beam_shim())


# ------------------------------------------------------------------------------------------------ bit parity
@pytest.mark.parametrize("name", le.PARITY_FUNCTIONS)
def test_device_matches_host_bit_for_bit(name, hostb, devb):
    rows, aux = le.build_rows(name, N_RANDOM, hostb)
    assert len(rows) >= N_RANDOM, len(rows)
    want, got = hostb.run(name, rows, aux), devb.run(name, rows, aux)
    bad = le.same_words(got, want, le.float_cols(name))
    if len(bad):
        for k in bad[:8]:
            print(f"{name}: in {rows[k]!r} ({rows[k].view(np.uint32)!r})\n  host   {want[k].view(np.float32)!r} ({want[k]!r})\n  device {got[k].view(np.float32)!r} ({got[k]!r})")
    assert not len(bad), f"{name}: {len(bad)} of {len(rows)} rows differ between the host and the gfx950 build"


# ------------------------------------------------------------------------------------------------ pt_region.h on the device's own results
def test_device_regions_rejected_boxes_are_never_passed(devb):
    """regions from the device's region_set_cone, boxes rejected by the device's region_meets_box; more than 1000 rejected (the body's floor)"""
    trr.test_rejected_boxes_are_never_passed(le.RegionShim(devb))


def test_device_regions_accepted_rays_lie_in_the_region(devb):
    """rays the device's region_contains accepts lie in O and within the device's own g.theta of the axis"""
    trr.test_accepted_rays_lie_in_the_region(le.RegionShim(devb))


def test_device_records_accept_mirror_bounces(devb):
    """records from the device's region_from_hits accept the mirror bounces the device's own rg_lane forms"""
    trr.test_records_accept_mirror_bounces(le.RegionShim(devb))


# ------------------------------------------------------------------------------------------------ pt_beam.h on the device's own results
LENSES_DEG = [10.0, 22.0, 60.0, 150.0]  # the lenses of tests/test_gpu_primary_beams.py
SLACKS = [0.0, 0.05, 0.5]               # none; about the smallest radius of the test scenes; a large one
MARGINS = [0.0, 8.0]                    # none; the margin cap (PT_BEAM_MAX_MARGIN's default)


def lens_camera(rng, hfov_deg, k):
    """(cam[12], w, h): a random pose with the given horizontal field of view; sizes mostly not multiples of 8"""
    w, h = int(rng.integers(40, 400)), int(rng.integers(40, 300))
    Rm = tpb.rotation(rng.normal(size=3), rng.uniform(0, np.pi))
    lr = np.tan(0.5 * np.radians(hfov_deg))
    pos = rng.uniform(-20, 20, 3) * (1e3 if k % 5 == 4 else 1.0)
    return tpb.c32(np.concatenate([pos, Rm[0] * lr, Rm[1] * lr * h / w, Rm[2]])), w, h


def p1_sweep(shim, seed, n_iter):
    """P1 of test_primary_beams.py (check_beam: float64 brute force) over LENSES_DEG x SLACKS x MARGINS -> (rejected boxes per lens, rejected leaves)"""
    rng = np.random.default_rng(seed)
    n_box, n_leaf = {d: 0 for d in LENSES_DEG}, 0
    for it in range(n_iter):
        deg = LENSES_DEG[it % 4]
        slack, margin = SLACKS[(it // 4) % 3], MARGINS[(it // 12) % 2]
        cam, w, h = lens_camera(rng, deg, it)
        px, py = tpb.pick_block(rng, w, h, tpb.WHERE[(it // 3) % len(tpb.WHERE)])
        g = tpb.make_beam(shim, cam, w, h, px, py, slack, margin)
        pix, jit = tpb.block_samples(rng, w, h, px, py, 96)
        o, d = tpb.rays(shim, cam, w, h, pix, jit, tpb.positions_within(rng, cam[:3], slack, len(pix)))
        nb, nl = tpb.check_beam(shim, rng, g, o, d, slack)
        n_box[deg] += nb
        n_leaf += nl
    return n_box, n_leaf


P1_SEED, P1_ITER = 61, 144  # (the host build clears the floors below with this seed: 2829 / 2817 / 2792 / 3723 boxes per lens, 13394 leaves)


def test_device_beams_rejected_boxes_and_leaves_are_never_hit(devb, beam_host):
    n_box, n_leaf = p1_sweep(le.BeamShim(devb, beam_host), P1_SEED, P1_ITER)
    print("device P1 rejected:", n_box, n_leaf)
    assert sum(n_box.values()) >= 5000 and n_leaf >= 1000 and min(n_box.values()) >= 100, (n_box, n_leaf)  # test_primary_beams.py's floors


def test_device_beams_p1_of_the_cpu_suite(devb, beam_host):
    """test_primary_beams.py's own P1 body (its cameras, slacks, margins and floors) on the device's make_beam and box tests"""
    tpb.test_p1_rejected_boxes_and_leaves_are_never_hit(le.BeamShim(devb, beam_host))


# ------------------------------------------------------------------------------------------------ agreement report
def test_agreement_report(hostb, devb, beam_host):
    """How much of the margins the device uses: decisions that differ between the two builds, and how far device-made records are from
    host-made ones.  Printed; the only assertions are that the report saw enough decisions of either kind to mean something."""
    rng = np.random.default_rng(71)
    hs, ds = le.BeamShim(hostb, beam_host), le.BeamShim(devb, beam_host)
    n = {"box": 0, "leaf": 0}
    diff = {"box": 0, "leaf": 0}
    rejected = {"box": 0, "leaf": 0}
    plane = 0.0
    for it in range(120):
        cam, w, h = lens_camera(rng, LENSES_DEG[it % 4], it)
        px, py = tpb.pick_block(rng, w, h, tpb.WHERE[it % len(tpb.WHERE)])
        slack, margin = SLACKS[it % 3], MARGINS[it % 2]
        gh, gd = tpb.make_beam(hs, cam, w, h, px, py, slack, margin), tpb.make_beam(ds, cam, w, h, px, py, slack, margin)
        plane = max(plane, float(np.abs(gh.astype(np.float64) - gd)[3:15].max()))
        pix, jit = tpb.block_samples(rng, w, h, px, py, 32)
        o, d = tpb.rays(hs, cam, w, h, pix, jit)
        boxes = tpb.scatter_boxes(rng, o.astype(np.float64), d.astype(np.float64), slack, 2000)
        for kind, bx in (("box", boxes), ("leaf", tpb.leaf_boxes(rng, boxes))):
            a, b = tpb.meets(hs, gh, bx, leaf=kind == "leaf"), tpb.meets(ds, gd, bx, leaf=kind == "leaf")
            n[kind] += len(bx); diff[kind] += int((a != b).sum()); rejected[kind] += int((~b).sum())
    print(f"beams: largest |host - device| of a plane normal's component {plane:.3e}; beam_meets_box: {diff['box']} of {n['box']} decisions differ "
          f"({rejected['box']} rejected on the device); beam_meets_leaf: {diff['leaf']} of {n['leaf']} differ ({rejected['leaf']} rejected)")
    hr, dr = le.RegionShim(hostb), le.RegionShim(devb)
    n_reg = n_dec = n_diff = n_rej = 0
    d_theta = d_cos = 0.0
    for it in range(200):
        lo, hi, axis, theta = trr.random_region(rng)
        gh, gd = trr.make_region(hr, lo, hi, axis, theta), trr.make_region(dr, lo, hi, axis, theta)
        d_theta, d_cos = max(d_theta, abs(float(gh[9]) - float(gd[9]))), max(d_cos, abs(float(gh[10]) - float(gd[10])))
        n_reg += 1
        c = 0.5 * (lo + hi)
        centres = c + np.exp(rng.uniform(np.log(0.5), np.log(80.0), 2000))[:, None] * trr.cone_dirs(rng, axis, min(3.0 * theta + 0.05, 3.0), 2000)
        ext = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), (2000, 3)))
        boxes = np.concatenate([centres - ext, centres + ext], axis=1).astype(np.float32)
        a, b = trr.meets(hr, gh, boxes), trr.meets(dr, gd, boxes)
        n_dec += len(boxes); n_diff += int((a != b).sum()); n_rej += int((~b).sum())
    n_built = 0
    r_theta = r_cos = r_box = 0.0
    for _ in range(400):
        cam, dirs, Cs, r = trr.pyramid(rng)
        gh, gd = np.zeros(11, np.float32), np.zeros(11, np.float32)
        kh, kd = hr.rg_from_rays(trr.fp(cam), trr.fp(dirs), trr.fp(Cs), C.c_float(r), trr.fp(gh)), dr.rg_from_rays(trr.fp(cam), trr.fp(dirs), trr.fp(Cs), C.c_float(r), trr.fp(gd))
        if kh and kd:
            n_built += 1
            r_theta, r_cos = max(r_theta, abs(float(gh[9]) - float(gd[9]))), max(r_cos, abs(float(gh[10]) - float(gd[10])))
            r_box = max(r_box, float(np.abs(gh[:6].astype(np.float64) - gd[:6]).max()))
    print(f"regions: region_set_cone over {n_reg} regions: largest |dtheta| {d_theta:.3e} rad, |dcos_run| {d_cos:.3e}; region_meets_box: {n_diff} of {n_dec} "
          f"decisions differ ({n_rej} rejected on the device); region_from_hits over {n_built} records: |dtheta| {r_theta:.3e}, |dcos_run| {r_cos:.3e}, "
          f"largest difference of a coordinate of O {r_box:.3e}")
    assert rejected["box"] > 1000 and rejected["leaf"] > 1000 and n_rej > 1000 and n_built > 100
