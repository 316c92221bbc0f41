"""The refit reference (tests/refit_reference.py) against both host builders, and the conditions on the inputs of tests/test_gpu_refit.py:
all on the CPU.  The reference reproduces the builders' boxes bit for bit over the builders' own links, its boxes contain their spheres in
float64 for every layout and after every move, and every ray set the GPU tests trace hits enough spheres -- also with rays that have a
zero direction component -- for `BVH == brute force` to mean something."""
import numpy as np
import pytest

import refit_reference as rr
from test_abi import check_lbvh
from test_gpu_accel import make_rays

ALL_SIZES = rr.SIZES + (rr.NO_LDS_SIZE,)
MISS = 0xFFFFFFFF


def layouts(dxrs, n):
    """[(name, spheres)]: the built scene, every move of it, and for the sizes of the large-coordinate move the scene times 2^31"""
    base = rr.patch_scene(dxrs.SPHERE_DTYPE, n)
    out = [("base", base)] + rr.motions(base)
    if n in rr.LARGE_SIZES:
        out.append(("large", rr.scaled(base)))
    return out


@pytest.mark.parametrize("n", ALL_SIZES)
def test_refit_reproduces_the_host_builders(dxrs, n):
    lib = dxrs.load_hip()
    for name, sph in layouts(dxrs, n):
        for sah in (False, True):
            nodes, order, depth = lib.lbvh_build_host(sph, sah=sah)
            check_lbvh(sph, nodes, order, depth)
            ref = rr.refit(nodes, order, sph)
            assert rr.same_links(ref, nodes) and rr.box_mismatches(ref, nodes) == 0 and ref.tobytes() == nodes.tobytes(), (name, sah)
            assert rr.contains64(nodes, order, sph), (name, sah)
            assert rr.depth(nodes) == depth, (name, sah)


@pytest.mark.parametrize("n", ALL_SIZES)
def test_refit_over_the_old_links_contains_the_moved_spheres(dxrs, n):
    """what pt_refit_accel does: the links of the tree built for the base scene, the boxes of the moved spheres"""
    lib = dxrs.load_hip()
    states = layouts(dxrs, n)
    base = states[0][1]
    for sah in (False, True):
        nodes, order, depth = lib.lbvh_build_host(base, sah=sah)
        for name, sph in states[1:]:
            ref = rr.refit(nodes, order, sph)
            assert rr.same_links(ref, nodes) and rr.depth(ref) == depth, (name, sah)
            assert rr.contains64(ref, order, sph), (name, sah)
            assert rr.box_mismatches(ref, nodes) > 0, (name, sah)  # the move is visible in the boxes


def test_the_checks_can_fail(dxrs):
    """a box that is too small fails contains64; a stale, larger pad still contains the spheres and fails only the bit compare"""
    lib = dxrs.load_hip()
    base = rr.patch_scene(dxrs.SPHERE_DTYPE, 65)
    moves = dict(rr.motions(base))
    nodes, order, _ = lib.lbvh_build_host(base)
    good = rr.refit(nodes, order, moves["jitter"])
    i = int(np.nonzero(good["child1"] < 0)[0][0])  # a node whose second child is a leaf
    s = moves["jitter"][order[~good["child1"][i]]]
    bad = good.copy()
    bad["hi1"][i, 1] = s["cy"] + s["r"] * np.float32(0.999)
    assert rr.contains64(good, order, moves["jitter"]) and not rr.contains64(bad, order, moves["jitter"])
    assert rr.box_mismatches(bad, good) == 1
    # the boxes of the translated scene moved back by the translation: the pad of bounds two orders of magnitude larger
    stale = rr.refit(nodes, order, moves["translated"])
    for f in rr.BOX_FIELDS:
        stale[f] -= np.array([3000.0, -7000.0, 500.0], dtype=np.float32)
    assert rr.padding(moves["translated"]) > 50 * rr.padding(moves["jitter"])
    assert rr.box_mismatches(stale, good) == len(good)
    wide = good.copy()
    extra = rr.padding(moves["translated"])
    for f in ("lo0", "lo1"):
        wide[f] -= extra
    for f in ("hi0", "hi1"):
        wide[f] += extra
    assert rr.contains64(wide, order, moves["jitter"]) and rr.box_mismatches(wide, good) == len(good)
    # a skipped node: one record keeps the boxes of the previous positions
    skipped = good.copy()
    old = rr.refit(nodes, order, base)
    for f in rr.BOX_FIELDS:
        skipped[f][i] = old[f][i]
    assert rr.box_mismatches(skipped, good) == 1


def check_floors(ids, d, what):
    hit = ids != MISS
    zero = rr.has_zero_component(d)
    assert hit.mean() >= rr.HIT_SHARE, (what, hit.mean())
    assert int((hit & zero).sum()) >= rr.ZERO_HITS, (what, int((hit & zero).sum()), int(zero.sum()))


@pytest.mark.parametrize("n", ALL_SIZES)
def test_ray_sets_hit_enough(dxrs, oracle, n):
    """the oracle's brute force over every ray set tests/test_gpu_refit.py traces: at least 30 % of the rays hit, and at least 200 of those with
    a direction component that is exactly zero"""
    base = rr.patch_scene(dxrs.SPHERE_DTYPE, n)
    for k, (name, sph) in enumerate(rr.motions(base)):
        o, d = rr.rays_for(make_rays, sph, rr.ray_seed(n, k))
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (rr.N_RAYS, 3)
        # (a ray that hits beyond tmin = 0.3 hits beyond tmin = 0 too: the floors at 0.3 are the floors at both)
        _, ids = oracle.closest_hits(sph, o, d, tmin=0.3, use_bvh=False)
        check_floors(ids, d, name)


@pytest.mark.parametrize("n", rr.LARGE_SIZES)
def test_large_move_ray_sets_hit_enough(dxrs, oracle, n):
    base = rr.patch_scene(dxrs.SPHERE_DTYPE, n)
    big = rr.scaled(base)
    o, d, n_first = rr.large_move_rays(make_rays, base)
    assert (np.abs(o[n_first:]) > 4e8).all() and rr.has_zero_component(d[n_first:]).all()
    n_zero = (d[n_first:] == 0).sum(1)
    assert ((n_zero == 1) | (n_zero == 2)).all() and (n_zero == 1).any() and (n_zero == 2).any()
    _, ids = oracle.closest_hits(big, o, d, tmin=0.3 * float(rr.LARGE_SCALE), use_bvh=False)  # (the floors at the larger tmin hold at 0 too)
    check_floors(ids[:n_first], d[:n_first], "large")
    assert int((ids[n_first:] != MISS).sum()) >= rr.ZERO_HITS
    # a power of two rescales every float32 operation of the intersection exactly: the hits are those of the unscaled scene
    t1, ids1 = oracle.closest_hits(base, o[:2000] / rr.LARGE_SCALE, d[:2000], tmin=0.0, use_bvh=False)
    t2, ids2 = oracle.closest_hits(big, o[:2000], d[:2000], tmin=0.0, use_bvh=False)
    assert np.array_equal(ids1, ids2) and np.array_equal((t1 * rr.LARGE_SCALE).view(np.uint32), t2.view(np.uint32))
