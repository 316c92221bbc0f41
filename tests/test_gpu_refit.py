"""The refit of moved spheres (pt_update_spheres + pt_refit_accel, or the refit a render call makes by itself), looked at directly: the
refitted tree of the lane the next frame uses is downloaded and compared bit for bit with tests/refit_reference.py, its boxes must contain
their spheres in float64, and rays traced through it must find what the brute-force kernel finds.  Covers refit_fused_small_kernel,
refit_small_kernel and refit_pass_kernel (csrc/pt_lbvh_gpu.hip) over both builders' topologies, on all three lanes of a context with
three frames in flight, for moves that change the scene bounds -- and the padding -- by orders of magnitude.  The inputs are checked on the
CPU by tests/test_refit_reference.py."""
import numpy as np
import pytest

import refit_reference as rr
from test_gpu_accel import make_rays
from util import assert_hits_match_oracle

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF


def assert_bvh_equals_brute_force(r, sph, o, d, tmins, n_floor=None):
    """BVH == brute-force kernel bit for bit in t and id, for every tmin; the hit floors of tests/test_refit_reference.py over the first n_floor
    rays (all by default) and ZERO_HITS hits among the rest.  Returns the BVH's (t, id) for the first tmin."""
    n_floor = len(o) if n_floor is None else n_floor
    first = None
    for tmin in tmins:
        t_bvh, id_bvh = r.trace_rays(o, d, tmin=tmin, use_bvh=True)
        t_bf, id_bf = r.trace_rays(o, d, tmin=tmin, use_bvh=False)
        differ = (id_bvh != id_bf) | (t_bvh.view(np.uint32) != t_bf.view(np.uint32))
        zero = rr.has_zero_component(d)
        assert not differ.any(), (tmin, int(differ.sum()), int((differ & zero).sum()), int(((id_bvh == MISS) & (id_bf != MISS)).sum()))
        hit = id_bf != MISS
        assert hit[:n_floor].mean() >= rr.HIT_SHARE, (tmin, hit[:n_floor].mean())
        assert int((hit & zero)[:n_floor].sum()) >= rr.ZERO_HITS, tmin
        assert n_floor == len(o) or int(hit[n_floor:].sum()) >= rr.ZERO_HITS, tmin
        first = first or (t_bvh, id_bvh)
    return first


def assert_refitted(r, nodes0, order0, sph):
    """the tree the next frame walks: the links and the order of the build, every box the reference's, every box around its spheres"""
    nodes, order = r.download_accel()
    assert rr.same_links(nodes, nodes0) and np.array_equal(order, order0)
    assert rr.box_mismatches(nodes, rr.refit(nodes0, order0, sph)) == 0
    assert rr.contains64(nodes, order, sph)


@pytest.mark.parametrize("fused", ["1", "0"])  # PT_FUSED_REFIT: n <= 1024 in one launch that reads the staging buffer / copy + bounds + gather + refit
@pytest.mark.parametrize("fast_build", [False, True])  # the host SAH topology adopted (n <= 4096) / the device LBVH (PT_FLAG_FAST_BUILD)
@pytest.mark.parametrize("n,no_lds", [(n, False) for n in rr.SIZES] + [(rr.NO_LDS_SIZE, True)])
def test_refit_after_each_move(dxrs, host, oracle, monkeypatch, n, no_lds, fast_build, fused):
    t = dxrs.types
    monkeypatch.setenv("PT_FUSED_REFIT", fused)
    base = rr.patch_scene(dxrs.SPHERE_DTYPE, n)
    mats, sd = t.default_material(n), host.scene(dxrs.host.SCENE_SMALL)[2]
    flags = (t.PT_FLAG_NO_LDS_SCENE if no_lds else 0) | (t.PT_FLAG_FAST_BUILD if fast_build else 0)
    r = dxrs.Renderer(flags=flags, frames_in_flight=3)
    twin = dxrs.Renderer(flags=flags, frames_in_flight=3)  # makes the same updates and frames and never calls a hook
    try:
        for x in (r, twin):
            info = x.set_scene(base, mats, sd)
            x.set_camera(host.camera(8, 8)); x.set_constants(t.graphics_settings(8, 8, bounces=2, spp=1))
        assert info.builder == (t.PT_BUILDER_HOST_SAH if 2 < n <= 4096 and not fast_build else t.PT_BUILDER_DEVICE_LBVH)
        assert not (no_lds and info.lds_resident)
        nodes0, order0 = r.download_accel()  # (no update yet: the master tree)
        assert rr.box_mismatches(nodes0, rr.refit(nodes0, order0, base)) == 0 and rr.depth(nodes0) == info.depth
        frames = [0]

        def small_frame():
            a, sa = r.render()
            b, sb = twin.render()
            assert sa.rays == sb.rays and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            frames[0] += 1

        lanes_checked = set()
        moves = rr.motions(base)
        for k, (name, sph) in enumerate(moves):
            # every second move leaves the refit to whoever needs the tree next (lane_catch_up): here the hook, in the twin the frame
            for x in (r, twin):
                x.update_spheres(sph, refit=k % 2 == 0)
            assert_refitted(r, nodes0, order0, sph)
            o, d = rr.rays_for(make_rays, sph, rr.ray_seed(n, k))
            t_bvh, id_bvh = assert_bvh_equals_brute_force(r, sph, o, d, (0.0, 0.3))
            assert_hits_match_oracle(oracle.lib, sph, o[:300], d[:300], t_bvh[:300], id_bvh[:300])
            lanes_checked.add(frames[0] % 3)
            small_frame()  # the next update lands on the next lane
            if name in ("jitter", "negative"):
                # no update for this frame: its lane is behind and takes the spheres over from the lane that received them (sync_lane_spheres)
                assert_refitted(r, nodes0, order0, sph)
                assert_bvh_equals_brute_force(r, sph, o, d, (0.0,))
                lanes_checked.add(frames[0] % 3)
                small_frame()
        assert lanes_checked == {0, 1, 2}
        # a frame rendered after the hooks were used == the same frame of the context that never called one: bits, rays, and the totals over all frames
        w, h = 64, 40
        for x in (r, twin):
            x.update_spheres(moves[0][1], refit=False)
            # (the jittered ground sphere reaches up to y = 10.3: a camera above it)
            x.set_camera(host.camera(w, h, position=(0.0, 14.0, -30.0), look_at=(0.0, 0.0, 0.0))); x.set_constants(t.graphics_settings(w, h, frame_index=3, bounces=4, spp=1))
        assert_refitted(r, nodes0, order0, moves[0][1])
        r.trace_rays(o[:64], d[:64])
        a, sa = r.render()
        b, sb = twin.render()
        assert sa.rays == sb.rays and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert len(np.unique(a.view(np.uint32)[..., :3].reshape(-1, 3), axis=0)) > 1  # (spheres and sky)
        ta, tb = r.totals(), twin.totals()
        assert (ta.rays, ta.paths, ta.pixels) == (tb.rays, tb.paths, tb.pixels) and ta.rays >= sa.rays + frames[0]
    finally:
        r.close(); twin.close()


@pytest.mark.parametrize("n", rr.LARGE_SIZES)
def test_large_coordinate_move(dxrs, host, oracle, n):
    """A scene built below 1e8 (slab_tiny = 1e-30) and moved to |coordinate| ~ 1e10 .. 1e11 by pt_update_spheres: for a ray with a zero direction
    component -o * 1e30 overflows to an infinity of one sign for both planes of a slab that holds the origin, which closes the slab -- the walk
    must give up on that axis (slab_tiny = NaN) as it does for a scene BUILT that large.  Before pt_update_spheres chose slab_tiny from the
    moved coordinates the lane kept the build's 1e-30, and on these very rays the walk returned a miss for 1748 of the brute force's 17626 hits
    (n = 65) and for 2743 of 19963 (n = 1500), every one on a ray with a zero component (all but one of such rays that hit anything); in the
    frame below 22 of the centre column's 41 pixels differed from the oracle and none elsewhere."""
    t = dxrs.types
    scale = float(rr.LARGE_SCALE)
    base = rr.patch_scene(dxrs.SPHERE_DTYPE, n)
    big = rr.scaled(base)
    mats, sd = t.default_material(n), host.scene(dxrs.host.SCENE_SMALL)[2]
    r = dxrs.Renderer(frames_in_flight=3)
    try:
        r.set_scene(base, mats, sd)
        nodes0, order0 = r.download_accel()
        r.update_spheres(big)
        assert_refitted(r, nodes0, order0, big)
        o, d, n_first = rr.large_move_rays(make_rays, base)
        t_bvh, id_bvh = assert_bvh_equals_brute_force(r, big, o, d, (0.0, 0.3 * scale), n_floor=n_first)
        for part in (slice(0, 300), slice(n_first, n_first + 300)):  # make_rays' first 300, and 300 of the zero-component rays beyond 4e8
            assert_hits_match_oracle(oracle.lib, big, o[part], d[part], t_bvh[part], id_bvh[part])
        # the frame path: zero jitter and an odd width give the centre column d.x == 0, from a camera whose x is beyond 4e8
        w, h = 63, 41
        cam = host.camera(w, h, position=(1.0 * scale, 2.0 * scale, -15.0 * scale), jitter=False)
        gs = t.graphics_settings(w, h, bounces=4, spp=1)
        r.set_camera(cam); r.set_constants(gs)
        ref, ost = oracle.render(big, mats, sd, cam, gs, threads=4)
        for _ in range(3):  # every lane: the one that received the spheres and the two that take them over
            img, st = r.render()
            assert st.rays == ost.rays and np.array_equal(img.view(np.uint32)[..., :3], ref.view(np.uint32)[..., :3])
        assert ost.rays > w * h  # (primary rays hit: there are secondary ones)
        # pt_set_scene returns every lane to the master scene and its slab_tiny
        r.set_scene(base, mats, sd)
        o1, d1 = make_rays(base, rr.N_RAYS, seed=rr.ray_seed(n, 97))
        assert_bvh_equals_brute_force(r, base, o1, d1, (0.0,))
    finally:
        r.close()
