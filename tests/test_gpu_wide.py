"""The 4-wide, quantised view of the tree on the device: the records collapse4_kernel wrote, read back with
pt_accel_download_wide, against tests/wide_reference.py -- property by property in exact arithmetic (T1), word for word against the
restatement (T2) -- and the walk through them against the binary global-memory walk (PT_WIDE=0), the brute-force kernel and the CPU
oracle (T3), with the proof that the wide walk was the one measured (T4) and a model of its stack against stack_entries (T5).
Every scene is kept out of LDS (PT_FLAG_NO_LDS_SCENE), so small ones walk the wide view too."""
import numpy as np
import pytest

import wide_reference as wr
import wide_scenes
from util import assert_hits_match_oracle

pytestmark = pytest.mark.gpu

BUILDERS = ["default", "fast_build"]  # SAH topology up to 4096 spheres, adopted / the device LBVH
N_RAYS = 40000


def _flags(dxrs, builder):
    return dxrs.types.PT_FLAG_NO_LDS_SCENE | (dxrs.types.PT_FLAG_FAST_BUILD if builder == "fast_build" else 0)


def _scene(dxrs, host, name):
    spheres = np.ascontiguousarray(wide_scenes.layout(name, host, dxrs))
    return spheres, dxrs.types.default_material(len(spheres)), host.scene(dxrs.host.SCENE_SMALL)[2]


@pytest.fixture(scope="module")
def downloads(dxrs, host):
    """(scene, builder) -> (binary records, wide records or None, accel info), downloaded once and shared read-only by T1, T2 and T5"""
    cache = {}

    def get(name, builder):
        if (name, builder) not in cache:
            spheres, materials, sd = _scene(dxrs, host, name)
            r = dxrs.Renderer(flags=_flags(dxrs, builder))
            try:
                info = r.set_scene(spheres, materials, sd)
                assert info.lds_resident == 0 and info.node_count == len(spheres) - 1
                nodes, _ = r.download_accel()
                rec = r.download_wide()
            finally:
                r.close()
            if rec is not None:
                rec.setflags(write=False)
            cache[(name, builder)] = (nodes, rec, info)
        return cache[(name, builder)]
    return get


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", wide_scenes.NAMES)
def test_t1_device_records_have_the_properties(downloads, name, builder):
    nodes, rec, info = downloads(name, builder)
    if len(nodes) <= 1:
        assert rec is None  # one node: nothing to collapse, the binary record is walked
        return
    assert rec is not None and rec.shape == (len(nodes), 16) and rec.dtype == np.uint32
    if len(nodes) + 1 <= wide_scenes.CHECK_WIDE_MAX_SPHERES:
        wr.check_wide(nodes, rec)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", wide_scenes.NAMES)
def test_t2_device_records_equal_the_restatement(downloads, name, builder):
    nodes, rec, info = downloads(name, builder)
    if rec is None:
        assert len(nodes) <= 1
        return
    expected, populated = wr.collapse4(nodes)
    if not np.array_equal(rec[populated], expected[populated]):
        pytest.fail(wr.describe_difference(nodes, np.where(populated[:, None], rec, 0), expected))
    assert not rec[~populated].any()  # the buffer is cleared before the even-depth slots are written


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", wide_scenes.NAMES)
def test_t3_wide_walk_equals_binary_walk_and_brute_force(dxrs, host, oracle, monkeypatch, name, builder):
    """`geometric` (|coordinate| up to 1e25) is the layout that showed what slab_rcp (csrc/pt_trace.h) did to a zero direction component in a
    large scene: walked as +-1e-30, -o * 1e30 overflowed beyond |o| = 3.4e8 to an infinity of one sign for both planes of a slab that holds
    the origin (in the wide walk cell * 1e30 too), the slab closed, and of the 5000 such rays the wide walk lost the hit of 547 and the binary
    global-memory walk of 1098.  Scenes that reach 1e8 now take such an axis out of the slab tests (SceneView::slab_tiny)."""
    spheres, materials, sd = _scene(dxrs, host, name)
    o, d = wide_scenes.rays(spheres, N_RAYS, seed=len(spheres) + len(name))
    wide = dxrs.Renderer(flags=_flags(dxrs, builder))
    monkeypatch.setenv("PT_WIDE", "0")  # read once, at pt_create
    binary = dxrs.Renderer(flags=_flags(dxrs, builder))
    monkeypatch.delenv("PT_WIDE")
    try:
        for r in (wide, binary):
            assert r.set_scene(spheres, materials, sd).lds_resident == 0
        assert binary.download_wide() is None
        assert (wide.download_wide() is None) == (len(spheres) <= 2)
        for tmin in (0.0, 0.3):
            t_w, id_w = wide.trace_rays(o, d, tmin=tmin, use_bvh=True)
            t_b, id_b = binary.trace_rays(o, d, tmin=tmin, use_bvh=True)
            t_f, id_f = wide.trace_rays(o, d, tmin=tmin, use_bvh=False)
            hit = float((id_f != 0xFFFFFFFF).mean())
            print(f"{name} {builder} tmin {tmin}: {hit:.3f} of the rays hit")
            wrong = []
            for what, t_x, id_x in (("wide walk", t_w, id_w), ("binary global walk", t_b, id_b)):
                bad = np.nonzero((id_x != id_f) | (t_x.view(np.uint32) != t_f.view(np.uint32)))[0]
                if len(bad):
                    wrong.append(f"{what} differs from brute force on {len(bad)} rays, kinds {np.bincount(bad % 8, minlength=8).tolist()}; first: ray {bad[0]} "
                                 f"o {o[bad[0]].tolist()} d {d[bad[0]].tolist()}: id {id_x[bad[0]]} t {t_x[bad[0]]!r}, brute force id {id_f[bad[0]]} t {t_f[bad[0]]!r}")
            assert not wrong, "; ".join(wrong)
            assert hit > 0.2
            if tmin == 0.0:
                assert_hits_match_oracle(oracle.lib, spheres, o[:300], d[:300], t_w[:300], id_w[:300])
    finally:
        wide.close(); binary.close()


@pytest.mark.parametrize("name", ["demo", "procedural_40000"])
def test_t4_wide_walk_visits_fewer_nodes(dxrs, host, monkeypatch, name):
    """the counts of pt_trace_rays_stats show which walk ran: one visit of a wide node stands for up to three of binary nodes"""
    spheres, materials, sd = _scene(dxrs, host, name)
    o, d = wide_scenes.rays(spheres, N_RAYS, seed=4)
    visits = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("PT_WIDE", knob)
        r = dxrs.Renderer(flags=_flags(dxrs, "default"))
        try:
            r.set_scene(spheres, materials, sd)
            assert (r.download_wide() is not None) == (knob == "1")
            t, ids, v = r.trace_rays_stats(o, d)
            visits[knob] = (int(v[:, 0].astype(np.int64).sum()), t.copy(), ids.copy())
        finally:
            r.close()
    assert np.array_equal(visits["1"][2], visits["0"][2]) and np.array_equal(visits["1"][1].view(np.uint32), visits["0"][1].view(np.uint32))
    print(f"{name}: {visits['1'][0]} wide node visits, {visits['0'][0]} binary: ratio {visits['1'][0] / visits['0'][0]:.3f}")
    assert 0 < visits["1"][0] < visits["0"][0]


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["concentric", "geometric"])
def test_t5_stack_model_stays_within_stack_entries(downloads, name, builder):
    """wide_reference.stack_model over the device's records: nothing on the device is driven towards the bound"""
    nodes, rec, info = downloads(name, builder)
    o, d = wr.stack_rays(name, 2000, seed=9)
    peak = wr.stack_model(rec, o, d)
    print(f"{name} {builder}: depth {info.depth}, largest stack occupancy {peak}, stack_entries {info.depth + (info.depth + 1) // 2 + 2}")
    assert peak <= info.depth + (info.depth + 1) // 2 + 2
    if name == "concentric":
        assert peak >= info.depth
