"""Row N24 -- pt_physics_publish / pt_render_gbuffer_published (DESIGN.md spec S28): the simulated pose handed to the frames on the device.

CPU: the ABI, and csrc/pt_publish_order.h (through tests/hostshim/publish_host.cpp) against a restatement that keeps every outstanding read
as a (lane, slot) pair.  GPU: two contexts with the same scene and the same simulation; A publishes, B goes pt_physics_download ->
pt_update_spheres (-> pt_update_rotations): images, trees and ray hits are compared as uint32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_physics import ALL, ATTRACTOR, LARGE, cluster, density_bodies, settings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 160, 90


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ CPU: ABI
def test_library_exports_and_binding(dxrs):
    lib = dxrs.load_hip().lib
    for name in ("pt_physics_publish", "pt_render_gbuffer_published"):
        assert hasattr(lib, name) and name in dxrs.binding.API_SYMBOLS
    assert callable(dxrs.Renderer.physics_publish)
    import inspect
    assert "previous" in inspect.signature(dxrs.Renderer.render_gbuffer).parameters
    assert "previous" in inspect.signature(dxrs.Renderer.render_gbuffer_device).parameters
    assert lib.pt_physics_publish(None) == 1 and lib.pt_render_gbuffer_published(None, None, None) == 1  # PT_ERR_INVALID_ARG


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_as_c_and_cxx(tmp_path, compiler, lang):
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "pt_api.h"\nPtStatus (*a)(PtContext *) = pt_physics_publish;\n'
                   "PtStatus (*b)(PtContext *, const PtRect *, const PtGBuffer *) = pt_render_gbuffer_published;\nint main(void) { return a == 0 || b == 0; }\n")
    res = subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ------------------------------------------------------------------------------------------------ CPU: the ordering header
@pytest.fixture(scope="module")
def pub():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_publish_shim())
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.pub_new.restype = vp
    lib.pub_new.argtypes = [u32]
    lib.pub_free.argtypes = [vp]
    for name in ("pub_ring_size", "pub_max_lanes", "pub_max_slots"):
        getattr(lib, name).restype = u32
    lib.pub_ring_size.argtypes = [u32]
    lib.pub_slot.restype = u32
    lib.pub_slot.argtypes = [vp, u64]
    lib.pub_prev_intact.restype = C.c_int
    lib.pub_prev_intact.argtypes = [vp, u64]
    lib.pub_publish.argtypes = [vp, C.c_int, vp]
    lib.pub_take.argtypes = [vp, u32, C.c_int, C.c_int, vp]
    lib.pub_reader_done.argtypes = [vp, u32]
    for name in ("pub_host_spheres", "pub_host_rotations", "pub_restart", "pub_forget"):
        getattr(lib, name).argtypes = [vp]
    lib.pub_state.argtypes = [vp, vp]
    return lib


class Header:
    """pt_publish_order.h through the shim"""

    def __init__(self, lib, n_lanes):
        self.lib, self.o, self.slots = lib, lib.pub_new(n_lanes), lib.pub_max_slots()

    def close(self):
        self.lib.pub_free(self.o)

    def publish(self, with_rot=True):
        out = (C.c_uint64 * 3)()
        self.lib.pub_publish(self.o, int(with_rot), out)
        return int(out[0]), int(out[1]), int(out[2])

    def take(self, lane, cur=True, prev=False):
        out = (C.c_int64 * 3)()
        self.lib.pub_take(self.o, lane, int(cur), int(prev), out)
        return int(out[0]), int(out[1]), int(out[2])

    def state(self):
        out = (C.c_uint64 * (4 + 2 * self.slots))()
        self.lib.pub_state(self.o, out)
        v = [int(x) for x in out]
        return dict(gen=v[0], first=v[1], sph_live=bool(v[2]), rot_live=bool(v[3]), slot_gen=v[4:4 + self.slots], readers=v[4 + self.slots:])


class Model:
    """the rules of pt_publish_order.h restated: every read of a slot that may still be running is a (lane, slot) pair"""

    def __init__(self, n_lanes):
        self.ring, self.gen, self.first, self.slot_gen, self.reads = n_lanes + 2, 0, 1, {}, []
        self.sph_live = self.rot_live = False

    def prev_intact(self):
        g = self.gen
        return g >= 2 and g - 1 >= self.first and self.slot_gen.get((g - 1) % self.ring) == g - 1

    def publish(self, with_rot):
        self.gen += 1
        s = self.gen % self.ring
        mask = 0
        for lane, slot in self.reads:
            if slot == s:
                mask |= 1 << lane
        self.reads = [r for r in self.reads if r[1] != s]  # the stream wait stands for them
        self.slot_gen[s] = self.gen
        self.sph_live = True
        self.rot_live = self.rot_live or with_rot
        return self.gen, s, mask

    def take(self, lane, cur, prev):
        if self.gen == 0:
            return 0, 0, -1
        s = self.gen % self.ring
        if cur:
            self.reads.append((lane, s))
        ps = -1
        if prev and self.prev_intact():
            ps = (self.gen - 1) % self.ring
            self.reads.append((lane, ps))
        return self.gen, s, ps

    def mask(self, slot):
        m = 0
        for lane, s in self.reads:
            if s == slot:
                m |= 1 << lane
        return m


def check_state(h, m):
    st = h.state()
    assert (st["gen"], st["first"], st["sph_live"], st["rot_live"]) == (m.gen, m.first, m.sph_live, m.rot_live)
    for s in range(m.ring):
        # the markers a publish would be told to wait for are exactly the outstanding readers of the slot
        assert st["readers"][s] == m.mask(s) and st["slot_gen"][s] == m.slot_gen.get(s, 0)
    # the next publish writes neither the newest generation's slot nor, where intact, its predecessor's
    nxt = h.lib.pub_slot(h.o, m.gen + 1)
    assert bool(h.lib.pub_prev_intact(h.o, m.gen)) == m.prev_intact()
    if m.gen:
        assert nxt != h.lib.pub_slot(h.o, m.gen)
    if m.prev_intact():
        assert nxt != h.lib.pub_slot(h.o, m.gen - 1)


@pytest.mark.parametrize("n_lanes", [1, 2, 3, 8])
def test_order_header_matches_restatement(pub, n_lanes):
    """600 random sequences per lane count (2400 in all) of publish / take / reader-done / pt_update_spheres / pt_update_rotations / restart /
    forget, every answer and the whole state compared after every event"""
    assert pub.pub_ring_size(n_lanes) == n_lanes + 2 <= pub.pub_max_slots() and n_lanes <= pub.pub_max_lanes()
    rng = np.random.default_rng(n_lanes)
    fallbacks = waits = 0
    for _ in range(600):
        h, m = Header(pub, n_lanes), Model(n_lanes)
        try:
            for _ in range(int(rng.integers(20, 80))):
                kind = int(rng.integers(17))
                if kind < 6:
                    rot = bool(rng.integers(2))
                    got, want = h.publish(rot), m.publish(rot)
                    assert got == want
                    waits += want[2] != 0
                elif kind < 11:
                    lane, cur, prev = int(rng.integers(n_lanes)), bool(rng.integers(4)), bool(rng.integers(2))
                    had_prev = m.prev_intact()
                    got, want = h.take(lane, cur, prev), m.take(lane, cur, prev)
                    assert got == want
                    if prev and m.gen:
                        assert (got[2] == -1) == (not had_prev)  # "previous = current" exactly when generation g - 1 does not exist
                        fallbacks += got[2] == -1
                elif kind < 13:
                    lane = int(rng.integers(n_lanes))
                    pub.pub_reader_done(h.o, lane)
                    m.reads = [r for r in m.reads if r[0] != lane]
                elif kind == 13:
                    pub.pub_host_spheres(h.o)
                    m.sph_live = False
                elif kind == 14:
                    pub.pub_host_rotations(h.o)
                    m.rot_live = False
                elif kind == 15:
                    pub.pub_restart(h.o)
                    m.first = m.gen + 1
                else:
                    pub.pub_forget(h.o)
                    m.first, m.sph_live, m.rot_live = m.gen + 1, False, False
                check_state(h, m)
        finally:
            h.close()
    assert fallbacks > 100 and waits > 100


def test_order_known_answers(pub):
    n_lanes, ring = 3, 5
    h = Header(pub, n_lanes)
    try:
        # nothing published: nothing to take
        assert h.take(0, True, True) == (0, 0, -1) and h.state()["readers"] == [0] * h.slots
        # the first publish: generation 1 in slot 1, nobody to wait for, no predecessor
        assert h.publish() == (1, 1, 0)
        assert h.take(0, True, True) == (1, 1, -1)
        assert h.state()["readers"][1] == 0b001
        pub.pub_reader_done(h.o, 0)
        # ring + 1 publishes without a reader: slots 2, 3, 4, 0, 1, 2 -- never a wait; the newest has its predecessor
        assert [h.publish() for _ in range(ring + 1)] == [(g, g % ring, 0) for g in range(2, ring + 3)]
        assert h.take(1, True, True) == (7, 2, 1)
        # a lane that sleeps through `ring` publishes: lane 2 read generation 7 (slot 2) and its predecessor (slot 1) ...
        assert h.take(2, True, True) == (7, 2, 1)
        got = [h.publish() for _ in range(ring)]
        # ... so publish 11 (slot 1) and publish 12 (slot 2) are told to wait for lanes 1 and 2, the others for nobody
        assert got == [(8, 3, 0), (9, 4, 0), (10, 0, 0), (11, 1, 0b110), (12, 2, 0b110)]
        # ... and when it wakes up it takes the newest generation, whose predecessor is intact
        assert h.take(2, True, True) == (12, 2, 1)
        # pt_update_spheres between two publishes: the host's spheres are the newest until the next publish; its predecessor is still
        # the generation published before it
        pub.pub_host_spheres(h.o)
        assert h.state()["sph_live"] is False and h.state()["rot_live"] is True
        assert h.publish(with_rot=False) == (13, 3, 0)
        assert h.state()["sph_live"] is True and h.take(0, True, True) == (13, 3, 2)
        # a new simulation: the newest generation, and the next one, have no predecessor; the one after it has
        pub.pub_restart(h.o)
        assert h.take(0, False, True) == (13, 3, -1)
        assert h.publish()[0] == 14 and h.take(0, True, True) == (14, 4, -1)
        assert h.publish()[0] == 15 and h.take(0, True, True) == (15, 0, 4)
        # pt_set_scene: nothing is live
        pub.pub_forget(h.o)
        st = h.state()
        assert (st["sph_live"], st["rot_live"], st["first"]) == (False, False, 16)
    finally:
        h.close()


def test_sanitizer_program(tmp_path):
    """tests/hostshim/publish_sanitize.cpp: the header over the same kinds of sequences under AddressSanitizer + UBSan, as a stand-alone program
    run as a child process"""
    import __graft_entry__ as g

    exe = g.build_publish_sanitizer(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "publish_sanitize ok" in res.stdout, res.stdout + res.stderr


# ------------------------------------------------------------------------------------------------ GPU
def cluster_scene(dxrs, seed, n):
    """test_physics.cluster as a renderable scene: materials of every kind, a camera in front of the cube"""
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    scene = cluster(seed, n)
    sph = scene[0]
    rng = np.random.default_rng(1000 + seed)
    spheres = np.zeros(n, SPHERE_DTYPE)
    for i, name in enumerate(("cx", "cy", "cz", "r")):
        spheres[name] = sph[:, i]
    mats = default_material(n)
    if n:
        mats["BaseColor"][:, :3] = rng.uniform(0.1, 1, (n, 3))
        mats["Metallic"] = rng.choice([0.0, 0.3, 1.0], n)
        mats["Roughness"] = rng.uniform(0, 1, n)
        mats["Transmission"] = rng.choice([0.0, 0.0, 0.8], n)
        mats["EmissiveColor"] = rng.uniform(0, 1, (n, 3)) * (rng.random((n, 1)) < 0.2)
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.4, 0.5, 0.7, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    side = float(sph[:, :3].max()) if n else 1.0
    centre = (side / 2, side / 2, side / 2)
    position = (side / 2, side / 2, -0.8 * side)
    return scene, spheres, mats, sd, position, centre


def as_spheres(base, s):
    moved = base.copy()
    for i, name in enumerate(("cx", "cy", "cz", "r")):
        moved[name] = s[:, i]
    return moved


class Pair:
    """contexts A (publishes) and B (download -> pt_update_spheres -> pt_update_rotations) over one scene and one simulation"""

    def __init__(self, dxrs, host, spheres, mats, sd, scene, lanes_a=0, textures=None, attractors=None, camera=None, size=(W, H), env=None):
        self.dxrs, self.host, self.base, self.mats, self.sd, self.textured = dxrs, host, spheres, mats, sd, textures is not None
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.a, self.b = dxrs.Renderer(device=0, frames_in_flight=lanes_a), dxrs.Renderer(device=0)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        self.size = size
        for r in (self.a, self.b):
            r.set_scene(spheres, mats, sd)
            if textures is not None:
                r.set_textures(textures)
            self.set_frame(r, 0, camera)
            r.physics_create(*scene, settings())
            if attractors is not None:
                r.physics_set_attractors(attractors)
        self.camera = camera

    def set_frame(self, r, k, camera=None):
        w, h = self.size
        r.set_camera(camera or self.host.camera(w, h, jitter_index=k))
        r.set_constants(self.dxrs.types.graphics_settings(w, h, frame_index=k, bounces=8, spp=1))

    def step(self, dt=1 / 60, substeps=1):
        for r in (self.a, self.b):
            r.physics_step(dt, substeps, report=False)

    def hand_over(self):
        """-> the pose B downloaded (spheres as the scene's dtype, rotations)"""
        self.a.physics_publish()
        s, rot, _, _ = self.b.physics_download()
        moved = as_spheres(self.base, s)
        self.b.update_spheres(moved)
        if self.textured:
            self.b.update_rotations(rot)
        return moved, rot

    def close(self):
        self.a.close()
        self.b.close()


def rays_for(position, centre, n=4096, seed=5):
    rng = np.random.default_rng(seed)
    o = np.tile(np.asarray(position, np.float32), (n, 1)) + rng.normal(size=(n, 3)).astype(np.float32) * 0.05
    d = (np.asarray(centre, np.float32) - o) + rng.normal(size=(n, 3)).astype(np.float32) * 0.6 * float(np.linalg.norm(np.subtract(centre, position)))
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def compare_everything(p, rays, what):
    img_a, _ = p.a.render()
    img_b, _ = p.b.render()
    assert np.array_equal(bits(img_a), bits(img_b)), f"{what}: images differ"
    if rays is not None:
        ta, ia = p.a.trace_rays(*rays)
        tb, ib = p.b.trace_rays(*rays)
        assert np.array_equal(bits(ta), bits(tb)) and np.array_equal(ia, ib), f"{what}: pt_trace_rays differs"
    if p.a.accel.node_count:
        na, oa = p.a.download_accel()
        nb, ob = p.b.download_accel()
        assert na.tobytes() == nb.tobytes() and np.array_equal(oa, ob), f"{what}: trees differ"
    return img_a


@pytest.mark.gpu
@pytest.mark.parametrize("n,fused", [(0, 1), (1, 1), (2, 1), (3, 1), (64, 1), (65, 1), (1024, 1), (1025, 1), (1024, 0)])
def test_gpu_sizes(dxrs, host, n, fused):
    scene, spheres, mats, sd, position, centre = cluster_scene(dxrs, 200 + n, n)
    cam = host.camera(W, H, position=position, look_at=centre)
    p = Pair(dxrs, host, spheres, mats, sd, scene, camera=cam, env={"PT_FUSED_REFIT": str(fused)})
    try:
        first = compare_everything(p, rays_for(position, centre), "before any publish")
        imgs = []
        for k in range(3):
            p.step()
            p.hand_over()
            imgs.append(compare_everything(p, rays_for(position, centre), f"step {k}"))
        if n >= 2:
            assert not np.array_equal(bits(imgs[-1]), bits(first))  # the spheres have moved in the picture
            _, ids = p.a.trace_rays(*rays_for(position, centre))
            assert (ids != 0xFFFFFFFF).sum() > 20
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_global_memory_tree(dxrs, host):
    """32 769 bodies: the tree in global memory, walked with the 32-bit stack"""
    n = 32769
    scene, spheres, mats, sd, position, centre = cluster_scene(dxrs, 9, n)
    cam = host.camera(W, H, position=position, look_at=centre)
    p = Pair(dxrs, host, spheres, mats, sd, scene, camera=cam)
    try:
        for k in range(2):
            p.step()
            p.hand_over()
            img_a, _ = p.a.render()
            img_b, _ = p.b.render()
            assert np.array_equal(bits(img_a), bits(img_b)), f"step {k}"
            rays = rays_for(position, centre)
            ta, ia = p.a.trace_rays(*rays)
            tb, ib = p.b.trace_rays(*rays)
            assert np.array_equal(bits(ta), bits(tb)) and np.array_equal(ia, ib)
    finally:
        p.close()


def demo_pair(dxrs, host, lanes, n_small=None):
    """the demo scene on `lanes` lanes with Star gravity, as test_gpu_whole_loop_matches_oracle sets it up (untextured)"""
    spheres0, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    n = len(spheres0)
    sph = np.stack([spheres0[k] for k in ("cx", "cy", "cz", "r")], 1).astype(np.float32)
    bodies = density_bodies(sph[:, 3])
    bodies["InvMass"][-1] = 0
    bodies["Flags"][-1] = LARGE
    ang = np.zeros((n, 3), np.float32)
    ang[:, 1] = 2.0
    att = np.array([(n - 1, 1, 10.0, ALL)], ATTRACTOR)
    return Pair(dxrs, host, spheres0, materials, sd, (sph, bodies, None, ang, None), lanes_a=lanes, attractors=att)


@pytest.mark.gpu
def test_gpu_lanes_catch_up(dxrs, host):
    """three lanes, one publish, four frames: every lane takes the pose on its own (the failure sync_lane_spheres was written for)"""
    p = demo_pair(dxrs, host, 3)
    try:
        p.step(0.25, 15)
        p.hand_over()
        want, _ = p.b.render()
        plain = host.scene(dxrs.host.SCENE_DEMO, seed=0)
        for k in range(4):
            img, _ = p.a.render()
            assert np.array_equal(bits(img), bits(want)), f"frame {k}"
        r = dxrs.Renderer(device=0)
        try:
            r.set_scene(*plain); p.set_frame(r, 0)
            assert not np.array_equal(bits(r.render()[0]), bits(want))  # the pose shows
        finally:
            r.close()
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """eight rounds of step -> publish -> frame on three lanes into three rotating buffers with no synchronisation inside the loop"""
    import torch

    p = demo_pair(dxrs, host, 3)
    try:
        outs = [torch.zeros((H, W, 4), device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        for k in range(8):
            p.a.physics_step(1 / 15, 4, report=False)
            p.a.physics_publish()
            p.a.render_device(outs[k % 3].data_ptr())
        want = {}
        for k in range(8):
            p.b.physics_step(1 / 15, 4, report=False)
            s, _, _, _ = p.b.physics_download()
            p.b.update_spheres(as_spheres(p.base, s))
            want[k] = p.b.render()[0]
        p.a.synchronize()
        for k in (5, 6, 7):  # what the three buffers hold at the end
            assert np.array_equal(bits(outs[k % 3].cpu().numpy()), bits(want[k])), f"round {k}"
        assert not np.array_equal(bits(want[5]), bits(want[7]))
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_ring_reuse(dxrs, host):
    """2R + 1 publishes without a frame, then three frames; then one more publish and a frame"""
    p = demo_pair(dxrs, host, 3)
    try:
        ring = 3 + 2
        for _ in range(2 * ring + 1):
            p.a.physics_step(1 / 60, 1, report=False)
            p.a.physics_publish()
            p.b.physics_step(1 / 60, 1, report=False)
        s, _, _, _ = p.b.physics_download()
        p.b.update_spheres(as_spheres(p.base, s))
        want, _ = p.b.render()
        for k in range(3):
            assert np.array_equal(bits(p.a.render()[0]), bits(want)), f"frame {k}"
        p.step(0.25, 15)
        p.hand_over()
        want2, _ = p.b.render()
        assert np.array_equal(bits(p.a.render()[0]), bits(want2)) and not np.array_equal(bits(want), bits(want2))
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_mixing_with_host_updates(dxrs, host):
    p = demo_pair(dxrs, host, 3)
    try:
        master, _ = p.b.render()
        p.step(0.25, 15)
        p.hand_over()
        simulated, _ = p.b.render()
        assert np.array_equal(bits(p.a.render()[0]), bits(simulated))
        # publish -> pt_update_spheres(host pose) -> render: the host pose (the newest call wins)
        shifted = p.base.copy()
        shifted["cy"] += np.float32(0.75)
        p.a.physics_publish()
        for r in (p.a, p.b):
            r.update_spheres(shifted)
        host_img, _ = p.b.render()
        for k in range(4):
            assert np.array_equal(bits(p.a.render()[0]), bits(host_img)), f"host pose, frame {k}"
        with pytest.raises(dxrs.PtError, match="not a published pose"):
            p.a.render_gbuffer(["MotionVector"], previous="published")
        # ... then publish -> render: the simulated pose again
        p.a.physics_publish()
        for k in range(4):
            assert np.array_equal(bits(p.a.render()[0]), bits(simulated)), f"simulated pose, frame {k}"
        assert not np.array_equal(bits(host_img), bits(simulated))
        # pt_set_scene after a publish renders the master scene
        p.a.physics_publish()
        p.a.set_scene(p.base, p.mats, p.sd)
        for k in range(4):
            assert np.array_equal(bits(p.a.render()[0]), bits(master)), f"master scene, frame {k}"
    finally:
        p.close()


def gbuffers_equal(ga, gb, what):
    for name in ga:
        assert np.array_equal(bits(ga[name]), bits(gb[name])), f"{what}: {name} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("textured", [False, True])
def test_gpu_gbuffer_published(dxrs, host, textured):
    """all 13 channels over three publishes: A's previous pose comes from the ring, B is given the pose of the round before"""
    spheres0, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    sd.IsStatic = 0  # (the demo's scene data says static, as the reference's does while the physics rests)
    n = len(spheres0)
    tex = host.demo_textures(0, 0.0) if textured else None
    sph = np.stack([spheres0[k] for k in ("cx", "cy", "cz", "r")], 1).astype(np.float32)
    bodies = density_bodies(sph[:, 3])
    bodies["InvMass"][-1] = 0
    bodies["Flags"][-1] = LARGE
    ang = np.zeros((n, 3), np.float32)
    ang[:, 1] = 2.0
    att = np.array([(n - 1, 1, 10.0, ALL)], ATTRACTOR)
    cam = host.camera_matrices(W, H)
    p = Pair(dxrs, host, spheres0, materials, sd, (sph, bodies, None, ang, tex.rotations if textured else None), lanes_a=3, textures=tex, attractors=att, camera=cam)
    try:
        prev = None
        moving = 0
        for k in range(3):
            p.step(0.25, 15)
            pose = p.hand_over()
            ga = p.a.render_gbuffer(previous="published")
            gb = p.b.render_gbuffer(previous_spheres=prev[0] if prev else None, previous_rotations=prev[1] if prev and textured else None)
            gbuffers_equal(ga, gb, f"round {k}")
            still = p.b.render_gbuffer(channels=["MotionVector"])
            moving += int((bits(still["MotionVector"]) != bits(ga["MotionVector"])).any())
            assert (k == 0) == np.array_equal(bits(still["MotionVector"]), bits(ga["MotionVector"]))  # round 0: no object motion
            # the frame of the round: the lane is up to date, the frame takes nothing again
            assert np.array_equal(bits(p.a.render()[0]), bits(p.b.render()[0]))
            prev = pose
        assert moving == 2
        # IsStatic is honoured as on B: no previous pose is used
        static = type(sd).from_buffer_copy(sd)
        static.IsStatic = 1
        p.step(0.25, 15)
        for r in (p.a, p.b):
            r.set_scene(spheres0, materials, static)
            if textured:
                r.set_textures(tex)
        pose = p.hand_over()
        p.step(0.25, 15)
        pose2 = p.hand_over()
        gbuffers_equal(p.a.render_gbuffer(previous="published"), p.b.render_gbuffer(previous_spheres=pose[0], previous_rotations=pose[1] if textured else None), "IsStatic")
        # a new simulation: its first published pose has no predecessor
        for r in (p.a, p.b):
            r.set_scene(spheres0, materials, sd)
            if textured:
                r.set_textures(tex)
        p.hand_over()
        p.hand_over()
        for r in (p.a, p.b):
            r.physics_create(as_array(pose2[0]), bodies, None, ang, pose2[1] if textured else None, settings())
            r.physics_set_attractors(att)
        gbuffers_equal(p.a.render_gbuffer(previous="published"), p.b.render_gbuffer(), "after pt_physics_create, before a publish")
        p.step(0.25, 15)
        p.hand_over()
        gbuffers_equal(p.a.render_gbuffer(previous="published"), p.b.render_gbuffer(), "the first publish of a new simulation")
    finally:
        p.close()


def as_array(spheres):
    return np.stack([spheres[k] for k in ("cx", "cy", "cz", "r")], 1).astype(np.float32)


@pytest.mark.gpu
def test_gpu_textured_demo_scene_matches_oracle(dxrs, host, oracle):
    """the set-up of test_gpu_whole_loop_matches_oracle through publish: two rounds of 15 substeps, each frame the oracle's image of B's
    downloaded pose, bit for bit"""
    spheres0, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    n = len(spheres0)
    w, hgt, rect = 640, 360, (200, 140, 240, 120)
    sph = as_array(spheres0)
    bodies = density_bodies(sph[:, 3])
    bodies["InvMass"][-1] = 0
    bodies["Flags"][-1] = LARGE
    att = np.array([(n - 1, 1, 10.0, ALL)], ATTRACTOR)
    tex = host.demo_textures(0, 0.0)
    ang = np.zeros((n, 3), np.float32)
    ang[:, 1] = 2.0
    p = Pair(dxrs, host, spheres0, materials, sd, (sph, bodies, None, ang, tex.rotations.copy()), textures=tex, attractors=att, size=(w, hgt))
    try:
        for k in range(2):
            p.step(0.25, 15)
            moved, rot = p.hand_over()
            tex.rotations[:] = rot
            gs = dxrs.types.graphics_settings(w, hgt, frame_index=k, bounces=8, spp=1)
            p.a.set_camera(host.camera(w, hgt, jitter_index=k)); p.a.set_constants(gs)
            img, _ = p.a.render(rect)
            want, _ = oracle.render(moved, materials, sd, host.camera(w, hgt, jitter_index=k), gs, rect=rect, threads=8, textures=tex)
            assert np.array_equal(bits(img)[..., :3], bits(want)[..., :3]), f"frame {k}"
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_chain_queued_equals_chain_synchronised(dxrs, host):
    """G-buffer (published) -> pt_restir_di -> pt_render_with_di on three lanes, queued without waits, against the same chain
    synchronised after every call"""
    import torch
    from dxrs_amd.types import GBUFFER_CHANNELS, RESTIR_DI_TEXTURES

    width = dict(GBUFFER_CHANNELS)
    rounds = 4

    def run(sync):
        p = demo_pair(dxrs, host, 3)
        try:
            r = p.a
            r.set_camera(host.camera_matrices(W, H)); r.set_constants(dxrs.types.graphics_settings(W, H, bounces=8, spp=1, di=True))
            sets = []
            for _ in range(3):
                gb = {name: torch.zeros((H, W, width[name]), device="cuda") for name in RESTIR_DI_TEXTURES[:8]}
                sets.append((gb, torch.zeros((H, W, 4), device="cuda"), torch.zeros((H, W, 4), device="cuda"), torch.zeros((H, W, 4), device="cuda")))
            torch.cuda.synchronize()
            results = []
            for k in range(rounds):
                gb, diff, spec, out = sets[k % 3]
                r.physics_step(1 / 15, 4, report=False)
                r.physics_publish()
                calls = (lambda: r.render_gbuffer_device({name: b.data_ptr() for name, b in gb.items()}, previous="published"),
                         lambda: r.restir_di_device(W, H, {**{name: b.data_ptr() for name, b in gb.items()}, "Diffuse": diff.data_ptr(), "Specular": spec.data_ptr()}, frame_index=k),
                         lambda: r.render_with_di_device(out.data_ptr(), diff.data_ptr(), spec.data_ptr()))
                for call in calls:
                    call()
                    if sync:
                        r.synchronize()
                if sync:
                    results.append(out.cpu().numpy().copy())
            r.synchronize()
            if not sync:
                results = {k: sets[k % 3][3].cpu().numpy().copy() for k in range(rounds - 3, rounds)}
            return results
        finally:
            p.close()

    want, got = run(True), run(False)
    for k, img in got.items():
        assert np.array_equal(bits(img), bits(want[k])), f"round {k}"
    assert not np.array_equal(bits(want[0]), bits(want[rounds - 1]))


@pytest.mark.gpu
def test_gpu_errors_leave_everything_untouched(dxrs, host):
    spheres0, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    n = len(spheres0)
    sph = as_array(spheres0)
    bodies = density_bodies(sph[:, 3])
    lin = np.zeros((n, 3), np.float32)
    lin[:, 1] = 1.0
    r = dxrs.Renderer(device=0)
    try:
        with pytest.raises(dxrs.PtError, match="pt_physics_create has not been called") as e:
            r.physics_publish()
        assert e.value.status == 4  # PT_ERR_STATE
        r.physics_create(sph, bodies, lin, None, None, settings())
        with pytest.raises(dxrs.PtError, match="pt_set_scene") as e:
            r.physics_publish()  # no scene
        assert e.value.status == 4
        r.set_scene(spheres0, materials, sd, build=False)
        with pytest.raises(dxrs.PtError, match="pt_build_accel") as e:
            r.physics_publish()  # no accel
        assert e.value.status == 4
        r.build_accel()
        r.set_camera(host.camera(W, H)); r.set_constants(dxrs.types.graphics_settings(W, H, bounces=8, spp=1))
        before_img, before_state = r.render()[0], r.physics_download()
        r.physics_create(sph[:-1], bodies[:-1], lin[:-1], None, None, settings())
        with pytest.raises(dxrs.PtError, match="body count") as e:
            r.physics_publish()
        assert e.value.status == 1  # PT_ERR_INVALID_ARG
        assert np.array_equal(bits(r.render()[0]), bits(before_img))
        with pytest.raises(dxrs.PtError, match="not a published pose") as e:
            r.render_gbuffer(["MotionVector"], previous="published")
        assert e.value.status == 4
        r.physics_create(sph, bodies, lin, None, None, settings())
        for a, b in zip(r.physics_download(), before_state):
            assert np.array_equal(bits(a), bits(b))
        r.physics_step(0.25, 15)
        r.physics_publish()
        assert not np.array_equal(bits(r.render()[0]), bits(before_img))
    finally:
        r.close()
    # no device builder
    r = dxrs.Renderer(device=0, flags=dxrs.types.PT_FLAG_HOST_LBVH)
    try:
        r.set_scene(spheres0, materials, sd)
        r.set_camera(host.camera(W, H)); r.set_constants(dxrs.types.graphics_settings(W, H, bounces=8, spp=1))
        r.physics_create(sph, bodies, lin, None, None, settings())
        r.physics_step(0.25, 15)
        before_img, before_state = r.render()[0], r.physics_download()
        with pytest.raises(dxrs.PtError, match="device LBVH builder") as e:
            r.physics_publish()
        assert e.value.status == 5  # PT_ERR_UNSUPPORTED
        assert np.array_equal(bits(r.render()[0]), bits(before_img))
        for a, b in zip(r.physics_download(), before_state):
            assert np.array_equal(bits(a), bits(b))
        # an empty scene with no bodies: nothing to do
        r.set_scene(spheres0[:0], materials[:0], sd)
        r.physics_create(sph[:0], bodies[:0], None, None, None, settings())
        sky = r.render()[0]
        r.physics_publish()
        assert np.array_equal(bits(r.render()[0]), bits(sky))
        r.physics_create(sph[:3], bodies[:3], None, None, None, settings())
        with pytest.raises(dxrs.PtError, match="body count"):
            r.physics_publish()
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, tmp_path):
    """dxrs::Physics in publishing mode and GBufferGeneration::RenderPublished (host/Physics.hpp, host/GBufferGeneration.hpp) from C++,
    against pt_api.h alone: the frame loop of tests/cpp/host_publish.cpp gives the pose, the frame and the motion vectors of the same loop
    made from Python with the bodies the program built"""
    from test_physics import BODY

    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_publish")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_publish.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    outp = str(tmp_path / "publish.bin")
    ticks = 12
    res = subprocess.run([exe, str(ticks), str(W), str(H), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "published" in res.stdout, res.stdout + res.stderr
    raw = np.fromfile(outp, np.float32)
    n = int(raw[0])
    blocks = np.split(raw[1:], np.cumsum([n * 4, n * 4, n * 3, n * 3, 16, n * 4, n * 4, n * 4, W * H * 4, W * H * 3]))
    sph0, body_raw, lin0, ang0, att_raw, rot0, sph1, rot1, frame, motion = blocks[:10]
    bodies = body_raw.view(np.uint32).reshape(n, 4).copy().view(BODY).reshape(n)
    att = att_raw.view(np.uint32).reshape(4, 4).copy().view(ATTRACTOR).reshape(4)
    att = att[att["Kind"] <= 1]
    spheres0, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    assert n == len(spheres0) and np.array_equal(sph0.reshape(n, 4)[:, 0], spheres0["cx"])
    r = dxrs.Renderer(device=0)
    try:
        r.set_scene(spheres0, materials, sd)
        r.set_camera(host.camera(W, H, jitter=False)); r.set_constants(dxrs.types.graphics_settings(W, H, bounces=8, spp=1))
        r.physics_create(sph0.reshape(n, 4), bodies, lin0.reshape(n, 3), ang0.reshape(n, 3), rot0.reshape(n, 4), None)
        r.physics_set_attractors(att)
        for _ in range(ticks):
            r.physics_step(1 / 60, 1, report=False)
            r.physics_publish()
            gb = r.render_gbuffer(["MotionVector"], previous="published")
            img, _ = r.render()
        s, rot, _, _ = r.physics_download()
        assert np.array_equal(bits(s), bits(sph1.reshape(n, 4))) and np.array_equal(bits(rot), bits(rot1.reshape(n, 4)))
        assert not np.array_equal(bits(s), bits(sph0.reshape(n, 4)))
        assert np.array_equal(bits(img), bits(frame.reshape(H, W, 4)))
        written = ~np.isnan(gb["MotionVector"])  # (the pass leaves pixels without a surface as they were)
        assert written.any() and np.array_equal(bits(gb["MotionVector"])[written], bits(motion.reshape(H, W, 3))[written])
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 2, 8])
def test_gpu_random_interleavings(dxrs, host, lanes):
    """random sequences of step / publish / pt_update_spheres / pt_refit_accel / frame / pt_trace_rays on 1, 2 and 8 lanes against the
    synchronous download path on one lane"""
    rng = np.random.default_rng(40 + lanes)
    p = demo_pair(dxrs, host, lanes)
    try:
        rays = rays_for((0.0, 0.0, -15.0), (0.0, 0.0, 0.0), n=1024)
        frames = 0
        for op in rng.choice(["step", "publish", "host", "refit", "frame", "frame", "trace"], 40):
            if op == "step":
                p.step(float(rng.uniform(0.02, 0.2)), int(rng.integers(1, 8)))
            elif op == "publish":
                p.hand_over()
            elif op == "host":
                shifted = p.base.copy()
                shifted["cy"] += np.float32(rng.uniform(-1, 1))
                for r in (p.a, p.b):
                    r.update_spheres(shifted, refit=bool(rng.integers(2)))
            elif op == "refit":
                for r in (p.a, p.b):
                    st = r._lib.pt_refit_accel(r._ctx)
                    assert st in (0, 4)  # PT_ERR_STATE while nothing has moved
            elif op == "frame":
                assert np.array_equal(bits(p.a.render()[0]), bits(p.b.render()[0])), f"frame {frames}"
                frames += 1
            else:
                ta, ia = p.a.trace_rays(*rays)
                tb, ib = p.b.trace_rays(*rays)
                assert np.array_equal(bits(ta), bits(tb)) and np.array_equal(ia, ib)
        assert frames > 3
    finally:
        p.close()
