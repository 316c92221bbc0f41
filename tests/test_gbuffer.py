"""Row N6 -- the G-buffer pass (pt_render_gbuffer: Source/GBufferGeneration.ixx, Shaders/GBufferGeneration.hlsl; DESIGN.md spec S12).
CPU: the product's header (csrc/pt_gbuffer.h compiled as host C++ by tests/hostshim/gbuffer_host.cpp) against the float64 numpy
restatement (tests/gbuffer_reference.py) and known answers; the host mirror's camera matrices (CameraController::FillMatrices).
GPU: pt_render_gbuffer against the host-compiled header bit for bit, fed the oracle's hit of every pixel; what it must leave
untouched; its interplay with pt_render and the frame lanes."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import gbuffer_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = (1 << 13) - 1
NAMES = [name for name, _ in ref.CHANNELS]
MISS = 0xFFFFFFFF
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_gbuffer_shim())
    vp, u32 = C.c_void_p, C.c_uint32
    lib.gb_pixels.restype = None
    lib.gb_pixels.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
    lib.gb_encode_unit_vector.restype = None
    lib.gb_encode_unit_vector.argtypes = [vp, vp]
    lib.gb_srgb_lut.restype = None
    lib.gb_srgb_lut.argtypes = [vp]
    lib.gb_previous_position.restype = None
    lib.gb_previous_position.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
    return lib


def ptr(a):
    return a.ctypes.data if a is not None else None


def linear_textures(shim, ts):
    """the texture table of a TextureSet as pt_set_textures holds it: (texels float32 (T, 4), info uint32 (n, 3))"""
    if ts is None or not ts.images:
        return None, None
    lut = np.empty(256, np.float32)
    shim.gb_srgb_lut(lut.ctypes.data)
    unorm = (np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    parts, info, at = [], [], 0
    for img, fmt in ts.images:
        h, w = img.shape[:2]
        if img.dtype == np.uint8:
            x = np.empty((h * w, 4), np.float32)
            src = img.reshape(-1, 4)
            x[:, :3] = (lut if fmt == 1 else unorm)[src[:, :3]]
            x[:, 3] = unorm[src[:, 3]]
        else:
            x = img.reshape(-1, 4).astype(np.float32)
        parts.append(x)
        info.append((at, w, h))
        at += h * w
    return np.ascontiguousarray(np.concatenate(parts)), np.ascontiguousarray(np.array(info, dtype=np.uint32))


def host_pixels(shim, cam, w, h, spheres, materials, sd, px, py, t, ids, want=ALL, textures=None, prev_spheres=None, prev_rotations=None,
                rotations=None):
    """gbuffer_pixel of the host-compiled header -> (values float32 (n, 32), mask uint32 (n,)); rotations: the current rotations of an
    untextured scene (a textured one takes them from `textures`)"""
    spheres = np.ascontiguousarray(spheres)
    materials = np.ascontiguousarray(materials)
    texels, info = linear_textures(shim, textures)
    maps = rot = None
    if texels is not None:
        maps = np.zeros((len(spheres), 8), np.uint32)
        maps[:, :7] = textures.maps
        maps[:, 7] = (textures.maps != 0xFFFFFFFF).any(axis=1)
        maps = np.ascontiguousarray(maps)
        rot = np.ascontiguousarray(textures.rotations, dtype=np.float32)
    elif rotations is not None:
        rot = np.ascontiguousarray(rotations, dtype=np.float32)
    px, py = (np.ascontiguousarray(a, dtype=np.uint32) for a in (px, py))
    t, ids = np.ascontiguousarray(t, dtype=np.float32), np.ascontiguousarray(ids, dtype=np.uint32)
    ps = np.ascontiguousarray(prev_spheres) if prev_spheres is not None else None
    pr = np.ascontiguousarray(prev_rotations, dtype=np.float32) if prev_rotations is not None else None
    out = np.empty((len(px), 32), np.float32)
    mask = np.empty(len(px), np.uint32)
    shim.gb_pixels(C.byref(cam), w, h, ptr(spheres), ptr(materials), len(spheres), C.byref(sd), ptr(texels), ptr(info),
                   0 if info is None else len(info), ptr(maps), ptr(rot), ptr(ps), ptr(pr), len(px), ptr(px), ptr(py), ptr(t), ptr(ids), want,
                   out.ctypes.data, mask.ctypes.data)
    return out, mask


def oracle_hits(oracle, cam, w, h, spheres, px, py, materials=None, textures=None):
    """the oracle's primary ray and closest hit of every pixel (alpha-tested when materials are given)"""
    lib = oracle.lib
    pf = C.POINTER(C.c_float)
    spheres = np.ascontiguousarray(spheres)
    tex = keep = None
    if materials is not None:
        materials = np.ascontiguousarray(materials)
        if textures is not None:
            tex, keep = oracle._textures_struct(textures)
    t = np.empty(len(px), np.float32)
    ids = np.empty(len(px), np.uint32)
    o, d = np.empty(3, np.float32), np.empty(3, np.float32)
    tmin, tmax = C.c_float(), C.c_float()
    cache = C.c_void_p(None)
    for k, (x, y) in enumerate(zip(px, py)):
        lib.oracle_primary_ray(C.byref(cam), int(x), int(y), w, h, o.ctypes.data_as(pf), d.ctypes.data_as(pf), C.byref(tmin), C.byref(tmax))
        tt, ii = C.c_float(), C.c_uint32()
        if materials is None:
            lib.oracle_closest_hit(spheres.ctypes.data, len(spheres), o.ctypes.data_as(pf), d.ctypes.data_as(pf), tmin.value, tmax.value, 1,
                                   C.byref(cache), C.byref(tt), C.byref(ii))
        else:
            lib.oracle_closest_hit_alpha(spheres.ctypes.data, materials.ctypes.data, len(spheres), C.addressof(tex) if tex is not None else None,
                                         o.ctypes.data_as(pf), d.ctypes.data_as(pf), tmin.value, tmax.value, C.byref(tt), C.byref(ii))
        t[k], ids[k] = tt.value, ii.value
    if cache.value:
        lib.oracle_free_bvh(cache)
    del keep
    return t, ids


def grid(x0, y0, w, h):
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w]
    return xx.ravel().astype(np.uint32), yy.ravel().astype(np.uint32)


def channel(vals, name):
    a, b = ref.OFFSET[name]
    return vals[..., a:b]


# ------------------------------------------------------------------------------------------------------------------ CPU


def test_octahedral_known_answers(shim):
    def enc(v):
        v = np.ascontiguousarray(v, dtype=np.float32)
        out = np.empty(2, np.float32)
        shim.gb_encode_unit_vector(v.ctypes.data, out.ctypes.data)
        return out

    known = {(1, 0, 0): (1, 0), (-1, 0, 0): (-1, 0), (0, 1, 0): (0, 1), (0, -1, 0): (0, -1), (0, 0, 1): (0, 0), (0, 0, -1): (1, 1)}
    for v, e in known.items():
        np.testing.assert_array_equal(enc(v), np.float32(e), err_msg=str(v))
    s = 1 / math.sqrt(3)
    np.testing.assert_allclose(enc((s, s, s)), (1 / 3, 1 / 3), rtol=1e-6)
    np.testing.assert_allclose(enc((s, s, -s)), (2 / 3, 2 / 3), rtol=1e-6)
    rng = np.random.default_rng(1)
    for v in rng.normal(size=(200, 3)):
        v /= np.linalg.norm(v)
        np.testing.assert_allclose(ref.decode_unit_vector(enc(v)), v, atol=2e-6)
        np.testing.assert_allclose(enc(v), ref.encode_unit_vector(v), atol=1e-6)


def random_case(host, rng, w, h, n=12):
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    hfov = math.radians(rng.uniform(10, 150))
    pos = tuple(rng.uniform(-2, 2, 3))
    look = (pos[0] + rng.uniform(-0.3, 0.3), pos[1] + rng.uniform(-0.3, 0.3), pos[2] + 1.0)
    prev = host.camera_matrices(w, h, position=tuple(np.add(pos, rng.uniform(-0.2, 0.2, 3))), look_at=look, hfov=hfov, jitter_index=int(rng.integers(8)),
                                near_depth=0.05, far_depth=float(rng.choice([math.inf, 500.0])), reversed_depth=bool(rng.integers(2)))
    cam = host.camera_matrices(w, h, position=pos, look_at=look, hfov=hfov, jitter_index=int(rng.integers(8)), near_depth=0.05,
                               far_depth=float(rng.choice([math.inf, 500.0])), reversed_depth=bool(rng.integers(2)), previous=prev)
    fwd = np.array(list(cam.ForwardDirection))
    fwd /= np.linalg.norm(fwd)
    right = np.array(list(cam.RightDirection))
    up = np.array(list(cam.UpDirection))
    spheres = np.zeros(n, SPHERE_DTYPE)
    for i in range(n):
        c = np.array(pos) + fwd * rng.uniform(3, 12) + right * rng.uniform(-1, 1) * 0.8 * 6 + up * rng.uniform(-1, 1) * 0.8 * 6
        spheres[i] = (*c, rng.uniform(0.3, 2.0))
    mats = default_material(n)
    mats["BaseColor"][:, :3] = rng.uniform(0, 1, (n, 3))
    mats["Metallic"] = rng.choice([0.0, 0.3, 1.0], n)
    mats["Roughness"] = rng.uniform(0, 1, n)
    mats["IOR"] = rng.uniform(1.0, 2.5, n)
    mats["Transmission"] = rng.uniform(0, 1, n)
    mats["EmissiveColor"] = rng.uniform(0, 1, (n, 3)) * (rng.random((n, 1)) < 0.3)
    mats["EmissiveStrength"] = rng.uniform(0, 10, n)
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.2, 0.3, 0.4, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = int(rng.integers(2))
    prev_sph = spheres.copy()
    for f in ("cx", "cy", "cz"):
        prev_sph[f] += rng.uniform(-0.2, 0.2, n).astype(np.float32)
    prev_sph["r"] *= rng.uniform(0.9, 1.1, n).astype(np.float32)
    return cam, spheres, mats, sd, prev_sph


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def test_header_matches_numpy_restatement(host, oracle, shim):
    rng = np.random.default_rng(7)
    misses = 0
    for case in range(8):
        w, h = int(rng.integers(40, 90)), int(rng.integers(30, 70))
        cam, spheres, mats, sd, prev_sph = random_case(host, rng, w, h)
        # previous poses: centres / radii, rotations (current and previous), both, or none -- every branch of previous_position
        rot, prev_rot = random_rotations(rng, len(spheres)), random_rotations(rng, len(spheres))
        kind = case % 4
        ps = prev_sph if kind in (0, 2) else None
        pr = prev_rot if kind in (1, 2) else None
        cur = rot if kind in (1, 2) else None
        if kind != 3:
            sd.IsStatic = 0
        px, py = grid(0, 0, w, h)
        t, ids = oracle_hits(oracle, cam, w, h, spheres, px, py)
        assert (ids != MISS).sum() > 100, f"case {case}: hits"
        misses += int((ids == MISS).sum())
        got, mask = host_pixels(shim, cam, w, h, spheres, mats, sd, px, py, t, ids, prev_spheres=ps, prev_rotations=pr, rotations=cur)
        for k in range(len(px)):
            want, wmask = ref.pixel(cam, w, h, spheres, mats, sd, int(px[k]), int(py[k]), t[k], int(ids[k]), rotations=cur, prev_spheres=ps,
                                    prev_rotations=pr)
            assert mask[k] == wmask, (case, k, hex(mask[k]), hex(wmask))
            for name in NAMES:
                if not wmask & ref.BIT[name]:
                    continue
                a, b = ref.OFFSET[name]
                g, r_ = got[k, a:b].astype(np.float64), want[a:b]
                # 1e-5 relative to the channel's scale (positions: the scene's; motion vectors: a pixel)
                scale = {"Position": 20.0, "MotionVector": 1e2, "LinearDepth": max(1.0, abs(r_[0]) if np.isfinite(r_[0]) else 1.0)}.get(name, 1.0)
                if name == "MotionVector" and ids[k] == MISS:
                    scale = np.array([1e2, 1e2, 1e8])  # the depth term of a miss point 1e8 away keeps float32's absolute error at 1e8
                with np.errstate(invalid="ignore"):  # (inf - inf of a miss's Position: equal, caught by g == r_)
                    ok = (np.abs(g - r_) <= 1e-5 * np.abs(r_) + 1e-5 * np.asarray(scale)) | (g == r_)
                assert ok.all(), f"case {case} pixel ({px[k]}, {py[k]}) id {ids[k]} {name}: {g.tolist()} vs {r_.tolist()}"
    assert misses > 50


def _depth_cam(host, reversed_depth, far):
    return host.camera_matrices(64, 48, position=(0.0, 1.0, -5.0), look_at=(0.5, 1.2, 0.0), hfov=math.radians(70), jitter=False,
                                near_depth=0.25, far_depth=far, reversed_depth=reversed_depth)


@pytest.mark.parametrize("reversed_depth", [False, True])
@pytest.mark.parametrize("far", [100.0, math.inf])
def test_normalized_depth_at_the_planes(host, reversed_depth, far):
    """the projection of FillMatrices uses the camera's own NearDepth / FarDepth (S12: the SetLens order of Camera.ixx is not kept)"""
    cam = _depth_cam(host, reversed_depth, far)
    assert cam.NearDepth == np.float32(0.25) and (cam.FarDepth == far or (math.isinf(far) and math.isinf(cam.FarDepth)))
    pos, f = np.array(list(cam.Position)), np.array(list(cam.ForwardDirection))
    f /= np.linalg.norm(f)
    W2P = list(cam.Matrices[5])
    near_z = (lambda c: c[2] / c[3])(ref.project(W2P, pos + 0.25 * f))
    assert abs(near_z - (1.0 if reversed_depth else 0.0)) < 1e-5
    far_pt = pos + (far if math.isfinite(far) else 1e12) * f
    far_z = (lambda c: c[2] / c[3])(ref.project(W2P, far_pt))
    assert abs(far_z - (0.0 if reversed_depth else 1.0)) < 1e-5
    mid = (lambda c: c[2] / c[3])(ref.project(W2P, pos + 3.0 * f))
    assert 0.0 < mid < 1.0


def test_camera_matrices_reproduce_the_primary_rays(host, oracle):
    rng = np.random.default_rng(11)
    pf = C.POINTER(C.c_float)
    for _ in range(40):
        w, h = int(rng.integers(16, 2000)), int(rng.integers(16, 1200))
        hfov = math.radians(rng.uniform(10, 150))
        cam = host.camera_matrices(w, h, position=tuple(rng.uniform(-5, 5, 3)), look_at=tuple(rng.uniform(-20, 20, 3)), hfov=hfov,
                                   jitter_index=int(rng.integers(8)), near_depth=float(rng.uniform(1e-3, 1)), far_depth=float(rng.choice([math.inf, 1e3])),
                                   reversed_depth=bool(rng.integers(2)))
        W2P = list(cam.Matrices[5])
        fwd = np.array(list(cam.ForwardDirection), dtype=np.float64)
        fwd /= np.linalg.norm(fwd)
        o, d = np.empty(3, np.float32), np.empty(3, np.float32)
        tmin, tmax = C.c_float(), C.c_float()
        for _ in range(20):
            x, y = int(rng.integers(w)), int(rng.integers(h))
            oracle.lib.oracle_primary_ray(C.byref(cam), x, y, w, h, o.ctypes.data_as(pf), d.ctypes.data_as(pf), C.byref(tmin), C.byref(tmax))
            o64, d64, want = ref.camera_ray(cam, x, y, w, h)  # the same ray in float64 (the oracle's, up to float32 rounding)
            np.testing.assert_allclose(d64, d, atol=1e-6)
            X = o64 + rng.uniform(1, 50) * d64
            uv = ref.screen_uv(W2P, X)
            # 1e-4 px at 1000 px across; float32 matrix entries limit it in proportion to the image size and the x scale
            # (one float32 ulp of a UV is 1.2e-4 px at 2048 px across)
            np.testing.assert_allclose(uv * (w, h), want * (w, h), atol=1e-4 * max(1.0, max(w, h) / 1000) * max(1.0, 1 / math.tan(hfov / 2)))
            assert abs(ref.project(W2P, X)[3] - (X - o) @ fwd) < 1e-4 * np.linalg.norm(X - o)
        m = [ref.mat(list(cam.Matrices[k])) for k in range(8)]
        W2V = np.linalg.inv(m[7])
        np.testing.assert_allclose(m[7] @ np.linalg.inv(m[7]), np.eye(4), atol=1e-5)
        np.testing.assert_allclose(ref.mat(list(cam.Matrices[5])), W2V @ np.linalg.inv(m[6]), rtol=1e-4, atol=1e-4 * np.abs(m[5]).max())
        np.testing.assert_allclose(m[6] @ np.linalg.inv(m[6]), np.eye(4), atol=1e-5)
        np.testing.assert_allclose(m[0] @ m[4], np.eye(4), atol=1e-4)  # PreviousWorldToView . PreviousViewToWorld
        np.testing.assert_allclose(m[1] @ m[3], np.eye(4), atol=1e-4)  # PreviousViewToProjection . PreviousProjectionToView


def _one_sphere_scene(dxrs, static=1):
    from dxrs_amd.types import SPHERE_DTYPE, PtSceneData, default_material
    spheres = np.zeros(1, SPHERE_DTYPE)
    spheres[0] = (0.0, 0.0, 0.0, 1.0)
    mats = default_material(1)
    mats["BaseColor"][0, :3] = (0.5, 0.25, 0.125)
    sd = PtSceneData()
    sd.EnvironmentLightColor[:] = (0.25, 0.5, 0.75, 1.0)
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    sd.IsStatic = static
    return spheres, mats, sd


def test_miss_conventions_and_resting_view(dxrs, host, oracle, shim):
    spheres, mats, sd = _one_sphere_scene(dxrs)
    w, h = 48, 32
    for reversed_depth in (False, True):
        cam = host.camera_matrices(w, h, position=(0.0, 0.0, -4.0), hfov=math.radians(60), reversed_depth=reversed_depth)
        px, py = grid(0, 0, w, h)
        t, ids = oracle_hits(oracle, cam, w, h, spheres, px, py)
        assert 0 < (ids == 0).sum() < len(ids)
        got, mask = host_pixels(shim, cam, w, h, spheres, mats, sd, px, py, t, ids)
        miss, hit = ids == MISS, ids == 0
        want_miss = ref.BIT["Position"] | ref.BIT["LinearDepth"] | ref.BIT["NormalizedDepth"] | ref.BIT["MotionVector"] | ref.BIT["Radiance"]
        assert (mask[miss] == want_miss).all() and (mask[hit] == ALL).all()
        assert np.isinf(channel(got[miss], "Position")).all() and np.isinf(channel(got[miss], "LinearDepth")).all()
        assert (channel(got[miss], "NormalizedDepth") == (0.0 if reversed_depth else 1.0)).all()
        assert (channel(got[miss], "Radiance") == np.float32([0.25, 0.5, 0.75])).all()
        # a static scene seen by a resting camera does not move
        np.testing.assert_allclose(channel(got, "MotionVector")[..., :2], 0.0, atol=2e-3)
        np.testing.assert_allclose(channel(got[hit], "MotionVector")[..., 2], 0.0, atol=1e-5 * 4)


def test_camera_translation_gives_the_analytic_shift(dxrs, host, oracle, shim):
    spheres, mats, sd = _one_sphere_scene(dxrs)
    w, h, hfov, delta = 64, 48, math.radians(75), 0.125
    prev = host.camera_matrices(w, h, position=(0.0, 0.0, -4.0), hfov=hfov, jitter=False)
    cam = host.camera_matrices(w, h, position=(delta, 0.0, -4.0), hfov=hfov, jitter=False, previous=prev)
    px, py = grid(0, 0, w, h)
    t, ids = oracle_hits(oracle, cam, w, h, spheres, px, py)
    got, mask = host_pixels(shim, cam, w, h, spheres, mats, sd, px, py, t, ids)
    hit = ids == 0
    z = channel(got[hit], "LinearDepth")[:, 0].astype(np.float64)
    mv = channel(got[hit], "MotionVector").astype(np.float64)
    xs = 1 / math.tan(hfov / 2)
    np.testing.assert_allclose(mv[:, 0], delta * xs * w / (2 * z), rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(mv[:, 1], 0.0, atol=2e-3)
    np.testing.assert_allclose(mv[:, 2], 0.0, atol=1e-5 * 5)


def test_previous_position_keeps_the_texture_coordinate(shim):
    """the header's Pprev of a point under a moved, resized and turned previous pose is the point with the same sphere UV (spec S6,
    float64 here) -- the convention of hit_uv_rot; static scenes and scenes without a previous pose do not move"""
    rng = np.random.default_rng(3)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)

    def prev_pos(s, q, ps, qp, P, N, static=0):
        out = np.empty(3, np.float32)
        shim.gb_previous_position(ptr(s), ptr(q), ptr(ps), ptr(qp), static, ptr(P), ptr(N), out.ctypes.data)
        return out

    for _ in range(200):
        s = f([*rng.uniform(-5, 5, 3), rng.uniform(0.5, 3)])
        ps = f([*rng.uniform(-5, 5, 3), rng.uniform(0.5, 3)])
        q, qp = random_rotations(rng, 2)
        N = rng.normal(size=3)
        N = f(N / np.linalg.norm(N))
        P = f(s[:3].astype(np.float64) + float(s[3]) * N.astype(np.float64))
        Pp = prev_pos(s, f(q), ps, f(qp), P, N).astype(np.float64)
        Np = (Pp - ps[:3]) / float(ps[3])
        assert abs(np.linalg.norm(Np) - 1) < 1e-5
        uv_now = ref.sphere_uv(ref.quat_rotate(ref.conj(q.astype(np.float64)), N.astype(np.float64)))
        uv_then = ref.sphere_uv(ref.quat_rotate(ref.conj(qp.astype(np.float64)), Np))
        d = np.abs(uv_then - uv_now)
        d[0] = min(d[0], 1 - d[0])  # u wraps at the seam
        assert (d < 1e-5).all(), (uv_then, uv_now)
        # only moved: the same normal on the previous sphere; no rotations in the scene: q = identity
        np.testing.assert_allclose(prev_pos(s, None, ps, None, P, N), ps[:3] + ps[3] * N, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(prev_pos(s, None, None, f(qp), P, N), s[:3] + s[3] * f(ref.quat_rotate(qp.astype(np.float64), N)), rtol=1e-5, atol=1e-5)
        # nothing moved, or a static scene: P itself, exactly
        assert (prev_pos(s, f(q), None, None, P, N) == P).all()
        assert (prev_pos(s, f(q), ps, f(qp), P, N, static=1) == P).all()


def test_abi_validation_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    from dxrs_amd.types import PtGBuffer
    gb = PtGBuffer()
    assert lib.pt_render_gbuffer(None, None, None, None, None) == 1
    assert lib.pt_render_gbuffer(None, None, C.byref(gb), None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU


def bits_equal(got, want, what=""):
    """bit-exact equality, NaN compared by mask"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ at {np.argwhere(gn != wn)[:5].tolist()}"
    g, wb = got[~gn].view(np.uint32), want[~wn].view(np.uint32)
    bad = np.nonzero(g != wb)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:5].tolist()}: {got[~gn][bad[:5]].tolist()} vs {want[~wn][bad[:5]].tolist()}"


def gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, rect=None, textures=None, alpha=False, prev_spheres=None, prev_rotations=None,
                hit_spheres=None, channels="all"):
    """pt_render_gbuffer (sentinel-filled buffers) against the host header fed the oracle's hits: every written word bit for bit,
    every other one untouched"""
    rx, ry, rw, rh = rect if rect is not None else (0, 0, w, h)
    px, py = grid(rx, ry, rw, rh)
    hs = spheres if hit_spheres is None else hit_spheres
    t, ids = oracle_hits(oracle, cam, w, h, hs, px, py, materials=mats if alpha else None, textures=textures if alpha else None)
    names = NAMES if channels == "all" else list(channels)
    want_bits = sum(ref.BIT[n] for n in names)
    got = renderer.render_gbuffer(names, rect=rect, previous_spheres=prev_spheres, previous_rotations=prev_rotations, fill=SENTINEL)
    want, mask = host_pixels(shim, cam, w, h, hs, mats, sd, px, py, t, ids, want_bits, textures, prev_spheres, prev_rotations)
    for name in names:
        g = got[name].reshape(rw * rh, -1)
        written = (mask & ref.BIT[name]) != 0
        bits_equal(g[written], channel(want, name)[written], name)
        assert (g[~written] == SENTINEL).all(), f"{name}: {int((g[~written] != SENTINEL).any(axis=1).sum())} unwritten pixels changed"
    return got, ids, mask


def setup(renderer, dxrs, spheres, mats, sd, cam, w, h, textures=None, bounces=8, spp=1):
    renderer.set_scene(spheres, mats, sd)
    if textures is not None:
        renderer.set_textures(textures)
    renderer.set_camera(cam)
    renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=0, bounces=bounces, spp=spp))


@pytest.mark.gpu
def test_gpu_c1_whole_frame(dxrs, host, oracle, renderer, shim):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    w, h = 256, 256
    cam = host.camera_matrices(w, h, jitter_index=0)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h, bounces=4)
    _, ids, _ = gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd)
    assert (ids != MISS).any() and (ids == MISS).any()


@pytest.mark.gpu
def test_gpu_c2_crop_and_pixels_outside_the_rect(dxrs, host, oracle, renderer, shim):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 1920, 1080
    cam = host.camera_matrices(w, h, jitter_index=3)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, rect=(928, 500, 64, 32))
    gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, rect=(1901, 1070, 19, 10))  # partial blocks at the corner
    # a rect's buffers hold rect.w * rect.h pixels: a guard band behind them stays untouched
    import torch
    buf = torch.full((32 * 64 + 256, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.render_gbuffer_device({"Position": buf.data_ptr()}, rect=(928, 500, 64, 32))
    renderer.synchronize()
    b = buf.cpu().numpy()
    assert not (b[:32 * 64] == SENTINEL).any() and (b[32 * 64:] == SENTINEL).all()


@pytest.mark.gpu
def test_gpu_each_output_alone(dxrs, host, oracle, renderer, shim):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    mats = mats.copy()
    mats["Metallic"][::2] = 1.0  # Transmission must stay untouched on these
    w, h = 320, 180
    cam = host.camera_matrices(w, h, position=(0.0, 2.0, -15.0), jitter_index=1)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    for name in NAMES:
        _, ids, mask = gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, channels=[name])
    hit = ids != MISS
    assert (hit & (mats["Metallic"][np.minimum(ids, len(mats) - 1)] >= 1)).any(), "some hits are fully metallic"
    assert ((mask & ref.BIT["Transmission"]) == 0)[hit & (mats["Metallic"][np.minimum(ids, len(mats) - 1)] >= 1)].all()


@pytest.mark.gpu
def test_gpu_alpha_scene(dxrs, host, oracle, renderer, shim):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    mats = mats.copy()
    mats["AlphaMode"][1::3] = 1          # Mask
    mats["BaseColor"][1::3, 3] = 0.25     # below the cutoff: the sphere does not exist for rays
    mats["AlphaMode"][2::3] = 2          # Blend, above the cutoff: visible
    w, h = 256, 256
    cam = host.camera_matrices(w, h, jitter_index=2)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h, bounces=4)
    gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, alpha=True)


@pytest.mark.gpu
def test_gpu_textured_demo_with_environment_map(dxrs, host, oracle, renderer, shim):
    spheres, mats, _ = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    ts, sd = host.demo_textures(seed=0, time=0.0, environment_map=True, return_scene_data=True)
    w, h = 1920, 1080
    cam = host.camera_matrices(w, h, jitter_index=5)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h, textures=ts)
    for rect in ((560, 360, 160, 96), (0, 0, 96, 64)):  # the textured heroes; sky (misses: the lat-long map)
        _, ids, _ = gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, rect=rect, textures=ts)
    assert (ids == MISS).any()


@pytest.mark.gpu
def test_gpu_animated_pair_with_previous_poses(dxrs, host, oracle, renderer, shim):
    spheres, mats, _ = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    t0, t1 = 1.0, 1.0 + 1 / 60
    ts0 = host.demo_textures(seed=0, time=t0)
    ts1, sd = host.demo_textures(seed=0, time=t1, return_scene_data=True)
    s0, s1 = host.scene_at_time(0, t0), host.scene_at_time(0, t1)
    sd.IsStatic = 0
    w, h = 1920, 1080
    prev_cam = host.camera_matrices(w, h, jitter_index=0)
    cam = host.camera_matrices(w, h, jitter_index=1, previous=prev_cam)
    setup(renderer, dxrs, s0, mats, sd, cam, w, h, textures=ts1)
    renderer.update_spheres(s1)
    got, ids, mask = gpu_vs_host(renderer, shim, oracle, cam, w, h, s1, mats, sd, rect=(560, 360, 160, 96), textures=ts1,
                                 prev_spheres=s0, prev_rotations=ts0.rotations)
    mv = got["MotionVector"].reshape(-1, 3)[ids != MISS]
    assert np.abs(mv[:, :2]).max() > 1e-3, "the spheres moved"
    # IsStatic: the previous poses are ignored
    sd.IsStatic = 1
    renderer.set_scene(s1, mats, sd)
    renderer.set_textures(ts1)
    gpu_vs_host(renderer, shim, oracle, cam, w, h, s1, mats, sd, rect=(560, 360, 64, 32), textures=ts1, prev_spheres=s0, prev_rotations=ts0.rotations)


@pytest.mark.gpu
def test_gpu_moved_and_turned_camera(dxrs, host, oracle, renderer, shim):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 640, 360
    prev = host.camera_matrices(w, h, position=(0.3, 0.1, -15.0), look_at=(0.0, 0.0, 0.0), hfov=math.radians(80), jitter_index=0)
    cam = host.camera_matrices(w, h, position=(0.0, 0.0, -14.5), look_at=(0.5, 0.2, 0.0), hfov=math.radians(80), jitter_index=1, previous=prev)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h)
    got, ids, _ = gpu_vs_host(renderer, shim, oracle, cam, w, h, spheres, mats, sd, rect=(200, 120, 128, 96))
    assert np.abs(got["MotionVector"][..., :2]).max() > 0.5


@pytest.mark.gpu
def test_gpu_large_scene_global_walk(dxrs, host, oracle, shim):
    spheres, mats, sd = host.scene(dxrs.host.SCENE_PROCEDURAL, seed=0, count=100000)
    w, h = 512, 512
    cam = host.camera_matrices(w, h, jitter_index=4)
    r = dxrs.Renderer(device=0)
    try:
        setup(r, dxrs, spheres, mats, sd, cam, w, h)
        assert not r.accel.lds_resident
        gpu_vs_host(r, shim, oracle, cam, w, h, spheres, mats, sd, rect=(192, 192, 96, 96))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("textured", [False, True])
def test_gpu_radiance_seeds_a_zero_bounce_frame(dxrs, host, renderer, textured):
    """Raytracing.hlsl:119,197,243: every sample starts from the G-buffer's radiance; with no bounce and no DI it is the frame"""
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    ts = None
    if textured:
        ts, sd = host.demo_textures(seed=0, time=0.0, environment_map=True, return_scene_data=True)
    w, h = 480, 270
    cam = host.camera_matrices(w, h, jitter_index=2)
    setup(renderer, dxrs, spheres, mats, sd, cam, w, h, textures=ts, bounces=0, spp=1)
    rad = renderer.render_gbuffer(["Radiance"])["Radiance"]
    img, _ = renderer.render(want_stats=False)
    bits_equal(img.reshape(h, w, 4)[..., :3], rad, "Radiance vs pt_render")


@pytest.mark.gpu
def test_gpu_frames_in_flight_unchanged_by_interleaved_gbuffers(dxrs, host, renderer):
    """three lanes, a G-buffer call before every frame: the frames and the totals are those of the same frames without them, and each
    G-buffer is that of its own frame -- with a G-buffer set per lane (ordered by the frame markers) and with buffers shared between
    lanes (ordered after everything the caller has queued)"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 640, 360
    frames = 9

    def cam_of(f):
        return host.camera_matrices(w, h, position=(0.0, 0.0, -15.0 + 0.05 * f), jitter_index=f)

    def run(mode):
        r = dxrs.Renderer(device=0, frames_in_flight=3)
        try:
            r.set_scene(spheres, mats, sd)
            outs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            gbs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            nrs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            res, gres = [], []
            for f in range(frames):
                r.set_camera(cam_of(f))
                r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
                if mode == "per_lane":
                    r.render_gbuffer_device({"Position": gbs[f % 3].data_ptr(), "NormalRoughness": nrs[f % 3].data_ptr()})
                elif mode == "shared":
                    r.render_gbuffer_device({"Position": gbs[f % 3].data_ptr(), "NormalRoughness": gbs[(f + 1) % 3].data_ptr()})
                r.render_device(outs[f % 3].data_ptr())
                if f % 3 == 2:
                    r.synchronize()
                    res += [o.cpu().numpy().copy() for o in outs]
                    gres += [(g.cpu().numpy().copy(), n.cpu().numpy().copy()) for g, n in zip(gbs, nrs)]
            r.synchronize()
            return res, r.totals(), gres
        finally:
            r.close()

    a, ta, _ = run("none")
    for mode in ("per_lane", "shared"):
        b, tb, gres = run(mode)
        for k, (x, y) in enumerate(zip(a, b)):
            bits_equal(y, x, f"{mode}: frame {k}")
        for f in ("rays", "paths", "pixels", "bytes_algorithmic"):
            assert getattr(ta, f) == getattr(tb, f), (mode, f)
        if mode == "per_lane":
            renderer.set_scene(spheres, mats, sd)
            for f in range(frames):
                renderer.set_camera(cam_of(f))
                renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
                want = renderer.render_gbuffer(["Position", "NormalRoughness"])
                bits_equal(gres[f][0], want["Position"], f"G-buffer of frame {f}: Position")
                written = ~np.isnan(want["NormalRoughness"])  # (a miss leaves NormalRoughness as it was)
                bits_equal(gres[f][1][written], want["NormalRoughness"][written], f"G-buffer of frame {f}: NormalRoughness")


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, host, renderer):
    from dxrs_amd.types import PtGBuffer, PtRect, SPHERE_DTYPE
    lib = renderer._lib
    ctx = renderer._ctx
    import torch
    buf = torch.zeros(64 * 64 * 4 + 4, dtype=torch.float32, device="cuda")
    fresh = dxrs.Renderer(device=0)
    try:
        gb = PtGBuffer(Position=buf.data_ptr())
        assert lib.pt_render_gbuffer(fresh._ctx, None, C.byref(gb), None, None) == 4  # no scene yet
    finally:
        fresh.close()
    spheres, mats, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    setup(renderer, dxrs, spheres, mats, sd, host.camera_matrices(64, 64), 64, 64)
    assert lib.pt_render_gbuffer(ctx, None, C.byref(PtGBuffer()), None, None) == 1  # nothing requested
    assert lib.pt_render_gbuffer(ctx, None, C.byref(PtGBuffer(Position=buf.data_ptr() + 4)), None, None) == 1  # misaligned float4
    gb = PtGBuffer(Position=buf.data_ptr())
    assert lib.pt_render_gbuffer(ctx, C.byref(PtRect(60, 0, 8, 8)), C.byref(gb), None, None) == 1
    assert lib.pt_render_gbuffer(ctx, C.byref(PtRect(0, 0, 0, 8)), C.byref(gb), None, None) == 1
    sd.IsStatic = 0
    renderer.set_scene(spheres, mats, sd)
    bad = spheres.copy()
    bad["r"][3] = 0.0
    assert lib.pt_render_gbuffer(ctx, None, C.byref(gb), bad.ctypes.data, None) == 1
    bad = spheres.copy()
    bad["cx"][0] = np.nan
    assert lib.pt_render_gbuffer(ctx, None, C.byref(gb), bad.ctypes.data, None) == 1
    rot = np.tile(np.float32([0, 0, 0, 1]), (len(spheres), 1))
    rot[2, 1] = np.inf
    assert lib.pt_render_gbuffer(ctx, None, C.byref(gb), None, rot.ctypes.data) == 1
    sd.EnvironmentLightTextureDescriptor = 7  # no such texture
    renderer.set_scene(spheres, mats, sd)
    assert lib.pt_render_gbuffer(ctx, None, C.byref(gb), None, None) == 4
    sd.EnvironmentLightTextureDescriptor = 0xFFFFFFFF
    renderer.set_scene(spheres, mats, sd)
    assert lib.pt_render_gbuffer(ctx, None, C.byref(gb), None, None) == 0  # the context still works
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, oracle, shim, tmp_path):
    """GBufferGeneration (host/GBufferGeneration.hpp) bound to pt_render_gbuffer from C++: the G-buffer of the demo scene equals the
    host-compiled header's, bit for bit"""
    import subprocess
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_gbuffer")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_gbuffer.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 160, 90
    outp = str(tmp_path / "gbuffer.f32")
    res = subprocess.run([exe, str(w), str(h), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(outp, dtype=np.float32).reshape(h * w, 32)
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    cam = host.camera_matrices(w, h, jitter=False)
    px, py = grid(0, 0, w, h)
    t, ids = oracle_hits(oracle, cam, w, h, spheres, px, py)
    want, mask = host_pixels(shim, cam, w, h, spheres, mats, sd, px, py, t, ids)
    for name in NAMES:
        written = (mask & ref.BIT[name]) != 0
        bits_equal(channel(got, name)[written], channel(want, name)[written], name)
