"""CPU: the reflection-beam header (csrc/pt_region.h, compiled as host C++ by tests/hostshim/region_host.cpp) against float64 brute force.
- the box test is conservative: rays sampled inside a region never pass a box it rejected;
- the run-time test accepts only rays that lie in the region its list is built for (origin in O, direction within theta of the axis);
- records built from pyramids over spheres accept the rays that start on the sphere and reflect within the GGX cap.
The device variant (atan2f, asinf, acosf, cosf of the device library) runs these same test bodies in test_gpu_leaf_edges.py."""
import ctypes as C

import numpy as np
import pytest

GGX_CAP = 2e-3  # kReflGgxCap


def load_shim():
    """region_host.cpp as __graft_entry__.build_region_shim() compiles it, with its signatures declared"""
    import __graft_entry__ as g

    lib = C.CDLL(g.build_region_shim())
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lib.rg_make.argtypes = [f32p, f32p, f32p, C.c_float, f32p]
    lib.rg_meets_boxes.argtypes = [f32p, C.c_uint32, f32p, u8p]
    lib.rg_contains.argtypes = [f32p, C.c_uint32, f32p, u8p]
    lib.rg_from_rays.argtypes = [f32p, f32p, f32p, C.c_float, f32p]
    lib.rg_from_rays.restype = C.c_int
    lib.rg_lane.argtypes = [f32p, f32p, f32p, C.c_float, C.c_float, C.c_float, f32p, f32p]
    lib.rg_lane.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def fp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_region(lib, lo, hi, axis, theta):
    g = np.zeros(11, np.float32)
    lib.rg_make(fp(lo), fp(hi), fp(axis), C.c_float(theta), fp(g))
    return g


def meets(lib, g, boxes):
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    out = np.zeros(len(boxes), np.uint8)
    lib.rg_meets_boxes(fp(g), len(boxes), fp(boxes), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out.astype(bool)


def contains(lib, g, o, d):
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=np.float32)
    out = np.zeros(len(rays), np.uint8)
    lib.rg_contains(fp(g), len(rays), fp(rays), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out.astype(bool)


def cone_dirs(rng, axis, theta, n, edge=False):
    """n unit directions within theta of axis (float64); edge: on the cone's boundary."""
    axis = unit(axis)
    t = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    t = unit(t)
    b = np.cross(axis, t)
    ang = np.full(n, theta) if edge else theta * np.sqrt(rng.random(n))
    phi = rng.uniform(0, 2 * np.pi, n)
    return (np.cos(ang)[:, None] * axis + np.sin(ang)[:, None] * (np.cos(phi)[:, None] * t + np.sin(phi)[:, None] * b))


def slab_hits(o, d, lo, hi):
    """float64: does the ray o + t d, t >= 0, meet the box?"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
    tn = np.max(np.minimum(t0, t1), axis=-1)
    tf = np.min(np.maximum(t0, t1), axis=-1)
    return np.maximum(tn, 0.0) <= tf


def random_region(rng):
    c = rng.uniform(-30, 30, 3)
    h = rng.uniform(1e-3, 2.0, 3) * rng.choice([1.0, 0.01])
    axis = unit(rng.normal(size=3))
    theta = float(np.exp(rng.uniform(np.log(5e-3), np.log(0.4))))
    return c - h, c + h, axis, theta


def test_rejected_boxes_are_never_passed(shim):
    rng = np.random.default_rng(1)
    n_rejected = 0
    for _ in range(60):
        lo, hi, axis, theta = random_region(rng)
        g = make_region(shim, lo, hi, axis, theta)
        c = 0.5 * (lo + hi)
        # boxes scattered around the region's cone, some near its boundary
        dist = np.exp(rng.uniform(np.log(0.5), np.log(80.0), 400))
        dirs = cone_dirs(rng, axis, min(3.0 * theta + 0.05, 3.0), 400)
        centres = c + dist[:, None] * dirs
        ext = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), (400, 3)))
        boxes = np.concatenate([centres - ext, centres + ext], axis=1).astype(np.float32)
        ok = meets(shim, g, boxes)
        rej = np.flatnonzero(~ok)
        n_rejected += len(rej)
        if not len(rej):
            continue
        m = 3000
        o = lo + rng.random((m, 3)) * (hi - lo)
        o[: m // 4] = np.where(rng.random((m // 4, 3)) < 0.5, lo, hi)  # corners of O
        d = np.concatenate([cone_dirs(rng, axis, theta, m // 2), cone_dirs(rng, axis, theta, m - m // 2, edge=True)])
        for k in rej:
            blo, bhi = boxes[k, :3].astype(np.float64), boxes[k, 3:].astype(np.float64)
            assert not slab_hits(o, d, blo, bhi).any(), f"a ray of the region passes rejected box {k}"
    assert n_rejected > 1000  # the test culls


def test_accepted_rays_lie_in_the_region(shim):
    rng = np.random.default_rng(2)
    n_acc = 0
    for _ in range(40):
        lo, hi, axis, theta = random_region(rng)
        g = make_region(shim, lo, hi, axis, theta)
        axis32 = g[6:9].astype(np.float64)
        m = 20000
        o = lo - 0.01 * (hi - lo) + rng.random((m, 3)) * 1.02 * (hi - lo)
        ang = theta * rng.uniform(0.98, 1.02, m)
        # directions at angles around theta (not normalised exactly: the kernels' |d| is 1 to rounding)
        t = unit(np.cross(axis, rng.normal(size=(m, 3))))
        d = np.cos(ang)[:, None] * unit(axis) + np.sin(ang)[:, None] * t
        d32 = d.astype(np.float32)
        o32 = o.astype(np.float32)
        acc = contains(shim, g, o32, d32)
        n_acc += acc.sum()
        oo, dd = o32[acc].astype(np.float64), d32[acc].astype(np.float64)
        assert ((oo >= g[0:3]) & (oo <= g[3:6])).all()
        cosang = (dd @ axis32) / (np.linalg.norm(dd, axis=1) * np.linalg.norm(axis32))
        assert (np.arccos(np.clip(cosang, -1, 1)) <= g[9]).all()  # the half-angle the candidate list is built for
        assert g[9] <= theta + 0.01
    assert n_acc > 1000


def pyramid(rng):
    """A random small pyramid from a camera outside a random sphere towards a visible point of it: (cam, dirs[5], C, r)."""
    C = rng.uniform(-20, 20, 3)
    r = float(np.exp(rng.uniform(np.log(0.5), np.log(500.0))))
    cam = C + unit(rng.normal(size=3)) * r * (1.0 + np.exp(rng.uniform(np.log(1e-3), np.log(5.0))))
    target = C + unit(rng.normal(size=3)) * r
    if np.dot(target - C, cam - C) < 0:
        target = 2 * C - target
    fwd = unit(target - cam)
    right = unit(np.cross(fwd, rng.normal(size=3)))
    up = np.cross(right, fwd)
    a = float(np.exp(rng.uniform(np.log(2e-4), np.log(2e-2))))
    corners = [unit(fwd + a * (sx * right + sy * up)) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    return cam, np.array(corners + [fwd]), C, r


def test_records_accept_mirror_bounces(shim):
    rng = np.random.default_rng(3)
    built = 0
    for _ in range(400):
        cam, dirs, Cs, r = pyramid(rng)
        g = np.zeros(11, np.float32)
        if not shim.rg_from_rays(fp(cam), fp(dirs), fp(Cs), C.c_float(r), fp(g)):
            continue
        built += 1
        # rays inside the pyramid (bilinear in its corners), each reflected off the sphere about a half-vector tilted by <= the cap
        for _ in range(64):
            u, v = rng.random(2)
            d = unit((1 - v) * ((1 - u) * dirs[0] + u * dirs[1]) + v * ((1 - u) * dirs[3] + u * dirs[2]))
            o, L = np.zeros(3, np.float32), np.zeros(3, np.float32)
            tilt = GGX_CAP * rng.random() ** 0.5
            if not shim.rg_lane(fp(cam), fp(d), fp(Cs), C.c_float(r), C.c_float(tilt), C.c_float(rng.uniform(0, 2 * np.pi)),
                                fp(o), fp(L)):
                continue
            assert contains(shim, g, o[None], L[None])[0], "a mirror bounce of the block falls outside its region"
    assert built > 100
