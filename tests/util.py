import ctypes as C
import os

import numpy as np


def context_under(dxrs, env, **kw):
    """A context created under the environment `env` (the knobs are read once, at pt_create); the environment is restored."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return dxrs.Renderer(device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rel_l2(a, b):
    """relative L2 error of the rgb channels of a against reference b"""
    a = np.asarray(a, dtype=np.float64)[..., :3]
    b = np.asarray(b, dtype=np.float64)[..., :3]
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def count_mismatch(a, b):
    """number of pixels whose rgb differs in any bit"""
    return int((bits(a)[..., :3] != bits(b)[..., :3]).any(axis=-1).sum())


def render_rested(renderer, rect=None, expect_beams=None):
    """Render the current view three times: the first frame traverses the BVH for every primary ray, the second (the view has
    rested) starts the primary-beam build, the third takes its primary candidates from the beam lists (DESIGN.md "Primary
    beams").  All three must agree bit for bit; returns the third (image, stats)."""
    first, st1 = renderer.render(rect)  # (a view that already rested under other settings may use its lists here: they do not depend on spp / bounces)
    renderer.render(rect)
    img, st = renderer.render(rect)
    if expect_beams is not None:
        assert bool(st.beams_used) == expect_beams
    assert st.rays == st1.rays
    assert np.array_equal(bits(img), bits(first)), "beam-list frame differs from the per-ray traversal frame"
    return img, st


def candidates(spheres, o, d):
    """cheap float64 prefilter so the per-ray oracle loop only visits spheres the ray passes near (margin 1e-3 r)"""
    c = np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(np.float64) - o.astype(np.float64)
    d = d.astype(np.float64); d = d / np.linalg.norm(d)  # a float32 "unit" vector is off by 6e-8: matters at b ~ 100
    b = c @ d
    dist2 = (c * c).sum(1) - b * b
    rr = spheres["r"].astype(np.float64) * 1.01 + 1e-3
    return dist2 <= rr * rr


def assert_hits_match_oracle(lib, spheres, o, d, t_gpu, id_gpu, tmin=0.0):
    """every ray's closest hit (id, and t bit for bit) is the one the CPU oracle's oracle_intersect_sphere finds, sphere by sphere in id
    order; lib = the `oracle` fixture's .lib"""
    fp = C.POINTER(C.c_float)
    spheres = np.ascontiguousarray(spheres)
    base, tmin_c = spheres.ctypes.data, C.c_float(tmin)  # (pointers made once per ray, not per sphere: layouts with thousands of candidates per ray)
    for i in range(len(t_gpu)):
        best, best_id = np.float32(np.inf), 0xFFFFFFFF
        tt = C.c_float()
        oi, di = np.ascontiguousarray(o[i]), np.ascontiguousarray(d[i])
        op, dp, best_c = oi.ctypes.data_as(fp), di.ctypes.data_as(fp), C.c_float(best)
        for sid in np.nonzero(candidates(spheres, oi, di))[0].tolist():
            if lib.oracle_intersect_sphere(op, dp, tmin_c, best_c, base + 16 * sid, C.byref(tt)):
                best, best_id = np.float32(tt.value), sid
                best_c = C.c_float(best)
        assert best_id == id_gpu[i] and (best_id == 0xFFFFFFFF or best == t_gpu[i]), (i, best_id, id_gpu[i], best, t_gpu[i])
