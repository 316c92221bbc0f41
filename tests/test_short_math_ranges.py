"""CPU: the operands that reach the call sites of pt_math.h's short exact forms stay inside the forms' contracts.
tests/hostshim/short_math_ranges_host.cpp compiles pt_math.h and pt_bsdf.h as host C++ with PT_RANGED defined: every operand of a switched site
is recorded (smallest and largest finite non-zero magnitude per site) before the -- on the host, plain -- operator sees it.  The bounce loop's
shading step (surf_init_unit, lobe_weights, bsdf_sample, bsdf_pdf_eval; every lobe forced in turn) and cosine_ray are driven with random and
adversarial inputs: roughness 0, 2e-3, 1 and far beyond 1, grazing V, a V that is not unit, N.z = +-1 and -0.0, u at both ends of (0, 1], index of
refraction at and around 1.  This backs the proofs written at the sites; it does not replace them.
primary_ray is not driven: none of its operations is switched (pt_set_camera accepts any camera, so its field of view bounds nothing)."""
import ctypes as C

import numpy as np
import pytest

# pt::RangedSite, in order, with the contract of the form the site uses
SQRT, RCP, HALF = (2.0 ** -96, np.inf), (2.0 ** -126, 2.0 ** 126), (2.0 ** -126, 2.0 ** 125)
SITES = [("basis_rcp", RCP), ("cosine_sin", SQRT), ("vndf_disk", SQRT), ("vndf_nh", SQRT), ("vndf_pdf_root", SQRT),
         ("vndf_pdf_half", HALF), ("geom_root_l", SQRT), ("geom_root_v", SQRT), ("fresnel_cos", SQRT), ("refract_root", SQRT)]
# what the proofs at the sites promise beyond the contract (a tighter interval per site; the contract is the assertion that matters)
PROVEN = {"basis_rcp": (1.0, 2.0 ** 12 + 1), "cosine_sin": (2.0 ** -24, 1.0), "vndf_disk": (2.0 ** -24, 1.0),
          "vndf_nh": (9.9e-15, np.inf), "vndf_pdf_root": (2.0 ** -85, np.inf), "vndf_pdf_half": (2.0 ** -18, 2.0 ** 65),
          "geom_root_l": (2.0 ** -85, 1.0), "geom_root_v": (2.0 ** -85, 1.0), "fresnel_cos": (2.0 ** -24, 1.0), "refract_root": (2.0 ** -24, np.inf)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    so = C.CDLL(g.build_short_math_ranges_shim())
    so.smr_site_count.restype = C.c_int
    so.smr_steps.argtypes = [C.c_uint32, C.c_void_p]
    so.smr_cosine.argtypes = [C.c_uint32, C.c_void_p]
    so.smr_get.argtypes = [C.c_void_p] * 4
    assert so.smr_site_count() == len(SITES)
    return so


def records(lib):
    n = len(SITES)
    mn, mx = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    seen, special = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    lib.smr_get(mn.ctypes.data, mx.ctypes.data, seen.ctypes.data, special.ctypes.data)
    return mn, mx, seen, special


def check(lib, need_seen):
    mn, mx, seen, special = records(lib)
    for k, (name, (lo, hi)) in enumerate(SITES):
        print(f"{name}: {int(seen[k])} operands ({int(special[k])} zero / inf / NaN), finite non-zero magnitudes in [{mn[k]:.9g}, {mx[k]:.9g}]")
    for k, (name, (lo, hi)) in enumerate(SITES):
        if name in need_seen:
            assert seen[k] > special[k], f"{name}: the drive reached the site with no finite non-zero operand"
        if seen[k] > special[k]:
            assert lo <= mn[k] and mx[k] <= hi, f"{name}: magnitudes [{mn[k]!r}, {mx[k]!r}] leave the contract [{lo!r}, {hi!r}]"
            plo, phi = PROVEN[name]
            assert plo <= mn[k] and mx[k] <= phi, f"{name}: magnitudes [{mn[k]!r}, {mx[k]!r}] leave what the site's proof states, [{plo!r}, {phi!r}]"


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rows(base, metallic, roughness, ior, transmission, front, a, V, rnd):
    n = len(rnd)
    r = np.zeros((n, 18), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4], r[:, 5], r[:, 6], r[:, 7] = base, metallic, roughness, ior, transmission, front
    r[:, 8:11], r[:, 11:14], r[:, 14:18] = a, V, rnd
    return np.ascontiguousarray(r)


def rng_floats(rng, shape):
    """rng_float()'s values: multiples of 2^-23 in (0, 1]"""
    return ((rng.integers(0, 1 << 23, shape) + 1).astype(np.float64) * 2.0 ** -23).astype(np.float32)


def test_random_shading_steps_stay_inside_the_contracts(lib):
    rng = np.random.default_rng(2025)
    n = 200_000
    lib.smr_reset()
    r = rows(rng.random((n, 3)), rng.choice([0.0, 0.5, 1.0], n), rng.choice([0.0, 2e-3, 0.05, 0.5, 1.0], n), rng.choice([1.0, 1.3, 1.5, 2.4], n),
             rng.choice([0.0, 0.5, 1.0], n), rng.integers(0, 2, n), rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-6, 6, (n, 1)),
             unit(rng.standard_normal((n, 3))), rng_floats(rng, (n, 4)))
    lib.smr_steps(n, r.ctypes.data)
    check(lib, {name for name, _ in SITES})


def test_adversarial_shading_steps_stay_inside_the_contracts(lib):
    rng = np.random.default_rng(7)
    roughness = [0.0, 2e-3, 1.0, 1.0000001, 45.0, 2048.0, 1e9, 1e15, 3e38, np.inf, np.nan, -1.0]
    normals = [(0, 0, 1), (0, 0, -1), (1, 0, -0.0), (1, 0, 0.0), (0, 1, -0.0), (1e-8, 0, -1), (1, 1, 1e-30), (1e-30, 0, 0), (1e-20, 1e-20, 1e-20),
               (2.0 ** -70, 0, 2.0 ** -74), (0, 0, 2.0 ** -74), (1e30, 0, 1e30), (3e38, 3e38, 3e38), (0, 0, 0), (1, 2, 3)]
    views = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (1, 0, 1e-7), (1, 0, -1e-7), (1, 1e-20, 1e-38), (0.6, 0.0, 0.8), (0, 0, 1.0000001), (0, 0, 0.99999994),
             (3, 4, 12), (1e-20, 0, 0), (0, 0, 0), (1e30, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0)]
    ends = np.array([2.0 ** -23, 1.0, 0.5, 1.0 - 2.0 ** -23, 2.0 ** -22, 0.25], dtype=np.float32)
    lib.smr_reset()
    total = 0
    for ro in roughness:
        for ior in (1.0, 1.0000001, 0.99999994, 1.5, 0.0, 1e20, np.inf):
            grid = [(a, v) for a in normals for v in views]
            n = len(grid) * 8
            a = np.repeat(np.array([g[0] for g in grid], dtype=np.float64), 8, axis=0)
            v = np.repeat(np.array([g[1] for g in grid], dtype=np.float64), 8, axis=0)
            rnd = ends[rng.integers(0, len(ends), (n, 4))]
            r = rows(rng.choice([0.0, 1.0, 0.5], (n, 3)), rng.choice([0.0, 1.0, 0.5], n), ro, ior, rng.choice([0.0, 1.0], n), rng.integers(0, 2, n), a, v, rnd)
            lib.smr_steps(n, r.ctypes.data)
            total += n
    assert total > 100_000
    check(lib, {"basis_rcp", "vndf_disk", "vndf_nh", "vndf_pdf_root", "vndf_pdf_half", "geom_root_l", "geom_root_v", "fresnel_cos", "refract_root"})


def test_cosine_ray_over_every_u1_the_generator_can_draw_and_below(lib):
    """all 2^23 values of rng_float() as u1, then subnormal and tiny ones: the switched radicand is 1 - fl(sqrt(u1))^2"""
    lib.smr_reset()
    u1 = (np.arange(1, (1 << 23) + 1, dtype=np.float64) * 2.0 ** -23).astype(np.float32)
    r = np.ascontiguousarray(np.stack([np.full_like(u1, 0.375), u1], axis=1))
    lib.smr_cosine(len(u1), r.ctypes.data)
    low = np.array([[0.375, u] for u in (1e-45, 1e-38, 1e-30, 2.0 ** -96, 1e-10, 0.0, -1.0, 2.0, np.inf, np.nan)], dtype=np.float32)
    lib.smr_cosine(len(low), low.ctypes.data)
    mn, mx, seen, special = records(lib)
    k = [name for name, _ in SITES].index("cosine_sin")
    assert seen[k] == len(u1) + len(low)
    assert special[k] >= 1  # u1 = 1 gives sin = 0: a special, which the short form returns as the hardware does
    check(lib, {"cosine_sin"})
