"""CPU: edge operands for every leaf function of the device headers, through tests/hostshim/leaf_batch.h -- one wrapper text that is
compiled as host C++ (here) and for gfx950 (tests/test_gpu_leaf_edges.py runs the same tables on the device and compares word for word).
- oracle == host wrapper, bit for bit, on random + edge operands, wherever the oracle exports the function;
- the batch wrappers == the scalar shim (devmath_host.cpp) on the same operands: the batch plumbing adds nothing;
- float64 accuracy of the spec'd approximations (sincos_2pi, log2_spec, exp2_spec, pow_spec(x, 2.4), atan2_spec) on 2^22 points plus edges;
- property P1 of test_primary_beams.py with beam_rsq one float too high and one too low (the device instruction's error class);
- the floating-point environment of the device build: fp32 subnormals kept ("Floating-point environment").
BUILDERS[name](rng, n) returns n seeded random operands (the distributions of test_leaf_parity.py) followed by the function's hand-written
edge table.  Operands outside a function's contract are left out, and the builder says which: a float -> int
conversion out of range is undefined in C++ and differs between x86 and gfx950 by design."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_primary_beams as tpb

F32P = C.POINTER(C.c_float)
f32 = np.float32
SUB_MIN, SUB_MAX, FLT_MIN, FLT_MAX = f32(1e-45), np.nextafter(f32(1.17549435e-38), f32(0)), f32(1.17549435e-38), np.finfo(np.float32).max
ONE_M, ONE_P = np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(2))
U_MIN = f32(2.0 ** -24)  # rng_float's smallest value; its largest is 1
K_MIN_ROUGHNESS = f32(2e-3)
COS_EDGES = [0.0, SUB_MIN, SUB_MAX, 1e-4, ONE_M, 1.0]  # a cosine's edge values
ETAS = [1.5, 1 / 1.5, 1.33, 1 / 1.33, 1.0]

HERE = os.path.dirname(os.path.abspath(__file__))


def _shapes():
    """name -> (words in, words out): the X(name, in, out) entries of leaf_batch.h's LB_FUNCTIONS, read from the header itself"""
    text = open(os.path.join(HERE, "hostshim", "leaf_batch.h")).read()
    text = text[text.index("#define LB_FUNCTIONS(X)"):]
    found = re.findall(r"X\((\w+), (\d+), (\d+)\)", text)
    assert len(found) == len(set(f[0] for f in found)) >= 40
    return {name: (int(n_in), int(n_out)) for name, n_in, n_out in found}


SHAPES = _shapes()


class Batch:
    """One build of leaf_batch.h: run(name, rows[, aux]) -> the output words (uint32) of every row."""

    def __init__(self, path, prefix):
        self.lib, self.prefix = C.CDLL(path), prefix
        for name in SHAPES:
            fn = getattr(self.lib, prefix + name)
            fn.restype, fn.argtypes = C.c_int, [C.c_uint32, F32P, F32P, F32P, C.c_uint32]

    def run(self, name, rows, aux=None):
        n_in, n_out = SHAPES[name]
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, n_in)
        out = np.zeros((len(rows), n_out), np.float32)
        aux = np.ascontiguousarray(aux, dtype=np.float32) if aux is not None else None
        err = getattr(self.lib, self.prefix + name)(len(rows), rows.ctypes.data_as(F32P), out.ctypes.data_as(F32P),
                                                    aux.ctypes.data_as(F32P) if aux is not None else None, aux.size if aux is not None else 0)
        assert err == 0, f"{self.prefix}{name}: error {err}"
        return out.view(np.uint32)


@pytest.fixture(scope="module")
def hostb():
    import __graft_entry__ as g

    return Batch(g.build_leaf_batch_host(), "lbh_")


# ------------------------------------------------------------------------------------------------ helpers of the builders
def words(*cols):
    """columns (float32 values, or uint32 arrays that travel as bit patterns) -> rows of 32-bit words"""
    n = max(np.size(c) for c in cols)
    out = np.zeros((n, len(cols)), np.float32)
    for k, c in enumerate(cols):
        c = np.asarray(c)
        out[:, k] = c.astype(np.uint32).view(np.float32) if c.dtype.kind in "ui" else c.astype(np.float32)
    return out


def grid(*axes):
    """every combination of the axes' values -> rows (uint32 axes keep their bit patterns)"""
    cols = np.meshgrid(*[np.arange(len(a)) for a in axes], indexing="ij")
    return words(*[np.asarray(a)[c.ravel()] for a, c in zip(axes, cols)])


def both(x):
    """x and its two float neighbours"""
    x = f32(x)
    return [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, np.asarray(parts[0]).shape[-1]) for p in parts])


def u01(rng, n):
    """rng_float's range (0, 1]"""
    return (1.0 - rng.random(n)).astype(np.float32)


AXES = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
U_EDGES = [U_MIN, 1.0]


# ------------------------------------------------------------------------------------------------ builders: random operands + edge table
def b_hash(rng, n):
    return words(np.concatenate([rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), np.uint32([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF])]))


def b_rng_init(rng, n):
    e = np.uint32([0, 1, 65535, 65536, 0xFFFFFFFF])
    return cat(words(rng.integers(0, 65536, n).astype(np.uint32), rng.integers(0, 65536, n).astype(np.uint32),
                     rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)), grid(e, e, e))


def b_sincos_2pi(rng, n):
    # contract: u in [0, 1] (a random number, or a fraction of a turn).  Left out: |u| beyond int range after * 4, inf, NaN -- (int)k is undefined there.
    e = [x for k in range(5) for x in both(k / 4)][1:-1] + [0.0, -0.0, U_MIN, 1 - 2.0 ** -24, SUB_MIN, SUB_MAX, FLT_MIN, 0.125, 1e-7]
    return cat(words(rng.random(n)), words(e))


def b_log2(rng, n):
    # contract: positive normal finite x (the exponent and mantissa are taken from the bits).  Left out: 0, subnormals, negatives, inf, NaN.
    e = [f32(2.0) ** k for k in range(-126, 128)] + both(np.sqrt(f32(2))) + both(f32(1.41421356237309504880)) + both(np.sqrt(f32(0.5))) + both(1.0) + [FLT_MIN, FLT_MAX, 0.526]
    return cat(words(np.exp(rng.uniform(-20, 20, n))), words(e))


def b_exp2(rng, n):
    # contract: floor(y + 0.5) in [-126, 127] (the scale 2^k is built from the bits).  Left out: beyond that, inf, NaN.  Results down to
    # 2^-126.5 are subnormal.  pt_denoise.h reaches -80 / ln 2 = -115.4.
    half = [f32(k / 2) for k in range(-252, 255)]
    e = half + [x for h in half[1::2] for x in both(h)] + [np.nextafter(f32(-126.5), f32(0)), f32(-80 / np.log(2)), -115.0, -116.0, 0.0, -0.0, SUB_MIN, -SUB_MIN, ONE_M, ONE_P, 127.49]
    return cat(words(rng.uniform(-30, 30, n)), words(rng.uniform(-126.4, 127.4, n // 4)), words(e))


def b_pow(rng, n):
    # contract: x as log2_spec, y log2(x) as exp2_spec
    e = grid([1.0, ONE_M, ONE_P, 0.5, 2.0, 0.02, 0.0031308, 1e-4, 1e4, FLT_MIN], [2.4, 1 / 2.4, 1 / 2.2, 0.1593017578, 78.84375 / 64, 0.0, 1.0, -1.0])
    return cat(words(rng.uniform(0.02, 1.0, n), np.full(n, 2.4)), words(np.exp(rng.uniform(-8, 8, n)), rng.uniform(-3, 3, n)), e)


def b_from_srgb(rng, n):
    # contract: any value (saturate first; NaN -> 0)
    e = both(0.04045) + [0.0, -0.0, 1.0, ONE_M, ONE_P, -1.0, 2.0, SUB_MIN, SUB_MAX, FLT_MIN, FLT_MAX, np.inf, -np.inf, np.nan, 0.5, 0.7]
    return cat(words(rng.uniform(-0.2, 1.2, n)), words(e))


def b_get_basis(rng, n):
    # contract: a unit N.  Sign(N.z) switches at -0 / the smallest negative subnormal; sz + N.z is -2 at N.z = -1 and never 0.
    z = [0.0, -0.0, SUB_MIN, -SUB_MIN, -1.0, np.nextafter(f32(-1), f32(0)), 1.0, ONE_M]
    e = [[np.sqrt(max(0.0, 1.0 - float(v) ** 2)), 0.0, v] for v in z] + [[0.0, np.sqrt(max(0.0, 1.0 - float(v) ** 2)), v] for v in z] + [[0.6, 0.8, v] for v in z[:4]]
    return cat(unit(rng, n), AXES, e)


def b_refract(rng, n):
    # contract: unit i and n, eta > 0.  k = 1 - eta^2 (1 - c^2) crosses 0 at the critical angle: every float within 16 of it.
    i, nn = unit(rng, n), unit(rng, n)
    rows = [np.concatenate([i, nn, rng.choice(f32(ETAS), n)[:, None]], axis=1)]
    for eta in (1.5, 1.33, 2.4):
        c = f32(np.sqrt(1.0 - 1.0 / eta ** 2))
        for _ in range(16):
            c = np.nextafter(c, f32(0))
        for _ in range(33):
            rows.append([[np.sqrt(max(0.0, 1.0 - float(c) ** 2)), 0.0, -c, 0.0, 0.0, 1.0, eta]])
            c = np.nextafter(c, f32(1))
    rows.append([[0, 0, -1, 0, 0, 1, 1.5], [1, 0, 0, 0, 0, 1, 1.5], [1, 0, -0.0, 0, 0, 1, 1.0], [0.6, 0, -0.8, 0, 0, 1, 1.0]])
    return cat(*rows)


def b_cosine_ray(rng, n):
    return cat(words(u01(rng, n), u01(rng, n)), grid(U_EDGES + [0.25, 0.5], U_EDGES + [ONE_M, SUB_MIN]))


def vl_of(z):
    return [np.sqrt(max(0.0, 1.0 - float(z) ** 2)), 0.0, z]


def b_vndf_ray(rng, n):
    # contract: u in (0, 1], roughness in [kMinRoughness, 1], unit Vl with Vl.z >= 0
    vl = unit(rng, n); vl[:, 2] = np.abs(vl[:, 2])
    e = [[u0, u1, r] + vl_of(z) for u0 in U_EDGES for u1 in U_EDGES for r in (K_MIN_ROUGHNESS, 1.0) for z in (0.0, 1e-7, 1.0, ONE_M, SUB_MIN)]
    return cat(np.concatenate([words(u01(rng, n), u01(rng, n), rng.uniform(2e-3, 1.0, n)), vl], axis=1), e)


def b_vndf_pdf(rng, n):
    vl = unit(rng, n); vl[:, 2] = np.abs(vl[:, 2])
    e = [vl_of(z) + [noh, r] for z in COS_EDGES for noh in COS_EDGES for r in (K_MIN_ROUGHNESS, 1.0)]
    return cat(np.concatenate([vl, words(rng.random(n), rng.uniform(2e-3, 1.0, n))], axis=1), e)


ROUGH_EDGES = [K_MIN_ROUGHNESS, 1.0]


def rough(rng, n):
    return np.concatenate([rng.uniform(2e-3, 1.0, n - n // 2), np.full(n // 2, 2e-3)]).astype(np.float32)


def b_distribution_term(rng, n):
    # contract of the BRDF terms: roughness in [kMinRoughness, 1], cosines in [0, 1].  Left out: NaN, inf, negatives.
    return cat(words(rough(rng, n), rng.random(n)), grid(ROUGH_EDGES, COS_EDGES))


def b_geometry_term_mod(rng, n):
    return cat(words(rough(rng, n), rng.random(n), rng.random(n)), grid(ROUGH_EDGES, COS_EDGES, COS_EDGES))


def b_fresnel_dielectric(rng, n):
    crit = [x for eta in ETAS for x in both(np.sqrt(f32(abs(1.0 - 1.0 / eta ** 2))))]
    return cat(words(rng.choice(f32(ETAS), n), rng.random(n)), grid(f32(ETAS), COS_EDGES + crit))


def b_diffuse_term(rng, n):
    return cat(words(rough(rng, n), rng.random(n), rng.random(n), rng.random(n)), grid(ROUGH_EDGES, COS_EDGES, COS_EDGES, [0.0, SUB_MIN, 1.0]))


def b_environment_term_rtg(rng, n):
    return cat(words(rng.random(n), rng.random(n), rng.random(n), rng.random(n), rough(rng, n)),
               grid([0.0, 1.0], [0.04], [1.0], COS_EDGES, ROUGH_EDGES))


def b_sky(rng, n):
    d = unit(rng, n)
    e = [[-1, -1, -1, -1] + list(a) for a in AXES] + [[0.25, 0.5, 0.75, 1.0, 0, 1, 0], [0.25, 0.5, 0.75, 0.0, 0, 1, 0], [0.25, 0.5, 0.75, -0.0, 0, 1, 0],
                                                       [-1, -1, -1, -SUB_MIN, 0, ONE_M, 0], [1, 1, 1, -1, 0, SUB_MIN, 1]]
    return cat(np.concatenate([np.tile(f32([-1, -1, -1, -1]), (n, 1)), d], axis=1), e)


def sphere_rays(rng, n):
    """test_leaf_parity.py's distribution: (o, d, C, r), most rays aimed into their sphere"""
    c = rng.uniform(-10, 10, (n, 3))
    r = np.exp(rng.uniform(np.log(0.02), np.log(50), n))
    o = rng.uniform(-20, 20, (n, 3))
    d = c + rng.normal(size=(n, 3)) * r[:, None] * 0.8 - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32), c.astype(np.float32), r.astype(np.float32)


def sphere_edge_rows():
    """(o, d, tmin, tmax, C, r): origin on the surface, inside, at the centre, 1e6 radii away; exactly tangent rays; tmin == tmax; r in {1e-6, 1, 1e6}"""
    rows = []
    for r in (1e-6, 1.0, 1e6):
        for c in ([0, 0, 0], [3, -2, 5]):
            c = np.float64(c) * (r if r > 1 else 1.0)
            for o, d in ((c + [0, 0, -r], [0, 0, 1]), (c + [0, 0, -r], [0, 0, -1]), (c + [0, 0, r], [0, 0, 1]), (c + [0.5 * r, 0, 0], [0, 0, 1]), (c, [0, 1, 0]),
                         (c + [0, 0, -1e6 * r], [0, 0, 1]), (c + [r, 0, -3 * r], [0, 0, 1]), (c + [-r, 0, -3 * r], [0, 0, 1]), (c + [0, r, 2 * r], [0, 0, -1]),
                         (c + [0, 0, -1e6 * r], [0, 0, -1]), (c + [0, 0, -2 * r], [0.6, 0, 0.8])):
                for tmin, tmax in ((0.0, np.inf), (0.0, 2 * r), (r, r), (2 * r, np.inf), (0.0, SUB_MIN)):
                    rows.append(list(o) + list(d) + [tmin, tmax] + list(c) + [r])
    return np.float32(rows)


def sphere_random_rows(rng, n):
    o, d, c, r = sphere_rays(rng, n)
    return np.concatenate([o, d, np.zeros((n, 1), np.float32), np.full((n, 1), np.inf, np.float32), c, r[:, None]], axis=1)


def b_intersect_sphere(rng, n):
    # contract: unit d, tmin >= 0, finite sphere with r > 0
    return cat(sphere_random_rows(rng, n), sphere_edge_rows())


def hits_of(hostb_, rows):
    """(rows that hit, their t) by the host build's own intersect_sphere"""
    out = hostb_.run("intersect_sphere", rows)
    hit = out[:, 0] == 1
    return rows[hit], out[hit, 1].view(np.float32)


def b_hit_frame(rng, n, hostb_):
    # n random rays that hit (drawn until there are n), then the edge table's hits
    rows, t = np.zeros((0, 12), np.float32), np.zeros(0, np.float32)
    while len(rows) < n:
        more, tm = hits_of(hostb_, sphere_random_rows(rng, max(2 * (n - len(rows)), 256)))
        rows, t = np.concatenate([rows, more]), np.concatenate([t, tm])
    edge, te = hits_of(hostb_, sphere_edge_rows())
    rows, t = np.concatenate([rows[:n], edge]), np.concatenate([t[:n], te])
    return np.concatenate([rows[:, :6], t[:, None], rows[:, 8:12]], axis=1)


def b_spawn_origin(rng, n, hostb_):
    hf = hostb_.run("hit_frame", b_hit_frame(rng, n, hostb_)).view(np.float32)
    L = unit(rng, len(hf))
    L[:6] = AXES
    tang = np.cross(hf[:, 3:6], L); L[6::7] = tang[6::7]  # directions in the tangent plane: dot(L, N) about 0, the Sign switch
    return np.concatenate([hf[:, :7], L], axis=1).astype(np.float32)


def cameras(rng, n):
    rows = []
    for _ in range(n):
        cam, w, h = tpb.random_camera(rng, list(tpb.LENS_CLASSES)[len(rows) % 3], far=(len(rows) % 5 == 4))
        rows.append((cam, w, h))
    return rows


def b_primary_ray(rng, n):
    out = []
    for cam, w, h in cameras(rng, max(8, n // 64)):
        m = 64
        px, py = rng.integers(0, w, m), rng.integers(0, h, m)
        px[:4], py[:4] = (0, w - 1, 0, w - 1), (0, 0, h - 1, h - 1)
        jit = rng.uniform(-0.5, 0.5, (m, 2)); jit[:4] = tpb.JIT_CORNERS
        near = rng.choice([0.0, 1e-2, 1.0], m)
        out.append(np.concatenate([np.tile(cam, (m, 1)), words(near, np.where(rng.random(m) < 0.5, np.inf, 1e4), jit[:, 0], jit[:, 1]),
                                   words(px.astype(np.uint32), py.astype(np.uint32), np.full(m, w, np.uint32), np.full(m, h, np.uint32))], axis=1))
    return cat(*out)


def bsdf_rows(base, metallic, roughness, ior, transmission, front, Ng, V, rnd):
    n = len(Ng)
    flip = (np.einsum("ij,ij->i", Ng, V) < 0)
    V = V.copy()
    V[(flip & (front == 1)) | (~flip & (front == 0))] *= -1  # V on the side of the shading normal (front ? Ng : -Ng)
    return np.concatenate([base, words(metallic, roughness, ior, transmission, front.astype(np.uint32)), Ng, V, rnd], axis=1).astype(np.float32).reshape(n, 18)


def b_bsdf_step(rng, n):
    # contract: what a hit hands over -- unit Ng and V on the shading side, rnd in (0, 1]^4, material fields in their documented ranges
    r = bsdf_rows(rng.random((n, 3)), rng.choice([0.0, 1.0, 0.5], n) * rng.random(n) ** 0.3, rng.choice([0.0, 1.0], n) * rng.random(n), rng.choice([1.5, 1.33, 1.0, 2.4], n),
                  rng.choice([0.0, 1.0, 0.5], n), rng.integers(0, 2, n), unit(rng, n), unit(rng, n), np.stack([u01(rng, n) for _ in range(4)], axis=1))
    # the material corners x random numbers at their ends x V from head-on to grazing
    c = grid([0.0, 1.0], [0.0, 1.0], [1.0, 1.5, 2.4], [0.0, 1.0], [0, 1], [0, 1, 2, 3], [0.0, 1e-7, 1e-3, 1.0])
    m = len(c)
    vz = c[:, 6]
    V = np.stack([np.sqrt(np.maximum(0.0, 1.0 - vz.astype(np.float64) ** 2)), np.zeros(m), vz], axis=1).astype(np.float32)
    rnd2 = f32([[U_MIN] * 4, [1.0] * 4, [U_MIN, 1.0, U_MIN, 1.0], [1.0, U_MIN, 1.0, U_MIN]])[c[:, 5].astype(int)]
    e = bsdf_rows(np.tile(f32([0.8, 0.5, 0.2]), (m, 1)), c[:, 0], c[:, 1], c[:, 2], c[:, 3], c[:, 4].astype(int), np.tile(f32([0, 0, 1]), (m, 1)), V, rnd2.astype(np.float32))
    return cat(r, e)


def b_tonemap_pixel(rng, n):
    # contract: any hdr (the curves clamp; NaN -> 0), the three operators, transfer functions and rotations
    hdr = np.exp(rng.uniform(-8, 4, (n, 3))) * rng.choice([1.0, 1.0, 1.0, 0.0, -1.0], (n, 3))
    r = np.concatenate([hdr, words(rng.integers(0, 4, n).astype(np.uint32), rng.integers(0, 3, n).astype(np.uint32), np.exp2(rng.integers(-3, 4, n)), rng.choice([80.0, 200.0, 1000.0], n),
                                   rng.integers(0, 3, n).astype(np.uint32))], axis=1)
    v = [0.0, -0.0, SUB_MIN, FLT_MIN, 0.5, 1.0, ONE_P, 1e4, FLT_MAX, np.inf, -1.0, np.nan]
    e = grid(v, [0.18], v[:6], np.uint32([0, 1, 2, 3]), np.uint32([0, 1, 2]), [1.0], [200.0], np.uint32([0, 1, 2]))
    return cat(r, e)


def accumulate_rows(accum, x, k):
    """(accum, x, inv, first) as pt_accumulate forms them from k, the number of frames already accumulated"""
    k = np.asarray(k, dtype=np.int64)
    return words(accum, x, f32(1.0) / (k + 1).astype(np.float32), (k == 0).astype(np.uint32))


def b_accumulate(rng, n):
    # contract: any accum and x; inv = 1 / (float)(k + 1) and first = (k == 0) for k frames accumulated
    e = grid([0.0, SUB_MIN, 1.0, FLT_MAX, np.inf, np.nan], [0.0, -0.0, SUB_MAX, 1.0, FLT_MAX], [0.0, 1.0, 2.0, 999.0, 2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 31])
    return cat(accumulate_rows(rng.random(n), rng.random(n), rng.integers(0, 1000, n)), accumulate_rows(e[:, 0], e[:, 1], e[:, 2].astype(np.int64)))


def b_unorm(rng, n):
    # v whose scaled value ends in exactly .5 rounds up by the + 0.5 (v = 0.5: 127.5 and 511.5); NaN and -0 -> 0
    e = [0.0, -0.0, np.nan, 0.5, 1.0, ONE_M, ONE_P, SUB_MIN, -1.0, np.inf, -np.inf, 0.25, 0.75] + [x for m in (0, 1, 127, 254) for x in both((m + 0.5) / 255.0)]
    return cat(words(rng.uniform(-0.2, 1.2, n), rng.choice([255.0, 1023.0], n)), grid(e, [255.0, 1023.0, 3.0]))


def b_sample_sphere_cone(rng, n):
    # contract: finite P, C, r > 0, u in (0, 1]
    P, C_ = rng.uniform(-20, 20, (n, 3)), rng.uniform(-20, 20, (n, 3))
    r = np.exp(rng.uniform(np.log(1e-2), np.log(30), n))
    e = [[0, 0, 0] + list(np.float64(a) * dist) + [1.0, u1, u2] for a in AXES[:3] for dist in (0.5, 1.0, ONE_P, 2.0, 1e3, 1e6) for u1 in U_EDGES for u2 in U_EDGES + [0.25]]
    return cat(np.concatenate([P, C_, words(r, u01(rng, n), u01(rng, n))], axis=1), e)


def b_pick_light(rng, n):
    # contract: u in (0, 1], 1 <= n_lights
    return cat(words(u01(rng, n), rng.integers(1, 1000, n).astype(np.uint32)), grid(U_EDGES + [ONE_M, 0.5], np.uint32([1, 2, 7, 1000, 1 << 24])))


def b_atan2(rng, n):
    # contract: finite operands (inf / inf would be NaN).  atan2(0, 0) = 0 for either sign of either zero.
    v = [0.0, -0.0, SUB_MIN, -SUB_MIN, FLT_MIN, 1.0, -1.0, ONE_M, ONE_P, 1e-30, 1e30, FLT_MAX, -FLT_MAX]
    return cat(words(rng.normal(size=n), rng.normal(size=n)), grid(v, v))


def dir_edges():
    t = [[1, 1, 0], [1, -1, 0], [0, 1, 1], [0, -1, 1], [1, 0, 1], [-1, 0, -1], [1, 1, 1], [-1, 1, -1], [-1, -1, -1], [1, -1, 1], [0, 0, 0], [-0.0, 0.0, -0.0],
         [SUB_MIN, 0, 0], [0, SUB_MIN, SUB_MIN], [FLT_MAX, 1, 1], [ONE_M, 1, ONE_M], [1, ONE_M, 1]]
    return cat(AXES, t, np.float32(t[:10]) * f32(0.57735026))


def b_dirs(rng, n):
    # contract: any direction; the zero vector divides 0 / 0 (a NaN coordinate the samplers turn into texel 0)
    return cat(unit(rng, n), dir_edges())


def b_quat_rotate(rng, n):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    e = [[0, 0, 0, 1] + list(a) for a in AXES] + [[1, 0, 0, 0] + list(a) for a in AXES] + [[0.5, 0.5, 0.5, 0.5, 1, 2, 3], [0, 0, 0, 1, SUB_MIN, 0, FLT_MAX]]
    return cat(np.concatenate([q, rng.normal(size=(n, 3))], axis=1), e)


def b_perturb_normal(rng, n):
    # contract: unit N, a tangent T not parallel to it (a parallel T normalises the zero vector: NaN, kept), sx, sy texel values in [0, 1]
    N = unit(rng, n)
    e = [list(a) + list(t) + [sx, sy] for a in AXES[::2] for t in AXES[1::2] for sx in (0.0, 127 / 255.0, 0.5, 1.0) for sy in (0.0, 127 / 255.0, 1.0)]
    return cat(np.concatenate([N, unit(rng, n), rng.random((n, 2))], axis=1), e)


TEXTURE_DIMS = [(1, 1), (2, 3)]  # (w, h)


def texture_images():
    """the two 8-bit RGBA images (h, w, 4) behind the samplers' table"""
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for w, h in TEXTURE_DIMS]


def texture_table():
    """leaf_batch.h's aux table: a 1 x 1 and a 2 x 3 (w x h) texture, texels = (float)byte * (1 / 255) as pt_set_textures converts RGBA8_UNORM"""
    head, texels, first = [], [], 2
    for (w, h), img in zip(TEXTURE_DIMS, texture_images()):
        head.append(np.uint32([w, h, first, 0]).view(np.float32))
        texels.append((img.astype(np.float32) * (f32(1.0) / f32(255.0))).ravel())
        first += w * h
    return np.concatenate(head + texels)


def b_sample_bilinear(rng, n):
    # contract: any uv (|uv| >= 65536 and NaN read texel 0), a texture of the table
    v = [0.0, 1.0, np.nextafter(f32(0), f32(-1)), ONE_P, 65535.999, -65535.999, 65536.0, -65536.0, np.nan, 0.5, 0.25, -0.25, 1 / 3.0, np.inf, SUB_MIN, ONE_M]
    return cat(words(rng.uniform(-2, 3, n), rng.uniform(-2, 3, n), rng.integers(0, 2, n).astype(np.uint32)), grid(v, v, np.uint32([0, 1])))


def regions(rng, n_regions):
    import test_refl_region as trr

    return [trr.random_region(rng) for _ in range(n_regions)]


def b_rg_contains(rng, n, hostb_):
    # contract: a region as region_set_cone / region_from_hits make it, finite rays; origins on O's faces and directions at the cone's edge
    out = []
    for lo, hi, axis, theta in regions(rng, max(4, n // 512)):
        g = hostb_.run("rg_make", np.concatenate([lo, hi, axis, [theta]])[None]).view(np.float32)[0]
        m = 512
        o = (lo - 0.01 * (hi - lo) + rng.random((m, 3)) * 1.02 * (hi - lo)).astype(np.float32)
        face = rng.random((m, 3)) < 0.2
        o = np.where(face, np.where(rng.random((m, 3)) < 0.5, g[0:3], g[3:6]), o)
        ang = theta * rng.uniform(0.98, 1.02, m)
        t = np.cross(axis, rng.normal(size=(m, 3))); t /= np.linalg.norm(t, axis=1, keepdims=True)
        d = (np.cos(ang)[:, None] * axis + np.sin(ang)[:, None] * t).astype(np.float32)
        out.append(np.concatenate([np.tile(g, (m, 1)), o, d], axis=1))
    return cat(*out)


BUILDERS = {
    "hash": b_hash, "rng_init": b_rng_init, "rng_next": b_hash, "rng_float": b_hash, "sincos_2pi": b_sincos_2pi, "log2": b_log2, "exp2": b_exp2, "pow": b_pow,
    "from_srgb": b_from_srgb, "get_basis": b_get_basis, "refract": b_refract, "cosine_ray": b_cosine_ray, "vndf_ray": b_vndf_ray, "vndf_pdf": b_vndf_pdf,
    "distribution_term": b_distribution_term, "geometry_term_mod": b_geometry_term_mod, "fresnel_dielectric": b_fresnel_dielectric, "diffuse_term": b_diffuse_term,
    "environment_term_rtg": b_environment_term_rtg, "sky": b_sky, "intersect_sphere": b_intersect_sphere, "hit_frame": b_hit_frame, "spawn_origin": b_spawn_origin,
    "primary_ray": b_primary_ray, "bsdf_step": b_bsdf_step, "tonemap_pixel": b_tonemap_pixel, "accumulate": b_accumulate, "unorm": b_unorm,
    "sample_sphere_cone": b_sample_sphere_cone, "pick_light": b_pick_light, "atan2": b_atan2, "cube_face_uv": b_dirs, "latlong_uv": b_dirs, "sphere_uv": b_dirs,
    "sphere_tangent": b_dirs, "quat_rotate": b_quat_rotate, "perturb_normal": b_perturb_normal, "sample_bilinear": b_sample_bilinear,
    "sample_bilinear_clamp": b_sample_bilinear, "rg_contains": b_rg_contains}
NEEDS_HOST = {"hit_frame", "spawn_origin", "rg_contains"}  # builders that derive operands from the host build's own results
PARITY_FUNCTIONS = sorted(BUILDERS)


def build_rows(name, n, hostb_):
    """(rows, aux) of a function: seeded by its name, so the CPU and the GPU tests see the same operands"""
    rng = np.random.default_rng([sum(name.encode()), len(name), 2024])
    rows = BUILDERS[name](rng, n, hostb_) if name in NEEDS_HOST else BUILDERS[name](rng, n)
    assert rows.dtype == np.float32 and rows.shape[1] == SHAPES[name][0], (name, rows.shape)
    return rows, (texture_table() if name.startswith("sample_bilinear") else None)


def same_words(a, b, float_cols=None):
    """rows whose words differ; two NaNs of a float column count as equal"""
    a, b = np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)
    diff = a != b
    fa, fb = a.view(np.float32), b.view(np.float32)
    both_nan = np.isnan(fa) & np.isnan(fb)
    if float_cols is not None:
        both_nan &= np.isin(np.arange(a.shape[1]), float_cols)[None, :]
    return np.flatnonzero((diff & ~both_nan).any(axis=1))


# columns of a function's output that are integers or flags (never NaN-compared); every other column is a float
INT_COLS = {"hash": [0], "rng_init": [0], "rng_next": [0, 1], "rng_float": [0], "intersect_sphere": [0], "hit_frame": [7], "bsdf_step": [0, 1], "tonemap_pixel": [0],
            "unorm": [0], "sample_sphere_cone": [0], "pick_light": [0], "cube_face_uv": [0], "rg_contains": [0]}


def float_cols(name):
    return [k for k in range(SHAPES[name][1]) if k not in INT_COLS.get(name, [])]


# ------------------------------------------------------------------------------------------------ scalar calls (oracle_ / dev_ prefix)
def fptr(a):
    return a.ctypes.data_as(F32P)


class Textures:
    """the samplers' two images as the scalar APIs take them: PtTexture descriptors (dev_sample_texture) and the oracle's texture table"""

    def __init__(self, dxrs):
        from oracle.binding import OracleTextures

        from dxrs_amd.textures import TextureSet  # (dxrs_amd_loader has registered the package: the dxrs fixture)

        self.set = TextureSet(1)
        for img in texture_images():
            self.set.add_image(img)
        self.tex, n_tex, obj, rot = self.set.as_ctypes()
        self.oracle = OracleTextures(C.cast(self.tex, C.c_void_p), n_tex, C.cast(obj, C.c_void_p), rot.ctypes.data)


def scalar_call(lib, prefix, name, row, dxrs, textures=None):
    """One row through the scalar API shared by the oracle and devmath_host.cpp (oracle.binding.declare_leaf_api, and their texture
    samplers) -> output words, or None if the API has no such function."""
    r = np.ascontiguousarray(row, dtype=np.float32)
    u = r.view(np.uint32)
    fn = getattr(lib, prefix + name, None)
    cf = lambda k: C.c_float(float(r[k])) if not np.isnan(r[k]) else C.c_float(np.nan)
    out = np.zeros(SHAPES[name][1], np.float32)
    ou = out.view(np.uint32)
    if name == "hash":
        ou[0] = fn(int(u[0]))
    elif name == "rng_init":
        ou[0] = fn(int(u[0]), int(u[1]), int(u[2]))
    elif name in ("rng_next", "rng_float"):
        s = C.c_uint32(int(u[0]))
        v = fn(C.byref(s))
        ou[0] = s.value
        if name == "rng_next":
            ou[1] = v
        else:
            out[1] = v
    elif name == "sincos_2pi":
        s, c = C.c_float(), C.c_float()
        fn(cf(0), C.byref(s), C.byref(c)); out[:] = (s.value, c.value)
    elif name in ("log2", "exp2", "from_srgb"):
        out[0] = fn(cf(0))
    elif name in ("pow", "distribution_term", "fresnel_dielectric", "atan2"):
        out[0] = fn(cf(0), cf(1))
    elif name == "geometry_term_mod":
        out[0] = fn(cf(0), cf(1), cf(2))
    elif name == "diffuse_term":
        out[0] = fn(cf(0), cf(1), cf(2), cf(3))
    elif name == "get_basis":
        fn(fptr(r[0:3]), fptr(out[0:3]), fptr(out[3:6]))
    elif name == "cosine_ray":
        fn(fptr(r[0:2]), fptr(out))
    elif name == "vndf_ray":
        fn(fptr(r[0:2]), cf(2), fptr(r[3:6]), fptr(out))
    elif name == "vndf_pdf":
        out[0] = fn(fptr(r[0:3]), cf(3), cf(4))
    elif name == "environment_term_rtg":
        fn(fptr(r[0:3]), cf(3), cf(4), fptr(out))
    elif name == "intersect_sphere":
        t = C.c_float(-1.0)
        ou[0] = fn(fptr(r[0:3]), fptr(r[3:6]), cf(6), cf(7), r[8:12].ctypes.data, C.byref(t)); out[1] = t.value
    elif name == "hit_frame":
        off, front = C.c_float(), C.c_int()
        fn(fptr(r[0:3]), fptr(r[3:6]), cf(6), r[7:11].ctypes.data, fptr(out[0:3]), fptr(out[3:6]), C.byref(off), C.byref(front))
        out[6] = off.value; ou[7] = front.value
    elif name == "spawn_origin":
        fn(fptr(r[0:3]), fptr(r[3:6]), cf(6), fptr(r[7:10]), fptr(out))
    elif name == "bsdf_step":
        m = dxrs.types.default_material(1)
        m["BaseColor"][0, :3] = r[0:3]
        m["Metallic"], m["Roughness"], m["IOR"], m["Transmission"] = r[3], r[4], r[5], r[6]
        fn(m.ctypes.data, int(u[7]), fptr(r[8:11]), fptr(r[11:14]), fptr(r[14:18]), C.cast(out.ctypes.data, C.c_void_p))
    elif name == "sample_sphere_cone":
        ip = C.c_float()
        ou[0] = fn(fptr(r[0:3]), fptr(r[3:6]), cf(6), cf(7), cf(8), fptr(out[1:4]), C.byref(ip)); out[4] = ip.value
    elif name == "cube_face_uv":
        ou[0] = fn(fptr(r[0:3]), fptr(out[1:3]))
    elif name in ("latlong_uv", "sphere_uv", "sphere_tangent"):
        fn(fptr(r[0:3]), fptr(out))
    elif name == "quat_rotate":
        fn(fptr(r[0:4]), fptr(r[4:7]), fptr(out))
    elif name == "perturb_normal":
        fn(fptr(r[0:3]), fptr(r[3:6]), cf(6), cf(7), fptr(out))
    elif name == "sky":
        sd = dxrs.types.PtSceneData()
        sd.EnvironmentLightColor[:] = [float(v) for v in r[0:4]]
        fn(C.addressof(sd), fptr(r[4:7]), fptr(out))
    elif name == "primary_ray":
        cam = dxrs.types.PtCamera()
        cam.Position[:], cam.RightDirection[:], cam.UpDirection[:], cam.ForwardDirection[:] = ([float(v) for v in r[k:k + 3]] for k in (0, 3, 6, 9))
        cam.NearDepth, cam.FarDepth, cam.Jitter[0], cam.Jitter[1] = float(r[12]), float(r[13]), float(r[14]), float(r[15])
        tmin, tmax = C.c_float(), C.c_float()
        fn(C.addressof(cam), int(u[16]), int(u[17]), int(u[18]), int(u[19]), fptr(out[0:3]), fptr(out[3:6]), C.byref(tmin), C.byref(tmax))
        out[6], out[7] = tmin.value, tmax.value
    elif name == "tonemap_pixel":
        tp = dxrs.types.PtToneMapParams()
        tp.Operator, tp.TransferFunction, tp.LinearExposure, tp.PaperWhiteNits, tp.ColorRotation = int(u[3]), int(u[4]), float(r[5]), float(r[6]), int(u[7])
        ou[0] = fn(fptr(r[0:3]), C.addressof(tp))
    elif name == "accumulate":
        # (accum, x, inv, first) -> the k frames already accumulated that pt_accumulate's caller states: inv = 1 / (float)(k + 1), first = (k == 0)
        k = 0 if u[3] else int(round(1.0 / float(r[2]))) - 1
        assert (k == 0) == bool(u[3]) and f32(1.0) / f32(k + 1) == r[2], (k, r)
        acc, rad = np.full(4, r[0], np.float32), np.full(4, r[1], np.float32)
        fn(acc.ctypes.data, rad.ctypes.data, 1, k)
        assert len(set(acc.view(np.uint32)[~np.isnan(acc)])) <= 1
        out[0] = acc[0]
    elif name == "sample_bilinear":
        if prefix == "oracle_":
            lib.oracle_sample_texture(C.addressof(textures.oracle), int(u[2]), fptr(r[0:2]), fptr(out))
        else:
            lib.dev_sample_texture(C.addressof(textures.tex[int(u[2])]), fptr(r[0:2]), fptr(out))
    else:
        return None
    return ou.copy()


SCALAR_FUNCTIONS = ["hash", "rng_init", "rng_next", "rng_float", "sincos_2pi", "log2", "exp2", "pow", "from_srgb", "get_basis", "cosine_ray", "vndf_ray", "vndf_pdf",
                    "distribution_term", "geometry_term_mod", "fresnel_dielectric", "diffuse_term", "environment_term_rtg", "sky", "intersect_sphere", "hit_frame",
                    "spawn_origin", "primary_ray", "bsdf_step", "tonemap_pixel", "accumulate", "sample_sphere_cone", "atan2", "cube_face_uv", "latlong_uv", "sphere_uv",
                    "sphere_tangent", "quat_rotate", "perturb_normal", "sample_bilinear"]
# what neither scalar API exports, and the test below that states its contract another way
CONTRACT_FUNCTIONS = {"refract": "test_refract_contract", "unorm": "test_unorm_and_pick_light_contracts", "pick_light": "test_unorm_and_pick_light_contracts",
                      "sample_bilinear_clamp": "test_clamp_sampler_matches_bloom_shim", "rg_contains": "test_region_contains_contract"}
N_SCALAR = 1500  # random rows per function in the scalar comparisons (one Python call each); the edge table is always whole


def test_every_function_is_vetted_on_the_cpu():
    """every function the GPU test gives to the device is compared with something else on the CPU first"""
    assert set(SCALAR_FUNCTIONS) | set(CONTRACT_FUNCTIONS) == set(PARITY_FUNCTIONS) and not set(SCALAR_FUNCTIONS) & set(CONTRACT_FUNCTIONS)
    assert all(callable(globals()[t]) for t in CONTRACT_FUNCTIONS.values())
    assert set(PARITY_FUNCTIONS) <= set(SHAPES)


@pytest.mark.parametrize("name", PARITY_FUNCTIONS)
def test_host_build_runs_every_table(name, hostb):
    """Every builder's rows (4096 random + the whole edge table) through the host library: under tools/sanitize.sh an index out of range
    or an undefined conversion caused by an edge operand shows here, before the same table is given to a GPU.  The results are finite
    or NaN words of the right shape; what they must be is the other tests' business."""
    rows, aux = build_rows(name, 4096, hostb)
    assert len(rows) >= 4096
    out = hostb.run(name, rows, aux)
    assert out.shape == (len(rows), SHAPES[name][1])
    again = hostb.run(name, rows, aux)
    assert not len(same_words(out, again, float_cols(name))), "the host build is not deterministic"


def compare_with_scalar(lib, prefix, name, hostb_, dxrs):
    from oracle.binding import declare_leaf_api

    declare_leaf_api(lib, prefix)
    getattr(lib, prefix + "bsdf_step").argtypes = [C.c_void_p, C.c_int, F32P, F32P, F32P, C.c_void_p]
    if prefix == "oracle_":
        lib.oracle_sample_texture.restype, lib.oracle_sample_texture.argtypes = None, [C.c_void_p, C.c_uint32, F32P, F32P]
    else:
        lib.dev_sample_texture.restype, lib.dev_sample_texture.argtypes = None, [C.c_void_p, F32P, F32P]
    textures = Textures(dxrs) if name == "sample_bilinear" else None
    rows, aux = build_rows(name, N_SCALAR, hostb_)
    got = hostb_.run(name, rows, aux)
    want = np.stack([scalar_call(lib, prefix, name, row, dxrs, textures) for row in rows])
    bad = same_words(got, want, float_cols(name))
    assert not len(bad), f"{name}: {len(bad)} of {len(rows)} rows differ; first: in {rows[bad[0]]!r} batch {got[bad[0]].view(np.float32)!r} {prefix} {want[bad[0]].view(np.float32)!r}"


@pytest.mark.parametrize("name", SCALAR_FUNCTIONS)
def test_oracle_matches_host_wrapper(name, hostb, oracle, dxrs):
    """The oracle and the device header (host build), bit for bit, on random + edge operands."""
    compare_with_scalar(oracle.lib, "oracle_", name, hostb, dxrs)


@pytest.mark.parametrize("name", SCALAR_FUNCTIONS)
def test_batch_wrapper_matches_scalar_shim(name, hostb, dxrs):
    """leaf_batch.h's wrapper and devmath_host.cpp's scalar export of the same function agree on every word: the batch plumbing adds nothing."""
    import __graft_entry__ as g

    compare_with_scalar(C.CDLL(g.build_test_shim()), "dev_", name, hostb, dxrs)


def test_clamp_sampler_matches_bloom_shim(hostb):
    """lb_sample_bilinear_clamp against bloom_host.cpp's bloom_sample (sample_bilinear_clamp on a caller's texel array), bit for bit"""
    import __graft_entry__ as g

    lib = C.CDLL(g.build_bloom_shim())
    lib.bloom_sample.restype, lib.bloom_sample.argtypes = None, [F32P, C.c_uint32, C.c_uint32, C.c_float, C.c_float, F32P]
    rows, aux = build_rows("sample_bilinear_clamp", N_SCALAR, hostb)
    got = hostb.run("sample_bilinear_clamp", rows, aux)
    au = aux.view(np.uint32)
    want = np.zeros((len(rows), 4), np.float32)
    for k, row in enumerate(rows):
        t = int(row.view(np.uint32)[2])
        w, h, first = (int(v) for v in au[4 * t:4 * t + 3])
        texels = np.ascontiguousarray(aux[4 * first:4 * (first + w * h)])
        lib.bloom_sample(fptr(texels), w, h, C.c_float(row[0]), C.c_float(row[1]), fptr(want[k]))
    bad = same_words(got, want)
    assert not len(bad), (rows[bad[0]], got[bad[0]].view(np.float32), want[bad[0]])


def test_unorm_and_pick_light_contracts(hostb):
    """unorm(v, scale) = (uint)fma(saturate(v), scale, 0.5) and pick_light(u, n) = min((uint)(u * (float)n), n - 1), restated in float64: the
    product and the sum of the first are exact in double (8 + 24 significant bits), so one rounding to fp32 is the fma; the second's product too"""
    rows, _ = build_rows("unorm", 4096, hostb)
    v, scale = rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        sat = np.where(v > 0, np.where(v > 1, 1.0, v), 0.0)  # NaN -> 0
    want = (sat * scale + 0.5).astype(np.float32).astype(np.uint32)
    assert np.array_equal(hostb.run("unorm", rows)[:, 0], want)
    assert (want <= scale.astype(np.uint32)).all()
    rows, _ = build_rows("pick_light", 4096, hostb)
    u, n = rows[:, 0].astype(np.float64), rows[:, 1].view(np.uint32).astype(np.int64)
    want = np.minimum((u * n.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.int64), n - 1)
    assert np.array_equal(hostb.run("pick_light", rows)[:, 0].astype(np.int64), want)


def test_refract_contract(hostb):
    """HLSL refract in float64: k = 1 - eta^2 (1 - c^2), c = n.i; k < 0 -> 0, else eta i - (eta c + sqrt k) n.  The fp32 k carries an absolute
    error below DK = 4e-6 (a handful of roundings of terms up to eta^2 = 5.76, one ulp of which is 4.8e-7), so within DK of 0 either
    answer is right, and elsewhere sqrt k is known to sqrt(k + DK) - sqrt(max(k - DK, 0)); the other operations add about 1e-6."""
    DK = 4e-6
    rows, _ = build_rows("refract", 4096, hostb)
    got = hostb.run("refract", rows).view(np.float32).astype(np.float64)
    i, n, eta = rows[:, 0:3].astype(np.float64), rows[:, 3:6].astype(np.float64), rows[:, 6].astype(np.float64)
    c = (n * i).sum(axis=1)
    k = 1.0 - eta * eta * (1.0 - c * c)
    ref = eta[:, None] * i - (eta * c + np.sqrt(np.maximum(k, 0.0)))[:, None] * n
    zero = (got == 0).all(axis=1)
    assert zero[k < -DK].all() and not zero[k > DK].any()
    assert (zero | (k >= -DK)).all()
    tol = np.sqrt(np.maximum(k + DK, 0.0)) - np.sqrt(np.maximum(k - DK, 0.0)) + 2e-6
    live = ~zero
    err = np.abs(got - ref).max(axis=1)
    assert (err[live] <= tol[live]).all(), (err[live] - tol[live]).max()
    assert (k < -DK).sum() > 100 and (k > DK).sum() > 100 and (np.abs(k) <= DK).sum() >= 3


def test_region_contains_contract(hostb):
    """region_contains = the origin inside O (six exact compares) and dot(d, axis) >= cos_run; the fp32 dot of two unit vectors is within
    4e-7 of the float64 one (three roundings of terms below 1), so outside that band of cos_run the decision is known"""
    rows, _ = build_rows("rg_contains", 4096, hostb)
    got = hostb.run("rg_contains", rows)[:, 0] == 1
    g, o, d = rows[:, :11], rows[:, 11:14], rows[:, 14:17]
    inside = ((o >= g[:, 0:3]) & (o <= g[:, 3:6])).all(axis=1)
    dot = (d.astype(np.float64) * g[:, 6:9]).sum(axis=1)
    assert not got[~inside].any()
    assert got[inside & (dot > g[:, 10] + 4e-7)].all() and not got[dot < g[:, 10] - 4e-7].any()
    assert got.sum() > 200 and (~got & inside).sum() > 200 and (~inside).sum() > 200


def test_beam_wrappers_match_beam_shim(hostb):
    """bm_* of leaf_batch.h (one row per box) against beam_host.cpp (one beam, a loop over boxes), bit for bit"""
    import __graft_entry__ as g

    rng = np.random.default_rng(5)
    ref = C.CDLL(g.build_beam_shim())
    mine = BeamShim(hostb, ref)
    for f in (ref.bm_make, ref.bm_meets_boxes, ref.bm_meets_leaves):
        f.restype = None
    ref.bm_make.argtypes = [F32P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, F32P]
    ref.bm_meets_boxes.argtypes = ref.bm_meets_leaves.argtypes = [F32P, C.c_uint32, F32P, C.POINTER(C.c_uint8)]
    for it in range(30):
        cam, w, h = tpb.random_camera(rng, list(tpb.LENS_CLASSES)[it % 3])
        px, py = tpb.pick_block(rng, w, h, tpb.WHERE[it % len(tpb.WHERE)])
        a, b = tpb.make_beam(mine, cam, w, h, px, py, 0.1 * (it % 2), 2.0 * (it % 3)), tpb.make_beam(ref, cam, w, h, px, py, 0.1 * (it % 2), 2.0 * (it % 3))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        boxes = tpb.scatter_boxes(rng, cam[None, :3].astype(np.float64), tpb.unit(cam[None, 9:12]), 0.0, 200)
        for leaf in (False, True):
            assert np.array_equal(tpb.meets(mine, a, boxes, leaf=leaf), tpb.meets(ref, a, boxes, leaf=leaf))


def test_region_wrappers_match_region_shim(hostb):
    """rg_* of leaf_batch.h against region_host.cpp, bit for bit (rg_lane's tanf / cosf / sinf included: the same glibc on both sides)"""
    import test_refl_region as trr

    rng = np.random.default_rng(6)
    mine, ref = RegionShim(hostb), trr.load_shim()
    for it in range(30):
        lo, hi, axis, theta = trr.random_region(rng)
        ga, gb = trr.make_region(mine, lo, hi, axis, theta), trr.make_region(ref, lo, hi, axis, theta)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
        c = 0.5 * (lo + hi)
        centres = c + np.exp(rng.uniform(np.log(0.5), np.log(80.0), 300))[:, None] * trr.cone_dirs(rng, axis, min(3.0 * theta + 0.05, 3.0), 300)
        ext = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), (300, 3)))
        boxes = np.concatenate([centres - ext, centres + ext], axis=1).astype(np.float32)
        assert np.array_equal(trr.meets(mine, ga, boxes), trr.meets(ref, ga, boxes))
    rows, _ = build_rows("rg_contains", 4096, hostb)
    for g11 in np.unique(rows[:, :11], axis=0):
        sel = rows[(rows[:, :11] == g11).all(axis=1)]
        assert np.array_equal(trr.contains(mine, g11, sel[:, 11:14], sel[:, 14:17]), trr.contains(ref, g11, sel[:, 11:14], sel[:, 14:17]))
    built = 0
    for _ in range(100):
        cam, dirs, Cs, r = trr.pyramid(rng)
        ga, gb = np.zeros(11, np.float32), np.zeros(11, np.float32)
        ka, kb = mine.rg_from_rays(trr.fp(cam), trr.fp(dirs), trr.fp(Cs), C.c_float(r), trr.fp(ga)), ref.rg_from_rays(trr.fp(cam), trr.fp(dirs), trr.fp(Cs), C.c_float(r), trr.fp(gb))
        assert ka == kb and (not ka or np.array_equal(ga.view(np.uint32), gb.view(np.uint32)))
        built += ka
        oa, La, ob, Lb = (np.zeros(3, np.float32) for _ in range(4))
        args = (trr.fp(cam), trr.fp(dirs[4]), trr.fp(Cs), C.c_float(r), C.c_float(1e-3), C.c_float(1.0))
        assert mine.rg_lane(*args, trr.fp(oa), trr.fp(La)) == ref.rg_lane(*args, trr.fp(ob), trr.fp(Lb))
        assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32)) and np.array_equal(La.view(np.uint32), Lb.view(np.uint32))
    assert built > 25


# ------------------------------------------------------------------------------------------------ the old shims' interfaces on a Batch
def _arr(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(n,))


def _val(x):
    return x.value if hasattr(x, "value") else x


class RegionShim:
    """region_host.cpp's exports (the interface test_refl_region.py's tests take), computed by a Batch: the host build or the device's."""

    def __init__(self, batch):
        self.b = batch

    def rg_make(self, lo, hi, axis, theta, g):
        _arr(g, 11)[:] = self.b.run("rg_make", np.concatenate([_arr(lo, 3), _arr(hi, 3), _arr(axis, 3), [f32(_val(theta))]])[None]).view(np.float32)[0]

    def _per_element(self, name, g, n, items, out):
        rows = np.concatenate([np.tile(_arr(g, 11), (n, 1)), _arr(items, 6 * n).reshape(n, 6)], axis=1)
        _arr(out, n)[:] = self.b.run(name, rows)[:, 0]

    def rg_meets_boxes(self, g, n, boxes, out):
        self._per_element("rg_meets_box", g, n, boxes, out)

    def rg_contains(self, g, n, rays, out):
        self._per_element("rg_contains", g, n, rays, out)

    def rg_from_rays(self, cam_o, dirs, Cs, r, g):
        res = self.b.run("rg_from_rays", np.concatenate([_arr(cam_o, 3), _arr(dirs, 15), _arr(Cs, 3), [f32(_val(r))]])[None])[0]
        if res[0]:
            _arr(g, 11)[:] = res[1:].view(np.float32)
        return int(res[0])

    def rg_lane(self, cam_o, d, Cs, r, tilt, phi, o, L):
        res = self.b.run("rg_lane", np.concatenate([_arr(cam_o, 3), _arr(d, 3), _arr(Cs, 3), f32([_val(r), _val(tilt), _val(phi)])])[None])[0]
        if res[0]:
            _arr(o, 3)[:] = res[1:4].view(np.float32); _arr(L, 3)[:] = res[4:7].view(np.float32)
        return int(res[0])


class BeamShim:
    """beam_host.cpp's device half (bm_make, bm_meets_boxes, bm_meets_leaves) computed by a Batch; the camera rays and the sphere hits the
    properties are judged with (bm_rays, bm_hits: pt_bsdf.h / pt_math.h, not pt_beam.h) stay with beam_host.cpp."""

    def __init__(self, batch, beam_host):
        self.b, self.bm_rays, self.bm_hits = batch, beam_host.bm_rays, beam_host.bm_hits
        self.bm_rays.argtypes = [F32P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), F32P, F32P, F32P, F32P]
        self.bm_hits.argtypes = [C.c_uint32, F32P, F32P, C.c_uint32, F32P, C.POINTER(C.c_uint8)]
        self.bm_rays.restype = self.bm_hits.restype = None

    def bm_make(self, cam, w, h, px, py, slack, margin, g):
        row = np.concatenate([_arr(cam, 12), np.uint32([w, h, px, py]).view(np.float32), f32([_val(slack), _val(margin)])])
        _arr(g, 16)[:] = self.b.run("bm_make", row[None]).view(np.float32)[0]

    def _per_element(self, name, g, n, boxes, out):
        rows = np.concatenate([np.tile(_arr(g, 16), (n, 1)), _arr(boxes, 6 * n).reshape(n, 6)], axis=1)
        _arr(out, n)[:] = self.b.run(name, rows)[:, 0]

    def bm_meets_boxes(self, g, n, boxes, out):
        self._per_element("bm_meets_box", g, n, boxes, out)

    def bm_meets_leaves(self, g, n, boxes, out):
        self._per_element("bm_meets_leaf", g, n, boxes, out)


# ------------------------------------------------------------------------------------------------ accuracy against float64
SWEEP = 1 << 22
# Largest errors of log2_spec and exp2_spec against float64, measured by test_spec_accuracy_dense_sweep on the host build (the device build
# is bit-identical: tests/test_gpu_leaf_edges.py); the bounds are twice the measured values.  DESIGN.md section 4 carries the same numbers.
#   log2_spec: 2^22 points x = 2^e (1 + j / 2^22), e cycling through [-126, 127] and j a permutation, plus b_log2's edge table;
#              max |log2_spec(x) - log2 x| / max(|log2 x|, 1) = 8.6242e-08
#   exp2_spec: 2^22 points y evenly spaced over [-126.5, 127.49] plus b_exp2's edge table; max relative error of the normal results = 7.7195e-08
#              (a subnormal result is that value rounded once more to the 2^-149 grid: within 0.5 + EXP2_BOUND * 2^23 units; measured 0.90)
LOG2_MEASURED = 8.6242e-08
EXP2_MEASURED = 7.7195e-08
LOG2_BOUND, EXP2_BOUND = 2 * LOG2_MEASURED, 2 * EXP2_MEASURED


def test_spec_accuracy_dense_sweep(hostb):
    rng = np.random.default_rng(9)
    i = np.arange(SWEEP, dtype=np.float64)
    # sincos_2pi: 5e-7 absolute (tests/test_oracle_kat.py::test_sincos_pow_accuracy), over [0, 1]
    u = np.concatenate([(i / SWEEP).astype(np.float32), build_rows("sincos_2pi", 0, hostb)[0][:, 0]])
    sc = hostb.run("sincos_2pi", u).view(np.float32).astype(np.float64)
    ang = 2 * np.pi * u.astype(np.float64)
    err_s, err_c = np.abs(sc[:, 0] - np.sin(ang)).max(), np.abs(sc[:, 1] - np.cos(ang)).max()
    print(f"sincos_2pi: max |sin err| {err_s:.3e} |cos err| {err_c:.3e}")
    # pow_spec(x, 2.4): 2e-6 relative, floored at 1e-3 of the value's scale (the same test), x over [0.02, 1]
    x = np.concatenate([(0.02 + 0.98 * i / (SWEEP - 1)).astype(np.float32), f32([0.02, 1.0, ONE_M, (0.04045 + 0.055) / 1.055])])
    p = hostb.run("pow", np.stack([x, np.full(len(x), 2.4, np.float32)], axis=1)).view(np.float32)[:, 0].astype(np.float64)
    ref = x.astype(np.float64) ** 2.4
    err_p = (np.abs(p - ref) / np.maximum(ref, 1e-3)).max()
    print(f"pow_spec(x, 2.4): max relative error {err_p:.3e}")
    # atan2_spec: 3e-5 rad (tests/test_textures.py::test_atan2_accuracy_and_parity), angles all round with magnitudes from 1e-18 to 1e18, and the
    # edge table (axes, signed zeros, subnormals, 1e-30 against 1e30, FLT_MAX)
    th = 2 * np.pi * i / SWEEP
    mag = np.exp(rng.uniform(np.log(1e-18), np.log(1e18), SWEEP))
    yx = np.concatenate([np.stack([np.sin(th) * mag, np.cos(th) * mag], axis=1).astype(np.float32), build_rows("atan2", 0, hostb)[0]])
    a = hostb.run("atan2", yx).view(np.float32)[:, 0].astype(np.float64)
    ref = np.arctan2(yx[:, 0].astype(np.float64), yx[:, 1].astype(np.float64))
    err = np.abs(a - ref); err = np.minimum(err, 2 * np.pi - err)
    err[(yx[:, 0] == 0) & (yx[:, 1] == 0)] = 0  # atan2(+-0, +-0) is defined as 0 here
    err_a = err.max()
    print(f"atan2_spec: max error {err_a:.3e} rad")
    # log2_spec: absolute error, every binade
    e = (np.arange(SWEEP) % 254) - 126
    xl = np.concatenate([np.ldexp(1.0 + rng.permutation(SWEEP) / SWEEP, e).astype(np.float32), build_rows("log2", 0, hostb)[0][:, 0]])
    xl = xl[np.isfinite(xl)]
    lg = hostb.run("log2", xl).view(np.float32)[:, 0].astype(np.float64)
    refl = np.log2(xl.astype(np.float64))
    err_l = (np.abs(lg - refl) / np.maximum(np.abs(refl), 1.0)).max()
    print(f"log2_spec: max error relative to max(|log2 x|, 1) {err_l:.4e}")
    # exp2_spec: relative error where the result is a normal number
    y = np.concatenate([(-126.5 + 253.99 * i / (SWEEP - 1)).astype(np.float32), build_rows("exp2", 0, hostb)[0][:, 0]])
    ex = hostb.run("exp2", y).view(np.float32)[:, 0].astype(np.float64)
    refe = np.exp2(y.astype(np.float64))
    normal = refe >= float(FLT_MIN)
    err_e = (np.abs(ex - refe) / refe)[normal].max()
    err_sub = (np.abs(ex - refe)[~normal]).max() / float(SUB_MIN)
    print(f"exp2_spec: max relative error (normal results) {err_e:.4e}; subnormal results within {err_sub:.2f} units of 2^-149")
    assert err_s < 5e-7 and err_c < 5e-7, (err_s, err_c)
    assert err_p <= 2e-6, err_p
    assert err_a < 3e-5, err_a
    assert err_l <= LOG2_BOUND, err_l
    assert err_e <= EXP2_BOUND, err_e
    assert err_sub <= 0.5 + EXP2_BOUND * 2.0 ** 23, err_sub


# ------------------------------------------------------------------------------------------------ pt_beam.h with beam_rsq one float off
@pytest.mark.parametrize("ulps", [-1, 1])
def test_p1_holds_with_beam_rsq_one_ulp_off(hostb, ulps):
    """Property P1 of test_primary_beams.py (rejected boxes and leaves are never hit, float64 brute force; its own floors on what is culled)
    with the planes' normalisation one float below / above the host's value: the error class of the device's instruction."""
    import __graft_entry__ as g

    hostb.lib.lbh_set_beam_rsq_ulps(ulps)
    try:
        shim = BeamShim(hostb, C.CDLL(g.build_beam_shim()))
        cam, w, h = tpb.random_camera(np.random.default_rng(1), "normal")
        moved = tpb.make_beam(shim, cam, w, h, 0, 0, 0.0, 0.0)
        hostb.lib.lbh_set_beam_rsq_ulps(0)
        exact = tpb.make_beam(shim, cam, w, h, 0, 0, 0.0, 0.0)
        assert not np.array_equal(moved.view(np.uint32), exact.view(np.uint32)), "the shift does not reach make_beam"
        hostb.lib.lbh_set_beam_rsq_ulps(ulps)
        tpb.test_p1_rejected_boxes_and_leaves_are_never_hit(shim)
    finally:
        hostb.lib.lbh_set_beam_rsq_ulps(0)


# ------------------------------------------------------------------------------------------------ the device build's floating-point environment
def test_device_code_keeps_fp32_subnormals(tmp_path):
    """DESIGN.md section 4, "Floating-point environment": every kernel of the gfx950 build of leaf_batch.h (the product's compiler and flags)
    and of one product translation unit has float_denorm_mode_32 = 3 (subnormal operands and results kept), read from the assembly."""
    import __graft_entry__ as g

    cmd = g.hipcc_command()
    if shutil.which(cmd[0]) is None and not os.path.exists(cmd[0]):
        pytest.skip(f"{cmd[0]} is not installed")
    here = os.path.dirname(os.path.abspath(__file__))
    for src in (os.path.join(here, "hostshim", "leaf_batch_gpu.hip"), os.path.join(g.PKG, "csrc", "pt_bloom.hip")):
        asm = str(tmp_path / (os.path.basename(src) + ".s"))
        subprocess.run([*cmd, "--cuda-device-only", "-S", "-o", asm, src], check=True)
        modes = [line.split()[1] for line in open(asm) if line.strip().startswith(".amdhsa_float_denorm_mode_32")]
        assert modes and set(modes) == {"3"}, (src, sorted(set(modes)), len(modes))
