"""CPU: the primary-beam headers (csrc/pt_beam.h: the pyramid of an 8x8 block and its box tests; csrc/pt_beam_cache.h: which later poses may use
a pyramid's lists, and the planner of a moving camera's next lists), compiled as host C++ by tests/hostshim/beam_host.cpp, against float64
brute force.  Rays are the product's own fp32 camera rays (primary_ray); everything judged about them is judged in float64.  Every property
is exact and one-sided: zero exceptions, no tolerance.
- P1: a box beam_meets_box rejects is met by no ray of the block (any jitter, any position within the slack); a leaf beam_meets_leaf rejects
  holds no sphere a ray hits; NaN and infinite boxes are never rejected.
- P2: a pose beam_within accepts has every pixel ray cross the lists' image plane within margin_px of its block's outline, and P1 holds for
  its rays against the lists' pyramids.
- P3: the same for bases that are not rotations of one another (lens shift, shear, axis lengths, mirror, half turn, degenerate axes):
  refused, or contained.
- P4: one directed case per constant of beam_within.
- P5: the lists beam_plan plans are accepted for every frame of the span they are planned for.
Leaves: beam_meets_leaf tests the ball around the box centre with the LARGEST half extent as radius (pt_beam.h; the tree builders make every
leaf box the padded cube around its sphere, pt_lbvh.cpp), so the spheres a rejected leaf is searched for are those inside that ball -- a
sphere tucked into a cube's corner fits the box but not the ball, and no builder makes one.
The device variant of pt_beam.h (beam_rsq is an instruction there) is tested in test_leaf_edges.py (one ulp either way) and test_gpu_leaf_edges.py."""
import ctypes as C

import numpy as np
import pytest

F32P, U8P, U32P, F64P = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
U32, F32, F64 = C.c_uint32, C.c_float, C.c_double


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_beam_shim())
    lib.bm_make.argtypes = [F32P, U32, U32, U32, U32, F32, F32, F32P]
    lib.bm_meets_boxes.argtypes = [F32P, U32, F32P, U8P]
    lib.bm_meets_leaves.argtypes = [F32P, U32, F32P, U8P]
    lib.bm_rays.argtypes = [F32P, U32, U32, U32, U32P, F32P, F32P, F32P, F32P]
    lib.bm_hits.argtypes = [U32, F32P, F32P, U32, F32P, U8P]
    lib.bc_lens.argtypes = [U32, U32, F32P, F64P]
    lib.bc_rotation_between.argtypes = [F32P, F32P, F64P]
    lib.bc_rotation_between.restype = F64
    lib.bc_turn_px.argtypes = [U32, U32, F32P, F64]
    lib.bc_turn_px.restype = F64
    lib.bc_lens_px.argtypes = [U32, U32, F32P, F32P, F32P]
    lib.bc_lens_px.restype = F64
    lib.bc_same_lens.argtypes = [U32, U32, F32P, F32P, F32P]
    lib.bc_same_lens.restype = C.c_int
    lib.bc_within.argtypes = [U32, U32, F32P, F32P, F32, F32, F32P, F32P]
    lib.bc_within.restype = C.c_int
    lib.bc_ahead.argtypes = [F32P, F64P, F32P, F64P, F64, F64, F32P, F32P]
    lib.bc_plan.argtypes = [U32, U32, F32P] + [F64] * 9 + [F64P]
    for f in (lib.bm_make, lib.bm_meets_boxes, lib.bm_meets_leaves, lib.bm_rays, lib.bm_hits, lib.bc_lens, lib.bc_ahead, lib.bc_plan):
        f.restype = None
    return lib


def fp(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(F32P)


def dp(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(F64P)


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rotation(axis, angle):
    """float64 rotation matrix (Rodrigues)"""
    k = unit(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


# ------------------------------------------------------------------------------------------------ the shim's functions on numpy arrays
def make_beam(lib, cam, w, h, px, py, slack, margin):
    g = np.zeros(16, np.float32)
    lib.bm_make(fp(cam), w, h, px, py, F32(slack), F32(margin), fp(g))
    return g


def meets(lib, g, boxes, leaf=False):
    boxes = c32(boxes)
    out = np.zeros(len(boxes), np.uint8)
    (lib.bm_meets_leaves if leaf else lib.bm_meets_boxes)(fp(g), len(boxes), fp(boxes), out.ctypes.data_as(U8P))
    return out.astype(bool)


def rays(lib, cam, w, h, pix, jit, pos=None):
    """The kernels' fp32 rays (primary_ray) as float64 arrays: pixel pix[i] with jitter jit[i] from pos[i] (None: the camera's position)."""
    pix = np.ascontiguousarray(pix, dtype=np.uint32)
    jit = c32(jit)
    n = len(pix)
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    lib.bm_rays(fp(cam), w, h, n, pix.ctypes.data_as(U32P), fp(jit), fp(c32(pos)) if pos is not None else None, fp(o), fp(d))
    return o, d


def dev_hits(lib, o, d, sph):
    out = np.zeros((len(o), len(sph)), np.uint8)
    lib.bm_hits(len(o), fp(o), fp(d), len(sph), fp(c32(sph)), out.ctypes.data_as(U8P))
    return out.astype(bool)


def within(lib, w, h, b, slack, margin, q):
    """b, q: cameras of 12 floats (Position, Right, Up, Forward); the lens is q's, as in beam_cache_lookup"""
    return bool(lib.bc_within(w, h, fp(b[:3]), fp(b[3:]), F32(slack), F32(margin), fp(q[:3]), fp(q[3:])))


def bound_px(lib, w, h, b, q):
    """turn_px + lens_px of the pair, as beam_within adds them for bases that are rotations of one another"""
    rot = np.zeros(3)
    ang = lib.bc_rotation_between(fp(b[3:]), fp(q[3:]), dp(rot))
    return lib.bc_turn_px(w, h, fp(q[3:]), ang) + lib.bc_lens_px(w, h, fp(q[3:]), fp(b[3:]), fp(q[3:]))


def least_margin(lib, w, h, b, q):
    """the smallest margin_px with which beam_within accepts the pair (same position), by bisection on beam_within itself; inf: none does"""
    lo, hi = 0.0, 1e9
    if not within(lib, w, h, b, 0.0, hi, q):
        return np.inf
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if within(lib, w, h, b, 0.0, mid, q) else (mid, hi)
    return float(np.float32(hi * (1.0 + 1e-6)))


# ------------------------------------------------------------------------------------------------ float64 references
def slab_hits(o, d, lo, hi):
    """float64: does ray i (o[i] + t d[i], t >= 0) meet box j?  -> (n_rays, n_boxes)"""
    o, d = o[:, None, :], d[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0, t1 = (lo[None] - o) * inv, (hi[None] - o) * inv
    tn = np.nanmax(np.minimum(t0, t1), axis=-1)
    tf = np.nanmin(np.maximum(t0, t1), axis=-1)
    return np.maximum(tn, 0.0) <= tf


def sphere_hits(o, d, sph):
    """float64: does ray i meet sphere j at some t >= 0?  -> (n_rays, n_spheres)"""
    f = o[:, None, :] - sph[None, :, :3]
    dd = (d * d).sum(-1)[:, None]
    b = (f * d[:, None, :]).sum(-1)
    c = (f * f).sum(-1) - sph[None, :, 3] ** 2
    disc = b * b - dd * c
    with np.errstate(invalid="ignore"):
        return (disc >= 0) & (-b + np.sqrt(np.maximum(disc, 0)) >= 0)


def crossing_px(basis, d, w, h):
    """float64: where direction d crosses the image plane of the camera with axes basis (rows Right, Up, Forward), in pixels; inf behind it"""
    c = np.linalg.solve(basis.astype(np.float64).T, d.astype(np.float64).T).T
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(c[:, 2] > 0, (c[:, 0] / c[:, 2] + 1.0) * 0.5 * w, np.inf)
        y = np.where(c[:, 2] > 0, (1.0 - c[:, 1] / c[:, 2]) * 0.5 * h, np.inf)
    return x, y


# ------------------------------------------------------------------------------------------------ generators
LENS_CLASSES = {"narrow": (10.0, 30.0), "normal": (30.0, 100.0), "wide": (100.0, 150.0)}


def random_camera(rng, cls, far=False):
    """(cam[12] fp32, w, h): a random orientation and position, HFOV of the class, aspect 1:4 to 4:1, sizes mostly not multiples of 8, and for
    a third of the cameras pixels that are not square"""
    hfov = np.radians(rng.uniform(*LENS_CLASSES[cls]))
    aspect = float(np.exp(rng.uniform(np.log(0.25), np.log(4.0))))
    w = int(rng.integers(40, 400))
    h = max(9, int(round(w / aspect)))
    if h > 400:
        h, w = 400, max(9, int(round(400 * aspect)))
    Rm = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
    lf = float(np.exp(rng.uniform(np.log(0.5), np.log(2.0))))
    lr = lf * np.tan(0.5 * hfov)
    lu = lr * h / w * (rng.uniform(0.6, 1.6) if rng.random() < 1 / 3 else 1.0)
    pos = rng.uniform(-20, 20, 3) * (1e3 if far else 1.0)
    cam = np.concatenate([pos, Rm[0] * lr, Rm[1] * lu, Rm[2] * lf])
    return c32(cam), w, h


def pick_block(rng, w, h, where):
    bx, by = (w - 1) // 8, (h - 1) // 8  # last block of each axis (partial when the size is not a multiple of 8)
    ix, iy = {"c00": (0, 0), "c10": (bx, 0), "c11": (bx, by), "c01": (0, by), "top": (rng.integers(0, bx + 1), 0), "bottom": (rng.integers(0, bx + 1), by),
              "left": (0, rng.integers(0, by + 1)), "right": (bx, rng.integers(0, by + 1)), "inside": (rng.integers(0, bx + 1), rng.integers(0, by + 1))}[where]
    return int(ix) * 8, int(iy) * 8


WHERE = ["c00", "c10", "c11", "c01", "top", "bottom", "left", "right", "inside"]
JIT_CORNERS = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])


def block_samples(rng, w, h, px, py, n):
    """n (pixel, jitter) samples of the block's valid pixels: its four corner pixels at the jitter square's corners first"""
    x1, y1 = min(px + 7, w - 1), min(py + 7, h - 1)
    pix = np.stack([rng.integers(px, x1 + 1, n), rng.integers(py, y1 + 1, n)], axis=1)
    jit = rng.uniform(-0.5, 0.5, (n, 2))
    k = 0
    for cx, cy in ((px, py), (x1, py), (x1, y1), (px, y1)):
        for j in JIT_CORNERS:
            pix[k] = (cx, cy); jit[k] = j; k += 1
    return pix, jit


def positions_within(rng, centre, slack, n):
    """n fp32 positions within slack * (1 - 1e-4) of the fp32 centre (judged in float64, as beam_within does), a third of them on that sphere"""
    if slack == 0.0:
        return np.tile(centre, (n, 1))
    r = slack * (1.0 - 1e-4) * np.where(rng.random(n) < 1 / 3, 1.0, rng.random(n) ** (1 / 3))
    p = c32(centre.astype(np.float64) + unit(rng.normal(size=(n, 3))) * r[:, None])
    for _ in range(4):  # rounding to fp32 may have pushed a point outside: pull those in
        out = np.linalg.norm(p.astype(np.float64) - centre, axis=1) > slack * (1.0 - 1e-4)
        if not out.any():
            break
        p[out] = c32(centre + (p[out].astype(np.float64) - centre) * (1.0 - 3e-7))
    out = np.linalg.norm(p.astype(np.float64) - centre, axis=1) > slack * (1.0 - 1e-4)
    p[out] = centre
    return p


def scatter_boxes(rng, o, d, slack, n):
    """n fp32 boxes around the bundle of rays (o, d): centres 0.5 to 1e6 from the apex, extents 1e-3 to 1e3, most of them within a few widths of
    the bundle's outline"""
    axis = unit(d.mean(axis=0))
    spread = float(np.arccos(np.clip((unit(d) @ axis).min(), -1, 1)))  # the bundle's half angle
    dist = np.exp(rng.uniform(np.log(0.5), np.log(1e6), n))
    ext = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 3)))
    ext *= np.minimum(1.0, dist / np.linalg.norm(ext, axis=1))[:, None] * rng.choice([1.0, 0.1, 0.01], (n, 1))
    perp = unit(np.cross(axis, rng.normal(size=(n, 3))))
    off = np.tan(np.minimum(spread * rng.uniform(0.0, 3.0, n), 1.4)) * dist
    off = off + (np.linalg.norm(ext, axis=1) + slack) * rng.uniform(0.0, 1.6, n)
    centre = o.mean(axis=0) + dist[:, None] * axis + off[:, None] * perp
    return c32(np.concatenate([centre - ext, centre + ext], axis=1))


def leaf_boxes(rng, boxes):
    """The builders' leaf boxes around spheres at the boxes' centres: the padded cube c -+ (r + pad) in fp32; every fourth box is left as it is"""
    b = boxes.astype(np.float64)
    c, r = c32(0.5 * (b[:, :3] + b[:, 3:])), c32(0.5 * (b[:, 3:] - b[:, :3]).min(axis=1))
    pad = c32(r * rng.choice([0.0, 1e-6, 1e-3], len(r)))
    cube = np.concatenate([c - r[:, None] - pad[:, None], c + r[:, None] + pad[:, None]], axis=1).astype(np.float32)
    keep = rng.random(len(boxes)) < 0.25
    return np.where(keep[:, None], boxes, cube)


def spheres_in_leaf(rng, box, n):
    """n fp32 spheres inside the ball beam_meets_leaf tests (box centre, largest half extent): the ball itself first, then smaller ones anywhere in it"""
    b = box.astype(np.float64)
    c, R = 0.5 * (b[:3] + b[3:]), 0.5 * (b[3:] - b[:3]).max()
    r = R * np.concatenate([[1.0], rng.random(n - 1)])
    cc = c + unit(rng.normal(size=(n, 3))) * ((R - r) * rng.random(n))[:, None]
    s = c32(np.concatenate([cc, r[:, None]], axis=1))
    for _ in range(3):  # fp32 rounding: shrink what pokes out of the ball
        out = np.linalg.norm(s[:, :3].astype(np.float64) - c, axis=1) + s[:, 3] > R
        s[out, 3] = np.maximum(s[out, 3] * np.float32(1.0 - 1e-6) - np.float32(1e-7 * np.abs(c).max()), 0).astype(np.float32)
    ok = np.linalg.norm(s[:, :3].astype(np.float64) - c, axis=1) + s[:, 3] <= R
    return s[ok & (s[:, 3] > 0)]


def check_beam(lib, rng, g, o32, d32, slack, n_boxes=160):
    """P1's two assertions for the fp32 rays (o32, d32) against beam g; returns (rejected boxes, rejected leaves)"""
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    boxes = scatter_boxes(rng, o, d, slack, n_boxes)
    rej = boxes[~meets(lib, g, boxes)].astype(np.float64)
    if len(rej):
        hit = slab_hits(o, d, rej[:, :3], rej[:, 3:])
        assert not hit.any(), f"a ray of the block meets a box beam_meets_box rejected: ray {np.argwhere(hit)[0]}, box {rej[np.argwhere(hit)[0][1]]}"
    leaves = leaf_boxes(rng, boxes)
    lrej = leaves[~meets(lib, g, leaves, leaf=True)]
    for box in lrej[:24]:
        sph = spheres_in_leaf(rng, box, 6)
        if not len(sph):
            continue
        assert not sphere_hits(o, d, sph.astype(np.float64)).any(), f"a ray hits a sphere of a leaf beam_meets_leaf rejected (float64): {box}"
        assert not dev_hits(lib, o32, d32, sph).any(), f"a ray hits a sphere of a leaf beam_meets_leaf rejected (intersect_sphere): {box}"
    return len(rej), len(lrej)


# ------------------------------------------------------------------------------------------------ P1
def test_p1_rejected_boxes_and_leaves_are_never_hit(shim):
    rng = np.random.default_rng(11)
    n_box = {k: 0 for k in LENS_CLASSES}
    n_leaf = 0
    for it in range(135):
        cls = list(LENS_CLASSES)[it % 3]
        cam, w, h = random_camera(rng, cls, far=(it % 5 == 4))
        px, py = pick_block(rng, w, h, WHERE[(it // 3) % len(WHERE)])
        slack = 0.0 if it % 4 == 0 else float(np.exp(rng.uniform(np.log(1e-4), np.log(2.0))))
        margin = 0.0 if it % 3 == 1 else float(rng.uniform(0.05, 8.0))
        g = make_beam(shim, cam, w, h, px, py, slack, margin)
        pix, jit = block_samples(rng, w, h, px, py, 96)
        o, d = rays(shim, cam, w, h, pix, jit, positions_within(rng, cam[:3], slack, len(pix)))
        nb, nl = check_beam(shim, rng, g, o, d, slack)
        # the pyramid is a whole pixel wider than the block's pixel centres (half a pixel for the jitter, half a pixel of slack: pt_beam.h):
        # rays up to 0.99 pixels off their centres stay inside
        o2, d2 = rays(shim, cam, w, h, pix, 1.98 * jit, positions_within(rng, cam[:3], slack, len(pix)))
        check_beam(shim, rng, g, o2, d2, slack, n_boxes=80)
        n_box[cls] += nb
        n_leaf += nl
    print("P1 rejected:", n_box, n_leaf)
    # the tests cull (seen: narrow 3370, normal 4967, wide 4273 boxes; 13804 leaves)
    assert sum(n_box.values()) >= 5000 and n_leaf >= 1000 and min(n_box.values()) >= 100, (n_box, n_leaf)


def test_p1_nan_and_infinite_boxes_are_never_rejected(shim):
    rng = np.random.default_rng(12)
    bad = [np.nan, np.inf, -np.inf]
    for it in range(30):
        cam, w, h = random_camera(rng, list(LENS_CLASSES)[it % 3])
        px, py = pick_block(rng, w, h, WHERE[it % len(WHERE)])
        g = make_beam(shim, cam, w, h, px, py, float(rng.choice([0.0, 0.3])), float(rng.choice([0.0, 2.0])))
        boxes = scatter_boxes(rng, cam[None, :3].astype(np.float64), unit(cam[None, 9:12]), 0.0, 64)
        finite_rejected = ~meets(shim, g, boxes)
        assert finite_rejected.any()  # (these boxes are ones the beam culls while finite)
        all_nan = np.full((1, 6), np.nan, np.float32)
        assert meets(shim, g, all_nan).all() and meets(shim, g, all_nan, leaf=True).all()
        # one NaN coordinate spoils at least the plane tests that read it; a whole NaN corner every test
        for k in range(len(boxes)):
            b = boxes[k].copy()
            b[:3] = np.nan
            b[3:] = rng.choice(bad, 3)
            boxes[k] = b
        assert meets(shim, g, boxes).all(), "a box with NaN / infinite corners was rejected"
        assert meets(shim, g, boxes, leaf=True).all(), "a leaf with NaN / infinite corners was rejected"
        inf_box = np.array([[-np.inf] * 3 + [np.inf] * 3], np.float32)  # all of space
        assert meets(shim, g, inf_box).all() and meets(shim, g, inf_box, leaf=True).all()


# ------------------------------------------------------------------------------------------------ P2 / P3
def image_samples(rng, w, h, n):
    """(pixel, jitter) samples over the whole image: the four corner pixels at the jitter square's corners, the edges, then anywhere"""
    pix = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)
    jit = rng.uniform(-0.5, 0.5, (n, 2))
    k = 0
    for cx, cy in ((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)):
        for j in JIT_CORNERS:
            pix[k] = (cx, cy); jit[k] = j; k += 1
    pix[k:k + 4, 0] = (0, w - 1, 0, w - 1)  # edge pixels at random heights
    return pix, jit


def displacement(lib, w, h, b, q, pix, jit):
    """(worst distance in pixels, per axis, of q's rays' crossings of b's image plane beyond their own blocks' outlines widened by half a pixel;
    worst displacement from where b's rays of the same pixels cross) -- float64 over the product's fp32 rays"""
    _, dq = rays(lib, q, w, h, pix, jit)
    x, y = crossing_px(b[3:].reshape(3, 3), dq, w, h)
    bx, by = pix[:, 0] - pix[:, 0] % 8, pix[:, 1] - pix[:, 1] % 8
    outside = np.max([bx - 0.5 - x, x - (bx + 8.5), by - 0.5 - y, y - (by + 8.5)])
    own = np.stack([pix[:, 0] + 0.5 + jit[:, 0], pix[:, 1] + 0.5 + jit[:, 1]], axis=1)
    moved = np.max(np.abs(np.stack([x, y], axis=1) - own))
    return outside, moved


def check_pose_against_lists(lib, rng, w, h, b, slack, margin, q, n_blocks=2):
    """P1's assertions for q's rays (q turned, and anywhere within the slack) against make_beam(b, ...) of a few blocks"""
    for where in rng.choice(WHERE, n_blocks, replace=False):
        px, py = pick_block(rng, w, h, where)
        g = make_beam(lib, b, w, h, px, py, slack, margin)
        pix, jit = block_samples(rng, w, h, px, py, 48)
        o, d = rays(lib, q, w, h, pix, jit, positions_within(rng, b[:3], slack, len(pix)))
        check_beam(lib, rng, g, o, d, slack, n_boxes=80)


def turned(b, Rm, rng=None):
    """camera b with its axes turned by the float64 rotation Rm, rounded to fp32"""
    q = b.copy()
    q[3:] = c32((b[3:].astype(np.float64).reshape(3, 3) @ Rm.T).ravel())
    return q


def angle_for(lib, w, h, b, px):
    """the turn whose turn_px is about px pixels (first order)"""
    return px / lib.bc_turn_px(w, h, fp(b[3:]), 1e-9) * 1e-9


def test_p2_accepted_turns_keep_every_ray_inside_its_widened_block(shim):
    rng = np.random.default_rng(21)
    n_acc = n_ref = n_tight = 0
    for it in range(5200):
        cls = list(LENS_CLASSES)[it % 3]
        b, w, h = random_camera(rng, cls)
        margin = float(rng.uniform(0.05, 8.0))
        slack = 0.0 if it % 2 else float(np.exp(rng.uniform(np.log(1e-4), np.log(2.0))))
        kind = it % 4
        ratio = rng.uniform(0.85, 1.15) if rng.random() < 0.6 else rng.uniform(0.05, 1.6)  # of the margin: most decisions are close ones
        ang = angle_for(shim, w, h, b, ratio * margin)
        if kind == 0:    # a true rotation about any axis
            q = turned(b, rotation(rng.normal(size=3), ang))
        elif kind == 1:  # a roll about the view axis
            q = turned(b, rotation(b[9:12].astype(np.float64), ang * rng.choice([-1, 1])))
        elif kind == 2:  # beam_ahead's extrapolation of a real turn: axes re-rounded to fp32, their lengths an ulp off
            f = float(rng.integers(2, 40))
            b1 = turned(b, rotation(rng.normal(size=3), ang / f))
            rot = np.zeros(3)
            t = shim.bc_rotation_between(fp(b[3:]), fp(b1[3:]), dp(rot))
            q = b.copy()
            shim.bc_ahead(fp(b1[:3]), dp(np.zeros(3)), fp(b1[3:]), dp(rot), t, f, fp(q[:3]), fp(q[3:]))
        else:            # the same orientation but for rounding: a margin that small refuses or accepts on lens_px alone
            q = b.copy()
            q[3:] = np.nextafter(b[3:], rng.choice([-np.inf, np.inf], 9).astype(np.float32))
            margin = float(np.exp(rng.uniform(np.log(1e-4), np.log(0.5))))
        q[:3] = positions_within(rng, b[:3], slack, 1)[0]
        if not within(shim, w, h, b, slack, margin, q):
            n_ref += 1
            continue
        n_acc += 1
        n_tight += bound_px(shim, w, h, b, q) > 0.9 * margin
        pix, jit = image_samples(rng, w, h, 40)
        outside, _ = displacement(shim, w, h, b, q, pix, jit)
        assert outside <= margin, f"an accepted pose's ray leaves its widened block by {outside} px > margin {margin} (kind {kind}, {cls})"
        if n_acc % 12 == 0:
            check_pose_against_lists(shim, rng, w, h, b, slack, margin, q)
    print("P2 accepted / refused / above 0.9 of the margin:", n_acc, n_ref, n_tight)
    # (seen: 2880 accepted, 2320 refused, 753 of the accepted above 0.9 of their margin)
    assert n_acc >= 2000 and n_ref >= 2000 and n_tight >= n_acc / 4, (n_acc, n_ref, n_tight)


def sheared(rng, b, kind, eps):
    q = b.copy()
    R, U, Fw = (b[3:6].astype(np.float64), b[6:9].astype(np.float64), b[9:12].astype(np.float64))
    if kind == "shift_x":
        Fw = Fw + eps * R
    elif kind == "shift_y":
        Fw = Fw + eps * U
    elif kind == "skew":
        U = U + eps * R
    elif kind == "lengths":
        s = 1.0 + eps * rng.choice([-1, 0, 1], 3)
        if not s.any():
            s[0] = 1.0 + eps
        R, U, Fw = R * s[0], U * s[1], Fw * s[2]
    elif kind == "mirror":
        R = -R
    elif kind == "half_turn":
        R, Fw = -R, -Fw
    q[3:] = c32(np.concatenate([R, U, Fw]))
    return q


def test_p3_bases_that_are_not_rotations_are_refused_or_contained(shim):
    rng = np.random.default_rng(31)
    kinds = ["shift_x", "shift_y", "skew", "lengths", "mirror", "half_turn"]
    n_real = {k: 0 for k in kinds}
    n_acc = 0
    for it in range(2400):
        cls = list(LENS_CLASSES)[it % 3]
        kind = kinds[(it // 3) % len(kinds)]
        b, w, h = random_camera(rng, cls)
        margin = float(rng.uniform(0.05, 8.0))
        # a shear worth 1e-3 to 30 margins: eps moves the crossings by about eps half-widths of the image
        eps = float(np.exp(rng.uniform(np.log(1e-3), np.log(30.0)))) * margin / (0.5 * min(w, h))
        q = sheared(rng, b, kind, eps)
        if it % 2:  # on top of a turn worth part of the margin
            q = sheared(rng, turned(b, rotation(rng.normal(size=3), angle_for(shim, w, h, b, rng.uniform(0.0, 0.9) * margin))), kind, eps)
        pix, jit = image_samples(rng, w, h, 40)
        outside, moved = displacement(shim, w, h, b, q, pix, jit)
        n_real[kind] += moved > margin
        if within(shim, w, h, b, 0.0, margin, q):
            n_acc += 1
            assert outside <= margin, f"{kind} (eps {eps}, {cls}): accepted, but a ray leaves its widened block by {outside} px > margin {margin}"
    shears = n_real["shift_x"] + n_real["shift_y"] + n_real["skew"]
    print("P3 beyond the margin:", n_real, "accepted:", n_acc)
    # refusals are real decisions (seen: 453 sheared pairs beyond their margin, 148 length changes, 399 mirrors, 399 half turns), and small ones are still accepted (seen: 526)
    assert shears >= 200 and n_real["lengths"] >= 50 and n_real["mirror"] >= 50 and n_real["half_turn"] >= 50 and n_acc >= 100, (n_real, n_acc)


def test_p3_degenerate_axes_are_refused(shim):
    rng = np.random.default_rng(32)
    for it in range(60):
        b, w, h = random_camera(rng, list(LENS_CLASSES)[it % 3])
        for bad in (0.0, np.nan, np.inf, -np.inf):
            q = b.copy()
            k = 3 + 3 * int(rng.integers(0, 3))
            if bad == 0.0:
                q[k:k + 3] = 0.0
            else:
                q[k + int(rng.integers(0, 3))] = bad
            assert not within(shim, w, h, b, 0.0, 8.0, q) and not within(shim, w, h, q, 0.0, 8.0, b), (bad, k)
            assert not within(shim, w, h, q, 0.0, 8.0, np.nextafter(q, np.float32(1)))


# ------------------------------------------------------------------------------------------------ P4
def lens_camera(w, h, tx, ty, seed=0):
    """a camera at the origin with tan(half HFOV) = tx, tan(half VFOV) = ty, in a random orientation"""
    Rm = rotation(np.random.default_rng(seed).normal(size=3), 1.0)
    return c32(np.concatenate([[0, 0, 0], Rm[0] * tx, Rm[1] * ty, Rm[2]]))


@pytest.mark.parametrize("over", [-5e-4, 5e-4])
def test_p4_turn_bound_at_the_corner_angle_clamp(shim, over):
    """corner + angle just below and just above the 1.55 rad at which turn_px stops following 1 / cos^2"""
    w, h = 256, 256
    t = np.tan(1.5490) / np.sqrt(2.0)
    b = lens_camera(w, h, t, t)
    lens = np.zeros(3)
    shim.bc_lens(w, h, fp(b[3:]), dp(lens))
    assert abs(lens[1] - 1.5490) < 1e-6
    ang = 1.55 + over - lens[1]
    rng = np.random.default_rng(41)
    pix, jit = image_samples(rng, w, h, 64)
    for axis in (b[6:9] * t - b[3:6] * t, b[6:9] * t + b[3:6] * t, b[3:6], b[6:9], b[9:12]):  # the diagonals' turns move a corner ray outwards
        for sgn in (-1.0, 1.0):
            q = turned(b, rotation(axis.astype(np.float64), sgn * ang))
            margin = least_margin(shim, w, h, b, q)
            assert within(shim, w, h, b, 0.0, margin, q) and bound_px(shim, w, h, b, q) > 0.99 * margin
            outside, _ = displacement(shim, w, h, b, q, pix, jit)
            assert outside <= margin, (over, outside, margin)


def test_p4_margin_at_its_cap_and_slack_at_the_distance(shim):
    rng = np.random.default_rng(42)
    for it in range(60):
        b, w, h = random_camera(rng, list(LENS_CLASSES)[it % 3])
        margin = 8.0  # PT_BEAM_MAX_MARGIN's default
        # the largest turn the cap accepts, found by bisection on beam_within itself
        lo, hi = 0.0, angle_for(shim, w, h, b, 2.0 * margin)
        axis = rng.normal(size=3)
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if within(shim, w, h, b, 0.0, margin, turned(b, rotation(axis, mid))) else (lo, mid)
        q = turned(b, rotation(axis, lo))
        assert lo > 0.0 and within(shim, w, h, b, 0.0, margin, q) and bound_px(shim, w, h, b, q) > 0.99 * margin
        pix, jit = image_samples(rng, w, h, 64)
        assert displacement(shim, w, h, b, q, pix, jit)[0] <= margin
        check_pose_against_lists(shim, rng, w, h, b, 0.0, margin, q, n_blocks=1)
        # slack against the distance: accepted only inside slack * (1 - 1e-4), and P1 holds at the largest accepted distance
        slack = float(np.exp(rng.uniform(np.log(1e-3), np.log(2.0))))
        u = unit(rng.normal(size=3))
        q = b.copy()
        q[:3] = c32(b[:3] + u * slack)
        dist = np.linalg.norm(q[:3].astype(np.float64) - b[:3])
        assert not within(shim, w, h, b, np.float32(dist), 0.0, q), "slack equal to the distance must be refused (the 1 - 1e-4 factor)"
        assert within(shim, w, h, b, np.float32(dist * (1.0 + 2e-4)), 0.0, q)
        px, py = pick_block(rng, w, h, WHERE[it % len(WHERE)])
        s = float(np.float32(dist * (1.0 + 2e-4)))
        g = make_beam(shim, b, w, h, px, py, s, 0.0)
        pix, jit = block_samples(rng, w, h, px, py, 48)
        o, d = rays(shim, q, w, h, pix, jit)
        check_beam(shim, rng, g, o, d, s, n_boxes=80)


def test_p4_same_view_threshold_and_one_bit_without_margin(shim):
    rng = np.random.default_rng(43)
    for it in range(60):
        b, w, h = random_camera(rng, list(LENS_CLASSES)[it % 3])
        # axes that differ in one bit: never with margin_px == 0
        q = b.copy()
        k = 3 + int(rng.integers(0, 9))
        q[k] = np.nextafter(q[k], np.float32(np.inf))
        assert not within(shim, w, h, b, 0.0, 0.0, q) and not within(shim, w, h, b, 1.0, 0.0, q)
        assert within(shim, w, h, b, 0.0, 0.0, b.copy())
        # the 0.02-pixel threshold of "the same view": a change of one axis' length worth just under / just over it
        base = shim.bc_lens_px(w, h, fp(b[3:]), fp(b[3:]), fp(c32(b[3:] * np.array([1] * 6 + [1.001] * 3))))
        for px_target, same in ((0.019, True), (0.021, False)):
            rel = 1e-3 * px_target / base
            if rel < 4e-7:  # (below fp32's resolution for this lens)
                continue
            q = b.copy()
            q[9:12] = c32(b[9:12].astype(np.float64) * (1.0 + rel))
            got = shim.bc_lens_px(w, h, fp(q[3:]), fp(b[3:]), fp(q[3:]))
            if abs(got - px_target) > 5e-4:
                continue
            assert bool(shim.bc_same_lens(w, h, fp(q[3:]), fp(b[3:]), fp(q[3:]))) == same
            # what lens_px charges covers what the lens change does to the rays
            pix, jit = image_samples(rng, w, h, 40)
            assert displacement(shim, w, h, b, q, pix, jit)[1] <= got


# ------------------------------------------------------------------------------------------------ P5
def plan(lib, w, h, basis, step, acc, turned_, turn_acc, n_build, lanes, reach, max_slack, max_margin):
    out = np.zeros(4)
    lib.bc_plan(w, h, fp(basis), step, acc, turned_, turn_acc, n_build, lanes, reach, max_slack, max_margin, dp(out))
    return out


@pytest.mark.parametrize("accelerating", [False, True])
def test_p5_planned_lists_are_accepted_over_their_whole_span(shim, accelerating):
    """beam_cache_lookup's promise: lists planned at frame 0 from the last step and turn (centre and basis from beam_ahead, slack and margin from
    beam_plan) hold for every frame from n_build + lanes to n_build + lanes + span of a camera of constant velocity and turn rate -- and of
    one whose velocity changes by exactly `acc` per frame."""
    rng = np.random.default_rng(51 + accelerating)
    n_planned = 0
    for it in range(240):
        cam, w, h = random_camera(rng, list(LENS_CLASSES)[it % 3])
        n_build, lanes, reach = float(rng.integers(1, 9)), float(rng.integers(1, 4)), 32.0
        max_slack, max_margin = float(np.exp(rng.uniform(np.log(0.05), np.log(2.0)))), 8.0
        v = unit(rng.normal(size=3)) * max_slack * np.exp(rng.uniform(np.log(1e-3), np.log(0.3))) * (it % 4 != 0)
        a = unit(rng.normal(size=3)) * np.linalg.norm(v) * rng.uniform(0.0, 0.05) * accelerating
        rate = angle_for(shim, w, h, cam, max_margin * np.exp(rng.uniform(np.log(1e-3), np.log(0.3)))) * (it % 4 != 1)
        k = unit(rng.normal(size=3))
        base = cam[3:].astype(np.float64).reshape(3, 3)

        def pose(n):  # frame n of the trajectory (frame 0 = the planning frame), fp32 as a host would hand it over
            p = cam.copy()
            p[:3] = c32(cam[:3].astype(np.float64) + n * v + 0.5 * n * (n + 1) * a)
            p[3:] = c32((base @ rotation(k, n * rate).T).ravel())
            return p

        p0, p_1 = pose(0), pose(-1)
        vel = p0[:3].astype(np.float64) - p_1[:3]
        rot = np.zeros(3)
        t = shim.bc_rotation_between(fp(p_1[3:]), fp(p0[3:]), dp(rot))
        step = float(np.linalg.norm(vel))
        acc = float(np.linalg.norm(a)) * 1.0001 + 2e-7 * float(np.abs(p0[:3]).max()) * accelerating  # (the host sees the rounded positions' second difference)
        pl = plan(shim, w, h, p0[3:], step, acc, t, 0.0, n_build, lanes, reach, max_slack, max_margin)
        span, centre_ahead, slack, margin = pl
        if span < 4.0 or (slack == 0.0 and margin == 0.0):
            continue
        n_planned += 1
        lists = cam.copy()
        shim.bc_ahead(fp(p0[:3]), dp(vel), fp(p0[3:]), dp(rot), t, centre_ahead, fp(lists[:3]), fp(lists[3:]))
        for n in range(int(n_build + lanes), int(n_build + lanes + span) + 1):
            assert within(shim, w, h, lists, slack, margin, pose(n)), (it, n, span, slack, margin, step, t)
    print("P5 planned:", n_planned)
    assert n_planned >= 120, n_planned  # (seen: 235 and 218)
