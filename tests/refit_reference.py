"""A refit of the binary tree in plain numpy, and the inputs of the refit tests.

refit(nodes, order, spheres) keeps the links of `nodes` and recomputes every box the way csrc/pt_lbvh.cpp does: scene bounds over
fl(c -+ r) in float32, pad = max|bound| * 2^-17, a leaf box (c - r) - pad .. (c + r) + pad with float32 operations in that order, an inner
box the min / max of the two boxes in the child's record.  Float32 min / max are exact and numpy's float32 add / subtract / multiply
are IEEE operations without contraction, so the result is exact to the bit: it is compared without a tolerance.

contains64(nodes, order, spheres) is the property the boxes exist for, in float64: the box stored for a child contains c -+ r of every
sphere below that child.  For the reference it holds by construction: the two roundings of a leaf plane ((c - r), then - pad) move it by
less than 2^-23 * max|coordinate| each, 2^-22 together, and pad is 2^-17 of it.

patch_scene / motions / zero_component_rays make the scenes, the moves and the extra rays that tests/test_refit_reference.py (CPU: the
conditions on the inputs) and tests/test_gpu_refit.py (GPU: the refit kernels) share."""
import numpy as np

F32 = np.float32
PAD_SCALE = F32(2.0 ** -17)
BOX_FIELDS = ("lo0", "hi0", "lo1", "hi1")
LINK_FIELDS = ("child0", "child1", "parent")


def _centres_radii(spheres, dtype):
    return np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(dtype), spheres["r"].astype(dtype)


def levels(nodes):
    """depth of every inner node below the root (root = 1), and the nodes of each depth, deepest last"""
    n_nodes = len(nodes)
    level = np.zeros(n_nodes, dtype=np.int64)
    by_level, front = [], np.array([0], dtype=np.int64)
    while len(front):
        level[front] = len(by_level) + 1
        by_level.append(front)
        kids = np.concatenate([nodes["child0"][front], nodes["child1"][front]]).astype(np.int64)
        front = kids[kids >= 0]
    assert sum(len(f) for f in by_level) == n_nodes and (level > 0).all()  # every node reached exactly once: the links form a tree
    return level, by_level


def depth(nodes):
    return len(levels(nodes)[1]) if len(nodes) else 0


def padding(spheres):
    c, r = _centres_radii(spheres, F32)
    lo, hi = (c - r[:, None]).min(0), (c + r[:, None]).max(0)
    return F32(max(np.abs(lo).max(), np.abs(hi).max())) * PAD_SCALE


def refit(nodes, order, spheres):
    """`nodes` with its links kept and every box recomputed for `spheres` (leaf slot k holds sphere order[k])"""
    out = nodes.copy()
    if not len(nodes):
        return out
    pad = padding(spheres)
    c, r = _centres_radii(spheres, F32)
    c, r = c[order], r[order, None]
    leaf_lo, leaf_hi = (c - r) - pad, (c + r) + pad
    assert leaf_lo.dtype == F32 and leaf_hi.dtype == F32
    for front in reversed(levels(nodes)[1]):  # children are exactly one level below their parent: deepest level first
        for ck, lk, hk in (("child0", "lo0", "hi0"), ("child1", "lo1", "hi1")):
            ch = nodes[ck][front].astype(np.int64)
            leaf = ch < 0
            inner = np.where(leaf, 0, ch)
            out[lk][front] = np.where(leaf[:, None], leaf_lo[np.where(leaf, ~ch, 0)], np.minimum(out["lo0"][inner], out["lo1"][inner]))
            out[hk][front] = np.where(leaf[:, None], leaf_hi[np.where(leaf, ~ch, 0)], np.maximum(out["hi0"][inner], out["hi1"][inner]))
    return out


def contains64(nodes, order, spheres):
    """True if the box stored for every child contains, in float64, c -+ r of every sphere below that child"""
    if not len(nodes):
        return True
    c, r = _centres_radii(spheres, np.float64)
    c, r = c[order], r[order, None]
    leaf_lo, leaf_hi = c - r, c + r
    n_nodes = len(nodes)
    sub_lo = {k: np.zeros((n_nodes, 3)) for k in ("child0", "child1")}  # exact bounds of the spheres below each child
    sub_hi = {k: np.zeros((n_nodes, 3)) for k in ("child0", "child1")}
    ok = True
    for front in reversed(levels(nodes)[1]):
        for ck, lk, hk in (("child0", "lo0", "hi0"), ("child1", "lo1", "hi1")):
            ch = nodes[ck][front].astype(np.int64)
            leaf = ch < 0
            inner = np.where(leaf, 0, ch)
            sub_lo[ck][front] = np.where(leaf[:, None], leaf_lo[np.where(leaf, ~ch, 0)], np.minimum(sub_lo["child0"][inner], sub_lo["child1"][inner]))
            sub_hi[ck][front] = np.where(leaf[:, None], leaf_hi[np.where(leaf, ~ch, 0)], np.maximum(sub_hi["child0"][inner], sub_hi["child1"][inner]))
            ok = ok and bool((nodes[lk][front].astype(np.float64) <= sub_lo[ck][front]).all() and (nodes[hk][front].astype(np.float64) >= sub_hi[ck][front]).all())
    return ok


def same_links(a, b):
    return all(np.array_equal(a[f], b[f]) for f in LINK_FIELDS)


def box_mismatches(a, b):
    """number of node records whose boxes differ in any bit"""
    bad = np.zeros(len(a), dtype=bool)
    for f in BOX_FIELDS:
        bad |= (a[f].view(np.uint32) != b[f].view(np.uint32)).any(1)
    return int(bad.sum())


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
SIZES = (2, 3, 64, 65, 1023, 1024, 1025, 1026, 5000)  # one node; the wave boundary; either side of kRefitSmall = 1024; several launches
NO_LDS_SIZE = 1500   # the column with PT_FLAG_NO_LDS_SCENE: the private tree walked in global memory
LARGE_SIZES = (65, 1500)
LARGE_SCALE = F32(2.0 ** 31)  # a power of two: every float32 operation of the intersection is rescaled exactly
N_RAYS = 20000
HIT_SHARE = 0.3      # of all rays
ZERO_HITS = 200      # among the rays with a direction component that is exactly +-0


def patch_scene(sphere_dtype, n, seed=0):
    """n - 1 spheres of radius 0.05 .. 0.5 in a 10 x 2 x 10 patch, and the ground sphere (r = 50) as the last element"""
    rng = np.random.default_rng(1000 * n + seed)
    s = np.zeros(n, dtype=sphere_dtype)
    m = n - 1
    s["r"][:m] = rng.uniform(0.05, 0.5, m)
    s["cx"][:m] = rng.uniform(-5, 5, m)
    s["cz"][:m] = rng.uniform(-5, 5, m)
    s["cy"][:m] = s["r"][:m] + rng.uniform(0, 2, m).astype(F32)
    s["cy"][m], s["r"][m] = -50.0, 50.0
    return s


def wave_edge_ids(n):
    """where motion 6 puts the extreme sphere: the last id, the one before it, and the id that lane 63 of the last full wave handles"""
    ids = [n - 1, n - 2] + ([(n // 64) * 64 - 1] if n >= 64 else [])
    return sorted({k for k in ids if k >= 0}, reverse=True)


def motions(base, seed=0):
    """[(name, spheres)]: the moves of one context, in the order they are applied.  Every one is a full set of centres and radii for the ids
    of `base`."""
    n = len(base)
    rng = np.random.default_rng(77 * n + seed)
    axes = ("cx", "cy", "cz")
    out = []
    jit = base.copy()
    for a in axes:
        jit[a] += rng.uniform(-0.3, 0.3, n).astype(F32)
    jit["r"] *= rng.uniform(0.7, 1.2, n).astype(F32)
    out.append(("jitter", jit))
    far = jit.copy()
    for a, t in zip(axes, (3000.0, -7000.0, 500.0)):
        far[a] += F32(t)
    out.append(("translated", far))   # the bounds, and the pad, two orders of magnitude larger
    small = jit.copy()
    for a in axes + ("r",):
        small[a] *= F32(2.0 ** -6)
    out.append(("shrunk", small))     # the pad shrinks: a stale one would still contain the spheres, and fail the bit compare
    out.append(("permuted", jit[rng.permutation(n)]))  # the topology has nothing to do with the positions any more
    neg = jit.copy()
    for a in axes:
        neg[a] -= (jit[a] + jit["r"]).max() + F32(1.0)
    assert all(((neg[a] + neg["r"]) < 0).all() for a in axes)
    out.append(("negative", neg))
    for k in wave_edge_ids(n):
        ext = jit.copy()
        if k == n - 1:
            ext[0] = ext[n - 1]  # (keep the ground in the scene: axis-parallel rays need something to hit)
        ext[k] = (80.0, 30.0, 90.0, 1.5)  # c + r is the maximum of the bounds on all three axes
        assert all((ext[a] + ext["r"]).argmax() == k for a in axes)
        out.append((f"extreme_at_{k}", ext))
    one = jit.copy()
    one["cx"], one["cy"], one["cz"], one["r"] = 1.0, 2.0, 3.0, 0.75
    out.append(("coincident", one))
    return out


def scaled(spheres, scale=LARGE_SCALE):
    s = spheres.copy()
    for a in ("cx", "cy", "cz", "r"):
        s[a] *= scale
    return s


def zero_component_rays(spheres, n, seed, scale=LARGE_SCALE):
    """n rays for `spheres` * scale with one or two direction components exactly +-0, from origins in the patch whose every coordinate is
    beyond 0.2 * scale in magnitude (> 4e8 at 2^31) and inside the scene bounds: half aimed at a sphere before the components are zeroed"""
    rng = np.random.default_rng(seed)
    c, _ = _centres_radii(spheres, np.float64)
    o = np.stack([rng.uniform(0.2, 5.0, n) * rng.choice([-1.0, 1.0], n), rng.uniform(0.2, 2.5, n), rng.uniform(0.2, 5.0, n) * rng.choice([-1.0, 1.0], n)], 1)
    d = np.where((np.arange(n) % 2 == 0)[:, None], c[rng.integers(0, len(spheres), n)] - o, rng.normal(size=(n, 3)))
    d32 = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    keep = rng.integers(1, 7, n)  # bit a set: component a stays (never none, never all three)
    for a in range(3):
        z = ((keep >> a) & 1) == 0
        d32[z, a] = np.where(rng.random(int(z.sum())) < 0.5, F32(0.0), F32(-0.0))
    d32 /= np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True).astype(F32)
    o32 = o.astype(F32) * scale
    assert (np.abs(o32) > 4e8).all() or scale != LARGE_SCALE
    return o32, d32


def ray_seed(n, k):
    """the seed of the rays traced after move k of the scene of n spheres"""
    return 100 * n + k


def rays_for(make_rays, spheres, seed):
    """test_gpu_accel.make_rays' N_RAYS rays for moved spheres.  make_rays draws its origins from the scene bounds clipped to +-60 around the
    origin of the coordinates, which a scene translated by thousands of units does not meet (it raises): the rays are made for the spheres
    shifted back by the whole-number median of their centres, and their origins shifted forth again."""
    shift = np.round(np.median(_centres_radii(spheres, np.float64)[0], axis=0)).astype(F32)
    back = spheres.copy()
    for a, t in zip(("cx", "cy", "cz"), shift):
        back[a] -= t
    o, d = make_rays(back, N_RAYS, seed=seed)
    return o + shift, d


def large_move_rays(make_rays, base, scale=LARGE_SCALE):
    """(origins, directions, n_first) for `base` * scale: make_rays' set on the unscaled scene with its origins scaled (the first n_first rays),
    then 2000 zero-component rays from origins beyond 4e8"""
    o, d = make_rays(base, N_RAYS, seed=ray_seed(len(base), 99))
    oz, dz = zero_component_rays(base, 2000, seed=ray_seed(len(base), 98), scale=scale)
    return np.concatenate([o * scale, oz]), np.concatenate([d, dz]), len(o)


def has_zero_component(d):
    return (d == 0).any(1)
