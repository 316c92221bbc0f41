"""The sphere layouts of the wide-view tests (tests/test_wide_view.py on host-built trees, tests/test_gpu_wide.py on the device's),
each from a fixed seed so both run the same spheres, and the rays that T3 traces through them."""
import numpy as np

SPHERE_DTYPE = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("r", "<f4")])

PLACEMENTS = {"pow2": (65536.0, -131072.0, 32768.0),  # nodes straddle a power of two on every axis: the ulp doubles inside a node's box
              "million": (1.0e6, 1.0e6, -1.0e6), "origin": (0.0, 0.0, 0.0), "offset": (3.0, -7.0, 11.0)}

# name -> host.scene arguments (kind name, count); the rest are made here
HOST_SCENES = {"small": ("SCENE_SMALL", 0), "demo": ("SCENE_DEMO", 0), "procedural_3000": ("SCENE_PROCEDURAL", 3000), "procedural_40000": ("SCENE_PROCEDURAL", 40000)}

NAMES = ([f"tiny_far-{p}-{n}" for p in PLACEMENTS for n in (3, 64, 2000)] + ["mixed_scale", "geometric", "concentric", "duplicates"]
         + [f"line-{n}" for n in (2, 3, 4, 5)] + list(HOST_SCENES))
CHECK_WIDE_MAX_SPHERES = 50000  # check_wide is vectorised: about a second per 10^4 spheres


def tiny_far(centre, n, seed):
    """radii 1e-4 .. 1e-3 (log-uniform), centres uniform in a cube of side 8 around `centre`"""
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=SPHERE_DTYPE)
    for a, k in enumerate(("cx", "cy", "cz")):
        s[k] = centre[a] + rng.uniform(-4.0, 4.0, n)
    s["r"] = 10.0 ** rng.uniform(-4.0, -3.0, n)
    return s


def layout(name, host=None, dxrs=None):
    """-> spheres (SPHERE_DTYPE) of the named layout; the host scenes need the `host` and `dxrs` fixtures"""
    if name in HOST_SCENES:
        kind, count = HOST_SCENES[name]
        return host.scene(getattr(dxrs.host, kind), seed=1, count=count)[0]
    if name.startswith("tiny_far-"):
        _, place, n = name.split("-")
        return tiny_far(PLACEMENTS[place], int(n), seed=1000 + int(n) + len(place))
    if name == "mixed_scale":  # the demo's ground under a swarm of tiny spheres: coarse cells, boxes one or two cells wide
        s = np.zeros(2001, dtype=SPHERE_DTYPE)
        s[:2000] = tiny_far(PLACEMENTS["origin"], 2000, seed=77)
        s[2000] = (0.0, -1004.5, 0.0, 1000.0)
        return s
    if name == "geometric":  # tests/test_abi.py test_host_sah_structure's cases: one-against-the-rest splits all the way down
        s = np.zeros(1000, dtype=SPHERE_DTYPE)
        s["cx"] = 2.0 ** (np.arange(1000) / 12.0); s["r"] = s["cx"] * 0.01
        return s
    if name == "concentric":
        s = np.zeros(300, dtype=SPHERE_DTYPE)
        s["r"] = 1 + np.arange(300)
        return s
    if name == "duplicates":
        s = np.zeros(64, dtype=SPHERE_DTYPE)
        s["r"] = 0.5; s["cx"] = 1.0
        return s
    if name.startswith("line-"):
        n = int(name.split("-")[1])
        s = np.zeros(n, dtype=SPHERE_DTYPE)
        s["cx"] = 3.0 * np.arange(n); s["r"] = 1.0
        return s
    raise KeyError(name)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rays(spheres, n, seed):
    """T3's mix, unit float32 directions: half aimed at jittered points of picked spheres, a quarter tangent to one (impact parameter
    r (1 +- 2^-k), k = 8 .. 20), an eighth with one or two direction components exactly +0 / -0 and the origin's matching coordinates inside
    the picked sphere's [c - r, c + r], an eighth random."""
    rng = np.random.default_rng(seed)
    c = np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(np.float64)
    r = spheres["r"].astype(np.float64)
    pick = rng.integers(0, len(spheres), n)
    cp, rp = c[pick], r[pick]
    dist = np.maximum(4.0, 3.0 * rp)[:, None]  # origins a few units (or radii) from the picked sphere
    kind = np.arange(n) % 8  # 0..3 aimed, 4..5 tangent, 6 axis-parallel, 7 random
    aimed, tang = kind < 4, (kind == 4) | (kind == 5)
    nt = int(tang.sum())
    dt = _unit(rng.normal(size=(nt, 3)))
    pt = _unit(np.cross(dt, rng.normal(size=(nt, 3))))  # a unit vector perpendicular to the direction
    b = rp[tang] * (1.0 + rng.choice([-1.0, 1.0], nt) * 2.0 ** -rng.integers(8, 21, nt).astype(np.float64))
    touch = cp[tang] + pt * b[:, None]  # the point at distance b from the centre that the tangent ray passes through
    o = cp + _unit(rng.normal(size=(n, 3))) * dist * rng.uniform(0.5, 1.5, (n, 1))
    o[tang] = touch - dt * dist[tang]
    # origins are rounded to float32 FIRST and the directions taken from the rounded origins: far from the world's origin one float32 step
    # is several radii of these spheres
    o32 = o.astype(np.float32)
    o = o32.astype(np.float64)
    d = _unit(rng.normal(size=(n, 3)))  # the random eighth keeps this
    d[aimed] = _unit(cp[aimed] + rng.normal(size=(int(aimed.sum()), 3)) * rp[aimed, None] * 0.5 - o[aimed])
    d[tang] = _unit(touch - o[tang])
    d32 = d.astype(np.float32)
    ax = np.nonzero(kind == 6)[0]
    zero_mask = rng.integers(1, 7, len(ax))  # bit a set: component a is zeroed (one or two of the three)
    for a in range(3):
        z = ax[((zero_mask >> a) & 1).astype(bool)]
        d32[z, a] = np.where(rng.random(len(z)) < 0.5, np.float32(0.0), np.float32(-0.0))
        inside = (cp[z, a] + rng.uniform(-0.9, 0.9, len(z)) * rp[z]).astype(np.float32)
        o32[z, a] = np.clip(inside, (cp[z, a] - rp[z]).astype(np.float32), (cp[z, a] + rp[z]).astype(np.float32))
    d32 = (d32 / np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return o32, d32
