"""Independent float64 numpy restatement of DESIGN.md spec S14 (row N8, the NRD composition pass), written from the spec text, not
from csrc/pt_nrd.h.  Buffers are numpy arrays over the pixels of a row-major w x h image: depth (n,), albedos (n, 3), float4 ones (n, 4).
The albedo quotients are IEEE float32 divisions, as the spec says (what decides whether a lobe is sanitised to black); everything after
them is evaluated in float64.  Each function returns the result and a per-pixel magnitude for tolerances."""
import numpy as np

REBLUR, RELAX = 2, 3
FP16_MAX = 65504.0
EPS = 1e-6
HIT_DISTANCE = (3.0, 0.1, 20.0, -25.0)  # nrd::ReblurSettings().hitDistanceParameters


def exp2_spec(y):
    """spec S2's exp2: k = floor(y + 0.5), degree-7 Taylor of e^(f ln 2), scaled by 2^k"""
    y = np.asarray(y, np.float64)
    k = np.floor(y + 0.5)
    t = (y - k) * np.log(2.0)
    p = sum(t ** j / float(np.prod(range(1, j + 1))) for j in range(8))
    return p * np.exp2(k)


def saturate(x):
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0.0, np.clip(x, 0.0, 1.0))


def norm_hit_dist(h, z, P, r):
    """saturate(h / ((P.x + |z| P.y) (1 + (P.z - 1) saturate(exp2((P.w r) r)))))"""
    h, z, r = (np.asarray(a, np.float64) for a in (h, z, r))
    with np.errstate(all="ignore"):
        f = (P[0] + np.abs(z) * P[1]) * (1.0 + (P[2] - 1.0) * saturate(exp2_spec(P[3] * r * r)))
        return saturate(h / f)


def sanitize_rgb(c):
    """a lobe with any NaN / inf channel -> 0, else each channel clamped to [0, 65504]"""
    bad = ~np.isfinite(c).all(axis=-1, keepdims=True)
    return np.where(bad, 0.0, np.clip(np.where(bad, 0.0, c), 0.0, FP16_MAX))


def keep_nonzero(a):
    return np.where(a != 0.0, np.maximum(a, EPS), a)


def to_ycocg(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([0.25 * r + 0.5 * g + 0.25 * b, 0.5 * r - 0.5 * b, -0.25 * r + 0.5 * g - 0.25 * b], axis=-1)


def from_ycocg(c):
    y, co, cg = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(invalid="ignore"):
        rgb = np.stack([y - cg + co, y + cg, y - cg - co], axis=-1)
    return np.where(np.isnan(rgb), 0.0, np.maximum(rgb, 0.0))


def quotient(lobe, albedo):
    with np.errstate(all="ignore"):
        return (np.asarray(lobe, np.float32)[..., :3] / np.asarray(albedo, np.float32)).astype(np.float64)


def pack(mode, depth, da, sa, nr, nd, ns, P=HIT_DISTANCE):
    """-> (packed diffuse, packed specular) (n, 4) float64; misses keep their input"""
    hit = np.isfinite(depth)
    out = []
    for lobe, albedo, rough in ((nd, da, np.ones(len(depth))), (ns, sa, None if nr is None else nr[:, 3])):
        rgb = sanitize_rgb(quotient(lobe, albedo))
        a = np.asarray(lobe, np.float64)[:, 3]
        if mode == REBLUR:
            a = norm_hit_dist(a, depth, P, rough)
            a = np.where(np.isfinite(a), saturate(a), 0.0)
            rgb = to_ycocg(rgb)
        else:
            a = np.where(np.isfinite(a), np.clip(np.where(np.isfinite(a), a, 0.0), 0.0, FP16_MAX), 0.0)
        res = np.concatenate([rgb, keep_nonzero(a)[:, None]], axis=1)
        out.append(np.where(hit[:, None], res, np.asarray(lobe, np.float64)))
    return out[0], out[1]


def compose(mode, depth, da, sa, dd, ds, rad):
    """-> (radiance (n, 4) float64, per-pixel magnitude (n, 1)); misses keep their input"""
    hit = np.isfinite(depth)
    dd, ds, rad = (np.asarray(a, np.float64) for a in (dd, ds, rad))
    drgb, srgb = dd[:, :3], ds[:, :3]
    if mode == REBLUR:
        drgb, srgb = from_ycocg(drgb), from_ycocg(srgb)
    with np.errstate(all="ignore"):
        ld, ls = drgb * np.asarray(da, np.float64), srgb * np.asarray(sa, np.float64)
        res = rad.copy()
        res[:, :3] = rad[:, :3] + (ld + ls)
        cross = [np.abs(x[:, :3]).max(axis=1, keepdims=True) * np.abs(np.asarray(a, np.float64)).max(axis=1, keepdims=True) for x, a in ((dd, da), (ds, sa))]
        scale = np.nanmax(np.abs(np.concatenate([rad[:, :3], ld, ls] + cross, axis=1)), axis=1, initial=0.0)[:, None]
    return np.where(hit[:, None], res, rad), scale
