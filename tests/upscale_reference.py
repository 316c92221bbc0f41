"""Spec S17 -- the super-resolution stand-in of row N11 -- restated in float64 numpy, written from the spec's
text and not from csrc/pt_upscale.h: every output pixel at once, tap by tap.  upscale() also returns, per output pixel, how far the
spec's discrete decisions (the nearest input pixel, the weight-sum fallback, the history's accept tests and the texel of its depth
test) are from flipping, relative to the magnitude of the quantity decided on, so a test can tell an fp32 rounding of such a decision
from an error."""
import numpy as np

MAX_RADIANCE = 65504.0
WEIGHT_MIN = 2.0 ** -10
COVERAGE_MIN = 1.0 / 16.0
DEPTH_REL = 0.1


def sanitize(c):
    c = np.asarray(c, np.float64)
    return np.where(np.isnan(c), 0.0, np.minimum(np.maximum(c, 0.0), MAX_RADIANCE))


def to_t(c):
    c = sanitize(c)
    return c / (1.0 + c.max(axis=-1, keepdims=True))


def from_t(t):
    return t / (1.0 - t.max(axis=-1, keepdims=True))


def lanczos(x2):
    x2 = np.asarray(x2, np.float64)
    v = (25.0 / 16.0 * (2.0 / 5.0 * x2 - 1.0) ** 2 - 9.0 / 16.0) * (x2 / 4.0 - 1.0) ** 2
    return np.where(x2 < 4.0, v, 0.0)


def halton(i, base):
    """the radical inverse of i >= 1"""
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def bilinear_clamp(img, x, y):
    """img (H, W, C) sampled at texel coordinates (x, y) (texel i covers [i, i + 1), its centre sampled at i), footprint clamped"""
    H, W = img.shape[:2]
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[..., None], (y - yf)[..., None]
    x0, x1 = np.clip(xf, 0, W - 1).astype(int), np.clip(xf + 1, 0, W - 1).astype(int)
    y0, y1 = np.clip(yf, 0, H - 1).astype(int), np.clip(yf + 1, 0, H - 1).astype(int)
    top = img[y0, x0] + (img[y0, x1] - img[y0, x0]) * fx
    bot = img[y1, x0] + (img[y1, x1] - img[y1, x0]) * fx
    return top + (bot - top) * fy


def upscale(color, depth, velocity, prev, out_size, jitter=(0.0, 0.0), max_a=16.0):
    """One call of S17.  color (h, w, 4), depth (h, w), velocity (h, w, 3); prev = None (a restart) or (hist (H, W, 4), z (H, W)), the
    previous slot; out_size = (W, H).  -> dict: out (H, W, 4), hist (H, W, 4), z (H, W), accepted (H, W) bool, margin (H, W)."""
    color, depth, velocity = (np.asarray(a, np.float64) for a in (color, depth, velocity))
    h, w = depth.shape
    W, H = out_size
    jx, jy = float(jitter[0]), float(jitter[1])
    sx, sy = W / w, H / h
    t_in = to_t(color[..., :3])
    oy, ox = np.mgrid[0:H, 0:W]
    px, py = (2 * ox + 1) * w / (2.0 * W), (2 * oy + 1) * h / (2.0 * H)
    nx, ny = np.clip(np.floor(px), 0, w - 1).astype(int), np.clip(np.floor(py), 0, h - 1).astype(int)
    margin = np.minimum(np.abs(px - np.round(px)) / np.maximum(px, 1.0), np.abs(py - np.round(py)) / np.maximum(py, 1.0))
    sw = np.zeros((H, W))
    acc = np.zeros((H, W, 3))
    lo, hi = np.full((H, W, 3), np.inf), np.full((H, W, 3), -np.inf)
    cov = np.zeros((H, W))
    z = np.full((H, W), np.nan)
    mv = np.zeros((H, W, 3))
    first = np.ones((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ix, iy = nx + dx, ny + dy
            ok = (ix >= 0) & (iy >= 0) & (ix < w) & (iy < h)
            cx, cy = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
            ddx, ddy = (ix + 0.5 - jx) - px, (iy + 0.5 - jy) - py
            wt = np.where(ok, lanczos(ddx * ddx) * lanczos(ddy * ddy), 0.0)
            t = t_in[cy, cx]
            sw += wt
            acc += wt[..., None] * t
            lo = np.where(ok[..., None], np.minimum(lo, t), lo)
            hi = np.where(ok[..., None], np.maximum(hi, t), hi)
            k = np.maximum(0.0, 1.0 - np.abs(ddx) * sx) * np.maximum(0.0, 1.0 - np.abs(ddy) * sy)
            cov = np.where(ok, np.maximum(cov, k), cov)
            zk = depth[cy, cx]
            with np.errstate(invalid="ignore"):
                take = ok & (first | (zk < z))
            z = np.where(take, zk, z)
            mv = np.where(take[..., None], velocity[cy, cx], mv)
            first &= ~ok
    small = sw <= WEIGHT_MIN
    margin = np.minimum(margin, np.abs(sw - WEIGHT_MIN))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(small[..., None], t_in[ny, nx], acc / np.where(small, 1.0, sw)[..., None])
    u = np.minimum(np.maximum(u, lo), hi)
    kappa = np.clip(cov, COVERAGE_MIN, 1.0)
    t_out, a_out = u.copy(), kappa.copy()
    accepted = np.zeros((H, W), bool)
    if prev is not None:
        hist, zprev = np.asarray(prev[0], np.float64), np.asarray(prev[1], np.float64)
        qx, qy = (ox + 0.5) + mv[..., 0] * sx, (oy + 0.5) + mv[..., 1] * sy
        inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
        nqx, nqy = np.maximum(np.abs(qx), 1.0), np.maximum(np.abs(qy), 1.0)  # (margins of q relative to its magnitude)
        margin = np.minimum(margin, np.minimum(np.minimum(np.abs(qx), np.abs(qx - W)) / nqx, np.minimum(np.abs(qy), np.abs(qy - H)) / nqy))
        margin = np.where(inside, np.minimum(margin, np.minimum(np.abs(qx - np.round(qx)) / nqx, np.abs(qy - np.round(qy)) / nqy)), margin)
        tx, ty = np.clip(np.floor(qx), 0, W - 1).astype(int), np.clip(np.floor(qy), 0, H - 1).astype(int)
        zp = zprev[ty, tx]
        ze = z + mv[..., 2]
        fin, finp = np.isfinite(z), np.isfinite(zp)
        with np.errstate(invalid="ignore"):
            gap = np.abs(zp - ze) - DEPTH_REL * ze
            depth_ok = (~fin & ~finp) | (fin & finp & (gap <= 0))
            margin = np.where(inside & fin & finp, np.minimum(margin, np.abs(gap) / np.maximum(np.abs(ze), 1e-30)), margin)
        s = bilinear_clamp(hist, np.where(inside, qx, 0.5) - 0.5, np.where(inside, qy, 0.5) - 0.5)
        accepted = inside & depth_ok & (s[..., 3] > 0)
        hc = np.minimum(np.maximum(s[..., :3], lo), hi)
        with np.errstate(invalid="ignore"):
            alpha = (kappa / (kappa + s[..., 3]))[..., None]
            t_out = np.where(accepted[..., None], hc + (u - hc) * alpha, u)
            a_out = np.where(accepted, np.minimum(s[..., 3] + kappa, max_a), kappa)
    out = np.concatenate([from_t(t_out), color[ny, nx, 3:4]], axis=-1)
    return dict(out=out, hist=np.concatenate([t_out, a_out[..., None]], axis=-1), z=z, accepted=accepted, margin=margin, kappa=kappa)


def bilinear_upsample(img, out_size):
    """the plain bilinear upsample the quality test compares with: output pixel centres mapped into the input's texel grid"""
    h, w = img.shape[:2]
    W, H = out_size
    oy, ox = np.mgrid[0:H, 0:W]
    return bilinear_clamp(np.asarray(img, np.float64), (ox + 0.5) * w / W - 0.5, (oy + 0.5) * h / H - 0.5)
