"""Spec S21 -- the ray-reconstruction stand-in of row N15 -- restated in float64 numpy, written from the spec's
text and not from csrc/pt_rr.h: every pixel at once, tap by tap.  prepare() and resolve() also return, per pixel, how far the spec's
discrete decisions (the nearest input pixel, the sign of the projected w, the history's inside, depth, normal and weight tests, the
weight-sum fallback, the floor of the variance) are from flipping, relative to the magnitude of the quantity decided on, so a test can
tell an fp32 rounding of such a decision from an error.  A pixel whose nearest input pixel is a miss is spec S17: upscale_reference."""
import numpy as np

import upscale_reference as up

ALBEDO_MIN = 2.0 ** -10
VIRTUAL_ROUGHNESS = 2.5
DEPTH_EDGE, DEPTH_EDGE_MIN = 0.05, 1e-30
NORMAL_EDGE, NORMAL_SCALE = 0.8, 5.0
ROUGHNESS_EDGE = 4.0
WIDE_INV_R2 = 1.0 / 9.0
LONG_HISTORY = 0.25
CLIP_SIGMA = 1.5
HISTORY_NORMAL = 0.8
HISTORY_WEIGHT_MIN = 1.0 / 64.0
LUMA = np.array([0.2126, 0.7152, 0.0722])


def project(m, p):
    """[p, 1] . M, M = 16 floats as DirectXMath rows; p (..., 3) -> (..., 4)"""
    m = np.asarray(m, np.float64).reshape(4, 4)
    return p @ m[:3] + m[3]


def albedo(diffuse, specular):
    return up.sanitize(np.asarray(diffuse, np.float64) + np.asarray(specular, np.float64))


def prepare(tex, cam, jitter=(0.0, 0.0)):
    """Step 1.  tex: dict of Color (h, w, 4), Depth (h, w), MotionVector (h, w, 3), NormalRoughness (h, w, 4), DiffuseAlbedo and
    SpecularAlbedo (h, w, 3), SpecularHitDistance (h, w); cam: dict of Position (3), ProjectionToView, ViewToWorld,
    PreviousWorldToProjection (16 each).  -> dict: tz (h, w, 4), nr (h, w, 4), virt (h, w, 3), margin (h, w)"""
    color, depth, mv, nr, da, sa, hit = (np.asarray(tex[k], np.float64) for k in ("Color", "Depth", "MotionVector", "NormalRoughness", "DiffuseAlbedo",
                                                                                  "SpecularAlbedo", "SpecularHitDistance"))
    h, w = depth.shape
    with np.errstate(invalid="ignore"):
        surface = np.isfinite(depth) & (depth > 0)
    c = up.sanitize(color[..., :3])
    A = albedo(da, sa)
    d = np.where(surface[..., None], np.minimum(c / np.maximum(A, ALBEDO_MIN), up.MAX_RADIANCE), c)
    t = d / (1.0 + d.max(axis=-1, keepdims=True))
    z = np.where(surface, depth, np.inf)
    n = np.where(np.isnan(nr[..., :3]), 0.0, np.clip(nr[..., :3], -1.0, 1.0))
    rough = np.where(np.isnan(nr[..., 3]), 0.0, np.clip(nr[..., 3], 0.0, 1.0))
    nr_out = np.where(surface[..., None], np.concatenate([n, rough[..., None]], axis=-1), 0.0)
    # the virtual motion of the specular reflection
    with np.errstate(invalid="ignore"):
        has_hit = surface & np.isfinite(hit) & (hit > 0)
    f = np.maximum(0.0, 1.0 - rough * VIRTUAL_ROUGHNESS)
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = (xs + 0.5 - jitter[0]) / w, (ys + 0.5 - jitter[1]) / h
    ndc = np.stack([2.0 * u - 1.0, 1.0 - 2.0 * v, np.full_like(u, 0.5)], axis=-1)
    zs = np.where(surface, depth, 1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = project(cam["ProjectionToView"], ndc)
        view = np.stack([p[..., 0] / p[..., 2] * zs, p[..., 1] / p[..., 2] * zs, zs], axis=-1)
        X = project(cam["ViewToWorld"], view)[..., :3]
        V = X - np.asarray(cam["Position"], np.float64)
        V = V / np.sqrt((V * V).sum(axis=-1, keepdims=True))
        clip = project(cam["PreviousWorldToProjection"], X + V * (np.where(has_hit, hit, 0.0) * f)[..., None])
        ok = has_hit & (clip[..., 3] > 0)
        up_, vp = clip[..., 0] / clip[..., 3] * 0.5 + 0.5, clip[..., 1] / clip[..., 3] * -0.5 + 0.5
        ld, ls = up.sanitize(da) @ LUMA, up.sanitize(sa) @ LUMA
        share = np.where(ld + ls > 0, ls / np.where(ld + ls > 0, ld + ls, 1.0), 0.0)
        virt = np.where(ok[..., None], np.stack([(up_ - u) * w, (vp - v) * h, share * f], axis=-1),
                        np.stack([mv[..., 0], mv[..., 1], np.zeros_like(u)], axis=-1))
        margin = np.where(has_hit, np.abs(clip[..., 3]) / np.maximum(np.abs(clip).max(axis=-1), 1e-30), np.inf)
    return dict(tz=np.concatenate([t, z[..., None]], axis=-1), nr=nr_out, virt=virt, margin=margin, position=X, virtual_clip=clip)


def history_tap(prev, qx, qy, ze, n, size):
    """the history at output position q: bilinear over the corners that pass the depth and normal tests -> (value (H, W, 4), margin)"""
    hist, hist_n, zprev = (np.asarray(a, np.float64) for a in prev)
    W, H = size
    with np.errstate(invalid="ignore"):
        inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
    nq = np.maximum(np.maximum(np.abs(qx), np.abs(qy)), 1.0)
    with np.errstate(invalid="ignore"):
        margin = np.minimum(np.minimum(np.abs(qx), np.abs(qx - W)), np.minimum(np.abs(qy), np.abs(qy - H))) / nq
    margin = np.where(np.isnan(margin), np.inf, margin)
    x, y = np.where(inside, qx, 0.5) - 0.5, np.where(inside, qy, 0.5) - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    sw = np.zeros(qx.shape)
    acc = np.zeros(qx.shape + (4,))
    for j, wy in ((0, 1.0 - fy), (1, fy)):
        for i, wx in ((0, 1.0 - fx), (1, fx)):
            cx, cy = np.clip(xf + i, 0, W - 1).astype(int), np.clip(yf + j, 0, H - 1).astype(int)
            zp = zprev[cy, cx]
            wk = wx * wy
            with np.errstate(invalid="ignore"):
                gap = np.abs(zp - ze) - up.DEPTH_REL * ze
                depth_ok = np.isfinite(zp) & (gap <= 0)
                cos = (hist_n[cy, cx, :3] * n).sum(axis=-1)
                ok = depth_ok & (cos >= HISTORY_NORMAL)
                # a corner that matters (its weight is not negligible) and whose test is about to flip
                near = np.minimum(np.where(np.isfinite(zp), np.abs(gap) / np.maximum(np.abs(ze), 1e-30), np.inf), np.abs(cos - HISTORY_NORMAL))
                near = np.where(np.isnan(near), np.inf, near)
            margin = np.where(inside & (wk > 1e-6), np.minimum(margin, near), margin)
            sw += np.where(ok, wk, 0.0)
            acc += np.where(ok, wk, 0.0)[..., None] * np.where(ok[..., None], hist[cy, cx], 0.0)
    margin = np.where(inside, np.minimum(margin, np.abs(sw - HISTORY_WEIGHT_MIN)), margin)
    good = inside & (sw > HISTORY_WEIGHT_MIN)
    val = acc / np.where(good, sw, 1.0)[..., None]
    good &= val[..., 3] > 0
    return np.where(good[..., None], val, 0.0), margin


def resolve(tex, prep, prev, out_size, jitter=(0.0, 0.0), max_a=16.0):
    """Steps 2-6 for every output pixel.  prep: prepare()'s records (or the header's); prev = None (a restart) or (hist (H, W, 4),
    normal (H, W, 4), z (H, W)), the previous slot.  -> dict: out, hist, hist_n (H, W, 4), z, surface, accepted, margin, kappa (H, W)"""
    color, mv, da, sa = (np.asarray(tex[k], np.float64) for k in ("Color", "MotionVector", "DiffuseAlbedo", "SpecularAlbedo"))
    tz, nr, virt = (np.asarray(prep[k], np.float64) for k in ("tz", "nr", "virt"))
    h, w = tz.shape[:2]
    W, H = out_size
    jx, jy = float(jitter[0]), float(jitter[1])
    sx, sy = W / w, H / h
    oy, ox = np.mgrid[0:H, 0:W]
    cx, cy = ox + 0.5, oy + 0.5
    px, py = (2 * ox + 1) * w / (2.0 * W), (2 * oy + 1) * h / (2.0 * H)
    nx, ny = np.clip(np.floor(px), 0, w - 1).astype(int), np.clip(np.floor(py), 0, h - 1).astype(int)
    margin = np.minimum(np.abs(px - np.round(px)) / np.maximum(px, 1.0), np.abs(py - np.round(py)) / np.maximum(py, 1.0))
    t0, zc = tz[ny, nx, :3], tz[ny, nx, 3]
    n0, r0 = nr[ny, nx, :3], nr[ny, nx, 3]
    surface = np.isfinite(zc)
    # the miss pixels: spec S17 on the staged colour (a miss is not demodulated, so its staged colour is S17's)
    prev17 = None if prev is None else (prev[0], prev[2])
    s17 = upscale_staged(tz, mv, color[..., 3], prev17, out_size, jitter, max_a)
    # step 2
    ap = np.zeros((H, W))
    hc = np.zeros((H, W, 3))
    if prev is not None:
        ze = zc + mv[ny, nx, 2]
        hs, m_s = history_tap(prev, cx + mv[ny, nx, 0] * sx, cy + mv[ny, nx, 1] * sy, ze, n0, out_size)
        vm = virt[ny, nx]
        hv, m_v = history_tap(prev, cx + vm[..., 0] * sx, cy + vm[..., 1] * sy, ze, n0, out_size)
        use_v = (vm[..., 2] > 0) & (hv[..., 3] > 0)
        both = use_v & (hs[..., 3] > 0)
        only = use_v & ~(hs[..., 3] > 0)
        mixed = hs + (hv - hs) * vm[..., 2:3]
        alone = np.concatenate([hv[..., :3], (vm[..., 2] * hv[..., 3])[..., None]], axis=-1)
        hsel = np.where(both[..., None], mixed, np.where(only[..., None], alone, hs))
        ap, hc = hsel[..., 3], hsel[..., :3]
        margin = np.minimum(margin, np.where(vm[..., 2] > 0, np.minimum(m_s, m_v), m_s))
    # step 3
    narrow = np.minimum(ap * LONG_HISTORY, 1.0)
    iz = 1.0 / np.maximum(DEPTH_EDGE * np.where(surface, zc, 1.0), DEPTH_EDGE_MIN)
    sw, sww, cov = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    m1, m1w, m2w = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ix, iy = nx + dx, ny + dy
            inb = (ix >= 0) & (iy >= 0) & (ix < w) & (iy < h)
            kx, ky = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
            zk = tz[ky, kx, 3]
            ok = inb & np.isfinite(zk)
            ddx, ddy = (ix + 0.5 - jx) - px, (iy + 0.5 - jy) - py
            x2, y2 = ddx * ddx, ddy * ddy
            wide = np.maximum(0.0, 1.0 - x2 * WIDE_INV_R2) ** 2 * np.maximum(0.0, 1.0 - y2 * WIDE_INV_R2) ** 2
            if abs(dx) <= 1 and abs(dy) <= 1:
                lan = np.maximum(0.0, up.lanczos(x2)) * np.maximum(0.0, up.lanczos(y2))
                k = np.maximum(0.0, 1.0 - np.abs(ddx) * sx) * np.maximum(0.0, 1.0 - np.abs(ddy) * sy)
                cov = np.where(ok, np.maximum(cov, k), cov)
            else:
                lan = 0.0
            ks = wide + narrow * (lan - wide)
            with np.errstate(invalid="ignore"):
                wz = np.maximum(0.0, 1.0 - np.abs(np.where(ok, zk, 0.0) - np.where(surface, zc, 0.0)) * iz)
            wn = np.clip(((nr[ky, kx, :3] * n0).sum(axis=-1) - NORMAL_EDGE) * NORMAL_SCALE, 0.0, 1.0)
            wr = np.maximum(0.0, 1.0 - np.abs(nr[ky, kx, 3] - r0) * ROUGHNESS_EDGE)
            edge = wz * wn * wr
            wt, ww = np.where(ok, ks * edge, 0.0), np.where(ok, wide * edge, 0.0)
            delta = tz[ky, kx, :3] - t0
            sw += wt
            m1 += wt[..., None] * delta
            sww += ww
            m1w += ww[..., None] * delta
            m2w += ww[..., None] * delta * delta
    # step 4: the resampled colour from the mixed kernel, mean and deviation from the wide one
    small, smallw = ~(sw > up.WEIGHT_MIN), ~(sww > up.WEIGHT_MIN)
    margin = np.minimum(margin, np.minimum(np.abs(sw - up.WEIGHT_MIN), np.abs(sww - up.WEIGHT_MIN)))
    u = np.where(small[..., None], t0, t0 + m1 / np.where(small, 1.0, sw)[..., None])
    inv = 1.0 / np.where(smallw, 1.0, sww)
    e = m1w * inv[..., None]
    second = m2w * inv[..., None]
    var = second - e * e
    mean = np.where(smallw[..., None], t0, t0 + e)
    sigma = np.where(smallw[..., None], 0.0, np.sqrt(np.maximum(var, 0.0)))
    kappa = np.clip(cov, up.COVERAGE_MIN, 1.0)
    # steps 5-6
    accepted = ap > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        # the floor of the variance: where the history is clipped, sigma's fp32 error grows as the variance falls against the second moment
        rel = np.where(second > 0, var / np.where(second > 0, second, 1.0), np.inf).min(axis=-1)
    margin = np.where(accepted & ~smallw, np.minimum(margin, rel), margin)
    lo, hi = mean - CLIP_SIGMA * sigma, mean + CLIP_SIGMA * sigma
    hcl = np.minimum(np.maximum(hc, lo), hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = (kappa / (kappa + ap))[..., None]
    t_out = np.where(accepted[..., None], hcl + (u - hcl) * alpha, u)
    a_out = np.where(accepted, np.minimum(ap + kappa, max_a), kappa)
    A = albedo(da, sa)[ny, nx]
    out = np.concatenate([up.from_t(t_out) * A, color[ny, nx, 3:4]], axis=-1)
    hist = np.concatenate([t_out, a_out[..., None]], axis=-1)
    s = surface
    return dict(out=np.where(s[..., None], out, s17["out"]), hist=np.where(s[..., None], hist, s17["hist"]),
                hist_n=np.where(s[..., None], nr[ny, nx], 0.0), z=np.where(s, zc, s17["z"]), surface=s,
                accepted=np.where(s, accepted, s17["accepted"]), margin=np.where(s, margin, s17["margin"]), kappa=np.where(s, kappa, s17["kappa"]),
                sigma=sigma, mean=mean)


def upscale_staged(tz, velocity, alpha, prev, out_size, jitter, max_a):
    """spec S17 from its step 2 on, over colour that is already staged (t-space, depth in .w): upscale_reference.upscale with its step 1
    undone first, so that the restatement of S17 stays in one place"""
    tz = np.asarray(tz, np.float64)
    color = np.concatenate([up.from_t(tz[..., :3]), np.asarray(alpha, np.float64)[..., None]], axis=-1)
    return up.upscale(color, tz[..., 3], velocity, prev, out_size, jitter, max_a)


def reconstruct(tex, cam, prev, out_size, jitter=(0.0, 0.0), max_a=16.0):
    """One call of S21: prepare, then resolve"""
    prep = prepare(tex, cam, jitter)
    res = resolve(tex, prep, prev, out_size, jitter, max_a)
    res["prep"] = prep
    return res
