"""Independent float64 numpy restatement of DESIGN.md spec S15 (row N9, the NRD stand-in pt_nrd_denoise), written from the spec text,
not from csrc/pt_denoise.h.  Images are numpy arrays (h, w, k); every pass takes the previous pass's results as arrays, so a test can
feed each pass the host header's fp32 output of the one before and compare pass by pass.  exp is numpy's (the header's exp2_spec
differs from it by ~1e-7 relative)."""
import numpy as np

REBLUR, RELAX = 2, 3
DEPTH_REL, NORMAL_MIN, WEIGHT_MIN, SPATIAL_BELOW = 0.05, 0.9, 1e-3, 4.0
SIGMA_Z, EPS_Z, SIGMA_L, EPS_L, ROUGH_DEN = 1.0, 1e-3, 4.0, 1e-4, 0.1 + 1e-6
BSPLINE = {0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
GAUSS = {0: 1 / 2, 1: 1 / 4}


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def from_ycocg(c):
    y, co, cg = c[..., 0], c[..., 1], c[..., 2]
    rgb = np.stack([y - cg + co, y + cg, y - cg - co], axis=-1)
    return np.where(np.isnan(rgb), 0.0, np.maximum(rgb, 0.0))


def to_ycocg(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([0.25 * r + 0.5 * g + 0.25 * b, 0.5 * r - 0.5 * b, -0.25 * r + 0.5 * g - 0.25 * b], axis=-1)


def decode(mode, v):
    v = np.asarray(v, np.float64)
    return from_ycocg(v[..., :3]) if mode == REBLUR else v[..., :3].copy()


def shift(a, dx, dy, fill=np.nan):
    """out[y, x] = a[y + dy, x + dx] where inside, else fill"""
    a = np.asarray(a, np.float64)
    h, w = a.shape[:2]
    out = np.full(a.shape, fill, np.float64)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
    return out


def hit_at(z, dx, dy):
    return np.isfinite(shift(z, dx, dy, np.nan))


def grad(z):
    """per axis, of the one-sided differences towards hit neighbours inside the image the one of smaller magnitude (backward on a tie)"""
    z = np.asarray(z, np.float64)
    out = []
    for (mx, my), (px, py) in (((-1, 0), (1, 0)), ((0, -1), (0, 1))):
        hm, hp = hit_at(z, mx, my), hit_at(z, px, py)
        with np.errstate(invalid="ignore"):
            dm, dp = z - shift(z, mx, my), shift(z, px, py) - z
        both = np.where(np.abs(dp) < np.abs(dm), dp, dm)
        out.append(np.where(hm & hp, both, np.where(hm, dm, np.where(hp, dp, 0.0))))
    return out


def w_z(zp, zq, gx, gy, ox, oy):
    with np.errstate(all="ignore"):
        return np.exp(-np.abs(zp - zq) / (SIGMA_Z * np.abs(gx * ox + gy * oy) + EPS_Z))


def w_n(n, m):
    return np.maximum((n * m).sum(axis=-1), 0.0) ** 128


def w_r(r, q):
    return np.exp(-np.abs(r - q) / ROUGH_DEN)


def temporal(mode, z, mv, nr, ind, ins, prev, max_d, max_s):
    """pass (a).  prev: None (restart) or dict sig_d, sig_s, mom, guide (h, w, 4) of the previous call.  -> dict sig_d, sig_s, mom,
    guide (misses: zeros, their depth in the guide) and hitd (h, w, 2)"""
    z = np.asarray(z, np.float64)
    h, w = z.shape
    hit = np.isfinite(z)
    nr, ind, ins, mv = (np.asarray(a, np.float64) for a in (nr, ind, ins, mv))
    n = nr[..., :3]
    cur = [decode(mode, ind), decode(mode, ins)]
    raw_w = [ind[..., 3], ins[..., 3]]
    any_n = np.zeros((h, w), bool)
    lmax = [np.full((h, w), -np.inf), np.full((h, w), -np.inf)]
    hsum = [np.zeros((h, w)), np.zeros((h, w))]
    hcnt = [np.zeros((h, w)), np.zeros((h, w))]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q_hit = hit_at(z, dx, dy)
            any_n |= q_hit
            with np.errstate(invalid="ignore"):
                near = q_hit & (np.abs(shift(z, dx, dy) - z) <= DEPTH_REL * np.abs(z))
            for k, src in enumerate((ind, ins)):
                q = shift(src, dx, dy, 0.0)
                lmax[k] = np.where(q_hit, np.maximum(lmax[k], lum(decode(mode, q))), lmax[k])
                use = near & (q[..., 3] != 0)
                hsum[k] += np.where(use, q[..., 3], 0.0)
                hcnt[k] += use
    hitd = [np.where((raw_w[k] == 0) & (hcnt[k] > 0), hsum[k] / np.maximum(hcnt[k], 1), raw_w[k]) for k in range(2)]
    for k in range(2):
        lk = lum(cur[k])
        clamp = any_n & (lk > lmax[k])
        with np.errstate(all="ignore"):
            cur[k] = np.where(clamp[..., None], cur[k] * (lmax[k] / lk)[..., None], cur[k])
    # reprojection
    sw = np.zeros((h, w))
    hist = [np.zeros((h, w, 3)), np.zeros((h, w, 3))]
    hlen = [np.zeros((h, w)), np.zeros((h, w))]
    hmom = np.zeros((h, w, 4))
    if prev is not None:
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        fx, fy, ze = xs + mv[..., 0], ys + mv[..., 1], z + mv[..., 2]
        with np.errstate(invalid="ignore"):
            ok = hit & (fx > -1) & (fy > -1) & (fx < w) & (fy < h)
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        g = np.asarray(prev["guide"], np.float64)
        for kx in (0, 1):
            for ky in (0, 1):
                qx, qy = x0.astype(int) + kx, y0.astype(int) + ky
                inside = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                gq = g[qyc, qxc]
                with np.errstate(invalid="ignore"):
                    valid = inside & np.isfinite(gq[..., 0]) & (np.abs(gq[..., 0] - ze) <= DEPTH_REL * np.abs(ze)) & ((gq[..., 1:] * n).sum(-1) >= NORMAL_MIN)
                wt = np.where(valid, (tx if kx else 1 - tx) * (ty if ky else 1 - ty), 0.0)
                sw += wt
                for k, name in enumerate(("sig_d", "sig_s")):
                    p = np.asarray(prev[name], np.float64)[qyc, qxc]
                    hist[k] += np.where(valid[..., None], p[..., :3] * wt[..., None], 0.0)
                    hlen[k] += np.where(valid, p[..., 3] * wt, 0.0)
                hmom += np.where(valid[..., None], np.asarray(prev["mom"], np.float64)[qyc, qxc] * wt[..., None], 0.0)
    has = sw >= WEIGHT_MIN
    inv = np.where(has, 1.0 / np.where(has, sw, 1.0), 0.0)
    hist = [hk * inv[..., None] for hk in hist]
    hlen = [lk * inv for lk in hlen]
    hmom = hmom * inv[..., None]
    caps = [np.full((h, w), float(max_d)), np.maximum(1.0, np.floor(max_s * np.clip(nr[..., 3] / 0.5, 0.0, 1.0) + 0.5))]
    out = dict(hitd=np.stack(hitd, axis=-1))
    mom = np.zeros((h, w, 4))
    for k, name in enumerate(("sig_d", "sig_s")):
        nk = np.minimum(hlen[k] + 1.0, caps[k])
        a = 1.0 / nk
        c = hist[k] + (cur[k] - hist[k]) * a[..., None]
        lk = lum(cur[k])
        mom[..., 2 * k] = hmom[..., 2 * k] + (lk - hmom[..., 2 * k]) * a
        mom[..., 2 * k + 1] = hmom[..., 2 * k + 1] + (lk * lk - hmom[..., 2 * k + 1]) * a
        out[name] = np.where(hit[..., None], np.concatenate([c, nk[..., None]], axis=-1), 0.0)
    out["mom"] = np.where(hit[..., None], mom, 0.0)
    out["guide"] = np.where(hit[..., None], np.concatenate([z[..., None], n], axis=-1), np.stack([z] + [np.zeros_like(z)] * 3, axis=-1))
    return out


def variance(z, nr, sig_d, sig_s, mom):
    """pass (b) -> (xd, xs): (accumulated RGB, variance); misses NaN (not written)"""
    z, nr, sig_d, sig_s, mom = (np.asarray(a, np.float64) for a in (z, nr, sig_d, sig_s, mom))
    hit = np.isfinite(z)
    gx, gy = grad(z)
    sums = np.zeros(z.shape + (6,))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            q_hit = hit_at(z, dx, dy)
            wgt = np.where(q_hit, w_z(z, shift(z, dx, dy, 0.0), gx, gy, dx, dy) * w_n(nr[..., :3], shift(nr[..., :3], dx, dy, 0.0)), 0.0)
            ws = wgt * w_r(nr[..., 3], shift(nr[..., 3], dx, dy, 0.0))
            mq = shift(mom, dx, dy, 0.0)
            for k, (wk, c) in enumerate(((wgt, mq[..., 0]), (wgt, mq[..., 1]), (wgt, 1.0), (ws, mq[..., 2]), (ws, mq[..., 3]), (ws, 1.0))):
                sums[..., k] += wk * c
    out = []
    for k, sig in enumerate((sig_d, sig_s)):
        s1, s2, sw = sums[..., 3 * k], sums[..., 3 * k + 1], sums[..., 3 * k + 2]
        with np.errstate(all="ignore"):
            a, c = np.where(sw > 0, s1 / sw, 0.0), np.where(sw > 0, s2 / sw, 0.0)
        spatial = np.maximum(c - a * a, 0.0)
        temporal_v = np.maximum(mom[..., 2 * k + 1] - mom[..., 2 * k] ** 2, 0.0)
        v = np.where(sig[..., 3] < SPATIAL_BELOW, spatial, temporal_v)
        out.append(np.where(hit[..., None], np.concatenate([sig[..., :3], v[..., None]], axis=-1), np.nan))
    return out[0], out[1]


def atrous(mode, z, nr, xd, xs, step, last, hitd=None):
    """one a-trous step -> (xd', xs') or, with `last`, (OutDiffuse, OutSpecular) in the mode's encoding with hitd in .w; misses NaN"""
    z, nr, xd, xs = (np.asarray(a, np.float64) for a in (z, nr, xd, xs))
    hit = np.isfinite(z)
    xd, xs = (np.where(hit[..., None], x, 0.0) for x in (xd, xs))  # (a miss's values are never taps)
    gx, gy = grad(z)
    gk, gv = np.zeros(z.shape), [np.zeros(z.shape), np.zeros(z.shape)]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            kk = np.where(hit_at(z, dx, dy), GAUSS[abs(dy)] * GAUSS[abs(dx)], 0.0)
            gk += kk
            for k, x in enumerate((xd, xs)):
                gv[k] += kk * shift(x[..., 3], dx, dy, 0.0)
    with np.errstate(all="ignore"):
        den = [SIGMA_L * np.sqrt(g / gk) + EPS_L for g in gv]
    lp = [lum(xd[..., :3]), lum(xs[..., :3])]
    sw = [np.zeros(z.shape), np.zeros(z.shape)]
    acc = [np.zeros(z.shape + (3,)), np.zeros(z.shape + (3,))]
    var = [np.zeros(z.shape), np.zeros(z.shape)]
    for ty in range(-2, 3):
        for tx in range(-2, 3):
            ox, oy = tx * step, ty * step
            q_hit = hit_at(z, ox, oy)
            base = BSPLINE[abs(ty)] * BSPLINE[abs(tx)] * w_z(z, shift(z, ox, oy, 0.0), gx, gy, ox, oy) * w_n(nr[..., :3], shift(nr[..., :3], ox, oy, 0.0))
            wr = w_r(nr[..., 3], shift(nr[..., 3], ox, oy, 0.0))
            for k, x in enumerate((xd, xs)):
                q = shift(x, ox, oy, 0.0)
                with np.errstate(all="ignore"):
                    wk = base * np.exp(-np.abs(lp[k] - lum(q[..., :3])) / den[k])
                if k == 1:  # specular: w_r, and off the centre the strength saturate(r_p / 0.5)
                    wk = wk * wr * (1.0 if tx == 0 and ty == 0 else np.clip(nr[..., 3] / 0.5, 0.0, 1.0))
                wk = np.where(q_hit & hit, wk, 0.0)
                sw[k] += wk
                acc[k] += (q[..., :3] - x[..., :3]) * wk[..., None]
                var[k] += wk * wk * q[..., 3]
    out = []
    for k, x in enumerate((xd, xs)):
        with np.errstate(all="ignore"):
            c = np.where((sw[k] > 0)[..., None], x[..., :3] + acc[k] / sw[k][..., None], x[..., :3])
            v = np.where(sw[k] > 0, var[k] / sw[k] ** 2, x[..., 3])
        if last:
            enc = to_ycocg(c) if mode == REBLUR else c
            r = np.concatenate([enc, np.asarray(hitd, np.float64)[..., k:k + 1]], axis=-1)
        else:
            r = np.concatenate([c, v[..., None]], axis=-1)
        out.append(np.where(hit[..., None], r, np.nan))
    return out[0], out[1]
