"""Independent float64 numpy restatement of DESIGN.md spec S32 (row N30, the ReBLUR stand-in pt_nrd_reblur), written from the spec text,
not from csrc/pt_reblur.h.  Images are numpy arrays (h, w, k); every pass takes the previous pass's results as arrays, so a test can
feed each pass the host header's fp32 output of the one before and compare pass by pass.  exp is numpy's.  Every pass also returns
`fragile`: the pixels where this restatement alone sees a compare of the spec (a validity test, the history-fix threshold, the rounding
of the specular cap, a tap's rounding to the nearest pixel) decided by a margin below what fp32 can resolve."""
import numpy as np

from denoise_reference import DEPTH_REL, NORMAL_MIN, WEIGHT_MIN, grad, hit_at, shift, w_n, w_r, w_z

ROUGH_FULL, MOTION, FIX_STRIDE, CLAMP_SIGMA, SIGMA_H, EPS_H = 0.5, 2.0, 2, 2.0, 1.0, 0.1
DISC = [(np.sqrt((k + 0.5) / 8.0) * np.cos(k * 2.399963229728653), np.sqrt((k + 0.5) / 8.0) * np.sin(k * 2.399963229728653)) for k in range(8)]
EPS32 = 2.0 ** -23


def near(a, b, scale=None, ulps=16.0):
    """|a - b| below `ulps` fp32 roundings of the larger magnitude (or of `scale`)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.maximum(np.abs(a), np.abs(b)) if scale is None else scale
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) <= ulps * EPS32 * np.maximum(s, 1e-30)


def spec_cap(max_n, rough, mx, my):
    """-> (cap, fragile)"""
    c15 = np.maximum(1.0, np.floor(max_n * np.clip(rough / ROUGH_FULL, 0.0, 1.0) + 0.5))
    m = np.sqrt(mx * mx + my * my)
    v = c15 + (max_n - c15) / (1.0 + MOTION * m) + 0.5
    v15 = max_n * np.clip(rough / ROUGH_FULL, 0.0, 1.0) + 0.5
    fragile = near(v, np.round(v), scale=np.abs(v)) | near(v15, np.round(v15), scale=np.abs(v15))
    return np.maximum(1.0, np.floor(v)), fragile


def radius(rmin, rmax, n, a):
    with np.errstate(all="ignore"):
        return np.clip(rmax * np.sqrt(a / n), rmin, rmax)


def temporal(z, mv, nr, ind, ins, prev, max_n, max_fast):
    """pass (a).  prev: None (restart) or dict slow_d, slow_s, fast_d, fast_s, guide of the previous call -> dict x_d, x_s (slow signal,
    hit distance), fast_d, fast_s (fast signal, n), guide, fragile"""
    z = np.asarray(z, np.float64)
    h, w = z.shape
    hit = np.isfinite(z)
    nr, ind, ins, mv = (np.asarray(a, np.float64) for a in (nr, ind, ins, mv))
    n = nr[..., :3]
    src = (ind, ins)
    cur = [ind[..., :3].copy(), ins[..., :3].copy()]
    any_n = np.zeros((h, w), bool)
    ymax = [np.full((h, w), -np.inf), np.full((h, w), -np.inf)]
    hsum, hcnt = [np.zeros((h, w)), np.zeros((h, w))], [np.zeros((h, w)), np.zeros((h, w))]
    fragile = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q_hit = hit_at(z, dx, dy)
            any_n |= q_hit
            with np.errstate(invalid="ignore"):
                dz = np.abs(shift(z, dx, dy) - z)
                nearz = q_hit & (dz <= DEPTH_REL * np.abs(z))
                fragile |= q_hit & hit & near(dz, DEPTH_REL * np.abs(z), scale=np.abs(z))
            for k in range(2):
                q = shift(src[k], dx, dy, 0.0)
                ymax[k] = np.where(q_hit, np.maximum(ymax[k], q[..., 0]), ymax[k])
                use = nearz & (q[..., 3] != 0)
                hsum[k] += np.where(use, q[..., 3], 0.0)
                hcnt[k] += use
    hitd = [np.where((src[k][..., 3] == 0) & (hcnt[k] > 0), hsum[k] / np.maximum(hcnt[k], 1), src[k][..., 3]) for k in range(2)]
    for k in range(2):
        yk = cur[k][..., 0]
        clamp = any_n & (yk > ymax[k])
        with np.errstate(all="ignore"):
            cur[k] = np.where(clamp[..., None], cur[k] * (ymax[k] / yk)[..., None], cur[k])
    sw = np.zeros((h, w))
    slow, fast = [np.zeros((h, w, 3)), np.zeros((h, w, 3))], [np.zeros((h, w, 3)), np.zeros((h, w, 3))]
    hlen = [np.zeros((h, w)), np.zeros((h, w))]
    if prev is not None:
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        fx, fy, ze = xs + mv[..., 0], ys + mv[..., 1], z + mv[..., 2]
        with np.errstate(invalid="ignore"):
            ok = hit & (fx > -1) & (fy > -1) & (fx < w) & (fy < h)
        for v, lim in ((fx, -1.0), (fy, -1.0), (fx, float(w)), (fy, float(h))):
            fragile |= hit & near(v, lim, scale=np.maximum(np.abs(v), 1.0))
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        g = np.asarray(prev["guide"], np.float64)
        for ky in (0, 1):
            for kx in (0, 1):
                qx, qy = x0.astype(int) + kx, y0.astype(int) + ky
                inside = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                gq = g[qyc, qxc]
                with np.errstate(invalid="ignore"):
                    dz, dn = np.abs(gq[..., 0] - ze), (gq[..., 1:] * n).sum(-1)
                    fin = inside & np.isfinite(gq[..., 0])
                    valid = fin & (dz <= DEPTH_REL * np.abs(ze)) & (dn >= NORMAL_MIN)
                    fragile |= fin & (near(dz, DEPTH_REL * np.abs(ze), scale=np.abs(ze)) | near(dn, NORMAL_MIN, scale=1.0))
                wt = np.where(valid, (tx if kx else 1 - tx) * (ty if ky else 1 - ty), 0.0)
                sw += wt
                for k in range(2):
                    ps = np.asarray(prev[("slow_d", "slow_s")[k]], np.float64)[qyc, qxc]
                    pf = np.asarray(prev[("fast_d", "fast_s")[k]], np.float64)[qyc, qxc]
                    slow[k] += np.where(valid[..., None], ps[..., :3] * wt[..., None], 0.0)
                    fast[k] += np.where(valid[..., None], pf[..., :3] * wt[..., None], 0.0)
                    hlen[k] += np.where(valid, pf[..., 3] * wt, 0.0)
        fragile |= hit & near(sw, WEIGHT_MIN, scale=1.0)
    has = sw >= WEIGHT_MIN
    inv = np.where(has, 1.0 / np.where(has, sw, 1.0), 0.0)
    cap_s, frag_cap = spec_cap(max_n, nr[..., 3], mv[..., 0], mv[..., 1])
    fragile |= hit & frag_cap
    caps = [np.full((h, w), float(max_n)), cap_s]
    out = {}
    for k, (xn, fn) in enumerate((("x_d", "fast_d"), ("x_s", "fast_s"))):
        hs, hf, hl = slow[k] * inv[..., None], fast[k] * inv[..., None], hlen[k] * inv
        nk = np.minimum(hl + 1.0, caps[k])
        nf = np.minimum(nk, float(max_fast))
        cs = hs + (cur[k] - hs) / nk[..., None]
        cf = hf + (cur[k] - hf) / nf[..., None]
        out[xn] = np.where(hit[..., None], np.concatenate([cs, hitd[k][..., None]], axis=-1), 0.0)
        out[fn] = np.where(hit[..., None], np.concatenate([cf, nk[..., None]], axis=-1), 0.0)
    out["guide"] = np.where(hit[..., None], np.concatenate([z[..., None], n], axis=-1), np.stack([z] + [np.zeros_like(z)] * 3, axis=-1))
    out["fragile"] = fragile & hit
    return out


def fix(z, nr, x_d, x_s, fast_d, fast_s, fix_frames):
    """pass (b) -> (slow_d, slow_s, fragile); misses NaN (pass (b) does not write them)"""
    z, nr, x_d, x_s, fast_d, fast_s = (np.asarray(a, np.float64) for a in (z, nr, x_d, x_s, fast_d, fast_s))
    hit = np.isfinite(z)
    gx, gy = grad(z)
    sp = np.clip(nr[..., 3] / ROUGH_FULL, 0.0, 1.0)
    xs_, fs_ = (x_d, x_s), (fast_d, fast_s)
    sw = [np.zeros(z.shape), np.zeros(z.shape)]
    acc = [np.zeros(z.shape + (3,)), np.zeros(z.shape + (3,))]
    h, w = z.shape
    ys, xs = np.mgrid[0:h, 0:w]
    frag_tap = np.zeros(z.shape, bool)
    for ty in range(-2, 3):
        for tx in range(-2, 3):
            ox, oy = tx * FIX_STRIDE, ty * FIX_STRIDE
            # diffuse: the tap at (ox, oy)
            q_hit = hit_at(z, ox, oy) & hit
            wk = w_z(z, shift(z, ox, oy, 0.0), gx, gy, ox, oy) * w_n(nr[..., :3], shift(nr[..., :3], ox, oy, 0.0)) * shift(fs_[0][..., 3], ox, oy, 0.0)
            wk = np.where(q_hit, wk, 0.0)
            sw[0] += wk
            acc[0] += (np.where(q_hit[..., None], shift(xs_[0][..., :3], ox, oy, 0.0), 0.0) - xs_[0][..., :3]) * wk[..., None]
            # specular: the offset scaled by saturate(r / 0.5), rounded to the nearest pixel; off the centre, the centre is no tap
            vx, vy = ox * sp, oy * sp
            for v in (vx, vy):
                frag_tap |= np.abs(v + 0.5 - np.round(v + 0.5)) <= 8.0 * EPS32 * 4.0
            sx, sy = np.floor(vx + 0.5).astype(int), np.floor(vy + 0.5).astype(int)
            qx, qy = xs + sx, ys + sy
            inside = hit & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
            if tx != 0 or ty != 0:
                inside &= (sx != 0) | (sy != 0)
            qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            zq = z[qyc, qxc]
            tap = inside & np.isfinite(zq)
            nq = nr[qyc, qxc]
            wk = w_z(z, np.where(tap, zq, 0.0), gx, gy, sx, sy) * w_n(nr[..., :3], nq[..., :3]) * w_r(nr[..., 3], nq[..., 3]) * fs_[1][qyc, qxc][..., 3]
            wk = np.where(tap, wk, 0.0)
            sw[1] += wk
            acc[1] += np.where(tap[..., None], xs_[1][qyc, qxc][..., :3] - xs_[1][..., :3], 0.0) * wk[..., None]
    cnt = np.zeros(z.shape)
    s1, s2 = [np.zeros(z.shape + (3,)) for _ in range(2)], [np.zeros(z.shape + (3,)) for _ in range(2)]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q_hit = hit_at(z, dx, dy) & hit
            cnt += q_hit
            for k in range(2):
                f = np.where(q_hit[..., None], shift(fs_[k][..., :3], dx, dy, 0.0), 0.0)
                s1[k] += f
                s2[k] += f * f
    out = []
    fragile = np.zeros(z.shape, bool)
    for k in range(2):
        nk = fs_[k][..., 3]
        short = nk + 0.5 < fix_frames
        fragile |= hit & near(nk + 0.5, float(fix_frames))
        if k == 1:
            fragile |= short & frag_tap
        with np.errstate(all="ignore"):
            fixed = np.where((short & (sw[k] > 0))[..., None], xs_[k][..., :3] + acc[k] / sw[k][..., None], xs_[k][..., :3])
            m = s1[k] / cnt[..., None]
            sig = CLAMP_SIGMA * np.sqrt(np.maximum(s2[k] / cnt[..., None] - m * m, 0.0))
        c = np.minimum(np.maximum(fixed, m - sig), m + sig)
        out.append(np.where(hit[..., None], np.concatenate([c, xs_[k][..., 3:4]], axis=-1), np.nan))
    return out[0], out[1], fragile & hit


def rotation(k):
    a = 2.0 * np.pi * (k % 16) / 16.0
    return np.cos(a), np.sin(a)


def blur(z, nr, src_d, src_s, fast_d, fast_s, frame, post, rmin, rmax):
    """pass (c) (post = False) or (d) (post = True) -> (d', s', fragile, (radius_d, radius_s)); misses NaN"""
    z, nr, src_d, src_s, fast_d, fast_s = (np.asarray(a, np.float64) for a in (z, nr, src_d, src_s, fast_d, fast_s))
    h, w = z.shape
    hit = np.isfinite(z)
    gx, gy = grad(z)
    ys, xs = np.mgrid[0:h, 0:w]
    rc, rs = rotation((xs & 3) + 4 * (ys & 3) + int(frame) + (8 if post else 0))
    sp = np.clip(nr[..., 3] / ROUGH_FULL, 0.0, 1.0)
    nsafe = [np.where(hit, f[..., 3], 1.0) for f in (fast_d, fast_s)]
    rad = [radius(rmin, rmax, nsafe[0], src_d[..., 3]), sp * radius(rmin, rmax, nsafe[1], src_s[..., 3])]
    out = []
    fragile = np.zeros((h, w), bool)
    for k, src in enumerate((src_d, src_s)):
        src = np.where(hit[..., None], src, 0.0)
        sw = np.ones((h, w))
        acc = np.zeros((h, w, 3))
        inv_h = 1.0 / (SIGMA_H * src[..., 3] + EPS_H)
        for px, py in DISC:
            vx, vy = (px * rc - py * rs) * rad[k], (px * rs + py * rc) * rad[k]
            for v in (vx, vy):
                fragile |= np.abs(v + 0.5 - np.round(v + 0.5)) <= 8.0 * EPS32 * np.maximum(rad[k], 1.0)
            ox, oy = np.floor(vx + 0.5).astype(int), np.floor(vy + 0.5).astype(int)
            qx, qy = xs + ox, ys + oy
            inside = hit & ((ox != 0) | (oy != 0)) & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
            qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            zq = z[qyc, qxc]
            tap = inside & np.isfinite(zq)
            nq, e = nr[qyc, qxc], src[qyc, qxc]
            wk = w_z(z, np.where(tap, zq, 0.0), gx, gy, ox, oy) * w_n(nr[..., :3], nq[..., :3])
            if k == 1:
                wk = wk * w_r(nr[..., 3], nq[..., 3])
            wk = wk * np.exp(-np.abs(src[..., 3] - e[..., 3]) * inv_h)
            wk = np.where(tap, wk, 0.0)
            sw += wk
            acc += np.where(tap[..., None], e[..., :3] - src[..., :3], 0.0) * wk[..., None]
        c = src[..., :3] + acc / sw[..., None]
        out.append(np.where(hit[..., None], np.concatenate([c, src[..., 3:4]], axis=-1), np.nan))
    return out[0], out[1], fragile & hit, rad
