"""A float64 numpy restatement of DESIGN.md spec S31 (pt_chromatic_aberration), written from the spec text for tests/
test_chromatic_aberration.py.  It starts from the same fp32 inputs as the header -- the fp32 image, the fp32 offsets and the fp32
products fx = FocusUV.x W, fy = FocusUV.y H -- and evaluates everything after them in float64."""
import numpy as np

MAX_RADIANCE = 65504.0
MAX_OFFSET = 1.0 / 16.0
DEFAULT_FOCUS_UV = (0.5, 0.5)
DEFAULT_OFFSETS = (0.003, 0.003, -0.003)
EPS32 = 2.0 ** -24  # fp32 unit roundoff


def sanitize(c):
    """NaN -> 0, else clamped to [0, 65504]; float64"""
    c = np.asarray(c, np.float64)
    return np.where(np.isnan(c), 0.0, np.clip(c, 0.0, MAX_RADIANCE))


def focus_texels(w, h, focus_uv):
    """fx, fy as the host makes them: one fp32 product each"""
    return float(np.float32(focus_uv[0]) * np.float32(w)), float(np.float32(focus_uv[1]) * np.float32(h))


def positions(n, f, k):
    """sample positions of the coordinates 0 .. n - 1 along one axis -> (s, p): s = x + p, p = ((x + 0.5) - f) k"""
    x = np.arange(n, dtype=np.float64)
    p = ((x + 0.5) - f) * k
    return x + p, p


def position_error(s, p):
    """how far the fp32 evaluation of s may lie from the float64 one: d = (x + 0.5) - f, p = d k and s = x + p round once each, a relative
    2^-24 at most, and d's rounding reaches s through p: |error| <= eps (2 |p| + |s|), with second-order room"""
    return EPS32 * (2.0 * np.abs(p) + np.abs(s)) * (1.0 + 2.0 ** -20)


def aberrate(color, focus_uv=DEFAULT_FOCUS_UV, offsets=DEFAULT_OFFSETS):
    """-> dict: out (h, w, 3) float64; per channel and texel, for the rounding bound: err_pos (the position error of sx plus that of sy),
    tap_range and tap_max (the largest difference among, and the largest of, the taps of every cell the position may fall into within
    its error: the four taps of the spec, and their neighbours one further where a floor may fall the other way in fp32); unclamped
    (no tap of the cell was clamped)"""
    color = np.asarray(color, np.float32)
    h, w = color.shape[:2]
    fx, fy = focus_texels(w, h, focus_uv)
    rgb = sanitize(color[..., :3])
    out = np.empty((h, w, 3), np.float64)
    err_pos, tap_range, tap_max = np.empty((h, w, 3)), np.empty((h, w, 3)), np.empty((h, w, 3))
    unclamped = np.empty((h, w, 3), bool)
    for ch in range(3):
        k = float(np.float32(offsets[ch]))
        plane = rgb[..., ch]
        sx, px = positions(w, fx, k)
        sy, py = positions(h, fy, k)
        ix, iy = np.floor(sx), np.floor(sy)
        tx, ty = (sx - ix)[None, :], (sy - iy)[:, None]
        ix, iy = ix.astype(np.int64), iy.astype(np.int64)

        def tap(jy, jx):
            return plane[np.clip(jy, 0, h - 1)[:, None], np.clip(jx, 0, w - 1)[None, :]]

        a, b, c, d = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
        out[..., ch] = (a * (1.0 - tx) + b * tx) * (1.0 - ty) + (c * (1.0 - tx) + d * tx) * ty
        ex, ey = position_error(sx, px), position_error(sy, py)
        err_pos[..., ch] = ex[None, :] + ey[:, None]
        # the columns (rows) of every cell that [s - e, s + e] meets: from floor(s - e) to floor(s + e) + 1, three at most
        cols = [np.floor(sx - ex).astype(np.int64), np.floor(sx - ex).astype(np.int64) + 1, np.floor(sx + ex).astype(np.int64) + 1]
        rows = [np.floor(sy - ey).astype(np.int64), np.floor(sy - ey).astype(np.int64) + 1, np.floor(sy + ey).astype(np.int64) + 1]
        taps = np.stack([tap(r, c_) for r in rows for c_ in cols])
        tap_range[..., ch] = taps.max(axis=0) - taps.min(axis=0)
        tap_max[..., ch] = taps.max(axis=0)
        unclamped[..., ch] = ((iy >= 0) & (iy + 1 <= h - 1))[:, None] & ((ix >= 0) & (ix + 1 <= w - 1))[None, :]
    return dict(out=out, err_pos=err_pos, tap_range=tap_range, tap_max=tap_max, unclamped=unclamped, fx=fx, fy=fy)
