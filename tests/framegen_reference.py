"""Spec S19 -- the frame-interpolation stand-in of row N13 -- restated in float64 numpy, written from the spec's
text and not from csrc/pt_framegen.h: the scatter as four np.minimum.at passes, the gather for every output pixel at once.  generate()
returns the field, the decisions and the unrounded colour v, and per output pixel the smallest margin of its floor / inside / depth
decisions (so a test can tell an fp32 rounding of such a decision from an error) and the rounding bound of S19's test notes."""
import numpy as np

HOLE = np.uint64(0xFFFFFFFFFFFFFFFF)
U = 2.0 ** -24  # fp32 unit roundoff
DEPTH_REL = 0.1


def channel_max(fmt):
    return 1023 if fmt == 1 else 255


def decode(p, fmt):
    """(..., 3) float64 code values of packed pixels, R in the low bits"""
    p = np.asarray(p, np.uint32)
    bits, mask = (10, 1023) if fmt == 1 else (8, 255)
    return np.stack([(p >> np.uint32(bits * k)) & np.uint32(mask) for k in range(3)], axis=-1).astype(np.float64)


def alpha_bits(p, fmt):
    return np.asarray(p, np.uint32) & np.uint32(0xC0000000 if fmt == 1 else 0xFF000000)


def pack(v, own, fmt):
    """code = min(max(floor(v + 0.5), 0), M) per channel under own's alpha bits, in the precision of v"""
    M = channel_max(fmt)
    half = v.dtype.type(0.5)
    c = np.clip(np.floor(v + half), 0, M).astype(np.uint32)
    bits = 10 if fmt == 1 else 8
    return c[..., 0] | (c[..., 1] << np.uint32(bits)) | (c[..., 2] << np.uint32(2 * bits)) | alpha_bits(own, fmt)


def keys_of(depth):
    """step 2's key per render pixel"""
    z = np.asarray(depth, np.float32).ravel()
    bad = ~(z >= 0) | ~np.isfinite(z)
    zk = np.where(bad, np.float32(np.inf), np.where(z == 0, np.float32(0.0), z)).astype(np.float32)
    return (zk.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(z.size, dtype=np.uint64)


def scatter(depth, mv):
    """steps 1-2: the field (h, w) uint64"""
    h, w = depth.shape
    field = np.full(h * w, HOLE, np.uint64)
    key = keys_of(depth)
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.asarray(mv, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = xs + 0.5 * m[..., 0], ys + 0.5 * m[..., 1]
        ok = np.isfinite(qx) & np.isfinite(qy)
        qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
        x0, y0 = np.floor(qx), np.floor(qy)
        fx, fy = qx - x0, qy - y0
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            use = ok & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            if dx:
                use &= fx > 0
            if dy:
                use &= fy > 0
            t = (ty[use].astype(np.int64) * w + tx[use].astype(np.int64))
            np.minimum.at(field, t, key.reshape(h, w)[use])
    return field.reshape(h, w)


def _int_margin(v):
    return np.abs(v - np.round(v))


def _bilinear(img, px, py):
    """the sample of img (H, W, 3) at (px, py) - 0.5, texels clamped into the image"""
    H, W = img.shape[:2]
    x, y = px - 0.5, py - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    xa, xb = np.clip(x0, 0, W - 1).astype(np.int64), np.clip(x0 + 1, 0, W - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, H - 1).astype(np.int64), np.clip(y0 + 1, 0, H - 1).astype(np.int64)
    top = img[ya, xa] + fx * (img[ya, xb] - img[ya, xa])
    bot = img[yb, xa] + fx * (img[yb, xb] - img[yb, xa])
    return top + fy * (bot - top)


def generate(color, depth, mv, prev_color, prev_z, fmt, near=1e-5):
    """steps 1-3 for one call that is not a restart.  color, prev_color: (H, W) uint32; depth, prev_z: (h, w) float32; mv: (h, w, 3).
    Returns a dict: field (h, w); k (H, W) the entry each output pixel read; hole, valid_a, valid_b (H, W) bool; v (H, W, 3) float64 (the
    previous colour's channels in a hole); margin (H, W): the smallest distance of a decision of the pixel from flipping (0 where the
    floor that picks the previous depth's texel is within `near` of an integer and the texel on the other side changes the depth test); bound (H, W):
    the fp32 rounding bound on v."""
    h, w = depth.shape
    H, W = color.shape
    M = channel_max(fmt)
    sx, sy, rx, ry = W / w, H / h, w / W, h / H
    field = scatter(depth, mv)
    oy, ox = np.mgrid[0:H, 0:W]
    cx, cy = ox + 0.5, oy + 0.5
    margin = np.minimum(_int_margin(cx * rx), _int_margin(cy * ry))
    ix, iy = np.minimum(np.floor(cx * rx), w - 1).astype(np.int64), np.minimum(np.floor(cy * ry), h - 1).astype(np.int64)
    k = field[iy, ix]
    hole = k == HOLE
    s = np.where(hole, np.uint64(0), k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    m = np.asarray(mv, np.float64).reshape(-1, 3)[s]
    z = np.asarray(depth, np.float64).ravel()[s]
    cur, prev = decode(color, fmt), decode(prev_color, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        hx, hy = (0.5 * m[..., 0]) * sx, (0.5 * m[..., 1]) * sy
        ax, ay, bx, by = cx - hx, cy - hy, cx + hx, cy + hy

        def inside(px, py):
            ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            edge = np.minimum(np.minimum(np.abs(px), np.abs(px - W)), np.minimum(np.abs(py), np.abs(py - H)))
            return ok, np.where(np.isfinite(edge), edge, np.inf)

        valid_a, edge_a = inside(ax, ay)
        in_b, edge_b = inside(bx, by)
        sbx, sby = np.where(in_b, bx, cx), np.where(in_b, by, cy)
        zx, zy = sbx * rx, sby * ry
        e = z + m[..., 2]
        pz = np.asarray(prev_z, np.float64)

        def depth_test(jx, jy):
            zp = pz[np.clip(jy, 0, h - 1).astype(np.int64), np.clip(jx, 0, w - 1).astype(np.int64)]
            both = np.isfinite(zp) & np.isfinite(e)
            ok = (~np.isfinite(zp) & ~np.isfinite(z)) | (both & (np.abs(zp - e) <= DEPTH_REL * e))
            return ok, np.where(both, np.abs(np.abs(zp - e) - DEPTH_REL * e), np.inf)

        depth_ok, depth_margin = depth_test(np.floor(zx), np.floor(zy))
        # the floor that picks the previous depth's texel is a decision only where the texel either side of it changes the test
        index_margin = np.full(zx.shape, np.inf)
        for jx in (np.floor(zx - near), np.floor(zx + near)):
            for jy in (np.floor(zy - near), np.floor(zy + near)):
                index_margin = np.where(depth_test(jx, jy)[0] != depth_ok, 0.0, index_margin)
        margin = np.minimum(margin, np.minimum(edge_a, edge_b))
        margin = np.minimum(margin, np.where(in_b, np.minimum(index_margin, depth_margin), np.inf))
        valid_b = in_b & depth_ok
        ca = _bilinear(cur, np.where(valid_a, ax, cx), np.where(valid_a, ay, cy))
        cb = _bilinear(prev, sbx, sby)
    va, vb = valid_a[..., None], valid_b[..., None]
    v = np.where(va & vb, 0.5 * (ca + cb), np.where(va, ca, np.where(vb, cb, cur)))
    v = np.where(hole[..., None], prev, v)
    # the rounding bound of S19's test notes: a side's position carries 3u (|h| + |p| + 1) per axis, which moves its bilinear sample by
    # at most M per unit; the lerps and the average add 6u M
    hx0, hy0 = np.where(np.isfinite(hx), np.abs(hx), 0.0), np.where(np.isfinite(hy), np.abs(hy), 0.0)

    def side(px, py, used):
        d = 3 * U * (hx0 + np.abs(px) + 1) + 3 * U * (hy0 + np.abs(py) + 1)
        return np.where(used, d, 0.0)

    bound = M * (side(np.where(valid_a, ax, 0.0), np.where(valid_a, ay, 0.0), valid_a) + side(sbx, sby, valid_b)) + 6 * U * M
    bound = np.where(hole, 0.0, bound)
    margin = np.where(hole, np.minimum(_int_margin(cx * rx), _int_margin(cy * ry)), margin)
    return dict(field=field, k=k, hole=hole, valid_a=valid_a & ~hole, valid_b=valid_b & ~hole, v=v, margin=margin, bound=bound)
