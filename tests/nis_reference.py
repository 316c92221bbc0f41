"""Spec S18 -- the sharpening stand-in of row N12 -- restated in float64 numpy, written from the spec's text and
not from csrc/pt_nis.h: every texel at once, the 5 x 5 patch as 25 shifted planes.  sharpen() takes the luma plane (step 1's result, so
that a test can feed it the header's own fp32 lumas) and evaluates steps 2-6 in float64.  It also returns, per texel, the smallest
relative margin of step 3's eight comparisons, so a test can tell an fp32 rounding of such a decision from an error, and the
quantities a rounding bound needs (the patch's largest luma, A + B, the limit, whether both edge classes fired)."""
import numpy as np

MAX_COLOR = 65504.0
K = 0.282842712
HDR_NONE, HDR_LINEAR = 0, 1


def config(sharpness, hdr):
    """the tables of S18 -> dict"""
    s = float(sharpness) - 0.5
    max_scale = 1.25 if s >= 0 else 1.75
    min_scale = 1.25 if s >= 0 else 1.0
    limit_scale = 1.25 if s >= 0 else 1.0
    lin = hdr == HDR_LINEAR
    c = dict(DetectRatio=2.0 * 1127.0 / 1024.0, DetectThres=(32.0 if lin else 64.0) / 1024.0, MinContrastRatio=1.5 if lin else 2.0,
             MaxContrastRatio=5.0 if lin else 10.0, SharpStartY=0.35 if lin else 0.45, SharpEndY=0.55 if lin else 0.9)
    if lin:
        c.update(StrengthMin=max(0.0, 0.4 + s * min_scale * 1.1), StrengthMax=2.2 + s * max_scale * 1.8,
                 LimitMin=max(0.06, 0.10 + s * limit_scale * 0.28), LimitMax=0.6 + s * limit_scale * 0.6, Eps=1e-4 * K * K)
    else:
        c.update(StrengthMin=max(0.0, 0.4 + s * min_scale * 1.2), StrengthMax=1.6 + s * max_scale * 1.8,
                 LimitMin=max(0.1, 0.14 + s * limit_scale * 0.32), LimitMax=0.5 + s * limit_scale * 0.6, Eps=1.0 / 255.0)
    c["RatioNorm"] = 1.0 / (c["MaxContrastRatio"] - c["MinContrastRatio"])
    c["ScaleY"] = 1.0 / (c["SharpEndY"] - c["SharpStartY"])
    c["StrengthScale"] = c["StrengthMax"] - c["StrengthMin"]
    c["LimitScale"] = c["LimitMax"] - c["LimitMin"]
    return c


def sanitize(c, dtype=np.float64):
    """step 1's rule per channel: NaN -> 0, else min(max(c, 0), 65504)"""
    c = np.asarray(c, dtype)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(c), dtype(0.0), np.minimum(np.maximum(c, dtype(0.0)), dtype(MAX_COLOR))).astype(dtype)


def luma32(color, hdr):
    """step 1 in numpy float32, in the spec's order: what the header must give bit for bit"""
    c = sanitize(np.asarray(color, np.float32)[..., :3], np.float32)
    f = np.float32
    y = (f(0.2126) * c[..., 0] + f(0.7152) * c[..., 1]) + f(0.0722) * c[..., 2]
    return (np.sqrt(y) * f(K)).astype(f) if hdr == HDR_LINEAR else y.astype(f)


def sat(x):
    return np.minimum(np.maximum(x, 0.0), 1.0)


def _margin(lhs, rhs):
    """relative distance of the two sides of a comparison; an exact tie counts as decided (inf): in float64 the three-term sums of
    fp32 lumas are exact, so a tie there is a tie of the real values, which the fp32 text reproduces wherever both sides are made
    from the same operands (a flat patch, a clamped border); random images have none"""
    d = np.abs(lhs - rhs)
    m = np.maximum(np.abs(lhs), np.abs(rhs))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0.0, np.inf, d / m)


def sharpen(luma, color, sharpness, hdr):
    """steps 2-6 of S18 in float64 on the luma plane (h, w) and the colour (h, w, 4) -> dict(usm, out, margin, M, apb, limit, both, cB)"""
    c = config(sharpness, hdr)
    y = np.asarray(luma, np.float64)
    h, w = y.shape
    pad = np.pad(y, 2, mode="edge")  # step 2: coordinates clamped into the image
    p = [[pad[i:i + h, j:j + w] for j in range(5)] for i in range(5)]
    q = [[p[a + 1][b + 1] for b in range(3)] for a in range(3)]
    # step 3
    g0 = np.abs((q[0][0] + q[0][1] + q[0][2]) - (q[2][0] + q[2][1] + q[2][2]))
    g45 = np.abs((q[1][0] + q[0][0] + q[0][1]) - (q[2][1] + q[2][2] + q[1][2]))
    g90 = np.abs((q[0][0] + q[1][0] + q[2][0]) - (q[0][2] + q[1][2] + q[2][2]))
    g135 = np.abs((q[1][0] + q[2][0] + q[2][1]) - (q[0][1] + q[0][2] + q[1][2]))
    A, a, B, b = np.maximum(g0, g90), np.minimum(g0, g90), np.maximum(g45, g135), np.minimum(g45, g135)
    nz = (A + B) != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(nz, np.minimum(A / (A + B), 1.0), 0.0)
    cA = nz & (A > a * c["DetectRatio"]) & (A > c["DetectThres"]) & (A > b)
    cB = nz & (B > b * c["DetectRatio"]) & (B > c["DetectThres"]) & (B > a)
    both = cA & cB
    fA, fB = np.where(both, e, 1.0), np.where(both, 1.0 - e, 1.0)
    w0 = np.where(cA & (A == g0), fA, 0.0)
    w90 = np.where(cA & (A != g0), fA, 0.0)
    w45 = np.where(cB & (B == g45), fB, 0.0)
    w135 = np.where(cB & (B != g45), fB, 0.0)
    thres = np.full_like(A, c["DetectThres"])
    # The eight comparisons.  The order of g0 and g90 is only used where cA holds (it picks which of w0, w90 takes fA), and cA needs
    # A > a DetectRatio: where that test fails by more than the margin, the two weights are 0 in fp32 as well, whichever of g0, g90 is
    # the larger; where it fails by less, the texel is marked by that test already.  So g0 vs g90 counts where the ratio test
    # passes (a luma of 65504 * 0.7 in a corner of the 3 x 3 makes g0 and g90 agree to 1e-5 and cA false by a factor 2.2).
    # Likewise g45 vs g135 and B > b DetectRatio.
    ratio_a, ratio_b = A > a * c["DetectRatio"], B > b * c["DetectRatio"]
    margin = np.minimum.reduce([_margin(A, a * c["DetectRatio"]), _margin(A, thres), _margin(A, b), _margin(B, b * c["DetectRatio"]),
                                _margin(B, thres), _margin(B, a), np.where(ratio_a, _margin(g0, g90), np.inf),
                                np.where(ratio_b, _margin(g45, g135), np.inf)])
    # step 4
    yc = p[2][2]
    k = 1.0 - sat((yc - c["SharpStartY"]) * c["ScaleY"])
    strength = k * c["StrengthScale"] + c["StrengthMin"]
    limit = (k * c["LimitScale"] + c["LimitMin"]) * yc

    # step 5
    def line(t):
        u = (-0.6001 * t[1] + 1.2002 * t[2] - 0.6001 * t[3]) * strength
        u = np.minimum(limit, np.maximum(-limit, u))
        ac = np.maximum.reduce(t[0:3]) - np.minimum.reduce(t[0:3])
        bc = np.maximum.reduce(t[2:5]) - np.minimum.reduce(t[2:5])
        r = np.maximum(ac, bc) / (np.minimum(ac, bc) + c["Eps"])
        return u * (1.0 - sat((r - c["MinContrastRatio"]) * c["RatioNorm"]))

    u0 = line([p[i][2] for i in range(5)])
    u90 = line([p[2][i] for i in range(5)])
    u45 = line([p[4 - i][i] for i in range(5)])
    u135 = line([p[i][i] for i in range(5)])
    usm = w0 * u0 + w90 * u90 + w45 * u45 + w135 * u135
    # step 6
    color = np.asarray(color)
    rgb = sanitize(color[..., :3])
    if hdr == HDR_LINEAR:
        yn = np.maximum(yc + usm, 0.0)
        corr = (yn * yn + c["Eps"]) / (yc * yc + c["Eps"])
        out = np.minimum(rgb * corr[..., None], MAX_COLOR)
    else:
        out = np.maximum(rgb + usm[..., None], 0.0)
    M = np.maximum.reduce([p[i][j] for i in range(5) for j in range(5)])
    return dict(usm=usm, out=out, margin=margin, M=M, apb=A + B, limit=limit, both=both, cB=cB, yc=yc, config=c)
