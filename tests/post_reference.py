"""Row N3's display transform in float64, written from the published standards -- the second reference of `pt_tonemap`.

Nothing here comes from csrc/pt_post.h, from oracle/ or from the host shims: numpy float64 only, constants as the standards print them.

* SMPTE ST 2084 (PQ): m1 = 2610/16384, m2 = 2523/4096 * 128, c1 = 3424/4096, c2 = 2413/4096 * 32, c3 = 2392/4096 * 32;
  inverse EOTF N = ((c1 + c2 Y^m1) / (1 + c3 Y^m1))^m2 with Y = luminance / 10000 cd/m2; EOTF Y = (max(N^(1/m2) - c1, 0) / (c2 - c3 N^(1/m2)))^(1/m1).
* Colour primaries as CIE xy chromaticities (ITU-R BT.709, SMPTE RP 431-2 with the D65 white "P3-D65", ITU-R BT.2020; white D65 =
  (0.3127, 0.3290)); RGB -> XYZ by the usual construction (columns = primaries' XYZ scaled so that RGB (1, 1, 1) is the white point), and a
  rotation is inv(RGB->XYZ_dst) . RGB->XYZ_src.
* Operators of DirectXTK's ToneMapPostProcess (public enum order None, Saturate, Reinhard, ACESFilmic): saturate, x / (1 + x), and Narkowicz's
  ACES fit x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14), saturated.  Transfer functions Linear, SRGB, ST2084; "SRGB" is the *estimate*
  clip(c, 0, 1)^(1/2.2) that csrc/pt_post.h documents (a documented choice, not IEC 61966-2-1's piecewise curve).  Exposure is the linear factor
  of the parameter block; HDR10 scales by PaperWhiteNits / 10000 and applies the curve to |y|.

`value(hdr, params, matrix)` returns the un-rounded code value clip(v, 0, 1) * scale (scale 255 for the SDR transfers, 1023 for ST 2084) and, per
sample, the allowance delta by which an fp32 implementation built on `pow_spec` may miss it before rounding.

The allowance (forward error propagation; u = 2^-24 is fp32's unit roundoff, every quantity below is >= 0)
----------------------------------------------------------------------------------------------------------
An implementation computes code = floor(fl(v32 * S + 0.5)) from its fp32 value v32 (one fma), so
    |code - V| <= 0.5 + u (S + 0.5) + S |v32 - v|,    V = S v,
and delta = u (S + 0.5) + S dv, where dv bounds |v32 - v|.  dv comes from carrying an interval [lo, hi] around the float64 value through the
chain.  Every stage is a non-decreasing function of its input (the Narkowicz fit too: the numerator of its derivative is
1.408 x^2 + 0.7028 x + 0.0042 > 0; g(t) = (c1 + c2 t) / (1 + c3 t) because c2 > c1 c3), so the image of an interval is the interval of the
images of its ends; a stage's own fp32 roundings then widen it by (1 +- e), e = (1 + u)^k - 1 for k roundings (all terms of every sum are
non-negative, so relative errors of the terms do not grow in the sum):

  SDR   a = hdr * exposure                                   k = 1
        Saturate / None                                      k = 0
        Reinhard a / (1 + a)                                 k = 2  (the sum, the quotient)
        ACES fit                                             k = 7  (numerator: fma, product; denominator: fma, fma; quotient; and the fp32
                                                                     literals, at most u on the numerator and u on the denominator)
        Linear                                               nothing more
        SRGB  c^(1/2.2)                                      pow_spec's relative error at (c, 1/2.2), plus u / 2.2 * |ln c| because the
                                                             implementation's exponent is the fp32 nearest to 1/2.2
  HDR10 r = row . hdr (x*y, fma, fma)                        e = ((1 + u)^3 - 1) * cond,  cond = sum |m c| / |sum m c|
        y = r * (PaperWhiteNits * (1 / 10000))               k = 3  (the fp32 1/10000, two products)
        t = y^m1                                             pow_spec's relative error at (y, m1); m1 is an fp32 number
        q = (c1 + c2 t) / (1 + c3 t)                         k = 3  (fma, fma, quotient; c1, c2, c3 are fp32 numbers)
        v = q^m2                                             pow_spec's relative error at (q, m2); m2 is an fp32 number

pow_spec(x, y) = exp2_spec(fl(y * log2_spec(x))).  tests/test_leaf_edges.py records, from 2^22-point sweeps against float64,
|log2_spec(x) - log2 x| <= 8.63e-8 max(|log2 x|, 1) =: eL and a relative error of exp2_spec of 7.72e-8 =: eE.  The exponent handed to exp2_spec
therefore misses y log2 x by at most dt = |y| (eL + u (|log2 x| + eL)) (the second term is the rounding of the product), and
    |pow_spec(x, y) / x^y - 1| <= (2^dt - 1) (1 + eE) + eE.
For y = 78.84375 on [0.8359375, 1] this is 5.64e-6; for 1/2.2 on [1e-6, 1] at most 1.0e-6; for m1 on [1e-12, 1e4] at most 7.2e-7.
"""
import numpy as np

U = 2.0 ** -24
LOG2_SPEC_ERROR = 8.63e-8  # of max(|log2 x|, 1): tests/test_leaf_edges.py (measured 8.6242e-8)
EXP2_SPEC_ERROR = 7.72e-8  # relative: tests/test_leaf_edges.py (measured 7.7195e-8)

# DirectX::ToneMapPostProcess's public enumerations
OP_NONE, OP_SATURATE, OP_REINHARD, OP_ACES_FILMIC = 0, 1, 2, 3
TF_LINEAR, TF_SRGB, TF_ST2084 = 0, 1, 2
ROT_709_TO_2020, ROT_P3D65_TO_2020, ROT_709_TO_P3D65 = 0, 1, 2

# SMPTE ST 2084
PQ_M1 = 2610.0 / 16384.0
PQ_M2 = 2523.0 / 4096.0 * 128.0
PQ_C1 = 3424.0 / 4096.0
PQ_C2 = 2413.0 / 4096.0 * 32.0
PQ_C3 = 2392.0 / 4096.0 * 32.0

# CIE xy of red, green, blue
BT709 = ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))
P3_D65 = ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))
BT2020 = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))
D65 = (0.3127, 0.3290)
ROTATION_PRIMARIES = {ROT_709_TO_2020: (BT709, BT2020), ROT_P3D65_TO_2020: (P3_D65, BT2020), ROT_709_TO_P3D65: (BT709, P3_D65)}


def pq_inverse_eotf(y):
    """linear luminance / 10000 cd/m2 in [0, 1] (any y >= 0 is accepted) -> non-linear signal"""
    t = np.asarray(y, dtype=np.float64) ** PQ_M1
    return ((PQ_C1 + PQ_C2 * t) / (1.0 + PQ_C3 * t)) ** PQ_M2


def pq_eotf(n):
    """non-linear signal in [0, 1] -> linear luminance / 10000 cd/m2 (the standard's formula, written on its own)"""
    p = np.asarray(n, dtype=np.float64) ** (1.0 / PQ_M2)
    return (np.maximum(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p)) ** (1.0 / PQ_M1)


def rgb_to_xyz(primaries, white=D65):
    xyz = lambda x, y: np.array([x / y, 1.0, (1.0 - x - y) / y])
    p = np.stack([xyz(*c) for c in primaries], axis=1)  # columns: XYZ of each primary at Y = 1
    s = np.linalg.solve(p, xyz(*white))                 # scale them so that RGB (1, 1, 1) is the white point
    return p * s


def rotation_matrix(rotation):
    src, dst = ROTATION_PRIMARIES[rotation]
    return np.linalg.solve(rgb_to_xyz(dst), rgb_to_xyz(src))  # inv(RGB->XYZ_dst) . RGB->XYZ_src


def aces_fit(x):
    return x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)


def operator(x, op):
    if op == OP_SATURATE:
        return np.clip(x, 0.0, 1.0)
    if op == OP_REINHARD:
        return x / (1.0 + x)
    if op == OP_ACES_FILMIC:
        return np.clip(aces_fit(x), 0.0, 1.0)
    return x


OPERATOR_ROUNDINGS = {OP_NONE: 0, OP_SATURATE: 0, OP_REINHARD: 2, OP_ACES_FILMIC: 7}


def roundings(k):
    return (1.0 + U) ** k - 1.0


def pow_spec_relative_error(x, y):
    """bound on |pow_spec(x, y) / x^y - 1| for a normal fp32 x > 0 and the fp32 exponent y (module docstring); 0 where x == 0"""
    x = np.asarray(x, dtype=np.float64)
    l2 = np.abs(np.log2(np.where(x > 0, x, 1.0)))
    e_log = LOG2_SPEC_ERROR * np.maximum(l2, 1.0)
    dt = abs(float(y)) * (e_log + U * (l2 + e_log))
    return np.where(x > 0, np.expm1(np.log(2.0) * dt) * (1.0 + EXP2_SPEC_ERROR) + EXP2_SPEC_ERROR, 0.0)


def _pow_interval(lo, hi, y, exponent_rounding=0.0):
    """x^y over [lo, hi] (y > 0), widened by pow_spec's error and, where the implementation's exponent is a rounded one, by that"""
    def rel(x):
        ln = np.abs(np.log(np.where(x > 0, x, 1.0)))
        return pow_spec_relative_error(x, np.float32(y)) + exponent_rounding * abs(y) * ln
    r = np.maximum(rel(lo), rel(hi))
    return lo ** y * (1.0 - r), hi ** y * (1.0 + r)


def condition(hdr, matrix):
    """sum |m c| / |sum m c| per output channel of matrix . hdr (inf where the sum is 0 and a term is not)"""
    c = np.asarray(hdr, dtype=np.float64)[..., :3]
    m = np.asarray(matrix, dtype=np.float64)
    num, den = np.abs(c) @ np.abs(m).T, np.abs(c @ m.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num > 0, num / den, 1.0)


def value(hdr, params, matrix=None):
    """hdr (n, >= 3) finite and >= 0; params: Operator, TransferFunction, LinearExposure, PaperWhiteNits, ColorRotation (a PtToneMapParams or
    anything shaped like it); matrix: the 3x3 rotation of the ST 2084 path (default: the one derived from the chromaticities).
    Returns (V, delta), both (n, 3) float64: the un-rounded code value and the allowance of the module docstring."""
    c = np.asarray(hdr, dtype=np.float64)[..., :3]
    assert np.isfinite(c).all() and (c >= 0).all()
    if params.TransferFunction == TF_ST2084:
        scale = 1023.0
        m = rotation_matrix(params.ColorRotation) if matrix is None else np.asarray(matrix, dtype=np.float64)
        e_in = (1.0 + roundings(3) * condition(c, m)) * (1.0 + roundings(3)) - 1.0
        y = np.abs(c @ m.T) * (float(params.PaperWhiteNits) / 10000.0)
        v = pq_inverse_eotf(y)
        lo, hi = _pow_interval(np.maximum(y * (1.0 - e_in), 0.0), y * (1.0 + e_in), PQ_M1)
        g = lambda t: (PQ_C1 + PQ_C2 * t) / (1.0 + PQ_C3 * t)
        lo, hi = g(np.maximum(lo, 0.0)) * (1.0 - roundings(3)), g(hi) * (1.0 + roundings(3))
        lo, hi = _pow_interval(lo, hi, PQ_M2)
    else:
        scale = 255.0
        a = c * float(params.LinearExposure)
        v = operator(a, params.Operator)
        k = roundings(OPERATOR_ROUNDINGS[params.Operator])
        lo, hi = operator(a * (1.0 - roundings(1)), params.Operator) * (1.0 - k), operator(a * (1.0 + roundings(1)), params.Operator) * (1.0 + k)
        v, lo, hi = np.clip(v, 0.0, 1.0), np.clip(lo, 0.0, 1.0), np.clip(hi, 0.0, 1.0)
        if params.TransferFunction == TF_SRGB:
            v = v ** (1.0 / 2.2)
            lo, hi = _pow_interval(lo, hi, 1.0 / 2.2, exponent_rounding=U)
    v, lo, hi = np.clip(v, 0.0, 1.0), np.clip(lo, 0.0, 1.0), np.clip(hi, 0.0, 1.0)
    return v * scale, U * (scale + 0.5) + scale * np.maximum(hi - v, v - lo)


def alpha(params):
    """R8G8B8A8_UNORM and R10G10B10A2_UNORM with alpha 1"""
    return 3 if params.TransferFunction == TF_ST2084 else 255
