"""Independent float64 restatement of the reference's bloom (row N5), written from Shaders/Bloom.hlsl, Shaders/Merge.hlsl
and the dispatch loop of Source/Bloom.ixx:71-125.  Imports nothing from the product.

The texel coordinates are formed in fp32 as spec S11 fixes them (uv = (p + 0.5) / dims with an IEEE divide, a tap at
uv + g_size * k, the texel position u * dims - 0.5 as one fused rounding, floor and fraction), because a coordinate that
lands on the other side of a texel boundary is a different answer, not a rounding difference.  Everything after that --
the bilinear weights, the filters, the Karis average with the exact sRGB curve, the merge -- is float64."""
import numpy as np

MIPS = 5
UPSAMPLE_RADIUS = np.float32(5e-3)
F32 = np.float32


def chain_dims(w, h):
    """(width, height) of the 5 levels of the half-size blur textures"""
    return [(max(1, (w // 2) >> k), max(1, (h // 2) >> k)) for k in range(MIPS)]


def _texel_coord(t, n):
    """fp32 texel position of a tap coordinate t on an axis of n texels: integer part and fraction (clamp addressing later)"""
    t = np.where(np.abs(t) < F32(65536), t, F32(0))
    x = (t.astype(np.float64) * float(n) - 0.5).astype(F32)  # the exact product and sum, rounded once (an fp32 fma)
    xf = np.floor(x)
    return xf.astype(np.int64), (x - xf).astype(np.float64)


def sample(img, u, v):
    """SampleLevel(linear min/mag/mip, clamp) on one level: img (h, w, c) float64, u / v fp32 arrays of the same shape"""
    h, w = img.shape[:2]
    xi, fx = _texel_coord(u, w)
    yi, fy = _texel_coord(v, h)
    x0, x1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    y0, y1 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    fx, fy = fx[..., None], fy[..., None]
    top = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
    bot = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
    return top * (1 - fy) + bot * fy


def _uv(ow, oh):
    """Math::CalculateUV for every texel of an ow x oh output, fp32"""
    x = (np.arange(ow, dtype=F32) + F32(0.5)) / F32(ow)
    y = (np.arange(oh, dtype=F32) + F32(0.5)) / F32(oh)
    return np.broadcast_to(x[None, :], (oh, ow)), np.broadcast_to(y[:, None], (oh, ow))


def _taps(img, ow, oh, gx, gy):
    u, v = _uv(ow, oh)
    return lambda kx, ky: sample(img, u + gx * F32(kx), v + gy * F32(ky))


def to_srgb(x):
    """IEC 61966-2-1"""
    with np.errstate(invalid="ignore"):
        return np.where(x < 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1 / 2.4) - 0.055)


def luminance(rgb):
    return rgb[..., 0] * 0.2126 + rgb[..., 1] * 0.7152 + rgb[..., 2] * 0.0722


def karis(rgb):
    return 1.0 / (1.0 + luminance(to_srgb(rgb)) * 0.25)


def downsample(img, ow, oh, karis_average):
    """13 taps at -2..2 output texels; Karis average of five groups while the input is level 0"""
    s = _taps(img, ow, oh, F32(1) / F32(ow), F32(1) / F32(oh))
    a, b, c = s(-2, 2), s(0, 2), s(2, 2)
    d, e, f = s(-2, 0), s(0, 0), s(2, 0)
    g, h, i = s(-2, -2), s(0, -2), s(2, -2)
    j, k, l, m = s(-1, 1), s(1, 1), s(-1, -1), s(1, -1)
    if not karis_average:
        return e * 0.125 + (a + c + g + i) * 0.03125 + (b + d + f + h) * 0.0625 + (j + k + l + m) * 0.125
    groups = [(a + b + d + e) * (0.125 / 4), (b + c + e + f) * (0.125 / 4), (d + e + g + h) * (0.125 / 4), (e + f + h + i) * (0.125 / 4),
              (j + k + l + m) * (0.5 / 4)]
    total = sum(gr * karis(gr)[..., None] for gr in groups)
    return np.maximum(total, 1e-4)


def upsample(img, ow, oh):
    """3x3 tent at +-UpsamplingFilterRadius in UV units on both axes"""
    s = _taps(img, ow, oh, UPSAMPLE_RADIUS, UPSAMPLE_RADIUS)
    a, b, c = s(-1, 1), s(0, 1), s(1, 1)
    d, e, f = s(-1, 0), s(0, 0), s(1, 0)
    g, h, i = s(-1, -1), s(0, -1), s(1, -1)
    return (e * 4 + (b + d + f + h) * 2 + a + c + g + i) / 16


def bloom(hdr, strength):
    """hdr (h, w, 4) -> (out (h, w, 4) float64, [the output of each of the 9 chain steps, (h_k, w_k, 3) float64])"""
    h, w = hdr.shape[:2]
    dims = chain_dims(w, h)
    rgb = hdr[..., :3].astype(np.float64)
    level = [None] * MIPS
    steps = []
    # Bloom::Process: dispatch 1 reads the input; the loop then reads InputMipLevel = the level written last.  The constants
    # start at zero, so dispatches 1 and 2 both run with InputMipLevel 0 (Karis); upsamples overwrite their level.
    level[0] = downsample(rgb, *dims[0], True)
    steps.append(level[0])
    for k in range(1, MIPS):
        level[k] = downsample(level[k - 1], *dims[k], k == 1)
        steps.append(level[k])
    for k in range(MIPS - 2, -1, -1):
        level[k] = upsample(level[k + 1], *dims[k])
        steps.append(level[k])
    # Merge: input * (1 - Strength) + SampleLevel(blur level 0, uv, 0) * Strength; the input at its own texel
    u, v = _uv(w, h)
    out = np.empty((h, w, 4), dtype=np.float64)
    s = float(F32(strength))
    out[..., :3] = rgb * float(F32(1) - F32(strength)) + sample(level[0], u, v) * s
    out[..., 3] = hdr[..., 3]
    return out, steps
