"""Row N26 -- a float64 restatement of DESIGN.md spec S29 (the thin-lens camera of pt_render_lens), written from the spec's text and not
from csrc/pt_lens.h: ImportanceSampling::Uniform::GetRay, the lens ray of a pixel and a lens sample, the lens stream's seed and draws.
Plain Python / numpy; inputs are the float32 values the header receives, everything after them is float64."""
import math

import numpy as np

LENS_SEED = 0x4C454E53


def get_ray_xy(u1, u2):
    """GetRay(u) = (r cos phi, r sin phi, z), phi = 2 pi u.x, z = u.y, r = Sqrt01(1 - z^2) -> its .xy"""
    phi = 2.0 * math.pi * float(u1)
    z = float(u2)
    r = math.sqrt(min(max(1.0 - z * z, 0.0), 1.0))
    return r * math.cos(phi), r * math.sin(phi)


def vec(a):
    return np.array([float(a[0]), float(a[1]), float(a[2])], np.float64)


def unit(v):
    return v / math.sqrt(float(v @ v))


def direction_unnormalised(cam, w, h, px, py):
    """D of the pinhole ray: nx = 2 u - 1, ny = 1 - 2 v with (u, v) = (pixel + 0.5 + Jitter) / RenderSize; D = nx Right + ny Up + Forward"""
    u = (px + 0.5 + float(cam.Jitter[0])) / w
    v = (py + 0.5 + float(cam.Jitter[1])) / h
    nx, ny = 2.0 * u - 1.0, 1.0 - 2.0 * v
    return nx * vec(cam.RightDirection) + ny * vec(cam.UpDirection) + vec(cam.ForwardDirection)


def lens_ray(cam, w, h, px, py, u1, u2):
    """-> dict(o, d, tmin, tmax, D, offset, v, length): Camera.hlsli:43-54; length = |D - offset| before the normalisation"""
    D = direction_unnormalised(cam, w, h, px, py)
    vx, vy = get_ray_xy(u1, u2)
    offset = (unit(vec(cam.RightDirection)) * vx + unit(vec(cam.UpDirection)) * vy) * float(cam.ApertureRadius)
    o = vec(cam.Position) + offset
    x = D - offset
    length = math.sqrt(float(x @ x))
    d = x / length
    inv_cos = 1.0 / float(unit(vec(cam.ForwardDirection)) @ d)
    return dict(o=o, d=d, tmin=float(cam.NearDepth) * inv_cos, tmax=float(cam.FarDepth) * inv_cos, D=D, offset=offset, v=(vx, vy), length=length)


# ---- the random numbers (spec S3's hash, restated)
def hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hash_combine(seed, v):
    return seed ^ ((hash32(v) + 0x9E3779B9 + ((seed << 6) & 0xFFFFFFFF) + (seed >> 2)) & 0xFFFFFFFF)


def rng_init(px, py, frame):
    return hash_combine(hash32((frame + 0x035F9F29) & 0xFFFFFFFF), ((px << 16) | py) & 0xFFFFFFFF)


def lens_stream(px, py, frame, n_samples):
    """the 2 n_samples lens numbers of a pixel in draw order: lens = hash_combine(rng_init(px, py, FrameIndex), LENS_SEED), each draw
    s = hash32(s), value = 2 - float(1.mantissa = s >> 9), in (0, 1]"""
    s = hash_combine(rng_init(px, py, frame), LENS_SEED)
    out = []
    for _ in range(2 * n_samples):
        s = hash32(s)
        out.append(2.0 - (1.0 + (s >> 9) / 8388608.0))
    return out
