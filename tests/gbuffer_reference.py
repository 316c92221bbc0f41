"""Independent float64 numpy restatement of the G-buffer pass (row N6, DESIGN.md spec S12) for untextured spheres: what one
pixel's primary hit (or miss) writes into each of the 13 channels.  Written from the spec (GBufferGeneration.hlsl::main, the
MathLib / NRD recollections of S12), not from csrc/pt_gbuffer.h; tests/test_gbuffer.py compares the header against it."""
import numpy as np

CHANNELS = (("Position", 4), ("FlatNormal", 2), ("GeometricNormal", 2), ("LinearDepth", 1), ("NormalizedDepth", 1), ("MotionVector", 3),
            ("BaseColorMetalness", 4), ("DiffuseAlbedo", 3), ("SpecularAlbedo", 3), ("NormalRoughness", 4), ("IOR", 1), ("Transmission", 1),
            ("Radiance", 3))
BIT = {name: 1 << k for k, (name, _) in enumerate(CHANNELS)}
OFFSET = {}
_at = 0
for _name, _w in CHANNELS:
    OFFSET[_name] = (_at, _at + _w)
    _at += _w
MISS_ID = 0xFFFFFFFF


def mat(m16):
    return np.asarray(m16, dtype=np.float64).reshape(4, 4)


def project(m16, p):
    """Geometry::ProjectiveTransform: [p, 1] . M (DirectXMath rows)"""
    return np.append(np.asarray(p, dtype=np.float64), 1.0) @ mat(m16)


def screen_uv(m16, p):
    c = project(m16, p)
    return np.array([c[0] / c[3] * 0.5 + 0.5, c[1] / c[3] * -0.5 + 0.5])


def encode_unit_vector(v):
    """Packing::EncodeUnitVector(v, signed = true): octahedral"""
    v = np.asarray(v, dtype=np.float64)
    v = v / np.abs(v).sum()
    if v[2] >= 0:
        return v[:2].copy()
    sgn = np.where(v[:2] >= 0, 1.0, -1.0)
    return (1.0 - np.abs(v[1::-1])) * sgn


def decode_unit_vector(e):
    e = np.asarray(e, dtype=np.float64)
    z = 1.0 - np.abs(e).sum()
    xy = e.copy() if z >= 0 else (1.0 - np.abs(e[::-1])) * np.where(e >= 0, 1.0, -1.0)
    v = np.array([xy[0], xy[1], z])
    return v / np.linalg.norm(v)


def quat_rotate(q, v):
    u, w = np.asarray(q[:3], dtype=np.float64), float(q[3])
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=np.float64)


def camera_ray(cam, px, py, w, h):
    """Camera::GeneratePinholeRay(CalculateNDC(CalculateUV(pixel, RenderSize, Jitter))) -> (o, d unit, uv)"""
    uv = np.array([(px + 0.5 + cam.Jitter[0]) / w, (py + 0.5 + cam.Jitter[1]) / h])
    nx, ny = uv[0] * 2 - 1, 1 - uv[1] * 2
    r, u, f = (np.array(list(v), dtype=np.float64) for v in (cam.RightDirection, cam.UpDirection, cam.ForwardDirection))
    d = nx * r + ny * u + f
    return np.array(list(cam.Position), dtype=np.float64), d / np.linalg.norm(d), uv


def environment_term_rtg(f0, nov, roughness):
    """EnvironmentTerm_Rtg (MathLib)"""
    m = roughness * roughness
    x1, x2, x3, y1, y3 = nov, nov * nov, nov ** 3, m, m ** 3
    b = ((-0.755907 * x1 + 1.29678) * y1 + (-1.28514 * x1 + 0.99044)) / (
        (316.627 * x3 + 626.13 * x1 + 121.563) * y3 + (222.592 * x3 - 27.0302 * x1 + 20.3225) * y1 + (59.4188 * x3 + 2.92338 * x1 + 1.0))
    s = ((-9.04756 * x1 + 9.0632) * y1 + (3.32707 * x1 + 0.0365463)) / (
        (-20.2123 * x3 + 19.7886 * x2 + 5.56589) * y3 + (9.22949 * x3 - 16.3174 * x2 + 9.04401) * y1 + (-1.36772 * x3 + 3.59685 * x2 + 1.0))
    return np.clip(np.asarray(f0) * s + b, 0.0, 1.0)


def previous_position(spheres, i, P, N, is_static, rotations=None, prev_spheres=None, prev_rotations=None):
    """S12: Pprev = c' + r' rot(q' conj(q), N); P itself while static or without a previous pose"""
    if is_static or (prev_spheres is None and prev_rotations is None):
        return P
    ps = prev_spheres[i] if prev_spheres is not None else spheres[i]
    c, r = np.array([ps["cx"], ps["cy"], ps["cz"]], dtype=np.float64), float(ps["r"])
    n = N
    if prev_rotations is not None:
        q = rotations[i] if rotations is not None else np.array([0, 0, 0, 1.0])
        n = quat_rotate(prev_rotations[i], quat_rotate(conj(q), N))
    return c + r * n


def pixel(cam, w, h, spheres, materials, sd, px, py, t, i, rotations=None, prev_spheres=None, prev_rotations=None):
    """-> (values float64[32] in CHANNELS order, mask) of an untextured scene; unwritten channels are NaN"""
    out = np.full(32, np.nan)
    o, d, uv = camera_ray(cam, px, py, w, h)
    m = cam.Matrices
    W2P, PW2P, PW2V = list(m[5]), list(m[2]), list(m[0])

    def put(name, v):
        a, b = OFFSET[name]
        out[a:b] = v

    def mv(depth, Pprev):
        uvp = screen_uv(PW2P, Pprev)
        return np.array([(uvp[0] - uv[0]) * w, (uvp[1] - uv[1]) * h, project(PW2V, Pprev)[2] - depth])

    if i == MISS_ID:
        put("Position", [np.inf] * 4)
        put("LinearDepth", np.inf)
        put("NormalizedDepth", 0.0 if cam.IsNormalizedDepthReversed else 1.0)
        Pm = o + 1e8 * d
        put("MotionVector", mv(project(W2P, Pm)[3], Pm))
        e = sd.EnvironmentLightColor
        assert e[3] >= 0, "the restatement covers the constant environment colour"
        put("Radiance", [e[0], e[1], e[2]])
        mask = BIT["Position"] | BIT["LinearDepth"] | BIT["NormalizedDepth"] | BIT["MotionVector"] | BIT["Radiance"]
        return out, mask
    s, mt = spheres[i], materials[i]
    C, r = np.array([s["cx"], s["cy"], s["cz"]], dtype=np.float64), float(s["r"])
    N = o + float(t) * d - C
    N /= np.linalg.norm(N)
    P = C + r * N
    front = N @ d < 0
    put("Position", [*P, 2.0 ** -16 * max(np.abs(P).max(), r)])
    put("FlatNormal", encode_unit_vector(N))
    put("GeometricNormal", encode_unit_vector(N))
    clip = project(W2P, P)
    put("LinearDepth", clip[3])
    put("NormalizedDepth", clip[2] / clip[3])
    put("MotionVector", mv(clip[3], previous_position(spheres, i, P, N, sd.IsStatic, rotations, prev_spheres, prev_rotations)))
    base = np.asarray(mt["BaseColor"][:3], dtype=np.float64)
    metal, rough, ior = float(mt["Metallic"]), float(mt["Roughness"]), float(mt["IOR"])
    Ns = N if front else -N
    albedo = base * (1 - metal)
    roughness = max(2e-3, rough)
    f0d = ((1 - ior) / (1 + ior)) ** 2
    F0 = f0d + metal * (base - f0d)
    put("BaseColorMetalness", [*base, metal])
    fe = environment_term_rtg(F0, abs(Ns @ -d), roughness)
    put("DiffuseAlbedo", albedo * (1 - fe))
    put("SpecularAlbedo", fe)
    put("NormalRoughness", [*Ns, roughness])
    put("IOR", ior)
    mask = (1 << 13) - 1 - BIT["Transmission"]
    if metal < 1:
        put("Transmission", float(mt["Transmission"]))
        mask |= BIT["Transmission"]
    put("Radiance", np.asarray(mt["EmissiveColor"], dtype=np.float64) * float(mt["EmissiveStrength"]))
    return out, mask


def sphere_uv(n):
    """spec S6 of an object-space normal (mesh z mirror included)"""
    nm = np.array([n[0], n[1], -n[2]])
    lon = np.arctan2(nm[0], -nm[2])
    lat = np.arccos(np.clip(nm[1], -1, 1))
    return np.array([1.0 - (lon / (2 * np.pi) + 0.5), lat / np.pi])
