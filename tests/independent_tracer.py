"""An INDEPENDENT restatement of the bounce loop, used only to cross-check oracle/pt_oracle.c (the oracle
and the device headers are siblings, so a shared misreading of the shaders would pass every GPU-vs-oracle test).

Written from the reference's shader text alone -- Shaders/Raytracing.hlsl:103-415 (DEFAULT permutation), Shaders/BxDF.hlsli:21-315,
SurfaceVectors.hlsli, HitInfo.hlsli:60-64,91-99, Camera.hlsli:27-41, Math.hlsli:7-33, ShadingHelpers.hlsli:11-235,
RaytracingHelpers.hlsli:19-43, Source/Scene.ixx:197-199 -- plus SURVEY.md Appendix A for the un-vendored MathLib bodies, DESIGN.md S3
for the build-defined ray-sphere hit, and where the reference has no text for analytic spheres (texture coordinates, sampler, cube
faces, alpha-tested crossings, the direct-illumination stand-in) the DESIGN.md spec items S6-S10 and section 10 N4.  It shares NO code with the
oracle or the kernels and deliberately differs from them in everything that is not the estimator itself:

  * double precision throughout, libm transcendentals (no fma placement, no polynomial sincos / pow / sky fits),
  * the literal formulas of the shader text (f and pdf evaluated separately and divided; textbook GGX D; HLSL lerp / pow),
  * brute-force closest hit, a flat procedural style (dicts and tuples) instead of the oracle's structs.

What has to agree with the oracle EXACTLY: the integer RNG stream (state after every bounce), every hit id, every lobe choice and
every termination reason, and with direct illumination the emitter, the shadow ray's hit and the cull; throughput, hit distance and radiance agree to rounding (1e-3 relative is asserted; typical 1e-6).
tests/test_independent_tracer.py compares per event against oracle_trace_pixel and keeps the traces as fixtures."""
import math

MISS = 0xFFFFFFFF
PI = math.pi


# ---------------------------------------------------------------- Rng::Hash (call sites Raytracing.hlsl:108,330,351)
def _hash(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def rng_seed(px, py, frame):
    seed = _hash((frame + 0x035F9F29) & 0xFFFFFFFF)
    v = ((px << 16) | py) & 0xFFFFFFFF
    return (seed ^ ((_hash(v) + 0x9E3779B9 + ((seed << 6) & 0xFFFFFFFF) + (seed >> 2)) & 0xFFFFFFFF)) & 0xFFFFFFFF


class Stream:
    def __init__(self, state):
        self.state = state

    def uint(self):
        self.state = _hash(self.state)
        return self.state

    def unit(self):
        """GetFloat = 2 - asfloat((u >> 9) | 0x3F800000): (0, 1], 23 bits"""
        mantissa = self.uint() >> 9
        return 2.0 - (1.0 + mantissa / 8388608.0)


# ---------------------------------------------------------------- small vector helpers (tuples of 3 floats)
def add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def mul(a, b): return (a[0] * b[0], a[1] * b[1], a[2] * b[2])
def scale(a, s): return (a[0] * s, a[1] * s, a[2] * s)
def neg(a): return (-a[0], -a[1], -a[2])
def dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def unit(a): return scale(a, 1.0 / math.sqrt(dot(a, a)))
def lum(c): return 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]
def saturate(x): return 0.0 if not (x > 0.0) else (1.0 if x > 1.0 else x)
def finite3(a): return all(math.isfinite(x) for x in a)


def sign_ml(x):  # Math::Sign: Sign(0) = +1
    return 1.0 if x >= 0.0 else -1.0


# ---------------------------------------------------------------- MathLib
def get_basis(n):
    sz = sign_ml(n[2])
    a = 1.0 / (sz + n[2])
    ya = n[1] * a
    b = n[0] * ya
    c = n[0] * sz
    t = (c * n[0] * a - 1.0, sz * b, c)
    bt = (b, n[1] * ya - sz, n[1])
    return t, bt, n


def to_local(basis, v): return (dot(basis[0], v), dot(basis[1], v), dot(basis[2], v))           # RotateVector
def to_world(basis, v): return add(add(scale(basis[0], v[0]), scale(basis[1], v[1])), scale(basis[2], v[2]))  # RotateVectorInverse


def cosine_ray(u):
    phi = 2.0 * PI * u[0]
    ct = math.sqrt(saturate(u[1]))
    st = math.sqrt(saturate(1.0 - ct * ct))
    return (st * math.cos(phi), st * math.sin(phi), ct)


def vndf_ray(u, rough, vl):
    m = rough * rough
    vh = unit((m * vl[0], m * vl[1], vl[2]))
    phi = 2.0 * PI * u[0]
    z = (1.0 - u[1]) * (1.0 + vh[2]) - vh[2]
    s = math.sqrt(saturate(1.0 - z * z))
    nh = add((s * math.cos(phi), s * math.sin(phi), z), vh)
    return unit((m * nh[0], m * nh[1], max(nh[2], 1e-7)))


def ggx_d(rough, noh):
    m = rough * rough
    m2 = m * m
    t = (noh * m2 - noh) * noh + 1.0
    return m2 / (PI * t * t)


def vndf_pdf(vl, noh, rough):
    m = rough * rough
    nov = abs(vl[2])
    g1 = 2.0 * nov / (nov + math.sqrt(m * m + (1.0 - m * m) * nov * nov))
    return ggx_d(rough, noh) * g1 / (4.0 * nov)


def geometry_mod(rough, nol, nov):
    m = rough * rough
    m2 = m * m
    a = nov * math.sqrt(saturate((nol - m2 * nol) * nol + m2))
    b = nol * math.sqrt(saturate((nov - m2 * nov) * nov + m2))
    return 0.5 / (a + b)


def schlick(f0, voh):
    k = (1.0 - voh) ** 5
    return tuple(f + (1.0 - f) * k for f in f0)


def fresnel_dielectric(eta, von):
    sa2 = eta * eta * (1.0 - von * von)
    ca = math.sqrt(saturate(1.0 - sa2))
    rs = (eta * von - ca) / (eta * von + ca)
    rp = (eta * ca - von) / (eta * ca + von)
    return 0.5 * (rs * rs + rp * rp)


def burley(rough, nol, nov, voh):
    f = 2.0 * voh * voh * rough - 0.5
    return (1.0 + f * (1.0 - nol) ** 5) * (1.0 + f * (1.0 - nov) ** 5) / PI


def env_term_rtg(f0, nov, rough):
    m = rough * rough
    x = (1.0, nov, nov * nov, nov ** 3)
    y = (1.0, m, m * m, m ** 3)
    m1 = ((0.99044, -1.28514), (1.29678, -0.755907))
    m2 = ((1.0, 2.92338, 59.4188), (20.3225, -27.0302, 222.592), (121.563, 626.13, 316.627))
    m3 = ((0.0365463, 3.32707), (9.0632, -9.04756))
    m4 = ((1.0, 3.59685, -1.36772), (9.04401, -16.3174, 9.22949), (5.56589, 19.7886, -20.2123))
    xy, xyw, xzw, yxy, yxyw = (x[0], x[1]), (x[0], x[1], x[3]), (x[0], x[2], x[3]), (y[0], y[1]), (y[0], y[1], y[3])

    def bil(mat, a, b):  # dot(mat * a, b)
        return sum(sum(mat[r][c] * a[c] for c in range(len(a))) * b[r] for r in range(len(b)))

    bias = bil(m1, xy, yxy) / bil(m2, xyw, yxyw)
    sc = bil(m3, xy, yxy) / bil(m4, xzw, yxyw)
    return tuple(saturate(f * sc + bias) for f in f0)


def from_srgb(c):
    c = saturate(c)
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def reflect(i, n): return sub(i, scale(n, 2.0 * dot(n, i)))


def refract(i, n, eta):
    ni = dot(n, i)
    k = 1.0 - eta * eta * (1.0 - ni * ni)
    if k < 0.0:
        return (0.0, 0.0, 0.0)
    return sub(scale(i, eta), scale(n, eta * ni + math.sqrt(k)))


# ---------------------------------------------------------------- texture maps (row N1: DESIGN.md section 10, specs S6, S7, S9)
# tex = {"images": [(texels, kind)], "maps": [[descriptor] * 7 per sphere], "rotations": [(x, y, z, w) per sphere]}: the raw data
# of a TextureSet.  kind "unorm" / "srgb": uint8 texels, "float": float32 texels.  Descriptor 0xFFFFFFFF = no map.
MAP_BASE_COLOR, MAP_EMISSIVE_COLOR, MAP_METALLIC, MAP_ROUGHNESS, MAP_METALLIC_ROUGHNESS, MAP_TRANSMISSION, MAP_NORMAL = range(7)  # Material.hlsli:24-34


def map_of(tex, sphere_id, kind):
    if tex is None or sphere_id is None:
        return None
    desc = int(tex["maps"][sphere_id][kind])
    return None if desc == MISS else desc


def texel(img, x, y):
    """one texel as linear RGBA, decoded where the upload decodes it (S7): x/255, colour channels of an sRGB image through the
    sRGB curve (alpha stays x/255), float texels as they are"""
    texels, kind = img
    v = [float(c) for c in texels[y][x]]
    if kind == "float":
        return v
    v = [c / 255.0 for c in v]
    if kind == "srgb":
        v = [from_srgb(v[0]), from_srgb(v[1]), from_srgb(v[2]), v[3]]
    return v


def bilinear(img, uv, wrap):
    """SampleLevel(sampler, uv, 0) (S7): level-0 bilinear filter between the four texel centres around uv, wrap addressing on a
    2D map, clamp addressing inside a cube face (S9); HLSL lerp"""
    texels = img[0]
    h, w = len(texels), len(texels[0])
    u, v = (c if math.isfinite(c) else 0.0 for c in uv)
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = math.floor(x), math.floor(y)
    fx, fy = x - x0, y - y0
    if wrap:
        ix, iy = (x0 % w, (x0 + 1) % w), (y0 % h, (y0 + 1) % h)
    else:
        ix = (min(max(x0, 0), w - 1), min(max(x0 + 1, 0), w - 1))
        iy = (min(max(y0, 0), h - 1), min(max(y0 + 1, 0), h - 1))
    c00, c10, c01, c11 = texel(img, ix[0], iy[0]), texel(img, ix[1], iy[0]), texel(img, ix[0], iy[1]), texel(img, ix[1], iy[1])
    lerp = lambda a, b, t: a + (b - a) * t
    return [lerp(lerp(c00[k], c10[k], fx), lerp(c01[k], c11[k], fx), fy) for k in range(4)]


def sample_map(tex, desc, uv):
    return bilinear(tex["images"][desc], uv, True)


def object_to_world(tex, sphere_id):
    """the rotation part of ObjectToWorld (Scene.ixx:197-199: diag(1, 1, -1) * pose): R(q) * Z, where q is the object's rotation
    as the host hands it over -- the pose conjugated with the mirror Z = diag(1, 1, -1), so Z * pose = R(q) * Z -- and R(q) the
    rotation matrix of the quaternion (x, y, z, w)"""
    x, y, z, w = (float(c) for c in tex["rotations"][sphere_id])
    R = ((1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)),
         (2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)),
         (2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)))
    return tuple((row[0], row[1], -row[2]) for row in R)


def mat_vec(M, v): return (dot(M[0], v), dot(M[1], v), dot(M[2], v))
def mat_t_vec(M, v): return (M[0][0] * v[0] + M[1][0] * v[1] + M[2][0] * v[2], M[0][1] * v[0] + M[1][1] * v[1] + M[2][1] * v[2],
                             M[0][2] * v[0] + M[1][2] * v[1] + M[2][2] * v[2])


def mesh_normal(tex, sphere_id, n_world):
    """the GeoSphere vertex normal at the point whose outward world normal is n_world: ObjectToWorld is orthogonal, so its
    inverse is its transpose"""
    return mat_t_vec(object_to_world(tex, sphere_id), n_world)


def uv_of_mesh_normal(nm):
    """S6: u = 1 - (atan2(n.x, -n.z) / 2pi + 1/2), v = acos(n.y) / pi"""
    return (1.0 - (math.atan2(nm[0], -nm[2]) / (2.0 * PI) + 0.5), math.acos(max(-1.0, min(1.0, nm[1]))) / PI)


def sphere_uv(tex, sphere_id, n_world):
    return uv_of_mesh_normal(mesh_normal(tex, sphere_id, n_world))


def sphere_tangent_world(tex, sphere_id, n_world):
    """S6: the tangent is the direction in which u increases.  d atan2(x, -z) = (x dz - z dx) / (x^2 + z^2), so grad u is along
    (z, 0, -x) of the mesh normal; zero at the poles.  Carried to world space by ObjectToWorld."""
    nm = mesh_normal(tex, sphere_id, n_world)
    l = math.hypot(nm[2], nm[0])
    if not l > 0.0:
        return (0.0, 0.0, 0.0)
    return mat_vec(object_to_world(tex, sphere_id), (nm[2] / l, 0.0, -nm[0] / l))


def cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def perturb_normal(N, T, s):
    """PerturbNormal (ShadingHelpers.hlsli:89-103): Geometry::UnpackLocalNormal of the map's RG -- the encoding the normal maps
    are made with, n.xy = s * 255/127 - 1, z = sqrt(saturate(1 - x^2 - y^2)) -- then Math::CalculateTBN (Math.hlsli:17-21:
    T = normalize(T - N dot(N, T)), rows T, cross(N, T), N) and normalize(RotateVectorInverse(TBN, n))"""
    x, y = s[0] * 255.0 / 127.0 - 1.0, s[1] * 255.0 / 127.0 - 1.0
    z = math.sqrt(saturate(1.0 - x * x - y * y))
    Tn = unit(sub(T, scale(N, dot(N, T))))
    B = cross(N, Tn)
    return unit(add(add(scale(Tn, x), scale(B, y)), scale(N, z)))


def evaluate_material(mat, hit, tex):
    """EvaluateMaterial (ShadingHelpers.hlsli:161-235) at a hit: the material with every map applied under the shader's guards,
    and the shading normal (the hit's front-facing normal, perturbed by the normal map).  The geometric normal is untouched."""
    e = dict(mat)
    e["Ns"] = hit["Ns"]
    sid = hit["id"]
    if tex is None or all(map_of(tex, sid, k) is None for k in range(7)):
        return e
    uv = sphere_uv(tex, sid, hit["N"])
    T = sphere_tangent_world(tex, sid, hit["N"])
    if not hit["front"]:                                          # HitInfo::GetFrontTangent, HitInfo.hlsli:91-94
        T = neg(T)
    base = list(e["BaseColor"])
    desc = map_of(tex, sid, MAP_BASE_COLOR)
    if any(c > 0.0 for c in base) and desc is not None:           # EvaluateBaseColor :61-72 (any over the float4)
        m = sample_map(tex, desc, uv)
        base = [base[k] * m[k] for k in range(4)]
    e["BaseColor"] = base
    desc = map_of(tex, sid, MAP_EMISSIVE_COLOR)
    if any(c * e["EmissiveStrength"] > 0.0 for c in e["EmissiveColor"]) and desc is not None:   # :178-184
        m = sample_map(tex, desc, uv)
        e["EmissiveColor"] = [e["EmissiveColor"][k] * m[k] for k in range(3)]
    desc = map_of(tex, sid, MAP_METALLIC_ROUGHNESS)
    if desc is not None:                                          # :186-196: metallic from B, roughness from G
        if e["Metallic"] > 0.0 or e["Roughness"] > 0.0:
            m = sample_map(tex, desc, uv)
            e["Metallic"], e["Roughness"] = e["Metallic"] * m[2], e["Roughness"] * m[1]
    else:                                                         # :197-213: the separate maps, red channel
        desc = map_of(tex, sid, MAP_METALLIC)
        if e["Metallic"] > 0.0 and desc is not None:
            e["Metallic"] = e["Metallic"] * sample_map(tex, desc, uv)[0]
        desc = map_of(tex, sid, MAP_ROUGHNESS)
        if e["Roughness"] > 0.0 and desc is not None:
            e["Roughness"] = e["Roughness"] * sample_map(tex, desc, uv)[0]
    desc = map_of(tex, sid, MAP_TRANSMISSION)
    if e["Metallic"] < 1.0 and e["Transmission"] > 0.0 and desc is not None:   # :215-222 with EvaluateTransmission :75-87
        e["Transmission"] = e["Transmission"] * sample_map(tex, desc, uv)[0]
    desc = map_of(tex, sid, MAP_NORMAL)
    if any(c != 0.0 for c in T) and desc is not None:            # :224-232
        e["Ns"] = perturb_normal(hit["Ns"], T, sample_map(tex, desc, uv))
    return e


# ---------------------------------------------------------------- geometry: analytic spheres, brute force
def hit_sphere(o, d, tmin, tmax, c, r):
    f = sub(o, c)
    bp = -dot(f, d)
    l = add(f, scale(d, bp))
    disc = r * r - dot(l, l)
    if not (disc >= 0.0):
        return None
    sq = math.sqrt(disc)
    q = bp + (sq if bp >= 0.0 else -sq)
    if q == 0.0:
        return None
    ta, tb = (dot(f, f) - r * r) / q, q
    t0, t1 = (ta, tb) if ta < tb else (tb, ta)
    t = t0 if t0 > tmin else t1
    return t if (t > tmin and t < tmax) else None


def surface_crossings(o, d, c, r):
    """both parameters at which the line meets the sphere, ascending (the textbook quadratic, unit d), or () -- the candidates
    of a non-opaque object, which the reference meets as the front and the back triangles of its mesh"""
    f = sub(o, c)
    b = dot(f, d)
    disc = b * b - (dot(f, f) - r * r)
    if not (disc >= 0.0):
        return ()
    sq = math.sqrt(disc)
    return (-b - sq, -b + sq)


def is_opaque(mat, tex=None, sphere_id=None, n=None, margins=None):
    """IsOpaque (ShadingHelpers.hlsli:105-115): EvaluateBaseColor (:61-72) multiplies the float4 BaseColor by the base-colour map
    when any of its four components is positive and the object has that map -- here at the texture coordinates of the crossing
    whose outward normal is n (DESIGN S10) -- and the crossing is accepted iff the resulting alpha >= AlphaCutoff"""
    alpha = mat["BaseColor"][3]
    desc = map_of(tex, sphere_id, MAP_BASE_COLOR)
    if desc is not None and any(c > 0.0 for c in mat["BaseColor"]):
        alpha *= sample_map(tex, desc, sphere_uv(tex, sphere_id, n))[3]
    if margins is not None:
        margins.append(abs(alpha - mat["AlphaCutoff"]) / max(abs(mat["AlphaCutoff"]), 1e-30))
    return alpha >= mat["AlphaCutoff"]


def cast_ray(spheres, o, d, tmin, tmax, materials=None, tex=None, margins=None):
    """closest hit, ties to the lowest id (ascending scan, strict <); returns the HitInfo the loop needs or None.
    An object whose AlphaMode is not Opaque is non-opaque geometry (Scene.ixx:242-243): each of its candidates is committed only
    if IsOpaque accepts it (RaytracingHelpers.hlsli:19-43).  margins: the relative margin of every alpha test is appended, and the
    geometric one of the query: the smallest angle by which the ray would have to turn to graze a sphere's silhouette (spheres
    ahead that do not contain the origin), and the relative gap between the two nearest hits."""
    best, best_id = tmax, MISS
    graze, ts = math.inf, []
    for i, (cx, cy, cz, r) in enumerate(spheres):
        if margins is not None:
            f = sub((cx, cy, cz), o)
            dist, along = math.sqrt(dot(f, f)), dot(f, d)
            if dist > r and along > 0.0:
                graze = min(graze, abs(math.sqrt(max(dist * dist - along * along, 0.0)) - r) / dist)
        if materials is not None and materials[i].get("AlphaMode", 0) != 0:
            t = None
            for candidate in surface_crossings(o, d, (cx, cy, cz), r):   # the nearer candidate first
                if candidate > tmin and candidate < best:
                    n = unit(sub(add(o, scale(d, candidate)), (cx, cy, cz)))
                    if is_opaque(materials[i], tex, i, n, margins):
                        t = candidate
                        break
        else:
            t = hit_sphere(o, d, tmin, math.inf, (cx, cy, cz), r)
        if t is not None and margins is not None:
            ts.append(t)
        if t is not None and t < best:
            best, best_id = t, i
    if margins is not None:
        ts.sort()
        margins.append(min(graze, (ts[1] - ts[0]) / ts[1] if len(ts) > 1 else math.inf))
    if best_id == MISS:
        return None
    cx, cy, cz, r = spheres[best_id]
    c = (cx, cy, cz)
    n = unit(sub(add(o, scale(d, best)), c))
    p = add(c, scale(n, r))
    front = dot(n, d) < 0.0                                      # HitInfo.hlsli:47
    return {"id": best_id, "t": best, "P": p, "N": n, "front": front, "Ns": n if front else neg(n),  # :60-64
            "offset": 2.0 ** -16 * max(abs(p[0]), abs(p[1]), abs(p[2]), r)}


def safe_origin(hit, L):                                         # HitInfo.hlsli:96-99
    return add(hit["P"], scale(hit["N"], hit["offset"] * sign_ml(dot(L, hit["N"]))))


# ---------------------------------------------------------------- BSDF (Shaders/BxDF.hlsli)
def bsdf_of(mat, front, primary):
    base = tuple(mat["BaseColor"][:3])
    metallic, rough, ior = mat["Metallic"], mat["Roughness"], mat["IOR"]
    trans = mat["Transmission"]
    if primary and not (metallic < 1.0):                          # Raytracing.hlsl:148
        trans = 0.0
    iori, ioro = (1.0, ior) if front else (ior, 1.0)              # BxDF.hlsli:57-63
    f0d = ((iori - ioro) / (iori + ioro)) ** 2
    return {"base": base, "metallic": metallic, "albedo": scale(base, 1.0 - metallic), "rough": max(2e-3, rough), "iori": iori, "ioro": ioro,
            "f0": tuple(f0d + (b - f0d) * metallic for b in base), "trans": trans}


def lobe_weights(b, sv, V):                                       # :184-196, :21-34
    nov = abs(dot(sv["Ns"], V))
    wt = b["trans"] * (1.0 - b["metallic"])
    wr = 1.0 - wt
    fe = env_term_rtg(b["f0"], nov, b["rough"])
    diffuse = lum(mul(b["albedo"], tuple(1.0 - f for f in fe)))
    specular = lum(fe)
    total = diffuse + specular
    pd = diffuse / total if total > 0.0 else 1.0
    if 0.0 < pd < 1.0:
        pd = min(max(pd, 0.05), 0.95)
    return (pd * wr, (1.0 - pd) * wr, wt)


def find_lobe(w, r):                                              # :198-212
    lobe, weight = 3, 0.0
    while True:
        lobe -= 1
        if not lobe > 0:
            break
        weight += w[lobe]
        if r < weight:
            break
    return lobe


def sample(b, sv, V, w, rnd, margins=None):                       # :214-226
    lobe = find_lobe(w, rnd[0])
    basis = sv["basis"]
    if lobe == 0:                                                 # :81-86
        L = to_world(basis, cosine_ray((rnd[1], rnd[2])))
        return dot(sv["FrontNg"], L) > 0.0, L, lobe
    H = to_world(basis, vndf_ray((rnd[1], rnd[2]), b["rough"], to_local(basis, V)))
    if lobe == 1:                                                 # :110-118
        L = reflect(neg(V), H)
        return dot(sv["FrontNg"], L) > 0.0, L, lobe
    voh, eta = abs(dot(V, H)), b["iori"] / b["ioro"]              # :148-170
    if margins is not None:
        margins.append(min(abs(eta * eta * (1.0 - voh * voh) - 1.0), abs(rnd[3] - fresnel_dielectric(eta, voh))))
    if eta * eta * (1.0 - voh * voh) > 1.0 or rnd[3] < fresnel_dielectric(eta, voh):
        L = reflect(neg(V), H)
    else:
        L = refract(neg(V), H, eta)
        if not finite3(L):
            L = neg(V)
    return True, L, lobe


def half_vector(b, sv, L, V, transmissive):                       # :228-245
    N = sv["FrontNg"]
    if transmissive and dot(N, L) < 0.0:
        H = unit(add(scale(L, b["ioro"]), scale(V, b["iori"])))
        return neg(H) if dot(N, H) < 0.0 else H
    return unit(add(L, V))


def pdf_of(b, sv, L, V, w, lobe):                                 # :287-299
    H = half_vector(b, sv, L, V, w[2] > 0.0)
    N = sv["Ns"]
    if lobe == 0:                                                 # :88-97
        return (abs(dot(N, L)) / PI if dot(sv["FrontNg"], L) > 0.0 else 0.0) * w[0]
    if lobe == 1:                                                 # :120-131
        if dot(sv["FrontNg"], L) > 0.0:
            return vndf_pdf(to_local(sv["basis"], V), abs(dot(N, H)), b["rough"]) * w[1]
        return 0.0
    return abs(dot(N, L)) * w[2]                                  # :172-177


def eval_of(b, sv, L, V, w, lobe):                                # :301-315
    H = half_vector(b, sv, L, V, w[2] > 0.0)
    N = sv["Ns"]
    if lobe == 2:                                                 # :179-182
        return scale(b["base"], abs(dot(N, L)) * w[2])
    wr = 1.0 - w[2]
    if not dot(sv["FrontNg"], L) > 0.0:
        return (0.0, 0.0, 0.0)
    nol, nov, voh = abs(dot(N, L)), abs(dot(N, V)), abs(dot(V, H))
    if lobe == 0:                                                 # :99-108
        return scale(b["albedo"], nol * burley(b["rough"], nol, nov, voh) * wr)
    noh = abs(dot(N, H))                                          # :133-146
    k = nol * ggx_d(b["rough"], noh) * geometry_mod(b["rough"], nol, nov)
    return scale(schlick(b["f0"], voh), k * wr)


# ---------------------------------------------------------------- environment (ShadingHelpers.hlsli:11-30)
def cube_face(d):
    """TextureCube addressing (S9): the face of the axis of largest magnitude (ties: z over y over x), D3D face order
    +X -X +Y -Y +Z -Z, and the face coordinates of the D3D cube-map table: (sc, tc, ma) =
    +X (-z, -y, x), -X (z, -y, x), +Y (x, z, y), -Y (x, -z, y), +Z (x, -y, z), -Z (-x, -y, z); u = (sc/|ma| + 1)/2, v = (tc/|ma| + 1)/2"""
    x, y, z = d
    ax, ay, az = abs(x), abs(y), abs(z)
    if az >= ax and az >= ay:
        face, sc, tc, ma = (4, x, -y, az) if z >= 0.0 else (5, -x, -y, az)
    elif ay >= ax:
        face, sc, tc, ma = (2, x, z, ay) if y >= 0.0 else (3, x, -z, ay)
    else:
        face, sc, tc, ma = (0, -z, -y, ax) if x >= 0.0 else (1, z, -y, ax)
    return face, ((sc / ma + 1.0) * 0.5, (tc / ma + 1.0) * 0.5)


def environment(env_color, d, env_map=None):
    """GetEnvironmentLightColor.  env_map = {"M": 3x3 rows of EnvironmentLightTransform, "cube": bool, "images": the lat-long image
    or the six faces}: d' = normalize(RotateVector((float3x3)M, d)) (:16), then the cube (:17-21) or the lat-long lookup (:22-23,
    Math::ToLatLongCoordinate, Math.hlsli:29-33: ((1 + atan2(x, z) / pi) / 2, acos(y) / pi))"""
    if env_map is not None:
        r = unit(mat_vec(env_map["M"], d))
        if env_map["cube"]:
            face, uv = cube_face(r)
            return tuple(bilinear(env_map["images"][face], uv, False)[:3])
        uv = ((1.0 + math.atan2(r[0], r[2]) / PI) / 2.0, math.acos(max(-1.0, min(1.0, r[1]))) / PI)
        return tuple(bilinear(env_map["images"][0], uv, True)[:3])
    if env_color[3] >= 0.0:
        return tuple(env_color[:3])
    t = (d[1] + 1.0) * 0.5
    return tuple(from_srgb(1.0 + (c - 1.0) * t) for c in (0.5, 0.7, 1.0))


# ---------------------------------------------------------------- direct illumination (row N4: DESIGN.md section 10 N4)
DI_SALT = 0x44495F31
DI_NEGLIGIBLE = 1e-7
DI_SHADOW, DI_CULLED, DI_NO_CANDIDATE, DI_NONE = 0, 1, 2, 3   # what became of the pixel's one DI sample


def emitters(materials):
    """the emissive objects in id order (LightPreparation.ixx:52-70): any component of EmissiveStrength * EmissiveColor > 0"""
    return [i for i, m in enumerate(materials) if any(m["EmissiveStrength"] * c > 0.0 for c in m["EmissiveColor"])]


def sphere_cone(P, C, r, u1, u2):
    """a direction uniform in the cone the sphere (C, r) subtends from P and 1 / its pdf, or None when P is inside.  The cone's
    solid angle is 2 pi (1 - cos theta_max), 1 - cos formed as sin^2 / (1 + cos); cos theta = 1 - u1 (1 - cos theta_max),
    phi = 2 pi u2, about the axis in the frame of Geometry::GetBasis (the samplers' frame)"""
    w = sub(C, P)
    d2 = dot(w, w)
    if not d2 > r * r:
        return None
    sin2 = r * r / d2
    omc = sin2 / (1.0 + math.sqrt(saturate(1.0 - sin2)))
    k = u1 * omc
    cos_t = 1.0 - k
    sin_t = math.sqrt(saturate(k * (1.0 + cos_t)))
    phi = 2.0 * PI * u2
    L = to_world(get_basis(unit(w)), (sin_t * math.cos(phi), sin_t * math.sin(phi), cos_t))
    return L, 2.0 * PI * omc


def direct_illumination(spheres, materials, tex, px, py, frame, primary, b, sv, V, lights, margins):
    """one emitter uniformly, one direction in its cone, the shadow ray must reach it first; DI = Le (f_d + f_s) cos n / pdf with
    Le = the emission EvaluateMaterial gives at the point the shadow ray reaches; no shadow ray when the bound with the emitter's
    untextured radiance is <= kDiNegligible.  Returns (DI, record) -- record = (emitter, L, inv_pdf, shadow hit id, outcome)."""
    rng = Stream(rng_seed(px, py, (frame ^ DI_SALT) & 0xFFFFFFFF))
    u0, u1, u2 = rng.unit(), rng.unit(), rng.unit()
    light = lights[min(int(u0 * len(lights)), len(lights) - 1)]
    cx, cy, cz, r = spheres[light]
    cone = sphere_cone(primary["P"], (cx, cy, cz), r, u1, u2)
    L, inv_pdf = cone if cone is not None else ((0.0, 0.0, 1.0), 0.0)
    zero = (0.0, 0.0, 0.0)
    if light == primary["id"] or cone is None or not dot(sv["FrontNg"], L) > 0.0:
        return zero, (light, L, inv_pdf, MISS, DI_NO_CANDIDATE)
    w = lobe_weights(b, sv, V)
    f = add(eval_of(b, sv, L, V, w, 0), eval_of(b, sv, L, V, w, 1))
    lm = materials[light]
    k = inv_pdf * len(lights)
    bound = max(f[c] * lm["EmissiveColor"][c] for c in range(3)) * lm["EmissiveStrength"] * k
    margins.append(abs(bound - DI_NEGLIGIBLE) / DI_NEGLIGIBLE)
    if not bound > DI_NEGLIGIBLE:
        return zero, (light, L, inv_pdf, MISS, DI_CULLED)
    sh = cast_ray(spheres, safe_origin(primary, L), L, 0.0, math.inf, materials, tex, margins)
    sid = MISS if sh is None else sh["id"]
    DI = zero
    if sid == light:
        e = evaluate_material(lm, sh, tex)
        DI = scale(mul(scale(tuple(e["EmissiveColor"]), e["EmissiveStrength"]), f), k)
    if not any(c > 0.0 for c in DI) or not finite3(DI):
        DI = zero
    return DI, (light, L, inv_pdf, sid, DI_SHADOW)


# ---------------------------------------------------------------- the pixel (Raytracing.hlsl:103-415, GBufferGeneration.hlsl:117-232)
def trace_pixel(spheres, materials, env_color, cam, w, h, frame, bounces, spp, rr, threshold, px, py, tex=None, env_map=None, di=False,
                record=None):
    """spheres: [(cx, cy, cz, r)], materials: [dict], cam: dict(Position, Right, Up, Forward, Near, Far, Jitter); tex: texture maps
    (see map_of), env_map: see environment, di: IsDIEnabled.
    Returns (rgb, events); event = dict(sample, bounce, id, t, L, T, rng, lobe, flag) -- flag as oracle_trace_pixel:
    0 continues, 1 primary miss, 2 bounce miss, 3 sample failed, 4 pdf 0, 5 f 0, 6 roulette, 7 throughput cut-off.
    record (a dict, optional) receives "margins" (per event: the smallest relative margin of the discrete decisions taken for it --
    alpha tests of the ray that found its hit, lobe choice, sidedness, Fresnel choice, roulette, cut-off) and "di" (the pixel's DI
    record: emitter, L, inv_pdf, shadow hit id, outcome, estimate; outcome DI_NONE without DI) with "di_margin"."""
    rng = Stream(rng_seed(px, py, frame))                         # :108
    u = (px + 0.5 + cam["Jitter"][0]) / w                          # Math.hlsli:7-10
    v = (py + 0.5 + cam["Jitter"][1]) / h
    ndc = (u * 2.0 - 1.0, v * -2.0 + 1.0)                          # :12-15
    d0 = unit(add(add(scale(cam["Right"], ndc[0]), scale(cam["Up"], ndc[1])), cam["Forward"]))  # Camera.hlsli:27-41
    inv_cos = 1.0 / dot(unit(cam["Forward"]), d0)
    o0 = tuple(cam["Position"])
    events, margins = [], []
    if record is None:
        record = {}
    record["margins"] = margins
    record["di"] = (MISS, (0.0, 0.0, 0.0), 0.0, MISS, DI_NONE, (0.0, 0.0, 0.0))
    record["di_margin"] = math.inf
    pm = []
    primary = cast_ray(spheres, o0, d0, cam["Near"] * inv_cos, cam["Far"] * inv_cos, materials, tex, pm)
    primary_margin = min(pm, default=math.inf)
    if primary is None:                                           # GBufferGeneration.hlsl:223-227; Raytracing.hlsl:249-252
        events.append({"sample": 0, "bounce": 0, "id": MISS, "t": math.inf, "L": (0, 0, 0), "T": (1, 1, 1), "rng": rng.state, "lobe": -1, "flag": 1})
        margins.append(primary_margin)
        return environment(env_color, d0, env_map), events
    # GBufferGeneration.hlsl:152-166: EvaluateMaterial at the primary hit; the shading normal it returns is the hit's
    pmat = evaluate_material(materials[primary["id"]], primary, tex)
    primary = {**primary, "Ns": pmat["Ns"]}
    lights = emitters(materials) if di else []
    DI, di_valid = (0.0, 0.0, 0.0), False
    if lights:
        b = bsdf_of(pmat, primary["front"], True)
        sv = {"FrontNg": primary["N"] if primary["front"] else neg(primary["N"]), "Ns": primary["Ns"], "basis": get_basis(primary["Ns"])}
        dm = []
        DI, rec = direct_illumination(spheres, materials, tex, px, py, frame, primary, b, sv, neg(d0), lights, dm)
        record["di"], record["di_margin"] = (*rec, DI), min(dm, default=math.inf)
        di_valid = True                                           # N4: the gate is "the pixel has a primary surface"
    radiance = (0.0, 0.0, 0.0)
    for s in range(spp):                                          # :191
        o, d, hit = o0, d0, primary
        T, sample_radiance, L, lobe = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), -1
        via_transmission = False
        for bounce in range(bounces + 1):                         # :213
            em = [primary_margin] if bounce == 0 else []
            if bounce:
                o, d = safe_origin(hit, L), L                     # :219-224
                hit = cast_ray(spheres, o, d, 0.0, math.inf, materials, tex, em)
            ev = {"sample": s, "bounce": bounce, "id": MISS if hit is None else hit["id"], "t": math.inf if hit is None else hit["t"], "lobe": lobe}

            def close(flag):
                events.append({**ev, "L": L, "T": T, "rng": rng.state, "flag": flag})
                margins.append(min(em, default=math.inf))
            if hit is None:                                       # :242-259
                sample_radiance = add(sample_radiance, mul(T, environment(env_color, d, env_map)))
                close(2)
                break
            mat = pmat if bounce == 0 else evaluate_material(materials[hit["id"]], hit, tex)   # :293-301
            hit = {**hit, "Ns": mat["Ns"]}
            b = bsdf_of(mat, hit["front"], bounce == 0)
            emission = scale(tuple(mat["EmissiveColor"]), mat["EmissiveStrength"])
            if di_valid and bounce == 1 and not via_transmission:  # :302 with the N4 departures
                emission = (0.0, 0.0, 0.0)
            sample_radiance = add(sample_radiance, mul(T, emission))  # :320
            sv = {"FrontNg": hit["N"] if hit["front"] else neg(hit["N"]), "Ns": hit["Ns"], "basis": get_basis(hit["Ns"])}  # SurfaceVectors.hlsli
            V = neg(d)
            w = lobe_weights(b, sv, V)
            rnd = (rng.unit(), rng.unit(), rng.unit(), rng.unit())   # :330
            ok, L, lobe = sample(b, sv, V, w, rnd, em)
            em.append(min(abs(rnd[0] - w[2]), abs(rnd[0] - (w[2] + w[1]))))   # FindLobe's comparisons
            if lobe != 2:
                em.append(abs(dot(sv["FrontNg"], L)))                # the sample's sidedness test
            ev["lobe"] = lobe
            if not ok:
                close(3); break
            pdf = pdf_of(b, sv, L, V, w, lobe)
            if pdf == 0.0:
                close(4); break
            f = eval_of(b, sv, L, V, w, lobe)
            if f == (0.0, 0.0, 0.0):
                close(5); break
            T = mul(T, scale(f, 1.0 / pdf))                        # :346
            if bounce == 0:
                via_transmission = lobe == 2
            if rr and bounce > 3:                                  # :348-356
                p = max(T)
                r = rng.unit()
                em.append(abs(r - p) / max(abs(p), 1e-30))
                if r >= p:
                    close(6); break
                T = scale(T, 1.0 / p)
            em.append(abs(lum(T) - threshold) / threshold)
            if lum(T) <= threshold:                                # :361
                close(7); break
            close(0)
        radiance = add(radiance, sample_radiance)                 # :373
    radiance = scale(radiance, 1.0 / spp) if finite3(radiance) else (0.0, 0.0, 0.0)   # :378
    if di:
        radiance = add(radiance, DI)                              # :381
    return radiance, events
