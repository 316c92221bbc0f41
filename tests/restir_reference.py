"""Row N10 -- a float64 restatement of DESIGN.md spec S16 (pt_restir_di), written from the spec, not from csrc/pt_restir.h: the surface of
RAB_GetGBufferSurface, the (emitter, u1, u2) sample and its target function, the initial / temporal / spatial passes with their three
normalisations, final shading; and a deterministic quadrature of the direct-light integral.  BSDF, cone sampling, RNG and the closest-hit
query are independent_tracer.py's (float64, written from the shaders)."""
import math

import numpy as np

import independent_tracer as it

SALT_INITIAL, SALT_TEMPORAL, SALT_SPATIAL = 0x52494E31, 0x52495431, 0x52495331
MIN_ROUGHNESS, DEPTH_T, NORMAL_T, OWN = 0.05, 0.1, 0.5, 1e-3
OFF, BASIC, RAYTRACED = 0, 1, 3
GOLDEN = float(np.float32(0.61803399))


def decode_oct(ex, ey):
    z = 1.0 - abs(ex) - abs(ey)
    x, y = ex, ey
    if z < 0.0:
        x = (1.0 - abs(ey)) * (1.0 if ex >= 0.0 else -1.0)
        y = (1.0 - abs(ex)) * (1.0 if ey >= 0.0 else -1.0)
    return it.unit((x, y, z))


def materials_of(mats):
    return [{k: (m[k].tolist() if hasattr(m[k], "tolist") else m[k]) for k in m.dtype.names} for m in mats]


class Scene:
    def __init__(self, spheres, mats):
        self.spheres = [tuple(float(s[k]) for k in ("cx", "cy", "cz", "r")) for s in spheres]
        self.materials = materials_of(mats)
        self.lights = it.emitters(self.materials)

    def first_hit(self, o, d):
        hit = it.cast_ray(self.spheres, o, d, 0.0, math.inf, self.materials, None, None)
        return (it.MISS, math.inf) if hit is None else (hit["id"], hit["t"])


def surface(gb, i, cam_pos):
    """gb: {channel: float array (n, width)}; None = no surface"""
    depth = float(gb["LinearDepth"][i, 0])
    nr = [float(x) for x in gb["NormalRoughness"][i]]
    if not math.isfinite(depth) or nr[3] < MIN_ROUGHNESS:
        return None
    pos = [float(x) for x in gb["Position"][i]]
    bcm = [float(x) for x in gb["BaseColorMetalness"][i]]
    P = tuple(pos[:3])
    V = it.unit(it.sub(cam_pos, P))
    Ng = decode_oct(float(gb["GeometricNormal"][i, 0]), float(gb["GeometricNormal"][i, 1]))
    front = it.dot(Ng, V) > 0.0
    Ns = tuple(nr[:3])
    sv = {"FrontNg": Ng if front else it.neg(Ng), "Ns": Ns, "basis": it.get_basis(Ns)}
    mat = {"BaseColor": bcm[:3] + [1.0], "Metallic": bcm[3], "Roughness": nr[3], "IOR": float(gb["IOR"][i, 0]),
           "Transmission": float(gb["Transmission"][i, 0]) if bcm[3] < 1.0 else 0.0}
    b = it.bsdf_of(mat, front, False)
    return {"P": P, "N": Ng, "offset": pos[3], "depth": depth, "V": V, "sv": sv, "b": b, "w": it.lobe_weights(b, sv, V)}


def shade(scene, s, j, u1, u2):
    """the sample aimed from surface s -> dict(sphere, L, inv_pdf, f_d, f_s, le, p_hat)"""
    sphere = scene.lights[min(j, len(scene.lights) - 1)]
    cx, cy, cz, r = scene.spheres[sphere]
    lm = scene.materials[sphere]
    le = it.scale(tuple(lm["EmissiveColor"]), lm["EmissiveStrength"])
    zero = (0.0, 0.0, 0.0)
    e = {"sphere": sphere, "L": (0.0, 0.0, 1.0), "inv_pdf": 0.0, "f_d": zero, "f_s": zero, "le": le, "p_hat": 0.0}
    cone = it.sphere_cone(s["P"], (cx, cy, cz), r, u1, u2)
    if cone is None:
        return e
    e["L"], e["inv_pdf"] = cone
    wv = it.sub((cx, cy, cz), s["P"])
    own = abs(it.dot(wv, wv) - r * r) <= OWN * r * r
    if own or not it.dot(s["sv"]["FrontNg"], e["L"]) > 0.0:
        return e
    f_d = it.eval_of(s["b"], s["sv"], e["L"], s["V"], s["w"], 0)
    f_s = it.eval_of(s["b"], s["sv"], e["L"], s["V"], s["w"], 1)
    p = it.lum(it.scale(it.mul(le, it.add(f_d, f_s)), e["inv_pdf"]))
    if p > 0.0 and math.isfinite(p):
        e.update(f_d=f_d, f_s=f_s, p_hat=p)
    return e


def visible(scene, s, e):
    hid, t = scene.first_hit(it.safe_origin(s, e["L"]), e["L"])
    return hid == e["sphere"], t


def empty_reservoir():
    return {"light": 0, "u1": 1.0, "u2": 1.0, "W": 0.0, "M": 0.0, "p_hat": 0.0, "age": 0}


def initial(scene, s, px, py, frame, n_samples, margins=None):
    rng = it.Stream(it.rng_seed(px, py, (frame ^ SALT_INITIAL) & 0xFFFFFFFF))
    r, w_sum, nl = empty_reservoir(), 0.0, len(scene.lights)
    for _ in range(n_samples):
        u0, u1, u2, rnd = rng.unit(), rng.unit(), rng.unit(), rng.unit()
        j = min(int(u0 * nl), nl - 1)
        e = shade(scene, s, j, u1, u2)
        w = e["p_hat"] * nl
        w_sum += w
        if w > 0.0:
            if margins is not None:
                margins.append(abs(rnd * w_sum - w) / w)
            if rnd * w_sum <= w:
                r.update(light=j, u1=u1, u2=u2, p_hat=e["p_hat"])
    r["M"] = float(n_samples)
    r["W"] = w_sum / (r["M"] * r["p_hat"]) if r["p_hat"] > 0.0 else 0.0
    if r["W"] > 0.0 and not visible(scene, s, shade(scene, s, r["light"], r["u1"], r["u2"]))[0]:
        r["W"] = 0.0
    return r


def temporal(scene, s, cur, prev_frame, px, py, w, h, mv, frame, bias, max_history, prev_cam_pos, margins=None):
    """prev_frame: (surfaces, reservoirs) of the previous call, or None.  Returns (reservoir, accepted)."""
    if prev_frame is None:
        return cur, False
    qx, qy = math.floor(px + mv[0] + 0.5), math.floor(py + mv[1] + 0.5)
    if not (0 <= qx < w and 0 <= qy < h):
        return cur, False
    qi = qy * w + qx
    ps = prev_frame[0](qi, prev_cam_pos)
    if ps is None:
        return cur, False
    expected = s["depth"] + mv[2]
    if margins is not None and expected != 0.0:
        margins.append(abs(abs(ps["depth"] - expected) - DEPTH_T * expected) / abs(expected))
        margins.append(abs(it.dot(s["sv"]["Ns"], ps["sv"]["Ns"]) - NORMAL_T))
    if not abs(ps["depth"] - expected) <= DEPTH_T * expected or not it.dot(s["sv"]["Ns"], ps["sv"]["Ns"]) >= NORMAL_T:
        return cur, False
    prev = dict(prev_frame[1][qi])
    if not prev["M"] > 0.0:
        return cur, False
    prev["M"] = min(prev["M"], max_history * cur["M"])
    rnd = it.Stream(it.rng_seed(px, py, (frame ^ SALT_TEMPORAL) & 0xFFFFFFFF)).unit()
    r = dict(cur)
    w_sum = cur["p_hat"] * cur["W"] * cur["M"]
    e = shade(scene, s, prev["light"], prev["u1"], prev["u2"])
    wt = e["p_hat"] * prev["W"] * prev["M"]
    w_sum += wt
    if wt > 0.0:
        if margins is not None:
            margins.append(abs(rnd * w_sum - wt) / wt)
        if rnd * w_sum <= wt:
            r.update(light=prev["light"], u1=prev["u1"], u2=prev["u2"], p_hat=e["p_hat"], age=prev["age"] + 1)
    r["M"] = cur["M"] + prev["M"]
    r["W"] = 0.0
    if not r["p_hat"] > 0.0:
        return r, True
    Z = r["M"]
    if bias != OFF:
        Z = cur["M"]
        ep = shade(scene, ps, r["light"], r["u1"], r["u2"])
        counts = ep["p_hat"] > 0.0
        if counts and bias == RAYTRACED:
            counts = visible(scene, ps, ep)[0]
        if counts:
            Z += prev["M"]
    r["W"] = w_sum / (Z * r["p_hat"])
    return r, True


def neighbour(px, py, w, h, k, rot, radius):
    rr = math.sqrt((k + 0.5) / 32.0) * radius
    a = k * GOLDEN + rot
    a -= math.floor(a)
    x = px + math.floor(rr * math.cos(2.0 * math.pi * a) + 0.5)
    y = py + math.floor(rr * math.sin(2.0 * math.pi * a) + 0.5)
    x, y = abs(x), abs(y)
    if x >= w:
        x = 2 * w - x - 1
    if y >= h:
        y = 2 * h - y - 1
    return min(max(x, 0), w - 1), min(max(y, 0), h - 1)


def similar(a, c):
    return (abs(a["rough"] - c["rough"]) <= 0.5 * max(a["rough"], c["rough"]) and abs(it.lum(a["f0"]) - it.lum(c["f0"])) <= 0.25
            and abs(it.lum(a["albedo"]) - it.lum(c["albedo"])) <= 0.25)


def spatial(scene, s, centre, surfaces, reservoirs, px, py, w, h, frame, bias, n_samples, radius, cam_pos):
    """surfaces(i, cam_pos) / reservoirs[i]: this call's temporal results.  Returns (reservoir, accepted neighbour indices)."""
    rng = it.Stream(it.rng_seed(px, py, (frame ^ SALT_SPATIAL) & 0xFFFFFFFF))
    start = rng.uint() & 31
    rot = rng.unit()
    r, w_sum, accepted = dict(centre), centre["p_hat"] * centre["W"] * centre["M"], []
    for i in range(n_samples):
        rnd = rng.unit()
        qx, qy = neighbour(px, py, w, h, (start + i) & 31, rot, radius)
        if (qx, qy) == (px, py):
            continue
        qi = qy * w + qx
        ns = surfaces(qi, cam_pos)
        if ns is None or not abs(ns["depth"] - s["depth"]) <= DEPTH_T * s["depth"] or not it.dot(s["sv"]["Ns"], ns["sv"]["Ns"]) >= NORMAL_T \
                or not similar(s["b"], ns["b"]):
            continue
        nr = reservoirs[qi]
        if not nr["M"] > 0.0:
            continue
        accepted.append(qi)
        e = shade(scene, s, nr["light"], nr["u1"], nr["u2"])
        wt = e["p_hat"] * nr["W"] * nr["M"]
        w_sum += wt
        if wt > 0.0 and rnd * w_sum <= wt:
            r.update(light=nr["light"], u1=nr["u1"], u2=nr["u2"], p_hat=e["p_hat"], age=nr["age"])
        r["M"] += nr["M"]
    if not accepted:
        return centre, accepted
    r["W"] = 0.0
    if not r["p_hat"] > 0.0:
        return r, accepted
    Z = r["M"]
    if bias != OFF:
        Z = centre["M"]
        for qi in accepted:
            ns = surfaces(qi, cam_pos)
            en = shade(scene, ns, r["light"], r["u1"], r["u2"])
            counts = en["p_hat"] > 0.0
            if counts and bias == RAYTRACED:
                counts = visible(scene, ns, en)[0]
            if counts:
                Z += reservoirs[qi]["M"]
    r["W"] = w_sum / (Z * r["p_hat"])
    return r, accepted


def final(scene, s, r):
    """-> (diffuse rgb, specular rgb, light distance) or None (not written); the emitters of these scenes carry no maps"""
    if not r["W"] > 0.0 or not math.isfinite(r["W"]):
        return None
    e = shade(scene, s, r["light"], r["u1"], r["u2"])
    if not e["p_hat"] > 0.0:
        return None
    vis, t = visible(scene, s, e)
    if not vis:
        return None
    k = e["inv_pdf"] * r["W"]
    d, sp = it.scale(it.mul(e["le"], e["f_d"]), k), it.scale(it.mul(e["le"], e["f_s"]), k)
    total = it.add(d, sp)
    if all(c == 0.0 for c in total) or not it.finite3(total):
        return None
    return d, sp, t


def quadrature(scene, s, k=12):
    """the direct-light integral at surface s: per emitter a k x k midpoint grid over its cone (u1, u2), brute-force visibility,
    Le (f_d + f_s) / pdf averaged -- deterministic, float64"""
    total = (0.0, 0.0, 0.0)
    for j in range(len(scene.lights)):
        acc = (0.0, 0.0, 0.0)
        for a in range(k):
            for c in range(k):
                e = shade(scene, s, j, (a + 0.5) / k, (c + 0.5) / k)
                if e["p_hat"] > 0.0 and visible(scene, s, e)[0]:
                    acc = it.add(acc, it.scale(it.mul(e["le"], it.add(e["f_d"], e["f_s"])), e["inv_pdf"]))
        total = it.add(total, it.scale(acc, 1.0 / (k * k)))
    return total
