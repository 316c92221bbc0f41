"""Row N17 -- a float64 restatement of DESIGN.md spec S23 (pt_restir_di_ex: BRDF candidates in initial sampling, the boiling filter),
written from the spec, not from csrc/pt_restir.h: the inverse of the cone sample, the lobe-summed BSDF pdf, the balance-heuristic
weights of the local and the BRDF candidates, the source pdf the BRDF side prices an emitter with, and the filter over a block of 64
weights.  The surface, the target function and visibility are restir_reference.py's (spec S16); the candidates' sources are
light_ris_reference.py's (spec S22); BSDF sampling, RNG and the closest-hit query are independent_tracer.py's.

Every discrete choice records how close its comparison came to flipping, as light_ris_reference.py does: `margins` is a list of
(kind, margin) -- besides its kinds, "lobe": |r0 - a lobe threshold|; "fresnel": the transmission lobe's reflect / refract choice;
"horizon": |dot(FrontNg, L)|; "hit": the smallest angle by which a ray would have to turn to graze a sphere's silhouette (or the relative
gap between its two nearest hits); "clamp": the inverted u1's distance to its upper clamp, scaled by r / d (the relative error of
1 - cos(theta) grows as d / r)."""
import math

import numpy as np

import independent_tracer as it
import light_ris_reference as lr
import restir_reference as ref

UNIFORM, POWER_RIS, REGIR_RIS = lr.UNIFORM, lr.POWER_RIS, lr.REGIR_RIS
MIN_U = 2.0 ** -24
ATAN_C = [float(np.float32(c)) for c in (0.99997726, -0.33262347, 0.19354346, -0.11643287, 0.05265332, -0.01172120)]  # spec S8's polynomial


def atan2_spec(y, x):
    """spec S8's atan2: a fixed odd polynomial in min / max of the magnitudes, unfolded by octant; atan2(0, 0) = 0"""
    ax, ay = abs(x), abs(y)
    mx, mn = (ax, ay) if ax > ay else (ay, ax)
    if not mx > 0.0:
        return 0.0
    a = mn / mx
    s = a * a
    r = a * (ATAN_C[0] + s * (ATAN_C[1] + s * (ATAN_C[2] + s * (ATAN_C[3] + s * (ATAN_C[4] + s * ATAN_C[5])))))
    if ay > ax:
        r = float(np.float32(math.pi / 2)) - r
    if x < 0.0:
        r = float(np.float32(math.pi)) - r
    return -r if y < 0.0 else r


def invert_cone(P, C, r, L, margins=None):
    """the (u1, u2) in (0, 1]^2 whose cone sample from P towards the sphere (C, r) is L; P inside the sphere: (1, 1)"""
    w = it.sub(C, P)
    d2 = it.dot(w, w)
    if not d2 > r * r:
        return 1.0, 1.0
    sin2 = r * r / d2
    omc = sin2 / (1.0 + math.sqrt(it.saturate(1.0 - sin2)))
    l = it.to_local(it.get_basis(it.unit(w)), L)
    a = (l[0] * l[0] + l[1] * l[1]) / (1.0 + l[2]) / omc
    if margins is not None:
        margins.append(("clamp", abs(a - 1.0) * math.sqrt(sin2)))
    u1 = MIN_U if not a > MIN_U else min(a, 1.0)
    t = atan2_spec(l[1], l[0]) / (2.0 * math.pi)
    if not t > 0.0:
        t += 1.0
    u2 = MIN_U if not t > MIN_U else min(t, 1.0)
    return u1, u2


def pdf_all(b, sv, L, V, w):
    """BSDFSample::EvaluatePDF without a lobe: transmission where its weight is > 0, the reflective lobes where it is < 1 and L is above
    the geometric horizon"""
    pdf = 0.0
    if w[2] > 0.0:
        pdf = it.pdf_of(b, sv, L, V, w, 2)
    if w[2] < 1.0 and it.dot(sv["FrontNg"], L) > 0.0:
        pdf += it.pdf_of(b, sv, L, V, w, 0) + it.pdf_of(b, sv, L, V, w, 1)
    return pdf


def source_pdf(scene, mode, j, pyr=None):
    """how the BRDF side prices the light technique's choice of emitter j: 1 / n_lights, or power_j / sum of powers (leaf over top of
    S22's pyramid, whose top is the mean over 4^Lv leaves)"""
    if mode == UNIFORM:
        return 1.0 / len(scene.lights)
    top = pyr[-1][0] * len(pyr[0])
    return pyr[0][j] / top if top > 0.0 else 0.0


def mis_weight(p_hat, w_l, p_src, w_b, p_brdf, inv_pdf):
    if not p_hat > 0.0:
        return 0.0
    w = p_hat / (w_l * p_src + w_b * (p_brdf * inv_pdf))
    return w if w > 0.0 and math.isfinite(w) else 0.0


def hit_margin(scene, o, d):
    """how close a ray's first hit is to changing: the angle to the nearest silhouette (spheres ahead that do not contain the origin;
    independent_tracer.cast_ray's measure), and the relative gap of the two nearest hits"""
    best, ts = math.inf, []
    for i, (cx, cy, cz, r) in enumerate(scene.spheres):
        oc = it.sub((cx, cy, cz), o)
        along, dist = it.dot(oc, d), math.sqrt(it.dot(oc, oc))
        if along > 0.0 and dist > r:
            best = min(best, abs(math.sqrt(max(dist * dist - along * along, 0.0)) - r) / dist)
        hit = it.hit_sphere(o, d, 0.0, math.inf, (cx, cy, cz), r)
        if hit is not None:
            ts.append(hit)
    ts.sort()
    if len(ts) > 1:
        best = min(best, (ts[1] - ts[0]) / ts[1])
    return best


def initial(scene, s, px, py, frame, n_local, n_brdf, mode=UNIFORM, ris=None, pyr=None, tile_size=0, tile_count=0, grid=0, lights_per_cell=0, cell_size=1.0,
            cam=None, margins=None):
    """spec S23's initial sampling: n_local candidates from the mode's source and n_brdf BSDF-sampled ones, one stream; M = n_local + n_brdf"""
    rng = it.Stream(it.rng_seed(px, py, (frame ^ ref.SALT_INITIAL) & 0xFFFFFFFF))
    n_all = n_local + n_brdf
    w_l, w_b = n_local / n_all, n_brdf / n_all
    nl = len(scene.lights)
    src = None
    if mode == REGIR_RIS:
        xi = (rng.unit(), rng.unit(), rng.unit())
        cell = lr.cell_of(s["P"], xi, cam, grid, cell_size, margins)
        if cell is not None:
            first = tile_size * tile_count + cell * lights_per_cell
            src = ris[first:first + lights_per_cell]
    if mode != UNIFORM and src is None:
        tile = lr.pick(it.Stream(it.rng_seed(px >> 4, py >> 4, (frame ^ lr.SALT_PIXEL_TILE) & 0xFFFFFFFF)).unit(), tile_count, margins)
        src = ris[tile * tile_size:(tile + 1) * tile_size]
    r, w_sum = ref.empty_reservoir(), 0.0

    def stream(w, rnd, **sample):
        nonlocal w_sum
        w_sum += w
        if w > 0.0:
            if margins is not None:
                margins.append(("ris", abs(rnd * w_sum - w) / w))
            if rnd * w_sum <= w:
                r.update(**sample)

    for _ in range(n_local):
        u0, u1, u2, rnd = rng.unit(), rng.unit(), rng.unit(), rng.unit()
        if mode == UNIFORM:
            j, p_sel = lr.pick(u0, nl, margins), 1.0 / nl
        else:
            j, inv = src[lr.pick(u0, len(src), margins)]
            p_sel = 1.0 / inv if j != lr.INVALID else 0.0
        w = p_hat = 0.0
        if j != lr.INVALID:
            e = ref.shade(scene, s, j, u1, u2)
            p_hat = e["p_hat"]
            if p_hat > 0.0:
                w = mis_weight(p_hat, w_l, p_sel, w_b, pdf_all(s["b"], s["sv"], e["L"], s["V"], s["w"]), e["inv_pdf"])
        stream(w, rnd, light=j, u1=u1, u2=u2, p_hat=p_hat)
    for _ in range(n_brdf):
        q = (rng.unit(), rng.unit(), rng.unit(), rng.unit())
        rnd = rng.unit()
        if margins is not None:
            margins.append(("lobe", min(abs(q[0] - s["w"][2]), abs(q[0] - (s["w"][2] + s["w"][1])))))
            fm = []
            ok, L, lobe = it.sample(s["b"], s["sv"], s["V"], s["w"], q, fm)
            margins.extend(("fresnel", m) for m in fm)
            margins.append(("horizon", abs(it.dot(s["sv"]["FrontNg"], L))))
        else:
            ok, L, lobe = it.sample(s["b"], s["sv"], s["V"], s["w"], q)
        w = p_hat = 0.0
        j, u1, u2 = 0xFFFFFFFF, 1.0, 1.0
        if ok and it.dot(s["sv"]["FrontNg"], L) > 0.0:
            o = it.safe_origin(s, L)
            if margins is not None:
                margins.append(("hit", hit_margin(scene, o, L)))
            hid, _t = scene.first_hit(o, L)
            if hid != it.MISS and hid in scene.lights:
                j = scene.lights.index(hid)
                cx, cy, cz, rad = scene.spheres[hid]
                u1, u2 = invert_cone(s["P"], (cx, cy, cz), rad, L, margins)
                e = ref.shade(scene, s, j, u1, u2)
                p_hat = e["p_hat"]
                if p_hat > 0.0:
                    w = mis_weight(p_hat, w_l, source_pdf(scene, mode, j, pyr), w_b, pdf_all(s["b"], s["sv"], e["L"], s["V"], s["w"]), e["inv_pdf"])
        stream(w, rnd, light=j, u1=u1, u2=u2, p_hat=p_hat)
    r["M"] = float(n_all)
    r["W"] = w_sum / (r["M"] * r["p_hat"]) if r["p_hat"] > 0.0 else 0.0
    if r["W"] > 0.0:
        e = ref.shade(scene, s, r["light"], r["u1"], r["u2"])
        if margins is not None:
            margins.append(("hit", hit_margin(scene, it.safe_origin(s, e["L"]), e["L"])))
        if not ref.visible(scene, s, e)[0]:
            r["W"] = 0.0
    return r


# ---------------------------------------------------------------- the boiling filter
def boiling_multiplier(strength):
    return 10.0 / min(max(strength, 1e-6), 1.0) - 9.0


def butterfly_sum32(w):
    """the sum of 64 float32 weights in the spec's order: six levels, level k adding the partial sums of lanes that differ in bit k"""
    v = np.asarray(w, np.float32).copy()
    assert v.shape == (64,)
    lanes = np.arange(64)
    for k in range(6):
        v = (v + v[lanes ^ (1 << k)]).astype(np.float32)
    assert (v.view(np.uint32) == v.view(np.uint32)[0]).all() or np.isnan(v).all()
    return v[0]


def boiling(w, strength):
    """-> (S, n, emptied flags) for one block of 64 weights (lanes without a surface carry 0)"""
    w = np.asarray(w, np.float64)
    n = int((w > 0).sum())
    S = float(butterfly_sum32(w))
    avg = S / n if n else 0.0
    return S, n, w > avg * boiling_multiplier(strength)
