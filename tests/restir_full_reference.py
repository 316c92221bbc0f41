"""Row N22 -- a float64 restatement of DESIGN.md spec S26 (pt_restir_di_full), written from the spec, not from csrc/pt_restir.h: the
visibility word (what is known, the travelled offset with its sticky saturation, the gate of final shading) and pairwise MIS in the
temporal and the spatial pass.  Surfaces, samples, target function, neighbour table and RNG are restir_reference.py's."""
import math

import numpy as np

import restir_reference as ref

it = ref.it
PAIRWISE = 2
LIMIT = 127  # an axis of the offset holds -127 .. 127; beyond: saturated, for good


# ---------------------------------------------------------------------------------------------------- part 1: the visibility word
# a word is (seen, dx, dy); dx or dy None = saturated
NOTHING = (False, None, None)
FRESH = (True, 0, 0)


def encode(word):
    seen, dx, dy = word
    return int(seen) | ((0 if dx is None else dx + 128) << 8) | ((0 if dy is None else dy + 128) << 16)


def decode(bits):
    bx, by = (bits >> 8) & 0xFF, (bits >> 16) & 0xFF
    return bool(bits & 1), None if bx == 0 else bx - 128, None if by == 0 else by - 128


def moved(word, ddx, ddy):
    """the word of a sample that pixel (x + ddx, y + ddy) takes from pixel (x, y)"""
    def axis(v, d):
        if v is None or abs(v + d) > LIMIT:
            return None
        return v + d
    return word[0], axis(word[1], ddx), axis(word[2], ddy)


def usable(reuse, max_age, max_distance, age, word, alpha_tested=False):
    seen, dx, dy = word
    if not reuse or not seen or age > max_age or dx is None or dy is None or alpha_tested:
        return False
    md = float(np.float32(max_distance))
    return dx * dx + dy * dy <= md * md


# ---------------------------------------------------------------------------------------------------- part 2: pairwise MIS
def pairwise_weights(M_c, W_c, pc_yc, neighbours):
    """neighbours: [(M_i, W_i, p_i(y_i), p_c(y_i), p_i(y_c))] -> the k stream weights of the neighbours' samples, then the canonical's"""
    k = len(neighbours)
    out, m_c = [], 0.0
    for M_i, W_i, pi_yi, pc_yi, pi_yc in neighbours:
        den = M_i * pi_yi + (M_c / k) * pc_yi
        m_i = M_i * pi_yi / den if den > 0.0 else 0.0
        out.append(pc_yi * W_i * m_i / k)
        den = M_i * pi_yc + (M_c / k) * pc_yc
        m_c += (M_c / k) * pc_yc / den if den > 0.0 else 1.0
    out.append(pc_yc * W_c * (m_c / k))
    return out


def stream(weights, rnds, margins):
    """streaming RIS over the weights in order -> (index selected or None, w_sum); margins gets |rnd w_sum - w| / w of every decision"""
    sel, w_sum = None, 0.0
    for i, (w, rnd) in enumerate(zip(weights, rnds)):
        w_sum += w
        if w > 0.0:
            margins.append(abs(rnd * w_sum - w) / w)
            if rnd * w_sum <= w:
                sel = i
    return sel, w_sum


def finish(r, w_sum):
    r["W"] = w_sum / r["p_hat"] if r["p_hat"] > 0.0 else 0.0
    if not math.isfinite(r["W"]):
        r["W"] = 0.0
    return r


def temporal_pairwise(scene, s, cur, prev_surface, prev_reservoirs, px, py, w, h, mv, frame, max_history, prev_cam_pos, margins):
    """cur: this call's initial reservoir (with its word under "vis"); prev_surface(i, cam_pos) / prev_reservoirs[i]: the previous call's.
    Returns (reservoir, accepted)."""
    qx, qy = math.floor(px + mv[0] + 0.5), math.floor(py + mv[1] + 0.5)
    if not (0 <= qx < w and 0 <= qy < h):
        return cur, False
    qi = qy * w + qx
    ps = prev_surface(qi, prev_cam_pos)
    if ps is None:
        return cur, False
    expected = s["depth"] + mv[2]
    if expected != 0.0:
        margins.append(abs(abs(ps["depth"] - expected) - ref.DEPTH_T * expected) / abs(expected))
    margins.append(abs(it.dot(s["sv"]["Ns"], ps["sv"]["Ns"]) - ref.NORMAL_T))
    if not abs(ps["depth"] - expected) <= ref.DEPTH_T * expected or not it.dot(s["sv"]["Ns"], ps["sv"]["Ns"]) >= ref.NORMAL_T:
        return cur, False
    prev = dict(prev_reservoirs[qi])
    if not prev["M"] > 0.0:
        return cur, False
    prev["M"] = min(prev["M"], max_history * cur["M"])
    rng = it.Stream(it.rng_seed(px, py, (frame ^ ref.SALT_TEMPORAL) & 0xFFFFFFFF))
    rnds = [rng.unit(), rng.unit()]
    pc_yi = ref.shade(scene, s, prev["light"], prev["u1"], prev["u2"])["p_hat"]
    pi_yc = ref.shade(scene, ps, cur["light"], cur["u1"], cur["u2"])["p_hat"]
    weights = pairwise_weights(cur["M"], cur["W"], cur["p_hat"], [(prev["M"], prev["W"], prev["p_hat"], pc_yi, pi_yc)])
    sel, w_sum = stream(weights, rnds, margins)
    r = dict(cur)
    if sel == 0:
        r.update(light=prev["light"], u1=prev["u1"], u2=prev["u2"], p_hat=pc_yi, age=prev["age"] + 1, vis=moved(prev["vis"], px - qx, py - qy))
    r["M"] = cur["M"] + prev["M"]
    return finish(r, w_sum), True


def spatial_pairwise(scene, s, centre, surfaces, reservoirs, px, py, w, h, frame, n_samples, radius, cam_pos, margins):
    """surfaces(i, cam_pos) / reservoirs[i]: this call's launch-1 results.  Returns (reservoir, accepted neighbour indices)."""
    rng = it.Stream(it.rng_seed(px, py, (frame ^ ref.SALT_SPATIAL) & 0xFFFFFFFF))
    start = rng.uint() & 31
    rot = rng.unit()
    accepted, rnds = [], []
    for i in range(n_samples):
        rnd = rng.unit()
        qx, qy = ref.neighbour(px, py, w, h, (start + i) & 31, rot, radius)
        if (qx, qy) == (px, py):
            continue
        qi = qy * w + qx
        ns = surfaces(qi, cam_pos)
        if ns is None:
            continue
        margins.append(abs(abs(ns["depth"] - s["depth"]) - ref.DEPTH_T * s["depth"]) / s["depth"])
        margins.append(abs(it.dot(s["sv"]["Ns"], ns["sv"]["Ns"]) - ref.NORMAL_T))
        a, c = s["b"], ns["b"]
        margins.append(abs(abs(a["rough"] - c["rough"]) - 0.5 * max(a["rough"], c["rough"])))
        margins.append(abs(abs(it.lum(a["f0"]) - it.lum(c["f0"])) - 0.25))
        margins.append(abs(abs(it.lum(a["albedo"]) - it.lum(c["albedo"])) - 0.25))
        if not abs(ns["depth"] - s["depth"]) <= ref.DEPTH_T * s["depth"] or not it.dot(s["sv"]["Ns"], ns["sv"]["Ns"]) >= ref.NORMAL_T or not ref.similar(a, c):
            continue
        if not reservoirs[qi]["M"] > 0.0:
            continue
        accepted.append((qi, qx, qy))
        rnds.append(rnd)
    if not accepted:
        return centre, []
    rnds.append(rng.unit())
    rows = []
    for qi, qx, qy in accepted:
        nr = reservoirs[qi]
        pc_yi = ref.shade(scene, s, nr["light"], nr["u1"], nr["u2"])["p_hat"]
        pi_yc = ref.shade(scene, surfaces(qi, cam_pos), centre["light"], centre["u1"], centre["u2"])["p_hat"]
        rows.append((nr["M"], nr["W"], nr["p_hat"], pc_yi, pi_yc))
    weights = pairwise_weights(centre["M"], centre["W"], centre["p_hat"], rows)
    sel, w_sum = stream(weights, rnds, margins)
    r = dict(centre)
    if sel is not None and sel < len(accepted):
        qi, qx, qy = accepted[sel]
        nr = reservoirs[qi]
        r.update(light=nr["light"], u1=nr["u1"], u2=nr["u2"], p_hat=rows[sel][3], age=nr["age"], vis=moved(nr["vis"], px - qx, py - qy))
    r["M"] = centre["M"] + sum(reservoirs[qi]["M"] for qi, _, _ in accepted)
    return finish(r, w_sum), [qi for qi, _, _ in accepted]
