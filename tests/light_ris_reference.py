"""Row N16 -- a float64 restatement of DESIGN.md spec S22 (local-light presampling of pt_restir_di_sampled), written from the spec, not
from csrc/pt_lightris.h: the emitters' powers, the Z-curve pyramid, a Power_RIS entry's walk down it, the ReGIR grid's cells, volume
target and build, and initial sampling over the three candidate sources.  RNG, emitter list and luminance are independent_tracer.py's;
the surface, the target function and visibility are restir_reference.py's (spec S16).

Every discrete choice records how close its comparison came to flipping: `margins` is a list the caller passes, and each item is
(kind, margin) -- "pick": |u n - nearest integer| / n of an index pick; "child": |u - prefix| / sum of a pyramid step; "ris":
|rnd w_sum - w| / w of a stream-RIS step; "cell": the distance of a cell coordinate to the nearest integer, in cells -- so a test can
exclude, and count, the entries whose float32 choice may legitimately differ."""
import math

import numpy as np

import independent_tracer as it
import restir_reference as ref

SALT_POWER, SALT_REGIR, SALT_REGIR_TILE, SALT_PIXEL_TILE = 0x4C525031, 0x4C525231, 0x4C525431, 0x4C525831
UNIFORM, POWER_RIS, REGIR_RIS = 0, 1, 2
INVALID = 0xFFFFFFFF
SQRT3, VOLUME_K = float(np.float32(1.7320508)), float(np.float32(1.1547))  # the spec's constants, as float32 holds them


def levels(n_lights):
    lv = 0
    while 4 ** lv < n_lights:
        lv += 1
    return lv


def power(scene, j):
    sphere = scene.lights[j]
    r = scene.spheres[sphere][3]
    m = scene.materials[sphere]
    p = r * r * it.lum(it.scale(tuple(m["EmissiveColor"]), m["EmissiveStrength"]))
    return p if p > 0.0 and math.isfinite(p) else 0.0


def pyramid(powers):
    """-> [level 0 (4^Lv leaves, padded with 0), ..., level Lv (one entry)], each level in Z-curve order: entry i of level k + 1 is a
    quarter of the sum of entries 4i .. 4i + 3 of level k"""
    lv = levels(len(powers))
    level = list(powers) + [0.0] * (4 ** lv - len(powers))
    out = [level]
    for _ in range(lv):
        level = [(level[4 * i] + level[4 * i + 1] + level[4 * i + 2] + level[4 * i + 3]) * 0.25 for i in range(len(level) // 4)]
        out.append(level)
    return out


def pick(u, n, margins=None):
    """pick_light: min(floor(u n), n - 1)"""
    x = u * n
    if margins is not None and n > 1:
        margins.append(("pick", abs(x - round(x)) / n))
    return min(int(x), n - 1)


def power_entry(pyr, t, s, frame, margins=None):
    """-> (emitter, 1 / pdf), or (INVALID, 0.0)"""
    lv = len(pyr) - 1
    rng = it.Stream(it.rng_seed(s, t, (frame ^ SALT_POWER) & 0xFFFFFFFF))
    node, pdf = 0, 1.0
    for level in range(lv - 1, -1, -1):
        q = pyr[level][4 * node:4 * node + 4]
        total = q[0] + q[1] + q[2] + q[3]
        if not total > 0.0:
            return INVALID, 0.0
        u = rng.unit() * total
        prefix = (q[0], q[0] + q[1], q[0] + q[1] + q[2], total)
        k = next(i for i in range(4) if prefix[i] >= u or i == 3)
        if margins is not None:
            margins.append(("child", min(abs(u - prefix[i]) for i in range(3)) / total))
        pdf *= q[k] / total
        node = 4 * node + k
    return node, 1.0 / pdf


def cell_centre(cam, grid, cell_size, cell):
    ix, iy, iz = cell % grid, (cell // grid) % grid, cell // (grid * grid)
    return tuple(cam[a] + (i + 0.5 - grid / 2) * cell_size for a, i in enumerate((ix, iy, iz)))


def volume_target(scene, j, centre, cell_size):
    sphere = scene.lights[j]
    cx, cy, cz, r = scene.spheres[sphere]
    m = scene.materials[sphere]
    R = SQRT3 * cell_size
    d = math.sqrt(sum((a - b) ** 2 for a, b in zip((cx, cy, cz), centre)))
    dist = d + R ** 3 / (d + VOLUME_K * R) ** 2
    t = min(math.pi * r * r / (dist * dist), 2.0 * math.pi) * it.lum(it.scale(tuple(m["EmissiveColor"]), m["EmissiveStrength"]))
    return t if t > 0.0 and math.isfinite(t) else 0.0


def regir_tile(g, frame, tile_count, margins=None):
    return pick(it.Stream(it.rng_seed(g >> 8, 0, (frame ^ SALT_REGIR_TILE) & 0xFFFFFFFF)).unit(), tile_count, margins)


def regir_entry(scene, cam, grid, cell_size, lights_per_cell, build_samples, tile, g, frame, margins=None):
    """tile: the (emitter, 1 / pdf) entries of the slot's Power_RIS tile -> (emitter, 1 / pdf) or (INVALID, 0.0)"""
    centre = cell_centre(cam, grid, cell_size, g // lights_per_cell)
    rng = it.Stream(it.rng_seed(g & 0xFFF, g >> 12, (frame ^ SALT_REGIR) & 0xFFFFFFFF))
    w_sum, sel, sel_target = 0.0, INVALID, 0.0
    for _ in range(build_samples):
        u, rnd = rng.unit(), rng.unit()
        j, inv = tile[pick(u, len(tile), margins)]
        target = w = 0.0
        if j != INVALID:
            target = volume_target(scene, j, centre, cell_size)
            w = target * inv
        w_sum += w
        if w > 0.0:
            if margins is not None:
                margins.append(("ris", abs(rnd * w_sum - w) / w))
            if rnd * w_sum <= w:
                sel, sel_target = j, target
    if sel == INVALID:
        return INVALID, 0.0
    return sel, w_sum / (build_samples * sel_target)


def cell_of(P, xi, cam, grid, cell_size, margins=None):
    """the cell of P' = P + (xi - 0.5) cell_size, or None outside the grid"""
    idx = []
    for a in range(3):
        x = (P[a] + (xi[a] - 0.5) * cell_size - cam[a]) / cell_size + grid / 2
        if margins is not None:
            margins.append(("cell", abs(x - round(x))))
        idx.append(math.floor(x))
    if not all(0 <= i < grid for i in idx):
        return None
    return (idx[2] * grid + idx[1]) * grid + idx[0]


def initial(scene, s, px, py, frame, n_samples, mode, ris=None, tile_size=0, tile_count=0, grid=0, lights_per_cell=0, cell_size=1.0, cam=None, margins=None):
    """spec S22's initial sampling: ris = the (emitter, 1 / pdf) entries of the Power segment then the ReGIR segment.  Uniform is S16's."""
    if mode == UNIFORM:
        plain = None if margins is None else []
        r = ref.initial(scene, s, px, py, frame, n_samples, plain)
        if margins is not None:
            margins.extend(("ris", m) for m in plain)
        return r
    rng = it.Stream(it.rng_seed(px, py, (frame ^ ref.SALT_INITIAL) & 0xFFFFFFFF))
    src = None
    if mode == REGIR_RIS:
        xi = (rng.unit(), rng.unit(), rng.unit())
        cell = cell_of(s["P"], xi, cam, grid, cell_size, margins)
        if cell is not None:
            first = tile_size * tile_count + cell * lights_per_cell
            src = ris[first:first + lights_per_cell]
    if src is None:
        tile = pick(it.Stream(it.rng_seed(px >> 4, py >> 4, (frame ^ SALT_PIXEL_TILE) & 0xFFFFFFFF)).unit(), tile_count, margins)
        src = ris[tile * tile_size:(tile + 1) * tile_size]
    r, w_sum = ref.empty_reservoir(), 0.0
    for _ in range(n_samples):
        u0, u1, u2, rnd = rng.unit(), rng.unit(), rng.unit(), rng.unit()
        j, inv = src[pick(u0, len(src), margins)]
        p_hat = ref.shade(scene, s, j, u1, u2)["p_hat"] if j != INVALID else 0.0
        w = p_hat * inv
        w_sum += w
        if w > 0.0:
            if margins is not None:
                margins.append(("ris", abs(rnd * w_sum - w) / w))
            if rnd * w_sum <= w:
                r.update(light=j, u1=u1, u2=u2, p_hat=p_hat)
    r["M"] = float(n_samples)
    r["W"] = w_sum / (r["M"] * r["p_hat"]) if r["p_hat"] > 0.0 else 0.0
    if r["W"] > 0.0 and not ref.visible(scene, s, ref.shade(scene, s, r["light"], r["u1"], r["u2"]))[0]:
        r["W"] = 0.0
    return r
