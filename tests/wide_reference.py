"""The 4-wide, quantised view of the tree ("4-wide view"; record layout: the comment above collapse4_kernel in
csrc/pt_lbvh_gpu.hip), restated in numpy from that text, and a checker of its properties in exact arithmetic.  No GPU, no product code.

The text, in the order the functions below follow it:
  * A binary node at EVEN depth becomes a wide node.  Its children are its grandchildren, in order child0's then child1's; a child that
    is a leaf stays as it is.  2 to 4 children.
  * Record i (16 dwords) lives in slot i of its own array; the slots of odd-depth nodes hold no record (zero).
      [0..2]   grid origin: per axis the minimum of the children's lower planes
      [3]      three biased exponents, x | y << 8 | z << 16: cell = 2^(e - 127), the smallest power of two above
               x = fp32(extent * fp32(1 / 254)), extent = fp32(max upper plane - origin): 254 * cell >= extent, and an x that is itself a
               power of two takes the next one.  An axis without extent stores e = 27 (2^-100); e is never below 7.
      [4..6]   lower x / y / z planes, child c in byte c; [7..9] upper planes
      [10..13] child references: >= 0 wide node, < 0 leaf ~k, 0x80000000 none;  [14..15] zero
  * A plane decodes as fma(byte, cell, origin), one rounding.  Builder's rule: lower byte = floor(fp32(lo - origin) / cell), upper byte =
    ceil(fp32(hi - origin) / cell), both clamped to [0, 255]; then the lower byte is decreased while it is above 0 and its decoded plane
    is above lo, and the upper byte increased while it is below 255 and its decoded plane is below hi.
"""
from fractions import Fraction

import numpy as np

EMPTY = np.uint32(0x80000000)


# ---------------------------------------------------------------------------------------------------------------- exact fma
def round32_fraction(x):
    """A Fraction -> the nearest float32, ties to even (finite results only)."""
    x = Fraction(x)
    if x == 0:
        return np.float32(0.0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1  # now 2^e <= a < 2^(e+1)
    q = max(e - 23, -149)  # the spacing of float32 around a is 2^q (subnormals: 2^-149)
    m = round(a / Fraction(2) ** q)  # Python rounds a Fraction half to even
    return np.float32(sign * float(m) * 2.0 ** q)  # m <= 2^24: float(m) * 2^q is exact in float64


def fma32(byte, cell, origin):
    """round32(byte * cell + origin), one rounding, elementwise: byte an integer in [0, 255], cell a power of two, origin float32.
    byte * cell is exact in float64.  The sum is taken in float64 and checked with the error term of Knuth's two-sum: where that is
    zero the float64 sum is exact and float64 -> float32 is the one rounding; elsewhere (an exponent gap beyond float64's 53 bits) the
    element is summed as a Fraction."""
    p = np.asarray(byte, dtype=np.float64) * np.asarray(cell, dtype=np.float64)
    o = np.asarray(origin, dtype=np.float64)
    p, o = np.broadcast_arrays(np.atleast_1d(p), np.atleast_1d(o))
    shape = np.broadcast_shapes(np.shape(byte), np.shape(cell), np.shape(origin))
    s = p + o
    bb = s - p
    err = (p - (s - bb)) + (o - bb)
    out = s.astype(np.float32)
    bad = np.nonzero(err != 0.0)
    for idx in zip(*bad):
        out[idx] = round32_fraction(Fraction(float(p[idx])) + Fraction(float(o[idx])))
    return out.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- topology
def depths(nodes):
    """depth of every binary node (root 0), by following `parent`"""
    parent = nodes["parent"].astype(np.int64)
    d = np.zeros(len(nodes), dtype=np.int64)
    cur = parent.copy()
    while (cur >= 0).any():
        live = cur >= 0
        d += live
        cur = np.where(live, parent[np.where(live, cur, 0)], -1)
    return d


def _children(nodes):
    """Per binary node the wide child list: lo, hi (n, 4, 3) float32, ref (n, 4) int64, count (n,).  Unused entries: ref = -2^31."""
    n = len(nodes)
    c = np.stack([nodes["child0"], nodes["child1"]], 1).astype(np.int64)  # (n, 2)
    lo = np.stack([nodes["lo0"], nodes["lo1"]], 1)  # (n, 2, 3): the boxes a node keeps of its two children
    hi = np.stack([nodes["hi0"], nodes["hi1"]], 1)
    # four candidates: (side 0, first), (side 0, second), (side 1, first), (side 1, second)
    cand_lo = np.zeros((n, 4, 3), np.float32); cand_hi = np.zeros((n, 4, 3), np.float32)
    cand_ref = np.full((n, 4), -2 ** 31, np.int64); valid = np.zeros((n, 4), bool)
    for side in range(2):
        leaf = c[:, side] < 0
        g = np.where(leaf, 0, c[:, side])  # the absorbed odd-depth child (index 0 as a harmless stand-in for leaves)
        cand_lo[:, 2 * side] = np.where(leaf[:, None], lo[:, side], lo[g, 0]); cand_hi[:, 2 * side] = np.where(leaf[:, None], hi[:, side], hi[g, 0])
        cand_ref[:, 2 * side] = np.where(leaf, c[:, side], c[g, 0]); valid[:, 2 * side] = True
        cand_lo[:, 2 * side + 1] = lo[g, 1]; cand_hi[:, 2 * side + 1] = hi[g, 1]
        cand_ref[:, 2 * side + 1] = np.where(leaf, -2 ** 31, c[g, 1]); valid[:, 2 * side + 1] = ~leaf
    order = np.argsort(~valid, axis=1, kind="stable")  # the valid candidates first, in their order
    rows = np.arange(n)[:, None]
    return cand_lo[rows, order], cand_hi[rows, order], cand_ref[rows, order], valid.sum(1)


def _cells(extent):
    """extent (float32, >= 0) -> (biased exponent, cell as float64)"""
    x = (extent * (np.float32(1.0) / np.float32(254.0))).astype(np.float32)
    _, e = np.frexp(x.astype(np.float64))  # x = m * 2^e, m in [0.5, 1): 2^e is the smallest power of two above x
    e = np.where(extent > 0, e, -100)
    e = np.maximum(e, -120)
    return (e + 127).astype(np.uint32), np.ldexp(1.0, e)


def collapse4(nodes):
    """binary records -> ((n_nodes, 16) uint32 wide records, mask of the populated slots)"""
    n = len(nodes)
    populated = depths(nodes) % 2 == 0
    lo, hi, ref, count = _children(nodes)
    used = np.arange(4)[None, :] < count[:, None]  # (n, 4)
    with np.errstate(invalid="ignore"):
        mn = np.where(used[:, :, None], lo, np.float32(np.inf)).min(1)  # (n, 3)
        mx = np.where(used[:, :, None], hi, np.float32(-np.inf)).max(1)
        extent = (mx - mn).astype(np.float32)
        be, cell = _cells(extent)
        c3, o3 = cell[:, None, :], mn[:, None, :]
        ql = np.clip(np.floor((lo - o3).astype(np.float32).astype(np.float64) / c3), 0, 255).astype(np.int64)
        qh = np.clip(np.ceil((hi - o3).astype(np.float32).astype(np.float64) / c3), 0, 255).astype(np.int64)
    live = used[:, :, None] & populated[:, None, None]
    while True:
        step = live & (ql > 0) & (fma32(ql, c3, o3) > lo)
        if not step.any():
            break
        ql -= step
    while True:
        step = live & (qh < 255) & (fma32(qh, c3, o3) < hi)
        if not step.any():
            break
        qh += step
    ql = np.where(used[:, :, None], ql, 0).astype(np.uint32); qh = np.where(used[:, :, None], qh, 0).astype(np.uint32)
    rec = np.zeros((n, 16), np.uint32)
    rec[:, 0:3] = np.ascontiguousarray(mn).view(np.uint32)
    rec[:, 3] = be[:, 0] | (be[:, 1] << 8) | (be[:, 2] << 16)
    shifts = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    rec[:, 4:7] = np.bitwise_or.reduce(ql << shifts, axis=1)
    rec[:, 7:10] = np.bitwise_or.reduce(qh << shifts, axis=1)
    rec[:, 10:14] = (ref & 0xFFFFFFFF).astype(np.uint32)
    rec[~populated] = 0
    return rec, populated


def decode(records):
    """-> lo, hi (n, 4, 3) float32 (child, axis; the exact fma), ref (n, 4) int64 (>= 0 node, < 0 leaf ~k, -2^31 none), cell (n, 3) float64,
    and the bytes ql, qh (n, 4, 3)"""
    rec = np.asarray(records, dtype=np.uint32)
    origin = np.ascontiguousarray(rec[:, 0:3]).view(np.float32)
    be = np.stack([(rec[:, 3] >> (8 * a)) & 0xFF for a in range(3)], 1).astype(np.int64)
    cell = np.ldexp(1.0, be - 127)
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    ql = ((rec[:, None, 4:7] >> sh) & 0xFF).astype(np.int64)
    qh = ((rec[:, None, 7:10] >> sh) & 0xFF).astype(np.int64)
    ref = rec[:, 10:14].astype(np.int64)
    ref = np.where(ref >= 2 ** 31, ref - 2 ** 32, ref)
    return fma32(ql, cell[:, None, :], origin[:, None, :]), fma32(qh, cell[:, None, :], origin[:, None, :]), ref, cell, ql, qh


# ---------------------------------------------------------------------------------------------------------------- the checker
class WideViolation(AssertionError):
    """check_wide's failure: `labels` is the set of violated properties ("P1" .. "P6")"""

    def __init__(self, failures):
        super().__init__("; ".join(failures))
        self.labels = {f[:2] for f in failures}


def _ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def check_wide(nodes, records, cleared=True):
    """Properties P1 to P6 of `records` (download_wide / collapse4) as the wide view of the binary records `nodes`; raises
    WideViolation naming every property that fails.  cleared: the buffer was zeroed before the even-depth slots were written."""
    rec = np.asarray(records, dtype=np.uint32)
    n = len(nodes)
    fails = []
    if rec.shape != (n, 16):
        raise WideViolation([f"P1: {rec.shape} is not ({n}, 16)"])
    d = depths(nodes)
    even = d % 2 == 0
    lo, hi, ref, count = _children(nodes)
    used = np.arange(4)[None, :] < count[:, None]
    dlo, dhi, rref, cell, ql, qh = decode(rec)
    E = even[:, None]

    # P1, slots: a record's first reference is never 0 (the root is nobody's child) nor empty; unwritten slots are zero
    if cleared and rec[~even].any():
        fails.append(f"P1: odd-depth slot {int(np.nonzero(rec[~even].any(1))[0][0])} (among the odd ones) is not zero")
    if ((rec[even, 10] == 0) | (rec[even, 10] == EMPTY)).any():
        fails.append(f"P1: even-depth slot {int(np.nonzero(even)[0][np.nonzero((rec[even, 10] == 0) | (rec[even, 10] == EMPTY))[0][0]])} holds no record")

    # P2, references: the list built from child0 then child1, the rest empty, words 14 and 15 zero, node references at even depth
    bad = E & (rref != ref)
    if bad.any():
        i, c = (int(v[0]) for v in np.nonzero(bad))
        fails.append(f"P2: node {i} child {c}: reference {int(rref[i, c])}, expected {int(ref[i, c])}")
    if rec[even, 14:16].any():
        fails.append("P2: words 14 / 15 are not zero")
    tgt = E & (rref >= 0)
    if (rref[tgt] >= n).any() or not even[np.minimum(rref[tgt], n - 1)].all():
        fails.append("P2: a node reference names no even-depth node")

    # P3, reachability: from wide node 0, every leaf and every even-depth node exactly once, nothing else
    seen_node = np.zeros(n, np.int64); seen_leaf = np.zeros(n + 1, np.int64); stray = 0
    frontier = np.array([0], np.int64); seen_node[0] = 1
    for _ in range(n + 2):
        if not len(frontier):
            break
        r = rref[frontier].ravel()
        r = r[r != -2 ** 31]
        leaves, inner = ~r[r < 0], r[r >= 0]
        stray += int((leaves > n).sum()) + int((inner >= n).sum())
        np.add.at(seen_leaf, leaves[leaves <= n], 1)
        inner = inner[inner < n]
        np.add.at(seen_node, inner, 1)
        frontier = inner[seen_node[inner] == 1] if (seen_node[inner] <= 1).all() else np.array([], np.int64)  # (a revisit ends the walk: it has failed)
    if stray or not (seen_leaf == 1).all() or not (seen_node == even).all():
        fails.append(f"P3: walk from wide node 0: {int((seen_leaf != 1).sum())} leaves and {int((seen_node != even).sum())} nodes not visited exactly as they should be, {stray} stray")

    # P4, containment: zero violations
    m = (E & used)[:, :, None]
    badl, badh = m & ~(dlo <= lo), m & ~(dhi >= hi)
    if badl.any() or badh.any():
        i, c, a = (int(v[0]) for v in np.nonzero(badl | badh))
        fails.append(f"P4: {int(badl.sum())} lower / {int(badh.sum())} upper planes inside the binary box; first: node {i} child {c} axis {a}: "
                     f"decoded [{dlo[i, c, a]!r}, {dhi[i, c, a]!r}] bytes ({ql[i, c, a]}, {qh[i, c, a]}) cell {cell[i, a]!r} "
                     f"origin {np.ascontiguousarray(rec[i, a:a + 1]).view(np.float32)[0]!r}, binary [{lo[i, c, a]!r}, {hi[i, c, a]!r}]")

    # P5, tightness.  U = one float32 ulp of the union box's largest |coordinate|.  floor leaves < one cell plus the rounding of lo - mn
    # (<= U / 2) plus the rounding of the decode (<= U / 2); a correction step is taken only while the decoded plane is on the wrong side,
    # i.e. while the exact plane is within U / 2 of it, and moves the exact plane by one cell, the decode rounding again by <= U / 2:
    # lo - decoded_lo < cell + 2U in every case, unless the byte is clamped.  The cell: 2^e is the smallest power of two above
    # x = fp32(extent * fp32(1/254)), so cell <= 2x and 127 * cell <= 254 x <= extent * (1 + 2^-23)^2 < extent * (1 + 2^-20).
    with np.errstate(invalid="ignore"):
        mn = np.where(used[:, :, None], lo, np.float32(np.inf)).min(1).astype(np.float64)
        mx = np.where(used[:, :, None], hi, np.float32(-np.inf)).max(1).astype(np.float64)
    U = _ulp32(np.maximum(np.abs(mn), np.abs(mx)).max(1))[:, None, None]
    bound = cell[:, None, :] + 2.0 * U
    free_l, free_h = m & (ql > 0) & (ql < 255), m & (qh > 0) & (qh < 255)
    slack_l = lo.astype(np.float64) - dlo.astype(np.float64); slack_h = dhi.astype(np.float64) - hi.astype(np.float64)
    loose = (free_l & ~(slack_l < bound)) | (free_h & ~(slack_h < bound))
    if loose.any():
        i, c, a = (int(v[0]) for v in np.nonzero(loose))
        fails.append(f"P5: {int(loose.sum())} planes further out than cell + 2U; first: node {i} child {c} axis {a}: slack ({slack_l[i, c, a]!r}, "
                     f"{slack_h[i, c, a]!r}), cell {cell[i, a]!r}, U {U[i, 0, 0]!r}")
    extent = mx - mn
    coarse = E & (extent > 0) & ~(127.0 * cell <= extent * (1.0 + 2.0 ** -20))
    if coarse.any():
        i, a = (int(v[0]) for v in np.nonzero(coarse))
        fails.append(f"P5: node {i} axis {a}: cell {cell[i, a]!r} for an extent of {extent[i, a]!r}")

    # P6, origin: the exact minimum of the children's lower planes
    origin = np.ascontiguousarray(rec[:, 0:3]).view(np.float32).astype(np.float64)
    bad = E & (origin != mn)
    if bad.any():
        i, a = (int(v[0]) for v in np.nonzero(bad))
        fails.append(f"P6: node {i} axis {a}: origin {origin[i, a]!r}, minimum of the lower planes {mn[i, a]!r}")
    if fails:
        raise WideViolation(fails)


def describe_difference(nodes, records, expected):
    """the first word in which two sets of records differ, with what went into it (T2's failure message)"""
    rec, exp = np.asarray(records, np.uint32), np.asarray(expected, np.uint32)
    i, w = (int(v[0]) for v in np.nonzero(rec != exp))
    lo, hi, ref, count = _children(nodes)
    msg = f"node {i} word {w}: {int(rec[i, w]):#010x}, expected {int(exp[i, w]):#010x}; children {int(count[i])}, references {ref[i, :count[i]].tolist()}"
    if 4 <= w < 10:
        a, upper = (w - 4) % 3, w >= 7
        c = int(np.nonzero(((rec[i, w] ^ exp[i, w]) >> (8 * np.arange(4, dtype=np.uint32))) & 0xFF)[0][0])
        origin = np.ascontiguousarray(rec[i, a:a + 1]).view(np.float32)[0]
        be = (int(rec[i, 3]) >> (8 * a)) & 0xFF
        msg += (f"; child {c} axis {a} {'upper' if upper else 'lower'} byte {(int(rec[i, w]) >> (8 * c)) & 0xFF}, expected {(int(exp[i, w]) >> (8 * c)) & 0xFF}; "
                f"plane {(hi if upper else lo)[i, c, a]!r}, origin {origin!r}, cell 2^{be - 127}")
    elif w == 3 or w < 3:
        msg += f"; lower planes {lo[i, :count[i]].tolist()}, upper planes {hi[i, :count[i]].tolist()}"
    return msg


# ---------------------------------------------------------------------------------------------------------------- the walk's stack (T5)
def stack_rays(name, n, seed):
    """n rays (float64) through the common centre of the `concentric` layout, or through the limit point of the `geometric` one
    (half of those nearly along its axis, so that they pierce many spheres), from origins at every scale of the layout"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    if name == "concentric":
        dist = rng.uniform(0.0, 400.0, (n, 1))
    else:
        u[::2] = np.array([1.0, 0.0, 0.0]) * rng.choice([-1.0, 1.0], (len(u[::2]), 1)) + rng.normal(size=(len(u[::2]), 3)) * 1e-3
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        dist = 2.0 ** rng.uniform(-1.0, 85.0, (n, 1))
    return u * dist, -u


def stack_model(records, o, d, tmin=0.0):
    """The wide walk's stack discipline (wide_visit, csrc/pt_trace.h) over `records`, all rays in lockstep: the children whose decoded box
    the ray meets are ordered near to far by the 5-exchange network, the nearest is descended into, the others are pushed far-first; a
    leaf pops.  Ray parameters in float64 on the decoded boxes, and no culling by a hit distance, so every child met is pushed: the device
    pushes a subset.  Returns the largest stack occupancy any ray saw."""
    dlo, dhi, ref, _, _, _ = decode(records)
    dlo, dhi = dlo.astype(np.float64), dhi.astype(np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    inv = 1.0 / np.where(d == 0.0, np.copysign(1e-30, d), d)
    n_rays, cap = len(o), 512
    stack = np.zeros((n_rays, cap), np.int64)
    node, sp, active, peak = np.zeros(n_rays, np.int64), np.zeros(n_rays, np.int64), np.ones(n_rays, bool), 0
    while active.any():
        idx = np.nonzero(active)[0]
        leaf = node[idx] < 0
        inner, pops = idx[~leaf], idx[leaf]
        if len(inner):
            nd = node[inner]
            t0 = (dlo[nd] - o[inner, None, :]) * inv[inner, None, :]
            t1 = (dhi[nd] - o[inner, None, :]) * inv[inner, None, :]
            tn, tf = np.maximum(np.minimum(t0, t1).max(2), tmin), np.maximum(t0, t1).min(2)
            r = ref[nd]
            tn = np.where((tn <= tf) & (r != -2 ** 31), tn, np.inf)
            for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                sw = tn[:, b] < tn[:, a]
                tn[:, a], tn[:, b] = np.where(sw, tn[:, b], tn[:, a]), np.where(sw, tn[:, a], tn[:, b])
                r[:, a], r[:, b] = np.where(sw, r[:, b], r[:, a]), np.where(sw, r[:, a], r[:, b])
            for k in (3, 2, 1):
                push = tn[:, k] < np.inf
                assert (sp[inner[push]] < cap).all()
                stack[inner[push], sp[inner[push]]] = r[push, k]
                sp[inner[push]] += 1
            peak = max(peak, int(sp[inner].max()))
            go = tn[:, 0] < np.inf
            node[inner[go]] = r[go, 0]
            pops = np.concatenate([pops, inner[~go]])
        done = sp[pops] == 0
        active[pops[done]] = False
        p = pops[~done]
        sp[p] -= 1
        node[p] = stack[p, sp[p]]
    return peak
