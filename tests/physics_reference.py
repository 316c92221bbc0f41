"""Float64 restatement of spec S27 (row N23, pt_physics_*), written from DESIGN.md, not from csrc/pt_physics.h.

Every rule is written once over a number type: plain float64 numpy arrays, or `Err`, which carries with each value a bound on what
float32 evaluation of the same expression can differ from it by (running error analysis: every operation adds u |result| to the
propagated first-order error, u = 2^-24; a fused multiply-add rounds once where two operations are charged here, so the bound holds for it).
"""
import numpy as np

U = 2.0 ** -24
QUANTUM = 2.0 ** -24
CLAMP = 2.0 ** 15
GROWTH = 1.0 + 64 * U  # second-order terms of at most 64 chained operations


class Err:
    """value +- err, elementwise"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(np.asarray(x, np.float64))

    def _r(self, v, e):
        return Err(v, e * GROWTH + U * np.abs(v))

    def __add__(self, o):
        o = Err.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = self.v / o.v
            den = np.maximum(np.abs(o.v) - o.e, 1e-300)
            return self._r(r, (self.e + np.abs(r) * o.e) / den)

    def __rtruediv__(self, o):
        return Err.of(o) / self


def val(x):
    return x.v if isinstance(x, Err) else np.asarray(x, np.float64)


def err(x):
    return x.e if isinstance(x, Err) else np.zeros_like(np.asarray(x, np.float64))


def sqrt(x):
    if isinstance(x, Err):
        r = np.sqrt(np.maximum(x.v, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(r > 0, x.e / np.maximum(2.0 * r, 1e-300), np.sqrt(x.e))
        return x._r(r, e)
    return np.sqrt(x)


def maximum0(x):
    if isinstance(x, Err):
        return Err(np.maximum(x.v, 0.0), x.e)
    return np.maximum(x, 0.0)


def minimum(a, b):
    if isinstance(a, Err) or isinstance(b, Err):
        a, b = Err.of(a), Err.of(b)
        return Err(np.minimum(a.v, b.v), np.maximum(a.e, b.e))
    return np.minimum(a, b)


def where(c, a, b):
    if isinstance(a, Err) or isinstance(b, Err):
        a, b = Err.of(a), Err.of(b)
        return Err(np.where(c, a.v, b.v), np.where(c, a.e, b.e))
    return np.where(c, a, b)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def contact(xa, ra, xb, rb):
    """S27.3 -> (in contact, normal a -> b, penetration, distance - reach: the quantity whose sign decides)"""
    d = [xb[k] - xa[k] for k in range(3)]
    dist = sqrt(dot(d, d))
    reach = ra + rb
    zero = val(dist) == 0
    safe = where(zero, 1.0, dist)
    n = [where(zero, c, d[k] / safe) for k, c in enumerate((0.0, 1.0, 0.0))]
    return val(dist) < val(reach), n, reach - dist, dist - reach


def pair_impulse(q, prm):
    """S27.5, one pair of one iteration; q: xa ra xb rb va wa vb wb v0a v0b (3-lists or scalars of arrays), ima imb na nb;
    prm: h e mu beta slop threshold.  -> dict(hit, dva, dwa, dvb, dwb, lam, jt, decide: the quantities whose sign picks a branch)"""
    hit, n, pen, gap = contact(q["xa"], q["ra"], q["xb"], q["rb"])
    den = q["na"] * q["ima"] + q["nb"] * q["imb"]
    live = val(den) > 0
    den_s = where(live, den, 1.0)
    vn = dot([q["vb"][k] - q["va"][k] for k in range(3)], n)
    vn0 = dot([q["v0b"][k] - q["v0a"][k] for k in range(3)], n)
    approach = -vn0 - prm["threshold"]
    target = where(val(approach) > 0, -(prm["e"] * vn0), 0.0)
    bias = prm["beta"] * maximum0(pen - prm["slop"]) / prm["h"]
    lam = maximum0((target + bias - vn) / den_s)
    cb = [n[k] * -q["rb"] for k in range(3)]
    ca = [n[k] * q["ra"] for k in range(3)]
    sb, sa = cross(q["wb"], cb), cross(q["wa"], ca)
    vrel = [(q["vb"][k] + sb[k]) - (q["va"][k] + sa[k]) for k in range(3)]
    vrn = dot(vrel, n)
    vt = [vrel[k] - n[k] * vrn for k in range(3)]
    tl = sqrt(dot(vt, vt))
    slide = (val(tl) > 0) & (prm["mu"] > 0)
    tl_s = where(slide, tl, 1.0)
    jt = where(slide, minimum(tl / (3.5 * den_s), prm["mu"] * lam), 0.0)
    J = [n[k] * lam - where(slide, vt[k] * (jt / tl_s), 0.0) for k in range(3)]
    nxJ = cross(n, J)
    ka, kb = -(2.5 * q["ima"] / q["ra"]), -(2.5 * q["imb"] / q["rb"])
    return dict(hit=hit & live, dva=[-(J[k] * q["ima"]) for k in range(3)], dvb=[J[k] * q["imb"] for k in range(3)], dwa=[nxJ[k] * ka for k in range(3)],
                dwb=[nxJ[k] * kb for k in range(3)], lam=lam, jt=jt, decide=[gap, approach])


def integrate(x, rot, v, w, h):
    """S27.7 -> (x', rot'): x += h v, q += h/2 (w, 0) q renormalised; rot = [qx, qy, qz, qw]"""
    xn = [x[k] + v[k] * h for k in range(3)]
    k2 = 0.5 * h
    qv = rot[:3]
    c = cross(w, qv)
    dv = [w[k] * rot[3] + c[k] for k in range(3)]
    q = [rot[k] + k2 * dv[k] for k in range(3)] + [rot[3] - k2 * dot(w, qv)]
    ln = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    inv = 1.0 / ln
    return xn, [c_ * inv for c_ in q]


def acceleration(sph, bodies, attractors):
    """S27.2 in float64: sph (n, 4), bodies / attractors structured arrays -> (n, 3)"""
    sph = np.asarray(sph, np.float64)
    n = len(sph)
    a = np.zeros((n, 3))
    active = (bodies["InvMass"] > 0) & ((bodies["Flags"] & 4) == 0)
    spring = active & ((bodies["Flags"] & 1) != 0)
    a[spring, 1] = -(bodies["SpringOmega2"][spring].astype(np.float64) * (sph[spring, 1] - bodies["SpringY0"][spring].astype(np.float64)))
    for t in attractors:
        body, kind, strength, target = int(t["Body"]), int(t["Kind"]), float(t["Strength"]), int(t["Target"])
        d = sph[body, :3] - sph[:, :3]
        d2 = (d * d).sum(1)
        who = active & (np.arange(n) != body) & (d2 > 0)
        if target != 0xFFFFFFFF:
            who &= np.arange(n) == target
        dist = np.sqrt(d2[who])
        mag = strength / d2[who] if kind == 0 else np.full(dist.shape, strength)
        a[who] += d[who] * (mag / dist)[:, None]
    return a


class State64:
    """The whole step of S27 in float64, pairs by brute force, the fixed-point accumulators included (round to nearest even, clamp)"""

    def __init__(self, sph, bodies, lin_vel=None, ang_vel=None, rotations=None):
        self.sph = np.array(sph, np.float64).reshape(-1, 4)
        n = self.n = len(self.sph)
        self.bodies = np.array(bodies).copy()
        self.vel = np.zeros((n, 3)) if lin_vel is None else np.array(lin_vel, np.float64).reshape(n, 3)
        self.ang = np.zeros((n, 3)) if ang_vel is None else np.array(ang_vel, np.float64).reshape(n, 3)
        self.rot = np.tile([0.0, 0, 0, 1], (n, 1)) if rotations is None else np.array(rotations, np.float64).reshape(n, 4)
        self.contacts = 0

    def pairs(self):
        x, r = self.sph[:, :3], self.sph[:, 3]
        live = (self.bodies["Flags"] & 4) == 0
        d = np.sqrt(((x[None] - x[:, None]) ** 2).sum(-1))
        hit = (d < r[None] + r[:, None]) & live[None] & live[:, None]
        lo, hi = np.nonzero(np.triu(hit, 1))
        return lo, hi

    def step(self, s, attractors, h, quantise=True):
        prm = dict(h=h, e=float(s.Restitution), mu=float(s.Friction), beta=float(s.Baumgarte), slop=float(s.Slop), threshold=float(s.BounceThreshold))
        self.vel = self.vel + h * acceleration(self.sph, self.bodies, attractors)
        v0 = self.vel.copy()
        lo, hi = self.pairs() if self.n > 1 else (np.zeros(0, int), np.zeros(0, int))
        self.contacts = len(lo)
        count = np.bincount(np.concatenate([lo, hi]), minlength=self.n).astype(np.float64)
        im = self.bodies["InvMass"].astype(np.float64)
        for _ in range(s.Iterations or 4):
            if not len(lo):
                break
            T = lambda a, idx: [a[idx, k] for k in range(3)]  # noqa: E731
            q = dict(xa=T(self.sph, lo), ra=self.sph[lo, 3], xb=T(self.sph, hi), rb=self.sph[hi, 3], va=T(self.vel, lo), wa=T(self.ang, lo), vb=T(self.vel, hi),
                     wb=T(self.ang, hi), v0a=T(v0, lo), v0b=T(v0, hi), ima=im[lo], imb=im[hi], na=count[lo], nb=count[hi])
            r = pair_impulse(q, prm)
            dv, dw = np.zeros((self.n, 3)), np.zeros((self.n, 3))
            for name, acc, idx in (("dva", dv, lo), ("dvb", dv, hi), ("dwa", dw, lo), ("dwb", dw, hi)):
                c = np.stack(r[name], 1) * r["hit"][:, None]
                if quantise:
                    c = np.rint(np.clip(c, -CLAMP, CLAMP) / QUANTUM) * QUANTUM
                np.add.at(acc, idx, c)
            self.vel, self.ang = self.vel + dv, self.ang + dw
        live = (self.bodies["Flags"] & 4) == 0
        x, rot = integrate([self.sph[:, k] for k in range(3)], [self.rot[:, k] for k in range(4)], [self.vel[:, k] for k in range(3)], [self.ang[:, k] for k in range(3)], h)
        self.sph[live, :3] = np.stack(x, 1)[live]
        self.rot[live] = np.stack(rot, 1)[live]

    def kinetic_energy(self):
        im = self.bodies["InvMass"].astype(np.float64)
        m = np.where(im > 0, 1.0 / np.where(im > 0, im, 1.0), 0.0)
        inertia = 0.4 * m * self.sph[:, 3] ** 2
        return 0.5 * (m * (self.vel ** 2).sum(1)).sum() + 0.5 * (inertia * (self.ang ** 2).sum(1)).sum()
