"""Row N23 -- pt_physics_*: the rigid-sphere dynamics stand-in for PhysX (DESIGN.md spec S27).
CPU: the host-compiled header (tests/hostshim/physics_host.cpp over csrc/pt_physics.h) against the float64 restatement of S27
(physics_reference.py) within a running-error bound plus one quantum, known answers, the handler rule with and without LARGE bodies,
closed forms, resting contact, energy, momentum, the freeze and the clamp, a sanitizer build of a stand-alone program, the ABI.
GPU: the device state against the host header bit for bit over sizes, degenerate layouts, LARGE bodies, attractors, substeps, the
tree rebuilt or only refitted, a step queued behind frames in flight, the loop into pt_render against the oracle, argument errors, the
C++ mirror."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import physics_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -24
BODY = np.dtype([("InvMass", np.float32), ("Flags", np.uint32), ("SpringY0", np.float32), ("SpringOmega2", np.float32)])
ATTRACTOR = np.dtype([("Body", np.uint32), ("Kind", np.uint32), ("Strength", np.float32), ("Target", np.uint32)])
SPRING, LARGE, DISABLED = 1, 2, 4
ALL = 0xFFFFFFFF
NO_ATTRACTORS = np.zeros(0, ATTRACTOR)


def p(a):
    return None if a is None else a.ctypes.data


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


import dxrs_amd_loader  # noqa: E402,F401
from dxrs_amd.abi_types import PtPhysicsSettings as Settings  # noqa: E402


def settings(iterations=4, rebuild=0, e=0.6, mu=0.5, beta=0.2, slop=0.005, threshold=2.0):
    return Settings(iterations, rebuild, e, mu, beta, slop, threshold, 0)


@pytest.fixture(scope="module")
def ph():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_physics_shim())
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    lib.ph_host_create.restype = vp
    lib.ph_host_create.argtypes = [vp, vp, vp, vp, vp, u32]
    for name, args in dict(ph_host_destroy=[vp], ph_host_step=[vp, C.POINTER(Settings), vp, u32, f32, u32, vp], ph_host_download=[vp, vp, vp, vp, vp, vp, vp],
                           ph_host_pairs=[vp, vp, u32, vp, vp, vp], ph_host_integrate=[vp, u32, f32, vp], ph_host_quantize=[vp, u32, vp, vp],
                           ph_host_apply=[vp, vp, u32, vp], ph_host_acceleration=[vp, vp, u32, vp, u32, vp]).items():
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    return lib


class Host:
    """pt_physics_* over the host-compiled header"""

    def __init__(self, lib, sph, bodies, lin=None, ang=None, rot=None, s=None, attractors=NO_ATTRACTORS):
        self.lib, self.n = lib, len(sph)
        self.s, self.attractors = s or settings(), np.ascontiguousarray(attractors, ATTRACTOR)
        a = [None if x is None else np.ascontiguousarray(x, np.float32) for x in (sph, lin, ang, rot)]
        self.h = lib.ph_host_create(p(a[0]), p(np.ascontiguousarray(bodies, BODY)), p(a[1]), p(a[2]), p(a[3]), self.n)

    def step(self, dt, substeps=1):
        r = np.zeros(4, np.uint32)
        self.lib.ph_host_step(self.h, C.byref(self.s), p(self.attractors), len(self.attractors), dt, substeps, p(r))
        return r

    def state(self):
        """-> spheres, rotations, lin_vel, ang_vel, flags, rule violations"""
        n = self.n
        out = [np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)]
        v = C.c_uint32(0)
        self.lib.ph_host_download(self.h, *[p(a) for a in out], C.addressof(v))
        return (*out, v.value)

    def close(self):
        self.lib.ph_host_destroy(self.h)


def density_bodies(radii, flags=0):
    b = np.zeros(len(radii), BODY)
    b["InvMass"] = (1.0 / (4.0 / 3.0 * np.pi * np.asarray(radii, np.float64) ** 3)).astype(np.float32)
    b["Flags"] = flags
    return b


def cluster(seed, n, fill=0.3, speed=1.0):
    """n spheres of radius 0.05 .. 0.15 in a cube filled to `fill`: many in contact; random velocities, spins and orientations; every eighth
    body immovable, every fifth on a spring"""
    rng = np.random.default_rng(seed)
    r = (0.05 * 3.0 ** rng.random(n)).astype(np.float32)
    side = max((float((4.0 / 3.0 * np.pi * r.astype(np.float64) ** 3).sum()) / fill) ** (1.0 / 3.0), 0.2) if n else 1.0
    sph = np.concatenate([rng.uniform(0, side, (n, 3)), r[:, None]], 1).astype(np.float32)
    bodies = density_bodies(r)
    bodies["InvMass"][::8] = 0
    bodies["Flags"][::5] |= SPRING
    bodies["SpringY0"] = sph[:, 1] + 0.1
    bodies["SpringOmega2"] = np.float32(4 * np.pi ** 2 / 9.0)
    lin = (speed * rng.normal(size=(n, 3))).astype(np.float32)
    ang = (3.0 * rng.normal(size=(n, 3))).astype(np.float32)
    rot = rng.normal(size=(n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32) if n else rot.astype(np.float32)
    return sph, bodies, lin, ang, rot


# ------------------------------------------------------------------------------------------------ restatement
def random_pairs(rng, n):
    """n pairs as ph_host_pairs takes them: a tenth apart, a twentieth coincident, a tenth with an immovable body, a few with both"""
    f = np.zeros((n, 28), np.float32)
    ra, rb = 0.05 * 20.0 ** rng.random(n), 0.05 * 20.0 ** rng.random(n)
    xa = rng.uniform(-5, 5, (n, 3))
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    gap = np.where(rng.random(n) < 0.1, rng.uniform(1.01, 2.0, n), rng.uniform(0.5, 0.999, n))
    gap[rng.random(n) < 0.05] = 0.0
    f[:, 0:3], f[:, 3], f[:, 4:7], f[:, 7] = xa, ra, xa + direction * (gap * (ra + rb))[:, None], rb
    f[:, 8:20] = rng.normal(size=(n, 12)) * np.array([2.0] * 3 + [5.0] * 3 + [2.0] * 3 + [5.0] * 3)
    f[:, 20:26] = f[:, [8, 9, 10, 14, 15, 16]] + rng.normal(size=(n, 6)) * 0.3
    f[:, 26], f[:, 27] = 1.0 / (4.19 * ra ** 3), 1.0 / (4.19 * rb ** 3)
    f[rng.random(n) < 0.1, 26] = 0
    f[rng.random(n) < 0.1, 27] = 0
    counts = rng.integers(1, 9, (n, 2)).astype(np.uint32)
    return f, counts


def test_pair_function_matches_float64_restatement(ph):
    """every pair of 20 000, none left out: each output of ph_pair_impulse within the running-error bound of its float32 evaluation plus one
    quantum of the float64 restatement of S27.5; no pair may sit on a branch (contact, bounce) closer than that bound"""
    rng = np.random.default_rng(23)
    n = 20000
    f, counts = random_pairs(rng, n)
    prm = np.array([1 / 60, 0.6, 0.5, 0.2, 0.005, 2.0], np.float32)
    out, hit = np.zeros((n, 14), np.float32), np.zeros(n, np.uint32)
    ph.ph_host_pairs(p(f), p(counts), n, p(prm), p(out), p(hit))
    E = ref.Err
    col = lambda a, b: [E(f[:, k]) for k in range(a, b)]  # noqa: E731
    q = dict(xa=col(0, 3), ra=E(f[:, 3]), xb=col(4, 7), rb=E(f[:, 7]), va=col(8, 11), wa=col(11, 14), vb=col(14, 17), wb=col(17, 20), v0a=col(20, 23), v0b=col(23, 26),
             ima=E(f[:, 26]), imb=E(f[:, 27]), na=E(counts[:, 0]), nb=E(counts[:, 1]))
    names = ("h", "e", "mu", "beta", "slop", "threshold")
    r = ref.pair_impulse(q, {k: float(prm[i]) for i, k in enumerate(names)})
    gap, approach = r["decide"]
    assert not (np.abs(ref.val(gap)) <= ref.err(gap)).any(), "a pair sits on the contact test"
    assert not ((np.abs(ref.val(approach)) <= ref.err(approach)) & r["hit"]).any(), "a pair sits on the bounce threshold"
    assert np.array_equal(hit != 0, r["hit"])
    worst = 0.0
    cols = [x for name in ("dva", "dwa", "dvb", "dwb") for x in r[name]] + [r["lam"], r["jt"]]
    for k, c in enumerate(cols):
        h = r["hit"]
        diff = np.abs(out[h, k].astype(np.float64) - ref.val(c)[h])
        bound = ref.err(c)[h] + ref.QUANTUM
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all(), (k, float((diff / bound).max()))
    print(f"pair function: largest error = {worst:.3f} of the bound over {int(r['hit'].sum())} contacts of {n} pairs")
    assert int(r["hit"].sum()) > n // 2 and int((~r["hit"]).sum()) > n // 20


def test_integrator_matches_float64_restatement(ph):
    rng = np.random.default_rng(24)
    n = 5000
    st = np.zeros((n, 14), np.float32)
    st[:, 0:3], st[:, 3] = rng.uniform(-50, 50, (n, 3)), 0.1
    q = rng.normal(size=(n, 4))
    st[:, 4:8] = q / np.linalg.norm(q, axis=1, keepdims=True)
    st[:, 8:11], st[:, 11:14] = rng.normal(size=(n, 3)) * 5, rng.normal(size=(n, 3)) * 20
    before = st.copy()
    ok = np.zeros(n, np.uint32)
    ph.ph_host_integrate(p(st), n, np.float32(1 / 60), p(ok))
    assert ok.all()
    E = ref.Err
    x, rot = ref.integrate([E(before[:, k]) for k in range(3)], [E(before[:, k]) for k in range(4, 8)], [E(before[:, k]) for k in range(8, 11)],
                           [E(before[:, k]) for k in range(11, 14)], float(np.float32(1 / 60)))
    worst = 0.0
    for k, c in enumerate(x + rot):
        diff = np.abs(st[:, k if k < 3 else k + 1].astype(np.float64) - ref.val(c))
        worst = max(worst, float((diff / ref.err(c)).max()))
        assert (diff <= ref.err(c)).all()
    print(f"integrator: largest error = {worst:.3f} of the bound")
    assert np.allclose(np.linalg.norm(st[:, 4:8].astype(np.float64), axis=1), 1.0, atol=4 * U)


def test_acceleration_matches_float64_restatement(ph):
    sph, bodies, *_ = cluster(5, 64)
    bodies["Flags"][3] |= DISABLED
    att = np.array([(0, 0, 30.0, ALL), (1, 1, 10.0, ALL), (2, 0, 5.0, 7), (9, 1, 2.0, 9)], ATTRACTOR)
    out = np.zeros((64, 3), np.float32)
    ph.ph_host_acceleration(p(sph), p(bodies), 64, p(att), 4, p(out))
    want = ref.acceleration(sph, bodies, att)
    scale = np.abs(want).max(1, keepdims=True) + 1e-3
    assert np.abs(out - want).max() <= 64 * U * float((np.abs(want).max() + 1))
    assert (np.abs(out - want) <= 64 * U * (scale + np.abs(want).max())).all()
    assert not out[bodies["InvMass"] == 0].any() and not out[3].any()


def test_quantise_and_apply(ph):
    x = np.array([0.0, 1.0, -1.0, 2.0 ** -25, 3 * 2.0 ** -25, 32768.0, 32769.0, -1e9, np.inf, np.nan, 1.2345678], np.float32)
    q, c = np.zeros(len(x), np.int64), np.zeros(len(x), np.uint32)
    ph.ph_host_quantize(p(x), len(x), p(q), p(c))
    assert q.tolist()[:10] == [0, 2 ** 24, -2 ** 24, 0, 2, 2 ** 39, 2 ** 39, -2 ** 39, 2 ** 39, 0]  # ties to even; the clamp
    assert c.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0]
    assert abs(q[10] * 2.0 ** -24 - float(x[10])) <= 2.0 ** -25
    # 2^20 contributions at the clamp stay far inside 64 bits
    assert 2 ** 20 * 2 ** 39 < 2 ** 62
    v = np.array([-0.0, 1.0, 1.0], np.float32)
    acc = np.array([0, 0, 2 ** 24], np.int64)
    out = np.zeros(3, np.float32)
    ph.ph_host_apply(p(v), p(acc), 3, p(out))
    assert bits(out).tolist() == bits(np.array([-0.0, 1.0, 2.0], np.float32)).tolist()


# ------------------------------------------------------------------------------------------------ known answers
def two(ph, xa, xb, va, vb, ima=1.0, imb=1.0, ra=0.5, rb=0.5, flags=(0, 0), wa=(0, 0, 0), wb=(0, 0, 0), steps=1, **kw):
    sph = np.array([[*xa, ra], [*xb, rb]], np.float32)
    bodies = np.zeros(2, BODY)
    bodies["InvMass"], bodies["Flags"] = (ima, imb), flags
    h = Host(ph, sph, bodies, np.array([va, vb], np.float32), np.array([wa, wb], np.float32), None, settings(**kw))
    rep = [h.step(1 / 60) for _ in range(steps)][-1]
    st = h.state()
    h.close()
    return st, rep


def test_head_on_equal_masses(ph):
    v = 3.0
    (sph, rot, lin, ang, flags, _), rep = two(ph, (0, 0, 0), (0.99, 0, 0), (v, 0, 0), (0, 0, 0), iterations=1, mu=0.0, beta=0.0)
    assert rep[0] == 1
    assert np.allclose(lin[:, 0], [(1 - 0.6) / 2 * v, (1 + 0.6) / 2 * v], atol=8 * U * v + 2.0 ** -24) and not lin[:, 1:].any() and not ang.any()


def test_against_an_immovable_body(ph):
    v = 4.0
    (sph, rot, lin, *_), rep = two(ph, (0, 0, 0), (0.99, 0, 0), (v, 0, 0), (0, 0, 0), imb=0.0, iterations=1, mu=0.0, beta=0.0)
    assert abs(lin[0, 0] + 0.6 * v) <= 8 * U * v + 2.0 ** -24 and not lin[1].any()
    assert sph[1].tolist() == [np.float32(0.99), 0, 0, 0.5]


def test_below_the_threshold_there_is_no_bounce(ph):
    v = 0.1
    (_, _, lin, *_), _ = two(ph, (0, 0, 0), (0.99, 0, 0), (v, 0, 0), (0, 0, 0), iterations=1, mu=0.0, beta=0.0)
    assert np.allclose(lin[:, 0], [v / 2, v / 2], atol=8 * U + 2.0 ** -24)


def test_glancing_contact_spins_both_and_friction_is_bounded(ph):
    (_, _, lin, ang, *_), _ = two(ph, (0, 0, 0), (0.7, 0.7, 0), (3.0, 0, 0), (0, 0, 0), iterations=1, beta=0.0)
    assert ang[0, 2] != 0 and ang[1, 2] != 0 and not ang[:, :2].any()
    assert ang[0, 2] * ang[1, 2] > 0  # the two surfaces drag each other the same way round
    f = np.zeros((1, 28), np.float32)
    f[0, 0:4], f[0, 4:8], f[0, 8:11], f[0, 20:23], f[0, 26:28] = (0, 0, 0, 0.5), (0.7, 0.7, 0, 0.5), (3, 0, 0), (3, 0, 0), (1, 1)
    out, hit = np.zeros((1, 14), np.float32), np.zeros(1, np.uint32)
    for mu in (0.05, 0.5, 50.0):
        ph.ph_host_pairs(p(f), p(np.ones((1, 2), np.uint32)), 1, p(np.array([1 / 60, 0.6, mu, 0, 0.005, 2.0], np.float32)), p(out), p(hit))
        lam, jt = float(out[0, 12]), float(out[0, 13])
        assert hit[0] and lam > 0 and 0 < jt <= np.float32(mu) * np.float32(lam)
    assert jt < 50.0 * lam  # with a huge coefficient the contact sticks: the impulse that stops the sliding, not mu lambda


def test_coincident_centres_separate_along_y(ph):
    (_, _, lin, *_), rep = two(ph, (1, 2, 3), (1, 2, 3), (0, 0, 0), (0, 0, 0))
    assert rep[0] == 1 and lin[0, 1] < 0 < lin[1, 1] and not lin[:, [0, 2]].any()


def test_disabled_partner_and_two_immovable_bodies(ph):
    (sph, _, lin, _, flags, _), rep = two(ph, (0, 0, 0), (0.9, 0, 0), (3, 0, 0), (0, 0, 0), flags=(0, DISABLED))
    assert rep[0] == 0 and lin.tolist() == [[3, 0, 0], [0, 0, 0]] and sph[1, 0] == np.float32(0.9)
    (sph, _, lin, *_), rep = two(ph, (0, 0, 0), (0.9, 0, 0), (3, 0, 0), (-1, 0, 0), ima=0.0, imb=0.0)
    assert lin.tolist() == [[3, 0, 0], [-1, 0, 0]]  # immovable bodies keep their velocities and move with them
    assert np.allclose(sph[:, 0], [3 / 60, 0.9 - 1 / 60], atol=4 * U)


# ------------------------------------------------------------------------------------------------ the handler rule
@pytest.mark.parametrize("flagged", ["none", "all", "more than the cap"])
def test_large_flags_do_not_change_the_pairs(ph, flagged):
    """S27.4: every pair has exactly one handler whoever is LARGE, and the state does not depend on the flags"""
    n = 64 if flagged != "more than the cap" else 90
    sph, bodies, lin, ang, rot = cluster(7, n, fill=0.45)
    sph[::7, 3] = sph[0, 3]  # ties of the radius
    plain = Host(ph, sph, bodies, lin, ang, rot)
    marked = bodies.copy()
    if flagged != "none":
        marked["Flags"] |= LARGE
    other = Host(ph, sph, marked, lin, ang, rot)
    contacts = 0
    for _ in range(10):
        contacts += int(plain.step(1 / 60)[0])
        other.step(1 / 60)
    a, b = plain.state(), other.state()
    assert contacts > 5 * n and a[5] == 0 and b[5] == 0
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(bits(x), bits(y))
    plain.close(); other.close()


# ------------------------------------------------------------------------------------------------ closed forms
def test_spring_follows_the_closed_form(ph):
    """one period (T = 3 s, 180 steps of 1/60): the header's distance from A cos(wt - phi) is the float64 restatement's (the truncation error
    of semi-implicit Euler, about A w h / 2 = 1.7 % of A) up to float32 rounding: 180 steps x 8 operations x u x the largest magnitude, and a
    margin of 1.05 on the truncation error for the rounding of h itself"""
    A, T, phi, y0 = 0.5, 3.0, 0.7, 0.5
    w = 2 * math.pi / T
    sph = np.array([[0, y0 + A * math.cos(-phi), 0, 0.075]], np.float32)
    bodies = density_bodies([0.075], SPRING)
    bodies["SpringY0"], bodies["SpringOmega2"] = y0, w * w
    lin = np.array([[0, -A * w * math.sin(-phi), 0]], np.float32)
    h = Host(ph, sph, bodies, lin)
    r64 = ref.State64(sph, bodies, lin)
    e32 = e64 = 0.0
    for k in range(1, 181):
        h.step(1 / 60)
        r64.step(settings(), NO_ATTRACTORS, float(np.float32(1 / 60)))
        want = y0 + A * math.cos(w * k * float(np.float32(1 / 60)) - phi)
        e32, e64 = max(e32, abs(float(h.state()[0][0, 1]) - want)), max(e64, abs(r64.sph[0, 1] - want))
    h.close()
    print(f"spring: float32 {e32:.3e}, float64 {e64:.3e}")
    assert 1e-4 < e64 < 0.03 * A and e32 <= 1.05 * e64 + 180 * 8 * U * (y0 + A)


def test_moon_orbit_keeps_its_radius(ph):
    """one orbit (10 s, 600 steps): |r - R| against the float64 restatement's, with the same allowance as the spring (600 steps, magnitudes <= R w^2 h ... R)"""
    R, T = 4.0, 10.0
    v = 2 * math.pi * R / T
    sph = np.array([[0, 4, 0, 1.0], [-R, 4, 0, 0.25]], np.float32)
    bodies = density_bodies([1.0, 0.25])
    lin = np.array([[0, 0, 0], [0, 0, v]], np.float32)
    att = np.array([(0, 0, v * v * R, 1)], ATTRACTOR)
    h = Host(ph, sph, bodies, lin, attractors=att)
    r64 = ref.State64(sph, bodies, lin)
    e32 = e64 = 0.0
    for _ in range(600):
        h.step(1 / 60)
        r64.step(settings(), att, float(np.float32(1 / 60)))
        s = h.state()[0].astype(np.float64)
        e32 = max(e32, abs(np.linalg.norm(s[1, :3] - s[0, :3]) - R))
        e64 = max(e64, abs(np.linalg.norm(r64.sph[1, :3] - r64.sph[0, :3]) - R))
    assert np.array_equal(h.state()[0][0], sph[0])  # the Earth is not attracted by the Moon-only attractor
    h.close()
    print(f"orbit: float32 {e32:.3e}, float64 {e64:.3e}")
    assert e64 < 0.05 * R and e32 <= 1.05 * e64 + 600 * 8 * U * R


# ------------------------------------------------------------------------------------------------ behaviour
def test_dropped_body_comes_to_rest(ph):
    """a small sphere falls 0.3 onto the immovable Star under the constant 10 m/s^2 pull.  At rest the pull adds g h to the approach speed
    each step (0.167 < BounceThreshold) and the bias takes out beta (pen - slop) of the penetration, so pen settles at slop + g h^2 / beta;
    the bound allows one more step's fall.  600 steps: the float64 restatement satisfies both."""
    g, hs, beta, slop = 10.0, float(np.float32(1 / 60)), 0.2, 0.005
    sph = np.array([[0, -50.1, 0, 50.0], [0.3, 0.3, 0.1, 0.075]], np.float32)
    bodies = density_bodies([50.0, 0.075], (LARGE, 0))
    bodies["InvMass"][0] = 0
    att = np.array([(0, 1, g, ALL)], ATTRACTOR)
    h = Host(ph, sph, bodies, attractors=att)
    r64 = ref.State64(sph, bodies)
    for _ in range(600):
        rep = h.step(1 / 60)
        r64.step(settings(), att, hs)
    s, _, lin, *_ = h.state()
    bound = slop + 2 * g * hs * hs / beta
    for name, x, v in (("float64", r64.sph, r64.vel), ("float32", s.astype(np.float64), lin.astype(np.float64))):
        pen = 50.075 - np.linalg.norm(x[1, :3] - x[0, :3])
        print(f"{name}: penetration {pen:.5f} (bound {bound:.5f}), speed {np.linalg.norm(v[1]):.4f}")
        assert 0 < pen < bound and np.linalg.norm(v[1]) < 0.2
    assert rep[0] == 1
    h.close()


def gas(seed, n):
    """n spheres on a jittered lattice, none touching, flying towards the middle"""
    rng = np.random.default_rng(seed)
    k = int(math.ceil(n ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    r = rng.uniform(0.08, 0.16, n)
    x = grid * 0.4 + rng.uniform(-0.03, 0.03, (n, 3))
    sph = np.concatenate([x, r[:, None]], 1).astype(np.float32)
    centre = x.mean(0)
    lin = (-(x - centre) * 1.5 + rng.normal(size=(n, 3)) * 0.5).astype(np.float32)
    return sph, density_bodies(r), lin, (rng.normal(size=(n, 3)) * 2).astype(np.float32)


def test_gas_does_not_gain_energy_and_keeps_its_momentum(ph):
    """200 bodies, no forces, beta = 0, 100 steps.  Energy: never above the start by more than the float64 restatement of the same steps
    gains (nothing: its energy only falls) plus float32 rounding of the sum.  Momentum: a pair's two shares are rounded to the quantum
    separately (m q / 2 each, per component) and every apply rounds a velocity once (u |v| m): the drift is bounded by their sum over
    the contacts and applies that happened."""
    n, steps, it = 200, 100, 4
    sph, bodies, lin, ang = gas(31, n)
    s = settings(beta=0.0)
    h = Host(ph, sph, bodies, lin, ang, s=s)
    r64 = ref.State64(sph, bodies, lin, ang)
    m = 1.0 / bodies["InvMass"].astype(np.float64)

    def energy(st):
        v, w = st[2].astype(np.float64), st[3].astype(np.float64)
        return 0.5 * (m * (v ** 2).sum(1)).sum() + 0.5 * (0.4 * m * sph[:, 3].astype(np.float64) ** 2 * (w ** 2).sum(1)).sum()

    e0, p0 = energy(h.state()), (m[:, None] * lin.astype(np.float64)).sum(0)
    assert ref.State64(sph, bodies).pairs()[0].size == 0
    top32 = top64 = 0.0
    contacts, vmax = 0, float(np.abs(lin).max())
    for _ in range(steps):
        contacts += int(h.step(1 / 60)[0])
        r64.step(s, NO_ATTRACTORS, float(np.float32(1 / 60)))
        top32, top64 = max(top32, energy(h.state())), max(top64, r64.kinetic_energy())
    st = h.state()
    print(f"gas: {contacts} contacts, energy {e0:.6f} -> {energy(st):.6f} (float64 {r64.kinetic_energy():.6f}), highest {top32 / e0:.7f} / {top64 / e0:.7f} of the start")
    assert contacts > n
    assert top32 <= max(top64, e0) * (1 + 16 * U)
    drift = np.abs((m[:, None] * st[2].astype(np.float64)).sum(0) - p0).max()
    bound = contacts * it * m.max() * ref.QUANTUM + contacts * 2 * it * U * 2 * vmax * m.max()
    print(f"gas: momentum drift {drift:.3e}, bound {bound:.3e}")
    assert drift <= bound
    h.close()


# ------------------------------------------------------------------------------------------------ robustness
def test_non_finite_result_freezes_the_body(ph):
    """a position that overflows, and a spin whose quaternion step overflows: the body keeps the state the step started from, is DISABLED from
    then on and is counted once"""
    sph = np.array([[0, 0, 0, 0.5], [5, 0, 0, 0.5], [9, 0, 0, 0.5]], np.float32)
    lin = np.array([[3e38, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    ang = np.array([[0, 0, 0], [0, 0, 0], [3e38, 0, 0]], np.float32)
    h = Host(ph, sph, density_bodies([0.5] * 3), lin, ang)
    rep = h.step(2.0, 1)
    s, rot, v, w, flags, _ = h.state()
    assert rep[2] == 2 and flags.tolist() == [DISABLED, 0, DISABLED]
    assert s[0].tolist() == [0, 0, 0, 0.5] and v[0].tolist() == [np.float32(3e38), 0, 0] and s[1, 0] == 7
    assert s[2].tolist() == [9, 0, 0, 0.5] and rot[2].tolist() == [0, 0, 0, 1] and w[2, 0] == np.float32(3e38)
    rep = h.step(2.0, 1)
    assert rep[2] == 0 and np.isfinite(h.state()[0]).all() and h.state()[0][0].tolist() == [0, 0, 0, 0.5]
    h.close()


def test_clamp_sets_the_sticky_bit(ph):
    (_, _, lin, *_), rep = two(ph, (0, 0, 0), (0.99, 0, 0), (1e6, 0, 0), (0, 0, 0), iterations=1, mu=0.0, beta=0.0)
    assert rep[1] == 1 and lin[1, 0] == 32768.0 and lin[0, 0] == np.float32(1e6) - 32768.0
    (_, _, lin, *_), rep = two(ph, (0, 0, 0), (0.99, 0, 0), (100, 0, 0), (0, 0, 0))
    assert rep[1] == 0


def test_null_context_is_refused(dxrs):
    lib = dxrs.load_hip().lib
    assert lib.pt_physics_step(None, 1 / 60, 1, None) == 1 and lib.pt_physics_create(None, None, None, None, None, None, 0, None) == 1
    assert lib.pt_physics_download(None, None, None, None, None) == 1 and lib.pt_physics_set_attractors(None, None, 0) == 1
    lib.pt_physics_destroy(None)
    t = dxrs.types
    assert C.sizeof(t.PtPhysicsSettings) == 32 and C.sizeof(t.PtPhysicsReport) == 16 and t.PHYSICS_BODY_DTYPE.itemsize == 16 and t.PHYSICS_ATTRACTOR_DTYPE.itemsize == 16
    assert t.PHYSICS_BODY_DTYPE == BODY and t.PHYSICS_ATTRACTOR_DTYPE == ATTRACTOR


def test_sanitizer_program(tmp_path):
    """tests/hostshim/physics_sanitize.cpp: the header's paths under AddressSanitizer + UBSan as a stand-alone program run as a child process"""
    import __graft_entry__ as g

    exe = g.build_physics_sanitizer(str(tmp_path))
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "physics_sanitize ok" in res.stdout, res.stdout + res.stderr


# ------------------------------------------------------------------------------------------------ GPU
def run_both(renderer, ph, scene, steps, s=None, attractors=NO_ATTRACTORS, substeps=1, dt=1 / 60, gpu_steps=None):
    """the same steps on the device and through the host header -> (device state, host state, device reports, host reports)"""
    sph, bodies, lin, ang, rot = scene
    s = s or settings()
    h = Host(ph, sph, bodies, lin, ang, rot, s, attractors)
    renderer.physics_create(sph, bodies, lin, ang, rot, s)
    renderer.physics_set_attractors(attractors)
    greps, hreps = [], []
    for _ in range(steps):
        hreps.append(h.step(dt, substeps).tolist())
    for dt_g, sub_g in (gpu_steps or [(dt, substeps)] * steps):
        r = renderer.physics_step(dt_g, sub_g)
        greps.append([r.Contacts, r.Clamped, r.Frozen, r.Steps])
    dev, host = renderer.physics_download(), h.state()
    h.close()
    return dev, host, greps, hreps


def assert_same(dev, host, greps=None, hreps=None):
    for name, a, b in zip(("spheres", "rotations", "lin_vel", "ang_vel"), dev, host):
        bad = np.nonzero((bits(a) != bits(b)).any(1))[0] if len(a) else []
        assert len(bad) == 0, f"{name}: {len(bad)} bodies differ, first {bad[:5]}: {a[bad[:2]]} != {b[bad[:2]]}"
    assert np.isfinite(dev[0]).all() and np.isfinite(dev[1]).all()
    if greps is not None:
        assert greps == hreps


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1024, 1025])
def test_gpu_matches_host_over_sizes(renderer, ph, n):
    dev, host, g, h = run_both(renderer, ph, cluster(100 + n, n), 8, attractors=np.array([(0, 1, 2.0, ALL)], ATTRACTOR) if n > 1 else NO_ATTRACTORS)
    assert_same(dev, host, g, h)
    if n >= 64:
        assert sum(x[0] for x in g) > n


@pytest.mark.gpu
def test_gpu_matches_host_on_the_global_memory_tree(renderer, ph):
    """32 769 bodies: the first size on the 32-bit stack and the tree in global memory"""
    dev, host, g, h = run_both(renderer, ph, cluster(9, 32769), 3)
    assert_same(dev, host, g, h)
    assert g[0][0] > 32769


@pytest.mark.gpu
def test_gpu_degenerate_layouts(renderer, ph):
    sph, bodies, lin, ang, rot = cluster(3, 40)
    sph[:, :3] = (1.0, 2.0, 3.0)  # all centres identical
    dev, host, g, h = run_both(renderer, ph, (sph, bodies, lin * 0, ang, rot), 8)
    assert_same(dev, host, g, h)
    assert g[0][0] == 40 * 39 // 2
    n = 100  # a collinear chain in contact
    sph = np.zeros((n, 4), np.float32)
    sph[:, 0], sph[:, 3] = np.arange(n) * 0.19, 0.1
    lin = np.zeros((n, 3), np.float32)
    lin[0, 0] = 5.0
    dev, host, g, h = run_both(renderer, ph, (sph, density_bodies(sph[:, 3]), lin, None, None), 8)
    assert_same(dev, host, g, h)
    assert g[0][0] == n - 1 and dev[2][n // 2, 0] != 0


@pytest.mark.gpu
def test_gpu_large_bodies(renderer, ph):
    """one LARGE sphere touched by every other body (every contact adds to the same accumulators), then 65 LARGE bodies: one past the cap"""
    rng = np.random.default_rng(12)
    n = 3000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sph = np.concatenate([d * 5.02, np.full((n, 1), 0.05)], 1).astype(np.float32)
    sph = np.concatenate([np.array([[0, 0, 0, 5.0]], np.float32), sph])
    bodies = density_bodies(sph[:, 3])
    bodies["Flags"][0] = LARGE
    lin = np.concatenate([np.zeros((1, 3)), -d * 2.0 + rng.normal(size=(n, 3)) * 0.3]).astype(np.float32)
    att = np.array([(0, 1, 10.0, ALL)], ATTRACTOR)
    dev, host, g, h = run_both(renderer, ph, (sph, bodies, lin, None, None), 6, attractors=att)
    assert_same(dev, host, g, h)
    assert g[0][0] >= n and dev[2][0].any()
    plain = bodies.copy()
    plain["Flags"][0] = 0  # ... and the same with the big sphere walking the tree
    dev2, host2, *_ = run_both(renderer, ph, (sph, plain, lin, None, None), 6, attractors=att)
    assert_same(dev2, host2)
    assert_same(dev2, dev)

    sph, bodies, lin, ang, rot = cluster(13, 400, fill=0.4)
    big = np.arange(65) * 6
    sph[big, 3] = 0.3
    bodies["Flags"][big] |= LARGE
    dev, host, g, h = run_both(renderer, ph, (sph, bodies, lin, ang, rot), 8)
    assert_same(dev, host, g, h)
    assert host[5] == 0 and g[0][0] > 400


@pytest.mark.gpu
def test_gpu_attractors_of_both_kinds(renderer, ph):
    sph, bodies, lin, ang, rot = cluster(14, 300, fill=0.2)
    att = np.array([(0, 0, 3.0, ALL), (1, 1, 10.0, ALL), (2, 0, 5.0, 7), (2, 1, 1.0, 2)], ATTRACTOR)
    dev, host, g, h = run_both(renderer, ph, (sph, bodies, lin, ang, rot), 8, attractors=att)
    assert_same(dev, host, g, h)
    still = Host(ph, sph, bodies, lin, ang, rot)
    for _ in range(8):
        still.step(1 / 60)
    assert not np.array_equal(bits(still.state()[2]), bits(host[2]))
    still.close()


@pytest.mark.gpu
def test_gpu_substeps_equal_single_steps(renderer, ph):
    scene = cluster(15, 200)
    dt = 1 / 60
    h4 = float(np.float32(dt) / np.float32(4))
    dev, host, *_ = run_both(renderer, ph, scene, 2, substeps=4)
    assert_same(dev, host)
    dev1, host1, g, _ = run_both(renderer, ph, scene, 8, dt=h4)
    assert_same(dev1, host1)
    assert_same(dev1, dev)
    assert g[-1][3] == 8


@pytest.mark.gpu
def test_gpu_tree_rebuilt_or_refitted(renderer, ph):
    """the same 300-body cluster, 20 steps, with RebuildInterval 0, 1 and 3: one state, bit for bit (the state after a step does not depend on the tree)"""
    scene = cluster(16, 300, speed=3.0)
    states = []
    for rebuild in (0, 1, 3):
        dev, host, g, h = run_both(renderer, ph, scene, 20, s=settings(rebuild=rebuild))
        assert_same(dev, host, g, h)
        states.append(dev)
    assert_same(states[1], states[0])
    assert_same(states[2], states[0])
    assert np.abs(states[0][0][:, :3] - scene[0][:, :3]).max() > 0.5  # the bodies have travelled: the refitted tree is far from the built one


@pytest.mark.gpu
def test_gpu_step_behind_frames_in_flight(dxrs, host, ph):
    """steps queued without waiting behind frames in flight on three lanes: the pass shares only the context's stream with them"""
    import torch

    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, hgt = 320, 180
    scene = cluster(17, 500)
    r = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        r.set_scene(spheres, mats, sd)
        r.set_camera(host.camera(w, hgt)); r.set_constants(dxrs.types.graphics_settings(w, hgt, bounces=8, spp=1))
        plain, _ = r.render()
        outs = [torch.zeros((hgt, w, 4), device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        r.physics_create(*scene, settings())
        hh = Host(ph, *scene)
        for k in range(6):
            r.render_device(outs[k % 3].data_ptr())
            r.physics_step(1 / 60, 1, report=False)
            hh.step(1 / 60)
        dev = r.physics_download()
        r.synchronize()
        assert_same(dev, hh.state())
        hh.close()
        for o in outs:
            assert np.array_equal(o.cpu().numpy().view(np.uint32), plain.view(np.uint32))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_whole_loop_matches_oracle(dxrs, host, oracle, ph):
    """step -> download -> pt_update_spheres -> pt_update_rotations -> pt_render: every frame equals the oracle's image of the downloaded
    positions bit for bit, as test_animated_scene_refit_matches_oracle checks for the closed-form motion"""
    spheres0, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    n = len(spheres0)
    w, hgt, rect = 640, 360, (200, 140, 240, 120)
    sph = np.stack([spheres0[k] for k in ("cx", "cy", "cz", "r")], 1).astype(np.float32)
    bodies = density_bodies(sph[:, 3])
    bodies["InvMass"][-1] = 0  # the Star
    bodies["Flags"][-1] = LARGE
    att = np.array([(n - 1, 1, 10.0, ALL)], ATTRACTOR)
    r = dxrs.Renderer(device=0)
    try:
        r.set_scene(spheres0, materials, sd)
        tex = host.demo_textures(0, 0.0)  # Alien-Metal, Moon and Earth are textured: their rotations show
        r.set_textures(tex)
        ang = np.zeros((n, 3), np.float32)
        ang[:, 1] = 2.0
        r.physics_create(sph, bodies, None, ang, tex.rotations, settings())
        r.physics_set_attractors(att)
        hh = Host(ph, sph, bodies, None, ang, tex.rotations, attractors=att)
        contacts = 0
        for k in range(4):
            rep = r.physics_step(0.25, 15)  # a quarter of a second in steps of 1/60
            hh.step(0.25, 15)
            contacts += rep.Contacts
            s, rot, _, _ = r.physics_download()
            moved = spheres0.copy()
            for i, name in enumerate(("cx", "cy", "cz", "r")):
                moved[name] = s[:, i]
            assert np.array_equal(moved["r"], spheres0["r"])
            r.update_spheres(moved)
            r.update_rotations(rot)
            tex.rotations[:] = rot
            gs = dxrs.types.graphics_settings(w, hgt, frame_index=k, bounces=8, spp=1)
            r.set_camera(host.camera(w, hgt, jitter_index=k)); r.set_constants(gs)
            img, _ = r.render(rect)
            want, _ = oracle.render(moved, materials, sd, host.camera(w, hgt, jitter_index=k), gs, rect=rect, threads=8, textures=tex)
            assert np.array_equal(img.view(np.uint32)[..., :3], want.view(np.uint32)[..., :3]), f"frame {k}"
        assert_same(r.physics_download(), hh.state())
        assert contacts > 100 and np.abs(s[:, 1] - sph[:, 1]).max() > 0.3  # the small spheres have fallen onto the ground
        assert np.abs(rot - host.demo_textures(0, 0.0).rotations).max() > 0.5  # ... and everything has turned
        hh.close()
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_argument_errors_leave_the_state_untouched(renderer, dxrs, ph):
    scene = cluster(18, 50)
    sph, bodies, lin, ang, rot = scene
    renderer.physics_destroy()
    with pytest.raises(dxrs.PtError, match="pt_physics_create has not been called"):
        renderer.physics_step(1 / 60)
    renderer.physics_create(*scene, settings())
    renderer.physics_step(1 / 60)
    before = renderer.physics_download()
    for dt, sub in ((0.0, 1), (-1.0, 1), (float("nan"), 1), (float("inf"), 1), (1 / 60, 0)):
        with pytest.raises(dxrs.PtError, match="pt_physics_step"):
            renderer.physics_step(dt, sub)
    for bad in ([(50, 0, 1.0, ALL)], [(0, 2, 1.0, ALL)], [(0, 0, float("nan"), ALL)], [(0, 0, 1.0, 50)], [(0, 0, 1.0, ALL)] * 5):
        with pytest.raises(dxrs.PtError, match="pt_physics_set_attractors"):
            renderer.physics_set_attractors(bad)
    nan_sph, zero_r, bad_body, bad_flags = sph.copy(), sph.copy(), bodies.copy(), bodies.copy()
    nan_sph[3, 1], zero_r[4, 3], bad_body["InvMass"][5], bad_flags["Flags"][6] = np.nan, 0.0, -1.0, 8
    bad_lin = lin.copy()
    bad_lin[7, 2] = np.inf
    for args in ((nan_sph, bodies, lin), (zero_r, bodies, lin), (sph, bad_body, lin), (sph, bad_flags, lin), (sph, bodies, bad_lin)):
        with pytest.raises(dxrs.PtError, match="pt_physics_create"):
            renderer.physics_create(*args, ang, rot, settings())
    for s in (settings(iterations=65), settings(e=1.5), settings(mu=-1.0), settings(beta=float("nan")), settings(slop=-1.0)):
        with pytest.raises(dxrs.PtError, match="settings"):
            renderer.physics_create(*scene, s)
    assert_same(renderer.physics_download(), before)  # every refused call kept the state
    assert renderer.physics_step(1 / 60).Steps == 2
    renderer.physics_destroy()
    renderer.physics_destroy()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, host, ph, tmp_path):
    """dxrs::Physics and MyScene::TickPhysics (host/Physics.hpp) from C++, against pt_api.h alone: the demo scene with Star gravity ticked
    as MyScene::Tick does it; the bodies, velocities and attractors the program built, stepped by the host header, give the state it wrote"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_physics")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_physics.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    outp = str(tmp_path / "physics.bin")
    ticks = 30
    res = subprocess.run([exe, str(ticks), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(outp, np.float32)
    n = int(raw[0])
    blocks = np.split(raw[1:], np.cumsum([n * 4, n * 4, n * 3, n * 3, 16, n * 4, n * 4, n * 4]))
    sph0, body_raw, lin0, ang0, att_raw, rot0, sph1, rot1 = blocks[:8]
    bodies = body_raw.view(np.uint32).reshape(n, 4).copy().view(BODY).reshape(n)
    att = att_raw.view(np.uint32).reshape(4, 4).copy().view(ATTRACTOR).reshape(4)
    att = att[att["Kind"] <= 1]
    spheres0 = host.scene(dxrs.host.SCENE_DEMO, seed=0)[0]
    assert n == len(spheres0) and np.array_equal(sph0.reshape(n, 4)[:, 0], spheres0["cx"])
    assert (bodies["Flags"] & SPRING).sum() > 400 and (bodies["Flags"] & LARGE).sum() >= 1 and len(att) == 2
    hh = Host(ph, sph0.reshape(n, 4), bodies, lin0.reshape(n, 3), ang0.reshape(n, 3), rot0.reshape(n, 4), settings(), att)
    for _ in range(ticks):
        hh.step(1 / 60)
    st = hh.state()
    hh.close()
    assert np.array_equal(bits(st[0]), bits(sph1.reshape(n, 4))) and np.array_equal(bits(st[1]), bits(rot1.reshape(n, 4)))
    assert "contacts" in res.stdout
