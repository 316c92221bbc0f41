"""Row N7 (DESIGN.md spec S13), CPU: the NRD modes split the direct-illumination estimate by lobe.  csrc/pt_light.h's
bsdf_eval_reflective_lobes, compiled as host C++ (tests/hostshim/denoiser_host.cpp), gives the two halves whose sum is
bsdf_eval_reflective bit for bit, and the halves' estimates sum to the estimate within rounding."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_denoiser_shim())
    lib.dn_lobes.restype = None
    lib.dn_lobes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p]
    return lib


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cases(rng, n, metallic=None):
    rows = np.zeros((n, 17), np.float32)
    rows[:, 0:3] = rng.uniform(0.0, 1.0, (n, 3))
    rows[:, 3] = rng.choice([0.0, 0.3, 1.0], n) if metallic is None else metallic
    rows[:, 4] = rng.uniform(0.02, 1.0, n)
    rows[:, 5] = rng.choice([1.0, 1.5, 2.4], n)
    rows[:, 6] = rng.choice([0.0, 0.5, 1.0], n)
    rows[:, 7] = 1.0
    N = unit(rng, n)
    V, L = unit(rng, n), unit(rng, n)
    V = np.where((V * N).sum(1, keepdims=True) < 0, -V, V)  # the viewer on the front side
    L = np.where((L * N).sum(1, keepdims=True) < 0, -L, L)  # the emitter above the surface (di_estimate's precondition)
    rows[:, 8:11], rows[:, 11:14], rows[:, 14:17] = N, V, L
    return rows


def run(shim, rows, le=(4.0, 2.0, 1.0), k=2.5):
    le = np.asarray(le, np.float32)
    out = np.empty((len(rows), 18), np.float32)
    shim.dn_lobes(rows.ctypes.data, len(rows), le.ctypes.data, k, out.ctypes.data)
    return [out[:, 3 * j: 3 * j + 3] for j in range(6)]


def test_halves_sum_to_the_reflective_bsdf(shim):
    f, fd, fs, est, ed, es = run(shim, cases(np.random.default_rng(7), 4000))
    assert np.array_equal((fd + fs).view(np.uint32), f.view(np.uint32))  # the sum IS bsdf_eval_reflective's
    assert (fd >= 0).all() and (fs >= 0).all() and (f > 0).any()
    # the halves' estimates sum to the estimate within the rounding of two products and a sum
    tol = 4 * np.finfo(np.float32).eps * np.maximum(np.abs(est), 1e-30) + 1e-37
    assert (np.abs((ed + es).astype(np.float64) - est) <= tol).all()


def test_metal_has_no_diffuse_half(shim):
    f, fd, fs, est, ed, es = run(shim, cases(np.random.default_rng(8), 1000, metallic=1.0))
    assert (fd == 0).all() and (ed == 0).all()
    assert np.array_equal(fs.view(np.uint32), f.view(np.uint32)) and np.array_equal(es.view(np.uint32), est.view(np.uint32))
