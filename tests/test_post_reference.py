"""Row N3 against a second, independent reference, and its kernels past their first grid stride.

CPU: csrc/pt_post.h (compiled for the host by tests/hostshim) and oracle/pt_oracle.c were written side by side from one recollection of
DirectXTK's ToneMap.fx, so their bit parity (tests/test_post.py) cannot see a shared misreading.  Here both are held against
tests/post_reference.py: float64, constants from SMPTE ST 2084 and from the CIE chromaticities of BT.709 / P3-D65 / BT.2020, with a per-sample
allowance delta derived by forward error propagation (its docstring).  A code may differ from the un-rounded float64 value by 0.5 + delta,
and delta <= 0.05 code is asserted for every sample, so a code that is off by one fails unless the float64 value lies within 0.05 of a
rounding boundary.

Recorded on the host build (header and oracle give the same figures: they are bit-identical), 2^20 pixels per setting:
  matrices    max |entry - derived|: 709->2020 1.115e-06, P3-D65->2020 1.194e-05, 709->P3-D65 3.869e-08 (tolerance 5e-5);
              max |row sum - 1|: 1.814e-06, 5.438e-07, 4.470e-08 (tolerance 2e-6)
  codes       largest (|code - value| - 0.5) / delta over the stops {0, -2, 1.5}:
                Linear  None / Saturate 0.234, 0.210, 0.417; Reinhard 0.295, 0.304, 0.264; ACES fit 0.135, 0.228, 0.168
                SRGB    None / Saturate 0.058, 0.284, 0.324; Reinhard 0.282, 0.326, 0.273; ACES fit 0.238, 0.182, 0.159
                        (the excess over 0.5 is at most 2.661e-05 code, the largest delta 1.221e-04 code)
              and over the nits {200, 80, 10000}:
                ST 2084 709->2020 0.462, 0.425, 0.516; P3-D65->2020 0.481, 0.508, 0.508; 709->P3-D65 0.489, 0.448, 0.466
                        (the excess at most 8.997e-03 code, the largest delta 1.949e-02 code, the largest condition number 1.269)
  pow_spec    largest relative error, and the largest error / bound: 1/2.2 on [1e-6, 1] 6.556e-07 (0.771), 0.1593017578 on [1e-12, 1e4]
              4.225e-07 (0.769), 78.84375 on [0.8359375, 1] 3.444e-06 (0.614)
  running mean  after N = 4096 frames: 0.0188 of the bound (N/2 + 8) 2^-24 M for M = 1, 0.0120 for M = 100

GPU: `tonemap_kernel` and `accumulate_kernel` are grid-stride loops whose launchers cap the grid at 8192 x 256 = 2,097,152 threads.  They run
here at the block edge, at exactly one stride, one past it and on a third trip with a ragged tail, bit-exact against the host-compiled header,
between guard words that must stay untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import post_reference as ref
from test_post import all_params, hdr_samples, unpack8

HERE = os.path.dirname(os.path.abspath(__file__))
F32P = C.POINTER(C.c_float)
SWEEP = 1 << 20
DELTA_LIMIT = 0.05  # code
STRIDE = 8192 * 256


def label(p):
    if p.TransferFunction == ref.TF_ST2084:
        return f"ST2084 {('709->2020', 'P3D65->2020', '709->P3D65')[p.ColorRotation]} {p.PaperWhiteNits:g} nits"
    return f"{('None', 'Saturate', 'Reinhard', 'ACESFilmic')[p.Operator]} {('Linear', 'SRGB')[p.TransferFunction]} x{p.LinearExposure:.4g}"


class Impl:
    """one restatement of row N3 behind the batch entries both libraries export"""

    def __init__(self, name, lib, prefix, tonemap):
        self.name, self._tonemap = name, tonemap
        self._rotate, self._pow, self._accumulate = (getattr(lib, prefix + s) for s in ("rotate_primaries", "pow_batch", "accumulate"))
        tonemap.restype = self._rotate.restype = self._pow.restype = None
        tonemap.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self._rotate.argtypes = [F32P, C.c_uint32, F32P]
        self._pow.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]

    def tonemap(self, hdr, p):
        hdr = np.ascontiguousarray(hdr, dtype=np.float32)
        out = np.empty(len(hdr), dtype=np.uint32)
        self._tonemap(hdr.ctypes.data, len(hdr), C.addressof(p), out.ctypes.data)
        return out

    def matrix(self, rotation):
        """the matrix read back through the unit vectors (exact: every product is c * 1 or c * 0)"""
        m = np.empty((3, 3), dtype=np.float32)
        for j in range(3):
            e, col = np.zeros(3, dtype=np.float32), np.empty(3, dtype=np.float32)
            e[j] = 1.0
            self._rotate(e.ctypes.data_as(F32P), rotation, col.ctypes.data_as(F32P))
            m[:, j] = col
        return m

    def pow(self, x, y):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        self._pow(x.ctypes.data, y, len(x), out.ctypes.data)
        return out

    def accumulate(self, acc, x, n):
        assert acc.dtype == np.float32 and x.dtype == np.float32 and acc.flags.c_contiguous and x.flags.c_contiguous
        self._accumulate(acc.ctypes.data, x.ctypes.data, acc.size // 4, n)


@pytest.fixture(scope="module")
def dev():
    from oracle.binding import declare_leaf_api
    lib = C.CDLL(os.path.join(HERE, "hostshim", "libdevmath_host.so"))
    declare_leaf_api(lib, "dev_")
    return lib


@pytest.fixture(scope="module")
def impls(dev, oracle):
    return {"header": Impl("header", dev, "dev_", dev.dev_tonemap), "oracle": Impl("oracle", oracle.lib, "oracle_", oracle.lib.oracle_tonemap)}


def unpack(codes, p):
    """(n,) packed -> (n, 3) colour codes, (n,) alpha"""
    if p.TransferFunction == ref.TF_ST2084:
        return np.stack([codes & 1023, (codes >> 10) & 1023, (codes >> 20) & 1023], -1).astype(np.int64), codes >> 30
    u = unpack8(codes)
    return u[:, :3].astype(np.int64), u[:, 3]


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_pq_round_trip_and_known_points():
    y = np.exp(np.linspace(np.log(1e-7), 0.0, 200001))
    err = np.abs(ref.pq_eotf(ref.pq_inverse_eotf(y)) / y - 1).max()
    print(f"EOTF(PQ(y)) = y: max relative error {err:.2e}")
    assert err < 1e-12
    # the published anchors of the curve: 10 000 cd/m2 is full scale, 100 cd/m2 is 0.508 (BT.2100: SDR white sits at ~51 % PQ), 0 is ~7.3e-7
    assert ref.pq_inverse_eotf(1.0) == 1.0 and abs(ref.pq_inverse_eotf(0.01) - 0.5081) < 5e-5 and ref.pq_inverse_eotf(0.0) < 1e-6
    assert (np.diff(ref.pq_inverse_eotf(y)) > 0).all()


def test_reference_matrices_against_bt2087():
    # ITU-R BT.2087's printed BT.709 -> BT.2020 matrix (four decimals), the one rotation a recommendation publishes
    bt2087 = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]])
    assert np.abs(ref.rotation_matrix(ref.ROT_709_TO_2020) - bt2087).max() <= 5e-5
    for rot in ref.ROTATION_PRIMARIES:
        m = ref.rotation_matrix(rot)
        assert np.abs(m.sum(1) - 1).max() < 1e-14  # white stays white by construction
    # BT.709's luminance weights fall out of the same construction
    assert np.abs(ref.rgb_to_xyz(ref.BT709)[1] - [0.2126, 0.7152, 0.0722]).max() < 5e-5


def test_exposure_is_two_to_the_stops(dxrs):
    for stops in (0.0, -2.0, 1.5, 1.0):
        assert dxrs.types.tonemap_params(exposure_stops=stops).LinearExposure == np.float32(2.0 ** stops)


# ------------------------------------------------------------------------------------------------ a. matrices
@pytest.mark.parametrize("which", ["header", "oracle"])
def test_matrices_against_chromaticities(impls, which):
    for rot, name in ((ref.ROT_709_TO_2020, "709->2020"), (ref.ROT_P3D65_TO_2020, "P3D65->2020"), (ref.ROT_709_TO_P3D65, "709->P3D65")):
        m = impls[which].matrix(rot).astype(np.float64)
        d, s = np.abs(m - ref.rotation_matrix(rot)).max(), np.abs(m.sum(1) - 1).max()
        print(f"{which} {name}: max |entry - derived| {d:.3e}, max |row sum - 1| {s:.3e}")
        assert d <= 5e-5 and s <= 2e-6


# ------------------------------------------------------------------------------------------------ b. codes against float64
def sdr_pixels(n):
    """independent channels, log-uniform over [1e-6, 1e4], with exact zeros and the values a display curve turns on"""
    rng = np.random.default_rng(2084)
    x = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), (n, 4))).astype(np.float32)
    x[rng.random((n, 4)) < 0.03] = 0.0
    x[:8, :3] = np.float32([1e-6, 0.18, 0.25, 0.5, 1.0, 2.0, 100.0, 1e4])[:, None]
    return x


def hdr10_pixels(n):
    """channel ratios within 100:1 (a common level, log-uniform over [1e-5, 1e3], times a factor in [0.1, 10] per channel), so that the
    rotation's condition number stays <= 2 even on the row with the negative coefficient; greys, and black"""
    rng = np.random.default_rng(709)
    x = (np.exp(rng.uniform(np.log(1e-5), np.log(1e3), (n, 1))) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (n, 4)))).astype(np.float32)
    grey = rng.random(n) < 0.05
    x[grey] = x[grey, :1]
    x[:4] = np.float32([0.0, 1.0, 50.0, 125.0])[:, None]
    return x


@pytest.fixture(scope="module")
def pixels():
    return {False: sdr_pixels(SWEEP), True: hdr10_pixels(SWEEP)}


def check_codes(impls, pixels, p):
    hdr = pixels[p.TransferFunction == ref.TF_ST2084]
    matrix = None
    if p.TransferFunction == ref.TF_ST2084:
        # the header's own matrix, widened: the matrix is judged in (a), and near black the curve is steep enough for a 1e-5 difference in
        # an entry to move a code by dozens
        matrix = impls["header"].matrix(p.ColorRotation).astype(np.float64)
        assert np.array_equal(matrix, impls["oracle"].matrix(p.ColorRotation))
        cond = ref.condition(hdr, matrix).max()
        assert cond <= 2.0, cond
    want, delta = ref.value(hdr, p, matrix)
    assert delta.max() <= DELTA_LIMIT, (label(p), delta.max())
    worst = {}
    for name, impl in impls.items():
        code, a = unpack(impl.tonemap(hdr, p), p)
        assert (a == ref.alpha(p)).all()
        excess = np.abs(code - want) - 0.5
        worst[name] = (excess / delta).max()
        print(f"{label(p)} [{name}]: max (|code - value| - 0.5) / delta = {worst[name]:.3f}, max excess {excess.max():.3e} code, max delta {delta.max():.3e} code"
              + (f", max condition {cond:.3f}" if matrix is not None else ""))
    assert max(worst.values()) < 1.0, (label(p), worst)


@pytest.mark.parametrize("index", range(33))
def test_codes_against_float64(dxrs, impls, pixels, index):
    params = all_params(dxrs)
    assert len(params) == 33
    check_codes(impls, pixels, params[index])


# ------------------------------------------------------------------------------------------------ c. pow_spec at the exponents in use
@pytest.mark.parametrize("which", ["header", "oracle"])
@pytest.mark.parametrize("y, lo, hi", [(1.0 / 2.2, 1e-6, 1.0), (0.1593017578, 1e-12, 1e4), (78.84375, 0.8359375, 1.0)])
def test_pow_spec_at_the_display_exponents(impls, which, y, lo, hi):
    rng = np.random.default_rng(24)
    x = np.exp(rng.uniform(np.log(lo), np.log(hi), SWEEP)).astype(np.float32)
    x = np.clip(np.concatenate([x, np.float32([lo, hi])]), np.float32(lo), np.float32(hi))
    y32 = np.float32(y)
    got = impls[which].pow(x, y32).astype(np.float64)
    want = x.astype(np.float64) ** np.float64(y32)
    err, bound = np.abs(got / want - 1), ref.pow_spec_relative_error(x, y32)
    print(f"{which} pow_spec(x, {y32:.10g}) on [{lo:g}, {hi:g}]: max relative error {err.max():.3e}, max error / bound {(err / bound).max():.3f}, bound up to {bound.max():.3e}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ d. monotonicity
def test_codes_never_decrease_along_a_grey_ramp(dxrs, impls):
    ramp = np.concatenate([[0.0], np.geomspace(1e-12, 1e4, (1 << 16) - 1)]).astype(np.float32)
    assert (np.diff(ramp) > 0).all()
    hdr = np.repeat(ramp[:, None], 4, axis=1)
    for p in all_params(dxrs):
        top = 1023 if p.TransferFunction == ref.TF_ST2084 else 255
        for name, impl in impls.items():
            code, _ = unpack(impl.tonemap(hdr, p), p)
            assert (np.diff(code, axis=0) >= 0).all(), (label(p), name)
            assert (code[0] == 0).all() and (code[-1] == top).all(), (label(p), name, code[0], code[-1])


# ------------------------------------------------------------------------------------------------ e. running mean
@pytest.mark.parametrize("which", ["header", "oracle"])
@pytest.mark.parametrize("M", [1.0, 100.0])
def test_running_mean_against_float64(impls, which, M):
    """Each step adds at most u M from the fma's rounding and at most 6 u M / (n + 1) from the difference and the reciprocal; with
    (n + 1) e_n = n e_(n-1) + (n + 1) eps_n the sum is e_N <= (N / 2 + 8) u M."""
    N, npix = 4096, 2000
    rng = np.random.default_rng(4096)
    flip = np.where(rng.random((npix, 4)) < 0.25, -1.0, 1.0)  # this quarter of the values changes sign from frame to frame
    acc, total, worst = np.zeros((npix, 4), dtype=np.float32), np.zeros((npix, 4)), 0.0
    for n in range(N):
        x = rng.uniform(0.0, M, (npix, 4))
        x = np.where((flip < 0) & (rng.random((npix, 4)) < 0.5), -x, x).astype(np.float32)
        impls[which].accumulate(acc, x, n)
        total += x
        if (n + 1) & n == 0:  # after 1, 2, 4, ... frames
            err, bound = np.abs(acc - total / (n + 1)).max(), ((n + 1) / 2 + 8) * 2.0 ** -24 * M
            worst = err / bound
            assert err <= bound, (n + 1, err, bound)
    print(f"{which} running mean, M = {M:g}: after {N} frames the error is {worst:.4f} of the bound")


# ------------------------------------------------------------------------------------------------ GPU: past the first stride
GUARD = 256
SENTINEL = -1515870811  # 0xA5A5A5A5
SMALL = [1, 255, 256, 257]
LARGE = [STRIDE - 1, STRIDE, STRIDE + 1, 2 * STRIDE + 77]
FRAMES = [0, 1, 7, (1 << 24) - 1, 1 << 24, 0xFFFFFFFE]


def indexed_pixels(n, seed, specials):
    """seeded radiance whose value also depends on the pixel index, so a pixel written from the wrong source shows; alpha is the index"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    x = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), (n, 4))).astype(np.float32)
    x[:, :3] *= (1.0 + ((i * 2654435761) % 4096) / 8192.0).astype(np.float32)[:, None]
    if specials:
        s = hdr_samples(rng, max(n // 64, 16))[:min(4096, n // 128 + 1)]
        x[rng.integers(0, n, len(s))] = s
    else:
        x[rng.random((n, 4)) < 0.25] *= -1.0
    x[:, 3] = i
    return x


class Guarded:
    """n_words 32-bit words on the device between two runs of guard words"""

    def __init__(self, torch, n_words, init=None):
        self.n = n_words
        self.buf = torch.full((n_words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        if init is not None:
            self.buf[GUARD:GUARD + n_words] = torch.from_numpy(np.ascontiguousarray(init).view(np.int32).reshape(-1)).cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        torch.cuda.synchronize()

    def read(self):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), "guard words overwritten"
        return b[GUARD:GUARD + self.n].view(np.uint32)


def large_settings(dxrs):
    t = dxrs.types
    return [t.tonemap_params(t.TONE_REINHARD, t.TRANSFER_LINEAR, 1.5), t.tonemap_params(t.TONE_ACES_FILMIC, t.TRANSFER_SRGB, 0.0),
            t.tonemap_params(t.TONE_NONE, t.TRANSFER_ST2084, 0.0, 200.0, t.ROTATE_P3D65_TO_2020)]


@pytest.fixture(scope="module")
def big(dxrs, impls):
    """the largest input and the header's codes for it, once; a smaller size is a prefix of both"""
    hdr = indexed_pixels(LARGE[-1], 31, specials=True)
    return hdr, [impls["header"].tonemap(hdr, p) for p in large_settings(dxrs)]


@pytest.fixture(scope="module")
def big_frames():
    """finite, sign-mixed accumulator and frame for the running mean, once"""
    return indexed_pixels(STRIDE + 1, 32, specials=False), indexed_pixels(STRIDE + 1, 33, specials=False)


def run_tonemap(torch, renderer, hdr, settings, want):
    d_hdr = torch.from_numpy(hdr).cuda()
    for p, w in zip(settings, want):
        out = Guarded(torch, len(hdr))
        renderer.tonemap(d_hdr.data_ptr(), len(hdr), p, out.ptr)
        renderer.synchronize()
        got = out.read()
        bad = np.flatnonzero(got != w)
        assert len(bad) == 0, (label(p), len(hdr), len(bad), bad[:8], got[bad[:8]], w[bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_gpu_tonemap_block_edges(dxrs, impls, renderer, n):
    import torch
    hdr = indexed_pixels(n, 30 + n, specials=True)
    settings = all_params(dxrs)
    run_tonemap(torch, renderer, hdr, settings, [impls["header"].tonemap(hdr, p) for p in settings])


@pytest.mark.gpu
@pytest.mark.parametrize("n", LARGE)
def test_gpu_tonemap_past_the_first_stride(dxrs, renderer, big, n):
    import torch
    hdr, want = big
    run_tonemap(torch, renderer, hdr[:n], large_settings(dxrs), [w[:n] for w in want])


@pytest.mark.gpu
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("n", [257, STRIDE + 1])
def test_gpu_accumulate_past_the_first_stride(impls, renderer, big_frames, n, frames):
    import torch
    acc0, x = big_frames[0][:n].copy(), big_frames[1][:n].copy()
    if frames == 0:
        acc0[:] = np.nan  # the first frame replaces whatever the accumulator held
    want = acc0.copy()
    impls["header"].accumulate(want, x, frames)
    if frames == 0:
        assert np.array_equal(want.view(np.uint32), x.view(np.uint32))
    d_x = torch.from_numpy(x).cuda()
    acc = Guarded(torch, 4 * n, init=acc0)
    renderer.accumulate(acc.ptr, d_x.data_ptr(), n, frames)
    renderer.synchronize()
    got = acc.read().reshape(n, 4)
    bad = np.flatnonzero((got != want.view(np.uint32)).any(1))
    assert len(bad) == 0, (n, frames, len(bad), bad[:8])
    assert np.array_equal(d_x.cpu().numpy().view(np.uint32), x.view(np.uint32))  # the frame is read only


@pytest.mark.gpu
def test_gpu_accumulate_rejects_a_full_frame_count(renderer):
    import torch
    buf = Guarded(torch, 2 * 4 * 4)
    with pytest.raises(RuntimeError):
        renderer.accumulate(buf.ptr, buf.ptr + 64, 4, 0xFFFFFFFF)
    renderer.synchronize()
    assert (buf.read().view(np.int32) == SENTINEL).all()


@pytest.mark.gpu
def test_gpu_queued_calls_equal_the_synchronised_sequence(dxrs, impls, renderer, big_frames):
    """two accumulates and a tone map back to back on the context's stream, no synchronise in between"""
    import torch
    n = STRIDE + 1
    f0, f1 = np.abs(big_frames[0]), np.abs(big_frames[1])
    p = dxrs.types.tonemap_params()
    want_acc = np.full((n, 4), np.nan, dtype=np.float32)
    impls["header"].accumulate(want_acc, f0, 0)
    impls["header"].accumulate(want_acc, f1, 1)
    want = impls["header"].tonemap(want_acc, p)
    d_f0, d_f1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    results = []
    for synchronise in (True, False):
        acc, out = Guarded(torch, 4 * n, init=np.full((n, 4), np.nan, dtype=np.float32)), Guarded(torch, n)
        for step in (lambda: renderer.accumulate(acc.ptr, d_f0.data_ptr(), n, 0), lambda: renderer.accumulate(acc.ptr, d_f1.data_ptr(), n, 1),
                     lambda: renderer.tonemap(acc.ptr, n, p, out.ptr)):
            step()
            if synchronise:
                renderer.synchronize()
        renderer.synchronize()
        results.append((acc.read().copy(), out.read().copy()))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert np.array_equal(results[1][0].reshape(n, 4), want_acc.view(np.uint32)) and np.array_equal(results[1][1], want)
