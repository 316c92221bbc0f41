"""Row N5 -- bloom (PostProcessing::Bloom + Merge: Source/Bloom.ixx, Shaders/Bloom.hlsl, Shaders/Merge.hlsl).
CPU: the numpy restatement (tests/bloom_reference.py) against hand-derived known answers, the product's header
(csrc/pt_bloom.h compiled as host C++ by tests/hostshim/bloom_host.cpp) against the restatement step by step, and the
C-ABI's argument validation.  GPU: pt_bloom against the host-compiled header, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import bloom_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(32, 32), (67, 45), (256, 256), (1920, 1080)]
STRENGTHS = [0.0, 0.05, 1.0]


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_bloom_shim())
    vp, u32, f = C.c_void_p, C.c_uint32, C.c_float
    lib.bloom_to_srgb.restype = f
    lib.bloom_to_srgb.argtypes = [f]
    lib.bloom_karis_weight.restype = f
    lib.bloom_karis_weight.argtypes = [vp]
    lib.bloom_chain_layout.restype = C.c_uint64
    lib.bloom_chain_layout.argtypes = [u32, u32, vp, vp]
    lib.bloom_down_px.restype = None
    lib.bloom_down_px.argtypes = [vp, u32, u32, u32, u32, u32, u32, C.c_int, vp]
    lib.bloom_up_px.restype = None
    lib.bloom_up_px.argtypes = [vp, u32, u32, u32, u32, u32, u32, vp]
    lib.bloom_sample.restype = None
    lib.bloom_sample.argtypes = [vp, u32, u32, f, f, vp]
    lib.bloom_merge.restype = None
    lib.bloom_merge.argtypes = [vp, vp, u32, u32, u32, u32, f, vp]
    lib.bloom_host.restype = None
    lib.bloom_host.argtypes = [vp, vp, u32, u32, f]
    lib.bloom_host_trace.restype = None
    lib.bloom_host_trace.argtypes = [vp, vp, u32, u32, f, vp]
    return lib


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_bloom(shim, img, strength):
    img = c32(img)
    out = np.empty_like(img)
    shim.bloom_host(img.ctypes.data, out.ctypes.data, img.shape[1], img.shape[0], strength)
    return out


def host_trace(shim, img, strength):
    img = c32(img)
    h, w = img.shape[:2]
    dims = ref.chain_dims(w, h)
    order = list(range(ref.MIPS)) + list(range(ref.MIPS - 2, -1, -1))
    steps = np.empty((sum(dims[k][0] * dims[k][1] for k in order), 4), dtype=np.float32)
    out = np.empty_like(img)
    shim.bloom_host_trace(img.ctypes.data, out.ctypes.data, w, h, strength, steps.ctypes.data)
    res, at = [], 0
    for k in order:
        n = dims[k][0] * dims[k][1]
        res.append(steps[at:at + n].reshape(dims[k][1], dims[k][0], 4))
        at += n
    return out, res


def random_hdr(rng, w, h):
    """radiance-like: log-uniform over 6 decades, some black texels, a few fireflies; alpha 1"""
    x = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 4))).astype(np.float32)
    x[rng.random((h, w, 4)) < 0.05] = 0.0
    x[rng.random((h, w)) < 0.001, :3] = 5e4
    x[..., 3] = 1.0
    return x


def const_image(w, h, c, alpha=0.25):
    img = np.empty((h, w, 4), dtype=np.float32)
    img[..., :3] = c
    img[..., 3] = alpha
    return img


# ------------------------------------------------------------------------------------------------------------------ CPU


def test_chain_layout(shim):
    dims = (C.c_uint32 * 10)()
    off = (C.c_uint64 * 5)()
    for w, h in [(32, 32), (67, 45), (1920, 1080), (33, 1000)]:
        total = shim.bloom_chain_layout(w, h, dims, off)
        want = ref.chain_dims(w, h)
        assert [(dims[2 * k], dims[2 * k + 1]) for k in range(5)] == want
        sizes = [a * b for a, b in want]
        assert list(off) == [sum(sizes[:k]) for k in range(5)] and total == sum(sizes)
    shim.bloom_chain_layout(1920, 1080, dims, off)
    assert (dims[8], dims[9]) == (60, 33)  # 960 >> 4, 540 >> 4


def test_known_answers_constant_image(shim):
    """a constant image: bilinear sampling, the plain downsample and the tent return it exactly (weights and sums are
    powers of two for these values); the Karis step returns 0.5c(k(0.125c) + k(0.5c)); the pipeline c(1-s) + c2 s."""
    c = np.array([0.375, 1.5, 5.0])
    w, h = 64, 48
    img = const_image(w, h, c)
    o = np.zeros(4, dtype=np.float32)
    for u, v in [(0.5, 0.5), (0.0, 0.0), (1.0, 0.3), (0.013, 0.977), (-3.0, 7.0)]:
        shim.bloom_sample(img.ctypes.data, w, h, u, v, o.ctypes.data)
        assert o[:3].tolist() == c.tolist() and o[3] == 0.25
    o3 = np.zeros(3, dtype=np.float32)
    for x, y in [(0, 0), (5, 7), (31, 23)]:
        shim.bloom_down_px(img.ctypes.data, w, h, w // 2, h // 2, x, y, 0, o3.ctypes.data)
        assert o3.tolist() == c.tolist()
        shim.bloom_up_px(img.ctypes.data, w, h, 2 * w, 2 * h, x, y, o3.ctypes.data)
        assert o3.tolist() == c.tolist()

    def k(rgb):  # KarisAverage, by hand in float64 with the exact sRGB curve
        s = np.where(rgb < 0.0031308, 12.92 * rgb, 1.055 * rgb ** (1 / 2.4) - 0.055)
        return 1.0 / (1.0 + (0.2126 * s[0] + 0.7152 * s[1] + 0.0722 * s[2]) * 0.25)

    def karis_step(v):
        return np.maximum(0.5 * v * (k(0.125 * v) + k(0.5 * v)), 1e-4)

    c1 = karis_step(c)
    shim.bloom_down_px(img.ctypes.data, w, h, w // 2, h // 2, 3, 4, 1, o3.ctypes.data)
    np.testing.assert_allclose(o3, c1, rtol=1e-5)
    np.testing.assert_allclose(ref.downsample(img[..., :3].astype(np.float64), w // 2, h // 2, True)[4, 3], c1, rtol=1e-12)
    c2 = karis_step(c1)  # step 2 is Karis again; steps 3-9 keep a constant
    for s in STRENGTHS:
        want = c * (1 - s) + c2 * s
        got = host_bloom(shim, img, s)
        np.testing.assert_allclose(got[..., :3].reshape(-1, 3), np.broadcast_to(want, (w * h, 3)), rtol=1e-5)
        assert (got[..., 3] == 0.25).all()
        r, _ = ref.bloom(img, s)
        np.testing.assert_allclose(r[..., :3].reshape(-1, 3), np.broadcast_to(want, (w * h, 3)), rtol=1e-7)  # the weights are fp32, as the ABI takes them
    # Karis weight and sRGB curve by themselves
    for x in [0.0, 0.001, 0.0031308, 0.05, 0.5, 1.0, 7.0]:
        want = 12.92 * x if x < 0.0031308 else 1.055 * x ** (1 / 2.4) - 0.055
        assert abs(shim.bloom_to_srgb(x) - want) <= 2e-6 * max(want, 1e-3)
    rgb = c32([0.2, 0.4, 0.9])
    np.testing.assert_allclose(shim.bloom_karis_weight(rgb.ctypes.data), k(rgb.astype(np.float64)), rtol=1e-6)


def _support(w, h, x0, y0):
    """conservative half-widths (in full-resolution pixels) of the region one texel can reach through the chain and the
    merge: every step reaches its widest tap plus one input texel of bilinear footprint"""
    dims = ref.chain_dims(w, h)
    rx = ry = 0.0
    sx, sy = [w / d[0] for d in dims], [h / d[1] for d in dims]
    in_sx, in_sy = 1.0, 1.0
    for k in range(ref.MIPS):  # downsample: taps at +-2 output texels
        rx += 2 * sx[k] + in_sx + sx[k]
        ry += 2 * sy[k] + in_sy + sy[k]
        in_sx, in_sy = sx[k], sy[k]
    for k in range(ref.MIPS - 2, -1, -1):  # upsample: taps at +-5e-3 UV
        rx += 5e-3 * w + sx[k + 1] + sx[k]
        ry += 5e-3 * h + sy[k + 1] + sy[k]
    return rx + sx[0] + 1, ry + sy[0] + 1


def test_impulse_spreads_over_its_footprint_only(shim):
    """one bright texel on black: the output differs from the all-black output inside the footprint the chain can reach
    and nowhere else, and it does cover (at least) the mip-4 texel around the impulse"""
    w, h = 320, 192
    x0, y0 = 131, 77
    black = const_image(w, h, 0.0, alpha=1.0)
    img = black.copy()
    img[y0, x0, :3] = 1000.0
    base = host_bloom(shim, black, 0.05)
    out = host_bloom(shim, img, 0.05)
    changed = (out != base).any(-1)
    ys, xs = np.nonzero(changed)
    rx, ry = _support(w, h, x0, y0)
    assert (np.abs(xs - x0) <= rx).all() and (np.abs(ys - y0) <= ry).all()
    # the mip-4 texel (32 x 32 full-resolution pixels here) that holds the impulse lights up in full, and the glow is wider
    # than a mip-3 texel on both axes
    m4 = 2 ** 5
    bx, by = (x0 // m4) * m4, (y0 // m4) * m4
    assert changed[by:by + m4, bx:bx + m4].all()
    assert xs.max() - xs.min() > 16 and ys.max() - ys.min() > 16
    assert (out[changed][:, :3] > base[changed][:, :3]).any(-1).all()
    r, _ = ref.bloom(img, 0.05)
    rb, _ = ref.bloom(black, 0.05)
    assert np.array_equal((np.abs(r - rb) > 0).any(-1), changed)


@pytest.mark.parametrize("w,h", SIZES)
def test_shim_matches_numpy_restatement(shim, w, h):
    rng = np.random.default_rng(w * 7919 + h)
    img = random_hdr(rng, w, h)
    out, steps = host_trace(shim, img, 0.05)
    want, want_steps = ref.bloom(img, 0.05)
    for i, (got_s, want_s) in enumerate(zip(steps, want_steps)):
        np.testing.assert_allclose(got_s[..., :3], want_s, rtol=1e-5, atol=0, err_msg=f"chain step {i + 1}")
        assert (got_s[..., 3] == 0).all()
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=0, err_msg="strength 0.05")
    for s in (0.0, 1.0):
        np.testing.assert_allclose(host_bloom(shim, img, s), ref.bloom(img, s)[0], rtol=1e-5, atol=0, err_msg=f"strength {s}")


def test_abi_validation_without_gpu(dxrs):
    lib = dxrs.load_hip().lib
    assert lib.pt_bloom(None, None, None, 64, 64, C.c_float(0.05)) == 1
    assert lib.pt_bloom(None, C.c_void_p(16), C.c_void_p(16), 1920, 1080, C.c_float(0.05)) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU


def bits_equal(got, want):
    """bit-exact equality, NaN compared by mask (payloads are not part of the contract)"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"NaN masks differ at {np.argwhere(gn != wn)[:5].tolist()}"
    g, wb = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.nonzero(g != wb)[0]
    assert bad.size == 0, f"{bad.size} words differ, first {bad[:5].tolist()}: {got[~gn][bad[:5]].tolist()} vs {want[~wn][bad[:5]].tolist()}"


def gpu_bloom(renderer, img, strength, in_place=False):
    import torch
    h, w = img.shape[:2]
    d_in = torch.from_numpy(c32(img)).cuda()
    d_out = d_in if in_place else torch.empty_like(d_in)
    renderer.bloom(d_in.data_ptr(), d_out.data_ptr(), w, h, strength)
    renderer.synchronize()
    return d_out.cpu().numpy()


def special_image(rng, w, h):
    img = random_hdr(rng, w, h)
    special = np.array([0.0, 1e-45, 1e-40, 1.17e-38, 3.4e38, 1e30, np.inf, np.nan], dtype=np.float32)
    mask = rng.random((h, w)) < 0.02
    img[mask, :3] = special[rng.integers(0, len(special), (int(mask.sum()), 3))]
    return img


@pytest.mark.gpu
def test_gpu_bit_exact_random_sizes(renderer, shim):
    rng = np.random.default_rng(5)
    for w, h in SIZES + [(3840, 2160)]:
        img = random_hdr(rng, w, h)
        for s in STRENGTHS:
            bits_equal(gpu_bloom(renderer, img, s), host_bloom(shim, img, s))


@pytest.mark.gpu
def test_gpu_bit_exact_rendered_c2_frame(dxrs, host, renderer, shim):
    spheres, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h = 1920, 1080
    renderer.set_scene(spheres, materials, sd)
    renderer.set_camera(host.camera(w, h, jitter_index=0))
    renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=0, bounces=8, spp=1))
    img, _ = renderer.render()
    img = img.reshape(h, w, 4)
    for s in (0.05, 1.0):
        bits_equal(gpu_bloom(renderer, img, s), host_bloom(shim, img, s))


@pytest.mark.gpu
def test_gpu_bit_exact_special_values(renderer, shim):
    rng = np.random.default_rng(9)
    for w, h in [(67, 45), (256, 256)]:
        img = special_image(rng, w, h)
        for s in STRENGTHS:
            bits_equal(gpu_bloom(renderer, img, s), host_bloom(shim, img, s))
    # all-zero and all-denormal images
    for v in (0.0, 1e-42):
        img = const_image(64, 64, v, alpha=1.0)
        bits_equal(gpu_bloom(renderer, img, 0.05), host_bloom(shim, img, 0.05))


@pytest.mark.gpu
def test_gpu_strength_zero_is_identity(renderer):
    rng = np.random.default_rng(12)
    img = random_hdr(rng, 256, 144)
    assert np.array_equal(gpu_bloom(renderer, img, 0.0).view(np.uint32), img.view(np.uint32))


@pytest.mark.gpu
def test_gpu_in_place(renderer, shim):
    rng = np.random.default_rng(13)
    img = random_hdr(rng, 1920, 1080)
    bits_equal(gpu_bloom(renderer, img, 0.05, in_place=True), gpu_bloom(renderer, img, 0.05))


@pytest.mark.gpu
def test_gpu_alternating_sizes_grow_and_reuse_scratch(dxrs, shim):
    rng = np.random.default_rng(14)
    small, large = random_hdr(rng, 256, 256), random_hdr(rng, 1920, 1080)
    r = dxrs.Renderer(device=0)
    try:
        for img in (small, large, small, large, small):
            bits_equal(gpu_bloom(r, img, 0.05), host_bloom(shim, img, 0.05))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_bloom_interleaved_with_frames_in_flight(dxrs, host, shim):
    """render -> bloom -> render -> bloom ... on a context with two frames in flight, then each bloomed frame against the
    same frame bloomed alone"""
    import torch
    w, h = 640, 360
    spheres, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0, frames_in_flight=2)
    try:
        r.set_scene(spheres, materials, sd)
        frames = [torch.empty((h * w, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
        outs = [torch.empty_like(f) for f in frames]
        gs = dxrs.types.graphics_settings(w, h, bounces=8, spp=1)
        for n in range(4):
            gs.FrameIndex = n
            r.set_camera(host.camera(w, h, jitter_index=n))
            r.set_constants(gs)
            r.render_device(frames[n].data_ptr())
            r.bloom(frames[n].data_ptr(), outs[n].data_ptr(), w, h, 0.05)
        r.synchronize()
        for n in range(4):
            f = frames[n].cpu().numpy().reshape(h, w, 4)
            got = outs[n].cpu().numpy().reshape(h, w, 4)
            bits_equal(got, host_bloom(shim, f, 0.05))
            bits_equal(got, gpu_bloom(r, f, 0.05))
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_invalid_arguments_on_live_context(dxrs, renderer):
    import torch
    lib = dxrs.load_hip().lib
    buf = torch.zeros((64 * 64, 4), dtype=torch.float32, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    ctx = renderer._ctx
    cases = [(None, p, 64, 64, 0.05), (p, None, 64, 64, 0.05), (p, p, 31, 64, 0.05), (p, p, 64, 31, 0.05), (p, p, 64, 64, float("nan")),
             (p, p, 64, 64, -0.01), (p, p, 64, 64, 1.01), (p, p, 64, 64, float("inf")), (p, p, 20000, 64, 0.05)]
    for a, b, w, h, s in cases:
        assert lib.pt_bloom(ctx, a, b, w, h, C.c_float(s)) == 1, (w, h, s)
        assert b"pt_bloom" in lib.pt_last_error(ctx)
    with pytest.raises(dxrs.PtError):
        renderer.bloom(buf.data_ptr(), buf.data_ptr(), 16, 16, 0.05)
    renderer.bloom(buf.data_ptr(), buf.data_ptr(), 64, 64, 1.0)  # the context still works
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(shim, tmp_path):
    """PostProcessing::Bloom (host/Bloom.hpp) with the reference's default settings: the bloomed frame equals the
    host-compiled header's bloom of the same radiance, bit for bit; a too-small size throws"""
    import subprocess
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_bloom")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_bloom.cpp"), "-o", exe,
                    "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 320, 180
    a, b = str(tmp_path / "radiance.f32"), str(tmp_path / "bloomed.f32")
    res = subprocess.run([exe, str(w), str(h), a, b], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout and "pt_bloom" in res.stdout and "strength 0.05" in res.stdout
    rad = np.fromfile(a, dtype=np.float32).reshape(h, w, 4)
    assert rad[..., :3].max() > 0
    bits_equal(np.fromfile(b, dtype=np.float32).reshape(h, w, 4), host_bloom(shim, rad, np.float32(0.05)))
