"""Row N12 -- the sharpening stand-in (pt_nis_sharpen: Streamline's NIS feature as App::ProcessNIS drives it; DESIGN.md spec S18).
CPU: the product's header (csrc/pt_nis.h compiled as host C++ by tests/hostshim/nis_host.cpp) against the float64 numpy restatement
(tests/nis_reference.py), the spec's properties (a flat image, a soft edge, a hard step, the limit, the transposed image, images smaller
than the border) and a stand-alone AddressSanitizer + UBSan program over the header.
GPU: pt_nis_sharpen against the host-compiled header bit for bit (random images at sizes around the workgroup's, a C2 frame through
pt_upscale), its ordering among frames in flight, argument errors, the C++ host mirror."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import nis_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENTINEL = np.uint32(0x7FC0BEEF).view(np.float32)  # test_upscale.py's payload NaN: survives exactly where nothing is written
GUARD = 64  # float4 texels either side of Output that a call must leave alone
MODES = (ref.HDR_NONE, ref.HDR_LINEAR)
SHARPNESS = (0.0, 0.5, 1.0)
EPS32 = 2.0 ** -24  # fp32 unit roundoff
# The header's usm (fp32) against the restatement's (float64), both on the same fp32 lumas.  M = the patch's largest luma, eps = 2^-24;
# each count below is a number of fp32 roundings times the magnitude they act on.
#  * u before its clamp, (-0.6001 y1 + 1.2002 y2 - 0.6001 y3) strength: three products and two sums on terms of at most 2.4 M in all
#    (7.2 eps M), times strength <= 3.73 (27 eps M); strength = k StrengthScale + StrengthMin with k = 1 - sat((Yc - start) ScaleY)
#    carries about 40 eps absolute (k 6 eps from ScaleY's own roundings, times StrengthScale <= 3.7, plus the constants' and the sum's
#    roundings), on |raw| <= 2.4 M: 96 eps M; the product 9 eps M.  The clamp to +-limit is 1-Lipschitz and limit itself is within 9 eps M:
#    132 eps M.
#  * the contrast term: ac and bc are one subtraction of exact fp32 lumas each, so r = max / (min + Eps) is off by a *relative* 4 eps --
#    the slope 1 / Eps multiplies an error that is itself eps * ac -- and r only matters up to MaxContrastRatio (10, or 5), beyond which
#    the factor is pinned to 0: (r - MinContrastRatio) RatioNorm moves by at most 10 eps, on |u| <= limit <= 0.875 M: 11 eps M with U's
#    product.  Together 143 eps M per line.
#  * the weights are 0, 1 or, where both edge classes fire, e and 1 - e with e = A / (A + B); a g is off by 13 eps M (two three-term
#    sums of lumas, one difference), so e by 39 eps M / (A + B) + 2 eps, acting on two lines of at most `limit` each; the weights sum
#    to 1, so the lines' own errors are not doubled; the three-term sum adds 3 eps 0.875 M.
# So |usm - usm64| <= eps M (K_LINE + K_EDGE limit / (A + B) [both classes fire]) with K_LINE = 160 (143 + 3.5 + 2.6, rounded up for
# the constants' own fp32 roundings) and K_EDGE = 78, evaluated per texel on the restatement's A + B and limit.  On the random images
# below limit / (A + B) is of order 0.1 to 1, so the bound is about 1e-5 M.  Largest error seen, as a share of this bound: 0.0075
# (both modes, Sharpness 1; 0.0015 to 0.0032 at Sharpness 0 and 0.5), so the bound is 134 times what is seen.  Why so far: it adds
# every rounding at its largest magnitude and with one sign, and its two largest terms are idle on most of these texels -- a centre
# luma above SharpEndY (0.9, most of a [0.01, 100] image) makes k = 0 exactly, so strength and limit are nis_config's values with no
# rounding of their own (96 + 9 of the 160), and a line either sits on the clamp +-limit or is scaled to 0 by the contrast term.
K_LINE, K_EDGE = 160.0, 78.0
# a decision of step 3 may go the other way in fp32 where its float64 margin is below this; such texels are left out, and may be at
# most FLIP_SHARE of an image.  Seen: none in Linear mode; in mode None 1 of 1189 and 3 of 3015 texels (8.4e-4, 9.95e-4), all next
# to a +inf channel: sanitised to 65504 it makes a luma of up to 46848 in a corner of the 3 x 3, where B and a are both that luma
# plus a few units and `B > a` is a call within 1e-5.  The image's 0.5 % of +inf channels alone put the share next to the cap.
MARGIN, FLIP_SHARE = 1e-5, 1e-3


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_nis_shim())
    lib.nis_host_config.restype = None
    lib.nis_host_config.argtypes = [C.c_float, C.c_uint32, C.c_void_p]
    lib.nis_host_frame.restype = None
    lib.nis_host_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nis_host_frame_tiled.restype = None
    lib.nis_host_frame_tiled.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_sharpen(shim, color, sharpness, hdr, tiled=False):
    """pt_nis_sharpen on the host-compiled header -> (out (h, w, 4), usm (h, w), luma (h, w)); tiled: the kernel's workgroup tiles"""
    color = c32(color)
    h, w = color.shape[:2]
    out = np.full((h, w, 4), SENTINEL, np.float32)
    if tiled:
        shim.nis_host_frame_tiled(w, h, sharpness, hdr, color.ctypes.data, out.ctypes.data)
        return out
    usm, luma = np.full((h, w), SENTINEL, np.float32), np.full((h, w), SENTINEL, np.float32)
    shim.nis_host_frame(w, h, sharpness, hdr, color.ctypes.data, out.ctypes.data, usm.ctypes.data, luma.ctypes.data)
    return out, usm, luma


@functools.lru_cache(maxsize=None)
def random_image(w, h, seed=0):
    """log-uniform in [0.01, 100] with about 1 % each of NaN, +-inf and negative channels; alpha uniform.  Shared: do not write to it."""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    rgb = np.exp(rng.uniform(np.log(0.01), np.log(100.0), (h, w, 3))).astype(np.float32)
    for value, share in ((np.nan, 0.01), (np.inf, 0.005), (-np.inf, 0.005), (-1.5, 0.01)):
        rgb[rng.random((h, w, 3)) < share] = value
    img = np.concatenate([rgb, rng.uniform(0.0, 1.0, (h, w, 1)).astype(np.float32)], axis=-1)
    img.setflags(write=False)
    return img


def grey(values, alpha=1.0):
    """(h, w) lumas -> a grey float4 image"""
    v = np.asarray(values, np.float32)
    return np.stack([v, v, v, np.full_like(v, alpha)], axis=-1)


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def usm_bound(want):
    """the rounding bound on usm derived above, per texel"""
    with np.errstate(divide="ignore", invalid="ignore"):
        edge = np.where(want["both"], want["limit"] / want["apb"], 0.0)
    return EPS32 * want["M"] * (K_LINE + K_EDGE * edge)


def check_against_restatement(shim, color, sharpness, hdr):
    """header against restatement on one image -> (largest usm error as a share of its bound, marked share); asserts the rest"""
    out, usm, luma = host_sharpen(shim, color, sharpness, hdr)
    want = ref.sharpen(luma, color, sharpness, hdr)
    keep = want["margin"] >= MARGIN
    tol = usm_bound(want)
    err = np.abs(usm.astype(np.float64) - want["usm"])
    assert (err[keep] <= tol[keep]).all(), (np.argwhere(keep & (err > tol))[:4].tolist(), float((err / tol)[keep].max()))
    # step 6 on top of it.  None: one sum.  Linear: corr = (Yn^2 + Eps) / (Yc^2 + Eps) moves by 2 Yn / (Yn^2 + Eps) per unit of usm, a
    # further 8 eps relative for its own operations and Eps's rounding
    rgb = ref.sanitize(color[..., :3])
    if hdr == ref.HDR_LINEAR:
        yn = np.maximum(want["yc"] + want["usm"], 0.0)
        eps = want["config"]["Eps"]
        rel = 2.0 * yn * tol / (yn * yn + eps) + 8.0 * EPS32
        tol_out = want["out"] * rel[..., None] + 1e-45
    else:
        tol_out = tol[..., None] + 2.0 * EPS32 * np.maximum(want["out"], rgb)
    err_out = np.abs(out[..., :3].astype(np.float64) - want["out"])
    assert (err_out[keep] <= tol_out[keep]).all(), np.argwhere(keep[..., None] & (err_out > tol_out))[:4].tolist()
    assert np.array_equal(out[..., 3].view(np.uint32), c32(color)[..., 3].view(np.uint32))  # alpha passes through
    assert np.isfinite(out[..., :3]).all() and (out[..., :3] >= 0).all()
    share = float((err / np.maximum(tol, 1e-300))[keep].max()) if keep.any() else 0.0
    return share, 1.0 - float(keep.mean())


# ------------------------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("hdr", MODES)
@pytest.mark.parametrize("size", [(41, 29), (67, 45)])
def test_step1_luma_bit_exact(shim, size, hdr):
    """sanitise and luma against numpy float32 in the spec's order"""
    color = random_image(*size)
    _, _, luma = host_sharpen(shim, color, 0.5, hdr)
    bits_equal(luma, ref.luma32(color, hdr), "luma")
    assert np.isfinite(luma).all() and (luma >= 0).all() and luma.max() > (1.0 if hdr else 50.0)


@pytest.mark.parametrize("hdr", MODES)
@pytest.mark.parametrize("sharpness", (0.0, 0.25, 0.5, 0.75, 1.0))
def test_config_matches_the_tables(shim, sharpness, hdr):
    got = np.zeros(12, np.float32)
    shim.nis_host_config(sharpness, hdr, got.ctypes.data)
    c = ref.config(sharpness, hdr)
    want = [c[k] for k in ("DetectRatio", "DetectThres", "MinContrastRatio", "RatioNorm", "SharpStartY", "ScaleY", "StrengthMin", "StrengthScale",
                           "LimitMin", "LimitScale", "LimitMax", "Eps")]
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (got, want)
    assert c["StrengthMin"] >= 0 and c["StrengthScale"] > 0 and c["LimitScale"] > 0


@pytest.mark.parametrize("hdr", MODES)
@pytest.mark.parametrize("sharpness", SHARPNESS)
@pytest.mark.parametrize("size", [(41, 29), (67, 45)])
def test_header_matches_numpy_restatement(shim, size, sharpness, hdr):
    share, marked = check_against_restatement(shim, random_image(*size), sharpness, hdr)
    print(f"{size[0]}x{size[1]} sharpness {sharpness} hdr {hdr}: largest usm error {share:.3g} of the bound, {marked:.2e} of the texels marked")
    assert marked <= FLIP_SHARE


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (3, 2), (5, 5)])
def test_images_smaller_than_the_border(shim, size):
    """the border clamp covers the whole patch: they run and agree with the restatement (every texel: the ties these images are full
    of are ties in the header too)"""
    for hdr in MODES:
        for sharpness in SHARPNESS:
            color = random_image(*size, seed=3)
            _, marked = check_against_restatement(shim, color, sharpness, hdr)
            assert marked == 0.0
            bits_equal(host_sharpen(shim, color, sharpness, hdr, tiled=True), host_sharpen(shim, color, sharpness, hdr)[0], "tiled")
    # 1 x 1: the patch is flat, so the texel is its sanitised self
    one = c32([[[0.3, np.nan, 7.0, 0.5]]])
    bits_equal(host_sharpen(shim, one, 1.0, 0)[0], c32([[[0.3, 0.0, 7.0, 0.5]]]), "1x1")


@pytest.mark.parametrize("size", [(31, 7), (32, 8), (33, 9), (67, 45), (100, 20)])
def test_workgroup_tiles_equal_the_whole_image(shim, size):
    """the kernel's staging, run on the host: per 32 x 8 block a 36 x 12 tile staged with clamped coordinates gives the frame of the
    whole-image path bit for bit"""
    for hdr in MODES:
        color = random_image(*size, seed=1)
        bits_equal(host_sharpen(shim, color, 0.5, hdr, tiled=True), host_sharpen(shim, color, 0.5, hdr)[0], f"{size} hdr {hdr}")


@pytest.mark.parametrize("hdr", MODES)
def test_flat_image_is_the_sanitised_input(shim, hdr):
    """equal lumas give usm = 0: the output is the sanitised input bit for bit, alpha bits kept"""
    w, h = 19, 11
    color = np.empty((h, w, 4), np.float32)
    color[...] = (0.6, 0.3, 1.7, 0.25)
    for sharpness in SHARPNESS:
        out, usm, _ = host_sharpen(shim, color, sharpness, hdr)
        assert (usm == 0).all()
        bits_equal(out, color, "constant")
    # NaN, inf and negative channels everywhere: the sanitised image is constant too
    color[...] = (np.nan, np.inf, -2.0, -0.0)
    color[..., 3] = np.uint32(0x7FC01234).view(np.float32)  # an alpha that only survives as bits
    out, usm, _ = host_sharpen(shim, color, 1.0, hdr)
    want = color.copy()
    want[..., :3] = (0.0, 65504.0, 0.0)
    assert (usm == 0).all()
    bits_equal(out, want, "sanitised constant")


RAMP = (0.25, 0.35, 0.5, 0.65, 0.75)  # columns 5..9 of the soft edge; 0.2 to their left, 0.8 to their right


def soft_edge(w=16, h=20):
    cols = np.full(w, 0.2, np.float32)
    cols[5:10] = RAMP
    cols[10:] = 0.8
    return grey(np.tile(cols, (h, 1)))


def test_soft_vertical_edge(shim):
    color = soft_edge()
    prev = None
    at_035 = []
    for sharpness in (0.0, 0.25, 0.5, 0.75, 1.0):
        out, usm, _ = host_sharpen(shim, color, sharpness, 0)
        for a in (out, usm):
            assert np.array_equal(a.view(np.uint32), np.broadcast_to(a[:1], a.shape).view(np.uint32))  # all rows identical
        row = usm[0].astype(np.float64)
        assert (row[:7] <= 0).all() and (row[5:7] < 0).all()    # darker than mid-grey (column 7): pushed down
        assert (row[8:] >= 0).all() and (row[8:10] > 0).all()   # brighter: pushed up
        assert (row[:4] == 0).all() and (row[11:] == 0).all()   # two or more columns away from the ramp (columns 5..9)
        assert abs(row[7]) < 1e-6                               # the ramp is symmetric about mid-grey
        if prev is not None:
            assert (np.abs(row) >= prev).all(), sharpness       # non-decreasing in Sharpness
        prev = np.abs(row)
        at_035.append(row[6])
        assert np.allclose(out[0, :, 0], np.maximum(color[0, :, 0] + usm[0], 0), rtol=0, atol=1e-7)
    print("usm at the 0.35 column over Sharpness 0 .. 1:", [round(v, 4) for v in at_035])
    # the float64 prototype: 0.6001 (2 * 0.35 - 0.25 - 0.5) StrengthMax = -0.030005 * (0.025 .. 2.725)
    assert abs(at_035[0] - -0.00075) < 5e-5 and abs(at_035[-1] - -0.0818) < 5e-5


@pytest.mark.parametrize("hdr", MODES)
def test_hard_step_is_left_alone(shim, hdr):
    """0.2 | 0.6: on every line through the step one side's contrast is 0, so r = 0.4 / Eps is far above MaxContrastRatio and the
    contrast-ratio term of step 5 scales the unsharp mask to 0; the pass does not ring a hard edge"""
    cols = np.where(np.arange(16) < 8, 0.2, 0.6).astype(np.float32)
    color = grey(np.tile(cols, (20, 1)))
    for sharpness in SHARPNESS:
        out, usm, _ = host_sharpen(shim, color, sharpness, hdr)
        assert (usm == 0).all()
        bits_equal(out, color, "hard step")
    out, usm, _ = host_sharpen(shim, np.ascontiguousarray(color.transpose(1, 0, 2)), 1.0, hdr)
    assert (usm == 0).all()


@pytest.mark.parametrize("sharpness", SHARPNESS)
def test_limit_and_transposed_image(shim, sharpness):
    """HdrMode None on a random image: |out - c'| <= LimitMax Yc plus rounding, and the transposed image gives the transposed output.
    Transposing swaps the roles of 0 and 90 degrees exactly (g0 <-> g90, the column <-> the row, in the same order of operations), so
    where no diagonal fires the two outputs are equal bit for bit.  The diagonals map onto themselves with the 45-degree line read in
    reverse and g45's sums in another order, so there the outputs agree to rounding: twice the bound of the restatement test."""
    color = random_image(67, 45)
    out, usm, luma = host_sharpen(shim, color, sharpness, 0)
    want = ref.sharpen(luma, color, sharpness, 0)
    rgb = ref.sanitize(color[..., :3])
    limit = want["config"]["LimitMax"] * luma.astype(np.float64)
    room = limit * (1.0 + 16.0 * EPS32)
    assert (np.abs(usm) <= room).all()
    assert (np.abs(out[..., :3] - rgb) <= room[..., None] + 2.0 * EPS32 * np.maximum(out[..., :3], rgb)).all()
    if sharpness == 1.0:
        assert (np.abs(usm) >= 0.99 * want["limit"])[want["limit"] > 0].mean() > 0.01  # and the texel's own limit is reached
    out_t, usm_t, luma_t = host_sharpen(shim, np.ascontiguousarray(color.transpose(1, 0, 2)), sharpness, 0)
    bits_equal(luma_t.T, luma, "luma of the transposed image")
    keep = (want["margin"] >= MARGIN) & (want["apb"] > 0)
    axis_only = keep & ~want["cB"]
    assert axis_only.mean() > 0.1 and (keep & want["cB"]).mean() > 0.1
    got_t = out_t.transpose(1, 0, 2)
    assert np.array_equal(got_t.view(np.uint32)[axis_only], out.view(np.uint32)[axis_only])
    tol = 2.0 * usm_bound(want)
    assert (np.abs(usm_t.T.astype(np.float64) - usm)[keep] <= tol[keep]).all()
    assert (np.abs(got_t[..., :3].astype(np.float64) - out[..., :3])[keep] <= (tol[..., None] + 2.0 * EPS32 * out[..., :3])[keep]).all()


def test_sanitizer_program(tmp_path):
    """tests/cpp/nis_sanitize.cpp: the header under AddressSanitizer + UBSan as a stand-alone program (guard bytes around every
    buffer, the whole-image and the workgroup-tile path, 1x1, 3x2, 33x9 and 67x45, both modes)"""
    exe = str(tmp_path / "nis_sanitize")
    build = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", os.path.join(HERE, "cpp", "nis_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "nis_sanitize ok" in res.stdout, res.stdout + res.stderr


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import PtNisSettings, PtNisTextures
    lib = dxrs.load_hip().lib
    assert C.sizeof(PtNisSettings) == 16 and C.sizeof(PtNisTextures) == 16
    assert PtNisSettings.Sharpness.offset == 8 and PtNisSettings.HdrMode.offset == 12
    s = PtNisSettings(Size=(C.c_uint32 * 2)(32, 32), Sharpness=0.5, HdrMode=0)
    assert lib.pt_nis_sharpen(None, C.byref(s), C.byref(PtNisTextures())) == 1
    assert lib.pt_nis_sharpen(None, None, None) == 1


# ------------------------------------------------------------------------------------------------------------------ GPU


def gpu_sharpen(renderer, color, sharpness, hdr):
    """pt_nis_sharpen on a device copy; Output starts as the sentinel and sits between two guard bands that must stay the sentinel"""
    import torch
    color = c32(color)
    h, w = color.shape[:2]
    d = torch.from_numpy(color.copy()).cuda()  # (the shared images are read-only)
    out = torch.from_numpy(np.full((h * w + 2 * GUARD, 4), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    renderer.nis_sharpen_device((w, h), dict(Color=d.data_ptr(), Output=out.data_ptr() + 16 * GUARD), sharpness=sharpness, hdr_mode=hdr)
    renderer.synchronize()
    res = out.cpu().numpy()
    for band in (res[:GUARD], res[GUARD + h * w:]):
        assert np.array_equal(band.view(np.uint32), np.full(band.shape, SENTINEL).view(np.uint32)), "the guard band was written"
    assert np.array_equal(d.cpu().numpy().view(np.uint32), color.view(np.uint32)), "Color was written"
    return res[GUARD:GUARD + h * w].reshape(h, w, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (1, 7), (3, 2), (31, 7), (32, 8), (33, 9), (67, 45), (640, 360)])
def test_gpu_bit_exact_random_images(renderer, shim, size):
    color = random_image(*size, seed=2)
    for hdr in MODES:
        for sharpness in SHARPNESS:
            got = gpu_sharpen(renderer, color, sharpness, hdr)
            bits_equal(got, host_sharpen(shim, color, sharpness, hdr)[0], f"{size} hdr {hdr} sharpness {sharpness}")
            assert np.array_equal(got[..., 3].view(np.uint32), color[..., 3].view(np.uint32))  # alpha


@pytest.mark.gpu
def test_gpu_c2_frame_through_the_post_chain(dxrs, host, renderer, shim):
    """a C2 frame at 192 x 108, upscaled to 384 x 216 by pt_upscale, sharpened -- equal to the host header applied to the downloaded
    upscaler output -- then pt_bloom and pt_tonemap on it"""
    import torch
    w, h, W, H = 192, 108, 384, 216
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    renderer.set_scene(spheres, mats, sd)
    up = renderer.upscaler((W, H), mode=dxrs.types.UPSCALE_PERFORMANCE)
    assert up.input_size == (w, h)
    color = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    mv = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    sharp = torch.from_numpy(np.full((H, W, 4), SENTINEL, np.float32)).cuda()
    ldr = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cam = host.camera_matrices(w, h, jitter_index=0, jitter_count=32)
    renderer.set_camera(cam)
    renderer.set_constants(dxrs.types.graphics_settings(w, h, frame_index=0, bounces=8, spp=1))
    renderer.render_gbuffer_device(dict(LinearDepth=depth.data_ptr(), MotionVector=mv.data_ptr()))
    renderer.render_device(color.data_ptr())
    upscaled = up(color, depth, mv, jitter=(-cam.Jitter[0], -cam.Jitter[1]))
    renderer.nis_sharpen_device((W, H), dict(Color=upscaled.data_ptr(), Output=sharp.data_ptr()), sharpness=0.5)
    renderer.synchronize()
    src, got = upscaled.cpu().numpy(), sharp.cpu().numpy()
    want, usm, _ = host_sharpen(shim, src, 0.5, 0)
    bits_equal(got, want, "sharpened C2 frame")
    assert src[..., :3].max() > 0 and np.abs(usm).max() > 1e-3  # the frame has edges and the pass moved them
    renderer.bloom(sharp.data_ptr(), sharp.data_ptr(), W, H, 0.05)
    renderer.tonemap(sharp.data_ptr(), W * H, dxrs.types.tonemap_params(), ldr.data_ptr())
    renderer.synchronize()
    assert np.isfinite(sharp.cpu().numpy()).all() and int(ldr.cpu().numpy().view(np.uint32).max()) > 0


@pytest.mark.gpu
def test_gpu_sharpen_interleaved_with_frames_in_flight(dxrs, host, oracle, shim):
    """render -> sharpen -> render -> sharpen ... on a context with two frames in flight and no wait in between: the frames still
    equal their oracle images and each sharpened frame the header's"""
    import torch
    w, h = 160, 90
    spheres, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    r = dxrs.Renderer(device=0, frames_in_flight=2)
    try:
        r.set_scene(spheres, materials, sd)
        frames = [torch.empty((h * w, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
        outs = [torch.from_numpy(np.full((h * w, 4), SENTINEL, np.float32)).cuda() for _ in range(4)]
        torch.cuda.synchronize()
        for n in range(4):
            r.set_camera(host.camera(w, h, jitter_index=n))
            r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=n, bounces=8, spp=1))
            r.render_device(frames[n].data_ptr())
            r.nis_sharpen_device((w, h), dict(Color=frames[n].data_ptr(), Output=outs[n].data_ptr()), sharpness=1.0)
        r.synchronize()
        for n in range(4):
            f = frames[n].cpu().numpy().reshape(h, w, 4)
            gs = dxrs.types.graphics_settings(w, h, frame_index=n, bounces=8, spp=1)
            want, _ = oracle.render(spheres, materials, sd, host.camera(w, h, jitter_index=n), gs, threads=8)
            assert np.array_equal(f.view(np.uint32)[..., :3], want.view(np.uint32)[..., :3]), f"frame {n}"
            bits_equal(outs[n].cpu().numpy().reshape(h, w, 4), host_sharpen(shim, f, 1.0, 0)[0], f"sharpened frame {n}")
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, host, oracle, renderer):
    """every refusal of pt_api.h's list returns its status and writes nothing; the context then renders a correct frame"""
    from dxrs_amd.types import PtNisSettings, PtNisTextures
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    w, h = 32, 16
    n = w * h
    src = torch.zeros((2 * n + 1, 4), dtype=torch.float32, device="cuda")
    dst = torch.from_numpy(np.full((n + 1, 4), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    pc, po = src.data_ptr(), dst.data_ptr()

    def call(size=(w, h), sharpness=0.5, hdr=0, color=pc, output=po):
        s = PtNisSettings(Size=(C.c_uint32 * 2)(*size), Sharpness=sharpness, HdrMode=hdr)
        t = PtNisTextures(Color=C.c_void_p(color), Output=C.c_void_p(output))
        st = lib.pt_nis_sharpen(ctx, C.byref(s), C.byref(t))
        if st:
            assert b"pt_nis_sharpen" in lib.pt_last_error(ctx)
        return st

    s = PtNisSettings(Size=(C.c_uint32 * 2)(w, h), Sharpness=0.5, HdrMode=0)
    assert lib.pt_nis_sharpen(None, None, None) == 1
    assert lib.pt_nis_sharpen(ctx, None, C.byref(PtNisTextures())) == 1 and lib.pt_nis_sharpen(ctx, C.byref(s), None) == 1
    assert call(color=None) == 1 and call(output=None) == 1
    for size in ((0, h), (w, 0), (16385, h), (w, 16385)):
        assert call(size=size) == 1, size
    for sharpness in (np.nan, -0.01, 1.01, np.inf, -np.inf):
        assert call(sharpness=sharpness) == 1, sharpness
    assert call(color=pc + 8) == 1 and call(output=po + 8) == 1 and call(color=pc + 4) == 1
    assert call(output=pc) == 1                       # in place
    assert call(output=pc + 16 * (n - 1)) == 1        # the last texel of Color is the first of Output
    assert call(color=pc + 16 * n, output=pc + 16) == 1
    for hdr in (3, 99, 0xFFFFFFFF):
        assert call(hdr=hdr) == 1, hdr
    assert call(hdr=2) == 5                           # PQ: PT_ERR_UNSUPPORTED
    assert dxrs.binding.STATUS[5] == "PT_ERR_UNSUPPORTED"
    with pytest.raises(dxrs.PtError):
        renderer.nis_sharpen_device((w, h), dict(Color=pc, Output=pc))
    with pytest.raises(ValueError):
        renderer.nis_sharpen_device((w, h), dict(Color=pc, Depth=po))
    renderer.synchronize()
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), np.full((n + 1, 4), SENTINEL).view(np.uint32))  # nothing was written
    assert not src.cpu().numpy().any()
    # the accepted edges: Output right behind Color, both extreme Sharpness values, Linear
    assert call(output=pc + 16 * n) == 0 and call(sharpness=0.0) == 0 and call(sharpness=1.0, hdr=1) == 0
    renderer.synchronize()
    assert np.array_equal(dst.cpu().numpy()[n:].view(np.uint32), np.full((1, 4), SENTINEL).view(np.uint32))
    # a correct frame afterwards
    spheres, materials, sd = host.scene(dxrs.host.SCENE_SMALL, seed=0)
    gs = dxrs.types.graphics_settings(64, 64, frame_index=0, bounces=4, spp=2)
    cam = host.camera(64, 64)
    renderer.set_scene(spheres, materials, sd)
    renderer.set_camera(cam)
    renderer.set_constants(gs)
    img, st = renderer.render()
    want, ost = oracle.render(spheres, materials, sd, cam, gs, threads=4)
    assert st.rays == ost.rays and np.array_equal(img.view(np.uint32)[..., :3], want.view(np.uint32)[..., :3])


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(renderer, shim, tmp_path):
    """dxrs::Streamline (host/Streamline.hpp) from C++, against pt_api.h alone: a frame of the demo scene tagged and evaluated as
    App::ProcessNIS does equals the host-compiled header applied to the radiance the program downloaded, and the Python path on the
    same radiance; the DLSS features are unavailable, a missing tag and an in-place call are refused"""
    pkg = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
    exe = str(tmp_path / "host_nis")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(pkg, "host"), os.path.join(HERE, "cpp", "host_nis.cpp"),
                    "-o", exe, "-L", pkg, "-lpt_hip", f"-Wl,-rpath,{pkg}"], check=True)
    w, h = 200, 120
    outp = str(tmp_path / "nis.f32")
    res = subprocess.run([exe, str(w), str(h), "0.5", "0", outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error: missing output tag" in res.stdout and "expected error: pt_nis_sharpen: Output overlaps Color" in res.stdout
    assert "sharpness 0.5" in res.stdout
    raw = np.fromfile(outp, dtype=np.float32)
    assert raw.size == 2 * w * h * 4
    radiance, sharpened = raw[:w * h * 4].reshape(h, w, 4), raw[w * h * 4:].reshape(h, w, 4)
    assert radiance[..., :3].max() > 0
    bits_equal(sharpened, host_sharpen(shim, radiance, 0.5, 0)[0], "C++ host mirror against the header")
    bits_equal(sharpened, gpu_sharpen(renderer, radiance, 0.5, 0), "C++ host mirror against the Python path")
