"""Row N13 -- the frame-interpolation stand-in (pt_frame_gen: what Streamline's DLSS-G plugin makes of the resources
App::ProcessDLSSFrameGeneration tags; DESIGN.md spec S19).
CPU: the product's header (csrc/pt_framegen.h compiled as host C++ by tests/hostshim/framegen_host.cpp, the scatter a sequential min)
against the float64 numpy restatement (tests/framegen_reference.py), the spec's properties, a stand-alone ASan + UBSan program, the ABI.
GPU: pt_frame_gen against the host-compiled header bit for bit (random sequences, contention, the restart rules, a rendered animated
chain), frames in flight, argument errors, the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import framegen_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "directx-raytracing-spheres-demo_amd")
SENTINEL = np.uint32(0xDEADBEEF)
GUARD = 64  # pixels either side of Output that a call must leave alone
# A floor / inside / depth decision of spec S19 within this of flipping may go the other way in fp32; such pixels are left out at the
# shape whose ratio is not a power of two, and only there, up to this share of the pixels
NEAR, NEAR_SHARE = 1e-5, 1e-3


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_framegen_shim())
    lib.fg_host_frame.restype = None
    lib.fg_host_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.fg_host_key.restype = C.c_uint64
    lib.fg_host_key.argtypes = [C.c_float, C.c_uint32]
    lib.fg_host_pack.restype = C.c_uint32
    lib.fg_host_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    return lib


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class HostFrameGen:
    """pt_frame_gen on the host-compiled header, with the history logic of pt_api_post.hip: the first call, Reset and a change of a size or
    of the Format restart (Output = Color, the slot takes Color and Depth); two history slots alternate."""

    def __init__(self, shim, tiled=False):
        self.shim, self.key, self.slots, self.cur, self.generated, self.tiled = shim, None, None, 0, None, tiled
        self.trace = None

    def __call__(self, color, depth, mv, fmt=0, reset=False):
        color, depth, mv = u32(color), c32(depth), c32(mv)
        (h, w), (H, W) = depth.shape, color.shape
        key = (w, h, W, H, fmt)
        restart = bool(reset) or self.key is None or self.key != key
        if self.key is None or self.key[:4] != key[:4]:
            self.slots = [(np.zeros((H, W), np.uint32), np.zeros((h, w), np.float32)) for _ in range(2)]
        self.key = key
        prev, cur = self.slots[self.cur], self.slots[self.cur ^ 1]
        out = np.full((H, W), SENTINEL, np.uint32)
        if restart:
            out[:], cur[0][:], cur[1][:] = color, color, depth
            self.trace = None
        else:
            field = np.zeros((h, w), np.uint64)
            keys, valid, v = np.zeros((H, W), np.uint64), np.zeros((H, W, 2), np.uint32), np.zeros((H, W, 3), np.float32)
            size = np.array([w, h, W, H, fmt], np.uint32)
            ptrs = (C.c_void_p * 9)(*[a.ctypes.data for a in (color, depth, mv, out, prev[0], prev[1], cur[0], cur[1], field)])
            self.shim.fg_host_frame(size.ctypes.data, ptrs, 1 if self.tiled else 0, keys.ctypes.data, valid.ctypes.data, v.ctypes.data)
            self.trace = dict(field=field, k=keys, valid_a=valid[..., 0] != 0, valid_b=valid[..., 1] != 0, v=v)
        self.cur ^= 1
        self.generated = not restart
        return out

    def history(self):
        """the slot the last call wrote: (Color (H, W), Depth (h, w))"""
        return self.slots[self.cur]


def pack_rgb(rgb, fmt, alpha=None):
    rgb = np.asarray(rgb).astype(np.uint32)
    bits = 10 if fmt == 1 else 8
    a = np.uint32((3 << 30) if fmt == 1 else (255 << 24)) if alpha is None else np.asarray(alpha, np.uint32)
    return (rgb[..., 0] | (rgb[..., 1] << np.uint32(bits)) | (rgb[..., 2] << np.uint32(2 * bits)) | a).astype(np.uint32)


def random_color(rng, W, H, fmt):
    """random codes over the whole range with random alpha bits"""
    M = ref.channel_max(fmt)
    alpha = rng.integers(0, 4 if fmt == 1 else 256, (H, W)).astype(np.uint32) << np.uint32(30 if fmt == 1 else 24)
    return pack_rgb(rng.integers(0, M + 1, (H, W, 3)), fmt, alpha)


def random_frame(rng, w, h, W, H, fmt, depth=None, span=6.0):
    """Color at output size; depths from {1, 2, 4, +inf} in blocks of 5 x 3 pixels, kept from frame to frame except for a tenth of
    the blocks; motion vectors multiples of 1/64 pixel within +-span, mv.z from {0, +-0.25} (mostly 0)"""
    color = random_color(rng, W, H, fmt)
    by, bx = (h + 2) // 3, (w + 4) // 5
    blocks = rng.choice(np.array([1.0, 2.0, 4.0, np.inf], np.float32), (by, bx))
    fresh = np.repeat(np.repeat(blocks, 3, axis=0), 5, axis=1)[:h, :w]
    if depth is None:
        depth = fresh
    else:
        change = np.repeat(np.repeat(rng.random((by, bx)) < 0.1, 3, axis=0), 5, axis=1)[:h, :w]
        depth = np.where(change, fresh, depth)
    mv = np.zeros((h, w, 3), np.float32)
    mv[..., :2] = rng.integers(-int(span * 64), int(span * 64) + 1, (h, w, 2)) / 64.0
    mv[..., 2] = rng.choice(np.array([0.0, 0.0, 0.0, 0.25, -0.25], np.float32), (h, w))
    return color, c32(depth), mv


# ------------------------------------------------------------------------------------------------------------------ CPU

SHAPES_EXACT = [((41, 29), (41, 29)), ((67, 45), (67, 45)), ((20, 12), (40, 24))]
SHAPE_RATIO = ((33, 9), (50, 14))


def compare_with_restatement(shim, sizes, fmt, seed, frames=4):
    """-> (pixels left out, pixels compared, the largest |v - v64| / bound).  Every frame of the header against the restatement fed the
    header's own previous history slot."""
    (w, h), (W, H) = sizes
    exact = sizes != SHAPE_RATIO
    rng = np.random.default_rng(seed)
    fg = HostFrameGen(shim)
    depth, left_out, total, worst, seen = None, 0, 0, 0.0, {}
    for f in range(frames):
        color, depth, mv = random_frame(rng, w, h, W, H, fmt, depth)
        prev = None if f == 0 else tuple(a.copy() for a in fg.history())
        out = fg(color, depth, mv, fmt)
        assert fg.generated == (f != 0)
        if f == 0:
            assert np.array_equal(out, color)
            continue
        want, got = ref.generate(color, depth, mv, prev[0], prev[1], fmt, NEAR), fg.trace
        assert np.array_equal(got["field"], want["field"]), "the motion field differs"
        keep = np.ones((H, W), bool) if exact else want["margin"] >= NEAR
        left_out += int((~keep).sum())
        total += H * W
        assert np.array_equal(got["k"][keep], want["k"][keep]), "a source index differs"
        for name in ("valid_a", "valid_b"):
            assert np.array_equal(got[name][keep], want[name][keep]), name
        err = np.abs(got["v"].astype(np.float64) - want["v"]).max(axis=-1)
        holes = want["hole"] & keep
        assert np.array_equal(out[holes], prev[0][holes]), "a hole is not the previous frame's pixel"
        live = keep & ~want["hole"]
        assert (err[live] <= want["bound"][live]).all(), f"v off by {err[live].max()} against a bound of {want['bound'][live].min()}"
        worst = max(worst, float((err[live] / want["bound"][live]).max()))
        # floor(v + 0.5) on its own: exactly, from the header's own v
        own = ref.pack(got["v"], color, fmt)
        assert np.array_equal(out[~want["hole"]], own[~want["hole"]]), "the rounding of v differs"
        assert np.array_equal(fg.history()[0], color) and np.array_equal(fg.history()[1].view(np.uint32), depth.view(np.uint32))
        for name, mask in (("holes", want["hole"]), ("both", want["valid_a"] & want["valid_b"]), ("a alone", want["valid_a"] & ~want["valid_b"])):
            seen[name] = seen.get(name, 0) + int(mask.sum())
    assert all(seen[name] > 0 for name in ("holes", "both", "a alone")), seen  # (the inputs reach the branches)
    return left_out, total, worst


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("sizes", SHAPES_EXACT)
def test_header_matches_numpy_restatement(shim, sizes, fmt):
    """Vectors in multiples of 1/64 pixel at 1:1 and 2:1: every position is exact in fp32, so no pixel is left out.  Largest error
    seen: 0.007 of the bound."""
    left_out, total, worst = compare_with_restatement(shim, sizes, fmt, seed=sizes[0][0] + fmt)
    print(f"{sizes} format {fmt}: {total} pixels, largest error {worst:.3g} of the bound")
    assert left_out == 0 and total > 0


@pytest.mark.parametrize("fmt", [0, 1])
def test_header_matches_numpy_restatement_at_an_odd_ratio(shim, fmt):
    """33x9 -> 50x14: sx = 50/33 is rounded, so pixels with a decision within 1e-5 of flipping are left out, at most 1e-3 of them.
    Left out with the seeds used: 5 of 16800 pixels for Format 0 and 10 of 16800 for Format 1 (8 sequences of 4 frames each, the first
    frame a restart); largest error seen 0.20 of the bound."""
    left_out = total = 0
    worst = 0.0
    for seed in range(8):
        a, b, c = compare_with_restatement(shim, SHAPE_RATIO, fmt, seed=100 + 10 * fmt + seed)
        left_out, total, worst = left_out + a, total + b, max(worst, c)
    print(f"33x9 -> 50x14 format {fmt}: {left_out} of {total} pixels left out, largest error {worst:.3g} of the bound")
    assert left_out <= NEAR_SHARE * total


def test_restatement_alone_stays_under_the_cap():
    """the restatement's own count of near decisions over the odd-ratio sequences, without the header: 15 of 33600 pixels"""
    (w, h), (W, H) = SHAPE_RATIO
    near = total = 0
    for fmt in (0, 1):
        for seed in range(8):
            rng = np.random.default_rng(100 + 10 * fmt + seed)
            prev, depth = None, None
            for f in range(4):
                color, depth, mv = random_frame(rng, w, h, W, H, fmt, depth)
                if prev is not None:
                    near += int((ref.generate(color, depth, mv, prev[0], prev[1], fmt, NEAR)["margin"] < NEAR).sum())
                    total += W * H
                prev = (color, depth)
    print(f"the restatement alone: {near} of {total} pixels have a near decision")
    assert near <= NEAR_SHARE * total, (near, total)


def two_frames(shim, first, second, fmt=0, tiled=False):
    """(color, depth, mv) twice -> (the generated frame, the HostFrameGen)"""
    fg = HostFrameGen(shim, tiled)
    assert np.array_equal(fg(first[0], first[1], first[2], fmt), u32(first[0])) and not fg.generated  # the restart: Output == Color
    out = fg(second[0], second[1], second[2], fmt)
    assert fg.generated
    return out, fg


@pytest.mark.parametrize("fmt", [0, 1])
def test_identical_frames_at_rest_come_back_bit_for_bit(shim, fmt):
    rng = np.random.default_rng(3)
    for (w, h), (W, H) in SHAPES_EXACT + [SHAPE_RATIO, ((1, 1), (1, 1)), ((1, 1), (4, 4))]:
        color, depth, mv = random_frame(rng, w, h, W, H, fmt)
        mv[:] = 0.0
        out, fg = two_frames(shim, (color, depth, mv), (color, depth, mv), fmt)
        assert np.array_equal(out, color), (w, h, W, H)
        assert np.array_equal(fg.trace["field"].ravel() & np.uint64(0xFFFFFFFF), np.arange(w * h, dtype=np.uint64))  # everyone onto itself


def test_uniform_translation_by_integer_halves_shifts_the_image(shim):
    """mv = (-4, 2): the scene moved by (4, -2) since the previous frame; the frame between is the current one shifted back by (2, -1),
    bit for bit in the interior (alpha is the output pixel's own)"""
    rng = np.random.default_rng(4)
    w, h = 40, 24
    big = random_color(rng, w + 8, h + 8, 0) | np.uint32(0xFF000000)
    prev, cur = big[4:4 + h, 4:4 + w], big[4 + 2:4 + 2 + h, 4 - 4:4 - 4 + w]  # cur(x, y) = prev(x - 4, y + 2)
    depth = np.full((h, w), 3.0, np.float32)
    mv = np.zeros((h, w, 3), np.float32)
    mv[..., 0], mv[..., 1] = -4.0, 2.0
    out, _ = two_frames(shim, (prev, depth, mv), (cur, depth, mv))
    mid = big[4 + 1:4 + 1 + h, 4 - 2:4 - 2 + w]  # mid(x, y) = prev(x - 2, y + 1)
    assert np.array_equal(out[2:-2, 4:-4], mid[2:-2, 4:-4])


def texture(x, y, k):
    """a smooth RGB pattern in code values (float64), for sub-pixel shifts"""
    return np.stack([127.5 + 100.0 * np.sin(0.9 * x + k) * np.cos(0.7 * y - k), 127.5 + 100.0 * np.sin(0.5 * x - 0.8 * y + 2 * k),
                     127.5 + 100.0 * np.cos(0.6 * x + 0.4 * y + k)], axis=-1)


def disc_scene(t, disc_v, plane_v, w=48, h=32):
    """the prototype's scene at time t (frames): a textured disc of radius 8.3 at depth 2 over a textured plane at depth 8, each
    texture moving with its surface -> (packed colour, depth, mv of a frame rendered at t)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = 20.0 + disc_v[0] * t, 15.0 + disc_v[1] * t
    disc = (xs + 0.5 - cx) ** 2 + (ys + 0.5 - cy) ** 2 <= 8.3 ** 2
    rgb = np.where(disc[..., None], texture(xs - disc_v[0] * t, ys - disc_v[1] * t, 1.0), texture(xs - plane_v[0] * t, ys - plane_v[1] * t, 2.5))
    depth = np.where(disc, 2.0, 8.0).astype(np.float32)
    mv = np.zeros((h, w, 3), np.float32)
    mv[..., 0] = np.where(disc, -disc_v[0], -plane_v[0])
    mv[..., 1] = np.where(disc, -disc_v[1], -plane_v[1])
    return pack_rgb(np.floor(rgb + 0.5), 0), depth, mv


def rmse(a, b):
    return float(np.sqrt(np.mean((ref.decode(a, 0) - ref.decode(b, 0)) ** 2)))


# RMSE to the mid-time truth in code values, interpolated / rounded 50:50 blend, as measured on the CPU with this header:
# 0.00 / 35.39, 12.41 / 34.17, 22.39 / 65.26
DISC_CASES = {"disc (6, 2), static plane": ((6.0, 2.0), (0.0, 0.0)), "disc (5, -3), plane (1.5, 0.5)": ((5.0, -3.0), (1.5, 0.5)),
              "everything (4, -2)": ((4.0, -2.0), (4.0, -2.0))}


@pytest.mark.parametrize("case", list(DISC_CASES))
def test_disc_scene_beats_the_blend(shim, case):
    disc_v, plane_v = DISC_CASES[case]
    prev, cur, truth = disc_scene(0.0, disc_v, plane_v), disc_scene(1.0, disc_v, plane_v), disc_scene(0.5, disc_v, plane_v)
    out, _ = two_frames(shim, prev, cur)
    blend = ref.pack(0.5 * (ref.decode(prev[0], 0) + ref.decode(cur[0], 0)), cur[0], 0)
    e_out, e_blend = rmse(out, truth[0]), rmse(blend, truth[0])
    print(f"{case}: RMSE {e_out:.2f} interpolated, {e_blend:.2f} blend")
    assert e_out < e_blend
    if case.startswith("disc (6, 2)"):
        assert e_out == 0.0  # integer half vectors and the revealed plane taken from the previous frame: exact
    if case.startswith("everything"):
        assert np.array_equal(out[2:-2, 4:-4], truth[0][2:-2, 4:-4])


def test_resting_disc_scene_is_the_identity(shim):
    f = disc_scene(0.0, (0.0, 0.0), (0.0, 0.0))
    out, _ = two_frames(shim, f, f)
    assert np.array_equal(out, f[0])


def test_depth_rejection_keeps_the_current_sample_only(shim):
    """the previous frame had a nearer surface where b lands: the pixel is the current frame's sample alone"""
    rng = np.random.default_rng(6)
    w, h = 24, 12
    prev_c, cur_c = random_color(rng, w, h, 0), random_color(rng, w, h, 0)
    mv = np.zeros((h, w, 3), np.float32)
    far, near = np.full((h, w), 8.0, np.float32), np.full((h, w), 2.0, np.float32)
    near[:, :12] = 8.0
    out, fg = two_frames(shim, (prev_c, near, mv), (cur_c, far, mv))
    assert fg.trace["valid_a"].all() and fg.trace["valid_b"][:, :12].all() and not fg.trace["valid_b"][:, 12:].any()
    assert np.array_equal(out[:, 12:], cur_c[:, 12:])
    both = ref.pack(c32(0.5 * (ref.decode(prev_c, 0) + ref.decode(cur_c, 0))), cur_c, 0)
    assert np.array_equal(out[:, :12], both[:, :12])
    # mv.z carries the surface's own approach: 8 now, 6 before, is the same surface
    mv[..., 2] = -2.0
    six = np.full((h, w), 6.0, np.float32)
    out, fg = two_frames(shim, (prev_c, six, mv), (cur_c, far, mv))
    assert fg.trace["valid_b"].all()


def test_holes_copy_the_previous_frame(shim):
    rng = np.random.default_rng(7)
    w, h = 20, 10
    prev_c, cur_c = random_color(rng, w, h, 1), random_color(rng, w, h, 1)
    depth = np.full((h, w), 2.0, np.float32)
    mv = np.zeros((h, w, 3), np.float32)
    mv[:, 10:, 0] = 8.0  # the right half lands 4 pixels to the right: columns 10..13 are reached by nobody
    out, fg = two_frames(shim, (prev_c, depth, mv), (cur_c, depth, mv), fmt=1)
    hole = fg.trace["k"] == ref.HOLE
    assert hole[:, 10:14].all() and not hole[:, :10].any() and not hole[:, 14:].any()
    assert np.array_equal(out[hole], prev_c[hole])  # alpha too: bit for bit


def test_equal_depths_pick_the_lowest_index_and_contention_resolves_to_the_minimum_key(shim):
    w, h = 16, 8
    rng = np.random.default_rng(8)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    mv = np.zeros((h, w, 3), np.float32)
    mv[..., 0], mv[..., 1] = 2.0 * (5 - xs), 2.0 * (3 - ys)  # everyone onto (5, 3)
    color = random_color(rng, w, h, 0)
    depth = np.full((h, w), 4.0, np.float32)
    _, fg = two_frames(shim, (color, depth, mv), (color, depth, mv))
    field = fg.trace["field"]
    assert field[3, 5] == np.uint64(shim.fg_host_key(4.0, 0)) and (np.delete(field.ravel(), 3 * w + 5) == ref.HOLE).all()
    depth = rng.choice(np.array([1.0, 2.0, 4.0, np.inf], np.float32), (h, w))
    depth[0, 0] = 4.0
    _, fg = two_frames(shim, (color, depth, mv), (color, depth, mv))
    assert fg.trace["field"][3, 5] == ref.keys_of(depth).min() == ref.scatter(depth, mv)[3, 5]
    first_near = int(np.flatnonzero(depth.ravel() == 1.0)[0])
    assert int(fg.trace["field"][3, 5] & np.uint64(0xFFFFFFFF)) == first_near


def test_bad_vectors_scatter_nothing_and_bad_depths_count_as_infinite(shim):
    w, h = 12, 6
    rng = np.random.default_rng(9)
    color = random_color(rng, w, h, 0)
    depth = np.full((h, w), 2.0, np.float32)
    mv = np.zeros((h, w, 3), np.float32)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3.0e38]
    for i, v in enumerate(bad):
        mv[0, i, 0] = v
        mv[1, i, 1] = v
        mv[2, i, :2] = v
    _, fg = two_frames(shim, (color, depth, mv), (color, depth, mv))
    field = fg.trace["field"]
    assert (field[:3, :len(bad)] == ref.HOLE).all()
    rest = np.ones((h, w), bool)
    rest[:3, :len(bad)] = False
    assert np.array_equal((field & np.uint64(0xFFFFFFFF))[rest], np.arange(w * h, dtype=np.uint64).reshape(h, w)[rest])
    assert np.array_equal(field, ref.scatter(depth, mv))
    inf_bits = np.uint64(0x7F800000)
    for z in (np.nan, -1.0, -np.inf, np.inf, np.float32(-1e-30)):
        assert np.uint64(shim.fg_host_key(float(z), 7)) == (inf_bits << np.uint64(32)) | np.uint64(7), z
    assert shim.fg_host_key(-0.0, 7) == shim.fg_host_key(0.0, 7) == 7
    assert shim.fg_host_key(1.0, 7) == (0x3F800000 << 32) | 7
    # a pixel with a bad depth loses its target to any finite one
    depth[2, 7], depth[2, 8] = np.nan, -3.0
    mv[:] = 0.0
    mv[2, 9, 0], mv[2, 6, 0] = -4.0, 2.0  # (9, 2) -> (7, 2), (6, 2) -> (7, 2): the lower index of the two finite ones wins
    _, fg = two_frames(shim, (color, depth, mv), (color, depth, mv))
    assert int(fg.trace["field"][2, 7] & np.uint64(0xFFFFFFFF)) == 2 * w + 6
    assert int(fg.trace["field"][2, 8] >> np.uint64(32)) == 0x7F800000


@pytest.mark.parametrize("size", [(31, 7), (32, 8), (33, 9)])
def test_workgroup_tiles_equal_the_whole_image(shim, size):
    w, h = size
    rng = np.random.default_rng(w)
    a = random_frame(rng, w, h, w, h, 0)
    b = random_frame(rng, w, h, w, h, 0, a[1])
    whole, fw = two_frames(shim, a, b)
    tiled, ft = two_frames(shim, a, b, tiled=True)
    assert np.array_equal(whole, tiled) and np.array_equal(fw.trace["field"], ft.trace["field"])


def test_sanitizers_stand_alone(tmp_path):
    """tests/cpp/framegen_sanitize.cpp under ASan + UBSan as a plain executable"""
    exe = str(tmp_path / "framegen_sanitize")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    os.path.join(HERE, "cpp", "framegen_sanitize.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "framegen_sanitize ok" in res.stdout, res.stdout + res.stderr


def test_abi_validation_without_gpu(dxrs):
    from dxrs_amd.types import PtFrameGenSettings, PtFrameGenTextures
    lib = dxrs.load_hip().lib
    assert C.sizeof(PtFrameGenSettings) == 32 and C.sizeof(PtFrameGenTextures) == 32
    assert (PtFrameGenSettings.RenderSize.offset, PtFrameGenSettings.OutputSize.offset, PtFrameGenSettings.Format.offset,
            PtFrameGenSettings.Reset.offset, PtFrameGenSettings._pad.offset) == (0, 8, 16, 20, 24)
    assert [getattr(PtFrameGenTextures, n).offset for n in ("Color", "Depth", "MotionVector", "Output")] == [0, 8, 16, 24]
    s = PtFrameGenSettings(RenderSize=(C.c_uint32 * 2)(32, 32), OutputSize=(C.c_uint32 * 2)(64, 64))
    g = C.c_uint32(7)
    assert lib.pt_frame_gen(None, C.byref(s), C.byref(PtFrameGenTextures()), C.byref(g)) == 1
    assert lib.pt_frame_gen(None, None, None, None) == 1
    assert g.value == 7


# ------------------------------------------------------------------------------------------------------------------ GPU


def bits_equal(got, want, what=""):
    got, want = u32(got), u32(want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x}"


class GpuFrameGen:
    """pt_frame_gen on device copies; Output starts as the sentinel and sits between two guard bands that must stay the sentinel"""

    def __init__(self, renderer):
        self.r, self.generated = renderer, None

    def __call__(self, color, depth, mv, fmt=0, reset=False):
        import torch
        (h, w), (H, W) = np.asarray(depth).shape, np.asarray(color).shape
        d = [torch.from_numpy(u32(color).view(np.int32)).cuda(), torch.from_numpy(c32(depth)).cuda(), torch.from_numpy(c32(mv)).cuda()]
        out = torch.from_numpy(np.full(H * W + 2 * GUARD, SENTINEL, np.uint32).view(np.int32)).cuda()
        torch.cuda.synchronize()
        self.generated = self.r.frame_gen_device((w, h), (W, H), dict(Color=d[0].data_ptr(), Depth=d[1].data_ptr(), MotionVector=d[2].data_ptr(),
                                                                      Output=out.data_ptr() + 4 * GUARD), fmt=fmt, reset=reset)
        self.r.synchronize()
        res = out.cpu().numpy().view(np.uint32)
        assert (res[:GUARD] == SENTINEL).all() and (res[GUARD + H * W:] == SENTINEL).all(), "the guard band was written"
        return res[GUARD:GUARD + H * W].reshape(H, W)


def compare_sequence(renderer, shim, frames, what):
    """the frames (color, depth, mv, fmt, reset) through the GPU and the host header -> bit for bit, `generated` included"""
    gpu, host = GpuFrameGen(renderer), HostFrameGen(shim)
    flags = []
    for f, (color, depth, mv, fmt, reset) in enumerate(frames):
        reset = True if f == 0 else reset  # (the shared context carries other tests' history)
        got, want = gpu(color, depth, mv, fmt, reset), host(color, depth, mv, fmt, reset)
        assert gpu.generated == host.generated, f"{what} frame {f}: generated"
        bits_equal(got, want, f"{what} frame {f}")
        flags.append(host.generated)
    return flags


GPU_SHAPES = [((1, 1), (1, 1)), ((1, 7), (1, 7)), ((3, 2), (3, 2)), ((31, 7), (31, 7)), ((32, 8), (32, 8)), ((33, 9), (33, 9)), ((67, 45), (67, 45)),
              ((20, 12), (40, 24)), ((33, 9), (50, 14)), ((160, 90), (640, 360))]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("sizes", GPU_SHAPES)
def test_gpu_bit_exact_random_sequences(renderer, shim, sizes, fmt):
    """three consecutive calls: a restart and one generated frame from each history slot; a few vectors are huge or not finite"""
    (w, h), (W, H) = sizes
    rng = np.random.default_rng(w + 3 * h + 5 * W + fmt)
    frames, depth = [], None
    for f in range(3):
        color, depth, mv = random_frame(rng, w, h, W, H, fmt, depth)
        mv[..., :2] += rng.uniform(-0.01, 0.01, (h, w, 2)).astype(np.float32)  # off the 1/64 lattice: arbitrary fractions
        for value in (np.nan, np.inf, -1e30, 3.0e38):
            mv[rng.random((h, w)) < 0.01, rng.integers(0, 2)] = value
        depth = depth.copy()
        depth[rng.random((h, w)) < 0.02] = np.nan
        depth[rng.random((h, w)) < 0.02] = -1.0
        frames.append((color, depth, mv, fmt, False))
    assert compare_sequence(renderer, shim, frames, f"{w}x{h} -> {W}x{H}") == [False, True, True]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["one target", "equal depths"])
def test_gpu_contention(renderer, shim, kind):
    """64 x 64: every vector aimed at one pixel (4096 atomics on one address), and all depths equal (the index decides every min)"""
    w = h = 64
    rng = np.random.default_rng(11)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    frames = []
    for f in range(3):
        color, depth, mv = random_frame(rng, w, h, w, h, 0)
        if kind == "one target":
            mv[..., 0], mv[..., 1] = 2.0 * (37 - xs), 2.0 * (11 - ys)
        else:
            depth[:] = 2.0
        frames.append((color, depth, mv, 0, False))
    compare_sequence(renderer, shim, frames, kind)


@pytest.mark.gpu
def test_gpu_restart_rules(renderer, shim):
    """Reset, a Format change, an OutputSize change and a RenderSize change in the middle of a sequence restart the history"""
    rng = np.random.default_rng(12)
    plan = [((20, 12), (40, 24), 0, False), ((20, 12), (40, 24), 0, False), ((20, 12), (40, 24), 0, True), ((20, 12), (40, 24), 0, False),
            ((20, 12), (40, 24), 1, False), ((20, 12), (40, 24), 1, False), ((20, 12), (50, 30), 1, False), ((20, 12), (50, 30), 1, False),
            ((25, 15), (50, 30), 1, False), ((25, 15), (50, 30), 1, False), ((25, 15), (50, 30), 1, False)]
    frames = []
    for (w, h), (W, H), fmt, reset in plan:
        color, depth, mv = random_frame(rng, w, h, W, H, fmt)
        frames.append((color, depth, mv, fmt, reset))
    assert compare_sequence(renderer, shim, frames, "restart rules") == [False, True, False, True, False, True, False, True, False, True, True]


def render_chain(dxrs, host, r, f, spheres, prev_spheres, bufs, w, h):
    """frame f of the animated demo scene: pt_render_gbuffer (previous spheres) -> pt_render -> pt_tonemap into bufs"""
    r.update_spheres(spheres)
    r.set_camera(host.camera_matrices(w, h, position=(0.0, 0.0, -15.0), look_at=(0.0, 0.0, 0.0), jitter=False))
    r.set_constants(dxrs.types.graphics_settings(w, h, frame_index=f, bounces=8, spp=1))
    r.render_gbuffer_device(dict(LinearDepth=bufs["Depth"].data_ptr(), MotionVector=bufs["MotionVector"].data_ptr()), previous_spheres=prev_spheres)
    r.render_device(bufs["Radiance"].data_ptr())
    r.tonemap(bufs["Radiance"].data_ptr(), w * h, dxrs.types.tonemap_params(), bufs["Color"].data_ptr())


def animated_spheres(spheres, f):
    moved = spheres.copy()
    moved["cx"] += np.float32(0.3 * f) * np.cos(np.arange(len(spheres), dtype=np.float32))
    moved["cy"] += np.float32(0.2 * f) * np.sin(np.arange(len(spheres), dtype=np.float32))
    return moved


def make_bufs(torch, w, h):
    return dict(Radiance=torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), Depth=torch.zeros((h, w), dtype=torch.float32, device="cuda"),
                MotionVector=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"), Color=torch.zeros((h, w), dtype=torch.int32, device="cuda"),
                Output=torch.zeros((h, w), dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
def test_gpu_animated_chain_bit_exact(dxrs, host, renderer, shim):
    """two animated frames of a 96 x 64 scene: pt_render_gbuffer (previous spheres) -> pt_render -> pt_tonemap -> pt_frame_gen, against
    the host header on the downloaded inputs"""
    import torch
    w, h = 96, 64
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    sd.IsStatic = 0
    renderer.set_scene(spheres, mats, sd)
    bufs = make_bufs(torch, w, h)
    torch.cuda.synchronize()
    hf = HostFrameGen(shim)
    prev = spheres
    for f in range(3):
        moved = animated_spheres(spheres, f)
        render_chain(dxrs, host, renderer, f, moved, prev, bufs, w, h)
        generated = renderer.frame_gen_device((w, h), (w, h), {k: bufs[k].data_ptr() for k in ("Color", "Depth", "MotionVector", "Output")}, reset=f == 0)
        renderer.synchronize()
        color, depth, mv = (bufs[k].cpu().numpy() for k in ("Color", "Depth", "MotionVector"))
        want = hf(color.view(np.uint32), depth, mv, 0, reset=f == 0)
        assert generated == hf.generated == (f != 0)
        bits_equal(bufs["Output"].cpu().numpy().view(np.uint32), want, f"animated frame {f}")
        if f:
            assert np.abs(mv[np.isfinite(depth)][:, :2]).max() > 0.5 and not np.array_equal(want, color.view(np.uint32))
        prev = moved
    assert np.isinf(depth).any() and np.isfinite(depth).any()


@pytest.mark.gpu
def test_gpu_frames_in_flight(dxrs, host):
    """two lanes and four animated frames queued without waiting, each followed by pt_frame_gen: the rendered frames are bit-identical
    to frames rendered without pt_frame_gen, and the generated frames equal a one-lane run's that waits after every frame"""
    import torch
    spheres, mats, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    sd.IsStatic = 0
    w, h, frames = 96, 64, 4

    def run(r, lanes, generate):
        sets = [make_bufs(torch, w, h) for _ in range(2)]
        torch.cuda.synchronize()
        r.set_scene(spheres, mats, sd)
        got, prev = [], spheres
        for f in range(frames):
            s, moved = sets[f % 2], animated_spheres(spheres, f)
            render_chain(dxrs, host, r, f, moved, prev, s, w, h)
            prev = moved
            if generate:
                r.frame_gen_device((w, h), (w, h), {k: s[k].data_ptr() for k in ("Color", "Depth", "MotionVector", "Output")}, reset=f == 0)
            if lanes == 1 or f % 2 == 1:
                r.synchronize()
                got += [{k: v.cpu().numpy().copy() for k, v in x.items()} for x in (sets if lanes > 1 else [s])]
        r.synchronize()
        return got

    results = {}
    for name, lanes, generate in (("many", 2, True), ("plain", 2, False), ("one", 1, True)):
        tstream = torch.cuda.Stream()
        r = dxrs.Renderer(device=0, stream=tstream.cuda_stream, frames_in_flight=lanes)
        try:
            with torch.cuda.stream(tstream):
                results[name] = run(r, lanes, generate)
        finally:
            r.close()
    for f in range(frames):
        for k in ("Depth", "MotionVector", "Radiance", "Color"):
            assert np.array_equal(results["many"][f][k].view(np.uint32), results["plain"][f][k].view(np.uint32)), f"frame {f}: {k} with and without pt_frame_gen"
        bits_equal(results["many"][f]["Output"].view(np.uint32), results["one"][f]["Output"].view(np.uint32), f"frame {f}: Output, two lanes and one")
    assert not np.array_equal(results["one"][-1]["Output"], results["one"][-1]["Color"])


@pytest.mark.gpu
def test_gpu_error_codes(dxrs, renderer):
    from dxrs_amd.types import FRAME_GEN_TEXTURES, PtFrameGenSettings, PtFrameGenTextures
    import torch
    lib, ctx = renderer._lib, renderer._ctx
    w, h, W, H = 32, 16, 64, 32
    bufs = {k: torch.zeros(4 * w * 4 * h * 3 + 8, dtype=torch.float32, device="cuda") for k in FRAME_GEN_TEXTURES}  # (room for the 4x case)
    p = {k: b.data_ptr() for k, b in bufs.items()}
    g = C.c_uint32(7)

    def call(size_in=(w, h), size_out=(W, H), fmt=0, pad=(0, 0), **over):
        s = PtFrameGenSettings(RenderSize=(C.c_uint32 * 2)(*size_in), OutputSize=(C.c_uint32 * 2)(*size_out), Format=fmt, Reset=1, _pad=(C.c_uint32 * 2)(*pad))
        t = PtFrameGenTextures(**{name: C.c_void_p(over.get(name, p[name])) for name in FRAME_GEN_TEXTURES})
        return lib.pt_frame_gen(ctx, C.byref(s), C.byref(t), C.byref(g))

    s = PtFrameGenSettings(RenderSize=(C.c_uint32 * 2)(w, h), OutputSize=(C.c_uint32 * 2)(W, H))
    assert lib.pt_frame_gen(None, None, None, None) == 1
    assert lib.pt_frame_gen(ctx, None, C.byref(PtFrameGenTextures()), None) == 1 and lib.pt_frame_gen(ctx, C.byref(s), None, None) == 1
    for size_in in ((0, h), (w, 0), (16385, h), (w, 16385)):
        assert call(size_in=size_in, size_out=size_in) == 1, size_in
    for size_out in ((w - 1, H), (W, h - 1), (4 * w + 1, H), (W, 4 * h + 1), (0, 0)):
        assert call(size_out=size_out) == 1, size_out
    assert call(size_in=(8192, 1), size_out=(16385, 1)) == 1
    assert call(fmt=2) == 1 and call(fmt=0xFFFFFFFF) == 1
    assert call(pad=(1, 0)) == 1 and call(pad=(0, 1)) == 1
    for name in FRAME_GEN_TEXTURES:
        assert call(**{name: None}) == 1, name
        assert call(**{name: p[name] + 2}) == 1, name
    for name in ("Color", "Depth", "MotionVector"):
        assert call(Output=p[name]) == 1, name
    two = torch.zeros(2 * W * H, dtype=torch.float32, device="cuda")  # Color, then Output
    assert call(Color=two.data_ptr(), Output=two.data_ptr() + 4 * (W * H - 1)) == 1
    assert g.value == 7  # no refused call wrote it
    assert call(Color=two.data_ptr(), Output=two.data_ptr() + 4 * W * H) == 0 and g.value == 0
    assert call(size_out=(w, h)) == 0 and call(size_out=(4 * w, 4 * h)) == 0 and call(fmt=1) == 0
    assert call(Depth=p["MotionVector"]) == 0  # two inputs may share a buffer
    assert call(Depth=p["Depth"] + 4) == 0
    s.Reset = 0
    t = PtFrameGenTextures(**{name: C.c_void_p(p[name]) for name in FRAME_GEN_TEXTURES})
    assert lib.pt_frame_gen(ctx, C.byref(s), C.byref(t), None) == 0  # a null `generated` is allowed; the sizes changed: a restart
    assert lib.pt_frame_gen(ctx, C.byref(s), C.byref(t), C.byref(g)) == 0 and g.value == 1
    renderer.synchronize()


@pytest.mark.gpu
def test_gpu_cpp_host_mirror(dxrs, shim, tmp_path):
    """dxrs::FrameGeneration (host/FrameGeneration.hpp) from C++, against pt_api.h alone: three animated frames of the demo scene
    rendered, tone mapped, tagged and generated the way App::ProcessDLSSFrameGeneration tags them, equal the host-compiled header fed
    the inputs the program downloaded; a missing tag is refused"""
    exe = str(tmp_path / "host_framegen")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-I", os.path.join(PKG, "host"), os.path.join(HERE, "cpp", "host_framegen.cpp"),
                    "-o", exe, "-L", PKG, "-lpt_hip", f"-Wl,-rpath,{PKG}"], check=True)
    w, h, frames = 96, 64, 3
    outp = str(tmp_path / "fg.bin")
    res = subprocess.run([exe, str(w), str(h), str(frames), outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "expected error" in res.stdout
    raw = np.fromfile(outp, dtype=np.uint32)
    per = 1 + w * h * 6
    assert raw.size == frames * per
    hf = HostFrameGen(shim)
    for f in range(frames):
        x = raw[f * per:(f + 1) * per]
        n = w * h
        color, depth, mv, out = x[1:1 + n].reshape(h, w), x[1 + n:1 + 2 * n].view(np.float32).reshape(h, w), x[1 + 2 * n:1 + 5 * n].view(np.float32).reshape(h, w, 3), x[1 + 5 * n:]
        want = hf(color, depth, mv, 0)
        assert int(x[0]) == int(hf.generated) == int(f != 0)
        bits_equal(out.reshape(h, w), want, f"C++ frame {f}")
    assert not np.array_equal(want, color)
