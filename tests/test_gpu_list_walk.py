"""GPU: the record readers of the 1-spp primary pass (csrc/pt_trace.h: scalar_load, ListHead, closest_hit_list, refl_contains).  A wave
reads its block's primary-beam record and its region record with scalar loads -- the count and the first ids in one load, the later ids
and the candidates' spheres fetched ahead of their tests -- so the cases here are the smallest shapes at which such a reader can go wrong:
lists of 0, 1, exactly kBeamListCap and more entries, region lists of 1, exactly kReflListCap and more entries, the last block of the frame
(no read may pass the end of either buffer), a frame whose size is no multiple of 8, coincident spheres (the lower id wins), invisible and
alpha-tested entries in a textured scene, and a moving camera whose lists are built in shares and swapped.
Every frame is compared bit for bit, with equal ray counts, with the same frame of a context created with PT_BEAMS=0 PT_REFL_BEAMS=0
(every ray traverses) and with the CPU oracle.  The scenes are made from strings of small spheres along one block's pyramid (or along the
mirrored centre ray of a block on a mirror sphere); what their lists hold is computed on the CPU with the product's own pyramid and
region tests (tests/hostshim/beam_host.cpp, region_host.cpp) over the padded leaf boxes of pt_lbvh.cpp, and checked to be what each case
intends -- without a GPU too (test_scenes_hold_the_intended_lists)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import test_primary_beams as tpb
import test_refl_region as trr
from util import count_mismatch

BEAM_CAP, REFL_CAP = 15, 21  # kBeamListCap (pt_beam.h), kReflListCap (pt_region.h)
MASK = 1
SPHERE = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("r", "<f4")])  # (dxrs.SPHERE_DTYPE)


# ------------------------------------------------------------------------------------------------ what the lists hold, on the CPU
@functools.lru_cache(maxsize=None)
def beam_lib():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_beam_shim())
    lib.bm_make.argtypes = [tpb.F32P, tpb.U32, tpb.U32, tpb.U32, tpb.U32, tpb.F32, tpb.F32, tpb.F32P]
    lib.bm_meets_boxes.argtypes = [tpb.F32P, tpb.U32, tpb.F32P, tpb.U8P]
    lib.bm_meets_leaves.argtypes = [tpb.F32P, tpb.U32, tpb.F32P, tpb.U8P]
    lib.bm_rays.argtypes = [tpb.F32P, tpb.U32, tpb.U32, tpb.U32, tpb.U32P, tpb.F32P, tpb.F32P, tpb.F32P, tpb.F32P]
    for f in (lib.bm_make, lib.bm_meets_boxes, lib.bm_meets_leaves, lib.bm_rays):
        f.restype = None
    return lib


@functools.lru_cache(maxsize=None)
def region_lib():
    return trr.load_shim()


def cam12(cam):
    return np.array([*cam.Position, *cam.RightDirection, *cam.UpDirection, *cam.ForwardDirection], np.float32)


def ray_through(cam, w, h, x, y):
    """the camera ray through the image point (x, y) in pixels (a pixel's centre is at +0.5): float64 origin and unit direction"""
    px, py = int(math.floor(x)), int(math.floor(y))
    o, d = tpb.rays(beam_lib(), cam12(cam), w, h, [(px, py)], [(x - px - 0.5, y - py - 0.5)])
    return o[0].astype(np.float64), tpb.unit(d[0])


def centres(spheres):
    return np.stack([spheres["cx"], spheres["cy"], spheres["cz"]], 1).astype(np.float32)


def leaf_boxes(spheres, scale=1.0):
    """the padded cubes the tree builders put around the spheres (pt_lbvh.cpp); scale != 1: the cubes grown or shrunk about their centres"""
    c, r = centres(spheres), spheres["r"].astype(np.float32)[:, None]
    bmin, bmax = (c - r).min(0), (c + r).max(0)
    pad = np.float32(max(np.abs(bmin).max(), np.abs(bmax).max())) * np.float32(2.0 ** -17)
    if scale == 1.0:
        return np.concatenate([c - r - pad, c + r + pad], 1)
    he = (r + pad) * np.float32(scale)
    return np.concatenate([c - he, c + he], 1)


def beam_members(cam, w, h, spheres, block, scale=1.0):
    """which spheres the primary-beam list of `block` (bx, by) holds: the leaves beam_walk_block reaches"""
    g = tpb.make_beam(beam_lib(), cam12(cam), w, h, 8 * block[0], 8 * block[1], 0.0, 0.0)
    boxes = leaf_boxes(spheres, scale)
    return tpb.meets(beam_lib(), g, boxes) & tpb.meets(beam_lib(), g, boxes, leaf=True)


def block_region(cam, w, h, block, sphere):
    """the region record of a block whose five rays land on `sphere` (cx, cy, cz, r): 11 floats, or None"""
    x0, y0, x1, y1 = 8 * block[0] - 0.5, 8 * block[1] - 0.5, 8 * block[0] + 8.5, 8 * block[1] + 8.5
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (0.5 * (x0 + x1), 0.5 * (y0 + y1))]  # beam_corners' order, then the centre
    rays = [ray_through(cam, w, h, x, y) for x, y in pts]
    dirs = np.ascontiguousarray([d for _, d in rays], dtype=np.float32)
    g = np.zeros(11, np.float32)
    ok = region_lib().rg_from_rays(trr.fp(rays[0][0]), trr.fp(dirs), trr.fp(np.array(sphere[:3], np.float32)), C.c_float(sphere[3]), trr.fp(g))
    return g if ok else None


def region_members(g, spheres, scale=1.0):
    return trr.meets(region_lib(), g, leaf_boxes(spheres, scale))


def robust(members):
    """the same decisions with every leaf cube a quarter smaller and a quarter larger: none of them is a close call, so the device's
    arithmetic (its reciprocal square root, its trigonometry) decides them alike"""
    return np.array_equal(members(0.75), members(1.0)) and np.array_equal(members(1.0), members(1.25))


def string_along(o, d, n, t0, dt, radius):
    """n spheres along the ray: centres o + (t0 + k dt) d, radius(t)"""
    t = t0 + dt * np.arange(n)
    s = np.zeros(n, dtype=SPHERE)
    p = o[None, :] + t[:, None] * d[None, :]
    s["cx"], s["cy"], s["cz"] = p[:, 0], p[:, 1], p[:, 2]
    s["r"] = [radius(x) for x in t]
    return s


def pixel_angle(cam, w, h):
    _, a = ray_through(cam, w, h, 0.5 * w, 0.5 * h)
    _, b = ray_through(cam, w, h, 0.5 * w + 1.0, 0.5 * h)
    return float(np.linalg.norm(a - b))


def materials_for(dxrs, n, seed):
    rng = np.random.default_rng(seed)
    m = dxrs.types.default_material(n)
    m["BaseColor"][:, :3] = rng.uniform(0.2, 1.0, (n, 3))
    m["Metallic"] = rng.choice([0.0, 1.0, 0.4], n)
    m["Roughness"] = rng.choice([0.0, 0.05, 0.5], n)
    m["EmissiveStrength"] = 0.0
    emit = rng.random(n) < 0.25
    m["EmissiveStrength"][emit] = rng.uniform(1.0, 8.0, emit.sum())
    m["EmissiveColor"][emit] = rng.random((emit.sum(), 3))
    return m


def block_centre(w, h, block):
    """the middle of the part of the block that lies inside the image"""
    x0, y0 = 8 * block[0], 8 * block[1]
    return x0 + 0.5 * min(8, w - x0), y0 + 0.5 * min(8, h - y0)


def n_blocks(w, h):
    return (w + 7) // 8, (h + 7) // 8


# ------------------------------------------------------------------------------------------------ the scenes
def primary_scene(dxrs, host, w, h):
    """Strings of small spheres along the pyramids of four blocks: exactly the cap, one more than fits (the wave traverses), a single
    sphere, the cap again in the last block of the frame; two coincident spheres of different colours in a fifth; nothing elsewhere.
    -> (spheres, materials, camera, {name: block})"""
    cam = host.camera(w, h)
    bw, bh = n_blocks(w, h)
    blocks = {"full": (bw // 4, bh // 4), "over": (bw - 1 - bw // 4, bh // 4), "one": (bw // 2, bh // 2), "twins": (bw - 1 - bw // 4, bh - 1 - bh // 4),
              "last": (bw - 1, bh - 1)}
    assert len(set(blocks.values())) == 5
    ang = pixel_angle(cam, w, h)
    parts = []
    for name, n in (("full", BEAM_CAP), ("over", BEAM_CAP + 2), ("one", 1), ("last", BEAM_CAP)):
        o, d = ray_through(cam, w, h, *block_centre(w, h, blocks[name]))
        parts.append(string_along(o, d, n, 6.0, 1.1, lambda t: 0.8 * ang * t))
    o, d = ray_through(cam, w, h, *block_centre(w, h, blocks["twins"]))
    twin = string_along(o, d, 1, 8.0, 0.0, lambda t: 1.5 * ang * t)
    parts += [twin, twin.copy()]
    spheres = np.concatenate(parts)
    materials = materials_for(dxrs, len(spheres), 11)
    materials["BaseColor"][-2, :3], materials["BaseColor"][-1, :3] = (1.0, 0.1, 0.1), (0.1, 0.1, 1.0)  # the twins differ: the frame shows which one answered
    materials["Metallic"][-2:], materials["Roughness"][-2:], materials["EmissiveStrength"][-2:] = 0.0, 0.5, 0.0
    return spheres, materials, cam, blocks


def check_primary_scene(spheres, cam, w, h, blocks):
    counts = {}
    for name, b in blocks.items():
        assert robust(lambda s: beam_members(cam, w, h, spheres, b, s)), name
        counts[name] = int(beam_members(cam, w, h, spheres, b).sum())
    assert counts["full"] == BEAM_CAP and counts["last"] == BEAM_CAP and counts["over"] > BEAM_CAP and counts["one"] == 1 and counts["twins"] == 2, counts
    bw, bh = n_blocks(w, h)
    empty = sum(1 for by in range(bh) for bx in range(bw) if not beam_members(cam, w, h, spheres, (bx, by), 1.25).any())
    assert empty > bw * bh // 2, empty  # sky blocks: lists of no entry


MIRROR_T, MIRROR_R = 10.0, 2.5


def mirror_camera(host, w, h):
    """A long lens (a pixel of 0.16 degrees at either size): a block's footprint on the mirror is small against the mirror's radius, so its
    reflected rays fit a cone narrow enough for a region (pt_region.h kReflMaxTheta)."""
    return host.camera(w, h, hfov=math.radians(20.0 * w / 128.0))


def mirror_scene(dxrs, host, w, h, alpha=False):
    """A mirror sphere over the lower right of the image, the frame's last block included.  Strings of small spheres along the mirrored centre
    rays of three of its blocks: as many as make the region's list exactly its cap (the mirror itself is an entry), more than fit (no
    region), the cap again for the last block -- whose primary list is filled to its cap by a string behind the mirror.  alpha: the first
    two spheres of the first string are an invisible one (constant alpha below the cutoff) and an alpha-tested one (a base-colour map whose
    alpha is 0 on one half), and so are the first two of a string of five in front of a block off the mirror (a textured scene).
    -> (spheres, materials, textures or None, camera, {name: block})"""
    cam = mirror_camera(host, w, h)
    bw, bh = n_blocks(w, h)
    o, d = ray_through(cam, w, h, w - 19.0, h - 14.0)
    mc = o + MIRROR_T * d
    mirror = (float(mc[0]), float(mc[1]), float(mc[2]), MIRROR_R)
    blocks = {"full": (bw - 4, bh - 5), "over": (bw - 6, bh - 2), "last": (bw - 1, bh - 1), "front": (2, 2)}
    ang = pixel_angle(cam, w, h)
    s0 = np.zeros(1, dtype=dxrs.SPHERE_DTYPE)
    s0[0] = mirror
    parts = [s0]
    first = {}
    for name, n in (("full", REFL_CAP - 1), ("over", REFL_CAP + 3), ("last", REFL_CAP - 1)):
        g = block_region(cam, w, h, blocks[name], mirror)
        assert g is not None, name
        first[name] = sum(len(p) for p in parts)
        parts.append(string_along(0.5 * (g[0:3] + g[3:6]).astype(np.float64), tpb.unit(g[6:9]), n, 1.5, 0.22, lambda t: 0.04))
    o, d = ray_through(cam, w, h, *block_centre(w, h, blocks["last"]))
    parts.append(string_along(o, d, BEAM_CAP - 1, MIRROR_T + MIRROR_R + 2.0, 0.9, lambda t: 0.5 * ang * t))  # behind the mirror
    o, d = ray_through(cam, w, h, *block_centre(w, h, blocks["front"]))
    first["front"] = sum(len(p) for p in parts)
    parts.append(string_along(o, d, 5, 6.0, 1.1, lambda t: 1.6 * ang * t))
    spheres = np.concatenate(parts)
    materials = materials_for(dxrs, len(spheres), 23)
    materials["BaseColor"][0, :3] = (0.9, 0.85, 0.8)
    materials["Metallic"][0], materials["Roughness"][0], materials["Transmission"][0], materials["EmissiveStrength"][0] = 1.0, 0.0, 0.0, 0.0
    textures = None
    if alpha:
        from dxrs_amd import textures as T
        textures = T.TextureSet(len(spheres))
        img = np.full((4, 64, 4), 255, np.uint8)
        img[:, :32, 3] = 0
        half = textures.add_image(img)
        for name in ("full", "front"):
            k = first[name]
            materials["AlphaMode"][k], materials["BaseColor"][k, 3], materials["AlphaCutoff"][k] = MASK, 0.2, 0.5      # invisible
            materials["AlphaMode"][k + 1], materials["BaseColor"][k + 1, 3], materials["AlphaCutoff"][k + 1] = MASK, 1.0, 0.5  # tested per crossing
            textures.assign(k + 1, dxrs.types.TEXTURE_MAP_BASE_COLOR, half)
    return spheres, materials, textures, cam, blocks


def check_mirror_scene(spheres, cam, w, h, blocks):
    mirror = tuple(float(x) for x in spheres[0])
    c = centres(spheres).astype(np.float64)
    o = np.array(cam.Position, np.float64)
    counts = {}
    for name in ("full", "over", "last"):
        b = blocks[name]
        assert robust(lambda s: beam_members(cam, w, h, spheres, b, s)), name
        prim = beam_members(cam, w, h, spheres, b)
        # the block's five rays land on the mirror: it is in the list, and every other entry lies behind it
        assert prim[0] and 1 <= prim.sum() <= BEAM_CAP, (name, prim.sum())
        assert (np.linalg.norm(c[prim][1:] - o, axis=1) > MIRROR_T + MIRROR_R).all(), name
        g = block_region(cam, w, h, b, mirror)
        assert g is not None, name
        if name == "over":  # (which spheres overflow the list does not matter: more than fit, even with every leaf cube a quarter smaller)
            counts[name] = int(region_members(g, spheres, 0.75).sum())
        else:
            assert robust(lambda s: region_members(g, spheres, s)), name
            counts[name] = int(region_members(g, spheres).sum())
    assert counts["full"] == REFL_CAP and counts["last"] == REFL_CAP and counts["over"] > REFL_CAP, counts
    assert int(beam_members(cam, w, h, spheres, blocks["last"]).sum()) == BEAM_CAP
    # some block of the mirror sees nothing but the mirror itself: a region list of one entry
    bw, bh = n_blocks(w, h)
    ones = 0
    for by in range(1, bh):
        for bx in range(1, bw):
            prim = beam_members(cam, w, h, spheres, (bx, by))
            g = block_region(cam, w, h, (bx, by), mirror) if prim[0] and prim.sum() == 1 else None
            if g is not None and robust(lambda s: region_members(g, spheres, s)) and region_members(g, spheres).sum() == 1:
                ones += 1
    assert ones >= 1
    front = beam_members(cam, w, h, spheres, blocks["front"])  # (the string of five is the scene's last part; the mirror may lie behind it)
    assert beam_members(cam, w, h, spheres, blocks["front"], 0.75)[-5:].all() and front[-5:].all() and front.sum() <= 6


SIZES = [(128, 72), (70, 42)]


@pytest.mark.parametrize("w,h", SIZES)
def test_scenes_hold_the_intended_lists(dxrs, host, w, h):
    """CPU: the scenes of the GPU cases below put into the lists what the cases are about"""
    spheres, _, cam, blocks = primary_scene(dxrs, host, w, h)
    check_primary_scene(spheres, cam, w, h, blocks)
    spheres, _, _, cam, blocks = mirror_scene(dxrs, host, w, h)
    check_mirror_scene(spheres, cam, w, h, blocks)


# ------------------------------------------------------------------------------------------------ the frames
@pytest.fixture(scope="module")
def renderer_plain(dxrs):
    """A context created with PT_BEAMS=0 PT_REFL_BEAMS=0 (the knobs are read once, at pt_create): every ray traverses the tree."""
    old = {k: os.environ.get(k) for k in ("PT_BEAMS", "PT_REFL_BEAMS")}
    os.environ["PT_BEAMS"] = os.environ["PT_REFL_BEAMS"] = "0"
    try:
        r = dxrs.Renderer(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield r
    r.close()


def rested_frame(r, scene, cam, gs, textures=None):
    """the third frame of a view: its primaries come from the beam lists, its bounce-1 rays from the region lists where there are any
    -> (image, stats, bounce-1 waves, waves served by a region list)"""
    r.set_scene(*scene)
    r.set_textures(textures)
    r.set_camera(cam)
    r.set_constants(gs)
    r.render()
    r.render()
    r.refl_stats(reset=True)
    img, st = r.render()
    waves, listed = r.refl_stats(reset=True)
    return img, st, waves, listed


def compare(dxrs, host, oracle, renderer, renderer_plain, spheres, materials, cam, w, h, textures=None, expect_regions=False, di=False):
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    gs = dxrs.types.graphics_settings(w, h, frame_index=5, bounces=4, spp=1, di=di)
    try:
        img, st, waves, listed = rested_frame(renderer, (spheres, materials, sd), cam, gs, textures)
        img0, st0, _, listed0 = rested_frame(renderer_plain, (spheres, materials, sd), cam, gs, textures)
    finally:
        renderer.set_textures(None)
        renderer_plain.set_textures(None)
    ref, ost = oracle.render(spheres, materials, sd, cam, gs, threads=8, textures=textures)
    assert st.beams_used and not st0.beams_used and listed0 == 0
    assert st.rays == st0.rays == ost.rays
    assert count_mismatch(img, img0) == 0
    assert count_mismatch(img, ref) == 0
    if expect_regions:
        assert listed > 0, (waves, listed)
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_primary_lists_empty_single_full_and_overflowing(dxrs, host, oracle, renderer, renderer_plain, w, h):
    spheres, materials, cam, blocks = primary_scene(dxrs, host, w, h)
    check_primary_scene(spheres, cam, w, h, blocks)
    img = compare(dxrs, host, oracle, renderer, renderer_plain, spheres, materials, cam, w, h)
    # the coincident twins (the scene's last two spheres, of different colours): the lower id answers wherever the pair is met, so the frame
    # is that of the scene without the higher twin, and not that of the scene without the lower one
    sd = host.scene(dxrs.host.SCENE_SMALL)[2]
    gs = dxrs.types.graphics_settings(w, h, frame_index=5, bounces=4, spp=1)
    n = len(spheres)
    lower, _ = oracle.render(spheres[:-1], materials[:-1], sd, cam, gs, threads=8)
    keep = np.r_[0:n - 2, n - 1]
    higher, _ = oracle.render(spheres[keep], materials[keep], sd, cam, gs, threads=8)
    assert count_mismatch(img, lower) == 0 and count_mismatch(img, higher) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("di", [False, True])
def test_region_lists_single_full_and_overflowing(dxrs, host, oracle, renderer, renderer_plain, w, h, di):
    spheres, materials, _, cam, blocks = mirror_scene(dxrs, host, w, h)
    check_mirror_scene(spheres, cam, w, h, blocks)
    compare(dxrs, host, oracle, renderer, renderer_plain, spheres, materials, cam, w, h, expect_regions=True, di=di)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_invisible_and_alpha_tested_entries_in_a_textured_scene(dxrs, host, oracle, renderer, renderer_plain, w, h):
    spheres, materials, textures, cam, blocks = mirror_scene(dxrs, host, w, h, alpha=True)
    check_mirror_scene(spheres, cam, w, h, blocks)  # (the lists hold the spheres whatever their alpha class)
    compare(dxrs, host, oracle, renderer, renderer_plain, spheres, materials, cam, w, h, textures=textures, expect_regions=True)


@pytest.mark.gpu
def test_moving_camera_through_a_swap_of_share_built_lists(dxrs, host, renderer_plain):
    """Three frames in flight over a camera in steady travel: the lists are built in shares inside the frames' primary passes, into the buffer
    no frame reads, and swapped in when every share's frame has finished.  The first lists are made for 32 frames (PT_BEAM_REACH), so frames
    from the 44th on that use lists use a later build's: a swap lies behind them.  Every frame equals the per-ray traversal's."""
    torch = pytest.importorskip("torch")
    spheres, materials, sd = host.scene(dxrs.host.SCENE_DEMO, seed=0)
    w, h, n, late = 256, 144, 56, 44
    gs = dxrs.types.graphics_settings(w, h, frame_index=0, bounces=3, spp=1)
    cams = [host.camera(w, h, position=(0.004 * k, 0.0, -15.0 + 0.003 * k), jitter_index=k % 8) for k in range(n)]
    out = {}
    r3 = dxrs.Renderer(device=0, frames_in_flight=3)
    try:
        for name, r in (("lists", r3), ("plain", renderer_plain)):
            r.set_scene(spheres, materials, sd)
            bufs = [torch.empty((h * w, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]
            used, rays = [], 0
            for lo, hi in ((0, late), (late, n)):
                r.totals(reset=True)
                for k in range(lo, hi):
                    gs.FrameIndex = k
                    r.set_constants(gs); r.set_camera(cams[k])
                    r.render_device(bufs[k].data_ptr())
                r.synchronize()
                tot = r.totals(reset=True)
                used.append(int(tot.beams_used))
                rays += int(tot.rays)
            out[name] = ([b.cpu().numpy().view(np.uint32) for b in bufs], rays, used)
    finally:
        r3.close()
    assert out["plain"][2] == [0, 0]
    assert out["lists"][2][0] > late // 2 and out["lists"][2][1] > 0, out["lists"][2]
    assert out["lists"][1] == out["plain"][1]
    for k in range(n):
        assert np.array_equal(out["lists"][0][k], out["plain"][0][k]), k
