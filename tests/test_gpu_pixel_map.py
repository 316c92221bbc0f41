"""GPU: the slot -> pixel mapping in its device build, and frames that depend on it.
- tests/hostshim/pixmap_gpu.hip (hipcc, the product's flags) evaluates block_origin on a wave-uniform block index + block_pixel, and the per-lane
  slot_to_pixel, for the maps of pixel_map_cases.py; every slot's {px, py, out_index, valid} equals the plain-integer restatement.
- Frames through the C-ABI (demo scene, 1 spp, 8 bounces, a resting view rendered three times so that the beam lists are in use, and once more
  in a context made with PT_BEAMS=0): pt_render on 70x42, 9x9 and a sub-rect of 64x48; pt_render_tiles with 8-pixel tiles under the partition
  (2, 3, 7) and the two partitions that own the rest, un-swizzled by pt_unpack_tiles_ex.  Each is bit-identical to the oracle's frame, with
  equal ray counts."""
import ctypes as C
import os

import numpy as np
import pytest

from pixel_map_cases import MAPS, expected, n_slots, slots_of
from util import bits, count_mismatch, render_rested

pytestmark = pytest.mark.gpu

FRAMES = {"70x42": (70, 42, None), "9x9": (9, 9, None), "subrect_64x48": (64, 48, (3, 5, 21, 13))}
PARTS = ((2, 3, 7), (0, 2, 7), (5, 2, 7))  # the issue's partition first; together the three own every residue of 7
TS = 8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    so = C.CDLL(g.build_pixmap_gpu())
    so.pix_gpu_map.restype = C.c_int
    so.pix_gpu_map.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
    return so


@pytest.mark.parametrize("name", [n for n in MAPS if n_slots(MAPS[n]) > 0])
@pytest.mark.parametrize("form", [0, 1], ids=["block_origin", "slot_to_pixel"])
def test_device_mapping_equals_the_plain_integer_restatement(lib, name, form):
    desc = np.array(MAPS[name], np.uint32)
    slots = slots_of(name)
    got = np.full((len(slots), 4), 0xFFFFFFFF, np.uint32)
    assert lib.pix_gpu_map(desc.ctypes.data, len(slots), slots.ctypes.data, got.ctypes.data, form) == 0
    want = expected(MAPS[name], slots)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} slots differ, the first is slot {int(slots[bad[0]])}: got {got[bad[0]]}, want {want[bad[0]]}"


@pytest.fixture(scope="module")
def scene(dxrs, host):
    return host.scene(dxrs.host.SCENE_DEMO, seed=0)


def view(dxrs, host, w, h):
    return host.camera(w, h), dxrs.types.graphics_settings(w, h, frame_index=0, bounces=8, spp=1)


@pytest.fixture(scope="module")
def references(dxrs, host, oracle, scene):
    """the oracle's frames, made once: name -> (image, stats)"""
    out = {}
    for name, (w, h, rect) in FRAMES.items():
        cam, gs = view(dxrs, host, w, h)
        out[name] = oracle.render(*scene, cam, gs, rect=rect, threads=8)
    return out


@pytest.fixture(scope="module")
def tile_renderers(dxrs):
    """contexts with 8-pixel tiles: the default one and one made with PT_BEAMS=0 (the knobs are read once, at pt_create)"""
    a = dxrs.Renderer(device=0, tile_size=TS)
    old = os.environ.get("PT_BEAMS")
    os.environ["PT_BEAMS"] = "0"
    try:
        b = dxrs.Renderer(device=0, tile_size=TS)
    finally:
        if old is None:
            os.environ.pop("PT_BEAMS", None)
        else:
            os.environ["PT_BEAMS"] = old
    yield {"beams": a, "no_beams": b}
    a.close()
    b.close()


@pytest.mark.parametrize("name", list(FRAMES))
def test_rect_frames_match_the_oracle(dxrs, host, scene, references, renderer, renderer_no_beams, name):
    w, h, rect = FRAMES[name]
    cam, gs = view(dxrs, host, w, h)
    ref, ostats = references[name]
    for r, beams in ((renderer, True), (renderer_no_beams, False)):
        r.set_scene(*scene); r.set_camera(cam); r.set_constants(gs)
        if beams:
            img, st = render_rested(r, rect)
        else:
            img, st = r.render(rect)
            assert st.beams_used == 0
        assert img.shape == ref.shape
        assert st.rays == ostats.rays, (name, beams)
        assert count_mismatch(img, ref) == 0, (name, beams)


@pytest.mark.parametrize("which", ["beams", "no_beams"])
def test_tile_frames_match_the_oracle(dxrs, host, scene, references, tile_renderers, which):
    import torch
    from dxrs_amd import tiles

    w, h, _ = FRAMES["70x42"]
    cam, gs = view(dxrs, host, w, h)
    ref, ostats = references["70x42"]
    r = tile_renderers[which]
    r.set_scene(*scene); r.set_camera(cam); r.set_constants(gs)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rays = 0
    try:
        for first, run, stride in PARTS:
            r.set_partition_ex(first, run, stride)
            n_tiles = tiles.range_tiles_count(w, h, first, run, stride, ts=TS)
            want = tiles.pack_range(ref, first, run, stride, ts=TS)
            assert want.shape[0] == n_tiles > 0
            packed = torch.full((n_tiles * TS * TS, 4), float("nan"), dtype=torch.float32, device="cuda")
            got = []
            for _ in range(3 if which == "beams" else 1):  # (a resting view: the third frame takes its candidates from the beam lists)
                st = r.render_tiles(packed.data_ptr(), want_stats=True)
                torch.cuda.synchronize()
                got.append((packed.cpu().numpy().reshape(want.shape).copy(), st.rays))
            for g, n in got:
                assert n == got[0][1] and np.array_equal(bits(g), bits(got[0][0]))
            assert np.array_equal(bits(got[-1][0])[..., :3], bits(want)[..., :3]), (first, run, stride)
            rays += got[-1][1]
            r.unpack_tiles_ex(packed.data_ptr(), n_tiles * TS * TS, 1, first, run, stride, frame.data_ptr())
        torch.cuda.synchronize()
    finally:
        r.set_partition_ex(0, 1, 1)
    assert rays == ostats.rays
    assert count_mismatch(frame.cpu().numpy(), ref) == 0
