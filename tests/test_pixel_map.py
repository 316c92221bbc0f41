"""CPU: the slot -> pixel mapping of the primary pass (csrc/pt_pixel_map.h) and its exact division by multiply-high (csrc/pt_magic_div.h),
compiled as host C++ (tests/hostshim/pixmap_host.cpp).
- The pair {mul, shift} that make_magic_div returns gives n / d: exhaustively below 2^26 for a list of divisors, and for every d <= 4096 over
  the small n, the neighbours of multiples of d, and the top of the range.
- block_origin + block_pixel (the primary pass: one origin per 8x8 block) and the per-lane slot_to_pixel both equal a restatement of the
  mapping in plain integers with // and %, written here, for every slot of rect maps, a sub-rect, a 16384 x 16384 rect (sampled), tile maps
  under three partitions and a partition that owns no tile.
- A stand-alone program over the same headers, built with ASan + UBSan, runs clean."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from pixel_map_cases import MAPS, expected, n_slots, slots_of


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    so = C.CDLL(g.build_pixmap_shim())
    vp, u32 = C.c_void_p, C.c_uint32
    for name, res, args in (("pix_host_pair", None, [u32, vp]), ("pix_host_div_range", C.c_uint64, [u32, u32, u32, vp]),
                            ("pix_host_div_list", C.c_uint64, [u32, u32, vp, vp]), ("pix_host_n_slots", u32, [vp]),
                            ("pix_host_map", None, [vp, u32, vp, vp, C.c_int])):
        getattr(so, name).restype = res
        getattr(so, name).argtypes = args
    return so


def pair(lib, d):
    out = np.zeros(2, np.uint32)
    lib.pix_host_pair(d, out.ctypes.data)
    return int(out[0]), int(out[1])


def test_the_pair_has_the_stated_form(lib):
    """powers of two (1 included) are a pure shift (mul = 0); every other divisor has 2^shift < d < 2^(shift + 1) and mul = ceil(2^(32 + shift) / d),
    which fits 32 bits and satisfies the inequality of the proof below 2^31"""
    for d in list(range(1, 4098)) + [65535, 65536, 65537, 2 ** 25 - 1, 2 ** 26 - 1, 2 ** 26, 2 ** 31 - 1]:
        mul, shift = pair(lib, d)
        if d & (d - 1) == 0:
            assert mul == 0 and 1 << shift == d, d
            continue
        assert (1 << shift) < d < (2 << shift), d
        k = 32 + shift
        assert mul == -(-(1 << k) // d) and mul < 2 ** 32, d
        e = mul * d - (1 << k)
        assert 0 <= e < d and (2 ** 31 - 1) * e < (1 << k), d


@pytest.mark.parametrize("d", [1, 2, 3, 5, 7, 8, 9, 129, 240, 241, 255, 256, 257, 4095, 4096, 4097, 65535, 2 ** 25 - 1, 2 ** 26 - 1])
def test_exact_for_every_n_below_2_26(lib, d):
    first = C.c_uint32(0)
    bad = lib.pix_host_div_range(d, 0, 1 << 26, C.byref(first))
    assert bad == 0, f"d = {d}: {bad} quotients differ from n // d, the first at n = {first.value}"


def test_every_divisor_up_to_4096(lib):
    """n in 0 .. 2^16, the neighbours k d - 1, k d, k d + 1 of 1000 random multiples, and the top 2^16 values below 2^26"""
    rng = np.random.default_rng(7)
    first = C.c_uint32(0)
    for d in range(1, 4097):
        assert lib.pix_host_div_range(d, 0, (1 << 16) + 1, C.byref(first)) == 0, (d, first.value)
        assert lib.pix_host_div_range(d, (1 << 26) - (1 << 16), 1 << 26, C.byref(first)) == 0, (d, first.value)
        k = rng.integers(1, (1 << 26) // d + 1, size=1000, dtype=np.int64) * d
        n = np.concatenate([k - 1, k, k + 1])
        n = np.ascontiguousarray(n[(n >= 0) & (n < (1 << 26))].astype(np.uint32))
        assert len(n) >= 2000
        assert lib.pix_host_div_list(d, len(n), n.ctypes.data, C.byref(first)) == 0, (d, first.value)


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("form", [0, 1], ids=["block_origin", "slot_to_pixel"])
def test_mapping_equals_the_plain_integer_restatement(lib, name, form):
    desc = np.array(MAPS[name], np.uint32)
    assert lib.pix_host_n_slots(desc.ctypes.data) == n_slots(MAPS[name])
    slots = slots_of(name)
    if len(slots) == 0:
        assert n_slots(MAPS[name]) == 0  # the partition that owns no tile: the host side launches nothing
        return
    got = np.zeros((len(slots), 4), np.uint32)
    lib.pix_host_map(desc.ctypes.data, len(slots), slots.ctypes.data, got.ctypes.data, form)
    want = expected(MAPS[name], slots)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} slots differ, the first is slot {int(slots[bad[0]])}: got {got[bad[0]]}, want {want[bad[0]]}"
    # every pixel of a rect is the valid image of exactly one slot when all slots were visited
    if MAPS[name][0] == 0 and len(slots) == n_slots(MAPS[name]):
        _, _, _, rx, ry, rw, rh = MAPS[name]
        v = got[got[:, 3] == 1]
        assert len(v) == rw * rh and len(np.unique(v[:, 2])) == rw * rh and int(v[:, 2].max()) == rw * rh - 1


def test_sanitizer_program_runs_clean(tmp_path):
    import __graft_entry__ as g

    exe = g.build_pixmap_sanitizer(str(tmp_path))
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok"), res.stdout
