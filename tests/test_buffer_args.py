"""The buffer-argument rule of the C-ABI passes (csrc/pt_args.h check_buffers), on the CPU: the header is compiled as host C++
(tests/hostshim/args_host.cpp) and compared with a brute-force restatement over integer intervals.  Addresses are only numbers: no
memory is touched.  The rule: every required pointer present, every pointer aligned to its channel width (both in table order), then
no written buffer sharing a byte with any other buffer of the call (written entries in table order, each against the others in table
order); the message names the first violation.  The GPU error-code tests of the passes check the same messages through the entry points."""
import ctypes as C

import numpy as np
import pytest

N = 5 * 3  # the pixels of a 5 x 3 image
N_OUT = 10 * 6  # ... and of its 10 x 6 output (pt_upscale, pt_frame_gen)


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_args_shim())
    lib.args_host_check.restype = C.c_uint32
    lib.args_host_check.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    return lib


def check(shim, who, table):
    """check_buffers over table = [(addr, bytes, align, written, required, name)] -> the message ("" = acceptable)"""
    n = len(table)
    addr = np.array([t[0] for t in table], np.uint64)
    size = np.array([t[1] for t in table], np.uint64)
    align = np.array([t[2] for t in table], np.uint32)
    written = np.array([t[3] for t in table], np.uint8)
    required = np.array([t[4] for t in table], np.uint8)
    names = (C.c_char_p * n)(*[t[5].encode() for t in table])
    msg = C.create_string_buffer(256)
    length = shim.args_host_check(who.encode(), n, addr.ctypes.data, size.ctypes.data, align.ctypes.data, written.ctypes.data, required.ctypes.data,
                                  names, msg, len(msg))
    assert length < len(msg)
    return msg.value.decode()


def brute(who, table):
    """the rule restated: Python integers, the bytes of a buffer as the interval [addr, addr + bytes); address 0 = a null pointer"""
    for addr, size, align, written, required, name in table:
        if addr == 0:
            if required:
                return f"{who}: {name} is required"
        elif addr % align:
            return f"{who}: {name} is not {align}-byte aligned"
    for i, a in enumerate(table):
        if a[0] == 0 or not a[3]:
            continue
        for j, b in enumerate(table):
            if j == i or b[0] == 0:
                continue
            if max(a[0], b[0]) < min(a[0] + a[1], b[0] + b[1]):  # a common byte
                return f"{who}: {a[5]} overlaps {b[5]}"
    return ""


# the tables of the six entry points as they build them: (name, bytes, alignment, written, required)
REAL_TABLES = {
    "pt_nrd_composition(pack, ReBLUR)": ("pt_nrd_composition", [
        ("LinearDepth", N * 4, 4, 0, 1), ("DiffuseAlbedo", N * 12, 4, 0, 1), ("SpecularAlbedo", N * 12, 4, 0, 1), ("NormalRoughness", N * 16, 16, 0, 1),
        ("NoisyDiffuse", N * 16, 16, 1, 1), ("NoisySpecular", N * 16, 16, 1, 1)]),
    "pt_nrd_composition(pack, ReLAX)": ("pt_nrd_composition", [
        ("LinearDepth", N * 4, 4, 0, 1), ("DiffuseAlbedo", N * 12, 4, 0, 1), ("SpecularAlbedo", N * 12, 4, 0, 1),
        ("NoisyDiffuse", N * 16, 16, 1, 1), ("NoisySpecular", N * 16, 16, 1, 1)]),
    "pt_nrd_composition(compose)": ("pt_nrd_composition", [
        ("LinearDepth", N * 4, 4, 0, 1), ("DiffuseAlbedo", N * 12, 4, 0, 1), ("SpecularAlbedo", N * 12, 4, 0, 1),
        ("DenoisedDiffuse", N * 16, 16, 0, 1), ("DenoisedSpecular", N * 16, 16, 0, 1), ("Radiance", N * 16, 16, 1, 1)]),
    "pt_nrd_denoise": ("pt_nrd_denoise", [
        ("ViewZ", N * 4, 4, 0, 1), ("MotionVector", N * 12, 4, 0, 1), ("NormalRoughness", N * 16, 16, 0, 1), ("BaseColorMetalness", N * 16, 16, 0, 0),
        ("InDiffuse", N * 16, 16, 0, 1), ("InSpecular", N * 16, 16, 0, 1), ("OutDiffuse", N * 16, 16, 1, 1), ("OutSpecular", N * 16, 16, 1, 1)]),
    "pt_upscale": ("pt_upscale", [
        ("Color", N * 16, 16, 0, 1), ("Depth", N * 4, 4, 0, 1), ("Velocity", N * 12, 4, 0, 1), ("Output", N_OUT * 16, 16, 1, 1)]),
    "pt_nis_sharpen": ("pt_nis_sharpen", [("Color", N * 16, 16, 0, 1), ("Output", N * 16, 16, 1, 1)]),
    "pt_frame_gen": ("pt_frame_gen", [
        ("Color", N_OUT * 4, 4, 0, 1), ("Depth", N * 4, 4, 0, 1), ("MotionVector", N * 12, 4, 0, 1), ("Output", N_OUT * 4, 4, 1, 1)]),
    "pt_restir_di": ("pt_restir_di", [
        ("Position", N * 16, 16, 0, 1), ("GeometricNormal", N * 8, 8, 0, 1), ("LinearDepth", N * 4, 4, 0, 1), ("MotionVector", N * 12, 4, 0, 1),
        ("BaseColorMetalness", N * 16, 16, 0, 1), ("NormalRoughness", N * 16, 16, 0, 1), ("IOR", N * 4, 4, 0, 1), ("Transmission", N * 4, 4, 0, 1),
        ("Diffuse", N * 16, 16, 1, 1), ("Specular", N * 16, 16, 1, 1)]),
}


def packed(entries, base=0x7F0000001000):
    """the entries placed back to back from base (every size here is a multiple of 4, and of 16 where the alignment is): touching, disjoint"""
    table, addr = [], base
    for name, size, align, written, required in entries:
        addr = (addr + align - 1) // align * align
        table.append((addr, size, align, written, required, name))
        addr += size
    return table


@pytest.mark.parametrize("case", list(REAL_TABLES))
def test_real_tables(shim, case):
    who, entries = REAL_TABLES[case]
    good = packed(entries)
    assert check(shim, who, good) == brute(who, good) == ""

    def both(t):
        got = check(shim, who, t)
        assert got == brute(who, t)
        return got

    for i, row in enumerate(good):
        addr, size, align, written, required, name = row
        moved = lambda a: good[:i] + [(a,) + row[1:]] + good[i + 1:]  # noqa: E731
        assert both(moved(0)) == (f"{who}: {name} is required" if required else "")
        for off in (1, align // 2):
            assert both(moved(addr + off)) == f"{who}: {name} is not {align}-byte aligned"
        for j, other in enumerate(good):
            if j == i:
                continue
            # onto the other's first bytes and onto its last byte (aligned: every buffer here is longer than 16 bytes) ...
            for a in (other[0] // align * align, (other[0] + other[1] - 1) // align * align):
                got = both(moved(a))
                if written or other[3]:
                    assert " overlaps " in got, (name, other[5], got)
            # ... and ending at or just before its first byte
            both(moved((other[0] - size) // align * align))


def test_message_text(shim):
    """the wording itself (the restatement above would follow a change of it): what the passes' GPU error-code tests match"""
    who, entries = REAL_TABLES["pt_nis_sharpen"]
    color, output = packed(entries)
    assert check(shim, who, [color, (color[0],) + output[1:]]) == "pt_nis_sharpen: Output overlaps Color"
    assert check(shim, who, [(0,) + color[1:], output]) == "pt_nis_sharpen: Color is required"
    assert check(shim, who, [(color[0] + 4,) + color[1:], output]) == "pt_nis_sharpen: Color is not 16-byte aligned"
    assert check(shim, who, [color, (0,) + output[1:]]) == "pt_nis_sharpen: Output is required"


def test_edges(shim):
    A = 0x10000
    def both(t):
        got = check(shim, "p", t)
        assert got == brute("p", t)
        return got
    # touching ranges, and ranges sharing one byte, on either side
    assert both([(A, 64, 4, 1, 1, "out"), (A + 64, 64, 4, 0, 1, "in")]) == ""
    assert both([(A + 64, 64, 4, 1, 1, "out"), (A, 64, 4, 0, 1, "in")]) == ""
    assert both([(A, 65, 4, 1, 1, "out"), (A + 64, 64, 4, 0, 1, "in")]) == "p: out overlaps in"
    assert both([(A + 64, 64, 4, 1, 1, "out"), (A, 65, 4, 0, 1, "in")]) == "p: out overlaps in"
    # an entry contained inside another, either way round
    assert both([(A, 256, 4, 0, 1, "in"), (A + 64, 16, 4, 1, 1, "out")]) == "p: out overlaps in"
    assert both([(A, 256, 4, 1, 1, "out"), (A + 64, 16, 4, 0, 1, "in")]) == "p: out overlaps in"
    # a null optional entry between two overlapping ones: skipped in both roles, whatever its other fields say
    assert both([(A, 64, 4, 0, 1, "in"), (0, 1 << 40, 4, 1, 0, "opt"), (A + 32, 64, 4, 1, 1, "out")]) == "p: out overlaps in"
    assert both([(A, 64, 4, 0, 1, "in"), (0, 1 << 40, 4, 1, 0, "opt"), (A + 64, 64, 4, 1, 1, "out")]) == ""
    # a missing required entry listed after a misaligned one: the misaligned one is reported; the other way round, the missing one
    assert both([(A + 2, 64, 4, 0, 1, "first"), (0, 64, 4, 0, 1, "second")]) == "p: first is not 4-byte aligned"
    assert both([(0, 64, 4, 0, 1, "first"), (A + 2, 64, 4, 0, 1, "second")]) == "p: first is required"
    # presence and alignment of the whole table come before any overlap
    assert both([(A, 64, 4, 1, 1, "out"), (A, 64, 4, 0, 1, "in"), (A + 1, 64, 4, 0, 1, "odd")]) == "p: odd is not 4-byte aligned"
    # two inputs may share memory
    assert both([(A, 64, 4, 0, 1, "a"), (A, 64, 4, 0, 1, "b"), (A + 64, 64, 4, 1, 1, "out")]) == ""
    # a written entry is not compared with itself, but a second row with the same memory is another buffer
    assert both([(A, 64, 4, 1, 1, "out")]) == ""
    assert both([(A, 64, 4, 1, 1, "out"), (A, 64, 4, 1, 1, "again")]) == "p: out overlaps again"
    assert both([(A, 64, 4, 0, 1, "in"), (A, 64, 4, 1, 1, "out")]) == "p: out overlaps in"
    # written entries in table order, each against the others in table order
    assert both([(A, 64, 4, 0, 1, "in"), (A + 128, 64, 4, 1, 1, "o1"), (A, 64, 4, 1, 1, "o2"), (A + 128, 64, 4, 0, 1, "late")]) == "p: o1 overlaps late"
    assert both([]) == ""


def test_random_tables(shim):
    """4000 seeded tables of 2 to 10 entries inside one 4 KiB window (so that overlaps are common), addresses below 2^40 so that
    addr + bytes cannot wrap, at least one byte per buffer (the rule speaks of shared bytes: an empty buffer has none)"""
    rng = np.random.default_rng(20261019)
    kinds = {"": 0, "required": 0, "aligned": 0, "overlaps": 0}
    for _ in range(4000):
        n = int(rng.integers(2, 11))
        base = int(rng.integers(1, (1 << 40) - (1 << 20))) // 4096 * 4096 + 4096
        table = []
        for k in range(n):
            align = int(rng.choice([4, 8, 16]))
            addr = base + int(rng.integers(0, 4096))
            if rng.random() < 0.93:
                addr = addr // align * align
            if rng.random() < 0.12:
                addr = 0
            table.append((addr, int(rng.integers(1, 1024)), align, int(rng.random() < 0.35), int(rng.random() < 0.6), f"b{k}"))
        want = brute("pt_x", table)
        assert check(shim, "pt_x", table) == want, table
        kinds[want.split(" ")[-1] if want.endswith(("required", "aligned")) else ("overlaps" if want else "")] += 1
    assert all(v >= 200 for v in kinds.values()), kinds  # every outcome is well represented
