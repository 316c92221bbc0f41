"""GPU: pt_math.h's short exact forms -- pt_sqrt_ranged (v_sqrt_f32 + the two-neighbour fix-up, no rescaling), pt_rcp_ranged (v_rcp_f32 + one
Newton step) and pt_half_rcp_ranged (that of x + x) -- against the compiler's correctly rounded expansions (pt_sqrt, pt_rcp, pt_half_rcp), in
the device build of the header with the product's compiler flags (tests/hostshim/short_math_gpu.hip).
- One launch sweeps all 2^32 bit patterns through all six functions.  Inside each contract (sqrt: |x| >= 2^-96; rcp: 2^-126 <= |x| <= 2^126;
  half_rcp: 2^-126 <= |x| <= 2^125) and for +-0, +-inf and NaN the result bits must be equal; two NaNs count as equal.  Operands outside the
  contracts that differ are printed, not asserted: no call site may produce them (tests/test_short_math_ranges.py, and the proofs at the sites).
- A second, tiny launch returns the results at the contracts' edges and their neighbours, and at the specials, for a check value by value."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NAMES = ("sqrt", "rcp", "half_rcp")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    so = C.CDLL(g.build_short_math_gpu())
    so.sm_sweep.restype = C.c_int
    so.sm_sweep.argtypes = [C.c_void_p, C.c_void_p]
    so.sm_edges.restype = C.c_int
    so.sm_edges.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    return so


def test_all_operands_inside_the_contracts_give_the_expansions_bits(lib):
    counts = np.zeros(6, dtype=np.uint64)
    first = np.zeros(6, dtype=np.uint32)
    assert lib.sm_sweep(counts.ctypes.data, first.ctypes.data) == 0
    for k, name in enumerate(NAMES):
        print(f"{name}: inside the contract {int(counts[k])} operands differ (first 0x{int(first[k]):08x}); outside it {int(counts[3 + k])} "
              f"(first 0x{int(first[3 + k]):08x})")
    for k, name in enumerate(NAMES):
        assert counts[k] == 0, f"{name}: {int(counts[k])} operands inside the contract differ from the expansion, the first is 0x{int(first[k]):08x}"


def two(e):
    return np.uint32((e + 127) << 23)


def test_edges_of_the_contracts_and_specials(lib):
    edges = []
    for e in (-96, -126, 126, 125, -127, 127, 0):
        b = int(two(e)) if e > -127 else 0x00400000  # 2^-127 is subnormal
        edges += [b - 1, b, b + 1]
    specials = [0x00000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x00000001, 0x007FFFFF, 0x7F7FFFFF]
    mags = np.array(edges + specials, dtype=np.uint32)
    x = np.concatenate([mags, mags | np.uint32(0x80000000)])
    out = np.zeros((len(x), 6), dtype=np.uint32)
    assert lib.sm_edges(len(x), x.ctypes.data, out.ctypes.data) == 0
    mag = x & np.uint32(0x7FFFFFFF)
    special = (mag == 0) | (mag >= 0x7F800000)
    inside = {
        "sqrt": special | (mag >= two(-96)),
        "rcp": special | ((mag >= two(-126)) & (mag <= two(126))),
        "half_rcp": special | ((mag >= two(-126)) & (mag <= two(125))),
    }
    checked = 0
    for k, name in enumerate(NAMES):
        got, want = out[:, 2 * k], out[:, 2 * k + 1]
        nan = lambda w: (w & np.uint32(0x7FFFFFFF)) > 0x7F800000  # noqa: E731
        same = (got == want) | (nan(got) & nan(want))
        for i in np.nonzero(inside[name] & ~same)[0]:
            print(f"{name}(0x{int(x[i]):08x}): short 0x{int(got[i]):08x}, expansion 0x{int(want[i]):08x}")
        assert same[inside[name]].all(), name
        # a NaN comes back as a NaN, whatever its payload
        assert nan(got[nan(x)]).all(), name
        checked += int(inside[name].sum())
    # the three edge values the contracts name, and the specials, are among what was compared
    for e, name in ((-96, "sqrt"), (-126, "rcp"), (126, "rcp"), (-126, "half_rcp"), (125, "half_rcp")):
        assert inside[name][np.nonzero(x == two(e))[0][0]]
    assert checked > 100
    # what the specials must give (the IEEE answers), read from the short forms' own columns
    val = lambda name, bits: out[np.nonzero(x == np.uint32(bits))[0][0], 2 * NAMES.index(name)]  # noqa: E731
    assert val("sqrt", 0x00000000) == 0x00000000 and val("sqrt", 0x80000000) == 0x80000000 and val("sqrt", 0x7F800000) == 0x7F800000
    assert val("rcp", 0x00000000) == 0x7F800000 and val("rcp", 0x80000000) == 0xFF800000
    assert val("rcp", 0x7F800000) == 0x00000000 and val("rcp", 0xFF800000) == 0x80000000
    assert val("half_rcp", 0x00000000) == 0x7F800000 and val("half_rcp", 0xFF800000) == 0x80000000
