"""The buffer ledger and ordering rule of frames and side passes (csrc/pt_lane_order.h), on the CPU: the header is compiled as host C++
(tests/hostshim/args_host.cpp) and compared with a plain restatement of its table.  Addresses are only numbers: no memory is touched.

Every lane keeps a ledger of the caller buffers its latest calls hold, in five groups: out (1), dn (3), di (2), gb (13), ri (2).  A call
on lane `own` is `shared` (it waits for everything the caller has queued) when something forces it or when another lane holds one of the
pointers it asks about in one of the groups it looks at; it then records on its own lane's ledger.  What each of the four families asks,
looks at, is forced by and records is the table of the header's opening comment; frame(), gbuffer(), reservoir() and cache() below are
that table in Python.  Null is no buffer: it never matches, not even an empty slot."""
import ctypes as C

import numpy as np
import pytest

OUT, DN, DI, GB, RI = 1, 2, 4, 8, 16
ALL = OUT | DN | DI | GB | RI
GROUPS = ((OUT, "out", 1), (DN, "dn", 3), (DI, "di", 2), (GB, "gb", 13), (RI, "ri", 2))  # the order of the shim's 21 addresses per lane


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    lib = C.CDLL(g.build_args_shim())
    u32, u64, ptr = C.c_uint32, C.c_uint64, C.c_void_p
    for name, args in (("lane_host_holds", [ptr, u32, u32, u64, u32]), ("lane_host_frame", [ptr, u32, u32, u64, ptr, u32, ptr]),
                       ("lane_host_gbuffer", [ptr, u32, u32, u32, ptr]), ("lane_host_reservoir", [ptr, u32, u32, u32, ptr]),
                       ("lane_host_cache", [ptr, u32, u32, u32, u32, u64, u32, ptr, u32, ptr])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = u32, args
    lib.lane_host_window_marker_slot.restype, lib.lane_host_window_marker_slot.argtypes = u64, [u64, u64]
    return lib


def empty(n_lanes):
    return [{name: [0] * count for _, name, count in GROUPS} for _ in range(n_lanes)]


def flat(ledgers):
    return np.array([a for led in ledgers for _, name, _ in GROUPS for a in led[name]], np.uint64)


def unflat(words, n_lanes):
    out, k = [], 0
    for _ in range(n_lanes):
        led = {}
        for _, name, count in GROUPS:
            led[name] = [int(a) for a in words[k:k + count]]
            k += count
        out.append(led)
    return out


def addresses(a):
    return np.array(list(a), np.uint64)


# ---- the restatement: ledgers are dicts of lists of integers, 0 = null; each returns (shared, forced) and updates ledgers[own]
def holds(ledgers, own, p, groups):
    return p != 0 and any(p in led[name] for i, led in enumerate(ledgers) if i != own for bit, name, _ in GROUPS if groups & bit)


def frame(ledgers, own, out, dn, di):
    forced = di is not None
    shared = forced or any(holds(ledgers, own, p, OUT | DN | DI) for p in [out] + list(dn))
    ledgers[own].update(out=[out], dn=list(dn), di=list(di) if di is not None else [0, 0])
    return shared, forced


def gbuffer(ledgers, own, first_call, gb):
    shared = first_call or any(holds(ledgers, own, p, OUT | GB | DN | DI) for p in gb)
    ledgers[own]["gb"] = list(gb)
    return shared, first_call


def reservoir(ledgers, own, first_call, io):
    forced = first_call or any(p not in ledgers[own]["gb"] for p in io[:8])
    shared = forced or any(holds(ledgers, own, p, ALL) for p in io)
    ledgers[own]["ri"] = list(io[8:])
    return shared, forced


def cache(ledgers, own, first_call, query, out, outputs, dn, di):
    forced = first_call or di is not None
    shared = forced or (query and any(holds(ledgers, own, p, ALL) for p in [out] + list(dn)))
    if di is not None or outputs:
        ledgers[own].update(dn=list(dn) if query else [0, 0, 0], di=list(di) if di is not None else [0, 0])
    return shared, forced


# ---- the header, through the shim: same arguments, returns (shared, the ledgers afterwards)
def run(shim, fn, ledgers, own, *args):
    words = flat(ledgers)
    shared = fn(words.ctypes.data, len(ledgers), own, *args)
    return bool(shared), unflat(words, len(ledgers))


def h_frame(shim, ledgers, own, out, dn, di):
    d, e = addresses(dn), addresses(di if di is not None else [0, 0])
    return run(shim, shim.lane_host_frame, ledgers, own, out, d.ctypes.data, int(di is not None), e.ctypes.data)


def h_gbuffer(shim, ledgers, own, first_call, gb):
    g = addresses(gb)
    return run(shim, shim.lane_host_gbuffer, ledgers, own, int(first_call), g.ctypes.data)


def h_reservoir(shim, ledgers, own, first_call, io):
    b = addresses(io)
    return run(shim, shim.lane_host_reservoir, ledgers, own, int(first_call), b.ctypes.data)


def h_cache(shim, ledgers, own, first_call, query, out, outputs, dn, di):
    d, e = addresses(dn), addresses(di if di is not None else [0, 0])
    return run(shim, shim.lane_host_cache, ledgers, own, int(first_call), int(query), out, int(outputs), d.ctypes.data, int(di is not None), e.ctypes.data)


FAMILIES = {"frame": (frame, h_frame), "gbuffer": (gbuffer, h_gbuffer), "reservoir": (reservoir, h_reservoir), "cache": (cache, h_cache)}


def both(shim, family, ledgers, own, *args):
    """the header against the restatement on one state -> (shared, forced, the ledgers afterwards); other lanes' ledgers must not change"""
    restated, header = FAMILIES[family]
    want = [{k: list(v) for k, v in led.items()} for led in ledgers]
    shared, forced = restated(want, own, *args)
    got_shared, got = header(shim, ledgers, own, *args)
    assert got_shared == bool(shared), (family, ledgers, own, args)
    assert got == want, (family, ledgers, own, args)
    assert all(got[i] == ledgers[i] for i in range(len(ledgers)) if i != own)
    return bool(shared), bool(forced), got


# ---- random states
POOL = [0x7F0000000000 + 0x1000 * k for k in range(1, 65)]  # 64 addresses
P_SLOT = 0.25       # a ledger slot is filled with this probability
P_FIRST_CALL = 0.1
P_OWN_GBUFFER = 0.9  # the reservoir pass takes its inputs from its own lane's G-buffer record


def draw(rng, family):
    """a random state and call of `family`, honouring the entry point's own non-null requirements: a frame's `out`; one of the G-buffer's
    channels; all ten buffers of the reservoir pass; the cache's `out` with QUERY, both DI buffers of a supplied DI, and denoiser
    outputs of a mode (1: SpecularHitDistance, else Diffuse and Specular)"""
    pick = lambda: int(rng.choice(POOL))  # noqa: E731
    maybe = lambda p=0.5: pick() if rng.random() < p else 0  # noqa: E731
    n = int(rng.integers(2, 9))
    own = int(rng.integers(0, n))
    ledgers = [{name: [maybe(P_SLOT) for _ in range(count)] for _, name, count in GROUPS} for _ in range(n)]
    first = bool(rng.random() < P_FIRST_CALL)
    if family == "frame":
        mode = int(rng.integers(0, 4))
        dn = [0, 0, pick()] if mode == 1 else ([pick(), pick(), 0] if mode else [0, 0, 0])
        return ledgers, own, (pick(), dn, [pick(), pick()] if rng.random() < 0.15 else None)
    if family == "gbuffer":
        gb = [maybe(0.3) for _ in range(13)]
        if not any(gb):
            gb[int(rng.integers(0, 13))] = pick()
        return ledgers, own, (first, gb)
    if family == "reservoir":
        io = [pick() for _ in range(10)]
        if rng.random() < P_OWN_GBUFFER:
            ledgers[own]["gb"] = [pick() for _ in range(13)]  # its own G-buffer call wrote all channels ...
            io[:8] = [int(a) for a in rng.choice(ledgers[own]["gb"], 8)]  # ... and the pass reads eight of them
        return ledgers, own, (first, io)
    query = bool(rng.random() < 0.75)
    mode = int(rng.integers(0, 4))
    dn = [pick(), 0, 0] if mode == 1 else ([0, pick(), pick()] if mode else [0, 0, 0])
    return ledgers, own, (first, query, pick() if query else maybe(), mode != 0, dn, [pick(), pick()] if rng.random() < 0.15 else None)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_random_states(shim, family):
    """1500 seeded states per entry-point family (6000 in all): `shared` and every lane's ledger afterwards equal the restatement's; among
    the cases with no forced cause both answers occur in at least a tenth"""
    rng = np.random.default_rng([20261019, list(FAMILIES).index(family)])
    answers = {False: 0, True: 0}
    for _ in range(1500):
        ledgers, own, args = draw(rng, family)
        shared, forced, _ = both(shim, family, ledgers, own, *args)
        if not forced:
            answers[shared] += 1
    unforced = answers[False] + answers[True]
    assert unforced >= 750 and min(answers.values()) >= 0.1 * unforced, answers


def test_random_membership(shim):
    """the membership test by itself, over every mask of groups"""
    rng = np.random.default_rng(7)
    hits = 0
    for _ in range(1500):
        n = int(rng.integers(2, 9))
        own = int(rng.integers(0, n))
        ledgers = [{name: [int(rng.choice(POOL)) if rng.random() < P_SLOT else 0 for _ in range(count)] for _, name, count in GROUPS} for _ in range(n)]
        p = int(rng.choice(POOL)) if rng.random() < 0.9 else 0
        groups = int(rng.integers(0, 32))
        got, after = run(shim, shim.lane_host_holds, ledgers, own, p, groups)
        assert got == holds(ledgers, own, p, groups) and after == ledgers
        hits += got
    assert 150 <= hits <= 1350


# ---- directed cases: one per clause of the table; each clause alone flips the answer
A, B, D, E = POOL[0], POOL[1], POOL[2], POOL[3]
GBUF = [POOL[10 + k] for k in range(13)]


def three_lanes(**other):
    """three lanes, lane 1 is the caller's; lane 2's ledger holds `other` (group name -> addresses)"""
    ledgers = empty(3)
    for name, a in other.items():
        ledgers[2][name][:len(a)] = a
    return ledgers


def test_frame_clauses(shim):
    assert both(shim, "frame", three_lanes(), 1, A, [0, 0, 0], None)[:2] == (False, False)
    for group in ("out", "dn", "di"):
        assert both(shim, "frame", three_lanes(**{group: [A]}), 1, A, [0, 0, 0], None)[0]
        for k in range(3):  # a denoiser buffer is held to the rule of `out`
            dn = [0, 0, 0]
            dn[k] = B
            assert both(shim, "frame", three_lanes(**{group: [B]}), 1, A, dn, None)[0]
    # a pointer that another lane holds only in gb, or only in ri: not shared
    assert not both(shim, "frame", three_lanes(gb=[A]), 1, A, [0, 0, 0], None)[0]
    assert not both(shim, "frame", three_lanes(ri=[A]), 1, A, [0, 0, 0], None)[0]
    # its own lane's record does not count
    own = three_lanes()
    own[1]["out"] = [A]
    assert not both(shim, "frame", own, 1, A, [0, 0, 0], None)[0]
    # a supplied DI forces it, and is recorded; a frame without one clears the record
    shared, forced, after = both(shim, "frame", three_lanes(), 1, A, [B, D, 0], [D, E])
    assert shared and forced and after[1] == dict(empty(1)[0], out=[A], dn=[B, D, 0], di=[D, E])
    assert both(shim, "frame", after, 1, B, [0, 0, E], None)[2][1] == dict(empty(1)[0], out=[B], dn=[0, 0, E])


def test_gbuffer_clauses(shim):
    gb = [A] + [0] * 12
    assert both(shim, "gbuffer", three_lanes(), 1, False, gb)[:2] == (False, False)
    for group in ("out", "gb", "dn", "di"):
        assert both(shim, "gbuffer", three_lanes(**{group: [A]}), 1, False, gb)[0]
    # a pointer that another lane holds only in ri: not shared -- the same pointer asked by the reservoir pass: shared
    assert not both(shim, "gbuffer", three_lanes(ri=[A]), 1, False, gb)[0]
    mine = three_lanes(ri=[A])
    mine[1]["gb"] = [A] + GBUF[1:]
    assert both(shim, "reservoir", mine, 1, False, [A] + GBUF[1:8] + [B, D])[:2] == (True, False)
    mine[2]["ri"] = [0, 0]
    assert both(shim, "reservoir", mine, 1, False, [A] + GBUF[1:8] + [B, D])[:2] == (False, False)
    # the first call forces it; the record holds the nulls too
    shared, forced, after = both(shim, "gbuffer", three_lanes(), 1, True, gb)
    assert shared and forced and after[1]["gb"] == gb
    full = three_lanes()
    full[1]["gb"] = list(GBUF)
    assert both(shim, "gbuffer", full, 1, False, gb)[2][1]["gb"] == gb


def test_reservoir_clauses(shim):
    def state(**other):
        ledgers = three_lanes(**other)
        ledgers[1]["gb"] = list(GBUF)
        return ledgers
    io = GBUF[:8] + [A, B]
    shared, forced, after = both(shim, "reservoir", state(), 1, False, io)
    assert (shared, forced) == (False, False) and after[1]["ri"] == [A, B]
    for group in ("out", "dn", "di", "gb", "ri"):
        assert both(shim, "reservoir", state(**{group: [A]}), 1, False, io)[:2] == (True, False)     # an output
        assert both(shim, "reservoir", state(**{group: [GBUF[3]]}), 1, False, io)[:2] == (True, False)  # an input
    # one input missing from the own lane's gb: shared, whichever input it is
    for k in range(8):
        missing = list(io)
        missing[k] = D
        assert both(shim, "reservoir", state(), 1, False, missing)[:2] == (True, True)
    # (that another lane's gb has it does not help)
    other = three_lanes(gb=GBUF)
    assert both(shim, "reservoir", other, 1, False, io)[:2] == (True, True)
    assert both(shim, "reservoir", state(), 1, True, io)[:2] == (True, True)


def test_cache_clauses(shim):
    none = [0, 0, 0]
    assert both(shim, "cache", three_lanes(), 1, False, True, A, False, none, None)[:2] == (False, False)
    for group in ("out", "dn", "di", "gb", "ri"):
        assert both(shim, "cache", three_lanes(**{group: [A]}), 1, False, True, A, False, none, None)[0]
        # without QUERY nothing is asked: `out`, and a denoiser output, that another lane holds: not shared
        assert not both(shim, "cache", three_lanes(**{group: [A]}), 1, False, False, A, False, none, None)[0]
        assert not both(shim, "cache", three_lanes(**{group: [B]}), 1, False, False, A, True, [B, 0, 0], None)[0]
        for k in range(3):
            dn = [0, 0, 0]
            dn[k] = B
            assert both(shim, "cache", three_lanes(**{group: [B]}), 1, False, True, A, True, dn, None)[0]
    # a supplied DI forces it, with and without QUERY; so does the first call
    assert both(shim, "cache", three_lanes(), 1, False, True, A, False, none, [D, E])[:2] == (True, True)
    assert both(shim, "cache", three_lanes(), 1, False, False, 0, False, none, [D, E])[:2] == (True, True)
    assert both(shim, "cache", three_lanes(), 1, True, True, A, False, none, None)[:2] == (True, True)
    # the record: never `out`; nothing at all without a DI or outputs; dn in the order given, nulls without QUERY; di or nulls
    before = three_lanes()
    before[1].update(out=[E], dn=[E, E, E], di=[E, E])
    assert both(shim, "cache", before, 1, False, True, A, False, none, None)[2][1] == before[1]
    assert both(shim, "cache", before, 1, False, True, A, True, [B, 0, 0], None)[2][1] == dict(before[1], dn=[B, 0, 0], di=[0, 0])
    assert both(shim, "cache", before, 1, False, True, A, True, [0, B, D], [D, B])[2][1] == dict(before[1], dn=[0, B, D], di=[D, B])
    assert both(shim, "cache", before, 1, False, False, A, True, [B, 0, 0], None)[2][1] == dict(before[1], dn=[0, 0, 0], di=[0, 0])
    assert both(shim, "cache", before, 1, False, False, 0, False, none, [D, B])[2][1] == dict(before[1], dn=[0, 0, 0], di=[D, B])


def test_null_never_matches(shim):
    """the other lanes' ledgers are all nulls: a null pointer of the call matches none of them, in any family"""
    ledgers = empty(3)
    assert run(shim, shim.lane_host_holds, ledgers, 1, 0, ALL) == (False, ledgers)
    assert not both(shim, "frame", empty(3), 1, 0, [0, 0, 0], None)[0]
    assert not both(shim, "gbuffer", empty(3), 1, False, [0] * 13)[0]
    assert not both(shim, "cache", empty(3), 1, False, True, 0, True, [0, 0, 0], None)[0]
    mine = empty(3)  # (the reservoir pass's inputs are in its own lane's gb, nulls as they are: that test is a plain comparison)
    assert not both(shim, "reservoir", mine, 1, False, [0] * 10)[0]


def test_window_marker_slot(shim):
    """the marker a call waits for: the slot (call number mod n_lanes) of the render call n_lanes - 1 calls ago, slot 0 before that call exists"""
    for n_lanes in range(1, 9):
        for calls in range(41):
            ago = calls - (n_lanes - 1)
            assert shim.lane_host_window_marker_slot(calls, n_lanes) == (ago % n_lanes if ago >= 0 else 0), (calls, n_lanes)
