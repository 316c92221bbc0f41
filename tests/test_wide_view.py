"""The 4-wide view of the tree without a GPU: tests/wide_reference.py's restatement against its own checker on host-built trees, the
proof that the checker can fail (one mutation per property), the exact fma both rest on, and the numpy model of the walk's stack."""
from fractions import Fraction

import numpy as np
import pytest

import wide_reference as wr
import wide_scenes

MUTATION_SCENES = [n for n in wide_scenes.NAMES if n not in ("procedural_40000",) and not n.startswith("line-") and not n.endswith("-3")]


@pytest.fixture(scope="module")
def trees(dxrs, host):
    """(scene, sah) -> (binary records, depth, restated wide records, populated mask), built once"""
    lib, cache = dxrs.load_hip(), {}

    def get(name, sah):
        if (name, sah) not in cache:
            nodes, _, depth = lib.lbvh_build_host(wide_scenes.layout(name, host, dxrs), sah=sah)
            rec, populated = wr.collapse4(nodes)
            rec.setflags(write=False)  # shared among the tests: nobody changes it
            cache[(name, sah)] = (nodes, depth, rec, populated)
        return cache[(name, sah)]
    return get


def test_fma_helper_is_correctly_rounded():
    """fma32 against round32_fraction of the exact sum, and round32_fraction against hand-worked cases: ties go to even, a 60-bit exponent
    gap leaves the large operand (or moves it by exactly one step where the sum leaves a power of two's lower neighbourhood)"""
    f32, one = np.float32, Fraction(1)
    eps = Fraction(1, 2 ** 23)
    assert wr.round32_fraction(one + eps / 2) == f32(1.0)                     # tie -> even (1.0)
    assert wr.round32_fraction(one + eps + eps / 2) == f32(1.0) + f32(2.0 ** -22)  # tie -> even (1 + 2 ulp)
    assert wr.round32_fraction(one + eps / 2 + Fraction(1, 2 ** 90)) == f32(1.0 + 2.0 ** -23)  # just above the tie: float64 cannot see this
    assert wr.round32_fraction(-(one + eps / 2)) == f32(-1.0)
    assert wr.round32_fraction(Fraction(3, 2 ** 150)) == f32(2.0 ** -148)       # subnormal tie -> even
    assert wr.round32_fraction(Fraction(2 ** 24 - 1, 2 ** 24) + Fraction(1, 2 ** 25)) == f32(1.0)  # the mantissa carries into the exponent
    # fma32 on ties: byte * cell is half an ulp of the origin
    assert wr.fma32(1, 2.0 ** -24, f32(1.0)) == f32(1.0)
    assert wr.fma32(1, 2.0 ** -24, f32(1.0 + 2.0 ** -23)) == f32(1.0 + 2.0 ** -22)
    assert wr.fma32(3, 2.0 ** -24, f32(1.0)) == f32(1.0 + 2.0 ** -22)          # 1 + 1.5 ulp: tie -> even
    assert wr.fma32(255, 2.0 ** -31, f32(-1.0)) == f32(-1.0 + 2.0 ** -24 * 2)  # below 1 the ulp halves: -1 + 255 * 2^-31 rounds to -1 + 2^-23
    # a 60-bit gap: float64's sum is inexact there (the Fraction path); the result is the origin
    big = f32(2.0 ** 30)
    assert wr.fma32(255, 2.0 ** -38, big) == big and wr.fma32(255, 2.0 ** -38, -big) == -big
    assert wr.fma32(1, 2.0 ** -30, f32(2.0 ** 30)) == big
    rng = np.random.default_rng(5)
    byte = rng.integers(0, 256, 4000)
    e_cell = rng.integers(-120, 20, 4000)
    origin = (rng.normal(size=4000) * 2.0 ** rng.integers(-30, 31, 4000)).astype(np.float32)
    # half of the cases: the product within a few bits of the origin's ulp, where rounding is decided
    e_org = np.frexp(origin.astype(np.float64))[1]
    e_cell[::2] = e_org[::2] - 24 - rng.integers(0, 10, 2000)
    got = wr.fma32(byte, np.ldexp(1.0, e_cell), origin)
    gaps = 0
    for b, e, o, g in zip(byte, e_cell, origin, got):
        exact = Fraction(int(b)) * Fraction(2) ** int(e) + Fraction(float(o))
        assert wr.round32_fraction(exact) == g, (b, e, o, g)
        gaps += b > 0 and abs(int(e) - int(np.frexp(float(o))[1])) >= 60
    assert gaps >= 100  # the 60-bit gaps are really among the cases


@pytest.mark.parametrize("sah", [False, True])
@pytest.mark.parametrize("name", wide_scenes.NAMES)
def test_restatement_satisfies_the_properties(trees, name, sah):
    """check_wide(nodes, collapse4(nodes)) on host-built trees: the text of DESIGN.md section 5 implies P1 to P6"""
    nodes, depth, rec, populated = trees(name, sah)
    if len(nodes) == 0:
        assert rec.shape == (0, 16)
        return
    assert np.array_equal(populated, wr.depths(nodes) % 2 == 0) and wr.depths(nodes).max() == depth - 1
    wr.check_wide(nodes, rec)
    if len(nodes) > 2:  # both parities of leaf depth, and wide nodes with fewer than 4 children, are what these layouts are for
        _, _, ref, *_ = wr.decode(rec[populated])
        assert name not in ("geometric", "concentric") or ((ref == -2 ** 31).sum(1) > 0).any()


def _labels(nodes, rec):
    with pytest.raises(wr.WideViolation) as e:
        wr.check_wide(nodes, rec)
    return e.value.labels


def _set_byte(rec, i, word, c, value):
    rec[i, word] = (int(rec[i, word]) & ~(0xFF << (8 * c))) | (int(value) << (8 * c))


@pytest.mark.parametrize("name", MUTATION_SCENES)
def test_mutations_are_rejected_with_their_label(trees, name):
    nodes, depth, good, populated = trees(name, True)
    lo, hi, ref, count = wr._children(nodes)
    used = (np.arange(4)[None, :] < count[:, None])[:, :, None] & populated[:, None, None]
    dlo, dhi, rref, cell, ql, qh = wr.decode(good)
    origin = np.ascontiguousarray(good[:, 0:3]).view(np.float32)[:, None, :]
    c3 = cell[:, None, :]
    # tight planes: contained with less than one cell to spare, and one byte inward is strictly inside the binary box
    tight_lo = used & (lo.astype(np.float64) - dlo < c3) & (ql < 255) & (wr.fma32(np.minimum(ql + 1, 255), c3, origin) > lo)
    tight_hi = used & (dhi.astype(np.float64) - hi < c3) & (qh > 0) & (wr.fma32(np.maximum(qh - 1, 0), c3, origin) < hi)
    assert tight_lo.sum() >= 10 and tight_hi.sum() >= 10, (int(tight_lo.sum()), int(tight_hi.sum()))
    rng = np.random.default_rng(11)
    for tight, word0, q, step in ((tight_lo, 4, ql, 1), (tight_hi, 7, qh, -1)):
        cand = np.stack(np.nonzero(tight), 1)
        for i, c, a in cand[rng.choice(len(cand), 5, replace=False)]:
            rec = good.copy()
            _set_byte(rec, i, word0 + a, c, q[i, c, a] + step)
            assert _labels(nodes, rec) == {"P4"}, (i, c, a)
    # a finer grid than the extent allows: exponent - 1, bytes doubled and clamped at 255, so an upper plane above byte 127 falls short
    # (the planes that keep their place may now be more than one of the halved cells out: P5 may join)
    i, a = (int(v[0]) for v in np.nonzero((used & (qh >= 129)).any(1)))
    rec = good.copy()
    rec[i, 3] = int(rec[i, 3]) - (1 << (8 * a))
    for c in range(count[i]):
        _set_byte(rec, i, 4 + a, c, min(2 * ql[i, c, a], 255)); _set_byte(rec, i, 7 + a, c, min(2 * qh[i, c, a], 255))
    assert "P4" in _labels(nodes, rec) and _labels(nodes, rec) <= {"P4", "P5"}
    # a coarser grid than the extent needs: exponent + 1, bytes halved outwards -- contained, but not tight
    rec = good.copy()
    rec[i, 3] = int(rec[i, 3]) + (1 << (8 * a))
    for c in range(count[i]):
        _set_byte(rec, i, 4 + a, c, ql[i, c, a] // 2); _set_byte(rec, i, 7 + a, c, (qh[i, c, a] + 1) // 2)
    assert _labels(nodes, rec) == {"P5"}
    # two child references swapped (their boxes stay): the list is out of order
    i = int(np.nonzero(populated & (count >= 2))[0][-1])
    rec = good.copy()
    rec[i, [10, 11]] = rec[i, [11, 10]]
    assert "P2" in _labels(nodes, rec)
    # a populated slot's reference replaced by the empty marker: its subtree is unreachable
    rec = good.copy()
    rec[i, 10 + count[i] - 1] = wr.EMPTY
    assert {"P2", "P3"} <= _labels(nodes, rec)
    # a record written into an odd-depth slot
    if (~populated).any():
        rec = good.copy()
        rec[int(np.nonzero(~populated)[0][0])] = good[0]
        assert "P1" in _labels(nodes, rec)
    # an origin word moved up by one ulp
    i, a = int(np.nonzero(populated)[0][-1]), 1
    rec = good.copy()
    rec[i, a:a + 1] = np.nextafter(origin[i, 0, a:a + 1], np.float32(np.inf)).view(np.uint32)
    assert "P6" in _labels(nodes, rec)
    wr.check_wide(nodes, good)  # and the unmutated records still pass


@pytest.mark.parametrize("name", ["concentric", "geometric"])
def test_stack_model_on_host_trees(trees, name):
    """T5 on the host SAH tree (the topology the default builder adopts): the model of the walk's stack stays within stack_entries"""
    nodes, depth, rec, _ = trees(name, True)
    o, d = wr.stack_rays(name, 2000, seed=9)
    peak = wr.stack_model(rec, o, d)
    assert peak <= depth + (depth + 1) // 2 + 2
    if name == "concentric":
        assert peak >= depth
