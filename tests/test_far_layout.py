"""The design of the far-offset tests (tests/far_arena.py,
tests/test_gpu_far_offsets.py), held on the CPU: for every layout and every
input of every GPU case, the places a truncated offset would address lie inside
the arena, never on the bytes they stand for, and hold other bytes than those;
rows straddle and follow 2^31 and 2^32; and the checker's rules reject a row
written at its 2^32 alias.  The GPU module's proof that its tests bite is here:
no kernel is broken on the GPU to show it."""
import numpy as np
import pytest

import far_arena
import test_gpu_far_offsets as far
from far_arena import BACKGROUND, GUARD, LEAD, SPAN, Layout, Sparse, aliases, judge, judge_source

CASES = list(far.all_cases())


def whole_layouts(case):
    return [getattr(case, n) for n in ("lin", "lout", "lay") if hasattr(case, n)]


def test_every_table_row_has_its_cases():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    assert len(CASES) == sum(len(v) for v in far.APPLY.values()) + 1 + len(far.MIXED) + len(far.REPAIR) + \
        len(far.VERIFY) + len(far.LOCATE) + len(far.CORRECT)
    assert [c.geom for c in far.SMALL + far.KS] == ["far_pair"] * 3
    assert {c.name for c in far.VERIFY} == {"matverify_reg<3,7>", "matverify_bsr<6>", "matverify_bsr<8,lds>",
                                            "matverify_bsr<10,lds,tbl>", "rows_differ"}
    assert [s.form for s in (c.shape for c in far.JIT)] == list(far.jit_forms.FORMS)


def test_aliases():
    assert aliases(5) == (5, 5, 5)
    assert aliases(2**31 + 7) == (2**31 + 7, 7, 7 - 2**31)
    assert aliases(2**32 + 7) == (7, 7, 7)
    assert aliases(2**32 + 2**28) == (2**28, 2**28, 2**28)
    assert aliases(3 * 2**30 + 1) == (3 * 2**30 + 1, 2**30 + 1, 1 - 2**30)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_layout_of(case):
    """Aliases inside the arena and off the true bytes; the extent fits; rows
    straddle and follow both edges; odd strides."""
    for lay in whole_layouts(case) + [lay for lay, _ in case.placed()]:
        assert lay.first >= 0 and lay.first + lay.extent <= SPAN, lay
        assert lay.bs >= lay.sz and (lay.bs % 2 == 1 or lay.rows == 1), lay
        assert lay.ss % 2 == 1 or lay.kind == "far_blocks", lay
        if lay.kind == "far_blocks":
            assert lay.ss == lay.sz + 8 and lay.ns * lay.ss <= lay.bs
        else:
            assert lay.rows * lay.bs <= lay.ss
        for s, j, o in lay.starts():
            for a in aliases(o):
                assert -LEAD <= a and a + lay.sz <= SPAN, (lay, s, j, a)
                assert a == o or a + lay.sz <= o or a >= o + lay.sz, (lay, s, j, "an alias overlaps the row")
            for a in aliases(o + lay.sz):
                assert -LEAD <= a <= SPAN, (lay, s, j, a)
    for lay in whole_layouts(case):
        both = lay.kind != "far_blocks" or far_arena.far_blocks_both(lay.rows, lay.sz, lay.ns)
        if lay.rows == 1 and lay.kind == "far_blocks":
            continue  # no block stride in play
        assert lay.straddlers(2**32), lay
        assert lay.beginners(2**31, 2**32) and lay.beginners(2**32), lay
        if both:
            assert lay.straddlers(2**31), lay
        for edge in (2**31, 2**32):
            for s, j in lay.straddlers(edge):
                o = lay.start(s, j)
                assert o < edge < o + lay.sz - 1


def test_which_block_counts_straddle_both_edges():
    assert [r for r in range(1, 14) if far_arena.far_blocks_both(r, far.SZ)] == [3, 5, 7, 9, 10, 11, 12, 13]
    used = {lay.rows for c in CASES for lay in whole_layouts(c) if lay.kind == "far_blocks"}
    assert {r for r in used if not far_arena.far_blocks_both(r, far.SZ)} <= {1, 2, 4, 6, 8}
    # every scrub call and the 3/10 encode, decode and repair have both
    assert all(far_arena.far_blocks_both(c.lay.rows, c.sz) for c in far.VERIFY + far.LOCATE + far.CORRECT)
    assert all(far_arena.far_blocks_both(r, far.SZ) for r in (3, 7, 10))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_source_bytes_at_every_alias_differ(case):
    """Where a truncated offset would read instead of an input row, the source
    arena holds BACKGROUND or parts of other rows: never the row's own bytes."""
    model = Sparse(BACKGROUND)
    placed = case.placed()
    for lay, blocks in placed:
        model.place(lay, blocks)
    seen = 0
    for lay, blocks in placed:
        assert (model.gather(Layout(lay.kind, lay.rows, lay.sz, 1, lay.first, (lay.bs, lay.ss)))[0] == blocks[0]).all()
        for s, j, o in lay.starts():
            for a in set(aliases(o)) - {o}:
                assert (model.read(a, lay.sz) != blocks[s, j]).any(), (case.id, lay, s, j, a)
                seen += 1
    assert seen or all(lay.rows == 1 and lay.kind == "far_blocks" for lay, _ in placed)


def test_one_block_past_4gib_fits():
    assert far.BIG <= SPAN
    for o in (far.BIG - 1, 2**32 + 4000):
        assert all(-LEAD <= a < SPAN for a in aliases(o))


# ---- the checker's rules on synthetic results ---------------------------------------------------

def synthetic():
    lay = Layout("far_stripes", 7, far.SZ)
    want = far_arena.data(1, lay.ns, lay.rows, lay.sz)
    s, j = lay.far_rows()[1]
    o = lay.start(s, j)
    assert o >= 2**32 and o % 2**32 != o
    return lay, want, (s, j), o % 2**32


def result(lay, want, skip=None):
    model = Sparse(GUARD)
    for s, j, o in lay.starts():
        if (s, j) != skip:
            model.write(o, want[s, j])
    return model


def test_checker_accepts_the_right_result():
    lay, want, _, _ = synthetic()
    model = result(lay, want)
    judge(model.gather(lay), want, model.count_not(GUARD), GUARD)
    judge_source(12345, 12345)


def test_checker_rejects_a_row_written_at_its_alias():
    """The row lands 2^32 bytes early (there on rows of stripe 5) and its true
    place keeps the guard: the gathered rows name it as untouched."""
    lay, want, (s, j), alias = synthetic()
    model = result(lay, want, skip=(s, j))
    model.write(alias, want[s, j])
    with pytest.raises(AssertionError, match="only untouched bytes") as info:
        judge(model.gather(lay), want, model.count_not(GUARD), GUARD)
    assert (s, j) in info.value.args[0][4]


def test_checker_rejects_a_row_written_at_its_alias_as_well():
    """One row is also written 2^32 bytes early, before the rows it lands on
    are written themselves: every row is right, and only the count over the
    whole arena sees the bytes left between those rows."""
    lay, want, (s, j), alias = synthetic()
    model = Sparse(GUARD)
    model.write(alias, want[s, j])
    model.place(lay, want)
    assert (model.gather(lay) == want).all()
    with pytest.raises(AssertionError, match="in the whole arena"):
        judge(model.gather(lay), want, model.count_not(GUARD), GUARD)


def test_checker_rejects_one_stray_byte_and_a_written_source():
    lay, want, _, _ = synthetic()
    model = result(lay, want)
    model.write(-LEAD + 9, np.array([GUARD ^ 1], dtype=np.uint8))
    with pytest.raises(AssertionError, match="in the whole arena"):
        judge(model.gather(lay), want, model.count_not(GUARD), GUARD)
    with pytest.raises(AssertionError, match="source arena was written"):
        judge_source(12345, 12346)
