"""CPU checks that every entry of the generated-kernel shape table
(tests/jit_forms.py) really is the form it claims: the source that
zfec_amd/csrc/bitslice.cpp generates for it (the zfec/fec.c:487-505 /
:527-557 apply, specialised per matrix) carries that form's markers and no
other form's.  tests/test_gpu_jit_forms.py runs the same table on the GPU, so
a shape that options_for moves to another form fails here instead of leaving
a form unexecuted.  No GPU: the kernels are generated and compiled for gfx950
by hipRTC in a child process."""
import re

import pytest

import jit_forms
from jit_forms import DMA, KSPLIT, ONE, RESIDENT, SHAPES, SPLIT


def one_source(tmp_path, shape):
    files = jit_forms.generated_sources(tmp_path, shape.k, shape.m, shape.op, shape.index, shape.flags)
    assert len(files) == 1, sorted(files)
    (name, src), = files.items()
    assert name.startswith(shape.kernel_prefix() + "_"), name
    return src


def test_table_holds_every_form_and_the_listed_shapes():
    assert set(s.form for s in SHAPES) == set(jit_forms.FORMS)
    assert len(set(s.id for s in SHAPES)) == len(SHAPES)
    have = set((s.k, s.m, s.op, s.r) for s in SHAPES)
    for want in [(1, 2, "enc", 1), (32, 42, "enc", 10), (33, 34, "enc", 1), (33, 43, "enc", 10), (40, 48, "enc", 10),
                 (33, 44, "enc", 11), (50, 82, "enc", 32), (34, 80, "enc", 46), (40, 48, "dec", 40),
                 (13, 33, "enc", 20), (20, 50, "enc", 30), (12, 20, "dec", 12), (21, 51, "enc", 30),
                 (32, 62, "enc", 30), (22, 30, "dec", 22)]:
        assert want in have, want
    for s in SHAPES:
        assert jit_forms.expected_form(s.k, s.r) == (s.form, s.tiles), s.id
        if s.op == "dec":  # some secondaries among the received blocks, some primaries present
            assert 0 < sum(n >= s.k for n in s.nums) < s.k, s.id
    k, m = jit_forms.PAST_LIMIT
    assert k * (m - k) > jit_forms.MAX_COEF


@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
def test_form_markers(tmp_path, shape):
    src = one_source(tmp_path, shape)
    k, r, form, tiles = shape.k, shape.r, shape.form, shape.tiles
    bounds = int(re.search(r"__launch_bounds__\((\d+)\)", src).group(1))
    assert bounds == (256 if form in (ONE, KSPLIT) else 64 * tiles), bounds
    assert ("red[" in src) == (form == KSPLIT)
    assert ("blockIdx.x * 4u" in src) == (form == ONE)
    assert ("dma16(ka->" in src) == (form == DMA)
    assert ("dma_wait();" in src) == (form == DMA)
    sh = re.search(r"__shared__ u32x4 sh\[(\d+)\]", src)
    assert (sh is not None) == (form in (RESIDENT, DMA)) and ("sh[" in src) == (sh is not None)
    if form == RESIDENT:
        assert int(sh.group(1)) == k * 128
    if form == DMA:
        assert int(sh.group(1)) == 2 * 4 * 128
        # the phases: ceil(k / 4) waits per tile branch, the last phase k - 4 (phases - 1) inputs
        assert src.count("dma_wait();") == tiles * -(-k // 4)
    branches = re.findall(r"if \(tile == (\d+)u\) \{", src)
    if form in (SPLIT, RESIDENT, DMA):
        assert branches == [str(t) for t in range(tiles)], branches
    else:
        assert not branches
    if form == KSPLIT:
        assert int(re.search(r"__shared__ u32x4 red\[(\d+)\]", src).group(1)) == r * 4 * 2 * 64
        # the input slices of the four waves, and the store of row i by wave i % 4
        slices = [(int(a), int(b)) for a, b in re.findall(r"if \(wave == \du\) \{  // inputs (\d+)\.\.(\d+)", src)]
        assert slices == [(w * k // 4, (w + 1) * k // 4 - 1) for w in range(4)], slices
        assert re.findall(r"if \(wave == (\d)u\) \{  // row (\d+):", src) == [(str(i % 4), str(i)) for i in range(r)]
    # every row is stored, both halves, and the walk's carry is there
    for i in range(r):
        assert src.count("st(ro%d, lo16" % i) == 2, i
    assert "if (c >= a.cps) { c -= a.cps; ++s; }" in src
    if shape.zero_slices:
        # a ksplit wave whose whole input slice has coefficient 0 for a row: all eight planes "= 0u"
        zero = re.findall(r"^    a(\d+)_(\d) = 0u;$", src, re.M)
        for row in shape.unit_cols:
            assert zero.count((str(row), "0")) == 3, (row, zero.count((str(row), "0")))
        assert len(zero) == 3 * 8 * len(shape.unit_cols), len(zero)
    elif shape.unit_cols:
        # Outside ksplit no plane of a non-zero row stays unset (a non-zero coefficient maps onto every
        # output bit), so a unit row's zero coefficients show as the first assignment coming from the
        # unit column's input instead of input 0: plane b of 1 * x is plane b of x.
        for row, col in shape.unit_cols.items():
            t = [x for x in range(tiles) if x * r // tiles <= row < (x + 1) * r // tiles][0]
            n = t * k + col
            for b in range(8):
                assert re.search(r"^    a%d_%d = q%d_%d;$" % (row, b, n, b), src, re.M), (row, b, n)
                assert len(re.findall(r"^    a%d_%d (=|\^=) " % (row, b), src, re.M)) == 1, (row, b)


def test_coefficient_sweep_matrices_hold_every_value():
    """What the GPU coefficient sweep launches: rows 2..255 of the 2/256 code
    hold every value 2..255 in each column and no 0 or 1; a k = 1 code's
    parity rows are [1]."""
    from oracle import oracle

    enc = oracle.enc_matrix(2, 256)[2:]
    for j in range(2):
        assert sorted(int(v) for v in enc[:, j]) == list(range(2, 256)), j
    assert (oracle.enc_matrix(1, 10)[1:] == 1).all()


def test_past_the_limit_generates_nothing(tmp_path):
    k, m = jit_forms.PAST_LIMIT
    assert jit_forms.generated_sources(tmp_path, k, m, "enc", list(range(k, m))) == {}


@pytest.mark.parametrize("k,m,groups", jit_forms.ROW_GROUPS)
def test_row_groups_each_get_a_kernel(tmp_path, k, m, groups):
    """More than 48 rows: one generated kernel per near-equal row group, all of
    the shared, all-resident form (k <= 8: no DMA phases)."""
    assert [n for _, n in jit_forms.row_groups(m - k)] == groups
    files = jit_forms.generated_sources(tmp_path, k, m, "enc", list(range(k, m)))
    assert len(files) == len(groups), sorted(files)
    got = sorted(int(re.match(r"zfec_hip_bitslice_k%d_r(\d+)_" % k, f).group(1)) for f in files)
    assert got == sorted(groups), got
    for name, src in files.items():
        rg = int(re.match(r"zfec_hip_bitslice_k%d_r(\d+)_" % k, name).group(1))
        assert jit_forms.expected_form(k, rg)[0] == RESIDENT
        assert "__launch_bounds__(%d)" % (64 * jit_forms.tiles_of(rg)) in src
        assert "__shared__ u32x4 sh[%d]" % (k * 128) in src and "dma16(ka->" not in src
