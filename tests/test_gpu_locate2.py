"""GPU checks of pair location (fec_locate2_batch: the location path of
fec_locate_batch, then zfec_amd/csrc/kernels.hip locate2_finish, pairs_locate
and pairs_finish).  The harness is tests/pair_cases.py: expected verdicts from
the numpy model (tests/pair_ref.py), the whole block buffer compared after every
call (nothing may be written), guard words around the two verdict planes, the
kernel name checked."""
import itertools

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from locate_ref import CLEAN, MANY
from pair_cases import FILL, NS, SIZES, Case, one, pair_patterns, saw_pairs, sweep, whole
from pair_ref import NONE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HEAL = False
SHUFFLED10 = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


# ---- sizes, batches, codes ---------------------------------------------------------------------

@pytest.mark.parametrize("nums", [list(range(10)), SHUFFLED10], ids=["in order", "shuffled"])
def test_all_sizes_and_batches(nums):
    """K=3/M=10 with all ten blocks (45 pairs: the pair bits cross a word
    boundary): the byte tail (1, 15), exact chunks (16, 1024), the overlapped
    last chunk (17, 1023), one wave plus one unit (1025), four waves plus one
    unit (4097); one stripe and 70 at a size of each kind."""
    code = capi.Code(3, 10)
    assert NS == (1, 3, 70)
    seen = sweep(code, 3, 10, nums, HEAL, SIZES, (3,), seed=310)
    seen |= sweep(code, 3, 10, nums, HEAL, (1, 17, 1024, 4097), (1, 70), seed=311)
    saw_pairs(seen)
    assert {(CLEAN, NONE), (MANY, NONE)} <= seen and any(a < 10 and b == NONE for a, b in seen)


@pytest.mark.parametrize("k,m,nb", [(1, 6, 5), (4, 12, 12), (10, 16, 16)])
def test_codes(k, m, nb):
    """c = 4, the minimum; 66 pairs in three words; the wide location path with
    120 pairs."""
    nums = list(range(nb))
    seen = sweep(capi.Code(k, m), k, m, nums, HEAL, SIZES, (3,), seed=100 * k + m)
    seen |= sweep(capi.Code(k, m), k, m, nums, HEAL, (17, 1025), (1, 70), seed=200 * k + m)
    saw_pairs(seen)


def test_the_limit_of_32_blocks():
    """K=20/M=60 with 32 blocks held: 496 pairs, exactly 16 words."""
    k, m = 20, 60
    nums = np.random.default_rng(2060).permutation(m)[:32].tolist()
    seen = sweep(capi.Code(k, m), k, m, nums, HEAL, (17, 1025), (3,), seed=2060,
                 only=("clean", "one byte", "far apart", "whole blocks"))
    saw_pairs(seen)
    case = Case(k, m, nums, 2, 64, HEAL)
    got, _ = case.run(capi.Code(k, m), [one(1, 30, 5), one(1, 31, 9)], "the last pair")
    assert got[:, 1].tolist() == [30, 31]


@pytest.mark.parametrize("k,m,nb", [(20, 60, 33), (3, 10, 6)])
def test_pair_pass_off(k, m, nb):
    """33 blocks held, and three checks: two corrupt blocks stay (MANY, NONE),
    and the call reports the single-block kernel (Case.name)."""
    nums = np.random.default_rng(nb).permutation(m)[:nb].tolist()
    seen = sweep(capi.Code(k, m), k, m, nums, HEAL, (17, 1025), (3,), seed=nb,
                 only=("clean", "one byte", "far apart", "whole blocks", "mix"))
    assert (MANY, NONE) in seen and all(b == NONE for a, b in seen)


@pytest.mark.parametrize("kind", ["packed", "bm"])
def test_layouts(kind):
    saw_pairs(sweep(capi.Code(3, 10), 3, 10, SHUFFLED10, HEAL, (15, 1025, 4097), (3, 70), seed=77, kind=kind))
    saw_pairs(sweep(capi.Code(10, 16), 10, 16, list(range(16)), HEAL, (1025,), (3,), seed=78, kind=kind))


# ---- every pair, triples, list walks ----------------------------------------------------------

def every_pair_case(sz):
    """Every pair of K=3/M=10 as the culprit, one stripe each, among clean and
    single-error stripes: 45 + 25 stripes."""
    nb, ns = 10, 70
    cor = []
    for s, (a, b) in enumerate(itertools.combinations(range(nb), 2)):
        cor += [one(s, a, (7 * s) % sz, 1 + s), one(s, b, (11 * s + 3) % sz, 2 + s)]
    for s in range(45, ns, 2):
        cor.append(one(s, s % nb, (5 * s) % sz, 0x40))
    return ns, cor


@pytest.mark.parametrize("sz", [16, 4097])
def test_every_pair(sz):
    ns, cor = every_pair_case(sz)
    case = Case(3, 10, range(10), ns, sz, HEAL)
    got, _ = case.run(capi.Code(3, 10), cor, "every pair")
    assert [tuple(v) for v in got[:, :45].T.tolist()] == list(itertools.combinations(range(10), 2))
    assert (got[1, 45:] == NONE).all()


def test_three_at_one_byte():
    """c = 7: the model says MANY for every triple tried."""
    ns, sz = 70, 1025
    triples = list(itertools.combinations(range(10), 3))[::2][:ns]
    cor = [one(s, j, 513, 1 + 3 * s + j) for s, tr in enumerate(triples) for j in tr]
    got, _ = Case(3, 10, range(10), ns, sz, HEAL).run(capi.Code(3, 10), cor, "triples")
    assert (got[0, :len(triples)] == MANY).all() and (got[1] == NONE).all()


@pytest.mark.parametrize("cap", [3, 1])
def test_list_walk(knobs, cap):
    """All 70 stripes dirty, and exactly one, under a grid of three workgroups
    and of one: the walk carries over many (entry, wave) steps per workgroup."""
    knobs(ZFEC_HIP_GRID_CAP=cap)
    code = capi.Code(3, 10)
    for sz in (1025, 4097):
        ns, cor = every_pair_case(sz)
        cor = [c for c in cor if c[0] < 45]
        for s in range(45, ns):
            cor += [one(s, s % 9, 0, 5), one(s, 9, sz - 1, 6)]
        got, _ = Case(3, 10, range(10), ns, sz, HEAL).run(code, cor, ("all dirty", cap, sz))
        assert (got[1] != NONE).all()
        got, _ = Case(3, 10, range(10), ns, sz, HEAL).run(code, [one(69, 2, 0, 1), one(69, 8, sz - 1, 1)],
                                                          ("one dirty", cap, sz))
        assert got[:, 69].tolist() == [2, 8] and (got[0, :69] == CLEAN).all()


def test_all_clean():
    for k, m, nb in ((3, 10, 10), (10, 16, 16)):
        got, _ = Case(k, m, range(nb), 70, 4097, HEAL).run(capi.Code(k, m), [], "clean")
        assert (got[0] == CLEAN).all() and (got[1] == NONE).all()


# ---- memory kinds, streams, refusals ---------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
@pytest.mark.parametrize("out_mem", ["numpy", "pinned"])
def test_culprit_in_host_memory(k, m, out_mem):
    code = capi.Code(k, m)
    for flags in (capi.FEC_FLAG_ASYNC, 0, capi.FEC_FLAG_LIBRARY_STREAM):
        saw_pairs(sweep(code, k, m, list(range(m)), HEAL, (1025,), (37,), seed=5, out_mem=out_mem, flags=flags))


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_blocks_in_page_locked_host_memory(k, m):
    code = capi.Code(k, m)
    for out_mem in ("device", "numpy"):
        saw_pairs(sweep(code, k, m, list(range(m)), HEAL, (1025,), (5,), seed=6, mem="pinned", out_mem=out_mem,
                        flags=0))


def test_streams():
    """A non-default stream, and the library's own."""
    code = capi.Code(3, 10)
    case = Case(3, 10, range(10), 5, 4097, HEAL)
    cor = [one(1, 4, 0, 1), one(1, 6, 4096, 2), one(3, 0, 9, 1)]
    s = torch.cuda.Stream()
    case.run(code, cor, "default")
    torch.cuda.synchronize()
    got, _ = case.run(code, cor, "own stream", stream=s.cuda_stream)
    assert got[:, 1].tolist() == [4, 6] and got[:, 3].tolist() == [0, NONE]
    case.run(code, cor, "library stream", flags=capi.FEC_FLAG_LIBRARY_STREAM)


def test_declines_under_graph_capture():
    code = capi.Code(3, 10)
    case = Case(3, 10, range(10), 5, 1025, HEAL)
    blocks = case.corrupt([one(1, 4, 5, 1), one(1, 5, 5, 1)])
    case.upload(blocks)
    out = torch.zeros(10, dtype=torch.int32, device="cuda")
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="fec_locate2_batch: the stream is being captured into a graph"):
                case.call(code, out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (case.buf.cpu().numpy() == case.lay_in(blocks)).all()


def test_empty_calls():
    """nstripes == 0 touches nothing; sz == 0 answers (CLEAN, NONE)."""
    m = 10
    code = capi.Code(3, m)
    buf = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((10,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code.locate2_batch(buf.data_ptr(), 0, 0, list(range(m)), 16, 0, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == FILL).all()
    want = [FILL] * 2 + [CLEAN] * 3 + [NONE] * 3 + [FILL] * 2
    code.locate2_batch(buf.data_ptr(), 0, 0, list(range(m)), 0, 3, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == want
    host = np.full(10, FILL, dtype=np.uint32)
    code.locate2_batch(buf.data_ptr(), 0, 0, list(range(m)), 0, 3, host.ctypes.data + 8, stream=st)
    assert host.tolist() == want
    assert (buf == 0x5A).all()


def test_pageable_blocks_are_refused():
    blocks = np.zeros(4 * 10 * 64, dtype=np.uint8)
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.FecError, match="fec_locate2_batch takes device or page-locked host memory: src is "
                                            "pageable host memory, which this call does not stage"):
        capi.Code(3, 10).locate2_batch(blocks.ctypes.data, 64, 640, list(range(10)), 64, 4, out.data_ptr())


def test_the_single_block_calls_are_unchanged():
    """On the same buffer fec_locate_batch still answers MANY for a pair, from
    the same kernel, and plane 0 of the new call differs only there."""
    k, m, ns, sz = 3, 10, 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz, HEAL)
    got, _ = case.run(code, [one(1, 4, 5, 1), one(1, 5, 900, 1), one(2, 7, 3, 9)], "pair and single")
    single = torch.full((ns,), -9, dtype=torch.int32, device="cuda")
    code.locate_batch(case.buf.data_ptr() + 3, case.lay.bs, case.lay.ss, case.nums, sz, ns, single.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    assert capi.last_kernel_name() == "matlocate_reg<3,7>"
    torch.cuda.synchronize()
    assert single.cpu().numpy().view(np.uint32).tolist() == [CLEAN, MANY, 7, CLEAN, CLEAN]
    assert got.tolist() == [[CLEAN, 4, 7, CLEAN, CLEAN], [NONE, 5, NONE, NONE, NONE]]


# ---- Python API --------------------------------------------------------------------------

def test_python_api():
    k, m, ns, sz = 3, 10, 70, 4097
    dec = zfec_amd.Decoder(k, m)
    case = Case(k, m, SHUFFLED10, ns, sz, HEAL)
    cor = pair_patterns(m, ns, sz, 9)["mix"] + [whole(68, 2, sz, 1), whole(68, 5, sz, 2)]
    host = case.corrupt(cor)
    want, _ = case.model(host)
    blocks = torch.from_numpy(host).cuda()
    out = dec.locate2_batch(blocks, SHUFFLED10)
    assert out.dtype == torch.int32 and tuple(out.shape) == (2, ns) and out.device == blocks.device
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert out[:, 68].tolist() == [2, 5] and (out[1] == zfec_amd.LOCATE_NONE).any()
    assert (blocks.cpu().numpy() == host).all()
    bm = torch.from_numpy(host).cuda().transpose(0, 1).contiguous().transpose(0, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dec.locate2_batch(bm, SHUFFLED10)
    s.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert tuple(dec.locate2_batch(blocks[:0], SHUFFLED10).shape) == (2, 0)
    empty = dec.locate2_batch(blocks[:, :, :0], SHUFFLED10)
    assert empty.tolist() == [[zfec_amd.LOCATE_CLEAN] * ns, [zfec_amd.LOCATE_NONE] * ns]
