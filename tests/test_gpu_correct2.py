"""GPU checks of pair correction (fec_correct2_batch: fec_locate2_batch's
path with the single-block correction of fec_correct_batch after
locate2_finish and zfec_amd/csrc/kernels.hip pairs_correct at the end).  The
harness is tests/pair_cases.py: expected verdicts and expected blocks from the
numpy model (tests/pair_ref.py), the ENTIRE block buffer compared after every
call (healed slots, untouched stripes, slack and guards in one comparison),
guard words around the two verdict planes, the kernel name checked."""
import itertools

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from locate_ref import CLEAN, MANY
from pair_cases import FILL, NS, SIZES, Case, one, pair_patterns, saw_pairs, sweep, whole
from pair_ref import NONE
from test_gpu_locate2 import SHUFFLED10, every_pair_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HEAL = True


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def verify_bits(code, case):
    """fec_verify_batch on the case's buffer as it stands: bool (ns,), any bit."""
    words = (case.c + 31) // 32
    mask = torch.zeros(case.ns * words, dtype=torch.int32, device="cuda")
    code.verify_batch(case.buf.data_ptr() + 3, case.lay.bs, case.lay.ss, case.nums, case.sz, case.ns, mask.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return mask.cpu().numpy().reshape(case.ns, words).any(axis=1)


# ---- sizes, batches, codes ---------------------------------------------------------------------

@pytest.mark.parametrize("nums", [list(range(10)), SHUFFLED10], ids=["in order", "shuffled"])
def test_all_sizes_and_batches(nums):
    """As test_gpu_locate2: every size at three stripes, one stripe and 70 at a
    size of each kind (byte tail, overlapped last chunk, exact wave, five
    waves)."""
    code = capi.Code(3, 10)
    assert NS == (1, 3, 70)
    seen = sweep(code, 3, 10, nums, HEAL, SIZES, (3,), seed=410)
    seen |= sweep(code, 3, 10, nums, HEAL, (1, 17, 1024, 4097), (1, 70), seed=411)
    saw_pairs(seen)
    assert {(CLEAN, NONE), (MANY, NONE)} <= seen and any(a < 10 and b == NONE for a, b in seen)


@pytest.mark.parametrize("k,m,nb", [(1, 6, 5), (4, 12, 12), (10, 16, 16)])
def test_codes(k, m, nb):
    nums = list(range(nb))
    seen = sweep(capi.Code(k, m), k, m, nums, HEAL, SIZES, (3,), seed=300 * k + m)
    seen |= sweep(capi.Code(k, m), k, m, nums, HEAL, (17, 1025), (1, 70), seed=400 * k + m)
    saw_pairs(seen)


def test_both_in_the_basis_one_each_and_both_checks():
    """The three forms of the 2 x k rows, K=10/M=16 shuffled: both lost slots in
    the basis, one of them, none."""
    k, m = 10, 16
    nums = np.random.default_rng(16).permutation(m).tolist()
    sz = 1025
    cor = []
    for s, (a, b) in enumerate(((0, 9), (3, 4), (2, 10), (9, 15), (0, 11), (10, 11), (12, 15), (10, 15))):
        cor += [whole(s, a, sz, s), one(s, b, (97 * s) % sz, 1 + s)]
    case = Case(k, m, nums, 8, sz, HEAL)
    got, after = case.run(capi.Code(k, m), cor, "forms")
    assert (got[1] != NONE).all() and (after == case.clean).all()


def test_the_limit_of_32_blocks():
    k, m = 20, 60
    nums = np.random.default_rng(2060).permutation(m)[:32].tolist()
    seen = sweep(capi.Code(k, m), k, m, nums, HEAL, (17, 1025), (3,), seed=2061,
                 only=("clean", "one byte", "far apart", "whole blocks"))
    saw_pairs(seen)
    case = Case(k, m, nums, 2, 64, HEAL)
    got, after = case.run(capi.Code(k, m), [one(1, 30, 5), one(1, 31, 9)], "the last pair")
    assert got[:, 1].tolist() == [30, 31] and (after == case.clean).all()


@pytest.mark.parametrize("k,m,nb", [(20, 60, 33), (3, 10, 6)])
def test_pair_pass_off(k, m, nb):
    """Two corrupt blocks stay (MANY, NONE) and nothing is written for them;
    single errors are healed as fec_correct_batch heals them."""
    nums = np.random.default_rng(nb).permutation(m)[:nb].tolist()
    seen = sweep(capi.Code(k, m), k, m, nums, HEAL, (17, 1025), (3,), seed=nb,
                 only=("clean", "one byte", "far apart", "whole blocks", "mix"))
    assert (MANY, NONE) in seen and all(b == NONE for a, b in seen)


@pytest.mark.parametrize("kind", ["packed", "bm"])
def test_layouts(kind):
    saw_pairs(sweep(capi.Code(3, 10), 3, 10, SHUFFLED10, HEAL, (15, 1025, 4097), (3, 70), seed=87, kind=kind))
    saw_pairs(sweep(capi.Code(10, 16), 10, 16, list(range(16)), HEAL, (1025,), (3,), seed=88, kind=kind))


# ---- every pair, triples, list walks ----------------------------------------------------------

@pytest.mark.parametrize("sz", [16, 4097])
def test_every_pair(sz):
    """Every pair of K=3/M=10 healed in one batch, single errors beside them;
    afterwards no stripe has a verify bit and a second call answers CLEAN and
    writes nothing."""
    ns, cor = every_pair_case(sz)
    code = capi.Code(3, 10)
    case = Case(3, 10, range(10), ns, sz, HEAL)
    got, after = case.run(code, cor, "every pair")
    assert [tuple(v) for v in got[:, :45].T.tolist()] == list(itertools.combinations(range(10), 2))
    assert (after == case.clean).all()
    assert not verify_bits(code, case).any()
    again, after2 = case.run(code, None, "second call", blocks=after)
    assert (again[0] == CLEAN).all() and (again[1] == NONE).all() and (after2 == after).all()


def test_verify_passes_after_any_verdict():
    """Whatever the corruption was -- pairs, triples at one byte (MANY with
    c = 7, possibly a pair with c = 4), whole blocks -- every stripe that got a
    slot or a pair verdict has no verify bit afterwards, and the others keep
    theirs."""
    for k, m, nb in ((3, 10, 10), (3, 10, 7), (1, 6, 5)):
        ns, sz = 70, 1025
        rng = np.random.default_rng(nb)
        cor = []
        for s in range(ns):
            for j in rng.permutation(nb)[:s % 4]:
                cor.append(one(s, int(j), 500 if s % 2 else int(rng.integers(0, sz)), int(rng.integers(1, 256))))
        code = capi.Code(k, m)
        case = Case(k, m, range(nb), ns, sz, HEAL)
        got, _ = case.run(code, cor, ("zero to three errors", nb))
        healed = got[0] < nb
        bits = verify_bits(code, case)
        assert not bits[healed].any() and bits[got[0] == MANY].all() and healed.any()


def test_three_at_one_byte():
    ns, sz = 70, 1025
    triples = list(itertools.combinations(range(10), 3))[1::2][:ns]
    cor = [one(s, j, 513, 1 + 3 * s + j) for s, tr in enumerate(triples) for j in tr]
    case = Case(3, 10, range(10), ns, sz, HEAL)
    got, after = case.run(capi.Code(3, 10), cor, "triples")
    assert (got[0, :len(triples)] == MANY).all() and (got[1] == NONE).all() and (after == case.corrupt(cor)).all()


@pytest.mark.parametrize("cap", [3, 1])
def test_list_walk(knobs, cap):
    knobs(ZFEC_HIP_GRID_CAP=cap)
    code = capi.Code(3, 10)
    for sz in (1025, 4097):
        ns, cor = every_pair_case(sz)
        cor = [c for c in cor if c[0] < 45]
        for s in range(45, ns):
            cor += [one(s, s % 9, 0, 5), whole(s, 9, sz, s)]
        case = Case(3, 10, range(10), ns, sz, HEAL)
        got, after = case.run(code, cor, ("all dirty", cap, sz))
        assert (got[1] != NONE).all() and (after == case.clean).all()
        got, after = case.run(code, [one(69, 2, 0, 1), one(69, 8, sz - 1, 1)], ("one dirty", cap, sz))
        assert got[:, 69].tolist() == [2, 8] and (got[0, :69] == CLEAN).all() and (after == case.clean).all()


def test_all_clean():
    for k, m, nb in ((3, 10, 10), (10, 16, 16)):
        got, _ = Case(k, m, range(nb), 70, 4097, HEAL).run(capi.Code(k, m), [], "clean")
        assert (got[0] == CLEAN).all() and (got[1] == NONE).all()


# ---- memory kinds, streams, refusals ---------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
@pytest.mark.parametrize("out_mem", ["numpy", "pinned"])
def test_culprit_in_host_memory(k, m, out_mem):
    """The verdict planes are gathered in device words the library owns, which
    both corrections read, and copied back."""
    code = capi.Code(k, m)
    for flags in (capi.FEC_FLAG_ASYNC, 0, capi.FEC_FLAG_LIBRARY_STREAM):
        saw_pairs(sweep(code, k, m, list(range(m)), HEAL, (1025,), (37,), seed=5, out_mem=out_mem, flags=flags))


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_blocks_in_page_locked_host_memory(k, m):
    """Read and healed in place, by plain stores."""
    code = capi.Code(k, m)
    for out_mem in ("device", "numpy"):
        saw_pairs(sweep(code, k, m, list(range(m)), HEAL, (1025,), (5,), seed=6, mem="pinned", out_mem=out_mem,
                        flags=0))


def test_streams():
    code = capi.Code(3, 10)
    case = Case(3, 10, range(10), 5, 4097, HEAL)
    cor = [one(1, 4, 0, 1), one(1, 6, 4096, 2), one(3, 0, 9, 1)]
    s = torch.cuda.Stream()
    case.run(code, cor, "default")
    torch.cuda.synchronize()
    got, after = case.run(code, cor, "own stream", stream=s.cuda_stream)
    assert got[:, 1].tolist() == [4, 6] and got[:, 3].tolist() == [0, NONE] and (after == case.clean).all()
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
            with pytest.raises(capi.FecError, match="fec_correct2_batch: the stream is being captured into a graph"):
                case.call(code, out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (case.buf.cpu().numpy() == case.lay_in(blocks)).all()


def test_empty_calls():
    m = 10
    code = capi.Code(3, m)
    buf = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((10,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code.correct2_batch(buf.data_ptr(), 0, 0, list(range(m)), 16, 0, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == FILL).all()
    want = [FILL] * 2 + [CLEAN] * 3 + [NONE] * 3 + [FILL] * 2
    code.correct2_batch(buf.data_ptr(), 0, 0, list(range(m)), 0, 3, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == want
    host = np.full(10, FILL, dtype=np.uint32)
    code.correct2_batch(buf.data_ptr(), 0, 0, list(range(m)), 0, 3, host.ctypes.data + 8, stream=st)
    assert host.tolist() == want
    assert (buf == 0x5A).all()


def test_pageable_blocks_are_refused():
    blocks = np.zeros(4 * 10 * 64, dtype=np.uint8)
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.FecError, match="fec_correct2_batch takes device or page-locked host memory: blocks is "
                                            "pageable host memory, which this call does not stage"):
        capi.Code(3, 10).correct2_batch(blocks.ctypes.data, 64, 640, list(range(10)), 64, 4, out.data_ptr())
    assert not blocks.any()


def test_single_errors_are_healed_as_by_correct_batch():
    """Without a pair in the batch the bytes and plane 0 are those of
    fec_correct_batch, which still reports its own kernel."""
    k, m, ns, sz = 3, 10, 37, 1025
    code = capi.Code(k, m)
    case = Case(k, m, SHUFFLED10, ns, sz, HEAL)
    cor = [one(s, s % m, (31 * s) % sz, 1 + s) for s in range(0, ns, 2)]
    got, after = case.run(code, cor, "singles")
    assert (got[0, ::2] == np.arange(0, ns, 2) % m).all() and (after == case.clean).all()
    case.upload(case.corrupt(cor))
    single = torch.full((ns,), -9, dtype=torch.int32, device="cuda")
    code.correct_batch(case.buf.data_ptr() + 3, case.lay.bs, case.lay.ss, case.nums, sz, ns, single.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    assert capi.last_kernel_name() == "matcorrect_reg<3>"
    torch.cuda.synchronize()
    assert (single.cpu().numpy().view(np.uint32) == got[0]).all()
    assert (case.buf.cpu().numpy() == case.lay_in(after)).all()


# ---- Python API --------------------------------------------------------------------------

def test_python_api():
    k, m, ns, sz = 3, 10, 70, 4097
    dec = zfec_amd.Decoder(k, m)
    case = Case(k, m, SHUFFLED10, ns, sz, HEAL)
    cor = pair_patterns(m, ns, sz, 9)["mix"] + [whole(68, 2, sz, 1), whole(68, 5, sz, 2)]
    host = case.corrupt(cor)
    want, after = case.model(host)
    assert (after == case.clean).all()
    blocks = torch.from_numpy(host).cuda()
    out = dec.correct2_batch(blocks, SHUFFLED10)
    assert out.dtype == torch.int32 and tuple(out.shape) == (2, ns) and out.device == blocks.device
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert out[:, 68].tolist() == [2, 5]
    assert (blocks.cpu().numpy() == case.clean).all()
    assert not dec.verify_batch(blocks, SHUFFLED10).any()
    again = dec.correct2_batch(blocks, SHUFFLED10)
    assert (again[0] == zfec_amd.LOCATE_CLEAN).all() and (again[1] == zfec_amd.LOCATE_NONE).all()
    bm = torch.from_numpy(host).cuda().transpose(0, 1).contiguous().transpose(0, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dec.correct2_batch(bm, SHUFFLED10)
    s.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == want).all() and (bm.cpu().numpy() == case.clean).all()
    assert tuple(dec.correct2_batch(blocks[:0], SHUFFLED10).shape) == (2, 0)
    empty = dec.correct2_batch(blocks[:, :, :0], SHUFFLED10)
    assert empty.tolist() == [[zfec_amd.LOCATE_CLEAN] * ns, [zfec_amd.LOCATE_NONE] * ns]
