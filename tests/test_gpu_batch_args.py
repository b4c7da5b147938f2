"""What the five batched scrub / repair / decode calls (fec_decode_batch_mixed,
fec_repair_batch, fec_verify_batch, fec_locate_batch, fec_correct_batch) do
with the memory and the stream they are handed, before any kernel runs: the
refusal of pageable host memory, of buffers on two devices, of a side pointer
(pattern_of / mismatch / culprit) on another device and of a capturing stream,
each with its status and its whole message; and the library's stream with and
without FEC_FLAG_ASYNC.  K=3 / M=10, 2 stripes of 64-byte blocks.

Then the k > 4 fallback of the two pattern-per-stripe calls (K=5 / M=8, 6
stripes of 48-byte blocks, ids [0, 0, 1, 1, 0, 2]): ids from host and from
device memory, and a device-side id that names no pattern."""
import re

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

from test_gpu_mixed import received, stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
FILL = 0xA5A5A5A5 - (1 << 32)  # the guard in every byte of an int32 word
K, M, NS, SZ = 3, 10, 2, 64
PATS = [[2, 0, 5], [7, 8, 9]]  # present blocks of the two patterns
TGTS = [[1, 9], [0, 3]]  # fec_repair_batch's targets
IDS = [0, 1]
NUMS = [0, 1, 2, 3, 4]  # verify / locate / correct: basis 0..2, checks 3 and 4
CALLS = ["mixed", "repair", "verify", "locate", "correct"]

# The messages, typed out from the library's source as it stood before the
# calls shared their plumbing.
PAGEABLE = {
    ("mixed", "src"): "fec_decode_batch_mixed takes device or page-locked host memory: src is pageable host memory, "
                      "which this call does not stage",
    ("mixed", "dst"): "fec_decode_batch_mixed takes device or page-locked host memory: dst is pageable host memory, "
                      "which this call does not stage",
    ("repair", "src"): "fec_repair_batch takes device or page-locked host memory: src is pageable host memory, "
                       "which this call does not stage",
    ("repair", "dst"): "fec_repair_batch takes device or page-locked host memory: dst is pageable host memory, "
                       "which this call does not stage",
    ("verify", "src"): "fec_verify_batch takes device or page-locked host memory: src is pageable host memory, "
                       "which this call does not stage",
    ("locate", "src"): "fec_locate_batch takes device or page-locked host memory: src is pageable host memory, "
                       "which this call does not stage",
    ("correct", "src"): "fec_correct_batch takes device or page-locked host memory: blocks is pageable host memory, "
                        "which this call does not stage",
}
TWO_DEVICES = "batched entry points take memory on one device"
SIDE_ELSEWHERE = {
    "mixed": "pattern_of lives on device 1, the blocks on device 0",
    "repair": "pattern_of lives on device 1, the blocks on device 0",
    "verify": "mismatch lives on device 1, the blocks on device 0",
    "locate": "culprit lives on device 1, the blocks on device 0",
    "correct": "culprit lives on device 1, the blocks on device 0",
}
CAPTURING = {
    "mixed": "fec_decode_batch_mixed: the stream is being captured into a graph (the pattern tables are uploaded "
             "when the call is made)",
    "repair": "fec_repair_batch: the stream is being captured into a graph (the pattern tables are uploaded when "
              "the call is made)",
    "verify": "fec_verify_batch: the stream is being captured into a graph (the call uses memory the library owns "
              "and reuses)",
    "locate": "fec_locate_batch: the stream is being captured into a graph (the call uses memory the library owns "
              "and reuses)",
    "correct": "fec_correct_batch: the stream is being captured into a graph (the call uses memory the library "
               "owns and reuses)",
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


class Args(object):
    """One call's buffers in device memory on cuda:0 and what it is expected to
    leave in them.  src: (NS, rows, SZ) packed; dst (mixed, repair): the output
    rows, pre-filled with the guard; side: pattern_of, or the NS result words
    (pre-filled with the guard).  Stripe 1 of the scrub calls has byte 7 of
    slot 4 (check 1) flipped: mismatch word 2, verdict slot 4, and
    fec_correct_batch puts the byte back."""

    def __init__(self, call):
        self.call = call
        data, allb = stripes(K, M, NS, SZ)
        self.want_dst = self.want_side = None
        if call in ("mixed", "repair"):
            src = received(allb, PATS, IDS, SZ)
            rows = K if call == "mixed" else len(TGTS[0])
            self.dst = torch.full((NS * rows * SZ,), GUARD, dtype=torch.uint8, device="cuda:0")
            self.side = torch.tensor(IDS, dtype=torch.int32, device="cuda:0")
            if call == "mixed":
                self.want_dst = data[:, :, :SZ]
            else:
                self.want_dst = np.stack([allb[s, TGTS[IDS[s]], :SZ] for s in range(NS)])
        else:
            clean = np.ascontiguousarray(allb[:, NUMS, :SZ])
            src = clean.copy()
            src[1, 4, 7] ^= 0x5A
            self.dst = None
            self.side = torch.full((NS,), FILL, dtype=torch.int32, device="cuda:0")
            self.want_side = [0, 2] if call == "verify" else [capi.FEC_LOCATE_CLEAN, 4]
            self.want_src = clean if call == "correct" else src
        self.src_host = np.ascontiguousarray(src)
        self.src = torch.from_numpy(self.src_host).to("cuda:0")

    def run(self, code, src=None, dst=None, side=None, stream=0, flags=capi.FEC_FLAG_ASYNC):
        src = self.src.data_ptr() if src is None else src
        dst = (self.dst.data_ptr() if self.dst is not None else 0) if dst is None else dst
        side = self.side.data_ptr() if side is None else side
        if self.call == "mixed":
            code.decode_batch_mixed(src, SZ, K * SZ, dst, SZ, K * SZ, PATS, side, SZ, NS, stream=stream, flags=flags)
        elif self.call == "repair":
            t = len(TGTS[0])
            code.repair_batch(src, SZ, K * SZ, dst, SZ, t * SZ, PATS, TGTS, side, SZ, NS, stream=stream, flags=flags)
        else:
            fn = {"verify": code.verify_batch, "locate": code.locate_batch, "correct": code.correct_batch}[self.call]
            fn(src, SZ, len(NUMS) * SZ, NUMS, SZ, NS, side, stream=stream, flags=flags)

    def untouched(self):
        """Nothing was written: the outputs hold the guard (pattern_of its ids), the blocks what was uploaded."""
        torch.cuda.synchronize()
        if self.dst is not None:
            return (self.dst.cpu().numpy() == GUARD).all() and self.side.cpu().tolist() == IDS
        return (self.side.cpu().numpy().view(np.uint8) == GUARD).all() and \
            (self.src.cpu().numpy() == self.src_host).all()

    def results(self):
        """(output bytes, result words) after the call."""
        torch.cuda.synchronize()
        if self.dst is not None:
            return self.dst.cpu().numpy().reshape(self.want_dst.shape), None
        return self.src.cpu().numpy(), self.side.cpu().numpy().view(np.uint32).tolist()


def refused(message):
    """The whole text of the FecError of a FEC_EINVAL refusal, as a regular expression."""
    return "^" + re.escape("zfec-hip status %d: %s" % (capi.FEC_EINVAL, message)) + "$"


@pytest.mark.parametrize("call,which", sorted(PAGEABLE))
def test_pageable_memory_is_refused(call, which):
    a = Args(call)
    size = a.src.numel() if which == "src" else a.dst.numel()
    host = np.full(size, GUARD, dtype=np.uint8)
    with pytest.raises(capi.FecError, match=refused(PAGEABLE[call, which])):
        a.run(capi.Code(K, M), **{which: host.ctypes.data})
    assert (host == GUARD).all() and a.untouched()


def test_pageable_src_is_named_before_a_pageable_dst():
    a = Args("mixed")
    host = np.full(a.src.numel() + a.dst.numel(), GUARD, dtype=np.uint8)
    with pytest.raises(capi.FecError, match=refused(PAGEABLE["mixed", "src"])):
        a.run(capi.Code(K, M), src=host.ctypes.data, dst=host.ctypes.data + a.src.numel())
    assert (host == GUARD).all()


def two_gpus():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")


@pytest.mark.parametrize("call", ["mixed", "repair"])
def test_src_and_dst_on_two_devices_are_refused(call):
    two_gpus()
    a = Args(call)
    other = torch.full((a.dst.numel(),), GUARD, dtype=torch.uint8, device="cuda:1")
    with pytest.raises(capi.FecError, match=refused(TWO_DEVICES)):
        a.run(capi.Code(K, M), dst=other.data_ptr())
    assert (other.cpu().numpy() == GUARD).all() and a.untouched()


@pytest.mark.parametrize("call", CALLS)
def test_side_pointer_on_another_device_is_refused(call):
    two_gpus()
    a = Args(call)
    other = a.side.to("cuda:1")
    with pytest.raises(capi.FecError, match=refused(SIDE_ELSEWHERE[call])):
        a.run(capi.Code(K, M), side=other.data_ptr())
    assert (other.cpu() == a.side.cpu()).all() and a.untouched()


@pytest.mark.parametrize("call", CALLS)
def test_capturing_stream_is_refused(call):
    a = Args(call)
    code = capi.Code(K, M)
    x = torch.zeros(16, device="cuda:0")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device="cuda:0")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match=refused(CAPTURING[call])):
                a.run(code, stream=s.cuda_stream)
    assert a.untouched()


@pytest.mark.parametrize("call", CALLS)
def test_library_stream_with_and_without_async(call):
    """FEC_FLAG_LIBRARY_STREAM alone returns when the work is done; with
    FEC_FLAG_ASYNC the caller waits for the device.  The same bytes either way,
    and the expected ones."""
    code = capi.Code(K, M)
    got = []
    for flags in (capi.FEC_FLAG_LIBRARY_STREAM, capi.FEC_FLAG_LIBRARY_STREAM | capi.FEC_FLAG_ASYNC):
        a = Args(call)
        torch.cuda.synchronize()
        a.run(code, flags=flags)
        got.append(a.results())
    (bytes_a, words_a), (bytes_b, words_b) = got
    assert (bytes_a == bytes_b).all() and words_a == words_b, call
    if a.want_dst is not None:
        assert (bytes_a == a.want_dst).all(), call
    else:
        assert words_a == a.want_side and (bytes_a == a.want_src).all(), call


# ---- the k > 4 fallback: runs of stripes with one id ---------------------------------------
WK, WM, WNS, WSZ = 5, 8, 6, 48
WIDS = [0, 0, 1, 1, 0, 2]
WPRES = [[0, 1, 2, 3, 4], [7, 5, 3, 1, 6], [2, 7, 4, 0, 6]]
WTGTS = [[5, 6], [0, capi.FEC_REPAIR_NONE], [3, 1]]


def wide_run(call, ids, where):
    """Run `call` over the received blocks laid out by WIDS with pattern ids
    `ids`; the output rows (WNS, rows, WSZ), pre-filled with the guard."""
    data, allb = stripes(WK, WM, WNS, WSZ)
    src = torch.from_numpy(received(allb, WPRES, WIDS, WSZ)).cuda()
    rows = WK if call == "mixed" else len(WTGTS[0])
    dst = torch.full((WNS, rows, WSZ), GUARD, dtype=torch.uint8, device="cuda")
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    keep = torch.from_numpy(ids.view(np.int32)).cuda() if where == "device" else ids
    ptr = keep.data_ptr() if where == "device" else ids.ctypes.data
    code = capi.Code(WK, WM)
    st = torch.cuda.current_stream().cuda_stream
    if call == "mixed":
        code.decode_batch_mixed(src.data_ptr(), WSZ, WK * WSZ, dst.data_ptr(), WSZ, rows * WSZ, WPRES, ptr, WSZ, WNS,
                                stream=st)
    else:
        code.repair_batch(src.data_ptr(), WSZ, WK * WSZ, dst.data_ptr(), WSZ, rows * WSZ, WPRES, WTGTS, ptr, WSZ, WNS,
                          stream=st)
    assert not capi.last_kernel_name().startswith(("matapply_mixed", "matrepair_mixed"))
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def wide_want(call, ids):
    """The oracle's rows; the guard for a NONE target and for a stripe whose id names no pattern."""
    data, allb = stripes(WK, WM, WNS, WSZ)
    rows = WK if call == "mixed" else len(WTGTS[0])
    want = np.full((WNS, rows, WSZ), GUARD, dtype=np.uint8)
    for s, i in enumerate(ids):
        if i >= len(WPRES):
            continue
        if call == "mixed":
            want[s] = data[s]
            continue
        for r, b in enumerate(WTGTS[i]):
            if b != capi.FEC_REPAIR_NONE:
                want[s, r] = allb[s, b]
    return want


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("call", ["mixed", "repair"])
def test_fallback_runs_of_one_id(call, where):
    assert (wide_run(call, WIDS, where) == wide_want(call, WIDS)).all()


@pytest.mark.parametrize("call", ["mixed", "repair"])
def test_fallback_device_id_out_of_range_leaves_the_stripe(call):
    ids = list(WIDS)
    ids[3] = len(WPRES)
    got, want = wide_run(call, ids, "device"), wide_want(call, ids)
    assert (want[3] == GUARD).all()
    assert (got == want).all()
