"""Shared by the GPU tests of the run-time-data bit-sliced kernels
(test_gpu_bsr.py, test_gpu_bsg.py): one batched encode or decode call over
device buffers laid out [stripe][block][ld] from odd bases at an odd row
stride, the output pre-filled with 0xA5, and the CPU oracle's rows for it."""
import numpy as np
import pytest

from zfec_amd import capi
from oracle import oracle

torch = pytest.importorskip("torch")

GUARD = 0xA5
IN_OFF, OUT_OFF, TAIL = 5, 3, 64


def flat(blocks):
    """(ns, rows, sz) -> (rows, ns * sz): output byte x depends only on byte x
    of the inputs, so the oracle takes a batch as one long stripe."""
    ns, rows, sz = blocks.shape
    return np.ascontiguousarray(blocks.transpose(1, 0, 2)).reshape(rows, ns * sz)


def unflat(rows2d, ns):
    rows, n = rows2d.shape
    return np.ascontiguousarray(rows2d.reshape(rows, ns, n // ns).transpose(1, 0, 2))


def encode_case(k, m, data, nums=None):
    """Inputs (ns, k, sz), the oracle's rows (ns, r, sz) and the index of an
    encode of the blocks `nums` (every parity block by default)."""
    nums = list(range(k, m)) if nums is None else list(nums)
    return data, unflat(oracle.encode(k, m, flat(data), nums), data.shape[0]), nums


def decode_case(k, m, data, slots):
    """The same for a decode from the blocks `slots` (slot order): the inputs
    are the oracle's encode, the rows the oracle's decode, which must equal the
    lost primaries."""
    ns = data.shape[0]
    f = flat(data)
    recv = np.ascontiguousarray(np.concatenate([f, oracle.encode(k, m, f)])[list(slots)])
    want = oracle.decode(k, m, recv, slots)
    assert (want == f[[i for i in range(k) if slots[i] >= k]]).all()
    return unflat(recv, ns), unflat(want, ns), list(slots)


class Batch(object):
    """One call: op "enc" or "dec", blocks (ns, k, sz), rows 12 or 13 bytes
    past sz apart, whichever is odd."""

    def __init__(self, k, m, op, index, blocks, r):
        self.op, self.index, self.r = op, index, r
        self.ns, self.k, self.sz = blocks.shape
        assert self.k == k
        self.ld = ld = (self.sz + 12) | 1
        assert ld % 2 == 1 and IN_OFF % 2 == 1 and OUT_OFF % 2 == 1
        self.code = capi.Code(k, m)
        n_in = self.ns * k * ld
        self.src = torch.zeros(IN_OFF + n_in + TAIL, dtype=torch.uint8, device="cuda")
        self.src[IN_OFF:IN_OFF + n_in].view(self.ns, k, ld)[:, :, :self.sz] = \
            torch.from_numpy(np.ascontiguousarray(blocks)).cuda()
        self.dst = torch.empty(OUT_OFF + self.ns * r * ld + TAIL, dtype=torch.uint8, device="cuda")

    def launch(self):
        """Refill the output, make the call, return the last kernel's name."""
        self.dst.fill_(GUARD)
        f = self.code.encode_batch if self.op == "enc" else self.code.decode_batch
        ld = self.ld
        f(self.src.data_ptr() + IN_OFF, ld, self.k * ld, self.dst.data_ptr() + OUT_OFF, ld, self.r * ld, self.index,
          self.sz, self.ns, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return capi.last_kernel_name()

    def rows(self, what=""):
        """The output rows (ns, r, sz), once the bytes before, between and
        after them have been found untouched."""
        host = self.dst.cpu().numpy()
        n = self.ns * self.r * self.ld
        assert (host[:OUT_OFF] == GUARD).all(), ("write before the output", what)
        assert (host[OUT_OFF + n:] == GUARD).all(), ("write after the output", what)
        body = host[OUT_OFF:OUT_OFF + n].reshape(self.ns, self.r, self.ld)
        assert (body[:, :, self.sz:] == GUARD).all(), ("write past a row", what)
        return body[:, :, :self.sz]


def check_rows(got, want, what):
    """Every stripe bit-exact; the message names the first wrong stripes and
    says whether their bytes were left untouched."""
    if (got == want).all():
        return
    bad = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
    untouched = [s for s in bad if (got[s][got[s] != want[s]] == GUARD).all()]
    raise AssertionError((what, "wrong stripes", bad[:8], "of them only untouched bytes", untouched[:8]))


def walk_steps(total, cps, cap):
    """The fewest iterations a workgroup makes when `cap` workgroups walk
    `total` units of cps per (virtual) stripe; the carry must be in play."""
    assert cap % cps != 0, "gs_c == 0: the walk never carries"
    assert total >= 3 * cap, (total, cap)
    return total // cap
