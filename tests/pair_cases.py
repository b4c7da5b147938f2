"""The harness test_gpu_locate2.py and test_gpu_correct2.py share, after
test_gpu_correct.Case: inputs at byte offset 3, the block buffer pre-filled with
random bytes (row slack and surroundings are guards), the two verdict planes
between 0xA5A5A5A5 guard words.  After every call the verdicts are exact, the
ENTIRE block buffer equals the model's blocks laid into the same pre-fill, and
the kernel name is the expected one.  Every expectation comes from
tests/pair_ref.py (the CPU oracle), never from the library."""
import itertools

import numpy as np
import torch

from zfec_amd import capi
from locate_ref import oracle_PQ
from pair_ref import NONE, corrected2, eligible, verdicts2
from test_gpu_correct import kernel_name as correct_name
from test_gpu_locate import kernel_name as locate_name
from test_gpu_verify import IN_OFF, TAIL, Layout, stripes

FILL = 0xA5A5A5A5
GW = 4
SIZES = (1, 15, 16, 17, 1023, 1024, 1025, 4097)
NS = (1, 3, 70)
NSMAX, SZMAX = 70, 4097


def one(s, j, x, v=0x21):
    return (s, j, np.array([x]), np.array([v], dtype=np.uint8))


def whole(s, j, sz, seed):
    return (s, j, np.arange(sz), np.random.default_rng(seed).integers(1, 256, size=sz, dtype=np.uint8))


class Case(object):
    """ns stripes of the blocks `nums` (first k the basis) in one layout;
    heal: fec_correct2_batch, else fec_locate2_batch."""

    def __init__(self, k, m, nums, ns, sz, heal, kind="padded", mem="device"):
        self.k, self.m, self.nums, self.ns, self.sz, self.heal = k, m, list(nums), ns, sz, heal
        self.nb = len(self.nums)
        self.c = self.nb - k
        self.mem = mem
        self.clean = np.ascontiguousarray(stripes(k, m, NSMAX, SZMAX)[:ns][:, self.nums, :sz])
        self.lay = Layout(kind, ns, self.nb, sz)
        self.P, self.Q = oracle_PQ(k, m, tuple(self.nums))
        self.prefill = np.random.default_rng(ns * 131 + sz).integers(
            0, 256, size=IN_OFF + self.lay.nbytes + TAIL, dtype=np.uint8)

    def lay_in(self, blocks):
        host = self.prefill.copy()
        self.lay.view(host[IN_OFF:IN_OFF + self.lay.nbytes])[:, :, :self.sz] = blocks
        return host

    def corrupt(self, corruptions):
        blocks = self.clean.copy()
        for s, j, xs, vs in corruptions:
            blocks[s, j, xs] ^= vs
        return blocks

    def upload(self, blocks):
        t = torch.from_numpy(self.lay_in(blocks))
        self.buf = t.cuda() if self.mem == "device" else t.pin_memory()
        return self.buf

    def model(self, blocks):
        if self.heal:
            return corrected2(self.k, self.m, self.nums, self.P, self.Q, blocks)
        return verdicts2(self.P, self.Q, blocks), blocks

    def name(self):
        if self.sz and eligible(self.k, self.c):
            return "pairs_correct" if self.heal else "pairs_locate"
        return correct_name(self.k) if self.heal else locate_name(self.k, self.c)

    def call(self, code, ptr, stream=None, flags=capi.FEC_FLAG_ASYNC):
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        fn = code.correct2_batch if self.heal else code.locate2_batch
        fn(self.buf.data_ptr() + IN_OFF, self.lay.bs, self.lay.ss, self.nums, self.sz, self.ns, ptr, stream=st,
           flags=flags)

    def run(self, code, corruptions, what, out_mem="device", stream=None, flags=capi.FEC_FLAG_ASYNC, blocks=None):
        """Corrupt (or take `blocks`), call, check everything; returns (the
        verdict planes (2, ns), the model's blocks afterwards)."""
        if blocks is None:
            blocks = self.corrupt(corruptions)
        want, after = self.model(blocks)
        self.upload(blocks)
        n = 2 * self.ns
        words = np.full(GW + n + GW, FILL, dtype=np.uint32)
        if out_mem == "device":
            out = torch.from_numpy(words.view(np.int32)).cuda()
            ptr = out.data_ptr() + 4 * GW
        elif out_mem == "pinned":
            out = torch.from_numpy(words.view(np.int32)).pin_memory()
            ptr = out.data_ptr() + 4 * GW
        else:
            out = words
            ptr = words.ctypes.data + 4 * GW
        if flags & capi.FEC_FLAG_LIBRARY_STREAM:
            torch.cuda.synchronize()  # the library's stream does not wait for the upload's
        self.call(code, ptr, stream, flags)
        got_name = capi.last_kernel_name()
        torch.cuda.synchronize()
        got = out if out_mem == "numpy" else out.cpu().numpy().view(np.uint32)
        assert (got[:GW] == FILL).all() and (got[GW + n:] == FILL).all(), ("guard words", what)
        got = got[GW:GW + n].reshape(2, self.ns).copy()
        assert (got == want).all(), (what, got_name, [(int(p), int(s), hex(got[p, s]), hex(want[p, s]))
                                                      for p, s in np.argwhere(got != want)[:4]])
        have = self.buf.cpu().numpy()
        expect = self.lay_in(after)
        if not (have == expect).all():
            bad = np.nonzero(have != expect)[0]
            raise AssertionError(("block buffer", what, got_name, len(bad), [int(o) - IN_OFF for o in bad[:4]]))
        assert got_name == self.name(), (what, got_name)
        return got, after


def pair_patterns(nb, ns, sz, seed):
    """name -> corruption list: pairs at one byte, at byte 0 of a and byte
    sz - 1 of b (at 4097 in different waves: only the OR across waves refutes
    the other pairs), whole blocks overwritten, single errors and clean stripes
    between them, three blocks at one byte."""
    rng = np.random.default_rng(seed)
    pairs = list(itertools.combinations(range(nb), 2))
    pick = lambda: pairs[int(rng.integers(0, len(pairs)))]  # noqa: E731
    nz = lambda: int(rng.integers(1, 256))  # noqa: E731
    mid = sz // 2
    out = {"clean": []}
    s = ns // 2
    a, b = pick()
    out["one byte"] = [one(s, a, mid, nz()), one(s, b, mid, nz())]
    a, b = pick()
    out["far apart"] = [one(s, a, 0, nz()), one(s, b, sz - 1, nz())] if sz >= 2 else []
    a, b = pick()
    out["whole blocks"] = [whole(s, a, sz, seed), whole(s, b, sz, seed + 1)]
    a, b = pick()
    out["first and last pair"] = [one(0, 0, 0, nz()), one(0, 1, sz - 1, nz()),
                                  one(ns - 1, nb - 2, mid, nz()), one(ns - 1, nb - 1, mid, nz())]
    if nb >= 3:
        t = [int(v) for v in rng.permutation(nb)[:3]]
        out["three at one byte"] = [one(s, j, mid, nz()) for j in t]
    if ns >= 3:
        cor = []
        for t in range(0, ns, 3):  # pair, single, clean, ...
            a, b = pick()
            cor += [one(t, a, int(rng.integers(0, sz)), nz()), one(t, b, int(rng.integers(0, sz)), nz())]
            if t + 1 < ns:
                cor.append(one(t + 1, int(rng.integers(0, nb)), int(rng.integers(0, sz)), nz()))
        out["mix"] = cor
    return {name: cor for name, cor in out.items() if cor or name == "clean"}


def sweep(code, k, m, nums, heal, sizes, nss, seed, kind="padded", mem="device", out_mem="device", flags=None,
          only=None):
    """Every pair pattern at every (ns, sz); returns the set of (first word,
    second word) verdicts seen."""
    seen = set()
    for ns in nss:
        for sz in sizes:
            case = Case(k, m, nums, ns, sz, heal, kind, mem)
            for pname, cor in pair_patterns(len(nums), ns, sz, seed + sz + ns).items():
                if only is not None and pname not in only:
                    continue
                kw = {} if flags is None else {"flags": flags}
                got, _ = case.run(code, cor, (k, m, len(nums), kind, ns, sz, pname), out_mem=out_mem, **kw)
                seen |= set(zip(got[0].tolist(), got[1].tolist()))
    return seen


def saw_pairs(seen):
    assert any(b != NONE for a, b in seen), sorted(seen)
