"""Single-stripe launches of the register kernels (zfec_amd/csrc/kernels.hip,
reg_body_one: one 16-byte unit per lane, no walk; for K*R*5 >= 50 table dwords
with each row's tables requested one row ahead).  Every result is compared byte
for byte with the CPU oracle.

* shapes (K,R): (1,1) and (3,3) keep their tables in registers, (2,5) has
  exactly 50 table dwords (the threshold), (3,7) and (4,8) are past it;
* sizes around one chunk, the shifted-back last chunk, one workgroup (4096),
  a second workgroup that holds only the shifted-back chunk (4097), and 15
  bytes, which stays on the walking form;
* outputs 16-byte aligned (stored nt sc1) and at 6 (mod 16) (stored nt), with
  64 guard bytes before and after every output row;
* the same launches in a fresh process with ZFEC_HIP_GRID_CAP=1 (one
  workgroup: the grid-stride walk) must give the same bytes;
* ns = 1 through the batched entry points with FEC_FLAG_ROW_PADDING.

Run as a script (the child of the grid-stride test) it writes every launch's
whole output buffer to the .npy file named on the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import zfec_amd  # noqa: E402
from zfec_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ROOM = 64  # guard bytes before and after every output row
SHAPES = ((1, 1), (3, 3), (2, 5), (3, 7), (4, 8))
SIZES = (15, 16, 17, 31, 32, 1023, 1024, 1025, 4096, 4097, 4111, 8192 + 5)
OUT_OFFS = (0, 6)


def row_stride(sz):
    """Rows 16 bytes apart modulo 16, ROOM guard bytes after one and before the next."""
    return (sz + 15) // 16 * 16 + 2 * ROOM


def inputs(k, sz):
    return np.random.default_rng(1000 * k + sz).integers(0, 256, size=(k, sz), dtype=np.uint8)


def cases():
    """(op, K, R, sz, out_off): every shape's encode, and for R <= K the decode
    of R lost primaries from the K/(K+R) code's R check blocks."""
    for K, R in SHAPES:
        for op in ("enc", "dec") if R <= K else ("enc",):
            for sz in SIZES:
                for off in OUT_OFFS:
                    yield op, K, R, sz, off


def launch_case(torch, code, op, K, R, sz, off, enc_out=None):
    """One launch over device buffers; returns (kernel name, the whole output
    buffer).  A decode's inputs are the encode's expected check blocks in the
    slots of the lost primaries 0..R-1."""
    ld = row_stride(sz)
    blocks = inputs(K, sz)
    if op == "dec":
        blocks = np.concatenate([enc_out, blocks[R:]])
        index = list(range(K, K + R)) + list(range(R, K))
    else:
        index = list(range(K, K + R))
    src = torch.zeros(3 + K * ld, dtype=torch.uint8, device="cuda")
    src[3:].view(K, ld)[:, :sz] = torch.from_numpy(np.ascontiguousarray(blocks)).cuda()
    dst = torch.full((256 + R * ld,), GUARD, dtype=torch.uint8, device="cuda")
    sp, dp = src.data_ptr() + 3, dst.data_ptr() + ROOM + off
    assert dst.data_ptr() % 16 == 0
    f = code.encode_ptrs if op == "enc" else code.decode_ptrs
    f([sp + j * ld for j in range(K)], [dp + i * ld for i in range(R)], index, sz,
      stream=torch.cuda.current_stream().cuda_stream)
    name = capi.last_kernel_name()
    torch.cuda.synchronize()
    return name, dst.cpu().numpy()


def expected(op, K, R, sz):
    from oracle import oracle

    data = inputs(K, sz)
    par = oracle.encode(K, K + R, data)
    if op == "enc":
        return par, par
    recv = np.concatenate([par, data[R:]])
    index = list(range(K, K + R)) + list(range(R, K))
    want = oracle.decode(K, K + R, recv, index)
    assert (want == data[:R]).all()
    return want, par


def run_all(with_oracle):
    """Every case's kernel name and output buffer (and the expected rows).
    The child process runs without the oracle: a decode's inputs are then the
    encode's own output rows, which the parent has checked."""
    import torch

    prev = capi.jit_mode(capi.JIT_OFF)
    try:
        out, codes = {}, {}
        for op, K, R, sz, off in cases():
            code = codes.setdefault((K, R), capi.Code(K, K + R))
            if with_oracle:
                want, par = expected(op, K, R, sz)
            else:
                want = None
                par = rows_of(out[("enc", K, R, sz, off)][1], R, sz, off) if op == "dec" else None
            name, buf = launch_case(torch, code, op, K, R, sz, off, par)
            out[(op, K, R, sz, off)] = (name, buf, want)
        return out
    finally:
        capi.jit_mode(prev)


def rows_of(buf, R, sz, off):
    ld = row_stride(sz)
    return np.stack([buf[ROOM + off + i * ld:][:sz] for i in range(R)])


@pytest.fixture(scope="module")
def results():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return run_all(True)


@pytest.mark.parametrize("K,R", SHAPES)
def test_bytes_guards_and_names(results, K, R):
    """Bytes [0, sz) of every row equal the oracle's, every other byte of the
    output buffer (64 or more before and after each row) is untouched, and the
    launch reports matapply_reg<K,R>."""
    seen = 0
    for (op, k, r, sz, off), (name, buf, want) in results.items():
        if (k, r) != (K, R):
            continue
        seen += 1
        what = (op, K, R, sz, off, name)
        assert name == "matapply_reg<%d,%d>" % (K, R), what
        ld = row_stride(sz)
        mask = np.ones(buf.shape, dtype=bool)
        for i in range(R):
            o = ROOM + off + i * ld
            mask[o:o + sz] = False
            assert (buf[o - ROOM:o] == GUARD).all() and (buf[o + sz:o + sz + ROOM] == GUARD).all(), what
        assert (buf[mask] == GUARD).all(), ("write outside the rows", what)
        assert np.array_equal(rows_of(buf, R, sz, off), want), what
    assert seen == len(SIZES) * len(OUT_OFFS) * (2 if R <= K else 1)


def test_grid_stride_walk_gives_the_same_bytes(results, tmp_path):
    """ZFEC_HIP_GRID_CAP=1 in a fresh process (the knob is read once): every
    launch is one workgroup walking grid-stride, the form these launches took
    before.  Names and whole output buffers, guard bytes included, must match."""
    out = tmp_path / "walk.npy"
    env = dict(os.environ, ZFEC_HIP_GRID_CAP="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True,
                         text=True, timeout=110)
    assert res.returncode == 0, res.stderr[-2000:]
    names = res.stdout.split()
    walked = np.load(out)
    assert names == [v[0] for v in results.values()]
    assert np.array_equal(walked, np.concatenate([v[1] for v in results.values()]))


@pytest.mark.parametrize("K,R", [(3, 7), (3, 3)])
def test_row_padding_single_stripe_batch(K, R):
    """ns = 1 through fec_encode_batch / fec_decode_batch with
    FEC_FLAG_ROW_PADDING, sz = 1000 in rows 1024 apart: the library may run the
    rows out to 1024 bytes.  Bytes [0, sz) are exact; the guard bytes before
    the first row and past the last row's stride are untouched."""
    import torch
    from oracle import oracle

    sz, ld = 1000, 1024
    M = K + R
    data = inputs(K, sz)
    par = oracle.encode(K, M, data)
    code = capi.Code(K, M)
    st = torch.cuda.current_stream().cuda_stream
    fl = capi.FEC_FLAG_ASYNC | capi.FEC_FLAG_ROW_PADDING
    prev = capi.jit_mode(capi.JIT_OFF)
    try:
        for op in ("enc", "dec") if R <= K else ("enc",):
            if op == "enc":
                blocks, index, want = data, list(range(K, M)), par
            else:
                blocks, index, want = np.concatenate([par, data[R:]]), list(range(K, M)) + list(range(R, K)), data[:R]
            host = np.full((K, ld), 0x3C, dtype=np.uint8)  # input padding the library may read
            host[:, :sz] = blocks
            src = torch.from_numpy(host).cuda()
            front = 2 * ROOM  # rows on 128-byte lines
            dst = torch.full((front + R * ld + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
            f = code.encode_batch if op == "enc" else code.decode_batch
            f(src.data_ptr(), ld, K * ld, dst.data_ptr() + front, ld, R * ld, index, sz, 1, stream=st, flags=fl)
            name = capi.last_kernel_name()
            torch.cuda.synchronize()
            buf = dst.cpu().numpy()
            assert name == "matapply_reg<%d,%d>" % (K, R), (op, name)
            assert (buf[:front] == GUARD).all() and (buf[front + R * ld:] == GUARD).all(), (op, "write outside the rows")
            assert np.array_equal(buf[front:front + R * ld].reshape(R, ld)[:, :sz], want), op
    finally:
        capi.jit_mode(prev)


if __name__ == "__main__":
    done = run_all(False)
    np.save(sys.argv[1], np.concatenate([v[1] for v in done.values()]))
    print(" ".join(v[0] for v in done.values()))
