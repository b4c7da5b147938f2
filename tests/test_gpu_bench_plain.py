"""A plain `bench.py --gpus 1 --steps N --warmup W` run: it times the steps and
prints the headline line without the --full legs, and --dump-outputs writes
what the last timed step computed.  One run serves both tests; its inputs come
from a fixed seed, so the test regenerates them and checks the dumped parity
against the CPU oracle and the dumped recovered blocks against the input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import zfec_amd
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, M, STEPS = 3, 10, 4
SZ = -(-(64 << 20) // K)  # cfg2: one 64 MiB stripe


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    d = tmp_path_factory.mktemp("dump")
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", "1", "--dump-outputs", str(d)], env=env, capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-3000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-3000:]
    return json.loads(lines[0]), d


def test_plain_run_prints_the_headline_only(plain_run):
    out, _ = plain_run
    assert out["unit"] == "GB/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["metric"].startswith("encode+decode GB/s")
    assert out["steps"] == STEPS and out["full"] is False
    assert out["ms_per_step"] > 0
    # value = input bytes of both directions per step / the step's time (ms_per_step is rounded to 1e-4 ms)
    want = 2 * K * SZ / (out["ms_per_step"] * 1e-3) / 1e9
    assert abs(out["value"] - want) <= want * (1e-4 / out["ms_per_step"] + 1e-4)
    for leg in ("roofline", "decode_roofline", "valu_roofline", "decode_fresh_pattern", "batched_1MiB",
                "first_seen_decode", "first_launch_encode", "cpu_baseline"):
        assert leg not in out, leg


def test_dumped_outputs_are_the_last_steps(plain_run):
    import torch

    import bench

    _, d = plain_run
    assert sorted(os.listdir(d)) == ["parity.npy", "recovered.npy"]
    par, rec = np.load(d / "parity.npy"), np.load(d / "recovered.npy")
    assert par.dtype == np.float32 and rec.dtype == np.float32
    assert par.nbytes + rec.nbytes <= 64 << 20
    # the bench's input (run_workload: seed 1234 + k, rows padded to the row stride)
    ld = bench.row_stride(SZ)
    gen = torch.Generator(device="cuda").manual_seed(1234 + K)
    data = torch.randint(0, 256, (1, K, ld), dtype=torch.uint8, device="cuda", generator=gen)[0, :, :SZ].cpu().numpy()
    # the decode recovers all k primaries from blocks m-k..m-1
    assert np.array_equal(rec, data.reshape(-1)[bench.dump_positions(K * SZ)].astype(np.float32))
    # parity byte c of a block depends on byte c of the k inputs alone: the oracle encodes the sampled columns
    row, col = np.divmod(bench.dump_positions((M - K) * SZ), SZ)
    want = oracle.encode(K, M, np.ascontiguousarray(data[:, col]))
    assert np.array_equal(par, want[row, np.arange(len(col))].astype(np.float32))
