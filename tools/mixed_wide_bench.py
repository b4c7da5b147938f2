#!/usr/bin/env python3
"""Pattern-per-stripe decode and repair on wide codes: the one-launch mix form
of matapply_bsr (fec_decode_batch_mixed / fec_repair_batch as shipped, and the
planned call over records built once) against the shared-pattern call on the
same buffers (the ceiling) and against the parent commit's run path.

Shapes (device-resident, ids on the device):
  a         1024 K=20/M=60 stripes of 1 MiB (blocks of 52,429 B), 1024 distinct
            random patterns
  b         2*10^5 K=10/M=16 stripes with 4 KiB blocks, 512 random patterns
            assigned at random
  a_repair  shape a, one lost block per stripe (fec_repair_batch, 1 target)
Arms:
  shared    fec_decode_batch (fec_repair_batch with pattern_of = NULL) with ONE
            pattern -- pattern 0's blocks -- on the same buffers: the bytes moved
            are the same
  mixed     the unplanned call as shipped
  planned   fec_repair_batch_planned over a plan made once (its creation timed)
  knob0     the unplanned call under ZFEC_HIP_MIXED_FUSED=0: the parent's path
  parent    the parent commit's library making the unplanned call
The parent's library is another process (--parent-lib, default
abuild/parent/libzfec_hip.so: `git worktree add ../parent HEAD~1 && make -C
../parent`, the .so copied there); rounds alternate between a parent process
and a process of this tree, each running every shape once, so all arms are
measured on one box in one session.  Cold: every call streams its whole buffer
set, 2 GiB or more (shape a rotates over two sets), many times the 256 MiB
Infinity Cache.  Per arm and round: wall ms per call (calls back to back, then
a synchronise: what a caller waits for), GPU ms per call (events around the same
calls: kernel time where the host keeps ahead of the GPU, as in the shared and
planned arms; the unplanned call runs the planned call's kernel) and host ms
per call (until the asynchronous calls have returned).
Medians over the rounds and the range of single-round ratios.  The outputs of
this tree's arms are compared with the data after timing.
Writes profiles/mixed_wide_bench.json.

    python tools/mixed_wide_bench.py [--rounds 9] [--parent-lib PATH] [--out FILE] [--shapes a,b,a_repair]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "ZFEC_HIP_MIXED_FUSED"
ASYNC, ALL_PRIMARIES = 1, 4

SHAPES = {  # k, m, sz, nstripes, npatterns, buffer sets, targets (0: decode)
    "a": (20, 60, 52429, 1024, 1024, 2, 0),
    "b": (10, 16, 4096, 200000, 512, 1, 0),
    "a_repair": (20, 60, 52429, 1024, 1024, 2, 1),
}

_P, _SZ, _U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
_UP = ctypes.POINTER(ctypes.c_uint)
SIGS = {
    "fec_new": (_P, [ctypes.c_ushort, ctypes.c_ushort]),
    "fec_encode_batch": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _U]),
    "fec_decode_batch": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _SZ, _P, _U]),
    "fec_decode_batch_mixed": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _P, _SZ, _SZ, _P, _U]),
    "fec_repair_batch": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _UP, _SZ, _SZ, _P, _SZ, _SZ, _P, _U]),
    "fec_reload_config": (ctypes.c_int, []),
    "fec_last_kernel_name": (ctypes.c_char_p, []),
    "fec_last_error_message": (ctypes.c_char_p, []),
}
PLAN_SIGS = {
    "fec_repair_plan_new": (ctypes.c_int, [_P, _UP, _UP, _SZ, _SZ, ctypes.c_int, ctypes.POINTER(_P)]),
    "fec_repair_plan_free": (None, [_P]),
    "fec_repair_batch_planned": (ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _U]),
}


def load(path):
    """The library at `path` through ctypes alone (the parent's has no plan
    symbols), after the one-HIP-runtime preload of zfec_amd/_runtime.py."""
    spec = importlib.util.spec_from_file_location("_zfec_runtime", os.path.join(ROOT, "zfec_amd", "_runtime.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    rt.preload()
    L = ctypes.CDLL(path)
    sigs = dict(SIGS)
    if hasattr(L, "fec_repair_plan_new"):
        sigs.update(PLAN_SIGS)
    for name, (res, args) in sigs.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    L.fec_init()
    return L, "fec_repair_plan_new" in sigs


def uints(vals):
    return (ctypes.c_uint * max(1, len(vals)))(*[int(v) for v in vals])


def ok(L, st, what):
    if st:
        raise RuntimeError("%s: status %d: %s" % (what, st, L.fec_last_error_message().decode()))


def decode_order(nums, k):
    """The blocks of one pattern in an order fec_decode takes (primary i at
    slot i): the shared-pattern arm's matrix is as dense as a mixed one's."""
    slots, rest = [None] * k, [int(b) for b in nums if b >= k]
    for b in nums:
        if b < k:
            slots[int(b)] = int(b)
    return [b if b is not None else rest.pop() for b in slots]


def setup(L, torch, np, name):
    """Buffer sets of one shape: received blocks [sets, ns, k, sz], outputs
    [sets, ns, rows, sz], the ids on the device and the expected rows."""
    k, m, sz, ns, npat, nsets, nt = SHAPES[name]
    rng = np.random.default_rng(len(name) + k)
    code = L.fec_new(k, m)
    st = torch.cuda.current_stream().cuda_stream
    full = torch.empty((ns, m, sz), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(k)
    full[:, :k] = torch.randint(0, 256, (ns, k, sz), dtype=torch.uint8, device="cuda", generator=g)
    ok(L, L.fec_encode_batch(code, full.data_ptr(), sz, m * sz, full.data_ptr() + k * sz, sz, m * sz,
                             uints(range(k, m)), m - k, sz, ns, st, ASYNC), "fec_encode_batch")
    pats = np.stack([rng.permutation(m)[:k] for _ in range(npat)]).astype(np.int64)
    ids = rng.permutation(ns) % npat if npat >= ns else rng.integers(0, npat, size=ns)
    nums = torch.from_numpy(pats[ids]).cuda()
    recv = full[torch.arange(ns, device="cuda")[:, None], nums].contiguous()  # [ns, k, sz]
    if nt:
        tg = np.array([[rng.choice(np.setdiff1d(np.arange(m), p))] for p in pats], dtype=np.int64)
        want = full[torch.arange(ns, device="cuda")[:, None], torch.from_numpy(tg[ids]).cuda()].contiguous()
    else:
        tg = np.tile(np.arange(k, dtype=np.int64), (npat, 1))
        want = full[:, :k].contiguous()
    torch.cuda.synchronize()
    del full
    rows = tg.shape[1]
    src = torch.stack([recv] * nsets)
    dst = torch.zeros((nsets, ns, rows, sz), dtype=torch.uint8, device="cuda")
    del recv
    torch.cuda.empty_cache()
    return dict(code=code, k=k, m=m, sz=sz, ns=ns, npat=npat, nsets=nsets, rows=rows, src=src, dst=dst, want=want,
                pats=uints(pats.reshape(-1)), tgts=uints(tg.reshape(-1)),
                ids=torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda(),
                shared=uints(decode_order(pats[0], k)), repair=bool(nt))


def calls(L, s, has_plan):
    """arm -> (f(set index, stream), checked)."""
    k, sz, ns, rows = s["k"], s["sz"], s["ns"], s["rows"]
    code, ids = s["code"], s["ids"].data_ptr()

    def args(i):
        return (s["src"][i].data_ptr(), sz, k * sz, s["dst"][i].data_ptr(), sz, rows * sz)

    out = {}
    if s["repair"]:
        out["shared"] = (lambda i, st: L.fec_repair_batch(code, *args(i), s["pats"], s["tgts"], rows, 1, None, sz, ns,
                                                          st, ASYNC), False)
        mixed = lambda i, st: L.fec_repair_batch(code, *args(i), s["pats"], s["tgts"], rows, s["npat"], ids, sz, ns,
                                                 st, ASYNC)
    else:
        out["shared"] = (lambda i, st: L.fec_decode_batch(code, *args(i), s["shared"], sz, ns, st,
                                                          ASYNC | ALL_PRIMARIES), False)
        mixed = lambda i, st: L.fec_decode_batch_mixed(code, *args(i), s["pats"], s["npat"], ids, sz, ns, st, ASYNC)
    out["mixed"] = (mixed, True)
    if has_plan:
        t0 = time.perf_counter()
        plan = _P()
        ok(L, L.fec_repair_plan_new(code, s["pats"], s["tgts"], rows, s["npat"], -1, ctypes.byref(plan)),
           "fec_repair_plan_new")
        s["plan_new_ms"] = (time.perf_counter() - t0) * 1e3
        s["plan"] = plan
        out["planned"] = (lambda i, st: L.fec_repair_batch_planned(plan, *args(i), ids, sz, ns, st, ASYNC), True)
        out["knob0"] = (mixed, True)
    return out


def time_arm(L, torch, s, f, n):
    """(wall ms, GPU ms, host ms) per call of n calls back to back, after one
    untimed call; the kernel name."""
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    ok(L, f(0, st), "warm-up call")
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record(stream)
    for i in range(n):
        ok(L, f((i + 1) % s["nsets"], st), "timed call")
    b.record(stream)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return ((t2 - t0) * 1e3 / n, a.elapsed_time(b) / n, (t1 - t0) * 1e3 / n), L.fec_last_kernel_name().decode()


def worker(args):
    """One process, one library, one round: every shape, every arm once."""
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "mixed_wide_bench.py measures on a GPU"
    L, has_plan = load(args.lib)
    res = {}
    for name in args.shapes.split(","):
        s = setup(L, torch, np, name)
        arms = calls(L, s, has_plan)
        if not has_plan:
            arms = {"parent": arms["mixed"]}
        out = {}
        for arm, (f, checked) in arms.items():
            if arm == "knob0":
                os.environ[KNOB] = "0"
                L.fec_reload_config()
            # the run path of shape b is 2*10^5 launches a call: one timed call there
            slow = arm in ("knob0", "parent")
            n = 1 if slow and s["ns"] > 10000 else 3 if slow else 10
            (wall, gpu, host), kern = time_arm(L, torch, s, f, n)
            if arm == "knob0":
                os.environ.pop(KNOB, None)
                L.fec_reload_config()
            out[arm] = {"wall_ms": wall, "gpu_ms": gpu, "host_ms": host, "kernel": kern, "calls": n}
            if checked:  # after timing, outside the events
                for i in range(s["nsets"]):
                    assert torch.equal(s["dst"][i], s["want"]), (name, arm, "set", i, "wrong bytes")
            s["dst"].zero_()
        if has_plan:
            out["plan_new_ms"] = s["plan_new_ms"]
            L.fec_repair_plan_free(s["plan"])
        res[name] = out
        del s
        torch.cuda.empty_cache()
        print(name, "done", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "shapes": res}))


def run_worker(lib, shapes):
    env = dict(os.environ)
    env.pop(KNOB, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--shapes", shapes],
                       env=env, check=True, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def ratio(num, den):
    r = [a / b for a, b in zip(num, den)]
    return {"median": round(statistics.median(r), 4), "range": [round(min(r), 4), round(max(r), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--shapes", default="a,b,a_repair")
    ap.add_argument("--lib", default=os.path.join(ROOT, "zfec_amd", "libzfec_hip.so"))
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "abuild", "parent", "libzfec_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_wide_bench.json"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # (this process never opens the GPU: every measurement is a child process)
    have_parent = os.path.exists(args.parent_lib)
    rounds = {"own": [], "parent": []}
    device = None
    for r in range(args.rounds):  # alternating process rounds
        if have_parent:
            rounds["parent"].append(run_worker(args.parent_lib, args.shapes)["shapes"])
        res = run_worker(args.lib, args.shapes)
        device = res["device"]
        rounds["own"].append(res["shapes"])
        print("round", r + 1, "of", args.rounds, file=sys.stderr, flush=True)
    out = {"device": device, "rounds": args.rounds,
           "timing": "per round one process of each library; per arm one untimed call, then calls back to back: wall "
                     "ms per call up to the synchronise, GPU ms per call between events, host ms per call until the "
                     "calls returned; medians over the rounds, ratios per round (median and range)",
           "parent": "the parent commit's library, %s" % os.path.relpath(args.parent_lib, ROOT) if have_parent
                     else "not run: %s is missing (unmeasured)" % os.path.relpath(args.parent_lib, ROOT),
           "shapes": {}}
    for name in args.shapes.split(","):
        series = {}
        for who in ("own", "parent"):
            for rd in rounds[who]:
                for arm, v in rd[name].items():
                    if arm == "plan_new_ms":
                        series.setdefault(arm, []).append(v)
                    else:
                        d = series.setdefault(arm, {"wall_ms": [], "gpu_ms": [], "host_ms": [], "kernel": v["kernel"],
                                                    "calls_per_round": v["calls"]})
                        for key in ("wall_ms", "gpu_ms", "host_ms"):
                            d[key].append(v[key])
        leg = {"arms": {}, "ratios_wall": {}, "ratios_gpu": {}}
        for arm, d in series.items():
            if arm == "plan_new_ms":
                leg["fec_repair_plan_new_ms"] = {"median": round(statistics.median(d), 3),
                                                 "rounds": [round(x, 3) for x in d]}
                continue
            leg["arms"][arm] = {"kernel": d["kernel"], "calls_per_round": d["calls_per_round"]}
            for key in ("wall_ms", "gpu_ms", "host_ms"):
                leg["arms"][arm][key] = {"median": round(statistics.median(d[key]), 4),
                                         "rounds": [round(x, 4) for x in d[key]]}
        for a, b in (("mixed", "shared"), ("planned", "shared"), ("mixed", "parent"), ("planned", "parent"),
                     ("knob0", "parent"), ("mixed", "knob0"), ("planned", "knob0")):
            if a in series and b in series:
                leg["ratios_wall"]["%s/%s" % (a, b)] = ratio(series[a]["wall_ms"], series[b]["wall_ms"])
                leg["ratios_gpu"]["%s/%s" % (a, b)] = ratio(series[a]["gpu_ms"], series[b]["gpu_ms"])
        out["shapes"][name] = leg
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
