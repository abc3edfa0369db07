"""What the packed descriptors cost on top of the transaction batch calls.

Input: the bench's config-4 transaction mix (workload.txn_batch: 1..12
signers, 64..1232-B messages, legacy and v0, every signature valid), once as
one packed payload array and once as pointers into a registered arena.  The
same payloads go through

  staged_tag       fd_ed25519_amd_verify_txns_tag             txn_err + txn_tag
  staged_desc      fd_ed25519_amd_verify_txns_desc            + desc_off, desc
  registered_tag   fd_ed25519_amd_verify_txns_registered_tag
  registered_desc  fd_ed25519_amd_verify_txns_registered_desc

at 4096 transactions (one chunk) and 2^17 (several chunks of 2^16 signature
slots), timed as whole calls, the variants of a row alternating forwards and
backwards after a warm-up, into preallocated outputs.  Two clocks per call:
the wall clock and the calling thread's CPU time (CLOCK_THREAD_CPUTIME_ID).
Per variant: p50, min, p10, p90, max of the wall time ("spread" is p90 - p10),
the p50 of the thread time, and both per transaction; per row the descriptor
bytes per transaction.  The descriptors of the two _desc calls are compared
with each other, and every call's verdicts are checked.

With --parent-lib (a library built from the parent commit, for instance with
`python -m firedancer_amd.build --variant OUT.so ""` in a checkout of it) the
two _tag calls are also timed in fresh child processes, --runs times on the
parent's library and --runs times on this one, alternating: "vs_parent"
holds each run's p50 ("parent_runs_p50_us" / "current_runs_p50_us"), every
parent run's own p90 - p10 spread, "parent_run_to_run_us", the range of the
parent's p50 over its runs, and the difference of the two medians of p50s.
There is no pass/fail ratio: the numbers are reported as they fall.

usage: python tools/txns_desc_cost.py [--steps K] [--warmup W] [--big-n N] [--parent-lib SO] [--runs R] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, workload  # noqa: E402
from tag_cost import _stats  # noqa: E402

SIGS_PER_TXN = 6.5          # workload.txn_batch: 1..12 signers
BATCH_MAX, BLOB_MAX = 1 << 16, 1 << 24


def _aligned(nbytes):
    raw = np.zeros(nbytes + 4096, np.uint8)
    o = (-raw.ctypes.data) % 4096
    return raw[o:o + nbytes]


def _row(n_txn, seed, steps, warmup, tag_only):
    L, P = ed25519.lib(), ed25519._ptr
    payload, toff, tsz, tbase = workload.txn_batch(int(n_txn * SIGS_PER_TXN), seed)
    n, nsig = int(toff.size), int(tbase[-1])
    arena = _aligned((payload.size + 4095) & ~4095)
    arena[:payload.size] = payload
    ptr = np.uint64(arena.ctypes.data) + toff.astype(np.uint64)
    psz = tsz.astype(np.uint64)
    eng = ed25519.Engine(device=0, batch_max=BATCH_MAX, blob_max=BLOB_MAX)
    ed25519.host_register(arena)
    terr, ttag = np.zeros(n, np.int8), np.zeros(n, np.uint64)
    h = eng._h
    calls = {"staged_tag": lambda: L.fd_ed25519_amd_verify_txns_tag(h, n, P(payload), P(toff), P(tsz), int(payload.size),
                                                                    P(terr), None, None, P(ttag), None),
             "registered_tag": lambda: L.fd_ed25519_amd_verify_txns_registered_tag(h, n, P(ptr), P(psz), P(terr), None, None,
                                                                                   P(ttag), None)}
    desc_bytes = None
    try:
        if not tag_only:
            cap = int(sum(ed25519.txn_desc_bound(int(z)) * int(c) for z, c in zip(*np.unique(tsz, return_counts=True))))
            doff, desc = np.zeros(n + 1, np.uint64), np.zeros(max(cap, 1), np.uint8)
            calls["staged_desc"] = lambda: L.fd_ed25519_amd_verify_txns_desc(
                h, n, P(payload), P(toff), P(tsz), int(payload.size), P(terr), None, None, P(ttag), None, P(doff), P(desc), cap)
            calls["registered_desc"] = lambda: L.fd_ed25519_amd_verify_txns_registered_desc(
                h, n, P(ptr), P(psz), P(terr), None, None, P(ttag), None, P(doff), P(desc), cap)
            # the two _desc calls return the same descriptors, one for every transaction
            assert calls["staged_desc"]() == 0
            a_off, a_desc = doff.copy(), desc[:int(doff[-1])].copy()
            doff[:] = 0
            desc[:] = 0
            assert calls["registered_desc"]() == 0
            assert np.array_equal(doff, a_off) and np.array_equal(desc[:int(doff[-1])], a_desc), "descriptors differ"
            assert (np.diff(doff.astype(np.int64)) >= 20).all(), "a transaction without a descriptor"
            desc_bytes = int(doff[-1])
        wall, cpu = {name: [] for name in calls}, {name: [] for name in calls}
        order = list(calls)
        for step in range(warmup + steps):
            for name in (order if step % 2 == 0 else order[::-1]):
                terr[:] = 0x55
                c0, t0 = time.thread_time_ns(), time.perf_counter_ns()
                rc = calls[name]()
                dt, dc = (time.perf_counter_ns() - t0) * 1e-3, (time.thread_time_ns() - c0) * 1e-3
                assert rc == 0, (name, rc)
                bad = terr != 0
                assert int(bad.sum()) < 64 and (terr[bad] == -3).all(), "verdicts off: " + name
                if step >= warmup:
                    wall[name].append(dt)
                    cpu[name].append(dc)
    finally:
        ed25519.host_unregister(arena)
        eng.close()
    r = {"txns": n, "signatures": nsig, "payload_bytes": int(payload.size) - 8}
    if desc_bytes is not None:
        r["desc_bytes"] = desc_bytes
        r["desc_bytes_per_txn"] = round(desc_bytes / n, 1)
        r["desc_bound_bytes_per_txn"] = round(cap / n, 1)
    for name in calls:
        s = _stats(wall[name])
        s["thread_p50_us"] = round(float(np.median(cpu[name])), 1)
        s["wall_ns_per_txn"] = round(1e3 * s["p50_us"] / n, 1)
        s["thread_ns_per_txn"] = round(1e3 * s["thread_p50_us"] / n, 1)
        r[name] = s
    if not tag_only:
        for k in ("staged", "registered"):
            t, d = r[k + "_tag"], r[k + "_desc"]
            d["p50_minus_tag_us"] = round(d["p50_us"] - t["p50_us"], 1)
            d["thread_p50_minus_tag_us"] = round(d["thread_p50_us"] - t["thread_p50_us"], 1)
            d["p50_over_tag"] = round(d["p50_us"] / t["p50_us"], 4)
            d["beyond_tag_spread"] = bool(abs(d["p50_us"] - t["p50_us"]) > t["spread_us"])
    return r


def _rows(a, tag_only):
    return {"txns_%d" % n: _row(n, seed, a.steps, a.warmup, tag_only) for n, seed in ((a.small_n, 20271), (a.big_n, 20272))}


def _child(a, lib):
    env = dict(os.environ)
    env.pop("FD_AMD_LIB", None)
    if lib:
        env["FD_AMD_LIB"] = os.path.abspath(lib)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tag-only", "--steps", str(a.steps), "--warmup",
                            str(a.warmup), "--small-n", str(a.small_n), "--big-n", str(a.big_n)],
                           capture_output=True, text=True, timeout=400, env=env)
    if child.returncode:
        sys.exit("txns_desc_cost: a --tag-only child failed:\n" + child.stderr[-2000:])
    return json.loads(child.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--small-n", type=int, default=4096)
    ap.add_argument("--big-n", type=int, default=1 << 17)
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit")
    ap.add_argument("--runs", type=int, default=3, help="child runs per library")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag-only", action="store_true", help="the child's mode: the two _tag calls; rows only")
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("txns_desc_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    if a.steps < 30:
        sys.exit("txns_desc_cost: medians of at least 30 calls")
    if a.tag_only:
        print(json.dumps(_rows(a, True)))
        return
    res = {"steps": a.steps, "warmup": a.warmup, "device": hip.device_name(0), "version": ed25519.version(),
           "batch_max": BATCH_MAX, "blob_max": BLOB_MAX}
    res.update(_rows(a, False))
    if a.parent_lib:
        runs = {"parent": [], "current": []}
        for _ in range(a.runs):
            runs["parent"].append(_child(a, a.parent_lib))
            runs["current"].append(_child(a, None))
        cmp_ = {}
        for row in ("txns_%d" % a.small_n, "txns_%d" % a.big_n):
            cmp_[row] = {}
            for call in ("staged_tag", "registered_tag"):
                p = [r[row][call]["p50_us"] for r in runs["parent"]]
                c = [r[row][call]["p50_us"] for r in runs["current"]]
                cmp_[row][call] = {"parent_runs_p50_us": p, "current_runs_p50_us": c,
                                   "parent_in_run_spread_us": [r[row][call]["spread_us"] for r in runs["parent"]],
                                   "parent_run_to_run_us": round(max(p) - min(p), 1),
                                   "current_minus_parent_median_us": round(float(np.median(c) - np.median(p)), 1),
                                   "slower_than_every_parent_run": bool(float(np.median(c)) > max(p))}
        res["vs_parent"] = cmp_
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
