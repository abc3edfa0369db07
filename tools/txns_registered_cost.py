"""What the transaction batch costs staged by the host and gathered by the GPU.

Input: the bench's config-4 transaction mix (workload.txn_batch: 1..12
signers, 64..1232-B messages, legacy and v0, every signature valid), the
payloads packed back to back in one arena registered with host_register, and
the pointer and size arrays a tile builds from its frags.  The same payloads
go through

  A   fd_ed25519_amd_verify_txns             one memcpy of the payload per
                                             transaction into the pinned
                                             staging, on the caller; four
                                             H2D copies per chunk; two chunks
                                             in flight
  B   fd_ed25519_amd_verify_txns_registered  one 32-B record per transaction;
                                             k_gather_txn fetches the bytes;
                                             no H2D copy

and B again on engines whose k_gather_txn wave cap is 32 and 128 instead of 64
(FD_ED25519_AMD_GATHER_TXN_WAVES, read when an engine is created).  Rows:
4096 transactions (one chunk) and 2^17 (several chunks of 2^16 signature
slots).

Each variant is timed as whole calls (a call returns after its last chunk is
drained), the variants of a row alternating A B .. .. B A after a warm-up,
into preallocated outputs.  Two clocks per call: the host's wall clock, and
the calling thread's CPU time (CLOCK_THREAD_CPUTIME_ID), which is what the
call costs the thread that makes it -- the staging copies, the records, the
launches, and whatever part of waiting for the GPU the runtime spends spinning
rather than asleep.  By default the runtime spins, so the thread time of a
call equals its wall time; the rows are therefore measured a second time in a
child process that asks the runtime to sleep while it waits
(hipSetDeviceFlags( hipDeviceScheduleBlockingSync ) before anything else:
"blocking_sync" in the output), where the thread time is the host work
alone.  Per variant: p50, min, p10, p90, max of the wall time ("spread" is
p90 - p10), the p50 of the thread time, and both per transaction.  There is
no pass/fail ratio: the numbers are reported as they fall.  Every call's
verdicts are checked (all signatures are valid: 0, or the
reference's rare -3 false reject), and B's per-transaction tags against A's.

usage: python tools/txns_registered_cost.py [--steps K] [--warmup W] [--big-n N] [--out FILE]
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

WAVES = (32, 64, 128)
SIGS_PER_TXN = 6.5          # workload.txn_batch: 1..12 signers


def _aligned(nbytes):
    raw = np.zeros(nbytes + 4096, np.uint8)
    o = (-raw.ctypes.data) % 4096
    return raw[o:o + nbytes]


def _engine(waves, batch_max, blob_max):
    os.environ["FD_ED25519_AMD_GATHER_TXN_WAVES"] = str(waves)    # read when the engine is created
    try:
        return ed25519.Engine(device=0, batch_max=batch_max, blob_max=blob_max)
    finally:
        del os.environ["FD_ED25519_AMD_GATHER_TXN_WAVES"]


def _row(n_txn, seed, steps, warmup):
    L, P = ed25519.lib(), ed25519._ptr
    payload, toff, tsz, tbase = workload.txn_batch(int(n_txn * SIGS_PER_TXN), seed)
    n, nsig = int(toff.size), int(tbase[-1])
    arena = _aligned((payload.size + 4095) & ~4095)
    arena[:payload.size] = payload
    ptr = np.uint64(arena.ctypes.data) + toff.astype(np.uint64)
    psz = tsz.astype(np.uint64)
    batch_max, blob_max = 1 << 16, 1 << 24
    eng = {w: _engine(w, batch_max, blob_max) for w in WAVES}
    ed25519.host_register(arena)
    terr, ttag_a, ttag_b = np.zeros(n, np.int8), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    calls = {"A_verify_txns": lambda: L.fd_ed25519_amd_verify_txns(eng[64]._h, n, P(payload), P(toff), P(tsz),
                                                                   int(payload.size), P(terr), None, None)}
    for w in WAVES:
        calls["B_registered_waves_%d" % w] = (lambda h: lambda: L.fd_ed25519_amd_verify_txns_registered(
            h, n, P(ptr), P(psz), P(terr), None, None))(eng[w]._h)
    try:
        # B's per-transaction tags once, against A's
        assert L.fd_ed25519_amd_verify_txns_tag(eng[64]._h, n, P(payload), P(toff), P(tsz), int(payload.size), P(terr),
                                                None, None, P(ttag_a), None) == 0
        assert L.fd_ed25519_amd_verify_txns_registered_tag(eng[64]._h, n, P(ptr), P(psz), P(terr), None, None, P(ttag_b),
                                                           None) == 0
        assert np.array_equal(ttag_a, ttag_b) and (ttag_a != 0).all(), "tags off"
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
        for e in eng.values():
            e.close()
    r = {"txns": n, "signatures": nsig, "payload_bytes": int(payload.size) - 8}
    for name in calls:
        s = _stats(wall[name])
        s["thread_p50_us"] = round(float(np.median(cpu[name])), 1)
        s["wall_ns_per_txn"] = round(1e3 * s["p50_us"] / n, 1)
        s["thread_ns_per_txn"] = round(1e3 * s["thread_p50_us"] / n, 1)
        s["M_sig_per_s"] = round(nsig / s["p50_us"], 2)
        r[name] = s
    a = r["A_verify_txns"]
    for w in WAVES:
        b = r["B_registered_waves_%d" % w]
        b["p50_minus_A_us"] = round(b["p50_us"] - a["p50_us"], 1)
        b["thread_p50_minus_A_us"] = round(b["thread_p50_us"] - a["thread_p50_us"], 1)
        b["beyond_A_spread"] = bool(abs(b["p50_us"] - a["p50_us"]) > a["spread_us"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--small-n", type=int, default=4096)
    ap.add_argument("--big-n", type=int, default=1 << 17)
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocking-sync", action="store_true", help="the child's mode: waits sleep; rows only")
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("txns_registered_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    if a.steps < 30:
        sys.exit("txns_registered_cost: medians of at least 30 calls")
    if a.blocking_sync:
        hip.check(hip.hip().hipSetDeviceFlags(4), "hipSetDeviceFlags( hipDeviceScheduleBlockingSync )")
        print(json.dumps({"txns_%d" % n: _row(n, seed, a.steps, a.warmup)
                          for n, seed in ((a.small_n, 20266), (a.big_n, 20267))}))
        return
    res = {"steps": a.steps, "warmup": a.warmup, "device": hip.device_name(0), "version": ed25519.version(),
           "default_waves": 64}
    res["txns_%d" % a.small_n] = _row(a.small_n, 20266, a.steps, a.warmup)
    res["txns_%d" % a.big_n] = _row(a.big_n, 20267, a.steps, a.warmup)
    # the same rows with sleeping waits, in a fresh process (the flag is set before the runtime does anything else)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--blocking-sync", "--steps", str(a.steps),
                            "--warmup", str(a.warmup), "--small-n", str(a.small_n), "--big-n", str(a.big_n)],
                           capture_output=True, text=True, timeout=300)
    if child.returncode:
        sys.exit("txns_registered_cost: the blocking-sync child failed:\n" + child.stderr[-2000:])
    res["blocking_sync"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
