"""What the pointer-array batch costs staged by the host and gathered by the GPU.

Input: n frags pub | sig | msg (200-B messages) at 64-B aligned offsets of one
arena registered with host_register, and the three pointer arrays and the size
array a tango tile builds from them (pub = p, sig = p + 32, msg = p + 96).
The same arrays go through

  A   fd_ed25519_amd_verify_batch             three memcpys per signature into
                                              the pinned staging, on the caller
  B   fd_ed25519_amd_verify_batch_registered  one 32-B record per signature;
                                              k_gather fetches the bytes

and, for the choice DESIGN.md s2 records, B with the chunk's records copied to
the device first (FD_ED25519_AMD_GATHER_COPY=1) instead of read in place.
Row "soa_registered": the same data pre-split into registered SoA planes
through fd_ed25519_amd_verify_soa_registered -- what a caller who already has
planes gets.  Rows: n = 4096 (one chunk, the latency kernels) and n = 2^20
(16 chunks of 2^16).

Each variant is timed as whole calls on the host clock (a call returns after
its last chunk is drained), the variants of a row alternating A B .. .. B A
after a warm-up, into preallocated outputs.  Per variant: p50, min, p10, p90,
max; "spread" is p90 - p10.  The yardstick of a row is its own A in the same
run: at 2^20, B's p50 must not exceed A's by more than A's spread.  Every
call's verdicts are checked (all signatures are valid: 0, or the reference's
rare -3 false reject), and B's tags against hashlib on a sample.

usage: python tools/batch_registered_cost.py [--steps K] [--warmup W] [--big-n N] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, workload  # noqa: E402
from tag_cost import _stats  # noqa: E402


def _aligned(nbytes):
    raw = np.zeros(nbytes + 4096, np.uint8)
    o = (-raw.ctypes.data) % 4096
    return raw[o:o + nbytes]


def _row(n, msg_sz, seed, batch_max, steps, warmup):
    L, P = ed25519.lib(), ed25519._ptr
    pub, sig, off, sz, blob = workload.sig_batch(n, msg_sz, seed)
    stride = (96 + msg_sz + 63) & ~63
    arena = _aligned((n * stride + 4095) & ~4095)
    fr = arena[:n * stride].reshape(n, stride)
    fr[:, :32], fr[:, 32:96], fr[:, 96:96 + msg_sz] = pub, sig, blob[:n * msg_sz].reshape(n, msg_sz)
    base = np.uint64(arena.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(stride)
    pp, sp, mp, zz = base, base + np.uint64(32), base + np.uint64(96), sz.astype(np.uint64)
    vpp = lambda a: ctypes.cast(P(a), ed25519.c_void_pp)
    sample = np.random.default_rng(5).choice(n, min(n, 64), replace=False)
    want = {int(i): int.from_bytes(hashlib.sha512(bytes(sig[i, :32]) + bytes(pub[i]) +
                                                  bytes(blob[int(off[i]):int(off[i]) + msg_sz])).digest()[:8], "little")
            for i in sample}

    def engine(copy):
        os.environ["FD_ED25519_AMD_GATHER_COPY"] = "1" if copy else "0"    # read when the engine is created
        try:
            return ed25519.Engine(device=0, batch_max=batch_max, blob_max=batch_max * 256)
        finally:
            del os.environ["FD_ED25519_AMD_GATHER_COPY"]

    eng, eng_copy = engine(False), engine(True)
    planes = ed25519.RegisteredPlanes(pub, sig, off, sz, blob)
    ed25519.host_register(arena)
    err, tag = np.zeros(n, np.int8), np.zeros(n, np.uint64)
    calls = {
        "A_verify_batch": lambda: L.fd_ed25519_amd_verify_batch(eng._h, n, vpp(mp), ctypes.cast(P(zz), ed25519.c_ulong_p),
                                                               vpp(sp), vpp(pp), P(err)),
        "B_registered": lambda: L.fd_ed25519_amd_verify_batch_registered_tag(eng._h, n, P(mp), P(zz), P(sp), P(pp), P(err), None),
        "B_registered_records_copied": lambda: L.fd_ed25519_amd_verify_batch_registered_tag(eng_copy._h, n, P(mp), P(zz), P(sp),
                                                                                          P(pp), P(err), None),
        "soa_registered": lambda: L.fd_ed25519_amd_verify_soa_registered(eng._h, n, P(planes[0]), P(planes[1]), P(planes[2]),
                                                                         P(planes[3]), P(planes[4]), int(planes[4].size),
                                                                         P(err)),
    }
    try:
        # B's tags once, against hashlib
        assert L.fd_ed25519_amd_verify_batch_registered_tag(eng._h, n, P(mp), P(zz), P(sp), P(pp), P(err), P(tag)) == 0
        assert all(int(tag[i]) == w for i, w in want.items()), "tags off"
        t = {name: [] for name in calls}
        order = list(calls)
        for step in range(warmup + steps):
            for name in (order if step % 2 == 0 else order[::-1]):
                err[:] = 0x55
                t0 = time.perf_counter_ns()
                rc = calls[name]()
                dt = (time.perf_counter_ns() - t0) * 1e-3
                assert rc == 0, (name, rc)
                bad = err != 0
                assert int(bad.sum()) < 64 and (err[bad] == -3).all(), "verdicts off: " + name
                if step >= warmup:
                    t[name].append(dt)
    finally:
        ed25519.host_unregister(arena)
        planes.close()
        eng.close()
        eng_copy.close()
    r = {name: _stats(v) for name, v in t.items()}
    for name in r:
        r[name]["M_per_s"] = round(n / r[name]["p50_us"], 2)
    a = r["A_verify_batch"]
    r["n"] = n
    for name in ("B_registered", "B_registered_records_copied"):
        r[name]["p50_minus_A_us"] = round(r[name]["p50_us"] - a["p50_us"], 1)
        r[name]["beyond_A_spread"] = bool(r[name]["p50_us"] - a["p50_us"] > a["spread_us"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--small-n", type=int, default=4096)
    ap.add_argument("--big-n", type=int, default=1 << 20)
    ap.add_argument("--msg-sz", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("batch_registered_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    if a.steps < 30:
        sys.exit("batch_registered_cost: medians of at least 30 calls")
    res = {"msg_sz": a.msg_sz, "steps": a.steps, "warmup": a.warmup, "device": hip.device_name(0),
           "version": ed25519.version()}
    res["frags_%d" % a.small_n] = _row(a.small_n, a.msg_sz, 20264, a.small_n, a.steps, a.warmup)
    res["frags_%d" % a.big_n] = _row(a.big_n, a.msg_sz, 20265, 1 << 16, a.steps, a.warmup)
    big = res["frags_%d" % a.big_n]
    res["big_row_meets_condition"] = not big["B_registered"]["beyond_A_spread"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
