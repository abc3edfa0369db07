"""What asking for the dedup tags costs, on the two host paths.

Row "4096": one 4096-signature batch of 200-B messages in registered memory
through verify_soa_registered -- the latency path: the GPU reads the planes in
place, and with tags one more kernel (k_tag_out) writes them to mapped host
memory after the DSM kernel.  Row "2^20": one 2^20-signature batch through
verify_soa -- the throughput path, 16 chunks of 2^16 through the pinned
staging: with tags each chunk adds one k_tag_out launch (8 B per signature
into mapped host memory) and the host's copy of its tags to the caller.

Each row times the whole call on the host clock (the calls return after their
last chunk is drained), with and without tags, the two alternating A B B A
after a warm-up of both, into preallocated outputs.  Per variant: p50, min,
p10, p90, max; "spread" is p90 - p10.  The yardstick of a row is its own
untagged variant in the same run.  Every call's verdicts are checked (all
signatures are valid: 0, or the reference's rare -3 false reject) and every
tagged call's tags against hashlib on a sample.

usage: python tools/tag_cost.py [--steps K] [--warmup W] [--big-n N] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, workload  # noqa: E402


def _stats(us):
    a = np.sort(np.asarray(us, np.float64))
    q = lambda f: float(a[min(a.size - 1, int(f * a.size))])
    return {"p50_us": round(float(np.median(a)), 1), "min_us": round(float(a[0]), 1), "p10_us": round(q(0.10), 1),
            "p90_us": round(q(0.90), 1), "max_us": round(float(a[-1]), 1), "spread_us": round(q(0.90) - q(0.10), 1),
            "calls": int(a.size)}


def _row(call, n, planes, steps, warmup):
    """call(tag pointer or None) -> rc, writing err / tag below."""
    pub, sig, off, sz, blob = planes
    err = np.zeros(n, np.int8)
    tag = np.zeros(n, np.uint64)
    sample = np.random.default_rng(5).choice(n, min(n, 64), replace=False)
    want = {int(i): int.from_bytes(hashlib.sha512(bytes(sig[i, :32]) + bytes(pub[i]) +
                                                  bytes(blob[int(off[i]):int(off[i]) + int(sz[i])])).digest()[:8], "little")
            for i in sample}
    t = {"untagged": [], "tagged": []}
    order = ("untagged", "tagged")
    for step in range(warmup + steps):
        for name in (order if step % 2 == 0 else order[::-1]):
            err[:] = 0x55
            tag[:] = 0
            t0 = time.perf_counter_ns()
            rc = call(err, tag if name == "tagged" else None)
            dt = (time.perf_counter_ns() - t0) * 1e-3
            assert rc == 0, rc
            bad = err != 0
            assert int(bad.sum()) < 64 and (err[bad] == -3).all(), "verdicts off"
            if name == "tagged":
                assert all(int(tag[i]) == w for i, w in want.items()), "tags off"
            if step >= warmup:
                t[name].append(dt)
    r = {name: _stats(v) for name, v in t.items()}
    r["n"] = n
    r["tag_cost_p50_us"] = round(r["tagged"]["p50_us"] - r["untagged"]["p50_us"], 1)
    r["beyond_untagged_spread"] = bool(r["tag_cost_p50_us"] > r["untagged"]["spread_us"])
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
        sys.exit("tag_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    if a.steps < 30:
        sys.exit("tag_cost: medians of at least 30 calls")
    L, P = ed25519.lib(), ed25519._ptr
    res = {"msg_sz": a.msg_sz, "steps": a.steps, "warmup": a.warmup, "device": hip.device_name(0),
           "version": ed25519.version()}

    # the latency path: registered planes, read in place
    n = a.small_n
    planes = workload.sig_batch(n, a.msg_sz, 20262)
    eng = ed25519.Engine(device=0, batch_max=n, blob_max=n * ed25519.MSG_MAX)
    r = ed25519.RegisteredPlanes(*planes)
    try:
        def small(err, tag):
            if tag is None:
                return L.fd_ed25519_amd_verify_soa_registered(eng._h, n, P(r[0]), P(r[1]), P(r[2]), P(r[3]), P(r[4]),
                                                              int(r[4].size), P(err))
            return L.fd_ed25519_amd_verify_soa_registered_tag(eng._h, n, P(r[0]), P(r[1]), P(r[2]), P(r[3]), P(r[4]),
                                                              int(r[4].size), P(err), P(tag))
        res["registered_%d" % n] = _row(small, n, planes, a.steps, a.warmup)
    finally:
        r.close()
        eng.close()

    # the throughput path: pinned staging, chunks of 2^16
    n = a.big_n
    planes = workload.sig_batch(n, a.msg_sz, 20263)
    pub, sig, off, sz, blob = planes
    eng = ed25519.Engine(device=0, batch_max=1 << 16, blob_max=(1 << 16) * 256)
    try:
        def big(err, tag):
            if tag is None:
                return L.fd_ed25519_amd_verify_soa(eng._h, n, P(pub), P(sig), P(off), P(sz), P(blob), int(blob.size), P(err))
            return L.fd_ed25519_amd_verify_soa_tag(eng._h, n, P(pub), P(sig), P(off), P(sz), P(blob), int(blob.size),
                                                   P(err), P(tag))
        res["soa_%d" % n] = _row(big, n, planes, a.steps, a.warmup)
    finally:
        eng.close()

    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
