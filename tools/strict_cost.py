"""What strict mode costs: k_strict's time on the flagship batch.

2^20 GPU-signed 200-B signatures resident in HBM, verified through
verify_dev_ev in reference and in strict mode, the two alternating (A B B A,
the same host work after every step) after a warm-up of both.  Per mode: the median of the whole step
(ev[0] -> ev[3]) and of the DSM stage (ev[2] -> ev[3]); k_strict's own time is
the difference of the two DSM-stage medians (it is enqueued after the DSM
kernels and before ev[3]).  Every step's verdicts are checked: all 0 in
strict mode (every signature is valid), 0 or the reference's -3 false rejects
in reference mode.

usage: python tools/strict_cost.py [--n N] [--steps K] [--warmup W] [--kernel default|k_dsm|k_dsmp|...] [--out FILE]
Run under `rocprofv3 --kernel-trace --stats` (small --steps) for the
per-kernel times of k_strict and k_fin themselves.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--msg-sz", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", default="default")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("strict_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    n = a.n
    pub, sig, off, sz, blob = workload.sig_batch(n, a.msg_sz, 20261)
    d = [hip.DeviceBuffer.from_array(x) for x in (pub, sig, off, sz, blob)]
    d_err = hip.DeviceBuffer(n)
    d_ws = hip.DeviceBuffer(ed25519.workspace_footprint(n))
    st = hip.Stream()
    ev = [hip.Event() for _ in range(4)]
    ed25519.select_dsm_kernel(a.kernel)
    modes = (("reference", ed25519.MODE_REFERENCE), ("strict", ed25519.MODE_STRICT))
    total = {m: [] for m, _ in modes}
    dsm = {m: [] for m, _ in modes}
    rejects = {}
    for step in range(a.warmup + a.steps):
        # A B B A ...: each mode runs as often after the other as after itself, and the host does the
        # same work between any two steps (an idle gap before a step lowers the clocks it starts at)
        for name, mode in (modes if step % 2 == 0 else modes[::-1]):
            ed25519.verify_dev_ev(n, *[b.ptr for b in d], d_err.ptr, d_ws.ptr, st.handle, ev, mode=mode)
            st.synchronize()
            err = d_err.to_array(np.int8, n)
            bad = int((err != 0).sum())
            only3 = bool((err[err != 0] == -3).all())
            if mode == ed25519.MODE_STRICT:
                assert bad == 0, "strict mode rejected %d valid signatures" % bad
            else:
                assert only3 and bad < 64, "reference verdicts off: %d rejects" % bad
            rejects[name] = bad
            if step >= a.warmup:
                total[name].append(ev[0].elapsed_ms(ev[3]))
                dsm[name].append(ev[2].elapsed_ms(ev[3]))
    ed25519.select_dsm_kernel("default")
    med = statistics.median
    res = {"n": n, "msg_sz": a.msg_sz, "steps": a.steps, "warmup": a.warmup, "kernel": a.kernel,
           "device": hip.device_name(0), "version": ed25519.version()}
    for name, _ in modes:
        res[name] = {"step_ms_median": round(med(total[name]), 4), "step_ms_min": round(min(total[name]), 4),
                     "step_ms_max": round(max(total[name]), 4), "dsm_stage_ms_median": round(med(dsm[name]), 4),
                     "sigs_per_s": round(n / med(total[name]) * 1e3), "rejected": rejects[name]}
    k = med(dsm["strict"]) - med(dsm["reference"])
    res["k_strict_ms"] = round(k, 4)
    res["k_strict_share_of_reference_step"] = round(k / med(total["reference"]), 5)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
