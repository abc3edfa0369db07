"""What strict verdicts cost in the streaming verify tile.

One pool of fresh GPU-signed 200-B signatures (all valid) through
fd_verify_amd_bench_stream, the tile in reference mode (k_tile_persist) and
in strict mode (k_tile_persist_strict) alternating A B B A in this process,
so each mode runs as often after the other as after itself.  Medians of:

  saturated   rate 0 (credit flow control), per forced chunk mode -- latency
              (8 lanes per signature; the overlay runs on 8 lanes of a wave
              that carries 8 signatures), quad, throughput -- and AUTO;
  paced       p50 / p99 at 1 M frags/s and at half the reference mode's
              saturated AUTO rate.

There is no pass threshold: the tool reports.  Latency percentiles come
from the bench's trace (no verdict check in these runs: check mode does not
measure latency); tests/test_tile_strict_gpu.py checks the verdicts.

usage: python tools/tile_strict_cost.py [--batch-max B] [--pool N] [--sat-frags F] [--paced-seconds S]
                                        [--rounds R] [--copy] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, tango, workload  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("latency", tango.CHUNK_LATENCY), ("quad", tango.CHUNK_QUAD), ("throughput", tango.CHUNK_THROUGHPUT),
         ("auto", tango.CHUNK_AUTO))


def abba(rounds, run):
    """run(strict) -> dict, in the order A B B A per round; {False: [...], True: [...]}."""
    out = {False: [], True: []}
    for _ in range(rounds):
        for strict in (False, True, True, False):
            out[strict].append(run(strict))
    return out


def med(rs, key):
    return statistics.median(r[key] for r in rs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch-max", type=int, default=4096)
    ap.add_argument("--pool", type=int, default=1 << 16)
    ap.add_argument("--msg-sz", type=int, default=200)
    ap.add_argument("--sat-frags", type=int, default=1 << 24)
    ap.add_argument("--paced-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=1, help="A B B A rounds per figure (2 runs per mode each)")
    ap.add_argument("--copy", action="store_true", help="copy staging instead of zero copy")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_strict_cost.json"))
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("tile_strict_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    pub, sig, off, sz, blob = workload.sig_batch(a.pool, a.msg_sz, 20262)
    pool = (pub, sig, off, sz, blob)
    zc = not a.copy

    def stream(strict, chunk_mode, nf, rate=0.0):
        r = tango.bench_stream(a.device, a.batch_max, 0, *pool, nf, rate=rate, zero_copy=zc, chunk_mode=chunk_mode,
                               strict=strict)
        # an all-valid pool: strict mode filters nothing, reference mode only its limb-compare false rejects
        assert r["published"] + r["sv_filt"] == nf and r["ovrn"] == 0, r
        # (about 1.6e-6 of the pool's entries, each repeated nf / pool times)
        assert r["sv_filt"] == 0 if strict else r["sv_filt"] <= 4 * (nf // a.pool + 1), (strict, r["sv_filt"])
        return r

    res = {"batch_max": a.batch_max, "pool": a.pool, "msg_sz": a.msg_sz, "staging": "zero_copy" if zc else "copy",
           "order": "A B B A (A reference, B strict), %d round(s) per figure" % a.rounds, "sat_frags": a.sat_frags,
           "paced_seconds": a.paced_seconds, "device": hip.device_name(a.device), "version": ed25519.version(),
           "saturated": {}, "paced": {}}
    stream(False, tango.CHUNK_AUTO, 1 << 20)     # warm-up of both kernels: code objects loaded, clocks up
    stream(True, tango.CHUNK_AUTO, 1 << 20)
    for name, cm in MODES:
        rs = abba(a.rounds, lambda strict: stream(strict, cm, a.sat_frags))
        ref, st = med(rs[False], "frags_per_s"), med(rs[True], "frags_per_s")
        res["saturated"][name] = {
            "reference_frags_per_s": round(ref), "strict_frags_per_s": round(st),
            "reference_runs": [round(r["frags_per_s"]) for r in rs[False]],
            "strict_runs": [round(r["frags_per_s"]) for r in rs[True]],
            "strict_cost": round(1.0 - st / ref, 5),
            "reference_sv_filt": int(max(r["sv_filt"] for r in rs[False]))}
        print(name, json.dumps(res["saturated"][name]), flush=True)
    half = 0.5 * res["saturated"]["auto"]["reference_frags_per_s"]
    for name, rate in (("1M_frags_per_s", 1e6), ("half_saturated", half)):
        nf = int(max(50000, rate * a.paced_seconds))
        rs = abba(max(a.rounds, 2), lambda strict: stream(strict, tango.CHUNK_AUTO, nf, rate))
        e = {"offered_frags_per_s": round(rate), "frags": nf}
        for strict, key in ((False, "reference"), (True, "strict")):
            e[key] = {"p50_us": round(med(rs[strict], "p50_ns") / 1e3, 1), "p99_us": round(med(rs[strict], "p99_ns") / 1e3, 1),
                      "service_p50_us": round(med(rs[strict], "service_p50_ns") / 1e3, 1),
                      "p50_us_runs": [round(r["p50_ns"] / 1e3, 1) for r in rs[strict]],
                      "frags_lat_quad_thr": [int(med(rs[strict], k)) for k in ("gpu_frags_lat", "gpu_frags_quad",
                                                                               "gpu_frags_thr")]}
        e["strict_p50_minus_reference_us"] = round(e["strict"]["p50_us"] - e["reference"]["p50_us"], 1)
        e["strict_service_p50_minus_reference_us"] = round(e["strict"]["service_p50_us"] - e["reference"]["service_p50_us"], 1)
        res["paced"][name] = e
        print(name, json.dumps(e), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
