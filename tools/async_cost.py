"""What one host thread gets from submitting batches asynchronously, and what a
poll that finds nothing costs.

Input: frags pub | sig | msg (200-B messages, all signatures valid) at 64-B
aligned offsets of one arena registered with host_register, and the pointer and
size arrays a tile with its own run loop builds from them.  The path is the
registered pointer batch (k_gather) throughout.

Rows, for 1024 and 4096 signatures per batch, `steps` batches each after a
warm-up, from one thread:

  sync      fd_ed25519_amd_verify_batch_registered in a loop: a batch's latency
            is its call
  async_d   d = 1, 2, 4 submissions kept in flight on an engine with 4 slots:
            submit while fewer than d are in flight, then one async_poll; a
            batch's latency runs from before its submit call to the return of
            the poll that delivers it

Per row: signatures/s over the whole loop and the latency's p50 / p99 (us).

Poll cost: the median time of an fd_ed25519_amd_async_poll that returns
ASYNC_NONE, with the completion word (default) and with
FD_ED25519_AMD_ASYNC_POLL=event (hipEventQuery), over 10^5 such polls made while
2^16-signature submissions run (a submission lasts about a millisecond, so the
polls span many submissions; a block of polls in which one delivered is thrown
away).  Polls are timed in blocks of 64 through ctypes; "call_ns" is the same
loop around fd_ed25519_amd_async_in_flight, the cost of getting into the
library and back, and "net_ns" the difference.  The A/B repeats `--ab-rounds`
times alternately; the spread of the medians is what the difference is held
against.

On a build without the submit calls only the sync rows are written.

usage: python tools/async_cost.py [--steps K] [--warmup W] [--polls N] [--ab-rounds R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, workload  # noqa: E402

MSG_SZ = 200
NONE = 1
now = time.perf_counter_ns


def _aligned(nbytes):
    raw = np.zeros(nbytes + 4096, np.uint8)
    o = (-raw.ctypes.data) % 4096
    return raw[o:o + nbytes]


def _pct(a, q):
    a = np.sort(np.asarray(a, np.float64))
    return float(a[min(a.size - 1, int(q * a.size))])


class Frags:
    def __init__(self, n, seed):
        pub, sig, off, sz, blob = workload.sig_batch(n, MSG_SZ, seed)
        stride = (96 + MSG_SZ + 63) & ~63
        self.arena = _aligned((n * stride + 4095) & ~4095)
        fr = self.arena[:n * stride].reshape(n, stride)
        fr[:, :32], fr[:, 32:96], fr[:, 96:96 + MSG_SZ] = pub, sig, blob[:n * MSG_SZ].reshape(n, MSG_SZ)
        base = np.uint64(self.arena.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(stride)
        self.pp, self.sp, self.mp, self.zz = base, base + np.uint64(32), base + np.uint64(96), sz.astype(np.uint64)
        ed25519.host_register(self.arena)

    def args(self, n):
        P = ed25519._ptr
        return P(self.mp[:n]), P(self.zz[:n]), P(self.sp[:n]), P(self.pp[:n])

    def close(self):
        ed25519.host_unregister(self.arena)


def _engine(batch_max, slots, poll=None):
    if poll:
        os.environ["FD_ED25519_AMD_ASYNC_POLL"] = poll       # read when the engine is created
    try:
        if not hasattr(ed25519.lib(), "fd_ed25519_amd_new_slots"):    # a build without the submit calls
            return ed25519.Engine(device=0, batch_max=batch_max, blob_max=batch_max * 256)
        return ed25519.Engine(device=0, batch_max=batch_max, blob_max=batch_max * 256, nslot=slots)
    finally:
        os.environ.pop("FD_ED25519_AMD_ASYNC_POLL", None)


def _check(err):
    assert ((err == 0) | (err == -3)).all() and (err == -3).mean() < 1e-3, "wrong verdicts"


def _row(kind, n, lat_ns, total_ns, steps):
    return {"kind": kind, "n": n, "steps": steps, "sig_per_s": n * steps / (total_ns * 1e-9),
            "lat_us_p50": _pct(lat_ns, 0.5) / 1e3, "lat_us_p99": _pct(lat_ns, 0.99) / 1e3,
            "lat_us_min": float(min(lat_ns)) / 1e3}


def sync_row(eng, fr, n, steps, warmup):
    L, P = ed25519.lib(), ed25519._ptr
    f, a, err = L.fd_ed25519_amd_verify_batch_registered, fr.args(n), np.full(n, 0x55, np.int8)
    pe, lat = P(err), []
    for k in range(warmup + steps):
        if k == warmup:
            t_begin = now()
        t0 = now()
        rc = f(eng._h, n, *a, pe)
        t1 = now()
        assert rc == 0
        if k >= warmup:
            lat.append(t1 - t0)
    total = now() - t_begin
    _check(err)
    return _row("sync", n, lat, total, steps)


def async_row(eng, fr, n, depth, steps, warmup):
    L, P = ed25519.lib(), ed25519._ptr
    submit, poll = L.fd_ed25519_amd_submit_batch_registered, L.fd_ed25519_amd_async_poll
    a = fr.args(n)
    errs = [np.full(n, 0x55, np.int8) for _ in range(depth)]
    pes = [P(e) for e in errs]
    t, tk = ctypes.c_ulong(0), ctypes.c_ulong(0)
    pt, ptk = ctypes.byref(t), ctypes.byref(tk)
    total_n = warmup + steps
    t_sub, lat = {}, []
    sub = done = 0
    t_begin = now()
    while done < total_n:
        while sub < total_n and sub - done < depth:
            t0 = now()
            rc = submit(eng._h, n, *a, pes[sub % depth], None, pt)
            assert rc == 0, rc
            t_sub[t.value] = t0
            sub += 1
        rc = poll(eng._h, ptk)
        if rc == NONE:
            continue
        t1 = now()
        assert rc == 0, rc
        done += 1
        t0 = t_sub.pop(tk.value)
        if done == warmup:
            t_begin = t1
        elif done > warmup:
            lat.append(t1 - t0)
    total = now() - t_begin
    for e in errs:
        _check(e)
    return _row("async_%d" % depth, n, lat, total, steps)


def poll_cost(eng, fr, n, polls, block=64):
    """Median ns of a poll that returns ASYNC_NONE, of the bare library call, and the blocks kept."""
    L, P = ed25519.lib(), ed25519._ptr
    submit, poll, wait, idle = (L.fd_ed25519_amd_submit_batch_registered, L.fd_ed25519_amd_async_poll,
                                L.fd_ed25519_amd_async_wait, L.fd_ed25519_amd_async_in_flight)
    a, err = fr.args(n), np.full(n, 0x55, np.int8)
    pe = P(err)
    t, tk = ctypes.c_ulong(0), ctypes.c_ulong(0)
    pt, ptk = ctypes.byref(t), ctypes.byref(tk)
    h, rng = eng._h, range(block)
    per, subs = [], 0
    deadline = time.monotonic() + 120.0
    while len(per) * block < polls:
        assert time.monotonic() < deadline, "poll_cost: too few polls found nothing"
        assert submit(h, n, *a, pe, None, pt) == 0
        subs += 1
        delivered = False
        while not delivered:
            t0 = now()
            for _ in rng:
                if poll(h, ptk) != NONE:
                    delivered = True
            t1 = now()
            if not delivered:
                per.append((t1 - t0) / block)
    _check(err)
    assert wait(h, ptk) == NONE
    base = []
    for _ in range(len(per)):
        t0 = now()
        for _ in rng:
            if idle(h) != 0:
                delivered = False
        t1 = now()
        base.append((t1 - t0) / block)
    p, b = _pct(per, 0.5), _pct(base, 0.5)
    return {"poll_none_ns_p50": p, "poll_none_ns_p10": _pct(per, 0.1), "poll_none_ns_p90": _pct(per, 0.9),
            "call_ns_p50": b, "net_ns": p - b, "polls": len(per) * block, "submissions": subs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--polls", type=int, default=100000)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "async_cost.json"))
    a = ap.parse_args()
    have_async = hasattr(ed25519.lib(), "fd_ed25519_amd_submit_batch_registered")
    big = 1 << 16
    fr = Frags(big if have_async else 4096, 20271)
    out = {"version": ed25519.version(), "msg_sz": MSG_SZ, "async": have_async, "rows": [], "poll": []}
    eng = _engine(4096, 4)
    try:
        for n in (1024, 4096):
            out["rows"].append(sync_row(eng, fr, n, a.steps, a.warmup))
            print(json.dumps(out["rows"][-1]), flush=True)
            if have_async:
                for d in (1, 2, 4):
                    out["rows"].append(async_row(eng, fr, n, d, a.steps, a.warmup))
                    print(json.dumps(out["rows"][-1]), flush=True)
    finally:
        eng.close()
    if have_async:
        engs = {"word": _engine(big, 2), "event": _engine(big, 2, "event")}
        try:
            for r in range(a.ab_rounds):
                for kind in (("word", "event") if r % 2 == 0 else ("event", "word")):
                    c = dict(poll_cost(engs[kind], fr, big, a.polls), kind=kind, round=r)
                    out["poll"].append(c)
                    print(json.dumps(c), flush=True)
        finally:
            for e in engs.values():
                e.close()
    fr.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
