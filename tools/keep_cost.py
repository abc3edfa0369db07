"""What the survivor filter of the _keep submissions costs, against doing the
same filter on the host.

Workload, from one thread with 4 submissions in flight on an engine with 4
slots (tools/async_cost.py's loop: submit while fewer than 4 are in flight,
then one async_poll):

  sig_4096, sig_1024   registered 200-B frags (async_cost's arena), 4096 and
                       1024 per batch, through the registered pointer batch
  txn_4096             the bench's config-4 transaction mix (workload.txn_batch:
                       1..12 signers, 64..1232-B messages), 4096 per batch, as
                       pointers into a registered arena

Every signature is valid; every eighth item of a batch points at the item
before it, so one item in eight is an in-batch duplicate.

Variants, run in rounds that alternate their order:

  plain   the submit call alone: verdicts only, nothing filtered (what
          tools/async_cost.py's async_4 rows measure)
  host    the submit call with tags, and on delivery the filter in numpy on
          the calling thread: passing items, first of each tag, ascending
  keep    the _keep form of the submit call: verdicts and the publish list

Two figures per variant and round: signatures/s over the loop, and the calling
thread's CPU time per item (CLOCK_THREAD_CPUTIME_ID around the submit calls,
the polls that deliver and the host filter; the polls that find nothing are a
spin and are left out).  The first delivery of `keep` and of `host` in a round
are compared with each other.

"parent_async_4" quotes, where profiles/async_cost.json holds them, the parent
commit's async_4 rows for the same frags and whether `plain` falls inside their
recorded run-to-run range: the baseline for "costs nothing when not asked for".
Nothing here passes or fails on a ratio: the numbers are reported as they fall.

usage: python tools/keep_cost.py [--steps K] [--warmup W] [--rounds R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, workload  # noqa: E402
from async_cost import Frags, _aligned  # noqa: E402

NONE, DEPTH, SLOTS = 1, 4, 4
now, cpu = time.perf_counter_ns, time.thread_time_ns
HERE = os.path.dirname(os.path.abspath(__file__))


def _dup(a):
    """Every eighth entry repeats the one before it."""
    a = a.copy()
    a[7::8] = a[6::8][:a[7::8].size]
    return a


def host_filter(err, tag):
    """The rule in numpy: passing items, the first of each nonzero tag, ascending."""
    idx = np.nonzero(err == 0)[0]
    t = tag[idx]
    _, first = np.unique(t, return_index=True)
    keep = np.zeros(idx.size, bool)
    keep[first] = True
    keep |= t == 0
    return idx[keep].astype(np.uint32)


class SigLoad:
    def __init__(self, fr, n):
        P = ed25519._ptr
        self.n, self.items = n, n
        self._a = [_dup(x[:n]) for x in (fr.mp, fr.zz, fr.sp, fr.pp)]
        self.args = tuple(P(x) for x in self._a)
        self.err = [np.zeros(n, np.int8) for _ in range(DEPTH)]
        self.tag = [np.zeros(n, np.uint64) for _ in range(DEPTH)]
        self.keep = [np.zeros(n, np.uint32) for _ in range(DEPTH)]
        self.cnt = [np.zeros(1, np.uint64) for _ in range(DEPTH)]
        L = ed25519.lib()
        self.f_plain, self.f_keep = L.fd_ed25519_amd_submit_batch_registered, L.fd_ed25519_amd_submit_batch_registered_keep

    def submit(self, h, kind, k, pt):
        P = ed25519._ptr
        if kind == "keep":
            return self.f_keep(h, self.n, *self.args, P(self.err[k]), None, P(self.keep[k]), P(self.cnt[k]), pt)
        return self.f_plain(h, self.n, *self.args, P(self.err[k]), P(self.tag[k]) if kind == "host" else None, pt)


class TxnLoad:
    def __init__(self, n_txn, seed):
        P = ed25519._ptr
        payload, toff, tsz, tbase = workload.txn_batch(int(n_txn * 6.5), seed)
        self.n, self.items = int(toff.size), int(tbase[-1])
        self.arena = _aligned((payload.size + 4095) & ~4095)
        self.arena[:payload.size] = payload
        ed25519.host_register(self.arena)
        self._ptr = _dup(np.uint64(self.arena.ctypes.data) + toff.astype(np.uint64))
        self._sz = _dup(tsz.astype(np.uint64))
        base, tot = ed25519.txn_slots_ptrs(self._ptr, self._sz)
        self.items = int(tot)                              # signatures per batch, duplicates included
        self.args = (P(self._ptr), P(self._sz))
        n = self.n
        self.err = [np.zeros(n, np.int8) for _ in range(DEPTH)]
        self.tag = [np.zeros(n, np.uint64) for _ in range(DEPTH)]
        self.keep = [np.zeros(n, np.uint32) for _ in range(DEPTH)]
        self.cnt = [np.zeros(1, np.uint64) for _ in range(DEPTH)]
        L = ed25519.lib()
        self.f_plain, self.f_keep = L.fd_ed25519_amd_submit_txns_registered, L.fd_ed25519_amd_submit_txns_registered_keep

    def submit(self, h, kind, k, pt):
        P = ed25519._ptr
        head = (h, self.n, *self.args, P(self.err[k]), None, None, P(self.tag[k]) if kind == "host" else None, None, None, None, 0)
        if kind == "keep":
            return self.f_keep(*head, P(self.keep[k]), P(self.cnt[k]), pt)
        return self.f_plain(*head, pt)

    def close(self):
        ed25519.host_unregister(self.arena)


def loop(eng, ld, kind, steps, warmup):
    """One variant: (signatures/s, thread ns per signature, the first delivery's publish list or None)."""
    poll = ed25519.lib().fd_ed25519_amd_async_poll
    t, tk = ctypes.c_ulong(0), ctypes.c_ulong(0)
    pt, ptk = ctypes.byref(t), ctypes.byref(tk)
    h, total_n = eng._h, warmup + steps
    sub = done = 0
    busy = 0
    first = None
    t_begin = now()
    while done < total_n:
        c0 = cpu()
        while sub < total_n and sub - done < DEPTH:
            rc = ld.submit(h, kind, sub % DEPTH, pt)
            assert rc == 0, (kind, rc)
            sub += 1
        c1 = cpu()
        rc = poll(h, ptk)
        if rc == NONE:
            busy += c1 - c0
            continue
        assert rc == 0, (kind, rc)
        k = done % DEPTH
        if kind == "host":
            out = host_filter(ld.err[k], ld.tag[k])
        elif kind == "keep":
            out = ld.keep[k][:int(ld.cnt[k][0])]
        else:
            out = None
        busy += cpu() - c0
        if first is None and out is not None:
            first = out.copy()
        done += 1
        if done == warmup:
            t_begin, busy = now(), 0
    total = now() - t_begin
    for e in ld.err:
        assert ((e == 0) | (e == -3)).all() and (e == -3).mean() < 1e-3, "wrong verdicts"
    return ld.items * steps / (total * 1e-9), busy / (ld.items * steps), first


def row(eng, ld, steps, warmup, rounds):
    kinds = ("plain", "host", "keep")
    r = {"items_per_batch": ld.n, "signatures_per_batch": ld.items, "steps": steps,
         "sig_per_s": {k: [] for k in kinds}, "thread_ns_per_sig": {k: [] for k in kinds}}
    for rd in range(rounds):
        firsts = {}
        for kind in (kinds if rd % 2 == 0 else kinds[::-1]):
            s, c, firsts[kind] = loop(eng, ld, kind, steps, warmup)
            r["sig_per_s"][kind].append(round(s))
            r["thread_ns_per_sig"][kind].append(round(c, 2))
        assert np.array_equal(firsts["keep"], firsts["host"]), "the GPU's publish list differs from the host filter's"
        r["survivors_per_batch"] = int(firsts["keep"].size)
    med = lambda v: float(np.median(v))  # noqa: E731
    r["keep_over_host_sig_per_s"] = round(med(r["sig_per_s"]["keep"]) / med(r["sig_per_s"]["host"]), 4)
    r["keep_over_plain_sig_per_s"] = round(med(r["sig_per_s"]["keep"]) / med(r["sig_per_s"]["plain"]), 4)
    r["thread_ns_per_sig_keep_minus_host"] = round(med(r["thread_ns_per_sig"]["keep"]) - med(r["thread_ns_per_sig"]["host"]), 2)
    return r


def parent_rows(res):
    """The parent commit's async_4 rows, when profiles/async_cost.json has them."""
    try:
        summ = json.load(open(os.path.join(HERE, "..", "profiles", "async_cost.json")))["summary"]
    except (OSError, KeyError, ValueError):
        return None
    out = {}
    for n in (1024, 4096):
        p = summ.get("async_4_%d" % n, {}).get("sig_per_s")
        if p:
            mine = res["sig_%d" % n]["sig_per_s"]["plain"]
            out["async_4_%d" % n] = {"parent_sig_per_s": p, "plain_sig_per_s": mine,
                                     "plain_median_within_parent_range": bool(min(p) <= float(np.median(mine)) <= max(p))}
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "keep_cost.json"))
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("keep_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    res = {"tool": "tools/keep_cost.py --steps %d --warmup %d --rounds %d" % (a.steps, a.warmup, a.rounds),
           "device": hip.device_name(0), "version": ed25519.version(), "depth": DEPTH, "duplicates": "every eighth item"}
    fr = Frags(4096, 20271)
    eng = ed25519.Engine(device=0, batch_max=4096, blob_max=4096 * 256, nslot=SLOTS)
    try:
        for n in (4096, 1024):
            res["sig_%d" % n] = row(eng, SigLoad(fr, n), a.steps, a.warmup, a.rounds)
            print(json.dumps({"sig_%d" % n: res["sig_%d" % n]}), flush=True)
    finally:
        eng.close()
        fr.close()
    tx = TxnLoad(4096, 20272)
    eng = ed25519.Engine(device=0, batch_max=1 << 16, blob_max=1 << 24, nslot=SLOTS)
    try:
        res["txn_4096"] = row(eng, tx, max(a.steps // 4, 1), max(a.warmup // 4, 1), a.rounds)
        print(json.dumps({"txn_4096": res["txn_4096"]}), flush=True)
    finally:
        eng.close()
        tx.close()
    res["parent_async_4"] = parent_rows(res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
