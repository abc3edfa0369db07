"""What dedup across submissions costs on the GPU (a window attached to the
engine, include/fd_ed25519_amd.h "The dedup window"), against the same rule
run on the calling thread behind a windowless _keep submission.

The loop is tools/keep_cost.py's: one thread, 4 submissions in flight on an
engine with 4 slots (submit while fewer than 4 are in flight, then one
async_poll).  The workloads are its three --

  sig_4096, sig_1024   registered 200-B frags, 4096 and 1024 per batch, through
                       the registered pointer batch
  txn_4096             the bench's config-4 transaction mix, 4096 per batch, as
                       pointers into a registered arena

-- but every batch is a different one: the batches walk through a POOL of
distinct signed items, round and round.  Every signature is valid.  Of every
eight items of a batch, the eighth repeats the seventh (an in-batch duplicate,
as in keep_cost) and the fourth repeats the third item of the same group of
the PREVIOUS batch (a duplicate only a window sees).  The pool is sized so
that an item comes round again after more distinct tags than the deepest
window holds: by then it has expired and is admitted again, so every variant
is in the same steady state -- three quarters of a batch inserted by the
window variants.  (--pool-sigs / --pool-txns shrink the pools; the output
says when a pool comes round inside a window.)

Variants, run in rounds that alternate their order, each from an empty window:

  keep          the _keep form, no window attached: in-batch dedup only
  host_D        the _keep form with tags, and on delivery
                fd_ed25519_amd_window_keep over the survivors, on a host-only
                window of depth D, on the calling thread
  window_D      the _keep form on an engine with a device window of depth D
                                                           D = 2^16 and 2^20

Two figures per variant and round, as in keep_cost: signatures/s over the loop,
and the calling thread's CPU time per signature (CLOCK_THREAD_CPUTIME_ID around
the submit calls, the polls that deliver and the host window; the polls that
find nothing are a spin and are left out).  host_D and window_D must publish
the same lists: the survivors of every delivery are counted, and the lists of
the warm-up deliveries compared, between the two.

"baseline" answers "does keep without a window cost what it cost before":
keep_cost's own `keep` rows (one batch, repeated) measured by this run, next
to those of --baseline FILE, a keep_cost.json the parent commit's build wrote
on the same machine in the same session (without the option:
profiles/keep_cost.json as recorded, and the output says so).  Nothing here
passes or fails on a ratio: the numbers are reported as they fall.

usage: python tools/keep_window_cost.py [--steps K] [--warmup W] [--rounds R] [--baseline FILE] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip, workload  # noqa: E402
from async_cost import MSG_SZ, Frags, _aligned  # noqa: E402
import keep_cost  # noqa: E402

NONE, DEPTH, SLOTS = 1, 4, 4
DEPTHS = (1 << 16, 1 << 20)
now, cpu = time.perf_counter_ns, time.thread_time_ns
HERE = os.path.dirname(os.path.abspath(__file__))
P = ed25519._ptr


def _mix(planes, n):
    """The batches of n over pool-ordered planes (one array per submit
    argument): in every group of eight the eighth item repeats the seventh, and
    the fourth repeats the third of the same group of the batch before (the
    last batch, for the first)."""
    nb = planes[0].size // n
    out = []
    for a in planes:
        a = a[:nb * n].reshape(nb, n).copy()
        a[:, 7::8] = a[:, 6::8]
        a[:, 3::8] = np.roll(a, 1, axis=0)[:, 2::8]
        out.append(a)
    return nb, out


class Pool:
    """The batches of one workload and a ring of DEPTH output sets."""

    def __init__(self, n, nb, items):
        self.n, self.nb, self.items = n, nb, items             # items[b]: the signatures of batch b
        self.err = [np.zeros(n, np.int8) for _ in range(DEPTH)]
        self.tag = [np.zeros(n, np.uint64) for _ in range(DEPTH)]
        self.keep = [np.zeros(n, np.uint32) for _ in range(DEPTH)]
        self.cnt = [np.zeros(1, np.uint64) for _ in range(DEPTH)]
        self.distinct = nb * n * 6 // 8                        # distinct tags before the pool comes round


class SigPool(Pool):
    def __init__(self, fr, n):
        nb, self._a = _mix((fr.mp, fr.zz, fr.sp, fr.pp), n)
        Pool.__init__(self, n, nb, np.full(nb, n, np.int64))
        self.args = [tuple(P(x[b]) for x in self._a) for b in range(nb)]
        self.f = ed25519.lib().fd_ed25519_amd_submit_batch_registered_keep

    def submit(self, h, b, k, tags, pt):
        return self.f(h, self.n, *self.args[b], P(self.err[k]), P(self.tag[k]) if tags else None, P(self.keep[k]), P(self.cnt[k]), pt)


class TxnPool(Pool):
    """pool_txns transactions of the config-4 mix, synthesised 2^17 at a time into one registered arena."""

    def __init__(self, n, pool_txns, seed):
        parts, total = [], 0
        while sum(p[1].size for p in parts) < pool_txns:
            want = min(1 << 17, pool_txns - sum(p[1].size for p in parts))
            payload, toff, tsz, _ = workload.txn_batch(int(want * 6.5) + 13, seed + len(parts))
            parts.append((payload, toff[:want], tsz[:want]))
            total += (payload.size + 63) & ~63
        self.arena = _aligned((total + 4095) & ~4095)
        ptr, sz, at = [], [], 0
        for payload, toff, tsz in parts:
            self.arena[at:at + payload.size] = payload
            ptr.append(np.uint64(self.arena.ctypes.data + at) + toff.astype(np.uint64))
            sz.append(tsz.astype(np.uint64))
            at += (payload.size + 63) & ~63
        ed25519.host_register(self.arena)
        nb, self._a = _mix((np.concatenate(ptr), np.concatenate(sz)), n)
        items = np.array([ed25519.txn_slots_ptrs(self._a[0][b], self._a[1][b])[1] for b in range(nb)], np.int64)
        Pool.__init__(self, n, nb, items)
        self.args = [tuple(P(x[b]) for x in self._a) for b in range(nb)]
        self.f = ed25519.lib().fd_ed25519_amd_submit_txns_registered_keep

    def submit(self, h, b, k, tags, pt):
        return self.f(h, self.n, *self.args[b], P(self.err[k]), None, None, P(self.tag[k]) if tags else None, None, None, None, 0,
                      P(self.keep[k]), P(self.cnt[k]), pt)

    def close(self):
        ed25519.host_unregister(self.arena)


def loop(eng, ld, kind, depth, steps, warmup):
    """One variant from an empty window: (signatures/s, thread ns per
    signature, survivors delivered, a digest of the warm-up deliveries' lists)."""
    L = ed25519.lib()
    poll, host_keep = L.fd_ed25519_amd_async_poll, L.fd_ed25519_amd_window_keep
    t, tk = ctypes.c_ulong(0), ctypes.c_ulong(0)
    pt, ptk = ctypes.byref(t), ctypes.byref(tk)
    h, total_n = eng._h, warmup + steps
    win = ed25519.Window(0 if kind == "window" else -1, depth) if kind != "keep" else None
    if kind == "window":
        eng.set_window(win)
    zero, sub_out = np.zeros(ld.n, np.int8), np.zeros(ld.n, np.uint32)
    sub = done = busy = sigs = survivors = digest = 0
    t_begin = now()
    try:
        while done < total_n:
            c0 = cpu()
            while sub < total_n and sub - done < DEPTH:
                rc = ld.submit(h, sub % ld.nb, sub % DEPTH, kind == "host", pt)
                assert rc == 0, (kind, rc)
                sub += 1
            c1 = cpu()
            rc = poll(h, ptk)
            if rc == NONE:
                busy += c1 - c0
                continue
            assert rc == 0, (kind, rc)
            k = done % DEPTH
            out = ld.keep[k][:int(ld.cnt[k][0])]
            if kind == "host":                                 # the window's rule over the survivors, on this thread
                tg = ld.tag[k][out]
                c = host_keep(win._h, tg.size, P(zero), P(tg), P(sub_out))
                assert c <= tg.size
                out = out[sub_out[:c]]
            busy += cpu() - c0
            survivors += out.size
            if done < warmup:
                digest = zlib.crc32(out.tobytes(), digest)
            done += 1
            if done == warmup:
                t_begin, busy = now(), 0
            elif done > warmup:
                sigs += int(ld.items[(done - 1) % ld.nb])
        total = now() - t_begin
    finally:
        if kind == "window":
            eng.set_window(None)
        if win:
            win.close()
    for e in ld.err:
        assert ((e == 0) | (e == -3)).all() and (e == -3).mean() < 1e-3, "wrong verdicts"
    return sigs / (total * 1e-9), busy / sigs, survivors, digest


def row(eng, ld, steps, warmup, rounds):
    kinds = [("keep", 0)] + [(k, d) for d in DEPTHS for k in ("host", "window")]
    name = lambda k, d: k if not d else "%s_%d" % (k, d)  # noqa: E731
    r = {"items_per_batch": ld.n, "batches_in_pool": ld.nb, "distinct_tags_per_pool_round": ld.distinct,
         "pool_comes_round_inside_window": {str(d): bool(ld.distinct <= d) for d in DEPTHS},
         "signatures_per_batch_mean": round(float(ld.items.mean()), 1), "steps": steps,
         "sig_per_s": {name(*k): [] for k in kinds}, "thread_ns_per_sig": {name(*k): [] for k in kinds}, "survivors": {}}
    for rd in range(rounds):
        seen = {}
        for k, d in (kinds if rd % 2 == 0 else kinds[::-1]):
            s, c, surv, dig = loop(eng, ld, k, d, steps, warmup)
            r["sig_per_s"][name(k, d)].append(round(s))
            r["thread_ns_per_sig"][name(k, d)].append(round(c, 2))
            seen[(k, d)] = (surv, dig)
            r["survivors"][name(k, d)] = surv
        for d in DEPTHS:
            assert seen[("host", d)] == seen[("window", d)], ("the device window's lists differ from the host window's", d, seen)
    med = lambda v: float(np.median(v))  # noqa: E731
    for d in DEPTHS:
        w, hst = "window_%d" % d, "host_%d" % d
        r["%s_over_%s_sig_per_s" % (w, hst)] = round(med(r["sig_per_s"][w]) / med(r["sig_per_s"][hst]), 4)
        r["%s_over_keep_sig_per_s" % w] = round(med(r["sig_per_s"][w]) / med(r["sig_per_s"]["keep"]), 4)
        r["thread_ns_per_sig_%s_minus_%s" % (w, hst)] = round(med(r["thread_ns_per_sig"][w]) - med(r["thread_ns_per_sig"][hst]), 2)
    return r


def baseline_row(eng, ld, steps, warmup, rounds, parent):
    """keep_cost's `keep` variant (one batch, repeated) on this build, next to the parent's rows for the same workload."""
    mine = [keep_cost.loop(eng, ld, "keep", steps, warmup)[:2] for _ in range(rounds)]
    r = {"keep_sig_per_s": [round(m[0]) for m in mine], "keep_thread_ns_per_sig": [round(m[1], 2) for m in mine]}
    if parent:
        p = parent["sig_per_s"]["keep"]
        r.update(parent_keep_sig_per_s=p, parent_keep_thread_ns_per_sig=parent["thread_ns_per_sig"]["keep"],
                 keep_median_within_parent_range=bool(min(p) <= float(np.median(r["keep_sig_per_s"])) <= max(p)),
                 keep_median_over_parent_median=round(float(np.median(r["keep_sig_per_s"])) / float(np.median(p)), 4))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool-sigs", type=int, default=3 << 19, help="frags in the signature pool (default: 1.5 x 2^20)")
    ap.add_argument("--pool-txns", type=int, default=3 << 19, help="transactions in the transaction pool")
    ap.add_argument("--baseline", default=None, help="a keep_cost.json written by the parent commit's build in this session")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "keep_window_cost.json"))
    a = ap.parse_args()
    if hip.device_count() < 1:
        sys.exit("keep_window_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    same_session = a.baseline is not None
    try:
        parent = json.load(open(a.baseline or os.path.join(HERE, "..", "profiles", "keep_cost.json")))
    except (OSError, ValueError):
        parent = {}
    res = {"tool": "tools/keep_window_cost.py --steps %d --warmup %d --rounds %d --pool-sigs %d --pool-txns %d"
                   % (a.steps, a.warmup, a.rounds, a.pool_sigs, a.pool_txns),
           "device": hip.device_name(0), "version": ed25519.version(), "in_flight": DEPTH, "msg_sz": MSG_SZ,
           "duplicates": "of every eight items one repeats its neighbour and one an item of the previous batch",
           "baseline": {"parent_rows": "measured in this session by the parent commit's build" if same_session
                        else "as recorded in profiles/keep_cost.json (another session)", "parent_tool": parent.get("tool")}}
    fr = Frags(a.pool_sigs, 20271)
    eng = ed25519.Engine(device=0, batch_max=4096, blob_max=4096 * 256, nslot=SLOTS)
    try:
        for n in (4096, 1024):
            key = "sig_%d" % n
            res["baseline"][key] = baseline_row(eng, keep_cost.SigLoad(fr, n), a.steps, a.warmup, a.rounds, parent.get(key))
            res[key] = row(eng, SigPool(fr, n), a.steps, a.warmup, a.rounds)
            print(json.dumps({key: res[key], "baseline": res["baseline"][key]}), flush=True)
    finally:
        eng.close()
        fr.close()
    steps, warmup = max(a.steps // 4, 1), max(a.warmup // 4, 1)
    tx, tp = keep_cost.TxnLoad(4096, 20272), TxnPool(4096, a.pool_txns, 20273)     # as keep_cost: the arenas before the engine
    eng = ed25519.Engine(device=0, batch_max=1 << 16, blob_max=1 << 24, nslot=SLOTS)
    try:
        res["baseline"]["txn_4096"] = baseline_row(eng, tx, steps, warmup, a.rounds, parent.get("txn_4096"))
        res["txn_4096"] = row(eng, tp, steps, warmup, a.rounds)
        print(json.dumps({"txn_4096": res["txn_4096"], "baseline": res["baseline"]["txn_4096"]}), flush=True)
    finally:
        eng.close()
        tx.close()
        tp.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
