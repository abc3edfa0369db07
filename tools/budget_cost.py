"""What having the GPU return each transaction's compute budget and fee costs,
against the calling thread running the same rule over returned descriptors
(include/fd_txn_amd.h, "Compute budget").

Workload: the bench's config-4 transaction mix from registered memory (every
signature valid; its transactions hold one instruction each, none addressed
to the compute budget program), one thread.

  submit   4096 transactions per submission, 4 in flight on an engine with 4
           slots (tools/keep_cost.py's loop)
  block    the blocking call over 4096 and over 2^17 transactions

Arms, run in rounds that alternate their order:

  plain    the call without budget: verdicts only
           (fd_ed25519_amd_submit_txns_registered /
           fd_ed25519_amd_verify_txns_registered)
  budget   the _budget call: verdicts and the records from the GPU
  host     the call with desc / desc_off, then fd_txn_amd_budget on the
           calling thread for every transaction, in a C loop over the
           returned descriptors (the loop of INTEGRATION.md s3, compiled here
           with gcc against include/ and the library)

Two figures per arm and round: transactions/s, and the calling thread's CPU
time per transaction (CLOCK_THREAD_CPUTIME_ID around the calls, the polls
that deliver and the host loop; polls that find nothing are a spin and are
left out).  The first delivery of `budget` and of `host` in a round must hold
the same records.

--parent-lib FILE: the parent commit's library, built in the same session.
Before it touches the GPU itself the tool runs the `plain` arm alone in child
processes of their own, by turns on the parent's library (FD_AMD_LIB) and on
this build's, --parent-procs times each, and reports whether the median of
this build's runs lies inside the range of the parent's: the feature must add
nothing to a call that does not ask for it.  Nothing here passes or fails on
a ratio: the numbers are reported as they fall.

usage: python tools/budget_cost.py [--steps K] [--warmup W] [--rounds R] [--parent-lib FILE] [--parent-procs N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip  # noqa: E402
from keep_cost import TxnLoad  # noqa: E402

NONE, DEPTH, SLOTS = 1, 4, 4
now, cpu = time.perf_counter_ns, time.thread_time_ns
HERE = os.path.dirname(os.path.abspath(__file__))
P = ed25519._ptr

HOST_LOOP = r'''
#include "fd_txn_amd.h"
/* the rule on the calling thread, from what a _desc call returned */
void
budget_host_loop( ulong txn_cnt, void const * const * txn, ulong const * txn_sz, ulong const * desc_off, uchar const * desc,
                  fd_txn_amd_budget_t * budget ) {
  for( ulong t=0UL; t<txn_cnt; t++ )
    fd_txn_amd_budget( (uchar const *)txn[t], txn_sz[t],
                       desc_off[t+1]>desc_off[t] ? (fd_txn_t const *)( desc + desc_off[t] ) : NULL, budget + t );
}
'''


def host_loop(tmp):
    src, so = os.path.join(tmp, "budget_host_loop.c"), os.path.join(tmp, "libbudget_host_loop.so")
    open(src, "w").write(HOST_LOOP)
    libdir = os.path.dirname(os.path.abspath(ed25519.LIB_PATH))
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(HERE, "..", "include"),
                           src, "-L", libdir, "-lfd_ed25519_amd", "-Wl,-rpath," + libdir, "-o", so])
    f = ctypes.CDLL(so).budget_host_loop
    f.argtypes, f.restype = [ctypes.c_ulong] + [ctypes.c_void_p] * 5, None
    return f


class Load(TxnLoad):
    """keep_cost's transaction load (n transactions, every eighth repeating
    the one before), `rep` times over, with the outputs of the three arms."""

    def __init__(self, n_txn, seed, rep=1, budget=True):
        super().__init__(n_txn, seed)
        if rep > 1:
            self._ptr, self._sz = np.tile(self._ptr, rep), np.tile(self._sz, rep)
            self.args, self.n = (P(self._ptr), P(self._sz)), int(self._ptr.size)
            self.err = [np.zeros(self.n, np.int8) for _ in range(DEPTH)]
        if budget:
            L = ed25519.lib()
            self.f_sub_budget, self.f_blk_budget = L.fd_ed25519_amd_submit_txns_registered_budget, L.fd_ed25519_amd_verify_txns_registered_budget
            sets = DEPTH if rep == 1 else 1             # the blocking call uses one set of outputs
            self.doff, self.desc = zip(*(ed25519._desc_buffers(self._sz) for _ in range(sets)))
            self.budget = [np.zeros(self.n, ed25519.BUDGET_DTYPE) for _ in range(sets)]
        self.f_blk_desc = ed25519.lib().fd_ed25519_amd_verify_txns_registered_desc

    def outs(self, kind, k):
        """(txn_err .. desc_cap) of the call for arm `kind` on output set k."""
        desc = (P(self.doff[k]), P(self.desc[k]), int(self.desc[k].size)) if kind == "host" else (None, None, 0)
        return (P(self.err[k]), None, None, None, None, *desc)

    def submit(self, h, kind, k, pt):
        head = (h, self.n, *self.args, *self.outs(kind, k))
        if kind == "budget":
            return self.f_sub_budget(*head, None, None, None, 0, None, None, P(self.budget[k]), pt)
        return self.f_plain(*head, pt)

    def block(self, h, kind, k):
        head = (h, self.n, *self.args, *self.outs(kind, k))
        if kind == "budget":
            return self.f_blk_budget(*head, P(self.budget[k]))
        return self.f_blk_desc(*head)

    def host(self, loop_fn, k):
        loop_fn(self.n, *self.args, P(self.doff[k]), P(self.desc[k]), P(self.budget[k]))


def check(ld):
    for e in ld.err:
        assert ((e == 0) | (e == -3)).all() and (e == -3).mean() < 1e-3, "wrong verdicts"


def loop_submit(eng, ld, kind, steps, warmup, loop_fn):
    """One arm of the submissions: (transactions/s, thread ns per transaction, the first delivery's records or None)."""
    poll = ed25519.lib().fd_ed25519_amd_async_poll
    t, tk = ctypes.c_ulong(0), ctypes.c_ulong(0)
    pt, ptk = ctypes.byref(t), ctypes.byref(tk)
    h, total_n = eng._h, warmup + steps
    sub = done = busy = 0
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
            ld.host(loop_fn, k)
        busy += cpu() - c0
        if first is None and kind != "plain":
            first = ld.budget[k].copy()
        done += 1
        if done == warmup:
            t_begin, busy = now(), 0
    total = now() - t_begin
    check(ld)
    return ld.n * steps / (total * 1e-9), busy / (ld.n * steps), first


def loop_block(eng, ld, kind, steps, warmup, loop_fn):
    """One arm of the blocking call, same triple."""
    h = eng._h
    first = None
    busy = 0
    t_begin = now()
    for i in range(warmup + steps):
        if i == warmup:
            t_begin, busy = now(), 0
        c0 = cpu()
        rc = ld.block(h, kind, 0)
        assert rc == 0, (kind, rc)
        if kind == "host":
            ld.host(loop_fn, 0)
        busy += cpu() - c0
        if first is None and kind != "plain":
            first = ld.budget[0].copy()
    total = now() - t_begin
    check(ld)
    return ld.n * steps / (total * 1e-9), busy / (ld.n * steps), first


def row(eng, ld, loop, steps, warmup, rounds, kinds, loop_fn):
    r = {"transactions_per_call": ld.n, "signatures_per_call": ld.items * (ld.n // len(ld.keep[0])), "steps": steps,
         "txn_per_s": {k: [] for k in kinds}, "thread_ns_per_txn": {k: [] for k in kinds}}
    for rd in range(rounds):
        firsts = {}
        for kind in (kinds if rd % 2 == 0 else kinds[::-1]):
            if hasattr(ld, "budget"):
                for b in ld.budget:
                    b.view(np.uint8)[:] = 0xA5
            s, c, firsts[kind] = loop(eng, ld, kind, steps, warmup, loop_fn)
            r["txn_per_s"][kind].append(round(s))
            r["thread_ns_per_txn"][kind].append(round(c, 2))
        if "budget" in kinds:
            assert np.array_equal(firsts["budget"], firsts["host"]), "the GPU's records differ from the host rule's"
            assert (firsts["budget"]["status"] == 0).all() and (firsts["budget"]["compute"] == 200000).all()
    rng = lambda v: [min(v), max(v)]  # noqa: E731
    med = lambda v: float(np.median(v))  # noqa: E731
    r["range_txn_per_s"] = {k: rng(r["txn_per_s"][k]) for k in kinds}
    r["range_thread_ns_per_txn"] = {k: rng(r["thread_ns_per_txn"][k]) for k in kinds}
    if "budget" in kinds:
        r["budget_over_plain_txn_per_s"] = round(med(r["txn_per_s"]["budget"]) / med(r["txn_per_s"]["plain"]), 4)
        r["budget_over_host_txn_per_s"] = round(med(r["txn_per_s"]["budget"]) / med(r["txn_per_s"]["host"]), 4)
        r["thread_ns_per_txn_budget_minus_plain"] = round(med(r["thread_ns_per_txn"]["budget"]) - med(r["thread_ns_per_txn"]["plain"]), 2)
        r["thread_ns_per_txn_host_minus_plain"] = round(med(r["thread_ns_per_txn"]["host"]) - med(r["thread_ns_per_txn"]["plain"]), 2)
        r["us_per_call_budget_minus_plain"] = round(ld.n / med(r["txn_per_s"]["budget"]) * 1e6 - ld.n / med(r["txn_per_s"]["plain"]) * 1e6, 1)
    return r


def measure(a, kinds, loop_fn):
    res = {}
    budget = "budget" in kinds
    eng = ed25519.Engine(device=0, batch_max=1 << 16, blob_max=1 << 24, nslot=SLOTS)
    try:
        ld = Load(4096, 20272, 1, budget)
        steps, warmup = max(a.steps // 4, 1), max(a.warmup // 4, 1)
        res["submit_4096"] = row(eng, ld, loop_submit, steps, warmup, a.rounds, kinds, loop_fn)
        print(json.dumps({"submit_4096": res["submit_4096"]}), flush=True)
        res["block_4096"] = row(eng, ld, loop_block, max(steps // 2, 1), warmup, a.rounds, kinds, loop_fn)
        print(json.dumps({"block_4096": res["block_4096"]}), flush=True)
        ld.close()
        ld = Load(4096, 20272, 32, budget)
        res["block_131072"] = row(eng, ld, loop_block, max(a.steps // 100, 3), 1, a.rounds, kinds, loop_fn)
        print(json.dumps({"block_131072": res["block_131072"]}), flush=True)
        ld.close()
    finally:
        eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-procs", type=int, default=3, help="child processes per build for the parent comparison")
    ap.add_argument("--plain-only", action="store_true", help="the plain arm alone (what the child on the parent's library runs)")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "budget_cost.json"))
    a = ap.parse_args()
    assert a.rounds >= 3, "at least three runs per arm"
    ab = {"parent": [], "this": []}
    if a.parent_lib:   # before this process touches the GPU: children of their own, the two builds by turns
        tmp = a.out + ".child.tmp"
        for _ in range(a.parent_procs):
            for who in ("parent", "this"):
                env = dict(os.environ)
                env.pop("FD_AMD_LIB", None)
                if who == "parent":
                    env["FD_AMD_LIB"] = os.path.abspath(a.parent_lib)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--steps", str(a.steps), "--warmup",
                                str(a.warmup), "--rounds", str(a.rounds), "--out", tmp], env=env, check=True, timeout=600,
                               stdout=subprocess.DEVNULL)
                ab[who].append(json.load(open(tmp)))
                os.remove(tmp)
                print("plain arm on %s's library: done" % who, flush=True)
    if hip.device_count() < 1:
        sys.exit("budget_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    res = {"tool": "tools/budget_cost.py --steps %d --warmup %d --rounds %d%s" % (a.steps, a.warmup, a.rounds,
                                                                                   " --plain-only" if a.plain_only else ""),
           "device": hip.device_name(0), "version": ed25519.version(), "depth": DEPTH}
    with tempfile.TemporaryDirectory() as tmpdir:
        kinds = ("plain",) if a.plain_only else ("plain", "budget", "host")
        res.update(measure(a, kinds, None if a.plain_only else host_loop(tmpdir)))
    if ab["parent"]:
        cmp = {}
        for k in ("submit_4096", "block_4096", "block_131072"):
            runs = {who: {f: [r[k][f]["plain"] for r in ab[who]] for f in ("txn_per_s", "thread_ns_per_txn")} for who in ab}
            p = sum(runs["parent"]["txn_per_s"], [])
            mine = sum(runs["this"]["txn_per_s"], [])
            cmp[k] = {"parent_plain_txn_per_s_by_process": runs["parent"]["txn_per_s"],
                      "plain_txn_per_s_by_process": runs["this"]["txn_per_s"],
                      "parent_plain_thread_ns_per_txn_by_process": runs["parent"]["thread_ns_per_txn"],
                      "plain_thread_ns_per_txn_by_process": runs["this"]["thread_ns_per_txn"],
                      "parent_range_txn_per_s": [min(p), max(p)], "plain_range_txn_per_s": [min(mine), max(mine)],
                      "plain_median_within_parent_range": bool(min(p) <= float(np.median(mine)) <= max(p)),
                      "plain_median_over_parent_median": round(float(np.median(mine)) / float(np.median(p)), 4)}
        res["parent"] = {"version": ab["parent"][0]["version"], "processes_per_build": a.parent_procs, "order": "parent, this, by turns",
                         "rows": cmp}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
