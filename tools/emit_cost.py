"""What having the GPU write the survivors' output frames costs, against the
calling thread copying them (include/fd_ed25519_amd.h, "Output frames").

Workload: tools/keep_cost.py's loops, unchanged -- one thread, 4 submissions
in flight on an engine with 4 slots; sig_4096 and sig_1024 (registered 200-B
frags), txn_4096 (the bench's config-4 transaction mix); every signature
valid, one item in eight an in-batch duplicate.

Arms, run in rounds that alternate their order:

  keep   the _keep submission alone: verdicts and the publish list; no frame
         is written by anybody (keep_cost's `keep` variant)
  emit   the _emit submission: the GPU writes the frames into a registered
         extent of the submission's own; the thread reads emit_off / emit_sz
  host   the _keep submission (for transactions with desc / desc_off, which
         the frames need) and then fd_ed25519_amd_emit / fd_txn_amd_emit on
         the calling thread into the same extent

Two figures per arm and round: signatures/s over the loop, and the calling
thread's CPU time per signature (CLOCK_THREAD_CPUTIME_ID around the submit
calls, the polls that deliver and the host copy; polls that find nothing are a
spin and are left out).  The first delivery of `emit` and of `host` in a round
must leave the same bytes in their extents.

--parent-lib FILE: the parent commit's library, built in the same session.
Before it touches the GPU itself the tool runs the `keep` arm alone in child
processes of their own, by turns on the parent's library (FD_AMD_LIB) and on
this build's, --parent-procs times each, and reports whether the median of
this build's runs lies inside the range of the parent's: the feature must add
nothing to a call that does not ask for it.  (A process differs from the next
by more than its own rounds differ from each other, so the run-to-run range
is taken over processes.)  Nothing here passes or fails on a ratio: the
numbers are reported as they fall.

usage: python tools/emit_cost.py [--steps K] [--warmup W] [--rounds R] [--parent-lib FILE] [--parent-procs N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from firedancer_amd import ed25519, hip  # noqa: E402
from async_cost import Frags, _aligned  # noqa: E402
from keep_cost import SigLoad, TxnLoad  # noqa: E402

NONE, DEPTH, SLOTS = 1, 4, 4
now, cpu = time.perf_counter_ns, time.thread_time_ns
HERE = os.path.dirname(os.path.abspath(__file__))
P = ed25519._ptr


class Extents:
    """DEPTH extents of `need` bytes each in one registered block, and the
    emit_off / emit_sz arrays of each."""

    def __init__(self, need, n):
        self.need = (need + 4095) & ~4095
        self.mem = _aligned(self.need * DEPTH)
        ed25519.host_register(self.mem)
        self.out = [self.mem[k * self.need:(k + 1) * self.need] for k in range(DEPTH)]
        self.ptr = [ctypes.c_void_p(o.ctypes.data) for o in self.out]
        self.eoff = [np.zeros(n + 1, np.uint64) for _ in range(DEPTH)]
        self.esz = [np.zeros(n, np.uint32) for _ in range(DEPTH)]

    def close(self):
        ed25519.host_unregister(self.mem)


class SigEmit(SigLoad):
    def __init__(self, fr, n, emit=True):
        super().__init__(fr, n)
        L = ed25519.lib()
        self.txn = False
        if emit:
            self.f_emit, self.f_host = L.fd_ed25519_amd_submit_batch_registered_emit, L.fd_ed25519_amd_emit
            self.x = Extents(sum(ed25519.emit_bound(int(z)) for z in self._a[1]), n)

    def submit(self, h, kind, k, pt):
        if kind == "emit":
            x = self.x
            return self.f_emit(h, self.n, *self.args, P(self.err[k]), None, P(self.keep[k]), P(self.cnt[k]), x.ptr[k], x.need,
                               P(x.eoff[k]), P(x.esz[k]), pt)
        return super().submit(h, "keep", k, pt)

    def host_emit(self, k):
        x = self.x
        m, z, s, p = self.args
        return self.f_host(int(self.cnt[k][0]), P(self.keep[k]), m, z, s, p, x.ptr[k], x.need, P(x.eoff[k]), P(x.esz[k]))


class TxnEmit(TxnLoad):
    def __init__(self, n_txn, seed, emit=True):
        super().__init__(n_txn, seed)
        L = ed25519.lib()
        self.txn = True
        if emit:
            self.f_emit, self.f_host = L.fd_ed25519_amd_submit_txns_registered_emit, L.fd_txn_amd_emit
            self.x = Extents(sum(ed25519.txn_emit_bound(int(z)) for z in self._sz), self.n)
            dcap = sum(ed25519.txn_desc_bound(int(z)) for z in self._sz)
            self.doff = [np.zeros(self.n + 1, np.uint64) for _ in range(DEPTH)]
            self.desc = [np.zeros(dcap, np.uint8) for _ in range(DEPTH)]

    def submit(self, h, kind, k, pt):
        if kind == "keep":
            return super().submit(h, "keep", k, pt)
        desc = (P(self.doff[k]), P(self.desc[k]), int(self.desc[k].size)) if kind == "host" else (None, None, 0)
        head = (h, self.n, *self.args, P(self.err[k]), None, None, None, None, *desc, P(self.keep[k]), P(self.cnt[k]))
        if kind == "host":
            return self.f_keep(*head, pt)
        x = self.x
        return self.f_emit(*head, x.ptr[k], x.need, P(x.eoff[k]), P(x.esz[k]), pt)

    def host_emit(self, k):
        x = self.x
        return self.f_host(int(self.cnt[k][0]), P(self.keep[k]), *self.args, P(self.doff[k]), P(self.desc[k]), x.ptr[k], x.need,
                           P(x.eoff[k]), P(x.esz[k]))

    def close(self):
        super().close()
        if hasattr(self, "x"):
            self.x.close()


def loop(eng, ld, kind, steps, warmup):
    """One arm: (signatures/s, thread ns per signature, the first delivery's extent bytes or None)."""
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
        tot = None
        if kind == "host":
            tot = int(ld.host_emit(k))
            assert tot <= ld.x.need
        elif kind == "emit":
            tot = int(ld.x.eoff[k][int(ld.cnt[k][0])])
        busy += cpu() - c0
        if first is None and tot is not None:
            c = int(ld.cnt[k][0])
            first = (ld.x.out[k][:tot].copy(), ld.x.eoff[k][:c + 1].copy(), ld.x.esz[k][:c].copy())
        done += 1
        if done == warmup:
            t_begin, busy = now(), 0
    total = now() - t_begin
    for e in ld.err:
        assert ((e == 0) | (e == -3)).all() and (e == -3).mean() < 1e-3, "wrong verdicts"
    return ld.items * steps / (total * 1e-9), busy / (ld.items * steps), first


def row(eng, ld, steps, warmup, rounds, kinds):
    r = {"items_per_batch": ld.n, "signatures_per_batch": ld.items, "steps": steps,
         "sig_per_s": {k: [] for k in kinds}, "thread_ns_per_sig": {k: [] for k in kinds}}
    for rd in range(rounds):
        firsts = {}
        for kind in (kinds if rd % 2 == 0 else kinds[::-1]):
            if hasattr(ld, "x"):
                ld.x.mem[:] = 0
            s, c, firsts[kind] = loop(eng, ld, kind, steps, warmup)
            r["sig_per_s"][kind].append(round(s))
            r["thread_ns_per_sig"][kind].append(round(c, 2))
        if "emit" in kinds:
            for a, b in zip(firsts["emit"], firsts["host"]):
                assert np.array_equal(a, b), "the GPU's frames differ from the host's"
            r["frame_bytes_per_batch"] = int(firsts["emit"][0].size)
            r["survivors_per_batch"] = int(firsts["emit"][2].size)
    rng = lambda v: [min(v), max(v)]  # noqa: E731
    r["range_sig_per_s"] = {k: rng(r["sig_per_s"][k]) for k in kinds}
    r["range_thread_ns_per_sig"] = {k: rng(r["thread_ns_per_sig"][k]) for k in kinds}
    if "emit" in kinds:
        med = lambda v: float(np.median(v))  # noqa: E731
        r["emit_over_host_sig_per_s"] = round(med(r["sig_per_s"]["emit"]) / med(r["sig_per_s"]["host"]), 4)
        r["emit_over_keep_sig_per_s"] = round(med(r["sig_per_s"]["emit"]) / med(r["sig_per_s"]["keep"]), 4)
        r["thread_ns_per_sig_emit_minus_host"] = round(med(r["thread_ns_per_sig"]["emit"]) - med(r["thread_ns_per_sig"]["host"]), 2)
        per_us = ld.items / med(r["sig_per_s"]["keep"]) * 1e6, ld.items / med(r["sig_per_s"]["emit"]) * 1e6
        r["us_per_batch_emit_minus_keep"] = round(per_us[1] - per_us[0], 1)
    return r


def measure(a, kinds):
    res = {}
    emit = "emit" in kinds
    fr = Frags(4096, 20271)
    eng = ed25519.Engine(device=0, batch_max=4096, blob_max=4096 * 256, nslot=SLOTS)
    try:
        for n in (4096, 1024):
            ld = SigEmit(fr, n, emit)
            res["sig_%d" % n] = row(eng, ld, a.steps, a.warmup, a.rounds, kinds)
            if emit:
                ld.x.close()
            print(json.dumps({"sig_%d" % n: res["sig_%d" % n]}), flush=True)
    finally:
        eng.close()
        fr.close()
    tx = TxnEmit(4096, 20272, emit)
    eng = ed25519.Engine(device=0, batch_max=1 << 16, blob_max=1 << 24, nslot=SLOTS)
    try:
        res["txn_4096"] = row(eng, tx, max(a.steps // 4, 1), max(a.warmup // 4, 1), a.rounds, kinds)
        print(json.dumps({"txn_4096": res["txn_4096"]}), flush=True)
    finally:
        eng.close()
        tx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-procs", type=int, default=3, help="child processes per build for the parent comparison")
    ap.add_argument("--keep-only", action="store_true", help="the keep arm alone (what the child on the parent's library runs)")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "emit_cost.json"))
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
                subprocess.run([sys.executable, os.path.abspath(__file__), "--keep-only", "--steps", str(a.steps), "--warmup",
                                str(a.warmup), "--rounds", str(a.rounds), "--out", tmp], env=env, check=True, timeout=600,
                               stdout=subprocess.DEVNULL)
                ab[who].append(json.load(open(tmp)))
                os.remove(tmp)
    if hip.device_count() < 1:
        sys.exit("emit_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    res = {"tool": "tools/emit_cost.py --steps %d --warmup %d --rounds %d%s" % (a.steps, a.warmup, a.rounds,
                                                                                 " --keep-only" if a.keep_only else ""),
           "device": hip.device_name(0), "version": ed25519.version(), "depth": DEPTH, "duplicates": "every eighth item"}
    res.update(measure(a, ("keep",) if a.keep_only else ("keep", "emit", "host")))
    if ab["parent"]:
        cmp = {}
        for k in ("sig_4096", "sig_1024", "txn_4096"):
            runs = {who: {f: [r[k][f]["keep"] for r in ab[who]] for f in ("sig_per_s", "thread_ns_per_sig")} for who in ab}
            p = sum(runs["parent"]["sig_per_s"], [])
            mine = sum(runs["this"]["sig_per_s"], [])
            cmp[k] = {"parent_keep_sig_per_s_by_process": runs["parent"]["sig_per_s"],
                      "keep_sig_per_s_by_process": runs["this"]["sig_per_s"],
                      "parent_keep_thread_ns_per_sig_by_process": runs["parent"]["thread_ns_per_sig"],
                      "keep_thread_ns_per_sig_by_process": runs["this"]["thread_ns_per_sig"],
                      "parent_range_sig_per_s": [min(p), max(p)], "keep_range_sig_per_s": [min(mine), max(mine)],
                      "keep_median_within_parent_range": bool(min(p) <= float(np.median(mine)) <= max(p)),
                      "keep_median_over_parent_median": round(float(np.median(mine)) / float(np.median(p)), 4)}
        res["parent"] = {"version": ab["parent"][0]["version"], "processes_per_build": a.parent_procs, "order": "parent, this, by turns",
                         "rows": cmp}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
