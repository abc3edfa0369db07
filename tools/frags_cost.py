"""What having the GPU read the frag metadata costs, against the calling thread
walking the mcache lines itself (include/fd_tango_amd.h, "Frag submissions").

Workload: one thread, 4 submissions in flight on an engine with 4 slots; 4096
and 1024 frags of 200-B messages per submission (tools/async_cost.py's arena:
every signature valid, frags 320 bytes apart), listed by an mcache of their
own whose every eighth line names the frag of the line before it (an in-batch
duplicate).  Every submission names the same lines, as keep_cost's loops name
the same pointers.

Arms, run in rounds that alternate their order, each once with keep + emit and
once without (verdicts alone):

  frags  fd_ed25519_amd_submit_frags( seq0, n ): the GPU reads the lines
  today  the loop a caller runs today: it walks the lines into the four
         arrays (fd_ed25519_amd_frags, the native walk), calls
         fd_ed25519_amd_submit_batch_registered[_emit] on them, and at
         delivery compares every line's seq again (one strided numpy compare)

Per arm and round: signatures/s over the loop, and the calling thread's CPU
time per frag (CLOCK_THREAD_CPUTIME_ID around the walk, the submit calls, the
polls that deliver and the recheck; polls that find nothing are a spin and are
left out).  The first deliveries of the two arms must agree in every output.

alone_us: with ONE submission in flight, the median time from before the
submit call to the poll that delivers, per arm; frags minus today is what the
GPU-side listing and the verdict override add to a submission that has the GPU
to itself, less the host's walk and record writing that it no longer waits for.

--parent-lib FILE: the parent commit's library, built in the same session.
Before this process touches the GPU, tools/async_cost.py runs in child
processes of their own, by turns on the parent's library (FD_AMD_LIB) and on
this build's, --parent-procs times each; the async_4 rows (the unchanged
submit call) are reported side by side with whether this build's median lies
inside the parent's run-to-run range.  Nothing here passes or fails on a
ratio: the numbers are reported as they fall.

usage: python tools/frags_cost.py [--steps K] [--warmup W] [--rounds R] [--parent-lib FILE] [--parent-procs N] [--out FILE]
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

from firedancer_amd import ed25519, hip, tango  # noqa: E402
from async_cost import Frags, MSG_SZ, _aligned  # noqa: E402

NONE, DEPTH, SLOTS = 1, 4, 4
FRAG_SZ, FRAG_CHUNKS = 96 + MSG_SZ, 5
now, cpu = time.perf_counter_ns, time.thread_time_ns
HERE = os.path.dirname(os.path.abspath(__file__))
P = ed25519._ptr


class Load:
    def __init__(self, fr, n, full):
        self.n, self.full, self.seq0 = n, full, 0
        self.region = fr.arena
        self.mcache = _aligned(32 * 4096).view(tango.FRAG_META)
        self.mcache[:] = tango.mcache_new(4096, 0)
        for i in range(n):
            tango.publish(self.mcache, i, i, FRAG_CHUNKS * (i - 1 if i % 8 == 7 else i), FRAG_SZ, 0, 0, 0)
        self._m8 = self.mcache.view(np.uint8)
        ed25519.host_register(self._m8)
        self.src = ed25519.frag_src(self.mcache, self.region, FRAG_SZ)
        self.psrc = ctypes.byref(self.src)
        self.seq_view, self.seq_want = self.mcache["seq"][:n], np.arange(n, dtype=np.uint64)
        self.status = np.zeros(n, np.int8)
        self.ptrs = [np.zeros(n, np.uint64) for _ in range(4)]         # pub, sig, msg, sz
        self.err = [np.zeros(n, np.int8) for _ in range(DEPTH)]
        self.keep = [np.zeros(n, np.uint32) for _ in range(DEPTH)]
        self.cnt = [np.zeros(1, np.uint64) for _ in range(DEPTH)]
        self.eoff = [np.zeros(n + 1, np.uint64) for _ in range(DEPTH)]
        self.esz = [np.zeros(n, np.uint32) for _ in range(DEPTH)]
        self.need = (n * ed25519.emit_bound(MSG_SZ) + 4095) & ~4095
        self.ext = _aligned(self.need * DEPTH)
        ed25519.host_register(self.ext)
        self.out = [ctypes.c_void_p(self.ext.ctypes.data + k * self.need) for k in range(DEPTH)]
        L = ed25519.lib()
        self.f_frags, self.f_walk, self.f_ptrs = L.fd_ed25519_amd_submit_frags, L.fd_ed25519_amd_frags, \
            L.fd_ed25519_amd_submit_batch_registered_emit
        # every ctypes argument made once: the loops time the calls, not their wrapping
        pub, sig, msg, sz = (P(x) for x in self.ptrs)
        self.a_walk, self.a_ptrs = (P(self.status), pub, sig, msg, sz), (msg, sz, sig, pub)
        self.a_out = [(P(self.err[k]), None) + self.tail(k) for k in range(DEPTH)]

    def tail(self, k):
        if not self.full:
            return (None, None, None, 0, None, None)
        return (P(self.keep[k]), P(self.cnt[k]), self.out[k], self.need, P(self.eoff[k]), P(self.esz[k]))

    def submit(self, h, kind, k, pt):
        if kind == "frags":
            return self.f_frags(h, self.psrc, self.seq0, self.n, *self.a_out[k], pt)
        good = self.f_walk(self.psrc, self.seq0, self.n, *self.a_walk)
        assert good == self.n
        return self.f_ptrs(h, self.n, *self.a_ptrs, *self.a_out[k], pt)

    def recheck(self):
        assert np.array_equal(self.seq_view, self.seq_want)

    def outputs(self, k):
        o = [self.err[k].copy()]
        if self.full:
            c = int(self.cnt[k][0])
            tot = int(self.eoff[k][c])
            o += [self.keep[k][:c].copy(), self.eoff[k][:c + 1].copy(), self.esz[k][:c].copy(),
                  self.ext[k * self.need:k * self.need + tot].copy()]
        return o

    def close(self):
        ed25519.host_unregister(self._m8)
        ed25519.host_unregister(self.ext)


def loop(eng, ld, kind, steps, warmup, depth=DEPTH):
    """One arm: (signatures/s, thread ns per frag, the first delivery's outputs, median us submit -> delivery)."""
    poll = ed25519.lib().fd_ed25519_amd_async_poll
    t, tk = ctypes.c_ulong(0), ctypes.c_ulong(0)
    pt, ptk = ctypes.byref(t), ctypes.byref(tk)
    h, total_n = eng._h, warmup + steps
    sub = done = busy = 0
    first, t_sub, lat = None, {}, []
    t_begin = now()
    while done < total_n:
        c0 = cpu()
        while sub < total_n and sub - done < depth:
            t0 = now()
            rc = ld.submit(h, kind, sub % DEPTH, pt)
            assert rc == 0, (kind, rc)
            t_sub[t.value] = t0
            sub += 1
        c1 = cpu()
        rc = poll(h, ptk)
        if rc == NONE:
            busy += c1 - c0
            continue
        assert rc == 0, (kind, rc)
        if kind == "today":
            ld.recheck()
        busy += cpu() - c0
        lat.append(now() - t_sub.pop(tk.value))
        if first is None:
            first = ld.outputs(done % DEPTH)
        done += 1
        if done == warmup:
            t_begin, busy, lat = now(), 0, []
    total = now() - t_begin
    for e in ld.err:
        assert ((e == 0) | (e == -3)).all() and (e == -3).mean() < 1e-3, "wrong verdicts"
    return ld.n * steps / (total * 1e-9), busy / (ld.n * steps), first, float(np.median(lat)) / 1e3


def row(eng, ld, steps, warmup, rounds):
    kinds = ("frags", "today")
    r = {"frags_per_submission": ld.n, "keep_and_emit": ld.full, "steps": steps,
         "sig_per_s": {k: [] for k in kinds}, "thread_ns_per_frag": {k: [] for k in kinds}, "alone_us": {k: [] for k in kinds}}
    for rd in range(rounds):
        firsts = {}
        for kind in (kinds if rd % 2 == 0 else kinds[::-1]):
            ld.ext[:] = 0
            s, c, firsts[kind], _ = loop(eng, ld, kind, steps, warmup)
            r["sig_per_s"][kind].append(round(s))
            r["thread_ns_per_frag"][kind].append(round(c, 2))
            r["alone_us"][kind].append(round(loop(eng, ld, kind, max(steps // 4, 8), max(warmup // 4, 2), depth=1)[3], 1))
        for a, b in zip(firsts["frags"], firsts["today"]):
            assert np.array_equal(a, b), "the two arms deliver different outputs"
        if ld.full:
            r["survivors_per_submission"] = int(firsts["frags"][1].size)
    rng = lambda v: [min(v), max(v)]  # noqa: E731
    med = lambda v: float(np.median(v))  # noqa: E731
    for f in ("sig_per_s", "thread_ns_per_frag", "alone_us"):
        r["range_" + f] = {k: rng(r[f][k]) for k in kinds}
    r["frags_over_today_sig_per_s"] = round(med(r["sig_per_s"]["frags"]) / med(r["sig_per_s"]["today"]), 4)
    r["thread_ns_per_frag_frags_minus_today"] = round(med(r["thread_ns_per_frag"]["frags"]) - med(r["thread_ns_per_frag"]["today"]), 2)
    r["alone_us_frags_minus_today"] = round(med(r["alone_us"]["frags"]) - med(r["alone_us"]["today"]), 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-procs", type=int, default=3, help="child processes per build for the parent comparison")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "frags_cost.json"))
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
                subprocess.run([sys.executable, os.path.join(HERE, "async_cost.py"), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                "--polls", "640", "--ab-rounds", "1", "--out", tmp], env=env, check=True, timeout=600,
                               stdout=subprocess.DEVNULL)
                ab[who].append(json.load(open(tmp)))
                os.remove(tmp)
    if hip.device_count() < 1:
        sys.exit("frags_cost: no HIP device (this is a GPU measurement; there is no CPU path)")
    res = {"tool": "tools/frags_cost.py --steps %d --warmup %d --rounds %d" % (a.steps, a.warmup, a.rounds),
           "device": hip.device_name(0), "version": ed25519.version(), "depth": DEPTH, "msg_sz": MSG_SZ,
           "duplicates": "every eighth item"}
    fr = Frags(4096, 20271)
    eng = ed25519.Engine(device=0, batch_max=4096, blob_max=4096 * 256, nslot=SLOTS)
    try:
        for n in (4096, 1024):
            for full in (True, False):
                ld = Load(fr, n, full)
                name = "frags_%d%s" % (n, "_keep_emit" if full else "_plain")
                res[name] = row(eng, ld, a.steps, a.warmup, a.rounds)
                ld.close()
                print(json.dumps({name: res[name]}), flush=True)
    finally:
        eng.close()
        fr.close()
    if ab["parent"]:
        cmp = {}
        for n in (1024, 4096):
            pick = lambda runs: [r["sig_per_s"] for run in runs for r in run["rows"] if r["kind"] == "async_4" and r["n"] == n]  # noqa: E731
            p, mine = pick(ab["parent"]), pick(ab["this"])
            cmp["async_4_%d" % n] = {"parent_sig_per_s_by_process": [round(x) for x in p], "sig_per_s_by_process": [round(x) for x in mine],
                                     "median_within_parent_range": bool(min(p) <= float(np.median(mine)) <= max(p)),
                                     "median_over_parent_median": round(float(np.median(mine)) / float(np.median(p)), 4)}
        res["parent"] = {"version": ab["parent"][0]["version"], "processes_per_build": a.parent_procs, "order": "parent, this, by turns",
                         "tool": "tools/async_cost.py --steps %d --warmup %d" % (a.steps, a.warmup), "rows": cmp}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
