"""GPU: the results of a verify launch are a function of its inputs alone.

Every other test hands the kernels a workspace fresh from hipMalloc and
looks at nothing beside a buffer.  In production no workspace is fresh: the
engine's ring slots, the bench's in-flight workspaces and a caller's
verify_dev workspace are reused launch after launch, with another n (so
another layout), another DSM kernel and another verdict mode.  Here each
launch gets a workspace that already holds something -- zeros, the leftovers
of a real launch, or a per-plane fill chosen to flip a result if it were
read (_wsguard.py) -- and every buffer a kernel writes sits between guards:

  - verdicts, tags, digits and top, decompression planes, R' and work
    statistics equal the expected values and are the same for every poison;
  - every verdict slot is written (d_err pre-filled with 0 and with 1);
  - nothing outside [0, workspace_footprint(n)), d_err[0, n) and the n
    entries of a read-back's output changes, and the inputs stay as they were.

Expected values never come from the GPU: golden.expect, the CPU oracle
(verify_batch, rprime_batch, decompress2), the independent strict verifier
(_strict_ref), _slide and hashlib.  All work is integer, every comparison
exact.  The plane-by-plane table of who writes and who reads what is in
DESIGN.md s2.
"""
import hashlib

import numpy as np
import pytest

import _edges
import _golden
import _oracle
import _slide
import _strict_ref
import _txn
import _wsguard
from _wsguard import Guarded
from test_tags_gpu import _sig_fields, txn_batch   # noqa: F401  (txn_batch: the fixture of test (c))

pytestmark = pytest.mark.gpu

KERNELS = ["k_dsm8", "k_dsm4", "k_dsm", "k_dsmp"]
LATENCY = ("k_dsm8", "k_dsm4")                    # k_front: the decompression runs for every signature
OTHER_KERNEL = {"k_dsm8": "k_dsmp", "k_dsm4": "k_dsm", "k_dsm": "k_dsm8", "k_dsmp": "k_dsm4"}
POOL_WAVES = 2                                    # k_dsmp on two waves: 224 slots for up to 300 signatures, slots refill
OUT_FILL = 0x5A                                   # what a read-back's output holds before the call

MUST = ("offcurve_a", "offcurve_r", "small_order", "noncanon", "false_reject")
SCHECK = ("s_window", "s_range", "malleate")      # the reference's -1 and its accept window
PER_CLASS, PER_EDGE, N_MAX = 10, 8, 300


# ---- the selection and its expected values (CPU, once per module) -------------------------------

class Expect:
    pass


def _build_expect(golden):
    """At most 300 signatures: the first PER_CLASS golden vectors of every
    class -- the MUST classes of test_stage_intermediates_gpu._selection
    first, then the s-check classes, then the rest -- and the first PER_EDGE
    vectors of every class of the _edges corpus (all of both would be 2300),
    dealt round robin so that the prefixes n = 65 and 113 hold every kind
    too, behind one valid signature that is the whole batch at n = 1."""
    rest = tuple(c for c in _golden.CLASSES if c not in MUST + SCHECK)
    _, eb = _edges.corpus()
    groups = []
    for c in MUST + SCHECK + rest:
        idx = np.nonzero(golden.cls == _golden.CLASSES.index(c))[0][:PER_CLASS]
        assert idx.size, c
        groups.append([(golden, int(i)) for i in idx])
    for c in range(len(_edges.CLASSES)):
        idx = np.nonzero(eb.cls == c)[0][:PER_EDGE]
        if idx.size:
            groups.append([(eb, int(i)) for i in idx])
    # index 0, the whole batch at n = 1: a valid signature (every plane it reads can flip its 0)
    lead = (MUST + SCHECK + rest).index("valid")
    order = [groups[lead].pop(0)]
    while any(groups):
        for g in groups:
            if g:
                order.append(g.pop(0))
    order = order[:N_MAX]
    n = len(order)
    E = Expect()
    E.n = n
    E.pub = np.stack([src.pub[i] for src, i in order]).astype(np.uint8)
    E.sig = np.stack([src.sig[i] for src, i in order]).astype(np.uint8)
    msgs = [src.msg(i) for src, i in order]
    E.msgs = msgs
    E.sz = np.array([len(m) for m in msgs], np.uint32)
    E.off = np.concatenate([[0], np.cumsum(E.sz)[:-1]]).astype(np.uint32)
    E.blob = np.frombuffer(b"".join(msgs) + b"\0" * 16, np.uint8).copy()
    b = _golden.Batch(E.pub, E.sig, E.off, E.sz, E.blob)
    E.batch = b

    ref, st = _oracle.verify_batch(b, stats=True)
    from_golden = np.array([src is golden for src, _ in order])
    assert np.array_equal(ref[from_golden], np.array([golden.expect[i] for src, i in order if src is golden], np.int8))
    oerr, ran, oxyz = _oracle.rprime_batch(b)
    assert np.array_equal(oerr, ref)
    strict = np.array(_strict_ref.verify_batch(b), np.int8)
    E.err = {0: ref, 1: strict}
    E.st, E.ran, E.xyz = st, ran, oxyz

    tags = np.array([int.from_bytes(hashlib.sha512(bytes(E.sig[i, :32]) + bytes(E.pub[i]) + msgs[i]).digest()[:8], "little")
                     for i in range(n)], np.uint64)
    tags[ref == -1] = 0
    E.tags = tags

    # k_prep leaves a signature pending exactly when s < L (its -1 and its accept window are both s >= L)
    s = [int.from_bytes(bytes(E.sig[i, 32:]), "little") for i in range(n)]
    E.pending = np.array([v < _slide.L for v in s])
    E.dig = np.zeros((n, 256), np.uint16)
    E.top = np.full(n, -1, np.int32)
    for i in np.nonzero(E.pending)[0]:
        ea = _slide.slide(_slide.h_scalar(E.sig[i], E.pub[i], msgs[i]))
        eb_ = _slide.slide(s[i])
        E.dig[i] = [(a & 0xff) | ((d & 0xff) << 8) for a, d in zip(ea, eb_)]
        nz = [p for p in range(256) if ea[p] or eb_[p]]
        E.top[i] = max(nz) if nz else -1

    E.A, E.R, E.ds = np.zeros((n, 30), np.int32), np.zeros((n, 20), np.int32), np.zeros((n, 2), np.uint8)
    for i in range(n):
        pub, r = bytes(E.pub[i]), bytes(E.sig[i, :32])
        rc, a, _ = _oracle.decompress2(pub, pub)
        E.ds[i, 0] = rc != 0
        E.A[i] = np.concatenate([(-a[0].astype(np.int64)).astype(np.int32), a[1], (-a[3].astype(np.int64)).astype(np.int32)])
        rc, q, _ = _oracle.decompress2(r, r)
        E.ds[i, 1] = rc != 0
        E.R[i] = np.concatenate([q[0], q[1]])
    assert np.array_equal(ran, E.pending & (E.ds == 0).all(axis=1))

    for a in vars(E).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return E


@pytest.fixture(scope="module")
def E(golden):
    return _build_expect(golden)


def test_selection_covers_every_case(E, golden):
    """CPU-side premises: at most 300 signatures; all four codes in both
    modes, in the whole selection and in the prefix of 113; signatures whose
    multiply ran, accepted and rejected; signatures the s check decided
    (k_decomp skips them, strict step 1 answers for them), among them the
    accept window; both kinds of undecodable point; verdicts that differ
    between the modes."""
    assert 113 < E.n <= N_MAX
    assert E.ran[0] and E.err[0][0] == 0 and E.err[1][0] == 0          # n = 1: a signature every plane can flip
    for m in (65, 113, E.n):
        for mode in (0, 1):
            assert set(E.err[mode][:m].tolist()) == {0, -1, -2, -3}, (m, mode)
        assert {0, -3} <= set(E.err[0][:m][E.ran[:m]].tolist())
        assert (~E.pending[:m]).any() and ((E.err[0][:m] == 0) & ~E.pending[:m]).any()
        assert E.ds[:m, 0].any() and E.ds[:m, 1].any()
        assert (E.err[0][:m] != E.err[1][:m]).any()
    assert (E.tags[E.err[0] == -1] == 0).all() and (E.tags[E.err[0] != -1] != 0).all()
    assert (E.st[~E.ran] == 0).all() and (E.st[E.ran, 0] > 0).all()


# ---- one launch, checked ------------------------------------------------------------------------

class Dev:
    """The first n signatures of a batch on the device, and guarded outputs."""

    def __init__(self, b, n):
        from firedancer_amd import hip
        self.n = n
        self.host = [np.ascontiguousarray(a) for a in
                     (b.pub[:n], b.sig[:n], np.asarray(b.msg_off[:n], np.uint32), np.asarray(b.msg_sz[:n], np.uint32), b.blob)]
        self.inp = [hip.DeviceBuffer.from_array(a) for a in self.host]
        self.err = Guarded(n)
        self.out = {"tag": Guarded(8 * n), "dig": Guarded(512 * n), "top": Guarded(4 * n), "A": Guarded(120 * n),
                    "R": Guarded(80 * n), "ds": Guarded(2 * n), "xyz": Guarded(120 * n), "st": Guarded(12 * n)}
        self.stream = hip.Stream()

    def reset(self, prefill):
        self.err.fill(np.full(self.n, prefill, np.int8))
        for g in self.out.values():
            g.fill(np.full(g.nbytes, OUT_FILL, np.uint8))

    def inputs_intact(self):
        for name, h, d in zip(("pub", "sig", "off", "sz", "blob"), self.host, self.inp):
            assert np.array_equal(d.to_array(np.uint8, h.nbytes), h.view(np.uint8).reshape(-1)), name

    def close(self):
        self.stream.destroy()


def _launch(dev, ws, kernel, mode, prefill, readback=True):
    """verify_dev of dev's batch on workspace ws with `kernel` forced (k_dsmp
    on POOL_WAVES waves), d_err pre-filled, then every read-back; synchronised."""
    from firedancer_amd import ed25519
    n, o, s = dev.n, dev.out, dev.stream.handle
    dev.reset(prefill)
    try:
        ed25519.select_dsm_kernel(kernel)
        if kernel == "k_dsmp":
            ed25519.debug_set_pool_waves(POOL_WAVES)
        ed25519.verify_dev(n, *[x.ptr for x in dev.inp], dev.err.ptr, ws.ptr, s, mode=mode)
        if readback:
            ed25519.tags_dev(n, ws.ptr, o["tag"].ptr, s)
            ed25519.debug_digits_dev(n, ws.ptr, o["dig"].ptr, o["top"].ptr, s)
            ed25519.debug_points_dev(n, ws.ptr, o["A"].ptr, o["R"].ptr, o["ds"].ptr, s)
            ed25519.debug_rprime_dev(n, ws.ptr, kernel, o["xyz"].ptr, s)
            ed25519.work_stats_dev(n, ws.ptr, o["st"].ptr, s)
        dev.stream.synchronize()
    finally:
        ed25519.debug_set_pool_waves(0)
        ed25519.select_dsm_kernel("default")


def _first_bad(got, want):
    bad = np.nonzero(np.asarray(got != want).reshape(len(want), -1).any(axis=1))[0]
    return int(bad.size), bad[:8].tolist()


def _run_checked(E, dev, ws, kernel, mode, prefill, what):
    """One launch on ws as it stands, everything compared with E.  Returns
    the results with their undefined parts masked out, for comparison across
    poisons."""
    from firedancer_amd import ed25519
    n = dev.n
    total = ed25519.workspace_footprint(n)
    assert ws.nbytes >= total
    beyond = ws.body()[total:] if ws.nbytes > total else None
    _launch(dev, ws, kernel, mode, prefill)
    what = (what, kernel, mode, n, prefill)

    # nothing outside the footprint, d_err[0, n) and the read-backs' n entries
    ws.check(what)
    dev.err.check(what)
    for name, g in dev.out.items():
        g.check(what + (name,))
    if beyond is not None:
        assert np.array_equal(ws.body()[total:], beyond), ("workspace written past the footprint",) + what

    err = dev.err.body(np.int8)
    assert not (err == ed25519.VERDICT_DEVICE).any(), ("step guard",) + what
    assert np.array_equal(err, E.err[mode][:n]), ("verdicts",) + what + _first_bad(err, E.err[mode][:n])
    tag = dev.out["tag"].body(np.uint64)
    assert np.array_equal(tag, E.tags[:n]), ("tags",) + what + _first_bad(tag, E.tags[:n])

    # k_prep writes evn / top for every signature: no event and top -1 where the s check decided
    dig = dev.out["dig"].body(np.uint16).reshape(n, 256)
    top = dev.out["top"].body(np.int32)
    assert np.array_equal(dig, E.dig[:n]), ("digits",) + what + _first_bad(dig, E.dig[:n])
    assert np.array_equal(top, E.top[:n]), ("top",) + what + _first_bad(top, E.top[:n])

    # the decompression ran for every signature (k_front) or for the pending ones (gated k_decomp)
    did = np.ones(n, bool) if kernel in LATENCY else E.pending[:n].copy()
    ds = dev.out["ds"].body(np.uint8).reshape(n, 2)
    A = dev.out["A"].body(np.int32).reshape(30, n).T
    Rr = dev.out["R"].body(np.int32).reshape(20, n).T
    assert np.array_equal(ds[did], E.ds[:n][did]), ("ds flags",) + what + _first_bad(ds[did], E.ds[:n][did])
    okA, okR = did & (E.ds[:n, 0] == 0), did & (E.ds[:n, 1] == 0)
    assert np.array_equal(A[okA], E.A[:n][okA]), ("A limbs",) + what + _first_bad(A[okA], E.A[:n][okA])
    assert np.array_equal(Rr[okR], E.R[:n][okR]), ("R limbs",) + what + _first_bad(Rr[okR], E.R[:n][okR])

    ran = E.ran[:n]
    xyz = dev.out["xyz"].body(np.int32).reshape(30, n).T
    assert np.array_equal(xyz[ran], E.xyz[:n][ran]), ("R' limbs",) + what + _first_bad(xyz[ran], E.xyz[:n][ran])
    st = dev.out["st"].body(np.uint32).reshape(3, n).T
    assert np.array_equal(st, E.st[:n]), ("work stats",) + what + _first_bad(st, E.st[:n])
    return [err, tag, dig, top, ds[did], A[okA], Rr[okR], xyz[ran], st]


def _reversed_batch(E):
    """The selection in reverse order: row i of its leftovers belongs to
    another signature than row i of the launch under test."""
    return _golden.Batch(E.pub[::-1].copy(), E.sig[::-1].copy(), E.off[::-1].copy(), E.sz[::-1].copy(), E.blob)


# ---- a. nothing depends on the workspace --------------------------------------------------------

POISONS = ("zero", "directed", "leftover")


class PoisonCase:
    """The launches of (a) for one (kernel, mode, n): run( poison, prefill )
    poisons a workspace and returns _run_checked's results.

    zero / directed: a workspace of exactly workspace_footprint(n) bytes (what
    a caller allocates) between its guards, filled over the planes of the
    layout the kernels are launched with.  leftover: a workspace as a real
    launch left it -- the selection in reverse order through another kernel
    in the other mode, all of it (so a larger n, another layout) or, under the
    full-size launch, all but one (the same layout, every row another
    signature's); it is as large as that launch needed, and what lies past
    footprint(n) must stay as that launch left it."""

    def __init__(self, E, kernel, mode, n):
        from firedancer_amd import ed25519
        self.E, self.kernel, self.mode, self.n = E, kernel, mode, n
        self.L = ed25519.debug_ws_layout(n)
        self.m = E.n if n < E.n else E.n - 1
        self.dev, self.prior = Dev(E.batch, n), Dev(_reversed_batch(E), self.m)
        fp = ed25519.workspace_footprint(n)
        self.ws = Guarded(fp)
        self.ws_left = Guarded(max(fp, ed25519.workspace_footprint(self.m)))

    def run(self, poison, prefill):
        E, kernel, mode = self.E, self.kernel, self.mode
        if poison == "leftover":
            _launch(self.prior, self.ws_left, OTHER_KERNEL[kernel], 1 - mode, 0x55, readback=False)
            assert np.array_equal(self.prior.err.body(np.int8), E.err[1 - mode][::-1][:self.m])
            return _run_checked(E, self.dev, self.ws_left, kernel, mode, prefill, poison)
        img = np.zeros(self.ws.nbytes, np.uint8)
        if poison == "directed":
            d = _wsguard.directed(self.L, self.n)
            k = min(d.nbytes, img.nbytes)
            img[:k] = d[:k]
        self.ws.fill(img)
        return _run_checked(E, self.dev, self.ws, kernel, mode, prefill, poison)

    def close(self):
        for d in (self.dev, self.prior):
            d.inputs_intact()
            d.close()
        for g in (self.ws, self.ws_left):
            g.free()


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_results_do_not_depend_on_workspace_contents(E, kernel, mode):
    """For n = 1, 65, 113 and the whole selection, each poison of PoisonCase
    twice -- d_err pre-filled with 0 and with 1 -- and every result the same
    for all six."""
    for n in (1, 65, 113, E.n):
        case = PoisonCase(E, kernel, mode, n)
        first = None
        for poison in POISONS:
            for prefill in (0, 1):
                got = case.run(poison, prefill)
                first = got if first is None else first
                for x, y in zip(got, first):
                    assert np.array_equal(x, y), (poison, prefill, n)
        case.close()


# ---- b. one workspace, many launches ------------------------------------------------------------

def test_one_workspace_many_launches(E):
    """One workspace sized for the largest n, never cleared: twelve launches
    that change kernel, mode and n every time (so the layout moves under the
    leftovers), each checked like a launch of (a).  Two k_dsmp launches start
    from the state a tripped step guard leaves -- the ctr pair seeded with a
    counter past n and the guard flag 1 (the directed ctr fill; the guard
    itself is not tripped): k_ai must zero both."""
    from firedancer_amd import ed25519
    R_, S_ = 0, 1
    seq = [("k_dsmp", S_, E.n, False), ("k_dsm8", R_, 64, False), ("k_dsm", S_, 113, False), ("k_dsm4", R_, 1, False),
           ("k_dsmp", R_, 65, False), ("k_dsm4", S_, E.n, False), ("k_dsmp", S_, 113, True), ("k_dsm", R_, E.n, False),
           ("k_dsm8", S_, 65, False), ("k_dsmp", R_, E.n, True), ("k_dsm", R_, 1, False), ("k_dsm8", R_, E.n, False)]
    assert len(seq) >= 8 and {k for k, _, _, _ in seq} == set(KERNELS)
    ws = Guarded(ed25519.workspace_footprint(E.n))
    devs = {n: Dev(E.batch, n) for n in sorted({n for _, _, n, _ in seq})}
    for k, (kernel, mode, n, seed_ctr) in enumerate(seq):
        if seed_ctr:
            L = ed25519.debug_ws_layout(n)
            ws.write(L["ctr"], _wsguard.directed_planes(L, n)["ctr"])
        _run_checked(E, devs[n], ws, kernel, mode, k & 1, "launch %d" % k)
    for d in devs.values():
        d.inputs_intact()
        d.close()


# ---- c. transactions ----------------------------------------------------------------------------

def _txn_ws_layout(txn_cnt, slots):
    """txn_ws_layout of fd_ed25519_engine.cpp: the verify workspace of `slots`
    signatures at offset 0, then the planes k_txn_parse fills slot by slot."""
    from firedancer_amd import ed25519
    S, o, L = max(slots, 1), 0, {}
    for name, size in (("vws", ed25519.workspace_footprint(S)), ("pub", 32 * S), ("sig", 64 * S), ("off", 4 * S),
                       ("sz", 4 * S), ("skip", S), ("err", S), ("fp", 4 * max(txn_cnt, 1))):
        L[name] = o
        o = (o + size + 255) & ~255
    L["total"] = o
    return L


class TxnDev:
    def __init__(self, blob, off, sz):
        from firedancer_amd import ed25519, hip
        self.n = len(off)
        self.tbase, self.slots = ed25519.txn_slots(blob, off, sz)
        self.host = [np.ascontiguousarray(a) for a in (blob, off, sz, self.tbase)]
        self.inp = [hip.DeviceBuffer.from_array(a) for a in self.host]
        self.terr, self.serr = Guarded(self.n), Guarded(self.slots)
        self.ttag, self.stag = Guarded(8 * self.n), Guarded(8 * self.slots)
        self.stream = hip.Stream()

    def run(self, ws, mode, kernel, what):
        """(txn_err, sig_err, txn tags, slot tags) of one verify_txns_dev on ws as it stands."""
        from firedancer_amd import ed25519
        s = self.stream.handle
        self.terr.fill(np.zeros(self.n, np.int8))
        self.serr.fill(np.zeros(self.slots, np.int8))
        for g in (self.ttag, self.stag):
            g.fill(np.full(g.nbytes, OUT_FILL, np.uint8))
        try:
            ed25519.select_dsm_kernel(kernel)
            if kernel == "k_dsmp":
                ed25519.debug_set_pool_waves(POOL_WAVES)
            ed25519.verify_txns_dev(self.n, self.slots, *[b.ptr for b in self.inp], self.terr.ptr, self.serr.ptr, ws.ptr, s,
                                    mode=mode)
            ed25519.txn_tags_dev(self.n, self.inp[3].ptr, ws.ptr, self.ttag.ptr, s)
            ed25519.tags_dev(self.slots, ws.ptr, self.stag.ptr, s)
            self.stream.synchronize()
        finally:
            ed25519.debug_set_pool_waves(0)
            ed25519.select_dsm_kernel("default")
        for name, g in (("ws", ws), ("txn_err", self.terr), ("sig_err", self.serr), ("txn tags", self.ttag),
                        ("slot tags", self.stag)):
            g.check((what, name))
        for h, d in zip(self.host, self.inp):
            assert np.array_equal(d.to_array(np.uint8, h.nbytes), h.view(np.uint8).reshape(-1)), what
        return self.terr.body(np.int8), self.serr.body(np.int8), self.ttag.body(np.uint64), self.stag.body(np.uint64)


@pytest.mark.parametrize("kernel", ["default", "k_dsmp"])
def test_transactions_ignore_stale_slots(txn_batch, kernel):
    """verify_txns_dev over a guarded transaction workspace: zeroed; with the
    directed fill over its verify part and zeros in the parse planes (a stale
    skip of 0 says "verify this slot"); and as a batch with the same 37 slots
    left it in which EVERY signature was valid -- so each of the 19 slots of
    the payload that fails to parse holds a signature that verifies, and a
    slot the parse kernel did not mark would report 0.  Both modes."""
    from firedancer_amd import ed25519, workload
    blob, off, sz, eterr, ebase, eserr, ttag, stag = txn_batch
    pays = [bytes(blob[o:o + s]) for o, s in zip(off.tolist(), sz.tolist())]
    dev = TxnDev(blob, off, sz)
    n, slots = dev.n, dev.slots
    assert np.array_equal(dev.tbase, ebase) and slots == 37

    # strict verdicts: the first failing signature's code; a parse failure stays -4 in both modes
    sterr, sserr = eterr.copy(), eserr.copy()
    for t, p in enumerate(pays):
        if eterr[t] == ed25519.FD_TXN_AMD_ERR_PARSE:
            continue
        k, m, a = _sig_fields(p)
        v = [_strict_ref.verify(p[m:], p[1 + 64 * j:65 + 64 * j], p[a + 32 * j:a + 32 * j + 32]) for j in range(k)]
        sserr[ebase[t]:ebase[t + 1]] = v
        sterr[t] = next((x for x in v if x), 0)
    assert (eserr[ebase[2]:ebase[3]] == ed25519.FD_TXN_AMD_ERR_PARSE).all() and ebase[3] - ebase[2] == 19
    want = {0: (eterr, eserr), 1: (sterr, sserr)}

    # the all-valid batch: 12 + 12 + 2 + 2 + 2 + 2 + 5 signers
    valid = (_txn.build_txns(911, 2, nsig_lo=12, nsig_hi=12)[0] + _txn.build_txns(912, 4, nsig_lo=2, nsig_hi=2, msg_hi=300)[0] +
             _txn.build_txns(913, 1, nsig_lo=5, nsig_hi=5, msg_hi=300)[0])
    vdev = TxnDev(*_txn.pack(valid))
    assert (vdev.n, vdev.slots) == (n, slots)
    vt, _, vs = _oracle.txn_verify_batch(*_txn.pack(valid))
    assert not vt.any() and not vs.any()

    TL = _txn_ws_layout(n, slots)
    total = workload._bind().fd_ed25519_amd_txn_workspace_footprint(n, slots)
    assert TL["total"] == total and TL["vws"] == 0
    VL = ed25519.debug_ws_layout(slots)
    assert VL["total"] <= TL["pub"]
    ws = Guarded(total)
    k_ = "k_dsm" if kernel == "k_dsmp" else "k_dsmp"          # the leftover batch goes through another kernel
    for mode in (0, 1):
        for poison in ("zero", "directed", "leftover"):
            if poison == "leftover":
                lt, ls, _, _ = vdev.run(ws, 1 - mode, k_, "all-valid batch")
                assert not lt.any() and not ls.any()
            else:
                img = np.zeros(total, np.uint8)
                if poison == "directed":
                    img[:VL["total"]] = _wsguard.directed(VL, slots)
                ws.fill(img)
            terr, serr, gt, gs = dev.run(ws, mode, kernel, (poison, mode))
            assert np.array_equal(terr, want[mode][0]), (poison, mode, terr.tolist())
            assert np.array_equal(serr, want[mode][1]), (poison, mode, serr.tolist())
            assert np.array_equal(gt, ttag) and np.array_equal(gs, stag), (poison, mode)


# ---- d. separate workspaces in flight -----------------------------------------------------------

def test_four_launches_in_flight_on_four_workspaces():
    """Four streams, four guarded workspaces, four batches of 1024 fresh
    signatures (0..400 B, 10 % corrupted): two k_dsmp and two k_dsm launches
    enqueued back to back without a synchronise between them, then all four
    synchronised.  Every verdict and tag is the oracle's and every guard is
    intact.  Whether the launches overlapped on the device is up to the
    runtime and cannot be observed from here: this asserts nothing about
    timing, only that launches which MAY overlap share no state but the
    read-only tables."""
    from firedancer_amd import ed25519
    from test_gpu_parity import _sign_stream
    n = 1024
    bs = [_sign_stream(5150 + k, n, 0, 400, True) for k in range(4)]
    want = [_oracle.verify_batch(b) for b in bs]
    assert all({0, -3} <= set(w.tolist()) for w in want)
    devs, wss = [], []
    for b in bs:
        b.blob = np.concatenate([np.asarray(b.blob, np.uint8), np.zeros(16, np.uint8)])
        devs.append(Dev(b, n))
        wss.append(Guarded(ed25519.workspace_footprint(n), _wsguard.directed(ed25519.debug_ws_layout(n), n)))
    for d in devs:
        d.reset(1)
    try:
        for k, kernel in enumerate(("k_dsmp", "k_dsm", "k_dsmp", "k_dsm")):
            ed25519.select_dsm_kernel(kernel)          # read by the launch code, on the host
            d = devs[k]
            ed25519.verify_dev(n, *[x.ptr for x in d.inp], d.err.ptr, wss[k].ptr, d.stream.handle, mode=k >> 1)
            ed25519.tags_dev(n, wss[k].ptr, d.out["tag"].ptr, d.stream.handle)
        for d in devs:
            d.stream.synchronize()
    finally:
        ed25519.select_dsm_kernel("default")
    for k, (b, d) in enumerate(zip(bs, devs)):
        wss[k].check(k)
        d.err.check(k)
        d.out["tag"].check(k)
        exp = want[k] if k < 2 else np.array(_strict_ref.verify_batch(b), np.int8)
        err = d.err.body(np.int8)
        assert np.array_equal(err, exp), (k, _first_bad(err, exp))
        tags = np.array([int.from_bytes(hashlib.sha512(bytes(b.sig[i, :32]) + bytes(b.pub[i]) + b.msg(i)).digest()[:8], "little")
                         for i in range(n)], np.uint64)
        tags[want[k] == -1] = 0
        assert np.array_equal(d.out["tag"].body(np.uint64), tags), k
        d.inputs_intact()
        d.close()
