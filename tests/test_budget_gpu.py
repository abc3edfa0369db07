"""GPU: the compute budget records (include/fd_txn_amd.h, "Compute budget")
from k_txn_budget -- the device-resident step fd_txn_amd_budget_dev, the two
blocking calls and the two submissions that take `budget`.

The expected record of a payload is the host rule's (fd_txn_amd_budget over
the oracle's descriptor), which test_budget_cpu.py holds equal to the
reference's own functions and to the Python restatement over the same corpus
(tests/_budget.py).  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import _budget as B
import _oracle
import _txn

pytestmark = pytest.mark.gpu

OK, INVAL, BUSY, ERR_PARSE = 0, -10, -12, -4
PAGE, GUARD, FILL = 4096, 4096, 0xA5
CAP, BLOB, SLOTS = 64, 64 * 1232, 4

_want = {}


def want(p):
    """The host rule's record of payload p as a REC tuple, cached."""
    from firedancer_amd import ed25519
    p = bytes(p)
    r = _want.get(p)
    if r is None:
        fp, desc, _ = _oracle.txn_parse(p)
        r = _want[p] = tuple(int(x) for x in ed25519.txn_budget(p, desc[:fp]).tolist())
    return r


def want_array(pays):
    from firedancer_amd import ed25519
    return np.array([want(p) for p in pays], ed25519.BUDGET_DTYPE)


def _dt():
    from firedancer_amd import ed25519
    return ed25519.BUDGET_DTYPE


def same_records(got, pays, what=""):
    from firedancer_amd import ed25519
    w = want_array(pays)
    assert got.dtype == ed25519.BUDGET_DTYPE and got.shape == w.shape, what
    bad = np.nonzero(got != w)[0]
    assert bad.size == 0, (what, bad[:8], got[bad[:4]], w[bad[:4]])


# ---- 1. the device-resident step -----------------------------------------------------------------

def dev_list():
    """Payloads for the step alone: 355 instructions and one instruction side
    by side in the first wave, then the corpus and the 355-instruction
    payloads above the MTU, repeated to 129."""
    c, big = dict(B.cases()), dict(B.big_cases())
    head = [big["instr_355_first"], c["none_1"], c["mtu_355_none"], c["kind_limit"], big["instr_355_last"], c["noparse_empty"]]
    rest = [p for _, p in B.cases()] + [p for n, p in B.big_cases() if n != "max_size"]
    out = head + rest
    return (out + rest)[:129]


def budget_dev(pays, fp_force=None):
    """fd_txn_amd_parse_dev then fd_txn_amd_budget_dev over pays; the record
    plane is FILL before the call and has GUARD bytes on both sides.
    fp_force: a footprint plane to use in place of the parser's.  Returns
    (footprints, records)."""
    from firedancer_amd import ed25519, hip
    n = len(pays)
    blob, off, sz = _txn.pack(pays)
    d_blob, d_off, d_sz = (hip.DeviceBuffer.from_array(a) for a in (blob, off, sz))
    d_fp = hip.DeviceBuffer.from_array(np.full(n, 0xDEADBEEF, np.uint32))
    d_b = hip.DeviceBuffer.from_array(np.full(2 * GUARD + 24 * n, FILL, np.uint8))
    stream = hip.Stream()
    ed25519.txn_parse_dev(n, d_blob.ptr, d_off.ptr, d_sz.ptr, d_fp.ptr, None, 0, stream.handle)
    stream.synchronize()
    fp = d_fp.to_array(np.uint32, n)
    if fp_force is not None:
        d_fp.free()
        d_fp = hip.DeviceBuffer.from_array(np.ascontiguousarray(fp_force, np.uint32))
    ed25519.txn_budget_dev(n, d_blob.ptr, d_off.ptr, d_sz.ptr, d_fp.ptr, d_b.ptr + GUARD, stream.handle)
    stream.synchronize()
    raw = d_b.to_array(np.uint8, 2 * GUARD + 24 * n)
    for b in (d_blob, d_off, d_sz, d_fp, d_b):
        b.free()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 24 * n:] == FILL).all(), "a guard byte changed"
    return fp, raw[GUARD:GUARD + 24 * n].copy().view(ed25519.BUDGET_DTYPE)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_1_budget_dev_equals_the_host_rule(n):
    pays = dev_list()[:n]
    assert n == 1 or {len(pays[0]), len(pays[1])} == {1273, 206}
    fp, got = budget_dev(pays)
    assert np.array_equal(fp, [_oracle.txn_parse(p)[0] for p in pays])
    same_records(got, pays)                     # every entry written: none is FILL


def test_1_budget_dev_max_size_payload():
    big = dict(B.big_cases())["max_size"]
    pays = [dict(B.cases())["none_1"], big, dict(B.cases())["kind_price"]]
    fp, got = budget_dev(pays)
    assert fp[1] == 20 + 10 * 21775
    same_records(got, pays)
    assert tuple(int(x) for x in got[1].tolist()) == (4355, 59832704, 0, B.F_FEE, 1, B.OK)


def test_1_budget_dev_footprint_plane():
    """A footprint of 0 is _NOPARSE whatever the payload holds; a payload cut
    short under a footprint that claims it parsed ends in _NOPARSE too (the
    cursor's bound fails), at every length."""
    pays = [p for _, p in B.cases()][:70]
    _, got = budget_dev(pays, fp_force=np.zeros(len(pays), np.uint32))
    assert all(tuple(int(x) for x in r.tolist()) == (0, 0, 0, 0, 0, B.NOPARSE) for r in got)
    whole = dict(B.cases())["align_1"]
    cuts = [whole[:k] for k in range(len(whole))] + [whole]
    _, got = budget_dev(cuts, fp_force=np.full(len(cuts), 50, np.uint32))
    assert (got["status"][:-1] == B.NOPARSE).all() and not got[:-1]["rewards"].any() and not got[:-1]["compute"].any()
    assert tuple(int(x) for x in got[-1].tolist()) == want(whole) and want(whole)[5] == B.OK


# ---- 2. the engine calls ------------------------------------------------------------------------

class Arena:
    """Page-aligned host memory in one registration; put() lays a byte string
    at the next 16-aligned slot + align."""

    def __init__(self, nbytes):
        from firedancer_amd import ed25519
        nbytes = (nbytes + PAGE - 1) & ~(PAGE - 1)
        self._raw = np.full(nbytes + 2 * PAGE, FILL, np.uint8)
        o = (-self._raw.ctypes.data) % PAGE
        self.mem = self._raw[o:o + nbytes]
        self.pos = 0
        ed25519.host_register(self.mem)

    def put(self, data, align):
        d = np.frombuffer(bytes(data), np.uint8)
        o = ((self.pos + 15) & ~15) + 16 + align
        assert o + d.size <= self.mem.size
        self.mem[o:o + d.size] = d
        self.pos = o + d.size
        return int(self.mem.ctypes.data) + o

    def close(self):
        from firedancer_amd import ed25519
        ed25519.host_unregister(self.mem)


class Batch:
    """About 200 transactions: the corpus (signatures that do not verify),
    validly signed 1..2-signer transactions, the corpus again backwards and
    some of the signed ones a second time (duplicates for the filter)."""

    def __init__(self):
        signed, _ = _txn.build_txns(7301, 20, nsig_lo=1, nsig_hi=2, msg_lo=64, msg_hi=300)
        corpus = [p for _, p in B.cases()]
        self.pays = corpus + signed + corpus[::-1] + signed[:10]
        self.n = len(self.pays)
        self.blob, self.off, self.sz32 = _txn.pack(self.pays)
        self.arena = Arena(sum(len(p) + 48 for p in self.pays))
        self.ptr = np.array([self.arena.put(p, t % 16) for t, p in enumerate(self.pays)], np.uint64)
        self.sz = self.sz32.astype(np.uint64)
        # one chunk of at most 64 signature slots: signed ones, corpus payloads (one slot each,
        # the last three do not parse), four of the signed ones again
        self.one = signed[:8] + corpus[:36] + corpus[-4:] + signed[:4]
        self.one_blob, self.one_off, self.one_sz32 = _txn.pack(self.one)
        self.one_ptr = np.array([self.arena_one(p, t) for t, p in enumerate(self.one)], np.uint64)
        self.one_sz = self.one_sz32.astype(np.uint64)

    def arena_one(self, p, t):
        if not hasattr(self, "arena1"):
            self.arena1 = Arena(sum(len(q) + 48 for q in self.one))
        return self.arena1.put(p, (t * 5) % 16)

    def close(self):
        self.arena.close()
        self.arena1.close()


@pytest.fixture(scope="module")
def tb():
    b = Batch()
    assert 190 <= b.n <= 260 and len(b.one) <= CAP
    yield b
    b.close()


@pytest.fixture(scope="module")
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ext():
    from firedancer_amd import ed25519
    nbytes = (2 * CAP * ed25519.txn_emit_bound(1232) + PAGE - 1) & ~(PAGE - 1)
    raw = np.zeros(nbytes + PAGE, np.uint8)
    o = (-raw.ctypes.data) % PAGE
    mem = raw[o:o + nbytes]
    ed25519.host_register(mem)
    yield mem
    ed25519.host_unregister(mem)


@pytest.fixture(autouse=True)
def _leave_the_engine_idle(request):
    yield
    if "eng" in request.fixturenames:
        from firedancer_amd import ed25519
        e = request.getfixturevalue("eng")
        while e.in_flight:
            e.wait()
        e.set_window(None)
        e.set_mode(ed25519.MODE_REFERENCE)


def _same(got, want_):
    assert len(got) == len(want_)
    for k, (a, b) in enumerate(zip(got, want_)):
        if isinstance(a, tuple):
            _same(a, b)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), (k, np.nonzero(a != b)[0][:6])


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_2_blocking_calls(eng, tb, mode, registered):
    """Four or more chunks of at most 64 transactions through every slot:
    budget is the host rule's for every transaction, every other output that
    of the _desc call, through Python's want_budget."""
    e, b = eng, tb
    e.set_mode(mode)
    kw = dict(want_sigs=True, want_tags=True, want_desc=True)
    if registered:
        plain = e.verify_txns_ptrs(b.ptr, b.sz, **kw)
        full = e.verify_txns_ptrs(b.ptr, b.sz, want_budget=True, **kw)
        bare = e.verify_txns_ptrs(b.ptr, b.sz, want_budget=True)
    else:
        plain = e.verify_txns(b.blob, b.off, b.sz32, **kw)
        full = e.verify_txns(b.blob, b.off, b.sz32, want_budget=True, **kw)
        bare = e.verify_txns(b.blob, b.off, b.sz32, want_budget=True)
    assert len(plain) == 7 and len(full) == 8 and len(bare) == 2
    _same(full[:7], plain)
    _same(bare[:1], plain[:1])
    same_records(full[7], b.pays, "full")
    same_records(bare[1], b.pays, "bare")
    terr = plain[0]
    assert np.array_equal(full[7]["status"] == B.NOPARSE, terr == ERR_PARSE)
    assert (terr == 0).sum() >= 30 and (terr == ERR_PARSE).sum() >= 6 and (full[7]["status"] == B.INVALID).sum() > 40


class RawBlocking:
    """One blocking call through C, every output prefilled."""

    def __init__(self, b, e, registered):
        from firedancer_amd import ed25519
        self.L, self.P, self.e, self.b, self.registered = ed25519.lib(), ed25519._ptr, e, b, registered
        n = b.n
        self.base, tot = ed25519.txn_slots(b.blob, b.off, b.sz32)
        self.terr, self.serr = np.full(n, 0x55, np.int8), np.full(tot, 0x55, np.int8)
        self.ttag, self.stag = np.full(n, 0x55, np.uint64), np.full(tot, 0x55, np.uint64)
        self.doff, self.desc = ed25519._desc_buffers(b.sz)
        self.desc[:] = 0x55
        self.budget = np.full(24 * n, 0x5A, np.uint8)

    def call(self, suffix, budget=False):
        P, b = self.P, self.b
        head = (P(b.ptr), P(b.sz)) if self.registered else (P(b.blob), P(b.off), P(b.sz32), int(b.blob.size))
        name = "fd_ed25519_amd_verify_txns" + ("_registered" if self.registered else "") + suffix
        tail = ((P(self.budget) if budget else None),) if suffix == "_budget" else ()
        return getattr(self.L, name)(self.e._h, b.n, *head, P(self.terr), P(self.base), P(self.serr), P(self.ttag), P(self.stag),
                                     P(self.doff), P(self.desc), int(self.desc.size), *tail)

    def outs(self):
        return (self.terr, self.base, self.serr, self.ttag, self.stag, self.doff, self.desc)


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
def test_2_budget_null_is_the_desc_call(eng, tb, registered):
    d, n, w = RawBlocking(tb, eng, registered), RawBlocking(tb, eng, registered), RawBlocking(tb, eng, registered)
    assert d.call("_desc") == OK and n.call("_budget", budget=False) == OK and w.call("_budget", budget=True) == OK
    _same(n.outs(), d.outs())
    _same(w.outs(), d.outs())
    assert (n.budget == 0x5A).all()
    same_records(w.budget.view(_dt()), tb.pays)


def _submit(e, b, registered, **kw):
    if registered:
        return e.submit_txns_ptrs(b.one_ptr, b.one_sz, **kw)
    return e.submit_txns(b.one_blob, b.one_off, b.one_sz32, **kw)


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
def test_3_submissions_keep_window_emit_and_budget(eng, tb, ext, registered):
    """keep, a window, emit and budget in one call: records for all the
    transactions, survivors or not; every other output, the extent included,
    byte for byte that of the same submission without budget (each on a fresh
    window); two in flight behind one another."""
    from firedancer_amd import ed25519
    e, b = eng, tb
    n = len(b.one)
    cap = sum(ed25519.txn_emit_bound(len(p)) for p in b.one)
    half = ext.size // 2
    kw = dict(want_sigs=True, want_tags=True, want_desc=True, want_keep=True)
    outs = []
    for k, budget in enumerate((False, True)):
        win = ed25519.Window(0, 4 * CAP)
        e.set_window(win)
        try:
            ext[:] = 0xC3
            t0 = _submit(e, b, registered, emit=ext[:cap], want_budget=budget, **kw)
            t1 = _submit(e, b, registered, emit=ext[half:half + cap], want_budget=budget, **kw)    # all duplicates of the first
            assert e.in_flight == 2 and t1 == t0 + 1
            (r0, a), (r1, c) = e.wait(), e.wait()
            assert (r0, r1) == (t0, t1)
            outs.append((a, c, ext.copy()))
        finally:
            e.set_window(None)
            win.close()
    (a0, c0, x0), (a1, c1, x1) = outs
    assert len(a1) == len(a0) + 1 and len(c1) == len(c0) + 1
    _same(a1[:-1], a0)
    _same(c1[:-1], c0)
    assert np.array_equal(x0, x1)
    keep, keep2 = a1[-3], c1[-3]
    assert 0 < keep.size < n and keep2.size == 0               # the window saw them all
    same_records(a1[-1], b.one, "first")
    same_records(c1[-1], b.one, "second")
    assert (a1[-1]["status"][[i for i in range(n) if i not in set(keep.tolist())]] != B.NOPARSE).any()


class RawSubmit:
    """One submission through a C _budget call: verdicts and budget only,
    both prefilled."""

    def __init__(self, b, e, registered, n=None):
        from firedancer_amd import ed25519
        self.L, self.P, self.e, self.b, self.registered = ed25519.lib(), ed25519._ptr, e, b, registered
        self.n = len(b.one) if n is None else n
        self.terr = np.full(len(b.one), 0x55, np.int8)
        self.budget = np.full(24 * len(b.one), 0x5A, np.uint8)
        self.ticket = ctypes.c_ulong(99)

    def submit(self, keep=None, kcnt=None):
        P, b = self.P, self.b
        head = (P(b.one_ptr), P(b.one_sz)) if self.registered else (P(b.one_blob), P(b.one_off), P(b.one_sz32), int(b.one_blob.size))
        name = "fd_ed25519_amd_submit_txns" + ("_registered" if self.registered else "") + "_budget"
        return getattr(self.L, name)(self.e._h, self.n, *head, P(self.terr), None, None, None, None, None, None, 0,
                                     keep, kcnt, None, 0, None, None, P(self.budget), ctypes.byref(self.ticket))

    def untouched(self):
        return bool((self.terr == 0x55).all() and (self.budget == 0x5A).all())


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
def test_3_budget_is_written_at_delivery_only(eng, tb, registered):
    """After submit and before the reporting poll budget still holds its
    sentinel; ERR_INVAL and BUSY returns leave it untouched."""
    e, b = eng, tb
    r = RawSubmit(b, e, registered)
    assert r.submit() == OK and e.in_flight == 1
    from firedancer_amd import hip
    hip.synchronize()                                          # the GPU is done; nothing was delivered yet
    assert r.untouched()
    t, _ = e.wait()
    assert t == r.ticket.value and not (r.terr == 0x55).any()
    same_records(r.budget.view(_dt()), b.one)
    # refused arguments: no transactions, keep without keep_cnt
    z = RawSubmit(b, e, registered, n=0)
    assert z.submit() == INVAL and z.untouched() and z.ticket.value == 99
    k = RawSubmit(b, e, registered)
    kbuf = np.zeros(len(b.one), np.uint32)
    assert k.submit(keep=ctypes.c_void_p(kbuf.ctypes.data)) == INVAL and k.untouched() and e.in_flight == 0
    # every slot taken: BUSY
    held = [RawSubmit(b, e, registered) for _ in range(SLOTS)]
    assert all(h.submit() == OK for h in held) and e.in_flight == SLOTS
    x = RawSubmit(b, e, registered)
    assert x.submit() == BUSY and x.untouched() and x.ticket.value == 99
    for h in held:
        e.wait()
        same_records(h.budget.view(_dt()), b.one)
    assert x.untouched()
