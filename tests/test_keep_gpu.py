"""GPU: a batch's survivors -- the in-batch dedup and verdict filter
(include/fd_ed25519_amd.h, "Survivors"; firedancer_amd/csrc/fd_ed25519_keep.h).

a / b  fd_ed25519_amd_keep_dev on synthetic (err, tag) arrays, no signatures
       involved: every case against the host reference keep(), under two
       salts, with the scratch prefilled with 0xFF and with the leftovers of
       a larger n, and guard regions around every buffer.
c / d  the four _keep submit forms, both verdict modes, staged and
       registered, on batches built from the async tests' signature and
       transaction fixtures: keep equals keep( err, tag ) over the outputs of
       the plain submit for the same arguments, every other output is byte for
       byte that call's; descriptors step exactly at the survivors.
e      the contract: argument errors, delivery, ticket order, event poll.
All comparisons are exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the event-poll child
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import _golden
import _txn
from _keep import CASES, random_case, rule
from test_async_gpu import Arena, Sigs, Txns

pytestmark = pytest.mark.gpu

OK, INVAL = 0, -10
CAP, SLOTS, BLOB = 256, 4, 256 * 1232
SALTS = (0, 0x9E3779B97F4A7C15)
S8, S32, S64 = 0x55, 0x55555555, 0x5555555555555555


# ---- a / b. keep_dev ---------------------------------------------------------------------------------

def _dev_cases():
    c = dict(CASES)
    for n in (1, 63, 64, 65, 4096, 4097, 4161):       # 4161: the one-workgroup scan's second turn, and odd
        c["random_n%d" % n] = random_case(n, n, max(2, n // 4))
    one = np.zeros(1 << 16, np.int8)
    one[:3] = -3                                       # three failing copies ahead of the chain's first passing item
    c["one_chain_65536"] = (one, np.full(1 << 16, 0xC0FFEE0000000001, np.uint64))
    c["top16_bits_65536"] = (np.zeros(1 << 16, np.int8), (np.arange(1 << 16, dtype=np.uint64) << np.uint64(48)) | np.uint64(1))
    return c


DEV_CASES = _dev_cases()


def _keep_dev(err, tag, salt, scratch_fill):
    """One guarded fd_ed25519_amd_keep_dev call: (keep[:cnt], the scratch as
    the call left it).  scratch_fill: a byte, or a byte image at least as long
    as the scratch whose front is used."""
    from firedancer_amd import ed25519, hip
    from _wsguard import Guarded
    n = int(err.size)
    fp = ed25519.keep_scratch_footprint(n)
    assert fp % 256 == 0 and fp >= 12 * 2 * n
    fill = np.full(fp, scratch_fill, np.uint8) if np.isscalar(scratch_fill) else scratch_fill[:fp]
    d_err, d_tag = Guarded(n, err), Guarded(8 * n, tag)
    d_keep, d_cnt, d_scr = Guarded(4 * n, np.full(n, S32, np.uint32)), Guarded(8, np.full(1, S64, np.uint64)), Guarded(fp, fill)
    try:
        ed25519.keep_dev(n, d_err.ptr, d_tag.ptr, d_keep.ptr, d_cnt.ptr, d_scr.ptr, salt=salt)
        hip.synchronize()
        cnt = int(d_cnt.body(np.uint64)[0])
        assert cnt <= n
        keep = d_keep.body(np.uint32)
        assert (keep[cnt:] == S32).all()               # nothing at or beyond d_keep[keep_cnt]
        for g, what in ((d_err, "d_err"), (d_tag, "d_tag"), (d_keep, "d_keep"), (d_cnt, "d_keep_cnt"), (d_scr, "d_scratch")):
            g.check(what)
        assert np.array_equal(d_err.body(np.int8), err) and np.array_equal(d_tag.body(np.uint64), tag)   # only read
        return keep[:cnt].copy(), d_scr.body()
    finally:
        for g in (d_err, d_tag, d_keep, d_cnt, d_scr):
            g.free()


@pytest.fixture(scope="module")
def leftovers():
    """The scratch a call over 2^16 + 77 random items leaves: the leftovers of
    a larger n for every case."""
    err, tag = random_case(99, (1 << 16) + 77, 1 << 12)
    keep, scr = _keep_dev(err, tag, SALTS[1], 0x00)
    from firedancer_amd import ed25519
    assert np.array_equal(keep, ed25519.keep(err, tag))
    return scr


@pytest.mark.parametrize("name", sorted(DEV_CASES))
def test_ab_keep_dev(name, leftovers):
    from firedancer_amd import ed25519
    err, tag = DEV_CASES[name]
    want = ed25519.keep(err, tag)
    if err.size <= 4161:
        assert np.array_equal(want, rule(err, tag))
    for salt, fill in ((SALTS[0], 0xFF), (SALTS[1], leftovers)):
        got, _ = _keep_dev(err, tag, salt, fill)
        assert got.size == want.size and np.array_equal(got, want), (name, hex(salt), got[:8], want[:8])


def test_ab_the_long_cases_are_what_they_say():
    from firedancer_amd import ed25519
    assert ed25519.keep(*DEV_CASES["one_chain_65536"]).tolist() == [3]
    assert ed25519.keep(*DEV_CASES["top16_bits_65536"]).size == 1 << 16


def test_b_n0_writes_the_count_only():
    """n == 0: *d_keep_cnt = 0 and nothing else, with every other pointer NULL
    and with real ones."""
    from firedancer_amd import ed25519, hip
    from _wsguard import Guarded
    cnt = Guarded(8, np.full(1, S64, np.uint64))
    scr = Guarded(ed25519.keep_scratch_footprint(0), np.full(ed25519.keep_scratch_footprint(0), 0xFF, np.uint8))
    try:
        ed25519.keep_dev(0, None, None, None, cnt.ptr, None)
        hip.synchronize()
        assert int(cnt.body(np.uint64)[0]) == 0
        cnt.fill(np.full(1, S64, np.uint64))
        ed25519.keep_dev(0, None, None, None, cnt.ptr, scr.ptr, salt=SALTS[1])
        hip.synchronize()
        assert int(cnt.body(np.uint64)[0]) == 0 and (scr.body() == 0xFF).all()
        cnt.check("d_keep_cnt"), scr.check("d_scratch")
        with pytest.raises(ed25519.EngineError, match="rc=-10"):          # no count pointer; an n beyond the table's range
            ed25519.keep_dev(0, None, None, None, None, None)
        assert ed25519.keep_scratch_footprint((1 << 30) + 1) == 0
    finally:
        cnt.free(), scr.free()


# ---- c / d / e. the submit forms -----------------------------------------------------------------------

class SigBatch:
    """256 signatures from the async tests' fixture: a copy of a valid one with
    the low bit of s changed (verdict -3, the same tag), the valid original,
    the valid original again, an s-window signature, then the rest of the
    fixture (the signature family has no payload to parse)."""

    def __init__(self, s):
        v = int(np.nonzero((s.expect == 0) & (s.cls == _golden.CLASSES.index("valid")))[0][0])
        bad = bytearray(s.sigs[v])
        bad[32] ^= 1
        rest = [k for k in range(s.n) if k not in (v, s.swin)][:CAP - 4]
        order = [v, v, v, s.swin] + rest
        self.msgs = [s.msgs[k] for k in order]
        self.sigs = [bytes(bad)] + [s.sigs[k] for k in order[1:]]
        self.pubs = [s.pubs[k] for k in order]
        self.sz = s.sz[order].copy()
        self.arena = Arena(64 + 4096)
        self.pp, self.mp = s.pp[order].copy(), s.mp[order].copy()
        self.sp = s.sp[order].copy()
        self.sp[0] = self.arena.put(bytes(bad))
        self.n = len(order)
        assert self.n == CAP

    def submit(self, e, n, registered, **kw):
        if registered:
            return e.submit_batch_ptrs(self.pp[:n], self.sp[:n], self.mp[:n], self.sz[:n], **kw)
        return e.submit_batch(self.msgs[:n], self.sigs[:n], self.pubs[:n], **kw)


class TxnBatch:
    """Transactions from the async tests' fixture, one chunk of the engine at
    the most: a copy of a valid one-signer transaction with the low bit of its
    signature's s changed (verdict -3, the same tag), the original, the
    original again, a one-signer transaction carrying an s-window signature,
    a payload that does not parse, then the fixture's other transactions (one
    to four signers) and fresh one-signer ones up to the chunk's limits."""

    def __init__(self, x):
        from firedancer_amd import ed25519
        g = _golden.load_vectors()
        ones = [p for p in x.pays[5:] if p[0] == 1]
        v, host = ones[0], bytearray(ones[1])
        bad = bytearray(v)
        bad[1 + 32] ^= 1
        host[1:65] = bytes(g.sig[int(np.nonzero(g.cls == _golden.CLASSES.index("s_window"))[0][0])])
        fresh, _ = _txn.build_txns(77, CAP, nsig_lo=1, nsig_hi=1, msg_lo=64, msg_hi=400)
        pays = [bytes(bad), v, v, bytes(host), x.pays[1]] + [p for p in x.pays[:1] + x.pays[2:] if p not in (v, ones[1])]
        pays = pays[:70] + fresh
        blob, off, sz = _txn.pack(pays)
        base, _ = ed25519.txn_slots(blob, off, sz)
        self.full = int(min(CAP, np.searchsorted(base, CAP, side="right") - 1))   # transactions and slots within batch_max
        assert self.full > 100 and (self.full == CAP or int(base[self.full + 1]) > CAP)
        self.pays = pays[:self.full]
        self.blob, self.off, self.sz32 = _txn.pack(self.pays)
        self.arena = Arena(sum(len(p) + 32 for p in self.pays) + 8192)
        self.ptr = np.array([self.arena.put(p) for p in self.pays], np.uint64)
        self.sz = np.array([len(p) for p in self.pays], np.uint64)

    def submit(self, e, n, registered, **kw):
        if registered:
            return e.submit_txns_ptrs(self.ptr[:n], self.sz[:n], **kw)
        return e.submit_txns(self.blob, self.off[:n], self.sz32[:n], **kw)


@pytest.fixture(scope="module")
def sb():
    s = Sigs()
    b = SigBatch(s)
    yield b
    b.arena.close()
    s.arena.close()


@pytest.fixture(scope="module")
def tb():
    x = Txns()
    b = TxnBatch(x)
    yield b
    b.arena.close()
    x.arena.close()


@pytest.fixture(scope="module")
def keng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _leave_the_engine_idle(request):
    yield
    if "keng" in request.fixturenames:
        from firedancer_amd import ed25519
        e = request.getfixturevalue("keng")
        while e.in_flight:
            e.wait()
        e.set_mode(ed25519.MODE_REFERENCE)


def _same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), (k, np.nonzero(a != b)[0][:6])


def _sig_forms(e, b, mode, registered):
    """1, 65 and 256 signatures, plain and _keep submissions interleaved on one
    engine: tickets in order, (err, tag) equal, keep = keep( err, tag )."""
    from firedancer_amd import ed25519
    e.set_mode(mode)
    for n in (1, 65, b.n):
        t0 = b.submit(e, n, registered, want_tags=True)
        t1 = b.submit(e, n, registered, want_tags=True, want_keep=True)
        t2 = b.submit(e, n, registered, want_keep=True)              # the tags are made on the device all the same
        assert (t1, t2) == (t0 + 1, t0 + 2)
        (r0, plain), (r1, full), (r2, bare) = e.wait(), e.wait(), e.wait()
        assert (r0, r1, r2) == (t0, t1, t2)
        err, tag = plain
        _same(full[:2], plain)
        _same(bare[:1], plain[:1])
        want = ed25519.keep(err, tag)
        assert np.array_equal(want, rule(err, tag))
        for got in (full[2], bare[1]):
            assert got.dtype == np.uint32 and np.array_equal(got, want), (n, got[:8], want[:8])
        # the batch is what its docstring says
        assert int(err[0]) == -3
        if n == 1:
            assert want.size == 0
        else:
            assert int(err[1]) == 0 and int(err[2]) == 0 and tag[0] == tag[1] == tag[2] != 0
            assert 1 in want and 0 not in want and 2 not in want
            assert int(err[3]) == (0 if mode == ed25519.MODE_REFERENCE else -1) and tag[3] != 0
            assert (3 in want) == (mode == ed25519.MODE_REFERENCE)
            assert want.size < int((err == 0).sum())


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_c_signature_forms(keng, sb, mode, registered):
    _sig_forms(keng, sb, mode, registered)


def _desc_of(doff, desc, t):
    return desc[int(doff[t]):int(doff[t + 1])]


def _txn_forms(e, b, mode, registered):
    """1, 65 and a full chunk of transactions with every optional output."""
    from firedancer_amd import ed25519
    e.set_mode(mode)
    kw = dict(want_sigs=True, want_tags=True, want_desc=True)
    for n in (1, 65, b.full):
        t0 = b.submit(e, n, registered, **kw)
        t1 = b.submit(e, n, registered, want_keep=True, **kw)
        t2 = b.submit(e, n, registered, want_keep=True)              # no other optional output
        assert (t1, t2) == (t0 + 1, t0 + 2)
        (r0, plain), (r1, full), (r2, bare) = e.wait(), e.wait(), e.wait()
        assert (r0, r1, r2) == (t0, t1, t2)
        terr, base, serr, ttag, stag, doff, desc = plain
        _same(full[:5], plain[:5])                                   # txn_err, sig_base, sig_err, txn_tag, sig_tag: unchanged
        _same(bare[:1], plain[:1])
        want = ed25519.keep(terr, ttag)
        assert np.array_equal(want, rule(terr, ttag))
        for got in (full[7], bare[1]):
            assert got.dtype == np.uint32 and np.array_equal(got, want), (n, got[:8], want[:8])
        # d. descriptors for the survivors only: desc_off steps exactly there, the bytes are the unfiltered call's
        koff, kdesc = full[5], full[6]
        assert koff.shape == doff.shape and int(koff[0]) == 0
        step = np.diff(koff.astype(np.int64))
        surv = np.zeros(n, bool)
        surv[want] = True
        assert np.array_equal(step != 0, surv)
        assert kdesc.size == int(koff[n]) == sum(_desc_of(doff, desc, t).size for t in want)
        for t in want:
            a, c = _desc_of(koff, kdesc, t), _desc_of(doff, desc, t)
            assert a.size == c.size and c.size > 0 and np.array_equal(a, c), t
        # the batch is what its docstring says
        assert int(terr[0]) == -3
        if n > 1:
            assert terr[1] == 0 and terr[2] == 0 and ttag[0] == ttag[1] == ttag[2] != 0
            assert int(terr[3]) == (0 if mode == ed25519.MODE_REFERENCE else -1) and ttag[3] != 0
            assert int(terr[4]) == ed25519.FD_TXN_AMD_ERR_PARSE and ttag[4] == 0
            assert want[:1].tolist() == [1] and (3 in want) == (mode == ed25519.MODE_REFERENCE) and 4 not in want
            assert int(base[6] - base[5]) == 4                      # a four-signer transaction among them


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_cd_transaction_forms(keng, tb, mode, registered):
    _txn_forms(keng, tb, mode, registered)


class Raw:
    """One registered signature submission through the C _keep call, its
    outputs prefilled with 0x55."""

    def __init__(self, b, n, h):
        from firedancer_amd import ed25519
        self.n, self.h, self.L, self.P = n, h, ed25519.lib(), ed25519._ptr
        self.err, self.tag = np.full(n, S8, np.int8), np.full(n, S64, np.uint64)
        self.keep, self.cnt = np.full(n, S32, np.uint32), np.full(1, S64, np.uint64)
        self._in = [a[:n].copy() for a in (b.mp, b.sz, b.sp, b.pp)]
        self.ticket = ctypes.c_ulong(99)

    def submit(self, keep=True, cnt=True, name="fd_ed25519_amd_submit_batch_registered_keep"):
        return getattr(self.L, name)(self.h, self.n, *(self.P(a) for a in self._in), self.P(self.err), self.P(self.tag),
                                     self.P(self.keep) if keep else None, self.P(self.cnt) if cnt else None,
                                     ctypes.byref(self.ticket))

    def untouched(self):
        return bool((self.err == S8).all() and (self.tag == S64).all() and (self.keep == S32).all() and (self.cnt == S64).all())


def _wait(e):
    from firedancer_amd import ed25519
    t = ctypes.c_ulong(0)
    return ed25519.lib().fd_ed25519_amd_async_wait(e._h, ctypes.byref(t)), int(t.value)


def test_e_one_pointer_without_the_other_is_refused(keng, sb, tb):
    from firedancer_amd import ed25519
    L, P = ed25519.lib(), ed25519._ptr
    for kw in (dict(keep=True, cnt=False), dict(keep=False, cnt=True)):
        for name in ("fd_ed25519_amd_submit_batch_registered_keep", "fd_ed25519_amd_submit_batch_keep"):
            r = Raw(sb, 65, keng._h)
            assert r.submit(name=name, **kw) == INVAL
            assert r.untouched() and r.ticket.value == 99 and keng.in_flight == 0
    # the transaction forms
    n = 5
    terr, keep, cnt, t = np.full(n, S8, np.int8), np.full(n, S32, np.uint32), np.full(1, S64, np.uint64), ctypes.c_ulong(99)
    ptr, sz, off, sz32 = tb.ptr[:n].copy(), tb.sz[:n].copy(), tb.off[:n].copy(), tb.sz32[:n].copy()
    for k, c in ((P(keep), None), (None, P(cnt))):
        rc = L.fd_ed25519_amd_submit_txns_registered_keep(keng._h, n, P(ptr), P(sz), P(terr), None, None,
                                                          None, None, None, None, 0, k, c, ctypes.byref(t))
        assert rc == INVAL
        rc = L.fd_ed25519_amd_submit_txns_keep(keng._h, n, P(tb.blob), P(off), P(sz32), int(tb.blob.size),
                                               P(terr), None, None, None, None, None, None, 0, k, c, ctypes.byref(t))
        assert rc == INVAL
    assert (terr == S8).all() and (keep == S32).all() and (cnt == S64).all() and t.value == 99 and keng.in_flight == 0


def test_e_delivery_and_order(keng, sb):
    """_keep and plain submissions interleaved: nothing is written before the
    wait that reports the ticket, both-NULL is the plain submit, and keep is
    untouched at and beyond keep_cnt."""
    from firedancer_amd import ed25519
    err, tag = keng.verify_batch_ptrs(sb.pp[:65], sb.sp[:65], sb.mp[:65], sb.sz[:65], want_tags=True)
    want = ed25519.keep(err, tag)
    assert 0 < want.size < 65
    a, b, c, d = (Raw(sb, 65, keng._h) for _ in range(4))
    assert a.submit() == OK
    assert b.submit(keep=False, cnt=False) == OK                                              # both NULL
    assert c.submit() == OK
    rc = d.L.fd_ed25519_amd_submit_batch_registered(d.h, d.n, *(d.P(x) for x in d._in), d.P(d.err), d.P(d.tag), ctypes.byref(d.ticket))
    assert rc == OK
    tk = [r.ticket.value for r in (a, b, c, d)]
    assert tk == list(range(tk[0], tk[0] + 4)) and keng.in_flight == 4
    assert all(r.untouched() for r in (a, b, c, d))
    for k, r in enumerate((a, b, c, d)):
        assert _wait(keng) == (OK, tk[k])
        assert np.array_equal(r.err, err) and np.array_equal(r.tag, tag)
        if r in (a, c):
            assert int(r.cnt[0]) == want.size and np.array_equal(r.keep[:want.size], want)
            assert (r.keep[want.size:] == S32).all()
        else:
            assert (r.keep == S32).all() and (r.cnt == S64).all()
        assert all(x.untouched() for x in (a, b, c, d)[k + 1:])
    assert keng.in_flight == 0


def test_e_event_poll_gives_the_same_results():
    """The submit forms in a fresh process whose engine polls with
    hipEventQuery (FD_ED25519_AMD_ASYNC_POLL=event, read at creation)."""
    env = dict(os.environ, FD_ED25519_AMD_ASYNC_POLL="event")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keep event poll: OK" in r.stdout, r.stdout + r.stderr


def _child():
    from firedancer_amd import ed25519
    assert os.environ.get("FD_ED25519_AMD_ASYNC_POLL") == "event"
    s, x = Sigs(), Txns()
    b, t = SigBatch(s), TxnBatch(x)
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    try:
        _sig_forms(e, b, ed25519.MODE_STRICT, True)
        _txn_forms(e, t, ed25519.MODE_REFERENCE, True)
        _sig_forms(e, b, ed25519.MODE_REFERENCE, False)
        _txn_forms(e, t, ed25519.MODE_STRICT, False)
    finally:
        e.close()
        for a in (b.arena, t.arena, s.arena, x.arena):
            a.close()
    print("keep event poll: OK")


if __name__ == "__main__":
    _child()
