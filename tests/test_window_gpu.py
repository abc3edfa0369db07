"""GPU: dedup across submissions -- the device-resident tag window
(include/fd_ed25519_amd.h, "The dedup window";
firedancer_amd/csrc/fd_ed25519_window.h).

a / b  fd_ed25519_amd_window_keep_dev on synthetic (err, tag) streams, no
       signatures involved: after EVERY call the keep list and the exported
       window equal the host window's (ring order and eviction, exactly),
       under two salts, the scratch prefilled with 0xFF, guard regions around
       every buffer.
c / d  the four _keep submit forms with a window attached, both verdict
       modes, staged and registered: the same batch four times back to back
       before any wait (the cross-stream order), then 1, 65 and a full chunk
       with plain submissions in between, a fresh batch that evicts and the
       first batch again; descriptors step exactly at the window's survivors.
e      the contract: set_window's refusals, detaching, delivery.
The reference is the host window (test_window_cpu.py holds it to the rule).
All comparisons are exact."""
import numpy as np
import pytest

import _txn
from _window import _arr, random_stream, tag_of
from test_window_cpu import SHAPES
from test_keep_gpu import Raw, SigBatch, TxnBatch, _desc_of, _same, _wait, sb, tb  # noqa: F401  (sb, tb: fixtures)
from test_async_gpu import Arena

pytestmark = pytest.mark.gpu

OK, INVAL = 0, -10
CAP, SLOTS, BLOB = 256, 4, 256 * 1232
SALTS = (1, 0x9E3779B97F4A7C15)
S32, S64 = 0x55555555, 0x5555555555555555
CALLS_MAX = 1000                                   # per stream: a call costs a dozen small copies


# ---- a / b. window_keep_dev --------------------------------------------------------------------------

class DevWindow:
    """A device window and a host window fed the same submissions through
    guarded buffers that are allocated once, for nmax items."""

    def __init__(self, depth, salt, nmax):
        from firedancer_amd import ed25519
        from _wsguard import Guarded
        self.ed, self.nmax = ed25519, nmax
        self.fp = ed25519.window_keep_scratch_footprint(nmax)
        assert self.fp % 256 == 0 and self.fp >= ed25519.keep_scratch_footprint(nmax) + 4 * nmax
        self.dev, self.host = ed25519.Window(0, depth, salt=salt), ed25519.Window(-1, depth)
        self.g = dict(err=Guarded(max(nmax, 1)), tag=Guarded(8 * max(nmax, 1)), keep=Guarded(4 * max(nmax, 1)),
                      cnt=Guarded(8), scr=Guarded(self.fp))

    def load(self, tags):
        self.dev.load(tags), self.host.load(tags)
        assert np.array_equal(self.dev.export(), np.asarray(tags, np.uint64))

    def call(self, err, tag, what=""):
        """One guarded call; the keep list, compared with the host window's, as is the state."""
        from firedancer_amd import hip
        g, n = self.g, int(err.size)
        g["err"].write(0, err), g["tag"].write(0, tag)
        g["keep"].fill(np.full(max(self.nmax, 1), S32, np.uint32)), g["cnt"].fill(np.full(1, S64, np.uint64))
        g["scr"].fill(np.full(self.fp, 0xFF, np.uint8))
        self.dev.keep_dev(n, g["err"].ptr, g["tag"].ptr, g["keep"].ptr, g["cnt"].ptr, g["scr"].ptr)
        hip.synchronize()
        cnt = int(g["cnt"].body(np.uint64)[0])
        assert cnt <= n, (what, cnt)
        keep = g["keep"].body(np.uint32)
        assert (keep[cnt:] == S32).all(), what                         # nothing at or beyond d_keep[keep_cnt]
        for k, x in g.items():
            x.check(k)
        assert np.array_equal(g["err"].body(np.int8, n), err) and np.array_equal(g["tag"].body(np.uint64, n), tag)   # only read
        if n < self.nmax:                                              # nothing beyond the footprint of this n
            assert (g["scr"].body()[self.ed.window_keep_scratch_footprint(n):] == 0xFF).all(), what
        want = self.host.keep(err, tag)
        assert np.array_equal(keep[:cnt], want), (what, keep[:8], want[:8])
        assert np.array_equal(self.dev.export(), self.host.export()), what
        return keep[:cnt].copy()

    def close(self):
        self.dev.close(), self.host.close()
        for x in self.g.values():
            x.free()


@pytest.mark.parametrize("depth,n", SHAPES)
def test_ab_streams(depth, n):
    """The CPU test's shapes.  A stream the call budget would not carry three
    times round the ring starts from a window loaded full, so every shape
    evicts; (64, 64) rebuilds the map ahead of every call."""
    calls = (12 * depth + n - 1) // n + 4
    full = [tag_of(k) for k in range(1 << 41, (1 << 41) + depth)] if calls > CALLS_MAX else []
    for salt in SALTS:
        w = DevWindow(depth, salt, n)
        try:
            if full:
                w.load(full)
            inserted = 0
            for k, (err, tag) in enumerate(random_stream(depth * 1000 + n + (salt & 1), depth, n, min(calls, CALLS_MAX), hist=full)):
                got = w.call(err, tag, (hex(salt), k))
                inserted += int((tag[got] != 0).sum())
            assert w.host.export().size == depth and inserted >= (1 if full else 3 * depth)   # full to begin with: every insert evicts
        finally:
            w.close()


def test_ab_long_probes():
    """Tags that differ only in their top 16 bits and one tag 4096 times over:
    chains a weak slot function would make quadratic; every call rebuilds."""
    D = 1 << 12
    one = np.zeros(D, np.int8)
    one[:3] = -3                                                       # three failing copies ahead of the first passing item
    chain = np.full(D, 0xC0FFEE0000000001, np.uint64)
    top = [(np.arange(1 + j * D, 1 + (j + 1) * D, dtype=np.uint64) << np.uint64(48)) | np.uint64(1) for j in range(2)]
    ok = np.zeros(D, np.int8)
    for salt in SALTS:
        w = DevWindow(D, salt, D)
        try:
            assert w.call(one, chain).tolist() == [3]
            assert w.call(one, chain).size == 0
            assert w.call(ok, top[0]).size == D                        # evicts the chain's tag with all the rest
            assert w.call(ok, top[0]).size == 0
            assert w.call(ok, top[1]).size == D
            assert w.call(ok, top[0]).size == D                        # expired, admitted again
            assert w.call(one, chain).tolist() == [3]
        finally:
            w.close()


def test_b_n0_writes_the_count_only():
    from firedancer_amd import ed25519, hip
    from _wsguard import Guarded
    w = DevWindow(8, SALTS[0], 8)
    cnt = Guarded(8, np.full(1, S64, np.uint64))
    try:
        w.call(*_arr([0, 0], [5, 6]))
        w.dev.keep_dev(0, None, None, None, cnt.ptr, None)
        hip.synchronize()
        assert int(cnt.body(np.uint64)[0]) == 0 and w.dev.export().tolist() == [5, 6]
        cnt.check("d_keep_cnt")
        assert w.call(*_arr([], [])).size == 0                         # with real pointers: the scratch stays 0xFF
        assert (w.g["scr"].body() == 0xFF).all()
        with pytest.raises(ed25519.EngineError, match="rc=-10"):
            w.dev.keep_dev(0, None, None, None, None, None)
        assert ed25519.window_keep_scratch_footprint((1 << 30) + 1) == 0
    finally:
        cnt.free(), w.close()


def test_b_import_a_full_window_then_one_call():
    D = 320
    full = [tag_of(k, "top16") for k in range(1, D + 1)]
    w = DevWindow(D, SALTS[1], 65)
    try:
        w.load(full)
        tag = full[:20] + [tag_of(k) for k in range(1, 41)] + full[-5:]
        got = w.call(*_arr([0] * 65, tag))
        assert got.tolist() == list(range(20, 60))                     # 40 fresh ones push the 40 oldest out
        assert w.dev.export().tolist() == full[40:] + tag[20:60]
        assert w.call(*_arr([0] * 3, [full[0], full[39], full[40]])).tolist() == [0, 1]
        w.load([])
        assert w.dev.export().size == 0
    finally:
        w.close()


def test_b_refusals_enqueue_nothing():
    from firedancer_amd import ed25519
    w = DevWindow(8, SALTS[0], 9)
    try:
        w.call(*_arr([0, 0], [5, 6]))
        g = w.g
        for win, n in ((w.dev, 9), (w.host, 2)):                       # n > depth; a host-only window
            with pytest.raises(ed25519.EngineError, match="rc=-10"):
                win.keep_dev(n, g["err"].ptr, g["tag"].ptr, g["keep"].ptr, g["cnt"].ptr, g["scr"].ptr)
        with pytest.raises(ed25519.EngineError):
            w.dev.keep(*_arr([0], [7]))                                # the host rule is the host-only window's
        assert w.dev.export().tolist() == [5, 6]
        assert w.call(*_arr([0, 0], [6, 7])).tolist() == [1]
    finally:
        w.close()


# ---- c / d / e. the submit forms with a window ---------------------------------------------------------

@pytest.fixture(scope="module")
def weng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _leave_the_engine_idle(request):
    yield
    if "weng" in request.fixturenames:
        from firedancer_amd import ed25519
        e = request.getfixturevalue("weng")
        while e.in_flight:
            e.wait()
        e.set_window(None)
        e.set_mode(ed25519.MODE_REFERENCE)


def _fresh_sigs(seed, n):
    """n valid signatures nothing else in this file carries, with SigBatch's submit."""
    from firedancer_amd import ed25519
    rng = np.random.default_rng(seed)
    prv, blob = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, 64 * n, dtype=np.uint8)
    off, sz = np.arange(n, dtype=np.uint32) * 64, np.full(n, 64, np.uint32)
    pub, sig = ed25519.sign_batch(prv, blob, off, sz)
    b = SigBatch.__new__(SigBatch)
    b.msgs = [blob[64 * k:64 * k + 64].tobytes() for k in range(n)]
    b.sigs, b.pubs = [sig[k].tobytes() for k in range(n)], [pub[k].tobytes() for k in range(n)]
    b.sz, b.n, b.arena = np.full(n, 64, np.uint64), n, Arena(n * (64 + 64 + 32 + 48) + 4096)
    b.pp = np.array([b.arena.put(p) for p in b.pubs], np.uint64)
    b.sp = np.array([b.arena.put(s) for s in b.sigs], np.uint64)
    b.mp = np.array([b.arena.put(m) for m in b.msgs], np.uint64)
    return b


def _fresh_txns(seed, n):
    """n valid one-signer transactions nothing else in this file carries, with TxnBatch's submit."""
    pays, _ = _txn.build_txns(seed, n, nsig_lo=1, nsig_hi=1, msg_lo=64, msg_hi=300)
    b = TxnBatch.__new__(TxnBatch)
    b.pays, b.full = pays, n
    b.blob, b.off, b.sz32 = _txn.pack(pays)
    b.arena = Arena(sum(len(p) + 32 for p in pays) + 8192)
    b.ptr = np.array([b.arena.put(p) for p in pays], np.uint64)
    b.sz = np.array([len(p) for p in pays], np.uint64)
    return b


@pytest.fixture(scope="module")
def sb2():
    b = _fresh_sigs(4242, CAP)
    yield b
    b.arena.close()


@pytest.fixture(scope="module")
def tb2():
    b = _fresh_txns(4343, 200)
    yield b
    b.arena.close()


class Model:
    """The engine's window and the host window that says what it must deliver."""

    def __init__(self, e, depth):
        from firedancer_amd import ed25519
        self.e, self.dev, self.host = e, ed25519.Window(0, depth), ed25519.Window(-1, depth)
        e.set_window(self.dev)

    def want(self, err, tag):
        return self.host.keep(err, tag)

    def same_state(self):
        assert np.array_equal(self.dev.export(), self.host.export())

    def close(self):
        while self.e.in_flight:
            self.e.wait()
        self.e.set_window(None)
        self.dev.close(), self.host.close()


def _plain(e, b, n, registered, **kw):
    """The plain submit's outputs for the first n items: the byte-for-byte reference of every output but keep."""
    t = b.submit(e, n, registered, **kw)
    r, out = e.wait()
    assert r == t
    return out


def _sig_forms(e, b, b2, mode, registered, depth):
    from firedancer_amd import ed25519
    e.set_mode(mode)
    plain = _plain(e, b, b.n, registered, want_tags=True)
    err, tag = plain
    err2, tag2 = _plain(e, b2, b2.n, registered, want_tags=True)
    assert (err2 == 0).all() and np.unique(tag2).size == b2.n and not np.isin(tag2, tag).any()
    m = Model(e, depth)
    try:
        # the same batch four times back to back, before any wait: submissions act on the window in ticket order
        tk = [b.submit(e, b.n, registered, want_tags=True, want_keep=True) for _ in range(SLOTS)]
        first = None
        for k, t in enumerate(tk):
            r, out = e.wait()
            assert r == t
            _same(out[:2], plain)
            want = m.want(err, tag)
            assert out[2].dtype == np.uint32 and np.array_equal(out[2], want), (k, out[2][:8], want[:8])
            if k == 0:
                first = want
                assert np.array_equal(want, ed25519.keep(err, tag)) and want.size > 1     # an empty window: today's list
            else:
                assert np.array_equal(want, np.nonzero((err == 0) & (tag == 0))[0])       # the tag-0 passers alone
        m.same_state()
        # 1, 65 and the full batch, plain submissions in between: they change nothing
        for n in (1, 65, b.n):
            t0 = b.submit(e, n, registered, want_tags=True)
            t1 = b.submit(e, n, registered, want_keep=True)
            t2 = b.submit(e, n, registered)
            (r0, p0), (r1, k1), (r2, p2) = e.wait(), e.wait(), e.wait()
            assert (r0, r1, r2) == (t0, t1, t2)
            _same(p0, (err[:n], tag[:n]))
            _same((k1[0], p2 if isinstance(p2, np.ndarray) else p2[0]), (err[:n], err[:n]))
            assert np.array_equal(k1[1], m.want(err[:n], tag[:n]))
            m.same_state()
        # 256 fresh tags, then the first batch again: at depth 256 they pushed every tag of it out
        t = b2.submit(e, b2.n, registered, want_keep=True)
        r, out = e.wait()
        assert r == t and np.array_equal(out[1], m.want(err2, tag2)) and out[1].size == b2.n
        t = b.submit(e, b.n, registered, want_keep=True)
        r, out = e.wait()
        again = m.want(err, tag)
        assert r == t and np.array_equal(out[1], again)
        assert np.array_equal(again, first) if depth == CAP else again.size == 0          # evicted and admitted again, or still live
        m.same_state()
    finally:
        m.close()


@pytest.mark.parametrize("depth", [256, 1024])
@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_c_signature_forms(weng, sb, sb2, mode, registered, depth):
    _sig_forms(weng, sb, sb2, mode, registered, depth)


def _check_desc(full, plain, want, n):
    """d. descriptors for the window's survivors only: desc_off steps exactly there, the bytes are the unfiltered call's."""
    doff, desc, koff, kdesc = plain[5], plain[6], full[5], full[6]
    assert koff.shape == doff[:n + 1].shape and int(koff[0]) == 0
    surv = np.zeros(n, bool)
    surv[want] = True
    assert np.array_equal(np.diff(koff.astype(np.int64)) != 0, surv)
    assert kdesc.size == int(koff[n]) == sum(_desc_of(doff, desc, t).size for t in want)
    for t in want:
        a, c = _desc_of(koff, kdesc, t), _desc_of(doff, desc, t)
        assert a.size == c.size and c.size > 0 and np.array_equal(a, c), t


def _txn_forms(e, b, b2, mode, registered, depth):
    from firedancer_amd import ed25519
    e.set_mode(mode)
    kw = dict(want_sigs=True, want_tags=True, want_desc=True)
    plain = _plain(e, b, b.full, registered, **kw)
    terr, ttag = plain[0], plain[3]
    p2 = _plain(e, b2, b2.full, registered, **kw)
    assert (p2[0] == 0).all() and np.unique(p2[3]).size == b2.full and not np.isin(p2[3], ttag).any()
    m = Model(e, depth)
    try:
        tk = [b.submit(e, b.full, registered, want_keep=True, **kw) for _ in range(SLOTS)]
        first = None
        for k, t in enumerate(tk):
            r, out = e.wait()
            assert r == t
            _same(out[:5], plain[:5])                                  # txn_err, sig_base, sig_err, txn_tag, sig_tag: unchanged
            want = m.want(terr, ttag)
            assert out[7].dtype == np.uint32 and np.array_equal(out[7], want), (k, out[7][:8], want[:8])
            _check_desc(out, plain, want, b.full)
            if k == 0:
                first = want
                assert np.array_equal(want, ed25519.keep(terr, ttag)) and want.size > 100
            else:
                assert np.array_equal(want, np.nonzero((terr == 0) & (ttag == 0))[0])
        m.same_state()
        for n in (1, 65, b.full):
            ref = _plain(e, b, n, registered, **kw)
            t0 = b.submit(e, n, registered)
            t1 = b.submit(e, n, registered, want_keep=True, **kw)
            t2 = b.submit(e, n, registered, want_keep=True)            # no other optional output
            (r0, _), (r1, full), (r2, bare) = e.wait(), e.wait(), e.wait()
            assert (r0, r1, r2) == (t0, t1, t2)
            _same(full[:5], ref[:5])
            want = m.want(terr[:n], ttag[:n])
            assert np.array_equal(full[7], want)
            _check_desc(full, ref, want, n)
            assert np.array_equal(bare[1], m.want(terr[:n], ttag[:n]))
            m.same_state()
        t = b2.submit(e, b2.full, registered, want_keep=True, **kw)
        r, out = e.wait()
        want = m.want(p2[0], p2[3])
        assert r == t and np.array_equal(out[7], want) and want.size == b2.full
        _check_desc(out, p2, want, b2.full)
        t = b2.submit(e, 56, registered, want_keep=True)               # duplicates of the batch before
        r, out = e.wait()
        assert r == t and np.array_equal(out[1], m.want(p2[0][:56], p2[3][:56])) and out[1].size == 0
        t = b.submit(e, b.full, registered, want_keep=True, **kw)
        r, out = e.wait()
        again = m.want(terr, ttag)
        assert r == t and np.array_equal(out[7], again)
        _check_desc(out, plain, again, b.full)
        assert first.size + b2.full > CAP                               # so depth 256 has forgotten the first batch's oldest tag
        assert (again.size > 0 and again[0] == first[0]) if depth == CAP else again.size == 0
        m.same_state()
    finally:
        m.close()


@pytest.mark.parametrize("depth", [256, 1024])
@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_cd_transaction_forms(weng, tb, tb2, mode, registered, depth):
    _txn_forms(weng, tb, tb2, mode, registered, depth)


def test_c_signatures_and_transactions_share_the_window(weng, tb2):
    """A transaction's tag is its first signature's: the signature submitted on
    its own first makes the transaction a duplicate, and the other way round."""
    from firedancer_amd import ed25519
    e, n = weng, 8
    e.submit_txns(tb2.blob, tb2.off[:n], tb2.sz32[:n], want_tags=True)
    terr, ttag, _ = e.wait()[1]
    assert (terr == 0).all()
    sigs, msgs, pubs = [], [], []
    for k in (2, 5):                                                   # the one signer of a transaction, as a bare signature
        p = tb2.pays[k]
        at = next(a for a in (69, 70) if ed25519.tag(p[65:], p[1:65], p[a:a + 32]) == int(ttag[k]))
        sigs.append(p[1:65]), msgs.append(p[65:]), pubs.append(p[at:at + 32])
    m = Model(e, CAP)
    try:
        t = e.submit_batch(msgs[:1], sigs[:1], pubs[:1], want_tags=True, want_keep=True)
        r, (err, tag, keep) = e.wait()
        assert r == t and err.tolist() == [0] and int(tag[0]) == int(ttag[2])
        assert np.array_equal(keep, m.want(err, tag)) and keep.tolist() == [0]
        t = e.submit_txns(tb2.blob, tb2.off[:n], tb2.sz32[:n], want_keep=True)
        r, out = e.wait()
        assert r == t and np.array_equal(out[1], m.want(terr, ttag)) and out[1].tolist() == [0, 1, 3, 4, 5, 6, 7]
        t = e.submit_batch(msgs, sigs, pubs, want_keep=True)
        r, out = e.wait()
        assert r == t and out[1].size == 0 and m.want(np.zeros(2, np.int8), ttag[[2, 5]]).size == 0
        m.same_state()
    finally:
        m.close()


def test_e_set_window_refusals(weng, sb):
    from firedancer_amd import ed25519, hip
    e = weng
    L = ed25519.lib()
    small, host, win = ed25519.Window(0, CAP - 1), ed25519.Window(-1, CAP), ed25519.Window(0, CAP)
    other = ed25519.Engine(device=0, batch_max=16, nslot=2)
    far = ed25519.Window(1, CAP) if hip.device_count() > 1 else None
    hip.set_device(0)
    try:
        assert L.fd_ed25519_amd_window(e._h) is None
        for w in (small, host) + ((far,) if far else ()):              # depth < batch_max; not the engine's device
            assert L.fd_ed25519_amd_set_window(e._h, w._h) == INVAL and L.fd_ed25519_amd_window(e._h) is None
        t = sb.submit(e, 5, False)
        assert L.fd_ed25519_amd_set_window(e._h, win._h) == INVAL      # a submission in flight
        assert e.wait()[0] == t
        e.set_window(win)
        assert L.fd_ed25519_amd_window(e._h) == win._h
        e.set_window(win)                                              # again: fine
        assert L.fd_ed25519_amd_set_window(other._h, win._h) == INVAL  # attached to another engine
        t = sb.submit(e, 5, False)
        assert L.fd_ed25519_amd_set_window(e._h, None) == INVAL and L.fd_ed25519_amd_window(e._h) == win._h
        assert e.wait()[0] == t
        with pytest.raises(ed25519.EngineError, match="rc=-10"):       # an attached window is the engine's
            win.keep_dev(0, None, None, None, 8, None)
        e.set_window(None)
        other.set_window(win)                                          # free again
        other.set_window(None)
    finally:
        other.close()
        for w in (small, host, win, far):
            if w:
                w.close()
        hip.set_device(0)


def test_e_detaching_restores_todays_lists(weng, sb):
    from firedancer_amd import ed25519
    e = weng
    err, tag = _plain(e, sb, 65, True, want_tags=True)
    today = ed25519.keep(err, tag)
    m = Model(e, CAP)
    try:
        for want in (today, today[:0]):
            t = sb.submit(e, 65, True, want_keep=True)
            r, out = e.wait()
            assert r == t and np.array_equal(out[1], want) and np.array_equal(m.want(err, tag), want)
        e.set_window(None)
        for _ in range(2):
            t = sb.submit(e, 65, True, want_keep=True)
            r, out = e.wait()
            assert r == t and np.array_equal(out[1], today)
        assert np.array_equal(m.dev.export(), m.host.export())         # and the window was left alone
    finally:
        m.close()


def test_e_delivery(weng, sb):
    """With a window: nothing is written before the wait that reports the
    ticket, and keep is untouched at and beyond keep_cnt."""
    e = weng
    err, tag = _plain(e, sb, 65, True, want_tags=True)
    m = Model(e, CAP)
    try:
        a, b, c = (Raw(sb, 65, e._h) for _ in range(3))
        assert a.submit() == OK and b.submit(keep=False, cnt=False) == OK and c.submit() == OK
        tk = [r.ticket.value for r in (a, b, c)]
        assert tk == list(range(tk[0], tk[0] + 3)) and all(r.untouched() for r in (a, b, c))
        wants = [m.want(err, tag), None, m.want(err, tag)]
        assert wants[0].size > 0 and wants[2].size == 0
        for k, r in enumerate((a, b, c)):
            assert _wait(e) == (OK, tk[k])
            assert np.array_equal(r.err, err) and np.array_equal(r.tag, tag)
            if wants[k] is None:
                assert (r.keep == S32).all() and (r.cnt == S64).all()
            else:
                assert int(r.cnt[0]) == wants[k].size and np.array_equal(r.keep[:wants[k].size], wants[k])
                assert (r.keep[wants[k].size:] == S32).all()
            assert all(x.untouched() for x in (a, b, c)[k + 1:])
        m.same_state()
    finally:
        m.close()
