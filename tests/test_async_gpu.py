"""GPU: the asynchronous submit / poll / wait calls of the batch engine
(include/fd_ed25519_amd.h, "Asynchronous submissions").

One engine: 512 signatures per chunk, 4 slots, blob_max sized for 512 messages
of 200 bytes (padded to 16: 208).  Inputs are the committed golden vectors whose
message is at most 200 bytes, in a fixed shuffle, and the transaction fixtures
with synthetic multi-signer transactions; the expected outputs are the
synchronous calls' on the same inputs (and, in reference mode, the golden
codes).  All comparisons are exact.  Every wait on the device goes through
wait() or a polling loop with a deadline."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the event-poll child of test 9
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import _golden
import _txn

pytestmark = pytest.mark.gpu

CAP, SLOTS, BLOB = 512, 4, 512 * 208
OK, NONE, INVAL, BUSY = 0, 1, -10, -12
SIZES = (1, 64, 65, 300)
DEADLINE_S = 20.0
S8, S64 = 0x55, 0x5555555555555555


class Arena:
    """A page-aligned block of host memory in one host_register registration;
    put() lays a byte string at the next 16-aligned place and returns its
    address."""

    def __init__(self, nbytes):
        from firedancer_amd import ed25519
        nbytes = (nbytes + 4095) & ~4095
        self._raw = np.zeros(nbytes + 4096, np.uint8)
        o = (-self._raw.ctypes.data) % 4096
        self.mem = self._raw[o:o + nbytes]
        self.base, self.size, self.pos = int(self.mem.ctypes.data), nbytes, 0
        ed25519.host_register(self.mem)

    def put(self, data):
        d = np.frombuffer(bytes(data), np.uint8)
        o = (self.pos + 15) & ~15
        assert o + d.size <= self.size
        self.mem[o:o + d.size] = d
        self.pos = o + max(d.size, 1)
        return self.base + o

    def close(self):
        from firedancer_amd import ed25519
        ed25519.host_unregister(self.mem)


class Sigs:
    """300 golden vectors with messages of at most 200 bytes (every class that
    has such, in a fixed shuffle), as lists of bytes and as pointer arrays into
    a registered arena."""

    def __init__(self):
        g = _golden.load_vectors()
        idx = np.nonzero(g.msg_sz <= 200)[0]
        idx = idx[np.linspace(0, idx.size - 1, 300).astype(np.int64)]
        idx = idx[np.random.default_rng(7).permutation(idx.size)]
        self.n = int(idx.size)
        self.msgs = [g.msg(i) for i in idx]
        self.sigs = [bytes(g.sig[i]) for i in idx]
        self.pubs = [bytes(g.pub[i]) for i in idx]
        self.expect = g.expect[idx].copy()
        self.cls = g.cls[idx].copy()
        self.sz = np.array([len(m) for m in self.msgs], np.uint64)
        self.arena = Arena(self.n * (32 + 64 + 208 + 48) + 8192)
        self.pp = np.array([self.arena.put(p) for p in self.pubs], np.uint64)
        self.sp = np.array([self.arena.put(s) for s in self.sigs], np.uint64)
        self.mp = np.array([self.arena.put(m) for m in self.msgs], np.uint64)
        self.swin = int(np.nonzero(self.cls == _golden.CLASSES.index("s_window"))[0][0])


class Txns:
    """70 payloads: the three reference fixtures (the first has four signers),
    one that fails to parse, and synthetic transactions with 1..4 valid
    signers; packed, and as pointers into a registered arena."""

    def __init__(self):
        fx = [f.payload for f in _txn.load_fixtures()]
        syn, _ = _txn.build_txns(5, 66, nsig_lo=1, nsig_hi=4, msg_lo=64, msg_hi=400)
        self.pays = fx[:1] + [fx[1][:-1]] + fx[1:] + syn
        assert len(self.pays) == 70 and self.pays[0][0] == 4
        self.arena = Arena(sum(len(p) + 32 for p in self.pays) + 8192)
        self.ptr = np.array([self.arena.put(p) for p in self.pays], np.uint64)
        self.sz = np.array([len(p) for p in self.pays], np.uint64)


@pytest.fixture(scope="module")
def sigs():
    s = Sigs()
    yield s
    s.arena.close()


@pytest.fixture(scope="module")
def txns():
    t = Txns()
    yield t
    t.arena.close()


@pytest.fixture(scope="module")
def aeng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    assert e.async_depth == SLOTS and e.in_flight == 0
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _leave_the_engine_idle(request):
    """Whatever a test does, the shared engine ends it idle and in reference mode."""
    yield
    if "aeng" in request.fixturenames:
        from firedancer_amd import ed25519
        e = request.getfixturevalue("aeng")
        while e.in_flight:
            e.wait()
        e.set_mode(ed25519.MODE_REFERENCE)


def _poll_until(e):
    """poll() in a loop with a deadline: the delivered (ticket, outputs)."""
    end = time.monotonic() + DEADLINE_S
    while time.monotonic() < end:
        r = e.poll()
        if r is not None:
            return r
    pytest.fail("a submission was not delivered within %g s" % DEADLINE_S)


def _same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), (k, np.nonzero(a != b)[0][:6])


# ---- 1. equivalence ------------------------------------------------------------------

def _batch_equivalence(e, s, mode, registered):
    """n = 1, 64, 65 and 300 submitted back to back, the fifth refused, then
    collected by polling: (err, tag) equal the synchronous call's."""
    from firedancer_amd import ed25519
    e.set_mode(mode)
    want = {}
    for n in SIZES:
        if registered:
            want[n] = e.verify_batch_ptrs(s.pp[:n], s.sp[:n], s.mp[:n], s.sz[:n], want_tags=True)
        else:
            want[n] = e.verify_batch(s.msgs[:n], s.sigs[:n], s.pubs[:n], want_tags=True)
        if mode == ed25519.MODE_REFERENCE:
            assert np.array_equal(want[n][0], s.expect[:n])
    tickets = []
    for n in SIZES:
        if registered:
            tickets.append(e.submit_batch_ptrs(s.pp[:n], s.sp[:n], s.mp[:n], s.sz[:n], want_tags=True))
        else:
            tickets.append(e.submit_batch(s.msgs[:n], s.sigs[:n], s.pubs[:n], want_tags=True))
    assert tickets == list(range(tickets[0], tickets[0] + 4)) and e.in_flight == 4
    with pytest.raises(ed25519.EngineBusy):
        e.submit_batch_ptrs(s.pp[:1], s.sp[:1], s.mp[:1], s.sz[:1])
    for k, n in enumerate(SIZES):
        t, out = _poll_until(e)
        assert t == tickets[k]
        _same(out, want[n])
    assert e.in_flight == 0 and e.poll() is None
    if mode == ed25519.MODE_STRICT:     # the modes differ on these inputs: s-window signatures are 0 / -1
        w = s.cls[:300] == _golden.CLASSES.index("s_window")
        assert w.any() and (want[300][0][w] == -1).all() and (s.expect[:300][w] == 0).all()


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_1_batch_equivalence(aeng, sigs, mode, registered):
    _batch_equivalence(aeng, sigs, mode, registered)


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_1_txn_equivalence(aeng, txns, mode, registered):
    """1, 5 and 70 transactions (a four-signer one first, one that does not
    parse second) with every optional output: txn_err, sig_base, sig_err,
    txn_tag, sig_tag, desc_off and the descriptor bytes equal
    verify_txns_desc / verify_txns_registered_desc."""
    e, x = aeng, txns
    e.set_mode(mode)
    kw = dict(want_sigs=True, want_tags=True, want_desc=True)
    blob, off, sz = _txn.pack(x.pays)
    want, tickets = {}, []
    for n in (1, 5, 70):
        want[n] = e.verify_txns_ptrs(x.ptr[:n], x.sz[:n], **kw) if registered else e.verify_txns(blob, off[:n], sz[:n], **kw)
    assert want[5][0][1] == _txn_parse_err() and want[70][1][1] == 4          # the parse failure; four slots for the first
    for n in (1, 5, 70):
        if registered:
            tickets.append(e.submit_txns_ptrs(x.ptr[:n], x.sz[:n], **kw))
        else:
            tickets.append(e.submit_txns(blob, off[:n], sz[:n], **kw))
    assert e.in_flight == 3
    for k, n in enumerate((1, 5, 70)):
        t, out = _poll_until(e)
        assert t == tickets[k]
        assert int(out[5][0]) == 0                                            # offsets relative to the submission
        _same(out, want[n])
    # no optional output: the bare verdicts
    t = e.submit_txns_ptrs(x.ptr[:5], x.sz[:5]) if registered else e.submit_txns(blob, off[:5], sz[:5])
    got = e.wait()
    assert got[0] == t
    _same(got[1], want[5][0])


def _txn_parse_err():
    from firedancer_amd import ed25519
    return ed25519.FD_TXN_AMD_ERR_PARSE


# ---- raw calls with sentinel-filled outputs ---------------------------------------------

class Raw:
    """One registered pointer-array submission through the C call, its outputs
    prefilled with 0x55."""

    def __init__(self, s, n, h):
        from firedancer_amd import ed25519
        self.n, self.h, self.L, self.P = n, h, ed25519.lib(), ed25519._ptr
        self.err = np.full(n, S8, np.int8)
        self.tag = np.full(n, S64, np.uint64)
        self._in = [a[:n].copy() for a in (s.mp, s.sz, s.sp, s.pp)]
        self.args = tuple(self.P(a) for a in self._in)
        self.ticket = ctypes.c_ulong(0)

    def submit(self):
        return self.L.fd_ed25519_amd_submit_batch_registered(self.h, self.n, *self.args, self.P(self.err), self.P(self.tag),
                                                             ctypes.byref(self.ticket))

    def untouched(self):
        return bool((self.err == S8).all() and (self.tag == S64).all())


def _raw_collect(e, name):
    from firedancer_amd import ed25519
    t = ctypes.c_ulong(0)
    rc = getattr(ed25519.lib(), name)(e._h, ctypes.byref(t))
    return rc, int(t.value)


# ---- 2. order and isolation --------------------------------------------------------------

def test_2_order_and_isolation(aeng, sigs):
    """Two in flight: one wait reports the first ticket and fills its outputs,
    the second's still hold 0x55; the next wait reports the second; then poll
    and wait have nothing."""
    want = aeng.verify_batch_ptrs(sigs.pp[:300], sigs.sp[:300], sigs.mp[:300], sigs.sz[:300], want_tags=True)
    a, b = Raw(sigs, 64, aeng._h), Raw(sigs, 300, aeng._h)
    assert a.submit() == OK and b.submit() == OK
    assert b.ticket.value == a.ticket.value + 1 and aeng.in_flight == 2
    assert a.untouched() and b.untouched()
    assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (OK, a.ticket.value)
    assert np.array_equal(a.err, want[0][:64]) and np.array_equal(a.tag, want[1][:64])
    assert b.untouched()
    assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (OK, b.ticket.value)
    assert np.array_equal(b.err, want[0]) and np.array_equal(b.tag, want[1])
    assert _raw_collect(aeng, "fd_ed25519_amd_async_poll") == (NONE, 0)
    assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (NONE, 0)


# ---- 3. busy --------------------------------------------------------------------------------

def test_3_busy(aeng, sigs):
    """With 4 in flight the fifth submit is refused, touches nothing and
    consumes no ticket: the next accepted ticket follows the fourth."""
    four = [Raw(sigs, 65, aeng._h) for _ in range(4)]
    for r in four:
        assert r.submit() == OK
    fifth = Raw(sigs, 65, aeng._h)
    fifth.ticket.value = 99
    assert fifth.submit() == BUSY
    assert fifth.untouched() and fifth.ticket.value == 99 and aeng.in_flight == 4
    assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (OK, four[0].ticket.value)
    assert fifth.submit() == OK
    assert fifth.ticket.value == four[3].ticket.value + 1
    for r in four[1:] + [fifth]:
        assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (OK, r.ticket.value)
        assert np.array_equal(r.err, four[0].err)


# ---- 4. one chunk ----------------------------------------------------------------------------

def test_4_one_chunk(aeng, sigs):
    """More than one chunk, or nothing: ERR_INVAL before anything launches."""
    from firedancer_amd import ed25519
    L, P = ed25519.lib(), ed25519._ptr
    before = aeng.in_flight
    outs = []            # an accepted submission's outputs are written at delivery: they stay alive until then

    def raw(n, pp, sp, mp, sz, registered):
        err, tag, t = np.full(max(n, 1), S8, np.int8), np.full(max(n, 1), S64, np.uint64), ctypes.c_ulong(99)
        outs.append((err, tag))
        f = L.fd_ed25519_amd_submit_batch_registered if registered else L.fd_ed25519_amd_submit_batch
        rc = f(aeng._h, n, P(mp), P(sz), P(sp), P(pp), P(err), P(tag), ctypes.byref(t))
        assert (err == S8).all() and (tag == S64).all()          # a refusal touches nothing; an accepted one not yet
        assert (t.value == 99) == (rc != OK)
        return rc

    rep = np.arange(513) % sigs.n
    big = np.full(100, 1232, np.uint64)                       # 100 x 1232 bytes > blob_max; any registered bytes will do
    base = np.full(100, sigs.arena.base, np.uint64)
    for registered in (True, False):
        assert raw(513, sigs.pp[rep], sigs.sp[rep], sigs.mp[rep], sigs.sz[rep], registered) == INVAL
        assert raw(100, sigs.pp[:100], sigs.sp[:100], base, big, registered) == INVAL
        assert raw(0, sigs.pp[:1], sigs.sp[:1], sigs.mp[:1], sigs.sz[:1], registered) == INVAL
        assert raw(512, sigs.pp[rep[:512]], sigs.sp[rep[:512]], sigs.mp[rep[:512]], sigs.sz[rep[:512]], registered) == OK
        assert aeng.in_flight == before + 1
        assert _raw_collect(aeng, "fd_ed25519_amd_async_wait")[0] == OK
        assert np.array_equal(outs[-1][0], sigs.expect[rep[:512]])
    # padded bytes: 512 x 208 fits exactly, one more padded byte does not (the registered form pads to 16)
    sz = np.full(512, 193, np.uint64)
    mp = np.full(512, sigs.arena.base, np.uint64)
    assert ed25519.gather_layout_c(sz, CAP, BLOB)[0] == 512
    sz[-1] = 209
    assert ed25519.gather_layout_c(sz, CAP, BLOB)[0] == 511
    assert raw(512, sigs.pp[rep[:512]], sigs.sp[rep[:512]], mp, sz, True) == INVAL
    with pytest.raises(ed25519.EngineError):
        aeng.submit_batch([], [], [])
    blob, off, tsz = _txn.pack([b"\x01" * 300] * 513)
    with pytest.raises(ed25519.EngineError):
        aeng.submit_txns(blob, off, tsz)
    assert aeng.in_flight == before


# ---- 5. staged copies at submit ---------------------------------------------------------------

def test_5_staged_inputs_are_copied_at_submit(aeng, sigs):
    """Every input array zeroed right after the staged submit returns: the
    delivered verdicts and tags are those of the original bytes."""
    from firedancer_amd import ed25519
    L, P = ed25519.lib(), ed25519._ptr
    n = 300
    want = aeng.verify_batch(sigs.msgs[:n], sigs.sigs[:n], sigs.pubs[:n], want_tags=True)
    data = [np.frombuffer(b"".join(x[:n]), np.uint8).copy() for x in (sigs.msgs, sigs.sigs, sigs.pubs)]
    sz = sigs.sz[:n].copy()
    moff = np.concatenate(([0], np.cumsum(sz)[:-1])).astype(np.uint64)
    mp = data[0].ctypes.data + moff
    sp = data[1].ctypes.data + 64 * np.arange(n, dtype=np.uint64)
    pp = data[2].ctypes.data + 32 * np.arange(n, dtype=np.uint64)
    err, tag, t = np.full(n, S8, np.int8), np.full(n, S64, np.uint64), ctypes.c_ulong(0)
    assert L.fd_ed25519_amd_submit_batch(aeng._h, n, P(mp), P(sz), P(sp), P(pp), P(err), P(tag), ctypes.byref(t)) == OK
    for a in data + [sz, mp, sp, pp]:
        a[...] = 0
    assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (OK, t.value)
    assert np.array_equal(err, want[0]) and np.array_equal(tag, want[1])


# ---- 6. mixing -------------------------------------------------------------------------------------

def test_6_synchronous_calls_refuse_while_a_submission_is_in_flight(aeng, sigs, txns):
    from firedancer_amd import ed25519
    blob, off, sz = _txn.pack(txns.pays[:5])
    r = Raw(sigs, 300, aeng._h)
    assert r.submit() == OK
    for call in (lambda: aeng.verify_batch(sigs.msgs[:4], sigs.sigs[:4], sigs.pubs[:4]),
                 lambda: aeng.verify_batch_ptrs(sigs.pp[:4], sigs.sp[:4], sigs.mp[:4], sigs.sz[:4]),
                 lambda: aeng.verify_txns(blob, off, sz),
                 lambda: aeng.verify_txns_ptrs(txns.ptr[:5], txns.sz[:5]),
                 lambda: aeng.set_mode(ed25519.MODE_STRICT)):
        with pytest.raises(ed25519.EngineError, match="rc=-10"):
            call()
    assert aeng.in_flight == 1 and aeng.mode == ed25519.MODE_REFERENCE and r.untouched()
    assert _raw_collect(aeng, "fd_ed25519_amd_async_wait") == (OK, r.ticket.value)
    assert np.array_equal(aeng.verify_batch(sigs.msgs[:4], sigs.sigs[:4], sigs.pubs[:4]), sigs.expect[:4])
    assert aeng.verify_txns(blob, off, sz).shape == (5,)
    aeng.set_mode(ed25519.MODE_STRICT)
    assert aeng.mode == ed25519.MODE_STRICT


# ---- 7. mode at submit ---------------------------------------------------------------------------------

def test_7_a_submission_keeps_the_mode_it_was_submitted_in(aeng, sigs):
    from firedancer_amd import ed25519
    k = sigs.swin
    one = (sigs.pp[k:k + 1], sigs.sp[k:k + 1], sigs.mp[k:k + 1], sigs.sz[k:k + 1])
    aeng.submit_batch_ptrs(*one)
    assert aeng.wait()[1][0] == 0
    aeng.set_mode(ed25519.MODE_STRICT)
    aeng.submit_batch_ptrs(*one)
    assert aeng.wait()[1][0] == -1


# ---- 8. delete with one in flight ------------------------------------------------------------------------

def test_8_delete_with_a_submission_in_flight(sigs):
    """The call returns and delivers nothing: the outputs still hold 0x55."""
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=2)
    r = Raw(sigs, 300, e._h)
    assert r.submit() == OK and e.in_flight == 1
    e.close()
    assert r.untouched()


# ---- 9. event poll ------------------------------------------------------------------------------------------

def test_9_event_poll_gives_the_same_results():
    """Test 1's batch case in a fresh process whose engine polls with
    hipEventQuery (FD_ED25519_AMD_ASYNC_POLL=event, read at creation)."""
    env = dict(os.environ, FD_ED25519_AMD_ASYNC_POLL="event")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "async event poll: OK" in r.stdout, r.stdout + r.stderr


def _child():
    from firedancer_amd import ed25519
    assert os.environ.get("FD_ED25519_AMD_ASYNC_POLL") == "event"
    s = Sigs()
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    try:
        for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
            for registered in (False, True):
                _batch_equivalence(e, s, mode, registered)
    finally:
        e.close()
        s.arena.close()
    print("async event poll: OK")


if __name__ == "__main__":
    _child()
