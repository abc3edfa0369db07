"""GPU: the batch engine's chunk loops at the smallest shapes where they can
go wrong -- chunks that end on the signature count, on the byte limit, on
the message window and (transactions) on the slot limit, through every host
entry point, against the CPU oracle (strict mode: tests/_strict_ref.py).

A 64-signature engine keeps every case to a few hundred signatures."""
import ctypes

import numpy as np
import pytest

import _golden
import _oracle
import _strict_ref
import _txn

pytestmark = pytest.mark.gpu

CAP, BLOB = 64, 4096
ERR_INVAL = -10   # FD_ED25519_AMD_ERR_INVAL


def _batch(seed, n, szlo, szhi):
    """n signed messages of szlo..szhi bytes packed in order; about one in
    eight corrupted: a flipped message bit, s >= L, or an off-curve A."""
    from firedancer_amd import ed25519
    rng = np.random.default_rng(seed)
    sz = rng.integers(szlo, szhi + 1, n).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint32)
    blob = rng.integers(0, 256, int(sz.sum()) + 1, dtype=np.uint8)
    pub, sig = ed25519.sign_batch(rng.integers(0, 256, (n, 32), dtype=np.uint8), blob, off, sz)
    y = 2
    while _strict_ref.decode(y.to_bytes(32, "little")) is not None:   # the smallest y >= 2 with no x on the curve
        y += 1
    kinds = 0
    for k, i in enumerate(range(int(rng.integers(0, 8)), n, 8)):
        kind = k % 3 if sz[i] else 1 + k % 2          # the three kinds in turn
        if kind == 0:
            blob[off[i] + int(rng.integers(0, sz[i]))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            sig[i, 32:] = 0xff
        else:
            pub[i] = np.frombuffer(y.to_bytes(32, "little"), np.uint8)
        kinds |= 1 << kind
    assert kinds == 7
    for a in (pub, sig, off, sz, blob):
        a.setflags(write=False)
    return _golden.Batch(pub, sig, off, sz, blob)


def _expect(b):
    e = _oracle.verify_batch(b)
    assert len(set(e.tolist())) >= 3          # valid and at least two kinds of rejection
    e.setflags(write=False)
    return e


@pytest.fixture(scope="module")
def short():
    """Case 1: 200 > 3 * CAP signatures of 0..16 B: at least four chunks, each ended by the count."""
    b = _batch(101, 200, 0, 16)
    assert int(b.msg_sz.sum()) <= BLOB and (b.msg_sz == 0).any()
    return b, _expect(b)


@pytest.fixture(scope="module")
def long_():
    """Case 2: 40 signatures of 600..1232 B, more than 5 * BLOB in all: every chunk ends on the byte limit."""
    b = _batch(102, 40, 600, 1232)
    assert int(b.msg_sz.sum()) > 5 * BLOB and CAP * 600 > BLOB
    return b, _expect(b)


@pytest.fixture(scope="module")
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB)
    yield e
    e.close()


def _three(e, b, off=None, blob=None):
    """The verdicts of verify_batch, verify_soa and verify_soa_registered."""
    from firedancer_amd import ed25519
    off = b.msg_off if off is None else off
    blob = b.blob if blob is None else blob
    n = len(b)
    msgs = [bytes(blob[int(off[i]):int(off[i]) + int(b.msg_sz[i])]) for i in range(n)]
    out = {"batch": e.verify_batch(msgs, [bytes(s) for s in b.sig], [bytes(p) for p in b.pub]),
           "soa": e.verify_soa(b.pub, b.sig, off, b.msg_sz, blob)}
    r = ed25519.RegisteredPlanes(b.pub, b.sig, off, b.msg_sz, blob)
    try:
        out["registered"] = e.verify_soa_registered(r[0], r[1], r[2], r[3], r[4])
    finally:
        r.close()
    return out


def _check(out, exp):
    for name, err in out.items():
        assert np.array_equal(err, exp), (name, np.nonzero(err != exp)[0][:10])


def test_count_bound_chunks(eng, short):
    b, exp = short
    _check(_three(eng, b), exp)


def test_blob_bound_chunks(eng, long_):
    b, exp = long_
    _check(_three(eng, b), exp)


def _reversed_with_gaps(b, gap):
    """b's messages laid out last to first, `gap` unused bytes after each."""
    n = len(b)
    off, parts, pos = np.zeros(n, np.uint32), [], 0
    for j in range(n - 1, -1, -1):
        off[j] = pos
        parts.append(b.msg(j) + bytes(gap))
        pos += int(b.msg_sz[j]) + gap
    return off, np.frombuffer(b"".join(parts), np.uint8)


@pytest.mark.parametrize("blob_max", [BLOB, 4 * BLOB])
def test_window_and_gather_layouts(eng, long_, blob_max):
    """Case 2's messages packed in order (one block copy or DMA per chunk's
    window) and laid out last to first, 2048 B apart.  Spread like that, k
    messages of b bytes span b + 2048 (k - 1):
    - verify_soa sizes chunks by bytes alone, so its chunks (3 messages or
      more) span more than blob_max on either engine and are gathered;
    - the 4096-B engine's registered path breaks every chunk on the window
      (3 messages never fit it);
    - the 16384-B engine's registered path takes 4 messages or more within
      the window, which exceeds b + b/4 + 4096: gathered as well."""
    from firedancer_amd import ed25519
    b, exp = long_
    off, blob = _reversed_with_gaps(b, 2048)
    assert 3 * 1232 <= BLOB < 3 * 600 + 2 * 2048 and 13 * 1232 <= 4 * BLOB < 13 * 600 + 12 * 2048
    assert 4 * 1232 + 3 * 2048 <= 4 * BLOB and 3 * 2048 > 4 * 1232 // 4 + 4096
    e = eng if blob_max == BLOB else ed25519.Engine(device=0, batch_max=CAP, blob_max=blob_max)
    try:
        dense, sparse = _three(e, b), _three(e, b, off, blob)
    finally:
        if e is not eng:
            e.close()
    for name in ("soa", "registered"):
        assert np.array_equal(dense[name], sparse[name]), name
    _check(dense, exp)
    _check(sparse, exp)


def test_empty_messages_no_blob(eng):
    """70 signatures over the empty message; the blob reaches the library as NULL / 0 bytes."""
    from firedancer_amd import ed25519
    n = 70
    z = np.zeros(n, np.uint32)
    none = np.zeros(0, np.uint8)
    assert ed25519._ptr(none).value is None
    pub, sig = ed25519.sign_batch(np.random.default_rng(104).integers(0, 256, (n, 32), dtype=np.uint8),
                                  np.zeros(1, np.uint8), z, z)
    sig[5, 0] ^= 1
    sig[69, 40] ^= 1
    b = _golden.Batch(pub, sig, z, z, none)
    exp = _oracle.verify_batch(_golden.Batch(pub, sig, z, z, np.zeros(1, np.uint8)))
    assert exp[5] != 0 and exp[69] != 0 and (np.delete(exp, [5, 69]) == 0).all()
    _check(_three(eng, b), exp)


def _txns_raw(fn, h, payload, off, sz):
    """verify_txns with caller arrays the call has to fill: (rc, txn_err, sig_base, sig_err)."""
    from firedancer_amd import ed25519
    _, tot = ed25519.txn_slots(payload, off, sz)
    terr = np.full(off.size, 0x55, np.int8)
    base = np.full(off.size + 1, 0xffffffff, np.uint32)
    serr = np.full(tot, 0x55, np.int8)
    rc = fn(h, int(off.size), ed25519._ptr(payload), ed25519._ptr(off), ed25519._ptr(sz), int(payload.size),
            ed25519._ptr(terr), ed25519._ptr(base), ed25519._ptr(serr))
    return rc, terr, base, serr


def test_transaction_chunks():
    """30 transactions of 1..4 signers on an 8-slot, 4096-B engine: chunks end
    on the slot limit and on the byte limit (both asserted by restating the
    rule); single engine and a two-engine MultiEngine against the oracle."""
    from firedancer_amd import ed25519
    pays, nsig = _txn.build_txns(105, 20, nsig_lo=1, nsig_hi=4)
    big, one = _txn.build_txns(106, 10, nsig_lo=1, nsig_hi=1, msg_lo=1100)   # four of these exceed 4096 B with 4 slots
    pays, nsig = [bytearray(p) for p in pays + big], np.concatenate([nsig, one])
    for t in (3, 11, 12, 26):
        pays[t][1 + 64 * (int(nsig[t]) - 1) + 7] ^= 4     # the last signature of the transaction
    pays[20][-1] ^= 1
    payload, off, sz = _txn.pack([bytes(p) for p in pays])
    ends, t = set(), 0
    while t < 30:                                         # the engine's rule, restated
        c = by = ns = 0
        while t + c < 30 and c < 8:
            if by + int(sz[t + c]) > 4096:
                ends.add("bytes")
                break
            if ns + int(nsig[t + c]) > 8:
                ends.add("slots")
                break
            by, ns, c = by + int(sz[t + c]), ns + int(nsig[t + c]), c + 1
        t += c
    assert ends == {"bytes", "slots"}
    eterr, ebase, eserr = _oracle.txn_verify_batch(payload, off, sz)
    assert (eterr != 0).sum() >= 4 and (eserr != 0).sum() >= 4
    assert np.array_equal(ed25519.txn_slots(payload, off, sz)[0], ebase)
    L = ed25519.lib()
    e = ed25519.Engine(device=0, batch_max=8, blob_max=4096)
    try:
        rc, terr, base, serr = _txns_raw(L.fd_ed25519_amd_verify_txns, e._h, payload, off, sz)
    finally:
        e.close()
    assert rc == 0
    assert np.array_equal(terr, eterr) and np.array_equal(base, ebase) and np.array_equal(serr, eserr)
    m = ed25519.MultiEngine([0, 0], batch_max=8, blob_max=4096)
    try:
        rc, terr, base, serr = _txns_raw(L.fd_ed25519_amd_multi_verify_txns, m._h, payload, off, sz)
    finally:
        m.close()
    assert rc == 0
    assert np.array_equal(terr, eterr) and np.array_equal(base, ebase) and np.array_equal(serr, eserr)


def test_engine_survives_refused_call(eng, short):
    """A 5000-B message (> blob_max) in the middle of case 1's batch: every
    entry point refuses the call with ERR_INVAL and leaves the caller's
    verdict array alone; the same engine then verifies case 1."""
    from firedancer_amd import ed25519
    b, exp = short
    n = len(b)
    off, sz = b.msg_off.copy(), b.msg_sz.copy()
    off[100], sz[100] = b.blob.size, 5000
    blob = np.concatenate([b.blob, np.zeros(5000, np.uint8)])
    L, p = ed25519.lib(), ed25519._ptr
    err = np.full(n, 0x55, np.int8)
    rc = L.fd_ed25519_amd_verify_soa(eng._h, n, p(b.pub), p(b.sig), p(off), p(sz), p(blob), int(blob.size), p(err))
    assert rc == ERR_INVAL and (err == 0x55).all()
    r = ed25519.RegisteredPlanes(b.pub, b.sig, off, sz, blob)
    try:
        rc = L.fd_ed25519_amd_verify_soa_registered(eng._h, n, p(r[0]), p(r[1]), p(r[2]), p(r[3]), p(r[4]),
                                                    int(blob.size), p(err))
    finally:
        r.close()
    assert rc == ERR_INVAL and (err == 0x55).all()
    msgs = [ctypes.create_string_buffer(bytes(blob[int(off[i]):int(off[i]) + int(sz[i])]), max(int(sz[i]), 1))
            for i in range(n)]
    arr = lambda rows: (ctypes.c_void_p * n)(*[ctypes.c_void_p(a.ctypes.data) for a in rows])
    mp = (ctypes.c_void_p * n)(*[ctypes.cast(m, ctypes.c_void_p) for m in msgs])
    rc = L.fd_ed25519_amd_verify_batch(eng._h, n, mp, (ctypes.c_ulong * n)(*[int(s) for s in sz]), arr(b.sig),
                                       arr(b.pub), p(err))
    assert rc == ERR_INVAL and (err == 0x55).all()
    _check(_three(eng, b), exp)
    assert (err == 0x55).all()                # no later call delivered into the refused calls' array


def test_strict_mode_chunks(short):
    from firedancer_amd import ed25519
    b, exp = short
    want = np.array(_strict_ref.verify_batch(b), np.int8)
    assert len(set(want.tolist())) >= 3
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, mode=ed25519.MODE_STRICT)
    r = ed25519.RegisteredPlanes(b.pub, b.sig, b.msg_off, b.msg_sz, b.blob)
    try:
        out = _three(e, b)
        # the registered call's DMA chunks again with tags asked for: three of 64 and a last one of 8
        terr, tag = e.verify_soa_registered(r[0], r[1], r[2], r[3], r[4], want_tags=True)
    finally:
        r.close()
        e.close()
    del out["batch"]
    _check(out, want)
    from test_tags_gpu import _expected as _tags
    assert len(b) % CAP == 8
    assert np.array_equal(terr, want), np.nonzero(terr != want)[0][:10]
    assert np.array_equal(tag, _tags(b, exp)), np.nonzero(tag != _tags(b, exp))[0][:10]
