"""GPU: fd_ed25519_amd_verify_txns_desc and
fd_ed25519_amd_verify_txns_registered_desc -- the host batch calls that
return the packed fd_txn_t descriptors with the verdicts and tags.

Expected descriptors are the oracle's fd_txn_parse, concatenated, and their
64-bit running sum; the other five outputs must equal those of the _tag call
on the same engine.  All comparisons are exact.

The engines are small (batch_max 64, blob_max 4096) so that a batch of a few
hundred transactions takes an ODD number of chunks: the descriptors of chunk
k lie behind those of all earlier chunks, so they must be delivered in chunk
order, and with 5 chunks on the default ring of 2 slots (7 on a ring of 3)
the chunks still in flight at the end are not in slot order."""
import numpy as np
import pytest

import _oracle
import _txn

pytestmark = pytest.mark.gpu

ERR_INVAL, ERR_PARSE = -10, -4
PAGE = 4096
CAP, BLOB = 64, 4096


def expected_desc(pays):
    ds = []
    for p in pays:
        fp, d, _ = _oracle.txn_parse(p)
        ds.append(d[:fp])
    off = np.zeros(len(pays) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in ds], dtype=np.uint64)
    return off, np.frombuffer(b"".join(ds), np.uint8)


@pytest.fixture(scope="module")
def corpus():
    """360 payloads, computed once: valid 1..4-signer transactions from
    _txn.build_txns, every fifth with one corrupted signature bit, every
    seventh with a corrupted header (a parse failure), every eleventh
    truncated, and junk of 0..40 B in between."""
    pays, nsig = _txn.build_txns(9101, 300, nsig_lo=1, nsig_hi=4, msg_lo=64, msg_hi=420)
    rng = np.random.default_rng(9102)
    out = []
    for t, p in enumerate(pays):
        p = bytearray(p)
        m = 1 + 64 * int(nsig[t])
        if t % 5 == 2:
            p[1 + int(rng.integers(0, 64 * int(nsig[t])))] ^= 1 << int(rng.integers(0, 8))
        if t % 7 == 3:
            p[m + (1 if p[m] & 0x80 else 0)] ^= 0x40
        if t % 11 == 5:
            p = p[:int(rng.integers(0, len(p)))]
        out.append(bytes(p))
        if t % 5 == 0:
            out.append(rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes())
    assert len(out) == 360
    blob, off, sz = _txn.pack(out)
    terr, _, _ = _oracle.txn_verify_batch(blob, off, sz)
    assert set(np.unique(terr).tolist()) >= {0, -3, ERR_PARSE} and (terr == 0).sum() > 150
    return out


def staged_chunks(pays, cap, blob_cap):
    """How fd_ed25519_amd_verify_txns cuts a batch: a chunk takes payloads
    while their count and signature slots stay <= cap and their bytes <=
    blob_cap."""
    from firedancer_amd import ed25519
    blob, off, sz = _txn.pack(pays)
    slots = np.diff(ed25519.txn_slots(blob, off, sz)[0].astype(np.int64))
    chunks, c, b, ns = [], 0, 0, 0
    for z, k in zip(sz.tolist(), slots.tolist()):
        if c and (c >= cap or b + z > blob_cap or ns + k > cap):
            chunks.append(c)
            c = b = ns = 0
        c, b, ns = c + 1, b + z, ns + k
    return chunks + ([c] if c else [])


def gathered_chunks(pays, cap, blob_cap):
    from firedancer_amd import ed25519
    blob, off, sz = _txn.pack(pays)
    slots = np.diff(ed25519.txn_slots(blob, off, sz)[0].astype(np.int64))
    chunks, i = [], 0
    while i < len(pays):
        c, _, _ = ed25519.txn_gather_layout(sz[i:].astype(np.uint64), slots[i:], cap, blob_cap)
        chunks.append(c)
        i += c
    return chunks


def prefix_with_chunks(pays, count, rule):
    """The shortest prefix of pays that `rule` cuts into `count` chunks."""
    for n in range(1, len(pays) + 1):
        if len(rule(pays[:n], CAP, BLOB)) == count:
            return pays[:n]
    raise AssertionError("the corpus never takes %d chunks" % count)


class Arena:
    """Page-aligned host memory, 0xA5-filled, registered whole (one
    registration); put() lays a byte string at the next 16-aligned slot +
    align, at least 16 filler bytes behind the previous one."""

    def __init__(self, nbytes):
        from firedancer_amd import ed25519
        nbytes = (nbytes + PAGE - 1) & ~(PAGE - 1)
        self._raw = np.full(nbytes + 2 * PAGE, 0xA5, np.uint8)
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


NAMES = ("txn_err", "sig_base", "sig_err", "txn_tag", "sig_tag", "desc_off", "desc")


def same(got, want, names=NAMES):
    assert len(got) == len(want)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:8])


def check_desc(pays, got, tagged):
    """got: the seven outputs of a _desc call; tagged: the five of the _tag
    call on the same engine."""
    same(got[:5], tagged)
    eoff, edesc = expected_desc(pays)
    same(got[5:], (eoff, edesc), NAMES[5:])
    empty = np.diff(got[5].astype(np.int64)) == 0
    assert np.array_equal(empty, got[0] == ERR_PARSE)
    assert empty.any() and not empty.all()


# ---- 4. the staged call -----------------------------------------------------------

@pytest.mark.parametrize("mode", ["reference", "strict"])
def test_verify_txns_desc_over_five_chunks(corpus, mode):
    from firedancer_amd import ed25519
    pays = prefix_with_chunks(corpus, 5, staged_chunks)
    blob, off, sz = _txn.pack(pays)
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB,
                       mode=ed25519.MODE_STRICT if mode == "strict" else ed25519.MODE_REFERENCE)
    try:
        tagged = e.verify_txns(blob, off, sz, want_sigs=True, want_tags=True)
        if mode == "reference":
            eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
            same(tagged[:3], (eterr, ebase, eserr))
        got = e.verify_txns(blob, off, sz, want_sigs=True, want_tags=True, want_desc=True)
        check_desc(pays, got, tagged)
        # the forms with fewer outputs
        terr, doff, desc = e.verify_txns(blob, off, sz, want_desc=True)
        same((terr, doff, desc), (tagged[0],) + tuple(got[5:]), (NAMES[0],) + NAMES[5:])
    finally:
        e.close()


def test_verify_txns_desc_single_chunk_and_empty_batch(corpus):
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB)
    try:
        for pays in (corpus[:9], [b"", b"\x01" * 30]):
            blob, off, sz = _txn.pack(pays)
            got = e.verify_txns(blob, off, sz, want_sigs=True, want_tags=True, want_desc=True)
            same(got[:5], e.verify_txns(blob, off, sz, want_sigs=True, want_tags=True))
            same(got[5:], expected_desc(pays), NAMES[5:])
        terr, doff, desc = e.verify_txns(np.zeros(4, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32), want_desc=True)
        assert terr.size == 0 and doff.tolist() == [0] and desc.size == 0
    finally:
        e.close()


# ---- 5. the registered call -------------------------------------------------------

@pytest.mark.parametrize("mode", ["reference", "strict"])
def test_verify_txns_registered_desc_over_seven_chunks_on_three_slots(corpus, mode, monkeypatch):
    """Payload pointers at every byte alignment 0..15 inside one registration,
    a ring of three slots, seven chunks."""
    from firedancer_amd import ed25519
    monkeypatch.setenv("FD_ED25519_AMD_NSLOT", "3")
    pays = prefix_with_chunks(corpus, 7, gathered_chunks)
    assert len(pays) >= 16
    a = Arena(sum(len(p) + 64 for p in pays) + PAGE)
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB,
                       mode=ed25519.MODE_STRICT if mode == "strict" else ed25519.MODE_REFERENCE)
    try:
        ptr = np.array([a.put(p, t % 16) for t, p in enumerate(pays)], np.uint64)
        assert sorted(set(int(p) % 16 for p in ptr)) == list(range(16))
        sz = np.array([len(p) for p in pays], np.uint64)
        before = a.mem.copy()
        tagged = e.verify_txns_ptrs(ptr, sz, want_sigs=True, want_tags=True)
        blob, off, psz = _txn.pack(pays)
        same(tagged, e.verify_txns(blob, off, psz, want_sigs=True, want_tags=True))
        got = e.verify_txns_ptrs(ptr, sz, want_sigs=True, want_tags=True, want_desc=True)
        check_desc(pays, got, tagged)
        assert np.array_equal(a.mem, before)               # the kernels only read caller memory
        terr, doff, desc = e.verify_txns_ptrs(ptr, sz, want_desc=True)
        same((terr, doff, desc), (tagged[0],) + tuple(got[5:]), (NAMES[0],) + NAMES[5:])
    finally:
        e.close()
        a.close()


def test_registered_desc_refusals_leave_desc_untouched(corpus):
    """An unregistered pointer, and a capacity one byte under the bound sum,
    return ERR_INVAL with desc and desc_off untouched; the bound sum itself is
    accepted."""
    from firedancer_amd import ed25519
    L, P = ed25519.lib(), ed25519._ptr
    pays = [p for p in corpus[:40]]
    a = Arena(sum(len(p) + 64 for p in pays) + PAGE)
    plain = np.frombuffer(pays[3] + bytes(64), np.uint8).copy()       # ordinary memory, never registered
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB)
    try:
        ptr = np.array([a.put(p, (3 * t) % 16) for t, p in enumerate(pays)], np.uint64)
        sz = np.array([len(p) for p in pays], np.uint64)
        n = len(pays)
        need = sum(ed25519.txn_desc_bound(len(p)) for p in pays)
        eoff, edesc = expected_desc(pays)

        def call(p, cap):
            terr = np.full(n, 0x55, np.int8)
            doff, desc = np.full(n + 1, 0x5555555555555555, np.uint64), np.full(need + 64, 0x55, np.uint8)
            rc = L.fd_ed25519_amd_verify_txns_registered_desc(e._h, n, P(p), P(sz), P(terr), None, None, None, None, P(doff),
                                                              P(desc), cap)
            return rc, terr, doff, desc

        bad = ptr.copy()
        bad[3] = plain.ctypes.data
        for p, cap in ((bad, need), (ptr, need - 1)):
            rc, terr, doff, desc = call(p, cap)
            assert rc == ERR_INVAL
            assert (terr == 0x55).all() and (doff == 0x5555555555555555).all() and (desc == 0x55).all()
        rc, terr, doff, desc = call(ptr, need)
        assert rc == 0
        total = int(eoff[-1])
        assert np.array_equal(doff, eoff) and np.array_equal(desc[:total], edesc) and (desc[total:] == 0x55).all()
        assert np.array_equal(terr, e.verify_txns_ptrs(ptr, sz))
    finally:
        e.close()
        a.close()


# ---- 6. reuse ---------------------------------------------------------------------

def test_reuse_of_an_engine_with_and_without_descriptors(corpus):
    """A call with descriptors, one without, one with descriptors of another
    batch, on one engine: the second and third equal a fresh engine's, so
    nothing depends on what the staging held."""
    from firedancer_amd import ed25519
    x = prefix_with_chunks(corpus, 5, staged_chunks)
    y = prefix_with_chunks(corpus[100:], 3, staged_chunks)
    bx, ox, sx = _txn.pack(x)
    by, oy, sy = _txn.pack(y)
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB)
    fresh1 = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB)
    fresh2 = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB)
    try:
        first = e.verify_txns(bx, ox, sx, want_sigs=True, want_tags=True, want_desc=True)
        second = e.verify_txns(bx, ox, sx, want_sigs=True, want_tags=True)
        third = e.verify_txns(by, oy, sy, want_sigs=True, want_tags=True, want_desc=True)
        same(second, fresh1.verify_txns(bx, ox, sx, want_sigs=True, want_tags=True))
        same(third, fresh2.verify_txns(by, oy, sy, want_sigs=True, want_tags=True, want_desc=True))
        same(first[5:], expected_desc(x), NAMES[5:])
        same(third[5:], expected_desc(y), NAMES[5:])
    finally:
        for k in (e, fresh1, fresh2):
            k.close()
