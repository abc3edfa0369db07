"""GPU: fd_ed25519_amd_verify_txns_registered -- the transaction batch in
pointer-array form whose payloads a kernel (k_gather_txn) fetches from
registered host memory.

The valid inputs come from _txn.build_txns (fresh keys, valid signatures; the
CPU oracle gives 0 for every one of them, asserted, seeds pinned), and the
calls ask for the dedup tags: a tag is SHA-512(R || A || M)[0:8], so a single
wrong gathered byte of R, A or the message shows twice, as a -3 verdict and as
a tag that differs from ed25519.tag's (host code, hashlib-equal:
test_tags_cpu.py); a wrong byte of s or of the signature count shows as a
wrong verdict or as -4.  Expected values come from _oracle.txn_verify_batch,
from Engine.verify_txns on the same payloads (the staged path) and from
ed25519.tag.  All comparisons are exact."""
import struct

import numpy as np
import pytest

import _oracle
import _txn

pytestmark = pytest.mark.gpu

ALIGNS = [0, 1, 2, 3, 5, 8, 13, 15]
ERR_INVAL = -10
PAGE = 4096


class Arena:
    """A page-aligned block of host memory, 0xA5-filled, with a whole page of
    ordinary (never registered) memory before and behind it; bytes
    [lo, size - hi) of it are registered with host_register (one
    registration).  put() lays a byte string at the next 16-aligned slot +
    `align`, at least 16 filler bytes after the previous one."""

    def __init__(self, nbytes, register=True, lo=0, hi=0):
        nbytes = (nbytes + PAGE - 1) & ~(PAGE - 1)
        self._raw = np.full(nbytes + 3 * PAGE, 0xA5, np.uint8)
        o = (-self._raw.ctypes.data) % PAGE + PAGE
        self.mem = self._raw[o:o + nbytes]
        self.base = int(self.mem.ctypes.data)
        self.size = nbytes
        self.pos = lo
        self._reg = []
        if register:
            self.register(lo, nbytes - hi)

    def register(self, a, b):
        from firedancer_amd import ed25519
        v = self.mem[a:b]
        ed25519.host_register(v)
        self._reg.append(v)

    def put(self, data, align=0):
        o = ((self.pos + 15) & ~15) + 16 + align
        return self.put_at(o, data)

    def put_at(self, o, data):
        d = np.frombuffer(bytes(data), np.uint8)
        assert o >= 0 and o + d.size <= self.size
        self.mem[o:o + d.size] = d
        self.pos = max(self.pos, o + d.size)
        return self.base + o

    def close(self):
        from firedancer_amd import ed25519
        for v in self._reg:
            ed25519.host_unregister(v)
        self._reg = []


class Expect:
    """Per payload: the oracle's transaction verdict and per-signature codes,
    and the tags by ed25519.tag over the fields the oracle's parser found (0
    where the payload did not parse or the reference's s check rejects).
    select(idx) gives the five outputs of a batch that lists payloads idx."""

    def __init__(self, pays):
        from firedancer_amd import ed25519
        self.pays = [bytes(p) for p in pays]
        blob, off, sz = _txn.pack(self.pays)
        terr, base, serr = _oracle.txn_verify_batch(blob, off, sz)
        self.terr = terr.copy()
        self.serr, self.stag, self.ttag = [], [], np.zeros(len(pays), np.uint64)
        for t, p in enumerate(self.pays):
            se = serr[base[t]:base[t + 1]].copy()
            tg = np.zeros(se.size, np.uint64)
            if terr[t] != -4:
                _, d, _ = _oracle.txn_parse(p)
                n = d[1]
                so, mo = struct.unpack_from("<HH", d, 2)
                ao = struct.unpack_from("<H", d, 10)[0]
                assert n == se.size
                for k in range(n):
                    if se[k] != -1:
                        tg[k] = ed25519.tag(p[mo:], p[so + 64 * k:so + 64 * k + 64], p[ao + 32 * k:ao + 32 * k + 32])
                self.ttag[t] = tg[0]
            self.serr.append(se)
            self.stag.append(tg)

    def select(self, idx):
        idx = [int(i) for i in idx]
        cnt = [self.serr[i].size for i in idx]
        base = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
        return (self.terr[idx], base, cat([self.serr[i] for i in idx], np.int8), self.ttag[idx],
                cat([self.stag[i] for i in idx], np.uint64))


def _bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return int(bad.size), [(int(i), int(want[i]), int(got[i])) for i in bad[:6]]


NAMES = ("txn_err", "sig_base", "sig_err", "txn_tag", "sig_tag")


def _same(got, want):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (name,) + _bad(g, w)


def _exact(e, ptr, sz, want):
    """The call with every output, against the five expected arrays."""
    got = e.verify_txns_ptrs(np.asarray(ptr, np.uint64), np.asarray(sz, np.uint64), want_sigs=True, want_tags=True)
    _same(got, want)


def _lens(pays):
    return np.array([len(p) for p in pays], np.uint64)


@pytest.fixture(scope="module")
def pool():
    """Valid transactions, computed once: 48 one-signer payloads whose sizes
    cover every residue mod 16, the smallest payload build_txns makes, three
    of exactly 1232 B, twelve 12-signer ones and 24 with 1..3 signers; and the
    unparseable payloads of 0, 1, 15, 16 and 17 bytes."""
    ones, _ = _txn.build_txns(7001, 48, nsig_lo=1, nsig_hi=1, msg_lo=200, msg_hi=263)
    tiny, _ = _txn.build_txns(7002, 1, nsig_lo=1, nsig_hi=1, msg_lo=0, msg_hi=0)
    full, _ = _txn.build_txns(7003, 3, nsig_lo=1, nsig_hi=1, msg_lo=1232, msg_hi=1232, mtu=1233)
    twelve, n12 = _txn.build_txns(7004, 12, nsig_lo=12, nsig_hi=12)
    mids, _ = _txn.build_txns(7005, 24, nsig_lo=1, nsig_hi=3, msg_lo=64, msg_hi=400)
    rng = np.random.default_rng(7006)
    junk = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 1, 15, 16, 17)]
    assert sorted(set(len(p) % 16 for p in ones)) == list(range(16))
    assert all(len(p) == 1232 for p in full) and len(tiny[0]) < min(len(p) for p in ones) and (n12 == 12).all()

    class P:
        pass
    p = P()
    p.ones, p.tiny, p.full, p.twelve, p.mids, p.junk = (list(range(0, 48)), [48], [49, 50, 51], list(range(52, 64)),
                                                        list(range(64, 88)), list(range(88, 93)))
    p.exp = Expect(ones + tiny + full + twelve + mids + junk)
    p.pays = p.exp.pays
    valid = p.ones + p.tiny + p.full + p.twelve + p.mids
    assert not p.exp.terr[valid].any() and not any(p.exp.serr[i].any() for i in valid), \
        "a fresh valid signature the reference rejects: pick another seed"
    assert (p.exp.terr[p.junk] == -4).all() and all(p.exp.serr[i].size == 0 for i in p.junk)
    assert all((p.exp.stag[i] != 0).all() for i in valid)
    return p


@pytest.fixture(scope="module")
def small_engine():
    """64 transactions, 64 signature slots and 4096 payload bytes per chunk, two slots."""
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=64, blob_max=4096)
    yield e
    e.close()


# ---- 1. alignment x size ----------------------------------------------------------

def test_every_alignment_at_every_size(engine, pool):
    """One-signer payloads of every size residue mod 16, the smallest, the
    1232-B ones and the unparseable 0 / 1 / 15 / 16 / 17-B ones, each at every
    start offset mod 16 of ALIGNS, 0xA5 filler around every one."""
    idx = [i for i in pool.ones + pool.tiny + pool.full + pool.junk for _ in ALIGNS]
    al = [a for _ in pool.ones + pool.tiny + pool.full + pool.junk for a in ALIGNS]
    a = Arena(sum(len(pool.pays[i]) + 64 for i in idx) + PAGE)
    try:
        ptr = np.array([a.put(pool.pays[i], x) for i, x in zip(idx, al)], np.uint64)
        assert sorted(set(int(p) % 16 for p in ptr)) == ALIGNS
        before = a.mem.copy()
        _exact(engine, ptr, _lens([pool.pays[i] for i in idx]), pool.exp.select(idx))
        assert np.array_equal(a.mem, before)               # the kernel only reads caller memory
    finally:
        a.close()


# ---- 2. registration edges --------------------------------------------------------

@pytest.mark.parametrize("start_mod", [0, 1, 15])
def test_payloads_flush_against_both_ends_of_a_registration(engine, pool, start_mod):
    """One payload starts at the first byte of a registration and the same
    payload ends at its last byte, ordinary unregistered pages on both sides;
    the registration's ends are chosen so that both copies start at
    start_mod mod 16 (k_gather_txn loads only aligned 16-B words holding a
    byte of the range, so neither copy makes it touch a neighbouring page:
    fd_ed25519_gather.h).  Also a 1232-B payload at each end."""
    for i in (pool.ones[3], pool.full[0]):
        p = pool.pays[i]
        hi = (2 * PAGE - start_mod - len(p)) % 16          # the registration ends where a copy starting at start_mod mod 16 ends
        a = Arena(2 * PAGE, lo=start_mod, hi=hi)
        try:
            end = a.size - hi
            first, last = a.put_at(start_mod, p), a.put_at(end - len(p), p)
            assert first % 16 == start_mod and last % 16 == start_mod and last + len(p) == a.base + end
            mid = a.put_at(PAGE + 64 + 7, pool.pays[pool.ones[5]])
            idx = [i, pool.ones[5], i]
            _exact(engine, [first, mid, last], _lens([pool.pays[k] for k in idx]), pool.exp.select(idx))
        finally:
            a.close()


# ---- 3. every size, every grammar failure -----------------------------------------

def test_every_mutation_and_truncation_of_the_fixtures(engine):
    """Every payload of _txn.mutation_list for the three committed fixtures
    (byte edits plus every truncation length), back to back and unaligned in
    one arena: txn_err equals the oracle's, and every output equals
    Engine.verify_txns's on the same bytes."""
    pays = []
    for f in _txn.load_fixtures():
        pays += _txn.mutation_list(f.payload)
    blob, off, sz = _txn.pack(pays)
    assert int(sz.min()) == 0 and len(set((sz % 16).tolist())) == 16
    eterr, ebase, _ = _oracle.txn_verify_batch(blob, off, sz)
    assert (eterr == -4).sum() > 5000 and (eterr != -4).sum() > 5000 and len(set(np.unique(eterr).tolist())) >= 3
    want = engine.verify_txns(blob, off, sz, want_sigs=True, want_tags=True)
    assert np.array_equal(want[0], eterr) and np.array_equal(want[1], ebase)
    a = Arena(int(blob.size) + PAGE)
    try:
        a.put_at(1, blob)                                  # payload t at arena offset 1 + off[t]
        got = engine.verify_txns_registered(a.mem, off.astype(np.uint64) + np.uint64(1), sz, want_sigs=True, want_tags=True)
        assert np.array_equal(got[0], eterr), _bad(got[0], eterr)
        _same(got, want)
    finally:
        a.close()


# ---- 4. pointer sources -----------------------------------------------------------

def test_two_registrations_repeats_and_overlapping_payloads(engine, pool):
    a, b = Arena(64 * 1024), Arena(64 * 1024)
    try:
        src = pool.mids + pool.twelve[:4] + pool.full[:2]
        ptr = [(a if k % 2 == 0 else b).put(pool.pays[i], (5 * k) % 16) for k, i in enumerate(src)]
        # the same payloads listed again, many times
        rep = [0, 3, 3, 3, 24, 3, 29, 3, 0, 3] * 5
        idx = src + [src[k] for k in rep]
        _exact(engine, ptr + [ptr[k] for k in rep], _lens([pool.pays[i] for i in idx]), pool.exp.select(idx))
        # a payload and truncations of it that share its bytes (the same pointer with a smaller size), and its
        # tail as a payload of its own (a pointer into the middle of it)
        p = pool.pays[pool.mids[2]]
        cuts = [len(p), len(p) - 1, 66, 65, 64, 1, 0, len(p)]
        over = [p[:c] for c in cuts] + [p[40:], p[1:]]
        exp = Expect(over)
        assert exp.terr[0] == 0 and exp.terr[7] == 0 and (exp.terr[1:7] == -4).all()
        q = ptr[src.index(pool.mids[2])]
        _exact(engine, [q] * len(cuts) + [q + 40, q + 1], _lens(over), exp.select(range(len(over))))
    finally:
        a.close()
        b.close()


# ---- 5. refusals ------------------------------------------------------------------

SENT8, SENT32, SENT64 = 0x55, 0x55555555, 0x5555555555555555


def test_refusals_leave_outputs_untouched_and_the_engine_usable(pool):
    """batch_max = 8 (so a 12-signer payload reserves more slots than a chunk
    has) and the smallest blob_max an engine has, 1232 B."""
    from firedancer_amd import ed25519
    L, P = ed25519.lib(), ed25519._ptr
    e = ed25519.Engine(device=0, batch_max=8, blob_max=1232)
    good = Arena(64 * 1024)
    plain = Arena(8192, register=False)                    # ordinary memory, never registered
    two = Arena(2 * PAGE, register=False)                  # two adjacent registrations, one page each
    two.register(0, PAGE)
    two.register(PAGE, 2 * PAGE)
    try:
        idx = (pool.mids[:6] + pool.ones[:4]) * 20          # 200 transactions, <= 3 signers each
        by = {i: good.put(pool.pays[i], i % 16) for i in set(idx)}
        ptr = np.array([by[i] for i in idx], np.uint64)
        sz = _lens([pool.pays[i] for i in idx])
        want = pool.exp.select(idx)
        nsl = int(want[1][-1])
        victim = pool.pays[idx[5]]
        twelve = good.put(pool.pays[pool.twelve[0]])
        big = good.put(bytes(1300))

        def call(p, z, n=200, base=True, serr=True, null=()):
            out = [np.full(200, SENT8, np.int8), np.full(201, SENT32, np.uint32), np.full(nsl + 64, SENT8, np.int8),
                   np.full(200, SENT64, np.uint64), np.full(nsl + 64, SENT64, np.uint64)]
            a = [None if "txn" in null else P(p), None if "sz" in null else P(z), None if "err" in null else P(out[0]),
                 P(out[1]) if base else None, P(out[2]) if serr else None, P(out[3]), P(out[4])]
            rc = L.fd_ed25519_amd_verify_txns_registered_tag(e._h, n, *a)
            return rc, out

        def refused(p, z, **kw):
            rc, out = call(p, z, **kw)
            assert rc == ERR_INVAL
            for o, s in zip(out, (SENT8, SENT32, SENT8, SENT64, SENT64)):
                assert (o.view(np.uint8 if o.dtype == np.int8 else o.dtype) == s).all()
            _exact(e, ptr, sz, want)                        # the next valid call is exact

        def edit(t, p=None, z=None):
            pp, zz = ptr.copy(), sz.copy()
            if p is not None:
                pp[t] = p
            if z is not None:
                zz[t] = z
            return pp, zz

        rc, out = call(ptr, sz)                             # the control: the unedited batch is accepted
        assert rc == 0
        _same((out[0], out[1], out[2][:nsl], out[3], out[4][:nsl]), want)
        assert (out[2][nsl:] == SENT8).all() and (out[4][nsl:] == SENT64).all()
        refused(ptr, sz, null=("txn",))                     # NULL arrays
        refused(ptr, sz, null=("sz",))
        refused(ptr, sz, null=("err",))
        refused(*edit(5, p=0))                              # a NULL pointer with a size
        refused(*edit(5, p=big, z=1233))                    # above the MTU (and above this engine's blob_max)
        refused(*edit(5, p=plain.put(victim)))              # unregistered memory
        refused(*edit(5, p=two.put_at(PAGE - 40, victim)))  # spans two adjacent registrations
        refused(*edit(5, p=good.base + good.size - len(victim) + 1))   # its last byte one past the registration
        refused(*edit(199, p=plain.put(pool.pays[idx[199]])))   # the last of 200: nothing was launched
        refused(*edit(5, p=twelve, z=len(pool.pays[pool.twelve[0]])))   # 12 slots > batch_max 8
        refused(ptr, sz, base=False)                        # sig_err (and sig_tag) without sig_base
        with pytest.raises(ed25519.EngineError):
            e.verify_txns_ptrs(*edit(5, p=0), want_sigs=True)
        with pytest.raises(ed25519.EngineError):
            e.verify_txns_ptrs(*edit(5, p=plain.put(victim)), want_sigs=True)
        # controls: the same edit where it stays legal is accepted -- wholly inside either of the two
        # registrations, flush against their shared edge
        for q in (two.put_at(PAGE - len(victim), victim), two.put_at(PAGE, victim)):
            _exact(e, edit(5, p=q)[0], sz, want)
    finally:
        e.close()
        for a in (good, plain, two):
            a.close()


def test_null_pointer_with_size_zero_is_accepted(small_engine, pool):
    """txn[t] is not looked at when txn_sz[t] is 0: NULL, or an address that is
    no memory at all, gets -4 and no slot, beside payloads that verify."""
    a = Arena(PAGE)
    try:
        i, k = pool.ones[0], pool.mids[1]
        ptr = [a.put(pool.pays[i], 3), 0, a.put(pool.pays[k], 9), 8, 0]
        exp = Expect([pool.pays[i], b"", pool.pays[k], b"", b""])
        assert exp.terr.tolist() == [0, -4, 0, -4, -4]
        _exact(small_engine, ptr, [len(pool.pays[i]), 0, len(pool.pays[k]), 0, 0], exp.select(range(5)))
        _exact(small_engine, [0, 0], [0, 0], exp.select([1, 3]))          # a batch of nothing but empty payloads
    finally:
        a.close()


# ---- 6. chunking ------------------------------------------------------------------

@pytest.fixture(scope="module")
def chunk_arena(pool):
    """200 transactions in one arena: 130 unparseable payloads of 0..40 B (64
    of them fit 4096 padded bytes: chunks end on the count), runs of 1232-B
    and of 12-signer payloads (three fit 4096 B: chunks end on bytes) between
    1..3-signer ones, then tiny ones again."""
    rng = np.random.default_rng(7007)
    tiny = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 41, 163)]
    exp_tiny = Expect(tiny)
    assert (exp_tiny.terr == -4).all()
    order = [("t", k) for k in range(130)] + [("p", i) for i in (pool.full * 4)[:10]] + [("p", i) for i in pool.mids[:20]] + \
            [("p", i) for i in pool.twelve[:7]] + [("t", k) for k in range(130, 163)]
    assert len(order) == 200
    pays = [tiny[k] if w == "t" else pool.pays[k] for w, k in order]
    a = Arena(sum(len(p) + 64 for p in pays) + PAGE)
    ptr = np.array([a.put(p, (7 * t) % 16) for t, p in enumerate(pays)], np.uint64)
    exp = Expect(pays)
    yield ptr, _lens(pays), exp, pays
    a.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_chunks_keep_caller_order_and_reuse_the_slots(small_engine, chunk_arena, n):
    """batch_max 64, blob_max 4096: chunks that end on the count and on the
    padded bytes; twice, so both slots are reused, caller order and the global
    sig_base / sig_err numbering kept across them.  Every output equals the
    expected one and verify_txns's of the same engine.  (No chunk of this
    engine can end on the slots: 64 slots take more than 4096 payload bytes;
    test_chunks_that_end_on_the_signature_slots has those.)"""
    from firedancer_amd import ed25519
    ptr, sz, exp, pays = chunk_arena
    want = exp.select(range(n))
    slots = np.diff(want[1].astype(np.int64))
    chunks, i = [], 0
    while i < n:
        c, _, ns = ed25519.txn_gather_layout(sz[i:n], slots[i:], 64, 4096)
        assert ns <= 64
        chunks.append(c)
        i += c
    assert chunks[0] == min(n, 64)
    if n == 200:
        assert chunks[:2] == [64, 64] and chunks.count(3) >= 3 and len(chunks) > 8   # more chunks than slots: reuse within a call
    blob, off, psz = _txn.pack(pays[:n])
    _same(small_engine.verify_txns(blob, off, psz, want_sigs=True, want_tags=True), want)
    for _ in range(2):
        _exact(small_engine, ptr[:n], sz[:n], want)
    # the forms with fewer outputs
    terr = small_engine.verify_txns_ptrs(ptr[:n], sz[:n])
    assert np.array_equal(terr, want[0])
    terr, ttag, stag = small_engine.verify_txns_ptrs(ptr[:n], sz[:n], want_tags=True)
    assert np.array_equal(terr, want[0]) and np.array_equal(ttag, want[3]) and np.array_equal(stag, want[4])


def test_chunks_that_end_on_the_signature_slots(pool):
    """batch_max 64 with room for the bytes: five 12-signer payloads are 60
    slots and a sixth would make 72, so chunks of 5; mixed with one-signer
    payloads so that slot bases differ from chunk to chunk."""
    from firedancer_amd import ed25519
    idx = pool.twelve + pool.ones[:7] + pool.twelve[:6] + pool.mids[:9] + pool.twelve[3:]
    slots = [pool.exp.serr[i].size for i in idx]
    sz = _lens([pool.pays[i] for i in idx])
    chunks, i, on_slots = [], 0, 0
    while i < len(idx):
        c, _, ns = ed25519.txn_gather_layout(sz[i:], slots[i:], 64, 1 << 16)
        on_slots += i + c < len(idx) and c < 64 and ns + slots[i + c] > 64
        chunks.append(c)
        i += c
    assert chunks[:2] == [5, 5] and on_slots >= 5
    e = ed25519.Engine(device=0, batch_max=64, blob_max=1 << 16)
    a = Arena(sum(len(pool.pays[i]) + 64 for i in idx) + PAGE)
    try:
        ptr = [a.put(pool.pays[i], (3 * k) % 16) for k, i in enumerate(idx)]
        want = pool.exp.select(idx)
        blob, off, psz = _txn.pack([pool.pays[i] for i in idx])
        _same(e.verify_txns(blob, off, psz, want_sigs=True, want_tags=True), want)
        _exact(e, ptr, sz, want)
    finally:
        a.close()
        e.close()


# ---- 7. mixed stream and modes ----------------------------------------------------

def _mixed_batch(seed, count):
    """test_txn_gpu._mixed_batch: valid multi-signer transactions with bit
    flips in signatures and signer keys, header corruptions and truncations."""
    rng = np.random.default_rng(seed)
    pays, nsig = _txn.build_txns(seed, count)
    pays = [bytearray(p) for p in pays]
    for t in range(count):
        r = rng.random()
        n = int(nsig[t])
        m = 1 + 64 * n
        if r < 0.08:     # one signature bit
            pays[t][1 + int(rng.integers(0, 64 * n))] ^= 1 << int(rng.integers(0, 8))
        elif r < 0.14:   # a signer's public key (inside the message)
            pays[t][m + (1 if pays[t][m] & 0x80 else 0) + 4 + int(rng.integers(0, 32 * n))] ^= 0x04
        elif r < 0.18:   # the header: parse failure
            pays[t][m + (1 if pays[t][m] & 0x80 else 0)] ^= 0x40
        elif r < 0.20:   # truncated
            pays[t] = pays[t][:int(rng.integers(0, len(pays[t])))]
    return [bytes(p) for p in pays]


def test_mixed_stream_in_both_modes(engine, golden, pool):
    """600 mixed transactions and 20 one-signer ones carrying a golden
    s-window signature or a golden small-order signer key, unaligned in one
    arena.  Reference mode: the oracle's verdicts and verify_txns's tags;
    MODE_STRICT: every output of a strict engine's verify_txns, and the two
    modes differ on the golden ones."""
    from firedancer_amd import ed25519
    import _golden
    pays = _mixed_batch(41, 600)
    win = np.nonzero(golden.cls == _golden.CLASSES.index("s_window"))[0][:12]
    small = np.nonzero(golden.cls == _golden.CLASSES.index("small_order"))[0][::32][:8]   # one per torsion point
    assert win.size == 12 and small.size == 8 and len(set(bytes(golden.pub[g]) for g in small)) == 8
    for k, g in enumerate(win):
        p = bytearray(pool.pays[pool.ones[k]])
        p[1:65] = bytes(golden.sig[g])
        pays.append(bytes(p))
    for k, g in enumerate(small):
        p = bytearray(pool.pays[pool.ones[12 + k]])
        assert p[0] == 1
        a0 = 65 + (1 if p[65] & 0x80 else 0) + 4
        p[a0:a0 + 32] = bytes(golden.pub[g])
        pays.append(bytes(p))
    blob, off, sz = _txn.pack(pays)
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert set(np.unique(eterr).tolist()) >= {0, -3, -4}
    a = Arena(int(blob.size) + PAGE)
    strict = ed25519.Engine(device=0, batch_max=4096, blob_max=1 << 20, mode=ed25519.MODE_STRICT)
    try:
        a.put_at(3, blob)
        aoff = off.astype(np.uint64) + np.uint64(3)
        want = engine.verify_txns(blob, off, sz, want_sigs=True, want_tags=True)
        assert np.array_equal(want[0], eterr) and np.array_equal(want[1], ebase) and np.array_equal(want[2], eserr)
        got = engine.verify_txns_registered(a.mem, aoff, sz, want_sigs=True, want_tags=True)
        _same(got, want)
        swant = strict.verify_txns(blob, off, sz, want_sigs=True, want_tags=True)
        sgot = strict.verify_txns_registered(a.mem, aoff, sz, want_sigs=True, want_tags=True)
        _same(sgot, swant)
        assert (sgot[0][600:612] == -1).all() and (sgot[0][612:] != 0).all()
        assert (got[0][600:612] != -1).all() and (got[0][600:] != sgot[0][600:]).sum() >= 16
    finally:
        strict.close()
        a.close()
