"""GPU: fd_ed25519_amd_verify_batch_registered -- the pointer-array batch whose
records a kernel (k_gather) fetches from registered host memory.

The inputs are valid signatures fresh from sign_batch, and every call asks for
the dedup tags: the tag is SHA-512(R || A || M)[0:8], so a single wrong
gathered byte of R, A or M shows twice, as a -3 verdict and as a tag that
differs from ed25519.tag's (host code, hashlib-equal: test_tags_cpu.py).  A
wrong byte of s shows as a verdict.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import _golden
import _oracle
import _strict_ref

pytestmark = pytest.mark.gpu

ALIGNS = [0, 1, 2, 3, 5, 8, 13, 15]
SIZES = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 111, 112, 113, 127, 128, 129, 255, 256, 1231, 1232]
ERR_INVAL = -10


class Arena:
    """A page-aligned block of host memory, 0xA5-filled, registered with
    host_register (one registration).  put() lays a byte string at the next
    16-aligned slot + `align`, at least 16 filler bytes after the previous one."""

    def __init__(self, nbytes, register=True):
        from firedancer_amd import ed25519
        nbytes = (nbytes + 4095) & ~4095
        self._raw = np.zeros(nbytes + 4096, np.uint8)
        o = (-self._raw.ctypes.data) % 4096
        self.mem = self._raw[o:o + nbytes]
        self.mem[:] = 0xA5
        self.base = int(self.mem.ctypes.data)
        self.size = nbytes
        self.pos = 0
        self._registered = register
        if register:
            ed25519.host_register(self.mem)

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
        if self._registered:
            ed25519.host_unregister(self.mem)
            self._registered = False


class Pool:
    """n valid signatures (fresh keys), their reference verdicts and tags."""

    def __init__(self, sizes, seed):
        from firedancer_amd import ed25519
        rng = np.random.default_rng(seed)
        self.sz = np.asarray(sizes, np.uint32)
        n = self.sz.size
        self.off = np.concatenate([[0], np.cumsum(self.sz)[:-1]]).astype(np.uint32)
        self.blob = rng.integers(0, 256, int(self.sz.sum()) + 1, dtype=np.uint8)
        self.pub, self.sig = ed25519.sign_batch(rng.integers(0, 256, (n, 32), dtype=np.uint8), self.blob, self.off, self.sz)
        b = _golden.Batch(self.pub, self.sig, self.off, self.sz, self.blob)
        self.err = _oracle.verify_batch(b)
        self.tag = np.array([ed25519.tag(b.msg(i), self.sig[i], self.pub[i]) for i in range(n)], np.uint64)
        self.batch = b
        for a in (self.sz, self.off, self.blob, self.pub, self.sig, self.err, self.tag):
            a.setflags(write=False)

    def msg(self, i):
        return self.batch.msg(i)


def _mixed_sizes(n, seed):
    """The edge sizes in turn, with runs of 1232-B messages (a blob_max of 4096 then holds 3 per chunk)."""
    rng = np.random.default_rng(seed)
    sz = [SIZES[i % len(SIZES)] for i in range(n)]
    for start in range(7, n, 40):
        run = int(rng.integers(3, 9))
        sz[start:start + run] = [1232] * len(sz[start:start + run])
    return sz


@pytest.fixture(scope="module")
def pool():
    """4096 signatures, mixed sizes, all valid: shared by the tests below, computed once."""
    p = Pool(_mixed_sizes(4096, 11), 20262)
    assert not p.err.any(), "a fresh valid signature the reference rejects: pick another seed"
    return p


@pytest.fixture(scope="module")
def pool_arena(pool):
    """Every pool record in one registered arena, pub | sig | msg apart, 16-aligned: (arena, pub, sig, msg addresses)."""
    a = Arena(int(pool.sz.sum()) + len(pool.sz) * (96 + 3 * 32) + 4096)
    pp = np.array([a.put(pool.pub[i]) for i in range(len(pool.sz))], np.uint64)
    sp = np.array([a.put(pool.sig[i]) for i in range(len(pool.sz))], np.uint64)
    mp = np.array([a.put(pool.msg(i)) for i in range(len(pool.sz))], np.uint64)
    yield a, pp, sp, mp
    a.close()


@pytest.fixture(scope="module")
def small_engine():
    """64 signatures and 4096 message bytes per chunk, two slots."""
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=64, blob_max=4096)
    yield e
    e.close()


def _bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return int(bad.size), [(int(i), int(want[i]), int(got[i])) for i in bad[:6]]


def _exact(e, pp, sp, mp, sz, want_err, want_tag):
    err, tag = e.verify_batch_ptrs(pp, sp, mp, sz, want_tags=True)
    assert err.dtype == np.int8 and tag.dtype == np.uint64 and err.shape == tag.shape == (len(pp),)
    assert np.array_equal(err, want_err), _bad(err, want_err)
    assert np.array_equal(tag, want_tag), _bad(tag, want_tag)


# ---- 1. alignment x size ----------------------------------------------------------

def test_every_alignment_of_every_pointer_at_every_edge_size(engine):
    """Each of pub, sig and msg swept over the byte alignments mod 16 while
    the other two sit at 0, and two all-odd cases, times the edge sizes."""
    combos = [(a, 0, 0) for a in ALIGNS] + [(0, a, 0) for a in ALIGNS[1:]] + [(0, 0, a) for a in ALIGNS[1:]]
    combos += [(1, 3, 5), (15, 13, 1)]
    cases = [(c, s) for c in combos for s in SIZES]
    p = Pool([s for _, s in cases], 31)
    assert not p.err.any()
    a = Arena(int(p.sz.sum()) + len(cases) * 256)
    try:
        pp, sp, mp = [], [], []
        for i, ((ap, as_, am), _) in enumerate(cases):
            pp.append(a.put(p.pub[i], ap))
            sp.append(a.put(p.sig[i], as_))
            mp.append(a.put(p.msg(i), am))
        pp, sp, mp = (np.array(x, np.uint64) for x in (pp, sp, mp))
        assert sorted(set(int(x) % 16 for x in pp)) == ALIGNS and sorted(set(int(x) % 16 for x in mp)) == ALIGNS
        before = a.mem.copy()
        _exact(engine, pp, sp, mp, p.sz, p.err, p.tag)
        assert np.array_equal(a.mem, before)               # the kernel only reads caller memory
    finally:
        a.close()


# ---- 2. registration edges --------------------------------------------------------

def test_records_flush_against_both_ends_of_a_registration(engine):
    """pub at the first byte of a page-aligned registration; a message that
    ends at the last byte of a registration whose size is a multiple of 4096
    (k_gather loads only aligned 16-B words holding a byte of the range, so
    neither reaches a page outside it: fd_ed25519_gather.h)."""
    p = Pool([200, 333, 1, 0], 32)
    assert not p.err.any()
    a = Arena(2 * 4096)
    try:
        assert a.base % 4096 == 0 and a.size % 4096 == 0
        pp = [a.put_at(0, p.pub[0]), a.put_at(512, p.pub[1]), a.put_at(600, p.pub[2]), a.put_at(700, p.pub[3])]
        sp = [a.put_at(1024 + 80 * k, p.sig[k]) for k in range(4)]
        mp = [a.put_at(2048, p.msg(0)), a.put_at(a.size - 333, p.msg(1)), a.put_at(a.size - 334, p.msg(2)), a.base + a.size - 1]
        assert pp[0] == a.base and mp[1] + 333 == a.base + a.size
        _exact(engine, np.array(pp, np.uint64), np.array(sp, np.uint64), np.array(mp, np.uint64), p.sz, p.err, p.tag)
        # and a signature / a key that end at the last byte
        sp[0] = a.put_at(a.size - 64, p.sig[0])
        _exact(engine, np.array(pp[:1], np.uint64), np.array(sp[:1], np.uint64), np.array(mp[:1], np.uint64), p.sz[:1],
               p.err[:1], p.tag[:1])
        pp[0] = a.put_at(a.size - 32, p.pub[0])
        sp[0] = a.put_at(0, p.sig[0])
        _exact(engine, np.array(pp[:1], np.uint64), np.array(sp[:1], np.uint64), np.array(mp[:1], np.uint64), p.sz[:1],
               p.err[:1], p.tag[:1])
    finally:
        a.close()


# ---- 3. pointer sources -----------------------------------------------------------

def test_two_registrations_shared_message_and_repeats(engine, pool):
    from firedancer_amd import ed25519
    n = 60
    a, b = Arena(64 * 1024), Arena(64 * 1024)
    try:
        # interleaved: even records in a, odd ones in b, and each record's parts in different arenas every third time
        pp, sp, mp = [], [], []
        for i in range(n):
            x, y = (a, b) if i % 2 == 0 else (b, a)
            pp.append(x.put(pool.pub[i], i % 16))
            sp.append((y if i % 3 == 0 else x).put(pool.sig[i], (3 * i) % 16))
            mp.append(x.put(pool.msg(i), (5 * i) % 16))
        idx = list(range(n)) + [4, 4, 17, 4]               # the same records listed again
        sel = lambda v: np.array([v[i] for i in idx], np.uint64)
        _exact(engine, sel(pp), sel(sp), sel(mp), pool.sz[idx], pool.err[idx], pool.tag[idx])

        # one message signed by 19 keys
        rng = np.random.default_rng(33)
        msg = rng.integers(0, 256, 177, dtype=np.uint8)
        pub, sig = ed25519.sign_batch(rng.integers(0, 256, (19, 32), dtype=np.uint8), msg, np.zeros(19, np.uint32),
                                      np.full(19, 177, np.uint32))
        m = a.put(msg, 7)
        pp = np.array([b.put(pub[k], k % 16) for k in range(19)], np.uint64)
        sp = np.array([b.put(sig[k], (k + 9) % 16) for k in range(19)], np.uint64)
        want = np.array([ed25519.tag(msg, sig[k], pub[k]) for k in range(19)], np.uint64)
        _exact(engine, pp, sp, np.full(19, m, np.uint64), np.full(19, 177, np.uint64), np.zeros(19, np.int8), want)
    finally:
        a.close()
        b.close()


# ---- 4. frag layout ---------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_frags(golden):
    """Every golden vector as a frag pub | sig | msg at a 64-B aligned offset of one registered arena."""
    n = len(golden)
    a = Arena(int(golden.msg_sz.sum()) + n * (96 + 64) + 4096)
    base = np.zeros(n, np.uint64)
    o = 0
    for i in range(n):
        base[i] = a.put_at(o, bytes(golden.pub[i]) + bytes(golden.sig[i]) + golden.msg(i))
        o = (o + 96 + int(golden.msg_sz[i]) + 63) & ~63
    yield a, base
    a.close()


def test_golden_vectors_as_frags_in_order_and_permuted(engine, golden, golden_frags):
    _, base = golden_frags
    n = len(golden)
    assert n == 2046
    ref_err, ref_tag = engine.verify_batch([golden.msg(i) for i in range(n)], [bytes(s) for s in golden.sig],
                                           [bytes(p) for p in golden.pub], want_tags=True)
    assert np.array_equal(ref_err, golden.expect)
    perm = np.random.default_rng(34).permutation(n)
    for idx in (np.arange(n), perm):
        b = base[idx]
        _exact(engine, b, b + np.uint64(32), b + np.uint64(96), golden.msg_sz[idx], golden.expect[idx], ref_tag[idx])


# ---- 5. refusals ------------------------------------------------------------------

def test_refusals_leave_outputs_untouched_and_the_engine_usable(small_engine, pool, pool_arena):
    from firedancer_amd import ed25519
    e = small_engine
    _, pp, sp, mp = pool_arena
    n = 10
    sz = pool.sz[:n].astype(np.uint64)
    assert sz[5] > 0
    plain = Arena(8192, register=False)                    # ordinary memory, never registered
    big = Arena(3 * 4096)
    try:
        up, us, um = plain.put(pool.pub[5]), plain.put(pool.sig[5]), plain.put(pool.msg(5))
        one_past = big.put_at(big.size - int(sz[5]) + 1, pool.msg(5)[:-1])   # its last byte would lie one past the registration
        inside = big.put_at(0, bytes(4097))

        def refused(pub=None, sig=None, msg=None, size=None):
            p, s, m, z = pp[:n].copy(), sp[:n].copy(), mp[:n].copy(), sz.copy()
            if pub is not None:
                p[5] = pub
            if sig is not None:
                s[5] = sig
            if msg is not None:
                m[5] = msg
            if size is not None:
                z[5] = size
            err, tag = np.full(n, 0x55, np.int8), np.full(n, 0x5555555555555555, np.uint64)
            rc = ed25519.lib().fd_ed25519_amd_verify_batch_registered_tag(e._h, n, ed25519._ptr(m), ed25519._ptr(z),
                                                                          ed25519._ptr(s), ed25519._ptr(p),
                                                                          ed25519._ptr(err), ed25519._ptr(tag))
            assert rc == ERR_INVAL
            assert (err == 0x55).all() and (tag == 0x5555555555555555).all()
            with pytest.raises(ed25519.EngineError):
                e.verify_batch_ptrs(p, s, m, z, want_tags=True, err=err, tags=tag)
            assert (err == 0x55).all() and (tag == 0x5555555555555555).all()
            _exact(e, pp[:n], sp[:n], mp[:n], sz, pool.err[:n], pool.tag[:n])   # the next valid call is exact

        refused(pub=up)
        refused(sig=us)
        refused(msg=um)
        refused(msg=one_past)
        refused(msg=inside, size=4097)                     # in registered memory, but larger than blob_max = 4096
        refused(msg=0)                                     # NULL with sz > 0
        refused(pub=0)
        refused(sig=0)
        # control: the same edits that stay legal are accepted (the last byte AT the end; NULL with sz = 0)
        at_end = big.put_at(big.size - int(sz[5]), pool.msg(5))
        m = mp[:n].copy()
        m[5] = at_end
        _exact(e, pp[:n], sp[:n], m, sz, pool.err[:n], pool.tag[:n])
    finally:
        plain.close()
        big.close()


def test_null_message_with_size_zero_is_accepted(small_engine):
    p = Pool([0, 5, 0], 35)
    a = Arena(4096)
    try:
        pp = np.array([a.put(p.pub[i]) for i in range(3)], np.uint64)
        sp = np.array([a.put(p.sig[i]) for i in range(3)], np.uint64)
        mp = np.array([0, a.put(p.msg(1), 3), 0], np.uint64)
        _exact(small_engine, pp, sp, mp, p.sz, p.err, p.tag)
    finally:
        a.close()


# ---- 6. chunking ------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_chunks_keep_caller_order_and_reuse_the_slots(small_engine, pool, pool_arena, n):
    """batch_max 64, blob_max 4096: count-bound chunks and, in the runs of
    1232-B messages, blob-bound chunks of 3; twice, so both slots are reused."""
    from firedancer_amd import ed25519
    _, pp, sp, mp = pool_arena
    # 130 small messages (64 of them pad to <= 3072 B: chunks end at the count), then runs of 1232 B between mixed sizes
    small = np.nonzero(pool.sz <= 33)[0]
    big = np.nonzero(pool.sz == 1232)[0]
    mid = np.nonzero((pool.sz > 33) & (pool.sz < 1232))[0]
    order = np.concatenate([small[:130], big[:10], mid[:20], big[10:17], small[130:163]])
    assert order.size == 200
    idx = order[:n]
    sz = pool.sz[idx]
    chunks, i = [], 0
    while i < n:
        c, _ = ed25519.gather_layout(sz[i:], 64, 4096)
        chunks.append(c)
        i += c
    assert chunks[0] == min(n, 64)
    if n == 200:
        assert chunks[:2] == [64, 64] and chunks.count(3) >= 3 and len(chunks) > 8   # more chunks than slots: reuse within a call
    for _ in range(2):
        _exact(small_engine, pp[idx], sp[idx], mp[idx], sz, pool.err[idx], pool.tag[idx])


# ---- 7. kernel paths and modes ----------------------------------------------------

def test_default_policy_latency_path(engine, pool, pool_arena):
    """n = 512: k_front and a latency DSM kernel on the gathered planes, verdicts written in place."""
    _, pp, sp, mp = pool_arena
    _exact(engine, pp[:512], sp[:512], mp[:512], pool.sz[:512], pool.err[:512], pool.tag[:512])


@pytest.mark.parametrize("kernel", ["k_dsm", "k_dsmp"])
def test_throughput_kernels(engine, pool, pool_arena, kernel):
    from firedancer_amd import ed25519
    _, pp, sp, mp = pool_arena
    n = 1000
    try:
        ed25519.select_dsm_kernel(kernel)
        _exact(engine, pp[:n], sp[:n], mp[:n], pool.sz[:n], pool.err[:n], pool.tag[:n])
    finally:
        ed25519.select_dsm_kernel("default")


def test_strict_mode_over_the_golden_frags(engine, golden, golden_frags):
    from firedancer_amd import ed25519
    _, base = golden_frags
    want = np.array(_strict_ref.verify_batch(golden), np.int8)
    assert (want != golden.expect).any()
    try:
        engine.set_mode(ed25519.MODE_STRICT)
        err = engine.verify_batch_ptrs(base, base + np.uint64(32), base + np.uint64(96), golden.msg_sz)
        assert np.array_equal(err, want), _bad(err, want)
    finally:
        engine.set_mode(ed25519.MODE_REFERENCE)


# ---- 8. mixed stream --------------------------------------------------------------

def test_mixed_stream_equals_verify_batch_and_the_oracle(engine, pool):
    """4096 signatures, one in ten with a single flipped bit (in pub, sig or
    msg): the same pointer arrays through verify_batch and through the
    gathered call, and the CPU oracle on the same bytes."""
    from firedancer_amd import ed25519
    n = len(pool.sz)
    rng = np.random.default_rng(36)
    pub, sig, blob = pool.pub.copy(), pool.sig.copy(), pool.blob.copy()
    hit = rng.choice(n, n // 10, replace=False)
    for i in hit:
        part = int(rng.integers(0, 3)) if pool.sz[i] else int(rng.integers(0, 2))
        bit = np.uint8(1 << int(rng.integers(0, 8)))
        if part == 0:
            pub[i, int(rng.integers(0, 32))] ^= bit
        elif part == 1:
            sig[i, int(rng.integers(0, 64))] ^= bit
        else:
            blob[int(pool.off[i]) + int(rng.integers(0, pool.sz[i]))] ^= bit
    b = _golden.Batch(pub, sig, pool.off, pool.sz, blob)
    want = _oracle.verify_batch(b)
    assert (want[hit] != 0).all() and not want[np.setdiff1d(np.arange(n), hit)].any()
    a = Arena(int(pool.sz.sum()) + n * 200 + 4096)
    try:
        pp = np.array([a.put(pub[i], i % 16) for i in range(n)], np.uint64)
        sp = np.array([a.put(sig[i], (7 * i) % 16) for i in range(n)], np.uint64)
        mp = np.array([a.put(b.msg(i), (11 * i) % 16) for i in range(n)], np.uint64)
        sz = pool.sz.astype(np.uint64)
        err0, tag0 = np.zeros(n, np.int8), np.zeros(n, np.uint64)
        P = ed25519._ptr
        rc = ed25519.lib().fd_ed25519_amd_verify_batch_tag(engine._h, n, ctypes.cast(P(mp), ed25519.c_void_pp),
                                                           ctypes.cast(P(sz), ed25519.c_ulong_p),
                                                           ctypes.cast(P(sp), ed25519.c_void_pp),
                                                           ctypes.cast(P(pp), ed25519.c_void_pp), P(err0), P(tag0))
        assert rc == 0
        assert np.array_equal(err0, want), _bad(err0, want)
        _exact(engine, pp, sp, mp, sz, want, tag0)
    finally:
        a.close()
