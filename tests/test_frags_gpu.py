"""GPU: frag submissions (include/fd_tango_amd.h, "Frag submissions";
firedancer_amd/csrc/fd_ed25519_frags.h).

1  fd_ed25519_amd_frag_list_dev on the rings of tests/_frags.py: records and
   statuses against the model, every record address inside the region or the
   idle block, guards behind both planes, the mcache and the region unchanged.
2  list, a stream sync, two lines republished one lap ahead, then
   fd_ed25519_amd_frag_check_dev: exactly those two items become FRAG_SEQ.
3  fd_ed25519_amd_submit_frags against the parent's own path: the pointers
   fd_ed25519_amd_frags returns for the good items through
   submit_batch_registered, then the host rules keep / window keep / emit.
4  the argument errors, BUSY, the optional outputs, through the C ABI.
All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import _emit
import _frags
from _frags import BAD, SEQ
from test_emit_gpu import Extent, pattern

pytestmark = pytest.mark.gpu

OK, INVAL, BUSY = 0, -10, -12
CAP, SLOTS, BLOB = 256, 4, 256 * 1232
S8, S32, S64 = 0x55, 0x55555555, 0x5555555555555555
FM = _frags.FRAG_MAX
BOUND = _emit.sig_bound(FM - 96)
SHAPES = [(d, n) for d in (64, 256) for n in _frags.NS[d]]


def data_sz_for(n):
    return _frags.ru(64 * (22 * max(n, 4) + 8), _frags.PAGE)


class Reg:
    """A ring whose mcache and data region are each ONE registration."""

    def __init__(self, ring):
        from firedancer_amd import ed25519, hip
        self.ring = ring
        self._m8 = ring.mcache.view(np.uint8)
        ed25519.host_register(self._m8)
        ed25519.host_register(ring.region)
        self.d_mcache = hip.host_device_pointer(ring.mcache.ctypes.data)
        self.d_region = hip.host_device_pointer(ring.region.ctypes.data)

    def dev_src(self):
        from firedancer_amd import ed25519
        r = self.ring
        return ed25519.frag_src(r.mcache, r.region, r.frag_max, self.d_mcache, self.d_region)

    def close(self):
        from firedancer_amd import ed25519
        ed25519.host_unregister(self._m8)
        ed25519.host_unregister(self.ring.region)


# ---- 1, 2. the steps alone ---------------------------------------------------------------------------

class Planes:
    def __init__(self, n):
        from firedancer_amd import hip
        from _wsguard import Guarded
        self.n = n
        self.idle = hip.DeviceBuffer(256)
        self.idle.zero()
        self.rec, self.st = Guarded(32 * n), Guarded(n)
        self.reset()

    def reset(self):
        self.rec.fill(np.full(32 * self.n, 0xEE, np.uint8))
        self.st.fill(np.full(self.n, S8, np.uint8))

    def read(self):
        from firedancer_amd import ed25519
        self.rec.check("records")
        self.st.check("statuses")
        return self.rec.body(ed25519.GATHER_REC), self.st.body(np.int8)

    def free(self):
        self.rec.free()
        self.st.free()
        self.idle.free()


def check_list(reg, p, seq0, n):
    from firedancer_amd import ed25519, hip
    r = reg.ring
    before = r.snapshot()
    p.reset()
    ed25519.frag_list_dev(reg.dev_src(), seq0, n, p.idle.ptr, p.rec.ptr, p.st.ptr)
    hip.synchronize()
    rec, st = p.read()
    assert (st[n:] == S8).all() and (rec[n:].view(np.uint8) == 0xEE).all()      # nothing behind item n - 1
    rec, st = rec[:n], st[:n]
    ws, off, msz = _frags.rule(r.mcache, r.data_sz, r.frag_max, seq0, n)
    assert np.array_equal(st, ws), (st, ws)
    want = _frags.records(ws, off, msz, reg.d_region, p.idle.ptr, r.frag_max)
    for name, w in zip(("pub", "sig", "msg", "sz", "dst"), want):
        assert np.array_equal(rec[name], w), (name, np.nonzero(rec[name] != w)[0][:6])
    # every address: inside the region with its whole range, or the idle block
    lo, hi, idle = reg.d_region, reg.d_region + r.data_sz, p.idle.ptr
    for name, ln in (("pub", 32), ("sig", 64)):
        a = rec[name].astype(object)
        assert all((lo <= x and x + ln <= hi) or idle <= x <= idle + 32 for x in a), name
    for x, z in zip(rec["msg"].astype(object), rec["sz"].astype(object)):
        assert (z > 0 and lo <= x and x + z <= hi) or (z == 0 and x == idle)
    after = r.snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    return st


@pytest.mark.parametrize("depth,n", SHAPES)
def test_1_frag_list_dev(depth, n):
    for seq0 in _frags.seq0s(depth):
        ring = _frags.Ring(depth, seq0, data_sz_for(n))
        _frags.corpus(ring, n)
        reg, p = Reg(ring), Planes(n)
        try:
            st = check_list(reg, p, seq0, n)
            assert np.array_equal(st, _frags.expect_status(ring.kind))
            if n >= 33:
                assert {int(x) for x in st} == {0, SEQ, BAD}
                assert "flush_end" in ring.kind.values() and ring.kind[0] == "good"      # flush against both ends
            if n == depth and n > 1:
                check_list(reg, p, seq0 + 1, n - 1)             # the same lines from one item further
                check_list(reg, p, seq0 - 1, n)                 # and from one before: item 0 is a lap behind
        finally:
            p.free()
            reg.close()


def test_1_largest_frag_max_and_the_region_rule():
    """frag_max 65535: a 65535-byte frag is refused by the region alone and
    listed where the region holds it; dst strides by round_up( 65439, 16 )."""
    ring = _frags.Ring(64, 7, 2 * 65536, 65535)
    for i, (chunk, sz) in enumerate([(0, 65535), (1024, 65535), (1025, 65535), (2047, 64), (2046, 128)]):
        ring.put(i, chunk, sz)
    reg, p = Reg(ring), Planes(5)
    try:
        assert check_list(reg, p, 7, 5).tolist() == [0, 0, BAD, BAD, 0]
    finally:
        p.free()
        reg.close()


def test_1_dev_argument_errors():
    from firedancer_amd import ed25519
    ring = _frags.Ring(64, 0, data_sz_for(16))
    _frags.corpus(ring, 16)
    reg, p = Reg(ring), Planes(64)
    L = ed25519.lib()
    try:
        def lst(src=None, n=16, idle=p.idle.ptr, rec=p.rec.ptr, st=p.st.ptr):
            src = src if src is not None else reg.dev_src()
            return L.fd_ed25519_amd_frag_list_dev(ctypes.byref(src), 0, n, idle, rec, st, None)

        def src(**kw):
            s = reg.dev_src()
            for k, v in kw.items():
                setattr(s, k, v)
            return s
        assert lst(n=0) == OK
        for kw in (dict(n=65), dict(idle=None), dict(rec=None), dict(st=None), dict(rec=p.rec.ptr + 16), dict(idle=p.idle.ptr + 8),
                   dict(src=src(depth=48)), dict(src=src(depth=0)), dict(src=src(frag_max=95)), dict(src=src(frag_max=65536)),
                   dict(src=src(mcache=None)), dict(src=src(chunk0=None)), dict(src=src(mcache=reg.d_mcache + 16))):
            assert lst(**kw) == INVAL, kw
            assert L.fd_ed25519_amd_frag_check_dev(ctypes.byref(kw["src"]), 0, 16, p.st.ptr, None) == INVAL if "src" in kw else True
        assert L.fd_ed25519_amd_frag_check_dev(ctypes.byref(reg.dev_src()), 0, 16, None, None) == INVAL
        assert L.fd_ed25519_amd_frag_check_dev(ctypes.byref(reg.dev_src()), 0, 65, p.st.ptr, None) == INVAL
        from firedancer_amd import hip
        hip.synchronize()
        rec, st = p.read()
        assert (st.view(np.uint8) == S8).all() and (rec.view(np.uint8) == 0xEE).all()       # nothing was launched
    finally:
        p.free()
        reg.close()


@pytest.mark.parametrize("depth,n", [(64, 64), (256, 130)])
def test_2_recheck(depth, n):
    """The consumer's recheck without a race: between the two steps, with the
    stream idle, the host republishes two lines one lap ahead."""
    from firedancer_amd import ed25519, hip, tango
    seq0 = _frags.seq0s(depth)[1]
    ring = _frags.Ring(depth, seq0, data_sz_for(n))
    _frags.corpus(ring, n)
    reg, p = Reg(ring), Planes(n)
    try:
        st0 = check_list(reg, p, seq0, n)
        good = np.nonzero(st0 == 0)[0]
        lap = [int(good[1]), int(good[-1])]
        hip.synchronize()
        for i in lap:
            seq = (seq0 + i) & _frags.M64
            line = ring.mcache[seq & (depth - 1)]
            tango.publish(ring.mcache, (seq + depth) & _frags.M64, 1, int(line["chunk"]), int(line["sz"]), 0, 0, 0)
        rec0, _ = p.read()
        before = ring.snapshot()
        ed25519.frag_check_dev(reg.dev_src(), seq0, n, p.st.ptr)
        hip.synchronize()
        rec1, st1 = p.read()
        want = st0.copy()
        want[lap] = SEQ
        assert np.array_equal(st1, want), np.nonzero(st1 != want)[0]
        assert np.array_equal(rec0, rec1)
        after = ring.snapshot()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        p.free()
        reg.close()


# ---- 3. the engine -----------------------------------------------------------------------------------

class Signed:
    """A registered ring of depth 256 from a sequence number that wraps
    2^64, its items' own room filled with signed frags: of the good items
    every fifth has s >= L, every fifth a flipped message byte; items 4, 12,
    20, ... name the frag of the item three before them (in-batch duplicates).
    second( n1, n2 ) publishes items [n1, n1 + n2) naming the rooms of items
    [0, n2) with their true sizes."""

    def __init__(self, n):
        from firedancer_amd import ed25519
        self.seq0, self.n = (1 << 64) - 7, n
        r = self.ring = _frags.Ring(256, self.seq0, data_sz_for(256))
        spots = []
        _frags.corpus(r, n, lambda i, off, msz: spots.append((i, off, msz)))
        rng = np.random.default_rng(99)
        sizes = np.array([z for _, _, z in spots], np.uint32)
        offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint32)
        blob = rng.integers(0, 256, int(sizes.sum()) + 1, dtype=np.uint8)
        pub, sig = ed25519.sign_batch(rng.integers(0, 256, (len(spots), 32), dtype=np.uint8), blob, offs, sizes)
        for k, (i, off, msz) in enumerate(spots):
            f = np.concatenate((pub[k], sig[k], blob[int(offs[k]):int(offs[k]) + msz]))
            if i % 5 == 1:
                f[95] = 0xFF                                   # s >= L
            elif i % 5 == 3 and msz:
                f[96 + msz // 2] ^= 0x40
            r.region[off:off + f.size] = f
        for i in range(4, n, 8):
            if r.kind[i] == "good" and i - 3 in r.where:
                c, z = r.where[i - 3]
                r.put(i, c, 96 + z)
        self.reg = Reg(r)

    def second(self, n1, n2):
        r = self.ring
        for j in range(n2):
            c, z = r.where.get(j, (0, 0))
            r.put(n1 + j, c, 96 + z)

    def frame(self, off, msz):
        return b"".join(self.ring.frag(int(off), int(msz)))

    def close(self):
        self.reg.close()


@pytest.fixture(scope="module")
def world():
    w = Signed(256)
    yield w
    w.close()


@pytest.fixture(scope="module")
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ext():
    x = Extent(SLOTS * CAP * BOUND + 4096)
    yield x
    x.close()


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


def oracle(e, w, seq0, n, hostwin=None):
    """(err, tag, keep, frames of the kept items) by the parent's path: the
    host rule's pointers for the good items through submit_batch_registered,
    the statuses for the others, then the host survivor rule."""
    from firedancer_amd import ed25519
    r = w.ring
    good, st, pub, sig, msg, sz = ed25519.frags(r.mcache, r.region, seq0, n, r.frag_max)
    ws, off, msz = _frags.rule(r.mcache, r.data_sz, r.frag_max, seq0 & _frags.M64, n)
    assert np.array_equal(st, ws) and good == int((ws == 0).sum())
    g = np.nonzero(st == 0)[0]
    err, tag = st.copy(), np.zeros(n, np.uint64)
    if g.size:
        t = e.submit_batch_ptrs(pub[g], sig[g], msg[g], sz[g], want_tags=True)
        rt, (eg, tg) = e.wait()
        assert rt == t
        err[g], tag[g] = eg, tg
    keep = hostwin.keep(err, tag) if hostwin is not None else ed25519.keep(err, tag)
    return err, tag, keep, [w.frame(off[i], msz[i]) for i in keep]


def check_delivery(out, want, ext, lo, cap, what=""):
    err, tag, keep, frames = want
    assert out[0].dtype == np.int8 and np.array_equal(out[0], err), (what, np.nonzero(out[0] != err)[0][:8])
    assert out[1].dtype == np.uint64 and np.array_equal(out[1], tag), (what, np.nonzero(out[1] != tag)[0][:8])
    assert out[2].dtype == np.uint32 and np.array_equal(out[2], keep), (what, out[2], keep)
    off, sz = ext.check(lo, cap, frames, what)
    assert np.array_equal(out[3][0], off) and np.array_equal(out[3][1], sz), what


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
@pytest.mark.parametrize("n", _frags.NS[256])
def test_3_submit_frags(eng, world, ext, n, mode):
    e, w, r = eng, world, world.ring
    e.set_mode(mode)
    want = oracle(e, w, w.seq0, n)
    before = r.snapshot()
    ext.reset()
    cap, lo = n * BOUND, 128 * n
    t = e.submit_frags(r.mcache, r.region, w.seq0, n, want_tags=True, want_keep=True, emit=ext.view(lo, cap))
    rt, out = e.wait()
    assert rt == t
    check_delivery(out, want, ext, lo, cap, "n=%d" % n)
    after = r.snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    if n >= 130:
        err, tag, keep, _ = want
        assert {0, -1, -3, SEQ, BAD} <= {int(x) for x in err}                         # every class of item is there
        assert (tag[err < -3] == 0).all() and not set(np.nonzero(err)[0].tolist()) & set(keep.tolist())
        dups = [i for i in range(4, n, 8) if err[i] == 0 and err[i - 3] == 0]
        assert dups and not set(dups) & set(keep.tolist()) and all(tag[i] == tag[i - 3] for i in dups)


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_3_throughput_kernels(eng, world, ext, mode):
    """With the latency and small-batch kernels off the verdicts leave through
    the copy kernel, behind the override."""
    from firedancer_amd import ed25519
    e, w, r, n = eng, world, world.ring, 130
    try:
        ed25519.set_latency_batch_max(0)
        ed25519.set_small_batch_max(0)
        e.set_mode(mode)
        want = oracle(e, w, w.seq0, n)
        ext.reset()
        e.submit_frags(r.mcache, r.region, w.seq0, n, want_tags=True, want_keep=True, emit=ext.view(0, n * BOUND))
        check_delivery(e.wait()[1], want, ext, 0, n * BOUND, "throughput kernels")
    finally:
        ed25519.set_latency_batch_max(ed25519.LATENCY_BATCH_MAX_DEFAULT)
        ed25519.set_small_batch_max(ed25519.SMALL_BATCH_MAX_DEFAULT)


def test_3_optional_outputs(eng, world, ext):
    e, w, r, n = eng, world, world.ring, 65
    err, tag, keep, _ = oracle(e, w, w.seq0, n)
    ext.reset()
    e.submit_frags(r.mcache, r.region, w.seq0, n)
    e.submit_frags(r.mcache, r.region, w.seq0, n, want_tags=True)
    e.submit_frags(r.mcache, r.region, w.seq0, n, want_keep=True)
    a, b, c = e.wait()[1], e.wait()[1], e.wait()[1]
    assert np.array_equal(a, err) and np.array_equal(b[0], err) and np.array_equal(b[1], tag)
    assert len(c) == 2 and np.array_equal(c[0], err) and np.array_equal(c[1], keep) and ext.untouched()


def test_3_window_and_a_second_submission(eng, ext):
    """A window attached; the second submission, in flight beside the first,
    names the first one's frags again.  What the first published is filtered;
    an item the first refused as BAD or SEQ left no tag in the window, so its
    frag survives in the second."""
    from firedancer_amd import ed25519
    e = eng
    n1 = n2 = 100
    w = Signed(n1)
    dev, host = ed25519.Window(0, CAP), ed25519.Window(-1, CAP)
    try:
        w.second(n1, n2)
        r = w.ring
        plain1 = oracle(e, w, w.seq0, n1)                       # no window: the in-batch rule alone
        want1 = oracle(e, w, w.seq0, n1, host)
        want2 = oracle(e, w, w.seq0 + n1, n2, host)
        assert np.array_equal(plain1[2], want1[2])              # an empty window filters nothing more
        e.set_window(dev)
        ext.reset()
        cap = n1 * BOUND
        lo2 = _frags.ru(cap, 4096)
        t1 = e.submit_frags(r.mcache, r.region, w.seq0, n1, want_tags=True, want_keep=True, emit=ext.view(0, cap))
        t2 = e.submit_frags(r.mcache, r.region, w.seq0 + n1, n2, want_tags=True, want_keep=True, emit=ext.view(lo2, cap))
        assert e.in_flight == 2 and t2 == t1 + 1
        (r1, o1), (r2, o2) = e.wait(), e.wait()
        assert (r1, r2) == (t1, t2)
        image = pattern(ext.size)
        for o, wnt, lo in ((o1, want1, 0), (o2, want2, lo2)):
            assert np.array_equal(o[0], wnt[0]) and np.array_equal(o[1], wnt[1]) and np.array_equal(o[2], wnt[2])
            off, sz = _emit.lay(wnt[3], image[lo:lo + cap], cap)
            assert np.array_equal(o[3][0], off) and np.array_equal(o[3][1], sz)
        assert np.array_equal(ext.mem, image)
        err1, err2, k1, k2 = want1[0], want2[0], set(want1[2].tolist()), set(want2[2].tolist())
        again = [j for j in range(n2) if j in k1 and r.kind[j] == "good" and j % 8 != 4]
        assert again and not set(again) & k2                    # published by the first: filtered from the second
        fresh = [j for j in range(n2) if err1[j] in (SEQ, BAD) and j in r.where and err2[j] == 0]
        assert {int(err1[j]) for j in fresh} == {SEQ, BAD} and set(fresh) <= k2
        assert np.array_equal(dev.export(), host.export())
    finally:
        while e.in_flight:
            e.wait()
        e.set_window(None)
        dev.close()
        host.close()
        w.close()


def test_3_four_in_flight_mixed_with_pointer_submissions(eng, world, ext):
    """Frag and pointer submissions interleaved, four in flight, polled in order."""
    import time
    from firedancer_amd import ed25519
    e, w, r = eng, world, world.ring
    spans = [(0, 130), (7, 65), (130, 17), (3, 256 - 3)]
    wants = [oracle(e, w, w.seq0 + a, n) for a, n in spans]
    good, st, pub, sig, msg, sz = ed25519.frags(r.mcache, r.region, w.seq0, 256, r.frag_max)
    g = np.nonzero(st[:spans[0][1]] == 0)[0]                   # the pointer submissions: the first span's good items
    ext.reset()
    los = [0, CAP * BOUND]
    tk = [e.submit_frags(r.mcache, r.region, w.seq0 + spans[0][0], spans[0][1], want_tags=True, want_keep=True,
                         emit=ext.view(los[0], spans[0][1] * BOUND)),
          e.submit_batch_ptrs(pub[g], sig[g], msg[g], sz[g], want_tags=True, want_keep=True),
          e.submit_frags(r.mcache, r.region, w.seq0 + spans[1][0], spans[1][1], want_tags=True, want_keep=True,
                         emit=ext.view(los[1], spans[1][1] * BOUND)),
          e.submit_batch_ptrs(pub[g], sig[g], msg[g], sz[g], want_tags=True, want_keep=True)]
    assert e.in_flight == 4 and tk == list(range(tk[0], tk[0] + 4))
    with pytest.raises(ed25519.EngineBusy):
        e.submit_frags(r.mcache, r.region, w.seq0, 1)
    got, deadline = [], time.monotonic() + 20.0
    while len(got) < 4:
        x = e.poll()
        if x is not None:
            got.append(x)
        assert time.monotonic() < deadline
    assert [t for t, _ in got] == tk
    image = pattern(ext.size)
    for k, j in ((0, 0), (2, 1)):
        o, wnt, cap = got[k][1], wants[j], spans[j][1] * BOUND
        assert np.array_equal(o[0], wnt[0]) and np.array_equal(o[1], wnt[1]) and np.array_equal(o[2], wnt[2])
        off, sz = _emit.lay(wnt[3], image[los[j]:los[j] + cap], cap)
        assert np.array_equal(o[3][0], off) and np.array_equal(o[3][1], sz)
    assert np.array_equal(ext.mem, image)
    for k in (1, 3):
        assert np.array_equal(got[k][1][0], wants[0][0][g]) and np.array_equal(got[k][1][1], wants[0][1][g])
    # the other two spans, one at a time
    for (a, n), wnt in zip(spans[2:], wants[2:]):
        ext.reset()
        e.submit_frags(r.mcache, r.region, w.seq0 + a, n, want_tags=True, want_keep=True, emit=ext.view(0, n * BOUND))
        check_delivery(e.wait()[1], wnt, ext, 0, n * BOUND, "span %d+%d" % (a, n))


# ---- 4. the C call: argument errors, BUSY, optional outputs -------------------------------------------

class Raw:
    """One fd_ed25519_amd_submit_frags call through the C ABI, every output prefilled."""

    def __init__(self, e, n):
        self.e, self.n = e, n
        self.err, self.tag = np.full(n, S8, np.int8), np.full(n, S64, np.uint64)
        self.keep, self.cnt = np.full(n, S32, np.uint32), np.full(1, S64, np.uint64)
        self.eoff, self.esz = np.full(n + 1, S64, np.uint64), np.full(n, S32, np.uint32)
        self.ticket = ctypes.c_ulong(99)

    def submit(self, src, seq0, out=None, cap=0, n=None, eng=True, err=True, tag=True, keep=True, cnt=True, eoff=None, esz=None,
               ticket=True):
        from firedancer_amd import ed25519
        P = ed25519._ptr
        eoff = (out is not None) if eoff is None else eoff
        esz = (out is not None) if esz is None else esz
        return ed25519.lib().fd_ed25519_amd_submit_frags(
            self.e._h if eng else None, ctypes.byref(src) if src is not None else None, seq0 & _frags.M64,
            self.n if n is None else n, P(self.err) if err else None, P(self.tag) if tag else None, P(self.keep) if keep else None,
            P(self.cnt) if cnt else None, ctypes.c_void_p(out) if out else None, cap, P(self.eoff) if eoff else None,
            P(self.esz) if esz else None, ctypes.byref(self.ticket) if ticket else None)

    def untouched(self):
        return bool((self.err == S8).all() and (self.tag == S64).all() and (self.keep == S32).all() and (self.cnt == S64).all()
                    and (self.eoff == S64).all() and (self.esz == S32).all() and self.ticket.value == 99)


def host_src(w, **kw):
    from firedancer_amd import ed25519
    r = w.ring
    s = ed25519.frag_src(r.mcache, r.region, r.frag_max)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_4_argument_errors(eng, world, ext):
    from firedancer_amd import ed25519, tango
    e, w, r, n = eng, world, world.ring, 65
    ext.reset()
    base, need = ext.mem.ctypes.data, n * BOUND
    t0 = e.submit_frags(r.mcache, r.region, w.seq0, 1)
    e.wait()
    flight = [e.submit_frags(r.mcache, r.region, w.seq0, 1)]                  # one in flight throughout
    big = _frags.Ring(512, 0, 8192)                                           # depth above batch_max
    loose = _frags.Ring(64, 0, 8192)                                          # registered nowhere
    two = _frags.aligned(4 * 4096)                                            # two adjacent registrations
    m8 = big.mcache.view(np.uint8)
    ed25519.host_register(m8)
    ed25519.host_register(two[:8192])
    ed25519.host_register(two[8192:])
    try:
        cases = [
            dict(eng=False), dict(src=None), dict(err=False), dict(ticket=False), dict(n=0),
            dict(src=host_src(w, depth=64), n=65),                             # n > depth
            dict(src=host_src(w, mcache=big.mcache.ctypes.data, depth=512), n=CAP + 1, big=True),      # n > batch_max
            dict(src=host_src(w, depth=48)), dict(src=host_src(w, depth=0)),
            dict(src=host_src(w, frag_max=95)), dict(src=host_src(w, frag_max=65536)),
            dict(src=host_src(w, frag_max=65535), n=5),                        # 5 * 65440 > blob_max
            dict(src=host_src(w, mcache=None)), dict(src=host_src(w, chunk0=None)), dict(src=host_src(w, data_sz=0)),
            dict(src=host_src(w, mcache=r.mcache.ctypes.data + 16)),           # lines are 32-aligned
            dict(src=host_src(w, mcache=loose.mcache.ctypes.data, depth=64), n=16),
            dict(src=host_src(w, chunk0=loose.region.ctypes.data, data_sz=8192)),
            dict(src=host_src(w, depth=512)),                                  # the lines run past their registration
            dict(src=host_src(w, data_sz=r.data_sz + 64)),                     # so does the region
            dict(src=host_src(w, chunk0=r.region.ctypes.data - 64)),
            dict(src=host_src(w, chunk0=two.ctypes.data + 4096, data_sz=8192)),    # across two registrations
            dict(cnt=False), dict(keep=False),                                 # keep and keep_cnt: both or neither
            dict(out=base, cap=need, keep=False, cnt=False),                   # frames without keep
            dict(out=base, cap=need, eoff=False), dict(out=base, cap=need, esz=False), dict(out=base, cap=0), dict(cap=need),
            dict(out=base + 32, cap=need),                                     # out is 64-aligned
            dict(out=base, cap=need - 1),                                      # the bound, not the data, decides
            dict(out=two.ctypes.data + 8192 - 64, cap=need),
        ]
        for kw in cases:
            kw = dict(kw)
            x = Raw(e, CAP + 1 if kw.pop("big", False) else n)
            src = kw.pop("src", host_src(w))
            assert x.submit(src, w.seq0, **kw) == INVAL, kw
            assert x.untouched() and ext.untouched() and e.in_flight == 1, kw
        # each of these one step inside the limit is accepted
        ok = Raw(e, 4)
        assert ok.submit(host_src(w, frag_max=65535), w.seq0, n=4, keep=False, cnt=False) == OK
        ok2 = Raw(e, n)
        assert ok2.submit(host_src(w, chunk0=two.ctypes.data + 8192, data_sz=8192), w.seq0, out=base, cap=need) == OK
        assert ok.ticket.value == flight[0] + 1 and ok2.ticket.value == flight[0] + 2      # the refusals consumed no ticket
        assert flight[0] == t0 + 1
    finally:
        while e.in_flight:
            e.wait()
        ed25519.host_unregister(m8)
        ed25519.host_unregister(two[:8192])
        ed25519.host_unregister(two[8192:])
    st = _frags.rule(r.mcache, 8192, FM, w.seq0, n)[0]                                    # over the small region most lines are BAD
    assert np.array_equal(ok2.err[st != 0], st[st != 0]) and int((st == BAD).sum()) > n // 2
    assert (ok2.tag[st != 0] == 0).all() and not set(np.nonzero(st)[0].tolist()) & set(ok2.keep[:int(ok2.cnt[0])].tolist())


def test_4_busy_comes_after_the_argument_checks(eng, world, ext):
    e, w, r = eng, world, world.ring
    ext.reset()
    for _ in range(SLOTS):
        e.submit_frags(r.mcache, r.region, w.seq0, 16)
    assert e.in_flight == SLOTS
    x = Raw(e, 16)
    assert x.submit(host_src(w), w.seq0, keep=False) == INVAL and x.untouched()
    assert x.submit(host_src(w, depth=48), w.seq0) == INVAL and x.untouched()
    assert x.submit(host_src(w), w.seq0) == BUSY and x.untouched() and e.in_flight == SLOTS
    last = 0
    for _ in range(SLOTS):
        last = e.wait()[0]
    assert x.submit(host_src(w), w.seq0) == OK and x.ticket.value == last + 1
    e.wait()


def test_4_outputs_through_the_c_call(eng, world, ext):
    """tag NULL, keep NULL, emit NULL, and all of them: nothing is written
    before the wait that reports the ticket, nothing at or beyond keep_cnt
    after it, and the extent's guard behind out_cap holds."""
    e, w, r, n = eng, world, world.ring, 130
    err, tag, keep, frames = oracle(e, w, w.seq0, n)
    ext.reset()
    cap = n * BOUND
    a, b, c, d = (Raw(e, n) for _ in range(4))
    assert a.submit(host_src(w), w.seq0, tag=False, keep=False, cnt=False) == OK
    assert b.submit(host_src(w), w.seq0, keep=False, cnt=False) == OK
    assert c.submit(host_src(w), w.seq0) == OK
    assert d.submit(host_src(w), w.seq0, out=ext.mem.ctypes.data + 4096, cap=cap) == OK
    tk = [x.ticket.value for x in (a, b, c, d)]
    assert tk == list(range(tk[0], tk[0] + 4)) and e.in_flight == 4
    for x in (a, b, c, d):
        x.ticket.value = 99
        assert x.untouched()
    for t in tk:
        assert e.wait()[0] == t
    for x in (a, b, c, d):
        assert np.array_equal(x.err, err)
    assert (a.tag == S64).all() and all(np.array_equal(x.tag, tag) for x in (b, c, d))
    assert all((x.keep == S32).all() and (x.cnt == S64).all() for x in (a, b))
    k = int(keep.size)
    for x in (c, d):
        assert int(x.cnt[0]) == k and np.array_equal(x.keep[:k], keep) and (x.keep[k:] == S32).all() and 0 < k < n
    assert (c.eoff == S64).all() and (c.esz == S32).all()
    off, sz = ext.check(4096, cap, frames, "C call")
    assert np.array_equal(d.eoff[:k + 1], off) and (d.eoff[k + 1:] == S64).all()
    assert np.array_equal(d.esz[:k], sz) and (d.esz[k:] == S32).all()
