"""GPU: the survivors' output frames (include/fd_ed25519_amd.h, "Output
frames"; firedancer_amd/csrc/fd_ed25519_emit.h).

1  fd_ed25519_amd_emit_dev on synthetic planes: every message size at every
   source residue, four keep lists, the whole output region (a pattern, and a
   guard behind out_cap) byte for byte against the model of tests/_emit.py.
2  fd_txn_amd_emit_dev behind fd_txn_amd_parse_packed_dev.
3  the two signature _emit submissions, 4 the two transaction ones (window,
   several in flight), 5 the argument errors, 6 emit arguments NULL.
All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import _emit
from test_async_gpu import Sigs, Txns
from test_keep_gpu import SigBatch, TxnBatch

pytestmark = pytest.mark.gpu

OK, INVAL = 0, -10
CAP, SLOTS, BLOB = 256, 4, 256 * 1232
S8, S32, S64 = 0x55, 0x55555555, 0x5555555555555555
PAGE = 4096
NS = (1, 63, 64, 65, 130)
KEEPS = ("all", "none", "third", "last")


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.uint64) * 37 + 11) & 0xFF).astype(np.uint8)


def keep_of(kind, n):
    return {"all": list(range(n)), "none": [], "third": list(range(0, n, 3)), "last": [n - 1]}[kind]


# ---- 1. emit_dev -------------------------------------------------------------------------------------

def sig_planes(n, rot):
    """n items of random bytes: item i has message size MSG_SIZES[(i + rot) %
    11] and its message starts at residue (7 i + rot) % 16 of the blob; the
    key and signature planes start rot % 16 bytes into their buffers."""
    rng = np.random.default_rng(1000 + 17 * n + rot)
    sizes = [_emit.MSG_SIZES[(i + rot) % len(_emit.MSG_SIZES)] for i in range(n)]
    res = [(7 * i + rot) % 16 for i in range(n)]
    pub = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    off, at = [], 0
    for z, r in zip(sizes, res):
        at = (at + 15) // 16 * 16 + 16 + r
        off.append(at)
        at += z
    blob = rng.integers(0, 256, at + 32, dtype=np.uint8)
    msgs = [bytes(blob[o:o + z]) for o, z in zip(off, sizes)]
    frames = [_emit.sig_frame(bytes(pub[i]), bytes(sig[i]), msgs[i]) for i in range(n)]
    return pub, sig, np.array(off, np.uint32), np.array(sizes, np.uint32), blob, frames, set(zip(sizes, res))


class DevRun:
    """The guarded device buffers of emit_dev / txn_emit_dev calls over at most
    n items and region bytes of output; run() makes one call and checks every
    byte the call may and may not write."""

    def __init__(self, n, region, in_bytes):
        from firedancer_amd import ed25519
        from _wsguard import Guarded
        self.n, self.region = n, region
        self.fp = ed25519.emit_scratch_footprint(n)
        assert self.fp % 256 == 0 and self.fp > 0
        self.g = {"keep": Guarded(4 * n), "cnt": Guarded(8), "out": Guarded(region), "eoff": Guarded(8 * (n + 1)),
                  "esz": Guarded(4 * n), "scr": Guarded(self.fp)}
        self.g.update({k: Guarded(v) for k, v in in_bytes.items()})

    def run(self, call, n, keep, cnt, frames, out_cap, what):
        """call( g, out_cap ) launches on the buffers g; keep: d_keep's n
        entries; cnt: *d_keep_cnt; frames: the model's frame per keep entry
        below min( cnt, n )."""
        from firedancer_amd import hip
        g = self.g
        k = np.full(self.n, 0xFFFFFFFF, np.uint32)
        k[:len(keep)] = keep
        g["keep"].fill(k)
        g["cnt"].fill(np.array([cnt], np.uint64))
        g["out"].fill(pattern(self.region))
        g["eoff"].fill(np.full(self.n + 1, S64, np.uint64))
        g["esz"].fill(np.full(self.n, S32, np.uint32))
        g["scr"].fill(np.full(self.fp, 0xFF, np.uint8))
        call(g, out_cap)
        hip.synchronize()
        c = min(cnt, n)
        assert len(frames) == c
        want = pattern(self.region)
        off, sz = _emit.lay(frames, want[:out_cap], out_cap)
        eoff, esz, out = g["eoff"].body(np.uint64), g["esz"].body(np.uint32), g["out"].body()
        assert np.array_equal(eoff[:c + 1], off) and (eoff[c + 1:] == S64).all(), (what, eoff[:c + 2], off)
        assert np.array_equal(esz[:c], sz) and (esz[c:] == S32).all(), what
        bad = np.nonzero(out != want)[0]
        assert bad.size == 0, (what, int(bad.size), bad[:8], out[bad[:8]], want[bad[:8]])
        for name, b in g.items():
            b.check(what + " " + name)
        return off

    def free(self):
        for b in self.g.values():
            b.free()


def _sig_call(n, shift):
    from firedancer_amd import ed25519

    def call(g, out_cap):
        ed25519.emit_dev(n, g["pub"].ptr + shift, g["sig"].ptr + shift, g["off"].ptr, g["sz"].ptr, g["blob"].ptr, g["keep"].ptr,
                         g["cnt"].ptr, g["out"].ptr, out_cap, g["eoff"].ptr, g["esz"].ptr, g["scr"].ptr)
    return call


def _sig_fill(r, n, rot):
    pub, sig, off, sz, blob, frames, combos = sig_planes(n, rot)
    shift = rot % 16
    for name, a, room in (("pub", pub, 32 * n + 16), ("sig", sig, 64 * n + 16), ("blob", blob, r.g["blob"].nbytes)):
        img = np.full(room, 0xEE, np.uint8)
        o = shift if name != "blob" else 0
        img[o:o + a.size] = a.reshape(-1)
        r.g[name].fill(img)
    r.g["off"].fill(off)
    r.g["sz"].fill(sz)
    return frames, shift, combos


@pytest.mark.parametrize("kind", KEEPS)
@pytest.mark.parametrize("n", NS)
def test_1_emit_dev(n, kind):
    """Every message size at every one of the 16 source residues (16 turns,
    the planes rotated each turn); the WHOLE region against the model laid
    over the pattern: the frames, the zero tails, every untouched byte, and
    the 256-B guard behind out_cap."""
    cap = sum(_emit.sig_bound(1232) for _ in range(n))
    r = DevRun(n, cap + 256, {"pub": 32 * n + 16, "sig": 64 * n + 16, "off": 4 * n, "sz": 4 * n, "blob": (1232 + 48) * n + 64})
    seen = set()
    try:
        for rot in range(16):
            frames, shift, combos = _sig_fill(r, n, rot)
            seen |= combos
            keep = keep_of(kind, n)
            off = r.run(_sig_call(n, shift), n, keep, len(keep), [frames[i] for i in keep], cap, "n%d %s rot%d" % (n, kind, rot))
            assert int(off[-1]) <= cap
        if n >= 63:
            assert seen == {(z, q) for z in _emit.MSG_SIZES for q in range(16)}
    finally:
        r.free()


def test_1_emit_dev_capacity_and_bounds():
    """out_cap one stride short: the last frame is absent and d_emit_off is
    complete.  keep_cnt == 0: only emit_off[0] is written.  *d_keep_cnt above
    n is clamped; an index >= n is a frame of size 0 and nothing is read for
    it; out_cap == 0 with d_out NULL computes the layout."""
    from firedancer_amd import ed25519, hip
    n = 65
    cap = n * _emit.sig_bound(1232)
    r = DevRun(n, cap + 256, {"pub": 32 * n + 16, "sig": 64 * n + 16, "off": 4 * n, "sz": 4 * n, "blob": (1232 + 48) * n + 64})
    try:
        frames, shift, _ = _sig_fill(r, n, 5)
        call = _sig_call(n, shift)
        keep = list(range(n))
        off, sz = _emit.place(frames)
        short = int(off[-1]) - 128
        assert int(off[n - 1]) <= short < int(off[n])
        got = r.run(call, n, keep, n, frames, short, "one stride short")
        assert np.array_equal(got, off)
        r.run(call, n, keep, 0, [], cap, "keep_cnt 0")
        r.run(call, n, keep, n + 1000, frames, cap, "keep_cnt clamped")
        wild = [3, n, 0xFFFFFFFE, 7, 1 << 31, n - 1]
        r.run(call, n, wild, len(wild), [frames[i] if i < n else b"" for i in wild], cap, "indices >= n")
        # layout only
        g = r.g
        g["eoff"].fill(np.full(n + 1, S64, np.uint64))
        g["keep"].fill(np.arange(n, dtype=np.uint32))
        g["cnt"].fill(np.array([n], np.uint64))
        ed25519.emit_dev(n, g["pub"].ptr + shift, g["sig"].ptr + shift, g["off"].ptr, g["sz"].ptr, g["blob"].ptr, g["keep"].ptr,
                         g["cnt"].ptr, None, 0, g["eoff"].ptr, g["esz"].ptr, g["scr"].ptr)
        hip.synchronize()
        assert np.array_equal(g["eoff"].body(np.uint64), off) and np.array_equal(g["esz"].body(np.uint32), sz)
        # refusals, before anything launches
        with pytest.raises(ed25519.EngineError, match="rc=-10"):
            ed25519.emit_dev(n, g["pub"].ptr, g["sig"].ptr, g["off"].ptr, g["sz"].ptr, g["blob"].ptr, g["keep"].ptr, g["cnt"].ptr,
                             g["out"].ptr + 32, cap, g["eoff"].ptr, g["esz"].ptr, g["scr"].ptr)      # d_out not 64-aligned
        with pytest.raises(ed25519.EngineError, match="rc=-10"):
            ed25519.emit_dev(n, g["pub"].ptr, g["sig"].ptr, g["off"].ptr, g["sz"].ptr, g["blob"].ptr, g["keep"].ptr, None,
                             g["out"].ptr, cap, g["eoff"].ptr, g["esz"].ptr, g["scr"].ptr)
        assert ed25519.emit_scratch_footprint((1 << 30) + 1) == 0
    finally:
        r.free()


# ---- 2. txn_emit_dev ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def txn_set():
    """The CPU test's payloads with a rejected one among them."""
    pays = list(_emit.txn_payloads().values())
    junk = bytes(range(7, 207))
    assert _emit.oracle_desc(junk) == b""
    return pays[:3] + [junk] + pays[3:]


@pytest.mark.parametrize("kind", KEEPS)
def test_2_txn_emit_dev(txn_set, kind):
    """Behind fd_txn_amd_parse_packed_dev, payloads at odd offsets: the model
    over the descriptors that call left (which are the oracle's)."""
    from firedancer_amd import ed25519, hip
    from _wsguard import Guarded
    pays = txn_set
    n = len(pays)
    off, at = [], 1
    for p in pays:
        off.append(at)
        at += len(p) + (2 if (at + len(p)) % 2 else 1)          # the next one at an odd offset again
    assert all(o % 2 == 1 for o in off)
    blob = np.full(at + 16, 0xEE, np.uint8)
    for o, p in zip(off, pays):
        blob[o:o + len(p)] = np.frombuffer(p, np.uint8)
    dcap = sum(_emit.desc_bound(len(p)) for p in pays)
    cap = sum(max(_emit.txn_bound(len(p)), _emit.ru(_emit.ru(len(p), 16) + 2, 128)) for p in pays)
    r = DevRun(n, cap + 256, {"blob": blob.size, "toff": 4 * n, "tsz": 4 * n})
    x = {"fp": Guarded(4 * n), "doff": Guarded(8 * (n + 1)), "desc": Guarded(dcap),
         "pscr": Guarded(ed25519.txn_parse_packed_scratch_footprint(n))}
    try:
        r.g["blob"].fill(blob)
        r.g["toff"].fill(np.array(off, np.uint32))
        r.g["tsz"].fill(np.array([len(p) for p in pays], np.uint32))
        ed25519.txn_parse_packed_dev(n, r.g["blob"].ptr, r.g["toff"].ptr, r.g["tsz"].ptr, x["fp"].ptr, x["doff"].ptr, x["desc"].ptr,
                                     dcap, x["pscr"].ptr)
        hip.synchronize()
        doff, desc = x["doff"].body(np.uint64), x["desc"].body()
        descs = [bytes(desc[int(doff[i]):int(doff[i + 1])]) for i in range(n)]
        assert descs == [_emit.oracle_desc(p) for p in pays] and descs[3] == b"" and len(descs[-1]) == 3570
        frames = [_emit.txn_frame(p, d) for p, d in zip(pays, descs)]

        def call(g, out_cap):
            ed25519.txn_emit_dev(n, g["blob"].ptr, g["toff"].ptr, g["tsz"].ptr, x["doff"].ptr, x["desc"].ptr, g["keep"].ptr,
                                 g["cnt"].ptr, g["out"].ptr, out_cap, g["eoff"].ptr, g["esz"].ptr, g["scr"].ptr)
        keep = keep_of(kind, n)
        got = r.run(call, n, keep, len(keep), [frames[i] for i in keep], cap, "txn " + kind)
        if kind == "all":
            short = int(got[-1]) - 128                           # one stride short: the MTU frame is absent
            r.run(call, n, keep, n, frames, short, "txn one stride short")
            wild = [n - 1, n, 2, 0xFFFFFFFF, 3]
            r.run(call, n, wild, len(wild), [frames[i] if i < n else b"" for i in wild], cap, "txn indices >= n")
        for name, b in x.items():
            b.check("txn " + name)
    finally:
        r.free()
        for b in x.values():
            b.free()


# ---- 3 - 6. the submit forms -------------------------------------------------------------------------

class Extent:
    """Page-aligned host memory in ONE registration, filled with the pattern;
    check( lo, cap, frames ) compares the whole registration with the model
    laid over the pattern at [lo, lo + cap)."""

    def __init__(self, nbytes, register=True):
        from firedancer_amd import ed25519
        nbytes = (nbytes + PAGE - 1) & ~(PAGE - 1)
        self._raw = np.zeros(nbytes + PAGE, np.uint8)
        o = (-self._raw.ctypes.data) % PAGE
        self.mem = self._raw[o:o + nbytes]
        self.size, self.registered = nbytes, register
        self.reset()
        if register:
            ed25519.host_register(self.mem)

    def reset(self):
        self.mem[:] = pattern(self.size)

    def view(self, lo, cap):
        assert lo % 64 == 0 and lo + cap <= self.size
        return self.mem[lo:lo + cap]

    def check(self, lo, cap, frames, what=""):
        want = pattern(self.size)
        off, sz = _emit.lay(frames, want[lo:lo + cap], cap)
        bad = np.nonzero(self.mem != want)[0]
        assert bad.size == 0, (what, int(bad.size), bad[:8], self.mem[bad[:8]], want[bad[:8]])
        return off, sz

    def untouched(self):
        return bool((self.mem == pattern(self.size)).all())

    def close(self):
        from firedancer_amd import ed25519
        if self.registered:
            ed25519.host_unregister(self.mem)


@pytest.fixture(scope="module")
def sb():
    s = Sigs()
    b = SigBatch(s)
    b.frames = [_emit.sig_frame(b.pubs[i], b.sigs[i], b.msgs[i]) for i in range(b.n)]
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
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=CAP, blob_max=BLOB, nslot=SLOTS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ext():
    x = Extent(CAP * _emit.txn_bound(1232))
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


def _same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), (k, np.nonzero(a != b)[0][:6])


def _sig_emit(e, b, ext, mode, registered, at_end=False):
    """1, 65 and 200 signatures (valid, corrupted and duplicate items) through
    the _keep and the _emit form: every other output equal, the extent the
    model over the delivered keep, emit_off / emit_sz the model's."""
    e.set_mode(mode)
    for n in (1, 65, 200):
        cap = sum(_emit.sig_bound(len(m)) for m in b.msgs[:n])
        lo = ext.size - cap if at_end else 128 * n              # at_end: out + out_cap at the registration's last byte
        assert lo % 64 == 0
        ext.reset()
        t0 = b.submit(e, n, registered, want_tags=True, want_keep=True)
        t1 = b.submit(e, n, registered, want_tags=True, want_keep=True, emit=ext.view(lo, cap))
        (r0, plain), (r1, full) = e.wait(), e.wait()
        assert (r0, r1) == (t0, t1) and t1 == t0 + 1
        _same(full[:3], plain)
        keep = full[2]
        off, sz = ext.check(lo, cap, [b.frames[i] for i in keep], "n=%d" % n)
        eoff, esz = full[3]
        assert eoff.dtype == np.uint64 and esz.dtype == np.uint32
        assert np.array_equal(eoff, off) and np.array_equal(esz, sz)
        if n > 1:
            assert 0 < keep.size < n and 1 in keep and 0 not in keep and 2 not in keep      # corrupted, valid, duplicate


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_3_signature_forms(eng, sb, ext, mode, registered):
    _sig_emit(eng, sb, ext, mode, registered)


def test_3_signature_forms_device_planes(eng, sb, ext):
    """With the latency and small-batch kernels off the staged form copies its
    planes to the device first: the frames are then read from device planes,
    above from the slot's mapped staging."""
    from firedancer_amd import ed25519
    try:
        ed25519.set_latency_batch_max(0)
        ed25519.set_small_batch_max(0)
        _sig_emit(eng, sb, ext, ed25519.MODE_REFERENCE, False)
        _sig_emit(eng, sb, ext, ed25519.MODE_STRICT, True)
    finally:
        ed25519.set_latency_batch_max(ed25519.LATENCY_BATCH_MAX_DEFAULT)
        ed25519.set_small_batch_max(ed25519.SMALL_BATCH_MAX_DEFAULT)


def test_3_extent_at_the_end_of_its_registration(eng, sb, ext):
    from firedancer_amd import ed25519
    _sig_emit(eng, sb, ext, ed25519.MODE_REFERENCE, True, at_end=True)


def _txn_frames(e, b, n, registered):
    """The model's frames of b's first n transactions, from the descriptors
    the plain want_desc submission returns."""
    b.submit(e, n, registered, want_desc=True)
    _, (terr, doff, desc) = e.wait()
    return [_emit.txn_frame(b.pays[i], bytes(desc[int(doff[i]):int(doff[i + 1])])) for i in range(n)]


@pytest.mark.parametrize("registered", [False, True], ids=["staged", "registered"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "strict"])
def test_4_transaction_forms(eng, tb, ext, mode, registered):
    """Both forms, with and without desc: the _keep call's outputs, the
    extent the model over the delivered keep."""
    e, b = eng, tb
    e.set_mode(mode)
    for n in (1, 65, b.full):
        frames = _txn_frames(e, b, n, registered)
        cap = sum(_emit.txn_bound(len(p)) for p in b.pays[:n])
        for kw in (dict(want_sigs=True, want_tags=True, want_desc=True), dict()):
            ext.reset()
            t0 = b.submit(e, n, registered, want_keep=True, **kw)
            t1 = b.submit(e, n, registered, want_keep=True, emit=ext.view(0, cap), **kw)
            (r0, plain), (r1, full) = e.wait(), e.wait()
            assert (r0, r1) == (t0, t0 + 1) and t1 == t0 + 1
            _same(full[:-1], plain)
            keep = full[-2]
            off, sz = ext.check(0, cap, [frames[i] for i in keep], "n=%d %s" % (n, sorted(kw)))
            assert np.array_equal(full[-1][0], off) and np.array_equal(full[-1][1], sz)
            if n > 1:
                assert keep[:1].tolist() == [1] and 4 not in keep and keep.size > 1
                assert all(len(frames[i]) > len(b.pays[i]) + 20 for i in keep)                 # a descriptor in every frame


def test_4_window_two_in_flight(eng, tb, ext):
    """A window attached, two submissions in flight, the second repeating
    items of the first: its frames are the window's survivors' only."""
    from firedancer_amd import ed25519
    e, b = eng, tb
    frames = _txn_frames(e, b, 60, True)
    win = ed25519.Window(0, CAP)
    e.set_window(win)
    try:
        ext.reset()
        cap0 = sum(_emit.txn_bound(len(p)) for p in b.pays[:40])
        cap1 = sum(_emit.txn_bound(len(p)) for p in b.pays[20:60])
        lo1 = _emit.ru(cap0, PAGE)
        t0 = e.submit_txns_ptrs(b.ptr[:40], b.sz[:40], want_keep=True, emit=ext.view(0, cap0))
        t1 = e.submit_txns_ptrs(b.ptr[20:60], b.sz[20:60], want_keep=True, emit=ext.view(lo1, cap1))
        assert e.in_flight == 2
        (r0, a), (r1, c) = e.wait(), e.wait()
        assert (r0, r1) == (t0, t1)
        k0, k1 = a[1], c[1]
        again = set(int(i) - 20 for i in k0 if i >= 20)          # the second submission's items the first published
        assert len(again) > 0 and not (again & set(k1.tolist())) and k1.size > 0 and int(k1.min()) >= 20
        want = pattern(ext.size)
        o0, z0 = _emit.lay([frames[i] for i in k0], want[:cap0], cap0)
        o1, z1 = _emit.lay([frames[20 + i] for i in k1], want[lo1:lo1 + cap1], cap1)
        assert np.array_equal(ext.mem, want)
        assert np.array_equal(a[2][0], o0) and np.array_equal(a[2][1], z0)
        assert np.array_equal(c[2][0], o1) and np.array_equal(c[2][1], z1)
    finally:
        while e.in_flight:
            e.wait()
        e.set_window(None)
        win.close()


def test_4_four_in_flight(eng, tb, ext):
    """Four submissions in flight on distinct extents, delivered in ticket order."""
    e, b = eng, tb
    frames = _txn_frames(e, b, 100, True)
    ext.reset()
    spans = [(0, 30), (30, 65), (5, 100), (64, 65)]
    los, caps, lo = [], [], 0
    for i0, i1 in spans:
        caps.append(sum(_emit.txn_bound(len(p)) for p in b.pays[i0:i1]))
        los.append(lo)
        lo = _emit.ru(lo + caps[-1], 64)
    tk = [e.submit_txns_ptrs(b.ptr[i0:i1], b.sz[i0:i1], want_keep=True, emit=ext.view(l, c))
          for (i0, i1), l, c in zip(spans, los, caps)]
    assert e.in_flight == 4 and tk == list(range(tk[0], tk[0] + 4))
    want = pattern(ext.size)
    for k, (i0, i1) in enumerate(spans):
        r, out = e.wait()
        assert r == tk[k]
        off, sz = _emit.lay([frames[i0 + i] for i in out[1]], want[los[k]:los[k] + caps[k]], caps[k])
        assert np.array_equal(out[2][0], off) and np.array_equal(out[2][1], sz) and out[1].size > 0
    assert np.array_equal(ext.mem, want)


FORMS = ("batch", "batch_registered", "txns", "txns_registered")


class Raw:
    """One submission through a C _emit call, its outputs prefilled with 0x55."""

    def __init__(self, form, b, n, e):
        from firedancer_amd import ed25519
        self.form, self.n, self.e, self.L, self.P = form, n, e, ed25519.lib(), ed25519._ptr
        self.err, self.tag = np.full(n, S8, np.int8), np.full(n, S64, np.uint64)
        self.keep, self.cnt = np.full(n, S32, np.uint32), np.full(1, S64, np.uint64)
        self.eoff, self.esz = np.full(n + 1, S64, np.uint64), np.full(n, S32, np.uint32)
        self.ticket = ctypes.c_ulong(99)
        if form.startswith("batch"):
            self._keepalive = [a[:n].copy() for a in (b.mp, b.sz, b.sp, b.pp)]
            self._in = [self.P(a) for a in self._keepalive]
            self.need = sum(_emit.sig_bound(int(z)) for z in b.sz[:n])
        else:
            self.need = sum(_emit.txn_bound(int(z)) for z in b.sz[:n])
            if form == "txns":
                self._keepalive = [b.blob, b.off[:n].copy(), b.sz32[:n].copy()]
                self._in = [self.P(a) for a in self._keepalive] + [int(b.blob.size)]
            else:
                self._keepalive = [b.ptr[:n].copy(), b.sz[:n].copy()]
                self._in = [self.P(a) for a in self._keepalive]

    def submit(self, out, cap, keep=True, cnt=True, eoff=True, esz=True, suffix="_emit"):
        P = self.P
        mid = (P(self.err), P(self.tag)) if self.form.startswith("batch") else (P(self.err), None, None, P(self.tag), None, None, None, 0)
        tail = (P(self.keep) if keep else None, P(self.cnt) if cnt else None)
        if suffix == "_emit":
            tail += (ctypes.c_void_p(out) if out else None, cap, P(self.eoff) if eoff else None, P(self.esz) if esz else None)
        return getattr(self.L, "fd_ed25519_amd_submit_" + self.form + suffix)(self.e._h, self.n, *self._in, *mid, *tail,
                                                                               ctypes.byref(self.ticket))

    def untouched(self):
        return bool((self.err == S8).all() and (self.tag == S64).all() and (self.keep == S32).all() and (self.cnt == S64).all()
                    and (self.eoff == S64).all() and (self.esz == S32).all() and self.ticket.value == 99)


def _refused(form, b, e, ext, **kw):
    """The call returns INVAL; every output and the extent are untouched,
    nothing is in flight and no ticket is consumed."""
    r = Raw(form, b, 65, e)
    out = kw.pop("out", ext.mem.ctypes.data)
    cap = kw.pop("cap", r.need)
    assert r.submit(out, cap, **kw) == INVAL, (form, kw)
    assert r.untouched() and ext.untouched() and e.in_flight == 0


def _tickets_are_consecutive(e, b, ext, form, before):
    r = Raw(form, b, 65, e)
    assert r.submit(ext.mem.ctypes.data, r.need) == OK and r.ticket.value == before + 1
    e.wait()
    return r


def _a_ticket(e, b):
    r = Raw("batch_registered", b, 1, e)
    assert r.submit(None, 0, suffix="_keep") == OK
    e.wait()
    return int(r.ticket.value)


def _b(form, sb, tb):
    return sb if form.startswith("batch") else tb


@pytest.mark.parametrize("form", FORMS)
def test_5_any_of_the_four_without_the_others(eng, sb, tb, ext, form):
    b = _b(form, sb, tb)
    ext.reset()
    t = _a_ticket(eng, sb)
    base = ext.mem.ctypes.data
    for kw in (dict(out=None), dict(cap=0), dict(eoff=False), dict(esz=False),                     # one missing
               dict(cap=0, eoff=False, esz=False), dict(out=None, eoff=False, esz=False),           # one alone
               dict(out=None, cap=0, esz=False), dict(out=None, cap=0, eoff=False)):
        _refused(form, b, eng, ext, **dict(dict(out=base), **kw))
    _tickets_are_consecutive(eng, b, ext, form, t)


@pytest.mark.parametrize("form", FORMS)
def test_5_emit_without_keep(eng, sb, tb, ext, form):
    b = _b(form, sb, tb)
    ext.reset()
    t = _a_ticket(eng, sb)
    _refused(form, b, eng, ext, keep=False, cnt=False)
    _tickets_are_consecutive(eng, b, ext, form, t)


@pytest.mark.parametrize("form", FORMS)
def test_5_out_not_64_aligned(eng, sb, tb, ext, form):
    b = _b(form, sb, tb)
    ext.reset()
    t = _a_ticket(eng, sb)
    for d in (1, 16, 32, 63):
        _refused(form, b, eng, ext, out=ext.mem.ctypes.data + d)
    _tickets_are_consecutive(eng, b, ext, form, t)


@pytest.mark.parametrize("form", FORMS)
def test_5_extent_not_in_one_registration(eng, sb, tb, ext, form):
    """Memory that is not registered; an extent that runs past the end of its
    registration; two adjacent registrations, which do not make one range."""
    from firedancer_amd import ed25519
    b = _b(form, sb, tb)
    ext.reset()
    t = _a_ticket(eng, sb)
    need = Raw(form, b, 65, eng).need
    loose = Extent(need, register=False)
    _refused(form, b, eng, ext, out=loose.mem.ctypes.data)
    assert loose.untouched()
    _refused(form, b, eng, ext, out=ext.mem.ctypes.data + ext.size - need + 64)                     # 64 bytes past the end
    _refused(form, b, eng, ext, out=ext.mem.ctypes.data - 64)                                       # 64 bytes before the start
    half = _emit.ru(need, 2 * PAGE) // 2
    two = Extent(2 * half, register=False)
    ed25519.host_register(two.mem[:half])
    ed25519.host_register(two.mem[half:])
    try:
        assert need > half
        _refused(form, b, eng, ext, out=two.mem.ctypes.data + 2 * half - _emit.ru(need, 64), cap=_emit.ru(need, 64))
        assert two.untouched()
        r = Raw(form, b, 1, eng)                                                                    # inside the second one: fine
        assert r.need <= half and r.submit(two.mem.ctypes.data + half, r.need) == OK
        eng.wait()
        t += 1
    finally:
        ed25519.host_unregister(two.mem[:half])
        ed25519.host_unregister(two.mem[half:])
    _tickets_are_consecutive(eng, b, ext, form, t)


@pytest.mark.parametrize("form", FORMS)
def test_5_out_cap_below_the_bound_sum(eng, sb, tb, ext, form):
    """The capacity is decided by the bound, never by the data: one byte
    below the sum is refused although the survivors' frames would fit."""
    b = _b(form, sb, tb)
    ext.reset()
    t = _a_ticket(eng, sb)
    r = Raw(form, b, 65, eng)
    _refused(form, b, eng, ext, cap=r.need - 1)
    r = _tickets_are_consecutive(eng, b, ext, form, t)
    assert int(r.eoff[int(r.cnt[0])]) < r.need - 1


@pytest.mark.parametrize("form", FORMS)
def test_6_emit_arguments_null(eng, sb, tb, ext, form):
    """All four NULL / 0 is exactly the _keep call; nothing is written before
    the wait that reports the ticket, and nothing beyond emit_off[keep_cnt] /
    emit_sz[keep_cnt) after it."""
    b = _b(form, sb, tb)
    ext.reset()
    a, c, d = (Raw(form, b, 65, eng) for _ in range(3))
    assert a.submit(None, 0, suffix="_keep") == OK
    assert c.submit(None, 0, eoff=False, esz=False) == OK
    assert d.submit(ext.mem.ctypes.data, d.need) == OK
    assert c.ticket.value == a.ticket.value + 1 and d.ticket.value == a.ticket.value + 2
    a.ticket.value = c.ticket.value = d.ticket.value = 99
    assert a.untouched() and c.untouched() and d.untouched() and eng.in_flight == 3
    for _ in range(3):
        eng.wait()
    for x in (c, d):
        assert np.array_equal(x.err, a.err) and np.array_equal(x.tag, a.tag)
        assert np.array_equal(x.keep, a.keep) and np.array_equal(x.cnt, a.cnt)
    assert (c.eoff == S64).all() and (c.esz == S32).all()
    k = int(d.cnt[0])
    assert 0 < k < 65 and (d.eoff[k + 1:] == S64).all() and (d.esz[k:] == S32).all() and (d.keep[k:] == S32).all()
    assert int(d.eoff[0]) == 0 and (np.diff(d.eoff[:k + 1].astype(np.int64)) == (d.esz[:k].astype(np.int64) + 127) // 128 * 128).all()
