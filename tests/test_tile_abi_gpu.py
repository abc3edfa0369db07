"""The streaming verify tile (include/fd_tango_amd.h) where a producer or a
caller can put it and the rest of the suite never does: frags the size guard
must refuse (both framings, copy and zero copy), a zero-copy run whose
in_chunk0 is not the mapped region's base and frags at that region's end, and
runs whose input and output sequences start anywhere in 64 bits -- across
2^63 (the sign of the tile's signed compares) and across the wrap -- with and
without output flow control.

Expected behaviour is modelled frag by frag in Python (_model below): verdicts
from the committed golden vectors and the CPU oracle, tags from hashlib, the
tcache window of FD_TCACHE_INSERT, sequence arithmetic in Python integers
reduced mod 2^64.  Nothing is compared against the tile's own output."""
import collections
import ctypes
import hashlib
import threading
import time

import numpy as np
import pytest

import _oracle
from test_tile_gpu import _pool, _txn_tag

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MSG_MAX = 1232
BAD_SIZES = (0, 1, 95, 96 + MSG_MAX + 1, 1408, 1409, 65535)     # PUB_SIG_MSG: below 96, above 96 + 1232
SLACK = 1 << 16      # bytes after the last frag: a refused frag's nominal bytes are ordinary host memory
SENTINEL = 99        # verdict-log entries no run wrote


def _sdiff(a, b):
    """a - b as a signed 64-bit distance."""
    d = (a - b) & M64
    return d - (1 << 64) if d >> 63 else d


class Frag:
    """One input frag: pool entry k (a well-formed pub | sig | msg frag), or
    raw bytes published with a size the tile must refuse (k None)."""

    def __init__(self, k=None, sz=None, data=b""):
        self.k, self.sz, self.data = k, sz, data


def _frag_bytes(pool, k):
    pub, sig, msgs, _ = pool
    return bytes(pub[k]) + bytes(sig[k]) + msgs[k]


def _packed_bytes(pool, frags, skip=()):
    """Bytes the compact chunk advance takes for frags (those in skip excepted)."""
    return 64 * sum((((len(f.data[:1536] if f.k is None else _frag_bytes(pool, f.k)) + 127) >> 7) << 1)
                    for i, f in enumerate(frags) if i not in skip)


def _feed(pool, frags, depth, seq0=0, lead=0, min_size=0, place=None):
    """Publish `frags` as sequence numbers seq0, seq0+1, ... (mod 2^64) into a
    fresh mcache whose first lap starts at seq0, and lay their bytes out in a
    page-aligned data region: `lead` unused bytes, the frags (compact chunk
    advance, chunk indices relative to the byte after the lead), SLACK bytes
    (the region holds min_size bytes at least).  place: {frag index: chunk}
    puts those frags at chunks of the caller's choice instead; a refused
    frag placed so gets no bytes.  ctl and tsorig vary per frag.  Returns
    (mcache, region, chunk0 view, per-frag (chunk, sz, ctl, tsorig))."""
    from firedancer_amd import tango
    place = place or {}
    stored = [f.data[:1536] if f.k is None else _frag_bytes(pool, f.k) for f in frags]
    need = _packed_bytes(pool, frags, place)
    nbytes = (max(lead + need + SLACK, min_size) + 4095) & ~4095
    region = tango._aligned(nbytes, 4096)
    chunk0 = region[lead:]
    mc = tango.mcache_new(depth, seq0)
    chunk, meta = 0, []
    for i, (f, b) in enumerate(zip(frags, stored)):
        sz = len(b) if f.k is not None else f.sz
        c = place.get(i, chunk)
        if not (i in place and f.k is None):
            chunk0[64 * c:64 * c + len(b)] = np.frombuffer(b, np.uint8)
        ctl = (0x9e37 * i + (i >> 3)) & 0xFFFF          # 0 at i = 0, every bit used
        tso = (1000 + 7 * i) & 0xFFFFFFFF
        tango.publish(mc, (seq0 + i) & M64, 0, c, sz, ctl, tso, 0)
        meta.append((c, sz, ctl, tso))
        if i not in place:
            chunk = tango.dcache_compact_next(chunk, len(b), 0, 1 << 40)
    return mc, region, chunk0, meta


def _model(pool, frags, tc_depth):
    """What the tile owes for `frags`: the published frags [(input index,
    SHA-512 tag)], and the HA_FILT, SV_FILT and bad frag counts.  A refused
    frag is only counted: it never reaches the dedup window."""
    pub, sig, msgs, verdict = pool
    seen, q = set(), collections.deque()
    out, ha, sv, bad = [], 0, 0, 0
    for i, f in enumerate(frags):
        if f.k is None:
            bad += 1
            continue
        k = f.k
        tag = int.from_bytes(bytes(sig[k][:8]), "little")
        if tc_depth and tag:
            if tag in seen:
                ha += 1
                continue
            seen.add(tag); q.append(tag)
            if len(q) > tc_depth:
                seen.discard(q.popleft())
        if verdict[k] != 0:
            sv += 1
            continue
        h = hashlib.sha512(bytes(sig[k][:32]) + bytes(pub[k]) + msgs[k]).digest()
        out.append((i, int.from_bytes(h[:8], "little")))
    return out, ha, sv, bad


def _model_log(pool, frags, tc_depth):
    """The verdict log the run must leave: the golden verdict of every frag
    that was verified, SENTINEL for the bad frags and the HA duplicates."""
    verdict = pool[3]
    log = np.full(len(frags), SENTINEL, np.int8)
    seen, q = set(), collections.deque()
    for i, f in enumerate(frags):
        if f.k is None:
            continue
        tag = int.from_bytes(bytes(pool[1][f.k][:8]), "little")
        if tc_depth and tag:
            if tag in seen:
                continue
            seen.add(tag); q.append(tag)
            if len(q) > tc_depth:
                seen.discard(q.popleft())
        log[i] = verdict[f.k]
    return log


def _check_counts(diag, n, exp, ha, sv, bad):
    got = {k: int(diag[k]) for k in ("in_cnt", "out_cnt", "ha_filt_cnt", "sv_filt_cnt", "bad_frag_cnt", "ovrn_cnt",
                                     "batch_sig_cnt")}
    want = {"in_cnt": n, "out_cnt": len(exp), "ha_filt_cnt": ha, "sv_filt_cnt": sv, "bad_frag_cnt": bad, "ovrn_cnt": 0,
            "batch_sig_cnt": n - bad - ha}
    assert got == want
    assert got["in_cnt"] == got["out_cnt"] + got["sv_filt_cnt"] + got["ha_filt_cnt"] + got["bad_frag_cnt"]


def _check_out(tile, mc_out, out_seq0, exp, pool, frags, meta, first=0):
    """The o-th published frag (o >= first) sits in line (out_seq0 + o) &
    (depth-1) with that sequence number, the model's tag, the input frag's
    sz / ctl / tsorig, and the verified bytes in the tile's output region."""
    depth = mc_out.size
    assert len(exp) - first <= depth
    for o in range(first, len(exp)):
        i, tag = exp[o]
        s = (out_seq0 + o) & M64
        line = mc_out[s & (depth - 1)]
        assert int(line["seq"]) == s, (o, int(line["seq"]), s)
        assert int(line["sig"]) == tag, o
        assert (int(line["sz"]), int(line["ctl"]), int(line["tsorig"])) == meta[i][1:], o
        assert tile.out_frame(line["chunk"], line["sz"]) == _frag_bytes(pool, frags[i].k), o


def _bad(pool_bytes, sz):
    """A frag of refused size sz whose bytes are a well-formed frag (cut or
    padded to sz): a guard that let it through would verify and publish it."""
    return Frag(None, sz, (pool_bytes + b"\xaa" * 1536)[:min(sz, 1536)])


def _class_picks(golden, name):
    """Pool indices (of _pool's every third vector) of one golden class."""
    import _golden
    c = _golden.CLASSES.index(name)
    return [j for j, i in enumerate(range(0, len(golden), 3)) if golden.cls[i] == c]


def _a1_stream(golden, pool, seed):
    """~300 pool frags with HA duplicates and every refused size, alone and in
    runs, at the head, in the middle and at the very end; frags of 96 B
    (zero_msg) and 1328 B (max_msg) next to the refused 95 and 1329."""
    rng = np.random.default_rng(seed)
    zero, big = _class_picks(golden, "zero_msg"), _class_picks(golden, "max_msg")
    assert len(zero) >= 3 and len(big) >= 3
    assert all(len(pool[2][k]) == 0 for k in zero) and all(len(pool[2][k]) == MSG_MAX for k in big)
    # the refused frags carry a golden vector outside the pool: valid on its own
    src = bytes(golden.pub[1]) + bytes(golden.sig[1]) + golden.msg(1)
    B = lambda sz: _bad(src, sz)                                    # noqa: E731
    ok = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 300)]
    head = [B(0), B(65535), Frag(zero[0]), B(95), B(1), Frag(big[0]), B(1329)]
    mid = [Frag(zero[1]), B(1408), B(1409), B(65535), B(0), Frag(big[1]), B(1329), Frag(big[1])]
    tail = [Frag(big[2]), B(1329), Frag(zero[2]), B(95)]
    frags = head + ok[:150] + mid + ok[150:] + tail
    for at, sz in zip((20, 47, 90, 133, 201, 250, 290), BAD_SIZES):   # each size once on its own
        frags.insert(at, B(sz))
    assert {f.sz for f in frags if f.k is None} == set(BAD_SIZES) and frags[-1].k is None and frags[0].k is None
    return frags


@pytest.mark.parametrize("chunk_mode", [0, 2])      # tango.CHUNK_AUTO, CHUNK_THROUGHPUT
@pytest.mark.parametrize("zero_copy", [False, True])
def test_bad_sizes_are_refused_and_only_counted(golden, zero_copy, chunk_mode):
    """A1.  PUB_SIG_MSG frags of size 0, 1, 95, 1329, 1408, 1409 and 65535
    among valid ones (96 and 1328 B included): each is counted in in_cnt and
    bad_frag_cnt, released through in_fseq, never staged (batch_sig_cnt),
    never logged; everything else publishes exactly as the model says, with
    its own ctl."""
    from firedancer_amd import tango
    pool = _pool(golden)
    frags = _a1_stream(golden, pool, 11)
    n, tc_depth = len(frags), 1 << 12
    mc_in, region, chunk0, meta = _feed(pool, frags, 2048)
    mc_out = tango.mcache_new(2048)
    exp, ha, sv, bad = _model(pool, frags, tc_depth)
    assert bad == sum(f.k is None for f in frags) == 19 and ha > 0 and sv > 0
    assert len({m[2] for m in meta}) > 300                      # ctl varies
    tile = tango.VerifyTile(0, batch_max=512, tcache_depth=tc_depth, chunk_mode=chunk_mode)
    log = np.full(n, SENTINEL, np.int8)
    tile.set_verdict_log(log)
    try:
        if zero_copy:
            tile.register_dcache(region)
        diag, _ = tile.run(mc_in, chunk0, 0, mc_out, 0, n)
        _check_counts(diag, n, exp, ha, sv, bad)
        assert tile.in_fseq == n
        _check_out(tile, mc_out, 0, exp, pool, frags, meta)
        assert np.array_equal(log, _model_log(pool, frags, tc_depth))
        assert all(log[i] == SENTINEL for i, f in enumerate(frags) if f.k is None)
    finally:
        tile.close()


@pytest.mark.parametrize("zero_copy", [False, True])
def test_refused_frag_does_not_enter_the_dedup_window(golden, zero_copy):
    """A2.  A refused frag (1329 B) carrying, where a signature's first 8
    bytes would be, the HA tag of a later valid frag: the later frag is
    published, not HA-filtered; a pair of valid duplicates in the same run
    still is."""
    from firedancer_amd import tango
    pool = _pool(golden)
    verdict = pool[3]
    good = [k for k in range(len(verdict)) if verdict[k] == 0 and len(pool[2][k]) >= 16][:12]
    victim, twin = good[5], good[7]
    vb = _frag_bytes(pool, victim)
    frags = [Frag(k) for k in good[:5]] + [_bad(vb, 1329)] + [Frag(good[6]), Frag(twin), Frag(victim), Frag(twin)] + \
        [Frag(k) for k in good[8:]]
    assert frags[5].data[32:40] == bytes(pool[1][victim][:8])
    n = len(frags)
    mc_in, region, chunk0, meta = _feed(pool, frags, 64)
    mc_out = tango.mcache_new(64)
    exp, ha, sv, bad = _model(pool, frags, 64)
    assert (ha, sv, bad) == (1, 0, 1) and 8 in [i for i, _ in exp] and 9 not in [i for i, _ in exp]
    tile = tango.VerifyTile(0, batch_max=64, tcache_depth=64)
    try:
        if zero_copy:
            tile.register_dcache(region)
        diag, _ = tile.run(mc_in, chunk0, 0, mc_out, 0, n)
        _check_counts(diag, n, exp, ha, sv, bad)
        _check_out(tile, mc_out, 0, exp, pool, frags, meta)
        assert tile.in_fseq == n
    finally:
        tile.close()


@pytest.mark.parametrize("zero_copy", [False, True])
def test_txn_empty_and_over_mtu_frags_are_refused(zero_copy):
    """A3.  TXN framing: frags of size 0 and 1233 (a 1232-B reference fixture
    transaction padded by one byte) among ~100 signed transactions, alone, in
    a run and as the last frag: counted as bad frags, never logged; every
    other frag's verdict equals the oracle's and the accepted ones publish in
    order with their bytes and first-signature tags."""
    import _txn
    from firedancer_amd import tango
    pays, _ = _txn.build_txns(303, 100, nsig_hi=6)
    pays = [bytearray(p) for p in pays]
    rng = np.random.default_rng(5)
    for t in rng.choice(len(pays), 12, replace=False):
        pays[t][1 + int(rng.integers(0, 64))] ^= 0x10                  # a signature byte
    fix = [f.payload for f in _txn.load_fixtures() if len(f.payload) == 1232]
    assert fix
    over = bytes(fix[0]) + b"\0"
    assert len(over) == 1233
    items = [bytes(p) for p in pays]
    for at in (0, 1, 30, 31, 32, 70):
        items.insert(at, b"" if at % 2 == 0 else over)
    items += [over, b""]                                               # a bad frag is the last one
    n = len(items)
    is_bad = [len(p) == 0 or len(p) > 1232 for p in items]
    assert sum(is_bad) == 8
    good = [p for p, b in zip(items, is_bad) if not b]
    blob, off, sz = _txn.pack(good)
    eterr, _, _ = _oracle.txn_verify_batch(blob, off, sz)
    want_log = np.full(n, SENTINEL, np.int8)
    want_log[[i for i in range(n) if not is_bad[i]]] = eterr
    assert (eterr == 0).sum() > 50 and (eterr != 0).sum() >= 12

    mtu_chunks = ((1233 + 127) >> 7) << 1
    region = tango._aligned((64 * mtu_chunks * n + SLACK + 4095) & ~4095, 4096)
    mc_in, mc_out = tango.mcache_new(256), tango.mcache_new(256)
    for s, p in enumerate(items):
        c = s * mtu_chunks
        if len(p):
            region[64 * c:64 * c + len(p)] = np.frombuffer(p, np.uint8)
        tango.publish(mc_in, s, 0, c, len(p), (s * 31 + 2) & 0xFFFF, s, 0)
    tile = tango.VerifyTile(0, batch_max=64, tcache_depth=0, framing=tango.VerifyTile.FRAMING_TXN)
    log = np.full(n, SENTINEL, np.int8)
    tile.set_verdict_log(log)
    try:
        if zero_copy:
            tile.register_dcache(region)
        diag, _ = tile.run(mc_in, region, 0, mc_out, 0, n)
        acc = [i for i in range(n) if want_log[i] == 0]
        assert (diag["in_cnt"], diag["bad_frag_cnt"], diag["out_cnt"], diag["ovrn_cnt"], diag["ha_filt_cnt"]) == \
            (n, 8, len(acc), 0, 0)
        assert diag["sv_filt_cnt"] == int((eterr != 0).sum())
        assert diag["in_cnt"] == diag["out_cnt"] + diag["sv_filt_cnt"] + diag["ha_filt_cnt"] + diag["bad_frag_cnt"]
        assert diag["batch_sig_cnt"] == sum(p[0] for p, b in zip(items, is_bad) if not b)   # their signature slots
        assert tile.in_fseq == n
        assert np.array_equal(log, want_log)
        for o, i in enumerate(acc):
            line = mc_out[o]
            assert (int(line["seq"]), int(line["sz"]), int(line["ctl"]), int(line["tsorig"])) == \
                (o, len(items[i]), (i * 31 + 2) & 0xFFFF, i)
            assert int(line["sig"]) == _txn_tag(items[i])
            assert tile.out_frame(line["chunk"], line["sz"]) == items[i]
    finally:
        tile.close()


def test_zero_copy_offset_origin_and_region_limit(golden):
    """A4.  Zero copy with in_chunk0 one page into the mapped region (chunk
    indices relative to it): the pool publishes as the model says.  A frag
    whose 64-B-rounded end is exactly the region's end is accepted; one whose
    rounded end is one chunk past it, and one whose chunk lies wholly past
    it, are refused as bad frags -- the guard is host-side and a refused frag
    writes no ring entry, so the GPU is never given either."""
    from firedancer_amd import tango
    pool = _pool(golden)
    rng = np.random.default_rng(44)
    verdict = pool[3]
    edge = next(k for k in range(len(verdict)) if verdict[k] == 0 and 100 <= len(pool[2][k]) <= 1000 and
                (96 + len(pool[2][k])) % 64)                           # its end is rounded up to the region's end
    frags = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 300)]
    at = 140
    eb = _frag_bytes(pool, edge)
    frags[at:at] = [Frag(edge), Frag(None, len(eb), eb), Frag(None, len(eb), eb)]
    n, tc_depth, lead = len(frags), 8, 4096
    # the three edge frags sit at the mapped region's end, behind the packed stream
    need = _packed_bytes(pool, frags, (at, at + 1, at + 2))
    region_sz = (lead + need + 4096 + 4095) & ~4095                    # the mapped bytes
    lim = region_sz - lead                                             # ... from in_chunk0 on
    rnd = (len(eb) + 63) & ~63
    c_edge = (lim - rnd) >> 6
    place = {at: c_edge, at + 1: c_edge + 1, at + 2: (lim >> 6) + 3}
    assert 64 * c_edge + rnd == lim and 64 * c_edge >= need
    mc_in, region, chunk0, meta = _feed(pool, frags, 1024, lead=lead, min_size=region_sz + SLACK, place=place)
    assert region.size >= region_sz + SLACK and region.ctypes.data % 4096 == 0
    assert bytes(chunk0[64 * c_edge:64 * c_edge + len(eb)]) == eb
    mc_out = tango.mcache_new(1024)
    exp, ha, sv, bad = _model(pool, frags, tc_depth)
    assert bad == 2 and at in [i for i, _ in exp]
    tile = tango.VerifyTile(0, batch_max=256, tcache_depth=tc_depth)
    log = np.full(n, SENTINEL, np.int8)
    tile.set_verdict_log(log)
    try:
        tile.register_dcache(region[:region_sz])                        # the slack behind it stays unmapped
        diag, _ = tile.run(mc_in, chunk0, 0, mc_out, 0, n)
        _check_counts(diag, n, exp, ha, sv, bad)
        assert tile.in_fseq == n
        _check_out(tile, mc_out, 0, exp, pool, frags, meta)
        assert np.array_equal(log, _model_log(pool, frags, tc_depth))
    finally:
        tile.close()


def test_in_chunk0_outside_the_mapped_region_stages_by_copy(golden):
    """A5.  A tile with a mapped region run on a data region elsewhere: the
    run stages by copy (header: zero copy only when in_chunk0 lies inside the
    mapped region) and publishes the same set."""
    from firedancer_amd import tango
    pool = _pool(golden)
    rng = np.random.default_rng(55)
    frags = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 300)]
    n, tc_depth = len(frags), 8
    mc_in, region, chunk0, meta = _feed(pool, frags, 1024)
    other = tango._aligned(1 << 16, 4096)
    assert not (other.ctypes.data <= chunk0.ctypes.data < other.ctypes.data + other.size)
    mc_out = tango.mcache_new(1024)
    exp, ha, sv, bad = _model(pool, frags, tc_depth)
    tile = tango.VerifyTile(0, batch_max=256, tcache_depth=tc_depth)
    try:
        tile.register_dcache(other)
        diag, _ = tile.run(mc_in, chunk0, 0, mc_out, 0, n)
        _check_counts(diag, n, exp, ha, sv, bad)
        assert tile.in_fseq == n
        _check_out(tile, mc_out, 0, exp, pool, frags, meta)
    finally:
        tile.close()


# ---- B. sequence origins ----

ORIGINS = [(12345, 777),
           ((1 << 63) - 40, (1 << 63) - 25),        # both cross the sign boundary of the signed compares
           ((1 << 64) - 100, (1 << 64) - 37),       # both wrap, at different frags
           (M64, M64)]


@pytest.mark.parametrize("zero_copy", [False, True])
@pytest.mark.parametrize("in_seq0,out_seq0", ORIGINS)
def test_sequence_origins(golden, in_seq0, out_seq0, zero_copy):
    """B.  ~400 pool frags with duplicates from any 64-bit origin: output line
    (out_seq0 + o) & (depth-1) holds seq out_seq0 + o for the o-th published
    frag, in_fseq ends at in_seq0 + n, the verdict log is indexed by seq -
    in_seq0; counts, tags and bytes as the model says (all mod 2^64)."""
    from firedancer_amd import tango
    pool = _pool(golden)
    rng = np.random.default_rng(in_seq0 & 0xFFFF)
    frags = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 400)]
    n, tc_depth = len(frags), 8
    mc_in, region, chunk0, meta = _feed(pool, frags, 1024, seq0=in_seq0)
    mc_out = tango.mcache_new(1024, out_seq0)
    exp, ha, sv, bad = _model(pool, frags, tc_depth)
    assert len(exp) > 100 and ha > 0 and sv > 100
    tile = tango.VerifyTile(0, batch_max=256, tcache_depth=tc_depth)
    log = np.full(n, SENTINEL, np.int8)
    tile.set_verdict_log(log)
    try:
        if zero_copy:
            tile.register_dcache(region)
        diag, _ = tile.run(mc_in, chunk0, in_seq0, mc_out, out_seq0, n)
        _check_counts(diag, n, exp, ha, sv, bad)
        assert tile.in_fseq == (in_seq0 + n) & M64
        _check_out(tile, mc_out, out_seq0, exp, pool, frags, meta)
        assert np.array_equal(log, _model_log(pool, frags, tc_depth))
        # the line after the last published frag still reads "older than out_seq0"
        nxt = (out_seq0 + len(exp)) & M64
        assert _sdiff(int(mc_out[nxt & 1023]["seq"]), out_seq0) < 0
    finally:
        tile.close()


@pytest.mark.parametrize("zero_copy", [False, True])
@pytest.mark.parametrize("second_out_seq0", [M64, 0])
def test_continuation_across_the_wrap(golden, second_out_seq0, zero_copy):
    """B.  Two frag_cnt runs on one tile: the second continues the input at
    in_seq0 + first and the output where the first stopped -- exactly at
    2^64-1, or exactly at 0 after the first run's last frag took 2^64-1.  The
    whole output is dense and in order, as one run's would be."""
    from firedancer_amd import tango
    pool = _pool(golden)
    rng = np.random.default_rng(9)
    frags = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 400)]
    n, first = len(frags), 230
    exp, ha, sv, bad = _model(pool, frags, 0)
    n_first = sum(1 for i, _ in exp if i < first)
    assert 0 < n_first < len(exp)
    in_seq0 = ((1 << 64) - 150) & M64                 # the input wraps inside run 1
    out_seq0 = (second_out_seq0 - n_first) & M64
    mc_in, region, chunk0, meta = _feed(pool, frags, 1024, seq0=in_seq0)
    mc_out = tango.mcache_new(1024, out_seq0)
    tile = tango.VerifyTile(0, batch_max=256, tcache_depth=0)
    log = np.full(n, SENTINEL, np.int8)
    try:
        if zero_copy:
            tile.register_dcache(region)
        tile.set_verdict_log(log[:first])
        d1, _ = tile.run(mc_in, chunk0, in_seq0, mc_out, out_seq0, first)
        assert (d1["in_cnt"], d1["out_cnt"]) == (first, n_first) and tile.in_fseq == (in_seq0 + first) & M64
        # run 1's bytes now: without an out_fseq nothing keeps run 2 from reusing its frames
        _check_out(tile, mc_out, out_seq0, exp[:n_first], pool, frags, meta)
        tile.set_verdict_log(log[first:])
        d2, _ = tile.run(mc_in, chunk0, (in_seq0 + first) & M64, mc_out, second_out_seq0, n - first)
        assert (d2["in_cnt"], d2["out_cnt"]) == (n - first, len(exp) - n_first)
        assert tile.in_fseq == (in_seq0 + n) & M64
        assert d1["sv_filt_cnt"] + d2["sv_filt_cnt"] == sv and d1["ovrn_cnt"] + d2["ovrn_cnt"] == 0
        _check_out(tile, mc_out, out_seq0, exp, pool, frags, meta, first=n_first)
        lines = [mc_out[((out_seq0 + o) & M64) & 1023] for o in range(len(exp))]
        assert [int(ln["seq"]) for ln in lines] == [(out_seq0 + o) & M64 for o in range(len(exp))]
        assert [int(ln["sig"]) for ln in lines] == [t for _, t in exp]
        assert np.array_equal(log, _model_log(pool, frags, 0))
    finally:
        tile.close()


def test_in_fseq_is_given_before_the_first_frag():
    """A run from in_seq0 = 2^64-1 that has seen no frag yet has already told
    the producer so: in_fseq reads in_seq0 while the run waits for input
    (every frag below it is released), whatever the word held before."""
    from firedancer_amd import tango
    in_seq0 = M64
    mc_in, mc_out = tango.mcache_new(64, in_seq0), tango.mcache_new(64, 5)
    region = tango._aligned(4096, 4096)
    fseq, stop, seen = ctypes.c_ulong(4242), ctypes.c_int(0), []

    def watch():
        t0 = time.time()
        while time.time() - t0 < 3.0 and fseq.value != in_seq0:
            time.sleep(0.0005)
        seen.append(fseq.value)
        stop.value = 1
    tile = tango.VerifyTile(0, batch_max=64, tcache_depth=0)
    th = threading.Thread(target=watch)
    th.start()
    try:
        diag, _ = tile.run(mc_in, region, in_seq0, mc_out, 5, 0, stop=stop, in_fseq=fseq)
    finally:
        stop.value = 1
        th.join(timeout=10)
        tile.close()
    assert seen == [in_seq0] and diag["in_cnt"] == 0 and tile.in_fseq == in_seq0


# ---- C. output flow control away from zero ----

def _wait(cond, th=None, limit=30.0):
    """Poll cond() until it holds, thread th has ended or `limit` s passed."""
    t0 = time.time()
    while not cond() and time.time() - t0 < limit and (th is None or th.is_alive()):
        time.sleep(0.0005)
    return cond()


@pytest.mark.parametrize("out_seq0", [(1 << 63) + 5, (1 << 64) - 100])
def test_stalled_consumer_holds_the_tile_to_its_credit(golden, out_seq0):
    """C1.  A consumer whose out_fseq stays at out_seq0: exactly out_depth
    (256) frags are published, seqs out_seq0 .. out_seq0 + 255 mod 2^64 (in
    the second case the credit window itself spans the wrap), the model's
    first 256; once every input frag is taken in, *stop ends the run and the
    rest counts in halt_drop_cnt.

    Before the fix (out_cr started at 0, so from an origin in [2^63, 2^64)
    the credit was never loaded until the sequence wrapped) the 2^63 + 5 case
    published every accepted frag: out_cnt == 720 instead of 256."""
    from firedancer_amd import tango
    pool = _pool(golden)
    rng = np.random.default_rng(21)
    frags = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 1500)]
    n, depth, in_seq0 = len(frags), 256, (1 << 64) - 700
    exp, ha, sv, bad = _model(pool, frags, 0)
    assert len(exp) > 2 * depth
    mc_in, region, chunk0, meta = _feed(pool, frags, 2048, seq0=in_seq0)
    mc_out = tango.mcache_new(depth, out_seq0)
    out_fseq, in_fseq, stop = ctypes.c_ulong(out_seq0), ctypes.c_ulong(in_seq0), ctypes.c_int(0)
    tile = tango.VerifyTile(0, batch_max=1024, tcache_depth=0, halt_grace_ns=5_000_000)
    res = {}

    def go():
        try:
            res["r"] = tile.run(mc_in, chunk0, in_seq0, mc_out, out_seq0, 0, stop=stop, out_fseq=out_fseq,
                                in_fseq=in_fseq)
        except Exception as e:   # noqa: BLE001
            res["e"] = e

    th = threading.Thread(target=go)
    th.start()
    try:
        last = (out_seq0 + depth - 1) & M64
        # the credit is used up (or overrun) and the whole input is taken in (copy mode releases at the copy)
        _wait(lambda: _sdiff(int(mc_out[last & (depth - 1)]["seq"]), last) >= 0 and
              in_fseq.value == (in_seq0 + n) & M64, th)
        alive = th.is_alive()
        stop.value = 1
        th.join(timeout=10)
        assert alive and not th.is_alive()
        assert "e" not in res, res.get("e")
        diag, _ = res["r"]
        assert diag["out_cnt"] == depth, (diag["out_cnt"], hex(out_seq0))
        _check_out(tile, mc_out, out_seq0, exp[:depth], pool, frags, meta)
        assert diag["halt_drop_cnt"] > 0 and diag["in_cnt"] == n and diag["ovrn_cnt"] == 0
        assert diag["out_cnt"] + diag["sv_filt_cnt"] + diag["halt_drop_cnt"] == diag["in_cnt"]
    finally:
        stop.value = 1
        th.join(timeout=10)
        tile.close()


@pytest.mark.parametrize("zero_copy", [False, True])
def test_moving_consumer_reused_frames_across_the_wrap(golden, zero_copy):
    """C2.  out_depth 64 and 192 output frames (the consumer's 64 + a window
    of 64 + a batch of 64: every frame is reused ~8 times over 1500 frags)
    from out_seq0 = 2^64 - 300, so the frag published as seq 2^64-1 and the
    reuse of its frame fall inside the run.  A consumer thread takes the
    output in order, as late as flow control allows (it reads frag s once
    s + 63, the last one its credit admits, is out), checks line, tag and
    bytes against the model and only then advances out_fseq by one: every
    frag is intact when read, no line ever holds a seq past out_fseq + 63,
    and the run ends with everything published."""
    from firedancer_amd import tango
    pool = _pool(golden)
    rng = np.random.default_rng(31)
    frags = [Frag(int(k)) for k in rng.integers(0, len(pool[2]), 1500)]
    n, depth, tc_depth = len(frags), 64, 8
    in_seq0, out_seq0 = (1 << 63) - 700, (1 << 64) - 300
    exp, ha, sv, bad = _model(pool, frags, tc_depth)
    assert len(exp) > 600
    mc_in, region, chunk0, meta = _feed(pool, frags, 2048, seq0=in_seq0)
    mc_out = tango.mcache_new(depth, out_seq0)
    out_fseq, stop, quit_ = ctypes.c_ulong(out_seq0), ctypes.c_int(0), []
    tile = tango.VerifyTile(0, batch_max=64, tcache_depth=tc_depth, window=64, out_frame_cnt=192,
                            halt_grace_ns=5_000_000)
    errs = []

    def line_of(s):
        return mc_out[s & (depth - 1)]

    def consume():
        try:
            for o, (i, tag) in enumerate(exp):
                s = (out_seq0 + o) & M64
                ahead = (out_seq0 + min(o + depth - 1, len(exp) - 1)) & M64    # the newest frag the credit admits
                if not _wait(lambda: quit_ or (_sdiff(int(line_of(s)["seq"]), s) >= 0 and
                                               _sdiff(int(line_of(ahead)["seq"]), ahead) >= 0), limit=60.0) or quit_:
                    errs.append(("never published", o))
                    return
                line = line_of(s)
                got = (int(line["seq"]), int(line_of(ahead)["seq"]), int(line["sig"]), int(line["sz"]),
                       int(line["ctl"]), int(line["tsorig"]))
                if got != (s, ahead, tag) + meta[i][1:]:      # a seq past s + 63 would show in one of the two lines
                    errs.append(("line", o, got, (s, ahead, tag) + meta[i][1:]))
                    return
                if tile.out_frame(line["chunk"], line["sz"]) != _frag_bytes(pool, frags[i].k):
                    errs.append(("bytes changed under the consumer", o, hex(s)))
                    return
                out_fseq.value = (s + 1) & M64
        finally:
            if errs:
                stop.value = 1

    th = threading.Thread(target=consume)
    th.start()
    try:
        if zero_copy:
            tile.register_dcache(region)
        diag, _ = tile.run(mc_in, chunk0, in_seq0, mc_out, out_seq0, n, stop=stop, out_fseq=out_fseq)
        th.join(timeout=60)
        assert not th.is_alive()
        assert not errs, errs
        _check_counts(diag, n, exp, ha, sv, bad)
        assert out_fseq.value == (out_seq0 + len(exp)) & M64 and diag["halt_drop_cnt"] == 0
        assert tile.in_fseq == (in_seq0 + n) & M64
    finally:
        stop.value = 1
        quit_.append(1)
        th.join(timeout=60)
        tile.close()


@pytest.mark.parametrize("zero_copy", [False, True])
def test_frame_of_seq_max_is_kept_for_a_lagging_consumer(golden, zero_copy):
    """The frame that carried out seq 2^64-1 is a frame in use like any other.
    Run 1 publishes 40 frags as seqs 2^64-40 .. 2^64-1 into frames 0..39 of
    64; the consumer then stands at 2^64-1 (it has not read that frag yet).
    Run 2 continues at seq 0: it may reuse frames 0..38 and publish 39 frags,
    and then has to wait -- frame 39 keeps run 1's last frag, and seq 39 is
    not published -- until out_fseq passes 2^64-1; then the rest follows.

    Before the fix (~0UL marked a frame that carried nothing) run 2 took
    frame 39 at once and overwrote the unread frag."""
    from firedancer_amd import tango
    pool = _pool(golden)
    good = [k for k in range(len(pool[3])) if pool[3][k] == 0][:100]
    assert len(good) == 100
    frags = [Frag(k) for k in good]
    n, n1, depth = len(frags), 40, 256
    exp, ha, sv, bad = _model(pool, frags, 0)
    assert len(exp) == n
    in_seq0, out_seq0 = 5, (1 << 64) - n1
    mc_in, region, chunk0, meta = _feed(pool, frags, 256, seq0=in_seq0)
    mc_out = tango.mcache_new(depth, out_seq0)
    out_fseq, stop = ctypes.c_ulong(out_seq0), ctypes.c_int(0)
    tile = tango.VerifyTile(0, batch_max=64, tcache_depth=0, window=64, out_frame_cnt=64, halt_grace_ns=5_000_000)
    res = {}

    def go():
        try:
            res["r"] = tile.run(mc_in, chunk0, in_seq0 + n1, mc_out, 0, 0, stop=stop, out_fseq=out_fseq)
        except Exception as e:   # noqa: BLE001
            res["e"] = e

    th = threading.Thread(target=go)
    try:
        if zero_copy:
            tile.register_dcache(region)
        d1, _ = tile.run(mc_in, chunk0, in_seq0, mc_out, out_seq0, n1, out_fseq=out_fseq)
        assert d1["out_cnt"] == n1
        _check_out(tile, mc_out, out_seq0, exp[:n1], pool, frags, meta)
        last = mc_out[M64 & (depth - 1)]
        assert int(last["seq"]) == M64
        out_fseq.value = M64                          # everything before the last frag is read
        th.start()
        assert _wait(lambda: int(mc_out[n1 - 2]["seq"]) == n1 - 2, th)      # run 2's 39th frag, seq 38
        assert tile.out_frame(last["chunk"], last["sz"]) == _frag_bytes(pool, frags[n1 - 1].k)
        assert int(mc_out[n1 - 1]["seq"]) != n1 - 1 and th.is_alive()
        out_fseq.value = 0                            # now it is read
        assert _wait(lambda: int(mc_out[n - n1 - 1]["seq"]) == n - n1 - 1, th)
        stop.value = 1
        th.join(timeout=10)
        assert not th.is_alive() and "e" not in res, res.get("e")
        d2, _ = res["r"]
        assert (d2["in_cnt"], d2["out_cnt"], d2["halt_drop_cnt"]) == (n - n1, n - n1, 0)
        _check_out(tile, mc_out, out_seq0, exp, pool, frags, meta, first=n1)
    finally:
        stop.value = 1
        if th.ident is not None:
            th.join(timeout=10)
        tile.close()
