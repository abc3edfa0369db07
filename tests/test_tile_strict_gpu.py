"""GPU: strict RFC 8032 verdicts in the streaming verify tile
(fd_verify_amd_tile_set_verdict_mode, k_tile_persist_strict): every chunk
mode's parked-R' layout, both pair subs, the chunk edges, TXN framing's
first-failing-signature rule and the stream bench, against the independent
Python verifier tests/_strict_ref.py.  The mode is the tile's and a run's:
a tile back in reference mode, and a second tile beside a strict one, give
the reference's codes bit for bit.  The directed edge corpus (tests/_edges.py)
goes through every chunk mode in both verdict modes."""
import hashlib
import os
import struct

import numpy as np
import pytest

import _oracle
import _strict_ref
import _txn
from test_tile_gpu import _feed, _stream_pool, _txn_tag

pytestmark = pytest.mark.gpu

LAT, THR, QUAD = 1, 2, 3          # tango.CHUNK_LATENCY, CHUNK_THROUGHPUT, CHUNK_QUAD
SLOTS = {LAT: 8, THR: 64, QUAD: 16}
PARSE = -4                        # FD_TXN_AMD_ERR_PARSE


@pytest.fixture(scope="module")
def strict_golden(golden):
    """The strict verdict of every golden vector, computed once (shared
    with test_strict_gpu.py through _strict_ref's cache)."""
    s = np.array(_strict_ref.verify_batch(golden), np.int8)
    s.setflags(write=False)
    assert int((s != golden.expect).sum()) == 760
    return s


@pytest.fixture(scope="module")
def golden_feed(golden):
    """All golden vectors as frags, in order, published once; every test
    that runs the whole set reads the same mcache / dcache."""
    msgs = [golden.msg(i) for i in range(len(golden))]
    assert max(len(m) for m in msgs) <= 1232
    mc_in, dc, _, _, _ = _feed(golden.pub, golden.sig, msgs, np.arange(len(golden)), 4096)
    tags = np.array([int.from_bytes(hashlib.sha512(bytes(golden.sig[i][:32]) + bytes(golden.pub[i]) + msgs[i]).digest()[:8],
                                    "little") for i in range(len(golden))], np.uint64)
    return mc_in, dc, tags


def _codes(v):
    return [int((v == c).sum()) for c in (0, -1, -2, -3)]


def _sv(diag):
    return [diag["sv_filt_sig_cnt"], diag["sv_filt_pubkey_cnt"], diag["sv_filt_msg_cnt"]]


def _report(log, want, n=10):
    bad = np.nonzero(log != want)[0]
    return bad.size, [(int(i), int(log[i]), int(want[i])) for i in bad[:n]]


@pytest.mark.parametrize("chunk_mode", [LAT, THR, QUAD])
@pytest.mark.parametrize("zero_copy", [False, True])
def test_strict_tile_golden_codes_per_chunk_mode(monkeypatch, golden, strict_golden, golden_feed, chunk_mode, zero_copy):
    """All 2046 golden vectors through a strict tile with every chunk forced
    to one mode (k_dsm8's, k_dsm's, k_dsm4's parked layout; quad chunks as
    pairs, so both subs run the overlay): the verdict log equals the strict
    verdict of every frag, and the published set, its SHA-512 tags in order
    and the per-code SV_FILT counts follow the strict verdicts."""
    from firedancer_amd import ed25519, tango
    monkeypatch.setenv("FD_AMD_TILE_PAIRS", "1")
    n = len(golden)
    mc_in, dc, tags = golden_feed
    mc_out = tango.mcache_new(4096)
    tile = tango.VerifyTile(0, batch_max=4096, tcache_depth=0, chunk_mode=chunk_mode, mode=ed25519.MODE_STRICT)
    if zero_copy:
        tile.register_dcache(dc)
    log = np.full(n, 99, np.int8)
    tile.set_verdict_log(log)
    try:
        assert tile.verdict_mode == ed25519.MODE_STRICT
        diag, _ = tile.run(mc_in, dc, 0, mc_out, 0, n)
    finally:
        tile.close()
    nbad, bad = _report(log, strict_golden)
    assert nbad == 0, (nbad, bad)
    assert _codes(strict_golden) == [1034, 152, 727, 133]
    assert diag["out_cnt"] == 1034 and diag["sv_filt_cnt"] == n - 1034 and _sv(diag) == [152, 727, 133]
    acc = np.nonzero(strict_golden == 0)[0]
    assert [int(mc_out[o]["seq"]) for o in range(acc.size)] == list(range(acc.size))
    assert [int(mc_out[o]["sig"]) for o in range(acc.size)] == [int(t) for t in tags[acc]]
    key = {LAT: "gpu_frag_lat_cnt", THR: "gpu_frag_thr_cnt", QUAD: "gpu_frag_quad_cnt"}[chunk_mode]
    assert diag[key] == n
    if chunk_mode == QUAD:
        assert diag["quad_pair_cnt"] > 0


def test_verdict_mode_is_per_run_and_per_tile(monkeypatch, golden, strict_golden, golden_feed):
    """One tile: a strict run, the same feed in reference mode (the log is
    the reference's codes), strict again.  A second tile created beside it
    stays in reference mode throughout.  A bad mode is refused and changes
    nothing."""
    from firedancer_amd import ed25519, tango
    n = len(golden)
    mc_in, dc, _ = golden_feed
    a = tango.VerifyTile(0, batch_max=4096, tcache_depth=0, mode=ed25519.MODE_STRICT)
    b = tango.VerifyTile(0, batch_max=4096, tcache_depth=0)
    try:
        assert (a.verdict_mode, b.verdict_mode) == (ed25519.MODE_STRICT, ed25519.MODE_REFERENCE)
        seq = {id(a): 0, id(b): 0}
        outs = {id(a): tango.mcache_new(8192), id(b): tango.mcache_new(8192)}

        def run(t, want):
            log = np.full(n, 99, np.int8)
            t.set_verdict_log(log)
            diag, _ = t.run(mc_in, dc, 0, outs[id(t)], seq[id(t)], n)
            seq[id(t)] += diag["out_cnt"]
            nbad, bad = _report(log, want)
            assert nbad == 0, (nbad, bad)
            assert diag["out_cnt"] == int((want == 0).sum()) and _sv(diag) == _codes(want)[1:]

        run(a, strict_golden)
        run(b, golden.expect)
        a.set_verdict_mode(ed25519.MODE_REFERENCE)
        assert a.verdict_mode == ed25519.MODE_REFERENCE
        run(a, golden.expect)
        for bad_mode in (2, -1, 1 << 20):
            with pytest.raises(ed25519.EngineError):
                a.set_verdict_mode(bad_mode)
            assert ed25519.lib().fd_verify_amd_tile_set_verdict_mode(a._h, bad_mode) == -10      # ERR_INVAL
            assert a.verdict_mode == ed25519.MODE_REFERENCE
        a.set_verdict_mode(ed25519.MODE_STRICT)
        with pytest.raises(ed25519.EngineError):
            a.set_verdict_mode(7)
        assert a.verdict_mode == ed25519.MODE_STRICT
        run(a, strict_golden)
        assert b.verdict_mode == ed25519.MODE_REFERENCE
        run(b, golden.expect)
    finally:
        a.close()
        b.close()


def _edge_order(n, slots, changed, same):
    """n golden indices whose last chunk (the slots past the last multiple
    of the chunk size) holds only vectors whose strict verdict differs from
    the reference's, spread over their classes (test_strict_gpu._tail_order
    for a chunk of `slots`)."""
    tail_len = n - slots * ((n - 1) // slots)
    tail = changed[::max(1, len(changed) // tail_len)][:tail_len]
    used = set(tail.tolist())
    head = [i for i in changed[3::7].tolist() + same.tolist() if i not in used][:n - tail_len]
    order = np.array(head + tail.tolist(), np.int64)
    assert order.size == n and len(set(order.tolist())) == n
    return order


EDGES = [(THR, n) for n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)] + \
        [(LAT, n) for n in (1, 7, 8, 9)] + [(QUAD, n) for n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)]


@pytest.mark.parametrize("chunk_mode,n", EDGES, ids=["%s-%d" % ({LAT: "lat", THR: "thr", QUAD: "quad"}[m], n) for m, n in EDGES])
def test_strict_tile_chunk_edges(monkeypatch, golden, strict_golden, chunk_mode, n):
    """n frags in chunks of one forced mode, n around every chunk size (a
    quad pair is 17..32: 17 is 16 + 1), the last slot of the last chunk a
    vector whose verdict the strict rule changes: the log equals the strict
    verdicts of all n, and nothing past n is written."""
    from firedancer_amd import ed25519, tango
    monkeypatch.setenv("FD_AMD_TILE_PAIRS", "1")
    changed = np.nonzero(strict_golden != golden.expect)[0]
    same = np.nonzero(strict_golden == golden.expect)[0]
    idx = _edge_order(n, SLOTS[chunk_mode], changed, same)
    assert strict_golden[idx[-1]] != golden.expect[idx[-1]]
    want = strict_golden[idx]
    mc_in, dc, _, _, _ = _feed(golden.pub, golden.sig, {int(i): golden.msg(int(i)) for i in idx}, idx, 128)
    mc_out = tango.mcache_new(128)
    tile = tango.VerifyTile(0, batch_max=128, tcache_depth=0, chunk_mode=chunk_mode, mode=ed25519.MODE_STRICT)
    pad = 64
    log = np.full(n + pad, 99, np.int8)
    tile.set_verdict_log(log)
    try:
        diag, _ = tile.run(mc_in, dc, 0, mc_out, 0, n)
    finally:
        tile.close()
    nbad, bad = _report(log[:n], want)
    assert nbad == 0, (n, nbad, bad)
    assert (log[n:] == 99).all()
    assert diag["out_cnt"] == int((want == 0).sum()) and _sv(diag) == _codes(want)[1:]
    assert diag["in_cnt"] == n and diag["bad_frag_cnt"] == 0
    key = {LAT: "gpu_frag_lat_cnt", THR: "gpu_frag_thr_cnt", QUAD: "gpu_frag_quad_cnt"}[chunk_mode]
    assert diag[key] == n
    if chunk_mode == QUAD and 17 <= n <= 32:
        assert diag["quad_pair_cnt"] == 1


# ---- TXN framing ------------------------------------------------------------------

WINDOW_S = bytes(16) + bytes([0, 0, 0, 0, 1]) + bytes(10) + bytes([0x10])   # s[31] = 0x10, s[20] = 1: the reference's early accept
IDENT = bytes([1]) + bytes(31)                                               # the identity (0, 1)
FREJ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txn_false_rejects.bin")


def _fields(p):
    """(signers, message offset, offset of signer 0's address) of a legacy or v0 transaction with < 128 accounts."""
    n = p[0]
    m = 1 + 64 * n
    return n, m, m + (1 if p[m] & 0x80 else 0) + 4


def _sig_codes(p, fn):
    n, m, a = _fields(p)
    return [int(fn(p[m:], p[1 + 64 * k:65 + 64 * k], p[a + 32 * k:a + 32 * k + 32])) for k in range(n)]


def _signed_txn(rng, nsig, v0, torsion=None):
    """A transaction of nsig signers, each signature valid -- except signer
    `torsion`, whose address is the identity, with R = identity and s = 0
    (the reference accepts that for any message; strict: -2)."""
    from firedancer_amd import ed25519
    prv = rng.integers(0, 256, (nsig, 32), dtype=np.uint8)
    z = np.zeros(nsig, np.uint32)
    pub, _ = ed25519.sign_batch(prv, np.zeros(1, np.uint8), z, z)
    pub = pub.copy()
    if torsion is not None:
        pub[torsion] = np.frombuffer(IDENT, np.uint8)
    msg = _txn.message(rng, pub, int(rng.integers(80, 200)), v0, 1)
    blob = np.frombuffer(msg + bytes(4), np.uint8)
    _, sig = ed25519.sign_batch(prv, blob, z, np.full(nsig, len(msg), np.uint32))
    sig = sig.copy()
    if torsion is not None:
        sig[torsion] = np.frombuffer(IDENT + bytes(32), np.uint8)
    return bytes([nsig]) + sig.tobytes() + msg


def _with_window(p, k):
    q = bytearray(p)
    q[1 + 64 * k + 32:1 + 64 * k + 64] = WINDOW_S
    return bytes(q)


def _with_flip(p, k):
    q = bytearray(p)
    q[1 + 64 * k + 32 + 5] ^= 0x10     # a low bit of s (still < L): the signature fails with -3 in both modes
    return bytes(q)


def _false_reject_txns():
    raw = open(FREJ, "rb").read()
    assert raw[:12] == b"FDTXNFREJ001"
    cnt = struct.unpack_from("<I", raw, 16)[0]
    at, out = 20, []
    for _ in range(cnt):
        nsig, pos, sz = struct.unpack_from("<III", raw, at)
        out.append((nsig, pos, raw[at + 12:at + 12 + sz]))
        at += 12 + sz + (-sz % 4)
    return out


@pytest.fixture(scope="module")
def txn_cases():
    """(payloads, strict verdict per transaction, positions of the
    changed-verdict signatures): 1, 2 and 12 signers with an s-window
    forgery, a torsion signer or a false-reject signature first, in the
    middle or last; clean transactions; one with a plain bad signature
    before / after a changed one (the first failing code wins); one that
    fails to parse.  The changed signatures' reference verdict (the CPU
    oracle) differs from the strict one."""
    rng = np.random.default_rng(20250)
    pays, marks = [], []

    def add(p, changed=()):
        pays.append(p)
        marks.append(tuple(changed))

    for nsig in (1, 2, 12):
        add(_signed_txn(rng, nsig, nsig == 2))
    for nsig, pos in ((1, 0), (2, 0), (2, 1), (12, 0), (12, 6), (12, 11)):
        add(_with_window(_signed_txn(rng, nsig, pos & 1 == 0), pos), [pos])
        add(_signed_txn(rng, nsig, pos & 1 == 1, torsion=pos), [pos])
    fr = _false_reject_txns()
    assert sorted((n, k) for n, k, _ in fr) == [(1, 0), (2, 1), (12, 6)]
    for nsig, pos, p in fr:
        add(p, [pos])
    base = _signed_txn(rng, 12, True)
    add(_with_flip(_with_window(base, 9), 2), [9])                  # -3 at 2 comes first
    add(_with_flip(_with_window(base, 3), 7), [3])                  # -1 at 3 comes first
    add(_with_window(fr[2][2], 10), [6, 10])                        # the false reject now passes, the forgery does not
    broken = bytearray(_signed_txn(rng, 2, False))
    broken[1 + 64 * 2] ^= 0x40                                      # the header's signature count: parse failure
    add(bytes(broken))
    add(_signed_txn(rng, 1, True))
    want = []
    for t, (p, ch) in enumerate(zip(pays, marks)):
        if t == len(pays) - 2:                                      # the broken one
            want.append(PARSE)
            continue
        s = _sig_codes(p, _strict_ref.verify)
        r = _sig_codes(p, _oracle.verify)
        assert all(s[k] != r[k] for k in ch), (ch, s, r)
        want.append(next((v for v in s if v), 0))
    want = np.array(want, np.int8)
    assert all(1 <= len(p) <= 1232 for p in pays)                   # every one a frag the tile takes
    blob, off, sz = _txn.pack(pays)
    assert (_oracle.txn_verify_batch(blob, off, sz)[0] == PARSE).tolist() == [t == len(pays) - 2 for t in range(len(pays))]
    assert set(want.tolist()) == {0, -1, -2, -3, PARSE}
    return pays, want


@pytest.mark.parametrize("chunk_mode", [0, THR, QUAD])
@pytest.mark.parametrize("zero_copy", [False, True])
def test_strict_tile_txn_framing(txn_cases, chunk_mode, zero_copy):
    """TXN framing keeps its rule over the strict codes: a transaction's
    verdict is its parse failure, else its first failing signature's strict
    code in signature order.  Published set, tags, verdict log and SV_FILT
    counts follow; the parse failure counts in sv_filt_cnt alone."""
    from firedancer_amd import ed25519, tango
    pays, want = txn_cases
    n = len(pays)
    mtu_chunks = ((1232 + 127) >> 7) << 1
    dcache = tango._aligned((64 * mtu_chunks * (n + 2) + 4095) & ~4095, 4096)
    mc_in, mc_out = tango.mcache_new(256), tango.mcache_new(256)
    for seq, p in enumerate(pays):
        c = seq * mtu_chunks
        dcache[64 * c:64 * c + len(p)] = np.frombuffer(p, np.uint8)
        tango.publish(mc_in, seq, 0, c, len(p), 3, seq, 0)
    tile = tango.VerifyTile(0, batch_max=256, tcache_depth=0, framing=tango.VerifyTile.FRAMING_TXN, chunk_mode=chunk_mode,
                            mode=ed25519.MODE_STRICT)
    if zero_copy:
        tile.register_dcache(dcache)
    log = np.full(n + 8, 99, np.int8)
    tile.set_verdict_log(log)
    try:
        diag, _ = tile.run(mc_in, dcache, 0, mc_out, 0, n)
        k = int(diag["out_cnt"])
        frames = [tile.out_frame(mc_out[o]["chunk"], mc_out[o]["sz"]) for o in range(k)]
        tags = [int(mc_out[o]["sig"]) for o in range(k)]
        seqs = [int(mc_out[o]["tsorig"]) for o in range(k)]
    finally:
        tile.close()
    nbad, bad = _report(log[:n], want)
    assert nbad == 0, (nbad, bad)
    assert (log[n:] == 99).all()
    acc = np.nonzero(want == 0)[0].tolist()
    assert seqs == acc and frames == [pays[i] for i in acc] and tags == [_txn_tag(pays[i]) for i in acc]
    assert diag["sv_filt_cnt"] == n - len(acc) and _sv(diag) == _codes(want)[1:]
    assert sum(_sv(diag)) == diag["sv_filt_cnt"] - 1                # the parse failure: SV_FILT, no code counter
    assert diag["bad_frag_cnt"] == 0 and diag["ha_filt_cnt"] == 0


# ---- the stream bench ---------------------------------------------------------------

def test_bench_stream_strict(golden, strict_golden):
    """bench_stream(strict=True) in AUTO mode at a ragged frag count over
    fresh signatures (10 % corrupted) plus the 760 golden vectors whose
    verdict the strict rule changes: every published frag checked against
    the strict verdicts and the host tag function, none missing."""
    import _golden
    from firedancer_amd import ed25519, tango
    pub, sig, off, sz, blob, _, _ = _stream_pool(31415, 320, 400)
    ch = np.nonzero(strict_golden != golden.expect)[0]
    assert ch.size == 760
    blob = np.concatenate([blob, golden.blob])
    base = np.uint32(blob.size - golden.blob.size)
    pub = np.concatenate([pub, golden.pub[ch]])
    sig = np.concatenate([sig, golden.sig[ch]])
    off = np.concatenate([off, golden.msg_off[ch] + base]).astype(np.uint32)
    sz = np.concatenate([sz, golden.msg_sz[ch]]).astype(np.uint32)
    b = _golden.Batch(pub, sig, off, sz, blob)
    err = np.array(_strict_ref.verify_batch(b), np.int8)
    assert np.array_equal(err[320:], strict_golden[ch]) and 0.05 < (err[:320] != 0).mean() < 0.15
    tag = np.array([ed25519.tag(b.msg(i), sig[i], pub[i]) for i in range(len(b))], np.uint64)
    nf = 11 * len(b) + 4 * 64 + 29
    r = tango.bench_stream(0, 4096, 0, pub, sig, off, sz, blob, nf, expect_err=err, expect_tag=tag, strict=True)
    want = int((err[np.arange(nf) % err.size] == 0).sum())
    assert r["mismatches"] == 0 and r["ovrn"] == 0
    assert r["checked"] == r["published"] == want and r["sv_filt"] == nf - want
    # the same stream in reference mode publishes another set: the flag is what made the difference
    ref = _oracle.verify_batch(b)
    assert int((ref != err).sum()) >= 760


# ---- the directed edge corpus (tests/_edges.py; its verdict table is pinned in test_edges_cpu.py) ----

FRAG_KEY = {LAT: "gpu_frag_lat_cnt", THR: "gpu_frag_thr_cnt", QUAD: "gpu_frag_quad_cnt"}
IDS = {LAT: "lat", THR: "thr", QUAD: "quad"}


@pytest.fixture(scope="module")
def corpus():
    """(names, batch, messages, {mode: verdicts}, tags) of the edge corpus:
    the CPU oracle's verdicts for reference mode, the independent Python
    verifier's for strict mode, hashlib's tags; computed once."""
    import _edges
    from firedancer_amd import ed25519
    from test_tags_gpu import _hashlib_tags
    names, b = _edges.corpus()
    ref = _oracle.verify_batch(b)
    strict = np.array(_strict_ref.verify_batch(b), np.int8)
    assert len(b) == 274 and int((ref != strict).sum()) == 117
    tags = _hashlib_tags(b)
    for a in (ref, strict, tags):
        a.setflags(write=False)
    return names, b, [b.msg(i) for i in range(len(b))], {ed25519.MODE_REFERENCE: ref, ed25519.MODE_STRICT: strict}, tags


@pytest.fixture(scope="module")
def corpus_feed(corpus):
    """The corpus as frags, in order, published once."""
    names, b, msgs, _, _ = corpus
    mc_in, dc, _, _, _ = _feed(b.pub, b.sig, msgs, np.arange(len(b)), 512)
    return mc_in, dc


def _check_corpus_run(names, idx, want, tags, log, diag, mc_out, chunk_mode):
    n = len(idx)
    bad = np.nonzero(log[:n] != want)[0]
    assert bad.size == 0, (int(bad.size), [(names[idx[i]], int(want[i]), int(log[i])) for i in bad[:10]])
    assert (log[n:] == 99).all()
    acc = np.nonzero(want == 0)[0]
    assert diag["in_cnt"] == n and diag["bad_frag_cnt"] == 0
    assert diag["out_cnt"] == acc.size and diag["sv_filt_cnt"] == n - acc.size and _sv(diag) == _codes(want)[1:]
    assert [int(mc_out[o]["seq"]) for o in range(acc.size)] == list(range(acc.size))
    assert [int(mc_out[o]["sig"]) for o in range(acc.size)] == [int(tags[idx[i]]) for i in acc]
    assert diag[FRAG_KEY[chunk_mode]] == n


@pytest.mark.parametrize("chunk_mode", [LAT, THR, QUAD], ids=[IDS[m] for m in (LAT, THR, QUAD)])
@pytest.mark.parametrize("strict", [False, True], ids=["reference", "strict"])
@pytest.mark.parametrize("zero_copy", [False, True], ids=["copy", "zero_copy"])
def test_tile_edge_corpus_per_chunk_mode(monkeypatch, corpus, corpus_feed, chunk_mode, strict, zero_copy):
    """All 274 edge vectors (non-canonical and mixed-order points, a
    half-right R', a neutral accumulator, near misses of the byte compares,
    s around L) through a tile with every chunk forced to one mode, in
    reference and in strict mode: the verdict log equals the mode's verdict
    of every frag; out_cnt, the three per-code SV_FILT counts and the
    published tags, in order, follow."""
    from firedancer_amd import ed25519, tango
    monkeypatch.setenv("FD_AMD_TILE_PAIRS", "1")
    names, b, msgs, verdicts, tags = corpus
    mode = ed25519.MODE_STRICT if strict else ed25519.MODE_REFERENCE
    n = len(b)
    mc_in, dc = corpus_feed
    mc_out = tango.mcache_new(512)
    tile = tango.VerifyTile(0, batch_max=512, tcache_depth=0, chunk_mode=chunk_mode, mode=mode)
    if zero_copy:
        tile.register_dcache(dc)
    log = np.full(n + 64, 99, np.int8)
    tile.set_verdict_log(log)
    try:
        assert tile.verdict_mode == mode
        diag, _ = tile.run(mc_in, dc, 0, mc_out, 0, n)
    finally:
        tile.close()
    _check_corpus_run(names, np.arange(n), verdicts[mode], tags, log, diag, mc_out, chunk_mode)
    if chunk_mode == QUAD:
        assert diag["quad_pair_cnt"] > 0


@pytest.mark.parametrize("chunk_mode", [LAT, THR, QUAD], ids=[IDS[m] for m in (LAT, THR, QUAD)])
@pytest.mark.parametrize("strict", [False, True], ids=["reference", "strict"])
def test_tile_edge_corpus_chunk_edge(monkeypatch, corpus, chunk_mode, strict):
    """n one past two whole chunks; the last frag, alone in its chunk, is a
    non-canonical public key that decodes (reference -3, strict -2)."""
    from firedancer_amd import ed25519, tango
    monkeypatch.setenv("FD_AMD_TILE_PAIRS", "1")
    names, b, msgs, verdicts, tags = corpus
    mode = ed25519.MODE_STRICT if strict else ed25519.MODE_REFERENCE
    n = 2 * SLOTS[chunk_mode] + 1
    last = names.index("nc_a/p+18/1")
    assert (verdicts[ed25519.MODE_REFERENCE][last], verdicts[ed25519.MODE_STRICT][last]) == (-3, -2)
    idx = np.array([(11 * i) % len(b) for i in range(n - 1)] + [last], np.int64)       # a stride over every class
    assert len(set(idx.tolist())) == n
    mc_in, dc, _, _, _ = _feed(b.pub, b.sig, msgs, idx, 256)
    mc_out = tango.mcache_new(256)
    tile = tango.VerifyTile(0, batch_max=256, tcache_depth=0, chunk_mode=chunk_mode, mode=mode)
    log = np.full(n + 64, 99, np.int8)
    tile.set_verdict_log(log)
    try:
        diag, _ = tile.run(mc_in, dc, 0, mc_out, 0, n)
    finally:
        tile.close()
    _check_corpus_run(names, idx, verdicts[mode][idx], tags, log, diag, mc_out, chunk_mode)
