"""GPU: the dedup tag -- the little-endian u64 of the first 8 bytes of
SHA-512(R || A || M), which k_prep / k_front hash anyway -- out of every
batch entry point.  Expected values come from hashlib alone; every comparison
is exact.  The tag is 0 exactly where the reference's s check rejects
(reference verdict -1: nothing is hashed) and in the slots of a transaction
that failed to parse, and it does not depend on the verdict mode."""
import hashlib

import numpy as np
import pytest

import _golden
import _oracle
import _strict_ref
import _txn
from test_tags_cpu import EDGE_SIZES

pytestmark = pytest.mark.gpu

KERNELS = ["k_dsm8", "k_dsm4", "k_dsm", "k_dsmp"]


def _hashlib_tags(b):
    """The plain hash tag of every signature of a batch."""
    t = np.array([int.from_bytes(hashlib.sha512(bytes(b.sig[i, :32]) + bytes(b.pub[i]) + b.msg(i)).digest()[:8], "little")
                  for i in range(len(b))], np.uint64)
    return t


def _expected(b, ref_err):
    """What the batch calls return: the hash, 0 where the reference verdict is -1."""
    t = _hashlib_tags(b)
    t[np.asarray(ref_err) == -1] = 0
    t.setflags(write=False)
    return t


def _bad(got, want):
    bad = np.nonzero(got != want)[0]
    return bad.size, [(int(i), hex(int(want[i])), hex(int(got[i]))) for i in bad[:6]]


@pytest.fixture(scope="module")
def golden_tags(golden):
    return _expected(golden, golden.expect)


@pytest.fixture(scope="module")
def strict_golden(golden):
    """The table test_strict_gpu.py uses: the independent Python verifier on every golden vector."""
    s = np.array(_strict_ref.verify_batch(golden), np.int8)
    s.setflags(write=False)
    return s


def test_golden_set_covers_both_tag_cases(golden, golden_tags):
    """At least one s-window vector (reference 0 without a multiply) that
    still carries its hash, and at least one reference -1 (tag 0)."""
    cls = lambda name: golden.cls == _golden.CLASSES.index(name)
    window = cls("s_window") & (golden.expect == 0)
    assert window.any() and (golden_tags[window] != 0).all()
    rejected = golden.expect == -1
    assert rejected.any() and (cls("s_range") | cls("malleate"))[rejected].any()
    assert (golden_tags[rejected] == 0).all() and (golden_tags[~rejected] != 0).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_golden_vectors_every_kernel_both_modes(engine, golden, golden_tags, strict_golden, kernel):
    from firedancer_amd import ed25519
    try:
        ed25519.select_dsm_kernel(kernel)
        for mode, want_err in ((ed25519.MODE_REFERENCE, golden.expect), (ed25519.MODE_STRICT, strict_golden)):
            engine.set_mode(mode)
            err, tag = engine.verify_soa(golden.pub, golden.sig, golden.msg_off, golden.msg_sz, golden.blob, want_tags=True)
            assert tag.dtype == np.uint64 and tag.shape == (len(golden),)
            assert np.array_equal(err, want_err), (mode, _bad(err, want_err))
            assert np.array_equal(tag, golden_tags), (mode, _bad(tag, golden_tags))   # same tags in both modes
    finally:
        engine.set_mode(ed25519.MODE_REFERENCE)
        ed25519.select_dsm_kernel("default")


# ---- ragged sizes, ring reuse, the three host calls -------------------------------

@pytest.fixture(scope="module")
def edge():
    """200 signatures whose messages cycle through the padding-edge sizes;
    one in seven corrupted: a flipped message bit (-3, hash tag), s >= L (-1,
    tag 0), an s in the reference's accept window (0, hash tag)."""
    from firedancer_amd import ed25519
    n = 200
    rng = np.random.default_rng(555)
    sz = np.array([EDGE_SIZES[i % len(EDGE_SIZES)] for i in range(n)], np.uint32)
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint32)
    blob = rng.integers(0, 256, int(sz.sum()) + 1, dtype=np.uint8)
    pub, sig = ed25519.sign_batch(rng.integers(0, 256, (n, 32), dtype=np.uint8), blob, off, sz)
    for k, i in enumerate(range(3, n, 7)):
        kind = k % 3 if sz[i] else 1 + k % 2
        if kind == 0:
            blob[off[i] + int(rng.integers(0, sz[i]))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            sig[i, 32:] = 0xff
        else:
            sig[i, 32:] = 0
            sig[i, 52], sig[i, 63] = 1, 0x10
    b = _golden.Batch(pub, sig, off, sz, blob)
    err = _oracle.verify_batch(b)
    assert set(err.tolist()) == {0, -1, -3}
    tags = _expected(b, err)
    assert (tags[err == -1] == 0).all() and (tags[err != -1] != 0).all()
    for a in (pub, sig, off, sz, blob, err):
        a.setflags(write=False)
    return b, err, tags


def _three(e, b, n, want_tags=True):
    """(err, tag) of the first n signatures through verify_batch, verify_soa and verify_soa_registered."""
    from firedancer_amd import ed25519
    out = {"batch": e.verify_batch([b.msg(i) for i in range(n)], [bytes(s) for s in b.sig[:n]], [bytes(p) for p in b.pub[:n]],
                                   want_tags=want_tags),
           "soa": e.verify_soa(b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob, want_tags=want_tags)}
    r = ed25519.RegisteredPlanes(b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob)
    try:
        out["registered"] = e.verify_soa_registered(r[0], r[1], r[2], r[3], r[4], want_tags=want_tags)
    finally:
        r.close()
    return out


def _check_three(e, b, n, want_err, want_tag):
    for name, (err, tag) in _three(e, b, n).items():
        assert np.array_equal(err, want_err[:n]), (name, n, _bad(err, want_err[:n]))
        assert np.array_equal(tag, want_tag[:n]), (name, n, _bad(tag, want_tag[:n]))
    for name, err in _three(e, b, n, want_tags=False).items():       # right after, on the same engine
        assert np.array_equal(err, want_err[:n]), (name, n)


@pytest.mark.parametrize("kernel", ["default", "k_dsm"])
def test_ragged_sizes_three_calls(engine, edge, kernel):
    """n around the wave size, through the latency kernels (registered: the
    in-place path) and with the throughput kernel forced (registered: DMA)."""
    from firedancer_amd import ed25519
    b, err, tags = edge
    try:
        ed25519.select_dsm_kernel(kernel)
        for n in (1, 2, 63, 64, 65, 129):
            _check_three(engine, b, n, err, tags)
    finally:
        ed25519.select_dsm_kernel("default")


@pytest.mark.parametrize("kernel", ["default", "k_dsm"])
def test_ring_reuse_four_chunks_on_two_slots(edge, kernel):
    """batch_max = 64 and 200 signatures: four chunks round a two-slot ring,
    so each slot's tags are drained before the slot is reused."""
    from firedancer_amd import ed25519
    b, err, tags = edge
    e = ed25519.Engine(device=0, batch_max=64, blob_max=64 * 1232)
    try:
        ed25519.select_dsm_kernel(kernel)
        _check_three(e, b, len(b), err, tags)
    finally:
        ed25519.select_dsm_kernel("default")
        e.close()


# ---- device-resident path ------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """2048 fresh signatures of 0..400 B, 10 % corrupted, with the oracle's verdicts."""
    from test_gpu_parity import _sign_stream
    b = _sign_stream(4242, 2048, 0, 400, True)
    err = _oracle.verify_batch(b)
    err.setflags(write=False)
    return b, err, _expected(b, err)


@pytest.mark.parametrize("n", [65, 2048])
def test_device_path_tags_dev(mixed, n):
    """verify_dev then tags_dev; strict mode leaves the same tags; nothing is written past d_tag[n)."""
    from firedancer_amd import ed25519, hip
    b, err, tags = mixed
    st = hip.Stream()
    bufs = [hip.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob)]
    d_err, d_ws = hip.DeviceBuffer(n), hip.DeviceBuffer(ed25519.workspace_footprint(n))
    pad = 32
    for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
        d_tag = hip.DeviceBuffer.from_array(np.full(n + pad, 0x5555555555555555, np.uint64))
        ed25519.verify_dev(n, *[x.ptr for x in bufs], d_err.ptr, d_ws.ptr, st.handle, mode=mode)
        ed25519.tags_dev(n, d_ws.ptr, d_tag.ptr, st.handle)
        st.synchronize()
        got = d_tag.to_array(np.uint64, n + pad)
        assert np.array_equal(got[:n], tags[:n]), (mode, _bad(got[:n], tags[:n]))
        assert (got[n:] == 0x5555555555555555).all()
        if mode == ed25519.MODE_REFERENCE:
            assert np.array_equal(d_err.to_array(np.int8, n), err[:n])
        # an output that is only 8-aligned takes the one-tag-per-lane form
        ed25519.tags_dev(n, d_ws.ptr, d_tag.ptr + 8, st.handle)
        st.synchronize()
        got = d_tag.to_array(np.uint64, n + pad)
        assert np.array_equal(got[1:n + 1], tags[:n]) and (got[n + 1:] == 0x5555555555555555).all()


# ---- transactions ------------------------------------------------------------------------

def _sig_fields(p):
    """(nsig, message offset, offset of the first signer's public key) of a well-formed wire transaction."""
    n = p[0]
    m = 1 + 64 * n
    a = m + (1 if p[m] & 0x80 else 0) + 3
    a += 1 if p[a] < 0x80 else 2
    return n, m, a


def _tag(msg, sig, pub):
    return int.from_bytes(hashlib.sha512(bytes(sig[:32]) + bytes(pub) + bytes(msg)).digest()[:8], "little")


@pytest.fixture(scope="module")
def txn_batch():
    """1-, 2- and 12-signer transactions (12 is the most a well-formed payload
    within the MTU holds), one with a corrupted signature, and two payloads
    that fail to parse: a 19-signer one -- 19 is the most signature slots a
    payload within the MTU reserves, 1 + 64 * 19 <= 1232, and what is left
    cannot hold 19 addresses, so all 19 slots are skipped -- and a truncated
    one that reserves no slot.  37 slots in all."""
    one, _ = _txn.build_txns(901, 2, nsig_lo=1, nsig_hi=1, msg_hi=300)
    two, _ = _txn.build_txns(902, 2, nsig_lo=2, nsig_hi=2, msg_hi=300)
    twelve, _ = _txn.build_txns(903, 1, nsig_lo=12, nsig_hi=12)
    rng = np.random.default_rng(904)
    nineteen = bytes([19]) + rng.integers(0, 256, 1231, dtype=np.uint8).tobytes()
    corrupt = bytearray(two[0])
    corrupt[1 + 64 + 5] ^= 0x20                                   # R of its second signature
    pays = [one[0], bytes(corrupt), nineteen, one[1], one[0][:40], twelve[0], two[1]]
    blob, off, sz = _txn.pack(pays)
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert ebase.tolist() == [0, 1, 3, 22, 23, 23, 35, 37]
    assert eterr.tolist() == [0, -3, -4, 0, -4, 0, 0] and eserr[1:3].tolist() == [0, -3]
    stag = np.zeros(37, np.uint64)
    ttag = np.zeros(len(pays), np.uint64)
    for t, p in enumerate(pays):
        if eterr[t] == -4:
            continue
        n, m, a = _sig_fields(p)
        for k in range(n):
            if eserr[ebase[t] + k] != -1:
                stag[ebase[t] + k] = _tag(p[m:], p[1 + 64 * k:65 + 64 * k], p[a + 32 * k:a + 32 * k + 32])
        ttag[t] = stag[ebase[t]]
    assert (ttag[eterr != -4] != 0).all() and len(set(stag[stag != 0].tolist())) == 18
    return blob, off, sz, eterr, ebase, eserr, ttag, stag


def _check_txns(out, txn_batch):
    blob, off, sz, eterr, ebase, eserr, ttag, stag = txn_batch
    terr, base, serr, got_t, got_s = out
    assert np.array_equal(terr, eterr) and np.array_equal(base, ebase) and np.array_equal(serr, eserr)
    assert np.array_equal(got_t, ttag), _bad(got_t, ttag)
    assert np.array_equal(got_s, stag), _bad(got_s, stag)


def test_transactions_host_calls(engine, txn_batch):
    """One chunk; then an engine whose batch_max forces two (22 + 1 + 0 slots, then 12 + 2); then without sig_err."""
    from firedancer_amd import ed25519
    blob, off, sz = txn_batch[:3]
    _check_txns(engine.verify_txns(blob, off, sz, want_sigs=True, want_tags=True), txn_batch)
    small = ed25519.Engine(device=0, batch_max=24, blob_max=1 << 16)
    try:
        _check_txns(small.verify_txns(blob, off, sz, want_sigs=True, want_tags=True), txn_batch)
        terr, got_t, got_s = small.verify_txns(blob, off, sz, want_tags=True)
        assert np.array_equal(terr, txn_batch[3]) and np.array_equal(got_t, txn_batch[6]) and np.array_equal(got_s, txn_batch[7])
        terr, base, serr = small.verify_txns(blob, off, sz, want_sigs=True)          # right after, untagged
        assert np.array_equal(terr, txn_batch[3]) and np.array_equal(serr, txn_batch[5])
    finally:
        small.close()


def test_transactions_device_path(txn_batch):
    from firedancer_amd import ed25519, hip, workload
    blob, off, sz, eterr, ebase, eserr, ttag, stag = txn_batch
    n = len(off)
    tbase, slots = ed25519.txn_slots(blob, off, sz)
    d = [hip.DeviceBuffer.from_array(a) for a in (blob, off, sz, tbase)]
    d_terr, d_serr = hip.DeviceBuffer(n), hip.DeviceBuffer(slots)
    d_ws = hip.DeviceBuffer(workload._bind().fd_ed25519_amd_txn_workspace_footprint(n, slots))
    pad = 8
    st = hip.Stream()
    for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
        d_tt = hip.DeviceBuffer.from_array(np.full(n + pad, 0x5555555555555555, np.uint64))
        d_st = hip.DeviceBuffer.from_array(np.full(slots + pad, 0x5555555555555555, np.uint64))
        ed25519.verify_txns_dev(n, slots, *[b.ptr for b in d], d_terr.ptr, d_serr.ptr, d_ws.ptr, st.handle, mode=mode)
        ed25519.txn_tags_dev(n, d[3].ptr, d_ws.ptr, d_tt.ptr, st.handle)
        ed25519.tags_dev(slots, d_ws.ptr, d_st.ptr, st.handle)
        st.synchronize()
        got_t, got_s = d_tt.to_array(np.uint64, n + pad), d_st.to_array(np.uint64, slots + pad)
        assert np.array_equal(got_t[:n], ttag) and (got_t[n:] == 0x5555555555555555).all(), (mode, _bad(got_t[:n], ttag))
        assert np.array_equal(got_s[:slots], stag) and (got_s[slots:] == 0x5555555555555555).all(), (mode, _bad(got_s[:slots], stag))
        if mode == ed25519.MODE_REFERENCE:
            assert np.array_equal(d_terr.to_array(np.int8, n), eterr) and np.array_equal(d_serr.to_array(np.int8, slots), eserr)


# ---- multi-device -------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_engine_tags_equal_single_engine(engine, mixed, txn_batch, devices):
    """Every shard writes its tags at its shard offset (per-signature
    transaction tags: at sig_base numbering over the whole batch)."""
    from firedancer_amd import ed25519
    b, err, tags = mixed
    n = 1000
    m = ed25519.MultiEngine(devices, batch_max=512, blob_max=512 * 1232)
    try:
        one = engine.verify_soa(b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob, want_tags=True)
        got = m.verify_soa(b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob, want_tags=True)
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]), _bad(got[1], one[1])
        assert np.array_equal(got[0], err[:n]) and np.array_equal(got[1], tags[:n])
        assert np.array_equal(m.verify_soa(b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob), err[:n])
        blob, off, sz = txn_batch[:3]
        one = engine.verify_txns(blob, off, sz, want_sigs=True, want_tags=True)
        got = m.verify_txns(blob, off, sz, want_sigs=True, want_tags=True)
        for x, y in zip(got, one):
            assert np.array_equal(x, y)
        _check_txns(got, txn_batch)
    finally:
        m.close()
