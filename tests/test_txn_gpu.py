"""Transaction front end on the GPU (through the C-ABI, include/fd_txn_amd.h):
k_txn_parse vs the compiled reference parser's fixture, and the
multi-signer batch verdicts of fd_ed25519_amd_verify_txns vs the CPU oracle.
Bar: bit-exact footprints, descriptor bytes and codes.
"""
import numpy as np
import pytest

import _oracle
import _txn

pytestmark = pytest.mark.gpu

STRIDE = 3584   # >= FD_TXN_MAX_SZ, even


def _gpu_parse(payloads, want_desc=True):
    from firedancer_amd import ed25519, hip
    blob, off, sz = _txn.pack(payloads)
    n = len(payloads)
    d_blob, d_off, d_sz = (hip.DeviceBuffer.from_array(a) for a in (blob, off, sz))
    d_fp = hip.DeviceBuffer(4 * max(n, 1))
    d_out = hip.DeviceBuffer(STRIDE * max(n, 1)) if want_desc else None
    stream = hip.Stream()
    ed25519.txn_parse_dev(n, d_blob.ptr, d_off.ptr, d_sz.ptr, d_fp.ptr, d_out.ptr if want_desc else None,
                          STRIDE if want_desc else 0, stream.handle)
    stream.synchronize()
    fp = d_fp.to_array(np.uint32, n)
    out = d_out.to_array(np.uint8, STRIDE * n).reshape(n, STRIDE) if want_desc else None
    return fp, out


def test_gpu_parse_reference_mutations():
    """All mutations of the reference's three fixture transactions: the
    GPU footprint equals the reference's for every one, and the digest of
    the accepted descriptors equals the reference's."""
    for f in _txn.load_fixtures():
        muts = _txn.mutation_list(f.payload)
        fp, out = _gpu_parse(muts)
        bad = np.nonzero(fp != f.footprint)[0]
        assert bad.size == 0, [(int(i), int(fp[i]), int(f.footprint[i]), int(f.line[i])) for i in bad[:10]]
        d = _txn.FNV0
        for k in np.nonzero(fp)[0]:
            d = _txn.fnv(d, out[k, :fp[k]].tobytes())
        assert d == f.digest


def test_gpu_parse_synthetic_fuzz():
    """Random byte edits and truncations of synthetic legacy/v0 transactions:
    GPU footprint and descriptor bytes vs the oracle."""
    rng = np.random.default_rng(5)
    base, _ = _txn.build_txns(21, 40, nsig_hi=4, msg_hi=400)
    pays = []
    for p in base:
        pays.append(p)
        for _ in range(40):
            q = bytearray(p)
            for _ in range(int(rng.integers(1, 3))):
                q[int(rng.integers(0, len(q)))] = int(rng.integers(0, 256))
            if rng.random() < 0.2:
                q = q[:int(rng.integers(0, len(q) + 1))]
            pays.append(bytes(q))
    fp, out = _gpu_parse(pays)
    for k, p in enumerate(pays):
        efp, eout, _ = _oracle.txn_parse(p)
        assert int(fp[k]) == efp, k
        if efp:
            assert out[k, :efp].tobytes() == eout, k


def test_gpu_parse_edge_sizes():
    """Empty payload, a single byte, and a payload above USHORT_MAX."""
    fp, _ = _gpu_parse([b"", b"\x01", b"\x01" + b"\0" * 70000], want_desc=False)
    assert fp.tolist() == [0, 0, 0]


def test_verify_txns_reference_fixtures(engine):
    fx = _txn.load_fixtures()
    blob, off, sz = _txn.pack([f.payload for f in fx])
    terr, base, serr = engine.verify_txns(blob, off, sz, want_sigs=True)
    assert terr.tolist() == [0, 0, 0]
    assert base.tolist() == [0, 4, 5, 6] and serr.tolist() == [0] * 6


def _mixed_batch(seed, count):
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


def test_verify_txns_mixed_vs_oracle(engine):
    """600 synthetic multi-signer transactions (1..12 signers, 64..1232-B
    messages, legacy and v0) with corruptions: per-transaction verdicts,
    signature numbering and per-signature codes vs the oracle."""
    pays = _mixed_batch(31, 600)
    blob, off, sz = _txn.pack(pays)
    terr, base, serr = engine.verify_txns(blob, off, sz, want_sigs=True)
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert np.array_equal(base, ebase)
    assert np.array_equal(serr, eserr), np.nonzero(serr != eserr)[0][:10]
    assert np.array_equal(terr, eterr)
    assert set(np.unique(terr).tolist()) >= {0, -4}


def test_verify_txns_chunked_small_engine():
    """An engine smaller than the batch: transactions are split into
    double-buffered chunks by count, payload bytes and signature slots."""
    from firedancer_amd import ed25519
    pays = _mixed_batch(32, 150)
    blob, off, sz = _txn.pack(pays)
    eng = ed25519.Engine(device=0, batch_max=40, blob_max=6000)
    try:
        terr, base, serr = eng.verify_txns(blob, off, sz, want_sigs=True)
    finally:
        eng.close()
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert np.array_equal(terr, eterr) and np.array_equal(serr, eserr)


def test_verify_txns_empty_and_limits(engine):
    from firedancer_amd import ed25519
    t = engine.verify_txns(np.zeros(4, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert t.shape == (0,)
    with pytest.raises(ed25519.EngineError):
        engine.verify_txns(np.zeros(1300, np.uint8), np.zeros(1, np.uint32), np.full(1, 1233, np.uint32))


def test_synth_txn_workload_and_device_path(engine):
    """Config-4 workload (GPU-signed multi-signer transactions, 64..1232-B
    messages): every transaction parses and verifies; the device-resident
    entry point agrees with the host-staged one and with the oracle, also
    after corruptions."""
    from firedancer_amd import hip, workload
    payload, toff, tsz, tbase = workload.txn_batch(3000, 77)
    assert (tsz <= 1232).all() and int(tbase[-1]) > 2500
    rng = np.random.default_rng(1)
    bad = rng.choice(toff.size, 40, replace=False)
    for t in bad[:20]:
        payload[toff[t] + 1 + int(rng.integers(0, 64))] ^= 0x20         # a signature byte
    for t in bad[20:]:
        payload[toff[t] + tsz[t] - 1] ^= 0x01                           # last byte (data or LUT count)
    dev = workload.TxnDevice(payload, toff, tsz, tbase)
    st = hip.Stream()
    dev.run(st.handle)
    st.synchronize()
    terr, serr = dev.verdicts()
    eterr, ebase, eserr = _oracle.txn_verify_batch(payload, toff, tsz)
    assert np.array_equal(ebase, tbase)
    assert np.array_equal(terr, eterr) and np.array_equal(serr, eserr)
    h_terr, h_base, h_serr = engine.verify_txns(payload, toff, tsz, want_sigs=True)
    assert np.array_equal(h_terr, terr) and np.array_equal(h_serr, serr)
    ok = np.setdiff1d(np.arange(toff.size), bad)
    assert (terr[ok] == 0).all() and (terr[bad] != 0).all()


def test_config4_shard_full_size_properties():
    """configs[3] at the size of one GPU's shard of 2^24 signatures over 2
    GPUs: 2^23 signatures in multi-signer transactions (64..1232-B
    messages).  Every signature is valid: each rejected transaction must
    hold a limb-compare false reject, confirmed by the oracle."""
    from firedancer_amd import hip, workload
    payload, toff, tsz, tbase = workload.txn_batch(1 << 23, 424242)
    dev = workload.TxnDevice(payload, toff, tsz, tbase)
    st = hip.Stream()
    dev.run(st.handle)
    st.synchronize()
    terr, serr = dev.verdicts()
    assert dev.slot_cnt >= (1 << 23) * 0.99
    bad = np.nonzero(terr)[0]
    assert bad.size <= 40, bad.size
    if bad.size:
        eterr, _, _ = _oracle.txn_verify_batch(payload, toff[bad], tsz[bad])
        assert np.array_equal(eterr, terr[bad]) and (eterr == -3).all()
    assert (serr != 0).sum() == bad.size


# ---- the grammar limits (tests/_txn.py: limit_cases) and payloads above the MTU ----

CANARY = 0xA5


@pytest.fixture(scope="module")
def limits():
    """[(name, payload, (footprint, descriptor, line))] by the oracle, computed once."""
    return [(n, p, _oracle.txn_parse(p)) for n, p in _txn.limit_cases()]


def test_gpu_parse_limit_cases(limits):
    """Every limit case in one launch, descriptor rows STRIDE apart: the
    footprint is the oracle's for every case (above the stride too), and the
    descriptor of an accepted case that fits its row is the oracle's."""
    fp, out = _gpu_parse([p for _, p, _ in limits])
    bad = [(n, int(fp[k]), w[0], w[2]) for k, (n, _, w) in enumerate(limits) if int(fp[k]) != w[0]]
    assert not bad, bad[:10]
    assert int(fp.max()) == 217910
    checked = 0
    for k, (n, _, (efp, eout, _)) in enumerate(limits):
        if 0 < efp <= STRIDE:
            assert out[k, :efp].tobytes() == eout, n
            checked += 1
    assert checked >= 25


def _whole_records_end(ninstr, nlut, cap):
    """End of the last descriptor record (header, then 10-B instruction
    records, then 8-B table records) that ends at or before cap."""
    end = 20 + 10 * min(ninstr, (cap - 20) // 10)
    if end == 20 + 10 * ninstr:
        end += 8 * min(nlut, (cap - end) // 8)
    return end


@pytest.mark.parametrize("stride", [3570, 3584])
def test_gpu_parse_descriptor_writes_stay_in_row(limits, stride):
    """Payloads whose footprint exceeds the row stride (the 356-instruction
    one, 3580, only the smaller of the two strides), each followed by an
    empty payload's row, in a canary-filled buffer with a tail guard: nothing
    is written outside the payload's own row, the row holds the header and
    exactly the records that end at or before the stride (byte-equal to the
    oracle's), and the footprint is still the reference's.  At stride 3570
    the 355th instruction record of the 356-instruction payload ends exactly
    at the capacity: it is present, the 356th is not.  At stride 3584 the
    same holds for the 8th table record of the 350 + 20 payload.

    The guard covers the largest descriptor any payload can have from the
    start of the last row, so even a parser that bounds nothing stays inside
    the allocation and fails the assertions below."""
    from firedancer_amd import ed25519, hip
    by = {n: (p, w) for n, p, w in limits}
    over = [("max_size", 21789, 0), ("max_size_trailing", 21788, 0), ("instr_356", 356, 0), ("instr_350_lut_20", 350, 20)]
    pays = []
    for n, _, _ in over:
        pays += [by[n][0], b""]
    rows = len(pays)
    guard = _oracle.txn_desc_max()
    blob, off, sz = _txn.pack(pays)
    d_blob, d_off, d_sz = (hip.DeviceBuffer.from_array(a) for a in (blob, off, sz))
    d_fp = hip.DeviceBuffer(4 * rows)
    d_out = hip.DeviceBuffer.from_array(np.full(rows * stride + guard, CANARY, np.uint8))
    stream = hip.Stream()
    ed25519.txn_parse_dev(rows, d_blob.ptr, d_off.ptr, d_sz.ptr, d_fp.ptr, d_out.ptr, stride, stream.handle)
    stream.synchronize()
    fp = d_fp.to_array(np.uint32, rows)
    raw = d_out.to_array(np.uint8, rows * stride + guard)
    out, tail = raw[:rows * stride].reshape(rows, stride), raw[rows * stride:]
    assert (tail == CANARY).all(), np.nonzero(tail != CANARY)[0][:4]
    for r in range(1, rows, 2):
        assert fp[r] == 0 and (out[r] == CANARY).all(), (r, np.nonzero(out[r] != CANARY)[0][:4])
    for k, (n, ninstr, nlut) in enumerate(over):
        row = out[2 * k]
        efp, eout, _ = by[n][1]
        assert int(fp[2 * k]) == efp, n
        end = _whole_records_end(ninstr, nlut, stride)
        assert (row[end:] == CANARY).all(), (n, end, np.nonzero(row[end:] != CANARY)[0][:4])
        if efp:
            assert end == min(efp, end) and row[:end].tobytes() == eout[:end], n
        else:
            assert (row[:20] == CANARY).all(), n     # the header is stored on acceptance only
    assert _whole_records_end(356, 0, 3570) == 3570 and _whole_records_end(350, 20, 3584) == 3584
    assert _whole_records_end(350, 20, 3570) == 3568 and _whole_records_end(356, 0, 3584) == 3580


def test_verify_txns_dev_above_mtu():
    """fd_ed25519_amd_verify_txns_dev does not cap payloads at the MTU:
    validly signed transactions with 20, 64 and 127 signers (k_txn_parse's
    copy loop above the 19 signers an MTU payload can hold), and a copy of
    the 127-signer one whose last signature is corrupted.  tbase from
    fd_ed25519_amd_txn_slots; every verdict and per-signature code vs the
    oracle."""
    from firedancer_amd import ed25519, hip, workload
    pays = []
    for k, n in enumerate((20, 64, 127)):
        p, nsig = _txn.build_txns(50 + k, 1, nsig_lo=n, nsig_hi=n, mtu=65535)
        assert int(nsig[0]) == n and len(p[0]) > 1232
        pays += p
    q = bytearray(pays[2])
    q[1 + 64 * 126 + 40] ^= 0x08
    pays.append(bytes(q))
    blob, off, sz = _txn.pack(pays)
    tbase, tot = ed25519.txn_slots(blob, off, sz)
    assert np.diff(tbase.astype(np.int64)).tolist() == [20, 64, 127, 127]
    dev = workload.TxnDevice(blob, off, sz, tbase)
    st = hip.Stream()
    dev.run(st.handle)
    st.synchronize()
    terr, serr = dev.verdicts()
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert np.array_equal(ebase, tbase)
    assert np.array_equal(terr, eterr) and np.array_equal(serr, eserr)
    assert eterr[:3].tolist() == [0, 0, 0] and eterr[3] != 0
    assert (eserr[:-1] == 0).all() and eserr[-1] == eterr[3]


def test_verify_txns_dev_wrong_slot_count_fails_closed():
    """A caller's tbase that reserves one slot too many for one transaction
    and one too few for another (later bases shifted to match): k_txn_parse
    rejects both (FD_TXN_AMD_ERR_PARSE in txn_err and in every reserved
    slot) and verifies no subset of their signatures; the other six get the
    oracle's verdicts."""
    from firedancer_amd import ed25519, hip, workload
    pays, nsig = _txn.build_txns(61, 8, nsig_lo=2, nsig_hi=6)
    pays = [bytearray(p) for p in pays]
    pays[6][1 + 3] ^= 0x01                     # one honest failure among the six
    blob, off, sz = _txn.pack([bytes(p) for p in pays])
    good, _ = ed25519.txn_slots(blob, off, sz)
    cnt = np.diff(good.astype(np.int64))
    assert cnt.tolist() == nsig.tolist()
    cnt[2] += 1
    cnt[5] -= 1
    tbase = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    dev = workload.TxnDevice(blob, off, sz, tbase)
    st = hip.Stream()
    dev.run(st.handle)
    st.synchronize()
    terr, serr = dev.verdicts()
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert eterr[6] != 0 and (np.delete(eterr, 6) == 0).all()
    for t in range(8):
        got = serr[tbase[t]:tbase[t + 1]]
        if t in (2, 5):
            assert terr[t] == -4 and got.size == cnt[t] > 0 and (got == -4).all(), t
        else:
            assert terr[t] == eterr[t] and np.array_equal(got, eserr[ebase[t]:ebase[t + 1]]), t


def test_verify_txns_limit_cases_at_most_mtu(engine, limits):
    """The limit cases an MTU-capped caller can receive (at most 1232 B),
    through the host batch entry point: transaction verdicts, signature
    numbering and per-signature codes vs the oracle."""
    pays = [p for _, p, _ in limits if len(p) <= 1232]
    assert len(pays) >= 60 and any(len(p) == 1232 for p in pays)
    blob, off, sz = _txn.pack(pays)
    terr, base, serr = engine.verify_txns(blob, off, sz, want_sigs=True)
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    assert np.array_equal(base, ebase)
    assert np.array_equal(serr, eserr) and np.array_equal(terr, eterr)
    assert (eterr == -4).sum() >= 30 and (eterr != -4).sum() >= 10
