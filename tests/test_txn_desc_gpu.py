"""GPU: packed descriptors from the device-resident parse
(fd_txn_amd_parse_packed_dev: k_desc_bsum, k_desc_bscan, k_desc_store).

Expected values are the oracle's fd_txn_parse (footprint and descriptor
bytes, itself proven equal to the compiled reference's over the same
corpus), their 64-bit running sum and their concatenation; every comparison
is exact.  The descriptor buffer is filled with a poison byte first and has a
guard region behind it: a byte the kernels did not write, or wrote where they
must not, shows.

Shapes of the scan (fd_txn_dev.h): a block is 64 transactions (one lane
each); k_desc_bscan is one 64-lane workgroup that scans 64 block totals per
turn of its loop, so its loop takes a second turn from 64*64 + 1 = 4097
transactions and a third from 8193; there is no further level.  SCAN_COUNTS
are 0, 1, and one below, at and one above each of 64, 4096 and 8192."""
import numpy as np
import pytest

import _oracle
import _txn

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xC3, 4096
BLOCK = 64
SCAN_COUNTS = [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK * BLOCK - 1, BLOCK * BLOCK, BLOCK * BLOCK + 1,
               2 * BLOCK * BLOCK - 1, 2 * BLOCK * BLOCK, 2 * BLOCK * BLOCK + 1]

_parsed = {}


def oracle_desc(p):
    """The oracle's descriptor of payload p (b"" where it rejects it), cached."""
    p = bytes(p)
    d = _parsed.get(p)
    if d is None:
        fp, d, _ = _oracle.txn_parse(p)
        assert len(d) == fp
        _parsed[p] = d
    return d


def expected(pays):
    """(footprint u32[n], desc_off u64[n+1], the descriptors concatenated)."""
    ds = [oracle_desc(p) for p in pays]
    fp = np.array([len(d) for d in ds], np.uint32)
    off = np.zeros(len(pays) + 1, np.uint64)
    off[1:] = np.cumsum(fp, dtype=np.uint64)
    return fp, off, np.frombuffer(b"".join(ds), np.uint8)


def gpu_packed(pays, cap=None, room=None):
    """fd_txn_amd_parse_packed_dev over pays with desc_cap = cap (None: the
    exact total) on a buffer of room >= cap bytes (None: cap) followed by the
    guard, all POISON before the call.  Returns (footprint, desc_off, the
    whole buffer with its guard)."""
    from firedancer_amd import ed25519, hip
    n = len(pays)
    blob, off, sz = _txn.pack(pays)
    if cap is None:
        cap = int(expected(pays)[1][-1])
    room = cap if room is None else room
    assert room >= cap
    d_blob, d_off, d_sz = (hip.DeviceBuffer.from_array(a if a.size else np.zeros(1, a.dtype)) for a in (blob, off, sz))
    d_fp = hip.DeviceBuffer.from_array(np.full(max(n, 1), 0xDEADBEEF, np.uint32))
    d_doff = hip.DeviceBuffer.from_array(np.full(n + 1, 0xDEADBEEFDEADBEEF, np.uint64))
    d_desc = hip.DeviceBuffer.from_array(np.full(room + GUARD, POISON, np.uint8))
    d_scr = hip.DeviceBuffer.from_array(np.full(ed25519.txn_parse_packed_scratch_footprint(n), 0xEE, np.uint8))
    stream = hip.Stream()
    ed25519.txn_parse_packed_dev(n, d_blob.ptr, d_off.ptr, d_sz.ptr, d_fp.ptr, d_doff.ptr, d_desc.ptr, cap, d_scr.ptr,
                                 stream.handle)
    stream.synchronize()
    return d_fp.to_array(np.uint32, max(n, 1))[:n], d_doff.to_array(np.uint64, n + 1), d_desc.to_array(np.uint8, room + GUARD)


def check_whole(pays, got):
    fp, doff, buf = got
    efp, eoff, edesc = expected(pays)
    total = int(eoff[-1])
    assert np.array_equal(fp, efp), np.nonzero(fp != efp)[0][:8]
    assert doff.dtype == np.uint64 and np.array_equal(doff, eoff), np.nonzero(doff != eoff)[0][:8]
    assert np.array_equal(buf[:total], edesc), int(np.nonzero(buf[:total] != edesc)[0][0])
    assert (buf[total:] == POISON).all()                   # the guard, and nothing behind the last descriptor
    assert not (doff & np.uint64(1)).any()


# ---- 1. the whole corpus against the oracle ---------------------------------------

def test_packed_parse_over_the_fixture_mutations_and_the_grammar_limits():
    """The three reference fixtures with all their mutations and every
    limit_cases() payload of up to 65535 B -- the 21789-instruction one with
    its 217910-B descriptor among them -- in one batch."""
    pays = []
    for f in _txn.load_fixtures():
        pays.append(f.payload)
        pays += _txn.mutation_list(f.payload)
    lim = [p for _, p in _txn.limit_cases() if len(p) <= 65535]
    assert any(len(oracle_desc(p)) == 217910 for p in lim)
    pays += lim
    assert len(pays) > 16000
    efp, eoff, edesc = expected(pays)
    assert (efp == 0).sum() > 5000 and (efp != 0).sum() > 5000
    got = gpu_packed(pays)
    check_whole(pays, got)
    # no poison is left inside [0, total): every byte there equals the oracle's, and the oracle's descriptors
    # of this corpus hold the poison value only where the GPU's do (compared above), so count it once more
    assert int((got[2][:int(eoff[-1])] == POISON).sum()) == int((edesc == POISON).sum())


# ---- 2. the scan's boundaries -----------------------------------------------------

ACCEPT = (_txn.mk(1, False, 0, 0, 1, []),                                   # 134 B, the smallest that parses: footprint 20
          _txn.mk(1, False, 0, 0, 2, [_txn.ins(1)]),                        # 30
          _txn.mk(2, True, 1, 0, 3, [_txn.ins(2, accts=b"\x00\x01"), _txn.EMPTY_IX], [_txn.lut(1, 1)]))   # 20 + 20 + 8
REJECT = (b"", b"\x01" * 40, _txn.mk(1, False, 0, 0, 2, [_txn.ins(1)], tail=b"\0"), _txn.mk(1, False, 0, 0, 2, [_txn.ins(2)]))


def scan_batch(n):
    """n short payloads: rejected ones at every block's first and last lane,
    the whole of blocks 1 and 65 and every fifth transaction, accepted ones of
    three footprints (20, 30, 48) elsewhere."""
    out = []
    for t in range(n):
        lane, blk = t % BLOCK, t // BLOCK
        if lane in (0, BLOCK - 1) or blk in (1, 65) or t % 5 == 3:
            out.append(REJECT[t % len(REJECT)])
        else:
            out.append(ACCEPT[(t // 2) % len(ACCEPT)])
    return out


def test_scan_batch_is_what_it_claims():
    assert [len(oracle_desc(p)) for p in ACCEPT] == [20, 30, 48] and not any(oracle_desc(p) for p in REJECT)
    fp = expected(scan_batch(2 * BLOCK * BLOCK + 1))[0]
    assert not fp[0::BLOCK].any() and not fp[BLOCK - 1::BLOCK].any()
    assert not fp[BLOCK:2 * BLOCK].any() and not fp[65 * BLOCK:66 * BLOCK].any() and fp[2 * BLOCK:3 * BLOCK].any()


@pytest.mark.parametrize("n", SCAN_COUNTS)
def test_scan_boundaries(n):
    pays = scan_batch(n)
    check_whole(pays, gpu_packed(pays))


# ---- 3. capacity ------------------------------------------------------------------

@pytest.mark.parametrize("where", ["mid", "end", "zero"])
def test_capacity_stores_whole_descriptors_below_the_cap_only(where):
    """desc_cap in the middle of a descriptor, exactly at a descriptor's end,
    and 0, on a buffer with room for everything: the offsets are complete,
    exactly the descriptors that end at or before the cap are stored, whole,
    and every other byte -- below the cap, at it and beyond -- keeps its
    poison."""
    pays = scan_batch(3 * BLOCK + 7)
    efp, eoff, edesc = expected(pays)
    total = int(eoff[-1])
    k = int(np.nonzero(efp)[0][70])                        # the 71st accepted transaction, in the third block
    cap = {"mid": int(eoff[k]) + int(efp[k]) // 2, "end": int(eoff[k + 1]), "zero": 0}[where]
    assert cap % 2 == 0 or where == "mid"
    fp, doff, buf = gpu_packed(pays, cap=cap, room=total)
    assert np.array_equal(fp, efp) and np.array_equal(doff, eoff) and int(doff[-1]) > cap
    want = np.full(total + GUARD, POISON, np.uint8)
    stored = 0
    for t in np.nonzero(efp)[0]:
        if int(eoff[t + 1]) <= cap:
            want[int(eoff[t]):int(eoff[t + 1])] = edesc[int(eoff[t]):int(eoff[t + 1])]
            stored += 1
    assert stored == {"mid": 70, "end": 71, "zero": 0}[where]
    assert np.array_equal(buf, want), np.nonzero(buf != want)[0][:8]
    assert (buf[cap:] == POISON).all()


def test_capacity_zero_without_a_buffer():
    """desc_cap == 0 admits d_desc == NULL: footprints and offsets only."""
    from firedancer_amd import ed25519, hip
    pays = scan_batch(BLOCK + 3)
    efp, eoff, _ = expected(pays)
    blob, off, sz = _txn.pack(pays)
    n = len(pays)
    d_blob, d_off, d_sz = (hip.DeviceBuffer.from_array(a) for a in (blob, off, sz))
    d_fp, d_doff = hip.DeviceBuffer(4 * n), hip.DeviceBuffer(8 * (n + 1))
    d_scr = hip.DeviceBuffer(ed25519.txn_parse_packed_scratch_footprint(n))
    stream = hip.Stream()
    ed25519.txn_parse_packed_dev(n, d_blob.ptr, d_off.ptr, d_sz.ptr, d_fp.ptr, d_doff.ptr, None, 0, d_scr.ptr, stream.handle)
    stream.synchronize()
    assert np.array_equal(d_fp.to_array(np.uint32, n), efp) and np.array_equal(d_doff.to_array(np.uint64, n + 1), eoff)
