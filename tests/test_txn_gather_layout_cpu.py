"""CPU: fd_ed25519_amd_txn_gather_layout, the one rule that sizes a chunk of
verify_txns_registered -- the first payload always, further ones while the
count stays <= cap, the signature-slot total stays <= cap and the padded byte
total (sizes rounded up to 16) stays <= blob_cap -- with its Python mirror
ed25519.txn_gather_layout, and fd_ed25519_amd_txn_slots_ptrs against
fd_ed25519_amd_txn_slots.  No device."""
import numpy as np

import _txn
from firedancer_amd import ed25519


def _both(sz, slots, cap, blob_cap):
    """(count, dst, slot_cnt) of the C function, checked equal to the Python mirror's."""
    c, dst, ns = ed25519.txn_gather_layout_c(sz, slots, cap, blob_cap)
    pc, pdst, pns = ed25519.txn_gather_layout(sz, slots, cap, blob_cap)
    assert c == pc and ns == pns and np.array_equal(dst, pdst), (list(sz)[:8], list(slots)[:8], cap, blob_cap)
    return c, dst, ns


def _pad(s):
    return (int(s) + 15) & ~15


def test_edge_sizes_and_offsets():
    sz = [0, 1, 15, 16, 17, 1232]
    c, dst, ns = _both(sz, [0, 0, 0, 0, 0, 1], 64, 1 << 20)
    assert c == 6 and ns == 1
    assert dst.tolist() == [0, 0, 16, 32, 48, 80]          # 0 -> 0, 1 -> 16, 15 -> 16, 16 -> 16, 17 -> 32
    assert dst[-1] + _pad(1232) == 80 + 1232


def test_chunk_ends_at_count():
    c, dst, ns = _both([100] * 100, [1] * 100, 64, 1 << 20)
    assert c == 64 and ns == 64 and dst.tolist() == [112 * k for k in range(64)]
    c, _, ns = _both([100] * 64, [1] * 64, 64, 1 << 20)
    assert c == 64 and ns == 64
    # payloads without a slot still count
    c, _, ns = _both([10] * 100, [0] * 100, 64, 1 << 20)
    assert c == 64 and ns == 0
    c, _, _ = _both([10] * 5, [0] * 5, 1, 1 << 20)
    assert c == 1


def test_chunk_ends_where_the_next_padded_size_would_pass_blob_cap():
    # 3 x 1232 -> 3696 padded bytes; a fourth would make 4928 > 4096
    c, dst, ns = _both([1232] * 10, [1] * 10, 64, 4096)
    assert c == 3 and ns == 3 and dst.tolist() == [0, 1232, 2464]
    # padded, not raw, sizes count
    c, _, _ = _both([1] * 10, [0] * 10, 64, 64)
    assert c == 4
    c, _, _ = _both([1] * 10, [0] * 10, 64, 63)
    assert c == 3


def test_chunk_ends_where_the_next_slots_would_pass_cap():
    # five 12-signer payloads are 60 slots; a sixth would make 72 > 64
    sz = [1 + 64 * 12 + 200] * 10
    c, dst, ns = _both(sz, [12] * 10, 64, 1 << 20)
    assert c == 5 and ns == 60 and dst.tolist() == [_pad(sz[0]) * k for k in range(5)]
    # exactly full: 12 x 5 + 4 = 64
    c, _, ns = _both(sz, [12] * 5 + [4] + [1] * 4, 64, 1 << 20)
    assert c == 6 and ns == 64
    # a payload whose slots alone equal cap is taken first, alone
    c, _, ns = _both(sz[:3], [8, 1, 1], 8, 1 << 20)
    assert c == 1 and ns == 8


def test_first_is_taken_even_past_a_blob_cap_that_is_no_multiple_of_16():
    blob_cap = 1232 + 7
    c, dst, ns = _both([blob_cap, 0, 0], [1, 0, 0], 64, blob_cap)
    assert c == 1 and ns == 1 and dst.tolist() == [0]
    # the same payload later in the list ends the chunk before it, then opens the next one
    c, _, _ = _both([16, blob_cap], [0, 1], 64, blob_cap)
    assert c == 1
    c, dst, _ = _both([blob_cap], [1], 64, blob_cap)
    assert c == 1 and dst.tolist() == [0]


def test_empty():
    c, dst, ns = _both([], [], 64, 4096)
    assert c == 0 and dst.size == 0 and ns == 0
    c, dst, ns = _both(np.zeros(0, np.uint64), np.zeros(0, np.uint32), 1, 1)
    assert c == 0 and dst.size == 0 and ns == 0


def test_python_mirror_equals_c_on_random_lists():
    rng = np.random.default_rng(20263)
    for k in range(1000):
        n = int(rng.integers(0, 80))
        top = int(rng.choice([1, 17, 300, 1233]))
        sz = rng.integers(0, top, n)
        cap = int(rng.integers(1, 70))
        slots = rng.integers(0, min(cap, 19) + 1, n)
        blob_cap = int(rng.choice([1232, 1239, 4096, 5000, 20000, 1 << 20]))
        c, dst, ns = _both(sz, slots, cap, blob_cap)
        assert c <= cap and (n == 0 or c >= 1)
        assert ns == int(slots[:c].sum()) and (c <= 1 or ns <= cap)
        if c:
            assert (dst % 16 == 0).all() and (np.diff(dst.astype(np.int64)) >= 0).all()
            total = int(dst[c - 1]) + _pad(sz[c - 1])
            assert c == 1 or total <= blob_cap
            if c < n and c < cap and ns + int(slots[c]) <= cap:   # ended on the byte bound: the next one does not fit
                assert int(sz[c]) > blob_cap or total + _pad(sz[c]) > blob_cap


def _pointers(payloads):
    """The payloads packed back to back (kept alive by the caller) and a pointer to each."""
    blob, off, sz = _txn.pack(payloads)
    return blob, off, sz, np.uint64(blob.ctypes.data) + off.astype(np.uint64)


def test_txn_slots_ptrs_equals_txn_slots_on_packed_payloads():
    fx = [f.payload for f in _txn.load_fixtures()]
    pays = list(fx)
    pays += [b"", b"\x00" + bytes(100), b"\x80" + bytes(300)]             # empty; a first byte of 0, of 128
    pays += [b"\x02" + bytes(128), b"\x02" + bytes(127), b"\x01" + bytes(64), b"\x01" + bytes(63), b"\x01"]   # 64 k <= sz - 1, or not
    pays += [b"\x13" + bytes(1231), b"\x14" + bytes(1231), b"\x7f" + bytes(1231), b"\xff" + bytes(50)]
    pays += [fx[0][:k] for k in (1, 2, 64, 65, 66, len(fx[0]) - 1)]
    blob, off, sz, ptr = _pointers(pays)
    want, wtot = ed25519.txn_slots(blob, off, sz)
    got, gtot = ed25519.txn_slots_ptrs(ptr, sz)
    assert gtot == wtot and np.array_equal(got, want)
    d = np.diff(want.astype(np.int64)).tolist()
    assert d[3:11] == [0, 0, 0, 2, 0, 1, 0, 0] and d[11:15] == [19, 0, 0, 0] and wtot > 30
    # a pointer is not looked at when its size is 0 (NULL, or an address that is no memory at all)
    ptr2, sz2 = ptr.copy(), sz.astype(np.uint64)
    ptr2[3] = 0
    ptr2[0], sz2[0] = 8, 0
    got2, _ = ed25519.txn_slots_ptrs(ptr2, sz2)
    assert np.array_equal(np.diff(got2.astype(np.int64))[1:], np.diff(want.astype(np.int64))[1:]) and got2[1] == 0


def test_declared_and_exported():
    import test_abi
    names = test_abi.declared_functions()
    for n in ("fd_ed25519_amd_verify_txns_registered", "fd_ed25519_amd_verify_txns_registered_tag",
              "fd_ed25519_amd_txn_slots_ptrs", "fd_ed25519_amd_txn_gather_layout"):
        assert n in names, n
        assert hasattr(ed25519.lib(), n), n


def test_entry_points_refuse_null_arguments_without_a_device():
    """ERR_INVAL before any device call: no engine, with or without arrays."""
    L = ed25519.lib()
    assert L.fd_ed25519_amd_verify_txns_registered(None, 0, None, None, None, None, None) == -10
    assert L.fd_ed25519_amd_verify_txns_registered(None, 4, None, None, None, None, None) == -10
    assert L.fd_ed25519_amd_verify_txns_registered_tag(None, 0, None, None, None, None, None, None, None) == -10
    assert L.fd_ed25519_amd_verify_txns_registered_tag(None, 4, None, None, None, None, None, None, None) == -10
