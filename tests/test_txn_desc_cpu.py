"""CPU: the host-side surface of the packed descriptors (include/fd_txn_amd.h,
"Packed descriptors").

fd_txn_amd_desc_bound is what decides the capacity of every _desc call, so it
must never be below a footprint the parser can return: checked against the
oracle's fd_txn_parse over the three reference fixtures, every mutation of
them and every limit_cases() payload the parser can accept (up to 65535 B).
The argument checks of the two host calls that can fail before a device is
looked for are checked on a fake engine, as test_tags_cpu.py does."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import _oracle
import _txn

INVAL, DEVICE = -10, -11
MTU, MAX_SZ, PAYLOAD_MAX, MIN_SZ = 1232, 3570, 65535, 134
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound(sz):
    from firedancer_amd import ed25519
    return ed25519.txn_desc_bound(sz)


def test_bound_formula_and_edges():
    """0 below 134 B and above 65535 B; 20 + 10*((sz - 134)/3) between, capped
    at FD_TXN_MAX_SZ up to the MTU; never decreasing up to the MTU."""
    for sz in list(range(0, MIN_SZ)) + [PAYLOAD_MAX + 1, PAYLOAD_MAX + 2, 1 << 20, 1 << 32, (1 << 64) - 1]:
        assert _bound(sz) == 0, sz
    prev = 0
    for sz in range(MIN_SZ, PAYLOAD_MAX + 1):
        want = 20 + 10 * ((sz - MIN_SZ) // 3)
        if sz <= MTU:
            want = min(want, MAX_SZ)
        b = _bound(sz)
        assert b == want, sz
        assert b >= prev and (sz > MTU or b <= MAX_SZ), sz
        prev = b
    assert _bound(MIN_SZ) == 20 and _bound(MTU) == MAX_SZ and _bound(MTU + 1) == 20 + 10 * 366
    assert _bound(PAYLOAD_MAX) == 20 + 10 * 21800


def test_bound_covers_every_fixture_mutation():
    """The committed footprints of the compiled reference parser: every
    mutation of every fixture, and the fixtures themselves (the oracle)."""
    fx = _txn.load_fixtures()
    total = 0
    for f in fx:
        fp, _, _ = _oracle.txn_parse(f.payload)
        assert 0 < fp <= _bound(len(f.payload))
        muts = _txn.mutation_list(f.payload)
        assert len(muts) == f.footprint.size
        bound = np.array([_bound(len(m)) for m in muts], np.int64)
        bad = np.nonzero(f.footprint.astype(np.int64) > bound)[0]
        assert bad.size == 0, [(int(i), len(muts[i]), int(f.footprint[i]), int(bound[i])) for i in bad[:5]]
        total += len(muts)
    assert total > 16000
    # fixture 3 is where the bound is reached: its footprint is the bound of its size
    f3 = fx[2]
    assert _oracle.txn_parse(f3.payload)[0] == _bound(len(f3.payload))


def test_bound_covers_the_grammar_limits():
    """Every limit_cases() payload of up to 65535 B (a longer one is rejected
    by its size and has bound 0): the oracle's footprint is within the bound;
    the 355-instruction payload at the MTU and the 21789-instruction one at
    65535 B are among them."""
    seen = 0
    for name, p in _txn.limit_cases():
        fp, _, _ = _oracle.txn_parse(p)
        if len(p) > PAYLOAD_MAX:
            assert fp == 0 and _bound(len(p)) == 0, name
            continue
        assert fp <= _bound(len(p)), (name, len(p), fp, _bound(len(p)))
        seen += fp != 0
    assert seen >= 20
    by = dict(_txn.limit_cases())
    assert _oracle.txn_parse(by["mtu_355_instr"])[0] == _bound(len(by["mtu_355_instr"])) == MAX_SZ
    assert _oracle.txn_parse(by["max_size"])[0] == 217910 <= _bound(PAYLOAD_MAX)


ABI_C = r"""
#include "fd_txn_amd.h"
/* an assignment of each function to a pointer of its declared type: a
   mismatch is a compile error under -Werror */
ulong (*p_bound)( ulong ) = fd_txn_amd_desc_bound;
int (*p_packed)( ulong, uchar const *, uint const *, uint const *, uint *, ulong *, uchar *, ulong, void *, void * ) =
  fd_txn_amd_parse_packed_dev;
ulong (*p_scratch)( ulong ) = fd_txn_amd_parse_packed_scratch_footprint;
int (*p_desc)( fd_ed25519_amd_t *, ulong, uchar const *, uint const *, uint const *, ulong, schar *, uint *, schar *,
               ulong *, ulong *, ulong *, uchar *, ulong ) = fd_ed25519_amd_verify_txns_desc;
int (*p_rdesc)( fd_ed25519_amd_t *, ulong, void const * const *, ulong const *, schar *, uint *, schar *, ulong *,
                ulong *, ulong *, uchar *, ulong ) = fd_ed25519_amd_verify_txns_registered_desc;
int main( void ) {
  if( fd_txn_amd_desc_bound( 133UL ) != 0UL || fd_txn_amd_desc_bound( 134UL ) != 20UL ) return 1;
  if( fd_txn_amd_desc_bound( FD_TXN_AMD_MTU ) != FD_TXN_MAX_SZ ) return 2;
  if( fd_txn_amd_parse_packed_scratch_footprint( 0UL ) < 8UL ) return 3;
  if( fd_txn_amd_parse_packed_scratch_footprint( 6401UL ) < 8UL*101UL ) return 4;
  return 0;
}
"""


def test_abi_symbols_and_signatures(tmp_path):
    """The new symbols are exported, and a plain-C caller that includes only
    include/*.h compiles against the declared signatures and links."""
    from firedancer_amd import ed25519
    L = ed25519.lib()
    for name in ("fd_txn_amd_desc_bound", "fd_txn_amd_parse_packed_dev", "fd_txn_amd_parse_packed_scratch_footprint",
                 "fd_ed25519_amd_verify_txns_desc", "fd_ed25519_amd_verify_txns_registered_desc"):
        assert hasattr(L, name), name
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(ABI_C)
    libdir = os.path.join(ROOT, "firedancer_amd")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lfd_ed25519_amd", "-Wl,-rpath," + libdir, "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    z = ctypes.c_void_p(0)
    # the device-resident call's argument checks come before any device call
    assert L.fd_txn_amd_parse_packed_dev(1 << 32, z, z, z, z, z, z, 0, z, z) == INVAL
    assert L.fd_txn_amd_parse_packed_dev(0, z, z, z, z, z, z, 0, z, z) == INVAL          # d_desc_off is always written
    one = ctypes.c_void_p(4096)
    assert L.fd_txn_amd_parse_packed_dev(4, z, one, one, one, one, one, 64, one, z) == INVAL
    assert L.fd_txn_amd_parse_packed_dev(4, one, one, one, one, one, z, 64, one, z) == INVAL    # capacity without a buffer
    assert L.fd_txn_amd_parse_packed_dev(4, one, one, one, one, one, ctypes.c_void_p(4097), 64, one, z) == INVAL   # odd d_desc
    assert L.fd_txn_amd_parse_packed_dev(4, one, one, one, one, ctypes.c_void_p(4100), one, 64, one, z) == INVAL   # d_desc_off


def _fake_engine(batch_max, blob_max):
    """test_tags_cpu._fake_engine with the two capacities the transaction
    argument check reads filled in (the first fields of struct fd_ed25519_amd,
    fd_ed25519_engine.h: int device; ulong cap; ulong blob_cap): a call that
    passes its argument checks fails at hipSetDevice, GPU or not."""
    buf = ctypes.create_string_buffer(1 << 16)
    struct.pack_into("<iiQQ", buf, 0, 0x7ffffff0, 0, batch_max, blob_max)
    return buf


SENT8, SENT32, SENT64 = 0x55, 0x55555555, 0x5555555555555555


def _outputs(n, nsl, cap):
    return [np.full(n, SENT8, np.int8), np.full(n + 1, SENT32, np.uint32), np.full(nsl, SENT8, np.int8),
            np.full(n, SENT64, np.uint64), np.full(nsl, SENT64, np.uint64), np.full(n + 1, SENT64, np.uint64),
            np.full(cap + 16, SENT8, np.uint8)]


def _untouched(out):
    sent = {1: SENT8, 4: SENT32, 8: SENT64}
    for o in out:
        assert (o.view(np.uint8 if o.dtype == np.int8 else o.dtype) == sent[o.itemsize]).all()


def test_desc_argument_errors_need_no_device():
    """Both host calls: desc without desc_off, desc_off without desc, and a
    capacity one byte under the bound sum are FD_ED25519_AMD_ERR_INVAL with
    every output untouched.  The staged call with exactly the bound sum passes
    its checks and gets as far as the device (ERR_DEVICE on the fake engine):
    the bound sum, not one more, is what is asked for."""
    from firedancer_amd import ed25519
    L, P = ed25519.lib(), ed25519._ptr
    buf = _fake_engine(64, 1 << 16)
    e = ctypes.cast(buf, ctypes.c_void_p)
    fx = [f.payload for f in _txn.load_fixtures()]
    pays = fx + [b"\x01" * 40, fx[0][:-1]]
    blob, off, sz = _txn.pack(pays)
    n = len(pays)
    need = sum(_bound(len(p)) for p in pays)
    assert need > 0 and _bound(40) == 0
    nsl = ed25519.txn_slots(blob, off, sz)[1]

    def staged(o, doff=True, desc=True, cap=need):
        return L.fd_ed25519_amd_verify_txns_desc(e, n, P(blob), P(off), P(sz), int(blob.size), P(o[0]), P(o[1]), P(o[2]),
                                                 P(o[3]), P(o[4]), P(o[5]) if doff else None, P(o[6]) if desc else None, cap)

    ptr = np.array([blob.ctypes.data + int(o) for o in off], np.uint64)
    sz64 = sz.astype(np.uint64)

    def registered(o, doff=True, desc=True, cap=need):
        return L.fd_ed25519_amd_verify_txns_registered_desc(e, n, P(ptr), P(sz64), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]),
                                                            P(o[5]) if doff else None, P(o[6]) if desc else None, cap)

    for call in (staged, registered):
        for kw in (dict(doff=False), dict(desc=False), dict(cap=need - 1), dict(cap=0)):
            o = _outputs(n, nsl, need)
            assert call(o, **kw) == INVAL, (call.__name__, kw)
            _untouched(o)
    # a NULL engine and a NULL txn_err are refused as in the _tag calls, descriptors asked for or not
    o = _outputs(n, nsl, need)
    z = ctypes.c_void_p(0)
    assert L.fd_ed25519_amd_verify_txns_desc(z, n, P(blob), P(off), P(sz), int(blob.size), P(o[0]), P(o[1]), P(o[2]), P(o[3]),
                                             P(o[4]), P(o[5]), P(o[6]), need) == INVAL
    assert L.fd_ed25519_amd_verify_txns_registered_desc(e, n, P(ptr), P(sz64), z, P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]),
                                                        P(o[6]), need) == INVAL
    _untouched(o)
    # exactly the bound sum: accepted by the checks, so the fake engine fails at its first device call
    o = _outputs(n, nsl, need)
    assert staged(o) == DEVICE
    assert (o[6][need:] == SENT8).all()
    # both NULL is the _tag call
    o = _outputs(n, nsl, need)
    assert staged(o, doff=False, desc=False, cap=0) == DEVICE
    _untouched(o[5:])


def test_want_desc_python_forms_raise_without_a_device():
    from firedancer_amd import ed25519
    buf = _fake_engine(64, 1 << 16)
    eng = ed25519.Engine.__new__(ed25519.Engine)
    eng._h = ctypes.cast(buf, ctypes.c_void_p)
    blob, off, sz = _txn.pack([f.payload for f in _txn.load_fixtures()])
    try:
        with pytest.raises(ed25519.EngineError, match="rc=-11"):
            eng.verify_txns(blob, off, sz, want_desc=True)
        with pytest.raises(ed25519.EngineError, match="rc=-10"):   # unregistered memory
            eng.verify_txns_ptrs(np.uint64(blob.ctypes.data) + off.astype(np.uint64), sz.astype(np.uint64), want_desc=True)
    finally:
        eng._h = None                                        # nothing to delete
