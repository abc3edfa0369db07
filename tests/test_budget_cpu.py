"""CPU: the compute budget rule (include/fd_txn_amd.h, "Compute budget").  The
corpus of tests/_budget.py is deterministic and pinned; the committed expected
records (the reference's own functions, tests/golden/README_budget.md), the
Python restatement and the host rule fd_txn_amd_budget agree on all of it; the
record's layout is the header's; the engine calls refuse bad arguments before
they touch a device."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import _budget as B
import _oracle
from firedancer_amd import ed25519

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA256 = "cd96694169787fc6cc6417f82dcc23c09458d749eee2faecff28a7197ca8d6c2"


@pytest.fixture(scope="module")
def corpus():
    """[(name, payload, descriptor bytes)], cases() then big_cases()."""
    return [(n, p, _oracle.txn_parse(p)[1]) for n, p in B.cases() + B.big_cases()]


def _host(p, desc):
    return tuple(int(x) for x in ed25519.txn_budget(p, desc).tolist())


def test_corpus_is_deterministic_and_pinned():
    cs = B.cases() + B.big_cases()
    names = [n for n, _ in cs]
    assert len(set(names)) == len(names) == 88
    assert B.digest(cs) == SHA256
    B._cases = B._big = None                      # built again from nothing
    assert B.digest(B.cases() + B.big_cases()) == SHA256
    assert B.REC.size == ed25519.BUDGET_DTYPE.itemsize        # the records the corpus is for
    assert max(len(p) for _, p in B.cases()) == 1232 and [len(p) for _, p in B.big_cases()][-1] == 65535


def test_golden_restatement_and_host_rule_agree(corpus):
    gold = B.load_golden()
    assert len(gold) == len(corpus)
    for (name, p, desc), (gp, rec) in zip(corpus, gold):
        assert gp == p, name
        assert B.restate(p, desc) == rec, name
        assert _host(p, desc) == rec, name


def test_directed_values(corpus):
    rec = {n: _host(p, d) for n, p, d in corpus}
    for (cu, pr), want in B.FEE_EXPECT.items():
        assert rec["fee_%d_%d" % (cu, pr)] == (want, cu, 0, B.F_CU | B.F_FEE, 2, B.OK)
    for cu, pr in B.FEE_PAIRS:                    # the plain formula, in big integers
        assert rec["fee_%d_%d" % (cu, pr)][0] == min(B.U64, -((-cu * pr) // 10**6))
    assert rec["none_1"] == (0, 200000, 0, 0, 0, B.OK) and rec["none_3"] == (0, 600000, 0, 0, 0, B.OK)
    assert rec["kind_deprecated"] == (0x05060708, 0x01020304, 0, B.F_CU | B.F_FEE | B.F_TOTAL, 1, B.OK)
    assert rec["fee_default_limit"] == (2800001, 400000, 0, B.F_FEE, 1, B.OK)
    # every rejected transaction is all zeros beside the status: no partial state
    for n in ("invalid_after_valid", "invalid_heap_after_valid", "heap_000003ff", "heap_ffffffff", "dup_1111",
              "order_limit_after_deprecated", "order_price_after_deprecated", "size_d2_4", "disc_255_9", "mtu_355_all_to_id"):
        assert rec[n] == (0, 0, 0, 0, 0, B.INVALID), n
    assert [rec["dup_%d%d%d%d" % c][5] for c in B.DUPLICATES] == [B.OK, B.INVALID, B.OK] + [B.INVALID] * 5
    # an address that is not the id, and a program index in the lookup tables, are not budget instructions
    for n in ("addr_differs_0", "addr_differs_15", "addr_differs_31", "lut_blockhash_is_id"):
        assert rec[n] == (0, 200000, 0, 0, 0, B.OK), n
    assert rec["id_twice"] == (77, 77, 0, B.F_CU | B.F_FEE, 2, B.OK)
    for n in ("mtu_342_first", "mtu_342_middle", "mtu_342_last"):
        assert rec[n] == (0, 0x31323334, 0, B.F_CU, 1, B.OK)
    assert rec["mtu_355_none"] == (0, 355 * 200000, 0, 0, 0, B.OK)
    for n in ("noparse_truncated", "noparse_empty", "noparse_trailing"):
        assert rec[n] == (0, 0, 0, 0, 0, B.NOPARSE)
    assert rec["max_size"] == (4355, 59832704, 0, B.F_FEE, 1, B.OK)


def test_limit_above_32_bits_by_hand_made_descriptor():
    """21789 instructions, one of them a SetComputeUnitPrice of 1: the limit
    is 21788 * 200000 = 4357600000, compute its low half and the fee uses all
    of it.  No payload holds that many beside a budget instruction
    (_budget.py), so the descriptor is made by hand over a small payload."""
    p = B.build([B.other(), B.cb(B.price(1))])
    _, desc, _ = _oracle.txn_parse(p)
    ix_other, ix_price = desc[20:30], desc[30:40]
    d = bytearray(desc[:18]) + struct.pack("<H", 21789) + ix_other * 21000 + ix_price + ix_other * 788
    assert _host(p, bytes(d)) == (4358, 62632704, 0, B.F_FEE, 1, B.OK) == B.restate(p, bytes(d))


def test_null_descriptor_and_foreign_descriptor():
    p = B.build([B.cb(B.limit(5))])
    assert _host(p, None) == _host(p, b"") == (0, 0, 0, 0, 0, B.NOPARSE)
    out = np.full(1, 0xA5, np.uint8).repeat(24).view(ed25519.BUDGET_DTYPE)
    assert ed25519.lib().fd_txn_amd_budget(None, 0, None, ctypes.c_void_p(out.ctypes.data)) == B.NOPARSE
    assert tuple(int(x) for x in out[0].tolist()) == (0, 0, 0, 0, 0, B.NOPARSE)
    # a descriptor whose ranges end beyond the payload given: no read outside it
    _, desc, _ = _oracle.txn_parse(p)
    assert _host(p[:-1], desc) == (0, 0, 0, 0, 0, B.NOPARSE)
    assert _host(p[:100], desc) == (0, 0, 0, 0, 0, B.NOPARSE)


def test_record_layout(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text('''
#include <stddef.h>
#include "fd_txn_amd.h"
_Static_assert( sizeof(fd_txn_amd_budget_t)==24UL && _Alignof(fd_txn_amd_budget_t)==8UL, "size" );
_Static_assert( offsetof(fd_txn_amd_budget_t, rewards)==0UL && offsetof(fd_txn_amd_budget_t, compute)==8UL, "offsets" );
_Static_assert( offsetof(fd_txn_amd_budget_t, heap_sz)==12UL && offsetof(fd_txn_amd_budget_t, flags)==16UL, "offsets" );
_Static_assert( offsetof(fd_txn_amd_budget_t, cb_instr_cnt)==18UL && offsetof(fd_txn_amd_budget_t, status)==20UL, "offsets" );
_Static_assert( FD_TXN_AMD_BUDGET_OK==0 && FD_TXN_AMD_BUDGET_INVALID==1 && FD_TXN_AMD_BUDGET_NOPARSE==2, "status" );
_Static_assert( FD_TXN_AMD_BUDGET_FLAG_SET_CU==1 && FD_TXN_AMD_BUDGET_FLAG_SET_FEE==2 && FD_TXN_AMD_BUDGET_FLAG_SET_HEAP==4 &&
                FD_TXN_AMD_BUDGET_FLAG_SET_TOTAL_FEE==8, "flags" );
int main( void ) { fd_txn_amd_budget_t b; return fd_txn_amd_budget( NULL, 0UL, NULL, &b )!=(int)FD_TXN_AMD_BUDGET_NOPARSE || b.status!=2U; }
''')
    exe = tmp_path / "layout"
    libdir = os.path.dirname(ed25519.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c),
                           "-L", libdir, "-lfd_ed25519_amd", "-Wl,-rpath," + libdir, "-o", str(exe)])
    subprocess.run([str(exe)], check=True)
    dt = ed25519.BUDGET_DTYPE
    assert dt.itemsize == 24
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == [
        ("rewards", 0, 8), ("compute", 8, 4), ("heap_sz", 12, 4), ("flags", 16, 2), ("cb_instr_cnt", 18, 2), ("status", 20, 4)]
    assert tuple(int(x) for x in np.frombuffer(B.REC.pack(1, 2, 3, 4, 5, 6), dt)[0].tolist()) == (1, 2, 3, 4, 5, 6)


def test_engine_calls_refuse_bad_arguments_without_a_device():
    L = ed25519.lib()
    INVAL = ed25519.ERR_INVAL
    b = np.full(24, 0xA5, np.uint8)
    t = ctypes.c_ulong(7)
    z = None
    # no engine: refused first, in all four
    assert L.fd_ed25519_amd_verify_txns_budget(z, 1, z, z, z, 0, z, z, z, z, z, z, z, 0, _p(b)) == INVAL
    assert L.fd_ed25519_amd_verify_txns_registered_budget(z, 1, z, z, z, z, z, z, z, z, z, 0, _p(b)) == INVAL
    assert L.fd_ed25519_amd_submit_txns_budget(z, 1, z, z, z, 0, z, z, z, z, z, z, z, 0, z, z, z, 0, z, z, _p(b),
                                               ctypes.byref(t)) == INVAL
    assert L.fd_ed25519_amd_submit_txns_registered_budget(z, 1, z, z, z, z, z, z, z, z, z, 0, z, z, z, 0, z, z, _p(b),
                                                          ctypes.byref(t)) == INVAL
    # the device-resident step: NULL planes, a misaligned record plane; nothing to do is fine
    assert L.fd_txn_amd_budget_dev(1, z, z, z, z, z, z) == INVAL
    assert L.fd_txn_amd_budget_dev(1, 64, 64, 64, 64, 68, z) == INVAL
    assert L.fd_txn_amd_budget_dev(1 << 32, 64, 64, 64, 64, 64, z) == INVAL
    assert L.fd_txn_amd_budget_dev(0, z, z, z, z, z, z) == 0
    assert (b == 0xA5).all() and t.value == 7


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)
