"""Compute budget test helpers (include/fd_txn_amd.h, "Compute budget"): the
directed corpus, an independent Python restatement of the rule, and the loader
of the committed expected records.

The corpus is built here from _txn.mk / _txn.ins at test time; account
addresses are patched in afterwards (mk's are k+1 repeated).  Unless a case
says otherwise a payload is legacy with one signer and three accounts: the fee
payer, some program (index 1) and the compute budget program (index 2).

tests/golden/budget_vectors.bin holds every payload with the record that the
reference's own fd_compute_budget_program_{init,parse,finalize} give for it
(tools/gen_budget_golden.c; tests/golden/README_budget.md).  `python
tests/_budget.py dump FILE` writes the generator's input.

Three things the corpus cannot hold as the words "355 instructions at the MTU"
and "65535 bytes, 21789 instructions" would have them, because neither shape
leaves a byte to spare (167 + 3*355 = 1232 and 168 + 3*21789 = 65535, every
instruction empty) while a valid budget instruction needs five data bytes and
a third account for the other instructions' program:
  - at the MTU the budget instruction is first, in the middle and last of the
    342 instructions that do fit 1232 bytes; the 355-instruction payload is
    there without one, and with its only program being the id (every
    instruction then has data_sz 0: _INVALID at the first);
  - 355 instructions with a budget instruction first, in the middle and last
    (1273 bytes) are in the list the device-resident and host forms take
    (big_cases), next to
  - the 65535-byte payload, which has 21775 instructions, one of them a
    SetComputeUnitPrice of 1: compute 59832704 (the low half of 21774 *
    200000 = 4354800000) and rewards 4355.
test_budget_cpu.py checks the issue's own figures for 21789 instructions
(compute 62632704, rewards 4358) on the host rule through a descriptor made by
hand.
"""
import hashlib
import os
import struct
import sys

import numpy as np

import _txn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "budget_vectors.bin")
GOLD_MAGIC = b"FDBUDGETGOLDEN1\0"
IN_MAGIC = b"FDBUDGETINPUT01\0"

PROGRAM_ID = bytes.fromhex("0306466fe5211732ffecadba72c39be7bc8ce5bbc5f7126b2c439b3a40000000")
OK, INVALID, NOPARSE = 0, 1, 2
F_CU, F_FEE, F_HEAP, F_TOTAL = 1, 2, 4, 8
U64 = (1 << 64) - 1

# (rewards, compute, heap_sz, flags, cb_instr_cnt, status)
REC = struct.Struct("<QIIHHI")
assert REC.size == 24


# ---- instruction data ----

def deprecated(units, fee):
    return struct.pack("<BII", 0, units, fee)


def heap(sz):
    return struct.pack("<BI", 1, sz)


def limit(units):
    return struct.pack("<BI", 2, units)


def price(ulamports):
    return struct.pack("<BQ", 3, ulamports)


def cb(data, prog=2):
    return _txn.ins(prog, data=data)


def other(data=b"", prog=1):
    return _txn.ins(prog, data=data)


def acct_off(nsig, v0, nacct):
    return 1 + 64 * nsig + (1 if v0 else 0) + 3 + len(_txn.cu16(nacct))


def build(instrs, nacct=3, ids=(2,), v0=False, luts=None, blockhash=None, addr=None):
    """A one-signer payload whose accounts `ids` hold the program id (addr:
    {index: 32 bytes} overrides), blockhash as given."""
    p = bytearray(_txn.mk(1, v0, 0, 0, nacct, instrs, luts if v0 else None))
    a = acct_off(1, v0, nacct)
    for k in ids:
        p[a + 32 * k:a + 32 * k + 32] = PROGRAM_ID
    for k, v in (addr or {}).items():
        p[a + 32 * k:a + 32 * k + 32] = v
    if blockhash is not None:
        p[a + 32 * nacct:a + 32 * nacct + 32] = blockhash
    return bytes(p)


def _flip(k):
    b = bytearray(PROGRAM_ID)
    b[k] ^= 0x01
    return bytes(b)


# The reference's test_duplicate counts (deprecated, heap, limit, price), issued in that order
DUPLICATES = ((1, 1, 0, 0), (2, 0, 0, 0), (0, 1, 1, 1), (1, 1, 1, 1), (0, 0, 2, 1), (0, 0, 1, 2), (1, 0, 1, 0), (1, 0, 0, 1))

# (cu, micro-lamports per cu): the last is the wrap of the split form's final
# addition with cu <= 2^32 - 1 that a search finds at once: ch = 1 and ph =
# floor( (2^64 - 1) / 10^12 ) put hh at its largest, 18446744073709000000,
# and cl * ph = 18446744073709 carries it past 2^64
FEE_PAIRS = ((10**6, 10**6), (10**6, (1 << 63) - 1), (2 * 10**6, U64), (9 * 10**6, 1 << 40), (1, 1), (0, U64),
             ((1 << 32) - 1, U64), (4 * 10**9, 4611686018 * 10**6), (4 * 10**9, 4611686019 * 10**6),
             (1000001, 18446744073709 * 10**6))
FEE_EXPECT = {(9 * 10**6, 1 << 40): 9895604649984, (1, 1): 1, (0, U64): 0,
              (4 * 10**9, 4611686018 * 10**6): 18446744072000000000, (4 * 10**9, 4611686019 * 10**6): U64,
              (1000001, 18446744073709 * 10**6): U64}

_cases = None
_big = None


def cases():
    """[(name, payload)]: the corpus, every payload at most 1232 bytes."""
    global _cases
    if _cases is not None:
        return _cases
    out = []

    def add(name, payload):
        assert len(payload) <= 1232, (name, len(payload))
        out.append((name, payload))

    # no budget instruction (the data looks like one; the program is not the id)
    add("none_1", build([other(limit(7))]))
    add("none_3", build([other(), other(price(5)), other(heap(1024))]))
    # each kind alone
    add("kind_deprecated", build([cb(deprecated(0x01020304, 0x05060708))]))
    add("kind_heap", build([cb(heap(64 * 1024))]))
    add("kind_limit", build([cb(limit(1400000))]))
    add("kind_price", build([cb(price(0x0102030405060708))]))
    # sizes and discriminants
    for d in (0, 1, 2, 3):
        for n in (0, 4, 5, 6, 9, 10):
            add("size_d%d_%d" % (d, n), build([cb((bytes([d]) + bytes(16))[:n])]))
    for d in (4, 255):
        for n in (5, 9):
            add("disc_%d_%d" % (d, n), build([cb(bytes([d]) + bytes(n - 1))]))
    # duplicates
    kinds = (deprecated(0x0a0b0c0d, 0x01020304), heap(0x00010000), limit(0x0a0b0c0d), price(0x0102030405060708))
    for cnt in DUPLICATES:
        add("dup_%d%d%d%d" % cnt, build([cb(kinds[k]) for k in range(4) for _ in range(cnt[k])]))
    add("order_limit_after_deprecated", build([cb(deprecated(1, 2)), cb(limit(3))]))
    add("order_deprecated_after_limit", build([cb(limit(3)), cb(deprecated(1, 2))]))
    add("order_price_after_deprecated", build([cb(deprecated(1, 2)), cb(price(3))]))
    add("order_deprecated_after_price", build([cb(price(3)), cb(deprecated(1, 2))]))
    # an invalid budget instruction after a valid one: nothing of the valid one may show
    add("invalid_after_valid", build([cb(limit(1000)), cb(heap(32 * 1024)), cb(price(9)), cb(bytes([2, 0, 0, 0]))]))
    add("invalid_heap_after_valid", build([cb(limit(1000)), cb(heap(1023))]))
    # heap values
    for v in (0, 1024, 1023, 1025, 0xFFFFFC00, 0xFFFFFFFF):
        add("heap_%08x" % v, build([cb(heap(v))]))
    # fees
    for cu, p in FEE_PAIRS:
        add("fee_%d_%d" % (cu, p), build([cb(limit(cu)), cb(price(p))]))
    add("fee_default_limit", build([other(), other(b"\x01\x02"), cb(price(7 * 10**6 + 1))]))
    add("fee_default_limit_sat", build([other(), cb(price(U64))]))
    # the budget instruction's data at each byte alignment (within the payload)
    for k in range(4):
        add("align_%d" % k, build([other(bytes(k)), cb(price(0x1112131415161718)), cb(limit(0x21222324))]))
    # program addresses
    for k in (0, 15, 31):
        add("addr_differs_%d" % k, build([cb(limit(5))], addr={2: _flip(k)}))
    add("id_twice", build([cb(limit(77), prog=2), cb(price(10**6), prog=3), other()], nacct=4, ids=(2, 3)))
    add("lut_blockhash_is_id", build([_txn.ins(2, data=limit(5))], nacct=2, ids=(), v0=True, luts=[_txn.lut(1, 0)],
                                     blockhash=PROGRAM_ID))
    add("v0_budget", build([cb(limit(300000)), _txn.ins(3, data=price(2))], nacct=3, v0=True, luts=[_txn.lut(1, 1)]))
    # at the MTU (module docstring): 342 instructions in 1232 bytes, and the 355-instruction payloads
    fill = [_txn.EMPTY_IX] * 340 + [other(b"\0\0")]
    for name, at in (("first", 0), ("middle", 170), ("last", 341)):
        p = build(fill[:at] + [cb(limit(0x31323334))] + fill[at:])
        assert len(p) == 1232
        add("mtu_342_" + name, p)
    add("mtu_355_none", _txn.mk(1, False, 0, 0, 2, [_txn.EMPTY_IX] * 355))
    add("mtu_355_all_to_id", build([_txn.EMPTY_IX] * 355, nacct=2, ids=(1,)))
    # payloads that do not parse
    add("noparse_truncated", build([cb(limit(5))])[:-1])
    add("noparse_empty", b"")
    add("noparse_trailing", build([cb(limit(5))]) + b"\0")
    _cases = out
    return out


def big_cases():
    """[(name, payload)] for the device-resident and host forms only:
    payloads above the MTU."""
    global _big
    if _big is not None:
        return _big
    out = []
    fill = [_txn.EMPTY_IX] * 354
    for name, at in (("first", 0), ("middle", 177), ("last", 354)):
        out.append(("instr_355_" + name, build(fill[:at] + [cb(price(3 * 10**6))] + fill[at:])))
    big = build([_txn.EMPTY_IX] * 21000 + [cb(price(1))] + [_txn.EMPTY_IX] * 773 + [other(b"\0")])
    assert len(big) == 65535
    out.append(("max_size", big))
    _big = out
    return out


def digest(cs):
    h = hashlib.sha256()
    for name, p in cs:
        h.update(struct.pack("<II", len(name), len(p)) + name.encode() + p)
    return h.hexdigest()


# ---- the rule, restated ----

def restate(payload, desc):
    """The record of one payload with descriptor bytes `desc` (empty: it did
    not parse), as a REC tuple: plain Python, big integers, the fee as
    min( 2^64 - 1, ceil( cu * price / 10^6 ) )."""
    if not desc:
        return (0, 0, 0, 0, 0, NOPARSE)
    nacct, aoff = struct.unpack_from("<HH", desc, 8)
    ninstr = struct.unpack_from("<H", desc, 18)[0]
    seen, cnt, cu, total, hp, micro = set(), 0, 0, 0, 0, 0
    for i in range(ninstr):
        prog, _, _, dsz, _, doff = struct.unpack_from("<BBHHHH", desc, 20 + 10 * i)
        if prog >= nacct or payload[aoff + 32 * prog:aoff + 32 * prog + 32] != PROGRAM_ID:
            continue
        data = payload[doff:doff + dsz]
        if len(data) < 5:
            return (0, 0, 0, 0, 0, INVALID)
        kind = data[0]
        want = {0: (9, {"cu", "fee"}), 1: (5, {"heap"}), 2: (5, {"cu"}), 3: (9, {"fee"})}.get(kind)
        if want is None or len(data) != want[0] or (seen & want[1]):
            return (0, 0, 0, 0, 0, INVALID)
        if kind == 0:
            cu, total = struct.unpack_from("<II", data, 1)
            seen |= {"cu", "fee", "total"}
        elif kind == 1:
            hp = struct.unpack_from("<I", data, 1)[0]
            if hp % 1024:
                return (0, 0, 0, 0, 0, INVALID)
            seen.add("heap")
        elif kind == 2:
            cu = struct.unpack_from("<I", data, 1)[0]
            seen.add("cu")
        else:
            micro = struct.unpack_from("<Q", data, 1)[0]
            seen.add("fee")
        cnt += 1
    lim = cu if "cu" in seen else (ninstr - cnt) * 200000
    rewards = total if "total" in seen else min(U64, -((-lim * micro) // 10**6))
    flags = sum(v for k, v in (("cu", F_CU), ("fee", F_FEE), ("heap", F_HEAP), ("total", F_TOTAL)) if k in seen)
    return (rewards, lim & 0xFFFFFFFF, hp, flags, cnt, OK)


# ---- the committed expected records ----

def load_golden():
    """[(payload, REC tuple)] in corpus order: cases() then big_cases()."""
    raw = open(GOLD, "rb").read()
    assert raw[:16] == GOLD_MAGIC
    n = struct.unpack_from("<I", raw, 16)[0]
    at, out = 24, []
    for _ in range(n):
        sz = struct.unpack_from("<I", raw, at)[0]
        at += 4
        p = raw[at:at + sz]
        at += sz
        out.append((p, REC.unpack_from(raw, at)))
        at += 24
    assert at == len(raw)
    return out


def dump_input(path):
    """The generator's input: every payload with the descriptor the oracle's
    fd_txn_parse writes for it (footprint 0: none)."""
    import _oracle
    cs = cases() + big_cases()
    with open(path, "wb") as f:
        f.write(IN_MAGIC + struct.pack("<II", len(cs), 0))
        for _, p in cs:
            fp, desc, _ = _oracle.txn_parse(p)
            f.write(struct.pack("<II", len(p), fp) + p + desc)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump_input(sys.argv[2])
    else:
        sys.exit("usage: python tests/_budget.py dump FILE")
