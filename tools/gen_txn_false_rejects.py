#!/usr/bin/env python3
"""Search for wire transactions in which one VALID signature is a limb-compare
false reject of the reference (its verdict -3, the strict verdict 0; about
1.6e-6 of valid signatures) and write them, as data, to
tests/golden/txn_false_rejects.bin.  CPU only: the product's host signer and
the CPU oracle (the reference's verdicts), checked with tests/_strict_ref.py.

    python tools/gen_txn_false_rejects.py [out]

One transaction per (signers, position) in CASES.  A candidate is a legacy
message over fixed seeded signer keys whose last 8 instruction-data bytes
count up; only the signer at `position` signs during the search, the others
sign the message that was found.  Deterministic (seeded keys, ascending
counter), so a rerun writes the same bytes.

File: "FDTXNFREJ001\\0\\0\\0\\0", u32 count, then per transaction u32 signers,
u32 position, u32 size, the payload, zero-padded to 4 bytes.
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((1, 0), (2, 1), (12, 6))   # (signers, position of the false reject): first, last, middle
BATCH = 1 << 18


def search(nsig, pos, seed):
    import _golden
    import _oracle
    import _strict_ref
    import _txn
    from firedancer_amd import ed25519
    rng = np.random.default_rng(seed)
    prv = rng.integers(0, 256, (nsig, 32), dtype=np.uint8)
    z = np.zeros(nsig, np.uint32)
    pub, _ = ed25519.sign_batch(prv, np.zeros(1, np.uint8), z, z)
    base = _txn.message(rng, pub, 0, False, 1 if nsig < 10 else 0)     # 12 signers + 8 data bytes fit the 1232-B MTU
    base = base[:-1] + _txn.cu16(8) + bytes(8)          # the instruction's data: 8 counter bytes, last in the message
    ml = len(base)
    assert 1 + 64 * nsig + ml <= 1232
    ctr = 0
    while True:
        blob = np.tile(np.frombuffer(base, np.uint8), (BATCH, 1))
        blob[:, ml - 8:] = (np.arange(ctr, ctr + BATCH, dtype="<u8")).view(np.uint8).reshape(BATCH, 8)
        flat = np.concatenate([blob.reshape(-1), np.zeros(4, np.uint8)])
        off = (np.arange(BATCH, dtype=np.uint64) * ml).astype(np.uint32)
        sz = np.full(BATCH, ml, np.uint32)
        p1, s1 = ed25519.sign_batch(np.repeat(prv[pos:pos + 1], BATCH, 0), flat, off, sz)
        err = _oracle.verify_batch(_golden.Batch(p1, s1, off, sz, flat))
        hit = np.nonzero(err == -3)[0]
        print("signers %d position %d: counters [%d, %d) -> %d false rejects" % (nsig, pos, ctr, ctr + BATCH, hit.size),
              flush=True)
        if hit.size:
            k = int(hit[0])
            msg = bytes(blob[k])
            m = np.frombuffer(msg + b"\0\0\0\0", np.uint8)
            _, sig = ed25519.sign_batch(prv, m, z, np.full(nsig, ml, np.uint32))
            assert bytes(sig[pos]) == bytes(s1[k])
            for i in range(nsig):
                assert _strict_ref.verify(msg, sig[i], pub[i]) == 0
                assert _oracle.verify(msg, sig[i], pub[i]) == (-3 if i == pos else 0), i
            return bytes([nsig]) + sig.tobytes() + msg
        ctr += BATCH


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "txn_false_rejects.bin")
    recs = []
    for nsig, pos in CASES:
        p = search(nsig, pos, 0xF0E1 + 97 * nsig + pos)
        recs.append(struct.pack("<III", nsig, pos, len(p)) + p + bytes(-len(p) % 4))
    with open(out, "wb") as f:
        f.write(b"FDTXNFREJ001\0\0\0\0" + struct.pack("<I", len(recs)) + b"".join(recs))
    print("wrote", out)


if __name__ == "__main__":
    main()
