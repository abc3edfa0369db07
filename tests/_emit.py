"""A byte-level model of the output frames (include/fd_ed25519_amd.h, "Output
frames"), written from the rule's text alone: both frame types, the
placement, the bytes a call may write, and the bounds.  The host functions
(test_emit_cpu.py) and the GPU (test_emit_gpu.py) are compared with it byte
for byte.

Descriptors are inputs here: from liboracle's fd_txn_parse on the CPU
(oracle_desc) and from the _desc calls on the GPU.
"""
import struct

import numpy as np

import _txn

MSG_SIZES = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 1232)
FILL = 0xA5


def ru(x, a):
    return (x + a - 1) // a * a


def sig_frame(pub, sig, msg):
    assert len(pub) == 32 and len(sig) == 64
    return bytes(pub) + bytes(sig) + bytes(msg)


def txn_frame(payload, desc):
    p = len(payload)
    assert p <= 0xFFFF and len(desc) % 2 == 0
    f = bytes(payload) + b"\0" * (ru(p, 16) - p) + bytes(desc) + struct.pack("<H", p)
    assert len(f) == ru(p, 16) + len(desc) + 2
    return f


def place(frames):
    """(emit_off, emit_sz) of a list of frames (b"": a frame of size 0)."""
    off = np.zeros(len(frames) + 1, np.uint64)
    for j, f in enumerate(frames):
        off[j + 1] = int(off[j]) + ru(len(f), 128)
    return off, np.array([len(f) for f in frames], np.uint32)


def lay(frames, image, cap=None):
    """Write the frames over `image` (a uint8 array, changed in place) as a
    call with capacity cap does: frame j only if emit_off[j+1] <= cap, as the
    frame and zeros up to the next multiple of 16; no other byte."""
    off, sz = place(frames)
    cap = image.size if cap is None else cap
    for j, f in enumerate(frames):
        if not f or int(off[j + 1]) > cap:
            continue
        o = int(off[j])
        image[o:o + len(f)] = np.frombuffer(f, np.uint8)
        image[o + len(f):o + ru(len(f), 16)] = 0
    return off, sz


def desc_bound(payload_sz):
    """fd_txn_amd_desc_bound, restated from its derivation."""
    if payload_sz < 134 or payload_sz > 65535:
        return 0
    b = 20 + 10 * ((payload_sz - 134) // 3)
    return min(b, 3570) if payload_sz <= 1232 else b


def sig_bound(msg_sz):
    return ru(96 + msg_sz, 128)


def txn_bound(payload_sz):
    d = desc_bound(payload_sz)
    return ru(ru(payload_sz, 16) + d + 2, 128) if d else 0


def keep_lists(n):
    """name -> keep: empty, all, sparse (every third), last item only."""
    return {"empty": [], "all": list(range(n)), "sparse": list(range(0, n, 3)), "last": [n - 1]}


def sig_items(seed=11, sizes=MSG_SIZES):
    """One (pub, sig, msg) of random bytes per message size."""
    rng = np.random.default_rng(seed)
    r = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    return [(r(32), r(64), r(z)) for z in sizes]


def txn_payloads():
    """name -> payload: the three fixture payloads, the smallest payload
    that parses (134 B), a v0 payload with lookup tables, a multi-signer one,
    and the MTU payload with 355 empty instructions (the largest descriptor an
    MTU payload has: 3570 B)."""
    out = {"fixture%d" % k: bytes(f.payload) for k, f in enumerate(_txn.load_fixtures())}
    assert len(out) == 3
    out["min_134"] = _txn.mk(1, False, 0, 0, 1, [])
    out["v0_luts"] = _txn.mk(1, True, 0, 0, 2, [_txn.ins(5, accts=b"\x05", data=b"\x01\x02\x03")], [_txn.lut(2, 2), _txn.lut(0, 1)])
    out["multi_signer"] = _txn.mk(3, False, 1, 0, 5, [_txn.ins(4, accts=b"\x00\x01\x02", data=bytes(range(40)))])
    out["mtu_355"] = _txn.mk(1, False, 0, 0, 2, [_txn.EMPTY_IX] * 355)
    assert len(out["min_134"]) == 134 and len(out["mtu_355"]) == 1232
    return out


def oracle_desc(payload):
    """The fd_txn_t bytes liboracle's fd_txn_parse writes (b"" when it rejects)."""
    import _oracle
    fp, d, _ = _oracle.txn_parse(payload)
    return bytes(d[:fp])


def pack_desc(descs):
    """(desc_off, desc) as the _desc calls return them."""
    off = np.zeros(len(descs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in descs], dtype=np.uint64)
    return off, np.frombuffer(b"".join(descs) + b"\0\0", np.uint8)[:int(off[-1])].copy()
