"""Independent RFC 8032 signer -- TEST CHECKER ONLY.

Python big integers and hashlib.sha512, over the curve arithmetic of
tests/_strict_ref.py (extended coordinates, double-and-add).  It shares
nothing with the host signer (fd_ed25519_host.cpp), the GPU signer
(fd_ed25519_sign.h), the generated constants or the CPU oracle, so a byte
that differs from it says which side is wrong.  Signing is deterministic:
the model gives the exact expected bytes of any (seed, message).

Also here: the directed corpus of (seed, message) items that the CPU tests
of the host signer (tests/test_sign_ref_cpu.py) and the GPU tests of k_sign
(tests/test_sign_gpu.py) share.
"""
import functools
import hashlib
import random

import numpy as np

from _strict_ref import B, L, P, add, mul  # noqa: F401  (add: part of the model's surface)


def encode(point):
    """32 bytes: y little-endian, the parity of x in bit 255 (RFC 8032 s5.1.2)."""
    X, Y, Z = point[0], point[1], point[2]
    zi = pow(Z, P - 2, P)
    x, y = X * zi % P, Y * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def scalarmult_base_enc(s):
    """encode([s]B) for any integer s >= 0."""
    return encode(mul(s, B))


def _expand(seed):
    h = hashlib.sha512(bytes(seed)).digest()
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a, h[32:]


def public_from_private(seed):
    """RFC 8032 s5.1.5."""
    return scalarmult_base_enc(_expand(seed)[0])


def sc_muladd(k, a, r):
    return (r + k * a) % L


def sign(seed, msg):
    """RFC 8032 s5.1.5 / s5.1.6: (public key, R || S)."""
    msg = bytes(msg)
    a, prefix = _expand(seed)
    pub = scalarmult_base_enc(a)
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    R = scalarmult_base_enc(r)
    k = int.from_bytes(hashlib.sha512(R + pub + msg).digest(), "little") % L
    return pub, R + sc_muladd(k, a, r).to_bytes(32, "little")


# ---- the directed corpus ---------------------------------------------------------

RFC_SECRETS = ["9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
               "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
               "c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7"]

PREFIXES = (32, 64)                            # sha512_pm<4> (r) and sha512_pm<8> (k)
EDGE_RESIDUES = (0, 111, 112, 119, 120, 127)   # (prefix + sz) % 128: block-count edges, 0x80 on a word's / block's last byte


def corpus_sizes():
    """Every sz < 256 at a padding edge of either prefixed hash, the small
    sizes around one word, and the largest message a transaction carries."""
    edge = {sz for sz in range(256) for p in PREFIXES if (p + sz) % 128 in EDGE_RESIDUES}
    return sorted(edge | set(range(0, 10)) | {1232})


class Corpus:
    """prv (n, 32), blob, off (n,), sz (n,) in the signers' input layout, and
    the model's pub (n, 32), sig (n, 64)."""

    def __init__(self, prv, blob, off, sz, pub, sig):
        self.prv, self.blob, self.off, self.sz, self.pub, self.sig = prv, blob, off, sz, pub, sig

    def __len__(self):
        return int(self.prv.shape[0])

    def msg(self, i):
        o = int(self.off[i])
        return bytes(self.blob[o:o + int(self.sz[i])])


def build_inputs():
    """(prv, blob, off, sz) of the corpus.  Messages are random bytes packed
    back to back with 0..7 filler bytes between them (a per-gap constant, so
    a read that strays into a gap changes the hash); the gap puts each
    message at a chosen residue of its start offset: every size at every
    msg_off % 4, sizes 1..9 at every msg_off % 8."""
    rng = random.Random(8032)
    plan = []
    for sz in corpus_sizes():
        for res in (range(8) if 1 <= sz <= 9 else (0, 5, 2, 7)):
            plan.append((sz, res))
    rng.shuffle(plan)
    seeds = [bytes(32), b"\xff" * 32] + [bytes.fromhex(s) for s in RFC_SECRETS]
    twice = bytes(rng.getrandbits(8) for _ in range(32))
    seeds += [twice, twice]                                   # one seed on two different messages
    seeds += [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(len(plan) - len(seeds))]
    blob, off = bytearray(), []
    for k, (sz, res) in enumerate(plan):
        blob += bytes([0xa5 ^ (k & 0x3f)]) * ((res - len(blob)) % 8)
        off.append(len(blob))
        blob += bytes(rng.getrandbits(8) for _ in range(sz))
    blob += b"\x5a" * 8
    n = len(plan)
    assert n <= 400 and n % 64 != 0
    return (np.frombuffer(b"".join(seeds), np.uint8).reshape(n, 32).copy(), np.frombuffer(bytes(blob), np.uint8).copy(),
            np.array(off, np.uint32), np.array([sz for sz, _ in plan], np.uint32))


@functools.lru_cache(maxsize=None)
def corpus():
    """The corpus with the model's expected bytes; computed once per process."""
    prv, blob, off, sz = build_inputs()
    n = prv.shape[0]
    pub, sig = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    for i in range(n):
        p, s = sign(bytes(prv[i]), bytes(blob[int(off[i]):int(off[i]) + int(sz[i])]))
        pub[i], sig[i] = np.frombuffer(p, np.uint8), np.frombuffer(s, np.uint8)
    for a in (prv, blob, off, sz, pub, sig):
        a.setflags(write=False)
    return Corpus(prv, blob, off, sz, pub, sig)


def first_difference(c, pub, sig, n=None):
    """None when pub / sig rows [0, n) equal the model's; else a message that
    names the first differing part of the first differing item: pub isolates
    the seed hash, the clamp and [a]B; R the prefixed hash and [r]B; S the
    third hash and the multiply-add."""
    n = len(c) if n is None else n
    pub, sig = np.asarray(pub)[:n], np.asarray(sig)[:n]
    bad = np.nonzero((pub != c.pub[:n]).any(1) | (sig != c.sig[:n]).any(1))[0]
    if not bad.size:
        return None
    i = int(bad[0])
    parts = (("pub", pub[i], c.pub[i]), ("R", sig[i, :32], c.sig[i, :32]), ("S", sig[i, 32:], c.sig[i, 32:]))
    what, got, want = next(p for p in parts if (p[1] != p[2]).any())
    return ("%d of %d items differ from the model; first item %d (msg_sz %d, msg_off %d = %d mod 8): %s differs first, "
            "got %s want %s" % (bad.size, n, i, int(c.sz[i]), int(c.off[i]), int(c.off[i]) % 8, what,
                                bytes(got).hex(), bytes(want).hex()))
