"""Directed edge corpus of points and scalars -- TEST INPUT GENERATOR ONLY.

Deterministic: big integers from tests/_strict_ref.py and hashlib, fixed
labels, no randomness (only the filler bytes of the transactions' messages
come from a seeded generator, which _txn.message takes).  It builds
signatures whose A, R or s sit on the edges the verdict code has to get right
(non-canonical y, mixed-order points, an R' that is half right, a neutral
accumulator, near misses of strict mode's byte compares, s around L and the
reference's accept window, s = L over a bad A or R, torsion pairs).  It
stores no expected verdicts: those come from the checkers (the oracle, the
compiled reference, _strict_ref) in the tests that use the corpus.

A vector's name is "<class>/<what>"; corpus() returns (names, _golden.Batch)
with Batch.cls the index into CLASSES.
"""
import hashlib
import math

import numpy as np

import _golden
import _strict_ref as S

P, L = S.P, S.L

CLASSES = [
    "valid", "r_negx", "r_negy", "a_negx", "mix_a", "mix_r", "mix_ra", "nc_a", "nc_r", "near_a", "near_r",
    "on_table", "s_plus_kL", "s_abs", "s_eq_L", "tor_pair",
]


# ---- points --------------------------------------------------------------------------

def affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def encode(p):
    x, y = affine(p)
    return (y | (x & 1) << 255).to_bytes(32, "little")


def from_affine(x, y):
    return (x % P, y % P, 1, x * y % P)


def neg(p):
    return (-p[0] % P, p[1], p[2], -p[3] % P)


def same_point(p, q):
    return affine(p) == affine(q)


_tors = None


def torsion():
    """The 8 torsion points [k]T, k = 0..7, T of order 8 -- found as
    tests/test_strict_api_cpu.py finds it: [L]Q kills the prime-order part
    of the first curve points Q (y = 2, 3, ...), and the first leftover of
    order exactly 8 is T."""
    global _tors
    if _tors is None:
        T, y = None, 2
        while T is None:
            Q = S.decode(y.to_bytes(32, "little"))
            y += 1
            if Q is None:
                continue
            t = S.mul(L, Q)
            if S.is_identity(S.mul(8, t)) and not S.is_identity(S.mul(4, t)):
                T = t
        _tors = [from_affine(*affine(S.mul(k, T))) for k in range(8)]
        assert len({affine(t) for t in _tors}) == 8 and affine(_tors[0]) == (0, 1)
    return _tors


def torsion_order(k):
    """Order of [k]T."""
    return 8 // math.gcd(k % 8, 8)


def y8():
    """The smaller y of the four points of order 8."""
    return min(affine(t)[1] for k, t in enumerate(torsion()) if k & 1)


def torsion_index(p):
    """k with p = [k]T, or None when p is not a torsion point."""
    for k, t in enumerate(torsion()):
        if same_point(p, t):
            return k
    return None


def torsion_part(p):
    """The torsion component of a curve point of order dividing 8 L: with
    p = Q + [k]T and Q of prime order, [L]p = [L mod 8][k]T, and L mod 8 = 5
    is its own inverse mod 8."""
    return torsion_index(S.mul(5, S.mul(L, p)))


# ---- scalars, hashing, signing ----------------------------------------------------------

def _h512(label):
    return hashlib.sha512(label).digest()


def _clamp(b):
    a = int.from_bytes(b[:32], "little")
    return (a & ((1 << 254) - 8)) | 1 << 254


KEY_A = _clamp(_h512(b"edge corpus: secret scalar"))
NONCE_R = int.from_bytes(_h512(b"edge corpus: nonce"), "little") % L
MSG = b"edge corpus: baseline message"


def hram(r_enc, a_enc, msg):
    return int.from_bytes(hashlib.sha512(bytes(r_enc) + bytes(a_enc) + bytes(msg)).digest(), "little") % L


def sign_chosen(a, a_enc, r, r_enc, msg):
    """Sign with chosen scalars: R || (r + H(R || A || M) a mod L) over the
    ENCODINGS given, which need not be those of [a]B and [r]B."""
    s = (r + hram(r_enc, a_enc, msg) * a) % L
    return bytes(r_enc) + s.to_bytes(32, "little")


def rprime(msg, sig, pub):
    """R' = [s]B - [h]A with big integers (A as _strict_ref decodes it)."""
    A = S.decode(pub)
    h = hram(sig[:32], pub, msg)
    return S.add(S.mul(int.from_bytes(sig[32:], "little"), S.B), S.mul(h, neg(A)))


def _grind(label, ok):
    """The first message label || counter that ok(msg) accepts."""
    for c in range(4096):
        msg = label + b" #%d" % c
        if ok(msg):
            return msg
    raise AssertionError("no message found for %r" % label)


def _yenc(y, sign):
    return (y | sign << 255).to_bytes(32, "little")


def near_ys():
    """Canonical y values one unit or one bit away from the constants strict
    mode compares bytes against (0, 1, p-1, y8, p-y8)."""
    y = y8()
    return [2, 3, P - 2, P - 3, y - 1, y + 1, (P - y) - 1, (P - y) + 1, 1 << 32, (1 << 32) + 1, 1 << 224,
            y ^ 1 << 31, y ^ 1 << 224, (P - 1) ^ 1 << 128]


def s_abs_values(s0):
    return [0, 1, L - 1, L, L + 1, (1 << 252) - 1, 1 << 252, (1 << 252) + (1 << 128) - 1, (1 << 252) + (1 << 128),
            (1 << 253) - 1, 1 << 253, 1 << 255, (1 << 256) - 1, s0 ^ 1, s0 ^ 1 << 251]


# ---- the corpus ---------------------------------------------------------------------------

def _build():
    out = []                                         # (name, pub, sig, msg)
    tors = torsion()
    Apt, Rpt = S.mul(KEY_A, S.B), S.mul(NONCE_R, S.B)
    Aenc, Renc = encode(Apt), encode(Rpt)
    base = sign_chosen(KEY_A, Aenc, NONCE_R, Renc, MSG)
    s0 = int.from_bytes(base[32:], "little")
    out.append(("valid/baseline", Aenc, base, MSG))

    # a half-right R': s is honest for the hash of the emitted bytes
    rx, ry = affine(Rpt)
    e = encode(neg(Rpt))
    out.append(("r_negx/-R", Aenc, sign_chosen(KEY_A, Aenc, NONCE_R, e, MSG), MSG))
    e = encode(from_affine(rx, -ry))
    out.append(("r_negy/(x,-y)", Aenc, sign_chosen(KEY_A, Aenc, NONCE_R, e, MSG), MSG))
    e = encode(neg(Apt))
    out.append(("a_negx/-A", e, sign_chosen(KEY_A, e, NONCE_R, Renc, MSG), MSG))

    # mixed-order points
    for k in range(1, 8):
        e = encode(S.add(Apt, tors[k]))
        o = torsion_order(k)
        for what, want in (("accept", True), ("reject", False)):
            msg = _grind(b"edge corpus: mix_a %d %s" % (k, what.encode()), lambda m: (hram(Renc, e, m) % o == 0) == want)
            out.append(("mix_a/T%d/%s" % (k, what), e, sign_chosen(KEY_A, e, NONCE_R, Renc, msg), msg))
    for k in range(1, 8):
        e = encode(S.add(Rpt, tors[k]))
        out.append(("mix_r/T%d" % k, Aenc, sign_chosen(KEY_A, Aenc, NONCE_R, e, MSG), MSG))
    for k in range(1, 8):
        o = torsion_order(k)
        m_ = (2 * k + 1) % o if o > 2 else 1         # T_R = -[m]T_A, m odd so that T_R is not the identity
        ea, er = encode(S.add(Apt, tors[k])), encode(S.add(Rpt, tors[(-m_ * k) % 8]))
        msg = _grind(b"edge corpus: mix_ra %d" % k, lambda m: hram(er, ea, m) % o == m_ and hram(er, ea, m) % 8 != 0)
        out.append(("mix_ra/T%d" % k, ea, sign_chosen(KEY_A, ea, NONCE_R, er, msg), msg))

    # non-canonical y = p + k, and the near misses of strict mode's byte compares
    for k in range(19):
        for sign in (0, 1):
            e = _yenc(P + k, sign)
            out.append(("nc_a/p+%d/%d" % (k, sign), e, base, MSG))
            out.append(("nc_r/p+%d/%d" % (k, sign), Aenc, e + base[32:], MSG))
    for j, y in enumerate(near_ys()):
        for sign in (0, 1):
            e = _yenc(y, sign)
            out.append(("near_a/%d/%d" % (j, sign), e, base, MSG))
            out.append(("near_r/%d/%d" % (j, sign), Aenc, e + base[32:], MSG))

    # A on the base point's own table, R' walking over the neutral element
    ident = encode(S.IDENT)
    for label, a in (("B", 1), ("-B", L - 1), ("2B", 2)):
        e = encode(S.mul(a, S.B))
        msg = b"edge corpus: on_table " + label.encode()
        out.append(("on_table/%s/honest" % label, e, sign_chosen(a, e, NONCE_R, Renc, msg), msg))
        out.append(("on_table/%s/R=identity" % label, e, sign_chosen(a, e, 0, ident, msg), msg))
        out.append(("on_table/%s/R=B" % label, e, sign_chosen(a, e, 1, encode(S.B), msg), msg))
        out.append(("on_table/%s/R=A" % label, e, sign_chosen(a, e, a, e, msg), msg))

    # s around L, 2^252 and the reference's accept window
    k = 1
    while s0 + k * L < 1 << 256:
        out.append(("s_plus_kL/%d" % k, Aenc, Renc + (s0 + k * L).to_bytes(32, "little"), MSG))
        k += 1
    for j, s in enumerate(s_abs_values(s0)):
        out.append(("s_abs/%d" % j, Aenc, Renc + s.to_bytes(32, "little"), MSG))

    # the rule's order at s = L exactly: step 1 answers before step 2 looks at the bytes of A and R
    for label, pub, r in (("A=identity", ident, Renc), ("A=p+3", _yenc(P + 3, 0), Renc),
                          ("R=T1", Aenc, encode(tors[1])), ("R=p+3", Aenc, _yenc(P + 3, 1))):
        out.append(("s_eq_L/%s" % label, pub, r + L.to_bytes(32, "little"), MSG))

    # every (torsion A, torsion R) pair, s = 0
    for i in range(8):
        for j in range(8):
            out.append(("tor_pair/A%d/R%d" % (i, j), encode(tors[i]), encode(tors[j]) + bytes(32), b"edge corpus: torsion pair"))
    return out


def make_batch(vectors):
    """(names, Batch) of a list of (name, pub, sig, msg)."""
    n = len(vectors)
    pub = np.frombuffer(b"".join(v[1] for v in vectors), np.uint8).reshape(n, 32).copy()
    sig = np.frombuffer(b"".join(v[2] for v in vectors), np.uint8).reshape(n, 64).copy()
    sz = np.array([len(v[3]) for v in vectors], np.uint32)
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint32)
    blob = np.frombuffer(b"".join(v[3] for v in vectors) + b"\0", np.uint8).copy()
    cls = np.array([CLASSES.index(v[0].split("/")[0]) for v in vectors], np.uint8)
    for a in (pub, sig, sz, off, blob, cls):
        a.setflags(write=False)
    return [v[0] for v in vectors], _golden.Batch(pub, sig, off, sz, blob, None, cls)


_corpus = None


def corpus(fresh=False):
    """(names, Batch), built once per process (fresh=True rebuilds, uncached)."""
    global _corpus
    if fresh:
        return make_batch(_build())
    if _corpus is None:
        _corpus = make_batch(_build())
    return _corpus


def digest(b):
    """SHA-256 over the batch's public keys, signatures, sizes and messages."""
    h = hashlib.sha256()
    for a in (b.pub, b.sig, b.msg_sz, b.blob):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def class_mask(b, *names):
    return np.isin(b.cls, [CLASSES.index(c) for c in names])


# ---- transactions whose one edge signer sits first, in the middle or last of three --------------

TXN_KINDS = ["nc_a", "mix_a_accept", "mix_a_reject", "A=B,R=identity", "near_a"]


def _edge_signer(kind, msg):
    """(encoded A, signature over msg) of the edge signer of `kind`; where the
    case needs a property of h, the nonce is ground, not the message."""
    tors = torsion()
    if kind == "nc_a":
        e = _yenc(P + 3, 0)                                   # decodes to the non-torsion point with y = 3
        return e, sign_chosen(KEY_A, e, NONCE_R, encode(S.mul(NONCE_R, S.B)), msg)
    if kind == "near_a":
        e = _yenc(y8() - 1, 0)                                # on the curve, one below an order-8 y
        return e, sign_chosen(KEY_A, e, NONCE_R, encode(S.mul(NONCE_R, S.B)), msg)
    if kind == "A=B,R=identity":
        e = encode(S.B)
        return e, sign_chosen(1, e, 0, encode(S.IDENT), msg)
    e = encode(S.add(S.mul(KEY_A, S.B), tors[1]))             # an order-8 component
    for c in range(256):
        r = (NONCE_R + c) % L
        re = encode(S.mul(r, S.B))
        if (hram(re, e, msg) % 8 == 0) == (kind == "mix_a_accept"):
            return e, sign_chosen(KEY_A, e, r, re, msg)
    raise AssertionError("no nonce found")


_txns = None


def txn_cases():
    """[(name, payload, position of the edge signer)]: 3-signer transactions
    over _txn.message, the edge signer of each TXN_KINDS first, in the middle
    and last; the other two signers are honest."""
    global _txns
    if _txns is None:
        import _txn
        rng = np.random.default_rng(0xed9e5)
        out = []
        for kind in TXN_KINDS:
            for pos in range(3):
                ks = [_clamp(_h512(b"edge corpus: txn signer %d %d" % (len(out), j))) for j in range(3)]
                pubs = [encode(S.mul(k, S.B)) for k in ks]
                pubs[pos] = _edge_signer(kind, b"")[0]
                msg = _txn.message(rng, pubs, 120 + 40 * pos, len(out) & 1 == 0, 1 + pos % 2)
                sigs = []
                for j in range(3):
                    if j == pos:
                        e, sg = _edge_signer(kind, msg)
                        assert e == pubs[j]
                    else:
                        r = int.from_bytes(_h512(b"edge corpus: txn nonce %d %d" % (len(out), j)), "little") % L
                        sg = sign_chosen(ks[j], pubs[j], r, encode(S.mul(r, S.B)), msg)
                    sigs.append(sg)
                out.append(("%s/%d" % (kind, pos), bytes([3]) + b"".join(sigs) + msg, pos))
        _txns = out
    return _txns
