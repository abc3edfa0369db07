"""Independent strict RFC 8032 verifier -- TEST CHECKER ONLY.

Python big integers and hashlib.sha512; extended coordinates, double-and-add.
It shares nothing with the device code, the generated constants or the CPU
oracle.  The rule (include/fd_ed25519_amd.h, FD_ED25519_AMD_MODE_STRICT), in
this order:
  1. s >= L                                                   -> -1
  2. A or R: y >= p, not on the curve, x = 0 with the sign bit
     set, or a torsion point ([8]P = identity)                -> -2
  3. [s]B - [h]A != R as points, h = SHA-512(R||A||M) mod L   -> -3
  4. otherwise                                                ->  0
"""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRTM1 = pow(2, (P - 1) // 4, P)
IDENT = (0, 1, 1, 0)


def add(p, q):
    """Unified addition on -x^2 + y^2 = 1 + d x^2 y^2, extended coordinates."""
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A, B = (Y1 - X1) * (Y2 - X2) % P, (Y1 + X1) * (Y2 + X2) % P
    C, Dd = 2 * D * T1 * T2 % P, 2 * Z1 * Z2 % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def mul(k, p):
    q = IDENT
    while k:
        if k & 1:
            q = add(q, p)
        p = add(p, p)
        k >>= 1
    return q


def is_identity(p):
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


def decode(b):
    """32 bytes -> point, or None when the strict rule rejects the encoding
    itself (y >= p, off the curve, x = 0 with the sign bit set)."""
    y = int.from_bytes(b, "little")
    sign, y = y >> 255, y & ((1 << 255) - 1)
    if y >= P:
        return None
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x2 = u * pow(v, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRTM1 % P
    if (x * x - x2) % P:
        return None
    if x == 0 and sign:
        return None
    if x & 1 != sign:
        x = P - x
    return (x, y, 1, x * y % P)


BY = 4 * pow(5, P - 2, P) % P
B = decode(BY.to_bytes(32, "little"))


def verify(msg, sig, pub):
    sig, pub, msg = bytes(sig), bytes(pub), bytes(msg)
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return -1
    A, R = decode(pub), decode(sig[:32])
    if A is None or R is None or is_identity(mul(8, A)) or is_identity(mul(8, R)):
        return -2
    h = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % L
    Rp = add(mul(s, B), mul(h, (P - A[0], A[1], 1, P - A[3])))
    if (Rp[0] - R[0] * Rp[2]) % P or (Rp[1] - R[1] * Rp[2]) % P:
        return -3
    return 0


_cache = {}


def verify_batch(batch, idx=None):
    """Strict verdicts of batch[idx] (all when idx is None) as a list; each
    distinct (msg, sig, pub) is computed once per process."""
    out = []
    for i in (range(len(batch)) if idx is None else idx):
        key = (batch.msg(i), bytes(batch.sig[i]), bytes(batch.pub[i]))
        if key not in _cache:
            _cache[key] = verify(*key)
        out.append(_cache[key])
    return out
