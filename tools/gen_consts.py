#!/usr/bin/env python3
"""Regenerate every numeric constant of the ed25519 verify path from first
principles and emit it as a C header.

Nothing here is copied from the reference: each table is recomputed from its
mathematical definition and then *checked* against the reference's own tables
by ``oracle/check_consts_vs_ref.py`` (run in the build container only).

  * SHA-512 K[80] / H0[8]      FIPS 180-4 s4.2.3 / s5.3.5 (cube / square roots
                               of the first primes).  Reference users:
                               src/ballet/sha512/fd_sha512.c (core), checked
                               against hashlib in tests.
  * d, 2d, sqrt(-1)            RFC 8032 s5.1; reference limbs at
                               src/ballet/ed25519/avx/fd_ed25519_ge.c:233-244,
                               :278-280, :426-437.
  * Bi[8] = (2k+1)*B, k=0..7   Duif form (y+x, y-x, 2dxy) of the odd multiples
                               of the base point; reference table
                               src/ballet/ed25519/table/fd_ed25519_ge_bi_precomp.c
                               and its lane-swizzled twin
                               table/fd_ed25519_ge_bi_precomp_avx.c:30-112
                               (lanes [1, y-x, y+x, 2dxy]).
  * L                          group order, fd_ed25519_user.c:368-376.

Limb convention: a field element v (mod p) is centred
(v -> v - p when 2v > p) and split over 10 signed limbs of widths
26,25,26,25,... with rounding carries c = (v + 2^(w-1)) >> w on limbs 0..8;
limb 9 keeps the remainder.

Usage:  python3 tools/gen_consts.py <out.h> <prefix>
"""
import sys
from math import isqrt

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
WIDTHS = [26, 25] * 5


def _primes(n):
    ps, k = [], 2
    while len(ps) < n:
        if all(k % p for p in ps if p * p <= k):
            ps.append(k)
        k += 1
    return ps


def _icbrt(n):
    x = int(round(n ** (1.0 / 3)))
    while True:
        y = (2 * x + n // (x * x)) // 3
        if abs(y - x) <= 1:
            for c in range(y - 3, y + 4):
                if c ** 3 <= n < (c + 1) ** 3:
                    return c
        x = y


def sha512_k():
    return [_icbrt(p << 192) & (2**64 - 1) for p in _primes(80)]


def sha512_h0():
    return [isqrt(p << 128) & (2**64 - 1) for p in _primes(8)]


def inv(x):
    return pow(x, P - 2, P)


D = (-121665 * inv(121666)) % P
D2 = (2 * D) % P
SQRTM1 = pow(2, (P - 1) // 4, P)


def recover_x(y, sign):
    x2 = (y * y - 1) * inv(D * y * y + 1) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRTM1 % P
    assert (x * x - x2) % P == 0
    if x & 1 != sign:
        x = P - x
    return x


BY = 4 * inv(5) % P
BX = recover_x(BY, 0)


def edwards_add(p1, p2):
    x1, y1 = p1
    x2, y2 = p2
    t = D * x1 * x2 * y1 * y2 % P
    x3 = (x1 * y2 + x2 * y1) * inv(1 + t) % P
    y3 = (y1 * y2 + x1 * x2) * inv(1 - t) % P
    return (x3, y3)


def limbs(v):
    v %= P
    if 2 * v > P:
        v -= P
    out = []
    for w in WIDTHS[:9]:
        c = (v + (1 << (w - 1))) >> w
        out.append(v - (c << w))
        v = c
    out.append(v)
    assert all(-(1 << 31) <= x < (1 << 31) for x in out)
    return out


def bi_table():
    """Bi[k] = (2k+1)B in Duif form, rows (yplusx, yminusx, xy2d)."""
    B = (BX, BY)
    B2 = edwards_add(B, B)
    pts, cur = [], B
    for _ in range(8):
        pts.append(cur)
        cur = edwards_add(cur, B2)
    rows = []
    for (x, y) in pts:
        rows.append((limbs(y + x), limbs(y - x), limbs(2 * D * x * y)))
    return rows


def edwards_double(p1):
    return edwards_add(p1, p1)


def base_comb_table():
    """BASE[j][k] = (k+1) * 256^j * B, j = 0..31, k = 0..7, Duif form
    (y+x, y-x, 2dxy): the fixed-base table of signed radix-16 scalar
    multiplication (RFC 8032 s5.1.4 [s]B; the GPU signer, workload
    synthesis only -- canonical outputs, so any exact table works)."""
    out = []
    P0 = (BX, BY)
    for j in range(32):
        row, cur = [], P0
        for k in range(8):
            x, y = cur
            row.append((limbs(y + x), limbs(y - x), limbs(2 * D * x * y)))
            cur = edwards_add(cur, P0)
        out.append(row)
        for _ in range(8):
            P0 = edwards_double(P0)
    return out


def fe_sqrt(a):
    """A square root of a mod p (p = 5 mod 8), or None when a is no square."""
    a %= P
    x = pow(a, (P + 3) // 8, P)
    if (x * x - a) % P:
        x = x * SQRTM1 % P
    return x if (x * x - a) % P == 0 else None


def torsion_y8():
    """y of the four points of order 8.  The double of (x, y) on
    -x^2 + y^2 = 1 + d x^2 y^2 has y' = (y^2 + x^2) / (1 - d x^2 y^2), so the
    points whose double is (+-sqrt(-1), 0), of order 4, are those with
    x^2 = -y^2; the curve equation then reads d y^4 + 2 y^2 - 1 = 0, i.e.
    y^2 = (-1 +- sqrt(1 + d)) / d, for the root that is itself a square.
    Returns the lesser y (the other is p - y).  Checked by doubling:
    [4](x, y) = (0, -1), [8](x, y) = (0, 1).  The 8 torsion points then have
    y in {1, p-1, 0, y8, p-y8} (strict mode's point check)."""
    ys = set()
    r = fe_sqrt(1 + D)
    for t in ((-1 + r) * inv(D) % P, (-1 - r) * inv(D) % P):
        y = fe_sqrt(t)
        if y is None:
            continue
        x = SQRTM1 * y % P
        for pt in ((x, y), (x, P - y), (P - x, y), (P - x, P - y)):
            p4 = edwards_double(edwards_double(pt))
            assert (-pt[0] * pt[0] + pt[1] * pt[1] - 1 - D * pt[0] * pt[0] * pt[1] * pt[1]) % P == 0
            assert p4 == (0, P - 1) and edwards_double(p4) == (0, 1)
        ys.update((y, P - y))
    assert len(ys) == 2
    return min(ys)


def _words(v):
    return "{ " + ", ".join("0x%08xu" % ((v >> (32 * k)) & 0xffffffff) for k in range(8)) + " }"


def _carr(vals):
    return "{ " + ", ".join(str(v) for v in vals) + " }"


def emit(path, prefix):
    pf = prefix.upper()
    lines = [
        "/* GENERATED by tools/gen_consts.py -- do not edit.  Every value is",
        "   recomputed from its definition (see the generator's docstring) and",
        "   checked against the reference tables by oracle/check_consts_vs_ref.py. */",
        f"#ifndef {pf}_CONSTS_H",
        f"#define {pf}_CONSTS_H",
        "",
        f"#define {pf}_SHA512_K {{ " + ", ".join("0x%016xUL" % k for k in sha512_k()) + " }",
        f"#define {pf}_SHA512_H0 {{ " + ", ".join("0x%016xUL" % h for h in sha512_h0()) + " }",
        "",
        "/* field constants, 10 x int32 limbs (26/25-bit, centred) */",
        f"#define {pf}_FE_D      {_carr(limbs(D))}",
        f"#define {pf}_FE_D2     {_carr(limbs(D2))}",
        f"#define {pf}_FE_SQRTM1 {_carr(limbs(SQRTM1))}",
        "",
        "/* Bi[k] = (2k+1)B, k = 0..7, as [k][row][limb] with rows",
        "   0: y+x, 1: y-x, 2: 2dxy (Duif form) */",
        f"#define {pf}_BI_PRECOMP {{ \\",
    ]
    for k, (ypx, ymx, xy2d) in enumerate(bi_table()):
        sep = "," if k < 7 else ""
        lines.append(f"  {{ {_carr(ypx)}, {_carr(ymx)}, {_carr(xy2d)} }}{sep} \\")
    lines.append("}")
    lines.append("")
    if pf == "FD_AMD":
        lines.append("/* BASE[j][k] = (k+1) 256^j B, rows y+x, y-x, 2dxy (GPU signer) */")
        lines.append(f"#define {pf}_BASE_COMB {{ \\")
        tab = base_comb_table()
        for j, row in enumerate(tab):
            ents = ", ".join("{ %s, %s, %s }" % (_carr(a), _carr(b), _carr(c)) for (a, b, c) in row)
            lines.append("  { %s }%s \\" % (ents, "," if j < 31 else ""))
        lines.append("}")
        lines.append("")
    lb = L.to_bytes(32, "little")
    lines.append(f"#define {pf}_L_BYTES {{ " + ", ".join("0x%02x" % b for b in lb) + " }")
    lines.append("")
    y8 = torsion_y8()
    lines.append("/* y of the points of order 8 (y8 and p - y8) as 8 little-endian 32-bit words:")
    lines.append("   with y in {0, 1, p-1} the y of every torsion point (strict mode) */")
    lines.append(f"#define {pf}_Y8_WORDS  {_words(y8)}")
    lines.append(f"#define {pf}_Y8N_WORDS {_words(P - y8)}")
    lines.append("")
    lines.append(f"#endif /* {pf}_CONSTS_H */")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    emit(sys.argv[1], sys.argv[2])
