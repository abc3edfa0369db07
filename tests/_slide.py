"""Pure-Python restatement of fd_ed25519_ge_slide (src/ballet/ed25519/
avx/fd_ed25519_ge.c:378-400) and of h = SHA-512(R||A||M) mod L
(fd_ed25519_user.c:411-414) -- small-case checker for the k_prep digits."""
import hashlib

L = 2**252 + 27742317777372353535851937790883648493


def slide(a):
    r = [(a >> i) & 1 for i in range(256)]
    for i in range(256):
        if not r[i]:
            continue
        for b in range(1, 7):
            if i + b >= 256:
                break
            if not r[i + b]:
                continue
            if r[i] + (r[i + b] << b) <= 15:
                r[i] += r[i + b] << b
                r[i + b] = 0
            elif r[i] - (r[i + b] << b) >= -15:
                r[i] -= r[i + b] << b
                for k in range(i + b, 256):
                    if not r[k]:
                        r[k] = 1
                        break
                    r[k] = 0
            else:
                break
    return r


def h_scalar(sig, pub, msg):
    return int.from_bytes(hashlib.sha512(bytes(sig[:32]) + bytes(pub) + bytes(msg)).digest(), "little") % L


def crafted_scalars():
    """Scalars < L aimed at the slide's carry: a hash output never holds a
    run of ~58 or more one-bits across a 64-bit word, so k_prep's multi-word
    carry (w1 += c; c = c && w1 == 0; ...) runs only on inputs like these.
    Also single bits, the ends of the range and the densest digit patterns
    (events are >= 5 positions apart: at most 51 per 253-bit scalar)."""
    out = [0, 1] + [1 << j for j in range(1, 253)] + [2**252 - 1, L - 1]
    out += [((1 << 130) - 1) << 60, ((1 << 192) - 1) << 58]
    for n in (58, 59, 64, 65, 130, 192):
        for edge in (64, 128, 192):
            for shift in (edge - n + 1, edge - n // 2, edge - 6, edge - 1):   # the run covers bit `edge`
                if shift >= 0:
                    out.append(((1 << n) - 1) << shift)
            # the run ends just below a word that is itself all ones: the carry crosses two words
            out.append((((1 << n) - 1) << max(edge - n, 0)) | (((1 << 64) - 1) << edge))
    out += [int("10" * 126, 2), int("100001" * 42, 2), int("10000" * 50 + "1", 2), int("1" * 252, 2),
            int("110111" * 42, 2), int("0111101" * 36, 2)]
    return sorted({a for a in out if 0 <= a < L})
