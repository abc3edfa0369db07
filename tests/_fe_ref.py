"""Plain-integer model of the reference's lane arithmetic (the AVX build's
field ops, avx/fd_ed25519_fe_avx_inl.h:484-674, and the group steps of
avx/fd_ed25519_ge.c:408-527 as oracle/fd_ed25519_oracle.c writes them), and
the directed input classes of the limb-exact field tests.

Field element = list of ten Python ints (int32 limbs, radix 2^25.5).  The
int32 pre-multiples (2f, 19g, 38f) WRAP as the reference's do, products and
column sums are exact, and every 64-bit intermediate is asserted to fit
int64, so no test input can rest on an overflow.  tests/test_fe_ref_cpu.py
pins this model to the oracle and to the mathematics; the GPU probes
(tests/test_field_probe_gpu.py) are compared against it limb for limb."""
import random

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
M64 = 1 << 64
EXP = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]   # limb k weighs 2^EXP[k]
WID = [26, 25] * 5


def i64(x):
    x %= M64
    return x - M64 if x >= 1 << 63 else x


def i32(x):
    x %= 1 << 32
    return x - (1 << 32) if x >= 1 << 31 else x


def fits64(x):
    assert -(1 << 63) <= x < (1 << 63), "int64 overflow in the model: %d" % x
    return x


def value(f):
    return sum(v << e for v, e in zip(f, EXP)) % P


def limbs(v):
    """Balanced limbs of v mod p (even |limb| <= 2^25, odd <= 2^24)."""
    v %= P
    if 2 * v > P:
        v -= P
    out = []
    for w in WID[:9]:
        c = (v + (1 << (w - 1))) >> w
        out.append(v - (c << w))
        v = c
    out.append(v)
    return out


D = (-121665 * pow(121666, P - 2, P)) % P
FE_D, FE_D2, FE_SQRTM1 = limbs(D), limbs(2 * D), limbs(pow(2, (P - 1) // 4, P))
FE_ONE = [1] + [0] * 9

# the twelve steps of the reference carry chain: (limb, width, next limb, factor)
CARRY_STEPS = [(0, 26, 1, 1), (4, 26, 5, 1), (1, 25, 2, 1), (5, 25, 6, 1), (2, 26, 3, 1), (6, 26, 7, 1),
               (3, 25, 4, 1), (7, 25, 8, 1), (4, 26, 5, 1), (8, 26, 9, 1), (9, 25, 0, 19), (0, 26, 1, 1)]


def ref_carry(h, trace=None):
    """Reference carry chain (avx/fd_ed25519_fe_avx_inl.h:570-584) on ten
    column sums; trace (a list) receives the value each step rounds."""
    h = [fits64(v) for v in h]
    for k, w, nxt, mul in CARRY_STEPS:
        if trace is not None:
            trace.append(h[k])
        cc = fits64(h[k] + (1 << (w - 1))) >> w
        h[nxt] = fits64(h[nxt] + cc * mul)
        h[k] -= cc << w
    return [i32(v) for v in h]


def fe_add(f, g): return [i32(a + b) for a, b in zip(f, g)]
def fe_sub(f, g): return [i32(a - b) for a, b in zip(f, g)]
def fe_neg(f): return [i32(-a) for a in f]


def mul_cols(f, g):
    """Column sums of FE_AVX_INL_MUL and whether a pre-multiple wrapped."""
    g19 = [i32(19 * v) for v in g]
    f2 = [i32(2 * v) for v in f]
    wrapped = any(g19[j] != 19 * g[j] for j in range(1, 10)) or any(f2[i] != 2 * f[i] for i in range(1, 10, 2))
    h = [0] * 10
    for i in range(10):
        for j in range(10):
            a = f2[i] if (i & 1 and j & 1) else f[i]
            b = g19[j] if i + j >= 10 else g[j]
            h[(i + j) % 10] = fits64(h[(i + j) % 10] + a * b)
    return h, wrapped


def fe_mul(f, g):
    return ref_carry(mul_cols(f, g)[0])


def sqn_cols(f, n=1):
    """Column sums of FE_AVX_INL_SQN (doubled when n == 2) and the wrap flag."""
    t2 = [i32(2 * v) for v in f]
    f5_38, f6_19, f7_38, f8_19, f9_38 = i32(38 * f[5]), i32(19 * f[6]), i32(38 * f[7]), i32(19 * f[8]), i32(38 * f[9])
    wrapped = (any(t2[k] != 2 * f[k] for k in range(8)) or f5_38 != 38 * f[5] or f6_19 != 19 * f[6]
               or f7_38 != 38 * f[7] or f8_19 != 19 * f[8] or f9_38 != 38 * f[9])
    h = [
        f[0]*f[0] + t2[1]*f9_38 + t2[2]*f8_19 + t2[3]*f7_38 + t2[4]*f6_19 + f[5]*f5_38,
        t2[0]*f[1] + f[2]*f9_38 + t2[3]*f8_19 + f[4]*f7_38 + t2[5]*f6_19,
        t2[0]*f[2] + t2[1]*f[1] + t2[3]*f9_38 + t2[4]*f8_19 + t2[5]*f7_38 + f[6]*f6_19,
        t2[0]*f[3] + t2[1]*f[2] + f[4]*f9_38 + t2[5]*f8_19 + f[6]*f7_38,
        t2[0]*f[4] + t2[1]*t2[3] + f[2]*f[2] + t2[5]*f9_38 + t2[6]*f8_19 + f[7]*f7_38,
        t2[0]*f[5] + t2[1]*f[4] + t2[2]*f[3] + f[6]*f9_38 + t2[7]*f8_19,
        t2[0]*f[6] + t2[1]*t2[5] + t2[2]*f[4] + t2[3]*f[3] + t2[7]*f9_38 + f[8]*f8_19,
        t2[0]*f[7] + t2[1]*f[6] + t2[2]*f[5] + t2[3]*f[4] + f[8]*f9_38,
        t2[0]*f[8] + t2[1]*t2[7] + t2[2]*f[6] + t2[3]*t2[5] + f[4]*f[4] + f[9]*f9_38,
        t2[0]*f[9] + t2[1]*f[8] + t2[2]*f[7] + t2[3]*f[6] + t2[4]*f[5],
    ]
    # a sum of at most six products below 2^62 in magnitude: checked term by term through the total
    h = [fits64(v) for v in h]
    if n == 2:
        h = [fits64(2 * v) for v in h]
    return h, wrapped


def fe_sqn(f, n=1):
    return ref_carry(sqn_cols(f, n)[0])


def fe_mul_one(f):
    return ref_carry(f)


def sq_term_cols(f, d2):
    """The device's sq_term column sums (fd_ed25519_dev.h): pair (i <= j) of
    column K, its power of two as a shift of f_i, the 19 on f_j, every
    operand an int32 with wrap (the shift and the x19 are 32-bit)."""
    h = [0] * 10
    f19 = [i32(19 * v) for v in f]
    for K in range(10):
        for i in range(10):
            j = (K - i + 10) % 10
            if i > j:
                continue
            c2 = (i != j) + (1 if (i & 1 and j & 1) else 0) + (1 if d2 else 0)
            h[K] = fits64(h[K] + i32(f[i] << c2) * (f19[j] if i + j >= 10 else f[j]))
    return h


def fe_sq_iter(f, n):
    for _ in range(n):
        f = fe_sqn(f, 1)
    return f


def fe_pow22523(z):
    """fe_avx_pow22523 (avx/fd_ed25519_fe_avx.h:246-275): z^(2^252-3)."""
    t0 = fe_sqn(z)
    t1 = fe_sq_iter(t0, 2)
    t1 = fe_mul(z, t1)
    t0 = fe_mul(t0, t1)
    t0 = fe_sqn(t0)
    t0 = fe_mul(t1, t0)
    t1 = fe_sq_iter(t0, 5)
    t0 = fe_mul(t1, t0)
    t1 = fe_sq_iter(t0, 10)
    t1 = fe_mul(t1, t0)
    t2 = fe_sq_iter(t1, 20)
    t1 = fe_mul(t2, t1)
    t1 = fe_sq_iter(t1, 10)
    t0 = fe_mul(t1, t0)
    t1 = fe_sq_iter(t0, 50)
    t1 = fe_mul(t1, t0)
    t2 = fe_sq_iter(t1, 100)
    t1 = fe_mul(t2, t1)
    t1 = fe_sq_iter(t1, 50)
    t0 = fe_mul(t1, t0)
    t0 = fe_sq_iter(t0, 2)
    return fe_mul(t0, z)


def fe_frombytes(s):
    """fd_ed25519_fe_frombytes (avx/fd_ed25519_fe.c:4-46); s = 32 bytes."""
    def ld(k, n): return int.from_bytes(s[k:k + n], "little")
    h = [ld(0, 4), ld(4, 3) << 6, ld(7, 3) << 5, ld(10, 3) << 3, ld(13, 3) << 2, ld(16, 4), ld(20, 3) << 7,
         ld(23, 3) << 5, ld(26, 3) << 4, (ld(29, 3) & 0x7fffff) << 2]
    for k, w, nxt, mul in [(9, 25, 0, 19), (1, 25, 2, 1), (3, 25, 4, 1), (5, 25, 6, 1), (7, 25, 8, 1),
                           (0, 26, 1, 1), (2, 26, 3, 1), (4, 26, 5, 1), (6, 26, 7, 1), (8, 26, 9, 1)]:
        c = (h[k] + (1 << (w - 1))) >> w
        h[nxt] += c * mul
        h[k] -= c << w
    return [i32(v) for v in h]


def fe_reduce(f):
    """fd_ed25519_fe_tobytes' canonicalisation (avx/fd_ed25519_fe.c:48-110) in
    its own int32 steps: the ten reduced limbs.  It yields value(f) mod p for
    the limb ranges the decompression feeds it (differences of two carried
    elements); outside (2p written in doubled limbs) it is still what the
    reference computes, and that is what the device must give."""
    h = list(f)
    q = i32(19 * h[9] + (1 << 24)) >> 25
    for i in range(10):
        q = i32(h[i] + q) >> WID[i]
    h[0] = i32(h[0] + 19 * q)
    for i in range(9):
        h[i + 1] = i32(h[i + 1] + (h[i] >> WID[i]))
        h[i] &= (1 << WID[i]) - 1
    h[9] &= (1 << 25) - 1
    return h


def fe_tobytes(f):
    return sum(v << e for v, e in zip(fe_reduce(f), EXP)).to_bytes(32, "little")


def fe_isnonzero(f): return int(any(fe_reduce(f)))
def fe_isnegative(f): return fe_reduce(f)[0] & 1


# ---- group steps, as the oracle writes them; points are 4-tuples of elements ----

def dbl(X, Y, Z):
    a, b, c, d = fe_sqn(fe_add(X, Y)), fe_sqn(Y), fe_sqn(X), fe_sqn(Z, 2)
    return ([i32(a[k] - b[k] - c[k]) for k in range(10)], fe_add(b, c), fe_sub(b, c),
            [i32(d[k] - b[k] + c[k]) for k in range(10)])


def p1p1_to_p3(t):
    X, Y, Z, T = t
    return (fe_mul(X, T), fe_mul(Y, Z), fe_mul(Z, T), fe_mul(X, Y))


def add_cached(u, q, neg):
    """u = p3 (X, Y, Z, T), q = cached (Z, YmX, YpX, T2d)."""
    X, Y, Z, T = u
    qZ, qM, qP, qT = q
    ZZ = fe_mul(Z, qZ)
    MM = fe_mul(fe_sub(Y, X), qP if neg else qM)
    PP = fe_mul(fe_add(Y, X), qM if neg else qP)
    TT = fe_mul(T, qT)
    z2 = fe_add(ZZ, ZZ)
    zp, zm = fe_add(z2, TT), fe_sub(z2, TT)
    return (fe_sub(PP, MM), fe_add(PP, MM), zm if neg else zp, zp if neg else zm)


def p3_to_cached(u):
    X, Y, Z, T = u
    Z1, Y1, X1 = fe_mul(Z, FE_ONE), fe_mul(Y, FE_ONE), fe_mul(X, FE_ONE)
    return (Z1, fe_sub(Y1, X1), fe_add(Y1, X1), fe_mul(T, FE_D2))


# ---- input classes ------------------------------------------------------------
# Bounds (tests/test_fe_ref_cpu.py::test_operand_maxima measures the oracle's
# operands and asserts they lie inside CALLER):
#   CARRIED  an output of the carry chain: even |limb| <= 2^25, odd <= 2^24
#            (+ a unit carry in limbs 1 and 5)
#   SUM2     a sum / difference of two carried elements (X+Y, Y-X, cached rows)
#   CALLER   a p1p1 mix of three (a-b-c, d-b+c, 2Z+-T): the widest operand
#   WRAP     2^27: 19 g and 38 f wrap in int32, sums still inside int64
CARRIED = [(1 << 25) if k % 2 == 0 else (1 << 24) for k in range(10)]
CARRIED[1] += 1
CARRIED[5] += 1
SUM2 = [2 * b for b in CARRIED]
CALLER = [3 * b for b in CARRIED]
WRAP = [1 << 27] * 10
SQ2W = [(1 << 26) if k % 2 == 0 else (1 << 25) for k in range(10)]    # fe_sq_fold2w's X+Y-like operand
SQ2W_D2 = [(1 << 25) if k % 2 == 0 else (1 << 24) for k in range(10)]  # its sq2 operand (Z-like)


def rand_fe(rng, bound):
    return [rng.randint(-b, b) for b in bound]


def rand_carried(rng):
    """An actual output of the reference carry chain on random column sums."""
    return ref_carry([rng.randrange(-(1 << 58), 1 << 58) for _ in range(10)])


def edge_fes(bound):
    """Every limb at +- its bound: all +, all -, both alternations, and each
    single limb at +-bound with the rest zero."""
    out = [list(bound), [-b for b in bound], [b * (-1) ** k for k, b in enumerate(bound)],
           [-b * (-1) ** k for k, b in enumerate(bound)]]
    for k in range(10):
        for s in (1, -1):
            e = [0] * 10
            e[k] = s * bound[k]
            out.append(e)
    return out


def onehot_pairs(bound_f, bound_g):
    """All 10 x 10 (i, j) one-hot operand pairs at the bound, three sign
    patterns: isolates each product term with its x2 / x19 factor."""
    out = []
    for i in range(10):
        for j in range(10):
            for sf, sg in ((1, 1), (1, -1), (-1, -1)):
                f, g = [0] * 10, [0] * 10
                f[i], g[j] = sf * bound_f[i], sg * bound_g[j]
                out.append((f, g))
    return out


def _centre(x, w):
    x %= 1 << w
    return x - (1 << w) if x >= 1 << (w - 1) else x


# step -> first limb of f that must be zero so that the variable limb (g[c]
# resp. f[c]) is in no column that carries into the step's limb earlier in
# its run of the chain (0->1->2->3->4 and 4->5->...->9): limb c meets f[j] in
# column c + j - 10
ZERO_FROM = {0: 10, 2: 9, 4: 8, 6: 7, 8: 6, 1: 10, 3: 9, 5: 8, 7: 7, 9: 6, 10: 5}


def boundary_mul_pairs(rng, per_d=2):
    """Operand pairs whose carry chain rounds, at a chosen step, a value
    h = k 2^w + 2^(w-1) + d with d in {-1, 0, 1} (the rounding boundary of
    (h + 2^(w-1)) >> w).  Found with the model: g[c] enters column c with
    the odd coefficient f[0], and with the top limbs of f zero (ZERO_FROM)
    it is in no column that carries in, so the residue of the step is
    solved exactly; the last step (limb 0 again) uses a one-hot f so that
    the x19 carry does not depend on g[0].  Every returned pair is verified
    to hit its step."""
    out = []
    for step, (c, w, _, _) in enumerate(CARRY_STEPS):
        for d in (-1, 0, 1):
            got = 0
            for _ in range(50):
                if got >= per_d:
                    break
                f, g = rand_carried(rng), rand_carried(rng)
                f[0] |= 1
                z = 1 if step == 11 else ZERO_FROM[step]
                f = f[:z] + [0] * (10 - z)
                tr = []
                ref_carry(mul_cols(f, g)[0], tr)
                need = (1 << (w - 1)) + d - tr[step]
                g[c] = _centre(g[c] + need * pow(f[0], -1, 1 << w), w)
                tr = []
                ref_carry(mul_cols(f, g)[0], tr)
                if (tr[step] - (1 << (w - 1)) - d) % (1 << w) == 0:
                    out.append((f, g) if got & 1 else (g, f))   # the sums are symmetric in f, g: both operand paths
                    got += 1
            assert got == per_d, ("no rounding-boundary pair found", step, d)
    return out


SQ_STEPS = [s for s in range(11) if CARRY_STEPS[s][0] not in (0, 9) and CARRY_STEPS[s][0] < ZERO_FROM[s]]


def boundary_sq(rng, n=1, tries=4000):
    """Squares whose carry chain rounds a boundary value (see
    boundary_mul_pairs): column c holds 2 n f0 f_c, so the residue of a step
    is solved when the parity allows.  Steps whose limb squares into an
    earlier column of its own run (limbs 7, 8) and limbs 0, 9 are left to
    the products' class."""
    out, hit = [], set()
    for _ in range(tries):
        if len(hit) >= 3 * len(SQ_STEPS):
            break
        step = rng.choice(SQ_STEPS)
        c, w, _, _ = CARRY_STEPS[step]
        f = rand_carried(rng)
        f[0] |= 1
        f = f[:ZERO_FROM[step]] + [0] * (10 - ZERO_FROM[step])
        tr = []
        ref_carry(sqn_cols(f, n)[0], tr)
        for d in (0, 1, -1):
            need = (1 << (w - 1)) + d - tr[step]
            if need % (2 * n) or (step, d) in hit:
                continue
            g = list(f)
            g[c] = _centre(f[c] + (need // (2 * n)) * pow(f[0], -1, 1 << w), w)
            tr2 = []
            ref_carry(sqn_cols(g, n)[0], tr2)
            if (tr2[step] - (1 << (w - 1)) - d) % (1 << w) == 0:
                out.append(g)
                hit.add((step, d))
                break
    assert {s for s, _ in hit} == set(SQ_STEPS) and len(hit) >= 2 * len(SQ_STEPS), ("too few rounding-boundary squares", sorted(hit))
    return out


def mul_pairs(seed, wrap=True, n_random=1024):
    """The (f, g) classes of a general product, as {class name: [pairs]}."""
    rng = random.Random(seed)
    cls = {}
    cls["random_carried"] = [(rand_carried(rng), rand_carried(rng)) for _ in range(n_random)]
    edges = []
    for bf, bg in ((CARRIED, CARRIED), (CALLER, SUM2), (SUM2, CALLER), (CALLER, CALLER)):
        ef, eg = edge_fes(bf), edge_fes(bg)
        edges += [(f, g) for f in ef[:4] for g in eg[:4]]
        edges += [(f, rand_fe(rng, bg)) for f in ef[4:]] + [(rand_fe(rng, bf), g) for g in eg[4:]]
        edges += onehot_pairs(bf, bg)
    cls["edges"] = edges
    cls["caller_maxima"] = ([(rand_fe(rng, CALLER), rand_fe(rng, CALLER)) for _ in range(512)]
                            + [([rng.choice((-b, b)) for b in CALLER], [rng.choice((-b, b)) for b in CALLER])
                               for _ in range(512)])
    cls["rounding"] = boundary_mul_pairs(rng)
    if wrap:
        cls["wrap"] = ([(rand_fe(rng, WRAP), rand_fe(rng, WRAP)) for _ in range(512)]
                       + [(f, g) for f in edge_fes(WRAP)[:4] for g in edge_fes(WRAP)[:4]] + onehot_pairs(WRAP, WRAP))
    return cls


def sq_inputs(seed, n=1, wrap=True, caller=SUM2, n_random=1024):
    """The classes of a square: {class name: [f]}.  caller: the widest
    operand the op's callers feed it (X+Y of carried limbs; Z for sq2)."""
    rng = random.Random(seed)
    cls = {}
    cls["random_carried"] = [rand_carried(rng) for _ in range(n_random)]
    cls["edges"] = edge_fes(CARRIED) + edge_fes(caller) + [
        [sf * caller[i] if k == i else sg * caller[j] if k == j else 0 for k in range(10)]
        for i in range(10) for j in range(i + 1, 10) for sf, sg in ((1, 1), (1, -1), (-1, -1))]
    cls["caller_maxima"] = ([rand_fe(rng, caller) for _ in range(512)]
                            + [[rng.choice((-b, b)) for b in caller] for _ in range(512)])
    cls["rounding"] = boundary_sq(rng, n)
    if wrap:
        cls["wrap"] = [rand_fe(rng, WRAP) for _ in range(512)] + edge_fes(WRAP)
    return cls


def predicate_inputs(seed):
    """Limb patterns for fe_isnonzero / fe_isnegative: encodings of 0, +-1,
    p, 2p, -p, p+-1, 2^255-19+-k, in canonical limbs, in doubled / negated
    limbs, and as differences of two carried elements."""
    rng = random.Random(seed)
    def canon(v):   # non-negative limbs of an integer 0 <= v < 2^255
        out = []
        for w in WID:
            out.append(v & ((1 << w) - 1))
            v >>= w
        return out
    pl = canon(P)
    out = [[0] * 10, FE_ONE, fe_neg(FE_ONE), pl, [2 * v for v in pl], fe_neg(pl)]
    for k in (1, 2, 3, 18, 19, 20):
        out += [canon(P + k) if P + k < 1 << 255 else fe_add(pl, canon(k)), canon(P - k), fe_add(pl, canon(k)),
                fe_sub(pl, canon(k)), fe_sub([2 * v for v in pl], canon(k)), fe_neg(canon(P - k))]
    for _ in range(200):
        a = rand_carried(rng)
        k = rng.choice((0, 0, 0, 1, -1, 2, 19, -19))
        b = limbs(value(a) - k)               # a - b has the value k, limbs generally nonzero
        out += [fe_sub(a, b), fe_add(a, fe_neg(b)), fe_add(a, limbs(-value(a) + k))]
        # the same value with p or 2p folded into the limbs
        out.append(fe_add(fe_sub(a, b), pl))
        out.append(fe_sub(fe_sub(a, b), [2 * v for v in pl]))
    out += [rand_carried(rng) for _ in range(64)]
    return out


def frombytes_inputs(seed):
    rng = random.Random(seed)
    ys = [0, 1, 2, P - 2, P - 1, P, P + 1, P + 18, (1 << 255) - 1, (1 << 255) - 19, (1 << 255) - 20]
    ys += [(1 << j) for j in range(255)] + [(1 << 255) - 1 - (1 << j) for j in range(255)]
    ys += [rng.getrandbits(255) for _ in range(256)]
    out = []
    for y in ys:
        out.append(y.to_bytes(32, "little"))
        out.append((y | (1 << 255)).to_bytes(32, "little"))
    return out


def sc_reduce_inputs(seed):
    rng = random.Random(seed)
    xs = [0, 1, L - 1, L, L + 1, (1 << 512) - 1]
    for base in (1 << 252, 1 << 259):
        for dk in (-2, -1, 0, 1, 2):
            k = base + dk
            xs += [k * L - 1, k * L, k * L + 1]
    xs += [((1 << 512) - 1) // L * L + d for d in (-1, 0, 1)]
    xs += [1 << j for j in range(512)]
    xs += [rng.getrandbits(512) for _ in range(512)]
    return [x for x in xs if 0 <= x < 1 << 512]


def pow_inputs(seed):
    rng = random.Random(seed)
    return [[0] * 10, FE_ONE, fe_neg(FE_ONE), FE_SQRTM1, [2] + [0] * 9] + [rand_carried(rng) for _ in range(256)]


def point_inputs(seed, n, kind):
    """Tuples of four elements in the range the group steps see: 'p3' has
    carried coordinates (outputs of p1p1_to_p3), 'p1p1' the mixes of three
    (CALLER), 'cached' rows [Z | Y-X | Y+X | 2dT] (carried and SUM2); the
    first cases sit at the bounds."""
    rng = random.Random(seed)
    bounds = {"p3": [CARRIED] * 4, "p1p1": [CALLER] * 4, "cached": [CARRIED, SUM2, SUM2, CARRIED]}[kind]
    out = []
    for sgn in range(4):
        out.append(tuple(edge_fes(b)[sgn] for b in bounds))
    for k in range(4):   # one coordinate at its bound with alternating signs, the others random
        out.append(tuple(edge_fes(b)[2] if j == k else rand_fe(rng, b) for j, b in enumerate(bounds)))
    while len(out) < n:
        if kind == "p3" or rng.random() < 0.5:
            out.append(tuple(rand_carried(rng) if b is CARRIED else rand_fe(rng, b) for b in bounds))
        else:
            out.append(tuple([rng.choice((-x, x)) for x in b] for b in bounds))
    return out[:n]


# ---- the case sets both the CPU pin and the GPU probes use (fixed seeds) -------
import functools


@functools.lru_cache(maxsize=None)
def cases_mul():
    return mul_pairs(101)


@functools.lru_cache(maxsize=None)
def cases_sq(n):
    return sq_inputs(102 + n, n=n, caller=SUM2)


@functools.lru_cache(maxsize=None)
def cases_sq2w(d2):
    """fe_sq_fold2w's operands: X+Y-like (even <= 2^26, odd <= 2^25), Z-like
    for the sq2 slot as its comment states; exact by design, so no wrap class."""
    return sq_inputs(110 + d2, n=2 if d2 else 1, wrap=False, caller=SQ2W_D2 if d2 else SQ2W)


def flat(cls):
    """({class: [case]}) -> ([case], [class name per case])"""
    cases, names = [], []
    for name, cs in cls.items():
        cases += cs
        names += [name] * len(cs)
    return cases, names


@functools.lru_cache(maxsize=None)
def cases_points(kind):
    return point_inputs({"p3": 106, "p1p1": 107, "cached": 108}[kind], 300, kind)
