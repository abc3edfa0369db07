"""The Python model of the reference's lane arithmetic (tests/_fe_ref.py),
which the GPU probes are compared with limb for limb, pinned on the CPU:

  - to the oracle (oracle/fd_ed25519_oracle.c, itself pinned to the compiled
    reference): equal limbs on every input class the GPU tests use;
  - to the mathematics: value(out) == value(f) value(g) mod p wherever no
    int32 pre-multiple wrapped;
  - the classes' bounds to the operands the oracle really multiplies
    (test_operand_maxima);
  - fe_sq_fold2w's exact column sums to the reference's at the edge of the
    domain where they agree (test_sq_term_domain_edge).

CPU only."""
import random

import numpy as np

import _fe_ref as R
import _golden
import _oracle
import _slide


def _products(cls_of, model, oracle, math, wrapped):
    for name, cases in cls_of.items():
        exact = 0
        for c in cases:
            got = model(c)
            assert got == oracle(c), (name, c)
            if not wrapped(c):
                assert R.value(got) == math(c), (name, c)
                exact += 1
        # only the wrap class may hold wrapped pre-multiples
        assert (exact == len(cases)) or name == "wrap", name
        assert exact < len(cases) or name != "wrap", "the wrap class wraps nothing"


def test_mul_model_equals_oracle_and_mathematics():
    _products(R.cases_mul(), lambda c: R.fe_mul(*c), lambda c: _oracle.fe_mul(*c),
              lambda c: R.value(c[0]) * R.value(c[1]) % R.P, lambda c: R.mul_cols(*c)[1])


def test_sqn_model_equals_oracle_and_mathematics():
    for n in (1, 2):
        _products(R.cases_sq(n), lambda f: R.fe_sqn(f, n), lambda f: _oracle.fe_sqn(f, n),
                  lambda f: n * R.value(f) ** 2 % R.P, lambda f: R.sqn_cols(f, n)[1])


def test_mul_one_is_the_carry_chain():
    rng = random.Random(5)
    for f in R.edge_fes(R.CALLER) + R.edge_fes(R.WRAP) + [R.rand_fe(rng, R.CALLER) for _ in range(500)]:
        got = R.fe_mul_one(f)
        assert got == _oracle.fe_mul(f, R.FE_ONE) == _oracle.fe_mul(R.FE_ONE, f)
        assert R.value(got) == R.value(f)


def test_pow22523_model_equals_oracle_and_mathematics():
    for z in R.pow_inputs(103):
        got = R.fe_pow22523(z)
        assert got == _oracle.fe_pow22523(z), z
        assert R.value(got) == pow(R.value(z), 2**252 - 3, R.P)
    assert R.value(R.FE_SQRTM1) ** 2 % R.P == R.P - 1


def test_frombytes_and_predicates_model_equals_oracle():
    for s in R.frombytes_inputs(104):
        got = R.fe_frombytes(s)
        assert got == _oracle.fe_frombytes(s), s.hex()
        assert R.value(got) == (int.from_bytes(s, "little") & ((1 << 255) - 1)) % R.P
    n_in = 0
    for f in R.predicate_inputs(105):
        b = R.fe_tobytes(f)
        assert b == _oracle.fe_tobytes(f), f
        assert R.fe_isnonzero(f) == int(any(b)) and R.fe_isnegative(f) == (b[0] & 1)
        if all(abs(v) <= m for v, m in zip(f, R.SUM2)):   # the range the decompression feeds the predicates
            assert int.from_bytes(b, "little") == R.value(f), f
            n_in += 1
    assert n_in > 600


def test_group_steps_model_equals_oracle():
    p3s, p1s, qs = R.cases_points("p3"), R.cases_points("p1p1"), R.cases_points("cached")
    for k in range(300):
        X, Y, Z, _ = p3s[k]
        assert R.dbl(X, Y, Z) == _oracle.ge_dbl(X, Y, Z)
        assert R.p1p1_to_p3(p1s[k]) == _oracle.ge_p1p1_to_p3(p1s[k])
        assert R.p3_to_cached(p3s[k]) == _oracle.ge_to_cached(p3s[k])
        for neg in (0, 1):
            assert R.add_cached(p3s[k], qs[k], neg) == _oracle.ge_add(p3s[k], qs[k], neg)
    assert R.FE_D2 == _oracle.ge_to_cached(([0] * 10, [0] * 10, [0] * 10, R.FE_ONE))[3]


def test_sc_reduce_and_slide_on_the_directed_inputs():
    for x in R.sc_reduce_inputs(109):
        assert int.from_bytes(_oracle.sc_reduce(x.to_bytes(64, "little")), "little") == x % R.L, hex(x)
    most = 0
    for a in _slide.crafted_scalars():
        r = _slide.slide(a)
        assert r == _oracle.slide(a), hex(a)
        assert sum(d << i for i, d in enumerate(r)) == a
        most = max(most, sum(1 for d in r if d))
    assert most == 51          # the densest pattern found; the event plane holds 64


def test_operand_maxima(golden):
    """The largest |limb| the oracle's fe_mul / fe_sqn see at entry, over the
    golden set and one 4096-signature mixed stream (single-threaded), lies
    inside the bounds the input classes are built from (_fe_ref.CALLER for a
    product, SUM2 for a square).  Measured:
        fe_mul  even 100628189 (2.9990 x 2^25)   odd 50317840 (2.9992 x 2^24)
        fe_sqn  even  67099001 (0.9999 x 2^26)   odd 33544807 (0.9997 x 2^25)
    i.e. products see p1p1 mixes of three carried elements (CALLER =
    3 x 2^25 | 3 x (2^24 + 1)), squares X+Y of two (SUM2)."""
    from firedancer_amd import ed25519
    prv, blob, off, sz, fk, fp = _oracle.stream_inputs(31337, 4096, 0, 300, True)
    pub, sig = ed25519.sign_batch(prv, blob, off, sz, nthread=4)
    for i in np.nonzero(fk)[0]:
        byte, bit = divmod(int(fp[i]), 8)
        tgt = sig[i] if fk[i] == 1 else (blob[off[i]:] if fk[i] == 2 else pub[i])
        tgt[byte] ^= 1 << bit
    stream = _golden.Batch(pub, sig, off, sz, blob)

    def run():
        _oracle.verify_batch(golden, nthread=1)
        _oracle.verify_batch(stream, nthread=1)
    me, mo, se, so = _oracle.opmax_measure(run)
    print("operand maxima: fe_mul even %d odd %d, fe_sqn even %d odd %d" % (me, mo, se, so))
    assert 0 < me <= R.CALLER[0] and 0 < mo <= R.CALLER[3]
    assert 0 < se <= R.SUM2[0] and 0 < so <= R.SUM2[3]
    # and the classes reach what was measured: nothing real lies outside them
    assert me > R.SUM2[0] and se > R.CARRIED[0]


def test_sq_term_domain_edge():
    """fe_sq_fold2w / sq_term form exact column sums (no pre-multiple
    wraps), so they equal the reference's square only where the reference's
    own 38 f (limbs 5, 7, 9) and 19 f do not wrap either.  The domain the
    callers use -- even |limb| <= 2^26, odd <= 2^25 (X+Y of carried limbs),
    and the carried range for the sq2 operand -- is inside it; its edge is
    odd |limb| = floor((2^31 - 1) / 38), where the two part."""
    rng = random.Random(11)
    edge = ((1 << 31) - 1) // 38
    dom = [(1 << 26) if k % 2 == 0 else edge for k in range(10)]
    cases = R.edge_fes(dom) + R.edge_fes(R.SQ2W) + [R.rand_fe(rng, dom) for _ in range(2000)]
    for f in cases:
        assert R.sq_term_cols(f, False) == R.sqn_cols(f, 1)[0], f
    for f in R.edge_fes(R.SQ2W) + R.edge_fes(R.SQ2W_D2) + [R.rand_fe(rng, R.SQ2W) for _ in range(2000)]:
        assert R.sq_term_cols(f, True) == R.sqn_cols(f, 2)[0], f
    for d2 in (0, 1):        # the GPU probe's own inputs lie inside the domain
        for f in R.flat(R.cases_sq2w(d2))[0]:
            assert R.sq_term_cols(f, bool(d2)) == R.sqn_cols(f, 1 + d2)[0], f
            assert R.value(R.fe_sqn(f, 1 + d2)) == (1 + d2) * R.value(f) ** 2 % R.P
            assert R.fe_sqn(f, 1 + d2) == _oracle.fe_sqn(f, 1 + d2)
    for k in (5, 7, 9):      # one past the edge the reference's 38 f wraps and the limbs differ
        f = [3] * 10
        f[k] = edge + 1
        assert R.sq_term_cols(f, False) != R.sqn_cols(f, 1)[0]
        assert R.sqn_cols(f, 1)[1]
