"""Every device field-op variant and group step, limb for limb, against the
Python model of the reference's arithmetic (tests/_fe_ref.py, pinned to the
oracle and to the mathematics by tests/test_fe_ref_cpu.py), through the
probe kernels of tests/hip/fd_probe.hip.

Inputs are directed at where the variants can differ: random carried limbs,
every limb at +- its bound (one-hot pairs isolate each product term with its
x2 / x19 factor), the callers' measured maxima, column sums on the rounding
boundaries of the carry chain, and -- for the variants that claim the
reference's int32 wrap -- limbs up to 2^27.

Bar: every output limb equal (integer work, no tolerance)."""
import random

import numpy as np
import pytest

import _fe_ref as R
import _probe

pytestmark = pytest.mark.gpu

BIAS = np.array([(1 << 25) if k % 2 == 0 else (1 << 24) for k in range(10)], np.int64)


def _arr(cases):
    """[case] -> (n, ints) int64; a case is an element, or a tuple of elements / tuples."""
    def fl(c):
        return [int(v) for v in c] if isinstance(c[0], int) else [v for e in c for v in fl(e)]
    return np.array([fl(c) for c in cases], np.int64)


def _check(op, got, want, names=None, what=""):
    want = ((np.asarray(want, np.int64) & 0xffffffff).astype(np.uint32)).view(np.int32).reshape(got.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        k = int(bad[0])
        by_class = {}
        for b in bad:
            c = names[b] if names else "-"
            by_class[c] = by_class.get(c, 0) + 1
        limb = np.nonzero(got[k] != want[k])[0].tolist()
        raise AssertionError("%s%s: %d of %d cases differ, by class %s; first case %d (%s): limbs %s got %s want %s"
                             % (op, what, bad.size, len(got), by_class, k, names[k] if names else "-", limb,
                                got[k][limb].tolist(), want[k][limb].tolist()))


_memo = {}


def _mul_ref():
    if "mul" not in _memo:
        cases, names = R.flat(R.cases_mul())
        _memo["mul"] = (cases, names, _arr([R.fe_mul(f, g) for f, g in cases]))
    return _memo["mul"]


def _sq_ref(n):
    if ("sq", n) not in _memo:
        cases, names = R.flat(R.cases_sq(n))
        _memo["sq", n] = (cases, names, _arr([R.fe_sqn(f, n) for f in cases]))
    return _memo["sq", n]


@pytest.mark.parametrize("op", ["fe_mul", "fe_mul_fold1", "fe_mul_half5"])
def test_mul_variants(op):
    cases, names, want = _mul_ref()
    got = _probe.run(op, _arr([f for f, _ in cases]), _arr([g for _, g in cases]))
    if op == "fe_mul_half5":      # case k on lanes 8k..8k+7: every lane's joined element
        want = np.tile(want, (1, 8))
    _check(op, got, want, names)


@pytest.mark.parametrize("b1,b2", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_mul_fold2w(b1, b2):
    """Two products per case (the second runs through the list in reverse);
    a BIAS output is the limb plus its rounding offset."""
    cases, names, want = _mul_ref()
    n = len(cases)
    f, g = _arr([c[0] for c in cases]), _arr([c[1] for c in cases])
    got = _probe.run("fe_mul_fold2w_%d%d" % (b1, b2), np.hstack([f, f[::-1]]), np.hstack([g, g[::-1]]))
    w = np.hstack([want + b1 * BIAS, want[::-1] + b2 * BIAS])
    _check("fe_mul_fold2w", got, w, ["%s|%s" % (names[k], names[n - 1 - k]) for k in range(n)], " BIAS=%d%d" % (b1, b2))


def test_mul_one():
    rng = random.Random(5)
    cases = R.edge_fes(R.CALLER) + R.edge_fes(R.WRAP) + [R.rand_fe(rng, R.CALLER) for _ in range(500)]
    _check("fe_mul_one", _probe.run("fe_mul_one", _arr(cases)), _arr([R.fe_mul_one(f) for f in cases]))


@pytest.mark.parametrize("op,n", [("fe_sqn1", 1), ("fe_sq_fold", 1), ("fe_sqn2", 2)])
def test_sq_variants(op, n):
    cases, names, want = _sq_ref(n)
    _check(op, _probe.run(op, _arr(cases)), want, names)


@pytest.mark.parametrize("d2a,d2b", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_sq_fold2w(d2a, d2b):
    """Two squares per case, each slot fed its own callers' range (X+Y-like
    for a square, Z-like for the sq2 slot); exact by design, so no wrap
    class (tests/test_fe_ref_cpu.py::test_sq_term_domain_edge)."""
    ca, na = R.flat(R.cases_sq2w(d2a))
    cb, nb = R.flat(R.cases_sq2w(d2b))
    cb, nb = cb[::-1], nb[::-1]
    n = max(len(ca), len(cb))
    fa, fb = [ca[k % len(ca)] for k in range(n)], [cb[k % len(cb)] for k in range(n)]
    got = _probe.run("fe_sq_fold2w_%d%d" % (d2a, d2b), np.hstack([_arr(fa), _arr(fb)]))
    want = np.hstack([_arr([R.fe_sqn(f, 1 + d2a) for f in fa]), _arr([R.fe_sqn(f, 1 + d2b) for f in fb])])
    _check("fe_sq_fold2w", got, want, ["%s|%s" % (na[k % len(na)], nb[k % len(nb)]) for k in range(n)],
           " D2=%d%d" % (d2a, d2b))


def test_pow22523():
    cases = R.pow_inputs(103)
    _check("fe_pow22523", _probe.run("fe_pow22523", _arr(cases)), _arr([R.fe_pow22523(z) for z in cases]))


def test_frombytes():
    cases = R.frombytes_inputs(104)
    words = np.array([np.frombuffer(s, "<u4") for s in cases], np.int64)
    _check("fe_frombytes", _probe.run("fe_frombytes", words), _arr([R.fe_frombytes(s) for s in cases]))


def test_predicates():
    """fe_isnonzero / fe_isnegative on limb patterns whose value is 0, +-1,
    +-k mod p while the limbs are not (p, 2p, -p in limbs; differences of two
    carried elements): the -2 against 0 decision of the decompression."""
    cases = R.predicate_inputs(105)
    a = _arr(cases)
    _check("fe_isnonzero", _probe.run("fe_isnonzero", a), np.array([[R.fe_isnonzero(f)] for f in cases]))
    _check("fe_isnegative", _probe.run("fe_isnegative", a), np.array([[R.fe_isnegative(f)] for f in cases]))


def test_sc_reduce():
    xs = R.sc_reduce_inputs(109)
    words = np.array([np.frombuffer(x.to_bytes(64, "little"), "<u4") for x in xs], np.int64)
    want = np.array([np.frombuffer((x % R.L).to_bytes(32, "little"), "<u4") for x in xs], np.int64)
    _check("sc_reduce", _probe.run("sc_reduce", words), want)


# ---- group steps ---------------------------------------------------------------

def _points():
    if "pts" not in _memo:
        _memo["pts"] = (R.cases_points("p3"), R.cases_points("p1p1"), R.cases_points("cached"))
    return _memo["pts"]


def test_ge_dbl_and_to_cached():
    p3s, _, _ = _points()
    _check("ge_dbl", _probe.run("ge_dbl", _arr([u[:3] for u in p3s])), _arr([R.dbl(*u[:3]) for u in p3s]))
    _check("ge_to_cached", _probe.run("ge_to_cached", _arr(p3s)), _arr([R.p3_to_cached(u) for u in p3s]))


def _p3_ref():
    if "p3" not in _memo:
        _memo["p3"] = [R.p1p1_to_p3(t) for t in _points()[1]]
    return _memo["p3"]


@pytest.mark.parametrize("op", ["ge_p1p1_to_p3", "ge_p1p1_to_p3_fold"])
def test_ge_p1p1_to_p3(op):
    _check(op, _probe.run(op, _arr(_points()[1])), _arr(_p3_ref()))


@pytest.mark.parametrize("op", ["ge_add", "ge_madd"])
def test_ge_add(op):
    """ge_add<false> (table Z multiplied in) and ge_add<true> (Z = 1: the
    carry chain alone), neg = 0 and 1."""
    p3s, _, qs = _points()
    if op == "ge_madd":
        qs = [(R.FE_ONE,) + q[1:] for q in qs]
    neg = [k & 1 for k in range(len(p3s))] + [1 - (k & 1) for k in range(len(p3s))]
    u, q = p3s + p3s, qs + qs
    got = _probe.run(op, _arr(u), _arr(q), np.array(neg).reshape(-1, 1))
    _check(op, got, _arr([R.add_cached(u[k], q[k], neg[k]) for k in range(len(u))]),
           ["neg=%d" % v for v in neg])


def _body_cases():
    """(u, rows per lane, isD, neg, p1p1 out): the op body on a quad.  Lane q
    multiplies by its own table row: q0 qP, q1 qM (swapped when neg), q2 qZ,
    q3 qT; a DBL ignores the rows."""
    if "body" not in _memo:
        p3s, _, qs = _points()
        out = []
        for k, (u, q) in enumerate(zip(p3s, qs)):
            isD, neg = ((1, 0), (0, 0), (0, 1))[k % 3]
            rows = (q[1] if neg else q[2], q[2] if neg else q[1], q[0], q[3])
            t = R.dbl(*u[:3]) if isD else R.add_cached(u, q, neg)
            out.append((u, rows, isD, neg, t))
        _memo["body"] = out
    return _memo["body"]


def test_quad_p3_and_cached_row():
    p3s, p1s, _ = _points()
    got = _probe.run("quad_p3", _arr(p1s))
    _check("quad_p3", got, np.tile(_arr(_p3_ref()), (1, 4)))            # every lane ends with the full u
    _check("quad_cached_row", _probe.run("quad_cached_row", _arr(p3s)), _arr([R.p3_to_cached(u) for u in p3s]))


def test_quad_body():
    b = _body_cases()
    got = _probe.run("quad_body", _arr([c[0] for c in b]), _arr([c[1] for c in b]), np.array([[c[2], c[3]] for c in b]))
    _check("quad_body", got, np.tile(_arr([c[4] for c in b]), (1, 4)), ["isD=%d neg=%d" % (c[2], c[3]) for c in b])


def _ownc_cases():
    """Own-coordinate form: lane q holds C = (Z, T, X, Y)[q] of a p1p1 t;
    one step is u = p1p1_to_p3( t ) (lane products u.Z, u.Y, u.X, u.T), then
    the body on u, and the lane's coordinate of the new p1p1."""
    if "ownc" not in _memo:
        _, p1s, qs = _points()
        out = []
        for k, (t, q) in enumerate(zip(p1s, qs)):
            isD, neg = ((1, 0), (0, 0), (0, 1))[k % 3]
            u = _p3_ref()[k]
            rows = (q[1] if neg else q[2], q[2] if neg else q[1], q[0], q[3])
            t2 = R.dbl(*u[:3]) if isD else R.add_cached(u, q, neg)
            C = (t[2], t[3], t[0], t[1])
            pm = (u[2], u[1], u[0], u[3])
            C2 = (t2[2], t2[3], t2[0], t2[1])
            out.append((C, rows, isD, neg, pm, C2))
        _memo["ownc"] = out
    return _memo["ownc"]


@pytest.mark.parametrize("op", ["quad_ownc", "quad8_ownc5"])
def test_quad_ownc(op):
    """quad_p3_ownc + quad_body_ownc (fe_mul_fold1, lin2 / lin3, DPP
    quad_perm) and the 8-lane split form quad8_p3_ownc5 + quad8_body_ownc5
    (fe_mul_half5 / fe_join5), DBL and ADD+-."""
    c = _ownc_cases()
    got = _probe.run(op, _arr([x[0] for x in c]), _arr([x[1] for x in c]), np.array([[x[2], x[3]] for x in c]))
    pm, C2 = _arr([x[4] for x in c]), _arr([x[5] for x in c])
    want = np.hstack([pm, C2]) if op == "quad_ownc" else np.hstack([pm, pm, C2, C2])
    _check(op, got, want, ["isD=%d neg=%d" % (x[2], x[3]) for x in c])
