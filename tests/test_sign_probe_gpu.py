"""The device functions of the GPU signer (firedancer_amd/csrc/
fd_ed25519_sign.h), each alone on directed inputs through the sign_* probe
kernels of tests/hip/fd_probe.hip, against plain integer arithmetic and the
independent RFC 8032 model (tests/_sign_ref.py).

fe_invert is compared as a field value (the reference signer has no function
to be limb-exact with) and its output limbs must lie in the carried range
its consumer fe_mul is proven for; everything else is compared word for
word.  Every check is equality; one launch per test."""
import random

import numpy as np
import pytest

import _fe_ref as R
import _probe
import _sign_ref as S

pytestmark = pytest.mark.gpu

P, L = S.P, S.L


def _canon(v):
    """Non-negative limbs of an integer 0 <= v < 2^255."""
    out = []
    for w in R.WID:
        out.append(v & ((1 << w) - 1))
        v >>= w
    assert v == 0
    return out


def _ival(f):
    return sum(v << e for v, e in zip(f, R.EXP))


def _words(x, n=8):
    return np.frombuffer(int(x).to_bytes(4 * n, "little"), "<u4").astype(np.int64)


def _u32(out):
    return out.view(np.uint32)


def _first_bad(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return bad


# ---- fe_invert ---------------------------------------------------------------------

def test_sign_fe_invert():
    rng = random.Random(201)
    cases = [R.limbs(0), R.limbs(1), R.limbs(2), R.limbs(P - 1)] + R.edge_fes(R.CARRIED)
    cases += [R.rand_carried(rng) for _ in range(256)]
    out = _probe.run("sign_fe_invert", np.array(cases, np.int64)).tolist()
    for k, (f, g) in enumerate(zip(cases, out)):
        v = R.value(f)
        assert R.value(g) == pow(v, P - 2, P), ("case", k, f, g)      # 0 -> 0
        assert all(abs(x) <= b for x, b in zip(g, R.CARRIED)), ("output limb outside the carried range", k, g)


# ---- fe_tobytes_w ------------------------------------------------------------------

def _tobytes_inputs():
    pl = _canon(P)
    named = {"0": _canon(0), "1": _canon(1), "19": _canon(19), "p-1": _canon(P - 1), "p": pl, "p+1": _canon(P + 1),
             "p+18": _canon(P + 18), "2p-1": R.fe_add(pl, _canon(P - 1)), "2p": R.fe_add(pl, pl),
             "2^255-1": _canon(2**255 - 1), "-1": R.fe_neg(_canon(1)), "-p": R.fe_neg(pl)}
    want_int = {"0": 0, "1": 1, "19": 19, "p-1": P - 1, "p": P, "p+1": P + 1, "p+18": P + 18, "2p-1": 2 * P - 1,
                "2p": 2 * P, "2^255-1": 2**255 - 1, "-1": -1, "-p": -P}
    cases, names = [], []
    for name, f in named.items():
        v = want_int[name]
        assert _ival(f) == v
        cases.append(f)
        names.append(name)
        # the same value mod p in limbs that are all <= 0 ...
        for w in ((-v) % P, (-v) % P + P):
            if w < 2**255:
                cases.append(R.fe_neg(_canon(w)))
                names.append(name + " (negative limbs)")
        # ... and around every limb at +- its carried bound (all +, all -, both alternations)
        for e in R.edge_fes(R.CARRIED)[:4]:
            cases.append(R.fe_add(e, R.limbs(v - _ival(e))))
            names.append(name + " (limbs at +-CARRIED)")
    # every limb at +- its bound, and each limb alone at its maximum / minimum: the sh == 0 limbs at bit
    # offsets 0 and 128, and limb 9, which must not spill past word 7
    edge = R.edge_fes(R.CARRIED)
    cases += edge
    names += ["edge_fes(CARRIED)[%d]" % k for k in range(len(edge))]
    for k in range(10):
        for x in ((1 << R.WID[k]) - 1, -((1 << R.WID[k]) - 1)):   # the widest canonical limb, and its negative
            f = [0] * 10
            f[k] = x
            cases.append(f)
            names.append("limb %d alone = %d" % (k, x))
    rng = random.Random(202)
    cases += [R.rand_carried(rng) for _ in range(256)]
    names += ["random carried"] * 256
    return cases, names


def test_sign_fe_tobytes():
    cases, names = _tobytes_inputs()
    want = np.array([_words(_ival(f) % P) for f in cases], np.int64).astype(np.uint32)
    assert not (want[:, 7] >> 31).any()
    # the limb model of the same canonicalisation agrees: every input is inside its domain
    for f, w, nm in zip(cases, want, names):
        assert R.fe_tobytes(f) == w.tobytes(), ("input outside fe_reduce's domain", nm)
    got = _u32(_probe.run("sign_fe_tobytes", np.array(cases, np.int64)))
    bad = _first_bad(got, want)
    assert bad.size == 0, ("%d of %d differ; first %d (%s): limbs %s got %s want %s"
                           % (bad.size, len(cases), bad[0], names[bad[0]], cases[bad[0]],
                              got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex()))


# ---- the signed radix-16 recoding and [s]B ---------------------------------------------

def _directed_scalars():
    """Scalars aimed at the recoding's carries and at every table entry: a
    single nibble d 16^i gives digit i = d (d < 8) or d - 16 with a carry
    into digit i + 1, so the 960 of them reach every BASE[j][k] (|digit| =
    k + 1), nibbles d and 16 - d with either sign; -8 comes from a nibble 8
    and +8 only from the top digit's absorbed carry (0x78...8).

    scalarmult_base_enc's contract is s < 2^255 (its callers pass a clamped
    a and r < L).  The nine scalars here at or above 2^255 (0x88...8 and
    d 16^63 for d >= 8) leave digit 63 above 8, where madd_base would index
    past the table: they are run through the recoding only, never through
    [s]B."""
    s = [0, 1, 8, 2**255 - 1, L - 1, L]
    s += [int("8" * 64, 16), int("7" + "8" * 63, 16), int("0" + "8" * 63, 16), int("7" * 64, 16), int("7" + "f" * 63, 16)]
    s += [d << (4 * i) for i in range(64) for d in range(1, 16)]
    s += [(7 << 252) | (8 << 248)]
    names = ["0", "1", "8", "2^255-1", "L-1", "L", "nibbles 8", "nibbles 8, top 7", "nibbles 8, top 0", "nibbles 7",
             "nibbles f, top 7"]
    names += ["%d*16^%d" % (d, i) for i in range(64) for d in range(1, 16)]
    names += ["7*16^63 + 8*16^62"]
    return s, names


def test_sign_recode():
    s, names = _directed_scalars()
    rng = random.Random(203)
    s += [rng.getrandbits(255) for _ in range(256)]
    names += ["random"] * 256
    out = _probe.run("sign_recode", np.array([_words(x) for x in s], np.int64))
    dig = np.ascontiguousarray(out).view(np.int8).reshape(len(s), 64).astype(np.int64)
    assert sum(x >= 2**255 for x in s) == 9
    for k, x in enumerate(s):
        e = dig[k].tolist()
        assert sum(d << (4 * i) for i, d in enumerate(e)) == x, ("digits do not recombine", names[k], hex(x), e)
        assert all(-8 <= d < 8 for d in e[:63]), ("digit below 63 out of [-8, 8)", names[k], e)
        if x < 2**255:     # the contract; above it the top digit is the top nibble plus its carry, up to 16
            assert -8 <= e[63] <= 8, ("top digit out of [-8, 8]", names[k], e)
        else:
            assert e[63] == (x >> 252) + (e[62] < 0), ("top digit", names[k], e)


@pytest.fixture(scope="module")
def smb_cases():
    s, names = _directed_scalars()
    keep = [k for k, x in enumerate(s) if x < 2**255]          # the contract: see _directed_scalars
    s, names = [s[k] for k in keep], [names[k] for k in keep]
    rng = random.Random(204)
    s += [L + 1] + [rng.getrandbits(255) for _ in range(64)]
    names += ["L+1"] + ["random"] * 64
    want = np.array([np.frombuffer(S.scalarmult_base_enc(x), "<u4") for x in s], np.uint32)
    return s, names, want


def test_sign_scalarmult_base(smb_cases):
    s, names, want = smb_cases
    ident, base = (1).to_bytes(32, "little"), (4 * pow(5, P - 2, P) % P).to_bytes(32, "little")
    at = {nm: k for k, nm in enumerate(names) if nm != "random"}
    assert want[at["0"]].tobytes() == ident and want[at["L"]].tobytes() == ident
    assert want[at["1"]].tobytes() == base and want[at["L+1"]].tobytes() == base
    got = _u32(_probe.run("sign_scalarmult_base", np.array([_words(x) for x in s], np.int64)))
    bad = _first_bad(got, want)
    assert bad.size == 0, ("%d of %d differ; first %d (s = %s = %s): got %s want %s"
                           % (bad.size, len(s), bad[0], names[bad[0]], hex(s[bad[0]]),
                              got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex()))


# ---- (r + k a) mod L -----------------------------------------------------------------

def test_sign_sc_muladd():
    rng = random.Random(205)
    edge = [0, 1, 2**252, L - 1]
    tri = [(k, a, r) for k in edge for a in edge for r in edge]
    tri += [(rng.randrange(L), rng.randrange(L), rng.randrange(L)) for _ in range(512)]
    ka = np.array([np.concatenate([_words(k), _words(a)]) for k, a, _ in tri], np.int64)
    r = np.array([_words(r) for _, _, r in tri], np.int64)
    want = np.array([_words(S.sc_muladd(k, a, r)) for k, a, r in tri], np.int64).astype(np.uint32)
    got = _u32(_probe.run("sign_sc_muladd", ka, r))
    bad = _first_bad(got, want)
    assert bad.size == 0, ("%d of %d differ; first %d: k, a, r = %s got %s want %s"
                           % (bad.size, len(tri), bad[0], [hex(x) for x in tri[bad[0]]],
                              got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex()))
