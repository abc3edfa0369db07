"""CPU tests of the oracle's R' export (oracle_ed25519_verify_rprime): the
double-scalar multiply's output R' = [s]B - [h]A = (X, Y, Z) that the GPU
read-back tests compare the device kernels with, limb for limb.

Pinned two ways on the golden vectors: the limbs reproduce the oracle's own
verdict through the reference's compare (limbs 0..7 of Z R.x against X and of
Z R.y against Y), and their value is the affine [s]B - [h]A computed with
Python integers (tests/_strict_ref.py's point arithmetic, which shares
nothing with the oracle).
"""
import hashlib

import numpy as np
import pytest

import _fe_ref as R
import _golden
import _oracle
import _strict_ref as S


@pytest.fixture(scope="module")
def rprime(golden):
    err, ran, xyz = _oracle.rprime_batch(golden, nthread=8)
    for a in (err, ran, xyz):
        a.setflags(write=False)
    return err, ran, xyz


def test_flag_and_verdict_consistency(golden, rprime):
    """The batch form's verdicts are oracle.verify's; the flag is clear
    exactly for s >= L (the s window lies above L), or an undecodable A or R;
    where it is set the reference's limb compare on (X, Y, Z) reproduces the
    verdict, 0 or -3 -- every false_reject vector among them."""
    err, ran, xyz = rprime
    n = len(golden)
    assert np.array_equal(err, golden.expect)
    fr = _golden.CLASSES.index("false_reject")
    seen = {0: 0, -3: 0}
    for i in range(n):
        msg, sig, pub = golden.msg(i), bytes(golden.sig[i]), bytes(golden.pub[i])
        s = int.from_bytes(sig[32:], "little")
        rc, _, Rd = _oracle.decompress2(pub, sig[:32])
        assert bool(ran[i]) == (s < R.L and rc == 0), (i, _golden.CLASSES[golden.cls[i]])
        if not ran[i]:
            assert int(err[i]) == (-2 if s < R.L else _oracle.verify(msg, sig, pub)) and int(err[i]) in (0, -1, -2)
            assert not xyz[i].any()
            continue
        X, Y, Z = (xyz[i, 10 * k:10 * k + 10].tolist() for k in range(3))
        xZ, yZ = _oracle.fe_mul(Z, Rd[0].tolist()), _oracle.fe_mul(Z, Rd[1].tolist())
        got = 0 if xZ[:8] == X[:8] and yZ[:8] == Y[:8] else -3
        assert got == int(err[i]) == _oracle.verify(msg, sig, pub), (i, _golden.CLASSES[golden.cls[i]])
        seen[got] += 1
        if golden.cls[i] == fr:
            assert got == -3
    assert ran[golden.cls == fr].all() and (golden.cls == fr).sum() >= 4
    assert seen[0] > 100 and seen[-3] > 100
    # the single-signature form gives the same rows
    for i in list(range(0, n, 97)) + np.nonzero(~ran)[0][:8].tolist():
        rc, r1, x1 = _oracle.rprime(golden.msg(i), golden.sig[i], golden.pub[i])
        assert rc == int(err[i]) and r1 == bool(ran[i]) and np.array_equal(x1.reshape(30), xyz[i])


def test_value_is_sB_minus_hA(golden, rprime):
    """On 16 vectors each of valid, flip_msg (-3), flip_sig and false_reject
    whose multiply ran: X/Z and Y/Z mod p equal the affine [s]B - [h]A in
    Python integers, and Z != 0."""
    err, ran, xyz = rprime
    picked = 0
    for cname in ("valid", "flip_msg", "flip_sig", "false_reject"):
        idx = [i for i in np.nonzero((golden.cls == _golden.CLASSES.index(cname)) & ran)[0]
               if S.decode(bytes(golden.pub[i])) is not None][:16]
        assert len(idx) >= 4, cname
        for i in idx:
            msg, sig, pub = golden.msg(i), bytes(golden.sig[i]), bytes(golden.pub[i])
            A = S.decode(pub)
            s = int.from_bytes(sig[32:], "little")
            h = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % S.L
            want = S.add(S.mul(s, S.B), S.mul(h, (S.P - A[0], A[1], 1, S.P - A[3])))
            zi = pow(want[2], S.P - 2, S.P)
            wx, wy = want[0] * zi % S.P, want[1] * zi % S.P
            X, Y, Z = (R.value(xyz[i, 10 * k:10 * k + 10].tolist()) % R.P for k in range(3))
            assert Z != 0, i
            gi = pow(Z, R.P - 2, R.P)
            assert (X * gi % R.P, Y * gi % R.P) == (wx, wy), (cname, int(i))
            picked += 1
    assert picked >= 36
