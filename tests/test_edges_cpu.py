"""CPU: the directed edge corpus (tests/_edges.py) is deterministic, is what
its vector names say (checked with big integers), and its verdicts under the
compiled reference, the clean-room oracle and the strict checker are pinned.
The table of (class, reference code, strict code) counts is the contract the
GPU tests of the corpus (test_edges_gpu.py, test_tile_strict_gpu.py) rest on."""
import collections

import numpy as np
import pytest

import _edges as E
import _oracle
import _strict_ref as S

SHA256 = "caa0ed5f466fc62231438c5b88e90920f3bf57fb6691861945d007b377f2bf80"

# class -> {(reference code, strict code): count}
TABLE = {
    "valid": {(0, 0): 1},
    "r_negx": {(-3, -3): 1},
    "r_negy": {(-3, -3): 1},
    "a_negx": {(-3, -3): 1},
    "mix_a": {(0, 0): 7, (-3, -3): 7},
    "mix_r": {(-3, -3): 7},
    "mix_ra": {(0, 0): 7},
    "nc_a": {(-3, -2): 24, (-2, -2): 14},
    "nc_r": {(-3, -2): 24, (-2, -2): 14},
    "near_a": {(-2, -2): 12, (-3, -3): 16},
    "near_r": {(-2, -2): 12, (-3, -3): 16},
    "on_table": {(0, 0): 9, (0, -2): 3},
    "s_plus_kL": {(0, -1): 1, (-1, -1): 14},      # s0 + L happens to fall in the reference's accept window
    "s_abs": {(-3, -3): 7, (-1, -1): 7, (0, -1): 1},
    "s_eq_L": {(-1, -1): 4},                      # s = L over a torsion or non-canonical A or R: the s check answers first
    "tor_pair": {(0, -2): 11, (-3, -2): 53},      # R = -[h]A as points, h hashed from R: 0 to 3 of the 8 R per A
}


def _cls(names, i):
    return names[i].split("/")[0]


def _index(names):
    return {n: i for i, n in enumerate(names)}


def test_corpus_is_deterministic_and_pinned():
    names, b = E.corpus()
    names2, b2 = E.corpus(fresh=True)
    assert names == names2 and len(set(names)) == len(names) == len(b) == 274
    for x, y in ((b.pub, b2.pub), (b.sig, b2.sig), (b.msg_off, b2.msg_off), (b.msg_sz, b2.msg_sz), (b.blob, b2.blob), (b.cls, b2.cls)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert E.digest(b) == E.digest(b2) == SHA256
    assert {_cls(names, i) for i in range(len(b))} == set(E.CLASSES) == set(TABLE)
    assert [E.CLASSES[c] for c in b.cls.tolist()] == [_cls(names, i) for i in range(len(b))]


def test_oracle_equals_compiled_reference_on_the_corpus():
    if _oracle.ref() is None:
        pytest.skip("oracle/_ref/libfdref.so not built")
    names, b = E.corpus()
    o = _oracle.verify_batch(b)
    r = np.array([_oracle.ref_verify(b.msg(i), b.sig[i], b.pub[i]) for i in range(len(b))], np.int8)
    assert np.array_equal(o, r), [(names[i], int(r[i]), int(o[i])) for i in np.nonzero(o != r)[0][:8]]
    got = collections.defaultdict(collections.Counter)
    strict = S.verify_batch(b)
    for i in range(len(b)):
        got[_cls(names, i)][(int(r[i]), strict[i])] += 1
    assert {k: dict(v) for k, v in got.items()} == TABLE


def test_the_table_of_reference_and_strict_verdicts():
    """The oracle stands in for the reference (the test above holds the two
    equal where the compiled reference is present)."""
    names, b = E.corpus()
    ref = _oracle.verify_batch(b)
    strict = np.array(S.verify_batch(b), np.int8)
    got = collections.defaultdict(collections.Counter)
    for i in range(len(b)):
        got[_cls(names, i)][(int(ref[i]), int(strict[i]))] += 1
    assert {k: dict(v) for k, v in got.items()} == TABLE
    assert int((ref != strict).sum()) == 117
    assert (strict[ref == -1] == -1).all() and (strict[ref == -2] == -2).all()
    ix = _index(names)
    v = lambda n: (int(ref[ix[n]]), int(strict[ix[n]]))
    # the cells the corpus exists for, by name
    for k in range(1, 8):
        assert v("mix_a/T%d/accept" % k) == (0, 0) and v("mix_a/T%d/reject" % k) == (-3, -3)
    for label in ("B", "-B", "2B"):
        assert v("on_table/%s/R=identity" % label) == (0, -2)
    assert v("s_abs/8") == (0, -1) and v("s_abs/7") == (-1, -1)       # the bottom of the reference's window, and one below
    assert v("s_abs/2") == (-3, -3) and v("s_abs/3") == (-1, -1)       # L - 1 and L
    assert v("nc_a/p+18/1") == (-3, -2) and v("nc_r/p+18/0") == (-3, -2)
    # nc_*, near_*: -2 in reference mode exactly where the checker finds y off the curve
    for i, n in enumerate(names):
        c = _cls(names, i)
        if c in ("nc_a", "nc_r", "near_a", "near_r"):
            enc = bytes(b.pub[i]) if c.endswith("_a") else bytes(b.sig[i][:32])
            y = int.from_bytes(enc, "little") & ((1 << 255) - 1)
            on = S.decode((y % S.P).to_bytes(32, "little")) is not None
            assert (ref[i] == -2) == (not on), n
            assert strict[i] == (-2 if not on or y >= S.P else -3), n


def test_near_values_are_canonical_near_misses():
    ys, y8 = E.near_ys(), E.y8()
    assert len(ys) == len(set(ys)) == 14 and all(1 < y < S.P - 1 and y not in (y8, S.P - y8) for y in ys)
    tors_y = {E.affine(t)[1] for t in E.torsion()}
    assert tors_y == {0, 1, S.P - 1, y8, S.P - y8}
    for y in ys:                                   # one unit or one bit from a constant strict mode compares against
        assert any(abs(y - c) == 1 or bin(y ^ c).count("1") == 1 for c in tors_y | {2, S.P - 2}), y


def test_half_right_rprime_constructions():
    names, b = E.corpus()
    ix = _index(names)
    i = ix["valid/baseline"]
    R = S.decode(bytes(b.sig[i][:32]))
    assert E.same_point(E.rprime(b.msg(i), bytes(b.sig[i]), bytes(b.pub[i])), R)
    for name, flip in (("r_negx/-R", (-1, 1)), ("r_negy/(x,-y)", (1, -1))):
        i = ix[name]
        msg, sig, pub = b.msg(i), bytes(b.sig[i]), bytes(b.pub[i])
        Re = S.decode(sig[:32])
        x, y = E.affine(Re)
        assert x != 0 and y != 0
        rx, ry = E.affine(E.rprime(msg, sig, pub))
        assert (rx, ry) == (flip[0] * x % S.P, flip[1] * y % S.P), name     # one coordinate equal, the other negated
    i = ix["a_negx/-A"]
    A, A0 = S.decode(bytes(b.pub[i])), S.decode(bytes(b.pub[ix["valid/baseline"]]))
    assert E.same_point(A, E.neg(A0)) and E.affine(A)[0] != 0


def test_mixed_order_constructions():
    names, b = E.corpus()
    ix = _index(names)
    tors = E.torsion()
    Apure, Rpure = S.mul(E.KEY_A, S.B), S.mul(E.NONCE_R, S.B)
    assert E.torsion_part(Apure) == 0 and E.torsion_part(Rpure) == 0 and E.torsion_part(S.add(Apure, tors[3])) == 3
    for k in range(1, 8):
        for what in ("accept", "reject"):
            i = ix["mix_a/T%d/%s" % (k, what)]
            msg, sig, pub = b.msg(i), bytes(b.sig[i]), bytes(b.pub[i])
            A, R = S.decode(pub), S.decode(sig[:32])
            assert E.same_point(A, S.add(Apure, tors[k])) and E.torsion_part(A) == k and E.torsion_part(R) == 0
            hT = S.mul(E.hram(sig[:32], pub, msg), tors[k])
            assert S.is_identity(hT) == (what == "accept")
            assert E.same_point(E.rprime(msg, sig, pub), S.add(Rpure, E.neg(hT)))
        i = ix["mix_r/T%d" % k]
        msg, sig, pub = b.msg(i), bytes(b.sig[i]), bytes(b.pub[i])
        assert E.torsion_part(S.decode(pub)) == 0 and E.torsion_part(S.decode(sig[:32])) == k
        assert E.same_point(E.rprime(msg, sig, pub), Rpure)                # R' is the pure part: R - R' = T
        i = ix["mix_ra/T%d" % k]
        msg, sig, pub = b.msg(i), bytes(b.sig[i]), bytes(b.pub[i])
        A, R = S.decode(pub), S.decode(sig[:32])
        h = E.hram(sig[:32], pub, msg)
        kr = E.torsion_part(R)
        assert E.torsion_part(A) == k and kr not in (0, None) and h % 8 != 0
        assert E.same_point(tors[kr], E.neg(S.mul(h, tors[k])))            # T_R = -[h]T_A
        assert E.same_point(E.rprime(msg, sig, pub), R)


def test_on_table_constructions():
    names, b = E.corpus()
    ix = _index(names)
    for label, a in (("B", 1), ("-B", S.L - 1), ("2B", 2)):
        Aw = S.mul(a, S.B)
        for what in ("honest", "R=identity", "R=B", "R=A"):
            i = ix["on_table/%s/%s" % (label, what)]
            msg, sig, pub = b.msg(i), bytes(b.sig[i]), bytes(b.pub[i])
            A, R = S.decode(pub), S.decode(sig[:32])
            assert E.same_point(A, Aw) and (label != "-B" or E.same_point(A, E.neg(S.B)))
            Rp = E.rprime(msg, sig, pub)
            assert E.same_point(Rp, R)
            if what == "R=identity":
                assert S.is_identity(Rp) and S.is_identity(R) and sig[:32] == (1).to_bytes(32, "little")
                s, h = int.from_bytes(sig[32:], "little"), E.hram(sig[:32], pub, msg)
                assert s == h * a % S.L                                     # [s]B and [h]A cancel
            if what == "R=B":
                assert E.same_point(R, S.B)
            if what == "R=A":
                assert sig[:32] == pub


def test_scalar_and_torsion_classes():
    names, b = E.corpus()
    ix = _index(names)
    s0 = int.from_bytes(bytes(b.sig[ix["valid/baseline"]][32:]), "little")
    assert s0 < S.L
    ks = [int(n.split("/")[1]) for n in names if n.startswith("s_plus_kL/")]
    assert ks == list(range(1, 16)) and s0 + 15 * S.L < 1 << 256 <= s0 + 16 * S.L
    for k in ks:
        assert int.from_bytes(bytes(b.sig[ix["s_plus_kL/%d" % k]][32:]), "little") == s0 + k * S.L
    got = [int.from_bytes(bytes(b.sig[ix["s_abs/%d" % j]][32:]), "little") for j in range(15)]
    assert got == E.s_abs_values(s0) and len(set(got)) == 15
    pairs = {(bytes(b.pub[i]), bytes(b.sig[i][:32])) for i, n in enumerate(names) if n.startswith("tor_pair/")}
    for n in ("A=identity", "A=p+3", "R=T1", "R=p+3"):                     # s = L exactly, and A or R alone would be -2 in strict mode
        i = ix["s_eq_L/" + n]
        assert int.from_bytes(bytes(b.sig[i][32:]), "little") == S.L
        good = bytes(b.sig[ix["valid/baseline"]])
        assert S.verify(b.msg(i), bytes(b.sig[i][:32]) + good[32:], bytes(b.pub[i])) == -2
    encs = {E.encode(t) for t in E.torsion()}
    assert len(encs) == 8 and pairs == {(x, y) for x in encs for y in encs}
    for i, n in enumerate(names):
        if n.startswith("tor_pair/"):
            assert bytes(b.sig[i][32:]) == bytes(32)


# (reference code, strict code) of the edge signer, which is the transaction's: its other signers are honest
TXN_WANT = {"nc_a": (-3, -2), "mix_a_accept": (0, 0), "mix_a_reject": (-3, -3), "A=B,R=identity": (0, -2), "near_a": (-3, -3)}


def test_transaction_cases():
    import _txn
    cases = E.txn_cases()
    assert [n for n, _, _ in cases] == ["%s/%d" % (k, p) for k in E.TXN_KINDS for p in range(3)]
    pays = [p for _, p, _ in cases]
    terr, base, serr = _oracle.txn_verify_batch(*_txn.pack(pays))
    assert base.tolist() == list(range(0, 3 * len(pays) + 1, 3))
    for t, (name, p, pos) in enumerate(cases):
        assert p[0] == 3 and len(p) <= 1232
        m = 1 + 64 * 3
        a = m + (1 if p[m] & 0x80 else 0) + 4
        assert p[a - 1] < 0x80                                  # one-byte account count
        ref = [_oracle.verify(p[m:], p[1 + 64 * k:65 + 64 * k], p[a + 32 * k:a + 32 * k + 32]) for k in range(3)]
        strict = [S.verify(p[m:], p[1 + 64 * k:65 + 64 * k], p[a + 32 * k:a + 32 * k + 32]) for k in range(3)]
        want = TXN_WANT[name.split("/")[0]]
        assert ref == [want[0] if k == pos else 0 for k in range(3)], name
        assert strict == [want[1] if k == pos else 0 for k in range(3)], name
        assert serr[3 * t:3 * t + 3].tolist() == ref and int(terr[t]) == want[0], name
