"""CPU: the strict-mode checker (tests/_strict_ref.py) over the committed
golden vectors.  The table of (class, reference code -> strict code) counts
is the contract the GPU tests of strict mode (test_strict_gpu.py) rest on."""
import collections

import numpy as np

import _golden
import _strict_ref

# class -> {(reference code, strict code): count}
TABLE = {
    "valid": {(0, 0): 845},
    "rfc8032": {(0, 0): 3},
    "mainnet": {(0, 0): 6},
    "zero_msg": {(0, 0): 16},
    "max_msg": {(0, 0): 8, (-3, -3): 8},
    "false_reject": {(-3, 0): 156},
    "s_window": {(0, -1): 32},
    "malleate": {(-1, -1): 92, (0, -1): 4},
    "s_range": {(-1, -1): 24, (-3, -3): 8},
    "small_order": {(0, -2): 83, (-3, -2): 365},
    "noncanon": {(0, -2): 23, (-3, -2): 97},
    "offcurve_a": {(-2, -2): 16},
    "offcurve_r": {(-2, -2): 16},
    "flip_sig": {(-3, -3): 14, (-2, -2): 2},
    "flip_msg": {(-3, -3): 37},
    "flip_pub": {(-3, -3): 14, (-2, -2): 17},
    "random": {(-3, -3): 52, (-2, -2): 108},
}


def test_strict_verdicts_of_the_golden_vectors(golden):
    assert len(golden) == 2046
    strict = np.array(_strict_ref.verify_batch(golden), np.int8)
    got = collections.defaultdict(collections.Counter)
    for c, r, s in zip(golden.cls.tolist(), golden.expect.tolist(), strict.tolist()):
        got[_golden.CLASSES[c]][(r, s)] += 1
    assert {k: dict(v) for k, v in got.items()} == TABLE
    hist = collections.Counter(strict.tolist())
    assert (hist[0], hist[-1], hist[-2], hist[-3]) == (1034, 152, 727, 133)
    assert int((strict != golden.expect).sum()) == 760
    # the strict rule only ever tightens an s or a point rejection
    assert (strict[golden.expect == -1] == -1).all()
    assert (strict[golden.expect == -2] == -2).all()


def test_strict_rule_on_hand_made_cases(golden):
    """The rule's order and its edges, on inputs small enough to read."""
    v = _strict_ref
    i0 = int(np.nonzero(golden.cls == _golden.CLASSES.index("rfc8032"))[0][0])
    msg, sig, pub = golden.msg(i0), bytes(golden.sig[i0]), bytes(golden.pub[i0])
    assert v.verify(msg, sig, pub) == 0
    s = int.from_bytes(sig[32:], "little")
    assert v.verify(msg, sig[:32] + (s + v.L).to_bytes(32, "little"), pub) == -1          # malleated s
    assert v.verify(msg, sig[:32] + v.L.to_bytes(32, "little"), pub) == -1                # s = L exactly
    ident = (1).to_bytes(32, "little")
    zero_s = bytes(32)
    assert v.verify(b"anything", ident + zero_s, ident) == -2                             # A = R = identity, s = 0
    assert v.verify(msg, sig, (v.P + 1).to_bytes(32, "little")) == -2                     # y = p + 1: non-canonical
    assert v.verify(msg, sig, (1 | 1 << 255).to_bytes(32, "little")) == -2                # "-0": x = 0, sign set
    assert v.verify(msg, ident + (s + v.L).to_bytes(32, "little"), ident) == -1           # s is checked first
    assert v.verify(msg + b"x", sig, pub) == -3
