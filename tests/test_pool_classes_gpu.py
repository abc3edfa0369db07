"""k_dsmp's step classes: DBL steps (no event pop), ADD-only steps (a mixed
step whose selection holds no DBL slot, with and without dead lanes) and
mixed steps, at batch shapes that force each of them.

Every test forces the pooled kernel, whatever the batch size, and checks
verdict equality with the CPU oracle.  A valid signature is the sensitive
input: k_fin's limb compare turns any wrong limb of its final point into -3.
"""
import numpy as np
import pytest

import _golden
import _oracle
import _slide

pytestmark = pytest.mark.gpu


@pytest.fixture
def pooled():
    from firedancer_amd import ed25519
    ed25519.select_dsm_kernel("k_dsmp")
    yield
    ed25519.select_dsm_kernel("default")


def _valid(golden, count):
    """Indices of the first `count` golden vectors of class "valid" that verify."""
    idx = [i for i in range(len(golden))
           if golden.cls[i] == _golden.CLASSES.index("valid") and golden.expect[i] == 0 and golden.msg_sz[i] > 0]
    assert len(idx) >= count
    return idx[:count]


def _replicated(golden, idx, n, flip=False, s_of=None):
    """n signatures that cycle through the golden vectors `idx`; flip: one
    message bit of each flipped; s_of: the scalar s replaced."""
    msgs = [bytearray(golden.msg(i)) for i in idx]
    if flip:
        for m in msgs:
            m[0] ^= 1
    offs = np.cumsum([0] + [len(m) for m in msgs])
    blob = np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\0" * 16, np.uint8).copy()
    which = np.arange(n) % len(idx)
    sel = np.asarray(idx)[which]
    sig = golden.sig[sel].copy()
    if s_of is not None:
        sig[:, 32:] = np.frombuffer(s_of.to_bytes(32, "little"), np.uint8)
    return _golden.Batch(golden.pub[sel].copy(), sig, offs[which].astype(np.uint32),
                         golden.msg_sz[sel].copy(), blob)


def _verify(engine, b):
    return engine.verify_soa(b.pub, b.sig, b.msg_off, b.msg_sz, b.blob)


@pytest.mark.parametrize("n", [64, 65, 111, 112, 113, 128])
def test_lockstep_pools(engine, golden, pooled, n):
    """One valid signature n times: the slots of a pool move in lockstep, so
    every step is a DBL step or an ADD-only step, full with 64 slots or more
    and with dead lanes below (at 128 the second wave holds 16 slots; at 65
    and 113 a wave holds one).  Around the 64-lane step width and the pool
    size of 112."""
    i = _valid(golden, 1)
    assert np.array_equal(_verify(engine, _replicated(golden, i, n)), np.zeros(n, np.int8)), n
    assert np.array_equal(_verify(engine, _replicated(golden, i, n, flip=True)), np.full(n, -3, np.int8)), n


def test_two_interleaved_signatures(engine, golden, pooled):
    """Two signatures alternating, 224 in all: their op streams differ, so
    the pool's classes split and one wave runs DBL, ADD-only and mixed
    steps."""
    b = _replicated(golden, _valid(golden, 2), 224)
    err = _verify(engine, b)
    assert np.array_equal(err, _oracle.verify_batch(b))
    assert np.array_equal(err, np.zeros(224, np.int8))


def test_seeded_random(engine, pooled):
    """4096 fresh signatures over 32-byte messages, a message bit flipped in
    every 16th: every verdict equals the oracle's, and the rejections among
    the untouched ones are the oracle's own limb-compare false rejects."""
    from firedancer_amd import workload
    n = 4096
    pub, sig, off, sz, blob = workload.sig_batch(n, 32, 7001)
    blob = blob.copy()
    flipped = np.arange(n) % 16 == 5
    for i in np.nonzero(flipped)[0]:
        blob[int(off[i]) + (int(i) % 32)] ^= 1 << (int(i) % 8)
    b = _golden.Batch(pub, sig, off, sz, blob)
    err = _verify(engine, b)
    exp = _oracle.verify_batch(b)
    assert np.array_equal(err, exp), np.nonzero(err != exp)[0][:10]
    assert np.all(exp[flipped] == -3)
    assert int((err[~flipped] == -3).sum()) == int((exp[~flipped] == -3).sum())


@pytest.mark.parametrize("s", [0, 1, 2, 1 << 2, 1 << 5, 1 << 252, _slide.L - 1],
                         ids=["0", "1", "2", "2^2", "2^5", "2^252", "L-1"])
def test_crafted_s(engine, golden, pooled, s):
    """128 copies of a golden R, A and message under a crafted s (all below
    L): no s event at all; a single event at position 0, after the last
    doubling; one at position 1; single events higher up; the densest stream.
    The verdict is the oracle's (0 or -3)."""
    b = _replicated(golden, _valid(golden, 1), 128, s_of=s)
    err = _verify(engine, b)
    exp = _oracle.verify_batch(b)
    assert set(int(v) for v in exp) <= {0, -3}
    assert np.array_equal(err, exp), (hex(s), err[:4], exp[:4])


def test_goldens_one_batch(engine, golden, pooled):
    """Every golden vector class in one batch through k_dsmp."""
    assert np.array_equal(_verify(engine, golden), golden.expect)
