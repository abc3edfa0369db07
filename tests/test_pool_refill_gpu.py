"""k_dsmp's slot refill, directed: a wave claims new signatures from the
shared counter into the pool slots that finished signatures have freed.

Under the launch policy a batch of n starts min(ceil(n / 64), 8 per CU)
waves and a wave's first claim takes FD_POOL_P = 112 signatures, so below
64 * 8 * CUs signatures no wave ever loads a signature into a slot that held
another one.  These tests set the wave count W through
debug_set_pool_waves, so that one to three waves work through a few hundred
signatures and every slot is reused, and check more than the verdict: the
R' = [s]B - [h]A each signature parked (debug_rprime_dev), all 30 limbs
against the oracle's, for every signature whose multiply ran -- the -3 ones
included, which a verdict test cannot tell from one that took another
signature's place.  Every case asserts its own premise by arithmetic on n,
W and the oracle's ran flags, so a change of policy cannot silently turn it
into a run without refill.
"""
import numpy as np
import pytest

import _golden
import _oracle
import _strict_ref

pytestmark = pytest.mark.gpu

P = 112   # FD_POOL_P: slots per wave, and the size of a wave's first claim


@pytest.fixture
def pooled():
    from firedancer_amd import ed25519
    ed25519.select_dsm_kernel("k_dsmp")
    yield
    ed25519.debug_set_pool_waves(0)
    ed25519.select_dsm_kernel("default")


def _mixed(seed, n):
    """n fresh signatures over 0..200-byte messages, 10 % with one bit of the
    signature, message or public key flipped."""
    from test_gpu_parity import _sign_stream
    return _sign_stream(seed, n, 0, 200, True)


def _run_twice(b, W, mode=None):
    """Two verify_dev calls on one workspace with k_dsmp on W waves, R' read
    back after each: [(verdicts, xyz [n][30])] * 2."""
    from firedancer_amd import ed25519, hip
    n = len(b)
    blob = np.concatenate([np.asarray(b.blob, np.uint8), np.zeros(16, np.uint8)])
    d = [hip.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in
         (b.pub, b.sig, np.asarray(b.msg_off, np.uint32), np.asarray(b.msg_sz, np.uint32), blob)]
    ws = hip.DeviceBuffer(ed25519.workspace_footprint(n))
    st = hip.Stream()
    out = []
    ed25519.debug_set_pool_waves(W)
    try:
        for _ in range(2):
            err = hip.DeviceBuffer.from_array(np.full(n, 0x55, np.int8))
            xyz = hip.DeviceBuffer.from_array(np.zeros(30 * n, np.int32))
            ed25519.verify_dev(n, *[x.ptr for x in d], err.ptr, ws.ptr, st.handle,
                               mode=ed25519.MODE_REFERENCE if mode is None else mode)
            ed25519.debug_rprime_dev(n, ws.ptr, "k_dsmp", xyz.ptr, st.handle)
            st.synchronize()
            out.append((err.to_array(np.int8, n), xyz.to_array(np.int32, 30 * n).reshape(30, n).T.copy()))
    finally:
        ed25519.debug_set_pool_waves(0)
    return out


def _check(b, W, want=None):
    """Verdicts (the oracle's, or `want`), R' limb for limb where the oracle's
    multiply ran, and a second run on the same workspace; returns the
    oracle's (err, ran)."""
    from firedancer_amd import ed25519
    oerr, ran, oxyz = _oracle.rprime_batch(b)
    runs = _run_twice(b, W, mode=None if want is None else ed25519.MODE_STRICT)
    exp = oerr if want is None else want
    for k, (err, xyz) in enumerate(runs):
        assert not (err == ed25519.VERDICT_DEVICE).any(), ("step guard", k)
        bad = np.nonzero(err != exp)[0]
        assert bad.size == 0, ("verdict", k, [(int(i), int(exp[i]), int(err[i])) for i in bad[:8]], int(bad.size))
        bad = np.nonzero(ran & (xyz != oxyz).any(axis=1))[0]
        assert bad.size == 0, ("R' limbs", k, [(int(i), int(oerr[i]), np.nonzero(xyz[i] != oxyz[i])[0][:4].tolist())
                                              for i in bad[:8]], int(bad.size))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1][ran], runs[1][1][ran])
    return oerr, ran


@pytest.mark.parametrize("n", [1, 112, 113, 127, 128, 129, 224, 225, 600])
def test_one_wave(pooled, n):
    """W = 1: the claim sequence is deterministic.  112 is exactly the first
    claim (the counter reaches n at once); 113 needs one refill that yields a
    single signature; 127..129 sit around the point where the refills after
    the first claim have covered 16 more; 224 / 225 are two whole pools and
    one more; at 600 every slot holds several generations."""
    b = _mixed(4100 + n, n)
    oerr, ran = _check(b, 1)
    loaded = int(ran.sum())                 # signatures that enter a pool slot
    if n <= P:
        assert loaded <= P                  # the first claim [0, P) takes them all: no refill loads anything
    elif n < 2 * P:
        assert ran[P:].all()                # 1 to 17 signatures past the first claim, each loaded by a refill
    else:
        assert loaded > P, (n, loaded)      # one wave, P slots: at least loaded - P entered a reused slot
        assert {0, -3} <= set(oerr[ran].tolist())      # R' of rejected signatures is checked too
    if n == 600:
        assert loaded - P >= 3 * P          # on average three or more later generations per slot


@pytest.mark.parametrize("W,n", [(2, 700), (3, 1000)])
def test_waves_race_on_the_counter(pooled, W, n):
    """Second and later claims of several waves interleave on the counter:
    which wave gets which signatures is not deterministic, every answer is."""
    b = _mixed(4200 + W, n)
    oerr, ran = _check(b, W)
    loaded = int(ran.sum())
    assert n > P * W and loaded > 2 * P * W, (loaded, W)   # loaded - P W signatures entered a reused slot: more than P W
    assert {0, -3} <= set(oerr[ran].tolist())


def test_waves_that_claim_nothing(pooled):
    """W = 8, n = 100: the first claim on the counter (112) passes n, so seven
    waves find nothing to take and must leave without touching a slab or
    raising the guard flag."""
    W, n = 8, 100
    assert n <= P and W > 1
    _check(_mixed(4300, n), W)


# ---- inactive signatures: decided before the multiply, they leave their slot free ----------

INACTIVE = ("s_range", "s_window", "offcurve_a", "offcurve_r")   # -1, 0 without a DSM (k_prep); -2, -2 (k_ai)
ACTIVE = ("valid", "flip_msg", "random", "mainnet", "false_reject")

_ref = {}


def _pick(golden, classes, ran, want):
    return [i for i in range(len(golden)) if _golden.CLASSES[golden.cls[i]] in classes and bool(ran[i]) == want]


def _pools(golden):
    """(inactive, active): golden indices, the four inactive kinds
    interleaved; the oracle's flag decides membership."""
    if "pools" not in _ref:
        _, ran, _ = _oracle.rprime_batch(golden)
        per = [_pick(golden, (c,), ran, False) for c in INACTIVE]
        assert all(len(p) >= 4 for p in per), [len(p) for p in per]
        m = max(len(p) for p in per)
        inactive = [p[k % len(p)] for k in range(m) for p in per]
        active = _pick(golden, ACTIVE, ran, True)
        assert len(active) >= 300
        _ref["pools"] = (inactive, active)
    return _ref["pools"]


def _layout(golden, pattern):
    """A batch of golden vectors: pattern is a list of booleans, True = the
    next active vector, False = the next inactive one (cycling)."""
    inactive, active = _pools(golden)
    ia = ii = 0
    sel = []
    for a in pattern:
        if a:
            sel.append(active[ia % len(active)])
            ia += 1
        else:
            sel.append(inactive[ii % len(inactive)])
            ii += 1
    sel = np.asarray(sel)
    b = _golden.Batch(golden.pub[sel].copy(), golden.sig[sel].copy(), golden.msg_off[sel].copy(),
                      golden.msg_sz[sel].copy(), golden.blob)
    return b, sel


def test_first_claim_all_inactive(golden, pooled):
    """112 inactive signatures, then 40 valid ones: the wave's first claim
    loads nothing while the counter has not reached n, so it must claim again
    (the empty-pool `continue`)."""
    pat = [False] * P + [True] * 40
    b, sel = _layout(golden, pat)
    oerr, ran = _check(b, 1)
    assert np.array_equal(ran, np.asarray(pat)) and len(b) > P
    assert np.array_equal(oerr, golden.expect[sel]) and {-1, -2, 0} <= set(oerr[:P].tolist())


def test_empty_claim_with_live_slots(golden, pooled):
    """16 valid, 230 inactive, 16 valid: the first claim [0, 112) loads 16
    slots; with 96 slots free the next claim [112, 208) follows at once and
    comes back empty while those 16 are mid-stream; the third crosses n."""
    pat = [True] * 16 + [False] * 230 + [True] * 16
    b, sel = _layout(golden, pat)
    oerr, ran = _check(b, 1)
    assert np.array_equal(ran, np.asarray(pat))
    assert ran[:16].all() and not ran[P:P + (P - 16)].any() and P + (P - 16) < len(b)
    assert np.array_equal(oerr, golden.expect[sel])


def test_refills_with_holes(golden, pooled):
    """Blocks of 7 inactive / 9 active over 500 signatures: a claim of ten or
    more signatures always spans inactive ones, so the claimed indices and
    the slots they land in run out of step (a free slot stays free)."""
    pat = [(i % 16) >= 7 for i in range(500)]
    b, sel = _layout(golden, pat)
    oerr, ran = _check(b, 1)
    assert np.array_equal(ran, np.asarray(pat))
    assert int(ran.sum()) > 2 * P           # 281 loads into 112 slots
    assert np.array_equal(oerr, golden.expect[sel])


def test_nothing_to_load(engine, golden, pooled):
    """300 inactive signatures: no slot is ever filled; the wave claims until
    the counter passes n and leaves.  No verdict is the step guard's marker,
    and the host call returns verdicts (OK), not FD_ED25519_AMD_ERR_DEVICE."""
    from firedancer_amd import ed25519
    b, sel = _layout(golden, [False] * 300)
    oerr, ran = _check(b, 1)
    assert not ran.any() and set(oerr.tolist()) == {-1, -2, 0}
    ed25519.debug_set_pool_waves(1)
    err = engine.verify_soa(b.pub, b.sig, b.msg_off, b.msg_sz, b.blob)
    assert np.array_equal(err, golden.expect[sel])


def test_strict_reads_reused_slots(pooled):
    """Strict mode, W = 1, n = 300 mixed: k_strict's pool_load_parked reads
    the slabs of signatures that went through reused slots; the verdicts are
    the independent Python verifier's."""
    n = 300
    b = _mixed(4400, n)
    want = np.array(_strict_ref.verify_batch(b), np.int8)
    oerr, ran = _check(b, 1, want=want)
    assert int(ran.sum()) > P + 100
    assert {0, -3} <= set(want.tolist()) and (want[oerr == -1] == -1).all() and (want[oerr == -2] == -2).all()
