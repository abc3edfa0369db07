"""GPU: strict RFC 8032 verdicts (FD_ED25519_AMD_MODE_STRICT) through every
entry point and every double-scalar-multiply kernel, against the independent
Python verifier tests/_strict_ref.py (whose verdicts on the golden vectors
test_strict_ref_cpu.py pins)."""
import numpy as np
import pytest

import _golden
import _oracle
import _strict_ref
import _txn

pytestmark = pytest.mark.gpu

KERNELS = ["k_dsm", "k_dsmp", "k_dsm4", "k_dsm8"]


@pytest.fixture(scope="module")
def strict_golden(golden):
    """The strict verdict of every golden vector, computed once."""
    s = np.array(_strict_ref.verify_batch(golden), np.int8)
    s.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(device=0, batch_max=1 << 15, blob_max=(1 << 15) * 512, mode=ed25519.MODE_STRICT)
    yield e
    e.close()


@pytest.fixture
def dsm_kernel(request):
    from firedancer_amd import ed25519
    ed25519.select_dsm_kernel(request.param)
    yield request.param
    ed25519.select_dsm_kernel("default")


def _soa(e, b):
    return e.verify_soa(b.pub, b.sig, b.msg_off, b.msg_sz, b.blob)


def _report(got, want, golden, idx=None):
    bad = np.nonzero(got != want)[0]
    return [(int(i if idx is None else idx[i]), _golden.CLASSES[golden.cls[i if idx is None else idx[i]]],
             int(want[i]), int(got[i])) for i in bad[:8]], bad.size


@pytest.mark.parametrize("dsm_kernel", KERNELS, indirect=True)
def test_golden_vectors_strict_then_reference(eng, golden, strict_golden, dsm_kernel):
    """Every golden vector (all 156 false rejects, the 36 s-window forgeries,
    every torsion and non-canonical point) through each kernel's parked-R'
    layout; then the same engine back in reference mode is bit-exact again."""
    from firedancer_amd import ed25519
    try:
        assert eng.mode == ed25519.MODE_STRICT
        err = _soa(eng, golden)
        assert np.array_equal(err, strict_golden), _report(err, strict_golden, golden)
        eng.set_mode(ed25519.MODE_REFERENCE)
        assert eng.mode == ed25519.MODE_REFERENCE
        err = _soa(eng, golden)
        assert np.array_equal(err, golden.expect), _report(err, golden.expect, golden)
    finally:
        eng.set_mode(ed25519.MODE_STRICT)


def _tail_order(n, changed, same):
    """n golden indices whose last partial wave (the lanes past the last
    multiple of 64) holds only vectors whose strict verdict differs from the
    reference's, spread over their classes."""
    tail_len = n - 64 * ((n - 1) // 64)
    tail = changed[::max(1, len(changed) // tail_len)][:tail_len]
    used = set(tail.tolist())
    head = [i for i in same.tolist() + changed.tolist() if i not in used][:n - tail_len]
    order = np.array(head + tail.tolist(), np.int64)
    assert order.size == n and len(set(order.tolist())) == n
    return order


@pytest.mark.parametrize("dsm_kernel", KERNELS, indirect=True)
def test_tail_lanes_device_path(golden, strict_golden, dsm_kernel):
    """verify_dev(mode=STRICT) at n = 1, 63, 65, 2046: the verdicts of a
    partial last wave, and nothing written past err[n)."""
    from firedancer_amd import ed25519, hip
    changed = np.nonzero(strict_golden != golden.expect)[0]
    same = np.nonzero(strict_golden == golden.expect)[0]
    st = hip.Stream()
    for n in (1, 63, 65, 2046):
        idx = _tail_order(n, changed, same)
        assert (strict_golden[idx[-1:]] != golden.expect[idx[-1:]]).all()
        bufs = [hip.DeviceBuffer.from_array(a) for a in (golden.pub[idx], golden.sig[idx], golden.msg_off[idx],
                                                          golden.msg_sz[idx], golden.blob)]
        pad = 256
        d_err = hip.DeviceBuffer.from_array(np.full(n + pad, 0x55, np.int8))
        d_ws = hip.DeviceBuffer(ed25519.workspace_footprint(n))
        ed25519.verify_dev(n, *[b.ptr for b in bufs], d_err.ptr, d_ws.ptr, st.handle, mode=ed25519.MODE_STRICT)
        st.synchronize()
        out = d_err.to_array(np.int8, n + pad)
        assert np.array_equal(out[:n], strict_golden[idx]), (n, _report(out[:n], strict_golden[idx], golden, idx))
        assert (out[n:] == 0x55).all(), n
        ed25519.verify_dev(n, *[b.ptr for b in bufs], d_err.ptr, d_ws.ptr, st.handle)   # default argument: reference
        st.synchronize()
        out = d_err.to_array(np.int8, n + pad)
        assert np.array_equal(out[:n], golden.expect[idx]) and (out[n:] == 0x55).all(), n


def test_two_engines_one_strict_one_reference(eng, golden, strict_golden):
    """Two engines on one device verify the same batch in alternation: the
    mode is the engine's, not the process's."""
    from firedancer_amd import ed25519
    ref = ed25519.Engine(device=0, batch_max=4096, blob_max=4096 * 1232)
    try:
        assert (ref.mode, eng.mode) == (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT)
        for _ in range(3):
            assert np.array_equal(_soa(eng, golden), strict_golden)
            assert np.array_equal(_soa(ref, golden), golden.expect)
        with pytest.raises(ed25519.EngineError):
            ref.set_mode(2)
        assert ref.mode == ed25519.MODE_REFERENCE
    finally:
        ref.close()


def test_registered_memory_in_place_and_dma(eng, golden, strict_golden):
    """verify_soa_registered in strict mode: the in-place latency path (the
    verdicts go straight to mapped host memory, written by k_strict and by no
    kernel before it), and the DMA path (a batch larger than the engine; the
    throughput kernel forced)."""
    from firedancer_amd import ed25519
    n = len(golden)
    r = ed25519.RegisteredPlanes(golden.pub, golden.sig, golden.msg_off, golden.msg_sz, golden.blob)
    small = ed25519.Engine(device=0, batch_max=1000, blob_max=1000 * 1232, mode=ed25519.MODE_STRICT)
    try:
        for _ in range(2):
            err = np.full(n, 0x55, np.int8)
            eng.verify_soa_registered(r[0], r[1], r[2], r[3], r[4], err=err)          # n <= batch_max: in place
            assert np.array_equal(err, strict_golden), _report(err, strict_golden, golden)
        err = small.verify_soa_registered(r[0], r[1], r[2], r[3], r[4])               # 3 chunks by DMA
        assert np.array_equal(err, strict_golden), _report(err, strict_golden, golden)
        ed25519.select_dsm_kernel("k_dsm")                                            # no latency path: DMA, k_dsm
        err = eng.verify_soa_registered(r[0], r[1], r[2], r[3], r[4])
        assert np.array_equal(err, strict_golden), _report(err, strict_golden, golden)
        eng.set_mode(ed25519.MODE_REFERENCE)
        ed25519.select_dsm_kernel("default")
        assert np.array_equal(eng.verify_soa_registered(r[0], r[1], r[2], r[3], r[4]), golden.expect)
    finally:
        ed25519.select_dsm_kernel("default")
        eng.set_mode(ed25519.MODE_STRICT)
        small.close()
        r.close()


def test_pointer_array_api_strict(eng, golden, strict_golden):
    idx = np.nonzero(strict_golden != golden.expect)[0][::6]
    err = eng.verify_batch([golden.msg(i) for i in idx], [golden.sig[i] for i in idx], [golden.pub[i] for i in idx])
    assert np.array_equal(err, strict_golden[idx])


def test_mixed_stream_both_modes(eng):
    """2^15 fresh signatures, 10 % corrupted, default kernel choice and
    k_dsmp: strict equals the Python verifier wherever the two modes differ
    and on a fixed sample of 256; everywhere a reference -1 / -2 stays."""
    from firedancer_amd import ed25519
    from test_gpu_parity import _sign_stream
    b = _sign_stream(90210, 1 << 15, 0, 400, True)
    sample = np.random.default_rng(7).choice(len(b), 256, replace=False)
    try:
        for kernel in ("default", "k_dsmp"):
            ed25519.select_dsm_kernel(kernel)
            eng.set_mode(ed25519.MODE_REFERENCE)
            ref = _soa(eng, b)
            eng.set_mode(ed25519.MODE_STRICT)
            strict = _soa(eng, b)
            assert set(np.unique(ref).tolist()) >= {0, -3} and set(np.unique(strict).tolist()) <= {0, -1, -2, -3}
            assert (strict[ref == -1] == -1).all() and (strict[ref == -2] == -2).all()
            differ = np.nonzero(ref != strict)[0]
            assert differ.size < 64                      # false rejects and chance torsion only
            idx = np.unique(np.concatenate([differ, sample]))
            want = np.array(_strict_ref.verify_batch(b, idx.tolist()), np.int8)
            assert np.array_equal(strict[idx], want), (kernel, idx[strict[idx] != want][:8])
    finally:
        ed25519.select_dsm_kernel("default")
        eng.set_mode(ed25519.MODE_STRICT)


# ---- transactions ----------------------------------------------------------------

def _sig_fields(p):
    """(nsig, message offset, offset of the first signer's public key) of a
    well-formed wire transaction (fd_txn.h: signatures, [0x80 | version],
    3 header bytes, compact-u16 account count, account addresses)."""
    n = p[0]
    m = 1 + 64 * n
    a = m + (1 if p[m] & 0x80 else 0) + 3
    a += 1 if p[a] < 0x80 else 2
    return n, m, a


def _strict_txn(p):
    """(transaction verdict, per-signature strict verdicts) by the rule:
    the first failing signature's code."""
    n, m, a = _sig_fields(p)
    s = [_strict_ref.verify(p[m:], p[1 + 64 * k:65 + 64 * k], p[a + 32 * k:a + 32 * k + 32]) for k in range(n)]
    return next((v for v in s if v), 0), s


def _txn_cases():
    fx = [bytes(f.payload) for f in _txn.load_fixtures()]
    assert [p[0] for p in fx] == [4, 1, 1]
    window = bytes(16) + bytes([0, 0, 0, 0, 1]) + bytes(10) + bytes([0x10])     # s[31] = 0x10, s[20] = 1
    assert len(window) == 32
    w = bytearray(fx[0])
    w[1 + 64 * 2 + 32:1 + 64 * 3] = window                                      # signer 2 of 4
    t = bytearray(fx[0])
    n, m, a = _sig_fields(fx[0])
    t[a:a + 32] = bytes(32)                                                     # first signer := (sqrt(-1), 0), order 4
    return fx + [bytes(w), bytes(t), fx[1][:len(fx[1]) - 7]], fx


def _check_txn_verdicts(terr, base, serr, pays, strict):
    from firedancer_amd import ed25519
    assert base.tolist() == [0, 4, 5, 6, 10, 14, 15]
    assert terr[:3].tolist() == [0, 0, 0] and serr[:6].tolist() == [0] * 6      # the fixtures, unmodified
    assert int(terr[5]) == ed25519.FD_TXN_AMD_ERR_PARSE and int(serr[14]) == ed25519.FD_TXN_AMD_ERR_PARSE
    eterr, ebase, eserr = _oracle.txn_verify_batch(*_txn.pack(pays))
    if not strict:
        assert np.array_equal(terr, eterr) and np.array_equal(serr, eserr)
        assert int(terr[3]) == 0 and serr[6:10].tolist() == [0, 0, 0, 0]         # the s window is accepted
        return
    assert int(terr[3]) == -1 and serr[6:10].tolist() == [0, 0, -1, 0]          # rejected, at that signature's index
    assert int(terr[4]) == -2 and int(serr[10]) == -2                           # torsion public key
    for t in range(5):
        want_t, want_s = _strict_txn(pays[t])
        assert int(terr[t]) == want_t and serr[base[t]:base[t + 1]].tolist() == want_s, t


def test_transactions_both_modes(eng):
    """The fixture transactions unmodified, with one signer's s in the
    reference's accept window, with the first signer replaced by a torsion
    point, and truncated: through verify_txns, the device-resident entry and
    a two-engine MultiEngine, in both modes."""
    from firedancer_amd import ed25519, hip, workload
    pays, _ = _txn_cases()
    blob, off, sz = _txn.pack(pays)
    try:
        for mode in (ed25519.MODE_STRICT, ed25519.MODE_REFERENCE):
            strict = mode == ed25519.MODE_STRICT
            eng.set_mode(mode)
            _check_txn_verdicts(*eng.verify_txns(blob, off, sz, want_sigs=True), pays, strict)
            # device-resident
            tbase, slots = ed25519.txn_slots(blob, off, sz)
            d = [hip.DeviceBuffer.from_array(a) for a in (blob, off, sz, tbase)]
            d_terr, d_serr = hip.DeviceBuffer(len(pays)), hip.DeviceBuffer(slots)
            d_ws = hip.DeviceBuffer(workload._bind().fd_ed25519_amd_txn_workspace_footprint(len(pays), slots))
            st = hip.Stream()
            ed25519.verify_txns_dev(len(pays), slots, *[b.ptr for b in d], d_terr.ptr, d_serr.ptr, d_ws.ptr, st.handle,
                                    mode=mode)
            st.synchronize()
            _check_txn_verdicts(d_terr.to_array(np.int8, len(pays)), tbase, d_serr.to_array(np.int8, slots), pays, strict)
            multi = ed25519.MultiEngine([0, 0], batch_max=64, blob_max=1 << 16, mode=mode)
            try:
                _check_txn_verdicts(*multi.verify_txns(blob, off, sz, want_sigs=True), pays, strict)
            finally:
                multi.close()
    finally:
        eng.set_mode(ed25519.MODE_STRICT)


def test_multi_engine_soa_strict(golden, strict_golden):
    from firedancer_amd import ed25519
    multi = ed25519.MultiEngine([0, 0], batch_max=2048, blob_max=2048 * 1232, mode=ed25519.MODE_STRICT)
    try:
        assert np.array_equal(_soa(multi, golden), strict_golden)
        multi.set_mode(ed25519.MODE_REFERENCE)
        assert np.array_equal(_soa(multi, golden), golden.expect)
    finally:
        multi.close()


def test_step_guard_marker_survives_strict_mode(golden):
    """k_dsmp's step guard, tripped through the debug cap, in strict mode:
    the batch call still fails with FD_ED25519_AMD_ERR_DEVICE and the device
    path still shows FD_ED25519_AMD_VERDICT_DEVICE in every verdict --
    k_strict leaves the marker alone and reads no unfinished slab."""
    from firedancer_amd import ed25519, hip
    e = ed25519.Engine(device=0, batch_max=4096, blob_max=4096 * 1232, mode=ed25519.MODE_STRICT)
    try:
        ed25519.select_dsm_kernel("k_dsmp")
        ed25519.debug_set_pool_iter_cap(10)
        with pytest.raises(ed25519.EngineError):
            _soa(e, golden)
        n = len(golden)
        bufs = [hip.DeviceBuffer.from_array(a) for a in (golden.pub, golden.sig, golden.msg_off, golden.msg_sz,
                                                          golden.blob)]
        d_err, d_ws = hip.DeviceBuffer(n), hip.DeviceBuffer(ed25519.workspace_footprint(n))
        st = hip.Stream()
        ed25519.verify_dev(n, *[b.ptr for b in bufs], d_err.ptr, d_ws.ptr, st.handle, mode=ed25519.MODE_STRICT)
        st.synchronize()
        assert (d_err.to_array(np.int8, n) == ed25519.VERDICT_DEVICE).all()
    finally:
        ed25519.debug_set_pool_iter_cap(0)
        ed25519.select_dsm_kernel("default")
        e.close()
