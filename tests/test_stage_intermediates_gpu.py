"""The product kernels' intermediates, read back from the workspace: the
decompression's limb planes (k_decomp on the throughput path, k_front on
the latency path) against the oracle's decompress2, limb for limb.  The
verdict shows a decompression only through -2 / not -2; a wrong limb in
-A.X, A.Y, -A.T, R.X or R.Y would otherwise surface only as a flipped
verdict downstream."""
import numpy as np
import pytest

import _fe_ref as R
import _golden
import _oracle

pytestmark = pytest.mark.gpu

_ref = {}


def _selection(golden):
    """Golden vectors that pass the s check (s < L), every offcurve_a,
    offcurve_r, small_order and noncanon vector first; at most 2046."""
    if "sel" not in _ref:
        s = [int.from_bytes(bytes(golden.sig[i][32:]), "little") for i in range(len(golden))]
        must = {_golden.CLASSES.index(c) for c in ("offcurve_a", "offcurve_r", "small_order", "noncanon")}
        ok = [i for i in range(len(golden)) if s[i] < R.L]
        first = [i for i in ok if int(golden.cls[i]) in must]
        sel = (first + [i for i in ok if int(golden.cls[i]) not in must])[:2046]
        for c in must:
            want = [i for i in ok if int(golden.cls[i]) == c]
            assert want and set(want) <= set(sel), _golden.CLASSES[c]
        # the reference, one point at a time (decompress2 stops at the first bad point of a pair)
        n = len(sel)
        A, Rr, ds = np.zeros((n, 30), np.int32), np.zeros((n, 20), np.int32), np.zeros((n, 2), np.uint8)
        for j, i in enumerate(sel):
            pub, r = bytes(golden.pub[i]), bytes(golden.sig[i][:32])
            rc, a, _ = _oracle.decompress2(pub, pub)
            ds[j, 0] = rc != 0
            A[j] = np.concatenate([(-a[0].astype(np.int64)).astype(np.int32), a[1], (-a[3].astype(np.int64)).astype(np.int32)])
            rc, b, _ = _oracle.decompress2(r, r)
            ds[j, 1] = rc != 0
            Rr[j] = np.concatenate([b[0], b[1]])
        _ref["sel"] = (sel, A, Rr, ds)
    return _ref["sel"]


@pytest.mark.parametrize("kernel", ["k_dsm", "k_dsm8"])
def test_decompression_planes(golden, kernel):
    """After one verify_dev: ds flags equal the oracle's per-point status,
    and where a point decoded its limbs equal decompress2's with A negated
    (user.c:406-407) -- through the gated k_decomp ("k_dsm") and the ungated
    k_front ("k_dsm8").  Also by value: x^2 (d y^2 + 1) == y^2 - 1 and
    T == x y (mod p)."""
    from firedancer_amd import ed25519, hip
    sel, eA, eR, eds = _selection(golden)
    n = len(sel)
    msgs = [golden.msg(i) for i in sel]
    off = np.cumsum([0] + [len(m) for m in msgs[:-1]]).astype(np.uint32)
    blob = np.frombuffer(b"".join(msgs) + b"\0" * 16, np.uint8)
    d = {k: hip.DeviceBuffer.from_array(v) for k, v in
         dict(pub=golden.pub[sel], sig=golden.sig[sel], off=off, sz=golden.msg_sz[sel], blob=blob).items()}
    err = hip.DeviceBuffer(n)
    ws = hip.DeviceBuffer(ed25519.workspace_footprint(n))
    dA, dR, dds = hip.DeviceBuffer(4 * 30 * n), hip.DeviceBuffer(4 * 20 * n), hip.DeviceBuffer(2 * n)
    stream = hip.Stream()
    ed25519.select_dsm_kernel(kernel)
    try:
        ed25519.verify_dev(n, d["pub"].ptr, d["sig"].ptr, d["off"].ptr, d["sz"].ptr, d["blob"].ptr, err.ptr, ws.ptr,
                           stream.handle)
        ed25519.debug_points_dev(n, ws.ptr, dA.ptr, dR.ptr, dds.ptr, stream.handle)
        stream.synchronize()
    finally:
        ed25519.select_dsm_kernel("default")
    assert np.array_equal(err.to_array(np.int8, n), golden.expect[sel])
    gA = dA.to_array(np.int32, 30 * n).reshape(30, n).T
    gR = dR.to_array(np.int32, 20 * n).reshape(20, n).T
    gds = dds.to_array(np.uint8, 2 * n).reshape(n, 2)
    assert np.array_equal(gds, eds), np.nonzero((gds != eds).any(axis=1))[0][:10]
    assert eds[:, 0].any() and eds[:, 1].any() and (eds == 0).all(axis=1).any()
    okA, okR = eds[:, 0] == 0, eds[:, 1] == 0
    badA = np.nonzero(okA & (gA != eA).any(axis=1))[0]
    badR = np.nonzero(okR & (gR != eR).any(axis=1))[0]
    assert badA.size == 0, ("A limbs", [(int(sel[j]), _golden.CLASSES[golden.cls[sel[j]]]) for j in badA[:5]])
    assert badR.size == 0, ("R limbs", [(int(sel[j]), _golden.CLASSES[golden.cls[sel[j]]]) for j in badR[:5]])
    dv = R.D
    for j in range(n):
        if okA[j]:
            x, y, t = (-R.value(gA[j, :10].tolist())) % R.P, R.value(gA[j, 10:20].tolist()), (-R.value(gA[j, 20:].tolist())) % R.P
            assert (x * x * (dv * y * y + 1) - (y * y - 1)) % R.P == 0 and (t - x * y) % R.P == 0, ("A value", int(sel[j]))
        if okR[j]:
            x, y = R.value(gR[j, :10].tolist()), R.value(gR[j, 10:].tolist())
            assert (x * x * (dv * y * y + 1) - (y * y - 1)) % R.P == 0, ("R value", int(sel[j]))
