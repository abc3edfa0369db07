"""The product kernels' intermediates, read back from the workspace: the
decompression's limb planes (k_decomp on the throughput path, k_front on
the latency path) against the oracle's decompress2, limb for limb.  The
verdict shows a decompression only through -2 / not -2; a wrong limb in
-A.X, A.Y, -A.T, R.X or R.Y would otherwise surface only as a flipped
verdict downstream.

And stage 3's: the R' = [s]B - [h]A = (X, Y, Z) that each double-scalar-
multiply kernel parks in the signature's slab (debug_rprime_dev reads it
through the kernel's parking layout, the loaders strict mode uses), all 30
limbs against the oracle's dsm().  The verdict compares limbs 0..7 of X and
Y only, never Z, and says nothing about the R' of a signature that is -3
either way."""
import numpy as np
import pytest

import _fe_ref as R
import _golden
import _oracle

pytestmark = pytest.mark.gpu

_ref = {}


def _selection(golden):
    """Golden vectors that pass the s check (s < L), every offcurve_a,
    offcurve_r, small_order, noncanon and false_reject vector first; at most
    2046."""
    if "sel" not in _ref:
        s = [int.from_bytes(bytes(golden.sig[i][32:]), "little") for i in range(len(golden))]
        must = {_golden.CLASSES.index(c) for c in ("offcurve_a", "offcurve_r", "small_order", "noncanon", "false_reject")}
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


def _upload(b):
    """Device buffers (pub, sig, off, sz, blob) of a batch, the blob padded."""
    from firedancer_amd import hip
    blob = np.concatenate([np.asarray(b.blob, np.uint8), np.zeros(16, np.uint8)])
    return [hip.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in
            (b.pub, b.sig, np.asarray(b.msg_off, np.uint32), np.asarray(b.msg_sz, np.uint32), blob)]


def _verify_rprime(b, n, kinds):
    """One verify_dev over b's first n signatures (the kernel choice as set
    now), then the parked R' read through each layout of `kinds`: (verdicts,
    {kind: int32 [n][30]})."""
    from firedancer_amd import ed25519, hip
    d = _upload(b)
    err, ws = hip.DeviceBuffer(n), hip.DeviceBuffer(ed25519.workspace_footprint(n))
    xyz = {k: hip.DeviceBuffer.from_array(np.zeros(30 * n, np.int32)) for k in kinds}
    stream = hip.Stream()
    ed25519.verify_dev(n, *[x.ptr for x in d], err.ptr, ws.ptr, stream.handle)
    for k in kinds:
        ed25519.debug_rprime_dev(n, ws.ptr, k, xyz[k].ptr, stream.handle)
    stream.synchronize()
    return err.to_array(np.int8, n), {k: v.to_array(np.int32, 30 * n).reshape(30, n).T for k, v in xyz.items()}


def _rprime_selection(golden):
    """The _selection batch and the oracle's (verdicts, ran flags, R' limbs)."""
    if "rp" not in _ref:
        sel = np.asarray(_selection(golden)[0])
        b = _golden.Batch(golden.pub[sel], golden.sig[sel], golden.msg_off[sel], golden.msg_sz[sel], golden.blob)
        _ref["rp"] = (sel, b) + _oracle.rprime_batch(b)
    return _ref["rp"]


@pytest.mark.parametrize("kernel", ["k_dsm", "k_dsm4", "k_dsm8", "k_dsmp"])
def test_rprime_limbs_per_kernel(golden, kernel):
    """Each DSM kernel (k_dsmp on its policy grid) over the golden selection,
    every false_reject vector in it: wherever the oracle's multiply ran, the
    parked R' decodes to the oracle's X, Y and Z, all 30 limbs -- for accepted
    and for rejected signatures."""
    from firedancer_amd import ed25519
    sel, b, oerr, ran, oxyz = _rprime_selection(golden)
    n = len(sel)
    fr = golden.cls[sel] == _golden.CLASSES.index("false_reject")
    assert fr.sum() == (golden.cls == _golden.CLASSES.index("false_reject")).sum() >= 4 and n <= 2046
    assert np.array_equal(oerr, golden.expect[sel])
    assert ran.any() and ran[fr].all() and {0, -3} <= set(oerr[ran].tolist())
    ed25519.select_dsm_kernel(kernel)
    try:
        err, xyz = _verify_rprime(b, n, [kernel])
    finally:
        ed25519.select_dsm_kernel("default")
    assert np.array_equal(err, oerr)
    bad = np.nonzero(ran & (xyz[kernel] != oxyz).any(axis=1))[0]
    assert bad.size == 0, (kernel, int(bad.size), [(int(sel[j]), _golden.CLASSES[golden.cls[sel[j]]], int(oerr[j]),
                                                   np.nonzero(xyz[kernel][j] != oxyz[j])[0][:4].tolist()) for j in bad[:5]])


def _fresh(n):
    """n fresh valid signatures over 32-byte messages, and the oracle's
    (verdicts, ran, R' limbs); made once at the largest size and sliced."""
    if "fresh" not in _ref:
        from firedancer_amd import workload
        pub, sig, off, sz, blob = workload.sig_batch(16385, 32, 8801)
        b = _golden.Batch(pub, sig, off, sz, blob)
        _ref["fresh"] = (b,) + _oracle.rprime_batch(b)
    b, oerr, ran, oxyz = _ref["fresh"]
    return _golden.Batch(b.pub[:n], b.sig[:n], b.msg_off[:n], b.msg_sz[:n], b.blob), oerr[:n], ran[:n], oxyz[:n]


@pytest.mark.parametrize("n,kernel", [(8192, "k_dsm8"), (8193, "k_dsm4"), (16384, "k_dsm4"), (16385, "k_dsm")])
def test_rprime_default_resolution_at_thresholds(n, kernel):
    """The default policy on both sides of its two thresholds: the verdicts
    are the oracle's and debug_rprime_dev(kind="default") -- resolved by the
    function the launch itself uses -- decodes every R' limb for limb.  The
    layout of the kernel the policy is documented to choose at this size
    reads the same rows; across the k_dsm4 / k_dsm threshold the other
    kernel's layout does not, so a wrong resolution would show."""
    b, oerr, ran, oxyz = _fresh(n)
    assert ran.all() and set(oerr.tolist()) <= {0, -3}
    other = "k_dsm" if kernel != "k_dsm" else "k_dsm4"
    err, xyz = _verify_rprime(b, n, ["default", kernel, other])
    assert np.array_equal(err, oerr), np.nonzero(err != oerr)[0][:10]
    bad = np.nonzero((xyz["default"] != oxyz).any(axis=1))[0]
    assert bad.size == 0, (n, int(bad.size), bad[:5].tolist())
    assert np.array_equal(xyz[kernel], oxyz)
    assert (xyz[other] != oxyz).any(axis=1).all()
