"""GPU: the directed edge corpus (tests/_edges.py; its verdict table is
pinned in test_edges_cpu.py) through every double-scalar-multiply kernel in
both verdict modes, and through the host entry points and the transaction
calls.  Reference-mode verdicts are the CPU oracle's, strict verdicts the
independent Python verifier's, tags hashlib's, R' and the decompression
planes the oracle's limb for limb: every comparison is an integer equality."""
import numpy as np
import pytest

import _edges as E
import _fe_ref as R
import _oracle
import _strict_ref
import _txn
from test_tags_gpu import _hashlib_tags

pytestmark = pytest.mark.gpu

KERNELS = ["k_dsm8", "k_dsm4", "k_dsm", "k_dsmp"]
RAN_CLASSES = ("mix_a", "mix_r", "mix_ra", "on_table", "nc_a", "nc_r", "near_a", "near_r")
P = 112   # FD_POOL_P: slots per k_dsmp wave

_ref = {}


def _expected():
    """The corpus and everything the tests compare against, computed once:
    (names, batch, oracle verdicts, ran flags, R' limbs, strict verdicts, tags)."""
    if "exp" not in _ref:
        names, b = E.corpus()
        oerr, ran, oxyz = _oracle.rprime_batch(b)
        strict = np.array(_strict_ref.verify_batch(b), np.int8)
        tags = _hashlib_tags(b)
        tags[oerr == -1] = 0
        for a in (oerr, ran, oxyz, strict, tags):
            a.setflags(write=False)
        assert len(b) == 274 and int((oerr != strict).sum()) == 117
        for c in RAN_CLASSES:
            assert ran[E.class_mask(b, c)].any(), c
        m = E.class_mask(b, "mix_a", "mix_r", "mix_ra", "on_table")
        assert ran[m].all() and {0, -3} <= set(oerr[m].tolist())
        m = E.class_mask(b, "nc_a", "nc_r", "near_a", "near_r")
        assert np.array_equal(ran[m], oerr[m] == -3) and set(oerr[m].tolist()) == {-2, -3}      # every one that decodes multiplies
        _ref["exp"] = (names, b, oerr, ran, oxyz, strict, tags)
    return _ref["exp"]


def _want(mode):
    from firedancer_amd import ed25519
    exp = _expected()
    return exp[5] if mode == ed25519.MODE_STRICT else exp[2]


def _bad(names, idx, got, want):
    bad = np.nonzero(got != want)[0]
    return int(bad.size), [(names[idx[i]], int(want[i]), int(got[i])) for i in bad[:8]]


def _run_dev(idx, mode, kind=None, pad=0, points=False):
    """verify_dev over corpus vectors idx (the kernel choice as set now):
    a dict with err (n + pad entries over a 0x55 fill), tags, and on request
    the parked R' read through layout `kind` and the decompression planes."""
    from firedancer_amd import ed25519, hip
    _, b = _expected()[:2]
    idx = np.asarray(idx, np.int64)
    n = idx.size
    blob = np.concatenate([np.asarray(b.blob, np.uint8), np.zeros(16, np.uint8)])
    d = [hip.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (b.pub[idx], b.sig[idx], b.msg_off[idx], b.msg_sz[idx], blob)]
    err = hip.DeviceBuffer.from_array(np.full(n + pad, 0x55, np.int8))
    ws = hip.DeviceBuffer(ed25519.workspace_footprint(n))
    tag = hip.DeviceBuffer.from_array(np.full(n + pad, 0x5555555555555555, np.uint64))
    st = hip.Stream()
    ed25519.verify_dev(n, *[x.ptr for x in d], err.ptr, ws.ptr, st.handle, mode=mode)
    ed25519.tags_dev(n, ws.ptr, tag.ptr, st.handle)
    out = {}
    if kind is not None:
        xyz = hip.DeviceBuffer.from_array(np.zeros(30 * n, np.int32))
        ed25519.debug_rprime_dev(n, ws.ptr, kind, xyz.ptr, st.handle)
    if points:
        dA, dR, dds = hip.DeviceBuffer(4 * 30 * n), hip.DeviceBuffer(4 * 20 * n), hip.DeviceBuffer(2 * n)
        ed25519.debug_points_dev(n, ws.ptr, dA.ptr, dR.ptr, dds.ptr, st.handle)
    st.synchronize()
    out["err"] = err.to_array(np.int8, n + pad)
    out["tag"] = tag.to_array(np.uint64, n + pad)
    if kind is not None:
        out["xyz"] = xyz.to_array(np.int32, 30 * n).reshape(30, n).T.copy()
    if points:
        out["A"] = dA.to_array(np.int32, 30 * n).reshape(30, n).T
        out["R"] = dR.to_array(np.int32, 20 * n).reshape(20, n).T
        out["ds"] = dds.to_array(np.uint8, 2 * n).reshape(n, 2)
    return out


def _check_run(idx, mode, out, what):
    """Verdicts and tags of one _run_dev, and the parked R' where it was read:
    all 30 limbs wherever the oracle's multiply ran."""
    from firedancer_amd import ed25519
    names, b, oerr, ran, oxyz, strict, tags = _expected()
    idx = np.asarray(idx, np.int64)
    n = idx.size
    assert not (out["err"][:n] == ed25519.VERDICT_DEVICE).any(), what
    want = _want(mode)[idx]
    assert np.array_equal(out["err"][:n], want), (what, _bad(names, idx, out["err"][:n], want))
    assert np.array_equal(out["tag"][:n], tags[idx]), (what, _bad(names, idx, out["tag"][:n], tags[idx]))
    assert (out["err"][n:] == 0x55).all() and (out["tag"][n:] == 0x5555555555555555).all(), what
    if "xyz" in out:
        r = ran[idx]
        bad = np.nonzero(r & (out["xyz"] != oxyz[idx]).any(axis=1))[0]
        assert bad.size == 0, (what, int(bad.size), [(names[idx[j]], int(oerr[idx[j]]),
                                                      np.nonzero(out["xyz"][j] != oxyz[idx[j]])[0][:6].tolist()) for j in bad[:6]])


@pytest.fixture
def dsm_kernel(request):
    from firedancer_amd import ed25519
    ed25519.select_dsm_kernel(request.param)
    yield request.param
    ed25519.debug_set_pool_waves(0)
    ed25519.select_dsm_kernel("default")


@pytest.mark.parametrize("dsm_kernel", KERNELS, indirect=True)
def test_corpus_every_kernel_both_modes(dsm_kernel):
    """The whole corpus through one kernel: reference verdicts, tags and the
    parked R' (every mix_*, on_table vector and every nc_* / near_* vector
    that decodes among them: _expected asserts their ran flags); then strict
    verdicts, the same tags and the same parked R'."""
    from firedancer_amd import ed25519
    n = len(_expected()[1])
    for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
        _check_run(np.arange(n), mode, _run_dev(np.arange(n), mode, kind=dsm_kernel), (dsm_kernel, mode))


@pytest.mark.parametrize("dsm_kernel", ["k_dsm", "k_dsm8"], indirect=True)
def test_decompression_planes_of_the_corpus(dsm_kernel):
    """ds flags and the A / R limb planes of every vector with s < L (all of
    nc_* and near_* are) against the oracle's decompress2, through the gated
    k_decomp ("k_dsm") and the ungated k_front ("k_dsm8")."""
    from firedancer_amd import ed25519
    names, b, oerr = _expected()[:3]
    sel = np.array([i for i in range(len(b)) if int.from_bytes(bytes(b.sig[i][32:]), "little") < R.L], np.int64)
    must = E.class_mask(b, "nc_a", "nc_r", "near_a", "near_r")
    assert must[sel].sum() == must.sum() == 132
    if "planes" not in _ref:
        n = sel.size
        eA, eR, eds = np.zeros((n, 30), np.int32), np.zeros((n, 20), np.int32), np.zeros((n, 2), np.uint8)
        for j, i in enumerate(sel):                  # one point at a time: decompress2 stops at the first bad point of a pair
            pub, r = bytes(b.pub[i]), bytes(b.sig[i][:32])
            rc, a, _ = _oracle.decompress2(pub, pub)
            eds[j, 0] = rc != 0
            eA[j] = np.concatenate([(-a[0].astype(np.int64)).astype(np.int32), a[1], (-a[3].astype(np.int64)).astype(np.int32)])
            rc, c, _ = _oracle.decompress2(r, r)
            eds[j, 1] = rc != 0
            eR[j] = np.concatenate([c[0], c[1]])
        _ref["planes"] = (eA, eR, eds)
    eA, eR, eds = _ref["planes"]
    assert np.array_equal(eds.any(axis=1), oerr[sel] == -2)
    for c in ("nc_a", "near_a"):
        m = E.class_mask(b, c)[sel]
        assert eds[m, 0].any() and (eds[m, 0] == 0).any() and not eds[m, 1].any()
    for c in ("nc_r", "near_r"):
        m = E.class_mask(b, c)[sel]
        assert eds[m, 1].any() and (eds[m, 1] == 0).any() and not eds[m, 0].any()
    out = _run_dev(sel, ed25519.MODE_REFERENCE, points=True)
    _check_run(sel, ed25519.MODE_REFERENCE, out, dsm_kernel)
    assert np.array_equal(out["ds"], eds), [names[sel[j]] for j in np.nonzero((out["ds"] != eds).any(axis=1))[0][:8]]
    badA = np.nonzero((eds[:, 0] == 0) & (out["A"] != eA).any(axis=1))[0]
    badR = np.nonzero((eds[:, 1] == 0) & (out["R"] != eR).any(axis=1))[0]
    assert badA.size == 0, ("A limbs", [names[sel[j]] for j in badA[:8]])
    assert badR.size == 0, ("R limbs", [names[sel[j]] for j in badR[:8]])


@pytest.mark.parametrize("dsm_kernel", ["k_dsmp"], indirect=True)
@pytest.mark.parametrize("n,reverse", [(3 * P, False), (P + 1, True)])
def test_pool_placement(dsm_kernel, n, reverse):
    """k_dsmp on one wave: at 3 * 112 the corpus cycled, so every slot holds
    three generations and the on_table and s_abs vectors (a neutral
    accumulator; slots that stay free) share a pool with ordinary ones; at
    113 the corpus reversed, one refill.  Verdicts in both modes and the
    parked R' limb for limb."""
    from firedancer_amd import ed25519
    names, b, oerr, ran = _expected()[:4]
    N = len(b)
    idx = np.array([(N - 1 - i if reverse else i) % N for i in range(n)], np.int64)
    special = E.class_mask(b, "on_table", "s_abs")[idx]
    if reverse:
        assert n == P + 1 and special[:P].sum() == 27                      # all of them in the first claim; then one refill of one
    else:
        assert n > N and int(ran[idx].sum()) > 2 * P                        # the corpus and a second pass; slots refill twice over
        assert special[:P].sum() == 0 and special[P:].sum() == 27          # every on_table / s_abs vector enters through a refill
    ed25519.debug_set_pool_waves(1)
    for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
        _check_run(idx, mode, _run_dev(idx, mode, kind="k_dsmp"), (n, reverse, mode))


@pytest.mark.parametrize("dsm_kernel", KERNELS, indirect=True)
def test_partial_wave(dsm_kernel):
    """n = 65: the last lane, alone in its wave, is a vector whose strict
    verdict differs from the reference's; nothing is written past err[n) or
    tag[n)."""
    from firedancer_amd import ed25519
    names, b, oerr, ran, oxyz, strict, tags = _expected()
    differ = np.nonzero(oerr != strict)[0]
    last = int(differ[E.class_mask(b, "nc_a")[differ] & (oerr[differ] == -3)][5])
    head = [i for i in np.arange(len(b))[::4].tolist() if i != last][:64]
    idx = np.array(head + [last], np.int64)
    assert idx.size == 65 and (oerr[last], strict[last]) == (-3, -2) and (oerr[idx[:64]] != strict[idx[:64]]).any()
    for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
        _check_run(idx, mode, _run_dev(idx, mode, kind=dsm_kernel, pad=192), (dsm_kernel, mode))


def test_host_entry_points_both_modes():
    """verify_soa, verify_batch, verify_soa_registered and the registered
    pointer-array call, default kernel choice, once each per mode, with tags."""
    from firedancer_amd import ed25519
    names, b, oerr, ran, oxyz, strict, tags = _expected()
    n = len(b)
    idx = np.arange(n)
    e = ed25519.Engine(device=0, batch_max=512, blob_max=512 * 1232)
    planes = ed25519.RegisteredPlanes(b.pub, b.sig, b.msg_off, b.msg_sz, b.blob)
    # one arena for the pointer-array form: keys, signatures and messages at odd offsets
    recs = [bytes(b.pub[i]) + b"\xa5" + bytes(b.sig[i]) + b"\x5a" + b.msg(i) for i in range(n)]
    ends = np.cumsum([len(r) for r in recs])
    start = np.concatenate([[0], ends[:-1]]).astype(np.uint64) + 3
    arena = ed25519.RegisteredPlanes(np.frombuffer(b"\0\0\0" + b"".join(recs) + bytes(16), np.uint8))
    try:
        for mode in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
            e.set_mode(mode)
            want = _want(mode)
            outs = {
                "verify_soa": e.verify_soa(b.pub, b.sig, b.msg_off, b.msg_sz, b.blob, want_tags=True),
                "verify_batch": e.verify_batch([b.msg(i) for i in range(n)], [bytes(s) for s in b.sig], [bytes(p) for p in b.pub],
                                               want_tags=True),
                "verify_soa_registered": e.verify_soa_registered(planes[0], planes[1], planes[2], planes[3], planes[4],
                                                                 want_tags=True),
                "verify_batch_registered": e.verify_batch_registered(arena[0], start, start + 33, start + 98, b.msg_sz,
                                                                     want_tags=True),
            }
            for name, (err, tag) in outs.items():
                assert np.array_equal(err, want), (name, mode, _bad(names, idx, err, want))
                assert np.array_equal(tag, tags), (name, mode, _bad(names, idx, tag, tags))
    finally:
        arena.close()
        planes.close()
        e.close()


# ---- transactions -----------------------------------------------------------------------

def test_transactions_with_an_edge_signer_both_modes():
    """3-signer transactions whose edge signer (a non-canonical A that
    decodes, a mixed-order A that accepts / rejects, A = B with R the
    identity, a near-miss A) is first, in the middle or last: the verdict is
    that signature's code, through verify_txns and verify_txns_registered."""
    from firedancer_amd import ed25519
    from test_strict_gpu import _strict_txn
    cases = E.txn_cases()
    pays = [p for _, p, _ in cases]
    blob, off, sz = _txn.pack(pays)
    eterr, ebase, eserr = _oracle.txn_verify_batch(blob, off, sz)
    st = [_strict_txn(p) for p in pays]
    sterr = np.array([t for t, _ in st], np.int8)
    sserr = np.array([v for _, s in st for v in s], np.int8)
    assert {0, -3} <= set(eterr.tolist()) and {0, -2, -3} <= set(sterr.tolist()) and int((eterr != sterr).sum()) == 6
    e = ed25519.Engine(device=0, batch_max=256, blob_max=256 * 1232)
    arena = ed25519.RegisteredPlanes(blob)
    try:
        for mode, wt, ws in ((ed25519.MODE_REFERENCE, eterr, eserr), (ed25519.MODE_STRICT, sterr, sserr)):
            e.set_mode(mode)
            for name, out in (("verify_txns", e.verify_txns(blob, off, sz, want_sigs=True)),
                              ("verify_txns_registered", e.verify_txns_registered(arena[0], off, sz, want_sigs=True))):
                terr, base, serr = out
                assert np.array_equal(base, ebase), name
                assert np.array_equal(terr, wt), (name, mode, [(cases[t][0], int(wt[t]), int(terr[t])) for t in np.nonzero(terr != wt)[0]])
                assert np.array_equal(serr, ws), (name, mode, np.nonzero(serr != ws)[0].tolist())
    finally:
        arena.close()
        e.close()
