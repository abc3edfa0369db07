"""CPU: the dedup tag's host-side surface.  fd_ed25519_amd_tag is the written
definition of the value every *_tag batch call returns -- the little-endian
u64 of the first 8 bytes of SHA-512(R || A || M) -- checked here against
hashlib; and the *_tag batch calls fail without a device exactly as the
untagged calls do."""
import ctypes
import hashlib

import numpy as np
import pytest

INVAL, DEVICE = -10, -11

# message sizes at the padding edges of nblk = (64 + sz + 17 + 127) / 128: one | two blocks at 47 | 48, two | three
# at 175 | 176, the 111 | 112 pair (the length field's edge for an unprefixed message), and the MTU
EDGE_SIZES = [0, 47, 48, 111, 112, 175, 176, 1232]


def hashlib_tag(msg, sig, pub):
    return int.from_bytes(hashlib.sha512(bytes(sig)[:32] + bytes(pub) + bytes(msg)).digest()[:8], "little")


def test_host_tag_on_the_golden_vectors(golden):
    from firedancer_amd import ed25519
    for i in range(len(golden)):
        m, s, p = golden.msg(i), bytes(golden.sig[i]), bytes(golden.pub[i])
        assert ed25519.tag(m, s, p) == hashlib_tag(m, s, p), i


@pytest.mark.parametrize("sz", EDGE_SIZES)
def test_host_tag_at_the_padding_edges(sz):
    from firedancer_amd import ed25519
    rng = np.random.default_rng(1000 + sz)
    for _ in range(4):
        m, s, p = (rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (sz, 64, 32))
        assert ed25519.tag(m, s, p) == hashlib_tag(m, s, p)
        assert ed25519.tag(m, s[:32] + bytes(32), p) == hashlib_tag(m, s, p)     # only R = sig[0:32] is hashed


def _fake_engine():
    """Zeroed memory the size of an engine whose first field, the device
    ordinal, is one no host has: a batch call on it passes its argument checks
    and fails at its first device call (hipSetDevice), with or without a GPU
    in the machine, before it looks at anything else in the engine."""
    buf = ctypes.create_string_buffer(1 << 16)
    ctypes.c_int.from_buffer(buf).value = 0x7ffffff0
    return buf


def test_tag_calls_without_a_device_fail_like_the_untagged_calls():
    from firedancer_amd import ed25519
    L = ed25519.lib()
    z = ctypes.c_void_p(0)
    buf = _fake_engine()
    e = ctypes.cast(buf, ctypes.c_void_p)
    pub, sig = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)
    off, sz, blob = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(4, np.uint8)
    err, tag = np.zeros(1, np.int8), np.zeros(1, np.uint64)
    P = ed25519._ptr
    soa = (P(pub), P(sig), P(off), P(sz), P(blob), 4)

    # the device error, tags asked for or not
    assert L.fd_ed25519_amd_verify_soa(e, 1, *soa, P(err)) == DEVICE
    assert L.fd_ed25519_amd_verify_soa_tag(e, 1, *soa, P(err), P(tag)) == DEVICE
    assert L.fd_ed25519_amd_verify_soa_tag(e, 1, *soa, P(err), z) == DEVICE
    mp = (ctypes.c_void_p * 1)(blob.ctypes.data)
    sp = (ctypes.c_void_p * 1)(sig.ctypes.data)
    pp = (ctypes.c_void_p * 1)(pub.ctypes.data)
    msz = (ctypes.c_ulong * 1)(0)
    assert L.fd_ed25519_amd_verify_batch(e, 1, mp, msz, sp, pp, P(err)) == DEVICE
    assert L.fd_ed25519_amd_verify_batch_tag(e, 1, mp, msz, sp, pp, P(err), P(tag)) == DEVICE
    # (the fake engine stages no payload: an empty transaction batch reaches the device call too)
    assert L.fd_ed25519_amd_verify_txns(e, 0, z, z, z, 0, z, z, z) == DEVICE
    assert L.fd_ed25519_amd_verify_txns_tag(e, 0, z, z, z, 0, z, z, z, P(tag), z) == DEVICE
    # unregistered planes are refused before the device is looked for, tagged or not
    assert L.fd_ed25519_amd_verify_soa_registered_tag(e, 1, *soa, P(err), P(tag)) == \
        L.fd_ed25519_amd_verify_soa_registered(e, 1, *soa, P(err)) != 0

    # NULL planes and NULL engines: ERR_INVAL, exactly as the untagged calls
    for n, args in ((1, (z, P(sig), P(off), P(sz), P(blob), 4, P(err))), (1, (P(pub), P(sig), P(off), P(sz), P(blob), 4, z))):
        assert L.fd_ed25519_amd_verify_soa(e, n, *args) == INVAL
        assert L.fd_ed25519_amd_verify_soa_tag(e, n, *args, P(tag)) == INVAL
        assert L.fd_ed25519_amd_verify_soa_registered_tag(e, n, *args, P(tag)) == INVAL
        assert L.fd_ed25519_amd_multi_verify_soa_tag(z, n, *args, P(tag)) == INVAL
    assert L.fd_ed25519_amd_verify_soa_tag(z, 1, *soa, P(err), P(tag)) == INVAL
    assert L.fd_ed25519_amd_multi_verify_soa_tag(z, 1, *soa, P(err), P(tag)) == INVAL
    assert L.fd_ed25519_amd_verify_batch_tag(e, 1, None, msz, sp, pp, P(err), P(tag)) == INVAL
    assert L.fd_ed25519_amd_verify_batch_tag(z, 1, mp, msz, sp, pp, P(err), P(tag)) == INVAL
    pay, toff, tsz, terr = np.zeros(8, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.int8)
    assert L.fd_ed25519_amd_verify_txns(e, 1, z, P(toff), P(tsz), 8, P(terr), z, z) == INVAL
    assert L.fd_ed25519_amd_verify_txns_tag(e, 1, z, P(toff), P(tsz), 8, P(terr), z, z, P(tag), z) == INVAL
    assert L.fd_ed25519_amd_verify_txns_tag(z, 0, z, z, z, 0, z, z, z, P(tag), z) == INVAL
    assert L.fd_ed25519_amd_multi_verify_txns_tag(z, 0, z, z, z, 0, z, z, z, P(tag), z) == INVAL
    # per-signature tags are numbered by sig_base, as sig_err is: refused without it
    assert L.fd_ed25519_amd_verify_txns_tag(e, 0, z, z, z, 0, z, z, z, z, P(tag)) == INVAL
    # the device-resident readers: n = 0 is OK and touches nothing, NULL and misaligned outputs are refused
    assert L.fd_ed25519_amd_tags_dev(0, z, z, z) == 0 and L.fd_ed25519_amd_txn_tags_dev(0, z, z, z, z) == 0
    assert L.fd_ed25519_amd_tags_dev(64, z, z, z) == INVAL and L.fd_ed25519_amd_txn_tags_dev(64, z, z, z, z) == INVAL
    one = ctypes.c_void_p(4096 + 4)
    assert L.fd_ed25519_amd_tags_dev(64, one, one, z) == INVAL and L.fd_ed25519_amd_txn_tags_dev(64, one, one, one, z) == INVAL


def test_want_tags_python_forms_raise_without_a_device():
    from firedancer_amd import ed25519
    buf = _fake_engine()
    pub, sig = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)
    off, sz, blob = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(4, np.uint8)
    eng = ed25519.Engine.__new__(ed25519.Engine)
    eng._h = ctypes.cast(buf, ctypes.c_void_p)
    try:
        for want_tags in (False, True):
            with pytest.raises(ed25519.EngineError, match="rc=-11"):
                eng.verify_soa(pub, sig, off, sz, blob, want_tags=want_tags)
            with pytest.raises(ed25519.EngineError, match="rc=-11"):
                eng.verify_batch([b""], [bytes(64)], [bytes(32)], want_tags=want_tags)
            with pytest.raises(ed25519.EngineError):
                eng.verify_soa_registered(pub, sig, off, sz, blob, want_tags=want_tags)
            with pytest.raises(ed25519.EngineError, match="rc=-11"):
                eng.verify_txns(np.zeros(4, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32),
                                want_sigs=True, want_tags=want_tags)
    finally:
        eng._h = None                                        # nothing to delete
    multi = ed25519.MultiEngine.__new__(ed25519.MultiEngine)
    multi._h = None
    for want_tags in (False, True):
        with pytest.raises(ed25519.EngineError):
            multi.verify_soa(pub, sig, off, sz, blob, want_tags=want_tags)
        with pytest.raises(ed25519.EngineError):
            multi.verify_txns(np.zeros(4, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32), want_tags=want_tags)
