"""ctypes binding of the CPU oracle (oracle/liboracle.so) -- TEST CHECKER ONLY.

The oracle is the clean-room C restatement of the reference verdict function
(oracle/fd_ed25519_oracle.c); it is used here to check the HIP engine, never
as the thing measured or shipped.  oracle/_ref/libfdref.so (the reference's
own sources, compiled) is bound too when present, as a second checker.
"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfdref.so")

_o = None
_r = None


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else ctypes.c_void_p(0)


def oracle():
    global _o
    if _o is None:
        if not os.path.exists(ORACLE_SO):
            raise RuntimeError("oracle/liboracle.so missing: run __graft_entry__.build()")
        L = ctypes.CDLL(ORACLE_SO)
        vp = ctypes.c_void_p
        L.oracle_ed25519_verify.argtypes = [vp, ctypes.c_size_t, vp, vp]
        L.oracle_ed25519_verify.restype = ctypes.c_int
        L.oracle_ed25519_verify_batch.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        L.oracle_ed25519_verify_batch.restype = ctypes.c_int
        L.oracle_ed25519_verify_rprime.argtypes = [vp, ctypes.c_size_t, vp, vp, vp, vp]
        L.oracle_ed25519_verify_rprime.restype = ctypes.c_int
        L.oracle_ed25519_rprime_batch.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        L.oracle_ed25519_rprime_batch.restype = ctypes.c_int
        L.oracle_sha512.argtypes = [vp, ctypes.c_size_t, vp]
        L.oracle_sha512.restype = None
        L.oracle_sc_reduce.argtypes = [vp, vp]
        L.oracle_sc_reduce.restype = None
        L.oracle_stream_gen.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_int, vp, vp, vp, vp, vp, vp]
        L.oracle_stream_gen.restype = ctypes.c_uint64
        L.oracle_txn_parse.argtypes = [vp, ctypes.c_ulong, vp, vp]
        L.oracle_txn_parse.restype = ctypes.c_ulong
        L.oracle_txn_parse_fail_line.argtypes = [vp, ctypes.c_ulong]
        L.oracle_txn_parse_fail_line.restype = ctypes.c_ulong
        L.oracle_txn_desc_max.argtypes = []
        L.oracle_txn_desc_max.restype = ctypes.c_ulong
        L.oracle_txn_verify_batch.argtypes = [ctypes.c_ulong, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        L.oracle_txn_verify_batch.restype = ctypes.c_int
        ci = ctypes.c_int
        for name, args in (("oracle_fe_mul", [vp, vp, vp]), ("oracle_fe_sqn", [vp, vp, ci]),
                           ("oracle_fe_pow22523", [vp, vp]), ("oracle_fe_frombytes", [vp, vp]),
                           ("oracle_fe_tobytes", [vp, vp]), ("oracle_ge_dbl", [vp, vp]),
                           ("oracle_ge_add", [vp, vp, vp, ci]), ("oracle_ge_p1p1_to_p3", [vp, vp]),
                           ("oracle_ge_to_cached", [vp, vp]), ("oracle_slide", [vp, vp]),
                           ("oracle_opmax_enable", [ci]), ("oracle_opmax_reset", []), ("oracle_opmax_get", [vp])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = None
        L.oracle_decompress2.argtypes = [vp, vp, vp, vp]
        L.oracle_decompress2.restype = ci
        _o = L
    return _o


# ---- limb-level exports (field elements: lists of ten ints; points: lists of elements) ----

def _limbs_in(*fes):
    return np.ascontiguousarray(np.array([v for f in fes for v in f], np.int64).astype(np.int32))


def _call_limbs(name, n_out, *args):
    out = np.zeros(10 * n_out, np.int32)
    getattr(oracle(), name)(_p(out), *args)
    o = out.tolist()
    return [o[10 * k:10 * k + 10] for k in range(n_out)]


def fe_mul(f, g):
    a, b = _limbs_in(f), _limbs_in(g)
    return _call_limbs("oracle_fe_mul", 1, _p(a), _p(b))[0]


def fe_sqn(f, n=1):
    a = _limbs_in(f)
    return _call_limbs("oracle_fe_sqn", 1, _p(a), n)[0]


def fe_pow22523(f):
    a = _limbs_in(f)
    return _call_limbs("oracle_fe_pow22523", 1, _p(a))[0]


def fe_frombytes(s):
    return _call_limbs("oracle_fe_frombytes", 1, bytes(s))[0]


def fe_tobytes(f):
    out = ctypes.create_string_buffer(32)
    a = _limbs_in(f)
    oracle().oracle_fe_tobytes(out, _p(a))
    return out.raw


def ge_dbl(X, Y, Z):
    a = _limbs_in(X, Y, Z)
    return tuple(_call_limbs("oracle_ge_dbl", 4, _p(a)))


def ge_add(u, q, neg):
    a, b = _limbs_in(*u), _limbs_in(*q)
    return tuple(_call_limbs("oracle_ge_add", 4, _p(a), _p(b), int(neg)))


def ge_p1p1_to_p3(t):
    a = _limbs_in(*t)
    return tuple(_call_limbs("oracle_ge_p1p1_to_p3", 4, _p(a)))


def ge_to_cached(u):
    a = _limbs_in(*u)
    return tuple(_call_limbs("oracle_ge_to_cached", 4, _p(a)))


def decompress2(pub, r):
    """(rc, A, R): the reference's 2-point decompression, limbs out; A and R
    are (X, Y, Z, T) as int32 arrays of shape (4, 10) (A not yet negated)."""
    A, R = np.zeros(40, np.int32), np.zeros(40, np.int32)
    rc = oracle().oracle_decompress2(_p(A), bytes(pub), _p(R), bytes(r))
    return rc, A.reshape(4, 10), R.reshape(4, 10)


def slide(a):
    """fd_ed25519_ge_slide of the 256-bit integer a: 256 digits."""
    out = np.zeros(256, np.int8)
    oracle().oracle_slide(_p(out), int(a).to_bytes(32, "little"))
    return out.tolist()


def opmax_measure(fn):
    """Run fn() with the oracle's operand maxima enabled; returns
    (mul even, mul odd, sqn even, sqn odd) max |limb|."""
    o = oracle()
    o.oracle_opmax_reset()
    o.oracle_opmax_enable(1)
    try:
        fn()
    finally:
        o.oracle_opmax_enable(0)
    m = np.zeros(4, np.int64)
    o.oracle_opmax_get(_p(m))
    return tuple(int(v) for v in m)


def ref():
    """The compiled reference (None when oracle/_ref was not built)."""
    global _r
    if _r is None and os.path.exists(REF_SO):
        L = ctypes.CDLL(REF_SO)
        vp = ctypes.c_void_p
        L.fd_sha512_new.argtypes = [vp]
        L.fd_sha512_new.restype = vp
        L.fd_sha512_join.argtypes = [vp]
        L.fd_sha512_join.restype = vp
        L.fd_ed25519_verify.argtypes = [vp, ctypes.c_ulong, vp, vp, vp]
        L.fd_ed25519_verify.restype = ctypes.c_int
        L.fd_ed25519_public_from_private.argtypes = [vp, vp, vp]
        L.fd_ed25519_public_from_private.restype = vp
        L.fd_ed25519_sign.argtypes = [vp, vp, ctypes.c_ulong, vp, vp, vp]
        L.fd_ed25519_sign.restype = vp
        L.fd_txn_parse.argtypes = [vp, ctypes.c_ulong, vp, vp]
        L.fd_txn_parse.restype = ctypes.c_ulong
        _r = L
    return _r


def verify(msg, sig, pub):
    m = bytes(msg)
    return oracle().oracle_ed25519_verify(m if m else None, len(m), bytes(sig), bytes(pub))


def verify_batch(batch, nthread=None, stats=False):
    n = len(batch)
    err = np.zeros(n, np.int8)
    st = np.zeros((n, 3), np.uint32) if stats else None
    if nthread is None:
        nthread = min(16, os.cpu_count() or 1)
    oracle().oracle_ed25519_verify_batch(
        n, _p(np.ascontiguousarray(batch.pub)), _p(np.ascontiguousarray(batch.sig)),
        _p(np.ascontiguousarray(batch.msg_off)), _p(np.ascontiguousarray(batch.msg_sz)),
        _p(np.ascontiguousarray(batch.blob)), _p(err), _p(st) if stats else None, nthread)
    return (err, st) if stats else err


def rprime(msg, sig, pub):
    """(verdict, ran, xyz): oracle.verify's verdict, whether the double-scalar
    multiply ran (False: s >= L, the s window's early 0, an undecodable
    point), and then its output R' = [s]B - [h]A as int32 (3, 10): the limbs
    of X, Y, Z (zeros when it did not run)."""
    m = bytes(msg)
    ran = ctypes.c_int(0)
    xyz = np.zeros(30, np.int32)
    rc = oracle().oracle_ed25519_verify_rprime(m if m else None, len(m), bytes(sig), bytes(pub), ctypes.byref(ran), _p(xyz))
    return rc, bool(ran.value), xyz.reshape(3, 10)


def rprime_batch(batch, nthread=None):
    """rprime over a batch, threaded like verify_batch: (err int8 [n], ran
    bool [n], xyz int32 [n][30])."""
    n = len(batch)
    err, ran, xyz = np.zeros(n, np.int8), np.zeros(n, np.uint8), np.zeros((n, 30), np.int32)
    if nthread is None:
        nthread = min(16, os.cpu_count() or 1)
    oracle().oracle_ed25519_rprime_batch(
        n, _p(np.ascontiguousarray(batch.pub)), _p(np.ascontiguousarray(batch.sig)),
        _p(np.ascontiguousarray(batch.msg_off)), _p(np.ascontiguousarray(batch.msg_sz)),
        _p(np.ascontiguousarray(batch.blob)), _p(err), _p(ran), _p(xyz), nthread)
    return err, ran.astype(bool), xyz


def sha512(data):
    out = ctypes.create_string_buffer(64)
    d = bytes(data)
    oracle().oracle_sha512(d if d else None, len(d), out)
    return out.raw


def sc_reduce(b64):
    out = ctypes.create_string_buffer(32)
    oracle().oracle_sc_reduce(out, bytes(b64))
    return out.raw


def _ref_sha(R):
    """One fd_sha512 object for the compiled reference's calls."""
    if not hasattr(ref_verify, "_sha"):
        buf = ctypes.create_string_buffer(256 + 128)
        addr = (ctypes.addressof(buf) + 127) & ~127
        ref_verify._buf = buf
        ref_verify._sha = R.fd_sha512_join(R.fd_sha512_new(addr))
    return ref_verify._sha


def ref_verify(msg, sig, pub):
    R = ref()
    if R is None:
        return None
    m = bytes(msg)
    return R.fd_ed25519_verify(m if m else None, len(m), bytes(sig), bytes(pub), _ref_sha(R))


def ref_sign(seed, msg):
    """The compiled reference's own fd_ed25519_public_from_private and
    fd_ed25519_sign: (pub, sig); None when oracle/_ref was not built."""
    R = ref()
    if R is None:
        return None
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    m, prv = bytes(msg), bytes(seed)
    R.fd_ed25519_public_from_private(pub, prv, _ref_sha(R))
    R.fd_ed25519_sign(sig, m if m else None, len(m), pub, prv, _ref_sha(R))
    return pub.raw, sig.raw


def stream_inputs(seed, count, szlo, szhi, mixed):
    """Draw-for-draw regeneration of oracle/vecgen.h streams (unsigned)."""
    prv = np.zeros((count, 32), np.uint8)
    blob = np.zeros(count * max(szhi, 1) + 1, np.uint8)
    off = np.zeros(count, np.uint32)
    sz = np.zeros(count, np.uint32)
    fk = np.zeros(count, np.uint8)
    fp = np.zeros(count, np.uint32)
    used = oracle().oracle_stream_gen(seed, count, szlo, szhi, int(mixed), _p(prv), _p(blob), _p(off), _p(sz),
                                      _p(fk), _p(fp))
    return prv, blob[:used + 1], off, sz, fk, fp


def txn_desc_max():
    """Room a descriptor buffer needs for any payload the parser accepts (up
    to 65535 B): the oracle's ORACLE_TXN_DESC_MAX."""
    return int(oracle().oracle_txn_desc_max())


_txn_buf = None


def txn_parse(payload):
    """oracle fd_txn_parse: (footprint, descriptor bytes[:footprint], fail line)."""
    global _txn_buf
    p = bytes(payload)
    if _txn_buf is None:
        _txn_buf = ctypes.create_string_buffer(txn_desc_max())
    fp = oracle().oracle_txn_parse(p if p else None, len(p), _txn_buf, None)
    line = 0 if fp else oracle().oracle_txn_parse_fail_line(p if p else None, len(p))
    return int(fp), ctypes.string_at(_txn_buf, fp), int(line)


def ref_txn_parse(payload):
    """The compiled reference's fd_txn_parse, same triple as txn_parse (the
    line from its counters ring); None when oracle/_ref was not built."""
    R = ref()
    if R is None:
        return None
    p = bytes(payload)
    buf = ctypes.create_string_buffer(txn_desc_max())
    ctr = (ctypes.c_ulong * 34)()   # fd_txn_parse_counters_t: success_cnt, failure_cnt, failure_ring[32]
    fp = R.fd_txn_parse(p if p else None, len(p), buf, ctr)
    return int(fp), ctypes.string_at(buf, fp), 0 if fp else int(ctr[2])


def txn_verify_batch(payload, txn_off, txn_sz, nthread=None):
    """Multi-signer verdicts: (txn_err, sig_base, sig_err) -- the rule of
    fd_ed25519_amd_verify_txns on the CPU oracle."""
    payload = np.ascontiguousarray(payload, np.uint8)
    off = np.ascontiguousarray(txn_off, np.uint32)
    sz = np.ascontiguousarray(txn_sz, np.uint32)
    n = off.size
    terr = np.zeros(max(n, 1), np.int8)
    base = np.zeros(n + 1, np.uint32)
    serr = np.zeros(max(payload.size // 65 + 1, 1), np.int8)
    if nthread is None:
        nthread = min(16, os.cpu_count() or 1)
    if oracle().oracle_txn_verify_batch(n, _p(payload), _p(off), _p(sz), _p(terr), _p(base), _p(serr), nthread):
        raise MemoryError("oracle_txn_verify_batch: no descriptor buffer")
    return terr[:n], base, serr[:int(base[-1])]
