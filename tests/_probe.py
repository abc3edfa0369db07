"""ctypes binding of the probe library (tests/hip/libfd_probe.so, built by
firedancer_amd.build.build_probe from tests/hip/fd_probe.hip): small kernels
around the device field / group functions -- TEST INFRASTRUCTURE ONLY."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SO = os.path.join(ROOT, "tests", "hip", "libfd_probe.so")

_l = None
_dead = None  # the first HIP error: nothing more is launched after one
OPS = {}      # name -> (op, lanes per case, in0, in1, aux, out ints per case)


def lib():
    global _l
    if _l is None:
        if not os.path.exists(PROBE_SO):
            raise RuntimeError("tests/hip/libfd_probe.so missing: run __graft_entry__.build()")
        L = ctypes.CDLL(PROBE_SO)
        vp = ctypes.c_void_p
        L.fd_probe_run.argtypes = [ctypes.c_int, ctypes.c_ulong, vp, vp, vp, vp]
        L.fd_probe_run.restype = ctypes.c_int
        L.fd_probe_name.argtypes = [ctypes.c_int]
        L.fd_probe_name.restype = ctypes.c_char_p
        L.fd_probe_shape.argtypes = [ctypes.c_int, vp]
        L.fd_probe_shape.restype = ctypes.c_int
        L.fd_probe_op_cnt.restype = ctypes.c_int
        for op in range(L.fd_probe_op_cnt()):
            sh = (ctypes.c_int * 5)()
            assert L.fd_probe_shape(op, sh) == 0
            OPS[L.fd_probe_name(op).decode()] = (op,) + tuple(sh)
        _l = L
    return _l


def _i32(a, n, stride, what):
    """(n, stride) int32 from any integer array; values may be given as
    int32 or as uint32 words."""
    if not stride:
        return None
    a = (np.asarray(a, np.int64).reshape(n, -1) & 0xffffffff).astype(np.uint32).view(np.int32)
    assert a.shape == (n, stride), (what, a.shape, stride)
    return np.ascontiguousarray(a)


def run(name, in0, in1=None, aux=None):
    """Run probe `name` on n cases; returns the (n, out stride) int32 result."""
    global _dead
    if _dead:
        raise RuntimeError("probe library not used after %s" % _dead)
    L = lib()
    op, _, s0, s1, sa, so = OPS[name]
    n = len(in0)
    a, b, x = _i32(in0, n, s0, "in0"), _i32(in1, n, s1, "in1"), _i32(aux, n, sa, "aux")
    out = np.zeros((n, so), np.int32)
    ptr = lambda v: ctypes.c_void_p(v.ctypes.data) if v is not None else None
    rc = L.fd_probe_run(op, n, ptr(a), ptr(b), ptr(x), ptr(out))
    if rc:
        _dead = "fd_probe_run(%s) failed: HIP error %d" % (name, rc)
        raise RuntimeError(_dead)
    return out
