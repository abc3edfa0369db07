"""Python mirror of the reference's ed25519 API over the MI355X engine.

Reference interface: src/ballet/ed25519/fd_ed25519.h (fd_ed25519_verify,
fd_ed25519_sign, fd_ed25519_public_from_private, fd_ed25519_strerror,
FD_ED25519_SUCCESS / ERR_SIG / ERR_PUBKEY / ERR_MSG).  Same names, same
argument meaning, same codes.  Everything here is a thin ctypes layer over
firedancer_amd/libfd_ed25519_amd.so (include/fd_ed25519_amd.h); the verify
work always runs in the HIP kernels.  If the library is missing this module
raises at import of the first call -- there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

FD_ED25519_SUCCESS = 0
FD_ED25519_ERR_SIG = -1
FD_ED25519_ERR_PUBKEY = -2
FD_ED25519_ERR_MSG = -3
FD_ED25519_SIG_SZ = 64
MSG_MAX = 1232

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FD_AMD_LIB") or os.path.join(_HERE, "libfd_ed25519_amd.so")   # override: A/B builds only

_lib = None

c_ulong_p = ctypes.POINTER(ctypes.c_ulong)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)


def lib():
    """Load the engine library (once).  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "firedancer_amd: %s missing -- build it with __graft_entry__.build() "
            "(the verify engine is HIP-only; there is no CPU path)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
    vp, ul, ui, i = ctypes.c_void_p, ctypes.c_ulong, ctypes.c_uint, ctypes.c_int
    L.fd_ed25519_verify.argtypes = [vp, ul, vp, vp, vp]
    L.fd_ed25519_verify.restype = i
    L.fd_ed25519_strerror.argtypes = [i]
    L.fd_ed25519_strerror.restype = ctypes.c_char_p
    L.fd_ed25519_public_from_private.argtypes = [vp, vp, vp]
    L.fd_ed25519_public_from_private.restype = vp
    L.fd_ed25519_sign.argtypes = [vp, vp, ul, vp, vp, vp]
    L.fd_ed25519_sign.restype = vp
    L.fd_ed25519_amd_new.argtypes = [i, ul, ul]
    L.fd_ed25519_amd_new.restype = vp
    L.fd_ed25519_amd_delete.argtypes = [vp]
    L.fd_ed25519_amd_delete.restype = None
    L.fd_ed25519_amd_verify_batch.argtypes = [vp, ul, c_void_pp, c_ulong_p, c_void_pp, c_void_pp, vp]
    L.fd_ed25519_amd_verify_batch.restype = i
    L.fd_ed25519_amd_verify_soa.argtypes = [vp, ul, vp, vp, vp, vp, vp, ul, vp]
    L.fd_ed25519_amd_verify_soa.restype = i
    L.fd_ed25519_amd_workspace_footprint.argtypes = [ul]
    L.fd_ed25519_amd_workspace_footprint.restype = ul
    L.fd_ed25519_amd_verify_dev.argtypes = [ul, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fd_ed25519_amd_verify_dev.restype = i
    L.fd_ed25519_amd_verify_dev_ev.argtypes = [ul, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fd_ed25519_amd_verify_dev_ev.restype = i
    L.fd_ed25519_amd_work_stats_dev.argtypes = [ul, vp, vp, vp]
    L.fd_ed25519_amd_work_stats_dev.restype = i
    L.fd_ed25519_amd_debug_digits_dev.argtypes = [ul, vp, vp, vp, vp]
    L.fd_ed25519_amd_debug_digits_dev.restype = i
    L.fd_ed25519_amd_debug_points_dev.argtypes = [ul, vp, vp, vp, vp, vp]
    L.fd_ed25519_amd_debug_points_dev.restype = i
    L.fd_ed25519_amd_version.argtypes = []
    L.fd_ed25519_amd_version.restype = ctypes.c_char_p
    L.fd_ed25519_amd_sign_batch.argtypes = [ul, vp, vp, vp, vp, vp, vp, i]
    L.fd_ed25519_amd_sign_batch.restype = i
    L.fd_ed25519_amd_verify_txns.argtypes = [vp, ul, vp, vp, vp, ul, vp, vp, vp]
    L.fd_ed25519_amd_verify_txns.restype = i
    L.fd_txn_amd_parse_dev.argtypes = [ul, vp, vp, vp, vp, vp, ul, vp]
    L.fd_txn_amd_parse_dev.restype = i
    L.fd_ed25519_amd_sign_dev.argtypes = [ul, vp, vp, vp, vp, vp, vp, vp]
    L.fd_ed25519_amd_sign_dev.restype = i
    L.fd_ed25519_amd_set_small_batch_max.argtypes = [ul]
    L.fd_ed25519_amd_set_small_batch_max.restype = None
    L.fd_ed25519_amd_set_latency_batch_max.argtypes = [ul]
    L.fd_ed25519_amd_set_latency_batch_max.restype = None
    L.fd_ed25519_amd_set_pool_batch_min.argtypes = [ul]
    L.fd_ed25519_amd_set_pool_batch_min.restype = None
    L.fd_ed25519_amd_debug_set_pool_iter_cap.argtypes = [ul]
    L.fd_ed25519_amd_debug_set_pool_iter_cap.restype = None
    L.fd_verify_amd_tile_new.argtypes = [i, ul, ul, ul, ul]
    L.fd_verify_amd_tile_new.restype = vp
    L.fd_verify_amd_tile_cfg_default.argtypes = [vp]
    L.fd_verify_amd_tile_cfg_default.restype = None
    L.fd_verify_amd_tile_new_cfg.argtypes = [vp]
    L.fd_verify_amd_tile_new_cfg.restype = vp
    L.fd_verify_amd_tile_set_trace.argtypes = [vp, vp, ul]
    L.fd_verify_amd_tile_set_trace.restype = None
    L.fd_verify_amd_tile_set_verdict_log.argtypes = [vp, vp, ul]
    L.fd_verify_amd_tile_set_verdict_log.restype = None
    L.fd_verify_amd_tile_cut.argtypes = [vp, ul, ul, ul, i, ul, i]
    L.fd_verify_amd_tile_cut.restype = ul
    L.fd_verify_amd_tile_mode.argtypes = [i, i, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    L.fd_verify_amd_tile_mode.restype = i

    L.fd_verify_amd_tile_pack.argtypes = [vp, ul, i, c_ulong_p]
    L.fd_verify_amd_tile_pack.restype = ul
    L.fd_verify_amd_tile_out_chunk0.argtypes = [vp]
    L.fd_verify_amd_tile_out_chunk0.restype = vp
    L.fd_verify_amd_tile_out_data_sz.argtypes = [vp]
    L.fd_verify_amd_tile_out_data_sz.restype = ul
    L.fd_ed25519_amd_host_register.argtypes = [vp, ul]
    L.fd_ed25519_amd_host_register.restype = i
    L.fd_ed25519_amd_host_unregister.argtypes = [vp]
    L.fd_ed25519_amd_host_unregister.restype = i
    L.fd_ed25519_amd_verify_soa_registered.argtypes = [vp, ul, vp, vp, vp, vp, vp, ul, vp]
    L.fd_ed25519_amd_verify_soa_registered.restype = i
    L.fd_ed25519_amd_multi_new.argtypes = [vp, ul, ul, ul]
    L.fd_ed25519_amd_multi_new.restype = vp
    L.fd_ed25519_amd_multi_delete.argtypes = [vp]
    L.fd_ed25519_amd_multi_delete.restype = None
    L.fd_ed25519_amd_multi_ndev.argtypes = [vp]
    L.fd_ed25519_amd_multi_ndev.restype = ul
    L.fd_ed25519_amd_shard_range.argtypes = [ul, ul, ul, c_ulong_p, c_ulong_p]
    L.fd_ed25519_amd_shard_range.restype = None
    L.fd_ed25519_amd_multi_verify_soa.argtypes = [vp, ul, vp, vp, vp, vp, vp, ul, vp]
    L.fd_ed25519_amd_multi_verify_soa.restype = i
    L.fd_ed25519_amd_multi_verify_txns.argtypes = [vp, ul, vp, vp, vp, ul, vp, vp, vp]
    L.fd_ed25519_amd_multi_verify_txns.restype = i
    L.fd_ed25519_amd_txn_slots.argtypes = [ul, vp, vp, vp, vp]
    L.fd_ed25519_amd_txn_slots.restype = ul
    L.fd_verify_amd_tile_register_dcache.argtypes = [vp, vp, ul]
    L.fd_verify_amd_tile_register_dcache.restype = i
    L.fd_verify_amd_tile_set_framing.argtypes = [vp, i]
    L.fd_verify_amd_tile_set_framing.restype = i
    L.fd_verify_amd_tile_delete.argtypes = [vp]
    L.fd_verify_amd_tile_delete.restype = None
    L.fd_verify_amd_tile_run.argtypes = [vp, vp, ul, vp, ul, vp, vp, ul, ul, vp, ul, vp, vp, vp, ul]
    L.fd_verify_amd_tile_run.restype = i
    L.fd_verify_amd_tickcount.argtypes = []
    L.fd_verify_amd_tickcount.restype = ui
    L.fd_verify_amd_bench_stream.argtypes = [i, ul, ul, ctypes.c_double, i, ul, ul, vp, vp, vp, vp, vp, vp, vp, ul,
                                             ul, vp]
    L.fd_verify_amd_bench_stream.restype = i
    # entry points added in round 6 and later (an A/B build of an earlier round, FD_AMD_LIB, lacks them)
    opt = {"fd_ed25519_amd_set_mode": ([vp, i], i), "fd_ed25519_amd_mode": ([vp], i),
           "fd_ed25519_amd_multi_set_mode": ([vp, i], i),
           "fd_ed25519_amd_verify_dev_mode": ([ul] + [vp] * 8 + [i], i),
           "fd_ed25519_amd_verify_dev_ev_mode": ([ul] + [vp] * 9 + [i], i),
           "fd_ed25519_amd_verify_txns_dev_mode": ([ul, ul] + [vp] * 8 + [i], i),
           "fd_ed25519_amd_dropin_set_device": ([i], i), "fd_ed25519_amd_dropin_device": ([], i),
           "fd_ed25519_amd_dropin_pick": ([ctypes.POINTER(i), i, i, ul], i),
           "fd_verify_amd_tile_level": ([i, i] + [ctypes.c_double] * 5, i),
           "fd_verify_amd_tile_level_step": ([i, i, ul, ul, ctypes.POINTER(ul)], i),
           # dedup tags
           "fd_ed25519_amd_tag": ([vp, ul, vp, vp], ul),
           "fd_ed25519_amd_verify_batch_tag": ([vp, ul, c_void_pp, c_ulong_p, c_void_pp, c_void_pp, vp, vp], i),
           "fd_ed25519_amd_verify_soa_tag": ([vp, ul, vp, vp, vp, vp, vp, ul, vp, vp], i),
           "fd_ed25519_amd_verify_soa_registered_tag": ([vp, ul, vp, vp, vp, vp, vp, ul, vp, vp], i),
           "fd_ed25519_amd_multi_verify_soa_tag": ([vp, ul, vp, vp, vp, vp, vp, ul, vp, vp], i),
           "fd_ed25519_amd_verify_txns_tag": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_multi_verify_txns_tag": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_tags_dev": ([ul, vp, vp, vp], i),
           "fd_ed25519_amd_txn_tags_dev": ([ul, vp, vp, vp, vp], i),
           # pointer-array batches gathered by the GPU from registered memory
           "fd_ed25519_amd_verify_batch_registered": ([vp, ul, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_verify_batch_registered_tag": ([vp, ul, vp, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_gather_layout": ([ul, vp, ul, ul, vp], ul),
           # transaction batches gathered by the GPU from registered memory
           "fd_ed25519_amd_verify_txns_registered": ([vp, ul, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_verify_txns_registered_tag": ([vp, ul, vp, vp, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_txn_slots_ptrs": ([ul, vp, vp, vp], ul),
           "fd_ed25519_amd_txn_gather_layout": ([ul, vp, vp, ul, ul, vp, vp], ul),
           # packed descriptors
           "fd_txn_amd_desc_bound": ([ul], ul),
           "fd_txn_amd_parse_packed_dev": ([ul, vp, vp, vp, vp, vp, vp, ul, vp, vp], i),
           "fd_txn_amd_parse_packed_scratch_footprint": ([ul], ul),
           "fd_ed25519_amd_verify_txns_desc": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp, vp, vp, ul], i),
           "fd_ed25519_amd_verify_txns_registered_desc": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul], i),
           # asynchronous submissions
           "fd_ed25519_amd_new_slots": ([i, ul, ul, ul], vp),
           "fd_ed25519_amd_async_depth": ([vp], ul), "fd_ed25519_amd_async_in_flight": ([vp], ul),
           "fd_ed25519_amd_submit_batch": ([vp, ul, vp, vp, vp, vp, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_batch_registered": ([vp, ul, vp, vp, vp, vp, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_txns": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp, vp, vp, ul, c_ulong_p], i),
           "fd_ed25519_amd_submit_txns_registered": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, c_ulong_p], i),
           "fd_ed25519_amd_async_poll": ([vp, c_ulong_p], i), "fd_ed25519_amd_async_wait": ([vp, c_ulong_p], i),
           # survivors: in-batch dedup and the verdict filter
           "fd_ed25519_amd_keep": ([ul, vp, vp, vp], ul),
           "fd_ed25519_amd_keep_scratch_footprint": ([ul], ul),
           "fd_ed25519_amd_keep_dev": ([ul, vp, vp, vp, vp, vp, ul, vp], i),
           "fd_ed25519_amd_submit_batch_keep": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_batch_registered_keep": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_txns_keep": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_txns_registered_keep": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, c_ulong_p], i),
           # output frames: the survivors' bytes, written by the GPU
           "fd_ed25519_amd_emit_bound": ([ul], ul), "fd_txn_amd_emit_bound": ([ul], ul),
           "fd_ed25519_amd_emit": ([ul, vp, vp, vp, vp, vp, vp, ul, vp, vp], ul),
           "fd_txn_amd_emit": ([ul, vp, vp, vp, vp, vp, vp, ul, vp, vp], ul),
           "fd_ed25519_amd_emit_scratch_footprint": ([ul], ul),
           "fd_ed25519_amd_emit_dev": ([ul, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, vp, vp], i),
           "fd_txn_amd_emit_dev": ([ul, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, vp, vp], i),
           "fd_ed25519_amd_submit_batch_emit": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_batch_registered_emit": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_txns_emit": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, vp, ul, vp, vp,
                                                c_ulong_p], i),
           "fd_ed25519_amd_submit_txns_registered_emit": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, vp, ul, vp, vp,
                                                           c_ulong_p], i),
           # compute budget: per transaction its compute units and fee
           "fd_txn_amd_budget": ([vp, ul, vp, vp], i),
           "fd_txn_amd_budget_dev": ([ul, vp, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_verify_txns_budget": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp, vp, vp, ul, vp], i),
           "fd_ed25519_amd_verify_txns_registered_budget": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp], i),
           "fd_ed25519_amd_submit_txns_budget": ([vp, ul, vp, vp, vp, ul, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, vp, ul, vp, vp,
                                                  vp, c_ulong_p], i),
           "fd_ed25519_amd_submit_txns_registered_budget": ([vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, ul, vp, vp, vp, ul, vp, vp,
                                                             vp, c_ulong_p], i),
           # the dedup window: dedup across submissions
           "fd_ed25519_amd_window_new": ([i, ul, ul], vp), "fd_ed25519_amd_window_delete": ([vp], None),
           "fd_ed25519_amd_window_depth": ([vp], ul),
           "fd_ed25519_amd_window_keep": ([vp, ul, vp, vp, vp], ul),
           "fd_ed25519_amd_window_keep_scratch_footprint": ([ul], ul),
           "fd_ed25519_amd_window_keep_dev": ([vp, ul, vp, vp, vp, vp, vp, vp], i),
           "fd_ed25519_amd_window_export": ([vp, vp], ul), "fd_ed25519_amd_window_import": ([vp, vp, ul], i),
           "fd_ed25519_amd_set_window": ([vp, vp], i), "fd_ed25519_amd_window": ([vp], vp),
           # frag submissions: the GPU reads the frag metadata
           "fd_ed25519_amd_frags": ([vp, ul, ul, vp, vp, vp, vp, vp], ul),
           "fd_ed25519_amd_submit_frags": ([vp, vp, ul, ul, vp, vp, vp, vp, vp, ul, vp, vp, c_ulong_p], i),
           "fd_ed25519_amd_frag_list_dev": ([vp, ul, ul, vp, vp, vp, vp], i),
           "fd_ed25519_amd_frag_check_dev": ([vp, ul, ul, vp, vp], i),
           # the streaming tile's verdict mode
           "fd_verify_amd_tile_set_verdict_mode": ([vp, i], i), "fd_verify_amd_tile_verdict_mode": ([vp], i),
           # debug: k_dsmp's grid, the parked R'
           "fd_ed25519_amd_debug_set_pool_waves": ([ul], None),
           "fd_ed25519_amd_debug_rprime_dev": ([ul, vp, i, vp, vp], i),
           # debug: the workspace's plane offsets (host only)
           "fd_ed25519_amd_debug_ws_layout": ([ul, c_ulong_p], None)}
    for name, (args, res) in opt.items():
        if hasattr(L, name) or not os.environ.get("FD_AMD_LIB"):
            f = getattr(L, name)
            f.argtypes, f.restype = args, res
    _lib = L
    return L


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


# ---------------------------------------------------------------- reference API

def strerror(err):
    """fd_ed25519_strerror (fd_ed25519.h:108-109)."""
    return lib().fd_ed25519_strerror(int(err)).decode()


def verify(msg, sig, public_key):
    """fd_ed25519_verify (fd_ed25519.h:96-101): returns 0 or FD_ED25519_ERR_*.
    Runs on the GPU as a batch of one."""
    m = bytes(msg)
    s = bytes(sig)
    p = bytes(public_key)
    assert len(s) == 64 and len(p) == 32
    mb = ctypes.create_string_buffer(m, max(len(m), 1))
    return lib().fd_ed25519_verify(mb if m else None, len(m), s, p, None)


DROPIN_AUTO = -1


def dropin_set_device(device):
    """fd_ed25519_amd_dropin_set_device: the calling thread's device for
    verify() (DROPIN_AUTO: the default rule).  Raises on a bad device."""
    rc = lib().fd_ed25519_amd_dropin_set_device(int(device))
    if rc:
        raise EngineError("fd_ed25519_amd_dropin_set_device(%d) rc=%d" % (device, rc))


def dropin_device():
    """The device of the calling thread's drop-in engine (-1 before its first call)."""
    return int(lib().fd_ed25519_amd_dropin_device())


def dropin_pick(dev_node, cpu_node, ordinal):
    """fd_ed25519_amd_dropin_pick: the default device rule (pure)."""
    a = (ctypes.c_int * max(len(dev_node), 1))(*dev_node)
    return int(lib().fd_ed25519_amd_dropin_pick(a, len(dev_node), int(cpu_node), int(ordinal)))


def public_from_private(private_key):
    """fd_ed25519_public_from_private (fd_ed25519.h:40-44)."""
    out = ctypes.create_string_buffer(32)
    lib().fd_ed25519_public_from_private(out, bytes(private_key), None)
    return out.raw


def sign(msg, public_key, private_key):
    """fd_ed25519_sign (fd_ed25519.h:71-78) -> 64-byte signature."""
    out = ctypes.create_string_buffer(64)
    m = bytes(msg)
    lib().fd_ed25519_sign(out, m if m else None, len(m), bytes(public_key), bytes(private_key), None)
    return out.raw


def sign_batch(prv, blob, msg_off, msg_sz, nthread=None):
    """Keygen + sign n messages on host threads: prv (n,32) u8 -> pub (n,32), sig (n,64)."""
    prv = np.ascontiguousarray(prv, np.uint8)
    n = prv.shape[0]
    blob = np.ascontiguousarray(blob, np.uint8)
    off = np.ascontiguousarray(msg_off, np.uint32)
    sz = np.ascontiguousarray(msg_sz, np.uint32)
    pub = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    if nthread is None:
        nthread = min(16, os.cpu_count() or 1)
    rc = lib().fd_ed25519_amd_sign_batch(n, _ptr(prv), _ptr(blob), _ptr(off), _ptr(sz), _ptr(pub), _ptr(sig), nthread)
    assert rc == 0
    return pub, sig


def tag(msg, sig, public_key):
    """fd_ed25519_amd_tag: the dedup tag of (msg, sig, pub) -- the
    little-endian u64 of the first 8 bytes of SHA-512(sig[0:32] || pub || msg),
    on the host (no device).  The want_tags batch forms return it from the
    GPU's hash, and 0 where the reference's s check rejects."""
    m = bytes(msg)
    s = bytes(sig)
    p = bytes(public_key)
    assert len(s) == 64 and len(p) == 32
    return int(lib().fd_ed25519_amd_tag(m if m else None, len(m), s, p))


def keep(err, tag):
    """fd_ed25519_amd_keep: the survivor rule on the host (no device).  The
    ascending indices (uint32) of the items with err == 0 that are the first
    passing item of their tag; tag 0 is never a duplicate.  What a want_keep
    submission delivers from the GPU."""
    e = np.ascontiguousarray(err, np.int8)
    t = np.ascontiguousarray(tag, np.uint64)
    n = int(e.size)
    assert t.size == n
    out = np.zeros(max(n, 1), np.uint32)
    cnt = int(lib().fd_ed25519_amd_keep(n, _ptr(e), _ptr(t), _ptr(out)))
    return out[:cnt]


class _Keep:
    """The survivor outputs of one want_keep submission, alive until it is
    delivered: args() is the (keep, keep_cnt) pair of the _keep submit calls
    (NULL, NULL when not asked for), result() keep[:keep_cnt].  With emit (a
    registered uint8 array, the submission's extent) the call is the _emit
    form (suffix): args() ends with out, out_cap, emit_off, emit_sz and
    results() with the pair (emit_off[:keep_cnt + 1], emit_sz[:keep_cnt])."""

    def __init__(self, n, want, emit=None):
        if emit is not None:
            if not want:
                raise EngineError("emit= needs want_keep=True: the frames are the survivors'")
            if emit.dtype != np.uint8 or not emit.flags["C_CONTIGUOUS"]:
                raise EngineError("emit= takes a contiguous uint8 array")
        self.keep = np.zeros(max(n, 1), np.uint32) if want else None
        self.cnt = np.zeros(1, np.uint64) if want else None
        self.emit = emit
        self.eoff = np.zeros(n + 1, np.uint64) if emit is not None else None
        self.esz = np.zeros(max(n, 1), np.uint32) if emit is not None else None
        self.suffix = "_emit" if emit is not None else "_keep"

    def args(self):
        a = (_ptr(self.keep), _ptr(self.cnt)) if self.keep is not None else (None, None)
        if self.emit is not None:
            a += (ctypes.c_void_p(self.emit.ctypes.data), int(self.emit.nbytes), _ptr(self.eoff), _ptr(self.esz))
        return a

    def result(self):
        return self.keep[:int(self.cnt[0])]

    def results(self):
        """What a want_keep submission appends to its delivered tuple."""
        c = int(self.cnt[0])
        return (self.keep[:c],) + (((self.eoff[:c + 1], self.esz[:c]),) if self.emit is not None else ())


def emit_bound(msg_sz):
    """fd_ed25519_amd_emit_bound: round_up(96 + msg_sz, 128), the extent a
    signature item needs in an emit= submission (no device)."""
    return int(lib().fd_ed25519_amd_emit_bound(int(msg_sz)))


def txn_emit_bound(payload_sz):
    """fd_txn_amd_emit_bound: the extent a transaction of payload_sz bytes
    needs in an emit= submission; 0 where no payload of that size parses."""
    return int(lib().fd_txn_amd_emit_bound(int(payload_sz)))


def _ptr_array(items):
    """(buffers, uint64 addresses, uint64 sizes) of a list of bytes-like."""
    raw = [bytes(b) for b in items]
    bufs = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in raw]
    return bufs, np.array([ctypes.addressof(b) for b in bufs], np.uint64), np.array([len(b) for b in raw], np.uint64)


def _emit_host(fn, keep, args, n_items, out, out_cap):
    k = np.ascontiguousarray(keep, np.uint32)
    c = int(k.size)
    eoff, esz = np.zeros(c + 1, np.uint64), np.zeros(max(c, 1), np.uint32)
    cap = (int(out.nbytes) if out_cap is None else int(out_cap)) if out is not None else 0
    assert out is None or (out.dtype == np.uint8 and cap <= out.nbytes)
    assert not c or int(k.max()) < n_items
    tot = int(fn(c, _ptr(k), *args, ctypes.c_void_p(out.ctypes.data) if out is not None else None, cap, _ptr(eoff), _ptr(esz)))
    return tot, eoff, esz[:c]


def emit(keep, msgs, sigs, pubs, out=None, out_cap=None):
    """fd_ed25519_amd_emit: the output-frame rule of the signature family on
    the host (no device).  For survivor j, item i = keep[j], the frame pub[i]
    | sig[i] | msg[i] goes to out + emit_off[j] (emit_sz[j] = 96 + len(msg[i])
    bytes, then zeros up to a multiple of 16); emit_off[j+1] = emit_off[j] +
    round_up(emit_sz[j], 128).  out: a uint8 array or None (layout only);
    out_cap: its capacity (default: all of it).  Returns (total, emit_off,
    emit_sz); total is 2**64 - 1, and nothing is written, when the frames do
    not fit.  What an emit= submission writes from the GPU."""
    mb, mp, msz = _ptr_array(msgs)
    sb, sp, _ = _ptr_array(sigs)
    pb, pp, _ = _ptr_array(pubs)
    return _emit_host(lib().fd_ed25519_amd_emit, keep, (_ptr(mp), _ptr(msz), _ptr(sp), _ptr(pp)), len(mb), out, out_cap)


def txn_emit(keep, payloads, desc_off, desc, out=None, out_cap=None):
    """fd_txn_amd_emit: the rule of the transaction family on the host.  The
    frame of transaction i is payload | zeros up to round_up(P, 16) | its
    fd_txn_t, desc[desc_off[i]:desc_off[i+1]] as the want_desc calls return
    them | P as a little-endian u16.  Arguments and result as emit."""
    tb, tp, tsz = _ptr_array(payloads)
    do = np.ascontiguousarray(desc_off, np.uint64)
    d = np.ascontiguousarray(desc, np.uint8)
    assert do.size == len(tb) + 1 and int(do[-1]) <= d.size
    return _emit_host(lib().fd_txn_amd_emit, keep, (_ptr(tp), _ptr(tsz), _ptr(do), _ptr(d)), len(tb), out, out_cap)


# ---------------------------------------------------------------- frag sources

VERDICT_FRAG_SEQ = -5   # FD_ED25519_AMD_VERDICT_FRAG_SEQ: the line did not (or no longer) hold the item's sequence number
VERDICT_FRAG_BAD = -6   # FD_ED25519_AMD_VERDICT_FRAG_BAD: the line's chunk / sz name no frag of the source
FRAG_MAX_DEFAULT = 96 + MSG_MAX
GATHER_REC = np.dtype([("pub", "<u8"), ("sig", "<u8"), ("msg", "<u8"), ("sz", "<u4"), ("dst", "<u4")])   # fd_amd_gather_rec_t


class FragSrc(ctypes.Structure):
    """fd_ed25519_amd_frag_src_t (include/fd_tango_amd.h)."""
    _fields_ = [("mcache", ctypes.c_void_p), ("depth", ctypes.c_ulong), ("chunk0", ctypes.c_void_p),
                ("data_sz", ctypes.c_ulong), ("frag_max", ctypes.c_ulong)]


def frag_src(mcache, region, frag_max=FRAG_MAX_DEFAULT, mcache_addr=None, chunk0_addr=None):
    """The FragSrc of an mcache (tango.mcache_new: a FRAG_META array of depth
    lines) and a data region (a uint8 array, chunk 0 at its first byte).
    mcache_addr / chunk0_addr: other addresses of the same memory (the device
    addresses the _dev calls take)."""
    return FragSrc(int(mcache.ctypes.data if mcache_addr is None else mcache_addr), int(mcache.size),
                   int(region.ctypes.data if chunk0_addr is None else chunk0_addr), int(region.nbytes), int(frag_max))


def frags(mcache, region, seq0, n, frag_max=FRAG_MAX_DEFAULT):
    """fd_ed25519_amd_frags: the frag rule on the host (no device) for items
    (seq0, n) of the source.  Returns (good, status, pub, sig, msg, sz):
    status int8 [n] (0, VERDICT_FRAG_SEQ or VERDICT_FRAG_BAD), the three
    addresses as uint64 [n] and the message sizes as uint64 [n] (0 where the
    status is nonzero), and the number of items whose status is 0.  What
    Engine.submit_frags decides on the GPU."""
    n = int(n)
    src = frag_src(mcache, region, frag_max)
    status = np.zeros(max(n, 1), np.int8)
    pub, sig, msg, sz = (np.zeros(max(n, 1), np.uint64) for _ in range(4))
    good = int(lib().fd_ed25519_amd_frags(ctypes.byref(src), int(seq0) & 0xFFFFFFFFFFFFFFFF, n, _ptr(status), _ptr(pub),
                                          _ptr(sig), _ptr(msg), _ptr(sz)))
    return good, status[:n], pub[:n], sig[:n], msg[:n], sz[:n]


def frag_list_dev(src, seq0, n, d_idle, d_rec, d_status, stream=0):
    """fd_ed25519_amd_frag_list_dev: k_frag_list alone, on `stream`, no sync.
    src: a FragSrc whose mcache and chunk0 are device addresses; d_idle: 96
    zero bytes of device memory; d_rec: n GATHER_REC records; d_status: n int8."""
    rc = lib().fd_ed25519_amd_frag_list_dev(ctypes.byref(src), int(seq0) & 0xFFFFFFFFFFFFFFFF, int(n), d_idle, d_rec, d_status,
                                            stream)
    if rc:
        raise EngineError("fd_ed25519_amd_frag_list_dev rc=%d" % rc)


def frag_check_dev(src, seq0, n, d_status, stream=0):
    """fd_ed25519_amd_frag_check_dev: the recheck alone (k_frag_check), on
    `stream`, no sync: every item whose d_status is 0 and whose line no longer
    holds seq0 + i becomes VERDICT_FRAG_SEQ."""
    rc = lib().fd_ed25519_amd_frag_check_dev(ctypes.byref(src), int(seq0) & 0xFFFFFFFFFFFFFFFF, int(n), d_status, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_frag_check_dev rc=%d" % rc)


# ---------------------------------------------------------------- batch engine

class EngineError(RuntimeError):
    pass


WINDOW_DEPTH_MAX = 1 << 22   # FD_ED25519_AMD_WINDOW_DEPTH_MAX


class Window:
    """fd_ed25519_amd_window_t: the last `depth` tags a caller published
    (include/fd_ed25519_amd.h, "The dedup window").  device < 0: host-only
    (keep); otherwise device-resident (keep_dev, or Engine.set_window).
    salt 0: drawn from the OS; no output depends on it."""

    def __init__(self, device, depth, salt=0):
        self._h = lib().fd_ed25519_amd_window_new(int(device), int(depth), int(salt) & (2**64 - 1))
        if not self._h:
            raise EngineError("fd_ed25519_amd_window_new(device=%d, depth=%d) failed" % (device, depth))
        self.device, self.depth = int(device), int(lib().fd_ed25519_amd_window_depth(self._h))

    def keep(self, err, tag):
        """fd_ed25519_amd_window_keep (host-only window): one submission; the
        survivors' indices (uint32), ascending."""
        e = np.ascontiguousarray(err, np.int8)
        t = np.ascontiguousarray(tag, np.uint64)
        n = int(e.size)
        assert t.size == n
        out = np.zeros(max(n, 1), np.uint32)
        cnt = int(lib().fd_ed25519_amd_window_keep(self._h, n, _ptr(e), _ptr(t), _ptr(out)))
        if cnt == 2**64 - 1:
            raise EngineError("fd_ed25519_amd_window_keep(n=%d) refused (n > depth %d, or a device window)" % (n, self.depth))
        return out[:cnt]

    def keep_dev(self, n, d_err, d_tag, d_keep, d_keep_cnt, d_scratch, stream=0):
        """fd_ed25519_amd_window_keep_dev: keep_dev's arguments; d_scratch
        holds window_keep_scratch_footprint(n) bytes.  No sync."""
        rc = lib().fd_ed25519_amd_window_keep_dev(self._h, int(n), d_err, d_tag, d_keep, d_keep_cnt, d_scratch, stream)
        if rc:
            raise EngineError("fd_ed25519_amd_window_keep_dev rc=%d" % rc)

    def export(self):
        """fd_ed25519_amd_window_export: the live tags (uint64), oldest first;
        waits for the window's queued work."""
        out = np.zeros(self.depth, np.uint64)
        cnt = int(lib().fd_ed25519_amd_window_export(self._h, _ptr(out)))
        if cnt > self.depth:
            raise EngineError("fd_ed25519_amd_window_export failed")
        return out[:cnt].copy()

    def load(self, tags):
        """fd_ed25519_amd_window_import: replace the contents with tags
        (nonzero, distinct, oldest first, at most depth); none: a reset."""
        t = np.ascontiguousarray(tags, np.uint64)
        rc = lib().fd_ed25519_amd_window_import(self._h, _ptr(t), int(t.size))
        if rc:
            raise EngineError("fd_ed25519_amd_window_import(cnt=%d) rc=%d" % (t.size, rc))

    def close(self):
        if self._h:
            lib().fd_ed25519_amd_window_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def window_keep_scratch_footprint(n):
    """fd_ed25519_amd_window_keep_scratch_footprint: device scratch bytes of Window.keep_dev for n items."""
    return int(lib().fd_ed25519_amd_window_keep_scratch_footprint(int(n)))


class EngineBusy(EngineError):
    """FD_ED25519_AMD_ERR_BUSY: every slot of the engine carries a submission."""


ERR_INVAL = -10      # FD_ED25519_AMD_ERR_INVAL
ERR_DEVICE = -11     # FD_ED25519_AMD_ERR_DEVICE
ERR_BUSY = -12       # FD_ED25519_AMD_ERR_BUSY
ASYNC_NONE = 1       # FD_ED25519_AMD_ASYNC_NONE
SLOT_MAX = 16        # FD_ED25519_AMD_SLOT_MAX


MODE_REFERENCE = 0   # FD_ED25519_AMD_MODE_REFERENCE: the reference's verdicts, bit for bit (default)
MODE_STRICT = 1      # FD_ED25519_AMD_MODE_STRICT: strict RFC 8032 (include/fd_ed25519_amd.h)


def _check_mode(mode):
    """A bad mode is refused here as the library refuses it: before any device call."""
    if mode not in (MODE_REFERENCE, MODE_STRICT):
        raise EngineError("bad verdict mode %r (MODE_REFERENCE or MODE_STRICT)" % (mode,))
    return int(mode)


class Engine:
    """fd_ed25519_amd_t: one engine per device (multi-GPU = one per device).
    mode: MODE_REFERENCE (default) or MODE_STRICT, for every entry point of
    this engine; set_mode changes it between batches.  nslot: its slot count
    (fd_ed25519_amd_new_slots, 2..SLOT_MAX), the depth of the submit_* /
    poll / wait calls; None: fd_ed25519_amd_new's."""

    def __init__(self, device=0, batch_max=1 << 16, blob_max=None, mode=MODE_REFERENCE, nslot=None):
        _check_mode(mode)
        self._h = None
        self._window = None  # the attached Window, kept alive
        self._pending = {}   # ticket -> (outputs of the delivered submission, what must stay alive until then)
        if blob_max is None:
            blob_max = max(batch_max * 256, MSG_MAX)
        if nslot is None:
            self._h = lib().fd_ed25519_amd_new(int(device), int(batch_max), int(blob_max))
        else:
            self._h = lib().fd_ed25519_amd_new_slots(int(device), int(batch_max), int(blob_max), int(nslot))
        if not self._h:
            raise EngineError("fd_ed25519_amd_new(device=%d) failed (no HIP device, or a bad slot count?)" % device)
        self.device = device
        if mode != MODE_REFERENCE:
            self.set_mode(mode)

    def set_mode(self, mode):
        rc = lib().fd_ed25519_amd_set_mode(self._h, int(mode))
        if rc:
            raise EngineError("fd_ed25519_amd_set_mode(%r) rc=%d" % (mode, rc))

    @property
    def mode(self):
        return int(lib().fd_ed25519_amd_mode(self._h))

    def set_window(self, win):
        """fd_ed25519_amd_set_window: the want_keep submissions filter against
        win (a Window on this engine's device, depth >= batch_max) and feed
        it; None detaches.  Refused while submissions are in flight."""
        rc = lib().fd_ed25519_amd_set_window(self._h, win._h if win is not None else None)
        if rc:
            raise EngineError("fd_ed25519_amd_set_window rc=%d" % rc)
        self._window = win

    def close(self):
        """fd_ed25519_amd_delete: waits for the submissions in flight and
        delivers none of them."""
        if self._h:
            lib().fd_ed25519_amd_delete(self._h)
            self._h = None
            self._pending.clear()
            self._window = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ asynchronous submissions

    @property
    def async_depth(self):
        """fd_ed25519_amd_async_depth: submissions the engine keeps in flight (its slot count)."""
        return int(lib().fd_ed25519_amd_async_depth(self._h))

    @property
    def in_flight(self):
        """fd_ed25519_amd_async_in_flight."""
        return int(lib().fd_ed25519_amd_async_in_flight(self._h))

    def _submitted(self, name, rc, ticket, finish, keep):
        if rc == ERR_BUSY:
            raise EngineBusy("%s: %d submissions in flight" % (name, self.in_flight))
        if rc:
            if not self.in_flight:        # a device error dropped what was in flight
                self._pending.clear()
            raise EngineError("%s rc=%d" % (name, rc))
        self._pending[int(ticket.value)] = (finish, keep)
        return int(ticket.value)

    def submit_batch_ptrs(self, pub_ptr, sig_ptr, msg_ptr, msg_sz, want_tags=False, registered=True, want_keep=False,
                          emit=None):
        """fd_ed25519_amd_submit_batch_registered (registered=False:
        fd_ed25519_amd_submit_batch, which copies the bytes behind the
        pointers before it returns): verify_batch_ptrs as one chunk, launched
        now and delivered by poll() / wait().  Returns the ticket; raises
        EngineBusy with async_depth submissions in flight, EngineError when the
        batch is empty or exceeds one chunk.  Registered: the bytes behind the
        pointers must stay valid until delivery.  want_keep (the _keep form of
        either call): the delivered result is a tuple that ends with keep, the
        uint32 indices of the survivors (module function keep), ascending.
        emit (the _emit form, with want_keep): a uint8 array inside one
        host_register registration, 64-aligned, at least the sum of
        emit_bound(msg_sz) bytes; the GPU writes the survivors' frames into it
        (module function emit) and the tuple ends with (emit_off, emit_sz)."""
        pp = np.ascontiguousarray(pub_ptr, np.uint64)
        sp = np.ascontiguousarray(sig_ptr, np.uint64)
        mp = np.ascontiguousarray(msg_ptr, np.uint64)
        sz = np.ascontiguousarray(msg_sz, np.uint64)
        n = int(pp.size)
        assert sp.size == n and mp.size == n and sz.size == n
        err = np.zeros(max(n, 1), np.int8)
        tags = np.zeros(max(n, 1), np.uint64) if want_tags else None
        name = "fd_ed25519_amd_submit_batch_registered" if registered else "fd_ed25519_amd_submit_batch"
        t = ctypes.c_ulong(0)
        args = (self._h, n, _ptr(mp), _ptr(sz), _ptr(sp), _ptr(pp), _ptr(err), _ptr(tags) if want_tags else None)
        if want_keep or emit is not None:
            k = _Keep(n, want_keep, emit)
            name = name + k.suffix
            rc = getattr(lib(), name)(*args, *k.args(), ctypes.byref(t))
            finish = lambda: ((err[:n], tags[:n]) if want_tags else (err[:n],)) + k.results()
        else:
            rc = getattr(lib(), name)(*args, ctypes.byref(t))
            finish = lambda: (err[:n], tags[:n]) if want_tags else err[:n]
        return self._submitted(name, rc, t, finish, ((pub_ptr, sig_ptr, msg_ptr) if registered else None, emit))

    def submit_batch(self, msgs, sigs, pubs, want_tags=False, want_keep=False, emit=None):
        """verify_batch (lists of bytes-like) as a submission: staged, every
        byte copied before it returns.  Returns the ticket.  want_keep, emit:
        as submit_batch_ptrs."""
        n = len(msgs)
        keep = [bytes(m) for m in msgs] + [bytes(s) for s in sigs] + [bytes(p) for p in pubs]
        bufs = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in keep]
        addr = np.array([ctypes.addressof(b) for b in bufs], np.uint64)
        return self.submit_batch_ptrs(addr[2 * n:], addr[n:2 * n], addr[:n], [len(b) for b in keep[:n]],
                                      want_tags=want_tags, registered=False, want_keep=want_keep, emit=emit)

    def submit_frags(self, mcache, region, seq0, n, frag_max=FRAG_MAX_DEFAULT, want_tags=False, want_keep=False, emit=None):
        """fd_ed25519_amd_submit_frags: items (seq0, n) of the frag source
        (mcache, region: each inside one host_register registration) as one
        submission; the GPU reads the lines (module function frags is the
        rule).  Returns the ticket; the lines, the frags and the registrations
        must stay valid until delivery.  The delivered result is what
        submit_batch_ptrs delivers: err (VERDICT_FRAG_SEQ / VERDICT_FRAG_BAD
        for an item without a frag), with want_tags the tags (0 for those),
        with want_keep keep, with emit (a uint8 array of at least n *
        emit_bound(frag_max - 96) bytes) also (emit_off, emit_sz)."""
        n = int(n)
        src = frag_src(mcache, region, frag_max)
        err = np.zeros(max(n, 1), np.int8)
        tags = np.zeros(max(n, 1), np.uint64) if want_tags else None
        k = _Keep(n, want_keep, emit)
        t = ctypes.c_ulong(0)
        ea = k.args() if emit is not None else k.args() + (None, 0, None, None)
        rc = lib().fd_ed25519_amd_submit_frags(self._h, ctypes.byref(src), int(seq0) & 0xFFFFFFFFFFFFFFFF, n, _ptr(err),
                                               _ptr(tags) if want_tags else None, *ea, ctypes.byref(t))
        if want_keep:
            finish = lambda: ((err[:n], tags[:n]) if want_tags else (err[:n],)) + k.results()
        else:
            finish = lambda: (err[:n], tags[:n]) if want_tags else err[:n]
        return self._submitted("fd_ed25519_amd_submit_frags", rc, t, finish, (mcache, region, emit))

    def submit_txns_ptrs(self, txn_ptr, txn_sz, want_sigs=False, want_tags=False, want_desc=False, registered=True,
                         want_keep=False, emit=None, want_budget=False):
        """fd_ed25519_amd_submit_txns_registered: verify_txns_ptrs as one
        chunk, launched now and delivered by poll() / wait(); the payloads must
        stay valid until then.  registered=False: the payloads are copied here
        and go through fd_ed25519_amd_submit_txns (submit_txns).  Returns the
        ticket.  want_keep (fd_ed25519_amd_submit_txns_registered_keep): the
        delivered tuple ends with keep, the uint32 indices of the surviving
        transactions, ascending; with want_desc the descriptors are then those
        of the survivors only.  emit (the _emit form, with want_keep): as
        submit_batch_ptrs, at least the sum of txn_emit_bound(txn_sz) bytes;
        the frames are module function txn_emit's.  want_budget (the _budget
        form): the delivered tuple ends with the BUDGET_DTYPE records of all
        the transactions (module function txn_budget), behind everything else."""
        tp = np.ascontiguousarray(txn_ptr, np.uint64)
        sz = np.ascontiguousarray(txn_sz, np.uint64)
        n = int(tp.size)
        assert sz.size == n
        if ((tp == 0) & (sz != 0)).any():
            raise EngineError("submit_txns_ptrs: NULL payload pointer with a size")
        if not registered:
            pays = [ctypes.string_at(int(p), int(z)) if z else b"" for p, z in zip(tp.tolist(), sz.tolist())]
            off = np.concatenate(([0], np.cumsum(sz)[:-1])).astype(np.uint32) if n else np.zeros(0, np.uint32)
            return self.submit_txns(np.frombuffer(b"".join(pays), np.uint8), off, sz.astype(np.uint32),
                                    want_sigs=want_sigs, want_tags=want_tags, want_desc=want_desc, want_keep=want_keep,
                                    emit=emit, want_budget=want_budget)
        base, tot = txn_slots_ptrs(tp, sz) if (want_sigs or want_tags) else (None, 0)
        o = _TxnOutputs(n, sz, base, tot, want_sigs, want_tags, want_desc, want_keep, emit, want_budget)
        t = ctypes.c_ulong(0)
        name = "fd_ed25519_amd_submit_txns_registered" + o.suffix
        rc = getattr(lib(), name)(self._h, n, _ptr(tp), _ptr(sz), *o.args(), ctypes.byref(t))
        return self._submitted(name, rc, t, o.result, (txn_ptr, emit))

    def submit_txns(self, payload, txn_off, txn_sz, want_sigs=False, want_tags=False, want_desc=False, want_keep=False,
                    emit=None, want_budget=False):
        """fd_ed25519_amd_submit_txns: verify_txns as one chunk, the payload
        bytes copied before it returns, delivered by poll() / wait().  Returns
        the ticket.  want_keep (fd_ed25519_amd_submit_txns_keep), emit
        (fd_ed25519_amd_submit_txns_emit), want_budget
        (fd_ed25519_amd_submit_txns_budget): as submit_txns_ptrs."""
        payload = np.ascontiguousarray(payload, np.uint8)
        off = np.ascontiguousarray(txn_off, np.uint32)
        sz = np.ascontiguousarray(txn_sz, np.uint32)
        n = int(off.size)
        base, tot = txn_slots(payload, off, sz) if (want_sigs or want_tags) else (None, 0)
        o = _TxnOutputs(n, sz, base, tot, want_sigs, want_tags, want_desc, want_keep, emit, want_budget)
        t = ctypes.c_ulong(0)
        name = "fd_ed25519_amd_submit_txns" + o.suffix
        rc = getattr(lib(), name)(self._h, n, _ptr(payload), _ptr(off), _ptr(sz), int(payload.size), *o.args(), ctypes.byref(t))
        return self._submitted(name, rc, t, o.result, emit)

    def _collect(self, name):
        t = ctypes.c_ulong(0)
        rc = getattr(lib(), name)(self._h, ctypes.byref(t))
        if rc == ASYNC_NONE:
            return None
        finish, _ = self._pending.pop(int(t.value), (None, None))
        if rc:
            if not self.in_flight:        # a runtime error dropped every submission in flight
                self._pending.clear()
            raise EngineError("%s rc=%d (ticket %d)" % (name, rc, t.value))
        return int(t.value), finish() if finish else None    # None: submitted through the C call directly

    def poll(self):
        """fd_ed25519_amd_async_poll: None when nothing is in flight or the
        oldest submission has not finished; else (ticket, outputs), outputs
        being what the synchronous method returns.  Never blocks."""
        return self._collect("fd_ed25519_amd_async_poll")

    def wait(self):
        """fd_ed25519_amd_async_wait: poll() that blocks for the oldest
        submission; None only when nothing is in flight."""
        return self._collect("fd_ed25519_amd_async_wait")

    # ------------------------------------------------------------ synchronous calls

    def verify_soa(self, pub, sig, msg_off, msg_sz, blob, want_tags=False):
        """want_tags: returns (err, tag), tag uint64 (n,): the dedup tags
        (fd_ed25519_amd_verify_soa_tag; see tag())."""
        pub = np.ascontiguousarray(pub, np.uint8)
        sig = np.ascontiguousarray(sig, np.uint8)
        off = np.ascontiguousarray(msg_off, np.uint32)
        sz = np.ascontiguousarray(msg_sz, np.uint32)
        blob = np.ascontiguousarray(blob, np.uint8)
        n = int(pub.shape[0])
        err = np.zeros(n, np.int8)
        if want_tags:
            tags = np.zeros(n, np.uint64)
            rc = lib().fd_ed25519_amd_verify_soa_tag(self._h, n, _ptr(pub), _ptr(sig), _ptr(off), _ptr(sz),
                                                     _ptr(blob), int(blob.size), _ptr(err), _ptr(tags))
        else:
            rc = lib().fd_ed25519_amd_verify_soa(self._h, n, _ptr(pub), _ptr(sig), _ptr(off), _ptr(sz),
                                                 _ptr(blob), int(blob.size), _ptr(err))
        if rc:
            raise EngineError("fd_ed25519_amd_verify_soa rc=%d" % rc)
        return (err, tags) if want_tags else err

    def verify_soa_registered(self, pub, sig, msg_off, msg_sz, blob, err=None, want_tags=False):
        """fd_ed25519_amd_verify_soa_registered: every plane must lie in memory
        registered with host_register (see RegisteredPlanes); no host copy.
        want_tags: returns (err, tag) as verify_soa (the outputs are plain
        memory)."""
        n = int(pub.shape[0])
        if err is None:
            err = np.zeros(n, np.int8)
        if want_tags:
            tags = np.zeros(n, np.uint64)
            rc = lib().fd_ed25519_amd_verify_soa_registered_tag(self._h, n, _ptr(pub), _ptr(sig), _ptr(msg_off),
                                                                _ptr(msg_sz), _ptr(blob), int(blob.size), _ptr(err),
                                                                _ptr(tags))
        else:
            rc = lib().fd_ed25519_amd_verify_soa_registered(self._h, n, _ptr(pub), _ptr(sig), _ptr(msg_off),
                                                            _ptr(msg_sz), _ptr(blob), int(blob.size), _ptr(err))
        if rc:
            raise EngineError("fd_ed25519_amd_verify_soa_registered rc=%d" % rc)
        return (err, tags) if want_tags else err

    def verify_batch(self, msgs, sigs, pubs, want_tags=False):
        """Pointer-array form: lists of bytes-like.  want_tags: (err, tag)."""
        n = len(msgs)
        keep = [bytes(m) for m in msgs] + [bytes(s) for s in sigs] + [bytes(p) for p in pubs]
        bufs = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in keep]
        mp = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs[:n]])
        sp = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs[n:2 * n]])
        pp = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs[2 * n:]])
        sz = (ctypes.c_ulong * max(n, 1))(*[len(b) for b in keep[:n]])
        err = np.zeros(max(n, 1), np.int8)
        if want_tags:
            tags = np.zeros(max(n, 1), np.uint64)
            rc = lib().fd_ed25519_amd_verify_batch_tag(self._h, n, mp, sz, sp, pp, _ptr(err), _ptr(tags))
        else:
            rc = lib().fd_ed25519_amd_verify_batch(self._h, n, mp, sz, sp, pp, _ptr(err))
        if rc:
            raise EngineError("fd_ed25519_amd_verify_batch rc=%d" % rc)
        return (err[:n], tags[:n]) if want_tags else err[:n]

    def verify_batch_ptrs(self, pub_ptr, sig_ptr, msg_ptr, msg_sz, want_tags=False, err=None, tags=None):
        """fd_ed25519_amd_verify_batch_registered: the pointer-array batch
        with no host staging.  pub_ptr, sig_ptr, msg_ptr: uint64 arrays of
        host addresses (32, 64 and msg_sz[i] bytes behind them, any
        alignment), every range inside one host_register registration; the
        GPU fetches the bytes itself.  want_tags: (err, tag).  err / tags:
        preallocated outputs (int8 / uint64, n entries); an EngineError
        leaves them untouched."""
        pp = np.ascontiguousarray(pub_ptr, np.uint64)
        sp = np.ascontiguousarray(sig_ptr, np.uint64)
        mp = np.ascontiguousarray(msg_ptr, np.uint64)
        sz = np.ascontiguousarray(msg_sz, np.uint64)
        n = int(pp.size)
        assert sp.size == n and mp.size == n and sz.size == n
        if err is None:
            err = np.zeros(max(n, 1), np.int8)
        if want_tags:
            if tags is None:
                tags = np.zeros(max(n, 1), np.uint64)
            rc = lib().fd_ed25519_amd_verify_batch_registered_tag(self._h, n, _ptr(mp), _ptr(sz), _ptr(sp), _ptr(pp),
                                                                  _ptr(err), _ptr(tags))
        else:
            rc = lib().fd_ed25519_amd_verify_batch_registered(self._h, n, _ptr(mp), _ptr(sz), _ptr(sp), _ptr(pp), _ptr(err))
        if rc:
            raise EngineError("fd_ed25519_amd_verify_batch_registered rc=%d" % rc)
        return (err[:n], tags[:n]) if want_tags else err[:n]

    def verify_batch_registered(self, arena, pub_off, sig_off, msg_off, msg_sz, want_tags=False):
        """verify_batch_ptrs over one registered uint8 arena (host_register):
        signature i has its key at arena[pub_off[i]], its signature at
        arena[sig_off[i]] and its message at arena[msg_off[i] : + msg_sz[i]]."""
        assert arena.dtype == np.uint8 and arena.flags["C_CONTIGUOUS"]
        base = np.uint64(arena.ctypes.data)
        return self.verify_batch_ptrs(base + np.asarray(pub_off, np.uint64), base + np.asarray(sig_off, np.uint64),
                                      base + np.asarray(msg_off, np.uint64), msg_sz, want_tags=want_tags)

    def verify_txns(self, payload, txn_off, txn_sz, want_sigs=False, want_tags=False, want_desc=False, want_budget=False):
        """Wire-format transaction batch (include/fd_txn_amd.h): parse on the
        GPU, verify every signature (multi-signer rule), one verdict per
        transaction in {0, -1, -2, -3, FD_TXN_AMD_ERR_PARSE}.  With
        want_sigs, also returns (sig_base, sig_err); with want_tags the
        tuple ends with (txn_tag, sig_tag): uint64 per transaction (its
        first signature's dedup tag, 0 where it did not parse) and per
        signature slot (the numbering of sig_err / txn_slots).  With
        want_desc (fd_ed25519_amd_verify_txns_desc) the tuple ends with
        (desc_off, desc): uint64[n+1] offsets and the uint8[desc_off[-1]]
        packed fd_txn_t descriptors of the transactions that parse; the
        buffer is sized with txn_desc_bound.  With want_budget
        (fd_ed25519_amd_verify_txns_budget) the tuple ends with the
        BUDGET_DTYPE records of all the transactions (txn_budget)."""
        return _verify_txns("fd_ed25519_amd_verify_txns", self._h, payload, txn_off, txn_sz, want_sigs, want_tags, want_desc,
                            want_budget)

    def verify_txns_ptrs(self, txn_ptr, txn_sz, want_sigs=False, want_tags=False, want_desc=False, want_budget=False):
        """fd_ed25519_amd_verify_txns_registered: the transaction batch in
        pointer-array form with no host staging.  txn_ptr: uint64 array of
        host addresses (txn_sz[t] payload bytes behind each, any alignment),
        every non-empty range inside one host_register registration; the GPU
        fetches the payloads itself.  Returns what verify_txns returns for
        the same payloads (want_desc: fd_ed25519_amd_verify_txns_registered_desc;
        want_budget: fd_ed25519_amd_verify_txns_registered_budget)."""
        tp = np.ascontiguousarray(txn_ptr, np.uint64)
        sz = np.ascontiguousarray(txn_sz, np.uint64)
        n = int(tp.size)
        assert sz.size == n
        if ((tp == 0) & (sz != 0)).any():     # refused by the library too; the slot count below would read the bytes
            raise EngineError("verify_txns_ptrs: NULL payload pointer with a size")
        terr = np.zeros(max(n, 1), np.int8)
        base = serr = None
        if want_sigs or want_tags:
            base, tot = txn_slots_ptrs(tp, sz)
        if want_sigs:
            serr = np.zeros(max(tot, 1), np.int8)
        args = (self._h, n, _ptr(tp), _ptr(sz), _ptr(terr), _ptr(base) if base is not None else None,
                _ptr(serr) if want_sigs else None)
        ttag = stag = None
        if want_tags:
            ttag, stag = np.zeros(max(n, 1), np.uint64), np.zeros(max(tot, 1), np.uint64)
        doff = desc = None
        if want_desc:
            doff, desc = _desc_buffers(sz)
        if want_budget:
            budget = np.zeros(max(n, 1), BUDGET_DTYPE)
            rc = lib().fd_ed25519_amd_verify_txns_registered_budget(*args, _ptr(ttag) if want_tags else None,
                                                                    _ptr(stag) if want_tags else None,
                                                                    _ptr(doff) if want_desc else None,
                                                                    _ptr(desc) if want_desc else None,
                                                                    int(desc.size) if want_desc else 0, _ptr(budget))
        elif want_desc:
            rc = lib().fd_ed25519_amd_verify_txns_registered_desc(*args, _ptr(ttag) if want_tags else None,
                                                                  _ptr(stag) if want_tags else None, _ptr(doff), _ptr(desc),
                                                                  int(desc.size))
        elif want_tags:
            rc = lib().fd_ed25519_amd_verify_txns_registered_tag(*args, _ptr(ttag), _ptr(stag))
        else:
            rc = lib().fd_ed25519_amd_verify_txns_registered(*args)
        if rc:
            raise EngineError("fd_ed25519_amd_verify_txns_registered rc=%d" % rc)
        out = (terr[:n],)
        if want_sigs:
            out += (base, serr[:int(base[-1])])
        if want_tags:
            out += (ttag[:n], stag[:int(base[-1])])
        if want_desc:
            out += (doff, desc[:int(doff[-1])])
        if want_budget:
            out += (budget[:n],)
        return out if len(out) > 1 else out[0]

    def verify_txns_registered(self, arena, txn_off, txn_sz, want_sigs=False, want_tags=False, want_desc=False,
                               want_budget=False):
        """verify_txns_ptrs over one registered uint8 arena (host_register):
        transaction t is arena[txn_off[t] : + txn_sz[t]]."""
        assert arena.dtype == np.uint8 and arena.flags["C_CONTIGUOUS"]
        base = np.uint64(arena.ctypes.data)
        return self.verify_txns_ptrs(base + np.asarray(txn_off, np.uint64), txn_sz, want_sigs=want_sigs,
                                     want_tags=want_tags, want_desc=want_desc, want_budget=want_budget)


class _TxnOutputs:
    """The output arrays of one transaction submission, alive until it is
    delivered: args() is the (txn_err .. desc_cap) run of the submit calls'
    arguments (want_keep: and keep, keep_cnt of the _keep forms; emit: and
    the four of the _emit forms), result() what verify_txns returns once they
    are filled (want_keep: and keep; emit: and (emit_off, emit_sz)); suffix:
    the submit call's ("", "_keep", "_emit" or "_budget").  want_budget: the
    _budget form, whose arguments are the _emit form's and the record array,
    which result() appends behind everything else."""

    def __init__(self, n, txn_sz, base, tot, want_sigs, want_tags, want_desc, want_keep=False, emit=None, want_budget=False):
        self.n, self.base, self.want = n, base, (want_sigs, want_tags, want_desc)
        self.k = _Keep(n, want_keep, emit) if (want_keep or emit is not None) else None
        self.suffix = "_budget" if want_budget else (self.k.suffix if self.k else "")
        self.budget = np.zeros(max(n, 1), BUDGET_DTYPE) if want_budget else None
        self.terr = np.zeros(max(n, 1), np.int8)
        self.serr = np.zeros(max(tot, 1), np.int8) if want_sigs else None
        self.ttag = np.zeros(max(n, 1), np.uint64) if want_tags else None
        self.stag = np.zeros(max(tot, 1), np.uint64) if want_tags else None
        self.doff, self.desc = _desc_buffers(txn_sz) if want_desc else (None, None)

    def args(self):
        p = lambda a: _ptr(a) if a is not None else None
        return (p(self.terr), p(self.base), p(self.serr), p(self.ttag), p(self.stag), p(self.doff), p(self.desc),
                int(self.desc.size) if self.desc is not None else 0) + self._tail()

    def _tail(self):
        if self.budget is None:
            return self.k.args() if self.k else ()
        k = self.k.args() if self.k else (None, None)              # keep, keep_cnt
        k += (None, 0, None, None) if len(k) == 2 else ()          # out, out_cap, emit_off, emit_sz
        return k + (_ptr(self.budget),)

    def result(self):
        want_sigs, want_tags, want_desc = self.want
        out = (self.terr[:self.n],)
        if want_sigs:
            out += (self.base, self.serr[:int(self.base[-1])])
        if want_tags:
            out += (self.ttag[:self.n], self.stag[:int(self.base[-1])])
        if want_desc:
            out += (self.doff, self.desc[:int(self.doff[-1])])
        if self.k:
            out += self.k.results()
        if self.budget is not None:
            out += (self.budget[:self.n],)
        return out if len(out) > 1 else out[0]


# fd_txn_amd_budget_t (include/fd_txn_amd.h, "Compute budget"): 24 bytes, little endian
BUDGET_DTYPE = np.dtype([("rewards", "<u8"), ("compute", "<u4"), ("heap_sz", "<u4"), ("flags", "<u2"),
                         ("cb_instr_cnt", "<u2"), ("status", "<u4")])
BUDGET_OK, BUDGET_INVALID, BUDGET_NOPARSE = 0, 1, 2


def txn_budget(payload, desc):
    """fd_txn_amd_budget: the compute budget rule on the host (no device) for
    one payload and its fd_txn_t descriptor bytes as fd_txn_parse or the
    _desc calls return them (None or empty: the payload did not parse).
    Returns a BUDGET_DTYPE scalar."""
    p = np.frombuffer(bytes(payload), np.uint8)
    d = np.frombuffer(bytes(desc), np.uint8) if desc is not None and len(desc) else None
    out = np.zeros(1, BUDGET_DTYPE)
    lib().fd_txn_amd_budget(_ptr(p), int(p.size), _ptr(d) if d is not None else None, _ptr(out))
    return out[0]


def txn_budget_dev(txn_cnt, d_payload, d_toff, d_tsz, d_fp, d_budget, stream=0):
    """fd_txn_amd_budget_dev: the compute budget records alone,
    device-resident, from the payload planes and the footprint plane
    txn_parse_dev left; d_budget: 24 * txn_cnt bytes, 8-aligned.  Enqueued on
    `stream`, no sync."""
    rc = lib().fd_txn_amd_budget_dev(int(txn_cnt), d_payload, d_toff, d_tsz, d_fp, d_budget, stream)
    if rc:
        raise EngineError("fd_txn_amd_budget_dev rc=%d" % rc)


def txn_desc_bound(sz):
    """fd_txn_amd_desc_bound: an upper bound on the fd_txn_t footprint of any
    payload of sz bytes (0 where no payload of that size parses; no device)."""
    return int(lib().fd_txn_amd_desc_bound(int(sz)))


def _desc_buffers(txn_sz):
    """(desc_off, desc) for a batch with these payload sizes: desc holds the
    sum of txn_desc_bound, the capacity the _desc calls ask for (at least one
    byte: the calls take no NULL desc)."""
    bound = lib().fd_txn_amd_desc_bound
    by_sz = {int(z): int(bound(int(z))) for z in np.unique(txn_sz)}
    cap = sum(by_sz[int(z)] for z in np.asarray(txn_sz).tolist())
    return np.zeros(len(txn_sz) + 1, np.uint64), np.zeros(max(cap, 1), np.uint8)


def txn_slots_ptrs(txn_ptr, txn_sz):
    """fd_ed25519_amd_txn_slots_ptrs: (tbase[txn_cnt+1], total signature slots)
    of a pointer-array batch; reads the first byte behind every pointer with
    a size (no device)."""
    tp = np.ascontiguousarray(txn_ptr, np.uint64)
    sz = np.ascontiguousarray(txn_sz, np.uint64)
    assert tp.size == sz.size
    base = np.zeros(tp.size + 1, np.uint32)
    tot = lib().fd_ed25519_amd_txn_slots_ptrs(int(tp.size), _ptr(tp), _ptr(sz), _ptr(base))
    return base, int(tot)


def txn_gather_layout(sz, slots, cap, blob_cap):
    """Python mirror of fd_ed25519_amd_txn_gather_layout: how
    verify_txns_registered sizes one chunk.  Of the payload sizes sz with
    signature-slot counts slots the chunk takes the first, always, and
    further ones while the count stays <= cap, the slot total stays <= cap
    and the padded byte total, the sum of the sizes rounded up to 16, stays
    <= blob_cap.  Returns (count, dst, slot_cnt): dst uint32 (count,), each
    payload's offset in the chunk's blob."""
    dst, b, ns = [], 0, 0
    for s, k in zip(sz, slots):
        s, k = int(s), int(k)
        pad = (s + 15) & ~15
        if dst and (len(dst) >= cap or ns + k > cap or s > blob_cap or b + pad > blob_cap):
            break
        dst.append(b)
        b += pad
        ns += k
    return len(dst), np.asarray(dst, np.uint32), ns


def txn_gather_layout_c(sz, slots, cap, blob_cap):
    """fd_ed25519_amd_txn_gather_layout itself (the library's; no device)."""
    sz = np.ascontiguousarray(sz, np.uint64)
    slots = np.ascontiguousarray(slots, np.uint32)
    assert sz.size == slots.size
    dst = np.zeros(max(sz.size, 1), np.uint32)
    ns = ctypes.c_ulong(0)
    c = int(lib().fd_ed25519_amd_txn_gather_layout(int(sz.size), _ptr(sz), _ptr(slots), int(cap), int(blob_cap),
                                                   _ptr(dst), ctypes.byref(ns)))
    return c, dst[:c], int(ns.value)


def txn_slots(payload, txn_off, txn_sz):
    """fd_ed25519_amd_txn_slots: (tbase[txn_cnt+1], total signature slots)."""
    payload = np.ascontiguousarray(payload, np.uint8)
    off = np.ascontiguousarray(txn_off, np.uint32)
    sz = np.ascontiguousarray(txn_sz, np.uint32)
    base = np.zeros(off.size + 1, np.uint32)
    tot = lib().fd_ed25519_amd_txn_slots(int(off.size), _ptr(payload), _ptr(off), _ptr(sz), _ptr(base))
    return base, int(tot)


def _verify_txns(name, h, payload, txn_off, txn_sz, want_sigs, want_tags=False, want_desc=False, want_budget=False):
    """name: fd_ed25519_amd_verify_txns or the multi form; want_tags calls its
    _tag form, want_desc its _desc form, want_budget its _budget form (the
    last two: the single-device call only)."""
    payload = np.ascontiguousarray(payload, np.uint8)
    off = np.ascontiguousarray(txn_off, np.uint32)
    sz = np.ascontiguousarray(txn_sz, np.uint32)
    n = int(off.size)
    terr = np.zeros(max(n, 1), np.int8)
    base = serr = None
    if want_sigs or want_tags:
        # sig_err / sig_tag are sized by the engine's own slot rule (overlapping
        # or repeated txn_off entries reserve slots more than once)
        base, tot = txn_slots(payload, off, sz)
    if want_sigs:
        serr = np.zeros(max(tot, 1), np.int8)
    args = (h, n, _ptr(payload), _ptr(off), _ptr(sz), int(payload.size), _ptr(terr),
            _ptr(base) if base is not None else None, _ptr(serr) if want_sigs else None)
    ttag = stag = None
    if want_tags:
        ttag, stag = np.zeros(max(n, 1), np.uint64), np.zeros(max(tot, 1), np.uint64)
    doff = desc = None
    if want_desc:
        doff, desc = _desc_buffers(sz)
    if want_budget:
        budget = np.zeros(max(n, 1), BUDGET_DTYPE)
        rc = getattr(lib(), name + "_budget")(*args, _ptr(ttag) if want_tags else None, _ptr(stag) if want_tags else None,
                                              _ptr(doff) if want_desc else None, _ptr(desc) if want_desc else None,
                                              int(desc.size) if want_desc else 0, _ptr(budget))
    elif want_desc:
        rc = getattr(lib(), name + "_desc")(*args, _ptr(ttag) if want_tags else None, _ptr(stag) if want_tags else None,
                                            _ptr(doff), _ptr(desc), int(desc.size))
    elif want_tags:
        rc = getattr(lib(), name + "_tag")(*args, _ptr(ttag), _ptr(stag))
    else:
        rc = getattr(lib(), name)(*args)
    if rc:
        raise EngineError("verify_txns rc=%d" % rc)
    out = (terr[:n],)
    if want_sigs:
        out += (base, serr[:int(base[-1])])
    if want_tags:
        out += (ttag[:n], stag[:int(base[-1])])
    if want_desc:
        out += (doff, desc[:int(doff[-1])])
    if want_budget:
        out += (budget[:n],)
    return out if len(out) > 1 else out[0]


def gather_layout(sz, cap, blob_cap):
    """Python mirror of fd_ed25519_amd_gather_layout: how
    verify_batch_registered sizes one chunk.  Of the message sizes sz the chunk
    takes the first, always, and further ones while the count stays <= cap and
    the padded total, the sum of the sizes rounded up to 16, stays <=
    blob_cap.  Returns (count, dst): dst uint32 (count,), each message's
    offset in the chunk's blob."""
    dst, b = [], 0
    for s in sz:
        s = int(s)
        pad = (s + 15) & ~15
        if dst and (len(dst) >= cap or s > blob_cap or b + pad > blob_cap):
            break
        dst.append(b)
        b += pad
    return len(dst), np.asarray(dst, np.uint32)


def gather_layout_c(sz, cap, blob_cap):
    """fd_ed25519_amd_gather_layout itself (the library's; no device)."""
    sz = np.ascontiguousarray(sz, np.uint64)
    dst = np.zeros(max(sz.size, 1), np.uint32)
    c = int(lib().fd_ed25519_amd_gather_layout(int(sz.size), _ptr(sz), int(cap), int(blob_cap), _ptr(dst)))
    return c, dst[:c]


def shard_range(n, ndev, r):
    """fd_ed25519_amd_shard_range: engine r's contiguous shard [lo, hi) of n."""
    lo, hi = ctypes.c_ulong(), ctypes.c_ulong()
    lib().fd_ed25519_amd_shard_range(int(n), int(ndev), int(r), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


class MultiEngine:
    """fd_ed25519_amd_multi_t: one engine + one persistent host thread per
    entry of `devices` (repeats allowed); a batch is split into contiguous
    shards verified concurrently, no collective.  mode: as Engine's, for
    every engine."""

    def __init__(self, devices, batch_max=1 << 16, blob_max=None, mode=MODE_REFERENCE):
        _check_mode(mode)
        if blob_max is None:
            blob_max = max(batch_max * 256, MSG_MAX)
        dv = np.ascontiguousarray(devices, np.int32)
        self._h = lib().fd_ed25519_amd_multi_new(_ptr(dv), int(dv.size), int(batch_max), int(blob_max))
        if not self._h:
            raise EngineError("fd_ed25519_amd_multi_new(%r) failed" % (list(devices),))
        self.ndev = int(lib().fd_ed25519_amd_multi_ndev(self._h))
        if mode != MODE_REFERENCE:
            self.set_mode(mode)

    def set_mode(self, mode):
        rc = lib().fd_ed25519_amd_multi_set_mode(self._h, int(mode))
        if rc:
            raise EngineError("fd_ed25519_amd_multi_set_mode(%r) rc=%d" % (mode, rc))

    def close(self):
        if self._h:
            lib().fd_ed25519_amd_multi_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify_soa(self, pub, sig, msg_off, msg_sz, blob, want_tags=False):
        """want_tags: (err, tag) as Engine.verify_soa, every shard's tags at its offset."""
        pub = np.ascontiguousarray(pub, np.uint8)
        sig = np.ascontiguousarray(sig, np.uint8)
        off = np.ascontiguousarray(msg_off, np.uint32)
        sz = np.ascontiguousarray(msg_sz, np.uint32)
        blob = np.ascontiguousarray(blob, np.uint8)
        n = int(pub.shape[0])
        err = np.zeros(max(n, 1), np.int8)
        if want_tags:
            tags = np.zeros(max(n, 1), np.uint64)
            rc = lib().fd_ed25519_amd_multi_verify_soa_tag(self._h, n, _ptr(pub), _ptr(sig), _ptr(off), _ptr(sz),
                                                           _ptr(blob), int(blob.size), _ptr(err), _ptr(tags))
        else:
            rc = lib().fd_ed25519_amd_multi_verify_soa(self._h, n, _ptr(pub), _ptr(sig), _ptr(off), _ptr(sz), _ptr(blob),
                                                       int(blob.size), _ptr(err))
        if rc:
            raise EngineError("fd_ed25519_amd_multi_verify_soa rc=%d" % rc)
        return (err[:n], tags[:n]) if want_tags else err[:n]

    def verify_txns(self, payload, txn_off, txn_sz, want_sigs=False, want_tags=False):
        return _verify_txns("fd_ed25519_amd_multi_verify_txns", self._h, payload, txn_off, txn_sz, want_sigs, want_tags)


class RegisteredPlanes:
    """Page-aligned copies of numpy arrays, registered with
    fd_ed25519_amd_host_register (inputs of Engine.verify_soa_registered);
    planes[k] is the registered copy of arrays[k].  close() unregisters."""

    def __init__(self, *arrays):
        self._raw = []
        self.planes = []
        for a in arrays:
            a = np.ascontiguousarray(a)
            nb = (max(a.nbytes, 1) + 4095) & ~4095
            raw = np.zeros(nb + 4096, np.uint8)
            o = (-raw.ctypes.data) % 4096
            region = raw[o:o + nb]
            b = region[:a.nbytes].view(a.dtype).reshape(a.shape)
            b[...] = a
            host_register(region)
            self._raw.append(region)
            self.planes.append(b)

    def __getitem__(self, k):
        return self.planes[k]

    def close(self):
        for r in self._raw:
            host_unregister(r)
        self._raw = []


def host_register(arr):
    """Pin a numpy array's memory for fd_ed25519_amd_verify_soa_registered."""
    rc = lib().fd_ed25519_amd_host_register(_ptr(arr), int(arr.nbytes))
    if rc:
        raise EngineError("fd_ed25519_amd_host_register rc=%d" % rc)


def host_unregister(arr):
    rc = lib().fd_ed25519_amd_host_unregister(_ptr(arr))
    if rc:
        raise EngineError("fd_ed25519_amd_host_unregister rc=%d" % rc)


# ---------------------------------------------------------------- device-resident path

def workspace_footprint(n):
    return int(lib().fd_ed25519_amd_workspace_footprint(int(n)))


WS_PLANES = ("dig", "evn", "top", "A", "R", "Ai", "st", "tag", "ds", "init", "ctr")   # FD_ED25519_AMD_WS_DIG ..


def debug_ws_layout(n):
    """fd_ed25519_amd_debug_ws_layout (host only, no device): {"N": rows,
    plane name: byte offset for each of WS_PLANES, "total": the footprint}
    of an n-signature workspace."""
    out = (ctypes.c_ulong * (len(WS_PLANES) + 2))()
    lib().fd_ed25519_amd_debug_ws_layout(int(n), out)
    return dict(zip(("N",) + WS_PLANES + ("total",), (int(v) for v in out)))


def verify_dev(n, d_pub, d_sig, d_off, d_sz, d_blob, d_err, d_ws, stream=0, mode=MODE_REFERENCE):
    """All arguments are device pointers (ints, e.g. torch tensor .data_ptr());
    enqueued on `stream` (hipStream_t as int), not synchronised.  mode:
    MODE_REFERENCE or MODE_STRICT (fd_ed25519_amd_verify_dev_mode)."""
    if mode == MODE_REFERENCE:
        rc = lib().fd_ed25519_amd_verify_dev(int(n), d_pub, d_sig, d_off, d_sz, d_blob, d_err, d_ws, stream)
    else:
        rc = lib().fd_ed25519_amd_verify_dev_mode(int(n), d_pub, d_sig, d_off, d_sz, d_blob, d_err, d_ws, stream,
                                                  int(mode))
    if rc:
        raise EngineError("fd_ed25519_amd_verify_dev rc=%d" % rc)


def verify_dev_ev(n, d_pub, d_sig, d_off, d_sz, d_blob, d_err, d_ws, stream, events, mode=MODE_REFERENCE):
    """verify_dev recording 4 HIP events (hip.Event) around/between the
    three kernels on `stream` (strict mode: k_strict runs before the last)."""
    arr = None
    if events is not None:
        arr = (ctypes.c_void_p * 4)(*[e.handle for e in events])
    if mode == MODE_REFERENCE:
        rc = lib().fd_ed25519_amd_verify_dev_ev(int(n), d_pub, d_sig, d_off, d_sz, d_blob, d_err, d_ws, stream, arr)
    else:
        rc = lib().fd_ed25519_amd_verify_dev_ev_mode(int(n), d_pub, d_sig, d_off, d_sz, d_blob, d_err, d_ws, stream,
                                                     arr, int(mode))
    if rc:
        raise EngineError("fd_ed25519_amd_verify_dev_ev rc=%d" % rc)


def verify_txns_dev(txn_cnt, slot_cnt, d_payload, d_txn_off, d_txn_sz, d_tbase, d_txn_err, d_sig_err, d_ws,
                    stream=0, mode=MODE_REFERENCE):
    """fd_ed25519_amd_verify_txns_dev_mode: the device-resident transaction
    batch (include/fd_txn_amd.h), device pointers as ints; d_sig_err may be
    0 / None.  Enqueued on `stream`, not synchronised."""
    rc = lib().fd_ed25519_amd_verify_txns_dev_mode(int(txn_cnt), int(slot_cnt), d_payload, d_txn_off, d_txn_sz,
                                                   d_tbase, d_txn_err, d_sig_err, d_ws, stream, int(mode))
    if rc:
        raise EngineError("fd_ed25519_amd_verify_txns_dev_mode rc=%d" % rc)


def work_stats_dev(n, d_ws, d_stats, stream=0):
    rc = lib().fd_ed25519_amd_work_stats_dev(int(n), d_ws, d_stats, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_work_stats_dev rc=%d" % rc)


def tags_dev(n, d_ws, d_tag, stream=0):
    """fd_ed25519_amd_tags_dev: the dedup tags (uint64 [n], device pointer)
    of the last verify_dev / verify_txns_dev call on workspace d_ws, in
    either mode.  Enqueued on `stream`, not synchronised."""
    rc = lib().fd_ed25519_amd_tags_dev(int(n), d_ws, d_tag, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_tags_dev rc=%d" % rc)


def keep_scratch_footprint(n):
    """fd_ed25519_amd_keep_scratch_footprint: device scratch bytes of keep_dev for n items."""
    return int(lib().fd_ed25519_amd_keep_scratch_footprint(int(n)))


def keep_dev(n, d_err, d_tag, d_keep, d_keep_cnt, d_scratch, salt=0, stream=0):
    """fd_ed25519_amd_keep_dev: the survivor filter alone, device-resident --
    d_keep[0 .. *d_keep_cnt) (uint32) = keep(err, tag) over the n verdicts
    d_err (int8) and tags d_tag (uint64: what tags_dev / txn_tags_dev
    produce), *d_keep_cnt (uint64) their number.  d_scratch: at least
    keep_scratch_footprint(n) bytes, 256-aligned, contents irrelevant.  No
    output depends on salt.  Enqueued on `stream`, not synchronised."""
    rc = lib().fd_ed25519_amd_keep_dev(int(n), d_err, d_tag, d_keep, d_keep_cnt, d_scratch, int(salt) & (2**64 - 1), stream)
    if rc:
        raise EngineError("fd_ed25519_amd_keep_dev rc=%d" % rc)


def emit_scratch_footprint(n):
    """fd_ed25519_amd_emit_scratch_footprint: device scratch bytes of emit_dev / txn_emit_dev for n items."""
    return int(lib().fd_ed25519_amd_emit_scratch_footprint(int(n)))


def emit_dev(n, d_pub, d_sig, d_off, d_sz, d_blob, d_keep, d_keep_cnt, d_out, out_cap, d_emit_off, d_emit_sz, d_scratch,
             stream=0):
    """fd_ed25519_amd_emit_dev: the output frames alone, device-resident --
    for j < min(*d_keep_cnt, n) the frame of item d_keep[j] (module function
    emit) at d_out + d_emit_off[j]; frame j is stored only if d_emit_off[j+1]
    <= out_cap, d_emit_off[0 .. cnt] and d_emit_sz[0 .. cnt) are complete
    either way.  The inputs are verify_dev's planes.  d_out: 64-aligned;
    d_scratch: at least emit_scratch_footprint(n) bytes, 256-aligned, contents
    irrelevant.  No sync."""
    rc = lib().fd_ed25519_amd_emit_dev(int(n), d_pub, d_sig, d_off, d_sz, d_blob, d_keep, d_keep_cnt, d_out, int(out_cap),
                                       d_emit_off, d_emit_sz, d_scratch, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_emit_dev rc=%d" % rc)


def txn_emit_dev(txn_cnt, d_payload, d_toff, d_tsz, d_desc_off, d_desc, d_keep, d_keep_cnt, d_out, out_cap, d_emit_off,
                 d_emit_sz, d_scratch, stream=0):
    """fd_txn_amd_emit_dev: emit_dev for transactions (module function
    txn_emit); d_desc_off / d_desc are what txn_parse_packed_dev left."""
    rc = lib().fd_txn_amd_emit_dev(int(txn_cnt), d_payload, d_toff, d_tsz, d_desc_off, d_desc, d_keep, d_keep_cnt, d_out,
                                   int(out_cap), d_emit_off, d_emit_sz, d_scratch, stream)
    if rc:
        raise EngineError("fd_txn_amd_emit_dev rc=%d" % rc)


def txn_tags_dev(txn_cnt, d_tbase, d_ws, d_txn_tag, stream=0):
    """fd_ed25519_amd_txn_tags_dev: per transaction the dedup tag of its
    first signature (0 where it did not parse), after verify_txns_dev on the
    same workspace and d_tbase."""
    rc = lib().fd_ed25519_amd_txn_tags_dev(int(txn_cnt), d_tbase, d_ws, d_txn_tag, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_txn_tags_dev rc=%d" % rc)


def debug_digits_dev(n, d_ws, d_dig, d_top, stream=0):
    rc = lib().fd_ed25519_amd_debug_digits_dev(int(n), d_ws, d_dig, d_top, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_debug_digits_dev rc=%d" % rc)


def debug_points_dev(n, d_ws, d_A, d_R, d_ds, stream=0):
    """Copy the decompression planes of the last device-resident call: d_A
    int32 [30][n] (-A.X, A.Y, -A.T), d_R int32 [20][n] (R.X, R.Y), d_ds uint8
    [n][2] (status of A / R)."""
    rc = lib().fd_ed25519_amd_debug_points_dev(int(n), d_ws, d_A, d_R, d_ds, stream)
    if rc != 0:
        raise EngineError("fd_ed25519_amd_debug_points_dev rc=%d" % rc)


def sign_dev(n, d_prv, d_off, d_sz, d_blob, d_pub, d_sig, stream=0):
    """GPU keygen + sign on device buffers (fd_ed25519_amd_sign_dev)."""
    rc = lib().fd_ed25519_amd_sign_dev(int(n), d_prv, d_off, d_sz, d_blob, d_pub, d_sig, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_sign_dev rc=%d" % rc)


def sign_batch_gpu(prv, blob, msg_off, msg_sz):
    """Host arrays in, (pub, sig) out, signed on the GPU (k_sign)."""
    from . import hip
    prv = np.ascontiguousarray(prv, np.uint8)
    n = prv.shape[0]
    if not n:
        return np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8)
    d = [hip.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in
         (prv, np.asarray(msg_off, np.uint32), np.asarray(msg_sz, np.uint32), np.asarray(blob, np.uint8))]
    d_pub, d_sig = hip.DeviceBuffer(32 * n), hip.DeviceBuffer(64 * n)
    st = hip.Stream()
    sign_dev(n, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d_pub.ptr, d_sig.ptr, st.handle)
    st.synchronize()
    return d_pub.to_array(np.uint8, 32 * n).reshape(n, 32), d_sig.to_array(np.uint8, 64 * n).reshape(n, 64)


def set_small_batch_max(n):
    """Batches of at most n signatures use the 4-lane latency kernel (k_dsm4)."""
    lib().fd_ed25519_amd_set_small_batch_max(int(n))


def set_latency_batch_max(n):
    """Batches of at most n signatures use the 8-lane latency kernel (k_dsm8)."""
    lib().fd_ed25519_amd_set_latency_batch_max(int(n))


def set_pool_batch_min(n):
    """Throughput batches of at least n signatures use the pooled kernel (k_dsmp)."""
    lib().fd_ed25519_amd_set_pool_batch_min(int(n))


VERDICT_DEVICE = -128   # FD_ED25519_AMD_VERDICT_DEVICE: k_dsmp's step guard tripped


def device_numa_node(device):
    """fd_ed25519_amd_device_numa_node: the NUMA node of HIP device `device` (-1 unknown)."""
    f = lib().fd_ed25519_amd_device_numa_node
    f.restype = ctypes.c_int
    return int(f(int(device)))


def debug_set_pool_iter_cap(cap):
    """Debug: cap k_dsmp's step guard at `cap` steps per wave (0 restores it)."""
    lib().fd_ed25519_amd_debug_set_pool_iter_cap(int(cap))


def debug_set_pool_waves(w):
    """Debug: launch k_dsmp with min(w, 8 per CU) waves whatever the batch size
    (0 restores the policy min(ceil(n / 64), 8 per CU))."""
    lib().fd_ed25519_amd_debug_set_pool_waves(int(w))


DSM_KINDS = {"default": 0, "k_dsm": 1, "k_dsm4": 2, "k_dsm8": 3, "k_dsmp": 4}   # FD_ED25519_AMD_DSM_*


def debug_rprime_dev(n, d_ws, kind, d_xyz, stream=0):
    """The R' = [s]B - [h]A that the last device-resident call parked in
    workspace d_ws: d_xyz int32 [30][n] (X | Y | Z limbs), read through the
    parking layout of DSM kernel `kind` (a select_dsm_kernel name; 'default'
    resolves by n under the thresholds set now, as the launch does).  A row is
    defined only where the multiply ran."""
    rc = lib().fd_ed25519_amd_debug_rprime_dev(int(n), d_ws, DSM_KINDS[kind], d_xyz, stream)
    if rc:
        raise EngineError("fd_ed25519_amd_debug_rprime_dev rc=%d" % rc)


def select_dsm_kernel(name):
    """Force one double-scalar-mult kernel for every batch size (tests):
    'k_dsm', 'k_dsmp', 'k_dsm4', 'k_dsm8'; 'default' restores the size rule."""
    big = (1 << 32) - 1
    small, lat, pool = {"k_dsm": (0, 0, big), "k_dsmp": (0, 0, 0), "k_dsm4": (big, 0, big),
                        "k_dsm8": (big, big, big),
                        "default": (SMALL_BATCH_MAX_DEFAULT, LATENCY_BATCH_MAX_DEFAULT, POOL_BATCH_MIN_DEFAULT)}[name]
    set_small_batch_max(small)
    set_latency_batch_max(lat)
    set_pool_batch_min(pool)


SMALL_BATCH_MAX_DEFAULT = 16384
LATENCY_BATCH_MAX_DEFAULT = 8192
POOL_BATCH_MIN_DEFAULT = 1 << 19   # k_dsmp from 2^19 signatures
FD_TXN_AMD_ERR_PARSE = -4
FD_TXN_MAX_SZ = 3570


def txn_parse_packed_scratch_footprint(txn_cnt):
    """fd_txn_amd_parse_packed_scratch_footprint (no device)."""
    return int(lib().fd_txn_amd_parse_packed_scratch_footprint(int(txn_cnt)))


def txn_parse_packed_dev(txn_cnt, d_payload, d_toff, d_tsz, d_fp, d_desc_off, d_desc, desc_cap, d_scratch, stream=0):
    """Device batch parse with packed descriptors (fd_txn_amd_parse_packed_dev):
    footprints, their 64-bit running sum d_desc_off[txn_cnt+1] and the
    descriptors end to end in d_desc[desc_cap]; device pointers as ints,
    d_scratch of txn_parse_packed_scratch_footprint(txn_cnt) bytes."""
    rc = lib().fd_txn_amd_parse_packed_dev(int(txn_cnt), d_payload, d_toff, d_tsz, d_fp, d_desc_off, d_desc, int(desc_cap),
                                           d_scratch, stream)
    if rc:
        raise EngineError("fd_txn_amd_parse_packed_dev rc=%d" % rc)


def txn_parse_dev(txn_cnt, d_payload, d_toff, d_tsz, d_fp, d_out=None, out_stride=0, stream=0):
    """Device batch parse (fd_txn_amd_parse_dev): footprints (and optionally
    fd_txn_t descriptors, out_stride apart) of txn_cnt wire transactions."""
    rc = lib().fd_txn_amd_parse_dev(int(txn_cnt), d_payload, d_toff, d_tsz, d_fp, d_out, int(out_stride), stream)
    if rc:
        raise EngineError("fd_txn_amd_parse_dev rc=%d" % rc)


def version():
    return lib().fd_ed25519_amd_version().decode()
