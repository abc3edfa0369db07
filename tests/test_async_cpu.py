"""CPU tests of the asynchronous submit / poll interface
(include/fd_ed25519_amd.h, "Asynchronous submissions"): the symbols and codes
are declared (tests/test_abi.py's export test then covers them), and the
argument checks that need no device come before any device call."""
import ctypes
import os
import re

import test_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL = -10

NEW_FUNCTIONS = ("fd_ed25519_amd_new_slots", "fd_ed25519_amd_async_depth", "fd_ed25519_amd_async_in_flight",
                 "fd_ed25519_amd_submit_batch", "fd_ed25519_amd_submit_batch_registered", "fd_ed25519_amd_submit_txns",
                 "fd_ed25519_amd_submit_txns_registered", "fd_ed25519_amd_async_poll", "fd_ed25519_amd_async_wait")


def test_symbols_and_codes_are_declared():
    from firedancer_amd import ed25519
    names = test_abi.declared_functions()
    for n in NEW_FUNCTIONS:
        assert n in names, n
        assert hasattr(ed25519.lib(), n), n
    hdr = open(os.path.join(ROOT, "include", "fd_ed25519_amd.h")).read()
    for name, val in (("FD_ED25519_AMD_ERR_BUSY", -12), ("FD_ED25519_AMD_ASYNC_NONE", 1), ("FD_ED25519_AMD_SLOT_MAX", 16)):
        assert re.search(r"#define %s\s+\(\s*%d\)" % (name, val), hdr), name
    assert (ed25519.ERR_BUSY, ed25519.ASYNC_NONE, ed25519.SLOT_MAX) == (-12, 1, 16)
    assert issubclass(ed25519.EngineBusy, ed25519.EngineError)
    # the transaction submits are declared with the calls they mirror
    txn = open(os.path.join(ROOT, "include", "fd_txn_amd.h")).read()
    assert "fd_ed25519_amd_submit_txns(" in txn and "fd_ed25519_amd_submit_txns_registered(" in txn


def test_null_engine_is_refused_by_every_call():
    """Each of the four submits, poll and wait with eng == NULL: ERR_INVAL, and
    the ticket is left alone.  Every other argument is a plausible pointer, so
    it is the engine check that answers."""
    from firedancer_amd import ed25519
    L = ed25519.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    t = ctypes.c_ulong(77)
    tk = ctypes.byref(t)
    assert L.fd_ed25519_amd_submit_batch(None, 1, p, p, p, p, p, p, tk) == INVAL
    assert L.fd_ed25519_amd_submit_batch_registered(None, 1, p, p, p, p, p, p, tk) == INVAL
    assert L.fd_ed25519_amd_submit_txns(None, 1, p, p, p, 64, p, p, p, p, p, p, p, 4096, tk) == INVAL
    assert L.fd_ed25519_amd_submit_txns_registered(None, 1, p, p, p, p, p, p, p, p, p, 4096, tk) == INVAL
    assert L.fd_ed25519_amd_async_poll(None, tk) == INVAL
    assert L.fd_ed25519_amd_async_wait(None, tk) == INVAL
    assert t.value == 77
    assert L.fd_ed25519_amd_async_depth(None) == 0 and L.fd_ed25519_amd_async_in_flight(None) == 0


def test_new_slots_refuses_a_bad_slot_count_before_any_device_call():
    """0, 1 and 17 slots: NULL.  The device number is one no machine has, so a
    call that got as far as the device would fail too -- but with a message on
    stderr; the slot check is silent and comes first."""
    from firedancer_amd import ed25519
    L = ed25519.lib()
    for slots in (0, 1, 17, 1 << 40):
        assert not L.fd_ed25519_amd_new_slots(0, 512, 1 << 16, slots), slots


def test_new_slots_check_is_silent(capfd):
    from firedancer_amd import ed25519
    assert not ed25519.lib().fd_ed25519_amd_new_slots(0x7ffffff0, 512, 1 << 16, 17)
    assert "no HIP device" not in capfd.readouterr().err
