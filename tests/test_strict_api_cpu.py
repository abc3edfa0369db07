"""CPU: strict mode's host-side surface -- the mode argument is validated
before any device call, the Python mirror exports it, and the torsion
constants the kernel compares against regenerate from first principles."""
import ctypes
import importlib.util
import os
import re

import pytest

import _strict_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL = -10


@pytest.mark.parametrize("mode", [2, -1, 1 << 20])
def test_bad_mode_is_refused_before_any_device_call(mode):
    """n = 0 / txn_cnt = 0 is FD_ED25519_AMD_OK for a valid mode and needs no
    device, so ERR_INVAL here is the mode check alone; with n > 0 and NULL
    pointers the mode is still what is reported first."""
    from firedancer_amd import ed25519
    L = ed25519.lib()
    z = ctypes.c_void_p(0)
    for n in (0, 64):
        assert L.fd_ed25519_amd_verify_dev_mode(n, z, z, z, z, z, z, z, z, mode) == INVAL
        assert L.fd_ed25519_amd_verify_dev_ev_mode(n, z, z, z, z, z, z, z, z, z, mode) == INVAL
        assert L.fd_ed25519_amd_verify_txns_dev_mode(n, n, z, z, z, z, z, z, z, z, mode) == INVAL
    for ok in (ed25519.MODE_REFERENCE, ed25519.MODE_STRICT):
        assert L.fd_ed25519_amd_verify_dev_mode(0, z, z, z, z, z, z, z, z, ok) == 0
        assert L.fd_ed25519_amd_verify_txns_dev_mode(0, 0, z, z, z, z, z, z, z, z, ok) == 0
    assert L.fd_ed25519_amd_set_mode(z, 1) == INVAL and L.fd_ed25519_amd_multi_set_mode(z, 1) == INVAL
    with pytest.raises(ed25519.EngineError):
        ed25519.verify_dev(0, z, z, z, z, z, z, z, 0, mode=mode)
    with pytest.raises(ed25519.EngineError):                 # refused before fd_ed25519_amd_new looks for a device
        ed25519.Engine(device=0, mode=mode)
    with pytest.raises(ed25519.EngineError):
        ed25519.MultiEngine([0], mode=mode)


def test_mode_constants_match_the_header():
    import firedancer_amd
    from firedancer_amd import ed25519
    hdr = open(os.path.join(ROOT, "include", "fd_ed25519_amd.h")).read()
    for name, val in (("FD_ED25519_AMD_MODE_REFERENCE", ed25519.MODE_REFERENCE), ("FD_ED25519_AMD_MODE_STRICT", ed25519.MODE_STRICT)):
        assert re.search(r"#define %s\s+\(\s*%d\)" % (name, val), hdr), name
    assert (firedancer_amd.MODE_REFERENCE, firedancer_amd.MODE_STRICT) == (0, 1)


def _gen_consts():
    spec = importlib.util.spec_from_file_location("gen_consts", os.path.join(ROOT, "tools", "gen_consts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _words(line):
    ws = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", line)]
    assert len(ws) == 8
    return sum(w << (32 * k) for k, w in enumerate(ws))


def test_torsion_constants_regenerate_and_are_the_order_8_ys(tmp_path):
    gc = _gen_consts()
    out = tmp_path / "consts.h"
    gc.emit(str(out), "FD_AMD")
    new = {m.group(1): m.group(0) for m in re.finditer(r"#define (FD_AMD_Y8N?_WORDS) .*", out.read_text())}
    built = open(os.path.join(ROOT, "firedancer_amd", "csrc", "fd_ed25519_consts.h")).read()   # what the engine was compiled with
    assert set(new) == {"FD_AMD_Y8_WORDS", "FD_AMD_Y8N_WORDS"}
    for line in new.values():
        assert line in built
    y8, y8n = _words(new["FD_AMD_Y8_WORDS"]), _words(new["FD_AMD_Y8N_WORDS"])
    assert y8 + y8n == S.P and y8 < y8n

    # an order-8 point T, found here with the checker's big-integer arithmetic
    # alone: [L]Q kills the prime-order part of any curve point Q, what is left
    # is torsion; take one whose order is exactly 8
    T, y = None, 2
    while T is None:
        Q = S.decode(y.to_bytes(32, "little"))
        y += 1
        if Q is None:
            continue
        t = S.mul(S.L, Q)
        if S.is_identity(S.mul(8, t)) and not S.is_identity(S.mul(4, t)):
            T = t
    aff = lambda p: (p[0] * pow(p[2], S.P - 2, S.P) % S.P, p[1] * pow(p[2], S.P - 2, S.P) % S.P)
    pts = [aff(S.mul(k, T)) for k in range(8)]
    assert len(set(pts)) == 8
    assert {py for k, (px, py) in enumerate(pts) if k & 1} == {y8, y8n}            # the four points of order 8
    assert {py for px, py in pts} == {0, 1, S.P - 1, y8, y8n}                      # the kernel's list is the whole torsion
    assert {px for px, py in pts if py in (1, S.P - 1)} == {0}                     # and y = +-1 are the points with x = 0
    for px, py in pts:                                                             # each is rejected by the checker as torsion
        enc = (py | (px & 1) << 255).to_bytes(32, "little")
        P8 = S.decode(enc)
        assert P8 is not None and S.is_identity(S.mul(8, P8))
