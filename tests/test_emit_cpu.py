"""CPU: the host output-frame functions (fd_ed25519_amd_emit, fd_txn_amd_emit,
fd_ed25519_amd_emit_bound, fd_txn_amd_emit_bound) against the byte-level
model of tests/_emit.py, and the same cases through a stand-alone C program
built with the address and undefined-behaviour sanitizers.  No GPU, nothing
preloaded.  All comparisons are exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _emit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def sigs():
    return _emit.sig_items()


@pytest.fixture(scope="module")
def txns():
    """(names, payloads, descriptors): the payload set and liboracle's
    fd_txn_parse of each; every one parses."""
    pays = _emit.txn_payloads()
    descs = [_emit.oracle_desc(p) for p in pays.values()]
    assert all(len(d) >= 20 for d in descs)
    assert len(descs[-1]) == 3570                      # the MTU payload's 355 instructions
    return list(pays), list(pays.values()), descs


def _check(call, frames, keep):
    """One keep list through `call( keep, out, out_cap )`: out == NULL, the
    exact capacity, and one byte short."""
    fr = [frames[i] for i in keep]
    image = np.full(int(_emit.place(fr)[0][-1]), _emit.FILL, np.uint8)
    off, sz = _emit.lay(fr, image)
    tot = int(off[-1])
    got = call(keep, None, None)                        # out == NULL only computes the layout
    assert got[0] == tot and np.array_equal(got[1], off) and np.array_equal(got[2], sz)
    out = np.full(max(tot, 1), _emit.FILL, np.uint8)
    got = call(keep, out, tot)                          # out_cap exact
    assert got[0] == tot and np.array_equal(got[1], off) and np.array_equal(got[2], sz)
    assert np.array_equal(out[:tot], image), np.nonzero(out[:tot] != image)[0][:8]
    if tot:
        out[:] = _emit.FILL
        got = call(keep, out, tot - 1)                  # one byte short: ~0UL and the buffer untouched
        assert got[0] == NONE and (out == _emit.FILL).all()
        assert not got[1].any() and not got[2].any()    # the layout is not written either
    return tot


@pytest.mark.parametrize("kname", ["empty", "all", "sparse", "last"])
def test_signature_frames(sigs, kname):
    from firedancer_amd import ed25519
    keep = _emit.keep_lists(len(sigs))[kname]
    frames = [_emit.sig_frame(p, s, m) for p, s, m in sigs]
    call = lambda k, out, cap: ed25519.emit(k, [m for _, _, m in sigs], [s for _, s, _ in sigs], [p for p, _, _ in sigs], out, cap)
    tot = _check(call, frames, keep)
    assert (tot == 0) == (kname == "empty")


@pytest.mark.parametrize("kname", ["empty", "all", "sparse", "last"])
def test_transaction_frames(txns, kname):
    from firedancer_amd import ed25519
    _, pays, descs = txns
    keep = _emit.keep_lists(len(pays))[kname]
    frames = [_emit.txn_frame(p, d) for p, d in zip(pays, descs)]
    doff, desc = _emit.pack_desc(descs)
    call = lambda k, out, cap: ed25519.txn_emit(k, pays, doff, desc, out, cap)
    _check(call, frames, keep)


def test_transaction_frame_fields(txns):
    """What a consumer does with a frame: P from the last two bytes, the
    descriptor at the 16-aligned offset round_up( P, 16 )."""
    from firedancer_amd import ed25519
    _, pays, descs = txns
    doff, desc = _emit.pack_desc(descs)
    out = np.full(1 << 16, _emit.FILL, np.uint8)
    tot, off, sz = ed25519.txn_emit(list(range(len(pays))), pays, doff, desc, out)
    assert tot <= out.size
    for j, (p, d) in enumerate(zip(pays, descs)):
        fr = bytes(out[int(off[j]):int(off[j]) + int(sz[j])])
        P = struct.unpack("<H", fr[-2:])[0]
        assert P == len(p) and fr[:P] == p
        at = _emit.ru(P, 16)
        assert at % 16 == 0 and int(off[j]) % 128 == 0 and fr[at:-2] == d and len(d) % 2 == 0


def test_bounds(sigs, txns):
    """Each bound is the issue's formula and at least the stride of every
    case; the MTU payload of 355 empty instructions meets its bound with
    equality (1232 + 3570 + 2 bytes)."""
    from firedancer_amd import ed25519
    for z in list(_emit.MSG_SIZES) + [2, 200, 65535, 1 << 20]:
        assert ed25519.emit_bound(z) == _emit.sig_bound(z) >= _emit.ru(96 + z, 128)
    for z in list(range(0, 1400)) + [65535, 65536, 1 << 20]:
        assert ed25519.txn_emit_bound(z) == _emit.txn_bound(z)
        assert (ed25519.txn_emit_bound(z) == 0) == (ed25519.txn_desc_bound(z) == 0)
    names, pays, descs = txns
    for name, p, d in zip(names, pays, descs):
        stride = _emit.ru(len(_emit.txn_frame(p, d)), 128)
        assert ed25519.txn_emit_bound(len(p)) >= stride, name
    assert len(_emit.txn_frame(pays[-1], descs[-1])) == 1232 + 3570 + 2
    assert ed25519.txn_emit_bound(1232) == _emit.ru(1232 + 3570 + 2, 128)


def _u64(*v):
    return struct.pack("<%dQ" % len(v), *[int(x) for x in v])


def _case(fam, items, frames, keep):
    fr = [frames[i] for i in keep]
    image = np.full(int(_emit.place(fr)[0][-1]), _emit.FILL, np.uint8)
    off, sz = _emit.lay(fr, image)
    b = _u64(fam, len(items), len(keep), *keep)
    for it in items:
        b += (_u64(len(it[2])) + it[0] + it[1] + it[2]) if fam == 0 else (_u64(len(it[0]), len(it[1])) + it[0] + it[1])
    return b + _u64(int(off[-1]), *off.tolist(), *sz.tolist()) + image.tobytes()


def test_host_functions_under_sanitizers(sigs, txns, tmp_path):
    """fd_ed25519_host.cpp and tests/c/emit_host_check.c compiled with gcc
    -fsanitize=address,undefined; the program runs the cases above (every
    keep list, both families, exact capacity / one byte short / layout only)
    on heap blocks of exactly each buffer's size."""
    _, pays, descs = txns
    cases = []
    for keep in _emit.keep_lists(len(sigs)).values():
        cases.append(_case(0, sigs, [_emit.sig_frame(*s) for s in sigs], keep))
    for keep in _emit.keep_lists(len(pays)).values():
        cases.append(_case(1, list(zip(pays, descs)), [_emit.txn_frame(p, d) for p, d in zip(pays, descs)], keep))
    path = tmp_path / "cases.bin"
    path.write_bytes(b"FDEMIT01" + _u64(len(cases)) + b"".join(cases))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    csrc = os.path.join(ROOT, "firedancer_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "fd_ed25519_consts.h")), "build() generates it"
    host_o, chk_o, exe = tmp_path / "host.o", tmp_path / "check.o", tmp_path / "emit_host_check"
    subprocess.check_call(["gcc", "-std=c++17", "-Wall", "-Wno-unused-function"] + san +
                          ["-c", os.path.join(csrc, "fd_ed25519_host.cpp"), "-o", str(host_o)])
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror"] + san + ["-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "c", "emit_host_check.c"), "-o", str(chk_o)])
    # the sanitizer runtimes linked statically: the program needs nothing preloaded and no particular library order
    subprocess.check_call(["gcc"] + san + ["-static-libasan", "-static-libubsan", str(chk_o), str(host_o), "-lstdc++", "-lpthread",
                                           "-lm", "-o", str(exe)])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "emit_host_check: %d cases OK" % len(cases) in r.stdout, r.stdout + r.stderr
