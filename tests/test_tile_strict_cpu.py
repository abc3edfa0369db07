"""CPU: the streaming tile's strict verdict mode without a GPU -- the build
guard over the strict instantiation of the persistent kernel, the exported
and declared entry points, their argument checks, the bench flag."""
import ctypes
import os
import re

import pytest

from firedancer_amd import build
from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(build.PKG, "_obj", "libfd_ed25519_amd", "fd_ed25519_kernels.hip.o")
INVAL = -10


@pytest.mark.skipif(not os.path.exists(OBJ), reason="engine objects not built here")
def test_strict_tile_kernel_has_no_loop_spills():
    """k_tile_persist_strict is in the code object, the guard finds its loop
    and counts no scratch store in it; both tile kernels are distinct
    symbols and the reference one keeps its name."""
    assert build.TILE_KERNEL == "_Z14k_tile_persist18fd_amd_tile_args_t"
    assert build.TILE_KERNEL_STRICT != build.TILE_KERNEL and "k_tile_persist_strict" in build.TILE_KERNEL_STRICT
    assert build.loop_spill_stores(OBJ, build.TILE_KERNEL_STRICT) == 0
    v = build.kernel_vgprs(OBJ, build.TILE_KERNEL_STRICT)
    assert v is not None and 0 < v <= 256


def test_build_guards_both_tile_kernels(monkeypatch, tmp_path):
    """build_engine refuses a build whose STRICT kernel spills in its loop
    (or cannot be inspected) even when the reference kernel is clean."""
    monkeypatch.setattr(build.subprocess, "check_call", lambda *a, **k: None)
    for strict_result, msg in ((3, "k_tile_persist_strict spills"), (None, "cannot inspect k_tile_persist_strict")):
        asked = []

        def fake(obj, kernel, r=strict_result):
            asked.append(kernel)
            return r if kernel == build.TILE_KERNEL_STRICT else 0
        monkeypatch.setattr(build, "loop_spill_stores", fake)
        with pytest.raises(RuntimeError, match=msg):
            build.build_engine(force=True, out=str(tmp_path / "lib.so"), defines=("FD_AMD_GUARD_TEST",))
        assert asked == [build.TILE_KERNEL, build.TILE_KERNEL_STRICT]


def test_verdict_mode_entry_points_declared_and_exported():
    from firedancer_amd import ed25519
    L = ed25519.lib()
    names = declared_functions()
    for n in ("fd_verify_amd_tile_set_verdict_mode", "fd_verify_amd_tile_verdict_mode"):
        assert n in names and hasattr(L, n), n
    assert "fd_verify_amd_tile_mode" in names           # the chunk-mode rule keeps its name


@pytest.mark.parametrize("mode", [0, 1, 2, -1])
def test_null_tile_is_refused(mode):
    from firedancer_amd import ed25519
    L = ed25519.lib()
    assert L.fd_verify_amd_tile_set_verdict_mode(ctypes.c_void_p(0), mode) == INVAL
    assert L.fd_verify_amd_tile_verdict_mode(ctypes.c_void_p(0)) == INVAL


def test_bench_flag_is_its_own_bit_and_mirrored():
    from firedancer_amd import tango
    hdr = open(os.path.join(ROOT, "include", "fd_tango_amd.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (FD_VERIFY_AMD_BENCH_\w+)\s+\((\d+)\)", hdr)}
    assert flags["FD_VERIFY_AMD_BENCH_STRICT"] == 2048 == tango.BENCH_STRICT
    vals = list(flags.values())
    assert len(flags) >= 12 and len(set(vals)) == len(vals)
    assert all(v and not v & (v - 1) for v in vals)     # one bit each: no flag is a combination of others
    import inspect
    sig = inspect.signature(tango.bench_stream)
    assert sig.parameters["strict"].default is False
    assert inspect.signature(tango.VerifyTile.__init__).parameters["mode"].default == 0
