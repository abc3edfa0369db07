"""CPU: the verify workspace's layout, read back through
fd_ed25519_amd_debug_ws_layout (host code, no device).  The GPU tests that
fill single planes (_wsguard.py, test_workspace_state_gpu.py) stand on it:
the planes lie where the kernels are told they lie, do not overlap, and end
at the footprint a caller allocates."""
import os
import re

import pytest

import _wsguard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [0, 1, 63, 64, 65, 112, 113, 4096, 1 << 20]


@pytest.mark.parametrize("n", NS)
def test_planes_ordered_aligned_disjoint(n):
    from firedancer_amd import ed25519
    L = ed25519.debug_ws_layout(n)
    assert set(L) == {"N", "total"} | set(ed25519.WS_PLANES) == {"N", "total"} | set(_wsguard.PLANE_BYTES)
    N = L["N"]
    assert N == max(64, (n + 63) // 64 * 64) and N % 64 == 0 and N >= n
    assert L["total"] == ed25519.workspace_footprint(n)
    order = sorted(ed25519.WS_PLANES, key=lambda p: L[p])
    assert tuple(order) == ed25519.WS_PLANES                     # ascending in the order the header names them
    assert L[order[0]] == 0
    for p, q in zip(order, order[1:] + ["total"]):
        assert L[p] % 256 == 0, p
        assert L[p] + _wsguard.plane_bytes(p, N) <= L[q], (p, q)  # ends before the next one starts
        assert L[q] - (L[p] + _wsguard.plane_bytes(p, N)) < 256   # and only alignment lies between them
    assert L["total"] % 256 == 0


def test_footprint_non_decreasing():
    from firedancer_amd import ed25519
    f = [ed25519.workspace_footprint(n) for n in NS]
    assert f == sorted(f) and f[0] == f[1] == f[3] < f[4] == f[5] == f[6] < f[7] < f[8]   # N = 64, 64, .., 128, ..
    dense = [ed25519.workspace_footprint(n) for n in range(0, 400)]
    assert dense == sorted(dense)
    assert ed25519.debug_ws_layout(0) == ed25519.debug_ws_layout(1) == ed25519.debug_ws_layout(64)


def test_plane_sizes_are_the_ones_the_layout_header_writes():
    """_wsguard.PLANE_BYTES restates the sizes of ws_layout_const
    (firedancer_amd/csrc/fd_ed25519_ws.h); a plane added or resized there must
    be restated here, or the directed fills would miss part of it."""
    src = open(os.path.join(ROOT, "firedancer_amd", "csrc", "fd_ed25519_ws.h")).read()
    got = {}
    for name, expr in re.findall(r"L\.(\w+)\s*=\s*o;\s*o\s*=\s*ws_al\(\s*o\s*\+\s*([^;]*?)\s*\);", src):
        factors = [int(x) for x in re.findall(r"(\d+)UL", expr)]
        per = 1
        for x in factors:
            per *= x
        got[name] = (per, "N" in expr)
    assert got == _wsguard.PLANE_BYTES
