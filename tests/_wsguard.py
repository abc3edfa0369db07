"""Guarded device buffers and workspace poisons, for tests that pin "the
results are a function of the inputs alone" (test_workspace_state_gpu.py).

Guarded( nbytes, fill ) is ONE device allocation of G + nbytes + G bytes:
two guards of a fixed byte around the body a kernel is given.  A stray write
next to the body lands in memory the test owns and check() sees it.  (A
stray READ cannot be seen this way, and nothing here tries to.)

The poisons fill a verify workspace before a launch:
  zero      all 0x00: what a fresh allocation usually holds, and what a
            forgotten "0 = accepted / no event / decoded" would read;
  leftover  no fill at all: the body is what an earlier real launch left;
  directed  per plane, a value a finished, legitimate launch could have left
            in that plane -- so no count or position read from it exceeds
            what the kernels produce themselves and no loop or index leaves
            its range -- chosen so that a kernel that did read it would
            answer differently.
"""
import numpy as np

G = 4096            # guard bytes on each side; a multiple of 256, so the body keeps the allocation's alignment
GUARD_BYTE = 0xA5

# bytes of each workspace plane: (factor, per row of N?) -- ws_layout_const, firedancer_amd/csrc/fd_ed25519_ws.h
# (test_ws_layout_cpu.py compares this table with that source)
PLANE_BYTES = {"dig": (256, True), "evn": (4, True), "top": (4, True), "A": (120, True), "R": (80, True),
               "Ai": (1536, True), "st": (12, True), "tag": (8, True), "ds": (2, True), "init": (16, True),
               "ctr": (16, False)}


def plane_bytes(plane, N):
    per, rows = PLANE_BYTES[plane]
    return per * N if rows else per


class Guarded:
    """A device buffer of nbytes between two guards.  fill: a host array of
    nbytes bytes (any dtype) for the body, or None to leave the body as the
    allocation came (only the guards are written)."""

    def __init__(self, nbytes, fill=None):
        from firedancer_amd import hip
        self.nbytes = int(nbytes)
        self.buf = hip.DeviceBuffer(G + self.nbytes + G)
        assert self.buf.ptr % 256 == 0
        self.ptr = self.buf.ptr + G
        guard = np.full(G, GUARD_BYTE, np.uint8)
        self._h2d(0, guard)
        self._h2d(G + self.nbytes, guard)
        if fill is not None:
            self.fill(fill)

    def _h2d(self, at, a):
        from firedancer_amd import hip
        a = np.ascontiguousarray(a)
        if a.nbytes:
            hip.check(hip.hip().hipMemcpy(self.buf.ptr + at, a.ctypes.data, a.nbytes, hip.H2D), "hipMemcpy H2D")

    def fill(self, a):
        """Overwrite the whole body."""
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        self._h2d(G, a)

    def write(self, at, a):
        """Overwrite body bytes [at, at + a.nbytes)."""
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert 0 <= at and at + a.nbytes <= self.nbytes
        self._h2d(G + at, a)

    def body(self, dtype=np.uint8, count=None):
        """The body (or its first `count` elements) read back."""
        item = np.dtype(dtype).itemsize
        count = self.nbytes // item if count is None else count
        assert count * item <= self.nbytes
        whole = self.buf.to_array(np.uint8, G + count * item)
        return whole[G:].view(dtype).copy()

    def check(self, what=""):
        """Both guards read back: every byte intact."""
        whole = self.buf.to_array(np.uint8, 2 * G + self.nbytes)
        for name, g in (("below", whole[:G]), ("above", whole[G + self.nbytes:])):
            bad = np.nonzero(g != GUARD_BYTE)[0]
            assert bad.size == 0, ("guard %s the body touched" % name, what, int(bad.size),
                                   [(int(k), hex(int(g[k]))) for k in bad[:8]])

    def free(self):
        self.buf.free()


# ---- poisons ----------------------------------------------------------------------------------

OP_D = 0                      # fd_ed25519_pool.h: a signature that enters the pool with a doubling
EV_TOP = 255 | (0xff << 8)    # a digit event: position 255, digit -1
EV_REAL = 252 | (1 << 8)      # the top event of a real scalar: position 252, digit +1


def zero(total):
    return np.zeros(total, np.uint8)


def directed_planes(L, n):
    """{plane: host array} of the directed fill for a workspace of layout L
    (ed25519.debug_ws_layout( n )):

      ds    1 in both flags                    a decoded point reads as undecodable (-2)
      evn   52 | 52 << 8                       the most events a 253-bit scalar has, for h and s
      top   255                                the highest position there is
      dig   events of position 255, digit -1   with evn / top above: an op stream that adds at the top
      A, R, Ai   0x55555555 limbs              no point, and R' != R
      st    0xFFFFFFFF                         no work statistic is that large
      tag   0x5555555555555555                 no hash, and not the 0 of a rejected s
      init  { 0, EV_REAL | EV_REAL << 16, 252 | 52 << 16 | 52 << 24, OP_D }
                                               what k_ai writes for a signature whose h and s both have
                                               their top digit at position 252: "enter the pool"
      ctr   { N + 112, 1, 0, 0 }               a work counter past n and the guard flag raised, as a
                                               launch whose step guard tripped leaves them
    """
    N = L["N"]
    init = np.tile(np.array([0, EV_REAL | (EV_REAL << 16), 252 | (52 << 16) | (52 << 24), OP_D], np.uint32), N)
    out = {"ds": np.full(2 * N, 1, np.uint8),
           "evn": np.full(N, 52 | (52 << 8), np.uint32),
           "top": np.full(N, 255, np.int32),
           "dig": np.full(128 * N, EV_TOP, np.uint16),
           "A": np.full(30 * N, 0x55555555, np.uint32),
           "R": np.full(20 * N, 0x55555555, np.uint32),
           "Ai": np.full(384 * N, 0x55555555, np.uint32),
           "st": np.full(3 * N, 0xFFFFFFFF, np.uint32),
           "tag": np.full(N, 0x5555555555555555, np.uint64),
           "init": init,
           "ctr": np.array([N + 112, 1, 0, 0], np.uint32)}
    assert N + 112 >= n and set(out) == set(PLANE_BYTES)
    for p, a in out.items():
        assert a.nbytes == plane_bytes(p, N), p
    return out


def directed(L, n):
    """The directed fill as one byte image of L["total"] bytes (the alignment
    gaps between planes are 0)."""
    img = np.zeros(L["total"], np.uint8)
    for p, a in directed_planes(L, n).items():
        img[L[p]:L[p] + a.nbytes] = a.view(np.uint8)
    return img
