"""The frag rule of include/fd_tango_amd.h ("Frag submissions") restated in
Python, and the rings the frag tests run it on.  No GPU, no library call in
the rule itself: rule() reads the FRAG_META array.

A Ring is an mcache of `depth` lines and a data region in page-aligned host
memory of their own (so each can be one registration and a frag can lie flush
against either end of the region's).  corpus() publishes n items from seq0:
good frags of every message size, and at fixed positions one of every case
the rule names."""
import numpy as np

SEQ, BAD = -5, -6
M64 = (1 << 64) - 1
PAGE = 4096
MSG_SIZES = (0, 1, 15, 16, 17, 104, 1232)
FRAG_MAX = 96 + 1232
# one of each at items 2, 5, 8, ... (as far as n goes); the others are good frags
SPECIALS = ("sz0", "seq-depth", "flush_end", "sz95", "seq-1", "past_end", "szmax+1", "seq+depth", "chunk_max", "sz65535",
            "chunk0_again")
NS = {64: (1, 15, 16, 17, 64), 256: (1, 15, 16, 17, 65, 130, 256)}


def seq0s(depth):
    """A start that wraps the line index, one that wraps the sequence itself."""
    return (5 * depth + depth - 3, (1 << 64) - 7)


def ru(x, a):
    return (x + a - 1) // a * a


def aligned(nbytes, align=PAGE):
    raw = np.zeros(ru(nbytes, align) + align, np.uint8)
    o = (-raw.ctypes.data) % align
    a = raw[o:o + nbytes]
    assert a.ctypes.data % align == 0
    return a


def rule(mcache, data_sz, frag_max, seq0, n):
    """(status int8 [n], off uint64 [n], msz uint64 [n]): the item's status,
    and for a good item its frag's byte offset in the region and its message
    size (0, 0 for any other)."""
    depth = int(mcache.size)
    assert depth and not depth & (depth - 1) and 96 <= frag_max <= 65535
    st, off, msz = np.zeros(n, np.int8), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for i in range(n):
        seq = (seq0 + i) & M64
        line = mcache[seq & (depth - 1)]
        if int(line["seq"]) != seq:
            st[i] = SEQ
            continue
        at, sz = int(line["chunk"]) << 6, int(line["sz"])
        if sz < 96 or sz > frag_max or at + sz > data_sz:
            st[i] = BAD
            continue
        off[i], msz[i] = at, sz - 96
    return st, off, msz


def host_outputs(st, off, msz, base):
    """What fd_ed25519_amd_frags writes: (pub, sig, msg, sz), NULL / 0 for an item without a frag."""
    good = st == 0
    z = np.zeros(st.size, np.uint64)
    b = np.uint64(base)
    return (np.where(good, b + off, z), np.where(good, b + off + np.uint64(32), z), np.where(good, b + off + np.uint64(96), z),
            np.where(good, msz, z))


def records(st, off, msz, base, idle, frag_max):
    """The fd_amd_gather_rec_t k_frag_list writes per item: (pub, sig, msg, sz, dst) columns."""
    good = st == 0
    n = st.size
    b, d = np.uint64(base), np.full(n, idle, np.uint64)
    pub = np.where(good, b + off, d)
    msg = np.where(good & (msz > 0), b + off + np.uint64(96), d)
    dst = np.arange(n, dtype=np.uint64) * np.uint64(ru(frag_max - 96, 16))
    return pub, pub + np.uint64(32), msg, np.where(good, msz, 0).astype(np.uint32), dst.astype(np.uint32)


class Ring:
    def __init__(self, depth, seq0, data_sz, frag_max=FRAG_MAX):
        from firedancer_amd import tango
        self.depth, self.seq0, self.data_sz, self.frag_max = depth, seq0 & M64, data_sz, frag_max
        self.mcache = aligned(32 * depth).view(tango.FRAG_META)
        self.mcache[:] = tango.mcache_new(depth, self.seq0)
        self.region = aligned(data_sz)
        self.region[:] = np.random.default_rng(depth + data_sz).integers(0, 256, data_sz, dtype=np.uint8)
        self.kind, self.where = {}, {}             # corpus(): item -> kind, item -> (chunk, message size) of its own room

    def put(self, i, chunk, sz, seq_delta=0):
        """Publish item i's line with the given fields; seq_delta: what the
        line's seq differs by from seq0 + i."""
        from firedancer_amd import tango
        seq = (self.seq0 + i) & M64
        line = self.mcache[seq & (self.depth - 1)]
        tango.publish(self.mcache, seq, 0x1111 * (i + 1), chunk, sz, i & 3, 7 * i, 9 * i)
        line["seq"] = (seq + seq_delta) & M64

    def snapshot(self):
        return self.mcache.copy(), self.region.copy()

    def frag(self, off, msz):
        """(pub, sig, msg) bytes of the frag at byte offset off."""
        r = self.region
        return bytes(r[off:off + 32]), bytes(r[off + 32:off + 96]), bytes(r[off + 96:off + 96 + msz])


def corpus(ring, n, fill=None):
    """Items [0, n) of ring: a good frag per item (message sizes in turn,
    packed chunk by chunk from chunk 1), except at items 2, 5, 8, ... which
    take SPECIALS in turn.  The first good frag lies at chunk 0.  fill( i, off, msz ) writes the bytes of
    every item that has room of its own in the region (ring.where), whatever
    its line then says.  Returns {item: kind}."""
    assert n <= ring.depth
    chunk, kinds, first = 1, {}, True
    last = ring.data_sz // 64 - 2                  # flush_end: a 128-byte frag whose last byte is the region's last
    assert ring.data_sz % 64 == 0
    for i in range(n):
        msz = MSG_SIZES[i % len(MSG_SIZES)]
        kind = SPECIALS[(i // 3) % len(SPECIALS)] if i % 3 == 2 else "good"
        at, sz, delta = chunk, 96 + msz, 0
        if kind == "good" and first:
            at, first = 0, False
        elif kind == "chunk0_again":
            at, sz = 0, 96                         # a good frag: the key and signature at chunk 0, no message
        elif kind == "flush_end":
            at, sz = last, 128
        elif kind == "past_end":
            at, sz = last, 129
        elif kind == "chunk_max":
            at = 0xFFFFFFFF
        elif kind.startswith("sz"):
            sz = {"sz0": 0, "sz95": 95, "szmax+1": ring.frag_max + 1, "sz65535": 65535}[kind]
        elif kind.startswith("seq"):
            delta = {"seq-depth": -ring.depth, "seq-1": -1, "seq+depth": ring.depth}[kind]
        if at == chunk:                            # the item has room of its own, whatever its line says
            assert (chunk << 6) + 96 + msz <= (last << 6), "region too small"
            ring.where[i] = (chunk, msz)
            if fill is not None:
                fill(i, chunk << 6, msz)
            chunk += ru(96 + msz, 64) // 64
        elif kind == "good":
            ring.where[i] = (0, msz)
            if fill is not None:
                fill(i, 0, msz)
        ring.put(i, at, sz, delta)
        kinds[i] = kind
    ring.kind = kinds
    return kinds


def expect_status(kinds, frag_max=FRAG_MAX):
    out = []
    for i in sorted(kinds):
        k = kinds[i]
        out.append(SEQ if k.startswith("seq") else BAD if k in ("sz0", "sz95", "szmax+1", "sz65535", "past_end", "chunk_max") else 0)
    return np.array(out, np.int8)
