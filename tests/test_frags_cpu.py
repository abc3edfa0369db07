"""CPU: fd_ed25519_amd_frags, the frag rule as host code (include/fd_tango_amd.h,
"Frag submissions"), against the Python restatement of tests/_frags.py on
rings of depth 64 and 256.  No GPU.  All comparisons are exact."""
import ctypes
import os
import re

import numpy as np
import pytest

import _frags
from _frags import BAD, SEQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S8, S64 = 0x55, 0x5555555555555555
PAD = 8                                   # guard elements on each side of every output


def ring_of(depth, seq0, n, frag_max=_frags.FRAG_MAX):
    r = _frags.Ring(depth, seq0, _frags.ru(64 * (22 * max(n, 4) + 8), _frags.PAGE), frag_max)
    _frags.corpus(r, n)
    return r


def call_raw(ring, seq0, n, src=None):
    """The C function on outputs with PAD guard elements around each: (return
    value, status, pub, sig, msg, sz) after checking that the guards hold."""
    from firedancer_amd import ed25519
    st = np.full(n + 2 * PAD, S8, np.int8)
    outs = [np.full(n + 2 * PAD, S64, np.uint64) for _ in range(4)]
    src = src if src is not None else ed25519.frag_src(ring.mcache, ring.region, ring.frag_max)
    at = lambda a: ctypes.c_void_p(a.ctypes.data + PAD * a.itemsize)
    good = int(ed25519.lib().fd_ed25519_amd_frags(ctypes.byref(src) if src else None, seq0 & _frags.M64, n, at(st),
                                                  *[at(a) for a in outs]))
    for a, fill in [(st, S8)] + [(a, S64) for a in outs]:
        assert (a[:PAD] == fill).all() and (a[PAD + n:] == fill).all(), "a guard element was written"
    return (good, st[PAD:PAD + n]) + tuple(a[PAD:PAD + n] for a in outs)


def check(ring, seq0, n):
    st, off, msz = _frags.rule(ring.mcache, ring.data_sz, ring.frag_max, seq0, n)
    want = _frags.host_outputs(st, off, msz, ring.region.ctypes.data)
    before = ring.snapshot()
    got = call_raw(ring, seq0, n)
    assert got[0] == int((st == 0).sum())
    assert np.array_equal(got[1], st), (got[1], st)
    for g, w, name in zip(got[2:], want, ("pub", "sig", "msg", "sz")):
        assert np.array_equal(g, w), name
    after = ring.snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    return st


@pytest.mark.parametrize("which", [0, 1], ids=["line_wrap", "seq_wrap"])
@pytest.mark.parametrize("depth,n", [(d, n) for d in (64, 256) for n in _frags.NS[d]])
def test_host_rule_on_the_corpus(depth, n, which):
    seq0 = _frags.seq0s(depth)[which]
    assert which or (seq0 & (depth - 1)) == depth - 3
    r = ring_of(depth, seq0, n)
    st = check(r, seq0, n)
    assert np.array_equal(st, _frags.expect_status(r.kind))          # the corpus is what it says
    if n >= 33:
        assert set(r.kind.values()) == set(_frags.SPECIALS) | {"good"}
        assert {int(x) for x in st} == {0, SEQ, BAD}


def test_python_wrapper_and_python_call():
    from firedancer_amd import ed25519
    depth, n, seq0 = 64, 64, (1 << 64) - 7
    r = ring_of(depth, seq0, n)
    st, off, msz = _frags.rule(r.mcache, r.data_sz, r.frag_max, seq0, n)
    good, status, pub, sig, msg, sz = ed25519.frags(r.mcache, r.region, seq0, n, r.frag_max)
    assert good == int((st == 0).sum()) and np.array_equal(status, st)
    for g, w in zip((pub, sig, msg, sz), _frags.host_outputs(st, off, msz, r.region.ctypes.data)):
        assert np.array_equal(g, w)
    assert (ed25519.VERDICT_FRAG_SEQ, ed25519.VERDICT_FRAG_BAD) == (SEQ, BAD)


def test_every_named_case_alone():
    """One line at a time on a ring of 64: the boundary on each side of
    every comparison the rule makes."""
    depth, seq0, dsz = 64, 1000, 8192
    r = _frags.Ring(depth, seq0, dsz)
    cases = [  # chunk, sz, seq_delta, status
        (0, 96, 0, 0), (0, 95, 0, BAD), (0, 0, 0, BAD), (0, r.frag_max, 0, 0), (0, r.frag_max + 1, 0, BAD), (0, 65535, 0, BAD),
        (dsz // 64 - 2, 128, 0, 0), (dsz // 64 - 2, 129, 0, BAD), (dsz // 64, 96, 0, BAD), (dsz // 64 - 1, 96, 0, BAD),
        (0xFFFFFFFF, 200, 0, BAD), (0x04000000, 200, 0, BAD),
        (3, 200, -depth, SEQ), (3, 200, -1, SEQ), (3, 200, depth, SEQ), (3, 200, 1, SEQ), (3, 200, 1 << 63, SEQ),
        (0xFFFFFFFF, 0, -1, SEQ),                       # the sequence number is looked at first
    ]
    for i, (chunk, sz, delta, want) in enumerate(cases):
        r.put(i, chunk, sz, delta)
    st = check(r, seq0, len(cases))
    assert st.tolist() == [c[3] for c in cases]
    # items past the published ones: the lines still hold what mcache_new left (seq - depth)
    st = check(r, seq0 + len(cases), depth - len(cases))
    assert (st == SEQ).all()
    # n beyond depth reads the lines again, now one lap late: only the line published one lap ahead matches
    st = check(r, seq0, 2 * depth)
    ahead = [c[2] for c in cases].index(depth)
    assert st[:len(cases)].tolist() == [c[3] for c in cases]
    assert st[depth + ahead] == 0 and int((st[depth:] == SEQ).sum()) == depth - 1


def test_frag_max_65535_leaves_the_region_rule():
    """With the largest frag_max a frag of 65535 bytes is refused by the
    region alone, and accepted where the region holds it."""
    depth, seq0 = 64, 7
    r = _frags.Ring(depth, seq0, 2 * 65536, 65535)
    r.put(0, 0, 65535)
    r.put(1, 1024, 65535)                                # 65536 + 65535 <= 131072
    r.put(2, 1025, 65535)                                # one chunk further: past the end
    r.put(3, 2047, 64)
    r.put(4, 2046, 128)
    assert check(r, seq0, 5).tolist() == [0, 0, BAD, BAD, 0]


def test_bad_sources_write_nothing():
    from firedancer_amd import ed25519
    r = ring_of(64, 0, 16)
    ok = lambda **kw: ed25519.FragSrc(**dict(dict(mcache=r.mcache.ctypes.data, depth=64, chunk0=r.region.ctypes.data,
                                                  data_sz=r.data_sz, frag_max=r.frag_max), **kw))
    assert call_raw(r, 0, 16, ok())[0] > 0
    for kw in (dict(mcache=None), dict(chunk0=None), dict(depth=0), dict(depth=48), dict(depth=65), dict(frag_max=95),
               dict(frag_max=65536)):
        got = call_raw(r, 0, 16, ok(**kw))
        assert got[0] == 0 and (got[1] == S8).all() and all((a == S64).all() for a in got[2:]), kw
    st = np.full(4, S8, np.int8)
    assert ed25519.lib().fd_ed25519_amd_frags(None, 0, 4, ed25519._ptr(st), None, None, None, None) == 0 and (st == S8).all()


def test_header_states_the_values_and_the_struct():
    from firedancer_amd import ed25519
    hdr = open(os.path.join(ROOT, "include", "fd_tango_amd.h")).read()
    assert re.search(r"#define FD_ED25519_AMD_VERDICT_FRAG_SEQ\s+\(-5\)", hdr)
    assert re.search(r"#define FD_ED25519_AMD_VERDICT_FRAG_BAD\s+\(-6\)", hdr)
    assert ctypes.sizeof(ed25519.FragSrc) == 40 and ed25519.GATHER_REC.itemsize == 32
    for name in ("fd_ed25519_amd_frags", "fd_ed25519_amd_submit_frags", "fd_ed25519_amd_frag_list_dev",
                 "fd_ed25519_amd_frag_check_dev"):
        assert name in hdr and hasattr(ed25519.lib(), name)
    # the submit call's argument errors that need no device: refused before anything touches one
    t = ctypes.c_ulong(99)
    assert ed25519.lib().fd_ed25519_amd_submit_frags(None, None, 0, 1, None, None, None, None, None, 0, None, None,
                                                     ctypes.byref(t)) == ed25519.ERR_INVAL and t.value == 99
    assert ed25519.lib().fd_ed25519_amd_frag_list_dev(None, 0, 1, None, None, None, None) == ed25519.ERR_INVAL
    assert ed25519.lib().fd_ed25519_amd_frag_check_dev(None, 0, 1, None, None) == ed25519.ERR_INVAL
