"""CPU: the dedup window's rule on a host-only window
(fd_ed25519_amd_window_keep; include/fd_ed25519_amd.h, "The dedup window")
against the rule restated in Python, the directed cases of its text, its
relation to an item-by-item tcache, and export / import.  No device.  All
comparisons are exact."""
import numpy as np
import pytest

from _window import Rule, Tcache, _arr, conditioned_stream, random_stream

# depth, n: n <= depth, around the 64-item block of the scan and beyond one
SHAPES = [(1, 1), (64, 1), (64, 63), (64, 64), (320, 1), (320, 63), (320, 64), (320, 65), (320, 257)]


def _calls(depth, n):
    return (12 * depth + n - 1) // n + 4       # about a third of the items are inserted: the ring wraps three times and more


@pytest.mark.parametrize("depth,n", SHAPES)
def test_host_window_against_the_rule(depth, n):
    from firedancer_amd import ed25519
    w, r = ed25519.Window(-1, depth), Rule(depth)
    try:
        assert w.depth == depth and w.export().size == 0
        for k, (err, tag) in enumerate(random_stream(depth * 1000 + n, depth, n, _calls(depth, n))):
            got, want = w.keep(err, tag), r.keep(err, tag)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (k, got[:8], want[:8])
            assert np.array_equal(w.export(), r.export()), k
        assert len(r.T) >= 3 * depth               # the ring wrapped at least three times
    finally:
        w.close()


def _one(w, r, err, tag):
    got = w.keep(*_arr(err, tag))
    assert np.array_equal(got, r.keep(*_arr(err, tag)))
    assert np.array_equal(w.export(), r.export())
    return got.tolist()


@pytest.fixture
def pair():
    from firedancer_amd import ed25519
    w = ed25519.Window(-1, 8, salt=5)
    yield w, Rule(8)
    w.close()


def test_a_tag_expires_after_exactly_depth_inserts(pair):
    """A tag is live for exactly D inserts.  Counting inserts from one, as the
    map's stamps do (the q-th insert is T[q - 1]): re-offered when head =
    q + D - 1 it is dropped (live: max( 0, H - D ) <= q - 1), at head = q + D
    it is kept."""
    w, r = pair
    assert _one(w, r, [0, 0], [100, 200]) == [0, 1]            # 200 is insert q = 2 (T[1])
    assert _one(w, r, [0] * 6, range(1, 7)) == list(range(6))  # head = 8
    assert _one(w, r, [0], [100]) == []                        # insert 1 at head = 8 = 1 + D - 1: the oldest live tag
    assert _one(w, r, [0], [300]) == [0]                       # head = 9 = 1 + D = 2 + D - 1
    assert _one(w, r, [0], [200]) == []                        # insert 2 at head = 2 + D - 1: still live
    assert _one(w, r, [0], [100]) == [0]                       # insert 1 at head = 1 + D: kept; head = 10 = 2 + D
    assert _one(w, r, [0], [200]) == [0]                       # insert 2 at head = 2 + D: kept
    assert w.export().tolist() == [2, 3, 4, 5, 6, 300, 100, 200]


def test_tag0_passes_and_is_never_inserted(pair):
    w, r = pair
    assert _one(w, r, [0, 0, 0], [0, 0, 7]) == [0, 1, 2]
    assert w.export().tolist() == [7]
    assert _one(w, r, [0, 0], [0, 7]) == [0]


def test_failing_items_neither_insert_nor_suppress(pair):
    w, r = pair
    assert _one(w, r, [0], [7]) == [0]
    assert _one(w, r, [-3], [7]) == [] and w.export().tolist() == [7]          # a failing copy of a live tag
    assert _one(w, r, [-3, -1], [8, 9]) == [] and w.export().tolist() == [7]   # failing fresh tags
    assert _one(w, r, [-3, 0, 0], [8, 8, 8]) == [1]                            # a failing copy ahead of the fresh passing one
    assert w.export().tolist() == [7, 8]


def test_an_all_duplicate_submission(pair):
    w, r = pair
    assert _one(w, r, [0] * 4, [1, 2, 3, 4]) == [0, 1, 2, 3]
    assert _one(w, r, [0] * 8, [4, 3, 2, 1, 1, 2, 3, 4]) == []
    assert w.export().tolist() == [1, 2, 3, 4]


def test_a_tag_its_own_submission_evicts_still_counts(pair):
    """The window is queried as of the submission's start: 8 fresh tags push
    tag 1 out, and the copy of tag 1 behind them is dropped all the same."""
    w, r = pair
    assert _one(w, r, [0] * 8, range(1, 9)) == list(range(8))
    assert _one(w, r, [0] * 8, [11, 12, 13, 14, 15, 16, 17, 1]) == list(range(7))
    assert w.export().tolist() == [8, 11, 12, 13, 14, 15, 16, 17]


def test_more_items_than_depth_is_refused(pair):
    from firedancer_amd import ed25519
    w, r = pair
    assert _one(w, r, [0] * 3, [1, 2, 3]) == [0, 1, 2]
    keep = np.full(9, 0x55555555, np.uint32)
    e, t = _arr([0] * 9, range(10, 19))
    rc = ed25519.lib().fd_ed25519_amd_window_keep(w._h, 9, ed25519._ptr(e), ed25519._ptr(t), ed25519._ptr(keep))
    assert rc == 2**64 - 1 and (keep == 0x55555555).all() and w.export().tolist() == [1, 2, 3]
    with pytest.raises(ed25519.EngineError):
        w.keep(e, t)
    assert _one(w, r, [0] * 8, range(10, 18)) == list(range(8))                # n == depth is fine


def test_window_new_refuses_bad_depths():
    from firedancer_amd import ed25519
    for depth in (0, ed25519.WINDOW_DEPTH_MAX + 1):
        with pytest.raises(ed25519.EngineError):
            ed25519.Window(-1, depth)


@pytest.mark.parametrize("n", [1, 16, 65])
def test_equal_to_the_tcache_where_the_condition_holds(n):
    """Streams built so that no tag evicted during a submission sits on a
    passing item of it: keep lists and exported state equal the item-by-item
    model's, and the test checks the condition itself on every submission."""
    from firedancer_amd import ed25519
    depth, subs = conditioned_stream(n, n, 40 if n > 1 else 40 * 8)
    w, m = ed25519.Window(-1, depth), Tcache(depth)
    try:
        dups = evictions = 0
        for k, (err, tag) in enumerate(subs):
            want, evicted = m.keep(err, tag)
            assert not set(evicted) & set(tag[err == 0].tolist()), k          # the condition, in the test's own model
            got = w.keep(err, tag)
            assert np.array_equal(got, want), (k, got[:8], want[:8])
            assert np.array_equal(w.export(), m.export()), k
            dups += n - want.size
            evictions += len(evicted)
        assert dups > 0 and evictions >= 2 * depth
    finally:
        w.close()


@pytest.mark.parametrize("depth,n", [(8, 8), (64, 17), (64, 64)])
def test_never_keeps_what_the_tcache_drops(depth, n):
    """Unrestricted streams: from the same state, every item the item-by-item
    model drops the window drops too.  (Once their states differ the model is
    set to the window's, so every submission is compared.)"""
    from firedancer_amd import ed25519
    w, m = ed25519.Window(-1, depth), Tcache(depth)
    try:
        differed = 0
        for k, (err, tag) in enumerate(random_stream(depth + n, depth, n, 40 * depth // n)):
            m.ring = w.export().tolist()
            want, _ = m.keep(err, tag)
            got = w.keep(err, tag)
            assert set(got.tolist()) <= set(want.tolist()), k
            differed += got.size != want.size
        assert differed > 0                                                   # the streams do leave the condition
    finally:
        w.close()


def test_export_import_then_continue():
    from firedancer_amd import ed25519
    depth, n = 64, 17
    subs = random_stream(7, depth, n, 60)
    a, b = ed25519.Window(-1, depth, salt=1), None
    try:
        for err, tag in subs[:30]:
            a.keep(err, tag)
        state = a.export()
        assert state.size == depth
        b = ed25519.Window(-1, depth, salt=2)
        b.load(state)
        assert np.array_equal(b.export(), state)
        for k, (err, tag) in enumerate(subs[30:]):
            assert np.array_equal(a.keep(err, tag), b.keep(err, tag)), k
            assert np.array_equal(a.export(), b.export()), k
        for bad in ([0], [1, 0, 2], list(range(1, depth + 2))):               # a null tag; more than depth
            with pytest.raises(ed25519.EngineError):
                b.load(bad)
        assert np.array_equal(a.export(), b.export())
        b.load(state[:5])
        assert np.array_equal(b.export(), state[:5])
        b.load([])
        assert b.export().size == 0
    finally:
        a.close()
        if b:
            b.close()
