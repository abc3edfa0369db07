"""CPU: fd_ed25519_amd_keep, the survivor rule as pure host code
(include/fd_ed25519_amd.h, "Survivors"), against the restatement of the rule
in Python (_keep.rule).  No device."""
import numpy as np
import pytest

from _keep import CASES, rule

GUARD = 0xA5A5A5A5


def _raw(err, tag, keep):
    from firedancer_amd import ed25519
    P = ed25519._ptr
    return int(ed25519.lib().fd_ed25519_amd_keep(int(err.size), P(err), P(tag), P(keep) if keep is not None else None))


@pytest.mark.parametrize("name", sorted(CASES))
def test_keep_matches_the_rule(name):
    err, tag = CASES[name]
    want = rule(err, tag)
    n = int(err.size)
    keep = np.full(n + 4, GUARD, np.uint32)           # room for n, and guard words behind
    err0, tag0 = err.copy(), tag.copy()
    cnt = _raw(err, tag, keep)
    assert cnt == want.size
    assert np.array_equal(keep[:cnt], want)
    assert (keep[cnt:] == GUARD).all()                # nothing at or beyond keep[keep_cnt]
    assert np.array_equal(err, err0) and np.array_equal(tag, tag0)
    assert _raw(err, tag, None) == cnt                # keep == NULL only counts


def test_the_named_cases_are_what_they_say():
    assert rule(*CASES["failing_copy_first"]).tolist() == [1]
    assert rule(*CASES["all_same_tag"]).tolist() == [0]
    assert rule(*CASES["tag0_repeated"]).tolist() == list(range(17))
    assert rule(*CASES["all_fail"]).size == 0 and rule(*CASES["n0"]).size == 0
    e, t = CASES["random_4096"]
    k = rule(e, t)
    assert int((e == 0).sum()) > k.size > 64          # duplicates were dropped, tag 0 kept repeatedly
    assert set(np.unique(e).tolist()) == {0, -1, -2, -3, -4} and np.unique(t).size == 64


def test_module_function():
    from firedancer_amd import ed25519
    e, t = CASES["random_4096"]
    got = ed25519.keep(e, t)
    assert got.dtype == np.uint32 and np.array_equal(got, rule(e, t))
    assert ed25519.keep([], []).size == 0
