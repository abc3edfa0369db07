"""The dedup window's rule (include/fd_ed25519_amd.h, "The dedup window")
restated in plain Python, a sequential FD_TCACHE_INSERT model to compare it
with, and the (err, tag) stream generators both window tests run: the host
window (test_window_cpu.py) and the device window (test_window_gpu.py)."""
import numpy as np


class Rule:
    """The rule written straight from its text: T is the list of every tag
    ever inserted, the live tags are its last D entries."""

    def __init__(self, depth):
        self.D, self.T = int(depth), []

    def live(self):
        return self.T[max(0, len(self.T) - self.D):]

    def keep(self, err, tag):
        err, tag = np.asarray(err).tolist(), np.asarray(tag).tolist()
        assert len(err) <= self.D
        live = set(self.live())                # the window as it stands when the submission starts
        seen, out, ins = set(), [], []
        for i, (e, t) in enumerate(zip(err, tag)):
            if e != 0:
                continue
            if t != 0:
                first = t not in seen
                seen.add(t)                    # every passing item occupies its tag, a dropped one too
                if not first or t in live:
                    continue
                ins.append(t)
            out.append(i)
        self.T += ins                          # the survivors with a nonzero tag, ascending i
        return np.array(out, np.uint32)

    def export(self):
        return np.array(self.live(), np.uint64)


class Tcache:
    """FD_TCACHE_INSERT item by item (src/tango/tcache/fd_tcache.h:372-403):
    a passing nonzero tag that is in the cache is a duplicate; otherwise it
    evicts the oldest once the cache holds D and goes in."""

    def __init__(self, depth):
        self.D, self.ring = int(depth), []     # oldest first, at most D

    def keep(self, err, tag):
        """(survivors, the tags evicted while this submission ran)."""
        out, evicted = [], []
        for i, (e, t) in enumerate(zip(np.asarray(err).tolist(), np.asarray(tag).tolist())):
            if e != 0:
                continue
            if t != 0:
                if t in self.ring:
                    continue
                if len(self.ring) == self.D:
                    evicted.append(self.ring.pop(0))
                self.ring.append(t)
            out.append(i)
        return np.array(out, np.uint32), evicted

    def export(self):
        return np.array(self.ring, np.uint64)


def _arr(err, tag):
    return np.ascontiguousarray(err, np.int8), np.ascontiguousarray(tag, np.uint64)


def tag_of(k, pattern="mix"):
    """The k-th fresh tag (k >= 1) of a pattern: "mix" well spread 64-bit
    values; "top16" k << 48 | 1, which differ only in bits a weak slot function
    would ignore.  Never 0."""
    if pattern == "top16":
        return ((k & 0xFFFF) << 48) | 1 | ((k >> 16) << 1)
    x = (k * 0x9E3779B97F4A7C15) & (2**64 - 1)
    x ^= x >> 29
    return x | 1


def random_stream(seed, depth, n, calls, pattern="mix", hist=()):
    """`calls` submissions of n items against a window of `depth`: per item a
    verdict from {0, 0, 0, -1, -3}, and a tag that is fresh (a counter), the
    null tag, a copy of an item of this submission, or one of the last 2 depth
    tags ever offered -- live, just expired and long expired ones.  hist: tags
    offered before the stream starts (a window loaded with them), none of
    them a tag_of value below 2^40."""
    rng = np.random.default_rng(seed)
    hist, k, out = list(hist), 0, []
    for _ in range(calls):
        err = rng.choice(np.array([0, 0, 0, -1, -3], np.int8), n)
        tag = []
        for i in range(n):
            u = rng.random()
            if u < 0.05:
                t = 0
            elif u < 0.20 and tag:
                t = tag[int(rng.integers(0, len(tag)))]
            elif u < 0.50 and hist:
                t = hist[-1 - int(rng.integers(0, min(len(hist), 2 * depth + 3)))]
            else:
                k += 1
                t = tag_of(k, pattern)
            tag.append(t)
        hist += [t for t in tag if t]
        out.append(_arr(err, tag))
    return out


def conditioned_stream(seed, n, calls):
    """Submissions on which the rule and the item-by-item tcache agree
    exactly: depth = 4 n, every item passes, fresh tags from a counter, and
    duplicates drawn only from the newest depth - 2 n tags inserted before the
    submission -- a submission evicts at most n tags, the oldest ones, so none
    of them sits on one of its items.  Returns (depth, submissions)."""
    depth = 4 * n
    rng = np.random.default_rng(seed)
    model, k, out = Tcache(depth), 0, []
    for _ in range(calls):
        young = model.ring[max(0, len(model.ring) - (depth - 2 * n)):]
        tag = []
        for i in range(n):
            if young and rng.random() < 0.3:
                tag.append(young[int(rng.integers(0, len(young)))])
            else:
                k += 1
                tag.append(tag_of(k))
        sub = _arr(np.zeros(n, np.int8), tag)
        model.keep(*sub)
        out.append(sub)
    return depth, out
