"""The survivor rule (include/fd_ed25519_amd.h, "Survivors") restated in
Python, and the directed (err, tag) cases both keep tests run: the host
reference (test_keep_cpu.py) and the device filter (test_keep_gpu.py)."""
import numpy as np


def rule(err, tag):
    """Item i survives iff err[i] == 0 and (tag[i] == 0 or no earlier passing
    item has tag[i]).  Returns the survivors' indices, ascending, uint32."""
    seen, out = set(), []
    for i, (e, t) in enumerate(zip(np.asarray(err).tolist(), np.asarray(tag).tolist())):
        if e != 0:
            continue
        if t != 0 and t in seen:
            continue
        seen.add(t)
        out.append(i)
    return np.array(out, np.uint32)


def random_case(seed, n, ntag):
    """n items: tags drawn from ntag values (the null tag one of them),
    verdicts from {0, -1, -2, -3, -4}."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(1, 2**64, ntag, dtype=np.uint64)
    pool[0] = 0
    return (rng.choice(np.array([0, -1, -2, -3, -4], np.int8), n), pool[rng.integers(0, ntag, n)])


def _arr(err, tag):
    return np.ascontiguousarray(err, np.int8), np.ascontiguousarray(tag, np.uint64)


CASES = {
    "n0": _arr([], []),
    "n1_pass": _arr([0], [9]),
    "n1_fail": _arr([-3], [9]),
    "all_fail": _arr([-1, -2, -3, -4] * 8, list(range(1, 33))),
    "all_same_tag": _arr([0] * 40, [0xDEADBEEF00000001] * 40),
    "tag0_repeated": _arr([0] * 17, [0] * 17),
    "failing_copy_first": _arr([-3, 0, 0], [77, 77, 77]),          # only the middle one is kept
    "random_4096": random_case(4096, 1 << 12, 64),
}
