"""Write the directed grammar-limit transaction payloads (tests/_txn.py:
limit_cases) as one packed file for oracle/txn_limits_check.c:

    python tools/gen_txn_limits.py OUT.bin

little endian: u32 count, count x { u32 sz, payload[sz] }.  CPU only.
"""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import _txn  # noqa: E402


def main(out):
    cases = _txn.limit_cases()
    with open(out, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, p in cases:
            f.write(struct.pack("<I", len(p)) + p)
    print("%s: %d payloads" % (out, len(cases)))


if __name__ == "__main__":
    main(sys.argv[1])
