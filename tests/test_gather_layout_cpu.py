"""CPU: fd_ed25519_amd_gather_layout, the one rule that sizes a chunk of
verify_batch_registered -- the first signature always, further ones while the
count stays <= cap and the padded total (sizes rounded up to 16) stays <=
blob_cap -- and its Python mirror ed25519.gather_layout.  No device."""
import numpy as np
import pytest

from firedancer_amd import ed25519


def _both(sz, cap, blob_cap):
    """(count, dst) of the C function, checked equal to the Python mirror's."""
    c, dst = ed25519.gather_layout_c(sz, cap, blob_cap)
    pc, pdst = ed25519.gather_layout(sz, cap, blob_cap)
    assert c == pc and np.array_equal(dst, pdst), (list(sz)[:8], cap, blob_cap)
    return c, dst


def _pad(s):
    return (int(s) + 15) & ~15


def test_edge_sizes_and_offsets():
    sz = [0, 1, 15, 16, 17, 1232]
    c, dst = _both(sz, 64, 1 << 20)
    assert c == 6
    assert dst.tolist() == [0, 0, 16, 32, 48, 80]          # 0 -> 0, 1 -> 16, 15 -> 16, 16 -> 16, 17 -> 32
    assert dst[-1] + _pad(1232) == 80 + 1232


def test_offsets_aligned_ascending_disjoint():
    rng = np.random.default_rng(1)
    sz = rng.integers(0, 1233, 500)
    c, dst = _both(sz, 1000, 1 << 30)
    assert c == 500
    assert (dst % 16 == 0).all()
    end = dst.astype(np.int64) + np.array([_pad(s) for s in sz])
    assert (dst[1:].astype(np.int64) >= end[:-1]).all()     # each padded range starts at or after the previous one's end
    assert (np.diff(dst.astype(np.int64)) >= 0).all()


def test_message_of_exactly_blob_cap_is_taken_alone():
    """blob_cap not a multiple of 16: the padded size passes it, and the first signature is taken all the same."""
    blob_cap = 1232 + 7
    c, dst = _both([blob_cap, 0, 0], 64, blob_cap)
    assert c == 1 and dst.tolist() == [0]
    # the same message later in the list ends the chunk before it, then opens the next one
    c, dst = _both([16, blob_cap], 64, blob_cap)
    assert c == 1
    c, dst = _both([blob_cap], 64, blob_cap)
    assert c == 1 and dst.tolist() == [0]


def test_chunk_ends_at_cap():
    c, dst = _both([10] * 100, 64, 1 << 20)
    assert c == 64 and dst.tolist() == [16 * k for k in range(64)]
    c, _ = _both([10] * 64, 64, 1 << 20)
    assert c == 64
    c, _ = _both([10] * 5, 1, 1 << 20)
    assert c == 1


def test_chunk_ends_where_the_next_padded_size_would_pass_blob_cap():
    # 3 x 1232 -> 3696 padded bytes; a fourth would make 4928 > 4096
    c, dst = _both([1232] * 10, 64, 4096)
    assert c == 3 and dst.tolist() == [0, 1232, 2464]
    # padded, not raw, sizes count: 4 x 1 B are 64 padded bytes
    c, _ = _both([1] * 10, 64, 64)
    assert c == 4
    c, _ = _both([1] * 10, 64, 63)
    assert c == 3
    # exactly full
    c, dst = _both([16] * 10, 64, 48)
    assert c == 3 and dst.tolist() == [0, 16, 32]


def test_all_zero_sizes_take_cap():
    c, dst = _both([0] * 300, 200, 1232)
    assert c == 200 and not dst.any()
    c, dst = _both([0] * 100, 200, 1232)
    assert c == 100


def test_empty():
    assert _both([], 64, 4096)[0] == 0
    assert _both(np.zeros(0, np.uint64), 1, 1)[0] == 0


def test_python_mirror_equals_c_on_random_lists():
    rng = np.random.default_rng(20262)
    for k in range(1000):
        n = int(rng.integers(0, 80))
        top = int(rng.choice([1, 17, 300, 1233, 5000]))
        sz = rng.integers(0, top, n)
        cap = int(rng.integers(1, 70))
        blob_cap = int(rng.choice([1232, 1239, 4096, 5000, 20000, 1 << 20]))
        c, dst = _both(sz, cap, blob_cap)
        assert c <= cap and (n == 0 or c >= 1)
        if c:
            total = int(dst[c - 1]) + _pad(sz[c - 1])
            assert c == 1 or total <= blob_cap
            if c < n and c < cap:                           # ended on the blob bound: the next one does not fit
                assert int(sz[c]) > blob_cap or total + _pad(sz[c]) > blob_cap


def test_declared_and_exported():
    import test_abi
    assert "fd_ed25519_amd_gather_layout" in test_abi.declared_functions()
    assert "fd_ed25519_amd_verify_batch_registered" in test_abi.declared_functions()
    assert "fd_ed25519_amd_verify_batch_registered_tag" in test_abi.declared_functions()


def test_entry_points_refuse_null_arguments_without_a_device():
    """ERR_INVAL before any device call: no engine, or NULL arrays with n > 0."""
    L = ed25519.lib()
    assert L.fd_ed25519_amd_verify_batch_registered(None, 0, None, None, None, None, None) == -10
    assert L.fd_ed25519_amd_verify_batch_registered_tag(None, 4, None, None, None, None, None, None) == -10
