"""The independent RFC 8032 signer model (tests/_sign_ref.py) pinned to the
RFC's vectors and to the strict verifier, and the host signer
(fd_ed25519_public_from_private, fd_ed25519_sign, fd_ed25519_amd_sign_batch)
compared with it byte for byte on the directed corpus: message sizes at the
padding edges of both prefixed hashes, every start alignment, edge seeds.
Where oracle/_ref is built the comparison is three-way with the compiled
reference's own signer.  Every check is equality; nothing here needs a GPU."""
import numpy as np
import pytest

import _golden
import _oracle
import _sign_ref as S
import _strict_ref


def test_model_reproduces_rfc8032(golden):
    idx = np.nonzero(golden.cls == _golden.CLASSES.index("rfc8032"))[0]
    assert len(idx) == 3
    for k, i in enumerate(idx):
        seed = bytes.fromhex(S.RFC_SECRETS[k])
        pub, sig = S.sign(seed, golden.msg(i))
        assert pub == bytes(golden.pub[i]) and S.public_from_private(seed) == pub
        assert sig == bytes(golden.sig[i])


def test_model_pieces():
    ident, base = (1).to_bytes(32, "little"), (4 * pow(5, S.P - 2, S.P) % S.P).to_bytes(32, "little")
    assert S.scalarmult_base_enc(0) == ident and S.scalarmult_base_enc(S.L) == ident
    assert S.scalarmult_base_enc(1) == base and S.scalarmult_base_enc(S.L + 1) == base
    assert S.encode(S.add(S.B, S.B)) == S.scalarmult_base_enc(2)
    assert S.sc_muladd(S.L - 1, S.L - 1, S.L - 1) == 0 and S.sc_muladd(2, 3, 4) == 10


def test_corpus_covers_what_it_claims():
    c = S.corpus()
    n = len(c)
    assert n <= 400 and n % 64 != 0
    sizes = set(c.sz.tolist())
    for p in S.PREFIXES:
        for sz in range(256):
            if (p + sz) % 128 in S.EDGE_RESIDUES:
                assert sz in sizes, (p, sz)
    assert {0, 1, 7, 8, 9, 1232} <= sizes and {sz % 8 for sz in sizes} == set(range(8))
    # the block-count edges of both hashes
    assert {79, 80, 207, 208, 47, 48, 175, 176} <= sizes
    at = {}
    for o, sz in zip(c.off.tolist(), c.sz.tolist()):
        at.setdefault(sz, set()).add(o % 8)
    for sz, res in at.items():
        assert {r % 4 for r in res} == {0, 1, 2, 3}, sz
        if 1 <= sz <= 9:
            assert res == set(range(8)), sz
    # back to back: a gap of at most 7 filler bytes, none of them message bytes
    end = 0
    for o, sz in sorted(zip(c.off.tolist(), c.sz.tolist())):
        assert 0 <= o - end <= 7
        end = o + sz
    assert end + 8 == c.blob.size
    seeds = [bytes(r) for r in c.prv]
    assert bytes(32) in seeds and b"\xff" * 32 in seeds
    assert all(bytes.fromhex(s) in seeds for s in S.RFC_SECRETS)
    dup = [k for k in range(n) if seeds.count(seeds[k]) == 2]
    assert len(dup) == 2 and c.msg(dup[0]) != c.msg(dup[1])


def test_model_signatures_verify_strict():
    c = S.corpus()
    bad = [i for i in range(len(c)) if _strict_ref.verify(c.msg(i), c.sig[i], c.pub[i]) != 0]
    assert not bad, bad[:10]


def test_oracle_accepts_every_corpus_signature():
    """No corpus item is one of the reference's limb false rejects (about
    1.6e-6 per signature, deterministic): the verify side can use the corpus."""
    c = S.corpus()
    err = _oracle.verify_batch(_golden.Batch(c.pub, c.sig, c.off, c.sz, c.blob), nthread=4)
    assert (err == 0).all(), np.nonzero(err)[0][:10]


def test_host_sign_batch_matches_model():
    from firedancer_amd import ed25519
    c = S.corpus()
    pub, sig = ed25519.sign_batch(c.prv, c.blob, c.off, c.sz)
    msg = S.first_difference(c, pub, sig)
    assert msg is None, msg


def test_host_sign_batch_thread_count():
    from firedancer_amd import ed25519
    c = S.corpus()
    p1, s1 = ed25519.sign_batch(c.prv, c.blob, c.off, c.sz, nthread=1)
    p16, s16 = ed25519.sign_batch(c.prv, c.blob, c.off, c.sz, nthread=16)
    assert np.array_equal(p1, p16) and np.array_equal(s1, s16)
    msg = S.first_difference(c, p1, s1)
    assert msg is None, msg


def test_host_single_calls_match_model():
    """fd_ed25519_public_from_private and fd_ed25519_sign one call at a time:
    every corpus item, and the empty message (msg = NULL, sz = 0) under the
    directed seeds."""
    from firedancer_amd import ed25519
    c = S.corpus()
    for i in range(len(c)):
        seed = bytes(c.prv[i])
        pub = ed25519.public_from_private(seed)
        assert pub == bytes(c.pub[i]), ("pub", i)
        sig = ed25519.sign(c.msg(i), pub, seed)
        assert sig == bytes(c.sig[i]), ("R" if sig[:32] != bytes(c.sig[i, :32]) else "S", i, int(c.sz[i]))
    for seed in [bytes(32), b"\xff" * 32] + [bytes.fromhex(s) for s in S.RFC_SECRETS]:
        pub, sig = S.sign(seed, b"")
        assert ed25519.public_from_private(seed) == pub
        assert ed25519.sign(b"", pub, seed) == sig, seed.hex()      # the binding passes msg = NULL for size 0


def test_model_reference_host_three_way():
    """model = compiled reference = host signer on the whole corpus."""
    if _oracle.ref() is None:
        pytest.skip("oracle/_ref not built (no /root/reference on this host)")
    from firedancer_amd import ed25519
    c = S.corpus()
    n = len(c)
    rp, rs = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    for i in range(n):
        p, s = _oracle.ref_sign(c.prv[i], c.msg(i))
        rp[i], rs[i] = np.frombuffer(p, np.uint8), np.frombuffer(s, np.uint8)
    msg = S.first_difference(c, rp, rs)
    assert msg is None, "compiled reference: " + msg
    hp, hs = ed25519.sign_batch(c.prv, c.blob, c.off, c.sz)
    assert np.array_equal(hp, rp) and np.array_equal(hs, rs)
    for seed in [bytes(32), b"\xff" * 32]:
        assert _oracle.ref_sign(seed, b"") == S.sign(seed, b"")
