"""libecc_amd/csrc/ecamd_digest_msgs.h on the host (tests/digest_msgs_host_shim.cpp, g++): (a) every digest of
tests/golden/digest_msgs.json -- the unmodified reference's -- through the three-segment source; (b) hashlib where it has the hash;
(c) 200 seeded random (segment lengths, alignment) cases per hash against hashlib, or against the contiguous walk of the trait
(hmac_ht_ref.shim_hash) for the hashes hashlib lacks; (d) item_ok on its edges; (e) the fixture regenerated from the reference where
oracle/_ref is built; (f) the counts; (g) the shim as a stand-alone program under -fsanitize=address,undefined over every fixture case with
exact-size allocations."""
import os
import random
import struct
import subprocess
import sys

import pytest

import oracles as O
import hmac_ht_ref as M
import digest_msgs_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture()


def test_counts_are_pinned(fx):
    assert len(D.NAMES) == 18 and sorted(D.HASH_IDS[n] for n in D.NAMES) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20]
    assert sum(len(D.cases(n)) for n in D.NAMES) == 1256 == sum(len(fx["digests"][n]["tags"]) for n in D.NAMES)
    for name in D.NAMES:
        # the Merkle-Damgard hashes have 18 distinct totals; where the padding is one octet B - L and B - 1 are one length
        assert len(D.totals(name)) == (18 if D.length_field(name) > 1 else 17), name
        assert {4092, 4093, 4097, D.LONG} <= set(D.totals(name))
        assert D.coverage(name) == ({0, 1, 2, 3},) * 3, name
        assert D.cases(name)[0] == (0, 0, 0)                                     # all three segments empty
        assert any(c[0] and c[0] == c[1] + c[2] for c in D.cases(name)), name    # an empty message behind prefixes
    assert os.path.getsize(D.FIXTURE) <= 100 * 1024
    assert [len(v["sigs"]) for v in fx["proto"].values()] == [6, 6, 6] and list(fx["proto"]) == ["%s/%s" % p for p in D.PROTO]
    assert all(v["verdicts"] == [[0, -1, -1]] * 6 for v in fx["proto"].values())
    sums = [bytes.fromhex(fx["digests"][n]["all"]) for n in D.NAMES] + [bytes.fromhex(s) for v in fx["proto"].values() for s in v["sigs"]]
    assert D.checksum(sums) == fx["sha256"]


@pytest.mark.parametrize("name", D.NAMES)
def test_fixture_digests_through_the_unit(fx, name):
    """every case at every start offset mod 4 of its message in the array"""
    cs = D.cases(name)
    for lead in range(4):
        digs = []
        for idx in range(len(cs)):
            cp, ip, m = D.case_input(name, idx)
            if lead and len(m) > 5000 and idx % 4 != lead:    # the long ones: each start offset once
                digs.append(None)
                continue
            st, d = D.shim_digest(name, cp, ip, b"\xee" * lead + m, lead, lead + len(m))
            assert st == 0
            if M.have_hashlib(name):
                assert d == M.py_hash(name, cp + ip + m), (name, idx, lead)
            digs.append(d)
        if lead == 0:
            D.assert_digests(fx, name, digs)
            first = digs
        else:
            assert all(d is None or d == f for d, f in zip(digs, first)), (name, lead)


@pytest.mark.parametrize("name", D.NAMES)
def test_random_segments_and_alignments(name):
    rng = random.Random("digest_msgs/random/" + name)
    b = D.BLOCKS[name]
    arr = D.stream("digest_msgs/random/" + name, 4 * b + 600)
    for k in range(200):
        cpl, ipl = rng.choice([0, rng.randint(0, 256)]), rng.choice([0, rng.randint(0, 256)])
        mlen = rng.choice([rng.randint(0, 8), rng.randint(0, 3 * b + 9)])
        off0 = rng.randint(0, len(arr) - mlen)
        # the array ends where the message ends, or goes on behind it
        total = rng.choice([off0 + mlen, len(arr)])
        cp, ip = D.stream("cp/%s/%d" % (name, k), cpl), D.stream("ip/%s/%d" % (name, k), ipl)
        st, d = D.shim_digest(name, cp, ip, arr[:total], off0, off0 + mlen)
        x = cp + ip + arr[off0:off0 + mlen]
        assert st == 0 and d == (M.py_hash(name, x) if M.have_hashlib(name) else M.shim_hash(name, x)), (name, k, cpl, ipl, off0, mlen)


def test_item_ok_edges():
    ok = D.shim().dm_item_ok
    lim = D.MAX_HASHED
    assert ok(0, 0, 0, 0, 0) == 1 and ok(5, 5, 5, 0, 0) == 1 and ok(0, 7, 7, 256, 256) == 1
    assert ok(6, 5, 10, 0, 0) == 0                                       # decreasing offsets
    assert ok(0, 11, 10, 0, 0) == 0 and ok(11, 11, 10, 0, 0) == 0        # off1 > total
    assert ok(0, lim, lim, 0, 0) == 1 and ok(0, lim + 1, lim + 1, 0, 0) == 0
    assert ok(0, lim - 3, lim, 1, 2) == 1 and ok(0, lim - 3, lim, 2, 2) == 0 and ok(0, lim - 3, lim, 1, 3) == 0   # the sum exactly 2^28, and one more
    assert ok(3, lim - 509, lim, 256, 256) == 1 and ok(3, lim - 508, lim, 256, 256) == 0
    big = 1 << 40
    assert ok(big, big + 100, big + 100, 3, 5) == 1 and ok(big + 1, big, big + 100, 0, 0) == 0           # u64 values above 2^32
    assert ok(big, big + lim, big + lim, 0, 0) == 1 and ok(big, big + lim + 1, 2 * big, 0, 0) == 0
    assert ok(1, (1 << 32) + 1, 1 << 33, 0, 0) == 0                      # a length whose low 32 bits are zero is no empty message
    assert ok(0, 2 ** 64 - 1, 2 ** 64 - 1, 0, 0) == 0 and ok(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 256, 256) == 1
    assert ok(2 ** 64 - 1, 2 ** 64 - 1, 10, 0, 0) == 0                   # what the host form gives an offset outside its piece
    assert ok(0, 0, 0, 257, 0) == 0 and ok(0, 0, 0, 0, 257) == 0


def test_unusable_items_are_zero_with_status_one():
    for name in ("SHA256", "SHA3_384", "STREEBOG512", "BASH256"):
        arr = bytes(range(40))
        assert D.shim_digest(name, b"ab", b"c", arr, 9, 8) == (1, bytes(D.HASH_SIZES[name]))
        assert D.shim_digest(name, b"ab", b"c", arr, 8, 41) == (1, bytes(D.HASH_SIZES[name]))
        assert D.shim_digest(name, b"", b"", arr, 8, 33, total=32) == (1, bytes(D.HASH_SIZES[name]))


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_digest_msgs_fixture as G
    with open(D.FIXTURE) as f:
        assert G.dumps(G.build()) == f.read()


def test_stand_alone_sanitizer_walk(fx):
    """every fixture case, the message array allocated at exactly round_up(total, 4) octets with the message ending at its last octet,
    behind 0 .. 3 leading octets; the digests that come back are the fixture's"""
    exe = D.build_shim(main=True)
    blob, want = [], []
    for name in D.NAMES:
        tags = fx["digests"][name]["tags"]
        for idx, (t, cpl, ipl) in enumerate(D.cases(name)):
            cp, ip, m = D.case_input(name, idx)
            blob.append(struct.pack("<6I", D.HASH_IDS[name], cpl, ipl, idx & 3, len(m), 0) + cp + ip + m)
            want.append(tags[idx])
    r = subprocess.run([exe], input=b"".join(blob), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"host walk done (%d cases)" % len(want) in r.stderr
    got = r.stdout.decode().split()
    assert [g[:2 * D.TAG] for g in got] == want
