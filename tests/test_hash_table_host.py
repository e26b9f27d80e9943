"""SHA-3, SHA-512/t, RIPEMD-160 and BASH on the CPU: libecc_amd/csrc/ecamd_keccak.h, ecamd_sha512t.h, ecamd_rmd160.h and ecamd_bash.h
-- the per-item code of k_sha3_slots, k_sha512t_slots, k_rmd160_slots and k_bash_slots -- compiled with g++
(tests/hash_table_host_shim.cpp, no HIP) against every known answer that tests/golden/hash_table.json records from the unmodified
reference, against hashlib where it offers the hash, and once as a stand-alone binary under the address and undefined-behaviour
sanitizers (never loaded into Python)."""
import ctypes as C
import os
import random
import subprocess

import pytest

import libecc_amd
import hashtable_ref as T


@pytest.fixture(scope="module")
def fx():
    return T.load_fixture()


@pytest.fixture(scope="module")
def kats(fx):
    return T.kat_table(fx)


def test_fixture_covers_what_it_must(fx, kats):
    assert set(kats) == set(T.TABLE)
    for name, rows in kats.items():
        b = T.BLOCKS[name]
        want = {0, 1, b - 2, b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1, 4092}
        if name == "RIPEMD160":
            want |= {55, 56}
        if name.startswith("SHA512_"):
            want |= {111, 112}
        assert set(rows) == want == set(T.kat_lengths(name)), name
        assert all(len(d) == T.HASH_SIZES[name] for d in rows.values())
    assert set(fx["items"]) == {"%s/%s/%s" % c for c in T.COMBOS}
    for key, rows in fx["items"].items():
        assert [r["ret"] for r in rows] == [0, 0, -1, -1], key
        assert all(r["sig"] == r["signed"] for r in rows[:2]) and all(r["sig"] != r["signed"] for r in rows[2:])
    assert os.path.getsize(T.FIXTURE) < (1 << 18)


def test_sizes_and_blocks_of_the_units():
    L = T.shim()
    for name, (ht, hs, bs, _, _) in T.TABLE.items():
        blk = C.c_int(0)
        assert L.ht_sizes(ht, C.byref(blk)) == hs and blk.value == bs, name
        assert libecc_amd.api.DIGEST_SIZES[ht] == hs
    for ht in (0, 1, 2, 3, 4, 11, 12, 13, 14, 16, 21, -1):
        assert L.ht_sizes(ht, None) == 0
    assert {ht: libecc_amd.api.DIGEST_SIZES[ht] for ht in T.OLD_IDS} == T.OLD_IDS
    assert set(libecc_amd.api.DIGEST_SIZES) == set(T.ALL_SIZES) == set(range(1, 21)) - {12, 16}


def test_kats_through_the_headers(kats):
    for name, rows in kats.items():
        for n, dg in rows.items():
            assert T.shim_hash(name, T.counting(n)) == dg, (name, n)


def test_hashlib_agrees_where_it_offers_the_hash(kats):
    """hashlib for SHA-3 always; sha512_224, sha512_256 and ripemd160 wherever this Python's hashlib has them.  The fixture is the
    authority where it does not."""
    for name in T.TABLE:
        if not T.have_hashlib(name):
            assert not name.startswith("SHA3_"), name
            continue
        for n, dg in kats[name].items():
            assert T.py_hash(name, T.counting(n)) == dg, (name, n)
        for n in range(0, 2 * T.BLOCKS[name] + 2):
            m = T.counting(n)[::-1]
            assert T.shim_hash(name, m) == T.py_hash(name, m), (name, n)


def test_sha3_at_random_lengths():
    rnd = random.Random(1902)
    for name in ("SHA3_224", "SHA3_256", "SHA3_384", "SHA3_512"):
        for _ in range(200):
            m = rnd.randbytes(rnd.randrange(0, 4093))
            assert T.shim_hash(name, m) == T.py_hash(name, m), (name, len(m))


def test_bash_round_constants_follow_the_standards_rule():
    """C_1 = 3bf5080ac8ba94b1; C_(t+1) = C_t >> 1, XORed with dc2be1997fe0d8ae where C_t is odd"""
    L = T.shim()
    c = 0x3bf5080ac8ba94b1
    for t in range(24):
        assert L.ht_bash_rc(t) == c, t
        c = (c >> 1) ^ (0xdc2be1997fe0d8ae if c & 1 else 0)


def test_a_slot_that_does_not_fit_gives_zeros(kats):
    L = T.shim()
    for name in T.TABLE:
        ht, hs = T.HASH_IDS[name], T.HASH_SIZES[name]
        out = C.create_string_buffer(64)
        msg = T.counting(36)
        assert L.ht_slot(ht, T.slot(msg, 40), 40, out) == hs and out.raw[:hs] == T.shim_hash(name, msg)
        for field in (37, 40, 4096, 0xffffffff):
            out = C.create_string_buffer(b"\xff" * 64, 64)
            assert L.ht_slot(ht, T.slot(msg, 40, length=field), 40, out) == hs
            assert out.raw[:hs] == bytes(hs) and out.raw[hs:] == b"\xff" * (64 - hs), (name, field)


def test_stand_alone_program_under_the_sanitizers(kats, tmp_path):
    """every known answer at the smallest stride that holds it (4092 at 4096), and length fields that do not fit their stride, through
    the slot code on heap slots of exactly the stride"""
    exe = T.build_shim(main=True)
    lines = []
    for name, rows in kats.items():
        ht, hs = T.HASH_IDS[name], T.HASH_SIZES[name]
        for n, dg in rows.items():
            m = T.counting(n)
            lines.append("H %d %d %d %s %s" % (ht, (4 + n + 3) & ~3, n, m.hex() or "-", dg.hex()))
        for stride, field in ((4, 1), (40, 37), (4096, 4093), (64, 0xffffffff)):
            lines.append("H %d %d %d %s %s" % (ht, stride, field, T.counting(stride - 4).hex() or "-", bytes(hs).hex()))
    vec = tmp_path / "vectors.txt"
    vec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(vec)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "checked %d bad 0" % len(lines)
