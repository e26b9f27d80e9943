"""SM3, Streebog and SM2's Z on the CPU: libecc_amd/csrc/ecamd_sm3.h, ecamd_streebog.h and ecamd_sm2z.h -- the per-item code of
k_sm3_slots, k_streebog_slots and k_sm2_z -- compiled with g++ (tests/sighash2_host_shim.cpp, no HIP) against every hash known answer
and every Z that tests/golden/sig_msg.json records from the unmodified reference; and the same program once as a stand-alone binary
under the address and undefined-behaviour sanitizers (never loaded into Python)."""
import hashlib
import os
import subprocess

import pytest

import oracles as O
import sigmsg_ref as M


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture()


def test_fixture_covers_what_it_must(fx):
    for name in ("SM3", "STREEBOG256", "STREEBOG512"):
        lens = [len(i["msg"]) // 2 for i in fx["hash"] if i["hash"] == name]
        assert lens[:len(M.KAT_LENGTHS)] == M.KAT_LENGTHS
        if name != "SM3":
            ff = [i for i in fx["hash"] if i["hash"] == name and i["msg"] and set(i["msg"]) == {"f"}]
            assert sorted(len(i["msg"]) // 2 for i in ff) == [64, 128, 192]
    combos = {(i["alg"], i["hash"], i["curve"]) for i in fx["verify"]}
    assert set(M.COMBOS) <= combos and ("SM2", "SM3", "SM2P256TEST") in combos
    assert {(i["alg"], i["hash"], i["curve"]) for i in fx["sign"]} >= set(M.COMBOS)
    ids = {len(i["id"]) // 2 for i in fx["verify"] if i["alg"] == "SM2" and i["family"].startswith("id_len")}
    assert ids == {0, 16, 62, 63}
    assert os.path.getsize(M.FIXTURE) < (1 << 20)


def test_hash_kats_through_the_headers(fx):
    for i in fx["hash"]:
        msg = bytes.fromhex(i["msg"])
        assert M.shim_hash(i["hash"], msg).hex() == i["digest"], (i["hash"], len(msg))


def test_sm3_equals_hashlib_and_the_streamed_form(fx):
    import ctypes as C
    for i in fx["hash"]:
        if i["hash"] != "SM3":
            continue
        msg = bytes.fromhex(i["msg"])
        assert hashlib.new("sm3", msg).hexdigest() == i["digest"]
        out = C.create_string_buffer(32)
        M.shim().s2_sm3_streamed(msg, len(msg), out)
        assert out.raw.hex() == i["digest"], len(msg)


def test_streebog_table_is_linear_in_pi(fx):
    """T[j][b] is the XOR of the rows that the set bits of pi(b) select: pi(b) = 0 gives 0, and the entries of two octets whose
    substitutes differ in one bit differ by one row of A"""
    L = M.shim()
    zero = [b for b in range(256) if all(L.s2_table_entry(j, b) == 0 for j in range(8))]
    assert len(zero) == 1
    for j in range(8):
        assert len({L.s2_table_entry(j, b) for b in range(256)}) == 256      # l is invertible
    assert L.s2_table_entry(7, 0x2D) == 0x83478b07b2468764      # pi(0x2D) = 1: row 7 of A in octet 7
    assert L.s2_table_entry(0, 0x2D) == 0x641c314b2b8ee083      # ... row 63 in octet 0


def test_every_z_and_digest_of_the_fixture(fx):
    seen = set()
    for i in fx["verify"] + fx["sign"]:
        msg, pub = bytes.fromhex(i["msg"]), bytes.fromhex(i["pub"])
        if i["alg"] != "SM2":
            assert M.shim_hash(i["hash"], msg).hex() == i["digest"]
            continue
        ident = bytes.fromhex(i["id"])
        z, absorbed, tail = M.shim_z(i["hash"], i["curve"], ident, pub)
        assert z.hex() == i["z"], (i["family"], len(ident))
        assert absorbed + tail == 2 + len(ident) + 4 * O.clen(i["curve"]) and absorbed % 64 == 0 and tail < 64
        seen.add((len(ident), tail))
        assert M.shim_hash(i["hash"], z + msg).hex() == i["digest"]
    assert (62, 0) in seen and (63, 1) in seen      # the prefix that ends on a block boundary, and one octet past it


def test_standalone_program_under_sanitizers(fx, tmp_path):
    vec = tmp_path / "vectors.txt"
    lines = ["H %d %s %s" % (M.HASH_IDS[i["hash"]], i["msg"] or "-", i["digest"]) for i in fx["hash"]]
    for i in fx["verify"] + fx["sign"]:
        if i["alg"] != "SM2":
            continue
        c, cl = O.CURVES[i["curve"]], O.clen(i["curve"])
        lines.append("Z %d %s %s %s %s %s %s %s" % (M.HASH_IDS[i["hash"]], i["id"] or "-", c["a"].to_bytes(cl, "big").hex(),
                                                    c["b"].to_bytes(cl, "big").hex(), c["gx"].to_bytes(cl, "big").hex(),
                                                    c["gy"].to_bytes(cl, "big").hex(), i["pub"], i["z"]))
    vec.write_text("\n".join(lines) + "\n")
    exe = M.build_shim(main=True)
    r = subprocess.run([exe, str(vec)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checked %d bad 0" % len(lines)), r.stdout
