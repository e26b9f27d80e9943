"""libecc_amd/csrc/ecamd_eddsa_msgs.h on the host (tests/eddsa_msgs_host_shim.cpp, g++): (a) what tests/golden/eddsa_msgs.json -- the
unmodified reference's keys, signatures and verdicts -- covers; (b) the fixture regenerated from the reference where oracle/_ref is built;
(c) the per-item steps over a packed array whose message starts fall at all eight residues mod 8: the verifier's hram, and the signer's
a, r_hash and hram, against hashlib for every fixture case, and tied to the REFERENCE's signature through S = r_hash + hram a mod q;
(d) item_ok on its edges and unusable items; (e) the same walk as a stand-alone program under -fsanitize=address,undefined over an
array with no slack before its first and behind its last octet; (f) the public names."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

import oracles as O
import eddsa_sign_ref as E
import eddsa_msgs_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ec_eddsa_verify_msgs_batch", "ec_eddsa_verify_msgs_all_batch", "ec_eddsa_sign_msgs_batch"]


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture()


def packed(items, lead=0):
    """the messages back to back behind `lead` octets: (array, offsets).  The lengths of the fixture are mixed, so the starts take every
    residue mod 8 (asserted by the caller where it matters)."""
    offs, pos = [lead], lead
    for it in items:
        pos += len(it["msg"])
        offs.append(pos)
    return b"\xee" * lead + b"".join(it["msg"] for it in items), offs


def test_what_the_fixture_covers(fx):
    assert D.ALGS == [9, 10, 11, 12, 13] and list(fx["cases"]) == D.NAMES
    assert os.path.getsize(D.FIXTURE) <= 100 * 1024
    parts = []
    for alg in D.ALGS:
        cs, items = D.cases(alg), D.fixture_items(fx, alg)
        lens = {m for _, m in cs}
        assert set(D.BASE_LENS) | {D.PAST_SLOT, D.LONG} <= lens
        assert {c for c, _ in cs} == ({0, 1, 255} if E.takes_ctx(alg) else {None})
        cov = D.coverage(alg)
        assert set(cov) == ({"prehash"} if E.is_ph(alg) else {"r_hash", "hram"}) and all(v == set(D.edges(alg)) for v in cov.values())
        for it in items:
            kinds = [v[0] for v in it["variants"]]
            assert kinds == [k for k in D.KINDS if it["msg"] or k != "msg"]
            assert [v[4] for v in it["variants"]] == [0] + [-1] * (len(kinds) - 1)
            assert len(it["pub"]) == E.klen(alg) and len(it["sig"]) == 2 * E.klen(alg)
        parts += [it["pub"] for it in items] + [it["sig"] for it in items]
    assert D.hashlib.sha256(b"".join(parts)).hexdigest() == fx["sha256"]


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_eddsa_msgs_fixture as G
    with open(D.FIXTURE) as f:
        assert G.dumps(G.build()) == f.read()


@pytest.mark.parametrize("alg", D.ALGS)
def test_steps_over_a_packed_array(fx, alg):
    kl, q = E.klen(alg), D.order(alg)
    starts = set()
    for adata, items in D.by_context(D.fixture_items(fx, alg)).items():
        for lead in range(8):
            arr, offs = packed(items, lead)
            for i, it in enumerate(items):
                if lead and len(it["msg"]) > 300 and i % 8 != lead:    # the long ones: behind one lead each
                    continue
                starts.add(offs[i] % 8)
                R_enc, S = it["sig"][:kl], int.from_bytes(it["sig"][kl:], "little")
                bad, vh = D.shim_vhram(alg, adata, R_enc, it["pub"], arr, offs[i], offs[i + 1])
                assert bad == 0 and vh == E.hram(alg, adata, R_enc, it["pub"], it["msg"]), (alg, i, lead)
                bad, a, rh, sh = D.shim_sign_hashes(alg, adata, it["sk"], R_enc, it["pub"], arr, offs[i], offs[i + 1])
                assert bad == 0 and a == E.expand(alg, it["sk"])[0] and sh == vh, (alg, i, lead)
                assert rh == E.r_hash(alg, it["sk"], adata, it["msg"]), (alg, i, lead)
                # the reference's S from the unit's two hashes (sig/eddsa.c:1847-1857)
                assert (int.from_bytes(rh, "little") + int.from_bytes(sh, "little") * int.from_bytes(a, "little")) % q == S, (alg, i)
    assert starts == set(range(8)), starts


def test_item_ok_edges():
    ok = D.shim().edm_item_ok
    lim, big = D.MAX_HASHED, 1 << 40
    for alg in D.ALGS:
        kl = E.klen(alg)
        for dl in (0, 35, 289):
            fixed = 0 if E.is_ph(alg) else dl + 2 * kl
            assert ok(alg, 0, 0, 0, dl) == 1 and ok(alg, 5, 5, 5, dl) == 1
            assert ok(alg, 6, 5, 10, dl) == 0                                        # decreasing offsets
            assert ok(alg, 0, 11, 10, dl) == 0 and ok(alg, 11, 11, 10, dl) == 0      # off1 > total
            assert ok(alg, 3, 3 + lim - fixed, big, dl) == 1 and ok(alg, 3, 4 + lim - fixed, big, dl) == 0   # exactly 2^28, and one more
            assert ok(alg, big, big + 100, big + 100, dl) == 1 and ok(alg, big + 1, big, big + 100, dl) == 0
            assert ok(alg, 1, (1 << 32) + 1, 1 << 33, dl) == 0                       # a length whose low 32 bits are zero is no empty message
            assert ok(alg, 2 ** 64 - 1, 2 ** 64 - 1, 10, dl) == 0                    # what the host form gives an offset outside its piece
            assert ok(alg, 0, 2 ** 64 - 1, 2 ** 64 - 1, dl) == 0
    assert ok(8, 0, 0, 0, 0) == -1 and ok(14, 0, 0, 0, 0) == -1


@pytest.mark.parametrize("alg", D.ALGS)
def test_unusable_items_read_nothing(alg):
    kl = E.klen(alg)
    R_enc, A_enc, sk = bytes(range(kl)), bytes(range(1, kl + 1)), bytes(range(2, kl + 2))
    adata = b"c" if E.takes_ctx(alg) else None
    for off0, off1, total in ((9, 8, 40), (8, 41, 40), (8, 33, 32)):
        # a NULL array: the unit must not touch it
        assert D.shim_vhram(alg, adata, R_enc, A_enc, None, off0, off1, total) == (1, bytes(2 * kl))
        bad, a, rh, sh = D.shim_sign_hashes(alg, adata, sk, R_enc, A_enc, None, off0, off1, total)
        # the signer hashes an empty message for it (its signature is zeroed behind the core)
        assert bad == 1 and a == E.expand(alg, sk)[0] and rh == E.r_hash(alg, sk, adata, b"") and sh == E.hram(alg, adata, R_enc, A_enc, b"")


@pytest.mark.parametrize("alg", D.ALGS)
def test_stand_alone_sanitizer_walk(fx, alg):
    """every fixture case of the variant, one batch per context: the packed array is a heap block of exactly its length, the first
    message begins at its first octet and the last one ends at its last"""
    exe = D.build_shim(main=True)
    kl = E.klen(alg)
    for adata, items in D.by_context(D.fixture_items(fx, alg)).items():
        arr, offs = packed(items)
        ad = adata or b""
        blob = struct.pack("<3I", len(items), alg, len(ad)) + ad
        blob += b"".join(it["sk"] + it["sig"][:kl] + it["pub"] for it in items) + struct.pack("<%dQ" % len(offs), *offs) + arr
        r = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"host walk done (%d items)" % len(items) in r.stderr
        got = r.stdout.decode().split()
        want = []
        for it in items:
            h = E.hram(alg, adata, it["sig"][:kl], it["pub"], it["msg"])
            want += [h.hex(), E.expand(alg, it["sk"])[0].hex(), E.r_hash(alg, it["sk"], adata, it["msg"]).hex(), h.hex()]
        assert got == want


def test_public_names():
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in SYMBOLS:
        assert "int %s(" % sym in header and "int %s_dev(" % sym in header, sym
    import libecc_amd.api
    for m in ("eddsa_verify_msg_list", "eddsa_verify_msg_list_all", "eddsa_sign_msg_list"):
        assert hasattr(libecc_amd.api.Curve, m) and hasattr(libecc_amd.api.Curve, m + "_dev"), m
    lib = libecc_amd.api.lib_path()
    if os.path.exists(lib):
        L = C.CDLL(lib)
        for sym in SYMBOLS:
            assert hasattr(L, sym) and hasattr(L, sym + "_dev"), sym
