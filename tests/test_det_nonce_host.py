"""CPU tests of DBIGN's and BIP0340's nonce generators (libecc_amd/csrc/ecamd_dbign_nonce.h, ecamd_bip0340_nonce.h) through
tests/det_nonce_host_shim.cpp (g++, no HIP): (a) the headers against the Python restatements (tests/det_sign_ref.py) and the recorded
reference answers (tests/golden/det_sign.json) on every fixture item, the signature assembled from that k in Python integers;
(b) BelT's rolled cipher and scanning table against the unrolled one; (c) the fixture's conditions and, where oracle/_ref is built,
the fixture regenerated from the reference; (d) the shim as a stand-alone program under -fsanitize=address,undefined over the
fixture; (e) the kernels k_dbign_nonce<SCAN> and k_bip0340_nonce<ALG> themselves (libecc_amd/csrc/ecamd_detnonce.hip) lane by lane
over tests/hipstub; (f) the new symbols in header, binding and library."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import bign_ref as B
import schnorr_ref as S
import det_sign_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "det_sign.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "det_nonce_host_shim.cpp")
SYMBOLS = ["ec_dbign_nonce_batch", "ec_dbign_nonce_batch_dev", "ec_dbign_sign_batch", "ec_dbign_sign_batch_dev",
           "ec_bip0340_nonce_batch", "ec_bip0340_nonce_batch_dev", "ec_bip0340_sign_batch", "ec_bip0340_sign_batch_dev"]
u32 = C.c_uint32


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture(FIXTURE)


@pytest.fixture(scope="module")
def shimlib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "det_nonce_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM])
    lib = C.CDLL(so)
    u32p = C.POINTER(u32)
    lib.dn_dbign_nonce.argtypes = [C.c_int, C.c_char_p, u32p, u32, C.c_char_p, u32, C.c_char_p, u32, C.c_char_p, u32, C.c_char_p, u32p]
    lib.dn_bip_nonce.argtypes = [C.c_int, C.c_char_p, C.c_char_p, u32, C.c_char_p, C.c_char_p, u32, u32p, u32, C.c_char_p]
    lib.dn_belt_encrypt4.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    lib.dn_tag_hash.argtypes = [C.c_int, C.c_char_p, u32, C.c_char_p]
    lib.dn_slot_ok.argtypes = [u32] * 4
    lib.dn_blocks.argtypes = [u32]
    lib.dn_blocks.restype = u32
    return lib


@pytest.fixture(scope="module")
def kernlib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "det_nonce_kernel_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__shared__=static", "-I" + os.path.join(ROOT, "tests", "hipstub"),
                           "-o", so, os.path.join(ROOT, "tests", "det_nonce_kernel_host_shim.cpp")])
    lib = C.CDLL(so)
    u32p = C.POINTER(u32)
    lib.dk_dbign_batch.argtypes = [C.c_int, u32, C.c_char_p, C.c_char_p, u32, C.c_char_p, u32, C.c_char_p, u32, u32p, u32, C.c_char_p, C.c_char_p]
    lib.dk_bip_batch.argtypes = [C.c_int, u32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, u32, u32, u32p, u32, C.c_char_p,
                                 C.c_char_p]
    return lib


def qwords(curve):
    q = O.CURVES[curve]["q"]
    return (u32 * 17)(*[(q >> (32 * w)) & 0xFFFFFFFF for w in range(17)]), q.bit_length()


def shim_dbign(lib, scan, curve, priv, dg, oid, t):
    """(status, k, rejected candidates) of the header's generator"""
    qw, qbits = qwords(curve)
    k, r = C.create_string_buffer(O.qlen(curve)), u32(0)
    st = lib.dn_dbign_nonce(scan, priv, qw, qbits, dg, len(dg), oid, len(oid), t, len(t), k, C.byref(r))
    return st, int.from_bytes(k.raw, "big"), r.value


def shim_bip(lib, curve, h, priv, pub, aux, msg):
    qw, qbits = qwords(curve)
    k = C.create_string_buffer(O.qlen(curve))
    st = lib.dn_bip_nonce(D.HT[h], priv, pub, O.clen(curve), aux, msg, len(msg), qw, qbits, k)
    return st, int.from_bytes(k.raw, "big")


def bip_key(curve, i):
    """the item's key bytes; for a key the scheme refuses, the generator's point (it is not read for its value)"""
    x, q = int(i["x"], 16), O.CURVES[curve]["q"]
    return D.bip_pub(curve, x) if 0 < x < q else S.pt_bytes(curve, S._curve(curve)[4])


def test_fixture_covers_what_it_must(fx):
    assert list(fx["dbign"]) == D.DBIGN_CURVES and list(fx["bip0340"]) == D.BIP_CURVES and os.path.getsize(FIXTURE) < 1 << 19
    branches = set()
    for curve, items in fx["dbign"].items():
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        for h in D.DBIGN_HASHES:
            mine = [i for i in items if i["hash"] == h]
            branches.add(ql < 16 * D.blocks(D.HSIZE[h]))
            assert {len(i["t"]) > 0 for i in mine if i["family"] == "t"} == {True, False}, (curve, h)
            edge = {int(i["x"], 16): i["ret"] for i in mine if i["family"] == "x_edge"}
            # what the reference does with the edge keys, as recorded: x = 0 imports and signs, x = q does not import
            assert edge == ({0: 0, 1: 0, q - 1: 0, q: -2} if h in D.dbign_edge_hashes(curve) else {}), (curve, h)
            if curve in D.RETRY_CURVES:
                assert {min(i["rejects"], 2) for i in mine} == {0, 1, 2}, (curve, h)
            else:
                assert all(i["rejects"] == 0 for i in mine), (curve, h)     # these orders fill their bits: nothing to reject
        assert all((i["sig"] is not None) == (i["ret"] == 0) and len(i["x"]) == 2 * ql for i in items)
    assert branches == {True, False}
    assert {h for c in D.DBIGN_CURVES for h in D.dbign_edge_hashes(c)} == set(D.DBIGN_HASHES)
    assert {h for c in D.BIP_CURVES for h in D.bip_edge_hashes(c)} == set(D.BIP_HASHES)
    assert O.qlen("SECP521R1") == 66 and O.qlen("SECP224K1") == 29 and O.CURVES["SECP224K1"]["q"].bit_length() == 225
    assert O.CURVES["WEI25519"]["q"].bit_length() == 253
    for curve, items in fx["bip0340"].items():
        q = O.CURVES[curve]["q"]
        for h in D.BIP_HASHES:
            mine = [i for i in items if i["hash"] == h]
            block = 64 if D.HSIZE[h] <= 32 else 128
            got = sorted(D.nonce_input_len(curve, h, len(i["msg"]) // 2) % block for i in mine if i["family"] == "edge")
            assert got == [e for e in S.PAD_EDGES if e < block], (curve, h)
            if h not in D.bip_edge_hashes(curve):
                assert {i["family"] for i in mine} == {"edge"}
                continue
            top = (1 << (8 * O.qlen(curve))) - 1
            assert {0, top} < {int(i["aux"], 16) for i in mine if i["family"] == "aux"}
            edge = {int(i["x"], 16): i["ret"] == 0 for i in mine if i["family"] == "x_edge"}
            assert edge == {0: False, 1: True, q - 1: True, q: False}, (curve, h)
            assert {i["y_odd"] for i in mine if i["family"] == "parity"} == {0, 1}
    assert len(fx["dbign_vectors"]) == 3 and len(fx["bip0340_vectors"]) == 4
    assert {len(v["t"]) > 0 for v in fx["dbign_vectors"]} == {True, False}


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_det_sign_fixture as M
    with open(FIXTURE) as f:
        assert M.dumps(M.build()) == f.read()


def test_belt_rolled_cipher_and_scanning_table(shimlib):
    rng = np.random.default_rng(31)
    out = C.create_string_buffer(16)
    for _ in range(200):
        key, blk = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=16, dtype=np.uint8).tobytes()
        assert shimlib.dn_belt_encrypt4(key, blk, out) == 0
        assert out.raw == B.belt_encrypt(blk, key)
    for key, blk in ((bytes(32), bytes(16)), (b"\xff" * 32, b"\xff" * 16)):
        assert shimlib.dn_belt_encrypt4(key, blk, out) == 0 and out.raw == B.belt_encrypt(blk, key)


def test_tag_hashes_and_small_rules(shimlib):
    import hashlib
    for h in D.BIP_HASHES:
        out = C.create_string_buffer(D.HSIZE[h])
        for tag in (S.TAG_AUX, S.TAG_NONCE, S.TAG_CHALLENGE, b"", b"x" * 55):
            assert shimlib.dn_tag_hash(D.HT[h], tag, len(tag), out) == 0
            assert out.raw == hashlib.new(O.HASHLIB[h], tag).digest(), (h, tag)
    assert shimlib.dn_tag_hash(2, b"x" * 56, 56, C.create_string_buffer(32)) == -1
    assert [shimlib.dn_blocks(n) for n in (1, 15, 16, 28, 31, 32, 47, 48, 64, 114, 128)] == [2, 2, 2, 2, 2, 2, 2, 3, 4, 7, 8]
    # a BIP0340 slot holds 2 hsize + 2 clen fixed octets and fits the stride
    for ln, stride, want in ((127, 256, 0), (128, 256, 1), (252, 256, 1), (253, 256, 0), (0xFFFFFFFF, 256, 0), (128, 128, 0), (128, 132, 1)):
        assert shimlib.dn_slot_ok(ln, stride, 32, 32) == want, (ln, stride)


@pytest.mark.parametrize("curve", D.DBIGN_CURVES)
def test_dbign_generator_and_signature_on_the_fixture(shimlib, fx, curve):
    for i in fx["dbign"][curve]:
        priv, msg, oid, t = (bytes.fromhex(i[f]) for f in ("x", "msg", "oid", "t"))
        dg = D.H(i["hash"], msg)
        want = (0, int(i["k"], 16), i["rejects"])
        assert D.dbign_nonce_from_digest(curve, priv, dg, oid, t) == want
        for scan in (0, 1):
            assert shim_dbign(shimlib, scan, curve, priv, dg, oid, t) == want, (curve, i["hash"], i["family"], scan)
        st, sig = B.sign_digest(curve, oid, int(i["x"], 16), want[1], dg)
        assert (st, sig) == ((0, bytes.fromhex(i["sig"])) if i["ret"] == 0 else (1, bytes(B.sig_len(curve)))), (curve, i["hash"], i["family"])


def test_dbign_generator_on_the_reference_vectors_and_odd_digests(shimlib, fx):
    for v in fx["dbign_vectors"]:
        priv, msg, oid, t = (bytes.fromhex(v[f]) for f in ("x", "msg", "oid", "t"))
        dg = D.H(v["hash"], msg)
        st, k, rej = shim_dbign(shimlib, 1, v["curve"], priv, dg, oid, t)
        assert (st, k, rej) == D.dbign_nonce_from_digest(v["curve"], priv, dg, oid, t)
        assert B.sign_digest(v["curve"], oid, int(v["x"], 16), k, dg) == (0, bytes.fromhex(v["sig"]))
    # digests of every length class the call takes (hash_type 0: 1 .. 128 octets), OIDs and t at their limits
    rng = np.random.default_rng(45)
    for curve in ("BIGN256V1", "SECP224K1", "SECP521R1"):
        ql = O.qlen(curve)
        for hlen in (1, 15, 16, 17, 33, 47, 49, 80, 96, 113, 127, 128):
            for oid, t in ((b"", b""), (bytes(range(64)), bytes(range(64, 128))), (B.OID_BELT, b"\x01")):
                priv, dg = rng.integers(0, 256, size=ql, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=hlen, dtype=np.uint8).tobytes()
                want = D.dbign_nonce_from_digest(curve, priv, dg, oid, t)
                assert shim_dbign(shimlib, 0, curve, priv, dg, oid, t) == want and shim_dbign(shimlib, 1, curve, priv, dg, oid, t) == want
    qw, qbits = qwords("BIGN256V1")
    k, r = C.create_string_buffer(32), u32(0)
    assert shimlib.dn_dbign_nonce(0, bytes(32), qw, qbits, bytes(129), 129, b"", 0, b"", 0, k, C.byref(r)) == -1
    assert shimlib.dn_dbign_nonce(0, bytes(32), qw, qbits, bytes(32), 32, bytes(65), 65, b"", 0, k, C.byref(r)) == -1
    assert shimlib.dn_dbign_nonce(0, bytes(32), qw, qbits, bytes(32), 32, b"", 0, bytes(65), 65, k, C.byref(r)) == -1


@pytest.mark.parametrize("curve", D.BIP_CURVES)
def test_bip0340_generator_and_signature_on_the_fixture(shimlib, fx, curve):
    cl, ql = O.clen(curve), O.qlen(curve)
    for i in fx["bip0340"][curve]:
        priv, msg, aux = (bytes.fromhex(i[f]) for f in ("x", "msg", "aux"))
        x, h = int(i["x"], 16), i["hash"]
        ok = i["ret"] == 0
        want = (0, int(i["k"], 16)) if ok else (1, 0)
        assert D.bip_nonce(curve, h, x, int(i["aux"], 16), msg) == want
        assert shim_bip(shimlib, curve, h, priv, bip_key(curve, i), aux, msg) == want, (curve, h, i["family"])
        st, sig = S.sign(curve, S.BIP0340, h, x, want[1], msg)
        assert (st, sig) == ((0, bytes.fromhex(i["sig"])) if ok else (1, bytes(cl + ql))), (curve, h, i["family"])
    if curve == "SECP256K1":
        for v in fx["bip0340_vectors"]:
            priv, msg, aux = (bytes.fromhex(v[f]) for f in ("x", "msg", "aux"))
            x = int(v["x"], 16)
            st, k = shim_bip(shimlib, curve, v["hash"], priv, D.bip_pub(curve, x), aux, msg)
            assert (st, k) == D.bip_nonce(curve, v["hash"], x, int(v["aux"], 16), msg) and st == 0
            assert S.sign(curve, S.BIP0340, v["hash"], x, k, msg) == (0, bytes.fromhex(v["sig"]))


def items_file(fx, path):
    lines = []
    hx = lambda b: b.hex() if b else "-"
    for curve, items in fx["dbign"].items():
        q = O.CURVES[curve]["q"]
        for i in items:
            dg = D.H(i["hash"], bytes.fromhex(i["msg"]))
            lines.append("D %d %s %s %s %s %s 0 %s %d" % (q.bit_length(), q.to_bytes(O.qlen(curve), "big").hex(), i["x"], dg.hex(), i["oid"] or "-",
                                                          i["t"] or "-", i["k"], i["rejects"]))
    for curve, items in fx["bip0340"].items():
        q = O.CURVES[curve]["q"]
        for i in items:
            lines.append("B %d %d %s %d %s %s %s %s %d %s" % (D.HT[i["hash"]], q.bit_length(), q.to_bytes(O.qlen(curve), "big").hex(), O.clen(curve), i["x"],
                                                             hx(bip_key(curve, i)), i["aux"], i["msg"] or "-", 0 if i["ret"] == 0 else 1, i["k"]))
    path.write_text("\n".join(lines) + "\n")
    return len(lines)


def test_shim_as_a_sanitized_program_over_the_fixture(fx, tmp_path):
    """the word buffers, the odd-qlen indexing and the message stream under AddressSanitizer and UBSan: a stand-alone program with
    exact-length heap inputs, run as a child process"""
    exe = os.path.join(BUILD, "det_nonce_host_asan")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DDET_NONCE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SHIM])
    n = items_file(fx, tmp_path / "items.txt")
    p = subprocess.run([exe, str(tmp_path / "items.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "%d items, 0 bad" % n


@pytest.mark.parametrize("curve", D.DBIGN_CURVES)
def test_dbign_kernel_lane_by_lane_on_the_host(kernlib, fx, curve):
    """more than one block and a partial last one, both Tab instantiations"""
    qw, qbits = qwords(curve)
    ql = O.qlen(curve)
    for h in D.DBIGN_HASHES:
        for t in (b"", D.T_SAMPLE):
            items = [i for i in fx["dbign"][curve] if i["hash"] == h and bytes.fromhex(i["t"]) == t]
            items = (items * 66)[:70] if t == b"" else items
            n = len(items)
            privs = b"".join(bytes.fromhex(i["x"]) for i in items)
            dgs = b"".join(D.H(h, bytes.fromhex(i["msg"])) for i in items)
            want = b"".join(bytes.fromhex(i["k"]) for i in items)
            for scan in (0, 1):
                k, st = C.create_string_buffer(n * ql), C.create_string_buffer(b"\x07" * n, n)
                assert kernlib.dk_dbign_batch(scan, n, privs, dgs, D.HSIZE[h], B.OID_BELT, len(B.OID_BELT), t, len(t), qw, qbits, k, st) == 0
                assert (k.raw, st.raw) == (want, bytes(n)), (curve, h, scan)
    assert kernlib.dk_dbign_batch(0, 1, privs, dgs, 129, b"", 0, b"", 0, qw, qbits, k, st) != 0
    assert kernlib.dk_dbign_batch(0, 1, privs, dgs, 32, b"", 0, b"", 0, qw, 8 * 67, k, st) != 0
    assert kernlib.dk_dbign_batch(0, 0, None, None, 32, b"", 0, b"", 0, qw, qbits, None, None) == 0


@pytest.mark.parametrize("curve", D.BIP_CURVES)
def test_bip0340_kernel_lane_by_lane_on_the_host(kernlib, fx, curve):
    """more than one block and a partial last one, the slot check, a key that did not import"""
    qw, qbits = qwords(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    for h in D.BIP_HASHES:
        items = [i for i in fx["bip0340"][curve] if i["hash"] == h]
        items = (items * 14)[:70]
        n = len(items)
        msgs = [bytes.fromhex(i["msg"]) for i in items]
        stride = D.bip_stride(curve, h, max(len(m) for m in msgs))
        sl = [D.bip_slot(curve, h, m, stride) for m in msgs]
        privs = b"".join(bytes.fromhex(i["x"]) for i in items)
        keys = b"".join(bip_key(curve, i) for i in items)
        aux = b"".join(bytes.fromhex(i["aux"]) for i in items)
        want = [bytes.fromhex(i["k"]) for i in items]
        wst = [0 if i["ret"] == 0 else 1 for i in items]
        k, st = C.create_string_buffer(n * ql), C.create_string_buffer(b"\x07" * n, n)
        assert kernlib.dk_bip_batch(D.HT[h], n, privs, keys, bytes(n), aux, b"".join(sl), stride, cl, qw, qbits, k, st) == 0
        assert (k.raw, st.raw) == (b"".join(want), bytes(wst)), (curve, h)
        # a length that does not fit the stride or does not hold the fixed fields, a flagged key: a zero nonce and status 1, to that item alone
        fixed = 2 * D.HSIZE[h] + 2 * cl
        sl[0] = D.bip_slot(curve, h, msgs[0], stride, length=stride - 3)
        sl[63] = D.bip_slot(curve, h, msgs[63], stride, length=fixed - 1)
        kst = bytearray(n)
        kst[64] = kst[n - 1] = 1
        bad = (0, 63, 64, n - 1)
        assert kernlib.dk_bip_batch(D.HT[h], n, privs, keys, bytes(kst), aux, b"".join(sl), stride, cl, qw, qbits, k, st) == 0
        assert k.raw == b"".join(bytes(ql) if j in bad else w for j, w in enumerate(want))
        assert st.raw == bytes(1 if j in bad else s for j, s in enumerate(wst))
    assert kernlib.dk_bip_batch(5, 1, privs, keys, bytes(n), aux, b"".join(sl), stride, cl, qw, qbits, k, st) != 0
    assert kernlib.dk_bip_batch(2, 1, privs, keys, bytes(n), aux, b"".join(sl), stride + 2, cl, qw, qbits, k, st) != 0
    assert kernlib.dk_bip_batch(2, 0, None, None, None, None, None, stride, cl, qw, qbits, None, None) == 0


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in libecc_amd.api.EXPORTED_SYMBOLS, sym
    for m in ("dbign_nonce", "dbign_nonce_dev", "dbign_sign", "dbign_sign_dev", "bip0340_nonce", "bip0340_nonce_dev", "bip0340_sign",
              "bip0340_sign_dev"):
        assert hasattr(libecc_amd.api.Curve, m), m
    assert "sig/bign_common.c:200-342" in header and "sig/bip0340.c:213-294" in header
    assert "WITH THE CALLER" not in header
    lib = libecc_amd.api.lib_path()
    if os.path.exists(lib):
        L = C.CDLL(lib)
        for sym in SYMBOLS:
            assert hasattr(L, sym), sym
