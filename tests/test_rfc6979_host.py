"""CPU tests of deterministic ECDSA's nonce derivation (libecc_amd/csrc/ecamd_rfc6979.h) through tests/rfc6979_host_shim.cpp (g++, no
HIP): (a) the header's HMAC against Python's hmac; (b) the generator against oracles.rfc6979_nonce and the restatement with a retry
counter (tests/decdsa_ref.py) on the 32 RFC 6979 vectors and on the recorded reference answers (tests/golden/decdsa.json); (c) the
signature assembled from that k in Python integers against the vectors and the recording; (d) the fixture's conditions and, where
oracle/_ref is built, the fixture regenerated from the reference; (e) the shim as a stand-alone program under
-fsanitize=address,undefined over the fixture; (f) the kernel k_rfc6979_nonce itself (libecc_amd/csrc/ecamd_rfc6979.hip) lane by lane
over tests/hipstub; (g) the new symbols in header, binding and library."""
import ctypes as C
import hmac
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import decdsa_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "decdsa.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "rfc6979_host_shim.cpp")
SYMBOLS = ["ec_rfc6979_nonce_batch", "ec_rfc6979_nonce_batch_dev", "ec_decdsa_sign_batch", "ec_decdsa_sign_batch_dev"]


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture(FIXTURE)


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(O.GOLDEN, "ecdsa_kats.json")) as f:
        return [v for v in json.load(f) if v["sig_type"] == "DECDSA"]


@pytest.fixture(scope="module")
def shimlib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "rfc6979_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM])
    lib = C.CDLL(so)
    u32, u32p = C.c_uint32, C.POINTER(C.c_uint32)
    lib.r_hmac.argtypes = [C.c_int, C.c_char_p, C.c_char_p, u32, C.c_char_p]
    lib.r_nonce.argtypes = [C.c_int, C.c_char_p, C.c_char_p, u32p, u32, C.c_char_p, u32p]
    lib.r_slot_ok.argtypes = [u32, u32]
    return lib


def shim_nonce(lib, curve, hash_name, priv, dg):
    """(status, k, rejected candidates) of the header's generator"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    qw = (C.c_uint32 * 17)(*[(q >> (32 * w)) & 0xFFFFFFFF for w in range(17)])
    k, r = C.create_string_buffer(ql), C.c_uint32(0)
    st = lib.r_nonce(D.HT[hash_name], priv, dg, qw, q.bit_length(), k, C.byref(r))
    return st, int.from_bytes(k.raw, "big"), r.value


def test_fixture_covers_what_it_must(fx):
    assert list(fx) == D.CURVES and os.path.getsize(FIXTURE) < 1 << 18
    for curve, items in fx.items():
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        for h in D.HASHES:
            mine = [i for i in items if i["hash"] == h]
            assert sorted(len(i["msg"]) // 2 for i in mine if i["family"] == "msg_len") == D.MSG_LENS, (curve, h)
            edge = {int(i["x"], 16): i["ret"] for i in mine if i["family"] == "x_edge"}
            # what the reference does with the edge keys, as recorded: x = 0 imports and signs, x >= q does not import
            assert edge == {0: 0, 1: 0, q - 1: 0, q: -2, (1 << (8 * ql)) - 1: -2}, (curve, h)
        assert all(i["ret"] == 0 for i in items if i["family"] != "x_edge")
        assert all((i["sig"] is not None) == (i["ret"] == 0) and len(i["x"]) == 2 * ql for i in items)
        retries = [i["retries"] for i in items]
        if curve in D.RETRY_CURVES:
            # the retry path is covered by these three curves or not at all
            assert 0 in retries and 1 in retries and max(retries) >= 2, curve
            for h in D.HASHES:
                assert {min(i["retries"], 2) for i in items if i["hash"] == h} == {0, 1, 2}, (curve, h)
    assert D.nonce("SECP521R1", "SHA224", bytes(66), b"")[1] == 0       # three rounds of V fill T there; one on secp192r1 / SHA-512
    assert O.qlen("SECP224K1") == 29 and O.qlen("SECP521R1") == 66


def test_restatement_gives_the_reference_answers(fx, kats):
    for curve, items in fx.items():
        q = O.CURVES[curve]["q"]
        for i in items:
            priv, msg = bytes.fromhex(i["x"]), bytes.fromhex(i["msg"])
            k, r = D.nonce(curve, i["hash"], priv, msg)
            assert (k, r) == (int(i["k"], 16), i["retries"])
            assert k == O.rfc6979_nonce(curve, i["hash"], priv, msg)
            st, sig = D.sign_with(curve, int(i["x"], 16), k, D.H(i["hash"], msg))
            assert (st, sig.hex()) == ((0, i["sig"]) if i["ret"] == 0 else (1, bytes(2 * O.qlen(curve)).hex())), (curve, i["family"])
    assert len(kats) == 32


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_decdsa_fixture as M
    with open(FIXTURE) as f:
        assert M.dumps(M.build()) == f.read()


@pytest.mark.parametrize("hash_name", D.HASHES)
def test_header_hmac_on_every_length(shimlib, hash_name):
    rng = np.random.default_rng(D.HT[hash_name])
    hs = D.HSIZE[hash_name]
    out = C.create_string_buffer(hs)
    for n in range(301):
        key, msg = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert shimlib.r_hmac(D.HT[hash_name], key, msg, n, out) == 0
        assert out.raw == hmac.new(key, msg, O.HASHLIB[hash_name]).digest(), (hash_name, n)
    for key in (bytes(hs), b"\xff" * hs):
        shimlib.r_hmac(D.HT[hash_name], key, b"", 0, out)
        assert out.raw == hmac.new(key, b"", O.HASHLIB[hash_name]).digest()
    assert shimlib.r_hmac(0, bytes(64), b"", 0, out) == -1 and shimlib.r_hmac(5, bytes(64), b"", 0, out) == -1


def test_generator_and_signature_on_the_rfc6979_vectors(shimlib, kats):
    for v in kats:
        curve, h = v["curve"], v["hash"]
        priv, msg = bytes.fromhex(v["priv_key"]), bytes.fromhex(v["msg"])
        priv = priv[-O.qlen(curve):].rjust(O.qlen(curve), b"\0")
        dg = D.H(h, msg)
        st, k, r = shim_nonce(shimlib, curve, h, priv, dg)
        assert (st, k) == (0, O.rfc6979_nonce(curve, h, priv, msg)) and (k, r) == D.nonce(curve, h, priv, msg), v["name"]
        assert D.sign_with(curve, int.from_bytes(priv, "big"), k, dg) == (0, bytes.fromhex(v["exp_sig"])), v["name"]


@pytest.mark.parametrize("curve", D.CURVES)
def test_generator_and_signature_on_the_fixture(shimlib, fx, curve):
    ql = O.qlen(curve)
    for i in fx[curve]:
        priv, msg = bytes.fromhex(i["x"]), bytes.fromhex(i["msg"])
        dg = D.H(i["hash"], msg)
        st, k, r = shim_nonce(shimlib, curve, i["hash"], priv, dg)
        assert (st, k, r) == (0, int(i["k"], 16), i["retries"]), (curve, i["hash"], i["family"])
        assert k == O.rfc6979_nonce(curve, i["hash"], priv, msg)
        st, sig = D.sign_with(curve, int(i["x"], 16), k, dg)
        assert (st, sig) == ((0, bytes.fromhex(i["sig"])) if i["ret"] == 0 else (1, bytes(2 * ql))), (curve, i["hash"], i["family"])


def test_generator_on_edge_digests_and_slot_rule(shimlib):
    rng = np.random.default_rng(79)
    for curve in D.CURVES:
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        for h in D.HASHES:
            hs = D.HSIZE[h]
            # digests whose bits2octets value sits at 0, q - 1, q and the top
            sh = max(0, 8 * hs - q.bit_length())
            dgs = [bytes(hs), b"\xff" * hs] + [(v << sh).to_bytes(hs, "big") for v in (q - 1, q, q + 1) if (v << sh) < 1 << (8 * hs)]
            for dg in dgs:
                priv = rng.integers(0, 256, size=ql, dtype=np.uint8).tobytes()
                st, k, r = shim_nonce(shimlib, curve, h, priv, dg)
                assert (st, (k, r)) == (0, D.nonce_from_digest(curve, h, priv, dg)), (curve, h)
    for ln, stride, want in ((0, 4, 1), (1, 4, 0), (252, 256, 1), (253, 256, 0), (0xFFFFFFFF, 256, 0), (4092, 4096, 1), (4093, 4096, 0)):
        assert shimlib.r_slot_ok(ln, stride) == want
    assert [shimlib.r_hash_size(t) for t in (0, 1, 2, 3, 4, 5, 16)] == [0, 28, 32, 48, 64, 0, 0]


def test_shim_as_a_sanitized_program_over_the_fixture(fx, tmp_path):
    """the T buffer and the odd-qlen indexing under AddressSanitizer and UBSan: a stand-alone program, run as a child process"""
    exe = os.path.join(BUILD, "rfc6979_host_asan")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DRFC6979_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SHIM])
    lines = []
    for curve, items in fx.items():
        q = O.CURVES[curve]["q"]
        for i in items:
            dg = D.H(i["hash"], bytes.fromhex(i["msg"]))
            lines.append("%d %d %s %s %s %s %d" % (D.HT[i["hash"]], q.bit_length(), q.to_bytes(O.qlen(curve), "big").hex(), i["x"], dg.hex(), i["k"], i["retries"]))
    path = tmp_path / "items.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "%d items, 0 bad" % len(lines)


@pytest.mark.parametrize("curve", D.CURVES)
def test_kernel_lane_by_lane_on_the_host(fx, curve):
    """tests/rfc6979_kernel_host_shim.cpp: more than one block, a partial last one, the slot check"""
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "rfc6979_kernel_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__shared__=static", "-I" + os.path.join(ROOT, "tests", "hipstub"),
                           "-o", so, os.path.join(ROOT, "tests", "rfc6979_kernel_host_shim.cpp")])
    lib = C.CDLL(so)
    u32 = C.c_uint32
    lib.rk_nonce_batch.argtypes = [C.c_int, u32, C.c_char_p, C.c_char_p, C.c_char_p, u32, C.POINTER(u32), u32, C.c_char_p, C.c_char_p]
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    qw = (u32 * 17)(*[(q >> (32 * w)) & 0xFFFFFFFF for w in range(17)])
    for h in D.HASHES:
        items = [i for i in fx[curve] if i["hash"] == h] * 6
        n = len(items)
        assert n > 64 and n % 64
        privs = b"".join(bytes.fromhex(i["x"]) for i in items)
        msgs = [bytes.fromhex(i["msg"]) for i in items]
        dgs = b"".join(D.H(h, m) for m in msgs)
        want = [bytes.fromhex(i["k"]) for i in items]
        k, st = C.create_string_buffer(n * ql), C.create_string_buffer(b"\x07" * n, n)
        assert lib.rk_nonce_batch(D.HT[h], n, privs, dgs, None, 0, qw, q.bit_length(), k, st) == 0
        assert (k.raw, st.raw) == (b"".join(want), bytes(n)), (curve, h)
        # with the slots the digests came from: a length that does not fit gives a zero nonce and status 1, to that item alone
        stride = D.stride_for(max(len(m) for m in msgs))
        sl = [D.slot(m, stride) for m in msgs]
        bad = (0, 63, 64, n - 1)
        for j in bad:
            sl[j] = D.slot(msgs[j], stride, length=stride - 3)
        assert lib.rk_nonce_batch(D.HT[h], n, privs, dgs, b"".join(sl), stride, qw, q.bit_length(), k, st) == 0
        assert k.raw == b"".join(bytes(ql) if j in bad else w for j, w in enumerate(want))
        assert st.raw == bytes(1 if j in bad else 0 for j in range(n))
    assert lib.rk_nonce_batch(5, 1, privs, dgs, None, 0, qw, q.bit_length(), k, st) != 0
    assert lib.rk_nonce_batch(2, 1, privs, dgs, None, 0, qw, 8 * 67, k, st) != 0          # qlen beyond the word buffer
    assert lib.rk_nonce_batch(2, 0, None, None, None, 0, qw, q.bit_length(), None, None) == 0


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in libecc_amd.api.EXPORTED_SYMBOLS, sym
    for m in ("rfc6979_nonce", "rfc6979_nonce_dev", "decdsa_sign", "decdsa_sign_dev"):
        assert hasattr(libecc_amd.api.Curve, m), m
    assert "sig/ecdsa_common.c:48-169" in header
    lib = libecc_amd.api.lib_path()
    if os.path.exists(lib):
        L = C.CDLL(lib)
        for sym in SYMBOLS:
            assert hasattr(L, sym), sym
