"""CPU tests of the hashing front end of one-call EdDSA signing (libecc_amd/csrc/ecamd_eddsa_sign.h and the kernels of
ecamd_eddsa_sign.hip, lane by lane over tests/hipstub through tests/eddsa_sign_host_shim.cpp; g++, no HIP): (a) what the recorded
reference answers (tests/golden/eddsa_sign.json) cover, and that oracles.ed25519_sign / ed448_sign give every one of them; (b) where
oracle/_ref is built, the fixture regenerated from the reference; (c) key expansion and clamp, PH(M), r_hash and hram of all five
variants on every fixture item and on every message length 0 .. 300 under four context lengths, against hashlib; (d) the slot check,
the final kernel and the launchers' argument checks; (e) the shim as a stand-alone program under -fsanitize=address,undefined;
(f) the new symbols in header, binding and library."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import eddsa_sign_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "eddsa_sign.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "eddsa_sign_host_shim.cpp")
SYMBOLS = ["ec_eddsa_sign_msg_batch", "ec_eddsa_sign_msg_batch_dev", "ec_eddsa_pub_key_batch", "ec_eddsa_pub_key_batch_dev"]
ALGS = sorted(E.ALGS.values())
SHA_EDGES = [111, 112, 127, 128, 129, 239, 240]
SHAKE_EDGES = [135, 136, 137, 271, 272, 273]


@pytest.fixture(scope="module")
def fx():
    return E.load_fixture(FIXTURE)


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "eddsa_sign_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tests", "hipstub"), "-o", so, SHIM])
    lib = C.CDLL(so)
    u32, cp = C.c_uint32, C.c_char_p
    lib.eds_dom.argtypes = [C.c_int, cp, u32, cp]
    lib.eds_slot_ok.argtypes = [u32, u32]
    lib.eds_expand.argtypes = [C.c_int, u32, cp, cp, u32, cp, u32, cp, cp, cp, cp, cp]
    lib.eds_hram.argtypes = [C.c_int, u32, cp, cp, cp, u32, cp, cp, u32, cp, cp]
    lib.eds_fin.argtypes = [C.c_int, u32, cp, cp, cp, cp, cp, cp]
    return lib


def run_front_end(lib, alg, sks, adata, msgs, Rs, As, bad_lengths=None):
    """the two hashing kernels over one batch: (a, a_wide, r_hash, ph, bad, hram, sigs) as lists of per-item bytes"""
    n, kl = len(sks), E.klen(alg)
    hl = 2 * kl
    stride = E.stride_for(max(len(m) for m in msgs))
    sl = [E.slot(m, stride) for m in msgs]
    for j, ln in (bad_lengths or {}).items():
        sl[j] = E.slot(msgs[j], stride, length=ln(stride))
    sl = b"".join(sl)
    a, aw, rh, ph = (C.create_string_buffer(b"\xee" * (n * w), n * w) for w in (kl, hl, hl, 64))
    bad = C.create_string_buffer(b"\xee" * n, n)
    alen = len(adata) if adata is not None else 0
    assert lib.eds_expand(alg, n, b"".join(sks), sl, stride, adata, alen, a, aw, rh, ph, bad) == 0
    hr, sg = C.create_string_buffer(b"\xee" * (n * hl), n * hl), C.create_string_buffer(b"\xee" * (2 * n * kl), 2 * n * kl)
    assert lib.eds_hram(alg, n, b"".join(Rs), b"".join(As), sl, stride, ph, adata, alen, hr, sg) == 0

    def cut(buf, w):
        return [buf.raw[w * j:w * (j + 1)] for j in range(n)]
    return cut(a, kl), cut(aw, hl), cut(rh, hl), cut(ph, 64), bad.raw, cut(hr, hl), cut(sg, 2 * kl)


def test_fixture_covers_what_it_must(fx):
    assert 200 <= len(fx) <= 400 and os.path.getsize(FIXTURE) < 1 << 18
    for alg in ALGS:
        mine = [i for i in fx if i["alg"] == alg]
        kl, edges = E.klen(alg), SHAKE_EDGES if E.is448(alg) else SHA_EDGES
        signed = [i for i in mine if i["ret"] == 0]
        assert all(len(i["sk"]) == 2 * kl and len(i["pub"]) == 2 * kl and (i["sig"] is not None) == (i["ret"] == 0) for i in mine)
        if E.is_ph(alg):
            assert {len(i["msg"]) // 2 for i in signed} >= set(edges)
        else:
            dl = [len(E.dom(alg, bytes.fromhex(i["adata"] or ""))) for i in signed]
            assert {d + kl + len(i["msg"]) // 2 for d, i in zip(dl, signed)} >= set(edges), alg
            assert {d + 2 * kl + len(i["msg"]) // 2 for d, i in zip(dl, signed)} >= set(edges), alg
        assert {len(i["msg"]) // 2 for i in mine} >= {0, 1, 1000}
        assert {i["sk"] for i in mine} >= {"00" * kl, "ff" * kl}
        if E.takes_ctx(alg):
            assert {len(i["adata"]) // 2 for i in signed if i["adata"] is not None} >= ({1, 3, 255} | ({0} if alg != E.EDDSA25519CTX else set()))
    # what the reference does without a context, as recorded: EDDSA25519CTX refuses (sig/eddsa.c:1683), the others hash OLEN = 0
    assert {i["alg"]: i["ret"] for i in fx if i["family"] == "null_ctx"} == {10: -1, 11: 0, 12: 0, 13: 0}
    assert all(i["ret"] == 0 for i in fx if i["family"] != "null_ctx")


def test_restatements_give_the_reference_answers(fx):
    for i in fx:
        alg, ad = i["alg"], bytes.fromhex(i["adata"] or "")
        A, sig = E.py_sign(alg, bytes.fromhex(i["sk"]), ad, bytes.fromhex(i["msg"]))
        assert A.hex() == i["pub"], (alg, i["family"])
        if i["ret"] == 0:
            assert sig.hex() == i["sig"], (alg, i["family"])


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_eddsa_sign_fixture as M
    with open(FIXTURE) as f:
        assert M.dumps(M.build()) == f.read()


def test_dom_builder(shim):
    out = C.create_string_buffer(296)
    for alg in ALGS:
        for ad in (None, b"", b"a", b"abc", bytes(range(255))):
            n = shim.eds_dom(alg, ad, len(ad) if ad else 0, out)
            want = E.dom(alg, ad or b"")
            assert out.raw[:n] == want and out.raw[n:] == bytes(296 - n), (alg, ad)
    # a NULL context with a length: OLEN and no octets, as sig/eddsa.c:79
    n = shim.eds_dom(12, None, 5, out)
    assert out.raw[:n] == b"SigEd448\x00\x05"


@pytest.mark.parametrize("alg", ALGS)
def test_kernels_on_the_fixture(shim, fx, alg):
    """every item of the variant in one batch per context (the context is the call's), more than one block where there are enough"""
    kl = E.klen(alg)
    mine = [i for i in fx if i["alg"] == alg and i["ret"] == 0]
    for adata in sorted({i["adata"] for i in mine}, key=lambda x: (x is not None, x)):
        items = [i for i in mine if i["adata"] == adata]
        ad = bytes.fromhex(adata) if adata is not None else None
        sks, msgs = [bytes.fromhex(i["sk"]) for i in items], [bytes.fromhex(i["msg"]) for i in items]
        Rs, As = [bytes.fromhex(i["sig"])[:kl] for i in items], [bytes.fromhex(i["pub"]) for i in items]
        a, aw, rh, ph, bad, hr, sg = run_front_end(shim, alg, sks, ad, msgs, Rs, As)
        assert bad == bytes(len(items))
        for j, i in enumerate(items):
            wa, prefix = E.expand(alg, sks[j])
            assert a[j] == wa and aw[j] == wa + bytes(kl), (alg, i["family"])
            assert rh[j] == E.r_hash(alg, sks[j], ad or b"", msgs[j]), (alg, i["family"], len(msgs[j]))
            assert hr[j] == E.hram(alg, ad or b"", Rs[j], As[j], msgs[j]), (alg, i["family"], len(msgs[j]))
            assert sg[j][:kl] == Rs[j]
            if E.is_ph(alg):
                assert ph[j] == E.PH(alg, msgs[j])
            # the restatement's S from these hashes is the recorded one
            q = O.E4_Q if E.is448(alg) else O.ED_Q
            S = (int.from_bytes(rh[j], "little") + int.from_bytes(hr[j], "little") * int.from_bytes(a[j], "little")) % q
            assert S.to_bytes(kl, "little") == bytes.fromhex(i["sig"])[kl:]


@pytest.mark.parametrize("alg", ALGS)
def test_kernels_on_every_length(shim, alg):
    """|M| = 0 .. 300 in one batch of 301 items (five blocks of lanes, lengths mixed inside each), under contexts of 0, 1, 3 and 255
    octets: every total length of both hashes from |dom| + klen up, across every block boundary"""
    kl = E.klen(alg)
    rng = np.random.default_rng(alg)

    def rnd(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    for alen in (0, 1, 3, 255) if E.takes_ctx(alg) else (0,):
        ad = rnd(alen)
        msgs = [rnd(n) for n in rng.permutation(301)]
        sks, Rs, As = [rnd(kl) for _ in msgs], [rnd(kl) for _ in msgs], [rnd(kl) for _ in msgs]
        a, aw, rh, ph, bad, hr, sg = run_front_end(shim, alg, sks, ad, msgs, Rs, As)
        assert bad == bytes(301)
        for j, m in enumerate(msgs):
            assert a[j] == E.expand(alg, sks[j])[0], (alg, alen, len(m))
            assert rh[j] == E.r_hash(alg, sks[j], ad, m), (alg, alen, len(m))
            assert hr[j] == E.hram(alg, ad, Rs[j], As[j], m), (alg, alen, len(m))


def test_bad_slots_final_kernel_and_launch_checks(shim):
    for alg in ALGS:
        kl = E.klen(alg)
        msgs = [bytes([j]) * (j % 40) for j in range(70)]
        sks, Rs, As = [bytes([j + 1]) * kl for j in range(70)], [bytes([j + 2]) * kl for j in range(70)], [bytes([j + 3]) * kl for j in range(70)]
        badl = {0: lambda s: s - 3, 63: lambda s: 0xFFFFFFFF, 64: lambda s: s, 69: lambda s: s - 3}
        a, aw, rh, ph, bad, hr, sg = run_front_end(shim, alg, sks, b"ctx", msgs, Rs, As, badl)
        assert bad == bytes(1 if j in badl else 0 for j in range(70))
        good = run_front_end(shim, alg, sks, b"ctx", msgs, Rs, As)
        for j in range(70):
            assert a[j] == good[0][j]
            if j not in badl:
                assert (rh[j], hr[j]) == (good[2][j], good[5][j])
        # the final kernel: S behind R; a bad slot or a failed encoding gives status 1 and zero bytes to that item alone
        S = b"".join(bytes([j + 4]) * kl for j in range(70))
        stR = bytes(1 if j == 5 else 0 for j in range(70))
        stA = bytes(1 if j == 7 else 0 for j in range(70))
        for sa in (stA, None):
            sigs = C.create_string_buffer(b"".join(sg), 140 * kl)
            st = C.create_string_buffer(b"\xee" * 70, 70)
            assert shim.eds_fin(alg, 70, bad, stR, sa, S, sigs, st) == 0
            rej = set(badl) | {5} | ({7} if sa else set())
            assert st.raw == bytes(1 if j in rej else 0 for j in range(70))
            for j in range(70):
                assert sigs.raw[2 * kl * j:2 * kl * (j + 1)] == (bytes(2 * kl) if j in rej else Rs[j] + bytes([j + 4]) * kl), (alg, j)
    for ln, stride, want in ((0, 4, 1), (1, 4, 0), (252, 256, 1), (253, 256, 0), (0xFFFFFFFF, 256, 0), (4092, 4096, 1), (4093, 4096, 0)):
        assert shim.eds_slot_ok(ln, stride) == want
    b = C.create_string_buffer(4096)
    for alg in (0, 8, 14, -1):
        assert shim.eds_expand(alg, 1, b, b, 8, None, 0, b, b, b, b, b) != 0
        assert shim.eds_hram(alg, 1, b, b, b, 8, b, None, 0, b, b) != 0
        assert shim.eds_fin(alg, 1, b, b, None, b, b, b) != 0
    for stride in (0, 6, 4100):
        assert shim.eds_expand(9, 1, b, b, stride, None, 0, b, b, b, b, b) != 0
    assert shim.eds_expand(9, 0, None, None, 0, None, 0, None, None, None, None, None) == 0
    assert shim.eds_expand(11, 1, b, b, 8, None, 0, b, b, b, None, b) != 0          # a PH variant without the PH(M) buffer


def test_shim_as_a_sanitized_program_over_the_fixture(fx, tmp_path):
    """exact-size heap buffers under AddressSanitizer and UBSan: a stand-alone program, run as a child process"""
    exe = os.path.join(BUILD, "eddsa_sign_host_asan")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEDDSA_SIGN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "tests", "hipstub"), "-o", exe, SHIM])
    lines = []
    for i in fx:
        if i["ret"] != 0 or i["adata"] is None:
            continue
        alg, kl = i["alg"], E.klen(i["alg"])
        sk, ad, msg, sig, pub = (bytes.fromhex(i[k]) for k in ("sk", "adata", "msg", "sig", "pub"))
        lines.append(" ".join([str(alg), ad.hex() or "-", msg.hex() or "-", sk.hex(), sig[:kl].hex(), pub.hex(), E.expand(alg, sk)[0].hex(),
                               E.r_hash(alg, sk, ad, msg).hex(), E.hram(alg, ad, sig[:kl], pub, msg).hex()]))
    path = tmp_path / "items.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "%d items, 0 bad" % len(lines)


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in libecc_amd.api.EXPORTED_SYMBOLS, sym
    for m in ("eddsa_sign_msgs", "eddsa_sign_msgs_dev", "eddsa_pub_keys", "eddsa_pub_keys_dev"):
        assert hasattr(libecc_amd.api.Curve, m), m
    assert "sig/eddsa.c:1028" in header and "sig/eddsa.c:611-688" in header
    lib = libecc_amd.api.lib_path()
    if os.path.exists(lib):
        L = C.CDLL(lib)
        for sym in SYMBOLS:
            assert hasattr(L, sym), sym
