"""CPU tests for ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA and BIP0340 over the whole hash table: libecc_amd/csrc/ecamd_bip0340_nonce_ht.h compiled
for the host (tests/bip0340_nonce_ht_host_shim.cpp) against the unmodified reference's recorded answers (tests/golden/sighash_ht.json)
and against a Python restatement over hashlib; the Python restatement of the five schemes against the same fixture, so that two
references are shown to agree; a stand-alone sanitizer walk; the exported symbols."""
import hashlib
import os
import re
import subprocess

import pytest

import oracles as O
import sighash_ht_ref as R
import hmac_ht_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def test_fixture_covers_every_case(fx):
    want = {R.case_key(s, c, n) for s, c in R.cases() for n in R.NEW_NAMES}
    assert set(fx) == want and len(want) == 5 * 4 * 14
    assert os.path.getsize(R.FIXTURE) < 1 << 20
    for scheme in R.SCHEMES:      # every hash is kept in full on exactly one curve of every scheme
        assert sorted(n for c in R.curves_for(scheme) for n in R.NEW_NAMES if R.full_kept(scheme, c, n)) == sorted(R.NEW_NAMES)
    for key, rec in fx.items():
        scheme = key.split("/")[0]
        assert len(rec["ver"]) == R.N and len(rec["rets"]) == len(R.SIGN_EDGES), key
        assert len(rec["first"]) == (R.N_FULL if R.full_kept(*key.split("/")) else 0), key
        # the reference signed every item outside SIGN_EDGES and accepted every signature that was not corrupted
        assert len(rec["tags"]) == R.TAG_W * (R.N - len(R.SIGN_EDGES) + rec["rets"].count(0)), key
        assert all(rec["ver"][i] == "0" for i in range(R.N) if i not in R.VERIFY_EDGES), key
        # k = 0 and k = q never sign; an aux value is any qlen octets
        assert rec["rets"][:2] == ([0, 0] if scheme == "BIP0340" else [-1, -1]), key
        # x = 0 and x >= q: ECSDSA / ECOSDSA have no range check, ECFSDSA signs x = 0, ECKCDSA and BIP0340 need 0 < x < q
        assert [r == 0 for r in rec["rets"][2:]] == {"ECSDSA": [True] * 3, "ECOSDSA": [True] * 3, "ECFSDSA": [True, False, False],
                                                    "ECKCDSA": [False] * 3, "BIP0340": [False] * 3}[scheme], key


def test_message_lengths_land_on_the_block_boundaries():
    for scheme, curve in R.cases():
        alg = R.SCHEMES[scheme]
        for name in R.NEW_NAMES + [R.TWIN]:
            b, fl = R.BLOCK[name], R.fixed_len(alg, name, curve)
            ends = {(fl + ml) % b for ml in R.msg_lengths(alg, name, curve)}
            assert {b - 1, 0, 1} <= ends, (scheme, curve, name)
            tail = R.MD_TAIL.get(R.HASH_IDS[name])
            if tail:
                assert {b - tail, b - tail + 1} <= ends, (scheme, curve, name)
            assert 0 in R.msg_lengths(alg, name, curve) and max(R.msg_lengths(alg, name, curve)) > 3 * b
            assert R.stride_for(alg, name, curve) <= 4096


@pytest.mark.parametrize("scheme,curve", R.cases())
def test_python_restatement_agrees_with_the_reference(fx, scheme, curve):
    """per hash: the first signatures (their tags; their bytes where the fixture keeps them in full) and the signing edges; for the
    hashes of full_kept() also the verdicts on the corrupted items and on two honest ones (the other honest items are pinned through
    the SHA-256 over all signatures by the GPU tests; Python's point multiplication is slow)"""
    q = O.CURVES[curve]["q"]
    for name in R.NEW_NAMES:
        rec = fx[R.case_key(scheme, curve, name)]
        sigs = {}
        for i in list(range(R.N_FULL)) + sorted(R.SIGN_EDGES):
            st, sig = R.py_sign(scheme, curve, name, *R.sign_item(scheme, curve, name, i))
            if i < R.N_FULL:
                assert st == 0 and R.tag(sig) == rec["tags"][R.TAG_W * i:R.TAG_W * (i + 1)], (scheme, curve, name, i)
                assert not rec["first"] or sig.hex() == rec["first"][i], (scheme, curve, name, i)
                sigs[i] = sig
            else:
                assert (st == 0) == (rec["rets"][sorted(R.SIGN_EDGES).index(i)] == 0), (scheme, curve, name, i)
        if not R.full_kept(scheme, curve, name):
            continue       # the verdicts: the hashes of full_kept(), every hash on one curve of every scheme
        for i in sorted(R.VERIFY_EDGES) + [0, 121]:
            j = i - 120 if i >= 120 else i
            if j not in sigs:
                st, sigs[j] = R.py_sign(scheme, curve, name, *R.sign_item(scheme, curve, name, j))
                assert st == 0 and R.tag(sigs[j]) == rec["tags"][R.TAG_W * j:R.TAG_W * (j + 1)]
            pk, sig, msg, fault = R.verify_item(scheme, curve, name, i, sigs)
            want = 1 if fault else R.py_verify(scheme, curve, name, pk, sig, msg)
            assert str(want) == rec["ver"][i], (scheme, curve, name, i)


def k_py(name, curve, x, pk, aux, msg):
    """the generator over hashlib, with the key's octets as given"""
    q, ql, cl, hs = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve), R.HSIZE[name]
    d = q - x if pk[-1] & 1 else x
    ta, tn = M.py_hash(name, R.TAG_AUX), M.py_hash(name, R.TAG_NONCE)
    mask = M.py_hash(name, ta + ta + aux.to_bytes(ql, "big"))
    tl = max(ql, hs)
    t = bytes(u ^ v for u, v in zip(d.to_bytes(ql, "big").ljust(tl, b"\0"), mask.ljust(tl, b"\0")))
    return int.from_bytes(M.py_hash(name, tn + tn + t + pk[:cl] + msg), "big") % q


@pytest.mark.parametrize("curve", R.curves_for("BIP0340"))
def test_nonce_unit_equals_the_fixture_and_hashlib(fx, curve):
    """every signing item of every hash (the older four included): the unit's k is the restatement's over H (R.nonce_from_pub: hashlib
    where hashlib has the hash, the pinned hash traits otherwise) and over hashlib itself where it has the hash; x = 0 and x >= q fail
    with k = 0.  For every new hash the first N_FULL items are tied to the reference directly: the signature rebuilt from the UNIT's
    k in Python integers has the recorded tag (and the recorded bytes where the fixture keeps them), and k is k' = s - e d' from the
    recorded signature un-flipped by the recorded parity of R.y where the bytes are kept."""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    for name in R.NEW_NAMES + M.OLD_NAMES:
        rec = fx.get(R.case_key("BIP0340", curve, name))
        checked = 0
        for i in range(R.N):
            x, aux, msg = R.sign_item("BIP0340", curve, name, i)
            pk = R.pub("BIP0340", curve, i % R.N_KEYS)
            if x >= 1 << (8 * ql):
                continue
            st, k, calls = R.shim_nonce(name, curve, x, pk, aux, msg)
            if not 0 < x < q:
                assert (st, k) == (1, 0), (curve, name, i)
                continue
            assert st == 0 and k == R.nonce_from_pub(name, curve, x, pk, aux, msg), (curve, name, i)
            if M.have_hashlib(name):
                assert k == k_py(name, curve, x, pk, aux, msg), (curve, name, i)
            checked += 1
            if rec is None or i >= R.N_FULL:
                continue
            st, sig = R.py_sign("BIP0340", curve, name, x, aux, msg, k=k)
            assert st == 0 and R.tag(sig) == rec["tags"][R.TAG_W * i:R.TAG_W * (i + 1)], (curve, name, i)
            if rec["first"]:
                assert sig.hex() == rec["first"][i], (curve, name, i)
                ke = R.bip_k_even(name, curve, i % R.N_KEYS, sig, msg)
                assert k == (q - ke if rec["rodd"][i] == "1" else ke), (curve, name, i)
        assert checked == R.N - 3


def test_tag_hashes_and_one_block_count():
    for name in M.NAMES:
        for t in (R.TAG_AUX, R.TAG_NONCE, R.TAG_CHALLENGE):
            assert R.shim_tag(name, t) == R.H(name, t), (name, t)
    # SHA3-512 (BLOCK 72) on SECP521R1: mask 128 + 66 = 194 octets -> 3 permutations; nonce 128 + 66 + 66 + 10 = 270 -> 4
    x, aux, msg = R.sign_item("BIP0340", "SECP521R1", "SHA3_512", 1)
    st, k, calls = R.shim_nonce("SHA3_512", "SECP521R1", x, R.pub("BIP0340", "SECP521R1", 1), aux, msg[:10])
    assert st == 0 and calls == 3 + 4


def test_stand_alone_sanitizer_walk():
    """the shim with its own main under the address and undefined-behaviour sanitizers: every hash once per order size, message
    lengths around the block in exact-size buffers"""
    exe = R.build_shim(main=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout + r.stderr)[-2000:]


NEW_SYMBOLS = [b + "_ht_batch" + t for b in ("ec_sig_hashed_verify", "ec_sig_hashed_sign", "ec_schnorr_verify", "ec_schnorr_sign", "ec_bip0340_nonce",
                                             "ec_bip0340_sign") for t in ("", "_dev")]


def test_new_symbols_are_declared_listed_and_exported():
    from libecc_amd import api
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in api.EXPORTED_SYMBOLS, sym
    lib = os.path.join(ROOT, "libecc_amd", "lib", "libecc_amd.so")
    assert os.path.exists(lib), "build the library first (python -m libecc_amd.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW_SYMBOLS) <= exported
