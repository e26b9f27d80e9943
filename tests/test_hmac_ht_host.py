"""CPU tests of libecc_amd/csrc/ecamd_hmac.h compiled for the host (tests/hmac_ht_host_shim.cpp): the hash traits, HMAC and the RFC 6979
generator that k_hmac_slots and k_rfc6979_nonce_ht run per lane, byte for byte against Python (hmac.new over hashlib, where hashlib
has the hash) and against the unmodified reference's recorded answers (tests/golden/hmac_ht.json) for every served hash."""
import subprocess

import pytest

import hmac_ht_ref as M
from decdsa_ref import sign_with


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture()


def test_sizes_are_libeccs_table():
    import ctypes as C
    for name in M.NAMES:
        out = (C.c_int * 2)()
        assert M.shim().hh_sizes(M.HASH_IDS[name], out) == 0
        assert (out[0], out[1]) == (M.HASH_SIZES[name], M.BLOCKS[name]), name
    for ht in M.NOT_SERVED:
        out = (C.c_int * 2)()
        assert M.shim().hh_sizes(ht, out) == -1 and out[0] == 0


@pytest.mark.parametrize("name", M.NAMES)
def test_hmac_equals_fixture_and_python(fx, name):
    """every key length (0, 1, B - 1, B, B + 1, 2 B + 3) with every message length: Python's bytes where hashlib has the hash, and the
    reference's recorded answers for the pairs the fixture covers"""
    mac_of = {}
    for kl in M.key_lengths(name):
        for ml in M.msg_lengths(name):
            key, msg = M.key_bytes(kl), M.msg_bytes(ml)
            mac_of[(kl, ml)] = M.shim_hmac(name, key, msg)[0]
            if M.have_hashlib(name):
                assert mac_of[(kl, ml)] == M.py_hmac(name, key, msg), (name, kl, ml)
    pairs = M.hmac_pairs(name)
    assert {kl for kl, _ in pairs} == set(M.key_lengths(name)) and {ml for _, ml in pairs} == set(M.msg_lengths(name))
    M.assert_macs(fx, name, mac_of)


@pytest.mark.parametrize("name", M.NAMES)
def test_plain_hash_through_the_trait(name):
    """the trait alone: hashlib's digests, and for the hashes of tests/golden/hash_table.json the reference's known answers (SM3 and
    Streebog are pinned through their MACs and signatures)"""
    import hashtable_ref as T
    if M.have_hashlib(name):
        for n in M.msg_lengths(name):
            assert M.shim_hash(name, M.msg_bytes(n)) == M.py_hash(name, M.msg_bytes(n))
    if name in T.TABLE:
        for n, dg in T.kat_table(T.load_fixture())[name].items():
            assert M.shim_hash(name, T.counting(n)) == dg, (name, n)


@pytest.mark.parametrize("name", M.NAMES)
def test_slot_form_and_unfit_slots(fx, name):
    kl, ml = M.BLOCKS[name] + 1, 5
    key, msg = M.key_bytes(kl), M.msg_bytes(ml)
    ks, ms = M.stride_for(kl), M.stride_for(ml)
    assert M.shim_slot_hmac(name, M.slot(key, ks), M.slot(msg, ms)) == M.shim_hmac(name, key, msg)[0]
    zero = bytes(M.HASH_SIZES[name])
    assert M.shim_slot_hmac(name, M.slot(key, ks, length=ks - 3), M.slot(msg, ms)) == zero
    assert M.shim_slot_hmac(name, M.slot(key, ks), M.slot(msg, ms, length=ms - 3)) == zero
    assert M.shim_slot_hmac(name, M.slot(key, ks), M.slot(msg, ms, length=0xffffffff)) == zero


def shim_sign(curve, name, priv, msg):
    """(status, signature, rejected candidates): the unit's digest and nonce, then ECDSA's equations in Python integers"""
    h1 = M.shim_hash(name, msg)
    st, k, retries, _ = M.shim_nonce(curve, name, priv, h1)
    assert st == 0
    if M.have_hashlib(name):
        assert (int.from_bytes(k, "big"), retries) == M.py_nonce(curve, name, priv, h1)
    return sign_with(curve, int.from_bytes(priv, "big"), int.from_bytes(k, "big"), h1) + (retries,)


@pytest.mark.parametrize("curve", M.CURVES)
def test_signatures_equal_the_reference(fx, curve):
    """the generator on the recorded items of every new hash: ECDSA's equations over its k give the reference's signatures, so k is
    the nonce the reference signed with; x = 0 and q - 1 sign, x = q does not import"""
    for name in M.NEW_NAMES:
        got = [shim_sign(curve, name, *M.derive(curve, name, i)) for i in range(M.n_items(curve))]
        edges = [shim_sign(curve, name, priv, M.EDGE_MSG)[:2] for priv in M.edge_keys(curve)]
        assert fx["decdsa"]["%s/%s" % (curve, name)]["edges"] == [0, 0, -2]
        M.assert_sigs(fx, curve, name, [g[:2] for g in got], edges)
        if curve == M.RETRY_CURVE:
            assert sum(g[2] for g in got) > 0, name


def test_t_takes_four_v_with_ripemd160_on_secp521r1():
    """qlen 66 over hsize 20: four HMAC_K(V) per candidate, counted by the unit in compressions"""
    priv, msg = M.derive("SECP521R1", "RIPEMD160", 1)
    st, _, retries, calls = M.shim_nonce("SECP521R1", "RIPEMD160", priv, M.shim_hash("RIPEMD160", msg))
    assert st == 0 and retries == 0
    # d, f: inner key block + ceil((20 + 1 + 132 + 9) / 64) = 1 + 3, outer 2; e, g and the four of T: 2 + 2 each
    assert calls == 2 * (4 + 2) + 2 * (2 + 2) + 4 * (2 + 2)


def test_stand_alone_sanitizer_walk():
    """the shim with its own main under the address and undefined-behaviour sanitizers: every hash, key and message lengths around the
    block, exact-size buffers, and the generator at qlen 24 and 66"""
    exe = M.build_shim(main=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout + r.stderr)[-2000:]
