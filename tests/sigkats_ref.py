"""Shared by tests/golden/make_sig_kats_fixture.py, tests/test_sig_kats_host.py and tests/test_gpu_sig_kats.py: the reference's own
known answers of ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA, ECGDSA, BIGN and DBIGN (the published ISO/IEC 14888-3, TTA and STB 34.101.45
examples of its self tests) as tests/golden/sig_kats.json holds them, and one sign / verify pair per case that goes to the family's
Python restatement (sighash_ref, schnorr_ref, sigfam_ref, bign_ref) or to the unmodified reference through the same modules.

A case is {id, name, curve, alg, hash, msg, adata, x, k, pub, sig, digest, variants}; everything but the names is hexadecimal:
  id, name  the C identifier of the reference's ec_test_case and its .name string
  adata     the reference's framing for BIGN / DBIGN (u16 OID length, u16 t length, OID, t -- t is empty in every case here), else ""
  x, k      qlen octets, big-endian; DBIGN has no nonce of its own: k is solved from the published signature (k_from_sig)
  pub       the affine key of the scheme: [1/x]G for ECKCDSA and ECGDSA, [x]G for the others
  sig       the published signature
  digest    the reference's H(msg): what the digest-level entry points (ECGDSA, BIGN, DBIGN) are fed with
  variants  [{pub, sig, msg, ret}]: ec_verify's 0 / -1 for the honest triple, sig with one bit flipped in its first and in its second
            component, the message with its first bit flipped, and the honest signature under another case's key on the same curve
            (where there is one).  The file leaves out a variant's field where it equals the case's; load_fixture puts it back."""
import contextlib
import json
import os

import oracles as O
import sigfam_ref as SF
import sighash_ref as SH
import schnorr_ref as S
import bign_ref as B
import hashtable_ref as T
import hmac_ht_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sig_kats.json")

# libecc's ec_alg_type numbers, in the order the fixture is written in
ALGS = {"ECKCDSA": 2, "ECSDSA": 3, "ECOSDSA": 4, "ECFSDSA": 5, "ECGDSA": 6, "BIGN": 18, "DBIGN": 19}
HSIG = ("ECKCDSA", "ECSDSA", "ECOSDSA")
BIGNS = ("BIGN", "DBIGN")
# the reference's name of belt-hash, which tests/bign_ref.py calls BELT
HASH_NAMES = {"BELT_HASH": "BELT"}
HASH_IDS = dict(M.HASH_IDS, BELT=B.HASH_BELT)
HSIZE = dict(M.HASH_SIZES, BELT=32)
B.HASH_IDS.update(T.HASH_IDS)                        # bign_ref's reference calls look the BASH numbers up there

hx = bytes.fromhex


def load_fixture():
    with open(FIXTURE) as f:
        cases = json.load(f)
    for c in cases:
        for v in c["variants"]:
            for k in ("pub", "sig", "msg"):
                v.setdefault(k, c[k])
    return cases


def oid_of(case):
    """the OID octets inside a BIGN / DBIGN case's adata (its t must be empty: no case here carries one)"""
    ad = hx(case["adata"])
    ol, tl = int.from_bytes(ad[:2], "big"), int.from_bytes(ad[2:4], "big")
    assert tl == 0 and len(ad) == 4 + ol
    return ad[4:]


def pub_of(curve, alg, x):
    """the affine key octets of private key x under the scheme"""
    p, a, b, q, G = SF._curve(curve)
    return SF.pt_bytes(curve, S.py_mul(pow(x, -1, q) if alg in ("ECKCDSA", "ECGDSA") else x, G, a, p))


def k_from_sig(curve, x, dg, sig):
    """the nonce a BIGN / DBIGN signature was made with: k = s1 + hbar + (s0 + 2^(8l)) x mod q"""
    q, l = O.CURVES[curve]["q"], B.s0_len(curve)
    return (int.from_bytes(sig[l:], "little") + int.from_bytes(dg, "little") + (int.from_bytes(sig[:l], "little") + (1 << (8 * l))) * x) % q


def components(curve, alg, hname):
    """(octets of the signature's first component, octets of its second)"""
    ql, cl = O.qlen(curve), O.clen(curve)
    if alg in HSIG:
        return SH.r_len(ALGS[alg], hname, ql), ql
    if alg == "ECFSDSA":
        return 2 * cl, ql
    if alg == "ECGDSA":
        return ql, ql
    return B.s0_len(curve), ql


# ---- the Python restatement of each family ----
@contextlib.contextmanager
def jacobian_points():
    """sighash_ref and sigfam_ref multiply with oracles.py_mul, an affine ladder with a Fermat inversion per step: 0.2 s per
    multiplication on the 512- and 521-bit curves, a minute over this fixture.  While their rules run here, the point arithmetic is
    schnorr_ref's Jacobian one (the same affine-or-None results, one inversion per multiplication)."""
    keep = O.py_mul, O.py_add
    O.py_mul, O.py_add = S.py_mul, S.py_add
    try:
        yield
    finally:
        O.py_mul, O.py_add = keep


def py_sign(curve, alg, hname, x, k, msg, dg, oid=b""):
    """(status, signature); dg: H(msg), which ECGDSA, BIGN and DBIGN start from"""
    if alg == "ECFSDSA":
        return S.sign(curve, S.ECFSDSA, hname, x, k, msg)
    if alg in BIGNS:
        return B.sign_digest(curve, oid, x, k, dg)
    with jacobian_points():
        if alg in HSIG:
            return SH.sign(curve, ALGS[alg], hname, x, k, msg)
        return SF.sign(curve, SF.ECGDSA, x, k, dg)


def py_verify(curve, alg, hname, pub, sig, msg, dg, oid=b""):
    """0 accept / 1 reject"""
    if alg == "ECFSDSA":
        return S.verify(curve, S.ECFSDSA, hname, pub, S.AFF, sig, msg)
    if alg in BIGNS:
        return B.verify_digest(curve, oid, pub, sig, dg)
    with jacobian_points():
        if alg in HSIG:
            return SH.verify(curve, ALGS[alg], hname, pub, sig, msg)
        return SF.verify(curve, SF.ECGDSA, pub, sig, dg)


def py_digest(hname, msg):
    """H(msg) without the reference: hashlib, the pure-Python belt-hash of tests/bign_ref.py, and for BASH the host build of the
    library's own hash code (hashtable_ref.shim_hash, which tests/test_hash_table_host.py pins to the reference's known answers)"""
    if hname == "BELT":
        return B.belt_hash(msg)
    if hname in T.TABLE and not T.have_hashlib(hname):
        return T.shim_hash(hname, msg)
    return M.py_hash(hname, msg)


# ---- the unmodified reference -- needs oracle/_ref ----
def ref_digest(hname, msg):
    return B.ref_belt_hash(msg) if hname == "BELT" else M.ref_hash(hname, msg)


def ref_sign(curve, alg, hname, x, k, msg, oid=b""):
    """(ret, signature or None) of ec_key_pair_import_from_priv_key_buf + _ec_sign with the nonce k; DBIGN is signed as BIGN with the
    solved nonce (ref_dbign_sign is the deterministic call)"""
    if alg in HSIG:
        return SH.ref_sign(curve, ALGS[alg], hname, x, k, msg)
    if alg == "ECFSDSA":
        return S.ref_sign(curve, S.ECFSDSA, hname, x, k, msg)
    if alg == "ECGDSA":
        return SF.ref_sign(curve, SF.ECGDSA, hname, x, k, msg)
    return B.ref_sign(curve, hname, oid, x, k, msg, alg=B.BIGN)


def ref_dbign_sign(curve, hname, x, msg, oid):
    import det_sign_ref as D
    return D.ref_dbign_sign(curve, hname, oid, b"", x, msg)


def ref_verify(curve, alg, hname, pub, sig, msg, oid=b""):
    """ec_pub_key_import_from_aff_buf + ec_verify: 0 / -1"""
    if alg in HSIG:
        return SH.ref_verify(curve, ALGS[alg], hname, pub, sig, msg)
    if alg == "ECFSDSA":
        return S.ref_verify(curve, S.ECFSDSA, hname, pub, S.AFF, sig, msg)
    if alg == "ECGDSA":
        return SF.ref_verify(curve, SF.ECGDSA, hname, pub, sig, msg)
    return B.ref_verify(curve, hname, oid, pub, sig, msg, alg=ALGS[alg])
