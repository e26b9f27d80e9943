#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for the message-level ECGDSA / ECRDSA / SM2 entry points and their device hashes, so
that this pin travels without oracle/_ref:
    python tests/golden/make_sig_msg_fixture.py  ->  tests/golden/sig_msg.json
  "hash"    known answers of libecc's sm3, streebog256 and streebog512 one-shots: a counting pattern of every length around the block and
            padding boundaries of a 64-octet block and of the largest slot, and for Streebog all-0xFF messages of 64, 128 and 192
            octets (the carries of Sigma and N through every word)
  "verify"  (curve, scheme, hash, id, message, public key, signature) -> ec_pub_key_import_from_aff_buf + ec_verify's 0 / -1
  "sign"    (curve, scheme, hash, id, message, x, k) -> -2 where ec_key_pair_import_from_priv_key_buf fails, else _ec_sign's return
            value and signature bytes
Each signature item also holds the reference digest the digest-level entry points would be fed (H(m), or H(Z || m) with Z for SM2).
Items: the reference's own vectors (src/tests/ec_self_tests_core.h, parsed as data like tests/golden/extract_kats.py does), the
crafted families of tests/sigfam_ref.py with the hash swapped in (tests/sigmsg_ref.py), and for SM2 honest items with ids of 0, 16, 62
and 63 octets: with 62 the prefix ENTL || ID || a || b || xG || yG of Z ends exactly on a block boundary (2 + 62 + 4 * 32 = 192)."""
import json
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracles as O  # noqa: E402
import sigfam_ref as S  # noqa: E402
import sigmsg_ref as M  # noqa: E402
import extract_kats as E  # noqa: E402

SEED = 17017
KAT_CURVES = {"GOST_256BITS_CURVE": "GOST256", "GOST_512BITS_CURVE": "GOST512"}
ID_LENGTHS = [0, 16, 62, 63]


def hash_kats():
    out = []
    for name in ("SM3", "STREEBOG256", "STREEBOG512"):
        msgs = [M.counting(n) for n in M.KAT_LENGTHS]
        if name != "SM3":
            msgs += [b"\xff" * n for n in (64, 128, 192)]
        for m in msgs:
            out.append({"hash": name, "msg": m.hex(), "digest": M.ref_hash(name, m).hex()})
    return out


def digest_and_z(curve, alg, hname, pub, msg):
    if alg != S.SM2:
        return S.digest_for(curve, alg, hname, pub, msg).hex(), None
    z = S.sm2_z(curve, hname, pub)
    return S.H(hname, z + msg).hex(), z.hex()


def verify_item(curve, name, hname, family, ident, msg, pub, sig):
    alg = S.SCHEMES[name]
    dg, z = digest_and_z(curve, alg, hname, pub, msg)
    return {"curve": curve, "alg": name, "hash": hname, "family": family, "id": ident.hex(), "msg": msg.hex(), "pub": pub.hex(),
            "sig": sig.hex(), "ret": S.ref_verify(curve, alg, hname, pub, sig, msg), "digest": dg, "z": z}


def sign_item(curve, name, hname, family, ident, msg, x, k):
    alg, ql = S.SCHEMES[name], O.qlen(curve)
    ret, sig = S.ref_sign(curve, alg, hname, x, k, msg)
    P = S.pub_point(curve, alg, x) if S.key_ok(alg, O.CURVES[curve]["q"], x) else None
    pub = S.pt_bytes(curve, P) if P else bytes(2 * O.clen(curve))
    dg, z = digest_and_z(curve, alg, hname, pub, msg)
    return {"curve": curve, "alg": name, "hash": hname, "family": family, "id": ident.hex(), "msg": msg.hex(),
            "x": x.to_bytes(ql + 1, "big").hex(), "k": k.to_bytes(ql + 1, "big").hex(), "pub": pub.hex(), "ret": ret,
            "sig": sig.hex() if sig else None, "digest": dg, "z": z}


ARR2 = re.compile(r"(?:static\s+)?const\s+(?:unsigned\s+char|char)\s+(\w+)\[\]\s*=\s*(\{[^}]*\}|\"[^\"]*\")\s*;", re.S)


def reference_vectors(ver, sgn):
    # the default build's vectors: the branches of `#ifndef USE_ISO14888_3_ECRDSA ... #else ... #endif` that the reference compiles
    # without that toggle (oracle/_ref is built without it: ECRDSA reads its digest byte-reversed)
    src = open(os.path.join(E.REF, "ec_self_tests_core.h"), encoding="latin-1").read()
    src = re.sub(r"#else /\* !?defined\(USE_ISO14888_3_ECRDSA\) \*/.*?#endif /\* defined\(USE_ISO14888_3_ECRDSA\) \*/", "", src, flags=re.S)
    with tempfile.NamedTemporaryFile("w", suffix=".h", encoding="latin-1") as tf:
        tf.write(src)
        tf.flush()
        arrays, nonces, cases = E.load(tf.name)
    # (messages and ids declared as `unsigned char x[] = {..}` or `char x[] = ".."`, which extract_kats' u8 pattern leaves out)
    for m in ARR2.finditer(src):
        arrays.setdefault(m.group(1), E.c_string(m.group(2)) if m.group(2).startswith('"') else E.parse_bytes(m.group(2)))

    def named(expr):
        return arrays[re.sub(r"^\(const (?:char|u8)\s*\*\)\s*", "", expr)]

    for kind, cname, f in cases:
        name, hname = f.get("sig_type"), f.get("hash_type")
        if kind != "ec_test_case" or (name, hname) not in (("SM2", "SM3"), ("ECRDSA", "STREEBOG256"), ("ECRDSA", "STREEBOG512")):
            continue
        curve = E.curve_of(f)
        curve = KAT_CURVES.get(curve, curve)
        msg = E.c_string(f["msg"]) if f["msg"].startswith('"') else named(f["msg"])
        if f.get("msglen", "").isdigit():
            msg = msg[:int(f["msglen"])]
        ident = b""
        if f.get("adata", "NULL") != "NULL":
            ident = named(f["adata"])
            if f.get("adata_len", "").isdigit():
                ident = ident[:int(f["adata_len"])]
        x = int.from_bytes(arrays[f["priv_key"]], "big")
        sig = arrays[f["exp_sig"]]
        alg = S.SCHEMES[name]
        with M.swapped(M.ref_hash, hname, ident):
            pub = S.pt_bytes(curve, S.pub_point(curve, alg, x))
            ver.append(verify_item(curve, name, hname, "reference:" + cname, ident, msg, pub, sig))
            assert ver[-1]["ret"] == 0, cname
            nr = f.get("nn_random", "NULL")
            if nr in nonces:
                sgn.append(sign_item(curve, name, hname, "reference:" + cname, ident, msg, x, int.from_bytes(nonces[nr], "big")))
                assert sgn[-1]["sig"] == sig.hex(), cname


def build():
    rng = np.random.default_rng(SEED)
    ver, sgn = [], []
    reference_vectors(ver, sgn)
    for name, hname, curve in M.COMBOS:
        alg = S.SCHEMES[name]
        ident = S.SM2_ID if alg == S.SM2 else b""
        with M.swapped(M.ref_hash, hname, ident or S.SM2_ID):
            for family, items in S.verify_families(curve, alg, rng).items():
                for h, msg, pub, sig in items:
                    ver.append(verify_item(curve, name, h, family, ident, msg, pub, sig))
            for family, items in S.sign_families(curve, alg, rng).items():
                for h, msg, x, k in items:
                    sgn.append(sign_item(curve, name, h, family, ident, msg, x, k))
        if alg != S.SM2:
            continue
        q = O.CURVES[curve]["q"]
        for n in ID_LENGTHS:
            ident = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
            with M.swapped(M.ref_hash, hname, ident):
                x, k = 1 + S.rand_int(rng, q - 2), 1 + S.rand_int(rng, q - 1)
                msg = rng.integers(0, 256, size=int(rng.integers(1, 48)), dtype=np.uint8).tobytes()
                sgn.append(sign_item(curve, name, hname, "id_len_%d" % n, ident, msg, x, k))
                assert sgn[-1]["ret"] == 0
                pub, sig = bytes.fromhex(sgn[-1]["pub"]), bytes.fromhex(sgn[-1]["sig"])
                ver.append(verify_item(curve, name, hname, "id_len_%d" % n, ident, msg, pub, sig))
                ver.append(verify_item(curve, name, hname, "id_len_%d_tampered" % n, ident, msg + b"!", pub, sig))
    return {"hash": hash_kats(), "verify": ver, "sign": sgn}


def dumps(fx):
    """one item per line"""
    out = ["{"]
    kinds = ("hash", "sign", "verify")
    for ki, kind in enumerate(kinds):
        out.append(json.dumps(kind) + ": [")
        for j, i in enumerate(fx[kind]):
            out.append(json.dumps(i, sort_keys=True) + ("," if j + 1 < len(fx[kind]) else ""))
        out.append("]," if ki + 1 < len(kinds) else "]")
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(M.FIXTURE, "w") as f:
        f.write(dumps(fx))
    print("wrote", {k: len(v) for k, v in fx.items()}, os.path.getsize(M.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
