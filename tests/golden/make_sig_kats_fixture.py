#!/usr/bin/env python3
"""Turn the reference's OWN signature known answers of ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA, ECGDSA, BIGN and DBIGN into a fixture that
travels without the reference tree:
    python tests/golden/make_sig_kats_fixture.py  ->  tests/golden/sig_kats.json
Sources, read as data the way tests/golden/extract_kats.py and tests/golden/make_sig_msg_fixture.py read them (byte arrays, the
record fields that bind them, the nonce of each case's nn_random callback; the ECRDSA branches the default build does not compile
removed):
    src/tests/ec_self_tests_core.h   10 ECKCDSA, 8 ECSDSA, 8 ECOSDSA, 8 ECFSDSA, 4 ECGDSA (ISO/IEC 14888-3 and TTA examples)
    src/tests/bign_test_vectors.h    8 BIGN (STB 34.101.45: belt-hash on bign256v1, BASH384 on bign384v1, BASH512 on bign512v1)
    src/tests/dbign_test_vectors.h   DBIGN 4 - 7 (1 - 3 are in tests/golden/det_sign.json already)
The format of a case is described in tests/sigkats_ref.py.  Before anything is written the script asserts, per case, that
  * the unmodified reference (oracle/_ref) accepts the published triple, and _ec_sign with the recorded nonce returns the published
    bytes (DBIGN: its deterministic signer does, and so does BIGN's signer with the nonce solved from the signature);
  * the Python restatement of the family signs to the same bytes and gives the reference's verdict for every variant;
  * every damaged variant is rejected: a fixture whose non-honest variants are not all -1 cannot tell an always-accept kernel from a
    right one.
It prints the number of cases per family."""
import json
import os
import re
import sys
import tempfile
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracles as O  # noqa: E402
import sigkats_ref as K  # noqa: E402
import extract_kats as E  # noqa: E402
import make_sig_msg_fixture as G  # noqa: E402

HEADERS = ("ec_self_tests_core.h", "bign_test_vectors.h", "dbign_test_vectors.h")
# extract_kats.NONCE with any white space in the callback's parameter list (some are broken over two lines)
NONCE = re.compile(r"static\s+int\s+(\w+)\(nn_t\s+out,\s*nn_src_t\s+q\)\s*\{(.*?)\n\}", re.S)
IN_DET_SIGN = ("dbign_1_test_case", "dbign_2_test_case", "dbign_3_test_case")      # tests/golden/det_sign.json holds these


def parse(header):
    """(arrays, nonces, cases) of a header: extract_kats.load over the text the default build compiles, with the messages and
    additional data declared as char[] / unsigned char[] added"""
    src = open(os.path.join(E.REF, header), encoding="latin-1").read()
    src = re.sub(r"#else /\* !?defined\(USE_ISO14888_3_ECRDSA\) \*/.*?#endif /\* defined\(USE_ISO14888_3_ECRDSA\) \*/", "", src, flags=re.S)
    with tempfile.NamedTemporaryFile("w", suffix=".h", encoding="latin-1") as tf:
        tf.write(src)
        tf.flush()
        arrays, nonces, cases = E.load(tf.name)
    for m in NONCE.finditer(src):
        inner = E.ARR.search(m.group(2))
        if inner:
            nonces.setdefault(m.group(1), E.parse_bytes(inner.group(2)))
    for m in G.ARR2.finditer(src):
        arrays.setdefault(m.group(1), E.c_string(m.group(2)) if m.group(2).startswith('"') else E.parse_bytes(m.group(2)))
    return arrays, nonces, cases


def published():
    """the cases as the headers give them, in the order of K.ALGS and then of the headers"""
    out = []
    for header in HEADERS:
        arrays, nonces, cases = parse(header)

        def named(expr):
            return arrays[re.sub(r"^\(const (?:char|u8)\s*\*\)\s*", "", expr)]

        for kind, cname, f in cases:
            alg = f.get("sig_type")
            if kind != "ec_test_case" or alg not in K.ALGS or cname in IN_DET_SIGN:
                continue
            curve = E.curve_of(f)
            hname = K.HASH_NAMES.get(f["hash_type"], f["hash_type"])
            msg = E.c_string(f["msg"]) if f["msg"].startswith('"') else named(f["msg"])
            if f.get("msglen", "").isdigit():
                msg = msg[:int(f["msglen"])]
            adata = b""
            if f.get("adata", "NULL") != "NULL":
                adata = named(f["adata"])
                if f.get("adata_len", "").isdigit():
                    adata = adata[:int(f["adata_len"])]
            nr = f.get("nn_random", "NULL")
            out.append({"id": cname, "name": E.c_string(f["name"]).decode(), "curve": curve, "alg": alg, "hash": hname, "msg": msg,
                        "adata": adata, "x": int.from_bytes(arrays[f["priv_key"]], "big"),
                        "k": int.from_bytes(nonces[nr], "big") if nr != "NULL" else None, "sig": arrays[f["exp_sig"]]})
    order = list(K.ALGS)
    return sorted(out, key=lambda c: order.index(c["alg"]))       # (a stable sort: the headers' order within a family)


def flip_bit(bs, at, bit):
    return bs[:at] + bytes([bs[at] ^ (1 << bit)]) + bs[at + 1:]


def record(c, others):
    """the fixture's form of a published case; others: the public keys of the other cases on its curve, in the order they are tried"""
    curve, alg, hname, msg, x, sig = c["curve"], c["alg"], c["hash"], c["msg"], c["x"], c["sig"]
    ql = O.qlen(curve)
    oid = K.oid_of({"adata": c["adata"].hex()}) if alg in K.BIGNS else b""
    assert alg in K.BIGNS or not c["adata"], c["id"]
    dg = K.ref_digest(hname, msg)
    assert dg == K.py_digest(hname, msg), c["id"]
    k = c["k"]
    if alg == "DBIGN":
        assert k is None
        assert K.ref_dbign_sign(curve, hname, x, msg, oid) == (0, sig), c["id"]
        k = K.k_from_sig(curve, x, dg, sig)
    pub = K.pub_of(curve, alg, x)
    assert K.ref_sign(curve, alg, hname, x, k, msg, oid) == (0, sig), (c["id"], "the reference does not sign to the published bytes")
    assert K.py_sign(curve, alg, hname, x, k, msg, dg, oid) == (0, sig), (c["id"], "the restatement does not sign to the published bytes")
    r_len, s_len = K.components(curve, alg, hname)
    assert len(sig) == r_len + s_len, c["id"]
    # the least significant octet of each component (BIGN writes little-endian), so that the damaged number stays in its range and
    # the verdict comes from the scheme's equation, not from a range check
    at = (0, r_len) if alg in K.BIGNS else (r_len - 1, r_len + s_len - 1)
    variants = [{}]
    for comp in (0, 1):
        # if a chosen bit happens to be accepted, the next bit of the same octet is taken (and the script says so)
        for bit in range(8):
            bad = flip_bit(sig, at[comp], bit)
            if K.ref_verify(curve, alg, hname, pub, bad, msg, oid) != 0:
                break
            print("%s: component %d with bit %d flipped is accepted; trying the next bit" % (c["id"], comp, bit))
        variants.append({"sig": bad})
    variants.append({"msg": flip_bit(msg, 0, 7)})
    other = next((p for p in others if p != pub), None)
    if other is not None:
        variants.append({"pub": other})
    out = []
    for j, v in enumerate(variants):
        vp, vs, vm = v.get("pub", pub), v.get("sig", sig), v.get("msg", msg)
        ret = K.ref_verify(curve, alg, hname, vp, vs, vm, oid)
        assert ret == (0 if j == 0 else -1), (c["id"], j, ret)
        assert K.py_verify(curve, alg, hname, vp, vs, vm, K.py_digest(hname, vm), oid) == (0 if ret == 0 else 1), (c["id"], j)
        out.append(dict({f: b.hex() for f, b in v.items()}, ret=ret))
    return {"id": c["id"], "name": c["name"], "curve": curve, "alg": alg, "hash": hname, "msg": msg.hex(), "adata": c["adata"].hex(),
            "x": x.to_bytes(ql, "big").hex(), "k": k.to_bytes(ql, "big").hex(), "pub": pub.hex(), "sig": sig.hex(), "digest": dg.hex(),
            "variants": out}


def build():
    cases = published()
    pubs = [K.pub_of(c["curve"], c["alg"], c["x"]) for c in cases]
    out = []
    for j, c in enumerate(cases):
        # the other cases on the same curve, those after this one first
        others = [pubs[i % len(cases)] for i in range(j + 1, j + len(cases)) if cases[i % len(cases)]["curve"] == c["curve"]]
        out.append(record(c, others))
    return out


def dumps(cases):
    """one case per line"""
    return "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    cases = build()
    with open(K.FIXTURE, "w") as f:
        f.write(dumps(cases))
    n = Counter(c["alg"] for c in cases)
    print("wrote", {a: n[a] for a in K.ALGS}, os.path.getsize(K.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
