"""Shared by tests/golden/make_sighash_ht_fixture.py, tests/test_sighash_ht_host.py and tests/test_gpu_sighash_ht.py: ECKCDSA, ECSDSA,
ECOSDSA, ECFSDSA and BIP0340 over every hash of ec_digest_slots_batch -- the cases, their items (derived from their index, so that
the fixture records answers only), the unmodified reference through ctypes, a Python-integer restatement of the five schemes over any
hash, and the host build of libecc_amd/csrc/ecamd_bip0340_nonce_ht.h.

H(name, data) is hashlib's where hashlib has the hash here (hmac_ht_ref.have_hashlib: SHA-2, SHA-3, SHA-512/t, SM3 on this OpenSSL) and
otherwise the host build of the hash traits (hmac_ht_ref.shim_hash: Streebog, BASH, RIPEMD-160 where OpenSSL has dropped it), which
tests/test_hmac_ht_host.py pins to the reference's known answers.  For those hashes the restatement is therefore no second
reference of the HASH; it still is one of the scheme around it.

A case is (scheme, curve, hash); it has N = 130 signing items and 130 verification items:
  signing item i        key x (one of eight per case; BIP0340: keys 0 .. 3 have an odd Y.y, 4 .. 7 an even one), v (the nonce k, or
                        BIP0340's aux value), the message; SIGN_EDGES replace x or v at fixed indices
  verification item i   the reference's signature of signing item i (of i - 120 for the last ten), corrupted as VERIFY_EDGES says
Message lengths walk msg_lengths() round and round: the whole hash input (ECKCDSA: z || m) lands on BLOCK - 1, BLOCK, BLOCK + 1 and, for
the Merkle-Damgard hashes, on both sides of the point where the length field no longer fits; the empty message; several blocks."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import oracles as O
import sigfam_ref as SF
import schnorr_ref as S
import hmac_ht_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sighash_ht.json")
SHIM_SRC = os.path.join(HERE, "bip0340_nonce_ht_host_shim.cpp")
BUILD = os.path.join(HERE, "_build")

ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA, BIP0340 = 2, 3, 4, 5, 20          # libecc's ec_alg_type numbers
SCHEMES = {"ECKCDSA": ECKCDSA, "ECSDSA": ECSDSA, "ECOSDSA": ECOSDSA, "ECFSDSA": ECFSDSA, "BIP0340": BIP0340}
HSIG = (ECKCDSA, ECSDSA, ECOSDSA)                                    # ec_sig_hashed_*; the other two: ec_schnorr_*
NEW_NAMES = M.NEW_NAMES                                              # the 14 hashes the older names refuse
TWIN = "SHA256"                                                      # through the new name, byte for byte the old name's
HASH_IDS, HSIZE, BLOCK = M.HASH_IDS, M.HASH_SIZES, M.BLOCKS
NOT_SERVED = M.NOT_SERVED
N = M.N_GPU                                                          # 130: two full waves and a tail of two lanes
N_KEYS = 8
N_FULL = 2                                                           # signatures the fixture keeps in full, in the cases of full_kept()
TAG_W = 1                                                            # characters of a signature's tag in the fixture
TAG_AUX, TAG_NONCE, TAG_CHALLENGE = b"BIP0340/aux", b"BIP0340/nonce", b"BIP0340/challenge"
# length-field Merkle-Damgard hashes: libecc's number -> octets of (0x80 and the length field)
MD_TAIL = {1: 9, 2: 9, 11: 9, 15: 9, 3: 17, 4: 17, 9: 17, 10: 17}


def curves_for(scheme):
    """SECP192R1: hsize 28 .. 64 > qlen 24 and RIPEMD-160's 20 < 24 (ECKCDSA's min(hsize, qlen) both ways); a 256-bit curve;
    BRAINPOOLP384R1; SECP521R1: hsize 64 < qlen 66, 2 clen = 132 octets over two or more blocks of every hash"""
    return ["SECP192R1", "SECP256K1" if scheme == "BIP0340" else "SECP256R1", "BRAINPOOLP384R1", "SECP521R1"]


def cases():
    return [(s, c) for s in SCHEMES for c in curves_for(s)]


def H(name, data):
    if M.have_hashlib(name):
        return M.py_hash(name, data)
    return M.shim_hash(name, data)


_curve = SF._curve
pt_bytes = SF.pt_bytes
py_mul, py_add = S.py_mul, S.py_add


# ---- geometry ----
def r_len(alg, name, curve):
    cl, ql = O.clen(curve), O.qlen(curve)
    if alg == ECKCDSA:
        return min(HSIZE[name], ql)
    if alg in (ECSDSA, ECOSDSA):
        return HSIZE[name]
    return cl if alg == BIP0340 else 2 * cl


def sig_len(alg, name, curve):
    return r_len(alg, name, curve) + O.qlen(curve)


def fixed_len(alg, name, curve):
    """octets of the hash input in front of the message (ECKCDSA: of h = H(z || m), which the caller hashes)"""
    cl = O.clen(curve)
    return {ECKCDSA: BLOCK[name], ECSDSA: 2 * cl, ECOSDSA: cl, ECFSDSA: 2 * cl, BIP0340: 2 * HSIZE[name] + 2 * cl}[alg]


def msg_lengths(alg, name, curve):
    b, fl = BLOCK[name], fixed_len(alg, name, curve)
    targets = [b - 1, b, b + 1]
    tail = MD_TAIL.get(HASH_IDS[name])
    if tail:
        targets += [b - tail, b - tail + 1]          # the length field just fits / no longer fits
    return [0] + [(t - fl) % b for t in targets] + [3 * b + 5]


def max_msg(name):
    return 4 * BLOCK[name] + 5


def stride_for(alg, name, curve):
    return (4 + (0 if alg == ECKCDSA else fixed_len(alg, name, curve)) + max_msg(name) + 3) & ~3


# ---- items ----
SIGN_EDGES = {120: "v=0", 121: "v=max", 122: "x=0", 123: "x=q", 124: "x=q+1"}
#   v=max: k = q for the four schemes that take a nonce (refused); aux = 2^(8 qlen) - 1 for BIP0340 (signs: aux is any qlen octets)
#   v=0:   k = 0 (refused); aux = 0 (signs)
VERIFY_EDGES = {100: "s=0", 101: "s=q", 102: "s=q-1", 103: "r^first", 104: "r^last", 105: "key_off_curve", 106: "w_off_curve",
                107: "msg^", 110: "slot_short", 111: "slot_unfit"}
#   w_off_curve: ECFSDSA only (W.y + 1); for the others item 106 appends an octet to the message
#   slot_short / slot_unfit: the slot's length word is one less than the fixed fields / three more than the stride holds.  No
#   reference call has such an input: the entry points define result 1 (ECKCDSA takes digests, not slots: its two items are honest)


def _seed_int(tag, seed, nbytes):
    out = b""
    j = 0
    while len(out) < nbytes:
        out += hashlib.sha512(tag + seed + bytes([j])).digest()
        j += 1
    return int.from_bytes(out[:nbytes], "big")


_keys = {}


def key(scheme, curve, j):
    """private key j (0 .. 7) of (scheme, curve), in [1, q - 1]; BIP0340: j < 4 has Y.y odd, j >= 4 even (searched once per curve)"""
    if (scheme, curve, j) not in _keys:
        p, a, b, q, G = _curve(curve)
        t = 0
        while True:
            x = 1 + _seed_int(b"x", ("%s/%s/%d/%d" % (scheme, curve, j, t)).encode(), O.qlen(curve) + 8) % (q - 1)
            if scheme != "BIP0340" or bool(py_mul(x, G, a, p)[1] & 1) == (j < 4):
                break
            t += 1
        _keys[(scheme, curve, j)] = x
    return _keys[(scheme, curve, j)]


_pubs = {}


def pub(scheme, curve, j):
    """the public key of key(j) as affine octets: [1/x]G for ECKCDSA, [x]G otherwise"""
    if (scheme, curve, j) not in _pubs:
        p, a, b, q, G = _curve(curve)
        x = key(scheme, curve, j)
        _pubs[(scheme, curve, j)] = pt_bytes(curve, py_mul(pow(x, -1, q) if scheme == "ECKCDSA" else x, G, a, p))
    return _pubs[(scheme, curve, j)]


def sign_item(scheme, curve, name, i):
    """(x, v, message) of signing item i"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    seed = ("%s/%s/%s/%d" % (scheme, curve, name, i)).encode()
    ls = msg_lengths(SCHEMES[scheme], name, curve)
    ml = ls[i % len(ls)]
    msg = bytes(_seed_int(b"m", seed, ml).to_bytes(ml, "big")) if ml else b""
    x = key(scheme, curve, i % N_KEYS)
    if scheme == "BIP0340":
        v = _seed_int(b"a", seed, ql)
    else:
        v = 1 + _seed_int(b"k", seed, ql + 8) % (q - 1)
    edge = SIGN_EDGES.get(i)
    if edge == "v=0":
        v = 0
    elif edge == "v=max":
        v = (1 << (8 * ql)) - 1 if scheme == "BIP0340" else q
    elif edge == "x=0":
        x = 0
    elif edge == "x=q":
        x = q
    elif edge == "x=q+1":
        x = q + 1 if q + 1 < (1 << (8 * ql)) else q
    return x, v, msg


def flip(bs, i, bit=1):
    return bs[:i] + bytes([bs[i] ^ bit]) + bs[i + 1:]


def verify_item(scheme, curve, name, i, sigs):
    """(public key octets, signature, message, slot fault or None) of verification item i; sigs: the reference's signatures of the signing items"""
    alg = SCHEMES[scheme]
    q, p, cl, ql = O.CURVES[curve]["q"], O.CURVES[curve]["p"], O.clen(curve), O.qlen(curve)
    j = i - 120 if i >= 120 else i
    x, v, msg = sign_item(scheme, curve, name, j)
    pk, sig = pub(scheme, curve, j % N_KEYS), sigs[j]
    rl = r_len(alg, name, curve)
    edge = VERIFY_EDGES.get(i)
    fault = None
    if edge in ("s=0", "s=q", "s=q-1"):
        sig = sig[:rl] + {"s=0": 0, "s=q": q, "s=q-1": q - 1}[edge].to_bytes(ql, "big")
    elif edge == "r^first":
        sig = flip(sig, 0)
    elif edge == "r^last":
        sig = flip(sig, rl - 1)
    elif edge == "key_off_curve":
        pk = pk[:cl] + ((int.from_bytes(pk[cl:], "big") + 1) % p).to_bytes(cl, "big")
    elif edge == "w_off_curve":
        if alg == ECFSDSA:
            sig = sig[:cl] + ((int.from_bytes(sig[cl:2 * cl], "big") + 1) % p).to_bytes(cl, "big") + sig[2 * cl:]
        else:
            msg = msg + b"!"
    elif edge == "msg^":
        msg = flip(msg, 0) if msg else b"?"
    elif edge in ("slot_short", "slot_unfit") and alg != ECKCDSA:
        fault = edge
    return pk, sig, msg, fault


def kcdsa_h(name, pk, msg):
    """ECKCDSA's h = H(z || m): z is the first BLOCK octets of the public key's octets, zero-padded"""
    return H(name, kcdsa_z(name, pk) + msg)


def kcdsa_z(name, pk):
    return (pk + bytes(BLOCK[name]))[:BLOCK[name]]


def slot(alg, name, curve, msg, stride, r=None, fault=None):
    """what the entry points take for an item: `u32 length | fixed fields | message`, the fields the device fills left blank (r: the
    commitment octets a verification slot carries for ECFSDSA / BIP0340 -- the device writes the signature's own over them)"""
    cl, hs = O.clen(curve), HSIZE[name]
    if alg == BIP0340:
        t = H(name, TAG_CHALLENGE)
        body = t + t + (bytes(cl) if r is None else r) + bytes(cl) + msg
    elif alg == ECFSDSA:
        body = (bytes(2 * cl) if r is None else r) + msg
    else:
        body = bytes(2 * cl if alg == ECSDSA else cl) + msg
    ln = len(body)
    if fault == "slot_short":
        ln = (fixed_len(alg, name, curve) if alg != ECKCDSA else 0) - 1
    elif fault == "slot_unfit":
        ln = stride - 3
    assert 4 + len(body) <= stride
    return ln.to_bytes(4, "little") + body + bytes(stride - 4 - len(body))


# ---- the Python-integer restatement over any hash ----
def commit_digest(alg, name, curve, W, msg, yx=b""):
    cl = O.clen(curve)
    wx, wy = W[0].to_bytes(cl, "big"), W[1].to_bytes(cl, "big")
    if alg == ECKCDSA:
        return H(name, wx)
    if alg == ECSDSA:
        return H(name, wx + wy + msg)
    if alg == ECOSDSA:
        return H(name, wx + msg)
    if alg == ECFSDSA:
        return H(name, wx + wy + msg)
    t = H(name, TAG_CHALLENGE)
    return H(name, t + t + wx + yx + msg)


def kcdsa_e(r, h, q):
    return int.from_bytes(bytes(u ^ v for u, v in zip(r, h[len(h) - len(r):])), "big") % q


def nonce_from_pub(name, curve, x, pk, aux, msg):
    """k of _bip0340_sign (sig/bip0340.c:237-294) over H, for 0 < x < q and the key pair's public octets pk; 0 where it fails"""
    q, cl, ql, hs = O.CURVES[curve]["q"], O.clen(curve), O.qlen(curve), HSIZE[name]
    d = q - x if pk[-1] & 1 else x
    ta, tn = H(name, TAG_AUX), H(name, TAG_NONCE)
    mask = H(name, ta + ta + aux.to_bytes(ql, "big"))
    tl = max(ql, hs)
    t = bytes(u ^ v for u, v in zip(d.to_bytes(ql, "big").ljust(tl, b"\0"), mask.ljust(tl, b"\0")))
    return int.from_bytes(H(name, tn + tn + t + pk[:cl] + msg), "big") % q


def py_bip_nonce(name, curve, x, aux, msg):
    """the same with Y = [x]G computed here"""
    p, a, b, q, G = _curve(curve)
    return nonce_from_pub(name, curve, x, pt_bytes(curve, py_mul(x, G, a, p)), aux, msg)


def py_sign(scheme, curve, name, x, v, msg, k=None):
    """(status, signature) as the entry points return them; v: the nonce, or BIP0340's aux value (k given: BIP0340 signs with it)"""
    alg = SCHEMES[scheme]
    p, a, b, q, G = _curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    bad = (1, bytes(sig_len(alg, name, curve)))
    if alg in (ECKCDSA, BIP0340) and not 0 < x < q:
        return bad
    if alg == ECFSDSA and not x < q:
        return bad
    if k is None:
        k = py_bip_nonce(name, curve, x, v, msg) if alg == BIP0340 else v
    if not 0 < k < q:
        return bad
    W = py_mul(k, G, a, p)
    if alg == BIP0340:
        Y = py_mul(x, G, a, p)
        d, kk = (q - x if Y[1] & 1 else x), (q - k if W[1] & 1 else k)
        e = int.from_bytes(commit_digest(alg, name, curve, W, msg, Y[0].to_bytes(cl, "big")), "big") % q
        return 0, W[0].to_bytes(cl, "big") + ((kk + e * d) % q).to_bytes(ql, "big")
    dg = commit_digest(alg, name, curve, W, msg)
    if alg == ECFSDSA:
        s = (k + int.from_bytes(dg, "big") * x) % q
        return (0, pt_bytes(curve, W) + s.to_bytes(ql, "big")) if s else bad
    rl = r_len(alg, name, curve)
    r = dg[len(dg) - rl:]
    if alg == ECKCDSA:
        pk = pt_bytes(curve, py_mul(pow(x, -1, q), G, a, p))
        s = x * (k - kcdsa_e(r, kcdsa_h(name, pk, msg), q)) % q
    else:
        e = int.from_bytes(r, "big") % q
        if e == 0:
            return bad
        s = (k + e * x) % q
    return (0, r + s.to_bytes(ql, "big")) if s else bad


def py_verify(scheme, curve, name, pk, sig, msg):
    """0 accept / 1 reject"""
    alg = SCHEMES[scheme]
    p, a, b, q, G = _curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    rl = r_len(alg, name, curve)
    Y = SF.import_pub(curve, pk)
    if Y is None:
        return 1
    r, s = sig[:rl], int.from_bytes(sig[rl:], "big")
    if alg in HSIG:
        if not 0 < s < q:
            return 1
        if alg == ECKCDSA:
            u, v = kcdsa_e(r, kcdsa_h(name, pk, msg), q), s
        else:
            u, v = s, -int.from_bytes(r, "big") % q
            if v == 0:
                return 1
        W = py_add(py_mul(u, G, a, p), py_mul(v, Y, a, p), a, p)
        if W is None:
            return 1
        dg = commit_digest(alg, name, curve, W, msg)
        return 0 if dg[len(dg) - rl:] == r else 1
    rx = int.from_bytes(r[:cl], "big")
    if alg == BIP0340:
        if rx >= p or s >= q:
            return 1
        e = int.from_bytes(commit_digest(alg, name, curve, (rx, 0), msg, pk[:cl]), "big") % q
        if Y[1] & 1:
            Y = (Y[0], p - Y[1])
        R = py_add(py_mul(s, G, a, p), py_mul(-e % q, Y, a, p), a, p)
        return 0 if R is not None and not (R[1] & 1) and R[0] == rx else 1
    ry = int.from_bytes(r[cl:], "big")
    if rx >= p or ry >= p or (ry * ry - rx * rx * rx - a * rx - b) % p or not 0 < s < q:
        return 1
    e = int.from_bytes(commit_digest(alg, name, curve, (rx, ry), msg), "big") % q
    W = py_add(py_mul(s, G, a, p), py_mul(-e % q, Y, a, p), a, p)
    return 0 if W == (rx, ry) else 1


def bip_k_even(name, curve, j, sig, msg):
    """BIP0340: k' = s - e d' mod q, the nonce AFTER the flip by the parity of R.y, from a signature of key j: the generator's k is
    k' when R.y is even and q - k' when it is odd"""
    q, cl = O.CURVES[curve]["q"], O.clen(curve)
    x, pk = key("BIP0340", curve, j), pub("BIP0340", curve, j)
    d = q - x if pk[-1] & 1 else x
    t = H(name, TAG_CHALLENGE)
    e = int.from_bytes(H(name, t + t + sig[:cl] + pk[:cl] + msg), "big") % q
    return (int.from_bytes(sig[cl:], "big") - e * d) % q


# ---- the unmodified reference -- needs oracle/_ref ----
def ref_sign(scheme, curve, name, x, v, msg):
    """ec_key_pair_import_from_priv_key_buf + _ec_sign whose `rand` hook returns v once (the nonce, asked below q; BIP0340: the aux
    value, asked below 2^(8 qlen)): (ret, signature or None); ret -2: the key pair did not import"""
    alg = SCHEMES[scheme]
    L, params = SF.ref_params(curve)
    ql = O.qlen(curve)
    kp = C.create_string_buffer(SF.BUF)
    if x >= 1 << (8 * ql) or L.ec_key_pair_import_from_priv_key_buf(kp, params, x.to_bytes(ql, "big"), ql, alg) != 0:
        return -2, None
    calls = [0]
    vb = v.to_bytes(ql + 1, "big")

    def hook(out, bound):
        calls[0] += 1
        if calls[0] > 1:
            return -1          # a restart: the same value again would loop for ever
        cmp = C.c_int(0)
        if L.nn_init_from_buf(out, vb, len(vb)) != 0 or L.nn_cmp(out, bound, C.byref(cmp)) != 0:
            return -1
        return -1 if cmp.value >= 0 else 0

    cb = SF.RAND_FN(hook)
    sl = sig_len(alg, name, curve)
    sig = C.create_string_buffer(sl)
    ret = L._ec_sign(sig, sl, kp, msg, len(msg), cb, alg, HASH_IDS[name], None, 0)
    return (0, sig.raw[:sl]) if ret == 0 else (-1, None)


def ref_verify(scheme, curve, name, pk, sig, msg):
    """ec_pub_key_import_from_aff_buf + ec_verify: 0 / 1"""
    alg = SCHEMES[scheme]
    L, params = SF.ref_params(curve)
    kb = C.create_string_buffer(SF.BUF)
    if L.ec_pub_key_import_from_aff_buf(kb, params, pk, len(pk), alg) != 0:
        return 1
    return 1 if L.ec_verify(sig, len(sig), kb, msg, len(msg), alg, HASH_IDS[name], None, 0) != 0 else 0


# ---- the fixture ----
_B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"


def tag(sig):
    """six bits of SHA-256(signature) as one character: it says WHICH item differs; "all" is the check"""
    return _B64[hashlib.sha256(sig).digest()[0] & 63]


def checksum(parts):
    return hashlib.sha256(b"".join(parts)).hexdigest()


def case_key(scheme, curve, name):
    return "%s/%s/%s" % (scheme, curve, name)


def full_kept(scheme, curve, name):
    """the cases whose first signatures the fixture keeps in full, and whose corrupted items the Python restatement verifies: three
    or four hashes per (scheme, curve) -- the four curves of a scheme take NEW_NAMES[0::4], [1::4], [2::4] and [3::4], so every one of
    the 14 hashes is kept on exactly one curve of every scheme (tests/test_sighash_ht_host.py asserts that)"""
    return name in NEW_NAMES[cases().index((scheme, curve)) % 4::4]


def pack(rec):
    """a case as the file holds it: [tags, all, rets as digits of -ret, the verdicts of VERIFY_EDGES in order of index, rodd as a
    hexadecimal bit field (item i at bit i) or "", first]"""
    rodd = "%x" % sum(1 << i for i, c in enumerate(rec["rodd"]) if c == "1") if "rodd" in rec else ""
    return [rec["tags"], rec["all"], "".join(str(-r) for r in rec["rets"]), "".join(rec["ver"][i] for i in sorted(VERIFY_EDGES)), rodd,
            rec["first"]]


def unpack(key, row):
    tags, all_, rets, ver_e, rodd, first = row
    rec = {"tags": tags, "all": all_, "rets": [-int(c) for c in rets], "first": first}
    ver = ["0"] * N
    for i, c in zip(sorted(VERIFY_EDGES), ver_e):
        ver[i] = c
    rec["ver"] = "".join(ver)
    if key.startswith("BIP0340/"):
        bits, unsigned = int(rodd, 16), {i for i, r in zip(sorted(SIGN_EDGES), rec["rets"]) if r != 0}
        rec["rodd"] = "".join("-" if i in unsigned else str(bits >> i & 1) for i in range(N))
    return rec


def load_fixture():
    """tests/golden/sighash_ht.json, one row per "SCHEME/CURVE/HASH" (pack), as
      "first"  the signatures of signing items 0 .. N_FULL - 1 in full, in the cases of full_kept(); [] in the others
      "tags"   tag(signature) of every signing item that signed, concatenated in order (TAG_W characters each)
      "rets"   the reference's return value for the items of SIGN_EDGES, in order of index (0, -1: _ec_sign failed, -2: no key pair)
      "all"    SHA-256 over all signatures in order
      "ver"    the reference's verdict per verification item, '0' accept / '1' reject ('1' for the two slot faults, which the
               entry points define and no reference call can have); the file holds those of VERIFY_EDGES: the recorder asserted that
               the reference accepted every other item
      "rodd"   BIP0340 only: per signing item '1' where the commitment [k]G has an odd y, '0' where even, '-' where it did not sign"""
    with open(FIXTURE) as f:
        return {k: unpack(k, row) for k, row in json.load(f).items()}


def expected_sigs(rec, scheme, curve, name, got):
    """assert that got = [(status, signature)] of the N signing items are the reference's"""
    alg = SCHEMES[scheme]
    sl = sig_len(alg, name, curve)
    rets = dict(zip(sorted(SIGN_EDGES), rec["rets"]))
    assert len(got) == N
    signed = []
    for i, (st, sig) in enumerate(got):
        ret = rets.get(i, 0)
        assert (st == 0) == (ret == 0), (scheme, curve, name, i, st, ret)
        if ret == 0:
            signed.append(sig)
        else:
            assert sig == bytes(sl), (scheme, curve, name, i)
    for i, h in enumerate(rec["first"]):
        assert got[i][1].hex() == h, (scheme, curve, name, i)
    tags = "".join(tag(s) for s in signed)
    if tags != rec["tags"]:
        bad = [i for i in range(len(signed)) if tags[TAG_W * i:TAG_W * (i + 1)] != rec["tags"][TAG_W * i:TAG_W * (i + 1)]]
        assert False, (scheme, curve, name, "signatures differ at (counting those that signed)", bad[:8])
    assert checksum(signed) == rec["all"], (scheme, curve, name)


def ref_sigs_or_none(rec, scheme, curve, name, got):
    """the signatures per signing item (None where the reference did not sign), taken from `got` once expected_sigs has passed"""
    rets = dict(zip(sorted(SIGN_EDGES), rec["rets"]))
    return [sig if rets.get(i, 0) == 0 else None for i, (st, sig) in enumerate(got)]


# ---- the host build of the unit ----
def build_shim(main=False):
    os.makedirs(BUILD, exist_ok=True)
    if main:
        exe = os.path.join(BUILD, "bip0340_nonce_ht_host_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", "-DBIP_HT_MAIN", "-o", exe, SHIM_SRC])
        return exe
    so = os.path.join(BUILD, "bip0340_nonce_ht_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM_SRC])
    return so


_shim = []


def shim():
    if not _shim:
        L = C.CDLL(build_shim())
        L.bh_nonce.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p,
                               C.POINTER(C.c_uint32)]
        L.bh_tag.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
        _shim.append(L)
    return _shim[0]


def shim_nonce(name, curve, x, pk, aux, msg):
    """(status, k, compression / permutation / g_N calls) of the unit for a key of qlen octets"""
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    out, calls = C.create_string_buffer(ql), C.c_uint32()
    st = shim().bh_nonce(HASH_IDS[name], x.to_bytes(ql, "big"), pk, cl, aux.to_bytes(ql, "big"), msg, len(msg), q.to_bytes(ql, "big"),
                         q.bit_length(), out, C.byref(calls))
    return st, int.from_bytes(out.raw[:ql], "big"), calls.value


def shim_tag(name, t):
    out = C.create_string_buffer(64)
    assert shim().bh_tag(HASH_IDS[name], t, len(t), out) == HSIZE[name]
    return out.raw[:HSIZE[name]]
