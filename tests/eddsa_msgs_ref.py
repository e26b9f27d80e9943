"""EdDSA from the ragged message array (ec_eddsa_verify_msgs_batch, ec_eddsa_sign_msgs_batch): the cases of tests/golden/eddsa_msgs.json
and their inputs from seeds, the UNMODIFIED reference's verification through ctypes on oracle/_ref/libecc_ref.so's own symbols
(eddsa_import_pub_key + ec_verify with adata; signing is eddsa_sign_ref.ref_sign), the damaged variants of an item, and the host build
of the per-item steps (tests/eddsa_msgs_host_shim.cpp)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import eddsa_sign_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eddsa_msgs.json")
SHIM_SRC = os.path.join(HERE, "eddsa_msgs_host_shim.cpp")
BUILD = os.path.join(HERE, "_build")
CSRC = os.path.join(os.path.dirname(HERE), "libecc_amd", "csrc")

NAMES = ["EDDSA25519", "EDDSA25519CTX", "EDDSA25519PH", "EDDSA448", "EDDSA448PH"]
ALGS = [E.ALGS[n] for n in NAMES]
Q25519 = 2 ** 252 + 27742317777372353535851937790883648493
Q448 = 2 ** 446 - 13818066809895115352007386748515426880336692474882178609894547503885
MAX_HASHED = 1 << 28
BASE_LENS = [0, 1, 7, 8, 9, 15, 16, 17]
PAST_SLOT, LONG = 4093, 70001
# input lengths around the padding boundaries of the two hashes, and one block further: SHA-512 pads into the block up to 111 octets
# and opens another from 112, its block is 128; SHAKE256 absorbs 136 octets per permutation
SHA512_EDGES = [111, 112, 113, 127, 128, 129, 239, 240, 241, 255, 256, 257]
SHAKE256_EDGES = [135, 136, 137, 271, 272, 273]
CTX_LENS = [0, 1, 255]
EDGE_CTX = 1   # the context length under which the boundary lengths are derived (an odd dom: segments end off the words)


def order(alg):
    return Q448 if E.is448(alg) else Q25519


def edges(alg):
    return SHAKE256_EDGES if E.is448(alg) else SHA512_EDGES


def stream(tag, n):
    return hashlib.shake_256(tag.encode()).digest(n) if n else b""


def context(alg, clen):
    """the call's adata: EDDSA25519 hashes no dom and takes none"""
    return stream("eddsa_msgs/ctx/%d" % clen, clen) if E.takes_ctx(alg) else None


def dlen(alg, adata):
    return len(E.dom(alg, adata))


def fixed_parts(alg, adata):
    """the octets in front of the message in the hashes that absorb it: {hash name: length}.  The PH variants absorb the message alone
    (the pre-hash); their r_hash and hram inputs have one length whatever the message."""
    if E.is_ph(alg):
        return {"prehash": 0}
    d, kl = dlen(alg, adata), E.klen(alg)
    return {"r_hash": d + kl, "hram": d + 2 * kl}


def edge_lens(alg):
    """the message lengths that put each message-absorbing hash input at every edge of edges(alg); asserts that each edge is reached"""
    adata = context(alg, EDGE_CTX)
    out = set()
    for what, fixed in fixed_parts(alg, adata).items():
        hit = {t for t in edges(alg) if t >= fixed}
        assert hit == set(edges(alg)), (alg, what, fixed)
        out |= {t - fixed for t in hit}
    return sorted(out)


def cases(alg):
    """[(context length or None, message length)]"""
    if not E.takes_ctx(alg):
        return [(None, m) for m in sorted(set(BASE_LENS + edge_lens(alg))) + [PAST_SLOT, LONG]]
    out = []
    for cl in CTX_LENS:
        lens = sorted(set(BASE_LENS + (edge_lens(alg) if cl == EDGE_CTX else []))) + [PAST_SLOT] + ([LONG] if cl == EDGE_CTX else [])
        out += [(cl, m) for m in lens]
    return out


def case_input(alg, idx):
    """(secret key, adata or None, message) of case idx"""
    cl, mlen = cases(alg)[idx]
    return stream("eddsa_msgs/sk/%d/%d" % (alg, idx), E.klen(alg)), context(alg, cl or 0), stream("eddsa_msgs/msg/%d/%d" % (alg, idx), mlen)


def coverage(alg):
    """{hash name: the set of edges its input reaches over cases(alg)}"""
    got = {}
    for idx, (cl, mlen) in enumerate(cases(alg)):
        for what, fixed in fixed_parts(alg, context(alg, cl or 0)).items():
            got.setdefault(what, set()).add(fixed + mlen)
    return {what: v & set(edges(alg)) for what, v in got.items()}


# ---- damaged variants ----
KINDS = ["honest", "R", "S", "A", "msg", "S+q", "key"]


def damaged(alg, pub, sig, msg, other_pub):
    """[(kind, pub, sig, msg)]: the honest triple, a flipped bit in R, in S, in A and in the last message octet (not for an empty
    message), S + q, and another case's key"""
    kl = E.klen(alg)
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    s_plus_q = (int.from_bytes(sig[kl:], "little") + order(alg)).to_bytes(kl, "little")
    out = [("honest", pub, sig, msg), ("R", pub, flip(sig, 0), msg), ("S", pub, flip(sig, kl), msg), ("A", flip(pub, 0), sig, msg)]
    if msg:
        out.append(("msg", pub, sig, msg[:-1] + bytes([msg[-1] ^ 0x80])))
    return out + [("S+q", pub, sig[:kl] + s_plus_q, msg), ("key", other_pub, sig, msg)]


# ---- the reference ----
def ref_verify(alg, pub, sig, adata, msg):
    """the unmodified reference -- needs oracle/_ref: eddsa_import_pub_key + ec_verify with adata, 0 / -1"""
    import sigfam_ref as R
    L, params = R.ref_params(E.curve_of(alg))
    L.eddsa_import_pub_key.argtypes = [C.c_void_p, C.c_char_p, C.c_uint16, C.c_void_p, C.c_int]
    key = C.create_string_buffer(R.BUF)
    if L.eddsa_import_pub_key(key, pub, len(pub), params, alg) != 0:
        return -1
    mbuf = C.create_string_buffer(msg, max(1, len(msg)))
    ret = L.ec_verify(sig, len(sig), key, mbuf, len(msg), alg, E.SHAKE256 if E.is448(alg) else E.SHA512, adata, len(adata) if adata is not None else 0)
    return -1 if ret != 0 else 0


# ---- the fixture ----
def load_fixture():
    """tests/golden/eddsa_msgs.json: {"cases": {name: {"pubs": [hex], "sigs": [hex], "verdicts": ["v,v,..." in the order of damaged()]}},
    "sha256": SHA-256 over every public key and signature in order}; the cases and their inputs are cases() / case_input()"""
    with open(FIXTURE) as f:
        return json.load(f)


def fixture_items(fx, alg):
    """[{"sk", "adata", "msg", "pub", "sig", "variants": [(kind, pub, sig, msg, verdict)]}] of one alg"""
    rec = fx["cases"][NAMES[ALGS.index(alg)]]
    n = len(cases(alg))
    assert len(rec["sigs"]) == len(rec["pubs"]) == len(rec["verdicts"]) == n
    pubs, sigs = [bytes.fromhex(p) for p in rec["pubs"]], [bytes.fromhex(s) for s in rec["sigs"]]
    out = []
    for idx in range(n):
        sk, adata, msg = case_input(alg, idx)
        var = damaged(alg, pubs[idx], sigs[idx], msg, pubs[(idx + 1) % n])
        verdicts = [int(v) for v in rec["verdicts"][idx].split(",")]
        assert len(var) == len(verdicts)
        out.append({"sk": sk, "adata": adata, "msg": msg, "pub": pubs[idx], "sig": sigs[idx],
                    "variants": [v + (w,) for v, w in zip(var, verdicts)]})
    return out


def by_context(items):
    """{adata: [item]} in first-seen order: one call takes one context"""
    out = {}
    for it in items:
        out.setdefault(it["adata"], []).append(it)
    return out


# ---- the host build of the per-item steps ----
def build_shim(main=False):
    """tests/eddsa_msgs_host_shim.cpp as a ctypes library, or (main) as a stand-alone program built with the address and
    undefined-behaviour sanitizers: the path of what was built"""
    os.makedirs(BUILD, exist_ok=True)
    if main:
        exe = os.path.join(BUILD, "eddsa_msgs_host_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", "-DEDDSA_MSGS_MAIN", "-o", exe, SHIM_SRC])
        return exe
    so = os.path.join(BUILD, "eddsa_msgs_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM_SRC])
    return so


_shim = []


def shim():
    if not _shim:
        L = C.CDLL(build_shim())
        u64, u32, cp = C.c_uint64, C.c_uint32, C.c_char_p
        L.edm_item_ok.argtypes = [C.c_int, u64, u64, u64, u32]
        L.edm_vhram.argtypes = [C.c_int, cp, u32, cp, cp, cp, u64, u64, u64, cp]
        L.edm_sign_hashes.argtypes = [C.c_int, cp, u32, cp, cp, cp, cp, u64, u64, u64, cp, cp, cp]
        _shim.append(L)
    return _shim[0]


def shim_vhram(alg, adata, R_enc, A_enc, arr, off0, off1, total=None):
    """(bad, hram) of the verifier's step for the item arr[off0 .. off1) of an array of `total` octets"""
    out = C.create_string_buffer(114)
    bad = shim().edm_vhram(alg, adata, len(adata) if adata else 0, R_enc, A_enc, arr, off0, off1, len(arr) if total is None else total, out)
    assert bad in (0, 1), bad
    return bad, out.raw[:2 * E.klen(alg)]


def shim_sign_hashes(alg, adata, sk, R_enc, A_enc, arr, off0, off1, total=None):
    """(bad, a, r_hash, hram) of the signer's two steps for the same item; R_enc is what [r]B encodes to"""
    kl = E.klen(alg)
    a, rh, h = C.create_string_buffer(57), C.create_string_buffer(114), C.create_string_buffer(114)
    bad = shim().edm_sign_hashes(alg, adata, len(adata) if adata else 0, sk, R_enc, A_enc, arr, off0, off1, len(arr) if total is None else total,
                                 a, rh, h)
    assert bad in (0, 1), bad
    return bad, a.raw[:kl], rh.raw[:2 * kl], h.raw[:2 * kl]
