"""GPU tests of one-call EdDSA signing (ec_eddsa_sign_msg_batch, ec_eddsa_pub_key_batch and their _dev forms): the RFC 8032 vectors of
the reference, the recorded answers of the unmodified reference (tests/golden/eddsa_sign.json; the reference itself is not read
here) and the Python restatements oracles.ed25519_sign / ed448_sign."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import libecc_amd
import oracles as O
import eddsa_sign_ref as E

pytestmark = pytest.mark.gpu
ALGS = sorted(E.ALGS.values())


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return E.load_fixture(os.path.join(O.GOLDEN, "eddsa_sign.json"))


def groups(items):
    """the items of one variant by context: the context is the call's"""
    out = {}
    for i in items:
        out.setdefault(i["adata"], []).append(i)
    return sorted(out.items(), key=lambda kv: (kv[0] is not None, kv[0]))


def sign(cv, alg, sks, pubs, adata, msgs, lengths=None):
    """one ec_eddsa_sign_msg_batch call: ([(status, signature)], [pub_out])"""
    kl = E.klen(alg)
    stride = E.stride_for(max(len(m) for m in msgs))
    sl = [E.slot(m, stride) for m in msgs]
    for j, ln in (lengths or {}).items():
        sl[j] = E.slot(msgs[j], stride, length=ln)
    sigs, pub, st = cv.eddsa_sign_msgs(alg, b"".join(sks), b"".join(pubs) if pubs else None, adata, b"".join(sl), stride)
    n = len(sks)
    return [(st[j], sigs[2 * kl * j:2 * kl * (j + 1)]) for j in range(n)], [pub[kl * j:kl * (j + 1)] for j in range(n)]


def assert_all_verify(cv, alg, adata, pubs, msgs, got):
    """every signature the device produced is accepted by ec_eddsa_verify_batch under a host-computed hram"""
    kl = E.klen(alg)
    assert all(st == 0 for st, _ in got)
    hram = b"".join(E.hram(alg, adata or b"", s[:kl], p, m) for (_, s), p, m in zip(got, pubs, msgs))
    assert cv.eddsa_verify(b"".join(pubs), b"".join(s for _, s in got), hram) == bytes(len(got))


def rfc_vectors():
    """[(alg, adata, [(sk, pub, msg, sig)])] from the three files of known answers"""
    with open(os.path.join(O.GOLDEN, "rfc_vectors.json")) as f:
        v = json.load(f)["ed25519"]
    out = {(E.EDDSA25519, b""): [tuple(bytes.fromhex(x[k]) for k in ("secret_key", "public_key", "message", "signature")) for x in v]}
    for name in ("eddsa_kats.json", "eddsa448_kats.json"):
        with open(os.path.join(O.GOLDEN, name)) as f:
            for x in json.load(f):
                key = (E.ALGS[x["sig_type"]], bytes.fromhex(x["adata"]))
                out.setdefault(key, []).append(tuple(bytes.fromhex(x[k]) for k in ("priv_key", "pub_key", "msg", "exp_sig")))
    return [(alg, ad, vs) for (alg, ad), vs in sorted(out.items())]


@pytest.mark.parametrize("derive", [False, True])
def test_rfc8032_vectors(ctx, derive):
    vecs = rfc_vectors()
    assert {alg for alg, _, _ in vecs} == set(ALGS) and sum(len(v) for _, _, v in vecs) >= 16
    cvs = {c: ctx.curve(c) for c in ("WEI25519", "WEI448")}
    for alg, ad, vs in vecs:
        cv = cvs[E.curve_of(alg)]
        sks, pubs, msgs, sigs = ([v[k] for v in vs] for k in range(4))
        got, pub_out = sign(cv, alg, sks, None if derive else pubs, ad, msgs)
        assert got == [(0, s) for s in sigs], (alg, ad, derive)
        assert pub_out == pubs, (alg, derive)
    for cv in cvs.values():
        cv.free()


@pytest.mark.parametrize("alg", ALGS)
def test_fixture_host_pointers(ctx, fx, alg):
    cv = ctx.curve(E.curve_of(alg))
    for adata, items in groups([i for i in fx if i["alg"] == alg and i["ret"] == 0]):
        ad = bytes.fromhex(adata) if adata is not None else None
        sks, pubs, msgs = ([bytes.fromhex(i[k]) for i in items] for k in ("sk", "pub", "msg"))
        want = [(0, bytes.fromhex(i["sig"])) for i in items]
        for derive in (False, True):
            got, pub_out = sign(cv, alg, sks, None if derive else pubs, ad, msgs)
            assert got == want, (alg, adata, derive)
            assert pub_out == pubs, (alg, adata, derive)
        assert_all_verify(cv, alg, ad, pubs, msgs, got)
    cv.free()


@pytest.mark.parametrize("alg", ALGS)
def test_fixture_device_pointers(ctx, fx, alg):
    import torch
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    cv = ctx.curve(E.curve_of(alg))
    kl = E.klen(alg)
    stream = torch.cuda.current_stream().cuda_stream
    for adata, items in groups([i for i in fx if i["alg"] == alg and i["ret"] == 0]):
        ad = bytes.fromhex(adata) if adata is not None else None
        n = len(items)
        sks, pubs, msgs = ([bytes.fromhex(i[k]) for i in items] for k in ("sk", "pub", "msg"))
        stride = E.stride_for(max(len(m) for m in msgs))
        d_sk, d_pub, d_slots = t(b"".join(sks)), t(b"".join(pubs)), t(b"".join(E.slot(m, stride) for m in msgs))
        for derive in (False, True):
            d_sig = torch.full((n * 2 * kl,), 0xEE, dtype=torch.uint8, device=dev)
            d_po = torch.full((n * kl,), 0xEE, dtype=torch.uint8, device=dev)
            d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            cv.eddsa_sign_msgs_dev(alg, n, d_sk.data_ptr(), None if derive else d_pub.data_ptr(), ad, d_slots.data_ptr(), stride,
                                   d_sig.data_ptr(), d_po.data_ptr(), d_st.data_ptr(), stream)
            torch.cuda.synchronize()
            assert bytes(d_st.cpu().numpy()) == bytes(n), (alg, adata, derive)
            assert bytes(d_sig.cpu().numpy()) == b"".join(bytes.fromhex(i["sig"]) for i in items), (alg, adata, derive)
            assert bytes(d_po.cpu().numpy()) == b"".join(pubs), (alg, adata, derive)
        # without pub_out, and the keys alone
        d_sig = torch.full((n * 2 * kl,), 0xEE, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        cv.eddsa_sign_msgs_dev(alg, n, d_sk.data_ptr(), None, ad, d_slots.data_ptr(), stride, d_sig.data_ptr(), None, d_st.data_ptr(), stream)
        d_po = torch.full((n * kl,), 0xEE, dtype=torch.uint8, device=dev)
        d_st2 = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        cv.eddsa_pub_keys_dev(n, d_sk.data_ptr(), d_po.data_ptr(), d_st2.data_ptr(), stream)
        torch.cuda.synchronize()
        assert bytes(d_sig.cpu().numpy()) == b"".join(bytes.fromhex(i["sig"]) for i in items) and bytes(d_st.cpu().numpy()) == bytes(n)
        assert bytes(d_po.cpu().numpy()) == b"".join(pubs) and bytes(d_st2.cpu().numpy()) == bytes(n)
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


@pytest.mark.parametrize("alg", ALGS)
def test_split_path_gives_the_same_bytes(ctx, fx, alg):
    """ec_eddsa_sign_R_batch + ec_eddsa_sign_S_batch around host hashes, on the same items"""
    cv = ctx.curve(E.curve_of(alg))
    kl = E.klen(alg)
    for adata, items in groups([i for i in fx if i["alg"] == alg and i["ret"] == 0])[:2]:
        ad = bytes.fromhex(adata) if adata is not None else None
        sks, pubs, msgs = ([bytes.fromhex(i[k]) for i in items] for k in ("sk", "pub", "msg"))
        rh = b"".join(E.r_hash(alg, sk, ad or b"", m) for sk, m in zip(sks, msgs))
        Renc, st = cv.eddsa_sign_R(rh)
        assert st == bytes(len(items))
        Rs = [Renc[kl * j:kl * (j + 1)] for j in range(len(items))]
        hr = b"".join(E.hram(alg, ad or b"", r, p, m) for r, p, m in zip(Rs, pubs, msgs))
        S = cv.eddsa_sign_S(rh, hr, b"".join(E.expand(alg, sk)[0] for sk in sks))
        got, _ = sign(cv, alg, sks, None, ad, msgs)
        assert [s for _, s in got] == [Rs[j] + S[kl * j:kl * (j + 1)] for j in range(len(items))], (alg, adata)
    cv.free()


@pytest.fixture(scope="module")
def mixed_waves():
    """n = 197 (three full waves and a partial one) for EDDSA25519CTX and EDDSA448 under a three-octet context: message lengths 10, 100
    and 300 in turn, so that the lanes of every wave absorb one, two and three or more blocks side by side; the restatements' answers,
    computed once"""
    out = {}
    for alg in (E.EDDSA25519CTX, E.EDDSA448):
        rng = np.random.default_rng(197 + alg)
        kl, ad = E.klen(alg), b"ctx"
        sks = [rng.integers(0, 256, size=kl, dtype=np.uint8).tobytes() for _ in range(197)]
        msgs = [rng.integers(0, 256, size=(10, 100, 300)[j % 3], dtype=np.uint8).tobytes() for j in range(197)]
        block = 136 if E.is448(alg) else 128
        tail = 1 if E.is448(alg) else 17
        for w in range(0, 197, 64):
            assert {min((len(E.dom(alg, ad)) + kl + len(m) + tail + block - 1) // block, 3) for m in msgs[w:w + 64]} == {1, 2, 3}
        res = [E.py_sign(alg, sk, ad, m) for sk, m in zip(sks, msgs)]
        out[alg] = (ad, sks, msgs, [r[0] for r in res], [(0, r[1]) for r in res])
    return out


@pytest.mark.parametrize("alg", [E.EDDSA25519CTX, E.EDDSA448])
def test_chunks_and_waves(ctx, mixed_waves, alg):
    ad, sks, msgs, pubs, want = mixed_waves[alg]
    cv = ctx.curve(E.curve_of(alg))
    try:
        for chunk in (64, 1 << 20):
            ctx.set_max_chunk(chunk)
            for derive in (True, False):
                got, pub_out = sign(cv, alg, sks, None if derive else pubs, ad, msgs)
                assert got == want and pub_out == pubs, (alg, chunk, derive)
            pk, st = cv.eddsa_pub_keys(b"".join(sks))
            assert pk == b"".join(pubs) and st == bytes(197), (alg, chunk)
    finally:
        ctx.set_max_chunk(1 << 20)
    for n in (1, 63, 64, 65):
        got, pub_out = sign(cv, alg, sks[:n], None, ad, msgs[:n])
        assert got == want[:n] and pub_out == pubs[:n], (alg, n)
    assert_all_verify(cv, alg, ad, pubs, msgs, want)
    cv.free()


@pytest.mark.parametrize("alg", [E.EDDSA25519CTX, E.EDDSA448])
def test_secret_scalar_mode_gives_the_same_bytes(ctx, mixed_waves, alg):
    ad, sks, msgs, pubs, want = mixed_waves[alg]
    ctx.set_secret_scalars(True)
    try:
        cv = ctx.curve(E.curve_of(alg))
        got, pub_out = sign(cv, alg, sks, None, ad, msgs)
        assert got == want and pub_out == pubs
        cv.free()
    finally:
        ctx.set_secret_scalars(False)


@pytest.mark.parametrize("alg", ALGS)
def test_bad_slot_rejects_its_own_item_only(ctx, fx, alg):
    cv = ctx.curve(E.curve_of(alg))
    kl = E.klen(alg)
    adata, items = max(groups([i for i in fx if i["alg"] == alg and i["ret"] == 0]), key=lambda kv: len(kv[1]))
    ad = bytes.fromhex(adata) if adata is not None else None
    assert len(items) >= 6
    sks, pubs, msgs = ([bytes.fromhex(i[k]) for i in items] for k in ("sk", "pub", "msg"))
    stride = E.stride_for(max(len(m) for m in msgs))
    bad = {0: stride - 3, 3: 0xFFFFFFFF, len(items) - 1: stride}
    for derive in (True, False):
        got, pub_out = sign(cv, alg, sks, None if derive else pubs, ad, msgs, bad)
        for j, i in enumerate(items):
            assert got[j] == ((1, bytes(2 * kl)) if j in bad else (0, bytes.fromhex(i["sig"]))), (alg, derive, j)
        assert pub_out == pubs
    cv.free()


def test_public_keys_alone(ctx, fx):
    for curve, algs in (("WEI25519", (9, 10, 11)), ("WEI448", (12, 13))):
        cv = ctx.curve(curve)
        items = [i for i in fx if i["alg"] in algs]
        pk, st = cv.eddsa_pub_keys(b"".join(bytes.fromhex(i["sk"]) for i in items))
        assert pk == b"".join(bytes.fromhex(i["pub"]) for i in items) and st == bytes(len(items)), curve
        cv.free()


def test_call_level_arguments(ctx, fx):
    L = ctx.L
    ed, e4, p256 = ctx.curve("WEI25519"), ctx.curve("WEI448"), ctx.curve("SECP256R1")

    def call(cv, alg, n=1, sk=b"\1" * 57, pub=None, ad=b"c", alen=1, slots=b"\0" * 8, stride=8, sig=True, st=True, ctxh=None, dev=False):
        sg, pb, s = C.create_string_buffer(b"\x07" * 114, 114), C.create_string_buffer(b"\x07" * 57, 57), C.create_string_buffer(b"\x07", 1)
        args = [ctx.h if ctxh is None else ctxh[0], cv, alg, n, sk, pub, ad, alen, slots, stride, sg if sig else None, pb, s if st else None]
        if dev:
            assert n == 0                      # a refused call returns before a pointer is used; nothing to point at here
            r = L.ec_eddsa_sign_msg_batch_dev(args[0], cv, alg, 0, None, None, ad, alen, None, stride, None, None, None, None)
        else:
            r = L.ec_eddsa_sign_msg_batch(*args)
        return r, sg.raw, pb.raw, s.raw

    untouched = (b"\x07" * 114, b"\x07" * 57, b"\x07")
    # wrong alg / handle pairs
    for cv, alg in ((ed.h, 12), (ed.h, 13), (e4.h, 9), (e4.h, 10), (e4.h, 11), (ed.h, 8), (ed.h, 14), (ed.h, 0), (e4.h, -1), (p256.h, 9), (p256.h, 12)):
        r = call(cv, alg)
        assert r[0] == -1 and r[1:] == untouched and len(L.ecamd_last_error()) > 0, alg
        assert call(cv, alg, n=0, dev=True)[0] == -1
    # the context: 256 octets; EDDSA25519CTX without one (the reference refuses, as recorded); plain EDDSA25519 ignores both arguments
    assert [i["ret"] for i in fx if i["alg"] == 10 and i["family"] == "null_ctx"] == [-1]
    for cv, alg in ((ed.h, 10), (ed.h, 11), (e4.h, 12), (e4.h, 13)):
        r = call(cv, alg, ad=b"\0" * 256, alen=256)
        assert r[0] == -1 and r[1:] == untouched and b"adata_len" in L.ecamd_last_error()
    r = call(ed.h, 10, ad=None, alen=0)
    assert r[0] == -1 and r[1:] == untouched and b"EDDSA25519CTX" in L.ecamd_last_error()
    assert call(ed.h, 9, ad=None, alen=256)[0] == 0
    # strides, NULL arguments with n > 0, NULL and foreign handles
    for stride in (0, 6, 2, 4100, 4098):
        r = call(ed.h, 9, stride=stride)
        assert r[0] == -1 and r[1:] == untouched and b"msg_stride" in L.ecamd_last_error()
    for kw in ({"sk": None}, {"slots": None}, {"sig": False}, {"st": False}, {"ctxh": [None]}):
        r = call(ed.h, 9, **kw)
        assert r[0] == -1 and r[1][:64] == untouched[0][:64], kw
    assert call(None, 9)[0] == -1
    other = libecc_amd.Context(0)
    assert call(ed.h, 9, ctxh=[other.h])[0] == -1
    other.close()
    for n_args in ((ctx.h, ed.h, 1, None, C.create_string_buffer(32), C.create_string_buffer(1)), (ctx.h, ed.h, 1, b"\1" * 32, None, C.create_string_buffer(1)),
                   (ctx.h, None, 1, b"\1" * 32, C.create_string_buffer(32), C.create_string_buffer(1)), (ctx.h, p256.h, 1, b"\1" * 32, C.create_string_buffer(32), C.create_string_buffer(1))):
        assert L.ec_eddsa_pub_key_batch(*n_args) == -1
    # n = 0 touches nothing, NULL pointers welcome
    assert L.ec_eddsa_sign_msg_batch(ctx.h, ed.h, 9, 0, None, None, None, 0, None, 8, None, None, None) == 0
    assert L.ec_eddsa_sign_msg_batch_dev(ctx.h, e4.h, 13, 0, None, None, b"c", 1, None, 8, None, None, None, None) == 0
    assert L.ec_eddsa_pub_key_batch(ctx.h, ed.h, 0, None, None, None) == 0 and L.ec_eddsa_pub_key_batch_dev(ctx.h, e4.h, 0, None, None, None, None) == 0
    r = call(ed.h, 10, n=0)
    assert r[0] == 0 and r[1:] == untouched
    # and a good call after all that; the scratch wipes
    r = call(ed.h, 9, sk=b"\1" * 32)
    assert r[0] == 0 and r[3] == b"\0" and r[1][:64] == E.py_sign(9, b"\1" * 32, b"", b"")[1]
    assert L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    for cv in (ed, e4, p256):
        cv.free()
