"""GPU tests of the reference's own signature known answers (tests/golden/sig_kats.json: the published ISO/IEC 14888-3, TTA and
STB 34.101.45 examples of ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA, ECGDSA, BIGN and DBIGN) through every entry point that serves each
family, byte for byte.  They put the family kernels on curves no other family test names -- secp224r1, brainpoolP192r1 / P224r1 /
P384r1 / P512r1, frp256v1, bign384v1, bign512v1 -- and on ECKCDSA's truncation shapes (SHA-256 on a 224-bit order, SHA-512 on
secp256r1).  Per case:
  key          [x]G (ECKCDSA, ECGDSA: [1/x]G, inverted here) from ec_prj_pt_mul_batch is the recorded key
  signing      (x, k, msg) gives the published bytes with status 0, with and without secret-scalar mode:
                 ECKCDSA / ECSDSA / ECOSDSA   ec_sig_hashed_sign_batch, ec_sig_hashed_sign_ht_batch
                 ECFSDSA                      ec_schnorr_sign_batch, ec_schnorr_sign_ht_batch
                 ECGDSA                       ec_sig_sign_batch on the reference's digest, ec_sig_sign_msg_batch on the message
                 BIGN                         ec_bign_sign_batch on the message and on the reference's digest
                 DBIGN                        ec_dbign_sign_batch (the nonce derived on the device), ec_bign_sign_batch with the nonce
                                              solved from the published signature
  verification 130 items that cycle the case's variants (the honest triple, a bit flipped in either component, in the message, and
               another case's key): two waves and a ragged tail, in chunks of 64 and in one chunk, through the verifying twins of the
               calls above; the verdicts are the reference's recorded ones, zeros and ones both.
BASH is not among the hashes the BIGN / DBIGN entry points take (include/libecc_amd.h: 0, 1 .. 4 and belt-hash; anything else is a
call-level error).  For (BIGN384V1, BASH384) and (BIGN512V1, BASH512) the test asserts that refusal and takes the route of
tests/test_gpu_hash_table.py: ec_digest_slots_batch_dev into a device buffer, then ec_bign_sign_batch_dev, ec_dbign_sign_batch_dev
and ec_bign_verify_batch_dev with hash_type 0 on the same stream.
Whole-batch (multi-scalar) verification is not run here: a batch of repeated items is an exceptional case there by design."""
import ctypes as C

import pytest

import libecc_amd
import oracles as O
import sigkats_ref as K
import sigfam_ref as SF
import sighash_ref as SH
import schnorr_ref as S
import bign_ref as B
import hashtable_ref as T
import test_gpu_hash_table as TH
from test_gpu_schnorr_items import sslots, vslots

pytestmark = pytest.mark.gpu
hx = bytes.fromhex
N = 130
CASES = K.load_fixture()
IDS = [c["id"] for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def curves(ctx):
    """one handle per curve for the whole module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = ctx.curve(name)
        return made[name]

    yield get
    for cv in made.values():
        cv.free()


def on_device_digest_route(case):
    return case["hash"].startswith("BASH")


def device_out(n, fill=0xEE):
    import torch
    return torch.full((max(n, 1),), fill, dtype=torch.uint8, device=torch.device("cuda:0"))


def digests_on_device(ctx, hname, msgs, stream):
    """ec_digest_slots_batch_dev of the messages' slots, enqueued on `stream`: (the slots, the digests, the digest length).  The
    caller keeps BOTH buffers until it has synchronized, and allocates nothing in between: the library's work runs on a stream
    torch's allocator does not know, so a buffer dropped early could be handed out again and filled before the kernel has read it."""
    import torch
    stride = T.stride_for(msgs)
    d_slots = TH.to_dev(T.pack_slots(msgs, stride))
    hl = T.HASH_SIZES[hname]
    d_dg = torch.zeros(len(msgs) * hl, dtype=torch.uint8, device=d_slots.device)
    torch.cuda.synchronize()        # the fills above run on torch's stream
    ctx.digest_slots_dev(T.HASH_IDS[hname], len(msgs), d_slots.data_ptr(), stride, d_dg.data_ptr(), stream)
    return d_slots, d_dg, hl


def sign_everywhere(ctx, cv, case):
    """{entry point: (signature bytes, status bytes)} of the case's (x, k, msg)"""
    curve, alg, hname = case["curve"], case["alg"], case["hash"]
    num, ht = K.ALGS[alg], K.HASH_IDS[hname]
    x, k, msg, pub, dg = (hx(case[f]) for f in ("x", "k", "msg", "pub", "digest"))
    cl = O.clen(curve)
    if alg in K.HSIG:
        stride = SH.HSIZE[hname] if alg == "ECKCDSA" else SH.stride_for(num, cl, len(msg))
        inp = SH.device_input(curve, num, hname, pub, msg, stride)
        return {"ec_sig_hashed_sign_batch": cv.sig_hashed_sign(num, ht, x, k, inp, stride),
                "ec_sig_hashed_sign_ht_batch": cv.sig_hashed_sign_ht(num, ht, x, k, inp, stride)}
    if alg == "ECFSDSA":
        slots, stride = sslots(curve, num, hname, [msg])
        return {"ec_schnorr_sign_batch": cv.schnorr_sign(num, ht, x, None, k, slots, stride),
                "ec_schnorr_sign_ht_batch": cv.schnorr_sign_ht(num, ht, x, None, k, slots, stride)}
    if alg == "ECGDSA":
        stride = T.stride_for([msg])
        return {"ec_sig_sign_batch": cv.sig_sign(num, x, k, dg, len(dg)),
                "ec_sig_sign_msg_batch": cv.sig_sign_msg(num, ht, x, k, T.pack_slots([msg], stride), stride)}
    oid = K.oid_of(case)
    if not on_device_digest_route(case):
        assert alg == "BIGN" and hname == "BELT"
        stride = B.stride_for(len(msg))
        return {"ec_bign_sign_batch": cv.bign_sign(num, ht, x, k, B.device_input(hname, msg, stride), stride, oid),
                "ec_bign_sign_batch on the digest": cv.bign_sign(num, 0, x, k, dg, len(dg), oid)}
    import torch
    sl = cv.bign_siglen()
    tstream = torch.cuda.Stream(device=torch.device("cuda:0"))
    stream = tstream.cuda_stream
    d_x, d_k = TH.to_dev(x), TH.to_dev(k)
    out = {"ec_bign_sign_batch_dev": (device_out(sl), device_out(1))}
    if alg == "DBIGN":
        out["ec_dbign_sign_batch_dev"] = (device_out(sl), device_out(1))
    d_slots, d_dg, hl = digests_on_device(ctx, hname, [msg], stream)
    cv.bign_sign_dev(num, 0, 1, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, oid, out["ec_bign_sign_batch_dev"][0].data_ptr(),
                     out["ec_bign_sign_batch_dev"][1].data_ptr(), stream)
    if alg == "DBIGN":
        cv.dbign_sign_dev(0, 1, d_x.data_ptr(), d_dg.data_ptr(), hl, oid, b"", out["ec_dbign_sign_batch_dev"][0].data_ptr(),
                          out["ec_dbign_sign_batch_dev"][1].data_ptr(), stream)
    torch.cuda.synchronize()
    assert TH.from_dev(d_dg) == dg, (case["id"], "the digest computed on the device")
    return {name: (TH.from_dev(s), TH.from_dev(st)) for name, (s, st) in out.items()}


def verify_everywhere(ctx, cv, case, items):
    """{entry point: verdict bytes} of items = [variant]"""
    curve, alg, hname = case["curve"], case["alg"], case["hash"]
    num, ht = K.ALGS[alg], K.HASH_IDS[hname]
    pubs, sigs, msgs = ([hx(v[f]) for v in items] for f in ("pub", "sig", "msg"))
    allpub, allsig = b"".join(pubs), b"".join(sigs)
    cl = O.clen(curve)
    if alg in K.HSIG:
        stride = SH.HSIZE[hname] if alg == "ECKCDSA" else SH.stride_for(num, cl, max(len(m) for m in msgs))
        inp = b"".join(SH.device_input(curve, num, hname, p, m, stride) for p, m in zip(pubs, msgs))
        return {"ec_sig_hashed_verify_batch": cv.sig_hashed_verify(num, ht, allpub, allsig, inp, stride),
                "ec_sig_hashed_verify_ht_batch": cv.sig_hashed_verify_ht(num, ht, allpub, allsig, inp, stride)}
    if alg == "ECFSDSA":
        slots, stride = vslots(curve, num, hname, sigs, msgs)
        return {"ec_schnorr_verify_batch": cv.schnorr_verify(num, ht, allpub, S.AFF, allsig, slots, stride),
                "ec_schnorr_verify_ht_batch": cv.schnorr_verify_ht(num, ht, allpub, S.AFF, allsig, slots, stride)}
    if alg == "ECGDSA":
        stride = T.stride_for(msgs)
        dgs = b"".join(SF.H(hname, m) for m in msgs)
        return {"ec_sig_verify_batch": cv.sig_verify(num, allpub, allsig, dgs, K.HSIZE[hname]),
                "ec_sig_verify_msg_batch": cv.sig_verify_msg(num, ht, allpub, allsig, T.pack_slots(msgs, stride), stride)}
    oid = K.oid_of(case)
    if not on_device_digest_route(case):
        stride = B.stride_for(max(len(m) for m in msgs))
        return {"ec_bign_verify_batch": cv.bign_verify(num, ht, allpub, allsig, b"".join(B.slot(m, stride) for m in msgs), stride, oid),
                "ec_bign_verify_batch on the digest": cv.bign_verify(num, 0, allpub, allsig, b"".join(B.H(hname, m) for m in msgs), 32, oid)}
    import torch
    n = len(items)
    tstream = torch.cuda.Stream(device=torch.device("cuda:0"))
    stream = tstream.cuda_stream
    d_pub, d_sig, d_res = TH.to_dev(allpub), TH.to_dev(allsig), device_out(n, 7)
    d_slots, d_dg, hl = digests_on_device(ctx, hname, msgs, stream)
    cv.bign_verify_dev(num, 0, n, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, oid, d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    return {"ec_bign_verify_batch_dev": TH.from_dev(d_res)}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_key_derivation(curves, case):
    curve, alg = case["curve"], case["alg"]
    q, x = O.CURVES[curve]["q"], int(case["x"], 16)
    if alg in ("ECKCDSA", "ECGDSA"):
        x = pow(x, -1, q)
    assert curves(curve).scalar_mult(x.to_bytes(O.qlen(curve), "big")) == (hx(case["pub"]), b"\0"), case["id"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_signing_gives_the_published_bytes(ctx, curves, case):
    cv = curves(case["curve"])
    want = (hx(case["sig"]), b"\0")
    names = None
    try:
        for secret in (False, True):
            ctx.set_secret_scalars(secret)
            got = sign_everywhere(ctx, cv, case)
            # (BIGN with BASH has one call on its route: ec_bign_sign_batch_dev behind the device digest)
            assert len(got) == (1 if case["alg"] == "BIGN" and on_device_digest_route(case) else 2) and names in (None, sorted(got))
            names = sorted(got)
            for name, out in got.items():
                assert out == want, (case["id"], name, "secret scalars" if secret else "public scalars")
    finally:
        ctx.set_secret_scalars(False)
        assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_verdicts_of_130_items(ctx, curves, case):
    cv = curves(case["curve"])
    vs = case["variants"]
    items = [vs[i % len(vs)] for i in range(N)]
    want = bytes(0 if v["ret"] == 0 else 1 for v in items)
    assert 0 in want and 1 in want and want[-1] != want[0]
    try:
        for chunk in (64, 1 << 20):      # three chunks with a ragged last one; one chunk
            ctx.set_max_chunk(chunk)
            got = verify_everywhere(ctx, cv, case, items)
            assert len(got) == (1 if on_device_digest_route(case) else 2)
            for name, res in got.items():
                assert res == want, (case["id"], name, chunk, [i for i in range(N) if res[i:i + 1] != want[i:i + 1]][:8])
                assert 0 in res and 1 in res
    finally:
        ctx.set_max_chunk(1 << 20)


@pytest.mark.parametrize("case", [c for c in CASES if on_device_digest_route(c)], ids=[c["id"] for c in CASES if on_device_digest_route(c)])
def test_bash_is_refused_by_the_message_level_bign_calls(ctx, curves, case):
    """the documented contract that sends these cases through ec_digest_slots_batch_dev: -1, an error that names hash_type, and
    outputs left as they were"""
    cv = curves(case["curve"])
    L = ctx.L
    alg, ht = K.ALGS[case["alg"]], K.HASH_IDS[case["hash"]]
    assert ht in (19, 20) and L.ecamd_digest_len(ht) == K.HSIZE[case["hash"]]
    x, k, msg, pub, sig = (hx(case[f]) for f in ("x", "k", "msg", "pub", "sig"))
    oid = K.oid_of(case)
    stride = B.stride_for(len(msg))
    slot = B.slot(msg, stride)
    so, st, res = (C.create_string_buffer(b"\x55" * n, n) for n in (len(sig), 1, 1))
    assert L.ec_bign_sign_batch(ctx.h, cv.h, alg, ht, 1, x, k, slot, stride, oid, len(oid), so, st) == -1
    err = L.ecamd_last_error().decode()
    assert err.startswith("ec_bign_sign_batch:") and "hash_type" in err
    assert L.ec_bign_verify_batch(ctx.h, cv.h, alg, ht, 1, pub, sig, slot, stride, oid, len(oid), res) == -1
    err = L.ecamd_last_error().decode()
    assert err.startswith("ec_bign_verify_batch:") and "hash_type" in err
    assert L.ec_dbign_sign_batch(ctx.h, cv.h, ht, 1, x, slot, stride, oid, len(oid), b"", 0, so, st) == -1
    err = L.ecamd_last_error().decode()
    assert err.startswith("ec_dbign_sign_batch") and "hash_type" in err
    assert (so.raw, st.raw, res.raw) == (b"\x55" * len(sig), b"\x55", b"\x55")
