#!/usr/bin/env python3
"""Throughput of the protocol entry points with inputs resident in HBM (the *_dev forms):
BASELINE.json configs[3] (secp256r1 ECDSA batch verification) and configs[4] (Ed25519 verification,
X25519).  Same launch contract and JSON line as bench.py (one process per GPU under
torch.distributed.run, weak scaling, contiguous shards, one RCCL all-gather of the per-rank result
bytes per step); not the driver's headline bench.  --workload ecdsa_recover is the exception: one GPU, recovery beside the
verification of the same signatures in alternating windows (recover_row).  sig_hashed_verify / sig_hashed_sign / schnorr_verify /
schnorr_sign / bip0340_sign with --hash 5 .. 11, 13 .. 15, 17 .. 20 or --hashes LIST|new go through the _ht entry points (commit_ht_rows).

    python tools/bench_protocols.py --workload ecdsa_verify|ecdsa_recover|sig_verify|sig_sign [--alg ecgdsa|ecrdsa|sm2]|sig_msg_verify|sig_msg_sign|hash_slots [--alg sm2|ecrdsa|ecgdsa --hash 11|13|14|2 --curve C]|digest_msgs [--hash N --lens 32|1024|mixed]|eddsa_verify_msgs|eddsa_sign_msgs [--alg ed25519|.. --lens 32|1024|mixed]|digest_slots|hmac_slots [--hash 1..11|13..15|17..20]|bign_verify|bign_sign [--hash 0|16]|decdsa_sign [--hash 1..11|13..15|17..20 --curve C]|dbign_sign [--secret]|bip0340_sign [--secret]|eddsa_sign --alg ed25519|ed25519ctx|ed25519ph|ed448|ed448ph [--derive-pub]|ecdsa_sign|ecccdh|ed25519_verify|ed448_verify|x25519|x448|bip0340_msm|ed25519_msm [--gpus N --steps K --warmup W]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libecc_amd  # noqa: E402

SEED = 0x5EC9256


def recover_row(a, ctx, dev, stream, rng, B):
    """ECDSA public-key recovery (ec_ecdsa_recover_batch_dev), inputs resident in HBM, beside the ECDSA verification of the SAME
    signatures in the same run: the two are timed in alternating windows of a.steps calls, so what the pair prints is a ratio taken
    under one clock and one neighbourhood.  Gates: every recovered pair holds the signer's key (prime-order curves), every recovered
    signer key verifies, 256 random items identical to the unmodified reference where it is built.  One GPU only (no all-gather: the
    row is a ratio on one device); run it with --steps 10 or more, so that a window is a quarter of a second of work."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload ecdsa_recover measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import oracles as O
    curve = a.curve
    cv = ctx.curve(curve)
    q = O.CURVES[curve]["q"]
    ql, cl = O.qlen(curve), O.clen(curve)
    hl = 32
    raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

    def scal(rows):
        return b"".join(((int.from_bytes(rows[i].tobytes(), "big") % (q - 1)) + 1).to_bytes(ql, "big") for i in range(B))

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    privs, nonces = scal(raw[0]), scal(raw[1])
    dg = rng.integers(0, 256, size=hl * B, dtype=np.uint8).tobytes()
    pubs, st = cv.scalar_mult(privs)
    assert set(st) == {0}
    sigs, st = cv.ecdsa_sign(privs, nonces, dg, hl)
    assert set(st) == {0}
    d_pub, d_sig, d_dg = t(pubs), t(sigs), t(dg)
    d_res = torch.empty(B, dtype=torch.uint8, device=dev)
    d_k1, d_k2 = (torch.empty(2 * cl * B, dtype=torch.uint8, device=dev) for _ in range(2))
    d_s1, d_s2 = (torch.empty(B, dtype=torch.uint8, device=dev) for _ in range(2))

    def verify():
        cv.ecdsa_verify_dev(B, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)

    def recover():
        cv.ecdsa_recover_dev(B, d_sig.data_ptr(), d_dg.data_ptr(), hl, d_k1.data_ptr(), d_k2.data_ptr(), d_s1.data_ptr(), d_s2.data_ptr(),
                             stream.cuda_stream)
    # ---- gates ----
    verify()
    recover()
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: an honest signature was rejected")
    k1, k2 = d_k1.cpu().numpy().reshape(B, 2 * cl), d_k2.cpu().numpy().reshape(B, 2 * cl)
    s1, s2 = d_s1.cpu().numpy(), d_s2.cpu().numpy()
    pk = np.frombuffer(pubs, dtype=np.uint8).reshape(B, 2 * cl)
    first = (k1 == pk).all(axis=1)
    if O.CURVES[curve]["order"] == q and not ((first | (k2 == pk).all(axis=1)).all() and (s1 == 0).all() and (s2 == 0).all()):
        raise SystemExit("PARITY FAILURE: a signer's key is not among the two recovered keys")
    gate = "the signer's key among the two recovered keys for all 2^%d items (the first one %.1f %% of the time)" % (a.batch_log2, 100.0 * first.mean())
    if O.have_ref() and a.ref_items > 0:
        import recover_ref as RR
        idx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, 256), replace=False))]
        exp = RR.ref_recover_threaded(curve, b"".join(sigs[2 * ql * i:2 * ql * (i + 1)] for i in idx), b"".join(dg[hl * i:hl * (i + 1)] for i in idx), hl)
        got = (k1[idx].tobytes(), k2[idx].tobytes(), s1[idx].tobytes(), s2[idx].tobytes())
        if got != exp:
            raise SystemExit("PARITY FAILURE: GPU output differs from the unmodified reference binary")
        gate += "; 256 random items identical to the unmodified reference's ecdsa_public_key_from_sig"
    # ---- timing: alternating windows ----
    for _ in range(a.warmup):
        verify()
        recover()
    torch.cuda.synchronize()
    tv, tr = [], []
    for _ in range(3):
        for fn, acc in ((verify, tv), (recover, tr)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
    # ---- per-kernel time of ONE recovery call from the library's own events around its scalar-multiplication pipelines ----
    kern = None
    try:
        ctx.enable_kernel_timing(True)
        recover()
        torch.cuda.synchronize()
        kern = ctx.kernel_times()
        ctx.enable_kernel_timing(False)
    except Exception as e:
        kern = {"error": str(e)}
    mv, mr = float(np.median(tv)), float(np.median(tr))
    print(json.dumps({"metric": "ECDSA public keys recovered/sec (%s, batch=2^%d, device-resident)" % (curve.lower(), a.batch_log2),
                      "value": B / mr, "unit": "recoveries/s", "recover_ms": [1e3 * x for x in tr],
                      "ecdsa_verify_same_run": {"value": B / mv, "unit": "verifications/s", "verify_ms": [1e3 * x for x in tv]},
                      "recover_over_verify": mv / mr, "gate": gate, "last_smul_kernel_ms": kern,
                      "config": {"workload": "ecdsa_recover", "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


def sig_family_row(a, ctx, dev, stream, rng, B):
    """ECGDSA / ECRDSA / SM2 (ec_sig_verify_batch_dev or ec_sig_sign_batch_dev, --alg), inputs resident in HBM, beside the ECDSA
    call of the same kind on the same curve in the same run, in alternating windows of a.steps calls as recover_row does.  Gates:
    every signature the device made is accepted, and with the digests of the next item none is.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload sig_verify / sig_sign measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import oracles as O
    alg = {"ecgdsa": 6, "ecrdsa": 7, "sm2": 8}[a.alg]
    curve = a.curve
    cv = ctx.curve(curve)
    q = O.CURVES[curve]["q"]
    ql, cl = O.qlen(curve), O.clen(curve)
    hl = 32
    raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

    def scal(rows, below):
        return [(int.from_bytes(rows[i].tobytes(), "big") % below) + 1 for i in range(B)]

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    xs, ks = scal(raw[0], q - 2), scal(raw[1], q - 1)
    privs, nonces = (b"".join(v.to_bytes(ql, "big") for v in vs) for vs in (xs, ks))
    dg = rng.integers(0, 256, size=hl * B, dtype=np.uint8).tobytes()   # H(m); for SM2 they stand for H(Z || m)
    pubs_e, st = cv.scalar_mult(privs)
    assert set(st) == {0}
    pubs = cv.scalar_mult(b"".join(pow(x, -1, q).to_bytes(ql, "big") for x in xs))[0] if alg == 6 else pubs_e
    sigs_e, st = cv.ecdsa_sign(privs, nonces, dg, hl)
    assert set(st) == {0}
    sigs, st = cv.sig_sign(alg, privs, nonces, dg, hl)
    assert set(st) == {0}
    d_pub_e, d_sig_e, d_pub, d_sig, d_dg, d_x, d_k = (t(b) for b in (pubs_e, sigs_e, pubs, sigs, dg, privs, nonces))
    d_res = torch.empty(B, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.empty(2 * ql * B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    sign = a.workload == "sig_sign"

    def ecdsa():
        if sign:
            cv.ecdsa_sign_dev(B, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        else:
            cv.ecdsa_verify_dev(B, d_pub_e.data_ptr(), d_sig_e.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)

    def family():
        if sign:
            cv.sig_sign_dev(alg, B, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        else:
            cv.sig_verify_dev(alg, B, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)
    # ---- gates ----
    cv.sig_verify_dev(alg, B, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    d_rot = torch.roll(d_dg, hl)
    cv.sig_verify_dev(alg, B, d_pub.data_ptr(), d_sig.data_ptr(), d_rot.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != b"\1" * B:
        raise SystemExit("PARITY FAILURE: a signature was accepted for another item's digest")
    family()
    torch.cuda.synchronize()
    if sign and (bytes(d_out.cpu().numpy()) != sigs or bytes(d_st.cpu().numpy()) != bytes(B)):
        raise SystemExit("PARITY FAILURE: the device-pointer form signs differently")
    gate = "all 2^%d device-made signatures accepted, none for its neighbour's digest" % a.batch_log2
    # ---- timing: alternating windows ----
    for _ in range(a.warmup):
        ecdsa()
        family()
    torch.cuda.synchronize()
    te, tf = [], []
    for _ in range(3):
        for fn, acc in ((ecdsa, te), (family, tf)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
    me, mf = float(np.median(te)), float(np.median(tf))
    kind = "signatures" if sign else "verifications"
    print(json.dumps({"metric": "%s %s/sec (%s, batch=2^%d, device-resident)" % (a.alg.upper(), kind, curve.lower(), a.batch_log2),
                      "value": B / mf, "unit": kind + "/s", "family_ms": [1e3 * x for x in tf],
                      "ecdsa_same_run": {"value": B / me, "unit": kind + "/s", "ecdsa_ms": [1e3 * x for x in te]},
                      "family_over_ecdsa": me / mf, "gate": gate,
                      "config": {"workload": a.workload, "alg": a.alg, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


def digest_slots_row(a, ctx, dev, stream, rng, B):
    """--workload digest_slots: the bare slot hash over the whole table (ec_digest_slots_batch_dev, --hash 1 .. 11, 13 .. 15, 17 .. 20)
    beside SHA-256 of the same slots through the same call, in alternating windows of a.steps calls: ns per item at 32-octet messages,
    inputs resident in HBM.  Gate: the digests of the first 64 slots equal the host's (hashlib) where hashlib offers the hash.  One
    GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload digest_slots measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    ht = a.hash
    hl = libecc_amd.api.DIGEST_SIZES.get(ht)
    if hl is None:
        raise SystemExit("--workload digest_slots: --hash 1 .. 11, 13 .. 15 or 17 .. 20")
    mlen, stride = 32, 36
    sl = np.zeros((B, stride), dtype=np.uint8)
    sl[:, 0] = mlen
    sl[:, 4:] = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
    d_sl = torch.frombuffer(bytearray(sl.tobytes()), dtype=torch.uint8).to(dev)
    d_a, d_b = torch.empty(hl * B, dtype=torch.uint8, device=dev), torch.empty(32 * B, dtype=torch.uint8, device=dev)
    fns = [lambda: ctx.digest_slots_dev(ht, B, d_sl.data_ptr(), stride, d_a.data_ptr(), stream.cuda_stream),
           lambda: ctx.digest_slots_dev(2, B, d_sl.data_ptr(), stride, d_b.data_ptr(), stream.cuda_stream)]
    for _ in range(max(1, a.warmup)):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    names = {1: "sha224", 2: "sha256", 3: "sha384", 4: "sha512", 5: "sha3_224", 6: "sha3_256", 7: "sha3_384", 8: "sha3_512", 9: "sha512_224",
             10: "sha512_256", 11: "sm3", 15: "ripemd160"}
    gate = "not checked: hashlib does not offer this hash"
    if names.get(ht) in hashlib.algorithms_available:
        got = bytes(d_a[:64 * hl].cpu().numpy())
        if got != b"".join(hashlib.new(names[ht], sl[i, 4:].tobytes()).digest() for i in range(64)):
            raise SystemExit("PARITY FAILURE: the device's digests differ from hashlib's")
        gate = "the first 64 digests equal hashlib's"
    acc = [[], []]
    for _ in range(3):
        for fn, ac in zip(fns, acc):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ac.append((time.perf_counter() - t0) / a.steps)
    ma, mb = float(np.median(acc[0])), float(np.median(acc[1]))
    print(json.dumps({"metric": "hash_type %d of 2^%d slots of 32-octet messages, ns per item (device-resident)" % (ht, a.batch_log2),
                      "value": 1e9 * ma / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[0]],
                      "sha256_same_run": {"value": 1e9 * mb / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[1]]},
                      "gate": gate,
                      "config": {"workload": a.workload, "hash": ht, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    ctx.close()


def digest_msgs_lens(kind, B):
    """the message lengths of --workload digest_msgs.  "32" and "1024": every message that long.  "mixed": a fixed distribution from
    numpy's default_rng(20): 97 % of the messages uniform in 16 .. 256 octets, 2.9 % uniform in 257 .. 2048, 0.1 % uniform in 2049 .. 4092,
    and item 0 exactly 4092 octets, the longest a slot holds -- so the slot path runs at stride 4096 whatever the draw."""
    if kind != "mixed":
        return np.full(B, int(kind), dtype=np.int64)
    r = np.random.default_rng(20)
    u = r.random(B)
    lens = np.where(u < 0.97, r.integers(16, 257, size=B), np.where(u < 0.999, r.integers(257, 2049, size=B), r.integers(2049, 4093, size=B)))
    lens[0] = 4092
    return lens.astype(np.int64)


def eddsa_msgs_row(a, ctx, dev, stream, rng, B):
    """--workload eddsa_verify_msgs | eddsa_sign_msgs (--alg ed25519 .. ed448ph, --lens 32 | 1024 | mixed, digest_msgs_lens): EdDSA from
    the packed array, device-resident, beside its slot twin on the SAME content in alternating windows of a.steps calls.
      eddsa_sign_msgs    ec_eddsa_sign_msgs_batch_dev beside ec_eddsa_sign_msg_batch_dev (message slots resident in HBM)
      eddsa_verify_msgs  ec_eddsa_verify_msgs_batch_dev beside ec_eddsa_verify_msg_batch, the HOST form with host-assembled slots
                         dom2 || R || A || PH(M) (it has no device form, so its time includes the upload of the slots; Ed25519 only --
                         the Ed448 variants have no slot twin and run alone).  Every 10th signature is damaged.  `mixed` lengths are
                         clipped so that the assembled input fits a slot.
    Gates: the two paths give the same bytes for the whole batch; every signature made is accepted and every damaged one rejected.
    One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload %s measures one GPU: run it with --gpus 1, outside torch.distributed.run" % a.workload)
    if not a.alg.startswith("ed"):
        raise SystemExit("--workload %s: --alg ed25519 | ed25519ctx | ed25519ph | ed448 | ed448ph" % a.workload)
    import ctypes as C
    import eddsa_sign_ref as E
    alg = {"ed25519": E.EDDSA25519, "ed25519ctx": E.EDDSA25519CTX, "ed25519ph": E.EDDSA25519PH, "ed448": E.EDDSA448, "ed448ph": E.EDDSA448PH}[a.alg]
    verify = a.workload == "eddsa_verify_msgs"
    cv = ctx.curve(E.curve_of(alg))
    kl = E.klen(alg)
    ad = b"bench" if E.takes_ctx(alg) else None
    dom = E.dom(alg, ad or b"")
    lens = digest_msgs_lens(a.lens, B)
    twin = not (verify and E.is448(alg))
    if verify and not E.is_ph(alg):
        lens = np.minimum(lens, 4092 - len(dom) - 2 * kl)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[B])
    content = rng.integers(0, 256, size=(total + 3) & ~3, dtype=np.uint8)
    d_msgs, d_offs = torch.from_numpy(content).to(dev), torch.from_numpy(offs).to(dev)
    sp = stream.cuda_stream
    d_sk = torch.from_numpy(rng.integers(0, 256, size=B * kl, dtype=np.uint8)).to(dev)
    d_pub, d_st = torch.empty(B * kl, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    d_sig, d_sig2 = torch.empty(B * 2 * kl, dtype=torch.uint8, device=dev), torch.empty(B * 2 * kl, dtype=torch.uint8, device=dev)
    cv.eddsa_pub_keys_dev(B, d_sk.data_ptr(), d_pub.data_ptr(), d_st.data_ptr(), sp)
    cv.eddsa_sign_msg_list_dev(alg, B, d_sk.data_ptr(), d_pub.data_ptr(), ad, d_msgs.data_ptr(), total, d_offs.data_ptr(), d_sig.data_ptr(), None,
                               d_st.data_ptr(), sp)
    torch.cuda.synchronize()
    if int(d_st.max()) != 0:
        raise SystemExit("PARITY FAILURE: an item was not signed")
    if not verify:
        # the message slots of the same content, laid out on the device
        stride = (4 + int(lens.max()) + 3) & ~3
        d_lens = torch.from_numpy(lens).to(dev)
        d_sl = torch.zeros(B * stride, dtype=torch.uint8, device=dev)
        d_sl.view(B, stride)[:, :4] = torch.stack([(d_lens >> (8 * k)) & 255 for k in range(4)], dim=1).to(torch.uint8)
        item = torch.repeat_interleave(torch.arange(B, device=dev), d_lens)
        d_sl[item * stride + 4 + (torch.arange(total, device=dev) - d_offs[item])] = d_msgs[:total]
        del item
        fns = [lambda: cv.eddsa_sign_msg_list_dev(alg, B, d_sk.data_ptr(), d_pub.data_ptr(), ad, d_msgs.data_ptr(), total, d_offs.data_ptr(),
                                                  d_sig.data_ptr(), None, d_st.data_ptr(), sp),
               lambda: cv.eddsa_sign_msgs_dev(alg, B, d_sk.data_ptr(), d_pub.data_ptr(), ad, d_sl.data_ptr(), stride, d_sig2.data_ptr(), None,
                                              d_st.data_ptr(), sp)]
        twin_name, twin_octets = "ec_eddsa_sign_msg_batch_dev", B * stride
    else:
        bad = np.zeros(B, dtype=np.uint8)
        bad[::10] = 1
        d_sig.view(B, 2 * kl)[::10, kl] ^= 1          # a bit of S of every 10th signature
        expected = torch.from_numpy(bad).to(dev)
        d_res, d_res2 = torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
        fns = [lambda: cv.eddsa_verify_msg_list_dev(alg, B, d_pub.data_ptr(), d_sig.data_ptr(), ad, d_msgs.data_ptr(), total, d_offs.data_ptr(),
                                                    d_res.data_ptr(), sp)]
        twin_name, twin_octets, stride = None, 0, 0
        if twin:
            # dom2 || R || A || PH(M) per item, assembled on the host as a caller of ec_eddsa_verify_msg_batch has to
            pubs, sigs = d_pub.cpu().numpy().reshape(B, kl), d_sig.cpu().numpy().reshape(B, 2 * kl)
            tail = [E.PH(alg, content[offs[i]:offs[i + 1]].tobytes()) for i in range(B)] if E.is_ph(alg) else None
            tl = np.full(B, 64, dtype=np.int64) if E.is_ph(alg) else lens
            head = len(dom) + 2 * kl
            stride = (4 + head + int(tl.max()) + 3) & ~3
            slots = np.zeros((B, stride), dtype=np.uint8)
            slots[:, :4] = np.stack([((head + tl) >> (8 * k)) & 255 for k in range(4)], axis=1).astype(np.uint8)
            slots[:, 4:4 + len(dom)] = np.frombuffer(dom, dtype=np.uint8)
            slots[:, 4 + len(dom):4 + len(dom) + kl] = sigs[:, :kl]
            slots[:, 4 + len(dom) + kl:4 + head] = pubs
            for i in range(B):
                slots[i, 4 + head:4 + head + tl[i]] = np.frombuffer(tail[i], dtype=np.uint8) if tail else content[offs[i]:offs[i + 1]]
            pubs_b, sigs_b, slots_b = pubs.tobytes(), sigs.tobytes(), slots.ctypes.data_as(C.c_char_p)   # (slots stays alive: no second copy)
            res2 = C.create_string_buffer(B)

            def slot_call():
                if cv.L.ec_eddsa_verify_msg_batch(ctx.h, cv.h, B, pubs_b, sigs_b, slots_b, stride, res2) != 0:
                    raise SystemExit("ec_eddsa_verify_msg_batch failed")
            fns.append(slot_call)
            twin_name, twin_octets = "ec_eddsa_verify_msg_batch (host form, upload included)", B * (stride + 3 * kl)
    torch.cuda.synchronize()
    for _ in range(max(1, a.warmup)):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    if verify:
        if not torch.equal(d_res, expected):
            raise SystemExit("PARITY FAILURE: the verdicts are not: every 10th item rejected")
        if twin and res2.raw[:B] != bad.tobytes():
            raise SystemExit("PARITY FAILURE: the slot twin's verdicts differ")
        gate = "every 10th signature rejected, all others accepted" + (", by both paths" if twin else "")
    else:
        if not torch.equal(d_sig, d_sig2) or int(d_st.max()) != 0:
            raise SystemExit("PARITY FAILURE: the two paths give different signatures")
        d_res = torch.empty(B, dtype=torch.uint8, device=dev)
        cv.eddsa_verify_msg_list_dev(alg, B, d_pub.data_ptr(), d_sig.data_ptr(), ad, d_msgs.data_ptr(), total, d_offs.data_ptr(), d_res.data_ptr(), sp)
        torch.cuda.synchronize()
        if int(d_res.max()) != 0:
            raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
        gate = "both paths give the same 2^%d signatures; ec_eddsa_verify_msgs_batch_dev accepts all" % a.batch_log2
    acc = [[] for _ in fns]
    for _ in range(3):
        for fn, ac in zip(fns, acc):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ac.append((time.perf_counter() - t0) / a.steps)
    ma = float(np.median(acc[0]))
    row = {"metric": "%s %s of 2^%d messages (--lens %s) from the packed array, ns per item (device-resident)" % (a.alg, a.workload, a.batch_log2, a.lens),
           "value": 1e9 * ma / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[0]], "items_per_s": B / ma, "message_octets": total,
           "octets_uploaded": total + 8 * (B + 1) + B * 3 * kl, "gate": gate,
           "config": {"workload": a.workload, "alg": a.alg, "lens": a.lens, "steps": a.steps, "warmup": a.warmup, "windows": 3}}
    if len(fns) == 2:
        mb = float(np.median(acc[1]))
        row["slot_twin_same_run"] = {"call": twin_name, "value": 1e9 * mb / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[1]], "stride": stride,
                                     "octets_uploaded": twin_octets + (0 if verify else B * 2 * kl)}
        row["ratio_msgs_over_slots_time"] = ma / mb
    else:
        row["slot_twin_same_run"] = None
    print(json.dumps(row))
    ctx.close()


def digest_msgs_row(a, ctx, dev, stream, rng, B):
    """--workload digest_msgs: ec_digest_msgs_batch_dev (--hash 1 .. 11, 13 .. 15, 17 .. 20; --lens 32 | 1024 | mixed, digest_msgs_lens) over
    a packed array beside ec_digest_slots_batch_dev on the SAME content at the stride the longest message forces, in alternating windows
    of a.steps calls, inputs resident in HBM: ns per item, GB/s of message octets, and the octets each format uploads.  Gate: the two
    paths give the same digests for the whole batch, and the first 64 equal hashlib's where hashlib offers the hash.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload digest_msgs measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    ht = a.hash
    hl = libecc_amd.api.DIGEST_SIZES.get(ht)
    if hl is None:
        raise SystemExit("--workload digest_msgs: --hash 1 .. 11, 13 .. 15 or 17 .. 20")
    lens = digest_msgs_lens(a.lens, B)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[B])
    stride = (4 + int(lens.max()) + 3) & ~3
    content = rng.integers(0, 256, size=(total + 3) & ~3, dtype=np.uint8)
    d_msgs = torch.from_numpy(content).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    # the slots of the same content, laid out on the device: a u32 length, then the message
    d_lens = torch.from_numpy(lens).to(dev)
    d_sl = torch.zeros(B * stride, dtype=torch.uint8, device=dev)
    d_sl.view(B, stride)[:, :4] = torch.stack([(d_lens >> (8 * k)) & 255 for k in range(4)], dim=1).to(torch.uint8)
    item = torch.repeat_interleave(torch.arange(B, device=dev), d_lens)
    d_sl[item * stride + 4 + (torch.arange(total, device=dev) - d_offs[item])] = d_msgs[:total]
    del item
    d_a, d_b, d_st = torch.empty(hl * B, dtype=torch.uint8, device=dev), torch.empty(hl * B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    fns = [lambda: ctx.digest_msgs_dev(ht, B, d_msgs.data_ptr(), total, d_offs.data_ptr(), d_a.data_ptr(), d_st.data_ptr(), stream=stream.cuda_stream),
           lambda: ctx.digest_slots_dev(ht, B, d_sl.data_ptr(), stride, d_b.data_ptr(), stream.cuda_stream)]
    torch.cuda.synchronize()
    for _ in range(max(1, a.warmup)):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    if not torch.equal(d_a, d_b) or int(d_st.max()) != 0:
        raise SystemExit("PARITY FAILURE: ec_digest_msgs_batch_dev and ec_digest_slots_batch_dev differ on the same content")
    gate = "both paths give the same %d digests" % B
    names = {1: "sha224", 2: "sha256", 3: "sha384", 4: "sha512", 5: "sha3_224", 6: "sha3_256", 7: "sha3_384", 8: "sha3_512", 9: "sha512_224",
             10: "sha512_256", 11: "sm3", 15: "ripemd160"}
    if names.get(ht) in hashlib.algorithms_available:
        got = bytes(d_a[:64 * hl].cpu().numpy())
        if got != b"".join(hashlib.new(names[ht], content[offs[i]:offs[i + 1]].tobytes()).digest() for i in range(64)):
            raise SystemExit("PARITY FAILURE: the device's digests differ from hashlib's")
        gate += "; the first 64 equal hashlib's"
    acc = [[], []]
    for _ in range(3):
        for fn, ac in zip(fns, acc):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ac.append((time.perf_counter() - t0) / a.steps)
    ma, mb = float(np.median(acc[0])), float(np.median(acc[1]))
    print(json.dumps({"metric": "hash_type %d of 2^%d messages (--lens %s) from the packed array, ns per item (device-resident)" % (ht, a.batch_log2, a.lens),
                      "value": 1e9 * ma / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[0]], "gb_per_s_of_message_octets": total / ma / 1e9,
                      "octets_uploaded": total + 8 * (B + 1),
                      "digest_slots_same_run": {"value": 1e9 * mb / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[1]], "stride": stride,
                                                "gb_per_s_of_message_octets": total / mb / 1e9, "octets_uploaded": B * stride},
                      "ratio_msgs_over_slots_time": ma / mb, "message_octets": total, "gate": gate,
                      "config": {"workload": a.workload, "hash": ht, "lens": a.lens, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    ctx.close()


def hmac_slots_row(a, ctx, dev, stream, rng, B):
    """--workload hmac_slots: ec_hmac_slots_batch_dev (--hash 1 .. 11, 13 .. 15, 17 .. 20) of 32-octet keys and 32-octet messages beside
    the bare hash of the same message slots (ec_digest_slots_batch_dev of the same hash), between HIP events in alternating windows of
    a.steps calls: ns per item, inputs resident in HBM.  Gate: the first 64 MACs equal hmac.new's where hashlib offers the hash.  One
    GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload hmac_slots measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import hmac
    ht = a.hash
    hl = libecc_amd.api.DIGEST_SIZES.get(ht)
    if hl is None:
        raise SystemExit("--workload hmac_slots: --hash 1 .. 11, 13 .. 15 or 17 .. 20")
    stride = 36
    sls = []
    for _ in range(2):
        sl = np.zeros((B, stride), dtype=np.uint8)
        sl[:, 0] = 32
        sl[:, 4:] = rng.integers(0, 256, size=(B, 32), dtype=np.uint8)
        sls.append(sl)
    d_k, d_m = (torch.frombuffer(bytearray(sl.tobytes()), dtype=torch.uint8).to(dev) for sl in sls)
    d_a, d_b = torch.empty(hl * B, dtype=torch.uint8, device=dev), torch.empty(hl * B, dtype=torch.uint8, device=dev)
    fns = [lambda: ctx.hmac_slots_dev(ht, B, d_k.data_ptr(), stride, d_m.data_ptr(), stride, d_a.data_ptr(), stream.cuda_stream),
           lambda: ctx.digest_slots_dev(ht, B, d_m.data_ptr(), stride, d_b.data_ptr(), stream.cuda_stream)]
    for _ in range(max(1, a.warmup)):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    names = {1: "sha224", 2: "sha256", 3: "sha384", 4: "sha512", 5: "sha3_224", 6: "sha3_256", 7: "sha3_384", 8: "sha3_512", 9: "sha512_224",
             10: "sha512_256", 11: "sm3", 15: "ripemd160"}
    gate = "not checked: hashlib does not offer this hash"
    if names.get(ht) in hashlib.algorithms_available:
        got = bytes(d_a[:64 * hl].cpu().numpy())
        if got != b"".join(hmac.new(sls[0][i, 4:].tobytes(), sls[1][i, 4:].tobytes(), names[ht]).digest() for i in range(64)):
            raise SystemExit("PARITY FAILURE: the device's MACs differ from hmac.new's")
        gate = "the first 64 MACs equal hmac.new's"
    acc = [[], []]
    for _ in range(3):
        for fn, ac in zip(fns, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ac.append(e0.elapsed_time(e1) / 1e3 / a.steps)
    ma, mb = float(np.median(acc[0])), float(np.median(acc[1]))
    print(json.dumps({"metric": "HMAC with hash_type %d of 2^%d pairs of 32-octet keys and messages, ns per item (device-resident)" % (ht, a.batch_log2),
                      "value": 1e9 * ma / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[0]],
                      "bare_hash_same_run": {"value": 1e9 * mb / B, "unit": "ns/item", "ms": [1e3 * x for x in acc[1]]},
                      "gate": gate,
                      "config": {"workload": a.workload, "hash": ht, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    ctx.close()


def sig_msg_row(a, ctx, dev, stream, rng, B):
    """ECGDSA / ECRDSA / SM2 from messages (ec_sig_verify_msg_batch_dev / ec_sig_sign_msg_batch_dev, --alg, --hash 1 .. 4, 11, 13, 14) beside
    the digest-level twin (ec_sig_verify_batch_dev / ec_sig_sign_batch_dev) on the same keys in the same run, in alternating windows of
    a.steps calls; --workload hash_slots: the bare slot hash (ec_hash_slots_batch_dev) beside SHA-256 of the same slots, ns per item.
    32-octet messages, inputs resident in HBM.  The twin's digests are random octets of the hash's size: its cost does not depend on
    them.  Gates: every signature the message-level call made is accepted by the message-level verification, none with its
    neighbour's slot.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload %s measures one GPU: run it with --gpus 1, outside torch.distributed.run" % a.workload)
    import oracles as O
    ht = a.hash
    hl = libecc_amd.api.HASH_SLOT_SIZES.get(ht)
    if hl is None:
        raise SystemExit("--workload %s: --hash 1 .. 4, 11, 13 or 14" % a.workload)

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def windows(fns):
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        acc = [[] for _ in fns]
        for _ in range(3):
            for fn, ac in zip(fns, acc):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                ac.append((time.perf_counter() - t0) / a.steps)
        return acc

    mlen = 32
    if a.workload == "hash_slots":
        stride = 4 + mlen
        sl = np.zeros((B, stride), dtype=np.uint8)
        sl[:, 0] = mlen
        sl[:, 4:] = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
        d_sl = t(sl.tobytes())
        d_a, d_b = torch.empty(hl * B, dtype=torch.uint8, device=dev), torch.empty(32 * B, dtype=torch.uint8, device=dev)
        ta, tb = windows([lambda: ctx.hash_slots_dev(ht, B, d_sl.data_ptr(), stride, d_a.data_ptr(), stream.cuda_stream),
                          lambda: ctx.hash_slots_dev(2, B, d_sl.data_ptr(), stride, d_b.data_ptr(), stream.cuda_stream)])
        ma, mb = float(np.median(ta)), float(np.median(tb))
        print(json.dumps({"metric": "hash_type %d of 2^%d slots of 32-octet messages, ns per item (device-resident)" % (ht, a.batch_log2),
                          "value": 1e9 * ma / B, "unit": "ns/item", "ms": [1e3 * x for x in ta],
                          "sha256_same_run": {"value": 1e9 * mb / B, "unit": "ns/item", "ms": [1e3 * x for x in tb]},
                          "config": {"workload": a.workload, "hash": ht, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
        ctx.close()
        return
    alg = {"ecgdsa": 6, "ecrdsa": 7, "sm2": 8}[a.alg]
    ident = b"1234567812345678" if alg == 8 else None
    blank = hl if alg == 8 else 0
    curve = a.curve
    cv = ctx.curve(curve)
    q = O.CURVES[curve]["q"]
    ql = O.qlen(curve)
    raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

    def scal(rows, below):
        return [(int.from_bytes(rows[i].tobytes(), "big") % below) + 1 for i in range(B)]
    xs, ks = scal(raw[0], q - 2), scal(raw[1], q - 1)
    privs, nonces = (b"".join(v.to_bytes(ql, "big") for v in vs) for vs in (xs, ks))
    pubs, st = cv.scalar_mult(b"".join(pow(x, -1, q).to_bytes(ql, "big") for x in xs) if alg == 6 else privs)
    assert set(st) == {0}
    stride = 4 + blank + mlen
    sl = np.zeros((B, stride), dtype=np.uint8)
    sl[:, 0] = blank + mlen
    sl[:, 4 + blank:] = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
    slots = sl.tobytes()
    dg = rng.integers(0, 256, size=hl * B, dtype=np.uint8).tobytes()
    sigs_t, st = cv.sig_sign(alg, privs, nonces, dg, hl)
    assert set(st) == {0}
    sigs, st = cv.sig_sign_msg(alg, ht, privs, nonces, slots, stride, ident, pubs if alg == 8 else None)
    assert set(st) == {0}
    d_pub, d_sig, d_sig_t, d_dg, d_x, d_k, d_sl = (t(b) for b in (pubs, sigs, sigs_t, dg, privs, nonces, slots))
    d_res = torch.empty(B, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.empty(2 * ql * B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    sign = a.workload == "sig_msg_sign"
    p_pub = d_pub.data_ptr() if alg == 8 else None

    def twin():
        if sign:
            cv.sig_sign_dev(alg, B, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        else:
            cv.sig_verify_dev(alg, B, d_pub.data_ptr(), d_sig_t.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)

    def msg():
        if sign:
            cv.sig_sign_msg_dev(alg, ht, B, d_x.data_ptr(), p_pub, d_k.data_ptr(), d_sl.data_ptr(), stride, ident, d_out.data_ptr(), d_st.data_ptr(),
                                stream.cuda_stream)
        else:
            cv.sig_verify_msg_dev(alg, ht, B, d_pub.data_ptr(), d_sig.data_ptr(), d_sl.data_ptr(), stride, ident, d_res.data_ptr(), stream.cuda_stream)
    # ---- gates ----
    cv.sig_verify_msg_dev(alg, ht, B, d_pub.data_ptr(), d_sig.data_ptr(), d_sl.data_ptr(), stride, ident, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    d_rot = torch.roll(d_sl, stride)
    cv.sig_verify_msg_dev(alg, ht, B, d_pub.data_ptr(), d_sig.data_ptr(), d_rot.data_ptr(), stride, ident, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != b"\1" * B:
        raise SystemExit("PARITY FAILURE: a signature was accepted for another item's message")
    msg()
    torch.cuda.synchronize()
    if sign and (bytes(d_out.cpu().numpy()) != sigs or bytes(d_st.cpu().numpy()) != bytes(B)):
        raise SystemExit("PARITY FAILURE: the device-pointer form signs differently")
    tt, tm = windows([twin, msg])
    mt, mm = float(np.median(tt)), float(np.median(tm))
    kind = "signatures" if sign else "verifications"
    print(json.dumps({"metric": "%s %s/sec from 32-octet messages, hash_type %d (%s, batch=2^%d, device-resident)" % (a.alg.upper(), kind, ht, curve.lower(), a.batch_log2),
                      "value": B / mm, "unit": kind + "/s", "msg_ms": [1e3 * x for x in tm],
                      "digest_level_same_run": {"value": B / mt, "unit": kind + "/s", "ms": [1e3 * x for x in tt]},
                      "msg_over_digest_level": mt / mm,
                      "gate": "all 2^%d device-made signatures accepted, none for its neighbour's message" % a.batch_log2,
                      "config": {"workload": a.workload, "alg": a.alg, "hash": ht, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


def sig_hashed_row(a, ctx, dev, stream, rng, B):
    """ECSDSA / ECOSDSA / ECKCDSA (ec_sig_hashed_verify_batch_dev or ec_sig_hashed_sign_batch_dev, --alg, SHA-256, 24-byte messages),
    inputs resident in HBM, beside ec_ecdsa_verify_batch_dev and ec_ecdsa_recover_batch_dev (the same structure: comb, window loop,
    shared-inversion finish) on the same curve in the same run, in alternating windows of a.steps calls.  Gates: every signature
    the device made is accepted, and with the inputs of the next item none is.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload sig_hashed_verify / sig_hashed_sign measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import hashlib
    import oracles as O
    alg = {"eckcdsa": 2, "ecsdsa": 3, "ecosdsa": 4}[a.alg]
    curve = a.curve
    cv = ctx.curve(curve)
    q = O.CURVES[curve]["q"]
    ql, cl = O.qlen(curve), O.clen(curve)
    ht, hl, mlen = 2, 32, 24
    raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

    def scal(rows):
        return [(int.from_bytes(rows[i].tobytes(), "big") % (q - 1)) + 1 for i in range(B)]

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    xs, ks = scal(raw[0]), scal(raw[1])
    privs, nonces = (b"".join(v.to_bytes(ql, "big") for v in vs) for vs in (xs, ks))
    pubs_e, st = cv.scalar_mult(privs)
    assert set(st) == {0}
    pubs = cv.scalar_mult(b"".join(pow(x, -1, q).to_bytes(ql, "big") for x in xs))[0] if alg == 2 else pubs_e
    msgs = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
    if alg == 2:
        # h = H(z || m), z the first 64 octets of Yx || Yy (zero padded): hashed by the caller
        stride = hl
        inp = b"".join(hashlib.sha256((pubs[2 * cl * i:2 * cl * (i + 1)] + bytes(64))[:64] + msgs[i].tobytes()).digest() for i in range(B))
    else:
        bl = 2 * cl if alg == 3 else cl
        stride = (4 + bl + mlen + 3) & ~3
        slots = np.zeros((B, stride), dtype=np.uint8)
        slots[:, 0] = bl + mlen
        slots[:, 4 + bl:4 + bl + mlen] = msgs
        inp = slots.tobytes()
    dg = rng.integers(0, 256, size=hl * B, dtype=np.uint8).tobytes()
    sigs_e, st = cv.ecdsa_sign(privs, nonces, dg, hl)
    assert set(st) == {0}
    sigs, st = cv.sig_hashed_sign(alg, ht, privs, nonces, inp, stride)
    assert set(st) == {0}
    d_pub_e, d_sig_e, d_pub, d_sig, d_dg, d_in, d_x, d_k = (t(b) for b in (pubs_e, sigs_e, pubs, sigs, dg, inp, privs, nonces))
    d_res = torch.empty(B, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.empty(len(sigs), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    d_k1, d_k2 = (torch.empty(2 * cl * B, dtype=torch.uint8, device=dev) for _ in range(2))
    d_s1, d_s2 = (torch.empty(B, dtype=torch.uint8, device=dev) for _ in range(2))
    sign = a.workload == "sig_hashed_sign"

    def ecdsa():
        cv.ecdsa_verify_dev(B, d_pub_e.data_ptr(), d_sig_e.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)

    def recover():
        cv.ecdsa_recover_dev(B, d_sig_e.data_ptr(), d_dg.data_ptr(), hl, d_k1.data_ptr(), d_k2.data_ptr(), d_s1.data_ptr(), d_s2.data_ptr(),
                             stream.cuda_stream)

    def hashed():
        if sign:
            cv.sig_hashed_sign_dev(alg, ht, B, d_x.data_ptr(), d_k.data_ptr(), d_in.data_ptr(), stride, d_out.data_ptr(), d_st.data_ptr(),
                                   stream.cuda_stream)
        else:
            cv.sig_hashed_verify_dev(alg, ht, B, d_pub.data_ptr(), d_sig.data_ptr(), d_in.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)
    # ---- gates ----
    cv.sig_hashed_verify_dev(alg, ht, B, d_pub.data_ptr(), d_sig.data_ptr(), d_in.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    d_rot = torch.roll(d_in, stride)
    cv.sig_hashed_verify_dev(alg, ht, B, d_pub.data_ptr(), d_sig.data_ptr(), d_rot.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != b"\1" * B:
        raise SystemExit("PARITY FAILURE: a signature was accepted for another item's input")
    hashed()
    torch.cuda.synchronize()
    if sign and (bytes(d_out.cpu().numpy()) != sigs or bytes(d_st.cpu().numpy()) != bytes(B)):
        raise SystemExit("PARITY FAILURE: the device-pointer form signs differently")
    gate = "all 2^%d device-made signatures accepted, none for its neighbour's input" % a.batch_log2
    # ---- timing: alternating windows ----
    for _ in range(a.warmup):
        ecdsa()
        recover()
        hashed()
    torch.cuda.synchronize()
    te, tr, tf = [], [], []
    for _ in range(3):
        for fn, acc in ((ecdsa, te), (recover, tr), (hashed, tf)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
    me, mr, mf = float(np.median(te)), float(np.median(tr)), float(np.median(tf))
    kind = "signatures" if sign else "verifications"
    print(json.dumps({"metric": "%s %s/sec (%s, SHA-256, batch=2^%d, device-resident)" % (a.alg.upper(), kind, curve.lower(), a.batch_log2),
                      "value": B / mf, "unit": kind + "/s", "hashed_ms": [1e3 * x for x in tf],
                      "ecdsa_verify_same_run": {"value": B / me, "unit": "verifications/s", "ms": [1e3 * x for x in te]},
                      "ecdsa_recover_same_run": {"value": B / mr, "unit": "recoveries/s", "ms": [1e3 * x for x in tr]},
                      "hashed_over_recover": mr / mf, "gate": gate,
                      "config": {"workload": a.workload, "alg": a.alg, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


def schnorr_row(a, ctx, dev, stream, rng, B):
    """BIP0340 / ECFSDSA item by item (ec_schnorr_verify_batch_dev or ec_schnorr_sign_batch_dev, --alg, SHA-256, 24-byte messages),
    inputs resident in HBM, beside ec_ecdsa_verify_batch_dev and ECSDSA (ec_sig_hashed_verify_batch_dev / _sign_batch_dev: the same two
    multiplications, the same shared-inversion finish, the same hash) on the same curve in the same run, in alternating windows of
    a.steps calls.  Signing is timed with the key derived on the device (BIP0340: a second fixed-base multiplication) and with the key
    supplied.  Gates: every signature the device made is accepted, with the slots of the next item none is, and --ref-items random items
    (and as many damaged ones) get the unmodified reference's verdict.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload schnorr_verify / schnorr_sign measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import oracles as O
    import schnorr_ref as S
    alg = {"bip0340": S.BIP0340, "ecfsdsa": S.ECFSDSA}[a.alg]
    curve = a.curve
    cv = ctx.curve(curve)
    q = O.CURVES[curve]["q"]
    ql, cl = O.qlen(curve), O.clen(curve)
    ht, hl, mlen, hname = 2, 32, 24, "SHA256"
    rl = S.r_len(alg, cl)
    sl = rl + ql
    raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

    def scal(rows):
        return [(int.from_bytes(rows[i].tobytes(), "big") % (q - 1)) + 1 for i in range(B)]

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    privs, nonces = (b"".join(v.to_bytes(ql, "big") for v in vs) for vs in (scal(raw[0]), scal(raw[1])))
    pubs, st = cv.scalar_mult(privs)
    assert set(st) == {0}
    msgs = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
    fl = S.fixed_len(alg, hname, cl)
    stride = (4 + fl + mlen + 3) & ~3
    slots = np.zeros((B, stride), dtype=np.uint8)
    slots[:, 0:4] = np.frombuffer((fl + mlen).to_bytes(4, "little"), dtype=np.uint8)
    if alg == S.BIP0340:
        slots[:, 4:4 + 2 * hl] = np.frombuffer(S.tagged(hname, S.TAG_CHALLENGE), dtype=np.uint8)
    slots[:, 4 + fl:4 + fl + mlen] = msgs
    sigs, st = cv.schnorr_sign(alg, ht, privs, None, nonces, slots.tobytes(), stride)
    assert set(st) == {0}
    # verification takes the arrays of ec_schnorr_verify_msg_all_batch: the commitment field holds the signature's r
    r_off = 4 + S.fixed_len(alg, hname, cl) - 2 * cl
    vsl = slots.copy()
    vsl[:, r_off:r_off + rl] = np.frombuffer(sigs, dtype=np.uint8).reshape(B, sl)[:, :rl]
    # the yardsticks: ECDSA on random digests, ECSDSA on the same messages
    dg = rng.integers(0, 256, size=hl * B, dtype=np.uint8).tobytes()
    sigs_e, st = cv.ecdsa_sign(privs, nonces, dg, hl)
    assert set(st) == {0}
    hstride = (4 + 2 * cl + mlen + 3) & ~3
    hsl = np.zeros((B, hstride), dtype=np.uint8)
    hsl[:, 0] = 2 * cl + mlen
    hsl[:, 4 + 2 * cl:4 + 2 * cl + mlen] = msgs
    sigs_h, st = cv.sig_hashed_sign(3, ht, privs, nonces, hsl.tobytes(), hstride)
    assert set(st) == {0}
    d_pub, d_sig, d_in, d_vin, d_x, d_k, d_sig_e, d_dg, d_sig_h, d_hin = (t(b) for b in (pubs, sigs, slots.tobytes(), vsl.tobytes(), privs, nonces,
                                                                                           sigs_e, dg, sigs_h, hsl.tobytes()))
    d_res = torch.empty(B, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.empty(max(len(sigs), len(sigs_h)), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    sign = a.workload == "schnorr_sign"

    def ecdsa():
        cv.ecdsa_verify_dev(B, d_pub.data_ptr(), d_sig_e.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)

    def ecsdsa():
        if sign:
            cv.sig_hashed_sign_dev(3, ht, B, d_x.data_ptr(), d_k.data_ptr(), d_hin.data_ptr(), hstride, d_out.data_ptr(), d_st.data_ptr(),
                                   stream.cuda_stream)
        else:
            cv.sig_hashed_verify_dev(3, ht, B, d_pub.data_ptr(), d_sig_h.data_ptr(), d_hin.data_ptr(), hstride, d_res.data_ptr(), stream.cuda_stream)

    def schnorr(with_key=False):
        if sign:
            cv.schnorr_sign_dev(alg, ht, B, d_x.data_ptr(), d_pub.data_ptr() if with_key else None, d_k.data_ptr(), d_in.data_ptr(), stride,
                                d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        else:
            cv.schnorr_verify_dev(alg, ht, B, d_pub.data_ptr(), 0, d_sig.data_ptr(), d_vin.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)

    def schnorr_key():
        schnorr(True)
    # ---- gates ----
    cv.schnorr_verify_dev(alg, ht, B, d_pub.data_ptr(), 0, d_sig.data_ptr(), d_vin.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    d_rot = torch.roll(d_in, stride)   # the next item's message; the commitment field is the device's to fill
    cv.schnorr_verify_dev(alg, ht, B, d_pub.data_ptr(), 0, d_sig.data_ptr(), d_rot.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != b"\1" * B:
        raise SystemExit("PARITY FAILURE: a signature was accepted for another item's message")
    for wk in (False, True):
        schnorr(wk)
        torch.cuda.synchronize()
        if sign and (bytes(d_out.cpu().numpy())[:len(sigs)] != sigs or bytes(d_st.cpu().numpy()) != bytes(B)):
            raise SystemExit("PARITY FAILURE: the device-pointer form signs differently")
    gate = "all 2^%d device-made signatures accepted, none for its neighbour's message" % a.batch_log2
    if O.have_ref() and a.ref_items > 0:
        from concurrent.futures import ThreadPoolExecutor
        idx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, a.ref_items), replace=False))]

        def one(i):
            key, sig, msg = pubs[2 * cl * i:2 * cl * (i + 1)], sigs[sl * i:sl * (i + 1)], msgs[i].tobytes()
            bad = sig[:-1] + bytes([sig[-1] ^ 1])
            return S.ref_verify(curve, alg, hname, key, S.AFF, sig, msg), S.ref_verify(curve, alg, hname, key, S.AFF, bad, msg)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            got = list(ex.map(one, idx))
        if got != [(0, -1)] * len(idx):
            raise SystemExit("PARITY FAILURE: the reference disagrees on %d of %d sampled items" % (sum(g != (0, -1) for g in got), len(idx)))
        bs = np.frombuffer(sigs, dtype=np.uint8).reshape(B, sl).copy()
        bs[idx, sl - 1] ^= 1
        cv.schnorr_verify_dev(alg, ht, B, d_pub.data_ptr(), 0, t(bs.tobytes()).data_ptr(), d_vin.data_ptr(), stride, d_res.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        exp = np.zeros(B, dtype=np.uint8)
        exp[idx] = 1
        if bytes(d_res.cpu().numpy()) != exp.tobytes():
            raise SystemExit("PARITY FAILURE: damaged items are not the ones rejected")
        gate += "; %d items and their damaged twins as the reference decides" % len(idx)
    # ---- timing: alternating windows ----
    fns = [ecdsa, ecsdsa, schnorr] + ([schnorr_key] if sign else [])
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(3):
        for fn, acc in zip(fns, times):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
    med = [float(np.median(x)) for x in times]
    kind = "signatures" if sign else "verifications"
    row = {"metric": "%s %s/sec (%s, SHA-256, batch=2^%d, device-resident)" % (a.alg.upper(), kind, curve.lower(), a.batch_log2),
           "value": B / med[2], "unit": kind + "/s", "schnorr_ms": [1e3 * x for x in times[2]],
           "ecdsa_verify_same_run": {"value": B / med[0], "unit": "verifications/s", "ms": [1e3 * x for x in times[0]]},
           "ecsdsa_same_run": {"value": B / med[1], "unit": kind + "/s", "ms": [1e3 * x for x in times[1]]},
           "schnorr_over_ecsdsa": med[1] / med[2], "gate": gate,
           "config": {"workload": a.workload, "alg": a.alg, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}
    if sign:
        row["key_supplied"] = {"value": B / med[3], "unit": "signatures/s", "ms": [1e3 * x for x in times[3]]}
    print(json.dumps(row))
    cv.free()
    ctx.close()


def bign_row(a, ctx, dev, stream, rng, B):
    """BIGN (ec_bign_verify_batch_dev or ec_bign_sign_batch_dev, 24-byte messages), inputs resident in HBM, beside ECKCDSA
    (ec_sig_hashed_verify_batch_dev / _sign_batch_dev, SHA-256: the same two multiplications, the same shared-inversion finish, one
    short hash of the commitment) under the same private keys on the same curve in the same run, in alternating windows of a.steps
    calls.  --hash 0: the caller hashed (SHA-256 on the host, the digests resident); --hash 16: message slots, belt-hash on the
    device.  Gates: every signature the device made is accepted, with the inputs of the next item none is, the device-pointer form
    signs what the host-pointer form signed, and --ref-items random items (and as many damaged ones) get the unmodified reference's
    verdict where it is built.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload bign_verify / bign_sign measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import oracles as O
    import bign_ref as BR
    from libecc_amd import api as A
    curve = a.curve
    cv = ctx.curve(curve)
    q = O.CURVES[curve]["q"]
    ql, cl = O.qlen(curve), O.clen(curve)
    hl, mlen = 32, 24
    sl = cv.bign_siglen()
    raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

    def scal(rows):
        return [(int.from_bytes(rows[i].tobytes(), "big") % (q - 1)) + 1 for i in range(B)]

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    xs, ks = scal(raw[0]), scal(raw[1])
    privs, nonces = (b"".join(v.to_bytes(ql, "big") for v in vs) for vs in (xs, ks))
    pubs, st = cv.scalar_mult(privs)
    assert set(st) == {0}
    pubs_k = cv.scalar_mult(b"".join(pow(x, -1, q).to_bytes(ql, "big") for x in xs))[0]     # ECKCDSA's key is [1 / x]G
    msgs = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
    if a.hash == 0:
        hname, oid, stride = "SHA256", bytes.fromhex("0609608648016503040201"), hl
        inp = b"".join(hashlib.sha256(msgs[i].tobytes()).digest() for i in range(B))
    else:
        hname, oid, stride = "BELT", BR.OID_BELT, BR.stride_for(mlen)
        slots = np.zeros((B, stride), dtype=np.uint8)
        slots[:, 0] = mlen
        slots[:, 4:4 + mlen] = msgs
        inp = slots.tobytes()
    # the yardstick's input: h = H(z || m), z the first 64 octets of Yx || Yy (zero padded), hashed by the caller
    inp_k = b"".join(hashlib.sha256((pubs_k[2 * cl * i:2 * cl * (i + 1)] + bytes(64))[:64] + msgs[i].tobytes()).digest() for i in range(B))
    sigs, st = cv.bign_sign(A.SIG_BIGN, a.hash, privs, nonces, inp, stride, oid)
    assert set(st) == {0}
    sigs_k, st = cv.sig_hashed_sign(2, 2, privs, nonces, inp_k, hl)
    assert set(st) == {0}
    d_pub, d_sig, d_in, d_pub_k, d_sig_k, d_in_k, d_x, d_k = (t(b) for b in (pubs, sigs, inp, pubs_k, sigs_k, inp_k, privs, nonces))
    d_res = torch.empty(B, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.empty(max(len(sigs), len(sigs_k)), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    sign = a.workload == "bign_sign"

    def bverify(d_s, d_i):
        cv.bign_verify_dev(A.SIG_BIGN, a.hash, B, d_pub.data_ptr(), d_s.data_ptr(), d_i.data_ptr(), stride, oid, d_res.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        return bytes(d_res.cpu().numpy())

    def eckcdsa():
        if sign:
            cv.sig_hashed_sign_dev(2, 2, B, d_x.data_ptr(), d_k.data_ptr(), d_in_k.data_ptr(), hl, d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        else:
            cv.sig_hashed_verify_dev(2, 2, B, d_pub_k.data_ptr(), d_sig_k.data_ptr(), d_in_k.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)

    def bign():
        if sign:
            cv.bign_sign_dev(A.SIG_BIGN, a.hash, B, d_x.data_ptr(), d_k.data_ptr(), d_in.data_ptr(), stride, oid, d_out.data_ptr(), d_st.data_ptr(),
                             stream.cuda_stream)
        else:
            cv.bign_verify_dev(A.SIG_BIGN, a.hash, B, d_pub.data_ptr(), d_sig.data_ptr(), d_in.data_ptr(), stride, oid, d_res.data_ptr(), stream.cuda_stream)
    # ---- gates ----
    if bverify(d_sig, d_in) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    if bverify(d_sig, torch.roll(d_in, stride)) != b"\1" * B:
        raise SystemExit("PARITY FAILURE: a signature was accepted for another item's input")
    cv.sig_hashed_verify_dev(2, 2, B, d_pub_k.data_ptr(), d_sig_k.data_ptr(), d_in_k.data_ptr(), hl, d_res.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: the yardstick's own signature was rejected")
    bign()
    torch.cuda.synchronize()
    if sign and (bytes(d_out.cpu().numpy())[:len(sigs)] != sigs or bytes(d_st.cpu().numpy()) != bytes(B)):
        raise SystemExit("PARITY FAILURE: the device-pointer form signs differently")
    gate = "all 2^%d device-made signatures accepted, none for its neighbour's input" % a.batch_log2
    if O.have_ref() and a.ref_items > 0:
        from concurrent.futures import ThreadPoolExecutor
        idx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, a.ref_items), replace=False))]

        def one(i):
            key, sig, msg = pubs[2 * cl * i:2 * cl * (i + 1)], sigs[sl * i:sl * (i + 1)], msgs[i].tobytes()
            bad = sig[:-1] + bytes([sig[-1] ^ 1])
            return BR.ref_verify(curve, hname, oid, key, sig, msg), BR.ref_verify(curve, hname, oid, key, bad, msg)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            got = list(ex.map(one, idx))
        if got != [(0, -1)] * len(idx):
            raise SystemExit("PARITY FAILURE: the reference disagrees on %d of %d sampled items" % (sum(g != (0, -1) for g in got), len(idx)))
        bs = np.frombuffer(sigs, dtype=np.uint8).reshape(B, sl).copy()
        bs[idx, sl - 1] ^= 1
        exp = np.zeros(B, dtype=np.uint8)
        exp[idx] = 1
        if bverify(t(bs.tobytes()), d_in) != exp.tobytes():
            raise SystemExit("PARITY FAILURE: damaged items are not the ones rejected")
        gate += "; %d items and their damaged twins as the reference decides" % len(idx)
    # ---- timing: alternating windows ----
    for _ in range(a.warmup):
        eckcdsa()
        bign()
    torch.cuda.synchronize()
    te, tb = [], []
    for _ in range(3):
        for fn, acc in ((eckcdsa, te), (bign, tb)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
    me, mb = float(np.median(te)), float(np.median(tb))
    kind = "signatures" if sign else "verifications"
    how = "SHA-256 digests supplied" if a.hash == 0 else "belt-hash of the message on the device"
    print(json.dumps({"metric": "BIGN %s/sec (%s, %s, batch=2^%d, device-resident)" % (kind, curve.lower(), how, a.batch_log2),
                      "value": B / mb, "unit": kind + "/s", "bign_ms": [1e3 * x for x in tb],
                      "eckcdsa_same_run": {"value": B / me, "unit": kind + "/s", "ms": [1e3 * x for x in te]},
                      "bign_over_eckcdsa": me / mb, "gate": gate,
                      "config": {"workload": a.workload, "hash": a.hash, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


def decdsa_row(a, ctx, dev, stream, rng, B):
    """Deterministic ECDSA (ec_decdsa_sign_batch_dev on digests: the nonce of RFC 6979 derived on the device, then the signing core)
    beside ec_ecdsa_sign_batch_dev with SUPPLIED nonces on the same keys and digests, in the same run, in alternating windows of
    a.steps calls; and the nonce kernel by itself (ec_rfc6979_nonce_batch_dev) between HIP events.  --hash 1 .. 4: the SHA-2 of the
    digests and of the HMAC; any other number of ec_digest_slots_batch goes through ec_decdsa_sign_ht_batch_dev and
    ec_rfc6979_nonce_ht_batch_dev, and the row then also holds the bare hash of 32-octet message slots (ec_digest_slots_batch_dev of the
    same hash, one block per item) measured in the same windows: the yardstick for the nonce kernel's time per compression.
    Gates: the nonces the device derives are the Python restatement's on --ref-items random items (where hashlib has the hash), the
    signatures are those of the supplied-nonce call fed with them, and every signature is accepted.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload decdsa_sign measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import oracles as O
    import hmac_ht_ref as M
    curve = a.curve
    ht = a.hash >= 5
    hname = {i: name for name, i in M.HASH_IDS.items()}[a.hash]
    cv = ctx.curve(curve)
    q, ql, hl = O.CURVES[curve]["q"], O.qlen(curve), M.HASH_SIZES[hname]
    raw = rng.integers(0, 256, size=(B, ql + 8), dtype=np.uint8)
    privs = b"".join(((int.from_bytes(raw[i].tobytes(), "big") % (q - 1)) + 1).to_bytes(ql, "big") for i in range(B))
    dgs = rng.integers(0, 256, size=B * hl, dtype=np.uint8).tobytes()       # digests of messages nobody needs to know
    pubs, st = cv.scalar_mult(privs)
    assert set(st) == {0}

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_x, d_dg, d_pub = t(privs), t(dgs), t(pubs)
    d_k = torch.empty(B * ql, dtype=torch.uint8, device=dev)
    d_sig, d_sig2 = (torch.empty(B * 2 * ql, dtype=torch.uint8, device=dev) for _ in range(2))
    d_st, d_st2, d_res = (torch.empty(B, dtype=torch.uint8, device=dev) for _ in range(3))
    sp = stream.cuda_stream

    sl = np.zeros((B, 36), dtype=np.uint8)
    sl[:, 0] = 32
    sl[:, 4:] = rng.integers(0, 256, size=(B, 32), dtype=np.uint8)
    d_sl, d_bare = t(sl.tobytes()), torch.empty(B * hl, dtype=torch.uint8, device=dev)

    def nonces():
        (cv.rfc6979_nonce_ht_dev if ht else cv.rfc6979_nonce_dev)(a.hash, B, d_x.data_ptr(), d_dg.data_ptr(), d_k.data_ptr(), d_st.data_ptr(), sp)

    def decdsa():
        (cv.decdsa_sign_ht_dev if ht else cv.decdsa_sign_dev)(a.hash, B, d_x.data_ptr(), d_dg.data_ptr(), hl, True, d_sig.data_ptr(),
                                                              d_st.data_ptr(), sp)

    def bare():
        ctx.digest_slots_dev(a.hash, B, d_sl.data_ptr(), 36, d_bare.data_ptr(), sp)

    def supplied():
        cv.ecdsa_sign_dev(B, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, d_sig2.data_ptr(), d_st2.data_ptr(), sp)
    # ---- gates ----
    nonces()
    torch.cuda.synchronize()
    ks = bytes(d_k.cpu().numpy())
    if bytes(d_st.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a nonce was not derived")
    idx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, max(1, a.ref_items)), replace=False))]
    retries = 0
    if not M.have_hashlib(hname):
        idx = []
    for i in idx:
        k, r = M.py_nonce(curve, hname, privs[ql * i:ql * (i + 1)], dgs[hl * i:hl * (i + 1)])
        retries += r
        if k.to_bytes(ql, "big") != ks[ql * i:ql * (i + 1)]:
            raise SystemExit("PARITY FAILURE: item %d's nonce is not the restatement's" % i)
    decdsa()
    supplied()
    cv.ecdsa_verify_dev(B, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), sp)
    torch.cuda.synchronize()
    if bytes(d_sig.cpu().numpy()) != bytes(d_sig2.cpu().numpy()) or bytes(d_st.cpu().numpy()) != bytes(B) or bytes(d_st2.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: the deterministic call does not sign what the supplied-nonce call signs with its nonces")
    if bytes(d_res.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    gate = "%d nonces as the Python restatement derives them (%d rejected candidates among them); all 2^%d signatures equal those of the supplied-nonce call and accepted" % (len(idx), retries, a.batch_log2)
    # ---- timing: alternating windows; the nonce kernel between events ----
    for _ in range(a.warmup):
        supplied()
        decdsa()
        nonces()
        bare()
    torch.cuda.synchronize()
    ts, td, tn, tb = [], [], [], []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            bare()
        e1.record(stream)
        torch.cuda.synchronize()
        tb.append(e0.elapsed_time(e1) / 1e3 / a.steps)
        for fn, acc in ((supplied, ts), (decdsa, td)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            nonces()
        e1.record(stream)
        torch.cuda.synchronize()
        tn.append(e0.elapsed_time(e1) / 1e3 / a.steps)
    ms, md, mn = float(np.median(ts)), float(np.median(td)), float(np.median(tn))
    print(json.dumps({"metric": "deterministic ECDSA signatures/sec (%s, %s digests supplied, nonces derived on the device, batch=2^%d, device-resident)"
                                % (curve.lower(), hname, a.batch_log2),
                      "value": B / md, "unit": "signatures/s", "decdsa_ms": [1e3 * x for x in td],
                      "supplied_nonces_same_run": {"value": B / ms, "unit": "signatures/s", "ms": [1e3 * x for x in ts]},
                      "decdsa_over_supplied": ms / md,
                      "nonce_kernel": {"ms": [1e3 * x for x in tn], "ns_per_item": 1e9 * mn / B, "items_per_s": B / mn},
                      "bare_hash_one_block": {"ms": [1e3 * x for x in tb], "ns_per_item": 1e9 * float(np.median(tb)) / B},
                      "gate": gate,
                      "config": {"workload": a.workload, "hash": a.hash, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


def det_sign_row(a, ctx, dev, stream, rng, B):
    """DBIGN (--workload dbign_sign: ec_dbign_sign_batch_dev on 32-byte digests, bign256v1 unless --curve says otherwise) or BIP0340
    (--workload bip0340_sign: ec_bip0340_sign_batch_dev on 32-byte messages with SHA-256, Y derived on the device) with the nonce
    derived on the device, beside the supplied-nonce twin (ec_bign_sign_batch_dev / ec_schnorr_sign_batch_dev) on the same
    device-resident items, in the same run, in alternating windows of a.steps calls; and the generator by itself
    (ec_dbign_nonce_batch_dev / ec_bip0340_nonce_batch_dev; the latter includes Y = [x]G) between HIP events.  --secret: the context in
    secret-scalar mode (DBIGN's generator scans its substitution table).  Gates: the nonces are the Python restatement's on
    min(--ref-items, 256) random items, and all signatures equal those of the twin fed with the derived nonces.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload %s measures one GPU: run it with --gpus 1, outside torch.distributed.run" % a.workload)
    import oracles as O
    import bign_ref as BR
    import schnorr_ref as SR
    import det_sign_ref as D
    dbign = a.workload == "dbign_sign"
    curve = a.curve if a.curve != "SECP256R1" else ("BIGN256V1" if dbign else "SECP256K1")
    cv = ctx.curve(curve)
    ctx.set_secret_scalars(bool(a.secret))
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    raw = rng.integers(0, 256, size=(B, ql + 8), dtype=np.uint8)
    privs = b"".join(((int.from_bytes(raw[i].tobytes(), "big") % (q - 1)) + 1).to_bytes(ql, "big") for i in range(B))
    oid, tdata = BR.OID_BELT, D.T_SAMPLE

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    sp = stream.cuda_stream
    d_x = t(privs)
    d_k = torch.empty(B * ql, dtype=torch.uint8, device=dev)
    d_st, d_st2 = (torch.empty(B, dtype=torch.uint8, device=dev) for _ in range(2))
    if dbign:
        hl, sl = 32, BR.sig_len(curve)
        inp = rng.integers(0, 256, size=B * hl, dtype=np.uint8).tobytes()
        d_in = t(inp)

        def nonces():
            cv.dbign_nonce_dev(B, d_x.data_ptr(), d_in.data_ptr(), hl, oid, tdata, d_k.data_ptr(), d_st.data_ptr(), sp)

        def derived():
            cv.dbign_sign_dev(0, B, d_x.data_ptr(), d_in.data_ptr(), hl, oid, tdata, d_sig.data_ptr(), d_st.data_ptr(), sp)

        def supplied():
            cv.bign_sign_dev(BR.DBIGN, 0, B, d_x.data_ptr(), d_k.data_ptr(), d_in.data_ptr(), hl, oid, d_sig2.data_ptr(), d_st2.data_ptr(), sp)

        def restated(i):
            return D.dbign_nonce_from_digest(curve, privs[ql * i:ql * (i + 1)], inp[hl * i:hl * (i + 1)], oid, tdata)[1]
    else:
        hname, ht, ml, sl = "SHA256", 2, 32, cl + ql
        stride = D.bip_stride(curve, hname, ml)
        slots = np.zeros((B, stride), dtype=np.uint8)
        head = np.frombuffer(D.bip_slot(curve, hname, bytes(ml), stride), dtype=np.uint8)
        slots[:] = head
        msgs = rng.integers(0, 256, size=(B, ml), dtype=np.uint8)
        off = 4 + 2 * 32 + 2 * cl
        slots[:, off:off + ml] = msgs
        aux = rng.integers(0, 256, size=B * ql, dtype=np.uint8).tobytes()
        d_in, d_aux = t(slots.tobytes()), t(aux)

        def nonces():
            cv.bip0340_nonce_dev(ht, B, d_x.data_ptr(), None, d_aux.data_ptr(), d_in.data_ptr(), stride, d_k.data_ptr(), d_st.data_ptr(), sp)

        def derived():
            cv.bip0340_sign_dev(ht, B, d_x.data_ptr(), None, d_aux.data_ptr(), d_in.data_ptr(), stride, d_sig.data_ptr(), d_st.data_ptr(), sp)

        def supplied():
            cv.schnorr_sign_dev(SR.BIP0340, ht, B, d_x.data_ptr(), None, d_k.data_ptr(), d_in.data_ptr(), stride, d_sig2.data_ptr(), d_st2.data_ptr(), sp)

        def restated(i):
            return D.bip_nonce(curve, hname, int.from_bytes(privs[ql * i:ql * (i + 1)], "big"), int.from_bytes(aux[ql * i:ql * (i + 1)], "big"),
                               msgs[i].tobytes())[1]
    d_sig, d_sig2 = (torch.empty(B * sl, dtype=torch.uint8, device=dev) for _ in range(2))
    # ---- gates ----
    nonces()
    torch.cuda.synchronize()
    ks = bytes(d_k.cpu().numpy())
    if bytes(d_st.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a nonce was not derived")
    idx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, 256, max(1, a.ref_items)), replace=False))]
    for i in idx:
        if restated(i).to_bytes(ql, "big") != ks[ql * i:ql * (i + 1)]:
            raise SystemExit("PARITY FAILURE: item %d's nonce is not the restatement's" % i)
    derived()
    supplied()
    torch.cuda.synchronize()
    if bytes(d_sig.cpu().numpy()) != bytes(d_sig2.cpu().numpy()) or bytes(d_st.cpu().numpy()) != bytes(B) or bytes(d_st2.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: the one-call form does not sign what the supplied-nonce call signs with its nonces")
    gate = "%d nonces as the Python restatement derives them; all 2^%d signatures equal those of the supplied-nonce call" % (len(idx), a.batch_log2)
    # ---- timing: alternating windows; the generator between events ----
    for _ in range(a.warmup):
        supplied()
        derived()
        nonces()
    torch.cuda.synchronize()
    ts, td, tn = [], [], []
    for _ in range(3):
        for fn, acc in ((supplied, ts), (derived, td)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / a.steps)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            nonces()
        e1.record(stream)
        torch.cuda.synchronize()
        tn.append(e0.elapsed_time(e1) / 1e3 / a.steps)
    ms, md, mn = float(np.median(ts)), float(np.median(td)), float(np.median(tn))
    what = "DBIGN signatures/sec (%s, 32-byte digests supplied" % curve.lower() if dbign else "BIP0340 signatures/sec (%s, SHA-256, 32-byte messages, Y derived" % curve.lower()
    print(json.dumps({"metric": "%s, nonces derived on the device, %s mode, batch=2^%d, device-resident)"
                                % (what, "secret-scalar" if a.secret else "default", a.batch_log2),
                      "value": B / md, "unit": "signatures/s", "derived_ms": [1e3 * x for x in td],
                      "supplied_nonces_same_run": {"value": B / ms, "unit": "signatures/s", "ms": [1e3 * x for x in ts]},
                      "derived_over_supplied": ms / md,
                      "nonce_call": {"ms": [1e3 * x for x in tn], "ns_per_item": 1e9 * mn / B, "items_per_s": B / mn},
                      "gate": gate,
                      "config": {"workload": a.workload, "curve": curve, "secret": bool(a.secret), "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    ctx.set_secret_scalars(False)
    cv.free()
    ctx.close()


def eddsa_sign_row(a, ctx, dev, stream, rng, B):
    """One-call EdDSA signing (ec_eddsa_sign_msg_batch_dev: key expansion, PH(M), r_hash and hram hashed on the device) on 32-byte
    messages, device-resident, with the public keys supplied or (--derive-pub) derived on the device; beside it, in the same run and in
    alternating windows of a.steps calls, the existing split path on the same items -- ec_eddsa_sign_R_batch + ec_eddsa_sign_S_batch,
    which take HOST pointers (the split path has no device-pointer form), with r_hash, hram and the clamped scalars precomputed and
    not timed.  Gates: --ref-items (at most 512) random signatures are the Python restatement's, all signatures equal the split
    path's, and every signature is accepted by ec_eddsa_verify_batch.  One GPU only."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload eddsa_sign measures one GPU: run it with --gpus 1, outside torch.distributed.run")
    import eddsa_sign_ref as E
    alg = {"ed25519": E.EDDSA25519, "ed25519ctx": E.EDDSA25519CTX, "ed25519ph": E.EDDSA25519PH, "ed448": E.EDDSA448, "ed448ph": E.EDDSA448PH}[a.alg]
    cv = ctx.curve(E.curve_of(alg))
    kl, ml = E.klen(alg), 32
    hl = 2 * kl
    ad = b"bench" if E.takes_ctx(alg) else None
    stride = 4 + ml
    sks = rng.integers(0, 256, size=B * kl, dtype=np.uint8).tobytes()
    msgs = rng.integers(0, 256, size=B * ml, dtype=np.uint8).tobytes()
    slots = np.zeros((B, stride), dtype=np.uint8)
    slots[:, 0] = ml
    slots[:, 4:] = np.frombuffer(msgs, dtype=np.uint8).reshape(B, ml)

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_sk, d_slots = t(sks), t(slots.tobytes())
    d_sig = torch.empty(B * 2 * kl, dtype=torch.uint8, device=dev)
    d_pub = torch.empty(B * kl, dtype=torch.uint8, device=dev)
    d_st = torch.empty(B, dtype=torch.uint8, device=dev)
    sp = stream.cuda_stream
    cv.eddsa_pub_keys_dev(B, d_sk.data_ptr(), d_pub.data_ptr(), d_st.data_ptr(), sp)
    torch.cuda.synchronize()
    pubs = bytes(d_pub.cpu().numpy())
    if bytes(d_st.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: a public key was not derived")

    def one_call():
        cv.eddsa_sign_msgs_dev(alg, B, d_sk.data_ptr(), None if a.derive_pub else d_pub.data_ptr(), ad, d_slots.data_ptr(), stride,
                               d_sig.data_ptr(), None, d_st.data_ptr(), sp)
    # ---- the split path's inputs, on the host and not timed ----
    sk_l = [sks[kl * i:kl * (i + 1)] for i in range(B)]
    msg_l = [msgs[ml * i:ml * (i + 1)] for i in range(B)]
    exp = [E.expand(alg, k) for k in sk_l]
    a_sc = b"".join(e[0] for e in exp)
    dom = E.dom(alg, ad or b"")
    rh = b"".join(E.H(alg, dom + e[1] + E.PH(alg, m)) for e, m in zip(exp, msg_l))
    Renc, stR = cv.eddsa_sign_R(rh)
    hr = b"".join(E.H(alg, dom + Renc[kl * i:kl * (i + 1)] + pubs[kl * i:kl * (i + 1)] + E.PH(alg, msg_l[i])) for i in range(B))
    split_out = {}

    def split():
        split_out["R"], split_out["st"] = cv.eddsa_sign_R(rh)
        split_out["S"] = cv.eddsa_sign_S(rh, hr, a_sc)
    # ---- gates ----
    one_call()
    torch.cuda.synchronize()
    sig = bytes(d_sig.cpu().numpy())
    if bytes(d_st.cpu().numpy()) != bytes(B):
        raise SystemExit("PARITY FAILURE: an item was not signed")
    split()
    Rn, Sn = np.frombuffer(split_out["R"], dtype=np.uint8).reshape(B, kl), np.frombuffer(split_out["S"], dtype=np.uint8).reshape(B, kl)
    if np.concatenate([Rn, Sn], axis=1).tobytes() != sig or split_out["st"] != bytes(B):
        raise SystemExit("PARITY FAILURE: the one-call signatures are not the split path's")
    idx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, 512, max(1, a.ref_items)), replace=False))]
    for i in idx:
        A, s1 = E.py_sign(alg, sk_l[i], ad or b"", msg_l[i])
        if A != pubs[kl * i:kl * (i + 1)] or s1 != sig[2 * kl * i:2 * kl * (i + 1)]:
            raise SystemExit("PARITY FAILURE: item %d is not the restatement's" % i)
    if cv.eddsa_verify(pubs, sig, hr) != bytes(B):
        raise SystemExit("PARITY FAILURE: a signature the device made was rejected")
    gate = "%d signatures and public keys as the Python restatement gives them; all 2^%d signatures equal the split path's and accepted" % (len(idx), a.batch_log2)
    # ---- timing: alternating windows ----
    for _ in range(a.warmup):
        one_call()
        split()
    torch.cuda.synchronize()
    to, tsp = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            one_call()
        torch.cuda.synchronize()
        to.append((time.perf_counter() - t0) / a.steps)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            split()
        tsp.append((time.perf_counter() - t0) / a.steps)
    mo, msp = float(np.median(to)), float(np.median(tsp))
    print(json.dumps({"metric": "EdDSA signatures/sec (%s, one call, every hash on the device, public keys %s, 32-byte messages, batch=2^%d, device-resident)"
                                % (a.alg, "derived on the device" if a.derive_pub else "supplied", a.batch_log2),
                      "value": B / mo, "unit": "signatures/s", "one_call_ms": [1e3 * x for x in to],
                      "split_path_host_pointers_same_run": {"value": B / msp, "unit": "signatures/s", "ms": [1e3 * x for x in tsp],
                                                            "note": "ec_eddsa_sign_R_batch + ec_eddsa_sign_S_batch, hashes precomputed and not timed, host-to-device copies of 3 x hlen + klen bytes per item timed"},
                      "one_call_over_split": msp / mo,
                      "gate": gate,
                      "config": {"workload": a.workload, "alg": a.alg, "derive_pub": bool(a.derive_pub), "steps": a.steps, "warmup": a.warmup, "windows": 3}}))
    cv.free()
    ctx.close()


NEW_COMMIT_HASHES = [5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20]
HASH_BLOCKS = {1: 64, 2: 64, 3: 128, 4: 128, 5: 144, 6: 136, 7: 104, 8: 72, 9: 128, 10: 128, 11: 64, 13: 64, 14: 64, 15: 64, 17: 136, 18: 128, 19: 96,
               20: 64}


def commit_ht_rows(a, ctx, dev, stream, rng, B, hashes):
    """sig_hashed_verify / sig_hashed_sign / schnorr_verify / schnorr_sign / bip0340_sign with a hash of ec_digest_slots_batch that the
    older names refuse (--hash 5 .. 11, 13 .. 15, 17 .. 20, or --hashes): the _ht entry point under that hash beside its SHA-256 twin
    through the OLD name on the same keys, and beside the bare ec_digest_slots_batch_dev of both hashes at the length of each one's
    commitment hash input, in alternating windows of a.steps calls in one run.  bip0340_sign also times the nonce call by itself
    (keys supplied, so it is the on-curve test and the nonce kernel).  32-octet messages, device-resident inputs, 4096 distinct keys
    tiled over the batch.  ECKCDSA's h = H(z || m) is made by ec_digest_slots_batch_dev before the timed region, as the header's
    composition does it.  Gates per hash: every item signs, every device-made signature is accepted, none for its neighbour's input.
    One JSON line per hash.  expected_ms = twin + (bare_new - bare_twin)."""
    if a.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise SystemExit("--workload %s measures one GPU: run it with --gpus 1, outside torch.distributed.run" % a.workload)
    import oracles as O
    from libecc_amd.api import DIGEST_SIZES
    wl = a.workload
    if wl.startswith("sig_hashed"):
        alg = {"eckcdsa": 2, "ecsdsa": 3, "ecosdsa": 4}.get(a.alg)
    elif wl.startswith("schnorr"):
        alg = {"bip0340": 20, "ecfsdsa": 5}.get(a.alg)
    else:
        alg = 20
    if alg is None:
        raise SystemExit("--workload %s: --alg does not name one of its schemes" % wl)
    sign, derive, hsig, bip, kcdsa = wl.endswith("_sign"), wl == "bip0340_sign", alg in (2, 3, 4), alg == 20, alg == 2
    curve = a.curve
    cv = ctx.curve(curve)
    q, ql, cl, mlen = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve), 32
    if q.bit_length() <= 8 * ql - 8:
        raise SystemExit("--workload %s: the order must fill its top octet's neighbour (nonces are drawn below 2^(8 qlen - 8))" % wl)
    K = min(B, 4096)
    xs = [1 + int.from_bytes(rng.integers(0, 256, size=ql + 8, dtype=np.uint8).tobytes(), "big") % (q - 1) for _ in range(K)]
    pubs_k, st = cv.scalar_mult(b"".join((pow(x, -1, q) if kcdsa else x).to_bytes(ql, "big") for x in xs))
    assert set(st) == {0}
    tile = lambda bs, w: np.tile(np.frombuffer(bs, dtype=np.uint8).reshape(K, w), (B // K, 1))
    privs, pubs = tile(b"".join(x.to_bytes(ql, "big") for x in xs), ql), tile(pubs_k, 2 * cl)
    vals = rng.integers(0, 256, size=(B, ql), dtype=np.uint8)      # nonces (below 2^(8 qlen - 8) < q, odd) or BIP0340's aux values
    if not derive:
        vals[:, 0] = 0
        vals[:, -1] |= 1
    msgs = rng.integers(0, 256, size=(B, mlen), dtype=np.uint8)
    S = stream.cuda_stream
    tt = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    d_priv, d_pub, d_val = tt(privs), tt(pubs), tt(vals)
    d_st, d_res = torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)

    def slots_of(fixed, length):
        stride = (4 + length + 3) & ~3
        sl = np.zeros((B, stride), dtype=np.uint8)
        sl[:, :4] = np.frombuffer(np.uint32(length).tobytes(), dtype=np.uint8)
        sl[:, 4:4 + len(fixed)] = np.frombuffer(fixed, dtype=np.uint8) if fixed else 0
        return sl, stride

    def setup(ht, new):
        """the device inputs of one hash, its signatures (made by the device, all status 0) and the four timed calls"""
        hs, blk = DIGEST_SIZES[ht], HASH_BLOCKS[ht]
        sfx = "_ht" if new else ""
        if kcdsa:
            z = np.zeros((B, blk), dtype=np.uint8)
            z[:, :min(blk, 2 * cl)] = pubs[:, :min(blk, 2 * cl)]
            zs, zstride = slots_of(b"", blk + mlen)
            zs[:, 4:4 + blk], zs[:, 4 + blk:4 + blk + mlen] = z, msgs
            d_in, stride = torch.empty(B * hs, dtype=torch.uint8, device=dev), hs
            ctx.digest_slots_dev(ht, B, tt(zs).data_ptr(), zstride, d_in.data_ptr(), S)
            hin = cl                                                   # the device hashes FE2OS(W.x)
        else:
            if bip:
                tag = ctx.digest_slots(ht, (17).to_bytes(4, "little") + b"BIP0340/challenge" + bytes(3), 24)
                fixed = tag + tag + bytes(2 * cl)
            else:
                fixed = bytes(cl if alg == 4 else 2 * cl)
            hin = len(fixed) + mlen
            sl, stride = slots_of(fixed, hin)
            sl[:, 4 + len(fixed):4 + hin] = msgs
            d_in = tt(sl)
        siglen = ((min(hs, ql) if kcdsa else hs) if hsig else (cl if bip else 2 * cl)) + ql
        d_sig = torch.empty(B * siglen, dtype=torch.uint8, device=dev)
        P = lambda x: x.data_ptr()
        if hsig:
            do_sign = lambda: getattr(cv, "sig_hashed_sign%s_dev" % sfx)(alg, ht, B, P(d_priv), P(d_val), P(d_in), stride, P(d_sig), P(d_st), S)
            do_ver = lambda inp: getattr(cv, "sig_hashed_verify%s_dev" % sfx)(alg, ht, B, P(d_pub), P(d_sig), P(inp), stride, P(d_res), S)
        else:
            if derive:
                do_sign = lambda: getattr(cv, "bip0340_sign%s_dev" % sfx)(ht, B, P(d_priv), None, P(d_val), P(d_in), stride, P(d_sig), P(d_st), S)
            else:
                do_sign = lambda: getattr(cv, "schnorr_sign%s_dev" % sfx)(alg, ht, B, P(d_priv), None, P(d_val), P(d_in), stride, P(d_sig), P(d_st), S)
            do_ver = lambda inp: getattr(cv, "schnorr_verify%s_dev" % sfx)(alg, ht, B, P(d_pub), 0, P(d_sig), P(inp), stride, P(d_res), S)
        do_sign()
        torch.cuda.synchronize()
        if bytes(d_st.cpu().numpy()) != bytes(B):
            raise SystemExit("PARITY FAILURE: hash %d: an item did not sign" % ht)
        do_ver(d_in)
        torch.cuda.synchronize()
        if bytes(d_res.cpu().numpy()) != bytes(B):
            raise SystemExit("PARITY FAILURE: hash %d: a signature the device made was rejected" % ht)
        do_ver(torch.roll(d_in, stride))
        torch.cuda.synchronize()
        if bytes(d_res.cpu().numpy()) != b"\1" * B:
            raise SystemExit("PARITY FAILURE: hash %d: a signature was accepted for another item's input" % ht)
        bs, bstride = slots_of(b"", hin)
        bs[:, 4:4 + hin] = rng.integers(0, 256, size=(B, hin), dtype=np.uint8)
        d_bare, d_dg = tt(bs), torch.empty(B * hs, dtype=torch.uint8, device=dev)
        bare = lambda: ctx.digest_slots_dev(ht, B, P(d_bare), bstride, P(d_dg), S)
        nonce = None
        if derive:
            d_k = torch.empty(B * ql, dtype=torch.uint8, device=dev)
            nonce = lambda: getattr(cv, "bip0340_nonce%s_dev" % sfx)(ht, B, P(d_priv), P(d_pub), P(d_val), P(d_in), stride, P(d_k), P(d_st), S)
        keep = (d_in, d_sig, d_bare, d_dg)
        return (do_sign if sign else (lambda: do_ver(d_in))), bare, nonce, hin, keep

    twin = setup(2, False)
    for ht in hashes:
        new = setup(ht, True)
        fns = [("twin", twin[0]), ("new", new[0]), ("bare_new", new[1]), ("bare_twin", twin[1])]
        if derive:
            fns += [("nonce_new", new[2]), ("nonce_twin", twin[2])]
        for _ in range(a.warmup):
            for _, fn in fns:
                fn()
        torch.cuda.synchronize()
        acc = {name: [] for name, _ in fns}
        for _ in range(3):
            for name, fn in fns:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                acc[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
        med = {name: float(np.median(v)) for name, v in acc.items()}
        expected = med["twin"] + med["bare_new"] - med["bare_twin"]
        kind = "signatures" if sign else "verifications"
        rec = {"metric": "%s %s/sec (%s, hash %d through the _ht name, batch=2^%d, device-resident)" % (a.alg.upper() if not derive else "BIP0340", kind,
                                                                                                         curve.lower(), ht, a.batch_log2),
               "value": B / (1e-3 * med["new"]), "unit": kind + "/s", "hash": ht, "ms": med, "windows_ms": acc, "hash_input_octets": {"new": new[3], "twin": twin[3]},
               "expected_ms": expected, "new_over_expected": med["new"] / expected,
               "gate": "all 2^%d items sign, all device-made signatures accepted, none for its neighbour's input" % a.batch_log2,
               "config": {"workload": wl, "alg": a.alg, "curve": curve, "steps": a.steps, "warmup": a.warmup, "windows": 3}}
        if derive:
            rec["nonce_over_bare"] = {"new": med["nonce_new"] / med["bare_new"], "twin": med["nonce_twin"] / med["bare_twin"]}
        print(json.dumps(rec), flush=True)
        del new
    cv.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["ecdsa_verify", "ecdsa_recover", "sig_verify", "sig_sign", "sig_msg_verify", "sig_msg_sign", "hash_slots", "digest_slots", "digest_msgs", "eddsa_verify_msgs", "eddsa_sign_msgs", "hmac_slots", "sig_hashed_verify", "sig_hashed_sign", "schnorr_verify", "schnorr_sign", "bign_verify", "bign_sign", "decdsa_sign", "dbign_sign", "bip0340_sign", "eddsa_sign", "ecdsa_sign", "ecccdh", "ed25519_verify", "ed448_verify", "x25519", "x448", "bip0340_msm", "ed25519_msm", "ed448_msm"])
    ap.add_argument("--alg", default="sm2", choices=["ecgdsa", "ecrdsa", "sm2", "eckcdsa", "ecsdsa", "ecosdsa", "bip0340", "ecfsdsa",
                                                    "ed25519", "ed25519ctx", "ed25519ph", "ed448", "ed448ph"],
                    help="eddsa_sign: ed25519, ed25519ctx, ed25519ph, ed448, ed448ph; sig_verify / sig_sign: ecgdsa, ecrdsa, sm2; sig_hashed_verify / sig_hashed_sign: eckcdsa, ecsdsa, ecosdsa; schnorr_verify / schnorr_sign: bip0340, ecfsdsa")
    ap.add_argument("--hash", type=int, default=None, choices=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20],
                    help="bign_verify / bign_sign: 0 the caller hashed (SHA-256 digests supplied), 16 (default) belt-hash of message slots on the device; "
                         "decdsa_sign: SHA-256 by default, 1 .. 4 through ec_decdsa_sign_batch, the rest through ec_decdsa_sign_ht_batch; digest_slots, hmac_slots: any of libecc's numbers but 0 and 16 (default 6, SHA3-256)")
    ap.add_argument("--hashes", default=None, help="sig_hashed_verify / sig_hashed_sign / schnorr_verify / schnorr_sign / bip0340_sign: a comma-separated list of the "
                    "hash numbers 5 .. 11, 13 .. 15, 17 .. 20, or 'new' for all fourteen, measured in one run through the _ht names (--hash N: one of them)")
    ap.add_argument("--lens", default="32", choices=["32", "1024", "mixed"], help="digest_msgs / eddsa_verify_msgs / eddsa_sign_msgs: the message lengths (digest_msgs_lens documents `mixed`)")
    ap.add_argument("--secret", action="store_true", help="dbign_sign / bip0340_sign: the context in secret-scalar mode")
    ap.add_argument("--derive-pub", action="store_true", help="eddsa_sign: pubkeys = NULL, A = encode([a]B) derived on the device (a second comb multiplication per item)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch-log2", type=int, default=20)
    ap.add_argument("--curve", default="SECP256R1", help="ecdsa_verify / ecdsa_sign / ecccdh: any 256-bit prime-order curve libecc names")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--ref-items", type=int, default=4096, help="random items of the batch checked against the unmodified reference binary (all host threads)")
    ap.add_argument("--traffic", action="store_true", help="after the timed region: HBM bytes per launch from two rocprofv3 --pmc child runs (tools/pmc.py)")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--mad-peak", type=float, default=0.0, help="lane-MADs/s of the v_mad_u64_u32 streams measured by ubench (VGPR multiplier); 0: measure now")
    ap.add_argument("--mad-peak-sgpr", type=float, default=0.0, help="the same with an SGPR multiplier")
    a = ap.parse_args()
    commit_hashes = None
    if a.workload in ("sig_hashed_verify", "sig_hashed_sign", "schnorr_verify", "schnorr_sign", "bip0340_sign"):
        if a.hashes is not None:
            commit_hashes = NEW_COMMIT_HASHES if a.hashes == "new" else [int(h) for h in a.hashes.split(",")]
        elif a.hash in NEW_COMMIT_HASHES:
            commit_hashes = [a.hash]
        if commit_hashes is not None and not set(commit_hashes) <= set(NEW_COMMIT_HASHES):
            raise SystemExit("--workload %s: --hash / --hashes 5 .. 11, 13 .. 15 or 17 .. 20 (1 .. 4 are the workload without --hash)" % a.workload)
    if a.hash is None and a.workload in ("sig_msg_verify", "sig_msg_sign", "hash_slots"):
        a.hash = {"sm2": 11, "ecrdsa": 13, "ecgdsa": 2}.get(a.alg, 11)   # the hash each scheme is deployed with
    if a.hash is None and a.workload in ("digest_slots", "digest_msgs", "hmac_slots"):
        a.hash = 6
    if a.hash is None:
        a.hash = 2 if a.workload == "decdsa_sign" else 16
    # the option means something to these workloads only; the others ignore it, as they always have
    if a.workload == "decdsa_sign" and a.hash in (0, 16):
        raise SystemExit("--workload decdsa_sign: --hash 1 .. 11, 13 .. 15 or 17 .. 20")
    if a.workload in ("bign_verify", "bign_sign") and a.hash not in (0, 16):
        raise SystemExit("--workload %s: --hash 0 or 16" % a.workload)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_
        dist = dist_
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=dev)
    import oracles as O
    if rank == 0:
        O.build_oracle()
    if dist is not None:
        dist.barrier()
    B = 1 << a.batch_log2
    rng = np.random.default_rng(SEED + rank)
    ctx = libecc_amd.Context(local_rank)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)

    def rb(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    def t(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    t_setup = time.time()
    ref_subset = work = gate_ref = None
    if a.workload == "ecdsa_recover":
        return recover_row(a, ctx, dev, stream, rng, B)
    if a.workload in ("sig_verify", "sig_sign"):
        return sig_family_row(a, ctx, dev, stream, rng, B)
    if a.workload in ("sig_msg_verify", "sig_msg_sign", "hash_slots"):
        return sig_msg_row(a, ctx, dev, stream, rng, B)
    if a.workload == "digest_slots":
        return digest_slots_row(a, ctx, dev, stream, rng, B)
    if a.workload == "digest_msgs":
        return digest_msgs_row(a, ctx, dev, stream, rng, B)
    if a.workload in ("eddsa_verify_msgs", "eddsa_sign_msgs"):
        return eddsa_msgs_row(a, ctx, dev, stream, rng, B)
    if a.workload == "hmac_slots":
        return hmac_slots_row(a, ctx, dev, stream, rng, B)
    if commit_hashes is not None:
        return commit_ht_rows(a, ctx, dev, stream, rng, B, commit_hashes)
    if a.workload in ("sig_hashed_verify", "sig_hashed_sign"):
        return sig_hashed_row(a, ctx, dev, stream, rng, B)
    if a.workload in ("schnorr_verify", "schnorr_sign"):
        return schnorr_row(a, ctx, dev, stream, rng, B)
    if a.workload in ("bign_verify", "bign_sign"):
        return bign_row(a, ctx, dev, stream, rng, B)
    if a.workload == "decdsa_sign":
        return decdsa_row(a, ctx, dev, stream, rng, B)
    if a.workload in ("dbign_sign", "bip0340_sign"):
        return det_sign_row(a, ctx, dev, stream, rng, B)
    if a.workload == "eddsa_sign":
        if not a.alg.startswith("ed"):
            raise SystemExit("--workload eddsa_sign: --alg ed25519 | ed25519ctx | ed25519ph | ed448 | ed448ph")
        return eddsa_sign_row(a, ctx, dev, stream, rng, B)
    if a.workload == "ecdsa_verify":
        curve = a.curve
        cv = ctx.curve(curve)
        q = O.CURVES[curve]["q"]
        ql, cl = O.qlen(curve), O.clen(curve)
        hname, hl = ("SHA256", 32) if ql <= 32 else (("SHA384", 48) if ql <= 48 else ("SHA512", 64))
        raw = rng.integers(0, 256, size=(2, B, ql + 8), dtype=np.uint8)

        def scal(rows):
            return b"".join(((int.from_bytes(rows[i].tobytes(), "big") % (q - 1)) + 1).to_bytes(ql, "big") for i in range(B))
        ML = 32
        msgs = rb(ML * B)
        privs, nonces = scal(raw[0]), scal(raw[1])
        hf = getattr(hashlib, hname.lower())
        dg = b"".join(hf(msgs[ML * i:ML * (i + 1)]).digest() for i in range(B))
        pubs, st = cv.scalar_mult(privs)
        assert set(st) == {0}
        sigs, st = cv.ecdsa_sign(privs, nonces, dg, hl)
        assert set(st) == {0}
        sigs = bytearray(sigs)
        bad = np.zeros(B, dtype=np.uint8)
        for i in range(0, B, 10):          # every 10th signature corrupted
            sigs[2 * ql * i + ql + (i % ql)] ^= 1 << (i % 8)
            bad[i] = 1
        sigs = bytes(sigs)
        ins = [t(pubs), t(sigs), t(dg)]
        d_res = torch.empty(B, dtype=torch.uint8, device=dev)

        def step():
            cv.ecdsa_verify_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), hl, d_res.data_ptr(),
                                stream.cuda_stream)
        expected = bad.tobytes()

        def oracle_subset(idx):
            o = O.Oracle(curve)
            return o.ecdsa_verify(b"".join(pubs[2 * cl * i:2 * cl * (i + 1)] for i in idx), b"".join(sigs[2 * ql * i:2 * ql * (i + 1)] for i in idx),
                                  b"".join(dg[hl * i:hl * (i + 1)] for i in idx), hl)

        def ref_subset(idx):
            r = O.RefLib(curve)
            sp, ss, sm = (b"".join(x[w * i:w * i + w] for i in idx) for x, w in ((pubs, 2 * cl), (sigs, 2 * ql), (msgs, ML)))
            return O.join_slices(O.in_slices(lambda lo, hi: r.ecdsa_verify(hname, sp[2 * cl * lo:2 * cl * hi], ss[2 * ql * lo:2 * ql * hi], sm[ML * lo:ML * hi], ML), len(idx)))
        # dominant kernel k_p256_verify_loop<COMB>: the top digit's mixed addition, 64 windows of 4 doublings + 1 mixed addition on Q's
        # table, 17 mixed additions from the comb table of G, the projective x mod q == r test (1 S + 6 M); M = 117, S = 81 MADs
        work = {"kernel": "k_p256_verify_loop<true>", "mads_per_item": 64 * (24 * 117 + 19 * 81) + 18 * (8 * 117 + 3 * 81) + 81 + 6 * 117,
                "sgpr_mads_per_item": 36 * (64 * 43 + 18 * 11 + 7)} if curve == "SECP256R1" else None
        if work:
            # the whole step: k_p256_table (44 M + 27 S) and k_p256_affine (42 M + 7 S + one Fermat inversion, 255 S + 13 M, per 8 items)
            # in front of the loop; k_ecdsa_prep / k_ecdsa_fin (mod-q words on the saturated unit) not counted
            work["step_mads_per_item"] = work["mads_per_item"] + (44 + 42 + 13 / 8) * 117 + (27 + 7 + 255 / 8) * 81
            work["alg_bytes_per_item"] = 2 * cl + 2 * ql + hl + 1
        metric, unit, cfg = "ECDSA verifications/sec (%s, %s digests, batch=2^%d)" % (curve.lower(), hname, a.batch_log2), "verifications/s", 3
    elif a.workload in ("ecdsa_sign", "ecccdh"):
        # secp256r1: signing with caller-supplied nonces (the tail of ec_sign) / ECC-CDH shared secrets
        curve = a.curve
        assert O.CURVES[curve]["p"].bit_length() == 256 and O.CURVES[curve]["q"].bit_length() == 256
        cv = ctx.curve(curve)
        q = O.CURVES[curve]["q"]
        raw = rng.integers(0, 256, size=(2, B, 40), dtype=np.uint8)

        def scal(rows):
            return b"".join(((int.from_bytes(rows[i].tobytes(), "big") % (q - 1)) + 1).to_bytes(32, "big") for i in range(B))
        privs, other = scal(raw[0]), scal(raw[1])
        d_res = torch.empty(B, dtype=torch.uint8, device=dev)
        expected = bytes(B)
        if a.workload == "ecdsa_sign":
            dg = rb(32 * B)
            ins = [t(privs), t(other), t(dg)]
            out_w = 64
            d_out = torch.empty(out_w * B, dtype=torch.uint8, device=dev)

            def step():
                cv.ecdsa_sign_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), 32, d_out.data_ptr(),
                                  d_res.data_ptr(), stream.cuda_stream)

            def oracle_subset(idx):
                cut = lambda b: b"".join(b[32 * i:32 * i + 32] for i in idx)
                return O.Oracle(curve).ecdsa_sign(cut(privs), cut(other), cut(dg), 32)
            metric, unit, cfg = "ECDSA signatures/sec (%s, nonces supplied, batch=2^%d)" % (curve.lower(), a.batch_log2), "signatures/s", 3
        else:
            peers, st = cv.scalar_mult(other)
            assert set(st) == {0}
            ins = [t(privs), t(peers)]
            out_w = 32
            d_out = torch.empty(out_w * B, dtype=torch.uint8, device=dev)

            def step():
                cv.ecccdh_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), d_out.data_ptr(), d_res.data_ptr(), stream.cuda_stream)

            def oracle_subset(idx):
                return O.Oracle(curve).ecccdh(b"".join(privs[32 * i:32 * i + 32] for i in idx),
                                              b"".join(peers[64 * i:64 * i + 64] for i in idx))
            metric, unit, cfg = "ECC-CDH shared secrets/sec (%s, batch=2^%d)" % (curve.lower(), a.batch_log2), "shared-secrets/s", 3
    elif a.workload == "ed25519_verify":
        cv = ctx.curve("WEI25519")
        if a.traffic_child:
            # the PMC passes only need the shape of the work: 512 signatures of the Python signer, tiled
            m = 512
            emsgs = [rb(32) for _ in range(m)]
            items = [O.ed25519_sign(rb(32), emsgs[j]) for j in range(m)]
            reps = B // m
            pubs = b"".join(i[0] for i in items) * reps
            sigs = bytearray(b"".join(i[1] for i in items) * reps)
            hram = b"".join(i[2] for i in items) * reps
            msgs = b"".join(emsgs) * reps
            distinct = "%d distinct signatures tiled" % m
        else:
            # B DISTINCT (key, message, signature) triples: RFC 8032 5.1.5 / 5.1.6 with the hashes on the host and the
            # three scalar-multiplication / mod-q steps on the GPU through the library's own signing entry points
            # (ec_eddsa_sign_R_batch also serves for A = [a]B: it encodes [x mod q]B for any 64-byte x)
            seeds, msgs = rb(32 * B), rb(32 * B)
            hk = [hashlib.sha512(seeds[32 * i:32 * i + 32]).digest() for i in range(B)]
            a_np = np.frombuffer(b"".join(h[:32] for h in hk), dtype=np.uint8).reshape(B, 32).copy()
            a_np[:, 0] &= 248
            a_np[:, 31] &= 127
            a_np[:, 31] |= 64
            a_le = a_np.tobytes()
            wide = np.zeros((B, 64), dtype=np.uint8)
            wide[:, :32] = a_np
            pubs, st = cv.eddsa_sign_R(wide.tobytes())
            assert set(st) == {0}
            r_hash = b"".join(hashlib.sha512(hk[i][32:] + msgs[32 * i:32 * i + 32]).digest() for i in range(B))
            Renc, st = cv.eddsa_sign_R(r_hash)
            assert set(st) == {0}
            hram = b"".join(hashlib.sha512(Renc[32 * i:32 * i + 32] + pubs[32 * i:32 * i + 32] + msgs[32 * i:32 * i + 32]).digest() for i in range(B))
            S = cv.eddsa_sign_S(r_hash, hram, a_le)
            sg = np.empty((B, 64), dtype=np.uint8)
            sg[:, :32] = np.frombuffer(Renc, dtype=np.uint8).reshape(B, 32)
            sg[:, 32:] = np.frombuffer(S, dtype=np.uint8).reshape(B, 32)
            sigs = bytearray(sg.tobytes())
            del hk, wide, sg
            distinct = "all keys, messages and signatures distinct, signed on the GPU by ec_eddsa_sign_R/S_batch"
        bad = np.zeros(B, dtype=np.uint8)
        for i in range(0, B, 10):          # every 10th signature corrupted in S (the hash binds R, A and M, not S)
            sigs[64 * i + 32 + (i % 31)] ^= 1 << (i % 8)
            bad[i] = 1
        sigs = bytes(sigs)
        ins = [t(pubs), t(sigs), t(hram)]
        d_res = torch.empty(B, dtype=torch.uint8, device=dev)

        def step():
            cv.eddsa_verify_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), d_res.data_ptr(), stream.cuda_stream)
        expected = bad.tobytes()

        def oracle_subset(idx):
            o = O.Oracle("WEI25519")
            return o.eddsa_verify(b"".join(pubs[32 * i:32 * i + 32] for i in idx), b"".join(sigs[64 * i:64 * i + 64] for i in idx),
                                  b"".join(hram[64 * i:64 * i + 64] for i in idx))

        def ref_subset(idx):
            sp, ss, sm = (b"".join(x[w * i:w * i + w] for i in idx) for x, w in ((pubs, 32), (sigs, 64), (msgs, 32)))
            return O.join_slices(O.in_slices(lambda lo, hi: O.ref_ed25519_verify(sp[32 * lo:32 * hi], ss[64 * lo:64 * hi], sm[32 * lo:32 * hi], 32), len(idx)))
        if os.environ.get("ECAMD_NO_ED_LATTICE") or os.environ.get("ECAMD_NO_ED_TAIL"):
            # the full-length form (round 4, first step): k_ed_smul_c25519<1>, 64 windows of 3 doublings (3M + 4S), 1 doubling (4M + 4S) and
            # 1 addition without its T (7M); M = 81 + 16 = 97, S = 45 + 16 = 61 MADs, 16 of them with a constant multiplier
            work = {"kernel": "k_ed_smul_c25519<1>", "mads_per_item": 64 * (20 * 97 + 16 * 61), "sgpr_mads_per_item": 64 * 36 * 16}
            # whole step: decode 59 M + 522 S, window table 49 M + 16 S, the loop, k_ed_tail_c25519 162 M + 13 S
            work["step_mads_per_item"] = (59 + 49 + 64 * 20 + 162) * 97 + (522 + 16 + 64 * 16 + 13) * 61
        else:
            # half-length scalars (k_ed_lat): dominant kernel k_ed_smul2_c25519<1, 33>, 33 windows of 3 doublings (3M + 4S), 1 doubling with T
            # (4M + 4S), 1 addition with T (8M) and 1 without (7M) over the tables of A and R
            work = {"kernel": "k_ed_smul2_c25519<1, 33>", "mads_per_item": 33 * (28 * 97 + 16 * 61), "sgpr_mads_per_item": 33 * 44 * 16}
            # the whole step: k_ed_decode_ed_c25519 (two square roots: 2 x (255 S + 25 M), the key's cofactor doublings: 59 M + 522 S),
            # k_ed_lat (word arithmetic mod q and the Euclidean loop: no MADs of this unit), the two window tables (2 x (49 M + 16 S): four
            # doublings with T, three additions, eight entries of one multiplication each), the loop, k_ed_tail2_c25519 (two comb passes
            # of 17 mixed additions, the comparisons, one addition, three doublings: 264 M + 13 S)
            work["step_mads_per_item"] = (59 + 98 + 33 * 28 + 264) * 97 + (522 + 32 + 33 * 16 + 13) * 61
        work["alg_bytes_per_item"] = 32 + 64 + 64 + 1
        metric, unit, cfg = "Ed25519 verifications/sec (batch=2^%d, %s)" % (a.batch_log2, distinct), "verifications/s", 4
    elif a.workload in ("bip0340_msm", "ed25519_msm", "ed448_msm"):
        # the reference's whole-batch verification (ec_verify_batch -> bip0340_verify_batch sig/bip0340.c:1296,
        # eddsa_verify_batch sig/eddsa.c:2904) as ONE multi-scalar multiplication.  A step is one verdict over B VALID signatures resident in
        # HBM (a batch with a bad item comes back "not decided" in the same time and the caller then runs the item form: that path is
        # the ed25519_verify / item-form workload).  Gates: the verdict for the valid batch, the verdict with one item damaged at a random
        # index, and the unmodified reference's own batch function on random contiguous pieces of the same batch (see oracles.py:
        # its Bos-Coster / no-memory verifiers take minutes per 2^17 items on one thread, so the batch is sampled in pieces).
        msm_bad = None
        d_res = torch.full((1,), 7, dtype=torch.uint8, device=dev)
        expected = bytes(1)
        if a.workload == "bip0340_msm":
            curve = "SECP256K1" if a.curve == "SECP256R1" else a.curve
            cv = ctx.curve(curve)
            assert cv.schnorr_msm_available(1)
            if a.traffic_child:
                # the PMC passes only need the shape of the work: valid points and scalars below q; the equation need not hold
                cl, ql = cv.clen, cv.qlen
                raw = rng.integers(0, 256, size=(4, B * ql), dtype=np.uint8)
                raw[:, ::ql] &= 0x7f
                Pk, _ = cv.scalar_mult(raw[0].tobytes())
                Rk, _ = cv.scalar_mult(raw[1].tobytes())
                it = {"s": raw[2].tobytes(), "ne": raw[3].tobytes(), "keys": Pk, "cl": cl, "ql": ql,
                      "rx": np.frombuffer(Rk, dtype=np.uint8).reshape(B, 2 * cl)[:, :cl].tobytes()}
            else:
                it = O.make_bip0340_batch(lambda sc: cv.scalar_mult(sc), curve, B, rng)
            cl, ql = it["cl"], it["ql"]
            ins = [t(it["s"]), t(it["ne"]), t(it["keys"]), t(it["rx"])]
            bad_i = int(rng.integers(0, B))
            bad_s = bytearray(it["s"][ql * bad_i:ql * (bad_i + 1)])
            bad_s[ql - 1] ^= 1

            def step():
                cv.schnorr_verify_all_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), 1, d_res.data_ptr(),
                                          stream.cuda_stream)

            def msm_bad():
                good = ins[0][ql * bad_i:ql * (bad_i + 1)].clone()
                ins[0][ql * bad_i:ql * (bad_i + 1)] = t(bytes(bad_s))
                step()
                torch.cuda.synchronize()
                v = int(d_res.item())
                ins[0][ql * bad_i:ql * (bad_i + 1)] = good
                return v, bad_i

            def ref_pieces(pieces):
                def one(lo, hi):
                    return all(O.ref_sig_verify_all(curve, "BIP0340", "SHA256", it["pubs"][2 * cl * l:2 * cl * h], it["sigs"][(cl + ql) * l:(cl + ql) * h],
                                                    cl + ql, it["msgs"][32 * l:32 * h], 32) for l, h in pieces[lo:hi])
                return all(O.in_slices(one, len(pieces)))
            K = max(1, min(8, B >> 18))
            nl, M, S, red = 9, 101, 65, 20       # secp256k1's flavour (ecamd_u29g.h: 81 + 20 / 45 + 20 MADs)
            if curve != "SECP256K1":
                import bench as _b
                nl, M, S, red = _b.field_mads(O.CURVES[curve]["p"])
            dbl = (3, 4) if O.CURVES[curve]["a"] == 0 else (4, 4)
            # k_msm_loop_g: per lane 64 windows x 4 doublings shared by K items; per item 64 additions of key multiples and 33 of R's
            # (z_i has 128 bits), Jacobian + Jacobian 12M + 4S each
            loop = (256 / K) * (dbl[0] * M + dbl[1] * S) + 97 * (12 * M + 4 * S)
            # k_msm_table_g per item: lift_x of r (a square root: ~ |p| squarings + 12 M) and the import of Y, then 2 x (4 doublings + 3 additions)
            pb = O.CURVES[curve]["p"].bit_length()
            table = (pb * S + 12 * M) + 2 * (4 * (dbl[0] * M + dbl[1] * S) + 3 * (12 * M + 4 * S)) + 8 * M
            work = {"kernel": "k_msm_loop_g", "mads_per_item": loop, "sgpr_mads_per_item": loop * red / M,
                    "step_mads_per_item": loop + table, "alg_bytes_per_item": ql + ql + 2 * cl + cl}
            how = "Straus, K = %d items per lane" % K
            qb = O.CURVES[curve]["q"].bit_length()
            algo = os.environ.get("ECAMD_SCHNORR_MSM_ALGO") or ("bucket" if B >= (1 << 17) else "straus")
            if algo == "bucket" and qb - 16 * ((qb - 1) // 16) >= 12:
                # round 6, the bucket evaluation (ecamd_host_msm.cpp:schnorr_msm_use_buckets): per item 8 ql / 16 windows of the key's scalar and 8 of
                # z_i, one complete addition with an affine operand each (add_aff: 10M + 3S) in k_bkt_accum_g, the dominant kernel; the step
                # adds the import of the two points (the key: on-curve check; r: a square root), and the bucket reduction -- 2^16 buckets
                # per window, 2 Jacobian additions (12M + 4S) each, whatever the batch size
                pairs = (8 * ql + 15) // 16 + 8
                acc = pairs * (10 * M + 3 * S)
                front = (pb * S + 14 * M) + 5 * M + 2 * S
                reduce_ = ((8 * ql + 15) // 16) * 65536 * 2 * (12 * M + 4 * S) / B
                work = {"kernel": "k_bkt_accum_g", "mads_per_item": acc, "sgpr_mads_per_item": acc * red / M,
                        "step_mads_per_item": acc + front + reduce_, "alg_bytes_per_item": ql + ql + 2 * cl + cl}
                how = "buckets, 16-bit windows, %d additions per item" % pairs
            metric, unit, cfg = "BIP0340 signatures/sec in whole-batch verification (%s, one multi-scalar multiplication per 2^%d-item batch: %s)" % (curve.lower(), a.batch_log2, how), "verifications/s", "f4"
            ref_what = "ec_verify_batch (BIP0340: bip0340_verify_batch, no scratch pad)"
        elif a.workload == "ed448_msm":
            # round 6: EDDSA448's batch equation on the Weierstrass model WEI448 -- 2^batch_log2 DISTINCT signatures made here (keys, [r]B and S on
            # the device, SHAKE256 by hashlib), the Schnorr-type combination on the Goldilocks unit with the cofactored final test
            cv = ctx.curve("WEI448")
            dom = O.ed_dom4(0, b"")
            shake = lambda x: hashlib.shake_256(x).digest(114)
            if a.traffic_child:
                pubs, _ = cv.eddsa_sign_R(rb(114 * B))
                Renc, _ = cv.eddsa_sign_R(rb(114 * B))
                sg = np.zeros((B, 114), dtype=np.uint8)
                sg[:, :57] = np.frombuffer(Renc, dtype=np.uint8).reshape(B, 57)
                sg[:, 57:112] = rng.integers(0, 256, size=(B, 55), dtype=np.uint8)
                sigs, hram, msgs = sg.tobytes(), rb(114 * B), b""
            else:
                seeds, msgs = rb(57 * B), rb(32 * B)
                hk = [shake(seeds[57 * i:57 * i + 57]) for i in range(B)]
                a_np = np.frombuffer(b"".join(h[:57] for h in hk), dtype=np.uint8).reshape(B, 57).copy()
                a_np[:, 0] &= 252
                a_np[:, 55] |= 128
                a_np[:, 56] = 0
                wide = np.zeros((B, 114), dtype=np.uint8)
                wide[:, :57] = a_np
                pubs, st = cv.eddsa_sign_R(wide.tobytes())
                assert set(st) == {0}
                r_hash = b"".join(shake(dom + hk[i][57:] + msgs[32 * i:32 * i + 32]) for i in range(B))
                Renc, st = cv.eddsa_sign_R(r_hash)
                assert set(st) == {0}
                hram = b"".join(shake(dom + Renc[57 * i:57 * i + 57] + pubs[57 * i:57 * i + 57] + msgs[32 * i:32 * i + 32]) for i in range(B))
                Sb = cv.eddsa_sign_S(r_hash, hram, a_np.tobytes())
                sg = np.empty((B, 114), dtype=np.uint8)
                sg[:, :57] = np.frombuffer(Renc, dtype=np.uint8).reshape(B, 57)
                sg[:, 57:] = np.frombuffer(Sb, dtype=np.uint8).reshape(B, 57)
                sigs = sg.tobytes()
                del hk, wide, sg
            ins = [t(pubs), t(sigs), t(hram)]
            bad_i = int(rng.integers(0, B))
            ctx.set_eddsa_msm(2, 0, 0)

            def step():
                cv.eddsa_verify_all_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), d_res.data_ptr(), stream.cuda_stream)

            def msm_bad():
                pos = 114 * bad_i + 70
                ins[1][pos] ^= 1
                step()
                torch.cuda.synchronize()
                v = int(d_res.item())
                ins[1][pos] ^= 1
                return v, bad_i

            def ref_pieces(pieces):
                def one(lo, hi):
                    return all(O.ref_eddsa_verify_all(pubs[57 * l:57 * h], sigs[114 * l:114 * h], msgs[32 * l:32 * h], 32, ed448=True) for l, h in pieces[lo:hi])
                return all(O.in_slices(one, len(pieces)))
            import bench as _b
            nl, M, S, red = _b.field_mads(O.CURVES["WEI448"]["p"])
            K = max(1, min(8, B >> 18))
            loop = (448 / K) * (4 * M + 4 * S) + (112 + 33) * (12 * M + 4 * S)
            # the front end: two decodings (a square root and two inversions-by-exponentiation each: ~ 3 x 448 S + 60 M), [4]A, S and h mod q
            front = 2 * (3 * 448 * S + 60 * M) + 2 * (4 * M + 4 * S)
            work = {"kernel": "k_msm_loop_g", "mads_per_item": loop, "sgpr_mads_per_item": loop * red / M, "step_mads_per_item": loop + front,
                    "alg_bytes_per_item": 57 + 114 + 114}
            how = "Straus, K = %d items per lane" % K
            algo = os.environ.get("ECAMD_SCHNORR_MSM_ALGO") or ("bucket" if B >= (1 << 17) else "straus")
            if algo == "bucket":
                pairs = 28 + 8
                acc = pairs * (10 * M + 3 * S)
                reduce_ = 28 * 65536 * 2 * (12 * M + 4 * S) / B
                work = {"kernel": "k_bkt_accum_g", "mads_per_item": acc, "sgpr_mads_per_item": acc * red / M, "step_mads_per_item": acc + front + reduce_,
                        "alg_bytes_per_item": 57 + 114 + 114}
                how = "buckets, 16-bit windows, %d additions per item" % pairs
            metric, unit, cfg = "Ed448 signatures/sec in whole-batch verification (one multi-scalar multiplication per 2^%d-item batch: %s)" % (a.batch_log2, how), "verifications/s", "f4"
            ref_what = "ec_verify_batch (EDDSA448: eddsa_verify_batch, no scratch pad)"
        else:
            cv = ctx.curve("WEI25519")
            if a.traffic_child:
                # the PMC passes only need the shape of the work: encodings that decode, S below q; the equation need not hold
                pubs, _ = cv.eddsa_sign_R(rb(64 * B))
                Renc, _ = cv.eddsa_sign_R(rb(64 * B))
                sg = np.empty((B, 64), dtype=np.uint8)
                sg[:, :32] = np.frombuffer(Renc, dtype=np.uint8).reshape(B, 32)
                sg[:, 32:] = rng.integers(0, 256, size=(B, 32), dtype=np.uint8)
                sg[:, 63] &= 0x0f
                sigs, hram, msgs = sg.tobytes(), rb(64 * B), b""
            else:
                seeds, msgs = rb(32 * B), rb(32 * B)
                hk = [hashlib.sha512(seeds[32 * i:32 * i + 32]).digest() for i in range(B)]
                a_np = np.frombuffer(b"".join(h[:32] for h in hk), dtype=np.uint8).reshape(B, 32).copy()
                a_np[:, 0] &= 248
                a_np[:, 31] &= 127
                a_np[:, 31] |= 64
                wide = np.zeros((B, 64), dtype=np.uint8)
                wide[:, :32] = a_np
                pubs, st = cv.eddsa_sign_R(wide.tobytes())
                assert set(st) == {0}
                r_hash = b"".join(hashlib.sha512(hk[i][32:] + msgs[32 * i:32 * i + 32]).digest() for i in range(B))
                Renc, st = cv.eddsa_sign_R(r_hash)
                assert set(st) == {0}
                hram = b"".join(hashlib.sha512(Renc[32 * i:32 * i + 32] + pubs[32 * i:32 * i + 32] + msgs[32 * i:32 * i + 32]).digest() for i in range(B))
                Sb = cv.eddsa_sign_S(r_hash, hram, a_np.tobytes())
                sg = np.empty((B, 64), dtype=np.uint8)
                sg[:, :32] = np.frombuffer(Renc, dtype=np.uint8).reshape(B, 32)
                sg[:, 32:] = np.frombuffer(Sb, dtype=np.uint8).reshape(B, 32)
                sigs = sg.tobytes()
                del hk, wide, sg
            ins = [t(pubs), t(sigs), t(hram)]
            bad_i = int(rng.integers(0, B))
            ctx.set_eddsa_msm(2, 0, 0)      # the multi-scalar form whatever the size

            def step():
                cv.eddsa_verify_all_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), d_res.data_ptr(), stream.cuda_stream)

            def msm_bad():
                pos = 64 * bad_i + 40
                ins[1][pos] ^= 1
                step()
                torch.cuda.synchronize()
                v = int(d_res.item())
                ins[1][pos] ^= 1
                return v, bad_i

            def ref_pieces(pieces):
                def one(lo, hi):
                    return all(O.ref_eddsa_verify_all(pubs[32 * l:32 * h], sigs[64 * l:64 * h], msgs[32 * l:32 * h], 32) for l, h in pieces[lo:hi])
                return all(O.in_slices(one, len(pieces)))
            K = max(1, min(8, B >> 16))
            M, S = 97, 61
            # k_edmsm_loop: per lane 64 windows of 3 doublings (3M + 4S), 1 doubling with T (4M + 4S) and one addition from B's table (8M),
            # shared by K items; per item 64 additions from A's table and 33 from R's, 8M each
            loop = (64 / K) * (13 * M + 16 * S + 8 * M) + 97 * 8 * M
            # k_edmsm_prep: two decodings (a square root each: 255 S + 25 M), [8]A (3 doublings), two window tables (49 M + 16 S each)
            prep = 2 * (255 * S + 25 * M) + 3 * (4 * M + 4 * S) + 2 * (49 * M + 16 * S)
            work = {"kernel": "k_edmsm_loop", "mads_per_item": loop, "sgpr_mads_per_item": loop * 16 / 97, "step_mads_per_item": loop + prep,
                    "alg_bytes_per_item": 32 + 64 + 64}
            how = "Straus, K = %d items per lane" % K
            algo = os.environ.get("ECAMD_ED_MSM_ALGO") or ("bucket" if B >= (1 << 18) else "straus")
            if algo == "bucket":
                # round 6, the bucket evaluation (ecamd_host_eddsa.cpp:eddsa_bkt_dev_locked): 16 windows of z h mod q, 8 of z, and a copy of B per 64
                # items with 16 windows: one addition with an affine precomputed operand (ed_madd: 7M) per pair in k_edbkt_accum; the step adds
                # the decoding (two square roots, the key's cofactor doublings, two precomputed entries of 3M), and the reduction -- 2^16
                # buckets per window, 2 unified additions (8M + the operand's conversion 1M) each, whatever the batch size
                pairs = 16 + 8 + 16 / 64
                acc = pairs * 7 * M
                front = 2 * (255 * S + 25 * M) + 3 * (4 * M + 4 * S) + 2 * 3 * M
                reduce_ = 16 * 65536 * 2 * 9 * M / B
                work = {"kernel": "k_edbkt_accum", "mads_per_item": acc, "sgpr_mads_per_item": acc * 16 / 97, "step_mads_per_item": acc + front + reduce_,
                        "alg_bytes_per_item": 32 + 64 + 64}
                how = "buckets, 16-bit windows, %.2f additions per item" % pairs
            metric, unit, cfg = "Ed25519 signatures/sec in whole-batch verification (one multi-scalar multiplication per 2^%d-item batch: %s)" % (a.batch_log2, how), "verifications/s", "f4"
            ref_what = "ec_verify_batch (EDDSA25519: eddsa_verify_batch, no scratch pad)"
    elif a.workload == "ed448_verify":
        cv = ctx.curve("WEI448")
        m = 128
        items = [O.ed448_sign(rb(57), rb(32)) for _ in range(m)]
        reps = B // m
        pubs = b"".join(i[0] for i in items) * reps
        sigs = b"".join(i[1] for i in items) * reps
        hram = bytearray(b"".join(i[2] for i in items) * reps)
        bad = np.zeros(B, dtype=np.uint8)
        for i in range(0, B, 10):
            hram[114 * i + (i % 114)] ^= 1 << (i % 8)
            bad[i] = 1
        hram = bytes(hram)
        ins = [t(pubs), t(sigs), t(hram)]
        d_res = torch.empty(B, dtype=torch.uint8, device=dev)

        def step():
            cv.eddsa_verify_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), d_res.data_ptr(), stream.cuda_stream, 114)
        expected = bad.tobytes()

        def oracle_subset(idx):
            o = O.Oracle("WEI448")
            return o.eddsa_verify(b"".join(pubs[57 * i:57 * i + 57] for i in idx), b"".join(sigs[114 * i:114 * i + 114] for i in idx),
                                  b"".join(hram[114 * i:114 * i + 114] for i in idx))
        metric, unit, cfg = "Ed448 verifications/sec (batch=2^%d, %d distinct signatures tiled)" % (a.batch_log2, m), "verifications/s", "4], Ed448 counterpart [not in BASELINE"
    else:
        x448 = a.workload == "x448"
        xw, xcurve = (56, "WEI448") if x448 else (32, "WEI25519")
        cv = ctx.curve(xcurve)
        k1, k2 = rb(xw * B), rb(xw * B)
        pub, st = cv.xdh(k1, (5 if x448 else 9).to_bytes(xw, "little") * B)   # peers' public keys: u on the curve
        assert set(st) == {0}
        ins = [t(k2), t(pub)]
        d_out = torch.empty(xw * B, dtype=torch.uint8, device=dev)
        d_res = torch.empty(B, dtype=torch.uint8, device=dev)

        def step():
            cv.xdh_dev(B, ins[0].data_ptr(), ins[1].data_ptr(), d_out.data_ptr(), d_res.data_ptr(), stream.cuda_stream)
        expected = bytes(B)

        def oracle_subset(idx):
            o = O.Oracle(xcurve)
            return o.xdh(b"".join(k2[xw * i:xw * i + xw] for i in idx), b"".join(pub[xw * i:xw * i + xw] for i in idx))
        out_w = xw

        def ref_subset(idx):
            sk, su = (b"".join(x[xw * i:xw * i + xw] for i in idx) for x in (k2, pub))
            return O.join_slices(O.in_slices(lambda lo, hi: O.ref_xdh(xw, sk[xw * lo:xw * hi], su[xw * lo:xw * hi]), len(idx)))
        if x448:
            # dominant kernel k_x448_ladder: 448 steps of 5 multiplications, 4 squarings and a24 e as sixteen MADs (round 3: a full
            # product) on the Goldilocks unit (16 limbs of 28 bits: M = 256, S = 136 MADs)
            work = {"kernel": "k_x448_ladder", "mads_per_item": 448 * (5 * 256 + 4 * 136 + 16) + 256, "sgpr_mads_per_item": 448 * 16}
            metric, unit, cfg = "X448 shared secrets/sec (batch=2^%d)" % a.batch_log2, "shared-secrets/s", "5], X448 counterpart [not in BASELINE"
        else:
            # dominant kernel k_x25519_ladder: 255 steps of 5 multiplications, 4 squarings and a24 e as nine MADs (round 3: a full
            # product); M = 81 + 16 = 97, S = 45 + 16 = 61 MADs (ecamd_u29g.h:mul_p25519)
            work = {"kernel": "k_x25519_ladder", "mads_per_item": 255 * (5 * 97 + 4 * 61 + 9) + 97, "sgpr_mads_per_item": 255 * (9 * 16 + 9)}
            # the whole step: k_xdh_prep_c25519 (the on-curve square root and the small-order doublings: 267 S + 35 M), the ladder,
            # k_x25519_fin (one inversion per 8 items: 32 S + 6 M per item)
            work["step_mads_per_item"] = work["mads_per_item"] + (35 + 6) * 97 + (267 + 32) * 61
            work["alg_bytes_per_item"] = 32 + 32 + 32 + 1
            metric, unit, cfg = "X25519 shared secrets/sec (batch=2^%d)" % a.batch_log2, "shared-secrets/s", 4
    gathered = torch.empty(world * d_res.numel(), dtype=torch.uint8, device=dev) if world > 1 else None

    def full_step():
        step()
        if world > 1:
            dist.all_gather_into_tensor(gathered, d_res)

    if a.traffic_child:
        for _ in range(a.warmup + a.steps):
            full_step()
        torch.cuda.synchronize()
        cv.free()
        ctx.close()
        return
    # ---- parity gate: the whole result against what the construction implies, 128 items against the oracle ----
    full_step()
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().tobytes()
    if res != expected:
        raise SystemExit("PARITY FAILURE: accept/reject bits differ from the construction of the batch")
    msm = a.workload in ("bip0340_msm", "ed25519_msm", "ed448_msm")
    if msm:
        v, where = msm_bad()
        if v != 1:
            raise SystemExit("PARITY FAILURE: the whole-batch form accepted a batch with a damaged item")
        full_step()
        torch.cuda.synchronize()
        if int(d_res.item()) != 0:
            raise SystemExit("PARITY FAILURE: the whole-batch form rejected the restored batch")
        gate = f"valid batch of 2^{a.batch_log2} accepted; rejected with item {where} damaged; accepted again once restored"
        if O.have_ref() and rank == 0 and a.ref_items > 0:
            # the unmodified reference's batch function on random contiguous pieces of 256 items of the same batch, one piece list per host thread
            nt = O.host_threads()
            npieces = max(nt, min(a.ref_items, B) // 256)
            starts = sorted(int(x) for x in np.random.default_rng(2).choice(max(1, B // 256), size=min(npieces, max(1, B // 256)), replace=False))
            pieces = [(256 * x, min(B, 256 * x + 256)) for x in starts]
            tr0 = time.time()
            if not ref_pieces(pieces):
                raise SystemExit("PARITY FAILURE: the unmodified reference's batch verifier rejects a piece of the batch the GPU accepted")
            el = time.time() - tr0
            items = sum(h - l for l, h in pieces)
            gate_ref = {"items": items, "seconds": el, "cores": nt, "what": ref_what}
            gate += f"; {len(pieces)} random pieces of 256 items ({items} items) accepted by the unmodified reference's {ref_what} on {nt} threads, {el:.1f} s"
    idx = [int(i) for i in np.random.default_rng(1).choice(B, size=128, replace=False)] if not msm else []
    exp = oracle_subset(idx) if not msm else None
    payload = a.workload in ("x25519", "x448", "ecdsa_sign", "ecccdh")
    if payload:
        out = d_out.cpu().numpy().tobytes()
        got = (b"".join(out[out_w * i:out_w * i + out_w] for i in idx), bytes(res[i] for i in idx))
    elif not msm:
        got = bytes(res[i] for i in idx)
    if not msm and got != exp:
        raise SystemExit("PARITY FAILURE: GPU output differs from the CPU oracle")
    if not msm:
        gate = "all accept/reject bits as constructed; 128 random items identical to the CPU oracle"
    if ref_subset is not None and O.have_ref() and rank == 0 and a.ref_items > 0:
        tg = time.time()
        ridx = [int(i) for i in np.sort(np.random.default_rng(2).choice(B, size=min(B, a.ref_items), replace=False))]
        tr0 = time.time()
        rexp = ref_subset(ridx)
        gate_ref = {"items": len(ridx), "seconds": time.time() - tr0, "cores": O.host_threads()}
        if payload:
            rgot = (b"".join(out[out_w * i:out_w * i + out_w] for i in ridx), bytes(res[i] for i in ridx))
        else:
            rgot = bytes(res[i] for i in ridx)
        if rgot != rexp:
            raise SystemExit("PARITY FAILURE: GPU output differs from the unmodified reference binary")
        gate += f"; {len(ridx)} random items identical to the unmodified reference (oracle/_ref) on {O.host_threads()} threads, {time.time() - tg:.1f} s"
    setup_s = time.time() - t_setup

    for _ in range(a.warmup):
        full_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        full_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    # roofline of the dominant kernel: one more step with the library's own HIP events around it (on the launch stream)
    roof = None
    if rank == 0 and work is not None:
        try:
            ctx.enable_kernel_timing(True)
            kms = []
            for _ in range(3):
                full_step()
                torch.cuda.synchronize()
                kms.append(ctx.dominant_kernel_ms())
            ctx.enable_kernel_timing(False)
            kernel_ms = float(np.mean(kms))
            pv, ps = a.mad_peak, a.mad_peak_sgpr
            if not pv:
                ub = json.loads(subprocess.run([os.path.join(ROOT, "libecc_amd", "lib", "ubench"), "2000"], capture_output=True, text=True, timeout=120).stdout)
                pv, ps = ub["v_mad_u64_u32"]["lane_ops_per_s"], ub.get("v_mad_u64_u32_sgpr", {}).get("lane_ops_per_s", 0.0)
            fs = work["sgpr_mads_per_item"] / work["mads_per_item"] if ps else 0.0
            peak = 1.0 / ((1.0 - fs) / pv + (fs / ps if ps else 0.0))     # operand-mix weighted stream (VGPR / SGPR multiplier)
            rate = B * work["mads_per_item"] / (kernel_ms * 1e-3)
            roof = {"bound": "valu-int-mad (v_mad_u64_u32 issue)", "kernel": work["kernel"], "kernel_ms": kernel_ms,
                    "kernel_mads_per_item": work["mads_per_item"], "sgpr_multiplier_share": fs, "achieved": rate / 1e9, "peak": peak / 1e9,
                    "unit": "GMAD/s (one GPU)", "frac": rate / peak, "peak_vgpr_stream": pv / 1e9, "peak_sgpr_stream": ps / 1e9,
                    "kernel_share_of_step": kernel_ms / (1e3 * elapsed / a.steps)}
            if work.get("step_mads_per_item"):
                step_ms = 1e3 * elapsed / a.steps
                roof["step_ms"] = step_ms
                roof["mads_per_item"] = work["step_mads_per_item"]
                roof["pipeline_frac"] = (B * work["step_mads_per_item"] / (step_ms * 1e-3)) / peak
                hb = B * work["alg_bytes_per_item"] / (step_ms * 1e-3)
                roof["hbm"] = {"achieved": hb / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": hb / 8e12,
                               "algorithmic_bytes_per_item": work["alg_bytes_per_item"]}
        except Exception as e:   # the timing hook only covers the fast paths
            roof = {"error": str(e)}
    cpu = None
    # HBM bytes per launch from PMC counters: two profiled child runs of this workload (tools/pmc.py), after the timed region
    if rank == 0 and world == 1 and a.traffic and isinstance(roof, dict) and "kernel" in roof:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import pmc
        tt = time.time()
        child = [sys.executable, os.path.abspath(__file__), "--workload", a.workload, "--curve", a.curve, "--batch-log2", str(a.batch_log2),
                 "--traffic-child", "--steps", "2", "--warmup", "1"]
        by_kernel, note = pmc.hbm_bytes_per_launch(child, timeout=300)
        roof["traffic_by_kernel"] = by_kernel
        dom = [v for k, v in (by_kernel or {}).items() if roof["kernel"].split("<")[0] in k]
        roof["traffic"] = max(dom) if dom else None
        roof["traffic_note"] = f"{note}; {time.time() - tt:.0f} s"
        if by_kernel and work.get("alg_bytes_per_item"):
            roof["step_traffic"] = sum(by_kernel.values())
            roof["traffic_over_algorithmic"] = roof["step_traffic"] / (B * work["alg_bytes_per_item"])
    if rank == 0 and world == 1 and not a.no_cpu_baseline and gate_ref and (gate_ref["seconds"] >= 3.0 or msm):
        # the parity gate already ran the unmodified reference over a random subset of this batch on every host thread: that run
        # IS the CPU baseline of the workload (ec_verify / x25519() of the reference beside configs 3-5)
        what = {"ecdsa_verify": "ec_pub_key_import_from_aff_buf + ec_verify (ECDSA)", "ecdsa_sign": "ec_sign (ECDSA, nonce supplied)",
                "ecccdh": "ecccdh_derive_secret", "ed25519_verify": "eddsa_import_pub_key + ec_verify (EDDSA25519)",
                "ed448_verify": "eddsa_import_pub_key + ec_verify (EDDSA448)", "x25519": "x25519()", "x448": "x448()",
                "bip0340_msm": gate_ref.get("what"), "ed25519_msm": gate_ref.get("what"), "ed448_msm": gate_ref.get("what")}[a.workload]
        cpu = {"value": gate_ref["items"] / gate_ref["seconds"], "unit": unit, "cores": gate_ref["cores"], "kind": "reference",
               "sample": f"the parity gate's own run: {gate_ref['items']} random items of the same batch through {what} of the unmodified "
                         f"reference (oracle/_ref) on {gate_ref['cores']} threads, {gate_ref['seconds']:.1f} s wall"}
    elif rank == 0 and world == 1 and not a.no_cpu_baseline and O.have_ref() and not msm:
        # the unmodified reference on this host, one thread, on a bounded sample of the same inputs
        m = 1536 if a.workload != "x25519" else 3072
        if a.workload == "x448":
            m = 512
        t0 = time.time()
        if a.workload == "ecdsa_verify":
            # ec_verify hashes the message itself: time it on messages of the digest's length (SHA-256 of 32 bytes
            # is noise next to the two scalar multiplications); accept bits are not compared here
            O.RefLib(curve).ecdsa_verify(hname, pubs[:2 * cl * m], sigs[:2 * ql * m], msgs[:32 * m], 32)
            what = "ec_pub_key_import_from_aff_buf + ec_verify (ECDSA, SHA-256 over 32-byte messages)"
        elif a.workload == "ecdsa_sign":
            O.RefLib(curve).ecdsa_sign("SHA256", privs[:32 * m], other[:32 * m], dg[:32 * m], 32)
            what = "ec_key_pair_import_from_priv_key_buf + ec_sign (ECDSA, SHA-256 over 32-byte messages, nonce supplied)"
        elif a.workload == "ecccdh":
            O.RefLib(curve).ecccdh(privs[:32 * m], peers[:64 * m])
            what = "ecccdh_derive_secret"
        elif a.workload == "ed25519_verify":
            O.ref_ed25519_verify(pubs[:32 * m], sigs[:64 * m], msgs[:32 * m], 32)
            what = "eddsa_import_pub_key + ec_verify (EDDSA25519, 32-byte messages)"
        elif a.workload == "ed448_verify":
            m = 256
            O.ref_ed448_verify(pubs[:57 * m], sigs[:114 * m], hram[:114 * m], 114)
            what = "eddsa_import_pub_key + ec_verify (EDDSA448, SHAKE256 over 114-byte messages)"
        else:
            O.ref_xdh(xw, k2[:xw * m], pub[:xw * m])
            what = "x448()" if x448 else "x25519()"
        el = time.time() - t0
        cpu = {"value": m / el, "unit": unit, "cores": 1, "kind": "reference",
               "sample": f"first {m} items of the same batch through {what} of the unmodified reference (oracle/_ref), "
                         f"1 thread, {el:.1f} s"}
    if rank == 0:
        print(json.dumps({
            "metric": metric, "value": B * world * a.steps / elapsed, "unit": unit, "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32 (%d-bit limbs, v_mad_u64_u32 integer MAD, u64 accumulators)" % (28 if a.workload in ("x448", "ed448_verify", "ed448_msm") else 29),
            "data": ("synthetic (seeded), inputs resident in HBM; every signature valid (the form vouches for valid batches)" if msm else
                     "synthetic (seeded), inputs resident in HBM; 10 % of the signatures corrupted") if not payload
                    else "synthetic (seeded), inputs resident in HBM; valid keys",
            "config": {"workload": (f"{a.workload} (SURVEY.md section 8 row f4), batch 2^{a.batch_log2} per GPU" if msm else
                                    f"{a.workload} (BASELINE.json configs[{cfg}]), batch 2^{a.batch_log2} per GPU"),
                       "sharding": "contiguous per-rank shards" + (", RCCL all_gather of result bytes per step" if world > 1 else ""),
                       "parity_gate": gate},
            "roofline": roof, "cpu_baseline": cpu, "setup_s": setup_s}))
    cv.free()
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
