"""GPU tests of batched ECDSA public-key recovery (ec_ecdsa_recover_batch / _dev) against the unmodified reference's
ecdsa_public_key_from_sig: the recorded verdicts of tests/golden/ecdsa_recover.json item for item and byte for byte, random
batches checked against the reference at run time, a chunked 2^20-item batch, the round trip through verification, the redo
items among ordinary ones, and secret-scalar mode."""
import json
import os

import numpy as np
import pytest

import oracles as O
import recover_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR, INF = RR.ECAMD_OK, RR.ECAMD_ERR, RR.ECAMD_INF


def fixture_arrays(curve, items):
    """items of one digest length -> (sigs, digests, hlen, expected (pub1, pub2, st1, st2))"""
    cl = O.clen(curve)
    zero = bytes(2 * cl)
    sigs = b"".join(bytes.fromhex(i["sig"]) for i in items)
    dgs = b"".join(bytes.fromhex(i["digest"]) for i in items)

    def key(i, k):
        if i["ret"] != 0:
            return zero, ERR
        return (zero, INF) if i[k] == "infinity" else (bytes.fromhex(i[k]), OK)
    k1, k2 = [key(i, "key1") for i in items], [key(i, "key2") for i in items]
    exp = (b"".join(k[0] for k in k1), b"".join(k[0] for k in k2), bytes(k[1] for k in k1), bytes(k[1] for k in k2))
    return sigs, dgs, len(dgs) // len(items), exp


def by_digest_len(items):
    groups = {}
    for i in items:
        groups.setdefault(len(i["digest"]) // 2, []).append(i)
    return groups


def recover_dev(cv, curve, sigs, dgs, hlen, stream=None):
    """the _dev form on torch buffers: the same four byte strings as Curve.ecdsa_recover"""
    import torch
    dev = torch.device("cuda:0")
    n = len(sigs) // (2 * O.qlen(curve))
    cl = O.clen(curve)
    stream = stream or torch.cuda.Stream(device=dev)
    ds = torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to(dev)
    dd = torch.frombuffer(bytearray(dgs), dtype=torch.uint8).to(dev)
    outs = [torch.full((m,), 0xAA, dtype=torch.uint8, device=dev) for m in (2 * cl * n, 2 * cl * n, n, n)]
    torch.cuda.synchronize()
    cv.ecdsa_recover_dev(n, ds.data_ptr(), dd.data_ptr(), hlen, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                         outs[3].data_ptr(), stream.cuda_stream)
    stream.synchronize()   # the _dev form only enqueues
    return tuple(bytes(o.cpu().numpy()) for o in outs)


def first_difference(got, exp, curve):
    cl = O.clen(curve)
    for i in range(len(exp[2])):
        g = (got[0][2 * cl * i:2 * cl * (i + 1)], got[1][2 * cl * i:2 * cl * (i + 1)], got[2][i], got[3][i])
        e = (exp[0][2 * cl * i:2 * cl * (i + 1)], exp[1][2 * cl * i:2 * cl * (i + 1)], exp[2][i], exp[3][i])
        if g != e:
            return "item %d: got status (%d, %d), the reference (%d, %d)" % (i, g[2], g[3], e[2], e[3])
    return None


@pytest.mark.parametrize("curve", RR.CURVES)
def test_fixture_item_for_item(gpu_ctx, curve):
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_recover.json")) as f:
        items = json.load(f)[curve]
    cv = gpu_ctx.curve(curve)
    try:
        seen = 0
        for hlen, group in sorted(by_digest_len(items).items()):
            sigs, dgs, hl, exp = fixture_arrays(curve, group)
            assert hl == hlen
            got = cv.ecdsa_recover(sigs, dgs, hlen)
            assert got == exp, first_difference(got, exp, curve)
            got = recover_dev(cv, curve, sigs, dgs, hlen)
            assert got == exp, first_difference(got, exp, curve)
            seen += len(group)
        assert seen == len(items)   # every item of the fixture went through both forms
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["BRAINPOOLP256R1", "SECP224K1", "SECP384R1"])
def test_fixture_on_a_handle_from_params(gpu_ctx, curve):
    """the same golden items on an ecamd_curve_from_params handle (its own square-root constants and order slot), first on a fresh
    handle with a batch too small for a comb table of the generator (fixed-base fallback), then on a batch that builds one"""
    import libecc_amd
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_recover.json")) as f:
        items = json.load(f)[curve]
    cv = libecc_amd.Curve(gpu_ctx, params=O.CURVES[curve])
    try:
        seen = 0
        for hlen, group in sorted(by_digest_len(items).items(), key=lambda g: len(g[1])):   # smallest group first
            for rep in (1, 4):
                sigs, dgs, hl, exp = fixture_arrays(curve, group * rep)
                got = cv.ecdsa_recover(sigs, dgs, hlen)
                assert got == exp, first_difference(got, exp, curve)
            got = recover_dev(cv, curve, sigs, dgs, hlen)
            assert got == exp, first_difference(got, exp, curve)
            seen += len(group)
        assert seen == len(items)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", RR.CURVES)
def test_random_batch_against_the_reference(gpu_ctx, curve):
    """half honest signatures (ec_ecdsa_sign_batch), half with a random r -- about half of those are no abscissa"""
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    n = 1 << (11 if curve in ("SECP384R1", "SECP521R1") else 14)
    rng = np.random.default_rng(8100 + RR.CURVES.index(curve))
    cl, ql = O.clen(curve), O.qlen(curve)
    cv = gpu_ctx.curve(curve)
    try:
        sigs, dgs, privs = RR.random_batch(curve, n, rng, lambda x, k, d: cv.ecdsa_sign(x, k, d, 32))
        pubs, st = cv.scalar_mult(privs)
        assert st == bytes(n // 2)
        got = cv.ecdsa_recover(sigs, dgs, 32)
        exp = RR.ref_recover_threaded(curve, sigs, dgs, 32)
        assert got == exp, first_difference(got, exp, curve)
        errs = sum(s == ERR for s in got[2][n // 2:])
        assert n // 8 < errs < 7 * n // 16, errs     # a random r is no abscissa about half the time
        if curve in RR.PRIME_ORDER:
            for i in range(n // 2):
                signer = pubs[2 * cl * i:2 * cl * (i + 1)]
                assert got[2][i] == OK and got[3][i] == OK
                assert signer in (got[0][2 * cl * i:2 * cl * (i + 1)], got[1][2 * cl * i:2 * cl * (i + 1)]), i
    finally:
        cv.free()


def k256_batch(cv, n, rng):
    """n honest secp256k1 signatures with numpy-made scalars in [1, 2^255): (sigs, digests, signers' keys)"""
    def scalars():
        a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        a[:, 0] &= 0x7F
        a[:, 31] |= 1
        return a.tobytes()
    privs, nonces, dgs = scalars(), scalars(), rng.integers(0, 256, size=32 * n, dtype=np.uint8).tobytes()
    sigs, st = cv.ecdsa_sign(privs, nonces, dgs, 32)
    assert st == bytes(n)
    pubs, st = cv.scalar_mult(privs)
    assert st == bytes(n)
    return sigs, dgs, pubs


def test_large_batch_in_chunks(gpu_ctx):
    """2^20 secp256k1 items with max_chunk below n: a seeded 2^14-item sample and the crafted edge items placed on the chunk
    boundaries against the reference, every honest item against its signer"""
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    curve, n, chunk = "SECP256K1", 1 << 20, 300000
    rng = np.random.default_rng(8200)
    cv = gpu_ctx.curve(curve)
    try:
        sigs, dgs, pubs = k256_batch(cv, n, rng)
        sigs, dgs = bytearray(sigs), bytearray(dgs)
        with open(os.path.join(ROOT, "tests", "golden", "ecdsa_recover.json")) as f:
            short = [i for i in json.load(f)[curve] if len(i["digest"]) == 64]
        edge = [i for fam in ("redo", "not_abscissa", "e_zero", "range") for i in [x for x in short if x["family"] == fam][:4]]
        places = [c * chunk + d for c in (1, 2, 3) for d in (-2, -1, 0, 1)] + [0, n - 1]
        placed = {}
        assert len(edge) >= len(places)
        for pos, item in zip(places, edge):
            sigs[64 * pos:64 * pos + 64] = bytes.fromhex(item["sig"])
            dgs[32 * pos:32 * pos + 32] = bytes.fromhex(item["digest"])
            placed[pos] = item
        assert len(placed) == len(places) and {i["family"] for i in placed.values()} >= {"not_abscissa", "range", "redo"}
        sigs, dgs = bytes(sigs), bytes(dgs)
        gpu_ctx.set_max_chunk(chunk)
        try:
            got = recover_dev(cv, curve, sigs, dgs, 32)
        finally:
            gpu_ctx.set_max_chunk(1 << 20)
        # every item that was not overwritten is an honest signature: both keys finite, the signer among them
        g1, g2 = np.frombuffer(got[0], dtype=np.uint8).reshape(n, 64), np.frombuffer(got[1], dtype=np.uint8).reshape(n, 64)
        pk = np.frombuffer(pubs, dtype=np.uint8).reshape(n, 64)
        hit = (g1 == pk).all(axis=1) | (g2 == pk).all(axis=1)
        st1, st2 = np.frombuffer(got[2], dtype=np.uint8), np.frombuffer(got[3], dtype=np.uint8)
        honest = np.ones(n, dtype=bool)
        honest[list(placed)] = False
        assert hit[honest].all() and (st1[honest] == OK).all() and (st2[honest] == OK).all()
        # the reference on a seeded sample and on the placed items
        idx = sorted(set(int(i) for i in np.random.default_rng(8201).choice(n, size=1 << 14, replace=False)) | set(placed))
        ss, sd = b"".join(sigs[64 * i:64 * i + 64] for i in idx), b"".join(dgs[32 * i:32 * i + 32] for i in idx)
        exp = RR.ref_recover_threaded(curve, ss, sd, 32)
        sub = (b"".join(got[0][64 * i:64 * i + 64] for i in idx), b"".join(got[1][64 * i:64 * i + 64] for i in idx),
               bytes(got[2][i] for i in idx), bytes(got[3][i] for i in idx))
        assert sub == exp, first_difference(sub, exp, curve)
        for pos, item in placed.items():
            if item["family"] in ("not_abscissa", "range") and item["ret"] == -1:
                assert got[2][pos] == ERR and got[3][pos] == ERR
            if item["family"] == "redo":
                assert sorted((got[2][pos], got[3][pos])) == [OK, INF]
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP384R1"])
def test_recovered_signer_key_verifies(gpu_ctx, curve):
    rng = np.random.default_rng(8300)
    n, cl = 512, O.clen(curve)
    cv = gpu_ctx.curve(curve)
    try:
        sigs, dgs, privs = RR.random_batch(curve, 2 * n, rng, lambda x, k, d: cv.ecdsa_sign(x, k, d, 32))
        sigs, dgs = sigs[:2 * O.qlen(curve) * n], dgs[:32 * n]    # the honest half
        pubs, st = cv.scalar_mult(privs)
        assert st == bytes(n)
        p1, p2, s1, s2 = cv.ecdsa_recover(sigs, dgs, 32)
        keys = []
        for i in range(n):
            signer = pubs[2 * cl * i:2 * cl * (i + 1)]
            cands = [k for k, s in ((p1[2 * cl * i:2 * cl * (i + 1)], s1[i]), (p2[2 * cl * i:2 * cl * (i + 1)], s2[i])) if s == OK and k == signer]
            assert cands, i            # prime order: the signer is always one of the two
            keys.append(cands[0])
        assert cv.ecdsa_verify(b"".join(keys), sigs, dgs, 32) == bytes(n)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "BRAINPOOLP256R1", "WEI25519"])
def test_redo_items_among_ordinary_ones(gpu_ctx, curve):
    """a lane marked for the redo pass sits among fast-path lanes (and inside a group that shares one inversion)"""
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_recover.json")) as f:
        items = [i for i in json.load(f)[curve] if len(i["digest"]) == 64]
    redo = [i for i in items if i["family"] == "redo"]
    other = [i for i in items if i["family"] != "redo"]
    assert redo and other
    rng = np.random.default_rng(8400)
    n = 4096
    batch = [other[int(k)] for k in rng.integers(0, len(other), size=n)]
    where = sorted(int(k) for k in rng.choice(n, size=97, replace=False)) + [0, 7, 8, n - 1]
    for j, pos in enumerate(where):
        batch[pos] = redo[j % len(redo)]
    sigs, dgs, hlen, exp = fixture_arrays(curve, batch)
    cv = gpu_ctx.curve(curve)
    try:
        got = cv.ecdsa_recover(sigs, dgs, hlen)
        assert got == exp, first_difference(got, exp, curve)
        assert sum(s == INF for s in got[2]) + sum(s == INF for s in got[3]) == len(set(where))
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP521R1"])
def test_secret_scalar_mode_gives_the_same_bytes(gpu_ctx, curve):
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_recover.json")) as f:
        items = [i for i in json.load(f)[curve] if len(i["digest"]) == 64]
    sigs, dgs, hlen, exp = fixture_arrays(curve, items * 3)
    cv = gpu_ctx.curve(curve)
    try:
        gpu_ctx.set_secret_scalars(True)
        try:
            got = cv.ecdsa_recover(sigs, dgs, hlen)
        finally:
            gpu_ctx.set_secret_scalars(False)
        assert got == exp, first_difference(got, exp, curve)
        assert cv.ecdsa_recover(sigs, dgs, hlen) == exp
    finally:
        cv.free()
