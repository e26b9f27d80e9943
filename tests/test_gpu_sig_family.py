"""GPU tests of batched ECGDSA / ECRDSA / SM2 (ec_sig_verify_batch / ec_sig_sign_batch and their _dev forms): the recorded
reference answers of tests/golden/sig_family.json item for item through both forms on every curve and scheme, the same on an
ecamd_curve_from_params handle, random batches against the reference at run time, the sign -> verify round trip at 2^16, a
chunked 2^20-item batch with edge items on the chunk boundaries, redo items among ordinary ones, secret-scalar mode, and an
ECDSA signature offered under each of the three schemes."""
import json
import os

import numpy as np
import pytest

import oracles as O
import sigfam_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGS = sorted(S.SCHEMES.items())


_FIXTURE = []


def load(curve):
    if not _FIXTURE:
        _FIXTURE.append(S.load_fixture(os.path.join(ROOT, "tests", "golden", "sig_family.json")))
    return _FIXTURE[0][curve]


def by_digest_len(items):
    groups = {}
    for i in items:
        groups.setdefault(len(i["digest"]) // 2, []).append(i)
    return groups


def verify_arrays(items):
    return (b"".join(bytes.fromhex(i["pub"]) for i in items), b"".join(bytes.fromhex(i["sig"]) for i in items),
            b"".join(bytes.fromhex(i["digest"]) for i in items), bytes(0 if i["ret"] == 0 else 1 for i in items))


def sign_arrays(curve, items):
    """items whose x and k fit the qlen bytes of the interface (q + 1 may not where q is just below 2^(8 qlen): the all-ones
    value stands in, as out of range as q + 1)"""
    ql = O.qlen(curve)
    top = (1 << (8 * ql)) - 1
    xs = b"".join(min(int(i["x"], 16), top).to_bytes(ql, "big") for i in items)
    ks = b"".join(min(int(i["k"], 16), top).to_bytes(ql, "big") for i in items)
    sigs = b"".join(bytes.fromhex(i["sig"]) if i["ret"] == 0 else bytes(2 * ql) for i in items)
    return xs, ks, b"".join(bytes.fromhex(i["digest"]) for i in items), sigs, bytes(0 if i["ret"] == 0 else 1 for i in items)


def verify_dev(cv, alg, pubs, sigs, dgs, hlen):
    import torch
    dev = torch.device("cuda:0")
    n = len(pubs) // (2 * cv.clen)
    stream = torch.cuda.Stream(device=dev)
    bufs = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (pubs, sigs, dgs)]
    res = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cv.sig_verify_dev(alg, n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), hlen, res.data_ptr(), stream.cuda_stream)
    stream.synchronize()   # the _dev form only enqueues
    return bytes(res.cpu().numpy())


def sign_dev(cv, alg, xs, ks, dgs, hlen):
    import torch
    dev = torch.device("cuda:0")
    n = len(xs) // cv.qlen
    stream = torch.cuda.Stream(device=dev)
    bufs = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (xs, ks, dgs)]
    sig = torch.full((2 * cv.qlen * n,), 0xAA, dtype=torch.uint8, device=dev)
    st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cv.sig_sign_dev(alg, n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), hlen, sig.data_ptr(), st.data_ptr(),
                    stream.cuda_stream)
    stream.synchronize()
    return bytes(sig.cpu().numpy()), bytes(st.cpu().numpy())


def mismatch(got, exp, items):
    bad = [(k, items[k]["family"], got[k], exp[k]) for k in range(len(exp)) if got[k] != exp[k]]
    return "items (index, family, got, reference): %r" % (bad[:8],)


def run_fixture(cv, curve, reps=(1,)):
    fx = load(curve)
    for name, alg in ALGS:
        seen = 0
        for hlen, group in sorted(by_digest_len(fx[name]["verify"]).items(), key=lambda g: len(g[1])):
            for rep in reps:
                items = group * rep
                pubs, sigs, dgs, exp = verify_arrays(items)
                got = cv.sig_verify(alg, pubs, sigs, dgs, hlen)
                assert got == exp, (curve, name, hlen, mismatch(got, exp, items))
            got = verify_dev(cv, alg, pubs, sigs, dgs, hlen)
            assert got == exp, (curve, name, hlen, "dev", mismatch(got, exp, items))
            seen += len(group)
        assert seen == len(fx[name]["verify"])
        seen = 0
        for hlen, group in sorted(by_digest_len(fx[name]["sign"]).items()):
            xs, ks, dgs, sigs, st = sign_arrays(curve, group)
            assert cv.sig_sign(alg, xs, ks, dgs, hlen) == (sigs, st), (curve, name, hlen)
            assert sign_dev(cv, alg, xs, ks, dgs, hlen) == (sigs, st), (curve, name, hlen, "dev")
            seen += len(group)
        assert seen == len(fx[name]["sign"])


@pytest.mark.parametrize("curve", S.CURVES)
def test_fixture_item_for_item(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    try:
        run_fixture(cv, curve)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["BRAINPOOLP256R1", "SECP224K1", "SECP384R1"])
def test_fixture_on_a_handle_from_params(gpu_ctx, curve):
    """a fresh ecamd_curve_from_params handle: first batches too small for a comb table of the generator (the two-multiplication
    path), then batches that build it (the fused loop)"""
    import libecc_amd
    cv = libecc_amd.Curve(gpu_ctx, params=O.CURVES[curve])
    try:
        run_fixture(cv, curve, reps=(1, 8))
    finally:
        cv.free()


@pytest.mark.parametrize("curve", S.CURVES)
def test_random_batch_against_the_reference(gpu_ctx, curve):
    """half honest (made by ec_sig_sign_batch), half random (r, s): the honest half is accepted entirely, and every verdict is the
    reference's"""
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    cv = gpu_ctx.curve(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    n = 96
    try:
        for name, alg in ALGS:
            rng = np.random.default_rng(9100 + alg)
            pubs, sigs, dgs, msgs = S.random_batch(curve, alg, n, rng, lambda x, k, d, h: cv.sig_sign(alg, x, k, d, h))
            got = cv.sig_verify(alg, pubs, sigs, dgs, 32)
            assert got[:n // 2] == bytes(n // 2), (curve, name, "an honest signature was rejected")
            ref = bytes(0 if S.ref_verify(curve, alg, "SHA256", pubs[2 * cl * i:2 * cl * (i + 1)], sigs[2 * ql * i:2 * ql * (i + 1)],
                                          msgs[i]) == 0 else 1 for i in range(n))
            assert got == ref, (curve, name)
            print(curve, name, "accepted", got.count(0), "of", n)
            # the signatures themselves are the reference's for the same nonces: sign a few again there
            for i in range(4):
                x = int.from_bytes(rng.integers(0, 256, size=ql, dtype=np.uint8).tobytes(), "big") % (O.CURVES[curve]["q"] - 2) + 1
                k = int.from_bytes(rng.integers(0, 256, size=ql, dtype=np.uint8).tobytes(), "big") % (O.CURVES[curve]["q"] - 1) + 1
                pub = S.pt_bytes(curve, S.pub_point(curve, alg, x))
                ret, rsig = S.ref_sign(curve, alg, "SHA512", x, k, msgs[i])
                gsig, gst = cv.sig_sign(alg, x.to_bytes(ql, "big"), k.to_bytes(ql, "big"), S.digest_for(curve, alg, "SHA512", pub, msgs[i]), 64)
                assert (ret, rsig) == (0, gsig) and gst == b"\0", (curve, name)
    finally:
        cv.free()


def random_signed(cv, curve, alg, n, seed, hlen=32):
    """n random (x, k, digest) signed on the device, with the public keys from the device's own fixed-base multiplication"""
    q = O.CURVES[curve]["q"]
    ql = O.qlen(curve)
    rng = np.random.default_rng(seed)

    def scalars(lo_excl_top):
        raw = rng.integers(0, 256, size=(n, ql + 8), dtype=np.uint8)
        return [1 + int.from_bytes(row.tobytes(), "big") % lo_excl_top for row in raw]
    xs, ks = scalars(q - 2), scalars(q - 1)
    dgs = rng.integers(0, 256, size=hlen * n, dtype=np.uint8).tobytes()
    xb = b"".join(x.to_bytes(ql, "big") for x in xs)
    kb = b"".join(k.to_bytes(ql, "big") for k in ks)
    keysc = b"".join(pow(x, -1, q).to_bytes(ql, "big") for x in xs) if alg == S.ECGDSA else xb
    pubs, st = cv.scalar_mult(keysc)
    assert st == bytes(n)
    sigs, sst = cv.sig_sign(alg, xb, kb, dgs, hlen)
    return pubs, sigs, sst, dgs, xb, kb


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP384R1", "WEI25519"])
def test_sign_verify_round_trip(gpu_ctx, curve):
    """2^16 signatures per scheme verify; with the top bit of the digest changed none does (the top bit: ECGDSA drops the low
    bits of a digest longer than q).  (The digests are random bytes: for SM2 they stand for H(Z || m), which the entry points
    never look into.)"""
    cv = gpu_ctx.curve(curve)
    n = 1 << 16
    try:
        for name, alg in ALGS:
            pubs, sigs, sst, dgs, _, _ = random_signed(cv, curve, alg, n, 9200 + alg)
            assert sst == bytes(n), (curve, name)
            assert cv.sig_verify(alg, pubs, sigs, dgs, 32) == bytes(n), (curve, name)
            bad = bytearray(dgs)
            for i in range(n):
                bad[32 * i] ^= 0x80
            assert cv.sig_verify(alg, pubs, sigs, bytes(bad), 32) == b"\1" * n, (curve, name)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1"])
def test_large_batch_in_chunks(gpu_ctx, curve):
    """2^20 items with max_chunk below n: a signed 2^14-item block repeated, with the fixture's items (every family) laid over the
    chunk boundaries; the verdicts are those of the unchunked small calls"""
    cv = gpu_ctx.curve(curve)
    n, block, chunk = 1 << 20, 1 << 14, 300000
    cl, ql = O.clen(curve), O.qlen(curve)
    fx = load(curve)
    try:
        for name, alg in ALGS:
            pubs, sigs, sst, dgs, _, _ = random_signed(cv, curve, alg, block, 9300 + alg)
            assert sst == bytes(block)
            reps = n // block
            P, Sg, D, exp = bytearray(pubs * reps), bytearray(sigs * reps), bytearray(dgs * reps), bytearray(n)
            items = [i for i in fx[name]["verify"] if len(i["digest"]) == 64]
            assert {i["family"] for i in items} >= {"honest", "range", "w_infinity", "equal_operands", "key_not_importable"}
            pos = chunk - len(items) // 2
            for b in range(1, 4):
                for j, it in enumerate(items):
                    k = b * chunk - len(items) // 2 + j
                    P[2 * cl * k:2 * cl * (k + 1)] = bytes.fromhex(it["pub"])
                    Sg[2 * ql * k:2 * ql * (k + 1)] = bytes.fromhex(it["sig"])
                    D[32 * k:32 * (k + 1)] = bytes.fromhex(it["digest"])
                    exp[k] = 0 if it["ret"] == 0 else 1
            assert pos > 0
            gpu_ctx.set_max_chunk(chunk)
            try:
                got = cv.sig_verify(alg, bytes(P), bytes(Sg), bytes(D), 32)
                gdev = verify_dev(cv, alg, bytes(P), bytes(Sg), bytes(D), 32)
            finally:
                gpu_ctx.set_max_chunk(1 << 20)
            assert got == bytes(exp), (curve, name, [k for k in range(n) if got[k] != exp[k]][:8])
            assert gdev == bytes(exp), (curve, name, "dev")
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP521R1"])
def test_redo_items_among_ordinary_ones(gpu_ctx, curve):
    """the items whose loop meets [u]G = +-[v]Y (w_infinity, opposite_operands, equal_operands) scattered in a batch large enough
    for the interleaved / fused loops"""
    cv = gpu_ctx.curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    fx = load(curve)
    n = 1 << 13
    try:
        for name, alg in ALGS:
            pubs, sigs, sst, dgs, _, _ = random_signed(cv, curve, alg, n, 9400 + alg)
            P, Sg, D, exp = bytearray(pubs), bytearray(sigs), bytearray(dgs), bytearray(n)
            items = [i for i in fx[name]["verify"] if i["family"] in ("w_infinity", "opposite_operands", "equal_operands")
                     and len(i["digest"]) == 64]
            assert len(items) >= 2
            for j, it in enumerate(items * 5):
                k = (j * 1237 + 11) % n
                P[2 * cl * k:2 * cl * (k + 1)] = bytes.fromhex(it["pub"])
                Sg[2 * ql * k:2 * ql * (k + 1)] = bytes.fromhex(it["sig"])
                D[32 * k:32 * (k + 1)] = bytes.fromhex(it["digest"])
                exp[k] = 0 if it["ret"] == 0 else 1
            got = cv.sig_verify(alg, bytes(P), bytes(Sg), bytes(D), 32)
            assert got == bytes(exp), (curve, name, [k for k in range(n) if got[k] != exp[k]][:8])
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1"])
def test_secret_scalar_mode_gives_the_same_bytes(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    n = 1 << 12
    try:
        for name, alg in ALGS:
            pubs, sigs, sst, dgs, xb, kb = random_signed(cv, curve, alg, n, 9500 + alg)
            gpu_ctx.set_secret_scalars(True)
            try:
                assert cv.sig_sign(alg, xb, kb, dgs, 32) == (sigs, sst), (curve, name)
                assert cv.sig_verify(alg, pubs, sigs, dgs, 32) == bytes(n), (curve, name)
            finally:
                gpu_ctx.set_secret_scalars(False)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1"])
def test_an_ecdsa_signature_is_no_signature_of_the_family(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    n = 512
    rng = np.random.default_rng(9600)
    try:
        xs = b"".join((1 + S.rand_int(rng, q - 2)).to_bytes(ql, "big") for _ in range(n))
        ks = b"".join((1 + S.rand_int(rng, q - 1)).to_bytes(ql, "big") for _ in range(n))
        dgs = rng.integers(0, 256, size=32 * n, dtype=np.uint8).tobytes()
        pubs, st = cv.scalar_mult(xs)
        sigs, sst = cv.ecdsa_sign(xs, ks, dgs, 32)
        assert st == bytes(n) and sst == bytes(n)
        assert cv.ecdsa_verify(pubs, sigs, dgs, 32) == bytes(n)
        for name, alg in ALGS:
            assert cv.sig_verify(alg, pubs, sigs, dgs, 32) == b"\1" * n, (curve, name)
    finally:
        cv.free()


def test_argument_errors_and_empty_batches(gpu_ctx):
    import libecc_amd
    cv = gpu_ctx.curve("SECP256R1")
    try:
        for alg in (S.ECGDSA, S.ECRDSA, S.SM2):
            assert cv.sig_verify(alg, b"", b"", b"", 32) == b""
            assert cv.sig_sign(alg, b"", b"", b"", 32) == (b"", b"")
            for hlen in (0, 129):
                with pytest.raises(libecc_amd.EcamdError):
                    cv.sig_verify(alg, bytes(64), bytes(64), bytes(max(hlen, 1)), hlen)
        for alg in (0, 1, 5, 9):   # ECDSA's own number included: it has its own entry points
            with pytest.raises(libecc_amd.EcamdError):
                cv.sig_verify(alg, bytes(64), bytes(64), bytes(32), 32)
            with pytest.raises(libecc_amd.EcamdError):
                cv.sig_sign(alg, bytes(32), bytes(32), bytes(32), 32)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256K1"])
def test_sign_in_pieces_of_max_chunk(gpu_ctx, curve):
    """ec_sig_sign_batch and its _dev form with n above max_chunk: max_chunk 64 and n = 130 (three pieces, the last of two items, n a
    multiple of neither 8 nor 64) give the bytes and status of the one-piece call, which are the reference's recorded answers, with an
    item the reference refuses to sign at 63, 64 (the two sides of a boundary) and 129 (last)"""
    cv = gpu_ctx.curve(curve)
    fx = load(curve)
    n, at = 130, (63, 64, 129)
    try:
        for name, alg in ALGS:
            hlen, group = max(sorted(by_digest_len(fx[name]["sign"]).items()), key=lambda g: len(g[1]))
            good = [i for i in group if i["ret"] == 0]
            bad = next(i for i in group if i["ret"] != 0)
            assert len(good) >= 2
            items = [good[i % len(good)] for i in range(n)]
            for k in at:
                items[k] = bad
            xs, ks, dgs, sigs, st = sign_arrays(curve, items)
            assert [i for i in range(n) if st[i] != 0] == list(at)
            whole = cv.sig_sign(alg, xs, ks, dgs, hlen)
            gpu_ctx.set_max_chunk(64)
            try:
                pieces = cv.sig_sign(alg, xs, ks, dgs, hlen)
                pdev = sign_dev(cv, alg, xs, ks, dgs, hlen)
            finally:
                gpu_ctx.set_max_chunk(1 << 20)
            assert whole == (sigs, st), (curve, name, "one piece against the recorded reference answers")
            assert pieces == whole, (curve, name, "three pieces against one")
            assert pdev == whole, (curve, name, "three pieces against one, dev")
    finally:
        cv.free()
