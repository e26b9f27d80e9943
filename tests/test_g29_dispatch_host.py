"""CPU test of libecc_amd/csrc/ecamd_g29_dispatch.cpp ITSELF: the file is compiled for the host beside tests/g29_dispatch_host_shim.cpp,
whose per-unit entry points are stubs that record their own name.  The program calls every dispatcher for every (|p|, flavour) pair of
PBITS x FLAVOURS and prints where the call went; this test holds that against the routing rule WRITTEN OUT below (the seven flavoured
pairs, else the dense unit of the size, else hipErrorInvalidValue) and the geometry functions against their formulas restated in
Python.  The same program is built and run once more with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SOURCES = [os.path.join(ROOT, "tests", "g29_dispatch_host_shim.cpp"), os.path.join(ROOT, "libecc_amd", "csrc", "ecamd_g29_dispatch.cpp")]

PBITS = [0, 160, 191, 192, 224, 255, 256, 257, 320, 384, 448, 511, 512, 521, 522]
FLAVOURS = list(range(-1, 9))
DENSE = [192, 224, 255, 256, 320, 384, 448, 511, 512, 521]
FLAVOURED = {(521, 1): "521m", (255, 2): "255c", (384, 3): "384n", (256, 4): "256k", (448, 5): "448g", (224, 6): "224s", (192, 7): "192s"}
ROUTED = ["upload", "launch", "msm", "prj_import", "comb_build"]
NBIAS = 16


def unit_of(pbits, flavour):
    """the tag the calls for (pbits, flavour) must reach, or None"""
    if (pbits, flavour) in FLAVOURED:
        return FLAVOURED[(pbits, flavour)]
    return str(pbits) if pbits in DENSE else None


def _run(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"] + flags
                          + ["-o", exe] + SOURCES)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def out():
    text = _run("g29_dispatch_host", [])
    rec = {"route": {}, "geom": {}, "supported": {}}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "codes":
            rec["codes"] = (int(w[1]), int(w[2]))
        elif w[0] == "route":
            assert (w[1], int(w[2]), int(w[3])) not in rec["route"]
            rec["route"][(w[1], int(w[2]), int(w[3]))] = (int(w[4]), w[5], int(w[6]))
        elif w[0] == "geom":
            rec["geom"][(int(w[1]), int(w[2]))] = tuple(int(x) for x in w[3:])
        elif w[0] == "supported":
            rec["supported"][int(w[1])] = int(w[2])
        else:
            assert w[0] == "slots"
            rec["slots"] = int(w[1])
    rec["text"] = text
    return rec


def test_every_pair_was_called(out):
    assert out["codes"] == (0, 1)   # hipSuccess, hipErrorInvalidValue
    assert len(out["route"]) == len(PBITS) * len(FLAVOURS) * (len(ROUTED) + 1) + len(PBITS) + len(FLAVOURS)
    assert len(out["geom"]) == len(PBITS) * len(FLAVOURS)


@pytest.mark.parametrize("fn", ROUTED)
def test_routing_by_size_and_flavour(out, fn):
    ok, invalid = out["codes"]
    for pb in PBITS:
        for fl in FLAVOURS:
            tag = unit_of(pb, fl)
            want = (ok, f"{fn}:{tag}", 1) if tag else (invalid, "-", 0)
            assert out["route"][(fn, pb, fl)] == want, (fn, pb, fl)


def test_routing_examples_spelled_out(out):
    """a few pairs by hand, so that a slip in unit_of() above cannot hide one in the dispatcher"""
    r = out["route"]
    assert r[("launch", 256, 4)][1] == "launch:256k" and r[("launch", 256, 0)][1] == "launch:256"
    assert r[("launch", 256, 3)][1] == "launch:256"      # a flavour that does not belong to the size: the dense unit
    assert r[("upload", 521, 1)][1] == "upload:521m" and r[("upload", 521, 7)][1] == "upload:521"
    assert r[("msm", 255, 2)][1] == "msm:255c" and r[("prj_import", 448, 5)][1] == "prj_import:448g"
    assert r[("comb_build", 192, 7)][1] == "comb_build:192s" and r[("comb_build", 224, 6)][1] == "comb_build:224s"
    assert r[("upload", 384, 3)][1] == "upload:384n" and r[("upload", 384, -1)][1] == "upload:384"
    assert r[("launch", 257, 4)] == (out["codes"][1], "-", 0) and r[("msm", 0, 0)] == (out["codes"][1], "-", 0)


def test_empty_batch_returns_before_routing(out):
    for pb in PBITS:
        for fl in FLAVOURS:
            assert out["route"][("launch_n0", pb, fl)] == (out["codes"][0], "-", 0), (pb, fl)


def test_ecdsa_prep_routes_over_the_dense_units(out):
    ok, invalid = out["codes"]
    for pb in PBITS:
        want = (ok, f"ecdsa_prep:{pb}", 1) if pb in DENSE else (invalid, "-", 0)
        assert out["route"][("ecdsa_prep", pb, 0)] == want, pb
        assert out["supported"][pb] == (1 if pb in DENSE else 0)


def test_ed_fin_knows_the_two_edwards_units(out):
    ok, invalid = out["codes"]
    for fl in FLAVOURS:
        want = {2: (ok, "ed_fin:255c", 1), 5: (ok, "ed_fin:448g", 1)}.get(fl, (invalid, "-", 0))
        assert out["route"][("ed_fin", 0, fl)] == want, fl


def _nl(pbits, flavour):
    return {2: 9, 4: 9, 5: 16, 1: 18}.get(flavour, (pbits + 16 + 28) // 29)


def _up4(x):
    return (x + 3) // 4 * 4


def _geometry(pb, fl):
    nl, nw = _nl(pb, fl), (pb + 31) // 32
    bkt = _up4(2 * nl)
    bkt = 16 if bkt <= 16 else (32 if bkt <= 32 else (64 if bkt <= 64 else 128))
    return (8 * _up4(3 * nl) + _up4(2 * nw + 2),    # table words
            8 * _up4(2 * nl),                       # affine words
            _up4(2 * nl),                           # comb entry words
            bkt,                                    # bucket point words
            _up4(3 * nl) + 4,                       # msm record words
            ((10 + NBIAS) * nl + 4) * 4,            # image bytes
            8 * nw + 4,                             # max_slen
            4 * nw,                                 # comb_max_slen
            nl,
            2 * nw * 32768 + 1)                     # comb entries


def test_geometry_formulas(out):
    assert out["slots"] == 8
    pairs = [(pb, 0) for pb in DENSE] + list(FLAVOURED)
    assert len(pairs) == 17
    for pb, fl in pairs:
        assert out["geom"][(pb, fl)] == _geometry(pb, fl), (pb, fl)
    # a flavour is an argument of the formulas, whatever the size: flavours 1, 2, 4, 5 fix the limb count on any size (so (256, 2)
    # answers with nine limbs though it is routed to the dense unit), the others give the dense formula
    for pb in PBITS:
        for fl in FLAVOURS:
            assert out["geom"][(pb, fl)] == _geometry(pb, fl), (pb, fl)
    for pb in DENSE:
        for fl in (-1, 0, 3, 6, 7, 8):
            assert out["geom"][(pb, fl)] == out["geom"][(pb, 0)]


def test_same_program_under_sanitizers(out):
    assert _run("g29_dispatch_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == out["text"]
