"""CPU test of k_belt_slots itself (libecc_amd/csrc/ecamd_hash.hip compiled for the host through tests/hipstub, as
tests/test_hash_host.py does for the SHA-2 kernels): several blocks of lanes, every length 0 .. 259, a 4092-byte message, a length
word the slot cannot hold, an output stride wider than the digest, and the launcher's argument checks."""
import ctypes as C
import os
import subprocess

import pytest

import bign_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "belt_kernel_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-I", os.path.join(ROOT, "tests", "hipstub"), "-o", so,
                           os.path.join(ROOT, "tests", "belt_kernel_host_shim.cpp")])
    L = C.CDLL(so)
    L.belt_slots_host.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    return L


def test_kernel_on_every_length_over_several_blocks(lib):
    fx = dict(B.load_fixture(os.path.join(ROOT, "tests", "golden", "bign.json"))["belt"])
    msgs = [B.pattern_msg(n) for n in range(260)]          # 260 lanes: five blocks of 64, the last one ragged
    stride, ostride = 264, 40
    out = C.create_string_buffer(ostride * len(msgs))
    assert lib.belt_slots_host(b"".join(B.slot(m, stride) for m in msgs), stride, len(msgs), out, ostride) == 0
    for n, m in enumerate(msgs):
        got = out.raw[ostride * n:ostride * n + 32]
        assert got == B.belt_hash(m), n
        assert out.raw[ostride * n + 32:ostride * (n + 1)] == bytes(8), n     # nothing written beyond the digest
        if n <= 100:
            assert got.hex() == fx[n]
    out = C.create_string_buffer(32)
    assert lib.belt_slots_host(B.slot(B.pattern_msg(4092), 4096), 4096, 1, out, 32) == 0
    assert out.raw.hex() == fx[4092]
    assert lib.belt_slots_host(B.slot(b"0123456789ab", 16, length=0xFFFFFFFF), 16, 1, out, 32) == 0
    assert out.raw == B.belt_hash(b"0123456789ab")


def test_launcher_argument_checks(lib):
    out = C.create_string_buffer(64)
    assert lib.belt_slots_host(bytes(8), 8, 0, out, 32) == 0
    for stride, ostride in ((0, 32), (2, 32), (10, 32), (8, 31)):
        assert lib.belt_slots_host(bytes(16), stride, 1, out, ostride) != 0
