"""CPU-side checks of the blocked gzip (BGZF) writer, ndfl_deflate_bgzf (include/ndfl.h): its host-only bound
against a restatement of the rule, and -- with zlib alone -- the two sizes its GPU tests rest on."""
import ctypes
import os
import random
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deflate-library-java_amd", "lib", "libndfl.so")


def stored_member(n):
    """A member's length with its n bytes stored: 18 header bytes, 5 per stored block of at most 65,535
    bytes (an empty block still has one), the bytes, CRC-32 and ISIZE."""
    return 18 + 5 * max(1, -(-n // 65535)) + n + 8


def bound(in_len, block_len):
    """ndfl_bgzf_bound restated: every member stored, and the 28-byte closing member."""
    if not 1 <= block_len <= 65536:
        return 0
    full, tail = divmod(in_len, block_len)
    return full * stored_member(block_len) + (stored_member(tail) if tail else 0) + 28


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB)                                  # (loads without a GPU)
    L.ndfl_bgzf_bound.restype = ctypes.c_uint64
    L.ndfl_bgzf_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    return L


@pytest.mark.parametrize("block_len", [1, 65280, 65505, 65535, 65536])
def test_bound_is_the_stored_file(lib, block_len):
    for in_len in (0, 1, block_len - 1, block_len, block_len + 1, 3 * block_len + 7):
        assert lib.ndfl_bgzf_bound(in_len, block_len) == bound(in_len, block_len), (in_len, block_len)
    assert lib.ndfl_bgzf_bound(0, block_len) == 28


def test_bound_by_hand(lib):
    assert lib.ndfl_bgzf_bound(65505, 65505) == 65536 + 28
    assert lib.ndfl_bgzf_bound(65536, 65536) == 65572 + 28           # two stored blocks: 65,535 bytes and 1
    assert lib.ndfl_bgzf_bound(10, 4) == 2 * 35 + 33 + 28


@pytest.mark.parametrize("block_len", [0, 65537, 1 << 31])
def test_bound_of_an_invalid_block_len(lib, block_len):
    for in_len in (0, 1, 100000):
        assert lib.ndfl_bgzf_bound(in_len, block_len) == 0


def test_sizes_the_gpu_tests_rest_on():
    """A random block of 65,505 bytes fits a member only stored, and then exactly; one of 65,536 bytes fits
    in no form.  (zlib -9 here: members of 65,551 and 65,582 bytes.)"""
    rng = random.Random(65505)
    for n, stored in ((65505, 65536), (65536, 65572)):
        d = rng.randbytes(n)
        co = zlib.compressobj(9, zlib.DEFLATED, -15)
        deflated = 18 + len(co.compress(d) + co.flush()) + 8
        print(n, "stored", stored_member(n), "zlib -9", deflated)
        assert stored_member(n) == stored
        assert deflated > 65536
    assert stored_member(65505) <= 65536 < stored_member(65506)
