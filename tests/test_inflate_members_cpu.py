"""ndfl_inflate_members without a GPU: the argument check that needs no context, the struct sizes of
the C ABI, and the members kernel's resources from the built library's metadata.  Like the plain batch
kernel (tests/test_inflate_batch_cpu.py) it must use no scratch memory and spill nothing (DESIGN.md §7
item 9), and four waves' LDS must fit a CU.
"""
import ctypes

from test_kernel_resources import kernel_metadata, needs_tools

KERNEL = "ndfl_inflate_members_kernel"


def test_null_context_is_an_argument_error():
    from ndfl import _lib as L
    lib = L.load()
    assert "ndfl_inflate_members" in L.EXPORTS
    item = (L.MemberItem * 1)(L.MemberItem(0, 2, 0, 16, L.FMT_RAW, L.SUM_CRC32))
    res = (L.MemberResult * 1)()
    src = ctypes.create_string_buffer(b"\x03\x00", 2)
    out = ctypes.create_string_buffer(16)
    assert lib.ndfl_inflate_members(None, ctypes.addressof(src), 2, ctypes.addressof(out), 16, item, res, 1, 0) == L.E_ARG
    assert lib.ndfl_inflate_members(None, None, 0, None, 0, None, None, 0, 0) == L.E_ARG


def test_struct_sizes_and_constants():
    import ndfl
    from ndfl import _lib as L
    assert ctypes.sizeof(L.MemberItem) == 40 and ctypes.sizeof(L.MemberResult) == 32
    assert (L.FMT_RAW, L.FMT_ZLIB, L.FMT_GZIP) == (0, 1, 2) == (ndfl.FMT_RAW, ndfl.FMT_ZLIB, ndfl.FMT_GZIP)
    assert (L.SUM_NONE, L.SUM_CRC32, L.SUM_ADLER32) == (0, 1, 2) == (ndfl.SUM_NONE, ndfl.SUM_CRC32, ndfl.SUM_ADLER32)


@needs_tools
def test_members_kernel_uses_no_scratch_and_fits_four_waves():
    ks = kernel_metadata()
    assert KERNEL in ks, sorted(ks)
    k = ks[KERNEL]
    print(KERNEL, k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] * 4 <= 160 * 1024, k
