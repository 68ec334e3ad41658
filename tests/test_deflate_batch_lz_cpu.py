"""ndfl_deflate_batch_lz77 without a GPU: the symbol, the argument check that needs no context, and the
resources of its kernel (csrc/hip/deflate_batch_lz.hip) from the built library's metadata.  The kernel
puts several waves on each SIMD, so it must use no scratch memory and spill nothing (DESIGN.md §7 item
9), and its LDS and VGPRs must leave the waves per CU that DESIGN.md §4 ("Batched LZ77 deflate")
documents.  Adding it must not have changed ndfl_deflate_batch_kernel, whose helpers it shares.
"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from test_kernel_resources import kernel_metadata, needs_tools

KERNEL = "ndfl_deflate_batch_lz_kernel"


def test_null_context_is_an_argument_error():
    from ndfl import _lib as L
    lib = L.load()
    assert "ndfl_deflate_batch_lz77" in L.EXPORTS
    item = (L.MemberItem * 1)(L.MemberItem(0, 2, 0, 16, L.FMT_RAW, L.SUM_NONE))
    res = (L.DeflateResult * 1)()
    src = ctypes.create_string_buffer(b"ab", 2)
    out = ctypes.create_string_buffer(16)
    full = (1, 3, 258, 1, 32768)
    assert lib.ndfl_deflate_batch_lz77(None, ctypes.addressof(src), 2, ctypes.addressof(out), 16, item, res, 1, *full,
                                       65536, 32768, 0) == L.E_ARG
    assert lib.ndfl_deflate_batch_lz77(None, None, 0, None, 0, None, None, 0, *full, 65536, 32768, 0) == L.E_ARG
    assert out.raw == bytes(16) and res[0].out_len == 0 and res[0].status == 0 and res[0].end_bits == 0


def documented_waves_per_cu():
    """The figure DESIGN.md states for the batched LZ77 kernel ("N waves per CU")."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### Batched LZ77 deflate"):]
    m = re.search(r"(\d+) waves per CU", sec)
    assert m, "DESIGN.md: the batched LZ77 kernel's waves per CU"
    return int(m.group(1))


@needs_tools
def test_lz_batch_kernel_uses_no_scratch_and_fits_its_occupancy():
    ks = kernel_metadata()
    assert KERNEL in ks, sorted(ks)
    k = ks[KERNEL]
    print(KERNEL, k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["sgpr_spill_count"] == 0, k
    waves = documented_waves_per_cu()
    assert waves >= 1 and k["group_segment_fixed_size"] * waves <= 160 * 1024, (k, waves)
    # `waves` one-wave workgroups spread over the CU's 4 SIMDs, 512 VGPRs each: VGPRs must not bound it
    assert k["vgpr_count"] * -(-waves // 4) <= 512, (k, waves)
    # what the kernel took before its stream frame became deflate_batch.hip's (upper bounds: smaller is welcome)
    assert k["vgpr_count"] <= 122 and k["group_segment_fixed_size"] <= 20824, k


@needs_tools
def test_rle_batch_kernel_did_not_drift():
    """ndfl_deflate_batch_kernel as DESIGN.md §4 "Batched deflate" states it."""
    k = kernel_metadata()["ndfl_deflate_batch_kernel"]
    assert k == {"group_segment_fixed_size": 12632, "vgpr_count": 111, "private_segment_fixed_size": 0,
                 "vgpr_spill_count": 0, "sgpr_spill_count": 0}, k
