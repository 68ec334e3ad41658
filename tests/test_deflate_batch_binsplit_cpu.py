"""ndfl_deflate_batch_binsplit without a GPU: the symbol, the argument check that needs no context, and the
resources of its kernel (csrc/hip/deflate_batch_binsplit.hip) from the built library's metadata.  Like its
siblings the kernel puts several waves on each SIMD, so it must use no scratch memory and spill nothing
(DESIGN.md §7 item 9), and its LDS and VGPRs must leave the waves per CU that DESIGN.md §4 ("Batched
BinarySplit deflate") documents.
"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from test_kernel_resources import kernel_metadata, needs_tools

KERNEL = "ndfl_deflate_batch_binsplit_kernel"


def test_null_context_is_an_argument_error():
    from ndfl import _lib as L
    lib = L.load()
    assert "ndfl_deflate_batch_binsplit" in L.EXPORTS
    item = (L.MemberItem * 1)(L.MemberItem(0, 2, 0, 16, L.FMT_RAW, L.SUM_NONE))
    res = (L.DeflateResult * 1)()
    src = ctypes.create_string_buffer(b"ab", 2)
    out = ctypes.create_string_buffer(16)
    sub = L.StrategyDesc(L.KIND_LZ77, 1, 3, 258, 1, 32768)
    assert lib.ndfl_deflate_batch_binsplit(None, ctypes.addressof(src), 2, ctypes.addressof(out), 16, item, res, 1,
                                           ctypes.byref(sub), 100, 65536, 32768, 0) == L.E_ARG
    assert lib.ndfl_deflate_batch_binsplit(None, None, 0, None, 0, None, None, 0, ctypes.byref(sub), 100, 65536, 32768,
                                           0) == L.E_ARG
    assert out.raw == bytes(16) and res[0].out_len == 0 and res[0].status == 0 and res[0].end_bits == 0


def documented_waves_per_cu():
    """The figure DESIGN.md states for the batched BinarySplit kernel ("N waves per CU")."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### Batched BinarySplit deflate"):]
    m = re.search(r"(\d+) waves per CU", sec)
    assert m, "DESIGN.md: the batched BinarySplit kernel's waves per CU"
    return int(m.group(1))


@needs_tools
def test_binsplit_batch_kernel_uses_no_scratch_and_fits_its_occupancy():
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
