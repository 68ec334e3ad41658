"""ndfl_deflate_batch_chunked without a GPU: the symbol, the argument check that needs no context, and the
resources of the kernels from the built library's metadata.  The segmented chunk encoders (the *_seg_kernel
entry points) are instantiations of the bodies the existing chunk encoders run, so they must use no scratch
and spill nothing wherever their siblings do not (scratch under co-resident waves is DESIGN.md §7 item 9),
and adding them must not have changed the siblings: their metadata is pinned to what the commit before
this call gave.
"""
import ctypes

import pytest

from test_kernel_resources import kernel_metadata, needs_tools


def test_null_context_is_an_argument_error():
    from ndfl import _lib as L
    lib = L.load()
    assert "ndfl_deflate_batch_chunked" in L.EXPORTS
    item = (L.MemberItem * 1)(L.MemberItem(0, 2, 0, 16, L.FMT_RAW, L.SUM_NONE))
    res = (L.DeflateResult * 1)()
    src = ctypes.create_string_buffer(b"ab", 2)
    out = ctypes.create_string_buffer(16)
    for tup in ((1, 3, 258, 1, 32768), (1, 3, 258, 1, 1), (0, 0, 0, 0, 0)):
        assert lib.ndfl_deflate_batch_chunked(None, ctypes.addressof(src), 2, ctypes.addressof(out), 16, item, res, 1,
                                              *tup, 65536, 32768, 0) == L.E_ARG
        assert lib.ndfl_deflate_batch_chunked(None, None, 0, None, 0, None, None, 0, *tup, 65536, 32768, 0) == L.E_ARG
    assert out.raw == bytes(16) and res[0].out_len == 0 and res[0].status == 0 and res[0].end_bits == 0


def meta(scratch, vgprs, lds, spills=0, sspills=0):
    return {"private_segment_fixed_size": scratch, "vgpr_count": vgprs, "group_segment_fixed_size": lds,
            "vgpr_spill_count": spills, "sgpr_spill_count": sspills}


# The existing chunk encoders, as the commit before ndfl_deflate_batch_chunked built them.
PARENT = {
    "ndfl_deflate_hist_kernel": meta(0, 43, 17552),
    "ndfl_deflate_codes_kernel": meta(0, 44, 8784),
    "ndfl_deflate_emit_kernel": meta(0, 64, 75952),
    "ndfl_deflate_offsets_sum_kernel": meta(0, 34, 32),
    "ndfl_deflate_offsets_kernel": meta(0, 48, 64),
    "ndfl_edge_fixup_kernel": meta(0, 10, 0),
    "ndfl_lz_parse_match_kernel": meta(0, 47, 157856),
    "ndfl_lz_encode_kernel": meta(192, 71, 141200),
    "ndfl_deflate_chunks_kernel": meta(28, 64, 76272, spills=11, sspills=52),
}


@needs_tools
@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_existing_chunk_encoders_did_not_change(kernel):
    assert kernel_metadata()[kernel] == PARENT[kernel]


# segmented kernel: its sibling
SIBLINGS = {
    "ndfl_deflate_hist_seg_kernel": "ndfl_deflate_hist_kernel",
    "ndfl_deflate_codes_seg_kernel": "ndfl_deflate_codes_kernel",
    "ndfl_deflate_emit_seg_kernel": "ndfl_deflate_emit_kernel",
    "ndfl_lz_parse_match_seg_kernel": "ndfl_lz_parse_match_kernel",
    "ndfl_lz_encode_seg_kernel": "ndfl_lz_encode_kernel",
}


@needs_tools
@pytest.mark.parametrize("kernel", sorted(SIBLINGS))
def test_segmented_kernels_add_no_scratch_and_no_spills(kernel):
    ks = kernel_metadata()
    assert kernel in ks, sorted(ks)
    k, sib = ks[kernel], ks[SIBLINGS[kernel]]
    print(kernel, k)
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    # hist, codes, emit and the search: 0 B; the LZ encoder may keep its sibling's 192 B argument copy
    assert k["private_segment_fixed_size"] <= sib["private_segment_fixed_size"], (k, sib)
    assert k["group_segment_fixed_size"] == sib["group_segment_fixed_size"], (k, sib)
    # the same launch bounds: 8 waves per SIMD for the split passes (64 VGPRs), 4 for the LZ kernels
    assert k["vgpr_count"] <= (64 if "deflate" in kernel else 128), k


@needs_tools
@pytest.mark.parametrize("kernel", ["ndfl_deflate_offsets_seg_kernel", "ndfl_seg_gather_kernel", "ndfl_seg_sums_kernel",
                                    "ndfl_seg_sums_combine_kernel", "ndfl_seg_finish_kernel"])
def test_new_kernels_use_no_scratch(kernel):
    ks = kernel_metadata()
    assert kernel in ks, sorted(ks)
    k = ks[kernel]
    print(kernel, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
