"""The resources of the blocked gzip (BGZF) writer's kernels (csrc/hip/deflate_bgzf.hip), read from the built
libndfl.so as tests/test_kernel_resources.py reads the others', CPU only.

None of them may use scratch memory: no stack, no spill of either kind.  The pack
kernel runs workgroups of 1,024 threads, four waves on each SIMD: at most 128 VGPRs.
"""
import pytest

from test_kernel_resources import kernel_metadata, needs_tools

BGZW_KERNELS = ["ndfl_bgzw_tables_kernel", "ndfl_bgzw_size_kernel", "ndfl_bgzw_offsets_kernel", "ndfl_bgzw_pack_kernel"]


@needs_tools
@pytest.mark.parametrize("kernel", BGZW_KERNELS)
def test_bgzf_writer_kernels_use_no_scratch(kernel):
    ks = kernel_metadata()
    assert kernel in ks, sorted(n for n in ks if "bgzw" in n)
    k = ks[kernel]
    print(kernel, k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 128, k


@needs_tools
def test_every_bgzf_writer_kernel_is_listed():
    assert sorted(n for n in kernel_metadata() if "ndfl_bgzw_" in n) == sorted(BGZW_KERNELS)
