"""The resources of the blocked gzip (BGZF) kernels (csrc/hip/inflate_bgzf.hip), read from the built
libndfl.so as tests/test_kernel_resources.py reads the others', CPU only.

None of them may use scratch memory (wrong values when two scratch-using waves of one
kernel share a SIMD): no stack, no spill of either kind.  They run before and after the members kernel on the
same stream, never beside it, so their registers and LDS bound nothing else.
"""
import pytest

from test_kernel_resources import kernel_metadata, needs_tools

# substring of the symbol (the two passes of the scan and of the layout are instances of one template)
BGZF_KERNELS = ["ndfl_bgzf_scan_kernelILb0E", "ndfl_bgzf_scan_kernelILb1E", "ndfl_bgzf_sum_kernel",
                "ndfl_bgzf_link_kernel", "ndfl_bgzf_mark_kernel", "ndfl_bgzf_layout_kernelILb0E",
                "ndfl_bgzf_layout_kernelILb1E", "ndfl_bgzf_reduce_kernel"]


@needs_tools
@pytest.mark.parametrize("kernel", BGZF_KERNELS)
def test_bgzf_kernels_use_no_scratch(kernel):
    ks = kernel_metadata()
    names = [n for n in ks if kernel in n]
    assert len(names) == 1, (kernel, names)
    k = ks[names[0]]
    print(names[0], k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["sgpr_spill_count"] == 0, k
    # a workgroup of 1,024 threads puts four waves on each SIMD: at most 128 VGPRs
    assert k["vgpr_count"] <= 128, k


@needs_tools
def test_every_bgzf_kernel_is_listed():
    assert len([n for n in kernel_metadata() if "ndfl_bgzf_" in n]) == len(BGZF_KERNELS)
