"""The header finder's resources, read from the built libndfl.so's metadata (CPU only).

ndfl_inflate_find_compact_kernel is bound by the instructions it issues and hides its LDS and load
latencies behind other waves, so it must stay at 8 waves per SIMD: no scratch, no spilled register of
either kind, at most 64 VGPRs, and LDS small enough for the 8 workgroups of 4 waves that make 32 waves
on a CU.
"""
import pytest

from test_kernel_resources import kernel_metadata, needs_tools

KERNEL = "ndfl_inflate_find_compact_kernel"
WAVES_PER_WORKGROUP = 256 // 64          # its launch bound
WAVES_PER_CU = 32
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def finder():
    return kernel_metadata()[KERNEL]


@needs_tools
def test_finder_uses_no_scratch(finder):
    assert finder["private_segment_fixed_size"] == 0, finder


@needs_tools
def test_finder_spills_nothing(finder):
    assert finder["vgpr_spill_count"] == 0, finder
    assert finder["sgpr_spill_count"] == 0, finder


@needs_tools
def test_finder_registers_allow_8_waves_per_simd(finder):
    assert 0 < finder["vgpr_count"] <= 64, finder


@needs_tools
def test_finder_lds_allows_32_waves_per_cu(finder):
    workgroups = WAVES_PER_CU // WAVES_PER_WORKGROUP
    assert finder["group_segment_fixed_size"] * workgroups <= LDS_PER_CU, finder
