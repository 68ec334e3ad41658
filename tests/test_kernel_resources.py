"""Kernel resources read from the built libndfl.so (its gfx950 code object's metadata notes), CPU only.

The strict stage (ndfl_inflate_strict_kernel) must not use scratch memory: builds of it that did --
a call to a non-inlined helper (its stack) or register spills -- lost real block headers at full
load, nondeterministically (tests/test_gpu_headers.py compares the accepted
set with the oracle).  The header finder and the count/emit passes are listed with their VGPRs and
spills for the record (profiles/ quote them).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deflate-library-java_amd", "lib", "libndfl.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_metadata(lib=LIB, tmp="/tmp"):
    """{kernel name: {key: int}} from the .hip_fatbin's gfx950 code object (llvm-readelf --notes)."""
    fb = os.path.join(tmp, f"ndfl_fatbin_{os.getpid()}.bin")
    co = os.path.join(tmp, f"ndfl_co_{os.getpid()}.o")
    cp = os.path.join(tmp, f"ndfl_lib_{os.getpid()}.so")
    try:
        # (on a copy: objcopy with one file argument rewrites that file, which would corrupt the
        # library a test process already has mapped)
        shutil.copyfile(lib, cp)
        subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fb}", cp, cp + ".out"])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    finally:
        for f in (fb, co, cp, cp + ".out"):
            if os.path.exists(f):
                os.remove(f)
    kernels, entry = {}, None
    for line in notes.splitlines():
        if re.match(r"\s*- \.", line):                 # a new kernel entry (keys come alphabetically)
            entry = {}
        m = re.match(r"\s*-?\s*\.name:\s+(\S+)$", line)
        if m and entry is not None and not m.group(1).endswith(".kd"):
            kernels[m.group(1)] = entry
            continue
        m = re.match(r"\s*-?\s*\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|"
                     r"group_segment_fixed_size):\s+(\d+)$", line)
        if m and entry is not None:
            entry[m.group(1)] = int(m.group(2))
    return kernels


needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which("objcopy") and
                                      os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                                 reason="needs the built library and the ROCm LLVM tools")


@needs_tools
def test_strict_stage_uses_no_scratch():
    k = kernel_metadata()["ndfl_inflate_strict_kernel"]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    # 5 waves per SIMD: 512 / 5 -> at most 96 VGPRs (granule 8), and 5 workgroups' tables in LDS
    assert k["vgpr_count"] <= 96, k
    assert 5 * k["group_segment_fixed_size"] <= 160 * 1024, k


@needs_tools
def test_every_exported_kernel_has_metadata():
    ks = kernel_metadata()
    for name in ("ndfl_inflate_find_compact_kernel", "ndfl_inflate_count_wave_kernel",
                 "ndfl_inflate_emit_fast_kernel", "ndfl_deflate_hist_kernel", "ndfl_deflate_emit_kernel"):
        assert name in ks and ks[name]["vgpr_count"] > 0, name


# The kernels that write and read the count pass's records (inflate_records.hpp): scratch bytes per
# lane, spilled VGPRs, VGPRs and LDS bytes must not grow past these (measured before the record helpers
# replaced the hand-written stores and loads).  The count kernels already spill, and scratch in these
# kernels is the project's open hazard (VERDICT, "Correctness hazard"), so a change that adds to it
# must be noticed.  Upper bounds: smaller is welcome.
RECORD_KERNEL_BOUNDS = {
    # kernel (substring of the symbol): scratch B, vgpr spills, vgprs, LDS B
    "ndfl_inflate_count_wave_kernel": (400, 65, 168, 12464),
    "count_wg_kernelILi2E": (464, 180, 168, 18160),
    "count_wg_kernelILi4E": (464, 205, 168, 28656),
    "count_wg_kernelILi8E": (448, 97, 168, 49648),
    "ndfl_inflate_emit_fast_kernel": (40, 9, 128, 9728),
    "ndfl_inflate_emit_wave_kernel": (72, 13, 168, 12208),
}


@needs_tools
@pytest.mark.parametrize("kernel", sorted(RECORD_KERNEL_BOUNDS))
def test_record_kernels_do_not_grow(kernel):
    names = [n for n in kernel_metadata() if kernel in n]
    assert len(names) == 1, (kernel, names)
    k = kernel_metadata()[names[0]]
    scratch, spills, vgprs, lds = RECORD_KERNEL_BOUNDS[kernel]
    print(names[0], k)
    assert k["private_segment_fixed_size"] <= scratch, k
    assert k["vgpr_spill_count"] <= spills, k
    assert k["vgpr_count"] <= vgprs, k
    assert k["group_segment_fixed_size"] <= lds, k


# The encoder kernels around the one code builder (huffman_build.hpp), measured before it replaced the
# wave-wide and the 1024-thread builders.  The split passes use no scratch and spill nothing; the
# one-kernel encoder and the LZ77 encoder must not add to theirs (the LZ77 encoder's 192 B are no
# spills: its argument block, which the parse walk's lambdas capture by reference, is copied to the
# stack at entry; the same before and after, not the builder's).  Upper bounds: smaller is
# welcome.  VGPRs of the two 1024-thread encoders are bounded by their launch bounds instead: 512 per
# SIMD over the 4 waves a workgroup puts on it (LZ77), over the 8 waves asked for (one-kernel encoder).
ENCODER_KERNEL_BOUNDS = {
    # kernel: scratch B, vgpr spills, sgpr spills, vgprs, LDS B
    "ndfl_lz_encode_kernel": (192, 0, 0, 128, 142272),
    "ndfl_deflate_chunks_kernel": (36, 13, 68, 64, 77336),
    "ndfl_deflate_codes_kernel": (0, 0, 0, 44, 8784),
    "ndfl_deflate_hist_kernel": (0, 0, 0, 43, 18832),
    "ndfl_deflate_emit_kernel": (0, 0, 0, 64, 75952),
}


@needs_tools
@pytest.mark.parametrize("kernel", sorted(ENCODER_KERNEL_BOUNDS))
def test_encoder_kernels_do_not_grow(kernel):
    k = kernel_metadata()[kernel]
    scratch, spills, sspills, vgprs, lds = ENCODER_KERNEL_BOUNDS[kernel]
    print(kernel, k)
    assert k["private_segment_fixed_size"] <= scratch, k
    assert k["vgpr_spill_count"] <= spills, k
    assert k["sgpr_spill_count"] <= sspills, k
    assert k["vgpr_count"] <= vgprs, k
    assert k["group_segment_fixed_size"] <= lds, k


# The four batched deflate kernels (deflate_batch*.hip): one wave per workgroup, everything forced inline,
# wave-uniform state parked in VGPRs -- so no scratch and no spill of either kind, which their sources
# claim and this asserts.  Measured before the LZ kernels' chunk layer (dblz::) was shared: 111, 122, 132
# and 131 VGPRs, here rounded up to the allocation granule of 8; LDS is exact.  Upper bounds: smaller is
# welcome.
BATCH_DEFLATE_KERNEL_BOUNDS = {
    # kernel: scratch B, vgpr spills, sgpr spills, vgprs, LDS B
    "ndfl_deflate_batch_kernel": (0, 0, 0, 112, 12632),
    "ndfl_deflate_batch_lz_kernel": (0, 0, 0, 128, 20824),
    "ndfl_deflate_batch_multi_kernel": (0, 0, 0, 136, 22424),
    "ndfl_deflate_batch_binsplit_kernel": (0, 0, 0, 136, 21016),
}


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BATCH_DEFLATE_KERNEL_BOUNDS))
def test_batch_deflate_kernels_do_not_grow(kernel):
    k = kernel_metadata()[kernel]
    scratch, spills, sspills, vgprs, lds = BATCH_DEFLATE_KERNEL_BOUNDS[kernel]
    print(kernel, k)
    assert k["private_segment_fixed_size"] <= scratch, k
    assert k["vgpr_spill_count"] <= spills, k
    assert k["sgpr_spill_count"] <= sspills, k
    assert k["vgpr_count"] <= vgprs, k
    assert k["group_segment_fixed_size"] <= lds, k
