"""ndfl_inflate_batch without a GPU: the argument check that needs no context, and the batch kernel's
resources from the built library's metadata.  The kernel must use no scratch memory and spill
nothing (two scratch-using waves of one kernel on a SIMD have given wrong values, DESIGN.md §7 item
9), and its LDS ring must leave the waves per CU that DESIGN.md §4 ("Batched inflate") documents.
"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from test_kernel_resources import kernel_metadata, needs_tools

KERNEL = "ndfl_inflate_batch_kernel"


def test_null_context_is_an_argument_error():
    from ndfl import _lib as L
    lib = L.load()
    assert "ndfl_inflate_batch" in L.EXPORTS
    item = (L.BatchItem * 1)(L.BatchItem(0, 2, 0, 16))
    res = (L.BatchResult * 1)()
    src = ctypes.create_string_buffer(b"\x03\x00", 2)
    out = ctypes.create_string_buffer(16)
    assert lib.ndfl_inflate_batch(None, ctypes.addressof(src), 2, ctypes.addressof(out), 16, item, res, 1, 0) == L.E_ARG
    assert lib.ndfl_inflate_batch(None, None, 0, None, 0, None, None, 0, 0) == L.E_ARG
    assert ctypes.sizeof(L.BatchItem) == 32 and ctypes.sizeof(L.BatchResult) == 24


def documented_waves_per_cu():
    """The figure DESIGN.md states for the batch kernel ("N waves per CU")."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("Batched inflate"):]
    m = re.search(r"(\d+) waves per CU", sec)
    assert m, "DESIGN.md: the batch kernel's waves per CU"
    return int(m.group(1))


@needs_tools
def test_batch_kernel_uses_no_scratch_and_fits_its_occupancy():
    ks = kernel_metadata()
    assert KERNEL in ks, sorted(ks)
    k = ks[KERNEL]
    print(KERNEL, k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["sgpr_spill_count"] == 0, k
    waves = documented_waves_per_cu()
    assert waves >= 1 and k["group_segment_fixed_size"] * waves <= 160 * 1024, (k, waves)
    # one wave per SIMD at the most (4 SIMDs per CU): up to 512 VGPRs each, so VGPRs never bound it
    assert waves <= 4 and k["vgpr_count"] <= 512, (k, waves)
