"""CPU: the fused backward slab pass keeps two blocks resident per CU.

`k_agg_sddmm` runs 768-lane blocks (12 waves); two of them per CU are 6 waves per SIMD, which the 512-entry register file
grants up to 80 VGPRs a lane (allocated in eights).  Its requests ahead of the slab barrier live in registers, and the
count moves by a dozen with the form of the gather loop (aggregate.hip), so it is read from the compiler here: at 81
the second block is gone and the pass is a tenth slower, with every result still right.
"""
import os

from test_no_register_spills import _kernel_metadata


def test_agg_sddmm_fits_two_blocks_per_cu(tmp_path):
    from ms_gat_amd import build
    rows = [r for r in _kernel_metadata(os.path.join(build.CSRC, "aggregate.hip"), str(tmp_path)) if "k_agg_sddmm" in r[0]]
    assert len(rows) == 4, rows                       # T / 4 = 1 ... 4
    for name, vgprs, spilled, _ in rows:
        assert spilled == 0 and vgprs <= 80, f"{name}: {vgprs} VGPRs, {spilled} spilled"
