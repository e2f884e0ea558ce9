"""CPU: which one-pass backward form the GACN projection of each registry model takes (msgat_contract_form_name, host only).

The [25 x 72] contraction + mix of msgat72 runs as two z-blocks over its 72 columns (k_chanpair_glds<2,3,128,3,1>, each
block stages all 25 rows and writes 36 mix channels): 0.027 ms per hot-path step below the one-block form <2,5,128,3,1>
at rows of 10596 positions, 0.004 ms at 3684 (profiles/project_wide_tiles/ab_parent_vs_tree.txt).  The rule names that
block by its two channel counts alone -- never the batch, the row length or the device -- so the form is the same at
every row length the LDS-DMA kernels take; its neighbours and the wider blocks, which lost as z-blocks, keep their forms.
Its numbers are checked on the GPU by test_stage_project_backward_matches_float64 (72 -> 24 at N = 883,
tests/test_gpu_branches.py) and by the headline golden of tests/test_gpu_parity.py."""
import pytest


@pytest.mark.parametrize("P", [512, 307 * 12, 883 * 12])
def test_the_25_x_72_backward_takes_two_z_blocks_at_any_row_length(P):
    from ms_gat_amd import _lib
    assert _lib.contract_form_name(25, 72, False, P, True) == "k_chanpair_glds<2,3,128,3,1> nzb=2"


def test_every_other_registry_form_is_what_it_was():
    from ms_gat_amd import _lib
    P = 883 * 12
    assert _lib.contract_form_name(17, 48, False, P, True) == "k_chanpair_glds<2,3,128,3,1>"
    assert _lib.contract_form_name(33, 96, False, P, True) == "k_chanpair_glds<3,6,64,3,2>"
    assert _lib.contract_form_name(98, 72, True, P, True) == "k_chanpair_glds<7,5,64,3,2>"
    assert _lib.contract_form_name(72, 72, True, P, True) == "k_chanpair_glds<5,5,64,3,2>"
    # the rule covers the measured [25 x 72] block alone: a row or a column more or less keeps the one-block form
    assert _lib.contract_form_name(24, 72, False, P, True) == "k_chanpair_glds<2,5,128,3,1>"
    assert _lib.contract_form_name(25, 72, True, P, True) == "k_chanpair_glds<2,5,128,3,1>"
    assert "nzb" not in _lib.contract_form_name(25, 80, False, P, True)
    # the plain contraction (no mix output) of the same shape is not touched by the rule
    assert _lib.contract_form_name(25, 72, False, P, False).startswith("k_chanpair_glds<2,5,128,3,0>")
