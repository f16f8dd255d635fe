"""The fused convolution epilogues alone against float64 (epilogue_cases.py) on a GPU-less box: the HIP sources compiled against
the fiber emulator (tests/emu).  The bounds are those of test_epilogue_gpu.py; its docstring lists the worst got / bound ratios
of both and the seeded faults that these tests catch.  The 96 tests of this file take about 21 s here."""
import pytest

import epilogue_cases as ex


@pytest.mark.parametrize("fam", ex.FWD_FAMILIES, ids=ex.fam_id)
def test_forward_eval_epilogue_against_float64(emu_backend, fam):
    ex.fwd_eval_case(emu_backend, fam)


@pytest.mark.parametrize("fam", ex.FWD_F32OUT, ids=ex.fam_id)
def test_forward_eval_epilogue_fp32_output_of_bf16_storage(emu_backend, fam):
    ex.fwd_eval_case(emu_backend, fam, f32out=True)


@pytest.mark.parametrize("fam", ex.STATS_FAMILIES, ids=ex.fam_id)
def test_forward_statistics_and_fold_against_float64(emu_backend, fam):
    ex.fwd_stats_case(emu_backend, fam)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32_entry", "bf16_entry"])
def test_forward_epilogue_refusals(emu_backend, bf16):
    ex.fwd_refusal_case(emu_backend, bf16)


@pytest.mark.parametrize("case", ex.GROUPED, ids=lambda c: "g%d_%dx%d_p%d" % c)
def test_forward_row_groups_against_float64(emu_backend, case):
    ex.fwd_grouped_case(emu_backend, *case)


def test_forward_row_groups_refusals(emu_backend):
    ex.fwd_grouped_refusal_case(emu_backend)


@pytest.mark.parametrize("case", ex.DGRAD, ids=ex.fam_id)
def test_data_gradient_epilogue_against_float64(emu_backend, case):
    ex.dgrad_case(emu_backend, case)


def test_data_gradient_epilogue_refusals(emu_backend):
    ex.dgrad_refusal_case(emu_backend)
