"""The fused convolution epilogues alone against float64 (epilogue_cases.py), on a real MI355X.

The 96 tests of this file take about 3.6 s on the GPU (the slowest 0.75 s: the first refusal case, which also loads the library; every
other one below 0.35 s) and about 21 s on the emulator (the slowest 2.7 s: the 3x3 big-tile forward case).

Worst got / bound ratios per quantity (bounds: epilogue_cases.py), emulator / MI355X:
    forward      y 0.408 / 0.408        y (bf16) 0.994 / 0.994     mean 0.019 / 0.020     M2 0.001 / 0.001
    fold         mean 0.022 / 0.023     invstd 0.001 / 0.001       scale 0.001 / 0.001    shift 0.001 / 0.001
                 running_mean 0.024 / 0.025    running_var 0.006 / 0.006
    data grad.   dx 0.049 / 0.049       dx (bf16) 0.993 / 0.993    S1 0.011 / 0.011       S2 0.011 / 0.011
                 dgamma 0.011 / 0.011   dbeta 0.010 / 0.010        gsum 0.014 / 0.014
y and dx of bf16 storage fill their bounds by construction (one stored rounding is up to 2^-8 of the value).  The statistics
bounds are worst-case chains of up to 142 roundings per tile mean and are filled to a few percent at most; what they exclude is
shown by the seeded faults below, not by the ratio.  The first runs found no kernel fault and no miscounted derivation.

Seeded faults (emulator only, in a scratch copy of the tree; each is a one-line change, -> the tests of test_epilogue_emu.py that
fail; a test id is test_<name>[<case>]):
    bf16s_glds.h, addend path: the reduction reads the unrounded v     -> data_gradient_epilogue[bf16_add, bf16_masked_add, bf16_dead]
    bf16s_glds.h: bn_invstd[cc + 1]                                    -> data_gradient_epilogue[every bf16_* case]
    f32_glds.h: invstd dropped from partial[..][1]                     -> data_gradient_epilogue[every f32_* case]
    bf16s_glds.h: sign bits indexed with (b & 15)                      -> data_gradient_epilogue[bf16_1x1, bf16_add, bf16_masked_add, bf16_3x3_*, bf16_dead]
    f32_glds.h: the mask of the reduced layer read one pixel off       -> data_gradient_epilogue[every f32_* case with a ReLU mask]
    f32_glds.h: ReLU before the residual add                           -> forward_eval_epilogue[epi1_*, breg_1x1, wide]
    igemm_store: bias added in esh and again behind it                 -> forward_eval_epilogue[reg_*, generic_*, epi0_*, breg_ring_epi0, bf16_reg_*], fp32_output[all]
    f32_glds.h: bn_grp_stride ignored (gmean = 0)                      -> data_gradient_epilogue[f32_groups2_3x3, f32_groups3_1x1, f32_groups3_3x3_t128]
    f32_glds.h: cnt += 1 for the dead rows of a ragged tile            -> forward_statistics_and_fold[epi1_* with a ragged tile, breg_1x1, wide], forward_row_groups[all]
    f32_glds.h: `live = nok` (dead rows of a ragged tile in the sums)  -> data_gradient_epilogue[f32_add, f32_masked_add, f32_masked_add_t128, f32_dead, f32_groups2_3x3]
    wf_merge: the d^2 n1 n2 / n term dropped                           -> forward_statistics_and_fold[all but bf16_big_*], forward_row_groups[all]
One change the issue lists fails NO test, and cannot: removing the `p1 >= 0` guard of the bf16 reduction without an addend
(bf16s_glds.h).  Rows past the end of a ragged tile have a tap mask of 0, their operand rows are zero-filled and their
accumulators are exactly 0, so with or without the guard they add +0 to both sums (0 * (y - mean) of the clamped, finite row 0).
The guard that does matter is the one of the addend paths, where the clamped row's addend makes a dead row's value non-zero:
that is the `live = nok` line above.
"""
import pytest
import torch

import epilogue_cases as ex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("fam", ex.FWD_FAMILIES, ids=ex.fam_id)
def test_forward_eval_epilogue_against_float64(fam):
    ex.fwd_eval_case(DEV, fam)


@pytest.mark.parametrize("fam", ex.FWD_F32OUT, ids=ex.fam_id)
def test_forward_eval_epilogue_fp32_output_of_bf16_storage(fam):
    ex.fwd_eval_case(DEV, fam, f32out=True)


@pytest.mark.parametrize("fam", ex.STATS_FAMILIES, ids=ex.fam_id)
def test_forward_statistics_and_fold_against_float64(fam):
    ex.fwd_stats_case(DEV, fam)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32_entry", "bf16_entry"])
def test_forward_epilogue_refusals(bf16):
    ex.fwd_refusal_case(DEV, bf16)


@pytest.mark.parametrize("case", ex.GROUPED, ids=lambda c: "g%d_%dx%d_p%d" % c)
def test_forward_row_groups_against_float64(case):
    ex.fwd_grouped_case(DEV, *case)


def test_forward_row_groups_refusals():
    ex.fwd_grouped_refusal_case(DEV)


@pytest.mark.parametrize("case", ex.DGRAD, ids=ex.fam_id)
def test_data_gradient_epilogue_against_float64(case):
    ex.dgrad_case(DEV, case)


def test_data_gradient_epilogue_refusals():
    ex.dgrad_refusal_case(DEV)
