"""Every BatchNorm entry of the C ABI alone against float64, per element and per channel, at the edge shapes of every code path
(bn_cases.py), on a real MI355X.

Worst got / bound ratios per quantity (bounds: bn_cases.py), emulator / MI355X:
(z, dy of bf16 storage and the merge-only cases are listed apart: one stored bf16 rounding is up to 2^-8 of the value and a correctly
rounded fp32 mean up to u |mean64|, so those fill their bounds by construction.)
    apply       z 0.808 / 0.621        z (bf16) 0.996 / 0.996
    statistics  mean 0.688 / 0.688     invstd 0.228 / 0.228   scale 0.365 / 0.365   shift 0.340 / 0.270
                running_mean 0.709 / 0.454   running_var 0.689 / 0.453   exact-stats M2 0.995 / 0.995
    merge only  mean 0.967 / 0.967     invstd 0.469 / 0.469   scale 0.497 / 0.497   shift 0.636 / 0.636
                running_mean 0.790 / 0.624   running_var 0.716 / 0.470
    backward    dbeta 0.175 / 0.175    dgamma 0.182 / 0.182   dy 0.252 / 0.252   dy (bf16) 0.995 / 0.995
                dy, use_batch_stats = 0: 0.941 / 0.941 (bf16 0.995 / 0.995)
                finalized entries: dy 0.596 / 0.578 (bf16 0.993 / 0.993), use_batch_stats = 0: 0.912 / 0.912 (bf16 0.978 / 0.978)
Where the two differ the GPU build contracts a product and a sum into one FMA and the host build of the emulator does not.
The first run found one miscounted derivation, no kernel fault: the M2 bound lacked the first-order term of the fp32 lane merges
(bn_cases.py, "Found by the first run"); the |mean| / std = 4000 channel of the 9-group case reached 1.44 of the bound without it.
The 263 tests of this file take about 5 s on the GPU (the slowest 0.25 s), about 20 s on the emulator.
"""
import pytest
import torch

import bn_cases as bx

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("shape", bx.SHAPES, ids=bx.shape_id)
def test_bn_apply_against_float64(shape):
    bx.apply_case(DEV, shape)


@pytest.mark.parametrize("shape", bx.STATS_SHAPES, ids=bx.shape_id)
def test_bn_statistics_and_finalize_against_float64(shape):
    bx.stats_case(DEV, shape)


@pytest.mark.parametrize("shape", bx.SHAPES, ids=bx.shape_id)
def test_bn_backward_against_float64(shape):
    bx.bwd_case(DEV, shape)


@pytest.mark.parametrize("shape", bx.ACC_SHAPES, ids=bx.shape_id)
def test_bn_backward_accumulators(shape):
    bx.bwd_acc_case(DEV, shape)


@pytest.mark.parametrize("chunks", bx.PREREDUCED_CHUNKS)
@pytest.mark.parametrize("shape", bx.PREREDUCED_SHAPES, ids=bx.shape_id)
def test_bn_backward_prereduced_and_finalized(shape, chunks):
    bx.bwd_prereduced_case(DEV, shape, chunks)


@pytest.mark.parametrize("case", bx.GROUPS, ids=bx.group_id)
def test_bn_groups(case):
    bx.groups_case(DEV, case)


def test_bn_groups_refuse_relu_bits_off_a_word_boundary():
    bx.groups_refusal_case(DEV)


@pytest.mark.parametrize("c", bx.FINALIZE_C)
@pytest.mark.parametrize("tiles", bx.FINALIZE_TILES)
def test_bn_finalize_synthetic_partials(tiles, c):
    bx.finalize_synthetic_case(DEV, tiles, c)


@pytest.mark.parametrize("tiles,c,groups", [(2, 4, 3), (33, 68, 3), (65, 132, 8), (513, 68, 2)])
def test_bn_finalize_groups_synthetic_partials(tiles, c, groups):
    bx.finalize_synthetic_case(DEV, tiles, c, groups)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", bx.EXACT, ids=lambda s: "g%d_r%d_c%d" % s)
def test_bn_exact_stats(case, dtype):
    bx.exact_stats_case(DEV, *case, dtype)


@pytest.mark.parametrize("c", [1, 4, 255, 257])
def test_bn_eval_coeffs(c):
    bx.eval_coeffs_case(DEV, c)


@pytest.mark.parametrize("n", [1, 255, 257, 65537])
def test_relu_bwd(n):
    bx.relu_bwd_case(DEV, n)
