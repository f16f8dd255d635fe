"""Every BatchNorm entry of the C ABI alone against float64, per element and per channel, at the edge shapes of every code path
(bn_cases.py), on a GPU-less box: the HIP sources compiled against the fiber emulator (tests/emu).  The bounds are those of
test_bn_gpu.py; its docstring lists the worst got / bound ratios of both.  The 263 tests
of this file take about 20 s here."""
import pytest
import torch

import bn_cases as bx


@pytest.mark.parametrize("shape", bx.SHAPES, ids=bx.shape_id)
def test_bn_apply_against_float64(emu_backend, shape):
    bx.apply_case(emu_backend, shape)


@pytest.mark.parametrize("shape", bx.STATS_SHAPES, ids=bx.shape_id)
def test_bn_statistics_and_finalize_against_float64(emu_backend, shape):
    bx.stats_case(emu_backend, shape)


@pytest.mark.parametrize("shape", bx.SHAPES, ids=bx.shape_id)
def test_bn_backward_against_float64(emu_backend, shape):
    bx.bwd_case(emu_backend, shape)


@pytest.mark.parametrize("shape", bx.ACC_SHAPES, ids=bx.shape_id)
def test_bn_backward_accumulators(emu_backend, shape):
    bx.bwd_acc_case(emu_backend, shape)


@pytest.mark.parametrize("chunks", bx.PREREDUCED_CHUNKS)
@pytest.mark.parametrize("shape", bx.PREREDUCED_SHAPES, ids=bx.shape_id)
def test_bn_backward_prereduced_and_finalized(emu_backend, shape, chunks):
    bx.bwd_prereduced_case(emu_backend, shape, chunks)


@pytest.mark.parametrize("case", bx.GROUPS, ids=bx.group_id)
def test_bn_groups(emu_backend, case):
    bx.groups_case(emu_backend, case)


def test_bn_groups_refuse_relu_bits_off_a_word_boundary(emu_backend):
    bx.groups_refusal_case(emu_backend)


@pytest.mark.parametrize("c", bx.FINALIZE_C)
@pytest.mark.parametrize("tiles", bx.FINALIZE_TILES)
def test_bn_finalize_synthetic_partials(emu_backend, tiles, c):
    bx.finalize_synthetic_case(emu_backend, tiles, c)


@pytest.mark.parametrize("tiles,c,groups", [(2, 4, 3), (33, 68, 3), (65, 132, 8), (513, 68, 2)])
def test_bn_finalize_groups_synthetic_partials(emu_backend, tiles, c, groups):
    bx.finalize_synthetic_case(emu_backend, tiles, c, groups)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", bx.EXACT, ids=lambda s: "g%d_r%d_c%d" % s)
def test_bn_exact_stats(emu_backend, case, dtype):
    bx.exact_stats_case(emu_backend, *case, dtype)


@pytest.mark.parametrize("c", [1, 4, 255, 257])
def test_bn_eval_coeffs(emu_backend, c):
    bx.eval_coeffs_case(emu_backend, c)


@pytest.mark.parametrize("n", [1, 255, 257, 65537])
def test_relu_bwd(emu_backend, n):
    bx.relu_bwd_case(emu_backend, n)
