"""The evaluation and data-contract entries of the C ABI off the square maps (contract_cases.py) on a real MI355X: the cases of
test_contract_emu.py and two of more than 2 M elements, which run the second trip of a grid-stride loop.

ConvLSTM gate entries, worst |got - ref64| / (u m) per output (bound K_LSTM = 16, fixed from the host's float32 evaluation of the
same formulas, worst 3.129: contract_cases.py), emulator / MI355X:
    lstm0_fwd  cell 2.411 / 2.295   hide 2.768 / 2.482        lstm0_bwd  dgates 2.779 / 3.029
    lstm_fwd   cell 2.364 / 2.171   hide 2.300 / 1.893        lstm_bwd   dgates 3.000 / 3.090   dcprev 3.030 / 2.993
(the MI355X column includes the 43 700-row case).  Everything else in this file is an equality and held at the first run.
The division by a number that is no power of two (up_normalize_image with std 58.395): 0 float32 ulps off torch's CPU division on
the MI355X at every shape, i.e. the kernel's `/` is correctly rounded there (the library is built without fast-math); the test
stays an equality of bits and the kernel is unchanged.
The 192 tests of this file take about 4 s on the GPU (the slowest 0.5 s), about 5 s on the emulator.
"""
import pytest
import torch

import contract_cases as cx

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


@pytest.mark.parametrize("shape", cx.ARGMAX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_argmax_rectangles_and_wavefront_edges(shape):
    cx.argmax_shape_case(DEV, shape)


def test_argmax_planted_ties_nan_inf():
    cx.argmax_planted_case(DEV)


@pytest.mark.parametrize("stack", cx.G18_STACKS)
def test_pck_equals_reference_on_rectangles(golden_dir, stack):
    cx.pck_golden_case(DEV, golden_dir, stack)


@pytest.mark.parametrize("j", [70, 256])
@pytest.mark.parametrize("ds", cx.O.DATASETS)
def test_pck_many_joints(ds, j):
    cx.pck_oracle_case(DEV, ds, j)


@pytest.mark.parametrize("mode", [None, "all_invisible", "joint0_invisible"])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("ds", cx.O.DATASETS)
def test_pck_batch_of_one_and_invisible_joints(ds, b, mode):
    cx.pck_oracle_case(DEV, ds, cx.NEED[ds] + 5, b, mode)


def test_pck_refusals():
    cx.pck_refusal_case(DEV)


@pytest.mark.parametrize("case", cx.HEATMAP_CASES, ids=lambda c: "%dx%d_s%g" % c[:3])
def test_target_heatmaps_non_square(case):
    cx.heatmaps_case(DEV, case)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", cx.CENTERMAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_centre_maps(size, n):
    cx.centermaps_case(DEV, size, n)


@pytest.mark.parametrize("divisor", cx.NORMALIZE_DIVISORS, ids=["pow2", "58.395"])
@pytest.mark.parametrize("shape", cx.NORMALIZE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_normalize_image_bits(shape, divisor):
    cx.normalize_case(DEV, shape, divisor)


@pytest.mark.parametrize("rows", cx.LSTM_ROWS)
@pytest.mark.parametrize("cg", cx.LSTM_CG)
def test_lstm0_entries_per_element(cg, rows):
    cx.lstm0_case(DEV, cg, rows)


@pytest.mark.parametrize("rows", cx.LSTM_ROWS)
@pytest.mark.parametrize("cg", cx.LSTM_CG)
def test_lstm_entries_per_element(cg, rows):
    cx.lstm_case(DEV, cg, rows)


def test_lstm_entries_second_grid_trip():
    """Cg = 48, 43 700 rows: 2 097 600 elements, 448 past the 8192 x 256 the grid covers in one trip"""
    cg, rows = cx.LSTM_BIG
    assert rows * cg > 8192 * 256
    cx.lstm0_case(DEV, cg, rows, scales=(1.0,), lds=[(3 * cg + 8, cg + 4, None)])
    cx.lstm_case(DEV, cg, rows, scales=(1.0,), lds=[(4 * cg + 8, cg + 4, cg + 8)])


def test_lstm_refusals():
    cx.lstm_refusal_case(DEV)


@DTYPES
@pytest.mark.parametrize("p", cx.DROPOUT_P)
@pytest.mark.parametrize("n", cx.DROPOUT_N)
def test_dropout_mask_and_values(n, p, dtype):
    cx.dropout_case(DEV, n, p, dtype)


@DTYPES
def test_dropout_second_grid_trip(dtype):
    """n = 4 194 304 + 513: past the 16384 blocks of 256 the launch is capped at"""
    assert cx.DROPOUT_BIG > 16384 * 256
    cx.dropout_case(DEV, cx.DROPOUT_BIG, 0.3, dtype, seeds=(0x5EED,))


@DTYPES
def test_dropout_keeps_at_the_threshold(dtype):
    cx.dropout_threshold_case(DEV, dtype)


@DTYPES
def test_dropout_external_mask(dtype):
    cx.dropout_ext_mask_case(DEV, dtype)


@DTYPES
def test_dropout_step_counter(dtype):
    cx.dropout_step_case(DEV, dtype)


def test_dropout_refusals():
    cx.dropout_refusal_case(DEV)


def test_zz_report_worst_ratios():
    print("\nworst |got - ref64| / (u m) per entry (MI355X):\n" + cx.report())
