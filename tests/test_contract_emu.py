"""The evaluation and data-contract entries of the C ABI off the square maps (contract_cases.py) on a GPU-less box: the HIP sources
compiled against the fiber emulator (tests/emu).  The cases and bounds are those of test_contract_gpu.py, less its two cases of
more than 2 M elements; its docstring lists the worst ratios of both.  The 189 tests of this file take about 5 s here."""
import pytest
import torch

import contract_cases as cx

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


@pytest.mark.parametrize("shape", cx.ARGMAX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_argmax_rectangles_and_wavefront_edges(emu_backend, shape):
    cx.argmax_shape_case(emu_backend, shape)


def test_argmax_planted_ties_nan_inf(emu_backend):
    cx.argmax_planted_case(emu_backend)


@pytest.mark.parametrize("stack", cx.G18_STACKS)
def test_pck_equals_reference_on_rectangles(emu_backend, golden_dir, stack):
    cx.pck_golden_case(emu_backend, golden_dir, stack)


@pytest.mark.parametrize("j", [70, 256])
@pytest.mark.parametrize("ds", cx.O.DATASETS)
def test_pck_many_joints(emu_backend, ds, j):
    cx.pck_oracle_case(emu_backend, ds, j)


@pytest.mark.parametrize("mode", [None, "all_invisible", "joint0_invisible"])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("ds", cx.O.DATASETS)
def test_pck_batch_of_one_and_invisible_joints(emu_backend, ds, b, mode):
    cx.pck_oracle_case(emu_backend, ds, cx.NEED[ds] + 5, b, mode)


def test_pck_refusals(emu_backend):
    cx.pck_refusal_case(emu_backend)


@pytest.mark.parametrize("case", cx.HEATMAP_CASES, ids=lambda c: "%dx%d_s%g" % c[:3])
def test_target_heatmaps_non_square(emu_backend, case):
    cx.heatmaps_case(emu_backend, case)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", cx.CENTERMAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_centre_maps(emu_backend, size, n):
    cx.centermaps_case(emu_backend, size, n)


@pytest.mark.parametrize("divisor", cx.NORMALIZE_DIVISORS, ids=["pow2", "58.395"])
@pytest.mark.parametrize("shape", cx.NORMALIZE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_normalize_image_bits(emu_backend, shape, divisor):
    cx.normalize_case(emu_backend, shape, divisor)


@pytest.mark.parametrize("rows", cx.LSTM_ROWS)
@pytest.mark.parametrize("cg", cx.LSTM_CG)
def test_lstm0_entries_per_element(emu_backend, cg, rows):
    cx.lstm0_case(emu_backend, cg, rows)


@pytest.mark.parametrize("rows", cx.LSTM_ROWS)
@pytest.mark.parametrize("cg", cx.LSTM_CG)
def test_lstm_entries_per_element(emu_backend, cg, rows):
    cx.lstm_case(emu_backend, cg, rows)


def test_lstm_refusals(emu_backend):
    cx.lstm_refusal_case(emu_backend)


@DTYPES
@pytest.mark.parametrize("p", cx.DROPOUT_P)
@pytest.mark.parametrize("n", cx.DROPOUT_N)
def test_dropout_mask_and_values(emu_backend, n, p, dtype):
    cx.dropout_case(emu_backend, n, p, dtype)


@DTYPES
def test_dropout_keeps_at_the_threshold(emu_backend, dtype):
    cx.dropout_threshold_case(emu_backend, dtype)


@DTYPES
def test_dropout_external_mask(emu_backend, dtype):
    cx.dropout_ext_mask_case(emu_backend, dtype)


@DTYPES
def test_dropout_step_counter(emu_backend, dtype):
    cx.dropout_step_case(emu_backend, dtype)


def test_dropout_refusals(emu_backend):
    cx.dropout_refusal_case(emu_backend)


def test_zz_report_worst_ratios(emu_backend):
    print("\nworst |got - ref64| / (u m) per entry (emulator):\n" + cx.report())
