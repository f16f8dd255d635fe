"""Training targets of the box head and the bbox=True model in train mode (box_target_cases.py) on a real MI355X: the cases of
test_box_targets_emu.py and one batch of 1100 samples on 46 x 46 maps, 2 327 600 output pixels (more than 2^21) in one launch.

up_make_box_maps against the reference's getBoundingBox (G19) and its numpy restatement, over every case of this file:
    worst float32-ulp difference      emulator 0   MI355X 0     (every map equals numpy's bit for bit; the rule allows 1)
    elements flipped across the cut   emulator 0   MI355X 0     (must be 0)
Train step of the bbox=True model (K = 14, B = 2, 32 x 32), error against the fp64 oracle, ours / the fp32 oracle's own, MI355X:
joint maps 6.9e-5 / 8.3e-5, box maps 7.4e-5 / 1.0e-4, loss 7.6e-7 / 4.4e-6.
The 44 tests of this file take about 6 s on the GPU (the slowest, one epoch of the trainer, 2.2 s).
"""
import pytest
import torch

import box_target_cases as bx

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZE_IDS = ["%dx%d_s%g" % s for s in bx.SIZES]


def test_restatement_equals_reference(golden_dir):
    bx.restatement_case(golden_dir)


def test_entry_equals_reference(golden_dir):
    bx.golden_case(DEV, golden_dir)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("k", bx.KS)
@pytest.mark.parametrize("size", bx.SIZES, ids=SIZE_IDS)
def test_entry_equals_restatement(size, k, b):
    bx.shape_case(DEV, size, k, b)


def test_failing_sample_in_the_middle():
    bx.middle_failure_case(DEV)


def test_other_sigmas():
    bx.sigma_case(DEV)


def test_more_than_2_21_output_pixels():
    bx.big_case(DEV)


def test_round_trip_with_the_decoder():
    bx.roundtrip_case(DEV)


def test_refusals():
    bx.refusal_case(DEV)


def test_empty_sample_policy():
    bx.empty_policy_case(DEV)


def test_bbox_model_train_step_vs_oracle():
    bx.bbox_train_case(DEV)


def test_batcher_box_maps():
    bx.batcher_case(DEV)


def test_trainer_with_box_head(monkeypatch):
    monkeypatch.setenv("UNIPOSE_NO_TQDM", "1")
    bx.trainer_case(DEV)


def test_zz_report():
    print("\n" + bx.report() + " (MI355X)")
    assert bx.WORST["flipped"] == 0
