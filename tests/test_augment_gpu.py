"""Augmentation on the device (augment_cases.py) on a real MI355X: the cases of test_augment_emu.py (without its guard pages) and one
launch of 20 images at 368 x 368 from 400 x 300 uint8 sources, 2 708 480 output pixels (more than 2^21: a second grid trip).
The fixture G20 holds the reference's point arithmetic and its numpy image steps (crop, hflip, normalize); nothing of the
reference's image resampling could be recorded, because OpenCV is absent where the fixture is made.

up_augment_image against the float64 restatement of its documented semantics, worst error / bound (augment_cases.BOUND notes) over
every case of this file:    emulator 0.146    MI355X 0.212 (the 2.7 M pixel launch; 0.146 without it)
"""
import pytest
import torch

import augment_cases as ac

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_restatement_equals_reference(golden_dir):
    ac.restatement_case(golden_dir)


def test_entry_equals_reference(golden_dir):
    ac.golden_case(DEV, golden_dir)


def test_identity_equals_normalize():
    ac.identity_case(DEV)


@pytest.mark.parametrize("case", ac.CASES, ids=ac.CASE_IDS)
def test_entry_equals_float64(case):
    ac.float64_case(DEV, case)


def test_cases_sample_the_source():
    ac.coverage_case(DEV)


def test_all_taps_outside_and_huge_coordinates():
    ac.outside_case(DEV)


def test_padding_is_never_read():
    ac.padding_case(DEV)


def test_points_follow_pixels():
    ac.follow_case(DEV)


def test_more_than_2_21_output_pixels():
    ac.big_case(DEV)


def test_refusals():
    ac.refusal_case(DEV)


@pytest.mark.parametrize("bbox", [False, True], ids=["plain", "bbox"])
def test_batcher_augment(bbox):
    ac.batcher_case(DEV, bbox)


def test_batcher_augment_clip():
    ac.clip_case(DEV)


def test_trainer_with_augment(monkeypatch):
    monkeypatch.setenv("UNIPOSE_NO_TQDM", "1")
    ac.trainer_case(DEV)


def test_zz_report():
    print("\n" + ac.report() + " (MI355X)")
    assert ac.WORST["elements"] > 0 and ac.WORST["ratio"] <= 1.0
