"""Pose from source frames (frame_cases.py) on the MI355X: up_crop_to_nhwc against the two calls it replaces, its frame indexing,
valid extents and refusals, one launch of more than 2^21 output pixels, and the four plan programs that start from frames.  Every
comparison is bit for bit or integer-exact."""
import pytest
import torch

import frame_cases as fc
import protocol_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_crop_equals_two_calls(case):
    fc.kernel_case(DEV, case)


def test_identity_equals_normalize():
    fc.identity_case(DEV)


def test_frame_indexing():
    fc.frame_index_case(DEV)


def test_valid_extent_per_frame():
    fc.valid_case(DEV)


def test_frame_index_out_of_range():
    fc.bad_frame_case(DEV)


def test_more_than_2_21_pixels():
    fc.big_case(DEV)


def test_crop_refusals():
    fc.refusal_case(DEV)


@pytest.mark.parametrize("case", fc.plan_cases(pc.PLAN_CASES_GPU), ids=fc.plan_id)
def test_plan_from_frames(case):
    fc.plan_case(DEV, **case)


def test_plan_from_frames_unset_weights_refused():
    fc.plan_unset_case(DEV)
