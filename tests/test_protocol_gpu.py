"""The evaluation protocol around the forward (protocol_cases.py) on the MI355X: up_nchw_to_nhwc_flip, up_flip_merge,
up_final_preds, the two plan programs and the trainer's flip test.  Every comparison is bit for bit or integer-exact."""
import pytest
import torch

import protocol_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_final_preds_equals_reference(golden_dir):
    pc.final_golden_case(DEV, golden_dir)


def test_final_preds_variants():
    pc.final_variants_case(DEV)


def test_final_preds_refusals():
    pc.final_refusal_case(DEV)


def test_flip_merge_equals_numpy():
    pc.merge_case(DEV)


def test_flip_merge_equals_flip_back(golden_dir):
    pc.merge_golden_case(DEV, golden_dir)


def test_flip_merge_refusals():
    pc.merge_refusal_case(DEV)


def test_layout_pass_with_mirror():
    pc.layout_flip_case(DEV)


def test_semantics():
    pc.semantics_case(DEV)


@pytest.mark.parametrize("case", pc.PLAN_CASES_GPU, ids=pc.plan_id)
def test_plan_flip_and_final_preds(case):
    pc.plan_case(DEV, **case)


def test_plan_unset_weights_refused():
    pc.plan_unset_case(DEV)


@pytest.mark.parametrize("bbox", [False, True], ids=["plain", "bbox"])
def test_trainer_flip_test(bbox, monkeypatch):
    monkeypatch.setenv("UNIPOSE_NO_TQDM", "1")
    pc.trainer_case(DEV, bbox)
