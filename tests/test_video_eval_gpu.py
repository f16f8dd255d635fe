"""The evaluation entries of the video plan on the MI355X (tests/video_eval_cases.py): the four clip kernels alone, the plan
programs at three small configurations (K=13 32x40; K=15 39x39, the widened hand-over; K=13 64x72 at output stride 8), and one
VideoTrainer validation epoch with the flip test.  Equal bits to the compositions of the existing entries throughout."""
import os

import pytest
import torch

import video_eval_cases as vc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PLANS = [dict(K=13, B=2, T=3, H=32, W=40), dict(K=15, B=2, T=2, H=39, W=39), dict(K=13, B=1, T=2, H=64, W=72, output_stride=8)]


def _id(cfg):
    return "K{K}-B{B}-T{T}-{H}x{W}".format(**cfg) + ("-os8" if cfg.get("output_stride") == 8 else "")


@pytest.fixture(params=PLANS, ids=_id)
def plan_ctx(request):
    return vc.ctx(DEV, **request.param)


@pytest.mark.parametrize("bt,hw", vc.LAYOUT_CASES)
def test_clip_layout_flip(bt, hw):
    vc.layout_flip_case(DEV, bt, hw)


@pytest.mark.parametrize("bt,hw,coff", vc.POOL_CASES)
def test_clip_pool_flip(bt, hw, coff):
    vc.pool_flip_case(DEV, bt, hw, coff)


@pytest.mark.parametrize("bt,layout", vc.DECODE_CASES)
def test_clip_heatmap_decode(bt, layout):
    vc.clip_decode_case(DEV, bt, layout)


@pytest.mark.parametrize("bt,layout", vc.DECODE_CASES)
def test_clip_final_preds(bt, layout):
    vc.clip_final_case(DEV, bt, layout)


def test_clip_kernel_refusals():
    vc.kernel_refusal_case(DEV)


def test_lstm_plan_clip_keypoints(plan_ctx):
    vc.plan_keypoints_case(plan_ctx)


def test_lstm_plan_clip_flip(plan_ctx):
    vc.plan_flip_case(plan_ctx)


def test_lstm_plan_clip_final_preds(plan_ctx):
    vc.plan_final_case(plan_ctx)


def test_lstm_plan_stream(plan_ctx):
    vc.plan_stream_case(plan_ctx)


def test_lstm_plan_eval_workspaces_and_refusals(plan_ctx):
    vc.plan_workspace_case(plan_ctx)


def test_lstm_plan_eval_unset_weights():
    vc.plan_unset_case(DEV)


def test_lstm_plan_eval_argument_checks(plan_ctx):
    vc.plan_argument_case(plan_ctx)


def test_video_trainer_flip_test():
    os.environ["UNIPOSE_NO_TQDM"] = "1"
    vc.trainer_case(DEV)
