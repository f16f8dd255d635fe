"""The video plan from source frames on the MI355X (tests/video_frame_cases.py): the clip crop against the batch crop, one launch of
more than 2^21 output pixels included, the three centre-pool entries against up_make_gaussian_maps and the pooling entries, and the
plan programs at three small configurations (K=13 32x40; K=15 39x39, the widened hand-over; K=13 64x72 at output stride 8).  Equal
bits to the compositions of the existing entries throughout."""
import pytest
import torch

import video_frame_cases as vf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PLANS = [dict(K=13, B=2, T=2, H=32, W=40), dict(K=15, B=2, T=2, H=39, W=39), dict(K=13, B=1, T=2, H=64, W=72, output_stride=8)]


def _id(cfg):
    return "K{K}-B{B}-T{T}-{H}x{W}".format(**cfg) + ("-os8" if cfg.get("output_stride") == 8 else "")


@pytest.fixture(params=PLANS, ids=_id)
def frame_ctx(request):
    return vf.frame_ctx(DEV, **request.param)


@pytest.mark.parametrize("case", vf.CLIP_CASES, ids=vf.CLIP_IDS)
def test_clip_crop_equals_batch_crop(case):
    vf.clip_crop_case(DEV, case)


def test_clip_crop_ops():
    vf.clip_ops_case(DEV)


def test_clip_crop_valid_extent_per_frame():
    vf.clip_valid_case(DEV)


def test_clip_crop_frame_index_out_of_range():
    vf.clip_bad_frame_case(DEV)


def test_clip_crop_more_than_2p21_pixels():
    vf.clip_big_case(DEV)


@pytest.mark.parametrize("case", vf.POOL_CLIP_CASES, ids=vf._pool_id)
def test_clip_center_pool_equals_two_calls(case):
    vf.center_pool_case(DEV, case)


@pytest.mark.parametrize("case", vf.POOL_PLAIN_CASES, ids=vf._pool_id)
def test_center_pool_equals_two_calls(case):
    vf.center_pool_case(DEV, case)


def test_video_frame_kernel_refusals():
    vf.kernel_refusal_case(DEV)


def test_lstm_plan_clip_frame_heatmaps(frame_ctx):
    vf.plan_heatmaps_case(frame_ctx)


def test_lstm_plan_clip_frame_flip(frame_ctx):
    vf.plan_flip_case(frame_ctx)


def test_lstm_plan_clip_frame_final_preds(frame_ctx):
    vf.plan_final_case(frame_ctx)


def test_lstm_plan_stream_frames(frame_ctx):
    vf.plan_stream_case(frame_ctx)


def test_lstm_plan_frame_workspaces_and_refusals(frame_ctx):
    vf.plan_workspace_case(frame_ctx)


def test_lstm_plan_frame_unset_weights():
    vf.plan_unset_case(DEV)


def test_lstm_plan_frame_argument_checks(frame_ctx):
    vf.plan_argument_case(frame_ctx)
