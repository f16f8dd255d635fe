"""The one-pass flip test on the MI355X (tests/flip_one_pass_cases.py): the _strided clip kernels and up_clip_flip_merge alone, the
create-time checks, the flagged image plan at three configurations (K=14 B=1 64x64 in both storages; K=14 B=2 52x68; K=16 B=2
48x48 at output stride 8 with the box head) and the flagged video plan at three (K=13 B=1 T=2 32x40 and K=15 B=2 T=3 39x39 in both
storages; K=13 B=1 T=2 64x72 at output stride 8), each against an unflagged plan of twice the batch.  Equal bits throughout; the
float64 comparisons hold the project's own bars for fp32 plans."""
import pytest
import torch

import flip_one_pass_cases as oc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("bt,hw", oc.LAYOUT_CASES)
def test_clip_layout_strided(bt, hw):
    oc.layout_strided_case(DEV, bt, hw)


@pytest.mark.parametrize("bt,hw,coff", oc.POOL_CASES)
def test_clip_pool_strided(bt, hw, coff):
    oc.pool_strided_case(DEV, bt, hw, coff)


@pytest.mark.parametrize("bt,hw,sigma", oc.CENTER_CASES)
def test_clip_center_pool_strided(bt, hw, sigma):
    oc.center_pool_strided_case(DEV, bt, hw, sigma)


@pytest.mark.parametrize("bt,typ", oc.CROP_CASES)
def test_clip_crop_strided(bt, typ):
    oc.crop_strided_case(DEV, bt, typ)


def test_clip_strided_refusals():
    oc.strided_refusal_case(DEV)


def test_clip_flip_merge():
    oc.clip_merge_case(DEV)


def test_clip_flip_merge_refusals():
    oc.clip_merge_refusal_case(DEV)


def test_plan_create_ex():
    oc.create_case(DEV)
    oc.argument_case(DEV)


@pytest.fixture(params=oc.IMAGE_STORAGES, ids=lambda p: "%s-case%d" % p)
def image(request):
    return oc.image_ctx(DEV, *request.param)


def test_image_plan_other_rows(image):
    oc.image_plain_rows_case(image)


def test_image_plan_flip_one_pass(image):
    oc.image_flip_case(image)


def test_image_plan_flip_one_pass_frames(image):
    oc.image_frames_case(image)


def test_image_plan_flip_one_pass_workspace(image):
    oc.image_workspace_case(image)


def test_image_plan_flip_one_pass_float64(image):
    oc.image_float64_case(image)


def test_image_plan_create_t_is_create_ex():
    oc.image_create_t_case(oc.image_ctx(DEV, "f32", 0))


@pytest.fixture(params=oc.VIDEO_STORAGES, ids=lambda p: "%s-case%d" % p)
def video(request):
    return oc.video_ctx(DEV, *request.param)


def test_lstm_plan_other_rows(video):
    oc.video_plain_rows_case(video)


def test_lstm_plan_flip_one_pass(video):
    oc.video_flip_case(video)


def test_lstm_plan_flip_one_pass_frames(video):
    oc.video_frames_case(video)


def test_lstm_plan_flip_one_pass_workspace(video):
    oc.video_workspace_case(video)


def test_lstm_plan_flip_one_pass_float64(video):
    oc.video_float64_case(video)


def test_lstm_plan_create_t_is_create_ex():
    oc.video_create_t_case(oc.video_ctx(DEV, "f32", 0))
