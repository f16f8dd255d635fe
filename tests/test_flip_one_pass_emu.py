"""The one-pass flip test on the CPU emulator (tests/flip_one_pass_cases.py): the _strided clip kernels and up_clip_flip_merge alone,
their destinations ending right before an inaccessible page (tests/emu/guard_alloc.py); the create-time checks; the flagged image
plan at K=14, B=1, 64x64 in both storages and the flagged video plan at K=13, B=1, T=2, 32x40 in both storages, each against an
unflagged plan of twice the batch."""
import pytest

import flip_one_pass_cases as oc

IMAGE = [("f32", 0), ("bf16", 0)]
VIDEO = [("f32", 0), ("bf16", 0)]


def _guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return guarded


@pytest.mark.parametrize("bt,hw", oc.LAYOUT_CASES)
def test_clip_layout_strided_emu(emu_backend, bt, hw):
    oc.layout_strided_case(emu_backend, bt, hw, _guard())


@pytest.mark.parametrize("bt,hw,coff", oc.POOL_CASES)
def test_clip_pool_strided_emu(emu_backend, bt, hw, coff):
    oc.pool_strided_case(emu_backend, bt, hw, coff, _guard())


@pytest.mark.parametrize("bt,hw,sigma", oc.CENTER_CASES)
def test_clip_center_pool_strided_emu(emu_backend, bt, hw, sigma):
    oc.center_pool_strided_case(emu_backend, bt, hw, sigma, _guard())


@pytest.mark.parametrize("bt,typ", oc.CROP_CASES)
def test_clip_crop_strided_emu(emu_backend, bt, typ):
    oc.crop_strided_case(emu_backend, bt, typ, _guard())


def test_clip_strided_refusals_emu(emu_backend):
    oc.strided_refusal_case(emu_backend)


def test_clip_flip_merge_emu(emu_backend):
    oc.clip_merge_case(emu_backend, _guard())


def test_clip_flip_merge_refusals_emu(emu_backend):
    oc.clip_merge_refusal_case(emu_backend)


def test_plan_create_ex_emu(emu_backend):
    oc.create_case(emu_backend)
    oc.argument_case(emu_backend)


@pytest.fixture(params=IMAGE, ids=lambda p: "%s-case%d" % p)
def image(request, emu_backend):
    return oc.image_ctx(emu_backend, *request.param)


def test_image_plan_other_rows_emu(image):
    oc.image_plain_rows_case(image)


def test_image_plan_flip_one_pass_emu(image):
    oc.image_flip_case(image)


def test_image_plan_flip_one_pass_frames_emu(image):
    oc.image_frames_case(image)


def test_image_plan_flip_one_pass_workspace_emu(image):
    oc.image_workspace_case(image)


def test_image_plan_flip_one_pass_float64_emu(image):
    oc.image_float64_case(image)


def test_image_plan_create_t_is_create_ex_emu(emu_backend):
    oc.image_create_t_case(oc.image_ctx(emu_backend, "f32", 0))


@pytest.fixture(params=VIDEO, ids=lambda p: "%s-case%d" % p)
def video(request, emu_backend):
    return oc.video_ctx(emu_backend, *request.param)


def test_lstm_plan_other_rows_emu(video):
    oc.video_plain_rows_case(video)


def test_lstm_plan_flip_one_pass_emu(video):
    oc.video_flip_case(video)


def test_lstm_plan_flip_one_pass_frames_emu(video):
    oc.video_frames_case(video)


def test_lstm_plan_flip_one_pass_workspace_emu(video):
    oc.video_workspace_case(video)


def test_lstm_plan_flip_one_pass_float64_emu(video):
    oc.video_float64_case(video)


def test_lstm_plan_create_t_is_create_ex_emu(emu_backend):
    oc.video_create_t_case(oc.video_ctx(emu_backend, "f32", 0))
