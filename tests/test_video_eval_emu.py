"""The evaluation entries of the video plan on the CPU emulator (tests/video_eval_cases.py): the four clip kernels alone — the
layout kernel's output and the decode kernels' maps ending right before an inaccessible page (tests/emu/guard_alloc.py) — the plan
programs at K=13, B=1, T=2, 32x32, and one VideoTrainer validation epoch with the flip test."""
import os

import pytest

import video_eval_cases as vc


def _guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return guarded


@pytest.mark.parametrize("bt,hw", vc.LAYOUT_CASES)
def test_clip_layout_flip_emu(emu_backend, bt, hw):
    vc.layout_flip_case(emu_backend, bt, hw, _guard())


@pytest.mark.parametrize("bt,hw,coff", vc.POOL_CASES)
def test_clip_pool_flip_emu(emu_backend, bt, hw, coff):
    vc.pool_flip_case(emu_backend, bt, hw, coff)


@pytest.mark.parametrize("bt,layout", vc.DECODE_CASES)
def test_clip_heatmap_decode_emu(emu_backend, bt, layout):
    vc.clip_decode_case(emu_backend, bt, layout, _guard())


@pytest.mark.parametrize("bt,layout", vc.DECODE_CASES)
def test_clip_final_preds_emu(emu_backend, bt, layout):
    vc.clip_final_case(emu_backend, bt, layout, _guard())


def test_clip_kernel_refusals_emu(emu_backend):
    vc.kernel_refusal_case(emu_backend)


def test_lstm_plan_clip_keypoints_emu(emu_backend):
    vc.plan_keypoints_case(vc.ctx(emu_backend))


def test_lstm_plan_clip_flip_emu(emu_backend):
    vc.plan_flip_case(vc.ctx(emu_backend))


def test_lstm_plan_clip_final_preds_emu(emu_backend):
    vc.plan_final_case(vc.ctx(emu_backend))


def test_lstm_plan_stream_emu(emu_backend):
    vc.plan_stream_case(vc.ctx(emu_backend))


def test_lstm_plan_eval_workspaces_and_refusals_emu(emu_backend):
    vc.plan_workspace_case(vc.ctx(emu_backend))
    vc.plan_unset_case(emu_backend)


def test_lstm_plan_eval_argument_checks_emu(emu_backend):
    vc.plan_argument_case(vc.ctx(emu_backend))


def test_video_trainer_flip_test_emu(emu_backend):
    os.environ["UNIPOSE_NO_TQDM"] = "1"
    vc.trainer_case(emu_backend)
