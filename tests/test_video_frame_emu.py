"""The video plan from source frames (tests/video_frame_cases.py) on a GPU-less box: the HIP sources compiled against the fiber
emulator (tests/emu).  The outputs of the clip crop and of the centre pool end right in front of an inaccessible page
(tests/emu/guard_alloc.py), the sources of the crop too, and for the frame indices -1 and F the source also once begins right
behind one.  The plan programs run at K=13, B=1, T=2, 32x32 (video_eval_cases.ctx: one plan for both files).  The launch of more
than 2^21 output pixels runs on the GPU only (test_video_frame_gpu.py)."""
import pytest

import video_eval_cases as vc
import video_frame_cases as vf


def _guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return guarded


def _float_guard():
    g = _guard()
    return lambda shape: g(shape)


@pytest.mark.parametrize("case", vf.CLIP_CASES, ids=vf.CLIP_IDS)
def test_clip_crop_equals_batch_crop_emu(emu_backend, case):
    vf.clip_crop_case(emu_backend, case, _guard())


def test_clip_crop_ops_emu(emu_backend):
    vf.clip_ops_case(emu_backend)


def test_clip_crop_valid_extent_per_frame_emu(emu_backend):
    vf.clip_valid_case(emu_backend, _guard())


def test_clip_crop_frame_index_out_of_range_emu(emu_backend):
    vf.clip_bad_frame_case(emu_backend, _guard(), front=True)


def test_center_pool_inputs_discriminate():
    vf.inputs_discriminate_case()


@pytest.mark.parametrize("case", vf.POOL_CLIP_CASES, ids=vf._pool_id)
def test_clip_center_pool_equals_two_calls_emu(emu_backend, case):
    vf.center_pool_case(emu_backend, case, _float_guard())


@pytest.mark.parametrize("case", vf.POOL_PLAIN_CASES, ids=vf._pool_id)
def test_center_pool_equals_two_calls_emu(emu_backend, case):
    vf.center_pool_case(emu_backend, case, _float_guard())


def test_video_frame_kernel_refusals_emu(emu_backend):
    vf.kernel_refusal_case(emu_backend)


def _ctx(dev):
    return vf.frame_ctx(dev)


def test_lstm_plan_clip_frame_heatmaps_emu(emu_backend):
    vf.plan_heatmaps_case(_ctx(emu_backend))


def test_lstm_plan_clip_frame_flip_emu(emu_backend):
    vf.plan_flip_case(_ctx(emu_backend))


def test_lstm_plan_clip_frame_final_preds_emu(emu_backend):
    vf.plan_final_case(_ctx(emu_backend))


def test_lstm_plan_stream_frames_emu(emu_backend):
    vf.plan_stream_case(_ctx(emu_backend))


def test_lstm_plan_frame_workspaces_and_refusals_emu(emu_backend):
    vf.plan_workspace_case(_ctx(emu_backend))
    vf.plan_unset_case(emu_backend)


def test_lstm_plan_frame_argument_checks_emu(emu_backend):
    vf.plan_argument_case(_ctx(emu_backend))
