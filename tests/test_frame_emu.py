"""Pose from source frames (frame_cases.py) on a GPU-less box: the HIP sources compiled against the fiber emulator (tests/emu).  The
first test needs no device.  Every source buffer and every output of up_crop_to_nhwc ends right in front of an inaccessible page
(tests/emu/guard_alloc.py), so a tap read past a frame's end — through a frame index outside 0 .. F-1, for instance — or a store
past an output's end faults.  The launch of more than 2^21 output pixels runs on the GPU only (test_frame_gpu.py)."""
import pytest

import frame_cases as fc
import protocol_cases as pc


def _guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return guarded


def test_crop_maps_equal_reference(golden_dir):
    fc.geometry_case(golden_dir)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_crop_equals_two_calls_emu(emu_backend, case):
    fc.kernel_case(emu_backend, case, _guard())


def test_identity_equals_normalize_emu(emu_backend):
    fc.identity_case(emu_backend, _guard())


def test_frame_indexing_emu(emu_backend):
    fc.frame_index_case(emu_backend, _guard())


def test_valid_extent_per_frame_emu(emu_backend):
    fc.valid_case(emu_backend, _guard())


def test_frame_index_out_of_range_emu(emu_backend):
    fc.bad_frame_case(emu_backend, _guard())


def test_crop_refusals_emu(emu_backend):
    fc.refusal_case(emu_backend)


@pytest.mark.parametrize("case", fc.plan_cases(pc.PLAN_CASES_EMU), ids=fc.plan_id)
def test_plan_from_frames_emu(emu_backend, case):
    fc.plan_case(emu_backend, **case)


def test_plan_from_frames_unset_weights_refused_emu(emu_backend):
    fc.plan_unset_case(emu_backend)
