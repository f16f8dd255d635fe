"""The video plan in bf16 storage (UniPoseLSTMPlan(..., storage="bf16"); up_unipose_lstm_plan_create_t) on the CPU emulator: equal
bits to the folded eval module under ops.set_conv_math("bf16s").  K = 13 and K = 15 at B = 1, T = 2, 32 x 32: the two forms of the
hand-over and the two arithmetics of the stacked gate convolution.  An emulated bf16 trunk costs seconds per image, so this file is
the lean cut of tests/lstm_plan_bf16_cases.py: every plan call runs once, in a 0xFF-filled workspace of exactly the reported size
that ends right in front of an inaccessible page (tests/emu/guard_alloc.py).  Every program, refresh and coexistence run on the
GPU (test_lstm_plan_bf16_gpu.py)."""
import pytest
import torch

import lstm_plan_bf16_cases as vb


def _bytes_guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return lambda n: guarded((n,), torch.uint8)


@pytest.mark.parametrize("case", [vb.EMU_A, vb.EMU_B], ids=vb.case_id)
def test_lstm_plan_bf16_clip_equals_module_emu(emu_backend, case):
    vb.lean_forward_case(emu_backend, _bytes_guard(), **case)


def test_lstm_plan_bf16_step_and_stream_emu(emu_backend):
    vb.lean_step_stream_case(emu_backend, _bytes_guard(), **vb.EMU_B)


def test_lstm_plan_bf16_flip_and_frames_emu(emu_backend):
    vb.lean_flip_frames_case(emu_backend, _bytes_guard(), **vb.EMU_A)


def test_lstm_plan_bf16_differs_from_fp32_and_figures_emu(emu_backend):
    vb.lean_differs_case(emu_backend, _bytes_guard(), **vb.EMU_A)


def test_lstm_plan_bf16_refusals_emu(emu_backend):
    vb.lean_refusal_case(emu_backend, _bytes_guard(), **vb.EMU_A)
