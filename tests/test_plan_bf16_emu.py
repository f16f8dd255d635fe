"""The image plan in bf16 storage (UniPosePlan(..., storage="bf16"); up_unipose_plan_create_t) on the CPU emulator: equal bits to
the folded eval module under ops.set_conv_math("bf16s"), through every program."""
import pytest

import plan_bf16_cases as bc

SMALL = dict(K=14, B=2, height=36, width=44)
ONE = dict(K=14, B=1, height=64, width=64)       # B = 1: the GAP branch's 1x1 convolution has one row on a 128-row bf16 tile


@pytest.mark.parametrize("case", bc.FORWARD_EMU, ids=bc.case_id)
def test_plan_bf16_forward_equals_module_emu(emu_backend, case):
    bc.forward_case(emu_backend, **case)


def test_plan_bf16_counters_emu(emu_backend):
    bc.counters_case(emu_backend, **ONE)


def test_plan_bf16_workspace_figures_emu(emu_backend):
    bc.workspace_case(emu_backend, **SMALL)


def test_plan_bf16_no_stale_workspace_emu(emu_backend):
    bc.stale_case(emu_backend, **SMALL)


def test_plan_bf16_every_program_emu(emu_backend):
    bc.programs_case(emu_backend, 36, 44)


def test_plan_bf16_refresh_emu(emu_backend):
    bc.refresh_case(emu_backend, **SMALL)


def test_plan_bf16_setters_emu(emu_backend):
    bc.setters_case(emu_backend)


def test_plan_bf16_coexistence_emu(emu_backend):
    bc.coexistence_case(emu_backend, **SMALL)


def test_plan_bf16_refusals_emu(emu_backend):
    bc.refusal_case(emu_backend, **SMALL)
