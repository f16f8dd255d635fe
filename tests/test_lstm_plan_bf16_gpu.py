"""The video plan in bf16 storage (UniPoseLSTMPlan(..., storage="bf16"); up_unipose_lstm_plan_create_t) on the MI355X: equal bits to
the folded eval module under ops.set_conv_math("bf16s"), through all 15 programs.  K = 13, B = 2, T = 3 at 32 x 40 (the spare pad lane
takes the centre map, the stacked gate convolution reads 32 lanes: bf16 operands, H != W); K = 15, B = 1, T = 2 at 39 x 39 (the widened
hand-over, the gate convolution reads 40 lanes: fp32, an odd size); K = 13 at 64 x 72 with output stride 8."""
import pytest
import torch

import lstm_plan_bf16_cases as vb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOTH = [vb.GPU_A, vb.GPU_B]
ODD_IMAGE = dict(K=14, B=2, height=52, width=68)       # the bf16 image plan test_plan_bf16_gpu.py shares


@pytest.mark.parametrize("case", BOTH + [vb.GPU_S8], ids=vb.case_id)
def test_lstm_plan_bf16_forward_equals_module(case):
    vb.forward_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH, ids=vb.case_id)
def test_lstm_plan_bf16_eval_programs(case):
    vb.eval_programs_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH, ids=vb.case_id)
def test_lstm_plan_bf16_frame_programs(case):
    vb.frame_programs_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH, ids=vb.case_id)
def test_lstm_plan_bf16_counters(case):
    vb.counters_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH, ids=vb.case_id)
def test_lstm_plan_bf16_differs_from_fp32(case):
    vb.differs_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH + [vb.GPU_S8], ids=vb.case_id)
def test_lstm_plan_bf16_workspace_and_state(case):
    vb.workspace_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH, ids=vb.case_id)
def test_lstm_plan_bf16_no_stale_workspace(case):
    vb.stale_case(DEV, **case)


@pytest.mark.parametrize("case", BOTH, ids=vb.case_id)
def test_lstm_plan_bf16_refresh(case):
    vb.refresh_case(DEV, **case)


def test_lstm_plan_bf16_coexistence():
    vb.coexistence_case(DEV, ODD_IMAGE, **vb.GPU_A)


def test_lstm_plan_bf16_refusals():
    vb.refusal_case(DEV, **vb.GPU_A)
