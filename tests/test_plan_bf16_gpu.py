"""The image plan in bf16 storage (UniPosePlan(..., storage="bf16"); up_unipose_plan_create_t) on the MI355X: equal bits to the
folded eval module under ops.set_conv_math("bf16s"), through every program; the G1 reference golden through it, reported."""
import os

import numpy as np
import pytest
import torch

import model_cases as mc
import plan_bf16_cases as bc
from oracle import unipose_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ONE = dict(K=14, B=1, height=64, width=64)       # B = 1: the GAP branch's 1x1 convolution has one row on a 128-row bf16 tile
ODD = dict(K=14, B=2, height=52, width=68)       # 7 x 9 maps: neither side a multiple of 8, H != W


@pytest.mark.parametrize("case", bc.FORWARD_GPU, ids=bc.case_id)
def test_plan_bf16_forward_equals_module(case):
    bc.forward_case(DEV, **case)


def test_plan_bf16_counters():
    bc.counters_case(DEV, **ONE)


def test_plan_bf16_workspace_figures():
    bc.workspace_case(DEV, **ODD)


def test_plan_bf16_no_stale_workspace():
    bc.stale_case(DEV, **ODD)


def test_plan_bf16_every_program():
    bc.programs_case(DEV, 52, 68)


def test_plan_bf16_refresh():
    bc.refresh_case(DEV, **ODD)


def test_plan_bf16_setters():
    bc.setters_case(DEV)


def test_plan_bf16_coexistence():
    bc.coexistence_case(DEV, **ODD)


def test_plan_bf16_refusals():
    bc.refusal_case(DEV, **ODD)


def test_plan_bf16_refusals_upsampled():
    bc.refusal_case(DEV, **bc.FORWARD_GPU[3])


def test_plan_bf16_g1_eval_368_reported(golden_dir):
    """G1 (the genuine reference's eval forward, K = 14, B = 2, 368 x 368) through the bf16 plan: a REPORT.  Nobody has measured
    bf16 storage at this size against G1, so no bound is fixed: the plan's accuracy is the module's (equal bits, above), and the
    module's is the business of tests/test_bf16s_gpu.py.  Asserted: the output is finite, and the fp32 plan on the same input is
    still under 2e-5.  The figures are kept in profiles/plan_bf16.txt (measured: max_rel 1.2e-2, 28 of the 30 argmaxes; fp32 1.6e-6)."""
    from unipose_amd.plan import UniPosePlan
    g = np.load(os.path.join(golden_dir, "g1_eval_368.npz"))
    K, wseed, xseed = (int(v) for v in g["meta"])
    m, _ = mc.build_image_model(K, wseed, DEV)
    m.eval()
    x = O.synth_input((2, 3, 368, 368), xseed).to(DEV)
    plan = UniPosePlan(m, 2, 368, 368, storage="bf16")
    y = plan(x)
    e = O.max_rel(y.cpu(), g["out"])
    share = float((y.cpu().reshape(2, K + 1, -1).argmax(2).numpy() == g["argmax"]).mean())
    print(f"G1 through the bf16 plan: max_rel {e:.3e}, joints with the reference's argmax {share:.4f}")
    assert bool(torch.isfinite(y).all())
    plan.close()
    plan32 = UniPosePlan(m, 2, 368, 368)
    e32 = O.max_rel(plan32(x).cpu(), g["out"])
    print(f"G1 through the fp32 plan: max_rel {e32:.3e}")
    assert e32 < 2e-5
    plan32.close()
