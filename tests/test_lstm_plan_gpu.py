"""up_unipose_lstm_step / up_unipose_lstm_clip (UniPose-LSTM inference entry, C ABI 10 additions) on the MI355X: equal bits to the
folded module, the G5 reference golden through both forms, and what the C entry buys against the module's eval clip."""
import os
import time

import numpy as np
import pytest
import torch

import lstm_plan_cases as lc
from oracle import unipose_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_lstm_plan_equals_folded_module_368():
    lc.lstm_plan_case(DEV, K=13, B=2, size=368, T=5)


def test_lstm_plan_equals_folded_module_367():
    """367 % 8 == 7: ceil(367 / 8) == (367 - 7) / 8 + 1 == 46, an accepted size that is not a multiple of 8"""
    lc.lstm_plan_case(DEV, K=13, B=2, size=367, T=5, unfolded=False)


def test_lstm_plan_widened_hand_over_gpu():
    lc.lstm_plan_case(DEV, K=15, B=2, size=160, T=3, unfolded=False)


def test_lstm_plan_g5_vs_reference_golden(golden_dir):
    """G5 (the genuine reference's five-frame eval unroll, K=13, B=1, 368x368) through both forms: 1e-3 on heat, cell and hide of
    every frame (expected ~1e-6: the folded weights are rounded once)"""
    from unipose_amd.plan import UniPoseLSTMPlan
    g = np.load(os.path.join(golden_dir, "g5_lstm_368.npz"))
    K, wseed, xseed, cseed = (int(v) for v in g["meta"])
    m = lc.mc.skeleton("lstm", K)
    m.load_state_dict(O.synth_state_dict(K, wseed, lstm=True))
    m = m.to(DEV).eval()
    x = O.synth_input((1, 5, 3, 368, 368), xseed).to(DEV)
    cm = O.synth_input((1, 5, 1, 368, 368), cseed, "rand").to(DEV)
    plan = UniPoseLSTMPlan(m, 1, 368, 368, frames=5)
    worst = 0.0
    prev = None
    for j in range(5):
        heat, cell, hide = plan.step(x[:, j], cm[:, j], prev)
        prev = (hide, cell)
        for t, n in ((heat, "heat"), (cell, "cell"), (hide, "hide")):
            e = O.max_rel(t.cpu(), g[f"{n}{j}"])
            worst = max(worst, e)
            assert e < 1e-3, (j, n, e)
    heats, cell, hide = plan.clip(x, cm)
    for j in range(5):
        e = O.max_rel(heats[:, j].cpu(), g[f"heat{j}"])
        worst = max(worst, e)
        assert e < 1e-3, (j, e)
    for t, n in ((cell, "cell"), (hide, "hide")):
        e = O.max_rel(t.cpu(), g[f"{n}4"])
        worst = max(worst, e)
        assert e < 1e-3, (n, e)
    print(f"G5 through up_unipose_lstm_step / _clip: worst max_rel {worst:.2e}")
    plan.close()


def test_lstm_plan_latency_report():
    """Eval clip latency, T = 5 at 368x368, B = 1 / 8: the module's whole-clip unroll (batch_frames, five calls) against ONE
    up_unipose_lstm_clip call.  A report; the only assertion is that the plan at B = 1 is no slower than 1.1x the module."""
    from unipose_amd.plan import UniPoseLSTMPlan
    K, T = 13, 5
    m = lc.lstm_model(DEV, K)
    m.batch_frames = True

    def ms(fn, n=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for B in (1, 8):
        x = O.synth_input((B, T, 3, 368, 368), 9).to(DEV)
        cm = O.synth_input((B, T, 1, 368, 368), 10, "rand").to(DEV)
        plan = UniPoseLSTMPlan(m, B, 368, 368, frames=T)
        out = (torch.empty((B, T, K + 1, 46, 46), device=DEV), torch.empty((B, K + 2, 46, 46), device=DEV),
               torch.empty((B, K + 2, 46, 46), device=DEV))
        module = ms(lambda: lc.module_frames(m, x, cm, K, T))
        planned = ms(lambda: plan.clip(x, cm, out=out))
        print(f"UniPose-LSTM eval clip T={T} 368x368 B={B}: module {module:.2f} ms, up_unipose_lstm_clip {planned:.2f} ms "
              f"({B * T / planned * 1e3:.0f} frames/s)")
        if B == 1:
            assert planned < module * 1.1
        plan.close()
