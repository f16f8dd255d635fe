"""Whole-clip / per-frame inference entry of UniPose-LSTM (up_unipose_lstm_step / up_unipose_lstm_clip, unipose_amd/plan.py
UniPoseLSTMPlan) against the drop-in module: shared by the emulator and the GPU tests.  The plan issues the launches of the
module's folded inference paths, so the comparisons are for EQUAL bits; the module itself is pinned to the reference by G5."""
import copy

import torch

from oracle import unipose_oracle as O

import model_cases as mc


def lstm_model(dev, K=13, wseed=4):
    m = mc.skeleton("lstm", K)
    m.load_state_dict(O.synth_state_dict(K, wseed, lstm=True))
    return m.to(dev).eval()


def folded_copy(m, batch_frames):
    from unipose_amd import checkpoint
    f = checkpoint.load_folded(copy.deepcopy(m), checkpoint.fold_batchnorm(m))
    f.batch_frames = batch_frames
    return f


def _equal(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got.cpu(), ref.cpu()), (what, float((got - ref).abs().max()))


def module_frames(model, x, cm, K, frames):
    """the reference driver's call pattern (uniposeLSTM.py:124-128) for `frames` frames: [(heat, cell, hide)] per frame"""
    h = (x.shape[-2] - 1) // 8 + 1
    w = (x.shape[-1] - 1) // 8 + 1
    heat = torch.zeros(K + 1, h, w, device=x.device)
    cell = torch.zeros(K + 2, h, w, device=x.device)
    hide = torch.zeros(K + 2, h, w, device=x.device)
    out = []
    with torch.no_grad():
        for j in range(frames):
            heat, cell, hide = model(x, cm, j, heat, hide, cell)
            out.append((heat, cell, hide))
    return out


def lstm_plan_case(dev, K=13, B=1, size=32, T=2, wseed=4, unfolded=True):
    """step form over T + 1 frames against the per-frame module, clip form over the first T frames against the whole-clip unroll,
    and the clip's last state handed to step for frame T"""
    from unipose_amd.plan import UniPoseLSTMPlan
    m = lstm_model(dev, K, wseed)
    x = O.synth_input((B, T + 1, 3, size, size), 15).to(dev)
    cm = O.synth_input((B, T + 1, 1, size, size), 16, "rand").to(dev)
    xc, cmc = x[:, :T].contiguous(), cm[:, :T].contiguous()
    plan = UniPoseLSTMPlan(m, B, size, size, frames=T)

    # step form: the module's per-frame path (batch_frames = False)
    ref = module_frames(folded_copy(m, False), x, cm, K, T + 1)
    prev = None
    for j in range(T + 1):
        got = plan.step(x[:, j], cm[:, j], prev)
        for g, r, n in zip(got, ref[j], ("heat", "cell", "hide")):
            _equal(g, r, f"step frame {j} {n}")
        prev = (got[2], got[1])
    if unfolded:                          # folding itself: one rounding per weight
        m.batch_frames = False
        raw = module_frames(m, x, cm, K, T + 1)
        for j in range(T + 1):
            for r, u in zip(ref[j], raw[j]):
                assert O.max_rel(r.cpu(), u.cpu()) < 1e-4, j

    # clip form: the module's whole-clip unroll (batch_frames = batch_head = True)
    ref_clip = module_frames(folded_copy(m, True), xc, cmc, K, T)
    heats, cell, hide = plan.clip(xc, cmc)
    assert heats.shape == (B, T, K + 1) + tuple(ref_clip[0][0].shape[-2:])
    for j in range(T):
        _equal(heats[:, j], ref_clip[j][0], f"clip heat {j}")
    _equal(cell, ref_clip[T - 1][1], "clip last cell")
    _equal(hide, ref_clip[T - 1][2], "clip last hide")

    # mixing the forms: the clip's last state carries on through step for frame T, like the module's next per-frame call
    with torch.no_grad():
        nxt = folded_copy(m, False)(x, cm, T, ref_clip[T - 1][0], hide, cell)
    got = plan.step(x[:, T], cm[:, T], (hide, cell))
    for g, r, n in zip(got, nxt, ("heat", "cell", "hide")):
        _equal(g, r, f"step after clip {n}")

    # a second clip on the same workspace, caller-provided outputs
    own = (torch.empty_like(heats), torch.empty_like(cell), torch.empty_like(hide))
    again = plan.clip(xc, cmc, out=own)
    assert all(a is o for a, o in zip(again, own))
    _equal(again[0], heats, "second clip")
    plan.close()
    return heats


def argument_checks(dev, K=13, size=32):
    """input / `out=` validation of UniPoseLSTMPlan (no launch reaches the device)"""
    from unipose_amd.plan import UniPoseLSTMPlan
    m = lstm_model(dev, K)
    B, T = 1, 2
    hs = (size - 1) // 8 + 1
    plan = UniPoseLSTMPlan(m, B, size, size, frames=T)
    x = torch.zeros(B, T, 3, size, size, device=dev)
    cm = torch.zeros(B, T, 1, size, size, device=dev)
    bad_calls = [
        lambda: plan.clip(torch.zeros(B, T + 1, 3, size, size, device=dev), torch.zeros(B, T + 1, 1, size, size, device=dev)),  # T
        lambda: plan.clip(x.double(), cm),
        lambda: plan.clip(x[..., :size - 8], cm),
        lambda: plan.step(x[:, 0], cm[:, 0, :, :8]),
        lambda: plan.step(x[:, 0], cm[:, 0], first=False),                      # a later frame needs a state
        lambda: plan.step(x[:, 0], cm[:, 0], (torch.zeros(K + 2, hs + 1, hs, device=dev), torch.zeros(K + 2, hs, hs, device=dev))),
    ]
    good = [torch.empty(B, T, K + 1, hs, hs, device=dev), torch.empty(B, K + 2, hs, hs, device=dev),
            torch.empty(B, K + 2, hs, hs, device=dev)]
    for i, bad in enumerate((torch.empty(B, T, K + 1, hs - 1, hs, device=dev), torch.empty(B, T, K + 1, hs, hs, device=dev).double(),
                             torch.empty(B, T, K + 1, hs, 2 * hs, device=dev)[..., ::2])):
        out = list(good)
        out[0] = bad
        bad_calls.append(lambda out=out: plan.clip(x, cm, out=out))
    out = list(good)
    out[2] = torch.empty(B, K + 2, hs, 2 * hs, device=dev)[..., ::2]                       # a strided hide
    bad_calls.append(lambda: plan.clip(x, cm, out=out))
    for i, call in enumerate(bad_calls):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(f"bad call {i} was not refused")
    plan.close()
