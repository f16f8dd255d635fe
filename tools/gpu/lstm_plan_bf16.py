"""The video plan in fp32 and in bf16 storage (UniPoseLSTMPlan(..., storage=...)), K = 13 at 368 x 368: device-event time per call
of clip at B = 1 and B = 8 (T = 5; BASELINE configs[3] is 8 x 5), of clip_final_preds with the flip test at B = 8, and of stream (a
later frame) at B = 1 — the plans timed in alternating blocks in one process (shared clocks and placement), the whole measurement
twice; the workspace and state bytes of both; and the G5 golden (the reference's five-frame eval unroll, B = 1) through both plans.

    python tools/gpu/lstm_plan_bf16.py [--out profiles/lstm_plan_bf16.txt] [--storages f32,bf16]

`--storages f32` times the fp32 plan alone and passes no `storage=`: that form also runs on a tree from before the option.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP, BLOCKS, PER_BLOCK = 10, 5, 8           # 40 timed calls per plan and run, after 10 warm-ups each
K, SIZE, T = 13, 368, 5
PAIRS = [[1, 2], [3, 4]]


def block_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def make_plan(model, B, storage):
    from unipose_amd.plan import UniPoseLSTMPlan
    kw = {} if storage == "f32" else {"storage": storage}
    return UniPoseLSTMPlan(model, B, SIZE, SIZE, frames=T, **kw)


def measure(calls, say, label):
    """calls: {storage: fn}; per storage the median, fastest and slowest block of each of two runs"""
    for run in (1, 2):
        for fn in calls.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        t = {s: [] for s in calls}
        for _ in range(BLOCKS):
            for s, fn in calls.items():
                t[s].append(block_ms(fn, PER_BLOCK))
        med = {s: statistics.median(v) for s, v in t.items()}
        cells = " ".join(f"{s:>5s} {med[s]:8.3f} [{min(t[s]):8.3f} .. {max(t[s]):8.3f}]" for s in calls)
        ratio = f"  fp32/bf16 {med['f32'] / med['bf16']:5.2f}" if "f32" in med and "bf16" in med else ""
        say(f"{label:34s} run {run}  {cells}{ratio}")


def timings(model, dev, storages, say):
    from unipose_amd import _C
    L = _C.lib()
    say("ms per call: median [fastest .. slowest] block")
    for B in (1, 8):
        x = torch.randn(B, T, 3, SIZE, SIZE, device=dev)
        cm = torch.rand(B, T, 1, SIZE, SIZE, device=dev)
        plans = {s: make_plan(model, B, s) for s in storages}
        h = plans[storages[0]].out_height
        outs = {s: (torch.empty((B, T, K + 1, h, h), device=dev), torch.empty((B, K + 2, h, h), device=dev),
                    torch.empty((B, K + 2, h, h), device=dev)) for s in plans}
        measure({s: (lambda p=p, s=s: p.clip(x, cm, out=outs[s])) for s, p in plans.items()}, say, f"clip B={B} T={T}")
        if B == 8:
            measure({s: (lambda p=p: p.clip_final_preds(x, cm, flip=True, pairs=PAIRS)) for s, p in plans.items()}, say,
                    f"clip_final_preds flip B={B} T={T}")
        else:
            states = {s: p.stream_state() for s, p in plans.items()}
            for s, p in plans.items():
                p.stream(x[:, 0], cm[:, 0], states[s], first=True)
            measure({s: (lambda p=p, s=s: p.stream(x[:, 1], cm[:, 1], states[s])) for s, p in plans.items()}, say, f"stream B={B} (a later frame)")
        for s, p in plans.items():
            assert all(bool(torch.isfinite(t).all()) for t in outs[s])
            say(f"  B={B} {s:>5s}: workspace {L.up_unipose_lstm_plan_workspace(p._plan) / 2 ** 20:8.2f} MB, flip workspace "
                f"{L.up_unipose_lstm_plan_flip_workspace(p._plan) / 2 ** 20:8.2f} MB, state {L.up_unipose_lstm_plan_state_bytes(p._plan)} bytes")
            p.close()


def g5(dev, storages, say):
    import lstm_plan_cases as lc
    from oracle import unipose_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g5_lstm_368.npz"))
    k, wseed, xseed, cseed = (int(v) for v in g["meta"])
    m = lc.mc.skeleton("lstm", k)
    m.load_state_dict(O.synth_state_dict(k, wseed, lstm=True))
    m = m.to(dev).eval()
    x = O.synth_input((1, T, 3, SIZE, SIZE), xseed).to(dev)
    cm = O.synth_input((1, T, 1, SIZE, SIZE), cseed, "rand").to(dev)
    for s in storages:
        plan = make_plan(m, 1, s)
        heats = plan.clip(x, cm)[0].cpu()
        worst = max(O.max_rel(heats[:, j], g[f"heat{j}"]) for j in range(T))
        want = np.stack([g[f"heat{j}"].reshape(k + 1, -1).argmax(1) for j in range(T)])
        share = float((heats[0].reshape(T, k + 1, -1).argmax(2).numpy() == want).mean())
        say(f"G5 (K = {k}, B = 1, T = {T}, {SIZE} x {SIZE}) through the {s} plan's clip: worst max_rel over the frames {worst:.3e}, "
            f"maps with the reference's argmax {share:.4f}")
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--storages", default="f32,bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_plan_bf16.py measures on the GPU; there is none here")
    import lstm_plan_cases as lc
    dev = torch.device("cuda:0")
    storages = args.storages.split(",")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = lc.lstm_model(dev, K)
    say(f"UniPoseLSTMPlan, K = {K}, {SIZE} x {SIZE}, {torch.cuda.get_device_name(0)}: ms per call by device events, {BLOCKS} alternating "
        f"blocks of {PER_BLOCK} calls per plan after {WARMUP} warm-ups, the whole measurement twice")
    timings(model, dev, storages, say)
    g5(dev, storages, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
