"""plan(x) of the image plan in fp32 and in bf16 storage (UniPosePlan(..., storage=...)), K = 16 at 368 x 368, B = 1 / 8 / 32:
device-event time per call, the two plans timed in alternating blocks in one process (shared clocks and placement), the whole
measurement twice; the workspace bytes of both; and the G1 golden (K = 14, B = 2, 368 x 368) through both plans.

    python tools/gpu/plan_bf16.py [--out profiles/plan_bf16.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP, BLOCKS, PER_BLOCK = 20, 5, 12          # 60 timed calls per plan and run, after 20 warm-ups each


def block_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def timings(model, dev, say):
    from unipose_amd import _C
    from unipose_amd.plan import UniPosePlan
    L = _C.lib()
    say(f"{'B':>3s} {'run':>3s} {'fp32 ms':>9s} {'bf16 ms':>9s} {'fp32/bf16':>9s} {'fp32 min':>9s} {'bf16 min':>9s} {'fp32 ws MB':>11s} {'bf16 ws MB':>11s}")
    for B in (1, 8, 32):
        x = torch.randn(B, 3, 368, 368, device=dev)
        plans = {s: UniPosePlan(model, B, 368, 368, storage=s) for s in ("f32", "bf16")}
        outs = {s: torch.empty((B, 17, 46, 46), device=dev) for s in plans}
        ws = {s: L.up_unipose_plan_workspace(p._plan) for s, p in plans.items()}
        for run in (1, 2):
            for s, p in plans.items():
                for _ in range(WARMUP):
                    p(x, out=outs[s])
            torch.cuda.synchronize()
            t = {s: [] for s in plans}
            for _ in range(BLOCKS):
                for s, p in plans.items():
                    t[s].append(block_ms(lambda: p(x, out=outs[s]), PER_BLOCK))
            m = {s: sum(v) / len(v) for s, v in t.items()}
            say(f"{B:3d} {run:3d} {m['f32']:9.3f} {m['bf16']:9.3f} {m['f32'] / m['bf16']:9.2f} {min(t['f32']):9.3f} {min(t['bf16']):9.3f} "
                f"{ws['f32'] / 2 ** 20:11.2f} {ws['bf16'] / 2 ** 20:11.2f}")
        assert bool(torch.isfinite(outs["bf16"]).all()) and bool(torch.isfinite(outs["f32"]).all())
        for p in plans.values():
            p.close()


def g1(dev, say):
    import model_cases as mc
    from oracle import unipose_oracle as O
    from unipose_amd.plan import UniPosePlan
    g = np.load(os.path.join(ROOT, "tests", "golden", "g1_eval_368.npz"))
    K, wseed, xseed = (int(v) for v in g["meta"])
    m, _ = mc.build_image_model(K, wseed, dev)
    m.eval()
    x = O.synth_input((2, 3, 368, 368), xseed).to(dev)
    for s in ("f32", "bf16"):
        plan = UniPosePlan(m, 2, 368, 368, storage=s)
        y = plan(x).cpu()
        share = float((y.reshape(2, K + 1, -1).argmax(2).numpy() == g["argmax"]).mean())
        say(f"G1 (K = {K}, B = 2, 368 x 368) through the {s} plan: max_rel {O.max_rel(y, g['out']):.3e}, "
            f"joints with the reference's argmax {share:.4f}")
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_bf16.py measures on the GPU; there is none here")
    from model.unipose import unipose
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    model = unipose("MPII", num_classes=16).to(dev).eval()
    say(f"UniPosePlan.__call__ (up_unipose_forward), K = 16, 368 x 368, {torch.cuda.get_device_name(0)}: ms per call by device events, "
        f"{BLOCKS} alternating blocks of {PER_BLOCK} calls per plan after {WARMUP} warm-ups; mean and fastest block")
    timings(model, dev, say)
    g1(dev, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
