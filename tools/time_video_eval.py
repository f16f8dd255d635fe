"""What do the one-call evaluation entries of the video plan buy?  (GPU; a measurement, not a test.)

    timeout -k 10 600 python tools/time_video_eval.py [--out profiles/video_eval.txt] [--reps 30]

UniPose-LSTM (Penn Action, 13 joints), 368 x 368 input, clips of T = 5 frames, B = 1 and B = 8.  Each new entry of
UniPoseLSTMPlan is timed against the composition of the entries there were before, from the inputs on the device to the results
on the device:

    clip_keypoints                 against   clip + ops.heatmap_decode of the (B * T, K+1, h, w) heat-maps
    clip_final_preds(flip=True)    against   clip of the clip and of the mirrored clip + ops.flip_merge + ops.final_preds
    stream, T frames               against   step + ops.heatmap_decode per frame, the state handed over as NCHW tensors

Wall time of a call (time.perf_counter) with a device synchronise before and after, the median of the repetitions after a warm-up,
with the 10th / 90th percentiles; the two forms of a pair alternate inside every repetition so that they see the same machine.
The results of the two forms are compared first (they must be equal).  Nothing is asserted about the ratios.  Writes the report,
with the commit and the command, to --out and prints it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = (1, 8)
K, SIZE, T = 13, 368, 5
PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12]]       # Penn Action's shoulders .. ankles (the reference has no list)


def spread(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[len(t) * 9 // 10]


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:       # noqa: BLE001  (a copy of the tree without its history)
        return "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_eval.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit to name in the report (default: git rev-parse of the tree)")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_video_eval.py measures on the GPU; there is none here")
    import lstm_plan_cases as lc
    from oracle import unipose_oracle as O
    from unipose_amd import ops, protocol
    from unipose_amd.plan import UniPoseLSTMPlan
    dev = torch.device("cuda:0")
    m = lc.lstm_model(dev, K)
    perm = protocol.flip_perm(None, K, False, PAIRS)
    lines = [f"evaluation entries of the video plan, UniPose-LSTM ({K} joints), {SIZE} x {SIZE} input, T = {T}, on "
             f"{torch.cuda.get_device_name(dev)}",
             f"commit {args.commit or commit()} (+ the change that adds this file); command: python {' '.join(sys.argv)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in ms", ""]
    for B in BATCHES:
        x = O.synth_input((B, T, 3, SIZE, SIZE), 9).to(dev)
        cm = O.synth_input((B, T, 1, SIZE, SIZE), 10, "rand").to(dev)
        xf, cmf = torch.flip(x, [-1]), torch.flip(cm, [-1])            # the composition's mirrored inputs, made once, not timed
        cen = np.stack([[np.array([180.0 + i + t, 190.0 - i]) for t in range(T)] for i in range(B)])
        sc = np.array([[1.5 + 0.01 * i + 0.001 * t for t in range(T)] for i in range(B)])
        plan = UniPoseLSTMPlan(m, B, SIZE, SIZE, frames=T)
        plan.clip_flip_heatmaps(x, cm, pairs=PAIRS)                    # the flip workspace exists before anything is timed
        state = plan.stream_state()

        def kp_one():
            return plan.clip_keypoints(x, cm)[0]

        def kp_comp():
            return ops.heatmap_decode(plan.clip(x, cm)[0].flatten(0, 1))[0].reshape(B, T, K + 1, 2)

        def fp_one():
            return plan.clip_final_preds(x, cm, cen, sc, flip=True, pairs=PAIRS)[0]

        def fp_comp():
            a, f = plan.clip(x, cm)[0], plan.clip(xf, cmf)[0]
            merged = ops.flip_merge(a.flatten(0, 1), f.flatten(0, 1), perm)
            return ops.final_preds(merged, cen.reshape(B * T, 2), sc.reshape(B * T)).reshape(B, T, K + 1, 2)

        def st_one():
            out = None
            for j in range(T):
                out = plan.stream(x[:, j], cm[:, j], state, first=j == 0)[0]
            return out

        def st_comp():
            prev, out = None, None
            for j in range(T):
                heat, cell, hide = plan.step(x[:, j], cm[:, j], prev)
                prev = (hide, cell)
                out = ops.heatmap_decode(heat)[0]
            return out

        pairs = (("clip_keypoints", kp_one, "clip + heatmap_decode", kp_comp),
                 ("clip_final_preds(flip)", fp_one, "2 x clip + flip_merge + final_preds", fp_comp),
                 (f"stream x {T} frames", st_one, f"(step + heatmap_decode) x {T}", st_comp))
        lines.append(f"B = {B}")
        for name, one, cname, comp in pairs:
            equal = bool(torch.equal(one(), comp()))
            for _ in range(args.warmup):
                one()
                comp()
            times = {name: [], cname: []}
            for _ in range(args.reps):
                for n, fn in ((name, one), (cname, comp)):
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    times[n].append((time.perf_counter() - t0) * 1e3)
            med = {}
            for n, t in times.items():
                med[n], lo, hi = spread(t)
                lines.append(f"  {n:38s} {med[n]:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]")
            lines.append(f"  composition / one call = {med[cname] / med[name]:.3f}x   (results of the two forms equal: {equal})")
        lines.append("")
        plan.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
