"""What does batching independent video streams cost and buy?  (GPU; a measurement, not a test.)

    timeout -k 10 900 python tools/time_stream_serve.py [--out profiles/stream_serve.txt] [--reps 30]

UniPose-LSTM (Penn Action, 13 joints), 368 x 368 input, fp32 and bf16 storage, B = 1 / 4 / 8 streams, all in one process.  One frame of
B streams, from the inputs on the device to the joints on the device, four ways:

    stream (next), batch B          UniPoseLSTMPlan.stream: one state buffer, all B samples continue (they started together)
    serve, none first               UniPoseLSTMPlan.serve: the state in a pool, every sample continues (the lstm_0 convolution is skipped)
    serve, one restart              the same with sample 0 restarting: both gate convolutions run
    B x stream (next), batch 1      B calls of a batch-1 plan, one state buffer each: what a user without serve does today

Wall time of a call (time.perf_counter) with a device synchronise before and after, the median of the repetitions after a warm-up,
with the 10th / 90th percentiles; the four forms alternate inside every repetition so that they see the same machine.  Before
anything is timed, `serve` of a frame is compared with `stream` of the same frame on the same state (they must be equal).  Nothing
is asserted about the times.  Writes the report, with the commit and the command, to --out and prints it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = (1, 4, 8)
STORAGES = ("f32", "bf16")
K, SIZE = 13, 368


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_serve.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit to name in the report (default: git rev-parse of the tree)")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_stream_serve.py measures on the GPU; there is none here")
    import lstm_plan_cases as lc
    from oracle import unipose_oracle as O
    from unipose_amd.plan import UniPoseLSTMPlan
    dev = torch.device("cuda:0")
    m = lc.lstm_model(dev, K)
    lines = [f"one frame of B independent streams, UniPose-LSTM ({K} joints), {SIZE} x {SIZE} input, on {torch.cuda.get_device_name(dev)}",
             f"commit {args.commit or commit()} (+ the change that adds this file); command: python {' '.join(sys.argv)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in ms, and the median per stream", ""]
    for storage in STORAGES:
        one = UniPoseLSTMPlan(m, 1, SIZE, SIZE, storage=storage)
        for B in BATCHES:
            x = O.synth_input((2, B, 3, SIZE, SIZE), 9).to(dev)
            cm = O.synth_input((2, B, 1, SIZE, SIZE), 10, "rand").to(dev)
            plan = UniPoseLSTMPlan(m, B, SIZE, SIZE, storage=storage)
            slots = B + 2
            slot = [slots - 1 - b for b in range(B)]                       # lane b is not slot b
            state, pool = plan.stream_state(), plan.stream_pool(slots)
            pool.fill_(0xFF)
            states1 = [one.stream_state() for _ in range(B)]
            # every stream starts on frame 0, both ways; frame 1 must then agree
            plan.stream(x[0], cm[0], state, first=True)
            plan.serve(x[0], cm[0], pool, slot, [1] * B)
            for b in range(B):
                one.stream(x[0, b:b + 1], cm[0, b:b + 1], states1[b], first=True)
            a = plan.stream(x[1], cm[1], state)
            s = plan.serve(x[1], cm[1], pool, slot, [0] * B)
            equal = all(bool(torch.equal(p, q)) for p, q in zip(a, s))
            none_first, restart = [0] * B, [1] + [0] * (B - 1)
            xs = [(x[1, b:b + 1].contiguous(), cm[1, b:b + 1].contiguous()) for b in range(B)]

            def f_stream():
                return plan.stream(x[1], cm[1], state)

            def f_serve():
                return plan.serve(x[1], cm[1], pool, slot, none_first)

            def f_restart():
                return plan.serve(x[1], cm[1], pool, slot, restart)

            def f_singles():
                out = None
                for b in range(B):
                    out = one.stream(xs[b][0], xs[b][1], states1[b])
                return out

            forms = (("stream (next), batch B", f_stream), ("serve, none first", f_serve), ("serve, one restart", f_restart),
                     (f"{B} x stream (next), batch 1", f_singles))
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            times = {n: [] for n, _ in forms}
            for _ in range(args.reps):
                for n, fn in forms:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    times[n].append((time.perf_counter() - t0) * 1e3)
            lines.append(f"{storage} storage, B = {B}   (serve equals stream on the same state: {equal})")
            med = {}
            for n, t in times.items():
                med[n], lo, hi = spread(t)
                lines.append(f"  {n:32s} {med[n]:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]   {med[n] / B:8.3f} ms per stream")
            base = med["stream (next), batch B"]
            lines.append(f"  serve / stream = {med['serve, none first'] / base:.3f}x, with one restart {med['serve, one restart'] / base:.3f}x; "
                         f"{B} single calls / serve = {med[forms[3][0]] / med['serve, none first']:.3f}x")
            lines.append("")
            plan.close()
        one.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
