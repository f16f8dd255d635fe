"""What does the flip test in ONE trunk pass over 2 B images buy?  (GPU; a measurement, not a test.)

    timeout -k 10 1100 python tools/time_flip_one_pass.py [--out profiles/flip_one_pass.txt] [--reps 30] [--only image|video]

Times the flip-test entries of a plan created with flip="one_pass" (UP_PLAN_FLIP_ONE_PASS) against the same entries of an
unflagged plan built in the same process from the same library and the same model — the two-pass form, the behaviour without the
flag:

    image   MPII (K = 16), 368 x 368, fp32 and bf16 storage, B = 1, 2, 4, 8, 16, 32:
            UniPosePlan.final_preds(x, center, scale, flip=True) and .frame_final_preds(frames, center, scale, flip=True)
    video   K = 13, T = 5, 368 x 368, fp32 and bf16 storage, B = 1, 2, 8: UniPoseLSTMPlan.clip_final_preds(..., flip=True)

Wall time of a call (time.perf_counter) with a device synchronise before and after, results left on the device; the median of the
repetitions after a warm-up of both forms, with the 10th / 90th percentiles; the two forms alternate inside every repetition so
that they see the same machine.  A point counts as a gain (or a loss) only where the [p10 .. p90] intervals of the two forms do
not overlap.  The two forms are not bit-equal (a convolution picks its kernel by its row count): the largest difference of their
predictions is reported beside the times, and so are the two workspace figures a caller pays.  Writes the report to --out and
prints it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = 368
IMAGE_K, IMAGE_BATCHES = 16, (1, 2, 4, 8, 16, 32)
VIDEO_K, VIDEO_T, VIDEO_BATCHES = 13, 5, (1, 2, 8)
STORAGES = ("f32", "bf16")
PAIRS = [[1, 2], [3, 4]]


def spread(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[len(t) * 9 // 10]


def measure(dev, forms, reps, warmup):
    """forms: {name: call}; alternating -> {name: (median, p10, p90)} in ms"""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    times = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: spread(t) for name, t in times.items()}


def verdict(two, one):
    if two[1] > one[2]:
        return "gain"
    if one[1] > two[2]:
        return "loss"
    return "within the spread"


def report(lines, label, stats, diff, ws):
    two, one = stats["two_pass"], stats["one_pass"]
    lines.append(f"  {label:34s} two passes {two[0]:8.3f} [{two[1]:8.3f} .. {two[2]:8.3f}]   one pass {one[0]:8.3f} [{one[1]:8.3f} .. {one[2]:8.3f}]"
                 f"   two / one = {two[0] / one[0]:5.3f}x  {verdict(two, one):17s}  workspace {ws[0] / 2**20:8.1f} -> {ws[1] / 2**20:8.1f} MiB"
                 f"   max |d preds| {diff:g}")


def image_points(dev, lines, reps, warmup):
    import model_cases as mc
    from oracle import unipose_oracle as O
    from unipose_amd import _C
    from unipose_amd.plan import UniPosePlan
    L = _C.lib()
    m, _ = mc.build_image_model(IMAGE_K, 3, dev)
    m.eval()
    frames = torch.randint(0, 256, (4, 480, 640, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(dev)
    for storage in STORAGES:
        lines.append(f"image plan, MPII ({IMAGE_K} joints), {SIZE} x {SIZE}, {storage} storage; ms per call")
        for B in IMAGE_BATCHES:
            x = O.synth_input((B, 3, SIZE, SIZE), 9).to(dev)
            cen = np.stack([np.array([180.0 + i, 190.0 - i]) for i in range(B)])
            sc = np.array([1.5 + 0.01 * i for i in range(B)])
            fcen = np.stack([np.array([320.0 + 3 * i, 240.0 - 2 * i]) for i in range(B)])
            fsc = np.array([1.8 + 0.01 * i for i in range(B)])
            fo = [i % 4 for i in range(B)]
            plans = {"two_pass": UniPosePlan(m, B, SIZE, SIZE, storage=storage),
                     "one_pass": UniPosePlan(m, B, SIZE, SIZE, storage=storage, flip="one_pass")}
            for label, row, call in (
                    ("final_preds(flip=True)", 5, lambda p: p.final_preds(x, cen, sc, flip=True, dataset="MPII")[0]),
                    ("frame_final_preds(flip=True)", _C.PROGRAM_FROM_FRAMES + 5,
                     lambda p: p.frame_final_preds(frames, fcen, fsc, frame_of=fo, flip=True, dataset="MPII")[0])):
                diff = float((call(plans["two_pass"]) - call(plans["one_pass"])).abs().max())
                stats = measure(dev, {name: (lambda p=p: call(p)) for name, p in plans.items()}, reps, warmup)
                ws = [L.up_unipose_plan_program_workspace(plans[n]._plan, row) for n in ("two_pass", "one_pass")]
                report(lines, f"B = {B:2d}  {label}", stats, diff, ws)
            for p in plans.values():
                p.close()
            del plans, x
            torch.cuda.empty_cache()
        lines.append("")


def video_points(dev, lines, reps, warmup):
    import lstm_plan_cases as lc
    from oracle import unipose_oracle as O
    from unipose_amd import _C
    from unipose_amd.plan import UniPoseLSTMPlan
    L = _C.lib()
    m = lc.lstm_model(dev, VIDEO_K)
    for storage in STORAGES:
        lines.append(f"video plan, K = {VIDEO_K}, T = {VIDEO_T}, {SIZE} x {SIZE}, {storage} storage; ms per call")
        for B in VIDEO_BATCHES:
            x = O.synth_input((B, VIDEO_T, 3, SIZE, SIZE), 15).to(dev)
            cm = O.synth_input((B, VIDEO_T, 1, SIZE, SIZE), 16, "rand").to(dev)
            rng = np.random.default_rng(3)
            cen, sc = rng.uniform(150, 220, (B, VIDEO_T, 2)), rng.uniform(1.2, 1.8, (B, VIDEO_T))
            plans = {"two_pass": UniPoseLSTMPlan(m, B, SIZE, SIZE, frames=VIDEO_T, storage=storage),
                     "one_pass": UniPoseLSTMPlan(m, B, SIZE, SIZE, frames=VIDEO_T, storage=storage, flip="one_pass")}
            call = lambda p: p.clip_final_preds(x, cm, cen, sc, flip=True, pairs=PAIRS)[0]        # noqa: E731
            diff = float((call(plans["two_pass"]) - call(plans["one_pass"])).abs().max())
            stats = measure(dev, {name: (lambda p=p: call(p)) for name, p in plans.items()}, reps, warmup)
            ws = [L.up_unipose_lstm_plan_program_workspace(plans[n]._plan, 5) for n in ("two_pass", "one_pass")]
            report(lines, f"B = {B:2d}  clip_final_preds(flip=True)", stats, diff, ws)
            for p in plans.values():
                p.close()
            del plans, x, cm
            torch.cuda.empty_cache()
        lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flip_one_pass.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("image", "video"), default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_flip_one_pass.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = [f"the flip test in one trunk pass over 2 B images against two passes over B, on {torch.cuda.get_device_name(dev)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in ms", "gain / loss: the [p10 .. p90] intervals of the two forms do not overlap", ""]
    if args.only != "video":
        image_points(dev, lines, args.reps, args.warmup)
    if args.only != "image":
        video_points(dev, lines, args.reps, args.warmup)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
