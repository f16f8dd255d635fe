"""What does pose from source frames in one call buy?  (GPU; a measurement, not a test.)

    timeout -k 10 600 python tools/time_frame_pose.py [--out profiles/frame_pose.txt] [--reps 30]

Times two ways to get the final_preds key points of persons found in ONE 1080 x 1920 uint8 camera frame (MPII, 16 joints, 368 x 368
network input), at B = 1 and B = 8 persons, with the flip test off and on, from the frame on the device to the (B, 17, 2)
predictions on the device:

    one call      UniPosePlan.frame_final_preds(frame, center, scale, frame_of=[0] * B, flip=...): up_unipose_frame_final_preds
    composition   what a user wrote in front of the plan before, from code the parent commit already has: the frame replicated
                  once per person (frame.expand(B, ...).contiguous(): up_augment_image takes one source image per sample),
                  ops.augment_image with the hand-built map, then UniPosePlan.final_preds(x, center, scale, flip=...)

Wall time of a call (time.perf_counter) with a device synchronise before and after, the median of the repetitions after a warm-up,
with the 10th / 90th percentiles; the two forms alternate inside every repetition so that they see the same machine.  The results
of the two forms are compared first (they must be equal bit for bit).  Then the crop alone: up_crop_to_nhwc (both outputs with the
flip test, else one) beside up_augment_image + the layout pass(es) it replaces, device events around 20 launches each.  Writes
the report to --out and prints it."""
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

BATCHES = (1, 8)
K, SIZE, FRAME = 16, 368, (1080, 1920)


def spread(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[len(t) * 9 // 10]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_pose.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_frame_pose.py measures on the GPU; there is none here")
    import model_cases as mc
    from unipose_amd import _C, ops, protocol
    from unipose_amd.plan import UniPosePlan
    dev = torch.device("cuda:0")
    m, _ = mc.build_image_model(K, 3, dev)
    m.eval()
    rng = np.random.default_rng(23)
    frame = torch.from_numpy(rng.integers(0, 256, (1, *FRAME, 3), dtype=np.uint8)).to(dev)
    frame_bytes = frame.numel()
    lines = [f"pose from a {FRAME[0]} x {FRAME[1]} uint8 frame, MPII ({K} joints), {SIZE} x {SIZE} input, on {torch.cuda.get_device_name(dev)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in ms", ""]
    L = _C.lib()
    for B in BATCHES:
        cen = np.stack([np.array([300.0 + 180.0 * i, 540.0 + 20.0 * (i % 3)]) for i in range(B)])
        sc = np.array([2.2 + 0.15 * i for i in range(B)])
        fo = [0] * B
        plan = UniPosePlan(m, B, SIZE, SIZE)
        maps = protocol.crop_maps(cen, sc, [SIZE, SIZE])
        for flip in (False, True):
            def one_call():
                return plan.frame_final_preds(frame, cen, sc, frame_of=fo, flip=flip, dataset="MPII")

            def composition():
                src = frame.expand(B, -1, -1, -1).contiguous()
                x = ops.augment_image(src, maps.reshape(B, 2, 3), (SIZE, SIZE))
                return plan.final_preds(x, cen, sc, flip=flip, dataset="MPII")

            equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one_call(), composition()))
            forms = {"one call": one_call, "composition": composition}
            for _ in range(args.warmup):
                for fn in forms.values():
                    fn()
            times = {name: [] for name in forms}
            for _ in range(args.reps):
                for name, fn in forms.items():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    times[name].append((time.perf_counter() - t0) * 1e3)
            lines.append(f"B = {B}, flip test {'on' if flip else 'off'}   (results of the two forms equal bit for bit: {equal})")
            med = {}
            for name, t in times.items():
                med[name], lo, hi = spread(t)
                lines.append(f"  {name:12s} {med[name]:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]")
            lines.append(f"  composition / one call = {med['composition'] / med['one call']:.3f}x")
            lines.append(f"  source bytes the composition replicates: {B} x {frame_bytes} = {B * frame_bytes} "
                         f"({B * frame_bytes / 2 ** 20:.1f} MiB); the one call reads the frame in place")
            # the crop alone
            st = torch.cuda.current_stream(dev).cuda_stream
            src = frame.expand(B, -1, -1, -1).contiguous()
            inv = torch.from_numpy(maps).to(dev)
            fot = torch.tensor(fo, dtype=torch.int32, device=dev)
            x = torch.empty((B, 3, SIZE, SIZE), device=dev)
            y, yf = torch.empty((B, SIZE, SIZE, 4), device=dev), torch.empty((B, SIZE, SIZE, 4), device=dev)

            def crop():
                return L.up_crop_to_nhwc(frame.data_ptr(), 0, 1, *FRAME, 3, fot.data_ptr(), None, inv.data_ptr(), B, 128.0, 128.0, 256.0,
                                         y.data_ptr(), yf.data_ptr() if flip else None, SIZE, SIZE, 4, st)

            def staged():
                e = L.up_augment_image(src.data_ptr(), 0, B, *FRAME, 3, None, inv.data_ptr(), 1, 128.0, 128.0, 256.0, x.data_ptr(), SIZE,
                                       SIZE, st)
                e |= L.up_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), B, 3, SIZE, SIZE, 4, st)
                if flip:
                    e |= L.up_nchw_to_nhwc_flip(x.data_ptr(), yf.data_ptr(), B, 3, SIZE, SIZE, 4, st)
                return e

            for name, fn in (("up_crop_to_nhwc", crop), ("augment + layout pass" + ("es" if flip else ""), staged)):
                assert fn() == 0, name
                ts = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) / 20 * 1e3)
                md, lo, hi = spread(ts)
                lines.append(f"  {name:24s} {md:8.1f} us per call [{lo:8.1f} .. {hi:8.1f}]  (20 back-to-back calls between two events; "
                             "without the replication)")
            lines.append("")
        plan.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
