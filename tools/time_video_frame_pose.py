"""What does the video plan from source frames in one call buy?  (GPU; a measurement, not a test.)

    timeout -k 10 900 python tools/time_video_frame_pose.py [--out profiles/video_frame_pose.txt] [--reps 30]

Times two ways to get the final_preds key points of a clip (Penn_Action, 13 joints, T = 5 frames, 368 x 368 network input) whose
frames are crops of 1080 x 1920 uint8 camera frames on the device, at B = 1 and B = 8 clips, with the flip test off and on, from
the frames on the device to the (B, T, 14, 2) predictions on the device:

    one call      UniPoseLSTMPlan.clip_frame_final_preds(frames, center, scale, frame_of=...): up_unipose_lstm_clip_frame_final_preds
    composition   what a user wrote in front of the plan before, from code the parent commit already has: the frames replicated
                  once per sample (frames[frame_of]: up_augment_image takes one source image per sample), ops.augment_image
                  with the hand-built maps, B * T full-resolution centre maps from ops.make_centermaps, then
                  UniPoseLSTMPlan.clip_final_preds(x, cm, center, scale)

and the same for one frame of a stream at B = 1: UniPoseLSTMPlan.stream_frames against frames[frame_of], ops.augment_image,
ops.make_centermaps, UniPoseLSTMPlan.stream(heat=) and ops.final_preds.

Wall time of a call (time.perf_counter) with a device synchronise before and after, the median of the repetitions after a warm-up,
with the 10th / 90th percentiles; the two forms alternate inside every repetition so that they see the same machine.  The results
of the two forms are compared first (they must be equal bit for bit).  Then the front kernels alone: up_clip_crop_to_nhwc +
up_clip_center_pool (+ _flip) beside up_augment_image + up_make_gaussian_maps + the layout and pooling passes they replace, device
events around 20 back-to-back rounds each.  Writes the report to --out and prints it."""
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
K, T, SIZE, FRAME = 13, 5, 368, (1080, 1920)
PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12]]


def spread(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[len(t) * 9 // 10]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def wall(forms, dev, warmup, reps):
    """{name: [ms]}: the forms alternating inside every repetition"""
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
    return times


def events(fn, reps):
    """[us per round]: 20 back-to-back rounds between two events"""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / 20 * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_frame_pose.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_video_frame_pose.py measures on the GPU; there is none here")
    import lstm_plan_cases as lc
    from unipose_amd import _C, ops, protocol
    from unipose_amd.plan import UniPoseLSTMPlan
    dev = torch.device("cuda:0")
    m = lc.lstm_model(dev, K)
    rng = np.random.default_rng(29)
    frames = torch.from_numpy(rng.integers(0, 256, (T, *FRAME, 3), dtype=np.uint8)).to(dev)      # one camera, T frames
    frame_bytes = frames[0].numel()
    map_bytes = SIZE * SIZE * 4
    P = (SIZE - 7) // 8 + 1
    lines = [f"a clip of {T} crops of {FRAME[0]} x {FRAME[1]} uint8 frames, Penn_Action ({K} joints), {SIZE} x {SIZE} input, on "
             f"{torch.cuda.get_device_name(dev)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in ms", ""]
    L = _C.lib()
    ratios, fronts = [], []
    for B in BATCHES:
        n = B * T
        cen = np.array([[[300.0 + 180.0 * b + 6.0 * t, 540.0 + 20.0 * (b % 3) - 4.0 * t] for t in range(T)] for b in range(B)])
        sc = np.array([[2.2 + 0.15 * b + 0.02 * t for t in range(T)] for b in range(B)])
        fo = np.array([[t for t in range(T)] for b in range(B)])                # B persons tracked through the same T frames
        cc = np.array([[[SIZE // 2 + 0.5 * t - b, SIZE // 2 - 0.25 * t + b] for t in range(T)] for b in range(B)], dtype=np.float64)
        fot = torch.from_numpy(fo.reshape(-1)).to(dev)
        plan = UniPoseLSTMPlan(m, B, SIZE, SIZE, frames=T)
        maps = protocol.crop_maps(cen.reshape(n, 2), sc.reshape(n), [SIZE, SIZE])
        for flip in (False, True):
            pairs = PAIRS if flip else None

            def one_call():
                return plan.clip_frame_final_preds(frames, cen, sc, frame_of=fo, flip=flip, pairs=pairs, crop_center=cc)

            def composition():
                src = frames[fot]
                x = ops.augment_image(src, maps.reshape(n, 2, 3), (SIZE, SIZE)).reshape(B, T, 3, SIZE, SIZE)
                cm = ops.make_centermaps(cc.reshape(n, 2), SIZE, SIZE, 3.0, device=dev).reshape(B, T, 1, SIZE, SIZE)
                return plan.clip_final_preds(x, cm, cen, sc, flip=flip, pairs=pairs)

            equal = same_bits(one_call(), composition())
            times = wall({"one call": one_call, "composition": composition}, dev, args.warmup, args.reps)
            lines.append(f"clip, B = {B}, T = {T}, flip test {'on' if flip else 'off'}   (results of the two forms equal bit for bit: {equal})")
            med = {}
            for name, t in times.items():
                med[name], lo, hi = spread(t)
                lines.append(f"  {name:12s} {med[name]:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]")
            ratios.append(med["composition"] / med["one call"])
            lines.append(f"  composition / one call = {ratios[-1]:.3f}x")
            lines.append(f"  bytes the composition stages: {n} replicated frames = {n * frame_bytes} ({n * frame_bytes / 2 ** 20:.1f} MiB), "
                         f"{n} centre maps of {SIZE} x {SIZE} = {n * map_bytes} ({n * map_bytes / 2 ** 20:.1f} MiB), the NCHW clip = "
                         f"{n * 3 * map_bytes} ({n * 3 * map_bytes / 2 ** 20:.1f} MiB); the one call reads the frames in place and "
                         f"writes {n} x {P} x {P} pooled values")
            # the front kernels alone
            st = torch.cuda.current_stream(dev).cuda_stream
            src = frames[fot].contiguous()
            inv = torch.from_numpy(maps).to(dev)
            fo32 = torch.from_numpy(fo).to(device=dev, dtype=torch.int32).contiguous()
            cxy = torch.from_numpy(cc).to(dev)
            x = torch.empty((n, 3, SIZE, SIZE), device=dev)
            cm = torch.empty((n, 1, SIZE, SIZE), device=dev)
            y, yf = torch.empty((n, SIZE, SIZE, 4), device=dev), torch.empty((n, SIZE, SIZE, 4), device=dev)
            z, zf = torch.zeros((n, P, P, 16), device=dev), torch.zeros((n, P, P, 16), device=dev)

            def front():
                e = L.up_clip_crop_to_nhwc(frames.data_ptr(), 0, T, *FRAME, 3, fo32.data_ptr(), None, inv.data_ptr(), B, T, 128.0, 128.0,
                                           256.0, y.data_ptr(), yf.data_ptr() if flip else None, SIZE, SIZE, 4, st)
                e |= L.up_clip_center_pool(cxy.data_ptr(), 3.0, z.data_ptr(), 16, 14, B, T, SIZE, SIZE, P, P, st)
                if flip:
                    e |= L.up_clip_center_pool_flip(cxy.data_ptr(), 3.0, zf.data_ptr(), 16, 14, B, T, SIZE, SIZE, P, P, st)
                return e

            def staged():
                e = L.up_augment_image(src.data_ptr(), 0, n, *FRAME, 3, None, inv.data_ptr(), 1, 128.0, 128.0, 256.0, x.data_ptr(), SIZE,
                                       SIZE, st)
                e |= L.up_make_gaussian_maps(cxy.data_ptr(), n, SIZE, SIZE, 3.0, cm.data_ptr(), st)
                e |= L.up_clip_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), B, T, 3, SIZE, SIZE, 4, st)
                e |= L.up_clip_avgpool9s8_fwd(cm.data_ptr(), z.data_ptr(), 16, 14, B, T, SIZE, SIZE, P, P, st)
                if flip:
                    e |= L.up_clip_nchw_to_nhwc_flip(x.data_ptr(), yf.data_ptr(), B, T, 3, SIZE, SIZE, 4, st)
                    e |= L.up_clip_avgpool9s8_flip_fwd(cm.data_ptr(), zf.data_ptr(), 16, 14, B, T, SIZE, SIZE, P, P, st)
                return e

            mds = []
            for name, fn in (("clip crop + centre pool" + ("s" if flip else ""), front),
                             ("augment, Gaussian, layout, pool", staged)):
                assert fn() == 0, name
                md, lo, hi = spread(events(fn, args.reps))
                mds.append(md)
                lines.append(f"  {name:32s} {md:8.1f} us per round [{lo:8.1f} .. {hi:8.1f}]  (20 back-to-back rounds between two events; "
                             "without the replication)")
            fronts.append(mds[1] / mds[0])
            lines.append("")
        plan.close()
    # one frame of a stream at B = 1
    plan = UniPoseLSTMPlan(m, 1, SIZE, SIZE)
    cen, sc, cc = np.array([[960.0, 540.0]]), np.array([2.4]), np.array([[SIZE // 2 + 1.5, SIZE // 2 - 0.5]])
    maps = protocol.crop_maps(cen, sc, [SIZE, SIZE]).reshape(1, 2, 3)
    sa, sb = plan.stream_state(), plan.stream_state()
    heat = torch.empty((1, K + 1, plan.out_height, plan.out_width), device=dev)

    def stream_call(first=False):
        return plan.stream_frames(frames, cen, sc, sa, first=first, frame_of=[2], crop_center=cc)

    def stream_composition(first=False):
        x = ops.augment_image(frames[2:3], maps, (SIZE, SIZE))
        cm = ops.make_centermaps(cc, SIZE, SIZE, 3.0, device=dev)
        plan.stream(x, cm, sb, first=first, heat=heat)
        return ops.final_preds(heat, cen, sc, return_coords=True)

    equal = same_bits(stream_call(True), stream_composition(True)) and same_bits(stream_call(), stream_composition())
    times = wall({"one call": stream_call, "composition": stream_composition}, dev, args.warmup, args.reps)
    lines.append(f"stream, B = 1, a later frame   (results of the two forms equal bit for bit: {equal})")
    med = {}
    for name, t in times.items():
        med[name], lo, hi = spread(t)
        lines.append(f"  {name:12s} {med[name]:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]")
    stream_ratio = med["composition"] / med["one call"]
    lines.append(f"  composition / one call = {stream_ratio:.3f}x")
    lines.append(f"  bytes the composition stages: one centre map = {map_bytes}, the NCHW frame = {3 * map_bytes}, the NCHW heat-maps for "
                 "ops.final_preds; the one call reads the camera frame in place")
    lines.append("")
    plan.close()
    lo, hi = min(ratios), max(ratios)
    faster = lo > 1.02
    lines.append("In plain words: end to end the one-call clip entry is " + ("faster" if faster else "NOT faster" if hi < 1.02 else
                 "faster in some cases and not in others") + f" than the composition (composition / one call {lo:.3f}x .. {hi:.3f}x over "
                 f"B = 1 / 8, flip test off / on); for one frame of a stream the ratio is {stream_ratio:.3f}x.  The network takes "
                 "milliseconds, the step in front of it microseconds either way.  The front kernels alone are "
                 f"{min(fronts):.1f}x .. {max(fronts):.1f}x shorter than the launches they replace.  What the entries are for is the "
                 "missing capability (camera frames, centres and scales in, joints in frame pixels out, in one C call) and the staging "
                 "they remove (replicated frames, full-resolution centre maps, the NCHW clip), not a headline number.")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
