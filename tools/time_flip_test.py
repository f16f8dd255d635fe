"""What does the one-call flip test + final_preds buy?  (GPU; a measurement, not a test.)

    timeout -k 10 600 python tools/time_flip_test.py [--out profiles/flip_test.txt] [--reps 30]

Times two ways to get the final_preds key points of the flip-tested network (MPII, 16 joints, 368 x 368 input) at B = 1 and
B = 32, from the input batch on the device to the (B, 17, 2) predictions:

    one call      UniPosePlan.final_preds(x, center, scale, flip=True): up_unipose_final_preds, results left on the device
    composition   what a user had to write around the plan before: plan(x), plan(torch.flip(x, [3])), torch.flip + index_select
                  of the second maps, add, * 0.5, ops.heatmap_argmax, the copy of maps and peaks to the host and the per-joint
                  refinement / transform loop of pytorch-pose's final_preds in numpy

Wall time of a call (time.perf_counter) with a device synchronise before and after, the median of the repetitions after a warm-up,
with the 10th / 90th percentiles; the two forms alternate inside every repetition so that they see the same machine.  The
predictions of the two forms are compared first (they must be equal).  Then the three kernels alone (up_nchw_to_nhwc_flip on the
input, up_flip_merge and up_final_preds on NHWC maps of the network's size), device events around 20 launches each, the median of
the repetitions.  Writes the report to --out and prints it."""
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

BATCHES = (1, 32)
K, SIZE = 16, 368


def host_final_preds(maps, peaks, maxvals, inv, res):
    """pytorch-pose's final_preds on host arrays: maps (B,J,H,W), peaks (B,J,2) 0-based (get_max_preds), per joint in Python"""
    b, j, h, w = maps.shape
    out = np.zeros((b, j, 2), np.float32)
    for n in range(b):
        for p in range(j):
            hm = maps[n, p]
            x, y = (peaks[n, p] + 1) * (maxvals[n, p, 0] > 0)
            px, py = int(x), int(y)
            if 1 < px < res[0] and 1 < py < res[1] and px < w and py < h:
                x += np.float32(0.25) * np.sign(hm[py - 1][px] - hm[py - 1][px - 2])
                y += np.float32(0.25) * np.sign(hm[py][px - 1] - hm[py - 2][px - 1])
            pt = np.array([x + np.float32(0.5) - 1, y + np.float32(0.5) - 1], dtype=np.float64)
            v = (inv[n, :, 0] * pt[0] + inv[n, :, 1] * pt[1]) + inv[n, :, 2]
            out[n, p] = v.astype(np.int64) + 1
    return out


def spread(t):
    t = sorted(t)
    return statistics.median(t), t[len(t) // 10], t[len(t) * 9 // 10]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flip_test.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_flip_test.py measures on the GPU; there is none here")
    import model_cases as mc
    from oracle import unipose_oracle as O
    from unipose_amd import _C, ops, protocol
    from unipose_amd.plan import UniPosePlan
    dev = torch.device("cuda:0")
    m, _ = mc.build_image_model(K, 3, dev)
    m.eval()
    perm = protocol.flip_perm("MPII", K)
    perm_t = torch.tensor(perm, device=dev)
    lines = [f"flip test + final_preds, MPII ({K} joints), {SIZE} x {SIZE} input, on {torch.cuda.get_device_name(dev)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in ms", ""]
    for B in BATCHES:
        x = O.synth_input((B, 3, SIZE, SIZE), 9).to(dev)
        cen = np.stack([np.array([180.0 + i, 190.0 - i]) for i in range(B)])
        sc = np.array([1.5 + 0.01 * i for i in range(B)])
        plan = UniPosePlan(m, B, SIZE, SIZE)
        res = [plan.map_width, plan.map_height]
        inv = protocol.inverse_maps(cen, sc, res)

        def one_call():
            return plan.final_preds(x, cen, sc, res, flip=True, dataset="MPII")[0]

        def composition():
            a = plan(x)
            f = plan(torch.flip(x, [3]))
            merged = (a + torch.flip(f, [3]).index_select(1, perm_t)) * 0.5
            peaks, mx, _ = ops.heatmap_argmax(merged)
            return host_final_preds(merged.cpu().numpy(), peaks.cpu().numpy(), mx.cpu().numpy(), inv, res)

        equal = bool(np.array_equal(one_call().cpu().numpy(), composition()))
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
        lines.append(f"B = {B}   (predictions of the two forms equal: {equal})")
        med = {}
        for name, t in times.items():
            med[name], lo, hi = spread(t)
            lines.append(f"  {name:12s} {med[name]:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]")
        lines.append(f"  composition / one call = {med['composition'] / med['one call']:.3f}x")
        # the three kernels alone, on tensors of this batch's sizes
        L = _C.lib()
        h, w, ld = plan.map_height, plan.map_width, (K + 1 + 3) // 4 * 4
        xin = torch.empty((B, SIZE, SIZE, 4), device=dev)
        a = torch.randn((B, h, w, ld), device=dev)
        f = torch.randn((B, h, w, ld), device=dev)
        out = torch.empty_like(a)
        inv_t = torch.from_numpy(inv).to(dev)
        preds, coords, mx = torch.empty((B, K + 1, 2), device=dev), torch.empty((B, K + 1, 2), device=dev), torch.empty((B, K + 1), device=dev)
        pa = ops._perm_array(perm, K + 1)
        st = torch.cuda.current_stream(dev).cuda_stream
        sb = h * w * ld
        kernels = {
            "up_nchw_to_nhwc_flip": lambda: L.up_nchw_to_nhwc_flip(x.data_ptr(), xin.data_ptr(), B, 3, SIZE, SIZE, 4, st),
            "up_flip_merge": lambda: L.up_flip_merge(a.data_ptr(), f.data_ptr(), sb, 1, ld, B, K + 1, h, w, pa, out.data_ptr(), sb, 1, ld, st),
            "up_final_preds": lambda: L.up_final_preds(out.data_ptr(), sb, 1, ld, B, K + 1, h, w, w, h, inv_t.data_ptr(), preds.data_ptr(),
                                                       coords.data_ptr(), mx.data_ptr(), st),
        }
        for name, fn in kernels.items():
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
            lines.append(f"  {name:22s} {md:8.1f} us per launch [{lo:8.1f} .. {hi:8.1f}]  (20 back-to-back launches between two events)")
        lines.append("")
        plan.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
