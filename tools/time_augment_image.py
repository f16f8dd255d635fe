"""Cost of the augmentation on the device (profiles/augment_image.txt): the kernel by device events for B = 32, 368 x 368 output
from 368 x 368 uint8 sources with an identity map and with a typical augmenting map, beside `pixels.float()` +
`ops.normalize_image` (the path it replaces when the option is on, untouched by it) and the traffic floor; and the wall time of
one `DeviceBatcher` call with and without `augment`.  Needs the GPU; prints the table.

    python tools/time_augment_image.py [--batch 32] [--size 368] [--iters 200]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unipose_amd import augment as A  # noqa: E402
from unipose_amd import ops  # noqa: E402
from unipose_amd.trainer import DeviceBatcher, SyntheticPoseData  # noqa: E402


def device_us(fn, iters, rounds=5):
    """median over `rounds` of the mean device time of `iters` back-to-back calls (events around the window)"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(res)), float(min(res)), float(max(res))


def wall_ms(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t) * 1e3)
    return float(np.median(res)), float(min(res)), float(max(res))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--size", type=int, default=368)
    p.add_argument("--iters", type=int, default=200)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_augment_image.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    b, s = args.batch, args.size
    item = next(iter(SyntheticPoseData(14, b, 1, size=s, seed=1)))
    px = item["pixels"].to(dev)
    ident = np.repeat(np.array([[[1.0, 0, 0], [0, 1.0, 0]]]), b, axis=0)
    aug = A.Augmenter("LSP", crop=s, seed=3)
    typical = aug((s, s), item["kpts"], item["center"])[0]
    ident_d, typical_d = ops._as_f64(ident, dev), ops._as_f64(typical, dev)
    floor_mb = b * (s * s * 3 + s * s * 3 * 4) / 1e6
    print("device: %s; B = %d, %d x %d x 3 uint8 -> %d x %d float32; traffic floor %.1f MB (read once, written once)"
          % (torch.cuda.get_device_name(0), b, s, s, s, s, floor_mb))
    print("kernel time by device events, us per call: median (min .. max) of 5 windows of %d calls" % args.iters)
    rows = (("up_augment_image, identity map", lambda: ops.augment_image(px, ident_d, (s, s))),
            ("up_augment_image, typical map (Augmenter draw)", lambda: ops.augment_image(px, typical_d, (s, s))),
            ("pixels.float() + up_normalize_image", lambda: ops.normalize_image(px.float())),
            ("up_normalize_image alone (float32 already there)", None))
    pf = px.float()
    for name, fn in rows:
        fn = fn or (lambda: ops.normalize_image(pf))
        med, lo, hi = device_us(fn, args.iters)
        print("  %-52s %8.1f  (%.1f .. %.1f)   %6.0f GB/s of the floor's bytes" % (name, med, lo, hi, floor_mb * 1e6 / (med * 1e-6) / 1e9))
    print("wall time of one DeviceBatcher call + synchronise (upload of the uint8 pixels, targets), ms: median (min .. max) of 30")
    plain = DeviceBatcher(dev, 8, 3)
    with_aug = DeviceBatcher(dev, 8, 3, augment=A.Augmenter("LSP", crop=s, seed=3))
    for name, bt in (("without augment", plain), ("with augment", with_aug), ("without augment (again)", plain), ("with augment (again)", with_aug)):
        med, lo, hi = wall_ms(lambda: bt(item), 30)
        print("  %-52s %8.2f  (%.2f .. %.2f)" % (name, med, lo, hi))
    t = time.perf_counter()
    for _ in range(20):
        aug((s, s), item["kpts"], item["center"])
    print("  of which the host side of the augmenter (draws, %d maps, points), ms: %.2f" % (b, (time.perf_counter() - t) * 1e3 / 20))


if __name__ == "__main__":
    main()
