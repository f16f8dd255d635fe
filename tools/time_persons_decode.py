"""What does the one-launch multi-person decode buy?  (GPU; a measurement, not a test.)

    timeout -k 10 300 python tools/time_persons_decode.py [--out profiles/persons_decode.txt] [--reps 50]

Times three ways to decode the persons of `lsp_two` from the G9 fixture (two persons, 20 maps of 46 x 46), at B = 1 and B = 32
(the sample repeated):

    per sample   ops.uniPose_kpts once per sample: up_peak_mask, torch.nonzero and the lists on the host, up_box_argmax, the copy back
    batch list   ops.uniPose_kpts_batch: one up_persons_decode launch and one copy to the host, then the Python lists
    device only  ops.persons_decode: the launch alone, results left on the device

Wall time of a call (time.perf_counter) with a device synchronise before and after, the median of the repetitions after a
warm-up, with the 10th / 90th percentiles.  The three forms alternate inside every repetition so that they see the same machine.
The lists of the first two forms are compared first (they must be equal).  Writes the report to --out and prints it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 32)


def measure(ops, maps, reps, warmup):
    dev = maps.device
    forms = {"per sample": lambda: [ops.uniPose_kpts(maps[b:b + 1], "LSP") for b in range(maps.shape[0])],
             "batch list": lambda: ops.uniPose_kpts_batch(maps, "LSP"),
             "device only": lambda: ops.persons_decode(maps, "LSP")}
    equal = forms["per sample"]() == forms["batch list"]()
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
            times[name].append((time.perf_counter() - t0) * 1e6)          # us
    return equal, times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "persons_decode.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 30:
        raise SystemExit("at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_persons_decode.py measures on the GPU; there is none here")
    from unipose_amd import ops
    dev = torch.device("cuda:0")
    one = np.load(os.path.join(ROOT, "tests", "golden", "g9_multi_person.npz"))["lsp_two_maps"]
    lines = [f"multi-person decode of lsp_two (G9: two persons, 20 maps of 46 x 46) on {torch.cuda.get_device_name(dev)}",
             f"wall time of a call with a synchronise, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in us", ""]
    for B in BATCHES:
        maps = torch.from_numpy(one).repeat(B, 1, 1, 1).contiguous().to(dev)
        equal, times = measure(ops, maps, args.reps, args.warmup)
        lines.append(f"B = {B}   (lists of the per-sample and the batch form equal: {equal})")
        med = {}
        for name, t in times.items():
            t = sorted(t)
            med[name] = statistics.median(t)
            lines.append(f"  {name:12s} {med[name]:10.1f} us [{t[len(t) // 10]:10.1f} .. {t[len(t) * 9 // 10]:10.1f}]")
        lines.append(f"  per sample / batch list = {med['per sample'] / med['batch list']:.2f}x,  "
                     f"per sample / device only = {med['per sample'] / med['device only']:.2f}x")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
