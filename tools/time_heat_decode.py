"""What does the fused key-point decode buy at full resolution?  (GPU; a measurement, not a test.)

    timeout -k 10 300 python tools/time_heat_decode.py [--out profiles/heat_decode.txt] [--reps 100]

Times up_heatmap_decode straight from the NHWC heat-maps against the composition it replaces on the same tensors
(up_bilinear_fwd -> up_nhwc_to_nchw -> up_heatmap_argmax), at the two sizes a user runs:

    B = 32, K = 16, 46 x 46 -> 368 x 368      B = 16, K = 16, 92 x 92 -> 736 x 736

Both forms are called through the C ABI on preallocated buffers, alternating, after a warm-up; every repetition is bracketed
by two hipEvents and the median is reported with the 10th / 90th percentiles.  The results of the two forms are compared first
(they must be equal).  The bytes are those the algorithm moves, computed from the shapes: whole NHWC rows (pad channels
included) where a kernel reads or writes NHWC.  Writes the report to --out and prints it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(32, 16, 46, 46, 368, 368), (16, 16, 92, 92, 736, 736)]


def rup4(c):
    return (c + 3) // 4 * 4


def measure(L, dev, B, K, h, w, P, Q, reps, warmup):
    J, ld = K + 1, rup4(K + 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    torch.manual_seed(0)
    x = torch.zeros(B, h, w, ld, device=dev)
    x[..., :J] = torch.randn(B, h, w, J, device=dev)
    up = torch.empty(B, P, Q, ld, device=dev)
    nchw = torch.empty(B, J, P, Q, device=dev)
    outs = [(torch.empty(B, J, dtype=torch.int32, device=dev), torch.empty(B, J, 2, device=dev), torch.empty(B, J, device=dev))
            for _ in range(2)]

    def fused():
        i, p, m = outs[0]
        e = L.up_heatmap_decode(x.data_ptr(), h * w * ld, 1, ld, B, J, h, w, P, Q, i.data_ptr(), p.data_ptr(), m.data_ptr(), stream)
        assert e == 0, L.up_last_error()

    def composed():
        i, p, m = outs[1]
        e = L.up_bilinear_fwd(x.data_ptr(), ld, up.data_ptr(), ld, B, h, w, ld, P, Q, stream)
        e = e or L.up_nhwc_to_nchw(up.data_ptr(), ld, nchw.data_ptr(), B, J, P, Q, stream)
        e = e or L.up_heatmap_argmax(nchw.data_ptr(), B, J, P, Q, i.data_ptr(), p.data_ptr(), m.data_ptr(), stream)
        assert e == 0, L.up_last_error()

    fused()
    composed()
    torch.cuda.synchronize(dev)
    equal = all(torch.equal(a, b) for a, b in zip(*outs))
    for _ in range(warmup):
        fused()
        composed()
    torch.cuda.synchronize(dev)
    times = {"fused": [], "composed": []}
    for _ in range(reps):
        for name, fn in (("fused", fused), ("composed", composed)):       # alternating: both see the same machine
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)                     # us
    coarse, fine_nhwc, fine_nchw, small = B * h * w * ld * 4, B * P * Q * ld * 4, B * J * P * Q * 4, B * J * 16
    moved = {"fused": coarse + small,
             # bilinear: coarse in, fine NHWC out; layout pass: fine NHWC in, fine NCHW out; argmax: fine NCHW in
             "composed": coarse + fine_nhwc + fine_nhwc + fine_nchw + fine_nchw + small}
    return equal, times, moved


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heat_decode.txt"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if args.reps < 50:
        raise SystemExit("at least 50 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_heat_decode.py measures on the GPU; there is none here")
    from unipose_amd import _C
    L = _C.lib()
    dev = torch.device("cuda:0")
    lines = [f"up_heatmap_decode from NHWC vs up_bilinear_fwd -> up_nhwc_to_nchw -> up_heatmap_argmax on {torch.cuda.get_device_name(dev)}",
             f"hipEvents around every repetition, {args.warmup} warm-up + {args.reps} timed repetitions per form, alternating; "
             "median [p10 .. p90] in us; bytes computed from the shapes", ""]
    for B, K, h, w, P, Q in SIZES:
        equal, times, moved = measure(L, dev, B, K, h, w, P, Q, args.reps, args.warmup)
        lines.append(f"B = {B}, K = {K}, {h} x {w} -> {P} x {Q}   ({B * (K + 1)} maps; results of the two forms equal: {equal})")
        med = {}
        for name in ("fused", "composed"):
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:9s} {med[name]:9.1f} us [{t[len(t) // 10]:9.1f} .. {t[len(t) * 9 // 10]:9.1f}]   "
                         f"{moved[name] / 1e6:9.2f} MB moved   {moved[name] / med[name] / 1e3:8.1f} GB/s")
        ratio = med["composed"] / med["fused"]
        lines.append(f"  composed / fused = {ratio:.2f}x" + ("" if ratio > 1 else "   (the fused form is NOT faster here)"))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
