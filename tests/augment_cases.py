"""Augmentation on the device (up_augment_image, ops.augment_image, unipose_amd/augment.py, DeviceBatcher(augment=...), Trainer with
args.augment): shared by test_augment_emu.py and test_augment_gpu.py.

Yardsticks.  The fixture G20 (tools/make_goldens.py g20) holds what the reference's OWN utils/Mytransforms.py computes for explicit
parameters: the points through resize / rotate / RandomCrop.get_params / crop / hflip / hflip_BBC (and through its Compose), and the
pixels through crop / hflip / to_tensor / normalize, which are pure numpy.  Nothing of the reference's image RESAMPLING is in it:
OpenCV is not installed where the fixture was made, so resize and warpAffine ran as shape-only stand-ins (tools/cv2_standin.py).
Beyond the fixture the reference is `restate`, the entry's documented semantics (include/unipose_hip.h) in float64 numpy.

POINT_TOL.  compose + transform_points and the reference both work in float64 on values up to about 1e3; the composition only
reorders a handful of multiplications and additions (ratio folded into the matrix, offsets into the translation), each worth one
rounding of 2^-53 * 1e3 = 1.1e-13: 1e-9 pixels is four orders above that and nine below a pixel.

BOUND for the entry against `restate`, from the float32 operation order of the header, with u = 2^-24, source values, border and
mean in 0 .. M, M = max(255, |border|):
    fx, fy       one rounding of an exact float64 difference in [0, 1]: moves a blend by at most u * M each;
    v01 - v00    one rounding, at most u * M;   top = fmaf(fx, ., v00) one rounding of a value in 0 .. M, u * M:  top within 3 u M,
    bot          likewise 3 u M;   val = fmaf(fy, bot - top, top): a convex mix of top and bot (3 u M) + the rounded difference
                 (u M) + fy's rounding (u M) + the fmaf's (u M) = 6 u M;
    val - mean   a value in -M .. M: u M more, 7 u M;   / std: 7 u M / std + one rounding of a quotient <= M / std = 8 u M / std.
A ninth u M / std covers the second-order terms and the float64 roundings of `restate` itself.  The coordinates: the device
evaluates sx = fma(i0, u, fma(i1, v, i2)) with two roundings, numpy's i0*u + i1*v + i2 with four, each at most
2^-53 * S, S = |i0| u + |i1| v + |i2|; bilinear sampling with a blending border is continuous with slope <= M per pixel in x and
in y (also across an integer, so a floor() that lands on the other side costs nothing extra), hence a further
M * 2^-50 * (Sx + Sy) / std per element.  No element is excluded.  WORST keeps the largest error / bound the run saw."""
import math
import os

import numpy as np
import torch

from unipose_amd import _C, ops
from unipose_amd import augment as A

F32 = torch.float32
U = 2.0 ** -24
SENT = 7.0
POINT_TOL = 1e-9
WORST = {"ratio": 0.0, "err": 0.0, "elements": 0}
U8, PF32 = 0, 1                                     # UP_PIX_U8, UP_PIX_F32
BIG = (20, 400, 300, 368)                           # 20 x 368 x 368 = 2 708 480 output pixels (> 2^21): a second grid trip


def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_augment.npz"))


# ---- the entry's semantics in float64 numpy ----------------------------------------------------------------------------------------
def restate(src, inv, out_hw, border=128.0, mean=128.0, std=256.0, valid=None, fpm=1):
    """src (B,Hs,Ws,C) numpy, inv (B / fpm, 2, 3) -> ((B,C,Ho,Wo) float64, (B,Ho,Wo) coordinate allowance in pixels)"""
    src = np.asarray(src)
    b, hs, ws, c = src.shape
    ho, wo = out_hw
    inv = np.asarray(inv, dtype=np.float64).reshape(-1, 6)
    u, v = np.meshgrid(np.arange(wo, dtype=np.float64), np.arange(ho, dtype=np.float64))
    out, slack = np.empty((b, c, ho, wo)), np.empty((b, ho, wo))
    for i in range(b):
        m = inv[i // fpm]
        hv, wv = (hs, ws) if valid is None else (min(max(int(valid[i][0]), 0), hs), min(max(int(valid[i][1]), 0), ws))
        sx, sy = m[0] * u + m[1] * v + m[2], m[3] * u + m[4] * v + m[5]
        slack[i] = 2.0 ** -50 * (abs(m[0]) * u + abs(m[1]) * v + abs(m[2]) + abs(m[3]) * u + abs(m[4]) * v + abs(m[5]))
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0

        def tap(yy, xx):
            inside = (xx >= 0) & (xx < wv) & (yy >= 0) & (yy < hv)
            yi = np.clip(yy, 0, max(hv - 1, 0)).astype(np.int64)          # clipped BEFORE the cast: 1e12 stays a float until here
            xi = np.clip(xx, 0, max(wv - 1, 0)).astype(np.int64)
            return np.where(inside[..., None], src[i, yi, xi].astype(np.float64), border)
        v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        top = v00 + fx[..., None] * (v01 - v00)
        bot = v10 + fx[..., None] * (v11 - v10)
        out[i] = (((top + fy[..., None] * (bot - top)) - mean) / std).transpose(2, 0, 1)
    return out, slack


def entry(dev, src, inv, out_hw, border=128.0, mean=128.0, std=256.0, valid=None, fpm=1, alloc=None):
    """up_augment_image itself on a sentinel-filled output -> (B,C,Ho,Wo) float32 on the host.  alloc(shape, dtype) places the
    source (the emulator's guarded allocation)."""
    s = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src))
    if alloc is not None:
        g = alloc(tuple(s.shape), s.dtype)
        g.copy_(s)
        s = g
    s = s.to(dev)
    b, hs, ws, c = s.shape
    m = torch.from_numpy(np.ascontiguousarray(inv, dtype=np.float64)).to(dev)
    vt = None if valid is None else torch.tensor(np.asarray(valid), dtype=torch.int32).to(dev)
    out = torch.full((b, c, out_hw[0], out_hw[1]), SENT, dtype=F32, device=dev)
    _C.check(_C.lib().up_augment_image(s.data_ptr(), U8 if s.dtype == torch.uint8 else PF32, b, hs, ws, c,
                                       None if vt is None else vt.data_ptr(), m.data_ptr(), fpm, border, mean, std, out.data_ptr(),
                                       out_hw[0], out_hw[1], ops._stream(out)), "augment_image")
    return out.cpu()


def compare(got, ref, slack, what, border=128.0, std=256.0):
    g = got.numpy().astype(np.float64)
    assert np.isfinite(g).all(), what
    big = max(255.0, abs(border))
    bound = (9 * U + slack[:, None]) * big / std
    err = np.abs(g - ref)
    ratio = float((err / bound).max())
    WORST["ratio"], WORST["err"] = max(WORST["ratio"], ratio), max(WORST["err"], float(err.max()))
    WORST["elements"] += g.size
    print("%s: worst error %.3g = %.3f of the bound" % (what, err.max(), ratio))
    assert ratio <= 1.0, (what, ratio, float(err.max()))


def report():
    return "up_augment_image against float64: worst error %.3g, worst error / bound %.3f over %d elements" % (
        WORST["err"], WORST["ratio"], WORST["elements"])


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- maps -------------------------------------------------------------------------------------------------------------------------
def centred(src_hw, out_hw, ratio, degree, flip):
    """the composed map whose crop is centred on the image of the source's middle -> inv (2, 3)"""
    h, w = src_hw
    pre, _ = A.resize_rotate(h, w, ratio, degree)
    left, up = A.crop_offsets(A.apply(pre, (w / 2.0, h / 2.0)), out_hw)
    return A.compose(h, w, ratio, degree, left, up, out_hw, flip)[1]


KINDS = {
    "rot0": lambda s, o: centred(s, o, 1.0, 0.0, False),
    "rot37": lambda s, o: centred(s, o, 1.0, 37.0, False),
    "rot90": lambda s, o: centred(s, o, 1.0, 90.0, False),
    "rot180flip": lambda s, o: centred(s, o, 1.0, 180.0, True),
    "ratio0.3": lambda s, o: centred(s, o, 0.3, 0.0, False),
    "ratio1.1": lambda s, o: centred(s, o, 1.1, 37.0, True),
    "half": lambda s, o: np.array([[0.5, 0.0, -0.75], [0.0, 0.25, -0.5]]),       # exact fractions, crosses the near edges
}
KIND_NAMES = list(KINDS)
OUTS = [(1, 1), (5, 7), (1, 64), (2, 63), (33, 65)]          # W = 63, 64, 65 around a wavefront; 33 x 65 = 9 blocks
SRCS = [(1, 1), (2, 3), (20, 12), (12, 20)]


def _cases():
    """out x source x source type, with C, the number of maps, frames_per_map, the first map kind, the valid extents and the border
    cycling with coprime periods; sample i of a case uses kind (first + i), so every case with three maps mixes three kinds"""
    res, n = [], 0
    for out in OUTS:
        for src in SRCS:
            for typ in ("u8", "f32"):
                res.append(dict(out=out, src=src, typ=typ, c=(1, 3, 4)[n % 3], maps=(1, 3)[(n // 2) % 2], fpm=(1, 2)[(n // 3) % 2],
                                kind=n % len(KIND_NAMES), valid=n % 4 != 0, border=300.5 if n % 5 == 0 else 128.0))
                n += 1
    return res


CASES = _cases()
CASE_IDS = ["%dx%d_from_%dx%d_%s_c%d_m%d_f%d_%s%s" % (*c["out"], *c["src"], c["typ"], c["c"], c["maps"], c["fpm"], KIND_NAMES[c["kind"]],
                                                      "_valid" if c["valid"] else "") for c in CASES]
assert {c["c"] for c in CASES} == {1, 3, 4} and {(c["maps"], c["fpm"]) for c in CASES} == {(1, 1), (1, 2), (3, 1), (3, 2)}
assert {c["kind"] for c in CASES} == set(range(len(KIND_NAMES))) and {c["valid"] for c in CASES} == {True, False}


def pixels_of(seed, shape, typ):
    rng = np.random.default_rng([20, *seed])
    if typ == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(0.0, 255.0, shape).astype(np.float32)


# 2 ---- restatement = reference (no device) ---------------------------------------------------------------------------------------
def restatement_case(golden_dir):
    g = g20(golden_dir)
    tags = [str(t) for t in g["tags"] if str(t)[0] == "p"]
    assert len(tags) >= 24
    narrow = kinds = 0
    for tag in tags:
        h, w, ratio, degree, rx, ry, size, kind = g[tag + "_cfg"].tolist()
        h, w, size, kind = int(h), int(w), int(size), int(kind)
        narrow += w < 64
        kinds |= 1 << kind
        k0, c0 = g[tag + "_kpt0"], g[tag + "_center0"]
        seen = k0[:, 2] == 1
        pre, canvas = A.resize_rotate(h, w, ratio, degree)
        assert list(canvas) == g[tag + "_canvas"].tolist(), tag                                   # the rotated canvas
        assert np.abs(A.apply(pre, k0[seen, :2]) - g[tag + "_k_rot"][seen, :2]).max() <= POINT_TOL, tag
        assert np.abs(A.apply(pre, c0) - g[tag + "_c_rot"]).max() <= POINT_TOL, tag
        off = A.crop_offsets(A.apply(pre, c0), size, (rx, ry), 5)
        assert list(off) == g[tag + "_off"].tolist(), tag                                         # exactly
        dataset, flip = {2: "BBC", 3: "NTID"}.get(kind, "LSP"), kind != 0
        fwd, inv = A.compose(h, w, ratio, degree, off[0], off[1], size, flip)
        assert np.abs(np.vstack([fwd, [0, 0, 1]]) @ np.vstack([inv, [0, 0, 1]]) - np.eye(3)).max() < 1e-9, tag
        mine = np.where(seen[:, None], k0[:, :2], -1.0)                                            # this project's invisible mark
        k2, c2 = A.transform_points(mine, c0, fwd, flip, dataset)
        want = g[tag + "_k_out"]
        vis = want[:, 2] == 1                                                                     # after the reference's row swaps
        assert np.abs(k2[vis] - want[vis, :2]).max() <= POINT_TOL, tag
        assert np.array_equal(k2[~vis], np.full((int((~vis).sum()), 2), -1.0)), tag               # kept, and swapped like the rows
        assert np.abs(c2 - g[tag + "_c_out"]).max() <= POINT_TOL, tag
        # the Augmenter with explicit draws says the same
        aug = A.Augmenter(dataset, crop=size, center_perturb_max=5, flip_prob=0.5)
        params = {"ratio": [ratio], "degree": [degree], "perturb": [(rx, ry)], "flip": [flip]}
        inv_a, k_a, c_a, fwd_a, _ = aug((h, w), mine[None], c0[None], params=params)
        assert np.array_equal(inv_a[0], inv) and np.array_equal(fwd_a[0], fwd) and np.array_equal(k_a[0], k2) and np.array_equal(c_a[0], c2)
    assert narrow >= 3 and kinds == 15                    # sources narrower than 64; no flip, hflip, hflip_BBC and hflip_NTID
    for bad in ("MPII", "Penn_Action"):
        try:
            A.transform_points(np.zeros((16, 2)), (0, 0), np.eye(3)[:2], True, bad)
            raise AssertionError("no table for " + bad)
        except ValueError:
            pass
        A.transform_points(np.zeros((16, 2)), (0, 0), np.eye(3)[:2], False, bad)
        try:
            A.Augmenter(bad)
            raise AssertionError("no table for " + bad)
        except ValueError:
            pass


# 3 ---- entry = the reference's crop / hflip / normalize, bit for bit ------------------------------------------------------------
def golden_case(dev, golden_dir, alloc=None):
    g = g20(golden_dir)
    tags = [str(t) for t in g["tags"] if str(t)[0] == "i"]
    assert len(tags) >= 10
    for tag in tags:
        left, up, size, flip = g[tag + "_cfg"].tolist()
        src = g[tag + "_src"]
        h, w, _ = src.shape
        fwd, inv = A.compose(h, w, 1.0, 0.0, left, up, size, bool(flip))
        assert np.array_equal(inv, np.round(inv)) and abs(inv[0, 0]) == 1 and inv[1, 1] == 1          # a translation, maybe mirrored
        want = torch.from_numpy(g[tag + "_out"])[None]
        for s in (src[None], src[None].astype(np.float32)):
            got = entry(dev, s, inv[None], (size, size), alloc=alloc)
            assert torch.equal(bits(got), bits(want)), (tag, s.dtype)
        op = ops.augment_image(torch.from_numpy(src[None]).to(dev), inv[None], (size, size))
        assert op.dtype == F32 and torch.equal(bits(op.cpu()), bits(want)), tag


# 4 ---- identity = up_normalize_image --------------------------------------------------------------------------------------------
def identity_case(dev, alloc=None):
    ident = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    for (b, h, w, c) in ((1, 1, 1, 1), (2, 20, 12, 3), (3, 5, 65, 4)):
        for typ in ("u8", "f32"):
            src = pixels_of((4, b, h, w, c), (b, h, w, c), typ)
            want = ops.normalize_image(torch.from_numpy(src.astype(np.float32)).to(dev)).cpu()
            got = entry(dev, src, np.repeat(ident, b, axis=0), (h, w), alloc=alloc)
            assert torch.equal(bits(got), bits(want)), (b, h, w, c, typ)
            if b > 1:                                                                              # one shared map
                assert torch.equal(bits(entry(dev, src, ident, (h, w), fpm=b)), bits(want)), (b, h, w, c, typ)
    src = pixels_of((5,), (2, 6, 9, 3), "f32")                                                     # other constants
    want = ops.normalize_image(torch.from_numpy(src).to(dev), mean=104.5, std=57.375).cpu()
    assert torch.equal(bits(entry(dev, src, ident, (6, 9), border=0.0, mean=104.5, std=57.375, fpm=2)), bits(want))


# 5 ---- entry = float64 restatement ----------------------------------------------------------------------------------------------
def float64_case(dev, case, alloc=None):
    out, (hs, ws), c, fpm = case["out"], case["src"], case["c"], case["fpm"]
    b = case["maps"] * fpm
    src = pixels_of((5, *out, hs, ws, c, b), (b, hs, ws, c), case["typ"])
    inv = np.stack([KINDS[KIND_NAMES[(case["kind"] + i) % len(KIND_NAMES)]]((hs, ws), out) for i in range(case["maps"])])
    valid = [(max(hs - i, 1), max(ws - 2 * i, 1)) for i in range(b)] if case["valid"] else None
    ref, slack = restate(src, inv, out, border=case["border"], valid=valid, fpm=fpm)
    got = entry(dev, src, inv, out, border=case["border"], valid=valid, fpm=fpm, alloc=alloc)
    assert not bool((got == SENT).any())
    compare(got, ref, slack, "case", border=case["border"])
    touched = float(np.abs(ref - (case["border"] - 128.0) / 256.0).max())
    return touched


def coverage_case(dev):
    """the maps of CASES are no empty exercise: most cases sample the source somewhere"""
    hit = sum(float64_case(dev, c) > 0 for c in CASES[::3])
    assert hit >= len(CASES[::3]) * 3 // 4, hit


def outside_case(dev, alloc=None):
    """every tap outside: the whole output is the normalised border; coordinates of 1e12 index nothing"""
    for typ in ("u8", "f32"):
        src = pixels_of((6,), (3, 12, 20, 3), typ)
        maps = np.array([[[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0]],                   # far outside
                         [[1.0, 0.0, 1e12], [0.0, 1.0, -1e12]],                      # a translation no int32 / int64 index survives
                         [[1e12, 0.0, 0.0], [0.0, 1e12, 0.0]]])                      # only output pixel (0, 0) meets the source
        for border in (128.0, 17.0):
            got = entry(dev, src, maps, (5, 7), border=border, alloc=alloc)
            flat = torch.tensor((np.float32(border) - np.float32(128.0)) / np.float32(256.0))
            assert bool((got[:2] == flat).all()), (typ, border)
            want = torch.full((3, 5, 7), float(flat))
            want[:, 0, 0] = torch.from_numpy((src[2, 0, 0].astype(np.float32) - np.float32(128.0)) / np.float32(256.0))
            assert torch.equal(bits(got[2]), bits(want)), (typ, border)
            ref, slack = restate(src, maps, (5, 7), border=border)
            compare(got, ref, slack, "outside", border=border)
        edge = np.array([[[1.0, 0.0, -1.0], [0.0, 1.0, 11.0]]])                      # x0 = -1 .. 20, y0 = the last row and the one after
        got = entry(dev, src[:1], edge, (2, 22), alloc=alloc)
        ref, slack = restate(src[:1], edge, (2, 22))
        compare(got, ref, slack, "edge")
        assert bool((got[:, :, 1] == 0.0).all()) and bool((got[:, :, 0, 0] == 0.0).all()) and float(got[:, :, 0, 1:21].abs().max()) > 0
        for bad in (float("nan"), float("inf")):                                    # past ops' refusal: still nothing is read
            m = np.array([[[1.0, 0.0, bad], [0.0, 1.0, 0.0]]])
            assert bool((entry(dev, src[:1], m, (3, 4), alloc=alloc) == 0.0).all())


# 6 ---- the padding is never read ----------------------------------------------------------------------------------------------------
def padding_case(dev, alloc=None):
    valid = [(20, 12), (7, 9), (1, 1)]
    hs, ws, c, out = 20, 12, 3, (9, 14)
    inv = np.stack([centred(v, out, 1.0, 37.0, False) for v in valid[:2]] + [np.array([[0.25, 0.0, -0.5], [0.0, 0.25, -0.5]])])
    for typ, fill in (("f32", float("nan")), ("u8", 255)):
        buf = np.full((3, hs, ws, c), fill, dtype=np.float32 if typ == "f32" else np.uint8)
        alone = []
        for i, (h, w) in enumerate(valid):
            img = pixels_of((7, i), (h, w, c), typ)
            if typ == "u8":
                img = img // 2                                                      # never 255: a padding pixel read would show
            buf[i, :h, :w] = img
            alone.append(entry(dev, img[None], inv[i:i + 1], out, alloc=alloc)[0])  # stored unpadded (and right before a guard page)
        got = entry(dev, buf, inv, out, valid=valid, alloc=alloc)
        assert bool(torch.isfinite(got).all()), typ
        for i in range(3):
            assert torch.equal(bits(got[i]), bits(alone[i])), (typ, i)
        assert float(got[2].abs().max()) > 0                                        # the 1 x 1 sample is sampled
        op = ops.augment_image(torch.from_numpy(buf).to(dev), inv, out, valid_hw=valid)
        assert torch.equal(bits(op.cpu()), bits(got)), typ
        if typ == "u8":                                                             # an extent beyond the buffer is cut to it
            wide = entry(dev, buf[:1], inv[:1], out, valid=[(1000, 1000)], alloc=alloc)
            assert torch.equal(bits(wide[0]), bits(alone[0]))
            none = entry(dev, buf[:1], inv[:1], out, valid=[(-3, 5)], alloc=alloc)
            assert bool((none == 0.0).all())


# 7 ---- the points follow the pixels ----------------------------------------------------------------------------------------------
def follow_case(dev):
    h, w, size = 60, 80, 64
    rng = np.random.default_rng(27)
    gx, gy = np.meshgrid(np.arange(10, 80, 16), np.arange(8, 56, 16))                # 5 x 3 cells of 16: blobs cannot meet
    spots = np.stack([gx.ravel(), gy.ravel()], axis=1)[rng.permutation(15)[:14]] + rng.integers(-3, 4, (14, 2))
    kpt = spots.astype(np.float64)
    kpt[[4, 9]] = -1.0
    src = np.zeros((1, h, w, 1), dtype=np.float32)
    for x, y in spots[(kpt >= 0).all(axis=1)]:
        src[0, y - 1:y + 2, x - 1:x + 2, 0] = 128.0                                  # a bright 3 x 3 blob, brightest in the middle
        src[0, y, x, 0] = 255.0
    centre = np.array([w / 2.0 + 3.0, h / 2.0 - 2.0])
    checked = 0
    for ratio, degree, flip in ((0.9, 25.0, True), (1.1, -25.0, False), (0.75, 25.0, False)):
        pre, _ = A.resize_rotate(h, w, ratio, degree)
        left, up = A.crop_offsets(A.apply(pre, centre), size, (0.9, 0.2))
        fwd, inv = A.compose(h, w, ratio, degree, left, up, size, flip)
        k2, _ = A.transform_points(kpt, centre, fwd, flip, "LSP")
        img = entry(dev, src, inv[None], (size, size), border=0.0, mean=0.0, std=1.0)[0, 0].numpy()
        assert img.max() > 100
        for x, y in k2[(k2 >= 0).all(axis=1)]:
            if not (2 <= x <= size - 3 and 2 <= y <= size - 3):
                continue
            x0, y0 = max(int(round(x)) - 3, 0), max(int(round(y)) - 3, 0)
            win = img[y0:int(round(y)) + 4, x0:int(round(x)) + 4]
            py, px = np.unravel_index(int(win.argmax()), win.shape)
            assert win.max() > 60 and max(abs(px + x0 - x), abs(py + y0 - y)) <= 1.0, (ratio, degree, flip, x, y, px + x0, py + y0)
            checked += 1
    assert checked >= 12, checked


# 8 ---- refusals ------------------------------------------------------------------------------------------------------------------
def refusal_case(dev):
    L = _C.lib()
    src = torch.zeros(4, 6, 5, 3, dtype=torch.uint8).to(dev)
    inv = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 4, dtype=torch.float64).to(dev)
    out = torch.full((4 * 3 * 8 * 8,), SENT, dtype=F32).to(dev)
    names = ("src", "typ", "B", "Hs", "Ws", "C", "valid", "inv", "fpm", "border", "mean", "std", "out", "Ho", "Wo", "stream")
    ok = (src.data_ptr(), U8, 4, 6, 5, 3, None, inv.data_ptr(), 1, 128.0, 128.0, 256.0, out.data_ptr(), 8, 8, ops._stream(out))

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_augment_image(*[a[n] for n in names])

    for bad in (dict(src=None), dict(inv=None), dict(out=None), dict(B=0), dict(B=-4), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-8),
                dict(C=0), dict(C=5), dict(C=-1), dict(fpm=0), dict(fpm=-1), dict(fpm=3), dict(fpm=8), dict(std=0.0), dict(std=-256.0),
                dict(std=float("nan")), dict(typ=2), dict(typ=-1)):
        assert call(**bad) == -1, bad
        assert L.up_last_error().startswith(b"augment_image:"), (bad, L.up_last_error())
    assert bool((out.cpu() == SENT).all())                                            # nothing was launched
    assert call() == 0 and call(fpm=2) == 0 and call(fpm=4) == 0
    assert not bool((out.cpu() == SENT).any())
    px = torch.zeros(2, 6, 5, 3, dtype=torch.uint8).to(dev)
    ident = np.array([[[1.0, 0, 0], [0, 1.0, 0]]] * 2)
    for bad in (float("nan"), float("inf"), -float("inf")):
        m = ident.copy()
        m[1, 0, 2] = bad
        for maps in (m, m.tolist(), torch.from_numpy(m)):
            try:
                ops.augment_image(px, maps, (4, 4))
                raise AssertionError("ValueError expected")
            except ValueError:
                pass
    for kw in (dict(inv=ident[:1]), dict(inv=ident, frames_per_map=2), dict(inv=ident, frames_per_map=0),
               dict(inv=ident, valid_hw=[(6, 5)])):
        try:
            ops.augment_image(px, kw.pop("inv"), (4, 4), **kw)
            raise AssertionError("ValueError expected")
        except ValueError:
            pass
    for dt in (torch.int32, torch.float64):
        try:
            ops.augment_image(px.to(dt), ident, (4, 4))
            raise AssertionError("TypeError expected")
        except TypeError:
            pass
    try:
        ops.augment_image(px, ident, (4, 0))
        raise AssertionError("an empty output is refused by the entry")
    except _C.UniPoseHipError:
        pass
    from unipose_amd.trainer import DeviceBatcher
    z = torch.zeros(1, 3, 8, 8)
    try:
        DeviceBatcher(dev, 8, 3, augment=A.Augmenter("LSP", crop=8))((z, z, z, ["a"]))
        raise AssertionError("a rendered tuple cannot be augmented")
    except ValueError:
        pass


# 9 ---- batcher and trainer -------------------------------------------------------------------------------------------------------
def _peaks_ok(heat, k2, size, stride):
    """every joint that lies in the image: its map's largest value is in the cell int(coordinate) / stride (to half a cell: the
    centre of the Gaussian is a fraction)"""
    n = 0
    heat = heat.cpu().numpy()
    for b in range(k2.shape[0]):
        for j, (x, y) in enumerate(k2[b]):
            if not (0 <= x < size and 0 <= y < size):
                continue
            m = heat[b, j + 1]
            row, col = np.unravel_index(int(m.argmax()), m.shape)
            cx, cy = min(int(x) / stride, m.shape[1] - 1), min(int(y) / stride, m.shape[0] - 1)
            assert m.max() > 0 and abs(col - cx) <= 0.5 and abs(row - cy) <= 0.5, (b, j, x, y, row, col)
            n += 1
    return n


def batcher_case(dev, bbox):
    from unipose_amd.trainer import DeviceBatcher, SyntheticPoseData
    size, crop = 48, 32
    item = next(iter(SyntheticPoseData(14, 2, 1, size=size, seed=1)))
    assert item["pixels"].dtype == torch.uint8
    seen = []
    real = ops.augment_image

    def spy(pixels, *a, **kw):
        seen.append(pixels.dtype)
        return real(pixels, *a, **kw)

    ops.augment_image = spy
    try:
        out = DeviceBatcher(dev, 8, 3, bbox=bbox, augment=A.Augmenter("LSP", crop=crop, seed=5))(item)
    finally:
        ops.augment_image = real
    assert seen == [torch.uint8]                                                      # no .float() pass over the pixels
    assert len(out) == (4 if bbox else 3)
    assert tuple(out[0].shape) == (2, 3, crop, crop) and tuple(out[1].shape) == (2, 15, 4, 4) and tuple(out[2].shape) == (2, 1, crop, crop)
    inv, k2, c2, _, params = A.Augmenter("LSP", crop=crop, seed=5)((size, size), item["kpts"], item["center"])
    assert torch.equal(out[0], ops.augment_image(item["pixels"].to(dev), inv, (crop, crop)))
    assert torch.equal(out[1], ops.make_heatmaps(k2, crop, crop, 8, 3.0, dev)) and torch.equal(out[2], ops.make_centermaps(c2, crop, crop, 3.0, dev))
    assert _peaks_ok(out[1], k2, crop, 8) >= 4
    if bbox:
        assert tuple(out[3].shape) == (2, 5, 4, 4) and torch.equal(out[3], ops.make_box_maps(k2, crop, crop, 8, dev))
    again = DeviceBatcher(dev, 8, 3, bbox=bbox, augment=A.Augmenter("LSP", crop=crop, seed=5))(item)
    other = DeviceBatcher(dev, 8, 3, bbox=bbox, augment=A.Augmenter("LSP", crop=crop, seed=6))(item)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert not torch.equal(out[0], other[0]) and not torch.equal(out[1], other[1])
    plain = DeviceBatcher(dev, 8, 3, bbox=bbox)(item)                                 # without the option: as before
    assert tuple(plain[0].shape) == (2, 3, size, size)
    assert torch.equal(plain[0], ops.normalize_image(item["pixels"].to(dev).float()))
    # images of different sizes padded into one buffer: the extents reach the kernel
    item2 = dict(item, valid_hw=np.array([[48, 48], [30, 40]]))
    pad = DeviceBatcher(dev, 8, 3, augment=A.Augmenter("LSP", crop=crop, seed=5))(item2)
    inv2 = A.Augmenter("LSP", crop=crop, seed=5)(item2["valid_hw"], item["kpts"], item["center"])[0]
    assert torch.equal(pad[0], ops.augment_image(item["pixels"].to(dev), inv2, (crop, crop), valid_hw=item2["valid_hw"]))


def clip_case(dev):
    from unipose_amd.trainer import DeviceBatcher, SyntheticPoseData
    size, crop, t = 48, 32, 3
    item = next(iter(SyntheticPoseData(13, 2, 1, size=size, frames=t, seed=2)))
    item["pixels"][:, 1] = item["pixels"][:, 0]                                       # two equal frames: one map per clip shows
    aug = A.Augmenter("Penn_Action", crop=crop, flip_prob=0.0, seed=9)
    x, heat, cm = DeviceBatcher(dev, 8, 1, augment=aug)(item)
    assert tuple(x.shape) == (2, t, 3, crop, crop) and tuple(heat.shape) == (2, t, 14, 4, 4) and tuple(cm.shape) == (2, t, 1, crop, crop)
    assert torch.equal(x[:, 0], x[:, 1]) and not torch.equal(x[:, 0], x[:, 2]) and not torch.equal(x[0, 0], x[1, 0])
    inv, k2, c2, fwd, _ = A.Augmenter("Penn_Action", crop=crop, flip_prob=0.0, seed=9)((size, size), item["kpts"], item["center"])
    assert inv.shape == (2, 2, 3) and k2.shape == (2, t, 13, 2)
    assert torch.equal(x.reshape(2 * t, 3, crop, crop),
                       ops.augment_image(item["pixels"].reshape(2 * t, size, size, 3).to(dev), inv, (crop, crop), frames_per_map=t))
    assert torch.equal(heat.reshape(2 * t, 14, 4, 4), ops.make_heatmaps(k2.reshape(2 * t, 13, 2), crop, crop, 8, 1.0, dev))
    assert _peaks_ok(heat.reshape(2 * t, 14, 4, 4), k2.reshape(2 * t, 13, 2), crop, 8) >= 6
    vis = (np.asarray(item["kpts"]) >= 0).all(axis=-1)
    for i in range(2):                                                                # every frame of a clip through the clip's map
        assert np.allclose(k2[i][vis[i]], A.apply(fwd[i], np.asarray(item["kpts"])[i][vis[i]]), atol=1e-9)


def trainer_case(dev):
    import argparse
    from unipose_amd.trainer import Trainer
    args = argparse.Namespace(dataset="LSP", pretrained=None, model_name=None, model_arch="unipose", train_dir=None, val_dir=None,
                              batch_size=2, size=32, train_batches=1, val_batches=1, augment=True)
    tr = Trainer(args, device=dev)
    assert tr.train_batcher is not tr.batcher and tr.train_batcher.augment is not None and tr.batcher.augment is None
    assert tr.train_batcher.augment.crop == (32, 32)
    loss = tr.training(0)
    assert np.isfinite(loss) and tr.iters == 1
    plain = Trainer(argparse.Namespace(**{**vars(args), "augment": False}), device=dev)
    assert plain.train_batcher is plain.batcher and plain.batcher.augment is None
    plain.model.load_state_dict(tr.model.state_dict())
    a, b = tr.validation(0), plain.validation(0)
    assert a.evals == b.evals == 1
    for name in ("AP", "PCK", "PCKh", "count"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    from unipose_amd.trainer import _augmenter
    assert _augmenter(argparse.Namespace(), "LSP", 32) is None                        # the option defaults to off
    assert _augmenter(args, "MPII", 32).flip_prob == 0.0 and _augmenter(args, "LSP", 32).flip_prob == 0.5
    import unipose as image_driver
    import uniposeLSTM as video_driver
    for drv in (image_driver, video_driver):
        assert drv.parse_args([]).augment is False and drv.parse_args(["--augment"]).augment is True


# GPU only ---- more than 2^21 output pixels in one launch ------------------------------------------------------------------------
def big_case(dev):
    b, hs, ws, crop = BIG
    assert b * crop * crop > 2 ** 21
    src = pixels_of((8,), (b, hs, ws, 3), "u8")
    rng = np.random.default_rng(28)
    kpt = np.stack([rng.uniform(0, ws, (b, 14)), rng.uniform(0, hs, (b, 14))], axis=2)
    centre = np.stack([ws / 2 + rng.uniform(-8, 8, b), hs / 2 + rng.uniform(-8, 8, b)], axis=1)
    inv = A.Augmenter("LSP", crop=crop, seed=3)((hs, ws), kpt, centre)[0]
    got = ops.augment_image(torch.from_numpy(src).to(dev), inv, (crop, crop)).cpu()
    ref, slack = restate(src, inv, (crop, crop))
    compare(got, ref, slack, "big")
    assert float(np.abs(ref[-1]).max()) > 0.2                                         # the last sample (second trip) shows pixels
