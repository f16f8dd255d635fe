"""Pose from source frames (up_crop_to_nhwc, up_unipose_frame_heatmaps, up_unipose_frame_final_preds; protocol.crop_maps,
ops.crop_to_nhwc, UniPosePlan.frame_heatmaps / frame_final_preds): shared by test_frame_emu.py and test_frame_gpu.py.

Yardsticks.  The fixture G22 (tools/make_goldens.py g22) holds what the reference's OWN utils/extra_utils/transforms.py computes:
get_transform, its inverse and the corners of crop's window, for three sizes, three rotations and both kinds of centre / scale.
Only the geometry is pinned to the reference: its crop resizes with scipy.misc.imresize, which SciPy has removed, so there are no
genuine pixels.  The pixel contract is this project's own: up_crop_to_nhwc must equal, bit for bit, the two calls it replaces —
up_augment_image (pinned element by element by test_augment_*) on frames[frame_of], then up_nchw_to_nhwc resp.
up_nchw_to_nhwc_flip.  Every comparison here is bit for bit or integer-exact; nothing has a tolerance."""
import ctypes as C
import os

import numpy as np
import torch

from unipose_amd import _C, ops, protocol

F32 = np.float32
SENT = 7.0
U8, PF32 = 0, 1                                     # UP_PIX_U8, UP_PIX_F32
FROM_FRAMES = 256                                   # UP_PROGRAM_FROM_FRAMES
BIG_OUT = (1449, 1449)                              # 2 099 601 output pixels (> 2^21): a second grid trip


def g22(golden_dir):
    return np.load(os.path.join(golden_dir, "g22_crop_geometry.npz"))


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    """equal bits; NaNs must sit at the same places (their payload is not compared)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


# ---- 1. geometry against G22, no device --------------------------------------------------------------------------------------------
def geometry_case(golden_dir):
    g = g22(golden_dir)
    n = 0
    for r, res in enumerate(g["res"].tolist()):
        for k, rot in enumerate(g["rot"].tolist()):
            for kind, c, s in (("32", torch.from_numpy(g["c32"]), torch.from_numpy(g["s32"])), ("64", g["c64"], g["s64"])):
                m = protocol.crop_maps(c, s, res, rot)
                assert m.dtype == np.float64 and m.shape == (len(c), 6)
                want = np.ascontiguousarray(g["Ti" + kind][r, k][:, :2]).reshape(len(c), 6)
                assert np.array_equal(m.view(np.int64), want.view(np.int64)), (res, rot, kind)
                for i in range(len(c)):
                    t = np.vstack([m[i].reshape(2, 3), [0.0, 0.0, 1.0]])
                    # transform(pt, ..., invert=1): np.dot(inv, [pt0 - 1, pt1 - 1, 1])[:2].astype(int) + 1 at pt = [0, 0] and pt = res
                    ul = np.dot(t, np.array([-1.0, -1.0, 1.0]))[:2].astype(int) + 1
                    br = np.dot(t, np.array([res[0] - 1.0, res[1] - 1.0, 1.0]))[:2].astype(int) + 1
                    assert np.array_equal(ul, g["ul" + kind][r, k, i]) and np.array_equal(br, g["br" + kind][r, k, i]), (res, rot, kind, i)
                    n += 1
    assert n == 3 * 3 * 2 * 4
    # one rotation per sample, and a list like an array
    per = protocol.crop_maps(g["c64"], g["s64"], [52, 68], [0, 30, -45, 30])
    for i, rot in enumerate((0, 30, -45, 30)):
        assert np.array_equal(per[i], protocol.crop_maps(g["c64"][i:i + 1].tolist(), g["s64"][i:i + 1].tolist(), [52, 68], rot)[0])
    # the crop that is the whole square image: the identity, bit for bit
    for size in (64, 368, 50):
        m = protocol.crop_maps([[size / 2, size / 2]], [size / 200], [size, size])
        assert np.array_equal(m.view(np.int64), np.array([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]]).view(np.int64)), size


# ---- 2. the kernel and the two calls it replaces -----------------------------------------------------------------------------------
def pixels_of(seed, shape, typ):
    rng = np.random.default_rng([22, *seed])
    if typ == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(0.0, 255.0, shape).astype(np.float32)


def _place(arr, dev, alloc):
    """a numpy array as a tensor on `dev`; with alloc (the emulator's guarded allocation) it ends right in front of a guard page"""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if alloc is not None:
        g = alloc(tuple(t.shape), t.dtype)
        g.copy_(t)
        t = g
    return t.to(dev)


def _sentinel(shape, dev, alloc):
    if alloc is not None:
        return alloc(shape, torch.float32, SENT).to(dev)
    return torch.full(shape, SENT, dtype=torch.float32, device=dev)


def run_crop(dev, frames, inv, out_hw, frame_of=None, valid=None, ld=4, which="both", alloc=None, border=128.0, mean=128.0, std=256.0):
    """up_crop_to_nhwc itself on sentinel-filled outputs -> (y, y_flip) numpy (B,Ho,Wo,ld), None for an output not asked for"""
    s = _place(frames, dev, alloc)
    nf, hs, ws, c = s.shape
    m = torch.from_numpy(np.ascontiguousarray(inv, dtype=np.float64).reshape(-1, 6)).to(dev)
    b = m.shape[0]
    fo = None if frame_of is None else torch.tensor(np.asarray(frame_of), dtype=torch.int32).to(dev)
    vt = None if valid is None else torch.tensor(np.asarray(valid), dtype=torch.int32).to(dev)
    shape = (b, out_hw[0], out_hw[1], ld)
    y = _sentinel(shape, dev, alloc) if which in ("both", "y") else None
    yf = _sentinel(shape, dev, alloc) if which in ("both", "flip") else None
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    _C.check(_C.lib().up_crop_to_nhwc(s.data_ptr(), U8 if s.dtype == torch.uint8 else PF32, nf, hs, ws, c, ptr(fo), ptr(vt), m.data_ptr(), b,
                                      border, mean, std, ptr(y), ptr(yf), out_hw[0], out_hw[1], ld, ops._stream(s)), "crop_to_nhwc")
    return None if y is None else host(y), None if yf is None else host(yf)


def composition(dev, frames, inv, out_hw, frame_of=None, valid=None, ld=4, border=128.0, mean=128.0, std=256.0):
    """what the entry replaces: up_augment_image on frames[frame_of] with valid[frame_of], then up_nchw_to_nhwc / _flip -> (y, y_flip)"""
    L = _C.lib()
    inv = np.ascontiguousarray(inv, dtype=np.float64).reshape(-1, 6)
    b = inv.shape[0]
    fo = np.arange(b) if frame_of is None else np.asarray(frame_of)
    s = torch.from_numpy(np.ascontiguousarray(np.asarray(frames)[fo])).to(dev)          # the replicated source the entry does without
    _, hs, ws, c = s.shape
    m = torch.from_numpy(inv).to(dev)
    vt = None if valid is None else torch.tensor(np.asarray(valid)[fo], dtype=torch.int32).to(dev)
    ho, wo = out_hw
    x = torch.full((b, c, ho, wo), SENT, dtype=torch.float32, device=dev)
    _C.check(L.up_augment_image(s.data_ptr(), U8 if s.dtype == torch.uint8 else PF32, b, hs, ws, c, None if vt is None else vt.data_ptr(),
                                m.data_ptr(), 1, border, mean, std, x.data_ptr(), ho, wo, ops._stream(x)), "augment_image")
    y = torch.full((b, ho, wo, ld), SENT, dtype=torch.float32, device=dev)
    yf = torch.full((b, ho, wo, ld), SENT, dtype=torch.float32, device=dev)
    _C.check(L.up_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), b, c, ho, wo, ld, ops._stream(x)), "nchw_to_nhwc")
    _C.check(L.up_nchw_to_nhwc_flip(x.data_ptr(), yf.data_ptr(), b, c, ho, wo, ld, ops._stream(x)), "nchw_to_nhwc_flip")
    return host(y), host(yf)


def same_pair(got, ref, c, what):
    for g, r, n in zip(got, ref, ("y", "y_flip")):
        if g is None:
            continue
        assert not (g == SENT).any(), (what, n, "an element was not written")
        assert (g[..., c:] == 0.0).all() and not np.signbit(g[..., c:]).any(), (what, n, "a pad lane is not +0")
        assert bits_equal(g, r), (what, n, g.reshape(-1)[:8], r.reshape(-1)[:8])
    if got[0] is not None and got[1] is not None:
        assert bits_equal(got[1], got[0][:, :, ::-1]), (what, "y_flip is not the mirror of y")


def rotation(src_hw, out_hw, scale=0.37, degree=30.0):
    """output -> source: a rotation by `degree` and a zoom by `scale` about the two centres"""
    a = np.deg2rad(degree)
    cs, sn = np.cos(a) / scale, np.sin(a) / scale
    cx, cy, ox, oy = (src_hw[1] - 1) / 2, (src_hw[0] - 1) / 2, (out_hw[1] - 1) / 2, (out_hw[0] - 1) / 2
    return [cs, -sn, cx - cs * ox + sn * oy, sn, cs, cy - sn * ox - cs * oy]


def maps_for(src_hw, out_hw):
    """one sample per kind: the identity, an integer translation, scale 0.37 with a 30 degree rotation (and the zoom the other way),
    entirely outside, coefficients of 1e12 (a translation and a scale), NaN coefficients"""
    nan = float("nan")
    return np.array([[1.0, 0, 0, 0, 1, 0], [1.0, 0, 2, 0, 1, -1], rotation(src_hw, out_hw), rotation(src_hw, out_hw, 1 / 0.37, -30.0),
                     [1.0, 0, 1000, 0, 1, 1000], [1.0, 0, 1e12, 0, 1, -1e12], [1e12, 0, 0, 0, 1e12, 0], [nan, 0, 0, 0, 1, 0],
                     [1.0, 0, 0, nan, nan, nan]])


SRCS = [(1, 1), (5, 7), (20, 12)]
OUTS = [(1, 1), (3, 5), (33, 65)]                   # Wo odd: the mirror has a centre column; 33 x 65 = 9 blocks per sample
LAYOUTS = [(1, 4), (3, 4), (4, 4), (1, 8), (3, 8), (4, 8)]
WHICH = ["both", "y", "flip"]


def _cases():
    res, n = [], 0
    for typ in ("u8", "f32"):
        for src in SRCS:
            for out in OUTS:
                res.append(dict(typ=typ, src=src, out=out, layout=LAYOUTS[n % 6], which=WHICH[(n // 6) % 3]))
                n += 1
    return res


CASES = _cases()
CASE_IDS = ["%s_%dx%d_to_%dx%d_c%d_ld%d_%s" % (c["typ"], *c["src"], *c["out"], *c["layout"], c["which"]) for c in CASES]
assert len({(c["layout"], c["which"]) for c in CASES}) == 18


def kernel_case(dev, case, alloc=None):
    """nine samples, one per map kind, alternating between two frames"""
    (hs, ws), out, (c, ld) = case["src"], case["out"], case["layout"]
    frames = pixels_of((1, hs, ws, c, *out), (2, hs, ws, c), case["typ"])
    inv = maps_for((hs, ws), out)
    fo = [i % 2 for i in range(len(inv))]
    ref = composition(dev, frames, inv, out, fo, ld=ld)
    got = run_crop(dev, frames, inv, out, fo, ld=ld, which=case["which"], alloc=alloc)
    assert (got[0] is None) == (case["which"] == "flip") and (got[1] is None) == (case["which"] == "y")
    same_pair(got, ref, c, case)
    flat = (F32(128.0) - F32(128.0)) / F32(256.0)
    for g in got:
        if g is not None:                           # outside, the 1e12 translation and both NaN maps: nothing but the border
            assert (g[[4, 5, 7, 8]][..., :c] == flat).all(), case
    if (hs, ws) != (1, 1) and out != (1, 1):
        g = got[0] if got[0] is not None else got[1]
        assert np.abs(g[2]).max() > 0 and np.abs(g[3]).max() > 0, "the rotated maps sample the source"


def identity_case(dev, alloc=None):
    """the identity map: up_normalize_image through the layout pass, bit for bit; frame_of == NULL with F == B == 2"""
    L = _C.lib()
    ident = np.array([[1.0, 0, 0, 0, 1, 0]] * 2)
    for (h, w, c, ld) in ((1, 1, 1, 4), (20, 12, 3, 4), (5, 65, 4, 8)):
        for typ in ("u8", "f32"):
            frames = pixels_of((2, h, w, c), (2, h, w, c), typ)
            x = ops.normalize_image(torch.from_numpy(frames.astype(np.float32)).to(dev))
            want = torch.full((2, h, w, ld), SENT, dtype=torch.float32, device=dev)
            wantf = torch.full((2, h, w, ld), SENT, dtype=torch.float32, device=dev)
            _C.check(L.up_nchw_to_nhwc(x.data_ptr(), want.data_ptr(), 2, c, h, w, ld, ops._stream(x)), "nchw_to_nhwc")
            _C.check(L.up_nchw_to_nhwc_flip(x.data_ptr(), wantf.data_ptr(), 2, c, h, w, ld, ops._stream(x)), "nchw_to_nhwc_flip")
            same_pair(run_crop(dev, frames, ident, (h, w), ld=ld, alloc=alloc), (host(want), host(wantf)), c, (h, w, c, ld, typ))
    frames = pixels_of((3,), (2, 6, 9, 3), "f32")                                    # other constants
    ref = composition(dev, frames, ident, (6, 9), border=0.0, mean=104.5, std=57.375)
    same_pair(run_crop(dev, frames, ident, (6, 9), border=0.0, mean=104.5, std=57.375, alloc=alloc), ref, 3, "constants")


def frame_index_case(dev, alloc=None):
    out = (9, 14)
    for typ in ("u8", "f32"):
        three = pixels_of((4,), (3, 20, 12, 3), typ)
        maps = np.array([rotation((20, 12), out), rotation((20, 12), out, 0.8, -70.0), [1.0, 0, -3, 0, 1, 4]])
        # F = 1, B = 3: three persons of one frame, three maps
        got = run_crop(dev, three[:1], maps, out, [0, 0, 0], alloc=alloc)
        same_pair(got, composition(dev, three[:1], maps, out, [0, 0, 0]), 3, (typ, "F1B3"))
        assert not bits_equal(got[0][0], got[0][1]) and not bits_equal(got[0][1], got[0][2])
        # F = 3, B = 2, frame_of = [2, 0]
        got = run_crop(dev, three, maps[:2], out, [2, 0], alloc=alloc)
        same_pair(got, composition(dev, three, maps[:2], out, [2, 0]), 3, (typ, "F3B2"))
        alone = run_crop(dev, three[2:], maps[:1], out, alloc=alloc)                   # sample 0 is frame 2 under map 0
        assert bits_equal(got[0][0], alone[0][0])
        # frame_of == NULL with F = B = 2
        got = run_crop(dev, three[:2], maps[:2], out, alloc=alloc)
        same_pair(got, composition(dev, three[:2], maps[:2], out), 3, (typ, "null"))
        # ops.crop_to_nhwc is the same entry
        t = torch.from_numpy(three).to(dev)
        y, yf = ops.crop_to_nhwc(t, maps[:2].reshape(2, 2, 3), out, frame_of=[2, 0], flip=True)
        ref = composition(dev, three, maps[:2], out, [2, 0])
        assert bits_equal(host(y), ref[0]) and bits_equal(host(yf), ref[1])
        y8 = ops.crop_to_nhwc(t[:2], maps[:2], out, ld=8)
        assert tuple(y8.shape) == (2, 9, 14, 8) and bits_equal(host(y8), composition(dev, three[:2], maps[:2], out, ld=8)[0])


def valid_case(dev, alloc=None):
    """valid_hw is per source FRAME; what lies beyond it (NaN resp. 255) is never read"""
    valid = [(20, 12), (7, 9), (1, 1)]
    hs, ws, c, out = 20, 12, 3, (9, 14)
    inv = np.stack([rotation(v, out, 0.6, 37.0) for v in valid[:2]] + [np.array([0.25, 0.0, -0.5, 0.0, 0.25, -0.5])])
    fo = [1, 2, 0, 1]                                                                  # two persons in the 7 x 9 frame
    maps = inv[[1, 2, 0, 0]]
    for typ, fill in (("f32", float("nan")), ("u8", 255)):
        buf = np.full((3, hs, ws, c), fill, dtype=np.float32 if typ == "f32" else np.uint8)
        imgs = []
        for i, (h, w) in enumerate(valid):
            img = pixels_of((5, i), (h, w, c), typ)
            if typ == "u8":
                img = img // 2                                                          # never 255: a padding pixel read would show
            buf[i, :h, :w] = img
            imgs.append(img)
        got = run_crop(dev, buf, maps, out, fo, valid=valid, alloc=alloc)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), typ
        same_pair(got, composition(dev, buf, maps, out, fo, valid=valid), c, (typ, "valid"))
        for b, f in enumerate(fo):                 # each frame stored unpadded (and right before a guard page), its sample alone
            alone = run_crop(dev, imgs[f][None], maps[b:b + 1], out, alloc=alloc)
            assert bits_equal(got[0][b], alone[0][0]) and bits_equal(got[1][b], alone[1][0]), (typ, b)
        assert np.abs(got[0][1]).max() > 0                                              # the 1 x 1 frame is sampled
        wide = run_crop(dev, buf, maps, out, fo, valid=[(1000, 1000), (7, 9), (1, 1)], which="y", alloc=alloc)
        cut = run_crop(dev, buf, maps, out, fo, valid=[(20, 12), (7, 9), (1, 1)], which="y", alloc=alloc)
        assert bits_equal(wide[0], cut[0])                                              # an extent beyond the buffer is cut to it
        none = run_crop(dev, buf, maps, out, fo, valid=[(20, 12), (-3, 5), (1, 1)], which="y", alloc=alloc)
        assert (none[0][[0, 3]][..., :c] == 0.0).all() and bits_equal(none[0][[1, 2]], got[0][[1, 2]])


def bad_frame_case(dev, alloc=None):
    """frame_of outside 0 .. F-1: that sample is all border, nothing is loaded for it, the other samples do not notice"""
    out = (9, 14)
    for typ in ("u8", "f32"):
        frames = pixels_of((6,), (2, 20, 12, 3), typ)
        maps = np.array([rotation((20, 12), out), [1.0, 0, 0, 0, 1, 0], rotation((20, 12), out, 0.8, -70.0), [1.0, 0, -3, 0, 1, 4]])
        good = composition(dev, frames, maps[[1, 3]], out, [1, 0])
        for fo in ([-1, 1, 2, 0], [-(2 ** 31), 1, 2 ** 31 - 1, 0], [2, 1, -7, 0]):
            for border in (128.0, 17.0):
                got = run_crop(dev, frames, maps, out, fo, border=border, alloc=alloc)
                flat = (F32(border) - F32(128.0)) / F32(256.0)
                for g in got:
                    assert (g[[0, 2]][..., :3] == flat).all() and (g[[0, 2]][..., 3:] == 0.0).all(), (typ, fo, border)
                if border == 128.0:
                    assert bits_equal(got[0][[1, 3]], good[0]) and bits_equal(got[1][[1, 3]], good[1]), (typ, fo)
        got = run_crop(dev, frames, maps, out, [0, 1, 0, 1], valid=[(20, 12), (20, 12)], alloc=alloc)      # and with extents given
        bad = run_crop(dev, frames, maps, out, [0, 5, 0, -1], valid=[(20, 12), (20, 12)], alloc=alloc)
        assert bits_equal(bad[0][[0, 2]], got[0][[0, 2]]) and (bad[0][[1, 3]][..., :3] == 0.0).all()
        for bad_fo in ([0, 2], [-1, 0]):                                               # ops refuses host indices before any launch
            try:
                ops.crop_to_nhwc(torch.from_numpy(frames).to(dev), maps[:2], out, frame_of=bad_fo)
                raise AssertionError("ValueError expected")
            except ValueError:
                pass


def big_case(dev, alloc=None):
    """more than 2^21 output pixels in one launch: the grid walks them in a second trip"""
    assert BIG_OUT[0] * BIG_OUT[1] > 2 ** 21
    frames = pixels_of((7,), (1, 20, 12, 3), "u8")
    inv = np.array([rotation((20, 12), BIG_OUT, 100.0, 30.0)])
    ref = composition(dev, frames, inv, BIG_OUT, [0])
    got = run_crop(dev, frames, inv, BIG_OUT, [0], alloc=alloc)
    assert bits_equal(got[0], ref[0]) and bits_equal(got[1], ref[1])
    assert (got[0][..., 3] == 0.0).all() and np.abs(got[0][0, -1]).max() > 0 and np.abs(got[0][0, 0]).max() > 0     # both trips show pixels


def refusal_case(dev):
    L = _C.lib()
    src = torch.zeros(2, 6, 5, 3, dtype=torch.uint8).to(dev)
    inv = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 2, dtype=torch.float64).to(dev)
    fo = torch.tensor([0, 1], dtype=torch.int32).to(dev)
    out = torch.full((2 * 2 * 8 * 8 * 8 + 4,), SENT, dtype=torch.float32).to(dev)
    y, yf = out.data_ptr(), out.data_ptr() + 4 * 2 * 8 * 8 * 8
    assert y % 16 == 0
    names = ("src", "typ", "F", "Hs", "Ws", "C", "fo", "valid", "inv", "B", "border", "mean", "std", "y", "yf", "Ho", "Wo", "ld", "stream")
    ok = (src.data_ptr(), U8, 2, 6, 5, 3, fo.data_ptr(), None, inv.data_ptr(), 2, 128.0, 128.0, 256.0, y, yf, 8, 8, 4, ops._stream(out))

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_crop_to_nhwc(*[a[n] for n in names])

    for bad in (dict(src=None), dict(inv=None), dict(y=None, yf=None), dict(yf=y), dict(typ=2), dict(typ=-1), dict(F=0), dict(F=-2),
                dict(B=0), dict(B=-1), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-8), dict(C=0), dict(C=5), dict(C=-1), dict(ld=2),
                dict(ld=6), dict(ld=0), dict(C=4, ld=3), dict(y=y + 4), dict(yf=yf + 8), dict(y=None, yf=yf + 4), dict(fo=None, F=1),
                dict(fo=None, F=3), dict(fo=None, B=1), dict(std=0.0), dict(std=-256.0), dict(std=float("nan"))):
        assert call(**bad) == -1, bad
        assert L.up_last_error().startswith(b"crop_to_nhwc:"), (bad, L.up_last_error())
    assert bool((out.cpu() == SENT).all())                                            # nothing was launched
    assert call() == 0 and call(fo=None) == 0 and call(yf=None) == 0 and call(y=None) == 0 and call(ld=8) == 0
    assert not bool((out.cpu()[:2 * 8 * 8 * 4] == SENT).any())
    px = torch.zeros(2, 6, 5, 3, dtype=torch.uint8).to(dev)
    ident = np.array([[1.0, 0, 0, 0, 1, 0]] * 2)
    for kw in (dict(inv=ident[:1]), dict(inv=ident, frame_of=[0]), dict(inv=ident, valid_hw=[(6, 5)]), dict(inv=ident.reshape(3, 4)),
               dict(inv=np.where(np.arange(6) == 2, np.nan, ident))):
        try:
            ops.crop_to_nhwc(px, kw.pop("inv"), (4, 4), **kw)
            raise AssertionError("ValueError expected")
        except ValueError:
            pass
    try:
        ops.crop_to_nhwc(px.to(torch.int32), ident, (4, 4))
        raise AssertionError("TypeError expected")
    except TypeError:
        pass
    for kw in (dict(ld=6), dict(ld=0)):
        try:
            ops.crop_to_nhwc(px, ident, (4, 4), **kw)
            raise AssertionError("refused by the entry")
        except _C.UniPoseHipError:
            pass


# ---- 3. the plan programs ----------------------------------------------------------------------------------------------------------
def plan_cases(cases):
    """protocol_cases' plan cases without the stride = 1 one, each with the flip test off and on"""
    return [dict(c, flip=f) for c in cases if c.get("stride", 8) == 8 for f in (False, True)]


def plan_id(case):
    return "-".join(f"{k}{v}" for k, v in case.items())


def plan_case(dev, K=14, B=1, height=64, width=64, output_stride=16, bbox=False, dataset="LSP", flip=False):
    import protocol_cases as pc
    from unipose_amd.plan import UniPosePlan
    L = _C.lib()
    m = pc._model(dev, K, output_stride, bbox)
    plan = UniPosePlan(m, B, height, width)
    frames = torch.from_numpy(pixels_of((8, K), (2, 40, 56, 3), "u8")).to(dev)
    fo = [1] * B
    cen = np.stack([np.array([28.0 + 5 * i, 20.0 - 3 * i]) for i in range(B)])
    sc = np.array([0.25 * (1 + 0.3 * i) for i in range(B)])
    rot = 30 if flip else 0
    # the workspace: each program from frames reports its own need; the figures of the existing programs are what they were
    base = [L.up_unipose_plan_program_workspace(plan._plan, k) for k in range(7)]
    needs = {k: L.up_unipose_plan_program_workspace(plan._plan, FROM_FRAMES + k) for k in range(8)}
    assert all(needs[k] > 0 for k in (0, 4, 5, 6)) and all(needs[k] == 0 for k in (1, 2, 3, 7))
    assert L.up_unipose_plan_program_workspace(plan._plan, FROM_FRAMES - 1) == 0
    assert needs[0] == base[0] and needs[6] == base[6]                              # the crop writes where the layout pass wrote
    print("workspace from frames", needs, "existing programs", base)
    assert L.up_unipose_plan_workspace(plan._plan) == max(base[:4]) and L.up_unipose_plan_flip_workspace(plan._plan) == max(base[4:7])
    x = ops.augment_image(frames[fo], protocol.crop_maps(cen, sc, [height, width], rot).reshape(B, 2, 3), (height, width))
    ref = plan.final_preds(x, cen, sc, flip=flip, dataset=dataset)
    got = plan.frame_final_preds(frames, cen, sc, frame_of=fo, rot=rot, flip=flip, dataset=dataset)
    pc.same_triple([host(t) for t in got], [host(t) for t in ref], ("frame_final_preds", flip))
    if flip:
        want = plan.flip_heatmaps(x, dataset)
    else:
        want = torch.cat(plan(x), 1) if bbox else plan(x)
    own = torch.full((B, plan.out_channels, plan.map_height, plan.map_width), SENT, device=dev)
    heat = plan.frame_heatmaps(frames, cen, sc, frame_of=fo, rot=rot, flip=flip, dataset=dataset, out=own)
    assert heat is own and bits_equal(host(heat), host(want))
    assert plan.workspace.numel() >= needs[4 if flip else 0] + 256
    if B == 2:                                       # two persons of one frame: two crops, two sets of maps
        assert not bits_equal(host(heat)[0], host(heat)[1])
    # refusals of the C entries, before anything is launched
    ws = plan.workspace
    off = (-ws.data_ptr()) % 256
    wp, wn = ws.data_ptr() + off, ws.numel() - off
    perm = protocol.flip_perm(dataset, K, bbox)
    pa = ops._perm_array(perm, len(perm)) if flip else None
    inv = torch.from_numpy(protocol.crop_maps(cen, sc, [height, width], rot)).to(dev)
    fot = torch.tensor(fo, dtype=torch.int32).to(dev)
    o = own.data_ptr()
    src = (frames.data_ptr(), U8, 2, 40, 56, fot.data_ptr(), None, inv.data_ptr(), 128.0, 128.0, 256.0)
    sent = torch.full_like(own, SENT)
    so = sent.data_ptr()
    need_h, need_p = needs[4 if flip else 0], needs[5 if flip else 6]
    assert L.up_unipose_frame_heatmaps(plan._plan, *src, pa, so, wp, need_h - 1, 0) == -1 and b"workspace" in L.up_last_error()
    assert L.up_unipose_frame_final_preds(plan._plan, *src, pa, None, 8, 8, so, None, so, wp, need_p - 1, 0) == -1
    assert b"workspace" in L.up_last_error()
    if flip:
        badp = ops._perm_array([len(perm)] + perm[1:], len(perm))
        assert L.up_unipose_frame_heatmaps(plan._plan, *src, badp, so, wp, wn, 0) == -1 and b"perm[0]" in L.up_last_error()
        assert L.up_unipose_frame_final_preds(plan._plan, *src, badp, None, 8, 8, so, None, so, wp, wn, 0) == -1
    assert L.up_unipose_frame_final_preds(plan._plan, *src, pa, None, 0, 8, so, None, so, wp, wn, 0) == -1
    assert L.up_unipose_frame_final_preds(plan._plan, *src, pa, None, 8, 8, None, None, so, wp, wn, 0) == -1
    for bad in (dict(i=0, v=None), dict(i=7, v=None), dict(i=1, v=2), dict(i=2, v=0), dict(i=3, v=-1), dict(i=4, v=0),
                dict(i=10, v=0.0), dict(i=10, v=float("nan"))):
        a = list(src)
        a[bad["i"]] = bad["v"]
        assert L.up_unipose_frame_heatmaps(plan._plan, *a, pa, so, wp, wn, 0) == -1, bad
        assert L.up_unipose_frame_final_preds(plan._plan, *a, pa, None, 8, 8, so, None, so, wp, wn, 0) == -1, bad
    a = list(src)
    a[2], a[5] = B + 1, None                         # no frame_of: F must be the batch
    assert L.up_unipose_frame_heatmaps(plan._plan, *a, pa, so, wp, wn, 0) == -1 and b"frame_of" in L.up_last_error()
    assert bool((sent == SENT).all())                # no refused call wrote anything
    for kw in (dict(frame_of=[1] * (B + 1)), dict(frame_of=None) if B != 2 else dict(valid_hw=[(40, 56)]), dict(valid_hw=[(40, 56)] * 3)):
        try:
            plan.frame_heatmaps(frames, cen, sc, **({"frame_of": fo} | kw))
            raise AssertionError(f"{kw} must be refused")
        except ValueError:
            pass
    try:
        plan.frame_heatmaps(frames.float().permute(0, 3, 1, 2), cen, sc, frame_of=fo)
        raise AssertionError("NCHW frames must be refused")
    except ValueError:
        pass
    plan.close()


def plan_unset_case(dev):
    from unipose_amd.plan import _Config
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_plan_create(C.byref(_Config(1, 64, 52, 16, 15)), C.byref(plan)) == 0
    buf = torch.zeros(4096).to(dev)
    p = buf.data_ptr()
    pa = ops._perm_array(list(range(15)), 15)
    src = (p, U8, 1, 4, 4, None, None, p, 128.0, 128.0, 256.0)
    for perm in (None, pa):
        assert L.up_unipose_frame_heatmaps(plan, *src, perm, p, p, 1 << 40, 0) != 0 and b"never set" in L.up_last_error()
        assert L.up_unipose_frame_final_preds(plan, *src, perm, None, 8, 7, p, None, p, p, 1 << 40, 0) != 0
        assert b"never set" in L.up_last_error()
    assert L.up_unipose_frame_heatmaps(plan, *src, None, None, p, 1 << 40, 0) == -1 and b"null" in L.up_last_error()
    L.up_unipose_plan_destroy(plan)
