"""The video plan from source frames (up_clip_crop_to_nhwc, up_center_pool, up_clip_center_pool, up_clip_center_pool_flip;
up_unipose_lstm_clip_frame_heatmaps / _clip_frame_final_preds / _stream_frame_final_preds; ops.clip_crop_to_nhwc, ops.center_pool;
UniPoseLSTMPlan.clip_frame_heatmaps / clip_frame_final_preds / stream_frames): shared by test_video_frame_emu.py and
test_video_frame_gpu.py.

Every new entry is a composition of existing entries with a reordering (and the Gaussian) folded in, so the yardstick is always that
composition — up_crop_to_nhwc of the flattened clip; up_make_gaussian_maps then the pooling entries; the existing plan entries on
ops.augment_image's crop and ops.make_centermaps' maps — and every comparison is for equal bits or exact integers.  Nothing here
has a tolerance."""
import ctypes as C
import functools
import mmap

import numpy as np
import torch

from unipose_amd import _C, ops, protocol

import frame_cases as fc
import video_eval_cases as vc
from frame_cases import FROM_FRAMES, PF32, SENT, U8, bits_equal, host

F32 = np.float32
PAIRS = vc.PAIRS


def _ptr(t):
    return None if t is None else t.data_ptr()


def front_guarded(arr):
    """a host tensor holding `arr` that BEGINS right behind an inaccessible page (guard_alloc.guarded ends right before one): a read
    in front of a source buffer — a frame index of -1 — faults on the emulator"""
    import guard_alloc
    arr = np.ascontiguousarray(arr)
    page = mmap.PAGESIZE
    body = (max(arr.nbytes, 1) + page - 1) // page * page
    m = mmap.mmap(-1, page + body)
    addr = C.addressof(C.c_char.from_buffer(m))
    if guard_alloc._libc.mprotect(C.c_void_p(addr), page, 0) != 0:
        raise OSError(C.get_errno(), "mprotect failed")
    guard_alloc._keep.append(m)
    t = torch.from_numpy(np.frombuffer(m, dtype=arr.dtype, count=arr.size, offset=page).reshape(arr.shape))
    t.copy_(torch.from_numpy(arr))
    return t


# ---- 1. up_clip_crop_to_nhwc against up_crop_to_nhwc of the flattened clip ----------------------------------------------------------
def run_clip_crop(dev, frames, inv, out_hw, bt, frame_of=None, valid=None, ld=4, which="both", alloc=None, border=128.0, src=None):
    """up_clip_crop_to_nhwc itself on sentinel-filled outputs -> (y, y_flip) numpy (T*B,Ho,Wo,ld) frame-major, None where not asked for.
    inv (B*T,6), frame_of (B*T) batch-major, flattened; src: the source tensor already placed (front_guarded)"""
    B, T = bt
    s = fc._place(frames, dev, alloc) if src is None else src
    nf, hs, ws, c = s.shape
    m = torch.from_numpy(np.ascontiguousarray(inv, dtype=np.float64).reshape(B * T, 6)).to(dev)
    fo = None if frame_of is None else torch.tensor(np.asarray(frame_of).reshape(B, T), dtype=torch.int32).to(dev)
    vt = None if valid is None else torch.tensor(np.asarray(valid), dtype=torch.int32).to(dev)
    shape = (T * B, out_hw[0], out_hw[1], ld)
    y = fc._sentinel(shape, dev, alloc) if which in ("both", "y") else None
    yf = fc._sentinel(shape, dev, alloc) if which in ("both", "flip") else None
    _C.check(_C.lib().up_clip_crop_to_nhwc(s.data_ptr(), U8 if s.dtype == torch.uint8 else PF32, nf, hs, ws, c, _ptr(fo), _ptr(vt),
                                           m.data_ptr(), B, T, border, 128.0, 256.0, _ptr(y), _ptr(yf), out_hw[0], out_hw[1], ld,
                                           ops._stream(s)), "clip_crop_to_nhwc")
    return None if y is None else host(y), None if yf is None else host(yf)


def frame_major(a, bt):
    """batch-major rows (B * T, ...) -> frame-major (T * B, ...)"""
    B, T = bt
    return np.ascontiguousarray(a.reshape((B, T) + a.shape[1:]).swapaxes(0, 1).reshape((T * B,) + a.shape[1:]))


def same_as_batch_crop(got, ref, bt, c, what):
    """got: the clip entry's pair; ref: up_crop_to_nhwc's pair of the B * T flattened samples (both outputs)"""
    for g, r, n in zip(got, ref, ("y", "y_flip")):
        if g is None:
            continue
        assert not (g == SENT).any(), (what, n, "an element was not written")
        assert (g[..., c:] == 0.0).all() and not np.signbit(g[..., c:]).any(), (what, n, "a pad lane is not +0")
        assert bits_equal(g, frame_major(r, bt)), (what, n)


CLIP_BT = [(1, 1), (2, 3), (3, 2)]
CLIP_SRCS = [(1, 1), (5, 7), (20, 12)]
CLIP_OUTS = [(1, 1), (2, 7), (5, 65), (33, 65)]
MODES = ["shared", "perm", "null"]         # frame_of: two frames shared by all samples; a permutation of B * T frames; NULL


def clip_maps_for(src_hw, out_hw, n, last):
    """n maps, all different: the identity, a fractional translation, a rotation with a zoom, the zoom the other way, another
    translation — and as the LAST sample one that is all border (outside, two with 1e12, two with NaN, chosen by `last`)"""
    nan = float("nan")
    fit = max(out_hw[0] / src_hw[0], out_hw[1] / src_hw[1])          # the zoom at which the output just covers the source
    sampling = [[1.0, 0, 0, 0, 1, 0], [1.0, 0, 0.25, 0, 1, -0.5], fc.rotation(src_hw, out_hw, 1.3 * fit, 30.0),
                fc.rotation(src_hw, out_hw, 0.8 * fit, -30.0), [1.0, 0, -0.5, 0, 1, 0.25]]
    border = [[1.0, 0, 1000, 0, 1, 1000], [1.0, 0, 1e12, 0, 1, -1e12], [1e12, 0, 0, 0, 1e12, 0], [nan, 0, 0, 0, 1, 0], [1.0, 0, 0, nan, nan, nan]]
    return np.array((sampling[:n - 1] if n > 1 else []) + [border[last % 5] if n > 1 else sampling[last % 5]])


def _clip_cases():
    res, n = [], 0
    for typ in ("u8", "f32"):
        for src in CLIP_SRCS:
            for out in CLIP_OUTS:
                mode = MODES[(n + n // 3) % 3]
                if mode == "shared" and (src == (1, 1) or out == (1, 1)):
                    mode = "perm"                   # one pixel: samples that share a frame could not all differ
                res.append(dict(typ=typ, src=src, out=out, bt=CLIP_BT[(n + n // 4) % 3], layout=fc.LAYOUTS[n % 6], which=fc.WHICH[(n // 2) % 3],
                                mode=mode, last=n))
                n += 1
    return res


CLIP_CASES = _clip_cases()
CLIP_IDS = ["%s_%dx%d_to_%dx%d_B%dT%d_c%d_ld%d_%s_%s" % (c["typ"], *c["src"], *c["out"], *c["bt"], *c["layout"], c["which"], c["mode"])
            for c in CLIP_CASES]
assert {c["layout"] for c in CLIP_CASES} == set(fc.LAYOUTS) and {c["which"] for c in CLIP_CASES} == set(fc.WHICH)
assert {c["mode"] for c in CLIP_CASES} == set(MODES) and {c["bt"] for c in CLIP_CASES} == set(CLIP_BT)
assert {c["last"] % 5 for c in CLIP_CASES if c["bt"] != (1, 1)} == set(range(5))


def clip_crop_case(dev, case, alloc=None):
    (hs, ws), out, (c, ld), bt = case["src"], case["out"], case["layout"], case["bt"]
    n = bt[0] * bt[1]
    nf = 2 if case["mode"] == "shared" else n
    frames = fc.pixels_of((31, hs, ws, c, *out, n), (nf, hs, ws, c), case["typ"])
    inv = clip_maps_for((hs, ws), out, n, case["last"])
    fo = {"shared": [i % 2 for i in range(n)], "perm": list(range(n))[::-1], "null": None}[case["mode"]]
    ref = fc.run_crop(dev, frames, inv, out, fo, ld=ld)                              # the batch entry, both outputs
    exp = ref[0][..., :c]
    for i in range(n):                              # a batch-major / frame-major mix-up cannot pass: no two samples agree
        for j in range(i + 1, n):
            assert not bits_equal(exp[i], exp[j]), (case, i, j)
    got = run_clip_crop(dev, frames, inv, out, bt, fo, ld=ld, which=case["which"], alloc=alloc)
    assert (got[0] is None) == (case["which"] == "flip") and (got[1] is None) == (case["which"] == "y")
    same_as_batch_crop(got, ref, bt, c, case)
    if bt[1] == 1:                                  # T = 1 is up_crop_to_nhwc itself
        for g, r in zip(got, ref):
            assert g is None or bits_equal(g, r)


def clip_ops_case(dev):
    """ops.clip_crop_to_nhwc is the same entry, its checks those of ops.crop_to_nhwc"""
    bt, out = (2, 3), (9, 14)
    frames = fc.pixels_of((32,), (3, 20, 12, 3), "u8")
    inv = clip_maps_for((20, 12), out, 6, 0)
    fo = [2, 0, 1, 1, 2, 0]
    ref = fc.run_crop(dev, frames, inv, out, fo)
    t = torch.from_numpy(frames).to(dev)
    y, yf = ops.clip_crop_to_nhwc(t, inv.reshape(2, 3, 6), out, clip=bt, frame_of=np.reshape(fo, bt), flip=True)
    assert tuple(y.shape) == (6, 9, 14, 4) and bits_equal(host(y), frame_major(ref[0], bt)) and bits_equal(host(yf), frame_major(ref[1], bt))
    y8 = ops.clip_crop_to_nhwc(t, inv.reshape(2, 3, 2, 3), out, clip=bt, frame_of=np.reshape(fo, bt), ld=8)
    assert tuple(y8.shape) == (6, 9, 14, 8) and bits_equal(host(y8)[..., :4], frame_major(ref[0], bt))
    for kw in (dict(inv=inv), dict(inv=inv.reshape(3, 2, 6)), dict(frame_of=fo), dict(frame_of=None), dict(frame_of=[[0, 1, 3], [0, 1, 2]]),
               dict(valid_hw=[(20, 12)]), dict(clip=(2, 0))):
        a = dict(inv=inv.reshape(2, 3, 6), clip=bt, frame_of=np.reshape(fo, bt))
        a.update(kw)
        try:
            ops.clip_crop_to_nhwc(t, a.pop("inv"), out, **a)
            raise AssertionError(f"{kw} must be refused")
        except ValueError:
            pass


def clip_valid_case(dev, alloc=None):
    """valid_hw is per source FRAME; what lies beyond it (NaN resp. 255) is never read"""
    valid = [(20, 12), (7, 9), (1, 1)]
    hs, ws, c, out, bt = 20, 12, 3, (9, 14), (2, 2)
    inv = np.stack([fc.rotation(v, out, 0.6, 37.0) for v in valid[:2]] + [np.array([0.25, 0.0, -0.5, 0.0, 0.25, -0.5])])
    fo = [1, 2, 0, 1]                                                                  # two samples in the 7 x 9 frame
    maps = inv[[1, 2, 0, 0]]
    for typ, fill in (("f32", float("nan")), ("u8", 255)):
        buf = np.full((3, hs, ws, c), fill, dtype=np.float32 if typ == "f32" else np.uint8)
        for i, (h, w) in enumerate(valid):
            img = fc.pixels_of((33, i), (h, w, c), typ)
            buf[i, :h, :w] = img // 2 if typ == "u8" else img                           # never 255: a padding pixel read would show
        ref = fc.run_crop(dev, buf, maps, out, fo, valid=valid)
        got = run_clip_crop(dev, buf, maps, out, bt, fo, valid=valid, alloc=alloc)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), typ
        same_as_batch_crop(got, ref, bt, c, (typ, "valid"))
        assert not bits_equal(got[0][1], got[0][2])                                     # samples (1, 0) and (0, 1) are not alike


def clip_bad_frame_case(dev, alloc=None, front=False):
    """a frame index of -1 and one of F: those samples are all border, nothing is loaded for them, the others do not notice.
    front (the emulator): the source also once BEGINS right behind an inaccessible page, as with alloc it ends right before one"""
    out, bt = (9, 14), (2, 2)
    for typ in ("u8", "f32"):
        frames = fc.pixels_of((34,), (2, 20, 12, 3), typ)
        maps = np.array([fc.rotation((20, 12), out), [1.0, 0, 0, 0, 1, 0], fc.rotation((20, 12), out, 0.8, -70.0), [1.0, 0, -3, 0, 1, 4]])
        good = fc.run_crop(dev, frames, maps, out, [0, 1, 1, 0])
        for fo in ([-1, 1, 2, 0], [2, 1, -1, 0]):                                      # F = 2: -1 and F
            for src in ([None, front_guarded(frames).to(dev)] if front else [None]):
                got = run_clip_crop(dev, frames, maps, out, bt, fo, alloc=alloc, src=src)
                flat = (F32(128.0) - F32(128.0)) / F32(256.0)
                for g, r in zip(got, good):
                    # batch-major samples 0 and 2 are frame-major images 0 and 1; samples 1 and 3 images 2 and 3
                    assert (g[[0, 1]][..., :3] == flat).all() and (g[[0, 1]][..., 3:] == 0.0).all(), (typ, fo)
                    assert bits_equal(g[[2, 3]], r[[1, 3]]), (typ, fo)
        try:                                                                           # ops refuses host indices before any launch
            ops.clip_crop_to_nhwc(torch.from_numpy(frames).to(dev), maps.reshape(2, 2, 6), out, clip=bt, frame_of=[[0, 2], [1, 0]])
            raise AssertionError("ValueError expected")
        except ValueError:
            pass


BIG_OUT = (725, 725)                                # 4 samples of 525 625 pixels: 2 102 500 > 2^21, the second trip starts inside sample 3


def clip_big_case(dev):
    """more than 2^21 output pixels in one launch: the grid walks them in a second trip"""
    bt = (2, 2)
    assert 4 * BIG_OUT[0] * BIG_OUT[1] > 2 ** 21 > 3 * BIG_OUT[0] * BIG_OUT[1]
    frames = fc.pixels_of((35,), (2, 20, 12, 3), "u8")
    inv = np.array([fc.rotation((20, 12), BIG_OUT, 50.0, 30.0), fc.rotation((20, 12), BIG_OUT, 40.0, -20.0), fc.rotation((20, 12), BIG_OUT, 60.0, 5.0),
                    fc.rotation((20, 12), BIG_OUT, 45.0, 77.0)])
    fo = [1, 0, 0, 1]
    ref = fc.run_crop(dev, frames, inv, BIG_OUT, fo)
    got = run_clip_crop(dev, frames, inv, BIG_OUT, bt, fo)
    same_as_batch_crop(got, ref, bt, 3, "big")
    assert np.abs(got[0][3, -1]).max() > 0 and np.abs(got[0][0, 0]).max() > 0         # both trips show pixels


# ---- 2. the centre pool against up_make_gaussian_maps then the pooling entries -------------------------------------------------------
POOL_HW = [(7, 7), (8, 16), (15, 23), (16, 24)]
POOL_BT = [(1, 2), (2, 3)]
POOL_N = [1, 5]
SIGMAS = [0.5, 3.0, 40.0]
CENTER_KINDS = 8


def centers_for(hw, n, first):
    """n centres, all different, walking the eight kinds from kind `first`: inside the map, (0, 0), (W-1, H-1), fractional, outside,
    on the last column (where the one-sided padding makes the mirrored pool differ), 1e12, NaN"""
    H, W = hw
    kinds = [(W * 0.47, H * 0.42), (0.0, 0.0), (W - 1.0, H - 1.0), (3.25, 7.5), (-5.0, H + 3.0), (W - 1.0, float(H // 2)), (1e12, 2.0),
             (float("nan"), 1.0)]
    assert len(kinds) == CENTER_KINDS
    return np.array([kinds[(first + i) % CENTER_KINDS] for i in range(n)], dtype=np.float64)


def _pool_cases():
    clip, plain, k = [], [], 0
    for hw in POOL_HW:
        for sigma in SIGMAS:
            for bt in POOL_BT:
                clip.append(dict(hw=hw, sigma=sigma, bt=bt, coff=14 + k % 2, first=(3 * k) % CENTER_KINDS))
                k += 1
            for n in POOL_N:
                plain.append(dict(hw=hw, sigma=sigma, n=n, coff=14 + k % 2, first=(3 * k) % CENTER_KINDS))
                k += 1
    return clip, plain


POOL_CLIP_CASES, POOL_PLAIN_CASES = _pool_cases()


def _pool_id(c):
    lead = "B%dT%d" % c["bt"] if "bt" in c else "N%d" % c["n"]
    return "%dx%d_s%g_%s_c%d_k%d" % (*c["hw"], c["sigma"], lead, c["coff"], c["first"])


def _kinds_seen(cases):
    seen = set()
    for c in cases:
        n = c["bt"][0] * c["bt"][1] if "bt" in c else c["n"]
        seen |= {(c["first"] + i) % CENTER_KINDS for i in range(n)}
    return seen


assert _kinds_seen(POOL_CLIP_CASES) == set(range(CENTER_KINDS)) == _kinds_seen(POOL_PLAIN_CASES)


def center_pool_case(dev, case, alloc=None):
    """the three entries into channel coff of a sentinel-filled ld = 16 tensor: equal bits, lane by lane, to the two-call form"""
    L = _C.lib()
    (H, W), sigma, coff, ld = case["hw"], case["sigma"], case["coff"], 16
    P, Q = (H - 7) // 8 + 1, (W - 7) // 8 + 1
    clip = "bt" in case
    B, T = case["bt"] if clip else (case["n"], 1)
    n = B * T
    cen = centers_for((H, W), n, case["first"])
    assert len({tuple(np.nan_to_num(c, nan=-77.0)) for c in cen}) == n                 # all different
    cxy = torch.from_numpy(cen).to(dev)
    maps = torch.full((n, 1, H, W), SENT, dtype=torch.float32, device=dev)
    st = ops._stream(maps)
    _C.check(L.up_make_gaussian_maps(cxy.data_ptr(), n, H, W, sigma, maps.data_ptr(), st), "make_gaussian_maps")
    forms = [("clip", L.up_clip_center_pool, L.up_clip_avgpool9s8_fwd), ("flip", L.up_clip_center_pool_flip, L.up_clip_avgpool9s8_flip_fwd)] \
        if clip else [("plain", L.up_center_pool, L.up_avgpool9s8_fwd)]
    for name, entry, pool in forms:
        lead = (B, T) if clip else (n,)
        got = vc._dev_tensor(dev, (n, P, Q, ld), alloc)
        ref = vc._dev_tensor(dev, (n, P, Q, ld))
        _C.check(entry(cxy.data_ptr(), sigma, got.data_ptr(), ld, coff, *lead, H, W, P, Q, st), name)
        _C.check(pool(maps.data_ptr(), ref.data_ptr(), ld, coff, *lead, H, W, P, Q, st), name + " (two calls)")
        g, r = host(got), host(ref)
        assert bits_equal(g, r), (case, name, g[..., coff].reshape(-1)[:8], r[..., coff].reshape(-1)[:8])
        keep = np.arange(ld) != coff
        assert (g[..., keep] == SENT).all(), (case, name, "another lane was touched")
        # NaN propagates, an infinite distance gives 0
        rows = g[..., coff].reshape((T, B, P, Q)).swapaxes(0, 1).reshape(n, P, Q) if clip else g[..., coff]
        for i, c in enumerate(cen):
            if np.isnan(c).any():
                assert np.isnan(rows[i]).all(), (case, name, i)
            elif abs(c[0]) >= 1e12:
                assert (rows[i] == 0).all() and not np.signbit(rows[i]).any(), (case, name, i)
    if clip:                                        # ops.center_pool is the same entries
        out = vc._dev_tensor(dev, (n, P, Q, ld))
        assert ops.center_pool(cen.reshape(B, T, 2), (H, W), sigma, out=out, coff=coff, clip=(B, T), flip=True) is out
        assert bits_equal(host(out), r)
    else:
        fresh = ops.center_pool(cen, (H, W), sigma, device=dev)
        assert tuple(fresh.shape) == (n, P, Q, 4) and bits_equal(host(fresh)[..., 0], r[..., coff]) and (host(fresh)[..., 1:] == 0).all()


def gauss_restated(cen, hw, sigma):
    """up_make_gaussian_maps in numpy: (maps (N, H, W) float32, d2 (N, H, W) float64)"""
    H, W = hw
    x, y = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    with np.errstate(all="ignore"):
        dx, dy = x - cen[:, 0, None, None], y - cen[:, 1, None, None]
        d2 = dx * dx + dy * dy
        v = np.exp(-d2 / 2.0 / sigma / sigma)
        v = np.where(v > 1.0, 1.0, v)
        v = np.where(v < 0.0099, 0.0, v)
    return v.astype(F32), d2


def inputs_discriminate_case():
    """What the cases above can tell apart, asserted on their own inputs with the numpy float32 restatement of the pooling
    (video_eval_cases._pool_restated): a kernel that summed a window in descending column order, or that mirrored the pooled result
    in place of pooling the mirrored map, gives other bits in at least one case.  No device."""
    order = mirror = 0
    for case in POOL_CLIP_CASES:
        n = case["bt"][0] * case["bt"][1]
        g, _ = gauss_restated(centers_for(case["hw"], n, case["first"]), case["hw"], case["sigma"])
        fin = ~np.isnan(g).any(axis=(1, 2))
        g = g[fin]
        right = vc._pool_restated(g, False)
        order += int((right.view(np.int32) != vc._pool_restated(g, True).view(np.int32)).any())
        flipped = vc._pool_restated(np.ascontiguousarray(g[:, :, ::-1]), False)
        mirror += int((flipped.view(np.int32) != np.ascontiguousarray(right[:, :, ::-1]).view(np.int32)).any())
    assert order >= 1, "no case tells the summation order"
    assert mirror >= 1, "no case tells the mirror definition"
    # at sigma = 3 on 16 x 24: a tap beyond any skip bound (a bound must lie above the cut, and nothing sensible lies above
    # 2 sigma^2 * 6) and a tap within one pixel of the 0.0099 radius, on either side of it
    cases = [c for c in POOL_CLIP_CASES + POOL_PLAIN_CASES if c["hw"] == (16, 24) and c["sigma"] == 3.0]
    assert cases
    far = near_in = near_out = False
    radius = 3.0 * np.sqrt(2.0 * np.log(1.0 / 0.0099))
    for case in cases:
        n = case["bt"][0] * case["bt"][1] if "bt" in case else case["n"]
        g, d2 = gauss_restated(centers_for(case["hw"], n, case["first"]), case["hw"], 3.0)
        ok = np.isfinite(d2)
        far |= bool((d2[ok] > 2 * 9.0 * 6.0).any())
        dist = np.sqrt(d2[ok])
        near_in |= bool(((dist < radius) & (dist > radius - 1.0) & (g[ok] > 0)).any())
        near_out |= bool(((dist > radius) & (dist < radius + 1.0) & (g[ok] == 0)).any())
    assert far and near_in and near_out
    return order, mirror


# ---- 3. refusals of the five kernels: UP_ERR_INVALID, nothing written (no launch: needs no device) ---------------------------------------
def kernel_refusal_case(dev):
    L = _C.lib()
    src = torch.zeros(4, 6, 5, 3, dtype=torch.uint8).to(dev)
    inv = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 4, dtype=torch.float64).to(dev)
    fo = torch.tensor([0, 1, 2, 3], dtype=torch.int32).to(dev)
    out = torch.full((2 * 4 * 8 * 8 * 8 + 4,), SENT, dtype=torch.float32).to(dev)
    y, yf = out.data_ptr(), out.data_ptr() + 4 * 4 * 8 * 8 * 8
    assert y % 16 == 0
    names = ("src", "typ", "F", "Hs", "Ws", "C", "fo", "valid", "inv", "B", "T", "border", "mean", "std", "y", "yf", "Ho", "Wo", "ld", "stream")
    ok = (src.data_ptr(), U8, 4, 6, 5, 3, fo.data_ptr(), None, inv.data_ptr(), 2, 2, 128.0, 128.0, 256.0, y, yf, 8, 8, 4, 0)

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_clip_crop_to_nhwc(*[a[n] for n in names])

    for bad in (dict(src=None), dict(inv=None), dict(y=None, yf=None), dict(yf=y), dict(typ=2), dict(typ=-1), dict(F=0), dict(F=-2),
                dict(B=0), dict(B=-1), dict(T=0), dict(T=-2), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-8), dict(C=0), dict(C=5),
                dict(C=-1), dict(ld=2), dict(ld=6), dict(ld=0), dict(C=4, ld=3), dict(y=y + 4), dict(yf=yf + 8), dict(y=None, yf=yf + 4),
                dict(fo=None, F=2), dict(fo=None, F=5), dict(fo=None, B=1), dict(fo=None, T=1), dict(std=0.0), dict(std=-256.0),
                dict(std=float("nan"))):
        assert call(**bad) == -1, bad
        assert L.up_last_error().startswith(b"clip_crop_to_nhwc:"), (bad, L.up_last_error())
    assert bool((out.cpu() == SENT).all())                                            # nothing was launched
    cxy = torch.tensor([[3.0, 4.0]] * 4, dtype=torch.float64).to(dev)
    q = out.data_ptr()
    for fn, lead in ((L.up_center_pool, (4,)), (L.up_clip_center_pool, (2, 2)), (L.up_clip_center_pool_flip, (2, 2))):
        pn = ("c", "sigma", "y", "ld", "coff") + (("N",) if len(lead) == 1 else ("B", "T")) + ("H", "W", "P", "Q", "st")
        pok = (cxy.data_ptr(), 3.0, q, 4, 3) + lead + (8, 16, 1, 2, 0)
        bads = [dict(c=None), dict(y=None), dict(sigma=0.0), dict(sigma=-3.0), dict(sigma=float("nan")), dict(ld=0), dict(coff=-1),
                dict(coff=4), dict(H=0), dict(W=0), dict(H=-8), dict(P=2), dict(Q=1), dict(P=0), dict(H=6, P=0), dict(W=6, Q=0),
                dict(H=1 << 16, W=1 << 16, P=8192, Q=8192)]
        bads += [dict(N=0), dict(N=-1)] if len(lead) == 1 else [dict(B=0), dict(T=0), dict(B=-1), dict(T=-3)]
        for bad in bads:
            a = dict(zip(pn, pok))
            a.update(bad)
            assert fn(*[a[n] for n in pn]) == -1, (fn, bad)
    assert bool((out.cpu() == SENT).all())
    # the arguments they were derived from are accepted
    assert call() == 0 and call(fo=None) == 0 and call(yf=None) == 0 and call(y=None) == 0 and call(ld=8) == 0
    assert L.up_clip_center_pool(cxy.data_ptr(), 3.0, q, 4, 3, 2, 2, 8, 16, 1, 2, 0) == 0
    for kw in (dict(hw=(8, 16), clip=(2, 3)), dict(hw=(8, 16), flip=True), dict(hw=(8, 16), out=torch.zeros(4, 1, 2, 4).to(dev)),
               dict(hw=(8, 16), out=torch.zeros(4, 1, 3, 4).to(dev), coff=0)):
        try:
            ops.center_pool(cxy, kw.pop("hw"), **kw)
            raise AssertionError(f"{kw} must be refused")
        except ValueError:
            pass


# ---- 4. the plan programs ------------------------------------------------------------------------------------------------------------
FRAME_HW = (45, 60)


class FrameCtx:
    """The inputs from frames of one plan (video_eval_cases.ctx: the plan is shared with those tests), what the existing entries make of
    them — computed once per configuration and shared, unchanged, by the tests — and the sizes the plan reported before any new
    entry ran."""

    def __init__(self, c):
        L = _C.lib()
        self.c, self.plan, self.dev = c, c.plan, c.dev
        B, T, H, W, dev, plan = c.B, c.T, c.H, c.W, c.dev, c.plan
        n = B * T
        self.ws_before = (L.up_unipose_lstm_plan_workspace(plan._plan), L.up_unipose_lstm_plan_flip_workspace(plan._plan))
        self.frames = torch.from_numpy(fc.pixels_of((36, c.K), (3,) + FRAME_HW + (3,), "u8")).to(dev)
        self.valid = [FRAME_HW, (40, 50), FRAME_HW]                                  # one frame with a smaller valid extent
        self.fo = np.array([(2 * i + 1) % 3 for i in range(n)]).reshape(B, T)      # shared (n > 3) and permuted
        self.center = np.array([[30.0 + 3 * i, 22.0 - 2 * i] for i in range(n)]).reshape(B, T, 2)
        self.scale = np.array([0.2 * (1 + 0.15 * i) for i in range(n)]).reshape(B, T)
        self.cc = np.array([[W / 2 + 2.5 * i - 3, H / 2 - 1.75 * i + 2] for i in range(n)]).reshape(B, T, 2)     # differs per frame
        self.rot = 20
        self.kw = dict(frame_of=self.fo, rot=self.rot, valid_hw=self.valid, crop_center=self.cc)
        fo = self.fo.reshape(-1)
        maps = protocol.crop_maps(self.center.reshape(n, 2), self.scale.reshape(n), [H, W], self.rot).reshape(n, 2, 3)
        self.x = ops.augment_image(self.frames[torch.from_numpy(fo).to(dev)], maps, (H, W),
                                   valid_hw=np.asarray(self.valid)[fo]).reshape(B, T, 3, H, W)
        self.cm = ops.make_centermaps(self.cc.reshape(n, 2), H, W, 3.0, device=dev).reshape(B, T, 1, H, W)
        self.heats, self.cell, self.hide = plan.clip(self.x, self.cm)
        self.flipped = plan.clip_flip_heatmaps(self.x, self.cm, pairs=PAIRS)


@functools.lru_cache(maxsize=None)
def frame_ctx(dev, **cfg):
    return FrameCtx(vc.ctx(dev, **cfg))


def _same(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bits_equal(host(got), host(ref)), what


def plan_heatmaps_case(f):
    c, plan = f.c, f.plan
    assert not bits_equal(host(f.x[0, 0]), host(f.x[-1, -1]))
    own = tuple(torch.full_like(t, SENT) for t in (f.heats, f.cell, f.hide))
    got = plan.clip_frame_heatmaps(f.frames, f.center, f.scale, out=own, **f.kw)
    assert all(g is o for g, o in zip(got, own))
    for g, r, n in zip(got, (f.heats, f.cell, f.hide), ("heat", "cell", "hide")):
        _same(g, r, n)
    # a centre of the centre map that differs between the frames changes the result: a constant one gives other maps, and so
    # does the same set of centres in another order (a batch-major / frame-major slip in the centre pool)
    const = plan.clip_frame_heatmaps(f.frames, f.center, f.scale, **dict(f.kw, crop_center=None))[0]
    assert not bits_equal(host(const), host(f.heats))
    default = ops.make_centermaps([[int(c.W / 2), int(c.H / 2)]] * (c.B * c.T), c.H, c.W, 3.0, device=c.dev).reshape(f.cm.shape)
    _same(const, plan.clip(f.x, default)[0], "the default crop_center is [int(W / 2), int(H / 2)]")
    swapped = plan.clip_frame_heatmaps(f.frames, f.center, f.scale, **dict(f.kw, crop_center=f.cc.reshape(-1, 2)[::-1].reshape(f.cc.shape)))[0]
    assert not bits_equal(host(swapped), host(f.heats))


def plan_flip_case(f):
    assert not bits_equal(host(f.flipped), host(f.heats))
    own = torch.full_like(f.flipped, SENT)
    got = f.plan.clip_frame_heatmaps(f.frames, f.center, f.scale, flip=True, pairs=PAIRS, out=own, **f.kw)
    assert got is own
    _same(got, f.flipped, "clip_frame_heatmaps(flip=True)")


def plan_final_case(f):
    c, plan, L = f.c, f.plan, _C.lib()
    B, T, K = c.B, c.T, c.K
    for flip in (False, True):
        pairs = PAIRS if flip else None
        ref = plan.clip_final_preds(f.x, f.cm, f.center, f.scale, flip=flip, pairs=pairs)
        got = plan.clip_frame_final_preds(f.frames, f.center, f.scale, flip=flip, pairs=pairs, **f.kw)
        for g, r, n in zip(got, ref, ("preds", "coords", "maxvals")):
            _same(g, r, (n, flip))
        assert not bits_equal(host(got[0]), host(got[1]))                           # the way back was taken
        # inv == NULL: preds = coords, as clip_final_preds(center=None) gives them
        ref = plan.clip_final_preds(f.x, f.cm, flip=flip, pairs=pairs)
        args, keep, _ = plan._frame_args("test", f.frames, f.center, f.scale, f.fo, f.rot, f.valid, (B, T))
        cc = torch.from_numpy(f.cc).to(c.dev)
        perm = ops._perm_array(c.perm, K + 1) if flip else None
        p2, c2, m2 = (torch.full_like(t, SENT) for t in ref)
        ws, nbytes = plan._frame_ws(5 if flip else 6)
        _C.check(L.up_unipose_lstm_clip_frame_final_preds(plan._plan, *args, cc.data_ptr(), 3.0, perm, None, c.w, c.h, p2.data_ptr(),
                                                          c2.data_ptr(), m2.data_ptr(), ws, nbytes, plan._stream()), "clip_frame_final_preds")
        for g, r, n in zip((p2, c2, m2), ref, ("preds", "coords", "maxvals")):
            _same(g, r, (n, flip, "inv == NULL"))
        del keep


def plan_stream_case(f):
    """three frames on two interleaved streams with separate state buffers, against stream's heat-maps through ops.final_preds"""
    c, plan = f.c, f.plan
    B, K, H, W, dev = c.B, c.K, c.H, c.W, c.dev
    rng = np.random.default_rng(37)
    streams = []
    for s in range(2):
        cen = np.array([[[28.0 + 4 * j + 2 * b + s, 20.0 + 2 * j - b - 3 * s] for b in range(B)] for j in range(3)])
        sc = np.array([[0.2 + 0.02 * j + 0.03 * b + 0.05 * s for b in range(B)] for j in range(3)])
        cc = np.array([[[W / 2 + j - b + 2 * s, H / 2 - 2 * j + b - s] for b in range(B)] for j in range(3)])
        fo = rng.integers(0, 3, (3, B))
        streams.append((cen, sc, cc, fo))

    def reference(s, j, state):
        cen, sc, cc, fo = (a[j] for a in streams[s])
        maps = protocol.crop_maps(cen, sc, [H, W], 0).reshape(B, 2, 3)
        x = ops.augment_image(f.frames[torch.from_numpy(fo).to(dev)], maps, (H, W), valid_hw=np.asarray(f.valid)[fo])
        cm = ops.make_centermaps(cc, H, W, 3.0, device=dev)
        heat = torch.empty((B, K + 1, c.h, c.w), device=dev)
        plan.stream(x, cm, state, first=j == 0, heat=heat)
        return ops.final_preds(heat, cen, sc, return_coords=True), heat

    ref_states = [plan.stream_state(), plan.stream_state()]
    refs = [[reference(s, j, ref_states[s]) for s in range(2)] for j in range(3)]
    states = [plan.stream_state(), plan.stream_state()]
    for j in range(3):
        for s in range(2):
            cen, sc, cc, fo = (a[j] for a in streams[s])
            heat = torch.full((B, K + 1, c.h, c.w), SENT, device=dev) if (j + s) % 2 == 0 else None
            got = plan.stream_frames(f.frames, cen, sc, states[s], first=j == 0, frame_of=fo, valid_hw=f.valid, crop_center=cc, heat=heat)
            assert len(got) == (3 if heat is None else 4)
            for g, r, n in zip(got, refs[j][s][0], ("preds", "coords", "maxvals")):
                _same(g, r, (n, j, s))
            if heat is not None:
                assert got[3] is heat
                _same(heat, refs[j][s][1], ("heat", j, s))
    for s in range(2):                              # the state is kept exactly as stream keeps it
        assert torch.equal(states[s].cpu(), ref_states[s].cpu())
    assert not torch.equal(states[0].cpu(), states[1].cpu())
    assert not bits_equal(host(refs[2][0][0][0]), host(refs[2][1][0][0]))


# ---- 5. workspaces and argument checks -----------------------------------------------------------------------------------------------
def plan_workspace_case(f):
    c, plan, L = f.c, f.plan, _C.lib()
    B, T, K, dev = c.B, c.T, c.K, c.dev
    needs = {k: L.up_unipose_lstm_plan_program_workspace(plan._plan, FROM_FRAMES + k) for k in range(-1, 11)}
    assert all((needs[k] > 0) == (k in (2, 4, 5, 6, 7, 8)) for k in needs), needs
    old = [L.up_unipose_lstm_plan_program_workspace(plan._plan, k) for k in range(9)]
    print("workspace from frames", needs, "existing programs", old)
    now = (L.up_unipose_lstm_plan_workspace(plan._plan), L.up_unipose_lstm_plan_flip_workspace(plan._plan))
    assert now == f.ws_before == (c.ws0, max(old[4], old[5])) and c.ws0 == max(old[k] for k in (0, 1, 2, 3, 6, 7, 8))
    # the C entries: one byte too few, then every refusal, on sentinel-filled outputs
    args, keep, _ = plan._frame_args("test", f.frames, f.center, f.scale, f.fo, f.rot, f.valid, (B, T))
    cen1, sc1 = f.center[:, 0], f.scale[:, 0]
    sargs, skeep, _ = plan._frame_args("test", f.frames, cen1, sc1, f.fo[:, 0], 0, f.valid)
    cc = torch.from_numpy(f.cc).to(dev)
    perm = ops._perm_array(c.perm, K + 1)
    bad_perm = ops._perm_array([K + 1] + list(range(1, K + 1)), K + 1)
    heat = torch.full_like(f.heats, SENT)
    st8 = torch.full_like(f.cell, SENT)
    p2 = torch.full((B, T, K + 1, 2), SENT, device=dev)
    m2 = torch.full((B, T, K + 1), SENT, device=dev)
    state = plan.stream_state()
    big = max(needs.values()) + 4096
    buf = torch.empty(big + 256, dtype=torch.uint8, device=dev)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    h_, p_, m_, s_, c_ = heat.data_ptr(), p2.data_ptr(), m2.data_ptr(), state.data_ptr(), cc.data_ptr()

    def heatmaps(a=args, cxy=c_, sigma=3.0, pm=None, out=h_, cell=None, hide=None, nbytes=big):
        return L.up_unipose_lstm_clip_frame_heatmaps(plan._plan, *a, cxy, sigma, pm, out, cell, hide, ws, nbytes, 0)

    def final(a=args, cxy=c_, sigma=3.0, pm=None, res=(c.w, c.h), preds=p_, mx=m_, nbytes=big):
        return L.up_unipose_lstm_clip_frame_final_preds(plan._plan, *a, cxy, sigma, pm, None, res[0], res[1], preds, None, mx, ws, nbytes, 0)

    def stream(a=sargs, cxy=c_, sigma=3.0, st=s_, first=1, res=(c.w, c.h), preds=p_, mx=m_, nbytes=big):
        return L.up_unipose_lstm_stream_frame_final_preds(plan._plan, *a, cxy, sigma, st, first, None, res[0], res[1], preds, None, mx, None,
                                                          ws, nbytes, 0)

    for call, k in ((lambda n: heatmaps(nbytes=n), 2), (lambda n: heatmaps(pm=perm, nbytes=n), 4), (lambda n: final(pm=perm, nbytes=n), 5),
                    (lambda n: final(nbytes=n), 6), (lambda n: stream(nbytes=n), 7), (lambda n: stream(first=0, nbytes=n), 8)):
        assert call(needs[k] - 1) != 0 and b"workspace" in L.up_last_error(), k
    no_fo = list(args)
    no_fo[5] = None                                 # frame_of == NULL: F = 3 is not B * T ...
    s_no_fo = list(sargs)
    s_no_fo[2], s_no_fo[5] = B + 1, None            # ... resp. not B
    nul = lambda a, i: [None if j == i else v for j, v in enumerate(a)]          # noqa: E731
    calls = (
        lambda: heatmaps(pm=bad_perm), lambda: final(pm=bad_perm),                                     # perm out of range
        lambda: final(res=(0, c.h)), lambda: final(res=(c.w, -1)), lambda: stream(res=(0, c.h)),       # res <= 0
        lambda: stream(st=None), lambda: stream(st=s_ + 64), lambda: stream(st=None, first=0),         # NULL or misaligned state
        lambda: heatmaps(pm=perm, cell=st8.data_ptr()), lambda: heatmaps(pm=perm, hide=st8.data_ptr()),      # a state with the flip test
        lambda: heatmaps(sigma=0.0), lambda: heatmaps(sigma=-3.0), lambda: heatmaps(sigma=float("nan")),
        lambda: final(sigma=0.0), lambda: stream(sigma=0.0), lambda: stream(sigma=float("nan")),
        lambda: heatmaps(a=no_fo), lambda: final(a=no_fo), lambda: stream(a=s_no_fo),                  # frame_of == NULL with F != samples
        lambda: heatmaps(cxy=None), lambda: final(cxy=None), lambda: stream(cxy=None),                 # null required pointers
        lambda: heatmaps(out=None), lambda: final(preds=None), lambda: final(mx=None), lambda: stream(preds=None),
        lambda: heatmaps(a=nul(args, 0)), lambda: heatmaps(a=nul(args, 7)), lambda: stream(a=nul(sargs, 0)),
        lambda: heatmaps(a=[2 if j == 1 else v for j, v in enumerate(args)]),                           # what the crop refuses
        lambda: final(a=[0.0 if j == 10 else v for j, v in enumerate(args)]),
        lambda: stream(a=[0 if j == 3 else v for j, v in enumerate(sargs)]),
    )
    for i, call in enumerate(calls):
        assert call() == -1, i
    assert (host(heat) == SENT).all() and (host(st8) == SENT).all() and (host(p2) == SENT).all() and (host(m2) == SENT).all()
    assert not state.any()
    del keep, skeep


def plan_unset_case(dev):
    """an entry from frames of a plan whose weights were never set: refused ("never set")"""
    from unipose_amd.plan import _LstmConfig
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(1, 2, 32, 32, 16, 13)), C.byref(plan)) == 0
    buf = torch.zeros(1 << 16).to(dev)
    p = buf.data_ptr() + (-buf.data_ptr()) % 256
    perm = ops._perm_array(list(range(14)), 14)
    big = 1 << 40
    src = (p, U8, 2, 4, 4, None, None, p, 128.0, 128.0, 256.0)
    one = (p, U8, 1, 4, 4, None, None, p, 128.0, 128.0, 256.0)
    for call in (lambda: L.up_unipose_lstm_clip_frame_heatmaps(plan, *src, p, 3.0, None, p, None, None, p, big, 0),
                 lambda: L.up_unipose_lstm_clip_frame_heatmaps(plan, *src, p, 3.0, perm, p, None, None, p, big, 0),
                 lambda: L.up_unipose_lstm_clip_frame_final_preds(plan, *src, p, 3.0, perm, None, 4, 4, p, None, p, p, big, 0),
                 lambda: L.up_unipose_lstm_clip_frame_final_preds(plan, *src, p, 3.0, None, None, 4, 4, p, None, p, p, big, 0),
                 lambda: L.up_unipose_lstm_stream_frame_final_preds(plan, *one, p, 3.0, p, 1, None, 4, 4, p, None, p, None, p, big, 0),
                 lambda: L.up_unipose_lstm_stream_frame_final_preds(plan, *one, p, 3.0, p, 0, None, 4, 4, p, None, p, None, p, big, 0)):
        assert call() != 0
        assert b"never set" in L.up_last_error(), L.up_last_error()
    assert not buf.any()
    L.up_unipose_lstm_plan_destroy(plan)


def plan_argument_case(f):
    """argument checks of the new methods: ValueError before any launch"""
    c, plan = f.c, f.plan
    B, T, K, dev = c.B, c.T, c.K, c.dev
    fr, cen, sc = f.frames, f.center, f.scale
    state = plan.stream_state()
    bad_calls = [
        lambda: plan.clip_frame_heatmaps(fr.float().permute(0, 3, 1, 2), cen, sc, **f.kw),                  # NCHW frames
        lambda: plan.clip_frame_heatmaps(fr, cen.reshape(B * T, 2), sc.reshape(B * T), **f.kw),              # one crop per (b, t)
        lambda: plan.clip_frame_heatmaps(fr, cen, None, **f.kw),
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, **dict(f.kw, frame_of=f.fo.reshape(-1))),
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, **dict(f.kw, frame_of=None)),                          # F = 3 is not B * T
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, **dict(f.kw, valid_hw=f.valid[:2])),
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, **dict(f.kw, crop_center=np.zeros((B, T + 1, 2)))),
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, flip=True, **f.kw),                                    # no pairs
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, out=(torch.empty_like(f.heats),) * 2, **f.kw),
        lambda: plan.clip_frame_heatmaps(fr, cen, sc, flip=True, pairs=PAIRS, out=torch.empty_like(f.cell), **f.kw),
        lambda: plan.clip_frame_final_preds(fr, cen, sc, res=[0, 4], **f.kw),
        lambda: plan.clip_frame_final_preds(fr, cen, sc, flip=True, **f.kw),
        lambda: plan.clip_frame_final_preds(fr, cen, sc, out=(torch.empty(B, T, K + 1, 2, device=dev),) * 2, **f.kw),
        lambda: plan.stream_frames(fr, cen[:, 0], sc[:, 0], None, first=True, frame_of=f.fo[:, 0]),
        lambda: plan.stream_frames(fr, cen[:, 0], sc[:, 0], state[:-1], first=True, frame_of=f.fo[:, 0]),
        lambda: plan.stream_frames(fr, cen[:, 0], sc[:, 0], state, first=True, frame_of=f.fo),
        lambda: plan.stream_frames(fr, cen[:, 0], sc[:, 0], state, first=True, frame_of=f.fo[:, 0], crop_center=np.zeros((B + 1, 2))),
        lambda: plan.stream_frames(fr, cen[:, 0], sc[:, 0], state, first=True, frame_of=f.fo[:, 0],
                                   heat=torch.empty(B, K + 1, c.h + 1, c.w, device=dev)),
    ]
    for i, call in enumerate(bad_calls):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(f"bad call {i} was not refused")
    assert not state.any()
