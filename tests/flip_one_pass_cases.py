"""The flip test in ONE trunk pass over 2 B images (UP_PLAN_FLIP_ONE_PASS; up_unipose_plan_create_ex / up_unipose_lstm_plan_create_ex,
the _strided clip kernels, up_clip_flip_merge; UniPosePlan / UniPoseLSTMPlan with flip="one_pass"): shared by
test_flip_one_pass_emu.py and test_flip_one_pass_gpu.py.

Yardsticks.  A _strided kernel is its neighbour writing other images: equal bits to the neighbour, image by image, and sentinels
everywhere else.  up_clip_flip_merge is up_flip_merge's arithmetic: numpy float32 (protocol_cases.merge_ref).  A flagged plan's flip
programs are DEFINED by an unflagged plan of batch 2 B on cat(x, mirror(x)), merged by ops.flip_merge: equal bits.  Every other
program of a flagged plan equals the unflagged plan's, bits and workspace figures.  Whether the one-pass and the two-pass maps have
equal bits is NOT asserted either way: a convolution picks its kernel by its row count.  The only tolerances are the project's own
bars against the float64 evaluation of the network (fp32 storage): 2e-5 for the image plan (G1), 1e-3 for the video plan's frames
(model_cases, G5); the two-pass figure is printed beside each."""
import ctypes as C
import functools

import numpy as np
import torch

from oracle import unipose_oracle as O
from unipose_amd import _C, ops, protocol

import frame_cases as fc
import lstm_plan_cases as lc
import protocol_cases as pc
import video_eval_cases as vc
from protocol_cases import SENT, bits_equal, host

F32 = np.float32
FROM_FRAMES = _C.PROGRAM_FROM_FRAMES
ONE_PASS = _C.PLAN_FLIP_ONE_PASS
PAIRS = vc.PAIRS
BT = [(1, 1), (2, 3), (3, 2)]


def _st(t):
    return ops._stream(t)


# ---- 1. the _strided clip kernels ---------------------------------------------------------------------------------------------------------
def strided_check(dev, image_shape, bt, plain, strided, alloc, what):
    """plain(out): the neighbour into out (T * B, *image_shape); strided(out, frame_images, first): the _strided entry into out
    (T * frame_images, *image_shape).  Every buffer starts as sentinels; with `alloc` (the emulator) each ends right before an
    inaccessible page."""
    B, T = bt
    ref = vc._dev_tensor(dev, (T * B,) + image_shape, alloc)
    plain(ref)
    r = host(ref)
    assert (r != SENT).any(), (what, "the neighbour wrote nothing")
    # frame_images = B, first = 0: the neighbour itself
    got = vc._dev_tensor(dev, (T * B,) + image_shape, alloc)
    strided(got, B, 0)
    assert bits_equal(host(got), r), (what, "frame_images = B")
    # the two halves of frames of 2 B images, one launch each into one buffer
    both = vc._dev_tensor(dev, (T * 2 * B,) + image_shape, alloc)
    strided(both, 2 * B, 0)
    g = host(both).reshape((T, 2, B) + image_shape)
    assert bits_equal(g[:, 0].reshape(r.shape), r) and (g[:, 1] == SENT).all(), (what, "first = 0")
    strided(both, 2 * B, B)
    g = host(both).reshape((T, 2, B) + image_shape)
    assert bits_equal(g[:, 0].reshape(r.shape), r) and bits_equal(g[:, 1].reshape(r.shape), r), (what, "first = B")
    # frames of 2 B + 1 images from image 1 on: images 0 and B + 1 .. 2 B of every frame are never addressed
    odd = vc._dev_tensor(dev, (T * (2 * B + 1),) + image_shape, alloc)
    strided(odd, 2 * B + 1, 1)
    g = host(odd).reshape((T, 2 * B + 1) + image_shape)
    assert bits_equal(g[:, 1:B + 1].reshape(r.shape), r), (what, "first = 1")
    assert (g[:, 0] == SENT).all() and (g[:, B + 1:] == SENT).all(), (what, "an image that is not addressed was written")


LAYOUT_CASES = [(bt, hw) for bt in BT for hw in ((3, 1), (2, 7), (5, 65))]


def layout_strided_case(dev, bt, hw, alloc=None):
    L = _C.lib()
    (B, T), (H, W), Cc, ld = bt, hw, 3, 4
    rng = np.random.default_rng(7 + 100 * B + 10 * T + W)
    x = torch.from_numpy(rng.standard_normal((B, T, Cc, H, W)).astype(F32)).to(dev)
    for name, near, far in (("plain", L.up_clip_nchw_to_nhwc, L.up_clip_nchw_to_nhwc_strided),
                            ("flip", L.up_clip_nchw_to_nhwc_flip, L.up_clip_nchw_to_nhwc_flip_strided)):
        strided_check(dev, (H, W, ld), bt,
                      lambda o: _C.check(near(x.data_ptr(), o.data_ptr(), B, T, Cc, H, W, ld, _st(x)), name),
                      lambda o, fi, first: _C.check(far(x.data_ptr(), o.data_ptr(), B, T, Cc, H, W, ld, fi, first, _st(x)), name),
                      alloc, ("layout", name, bt, hw))


POOL_CASES = [(bt, hw, coff) for bt in BT for hw in ((7, 7), (8, 16), (15, 23), (16, 24)) for coff in (14, 15)]


def pool_strided_case(dev, bt, hw, coff, alloc=None):
    L = _C.lib()
    (B, T), (H, W), ld = bt, hw, 16
    P, Q = (H - 7) // 8 + 1, (W - 7) // 8 + 1
    cm = torch.from_numpy(vc.pool_input(bt, hw)).to(dev)
    for name, near, far in (("plain", L.up_clip_avgpool9s8_fwd, L.up_clip_avgpool9s8_fwd_strided),
                            ("flip", L.up_clip_avgpool9s8_flip_fwd, L.up_clip_avgpool9s8_flip_fwd_strided)):
        strided_check(dev, (P, Q, ld), bt,
                      lambda o: _C.check(near(cm.data_ptr(), o.data_ptr(), ld, coff, B, T, H, W, P, Q, _st(cm)), name),
                      lambda o, fi, first: _C.check(far(cm.data_ptr(), o.data_ptr(), ld, coff, B, T, H, W, P, Q, fi, first, _st(cm)), name),
                      alloc, ("pool", name, bt, hw, coff))


CENTER_CASES = [(bt, hw, sigma) for bt in BT for hw in ((7, 7), (16, 24)) for sigma in (0.5, 3.0)]


def center_pool_strided_case(dev, bt, hw, sigma, alloc=None):
    import video_frame_cases as vf
    L = _C.lib()
    (B, T), (H, W), ld, coff = bt, hw, 16, 14 + (bt[0] + hw[0]) % 2
    P, Q = (H - 7) // 8 + 1, (W - 7) // 8 + 1
    cen = vf.centers_for((H, W), B * T, 3 * B + T)
    cxy = torch.from_numpy(cen).to(dev)
    for name, near, far in (("plain", L.up_clip_center_pool, L.up_clip_center_pool_strided),
                            ("flip", L.up_clip_center_pool_flip, L.up_clip_center_pool_flip_strided)):
        strided_check(dev, (P, Q, ld), bt,
                      lambda o: _C.check(near(cxy.data_ptr(), sigma, o.data_ptr(), ld, coff, B, T, H, W, P, Q, _st(o)), name),
                      lambda o, fi, first: _C.check(far(cxy.data_ptr(), sigma, o.data_ptr(), ld, coff, B, T, H, W, P, Q, fi, first, _st(o)),
                                                    name),
                      alloc, ("center_pool", name, bt, hw, sigma))
    # ops.center_pool(frame_images=...) is the same entries
    out = vc._dev_tensor(dev, (T * 2 * B, P, Q, ld))
    ref = vc._dev_tensor(dev, (T * B, P, Q, ld))
    ops.center_pool(cen.reshape(B, T, 2), (H, W), sigma, out=ref, coff=coff, clip=(B, T), flip=True)
    assert ops.center_pool(cen.reshape(B, T, 2), (H, W), sigma, out=out, coff=coff, clip=(B, T), flip=True, frame_images=2 * B, first=B) is out
    assert bits_equal(host(out).reshape(T, 2, B, P, Q, ld)[:, 1].reshape(T * B, P, Q, ld), host(ref))


CROP_CASES = [(bt, typ) for bt in BT for typ in ("u8", "f32")]


def crop_strided_case(dev, bt, typ, alloc=None):
    """sources 1 x 1 and 20 x 12, outputs 1 x 1 and 33 x 65, either or both outputs; the two outputs share frame_images / first"""
    import video_frame_cases as vf
    L = _C.lib()
    B, T = bt
    n, ld = B * T, 4
    for src_hw in ((1, 1), (20, 12)):
        for out_hw in ((1, 1), (33, 65)):
            frames = fc.pixels_of((5, B, T, src_hw[0]), (2,) + src_hw + (3,), typ)
            s = fc._place(frames, dev, None)
            inv = torch.from_numpy(np.ascontiguousarray(vf.clip_maps_for(src_hw, out_hw, n, B + T), dtype=np.float64)).to(dev)
            fo = torch.tensor([(i + 1) % 2 for i in range(n)], dtype=torch.int32).reshape(B, T).to(dev)
            head = (s.data_ptr(), fc.U8 if s.dtype == torch.uint8 else fc.PF32, 2, src_hw[0], src_hw[1], 3, fo.data_ptr(), None,
                    inv.data_ptr(), B, T, 100.0, 128.0, 256.0)
            tail = (out_hw[0], out_hw[1], ld)
            for which in ("y", "flip", "both"):
                # one output at a time through strided_check (the other NULL where only one is asked for; where both are, the other
                # output goes to a scratch tensor of the same frames and is compared below)
                for side in ("y", "flip") if which == "both" else (which,):
                    def plain(o, side=side):
                        other = vc._dev_tensor(dev, tuple(o.shape)) if which == "both" else None
                        y, yf = (o, other) if side == "y" else (other, o)
                        _C.check(L.up_clip_crop_to_nhwc(*head, fc_ptr(y), fc_ptr(yf), *tail, _st(s)), "clip_crop_to_nhwc")

                    def strided(o, fi, first, side=side):
                        other = vc._dev_tensor(dev, tuple(o.shape)) if which == "both" else None
                        y, yf = (o, other) if side == "y" else (other, o)
                        _C.check(L.up_clip_crop_to_nhwc_strided(*head, fc_ptr(y), fc_ptr(yf), *tail, fi, first, _st(s)),
                                 "clip_crop_to_nhwc_strided")
                    strided_check(dev, out_hw + (ld,), bt, plain, strided, alloc, ("crop", bt, typ, src_hw, out_hw, which, side))
            # the plan's use: ONE launch, y the first and y_flip the second half of every frame of one tensor
            image = out_hw[0] * out_hw[1] * ld
            one = vc._dev_tensor(dev, (T * 2 * B,) + out_hw + (ld,), alloc)
            y = vc._dev_tensor(dev, (T * B,) + out_hw + (ld,))
            yf = vc._dev_tensor(dev, (T * B,) + out_hw + (ld,))
            _C.check(L.up_clip_crop_to_nhwc(*head, y.data_ptr(), yf.data_ptr(), *tail, _st(s)), "clip_crop_to_nhwc")
            _C.check(L.up_clip_crop_to_nhwc_strided(*head, one.data_ptr(), one.data_ptr() + 4 * B * image, *tail, 2 * B, 0, _st(s)),
                     "clip_crop_to_nhwc_strided")
            g = host(one).reshape((T, 2, B) + out_hw + (ld,))
            assert bits_equal(g[:, 0].reshape(host(y).shape), host(y)) and bits_equal(g[:, 1].reshape(host(y).shape), host(yf)), (bt, typ)
            if out_hw[1] > 1 and src_hw[0] > 1:
                assert not bits_equal(host(y), host(yf))
    # ops.clip_crop_to_nhwc_strided is the same entry
    one2 = vc._dev_tensor(dev, (T * 2 * B,) + out_hw + (ld,))
    a, b = ops.clip_crop_to_nhwc_strided(s, inv.reshape(B, T, 6), out_hw, (B, T), 2 * B, 0, out=one2, out_flip=None, frame_of=fo, border=100.0)
    assert a is one2 and b is None
    assert bits_equal(host(one2).reshape((T, 2, B) + out_hw + (ld,))[:, 0], g[:, 0])


def fc_ptr(t):
    return None if t is None else t.data_ptr()


def strided_refusal_case(dev):
    """every _strided entry: its own refusals and its neighbour's, nothing written"""
    L = _C.lib()
    buf = torch.full((1 << 14,), SENT).to(dev)
    out = torch.full((1 << 14,), SENT).to(dev)
    cen = torch.zeros(64, dtype=torch.float64).to(dev)
    inv = torch.zeros(64, dtype=torch.float64).to(dev)
    p, q = buf.data_ptr(), out.data_ptr()
    own = (dict(first=-1), dict(fi=1), dict(fi=3, first=2), dict(fi=2, first=1), dict(fi=1 << 30), dict(fi=(1 << 31) - 1, first=0))

    def refused(fn, names, ok, bads):
        assert fn(*ok) == 0, (fn, _C.lib().up_last_error())
        out.fill_(SENT)
        for bad in own + tuple(bads):
            a = dict(zip(names, ok))
            a.update(bad)
            assert fn(*[a[n] for n in names]) == -1, bad
        assert (host(out) == SENT).all()
    lay = ("x", "y", "B", "T", "C", "H", "W", "ld", "fi", "first", "st")
    for fn in (L.up_clip_nchw_to_nhwc_strided, L.up_clip_nchw_to_nhwc_flip_strided):
        refused(fn, lay, (p, q, 2, 2, 3, 2, 3, 4, 4, 1, 0),
                (dict(x=None), dict(y=None), dict(B=0), dict(T=0), dict(C=0), dict(H=0), dict(W=-1), dict(ld=2), dict(ld=6), dict(y=q + 4)))
    pool = ("x", "y", "ld", "coff", "B", "T", "H", "W", "P", "Q", "fi", "first", "st")
    for fn in (L.up_clip_avgpool9s8_fwd_strided, L.up_clip_avgpool9s8_flip_fwd_strided):
        refused(fn, pool, (p, q, 4, 3, 2, 2, 8, 16, 1, 2, 4, 1, 0),
                (dict(x=None), dict(y=None), dict(ld=0), dict(coff=-1), dict(coff=4), dict(B=0), dict(T=0), dict(H=0), dict(W=0), dict(P=2),
                 dict(Q=1)))
    cp = ("c", "sigma", "y", "ld", "coff", "B", "T", "H", "W", "P", "Q", "fi", "first", "st")
    for fn in (L.up_clip_center_pool_strided, L.up_clip_center_pool_flip_strided):
        refused(fn, cp, (cen.data_ptr(), 3.0, q, 4, 3, 2, 2, 8, 16, 1, 2, 4, 1, 0),
                (dict(c=None), dict(y=None), dict(sigma=0.0), dict(sigma=float("nan")), dict(ld=0), dict(coff=4), dict(B=0), dict(T=0),
                 dict(H=0), dict(P=2), dict(Q=1)))
    crop = ("src", "typ", "F", "Hs", "Ws", "C", "fo", "valid", "inv", "B", "T", "border", "mean", "std", "y", "yf", "Ho", "Wo", "ld", "fi",
            "first", "st")
    refused(L.up_clip_crop_to_nhwc_strided, crop,
            (p, fc.PF32, 4, 2, 2, 3, None, None, inv.data_ptr(), 2, 2, 128.0, 128.0, 256.0, q, q + 4096, 2, 3, 4, 4, 1, 0),
            (dict(src=None), dict(inv=None), dict(y=None, yf=None), dict(yf=q), dict(typ=2), dict(F=0), dict(F=3), dict(B=0), dict(T=0),
             dict(Hs=0), dict(Wo=0), dict(C=5), dict(ld=6), dict(y=q + 4), dict(std=0.0)))


# ---- 2. up_clip_flip_merge ------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 3, 2), (3, 2, 16, 2, 65), (2, 2, 5, 4, 65), (1, 2, 16, 3, 2), (2, 1, 1, 2, 64)]      # T, B, J, H, W


def clip_merge_case(dev, alloc=None):
    L = _C.lib()
    rng = np.random.default_rng(23)
    for T, B, J, H, W in MERGE_SHAPES:
        ld = (J + 3) // 4 * 4 + 4
        image = H * W * ld
        perms = [("identity", list(range(J)))] + ([("3-cycle", pc.cycle(J))] if J >= 3 else [])
        for name, perm in perms:
            x = rng.standard_normal((T, 2, B, J, H, W)).astype(F32)
            a, f = x[:, 0].reshape(T * B, J, H, W), x[:, 1].reshape(T * B, J, H, W)          # views: the specials land in x
            a[0, 0, 0, 0], f[0, perm[0], 0, W - 1] = np.inf, -np.inf                          # inf + -inf: a NaN, at that place
            a[-1, J - 1, H - 1, 0] = np.nan
            if a.size > 1:
                a[-1, J - 1, H - 1, W - 1], f[-1, perm[J - 1], H - 1, 0] = np.inf, np.inf
            x = np.ascontiguousarray(np.stack([a.reshape(T, B, J, H, W), f.reshape(T, B, J, H, W)], 1))
            a, f = x[:, 0].reshape(T * B, J, H, W), x[:, 1].reshape(T * B, J, H, W)
            ref = pc.merge_ref(a, f, perm)
            assert np.isnan(ref[0, 0, 0, 0]) and np.isnan(ref[-1, J - 1, H - 1, 0])
            assert a.size == 1 or np.isposinf(ref[-1, J - 1, H - 1, W - 1])
            # interleaved NHWC input (T, 2 B, H, W, ld), pad lanes NaN; compact outputs, NHWC (pad lanes keep the sentinel) and NCHW
            xin = torch.full((T, 2 * B, H, W, ld), float("nan"))
            xin[..., :J] = torch.from_numpy(x.reshape(T, 2 * B, J, H, W)).permute(0, 1, 3, 4, 2)
            xin = xin.to(dev)
            pa = ops._perm_array(perm, J)
            for lout in ("nhwc", "nchw"):
                out = vc._dev_tensor(dev, (T * B, H, W, ld) if lout == "nhwc" else (T * B, J, H, W), alloc)
                so = (B * image, image, 1, ld) if lout == "nhwc" else (B * J * H * W, J * H * W, H * W, 1)
                _C.check(L.up_clip_flip_merge(xin.data_ptr(), xin.data_ptr() + 4 * B * image, 2 * B * image, image, 1, ld, B, T, J, H, W,
                                              pa, out.data_ptr(), *so, _st(xin)), "clip_flip_merge")
                o = host(out)
                if lout == "nhwc":
                    assert (o[..., J:] == SENT).all(), "a pad lane of `out` was written"
                    o = o[..., :J].transpose(0, 3, 1, 2)
                assert bits_equal(o, ref), (T, B, J, H, W, name, lout)
            # one-level strides: up_flip_merge of T * B images
            ta, tf = torch.from_numpy(np.array(a)).to(dev), torch.from_numpy(np.array(f)).to(dev)
            s = (J * H * W, H * W, 1)
            one, two = vc._dev_tensor(dev, a.shape), vc._dev_tensor(dev, a.shape)
            _C.check(L.up_flip_merge(ta.data_ptr(), tf.data_ptr(), *s, T * B, J, H, W, pa, one.data_ptr(), *s, _st(ta)), "flip_merge")
            _C.check(L.up_clip_flip_merge(ta.data_ptr(), tf.data_ptr(), B * s[0], *s, B, T, J, H, W, pa, two.data_ptr(), B * s[0], *s,
                                          _st(ta)), "clip_flip_merge")
            assert bits_equal(host(one), host(two)) and bits_equal(host(one), ref)
            # ops.clip_flip_merge: NCHW (T, 2 B, J, H, W)
            got = ops.clip_flip_merge(torch.from_numpy(x.reshape(T, 2 * B, J, H, W)).to(dev), perm)
            assert bits_equal(host(got).reshape(ref.shape), ref)


def clip_merge_refusal_case(dev):
    L = _C.lib()
    buf = torch.full((1 << 16,), SENT).to(dev)
    p, q, o = buf.data_ptr(), buf.data_ptr() + 4 * (1 << 13), buf.data_ptr() + 4 * (1 << 15)
    names = ("a", "f", "ist", "isb", "isj", "isp", "B", "T", "J", "H", "W", "perm", "out", "ost", "osb", "osj", "osp", "stream")

    def call(J=4, perm_list=None, **kw):
        a = dict(zip(names, (p, q, 2 * J * 6, J * 6, 6, 1, 2, 2, J, 2, 3, ops._perm_array(perm_list if perm_list is not None else list(range(J)), J),
                             o, 2 * J * 6, J * 6, 6, 1, 0)))
        a.update(kw)
        return L.up_clip_flip_merge(*[a[n] for n in names])
    assert call() == 0
    buf.fill_(SENT)
    assert call(out=q) == -1 and b"out == f" in L.up_last_error()
    assert call(perm_list=[0, 1, 2, 4]) == -1 and b"perm[3]" in L.up_last_error()
    assert call(perm_list=[0, -1, 2, 3]) == -1
    assert call(J=257) == -2
    assert call(out=p, ost=96) == -1 and b"out == a" in L.up_last_error()           # out == a with another frame stride
    for bad in (dict(a=None), dict(f=None), dict(out=None), dict(perm=None), dict(B=0), dict(T=0), dict(H=0), dict(W=-1), dict(ist=0),
                dict(isb=0), dict(isj=-1), dict(isp=0), dict(ost=0), dict(osb=0), dict(osj=0), dict(osp=-2), dict(ist=1 << 31),
                dict(ist=1 << 30, T=3), dict(ost=1 << 30, T=3), dict(isb=1 << 31, B=2), dict(osp=1 << 30)):
        assert call(**bad) == -1, bad
    assert (host(buf) == SENT).all()


# ---- 3. the plans: what the image and the video cases share ---------------------------------------------------------------------------
def _aligned(t):
    return t.data_ptr() + (-t.data_ptr()) % 256


def _ff_workspace(dev, need):
    """a workspace of exactly `need` bytes, every byte 0xFF (NaNs wherever a program reads before it writes)"""
    buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev)
    return buf, _aligned(buf)


def _same(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bits_equal(host(got), host(ref)), what


def _same_all(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        if g.dtype == torch.float32:
            _same(g, r, (what, i))
        else:
            assert torch.equal(g.cpu(), r.cpu()), (what, i)


def create_case(dev):
    """create-time checks of both plans: an unknown flag bit and a NULL argument are refused with *plan untouched; _flags reads back"""
    from unipose_amd.plan import _Config, _LstmConfig
    L = _C.lib()
    for create, flags, destroy, cfg in ((L.up_unipose_plan_create_ex, L.up_unipose_plan_flags, L.up_unipose_plan_destroy, _Config(1, 32, 32, 16, 15)),
                                        (L.up_unipose_lstm_plan_create_ex, L.up_unipose_lstm_plan_flags, L.up_unipose_lstm_plan_destroy,
                                         _LstmConfig(1, 2, 32, 32, 16, 13))):
        mark = 0x5A5A5A5A
        for bad in (2, 3, 4, -1, 1 << 16):
            plan = C.c_void_p(mark)
            assert create(C.byref(cfg), 0, bad, C.byref(plan)) == -1 and b"flags" in L.up_last_error(), bad
            assert plan.value == mark
        plan = C.c_void_p(mark)
        assert create(None, 0, ONE_PASS, C.byref(plan)) == -1 and plan.value == mark
        assert create(C.byref(cfg), 0, ONE_PASS, None) == -1
        assert create(C.byref(cfg), 2, ONE_PASS, C.byref(plan)) == -1 and plan.value == mark           # an unknown storage type
        assert flags(None) == -1
        for dt in (0, 1):
            for fl in (0, ONE_PASS):
                plan = C.c_void_p()
                assert create(C.byref(cfg), dt, fl, C.byref(plan)) == 0
                assert flags(plan) == fl
                destroy(plan)


def _raw(cls, prefix, model, cfg, dtype, flags, via_t):
    """a plan object around up_*_plan_create_t (via_t) or up_*_plan_create_ex, its weights set as the class sets them"""
    from unipose_amd import plan as P
    from unipose_amd.checkpoint import fold_batchnorm
    L = _C.lib()
    p = cls.__new__(cls)
    p._plan, p.device, p.workspace, p.cfg = C.c_void_p(), model.backbone.conv1.weight.device, None, cfg
    if via_t:
        _C.check(getattr(L, prefix + "_create_t")(C.byref(cfg), dtype, C.byref(p._plan)), "create_t")
    else:
        _C.check(getattr(L, prefix + "_create_ex")(C.byref(cfg), dtype, flags, C.byref(p._plan)), "create_ex")
    P._set_convs(p, prefix, fold_batchnorm(model))
    return p


# ---- 4. the image plan, flagged -------------------------------------------------------------------------------------------------------------
IMAGE_CASES = [dict(K=14, B=1, height=64, width=64), dict(K=14, B=2, height=52, width=68),
               dict(K=16, B=2, height=48, width=48, output_stride=8, bbox=True, dataset="MPII")]
IMAGE_STORAGES = [("f32", 0), ("bf16", 0), ("f32", 1), ("f32", 2)]          # (storage, index into IMAGE_CASES)
IMAGE_FLIP_ROWS = (4, 5, FROM_FRAMES + 4, FROM_FRAMES + 5)
IMAGE_PLAIN_ROWS = (0, 1, 2, 3, 6, FROM_FRAMES + 0, FROM_FRAMES + 6)


class ImageCtx:
    """One model, its three plans — unflagged, flagged, unflagged at batch 2 B — the inputs and the oracle's results: computed once per
    configuration and shared, unchanged, by the tests."""

    def __init__(self, dev, storage, K=14, B=1, height=64, width=64, output_stride=16, bbox=False, dataset="LSP"):
        from unipose_amd.plan import UniPosePlan
        self.dev, self.storage, self.K, self.B, self.H, self.W, self.bbox, self.dataset = dev, storage, K, B, height, width, bbox, dataset
        self.output_stride = output_stride
        self.model = m = pc._model(dev, K, output_stride, bbox)
        self.x = O.synth_input((B, 3, height, width), 5).to(dev)
        self.two = UniPosePlan(m, B, height, width, storage=storage)
        self.one = UniPosePlan(m, B, height, width, storage=storage, flip="one_pass")
        self.big = UniPosePlan(m, 2 * B, height, width, storage=storage)
        self.perm = protocol.flip_perm(dataset, K, bbox)
        self.C = self.one.out_channels
        maps = lambda plan, t: torch.cat(plan(t), 1) if bbox else plan(t)       # noqa: E731
        self.maps = maps
        xx = torch.cat([self.x, torch.flip(self.x, [3])]).contiguous()
        both = maps(self.big, xx)
        self.a, self.f = both[:B].contiguous(), both[B:].contiguous()
        self.merged = ops.flip_merge(self.a, self.f, self.perm)                  # the oracle of the one-pass form
        self.two_pass = ops.flip_merge(maps(self.two, self.x), maps(self.two, torch.flip(self.x, [3]).contiguous()), self.perm)
        self.cen = np.stack([np.array([width / 2.0 + 3 * i, height / 2.0 - 2 * i]) for i in range(B)])
        self.sc = np.array([max(height, width) / 200.0 * (1 + 0.1 * i) for i in range(B)])
        self.frames = torch.from_numpy(fc.pixels_of((8, K), (3, 40, 56, 3), "u8")).to(dev)
        self.fcen = np.stack([np.array([28.0 + 5 * i, 20.0 - 3 * i]) for i in range(B)])
        self.fsc = np.array([0.25 * (1 + 0.3 * i) for i in range(B)])


@functools.lru_cache(maxsize=None)
def image_ctx(dev, storage, index):
    return ImageCtx(dev, storage, **IMAGE_CASES[index])


def _need(c_plan, k, prefix="up_unipose_plan"):
    return getattr(_C.lib(), prefix + "_program_workspace")(c_plan._plan, k)


def image_plain_rows_case(c):
    """every program without the flip test: the unflagged plan's figures and bits"""
    L = _C.lib()
    one, two, B, dev = c.one, c.two, c.B, c.dev
    assert L.up_unipose_plan_flags(one._plan) == ONE_PASS and L.up_unipose_plan_flags(two._plan) == 0
    assert one.flip_mode == "one_pass" and two.flip_mode == "two_pass"
    assert L.up_unipose_plan_dtype(one._plan) == L.up_unipose_plan_dtype(two._plan) == (1 if c.storage == "bf16" else 0)
    for k in IMAGE_PLAIN_ROWS:
        assert _need(one, k) == _need(two, k) > 0, k
    for k in (7, FROM_FRAMES + 1, FROM_FRAMES + 7, -1):
        assert _need(one, k) == 0, k
    assert L.up_unipose_plan_workspace(one._plan) == L.up_unipose_plan_workspace(two._plan) == max(_need(two, k) for k in range(4))
    assert L.up_unipose_plan_flip_workspace(one._plan) == max(_need(one, k) for k in (4, 5, 6))
    _same(c.maps(one, c.x), c.maps(two, c.x), "program 0")
    up = [torch.full((B, c.C, c.H, c.W), SENT, device=dev) for _ in range(2)]
    for plan, out in zip((one, two), up):                                          # program 1 through the C entry (the model has stride 8)
        ws, nbytes = plan._ws()
        _C.check(L.up_unipose_forward_upsampled(plan._plan, c.x.data_ptr(), out.data_ptr(), ws, nbytes, plan._stream()), "upsampled")
    _same(up[0], up[1], "program 1")
    _same_all(one.keypoints(c.x), two.keypoints(c.x), "program 2")
    if c.bbox:
        (k1, n1, s1), (k2, n2, s2) = ([host(t) for t in p.persons(c.x, c.dataset)] for p in (one, two))      # program 3
        assert np.array_equal(n1, n2) and np.array_equal(s1, s2)
        for b in range(B):                                                         # (rows beyond the count are not written)
            assert np.array_equal(k1[b, :min(n1[b], k1.shape[1])], k2[b, :min(n2[b], k2.shape[1])]), ("program 3", b)
    _same_all(one.final_preds(c.x, c.cen, c.sc), two.final_preds(c.x, c.cen, c.sc), "program 6")
    fo = [(2 * i + 1) % 3 for i in range(B)]
    _same(one.frame_heatmaps(c.frames, c.fcen, c.fsc, frame_of=fo), two.frame_heatmaps(c.frames, c.fcen, c.fsc, frame_of=fo), "frames + 0")
    _same_all(one.frame_final_preds(c.frames, c.fcen, c.fsc, frame_of=fo), two.frame_final_preds(c.frames, c.fcen, c.fsc, frame_of=fo),
              "frames + 6")


def image_flip_case(c):
    """flip_heatmaps / final_preds(flip=True): the 2 B plan on cat(x, mirror(x)), merged"""
    one, two, B, K = c.one, c.two, c.B, c.K
    assert not bits_equal(host(c.merged), host(c.a))
    own = torch.full((B, c.C, one.map_height, one.map_width), SENT, device=c.dev)
    got = one.flip_heatmaps(c.x, c.dataset, out=own)
    assert got is own
    _same(got, c.merged, "flip_heatmaps")
    assert one.workspace.numel() >= _need(one, 4) + 256
    if c.bbox:                                                     # the box channels exchange tl <-> tr and bl <-> br
        fb = K + 1
        assert c.perm[fb:] == [fb, fb + 3, fb + 4, fb + 1, fb + 2]
        want = (host(c.a)[:, fb + 1] + host(c.f)[:, fb + 3][..., ::-1]) * F32(0.5)
        assert bits_equal(host(got)[:, fb + 1], want.astype(F32))
        assert not bits_equal(host(got)[:, fb + 1], ((host(c.a)[:, fb + 1] + host(c.f)[:, fb + 1][..., ::-1]) * F32(0.5)).astype(F32))
    res = [one.map_width, one.map_height]
    ref = ops.final_preds(c.merged, c.cen, c.sc, res, return_coords=True)
    _same_all(one.final_preds(c.x, c.cen, c.sc, res, flip=True, dataset=c.dataset), ref, "final_preds(flip=True)")
    ref = ops.final_preds(c.merged, return_coords=True)
    _same_all(one.final_preds(c.x, flip=True, dataset=c.dataset), ref, "final_preds(flip=True) without a centre")
    # a flagged and an unflagged plan alive together give their own results
    t1 = two.flip_heatmaps(c.x, c.dataset)
    o1 = one.flip_heatmaps(c.x, c.dataset)
    t2 = two.flip_heatmaps(c.x, c.dataset)
    _same(t1, c.two_pass, "the unflagged plan beside a flagged one")
    _same(t2, t1, "the unflagged plan after a call of the flagged one")
    _same(o1, c.merged, "the flagged plan after a call of the unflagged one")


def image_frames_case(c):
    """from frames with the flip test: the NCHW entries of the SAME flagged plan on the crop"""
    one, B = c.one, c.B
    orders = [[1] * B, [(2 * i + 2) % 3 for i in range(B)]]       # a shared frame; a permuted frame_of
    seen = []
    for fo, rots in zip(orders, ((0, 30), (0,))):
        for rot in rots:
            x = ops.augment_image(c.frames[fo], protocol.crop_maps(c.fcen, c.fsc, [c.H, c.W], rot).reshape(B, 2, 3), (c.H, c.W))
            want = one.flip_heatmaps(x, c.dataset)
            own = torch.full_like(want, SENT)
            got = one.frame_heatmaps(c.frames, c.fcen, c.fsc, frame_of=fo, rot=rot, flip=True, dataset=c.dataset, out=own)
            assert got is own
            _same(got, want, ("frame_heatmaps(flip=True)", fo, rot))
            ref = one.final_preds(x, c.fcen, c.fsc, flip=True, dataset=c.dataset)
            _same_all(one.frame_final_preds(c.frames, c.fcen, c.fsc, frame_of=fo, rot=rot, flip=True, dataset=c.dataset), ref,
                      ("frame_final_preds(flip=True)", fo, rot))
            seen.append(host(got).copy())
    assert not bits_equal(seen[0], seen[1]) and not bits_equal(seen[0], seen[2])          # the rotation and the frame matter
    assert one.workspace.numel() >= _need(one, FROM_FRAMES + 4) + 256


def _image_flip_calls(c, plan):
    """the four C entries of the flip rows -> {row: call(out tensors, ws pointer, ws bytes) -> status}, and the tensors kept alive"""
    L = _C.lib()
    pa = ops._perm_array(c.perm, c.C)
    fo = torch.tensor([1] * c.B, dtype=torch.int32).to(c.dev)
    inv = torch.from_numpy(protocol.crop_maps(c.fcen, c.fsc, [c.H, c.W], 30)).to(c.dev)
    src = (c.frames.data_ptr(), fc.U8, 3, 40, 56, fo.data_ptr(), None, inv.data_ptr(), 128.0, 128.0, 256.0)
    xp, w, h = c.x.data_ptr(), plan.map_width, plan.map_height
    calls = {
        4: lambda o, ws, n: L.up_unipose_flip_forward(plan._plan, xp, pa, o[0].data_ptr(), ws, n, plan._stream()),
        5: lambda o, ws, n: L.up_unipose_final_preds(plan._plan, xp, pa, None, w, h, o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws, n,
                                                     plan._stream()),
        FROM_FRAMES + 4: lambda o, ws, n: L.up_unipose_frame_heatmaps(plan._plan, *src, pa, o[0].data_ptr(), ws, n, plan._stream()),
        FROM_FRAMES + 5: lambda o, ws, n: L.up_unipose_frame_final_preds(plan._plan, *src, pa, None, w, h, o[1].data_ptr(), o[2].data_ptr(),
                                                                         o[3].data_ptr(), ws, n, plan._stream()),
    }
    return calls, (pa, fo, inv)


def _outs(c, plan, lead=None):
    lead = (c.B,) if lead is None else lead
    h, w = (plan.map_height, plan.map_width) if hasattr(plan, "map_height") else (plan.out_height, plan.out_width)
    ch = plan.out_channels
    return [torch.full(lead + (ch, h, w), SENT, device=c.dev), torch.full(lead + (ch, 2), SENT, device=c.dev),
            torch.full(lead + (ch, 2), SENT, device=c.dev), torch.full(lead + (ch, 1), SENT, device=c.dev)]


def _workspace_rows(c, plan, calls, rows, big_need, other_flip_ws, what):
    """each flip row: in a 0xFF workspace of exactly its reported need the bits of a generous one; 256 bytes less refused, nothing
    written; the need at least that of the 2 B plan's forward"""
    L = _C.lib()
    prefix = plan._prefix
    for k in rows:
        need = _need(plan, k, prefix)
        print(f"{what} row {k}: one-pass need {need}, the 2B plan's forward {big_need}, the two-pass plan's flip_workspace() {other_flip_ws}")
        assert need >= big_need > 0, (k, need, big_need)
        roomy = torch.zeros(need + 4096 + 256, dtype=torch.uint8, device=c.dev)
        ref = _outs(c, plan, c.lead)
        assert calls[k](ref, _aligned(roomy), need + 4096) == 0, (k, L.up_last_error())
        buf, ws = _ff_workspace(c.dev, need)
        got = _outs(c, plan, c.lead)
        assert calls[k](got, ws, need) == 0, (k, L.up_last_error())
        for g, r in zip(got, ref):
            assert bits_equal(host(g), host(r)), (k, "0xFF workspace")
        assert any((host(g) != SENT).any() for g in got)
        sent = _outs(c, plan, c.lead)
        assert calls[k](sent, ws, need - 256) != 0 and b"workspace" in L.up_last_error(), k
        assert all((host(s) == SENT).all() for s in sent), k
        del buf


def image_workspace_case(c):
    L = _C.lib()
    c.lead = (c.B,)
    calls, keep = _image_flip_calls(c, c.one)
    _workspace_rows(c, c.one, calls, IMAGE_FLIP_ROWS, _need(c.big, 0), L.up_unipose_plan_flip_workspace(c.two._plan), "image " + c.storage)
    assert L.up_unipose_plan_flip_workspace(c.one._plan) == max(_need(c.one, 4), _need(c.one, 5), _need(c.one, 6))
    # the mirrored input is half of the one input: the from-frames flip rows need no extra tensor
    assert _need(c.one, FROM_FRAMES + 4) == _need(c.one, 4) and _need(c.one, FROM_FRAMES + 5) == _need(c.one, 5)
    # the refusals of the entries are what they were: a perm entry, res, a null pointer
    ws, nbytes = c.one._flip_ws()
    sent = _outs(c, c.one)
    badp = ops._perm_array([c.C] + c.perm[1:], c.C)
    xp = c.x.data_ptr()
    assert L.up_unipose_flip_forward(c.one._plan, xp, badp, sent[0].data_ptr(), ws, nbytes, 0) == -1 and b"perm[0]" in L.up_last_error()
    assert L.up_unipose_flip_forward(c.one._plan, xp, None, sent[0].data_ptr(), ws, nbytes, 0) == -1
    assert L.up_unipose_final_preds(c.one._plan, xp, keep[0], None, 0, 8, sent[1].data_ptr(), None, sent[3].data_ptr(), ws, nbytes, 0) == -1
    assert L.up_unipose_final_preds(c.one._plan, xp, keep[0], None, 8, 8, None, None, sent[3].data_ptr(), ws, nbytes, 0) == -1
    assert all((host(s) == SENT).all() for s in sent)


def image_float64_case(c):
    """fp32 storage: the one-pass maps within 2e-5 (max_rel, the bar of an fp32 plan, G1) of the float64 evaluation of the network,
    merged in float64; bf16 storage: the figures, no bound (the project sets none)"""
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in c.model.state_dict().items()}
    x64 = c.x.detach().cpu().double()
    with torch.no_grad():
        a64 = O.unipose_forward(sd64, x64, output_stride=c.output_stride)
        f64 = O.unipose_forward(sd64, torch.flip(x64, [3]), output_stride=c.output_stride)
    ref = 0.5 * (a64 + torch.flip(f64[:, c.perm], [3]))
    e_one, e_two = O.max_rel(c.one.flip_heatmaps(c.x, c.dataset).cpu(), ref), O.max_rel(c.two_pass.cpu(), ref)
    print(f"image plan {c.storage} K={c.K} B={c.B} {c.H}x{c.W}: max_rel against float64, one pass {e_one:.3e}, two passes {e_two:.3e}")
    if c.storage == "f32":
        assert e_one < 2e-5, e_one


def image_create_t_case(c):
    """up_unipose_plan_create_t is up_unipose_plan_create_ex(..., 0, ...): the same figures, the same bits"""
    from unipose_amd.plan import UniPosePlan, _Config
    L = _C.lib()
    dt = 1 if c.storage == "bf16" else 0
    cfg = _Config(c.B, c.H, c.W, c.output_stride, c.C)
    plans = [_raw(UniPosePlan, "up_unipose_plan", c.model, cfg, dt, 0, via_t) for via_t in (True, False)]
    rows = list(range(7)) + [FROM_FRAMES + k for k in (0, 4, 5, 6)]
    for k in rows:
        assert _need(plans[0], k) == _need(plans[1], k) == _need(c.two, k), k
    assert L.up_unipose_plan_flags(plans[0]._plan) == L.up_unipose_plan_flags(plans[1]._plan) == 0
    outs = []
    pa = ops._perm_array(c.perm, c.C)
    for p in plans:
        need = L.up_unipose_plan_flip_workspace(p._plan)
        buf, ws = _ff_workspace(c.dev, need)
        out = torch.full_like(c.two_pass, SENT)
        _C.check(L.up_unipose_flip_forward(p._plan, c.x.data_ptr(), pa, out.data_ptr(), ws, need, p._stream()), "flip_forward")
        outs.append(out)
        p.close()
    _same(outs[0], outs[1], "create_t against create_ex(0)")
    _same(outs[0], c.two_pass, "create_t against the two-pass plan")


def argument_case(dev):
    """flip= of the two classes: anything but the two names is a ValueError, before the model is looked at"""
    from unipose_amd.plan import UniPoseLSTMPlan, UniPosePlan
    for cls in (UniPosePlan, UniPoseLSTMPlan):
        for bad in ("one", "ONE_PASS", "", None, 1, True):
            try:
                cls(None, 1, 64, 64, flip=bad)
            except ValueError as e:
                assert "flip" in str(e)
            else:
                raise AssertionError(f"flip={bad!r} was not refused")


# ---- 5. the video plan, flagged -------------------------------------------------------------------------------------------------------------
VIDEO_CASES = [dict(K=13, B=1, T=2, H=32, W=40), dict(K=15, B=2, T=3, H=39, W=39), dict(K=13, B=1, T=2, H=64, W=72, output_stride=8)]
VIDEO_STORAGES = [("f32", 0), ("bf16", 0), ("f32", 1), ("bf16", 1), ("f32", 2)]
VIDEO_FLIP_ROWS = (4, 5, FROM_FRAMES + 4, FROM_FRAMES + 5)
VIDEO_PLAIN_ROWS = (0, 1, 2, 3, 6, 7, 8, FROM_FRAMES + 2, FROM_FRAMES + 6, FROM_FRAMES + 7, FROM_FRAMES + 8)
FRAME_HW = (45, 60)


class VideoCtx:
    """One model, its three plans — unflagged, flagged, unflagged at batch 2 B — the clip, the clip from frames and the oracle's
    results: computed once per configuration and shared, unchanged, by the tests."""

    def __init__(self, dev, storage, K=13, B=1, T=2, H=32, W=40, output_stride=16):
        from unipose_amd.plan import UniPoseLSTMPlan
        self.dev, self.storage, self.K, self.B, self.T, self.H, self.W, self.output_stride = dev, storage, K, B, T, H, W, output_stride
        if output_stride == 16:
            m = lc.lstm_model(dev, K)
        else:
            m = lc.mc.skeleton("lstm", K, output_stride=output_stride)
            m.load_state_dict(O.synth_state_dict(K, 4, lstm=True))
            m = m.to(dev).eval()
        self.model = m
        self.x = O.synth_input((B, T, 3, H, W), 15).to(dev)
        self.cm = O.synth_input((B, T, 1, H, W), 16, "rand").to(dev)
        self.two = UniPoseLSTMPlan(m, B, H, W, frames=T, storage=storage)
        self.one = UniPoseLSTMPlan(m, B, H, W, frames=T, storage=storage, flip="one_pass")
        self.big = UniPoseLSTMPlan(m, 2 * B, H, W, frames=T, storage=storage)
        self.h, self.w = self.one.out_height, self.one.out_width
        self.lead = (B, T)
        self.perm = protocol.flip_perm(None, K, False, PAIRS)
        self.merged = self.oracle(self.x, self.cm)
        self.heats = self.two.clip(self.x, self.cm)[0]
        heats_f = self.two.clip(torch.flip(self.x, [-1]).contiguous(), torch.flip(self.cm, [-1]).contiguous())[0]
        self.two_pass = ops.flip_merge(self.heats.flatten(0, 1), heats_f.flatten(0, 1), self.perm).reshape(self.heats.shape)
        rng = np.random.default_rng(3)
        self.cen, self.sc = rng.uniform(40, 120, (B, T, 2)), rng.uniform(0.5, 1.5, (B, T))
        # from frames: a shared and permuted frame_of, one crop and one centre of the centre map per frame of the clip
        n = B * T
        self.frames = torch.from_numpy(fc.pixels_of((36, K), (3,) + FRAME_HW + (3,), "u8")).to(dev)
        self.valid = [FRAME_HW, (40, 50), FRAME_HW]
        self.fo = np.array([(2 * i + 1) % 3 for i in range(n)]).reshape(B, T)
        self.fcen = np.array([[30.0 + 3 * i, 22.0 - 2 * i] for i in range(n)]).reshape(B, T, 2)
        self.fsc = np.array([0.2 * (1 + 0.15 * i) for i in range(n)]).reshape(B, T)
        self.cc = np.array([[W / 2 + 2.5 * i - 3, H / 2 - 1.75 * i + 2] for i in range(n)]).reshape(B, T, 2)
        self.rot = 20
        self.kw = dict(frame_of=self.fo, rot=self.rot, valid_hw=self.valid, crop_center=self.cc)
        fo = self.fo.reshape(-1)
        maps = protocol.crop_maps(self.fcen.reshape(n, 2), self.fsc.reshape(n), [H, W], self.rot).reshape(n, 2, 3)
        self.fx = ops.augment_image(self.frames[torch.from_numpy(fo).to(dev)], maps, (H, W),
                                    valid_hw=np.asarray(self.valid)[fo]).reshape(B, T, 3, H, W)
        self.fcm = ops.make_centermaps(self.cc.reshape(n, 2), H, W, 3.0, device=dev).reshape(B, T, 1, H, W)

    def oracle(self, x, cm):
        """the definition of the one-pass form: the 2 B plan's clip on cat(x, mirror(x)), the two batch halves merged frame by frame"""
        B = self.B
        xx = torch.cat([x, torch.flip(x, [-1])]).contiguous()
        cc = torch.cat([cm, torch.flip(cm, [-1])]).contiguous()
        heats = self.big.clip(xx, cc)[0]
        a, f = heats[:B].contiguous(), heats[B:].contiguous()
        return ops.flip_merge(a.flatten(0, 1), f.flatten(0, 1), self.perm).reshape(a.shape)


@functools.lru_cache(maxsize=None)
def video_ctx(dev, storage, index):
    return VideoCtx(dev, storage, **VIDEO_CASES[index])


def video_plain_rows_case(c):
    """every program without the flip test: the unflagged plan's figures, bits and states, two interleaved streams included"""
    L = _C.lib()
    one, two, B, T = c.one, c.two, c.B, c.T
    prefix = "up_unipose_lstm_plan"
    assert L.up_unipose_lstm_plan_flags(one._plan) == ONE_PASS and L.up_unipose_lstm_plan_flags(two._plan) == 0
    assert one.flip_mode == "one_pass" and two.flip_mode == "two_pass"
    for k in VIDEO_PLAIN_ROWS:
        assert _need(one, k, prefix) == _need(two, k, prefix) > 0, k
    assert L.up_unipose_lstm_plan_workspace(one._plan) == L.up_unipose_lstm_plan_workspace(two._plan)
    assert L.up_unipose_lstm_plan_state_bytes(one._plan) == L.up_unipose_lstm_plan_state_bytes(two._plan)
    assert L.up_unipose_lstm_plan_flip_workspace(one._plan) == max(_need(one, 4, prefix), _need(one, 5, prefix))
    prev = [None, None]
    for j in range(T):                                                            # rows 0 and 1
        res = [p.step(c.x[:, j], c.cm[:, j], pv) for p, pv in zip((one, two), prev)]
        _same_all(res[0], res[1], ("step", j))
        prev = [(r[2], r[1]) for r in res]
    _same_all(one.clip(c.x, c.cm), two.clip(c.x, c.cm), "clip")                    # row 2
    _same_all(one.clip_keypoints(c.x, c.cm), two.clip_keypoints(c.x, c.cm), "clip_keypoints")          # row 3
    _same_all(one.clip_final_preds(c.x, c.cm, c.cen, c.sc), two.clip_final_preds(c.x, c.cm, c.cen, c.sc), "clip_final_preds")      # row 6
    # rows 7 and 8: two interleaved streams on each plan, the second on the frames in reverse order
    xb, cmb = torch.flip(c.x, [1]).contiguous(), torch.flip(c.cm, [1]).contiguous()
    states = [[p.stream_state(), p.stream_state()] for p in (one, two)]
    for j in range(T):
        ra = [p.stream(c.x[:, j], c.cm[:, j], s[0], first=j == 0) for p, s in zip((one, two), states)]
        rb = [p.stream(xb[:, j], cmb[:, j], s[1], first=j == 0) for p, s in zip((one, two), states)]
        _same_all(ra[0], ra[1], ("stream a", j))
        _same_all(rb[0], rb[1], ("stream b", j))
    assert torch.equal(states[0][0].cpu(), states[1][0].cpu()) and torch.equal(states[0][1].cpu(), states[1][1].cpu())
    assert T == 1 or not torch.equal(states[0][0].cpu(), states[0][1].cpu())
    # from frames
    _same_all(one.clip_frame_heatmaps(c.frames, c.fcen, c.fsc, **c.kw), two.clip_frame_heatmaps(c.frames, c.fcen, c.fsc, **c.kw), "frames + 2")
    _same_all(one.clip_frame_final_preds(c.frames, c.fcen, c.fsc, **c.kw), two.clip_frame_final_preds(c.frames, c.fcen, c.fsc, **c.kw),
              "frames + 6")
    states = [p.stream_state() for p in (one, two)]
    for j in range(T):
        res = [p.stream_frames(c.frames, c.fcen[:, j], c.fsc[:, j], s, first=j == 0, frame_of=c.fo[:, j], valid_hw=c.valid,
                               crop_center=c.cc[:, j]) for p, s in zip((one, two), states)]
        _same_all(res[0], res[1], ("stream_frames", j))
    assert torch.equal(states[0].cpu(), states[1].cpu())


def video_flip_case(c):
    one, B, T = c.one, c.B, c.T
    assert not bits_equal(host(c.merged), host(c.heats))
    own = torch.full_like(c.merged, SENT)
    got = one.clip_flip_heatmaps(c.x, c.cm, pairs=PAIRS, out=own)
    assert got is own
    _same(got, c.merged, "clip_flip_heatmaps")
    other = one.clip_flip_heatmaps(c.x, c.cm, pairs=[])                             # the permutation matters
    assert not bits_equal(host(other), host(got))
    flat = (c.cen.reshape(B * T, 2), c.sc.reshape(B * T))
    for cen, sc, fl in ((c.cen, c.sc, flat), (None, None, (None, None))):
        ref = ops.final_preds(c.merged.flatten(0, 1), fl[0], fl[1], return_coords=True)
        got3 = one.clip_final_preds(c.x, c.cm, cen, sc, flip=True, pairs=PAIRS)
        for g, r, n in zip(got3, ref, ("preds", "coords", "maxvals")):
            _same(g, r.reshape(g.shape), (n, cen is None))
    # a flagged and an unflagged plan alive together give their own results
    t1 = c.two.clip_flip_heatmaps(c.x, c.cm, pairs=PAIRS)
    o1 = one.clip_flip_heatmaps(c.x, c.cm, pairs=PAIRS)
    _same(t1, c.two_pass, "the unflagged plan beside a flagged one")
    _same(o1, c.merged, "the flagged plan after a call of the unflagged one")


def video_frames_case(c):
    """from frames with the flip test: the NCHW forms of the SAME flagged plan on the cropped clip and the centre maps"""
    L = _C.lib()
    one, B, T, K = c.one, c.B, c.T, c.K
    want = one.clip_flip_heatmaps(c.fx, c.fcm, pairs=PAIRS)
    _same(want, c.oracle(c.fx, c.fcm), "the cropped clip against the 2B plan")
    own = torch.full_like(want, SENT)
    got = one.clip_frame_heatmaps(c.frames, c.fcen, c.fsc, flip=True, pairs=PAIRS, out=own, **c.kw)
    assert got is own
    _same(got, want, "clip_frame_heatmaps(flip=True)")
    # a centre of the centre map that differs per frame changes the result: a constant one, and the same centres in another order
    const = one.clip_frame_heatmaps(c.frames, c.fcen, c.fsc, flip=True, pairs=PAIRS, **dict(c.kw, crop_center=None))
    assert not bits_equal(host(const), host(want))
    if B * T > 1:
        swapped = one.clip_frame_heatmaps(c.frames, c.fcen, c.fsc, flip=True, pairs=PAIRS,
                                          **dict(c.kw, crop_center=c.cc.reshape(-1, 2)[::-1].reshape(c.cc.shape)))
        assert not bits_equal(host(swapped), host(want))
    ref = one.clip_final_preds(c.fx, c.fcm, c.fcen, c.fsc, flip=True, pairs=PAIRS)
    _same_all(one.clip_frame_final_preds(c.frames, c.fcen, c.fsc, flip=True, pairs=PAIRS, **c.kw), ref, "clip_frame_final_preds(flip=True)")
    # a non-NULL cell_last / hide_last with a perm is still refused, nothing written
    args, keep, _ = one._frame_args("test", c.frames, c.fcen, c.fsc, c.fo, c.rot, c.valid, (B, T))
    cc = torch.from_numpy(c.cc).to(c.dev)
    pa = ops._perm_array(c.perm, K + 1)
    sent = torch.full_like(want, SENT)
    st = torch.full((B, K + 2, c.h, c.w), SENT, device=c.dev)
    ws, nbytes = one._frame_ws(4)
    for cell, hide in ((st.data_ptr(), None), (None, st.data_ptr())):
        assert L.up_unipose_lstm_clip_frame_heatmaps(one._plan, *args, cc.data_ptr(), 3.0, pa, sent.data_ptr(), cell, hide, ws, nbytes,
                                                     one._stream()) == -1 and b"state" in L.up_last_error()
    assert (host(sent) == SENT).all() and (host(st) == SENT).all()
    del keep


def video_workspace_case(c):
    L = _C.lib()
    one, B, T, K = c.one, c.B, c.T, c.K
    prefix = "up_unipose_lstm_plan"
    pa = ops._perm_array(c.perm, K + 1)
    args, keep, _ = one._frame_args("test", c.frames, c.fcen, c.fsc, c.fo, c.rot, c.valid, (B, T))
    cc = torch.from_numpy(c.cc).to(c.dev)
    xp, cp = c.x.data_ptr(), c.cm.data_ptr()
    calls = {
        4: lambda o, ws, n: L.up_unipose_lstm_clip_flip(one._plan, xp, cp, pa, o[0].data_ptr(), ws, n, one._stream()),
        5: lambda o, ws, n: L.up_unipose_lstm_clip_final_preds(one._plan, xp, cp, pa, None, c.w, c.h, o[1].data_ptr(), o[2].data_ptr(),
                                                               o[3].data_ptr(), ws, n, one._stream()),
        FROM_FRAMES + 4: lambda o, ws, n: L.up_unipose_lstm_clip_frame_heatmaps(one._plan, *args, cc.data_ptr(), 3.0, pa, o[0].data_ptr(), None,
                                                                                None, ws, n, one._stream()),
        FROM_FRAMES + 5: lambda o, ws, n: L.up_unipose_lstm_clip_frame_final_preds(one._plan, *args, cc.data_ptr(), 3.0, pa, None, c.w, c.h,
                                                                                   o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws, n,
                                                                                   one._stream()),
    }
    # the 2 B plan's program 0 is a step; its clip (program 2) is what a one-pass flip row runs, plus the merged tensor
    big0, big2 = _need(c.big, 0, prefix), _need(c.big, 2, prefix)
    _workspace_rows(c, one, calls, VIDEO_FLIP_ROWS, big0, L.up_unipose_lstm_plan_flip_workspace(c.two._plan), "video " + c.storage)
    for k in VIDEO_FLIP_ROWS:
        print(f"video {c.storage} row {k}: one-pass need {_need(one, k, prefix)}, the 2B plan's clip {big2}")
    assert _need(one, FROM_FRAMES + 4, prefix) == _need(one, 4, prefix) and _need(one, FROM_FRAMES + 5, prefix) == _need(one, 5, prefix)
    # the other refusals, before any launch
    ws, nbytes = one._flip_ws()
    sent = _outs(c, one, c.lead)
    badp = ops._perm_array([K + 1] + list(range(1, K + 1)), K + 1)
    assert L.up_unipose_lstm_clip_flip(one._plan, xp, cp, badp, sent[0].data_ptr(), ws, nbytes, 0) == -1
    assert L.up_unipose_lstm_clip_flip(one._plan, xp, cp, None, sent[0].data_ptr(), ws, nbytes, 0) == -1
    assert L.up_unipose_lstm_clip_final_preds(one._plan, xp, cp, pa, None, 0, c.h, sent[1].data_ptr(), None, sent[3].data_ptr(), ws, nbytes, 0) == -1
    assert all((host(s) == SENT).all() for s in sent)
    del keep


def _lstm_float64(c, x, cm):
    """the float64 evaluation of the video network on a clip: the oracle's own pieces, frame by frame -> (B, T, K+1, h, w)"""
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in c.model.state_dict().items()}
    heats, hide, cell = [], None, None
    for j in range(c.T):
        f, low = O.backbone(sd, x[:, j], False, None, output_stride=c.output_stride)
        f = O.wasp(sd, f, False, None, True, None, 0.5, output_stride=c.output_stride)
        y = O.decoder(sd, f, low, False, None, None, (0.5, 0.1))
        z = torch.cat((y, torch.nn.functional.avg_pool2d(cm[:, j], 9, 8, 1)), dim=1)
        cell, hide = O.lstm0_cell(sd, z) if j == 0 else O.lstm_cell(sd, z, hide, cell)
        heats.append(O.lstm_head(sd, hide))
    return torch.stack(heats, 1)


def video_float64_case(c):
    """fp32 storage: the one-pass maps within 1e-3 (max_rel, the bar model_cases holds G5's frames to) of the float64 evaluation"""
    x64, cm64 = c.x.detach().cpu().double(), c.cm.detach().cpu().double()
    with torch.no_grad():
        a64 = _lstm_float64(c, x64, cm64)
        f64 = _lstm_float64(c, torch.flip(x64, [-1]), torch.flip(cm64, [-1]))
    ref = 0.5 * (a64 + torch.flip(f64[:, :, c.perm], [-1]))
    e_one = O.max_rel(c.one.clip_flip_heatmaps(c.x, c.cm, pairs=PAIRS).cpu(), ref)
    e_two = O.max_rel(c.two_pass.cpu(), ref)
    print(f"video plan {c.storage} K={c.K} B={c.B} T={c.T} {c.H}x{c.W}: max_rel against float64, one pass {e_one:.3e}, two passes {e_two:.3e}")
    if c.storage == "f32":
        assert e_one < 1e-3, e_one


def video_create_t_case(c):
    from unipose_amd.plan import UniPoseLSTMPlan, _LstmConfig
    L = _C.lib()
    prefix = "up_unipose_lstm_plan"
    dt = 1 if c.storage == "bf16" else 0
    cfg = _LstmConfig(c.B, c.T, c.H, c.W, c.output_stride, c.K)
    plans = [_raw(UniPoseLSTMPlan, prefix, c.model, cfg, dt, 0, via_t) for via_t in (True, False)]
    for k in list(range(9)) + [FROM_FRAMES + k for k in (2, 4, 5, 6, 7, 8)]:
        assert _need(plans[0], k, prefix) == _need(plans[1], k, prefix) == _need(c.two, k, prefix), k
    pa = ops._perm_array(c.perm, c.K + 1)
    outs = []
    for p in plans:
        need = L.up_unipose_lstm_plan_flip_workspace(p._plan)
        buf, ws = _ff_workspace(c.dev, need)
        out = torch.full_like(c.two_pass, SENT)
        _C.check(L.up_unipose_lstm_clip_flip(p._plan, c.x.data_ptr(), c.cm.data_ptr(), pa, out.data_ptr(), ws, need, p._stream()), "clip_flip")
        outs.append(out)
        p.close()
    _same(outs[0], outs[1], "create_t against create_ex(0)")
    _same(outs[0], c.two_pass, "create_t against the two-pass plan")
