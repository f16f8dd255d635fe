"""Convolution geometries the network never uses, and the edge shapes of the spatial / element-wise kernels (shared by
test_geometry_emu.py and test_geometry_gpu.py).

The C ABI takes any stride >= 1, dilation >= 1, padding >= 0 and rectangular filters; the network only ever asks for "same"
padding, square filters and stride 2 with dilation 1.  The cases here are the launches whose out-of-image taps reach furthest
outside the tensor: over-padding (output pixels without one live tap), pad < dil, stride 2 on even sizes without padding
(the last input row / column is never read: its data gradient is exactly 0), stride 2 with dilation 2 (the generic strided
gather of the data gradient), 2x2 and R != S filters, filters at least as large as the image.

Checker: F.conv2d in float64 on the CPU with autograd, compared ELEMENT BY ELEMENT (max-error over max-magnitude passes a
wrong value on an element that is small next to the tensor maximum, e.g. in the padding ring):

    |got - ref64| <= 2 (L + 1) 2^-24 A

A is the same operation in float64 on |x|, |w|, |dy| (+ |bias|), L the reduction length (C R S for y, K R S for dx, N P Q for
dw / db): the standard bound of an fp32 dot product summed in any order, times 2 for non-nearest rounding inside the MFMA.  A
dropped or added tap exceeds it by about three orders of magnitude.  Where the dot-product part of A is 0 nothing may be
added at all: dx == 0 and y == bias exactly.  bf16 storage adds one rounding of the stored result, 2^-8 |ref64|, to y and dx.
"""
import ctypes as C
import functools
import math

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import glds32_cases as g32
import op_cases as oc
from unipose_amd import _C, ops

BF = torch.bfloat16
EPS = 2.0 ** -24

# (group, (n, h, w, r, s, stride, pad, dil)); bias is on for every second case
GEOMETRIES = [
    ("valid", (2, 9, 9, 3, 3, 1, 0, 1)),
    ("over-padded", (2, 9, 7, 3, 3, 1, 2, 1)),
    ("over-padded", (2, 8, 8, 1, 1, 1, 1, 1)),              # 1x1 with a ring of pure padding
    ("pad<dil", (1, 23, 23, 3, 3, 1, 3, 6)),
    ("no-pad dilated", (1, 23, 23, 3, 3, 1, 0, 6)),
    ("pad>dil", (3, 7, 7, 3, 3, 1, 4, 2)),
    ("stride 2", (2, 9, 9, 3, 3, 2, 0, 1)),
    ("stride 2", (2, 10, 10, 3, 3, 2, 0, 1)),               # even size, no padding: last row / column never read
    ("stride 2", (2, 10, 8, 1, 1, 2, 0, 1)),
    ("stride 2", (2, 10, 10, 3, 3, 2, 2, 1)),
    ("stride 2", (2, 12, 9, 3, 3, 2, 1, 1)),
    ("stride 2", (2, 11, 11, 5, 5, 2, 2, 1)),
    ("stride 2", (2, 9, 9, 3, 3, 2, 2, 2)),                 # dilation 2: the generic strided gather in the data gradient
    ("small/rect", (2, 9, 9, 2, 2, 1, 0, 1)),
    ("small/rect", (2, 9, 9, 2, 2, 2, 1, 1)),
    ("small/rect", (2, 9, 9, 1, 3, 1, 1, 1)),
    ("small/rect", (2, 9, 9, 3, 1, 1, 1, 1)),
    ("small/rect", (2, 9, 9, 2, 3, 2, 1, 1)),
    ("filter>=image", (1, 5, 5, 7, 7, 1, 3, 1)),
    ("filter>=image", (1, 3, 3, 3, 3, 1, 1, 1)),
    ("filter>=image", (1, 12, 12, 11, 11, 1, 2, 1)),        # the WIDE form (121 taps) with short padding
]
GEOS = [g_ for _, g_ in GEOMETRIES]
BIAS = {g_: i % 2 == 1 for i, g_ in enumerate(GEOS)}
ALIGNED, GENERIC = (32, 64), (10, 18)       # the direct-to-LDS path / the generic path with pad lanes (10 -> 12, 18 -> 20 channels)
# K-split tail tiles (chip shrunk to 3 CUs): valid, over-padded, pad < dil, stride 2 with pad = 2
SPLIT = [GEOS[0], GEOS[1], GEOS[3], GEOS[9]]
STRIDE1 = [g_ for g_ in GEOS if g_[5] == 1]
# one of each group, both stride-2 kinds (dilation 1: parity classes; dilation 2: strided gather); square filters
MODES = [GEOS[0], GEOS[1], GEOS[3], GEOS[4], GEOS[5], GEOS[7], GEOS[12], GEOS[14], GEOS[18]]
# conv -> BatchNorm: the BatchNorm passes take 4-aligned channel counts only (bn_apply refuses others), so only the input is ragged
CONV_BN_GENERIC = (10, 20)
CONV_BN = [GEOS[0], GEOS[1], GEOS[2], GEOS[3], GEOS[7], GEOS[12], GEOS[14], GEOS[18]]


def geo_id(g_):
    return "n%d_%dx%d_f%dx%d_s%d_p%d_d%d" % g_


def _gen(seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return gen


def _tune(**kw):
    for k, v in kw.items():
        _C.check(_C.lib().up_conv_tune(k.encode(), int(v)), k)


def _cnt(name):
    return int(_C.lib().up_conv_counter(name.encode()))


def _rb(t):
    return t.to(BF).float()


@functools.lru_cache(maxsize=None)
def conv_reference(geo, c, k, bias, bf16=False, seed=0):
    """Inputs (fp32, rounded to bf16 first for bf16 storage), the float64 results and the magnitudes A of one case; computed
    once and shared by every kernel form (callers must not modify it)."""
    n, h, w, r, s, stride, pad, dil = geo
    x = torch.randn(n, c, h, w, generator=_gen(seed))
    wt = torch.randn(k, c, r, s, generator=_gen(seed + 1)) * (2.0 / (c * r * s)) ** 0.5
    b = torch.randn(k, generator=_gen(seed + 2)) if bias else None
    if bf16:
        x, wt = _rb(x), _rb(wt)
    kw = dict(stride=stride, padding=pad, dilation=dil)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    y = F.conv2d(xr, wr, br, **kw)
    dy = torch.randn(y.shape, generator=_gen(seed + 3))
    if bf16:
        dy = _rb(dy)
    y.backward(dy.double())
    p, q = y.shape[2:]
    ax, aw, ady = x.double().abs(), wt.double().abs(), dy.double().abs()
    a_y = F.conv2d(ax, aw, None, **kw)
    ref = dict(x=x, w=wt, b=b, dy=dy, P=p, Q=q,
               y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if bias else None,
               A_y_dot=a_y, A_y=a_y + (b.double().abs().view(1, -1, 1, 1) if bias else 0.0),
               A_dx=conv2d_input(x.shape, aw, ady, **kw), A_dw=conv2d_weight(ax, wt.shape, ady, **kw), A_db=ady.sum((0, 2, 3)),
               L=dict(y=c * r * s, dx=k * r * s, dw=n * p * q, db=n * p * q))
    assert ref["A_dx"].shape == x.shape and ref["A_dw"].shape == wt.shape
    return ref


def _ratio(got, ref64, a, length, rel_term=0.0):
    """worst |got - ref64| / bound over the elements with a non-zero bound; elements with a zero bound must be exact."""
    got = got.double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    bound = 2.0 * (length + 1) * EPS * a + rel_term * ref64.abs()
    err = (got - ref64).abs()
    zero = bound == 0
    if bool(zero.any()) and float(err[zero].max()) != 0.0:
        return math.inf
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def check_conv(ref, y, dx, dw, db, c, k, bf16=False):
    """y, dx: NHWC device tensors (channel padded); dw: OIHW; db: (K,) or None.  Returns the worst got / bound ratio per tensor
    and asserts that none exceeds 1, that the elements no tap reaches are exact, and that the pad lanes (channels k..rup4(k) of y,
    c..rup4(c) of dx: present at the GENERIC pair, absent at the ALIGNED one and in bf16 storage) are zeros."""
    rel_term = 2.0 ** -8 if bf16 else 0.0
    yc, dxc = oc.nchw(y.float(), k), oc.nchw(dx.float(), c)
    ratios = {"y": _ratio(yc, ref["y"], ref["A_y"], ref["L"]["y"], rel_term),
              "dx": _ratio(dxc, ref["dx"], ref["A_dx"], ref["L"]["dx"], rel_term),
              "dw": _ratio(dw.cpu(), ref["dw"], ref["A_dw"], ref["L"]["dw"])}
    if db is not None:
        ratios["db"] = _ratio(db.cpu(), ref["db"], ref["A_db"], ref["L"]["db"])
    # no live tap: nothing may be added.  y == bias (0 without one) where the pixel lies wholly in padding, dx == 0 where no
    # tap reads the pixel
    dead_y, dead_dx = (ref["A_y_dot"] == 0).expand_as(yc), ref["A_dx"] == 0
    if ref["b"] is not None:
        bias_img = ref["b"].to(y.dtype).float().view(1, -1, 1, 1).expand_as(yc)
    else:
        bias_img = torch.zeros_like(yc)
    exact = {"y": bool((yc[dead_y] == bias_img[dead_y]).all()), "dx": bool((dxc[dead_dx] == 0).all())}
    pads = {"y": y.shape[3] == k or float(y.detach()[..., k:].float().abs().max()) == 0.0,
            "dx": dx.shape[3] == c or float(dx.detach()[..., c:].float().abs().max()) == 0.0}
    assert all(exact.values()) and all(pads.values()) and all(v <= 1.0 for v in ratios.values()), \
        dict(worst_got_over_bound=ratios, exact_where_no_tap=exact, pad_lanes_zero=pads,
             dead=(int(dead_y.sum()), int(dead_dx.sum())))
    return ratios


def _run_conv(dev, ref, geo, c, k, dtype):
    n, h, w, r, s, stride, pad, dil = geo
    bf = dtype == BF
    cp, kp = (ops.rup32(c), ops.rup32(k)) if bf else (ops.rup4(c), ops.rup4(k))
    x = oc.nhwc(ref["x"], dev, pad_to=cp).to(dtype)
    wt = ref["w"].clone().to(dev)
    b = ref["b"].clone().to(dev) if ref["b"] is not None else None
    dy = oc.nhwc(ref["dy"], dev, pad_to=kp).to(dtype)

    def run():
        y, d, _ = ops.conv_fwd_raw(x, wt, ops.ConvCfg(stride, pad, dil), bias=b)
        assert (d.P, d.Q) == (ref["P"], ref["Q"]) and y.shape == (n, d.P, d.Q, kp) and y.dtype == dtype
        dx = ops.conv_bwd_data_raw(dy, wt, d, x.shape, x.device)
        dw, db = ops.conv_bwd_weight_raw(x, dy, wt.shape, d, b is not None)
        assert dw.dtype == torch.float32
        return y, dx, dw, db
    return run


def conv_geometry_case(dev, geo, c, k, cus=0, tile_wants=(1, 100000)):
    """One geometry at one channel pair in fp32: both exact-fp32 generations (up_conv_tune glds32 = 1 / 0, the forward / data
    gradient and the weight gradient switched together) x tile_want (128- and 64-row tiles), every result against float64.
    cus: shrink the chip so that the launch has K-split tail tiles.  Returns the worst ratio per tensor over the forms."""
    n, h, w, r, s, stride, pad, dil = geo
    ref = conv_reference(geo, c, k, BIAS.get(geo, False))
    run = _run_conv(dev, ref, geo, c, k, torch.float32)
    names = ("glds32", "wgrad_glds32", "glds32_wide")
    worst = {}
    try:
        for gen in (1, 0):
            for tw in tile_wants:
                _tune(glds32=gen, glds32_wgrad=gen, tile_want=tw, cu_count=cus)
                c0 = {m: _cnt(m) for m in names}
                y, dx, dw, db = run()
                # the generic pair must really carry pad lanes (10 -> 12, 18 -> 20), or check_conv's pad-lane test is idle
                assert ((c, k) != GENERIC) or (y.shape[3] > k and dx.shape[3] > c), (y.shape, dx.shape)
                moved = {m: _cnt(m) - c0[m] for m in names}
                if not gen:
                    assert not any(moved.values()), ("glds32 = 0 still launched a direct-to-LDS kernel", moved)
                elif (c, k) == ALIGNED and stride == 1 and r * s <= 32:
                    assert moved["glds32"] > 0 and moved["wgrad_glds32"] > 0 and moved["glds32_wide"] == 0, moved
                elif (c, k) == ALIGNED and r * s > 32:
                    assert moved["glds32_wide"] > 0, moved
                try:
                    ratios = check_conv(ref, y, dx, dw, db, c, k)
                except AssertionError as e:
                    raise AssertionError(f"{geo_id(geo)} c={c} k={k} glds32={gen} tile_want={tw} cus={cus}: {e}") from None
                for k_, v in ratios.items():
                    worst[k_] = max(worst.get(k_, 0.0), v)
    finally:
        _tune(**g32.DEFAULTS)
    print(f"geometry {geo_id(geo)} c={c} k={k} cus={cus}: worst got/bound " + " ".join(f"{k_}={v:.3f}" for k_, v in worst.items()))
    return worst


def conv_geometry_bf16s_case(dev, geo):
    """The same in bf16 storage (aligned channel pair; inputs, weights and dy rounded to bf16 first)."""
    c, k = ALIGNED
    ref = conv_reference(geo, c, k, BIAS[geo], bf16=True)
    y, dx, dw, db = _run_conv(dev, ref, geo, c, k, BF)()
    try:
        ratios = check_conv(ref, y, dx, dw, db, c, k, bf16=True)
    except AssertionError as e:
        raise AssertionError(f"{geo_id(geo)} bf16 storage: {e}") from None
    print(f"geometry {geo_id(geo)} bf16 storage: worst got/bound " + " ".join(f"{k_}={v:.3f}" for k_, v in ratios.items()))
    return ratios


def operand_mode_case(dev, geo, math_, tol):
    """bf16x3 / bf16 operand kernels with the project's own metric and tolerances (test_conv_bf16_operand_kernels)."""
    n, h, w, r, s, stride, pad, dil = geo
    assert r == s
    ops.set_conv_math(math_)
    try:
        return oc.conv_case(dev, n, ALIGNED[0], h, w, ALIGNED[1], r, stride, pad, dil, tol=tol)
    finally:
        ops.set_conv_math("f32")


def _plain_conv_ok(dev):
    """an ordinary 3x3 convolution after a refused call: the refusal left no state behind"""
    conv_geometry_case(dev, (1, 6, 6, 3, 3, 1, 1, 1), *ALIGNED, tile_wants=(1,))


def stride3_case(dev, c, k):
    """Stride 3: the forward pass and the weight gradient are accepted and right, the data gradient refuses."""
    geo = (2, 10, 10, 3, 3, 3, 1, 1)
    n, h, w, r, s, stride, pad, dil = geo
    ref = conv_reference(geo, c, k, True)
    x = oc.nhwc(ref["x"], dev)
    wt, b, dy = ref["w"].clone().to(dev), ref["b"].clone().to(dev), oc.nhwc(ref["dy"], dev)
    y, d, _ = ops.conv_fwd_raw(x, wt, ops.ConvCfg(stride, pad, dil), bias=b)
    dw, db = ops.conv_bwd_weight_raw(x, dy, wt.shape, d, True)
    ratios = {"y": _ratio(oc.nchw(y, k), ref["y"], ref["A_y"], ref["L"]["y"]),
              "dw": _ratio(dw.cpu(), ref["dw"], ref["A_dw"], ref["L"]["dw"]),
              "db": _ratio(db.cpu(), ref["db"], ref["A_db"], ref["L"]["db"])}
    assert all(v <= 1.0 for v in ratios.values()), ratios
    try:
        ops.conv_bwd_data_raw(dy, wt, d, x.shape, x.device)
    except NotImplementedError as e:
        assert "stride 3" in str(e), e
    else:
        raise AssertionError("the stride-3 data gradient did not refuse")
    _plain_conv_ok(dev)
    return ratios


def stride2_addend_case(dev):
    """An addend with a stride-2 data gradient is refused."""
    c, k = ALIGNED
    x = torch.zeros(2, 9, 9, c).to(dev)
    wt = torch.randn(k, c, 3, 3, generator=_gen(1)).to(dev)
    d = ops.make_desc(x, wt, ops.ConvCfg(2, 1, 1))
    dy = torch.randn(2, d.P, d.Q, k, generator=_gen(2)).to(dev)
    try:
        ops.conv_bwd_data_raw(dy, wt, d, x.shape, x.device, add=torch.ones_like(x))
    except NotImplementedError as e:
        assert "addend" in str(e), e
    else:
        raise AssertionError("a stride-2 data gradient took an addend")
    _plain_conv_ok(dev)


# ---- empty outputs (host only) ------------------------------------------------------------------------
def empty_output_case(dev, stride):
    """5x5 on 4x4 without padding has no output pixel: refused by ops.make_desc before anything is allocated, and by
    check_desc behind every C entry, with a message that names the filter extent and the padded input; nothing is launched."""
    x = torch.zeros(1, 4, 4, 32).to(dev)
    wt = torch.zeros(64, 32, 5, 5).to(dev)
    names = ("igemm", "glds32", "wgrad_glds32")
    c0 = [_cnt(m) for m in names]
    for call in (lambda: ops.make_desc(x, wt, ops.ConvCfg(stride, 0, 1)),
                 lambda: ops.conv_fwd_raw(x, wt, ops.ConvCfg(stride, 0, 1))):
        try:
            call()
        except ValueError as e:
            assert "5x5" in str(e) and "4x4" in str(e) and "empty output" in str(e), e
        else:
            raise AssertionError("an empty convolution output was accepted")
    # the C entries themselves, with non-null pointers everywhere
    d = _C.ConvDesc()
    d.N, d.H, d.W, d.C, d.Cp, d.ldx = 1, 4, 4, 32, 32, 32
    d.K, d.R, d.S, d.stride, d.pad, d.dil = 64, 5, 5, stride, 0, 1
    d.ldy = d.Kp = 64
    buf = torch.zeros(64 * 32 * 25).to(dev)
    L = _C.lib()
    ep, p = _C.ConvEpilogue(), buf.data_ptr()
    calls = {
        "fwd": lambda: L.up_conv2d_fwd(C.byref(d), p, p, p, C.byref(ep), None),
        "bwd_data": lambda: L.up_conv2d_bwd_data(C.byref(d), p, p, p, None, 0, None),
        "bwd_weight": lambda: L.up_conv2d_bwd_weight_acc(C.byref(d), p, p, p, None, p, buf.numel() * 4, 0, 0, None),
    }
    # P = Q = 0 is what the geometry gives; 1 is what C's truncating division makes of (4 - 5) / 2 + 1
    for pq in (0, 1):
        d.P = d.Q = pq
        for what, call in calls.items():
            assert call() == -1, what                       # UP_ERR_INVALID
            msg = L.up_last_error().decode()
            assert "empty output" in msg and "5x5" in msg and "4x4" in msg, (what, msg)
    assert [_cnt(m) for m in names] == c0, "a refused call launched a kernel"


# ---- spatial and element-wise kernels at their edges ----------------------------------------------------
MAXPOOL_SHAPES = [(1, 4, 1, 1), (1, 4, 2, 2), (2, 6, 3, 4), (1, 4, 1, 7), (2, 12, 8, 1), (1, 4, 2, 9), (3, 20, 15, 16)]
MAXPOOL_TYPES = [(torch.float32, torch.float32), (torch.float32, BF), (BF, BF)]
BILINEAR_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (5, 3, 1, 1), (2, 2, 2, 2), (7, 5, 7, 5), (9, 12, 5, 7), (2, 3, 368, 300),
                   (1, 6, 4, 13), (6, 1, 13, 4), (3, 3, 4, 4), (47, 45, 368, 368)]
GAP_SHAPES = [(1, 4, 1, 1), (1, 1, 1, 3), (2, 64, 2, 1), (2, 68, 23, 23), (1, 130, 46, 46), (5, 8, 3, 3)]
BCAST_PQ = [(1, 1), (3, 5), (1, 17), (7, 9), (5, 13), (23, 23)]          # P * Q = 1, 15, 17, 63, 65, 529
AVGPOOL_SIZES = [(8, 8), (9, 9), (7, 15), (16, 23), (10, 17)]
MSE_SHAPES = [(1,), (255,), (257,), (131073,), (3, 17, 46, 46)]           # the last one uses all 512 partials


def maxpool_special():
    """6x6 planes: a window that is all -inf, a NaN, a plane of -0.0, a constant plane where every position ties."""
    x = torch.randn(1, 4, 6, 6, generator=_gen(31))
    x[0, 0, 1:4, 1:4] = -float("inf")
    x[0, 1, 2, 2] = float("nan")
    x[0, 2] = -0.0
    x[0, 3] = 1.5
    return x


def clip_avgpool_case(dev, h, w, b=2, t=3):
    """clip_avgpool9s8 on (B, T, 1, H, W) centre maps against the per-frame form: equal bits, frame-major output."""
    x = torch.rand(b, t, 1, h, w, generator=_gen(41)).to(dev)
    p, q = (h + 2 - 9) // 8 + 1, (w + 2 - 9) // 8 + 1
    y = torch.zeros(t * b, p, q, 16).to(dev)
    _C.check(_C.lib().up_clip_avgpool9s8_fwd(x.data_ptr(), y.data_ptr(), 16, 14, b, t, h, w, p, q, ops._stream(x)), "clip_avgpool")
    for ti in range(t):
        frame = torch.zeros(b, p, q, 16).to(dev)
        ops.avgpool9s8_into(x[:, ti].contiguous(), frame, 14)
        assert torch.equal(y[ti * b:(ti + 1) * b].cpu(), frame.cpu()), ti


def clip_layout_case(dev, c, b=2, t=3, h=5, w=7):
    """clip_nchw_to_nhwc (B, T, C, H, W) -> frame-major (T * B, H, W, ld) with zero pad lanes, and back, against permute."""
    ld = ops.rup4(c) + 4
    x = torch.randn(b, t, c, h, w, generator=_gen(42))
    xd = x.to(dev)
    y = torch.full((t * b, h, w, ld), 7.0).to(dev)
    _C.check(_C.lib().up_clip_nchw_to_nhwc(xd.data_ptr(), y.data_ptr(), b, t, c, h, w, ld, ops._stream(xd)), "clip_nchw_to_nhwc")
    want = x.permute(1, 0, 3, 4, 2).reshape(t * b, h, w, c)
    assert torch.equal(y.cpu()[..., :c], want) and float(y[..., c:].abs().max()) == 0
    z = torch.full((b, t, c, h, w), 7.0).to(dev)
    _C.check(_C.lib().up_clip_nhwc_to_nchw(y.data_ptr(), ld, z.data_ptr(), b, t, c, h, w, ops._stream(xd)), "clip_nhwc_to_nchw")
    assert torch.equal(z.cpu(), x)


def copy_add_case(dev, c, rows=37):
    """up_copy2d through ops._copy2d and up_add2d (no host wrapper: the C entry itself) with leading dimensions larger than C and
    element offsets: the copied / summed block is equal, everything around it untouched."""
    lds, ldd, soff, doff = c + 4 + c % 4, c + 8 - c % 4, 4, 8
    src = torch.randn(rows, lds + soff, generator=_gen(43))
    for so, do in ((0, 0), (soff, doff), (1, 3)):        # (16-byte aligned: vector form when C % 4 == 0; odd offsets: scalar form)
        dst = torch.full((rows, ldd + doff), 7.0)
        sd, dd = src.to(dev), dst.to(dev)
        ops._copy2d(sd, lds + soff, so, dd, ldd + doff, do, rows, c)
        want = dst.clone()
        want[:, do:do + c] = src[:, so:so + c]
        assert torch.equal(dd.cpu(), want), (c, so, do)
    a, b = torch.randn(rows, c + 3, generator=_gen(44)), torch.randn(rows, c + 5, generator=_gen(45))
    out = torch.full((rows, c + 1), 7.0)
    ad, bd, od = a.to(dev), b.to(dev), out.to(dev)
    _C.check(_C.lib().up_add2d(ad.data_ptr(), c + 3, bd.data_ptr(), c + 5, od.data_ptr(), c + 1, rows, c, ops._stream(ad)), "add2d")
    want = out.clone()
    want[:, :c] = a[:, :c] + b[:, :c]
    assert torch.equal(od.cpu(), want), c
