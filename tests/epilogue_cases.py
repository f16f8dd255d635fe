"""The fused epilogues of the convolution launches on their own, against float64 (shared by test_epilogue_emu.py and
test_epilogue_gpu.py): the forward epilogue (scale / shift / bias / residual / ReLU, the Welford partials, the folded BatchNorm
finalize, row groups) and the extended data-gradient epilogue (addend, the addend's ReLU mask, the fused BatchNorm-backward
reduction, its folded merge, row groups).  The convolution cores themselves are pinned by geometry_cases.py; the consumers of
the partial rows by bn_cases.py.  Every comparison is per element (per channel for sums) against a float64 restatement written
here, never against another kernel form and never over a tensor-wide maximum.  u = 2^-24; a quantity whose bound is 0 must be
exact.  L is the reduction length (C R S forward, K R S backward), A_dot / A_dx the same convolution on absolute values.

1. Forward eval epilogue.  The kernels evaluate  v = fl(fl(acc * scale) + esh),  esh = fl(shift + bias);  v = fl(v + res);
   v = max(v, 0)  (unipose_hip.h, up_conv_epilogue).  |acc - conv64| <= 2 (L + 1) u A_dot (geometry_cases.py), carried through the
   product: 2 (L + 1) u |scale| A_dot.  Then one rounding each for the product, esh, the sum with esh and the sum with the residual,
   every one of a value of at most |scale| A_dot + |shift| + |bias| + |res|:
       |y - ref| <= 2 (L + 1) u |scale| A_dot + 4 u (|scale| A_dot + |shift| + |bias| + |res|)      (+ 2^-8 |ref| stored as bf16)
   ReLU is 1-Lipschitz: no allowance, no element left out.  scale has both signs, so ReLU before the affine map differs by O(1);
   so do ReLU before the residual and a bias added twice.  The residual has pixel stride ldr > K with NaN in its pad lanes, y is
   written into a buffer with ldy > K filled with a sentinel that the lanes past K must keep.

2. Forward statistics.  A tile's row is (count, mean, M2) of the fp32 accumulators a_i = conv64_i + e_i, |e_i| <= E_i =
   2 (L + 1) u A_dot_i.  The tiles are merged here in float64 (Chan); N rows in all, c_i = conv64_i - mean64, Em = mean_i E_i:
   count == N exactly (every tile's count is at most the tile height, all tiles but the last of a group are equal).
   mean: the accumulators move it by at most Em.  A lane sums n <= bm / 2 values in fp32 and divides ((n - 1) u + u of amax =
       max_i (|conv64_i| + E_i)), the two Welford merges inside the tile (wf_merge: m1 + d (n2 / n), four roundings of terms of at
       most 2 amax, 7 u amax each) give a tile mean within  dl = (bm / 2 + 14) u amax  of the true mean of its accumulators; a
       weighted mean of tile means is no further off:
           |mean - mean64| <= Em + dl
   M2:  exact M2 of the accumulators differs from M2_64 by  P = sum_i (2 |c_i| (E_i + Em) + (E_i + Em)^2).
       A lane's two-pass q rounds the difference, the square and n - 1 sums: (n + 2) u q; a Welford merge rounds two sums and the
       four factors of d^2 n1 n2 / n: 6 u each, two merges; all terms are parts of M2:  (bm / 2 + 15) u (M2_64 + P).
       First order in the means' errors (as bn_cases.py found for the stand-alone statistics kernel): a merge adds
       (n1 n2 / n) (m2 - m1)^2 from ROUNDED means while q is (to second order) about the unrounded ones: 2 (n1 n2 / n) |d| 2 dl with
       |d| <= 2 dev, dev = max_i (|c_i| + E_i + Em), n1 n2 / n <= n / 4, summed over a level of merges: 2 N dev dl; three levels
       (half-waves, M-waves, tiles): 6 N dev dl.  Second order N dl^2 per level.
           |M2 - M2_64| <= P + (bm / 2 + 15) u (M2_64 + P) + 6 N dev dl + 3 N dl^2
       bm is the tallest tile height of the kernel family that gives the launch's tile count, and at most the number of rows (of
       the group): a single ragged tile sums its live rows only.
   bf16 storage takes the statistics from the fp32 accumulators, not from the rounded y: five statistics cases (OFFSET_FAMILIES) put
   an offset of 4096 on input channel 0, so output channels sit near w[k, 0] * 4096 (several hundred) with a standard deviation near
   1.4 (|mean| / std of a few hundred: the first-order term above is what such a channel needs; the other cases have |mean| / std
   below 1 and a bound of a few 1e-4 M2).  bf16 has
   a spacing of 1 .. 8 there: statistics of the ROUNDED y carry a quantisation variance of spacing^2 / 12 per element, M2 moves by
   tens of percent, while the bound above is a few percent of M2 (the case asserts that the rounded y would exceed it).
   Fold: up_bn_fold's outputs equal up_bn_finalize on the same partial rows bit for bit, and lie within bn_cases.propagate of the
   float64 statistics with the mean / M2 bounds above (+ u |mean64| for the stored mean).

3. Data-gradient epilogue.  dx = conv_input64(dy, w) + add [add bit]:
       |dx - ref| <= 2 (L + 1) u A_dx + 2 u |add|      (+ 2^-8 |ref| stored as bf16)
   (one rounding of the sum, of a value of at most A_dx + |add|, counted twice); where no tap reaches a pixel and nothing is
   added dx == 0.  The sums are defined on the STORED dx (both kernels: the bf16 addend path rounds first on purpose), so their
   reference is float64 on the launch's own dx:  g = dx [z bit],  S1 = sum g,  S2 = invstd sum g (y - mean).  A tile's partial
   is an fp32 sum of at most bm terms in some order: (bm - 1) u sum |g|; for S2 every term also rounds the difference and the
   product (2 u) and the sum is scaled by invstd (u):
       |sum_t partial[t][0] - S1| <= bm u sum |g|,      |sum_t partial[t][1] - S2| <= (bm + 4) u invstd sum |g (y - mean)|
   with bm as in section 2, so bm <= rows (of the group): never weaker than the issue's `rows u`.  No listed case has an input
   pixel that no tap reaches (stride 1 with a centre tap, or 1x1 without padding: A_dx > 0 everywhere), so the "dx == 0 exactly"
   clause has nothing to act on here; geometry_cases.py covers it for the plain data gradient, and a zero bound would demand
   exactness through _ratio all the same.  The folded merge adds a group's partial rows in double and rounds once; the issue's
   allowance `tiles u` (of sum_t |partial|, tiles = the group's tiles) is kept for gsum, and dgamma / dbeta take the sum of the
   groups' bounds.  mean / invstd differ strongly from channel to channel and from
   group to group, so a neighbour's value fails.

Refusals are tested only where the host returns before any launch (read off conv_igemm.hip: fill_fwd_args, run_igemm_bf16's
UP_REQUIREs and the head of up_conv2d_bwd_data_ex): return code, up_last_error, counters unmoved, a plain convolution afterwards.
"""
import ctypes as C
import functools
import math

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input

import bn_cases as bx
import geometry_cases as gx
import glds32_cases as g32
import op_cases as oc
from unipose_amd import _C, ops

BF, F32 = torch.bfloat16, torch.float32
U = bx.U
BF_TERM = 2.0 ** -8
SENT = 7.0
MATH_F32, MATH_BF16S, MATH_F32OUT = 0, 3, 4
DEFAULTS = dict(g32.DEFAULTS, bn_fold=1, glds=1, glds_big=1, tile_want_bf16=500, big_min_k=1024)
COUNTERS = ("igemm", "glds32", "glds32_epi1", "glds32_breg", "glds32_wide", "glds32_bnred", "glds32_grouped", "big")
OFFSET = 4096.0               # statistics cases named below: input channel 0 (docstring, section 2)
OFFSET_FAMILIES = ("epi1_1x1_t128", "reg_1x1", "bf16_glds_1x1", "bf16_reg_1x1", "bf16_big_1x1")
Worst, _ratio, _check = bx.Worst, bx._ratio, bx._check

# (n, h, w, r, s, stride, pad, dil)
G_1X1 = (2, 9, 9, 1, 1, 1, 0, 1)            # 162 rows: a ragged last tile
G_3X3 = (3, 7, 7, 3, 3, 1, 1, 1)            # tap-sorted rows
G_DEAD = (2, 8, 8, 3, 3, 1, 2, 2)           # dilated: dead taps
G_DIL3 = (4, 7, 7, 3, 3, 1, 3, 3)           # four 64-row tiles: K-split tails on a 3-CU chip
G_S2 = (2, 9, 9, 3, 3, 2, 1, 1)             # stride 2
G_RING = (2, 8, 8, 1, 1, 1, 1, 1)           # over-padded 1x1: a ring with A_dot = 0
G_WIDE = (1, 12, 12, 11, 11, 1, 5, 1)       # 121 taps: the WIDE form
G_192 = (3, 8, 8, 1, 1, 1, 0, 1)            # 192 rows: TM = 6 of the big tiles
ALIGNED, GENERIC = gx.ALIGNED, gx.GENERIC


def _fam(name, dtype, geo, ck, tune, expect):
    return dict(name=name, dtype=dtype, geo=geo, ck=ck, tune=tune, expect=expect)


_REG = dict(glds32=0)
_E1 = dict(glds32=1, glds32_epi=1)
_E0 = dict(glds32=1, glds32_epi=0)
# expect: counters that must move / must not move (proof of the kernel family)
_X_REG = dict(igemm=True, glds32=False)
_X_E1 = dict(glds32=True, glds32_epi1=True, glds32_wide=False, glds32_breg=False)
_X_E0 = dict(glds32=True, glds32_epi1=False)
FWD_FAMILIES = [
    _fam("reg_1x1", F32, G_1X1, ALIGNED, dict(_REG, tile_want=1), _X_REG),
    _fam("reg_3x3", F32, G_3X3, ALIGNED, dict(_REG, tile_want=100000), _X_REG),
    _fam("reg_dead", F32, G_DEAD, ALIGNED, dict(_REG, tile_want=1), _X_REG),
    _fam("reg_s2", F32, G_S2, ALIGNED, dict(_REG, tile_want=100000), _X_REG),
    _fam("reg_ring", F32, G_RING, ALIGNED, dict(_REG, tile_want=1), _X_REG),
    _fam("generic_1x1", F32, G_1X1, GENERIC, dict(_REG, tile_want=1), _X_REG),
    _fam("generic_3x3", F32, G_3X3, GENERIC, dict(_REG, tile_want=100000), _X_REG),
    _fam("generic_ring", F32, G_RING, GENERIC, dict(_REG, tile_want=1), _X_REG),
    _fam("epi1_1x1_t128", F32, G_1X1, ALIGNED, dict(_E1, tile_want=1), _X_E1),
    _fam("epi1_1x1_t64", F32, G_1X1, ALIGNED, dict(_E1, tile_want=100000), _X_E1),
    _fam("epi1_3x3_t128", F32, G_3X3, ALIGNED, dict(_E1, tile_want=1), _X_E1),
    _fam("epi1_3x3_t64", F32, G_3X3, ALIGNED, dict(_E1, tile_want=100000), _X_E1),
    _fam("epi1_dead", F32, G_DEAD, ALIGNED, dict(_E1, tile_want=1), _X_E1),
    _fam("epi1_s2", F32, G_S2, ALIGNED, dict(_E1, tile_want=100000), _X_E1),
    _fam("epi1_ring", F32, G_RING, ALIGNED, dict(_E1, tile_want=1), _X_E1),
    _fam("epi1_cu3", F32, G_DIL3, (64, 64), dict(_E1, tile_want=100000, cu_count=3), _X_E1),
    _fam("epi0_1x1", F32, G_1X1, ALIGNED, dict(_E0, tile_want=1), _X_E0),
    _fam("epi0_3x3", F32, G_3X3, ALIGNED, dict(_E0, tile_want=100000), _X_E0),
    _fam("epi0_s2", F32, G_S2, ALIGNED, dict(_E0, tile_want=1), _X_E0),
    _fam("breg_1x1", F32, G_1X1, ALIGNED, dict(_E1, tile_want=1, breg=1), dict(glds32=True, glds32_breg=True)),
    _fam("breg_ring_epi0", F32, G_RING, ALIGNED, dict(_E0, tile_want=100000, breg=1), dict(glds32=True, glds32_breg=True)),
    _fam("wide", F32, G_WIDE, ALIGNED, dict(_E1, tile_want=1), dict(glds32=True, glds32_wide=True)),
    _fam("bf16_glds_1x1", BF, G_1X1, (64, 64), dict(glds=1, tile_want_bf16=1), dict(big=False)),
    _fam("bf16_glds_3x3", BF, G_3X3, (64, 128), dict(glds=1, tile_want_bf16=100000), dict(big=False)),
    _fam("bf16_glds_dead", BF, G_DEAD, (64, 64), dict(glds=1, tile_want_bf16=1), dict(big=False)),
    _fam("bf16_glds_s2", BF, G_S2, (64, 64), dict(glds=1, tile_want_bf16=1), dict(big=False)),
    _fam("bf16_glds_ring", BF, G_RING, (64, 64), dict(glds=1, tile_want_bf16=100000), dict(big=False)),
    _fam("bf16_reg_1x1", BF, G_1X1, (64, 64), dict(glds=0, tile_want_bf16=1), dict(big=False)),
    _fam("bf16_reg_3x3", BF, G_3X3, (64, 128), dict(glds=0, tile_want_bf16=100000), dict(big=False)),
    _fam("bf16_reg_ring", BF, G_RING, (64, 64), dict(glds=0, tile_want_bf16=1), dict(big=False)),
    _fam("bf16_big_1x1", BF, G_1X1, (64, 256), dict(glds=1, glds_big=1, tile_want_bf16=1, big_min_k=64), dict(big=True)),
    _fam("bf16_big_3x3", BF, G_3X3, (64, 256), dict(glds=1, glds_big=1, tile_want_bf16=1, big_min_k=64), dict(big=True)),
    _fam("bf16_big_tm6", BF, G_192, (64, 256), dict(glds=1, glds_big=1, tile_want_bf16=1, big_min_k=64, cu_count=1), dict(big=True)),
]
FWD_F32OUT = [f for f in FWD_FAMILIES if f["name"] in ("bf16_glds_1x1", "bf16_glds_3x3", "bf16_glds_ring", "bf16_reg_1x1")]
# statistics: the same families (the generic pair with K = 20: the BatchNorm entries take 4-aligned channel counts only)
STATS_FAMILIES = [_fam("generic_1x1_k20", F32, G_1X1, gx.CONV_BN_GENERIC, dict(_REG, tile_want=1), _X_REG)] + [f for f in FWD_FAMILIES if f["name"] in (
    "reg_1x1", "reg_3x3", "reg_dead", "reg_s2", "epi1_1x1_t128", "epi1_1x1_t64", "epi1_3x3_t128", "epi1_3x3_t64",
    "epi1_dead", "epi1_s2", "epi1_ring", "epi1_cu3", "epi0_1x1", "epi0_3x3", "breg_1x1", "wide", "bf16_glds_1x1", "bf16_glds_3x3",
    "bf16_glds_dead", "bf16_glds_s2", "bf16_reg_1x1", "bf16_reg_3x3", "bf16_big_1x1", "bf16_big_3x3", "bf16_big_tm6")]


def fam_id(f):
    return f["name"]


def _gen(seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return gen


def _tune(**kw):
    for k, v in kw.items():
        _C.check(_C.lib().up_conv_tune(k.encode(), int(v)), k)


def _counters():
    return {m: int(_C.lib().up_conv_counter(m.encode())) for m in COUNTERS}


def _moved(c0):
    c1 = _counters()
    return {m: c1[m] - c0[m] for m in COUNTERS}


def _family_proof(moved, expect, what):
    for m, want in expect.items():
        assert (moved[m] > 0) == want, f"{what}: counter {m} moved by {moved[m]}, the case is not on the kernel family it names ({moved})"


def _rb(t, bf16):
    return t.to(BF).float() if bf16 else t


def _cl(t):
    """NCHW -> NHWC"""
    return t.permute(0, 2, 3, 1).contiguous()


def _wide(t, ld, dtype, dev, fill, live=None):
    """(n, h, w, c) values inside a buffer of pixel stride ld whose other lanes hold `fill`; (buffer, view of the first `live` lanes)"""
    n, h, w, c = t.shape
    buf = torch.full((n, h, w, ld), fill, dtype=torch.float32)
    buf[..., :c] = t
    buf = buf.to(dtype).to(dev)
    return buf, buf[..., :(live or c)]


def _pads(dtype):
    return ops.rup32 if dtype == BF else ops.rup4


def _tile_rows(rows, tiles, dtype):
    """most rows a tile of the launch can hold: the tallest tile of the family that cuts `rows` rows into `tiles` tiles, and no
    more than `rows` (the dead rows of a ragged tile add exact zeros and take no part in any sum)"""
    fits = [b for b in ((64, 128, 160, 192, 256) if dtype == BF else (64, 128)) if (rows + b - 1) // b == tiles]
    assert fits, (rows, tiles)
    return min(max(fits), rows)


def _merge64(st):
    """(tiles, K, 3) partial rows -> count, mean, M2 per channel: Chan's formula in float64"""
    st = st.double().cpu()
    n, mean, m2 = (torch.zeros(st.shape[1], dtype=torch.float64) for _ in range(3))
    for t in range(st.shape[0]):
        nb, mb, qb = st[t, :, 0], st[t, :, 1], st[t, :, 2]
        tot = n + nb
        w = torch.where(tot > 0, nb / tot.clamp_min(1), torch.zeros_like(tot))
        d = mb - mean
        mean = mean + d * w
        m2 = m2 + qb + d * d * n * w
        n = tot
    return n, mean, m2


# ---- forward ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_reference(geo, c, k, bf16, offset=0.0, groups=1):
    """Inputs and float64 results (NHWC) of one forward case; computed once, shared, never modified."""
    n, h, w, r, s, stride, pad, dil = geo
    x = torch.randn(n, c, h, w, generator=_gen(100))
    if offset:
        x[:, 0] += offset
    for g in range(groups):                              # every group's mean far from the others'
        x[g * (n // groups):(g + 1) * (n // groups)] += 8.0 * g
    wt = torch.randn(k, c, r, s, generator=_gen(101)) * (2.0 / (c * r * s)) ** 0.5
    x, wt = _rb(x, bf16), _rb(wt, bf16)
    kw = dict(stride=stride, padding=pad, dilation=dil)
    y = F.conv2d(x.double(), wt.double(), None, **kw)
    a = F.conv2d(x.double().abs(), wt.double().abs(), None, **kw)
    scale = torch.randn(k, generator=_gen(102))
    scale[0], scale[1] = -1.25, 0.75
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    shift, bias = torch.randn(k, generator=_gen(103)), torch.randn(k, generator=_gen(104))
    res = _rb(torch.randn(n, y.shape[2], y.shape[3], k, generator=_gen(105)), bf16)
    return dict(x=x, w=wt, y=_cl(y), A=_cl(a), scale=scale, shift=shift, bias=bias, res=res, P=y.shape[2], Q=y.shape[3], L=c * r * s)


def eval_reference(ref, with_affine, with_bias, with_res, relu, bf_out):
    """(float64 result, bound) of section 1"""
    k = ref["scale"].numel()
    sc = ref["scale"].double() if with_affine else torch.ones(k, dtype=torch.float64)
    sh = ref["shift"].double() if with_affine else torch.zeros(k, dtype=torch.float64)
    b = ref["bias"].double() if with_bias else torch.zeros(k, dtype=torch.float64)
    r = ref["res"].double() if with_res else torch.zeros_like(ref["y"])
    pre = ref["y"] * sc + sh + b + r
    out = pre.clamp(min=0) if relu else pre
    mag = sc.abs() * ref["A"] + sh.abs() + b.abs() + r.abs()
    bound = 2 * (ref["L"] + 1) * U * sc.abs() * ref["A"] + 4 * U * mag + (BF_TERM * out.abs() if bf_out else 0.0)
    return out, bound


class _Fwd:
    """device tensors of one forward case"""

    def __init__(self, dev, ref, geo, c, k, dtype):
        self.geo, self.c, self.k, self.dtype, self.dev, self.ref = geo, c, k, dtype, dev, ref
        pad = _pads(dtype)
        self.cp, self.kp = pad(c), pad(k)
        self.x = oc.nhwc(ref["x"], dev, pad_to=self.cp).to(dtype)
        self.w = ref["w"].clone().to(dev)
        self.scale, self.shift, self.bias = (ref[m].clone().to(dev) for m in ("scale", "shift", "bias"))
        self.ldr, self.ldy = self.kp + 8, self.kp + 16
        self.resbuf, self.res = _wide(ref["res"], self.ldr, dtype, dev, math.nan, live=self.kp)
        self.cfg = ops.ConvCfg(geo[5], geo[6], geo[7])

    def out(self, dtype=None):
        n, _, _, _, _, _, _, _ = self.geo
        buf = torch.full((n, self.ref["P"], self.ref["Q"], self.ldy), SENT, dtype=torch.float32).to(dtype or self.dtype).to(self.dev)
        return buf, buf[..., :self.kp]

    def check_y(self, buf, ref64, bound, what, name):
        got = buf.detach().cpu().float()
        assert bool((got[..., self.k:] == SENT).all()), f"{what}: lanes of y past K = {self.k} were written"
        return Worst({name: _ratio(got[..., :self.k], ref64, bound)})


def fwd_eval_case(dev, fam, f32out=False):
    """Section 1: the 16 combinations of {scale + shift, bias, residual, relu} of one kernel family (8 with an fp32 output of
    bf16 storage, which takes no residual)."""
    geo, (c, k), dtype = fam["geo"], fam["ck"], fam["dtype"]
    ref = fwd_reference(geo, c, k, dtype == BF)
    call = _Fwd(dev, ref, geo, c, k, dtype)
    worst = Worst()
    name = "y_bf16" if dtype == BF and not f32out else "y"
    try:
        _tune(**fam["tune"])
        for combo in range(16):
            aff, bia, res, relu = (bool(combo >> i & 1) for i in range(4))
            if f32out and res:
                continue
            what = f"fwd {fam['name']}{' f32out' if f32out else ''} affine={aff} bias={bia} residual={res} relu={relu}"
            buf, view = call.out(F32 if f32out else None)
            c0 = _counters()
            y, d, _ = ops.conv_fwd_raw(call.x, call.w, call.cfg, scale=call.scale if aff else None, shift=call.shift if aff else None,
                                       bias=call.bias if bia else None, residual=call.res if res else None, relu=relu, out=view,
                                       out_f32=f32out)
            _family_proof(_moved(c0), fam["expect"], what)
            assert d.ldy == call.ldy         # (a wrong ldr would read the residual's NaN pad lanes and fail the bound)
            if fam["tune"].get("cu_count") == 3:
                assert _C.lib().up_conv_split_parts(C.byref(d)) > 1, f"{what}: no K-split tail tiles"
            r64, bound = eval_reference(ref, aff, bia, res, relu, dtype == BF and not f32out)
            w = call.check_y(buf, r64, bound, what, name)
            _check(w, what)
            worst.merge(w)
    finally:
        _tune(**DEFAULTS)
    print(f"epilogue fwd {fam['name']}{' f32out' if f32out else ''}: worst got/bound {worst}")
    return worst


def stats_bounds(y64, a64, length, bm):
    """(mean64, M2_64, bound of the mean, bound of M2) per channel from the float64 result and A_dot, both (rows, K): section 2"""
    n = y64.shape[0]
    e = 2 * (length + 1) * U * a64
    em = e.mean(0)
    mean = y64.mean(0)
    cen = y64 - mean
    m2 = (cen * cen).sum(0)
    amax = (y64.abs() + e).amax(0)
    dl = (bm / 2 + 14) * U * amax
    dev = (cen.abs() + e + em).amax(0)
    prop = (2 * cen.abs() * (e + em) + (e + em) ** 2).sum(0)
    b_m2 = prop + (bm / 2 + 15) * U * (m2 + prop) + 6 * n * dev * dl + 3 * n * dl * dl
    return mean, m2, em + dl, b_m2


def _check_counts(st, rows, bm, what):
    cnt = st.cpu()[..., 0]
    assert bool((cnt == cnt[:, :1]).all()), f"{what}: a tile's count differs between channels"
    col = cnt[:, 0].double()
    assert float(col.sum()) == rows, f"{what}: the counts sum to {float(col.sum())}, not {rows}"
    assert float(col.max()) <= bm and (len(col) == 1 or bool((col[:-1] == col[0]).all())), f"{what}: tile counts {col.tolist()}"


def _fold_args(dev, k, gamma, beta, rm0, rv0):
    outs = torch.full((6, k), SENT).to(dev)                 # mean, invstd, scale, shift, running_mean, running_var
    outs[4], outs[5] = rm0.to(dev), rv0.to(dev)
    f = _C.BnFold()
    f.eps, f.momentum = bx.BN_EPS, bx.MOM
    f.gamma, f.beta = gamma.data_ptr(), beta.data_ptr()
    f.mean, f.invstd, f.scale, f.shift, f.running_mean, f.running_var = (outs[i].data_ptr() for i in range(6))
    f.folded = -1
    return f, outs


def fwd_stats_case(dev, fam):
    """Section 2: the partial rows of one family merged in float64 against the statistics of conv64; the folded finalize against
    up_bn_finalize on the same rows (bit for bit) and against float64; bn_fold = 0 leaves the six outputs alone."""
    geo, (c, k), dtype = fam["geo"], fam["ck"], fam["dtype"]
    bf = dtype == BF
    ref = fwd_reference(geo, c, k, bf, OFFSET if fam["name"] in OFFSET_FAMILIES else 0.0)
    call = _Fwd(dev, ref, geo, c, k, dtype)
    rows = geo[0] * ref["P"] * ref["Q"]
    y64, a64 = ref["y"].reshape(rows, k), ref["A"].reshape(rows, k)
    gamma, beta = 0.5 + torch.rand(k, generator=_gen(110)), 0.2 * torch.randn(k, generator=_gen(111))
    rm0, rv0 = 0.1 * torch.randn(k, generator=_gen(112)), 0.5 + torch.rand(k, generator=_gen(113))
    gd, bd = gamma.to(dev), beta.to(dev)
    lib, worst = _C.lib(), Worst()
    sfx = "_bf16" if bf else ""
    what = f"stats {fam['name']}"
    try:
        _tune(**fam["tune"])
        for fold_on in (1, 0):
            _tune(bn_fold=fold_on)
            fold, outs = _fold_args(dev, k, gd, bd, rm0, rv0)
            buf, view = call.out()
            c0 = _counters()
            y, d, st = ops.conv_fwd_raw(call.x, call.w, call.cfg, stats=True, out=view, fold=fold)
            _family_proof(_moved(c0), fam["expect"], what)
            if fam["tune"].get("cu_count") == 3:
                assert lib.up_conv_split_parts(C.byref(d)) > 1, f"{what}: no K-split tail tiles"
            tiles = st.shape[0]
            bm = _tile_rows(rows, tiles, dtype)
            mean64, m2_64, b_mean, b_m2 = stats_bounds(y64, a64, ref["L"], bm)
            _check_counts(st, rows, bm, what)
            cnt, mean, m2 = _merge64(st)
            assert bool((cnt == rows).all()), f"{what}: merged count"
            w = Worst({"mean": _ratio(mean, mean64, b_mean), "M2": _ratio(m2, m2_64, b_m2)})
            w.merge(call.check_y(buf, ref["y"], 2 * (ref["L"] + 1) * U * ref["A"] + (BF_TERM * ref["y"].abs() if bf else 0.0), what,
                                 "y" + sfx))
            if bf and fold_on and fam["name"] == "bf16_glds_1x1":
                # statistics of the ROUNDED output would not pass: the case can tell the two apart (docstring, section 2)
                yr = _rb(y64.float(), True).double()
                mr = yr.mean(0)
                bad = max(_ratio(mr, mean64, b_mean), _ratio(((yr - mr) ** 2).sum(0), m2_64, b_m2))
                assert bad > 4.0, f"{what}: statistics of the rounded y would pass ({bad:.2f} of the bound)"
            var64 = m2_64 / rows
            refs, bounds = bx.propagate(mean64[None], var64[None], rows, (b_mean + U * mean64.abs())[None], (b_m2 / rows)[None],
                                        gamma, beta, rm0, rv0)
            if fold_on:
                assert fold.folded == 1, f"{what}: the launch did not fold the finalize"
                two = torch.full((6, k), SENT).to(dev)
                two[4], two[5] = rm0.to(dev), rv0.to(dev)
                _C.check(lib.up_bn_finalize(st.data_ptr(), tiles, k, bx.BN_EPS, bx.MOM, two[4].data_ptr(), two[5].data_ptr(), gd.data_ptr(),
                                            bd.data_ptr(), two[0].data_ptr(), two[1].data_ptr(), two[2].data_ptr(), two[3].data_ptr(),
                                            ops._stream(st)), "bn_finalize")
                assert torch.equal(outs.cpu(), two.cpu()), f"{what}: the folded finalize differs from up_bn_finalize on the same partial rows"
                o = outs.cpu().double()
                for i, m in enumerate(("mean", "invstd", "scale", "shift", "running_mean", "running_var")):
                    w.add("fold_" + m, _ratio(o[i], refs[m].view(-1), bounds[m].view(-1)))
            else:
                assert fold.folded == 0, f"{what}: bn_fold = 0 still folded"
                o = outs.cpu()
                assert bool((o[:4] == SENT).all()) and torch.equal(o[4], rm0) and torch.equal(o[5], rv0), \
                    f"{what}: bn_fold = 0 wrote the fold's outputs"
            _check(w, f"{what} bn_fold={fold_on}")
            worst.merge(w)
    finally:
        _tune(**DEFAULTS)
    print(f"epilogue {what}: worst got/bound {worst}")
    return worst


def _desc(n, h, w, c, cp, k, kp, r, s, stride, pad, dil, ldx=None, ldy=None):
    d = _C.ConvDesc()
    d.N, d.H, d.W, d.C, d.Cp, d.ldx = n, h, w, c, cp, ldx or cp
    d.K, d.R, d.S, d.stride, d.pad, d.dil = k, r, s, stride, pad, dil
    d.P = (h + 2 * pad - dil * (r - 1) - 1) // stride + 1
    d.Q = (w + 2 * pad - dil * (s - 1) - 1) // stride + 1
    d.Kp, d.ldy = kp, ldy or kp
    return d


def _refused(call, code, text, what):
    lib = _C.lib()
    c0 = _counters()
    e = call()
    assert e == code, f"{what}: returned {e}, expected {code} ({lib.up_last_error().decode()})"
    msg = lib.up_last_error().decode()
    assert text in msg, f"{what}: up_last_error = {msg!r}"
    assert not any(_moved(c0).values()), f"{what}: a refused call launched a kernel"


def fwd_refusal_case(dev, bf16):
    """fill_fwd_args / run_igemm_bf16 refuse before any launch: stats with scale / bias / residual / relu, scale without shift,
    ldr < K, fold without stats, and (bf16 entry) an fp32 output with a residual or statistics."""
    dtype = BF if bf16 else F32
    c, k = 64, 64
    ref = fwd_reference(G_1X1, c, k, bf16)
    call = _Fwd(dev, ref, G_1X1, c, k, dtype)
    lib = _C.lib()
    d = ops.make_desc(call.x, call.w, call.cfg, call.ldy)
    buf, _ = call.out()
    st = torch.full((4, k, 3), SENT).to(dev)
    if bf16:
        wimg = ops._packed_bf16(call.w, d)[0]
    else:
        wimg = ops.packed_fwd(call.w, d)
    gd = torch.ones(k).to(dev)
    fold, outs = _fold_args(dev, k, gd, gd, torch.zeros(k), torch.ones(k))

    def launch(math_=None, **kw):
        ep = _C.ConvEpilogue()
        for key, v in kw.items():
            setattr(ep, key, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        if bf16:
            return lambda: lib.up_conv2d_fwd_bf16(C.byref(d), call.x.data_ptr(), wimg[0].data_ptr(), wimg[1].data_ptr(), buf.data_ptr(),
                                                  C.byref(ep), MATH_BF16S if math_ is None else math_, ops._stream(call.x))
        return lambda: lib.up_conv2d_fwd(C.byref(d), call.x.data_ptr(), wimg.data_ptr(), buf.data_ptr(), C.byref(ep), ops._stream(call.x))

    raw = "stats are taken on the raw accumulator"
    cases = [("stats + scale", launch(stats=st, scale=call.scale, shift=call.shift), raw),
             ("stats + bias", launch(stats=st, bias=call.bias), raw),
             ("stats + residual", launch(stats=st, residual=call.resbuf, ldr=call.ldr), raw),
             ("stats + relu", launch(stats=st, relu=1), raw),
             ("scale without shift", launch(scale=call.scale), "scale without shift"),
             ("ldr < K", launch(residual=call.resbuf, ldr=k - 8), "residual stride < K"),
             ("fold without stats", launch(fold=C.pointer(fold)), "fold needs stats")]
    if bf16:
        cases += [("f32out + residual", launch(MATH_F32OUT, residual=call.resbuf, ldr=call.ldr), "fp32 output"),
                  ("f32out + stats", launch(MATH_F32OUT, stats=st), "fp32 output")]
    for what, fn, text in cases:
        _refused(fn, -1, text, f"fwd refusal ({'bf16' if bf16 else 'fp32'} entry) {what}")
    assert bool((buf.cpu().float() == SENT).all()) and bool((st.cpu() == SENT).all()) and bool((outs.cpu()[:4] == SENT).all()), \
        "a refused call wrote an output"
    gx._plain_conv_ok(dev)


# ---- forward, row groups ------------------------------------------------------------------------------------
GROUPED = [(2, 3, 3, 1), (3, 3, 3, 1), (2, 1, 1, 0), (3, 1, 1, 0)]       # (groups, r, s, pad)


def fwd_grouped_case(dev, groups, r, s, pad, tile_want=100000):
    """up_conv2d_fwd_grouped on `groups` batches of two 10x10 images (200 rows per group: no multiple of 64), every group
    shifted by 8 against the previous one: y against float64, stats[g] merged against the group's own statistics."""
    c, k, per = 32, 64, 2
    geo = (groups * per, 10, 10, r, s, 1, pad, 1)
    ref = fwd_reference(geo, c, k, False, 0.0, groups)
    call = _Fwd(dev, ref, geo, c, k, F32)
    lib = _C.lib()
    d = ops.make_desc(call.x, call.w, call.cfg, call.ldy)
    rows = per * ref["P"] * ref["Q"]
    what = f"fwd grouped groups={groups} {r}x{s}"
    try:
        _tune(glds32=1, glds32_epi=1, tile_want=tile_want)
        tiles = lib.up_conv_stats_tiles_grouped(C.byref(d), groups)
        assert tiles > 0 and rows % 64 != 0, (tiles, rows)
        st = torch.full((groups * tiles + 1, k, 3), SENT).to(dev)               # (the last row must stay)
        buf, _ = call.out()
        wimg = ops.packed_fwd(call.w, d)
        c0 = _counters()
        _C.check(lib.up_conv2d_fwd_grouped(C.byref(d), call.x.data_ptr(), wimg.data_ptr(), buf.data_ptr(), st.data_ptr(), groups,
                                           ops._stream(call.x)), "conv2d_fwd_grouped")
        mv = _moved(c0)
        assert mv["glds32_grouped"] > 0 and mv["igemm"] == 0, mv
    finally:
        _tune(**DEFAULTS)
    assert bool((st.cpu()[groups * tiles:] == SENT).all()), f"{what}: the row behind the partial rows was written"
    w = call.check_y(buf, ref["y"], 2 * (ref["L"] + 1) * U * ref["A"], what, "y")
    bm = _tile_rows(rows, tiles, F32)
    y64, a64 = ref["y"].reshape(groups, rows, k), ref["A"].reshape(groups, rows, k)
    means = []
    for g in range(groups):
        sg = st[g * tiles:(g + 1) * tiles]
        _check_counts(sg, rows, bm, f"{what} group {g}")
        cnt, mean, m2 = _merge64(sg)
        mean64, m2_64, b_mean, b_m2 = stats_bounds(y64[g], a64[g], ref["L"], bm)
        w.add("mean", _ratio(mean, mean64, b_mean))
        w.add("M2", _ratio(m2, m2_64, b_m2))
        means.append(mean64)
    # the groups really are apart: another group's mean is far outside the bound
    assert float((means[1] - means[0]).abs().median()) > 1.0
    _check(w, what)
    print(f"epilogue {what}: worst got/bound {w}")
    return w


def fwd_grouped_refusal_case(dev):
    """up_conv_stats_tiles_grouped = 0 and up_conv2d_fwd_grouped = UP_ERR_UNSUPPORTED, nothing launched: N % groups != 0,
    Cp % 32 != 0, more than 32 taps, glds32_epi = 0."""
    lib = _C.lib()
    buf = torch.full((8 * 10 * 10 * 64,), SENT).to(dev)
    p = buf.data_ptr()
    cases = [("N % groups", _desc(6, 10, 10, 32, 32, 64, 64, 3, 3, 1, 1, 1), 4, {}),
             ("Cp % 32", _desc(6, 10, 10, 12, 12, 64, 64, 3, 3, 1, 1, 1), 2, {}),
             ("more than 32 taps", _desc(6, 10, 10, 32, 32, 64, 64, 7, 7, 1, 3, 1), 2, {}),
             ("glds32_epi = 0", _desc(6, 10, 10, 32, 32, 64, 64, 3, 3, 1, 1, 1), 2, dict(glds32_epi=0))]
    try:
        for what, d, groups, tune in cases:
            _tune(**dict(dict(glds32=1, glds32_epi=1), **tune))
            assert lib.up_conv_stats_tiles_grouped(C.byref(d), groups) == 0, what
            _refused(lambda: lib.up_conv2d_fwd_grouped(C.byref(d), p, p, p, p, groups, None), -2, "cannot be tiled per group",
                     f"fwd grouped refusal {what}")
    finally:
        _tune(**DEFAULTS)
    assert bool((buf.cpu() == SENT).all()), "a refused call wrote through a pointer"
    gx._plain_conv_ok(dev)


# ---- data gradient -------------------------------------------------------------------------------------------
def _dg(name, dtype, n, c, h, w, k, r, pad, dil, tune, add=False, mask_add=False, relu=True, expect=None, groups=1):
    return dict(name=name, dtype=dtype, n=n, c=c, h=h, w=w, k=k, r=r, pad=pad, dil=dil, tune=tune, add=add, mask_add=mask_add, relu=relu,
                expect=expect or {}, groups=groups)


_T64, _T128 = dict(_E1, tile_want=100000), dict(_E1, tile_want=1)
_X_BN = dict(glds32_bnred=True, igemm=False)
_B64, _B128 = dict(glds=1, tile_want_bf16=100000), dict(glds=1, tile_want_bf16=1)
_BIG = dict(glds=1, glds_big=1, tile_want_bf16=1, big_min_k=64)
DGRAD = [
    _dg("f32_1x1", F32, 2, 64, 9, 9, 64, 1, 0, 1, _T64, expect=_X_BN),
    _dg("f32_add", F32, 2, 64, 9, 9, 32, 1, 0, 1, _T64, add=True, expect=_X_BN),
    _dg("f32_masked_add", F32, 2, 64, 9, 9, 32, 1, 0, 1, _T64, add=True, mask_add=True, expect=_X_BN),
    _dg("f32_masked_add_t128", F32, 3, 128, 7, 7, 64, 1, 0, 1, _T128, add=True, mask_add=True, expect=_X_BN),
    _dg("f32_no_relu", F32, 2, 64, 9, 9, 64, 1, 0, 1, _T64, relu=False, expect=_X_BN),
    _dg("f32_3x3_t64", F32, 3, 128, 7, 7, 64, 3, 1, 1, _T64, expect=_X_BN),
    _dg("f32_3x3_t128", F32, 3, 128, 7, 7, 64, 3, 1, 1, _T128, expect=_X_BN),
    _dg("f32_3x3_mixed", F32, 3, 128, 7, 7, 64, 3, 1, 1, dict(_E1, tile_want=3), expect=_X_BN),
    _dg("f32_dead", F32, 4, 64, 7, 7, 64, 3, 3, 3, _T128, add=True, mask_add=True, expect=_X_BN),
    _dg("f32_cu3", F32, 4, 64, 7, 7, 64, 3, 3, 3, dict(_T64, cu_count=3), expect=_X_BN),
    _dg("bf16_1x1", BF, 2, 64, 9, 9, 64, 1, 0, 1, _B64, expect=dict(big=False)),
    _dg("bf16_add", BF, 2, 64, 9, 9, 32, 1, 0, 1, _B64, add=True, expect=dict(big=False)),
    _dg("bf16_masked_add", BF, 2, 64, 9, 9, 32, 1, 0, 1, _B64, add=True, mask_add=True, expect=dict(big=False)),
    _dg("bf16_no_relu", BF, 2, 64, 9, 9, 64, 1, 0, 1, _B64, relu=False, expect=dict(big=False)),
    _dg("bf16_3x3_t128", BF, 3, 128, 7, 7, 64, 3, 1, 1, _B128, expect=dict(big=False)),
    _dg("bf16_3x3_mixed", BF, 3, 128, 7, 7, 64, 3, 1, 1, dict(glds=1, tile_want_bf16=3), expect=dict(big=False)),
    _dg("bf16_dead", BF, 4, 64, 7, 7, 64, 3, 3, 3, _B128, add=True, expect=dict(big=False)),
    _dg("big_1x1", BF, 2, 256, 9, 9, 64, 1, 0, 1, _BIG, expect=dict(big=True)),
    _dg("big_add", BF, 2, 256, 9, 9, 64, 1, 0, 1, _BIG, add=True, expect=dict(big=True)),
    _dg("big_masked_add", BF, 2, 256, 9, 9, 64, 1, 0, 1, _BIG, add=True, mask_add=True, expect=dict(big=True)),
    _dg("big_3x3", BF, 3, 256, 7, 7, 64, 3, 1, 1, _BIG, expect=dict(big=True)),
    _dg("big_tm6_no_relu", BF, 3, 256, 8, 8, 128, 1, 0, 1, dict(_BIG, cu_count=1), relu=False, expect=dict(big=True)),
    _dg("f32_groups2_3x3", F32, 4, 64, 7, 7, 64, 3, 1, 1, _T64, add=True, mask_add=True, expect=_X_BN, groups=2),
    _dg("f32_groups3_1x1", F32, 6, 64, 7, 7, 32, 1, 0, 1, _T64, expect=_X_BN, groups=3),
    _dg("f32_groups3_3x3_t128", F32, 6, 64, 7, 7, 64, 3, 1, 1, _T128, relu=False, expect=_X_BN, groups=3),
]


@functools.lru_cache(maxsize=None)
def dgrad_reference(n, c, h, w, k, r, pad, dil, bf16, groups):
    """Inputs and the float64 data gradient (NHWC) of one case, the BatchNorm operands of the layer being reduced and the two
    masks; computed once, shared, never modified."""
    kw = dict(stride=1, padding=pad, dilation=dil)
    wt = _rb(torch.randn(k, c, r, r, generator=_gen(201)) * (2.0 / (c * r * r)) ** 0.5, bf16)
    p, q = h + 2 * pad - dil * (r - 1), w + 2 * pad - dil * (r - 1)
    dy = _rb(torch.randn(n, k, p, q, generator=_gen(202)), bf16)
    dx = conv2d_input((n, c, h, w), wt.double(), dy.double(), **kw)
    a = conv2d_input((n, c, h, w), wt.double().abs(), dy.double().abs(), **kw)
    add = _rb(torch.randn(n, h, w, c, generator=_gen(203)), bf16)
    # mean / invstd: far apart from channel to channel and from group to group
    mean = (3.0 * torch.randn(groups, c, generator=_gen(204)) + 0.37 * torch.arange(c) + 50.0 * torch.arange(groups).view(-1, 1)).float()
    invstd = (10.0 ** (2 * torch.rand(groups, c, generator=_gen(205)) - 1)).float()
    per = n // groups
    ybn = mean.view(groups, 1, 1, 1, c) + torch.randn(groups, per, h, w, c, generator=_gen(206)) / invstd.view(groups, 1, 1, 1, c)
    ybn = _rb(ybn.reshape(n, h, w, c), bf16)
    zpos = torch.rand(n, h, w, c, generator=_gen(207)) > 0.45
    apos = torch.rand(n, h, w, c, generator=_gen(208)) > 0.45
    return dict(w=wt, dy=dy, dx=_cl(dx), A=_cl(a), add=add, mean=mean, invstd=invstd, ybn=ybn, zpos=zpos, apos=apos, L=k * r * r, P=p, Q=q)


def _dgrad_launch(dev, case, ref, *, fold_pair=True, gsum=True):
    """One up_conv2d_bwd_data_ex call through the C entry.  Returns the device tensors and the slot."""
    n, c, h, w, k, r = (case[m] for m in ("n", "c", "h", "w", "k", "r"))
    dtype, groups = case["dtype"], case["groups"]
    bf = dtype == BF
    math_ = MATH_BF16S if bf else MATH_F32
    kp = _pads(dtype)(k)
    lib = _C.lib()
    x0 = torch.zeros(n, h, w, c, dtype=dtype).to(dev)
    wt = ref["w"].clone().to(dev)
    d = ops.make_desc(x0, wt, ops.ConvCfg(1, case["pad"], case["dil"]))
    dy = oc.nhwc(ref["dy"], dev, pad_to=kp).to(dtype)
    d.ldx, d.ldy = c, kp
    tiles = lib.up_conv2d_bwd_data_tiles_math(C.byref(d), math_)
    assert tiles > 0, "the launch cannot carry the extended epilogue"
    if groups > 1:
        gt = lib.up_conv2d_bwd_data_tiles_grouped(C.byref(d), groups)
        assert gt > 0
        tiles = groups * gt
    ld_add, ld_y = c + 8, c + 16
    addbuf, _ = _wide(ref["add"], ld_add, dtype, dev, math.nan)
    ybuf, _ = _wide(ref["ybn"], ld_y, dtype, dev, math.nan)
    coef = torch.full((groups, 4, c), math.nan)
    coef[:, 0], coef[:, 1] = ref["mean"], ref["invstd"]
    coef = coef.to(dev)
    zbits = bx.pack_bits(ref["zpos"]).to(dev) if case["relu"] else None
    abits = bx.pack_bits(ref["apos"]).to(dev) if case["mask_add"] else None
    partial = torch.full((tiles + 1, c, 2), SENT).to(dev)
    dgb = torch.full((2, c), SENT).to(dev)
    gs = torch.full((groups, 2, c), SENT).to(dev)
    dx = torch.full((n, h, w, c), SENT, dtype=torch.float32).to(dtype).to(dev)
    sl = _C.BnReduceSlot()
    sl.y, sl.relu_bits, sl.mean, sl.invstd = ybuf.data_ptr(), bx._ptr(zbits), coef[0, 0].data_ptr(), coef[0, 1].data_ptr()
    sl.partial, sl.ld, sl.C = partial.data_ptr(), ld_y, c
    sl.group_stride = 4 * c if groups > 1 else 0
    if fold_pair:
        sl.dgamma, sl.dbeta = dgb[0].data_ptr(), dgb[1].data_ptr()
    if groups > 1 and gsum:
        sl.gsum = gs.data_ptr()
    sl.folded = -1
    ep = _C.DgradEpilogue()
    ep.add, ep.add_relu_bits, ep.ld_add = (addbuf.data_ptr() if case["add"] else None), bx._ptr(abits), (ld_add if case["add"] else 0)
    ep.bn = C.pointer(sl)
    ep.groups = groups
    wimg = ops._packed_bf16(wt, d)[1][0] if bf else ops.packed_dgrad(wt, d)
    c0 = _counters()
    _C.check(lib.up_conv2d_bwd_data_ex(C.byref(d), dy.data_ptr(), wimg.data_ptr(), dx.data_ptr(), C.byref(ep), math_, ops._stream(dy)),
             "conv2d_bwd_data_ex")
    _family_proof(_moved(c0), case["expect"], "dgrad " + case["name"])
    keep = (x0, wt, dy, addbuf, ybuf, coef, zbits, abits, wimg)
    return dict(dx=dx, partial=partial, dgb=dgb, gsum=gs, folded=sl.folded, tiles=tiles, keep=keep)


def dgrad_case(dev, case):
    """Section 3: dx against float64; the partial rows, the folded dgamma / dbeta (/ gsum) against float64 sums of the launch's own
    stored dx; bn_fold = 0 (and a grouped launch without gsum) leaves the pair alone."""
    n, c, h, w, k, r = (case[m] for m in ("n", "c", "h", "w", "k", "r"))
    dtype, groups = case["dtype"], case["groups"]
    bf = dtype == BF
    ref = dgrad_reference(n, c, h, w, k, r, case["pad"], case["dil"], bf, groups)
    worst = Worst()
    sfx = "_bf16" if bf else ""
    rows_g = (n // groups) * h * w
    forms = [("fold", 1, True)] + ([("no gsum", 1, False)] if groups > 1 else []) + [("bn_fold=0", 0, True)]
    try:
        _tune(**case["tune"])
        for form, fold_on, with_gsum in forms:
            _tune(bn_fold=fold_on)
            what = f"dgrad {case['name']} {form}"
            out = _dgrad_launch(dev, case, ref, gsum=with_gsum)
            tiles = out["tiles"]
            # dx
            live_add = ref["add"].double() * (ref["apos"].double() if case["mask_add"] else 1.0) if case["add"] else torch.zeros_like(ref["dx"])
            dx64 = ref["dx"] + live_add
            bound = 2 * (ref["L"] + 1) * U * ref["A"] + 2 * U * live_add.abs() + (BF_TERM * dx64.abs() if bf else 0.0)
            got = out["dx"].cpu().float().double()
            w_ = Worst({"dx" + sfx: _ratio(got, dx64, bound)})
            assert bool((ref["A"] > 0).all())        # (no unreached pixel in these cases: docstring, section 3)
            # sums, from the stored dx
            g = (got * (ref["zpos"].double() if case["relu"] else 1.0)).view(groups, rows_g, c)
            mean, invstd = ref["mean"].double().view(groups, 1, c), ref["invstd"].double().view(groups, 1, c)
            cen = ref["ybn"].double().view(groups, rows_g, c) - mean
            s1, s2 = g.sum(1), invstd[:, 0] * (g * cen).sum(1)
            gt = tiles // groups
            bm = _tile_rows(rows_g, gt, dtype)
            b1 = bm * U * g.abs().sum(1)
            b2 = (bm + 4) * U * invstd[:, 0] * (g * cen).abs().sum(1)
            part = out["partial"].cpu()
            assert bool((part[tiles:] == SENT).all()), f"{what}: the row behind the partial rows was written"
            p64 = part[:tiles].double().view(groups, gt, c, 2)
            w_.add("S1", _ratio(p64[..., 0].sum(1), s1, b1))
            w_.add("S2", _ratio(p64[..., 1].sum(1), s2, b2))
            pabs = p64.abs().sum(1)
            dgb, gs = out["dgb"].cpu(), out["gsum"].cpu()
            if fold_on and with_gsum:
                assert out["folded"] == 1, f"{what}: the launch did not finish dgamma / dbeta"
                merge = gt * U * pabs                     # per group: its tiles, its partial rows
                if groups > 1:
                    w_.add("gsum", max(_ratio(gs[:, 1], s1, b1 + merge[..., 0]), _ratio(gs[:, 0], s2, b2 + merge[..., 1])))
                else:
                    assert bool((gs == SENT).all()), f"{what}: gsum written without row groups"
                w_.add("dbeta", _ratio(dgb[1], s1.sum(0), (b1 + merge[..., 0]).sum(0)))
                w_.add("dgamma", _ratio(dgb[0], s2.sum(0), (b2 + merge[..., 1]).sum(0)))
            else:
                assert out["folded"] == 0, f"{what}: folded = {out['folded']}"
                assert bool((dgb == SENT).all()) and bool((gs == SENT).all()), f"{what}: dgamma / dbeta / gsum written by a launch that did not fold"
            _check(w_, what)
            worst.merge(w_)
    finally:
        _tune(**DEFAULTS)
    print(f"epilogue dgrad {case['name']}: worst got/bound {worst}")
    return worst


def dgrad_refusal_case(dev):
    """The head of up_conv2d_bwd_data_ex refuses before fill_dgrad_args and any launch: add_relu_bits without add, dgamma without
    dbeta, slot.C != d->C, a slot on a stride-2 descriptor, a slot where up_conv2d_bwd_data_tiles_math = 0 (K = 48), row groups
    in bf16 storage."""
    lib = _C.lib()
    buf = torch.full((1 << 16,), SENT).to(dev)
    p = buf.data_ptr()

    def call(d, math_=MATH_F32, groups=1, slot=None, **kw):
        ep = _C.DgradEpilogue()
        for key, v in kw.items():
            setattr(ep, key, v)
        sl = None
        if slot is not None:
            sl = _C.BnReduceSlot()
            sl.y = sl.mean = sl.invstd = sl.partial = p
            sl.ld, sl.C = d.C, d.C
            for key, v in slot.items():
                setattr(sl, key, v)
            ep.bn = C.pointer(sl)
        ep.groups = groups
        return lambda: (lib.up_conv2d_bwd_data_ex(C.byref(d), p, p, p, C.byref(ep), math_, None), sl)[0]

    d1 = _desc(2, 9, 9, 64, 64, 64, 64, 1, 1, 1, 0, 1)
    d2 = _desc(2, 9, 9, 64, 64, 64, 64, 3, 3, 2, 1, 1)
    d48 = _desc(2, 9, 9, 64, 64, 48, 48, 1, 1, 1, 0, 1)
    d4 = _desc(4, 7, 7, 64, 64, 64, 64, 3, 3, 1, 1, 1)
    try:
        _tune(glds32=1, glds32_epi=1, glds=1)
        for d in (d1, d4):
            assert lib.up_conv2d_bwd_data_tiles_math(C.byref(d), MATH_F32) > 0 and lib.up_conv2d_bwd_data_tiles_math(C.byref(d), MATH_BF16S) > 0
        assert lib.up_conv2d_bwd_data_tiles_math(C.byref(d2), MATH_F32) == 0 and lib.up_conv2d_bwd_data_tiles_math(C.byref(d48), MATH_F32) == 0
        assert lib.up_conv2d_bwd_data_tiles_grouped(C.byref(d4), 2) > 0
        cases = [("add_relu_bits without add", call(d1, add_relu_bits=p), -1, "add_relu_bits without an addend"),
                 ("dgamma without dbeta", call(d1, slot=dict(dgamma=p)), -1, "dgamma and dbeta"),
                 ("slot.C != d->C", call(d1, slot=dict(C=32)), -1, "bad BatchNorm slot"),
                 ("slot, stride 2", call(d2, slot={}), -2, "up_conv2d_bwd_data_tiles_math = 0"),
                 ("slot, K = 48", call(d48, slot={}), -2, "up_conv2d_bwd_data_tiles_math = 0"),
                 ("row groups in bf16 storage", call(d4, MATH_BF16S, 2, slot=dict(group_stride=256)), -2, "cannot be tiled per row group")]
        for what, fn, code, text in cases:
            _refused(fn, code, text, f"dgrad refusal {what}")
    finally:
        _tune(**DEFAULTS)
    assert bool((buf.cpu() == SENT).all()), "a refused call wrote through a pointer"
    gx._plain_conv_ok(dev)
