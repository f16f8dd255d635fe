"""Every BatchNorm entry of the C ABI on its own, against float64, per element and per channel, at the smallest shapes that reach
each code path of norm_act.hip / bn_fold.h (shared by test_bn_emu.py and test_bn_gpu.py).

Each pass is isolated: its reference is evaluated in float64 from exactly the inputs the kernel receives (the fp32 coefficient
vectors as given, tensors rounded to bf16 first for bf16 storage), ReLU masks are drawn on the host (or come from planted +0.0 /
-0.0 / tiny values of z on the ZPATH), so no near-zero forward value can flip anything.  Nothing is compared with a tensor-wide
maximum.  u = 2^-24; every bound is (roundings) * u * (the same expression on absolute values), none carries a slack factor.

Inputs (make_input): per-channel scales from 1e-3 to 1e3, channel 0 with |mean| / std = 4000, channel 1 constant (var = 0),
channel 2 with gamma = 0, channel 3 with gamma < 0, outliers of 8 std in rows 0, 127, 128, 255, 256 and L - 1 of every group, the
groups shifted against each other.  Input pad lanes (ld > C) hold NaN, output pad lanes and the words behind relu_bits a sentinel.

Apply (z = relu?((y - mu) s + b (+ r)), mu = 0 in the uncentred form): one rounding each for the difference, the product and
the one or two sums:
    |z - relu?(pre64)| <= 4 u (|y - mu| |s| + |b| + |r|)  (+ 2^-8 |z64| for a result stored as bf16)
ReLU is 1-Lipschitz, so no element is excluded.  s = 0 gives fl(b + r) exactly.  relu_bits == (z_device > 0) bit for bit.

Statistics.  L rows per group, dev = max_r |y - mean64|.
    mean:   |mean - mean64| <= u (2 |mean64| + 4 (L + 1) dev)                                             =: Bm
    M2:     bn_batch_stats_kernel sums d = y - sh and d^2 per thread (n <= 16 rows of a 256-row chunk, sh = the chunk's first
            row), forms q - s^2 / n and merges 16 lanes (Welford, fp32); the chunks are merged in double.  With S = sum_r d_r^2:
            |fl(q) - q| <= (n + 2) u q, |fl(s^2 / n) - s^2 / n| <= 2 (n + 1) u (sum |d|)^2 / n <= 2 (n + 1) u q (Cauchy-Schwarz),
            every lane merge rounds the running M2 and one product d^2 n1 n2 / n (<= 4 u each, 16 merges, all terms <= S):
            |M2 - M2_64| <= (3 n + 4 + 64) u S = 116 u S at n = 16.  The fp32 lane merges also round the running mean: after j
            merges it is off by up to (j + 1) u max|y|, and the next merge's d^2 n1 n2 / n takes d from that rounded mean while the
            running M2 is about the unrounded one: a FIRST-order error 2 |d| (n1 n2 / n) (j + 1) u max|y| with |d| <= 2 dev and
            n1 n2 / n <= n; summed over the 15 merges of a chunk of 16 n rows: 4 dev n u max|y| 135 <= 34 u rows dev max|y|.
            (Found by the first run of these tests: the |mean| / std = 4000 channel exceeded 116 u S alone by 1.44; the term only
            loosens channels with a large |mean| / std, where the fp32 Welford chain really is that inexact.)  With the centre's own
            error L Bm^2 (second order, kept):   BM = 116 u S + 34 u L dev max|y| + L Bm^2.
            Beyond BN_MAXG groups bn_finalize_kernel merges the chunks in fp32 as well; the cases here have one chunk per group
            there (asserted), so that tree adds no rounding.
            up_bn_exact_stats_t (double two-pass): mean == float32(mean64) exactly, |M2 - M2_64| <= u M2_64 (one rounding).
    var = M2 / L, Bv = BM / L.  To first order, with 4 roundings for fl(var) + eps, sqrt and 1 / x:
    invstd: |invstd / invstd64 - 1| <= Bv / (2 (var + eps)) + 4 u                                        =: ri
    scale = gamma invstd:            |scale - scale64| <= (ri + u) |scale64|                            =: Bs
    shift = beta - mean scale:       |shift - shift64| <= |scale64| Bm + |mean64| Bs + u |mean64 scale64| + u |shift64|
    running_mean' = (1 - m) rm + m mean, per group in order:  B' = (1 - m) B + m Bm + 3 u (|(1 - m) rm| + |m mean|)
    running_var'  = (1 - m) rv + m unb, unb = M2 / (L - 1) (the UNBIASED variance).  Beyond BN_MAXG groups the kernel recovers
            var = 1 / invstd^2 - eps: |d var| <= 2 (var + eps) ri + 4 u (var + eps); the bound takes that (larger) form everywhere:
            Bunb = (2 (var + eps) (ri + 2 u)) L / (L - 1) + 2 u unb;   B' = (1 - m) B + m Bunb + 3 u (|(1 - m) rv| + |m unb|)
Synthetic partial rows (count, mean, M2) -> up_bn_finalize / up_bn_finalize_groups: the merge runs in double precision, so the
results match the float64 merge of the same fp32 partials: |mean - mean64| <= u |mean64|, |invstd / invstd64 - 1| <= 4 u; the
other outputs follow from the formulas above with Bm = u |mean64|, Bv = 0.

Backward.  g = dz mask, k = gamma invstd, xhat = (y - mean) invstd, M = L:
    dres == where(mask, dz, 0) exactly
    |dbeta - sum g| <= 2 (L + 1) u sum |g|                                         =: Bb
    |dgamma - invstd sum g (y - mean)| <= 2 (L + 3) u |invstd| sum |g| |y - mean|   =: Bg
    dy64 = k (g - dbeta64 / M - xhat dgamma64 / M);  |dy - dy64| <= |k| (Bb + |xhat| Bg) / M
                                                      + 6 u |k| (|g| + |dbeta64| / M + |xhat| |dgamma64| / M)  (+ 2^-8 |dy64| in bf16)
    use_batch_stats = 0: |dy - k g| <= 2 u |k g| (+ 2^-8 |k g| in bf16); dgamma / dbeta as above.
    a channel whose mask is all zero: dgamma == dbeta == 0 and dy == 0.
    up_bn_bwd_finalized_t / up_bn_bwd_groups_finalized_t take fp32 sums as inputs: the reference uses those, Bb = Bg = 0.
    grouped: every group's dy from its own sums; dgamma / dbeta = the sums over the groups, bound = the groups' bounds summed
    + (G + 1) u sum_g |.| for the summation.
    up_bn_bwd_acc_t: two calls onto accumulators that start at 3.25: bit-equal to fl(fl(a0 + d1) + d2) of the device's own d1, d2.

Not as the issue states it: up_bn_exact_stats_t asks for |y| < 2^10 AND a channel with mean ~ 4000; that channel is below 2^13
instead, which keeps the double sum of <= 4096 multiples of 2^-10 exact (13 + 10 + 12 = 35 bits).
"""
import functools
import math

import torch

from unipose_amd import _C, ops

BF = torch.bfloat16
F32 = torch.float32
U = 2.0 ** -24
BF_TERM = 2.0 ** -8
BN_EPS = 1e-5
MOM = 0.1
SENT = 7.0                    # output pad lanes
WORD_SENT = 0x5A5A5A5A        # words behind the live relu_bits
BN_MAXG = 8
TUNE_DEFAULTS = dict(bn_rows=1, bn_fold=1)
OUTLIER_ROWS = (0, 127, 128, 255, 256, -1)

# (dtype, C, rows, ld step): every tensor of a call gets its own leading dimension C + step * i
_FLAT = [(F32, c, r, 4) for c in (4, 12, 48) for r in (1, 2, 7, 9, 130, 257)]
_ROWS = [(F32, 32, r, 4) for r in (1, 31, 33, 127, 128, 129, 255, 256, 257, 515)]
_COLS = [(F32, 68, 257, 4), (F32, 1024, 9, 4), (F32, 2048, 5, 4)]
_BIG = [(F32, 32, 8449, 4)]
_BF_FLAT = [(BF, c, r, 4) for c in (4, 12, 24) for r in (9, 130)]
_BF_8 = [(BF, c, r, 8) for c in (8, 24, 32, 40) for r in (1, 9, 130, 257)]
_BF_ROWS = [(BF, 64, r, 8) for r in (1, 31, 129, 257)] + [(BF, 2048, 5, 8)]
_DENSE = [(F32, 12, 130, 0), (F32, 32, 257, 0), (BF, 24, 130, 0), (BF, 64, 257, 0)]
SHAPES = _FLAT + _ROWS + _COLS + _BIG + _BF_FLAT + _BF_8 + _BF_ROWS + _DENSE
# statistics read y only: one leading dimension; rows = L of one group
STATS_SHAPES = [s for s in SHAPES if s not in _DENSE]
ACC_SHAPES = [(F32, 4, 9, 4), (F32, 12, 130, 4), (F32, 32, 257, 4), (F32, 68, 257, 4), (BF, 12, 130, 4), (BF, 24, 130, 8), (BF, 64, 257, 8)]
PREREDUCED_SHAPES = [(F32, 12, 130, 4), (F32, 32, 257, 4), (F32, 68, 257, 4), (BF, 64, 257, 8)]
EXACT = [(1, 1, 4), (1, 2, 5), (3, 7, 12), (1, 9, 260), (3, 130, 8), (1, 4096, 4)]      # (groups, rows per group, C)
# (groups, rows per group, C, dtype)
GROUPS = [(2, 8, 4, F32), (2, 24, 12, F32), (3, 129, 32, F32), (8, 257, 32, F32), (8, 257, 64, BF), (9, 33, 32, F32),
          (9, 16, 12, F32)]
FINALIZE_TILES = (1, 2, 31, 32, 33, 64, 65, 513, 545)
FINALIZE_C = (4, 68, 132)
PREREDUCED_CHUNKS = (1, 33, 67)


def shape_id(s):
    return "%s_c%d_r%d_ld%d" % ("bf16" if s[0] == BF else "f32", s[1], s[2], s[3])


def group_id(s):
    return "g%d_r%d_c%d_%s" % (s[0], s[1], s[2], "bf16" if s[3] == BF else "f32")


def _gen(seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return gen


def _tune(**kw):
    for k, v in kw.items():
        _C.check(_C.lib().up_conv_tune(k.encode(), int(v)), k)


def _has_rows_geometry(c, dtype):
    e = 8 if dtype == BF else 4
    cgs = c // e
    return c % e == 0 and cgs >= 8 and (cgs & (cgs - 1)) == 0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dt(dtype):
    return 1 if dtype == BF else 0


def _sfx(dtype):
    """bf16 results fill the 2^-8 term of their bounds (one stored rounding): reported apart from the fp32 ones"""
    return "_bf16" if dtype == BF else ""


def _rt(t, dtype):
    """the fp32 values a tensor of `dtype` can hold"""
    return t.to(dtype).float()


class Worst(dict):
    """worst got / bound ratio per quantity"""

    def add(self, name, ratio):
        self[name] = max(self.get(name, 0.0), float(ratio))

    def merge(self, other):
        for k, v in other.items():
            self.add(k, v)

    def __str__(self):
        return " ".join(f"{k}={v:.3f}" for k, v in sorted(self.items()))


def _ratio(got, ref64, bound):
    """worst |got - ref64| / bound; where the bound is 0 the value must be exact (inf otherwise, as for a NaN)"""
    got, ref64, bound = got.double(), ref64.double(), bound.double().expand_as(ref64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if bool(torch.isnan(got).any()):
        return math.inf
    err = (got - ref64).abs()
    zero = bound == 0
    if bool(zero.any()) and float(err[zero].max()) != 0.0:
        return math.inf
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def _check(worst, what):
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: got / bound above 1: {bad} (all: {worst})"


# ---- inputs ---------------------------------------------------------------------------------------------
def make_input(groups, L, C, dtype, seed=0):
    """y (groups * L, C) as fp32 values representable in `dtype`, gamma, beta (see the module docstring)"""
    gen = _gen(seed)
    std = 10.0 ** (-3 + 6 * torch.rand(C, generator=gen, dtype=torch.float64))
    std[C - 1], std[C - 2] = 1e3, 1e-3
    mean = std * torch.randn(C, generator=gen, dtype=torch.float64)
    std[0], mean[0] = 1.0, 4000.0
    y = mean + std * torch.randn(groups * L, C, generator=gen, dtype=torch.float64)
    sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0).double()
    for g in range(groups):
        for r in OUTLIER_ROWS:
            if r < L:
                y[g * L + (r % L)] = mean + 8 * std * sign * (1 if r % 2 else -1)
        y[g * L:(g + 1) * L] += 0.75 * g * std
        y[g * L:(g + 1) * L, 1] = 2.5 + g
    gamma = 0.5 + torch.rand(C, generator=gen)
    gamma[2], gamma[3] = 0.0, -0.7
    beta = 0.2 * torch.randn(C, generator=gen)
    return _rt(y.float(), dtype), gamma, beta


def stats64(y, groups, L):
    y64 = y.double().view(groups, L, -1)
    mean = y64.mean(1)
    cen = y64 - mean[:, None]
    return dict(mean=mean, M2=(cen * cen).sum(1), dev=cen.abs().amax(1), var=(cen * cen).sum(1) / L)


def coefficients(y, gamma, beta, groups, L):
    """fp32 coef[groups][4][C] = mean, invstd, scale, shift as a correct finalize would give them"""
    s = stats64(y, groups, L)
    invstd = 1.0 / torch.sqrt(s["var"] + BN_EPS)
    scale = gamma.double() * invstd
    return torch.stack([s["mean"], invstd, scale, beta.double() - s["mean"] * scale], 1).float().contiguous()


def pack_bits(pos, extra_words=4):
    """dense bit array of a flat bool tensor (bit i of the array = pos[i]) + sentinel words behind it, as int32"""
    n = pos.numel()
    words = (n + 31) // 32
    b = torch.zeros(words * 32, dtype=torch.int64)
    b[:n] = pos.reshape(-1).long()
    w = (b.view(-1, 32) << torch.arange(32)).sum(1)
    w = torch.cat([w, torch.full((extra_words,), WORD_SENT, dtype=torch.int64)])
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bits(words, n):
    w = words.cpu().to(torch.int64) & 0xFFFFFFFF
    return ((w.view(-1, 1) >> torch.arange(32)) & 1).reshape(-1)[:n].bool()


def _padded(x, ld, dtype, dev, fill):
    rows, c = x.shape
    out = torch.full((rows, ld), fill, dtype=torch.float32)
    out[:, :c] = x
    return out.to(dtype).to(dev)


def _lds(c, step, n):
    return [c + step * (i % 4) for i in range(n)]


def _live(t, c):
    return t.cpu().float()[:, :c]


def _pads_kept(t, c, fill=SENT):
    return t.shape[1] == c or bool((t.cpu().float()[:, c:] == fill).all())


# ---- apply ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _apply_inputs(groups, L, C, dtype):
    y, gamma, beta = make_input(groups, L, C, dtype, seed=1)
    coef = coefficients(y, gamma, beta, groups, L)
    res = _rt(torch.randn(groups * L, C, generator=_gen(2)) * y.abs().mean(0).clamp(max=10.0), dtype)
    return y, gamma, beta, coef, res


def apply_case(dev, shape, groups=1):
    """up_bn_apply_t / up_bn_apply_centered_t (groups = 1) or up_bn_apply_groups_t with and without beta: relu x residual x
    bn_rows, z and relu_bits against float64, pad lanes and the words behind the bits untouched."""
    dtype, C, L, step = shape
    rows = groups * L
    y, gamma, beta, coef, res = _apply_inputs(groups, L, C, dtype)
    ldy, ldr, ldz = _lds(C, step, 4)[1:]
    yd, rd = _padded(y, ldy, dtype, dev, math.nan), _padded(res, ldr, dtype, dev, math.nan)
    cd, bd = coef.to(dev), beta.to(dev)
    lib, st = _C.lib(), ops._stream(yd)
    y64, r64 = y.double().view(groups, L, C), res.double().view(groups, L, C)
    mu, s, h, b = (coef[:, 0, None].double(), coef[:, 2, None].double(), coef[:, 3, None].double(), beta.double().view(1, 1, C))
    worst = Worst()
    nwords = (rows * C + 31) // 32
    try:
        for bn_rows in ((1, 0) if _has_rows_geometry(C, dtype) and groups == 1 else (1,)):
            _tune(bn_rows=bn_rows)
            for centred in (True, False):
                for relu in (1, 0):
                    for with_res in (True, False):
                        want_bits = bool(relu or with_res)
                        z = torch.full((rows, ldz), SENT, dtype=torch.float32).to(dtype).to(dev)
                        bits = torch.full((nwords + 4,), WORD_SENT, dtype=torch.int64).to(torch.int32).to(dev) if want_bits else None
                        r_ = rd if with_res else None
                        if groups == 1 and centred:
                            e = lib.up_bn_apply_centered_t(yd.data_ptr(), ldy, cd[0, 0].data_ptr(), cd[0, 2].data_ptr(), bd.data_ptr(),
                                                           _ptr(r_), ldr, relu, z.data_ptr(), ldz, _ptr(bits), rows, C, _dt(dtype), st)
                        elif groups == 1:
                            e = lib.up_bn_apply_t(yd.data_ptr(), ldy, cd[0, 2].data_ptr(), cd[0, 3].data_ptr(), _ptr(r_), ldr, relu,
                                                  z.data_ptr(), ldz, _ptr(bits), rows, C, _dt(dtype), st)
                        else:
                            e = lib.up_bn_apply_groups_t(yd.data_ptr(), ldy, cd.data_ptr(), bd.data_ptr() if centred else None, _ptr(r_),
                                                         ldr, relu, z.data_ptr(), ldz, _ptr(bits), L, C, groups, _dt(dtype), st)
                        _C.check(e, "bn_apply")
                        what = f"apply {shape_id(shape)} groups={groups} centred={centred} relu={relu} res={with_res} bn_rows={bn_rows}"
                        pre = (y64 - mu) * s + b if centred else y64 * s + h
                        a = ((y64 - mu).abs() * s.abs() + b.abs()) if centred else (y64.abs() * s.abs() + h.abs())
                        if with_res:
                            pre, a = pre + r64, a + r64.abs()
                        z64 = pre.clamp(min=0) if relu else pre
                        bound = 4 * U * a + (BF_TERM * z64.abs() if dtype == BF else 0.0)
                        zl = _live(z, C)
                        w = Worst({"z" + _sfx(dtype): _ratio(zl.view(groups, L, C), z64, bound)})
                        # s = 0 (gamma = 0, channel 2): fl(b + r), stored
                        add = (beta if centred else coef[:, 3]).view(-1, 1, C).expand(groups, L, C)[..., 2]
                        e2 = add + res.view(groups, L, C)[..., 2] if with_res else add
                        e2 = _rt(e2.clamp(min=0) if relu else e2, dtype)
                        assert torch.equal(zl.view(groups, L, C)[..., 2], e2), f"{what}: the gamma = 0 channel is not fl(b + r)"
                        assert _pads_kept(z, C), f"{what}: pad lanes of z written"
                        if want_bits:
                            assert torch.equal(unpack_bits(bits[:nwords], rows * C), (zl > 0).reshape(-1)), f"{what}: relu_bits != (z > 0)"
                            assert bool((bits[nwords:].cpu() == WORD_SENT).all()), f"{what}: words behind relu_bits written"
                        _check(w, what)
                        worst.merge(w)
    finally:
        _tune(**TUNE_DEFAULTS)
    print(f"bn apply {shape_id(shape)} groups={groups}: worst got/bound {worst}")
    return worst


def groups_refusal_case(dev):
    """relu_bits with rows_per_group * C % 32 != 0: UP_ERR_UNSUPPORTED from the grouped apply and backward, outputs untouched."""
    groups, L, C = 2, 7, 4
    y, gamma, beta, coef, _ = _apply_inputs(groups, L, C, F32)
    yd, cd, bd, gd = y.to(dev), coef.to(dev), beta.to(dev), gamma.to(dev)
    z = torch.full((groups * L, C), SENT).to(dev)
    bits = pack_bits(torch.zeros(groups * L * C, dtype=torch.bool), 0).fill_(WORD_SENT).to(dev)
    lib, st = _C.lib(), ops._stream(yd)
    e = lib.up_bn_apply_groups_t(yd.data_ptr(), C, cd.data_ptr(), bd.data_ptr(), None, 0, 1, z.data_ptr(), C, bits.data_ptr(), L, C,
                                 groups, 0, st)
    assert e == -2, e                                   # UP_ERR_UNSUPPORTED
    assert "multiple of 32" in lib.up_last_error().decode()
    dy, dg = torch.full((groups * L, C), SENT).to(dev), torch.full((2, C), SENT).to(dev)
    nbytes = lib.up_bn_bwd_groups_workspace(L, C, groups)
    ws = torch.zeros(nbytes // 4 + 1).to(dev)
    e = lib.up_bn_bwd_groups_t(yd.data_ptr(), C, bits.data_ptr(), yd.data_ptr(), C, gd.data_ptr(), cd.data_ptr(), 1, dy.data_ptr(), C,
                               None, 0, dg[0].data_ptr(), dg[1].data_ptr(), ws.data_ptr(), nbytes, L, C, groups, 0, st)
    assert e == -2, e
    for t in (z, dy, dg):
        assert bool((t.cpu() == SENT).all()), "a refused call wrote an output"
    assert bool((bits.cpu() == WORD_SENT).all()), "a refused call wrote relu_bits"


# ---- statistics and finalize ----------------------------------------------------------------------------
def propagate(mean, var, L, b_mean, b_var, gamma, beta, rm0, rv0, unb=None):
    """float64 coefficients and their first-order bounds from the statistics (groups, C) and their bounds (module docstring).
    Returns (refs, bounds): dicts of mean, invstd, scale, shift (per group) and running_mean, running_var (after all groups)."""
    g64, b64 = gamma.double(), beta.double()
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    ri = b_var / (2 * (var + BN_EPS)) + 4 * U
    scale = g64 * invstd
    shift = b64 - mean * scale
    b_scale = (ri + U) * scale.abs()
    b_shift = scale.abs() * b_mean + mean.abs() * b_scale + U * (mean * scale).abs() + U * shift.abs()
    if unb is None:
        unb = var * L / (L - 1) if L > 1 else var
    b_unb = 2 * (var + BN_EPS) * (ri + 2 * U) * (L / (L - 1) if L > 1 else 1.0) + 2 * U * unb
    rm, rv = rm0.double(), rv0.double()
    brm, brv = torch.zeros_like(rm), torch.zeros_like(rv)
    for g in range(mean.shape[0]):
        brm = (1 - MOM) * brm + MOM * b_mean[g] + 3 * U * (((1 - MOM) * rm).abs() + (MOM * mean[g]).abs())
        brv = (1 - MOM) * brv + MOM * b_unb[g] + 3 * U * (((1 - MOM) * rv).abs() + (MOM * unb[g]).abs())
        rm = (1 - MOM) * rm + MOM * mean[g]
        rv = (1 - MOM) * rv + MOM * unb[g]
    return (dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv),
            dict(mean=b_mean, invstd=ri * invstd, scale=b_scale, shift=b_shift, running_mean=brm, running_var=brv))


def _check_coef(coef, rm, rv, refs, bounds, what, tag=""):
    """tag: the merge-only cases report apart (a correctly rounded mean is up to 1.0 of its bound u |mean64|)"""
    co = coef.cpu().double()
    w = Worst()
    for i, name in enumerate(("mean", "invstd", "scale", "shift")):
        w.add(name + tag, _ratio(co[:, i], refs[name], bounds[name]))
    w.add("running_mean" + tag, _ratio(rm.cpu(), refs["running_mean"], bounds["running_mean"]))
    w.add("running_var" + tag, _ratio(rv.cpu(), refs["running_var"], bounds["running_var"]))
    _check(w, what)
    return w


def _running0(C, dev):
    rm0, rv0 = 0.1 * torch.randn(C, generator=_gen(5)), 0.5 + torch.rand(C, generator=_gen(6))
    return rm0, rv0, rm0.clone().to(dev), rv0.clone().to(dev)


def stats_case(dev, shape, groups=1):
    """up_bn_batch_stats_t -> up_bn_finalize (groups = 1) / up_bn_finalize_groups, and up_bn_stats_groups_t with bn_fold 1 / 0,
    from the tensor itself: counts exact, every coefficient and the running statistics inside the propagated bounds."""
    dtype, C, L, step = shape
    y, gamma, beta = make_input(groups, L, C, dtype, seed=3)
    ld = C + step
    yd, gd, bd = _padded(y, ld, dtype, dev, math.nan), gamma.to(dev), beta.to(dev)
    lib, st = _C.lib(), ops._stream(yd)
    s = stats64(y, groups, L)
    tiles = lib.up_bn_batch_stats_tiles(L)
    assert tiles == (L + 255) // 256
    # S = sum of squares about the shift the kernel uses: the first row of every 256-row chunk
    y64 = y.double().view(groups, L, C)
    first = y64[:, torch.arange(L) // 256 * 256]
    S = ((y64 - first) ** 2).sum(1)
    b_mean = U * (2 * s["mean"].abs() + 4 * (L + 1) * s["dev"])
    assert groups <= BN_MAXG or tiles == 1, "the M2 bound does not cover bn_finalize_kernel's fp32 tree over several chunks"
    b_var = (116 * U * S + 34 * U * L * s["dev"] * y64.abs().amax(1) + L * b_mean ** 2) / L
    rm0, rv0, _, _ = _running0(C, dev)
    refs, bounds = propagate(s["mean"], s["var"], L, b_mean, b_var, gamma, beta, rm0, rv0)
    worst = Worst()
    what = f"stats {shape_id(shape)} groups={groups}"
    try:
        for form in ("two launches", "fold", "no fold"):
            stats = torch.full((groups, tiles, C, 3), SENT).to(dev)
            coef = torch.full((groups, 4, C), SENT).to(dev)
            _, _, rm, rv = _running0(C, dev)
            if form == "two launches":
                _C.check(lib.up_bn_batch_stats_t(yd.data_ptr(), ld, L, C, groups, _dt(dtype), stats.data_ptr(), st), "bn_batch_stats")
                if groups == 1:
                    _C.check(lib.up_bn_finalize(stats.data_ptr(), tiles, C, BN_EPS, MOM, rm.data_ptr(), rv.data_ptr(), gd.data_ptr(),
                                                bd.data_ptr(), coef[0, 0].data_ptr(), coef[0, 1].data_ptr(), coef[0, 2].data_ptr(),
                                                coef[0, 3].data_ptr(), st), "bn_finalize")
                else:
                    _C.check(lib.up_bn_finalize_groups(stats.data_ptr(), tiles, C, groups, L, BN_EPS, MOM, rm.data_ptr(), rv.data_ptr(),
                                                       gd.data_ptr(), bd.data_ptr(), coef.data_ptr(), st), "bn_finalize_groups")
            else:
                _tune(bn_fold=int(form == "fold"))
                _C.check(lib.up_bn_stats_groups_t(yd.data_ptr(), ld, L, C, groups, _dt(dtype), stats.data_ptr(), BN_EPS, MOM,
                                                  rm.data_ptr(), rv.data_ptr(), gd.data_ptr(), bd.data_ptr(), coef.data_ptr(), st),
                         "bn_stats_groups")
            worst.merge(_check_coef(coef, rm, rv, refs, bounds, f"{what} {form}"))
            counts = stats.cpu()[..., 0]
            want = torch.tensor([min(256, L - 256 * t) for t in range(tiles)], dtype=torch.float32).view(1, tiles, 1)
            assert torch.equal(counts, want.expand_as(counts)), f"{what} {form}: partial counts"
    finally:
        _tune(**TUNE_DEFAULTS)
    print(f"bn {what}: worst got/bound {worst}")
    return worst


def exact_stats_case(dev, groups, L, C, dtype):
    """up_bn_exact_stats_t on multiples of 2^-10: the mean is float32(mean64) bit for bit, M2 within one rounding; then
    up_bn_finalize_groups on its single partial row."""
    gen = _gen(7)
    std = 10.0 ** (-2 + 4 * torch.rand(C, generator=gen, dtype=torch.float64))
    mean = std * torch.randn(C, generator=gen, dtype=torch.float64)
    std[0], mean[0] = 1.0, 4000.0
    y = mean + std * torch.randn(groups * L, C, generator=gen, dtype=torch.float64)
    y += torch.arange(groups).repeat_interleave(L).view(-1, 1) * 0.75 * std
    y[:, 1:] = y[:, 1:].clamp(-1023, 1023)
    if C > 1:
        y[:, 1] = 2.5
    y = _rt((torch.round(y * 1024) / 1024).float(), dtype)
    assert float(y.abs().max()) < 2.0 ** 13
    ld = C + 3
    yd = _padded(y, ld, dtype, dev, math.nan)
    stats = torch.full((groups, 1, C, 3), SENT).to(dev)
    lib, st = _C.lib(), ops._stream(yd)
    _C.check(lib.up_bn_exact_stats_t(yd.data_ptr(), ld, L, C, groups, _dt(dtype), stats.data_ptr(), st), "bn_exact_stats")
    s = stats64(y, groups, L)
    got = stats.cpu()[:, 0]
    assert bool((got[..., 0] == L).all())
    assert torch.equal(got[..., 1], s["mean"].float()), "the mean is not the correctly rounded one"
    w = Worst(M2=_ratio(got[..., 2], s["M2"], U * s["M2"] + 2.0 ** -40 * s["M2"]))
    _check(w, f"exact stats g{groups} L{L} C{C}")
    print(f"bn exact stats g{groups} L{L} C{C}: worst got/bound {w}")
    if C % 4 == 0:      # its partial row through the merge: one more rounding of each
        gamma, beta = 0.5 + torch.rand(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
        rm0, rv0, rm, rv = _running0(C, dev)
        coef = torch.full((groups, 4, C), SENT).to(dev)
        gd, bd = gamma.to(dev), beta.to(dev)
        _C.check(lib.up_bn_finalize_groups(stats.data_ptr(), 1, C, groups, L, BN_EPS, MOM, rm.data_ptr(), rv.data_ptr(),
                                           gd.data_ptr(), bd.data_ptr(), coef.data_ptr(), st), "bn_finalize_groups")
        refs, bounds = propagate(s["mean"], s["var"], L, U * s["mean"].abs(), 2 * U * s["var"], gamma, beta, rm0, rv0)
        w.merge(_check_coef(coef, rm, rv, refs, bounds, f"exact stats + finalize g{groups} L{L} C{C}", "_merge"))
    return w


def finalize_synthetic_case(dev, tiles, C, groups=1):
    """up_bn_finalize / up_bn_finalize_groups on partial rows (count, mean, M2) built on the host in float64 from an arbitrary
    partition of the rows (unequal counts, one tile with count 0), rounded to fp32: against the float64 merge of the same fp32
    partials.  groups <= BN_MAXG: beyond that the chunks are merged in fp32 (bn_finalize_kernel), which the tensor cases cover."""
    assert groups <= BN_MAXG
    gen = _gen(11 + tiles + C)
    counts = torch.randint(1, 9, (groups, tiles), generator=gen)
    if tiles > 1:
        counts[:, tiles // 2] = 0
    L = int(counts[0].sum())
    for g in range(1, groups):          # equal rows per group, another partition: group 0's counts in another order
        counts[g] = counts[0][torch.randperm(tiles, generator=gen)]
    y, gamma, beta = make_input(groups, L, C, F32, seed=13 + tiles)
    part = torch.zeros(groups, tiles, C, 3, dtype=torch.float64)
    for g in range(groups):
        r = g * L
        for t in range(tiles):
            n = int(counts[g, t])
            if n:
                blk = y[r:r + n].double()
                m = blk.mean(0)
                part[g, t, :, 0], part[g, t, :, 1], part[g, t, :, 2] = n, m, ((blk - m) ** 2).sum(0)
            r += n
    part32 = part.float()
    p = part32.double()
    n_, m_, q_ = p[..., 0], p[..., 1], p[..., 2]
    mean = (n_ * m_).sum(1) / L
    m2 = (q_ + n_ * (m_ - mean[:, None]) ** 2).sum(1)
    rm0, rv0, rm, rv = _running0(C, dev)
    refs, bounds = propagate(mean, m2 / L, L, U * mean.abs(), torch.zeros_like(mean), gamma, beta, rm0, rv0)
    bounds["invstd"] = 4 * U * refs["invstd"]
    pd, gd, bd = part32.to(dev), gamma.to(dev), beta.to(dev)
    coef = torch.full((groups, 4, C), SENT).to(dev)
    lib, st = _C.lib(), ops._stream(pd)
    if groups == 1:
        _C.check(lib.up_bn_finalize(pd.data_ptr(), tiles, C, BN_EPS, MOM, rm.data_ptr(), rv.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                    coef[0, 0].data_ptr(), coef[0, 1].data_ptr(), coef[0, 2].data_ptr(), coef[0, 3].data_ptr(), st),
                 "bn_finalize")
    else:
        _C.check(lib.up_bn_finalize_groups(pd.data_ptr(), tiles, C, groups, L, BN_EPS, MOM, rm.data_ptr(), rv.data_ptr(), gd.data_ptr(),
                                           bd.data_ptr(), coef.data_ptr(), st), "bn_finalize_groups")
    w = _check_coef(coef, rm, rv, refs, bounds, f"finalize synthetic tiles={tiles} C={C} groups={groups}", "_merge")
    print(f"bn finalize synthetic tiles={tiles} C={C} groups={groups}: worst got/bound {w}")
    return w


def eval_coeffs_case(dev, C):
    gen = _gen(17)
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    rm = torch.randn(C, generator=gen) * 10.0 ** (-2 + 4 * torch.rand(C, generator=gen))
    rv = 10.0 ** (-6 + 12 * torch.rand(C, generator=gen))
    rv[0] = 0.0
    out = torch.full((2, C), SENT).to(dev)
    gd, bd, md, vd = (t.to(dev) for t in (gamma, beta, rm, rv))
    _C.check(_C.lib().up_bn_eval_coeffs(gd.data_ptr(), bd.data_ptr(), md.data_ptr(), vd.data_ptr(), BN_EPS, C, out[0].data_ptr(),
                                        out[1].data_ptr(), ops._stream(gd)), "bn_eval_coeffs")
    eps32 = float(torch.tensor(BN_EPS, dtype=torch.float32))
    sc = gamma.double() / torch.sqrt(rv.double() + eps32)
    sh = beta.double() - rm.double() * sc
    # scale: rv + eps, sqrt, 1 / x, * gamma = 4 roundings; shift: the scale's error times |rm|, the product and the difference
    w = Worst(scale=_ratio(out[0].cpu(), sc, 4 * U * sc.abs()),
              shift=_ratio(out[1].cpu(), sh, 5 * U * (rm.double() * sc).abs() + U * sh.abs()))
    _check(w, f"eval coeffs C={C}")
    return w


def relu_bwd_case(dev, n):
    gen = _gen(19)
    z, dz = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    z[::3], z[1::7], z[2::11] = 0.0, -0.0, 1e-30
    dx = torch.full((n + 4,), SENT).to(dev)
    zd, dzd = z.to(dev), dz.to(dev)
    _C.check(_C.lib().up_relu_bwd(dzd.data_ptr(), zd.data_ptr(), dx.data_ptr(), n, ops._stream(zd)), "relu_bwd")
    assert torch.equal(dx.cpu()[:n], torch.where(z > 0, dz, torch.zeros(()))) and bool((dx.cpu()[n:] == SENT).all())


# ---- backward -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bwd_reference(groups, L, C, dtype, mode, seed=0):
    """Inputs and float64 results of one backward case.  mode: "none" (no ReLU), "bits" (mask drawn on the host), "z" (ZPATH: mask
    = z > 0 of a z with planted +0.0 / -0.0 / tiny values).  The last channel's mask is all zero.  Shared, never modified."""
    rows = groups * L
    y, gamma, beta = make_input(groups, L, C, dtype, seed=21 + seed)
    coef = coefficients(y, gamma, beta, groups, L)
    gen = _gen(23 + seed)
    dz = _rt(torch.randn(rows, C, generator=gen) * 10.0 ** (-2 + 4 * torch.rand(C, generator=gen)), dtype)
    z = None
    if mode == "none":
        mask = torch.ones(rows, C, dtype=torch.bool)
    elif mode == "bits":
        mask = torch.rand(rows, C, generator=gen) > 0.45
        mask[:, C - 1] = False
    else:
        z = torch.randn(rows, C, generator=gen)
        flat = z.view(-1)
        flat[0::5], flat[1::7], flat[2::9], flat[3::11] = 0.0, -0.0, 1e-30, -1e-30
        z[:, C - 1] = -z[:, C - 1].abs()
        z = _rt(z, dtype)
        mask = z > 0
    g = torch.where(mask, dz, torch.zeros(())).double().view(groups, L, C)
    y64 = y.double().view(groups, L, C)
    mean, invstd = coef[:, 0, None].double(), coef[:, 1, None].double()
    k = gamma.double().view(1, 1, C) * invstd
    cen = y64 - mean
    xhat = cen * invstd
    dbeta = g.sum(1, keepdim=True)
    dgamma = invstd * (g * cen).sum(1, keepdim=True)
    b_beta = 2 * (L + 1) * U * g.abs().sum(1, keepdim=True)
    b_gamma = 2 * (L + 3) * U * invstd.abs() * (g.abs() * cen.abs()).sum(1, keepdim=True)
    return dict(y=y, gamma=gamma, coef=coef, dz=dz, z=z, mask=mask, g=g, k=k, xhat=xhat, dbeta=dbeta, dgamma=dgamma, b_beta=b_beta,
                b_gamma=b_gamma)


def dy_reference(ref, L, dtype, use_batch, dgamma=None, dbeta=None):
    """(dy64, bound); dgamma / dbeta given (fp32 inputs of a finalized entry): they replace the float64 sums and their bounds"""
    g, k, xhat = ref["g"], ref["k"], ref["xhat"]
    bf = BF_TERM if dtype == BF else 0.0
    if not use_batch:
        dy = k * g
        return dy, 2 * U * dy.abs() + bf * dy.abs()
    given = dgamma is not None
    dg = dgamma.double() if given else ref["dgamma"]
    db = dbeta.double() if given else ref["dbeta"]
    dy = k * (g - db / L - xhat * dg / L)
    bound = 6 * U * k.abs() * (g.abs() + db.abs() / L + xhat.abs() * dg.abs() / L) + bf * dy.abs()
    if not given:
        bound = bound + k.abs() * (ref["b_beta"] + xhat.abs() * ref["b_gamma"]) / L
    return dy, bound


def _check_bwd(ref, groups, L, C, dtype, use_batch, dy, dres, dgamma, dbeta, what, given=None, sums=True):
    w = Worst()
    dy64, bound = dy_reference(ref, L, dtype, use_batch, *(given or ()))
    w.add(("dy" if use_batch else "dy_eval") + _sfx(dtype), _ratio(_live(dy, C).view(groups, L, C), dy64, bound))
    assert _pads_kept(dy, C), f"{what}: pad lanes of dy written"
    if dres is not None:
        assert torch.equal(_live(dres, C).double().view(groups, L, C), ref["g"]), f"{what}: dres != where(mask, dz, 0)"
        assert _pads_kept(dres, C), f"{what}: pad lanes of dres written"
    if sums:
        summing = (groups + 1) * U if groups > 1 else 0.0
        w.add("dbeta", _ratio(dbeta.cpu(), ref["dbeta"].sum(0).view(C), (ref["b_beta"].sum(0) + summing * ref["dbeta"].abs().sum(0)).view(C)))
        w.add("dgamma", _ratio(dgamma.cpu(), ref["dgamma"].sum(0).view(C), (ref["b_gamma"].sum(0) + summing * ref["dgamma"].abs().sum(0)).view(C)))
    _check(w, what)
    return w


class _BwdCall:
    """device tensors of one backward case, every one with its own leading dimension"""

    def __init__(self, dev, ref, C, dtype, step, mode):
        self.lddz, self.ldy, self.lddy, self.lddres = _lds(C, step, 4)
        self.ldz = self.ldy
        self.dz = _padded(ref["dz"], self.lddz, dtype, dev, math.nan)
        self.y = _padded(ref["y"], self.ldy, dtype, dev, math.nan)
        self.z = _padded(ref["z"], self.ldz, dtype, dev, math.nan) if mode == "z" else None
        self.bits = pack_bits(ref["mask"]).to(dev) if mode == "bits" else None
        self.gamma, self.coef = ref["gamma"].to(dev), ref["coef"].to(dev)
        self.rows, self.dtype, self.dev, self.C = ref["dz"].shape[0], dtype, dev, C
        self.relu = int(mode != "none")

    def outputs(self, with_dres):
        mk = lambda ld: torch.full((self.rows, ld), SENT).to(self.dtype).to(self.dev)
        return mk(self.lddy), (mk(self.lddres) if with_dres else None), torch.full((2, self.C), SENT).to(self.dev)


def bwd_case(dev, shape, quick=False):
    """up_bn_bwd_t: no ReLU / mask bits / ZPATH x dres x use_batch_stats x bn_fold x bn_rows, every form against float64."""
    dtype, C, L, step = shape
    lib = _C.lib()
    worst = Worst()
    nbytes = lib.up_bn_bwd_workspace(L, C)
    assert nbytes == (L + 127) // 128 * C * 8
    ws = torch.zeros(nbytes // 4).to(dev)
    try:
        for mode in ("bits", "z", "none"):
            ref = bwd_reference(1, L, C, dtype, mode)
            call = _BwdCall(dev, ref, C, dtype, step, mode)
            st = ops._stream(call.dz)
            for bn_rows in ((1, 0) if _has_rows_geometry(C, dtype) else (1,)):
                for bn_fold in (1, 0):
                    _tune(bn_rows=bn_rows, bn_fold=bn_fold)
                    for with_dres in (True, False):
                        for ub in (1, 0):
                            if quick and (with_dres, ub) not in ((True, 1), (False, 0)):
                                continue
                            dy, dres, dgb = call.outputs(with_dres)
                            _C.check(lib.up_bn_bwd_t(call.dz.data_ptr(), call.lddz, _ptr(call.z), call.ldz, _ptr(call.bits),
                                                     call.y.data_ptr(), call.ldy, call.gamma.data_ptr(), call.coef[0, 0].data_ptr(),
                                                     call.coef[0, 1].data_ptr(), call.relu, ub, dy.data_ptr(), call.lddy, _ptr(dres),
                                                     call.lddres, dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), nbytes, L, C,
                                                     _dt(dtype), st), "bn_bwd")
                            what = f"bwd {shape_id(shape)} mask={mode} dres={with_dres} use_batch={ub} bn_rows={bn_rows} bn_fold={bn_fold}"
                            worst.merge(_check_bwd(ref, 1, L, C, dtype, ub, dy, dres, dgb[0], dgb[1], what))
                            if mode != "none":       # the all-zero mask channel
                                assert float(dgb[:, C - 1].abs().max()) == 0 and float(_live(dy, C)[:, C - 1].abs().max()) == 0, what
    finally:
        _tune(**TUNE_DEFAULTS)
    print(f"bn bwd {shape_id(shape)}: worst got/bound {worst}")
    return worst


def bwd_acc_case(dev, shape):
    """up_bn_bwd_acc_t twice (two dz) onto accumulators that start at 3.25: acc == fl(fl(a0 + d1) + d2) of the device's own sums,
    each call's dy / dgamma / dbeta inside the float64 bounds (this form keeps bn_bwd_finalize_kernel)."""
    dtype, C, L, step = shape
    lib = _C.lib()
    nbytes = lib.up_bn_bwd_workspace(L, C)
    ws = torch.zeros(nbytes // 4).to(dev)
    acc = torch.full((2, C), 3.25).to(dev)
    want = acc.cpu().clone()
    worst = Worst()
    for seed, mode in ((0, "bits"), (1, "z")):
        ref = bwd_reference(1, L, C, dtype, mode, seed)
        call = _BwdCall(dev, ref, C, dtype, step, mode)
        dy, dres, dgb = call.outputs(True)
        _C.check(lib.up_bn_bwd_acc_t(call.dz.data_ptr(), call.lddz, _ptr(call.z), call.ldz, _ptr(call.bits), call.y.data_ptr(), call.ldy,
                                     call.gamma.data_ptr(), call.coef[0, 0].data_ptr(), call.coef[0, 1].data_ptr(), 1, 1, dy.data_ptr(),
                                     call.lddy, dres.data_ptr(), call.lddres, dgb[0].data_ptr(), dgb[1].data_ptr(), acc[0].data_ptr(),
                                     acc[1].data_ptr(), ws.data_ptr(), nbytes, L, C, _dt(dtype), ops._stream(call.dz)), "bn_bwd_acc")
        worst.merge(_check_bwd(ref, 1, L, C, dtype, 1, dy, dres, dgb[0], dgb[1], f"bwd_acc {shape_id(shape)} call {seed}"))
        want = want + dgb.cpu()                     # fp32 addition on the host: one rounding, like the kernel's +=
        assert torch.equal(acc.cpu(), want), f"bwd_acc {shape_id(shape)}: accumulators after call {seed}"
    return worst


def _synthetic_partials(ref, groups, L, C, chunks, seed=0):
    """[groups][chunks][C][2] = (sum g, invstd sum g (y - mean)) over an arbitrary partition of every group's rows, float64 -> fp32"""
    cuts = torch.sort(torch.randint(0, L + 1, (chunks - 1,), generator=_gen(29 + seed + chunks)))[0].tolist()
    edges = [0] + cuts + [L]
    cen = ref["xhat"]                                # (y - mean) invstd
    out = torch.zeros(groups, chunks, C, 2, dtype=torch.float64)
    for i in range(chunks):
        a, b = edges[i], edges[i + 1]
        out[:, i, :, 0] = ref["g"][:, a:b].sum(1)
        out[:, i, :, 1] = (ref["g"][:, a:b] * cen[:, a:b]).sum(1)
    return out.float()


def bwd_prereduced_case(dev, shape, chunks):
    """up_bn_bwd_prereduced_t on synthetic partials (the merge tree alone and, with accumulators, bn_bwd_finalize_kernel), and
    up_bn_bwd_finalized_t on given fp32 sums: relu on / off x dres x use_batch_stats."""
    dtype, C, L, step = shape
    lib = _C.lib()
    worst = Worst()
    for mode in ("bits", "none"):
        ref = bwd_reference(1, L, C, dtype, mode)
        call = _BwdCall(dev, ref, C, dtype, step, mode)
        st = ops._stream(call.dz)
        part = _synthetic_partials(ref, 1, L, C, chunks)[0].contiguous().to(dev)
        given = ((ref["dgamma"].view(C) * 1.37).float(), (ref["dbeta"].view(C) * 0.61).float())
        gdev = [t.to(dev) for t in given]
        for with_dres in (True, False):
            for ub in (1, 0):
                for acc in (False, True):
                    dy, dres, dgb = call.outputs(with_dres)
                    a = torch.full((2, C), 3.25).to(dev) if acc else None
                    _C.check(lib.up_bn_bwd_prereduced_t(call.dz.data_ptr(), call.lddz, _ptr(call.bits), call.y.data_ptr(), call.ldy,
                                                        call.gamma.data_ptr(), call.coef[0, 0].data_ptr(), call.coef[0, 1].data_ptr(),
                                                        call.relu, ub, dy.data_ptr(), call.lddy, _ptr(dres), call.lddres, dgb[0].data_ptr(),
                                                        dgb[1].data_ptr(), _ptr(a[0]) if acc else None, _ptr(a[1]) if acc else None,
                                                        part.data_ptr(), chunks, L, C, _dt(dtype), st), "bn_bwd_prereduced")
                    what = f"bwd_prereduced {shape_id(shape)} chunks={chunks} mask={mode} dres={with_dres} use_batch={ub} acc={acc}"
                    worst.merge(_check_bwd(ref, 1, L, C, dtype, ub, dy, dres, dgb[0], dgb[1], what))
                    if acc:
                        assert torch.equal(a.cpu(), torch.full((2, C), 3.25) + dgb.cpu()), what
                dy, dres, _ = call.outputs(with_dres)
                _C.check(lib.up_bn_bwd_finalized_t(call.dz.data_ptr(), call.lddz, _ptr(call.bits), call.y.data_ptr(), call.ldy,
                                                   call.gamma.data_ptr(), call.coef[0, 0].data_ptr(), call.coef[0, 1].data_ptr(), call.relu,
                                                   ub, dy.data_ptr(), call.lddy, _ptr(dres), call.lddres, gdev[0].data_ptr(),
                                                   gdev[1].data_ptr(), L, C, _dt(dtype), st), "bn_bwd_finalized")
                what = f"bwd_finalized {shape_id(shape)} mask={mode} dres={with_dres} use_batch={ub}"
                w = _check_bwd(ref, 1, L, C, dtype, ub, dy, dres, None, None, what,
                               given=(given[0].view(1, 1, C), given[1].view(1, 1, C)), sums=False)
                worst.merge({k + "_finalized": v for k, v in w.items()})
    print(f"bn bwd prereduced / finalized {shape_id(shape)} chunks={chunks}: worst got/bound {worst}")
    return worst


def groups_case(dev, case):
    """Grouped BatchNorm: statistics (the groups' coefficients one by one, running statistics after `groups` updates in order),
    both apply forms, and up_bn_bwd_groups_t (+ its prereduced / finalized forms where they apply) with bn_fold 1 / 0."""
    groups, L, C, dtype = case
    step = 8 if dtype == BF else 4
    shape = (dtype, C, L, step)
    worst = Worst()
    worst.merge(stats_case(dev, shape, groups))
    worst.merge(apply_case(dev, shape, groups))
    lib = _C.lib()
    nbytes = lib.up_bn_bwd_groups_workspace(L, C, groups)
    ws = torch.zeros(nbytes // 4 + 1).to(dev)
    strided = _has_rows_geometry(C, dtype)
    try:
        for mode in ("bits", "none"):
            ref = bwd_reference(groups, L, C, dtype, mode)
            call = _BwdCall(dev, ref, C, dtype, step, mode)
            st = ops._stream(call.dz)
            for bn_fold in (1, 0):
                _tune(bn_fold=bn_fold)
                for with_dres in (True, False):
                    dy, dres, dgb = call.outputs(with_dres)
                    _C.check(lib.up_bn_bwd_groups_t(call.dz.data_ptr(), call.lddz, _ptr(call.bits), call.y.data_ptr(), call.ldy,
                                                    call.gamma.data_ptr(), call.coef.data_ptr(), call.relu, dy.data_ptr(), call.lddy,
                                                    _ptr(dres), call.lddres, dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), nbytes,
                                                    L, C, groups, _dt(dtype), st), "bn_bwd_groups")
                    what = f"bwd_groups {group_id(case)} mask={mode} dres={with_dres} bn_fold={bn_fold}"
                    worst.merge(_check_bwd(ref, groups, L, C, dtype, 1, dy, dres, dgb[0], dgb[1], what))
            if not (strided and groups <= BN_MAXG and dtype == F32):
                continue
            assert lib.up_bn_bwd_groups_prereduced_ok(L, C, groups, call.lddz) == 1
            for chunks in PREREDUCED_CHUNKS:
                part = _synthetic_partials(ref, groups, L, C, chunks).contiguous().to(dev)
                dy, dres, dgb = call.outputs(True)
                _C.check(lib.up_bn_bwd_groups_prereduced_t(call.dz.data_ptr(), call.lddz, _ptr(call.bits), call.y.data_ptr(), call.ldy,
                                                           call.gamma.data_ptr(), call.coef.data_ptr(), call.relu, dy.data_ptr(), call.lddy,
                                                           dres.data_ptr(), call.lddres, dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(),
                                                           nbytes, part.data_ptr(), chunks, L, C, groups, 0, st), "bn_bwd_groups_prereduced")
                worst.merge(_check_bwd(ref, groups, L, C, dtype, 1, dy, dres, dgb[0], dgb[1],
                                       f"bwd_groups_prereduced {group_id(case)} mask={mode} chunks={chunks}"))
            gsum = torch.stack([ref["dgamma"].view(groups, C) * 1.37, ref["dbeta"].view(groups, C) * 0.61], 1).float().contiguous()
            gd = gsum.to(dev)
            dy, dres, _ = call.outputs(True)
            _C.check(lib.up_bn_bwd_groups_finalized_t(call.dz.data_ptr(), call.lddz, _ptr(call.bits), call.y.data_ptr(), call.ldy,
                                                      call.gamma.data_ptr(), call.coef.data_ptr(), call.relu, dy.data_ptr(), call.lddy,
                                                      dres.data_ptr(), call.lddres, gd.data_ptr(), L, C, groups, 0, st),
                     "bn_bwd_groups_finalized")
            w = _check_bwd(ref, groups, L, C, dtype, 1, dy, dres, None, None, f"bwd_groups_finalized {group_id(case)} mask={mode}",
                           given=(gsum[:, 0].view(groups, 1, C), gsum[:, 1].view(groups, 1, C)), sums=False)
            worst.merge({k + "_finalized": v for k, v in w.items()})
    finally:
        _tune(**TUNE_DEFAULTS)
    print(f"bn groups {group_id(case)}: worst got/bound {worst}")
    return worst
