"""The weight-gradient entries on their own, against float64, per element (shared by test_wgrad_emu.py and test_wgrad_gpu.py):
up_conv2d_bwd_weight_acc in its three math modes (and the three older entries, which must give the same bits), the pixel split
of plan_wgrad, the compensated slab merge wgrad_reduce_kernel with and without `accumulate`, the live rectangles, the bias
gradient (colsum4_kernel / colsum_kernel / colsum_finish_kernel), the documented fallback for operands that are not 16-byte
aligned, the reported workspace size and the refusals.  The tests call the C entries directly.

Reference and bounds (derived, not measured).  F.conv2d autograd in float64 on the CPU; u = 2^-24, L = N P Q:

    |dw - dw64| <= 2 (L + 1) u A_dw        |db - db64| <= 2 (L + 1) u A_db

A_dw is the same gradient of |x| and |dy|, A_db = sum |dy| (geometry_cases.py: an fp32 dot product summed in any order, times
2 for non-nearest rounding inside the MFMA; the split-K merge and the 16 x 16 + 64-lane trees of the bias gradient are such
orders).  Where A == 0 (a tap that never sees the image) the element must be exactly 0, or exactly the old value under
`accumulate`.
  bf16 storage:   x and dy are rounded to bf16 here first; products of bf16 values are exact in fp32: the same bound.
  bf16 operands:  wgrad_bf16_kernel rounds while it stages, with pack_bf16x2 = two (__bf16) casts of fp32 values: round to
                  nearest even, the rounding of torch's .to(bfloat16).  The launch gets the UNROUNDED fp32 tensors, the float64
                  reference of dw is computed from the operands rounded here, the bound stays the fp32 one (no 2^-8 term: it
                  would hide a dropped pixel).  The bias gradient of that mode sums the fp32 dy itself (colsum reads the tensor),
                  so db64 comes from the unrounded dy.
  accumulate = 1: (a) |got - (old + ref64)| <= bound + u |old + ref64|, (b) got == float32(old) + float32(r0) bit for bit, r0
                  the same launch with accumulate = 0.  old has both signs and the spread of the result, so a sum written over
                  old, or added twice, is outside (a).  dbias likewise.
  accumulate = 0: dw and dbias are prefilled with NaN; every launch runs twice and must give equal bits.
Every launch of this module gets the bytes up_conv2d_bwd_weight_workspace reports, prefilled with NaN (a slab element the merge
reads and no workgroup wrote shows in dw), with sentinel bytes (on the emulator: at most 12 of them, then an inaccessible page)
directly behind.  dw and dbias lie in the middle of larger buffers of sentinels; x and dy have pixel strides larger than their
channel counts with NaN in the lanes past Cp resp. rup4(K).  colsum4_kernel reads whole quads inside ldy, so the lanes
K .. rup4(K) - 1 of dy hold zeros, as the library's own tensors do; a NaN from the lanes behind them in a channel is a finding.

Which kernel ran.  Every launch must name the profile variant of its case (family and tile pair) in up_conv_counter's
"wgrad_variant"; on the GPU it is also bracketed by up_profile_begin / up_profile_end and must show exactly one launch, of that
variant (the emulator has no events: its profile stays empty, which bench.py's dry run relies on).  The counters
"wgrad_glds32", "wgrad_glds32_st1", "wgrad_st1", "wgrad_rect" and "wgrad_splits" must agree with plan_wgrad as restated in
`plan` below.
  FINDING: the one-stage forms of the 64x64 tile (wgrad_glds32_kernel<64,64,1,4>, wgrad_kernel<64,64,64>) cannot be reached
  through plan_wgrad.  bm = bn = 64 means K <= 64 and R S Cp <= 64, i.e. ONE tile; the one-stage rule wants more than 2 cu
  workgroups, and with one tile the split search stops at the latest at 2 cu splits (utilisation 1.0): one_stage_64x64_case
  sweeps the restated plan over every chip size and asserts it, and launches the closest shape.  The other three tile pairs
  run in both one-stage families.

Unaligned operands (unaligned_case).  glds32_form, glds_form and `quads` test the pointers and fall back to wgrad_kernel /
wgrad_bf16_kernel and the 1024-row colsum_kernel.  Those kernels still issue 16-byte loads (float4 / uint4) from addresses that
are then only 4-byte (fp32) or 8-byte (bf16) aligned: global loads of gfx950 need dword alignment only, and the emulator's
float4 has the alignment of a float, so the dispatch guarantees all the kernels assume; the cases pass on both.

Merge stays compensated: kahan_case (exact integers; the uncompensated four-chain sum restated in numpy gives 6, not 7, for
two of the three orders; in the order "-2^24 first, 2^24 in the tail split" the plain sum is right as well, because
-2^24 + 1 is representable: that order is kept for the kernel, which must return 7 in all three).
"""
import ctypes as C
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import bn_cases as bx
import glds32_cases as g32
from unipose_amd import _C, ops

BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
SENT = 7.0
TAIL = 0x5A                  # bytes behind the reported workspace
PAD = 8                      # sentinel floats on both sides of dw / dbias
M_F32, M_BF16, M_BF16S = ops.MATH_F32, ops.MATH_BF16, ops.MATH_BF16S
DEFAULTS = dict(g32.DEFAULTS, glds=1, wgrad_rect=1)
COUNTERS = ("wgrad_glds32", "wgrad_glds32_st1", "wgrad_st1", "wgrad_rect")
Worst, _ratio, _check = bx.Worst, bx._ratio, bx._check
REAL_CUS = 256               # compute units of the MI355X (and of the emulator's "chip")

FAMILIES = {
    "glds32": dict(math=M_F32, tune=dict(glds32_wgrad=1), st1=False, variant="wgrad_glds32_kernel<%d,%d>"),
    "glds32_st1": dict(math=M_F32, tune=dict(glds32_wgrad=1), st1=True, variant="wgrad_glds32_kernel<%d,%d>"),
    "reg": dict(math=M_F32, tune=dict(glds32_wgrad=0), st1=False, variant="wgrad_kernel<%d,%d>"),
    "reg_st1": dict(math=M_F32, tune=dict(glds32_wgrad=0), st1=True, variant="wgrad_kernel<%d,%d>"),
    "bf16op": dict(math=M_BF16, tune=dict(), st1=None, variant="wgrad_bf16_kernel<%d,%d>"),
    "bf16s_glds": dict(math=M_BF16S, tune=dict(glds=1), st1=None, variant="wgrad_glds_kernel<%d,%d> (bf16)"),
    "bf16s_reg": dict(math=M_BF16S, tune=dict(glds=0), st1=None, variant="wgrad_bf16_kernel<%d,%d>"),
}
FP = ("glds32", "reg", "bf16op")
BS = ("bf16s_glds", "bf16s_reg")
ALL5 = FP + BS
MODE = {M_F32: "f32", M_BF16: "bf16op", M_BF16S: "bf16s"}


def _gen(seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return gen


def _tune(**kw):
    for k, v in kw.items():
        _C.check(_C.lib().up_conv_tune(k.encode(), int(v)), k)


def _counters():
    return {m: int(_C.lib().up_conv_counter(m.encode())) for m in COUNTERS}


def _rb(t):
    return t.to(BF).float()


def _pq(geo):
    n, h, w, r, s, stride, pad, dil = geo
    return (h + 2 * pad - dil * (r - 1) - 1) // stride + 1, (w + 2 * pad - dil * (s - 1) - 1) // stride + 1


def _cdiv(a, b):
    return (a + b - 1) // b


def plan(geo, cp, k, cus=0, slice_=32):
    """plan_wgrad (conv_igemm.hip) restated: tile pair, tiles, pixel splits, rows per split, workgroups"""
    n, h, w, r, s, stride, pad, dil = geo
    p, q = _pq(geo)
    cus = cus or REAL_CUS
    ncols = r * s * cp
    bm, bn = (64 if k <= 64 else 128), (64 if ncols <= 64 else 128)
    ntm, ntn = _cdiv(k, bm), _cdiv(ncols, bn)
    m = n * p * q
    tiles = ntm * ntn
    splits, best, sp = 1, 0.0, 1
    while sp <= max(1, _cdiv(m, 256)) and tiles * sp <= 4 * cus:
        wgs = tiles * sp
        util = wgs / (cus * _cdiv(wgs, cus)) * (1.0 if wgs > cus else 0.8)
        if util > best + 1e-9:
            best, splits = util, sp
        if util >= 0.95:
            break
        sp += 1
    rps = _cdiv(_cdiv(m, splits), slice_) * slice_
    splits = _cdiv(m, rps)
    return dict(bm=bm, bn=bn, ntm=ntm, ntn=ntn, tiles=tiles, splits=splits, rps=rps, nwg=tiles * splits, M=m, ncols=ncols)


def rect_table(geo, cp, pl):
    """wgrad_rect_table restated: per column tile (rows, cols, rows per split, pixels) of the bounding rectangle of its taps"""
    n, h, w, r, s, stride, pad, dil = geo
    p, q = _pq(geo)

    def live(size_in, size_out, off):
        a = pad - off
        lo = 0 if a <= 0 else _cdiv(a, stride)
        b = size_in - 1 + pad - off
        hi = -1 if b < 0 else b // stride
        return lo, min(hi, size_out - 1)
    out = []
    for nt in range(pl["ntn"]):
        c_lo, c_hi = nt * pl["bn"], min(pl["ncols"], (nt + 1) * pl["bn"]) - 1
        p_lo, p_hi, q_lo, q_hi = p, -1, q, -1
        for t in range(c_lo // cp, c_hi // cp + 1):
            lo, hi = live(h, p, (t // s) * dil)
            if lo <= hi:
                p_lo, p_hi = min(p_lo, lo), max(p_hi, hi)
            lo, hi = live(w, q, (t % s) * dil)
            if lo <= hi:
                q_lo, q_hi = min(q_lo, lo), max(q_hi, hi)
        hr, wr = max(p_hi - p_lo + 1, 0), max(q_hi - q_lo + 1, 0)
        rows, cols = (hr, wr) if hr and wr else (0, 0)
        mt = n * rows * cols
        rps = max(32, _cdiv(_cdiv(mt, pl["splits"]), 32) * 32)
        out.append(dict(rows=rows, cols=cols, rps=rps, mt=mt))
    return out


# ---- reference ---------------------------------------------------------------------------------------------------
def _wgrad64(x, dy, geo, k):
    n, h, w, r, s, stride, pad, dil = geo
    wz = torch.zeros(k, x.shape[1], r, s, dtype=torch.float64, requires_grad=True)
    bz = torch.zeros(k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wz, bz, stride=stride, padding=pad, dilation=dil).backward(dy)
    return wz.grad, bz.grad


def _reference_of(x, dy, geo, k, mode):
    if mode == "bf16s":
        x, dy = _rb(x), _rb(dy)
    xo, dyo = (_rb(x), _rb(dy)) if mode == "bf16op" else (x, dy)       # what the MFMA multiplies
    dw, db = _wgrad64(xo.double(), dyo.double(), geo, k)
    a_dw, a_db = _wgrad64(xo.double().abs(), dyo.double().abs(), geo, k)
    if mode == "bf16op":                                               # the bias gradient sums the fp32 tensor itself
        db, a_db = dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
    length = dy.shape[0] * dy.shape[2] * dy.shape[3]
    g = _gen(991)
    scale = max(float(dw.abs().mean()), 1e-3)
    old_dw = (torch.randn(dw.shape, generator=g) * scale).float()
    old_db = (torch.randn(db.shape, generator=g) * max(float(db.abs().mean()), 1e-3)).float()
    assert bool((old_dw < 0).any()) or old_dw.numel() < 4
    return dict(x=x, dy=dy, dw=dw, db=db, A_dw=a_dw, A_db=a_db, L=length, old_dw=old_dw, old_db=old_db)


@functools.lru_cache(maxsize=None)
def reference(geo, c, k, mode, seed=0):
    """Inputs (fp32 values; rounded to bf16 first for bf16 storage), float64 gradients and magnitudes of one case; computed once,
    shared, never modified."""
    n, h, w, r, s, stride, pad, dil = geo
    p, q = _pq(geo)
    x = torch.randn(n, c, h, w, generator=_gen(seed + 10))
    dy = torch.randn(n, k, p, q, generator=_gen(seed + 11))
    return _reference_of(x, dy, geo, k, mode)


# ---- one launch ---------------------------------------------------------------------------------------------------
class Result:
    pass


class Call:
    """the tensors of one case.  guard: tests/emu/guard_alloc (emulator): x, dy and the workspace end in front of an
    inaccessible page."""

    def __init__(self, dev, geo, c, k, mode, ref, *, guard=None, misalign=False):
        n, h, w, r, s, stride, pad, dil = geo
        bf = mode == "bf16s"
        self.dev, self.geo, self.c, self.k, self.mode, self.ref, self.guard = dev, geo, c, k, mode, ref, guard
        self.dtype = BF if bf else F32
        q = 8 if bf else 4
        self.cp = ops.rup32(c) if bf else ops.rup4(c)
        self.kp = ops.rup32(k) if bf else ops.rup4(k)
        self.ldx, self.ldy = self.cp + q, self.kp + q
        p, qq = _pq(geo)
        self.x = self._operand(ref["x"], self.ldx, c, self.cp, misalign)
        self.dy = self._operand(ref["dy"], self.ldy, k, ops.rup4(k), misalign)
        d = _C.ConvDesc()
        d.N, d.H, d.W, d.C, d.Cp, d.ldx = n, h, w, c, self.cp, self.ldx
        d.K, d.R, d.S, d.stride, d.pad, d.dil = k, r, s, stride, pad, dil
        d.P, d.Q, d.Kp, d.ldy = p, qq, self.kp, self.ldy
        self.d = d
        self.nw = k * c * r * s
        self.dwbuf = torch.empty(self.nw + 2 * PAD, dtype=F32, device=dev)
        self.dbbuf = torch.empty(k + 2 * PAD, dtype=F32, device=dev)

    def _flat(self, numel, dtype):
        if self.guard is not None:
            return self.guard.guarded((numel,), dtype)
        return torch.empty(numel, dtype=dtype, device=self.dev)

    def _operand(self, t, ld, live, zero_to, misalign):
        """NCHW values -> (flat buffer, pointer) of an NHWC tensor of pixel stride ld: lanes live .. zero_to - 1 hold zeros, the
        lanes behind them NaN; misaligned: the tensor starts one float / four bf16 elements into a 16-byte aligned buffer"""
        n, ch, h, w = t.shape
        buf = torch.full((n, h, w, ld), math.nan)
        buf[..., :zero_to] = 0.0
        buf[..., :live] = t.permute(0, 2, 3, 1)
        item = 2 if self.dtype == BF else 4
        off = (16 // item // 4 * (1 if item == 4 else 2)) if misalign else 0       # one float / four bf16 elements
        flat = self._flat(buf.numel() + (16 // item if misalign else 0), self.dtype)
        flat[off:off + buf.numel()] = buf.to(self.dtype).reshape(-1).to(flat.device)
        ptr = flat.data_ptr() + off * item
        assert (ptr % 16 != 0) == bool(misalign)
        return flat, ptr

    def workspace(self):
        return int(_C.lib().up_conv2d_bwd_weight_workspace(C.byref(self.d)))

    def run(self, math_, *, accumulate=0, bias=True, entry="acc", old=None, ws_bytes=None, null=(), d=None):
        """one call of an entry; returns the code, dw / db (CPU), the moved counters, the launches per profile variant, the
        workspace as it was left, and whether everything around the outputs kept its sentinels"""
        lib = _C.lib()
        d = d or self.d
        need = self.workspace()
        assert need % 4 == 0
        tail = (-need) % 16 if self.guard is not None else 64
        ws = self._flat(need + tail, torch.uint8) if self.guard is not None else torch.empty(need + tail, dtype=torch.uint8, device=self.dev)
        assert ws.data_ptr() % 16 == 0
        ws[:need].view(F32).fill_(math.nan)
        ws[need:].fill_(TAIL)
        ws0 = ws.cpu().clone()
        self.dwbuf.fill_(SENT)
        self.dbbuf.fill_(SENT)
        self.dwbuf[PAD:PAD + self.nw] = math.nan if old is None else old[0].reshape(-1).to(self.dev)
        self.dbbuf[PAD:PAD + self.k] = math.nan if old is None else old[1].to(self.dev)
        dw0, db0 = self.dwbuf.cpu().clone(), self.dbbuf.cpu().clone()
        ptr = dict(x=self.x[1], dy=self.dy[1], dw=self.dwbuf.data_ptr() + 4 * PAD, db=self.dbbuf.data_ptr() + 4 * PAD if bias else None,
                   ws=ws.data_ptr())
        for m in null:
            ptr[m] = None
        nbytes = need if ws_bytes is None else ws_bytes
        st = ops._stream(self.dwbuf)
        nv = lib.up_profile_variants()
        arr = (C.c_double * (nv * 3))()
        c0 = _counters()
        lib.up_profile_begin()
        if entry == "acc":
            e = lib.up_conv2d_bwd_weight_acc(C.byref(d), ptr["x"], ptr["dy"], ptr["dw"], ptr["db"], ptr["ws"], nbytes, math_, accumulate, st)
        else:
            fn = {M_F32: lib.up_conv2d_bwd_weight, M_BF16: lib.up_conv2d_bwd_weight_bf16, M_BF16S: lib.up_conv2d_bwd_weight_bf16s}[math_]
            e = fn(C.byref(d), ptr["x"], ptr["dy"], ptr["dw"], ptr["db"], ptr["ws"], nbytes, st)
        msg = lib.up_last_error().decode(errors="replace") if e else ""
        _C.check(lib.up_profile_end(arr, nv), "profile_end")
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        c1 = _counters()
        res = Result()
        res.code, res.msg, res.need = e, msg, need
        res.moved = {m: c1[m] - c0[m] for m in COUNTERS}
        res.splits = int(lib.up_conv_counter(b"wgrad_splits"))
        res.variants = {lib.up_profile_variant_name(i).decode(): int(arr[3 * i]) for i in range(nv) if arr[3 * i]}
        res.profiled = self.dev.type == "cuda"          # (the emulator has no events: its profile is empty)
        res.variant = lib.up_profile_variant_name(int(lib.up_conv_counter(b"wgrad_variant"))).decode()
        dwc, dbc, wsc = self.dwbuf.cpu(), self.dbbuf.cpu(), ws.cpu()
        res.dw = dwc[PAD:PAD + self.nw].view(self.k, self.c, self.geo[3], self.geo[4]).clone()
        res.db = dbc[PAD:PAD + self.k].clone()
        res.ws = wsc[:need].view(F32).clone()
        res.around_ok = bool((dwc[:PAD] == SENT).all()) and bool((dwc[PAD + self.nw:] == SENT).all()) and \
            bool((dbc[:PAD] == SENT).all()) and bool((dbc[PAD + self.k:] == SENT).all()) and bool((wsc[need:] == TAIL).all())
        res.untouched = torch.equal(dwc.view(torch.int32), dw0.view(torch.int32)) and torch.equal(dbc.view(torch.int32), db0.view(torch.int32)) \
            and torch.equal(wsc, ws0)
        res.db_untouched = torch.equal(dbc.view(torch.int32), db0.view(torch.int32))
        return res

    def partial_rows(self, res, pl):
        """the bias gradient's partial rows as the launch left them: (rows the workspace has room for, K)"""
        off = _cdiv(pl["splits"] * self.k * pl["ncols"] * 4, 64) * 64 // 4
        rows = (res.ws.numel() - off) // self.k
        return res.ws[off:off + rows * self.k].view(rows, self.k)


def _ok(res, what):
    assert res.code == 0, f"{what}: returned {res.code} ({res.msg})"
    assert res.around_ok, f"{what}: wrote outside dw / dbias / the reported workspace"


def check_form(res, fam, pl, what, *, rect=None):
    """the launch ran once, on the variant of its family and tile pair, with the split count of the restated plan"""
    f = FAMILIES[fam]
    want = f["variant"] % (pl["bm"], pl["bn"])
    assert res.variant == want, f"{what}: ran on {res.variant}, the case was written for {want}"
    assert not res.profiled or res.variants == {want: 1}, f"{what}: profile shows {res.variants}, the case was written for one launch of {want}"
    assert res.splits == pl["splits"], f"{what}: {res.splits} splits, the restated plan has {pl['splits']}"
    mv = res.moved
    glds32 = fam.startswith("glds32")
    assert mv["wgrad_glds32"] == int(glds32), f"{what}: {mv}"
    assert mv["wgrad_glds32_st1"] == int(fam == "glds32_st1"), f"{what}: {mv} (one-stage direct-to-LDS form)"
    assert mv["wgrad_st1"] == int(fam == "reg_st1"), f"{what}: {mv} (one-stage register-staged form)"
    if rect is not None:
        assert mv["wgrad_rect"] == int(rect), f"{what}: wgrad_rect moved by {mv['wgrad_rect']}, expected {int(rect)}"


def compare(res, ref, what, *, old=None, bias=True):
    """per element against float64 (module docstring); returns the worst got / bound ratios"""
    w = Worst()
    assert not bool(torch.isnan(res.dw).any()), f"{what}: NaN in dw ({int(torch.isnan(res.dw).sum())} elements)"
    for name, got, r64, a, o in (("dw", res.dw, ref["dw"], ref["A_dw"], None if old is None else old[0]),
                                 ("db", res.db, ref["db"], ref["A_db"], None if old is None else old[1])):
        if name == "db" and not bias:
            continue
        assert not bool(torch.isnan(got).any()), f"{what}: NaN in {name}"
        bound = 2.0 * (ref["L"] + 1) * U * a
        if o is None:
            w.add(name, _ratio(got, r64, bound))
        else:
            tot = o.double() + r64
            w.add(name + "_acc", _ratio(got, tot, bound + U * tot.abs()))
            dead = a == 0
            assert torch.equal(got[dead], o[dead]), f"{what}: {name} changed where no tap sees the image"
    _check(w, what)
    return w


def full_case(call, fam, what, *, cus=0, rect=None, bias=True, accumulate=True, extra_tune=None):
    """accumulate = 0 on NaN (twice: equal bits), then accumulate = 1 on `old`: form, bounds (a) and bit rule (b)"""
    f, ref = FAMILIES[fam], call.ref
    pl = plan(call.geo, call.cp, call.k, cus, 64 if f["math"] == M_BF16S else 32)
    old = (ref["old_dw"], ref["old_db"])
    try:
        _tune(**dict(dict(f["tune"], cu_count=cus), **(extra_tune or {})))
        if f["st1"] is not None:
            assert (pl["nwg"] > 2 * (cus or REAL_CUS)) == f["st1"], f"{what}: {pl} on {cus} CUs is not the stage form of {fam}"
        r0 = call.run(f["math"], bias=bias)
        _ok(r0, what)
        check_form(r0, fam, pl, what, rect=rect)
        w = compare(r0, ref, what, bias=bias)
        r1 = call.run(f["math"], bias=bias)
        _ok(r1, what + " (second run)")
        assert torch.equal(r1.dw, r0.dw) and (not bias or torch.equal(r1.db, r0.db)), f"{what}: two runs differ"
        if accumulate:
            r2 = call.run(f["math"], accumulate=1, bias=bias, old=old)
            _ok(r2, what + " accumulate")
            check_form(r2, fam, pl, what + " accumulate", rect=rect)
            w.merge(compare(r2, ref, what + " accumulate", old=old, bias=bias))
            assert torch.equal(r2.dw, old[0] + r0.dw), f"{what}: accumulate is not one fp32 add of the accumulate = 0 result"
            if bias:
                assert torch.equal(r2.db, old[1] + r0.db), f"{what}: accumulated dbias is not one fp32 add"
            else:
                assert r2.db_untouched
        if not bias:
            assert r0.db_untouched, f"{what}: dbias = NULL, yet the buffer changed"
            assert bool(torch.isnan(call.partial_rows(r0, pl)).all()), f"{what}: dbias = NULL, yet partial rows were written"
    finally:
        _tune(**DEFAULTS)
    return w, r0, pl


def _mode(fam):
    return MODE[FAMILIES[fam]["math"]]


def _report(group, name, w):
    print(f"wgrad [{group}] {name}: worst got/bound {w}")
    return w


# ---- 1. tiles ---------------------------------------------------------------------------------------------------------
def _t(name, r, pad, c, k, fams, cus=0, pair=None):
    return dict(name=name, geo=(2, 7, 6, r, r, 1, pad, 1), c=c, k=k, fams=fams, cus=cus, pair=pair)


ST1 = ("glds32_st1", "reg_st1")
TILES = [
    _t("64x64_1x1_c32", 1, 0, 32, 64, ALL5, pair=(64, 64)),                    # the reduce pass's 16-byte branch (1x1, C % 4 == 0)
    _t("64x64_3x3_c3_k18", 3, 1, 3, 18, FP, pair=(64, 64)),                     # 36 columns, nine taps in one tile; C, K % 4 != 0
    _t("128x128_ragged_c72_k72", 1, 0, 72, 72, ALL5, pair=(128, 128)),          # ragged rows, one ragged column tile
    _t("128x128_two_by_two_c20_k136", 3, 1, 20, 136, FP, pair=(128, 128)),      # second row tile 8 rows, second column tile 52 columns
    _t("128x128_three_cols_c24_k136", 3, 1, 24, 136, BS, pair=(128, 128)),      # bf16 storage: Cp = 32, 288 columns, third tile 32
    _t("64x128_3x3_c10_k18", 3, 1, 10, 18, FP, pair=(64, 128)),
    _t("64x128_1x1_c72_k40", 1, 0, 72, 40, BS, pair=(64, 128)),
    _t("128x64_1x1_c32_k72", 1, 0, 32, 72, ALL5, pair=(128, 64)),
    _t("128x64_1x1_c15_k72", 1, 0, 15, 72, FP, pair=(128, 64)),                 # 1x1 with C % 4 != 0: the per-element scatter
    _t("st1_64x128_3x3_c32_k64", 3, 1, 32, 64, ST1, cus=1, pair=(64, 128)),     # three tiles on one CU; rectangles (RECT, one stage)
    _t("st1_128x64_1x1_c32_k264", 1, 0, 32, 264, ST1, cus=1, pair=(128, 64)),   # three row tiles, the third 8 rows; no table
    _t("st1_128x128_3x3_c20_k136", 3, 1, 20, 136, ST1, cus=1, pair=(128, 128)),
]
TILE_RUNS = [(t, f) for t in TILES for f in t["fams"]]


def run_id(tf):
    return f"{tf[0]['name']}-{tf[1]}"


def tile_case(dev, t, fam, guard=None):
    ref = reference(t["geo"], t["c"], t["k"], _mode(fam))
    call = Call(dev, t["geo"], t["c"], t["k"], _mode(fam), ref, guard=guard)
    what = f"tile {t['name']} {fam}"
    w, r0, pl = full_case(call, fam, what, cus=t["cus"])
    assert (pl["bm"], pl["bn"]) == t["pair"], (what, pl)
    return _report("tiles", f"{t['name']} {fam}", w)


def one_stage_64x64_case(dev, guard=None):
    """FINDING (module docstring): one 64x64 tile never exceeds two workgroups per CU.  The restated plan over every chip size
    and pixel count; the closest launch (one CU, 1024 pixels) stays on the two-stage forms."""
    for cus in list(range(1, 9)) + [16, 64, 255, 256, 304]:
        for m in (1, 256, 257, 512, 513, 1024, 4096, 65536, 1 << 20):
            pl = plan((1, 1, m, 1, 1, 1, 0, 1), 32, 32, cus)
            assert pl["tiles"] == 1 and pl["nwg"] <= 2 * cus, (cus, m, pl)
    geo = (1, 16, 64, 1, 1, 1, 0, 1)
    w = Worst()
    for fam in ("glds32", "reg"):
        call = Call(dev, geo, 32, 32, "f32", reference(geo, 32, 32, "f32"), guard=guard)
        ww, r0, pl = full_case(call, fam, f"64x64 on one CU {fam}", cus=1, accumulate=False)
        assert pl["splits"] == 2 and pl["nwg"] == 2
        w.merge(ww)
    return _report("tiles", "64x64 one CU", w)


# ---- 2. pixel counts and splits ----------------------------------------------------------------------------------------
PIXEL_SHAPES = [(1, 1), (3, 3), (1, 31), (4, 8), (3, 11), (7, 9), (8, 8), (5, 13), (33, 35)]     # M = 1 9 31 32 33 63 64 65 1155
SPLIT_COUNTS = (1, 2, 3, 4, 5, 7, 9)


def pixel_case(dev, fam, shapes=PIXEL_SHAPES, guard=None):
    w = Worst()
    for h, wd in shapes:
        geo = (1, h, wd, 1, 1, 1, 0, 1)
        ref = reference(geo, 32, 32, _mode(fam))
        call = Call(dev, geo, 32, 32, _mode(fam), ref, guard=guard)
        ww, r0, pl = full_case(call, fam, f"pixels M={h * wd} {fam}", rect=False, accumulate=h * wd in (1, 65, 1155))
        assert pl["M"] == h * wd and (h * wd != 1155 or (pl["splits"] == 5 and pl["M"] - 4 * pl["rps"] == 131)), pl
        w.merge(ww)
    return _report("pixels", fam, w)


def split_case(dev, s, fam, guard=None, square=False):
    """1x1 32 -> 32 on 256 s pixels: s splits on the real chip (16 x 16 s, or 48 x 48 for s = 9)"""
    geo = (1, 48, 48, 1, 1, 1, 0, 1) if square else (1, 16, 16 * s, 1, 1, 1, 0, 1)
    ref = reference(geo, 32, 32, _mode(fam))
    call = Call(dev, geo, 32, 32, _mode(fam), ref, guard=guard)
    w, r0, pl = full_case(call, fam, f"splits={s} {fam}", rect=False)
    assert r0.splits == s and pl["rps"] == 256, (r0.splits, pl)
    return _report("splits", f"{s} {fam}", w)


# ---- 3. the merge stays compensated ------------------------------------------------------------------------------------
KAHAN_ORDERS = {
    "2^24 first, -2^24 in the tail": [2 ** 24, 1, 1, 1, 1, 1, 1, 1, -2 ** 24],
    "-2^24 first, 2^24 in the tail": [-2 ** 24, 1, 1, 1, 1, 1, 1, 1, 2 ** 24],
    "2^24 in the second chain": [1, 2 ** 24, 1, 1, 1, 1, 1, 1, -2 ** 24],
}
KAHAN_PLAIN_WRONG = ("2^24 first, -2^24 in the tail", "2^24 in the second chain")


def plain_four_chain(partials):
    """wgrad_reduce_kernel's chain assignment WITHOUT the compensation, in numpy float32"""
    s = [np.float32(0)] * 4
    p = [np.float32(v) for v in partials]
    sp = 0
    while sp + 3 < len(p):
        for j in range(4):
            s[j] = np.float32(s[j] + p[sp + j])
        sp += 4
    while sp < len(p):
        s[0] = np.float32(s[0] + p[sp])
        sp += 1
    return float(np.float32(np.float32(np.float32(s[0] + s[1]) + s[2]) + s[3]))


def kahan_case(dev, order, fam, guard=None):
    """Exact integers, fp32, 1x1 32 -> 32 on 48 x 48 (nine splits of 256 pixels).  Element (k0, c0) has one non-zero pixel per
    split, its nine partial sums are KAHAN_ORDERS[order], the exact sum is 7; every other element sums small random integers."""
    partials = KAHAN_ORDERS[order]
    geo, c, k, k0, c0 = (1, 48, 48, 1, 1, 1, 0, 1), 32, 32, 5, 9
    g = _gen(77)
    x = torch.randint(-3, 4, (1, c, 48, 48), generator=g).float()
    dy = torch.randint(-3, 4, (1, k, 48, 48), generator=g).float()
    xf, dyf = x.view(c, -1), dy.view(k, -1)
    xf[c0], dyf[k0] = 0.0, 0.0
    for s, pv in enumerate(partials):
        m = 256 * s + 37 + 11 * s                        # one pixel inside split s
        big = abs(pv) == 2 ** 24
        xf[c0, m] = 4096.0 if big else 1.0
        dyf[k0, m] = math.copysign(4096.0 if big else 1.0, pv)
    ref = _reference_of(x, dy, geo, k, "f32")
    assert float(ref["dw"][k0, c0, 0, 0]) == 7.0
    per_split = (dyf[k0].double().view(9, 256) * xf[c0].double().view(9, 256)).sum(1)
    assert per_split.tolist() == [float(v) for v in partials]
    plain = plain_four_chain(partials)
    assert (plain != 7.0) == (order in KAHAN_PLAIN_WRONG), f"{order}: the uncompensated four-chain sum gives {plain}"
    call = Call(dev, geo, c, k, "f32", ref, guard=guard)
    pl = plan(geo, c, k)
    try:
        _tune(**FAMILIES[fam]["tune"])
        res = call.run(M_F32)
    finally:
        _tune(**DEFAULTS)
    what = f"kahan {order} {fam}"
    _ok(res, what)
    check_form(res, fam, pl, what, rect=False)
    assert res.splits == 9 and pl["rps"] == 256
    got = float(res.dw[k0, c0, 0, 0])
    assert got == 7.0, f"{what}: the merged element is {got}, not 7 (a plain sum gives {plain})"
    assert torch.equal(res.dw.double(), ref["dw"]), f"{what}: integer sums are not exact"
    assert torch.equal(res.db.double(), ref["db"]), f"{what}: integer bias sums are not exact"
    print(f"wgrad [kahan] {order} {fam}: exact (uncompensated four-chain sum: {plain})")


# ---- 4. live rectangles -------------------------------------------------------------------------------------------------
G_WASP = (1, 23, 23, 3, 3, 1, 18, 18)
G_WASP3 = (3, 23, 23, 3, 3, 1, 18, 18)
G_DIL5 = (2, 4, 4, 3, 3, 1, 5, 5)
G_S2 = (2, 9, 9, 3, 3, 2, 1, 1)
G_PLAIN = (2, 6, 6, 1, 1, 1, 0, 1)
# (name, geo, c, k, families)
RECTS = [
    ("wasp_c128_one_tap_per_tile", G_WASP, 128, 32, ("glds32", "bf16s_glds")),
    ("wasp_c32_four_taps_per_tile", G_WASP, 32, 32, ("reg", "bf16op")),
    ("dil5_on_4x4_empty_rectangles", G_DIL5, 32, 16, ALL5),
    ("stride2_output_coordinates", G_S2, 32, 24, ("glds32", "reg", "bf16s_reg")),
]
RECT_RUNS = [(dict(name=n_, geo=g_, c=c_, k=k_), f) for n_, g_, c_, k_, fams in RECTS for f in fams]


def _visits(call):
    frac = C.c_double(-1.0)
    _C.check(_C.lib().up_conv_wgrad_visits(C.byref(call.d), C.byref(frac)), "wgrad_visits")
    return frac.value


def rect_case(dev, t, fam, guard=None):
    """wgrad_rect = 1 and 0: both inside the bound, "wgrad_rect" moves only for 1"""
    ref = reference(t["geo"], t["c"], t["k"], _mode(fam))
    call = Call(dev, t["geo"], t["c"], t["k"], _mode(fam), ref, guard=guard)
    w = Worst()
    for on in (1, 0):
        ww, r0, pl = full_case(call, fam, f"rect {t['name']} {fam} wgrad_rect={on}", rect=bool(on), extra_tune=dict(wgrad_rect=on))
        w.merge(ww)
    assert _visits(call) < 0.999
    tab = rect_table(t["geo"], call.cp, pl)
    dead = ref["A_dw"] == 0
    if t["geo"] == G_WASP and t["c"] == 128:
        assert pl["bn"] == 128 and [e["rows"] * e["cols"] for e in tab] == [25, 115, 25, 115, 529, 115, 25, 115, 25], tab
    if t["geo"] == G_WASP and t["c"] == 32:
        assert [(e["rows"], e["cols"]) for e in tab] == [(23, 23), (23, 23), (5, 5)], tab        # bounding boxes of four taps; tap 8 alone
    if t["geo"] == G_DIL5:
        assert int(dead.sum()) == 8 * t["c"] * t["k"] and sum(e["mt"] == 0 for e in tab) > 0, tab    # eight taps never live
    return _report("rectangles", f"{t['name']} {fam}", w)


def no_table_case(dev, fam, guard=None):
    """1x1 without padding: no table (up_conv_wgrad_visits == 1.0), "wgrad_rect" does not move with the knob on"""
    ref = reference(G_PLAIN, 32, 32, _mode(fam))
    call = Call(dev, G_PLAIN, 32, 32, _mode(fam), ref, guard=guard)
    assert _visits(call) == 1.0
    w, r0, pl = full_case(call, fam, f"rect 1x1 no table {fam}", rect=False, extra_tune=dict(wgrad_rect=1))
    return _report("rectangles", f"no table {fam}", w)


def empty_domain_case(dev, fam, guard=None):
    """Three 23 x 23 images, dilation 18, C = 128 (one tap per column tile), seven splits: a corner tap sees 3 x 25 = 75 pixels
    in slices of 32, so splits 3 .. 6 of its tile start behind the end of their domain and must still write zeros to their
    slabs (the merge reads every slab; the workspace is NaN)."""
    c, k = 128, 32
    ref = reference(G_WASP3, c, k, _mode(fam))
    call = Call(dev, G_WASP3, c, k, _mode(fam), ref, guard=guard)
    w, r0, pl = full_case(call, fam, f"empty split domains {fam}", rect=True)
    tab = rect_table(G_WASP3, call.cp, pl)
    assert pl["splits"] == 7 and pl["ntn"] == 9
    empty = [sum(1 for sp in range(pl["splits"]) if sp * e["rps"] >= e["mt"]) for e in tab]
    assert empty == [4, 1, 4, 1, 0, 1, 4, 1, 4], (empty, tab)
    return _report("rectangles", f"empty split domains {fam}", w)


# ---- 5. bias gradient ---------------------------------------------------------------------------------------------------
BIAS_K = (1, 3, 4, 18, 64, 65, 136)
BIAS_SHAPES = [(1, 1), (3, 5), (4, 4), (1, 17), (7, 9), (8, 8), (5, 13), (1, 113), (15, 17), (16, 16), (1, 257)]   # M = 1 15 16 17 63 64 65 113 255 256 257


def bias_case(dev, k, fam, shapes=BIAS_SHAPES, guard=None):
    """per channel against float64, L = M, A = sum |dy|; the convolution is the cheapest the entry takes (1x1, C = 4 / 8)"""
    c = 8 if _mode(fam) == "bf16s" else 4
    w = Worst()
    for h, wd in shapes:
        geo = (1, h, wd, 1, 1, 1, 0, 1)
        ref = reference(geo, c, k, _mode(fam), seed=k)
        call = Call(dev, geo, c, k, _mode(fam), ref, guard=guard)
        assert call.ldy > ops.rup4(k)
        what = f"bias K={k} M={h * wd} {fam}"
        ww, r0, pl = full_case(call, fam, what, accumulate=h * wd in (17, 257))
        rows = call.partial_rows(r0, pl)
        nrows = _cdiv(h * wd, 256)
        assert not bool(torch.isnan(rows[:nrows]).any()) and bool(torch.isnan(rows[nrows:]).all()), f"{what}: partial rows"
        w.add("db", ww["db"])
    return _report("bias", f"K={k} {fam}", w)


def bias_big_case(dev, fam, guard=None):
    """64 * 256 + 1 = 16385 pixels, K = 4: 65 partial rows, lane 0 of colsum_finish_kernel adds two"""
    geo = (1, 5, 3277, 1, 1, 1, 0, 1)
    assert 5 * 3277 == 16385
    c = 8 if _mode(fam) == "bf16s" else 4
    ref = reference(geo, c, 4, _mode(fam))
    call = Call(dev, geo, c, 4, _mode(fam), ref, guard=guard)
    w, r0, pl = full_case(call, fam, f"bias 16385 pixels {fam}", accumulate=False)
    rows = call.partial_rows(r0, pl)
    assert rows.shape[0] >= 65 and not bool(torch.isnan(rows[:65]).any()) and bool(torch.isnan(rows[65:]).all())
    return _report("bias", f"16385 pixels {fam}", w)


def no_bias_case(dev, fam, guard=None):
    geo = (1, 7, 9, 1, 1, 1, 0, 1)
    ref = reference(geo, 8, 18, _mode(fam))
    call = Call(dev, geo, 8, 18, _mode(fam), ref, guard=guard)
    w, r0, pl = full_case(call, fam, f"dbias = NULL {fam}", bias=False)
    return _report("bias", f"dbias NULL {fam}", w)


# ---- 6. operands that are not 16-byte aligned ----------------------------------------------------------------------------
UNALIGNED = [("3x3_c10_k18", (2, 7, 6, 3, 3, 1, 1, 1), 10, 18), ("1x1_1025_pixels", (1, 25, 41, 1, 1, 1, 0, 1), 8, 18)]
UNALIGNED_FALLBACK = {"glds32": "reg", "bf16op": "bf16op", "bf16s_glds": "bf16s_reg"}


def unaligned_case(dev, t, fam, guard=None):
    """x and dy start one float (four bf16 elements) into their buffers, with the direct-to-LDS knobs ON: the launch must take the
    register-staged kernel and the 1024-row colsum_kernel; dw equals the aligned launch with the knob off bit for bit (the
    bias gradient is summed in another order by the two kernels: inside the bound, not equal)."""
    name, geo, c, k = t
    mode = _mode(fam)
    fb = UNALIGNED_FALLBACK[fam]
    ck = (ops.rup32(c) if mode == "bf16s" else c)
    ref = reference(geo, ck, k, mode)
    mis = Call(dev, geo, ck, k, mode, ref, guard=guard, misalign=True)
    w, r_mis, pl = full_case(mis, fb, f"unaligned {name} knobs of {fam}", extra_tune=FAMILIES[fam]["tune"])
    ali = Call(dev, geo, ck, k, mode, ref, guard=guard)
    w2, r_ali, _ = full_case(ali, fb, f"aligned {name} {fb}", accumulate=False)
    assert torch.equal(r_mis.dw, r_ali.dw), f"unaligned {name} {fam}: dw differs from the aligned register-staged launch"
    m = pl["M"]
    rows_mis, rows_ali = mis.partial_rows(r_mis, pl), ali.partial_rows(r_ali, pl)
    for rows, per in ((rows_mis, 1024), (rows_ali, 256)):
        nrows = _cdiv(m, per)
        assert not bool(torch.isnan(rows[:nrows]).any()) and bool(torch.isnan(rows[nrows:]).all()), \
            f"unaligned {name} {fam}: expected {nrows} partial rows of {per} pixels"
    w.merge(w2)
    return _report("unaligned", f"{name} {fam}", w)


# ---- 7. workspace, entries, refusals -----------------------------------------------------------------------------------
def entries_case(dev, guard=None):
    """up_conv2d_bwd_weight / _bf16 / _bf16s against up_conv2d_bwd_weight_acc with accumulate = 0: equal bits"""
    geo = (2, 7, 6, 3, 3, 1, 1, 1)
    for math_, c in ((M_F32, 10), (M_BF16, 10), (M_BF16S, 24)):
        ref = reference(geo, c, 18, MODE[math_])
        call = Call(dev, geo, c, 18, MODE[math_], ref, guard=guard)
        a, b = call.run(math_), call.run(math_, entry="old")
        _ok(a, "acc entry")
        _ok(b, "older entry")
        assert a.variant == b.variant and a.variants == b.variants and (not a.profiled or sum(a.variants.values()) == 1), (a.variants, b.variants)
        assert torch.equal(a.dw, b.dw) and torch.equal(a.db, b.db), f"math {math_}: the older entry differs from _acc"
        _check(compare(b, ref, f"older entry math {math_}"), "entries")


def refusal_case(dev, guard=None):
    """Every refusal: its code, a message that names the cause, dw / dbias / workspace untouched, no counter moved, nothing in
    the profile.  The first one is the defect this module found: a workspace that holds the slabs but not the bias gradient's
    partial rows was refused AFTER the weight gradient had been written (and, under accumulate, added)."""
    geo = (2, 7, 6, 3, 3, 1, 1, 1)
    ref = reference(geo, 24, 32, "f32")
    refb = reference(geo, 24, 32, "bf16s")
    call, callb = Call(dev, geo, 24, 32, "f32", ref, guard=guard), Call(dev, geo, 24, 32, "bf16s", refb, guard=guard)
    pl = plan(geo, call.cp, 32)
    slabs = pl["splits"] * 32 * pl["ncols"] * 4
    old = (ref["old_dw"], ref["old_db"])

    def bad(call_, **kw):
        d = _C.ConvDesc.from_buffer_copy(call_.d)
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    cases = [
        ("workspace of exactly the slabs with dbias", call, M_F32, dict(ws_bytes=slabs, accumulate=1, old=old), -4, "bias gradient's partial rows"),
        ("workspace of exactly the slabs with dbias, overwrite", call, M_BF16, dict(ws_bytes=slabs), -4, "bias gradient's partial rows"),
        ("workspace one byte short of the slabs", call, M_F32, dict(ws_bytes=slabs - 1), -4, "workspace"),
        ("null x", call, M_F32, dict(null=("x",)), -1, "null pointer"),
        ("null dy", call, M_BF16, dict(null=("dy",)), -1, "null pointer"),
        ("null dw", call, M_F32, dict(null=("dw",)), -1, "null pointer"),
        ("null workspace", call, M_F32, dict(null=("ws",)), -1, "null pointer"),
        ("ldy % 4", call, M_F32, dict(d=bad(call, ldy=call.ldy + 2)), -1, "multiple of 4"),
        ("math = bf16x3", call, 1, dict(), -1, "math mode 1"),
        ("math = 4", call, 4, dict(), -1, "math mode 4"),
        ("math = -1", call, -1, dict(), -1, "math mode -1"),
        ("bf16 storage, Cp % 8", callb, M_BF16S, dict(d=bad(callb, Cp=28, C=24)), -1, "multiples of 8"),
        ("bf16 storage, ldx % 8", callb, M_BF16S, dict(d=bad(callb, ldx=callb.ldx + 4)), -1, "multiples of 8"),
        ("bf16 storage, ldy % 8", callb, M_BF16S, dict(d=bad(callb, ldy=callb.ldy + 4)), -1, "multiples of 8"),
        ("bf16s entry, ldy % 8", callb, M_BF16S, dict(d=bad(callb, ldy=callb.ldy + 4), entry="old"), -1, "multiples of 8"),
    ]
    for what, cl, math_, kw, code, text in cases:
        kw = dict(kw)
        if "old" not in kw:
            kw["old"] = (cl.ref["old_dw"], cl.ref["old_db"])       # finite outputs: "untouched" compares bits either way
        res = cl.run(math_, **kw)
        assert res.code == code, f"refusal {what}: returned {res.code}, expected {code} ({res.msg})"
        assert text in res.msg, f"refusal {what}: up_last_error = {res.msg!r} does not name the cause ({text!r})"
        assert res.untouched, f"refusal {what}: the refused call wrote dw, dbias or the workspace"
        assert not any(res.moved.values()) and not res.variants, f"refusal {what}: launched {res.moved} {res.variants}"
    # the same workspace is enough without a bias gradient
    ok = call.run(M_F32, bias=False, ws_bytes=slabs)
    _ok(ok, "workspace of exactly the slabs, dbias = NULL")
    _check(compare(ok, ref, "workspace of exactly the slabs, dbias = NULL", bias=False), "refusals")
    # one ordinary 3x3 launch after the refusals
    w, _, _ = full_case(call, "glds32", "3x3 after the refusals")
    return _report("refusals", "3x3 afterwards", w)
