"""The evaluation and data-contract entries of the C ABI off the square maps: up_heatmap_argmax, up_pck_accuracy, up_make_heatmaps,
up_make_gaussian_maps, up_normalize_image, the ConvLSTM gate entries and the dropout entries, each against a plain reference of
the same operation at the shapes where a kernel goes wrong: H != W in both orientations, H * W around one wavefront, map counts
that are no multiple of 4, J in the second wavefront of the PCK workgroup, totals that are no multiple of 256, independent leading
dimensions, the second trip of a grid-stride loop (shared by test_contract_emu.py and test_contract_gpu.py).

References: numpy.argmax / max and oracle.get_max_preds; the genuine reference's `accuracy` through the fixture G18
(tools/make_goldens.py g18: all seven datasets on 12 x 20 and 20 x 12 maps) and oracle.accuracy, which G7 and G18 pin, beyond it;
oracle.make_heatmap / make_centermap, which G8 pins, under the rule of op_cases.check_target_maps; float32 (x - mean) / std of
torch on the CPU, bit for bit; the hash of norm_act.hip restated in numpy uint64 arithmetic, mask for mask; the formulas of
model/uniposeLSTM.py:17-22, 41-62 in float64, per element.

ConvLSTM bound.  u = 2^-24; every output element obeys |got - ref64| <= K_LSTM u m with m the output's natural magnitude from
the float64 reference:
    lstm0 cell, hide                 m = 1
    lstm  cell, hide                 m = 1 + |cprev|   (hide = o tanh(cell): the rounding of cell, up to u (1 + |cprev|), passes
                                                        through a slope <= 1)
    dgates g | i | o, dcprev         m = |dcell| + |dhide|
    dgates f                         m = (|dcell| + |dhide|) |cprev|
K_LSTM was fixed BEFORE any kernel ran, from the reference's own error: the same formulas evaluated in float32 by torch on the CPU
over these very inputs (host_float32_ratio(), `PYTHONPATH=. python tests/contract_cases.py`) are off by at most 3.129 u m (the
worst output: dgates of lstm0 at scale 1; no output is below 1.9); four times that, rounded up to a power of two: K_LSTM = 16.
The kernels' worst |got - ref64| / (u m): emulator 3.030, MI355X 3.090 (test_contract_gpu.py lists them per entry): the device
tanhf / expf are no looser than the host's here.
up_lstm_bwd reads `cell` as an input: the tests hand it the float64 cell rounded to float32, so the backward entries are judged
on their own.  Lanes >= Cg of every written buffer, and the lanes of dgates between 3 Cg (4 Cg) and ldg, keep a sentinel; input pad
lanes hold NaN.  dcprev is [rows][ldo] (include/unipose_hip.h); its buffer is max(ldo, ldc) wide, so a kernel that used ldc would
leave its marks in the rows it must not touch instead of writing out of bounds.
Scales: 1 and 6 are randn * scale (at 6, 1 - tanh^2 cancels); 40 is randn * 40 under the same bound AND a saturated draw,
+-[40, 80]: there every result is finite and every dgates element is below e^-40 m.  Not "exactly 0" as the issue has it: the
factors that saturate to 1 give an exact 0 (dgates g always), but sigmoid(-40) = e^-40 = 4.2e-18 is a normal float32, so
i (1 - i), o (1 - o) and f (1 - f) are that small and not 0, in float64 as well.

Dropout: the mask is a pure function of (seed, index), so the byte mask must equal the numpy restatement for every element, fp32
and bf16 alike; y = fl32(x * fl32(1 / (1 - p))) where kept (rounded to nearest-even for bf16: torch's own cast), +0 elsewhere;
p = 0 keeps everything and returns x bit for bit.  threshold_case sets p to one element's own h 2^-24: `>= p` keeps it.
"""
import math
import os

import numpy as np
import torch

from op_cases import check_target_maps
from oracle import unipose_oracle as O
from unipose_amd import _C, ops

BF = torch.bfloat16
F32 = torch.float32
U = 2.0 ** -24
SENT = 7.0
K_LSTM = 16.0
E40 = math.exp(-40.0)
MASK64 = 2 ** 64 - 1
GOLDEN_STEP = 0x9E3779B97F4A7C15
NEED = dict(LSP=15, COCO=14, Penn_Action=9, NTID=5, PoseTrack=14, BBC=8, MPII=11)
WORST = {}          # worst |got - ref64| / (u m) per ConvLSTM entry, and what the exact cases saw


def _gen(seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return gen


def _worst(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


def _same_bits(a, b):
    """equal float32 arrays bit for bit (a NaN equals a NaN: numpy does not promise which payload np.max returns)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def _p(t):
    return None if t is None else t.data_ptr()


# ---- 1. up_heatmap_argmax -------------------------------------------------------------------------------
ARGMAX_SHAPES = [(1, 1, 1, 1), (2, 3, 1, 7), (1, 5, 7, 1), (1, 1, 8, 8), (1, 2, 3, 21), (3, 5, 5, 13), (2, 4, 9, 31), (1, 7, 3, 50)]


def _argmax_entry(hm_d, with_idx=True):
    b, j, h, w = hm_d.shape
    idx = torch.full((b, j), -77, dtype=torch.int32, device=hm_d.device)
    preds = torch.full((b, j, 2), SENT, dtype=F32, device=hm_d.device)
    mx = torch.full((b, j, 1), SENT, dtype=F32, device=hm_d.device)
    _C.check(_C.lib().up_heatmap_argmax(hm_d.data_ptr(), b, j, h, w, _p(idx) if with_idx else None, preds.data_ptr(), mx.data_ptr(),
                                        ops._stream(hm_d)), "heatmap_argmax")
    return preds.cpu().numpy(), mx.cpu().numpy(), idx.cpu().numpy()


def _argmax_check(dev, hm, what):
    """idx / preds / maxvals of the entry, of the entry without idx and of ops.heatmap_decode(size=None) against numpy"""
    b, j, h, w = hm.shape
    flat = hm.reshape(b, j, -1)
    with np.errstate(invalid="ignore"):
        ref_idx, ref_mx = flat.argmax(2).astype(np.int32), flat.max(2)[:, :, None]
        ref_preds, o_mx = O.get_max_preds(hm)
    assert _same_bits(o_mx, ref_mx)
    hm_d = torch.from_numpy(hm).to(dev)
    preds, mx, idx = _argmax_entry(hm_d)
    assert np.array_equal(idx, ref_idx), (what, idx, ref_idx)
    assert _same_bits(preds, ref_preds), (what, preds, ref_preds)
    assert _same_bits(mx, ref_mx), (what, mx, ref_mx)
    preds0, mx0, idx0 = _argmax_entry(hm_d, with_idx=False)
    assert _same_bits(preds0, preds) and _same_bits(mx0, mx) and bool((idx0 == -77).all()), what
    dp, dm, di = ops.heatmap_decode(hm_d)
    assert _same_bits(dp.cpu().numpy(), preds) and _same_bits(dm.cpu().numpy(), mx) and np.array_equal(di.cpu().numpy(), idx), what
    return preds, mx, idx


def argmax_shape_case(dev, shape):
    rng = np.random.default_rng([1, *shape])
    _argmax_check(dev, rng.standard_normal(shape).astype(np.float32), shape)


def argmax_planted_case(dev):
    """a 9 x 31 map (279 elements: every lane walks more than four of them)"""
    rng = np.random.default_rng(2)
    h, w = 9, 31
    hm = rng.standard_normal((2, 4, h, w)).astype(np.float32)
    m = hm.reshape(8, h * w)
    nan, inf = np.float32("nan"), np.float32("inf")
    m[0] = -5.0 - np.abs(m[0]); m[0, -1] = 3.0               # the maximum in the last element
    m[1, 70] = m[1, 134] = 9.0                               # equal maxima 64 apart: one lane sees both
    m[2, 200] = m[2, 201] = 9.0                              # equal maxima in neighbouring lanes
    m[3, 150] = nan                                          # one NaN
    m[4, 50] = 1e30; m[4, 100] = nan; m[4, 230] = nan        # two NaNs behind a larger number: the first NaN
    m[5, 77] = inf
    m[6] = -inf                                              # only -inf: idx 0
    m[7] = -np.abs(m[7]) - 0.5                               # only negative values
    preds, mx, idx = _argmax_check(dev, hm, "planted")
    want = [h * w - 1, 70, 200, 150, 100, 77, 0, int(m[7].argmax())]
    assert idx.reshape(-1).tolist() == want, (idx, want)
    pr, mv = preds.reshape(8, 2), mx.reshape(8)
    assert pr[0].tolist() == [w - 1, h - 1] and pr[1].tolist() == [70 % w, 70 // w] and pr[2].tolist() == [200 % w, 200 // w]
    assert np.isnan(mv[3]) and np.isnan(mv[4]) and pr[3].tolist() == [0, 0] and pr[4].tolist() == [0, 0]
    assert mv[5] == inf and pr[5].tolist() == [77 % w, 77 // w]
    assert mv[6] == -inf and pr[6].tolist() == [0, 0]
    assert mv[7] == m[7].max() and mv[7] < 0 and pr[7].tolist() == [0, 0]


# ---- 2. up_pck_accuracy ---------------------------------------------------------------------------------
G18_STACKS = [f"{ds}_{h}x{w}_j{j}" for ds in O.DATASETS for h, w in ((12, 20), (20, 12)) for j in (NEED[ds], NEED[ds] + 3)]
_G18 = {}


def _g18(golden_dir):
    if not _G18:
        _G18.update(np.load(os.path.join(golden_dir, "g18_accuracy_rect.npz")))
    return _G18


def _equal_accuracy(got, ref, what):
    for name, a, b in zip(("acc", "pck", "pckh"), got[:3], ref[:3]):
        assert a.dtype == np.float64 and np.array_equal(a, np.asarray(b, dtype=np.float64)), (what, name, a, b)
    assert got[3] == int(ref[3]), (what, "cnt", got[3], ref[3])
    assert np.array_equal(got[4], ref[4]) and np.array_equal(got[5], ref[5]), (what, "pred / visible")


def pck_golden_case(dev, golden_dir, stack):
    """ops.accuracy == the genuine reference (G18), exactly"""
    g = _g18(golden_dir)
    ds = stack.rsplit("_", 2)[0]
    out, tgt = torch.from_numpy(g[stack + "_out"]).to(dev), torch.from_numpy(g[stack + "_tgt"]).to(dev)
    for tag in ("std", "tight"):
        tk, th = (float(v) for v in g[f"{stack}_{tag}_thr"])
        k = f"{stack}_{tag}_"
        _equal_accuracy(ops.accuracy(out, tgt, tk, th, ds), [g[k + n] for n in ("acc", "pck", "pckh", "cnt", "pred", "vis")], k)


def _pck_maps(seed, b, j, h, w, invisible=()):
    """peaked heat-map stacks like G18's; `invisible`: joints whose targets all lie in column 0 or 1 ("all": every joint)"""
    rng = np.random.default_rng(seed)
    tgt = np.zeros((b, j, h, w), np.float32)
    out = (rng.integers(-8, 8, (b, j, h, w)) / 64.0).astype(np.float32)
    for n in range(b):
        for c in range(j):
            ty, tx = int(rng.integers(0, h)), int(rng.integers(0, w))
            if invisible == "all" or c in invisible or rng.random() < 0.15:
                tx = int(rng.integers(0, 2))
            tgt[n, c, ty, tx] = 1.0
            dy, dx = rng.integers(-4, 5, 2) * (0 if invisible and c % 2 else 1)      # (odd joints exact when some are hidden)
            out[n, c, int(np.clip(ty + dy, 0, h - 1)), int(np.clip(tx + dx, 0, w - 1))] = 2.0 + rng.random()
    return out, tgt


def pck_oracle_case(dev, ds, j, b=3, mode=None):
    """beyond the fixture, against oracle.accuracy on 12 x 20 maps: J in the second wavefront (70) and at the limit (256), B = 1,
    no visible target at all (cnt == 0: all results 0, entry 0 NOT a mean), joint 0 invisible (entry 0 still the mean)"""
    h, w = 12, 20
    inv = {"all_invisible": "all", "joint0_invisible": (0,)}.get(mode, ())
    out, tgt = _pck_maps([3, O.DATASETS.index(ds), j, b], b, j, h, w, inv)
    for tk, th in ((0.2, 0.5), (0.03, 0.12)):
        ref = O.accuracy(out, tgt, tk, th, ds)
        got = ops.accuracy(torch.from_numpy(out).to(dev), torch.from_numpy(tgt).to(dev), tk, th, ds)
        _equal_accuracy(got, ref, (ds, j, b, mode, tk))
        if mode == "all_invisible":
            assert got[3] == 0 and not got[5].any() and all(not r.any() for r in got[:3]), got
        if mode == "joint0_invisible":
            vis = got[5] > 0
            assert got[5][0] == 0 and got[3] == int(vis.sum()) > 0
            assert got[0][0] == ref[0][0] and got[0][0] > 0      # the mean over the visible joints, not joint 0's own 0


def pck_refusal_case(dev):
    """J = 257, J one below each dataset's minimum, dataset id -1 and 7, a null pointer: the return code of the header, nothing written"""
    L = _C.lib()
    b, h, w = 2, 12, 20
    pred = torch.rand(b, 257, 2, generator=_gen(0)).mul(10).floor().to(dev)
    tgt = torch.rand(b, 257, 2, generator=_gen(1)).mul(10).floor().add(2).to(dev)
    res = torch.full((4, 257), SENT, dtype=torch.float64, device=dev)
    cnt = torch.full((1,), -77, dtype=torch.int32, device=dev)

    def call(j, ds, null=None):
        a = [pred.data_ptr(), tgt.data_ptr(), b, j, h, w, ds, 0.2, 0.5, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(),
             res[3].data_ptr(), cnt.data_ptr(), ops._stream(pred)]
        if null is not None:
            a[null] = None
        rc = L.up_pck_accuracy(*a)
        assert bool((res.cpu() == SENT).all()) and int(cnt.item()) == -77, ("written", j, ds, null)
        return rc

    assert call(257, 0) == -2 and b"257" in L.up_last_error()                 # UP_ERR_UNSUPPORTED
    assert call(0, 0) == -2
    for ds, name in enumerate(O.DATASETS):
        assert call(NEED[name] - 1, ds) == -1, name                           # UP_ERR_INVALID
    assert call(20, -1) == -1 and call(20, 7) == -1
    for null in (0, 1, 9, 10, 11, 12, 13):
        assert call(20, 0, null) == -1, null


# ---- 3. up_make_heatmaps / up_make_gaussian_maps --------------------------------------------------------
HEATMAP_CASES = [(96, 160, 8, 3.0, 3, 2), (100, 50, 3, 1.5, 2, 2), (16, 40, 8, 1.0, 1, 1), (368, 200, 8, 0.5, 14, 1)]
CENTERMAP_SIZES = [(1, 1), (1, 300), (300, 1), (37, 53)]


def heatmaps_case(dev, case):
    """non-square maps, a stride that does not divide the image (100 / 3: 33 rows), K = 1, negative coordinates (int() truncates
    towards zero), a joint whose map is all zero, a joint exactly on a grid point"""
    height, width, stride, sigma, K, B = case
    h, w = int(height / stride), int(width / stride)
    assert h != w
    gx, gy = min(3, w - 1), min(2, h - 1)
    plants = [("neg", (-0.5, -0.5)), ("trunc", (-1.5, 3.99999999)), ("far", (-1e4, 3e4)), ("grid", (float(gx * stride), float(gy * stride)))]
    rng = np.random.default_rng([4, *case[:3]])
    slots = B * K
    for first in range(0, len(plants), slots):
        kpt = np.stack([rng.uniform(-20, width + 20, (B, K)), rng.uniform(-20, height + 20, (B, K))], axis=2)
        planted = {}
        for s, (name, xy) in enumerate(plants[first:first + slots]):
            kpt[s // K, s % K] = xy
            planted[name] = (s // K, s % K)
        got = ops.make_heatmaps(kpt, height, width, stride, sigma, dev)
        assert tuple(got.shape) == (B, K + 1, h, w)
        ref = np.stack([O.make_heatmap(k, height, width, stride, sigma) for k in kpt])
        check_target_maps(got, ref, (case, first))
        g = got.cpu().numpy()
        if "far" in planted:
            bb, kk = planted["far"]
            assert not g[bb, kk + 1].any()
            nothing = ~g[bb, 1:].any(axis=0)                       # no joint reaches: the background is exactly 1
            assert bool((g[bb, 0][nothing] == 1.0).all())
        if "grid" in planted:
            bb, kk = planted["grid"]
            assert g[bb, kk + 1, gy, gx] == 1.0 and g[bb, 0, gy, gx] == 0.0
        if "neg" in planted:                                       # int(-0.5) = 0: centred on pixel (0, 0)
            bb, kk = planted["neg"]
            assert g[bb, kk + 1, 0, 0] == 1.0


def centermaps_case(dev, size, n):
    """1 x 1, one row, one column and an odd rectangle; centres inside, on the border and outside"""
    h, w = size
    centres = np.array([[w / 2.3, h / 2.7], [w - 1.0, 0.0], [-4.5, h + 2.0]])
    for c in ([centres] if n == 3 else [centres[i:i + 1] for i in range(3)]):
        got = ops.make_centermaps(c, h, w, 3.0, dev)
        assert tuple(got.shape) == (len(c), 1, h, w)
        check_target_maps(got, np.stack([O.make_centermap(x, h, w, 3.0) for x in c]), (size, n, c.tolist()))


# ---- 4. up_normalize_image ------------------------------------------------------------------------------
NORMALIZE_SHAPES = [(1, 1, 1, 1), (1, 5, 7, 1), (2, 7, 5, 3), (3, 37, 41, 4), (1, 16, 16, 3)]
NORMALIZE_DIVISORS = [(128.0, 256.0), (127.5, 58.395)]


def normalize_case(dev, shape, divisor):
    """C != 3 and a divisor that is no power of two: the bits of torch's float32 (x - mean) / std on the CPU, i.e. the device
    division must be correctly rounded.  Measured on the MI355X: 0 ulps off at every shape and both divisors, so the kernel keeps
    its plain `/` and this stays an equality (no one-ulp bound was needed)."""
    mean, std = divisor
    img = torch.randint(0, 256, shape, generator=_gen(5)).float()
    img.view(-1)[0] = 255.0
    got = ops.normalize_image(img.to(dev), mean, std).cpu()
    chw = img.permute(0, 3, 1, 2).contiguous()
    ref = (chw - torch.full_like(chw, mean)) / torch.full_like(chw, std)      # element-wise IEEE float32 division
    assert got.shape == ref.shape
    diff = (got.view(torch.int32) - ref.view(torch.int32)).abs().max().item()
    _worst("normalize ulps off (std %g)" % std, diff)
    assert diff == 0, (shape, divisor, "float32 ulps off:", diff)


# ---- 5. ConvLSTM gate entries, direct -------------------------------------------------------------------
LSTM_CG = (1, 5, 16, 48)
LSTM_ROWS = (1, 37, 300)
LSTM_SCALES = (1.0, 6.0, 40.0, "saturated")
LSTM_BIG = (48, 43700)        # 2 097 600 elements: one past the 8192 x 256 of the grid's first trip


rup4 = ops.rup4


def lstm_lds(cg, gates):
    """(ldg, ldo, ldc) of the issue's table; ldc always differs from ldo"""
    ldgs = (rup4(3 * cg), 3 * cg + 8) if gates == 3 else (4 * cg + 8,)
    out = []
    for ldg in ldgs:
        for ldo in (cg, rup4(cg) + 4):
            if gates == 3:
                out.append((ldg, ldo, None))
            else:
                out += [(ldg, ldo, ldc) for ldc in (rup4(cg), rup4(cg) + 8) if ldc != ldo]
    return out


def _lstm_inputs(cg, rows, gates, scale):
    gen = _gen(1000 * cg + rows + 7 * gates + (int(scale) if scale != "saturated" else 99))
    if scale == "saturated":
        mag = 40.0 + 40.0 * torch.rand(rows, gates * cg, generator=gen)
        G = torch.where(torch.rand(rows, gates * cg, generator=gen) < 0.5, -mag, mag)
    else:
        G = torch.randn(rows, gates * cg, generator=gen) * scale
    cprev = torch.randn(rows, cg, generator=gen) * 1.5
    dcell = torch.randn(rows, cg, generator=gen)
    dhide = torch.randn(rows, cg, generator=gen)
    return G, cprev, dcell, dhide


def lstm_reference(G, cprev, dcell, dhide, cg, dtype=torch.float64):
    """model/uniposeLSTM.py:17-22 (cprev None) / 41-62 and their derivatives, written out; -> dict of (value, m).  The backward of
    the four-gate cell takes tanh of the float32-rounded float64 cell, which is what the tests hand to up_lstm_bwd."""
    G, dcell, dhide = G.to(dtype), dcell.to(dtype), dhide.to(dtype)
    gg, ii, oo = torch.tanh(G[:, :cg]), torch.sigmoid(G[:, cg:2 * cg]), torch.sigmoid(G[:, 2 * cg:3 * cg])
    m = dcell.abs().double() + dhide.abs().double()
    if cprev is None:
        cell = torch.tanh(gg * ii)
        one = torch.ones_like(m)
        dc = dcell + dhide * oo
        dgi = dc * (1 - cell * cell)
        dG = torch.cat([dgi * ii * (1 - gg * gg), dgi * gg * ii * (1 - ii), dhide * cell * oo * (1 - oo)], 1)
        return dict(cell=(cell, one), hide=(oo * cell, one), dgates=(dG, torch.cat([m, m, m], 1)))
    cp = cprev.to(dtype)
    ff = torch.sigmoid(G[:, 3 * cg:4 * cg])
    cell = ff * cp + ii * gg
    mc = 1 + cprev.abs().double()
    cell_in = lstm_cell_input(G, cprev, cg).to(dtype)
    tc = torch.tanh(cell_in)
    dc = dcell + dhide * oo * (1 - tc * tc)
    dG = torch.cat([dc * ii * (1 - gg * gg), dc * gg * ii * (1 - ii), dhide * tc * oo * (1 - oo), dc * cp * ff * (1 - ff)], 1)
    return dict(cell=(cell, mc), hide=(oo * torch.tanh(cell), mc), dgates=(dG, torch.cat([m, m, m, m * cprev.abs().double()], 1)),
                dcprev=(dc * ff, m))


def lstm_cell_input(G, cprev, cg):
    """the `cell` argument of up_lstm_bwd: the float64 cell rounded to float32"""
    G, cp = G.double(), cprev.double()
    return (torch.sigmoid(G[:, 3 * cg:4 * cg]) * cp + torch.sigmoid(G[:, cg:2 * cg]) * torch.tanh(G[:, :cg])).float()


def _padded(x, ld, fill):
    out = torch.full((x.shape[0], ld), fill, dtype=F32)
    out[:, :x.shape[1]] = x
    return out


def _lstm_judge(name, got, ref, live, saturated=False):
    """got [rows][ld] from the device; ref = (value64, m); lanes >= live must hold the sentinel"""
    val, m = ref
    got = got.cpu()
    assert bool((got[:, live:] == SENT).all()), (name, "a lane >= %d was written" % live)
    g = got[:, :live].double()
    assert bool(torch.isfinite(g).all()), (name, "not finite")
    ratio = float(((g - val.double()).abs() / (U * m)).max())
    _worst(name, ratio)
    assert ratio <= K_LSTM, (name, "worst |got - ref64| / (u m) = %.3f > %g" % (ratio, K_LSTM))
    if saturated and "dgates" in name:
        assert bool((g.abs() <= 1.01 * E40 * m).all()) and bool((g[:, :live // (3 if "lstm0" in name else 4)] == 0).all()), (name, "not vanished")


def lstm0_case(dev, cg, rows, scales=LSTM_SCALES, lds=None):
    L = _C.lib()
    for scale in scales:
        G, _, dcell, dhide = _lstm_inputs(cg, rows, 3, scale)
        ref = lstm_reference(G, None, dcell, dhide, cg)
        sat = scale == "saturated"
        for ldg, ldo, _ in (lds or lstm_lds(cg, 3)):
            Gd = _padded(G, ldg, math.nan).to(dev)
            cell, hide = torch.full((rows, ldo), SENT).to(dev), torch.full((rows, ldo), SENT).to(dev)
            _C.check(L.up_lstm0_fwd(Gd.data_ptr(), ldg, cell.data_ptr(), hide.data_ptr(), ldo, rows, cg, ops._stream(Gd)), "lstm0_fwd")
            _lstm_judge("lstm0_fwd cell", cell, ref["cell"], cg)
            _lstm_judge("lstm0_fwd hide", hide, ref["hide"], cg)
            dcd, dhd = _padded(dcell, ldo, math.nan).to(dev), _padded(dhide, ldo, math.nan).to(dev)
            dG = torch.full((rows, ldg), SENT).to(dev)
            _C.check(L.up_lstm0_bwd(Gd.data_ptr(), ldg, dcd.data_ptr(), dhd.data_ptr(), ldo, dG.data_ptr(), rows, cg, ops._stream(Gd)),
                     "lstm0_bwd")
            _lstm_judge("lstm0_bwd dgates", dG, ref["dgates"], 3 * cg, sat)


def lstm_case(dev, cg, rows, scales=LSTM_SCALES, lds=None):
    L = _C.lib()
    for scale in scales:
        G, cprev, dcell, dhide = _lstm_inputs(cg, rows, 4, scale)
        ref = lstm_reference(G, cprev, dcell, dhide, cg)
        cell_in = lstm_cell_input(G, cprev, cg)
        sat = scale == "saturated"
        for ldg, ldo, ldc in (lds or lstm_lds(cg, 4)):
            assert ldc != ldo
            Gd, cpd = _padded(G, ldg, math.nan).to(dev), _padded(cprev, ldc, math.nan).to(dev)
            cell, hide = torch.full((rows, ldo), SENT).to(dev), torch.full((rows, ldo), SENT).to(dev)
            _C.check(L.up_lstm_fwd(Gd.data_ptr(), ldg, cpd.data_ptr(), ldc, cell.data_ptr(), hide.data_ptr(), ldo, rows, cg,
                                   ops._stream(Gd)), "lstm_fwd")
            _lstm_judge("lstm_fwd cell", cell, ref["cell"], cg)
            _lstm_judge("lstm_fwd hide", hide, ref["hide"], cg)
            cid, dcd, dhd = (_padded(t, ldo, math.nan).to(dev) for t in (cell_in, dcell, dhide))
            dG = torch.full((rows, ldg), SENT).to(dev)
            wide = max(ldo, ldc)                       # dcprev is [rows][ldo]: the first rows * ldo elements of this buffer
            dcp = torch.full((rows * wide,), SENT).to(dev)
            _C.check(L.up_lstm_bwd(Gd.data_ptr(), ldg, cpd.data_ptr(), ldc, cid.data_ptr(), dcd.data_ptr(), dhd.data_ptr(), ldo,
                                   dG.data_ptr(), dcp.data_ptr(), rows, cg, ops._stream(Gd)), "lstm_bwd")
            _lstm_judge("lstm_bwd dgates", dG, ref["dgates"], 4 * cg, sat)
            assert bool((dcp[rows * ldo:] == SENT).all()), "lstm_bwd wrote behind dcprev[rows][ldo]"
            _lstm_judge("lstm_bwd dcprev", dcp[:rows * ldo].view(rows, ldo), ref["dcprev"], cg)


def lstm_refusal_case(dev):
    """a leading dimension below the live width: UP_ERR_INVALID, nothing written"""
    L = _C.lib()
    t = torch.full((4, 32), SENT).to(dev)
    o = [torch.full((4, 32), SENT).to(dev) for _ in range(4)]
    p = t.data_ptr()
    assert L.up_lstm0_fwd(p, 14, o[0].data_ptr(), o[1].data_ptr(), 8, 4, 5, 0) == -1
    assert L.up_lstm0_fwd(p, 16, o[0].data_ptr(), o[1].data_ptr(), 4, 4, 5, 0) == -1
    assert L.up_lstm_fwd(p, 20, p, 4, o[0].data_ptr(), o[1].data_ptr(), 8, 4, 5, 0) == -1
    assert L.up_lstm_bwd(p, 20, p, 8, p, p, p, 4, o[2].data_ptr(), o[3].data_ptr(), 4, 5, 0) == -1
    assert L.up_lstm_bwd(p, 20, p, 8, p, p, p, 8, o[2].data_ptr(), None, 4, 5, 0) == -1
    assert L.up_lstm0_bwd(p, 16, p, p, 8, o[2].data_ptr(), 0, 5, 0) == -1
    assert all(bool((x.cpu() == SENT).all()) for x in o)


def host_float32_ratio():
    """the figure that fixed K_LSTM: the worst |float32 - float64| / (u m) of the reference formulas evaluated in float32 by
    torch on the CPU, over the inputs of every emulator / GPU case (the 43 700-row one included)"""
    worst = {}
    shapes = [(cg, rows) for cg in LSTM_CG for rows in LSTM_ROWS] + [LSTM_BIG]
    for cg, rows in shapes:
        for gates in (3, 4):
            for scale in (LSTM_SCALES if (cg, rows) != LSTM_BIG else (1.0,)):
                G, cprev, dcell, dhide = _lstm_inputs(cg, rows, gates, scale)
                cp = cprev if gates == 4 else None
                r64, r32 = lstm_reference(G, cp, dcell, dhide, cg), lstm_reference(G, cp, dcell, dhide, cg, F32)
                for k in r64:
                    name = "lstm%s %s @%s" % ("0" if gates == 3 else "", k, scale)
                    worst[name] = max(worst.get(name, 0.0), float(((r32[k][0].double() - r64[k][0]).abs() / (U * r64[k][1])).max()))
    return worst


# ---- 6. dropout -----------------------------------------------------------------------------------------
DROPOUT_N = (1, 255, 256, 257, 1031)
DROPOUT_P = (0.0, 0.3, 0.5, 0.999)
DROPOUT_SEEDS = (0, 0x5EED, MASK64)
DROPOUT_BIG = 4194304 + 513        # past the 16384-block cap: the grid-stride loop's second trip


def hash24(seed, n):
    """mix_hash of norm_act.hip for the indices 0 .. n - 1 in numpy uint64 arithmetic (which wraps modulo 2^64)"""
    u = np.uint64
    v = u(seed & MASK64) ^ (np.arange(n, dtype=np.uint64) * u(GOLDEN_STEP))
    v ^= v >> u(30)
    v *= u(0xBF58476D1CE4E5B9)
    v ^= v >> u(27)
    v *= u(0x94D049BB133111EB)
    v ^= v >> u(31)
    return (v >> u(40)).astype(np.uint32)


def keep_mask(seed, n, p):
    return torch.from_numpy((hash24(seed, n).astype(np.float32) * np.float32(2.0 ** -24)) >= np.float32(p))


def _inv_keep(p):
    return torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == BF else torch.int32)


def _dropout_x(n, dtype, seed):
    x = torch.randn(n, generator=_gen(seed)) * 3
    x[0] = -0.0
    return x.to(dtype)


def _dropout_call(dev, x, p, seed, ext=None, step=None, entry="up_dropout_fwd_step_t"):
    """-> rc, y, mask with 8 guard elements behind each"""
    n = x.numel()
    xd = x.to(dev)
    y = torch.full((n + 8,), SENT, dtype=x.dtype, device=dev)
    mask = torch.full((n + 8,), 0xAA, dtype=torch.uint8, device=dev)
    L, dt, st = _C.lib(), 1 if x.dtype == BF else 0, ops._stream(xd)
    if entry == "up_dropout_fwd_step_t":
        rc = L.up_dropout_fwd_step_t(xd.data_ptr(), y.data_ptr(), mask.data_ptr(), _p(ext), n, p, seed, _p(step), dt, st)
    else:
        rc = L.up_dropout_fwd_t(xd.data_ptr(), y.data_ptr(), mask.data_ptr(), _p(ext), n, p, seed, dt, st)
    return rc, y, mask


def _dropout_judge(dev, x, p, keep, y, mask, what):
    n = x.numel()
    inv = _inv_keep(p)
    assert bool((mask[n:].cpu() == 0xAA).all()) and bool((y[n:].cpu().float() == SENT).all()), (what, "wrote past n")
    got_keep = mask[:n].cpu()
    assert got_keep.dtype == torch.uint8 and int(got_keep.max()) <= 1
    bad = (got_keep.bool() != keep).nonzero().reshape(-1)
    assert bad.numel() == 0, (what, "mask differs at", bad[:8].tolist(), "of", int(bad.numel()))
    want = torch.where(keep, (x.float() * inv).to(x.dtype), torch.zeros((), dtype=x.dtype))
    assert torch.equal(_bits(y[:n]), _bits(want)), (what, "y")
    if p == 0.0:
        assert torch.equal(_bits(y[:n]), _bits(x)), (what, "p = 0 must return x bit for bit")
    dy = (torch.randn(n, generator=_gen(n + 1)) * 2).to(x.dtype)
    dx = torch.full((n + 8,), SENT, dtype=x.dtype, device=dev)
    dyd = dy.to(dev)
    _C.check(_C.lib().up_dropout_bwd_t(dyd.data_ptr(), mask.data_ptr(), dx.data_ptr(), n, p, 1 if x.dtype == BF else 0, ops._stream(dyd)),
             "dropout_bwd")
    want = torch.where(keep, (dy.float() * inv).to(x.dtype), torch.zeros((), dtype=x.dtype))
    assert torch.equal(_bits(dx[:n]), _bits(want)) and bool((dx[n:].cpu().float() == SENT).all()), (what, "dx")


def dropout_case(dev, n, p, dtype, seeds=DROPOUT_SEEDS):
    x = _dropout_x(n, dtype, n)
    for seed in seeds:
        rc, y, mask = _dropout_call(dev, x, p, seed, entry="up_dropout_fwd_t")
        assert rc == 0, _C.lib().up_last_error()
        keep = keep_mask(seed, n, p)
        if p == 0.0:
            assert bool(keep.all())
        _dropout_judge(dev, x, p, keep, y, mask, (n, p, dtype, hex(seed)))


def dropout_threshold_case(dev, dtype):
    """p equal to one element's own h 2^-24 (exact in float32): `>= p` keeps that element"""
    n, seed = 1031, 0x5EED
    h = hash24(seed, n)
    k = int(np.nonzero((h >= 2 ** 22) & (h < 3 * 2 ** 22))[0][0])
    p = float(h[k]) * 2.0 ** -24
    keep = keep_mask(seed, n, p)
    assert bool(keep[k]) and 0.25 <= p < 0.75
    x = _dropout_x(n, dtype, 3)
    rc, y, mask = _dropout_call(dev, x, p, seed)
    assert rc == 0 and int(mask[k].item()) == 1
    _dropout_judge(dev, x, p, keep, y, mask, ("threshold", dtype, k, p))


def dropout_ext_mask_case(dev, dtype):
    """the caller's mask: -0.0 is "not kept" (-0.0 != 0 is false), 2.0 is kept"""
    n = 257
    ext = torch.tensor([0.0, 1.0, -0.0, 2.0, 1.0, 0.0, -0.0])[torch.randint(0, 7, (n,), generator=_gen(6))]
    ext[:4] = torch.tensor([-0.0, 2.0, 0.0, 1.0])
    x = _dropout_x(n, dtype, 4)
    x[0] = 1.5
    rc, y, mask = _dropout_call(dev, x, 0.5, 1, ext=ext.to(dev))
    assert rc == 0
    keep = ext != 0
    assert keep[:4].tolist() == [False, True, False, True]
    _dropout_judge(dev, x, 0.5, keep, y, mask, ("ext", dtype))


def dropout_step_case(dev, dtype):
    """a device counter s: the mask of seed + s * 0x9E3779B97F4A7C15 (mod 2^64); a NULL counter is step 0"""
    n, p = 1031, 0.3
    x = _dropout_x(n, dtype, 5)
    for seed in (0x5EED, MASK64 - 2):
        masks = []
        for s in (None, 0, 1, 5):
            step = None if s is None else torch.tensor([s], dtype=torch.int64).to(dev)
            rc, y, mask = _dropout_call(dev, x, p, seed, step=step)
            assert rc == 0
            keep = keep_mask((seed + (s or 0) * GOLDEN_STEP) & MASK64, n, p)
            _dropout_judge(dev, x, p, keep, y, mask, ("step", s, dtype, hex(seed)))
            masks.append(keep)
        assert torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[2], masks[3])


def dropout_refusal_case(dev):
    """p < 0, p = 1, n = 0, an unknown dtype: UP_ERR_INVALID, y / dx untouched"""
    L = _C.lib()
    x = torch.ones(16).to(dev)
    m = torch.ones(16, dtype=torch.uint8).to(dev)
    for p, n, dt in ((-0.25, 16, 0), (1.0, 16, 0), (0.5, 0, 0), (0.5, 16, 2), (0.5, 16, -1)):
        y = torch.full((16,), SENT).to(dev)
        assert L.up_dropout_fwd_t(x.data_ptr(), y.data_ptr(), m.data_ptr(), None, n, p, 1, dt, ops._stream(x)) == -1, (p, n, dt)
        assert L.up_dropout_fwd_step_t(x.data_ptr(), y.data_ptr(), m.data_ptr(), None, n, p, 1, None, dt, ops._stream(x)) == -1, (p, n, dt)
        assert L.up_dropout_bwd_t(x.data_ptr(), m.data_ptr(), y.data_ptr(), n, p, dt, ops._stream(x)) == -1, (p, n, dt)
        assert bool((y.cpu() == SENT).all()) and bool((m.cpu() == 1).all()), (p, n, dt)


def report():
    return "\n".join("    %-36s %.3f" % kv for kv in sorted(WORST.items()))


if __name__ == "__main__":
    w = host_float32_ratio()
    for k_, v_ in sorted(w.items()):
        print("%-28s %.3f" % (k_, v_))
    top = max(w.values())
    print("worst %.3f -> K_LSTM = %g" % (top, 2.0 ** math.ceil(math.log2(4 * top))))
