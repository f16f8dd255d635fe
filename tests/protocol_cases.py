"""The evaluation protocol around the forward (up_nchw_to_nhwc_flip, up_flip_merge, up_final_preds, up_unipose_flip_forward,
up_unipose_final_preds; unipose_amd/protocol.py, ops.flip_merge / final_preds, UniPosePlan.flip_heatmaps / final_preds, Trainer
with args.flip_test): shared by test_protocol_emu.py and test_protocol_gpu.py.

Yardsticks.  The fixture G21 (tools/make_goldens.py g21) holds what the reference's OWN utils/extra_utils computes: get_preds,
final_preds, get_transform and its inverse, flip_back.  `restate` is the entry's documented arithmetic (include/unipose_hip.h) in
numpy, float32 where the kernel is float32 and float64 products and sums in the kernel's order.  Every comparison is bit for bit
or integer-exact; nothing here has a tolerance.  The one exclusion rule (restatement against G21 only): a coordinate whose
transformed value v is within 1e-9 of an integer may be excluded — there numpy's dot inside the reference may round to the other
side of the truncation — unless it belongs to the exact-integer case, where every v is an integer in float64 whatever the order
of the sum; at most 1 % of the coordinates may go that way."""
import ctypes as C
import os

import numpy as np
import torch

from unipose_amd import _C, ops, protocol

F32 = np.float32
SENT = 7.0
MPII16 = ([0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13])


def g21(golden_dir):
    return np.load(os.path.join(golden_dir, "g21_final_preds.npz"))


def tags(g):
    return ["c%d" % k for k in range(len(g["shapes"]))] + ["x"]


def bits_equal(a, b):
    """equal bits; NaNs must sit at the same places (their payload is not compared)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def host(t):
    return t.detach().cpu().numpy()


# ---- the entry's arithmetic in numpy ------------------------------------------------------------------------------------------------
def restate(hm, res, inv=None, refine=True):
    """hm (B,J,H,W) float32 numpy -> preds, coords (B,J,2) float32, maxvals (B,J,1) float32, v (B,J,2) float64 (zeros without inv)"""
    b, j, h, w = hm.shape
    preds, coords = np.zeros((b, j, 2), F32), np.zeros((b, j, 2), F32)
    mx, v = np.zeros((b, j, 1), F32), np.zeros((b, j, 2))
    q = F32(0.25)
    sgn = lambda p, r: F32(int(p > r) - int(p < r))
    for n in range(b):
        for k in range(j):
            m = hm[n, k]
            i = int(np.argmax(m.reshape(-1)))              # the first maximum; a NaN wins (the first NaN)
            top = m.reshape(-1)[i]
            mx[n, k, 0] = top
            x = y = F32(0)
            if top > 0:
                x, y = F32(i % w + 1), F32(i // w + 1)
            px, py = int(x), int(y)
            if refine and 1 < px < res[0] and 1 < py < res[1] and px < w and py < h:
                x = F32(x + q * sgn(m[py - 1][px], m[py - 1][px - 2]))
                y = F32(y + q * sgn(m[py][px - 1], m[py - 2][px - 1]))
            x, y = F32(x + F32(0.5)), F32(y + F32(0.5))
            coords[n, k] = (x, y)
            if inv is None:
                preds[n, k] = (x, y)
                continue
            p0, p1 = np.float64(x) - 1.0, np.float64(y) - 1.0
            for a in range(2):
                r = inv[n][a]
                v[n, k, a] = (r[0] * p0 + r[1] * p1) + r[2]          # numpy float64 scalars: every product and sum rounded
                preds[n, k, a] = F32(int(v[n, k, a]) + 1)            # int(): towards zero
    return preds, coords, mx, v


def kinds(g, tag):
    """the two forms of centre / scale the reference was recorded with"""
    return (("32", torch.from_numpy(g[tag + "_c32"]), torch.from_numpy(g[tag + "_s32"])), ("64", g[tag + "_c64"], g[tag + "_s64"]))


# ---- 1. restatement against G21, no device -----------------------------------------------------------------------------------------
def transform_case(golden_dir):
    g = g21(golden_dir)
    n = 0
    for tag in tags(g):
        for r, res in enumerate(g[tag + "_res"].tolist()):
            for kind, c, s in kinds(g, tag):
                mats = np.stack([protocol.get_transform(c[i], s[i], res) for i in range(len(c))])
                assert mats.dtype == np.float64 and np.array_equal(mats.view(np.int64), g[tag + "_T" + kind][r].view(np.int64)), (tag, res, kind)
                inv = protocol.inverse_maps(c, s, res)
                assert np.array_equal(inv.view(np.int64), np.ascontiguousarray(g[tag + "_Ti" + kind][r][:, :2]).view(np.int64)), (tag, res, kind)
                n += len(c)
    assert n > 100
    # lists are accepted like arrays, an int res like [res, res]
    a = protocol.get_transform([100.0, 120.0], 1.25, 16)
    assert np.array_equal(a, protocol.get_transform(np.array([100.0, 120.0]), np.float64(1.25), [16, 16]))


def restatement_case(golden_dir):
    g = g21(golden_dir)
    total = excluded = 0
    for tag in tags(g):
        hm = g[tag + "_hm"]
        gp = restate(hm, [1, 1], refine=False)[1] - F32(0.5)          # get_preds: no refinement, no + 0.5
        assert bits_equal(gp, g[tag + "_getpreds"]), tag
        for r, res in enumerate(g[tag + "_res"].tolist()):
            if not g[tag + "_ok"][r]:
                continue
            for kind in ("32", "64"):
                inv = g[tag + "_Ti" + kind][r][:, :2]
                preds, _, _, v = restate(hm, res, inv)
                near = np.abs(v - np.round(v)) < 1e-9
                if tag == "x":
                    assert near.all() and np.array_equal(v, np.round(v))       # the exact-integer case: nothing is excluded
                    near[:] = False
                    assert (v < 0).any() and (v > 0).any()                     # truncation, not floor, is what is tested
                want = g[tag + "_fp" + kind][r]
                wrong = (preds != want) & ~near
                assert not wrong.any(), (tag, res, kind, preds[wrong][:4], want[wrong][:4])
                total += near.size
                excluded += int(near.sum())
    print(f"restatement against G21: {total} coordinates, {excluded} excluded")
    assert total >= 1680 and excluded <= 0.01 * total


# ---- 2. up_final_preds ---------------------------------------------------------------------------------------------------------------
def nhwc_copy(hm, ld, fill=float("nan")):
    """NCHW torch maps as a convolution leaves them: NHWC with ld physical channels, the pad channels holding `fill`"""
    b, j, h, w = hm.shape
    x = torch.full((b, h, w, ld), fill, dtype=torch.float32, device=hm.device)
    x[..., :j] = hm.permute(0, 2, 3, 1)
    return x


def run_final(dev, hm, res, inv=None, layout="nchw", coords=True, alloc=None):
    """up_final_preds itself -> (preds, coords or None, maxvals) numpy.  alloc(shape): the emulator's guarded allocation of the maps"""
    b, j, h, w = hm.shape
    t = torch.from_numpy(np.ascontiguousarray(hm))
    if layout == "nhwc":
        ld = (j + 3) // 4 * 4 + 4
        t = nhwc_copy(t, ld)
        strides = (h * w * ld, 1, ld)
    else:
        strides = (j * h * w, h * w, 1)
    if alloc is not None:
        gt = alloc(tuple(t.shape))
        gt.copy_(t)
        t = gt
    t = t.to(dev)
    m = None if inv is None else torch.from_numpy(np.ascontiguousarray(inv, dtype=np.float64)).to(dev)
    preds = torch.full((b, j, 2), SENT, device=dev)
    co = torch.full((b, j, 2), SENT, device=dev) if coords else None
    mx = torch.full((b, j, 1), SENT, device=dev)
    _C.check(_C.lib().up_final_preds(t.data_ptr(), *strides, b, j, h, w, int(res[0]), int(res[1]), None if m is None else m.data_ptr(),
                                     preds.data_ptr(), None if co is None else co.data_ptr(), mx.data_ptr(), ops._stream(t)),
             "final_preds")
    return host(preds), None if co is None else host(co), host(mx)


def same_triple(got, ref, what):
    for a, b, n in zip(got, ref, ("preds", "coords", "maxvals")):
        if a is None:
            continue
        assert bits_equal(a, b), (what, n, a.reshape(-1)[:8], b.reshape(-1)[:8])


def final_golden_case(dev, golden_dir, alloc=None):
    """every G21 case from NCHW and from NHWC (ld > J, NaN in the pad lanes): equal to the restatement, and to the recorded
    final_preds under the restatement's exclusion rule; the IndexError combinations run too and stay inside the map"""
    g = g21(golden_dir)
    raised = {tuple(r) for r in g["index_error"].tolist()}
    ran = 0
    for tag in tags(g):
        hm = g[tag + "_hm"]
        h, w = hm.shape[-2:]
        for r, res in enumerate(g[tag + "_res"].tolist()):
            assert ((h, w, res[0], res[1]) in raised) == (not g[tag + "_ok"][r])
            for kind in ("32", "64"):
                inv = g[tag + "_Ti" + kind][r][:, :2]
                ref = restate(hm, res, inv)
                for layout in ("nchw", "nhwc"):
                    got = run_final(dev, hm, res, inv, layout, alloc=alloc)
                    same_triple(got, ref[:3], (tag, res, kind, layout))
                    if g[tag + "_ok"][r]:
                        near = np.zeros_like(ref[3], dtype=bool) if tag == "x" else np.abs(ref[3] - np.round(ref[3])) < 1e-9
                        assert not ((got[0] != g[tag + "_fp" + kind][r]) & ~near).any(), (tag, res, kind, layout)
                    ran += 1
    assert ran >= 100 and len(raised) >= 3


def final_variants_case(dev, alloc=None):
    rng = np.random.default_rng(5)
    for j in (1, 17, 22):
        hm = rng.standard_normal((2, j, 9, 11)).astype(F32)
        inv = rng.uniform(-3, 3, (2, 2, 3))
        ref = restate(hm, [11, 9], inv)
        for layout in ("nchw", "nhwc"):
            same_triple(run_final(dev, hm, [11, 9], inv, layout, alloc=alloc), ref[:3], (j, layout))
            got = run_final(dev, hm, [11, 9], inv, layout, coords=False, alloc=alloc)          # coords_xy == NULL
            assert got[1] is None and bits_equal(got[0], ref[0]) and bits_equal(got[2], ref[2])
            p, c, _ = run_final(dev, hm, [11, 9], None, layout, alloc=alloc)                   # inv == NULL: preds == coords
            assert bits_equal(p, c) and bits_equal(c, ref[1])
    # the identity of a 1:1 crop: preds = trunc(coords - 1) + 1
    hm = rng.standard_normal((3, 5, 16, 16)).astype(F32)
    inv = protocol.inverse_maps(np.full((3, 2), 8.0), np.full(3, 0.08), [16, 16])
    assert np.array_equal(inv, np.broadcast_to(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (3, 2, 3)))
    p, c, _ = run_final(dev, hm, [16, 16], inv, alloc=alloc)
    assert np.array_equal(p, np.trunc(c - 1) + 1) and (c != np.round(c)).all()
    # without the refinement coords - 0.5 is up_heatmap_argmax's preds + 1 wherever the maximum is positive
    hm[0, 0] = -np.abs(hm[0, 0]) - 1
    _, c, mx = run_final(dev, hm, [1, 1], None, alloc=alloc)
    ap, amx, _ = (host(t) for t in ops.heatmap_argmax(torch.from_numpy(hm).to(dev)))
    pos = mx[..., 0] > 0
    assert pos.sum() == 14 and np.array_equal((c - F32(0.5))[pos], (ap + 1)[pos]) and bits_equal(mx, amx)
    assert np.array_equal(c[~pos], np.full((1, 2), 0.5, F32))
    # ops.final_preds / final_preds_nhwc are the same entry
    t = torch.from_numpy(hm).to(dev)
    cen, sc = np.array([[100.0, 90.0], [50.0, 60.0], [70.0, 75.0]]), np.array([1.0, 0.7, 1.4])
    ref = restate(hm, [16, 16], protocol.inverse_maps(cen, sc, [16, 16]))
    got = ops.final_preds(t, cen, sc, [16, 16], return_coords=True)
    same_triple([host(a) for a in got], ref[:3], "ops.final_preds")
    assert bits_equal(host(ops.final_preds(t, cen, sc, [16, 16])), ref[0])
    got = ops.final_preds_nhwc(nhwc_copy(t, 8), 5, cen, sc, return_coords=True)
    same_triple([host(a) for a in got], ref[:3], "ops.final_preds_nhwc")
    same_triple([host(a) for a in ops.final_preds(t, return_coords=True)], restate(hm, [16, 16])[:3], "ops.final_preds, no centre")


def final_refusal_case(dev):
    L = _C.lib()
    buf = torch.zeros(4096).to(dev)
    p = buf.data_ptr()
    names = ("hm", "sb", "sj", "sp", "B", "J", "H", "W", "res0", "res1", "inv", "preds", "coords", "maxvals", "stream")
    ok = (p, 8 * 64, 64, 1, 1, 8, 8, 8, 8, 8, None, p, None, p, 0)

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_final_preds(*[a[n] for n in names])
    for bad in (dict(hm=None), dict(preds=None), dict(maxvals=None), dict(B=0), dict(J=-1), dict(H=0), dict(W=0), dict(sb=0), dict(sj=0),
                dict(sp=-1), dict(res0=0), dict(res1=-3), dict(H=1 << 16, W=1 << 16), dict(sb=1 << 31, B=2), dict(sp=1 << 26),
                dict(B=1 << 16, J=1 << 16)):
        assert call(**bad) == -1, bad


# ---- 3. up_flip_merge ----------------------------------------------------------------------------------------------------------------
def perm16():
    perm = list(range(16))
    for a, b in MPII16:
        perm[a], perm[b] = b, a
    return perm


def cycle(j):
    perm = list(range(j))
    perm[0], perm[1], perm[2] = 1, 2, 0
    return perm


def merge_ref(a, f, perm):
    with np.errstate(invalid="ignore"):                             # inf + -inf is part of the cases
        return (a + f[:, perm][..., ::-1]) * F32(0.5)


def run_merge(dev, a, f, perm, lin="nchw", lout="nchw", alias=False):
    """up_flip_merge itself; pad lanes of the inputs hold NaN, of the output a sentinel that must survive -> (B,J,H,W) numpy"""
    b, j, h, w = a.shape
    ld = (j + 3) // 4 * 4 + 4
    ta, tf = torch.from_numpy(np.array(a)), torch.from_numpy(np.array(f))           # copies: `out` may be `a`
    if lin == "nhwc":
        ta, tf = nhwc_copy(ta, ld), nhwc_copy(tf, ld)
        si = (h * w * ld, 1, ld)
    else:
        si = (j * h * w, h * w, 1)
    ta, tf = ta.to(dev), tf.to(dev)
    if alias:
        assert lin == lout
        out = ta
        if lin == "nhwc":
            ta[..., j:] = SENT
    elif lout == "nhwc":
        out = torch.full((b, h, w, ld), SENT, device=dev)
    else:
        out = torch.full((b, j, h, w), SENT, device=dev)
    so = (h * w * ld, 1, ld) if lout == "nhwc" else (j * h * w, h * w, 1)
    _C.check(_C.lib().up_flip_merge(ta.data_ptr(), tf.data_ptr(), *si, b, j, h, w, ops._perm_array(perm, j), out.data_ptr(), *so,
                                    ops._stream(out)), "flip_merge")
    o = host(out)
    if lout == "nhwc":
        assert (o[..., j:] == SENT).all(), "a pad lane of `out` was written"
        o = o[..., :j].transpose(0, 3, 1, 2)
    return o


MERGE_SHAPES = [(1, 1, 1, 1), (2, 16, 3, 2), (1, 16, 4, 5), (1, 16, 2, 64), (2, 16, 3, 65), (1, 256, 2, 5), (2, 3, 2, 65), (1, 1, 2, 64)]


def merge_case(dev):
    rng = np.random.default_rng(11)
    n = 0
    for b, j, h, w in MERGE_SHAPES:
        perms = [("identity", list(range(j)))]
        if j == 16:
            perms.append(("mpii", perm16()))
        if j >= 3:
            perms.append(("3-cycle", cycle(j)))
        a, f = rng.standard_normal((b, j, h, w)).astype(F32), rng.standard_normal((b, j, h, w)).astype(F32)
        for name, perm in perms:
            a[0, 0, 0, 0], f[0, perm[0], 0, w - 1] = np.inf, -np.inf              # inf + -inf: a NaN, at the same place
            if a.size > 1:
                a[-1, j - 1, h - 1, w - 1], f[-1, perm[j - 1], h - 1, 0] = np.inf, np.inf
            ref = merge_ref(a, f, perm)
            assert np.isnan(ref[0, 0, 0, 0]) and (a.size == 1 or np.isposinf(ref[-1, j - 1, h - 1, w - 1]))
            for lin in ("nchw", "nhwc"):
                for lout in ("nchw", "nhwc"):
                    assert bits_equal(run_merge(dev, a, f, perm, lin, lout), ref), (b, j, h, w, name, lin, lout)
                    n += 1
                assert bits_equal(run_merge(dev, a, f, perm, lin, lin, alias=True), ref), (b, j, h, w, name, lin, "out is a")
            f[0, perm[0], 0, w - 1] = f[-1, perm[j - 1], h - 1, 0] = 0.5
    assert n >= 60
    # ops.flip_merge, also into `a`
    a, f = torch.from_numpy(a).to(dev), torch.from_numpy(f).to(dev)
    ref = merge_ref(host(a), host(f), [0])
    assert bits_equal(host(ops.flip_merge(a, f, [0])), ref)
    assert ops.flip_merge(a, f, [0], out=a) is a and bits_equal(host(a), ref)


def merge_golden_case(dev, golden_dir):
    """a = 0: out = 0.5 * flip_back(f), exact"""
    g = g21(golden_dir)
    for k in range(2):
        f = g["fb%d_in" % k]
        got = run_merge(dev, np.zeros_like(f), f, perm16())
        assert bits_equal(got, g["fb%d_out" % k] * F32(0.5)), k
        for lin, lout in (("nhwc", "nchw"), ("nhwc", "nhwc")):
            assert bits_equal(run_merge(dev, np.zeros_like(f), f, perm16(), lin, lout), got)


def merge_refusal_case(dev):
    L = _C.lib()
    buf = torch.zeros(1 << 16).to(dev)
    p, q = buf.data_ptr(), buf.data_ptr() + 4 * (1 << 15)
    names = ("a", "f", "isb", "isj", "isp", "B", "J", "H", "W", "perm", "out", "osb", "osj", "osp", "stream")

    def call(J=4, perm_list=None, **kw):
        a = dict(zip(names, (p, q, J * 6, 6, 1, 1, J, 2, 3, ops._perm_array(perm_list if perm_list is not None else list(range(J)), J), p,
                             J * 6, 6, 1, 0)))
        a.update(kw)
        return L.up_flip_merge(*[a[n] for n in names])
    assert call() == 0
    assert call(out=q) == -1 and b"out == f" in L.up_last_error()
    assert call(perm_list=[0, 1, 2, 4]) == -1 and b"perm[3]" in L.up_last_error()
    assert call(perm_list=[0, -1, 2, 3]) == -1
    assert call(J=257) == -2
    assert call(J=256) == 0
    assert call(osb=48, osj=1, osp=8) == -1 and b"out == a" in L.up_last_error()     # out == a with other strides
    for bad in (dict(a=None), dict(f=None), dict(out=None), dict(perm=None), dict(B=0), dict(H=0), dict(W=-1), dict(isb=0), dict(isj=-1),
                dict(isp=0), dict(osb=0), dict(osj=0), dict(osp=-2), dict(isb=1 << 31, B=2), dict(out=q + 4, osp=1 << 30)):
        assert call(**bad) == -1, bad
    assert L.up_flip_merge(p, q, 6, 6, 1, 1, 0, 2, 3, ops._perm_array([0], 1), p, 6, 6, 1, 0) == -1          # J = 0


# ---- 4. up_nchw_to_nhwc_flip -----------------------------------------------------------------------------------------------------------
def layout_flip_case(dev):
    L = _C.lib()
    rng = np.random.default_rng(13)
    for w in (1, 7, 64, 65):
        for c in (1, 3, 4):
            x = torch.from_numpy(rng.standard_normal((2, c, 3, w)).astype(F32)).to(dev)
            ld = 4 if c < 4 else 8
            got, ref = torch.full((2, 3, w, ld), SENT, device=dev), torch.full((2, 3, w, ld), SENT, device=dev)
            xf = torch.flip(x, [3]).contiguous()
            _C.check(L.up_nchw_to_nhwc_flip(x.data_ptr(), got.data_ptr(), 2, c, 3, w, ld, ops._stream(x)), "nchw_to_nhwc_flip")
            _C.check(L.up_nchw_to_nhwc(xf.data_ptr(), ref.data_ptr(), 2, c, 3, w, ld, ops._stream(x)), "nchw_to_nhwc")
            assert bits_equal(host(got), host(ref)), (w, c)
            assert np.array_equal(host(got)[..., :c], host(x).transpose(0, 2, 3, 1)[:, :, ::-1])
    p = got.data_ptr()
    for bad in ((None, p, 1, 3, 2, 2, 4), (p, None, 1, 3, 2, 2, 4), (p, p, 0, 3, 2, 2, 4), (p, p, 1, 0, 2, 2, 4), (p, p, 1, 3, 0, 2, 4),
                (p, p, 1, 3, 2, 0, 4), (p, p, 1, 3, 2, 2, 2)):
        assert L.up_nchw_to_nhwc_flip(*bad, 0) == -1, bad


# ---- 5. the plan -----------------------------------------------------------------------------------------------------------------------
def _model(dev, K, output_stride, bbox, stride=8):
    import heat_decode_cases as hc
    kw = {}
    if output_stride != 16:
        kw["output_stride"] = output_stride
    if bbox:
        kw["bbox"] = True
    if stride != 8:
        kw["stride"] = stride
    return hc.image_model(dev, K, 1, **kw)


def plan_case(dev, K=14, B=1, height=64, width=64, output_stride=16, bbox=False, dataset="LSP", stride=8):
    from oracle import unipose_oracle as O
    from unipose_amd.plan import UniPosePlan
    L = _C.lib()
    m = _model(dev, K, output_stride, bbox, stride)
    x = O.synth_input((B, 3, height, width), 5).to(dev)
    plan = UniPosePlan(m, B, height, width)
    # the workspace the existing programs report is what they alone need; the flip programs have their own figure
    needs = [L.up_unipose_plan_program_workspace(plan._plan, k) for k in range(8)]
    assert needs[7] == 0 and all(n > 0 for n in needs[:7])
    assert L.up_unipose_plan_workspace(plan._plan) == max(needs[:4])
    assert L.up_unipose_plan_flip_workspace(plan._plan) == max(needs[4:7])
    assert min(needs[4], needs[5]) >= needs[0]                     # the forward's tensors and the first pass's heat-maps kept
    assert needs[6] == needs[2]                                    # one pass + a decode that allocates nothing
    maps = lambda t: torch.cat(plan_maps(t), 1) if bbox else plan_maps(t)         # noqa: E731
    if stride == 8:
        plan_maps = plan
    else:                                                          # a stride != 8 model: the flip entries work on the maps' own grid
        m8 = _model(dev, K, output_stride, bbox)
        plan8 = UniPosePlan(m8, B, height, width)
        plan_maps = plan8
    a, f = maps(x), maps(torch.flip(x, [3]).contiguous())
    perm = protocol.flip_perm(dataset, K, bbox)
    assert len(perm) == plan.out_channels
    merged = ops.flip_merge(a, f, perm)
    own = torch.full((B, plan.out_channels, plan.map_height, plan.map_width), SENT, device=dev)
    got = plan.flip_heatmaps(x, dataset, out=own)
    assert got is own
    assert plan.workspace.numel() >= max(needs[:7]) + 256          # grown, where it had to, at the first flip call
    assert got.shape == (B, plan.out_channels, plan.map_height, plan.map_width)
    assert bits_equal(host(got), host(merged))
    if bbox:                                                       # the box channels exchange tl <-> tr and bl <-> br
        fb = K + 1
        assert perm[fb:] == [fb, fb + 3, fb + 4, fb + 1, fb + 2]
        want = 0.5 * (host(a)[:, fb + 1] + host(f)[:, fb + 3][..., ::-1])
        assert bits_equal(host(got)[:, fb + 1], want.astype(F32))
    cen = np.stack([np.array([width / 2.0 + 3 * i, height / 2.0 - 2 * i]) for i in range(B)])
    sc = np.array([max(height, width) / 200.0 * (1 + 0.1 * i) for i in range(B)])
    res = [plan.map_width, plan.map_height]
    for flip, src in ((True, merged), (False, a)):
        ref = ops.final_preds(src, cen, sc, res, return_coords=True)
        got3 = plan.final_preds(x, cen, sc, res, flip=flip, dataset=dataset)
        same_triple([host(t) for t in got3], [host(t) for t in ref], ("plan.final_preds", flip))
    ref = ops.final_preds(a, return_coords=True)
    got3 = plan.final_preds(x)                                     # no centre: heat-map coordinates, res = [W, H]
    same_triple([host(t) for t in got3], [host(t) for t in ref], "plan.final_preds without a centre")
    assert bits_equal(host(got3[0]), host(got3[1]))
    # refusals
    for bad in (dict(dataset="COCO"), dict(pairs=[[0, K]])):
        try:
            plan.flip_heatmaps(x, **({"dataset": dataset} | bad))
            raise AssertionError(f"{bad} must be refused")
        except ValueError:
            pass
    try:
        plan.flip_heatmaps(x, dataset, out=torch.empty((B, plan.out_channels, plan.map_height + 1, plan.map_width), device=dev))
        raise AssertionError("a mis-shaped `out` must be refused")
    except ValueError:
        pass
    p_ = C.c_void_p(x.data_ptr())
    o = got.data_ptr()
    ws = plan.workspace
    off = (-ws.data_ptr()) % 256
    pa = ops._perm_array(perm, len(perm))
    assert L.up_unipose_flip_forward(plan._plan, p_, pa, o, ws.data_ptr() + off, needs[4] - 256, 0) == -1       # too small
    assert b"workspace" in L.up_last_error()
    assert L.up_unipose_final_preds(plan._plan, p_, pa, None, 8, 8, o, None, o, ws.data_ptr() + off, needs[5] - 256, 0) == -1
    badp = ops._perm_array([len(perm)] + perm[1:], len(perm))
    assert L.up_unipose_flip_forward(plan._plan, p_, badp, o, ws.data_ptr() + off, ws.numel() - off, 0) == -1
    assert b"perm[0]" in L.up_last_error()
    assert L.up_unipose_final_preds(plan._plan, p_, None, None, 0, 8, o, None, o, ws.data_ptr() + off, ws.numel() - off, 0) == -1
    assert L.up_unipose_final_preds(plan._plan, p_, None, None, 8, 8, None, None, o, ws.data_ptr() + off, ws.numel() - off, 0) == -1
    plan.close()
    if stride != 8:
        plan8.close()


PLAN_CASES_EMU = [dict(K=14, B=1, height=64, width=64), dict(K=14, B=2, height=52, width=68),
                  dict(K=16, B=2, height=48, width=48, output_stride=8, bbox=True, dataset="MPII"),
                  dict(K=14, B=1, height=64, width=64, stride=1)]
PLAN_CASES_GPU = PLAN_CASES_EMU


def plan_id(case):
    return "-".join(f"{k}{v}" for k, v in case.items())


def plan_unset_case(dev):
    from unipose_amd.plan import _Config
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_plan_create(C.byref(_Config(1, 64, 52, 16, 15)), C.byref(plan)) == 0
    assert L.up_unipose_plan_num_convs(plan) == 116                # the listed convolutions are those of the forward, once
    assert L.up_unipose_plan_flip_workspace(plan) >= L.up_unipose_plan_program_workspace(plan, 0) > 0
    buf = torch.zeros(4096).to(dev)
    p = buf.data_ptr()
    pa = ops._perm_array(list(range(15)), 15)
    assert L.up_unipose_flip_forward(plan, p, pa, p, p, 1 << 40, 0) != 0 and b"never set" in L.up_last_error()
    assert L.up_unipose_final_preds(plan, p, pa, None, 8, 7, p, None, p, p, 1 << 40, 0) != 0 and b"never set" in L.up_last_error()
    assert L.up_unipose_final_preds(plan, p, None, None, 8, 7, p, None, p, p, 1 << 40, 0) != 0 and b"never set" in L.up_last_error()
    assert L.up_unipose_flip_forward(plan, p, None, p, p, 1 << 40, 0) == -1 and b"null" in L.up_last_error()
    L.up_unipose_plan_destroy(plan)


# ---- 6. semantics ----------------------------------------------------------------------------------------------------------------------
def flip_perm_case():
    assert protocol.flip_perm("MPII", 16) == [0, 6, 5, 4, 3, 2, 1, 7, 8, 9, 10, 16, 15, 14, 13, 12, 11]
    lsp = [0, 6, 5, 4, 3, 2, 1, 12, 11, 10, 9, 8, 7, 13, 14]
    assert protocol.flip_perm("LSP", 14) == lsp and protocol.flip_perm("NTID", 14) == lsp
    assert protocol.flip_perm("BBC", 7) == [0, 1, 3, 2, 5, 4, 7, 6]
    assert protocol.flip_perm("LSP", 14, bbox=True) == lsp + [15, 18, 19, 16, 17]
    assert protocol.flip_perm("COCO", 3, pairs=[[0, 2]]) == [0, 3, 2, 1]
    for bad in (lambda: protocol.flip_perm("COCO", 17), lambda: protocol.flip_perm("Penn_Action", 13),
                lambda: protocol.flip_perm("LSP", 5)):
        try:
            bad()
            raise AssertionError("must be refused")
        except ValueError:
            pass


def semantics_case(dev):
    """mirror-image maps with exchanged channels merge to `a` itself; final_preds of a Gaussian target lands on its joint"""
    rng = np.random.default_rng(17)
    perm = protocol.flip_perm("LSP", 14)
    a = rng.standard_normal((2, 15, 6, 9)).astype(F32)
    f = np.empty_like(a)
    f[:, perm] = a[..., ::-1]                                       # f[b, perm[j], y, W-1-x] = a[b, j, y, x]
    got = ops.flip_merge(torch.from_numpy(a).to(dev), torch.from_numpy(f).to(dev), perm)
    assert bits_equal(host(got), a)
    # joints on multiples of the stride: the loaders' Gaussian is centred on int(x) / stride, so the peak is pixel k exactly
    kpt = np.array([[[8.0 * (3 + k), 8.0 * (2 + 2 * k)] for k in range(4)]])
    heat = ops.make_heatmaps(kpt, 128, 128, 8, 3, dev)
    preds, coords, mx = (host(t) for t in ops.final_preds(heat, return_coords=True))
    peak = host(ops.heatmap_argmax(heat)[0])
    assert np.array_equal(coords[0, 1:], peak[0, 1:] + F32(1.5))   # symmetric neighbours: sign 0, the 1-based peak + 0.5
    assert np.array_equal(peak[0, 1:], np.array([[3 + k, 2 + 2 * k] for k in range(4)], dtype=F32))
    # through a crop that is the whole 128 x 128 image on the 16 x 16 maps: back on the joint's pixel, to the 8-pixel cell
    cen, sc = np.array([[64.0, 64.0]]), np.array([128 / 200.0])
    back = host(ops.final_preds(heat, cen, sc, [16, 16]))
    assert np.array_equal(back, restate(host(heat), [16, 16], protocol.inverse_maps(cen, sc, [16, 16]))[0])
    assert (np.abs(back[0, 1:] - kpt[0]) <= 8).all() and (back[0, 1:] >= kpt[0]).all()


# ---- 7. the trainer --------------------------------------------------------------------------------------------------------------------
def trainer_case(dev, bbox=False):
    import argparse
    from unipose_amd.trainer import Trainer
    base = dict(dataset="LSP", pretrained=None, model_name=None, model_arch="unipose", train_dir=None, val_dir=None, batch_size=2, size=32,
                train_batches=1, val_batches=1, bbox=bbox)
    torch.manual_seed(3)
    tr = Trainer(argparse.Namespace(**base, flip_test=True), device=dev)
    off = Trainer(argparse.Namespace(**base), device=dev)          # no such attribute at all: today's arguments
    off.model.load_state_dict(tr.model.state_dict())
    seen = []
    real = ops.accuracy

    def spy(output, *a, **k):
        seen.append(output.detach().clone())
        return real(output, *a, **k)
    ops.accuracy = spy
    try:
        m_on = tr.validation(0)
        m_off = off.validation(0)
    finally:
        ops.accuracy = real
    assert len(seen) == 2 and m_on.evals == 1 and m_off.evals == 1
    item = next(iter(tr.val_loader))
    x = tr.batcher(item)[0]
    tr.model.eval()
    with torch.no_grad():
        a, f = tr.model(x), tr.model(torch.flip(x, [3]))
    perm = protocol.flip_perm("LSP", 14, bbox)
    if bbox:
        want = ops.flip_merge(torch.cat(a, 1), torch.cat(f, 1), perm)[:, :15]
        a = a[0]
    else:
        want = ops.flip_merge(a, f, perm)
    assert bits_equal(host(seen[0]), host(want))                    # the maps handed to ops.accuracy are the merge
    assert bits_equal(host(seen[1]), host(a))                       # flag off: the plain forward's maps, as before
    assert not bits_equal(host(seen[0]), host(a))
    want_off = real(a, tr.batcher(item)[1], 0.2, 0.5, "LSP")
    from unipose_amd.trainer import PoseMetrics
    ref = PoseMetrics(14)
    ref.update(want_off[0], want_off[1], want_off[2], want_off[5])
    for k in ("AP", "PCK", "PCKh"):
        assert np.array_equal(getattr(m_off, k), getattr(ref, k))
