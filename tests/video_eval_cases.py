"""The evaluation entries of the video plan (up_clip_nchw_to_nhwc_flip, up_clip_avgpool9s8_flip_fwd, up_clip_heatmap_decode,
up_clip_final_preds; up_unipose_lstm_clip_keypoints / _clip_flip / _clip_final_preds / _stream_keypoints; UniPoseLSTMPlan's
clip_keypoints / clip_flip_heatmaps / clip_final_preds / stream; VideoTrainer with args.flip_test): shared by
test_video_eval_emu.py and test_video_eval_gpu.py.

Every new entry is its existing neighbour with the frame-major order (and the mirror) folded in, so the yardstick is always the
composition of existing entries — which the existing tests pin to the reference — and every comparison is for equal bits or exact
integers.  Nothing here has a tolerance."""
import argparse
import ctypes as C
import functools

import numpy as np
import torch

from oracle import unipose_oracle as O
from unipose_amd import _C, ops, protocol

import lstm_plan_cases as lc
from protocol_cases import SENT, bits_equal, host

F32 = np.float32
PAIRS = [[1, 2], [3, 4]]          # a permutation that really moves channels


def _dev_tensor(dev, shape, alloc=None, fill=SENT, dtype=torch.float32):
    """a tensor of sentinels; alloc(shape): the emulator's allocation that ends right before an inaccessible page"""
    if alloc is not None and dtype == torch.float32:
        t = alloc(tuple(shape))
        t.fill_(fill)
        return t
    return torch.full(tuple(shape), fill, dtype=dtype, device=dev)


def _st(t):
    return ops._stream(t)


# ---- 1. up_clip_nchw_to_nhwc_flip ----------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(bt, hw) for bt in ((1, 1), (2, 3), (3, 2)) for hw in ((3, 1), (2, 7), (5, 65))]


def layout_flip_case(dev, bt, hw, alloc=None):
    L = _C.lib()
    (B, T), (H, W), Cc, ld = bt, hw, 3, 4
    rng = np.random.default_rng(100 * B + 10 * T + W)
    x = torch.from_numpy(rng.standard_normal((B, T, Cc, H, W)).astype(F32)).to(dev)
    xf = torch.flip(x, [-1]).contiguous()
    got = _dev_tensor(dev, (T * B, H, W, ld), alloc)
    ref = _dev_tensor(dev, (T * B, H, W, ld))
    _C.check(L.up_clip_nchw_to_nhwc_flip(x.data_ptr(), got.data_ptr(), B, T, Cc, H, W, ld, _st(x)), "clip_nchw_to_nhwc_flip")
    _C.check(L.up_clip_nchw_to_nhwc(xf.data_ptr(), ref.data_ptr(), B, T, Cc, H, W, ld, _st(x)), "clip_nchw_to_nhwc")
    g = host(got)
    assert bits_equal(g, host(ref)), (bt, hw)
    assert (g[..., Cc:] == 0).all()                                           # pad lanes are written as zeros
    # the definition itself: y[t * B + b, h, w, c] = x[b, t, c, h, W - 1 - w]
    want = host(x).transpose(1, 0, 3, 4, 2).reshape(T * B, H, W, Cc)[:, :, ::-1]
    assert np.array_equal(g[..., :Cc], want)


# ---- 2. up_clip_avgpool9s8_flip_fwd ----------------------------------------------------------------------------------------------------
POOL_CASES = [(bt, hw, coff) for bt in ((1, 2), (2, 3)) for hw in ((7, 7), (8, 16), (15, 23), (16, 24)) for coff in (14, 15)]
POOL_SEED = 7


def _pool_restated(m, stored_order):
    """AvgPool2d(9, 8, 1) of the planes m (N, H, W), the kernel's arithmetic in numpy float32: the window and the divisor of
    avgpool9s8_at, one float32 add per element, rows ascending; columns ascending (the kernel's order on the plane it is given)
    or, stored_order, descending — the order in which a kernel that walked the STORED map of a mirrored plane would add."""
    N, H, W = m.shape
    P, Q = (H - 7) // 8 + 1, (W - 7) // 8 + 1
    out = np.zeros((N, P, Q), F32)
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                hs, ws = p * 8 - 1, q * 8 - 1
                he, we = min(hs + 9, H + 1), min(ws + 9, W + 1)
                div = F32((he - hs) * (we - ws))
                hs, ws, he, we = max(hs, 0), max(ws, 0), min(he, H), min(we, W)
                s = F32(0)
                cols = range(we - 1, ws - 1, -1) if stored_order else range(ws, we)
                for h in range(hs, he):
                    for w in cols:
                        s = F32(s + m[n, h, w])
                out[n, p, q] = s / div
    return out


def pool_input(bt, hw):
    (B, T), (H, W) = bt, hw
    rng = np.random.default_rng(POOL_SEED + 1000 * B + 100 * T + H * W)
    return (rng.standard_normal((B, T, 1, H, W)) * 10.0 ** rng.integers(-3, 4, (B, T, 1, H, W))).astype(F32)


def pool_order_matters(bt, hw):
    """the mirrored planes pooled in the kernel's order and in the un-mirrored (stored) order: the two must differ somewhere, or
    the case could not tell a wrong summation order from the right one"""
    (B, T), (H, W) = bt, hw
    m = pool_input(bt, hw)[:, :, 0, :, ::-1].reshape(B * T, H, W)
    right, wrong = _pool_restated(m, False), _pool_restated(m, True)
    assert (right.view(np.int32) != wrong.view(np.int32)).any(), (bt, hw)
    return right


def pool_flip_case(dev, bt, hw, coff):
    L = _C.lib()
    (B, T), (H, W), ld = bt, hw, 16
    P, Q = (H - 7) // 8 + 1, (W - 7) // 8 + 1
    restated = pool_order_matters(bt, hw)                                    # batch-major (B * T, P, Q)
    cm = torch.from_numpy(pool_input(bt, hw)).to(dev)
    cmf = torch.flip(cm, [-1]).contiguous()
    got = _dev_tensor(dev, (T * B, P, Q, ld))
    ref = _dev_tensor(dev, (T * B, P, Q, ld))
    _C.check(L.up_clip_avgpool9s8_flip_fwd(cm.data_ptr(), got.data_ptr(), ld, coff, B, T, H, W, P, Q, _st(cm)), "clip_avgpool_flip")
    _C.check(L.up_clip_avgpool9s8_fwd(cmf.data_ptr(), ref.data_ptr(), ld, coff, B, T, H, W, P, Q, _st(cm)), "clip_avgpool")
    g, r = host(got), host(ref)
    assert bits_equal(g, r), (bt, hw, coff)
    keep = np.arange(ld) != coff
    assert (g[..., keep] == SENT).all()                                       # no other channel is touched
    # ... and the expected bits are the restatement's (frame-major rows from the batch-major ones)
    fm = restated.reshape(B, T, P, Q).transpose(1, 0, 2, 3).reshape(T * B, P, Q)
    assert bits_equal(r[..., coff], fm), (bt, hw, coff)


# ---- 3. up_clip_heatmap_decode / up_clip_final_preds ---------------------------------------------------------------------------------
DECODE_CASES = [(bt, layout) for bt in ((2, 3), (1, 4), (3, 1)) for layout in ("nhwc", "nchw")]
J, MH, MW = 3, 5, 7


def clip_maps(bt):
    """frame-major maps (T * B, J, 5, 7): every (b, t, j) map has its own distinct peak; a NaN, a tie and an all-negative map sit in
    three different (b, t)"""
    B, T = bt
    rng = np.random.default_rng(31 * B + T)
    hm = rng.standard_normal((T * B, J, MH, MW)).astype(F32)
    for f in range(T * B):
        for j in range(J):
            hm[f, j].reshape(-1)[(f * J + j) * 2 % (MH * MW)] = 5.0 + f + 0.25 * j
    n = T * B
    f_nan, f_tie, f_neg = 0, n // 2 if n > 2 else 1, n - 1
    assert len({f_nan, f_tie, f_neg}) == 3
    hm[f_nan, 1, 2, 3] = np.nan
    hm[f_tie, 0].reshape(-1)[[4, 30]] = 40.0
    hm[f_neg, 2] = -np.abs(hm[f_neg, 2]) - 1
    return hm


def _batch_major(a, B, T):
    """frame-major rows (T * B, ...) -> batch-major (B * T, ...)"""
    return np.ascontiguousarray(a.reshape((T, B) + a.shape[1:]).swapaxes(0, 1).reshape((B * T,) + a.shape[1:]))


def _layout(hm, layout, dev, alloc=None):
    n, j, h, w = hm.shape
    t = torch.from_numpy(np.ascontiguousarray(hm))
    if layout == "nhwc":
        ld = 4
        x = torch.full((n, h, w, ld), float("nan"))
        x[..., :j] = t.permute(0, 2, 3, 1)
        t, strides = x, (h * w * ld, 1, ld)
    else:
        strides = (j * h * w, h * w, 1)
    if alloc is not None:
        g = alloc(tuple(t.shape))
        g.copy_(t)
        t = g
    return t.to(dev), strides


def clip_decode_case(dev, bt, layout, alloc=None):
    L = _C.lib()
    B, T = bt
    hm = clip_maps(bt)
    fm, s = _layout(hm, layout, dev, alloc)
    bm, _ = _layout(_batch_major(hm, B, T), layout, dev, alloc)
    for size in ((MH, MW), (8 * MH, 8 * MW)):
        for with_idx in (True, False):
            got = [torch.full((B, T, J), -7, dtype=torch.int32, device=dev), _dev_tensor(dev, (B, T, J, 2)), _dev_tensor(dev, (B, T, J))]
            ref = [torch.full((B * T, J), -7, dtype=torch.int32, device=dev), _dev_tensor(dev, (B * T, J, 2)), _dev_tensor(dev, (B * T, J))]
            _C.check(L.up_clip_heatmap_decode(fm.data_ptr(), *s, B, T, J, MH, MW, *size, got[0].data_ptr() if with_idx else None,
                                              got[1].data_ptr(), got[2].data_ptr(), _st(fm)), "clip_heatmap_decode")
            _C.check(L.up_heatmap_decode(bm.data_ptr(), *s, B * T, J, MH, MW, *size, ref[0].data_ptr(), ref[1].data_ptr(),
                                         ref[2].data_ptr(), _st(fm)), "heatmap_decode")
            if with_idx:
                assert np.array_equal(host(got[0]).reshape(B * T, J), host(ref[0])), (bt, layout, size)
                assert len(set(host(got[0]).reshape(-1).tolist())) > 1
            else:
                assert (host(got[0]) == -7).all()                              # idx == NULL: nothing written
            assert bits_equal(host(got[1]).reshape(B * T, J, 2), host(ref[1])), (bt, layout, size)
            assert bits_equal(host(got[2]).reshape(B * T, J), host(ref[2])), (bt, layout, size)
    if T == 1:                                                                 # T == 1 is up_heatmap_decode itself
        assert bits_equal(hm, _batch_major(hm, B, T))


def clip_final_case(dev, bt, layout, alloc=None):
    L = _C.lib()
    B, T = bt
    hm = clip_maps(bt)
    fm, s = _layout(hm, layout, dev, alloc)
    bm, _ = _layout(_batch_major(hm, B, T), layout, dev, alloc)
    rng = np.random.default_rng(B + 7 * T)
    inv = torch.from_numpy(rng.uniform(-3, 3, (B, T, 2, 3))).to(dev)          # batch-major, one crop per frame
    for use_inv in (True, False):
        for use_coords in (True, False):
            got = [_dev_tensor(dev, (B, T, J, 2)), _dev_tensor(dev, (B, T, J, 2)), _dev_tensor(dev, (B, T, J))]
            ref = [_dev_tensor(dev, (B * T, J, 2)), _dev_tensor(dev, (B * T, J, 2)), _dev_tensor(dev, (B * T, J))]
            _C.check(L.up_clip_final_preds(fm.data_ptr(), *s, B, T, J, MH, MW, MW, MH, inv.data_ptr() if use_inv else None,
                                           got[0].data_ptr(), got[1].data_ptr() if use_coords else None, got[2].data_ptr(), _st(fm)),
                     "clip_final_preds")
            _C.check(L.up_final_preds(bm.data_ptr(), *s, B * T, J, MH, MW, MW, MH, inv.data_ptr() if use_inv else None,
                                      ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), _st(fm)), "final_preds")
            assert bits_equal(host(got[0]).reshape(B * T, J, 2), host(ref[0])), (bt, layout, use_inv)
            assert bits_equal(host(got[2]).reshape(B * T, J), host(ref[2])), (bt, layout, use_inv)
            if use_coords:
                assert bits_equal(host(got[1]).reshape(B * T, J, 2), host(ref[1])), (bt, layout, use_inv)
            else:
                assert (host(got[1]) == SENT).all()
            if use_inv and B * T > 1:                                          # the crops differ, so a wrong inv row would show
                assert not bits_equal(host(got[0]), host(got[1])) or not use_coords


# ---- 4. refusals of the kernels: non-zero, nothing written -------------------------------------------------------------------------
def kernel_refusal_case(dev):
    L = _C.lib()
    buf = torch.full((1 << 14,), SENT).to(dev)
    out = torch.full((1 << 12,), SENT).to(dev)
    p, q = buf.data_ptr(), out.data_ptr()

    def refused(fn, names, ok, bads):
        assert fn(*ok) == 0, fn
        out.fill_(SENT)
        for bad in bads:
            a = dict(zip(names, ok))
            a.update(bad)
            assert fn(*[a[n] for n in names]) != 0, bad
        assert (host(out) == SENT).all()
    refused(L.up_clip_nchw_to_nhwc_flip, ("x", "y", "B", "T", "C", "H", "W", "ld", "st"), (p, q, 2, 2, 3, 2, 3, 4, 0),
            (dict(x=None), dict(y=None), dict(B=0), dict(T=0), dict(C=0), dict(H=0), dict(W=-1), dict(ld=2), dict(ld=6), dict(y=q + 4)))
    refused(L.up_clip_avgpool9s8_flip_fwd, ("x", "y", "ld", "coff", "B", "T", "H", "W", "P", "Q", "st"), (p, q, 4, 3, 2, 2, 8, 16, 1, 2, 0),
            (dict(x=None), dict(y=None), dict(ld=0), dict(coff=-1), dict(coff=4), dict(B=0), dict(T=0), dict(H=0), dict(W=0), dict(P=2),
             dict(Q=1)))
    refused(L.up_clip_heatmap_decode, ("hm", "sb", "sj", "sp", "B", "T", "J", "H", "W", "P", "Q", "idx", "preds", "mx", "st"),
            (p, 64, 16, 1, 2, 2, 4, 4, 4, 8, 8, None, q, q + 1024, 0),
            (dict(hm=None), dict(preds=None), dict(mx=None), dict(B=0), dict(T=0), dict(J=0), dict(H=0), dict(W=0), dict(sb=0), dict(sj=-1),
             dict(sp=0), dict(P=3), dict(Q=3), dict(P=1 << 16, Q=1 << 16), dict(sb=1 << 31), dict(sb=1 << 30, B=2, T=2),
             dict(B=1 << 16, T=1 << 16)))
    refused(L.up_clip_final_preds, ("hm", "sb", "sj", "sp", "B", "T", "J", "H", "W", "r0", "r1", "inv", "preds", "co", "mx", "st"),
            (p, 64, 16, 1, 2, 2, 4, 4, 4, 4, 4, None, q, None, q + 1024, 0),
            (dict(hm=None), dict(preds=None), dict(mx=None), dict(B=0), dict(T=-1), dict(J=0), dict(H=0), dict(W=0), dict(sb=0), dict(sj=0),
             dict(sp=-1), dict(r0=0), dict(r1=-3), dict(sb=1 << 30, B=2, T=2), dict(B=1 << 16, T=1 << 16), dict(H=1 << 16, W=1 << 16)))


# ---- 5. the plan programs --------------------------------------------------------------------------------------------------------------
class PlanCtx:
    """One plan, its inputs and the results of the parent commit's entries (clip on the clip and on the mirrored clip, step frame
    by frame): computed once per configuration and shared, unchanged, by the tests."""

    def __init__(self, dev, K, B, T, H, W, output_stride):
        from unipose_amd.plan import UniPoseLSTMPlan
        self.dev, self.K, self.B, self.T, self.H, self.W = dev, K, B, T, H, W
        if output_stride == 16:
            m = lc.lstm_model(dev, K)
        else:
            m = lc.mc.skeleton("lstm", K, output_stride=output_stride)
            m.load_state_dict(O.synth_state_dict(K, 4, lstm=True))
            m = m.to(dev).eval()
        self.x = O.synth_input((B, T + 1, 3, H, W), 15).to(dev)
        self.cm = O.synth_input((B, T + 1, 1, H, W), 16, "rand").to(dev)
        self.xc, self.cmc = self.x[:, :T].contiguous(), self.cm[:, :T].contiguous()
        self.plan = plan = UniPoseLSTMPlan(m, B, H, W, frames=T)
        self.h, self.w = plan.out_height, plan.out_width
        self.ws0 = _C.lib().up_unipose_lstm_plan_workspace(plan._plan)
        self.heats, self.cell, self.hide = plan.clip(self.xc, self.cmc)
        self.heats_f = plan.clip(torch.flip(self.xc, [-1]), torch.flip(self.cmc, [-1]))[0]
        self.perm = protocol.flip_perm(None, K, False, PAIRS)
        self.merged = ops.flip_merge(self.heats.flatten(0, 1), self.heats_f.flatten(0, 1), self.perm)      # (B * T, K + 1, h, w)
        self.steps = []
        prev = None
        for j in range(T + 1):
            heat, cell, hide = plan.step(self.x[:, j], self.cm[:, j], prev)
            prev = (hide, cell)
            self.steps.append(heat)


@functools.lru_cache(maxsize=None)
def ctx(dev, K=13, B=1, T=2, H=32, W=32, output_stride=16):
    return PlanCtx(dev, K, B, T, H, W, output_stride)


def _same(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bits_equal(host(got), host(ref)), what


def plan_keypoints_case(c):
    B, T, K = c.B, c.T, c.K
    for full, size in ((False, None), (True, (c.H, c.W))):
        preds, mx, idx = ops.heatmap_decode(c.heats.flatten(0, 1), size)
        got = c.plan.clip_keypoints(c.xc, c.cmc, full_resolution=full)
        _same(got[0], preds.reshape(B, T, K + 1, 2), ("preds", full))
        _same(got[1], mx.reshape(B, T, K + 1, 1), ("maxvals", full))
        assert torch.equal(got[2].cpu(), idx.reshape(B, T, K + 1).cpu()), ("idx", full)
        _same(got[3], c.cell, "cell")
        _same(got[4], c.hide, "hide")
    own = tuple(torch.empty_like(t) for t in got)
    again = c.plan.clip_keypoints(c.xc, c.cmc, full_resolution=True, out=own)
    assert all(a is o for a, o in zip(again, own))
    for a, g in zip(again, got):
        _same(a, g, "out=")
    # idx, cell_last and hide_last may be NULL
    L = _C.lib()
    p2, m2 = torch.empty_like(got[0]), torch.empty_like(got[1])
    ws, nbytes = c.plan._ws()
    _C.check(L.up_unipose_lstm_clip_keypoints(c.plan._plan, c.xc.data_ptr(), c.cmc.data_ptr(), c.H, c.W, None, p2.data_ptr(),
                                              m2.data_ptr(), None, None, ws, nbytes, c.plan._stream()), "clip_keypoints")
    _same(p2, got[0], "idx == NULL")
    _same(m2, got[1], "idx == NULL")
    assert L.up_unipose_lstm_clip_keypoints(c.plan._plan, c.xc.data_ptr(), c.cmc.data_ptr(), c.H - 1, c.W, None, p2.data_ptr(),
                                            m2.data_ptr(), None, None, ws, nbytes, c.plan._stream()) == -1      # another grid
    assert b"grid" in L.up_last_error()


def plan_flip_case(c):
    B, T, K = c.B, c.T, c.K
    assert not bits_equal(host(c.merged), host(c.heats.flatten(0, 1)))
    got = c.plan.clip_flip_heatmaps(c.xc, c.cmc, pairs=PAIRS)
    _same(got, c.merged.reshape(B, T, K + 1, c.h, c.w), "clip_flip_heatmaps")
    # the permutation matters: the identity gives other maps
    other = c.plan.clip_flip_heatmaps(c.xc, c.cmc, pairs=[], out=torch.empty_like(got))
    _same(other, ops.flip_merge(c.heats.flatten(0, 1), c.heats_f.flatten(0, 1), list(range(K + 1))).reshape(got.shape), "identity perm")
    assert not bits_equal(host(other), host(got))


def plan_final_case(c):
    B, T, K = c.B, c.T, c.K
    rng = np.random.default_rng(3)
    center = rng.uniform(40, 120, (B, T, 2))
    scale = rng.uniform(0.5, 1.5, (B, T))
    scale_t = torch.from_numpy(scale.astype(F32))                               # a float32 tensor keeps the reference's float32 arithmetic
    for flip in (False, True):
        maps = c.merged if flip else c.heats.flatten(0, 1)
        for cen, sc in ((center, scale), (torch.from_numpy(center), scale_t), (None, None)):
            flat = (None, None) if cen is None else (cen.reshape(B * T, 2), sc.reshape(B * T))
            ref = ops.final_preds(maps, flat[0], flat[1], return_coords=True)
            got = c.plan.clip_final_preds(c.xc, c.cmc, cen, sc, flip=flip, pairs=PAIRS if flip else None)
            for g, r, n in zip(got, ref, ("preds", "coords", "maxvals")):
                _same(g, r.reshape(g.shape), (n, flip, cen is None))
            if cen is None:
                _same(got[0], got[1], "center=None: preds = coords")
    # coords_xy may be NULL
    L = _C.lib()
    p2, m2 = torch.empty_like(got[0]), torch.empty_like(got[2])
    ws, nbytes = c.plan._flip_ws()
    _C.check(L.up_unipose_lstm_clip_final_preds(c.plan._plan, c.xc.data_ptr(), c.cmc.data_ptr(), ops._perm_array(c.perm, K + 1), None,
                                                c.w, c.h, p2.data_ptr(), None, m2.data_ptr(), ws, nbytes, c.plan._stream()),
             "clip_final_preds")
    _same(p2, got[0], "coords == NULL")
    _same(m2, got[2], "coords == NULL")


def _decoded(heat, size):
    return ops.heatmap_decode(heat, size)


def plan_stream_case(c):
    B, T, K, plan = c.B, c.T, c.K, c.plan
    state = plan.stream_state()
    assert state.dtype == torch.uint8 and state.numel() == _C.lib().up_unipose_lstm_plan_state_bytes(plan._plan) and \
        state.data_ptr() % 256 == 0 and not state.any()
    runs = {}
    for full, size in ((False, None), (True, (c.H, c.W))):
        out = []
        for j in range(T + 1):
            heat = torch.empty((B, K + 1, c.h, c.w), device=c.dev) if j % 2 == 0 else None
            got = plan.stream(c.x[:, j], c.cm[:, j], state, first=j == 0, full_resolution=full, heat=heat)
            ref = _decoded(c.steps[j], size)
            for g, r, n in zip(got, ref, ("preds", "maxvals", "idx")):
                _same(g, r, (n, j, full))
            if heat is not None:
                _same(heat, c.steps[j], ("heat", j))
            out.append(got)
        runs[full] = out
    # first=True on a used buffer equals a fresh buffer (the second run above started on the first one's state); and two
    # interleaved streams on one plan, each with its own buffer and its own inputs, equal their own sequential runs
    xb, cmb = torch.flip(c.x, [1]).contiguous(), torch.flip(c.cm, [1]).contiguous()          # the frames in reverse order
    sb = plan.stream_state()
    seq_b = [plan.stream(xb[:, j], cmb[:, j], sb, first=j == 0) for j in range(T + 1)]
    assert not bits_equal(host(seq_b[-1][1]), host(runs[False][-1][1]))
    sa, sb = plan.stream_state(), plan.stream_state()
    for j in range(T + 1):
        ga = plan.stream(c.x[:, j], c.cm[:, j], sa, first=j == 0)
        gb = plan.stream(xb[:, j], cmb[:, j], sb, first=j == 0)
        for g, r in zip(ga, runs[False][j]):
            _same(g, r, ("stream a", j))
        for g, r in zip(gb, seq_b[j]):
            _same(g, r, ("stream b", j))


def plan_workspace_case(c):
    """clip in exactly up_unipose_lstm_plan_workspace() bytes, the flip programs refused there, the numbers of the queries"""
    L = _C.lib()
    B, T, K, plan = c.B, c.T, c.K, c.plan
    need = [L.up_unipose_lstm_plan_program_workspace(plan._plan, k) for k in range(9)]
    assert all(n > 0 for n in need)
    assert L.up_unipose_lstm_plan_program_workspace(plan._plan, -1) == 0 and L.up_unipose_lstm_plan_program_workspace(plan._plan, 9) == 0
    assert L.up_unipose_lstm_plan_workspace(plan._plan) == c.ws0 == max(need[k] for k in (0, 1, 2, 3, 6, 7, 8))
    flip_need = L.up_unipose_lstm_plan_flip_workspace(plan._plan)
    assert flip_need == max(need[4], need[5]) >= c.ws0
    assert c.ws0 == max(need[:3])                                              # what it was with step and clip alone
    buf = torch.empty(c.ws0 + 256, dtype=torch.uint8, device=c.dev)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    heat = torch.empty_like(c.heats)
    _C.check(L.up_unipose_lstm_clip(plan._plan, c.xc.data_ptr(), c.cmc.data_ptr(), heat.data_ptr(), None, None, ws, c.ws0,
                                    plan._stream()), "unipose_lstm_clip")
    _same(heat, c.heats, "clip in exactly workspace() bytes")
    # a flip program is refused with less than its own need: with workspace() bytes wherever it needs more than that (the
    # first pass's heat-maps outlive the second pass; where the planner finds them a hole between the live tensors of the second
    # pass the two sizes are equal — K = 13 here — and where it does not — K = 15, the widened hand-over — the flip need is larger),
    # and always with one 256-byte unit less than its need
    perm = ops._perm_array(c.perm, K + 1)
    sent = torch.full_like(c.heats, SENT)
    p2 = torch.full((B, T, K + 1, 2), SENT, device=c.dev)
    m2 = torch.full((B, T, K + 1), SENT, device=c.dev)
    for k, short in ((4, c.ws0), (4, need[4] - 256), (5, c.ws0), (5, need[5] - 256)):
        if short >= need[k]:
            continue
        if k == 4:
            e = L.up_unipose_lstm_clip_flip(plan._plan, c.xc.data_ptr(), c.cmc.data_ptr(), perm, sent.data_ptr(), ws, short, plan._stream())
        else:
            e = L.up_unipose_lstm_clip_final_preds(plan._plan, c.xc.data_ptr(), c.cmc.data_ptr(), perm, None, c.w, c.h, p2.data_ptr(),
                                                   None, m2.data_ptr(), ws, short, plan._stream())
        assert e != 0 and b"workspace" in L.up_last_error(), (k, short)
    # the other refusals, all before any launch: a perm entry, res, null pointers, the state buffer
    big = 1 << 40
    bad_perm = ops._perm_array([K + 1] + list(range(1, K + 1)), K + 1)
    x, cm = c.xc.data_ptr(), c.cmc.data_ptr()
    st = plan.stream_state()
    calls = (
        lambda: L.up_unipose_lstm_clip_flip(plan._plan, x, cm, bad_perm, sent.data_ptr(), ws, big, 0),
        lambda: L.up_unipose_lstm_clip_flip(plan._plan, x, cm, None, sent.data_ptr(), ws, big, 0),
        lambda: L.up_unipose_lstm_clip_flip(plan._plan, x, cm, perm, None, ws, big, 0),
        lambda: L.up_unipose_lstm_clip_final_preds(plan._plan, x, cm, bad_perm, None, c.w, c.h, p2.data_ptr(), None, m2.data_ptr(), ws, big, 0),
        lambda: L.up_unipose_lstm_clip_final_preds(plan._plan, x, cm, None, None, 0, c.h, p2.data_ptr(), None, m2.data_ptr(), ws, big, 0),
        lambda: L.up_unipose_lstm_clip_final_preds(plan._plan, x, cm, None, None, c.w, c.h, None, None, m2.data_ptr(), ws, big, 0),
        lambda: L.up_unipose_lstm_clip_keypoints(plan._plan, x, None, c.h, c.w, None, p2.data_ptr(), m2.data_ptr(), None, None, ws, big, 0),
        lambda: L.up_unipose_lstm_clip_keypoints(plan._plan, x, cm, c.h, c.w, None, p2.data_ptr(), m2.data_ptr(), None, None, ws, 256, 0),
        lambda: L.up_unipose_lstm_stream_keypoints(plan._plan, x, cm, None, 1, c.h, c.w, None, p2.data_ptr(), m2.data_ptr(), None, ws, big, 0),
        lambda: L.up_unipose_lstm_stream_keypoints(plan._plan, x, cm, st.data_ptr() + 64, 1, c.h, c.w, None, p2.data_ptr(), m2.data_ptr(),
                                                   None, ws, big, 0),
        lambda: L.up_unipose_lstm_stream_keypoints(plan._plan, x, cm, st.data_ptr(), 1, c.h, c.w + 1, None, p2.data_ptr(), m2.data_ptr(),
                                                   None, ws, big, 0),
        lambda: L.up_unipose_lstm_stream_keypoints(plan._plan, x, cm, st.data_ptr(), 0, c.h, c.w, None, None, m2.data_ptr(), None, ws, big, 0),
    )
    for i, call in enumerate(calls):
        assert call() != 0, i
    assert (host(sent) == SENT).all() and (host(p2) == SENT).all() and (host(m2) == SENT).all() and not st.any()


def plan_unset_case(dev):
    """an evaluation entry of a plan whose weights were never set: refused ("never set")"""
    from unipose_amd.plan import _LstmConfig
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(1, 2, 32, 32, 16, 13)), C.byref(plan)) == 0
    buf = torch.zeros(1 << 16).to(dev)
    p = buf.data_ptr() + (-buf.data_ptr()) % 256
    perm = ops._perm_array(list(range(14)), 14)
    big = 1 << 40
    assert L.up_unipose_lstm_plan_state_bytes(plan) == 2 * 4 * 4 * 16 * 4
    for call in (lambda: L.up_unipose_lstm_clip_keypoints(plan, p, p, 4, 4, None, p, p, None, None, p, big, 0),
                 lambda: L.up_unipose_lstm_clip_flip(plan, p, p, perm, p, p, big, 0),
                 lambda: L.up_unipose_lstm_clip_final_preds(plan, p, p, perm, None, 4, 4, p, None, p, p, big, 0),
                 lambda: L.up_unipose_lstm_clip_final_preds(plan, p, p, None, None, 4, 4, p, None, p, p, big, 0),
                 lambda: L.up_unipose_lstm_stream_keypoints(plan, p, p, p, 1, 4, 4, None, p, p, None, p, big, 0)):
        assert call() != 0
        assert b"never set" in L.up_last_error()
    L.up_unipose_lstm_plan_destroy(plan)
    assert L.up_unipose_lstm_plan_state_bytes(None) == 0 and L.up_unipose_lstm_plan_flip_workspace(None) == 0


def plan_argument_case(c):
    """argument checks of the new methods: ValueError before any launch"""
    B, T, K, H, W, h, w, dev, plan = c.B, c.T, c.K, c.H, c.W, c.h, c.w, c.dev, c.plan
    x, cm = c.xc, c.cmc
    state = plan.stream_state()
    bad_calls = [
        lambda: plan.clip_keypoints(x[:, :1], cm[:, :1]) if T > 1 else plan.clip_keypoints(x.double(), cm),
        lambda: plan.clip_keypoints(x.double(), cm),
        lambda: plan.clip_keypoints(x, cm[..., :W - 8]),
        lambda: plan.clip_keypoints(x, cm, out=(torch.empty(B, T, K + 1, 2, device=dev),) * 3),
        lambda: plan.clip_keypoints(x, cm, out=(torch.empty(B, T, K + 1, 2, device=dev), torch.empty(B, T, K + 1, 1, device=dev),
                                                torch.empty(B, T, K + 1, device=dev), torch.empty(B, K + 2, h, w, device=dev),
                                                torch.empty(B, K + 2, h, w, device=dev))),          # idx is int32
        lambda: plan.clip_flip_heatmaps(x, cm),                                                         # no dataset, no pairs
        lambda: plan.clip_flip_heatmaps(x, cm, dataset="Penn_Action"),                                  # the reference has no list
        lambda: plan.clip_flip_heatmaps(x, cm, pairs=[[0, K]]),
        lambda: plan.clip_flip_heatmaps(x, cm, pairs=PAIRS, out=torch.empty(B, T, K + 1, h, w + 1, device=dev)),
        lambda: plan.clip_flip_heatmaps(x[..., :H - 8, :], cm, pairs=PAIRS),
        lambda: plan.clip_final_preds(x, cm, center=np.zeros((B, 2)), scale=np.ones((B,))),             # one crop per FRAME
        lambda: plan.clip_final_preds(x, cm, center=np.zeros((B, T, 2))),                               # no scale
        lambda: plan.clip_final_preds(x, cm, res=[0, 4]),
        lambda: plan.clip_final_preds(x, cm, flip=True),                                                # no pairs
        lambda: plan.clip_final_preds(x, cm, out=(torch.empty(B, T, K + 1, 2, device=dev),) * 2),
        lambda: plan.stream(x[:, 0], cm[:, 0], None, first=True),
        lambda: plan.stream(x[:, 0], cm[:, 0], state[:-1], first=True),
        lambda: plan.stream(x[:, 0], cm[:, 0], state.float(), first=True),
        lambda: plan.stream(x[:, 0], cm[:, 0, :, :8], state, first=True),
        lambda: plan.stream(x[:, 0].double(), cm[:, 0], state, first=True),
        lambda: plan.stream(x[:, 0], cm[:, 0], state, first=True, heat=torch.empty(B, K + 1, h + 1, w, device=dev)),
    ]
    for i, call in enumerate(bad_calls):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(f"bad call {i} was not refused")
    assert not state.any()


# ---- 6. the trainer --------------------------------------------------------------------------------------------------------------------
def trainer_case(dev):
    from unipose_amd.trainer import PoseMetrics, VideoTrainer
    base = dict(dataset="Penn_Action", pretrained=None, model_name=None, model_arch="unipose", train_dir=None, val_dir=None, batch_size=1,
                size=32, frame_memory=2, train_batches=1, val_batches=1)
    try:
        VideoTrainer(argparse.Namespace(**base, flip_test=True), device=dev)      # the reference has no list for Penn_Action
    except ValueError as e:
        assert "pairs" in str(e)
    else:
        raise AssertionError("flip_test without pairs was not refused")
    torch.manual_seed(3)
    tr = VideoTrainer(argparse.Namespace(**base, flip_test=True, flip_pairs=PAIRS), device=dev)
    seen = []
    real = ops.accuracy

    def spy(output, *a, **k):
        seen.append(output.detach().clone())
        return real(output, *a, **k)
    ops.accuracy = spy
    try:
        m_on = tr.validation(0)
    finally:
        ops.accuracy = real
    assert len(seen) == 2 and m_on.evals == 2
    # by hand: two unrolls, the merge, ops.accuracy
    item = next(iter(tr.val_loader))
    x, hm, cm = tr.batcher(item)
    perm = protocol.flip_perm(None, 13, False, PAIRS)
    tr.model.eval()
    plain, mirrored = [], []
    with torch.no_grad():
        tr._unroll(x, hm, cm, lambda j, heat: plain.append(heat))
        tr._unroll(torch.flip(x, [-1]), hm, torch.flip(cm, [-1]), lambda j, heat: mirrored.append(heat))
    ref = PoseMetrics(13)
    for j in range(2):
        want = ops.flip_merge(plain[j], mirrored[j], perm)
        assert bits_equal(host(seen[j]), host(want)), j
        assert not bits_equal(host(seen[j]), host(plain[j]))
        acc = real(want, hm[:, j], 0.2, 0.5, "Penn_Action")
        ref.update(acc[0], acc[1], acc[2], acc[5], video=True)
    for k in ("AP", "PCK", "PCKh"):
        assert np.array_equal(getattr(m_on, k), getattr(ref, k)), k
    # the driver's flags
    import uniposeLSTM as drv
    a = drv.parse_args(["--flip-test", "--flip-pairs", "1,2;3,4"])
    assert a.flip_test is True and a.flip_pairs == PAIRS
    a = drv.parse_args([])
    assert a.flip_test is False and a.flip_pairs is None
