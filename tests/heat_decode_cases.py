"""Key-point output of the inference entries (up_heatmap_decode, up_unipose_forward_upsampled, up_unipose_keypoints;
ops.heatmap_decode, UniPosePlan at stride != 8, UniPosePlan.keypoints): shared by the emulator and the GPU tests.

The decode promises the bits of the composition it replaces (up_bilinear_fwd -> up_nhwc_to_nchw -> up_heatmap_argmax), so every
comparison with the project's own kernels is for EQUAL bits; the genuine reference's full-resolution decode is pinned by the
G17 fixture (tools/make_goldens.py g17)."""
import copy
import ctypes as C
import os

import numpy as np
import torch

from oracle import unipose_oracle as O

import model_cases as mc

LD = 20                                     # physical channels of the NHWC copies (17 maps + 3 pad channels)
SIZES = [((46, 46), (368, 368)), ((7, 7), (52, 52)), ((20, 23), (160, 184))]
BEYOND_LDS = ((112, 113), (224, 230))       # 12656 values > the 12288 the kernel stages in LDS: the global-memory path


def _bits_equal(a, b):
    """equal bits; NaNs must sit at the same places (their payload is not compared)"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])


def same(got, ref, what):
    """(preds, maxvals, idx) triples, bit for bit"""
    for g, r, n in zip(got, ref, ("preds", "maxvals", "idx")):
        assert _bits_equal(g, r), (what, n, g.cpu().reshape(-1)[:8], r.cpu().reshape(-1)[:8])


def nhwc_copy(hm, ld=LD):
    """the maps as a convolution leaves them: NHWC with `ld` physical channels; the pad channels hold a value that would win"""
    b, j, h, w = hm.shape
    x = torch.full((b, h, w, ld), 3.0e38, dtype=torch.float32, device=hm.device)
    x[..., :j] = hm.permute(0, 2, 3, 1)
    return x


def composition(hm, size):
    """what the decode replaces, on the same backend: ToNHWC, up_bilinear_fwd, up_nhwc_to_nchw, up_heatmap_argmax"""
    from unipose_amd import ops
    x = ops.ToNHWC.apply(hm)
    y = ops.Bilinear.apply(x, size[0], size[1])
    return ops.heatmap_argmax(ops.ToNCHW.apply(y, hm.shape[1]))


def both_layouts(hm, size, ref, what):
    from unipose_amd import ops
    same(ops.heatmap_decode(hm, size), ref, what + " from NCHW")
    same(ops.heatmap_decode_nhwc(nhwc_copy(hm), hm.shape[1], size), ref, what + " from NHWC")


# (a) ---------------------------------------------------------------------------------------------------------------------------
def identity_case(dev, golden_dir):
    from unipose_amd import ops
    g6 = torch.from_numpy(np.load(os.path.join(golden_dir, "g6_argmax.npz"))["hm"]).to(dev)     # ties, all-negative, last index
    rnd = torch.randn(4, 17, 46, 46, generator=torch.Generator().manual_seed(3)).to(dev)
    for name, hm in (("g6", g6), ("random", rnd)):
        ref = ops.heatmap_argmax(hm)
        both_layouts(hm, None, ref, name)
        both_layouts(hm, tuple(hm.shape[-2:]), ref, name + " with its own size")


# (b) ---------------------------------------------------------------------------------------------------------------------------
def upsampled_case(dev, maps=(4, 17), maps_beyond_lds=(2, 3)):
    g = torch.Generator().manual_seed(7)
    for (h, w), size in SIZES + [BEYOND_LDS]:
        b, j = maps_beyond_lds if (h, w) == BEYOND_LDS[0] else maps
        hm = torch.randn(b, j, h, w, generator=g).to(dev)
        both_layouts(hm, size, composition(hm, size), f"random {h}x{w} -> {size}")


def planted_case(dev):
    from unipose_amd import ops
    g = torch.Generator().manual_seed(9)
    # 24 -> 47: the scale 23 / 46 is exactly 0.5, every coarse point is a fine point, so the two peaks tie exactly on the fine grid
    hm = torch.zeros(1, 8, 24, 24)
    hm[0, 0, 10, 7] = hm[0, 0, 20, 3] = 2.0                 # two equal peaks: the first one in row-major order wins
    hm[0, 1, 20, 3] = hm[0, 1, 10, 7] = 2.0
    hm[0, 2] = 1.0                                          # constant: (1 - l) + l need not round to 1, near-ties everywhere
    hm[0, 3] = 0.0                                          # every fine value 0: index 0, and max <= 0 zeroes preds
    hm[0, 4] = torch.randn(24, 24, generator=g)
    hm[0, 4, 13, 5] = float("nan")                          # NaN wins; its fine neighbours are NaN too: the first of them
    hm[0, 5] = -torch.randn(24, 24, generator=g).abs() - 0.5      # all negative: preds zeroed, maxvals kept
    hm[0, 6] = torch.randn(24, 24, generator=g)
    hm[0, 6, 23, 23] = 50.0                                 # the maximum at the last index
    hm[0, 7, 0, 0] = 50.0
    hm = hm.to(dev)
    got = ops.heatmap_decode(hm, (47, 47))
    both_layouts(hm, (47, 47), composition(hm, (47, 47)), "planted 24 -> 47")
    preds, mx, idx = (t.cpu() for t in got)
    assert idx[0, 0] == 20 * 47 + 14 and idx[0, 1] == 20 * 47 + 14 and mx[0, 0, 0] == 2.0          # coarse (10, 7) = fine (20, 14)
    assert idx[0, 3] == 0 and preds[0, 3].tolist() == [0.0, 0.0] and mx[0, 3, 0] == 0.0
    assert torch.isnan(mx[0, 4, 0]) and idx[0, 4] == 24 * 47 + 8 and preds[0, 4].tolist() == [0.0, 0.0]   # rows 24..27, columns 8..11
    assert mx[0, 5, 0] < 0 and preds[0, 5].tolist() == [0.0, 0.0]
    assert idx[0, 6] == 47 * 47 - 1 and preds[0, 6].tolist() == [46.0, 46.0] and idx[0, 7] == 0
    # the same maps on a grid whose points are not coarse points (46 -> 368 has scale 45 / 367)
    big = torch.zeros(1, 4, 46, 46)
    big[0, 0, 10, 7] = big[0, 0, 30, 3] = 2.0
    big[0, 1] = 1.0
    big[0, 2] = torch.randn(46, 46, generator=g)
    big[0, 2, 45, 0] = float("nan")
    big[0, 3] = -torch.randn(46, 46, generator=g).abs() - 0.5
    big = big.to(dev)
    both_layouts(big, (368, 368), composition(big, (368, 368)), "planted 46 -> 368")


# (c) ---------------------------------------------------------------------------------------------------------------------------
def reference_case(dev, golden_dir):
    """G17: the reference's own F.interpolate + get_max_preds on its own heat-maps (G1, G10, G5 heat0..3): 103 maps"""
    load = lambda n: np.load(os.path.join(golden_dir, n))
    g17, g5 = load("g17_decode_full_res.npz"), load("g5_lstm_368.npz")
    groups = {"g1": load("g1_eval_368.npz")["out"], "g10": load("g10_eval_736.npz")["out"],
              "g5": np.concatenate([g5[f"heat{j}"].reshape(1, 14, 46, 46) for j in range(4)], 0)}
    from unipose_amd import ops
    maps = 0
    for (name, hm), size in zip(groups.items(), g17["sizes"].tolist()):
        hm = torch.from_numpy(hm).to(dev)
        maps += hm.shape[0] * hm.shape[1]
        for layout, got in (("NCHW", ops.heatmap_decode(hm, (size, size))),
                            ("NHWC", ops.heatmap_decode_nhwc(nhwc_copy(hm), hm.shape[1], (size, size)))):
            preds, mx, idx = (t.cpu().numpy() for t in got)
            rel = np.abs(mx - g17["maxvals_" + name]) / np.abs(g17["maxvals_" + name])
            print(f"g17 {name} {layout}: {int((idx != g17['idx_' + name]).sum())} of {idx.size} indices differ, "
                  f"maxvals rel {rel.max():.2e}")
            assert np.array_equal(idx, g17["idx_" + name]), (name, layout)
            assert np.array_equal(preds, g17["preds_" + name]), (name, layout)
            assert rel.max() < 1e-5, (name, layout, rel.max())
    assert maps == 103


# (d), (e) ------------------------------------------------------------------------------------------------------------------------
def image_model(dev, K=14, wseed=1, **kw):
    bbox = kw.get("bbox", False)
    m = mc.skeleton("image", K, **kw)
    sd = O.synth_state_dict(K, wseed)
    if bbox:        # the box head's five extra output channels have no synthetic entry: keep the constructor's
        own = m.state_dict()
        sd = {k: (v if v.shape == own[k].shape else own[k]) for k, v in sd.items()}
    m.load_state_dict(sd)
    return m.to(dev).eval()


def plan_upsampled_case(dev, K=14, B=1, size=64, wseed=1, xseed=5, output_stride=16, bbox=False):
    """plan_cases.plan_case for a model with stride = 1: the plan returns the maps up-sampled to the input size like the module"""
    from unipose_amd import checkpoint
    from unipose_amd.plan import UniPosePlan
    kw = {"stride": 1}
    if output_stride != 16:
        kw["output_stride"] = output_stride
    if bbox:
        kw["bbox"] = True
    m = image_model(dev, K, wseed, **kw)
    x = O.synth_input((B, 3, size, size), xseed).to(dev)
    plan = UniPosePlan(m, B, size, size)
    got = plan(x)
    folded = checkpoint.load_folded(copy.deepcopy(m), checkpoint.fold_batchnorm(m))
    with torch.no_grad():
        ref = folded(x)
    pairs = list(zip(got, ref)) if bbox else [(got, ref)]
    for g, r in pairs:
        assert g.shape == r.shape and g.shape[-2:] == (size, size)
        assert torch.equal(g.cpu(), r.cpu()), float((g - r).abs().max())
    first = torch.cat(got, 1) if bbox else got
    again = plan(x)
    assert torch.equal((torch.cat(again, 1) if bbox else again).cpu(), first.cpu())
    try:
        plan(x[:, :, :size - 8])
        raise AssertionError("a mis-shaped input must be refused")
    except ValueError:
        pass
    ch, oh = first.shape[1], (size - 1) // 8 + 1
    for bad in (torch.empty((B, ch, size - 1, size), device=dev), torch.empty((B, ch, size, size), device=dev).double(),
                torch.empty((B, ch, size, 2 * size), device=dev)[..., ::2], torch.empty((B, ch, oh, oh), device=dev)):
        try:
            plan(x, out=bad)
            raise AssertionError("a mis-shaped / mis-typed / strided `out` must be refused")
        except ValueError:
            pass
    own = torch.empty((B, ch, size, size), device=dev)
    assert plan(x, out=own) is own or bbox
    # key points at full resolution by default, equal to the argmax of the up-sampled maps
    from unipose_amd import ops
    same(plan.keypoints(x), ops.heatmap_argmax(first), "keypoints of the stride-1 plan")
    plan.close()
    return first


def plan_keypoints_case(dev, K=14, B=1, size=64):
    from unipose_amd import ops
    from unipose_amd.plan import UniPosePlan
    m8 = image_model(dev, K)
    m1 = image_model(dev, K, stride=1)
    x = O.synth_input((B, 3, size, size), 5).to(dev)
    plan8, plan1 = UniPosePlan(m8, B, size, size), UniPosePlan(m1, B, size, size)
    coarse = ops.heatmap_argmax(plan8(x))
    fine = ops.heatmap_argmax(plan1(x))
    assert plan1(x).shape[-2:] == (size, size)
    same(plan8.keypoints(x), coarse, "stride-8 plan, its own grid")
    same(plan8.keypoints(x, full_resolution=True), fine, "stride-8 plan, full resolution")
    same(plan1.keypoints(x), fine, "stride-1 plan, full resolution by default")
    same(plan1.keypoints(x, full_resolution=False), coarse, "stride-1 plan, the maps' own grid")
    same(plan8.keypoints(x, full_resolution=True), fine, "a second call on the same workspace")
    assert not _bits_equal(coarse[2], fine[2])                      # the two grids do differ
    # caller-supplied outputs: used when they fit, refused otherwise
    C_ = K + 1
    good = [torch.empty(B, C_, 2, device=dev), torch.empty(B, C_, 1, device=dev), torch.empty(B, C_, dtype=torch.int32, device=dev)]
    got = plan8.keypoints(x, out=good)
    assert all(g is o for g, o in zip(got, good))
    same(got, coarse, "caller-supplied outputs")
    for slot, bad in ((0, torch.empty(B, C_, 3, device=dev)), (0, torch.empty(B, C_, 2, device=dev).double()),
                      (1, torch.empty(B, C_, 2, device=dev)[..., ::2]), (2, torch.empty(B, C_, device=dev)),
                      (2, torch.empty(B, C_ + 1, dtype=torch.int32, device=dev))):
        out = list(good)
        out[slot] = bad
        try:
            plan8.keypoints(x, out=out)
            raise AssertionError(f"a mis-shaped / mis-typed / strided `out[{slot}]` must be refused")
        except ValueError:
            pass
    try:
        plan8.keypoints(x[:, :, :size - 8])
        raise AssertionError("a mis-shaped input must be refused")
    except ValueError:
        pass
    plan8.close()
    plan1.close()


def keypoints_c_abi_checks(dev):
    """up_unipose_keypoints / up_unipose_forward_upsampled / up_heatmap_decode refuse before anything is launched"""
    from unipose_amd import _C
    from unipose_amd.plan import _Config
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_plan_create(C.byref(_Config(1, 64, 52, 16, 15)), C.byref(plan)) == 0
    ws = L.up_unipose_plan_workspace(plan)
    assert ws >= 64 * 52 * 16 * 4                                   # covers the up-sampled (1, 64, 52, 16) tensor too
    buf = torch.zeros(4096).to(dev)
    p = buf.data_ptr()
    for oh, ow in ((8, 7), (64, 52)):                               # the two legal grids: the weights are what is missing
        assert L.up_unipose_keypoints(plan, p, oh, ow, p, p, p, p, 1 << 40, 0) != 0
        assert b"never set" in L.up_last_error(), L.up_last_error()
    assert L.up_unipose_forward_upsampled(plan, p, p, p, 1 << 40, 0) != 0
    assert b"never set" in L.up_last_error()
    for oh, ow in ((7, 8), (16, 14), (64, 64), (0, 0), (32, 26)):
        assert L.up_unipose_keypoints(plan, p, oh, ow, p, p, p, p, 1 << 40, 0) == -1
        assert b"grid" in L.up_last_error(), L.up_last_error()
    assert L.up_unipose_keypoints(plan, p, 8, 7, None, None, p, p, 1 << 40, 0) == -1
    assert b"null" in L.up_last_error()
    L.up_unipose_plan_destroy(plan)
    dec = L.up_heatmap_decode
    ok = (p, 8 * 46 * 46, 46 * 46, 1, 1, 8, 46, 46, 368, 368, p, p, p, 0)
    def call(**kw):
        names = ("hm", "sb", "sj", "sp", "B", "J", "H", "W", "P", "Q", "idx", "preds", "maxvals", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return dec(*[a[n] for n in names])
    for bad in (dict(hm=None), dict(preds=None), dict(maxvals=None), dict(B=0), dict(J=-1), dict(H=0), dict(W=0), dict(sb=0),
                dict(sj=0), dict(sp=-1), dict(P=45), dict(Q=45), dict(P=1 << 16, Q=1 << 16), dict(sb=1 << 31, B=2),
                dict(sp=1 << 20), dict(B=1 << 16, J=1 << 16)):
        assert call(**bad) == -1, bad
    assert call(H=46, W=46, P=47, Q=45) == -1 and b"down-sampling" in L.up_last_error()


# (f) ---------------------------------------------------------------------------------------------------------------------------
def video_case(dev, K=13, B=1, size=32, T=2):
    """the video entries keep returning heat-maps: decode them in one launch; model.stride is ignored as in the reference"""
    import lstm_plan_cases as lc
    from unipose_amd import ops
    from unipose_amd.plan import UniPoseLSTMPlan
    m = mc.skeleton("lstm", K, stride=1)
    m.load_state_dict(O.synth_state_dict(K, 4, lstm=True))
    m = m.to(dev).eval()
    x = O.synth_input((B, T, 3, size, size), 15).to(dev)
    cm = O.synth_input((B, T, 1, size, size), 16, "rand").to(dev)
    plan = UniPoseLSTMPlan(m, B, size, size, frames=T)             # stride = 1 is accepted: the module never up-samples either
    heats, _, _ = plan.clip(x, cm)
    ref = lc.module_frames(lc.folded_copy(m, True), x, cm, K, T)
    for j in range(T):
        lc._equal(heats[:, j], ref[j][0], f"clip heat {j} of a stride-1 video model")
    h, w = heats.shape[-2:]
    hm = heats.reshape(B * T, K + 1, h, w)
    same(ops.heatmap_decode(hm), ops.heatmap_argmax(hm), "video heat-maps, their own grid")
    same(ops.heatmap_decode(hm, (8 * h, 8 * w)), composition(hm, (8 * h, 8 * w)), "video heat-maps, 8x")
    plan.close()
