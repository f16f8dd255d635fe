"""Training targets of the box head (up_make_box_maps, ops.make_box_maps, DeviceBatcher(bbox=True), Trainer with args.bbox) and the
train-mode parity of the bbox=True model: shared by test_box_targets_emu.py and test_box_targets_gpu.py.

Yardsticks.  The fixture G19 (tools/make_goldens.py g19) holds outputs of the reference's OWN getBoundingBox, both loader forms
(utils/lsp_lspet_data.py:71-113 raises ValueError for a sample without a counted joint, utils/bbc_data.py:23-72 gives the zero
box).  `restate` below says the same in this project's words and must reproduce every G19 array bit for bit; beyond the fixture
it is the reference.  The entry is compared under the rule of the sibling target kernels, op_cases.check_target_maps (at most one
float32 ulp, exact elsewhere), and must ADDITIONALLY flip no element across the 0.0099 cut: (got == 0) == (ref == 0) everywhere.
That is a condition, not a measurement: the centres are integers, so D2 is an integer, and at sigma 3 the values nearest the cut
are exp(-82/18) = 0.01051 and exp(-85/18) = 0.00889 (83 and 84 are no sums of two squares) — a device exp() one float64 ulp off
cannot cross.  WORST collects the largest float32-ulp difference and the flipped count that the run saw.

bbox_train_case follows model_cases.train_case (same yardstick, slack and floors: the reference's own fp32-vs-fp64 error)."""
import math
import os

import numpy as np
import torch

import model_cases as mc
import persons_cases as pc
from contract_cases import HEATMAP_CASES
from op_cases import check_target_maps
from oracle import unipose_oracle as O
from unipose_amd import _C, ops

F32 = torch.float32
SENT = 7.0
OK, NO_VISIBLE = 0, 1
SIZES = [c[:3] for c in HEATMAP_CASES]            # (height, width, stride): 96x160 s8, 100x50 s3, 16x40 s8, 368x200 s8
KS = (1, 14, 65, 300)
BIG = (1100, 368, 368, 8)                         # 1100 x 46 x 46 = 2 327 600 output pixels (> 2^21), 11.6 M values
WORST = {"ulps": 0, "flipped": 0}


# ---- the reference's function in this project's words ---------------------------------------------------------------------------
def box_cells(kpt, height, width, stride):
    """-> (counted, [(column, row)] * 5): whether any joint has a coordinate >= 0, and the integer Gaussian centres of the maps
    centre, top-left, bottom-left, top-right, bottom-right.  The extent `lo2 .. hi2` of the SECOND coordinates is cut to
    0 .. width and picks the ROW, the extent of the first is cut to 0 .. height and picks the COLUMN (the reference's own order);
    every int() truncates towards zero.  Without a counted joint the box is 0, 0, 0, 0 (the BBC loader's guard)."""
    kpt = np.asarray(kpt, dtype=np.float64).reshape(-1, 2)
    keep = (kpt[:, 1] >= 0) | (kpt[:, 0] >= 0)
    lo2 = hi2 = lo1 = hi1 = 0
    if keep.any():
        first, second = kpt[keep, 0].tolist(), kpt[keep, 1].tolist()
        lo2, hi2 = math.trunc(max(min(second), 0)), math.trunc(min(max(second), width))
        lo1, hi1 = math.trunc(max(min(first), 0)), math.trunc(min(max(first), height))

    def cell(v, n):
        return math.trunc(min(math.trunc(v / stride), n / stride - 1))

    cols = [cell((lo1 + hi1) / 2, height), cell(lo1, height), cell(hi1, height)]
    rows = [cell((lo2 + hi2) / 2, width), cell(lo2, width), cell(hi2, width)]
    return bool(keep.any()), [(cols[0], rows[0]), (cols[1], rows[1]), (cols[1], rows[2]), (cols[2], rows[1]), (cols[2], rows[2])]


def restate(kpt, height, width, stride, sigma=3.0):
    """-> ((5, h, w) float32, counted): the Gaussian of the joint maps (oracle.gaussian_kernel, which G8 pins) around box_cells"""
    counted, centres = box_cells(kpt, height, width, stride)
    h, w = int(height / stride), int(width / stride)
    maps = np.stack([O._clip_map(O.gaussian_kernel(w, h, float(c), float(r), sigma)) for c, r in centres]).astype(np.float32)
    return maps, counted


_REF = {}


def restate_batch(kpt, height, width, stride, sigma=3.0, key=None):
    """(B,5,h,w) and the status vector; computed once per `key` and shared"""
    if key is not None and key in _REF:
        return _REF[key]
    res = [restate(k, height, width, stride, sigma) for k in kpt]
    out = np.stack([m for m, _ in res]), np.array([OK if c else NO_VISIBLE for _, c in res], dtype=np.int32)
    for a in out:
        a.setflags(write=False)
    if key is not None:
        _REF[key] = out
    return out


def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_box_targets.npz"))


def g19_cfg(g, tag):
    height, width, stride = g[tag + "_cfg"].tolist()
    return int(height), int(width), (int(stride) if stride == int(stride) else stride)


def draw(seed, b, k, height, width, invisible=0.15):
    """key points up to 30 pixels outside the image, some joints marked (-1, -1), never a sample without a counted joint"""
    rng = np.random.default_rng([19, *seed])
    kpt = np.stack([rng.uniform(-30, width + 30, (b, k)), rng.uniform(-30, height + 30, (b, k))], axis=2)
    kpt[rng.uniform(size=(b, k)) < invisible] = -1.0
    kpt[:, 0] = np.abs(kpt[:, 0]) + 1.0
    return kpt


# ---- the entry ------------------------------------------------------------------------------------------------------------------
def entry(dev, kpt, height, width, stride, sigma=3.0, with_status=True):
    """up_make_box_maps itself on a sentinel-filled output -> numpy (maps, status or None)"""
    k = torch.from_numpy(np.ascontiguousarray(kpt, dtype=np.float64)).to(dev)
    b, nk, _ = k.shape
    out = torch.full((b, 5, int(height / stride), int(width / stride)), SENT, dtype=F32, device=dev)
    st = torch.full((b,), -77, dtype=torch.int32, device=dev) if with_status else None
    _C.check(_C.lib().up_make_box_maps(k.data_ptr(), b, nk, height, width, float(stride), float(sigma), out.data_ptr(),
                                       st.data_ptr() if with_status else None, ops._stream(out)), "make_box_maps")
    return out.cpu(), (st.cpu().numpy() if with_status else None)


def compare(got, ref, what):
    """check_target_maps, no flip across the cut, and the float32-ulp distance for the record"""
    g = got.cpu().numpy()
    flipped = int(((g == 0) != (ref == 0)).sum())
    ulps = int(np.abs(g.view(np.int32).astype(np.int64) - np.ascontiguousarray(ref).view(np.int32).astype(np.int64))[(g != 0) & (ref != 0)]
               .max(initial=0))
    WORST["ulps"], WORST["flipped"] = max(WORST["ulps"], ulps), WORST["flipped"] + flipped
    print("%s: %d float32 ulps, %d flipped" % (what, ulps, flipped))
    check_target_maps(got, ref, what)
    assert flipped == 0, (what, flipped)
    assert ulps <= 1, (what, ulps)


def report():
    return "up_make_box_maps: worst float32-ulp difference %d, elements flipped across the 0.0099 cut %d" % (WORST["ulps"], WORST["flipped"])


# 1 ---- restatement = reference (no device) ---------------------------------------------------------------------------------------
def restatement_case(golden_dir):
    g = g19(golden_dir)
    tags = [str(t) for t in g["tags"]]
    assert len(tags) >= 23 and len({t[0] for t in tags}) == 9                   # the case groups a .. i of tools/make_goldens.py g19
    raised = 0
    for tag in tags:
        height, width, stride = g19_cfg(g, tag)
        maps, counted = restate(g[tag + "_kpt"], height, width, stride)
        assert maps.dtype == np.float32 and maps.shape == g[tag + "_bbc"].shape, tag
        assert np.array_equal(maps.view(np.uint32), g[tag + "_bbc"].view(np.uint32)), tag
        assert bool(g[tag + "_lsp_raises"]) == (not counted), tag
        if counted:
            assert np.array_equal(maps.view(np.uint32), g[tag + "_lsp"].view(np.uint32)), tag
        raised += not counted
    assert raised >= 2
    # what the fixture's cases are there to pin, said once by hand
    assert box_cells(g["b_truncation_kpt"], 368, 368, 8)[1][0][1] == -1 and box_cells(g["b_truncation_kpt"], 368, 368, 8)[1][4][1] == -2
    assert box_cells(g["c_beyond_100x50_s3_kpt"], 100, 50, 3)[1][4] == (32, 15)
    assert box_cells(g["d_swapped_160x96_kpt"], 160, 96, 8)[1][4][1] == 11      # the row from 150.75, cut at width = 96: last cell
    assert box_cells(g["f_none_counted_kpt"], 368, 368, 8) == (False, [(0, 0)] * 5)


# 2 ---- entry = G19 ------------------------------------------------------------------------------------------------------------
def golden_case(dev, golden_dir):
    g = g19(golden_dir)
    for tag in (str(t) for t in g["tags"]):
        height, width, stride = g19_cfg(g, tag)
        got, st = entry(dev, g[tag + "_kpt"][None], height, width, stride)
        compare(got, g[tag + "_bbc"][None], tag)
        assert st.tolist() == [NO_VISIBLE if g[tag + "_lsp_raises"] else OK], tag
        if not g[tag + "_lsp_raises"]:
            compare(ops.make_box_maps(g[tag + "_kpt"][None], height, width, stride, dev), g[tag + "_lsp"][None], tag + " (op)")


# 3 ---- entry = restatement at further shapes ----------------------------------------------------------------------------------
def shape_case(dev, size, k, b):
    height, width, stride = size
    kpt = draw((height, width, k, b), b, k, height, width)
    ref, ref_st = restate_batch(kpt, height, width, stride, key=(size, k, b))
    assert ref_st.tolist() == [OK] * b
    got, st = entry(dev, kpt, height, width, stride)
    compare(got, ref, (size, k, b))
    assert st.tolist() == ref_st.tolist()
    bare, none = entry(dev, kpt, height, width, stride, with_status=False)            # status == NULL
    assert none is None and torch.equal(bare, got)
    op = ops.make_box_maps(kpt, height, width, stride, dev, empty="bbc")
    assert op.dtype == F32 and torch.equal(op.cpu(), got)


def middle_failure_case(dev):
    """a sample without a counted joint between two ordinary ones: its neighbours are what they are alone"""
    height, width, stride = 96, 160, 8
    kpt = draw((5,), 3, 14, height, width)
    kpt[1] = np.stack([np.linspace(-40.0, -0.5, 14), np.linspace(-1.0, -300.0, 14)], axis=1)
    ref, ref_st = restate_batch(kpt, height, width, stride)
    assert ref_st.tolist() == [OK, NO_VISIBLE, OK]
    got, st = entry(dev, kpt, height, width, stride)
    compare(got, ref, "middle failure")
    assert st.tolist() == [OK, NO_VISIBLE, OK]
    assert float(got[1, :, 0, 0].min()) == 1.0                                        # five Gaussians at pixel (0, 0)
    for i in (0, 2):
        alone, st1 = entry(dev, kpt[i:i + 1], height, width, stride)
        assert torch.equal(alone[0], got[i]) and st1.tolist() == [OK]


def sigma_case(dev):
    """the entry takes sigma like its siblings (the reference hard-codes 3); here only the one-ulp rule applies"""
    height, width, stride = 96, 160, 8
    kpt = draw((6,), 2, 14, height, width)
    for sigma in (1.0, 4.5):
        got, _ = entry(dev, kpt, height, width, stride, sigma=sigma)
        check_target_maps(got, restate_batch(kpt, height, width, stride, sigma)[0], ("sigma", sigma))
        assert torch.equal(ops.make_box_maps(kpt, height, width, stride, dev, sigma=sigma).cpu(), got)


def big_case(dev):
    """more than 2^21 output pixels in one launch; every sample is one of three, so three restatements are the reference"""
    b, height, width, stride = BIG
    assert b * (height // stride) * (width // stride) > 2 ** 21
    base = draw((7,), 3, 14, height, width)
    base[1] = -1.0
    ref, ref_st = restate_batch(base, height, width, stride)
    pick = np.arange(b) % 3
    got = ops.make_box_maps(base[pick], height, width, stride, dev, empty="bbc")
    assert tuple(got.shape) == (b, 5, 46, 46)
    for i in range(3):
        compare(got[i], ref[i], ("big", i))
        assert bool((got[i::3] == got[i]).all()), i
    _, st = entry(dev, base[pick][-5:], height, width, stride)
    assert st.tolist() == ref_st[pick[-5:]].tolist()


# 4 ---- round trip with the decoder --------------------------------------------------------------------------------------------
def roundtrip_case(dev):
    """targets -> LSP layout (15 joint channels + 5 box channels) -> the multi-person decode: the device's list equals
    oracle.unipose_kpts_multi of the same maps, i.e. the targets and the decoder agree on the channel order"""
    def maps_of(kpt, size=368):
        k = np.asarray(kpt, dtype=np.float64)[None]
        m = torch.cat([ops.make_heatmaps(k, size, size, 8, 3.0, dev), ops.make_box_maps(k, size, size, 8, dev, empty="bbc")], 1)
        assert tuple(m.shape) == (1, 20, size // 8, size // 8)
        return m.cpu().numpy()

    rng = np.random.default_rng(23)
    for trial, (c0, c1, r0, r1) in enumerate(((5, 30, 8, 40), (12, 20, 3, 9), (0, 45, 0, 45))):
        cells = np.stack([rng.integers(c0, c1 + 1, 14), rng.integers(r0, r1 + 1, 14)], axis=1)
        cells[0], cells[1] = (c0, r0), (c1, r1)                                 # two joints span the box
        kpt = cells * 8.0 + 0.5                                                 # int(coordinate) / 8 is the cell itself
        want = pc.against_oracle(maps_of(kpt), dev)
        assert len(want) == 19 and {row[0] for row in want} == {0}, trial       # one person
        _, centres = box_cells(kpt, 368, 368, 8)
        assert [row[1:] for row in want[14:]] == [list(c) for c in centres], trial
        assert centres[1] == (c0, r0) and centres[4] == (c1, r1)
        for j, (cx, cy) in enumerate(cells.tolist()):                           # the box is half-open: rows r0 .. r1-1, columns c0 .. c1-1
            assert want[j][1:] == [min(cx, c1 - 1), min(cy, r1 - 1)], (trial, j)
    one = np.full((14, 2), -1.0)
    one[6] = (200.5, 120.5)                                                     # one joint: x_min == x_max, the box is empty
    assert pc.against_oracle(maps_of(one), dev) is ValueError


# 5 ---- refusals -----------------------------------------------------------------------------------------------------------------
def refusal_case(dev):
    L = _C.lib()
    kpt = torch.zeros(3, 14, 2, dtype=torch.float64).to(dev)
    out = torch.full((3 * 5 * 46 * 46,), SENT, dtype=F32).to(dev)
    st = torch.full((3,), -77, dtype=torch.int32).to(dev)
    names = ("kpt", "B", "K", "height", "width", "stride", "sigma", "out", "status", "stream")
    ok = (kpt.data_ptr(), 3, 14, 368, 368, 8.0, 3.0, out.data_ptr(), st.data_ptr(), ops._stream(out))

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.up_make_box_maps(*[a[n] for n in names])

    for bad in (dict(kpt=None), dict(out=None), dict(B=0), dict(B=-1), dict(K=0), dict(height=0), dict(width=-5), dict(stride=0.0),
                dict(stride=-8.0), dict(sigma=0.0), dict(sigma=-3.0), dict(height=7), dict(width=7), dict(stride=400.0),
                dict(B=1 << 20), dict(B=2, stride=0.01)):
        assert call(**bad) == -1, bad
        assert L.up_last_error().startswith(b"make_box_maps:"), (bad, L.up_last_error())
    assert bool((out.cpu() == SENT).all()) and st.cpu().tolist() == [-77] * 3          # nothing was launched
    assert call() == 0 and call(status=None) == 0
    assert st.cpu().tolist() == [OK] * 3 and not bool((out.cpu() == SENT).any())


def empty_policy_case(dev):
    """empty='raise' is the LSP loader (ValueError), decided on the host for host annotations and from the kernel's status for a
    tensor that is already on the device; empty='bbc' never raises"""
    kpt = draw((8,), 3, 14, 96, 160)
    kpt[2] = -1.0
    for data in (kpt, kpt.tolist(), torch.from_numpy(kpt), torch.from_numpy(kpt).to(dev)):
        try:
            ops.make_box_maps(data, 96, 160, 8, dev)
            raise AssertionError("ValueError expected")
        except ValueError as e:
            assert "sample 2" in str(e)
        got = ops.make_box_maps(data, 96, 160, 8, dev, empty="bbc")
        assert float(got[2, :, 0, 0].min()) == 1.0
    for data in (kpt[:2], torch.from_numpy(kpt[:2]).to(dev)):
        assert tuple(ops.make_box_maps(data, 96, 160, 8, dev).shape) == (2, 5, 12, 20)
    try:
        ops.make_box_maps(kpt, 96, 160, 8, dev, empty="zero")
        raise AssertionError("ValueError expected")
    except ValueError:
        pass


# 6 ---- the bbox=True model in train mode ----------------------------------------------------------------------------------------
def bbox_state_dict(K, wseed):
    """the synthetic weights with the widened output layer of test_multi_person._bbox_model"""
    sd = O.synth_state_dict(K, wseed)
    g = torch.Generator().manual_seed(3)
    sd["decoder.last_conv.8.weight"] = torch.randn(K + 6, 256, 1, 1, generator=g) * 0.05
    sd["decoder.last_conv.8.bias"] = torch.randn(K + 6, generator=g) * 0.1
    return sd


def bbox_train_case(dev, K=14, B=2, size=32, wseed=3):
    """model_cases.train_case for unipose(bbox=True): forward, the SUM of two MSE losses over the model's two outputs, one backward;
    targets from ops.make_heatmaps / ops.make_box_maps of synthetic key points.  Loss, both outputs, every parameter gradient and
    the running statistics against the oracle graph differentiated in fp32 and fp64 under the replayed ReLU signs."""
    import torch.nn.functional as F
    m = mc.skeleton("image", K, bbox=True)
    sd = bbox_state_dict(K, wseed)
    m.load_state_dict(sd)
    m = m.to(dev)
    assert m.bbox and m.decoder.last_conv[8].out_channels == K + 6
    m.train()
    m.wasp.dropout.p = 0.0
    m.decoder.last_conv[3].p = 0.0
    m.decoder.last_conv[7].p = 0.0
    pdrop = (0.0, 0.0, 0.0)
    x = O.synth_input((B, 3, size, size), 13)
    kpt = draw((9,), B, K, size, size)
    t_heat = ops.make_heatmaps(kpt, size, size, 8, 3.0, dev)
    t_box = ops.make_box_maps(kpt, size, size, 8, dev)
    assert tuple(t_heat.shape) == (B, K + 1, size // 8, size // 8) and tuple(t_box.shape) == (B, 5, size // 8, size // 8)
    sd32 = O.clone_sd(sd, requires_grad=True)
    sd64 = mc._sd64(sd, True)
    trace = []
    ops.set_relu_trace(trace)
    try:
        heat, box = m(x.to(dev))
        loss = ops.mse_loss(heat, t_heat) + ops.mse_loss(box, t_box)
        loss.backward()
    finally:
        ops.set_relu_trace(None)
    assert tuple(heat.shape) == tuple(t_heat.shape) and tuple(box.shape) == tuple(t_box.shape)
    trace = [z.cpu() for z in trace]
    th, tb = t_heat.cpu(), t_box.cpu()
    y = torch.cat([heat, box], 1).detach().cpu()
    with torch.no_grad(), O.relu_record() as rec:
        y_plain = O.unipose_forward(O.clone_sd(sd), x, train=True, p_drop=pdrop)
    assert y_plain.shape == y.shape and O.max_rel(y, y_plain) < 1e-3
    mc.relu_sign_agreement(trace, rec.pre)
    with O.relu_masks_from(trace):
        y32 = O.unipose_forward(sd32, x, train=True, p_drop=pdrop)
    l32 = F.mse_loss(y32[:, :K + 1], th) + F.mse_loss(y32[:, K + 1:], tb)
    l32.backward()
    with O.relu_masks_from(trace):
        y64 = O.unipose_forward(sd64, x.double(), train=True, p_drop=pdrop)
    l64 = F.mse_loss(y64[:, :K + 1], th.double()) + F.mse_loss(y64[:, K + 1:], tb.double())
    l64.backward()
    for name, sl in (("joint maps", slice(0, K + 1)), ("box maps", slice(K + 1, K + 6))):
        ok, eo, er = mc.yardstick(y[:, sl], y32.detach()[:, sl], y64.detach()[:, sl])
        print("%s: ours %.3g, fp32 oracle %.3g" % (name, eo, er))
        assert ok, (name, eo, er)
    ok, eo, er = mc.yardstick(loss.detach().cpu(), l32.detach(), l64.detach())
    print("loss: ours %.3g, fp32 oracle %.3g" % (eo, er))
    assert ok, ("loss", eo, er)
    worst = {}
    for name, p in m.named_parameters():
        g64 = sd64[name].grad
        if g64 is None:
            assert p.grad is None, name                      # decoder.conv2 / bn2
            continue
        ok, eo, er = mc.yardstick(p.grad.cpu(), sd32[name].grad, g64, floor=1e-4)
        if not ok:
            worst[name] = (eo, er)
    assert not worst, worst
    msd = m.state_dict()
    for k, v in sd64.items():
        if "running_" in k:
            ok, eo, er = mc.yardstick(msd[k].cpu(), sd32[k], v)
            assert ok, (k, eo, er)
        if k.endswith("num_batches_tracked") and not k.startswith("decoder.bn2"):
            assert int(msd[k]) == int(v) == 1, k
    head = m.decoder.last_conv[8].weight.grad.cpu()
    assert head.shape[0] == K + 6 and bool((head[K + 1:].abs().amax(dim=(1, 2, 3)) > 0).all())    # the box rows got a gradient


# 7 ---- batcher and trainer --------------------------------------------------------------------------------------------------------
def batcher_case(dev):
    from unipose_amd.trainer import DeviceBatcher, SyntheticPoseData
    item = next(iter(SyntheticPoseData(14, 2, 1, size=32, seed=1)))
    plain = DeviceBatcher(dev, 8, 3)(item)
    assert len(plain) == 3
    x, heat, cm, box = DeviceBatcher(dev, 8, 3, bbox=True)(item)
    assert all(torch.equal(a, b) for a, b in zip(plain, (x, heat, cm)))
    assert tuple(box.shape) == (2, 5, 4, 4)
    compare(box, restate_batch(item["kpts"], 32, 32, 8)[0], "batcher")
    clip = next(iter(SyntheticPoseData(13, 2, 1, size=32, frames=3, seed=2)))              # leading clip dimensions, as for heat
    out = DeviceBatcher(dev, 8, 1, bbox=True)(clip)
    assert tuple(out[1].shape) == (2, 3, 14, 4, 4) and tuple(out[3].shape) == (2, 3, 5, 4, 4)
    compare(out[3].reshape(6, 5, 4, 4), restate_batch(clip["kpts"].reshape(6, 13, 2), 32, 32, 8)[0], "batcher clip")
    tup = (x.cpu(), heat.cpu(), cm.cpu(), ["a", "b"], 0, box.cpu())                         # lsp_lspet_data.py:249
    moved = DeviceBatcher(dev, 8, 3, bbox=True)(tup)
    assert len(moved) == 4 and torch.equal(moved[3].cpu(), box.cpu())
    assert len(DeviceBatcher(dev, 8, 3)(tup)) == 3
    try:
        DeviceBatcher(dev, 8, 3, bbox=True)(tup[:4])
        raise AssertionError("a four-entry sample has no box maps")
    except ValueError:
        pass
    return tup


def trainer_case(dev):
    import argparse
    from unipose_amd.trainer import Trainer
    args = argparse.Namespace(dataset="LSP", pretrained=None, model_name=None, model_arch="unipose", train_dir=None, val_dir=None,
                              batch_size=2, size=32, train_batches=1, val_batches=1, bbox=True)
    tr = Trainer(args, device=dev)
    assert tr.model.bbox and tr.batcher.bbox and tr.model.decoder.last_conv[8].out_channels == 20
    w0 = tr.model.decoder.last_conv[8].weight.detach().clone()
    loss = tr.training(0)
    assert np.isfinite(loss) and tr.iters == 1
    w1 = tr.model.decoder.last_conv[8].weight.detach()
    assert bool(((w1 - w0)[15:].abs().amax(dim=(1, 2, 3)) > 0).all()) and not torch.equal(w0[:15], w1[:15])
    m = tr.validation(0)
    assert m.evals == 1 and 0.0 <= m.mPCKh <= 1.0
    pixels = torch.randint(0, 256, (32, 32, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    kpts, up = tr.test(pixels)
    assert len(kpts) == 14 and tuple(up.shape) == (1, 15, 32, 32)
    tr.train_loader = [batcher_case(dev)]                                                  # a reference-style six-entry tuple
    assert np.isfinite(tr.training(1)) and tr.iters == 2
    plain = Trainer(argparse.Namespace(**{**vars(args), "bbox": False}), device=dev)
    assert not plain.model.bbox and not plain.batcher.bbox and plain.model.decoder.last_conv[8].out_channels == 15
