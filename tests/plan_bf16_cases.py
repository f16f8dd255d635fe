"""The image plan in bf16 storage (``UniPosePlan(..., storage="bf16")``, up_unipose_plan_create_t) against the folded eval module
under ``ops.set_conv_math("bf16s")``: shared by the emulator and the GPU tests.  The plan issues the module's launches, so every
comparison is for EQUAL bits; how far bf16 storage is from fp32 is the business of tests/test_bf16s_*.py.

A model, its folded module, the bf16 plan, the input and the module's maps are made once per case (`setup`) and shared by the
tests that need them; nothing that is shared is written to."""
import copy
import ctypes as C

import numpy as np
import torch

import frame_cases as fc
import heat_decode_cases as hc
import protocol_cases as prc
from oracle import unipose_oracle as O
from unipose_amd import _C, ops, protocol

SENT = 7.0
FF = _C.PROGRAM_FROM_FRAMES
PROGRAMS = list(range(7)) + [FF + k for k in (0, 4, 5, 6)]


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    return prc.bits_equal(host(a), host(b))


def module_maps(folded, x):
    """the reference of every comparison: the folded eval module in bf16 storage; one (B, C, h, w) tensor also with the box head"""
    ops.set_conv_math("bf16s")
    try:
        with torch.no_grad():
            y = folded(x)
    finally:
        ops.set_conv_math("f32")
    return torch.cat(y, 1) if isinstance(y, tuple) else y


class Case:
    pass


_CASES = {}


def setup(dev, K=14, B=1, height=64, width=64, output_stride=16, bbox=False, stride=8, wseed=1):
    from unipose_amd import checkpoint
    from unipose_amd.plan import UniPosePlan
    key = (str(dev), K, B, height, width, output_stride, bbox, stride, wseed)
    if key in _CASES:
        return _CASES[key]
    kw = {}
    if output_stride != 16:
        kw["output_stride"] = output_stride
    if bbox:
        kw["bbox"] = True
    if stride != 8:
        kw["stride"] = stride
    c = Case()
    c.K, c.B, c.height, c.width, c.bbox, c.dev = K, B, height, width, bbox, dev
    c.model = hc.image_model(dev, K, wseed, **kw)
    c.folded = checkpoint.load_folded(copy.deepcopy(c.model), checkpoint.fold_batchnorm(c.model))
    c.x = O.synth_input((B, 3, height, width), 5).to(dev)
    c.plan = UniPosePlan(c.model, B, height, width, storage="bf16")
    c.ref = module_maps(c.folded, c.x)
    _CASES[key] = c
    return c


def maps(plan, x):
    y = plan(x)
    return torch.cat(y, 1) if isinstance(y, tuple) else y


# ---- 1. forward equals the module ---------------------------------------------------------------------------------------------------
FORWARD_GPU = [dict(K=14, B=1, height=64, width=64), dict(K=14, B=2, height=52, width=68),
               dict(K=16, B=2, height=48, width=48, output_stride=8, bbox=True), dict(K=14, B=2, height=52, width=68, stride=1)]
FORWARD_EMU = [dict(K=14, B=1, height=64, width=64), dict(K=14, B=2, height=36, width=44)]


def case_id(case):
    return "-".join(f"{k}{v}" for k, v in case.items())


def forward_case(dev, **case):
    c = setup(dev, **case)
    assert c.plan.storage == "bf16" and _C.lib().up_unipose_plan_dtype(c.plan._plan) == 1
    got = maps(c.plan, c.x)
    up = case.get("stride", 8) != 8                      # then plan(x) is up_unipose_forward_upsampled, as the module up-samples
    assert c.plan.upsampled == up
    hw = (c.height, c.width) if up else ((c.height - 1) // 8 + 1, (c.width - 1) // 8 + 1)
    assert tuple(got.shape) == (c.B, c.plan.out_channels) + hw == tuple(c.ref.shape)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert same(got, c.ref), float((got - c.ref).abs().max())
    return got


# ---- 2. the type is real ------------------------------------------------------------------------------------------------------------
def _fp32_forward_launches():
    L = _C.lib()
    return L.up_conv_counter(b"igemm") + L.up_conv_counter(b"glds32")


def counters_case(dev, **case):
    """up_conv_counter "igemm" + "glds32": every launch of the fp32 forward kernels (run_igemm counts one or the other; the bf16
    launches count neither).  A bf16 plan call adds the stem's launch and no more, the flip test two; the fp32 plan all 116."""
    from unipose_amd.plan import UniPosePlan
    c = setup(dev, **case)
    L = _C.lib()
    n0 = _fp32_forward_launches()
    c.plan(c.x)
    n1 = _fp32_forward_launches()
    assert n1 - n0 == 1, n1 - n0
    c.plan.flip_heatmaps(c.x, "LSP")
    n2 = _fp32_forward_launches()
    assert n2 - n1 == 2, n2 - n1
    plan32 = UniPosePlan(c.model, c.B, c.height, c.width)
    assert plan32.storage == "f32" and L.up_unipose_plan_dtype(plan32._plan) == 0
    n3 = _fp32_forward_launches()
    plan32(c.x)
    assert _fp32_forward_launches() - n3 == L.up_unipose_plan_num_convs(plan32._plan) == 116
    plan32.close()


def workspace_case(dev, **case):
    """the bf16 plan's figures are its own: every one strictly smaller than the fp32 plan's for the same shape"""
    from unipose_amd.plan import UniPosePlan
    c = setup(dev, **case)
    L = _C.lib()
    plan32 = UniPosePlan(c.model, c.B, c.height, c.width, storage="fp32")
    for f in (L.up_unipose_plan_workspace, L.up_unipose_plan_flip_workspace):
        assert 0 < f(c.plan._plan) < f(plan32._plan), (f(c.plan._plan), f(plan32._plan))
    for k in PROGRAMS:
        b, a = L.up_unipose_plan_program_workspace(c.plan._plan, k), L.up_unipose_plan_program_workspace(plan32._plan, k)
        assert 0 < b < a, (k, b, a)
    assert L.up_unipose_plan_program_workspace(c.plan._plan, 7) == 0
    need = [L.up_unipose_plan_program_workspace(c.plan._plan, k) for k in range(7)]
    assert L.up_unipose_plan_workspace(c.plan._plan) == max(need[:4]) and L.up_unipose_plan_flip_workspace(c.plan._plan) == max(need[4:])
    print("workspace bytes, bf16 / fp32:", L.up_unipose_plan_workspace(c.plan._plan), L.up_unipose_plan_workspace(plan32._plan))
    plan32.close()


# ---- 3. no stale workspace ----------------------------------------------------------------------------------------------------------
def stale_case(dev, **case):
    """every byte of the workspace 0xFF (a NaN in both types) before the call: the pad lanes a launch reads are zeroed by the program"""
    c = setup(dev, **case)
    c.plan.flip_heatmaps(c.x, "LSP")                     # (grows the workspace to the largest figure the case uses)
    c.plan.workspace.fill_(255)
    first = maps(c.plan, c.x)
    assert same(first, c.ref)
    assert same(maps(c.plan, c.x), first)
    c.plan.workspace.fill_(255)
    perm = protocol.flip_perm("LSP", c.K, c.bbox)
    a, f = maps(c.plan, c.x), maps(c.plan, c.x.flip(3).contiguous())
    c.plan.workspace.fill_(255)
    assert same(c.plan.flip_heatmaps(c.x, "LSP"), ops.flip_merge(a, f, perm))


# ---- 4. every program ---------------------------------------------------------------------------------------------------------------
def _differ(*ts):
    for i in range(len(ts)):
        for j in range(i + 1, len(ts)):
            assert not same(ts[i], ts[j]), (i, j)


def programs_case(dev, height, width):
    """K = 16 with the box head (22 channels: "MPII" puts the box at 17..21), B = 2.  Every identity is stated on the bf16 plan's
    own plan(x), as tests/protocol_cases.py and tests/frame_cases.py state them for the fp32 plan."""
    K, B, dataset = 16, 2, "MPII"
    c = setup(dev, K=K, B=B, height=height, width=width, bbox=True)
    plan, x = c.plan, c.x
    xf = x.flip(3).contiguous()
    a, f = maps(plan, x), maps(plan, xf)
    assert same(a, c.ref)
    perm = protocol.flip_perm(dataset, K, True)
    merged = ops.flip_merge(a, f, perm)
    # the two passes and the two samples differ pairwise, the mirrored pass also after it is mirrored back: a program that ran one
    # pass twice, or one sample twice, cannot pass
    _differ(a, f, f.flip(3), merged)
    _differ(a[0], a[1], f[0], f[1])
    # keypoints
    for full in (False, True):
        size = (height, width) if full else None
        want = ops.heatmap_decode(a, size)
        got = plan.keypoints(x, full_resolution=full)
        for g, w_, name in zip(got, want, ("preds", "maxvals", "idx")):
            assert same(g, w_), ("keypoints", full, name)
    # persons
    want = [host(t) for t in ops.persons_decode(a, dataset)]
    got = [host(t) for t in plan.persons(x, dataset)]
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    for b in range(B):
        if got[2][b] == 0:                                # PERSONS_OK: the rows of the persons found are specified
            assert np.array_equal(got[0][b, :got[1][b]], want[0][b, :want[1][b]])
    # the flip test
    own = torch.full((B, plan.out_channels, plan.map_height, plan.map_width), SENT, device=dev)
    assert plan.flip_heatmaps(x, dataset, out=own) is own
    assert same(own, merged)
    # final_preds
    cen = np.stack([np.array([width / 2.0 + 3 * i, height / 2.0 - 2 * i]) for i in range(B)])
    sc = np.array([max(height, width) / 200.0 * (1 + 0.1 * i) for i in range(B)])
    for flip, src in ((False, a), (True, merged)):
        for with_center in (True, False):
            args = (cen, sc) if with_center else ()
            want = ops.final_preds(src, *args, return_coords=True)
            got = plan.final_preds(x, *args, flip=flip, dataset=dataset)
            prc.same_triple([host(t) for t in got], [host(t) for t in want], ("final_preds", flip, with_center))
    # from frames: uint8 45 x 60, both samples in frame 1, their own centre and scale each
    frames = torch.from_numpy(fc.pixels_of((8, K), (2, 45, 60, 3), "u8")).to(dev)
    fo = [1] * B
    fcen = np.stack([np.array([30.0 + 5 * i, 22.0 - 3 * i]) for i in range(B)])
    fsc = np.array([0.25 * (1 + 0.3 * i) for i in range(B)])
    for flip in (False, True):
        rot = 30 if flip else 0
        xc = ops.augment_image(frames[fo], protocol.crop_maps(fcen, fsc, [height, width], rot).reshape(B, 2, 3), (height, width))
        assert tuple(xc.shape) == (B, 3, height, width)
        ac = maps(plan, xc)
        _differ(ac[0], ac[1], a[0])
        if flip:
            src = ops.flip_merge(ac, maps(plan, xc.flip(3).contiguous()), perm)
            _differ(src, ac)
        else:
            src = ac
        own = torch.full((B, plan.out_channels, plan.map_height, plan.map_width), SENT, device=dev)
        assert plan.frame_heatmaps(frames, fcen, fsc, frame_of=fo, rot=rot, flip=flip, dataset=dataset, out=own) is own
        assert same(own, src), ("frame_heatmaps", flip)
        want = ops.final_preds(src, fcen, fsc, return_coords=True)
        got = plan.frame_final_preds(frames, fcen, fsc, frame_of=fo, rot=rot, flip=flip, dataset=dataset)
        prc.same_triple([host(t) for t in got], [host(t) for t in want], ("frame_final_preds", flip))


# ---- 5. weights ---------------------------------------------------------------------------------------------------------------------
def refresh_case(dev, **case):
    """refresh(model) repacks in the plan's own type: afterwards the plan equals the changed module and no longer the old one.  (A
    plan of its own: the shared one keeps its weights.)"""
    from unipose_amd import checkpoint
    from unipose_amd.plan import UniPosePlan
    c = setup(dev, **case)
    plan = UniPosePlan(c.model, c.B, c.height, c.width, storage="bf16s")
    assert plan.storage == "bf16"
    assert same(maps(plan, c.x), c.ref)
    m2 = copy.deepcopy(c.model)
    m2.load_state_dict(O.synth_state_dict(c.K, 2))
    m2 = m2.to(dev).eval()
    plan.refresh(m2)
    got = maps(plan, c.x)
    ref2 = module_maps(checkpoint.load_folded(copy.deepcopy(m2), checkpoint.fold_batchnorm(m2)), c.x)
    assert same(got, ref2)
    assert not same(got, c.ref)
    assert _C.lib().up_unipose_plan_dtype(plan._plan) == 1
    plan.close()


def setters_case(dev):
    """a missing bias is refused as on the fp32 plan; a call before all weights are set is refused with the outputs untouched"""
    from unipose_amd.plan import _Config
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_plan_create_t(C.byref(_Config(1, 64, 52, 16, 15)), 1, C.byref(plan)) == 0
    assert L.up_unipose_plan_dtype(plan) == 1 and L.up_unipose_plan_num_convs(plan) == 116
    shape = (C.c_int32 * 4)()
    hb = C.c_int32()
    names = [L.up_unipose_plan_conv_name(plan, i).decode() for i in range(116)]
    i1 = names.index("backbone.layer1.0.conv1")
    assert L.up_unipose_plan_conv_shape(plan, i1, shape, C.byref(hb)) == 0 and tuple(shape) == (64, 64, 1, 1) and hb.value == 1
    w = torch.zeros(64 * 64).to(dev)
    out = torch.full((4096,), SENT).to(dev)
    ws = torch.zeros(1024).to(dev)
    assert L.up_unipose_plan_set_conv(plan, i1, w.data_ptr(), None, 0) == -1
    assert L.up_last_error().decode() == "unipose_plan_set_conv: backbone.layer1.0.conv1 needs a bias (folded network)"
    i2 = names.index("wasp.conv2")
    assert L.up_unipose_plan_set_conv(plan, i2, w.data_ptr(), w.data_ptr(), 0) == -1
    assert L.up_last_error().decode() == "unipose_plan_set_conv: wasp.conv2 has no a bias (folded network)"
    assert L.up_unipose_plan_set_conv(plan, i1, w.data_ptr(), w.data_ptr(), 0) == 0             # one set, 115 unset
    p, o = ws.data_ptr(), out.data_ptr()
    pa = ops._perm_array(list(range(15)), 15)
    src = (p, 0, 1, 4, 4, None, None, p, 128.0, 128.0, 256.0)
    for rc in (L.up_unipose_forward(plan, p, o, p, 1 << 40, 0), L.up_unipose_forward_upsampled(plan, p, o, p, 1 << 40, 0),
               L.up_unipose_keypoints(plan, p, 8, 7, None, o, o, p, 1 << 40, 0),
               L.up_unipose_flip_forward(plan, p, pa, o, p, 1 << 40, 0),
               L.up_unipose_final_preds(plan, p, pa, None, 8, 7, o, None, o, p, 1 << 40, 0),
               L.up_unipose_frame_heatmaps(plan, *src, pa, o, p, 1 << 40, 0),
               L.up_unipose_frame_final_preds(plan, *src, None, None, 8, 7, o, None, o, p, 1 << 40, 0)):
        assert rc == -1 and b"weights of backbone.conv1 were never set" in L.up_last_error()
    assert bool((out == SENT).all())
    L.up_unipose_plan_destroy(plan)


# ---- 6. coexistence -----------------------------------------------------------------------------------------------------------------
def coexistence_case(dev, **case):
    """the plan neither reads nor sets ops.CONV_MATH: plans of both storages of one model, alive together and called in turn"""
    from unipose_amd.plan import UniPosePlan
    c = setup(dev, **case)
    assert ops.CONV_MATH == ops.MATH_F32
    plan32 = UniPosePlan(c.model, c.B, c.height, c.width)
    before = maps(plan32, c.x).clone()
    plan16 = UniPosePlan(c.model, c.B, c.height, c.width, storage="bf16_storage")
    got16 = maps(plan16, c.x)
    assert ops.CONV_MATH == ops.MATH_F32
    after = maps(plan32, c.x)
    assert same(after, before)
    assert same(got16, c.ref) and not same(got16, before)
    assert bool(torch.isfinite(got16).all()) and bool(torch.isfinite(before).all())
    assert same(maps(plan16, c.x), got16)
    plan16.close()
    plan32.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def refusal_case(dev, **case):
    from unipose_amd.plan import UniPosePlan, _Config
    c = setup(dev, **case)
    L = _C.lib()
    # the storage type, at create: *out stays what it was
    for bad in (-1, 2):
        plan = C.c_void_p(12345)
        assert L.up_unipose_plan_create_t(C.byref(_Config(1, 64, 64, 16, 15)), bad, C.byref(plan)) == -1
        assert L.up_last_error().decode() == f"unipose_plan_create: storage type {bad} (UP_DT_F32 or UP_DT_BF16)"
        assert plan.value == 12345
    for bad in ("fp16", "", None, 1):
        try:
            UniPosePlan(None, c.B, c.height, c.width, storage=bad)       # refused before the model is looked at
            raise AssertionError(f"storage={bad!r} must be refused")
        except ValueError:
            pass
    # the workspace: one byte short of the bf16 plan's own figure, and a misaligned one — the fp32 plan's code and words
    plan, x = c.plan, c.x
    # (an entry asks for its own program's need; in bf16 storage program 1, which holds the up-sampled maps, is the largest of 0..3)
    need = L.up_unipose_plan_program_workspace(plan._plan, 1 if plan.upsampled else 0)
    assert 0 < need <= L.up_unipose_plan_workspace(plan._plan)
    big =torch.empty(need + 512, dtype=torch.uint8, device=dev)
    wp = big.data_ptr() + (-big.data_ptr()) % 256
    Bc, Cc = c.B, plan.out_channels
    sent = torch.full((Bc, Cc, plan.out_height, plan.out_width), SENT, device=dev)
    forward = L.up_unipose_forward_upsampled if plan.upsampled else L.up_unipose_forward
    who = "unipose_forward_upsampled" if plan.upsampled else "unipose_forward"
    assert forward(plan._plan, x.data_ptr(), sent.data_ptr(), wp, need - 1, 0) == -1
    assert L.up_last_error().decode() == f"{who}: workspace of {need} bytes (256-byte aligned) needed, got {need - 1}"
    assert forward(plan._plan, x.data_ptr(), sent.data_ptr(), wp + 4, need + 200, 0) == -1
    assert L.up_last_error().decode() == f"{who}: workspace of {need} bytes (256-byte aligned) needed, got {need + 200}"
    # the Python boundary is fp32 and contiguous as on the fp32 plan
    for bad_x in (x[:, :, :c.height - 8], x.double(), x.to(torch.bfloat16)):
        try:
            plan(bad_x)
            raise AssertionError("a mis-shaped / mis-typed input must be refused")
        except ValueError:
            pass
    h, w = plan.out_height, plan.out_width
    for bad in (torch.full((Bc, Cc, h - 1, w), SENT, device=dev), torch.full((Bc, Cc, h, w), SENT, device=dev).double(),
                torch.full((Bc, Cc, h, 2 * w), SENT, device=dev)[..., ::2], torch.full((Bc, Cc, h, w), SENT, device=dev).to(torch.bfloat16)):
        try:
            plan(x, out=bad)
            raise AssertionError("a mis-shaped / double / strided / bf16 `out` must be refused")
        except ValueError:
            pass
        assert bool((bad == SENT).all())
    assert bool((sent == SENT).all())                    # no refused call wrote anything
    own = torch.empty((Bc, Cc, h, w), device=dev)
    plan(x, out=own)
    assert same(own, c.ref)
