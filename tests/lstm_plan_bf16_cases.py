"""The video plan in bf16 storage (``UniPoseLSTMPlan(..., storage="bf16")``, up_unipose_lstm_plan_create_t) against the folded eval
module under ``ops.set_conv_math("bf16s")``: shared by the emulator and the GPU tests.  The plan issues the module's launches —
a bf16 trunk that hands over fp32 heat-maps, fp32 ConvLSTM state and head whose convolutions of 32-aligned input width run on
bf16 operands — so every comparison is for EQUAL bits; how far bf16 storage is from fp32 is the business of
tests/model_cases.py::lstm_bf16s_case.

The compositions every program must equal are the ones tests/video_eval_cases.py and tests/video_frame_cases.py state for the
fp32 plan: their case functions run here unchanged on a context whose plan is a bf16 one (`bf16_plans`).  A model, its folded
copies, the plans of both storages, the inputs and the module's results are made once per case (`setup`) and shared by the tests
that need them; nothing that is shared is written to."""
import contextlib
import copy
import ctypes as C

import torch

import lstm_plan_cases as lc
import plan_bf16_cases as bc
import video_eval_cases as vc
import video_frame_cases as vf
from unipose_amd import _C, ops

SENT = bc.SENT
PAIRS = vc.PAIRS
FF = _C.PROGRAM_FROM_FRAMES
PROGRAMS = list(range(9)) + [FF + k for k in (2, 4, 5, 6, 7, 8)]       # the 15 rows of LSTM_PROGRAMS
TRUNK_CONVS = 116                                                      # launches of the trunk, wasp.conv2 twice

# K = 13: (K + 1) % 4 != 0, the stacked gate convolution reads 16 + 16 = 32 lanes: bf16 operands.  K = 15: (K + 1) % 4 == 0, it reads
# 20 + 20 = 40 lanes: fp32.  32 x 40: 4 x 5 maps, H != W; 39 x 39: an odd size (39 % 8 == 7); 64 x 72 at output stride 8.
GPU_A = dict(K=13, B=2, T=3, H=32, W=40)
GPU_B = dict(K=15, B=1, T=2, H=39, W=39)
GPU_S8 = dict(K=13, B=1, T=2, H=64, W=72, output_stride=8)
EMU_A = dict(K=13, B=1, T=2, H=32, W=32)
EMU_B = dict(K=15, B=1, T=2, H=32, W=32)


def case_id(case):
    return "-".join(f"{k}{v}" for k, v in case.items())


same = bc.same


@contextlib.contextmanager
def bf16s():
    ops.set_conv_math("bf16s")
    try:
        yield
    finally:
        ops.set_conv_math("f32")


@contextlib.contextmanager
def bf16_plans(models=None):
    """The helpers of the fp32 files build their plan as ``UniPoseLSTMPlan(model, B, H, W, frames=T)``: inside this block that
    name makes the bf16 plan of the same arguments (and `models` collects the models it was built from)."""
    from unipose_amd import plan as P
    real = P.UniPoseLSTMPlan

    def make(model, *args, **kw):
        if models is not None:
            models.append(model)
        return real(model, *args, storage="bf16", **kw)
    P.UniPoseLSTMPlan = make
    try:
        yield
    finally:
        P.UniPoseLSTMPlan = real


class Case:
    pass


_CASES = {}


def setup(dev, K=13, B=1, T=2, H=32, W=32, output_stride=16):
    """ctx: video_eval_cases.PlanCtx on a bf16 plan — the inputs (T + 1 frames), and the plan's OWN clip, mirrored clip, merged
    maps and steps; ref_step / ref_clip: the folded module under bf16s, per frame resp. the whole-clip unroll."""
    key = (str(dev), K, B, T, H, W, output_stride)
    if key in _CASES:
        return _CASES[key]
    c = Case()
    c.dev, c.K, c.B, c.T, c.H, c.W = dev, K, B, T, H, W
    models = []
    with bf16_plans(models):
        c.ctx = vc.PlanCtx(dev, K, B, T, H, W, output_stride)
    c.model, c.plan = models[0], c.ctx.plan
    c.folded_step, c.folded_clip = lc.folded_copy(c.model, False), lc.folded_copy(c.model, True)
    with bf16s():
        c.ref_step = lc.module_frames(c.folded_step, c.ctx.x, c.ctx.cm, K, T + 1)
        c.ref_clip = lc.module_frames(c.folded_clip, c.ctx.xc, c.ctx.cmc, K, T)
    c.plan32 = c.frames = None
    _CASES[key] = c
    return c


def plan32(c):
    """the fp32 plan of the same model and shape, through the plain create entry"""
    from unipose_amd.plan import UniPoseLSTMPlan
    if c.plan32 is None:
        c.plan32 = UniPoseLSTMPlan(c.model, c.B, c.H, c.W, frames=c.T)
        assert c.plan32.storage == "f32"
    return c.plan32


def frame_ctx(c):
    if c.frames is None:
        c.frames = vf.FrameCtx(c.ctx)
    return c.frames


def _fine(t):
    assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())


# ---- 1. forward equals the module ---------------------------------------------------------------------------------------------------
def forward_case(dev, **case):
    """step over T + 1 frames, clip over T, the clip's last state handed to step for frame T (lstm_plan_cases.lstm_plan_case, with
    the module under bf16s), and a second clip on the same workspace into the caller's tensors"""
    c = setup(dev, **case)
    x, cm, plan, T = c.ctx.x, c.ctx.cm, c.plan, c.T
    assert plan.storage == "bf16" and _C.lib().up_unipose_lstm_plan_dtype(plan._plan) == 1
    prev = None
    for j in range(T + 1):
        got = plan.step(x[:, j], cm[:, j], prev)
        for g, r, n in zip(got, c.ref_step[j], ("heat", "cell", "hide")):
            _fine(g)
            lc._equal(g, r, f"step frame {j} {n}")
        prev = (got[2], got[1])
    heats, cell, hide = c.ctx.heats, c.ctx.cell, c.ctx.hide                   # plan.clip(xc, cmc), made by setup
    assert tuple(heats.shape) == (c.B, T, c.K + 1, (c.H - 1) // 8 + 1, (c.W - 1) // 8 + 1)
    for t in (heats, cell, hide):
        _fine(t)
    for j in range(T):
        lc._equal(heats[:, j], c.ref_clip[j][0], f"clip heat {j}")
    lc._equal(cell, c.ref_clip[T - 1][1], "clip last cell")
    lc._equal(hide, c.ref_clip[T - 1][2], "clip last hide")
    with bf16s(), torch.no_grad():
        nxt = c.folded_step(x, cm, T, c.ref_clip[T - 1][0], hide, cell)
    got = plan.step(x[:, T], cm[:, T], (hide, cell))
    for g, r, n in zip(got, nxt, ("heat", "cell", "hide")):
        lc._equal(g, r, f"step after clip {n}")
    own = tuple(torch.full_like(t, SENT) for t in (heats, cell, hide))
    again = plan.clip(c.ctx.xc, c.ctx.cmc, out=own)
    assert all(a is o for a, o in zip(again, own))
    for a, r, n in zip(again, (heats, cell, hide), ("heat", "cell", "hide")):
        lc._equal(a, r, f"second clip {n}")


# ---- 2. every program is an identity on the plan's own results ------------------------------------------------------------------------
def eval_programs_case(dev, **case):
    """programs 3 .. 8: clip_keypoints, clip_flip_heatmaps, clip_final_preds with and without the flip test, stream first / next"""
    c = setup(dev, **case)
    vc.plan_keypoints_case(c.ctx)
    vc.plan_flip_case(c.ctx)
    vc.plan_final_case(c.ctx)
    vc.plan_stream_case(c.ctx)


def frame_programs_case(dev, **case):
    """the six rows from frames (45 x 60 uint8 frames): against clip / clip_flip_heatmaps / clip_final_preds / stream of
    ops.augment_image(frames[frame_of], crop_maps(...)) and ops.make_centermaps(crop_center) on the same bf16 plan"""
    f = frame_ctx(setup(dev, **case))
    assert f.frames.dtype == torch.uint8 and tuple(f.frames.shape[1:3]) == vf.FRAME_HW == (45, 60)
    vf.plan_heatmaps_case(f)
    vf.plan_flip_case(f)
    vf.plan_final_case(f)
    vf.plan_stream_case(f)


# ---- 3. the type is real and the arithmetic rule holds ---------------------------------------------------------------------------------
def counters_case(dev, **case):
    """up_conv_counter "igemm" + "glds32": every launch of the fp32 forward kernels.  A bf16 plan's clip adds the stem, lstm_0 and the
    head's conv1, and at K = 15 the T - 1 gate convolutions of 40 lanes; conv2 .. conv5 (128 lanes) and the gate convolution of 32
    lanes at K = 13 run on bf16 operands and count neither."""
    c = setup(dev, **case)
    L = _C.lib()
    want = {13: 3, 15: 3 + (c.T - 1)}[c.K]
    n0 = bc._fp32_forward_launches()
    c.plan.clip(c.ctx.xc, c.ctx.cmc)
    n1 = bc._fp32_forward_launches()
    assert n1 - n0 == want, (n1 - n0, want)
    c.plan.clip_flip_heatmaps(c.ctx.xc, c.ctx.cmc, pairs=PAIRS)
    n2 = bc._fp32_forward_launches()
    assert n2 - n1 == 2 * want, (n2 - n1, want)
    p32 = plan32(c)
    assert L.up_unipose_lstm_plan_dtype(p32._plan) == 0 and L.up_unipose_lstm_plan_dtype(c.plan._plan) == 1
    n3 = bc._fp32_forward_launches()
    p32.clip(c.ctx.xc, c.ctx.cmc)
    assert bc._fp32_forward_launches() - n3 >= want + TRUNK_CONVS, (bc._fp32_forward_launches() - n3, want)


# ---- 4. a wrong arithmetic choice cannot pass ------------------------------------------------------------------------------------------
def differs_case(dev, **case):
    c = setup(dev, **case)
    heats32 = plan32(c).clip(c.ctx.xc, c.ctx.cmc)[0]
    _fine(heats32)
    assert not same(c.ctx.heats, heats32)
    ref32 = lc.module_frames(c.folded_step, c.ctx.x, c.ctx.cm, c.K, 1)[0]          # frame 0 of the module under f32
    assert ops.CONV_MATH == ops.MATH_F32
    for a, b in zip(c.ref_step[0], ref32):
        assert not same(a, b)


# ---- 5. workspace and state ------------------------------------------------------------------------------------------------------------
def workspace_case(dev, **case):
    c = setup(dev, **case)
    L = _C.lib()
    a, b = c.plan._plan, plan32(c)._plan
    for f in (L.up_unipose_lstm_plan_workspace, L.up_unipose_lstm_plan_flip_workspace):
        assert 0 < f(a) < f(b), (f(a), f(b))
    need = {k: (L.up_unipose_lstm_plan_program_workspace(a, k), L.up_unipose_lstm_plan_program_workspace(b, k)) for k in PROGRAMS}
    print("program workspace bytes, bf16 / fp32:", need)
    for k, (n16, n32) in need.items():
        assert 0 < n16 < n32, (k, n16, n32)
    assert L.up_unipose_lstm_plan_program_workspace(a, 9) == 0 and L.up_unipose_lstm_plan_program_workspace(a, FF + 3) == 0
    assert L.up_unipose_lstm_plan_workspace(a) == max(need[k][0] for k in (0, 1, 2, 3, 6, 7, 8))
    assert L.up_unipose_lstm_plan_flip_workspace(a) == max(need[4][0], need[5][0])
    # the state is fp32 NHWC of rup4(K + 2) lanes in both storages
    h, w = c.plan.out_height, c.plan.out_width
    state = L.up_unipose_lstm_plan_state_bytes(a)
    assert state == L.up_unipose_lstm_plan_state_bytes(b) >= 2 * c.B * h * w * ops.rup4(c.K + 2) * 4
    s16, s32 = c.plan.stream_state(), plan32(c).stream_state()
    c.plan.stream(c.ctx.x[:, 0], c.ctx.cm[:, 0], s16, first=True)
    assert s16.numel() == s32.numel() == state and s16.dtype == s32.dtype == torch.uint8 and bool(s16.any())


# ---- 6. nothing stale is read ----------------------------------------------------------------------------------------------------------
def stale_case(dev, alloc=None, **case):
    """A workspace of EXACTLY the size the program reports (alloc(n): n bytes that end right before an inaccessible page), every byte
    0xFF — a NaN in both types — before a clip, a flip clip and two stream calls: the results are the earlier ones, so every pad
    lane the gate and head convolutions read is written in the call."""
    c = setup(dev, **case)
    L = _C.lib()
    plan, ctx, K = c.plan, c.ctx, c.K
    x, cm = ctx.xc.data_ptr(), ctx.cmc.data_ptr()

    def filled(k):
        n = L.up_unipose_lstm_plan_workspace(plan._plan) if k == 2 else L.up_unipose_lstm_plan_program_workspace(plan._plan, k)
        if alloc is not None:
            buf = alloc(n)
            off = 0
        else:
            buf = torch.empty(n + 256, dtype=torch.uint8, device=dev)
            off = (-buf.data_ptr()) % 256
        assert buf.dtype == torch.uint8 and (buf.data_ptr() + off) % 256 == 0
        buf.fill_(255)
        return buf, buf.data_ptr() + off, n

    heat, cell, hide = (torch.full_like(t, SENT) for t in (ctx.heats, ctx.cell, ctx.hide))
    buf, ws, n = filled(2)
    _C.check(L.up_unipose_lstm_clip(plan._plan, x, cm, heat.data_ptr(), cell.data_ptr(), hide.data_ptr(), ws, n, plan._stream()), "clip")
    for g, r, name in zip((heat, cell, hide), (ctx.heats, ctx.cell, ctx.hide), ("heat", "cell", "hide")):
        assert same(g, r), ("clip", name)
    flip = torch.full_like(ctx.heats, SENT)
    buf, ws, n = filled(4)
    _C.check(L.up_unipose_lstm_clip_flip(plan._plan, x, cm, ops._perm_array(ctx.perm, K + 1), flip.data_ptr(), ws, n, plan._stream()),
             "clip_flip")
    assert same(flip, ctx.merged.reshape(flip.shape))
    state = plan.stream_state()
    for j in range(2):
        heat = torch.full_like(ctx.steps[j], SENT)
        preds, mx = torch.full((c.B, K + 1, 2), SENT, device=dev), torch.full((c.B, K + 1, 1), SENT, device=dev)
        buf, ws, n = filled(7 + j)
        _C.check(L.up_unipose_lstm_stream_keypoints(plan._plan, ctx.x[:, j].contiguous().data_ptr(), ctx.cm[:, j].contiguous().data_ptr(),
                                                    state.data_ptr(), int(j == 0), ctx.h, ctx.w, None, preds.data_ptr(), mx.data_ptr(),
                                                    heat.data_ptr(), ws, n, plan._stream()), "stream_keypoints")
        assert same(heat, ctx.steps[j]), ("stream", j)
        want = ops.heatmap_decode(ctx.steps[j], None)
        assert same(preds, want[0]) and same(mx, want[1]), ("stream joints", j)
    del buf


# ---- 7. refresh ------------------------------------------------------------------------------------------------------------------------
def refresh_case(dev, **case):
    """a trunk weight and one part of each stacked gate weight changed: after refresh(model) the plan equals the changed module and
    no longer the old one.  (A plan of its own: the shared one keeps its weights.)"""
    from unipose_amd.plan import UniPoseLSTMPlan
    c = setup(dev, **case)
    plan = UniPoseLSTMPlan(c.model, c.B, c.H, c.W, frames=c.T, storage="bf16s")
    assert plan.storage == "bf16"
    assert same(plan.clip(c.ctx.xc, c.ctx.cmc)[0], c.ctx.heats)
    m2 = copy.deepcopy(c.model)
    with torch.no_grad():
        m2.backbone.layer1[0].conv2.weight.mul_(1.25)
        m2.lstm_0.conv_i_lstm.weight.mul_(0.5)
        m2.lstm.conv_oh_lstm.weight.mul_(-0.75)
        m2.lstm.conv_gx_lstm.bias.add_(0.125)
    plan.refresh(m2)
    got = plan.clip(c.ctx.xc, c.ctx.cmc)
    with bf16s():
        ref2 = lc.module_frames(lc.folded_copy(m2, True), c.ctx.xc, c.ctx.cmc, c.K, c.T)
    for j in range(c.T):
        lc._equal(got[0][:, j], ref2[j][0], f"refreshed heat {j}")
    lc._equal(got[1], ref2[c.T - 1][1], "refreshed cell")
    lc._equal(got[2], ref2[c.T - 1][2], "refreshed hide")
    assert not same(got[0], c.ctx.heats) and not same(got[2], c.ctx.hide)
    assert _C.lib().up_unipose_lstm_plan_dtype(plan._plan) == 1
    plan.close()


# ---- 8. coexistence --------------------------------------------------------------------------------------------------------------------
def coexistence_case(dev, image_case, **case):
    """plans of both storages of one model, alive together and called in turn; closing one leaves the other working; a bf16 image
    plan beside the bf16 video plan (plan_bf16_cases.setup(**image_case))"""
    from unipose_amd.plan import UniPoseLSTMPlan
    c = setup(dev, **case)
    assert ops.CONV_MATH == ops.MATH_F32
    xc, cmc = c.ctx.xc, c.ctx.cmc
    p32 = UniPoseLSTMPlan(c.model, c.B, c.H, c.W, frames=c.T)              # (one of its own, to be closed below)
    first32 = [t.clone() for t in p32.clip(xc, cmc)]
    for _ in range(2):
        for g, r in zip(c.plan.clip(xc, cmc), (c.ctx.heats, c.ctx.cell, c.ctx.hide)):
            assert same(g, r)
        for g, r in zip(p32.clip(xc, cmc), first32):
            assert same(g, r)
    assert ops.CONV_MATH == ops.MATH_F32 and not same(first32[0], c.ctx.heats)
    p32.close()
    assert same(c.plan.clip(xc, cmc)[0], c.ctx.heats)
    p16 = UniPoseLSTMPlan(c.model, c.B, c.H, c.W, frames=c.T, storage="bf16")
    assert same(p16.clip(xc, cmc)[0], c.ctx.heats)
    p16.close()
    assert same(plan32(c).clip(xc, cmc)[0], first32[0])
    ic = bc.setup(dev, **image_case)
    assert ic.plan.storage == "bf16" and same(bc.maps(ic.plan, ic.x), ic.ref)
    assert same(c.plan.clip(xc, cmc)[0], c.ctx.heats)
    assert same(bc.maps(ic.plan, ic.x), ic.ref)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def refusal_case(dev, **case):
    from unipose_amd.plan import UniPoseLSTMPlan, _LstmConfig
    c = setup(dev, **case)
    L = _C.lib()
    INVALID, WORKSPACE = -1, -4
    # the storage type, at create: *out stays what it was
    for bad in (2, -1):
        plan = C.c_void_p(12345)
        assert L.up_unipose_lstm_plan_create_t(C.byref(_LstmConfig(1, 2, 32, 32, 16, 13)), bad, C.byref(plan)) == INVALID
        assert L.up_last_error().decode() == f"unipose_lstm_plan_create: storage type {bad} (UP_DT_F32 or UP_DT_BF16)"
        assert plan.value == 12345
    assert L.up_unipose_lstm_plan_dtype(None) == INVALID
    for bad in ("fp16", "", None, 1):
        try:
            UniPoseLSTMPlan(None, c.B, c.H, c.W, frames=c.T, storage=bad)      # refused before the model is looked at
            raise AssertionError(f"storage={bad!r} must be refused")
        except ValueError:
            pass
    # the workspace, one byte short of what each entry asks for: the fp32 plan's code and words, nothing launched
    plan, ctx, K = c.plan, c.ctx, c.K
    ws0 = L.up_unipose_lstm_plan_workspace(plan._plan)
    need4 = L.up_unipose_lstm_plan_program_workspace(plan._plan, 4)
    buf = torch.empty(max(ws0, need4) + 256, dtype=torch.uint8, device=dev)
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    heat, cell, hide = (torch.full_like(t, SENT) for t in (ctx.heats, ctx.cell, ctx.hide))
    x, cm = ctx.xc.data_ptr(), ctx.cmc.data_ptr()
    n0 = bc._fp32_forward_launches()
    assert L.up_unipose_lstm_clip(plan._plan, x, cm, heat.data_ptr(), cell.data_ptr(), hide.data_ptr(), ws, ws0 - 1, 0) == WORKSPACE
    assert L.up_last_error().decode() == f"unipose_lstm_clip: workspace of {ws0} bytes (256-byte aligned) needed, got {ws0 - 1}"
    assert L.up_unipose_lstm_step(plan._plan, ctx.x[:, 0].contiguous().data_ptr(), ctx.cm[:, 0].contiguous().data_ptr(), None, None,
                                  heat.data_ptr(), cell.data_ptr(), hide.data_ptr(), ws, ws0 - 1, 0) == WORKSPACE
    assert L.up_unipose_lstm_clip_flip(plan._plan, x, cm, ops._perm_array(ctx.perm, K + 1), heat.data_ptr(), ws, need4 - 1, 0) == WORKSPACE
    assert L.up_last_error().decode() == f"unipose_lstm_clip_flip: workspace of {need4} bytes (256-byte aligned) needed, got {need4 - 1}"
    assert L.up_unipose_lstm_clip(plan._plan, x, cm, heat.data_ptr(), None, None, ws + 4, ws0 + 200, 0) == WORKSPACE
    assert bc._fp32_forward_launches() == n0
    for t in (heat, cell, hide):
        assert bool((t == SENT).all())
    # the argument checks of the fp32 files, on bf16 plans
    with bf16_plans():
        lc.argument_checks(dev, K=K, size=32)
    vc.plan_argument_case(ctx)
    vf.plan_argument_case(frame_ctx(c))


# ---- the emulator's cut --------------------------------------------------------------------------------------------------------------
# An emulated bf16 trunk costs seconds per image, so the emulator file runs the cases above in a lean form: every call of the plan is
# made once, straight through the C entry, in a 0xFF-filled workspace of EXACTLY the size the plan reports for it (alloc(n): n bytes
# that end right before an inaccessible page), and serves the forward, counter and stale-memory checks at once.  The whole sets
# (every program, refresh, coexistence) run on the GPU.
def _exact(L, plan, k, alloc):
    n = L.up_unipose_lstm_plan_workspace(plan._plan) if k < 3 else L.up_unipose_lstm_plan_program_workspace(plan._plan, k)
    buf = alloc(n)
    assert buf.dtype == torch.uint8 and buf.numel() == n and buf.data_ptr() % 256 == 0
    buf.fill_(255)
    return buf, n


def lean_setup(dev, alloc, K=13, B=1, T=2, H=32, W=32):
    """model, bf16 plan, inputs, ONE clip of the plan (with its fp32-launch count) and the module's whole-clip unroll under bf16s"""
    from unipose_amd.plan import UniPoseLSTMPlan
    key = ("lean", str(dev), K, B, T, H, W)
    if key in _CASES:
        return _CASES[key]
    L = _C.lib()
    c = Case()
    c.dev, c.K, c.B, c.T, c.H, c.W, c.alloc = dev, K, B, T, H, W, alloc
    c.model = lc.lstm_model(dev, K)
    c.x = vc.O.synth_input((B, T, 3, H, W), 15).to(dev)
    c.cm = vc.O.synth_input((B, T, 1, H, W), 16, "rand").to(dev)
    c.plan = plan = UniPoseLSTMPlan(c.model, B, H, W, frames=T, storage="bf16")
    c.h, c.w = plan.out_height, plan.out_width
    c.heats = torch.full((B, T, K + 1, c.h, c.w), SENT)
    c.cell, c.hide = torch.full((B, K + 2, c.h, c.w), SENT), torch.full((B, K + 2, c.h, c.w), SENT)
    buf, n = _exact(L, plan, 2, alloc)
    n0 = bc._fp32_forward_launches()
    _C.check(L.up_unipose_lstm_clip(plan._plan, c.x.data_ptr(), c.cm.data_ptr(), c.heats.data_ptr(), c.cell.data_ptr(), c.hide.data_ptr(),
                                    buf.data_ptr(), n, 0), "unipose_lstm_clip")
    c.clip_launches = bc._fp32_forward_launches() - n0
    c.folded_clip = lc.folded_copy(c.model, True)
    with bf16s():
        c.ref_clip = lc.module_frames(c.folded_clip, c.x, c.cm, K, T)
    c.perm = vc.protocol.flip_perm(None, K, False, PAIRS)
    c.plan32 = None
    _CASES[key] = c
    return c


def lean_forward_case(dev, alloc, **case):
    """tests 1, 3 and 6 for the clip program: equal bits to the module out of a 0xFF workspace of exactly workspace() bytes, and the
    fp32 forward launches of that call: 3 at K = 13, 3 + (T - 1) at K = 15"""
    c = lean_setup(dev, alloc, **case)
    assert c.plan.storage == "bf16" and _C.lib().up_unipose_lstm_plan_dtype(c.plan._plan) == 1
    for t in (c.heats, c.cell, c.hide):
        _fine(t)
    for j in range(c.T):
        lc._equal(c.heats[:, j], c.ref_clip[j][0], f"clip heat {j}")
    lc._equal(c.cell, c.ref_clip[c.T - 1][1], "clip last cell")
    lc._equal(c.hide, c.ref_clip[c.T - 1][2], "clip last hide")
    assert c.clip_launches == {13: 3, 15: 3 + (c.T - 1)}[c.K], c.clip_launches


def lean_step_stream_case(dev, alloc, **case):
    """programs 0, 1, 7, 8: step on frames 0 and 1 against the module's per-frame path, stream on the same frames against step +
    decode, every call in a 0xFF workspace of exactly its size"""
    c = lean_setup(dev, alloc, **case)
    L = _C.lib()
    plan, K, B = c.plan, c.K, c.B
    with bf16s():
        ref = lc.module_frames(lc.folded_copy(c.model, False), c.x, c.cm, K, 2)
    state = plan.stream_state()
    prev = (None, None)
    for j in range(2):
        xj, cj = c.x[:, j].contiguous(), c.cm[:, j].contiguous()
        got = [torch.full_like(r, SENT) for r in ref[j]]
        ph, pc = (None, None) if j == 0 else (prev[0].data_ptr(), prev[1].data_ptr())
        buf, n = _exact(L, plan, j, alloc)
        _C.check(L.up_unipose_lstm_step(plan._plan, xj.data_ptr(), cj.data_ptr(), ph, pc, got[0].data_ptr(), got[1].data_ptr(),
                                        got[2].data_ptr(), buf.data_ptr(), n, 0), "unipose_lstm_step")
        for g, r, name in zip(got, ref[j], ("heat", "cell", "hide")):
            _fine(g)
            lc._equal(g, r, f"step frame {j} {name}")
        prev = (got[2], got[1])
        heat = torch.full_like(got[0], SENT)
        preds, mx = torch.full((B, K + 1, 2), SENT), torch.full((B, K + 1, 1), SENT)
        buf, n = _exact(L, plan, 7 + j, alloc)
        _C.check(L.up_unipose_lstm_stream_keypoints(plan._plan, xj.data_ptr(), cj.data_ptr(), state.data_ptr(), int(j == 0), c.h, c.w, None,
                                                    preds.data_ptr(), mx.data_ptr(), heat.data_ptr(), buf.data_ptr(), n, 0),
                 "unipose_lstm_stream_keypoints")
        want = ops.heatmap_decode(got[0], None)
        assert same(heat, got[0]) and same(preds, want[0]) and same(mx, want[1]), ("stream", j)


def lean_flip_frames_case(dev, alloc, **case):
    """programs 4 and FROM_FRAMES + 2: the flip clip against ops.flip_merge of the clip and the clip of the mirrored inputs; the clip
    from 45 x 60 uint8 frames against the clip of ops.augment_image / ops.make_centermaps of the same crops"""
    import numpy as np
    c = lean_setup(dev, alloc, **case)
    L = _C.lib()
    plan, K, B, T, H, W = c.plan, c.K, c.B, c.T, c.H, c.W
    mirrored = plan.clip(torch.flip(c.x, [-1]), torch.flip(c.cm, [-1]))[0]
    merged = ops.flip_merge(c.heats.flatten(0, 1), mirrored.flatten(0, 1), c.perm).reshape(c.heats.shape)
    assert not same(merged, c.heats)
    got = torch.full_like(c.heats, SENT)
    buf, n = _exact(L, plan, 4, alloc)
    n0 = bc._fp32_forward_launches()
    _C.check(L.up_unipose_lstm_clip_flip(plan._plan, c.x.data_ptr(), c.cm.data_ptr(), ops._perm_array(c.perm, K + 1), got.data_ptr(),
                                         buf.data_ptr(), n, 0), "unipose_lstm_clip_flip")
    assert bc._fp32_forward_launches() - n0 == 2 * c.clip_launches
    assert same(got, merged)
    nn = B * T
    frames = torch.from_numpy(vf.fc.pixels_of((36, K), (3,) + vf.FRAME_HW + (3,), "u8")).to(dev)
    fo = np.array([(2 * i + 1) % 3 for i in range(nn)]).reshape(B, T)
    center = np.array([[30.0 + 3 * i, 22.0 - 2 * i] for i in range(nn)]).reshape(B, T, 2)
    scale = np.array([0.2 * (1 + 0.15 * i) for i in range(nn)]).reshape(B, T)
    cc = np.array([[W / 2 + 2.5 * i - 3, H / 2 - 1.75 * i + 2] for i in range(nn)]).reshape(B, T, 2)
    maps = vc.protocol.crop_maps(center.reshape(nn, 2), scale.reshape(nn), [H, W], 20).reshape(nn, 2, 3)
    xa = ops.augment_image(frames[torch.from_numpy(fo.reshape(-1)).to(dev)], maps, (H, W)).reshape(B, T, 3, H, W)
    cma = ops.make_centermaps(cc.reshape(nn, 2), H, W, 3.0, device=dev).reshape(B, T, 1, H, W)
    want = plan.clip(xa, cma)
    assert not same(want[0], c.heats)
    got = plan.clip_frame_heatmaps(frames, center, scale, frame_of=fo, rot=20, crop_center=cc)
    for g, r, name in zip(got, want, ("heat", "cell", "hide")):
        assert same(g, r), ("clip_frame_heatmaps", name)


def lean_differs_case(dev, alloc, **case):
    """tests 4 and 5: the fp32 plan and the module under f32 give other bits; every workspace figure is strictly smaller, the state
    as large"""
    from unipose_amd.plan import UniPoseLSTMPlan
    c = lean_setup(dev, alloc, **case)
    L = _C.lib()
    c.plan32 = p32 = UniPoseLSTMPlan(c.model, c.B, c.H, c.W, frames=c.T)
    assert p32.storage == "f32" and L.up_unipose_lstm_plan_dtype(p32._plan) == 0
    n0 = bc._fp32_forward_launches()
    heats32 = p32.clip(c.x, c.cm)[0]
    assert bc._fp32_forward_launches() - n0 >= c.clip_launches + TRUNK_CONVS
    _fine(heats32)
    assert not same(heats32, c.heats)
    ref32 = lc.module_frames(c.folded_clip, c.x, c.cm, c.K, c.T)                  # the module under f32: the fp32 plan's bits
    assert ops.CONV_MATH == ops.MATH_F32
    for j in range(c.T):
        lc._equal(heats32[:, j], ref32[j][0], f"fp32 clip heat {j}")
        assert not same(ref32[j][0], c.ref_clip[j][0])
    _figures(L, c.plan, p32)
    p32.close()


def _figures(L, plan16, plan32_):
    a, b = plan16._plan, plan32_._plan
    for f in (L.up_unipose_lstm_plan_workspace, L.up_unipose_lstm_plan_flip_workspace):
        assert 0 < f(a) < f(b), (f(a), f(b))
    for k in PROGRAMS:
        n16, n32 = L.up_unipose_lstm_plan_program_workspace(a, k), L.up_unipose_lstm_plan_program_workspace(b, k)
        assert 0 < n16 < n32, (k, n16, n32)
    assert L.up_unipose_lstm_plan_state_bytes(a) == L.up_unipose_lstm_plan_state_bytes(b) > 0
    s16, s32 = plan16.stream_state(), plan32_.stream_state()
    assert s16.numel() == s32.numel() and s16.dtype == s32.dtype == torch.uint8


def lean_refusal_case(dev, alloc, **case):
    """test 9 without a launch: create_t, storage=, plan_dtype(NULL), a workspace one byte short, the Python argument checks"""
    from unipose_amd.plan import UniPoseLSTMPlan, _LstmConfig
    c = lean_setup(dev, alloc, **case)
    L = _C.lib()
    for bad in (2, -1):
        plan = C.c_void_p(12345)
        assert L.up_unipose_lstm_plan_create_t(C.byref(_LstmConfig(1, 2, 32, 32, 16, 13)), bad, C.byref(plan)) == -1
        assert L.up_last_error().decode() == f"unipose_lstm_plan_create: storage type {bad} (UP_DT_F32 or UP_DT_BF16)"
        assert plan.value == 12345
    assert L.up_unipose_lstm_plan_dtype(None) == -1
    for bad in ("fp16", "", None, 1):
        try:
            UniPoseLSTMPlan(None, c.B, c.H, c.W, frames=c.T, storage=bad)
            raise AssertionError(f"storage={bad!r} must be refused")
        except ValueError:
            pass
    ws0 = L.up_unipose_lstm_plan_workspace(c.plan._plan)
    buf = alloc(ws0)
    heat, cell, hide = (torch.full_like(t, SENT) for t in (c.heats, c.cell, c.hide))
    n0 = bc._fp32_forward_launches()
    assert L.up_unipose_lstm_clip(c.plan._plan, c.x.data_ptr(), c.cm.data_ptr(), heat.data_ptr(), cell.data_ptr(), hide.data_ptr(),
                                  buf.data_ptr(), ws0 - 1, 0) == -4
    assert L.up_last_error().decode() == f"unipose_lstm_clip: workspace of {ws0} bytes (256-byte aligned) needed, got {ws0 - 1}"
    assert bc._fp32_forward_launches() == n0
    for t in (heat, cell, hide):
        assert bool((t == SENT).all())
    with bf16_plans():
        lc.argument_checks(dev, K=c.K, size=32)
