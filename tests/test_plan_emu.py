"""up_unipose_forward (whole-graph inference entry, C ABI 9) on the CPU emulator: equal bits to the module's folded forward."""
import plan_cases as pc


def test_plan_forward_equals_folded_module_emu(emu_backend):
    pc.plan_case(emu_backend, K=14, B=1, size=64)


def test_plan_forward_size_not_a_multiple_of_8_emu(emu_backend):
    """52 x 52 gives ceil(52 / 8) = 7 x 7 heat-maps; the plan used to allocate 6 x 6 and write past the end"""
    out = pc.plan_case(emu_backend, K=14, B=1, size=52)
    assert out.shape[-2:] == (7, 7)


def test_plan_forward_output_stride_8_and_box_head_emu(emu_backend):
    pc.plan_case(emu_backend, K=16, B=2, size=48, output_stride=8, bbox=True)


def test_plan_argument_checks(emu_backend):
    import ctypes as C
    from unipose_amd import _C
    from unipose_amd.plan import _Config
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_plan_create(C.byref(_Config(1, 64, 64, 32, 15)), C.byref(plan)) != 0      # output stride 32: not built
    assert b"output stride" in L.up_last_error()
    assert L.up_unipose_plan_create(C.byref(_Config(1, 64, 64, 16, 15)), C.byref(plan)) == 0
    n = L.up_unipose_plan_num_convs(plan)
    names = [L.up_unipose_plan_conv_name(plan, i).decode() for i in range(n)]
    assert n == 116 and names[0] == "backbone.conv1" and names[-1] == "decoder.last_conv.8"       # 115 parameters, wasp.conv2 twice
    assert names.count("wasp.conv2") == 2 and len(set(names)) == 115
    assert L.up_unipose_plan_workspace(plan) > 0
    import torch
    buf = torch.zeros(1024)
    assert L.up_unipose_forward(plan, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1 << 40, 0) != 0   # weights never set
    assert b"never set" in L.up_last_error()
    L.up_unipose_plan_destroy(plan)


# Program numbers, workspace figures and refusals of both plans as the commit before the one that put them on one program
# table, one weight store and one call path gave them (58f581e, read from it; never from the code under test).
# (batch, height, width, output_stride, out_channels) -> programs 0..6, and from frames programs +4 / +5; +0 and +6 equal 0..6
_IMAGE_WS = {(1, 64, 64, 16, 15): (868352, 933888), (2, 52, 68, 8, 22): (3563776, 3676928), (1, 368, 368, 16, 17): (28709888, 30876672)}
# (batch, frames, height, width, output_stride, num_classes) -> programs 0..8, workspace(), flip_workspace(), state_bytes()
_VIDEO_WS = {
    (1, 1, 64, 64, 16, 13): ((868352,) * 9, 868352, 868352, 8192),
    (2, 3, 32, 40, 16, 13): ((542720,) * 2 + (1628160,) * 5 + (542720,) * 2, 1628160, 1628160, 5120),
    (1, 2, 39, 39, 16, 15): ((357376, 357376, 714496, 714496, 919296, 919296, 714496, 357376, 357376), 714496, 919296, 4096),   # (K + 1) % 4 == 0
    (1, 2, 64, 72, 8, 13): ((2451456,) * 2 + (4902912,) * 5 + (2451456,) * 2, 4902912, 4902912, 9216),
    (1, 5, 368, 368, 16, 13): ((28709888,) * 2 + (143549440,) * 5 + (28709888,) * 2, 143549440, 143549440, 270848),
}


def test_plan_programs_workspaces_and_refusals(emu_backend):
    import ctypes as C
    import torch
    import lstm_plan_cases as lc
    from unipose_amd import _C
    from unipose_amd.plan import UniPoseLSTMPlan, UniPosePlan, _Config, _LstmConfig
    L = _C.lib()
    FF = _C.PROGRAM_FROM_FRAMES
    buf = torch.zeros(1 << 16)
    p = buf.data_ptr()
    big = 1 << 40

    def refused(rc, code, text):
        assert (rc, L.up_last_error().decode()) == (code, text)

    # (a) numbering and workspace figures
    for cfg, (need, flip_frames) in _IMAGE_WS.items():
        plan = C.c_void_p()
        assert L.up_unipose_plan_create(C.byref(_Config(*cfg)), C.byref(plan)) == 0
        assert L.up_unipose_plan_num_convs(plan) == 116
        assert [L.up_unipose_plan_program_workspace(plan, k) for k in range(8)] == [need] * 7 + [0], cfg
        assert [L.up_unipose_plan_program_workspace(plan, FF + k) for k in range(8)] == \
            [need, 0, 0, 0, flip_frames, flip_frames, need, 0], cfg
        assert (L.up_unipose_plan_workspace(plan), L.up_unipose_plan_flip_workspace(plan)) == (need, need), cfg
        if cfg != (1, 64, 64, 16, 15):
            L.up_unipose_plan_destroy(plan)
            continue
        # (b) one refusal per shared helper, all before the weights are looked at
        bad = (C.c_int32 * 15)(*range(14), 15)
        refused(L.up_unipose_forward(plan, p, p, p, big, 0), -1,
                "unipose_forward: weights of backbone.conv1 were never set (up_unipose_plan_set_conv)")
        refused(L.up_unipose_flip_forward(plan, p, bad, p, p, 0, 0), -1, "unipose_flip_forward: perm[14] = 15 outside 0..14")
        refused(L.up_unipose_keypoints(plan, p, 9, 8, None, p, p, p, 0, 0), -1,
                "unipose_keypoints: a 9 x 8 grid; the plan decodes on the heat-maps' 8 x 8 or the input's 64 x 64")
        refused(L.up_unipose_forward(plan, None, p, p, big, 0), -1, "unipose_forward: null argument")
        L.up_unipose_plan_destroy(plan)
    for cfg, (programs, ws, flip_ws, state) in _VIDEO_WS.items():
        plan = C.c_void_p()
        assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(*cfg)), C.byref(plan)) == 0
        assert L.up_unipose_lstm_plan_num_convs(plan) == 132
        assert tuple(L.up_unipose_lstm_plan_program_workspace(plan, k) for k in range(10)) == programs + (0,), cfg
        assert (L.up_unipose_lstm_plan_workspace(plan), L.up_unipose_lstm_plan_flip_workspace(plan),
                L.up_unipose_lstm_plan_state_bytes(plan)) == (ws, flip_ws, state), cfg
        if cfg == (1, 1, 64, 64, 16, 13):
            bad = (C.c_int32 * 14)(-1, *range(1, 14))
            refused(L.up_unipose_lstm_clip(plan, p, p, p, None, None, p, big, 0), -1,
                    "unipose_lstm_clip: weights of backbone.conv1 were never set (up_unipose_lstm_plan_set_conv)")
            refused(L.up_unipose_lstm_clip_flip(plan, p, p, bad, p, p, 0, 0), -1, "unipose_lstm_clip_flip: perm[0] = -1 outside 0..13")
            refused(L.up_unipose_lstm_clip_keypoints(plan, p, p, 8, 9, None, p, p, None, None, p, 0, 0), -1,
                    "unipose_lstm_clip_keypoints: a 8 x 9 grid; the plan decodes on the heat-maps' 8 x 8 or the input's 64 x 64")
            refused(L.up_unipose_lstm_clip(plan, p, p, None, None, None, p, big, 0), -1, "unipose_lstm_clip: null argument")
        L.up_unipose_lstm_plan_destroy(plan)

    # a workspace one byte too small, with the weights set: UP_ERR_INVALID from the image plan, UP_ERR_WORKSPACE from the video plan
    aligned = p + (-p) % 256
    m = pc.mc.skeleton("image", 14)
    m.load_state_dict(pc.O.synth_state_dict(14, 1))
    plan = UniPosePlan(m.to(emu_backend).eval(), 1, 52, 52)
    refused(L.up_unipose_forward(plan._plan, p, p, aligned, 704512 - 1, 0), -1,
            "unipose_forward: workspace of 704512 bytes (256-byte aligned) needed, got 704511")
    plan.close()
    plan = UniPoseLSTMPlan(lc.lstm_model(emu_backend, 13), 1, 32, 32, frames=2)
    refused(L.up_unipose_lstm_clip(plan._plan, p, p, p, None, None, aligned, 434176 - 1, 0), -4,
            "unipose_lstm_clip: workspace of 434176 bytes (256-byte aligned) needed, got 434175")
    plan.close()
