"""up_unipose_lstm_step / up_unipose_lstm_clip (UniPose-LSTM inference entry, C ABI 10 additions) on the CPU emulator: equal bits to
the folded module's per-frame path and whole-clip unroll."""
import ctypes as C

import torch

import lstm_plan_cases as lc


def test_lstm_plan_step_and_clip_equal_folded_module_emu(emu_backend):
    lc.lstm_plan_case(emu_backend, K=13, B=1, size=32, T=2)


def test_lstm_plan_widened_hand_over_emu(emu_backend):
    """K = 15: (K + 1) % 4 == 0, no spare pad channel for the centre map: the hand-over tensor grows to rup4(K + 2) channels"""
    lc.lstm_plan_case(emu_backend, K=15, B=2, size=39, T=2, unfolded=False)


def test_lstm_plan_output_stride_8_emu(emu_backend):
    from unipose_amd.plan import UniPoseLSTMPlan
    m = lc.mc.skeleton("lstm", 13, output_stride=8)
    m.load_state_dict(lc.O.synth_state_dict(13, 4, lstm=True))
    m = m.to(emu_backend).eval()
    x = lc.O.synth_input((1, 2, 3, 32, 32), 15)
    cm = lc.O.synth_input((1, 2, 1, 32, 32), 16, "rand")
    plan = UniPoseLSTMPlan(m, 1, 32, 32, frames=2)
    ref = lc.module_frames(lc.folded_copy(m, True), x, cm, 13, 2)
    heats, cell, hide = plan.clip(x, cm)
    for j in range(2):
        lc._equal(heats[:, j], ref[j][0], f"heat {j}")
    lc._equal(hide, ref[1][2], "hide")
    plan.close()


def test_lstm_plan_argument_checks_emu(emu_backend):
    lc.argument_checks(emu_backend)


def test_lstm_plan_c_abi_checks(emu_backend):
    from unipose_amd import _C
    from unipose_amd.plan import _LstmConfig
    L = _C.lib()
    plan = C.c_void_p()
    assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(1, 2, 64, 64, 32, 13)), C.byref(plan)) != 0   # output stride 32
    assert b"output stride" in L.up_last_error()
    # 52 x 52: ceil(52 / 8) = 7 x 7 heat-maps, (52 - 7) / 8 + 1 = 6 x 6 pooled centre maps (the module's cat fails there too)
    assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(1, 2, 52, 52, 16, 13)), C.byref(plan)) != 0
    assert b"52x52" in L.up_last_error()
    assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(1, 2, 55, 56, 16, 13)), C.byref(plan)) == 0   # 55 % 8 == 7: accepted
    L.up_unipose_lstm_plan_destroy(plan)
    assert L.up_unipose_lstm_plan_create(C.byref(_LstmConfig(1, 2, 64, 64, 16, 13)), C.byref(plan)) == 0
    n = L.up_unipose_lstm_plan_num_convs(plan)
    names = [L.up_unipose_lstm_plan_conv_name(plan, i).decode() for i in range(n)]
    # the image trunk's 116 (wasp.conv2 twice), 3 + 8 gate parts, the five head convolutions
    assert n == 116 + 11 + 5 and names[0] == "backbone.conv1" and names[-1] == "conv5"
    assert names.count("wasp.conv2") == 2 and len(set(names)) == n - 1
    assert names[116:127] == ["lstm_0.conv_g_lstm", "lstm_0.conv_i_lstm", "lstm_0.conv_o_lstm"] + \
        [f"lstm.conv_{g}{p}_lstm" for p in "xh" for g in "giof"]
    assert names[127:] == [f"conv{i}" for i in range(1, 6)]
    shape, hb = (C.c_int32 * 4)(), C.c_int32()
    assert L.up_unipose_lstm_plan_conv_shape(plan, names.index("wasp.global_avg_pool.1"), shape, C.byref(hb)) == 0
    assert tuple(shape) == (256, 2048, 1, 1) and hb.value == 0                     # the video WASP: no BatchNorm, no bias
    assert L.up_unipose_lstm_plan_conv_shape(plan, names.index("lstm.conv_fh_lstm"), shape, C.byref(hb)) == 0
    assert tuple(shape) == (15, 15, 3, 3) and hb.value == 1
    assert L.up_unipose_lstm_plan_conv_shape(plan, names.index("conv1"), shape, C.byref(hb)) == 0
    assert tuple(shape) == (128, 15, 11, 11) and hb.value == 1
    ws = L.up_unipose_lstm_plan_workspace(plan)
    assert ws > 0
    buf = torch.zeros(1 << 16)
    p = buf.data_ptr()
    assert L.up_unipose_lstm_clip(plan, p, p, p, None, None, p, 1 << 40, 0) != 0                  # weights never set
    assert b"never set" in L.up_last_error()
    assert L.up_unipose_lstm_step(plan, p, p, None, None, p, p, p, p, 1 << 40, 0) != 0
    assert b"never set" in L.up_last_error()
    assert L.up_unipose_lstm_step(plan, p, p, p, None, p, p, p, p, 1 << 40, 0) != 0               # half a state
    # every convolution set (zeros): the workspace check is next
    for i in range(n):
        assert L.up_unipose_lstm_plan_conv_shape(plan, i, shape, C.byref(hb)) == 0
        w = torch.zeros(tuple(shape))
        b = torch.zeros(shape[0])
        assert L.up_unipose_lstm_plan_set_conv(plan, i, w.data_ptr(), b.data_ptr() if hb.value else None, 0) == 0, names[i]
    gap = names.index("wasp.global_avg_pool.1")
    assert L.up_unipose_lstm_plan_set_conv(plan, gap, buf.data_ptr(), buf.data_ptr(), 0) != 0        # a bias the conv has not
    aligned = p + (-p) % 256
    assert L.up_unipose_lstm_clip(plan, p, p, p, None, None, aligned, ws - 256, 0) != 0            # too small a workspace
    assert b"workspace" in L.up_last_error()
    L.up_unipose_lstm_plan_destroy(plan)
