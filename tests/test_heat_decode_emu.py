"""up_heatmap_decode, up_unipose_forward_upsampled and up_unipose_keypoints on the CPU emulator (tests/heat_decode_cases.py)."""
import heat_decode_cases as hc


def test_decode_identity_size_equals_argmax_emu(emu_backend, golden_dir):
    hc.identity_case(emu_backend, golden_dir)


def test_decode_upsampled_equals_composition_emu(emu_backend):
    """LDS path at three sizes and the global-memory path, from NCHW and NHWC: no tolerance"""
    hc.upsampled_case(emu_backend, maps=(2, 5), maps_beyond_lds=(1, 2))


def test_decode_planted_ties_nan_negative_emu(emu_backend):
    hc.planted_case(emu_backend)


def test_decode_full_resolution_vs_reference_golden_emu(emu_backend, golden_dir):
    hc.reference_case(emu_backend, golden_dir)


def test_plan_stride_1_equals_folded_module_emu(emu_backend):
    out = hc.plan_upsampled_case(emu_backend, K=14, B=1, size=64)
    assert out.shape == (1, 15, 64, 64)


def test_plan_stride_1_size_not_a_multiple_of_8_emu(emu_backend):
    """52 x 52 -> 7 x 7 maps -> 52 x 52"""
    out = hc.plan_upsampled_case(emu_backend, K=14, B=1, size=52)
    assert out.shape == (1, 15, 52, 52)


def test_plan_stride_1_output_stride_8_and_box_head_emu(emu_backend):
    out = hc.plan_upsampled_case(emu_backend, K=16, B=2, size=48, output_stride=8, bbox=True)
    assert out.shape == (2, 22, 48, 48)


def test_plan_keypoints_equal_argmax_of_heatmaps_emu(emu_backend):
    hc.plan_keypoints_case(emu_backend)


def test_keypoints_c_abi_checks(emu_backend):
    hc.keypoints_c_abi_checks(emu_backend)


def test_video_heatmaps_decode_emu(emu_backend):
    hc.video_case(emu_backend)
