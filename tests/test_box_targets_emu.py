"""Training targets of the box head and the bbox=True model in train mode (box_target_cases.py) on a GPU-less box: the HIP sources
compiled against the fiber emulator (tests/emu).  The cases and rules are those of test_box_targets_gpu.py, less its batch of more
than 2^21 output pixels; its docstring lists what both platforms measured.  The first test needs no device at all."""
import pytest

import box_target_cases as bx

SIZE_IDS = ["%dx%d_s%g" % s for s in bx.SIZES]


def test_restatement_equals_reference(golden_dir):
    bx.restatement_case(golden_dir)


def test_entry_equals_reference(emu_backend, golden_dir):
    bx.golden_case(emu_backend, golden_dir)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("k", bx.KS)
@pytest.mark.parametrize("size", bx.SIZES, ids=SIZE_IDS)
def test_entry_equals_restatement(emu_backend, size, k, b):
    bx.shape_case(emu_backend, size, k, b)


def test_failing_sample_in_the_middle(emu_backend):
    bx.middle_failure_case(emu_backend)


def test_other_sigmas(emu_backend):
    bx.sigma_case(emu_backend)


def test_round_trip_with_the_decoder(emu_backend):
    bx.roundtrip_case(emu_backend)


def test_refusals(emu_backend):
    bx.refusal_case(emu_backend)


def test_empty_sample_policy(emu_backend):
    bx.empty_policy_case(emu_backend)


def test_bbox_model_train_step_vs_oracle(emu_backend):
    bx.bbox_train_case(emu_backend)


def test_batcher_box_maps(emu_backend):
    bx.batcher_case(emu_backend)


def test_trainer_with_box_head(emu_backend, monkeypatch):
    monkeypatch.setenv("UNIPOSE_NO_TQDM", "1")
    bx.trainer_case(emu_backend)


def test_zz_report(emu_backend):
    print("\n" + bx.report() + " (emulator)")
    assert bx.WORST["flipped"] == 0
