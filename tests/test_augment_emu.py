"""Augmentation on the device (augment_cases.py) on a GPU-less box: the HIP sources compiled against the fiber emulator (tests/emu).
The cases and rules are those of test_augment_gpu.py, less its launch of more than 2^21 output pixels; here every source image
additionally sits right in front of an inaccessible page (tests/emu/guard_alloc.py), so a tap read past its end faults.  The first
test needs no device.  The fixture G20 holds the reference's point arithmetic and its numpy image steps (crop, hflip, normalize);
nothing of the reference's image resampling could be recorded, because OpenCV is absent where the fixture is made."""
import pytest

import augment_cases as ac


def _guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return guarded


def test_restatement_equals_reference(golden_dir):
    ac.restatement_case(golden_dir)


def test_entry_equals_reference(emu_backend, golden_dir):
    ac.golden_case(emu_backend, golden_dir, _guard())


def test_identity_equals_normalize(emu_backend):
    ac.identity_case(emu_backend, _guard())


@pytest.mark.parametrize("case", ac.CASES, ids=ac.CASE_IDS)
def test_entry_equals_float64(emu_backend, case):
    ac.float64_case(emu_backend, case, _guard())


def test_cases_sample_the_source(emu_backend):
    ac.coverage_case(emu_backend)


def test_all_taps_outside_and_huge_coordinates(emu_backend):
    ac.outside_case(emu_backend, _guard())


def test_padding_is_never_read(emu_backend):
    ac.padding_case(emu_backend, _guard())


def test_points_follow_pixels(emu_backend):
    ac.follow_case(emu_backend)


def test_refusals(emu_backend):
    ac.refusal_case(emu_backend)


@pytest.mark.parametrize("bbox", [False, True], ids=["plain", "bbox"])
def test_batcher_augment(emu_backend, bbox):
    ac.batcher_case(emu_backend, bbox)


def test_batcher_augment_clip(emu_backend):
    ac.clip_case(emu_backend)


def test_trainer_with_augment(emu_backend, monkeypatch):
    monkeypatch.setenv("UNIPOSE_NO_TQDM", "1")
    ac.trainer_case(emu_backend)


def test_zz_report(emu_backend):
    print("\n" + ac.report() + " (emulator)")
    assert ac.WORST["elements"] > 0 and ac.WORST["ratio"] <= 1.0
