"""The evaluation protocol around the forward (protocol_cases.py) on a GPU-less box: the HIP sources compiled against the fiber
emulator (tests/emu).  The first three tests need no device.  up_final_preds reads its maps from tensors that end right in front
of an inaccessible page (tests/emu/guard_alloc.py), so a read past a map's end faults — also at the (shape, res) combinations
where the reference raises IndexError."""
import pytest

import protocol_cases as pc


def _guard():
    from guard_alloc import guarded          # tests/emu is on the path once emu_backend has run
    return guarded


def test_flip_perm_lists():
    pc.flip_perm_case()


def test_transforms_equal_reference(golden_dir):
    pc.transform_case(golden_dir)


def test_restatement_equals_reference(golden_dir):
    pc.restatement_case(golden_dir)


def test_final_preds_equals_reference_emu(emu_backend, golden_dir):
    pc.final_golden_case(emu_backend, golden_dir, _guard())


def test_final_preds_variants_emu(emu_backend):
    pc.final_variants_case(emu_backend, _guard())


def test_final_preds_refusals_emu(emu_backend):
    pc.final_refusal_case(emu_backend)


def test_flip_merge_equals_numpy_emu(emu_backend):
    pc.merge_case(emu_backend)


def test_flip_merge_equals_flip_back_emu(emu_backend, golden_dir):
    pc.merge_golden_case(emu_backend, golden_dir)


def test_flip_merge_refusals_emu(emu_backend):
    pc.merge_refusal_case(emu_backend)


def test_layout_pass_with_mirror_emu(emu_backend):
    pc.layout_flip_case(emu_backend)


def test_semantics_emu(emu_backend):
    pc.semantics_case(emu_backend)


@pytest.mark.parametrize("case", pc.PLAN_CASES_EMU, ids=pc.plan_id)
def test_plan_flip_and_final_preds_emu(emu_backend, case):
    pc.plan_case(emu_backend, **case)


def test_plan_unset_weights_refused_emu(emu_backend):
    pc.plan_unset_case(emu_backend)


def test_trainer_flip_test_emu(emu_backend, monkeypatch):
    monkeypatch.setenv("UNIPOSE_NO_TQDM", "1")
    pc.trainer_case(emu_backend)
