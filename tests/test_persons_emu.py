"""up_persons_decode and up_unipose_persons on the CPU emulator (tests/persons_cases.py)."""
import pytest

import persons_cases as pc


@pytest.mark.parametrize("name", pc.G9_CASES)
def test_g9_through_the_batch_decode_emu(emu_backend, golden_dir, name):
    pc.g9_case(emu_backend, golden_dir, name)


def test_one_batch_mixed_outcomes_nchw_and_nhwc_emu(emu_backend, golden_dir):
    pc.mixed_batch_case(emu_backend, golden_dir)


def test_order_across_wave_and_chunk_boundaries_emu(emu_backend):
    pc.order_case(emu_backend)


def test_error_order_emu(emu_backend):
    pc.error_order_case(emu_backend)


def test_random_scenes_emu(emu_backend):
    pc.random_scenes_case(emu_backend)


def test_edges_emu(emu_backend):
    pc.edges_case(emu_backend)


@pytest.mark.parametrize("batch", [1, 2])
def test_plan_persons_equals_decode_of_the_maps_emu(emu_backend, batch):
    pc.plan_case(emu_backend, batch)


def test_python_argument_checks_emu(emu_backend):
    pc.python_argument_case(emu_backend)


def test_c_abi_argument_checks_emu(emu_backend):
    pc.c_abi_checks(emu_backend)
