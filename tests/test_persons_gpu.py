"""up_persons_decode and up_unipose_persons on the MI355X (tests/persons_cases.py)."""
import pytest
import torch

import persons_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", pc.G9_CASES)
def test_g9_through_the_batch_decode(golden_dir, name):
    pc.g9_case(DEV, golden_dir, name)


def test_one_batch_mixed_outcomes_nchw_and_nhwc(golden_dir):
    pc.mixed_batch_case(DEV, golden_dir)


def test_order_across_wave_and_chunk_boundaries():
    pc.order_case(DEV)


def test_error_order():
    pc.error_order_case(DEV)


def test_random_scenes():
    pc.random_scenes_case(DEV)


def test_edges():
    pc.edges_case(DEV)


@pytest.mark.parametrize("batch", [1, 2])
def test_plan_persons_equals_decode_of_the_maps(batch):
    pc.plan_case(DEV, batch)


def test_python_argument_checks():
    pc.python_argument_case(DEV)


def test_c_abi_argument_checks():
    pc.c_abi_checks(DEV)
