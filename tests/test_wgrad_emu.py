"""The weight-gradient entries alone against float64 (wgrad_cases.py) on a GPU-less box: the HIP sources compiled against the fiber
emulator (tests/emu).  Bounds, cases and kernel-form proofs are those of test_wgrad_gpu.py (its docstring lists the seeded faults
these tests catch).  The emulator runs these small shapes fast enough that nothing is cut: the same cases, shapes and
parametrisation as on the GPU.  x, dy and the workspace of every launch end in front of an inaccessible page (guard_pages)."""
import pytest

import wgrad_cases as wx
from test_ops_emu import guard_pages      # noqa: F401  (the fixture)


@pytest.mark.parametrize("tf", wx.TILE_RUNS, ids=wx.run_id)
def test_tile_pairs_in_every_family(guard_pages, tf):
    wx.tile_case(wx.torch.device("cpu"), *tf, guard=guard_pages)


def test_one_stage_64x64_is_unreachable(guard_pages):
    wx.one_stage_64x64_case(wx.torch.device("cpu"), guard=guard_pages)


@pytest.mark.parametrize("fam", wx.ALL5)
def test_pixel_counts(guard_pages, fam):
    wx.pixel_case(wx.torch.device("cpu"), fam, guard=guard_pages)


@pytest.mark.parametrize("s", wx.SPLIT_COUNTS)
def test_split_counts(guard_pages, s):
    wx.split_case(wx.torch.device("cpu"), s, "glds32", guard=guard_pages)


@pytest.mark.parametrize("fam", ("reg", "bf16op", "bf16s_glds", "bf16s_reg"))
def test_nine_splits_of_48x48(guard_pages, fam):
    wx.split_case(wx.torch.device("cpu"), 9, fam, guard=guard_pages, square=True)


@pytest.mark.parametrize("fam", ("glds32", "reg"))
@pytest.mark.parametrize("order", list(wx.KAHAN_ORDERS), ids=lambda o: o.replace(" ", "_"))
def test_merge_stays_compensated(guard_pages, order, fam):
    wx.kahan_case(wx.torch.device("cpu"), order, fam, guard=guard_pages)


@pytest.mark.parametrize("tf", wx.RECT_RUNS, ids=wx.run_id)
def test_live_rectangles(guard_pages, tf):
    wx.rect_case(wx.torch.device("cpu"), *tf, guard=guard_pages)


@pytest.mark.parametrize("fam", wx.ALL5)
def test_no_rectangle_table_for_unpadded_1x1(guard_pages, fam):
    wx.no_table_case(wx.torch.device("cpu"), fam, guard=guard_pages)


@pytest.mark.parametrize("fam", wx.ALL5)
def test_empty_split_domains_write_zero_slabs(guard_pages, fam):
    wx.empty_domain_case(wx.torch.device("cpu"), fam, guard=guard_pages)


@pytest.mark.parametrize("fam", ("glds32", "bf16s_glds"))
@pytest.mark.parametrize("k", wx.BIAS_K)
def test_bias_gradient(guard_pages, k, fam):
    wx.bias_case(wx.torch.device("cpu"), k, fam, guard=guard_pages)


@pytest.mark.parametrize("fam", ("glds32", "bf16s_glds"))
def test_bias_gradient_65_partial_rows(guard_pages, fam):
    wx.bias_big_case(wx.torch.device("cpu"), fam, guard=guard_pages)


@pytest.mark.parametrize("fam", ("glds32", "bf16op", "bf16s_glds"))
def test_null_dbias_launches_nothing(guard_pages, fam):
    wx.no_bias_case(wx.torch.device("cpu"), fam, guard=guard_pages)


@pytest.mark.parametrize("fam", list(wx.UNALIGNED_FALLBACK))
@pytest.mark.parametrize("t", wx.UNALIGNED, ids=lambda t: t[0])
def test_unaligned_operands_fall_back(guard_pages, t, fam):
    wx.unaligned_case(wx.torch.device("cpu"), t, fam, guard=guard_pages)


def test_older_entries_equal_acc(guard_pages):
    wx.entries_case(wx.torch.device("cpu"), guard=guard_pages)


def test_refusals_leave_everything_untouched(guard_pages):
    wx.refusal_case(wx.torch.device("cpu"), guard=guard_pages)
