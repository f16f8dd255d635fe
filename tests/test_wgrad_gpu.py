"""The weight-gradient entries alone against float64 (wgrad_cases.py), on a real MI355X.

The 109 tests of this file take about 3.5 s on the GPU (the slowest 1.1 s: the first one, which also loads the library; every
other one below 0.05 s) and about 12 s on the emulator, which runs the same cases.  Worst got / bound ratios per case group of the
GPU run: profiles/wgrad_tests.txt (a record of head-room, not a tolerance; the bound is the formula in wgrad_cases.py).  The
first runs found no kernel fault; they found that the bias gradient's workspace was tested after the weight gradient had been
launched (refusal_case fails on the commit before the fix: "the refused call wrote dw, dbias or the workspace") and that the
one-stage forms of the 64x64 tile cannot be reached (wgrad_cases.py).

Seeded faults (emulator only, in a scratch copy of the tree; each is a one-line change, -> the tests of test_wgrad_emu.py that
fail; a test id is test_<name>[<case>]):
    wgrad_reduce_kernel: kadd1 without the compensation (sum += a)     -> merge_stays_compensated[both orders in which the plain sum is 6, glds32 and reg]
                                                                           (and nothing else: the a-priori bound allows an uncompensated merge of nine slabs)
    wgrad_reduce_kernel: the last split is never added                 -> 48 tests: every case with more than one split (pixel_counts, split_counts[2 .. 9],
                                                                           nine_splits_of_48x48, merge_stays_compensated, live_rectangles[wasp_*],
                                                                           empty_split_domains, bias_gradient (its 257-pixel shape), unaligned[1x1_1025_pixels],
                                                                           one_stage_64x64)
    wgrad_glds32_kernel: return before the slab store when nsl == 0    -> live_rectangles[wasp_c128_one_tap_per_tile-glds32, dil5_on_4x4_empty_rectangles-glds32],
                                                                           empty_split_domains_write_zero_slabs[glds32]
"""
import pytest
import torch

import wgrad_cases as wx

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("tf", wx.TILE_RUNS, ids=wx.run_id)
def test_tile_pairs_in_every_family(tf):
    wx.tile_case(DEV, *tf)


def test_one_stage_64x64_is_unreachable():
    wx.one_stage_64x64_case(DEV)


@pytest.mark.parametrize("fam", wx.ALL5)
def test_pixel_counts(fam):
    wx.pixel_case(DEV, fam)


@pytest.mark.parametrize("s", wx.SPLIT_COUNTS)
def test_split_counts(s):
    wx.split_case(DEV, s, "glds32")


@pytest.mark.parametrize("fam", ("reg", "bf16op", "bf16s_glds", "bf16s_reg"))
def test_nine_splits_of_48x48(fam):
    wx.split_case(DEV, 9, fam, square=True)


@pytest.mark.parametrize("fam", ("glds32", "reg"))
@pytest.mark.parametrize("order", list(wx.KAHAN_ORDERS), ids=lambda o: o.replace(" ", "_"))
def test_merge_stays_compensated(order, fam):
    wx.kahan_case(DEV, order, fam)


@pytest.mark.parametrize("tf", wx.RECT_RUNS, ids=wx.run_id)
def test_live_rectangles(tf):
    wx.rect_case(DEV, *tf)


@pytest.mark.parametrize("fam", wx.ALL5)
def test_no_rectangle_table_for_unpadded_1x1(fam):
    wx.no_table_case(DEV, fam)


@pytest.mark.parametrize("fam", wx.ALL5)
def test_empty_split_domains_write_zero_slabs(fam):
    wx.empty_domain_case(DEV, fam)


@pytest.mark.parametrize("fam", ("glds32", "bf16s_glds"))
@pytest.mark.parametrize("k", wx.BIAS_K)
def test_bias_gradient(k, fam):
    wx.bias_case(DEV, k, fam)


@pytest.mark.parametrize("fam", ("glds32", "bf16s_glds"))
def test_bias_gradient_65_partial_rows(fam):
    wx.bias_big_case(DEV, fam)


@pytest.mark.parametrize("fam", ("glds32", "bf16op", "bf16s_glds"))
def test_null_dbias_launches_nothing(fam):
    wx.no_bias_case(DEV, fam)


@pytest.mark.parametrize("fam", list(wx.UNALIGNED_FALLBACK))
@pytest.mark.parametrize("t", wx.UNALIGNED, ids=lambda t: t[0])
def test_unaligned_operands_fall_back(t, fam):
    wx.unaligned_case(DEV, t, fam)


def test_older_entries_equal_acc():
    wx.entries_case(DEV)


def test_refusals_leave_everything_untouched():
    wx.refusal_case(DEV)
