"""Many video streams in one call on the MI355X (tests/stream_serve_cases.py): the two kernels alone, their refusals, and the serving
programs of three small plans, each in fp32 and in bf16 storage (K=13 B=3 32x40; K=15 B=2 39x39, the widened hand-over with the fp32
gate convolution and pad lanes 17..19; K=13 B=2 64x72 at output stride 8).  Equal bits to the plan's own stream programs, lane by
lane, throughout."""
import pytest
import torch

import stream_serve_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PLANS = [dict(K=13, B=3, H=32, W=40), dict(K=15, B=2, H=39, W=39), dict(K=13, B=2, H=64, W=72, output_stride=8)]


def _id(cfg):
    return "K{K}-B{B}-{H}x{W}".format(**cfg) + ("-os8" if cfg.get("output_stride") == 8 else "") + "-" + cfg["storage"]


@pytest.fixture(params=[dict(p, storage=s) for p in PLANS for s in ("f32", "bf16")], ids=_id)
def serve_ctx(request):
    return sc.ctx(DEV, **request.param)


@pytest.mark.parametrize("cg,ldo,rps,B", sc.KERNEL_CASES)
def test_lstm_serve_fwd(cg, ldo, rps, B):
    sc.serve_fwd_case(DEV, cg, ldo, rps, B)


@pytest.mark.parametrize("cg,ldo,rps,B", sc.KERNEL_CASES)
def test_lstm_state_gather(cg, ldo, rps, B):
    sc.gather_case(DEV, cg, ldo, rps, B)


def test_lstm_serve_kernel_refusals():
    sc.kernel_refusal_case(DEV)


def test_lstm_serve_ops():
    sc.ops_case(DEV)


def test_serve_schedule(serve_ctx):
    sc.schedule_case(serve_ctx)


def test_serve_two_pools(serve_ctx):
    sc.two_pools_case(serve_ctx)


def test_serve_all_idle_and_pool_view(serve_ctx):
    sc.idle_case(serve_ctx)


def test_serve_frames(serve_ctx):
    sc.frames_case(serve_ctx)


def test_serve_one_pass_plan(serve_ctx):
    sc.one_pass_case(serve_ctx)


def test_serve_refusals(serve_ctx):
    sc.refusal_case(serve_ctx)


def test_serve_unchanged_figures(serve_ctx):
    sc.figures_case(serve_ctx)


def test_serve_big_batch_and_unset_weights():
    sc.big_batch_case(DEV)
