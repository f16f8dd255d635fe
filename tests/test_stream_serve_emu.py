"""Many video streams in one call on the CPU emulator (tests/stream_serve_cases.py): the two kernels alone with an inaccessible page
directly in front of, then directly behind, the pool, the gate tensors and the gather's destination; their refusals; the serving
programs of the plan at K=13, B=3, 32x40 in both storages (the two other configurations run on the GPU: a plan takes minutes here)."""
import pytest

import stream_serve_cases as sc


@pytest.mark.parametrize("fence", ["front", "back"])
@pytest.mark.parametrize("cg,ldo,rps,B", sc.KERNEL_CASES)
def test_lstm_serve_fwd_emu(emu_backend, cg, ldo, rps, B, fence):
    sc.serve_fwd_case(emu_backend, cg, ldo, rps, B, fence)


@pytest.mark.parametrize("fence", ["front", "back"])
@pytest.mark.parametrize("cg,ldo,rps,B", sc.KERNEL_CASES)
def test_lstm_state_gather_emu(emu_backend, cg, ldo, rps, B, fence):
    sc.gather_case(emu_backend, cg, ldo, rps, B, fence)


def test_lstm_serve_kernel_refusals_emu(emu_backend):
    sc.kernel_refusal_case(emu_backend)


def test_lstm_serve_ops_emu(emu_backend):
    sc.ops_case(emu_backend)


def test_stream_slots():
    sc.stream_slots_case()


@pytest.fixture(params=["f32", "bf16"])
def serve_ctx(request, emu_backend):
    return sc.ctx(emu_backend, storage=request.param)


def test_serve_schedule_emu(serve_ctx):
    sc.schedule_case(serve_ctx)


def test_serve_two_pools_emu(serve_ctx):
    sc.two_pools_case(serve_ctx)


def test_serve_all_idle_and_pool_view_emu(serve_ctx):
    sc.idle_case(serve_ctx)


def test_serve_frames_emu(serve_ctx):
    sc.frames_case(serve_ctx)


def test_serve_one_pass_plan_emu(serve_ctx):
    sc.one_pass_case(serve_ctx, frames=1)


def test_serve_refusals_emu(serve_ctx):
    sc.refusal_case(serve_ctx)


def test_serve_unchanged_figures_emu(serve_ctx):
    sc.figures_case(serve_ctx)


def test_serve_big_batch_and_unset_weights_emu(emu_backend):
    sc.big_batch_case(emu_backend)
