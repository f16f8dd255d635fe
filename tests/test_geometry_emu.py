"""Off-network convolution geometries and the edge shapes of the spatial / element-wise kernels on a GPU-less box: the HIP
sources compiled against the fiber emulator (tests/emu), element by element against float64 (geometry_cases.py).  The
emulator models the LDS-DMA operand path with its own allocator, so the out-of-image taps of these launches are settled for
the GPU only by test_geometry_gpu.py; the empty-output refusal is host code and is tested here alone."""
import pytest
import torch

import bf16s_cases as bc
import geometry_cases as gx
import op_cases as oc

BF = torch.bfloat16


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
@pytest.mark.parametrize("geo", gx.GEOS, ids=gx.geo_id)
def test_conv_geometry_against_float64(emu_backend, geo, ck):
    gx.conv_geometry_case(emu_backend, geo, *ck)


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
@pytest.mark.parametrize("geo", gx.SPLIT, ids=gx.geo_id)
def test_conv_geometry_with_k_split_tail_tiles(emu_backend, geo, ck):
    gx.conv_geometry_case(emu_backend, geo, *ck, cus=3)


@pytest.mark.parametrize("geo", gx.GEOS, ids=gx.geo_id)
def test_conv_geometry_bf16_storage(emu_backend, geo):
    gx.conv_geometry_bf16s_case(emu_backend, geo)


@pytest.mark.parametrize("math,tol", [("bf16x3", 2e-4), ("bf16", 3e-2)])
@pytest.mark.parametrize("geo", gx.MODES, ids=gx.geo_id)
def test_conv_geometry_bf16_operand_kernels(emu_backend, geo, math, tol):
    gx.operand_mode_case(emu_backend, geo, math, tol)


@pytest.mark.parametrize("geo", gx.CONV_BN, ids=gx.geo_id)
def test_conv_bn_geometry(emu_backend, geo):
    n, h, w, r, s, stride, pad, dil = geo
    c, k = gx.CONV_BN_GENERIC if gx.CONV_BN.index(geo) % 2 else gx.ALIGNED
    oc.conv_bn_case(emu_backend, n, c, h, w, k, r, stride, pad, dil, relu=True, residual=True, train=True)


@pytest.mark.parametrize("geo", gx.CONV_BN, ids=gx.geo_id)
def test_conv_bn_geometry_bf16_storage(emu_backend, geo):
    n, h, w, r, s, stride, pad, dil = geo
    bc.conv_bn_case(emu_backend, n, gx.ALIGNED[0], h, w, gx.ALIGNED[1], r, stride, pad, dil, relu=True, residual=True, train=True)


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
@pytest.mark.parametrize("geo", gx.STRIDE1, ids=gx.geo_id)
def test_dgrad_addend_geometry(emu_backend, geo, ck):
    n, h, w, r, s, stride, pad, dil = geo
    oc.dgrad_add_case(emu_backend, n, ck[0], h, w, ck[1], (r, s), stride, pad, dil)


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
def test_stride3_forward_and_weight_gradient_run_data_gradient_refuses(emu_backend, ck):
    gx.stride3_case(emu_backend, *ck)


def test_stride2_data_gradient_refuses_an_addend(emu_backend):
    gx.stride2_addend_case(emu_backend)


@pytest.mark.parametrize("stride", [1, 2])
def test_empty_output_is_refused(emu_backend, stride):
    gx.empty_output_case(emu_backend, stride)


# ---- spatial and element-wise kernels ------------------------------------------------------------------
@pytest.mark.parametrize("types", gx.MAXPOOL_TYPES, ids=["f32_f32", "f32_bf16", "bf16_bf16"])
@pytest.mark.parametrize("shape", gx.MAXPOOL_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_maxpool_edges(emu_backend, shape, types):
    oc.maxpool_case(emu_backend, *shape, in_dtype=types[0], out_dtype=types[1])


@pytest.mark.parametrize("types", gx.MAXPOOL_TYPES, ids=["f32_f32", "f32_bf16", "bf16_bf16"])
def test_maxpool_special_values(emu_backend, types):
    oc.maxpool_case(emu_backend, 1, 4, 6, 6, in_dtype=types[0], out_dtype=types[1], x=gx.maxpool_special())


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [4, 20])
@pytest.mark.parametrize("shape", gx.BILINEAR_SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_bilinear_edges(emu_backend, shape, c, dtype):
    h, w, p, q = shape
    oc.bilinear_case(emu_backend, 1, c, h, w, p, q, dtype=dtype, f64=True)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [4, 68])
@pytest.mark.parametrize("pq", gx.BCAST_PQ, ids=lambda s: "%dx%d" % s)
def test_broadcast_backward(emu_backend, pq, c, dtype):
    oc.bilinear_case(emu_backend, 2, c, 1, 1, *pq, dtype=dtype, f64=True)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", gx.GAP_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_gap_edges(emu_backend, shape, dtype):
    oc.gap_case(emu_backend, *shape, dtype=dtype, f64=True)


@pytest.mark.parametrize("size", gx.AVGPOOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_avgpool9s8_edges(emu_backend, size):
    oc.avgpool_case(emu_backend, *size, f64=True)
    gx.clip_avgpool_case(emu_backend, *size)


@pytest.mark.parametrize("c", [3, 20])
def test_clip_layout(emu_backend, c):
    gx.clip_layout_case(emu_backend, c)


@pytest.mark.parametrize("cg", [13, 15, 16])
def test_lstm_gates_saturated(emu_backend, cg):
    oc.lstm_case(emu_backend, cg=cg, scale=40.0, f64=True, fwd_tol=1e-6)


@pytest.mark.parametrize("shape", gx.MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mse_sizes(emu_backend, shape):
    oc.mse_case(emu_backend, shape, f64=True)


@pytest.mark.parametrize("c", [3, 4, 20])
def test_copy2d_add2d(emu_backend, c):
    gx.copy_add_case(emu_backend, c)
