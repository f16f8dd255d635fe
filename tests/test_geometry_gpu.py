"""Off-network convolution geometries and the edge shapes of the spatial / element-wise kernels on a real MI355X, through the
C ABI: element by element against float64 (geometry_cases.py).  These are the launches whose out-of-image taps go furthest
outside the tensor; on the GPU the operands travel by LDS-DMA with the hardware's own out-of-range behaviour, which the CPU
emulator only models.  The spatial kernels run every element-type instantiation (hipcc once mis-compiled exactly one of them).

Worst got / bound ratios (bound = 2 (L + 1) 2^-24 A, see geometry_cases.py), over all geometries, kernel generations, tile
sizes and K-split runs.  Seen on the MI355X at the aligned pair (32, 64): fp32 dw 0.138, db 0.068; bf16 storage y 0.985, dx 0.974
(one rounding to bf16 is up to 2^-8 of the value and fills that term of the bound), dw 0.062, db 0.000.  The generic pair
(10, 18) gives the worst fp32 y 0.125 and dx 0.067 on the emulator, which has matched the MI355X figure for figure at every pair
measured on both (same k order, same MFMA arithmetic).  The 254 tests of this file take about 4 s on the GPU.
"""
import pytest
import torch

import bf16s_cases as bc
import geometry_cases as gx
import op_cases as oc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
@pytest.mark.parametrize("geo", gx.GEOS, ids=gx.geo_id)
def test_conv_geometry_against_float64(geo, ck):
    gx.conv_geometry_case(DEV, geo, *ck)


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
@pytest.mark.parametrize("geo", gx.SPLIT, ids=gx.geo_id)
def test_conv_geometry_with_k_split_tail_tiles(geo, ck):
    gx.conv_geometry_case(DEV, geo, *ck, cus=3)


@pytest.mark.parametrize("geo", gx.GEOS, ids=gx.geo_id)
def test_conv_geometry_bf16_storage(geo):
    gx.conv_geometry_bf16s_case(DEV, geo)


@pytest.mark.parametrize("math,tol", [("bf16x3", 2e-4), ("bf16", 3e-2)])
@pytest.mark.parametrize("geo", gx.MODES, ids=gx.geo_id)
def test_conv_geometry_bf16_operand_kernels(geo, math, tol):
    gx.operand_mode_case(DEV, geo, math, tol)


@pytest.mark.parametrize("geo", gx.CONV_BN, ids=gx.geo_id)
def test_conv_bn_geometry(geo):
    n, h, w, r, s, stride, pad, dil = geo
    c, k = gx.CONV_BN_GENERIC if gx.CONV_BN.index(geo) % 2 else gx.ALIGNED
    oc.conv_bn_case(DEV, n, c, h, w, k, r, stride, pad, dil, relu=True, residual=True, train=True, tol=1e-4)


@pytest.mark.parametrize("geo", gx.CONV_BN, ids=gx.geo_id)
def test_conv_bn_geometry_bf16_storage(geo):
    n, h, w, r, s, stride, pad, dil = geo
    bc.conv_bn_case(DEV, n, gx.ALIGNED[0], h, w, gx.ALIGNED[1], r, stride, pad, dil, relu=True, residual=True, train=True)


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
@pytest.mark.parametrize("geo", gx.STRIDE1, ids=gx.geo_id)
def test_dgrad_addend_geometry(geo, ck):
    n, h, w, r, s, stride, pad, dil = geo
    oc.dgrad_add_case(DEV, n, ck[0], h, w, ck[1], (r, s), stride, pad, dil)


@pytest.mark.parametrize("ck", [gx.ALIGNED, gx.GENERIC], ids=lambda p: "c%d_k%d" % p)
def test_stride3_forward_and_weight_gradient_run_data_gradient_refuses(ck):
    gx.stride3_case(DEV, *ck)


def test_stride2_data_gradient_refuses_an_addend():
    gx.stride2_addend_case(DEV)


# ---- spatial and element-wise kernels ------------------------------------------------------------------
@pytest.mark.parametrize("types", gx.MAXPOOL_TYPES, ids=["f32_f32", "f32_bf16", "bf16_bf16"])
@pytest.mark.parametrize("shape", gx.MAXPOOL_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_maxpool_edges(shape, types):
    oc.maxpool_case(DEV, *shape, in_dtype=types[0], out_dtype=types[1])


@pytest.mark.parametrize("types", gx.MAXPOOL_TYPES, ids=["f32_f32", "f32_bf16", "bf16_bf16"])
def test_maxpool_special_values(types):
    oc.maxpool_case(DEV, 1, 4, 6, 6, in_dtype=types[0], out_dtype=types[1], x=gx.maxpool_special())


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [4, 20])
@pytest.mark.parametrize("shape", gx.BILINEAR_SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_bilinear_edges(shape, c, dtype):
    h, w, p, q = shape
    oc.bilinear_case(DEV, 1, c, h, w, p, q, dtype=dtype, f64=True)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [4, 68])
@pytest.mark.parametrize("pq", gx.BCAST_PQ, ids=lambda s: "%dx%d" % s)
def test_broadcast_backward(pq, c, dtype):
    oc.bilinear_case(DEV, 2, c, 1, 1, *pq, dtype=dtype, f64=True)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", gx.GAP_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_gap_edges(shape, dtype):
    oc.gap_case(DEV, *shape, dtype=dtype, f64=True)


@pytest.mark.parametrize("size", gx.AVGPOOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_avgpool9s8_edges(size):
    oc.avgpool_case(DEV, *size, f64=True)
    gx.clip_avgpool_case(DEV, *size)


@pytest.mark.parametrize("c", [3, 20])
def test_clip_layout(c):
    gx.clip_layout_case(DEV, c)


@pytest.mark.parametrize("cg", [13, 15, 16])
def test_lstm_gates_saturated(cg):
    oc.lstm_case(DEV, cg=cg, scale=40.0, f64=True, fwd_tol=1e-6)


@pytest.mark.parametrize("shape", gx.MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mse_sizes(shape):
    oc.mse_case(DEV, shape, f64=True)


@pytest.mark.parametrize("c", [3, 4, 20])
def test_copy2d_add2d(c):
    gx.copy_add_case(DEV, c)
