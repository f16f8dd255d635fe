// Layout conversion at the NCHW boundary, max-pool 3/2/1, bilinear (align_corners) resampling,
// global average pool, AvgPool(9,8,1) of the centre map, strided copies (concat/slice), ConvLSTM
// gate math and the wave-reduced heat-map argmax.  All HBM-bound: 16-byte channel-vector accesses on
// NHWC tensors, one thread per (pixel, 4 channels).
#include "up_common.h"

namespace up {

static inline int grid_cap(int64_t work_items, int cap = 8192) {
    int64_t g = (work_items + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > cap ? cap : g);
}

#define UP_GRID_STRIDE(i, total) \
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (total); i += (int64_t)gridDim.x * 256)

// ---- layout ------------------------------------------------------------------------------
// channel c of the NCHW pixel at `src` (planes HW apart); the pad channels C <= c < ld of an NHWC row read as zeros
__device__ __forceinline__ float nchw_at(const float* src, int C, int HW, int c) { return c < C ? src[(int64_t)c * HW] : 0.f; }

template <typename TO>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* x, TO* y, int C, int HW, int ld,
                                                           int64_t npix) {
    UP_GRID_STRIDE(i, npix) {
        int64_t n = i / HW;
        int hw = (int)(i - n * HW);
        const float* src = x + n * C * HW + hw;
        TO* dst = y + i * ld;
        for (int c = 0; c < ld; ++c) st1(dst + c, nchw_at(src, C, HW, c));
    }
}
template <typename TI>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const TI* x, int ld, float* y, int C, int HW,
                                                           int64_t npix) {
    UP_GRID_STRIDE(i, npix) {
        int64_t n = i / HW;
        int hw = (int)(i - n * HW);
        const TI* src = x + i * ld;
        float* dst = y + n * C * HW + hw;
        for (int c = 0; c < C; ++c) dst[(int64_t)c * HW] = ld1(src + c);
    }
}

// Clip layout (the video plan, plan.hip): a clip is batch-major, (B, T, ...), the trunk and the head run frame-major, on T * B
// images with image f = t * B + b.  One thread per frame-major pixel; the NHWC side moves 16-byte channel quads (a wave writes
// resp. reads 1 KiB of consecutive pixels per instruction), the NCHW side one plane per channel, consecutive pixels on
// consecutive lanes.  ld % 4 == 0 and 16-byte aligned NHWC pointers (checked by the host wrappers).
__device__ __forceinline__ int64_t clip_image(int64_t f, int B, int T) {      // frame-major image f -> batch-major image b * T + t
    const int64_t t = f / B;
    return (f - t * B) * T + t;
}
// The _strided entries (the one-pass flip test of the video plan): frames of FI >= B images, the B samples of a launch from image
// `first` of each on, so the image written for frame-major f = t * B + b is t * FI + first + b.  Every clip kernel that writes
// frame-major images comes in both forms around ONE device function; STRIDED = false is f itself, the launch as it always was.
template <bool STRIDED>
__device__ __forceinline__ int64_t clip_dest(int64_t f, int B, int FI, int first) {
    if (!STRIDED) return f;
    const int64_t t = f / B;
    return t * FI + first + (f - t * B);
}
// FLIP: the mirror folded in (the flip test of the video plan): the NHWC pixel (h, w) takes the NCHW pixel (h, W - 1 - w)
template <bool FLIP, bool STRIDED>
__device__ __forceinline__ void clip_nchw_to_nhwc_body(const float* x, float* y, int B, int T, int C, int W, int HW, int ld,
                                                       int64_t npix, int FI, int first) {
    UP_GRID_STRIDE(i, npix) {
        const int64_t f = i / HW;
        const int pix = (int)(i - f * HW);
        int hw = pix;
        if (FLIP) {
            const int h = hw / W;
            hw = h * W + (W - 1 - (hw - h * W));
        }
        const float* src = x + clip_image(f, B, T) * C * HW + hw;
        float* dst = y + (STRIDED ? clip_dest<true>(f, B, FI, first) * HW + pix : i) * ld;
        for (int c = 0; c < ld; c += 4)
            *reinterpret_cast<float4*>(dst + c) =
                make_float4(nchw_at(src, C, HW, c), nchw_at(src, C, HW, c + 1), nchw_at(src, C, HW, c + 2), nchw_at(src, C, HW, c + 3));
    }
}
template <bool FLIP>
__global__ void __launch_bounds__(256) clip_nchw_to_nhwc_kernel(const float* x, float* y, int B, int T, int C, int W, int HW, int ld,
                                                                int64_t npix) {
    clip_nchw_to_nhwc_body<FLIP, false>(x, y, B, T, C, W, HW, ld, npix, B, 0);
}
template <bool FLIP>
__global__ void __launch_bounds__(256) clip_nchw_to_nhwc_strided_kernel(const float* x, float* y, int B, int T, int C, int W, int HW,
                                                                        int ld, int64_t npix, int FI, int first) {
    clip_nchw_to_nhwc_body<FLIP, true>(x, y, B, T, C, W, HW, ld, npix, FI, first);
}
__global__ void __launch_bounds__(256) clip_nhwc_to_nchw_kernel(const float* x, int ld, float* y, int B, int T, int C, int HW,
                                                                int64_t npix) {
    UP_GRID_STRIDE(i, npix) {
        const int64_t f = i / HW;
        const int hw = (int)(i - f * HW);
        const float* src = x + i * ld;
        float* dst = y + clip_image(f, B, T) * C * HW + hw;
        for (int c = 0; c < C; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(src + c);
            dst[(int64_t)c * HW] = v.x;
            if (c + 1 < C) dst[(int64_t)(c + 1) * HW] = v.y;
            if (c + 2 < C) dst[(int64_t)(c + 2) * HW] = v.z;
            if (c + 3 < C) dst[(int64_t)(c + 3) * HW] = v.w;
        }
    }
}

// ---- 2-D strided copy / add ----------------------------------------------------------------
__global__ void __launch_bounds__(256) copy2d_v4_kernel(const float* s, int lds, float* d, int ldd, int64_t total,
                                                        int C4, FastDiv fC4) {
    UP_GRID_STRIDE(i, total) {
        uint32_t row = fdiv((uint32_t)i, fC4);
        int c = ((int)i - (int)row * C4) * 4;
        *reinterpret_cast<float4*>(d + (size_t)row * ldd + c) = *reinterpret_cast<const float4*>(s + (size_t)row * lds + c);
    }
}
__global__ void __launch_bounds__(256) copy2d_s_kernel(const float* s, int lds, float* d, int ldd, int64_t total,
                                                       int C, FastDiv fC) {
    UP_GRID_STRIDE(i, total) {
        uint32_t row = fdiv((uint32_t)i, fC);
        int c = (int)i - (int)row * C;
        d[(size_t)row * ldd + c] = s[(size_t)row * lds + c];
    }
}
__global__ void __launch_bounds__(256) add2d_kernel(const float* a, int lda, const float* b, int ldb, float* d,
                                                    int ldd, int64_t total, int C, FastDiv fC) {
    UP_GRID_STRIDE(i, total) {
        uint32_t row = fdiv((uint32_t)i, fC);
        int c = (int)i - (int)row * C;
        d[(size_t)row * ldd + c] = a[(size_t)row * lda + c] + b[(size_t)row * ldb + c];
    }
}

// ---- max-pool 3x3 / stride 2 / pad 1 --------------------------------------------------------
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const TI* x, int ldx, TO* y, int ldy, uint8_t* idx,
                                                          int H, int W, int C4, int P, int Q, int64_t total,
                                                          FastDiv fC4, FastDiv fQ, FastDiv fP) {
    UP_GRID_STRIDE(i, total) {
        uint32_t pix = fdiv((uint32_t)i, fC4);
        int c = ((int)i - (int)pix * C4) * 4;
        uint32_t t = fdiv(pix, fQ);
        int q = (int)pix - (int)t * Q;
        uint32_t n = fdiv(t, fP);
        int p = (int)t - (int)n * P;
        // The first in-bounds window element is (r0, s0); starting every channel from its code with best = -inf makes the
        // scan branch-free ("first" flag gone): a later element replaces it iff it is larger or NaN, exactly F.max_pool2d's
        // rule (first maximum in scan order wins).  (With a `first` flag in the loop hipcc 7.2 mis-compiled the
        // <bf16, bf16> instantiation — stale code for element 0, values right — tools/gpu/dbg_maxpool.py.)
        const int r0 = 2 * p - 1 < 0 ? 1 : 0, s0 = 2 * q - 1 < 0 ? 1 : 0;
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {r0 * 3 + s0, r0 * 3 + s0, r0 * 3 + s0, r0 * 3 + s0};
        for (int r = r0; r < 3; ++r) {
            int h = 2 * p - 1 + r;
            if (h >= H) break;
            for (int s = s0; s < 3; ++s) {
                int w = 2 * q - 1 + s;
                if (w >= W) break;
                float4 v4 = ld4<TI>(x + ((size_t)(n * H + h) * W + w) * ldx + c);
                float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > best[e] || v[e] != v[e]) {
                        best[e] = v[e];
                        bi[e] = r * 3 + s;
                    }
            }
        }
        st4(y + (size_t)pix * ldy + c, make_float4(best[0], best[1], best[2], best[3]));
        // one 32-bit store of the four window codes
        *reinterpret_cast<uint32_t*>(idx + (size_t)pix * (C4 * 4) + c) =
            (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
    }
}
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const TI* dy, int lddy, const uint8_t* idx, TO* dx,
                                                          int lddx, int H, int W, int C4, int P, int Q,
                                                          int64_t total, FastDiv fC4, FastDiv fW, FastDiv fH) {
    UP_GRID_STRIDE(i, total) {
        uint32_t pix = fdiv((uint32_t)i, fC4);
        int c = ((int)i - (int)pix * C4) * 4;
        uint32_t t = fdiv(pix, fW);
        int w = (int)pix - (int)t * W;
        uint32_t n = fdiv(t, fH);
        int h = (int)t - (int)n * H;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < 3; ++r) {
            int tp = h + 1 - r;
            if (tp < 0 || (tp & 1) || (tp >> 1) >= P) continue;
            int p = tp >> 1;
            for (int s = 0; s < 3; ++s) {
                int tq = w + 1 - s;
                if (tq < 0 || (tq & 1) || (tq >> 1) >= Q) continue;
                int q = tq >> 1;
                size_t op = (size_t)(n * P + p) * Q + q;
                const uint8_t* ip = idx + op * (C4 * 4) + c;
                float4 g = ld4<TI>(dy + op * lddy + c);
                int code = r * 3 + s;
                if (ip[0] == code) acc[0] += g.x;
                if (ip[1] == code) acc[1] += g.y;
                if (ip[2] == code) acc[2] += g.z;
                if (ip[3] == code) acc[3] += g.w;
            }
        }
        st4(dx + (size_t)pix * lddx + c, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}

// ---- bilinear, align_corners=True ----------------------------------------------------------
// The two taps of output sample `o` (scale s, `n` input samples) with their weights, and the blend of the four neighbours
//     lh0 * (lw0 * a00 + lw1 * a01) + lh1 * (lw0 * a10 + lw1 * a11).
// bilinear_fwd_kernel and decode_kernel both go through these two: up_heatmap_decode promises the bits of up_bilinear_fwd.  Left
// to the compiler, the contraction of these expressions to FMAs depends on the code around them (in bilinear_fwd_kernel it came
// out differently for the even and the odd channels of a float4, in a scalar loop differently again), so the roundings are
// spelled out: they are the ones bilinear_fwd_kernel has always had on gfx950 (read off its ISA; its results are unchanged).
//   l1 = fma(s, o, -i0)                                                             (not the rounded product s * o minus i0)
//   even channel: t = fma(lw0, left, lw1 * right), result fma(lh1, t1, lh0 * t0)
//   odd channel:  t = fma(lw1, right, lw0 * left), result fma(lh0, t0, lh1 * t1)
struct BilTap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ BilTap bil_tap(float s, int o, int n) {
    BilTap t;
    const float fo = (float)o;
    t.i0 = (int)__fmul_rn(s, fo);
    t.i1 = t.i0 < n - 1 ? t.i0 + 1 : t.i0;
    t.l1 = __fmaf_rn(s, fo, -(float)t.i0);
    t.l0 = 1.f - t.l1;
    return t;
}
template <int ODD>
__device__ __forceinline__ float bil_mix(float lh0, float lh1, float lw0, float lw1, float a00, float a01, float a10,
                                         float a11) {
    if (ODD) {
        const float t0 = __fmaf_rn(lw1, a01, __fmul_rn(lw0, a00));
        const float t1 = __fmaf_rn(lw1, a11, __fmul_rn(lw0, a10));
        return __fmaf_rn(lh0, t0, __fmul_rn(lh1, t1));
    }
    const float t0 = __fmaf_rn(lw0, a00, __fmul_rn(lw1, a01));
    const float t1 = __fmaf_rn(lw0, a10, __fmul_rn(lw1, a11));
    return __fmaf_rn(lh1, t1, __fmul_rn(lh0, t0));
}
template <typename T>
__global__ void __launch_bounds__(256) bilinear_fwd_kernel(const T* x, int ldx, T* y, int ldy, int H, int W,
                                                           int C4, int P, int Q, float sh, float sw, int64_t total,
                                                           FastDiv fC4, FastDiv fQ, FastDiv fP) {
    UP_GRID_STRIDE(i, total) {
        uint32_t pix = fdiv((uint32_t)i, fC4);
        int c = ((int)i - (int)pix * C4) * 4;
        uint32_t t = fdiv(pix, fQ);
        int q = (int)pix - (int)t * Q;
        uint32_t n = fdiv(t, fP);
        int p = (int)t - (int)n * P;
        const BilTap th = bil_tap(sh, p, H), tw = bil_tap(sw, q, W);
        const T* b = x + (size_t)n * H * W * ldx + c;
        float4 a00 = ld4<T>(b + (size_t)(th.i0 * W + tw.i0) * ldx);
        float4 a01 = ld4<T>(b + (size_t)(th.i0 * W + tw.i1) * ldx);
        float4 a10 = ld4<T>(b + (size_t)(th.i1 * W + tw.i0) * ldx);
        float4 a11 = ld4<T>(b + (size_t)(th.i1 * W + tw.i1) * ldx);
        float4 o;
        o.x = bil_mix<0>(th.l0, th.l1, tw.l0, tw.l1, a00.x, a01.x, a10.x, a11.x);
        o.y = bil_mix<1>(th.l0, th.l1, tw.l0, tw.l1, a00.y, a01.y, a10.y, a11.y);
        o.z = bil_mix<0>(th.l0, th.l1, tw.l0, tw.l1, a00.z, a01.z, a10.z, a11.z);
        o.w = bil_mix<1>(th.l0, th.l1, tw.l0, tw.l1, a00.w, a01.w, a10.w, a11.w);
        st4(y + (size_t)pix * ldy + c, o);
    }
}
// weight with which output coordinate o (of `out` samples, scale s) reads input sample `in_i`
__device__ __forceinline__ float bil_weight(int o, int in_i, int in_n, float s) {
    float f = s * o;
    int i0 = (int)f;
    int i1 = i0 < in_n - 1 ? i0 + 1 : i0;
    float l1 = f - i0;
    float w = 0.f;
    if (i0 == in_i) w += 1.f - l1;
    if (i1 == in_i) w += l1;
    return w;
}
template <typename T>
__global__ void __launch_bounds__(256) bilinear_bwd_kernel(const T* dy, int lddy, T* dx, int lddx, int H,
                                                           int W, int C4, int P, int Q, float sh, float sw,
                                                           int64_t total, FastDiv fC4, FastDiv fW, FastDiv fH) {
    UP_GRID_STRIDE(i, total) {
        uint32_t pix = fdiv((uint32_t)i, fC4);
        int c = ((int)i - (int)pix * C4) * 4;
        uint32_t t = fdiv(pix, fW);
        int w = (int)pix - (int)t * W;
        uint32_t n = fdiv(t, fH);
        int h = (int)t - (int)n * H;
        int p_lo = 0, p_hi = P - 1, q_lo = 0, q_hi = Q - 1;
        if (sh > 0.f) {
            p_lo = max(0, (int)floorf((h - 1) / sh) - 1);
            p_hi = min(P - 1, (int)ceilf((h + 1) / sh) + 1);
        }
        if (sw > 0.f) {
            q_lo = max(0, (int)floorf((w - 1) / sw) - 1);
            q_hi = min(Q - 1, (int)ceilf((w + 1) / sw) + 1);
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = p_lo; p <= p_hi; ++p) {
            float wh = bil_weight(p, h, H, sh);
            if (wh == 0.f) continue;
            for (int q = q_lo; q <= q_hi; ++q) {
                float ww = bil_weight(q, w, W, sw);
                if (ww == 0.f) continue;
                float4 g = ld4<T>(dy + ((size_t)(n * P + p) * Q + q) * lddy + c);
                float k = wh * ww;
                acc[0] += k * g.x;
                acc[1] += k * g.y;
                acc[2] += k * g.z;
                acc[3] += k * g.w;
            }
        }
        st4(dx + (size_t)pix * lddx + c, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}

// Backward of the broadcast of a 1x1 map (the WASP global-pool branch is up-sampled from 1x1 to the feature-map size,
// wasp.py:83): dx[n][c] = sum over all P*Q output pixels of dy.  The generic gather above would give ONE thread the whole
// P*Q loop (868 us at 46x46); here a workgroup owns (image, 64 channels): 16 row lanes x 16 four-channel groups, four rows in
// flight per thread, LDS tree over the row lanes (fixed order: deterministic).
template <typename T>
__global__ void __launch_bounds__(256) bcast_bwd_kernel(const T* dy, int lddy, T* dx, int lddx, int PQ, int C) {
    __shared__ float red[16][64];
    const int n = blockIdx.x;
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.y * 64 + cq * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
        const T* base = dy + (size_t)n * PQ * lddy + c;
        int r = rl;
        for (; r + 48 < PQ; r += 64) {
            const float4 a = ld4<T>(base + (size_t)r * lddy), b = ld4<T>(base + (size_t)(r + 16) * lddy);
            const float4 e = ld4<T>(base + (size_t)(r + 32) * lddy), f = ld4<T>(base + (size_t)(r + 48) * lddy);
            s.x += (a.x + b.x) + (e.x + f.x);
            s.y += (a.y + b.y) + (e.y + f.y);
            s.z += (a.z + b.z) + (e.z + f.z);
            s.w += (a.w + b.w) + (e.w + f.w);
        }
        for (; r < PQ; r += 16) {
            const float4 a = ld4<T>(base + (size_t)r * lddy);
            s.x += a.x;
            s.y += a.y;
            s.z += a.z;
            s.w += a.w;
        }
    }
    red[rl][cq * 4 + 0] = s.x;
    red[rl][cq * 4 + 1] = s.y;
    red[rl][cq * 4 + 2] = s.z;
    red[rl][cq * 4 + 3] = s.w;
    __syncthreads();
    if (threadIdx.x < 16 && c < C) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 16; ++k)
            for (int e = 0; e < 4; ++e) t[e] += red[k][cq * 4 + e];
        st4(dx + (size_t)n * lddx + c, make_float4(t[0], t[1], t[2], t[3]));
    }
}

// ---- global average pool ---------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) gap_fwd_kernel(const T* x, int ldx, T* y, int HW, int C) {
    __shared__ float red[256];
    int n = blockIdx.x;
    int c = blockIdx.y * 64 + (threadIdx.x & 63);
    int rl = threadIdx.x >> 6;
    float s = 0.f;
    if (c < C)
        for (int r = rl; r < HW; r += 4) s += ld1(x + ((size_t)n * HW + r) * ldx + c);
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        int t = threadIdx.x;
        st1(y + (size_t)n * C + c, (red[t] + red[t + 64] + red[t + 128] + red[t + 192]) / (float)HW);
    }
}
template <typename T>
__global__ void __launch_bounds__(256) gap_bwd_kernel(const T* dy, T* dx, int lddx, int HW, int C4,
                                                      float inv, int64_t total, FastDiv fC4, FastDiv fHW) {
    UP_GRID_STRIDE(i, total) {
        uint32_t pix = fdiv((uint32_t)i, fC4);
        int c = ((int)i - (int)pix * C4) * 4;
        uint32_t n = fdiv(pix, fHW);
        float4 g = ld4<T>(dy + (size_t)n * (C4 * 4) + c);
        st4(dx + (size_t)pix * lddx + c, make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv));
    }
}

// ---- AvgPool2d(9, 8, 1), count_include_pad -----------------------------------------------------
// output pixel (p, q) of the H x W plane `x`: the arithmetic of both launches below (a clip's centre maps pool to the same bits)
// FLIP: ... of the MIRRORED plane, m[h][w] = x[h][W - 1 - w], read in place: the window and the divisor are those of column q of
// m (the padding sits on one side, so this is not the window of column Q - 1 - q of x), and the sum runs over ascending w of m
// tap(h, c): the value at row h, column c of the plane that is stored (c = W - 1 - w under FLIP).  The ONE statement of the
// window, the divisor and the order of the sum: the pooling launches and the centre-pool launches both return this.
template <bool FLIP, typename Tap>
__device__ __forceinline__ float avgpool9s8_window(int H, int W, int p, int q, Tap tap) {
    int hs = p * 8 - 1, ws = q * 8 - 1;
    int he = min(hs + 9, H + 1), we = min(ws + 9, W + 1);
    float div = (float)((he - hs) * (we - ws));
    hs = max(hs, 0);
    ws = max(ws, 0);
    he = min(he, H);
    we = min(we, W);
    float s = 0.f;
    for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) s += tap(h, FLIP ? W - 1 - w : w);
    return s / div;
}
template <bool FLIP = false>
__device__ __forceinline__ float avgpool9s8_at(const float* x, int H, int W, int p, int q) {
    return avgpool9s8_window<FLIP>(H, W, p, q, [=](int h, int c) { return x[h * W + c]; });
}
__global__ void __launch_bounds__(256) avgpool9s8_kernel(const float* x, float* y, int ldy, int coff, int H, int W,
                                                         int P, int Q, int64_t total) {
    UP_GRID_STRIDE(i, total) {
        int q = (int)(i % Q);
        int64_t t = i / Q;
        int p = (int)(t % P);
        int64_t n = t / P;
        y[i * ldy + coff] = avgpool9s8_at(x + n * H * W, H, W, p, q);
    }
}
// ... of a clip's (B, T, 1, H, W) centre maps into channel coff of the frame-major (T * B, P, Q, ldy) hand-over tensor
template <bool FLIP, bool STRIDED>
__device__ __forceinline__ void clip_avgpool9s8_body(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P,
                                                     int Q, int64_t total, int FI, int first) {
    UP_GRID_STRIDE(i, total) {
        int q = (int)(i % Q);
        int64_t t = i / Q;
        int p = (int)(t % P);
        int64_t f = t / P;
        const int64_t o = STRIDED ? (clip_dest<true>(f, B, FI, first) * P + p) * Q + q : i;
        y[o * ldy + coff] = avgpool9s8_at<FLIP>(x + clip_image(f, B, T) * H * W, H, W, p, q);
    }
}
template <bool FLIP>
__global__ void __launch_bounds__(256) clip_avgpool9s8_kernel(const float* x, float* y, int ldy, int coff, int B, int T, int H,
                                                              int W, int P, int Q, int64_t total) {
    clip_avgpool9s8_body<FLIP, false>(x, y, ldy, coff, B, T, H, W, P, Q, total, B, 0);
}
template <bool FLIP>
__global__ void __launch_bounds__(256) clip_avgpool9s8_strided_kernel(const float* x, float* y, int ldy, int coff, int B, int T, int H,
                                                                      int W, int P, int Q, int64_t total, int FI, int first) {
    clip_avgpool9s8_body<FLIP, true>(x, y, ldy, coff, B, T, H, W, P, Q, total, FI, first);
}

// ---- ConvLSTM gates -------------------------------------------------------------------------
__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }
// The two cell formulas, channel c of one row `g` of stacked gate pre-activations (g | i | o (| f), each Cg wide): shared by the
// plain forward kernels and lstm_serve_fwd_kernel, so a sample computes the same bits through either.
// LSTM_0 (uniposeLSTM.py:9-24) ...
__device__ __forceinline__ void lstm0_at(const float* g, int Cg, int c, float& cl, float& hd) {
    float gg = tanhf(g[c]), ii = sigm(g[Cg + c]), oo = sigm(g[2 * Cg + c]);
    cl = tanhf(gg * ii);
    hd = oo * cl;
}
// ... and LSTM (uniposeLSTM.py:27-64) with the previous cell value cp
__device__ __forceinline__ void lstm_at(const float* g, int Cg, int c, float cp, float& cl, float& hd) {
    float gg = tanhf(g[c]), ii = sigm(g[Cg + c]), oo = sigm(g[2 * Cg + c]), ff = sigm(g[3 * Cg + c]);
    cl = ff * cp + ii * gg;
    hd = oo * tanhf(cl);
}

__global__ void __launch_bounds__(256) lstm0_fwd_kernel(const float* G, int ldg, float* cell, float* hide, int ldo,
                                                        int64_t total, int Cg) {
    UP_GRID_STRIDE(i, total) {
        int64_t r = i / Cg;
        int c = (int)(i - r * Cg);
        float cl, hd;
        lstm0_at(G + r * ldg, Cg, c, cl, hd);
        cell[r * ldo + c] = cl;
        hide[r * ldo + c] = hd;
    }
}
__global__ void __launch_bounds__(256) lstm0_bwd_kernel(const float* G, int ldg, const float* dcell,
                                                        const float* dhide, int ldo, float* dG, int64_t total,
                                                        int Cg) {
    UP_GRID_STRIDE(i, total) {
        int64_t r = i / Cg;
        int c = (int)(i - r * Cg);
        const float* g = G + r * ldg;
        float gg = tanhf(g[c]), ii = sigm(g[Cg + c]), oo = sigm(g[2 * Cg + c]);
        float cl = tanhf(gg * ii);
        float dh = dhide[r * ldo + c];
        float dc = dcell[r * ldo + c] + dh * oo;
        float dgi = dc * (1.f - cl * cl);
        float* o = dG + r * ldg;
        o[c] = dgi * ii * (1.f - gg * gg);
        o[Cg + c] = dgi * gg * ii * (1.f - ii);
        o[2 * Cg + c] = dh * cl * oo * (1.f - oo);
    }
}
__global__ void __launch_bounds__(256) lstm_fwd_kernel(const float* G, int ldg, const float* cprev, int ldc,
                                                       float* cell, float* hide, int ldo, int64_t total, int Cg) {
    UP_GRID_STRIDE(i, total) {
        int64_t r = i / Cg;
        int c = (int)(i - r * Cg);
        float cl, hd;
        lstm_at(G + r * ldg, Cg, c, cprev[r * ldc + c], cl, hd);
        cell[r * ldo + c] = cl;
        hide[r * ldo + c] = hd;
    }
}
__global__ void __launch_bounds__(256) lstm_bwd_kernel(const float* G, int ldg, const float* cprev, int ldc,
                                                       const float* cell, const float* dcell, const float* dhide,
                                                       int ldo, float* dG, float* dcprev, int64_t total, int Cg) {
    UP_GRID_STRIDE(i, total) {
        int64_t r = i / Cg;
        int c = (int)(i - r * Cg);
        const float* g = G + r * ldg;
        float gg = tanhf(g[c]), ii = sigm(g[Cg + c]), oo = sigm(g[2 * Cg + c]), ff = sigm(g[3 * Cg + c]);
        float tc = tanhf(cell[r * ldo + c]);
        float dh = dhide[r * ldo + c];
        float dc = dcell[r * ldo + c] + dh * oo * (1.f - tc * tc);
        float* o = dG + r * ldg;
        o[c] = dc * ii * (1.f - gg * gg);
        o[Cg + c] = dc * gg * ii * (1.f - ii);
        o[2 * Cg + c] = dh * tc * oo * (1.f - oo);
        o[3 * Cg + c] = dc * cprev[r * ldc + c] * ff * (1.f - ff);
        dcprev[r * ldo + c] = dc * ff;
    }
}

// ---- ConvLSTM state of many streams in one batch (include/unipose_hip.h) ---------------------------------------------
// The per-call table travels by value, like FlipPerm: 264 bytes of kernel arguments.  A sample whose bit is set in `first` (a first
// or an idle one) is computed as a first frame and reads nothing of the pool; slot < 0 (idle) writes nothing of it either.
struct ServeTable {
    int32_t slot[UP_SERVE_CAP];
    uint64_t first;
};
// One thread per (row, lane < ldo), lanes fastest.  Record of slot s: hide (rps, ldo) then cell (rps, ldo) at pool + s * stride.
__global__ void __launch_bounds__(256) lstm_state_gather_kernel(const float* pool, int64_t stride, ServeTable tab, int64_t rps, int ldo,
                                                                float* dst, int ldd, int coff, int64_t total) {
    UP_GRID_STRIDE(i, total) {
        const int64_t row = i / ldo;
        const int c = (int)(i - row * ldo);
        const int b = (int)(row / rps);
        const int64_t rl = row - b * rps;
        const bool first = (tab.first >> b) & 1;
        dst[row * ldd + coff + c] = first ? 0.0f : pool[(int64_t)tab.slot[b] * stride + rl * ldo + c];
    }
}
__global__ void __launch_bounds__(256) lstm_serve_fwd_kernel(const float* G0, int ldg0, const float* G, int ldg, float* pool,
                                                             int64_t stride, ServeTable tab, float* cell, float* hide, int ldo,
                                                             int64_t rps, int64_t total, int Cg) {
    UP_GRID_STRIDE(i, total) {
        const int64_t row = i / ldo;
        const int c = (int)(i - row * ldo);
        const int b = (int)(row / rps);
        const int64_t rl = row - b * rps;
        const int slot = tab.slot[b];
        const bool first = (tab.first >> b) & 1;
        float* rec_hide = pool + (int64_t)(slot < 0 ? 0 : slot) * stride + rl * ldo + c;     // (not touched for slot < 0)
        float* rec_cell = rec_hide + rps * ldo;
        float cl = 0.0f, hd = 0.0f;
        if (c < Cg) {
            if (first) lstm0_at(G0 + row * ldg0, Cg, c, cl, hd);
            else lstm_at(G + row * ldg, Cg, c, *rec_cell, cl, hd);
            cell[row * ldo + c] = cl;
            hide[row * ldo + c] = hd;
        }
        if (slot >= 0) {
            *rec_hide = hd;
            *rec_cell = cl;
        }
    }
}

// ---- heat-map argmax: one wavefront per (b, j) map ------------------------------------------------
__device__ __forceinline__ bool am_better(float v, int i, float bv, int bi) {
    bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;        // NaN beats a number (np.argmax semantics)
    if (vn) return i < bi;          // both NaN: first one
    if (v != bv) return v > bv;
    return i < bi;                  // ties: lowest flat index
}
__global__ void __launch_bounds__(256) argmax_kernel(const float* hm, int maps, int HW, int W, int32_t* idx,
                                                     float* preds, float* maxvals) {
    int map = blockIdx.x * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (map >= maps) return;
    const float* p = hm + (size_t)map * HW;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < HW; i += 64) {
        float v = p[i];
        if (am_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        float ov = __shfl_down(bv, off);
        int oi = __shfl_down(bi, off);
        if (am_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        if (idx) idx[map] = bi;
        float keep = bv > 0.f ? 1.f : 0.f;
        preds[map * 2] = (float)(bi % W) * keep;
        preds[map * 2 + 1] = (float)(bi / W) * keep;
        maxvals[map] = bv;
    }
}

// ---- heat-map decode: the argmax of the maps AS IF up-sampled to P x Q by up_bilinear_fwd; one workgroup per (b, j) map ------
// The fine grid is never written.  Every thread evaluates the fine points i = tid, tid + 256, ... with the arithmetic of
// bilinear_fwd_kernel (bil_tap / bil_mix) from the coarse map — staged in LDS (STAGE), or read from global memory where it does
// not fit (it stays in L2) — and keeps (value, index); then the wave ladder of argmax_kernel and the four waves through LDS.
// am_better is a total order (NaN first, then the value, then the lowest index), so the order of the reduction does not matter.
// P == H and Q == W: no interpolation, the values are read as they are (never staged: each is read once).  A map is addressed
// by three strides: NHWC as the convolutions leave it (sj = 1, sp = ld, pad channels skipped) or NCHW (sj = H * W, sp = 1).
constexpr int DECODE_LDS = 12288;   // floats: 48 KB of the 64 KB static LDS limit (46 x 46 = 8.5 KB, 92 x 92 = 34 KB fit)
// CLIP (the video plan): the B * T images are frame-major, image f = t * B + b, and the results of image f go to the batch-major row
// clip_image(f) = b * T + t of the outputs; everything else is the same code.
template <bool STAGE, bool CLIP = false>
__global__ void __launch_bounds__(256) decode_kernel(const float* hm, int64_t sb, int64_t sj, int64_t sp, int J, int H, int W,
                                                     int P, int Q, float sh, float sw, FastDiv fQ, int32_t* idx, float* preds,
                                                     float* maxvals, int cB, int cT) {
    __shared__ float tile[STAGE ? DECODE_LDS : 1];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    const int map = blockIdx.x, tid = threadIdx.x;
    const int b = map / J, j = map - b * J;
    const float* src = hm + b * sb + j * sj;
    const bool interp = P != H || Q != W;
    const bool odd = j & 1;          // map j is channel j of the tensor up_bilinear_fwd would have run on
    if (STAGE) {
        for (int i = tid; i < H * W; i += 256) tile[i] = src[i * sp];
        __syncthreads();
    }
    auto at = [&](int k) -> float { return STAGE ? tile[k] : src[k * sp]; };
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    const int PQ = P * Q;
    for (int i = tid; i < PQ; i += 256) {
        float v;
        if (interp) {
            const int p = (int)fdiv((uint32_t)i, fQ), q = i - p * Q;
            const BilTap th = bil_tap(sh, p, H), tw = bil_tap(sw, q, W);
            const float a00 = at(th.i0 * W + tw.i0), a01 = at(th.i0 * W + tw.i1), a10 = at(th.i1 * W + tw.i0),
                        a11 = at(th.i1 * W + tw.i1);
            v = odd ? bil_mix<1>(th.l0, th.l1, tw.l0, tw.l1, a00, a01, a10, a11)
                    : bil_mix<0>(th.l0, th.l1, tw.l0, tw.l1, a00, a01, a10, a11);
        } else {
            v = src[i * sp];
        }
        if (am_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        float ov = __shfl_down(bv, off);
        int oi = __shfl_down(bi, off);
        if (am_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if ((tid & 63) == 0) {
        red_v[tid >> 6] = bv;
        red_i[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k)
            if (am_better(red_v[k], red_i[k], bv, bi)) {
                bv = red_v[k];
                bi = red_i[k];
            }
        const int o = CLIP ? (int)clip_image(b, cB, cT) * J + j : map;
        if (idx) idx[o] = bi;
        float keep = bv > 0.f ? 1.f : 0.f;
        preds[o * 2] = (float)(bi % Q) * keep;
        preds[o * 2 + 1] = (float)(bi / Q) * keep;
        maxvals[o] = bv;
    }
}

// ---- multi-person decode (the step after the path for the box head; utils/uniPose.py:14-200) -----------------------
// Peaks of a map as the reference finds them: negatives clamped to 0, then `maximum_filter(3x3) == map` XOR the eroded
// zero background (scipy, borders reflected / counted as background) — which is exactly: value > 0 and >= each of its
// in-bounds 8 neighbours (plateaus mark every member).
// The predicate itself, for pixel i = h * W + w of one map read through at(pixel): peak_mask_kernel and persons_kernel share it.
template <typename At>
__device__ __forceinline__ bool is_peak(At at, int i, int h, int w, int H, int W) {
    const float v = at(i);
    bool peak = v > 0.f;
    for (int dh = -1; dh <= 1; ++dh)
        for (int dw = -1; dw <= 1; ++dw) {
            const int hh = h + dh, ww = w + dw;
            if (hh < 0 || ww < 0 || hh >= H || ww >= W) continue;
            peak = peak && v >= at(i + dh * W + dw);
        }
    return peak;
}
__global__ void __launch_bounds__(256) peak_mask_kernel(const float* maps, long long total, int H, int W, uint8_t* mask) {
    long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int w = (int)(e % W);
    const int h = (int)((e / W) % H);
    const float* m = maps + (e - ((long long)h * W + w));
    mask[e] = is_peak([&](int k) -> float { return m[k]; }, h * W + w, h, w, H, W) ? 1 : 0;
}
// argmax of channels ch0 .. ch0+nch-1 inside one box per person: one wavefront per (person, channel); position
// relative to the box, first maximum in the row-major order of the BOX (np.argmax of the sliced array)
// The reduction, by one whole wavefront: the index (row-major inside the box of bh x bw at (r0, c0)) of the first maximum of a
// map read through at(row, col); the result is valid in lane 0.  box_argmax_kernel and persons_kernel share it.
template <typename At>
__device__ __forceinline__ int box_first_max(At at, int r0, int c0, int bh, int bw, int lane) {
    const int n = bh * bw;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const int rr = i / bw, cc = i - rr * bw;
        const float v = at(r0 + rr, c0 + cc);
        if (am_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        float ov = __shfl_down(bv, off);
        int oi = __shfl_down(bi, off);
        if (am_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    return bi == 0x7fffffff ? 0 : bi;   // a box of -inf only: np.argmax returns 0
}
__global__ void __launch_bounds__(256) box_argmax_kernel(const float* maps, int H, int W, const int32_t* boxes, int P,
                                                         int ch0, int nch, int32_t* out_hw) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (job >= P * nch) return;
    const int p = job / nch, c = job - p * nch;
    const int r0 = boxes[p * 4], r1 = boxes[p * 4 + 1], c0 = boxes[p * 4 + 2], c1 = boxes[p * 4 + 3];
    const int bw = c1 - c0;
    const float* m = maps + (size_t)(ch0 + c) * H * W;
    const int bi = box_first_max([&](int r, int cc) -> float { return m[(size_t)r * W + cc]; }, r0, c0, r1 - r0, bw, lane);
    if (lane == 0) {
        out_hw[job * 2] = bi / bw;
        out_hw[job * 2 + 1] = bi - (bi / bw) * bw;
    }
}

// ---- multi-person decode of a whole batch in one launch: one workgroup per sample (up_persons_decode) ---------------------------
// What ops.uniPose_kpts does with up_peak_mask, torch.nonzero, host lists and up_box_argmax, for every sample, without the host.
// Three phases, a barrier between them:
//  1. ordered compaction: the five box maps (centre, tl, bl, tr, br; staged in LDS (STAGE) when 5 * H * W <= DECODE_LDS, read
//     through L2 otherwise) are walked together in row-major chunks of 256 pixels.  Every thread tests its pixel in the five maps
//     (is_peak); the five flags travel as 10-bit fields of two words (a chunk counts at most 256 per map) through one scan: inclusive
//     suffix sums inside the wavefront with __shfl_down, the four wavefront totals through LDS, so
//     slot = running base + peaks of earlier wavefronts + (total of this wavefront - suffix sum).  The first max_persons peaks of
//     every map land in its LDS list as flat pixel indices, in row-major order; the running bases end as the true lengths.
//  2. status walk: thread 0 walks the centre peaks in the reference's order of checks and publishes n and the status.
//  3. box argmax: one wavefront per (person, joint) job with box_first_max, the joint maps read from global memory through the
//     strides; then the centre and corner rows.
constexpr int PERSONS_FIELD = 10;       // bits per map in the packed flags
template <bool STAGE>
__global__ void __launch_bounds__(256) persons_kernel(const float* maps, int64_t sb, int64_t sj, int64_t sp, int H, int W, FastDiv fW,
                                                      int box_ch0, int joint_ch0, int njoints, int max_persons, int32_t* count,
                                                      int32_t* status, int32_t* kpts) {
    __shared__ float tile[STAGE ? DECODE_LDS : 1];
    __shared__ int32_t list[5][UP_PERSONS_CAP];
    __shared__ uint32_t wsum[2][4][2];                  // [chunk parity][wavefront][word]: one barrier per chunk is enough
    __shared__ int s_n;
    __shared__ int s_status;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;
    const float* src = maps + b * sb;
    const float* box = src + box_ch0 * sj;
    if (STAGE) {
        for (int m = 0; m < 5; ++m)
            for (int i = tid; i < HW; i += 256) tile[m * HW + i] = box[m * sj + i * sp];
        __syncthreads();
    }
    int base[5] = {0, 0, 0, 0, 0};
    for (int c0 = 0, par = 0; c0 < HW; c0 += 256, par ^= 1) {
        const int i = c0 + tid;
        uint32_t flag[2] = {0u, 0u};
        if (i < HW) {
            const int h = (int)fdiv((uint32_t)i, fW), w = i - h * W;
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                auto at = [&](int k) -> float { return STAGE ? tile[m * HW + k] : box[m * sj + k * sp]; };
                if (is_peak(at, i, h, w, H, W)) flag[m / 3] |= 1u << (PERSONS_FIELD * (m % 3));
            }
        }
        uint32_t suf[2] = {flag[0], flag[1]};           // -> peaks at lanes >= this one, per field
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t0 = __shfl_down(suf[0], off), t1 = __shfl_down(suf[1], off);
            if (lane + off < 64) {
                suf[0] += t0;
                suf[1] += t1;
            }
        }
        if (lane == 0) {
            wsum[par][wave][0] = suf[0];
            wsum[par][wave][1] = suf[1];
        }
        __syncthreads();
        uint32_t before[2] = {0u, 0u}, total[2] = {0u, 0u};
        for (int k = 0; k < 4; ++k)
            for (int q = 0; q < 2; ++q) {
                if (k <= wave) before[q] += wsum[par][k][q];     // includes this wavefront: its suffix sum goes off below
                total[q] += wsum[par][k][q];
            }
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const int sh = PERSONS_FIELD * (m % 3);
            const uint32_t mask = (1u << PERSONS_FIELD) - 1u;
            const int slot = base[m] + (int)(((before[m / 3] - suf[m / 3]) >> sh) & mask);
            if (((flag[m / 3] >> sh) & 1u) && slot < max_persons) list[m][slot] = i;
            base[m] += (int)((total[m / 3] >> sh) & mask);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int n = base[0];
        int st = UP_PERSONS_OK;
        if (n > max_persons) {
            st = UP_PERSONS_OVERFLOW;
        } else {
            for (int idx = 0; idx < n && st == UP_PERSONS_OK; ++idx) {
                if (idx >= base[1] || idx >= base[4]) {          // tl[idx], br[idx]
                    st = UP_PERSONS_MISSING_CORNER;
                    break;
                }
                const int tl = list[1][idx], br = list[4][idx];
                const int r0 = tl / W, r1 = br / W;
                if (r1 <= r0 || br - r1 * W <= tl - r0 * W) st = UP_PERSONS_EMPTY_BOX;
                else if (idx >= base[2] || idx >= base[3]) st = UP_PERSONS_MISSING_CORNER;      // bl[idx], tr[idx]
            }
        }
        count[b] = n;
        status[b] = st;
        s_n = n;
        s_status = st;
    }
    __syncthreads();
    if (s_status != UP_PERSONS_OK) return;
    const int n = s_n, rows = njoints + 5;
    int32_t* out = kpts + (size_t)b * max_persons * rows * 2;
    for (int job = wave; job < n * njoints; job += 4) {
        const int p = job / njoints, j = job - p * njoints;
        const int tl = list[1][p], br = list[4][p];
        const int r0 = tl / W, c0 = tl - r0 * W, r1 = br / W, c1 = br - r1 * W;
        const int bw = c1 - c0;
        const float* m = src + (joint_ch0 + j) * sj;
        const int bi = box_first_max([&](int r, int c) -> float { return m[(r * W + c) * sp]; }, r0, c0, r1 - r0, bw, lane);
        if (lane == 0) {
            out[(p * rows + j) * 2] = c0 + bi % bw;
            out[(p * rows + j) * 2 + 1] = r0 + bi / bw;
        }
    }
    for (int t = tid; t < n * 5; t += 256) {
        const int p = t / 5, m = t - p * 5;
        const int pix = list[m][p], r = pix / W;
        out[(p * rows + njoints + m) * 2] = pix - r * W;
        out[(p * rows + njoints + m) * 2 + 1] = r;
    }
}

// ---- training targets (the step before the path: lsp_lspet_data.py:224-245, mpii_data.py:165-187) ----------------
// Gaussian joint maps exactly as the loaders build them: float64 exp(-D2 / 2.0 / sigma / sigma) on the integer pixel
// grid (utils/utils.py:200-203), clipped to <= 1, values < 0.0099 set to 0, then stored as float32; channel 0 is
// 1 - max over the joint channels (float32).  The joint centre is int(coordinate) / stride like the loaders compute it.
__device__ __forceinline__ float target_gauss(double x, double y, double cx, double cy, double sigma) {
    const double dx = x - cx, dy = y - cy;
    const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    double v = exp(-d2 / 2.0 / sigma / sigma);
    if (v > 1.0) v = 1.0;
    if (v < 0.0099) v = 0.0;
    return (float)v;
}
__global__ void __launch_bounds__(256) heatmap_target_kernel(const double* kpt, int K, int H, int W, double stride,
                                                             double sigma, float* out, long long total /* B*H*W */) {
    long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int x = (int)(e % W);
    const long long t = e / W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    float* o = out + (size_t)b * (K + 1) * H * W + (size_t)y * W + x;
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const double cx = (double)(long long)kpt[((size_t)b * K + k) * 2] * 1.0 / stride;       // int(kpt) * 1.0 / stride
        const double cy = (double)(long long)kpt[((size_t)b * K + k) * 2 + 1] * 1.0 / stride;
        const float g = target_gauss((double)x, (double)y, cx, cy, sigma);
        o[(size_t)(k + 1) * H * W] = g;
        mx = fmaxf(mx, g);
    }
    o[0] = 1.0f - mx;
}
__global__ void __launch_bounds__(256) gaussian_map_kernel(const double* center, int H, int W, double sigma, float* out,
                                                           long long total /* N*H*W */) {
    long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int x = (int)(e % W);
    const long long t = e / W;
    const int y = (int)(t % H);
    const int n = (int)(t / H);
    out[e] = target_gauss((double)x, (double)y, center[2 * n], center[2 * n + 1], sigma);
}
// The pooled centre map straight from the centre (up_center_pool and its clip forms, include/unipose_hip.h): avgpool9s8_window over
// target_gauss, so the (N, 1, H, W) maps never exist.  One thread per pooled pixel, consecutive threads consecutive q; only channel
// coff of a pixel is written.  CLIP: frame-major rows from batch-major centres.  FLIP: the plane is the mirrored map, whose column w
// holds target_gauss at column W - 1 - w of the map about (cx, cy) — not a Gaussian about W - 1 - cx, whose subtraction rounds
// differently.
// skip: a tap with d2 > 9.4 * sigma^2 is not evaluated.  target_gauss returns 0 where exp(-d2 / 2 / sigma / sigma) < 0.0099, that is
// where d2 / (2 sigma^2) > ln(1 / 0.0099) = 4.6152; the bound asks for 4.7, a margin of 1.8 %, against the few 1e-16 relative error
// of the products and divisions on both sides and exp's last-place error (exp(-4.7) = 0.00910).  d2 is target_gauss's own
// statement, so it is the value target_gauss would test; a skipped tap adds the +0.0f target_gauss would have returned.  A NaN
// centre gives a NaN d2, which fails the comparison and is evaluated: NaN propagates.  An infinite centre gives d2 = inf: skipped
// as the 0 that exp(-inf) is (at a sigma so large that the bound is inf too, it is evaluated).
template <bool CLIP, bool FLIP, bool STRIDED>
__device__ __forceinline__ void center_pool_body(const double* center, double sigma, double skip, float* y, int ldy, int coff, int B,
                                                 int T, int H, int W, int P, int Q, int64_t total, int FI, int first) {
    UP_GRID_STRIDE(i, total) {
        const int q = (int)(i % Q);
        const int64_t t = i / Q;
        const int p = (int)(t % P);
        const int64_t f = t / P;
        const int64_t n = CLIP ? clip_image(f, B, T) : f;
        const double cx = center[2 * n], cy = center[2 * n + 1];
        const int64_t o = STRIDED ? (clip_dest<true>(f, B, FI, first) * P + p) * Q + q : i;
        y[o * ldy + coff] = avgpool9s8_window<FLIP>(H, W, p, q, [=](int h, int c) {
            const double dx = (double)c - cx, dy = (double)h - cy;
            const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
            return d2 > skip ? 0.f : target_gauss((double)c, (double)h, cx, cy, sigma);
        });
    }
}
template <bool CLIP, bool FLIP>
__global__ void __launch_bounds__(256) center_pool_kernel(const double* center, double sigma, double skip, float* y, int ldy, int coff,
                                                          int B, int T, int H, int W, int P, int Q, int64_t total) {
    center_pool_body<CLIP, FLIP, false>(center, sigma, skip, y, ldy, coff, B, T, H, W, P, Q, total, B, 0);
}
template <bool FLIP>
__global__ void __launch_bounds__(256) clip_center_pool_strided_kernel(const double* center, double sigma, double skip, float* y, int ldy,
                                                                       int coff, int B, int T, int H, int W, int P, int Q, int64_t total,
                                                                       int FI, int first) {
    center_pool_body<true, FLIP, true>(center, sigma, skip, y, ldy, coff, B, T, H, W, P, Q, total, FI, first);
}
// Box-head targets (getBoundingBox, lsp_lspet_data.py:71-113 / bbc_data.py:23-72), every statement in float64 like Python's
// floats; int() is trunc().  The reference calls the SECOND coordinate x and the first y, bounds x by `width` and y by `height`,
// and then centres the Gaussian's column on the y-derived cell and its row on the x-derived one: kept as it is.
__device__ __forceinline__ double box_cell(double v, double stride, double lim) {     // int(min(int(v / stride), lim))
    const double q = trunc(v / stride);
    return trunc(lim < q ? lim : q);
}
__global__ void __launch_bounds__(256) box_target_kernel(const double* kpt, int K, int height, int width, double stride,
                                                         double sigma, int h, int w, float* out, int32_t* status,
                                                         long long total /* B*h*w */) {
    long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int x = (int)(e % w);
    const long long t = e / w;
    const int y = (int)(t % h);
    const int b = (int)(t / h);
    bool any = false;
    double xlo = 0, xhi = 0, ylo = 0, yhi = 0;
    for (int k = 0; k < K; ++k) {
        const double k0 = kpt[((size_t)b * K + k) * 2], k1 = kpt[((size_t)b * K + k) * 2 + 1];
        if (!(k1 >= 0.0 || k0 >= 0.0)) continue;                 // :76 — an OR: one coordinate >= 0 is enough
        if (!any) { xlo = xhi = k1; ylo = yhi = k0; any = true; continue; }
        xlo = k1 < xlo ? k1 : xlo;  xhi = k1 > xhi ? k1 : xhi;
        ylo = k0 < ylo ? k0 : ylo;  yhi = k0 > yhi ? k0 : yhi;
    }
    double x_min = 0, x_max = 0, y_min = 0, y_max = 0;           // no counted joint: the zero box of bbc_data.py:32-36
    if (any) {                                                   // :80-83
        x_min = trunc(0.0 > xlo ? 0.0 : xlo);
        x_max = trunc((double)width < xhi ? (double)width : xhi);
        y_min = trunc(0.0 > ylo ? 0.0 : ylo);
        y_max = trunc((double)height < yhi ? (double)height : yhi);
    }
    const double limh = (double)height / stride - 1.0, limw = (double)width / stride - 1.0;
    // :97-101, then :106-108: the column is coord[i][0] (from y), the row coord[i][1] (from x)
    const double col[3] = {box_cell((y_min + y_max) / 2.0, stride, limh), box_cell(y_min, stride, limh), box_cell(y_max, stride, limh)};
    const double row[3] = {box_cell((x_min + x_max) / 2.0, stride, limw), box_cell(x_min, stride, limw), box_cell(x_max, stride, limw)};
    const size_t hw = (size_t)h * w;
    float* o = out + (size_t)b * 5 * hw + (size_t)y * w + x;
    o[0] = target_gauss((double)x, (double)y, col[0], row[0], sigma);          // centre
    o[hw] = target_gauss((double)x, (double)y, col[1], row[1], sigma);         // (y_min, x_min): top-left
    o[2 * hw] = target_gauss((double)x, (double)y, col[1], row[2], sigma);     // (y_min, x_max): bottom-left
    o[3 * hw] = target_gauss((double)x, (double)y, col[2], row[1], sigma);     // (y_max, x_min): top-right
    o[4 * hw] = target_gauss((double)x, (double)y, col[2], row[2], sigma);     // (y_max, x_max): bottom-right
    if (status && x == 0 && y == 0) status[b] = any ? UP_BOX_OK : UP_BOX_NO_VISIBLE_JOINT;
}
// (pixel - mean) / std, HWC -> CHW (Mytransforms.to_tensor + normalize, Mytransforms.py:10-41)
__global__ void __launch_bounds__(256) normalize_image_kernel(const float* img, int C, int HW, float mean, float stdv,
                                                              float* out, long long total /* B*HW*C */) {
    long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const long long t = e / C;
    const int p = (int)(t % HW);
    const long long b = t / HW;
    out[((size_t)b * C + c) * HW + p] = (img[e] - mean) / stdv;
}
// Augmentation as ONE resample (RandomResized + RandomRotate + RandomCrop + RandomHorizontalFlip of utils/Mytransforms.py composed
// into one affine map by unipose_amd/augment.py), fused with to_tensor + normalize: one thread per output pixel, all C channels;
// the semantics, operation by operation, are in include/unipose_hip.h.  Coordinates in float64, the blend in float32 with fused
// multiply-adds written out (fma / fmaf, the same single rounding on the device and in the host build); a tap outside the sample's
// valid extent is the border constant and is not loaded.  Store-bound: the four taps of neighbouring threads share cache lines.
__device__ __forceinline__ float aug_px(const float* p) { return *p; }
__device__ __forceinline__ float aug_px(const uint8_t* p) { return (float)*p; }
// One output pixel (column u, row v) of a sample under the map m, read from source image `img` of valid extent Hv x Wv (Hv = Wv = 0:
// no image, every tap is border): val[c] = the normalised value of channel c < C, 0 for C <= c < 4.  The ONE statement of the
// resample's arithmetic: up_augment_image and up_crop_to_nhwc both store what this returns.
template <typename T>
__device__ __forceinline__ void aug_sample(const T* src, int64_t img, int Hs, int Ws, int C, int Hv, int Wv, const double* m, int u,
                                           int v, float border, float mean, float stdv, float out[4]) {
    const double sx = fma(m[0], (double)u, fma(m[1], (double)v, m[2]));
    const double sy = fma(m[3], (double)u, fma(m[4], (double)v, m[5]));
    const double x0d = floor(sx), y0d = floor(sy);
    // decided in float64 (false for NaN and for anything too large to index): otherwise all four taps are border
    const bool near = x0d >= -1.0 && x0d <= (double)(Wv - 1) && y0d >= -1.0 && y0d <= (double)(Hv - 1);
    float val[4] = {border, border, border, border};
    if (near) {
        const int x0 = (int)x0d, y0 = (int)y0d;      // -1 .. Wv-1, -1 .. Hv-1
        const float fx = (float)(sx - x0d), fy = (float)(sy - y0d);
        const bool xa = x0 >= 0, xb = x0 + 1 < Wv, ya = y0 >= 0, yb = y0 + 1 < Hv;
        const int64_t p = ((img * Hs + y0) * Ws + x0) * C;        // may lie before the image: read at valid taps only
        const int64_t row = (int64_t)Ws * C;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < C) {
                const float v00 = ya && xa ? aug_px(src + p + c) : border;
                const float v01 = ya && xb ? aug_px(src + p + C + c) : border;
                const float v10 = yb && xa ? aug_px(src + p + row + c) : border;
                const float v11 = yb && xb ? aug_px(src + p + row + C + c) : border;
                const float top = fmaf(fx, v01 - v00, v00);
                const float bot = fmaf(fx, v11 - v10, v10);
                val[c] = fmaf(fy, bot - top, top);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = c < C ? (val[c] - mean) / stdv : 0.f;
}
template <typename T>
__global__ void __launch_bounds__(256) augment_image_kernel(const T* src, int Hs, int Ws, int C, const int32_t* valid_hw,
                                                            const double* inv, int frames_per_map, float border, float mean,
                                                            float stdv, float* out, int Ho, int Wo,
                                                            long long total /* B*Ho*Wo */) {
    UP_GRID_STRIDE(e, total) {
        const int u = (int)(e % Wo);
        const int64_t t = e / Wo;
        const int v = (int)(t % Ho);
        const int64_t b = t / Ho;
        int Hv = Hs, Wv = Ws;
        if (valid_hw) {                                  // device data: cut to the buffer, never trusted beyond it
            Hv = min(max(valid_hw[2 * b], 0), Hs);
            Wv = min(max(valid_hw[2 * b + 1], 0), Ws);
        }
        float val[4];
        aug_sample(src, b, Hs, Ws, C, Hv, Wv, inv + (b / frames_per_map) * 6, u, v, border, mean, stdv, val);
        const int64_t hw = (int64_t)Ho * Wo;
        float* o = out + b * C * hw + (int64_t)v * Wo + u;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) o[c * hw] = val[c];
    }
}
// The crop in front of the network (up_crop_to_nhwc, include/unipose_hip.h): up_augment_image's resample written straight into the
// trunk's NHWC input and, from the same thread, into the mirrored input of the flip test.  Sample b reads source frame frame_of[b]
// (several persons of one frame share it); an index outside 0 .. F-1 is device data and makes the sample all border, nothing loaded.
// One thread per output pixel, consecutive threads consecutive u: with ld = 4 a wave stores 1 KiB of consecutive pixels per
// instruction, forwards into y and backwards into y_flip; the quads beyond the first are the zero pad channels.
// CLIP (up_clip_crop_to_nhwc): the outputs are frame-major, image t * cB + b holds sample b * cT + t of the batch-major frame_of
// and inv; everything else is the same code.
// STRIDED (up_clip_crop_to_nhwc_strided): image t * FI + first + b of both outputs; the source is read once all the same.
template <typename T, bool CLIP, bool STRIDED>
__device__ __forceinline__ void crop_to_nhwc_body(const T* src, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                                                  const int32_t* valid_hw, const double* inv, float border, float mean, float stdv,
                                                  float* y, float* yf, int Ho, int Wo, int ld, long long total /* B*Ho*Wo */, int cB,
                                                  int cT, int FI, int first) {
    UP_GRID_STRIDE(e0, total) {
        const int u = (int)(e0 % Wo);
        const int64_t t = e0 / Wo;
        const int v = (int)(t % Ho);
        const int64_t b = CLIP ? clip_image(t / Ho, cB, cT) : t / Ho;     // the sample; e is the output pixel
        const int64_t e = STRIDED ? (clip_dest<true>(t / Ho, cB, FI, first) * Ho + v) * Wo + u : e0;
        int64_t f = frame_of ? (int64_t)frame_of[b] : b;
        int Hv = 0, Wv = 0;
        if (f >= 0 && f < F) {
            Hv = Hs;
            Wv = Ws;
            if (valid_hw) {                              // per source frame; device data: cut to the buffer
                Hv = min(max(valid_hw[2 * f], 0), Hs);
                Wv = min(max(valid_hw[2 * f + 1], 0), Ws);
            }
        } else {
            f = 0;                                       // no such frame: no tap is valid, no address is used
        }
        float val[4];
        aug_sample(src, f, Hs, Ws, C, Hv, Wv, inv + b * 6, u, v, border, mean, stdv, val);
        const float4 q = make_float4(val[0], val[1], val[2], val[3]), z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y) {
            float* d = y + e * ld;
            *reinterpret_cast<float4*>(d) = q;
            for (int c = 4; c < ld; c += 4) *reinterpret_cast<float4*>(d + c) = z;
        }
        if (yf) {
            float* d = yf + (e - u + (Wo - 1 - u)) * ld;
            *reinterpret_cast<float4*>(d) = q;
            for (int c = 4; c < ld; c += 4) *reinterpret_cast<float4*>(d + c) = z;
        }
    }
}
template <typename T, bool CLIP>
__global__ void __launch_bounds__(256) crop_to_nhwc_kernel(const T* src, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                                                           const int32_t* valid_hw, const double* inv, float border, float mean,
                                                           float stdv, float* y, float* yf, int Ho, int Wo, int ld,
                                                           long long total /* B*Ho*Wo */, int cB, int cT) {
    crop_to_nhwc_body<T, CLIP, false>(src, F, Hs, Ws, C, frame_of, valid_hw, inv, border, mean, stdv, y, yf, Ho, Wo, ld, total, cB, cT,
                                      cB, 0);
}
template <typename T>
__global__ void __launch_bounds__(256) clip_crop_to_nhwc_strided_kernel(const T* src, int F, int Hs, int Ws, int C,
                                                                        const int32_t* frame_of, const int32_t* valid_hw,
                                                                        const double* inv, float border, float mean, float stdv,
                                                                        float* y, float* yf, int Ho, int Wo, int ld, long long total,
                                                                        int cB, int cT, int FI, int first) {
    crop_to_nhwc_body<T, true, true>(src, F, Hs, Ws, C, frame_of, valid_hw, inv, border, mean, stdv, y, yf, Ho, Wo, ld, total, cB, cT, FI,
                                     first);
}

// ---- PCK / PCKh accuracy on joint coordinates (utils/evaluate.py:5-29,58-172) -------------------------------------
// One workgroup; thread j owns joint j.  Arithmetic types follow the reference under NumPy >= 2: coordinates float32,
// head / torso sizes float32 (np.linalg.norm of float32), thresholds float32 products (python float * np.float32),
// normalised distances float64 (float32 coordinates divided by the float64 [H/10, W/10]).
__device__ __forceinline__ float pck_norm2(float x, float y) { return sqrtf(x * x + y * y); }
__device__ void pck_scales(const float* t0 /* (J,2) of sample 0 */, int dataset, float& head, float& torso) {
    auto X = [&](int j) { return t0[2 * j]; };
    auto Y = [&](int j) { return t0[2 * j + 1]; };
    auto midx = [&](int a, int b) { return (X(a) + X(b)) / 2.f; };
    auto midy = [&](int a, int b) { return (Y(a) + Y(b)) / 2.f; };
    switch (dataset) {
        case UP_DS_LSP:
            head = pck_norm2(X(14) - X(13), Y(14) - Y(13));
            torso = pck_norm2(X(13) - midx(3, 4), Y(13) - midy(3, 4));
            break;
        case UP_DS_COCO:
            head = pck_norm2(X(4) - X(5), Y(4) - Y(5));
            torso = pck_norm2(X(13) - midx(12, 13), Y(13) - midy(12, 13));
            break;
        case UP_DS_PENN_ACTION:
            head = pck_norm2(X(0) - midx(1, 2), Y(0) - midy(1, 2));
            torso = pck_norm2(midx(1, 2) - midx(7, 8), midy(1, 2) - midy(7, 8));
            break;
        case UP_DS_NTID:
            head = 2.f * pck_norm2(X(4) - X(3), Y(4) - Y(3));
            torso = pck_norm2(X(3) - X(1), Y(3) - Y(1));
            break;
        case UP_DS_POSETRACK:
            head = 2.f * pck_norm2(X(1) - X(2), Y(1) - Y(2));
            torso = pck_norm2(midx(12, 13) - midx(6, 7), midy(12, 13) - midy(6, 7));
            break;
        case UP_DS_BBC:   // the reference subtracts the neck POINT from the x coordinate of joint 1 (evaluate.py:147-149)
            head = pck_norm2(X(1) - midx(6, 7), Y(1) - midy(6, 7));
            torso = pck_norm2(3.f * (X(1) - midx(6, 7)), 3.f * (X(1) - midy(6, 7)));
            break;
        default:          // UP_DS_MPII
            head = pck_norm2(X(9) - X(10), Y(9) - Y(10));
            torso = fabsf(X(7) - X(8));
            break;
    }
}
__global__ void __launch_bounds__(256) pck_kernel(const float* pred, const float* tgt, int B, int J, int H, int W,
                                                  int dataset, float thr_pck, float thr_pckh, double* acc, double* pck,
                                                  double* pckh, double* visible, int32_t* cnt) {
    __shared__ double s_acc[256], s_pck[256], s_pckh[256];
    const int j = threadIdx.x;
    float head, torso;
    pck_scales(tgt, dataset, head, torso);
    const double t_h = (double)(thr_pckh * head), t_k = (double)(thr_pck * torso);   // float32 products
    const double nx = (double)H / 10.0, ny = (double)W / 10.0;   // x is divided by H/10, y by W/10 (evaluate.py:68-70)
    if (j < J) {
        int valid = 0, c0 = 0, ch = 0, ck = 0;
        for (int n = 0; n < B; ++n) {
            const float tx = tgt[(n * J + j) * 2], ty = tgt[(n * J + j) * 2 + 1];
            if (tx > 1.f && ty > 1.f) {
                const double dx = (double)pred[(n * J + j) * 2] / nx - (double)tx / nx;
                const double dy = (double)pred[(n * J + j) * 2 + 1] / ny - (double)ty / ny;
                const double d = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));   // no FMA contraction
                ++valid;
                c0 += d < 0.5;
                ch += d < t_h;
                ck += d < t_k;
            }
        }
        s_acc[j] = valid ? c0 * 1.0 / valid : -1.0;
        s_pckh[j] = valid ? ch * 1.0 / valid : -1.0;
        s_pck[j] = valid ? ck * 1.0 / valid : -1.0;
    }
    __syncthreads();
    if (j == 0) {   // the averages, summed in joint order like the reference's loops
        int c = 0;
        double sa = 0.0, sh = 0.0, sk = 0.0;
        for (int i = 0; i < J; ++i) {
            const bool vis = s_acc[i] >= 0.0;
            visible[i] = vis ? 1.0 : 0.0;
            if (vis) {
                sa += s_acc[i];
                ++c;
            }
            acc[i] = vis ? s_acc[i] : 0.0;
            if (s_pckh[i] >= 0.0) sh += s_pckh[i];
            pckh[i] = s_pckh[i] >= 0.0 ? s_pckh[i] : 0.0;
            if (s_pck[i] >= 0.0) sk += s_pck[i];
            pck[i] = s_pck[i] >= 0.0 ? s_pck[i] : 0.0;
        }
        if (c) {
            acc[0] = sa / c;
            pckh[0] = sh / c;
            pck[0] = sk / c;
        }
        *cnt = c;
    }
}

// ---- the evaluation protocol around the forward: flip test and final_preds (utils/extra_utils; include/unipose_hip.h) ---------
// up_nchw_to_nhwc with the mirror folded in: the NHWC pixel (h, w) takes the NCHW pixel (h, W - 1 - w); pad channels as there
__global__ void __launch_bounds__(256) nchw_to_nhwc_flip_kernel(const float* x, float* y, int C, int W, int HW, int ld,
                                                                int64_t npix) {
    UP_GRID_STRIDE(i, npix) {
        int64_t n = i / HW;
        int hw = (int)(i - n * HW);
        int h = hw / W, w = hw - h * W;
        const float* src = x + n * C * HW + h * W + (W - 1 - w);
        float* dst = y + i * ld;
        for (int c = 0; c < ld; ++c) st1(dst + c, nchw_at(src, C, HW, c));
    }
}

// The flip test's combine step: out[b, j, y, x] = 0.5f * (a[b, j, y, x] + f[b, perm[j], y, W - 1 - x]), one add and one multiply,
// each rounded once.  One thread per element; JFAST: consecutive threads walk the channels of a pixel (an NHWC output), else the
// pixels of a map (NCHW).  The permutation travels by value: 256 bytes of kernel arguments.
struct FlipPerm {
    uint8_t v[256];
};
// CLIP (up_clip_flip_merge): a two-level batch index, image t * B + b of the walk read at t * ist + b * isb and written at
// t * ost + b * osb — the two halves of a 2B-wide frame-major tensor merged into a compact one; else ist / ost / B are not read.
template <bool JFAST, bool CLIP>
__device__ __forceinline__ void flip_merge_body(const float* a, const float* f, int64_t ist, int64_t isb, int64_t isj, int64_t isp,
                                                int B, int J, int H, int W, const FlipPerm& perm, float* out, int64_t ost, int64_t osb,
                                                int64_t osj, int64_t osp, int64_t total) {
    const int HW = H * W;
    UP_GRID_STRIDE(i, total) {
        int64_t b;
        int j, pix;
        if (JFAST) {
            const int64_t bp = i / J;
            j = (int)(i - bp * J);
            b = bp / HW;
            pix = (int)(bp - b * HW);
        } else {
            const int64_t bj = i / HW;
            pix = (int)(i - bj * HW);
            b = bj / J;
            j = (int)(bj - b * J);
        }
        const int y = pix / W, x = pix - y * W;
        int64_t ib = b * isb, ob = b * osb;
        if (CLIP) {
            const int64_t t = b / B, s = b - t * B;
            ib = t * ist + s * isb;
            ob = t * ost + s * osb;
        }
        const float va = a[ib + j * isj + pix * isp];
        const float vf = f[ib + (int64_t)perm.v[j] * isj + (int64_t)(y * W + (W - 1 - x)) * isp];
        out[ob + j * osj + pix * osp] = __fmul_rn(0.5f, va + vf);
    }
}
template <bool JFAST>
__global__ void __launch_bounds__(256) flip_merge_kernel(const float* a, const float* f, int64_t isb, int64_t isj, int64_t isp,
                                                         int J, int H, int W, FlipPerm perm, float* out, int64_t osb, int64_t osj,
                                                         int64_t osp, int64_t total) {
    flip_merge_body<JFAST, false>(a, f, 0, isb, isj, isp, 1, J, H, W, perm, out, 0, osb, osj, osp, total);
}
template <bool JFAST>
__global__ void __launch_bounds__(256) clip_flip_merge_kernel(const float* a, const float* f, int64_t ist, int64_t isb, int64_t isj,
                                                              int64_t isp, int B, int J, int H, int W, FlipPerm perm, float* out,
                                                              int64_t ost, int64_t osb, int64_t osj, int64_t osp, int64_t total) {
    flip_merge_body<JFAST, true>(a, f, ist, isb, isj, isp, B, J, H, W, perm, out, ost, osb, osj, osp, total);
}

// final_preds (utils/extra_utils/evaluation.py:75-97): one wavefront per (b, j) map like argmax_kernel, then lane 0 does the
// quarter-pixel refinement and the way back through the (2, 3) float64 inverse of the crop transform; every product and sum
// of that transform is rounded on its own, in numpy's order (no FMA).
// CLIP: frame-major images, batch-major results and `inv` rows, as in decode_kernel.
template <bool CLIP>
__global__ void __launch_bounds__(256) final_preds_kernel(const float* hm, int64_t sb, int64_t sj, int64_t sp, int maps, int J,
                                                          int H, int W, int res0, int res1, const double* inv, float* preds,
                                                          float* coords, float* maxvals, int cB, int cT) {
    int map = blockIdx.x * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (map >= maps) return;
    const int b = map / J, j = map - b * J;
    const float* p = hm + b * sb + j * sj;
    const int HW = H * W;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < HW; i += 64) {
        float v = p[i * sp];
        if (am_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        float ov = __shfl_down(bv, off);
        int oi = __shfl_down(bi, off);
        if (am_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane != 0) return;
    const int ob = CLIP ? (int)clip_image(b, cB, cT) : b;     // the row of the results and of `inv`
    map = ob * J + j;
    maxvals[map] = bv;
    float x = 0.f, y = 0.f;
    if (bv > 0.f) {                 // a NaN maximum masks to 0 as maxval.gt(0) does
        x = (float)(bi % W + 1);
        y = (float)(bi / W + 1);
    }
    const int px = (int)x, py = (int)y;
    // px < W and py < H hold wherever the reference does not raise IndexError: they keep the four reads inside the map
    if (px > 1 && px < res0 && py > 1 && py < res1 && px < W && py < H) {
        const float r = p[((py - 1) * W + px) * sp], l = p[((py - 1) * W + px - 2) * sp];
        const float d = p[(py * W + px - 1) * sp], u = p[((py - 2) * W + px - 1) * sp];
        x += 0.25f * (float)((r > l) - (r < l));
        y += 0.25f * (float)((d > u) - (d < u));
    }
    x += 0.5f;
    y += 0.5f;
    if (coords) {
        coords[map * 2] = x;
        coords[map * 2 + 1] = y;
    }
    if (inv) {
        const double* m = inv + (int64_t)ob * 6;
        const double p0 = (double)x - 1.0, p1 = (double)y - 1.0;
        const double v0 = __dadd_rn(__dadd_rn(__dmul_rn(m[0], p0), __dmul_rn(m[1], p1)), m[2]);
        const double v1 = __dadd_rn(__dadd_rn(__dmul_rn(m[3], p0), __dmul_rn(m[4], p1)), m[5]);
        x = (float)((long long)v0 + 1);         // astype(int) truncates towards zero
        y = (float)((long long)v1 + 1);
    }
    preds[map * 2] = x;
    preds[map * 2 + 1] = y;
}

}  // namespace up

using namespace up;

#define UP_LAUNCH_1D(kernel, total, st, ...) \
    hipLaunchKernelGGL(kernel, dim3(grid_cap(total)), dim3(256), 0, st, __VA_ARGS__)

#define UP_DT_OK(dt) ((dt) == UP_DT_F32 || (dt) == UP_DT_BF16)
extern "C" int up_nchw_to_nhwc_t(const float* x, void* y, int N, int C, int H, int W, int ldy, int dt_out, void* stream) {
    UP_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0 && ldy >= C && UP_DT_OK(dt_out), UP_ERR_INVALID,
               "nchw_to_nhwc: bad argument");
    int64_t npix = (int64_t)N * H * W;
    if (dt_out == UP_DT_BF16)
        UP_LAUNCH_1D(nchw_to_nhwc_kernel<bf16_t>, npix, as_stream(stream), x, (bf16_t*)y, C, H * W, ldy, npix);
    else
        UP_LAUNCH_1D(nchw_to_nhwc_kernel<float>, npix, as_stream(stream), x, (float*)y, C, H * W, ldy, npix);
    return check_launch("nchw_to_nhwc");
}
extern "C" int up_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, int ldy, void* stream) {
    return up_nchw_to_nhwc_t(x, y, N, C, H, W, ldy, UP_DT_F32, stream);
}
extern "C" int up_nchw_to_nhwc_flip(const float* x, float* y, int N, int C, int H, int W, int ldy, void* stream) {
    UP_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0 && ldy >= C, UP_ERR_INVALID, "nchw_to_nhwc_flip: bad argument");
    int64_t npix = (int64_t)N * H * W;
    UP_LAUNCH_1D(nchw_to_nhwc_flip_kernel, npix, as_stream(stream), x, y, C, W, H * W, ldy, npix);
    return check_launch("nchw_to_nhwc_flip");
}
extern "C" int up_nhwc_to_nchw_t(const void* x, int ldx, float* y, int N, int C, int H, int W, int dt_in, void* stream) {
    UP_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0 && ldx >= C && UP_DT_OK(dt_in), UP_ERR_INVALID,
               "nhwc_to_nchw: bad argument");
    int64_t npix = (int64_t)N * H * W;
    if (dt_in == UP_DT_BF16)
        UP_LAUNCH_1D(nhwc_to_nchw_kernel<bf16_t>, npix, as_stream(stream), (const bf16_t*)x, ldx, y, C, H * W, npix);
    else
        UP_LAUNCH_1D(nhwc_to_nchw_kernel<float>, npix, as_stream(stream), (const float*)x, ldx, y, C, H * W, npix);
    return check_launch("nhwc_to_nchw");
}
extern "C" int up_nhwc_to_nchw(const float* x, int ldx, float* y, int N, int C, int H, int W, void* stream) {
    return up_nhwc_to_nchw_t(x, ldx, y, N, C, H, W, UP_DT_F32, stream);
}

// what every _strided clip entry asks of its two extra arguments, after its neighbour's own checks (B, T > 0): the B samples lie
// inside a frame of frame_images images, and the image index t * frame_images + first + b stays an int32
static int clip_stride_ok(const char* what, int B, int T, int frame_images, int first) {
    UP_REQUIRE(first >= 0 && (int64_t)frame_images >= (int64_t)first + B, UP_ERR_INVALID,
               "%s: %d samples from image %d of frames of %d images", what, B, first, frame_images);
    UP_REQUIRE((int64_t)T * frame_images <= INT32_MAX, UP_ERR_INVALID, "%s: %d frames of %d images: an image index beyond the int32 range",
               what, T, frame_images);
    return UP_OK;
}
// the four layout entries: one set of refusals, one device function (strided: the kernel that takes frame_images and first)
static int clip_nchw_to_nhwc(const char* what, bool flip, bool strided, const float* x, float* y, int B, int T, int C, int H, int W, int ldy,
                             int frame_images, int first, void* stream) {
    UP_REQUIRE(x && y && B > 0 && T > 0 && C > 0 && H > 0 && W > 0 && ldy >= C && ldy % 4 == 0 && (uintptr_t)y % 16 == 0,
               UP_ERR_INVALID, "%s: bad argument", what);
    if (flip) UP_REQUIRE((int64_t)H * W <= INT32_MAX, UP_ERR_INVALID, "%s: %d x %d: a pixel index beyond the int32 range", what, H, W);
    if (strided)
        if (int e = clip_stride_ok(what, B, T, frame_images, first)) return e;
    int64_t npix = (int64_t)T * B * H * W;
    if (strided && flip)
        UP_LAUNCH_1D(clip_nchw_to_nhwc_strided_kernel<true>, npix, as_stream(stream), x, y, B, T, C, W, H * W, ldy, npix, frame_images,
                     first);
    else if (strided)
        UP_LAUNCH_1D(clip_nchw_to_nhwc_strided_kernel<false>, npix, as_stream(stream), x, y, B, T, C, W, H * W, ldy, npix, frame_images,
                     first);
    else if (flip)
        UP_LAUNCH_1D(clip_nchw_to_nhwc_kernel<true>, npix, as_stream(stream), x, y, B, T, C, W, H * W, ldy, npix);
    else
        UP_LAUNCH_1D(clip_nchw_to_nhwc_kernel<false>, npix, as_stream(stream), x, y, B, T, C, W, H * W, ldy, npix);
    return check_launch(what);
}
extern "C" int up_clip_nchw_to_nhwc(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, void* stream) {
    return clip_nchw_to_nhwc("clip_nchw_to_nhwc", false, false, x, y, B, T, C, H, W, ldy, B, 0, stream);
}
extern "C" int up_clip_nchw_to_nhwc_flip(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, void* stream) {
    return clip_nchw_to_nhwc("clip_nchw_to_nhwc_flip", true, false, x, y, B, T, C, H, W, ldy, B, 0, stream);
}
extern "C" int up_clip_nchw_to_nhwc_strided(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, int frame_images,
                                            int first, void* stream) {
    return clip_nchw_to_nhwc("clip_nchw_to_nhwc_strided", false, true, x, y, B, T, C, H, W, ldy, frame_images, first, stream);
}
extern "C" int up_clip_nchw_to_nhwc_flip_strided(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, int frame_images,
                                                 int first, void* stream) {
    return clip_nchw_to_nhwc("clip_nchw_to_nhwc_flip_strided", true, true, x, y, B, T, C, H, W, ldy, frame_images, first, stream);
}
extern "C" int up_clip_nhwc_to_nchw(const float* x, int ldx, float* y, int B, int T, int C, int H, int W, void* stream) {
    UP_REQUIRE(x && y && B > 0 && T > 0 && C > 0 && H > 0 && W > 0 && ldx >= C && ldx % 4 == 0 && (uintptr_t)x % 16 == 0,
               UP_ERR_INVALID, "clip_nhwc_to_nchw: bad argument");
    int64_t npix = (int64_t)T * B * H * W;
    UP_LAUNCH_1D(clip_nhwc_to_nchw_kernel, npix, as_stream(stream), x, ldx, y, B, T, C, H * W, npix);
    return check_launch("clip_nhwc_to_nchw");
}

extern "C" int up_copy2d(const float* s, int lds, float* d, int ldd, int64_t rows, int C, void* stream) {
    UP_REQUIRE(s && d && rows > 0 && C > 0 && lds >= C && ldd >= C, UP_ERR_INVALID, "copy2d: bad argument");
    UP_REQUIRE(rows * C < (1ll << 31), UP_ERR_UNSUPPORTED, "copy2d: tensor too large");
    bool v4 = C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && ((uintptr_t)s % 16 == 0) && ((uintptr_t)d % 16 == 0);
    if (v4) {
        int64_t total = rows * (C / 4);
        UP_LAUNCH_1D(copy2d_v4_kernel, total, as_stream(stream), s, lds, d, ldd, total, C / 4, make_fastdiv(C / 4));
    } else {
        int64_t total = rows * C;
        UP_LAUNCH_1D(copy2d_s_kernel, total, as_stream(stream), s, lds, d, ldd, total, C, make_fastdiv(C));
    }
    return check_launch("copy2d");
}
extern "C" int up_add2d(const float* a, int lda, const float* b, int ldb, float* d, int ldd, int64_t rows, int C,
                        void* stream) {
    UP_REQUIRE(a && b && d && rows > 0 && C > 0, UP_ERR_INVALID, "add2d: bad argument");
    UP_REQUIRE(rows * C < (1ll << 31), UP_ERR_UNSUPPORTED, "add2d: tensor too large");
    int64_t total = rows * C;
    UP_LAUNCH_1D(add2d_kernel, total, as_stream(stream), a, lda, b, ldb, d, ldd, total, C, make_fastdiv(C));
    return check_launch("add2d");
}

static int pool_args_ok(int N, int H, int W, int C, int P, int Q, int lda, int ldb) {
    UP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && P > 0 && Q > 0, UP_ERR_INVALID, "spatial op: bad dimension");
    UP_REQUIRE(C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && lda >= C && ldb >= C, UP_ERR_INVALID,
               "spatial op: C and strides must be multiples of 4");
    UP_REQUIRE((int64_t)N * H * W * (C / 4) < (1ll << 31) && (int64_t)N * P * Q * (C / 4) < (1ll << 31),
               UP_ERR_UNSUPPORTED, "spatial op: tensor too large");
    return UP_OK;
}

// (dt_in, dt_out): the max-pool after the stem is where the bf16-storage network leaves fp32 (fp32 in, bf16 out; its
// backward bf16 in, fp32 out); all other uses have equal types
namespace up {
template <typename TI, typename TO>
static void launch_maxpool_fwd(const void* x, int ldx, void* y, int ldy, uint8_t* idx, int H, int W, int C, int P, int Q,
                               int64_t total, hipStream_t st) {
    UP_LAUNCH_1D((maxpool_fwd_kernel<TI, TO>), total, st, (const TI*)x, ldx, (TO*)y, ldy, idx, H, W, C / 4, P, Q, total,
                 make_fastdiv(C / 4), make_fastdiv(Q), make_fastdiv(P));
}
template <typename TI, typename TO>
static void launch_maxpool_bwd(const void* dy, int lddy, const uint8_t* idx, void* dx, int lddx, int H, int W, int C, int P,
                               int Q, int64_t total, hipStream_t st) {
    UP_LAUNCH_1D((maxpool_bwd_kernel<TI, TO>), total, st, (const TI*)dy, lddy, idx, (TO*)dx, lddx, H, W, C / 4, P, Q, total,
                 make_fastdiv(C / 4), make_fastdiv(W), make_fastdiv(H));
}
}  // namespace up
extern "C" int up_maxpool3s2_fwd_t(const void* x, int ldx, void* y, int ldy, uint8_t* idx, int N, int H, int W, int C,
                                   int P, int Q, int dt_in, int dt_out, void* stream) {
    if (int e = pool_args_ok(N, H, W, C, P, Q, ldx, ldy)) return e;
    UP_REQUIRE(x && y && idx && UP_DT_OK(dt_in) && UP_DT_OK(dt_out), UP_ERR_INVALID, "maxpool_fwd: bad argument");
    UP_REQUIRE(P == (H - 1) / 2 + 1 && Q == (W - 1) / 2 + 1, UP_ERR_INVALID, "maxpool_fwd: P,Q mismatch");
    int64_t total = (int64_t)N * P * Q * (C / 4);
    hipStream_t st = as_stream(stream);
    if (dt_in == UP_DT_F32 && dt_out == UP_DT_F32) launch_maxpool_fwd<float, float>(x, ldx, y, ldy, idx, H, W, C, P, Q, total, st);
    else if (dt_in == UP_DT_F32) launch_maxpool_fwd<float, bf16_t>(x, ldx, y, ldy, idx, H, W, C, P, Q, total, st);
    else if (dt_out == UP_DT_F32) launch_maxpool_fwd<bf16_t, float>(x, ldx, y, ldy, idx, H, W, C, P, Q, total, st);
    else launch_maxpool_fwd<bf16_t, bf16_t>(x, ldx, y, ldy, idx, H, W, C, P, Q, total, st);
    return check_launch("maxpool_fwd");
}
extern "C" int up_maxpool3s2_fwd(const float* x, int ldx, float* y, int ldy, uint8_t* idx, int N, int H, int W, int C,
                                 int P, int Q, void* stream) {
    return up_maxpool3s2_fwd_t(x, ldx, y, ldy, idx, N, H, W, C, P, Q, UP_DT_F32, UP_DT_F32, stream);
}
extern "C" int up_maxpool3s2_bwd_t(const void* dy, int lddy, const uint8_t* idx, void* dx, int lddx, int N, int H,
                                   int W, int C, int P, int Q, int dt_in, int dt_out, void* stream) {
    if (int e = pool_args_ok(N, H, W, C, P, Q, lddx, lddy)) return e;
    UP_REQUIRE(dy && idx && dx && UP_DT_OK(dt_in) && UP_DT_OK(dt_out), UP_ERR_INVALID, "maxpool_bwd: bad argument");
    int64_t total = (int64_t)N * H * W * (C / 4);
    hipStream_t st = as_stream(stream);
    if (dt_in == UP_DT_F32 && dt_out == UP_DT_F32) launch_maxpool_bwd<float, float>(dy, lddy, idx, dx, lddx, H, W, C, P, Q, total, st);
    else if (dt_in == UP_DT_F32) launch_maxpool_bwd<float, bf16_t>(dy, lddy, idx, dx, lddx, H, W, C, P, Q, total, st);
    else if (dt_out == UP_DT_F32) launch_maxpool_bwd<bf16_t, float>(dy, lddy, idx, dx, lddx, H, W, C, P, Q, total, st);
    else launch_maxpool_bwd<bf16_t, bf16_t>(dy, lddy, idx, dx, lddx, H, W, C, P, Q, total, st);
    return check_launch("maxpool_bwd");
}
extern "C" int up_maxpool3s2_bwd(const float* dy, int lddy, const uint8_t* idx, float* dx, int lddx, int N, int H,
                                 int W, int C, int P, int Q, void* stream) {
    return up_maxpool3s2_bwd_t(dy, lddy, idx, dx, lddx, N, H, W, C, P, Q, UP_DT_F32, UP_DT_F32, stream);
}

static inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

extern "C" int up_bilinear_fwd_t(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int P, int Q,
                                 int dtype, void* stream) {
    if (int e = pool_args_ok(N, H, W, C, P, Q, ldx, ldy)) return e;
    UP_REQUIRE(x && y && UP_DT_OK(dtype), UP_ERR_INVALID, "bilinear_fwd: bad argument");
    int64_t total = (int64_t)N * P * Q * (C / 4);
    if (dtype == UP_DT_BF16)
        UP_LAUNCH_1D(bilinear_fwd_kernel<bf16_t>, total, as_stream(stream), (const bf16_t*)x, ldx, (bf16_t*)y, ldy, H, W,
                     C / 4, P, Q, ac_scale(H, P), ac_scale(W, Q), total, make_fastdiv(C / 4), make_fastdiv(Q),
                     make_fastdiv(P));
    else
        UP_LAUNCH_1D(bilinear_fwd_kernel<float>, total, as_stream(stream), (const float*)x, ldx, (float*)y, ldy, H, W,
                     C / 4, P, Q, ac_scale(H, P), ac_scale(W, Q), total, make_fastdiv(C / 4), make_fastdiv(Q),
                     make_fastdiv(P));
    return check_launch("bilinear_fwd");
}
extern "C" int up_bilinear_fwd(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int P, int Q,
                               void* stream) {
    return up_bilinear_fwd_t(x, ldx, y, ldy, N, H, W, C, P, Q, UP_DT_F32, stream);
}
extern "C" int up_bilinear_bwd_t(const void* dy, int lddy, void* dx, int lddx, int N, int H, int W, int C, int P,
                                 int Q, int dtype, void* stream) {
    if (int e = pool_args_ok(N, H, W, C, P, Q, lddx, lddy)) return e;
    UP_REQUIRE(dy && dx && UP_DT_OK(dtype), UP_ERR_INVALID, "bilinear_bwd: bad argument");
    int64_t total = (int64_t)N * H * W * (C / 4);
    if (H == 1 && W == 1) {   // broadcast of a 1x1 map: a per-image column sum
        dim3 grid(N, cdiv(C, 64));
        if (dtype == UP_DT_BF16)
            hipLaunchKernelGGL(bcast_bwd_kernel<bf16_t>, grid, dim3(256), 0, as_stream(stream), (const bf16_t*)dy, lddy, (bf16_t*)dx,
                               lddx, P * Q, C);
        else
            hipLaunchKernelGGL(bcast_bwd_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)dy, lddy, (float*)dx, lddx,
                               P * Q, C);
        return check_launch("bilinear_bwd");
    }
    if (dtype == UP_DT_BF16)
        UP_LAUNCH_1D(bilinear_bwd_kernel<bf16_t>, total, as_stream(stream), (const bf16_t*)dy, lddy, (bf16_t*)dx, lddx, H,
                     W, C / 4, P, Q, ac_scale(H, P), ac_scale(W, Q), total, make_fastdiv(C / 4), make_fastdiv(W),
                     make_fastdiv(H));
    else
        UP_LAUNCH_1D(bilinear_bwd_kernel<float>, total, as_stream(stream), (const float*)dy, lddy, (float*)dx, lddx, H, W,
                     C / 4, P, Q, ac_scale(H, P), ac_scale(W, Q), total, make_fastdiv(C / 4), make_fastdiv(W),
                     make_fastdiv(H));
    return check_launch("bilinear_bwd");
}
extern "C" int up_bilinear_bwd(const float* dy, int lddy, float* dx, int lddx, int N, int H, int W, int C, int P,
                               int Q, void* stream) {
    return up_bilinear_bwd_t(dy, lddy, dx, lddx, N, H, W, C, P, Q, UP_DT_F32, stream);
}

extern "C" int up_gap_fwd_t(const void* x, int ldx, void* y, int N, int HW, int C, int dtype, void* stream) {
    UP_REQUIRE(x && y && N > 0 && HW > 0 && C > 0 && ldx >= C && UP_DT_OK(dtype), UP_ERR_INVALID, "gap_fwd: bad argument");
    if (dtype == UP_DT_BF16)
        hipLaunchKernelGGL(gap_fwd_kernel<bf16_t>, dim3(N, cdiv(C, 64)), dim3(256), 0, as_stream(stream), (const bf16_t*)x,
                           ldx, (bf16_t*)y, HW, C);
    else
        hipLaunchKernelGGL(gap_fwd_kernel<float>, dim3(N, cdiv(C, 64)), dim3(256), 0, as_stream(stream), (const float*)x,
                           ldx, (float*)y, HW, C);
    return check_launch("gap_fwd");
}
extern "C" int up_gap_fwd(const float* x, int ldx, float* y, int N, int HW, int C, void* stream) {
    return up_gap_fwd_t(x, ldx, y, N, HW, C, UP_DT_F32, stream);
}
extern "C" int up_gap_bwd_t(const void* dy, void* dx, int lddx, int N, int HW, int C, int dtype, void* stream) {
    UP_REQUIRE(dy && dx && N > 0 && HW > 0 && C > 0 && C % 4 == 0 && lddx % 4 == 0 && lddx >= C && UP_DT_OK(dtype),
               UP_ERR_INVALID, "gap_bwd: bad argument");
    int64_t total = (int64_t)N * HW * (C / 4);
    UP_REQUIRE(total < (1ll << 31), UP_ERR_UNSUPPORTED, "gap_bwd: tensor too large");
    if (dtype == UP_DT_BF16)
        UP_LAUNCH_1D(gap_bwd_kernel<bf16_t>, total, as_stream(stream), (const bf16_t*)dy, (bf16_t*)dx, lddx, HW, C / 4,
                     1.0f / (float)HW, total, make_fastdiv(C / 4), make_fastdiv(HW));
    else
        UP_LAUNCH_1D(gap_bwd_kernel<float>, total, as_stream(stream), (const float*)dy, (float*)dx, lddx, HW, C / 4,
                     1.0f / (float)HW, total, make_fastdiv(C / 4), make_fastdiv(HW));
    return check_launch("gap_bwd");
}
extern "C" int up_gap_bwd(const float* dy, float* dx, int lddx, int N, int HW, int C, void* stream) {
    return up_gap_bwd_t(dy, dx, lddx, N, HW, C, UP_DT_F32, stream);
}

extern "C" int up_avgpool9s8_fwd(const float* x, float* y, int ldy, int coff, int N, int H, int W, int P, int Q,
                                 void* stream) {
    UP_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && coff >= 0 && coff < ldy, UP_ERR_INVALID, "avgpool: bad argument");
    UP_REQUIRE(P == (H + 2 - 9) / 8 + 1 && Q == (W + 2 - 9) / 8 + 1, UP_ERR_INVALID, "avgpool: P,Q mismatch");
    int64_t total = (int64_t)N * P * Q;
    UP_LAUNCH_1D(avgpool9s8_kernel, total, as_stream(stream), x, y, ldy, coff, H, W, P, Q, total);
    return check_launch("avgpool9s8");
}

extern "C" int up_clip_avgpool9s8_fwd(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                                      void* stream) {
    UP_REQUIRE(x && y && B > 0 && T > 0 && H > 0 && W > 0 && coff >= 0 && coff < ldy, UP_ERR_INVALID, "clip_avgpool: bad argument");
    UP_REQUIRE(P == (H + 2 - 9) / 8 + 1 && Q == (W + 2 - 9) / 8 + 1, UP_ERR_INVALID, "clip_avgpool: P,Q mismatch");
    int64_t total = (int64_t)T * B * P * Q;
    UP_LAUNCH_1D(clip_avgpool9s8_kernel<false>, total, as_stream(stream), x, y, ldy, coff, B, T, H, W, P, Q, total);
    return check_launch("clip_avgpool9s8");
}

// the mirrored pooling and the two _strided poolings: the refusals of up_clip_avgpool9s8_flip_fwd (which holds all of its plain
// neighbour's, and P, Q > 0: with none of them a strided launch would have no pixel to write)
static int clip_avgpool_checked(const char* what, bool flip, bool strided, const float* x, float* y, int ldy, int coff, int B, int T, int H,
                                int W, int P, int Q, int frame_images, int first, void* stream) {
    UP_REQUIRE(x && y && B > 0 && T > 0 && H > 0 && W > 0 && ldy > 0 && coff >= 0 && coff < ldy, UP_ERR_INVALID, "%s: bad argument", what);
    UP_REQUIRE(P == (H + 2 - 9) / 8 + 1 && Q == (W + 2 - 9) / 8 + 1 && P > 0 && Q > 0, UP_ERR_INVALID, "%s: P,Q mismatch", what);
    UP_REQUIRE((int64_t)H * W <= INT32_MAX, UP_ERR_INVALID, "%s: %d x %d: a pixel index beyond the int32 range", what, H, W);
    if (strided)
        if (int e = clip_stride_ok(what, B, T, frame_images, first)) return e;
    int64_t total = (int64_t)T * B * P * Q;
    if (!strided)
        UP_LAUNCH_1D(clip_avgpool9s8_kernel<true>, total, as_stream(stream), x, y, ldy, coff, B, T, H, W, P, Q, total);
    else if (flip)
        UP_LAUNCH_1D(clip_avgpool9s8_strided_kernel<true>, total, as_stream(stream), x, y, ldy, coff, B, T, H, W, P, Q, total,
                     frame_images, first);
    else
        UP_LAUNCH_1D(clip_avgpool9s8_strided_kernel<false>, total, as_stream(stream), x, y, ldy, coff, B, T, H, W, P, Q, total,
                     frame_images, first);
    return check_launch(what);
}
extern "C" int up_clip_avgpool9s8_flip_fwd(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                                           void* stream) {
    return clip_avgpool_checked("clip_avgpool_flip", true, false, x, y, ldy, coff, B, T, H, W, P, Q, B, 0, stream);
}
extern "C" int up_clip_avgpool9s8_fwd_strided(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                                              int frame_images, int first, void* stream) {
    return clip_avgpool_checked("clip_avgpool_strided", false, true, x, y, ldy, coff, B, T, H, W, P, Q, frame_images, first, stream);
}
extern "C" int up_clip_avgpool9s8_flip_fwd_strided(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P,
                                                   int Q, int frame_images, int first, void* stream) {
    return clip_avgpool_checked("clip_avgpool_flip_strided", true, true, x, y, ldy, coff, B, T, H, W, P, Q, frame_images, first, stream);
}

extern "C" int up_lstm0_fwd(const float* gates, int ldg, float* cell, float* hide, int ldo, int64_t rows, int Cg,
                            void* stream) {
    UP_REQUIRE(gates && cell && hide && rows > 0 && Cg > 0 && ldg >= 3 * Cg && ldo >= Cg, UP_ERR_INVALID,
               "lstm0_fwd: bad argument");
    int64_t total = rows * Cg;
    UP_LAUNCH_1D(lstm0_fwd_kernel, total, as_stream(stream), gates, ldg, cell, hide, ldo, total, Cg);
    return check_launch("lstm0_fwd");
}
extern "C" int up_lstm0_bwd(const float* gates, int ldg, const float* dcell, const float* dhide, int ldo,
                            float* dgates, int64_t rows, int Cg, void* stream) {
    UP_REQUIRE(gates && dcell && dhide && dgates && rows > 0 && Cg > 0 && ldg >= 3 * Cg && ldo >= Cg, UP_ERR_INVALID,
               "lstm0_bwd: bad argument");
    int64_t total = rows * Cg;
    UP_LAUNCH_1D(lstm0_bwd_kernel, total, as_stream(stream), gates, ldg, dcell, dhide, ldo, dgates, total, Cg);
    return check_launch("lstm0_bwd");
}
extern "C" int up_lstm_fwd(const float* gates, int ldg, const float* cprev, int ldc, float* cell, float* hide, int ldo,
                           int64_t rows, int Cg, void* stream) {
    UP_REQUIRE(gates && cprev && cell && hide && rows > 0 && Cg > 0 && ldg >= 4 * Cg && ldo >= Cg && ldc >= Cg,
               UP_ERR_INVALID, "lstm_fwd: bad argument");
    int64_t total = rows * Cg;
    UP_LAUNCH_1D(lstm_fwd_kernel, total, as_stream(stream), gates, ldg, cprev, ldc, cell, hide, ldo, total, Cg);
    return check_launch("lstm_fwd");
}
extern "C" int up_lstm_bwd(const float* gates, int ldg, const float* cprev, int ldc, const float* cell,
                           const float* dcell, const float* dhide, int ldo, float* dgates, float* dcprev,
                           int64_t rows, int Cg, void* stream) {
    UP_REQUIRE(gates && cprev && cell && dcell && dhide && dgates && dcprev && rows > 0 && Cg > 0 && ldg >= 4 * Cg &&
                   ldo >= Cg && ldc >= Cg,
               UP_ERR_INVALID, "lstm_bwd: bad argument");
    int64_t total = rows * Cg;
    UP_LAUNCH_1D(lstm_bwd_kernel, total, as_stream(stream), gates, ldg, cprev, ldc, cell, dcell, dhide, ldo, dgates,
                 dcprev, total, Cg);
    return check_launch("lstm_bwd");
}

// the host tables of a serving call, checked, as the kernel argument
static int serve_table(const char* what, int slots, const int32_t* slot_host, const int32_t* first_host, int B, ServeTable& tab,
                       int& firsts, int& conts) {
    if (int e = serve_table_check(what, slots, slot_host, first_host, B, &firsts, &conts)) return e;
    memset(&tab, 0, sizeof(tab));
    for (int b = 0; b < B; ++b) {
        tab.slot[b] = slot_host[b];
        if (slot_host[b] < 0 || first_host[b] != 0) tab.first |= 1ull << b;
    }
    return UP_OK;
}
extern "C" int up_lstm_state_gather(const float* pool, int64_t slot_stride, int slots, const int32_t* slot_host, const int32_t* first_host,
                                    int B, int64_t rows_per_sample, int ldo, float* dst, int ldd, int coff, void* stream) {
    ServeTable tab;
    int firsts = 0, conts = 0;
    if (int e = serve_table("lstm_state_gather", slots, slot_host, first_host, B, tab, firsts, conts)) return e;
    UP_REQUIRE(pool && dst && rows_per_sample > 0 && ldo > 0 && coff >= 0 && (int64_t)coff + ldo <= ldd &&
                   rows_per_sample <= INT64_MAX / (2 * UP_SERVE_CAP) / ldo && slot_stride >= 2 * rows_per_sample * ldo,
               UP_ERR_INVALID, "lstm_state_gather: bad argument (%lld rows of %d lanes, record stride %lld, lanes %d.. of %d)",
               (long long)rows_per_sample, ldo, (long long)slot_stride, coff, ldd);
    const int64_t total = (int64_t)B * rows_per_sample * ldo;
    UP_LAUNCH_1D(lstm_state_gather_kernel, total, as_stream(stream), pool, slot_stride, tab, rows_per_sample, ldo, dst, ldd, coff, total);
    return check_launch("lstm_state_gather");
}
extern "C" int up_lstm_serve_fwd(const float* gates0, int ldg0, const float* gates, int ldg, float* pool, int64_t slot_stride, int slots,
                                 const int32_t* slot_host, const int32_t* first_host, float* cell, float* hide, int ldo, int B,
                                 int64_t rows_per_sample, int Cg, void* stream) {
    ServeTable tab;
    int firsts = 0, conts = 0;
    if (int e = serve_table("lstm_serve_fwd", slots, slot_host, first_host, B, tab, firsts, conts)) return e;
    UP_REQUIRE(pool && cell && hide && rows_per_sample > 0 && Cg > 0 && ldo >= Cg && rows_per_sample <= INT64_MAX / (2 * UP_SERVE_CAP) / ldo &&
                   slot_stride >= 2 * rows_per_sample * ldo,
               UP_ERR_INVALID, "lstm_serve_fwd: bad argument (%lld rows of %d lanes, %d gate channels, record stride %lld)",
               (long long)rows_per_sample, ldo, Cg, (long long)slot_stride);
    UP_REQUIRE(!firsts || (gates0 && ldg0 >= 3 * Cg), UP_ERR_INVALID,
               "lstm_serve_fwd: %d first or idle samples need gates0 (row stride %d >= %d)", firsts, ldg0, 3 * Cg);
    UP_REQUIRE(!conts || (gates && ldg >= 4 * Cg), UP_ERR_INVALID, "lstm_serve_fwd: %d continuing samples need gates (row stride %d >= %d)",
               conts, ldg, 4 * Cg);
    const int64_t total = (int64_t)B * rows_per_sample * ldo;
    UP_LAUNCH_1D(lstm_serve_fwd_kernel, total, as_stream(stream), gates0, ldg0, gates, ldg, pool, slot_stride, tab, cell, hide, ldo,
                 rows_per_sample, total, Cg);
    return check_launch("lstm_serve_fwd");
}

extern "C" int up_heatmap_argmax(const float* hm, int B, int J, int H, int W, int32_t* idx, float* preds_xy,
                                 float* maxvals, void* stream) {
    UP_REQUIRE(hm && preds_xy && maxvals && B > 0 && J > 0 && H > 0 && W > 0, UP_ERR_INVALID,
               "heatmap_argmax: bad argument");
    int maps = B * J;
    hipLaunchKernelGGL(argmax_kernel, dim3(cdiv(maps, 4)), dim3(256), 0, as_stream(stream), hm, maps, H * W, W, idx,
                       preds_xy, maxvals);
    return check_launch("heatmap_argmax");
}

extern "C" int up_heatmap_decode(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int J, int H,
                                 int W, int P, int Q, int32_t* idx, float* preds_xy, float* maxvals, void* stream) {
    UP_REQUIRE(hm && preds_xy && maxvals, UP_ERR_INVALID, "heatmap_decode: null argument");
    UP_REQUIRE(B > 0 && J > 0 && H > 0 && W > 0 && stride_b > 0 && stride_j > 0 && stride_p > 0, UP_ERR_INVALID,
               "heatmap_decode: %d x %d maps of %d x %d, strides %lld / %lld / %lld", B, J, H, W, (long long)stride_b,
               (long long)stride_j, (long long)stride_p);
    UP_REQUIRE(P >= H && Q >= W, UP_ERR_INVALID, "heatmap_decode: %d x %d -> %d x %d (down-sampling is not decoded)", H, W, P, Q);
    const int64_t lim = INT32_MAX;
    UP_REQUIRE((int64_t)P * Q <= lim && (int64_t)B * J <= lim && (int64_t)H * W <= lim && stride_b <= lim && stride_j <= lim &&
                   stride_p <= lim && (B - 1) * stride_b <= lim && (J - 1) * stride_j <= lim && ((int64_t)H * W - 1) * stride_p <= lim &&
                   (B - 1) * stride_b + (J - 1) * stride_j + ((int64_t)H * W - 1) * stride_p <= lim,
               UP_ERR_INVALID, "heatmap_decode: %d x %d maps of %d x %d -> %d x %d: an index beyond the int32 range", B, J, H, W, P, Q);
    const dim3 grid(B * J), block(256);
    const float sh = ac_scale(H, P), sw = ac_scale(W, Q);     // as up_bilinear_fwd computes them
    if ((P != H || Q != W) && H * W <= DECODE_LDS)
        hipLaunchKernelGGL(decode_kernel<true>, grid, block, 0, as_stream(stream), hm, stride_b, stride_j, stride_p, J, H, W, P, Q, sh,
                           sw, make_fastdiv(Q), idx, preds_xy, maxvals, 0, 0);
    else
        hipLaunchKernelGGL(decode_kernel<false>, grid, block, 0, as_stream(stream), hm, stride_b, stride_j, stride_p, J, H, W, P, Q, sh,
                           sw, make_fastdiv(Q), idx, preds_xy, maxvals, 0, 0);
    return check_launch("heatmap_decode");
}

extern "C" int up_clip_heatmap_decode(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int T, int J, int H,
                                      int W, int P, int Q, int32_t* idx, float* preds_xy, float* maxvals, void* stream) {
    UP_REQUIRE(hm && preds_xy && maxvals, UP_ERR_INVALID, "clip_heatmap_decode: null argument");
    UP_REQUIRE(B > 0 && T > 0 && J > 0 && H > 0 && W > 0 && stride_b > 0 && stride_j > 0 && stride_p > 0, UP_ERR_INVALID,
               "clip_heatmap_decode: %d x %d x %d maps of %d x %d, strides %lld / %lld / %lld", B, T, J, H, W, (long long)stride_b,
               (long long)stride_j, (long long)stride_p);
    UP_REQUIRE(P >= H && Q >= W, UP_ERR_INVALID, "clip_heatmap_decode: %d x %d -> %d x %d (down-sampling is not decoded)", H, W, P, Q);
    const int64_t lim = INT32_MAX, N = (int64_t)B * T;
    UP_REQUIRE((int64_t)P * Q <= lim && N <= lim && N * J * 2 <= lim && (int64_t)H * W <= lim && stride_b <= lim && stride_j <= lim &&
                   stride_p <= lim && (N - 1) * stride_b <= lim && (J - 1) * stride_j <= lim && ((int64_t)H * W - 1) * stride_p <= lim &&
                   (N - 1) * stride_b + (J - 1) * stride_j + ((int64_t)H * W - 1) * stride_p <= lim,
               UP_ERR_INVALID, "clip_heatmap_decode: %d x %d x %d maps of %d x %d -> %d x %d: an index beyond the int32 range", B, T, J,
               H, W, P, Q);
    const dim3 grid((int)N * J), block(256);
    const float sh = ac_scale(H, P), sw = ac_scale(W, Q);
    if ((P != H || Q != W) && H * W <= DECODE_LDS)
        hipLaunchKernelGGL((decode_kernel<true, true>), grid, block, 0, as_stream(stream), hm, stride_b, stride_j, stride_p, J, H, W, P,
                           Q, sh, sw, make_fastdiv(Q), idx, preds_xy, maxvals, B, T);
    else
        hipLaunchKernelGGL((decode_kernel<false, true>), grid, block, 0, as_stream(stream), hm, stride_b, stride_j, stride_p, J, H, W, P,
                           Q, sh, sw, make_fastdiv(Q), idx, preds_xy, maxvals, B, T);
    return check_launch("clip_heatmap_decode");
}

// B x J maps of H x W behind three positive element strides: every count and the offset of the last element within int32
static bool maps_in_int32(int64_t sb, int64_t sj, int64_t sp, int B, int J, int H, int W) {
    const int64_t lim = INT32_MAX;
    return (int64_t)B * J <= lim && (int64_t)H * W <= lim && sb <= lim && sj <= lim && sp <= lim && (B - 1) * sb <= lim &&
           (J - 1) * sj <= lim && ((int64_t)H * W - 1) * sp <= lim && (B - 1) * sb + (J - 1) * sj + ((int64_t)H * W - 1) * sp <= lim;
}

extern "C" int up_flip_merge(const float* a, const float* f, int64_t in_stride_b, int64_t in_stride_j, int64_t in_stride_p, int B,
                             int J, int H, int W, const int32_t* perm_host, float* out, int64_t out_stride_b, int64_t out_stride_j,
                             int64_t out_stride_p, void* stream) {
    UP_REQUIRE(a && f && perm_host && out, UP_ERR_INVALID, "flip_merge: null argument");
    UP_REQUIRE(B > 0 && J > 0 && H > 0 && W > 0 && in_stride_b > 0 && in_stride_j > 0 && in_stride_p > 0 && out_stride_b > 0 &&
                   out_stride_j > 0 && out_stride_p > 0,
               UP_ERR_INVALID, "flip_merge: %d x %d maps of %d x %d, strides %lld / %lld / %lld -> %lld / %lld / %lld", B, J, H, W,
               (long long)in_stride_b, (long long)in_stride_j, (long long)in_stride_p, (long long)out_stride_b,
               (long long)out_stride_j, (long long)out_stride_p);
    UP_REQUIRE(J <= 256, UP_ERR_UNSUPPORTED, "flip_merge: %d channels (the permutation travels as 256 bytes of kernel arguments)", J);
    FlipPerm perm;
    memset(&perm, 0, sizeof(perm));
    for (int j = 0; j < J; ++j) {
        UP_REQUIRE(perm_host[j] >= 0 && perm_host[j] < J, UP_ERR_INVALID, "flip_merge: perm[%d] = %d outside 0..%d", j,
                   (int)perm_host[j], J - 1);
        perm.v[j] = (uint8_t)perm_host[j];
    }
    UP_REQUIRE(out != f, UP_ERR_INVALID, "flip_merge: out == f (the mirrored reads cross threads)");
    UP_REQUIRE(out != a || (out_stride_b == in_stride_b && out_stride_j == in_stride_j && out_stride_p == in_stride_p), UP_ERR_INVALID,
               "flip_merge: out == a needs equal strides");
    UP_REQUIRE(maps_in_int32(in_stride_b, in_stride_j, in_stride_p, B, J, H, W) &&
                   maps_in_int32(out_stride_b, out_stride_j, out_stride_p, B, J, H, W),
               UP_ERR_INVALID, "flip_merge: %d x %d maps of %d x %d: an index beyond the int32 range", B, J, H, W);
    const int64_t total = (int64_t)B * J * H * W;
    if (out_stride_j < out_stride_p)
        UP_LAUNCH_1D(flip_merge_kernel<true>, total, as_stream(stream), a, f, in_stride_b, in_stride_j, in_stride_p, J, H, W, perm,
                     out, out_stride_b, out_stride_j, out_stride_p, total);
    else
        UP_LAUNCH_1D(flip_merge_kernel<false>, total, as_stream(stream), a, f, in_stride_b, in_stride_j, in_stride_p, J, H, W, perm,
                     out, out_stride_b, out_stride_j, out_stride_p, total);
    return check_launch("flip_merge");
}

// up_flip_merge over T * B images behind a two-level batch index (include/unipose_hip.h): the same device function, the same checks
extern "C" int up_clip_flip_merge(const float* a, const float* f, int64_t in_stride_t, int64_t in_stride_b, int64_t in_stride_j,
                                  int64_t in_stride_p, int B, int T, int J, int H, int W, const int32_t* perm_host, float* out,
                                  int64_t out_stride_t, int64_t out_stride_b, int64_t out_stride_j, int64_t out_stride_p, void* stream) {
    UP_REQUIRE(a && f && perm_host && out, UP_ERR_INVALID, "clip_flip_merge: null argument");
    UP_REQUIRE(B > 0 && T > 0 && J > 0 && H > 0 && W > 0 && in_stride_t > 0 && in_stride_b > 0 && in_stride_j > 0 && in_stride_p > 0 &&
                   out_stride_t > 0 && out_stride_b > 0 && out_stride_j > 0 && out_stride_p > 0,
               UP_ERR_INVALID, "clip_flip_merge: %d x %d x %d maps of %d x %d, strides %lld / %lld / %lld / %lld -> %lld / %lld / %lld / %lld",
               T, B, J, H, W, (long long)in_stride_t, (long long)in_stride_b, (long long)in_stride_j, (long long)in_stride_p,
               (long long)out_stride_t, (long long)out_stride_b, (long long)out_stride_j, (long long)out_stride_p);
    UP_REQUIRE(J <= 256, UP_ERR_UNSUPPORTED, "clip_flip_merge: %d channels (the permutation travels as 256 bytes of kernel arguments)", J);
    FlipPerm perm;
    memset(&perm, 0, sizeof(perm));
    for (int j = 0; j < J; ++j) {
        UP_REQUIRE(perm_host[j] >= 0 && perm_host[j] < J, UP_ERR_INVALID, "clip_flip_merge: perm[%d] = %d outside 0..%d", j,
                   (int)perm_host[j], J - 1);
        perm.v[j] = (uint8_t)perm_host[j];
    }
    UP_REQUIRE(out != f, UP_ERR_INVALID, "clip_flip_merge: out == f (the mirrored reads cross threads)");
    UP_REQUIRE(out != a || (out_stride_t == in_stride_t && out_stride_b == in_stride_b && out_stride_j == in_stride_j &&
                            out_stride_p == in_stride_p),
               UP_ERR_INVALID, "clip_flip_merge: out == a needs equal strides");
    // the maps of one frame as up_flip_merge bounds them, and the frames' own offset on top, all within int32
    const int64_t lim = INT32_MAX;
    UP_REQUIRE(maps_in_int32(in_stride_b, in_stride_j, in_stride_p, B, J, H, W) &&
                   maps_in_int32(out_stride_b, out_stride_j, out_stride_p, B, J, H, W) && (int64_t)T * B * J <= lim && in_stride_t <= lim &&
                   out_stride_t <= lim &&
                   (T - 1) * in_stride_t + (B - 1) * in_stride_b + (J - 1) * in_stride_j + ((int64_t)H * W - 1) * in_stride_p <= lim &&
                   (T - 1) * out_stride_t + (B - 1) * out_stride_b + (J - 1) * out_stride_j + ((int64_t)H * W - 1) * out_stride_p <= lim,
               UP_ERR_INVALID, "clip_flip_merge: %d x %d x %d maps of %d x %d: an index beyond the int32 range", T, B, J, H, W);
    const int64_t total = (int64_t)T * B * J * H * W;
    if (out_stride_j < out_stride_p)
        UP_LAUNCH_1D(clip_flip_merge_kernel<true>, total, as_stream(stream), a, f, in_stride_t, in_stride_b, in_stride_j, in_stride_p, B, J,
                     H, W, perm, out, out_stride_t, out_stride_b, out_stride_j, out_stride_p, total);
    else
        UP_LAUNCH_1D(clip_flip_merge_kernel<false>, total, as_stream(stream), a, f, in_stride_t, in_stride_b, in_stride_j, in_stride_p, B, J,
                     H, W, perm, out, out_stride_t, out_stride_b, out_stride_j, out_stride_p, total);
    return check_launch("clip_flip_merge");
}

extern "C" int up_final_preds(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int J, int H, int W,
                              int res0, int res1, const double* inv, float* preds_xy, float* coords_xy, float* maxvals,
                              void* stream) {
    UP_REQUIRE(hm && preds_xy && maxvals, UP_ERR_INVALID, "final_preds: null argument");
    UP_REQUIRE(B > 0 && J > 0 && H > 0 && W > 0 && stride_b > 0 && stride_j > 0 && stride_p > 0 && res0 > 0 && res1 > 0,
               UP_ERR_INVALID, "final_preds: %d x %d maps of %d x %d, strides %lld / %lld / %lld, res %d, %d", B, J, H, W,
               (long long)stride_b, (long long)stride_j, (long long)stride_p, res0, res1);
    UP_REQUIRE(maps_in_int32(stride_b, stride_j, stride_p, B, J, H, W) && (int64_t)B * J * 2 <= INT32_MAX, UP_ERR_INVALID,
               "final_preds: %d x %d maps of %d x %d: an index beyond the int32 range", B, J, H, W);
    const int maps = B * J;
    hipLaunchKernelGGL(final_preds_kernel<false>, dim3(cdiv(maps, 4)), dim3(256), 0, as_stream(stream), hm, stride_b, stride_j,
                       stride_p, maps, J, H, W, res0, res1, inv, preds_xy, coords_xy, maxvals, 0, 0);
    return check_launch("final_preds");
}

extern "C" int up_clip_final_preds(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int T, int J, int H,
                                   int W, int res0, int res1, const double* inv, float* preds_xy, float* coords_xy, float* maxvals,
                                   void* stream) {
    UP_REQUIRE(hm && preds_xy && maxvals, UP_ERR_INVALID, "clip_final_preds: null argument");
    UP_REQUIRE(B > 0 && T > 0 && J > 0 && H > 0 && W > 0 && stride_b > 0 && stride_j > 0 && stride_p > 0 && res0 > 0 && res1 > 0,
               UP_ERR_INVALID, "clip_final_preds: %d x %d x %d maps of %d x %d, strides %lld / %lld / %lld, res %d, %d", B, T, J, H, W,
               (long long)stride_b, (long long)stride_j, (long long)stride_p, res0, res1);
    const int64_t N = (int64_t)B * T;
    UP_REQUIRE(N <= INT32_MAX && maps_in_int32(stride_b, stride_j, stride_p, (int)N, J, H, W) && N * J * 2 <= INT32_MAX, UP_ERR_INVALID,
               "clip_final_preds: %d x %d x %d maps of %d x %d: an index beyond the int32 range", B, T, J, H, W);
    const int maps = (int)N * J;
    hipLaunchKernelGGL(final_preds_kernel<true>, dim3(cdiv(maps, 4)), dim3(256), 0, as_stream(stream), hm, stride_b, stride_j,
                       stride_p, maps, J, H, W, res0, res1, inv, preds_xy, coords_xy, maxvals, B, T);
    return check_launch("clip_final_preds");
}

extern "C" int up_make_heatmaps(const double* kpt_xy, int B, int K, int H, int W, double stride, double sigma,
                                float* out, void* stream) {
    UP_REQUIRE(kpt_xy && out && B > 0 && K > 0 && H > 0 && W > 0 && stride > 0 && sigma > 0, UP_ERR_INVALID,
               "make_heatmaps: bad argument");
    long long total = (long long)B * H * W;
    hipLaunchKernelGGL(heatmap_target_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), kpt_xy, K, H, W,
                       stride, sigma, out, total);
    return check_launch("make_heatmaps");
}
extern "C" int up_make_gaussian_maps(const double* center_xy, int N, int H, int W, double sigma, float* out,
                                     void* stream) {
    UP_REQUIRE(center_xy && out && N > 0 && H > 0 && W > 0 && sigma > 0, UP_ERR_INVALID, "make_gaussian_maps: bad argument");
    long long total = (long long)N * H * W;
    hipLaunchKernelGGL(gaussian_map_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), center_xy, H, W,
                       sigma, out, total);
    return check_launch("make_gaussian_maps");
}
extern "C" int up_make_box_maps(const double* kpt_xy, int B, int K, int height, int width, double stride, double sigma,
                                float* out, int32_t* status, void* stream) {
    UP_REQUIRE(kpt_xy && out, UP_ERR_INVALID, "make_box_maps: null argument");
    UP_REQUIRE(B > 0 && K > 0 && height > 0 && width > 0 && stride > 0 && sigma > 0, UP_ERR_INVALID,
               "make_box_maps: %d samples of %d joints, image %d x %d, stride %g, sigma %g", B, K, height, width, stride, sigma);
    const double hd = trunc((double)height / stride), wd = trunc((double)width / stride);      // int(height / stride)
    UP_REQUIRE(hd >= 1 && wd >= 1, UP_ERR_INVALID, "make_box_maps: image %d x %d at stride %g gives an empty map", height, width,
               stride);
    UP_REQUIRE((double)B * 5.0 * hd * wd <= (double)INT32_MAX, UP_ERR_INVALID,
               "make_box_maps: %d samples of 5 maps of %.0f x %.0f: an index beyond the int32 range", B, hd, wd);
    const int h = (int)hd, w = (int)wd;
    long long total = (long long)B * h * w;
    hipLaunchKernelGGL(box_target_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), kpt_xy, K, height, width,
                       stride, sigma, h, w, out, status, total);
    return check_launch("make_box_maps");
}
extern "C" int up_normalize_image(const float* img_hwc, int B, int H, int W, int C, float mean, float stdv,
                                  float* out_chw, void* stream) {
    UP_REQUIRE(img_hwc && out_chw && B > 0 && H > 0 && W > 0 && C > 0 && stdv != 0.f, UP_ERR_INVALID,
               "normalize_image: bad argument");
    long long total = (long long)B * H * W * C;
    hipLaunchKernelGGL(normalize_image_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), img_hwc, C,
                       H * W, mean, stdv, out_chw, total);
    return check_launch("normalize_image");
}
extern "C" int up_augment_image(const void* src_hwc, int src_type, int B, int Hs, int Ws, int C, const int32_t* valid_hw,
                                const double* inv, int frames_per_map, float border, float mean, float stdv, float* out_chw,
                                int Ho, int Wo, void* stream) {
    UP_REQUIRE(src_hwc && inv && out_chw, UP_ERR_INVALID, "augment_image: null argument");
    UP_REQUIRE(src_type == UP_PIX_U8 || src_type == UP_PIX_F32, UP_ERR_INVALID, "augment_image: source type %d", src_type);
    UP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, UP_ERR_INVALID,
               "augment_image: %d images of %d x %d to %d x %d", B, Hs, Ws, Ho, Wo);
    UP_REQUIRE(C >= 1 && C <= 4, UP_ERR_INVALID, "augment_image: %d channels (1 .. 4)", C);
    UP_REQUIRE(frames_per_map >= 1 && B % frames_per_map == 0, UP_ERR_INVALID,
               "augment_image: %d frames per map do not divide %d images", frames_per_map, B);
    UP_REQUIRE(stdv > 0.f, UP_ERR_INVALID, "augment_image: std %g", (double)stdv);
    const long long total = (long long)B * Ho * Wo;
    if (src_type == UP_PIX_U8)
        hipLaunchKernelGGL(augment_image_kernel<uint8_t>, dim3(grid_cap(total)), dim3(256), 0, as_stream(stream),
                           (const uint8_t*)src_hwc, Hs, Ws, C, valid_hw, inv, frames_per_map, border, mean, stdv, out_chw, Ho, Wo,
                           total);
    else
        hipLaunchKernelGGL(augment_image_kernel<float>, dim3(grid_cap(total)), dim3(256), 0, as_stream(stream),
                           (const float*)src_hwc, Hs, Ws, C, valid_hw, inv, frames_per_map, border, mean, stdv, out_chw, Ho, Wo,
                           total);
    return check_launch("augment_image");
}
// up_crop_to_nhwc (T == 0: B samples) and up_clip_crop_to_nhwc (B x T samples, frame-major outputs): one set of refusals, one kernel
template <typename PIX, bool CLIP>
static void crop_launch(const void* src_hwc, int F, int Hs, int Ws, int C, const int32_t* frame_of, const int32_t* valid_hw,
                        const double* inv, int B, int T, float border, float mean, float stdv, float* y, float* yf, int Ho, int Wo, int ldy,
                        long long total, void* stream) {
    hipLaunchKernelGGL((crop_to_nhwc_kernel<PIX, CLIP>), dim3(grid_cap(total)), dim3(256), 0, as_stream(stream), (const PIX*)src_hwc, F,
                       Hs, Ws, C, frame_of, valid_hw, inv, border, mean, stdv, y, yf, Ho, Wo, ldy, total, B, T);
}
template <typename PIX>
static void crop_launch_strided(const void* src_hwc, int F, int Hs, int Ws, int C, const int32_t* frame_of, const int32_t* valid_hw,
                                const double* inv, int B, int T, float border, float mean, float stdv, float* y, float* yf, int Ho, int Wo,
                                int ldy, long long total, int frame_images, int first, void* stream) {
    hipLaunchKernelGGL((clip_crop_to_nhwc_strided_kernel<PIX>), dim3(grid_cap(total)), dim3(256), 0, as_stream(stream),
                       (const PIX*)src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, border, mean, stdv, y, yf, Ho, Wo, ldy, total, B, T,
                       frame_images, first);
}
static int crop_to_nhwc(const char* what, const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                        const int32_t* valid_hw, const double* inv, int B, int T, float border, float mean, float stdv, float* y_nhwc,
                        float* y_flip_nhwc, int Ho, int Wo, int ldy, void* stream, bool strided = false, int frame_images = 0,
                        int first = 0) {
    const bool clip = T != 0;
    UP_REQUIRE(src_hwc && inv, UP_ERR_INVALID, "%s: null argument", what);
    UP_REQUIRE(y_nhwc || y_flip_nhwc, UP_ERR_INVALID, "%s: both outputs are null", what);
    UP_REQUIRE(y_nhwc != y_flip_nhwc, UP_ERR_INVALID, "%s: y_nhwc == y_flip_nhwc", what);
    UP_REQUIRE(src_type == UP_PIX_U8 || src_type == UP_PIX_F32, UP_ERR_INVALID, "%s: source type %d", what, src_type);
    UP_REQUIRE(F > 0 && B > 0 && T >= 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, UP_ERR_INVALID,
               "%s: %d samples (%d frames each) from %d frames of %d x %d to %d x %d", what, B, clip ? T : 1, F, Hs, Ws, Ho, Wo);
    UP_REQUIRE(C >= 1 && C <= 4, UP_ERR_INVALID, "%s: %d channels (1 .. 4)", what, C);
    UP_REQUIRE(ldy >= C && ldy % 4 == 0, UP_ERR_INVALID, "%s: ldy %d for %d channels (a multiple of 4)", what, ldy, C);
    UP_REQUIRE((uintptr_t)y_nhwc % 16 == 0 && (uintptr_t)y_flip_nhwc % 16 == 0, UP_ERR_INVALID,
               "%s: an output that is not 16-byte aligned", what);
    const long long samples = (long long)B * (clip ? T : 1);
    UP_REQUIRE(frame_of || F == samples, UP_ERR_INVALID, "%s: no frame_of with %d frames for %lld samples", what, F, samples);
    UP_REQUIRE(stdv > 0.f, UP_ERR_INVALID, "%s: std %g", what, (double)stdv);
    const long long total = samples * Ho * Wo;
    if (strided) {
        if (int e = clip_stride_ok(what, B, T, frame_images, first)) return e;
        if (src_type == UP_PIX_U8)
            crop_launch_strided<uint8_t>(src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc, y_flip_nhwc, Ho, Wo,
                                         ldy, total, frame_images, first, stream);
        else
            crop_launch_strided<float>(src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc, y_flip_nhwc, Ho, Wo,
                                       ldy, total, frame_images, first, stream);
        return check_launch(what);
    }
    if (src_type == UP_PIX_U8) {
        if (clip)
            crop_launch<uint8_t, true>(src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc, y_flip_nhwc, Ho, Wo,
                                       ldy, total, stream);
        else
            crop_launch<uint8_t, false>(src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc, y_flip_nhwc, Ho,
                                        Wo, ldy, total, stream);
    } else {
        if (clip)
            crop_launch<float, true>(src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc, y_flip_nhwc, Ho, Wo,
                                     ldy, total, stream);
        else
            crop_launch<float, false>(src_hwc, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc, y_flip_nhwc, Ho, Wo,
                                      ldy, total, stream);
    }
    return check_launch(what);
}
extern "C" int up_crop_to_nhwc(const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                               const int32_t* valid_hw, const double* inv, int B, float border, float mean, float stdv, float* y_nhwc,
                               float* y_flip_nhwc, int Ho, int Wo, int ldy, void* stream) {
    return crop_to_nhwc("crop_to_nhwc", src_hwc, src_type, F, Hs, Ws, C, frame_of, valid_hw, inv, B, 0, border, mean, stdv, y_nhwc,
                        y_flip_nhwc, Ho, Wo, ldy, stream);
}
extern "C" int up_clip_crop_to_nhwc(const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                                    const int32_t* valid_hw, const double* inv, int B, int T, float border, float mean, float stdv,
                                    float* y_nhwc, float* y_flip_nhwc, int Ho, int Wo, int ldy, void* stream) {
    UP_REQUIRE(T > 0, UP_ERR_INVALID, "clip_crop_to_nhwc: %d frames per sample", T);
    return crop_to_nhwc("clip_crop_to_nhwc", src_hwc, src_type, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv, y_nhwc,
                        y_flip_nhwc, Ho, Wo, ldy, stream);
}
extern "C" int up_clip_crop_to_nhwc_strided(const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                                            const int32_t* valid_hw, const double* inv, int B, int T, float border, float mean, float stdv,
                                            float* y_nhwc, float* y_flip_nhwc, int Ho, int Wo, int ldy, int frame_images, int first,
                                            void* stream) {
    UP_REQUIRE(T > 0, UP_ERR_INVALID, "clip_crop_to_nhwc_strided: %d frames per sample", T);
    return crop_to_nhwc("clip_crop_to_nhwc_strided", src_hwc, src_type, F, Hs, Ws, C, frame_of, valid_hw, inv, B, T, border, mean, stdv,
                        y_nhwc, y_flip_nhwc, Ho, Wo, ldy, stream, true, frame_images, first);
}

// the three centre-pool entries: one set of refusals, one kernel
static int center_pool(const char* what, bool clip, bool flip, const double* center_xy, double sigma, float* y, int ldy, int coff, int B,
                       int T, int H, int W, int P, int Q, void* stream, bool strided = false, int frame_images = 0, int first = 0) {
    UP_REQUIRE(center_xy && y, UP_ERR_INVALID, "%s: null argument", what);
    UP_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && ldy > 0, UP_ERR_INVALID, "%s: %d x %d maps of %d x %d, ldy %d", what, B, T, H, W, ldy);
    UP_REQUIRE(sigma > 0, UP_ERR_INVALID, "%s: sigma %g", what, sigma);
    UP_REQUIRE(coff >= 0 && coff < ldy, UP_ERR_INVALID, "%s: channel %d of %d", what, coff, ldy);
    UP_REQUIRE(P == (H + 2 - 9) / 8 + 1 && Q == (W + 2 - 9) / 8 + 1 && P > 0 && Q > 0, UP_ERR_INVALID, "%s: P,Q mismatch", what);
    UP_REQUIRE((int64_t)H * W <= INT32_MAX, UP_ERR_INVALID, "%s: %d x %d: a pixel index beyond the int32 range", what, H, W);
    const int64_t total = (int64_t)T * B * P * Q;
    const double skip = 9.4 * sigma * sigma;
    if (strided) {
        if (int e = clip_stride_ok(what, B, T, frame_images, first)) return e;
        if (flip)
            UP_LAUNCH_1D(clip_center_pool_strided_kernel<true>, total, as_stream(stream), center_xy, sigma, skip, y, ldy, coff, B, T, H, W, P,
                         Q, total, frame_images, first);
        else
            UP_LAUNCH_1D(clip_center_pool_strided_kernel<false>, total, as_stream(stream), center_xy, sigma, skip, y, ldy, coff, B, T, H, W, P,
                         Q, total, frame_images, first);
        return check_launch(what);
    }
    if (!clip)
        UP_LAUNCH_1D((center_pool_kernel<false, false>), total, as_stream(stream), center_xy, sigma, skip, y, ldy, coff, B, T, H, W, P, Q,
                     total);
    else if (!flip)
        UP_LAUNCH_1D((center_pool_kernel<true, false>), total, as_stream(stream), center_xy, sigma, skip, y, ldy, coff, B, T, H, W, P, Q,
                     total);
    else
        UP_LAUNCH_1D((center_pool_kernel<true, true>), total, as_stream(stream), center_xy, sigma, skip, y, ldy, coff, B, T, H, W, P, Q,
                     total);
    return check_launch(what);
}
extern "C" int up_center_pool(const double* center_xy, double sigma, float* y, int ldy, int coff, int N, int H, int W, int P, int Q,
                              void* stream) {
    return center_pool("center_pool", false, false, center_xy, sigma, y, ldy, coff, N, 1, H, W, P, Q, stream);
}
extern "C" int up_clip_center_pool(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W, int P,
                                   int Q, void* stream) {
    return center_pool("clip_center_pool", true, false, center_xy, sigma, y, ldy, coff, B, T, H, W, P, Q, stream);
}
extern "C" int up_clip_center_pool_flip(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W,
                                        int P, int Q, void* stream) {
    return center_pool("clip_center_pool_flip", true, true, center_xy, sigma, y, ldy, coff, B, T, H, W, P, Q, stream);
}
extern "C" int up_clip_center_pool_strided(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W,
                                           int P, int Q, int frame_images, int first, void* stream) {
    return center_pool("clip_center_pool_strided", true, false, center_xy, sigma, y, ldy, coff, B, T, H, W, P, Q, stream, true, frame_images,
                       first);
}
extern "C" int up_clip_center_pool_flip_strided(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H,
                                                int W, int P, int Q, int frame_images, int first, void* stream) {
    return center_pool("clip_center_pool_flip_strided", true, true, center_xy, sigma, y, ldy, coff, B, T, H, W, P, Q, stream, true,
                       frame_images, first);
}

extern "C" int up_peak_mask(const float* maps, int nmaps, int H, int W, uint8_t* mask, void* stream) {
    UP_REQUIRE(maps && mask && nmaps > 0 && H > 0 && W > 0, UP_ERR_INVALID, "peak_mask: bad argument");
    long long total = (long long)nmaps * H * W;
    hipLaunchKernelGGL(peak_mask_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), maps, total, H, W, mask);
    return check_launch("peak_mask");
}
extern "C" int up_box_argmax(const float* maps, int C, int H, int W, const int32_t* boxes, int P, int ch0, int nch,
                             int32_t* out_hw, void* stream) {
    UP_REQUIRE(maps && boxes && out_hw && C > 0 && H > 0 && W > 0 && P > 0, UP_ERR_INVALID, "box_argmax: bad argument");
    UP_REQUIRE(ch0 >= 0 && nch > 0 && ch0 + nch <= C, UP_ERR_INVALID, "box_argmax: channels %d..%d of %d", ch0,
               ch0 + nch - 1, C);
    hipLaunchKernelGGL(box_argmax_kernel, dim3(cdiv((long long)P * nch, 4)), dim3(256), 0, as_stream(stream), maps, H, W,
                       boxes, P, ch0, nch, out_hw);
    return check_launch("box_argmax");
}
extern "C" int up_persons_decode(const float* maps, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int C, int H, int W,
                                 int box_ch0, int joint_ch0, int njoints, int max_persons, int32_t* count, int32_t* status,
                                 int32_t* kpts, void* stream) {
    UP_REQUIRE(maps && count && status && kpts, UP_ERR_INVALID, "persons_decode: null argument");
    UP_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && stride_b > 0 && stride_j > 0 && stride_p > 0, UP_ERR_INVALID,
               "persons_decode: %d samples of %d maps of %d x %d, strides %lld / %lld / %lld", B, C, H, W, (long long)stride_b,
               (long long)stride_j, (long long)stride_p);
    UP_REQUIRE(max_persons >= 1 && max_persons <= UP_PERSONS_CAP, UP_ERR_INVALID, "persons_decode: max_persons %d (1..%d)", max_persons,
               UP_PERSONS_CAP);
    UP_REQUIRE(box_ch0 >= 0 && (int64_t)box_ch0 + 5 <= C, UP_ERR_INVALID, "persons_decode: box channels %d..%lld of %d", box_ch0,
               (long long)box_ch0 + 4, C);
    UP_REQUIRE(joint_ch0 >= 0 && njoints >= 1 && (int64_t)joint_ch0 + njoints <= C, UP_ERR_INVALID,
               "persons_decode: %d joint channels from %d of %d", njoints, joint_ch0, C);
    const int64_t lim = INT32_MAX;
    UP_REQUIRE((int64_t)H * W <= lim && stride_b <= lim && stride_j <= lim && stride_p <= lim && (B - 1) * stride_b <= lim &&
                   (C - 1) * stride_j <= lim && ((int64_t)H * W - 1) * stride_p <= lim &&
                   (B - 1) * stride_b + (C - 1) * stride_j + ((int64_t)H * W - 1) * stride_p <= lim &&
                   (int64_t)B * max_persons * (njoints + 5) * 2 <= lim,
               UP_ERR_INVALID, "persons_decode: %d samples of %d maps of %d x %d, %d persons: an index beyond the int32 range", B, C, H, W,
               max_persons);
    const dim3 grid(B), block(256);
    if ((int64_t)5 * H * W <= DECODE_LDS)
        hipLaunchKernelGGL(persons_kernel<true>, grid, block, 0, as_stream(stream), maps, stride_b, stride_j, stride_p, H, W,
                           make_fastdiv(W), box_ch0, joint_ch0, njoints, max_persons, count, status, kpts);
    else
        hipLaunchKernelGGL(persons_kernel<false>, grid, block, 0, as_stream(stream), maps, stride_b, stride_j, stride_p, H, W,
                           make_fastdiv(W), box_ch0, joint_ch0, njoints, max_persons, count, status, kpts);
    return check_launch("persons_decode");
}

extern "C" int up_pck_accuracy(const float* pred_xy, const float* target_xy, int B, int J, int H, int W, int dataset,
                               double thr_pck, double thr_pckh, double* acc, double* pck, double* pckh, double* visible,
                               int32_t* cnt, void* stream) {
    UP_REQUIRE(pred_xy && target_xy && acc && pck && pckh && visible && cnt && B > 0 && H > 0 && W > 0, UP_ERR_INVALID,
               "pck_accuracy: bad argument");
    UP_REQUIRE(J > 0 && J <= 256, UP_ERR_UNSUPPORTED, "pck_accuracy: %d joints (1..256 supported)", J);
    static const int need[] = {15, 14, 9, 5, 14, 8, 11};   // joints the head / torso formulas of each dataset touch
    UP_REQUIRE(dataset >= UP_DS_LSP && dataset <= UP_DS_MPII, UP_ERR_INVALID, "pck_accuracy: unknown dataset id %d", dataset);
    UP_REQUIRE(J >= need[dataset], UP_ERR_INVALID, "pck_accuracy: dataset %d needs at least %d joint channels, got %d",
               dataset, need[dataset], J);
    hipLaunchKernelGGL(pck_kernel, dim3(1), dim3(256), 0, as_stream(stream), pred_xy, target_xy, B, J, H, W, dataset,
                       (float)thr_pck, (float)thr_pckh, acc, pck, pckh, visible, cnt);
    return check_launch("pck_accuracy");
}
