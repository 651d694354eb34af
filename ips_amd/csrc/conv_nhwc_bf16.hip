// conv_nhwc_bf16.hip - the layer-by-layer trunk under IPSX_PRECISION=bf16 ("bf16 layered trunk"): implicit-GEMM
// convolution on channels-last bf16 activations, the bf16 average pool and the fp32 -> bf16 rounding of the pooled map.
// No reference behaviour exists at this precision; the oracle is a float64 emulation that rounds where this file
// rounds (tests/test_trunk_layered_bf16.py).
//
//   y[m][o] = bf16( relu( fma(sum_k x[m][k] * bf16(W[o][k]), alpha[o], shift[o]) + widen(res[m][o]) ) )
//
//  * A operand: the STORED bf16 activations, x[pixel][C_in]; a lane's 8 consecutive k of a k-step are one 16-byte raw
//    buffer load, halo (padding) lanes carry an out-of-range offset and read zeros, the pixel offset changes once per
//    tap and the channel offset is a scalar (the data path of conv_nhwc_kernel).
//  * B operand: ipsx_pack_conv_weight_bf16, [C_out/32][K/16][64 lanes][8 bf16], k tap-major - with C_in % 16 == 0 a
//    k-step never straddles a tap.
//  * v_mfma_f32_32x32x16_bf16, fp32 accumulation, ONE chain per output element over k-steps 0, 1, 2, ... whatever the
//    tile, launch or chunk the pixel falls into; padding taps are multiplied as zeros.
//  * Epilogue in fp32: affine, + the bf16 shortcut widened exactly, ReLU, one rounding to bf16 (nearest even).  The
//    accumulators hold 4 consecutive ROWS per lane, so each wavefront turns its 32 x 64 pieces through a private LDS
//    slab and a lane stores 8 consecutive channels (16 bytes) of one pixel; the shortcut is read the same way.
//
// Wave tile 64 pixels x 32 NTW channels (NTW = 4: eight accumulators, six loads per eight MFMAs - a weight load serves
// 64 pixels, an activation load 128 channels), operands through a register ring requested RING - 1 k-steps ahead; the
// four wavefronts of a workgroup lie WM x WN, along N for wide layers so that the activation rows are fetched from HBM
// once per workgroup and come out of the L1 for the other three.  M runs over ALL pixels of the launch (small maps:
// 512 channels at 4x4 are 16 pixels per patch).

#include <algorithm>

#include "ipsx_internal.h"
#include "ipsx_math.h"

namespace ipsx {

typedef __bf16 cb_bf16x8 __attribute__((ext_vector_type(8)));
typedef float cb_f32x16 __attribute__((ext_vector_type(16)));
typedef float cb_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cb_u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kOobH = 0x80000000u;     // voffset of a padding lane: beyond any buffer we bind
constexpr int CB_EP = 68;                   // floats per row of a wavefront's epilogue slab (64 channels + 4 pad)

struct NhwcBf16Args {
    const void* x;         // bf16 (n, h, w, c_in)
    const void* wp;        // packed bf16 weights
    const float* alpha;
    const float* shift;
    const void* res;       // bf16 (n, ho, wo, c_out) or null
    void* y;               // bf16 (n, ho, wo, c_out)
    unsigned m_total;      // n * ho * wo
    unsigned x_bytes, w_bytes;
    int c_in, h, w, c_out, ho, wo, kh, kw, stride, pad, relu;
    int spt;               // k-steps per tap = c_in / 16
    int ksteps;            // kh * kw * c_in / 16
};

template <int NTW>
struct CbStage {
    cb_u32x4 a0, a1, b[NTW];
};

__device__ __forceinline__ cb_u32x4 cb_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
}

struct CbPixel {
    int iy0, ix0;          // top-left input coordinate of the receptive field
    unsigned img_pix;      // img * h * w
    bool valid;
};

__device__ __forceinline__ CbPixel cb_pixel(const NhwcBf16Args& a, unsigned m) {
    CbPixel p;
    p.valid = m < a.m_total;
    const unsigned howo = (unsigned)(a.ho * a.wo);
    const unsigned mm = p.valid ? m : 0u;
    const unsigned img = mm / howo, pix = mm - img * howo;
    const unsigned oy = pix / (unsigned)a.wo, ox = pix - oy * (unsigned)a.wo;
    p.iy0 = (int)oy * a.stride - a.pad;
    p.ix0 = (int)ox * a.stride - a.pad;
    p.img_pix = img * (unsigned)(a.h * a.w);
    return p;
}

// byte offset of this lane's source pixel row (+ its half's 8 channels) for a tap, or kOobH
__device__ __forceinline__ unsigned cb_voff(const NhwcBf16Args& a, const CbPixel& p, int tap, int half) {
    const int ky = tap / a.kw, kx = tap - ky * a.kw;
    const int iy = p.iy0 + ky, ix = p.ix0 + kx;
    const bool ok = p.valid && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w;
    return ok ? ((p.img_pix + (unsigned)(iy * a.w + ix)) * (unsigned)a.c_in + 8u * half) * 2u : kOobH;
}

template <int WM, int WN, int NTW, int RING>
__global__ __launch_bounds__(256, 2) void conv_nhwc_bf16_kernel(NhwcBf16Args a) {
    __shared__ __attribute__((aligned(16))) float s_ep[4][32 * CB_EP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const unsigned m_base = (blockIdx.x * WM + wm) * 64u;
    const int nt0 = (blockIdx.y * WN + wn) * NTW;                   // first of this wave's n-tiles
    if (m_base >= a.m_total || nt0 * 32 >= a.c_out) return;         // wave-uniform (no workgroup barrier below)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wp), 0, (int)a.w_bytes, 0x00020000);
    const CbPixel p0 = cb_pixel(a, m_base + (lane & 31));
    const CbPixel p1 = cb_pixel(a, m_base + 32 + (lane & 31));
    const unsigned lb = lane * 16u;
    const int n_tiles = (a.c_out + 31) / 32;
    unsigned wb[NTW];                                               // byte offset of every n-tile's weight stream
#pragma unroll                                                      // (a tile beyond C_out re-reads the last real one;
    for (int t = 0; t < NTW; ++t)                                   //  its accumulators are never stored)
        wb[t] = (unsigned)min(nt0 + t, n_tiles - 1) * (unsigned)a.ksteps * 1024u;
    const int total = a.ksteps;

    cb_f32x16 acc[2][NTW];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // prefetch stream state: k-step gp = (tap pt, k-step pc of the tap); pv0 / pv1 = pixel offsets of tap pt
    int gp = 0, pt = 0, pc = 0;
    unsigned pv0 = cb_voff(a, p0, 0, half), pv1 = cb_voff(a, p1, 0, half);
    CbStage<NTW> st[RING];
#define CB_ISSUE(S)                                                         \
    do {                                                                    \
        const unsigned ca = (unsigned)pc * 32u, cb = (unsigned)gp * 1024u;  \
        S.a0 = cb_load(rx, pv0, ca);                                        \
        S.a1 = cb_load(rx, pv1, ca);                                        \
        _Pragma("unroll") for (int t = 0; t < NTW; ++t) S.b[t] = cb_load(rw, lb, wb[t] + cb); \
    } while (0)
// (past the last k-step the state stays there: the ring's look-ahead re-requests it and nobody consumes it)
#define CB_ADVANCE()                                                        \
    do {                                                                    \
        if (gp + 1 < total) {                                               \
            ++gp;                                                           \
            if (++pc == a.spt) {                                            \
                pc = 0; ++pt;                                               \
                pv0 = cb_voff(a, p0, pt, half);                             \
                pv1 = cb_voff(a, p1, pt, half);                             \
            }                                                               \
        }                                                                   \
    } while (0)
#pragma unroll
    for (int r = 0; r < RING - 1; ++r) { CB_ISSUE(st[r]); CB_ADVANCE(); }
#pragma unroll 1
    for (int g = 0; g < total; g += RING) {
#pragma unroll
        for (int r = 0; r < RING; ++r) {
            if (g + r < total) {                                    // wave-uniform
                CB_ISSUE(st[(r + RING - 1) % RING]);
                const cb_bf16x8 a0 = __builtin_bit_cast(cb_bf16x8, st[r].a0), a1 = __builtin_bit_cast(cb_bf16x8, st[r].a1);
#pragma unroll
                for (int t = 0; t < NTW; ++t) {
                    const cb_bf16x8 b = __builtin_bit_cast(cb_bf16x8, st[r].b[t]);
                    acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b, acc[1][t], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                CB_ADVANCE();
            }
        }
    }
#undef CB_ADVANCE
#undef CB_ISSUE

    // epilogue.  Accumulator register r of lane l: pixel 32 mt + (r & 3) + 8 (r >> 2) + 4 (l >> 5), channel 32 nt + (l & 31).
    // Pieces of 32 pixels x 64 channels go through this wavefront's slab (affine applied on the way in, where the
    // lane's channel is fixed); on the way out a lane holds 8 consecutive channels of one pixel.
    float* slab = s_ep[wave];
    const int i = lane & 31;
    const unsigned short* res = static_cast<const unsigned short*>(a.res);
    unsigned short* y = static_cast<unsigned short*>(a.y);
#pragma unroll
    for (int np = 0; np < NTW / 2; ++np) {
        const int c_base = (nt0 + 2 * np) * 32;                     // first channel of the piece
        if (c_base >= a.c_out) break;                               // wave-uniform
        float al[2], sh[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int n = min(c_base + 32 * q + i, a.c_out - 1);
            al[q] = a.alpha ? a.alpha[n] : 1.0f;
            sh[q] = a.shift ? a.shift[n] : 0.0f;
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[mt][2 * np + q][r];
                    if (a.alpha) v = __builtin_fmaf(v, al[q], sh[q]);
                    else if (a.shift) v = v + sh[q];
                    slab[((r & 3) + 8 * (r >> 2) + 4 * half) * CB_EP + 32 * q + i] = v;
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int id = q * 64 + lane, row = id >> 3, c0 = c_base + 8 * (id & 7);
                const unsigned m = m_base + 32 * mt + row;
                if (m >= a.m_total || c0 >= a.c_out) continue;      // (C_out % 8 == 0: a chunk is inside or outside)
                const cb_f32x4 lo = *reinterpret_cast<const cb_f32x4*>(slab + row * CB_EP + 8 * (id & 7));
                const cb_f32x4 hi = *reinterpret_cast<const cb_f32x4*>(slab + row * CB_EP + 8 * (id & 7) + 4);
                float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const size_t idx = (size_t)m * a.c_out + c0;
                if (res) {
                    const uint4 rr = *reinterpret_cast<const uint4*>(res + idx);
                    const unsigned w4[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[2 * j] = v[2 * j] + __uint_as_float(w4[j] << 16);
                        v[2 * j + 1] = v[2 * j + 1] + __uint_as_float(w4[j] & 0xffff0000u);
                    }
                }
                cb_bf16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float t = a.relu ? (v[j] > 0.0f ? v[j] : 0.0f) : v[j];
                    o[j] = (__bf16)t;
                }
                *reinterpret_cast<uint4*>(y + idx) = __builtin_bit_cast(uint4, o);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// the pooled fp32 map -> bf16 (round to nearest even), 8 values per thread
__global__ void round_to_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, size_t total8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const float4 lo = reinterpret_cast<const float4*>(x)[2 * i], hi = reinterpret_cast<const float4*>(x)[2 * i + 1];
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    cb_bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
    reinterpret_cast<uint4*>(y)[i] = __builtin_bit_cast(uint4, o);
}

// nn.AdaptiveAvgPool2d(1) on channels-last bf16 activations: (n, hw, c) -> (n, c) float32; the fp32 sum over the pixels
// in avgpool_nhwc_kernel's order, the same division
__global__ void avgpool_nhwc_bf16_kernel(const unsigned short* __restrict__ x, float* __restrict__ y, size_t total, int c, int hw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t img = i / c;
    const int ch = (int)(i - img * c);
    const unsigned short* src = x + img * (size_t)hw * c + ch;
    float s = 0.0f;
    for (int j = 0; j < hw; ++j) s = s + __uint_as_float((unsigned)src[(size_t)j * c] << 16);
    y[i] = s / (float)hw;
}

int round_to_bf16(const float* x, void* y, size_t count, hipStream_t s) {
    IPSX_REQUIRE(x && y && count % 8 == 0, "round_to_bf16: bad arguments");
    if (!count) return IPSX_OK;
    round_to_bf16_kernel<<<dim3((unsigned)cdiv(count / 8, 256)), dim3(256), 0, s>>>(x, static_cast<unsigned short*>(y), count / 8);
    return launched("round_to_bf16");
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_conv2d_affine_nhwc_bf16_supported(const ipsx_conv* cv) {
    return cv && cv->c_in > 0 && cv->c_in % 16 == 0 && cv->c_out > 0 && cv->c_out % 8 == 0 && cv->kh > 0 && cv->kw > 0 &&
           cv->stride > 0 && cv->pad >= 0 ? 1 : 0;
}

IPSX_API int ipsx_conv2d_affine_nhwc_bf16(const ipsx_conv* cv, const void* x, const void* residual, void* y, int64_t n, int h,
                                          int w, int relu, void* stream) {
    IPSX_REQUIRE(cv && x && y && n >= 0 && h > 0 && w > 0, "conv2d_affine_nhwc_bf16: bad arguments");
    IPSX_REQUIRE(cv->c_in > 0 && cv->c_in % 16 == 0, "conv2d_affine_nhwc_bf16: C_in = %d is not a multiple of 16", cv->c_in);
    IPSX_REQUIRE(ipsx_conv2d_affine_nhwc_bf16_supported(cv), "conv2d_affine_nhwc_bf16: %d -> %d, %dx%d / %d pad %d is not supported "
                 "(C_in %% 16 == 0, C_out %% 8 == 0)", cv->c_in, cv->c_out, cv->kh, cv->kw, cv->stride, cv->pad);
    IPSX_REQUIRE(cv->w_packed_bf16, "conv2d_affine_nhwc_bf16: cv->w_packed_bf16 (ipsx_pack_conv_weight_bf16) is needed");
    IPSX_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)residual & 15) == 0,
                 "conv2d_affine_nhwc_bf16: activations must start at 16-byte addresses");
    if (n == 0) return IPSX_OK;
    const int ho = conv_out(h, cv->kh, cv->stride, cv->pad), wo = conv_out(w, cv->kw, cv->stride, cv->pad);
    IPSX_REQUIRE(ho > 0 && wo > 0, "conv2d_affine_nhwc_bf16: empty output");
    const int64_t howo = (int64_t)ho * wo;
    const int ksteps = cv->kh * cv->kw * cv->c_in / 16;
    const int64_t w_bytes = (int64_t)cdiv(cv->c_out, 32) * ksteps * 1024;
    IPSX_REQUIRE(w_bytes < ((int64_t)1 << 31), "conv2d_affine_nhwc_bf16: weights too large for one buffer");
    // per launch: input below 2 GiB (buffer range + the out-of-range marker), output pixels below 2^30
    const int64_t in_img = (int64_t)h * w * cv->c_in * 2;
    int64_t per = std::min<int64_t>(n, std::max<int64_t>(1, (((int64_t)1 << 31) - 65536) / in_img));
    per = std::min<int64_t>(per, std::max<int64_t>(1, ((int64_t)1 << 30) / howo));
    hipStream_t s = as_stream(stream);
    for (int64_t i0 = 0; i0 < n; i0 += per) {
        const int64_t cnt = std::min(per, n - i0);
        NhwcBf16Args a;
        a.x = static_cast<const unsigned short*>(x) + (size_t)i0 * h * w * cv->c_in;
        a.y = static_cast<unsigned short*>(y) + (size_t)i0 * howo * cv->c_out;
        a.res = residual ? static_cast<const unsigned short*>(residual) + (size_t)i0 * howo * cv->c_out : nullptr;
        a.wp = cv->w_packed_bf16; a.alpha = cv->alpha; a.shift = cv->shift;
        a.m_total = (unsigned)(cnt * howo);
        a.x_bytes = (unsigned)(cnt * in_img);
        a.w_bytes = (unsigned)w_bytes;
        a.c_in = cv->c_in; a.h = h; a.w = w; a.c_out = cv->c_out; a.ho = ho; a.wo = wo;
        a.kh = cv->kh; a.kw = cv->kw; a.stride = cv->stride; a.pad = cv->pad; a.relu = relu;
        a.spt = cv->c_in / 16; a.ksteps = ksteps;
        const unsigned mt64 = (unsigned)cdiv(a.m_total, 64);
        const dim3 block(256);
        if (cv->c_out >= 512)             // 64 pixels x 512 channels per workgroup: the four waves share the activation rows
            conv_nhwc_bf16_kernel<1, 4, 4, 3><<<dim3(mt64, (unsigned)cdiv(cv->c_out, 512)), block, 0, s>>>(a);
        else if (cv->c_out >= 256)        // 128 x 256
            conv_nhwc_bf16_kernel<2, 2, 4, 3><<<dim3((unsigned)cdiv(mt64, 2), (unsigned)cdiv(cv->c_out, 256)), block, 0, s>>>(a);
        else if (cv->c_out > 64)          // 256 x 128
            conv_nhwc_bf16_kernel<4, 1, 4, 3><<<dim3((unsigned)cdiv(mt64, 4), (unsigned)cdiv(cv->c_out, 128)), block, 0, s>>>(a);
        else                              // 256 x 64
            conv_nhwc_bf16_kernel<4, 1, 2, 4><<<dim3((unsigned)cdiv(mt64, 4), 1), block, 0, s>>>(a);
        IPSX_TRY(launched("conv2d_affine_nhwc_bf16"));
    }
    return IPSX_OK;
}

IPSX_API int ipsx_avgpool_nhwc_bf16(const void* x, float* y, int64_t n, int c, int hw, void* stream) {
    IPSX_REQUIRE(x && y && n >= 0 && c > 0 && hw > 0, "avgpool_nhwc_bf16: bad arguments");
    const size_t total = (size_t)n * c;
    if (!total) return IPSX_OK;
    avgpool_nhwc_bf16_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream)>>>(
        static_cast<const unsigned short*>(x), y, total, c, hw);
    return launched("avgpool_nhwc_bf16");
}
