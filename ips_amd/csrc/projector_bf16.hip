// projector_bf16.hip - the feature projector (IPSNet.get_projector: LayerNorm -> Linear -> BatchNorm1d -> ReLU) on the
// bf16 matrix pipe, for IPSX_PRECISION=bf16 ("bf16 projector").  No reference behaviour exists at this
// precision; the oracle is a float64 emulation that rounds where this file rounds (tests/test_projector_bf16.py).
//
//   out[r][o] = relu(alpha[o] * (|rstd_r| * sum_k bf16(x[r][k] - mean_r) * bf16(W[o][k])) + shift[o])
//
//  * (mean_r, rstd_r): ipsx_projector_stats_typed - the fp32 moments of the STORED values widened exactly
//    (ipsx_rowstats.h row_moments_wave32<T>): a row stored as float16 / bfloat16 gets the bits of the same values passed
//    as float32.  rstd < 0 marks a row the fp32 path centres; here every row is centred, so only |rstd| is used.
//  * A operand: the row centred in fp32, then rounded to bf16 (nearest even) in registers.  Centring BEFORE rounding: the
//    fp32 path's folded epilogue rstd (x W^T - mean colsum W) cancels at 8 significant bits on rows whose mean dwarfs
//    their spread.
//  * B operand: W rounded to bf16 - ipsx_pack_conv_weight_bf16 of W as a 1x1 convolution, [D/32][F/16][64 lanes][8].
//  * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, k-steps ascending: every output's sum runs in one fixed order,
//    whichever rows share its tile or its launch.
//  * fp32 epilogue: |rstd| * acc, then the Linear bias + BatchNorm as one affine (fma(t, alpha, shift)), then ReLU.
//
// Tiles: a workgroup of four wavefronts takes 32 MT rows; wavefront w the NT output tiles of 32 columns from
// (4 blockIdx.y + w) NT on, for all MT 32-row blocks (MT x NT accumulators of 16 registers).  Every wavefront reads its
// rows itself (16 B per lane per 8 k when stored as 16-bit values, 32 B as float32; the four wavefronts of a workgroup
// share them through the L1), one k-step ahead of its MFMAs; W (2 MiB at F = 2048, D = 512) stays in the L2.  MT = 2:
// 64-row workgroups, the unit selection.py sizes the launches of features_persistent in.  MT = 4 (128 rows, 256
// accumulator registers) halves the weight traffic per row - 253 us for 65,536 f16 rows alone, against 292-294 us for
// MT = 2 in other runs of the same tool - but leaves half the compute units of those launches idle: 16 slides per call
// 95.8 -> 77.9 M rows/s.  A ring of four k-steps in flight instead of one was slower too: 352 us, 86.5 M.

#include "ipsx_common.h"
#include "ipsx_math.h"
#include "ipsx_rowstats.h"

namespace ipsx {

typedef __bf16 pb_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 pb_f16x8 __attribute__((ext_vector_type(8)));
typedef float pb_f32x16 __attribute__((ext_vector_type(16)));

// (mean, rstd) of rows stored as T (one wavefront per 32 rows): row_moments_kernel (aggregate.hip) for typed storage
template <typename T>
__global__ __launch_bounds__(256) void row_moments_typed_kernel(const T* __restrict__ x, long long n, int d, float eps,
                                                                float2* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long row0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (row0 >= n) return;
    const float2 st = row_moments_wave32(x, row0, n, d, eps, lane);
    if (lane < 32 && row0 + lane < n) stats[row0 + lane] = st;
}

// Row-indexed form (ipsx_projector_stats_indexed): stats[j] = the moments of source row index[j] - the bits of
// row_moments_typed_kernel run on x[index]; only the row base differs, computed in 64 bits (a row number outside the
// source tensor is clamped into it: never read out of bounds).
template <typename T>
__global__ __launch_bounds__(256) void row_moments_indexed_kernel(const T* __restrict__ x, const int* __restrict__ index,
                                                                  long long src_rows, long long n, int d, float eps,
                                                                  float2* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long row0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (row0 >= n) return;
    const long long row = row0 + (lane & 31);
    const long long src = source_row(index, row < n ? row : n - 1, src_rows);
    const float2 st = row_moments_at(x + (size_t)src * d + 4 * (lane >> 5), d, eps, lane);
    if (lane < 32 && row0 + lane < n) stats[row0 + lane] = st;
}

// eight consecutive stored values of one row, as loaded (widened at use, so the loads of the next k-step are in flight
// while this one's MFMAs run)
template <typename T> struct Raw8 { uint4 a; };
template <> struct Raw8<float> { uint4 a, b; };

__device__ __forceinline__ void raw_load(Raw8<float>& r, const float* p) {
    r.a = reinterpret_cast<const uint4*>(p)[0];
    r.b = reinterpret_cast<const uint4*>(p)[1];
}
template <typename T>
__device__ __forceinline__ void raw_load(Raw8<T>& r, const T* p) { r.a = *reinterpret_cast<const uint4*>(p); }

__device__ __forceinline__ void widen8(const Raw8<float>& r, float (&v)[8]) {
    v[0] = __uint_as_float(r.a.x); v[1] = __uint_as_float(r.a.y); v[2] = __uint_as_float(r.a.z); v[3] = __uint_as_float(r.a.w);
    v[4] = __uint_as_float(r.b.x); v[5] = __uint_as_float(r.b.y); v[6] = __uint_as_float(r.b.z); v[7] = __uint_as_float(r.b.w);
}
__device__ __forceinline__ void widen8(const Raw8<_Float16>& r, float (&v)[8]) {
    const pb_f16x8 h = __builtin_bit_cast(pb_f16x8, r.a);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
}
__device__ __forceinline__ void widen8(const Raw8<__bf16>& r, float (&v)[8]) {
    const unsigned w[4] = {r.a.x, r.a.y, r.a.z, r.a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[2 * j] = __uint_as_float(w[j] << 16);
        v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
    }
}

struct ProjBf16Args {
    const void* x;
    long long n;
    int f, d, ksteps;
    const uint4* wp;           // [D/32][F/16][64][8 bf16]
    const float2* stats;       // (mean, rstd) per row
    const float* alpha;
    const float* shift;
    float* out;                // (n, d)
    int* ready;                // optional: *ready = ready_value by the first thread (ipsx_projector_apply_publish)
    int ready_value;
    const int* index;          // IDX kernels: output row j reads source row index[j] of x (stats and out stay in output order)
    long long src_rows;
};

template <typename T, int NT, int MT, bool IDX>
__global__ __launch_bounds__(256) void projector_bf16_kernel(ProjBf16Args a) {
    // (everything enqueued before this launch has completed and is visible - the stream order of two kernels - so the
    //  first thread can say so on behalf of a launch of its own)
    if (a.ready && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        __hip_atomic_store(a.ready, a.ready_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int t0 = ((int)blockIdx.y * 4 + wave) * NT;               // first 32-column output tile of this wavefront
    if (t0 * 32 >= a.d) return;                                     // wave-uniform; (D / 32) % NT == 0
    const long long r0 = (long long)blockIdx.x * (32 * MT);
    const T* x = static_cast<const T*>(a.x);
    const T* xp[MT];
    float mean[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const long long row = r0 + 32 * m + (lane & 31);
        const long long rc = row < a.n ? row : a.n - 1;             // rows past the end read the last one, write nothing
        xp[m] = x + (size_t)(IDX ? source_row(a.index, rc, a.src_rows) : rc) * a.f + 8 * half;
        mean[m] = a.stats[rc].x;
    }
    const uint4* wp = a.wp + (size_t)t0 * a.ksteps * 64 + lane;
    pb_f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][i][r] = 0.0f;
    Raw8<T> ra[MT];
    uint4 rb[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) raw_load(ra[m], xp[m]);
#pragma unroll
    for (int i = 0; i < NT; ++i) rb[i] = wp[(size_t)i * a.ksteps * 64];
    for (int ks = 0; ks < a.ksteps; ++ks) {
        pb_bf16x8 av[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float v[8];
            widen8(ra[m], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) av[m][j] = (__bf16)(v[j] - mean[m]);
        }
        uint4 b[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) b[i] = rb[i];
        if (ks + 1 < a.ksteps) {
#pragma unroll
            for (int m = 0; m < MT; ++m) raw_load(ra[m], xp[m] + 16 * (ks + 1));
#pragma unroll
            for (int i = 0; i < NT; ++i) rb[i] = wp[((size_t)i * a.ksteps + ks + 1) * 64];
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int m = 0; m < MT; ++m)
                acc[m][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[m], __builtin_bit_cast(pb_bf16x8, b[i]), acc[m][i], 0, 0, 0);
    }
    // accumulator register r of lane l: row 32 m + (r & 3) + 8 (r >> 2) + 4 (l >> 5), column 32 t + (l & 31)
    float al[NT], sh[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int o = (t0 + i) * 32 + (lane & 31);
        al[i] = a.alpha ? a.alpha[o] : 1.0f;
        sh[i] = a.shift ? a.shift[o] : 0.0f;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long row = r0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (row >= a.n) continue;
            const float rs = __builtin_fabsf(a.stats[row].y);
            float* orow = a.out + (size_t)row * a.d + (lane & 31);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                float v = rs * acc[m][i][r];
                if (a.alpha) v = __builtin_fmaf(v, al[i], sh[i]);
                else if (a.shift) v = v + sh[i];
                orow[(t0 + i) * 32] = v > 0.0f ? v : 0.0f;
            }
        }
}

template <typename T, bool IDX>
static int launch_projector_bf16(const ProjBf16Args& a, hipStream_t s) {
    const int tiles = a.d / 32;
    const int nt = tiles % 4 == 0 ? 4 : (tiles % 2 == 0 ? 2 : 1);
    const dim3 block(256);
    if (nt == 4) projector_bf16_kernel<T, 4, 2, IDX><<<dim3((unsigned)cdiv(a.n, 64), (unsigned)cdiv(tiles, 16)), block, 0, s>>>(a);
    else if (nt == 2) projector_bf16_kernel<T, 2, 2, IDX><<<dim3((unsigned)cdiv(a.n, 64), (unsigned)cdiv(tiles, 8)), block, 0, s>>>(a);
    else projector_bf16_kernel<T, 1, 2, IDX><<<dim3((unsigned)cdiv(a.n, 64), (unsigned)cdiv(tiles, 4)), block, 0, s>>>(a);
    return launched("projector_bf16");
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_projector_stats_typed(const void* x, int dtype, int64_t n, int f, float ln_eps, float* stats, void* stream) {
    IPSX_REQUIRE(dtype >= 0 && dtype <= 2, "projector_stats_typed: dtype %d is not 0 (float32), 1 (bfloat16) or 2 (float16)", dtype);
    if (dtype == 0) return ipsx_projector_stats(static_cast<const float*>(x), n, f, ln_eps, stats, stream);
    IPSX_REQUIRE(x && stats && n >= 0 && f > 0 && f % 8 == 0, "projector_stats_typed: bad arguments (the row length is a multiple of 8)");
    IPSX_REQUIRE(((uintptr_t)x & 7) == 0, "projector_stats_typed: rows must start at 8-byte addresses");
    if (n == 0) return IPSX_OK;
    const dim3 grid((unsigned)cdiv(n, 128)), block(256);
    float2* st = reinterpret_cast<float2*>(stats);
    if (dtype == 1) row_moments_typed_kernel<__bf16><<<grid, block, 0, as_stream(stream)>>>(static_cast<const __bf16*>(x), n, f, ln_eps, st);
    else row_moments_typed_kernel<_Float16><<<grid, block, 0, as_stream(stream)>>>(static_cast<const _Float16*>(x), n, f, ln_eps, st);
    return launched("projector row moments (typed)");
}

IPSX_API int ipsx_projector_stats_indexed(const void* x, int dtype, const int32_t* index, int64_t src_rows, int64_t n, int f,
                                          float ln_eps, float* stats, void* stream) {
    IPSX_REQUIRE(dtype >= 0 && dtype <= 2, "projector_stats_indexed: dtype %d is not 0 (float32), 1 (bfloat16) or 2 (float16)", dtype);
    IPSX_REQUIRE(x && index && stats && src_rows > 0 && n >= 0 && f > 0 && f % 8 == 0,
                 "projector_stats_indexed: bad arguments (the row length is a multiple of 8)");
    IPSX_REQUIRE(((uintptr_t)x & (dtype == 0 ? 15 : 7)) == 0, "projector_stats_indexed: rows must start at %d-byte addresses", dtype == 0 ? 16 : 8);
    if (n == 0) return IPSX_OK;
    const dim3 grid((unsigned)cdiv(n, 128)), block(256);
    float2* st = reinterpret_cast<float2*>(stats);
    hipStream_t s = as_stream(stream);
    if (dtype == 0) row_moments_indexed_kernel<float><<<grid, block, 0, s>>>(static_cast<const float*>(x), index, src_rows, n, f, ln_eps, st);
    else if (dtype == 1) row_moments_indexed_kernel<__bf16><<<grid, block, 0, s>>>(static_cast<const __bf16*>(x), index, src_rows, n, f, ln_eps, st);
    else row_moments_indexed_kernel<_Float16><<<grid, block, 0, s>>>(static_cast<const _Float16*>(x), index, src_rows, n, f, ln_eps, st);
    return launched("projector row moments (indexed)");
}

IPSX_API int ipsx_projector_bf16_supported(const ipsx_conv* lin) {
    return lin && lin->kh == 1 && lin->kw == 1 && lin->stride == 1 && lin->pad == 0 && lin->c_in > 0 && lin->c_in % 16 == 0 &&
           lin->c_out > 0 && lin->c_out % 32 == 0;
}

static int projector_apply_bf16_impl(const ipsx_conv* lin, const void* x, int dtype, const int32_t* index, int64_t src_rows,
                                     int64_t n, const float* stats, float* out, int32_t* ready, int32_t ready_value, void* stream) {
    IPSX_REQUIRE(lin && x && out && stats && n >= 0 && (n > 0 || !ready), "projector_apply_bf16: bad arguments");
    IPSX_REQUIRE(dtype >= 0 && dtype <= 2, "projector_apply_bf16: dtype %d is not 0 (float32), 1 (bfloat16) or 2 (float16)", dtype);
    IPSX_REQUIRE(lin->kh == 1 && lin->kw == 1 && lin->stride == 1 && lin->pad == 0, "projector_apply_bf16: lin must be 1x1");
    IPSX_REQUIRE(lin->c_in > 0 && lin->c_in % 16 == 0, "projector_apply_bf16: F = %d features; the bf16 projector needs F %% 16 == 0",
                 lin->c_in);
    IPSX_REQUIRE(lin->c_out > 0 && lin->c_out % 32 == 0, "projector_apply_bf16: D = %d outputs; the bf16 projector needs D %% 32 == 0",
                 lin->c_out);
    IPSX_REQUIRE(lin->w_packed_bf16, "projector_apply_bf16: lin->w_packed_bf16 (ipsx_pack_conv_weight_bf16 of the Linear's weight "
                 "as a 1x1 convolution) is needed");
    IPSX_REQUIRE(((uintptr_t)x & 15) == 0, "projector_apply_bf16: rows must start at 16-byte addresses");
    if (n == 0) return IPSX_OK;
    ProjBf16Args a;
    a.x = x; a.n = n; a.f = lin->c_in; a.d = lin->c_out; a.ksteps = lin->c_in / 16;
    a.wp = static_cast<const uint4*>(lin->w_packed_bf16);
    a.stats = reinterpret_cast<const float2*>(stats);
    a.alpha = lin->alpha; a.shift = lin->shift; a.out = out;
    a.ready = ready; a.ready_value = ready_value;
    a.index = index; a.src_rows = src_rows;
    hipStream_t s = as_stream(stream);
    if (index) {
        if (dtype == 0) return launch_projector_bf16<float, true>(a, s);
        if (dtype == 1) return launch_projector_bf16<__bf16, true>(a, s);
        return launch_projector_bf16<_Float16, true>(a, s);
    }
    if (dtype == 0) return launch_projector_bf16<float, false>(a, s);
    if (dtype == 1) return launch_projector_bf16<__bf16, false>(a, s);
    return launch_projector_bf16<_Float16, false>(a, s);
}

IPSX_API int ipsx_projector_apply_bf16(const ipsx_conv* lin, const void* x, int dtype, int64_t n, const float* stats, float* out,
                                       int32_t* ready, int32_t ready_value, void* stream) {
    return projector_apply_bf16_impl(lin, x, dtype, nullptr, 0, n, stats, out, ready, ready_value, stream);
}

IPSX_API int ipsx_projector_apply_bf16_indexed(const ipsx_conv* lin, const void* x, int dtype, const int32_t* index, int64_t src_rows,
                                               int64_t n, const float* stats, float* out, int32_t* ready, int32_t ready_value,
                                               void* stream) {
    IPSX_REQUIRE(index && src_rows > 0, "projector_apply_bf16_indexed: an index into src_rows > 0 source rows is needed");
    return projector_apply_bf16_impl(lin, x, dtype, index, src_rows, n, stats, out, ready, ready_value, stream);
}
