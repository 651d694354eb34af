// projector_train.hip - the feature projector of the TRAINING step: LayerNorm (no affine) -> Linear -> BatchNorm1d in
// batch-statistics mode -> ReLU (reference architecture/ips_net.py:54-60 under net.train() with autograd, which
// training/iterative.py::compute_loss differentiates).  The features need no gradient and the LayerNorm has no
// parameters, so the step is two GEMMs over the RAW rows with (mean, rstd) per row as the only saved statistics:
//
//     forward   z[r, o]  = |rstd_r| * sum_f (x[r, f] - mean_r) * W[o, f] + b[o]          (rows x F) . (F x D)
//     backward  dW[o, f] = sum_r (dz[r, o] * |rstd_r|) * (x[r, f] - mean_r),  db[o] = sum_r dz[r, o]
//
// both on v_mfma_f32_32x32x2_f32, LN(x) never in memory.  The BatchNorm + ReLU behind z are bn_train.hip's kernels; the
// forward kernel hands them the column sums of z (around a shift) per 64-row slab off its accumulators, the contract of
// ipsx_conv2d_lds_nhwc_stats, so the BatchNorm's batch statistics cost no pass over z.
//
// The rows are CENTRED IN REGISTERS in both directions (x - mean between load and MFMA): nn.LayerNorm's own algebra on
// every row.  The no-grad projector folds the mean into its epilogue (acc - mean * colsum(W)) and needs a second path for
// the rows on which that cancels; here the subtraction is 8 vector instructions beside the 16 or 32 MFMAs (1,024 or 2,048
// matrix-pipe cycles) of a forward stage and 2 beside the 4 MFMAs of a weight-gradient step - a percent or two - and there is
// one path, no column sums to refresh after every optimiser step, and a constant row (mean exact, ipsx_rowstats.h
// rm_recentred) is exact zeros in both GEMMs.  The statistics are ipsx_projector_stats_typed's; only |rstd| is used (its
// sign marks the rows the no-grad path centres).
//
// Rows stored as float16 / bfloat16 are widened exactly in the operand load: the bits of the same values passed as float32.
//
// INDEXED instantiations (ipsx_projector_train_forward_indexed, ipsx_projector_wgrad_indexed): packed row j of
// stats / z / dz is computed from source row index[j] of x - the filled slots of a zero-padded batch, read where they lie.
// Slabs, chunks, k order and every tree of additions are those of the packed rows, so the results are the bits of the plain
// kernels on the gathered copy x[index].  Only the x operand's address changes; the `false` instantiations are the plain
// kernels.  The source is addressed with 32-bit buffer offsets: a source of 2 GiB or more is refused.

#include <algorithm>

#include "ipsx_common.h"
#include "ipsx_math.h"

namespace ipsx {

typedef float pt_f32x16 __attribute__((ext_vector_type(16)));
typedef float pt_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned pt_u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 pt_f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short pt_u16x4 __attribute__((ext_vector_type(4)));

#define PT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr unsigned kPtOob = 0x80000000u;      // voffset of a lane that must read zeros: beyond any buffer we bind

// four consecutive stored values at byte offset voff + soff, widened exactly
template <typename T>
__device__ __forceinline__ pt_f32x4 pt_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff);
template <>
__device__ __forceinline__ pt_f32x4 pt_load4<float>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(pt_f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
template <>
__device__ __forceinline__ pt_f32x4 pt_load4<_Float16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const pt_u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0);
    return __builtin_convertvector(__builtin_bit_cast(pt_f16x4, u), pt_f32x4);
}
template <>
__device__ __forceinline__ pt_f32x4 pt_load4<__bf16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const pt_u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0);
    return pt_f32x4{__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xffff0000u), __uint_as_float(u[1] << 16),
                    __uint_as_float(u[1] & 0xffff0000u)};
}

// one stored value, widened exactly
template <typename T>
__device__ __forceinline__ float pt_load1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff);
template <>
__device__ __forceinline__ float pt_load1<float>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
template <>
__device__ __forceinline__ float pt_load1<_Float16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const unsigned short u = __builtin_amdgcn_raw_buffer_load_b16(r, (int)voff, (int)soff, 0);
    return (float)__builtin_bit_cast(_Float16, u);
}
template <>
__device__ __forceinline__ float pt_load1<__bf16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const unsigned short u = __builtin_amdgcn_raw_buffer_load_b16(r, (int)voff, (int)soff, 0);
    return __uint_as_float((unsigned)u << 16);
}

// ------------------------------------------------------------------ forward: z = Linear(LN(x)), column sums per slab
// The stage loop of conv_nhwc_kernel for a 1x1 map (conv_nhwc.hip: raw buffer loads, a lane's four consecutive k of a
// k-group in one load, the packed B-operand stream of ipsx_pack_conv_weight, operands requested two stages ahead), the A
// operand typed and centred.  A workgroup is 64 rows x (4 waves x NTW x 32) columns; NTW = 4 at D >= 512: every row is
// read once per workgroup.
struct PtFwdArgs {
    const void* x;             // (n, c_in) as T
    const float* wp;           // ipsx_pack_conv_weight of the (c_out, c_in) weights
    const float* bias;         // c_out
    const float2* stats;       // n x (mean, +-rstd)
    const float* shift;        // c_out: the column sums are taken around it
    float* z;                  // (n, c_out)
    float* partial;            // this launch's first slab of [slabs][2][c_out]
    const int32_t* index;      // INDEXED: the source row of this launch's every row (x: the whole source, x_bytes its size)
    unsigned src_rows;
    unsigned n;
    unsigned x_bytes, w_bytes;
    int c_in, c_out, kgs;
};

// source row of an index entry: a number outside [0, src_rows) is clamped into it (the rule of ipsx_projector_stats_indexed)
__device__ __forceinline__ unsigned pt_src_row(int32_t ix, unsigned src_rows) { return min((unsigned)max(ix, 0), src_rows - 1u); }

template <int NTW>
struct PtStage {
    pt_f32x4 a0, a1, b[NTW];
};

template <typename T, int NTW, bool INDEXED>
__global__ __launch_bounds__(256, 2) void projector_train_fwd_kernel(PtFwdArgs a) {
    const int lane = threadIdx.x & 63, half = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned m_base = blockIdx.x * 64u;
    const int nt0 = (blockIdx.y * 4 + wave) * NTW;
    const int ntiles = a.c_out >> 5;
    if (nt0 >= ntiles) return;                                      // wave-uniform; no barrier below
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, (int)a.w_bytes, 0x00020000);
    const unsigned r0 = m_base + (unsigned)i, r1 = r0 + 32u;
    const bool ok0 = r0 < a.n, ok1 = r1 < a.n;
    unsigned x0 = r0, x1 = r1;                                      // where the lane's two rows lie in x
    if constexpr (INDEXED) {                                        // resolved once, in front of the k-loop
        x0 = ok0 ? pt_src_row(a.index[r0], a.src_rows) : 0u;
        x1 = ok1 ? pt_src_row(a.index[r1], a.src_rows) : 0u;
    }
    const unsigned pv0 = ok0 ? (x0 * (unsigned)a.c_in + 4u * half) * (unsigned)sizeof(T) : kPtOob;
    const unsigned pv1 = ok1 ? (x1 * (unsigned)a.c_in + 4u * half) * (unsigned)sizeof(T) : kPtOob;
    const float mean0 = ok0 ? a.stats[r0].x : 0.0f, mean1 = ok1 ? a.stats[r1].x : 0.0f;      // (a row that is not there: 0 - 0)
    const unsigned lb = lane * 16u;
    unsigned wb[NTW];                                               // a tile beyond C_out re-reads the last real one,
#pragma unroll                                                      // its accumulators are never stored
    for (int t = 0; t < NTW; ++t) wb[t] = (unsigned)min(nt0 + t, ntiles - 1) * (unsigned)a.kgs * 1024u;

    pt_f32x16 acc[2][NTW];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[u][t][r] = 0.0f;

    int gp = 0;
    PtStage<NTW> s0, s1, s2;
    auto issue = [&](PtStage<NTW>& s) {
        const unsigned ca = (unsigned)gp * 8u * (unsigned)sizeof(T), cb = (unsigned)gp * 1024u;
        s.a0 = pt_load4<T>(rx, pv0, ca);
        s.a1 = pt_load4<T>(rx, pv1, ca);
#pragma unroll
        for (int t = 0; t < NTW; ++t) s.b[t] = __builtin_bit_cast(pt_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)lb, (int)(wb[t] + cb), 0));
        if (gp + 1 < a.kgs) ++gp;
    };
    auto mma = [&](const PtStage<NTW>& s) {
        const pt_f32x4 c0 = s.a0 - mean0, c1 = s.a1 - mean1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[0][t] = PT_MFMA(c0[j], s.b[t][j], acc[0][t]);
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[1][t] = PT_MFMA(c1[j], s.b[t][j], acc[1][t]);
        }
    };
    issue(s0);
    issue(s1);
#pragma unroll 1
    for (int g = 0; g < a.kgs; g += 3) {
        issue(s2); mma(s0);
        if (g + 1 < a.kgs) { issue(s0); mma(s1); }
        if (g + 2 < a.kgs) { issue(s1); mma(s2); }
    }

    // epilogue: z = acc * |rstd| + b; the column sums of (z - shift) over this slab's rows, registers in ascending order,
    // then half 0 + half 1
    float rs[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned m = min(m_base + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, a.n - 1);
            rs[mt][r] = __builtin_fabsf(a.stats[m].y);
        }
    float* part = a.partial + (size_t)blockIdx.x * 2 * a.c_out;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        if (nt0 + nt >= ntiles) continue;
        const int n = (nt0 + nt) * 32 + i;
        const float bo = a.bias[n], sh = a.shift[n];
        float s = 0.0f, q = 0.0f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned m = m_base + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m >= a.n) continue;
                const float v = acc[mt][nt][r] * rs[mt][r] + bo;
                a.z[(size_t)m * a.c_out + n] = v;
                const float d = v - sh;
                s = s + d;
                q = q + d * d;
            }
        s = s + lane_xor_f32<32>(s, lane);
        q = q + lane_xor_f32<32>(q, lane);
        if (half == 0) part[n] = s;
        else part[a.c_out + n] = q;
    }
}

// shift[o] = the mean of column o of z over its first k = min(n, PT_SHIFT_ROWS) rows: the value the column sums are taken
// around.  bn_finalize_kernel takes any shift; the closer it is to the column mean, the less var = q / n - (s / n)^2
// cancels.  Around row 0 alone some column of 256 lies 3 sigma off, and the fp32 rounding of s and q of a single slab
// came to 9e-7 of invstd at 65 rows, 6 x the stock error; around the mean of eight rows it lies about 0.35 sigma off - if
// the eight rows are typical.  Where they are not (eight rows of tissue in front of a slide of near-identical background:
// sqrt(n / 8) sigma off, invstd to 2.7e-5) bn_finalize_kernel notices - a shift more than 2 sigma from the mean it led to
// - and sums those columns of z again in fp64 (csrc/bn_train.hip; tests/test_bn_train_conditioning.py).
// One wavefront per column, the lanes split F (coalesced reads of the row of W).
constexpr int PT_SHIFT_ROWS = 8;

template <typename T, bool INDEXED>
__global__ __launch_bounds__(256) void projector_train_shift_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, const float2* __restrict__ stats, int k,
                                                                    int c_in, int c_out, float* __restrict__ shift,
                                                                    const int32_t* __restrict__ index, unsigned src_rows) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (o >= c_out) return;                                         // wave-uniform; no barrier below
    float mean[PT_SHIFT_ROWS], acc[PT_SHIFT_ROWS];
    const T* xr[PT_SHIFT_ROWS];
#pragma unroll
    for (int u = 0; u < PT_SHIFT_ROWS; ++u) {                       // (a row that is not there repeats the last one; not added)
        const int r = min(u, k - 1);
        mean[u] = stats[r].x;
        xr[u] = x + (size_t)(INDEXED ? pt_src_row(index[r], src_rows) : (unsigned)r) * c_in;
        acc[u] = 0.0f;
    }
    const float* wr = w + (size_t)o * c_in;
    for (int f = lane; f < c_in; f += 64) {
        const float wv = wr[f];
#pragma unroll
        for (int u = 0; u < PT_SHIFT_ROWS; ++u) acc[u] = __builtin_fmaf((float)xr[u][f] - mean[u], wv, acc[u]);
    }
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < PT_SHIFT_ROWS; ++u)
        if (u < k) s = s + acc[u] * __builtin_fabsf(stats[u].y);
    s = s + lane_xor_f32<32>(s, lane); s = s + lane_xor_f32<16>(s, lane); s = s + lane_xor_f32<8>(s, lane);
    s = s + lane_xor_f32<4>(s, lane); s = s + lane_xor_f32<2>(s, lane); s = s + lane_xor_f32<1>(s, lane);
    if (lane == 0) shift[o] = s / (float)k + bias[o];
}

// ------------------------------------------------------------------ weight gradient
// conv_wgrad_kernel for a 1x1 map with the statistics applied in registers: a lane's A value is dz[row][o0 + i] * |rstd_row|,
// its B value x[row][f0 + i] - mean_row, 128 (typed: 64) contiguous bytes per half-wave and operand; the two halves of a
// wavefront hold the two rows of an MFMA.  The wavefronts of a workgroup do NOT split the rows (conv_wgrad_kernel: nothing
// shared, every MFMA needs 256 B of fresh operands from L2): the eight of them walk the SAME rows, each for its own 64 x 64
// block of a 128 (o) x 256 (f) region of dW - the layout of conv_wgrad_taps_kernel -, so a dz line serves four wavefronts and
// an x line two out of the compute unit's L1, and there is no block to add through LDS.
// The row axis is cut into chunks of PW_CHUNK rows, one workgroup per (region, chunk); the chunks' partial blocks are added
// in chunk order by projector_wgrad_reduce_kernel - onto what dW holds when the call continues an earlier slice of the
// same rows.  The chunk is a constant, so the tree of additions depends on a row's position alone: the same bits however
// many rows, compute units or slices (multiples of PW_CHUNK rows) there are.
constexpr int PW_CHUNK = 4096;
constexpr int PW_WAVES = 8, PW_BO = 128, PW_BF = 256;

struct PtWgArgs {
    const void* x;             // (n, f) as T
    const float* dz;           // (n, d)
    const float2* stats;       // n x (mean, +-rstd)
    float* partial;            // [chunks][d * f + d]: dW blocks, then db
    long long n;
    int f, d;
    int f_regions, regions;    // regions = o_regions * f_regions
    const int32_t* index;      // INDEXED: the source row of every row of dz / stats (x: the whole source, x_bytes its size)
    unsigned src_rows, x_bytes;
};

struct PtWgStage {
    float a0, a1, b0, b1;
    float2 st;
    int32_t ix;                // INDEXED: the index entry of the row this slot loads NEXT (requested one ring turn ahead)
};

template <typename T, bool INDEXED>
__global__ __launch_bounds__(PW_WAVES * 64) void projector_wgrad_kernel(PtWgArgs a) {
    const int lane = threadIdx.x & 63, half = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int region = (int)(blockIdx.x % (unsigned)a.regions), chunk = (int)(blockIdx.x / (unsigned)a.regions);
    const int fr = region % a.f_regions, orr = region / a.f_regions;
    const int o0 = orr * PW_BO + (wave >> 2) * 64, f0 = fr * PW_BF + (wave & 3) * 64;
    if (o0 >= a.d || f0 >= a.f) return;                              // wave-uniform; no barrier below
    const long long row_lo = (long long)chunk * PW_CHUNK;
    const long long left = a.n - row_lo;
    const unsigned rows = (unsigned)(left < PW_CHUNK ? left : PW_CHUNK);
    // the chunk's rows as buffers of their own: what lies beyond them - the next chunk's rows - reads as zeros
    // (INDEXED: x is the whole source, a row's base comes from the index, itself a buffer bounded to the chunk)
    const __amdgpu_buffer_rsrc_t rx = INDEXED
        ? __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000)
        : __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(static_cast<const T*>(a.x) + (size_t)row_lo * a.f), 0, (int)(rows * (unsigned)a.f * (unsigned)sizeof(T)), 0x00020000);
    __amdgpu_buffer_rsrc_t ri = rx;                                  // (the plain kernel has no index: never read there)
    if constexpr (INDEXED) ri = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(a.index + row_lo), 0, (int)(rows * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dz + (size_t)row_lo * a.d), 0,
                                                                        (int)(rows * (unsigned)a.d * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(a.stats + row_lo), 0, (int)(rows * 8u), 0x00020000);
    const unsigned ystride = 2u * (unsigned)a.d * 4u, xstride = 2u * (unsigned)a.f * (unsigned)sizeof(T);      // bytes per row pair
    const unsigned vy0 = ((unsigned)half * (unsigned)a.d + (unsigned)(o0 + i)) * 4u;
    const unsigned vy1 = o0 + 32 + i < a.d ? vy0 + 128u : kPtOob;                                              // (D = 32: no second tile)
    const unsigned vx0 = ((unsigned)half * (unsigned)a.f + (unsigned)(f0 + i)) * (unsigned)sizeof(T);
    const unsigned vx1 = f0 + 32 + i < a.f ? vx0 + 32u * (unsigned)sizeof(T) : kPtOob;
    const unsigned vs = (unsigned)half * 8u;
    unsigned soffy = 0u, soffx = 0u, soffs = 0u;

    pt_f32x16 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.0f;
    // sum of dz over this lane's rows (the wavefronts at f0 = 0 store it): one chain per slot of the operand ring - four
    // chains of a quarter of the length round less than one, at the same instruction count
    float db0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, db1[4] = {0.0f, 0.0f, 0.0f, 0.0f};

    // INDEXED: this lane's row of the pair being issued (its half's), and where the index of the pair one ring turn on lies
    unsigned prow = (unsigned)half, soffi = 0u;
    const unsigned vi = (unsigned)half * 4u, xrow = (unsigned)a.f * (unsigned)sizeof(T);
    const unsigned cx0 = (unsigned)(f0 + i) * (unsigned)sizeof(T), cx1 = cx0 + 32u * (unsigned)sizeof(T);
    const unsigned out1 = f0 + 32 + i < a.f ? 0u : kPtOob;
    auto issue = [&](PtWgStage& s) {
        s.a0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, (int)vy0, (int)soffy, 0));
        s.a1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, (int)vy1, (int)soffy, 0));
        if constexpr (INDEXED) {
            // a row beyond the chunk must read zeros as it does in the plain kernel: its index entry reads as 0, which is
            // a real source row (0 * NaN is not 0), so the lane goes to the out-of-range offset instead
            // (the source is below 2 GiB: OR-ing the marker's bit in is the select, and stays straight-line code)
            const unsigned out = prow < rows ? 0u : kPtOob;
            const unsigned base = pt_src_row(s.ix, a.src_rows) * xrow;
            s.b0 = pt_load1<T>(rx, (base + cx0) | out, 0u);
            s.b1 = pt_load1<T>(rx, (base + cx1) | out | out1, 0u);
            s.ix = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)vi, (int)(soffi + 32u), 0);      // (4 pairs x 8 bytes on)
            prow += 2u;
            soffi += 8u;
        } else {
            s.b0 = pt_load1<T>(rx, vx0, soffx);
            s.b1 = pt_load1<T>(rx, vx1, soffx);
        }
        const pt_u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)vs, (int)soffs, 0);
        s.st = make_float2(__uint_as_float(u[0]), __uint_as_float(u[1]));
        soffy += ystride;
        soffx += xstride;
        soffs += 16u;
    };
    // (a row pair beyond the chunk: every load returns zero - 0 * 0 into the accumulators, + 0 into db)
    auto mma = [&](const PtWgStage& s, int slot) {
        const float r = __builtin_fabsf(s.st.y);
        const float a0 = s.a0 * r, a1 = s.a1 * r, b0 = s.b0 - s.st.x, b1 = s.b1 - s.st.x;
        db0[slot] = db0[slot] + s.a0;
        db1[slot] = db1[slot] + s.a1;
        acc[0][0] = PT_MFMA(a0, b0, acc[0][0]);
        acc[0][1] = PT_MFMA(a0, b1, acc[0][1]);
        acc[1][0] = PT_MFMA(a1, b0, acc[1][0]);
        acc[1][1] = PT_MFMA(a1, b1, acc[1][1]);
    };
    const int steps = (int)((rows + 1u) >> 1);
    PtWgStage s0, s1, s2, s3;
    if constexpr (INDEXED) {                                        // the first ring turn's index entries
        s0.ix = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)vi, 0, 0);
        s1.ix = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)vi, 8, 0);
        s2.ix = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)vi, 16, 0);
        s3.ix = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ri, (int)vi, 24, 0);
    }
    issue(s0);
    issue(s1);
    issue(s2);
#pragma unroll 1
    for (int t = 0; t < steps; t += 4) {
        issue(s3); mma(s0, 0);
        issue(s0); mma(s1, 1);
        issue(s1); mma(s2, 2);
        issue(s2); mma(s3, 3);
    }
    // (x of a lane whose column lies beyond F read zeros, but zero minus the mean is not zero: those columns are not stored)
    float* out = a.partial + (size_t)chunk * ((size_t)a.d * a.f + a.d);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int col = f0 + 32 * v + i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = o0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < a.d && col < a.f) out[(size_t)row * a.f + col] = acc[u][v][r];
            }
        }
    if (f0 == 0) {
        float t0 = (db0[0] + db0[1]) + (db0[2] + db0[3]), t1 = (db1[0] + db1[1]) + (db1[2] + db1[3]);
        t0 = t0 + lane_xor_f32<32>(t0, lane);
        t1 = t1 + lane_xor_f32<32>(t1, lane);
        float* dbo = out + (size_t)a.d * a.f;
        if (half == 0) dbo[o0 + i] = t0;
        else if (o0 + 32 + i < a.d) dbo[o0 + 32 + i] = t1;
    }
}

// dw | db (total = d * f + d elements, db behind dw in the partial blocks) = [dw | db +] the chunks in ascending order
__global__ void projector_wgrad_reduce_kernel(const float* __restrict__ partial, int chunks, size_t total, size_t dw_elems,
                                              float* __restrict__ dw, float* __restrict__ db, int accumulate) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    float* dst = e < dw_elems ? dw + e : db + (e - dw_elems);
    float s = partial[e];
    if (accumulate) s = *dst + s;
    int k = 1;
    for (; k + 8 <= chunks; k += 8) {              // chunk order kept; eight loads in flight
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = partial[(size_t)(k + j) * total + e];
#pragma unroll
        for (int j = 0; j < 8; ++j) s = s + v[j];
    }
    for (; k < chunks; ++k) s = s + partial[(size_t)k * total + e];
    *dst = s;
}

static bool pt_shape(int f, int d) {
    // F: whole k-groups of the packed weights and whole 32-column tiles of dW; D: whole 32-column tiles, and what the
    // BatchNorm kernels behind z take (D / 4 a power of two <= 256: ipsx_bn_train_supported)
    if (f < 32 || f % 32 != 0 || d < 32 || d > 1024 || (d & (d - 1)) != 0) return false;
    return cdiv(d, 32) * (int64_t)(f / 8) * 1024 < ((int64_t)1 << 31);
}

// rows of one launch: activations below 2 GiB (32-bit buffer offsets + the out-of-range marker), whole units of `unit` rows
static int64_t pt_rows_per_launch(int f, int d, int esize, int64_t unit) {
    const int64_t row_bytes = std::max<int64_t>((int64_t)f * esize, (int64_t)d * 4);
    const int64_t per = ((((int64_t)1 << 31) - 65536) / row_bytes) / unit * unit;
    return std::max<int64_t>(per, unit);
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_projector_train_supported(int f, int d) { return pt_shape(f, d) ? 1 : 0; }

IPSX_API int64_t ipsx_projector_train_slabs(int64_t n) { return n > 0 ? cdiv(n, 64) : 0; }

// a source the INDEXED kernels address with 32-bit buffer offsets: below 2 GiB (less the margin of pt_rows_per_launch)
static bool pt_source_fits(int64_t src_rows, int f, int esize) {
    return src_rows > 0 && src_rows < ((int64_t)1 << 31) && src_rows * f * esize <= ((int64_t)1 << 31) - 65536;
}

template <typename T, bool INDEXED>
static void pt_launch_shift(const void* x, const float* weight, const ipsx_conv* lin, const float2* st2, int k, float* shift, const int32_t* index,
                            int64_t src_rows, hipStream_t s) {
    projector_train_shift_kernel<T, INDEXED><<<dim3((unsigned)cdiv(lin->c_out, 4)), dim3(256), 0, s>>>(
        static_cast<const T*>(x), weight, lin->shift, st2, k, lin->c_in, lin->c_out, shift, index, (unsigned)src_rows);
}

template <typename T, bool INDEXED>
static void pt_launch_fwd(const PtFwdArgs& a, hipStream_t s) {
    const unsigned mt = (unsigned)cdiv((int64_t)a.n, 64);
    if (a.c_out >= 512) projector_train_fwd_kernel<T, 4, INDEXED><<<dim3(mt, (unsigned)cdiv(a.c_out, 512)), dim3(256), 0, s>>>(a);
    else projector_train_fwd_kernel<T, 2, INDEXED><<<dim3(mt, (unsigned)cdiv(a.c_out, 256)), dim3(256), 0, s>>>(a);
}

// FN<T, INDEXED>(...) for the call's dtype and index
#define PT_DISPATCH(FN, ...)                                    \
    do {                                                        \
        if (index) {                                            \
            if (dtype == 0) FN<float, true>(__VA_ARGS__);       \
            else if (dtype == 1) FN<__bf16, true>(__VA_ARGS__); \
            else FN<_Float16, true>(__VA_ARGS__);               \
        } else {                                                \
            if (dtype == 0) FN<float, false>(__VA_ARGS__);      \
            else if (dtype == 1) FN<__bf16, false>(__VA_ARGS__);\
            else FN<_Float16, false>(__VA_ARGS__);              \
        }                                                       \
    } while (0)

// the one host path of ipsx_projector_train_forward (index NULL) and ipsx_projector_train_forward_indexed
static int pt_forward(const char* what, const ipsx_conv* lin, const float* weight, const void* x, int dtype, const int32_t* index,
                      int64_t src_rows, int64_t n, const float* stats, float* z, float* shift, float* partial, void* stream) {
    IPSX_REQUIRE(lin && lin->w_packed && lin->shift && weight && x && stats && z && shift && partial && n > 0, "%s: bad arguments", what);
    IPSX_REQUIRE(lin->kh == 1 && lin->kw == 1 && lin->stride == 1 && lin->pad == 0 && !lin->alpha,
                 "%s: lin is a Linear with its bias in `shift` and no affine", what);
    IPSX_REQUIRE(dtype >= 0 && dtype <= 2, "%s: dtype %d (0 float32, 1 bfloat16, 2 float16)", what, dtype);
    const int f = lin->c_in, d = lin->c_out;
    IPSX_REQUIRE(pt_shape(f, d), "%s: F = %d (a multiple of 32), D = %d (a power of two, 32 .. 1024)", what, f, d);
    const int esize = dtype == 0 ? 4 : 2;
    IPSX_REQUIRE(!index || pt_source_fits(src_rows, f, esize),
                 "%s: a source of %lld rows is not below 2 GiB (32-bit buffer offsets): gather the rows and take the plain call", what,
                 (long long)src_rows);
    hipStream_t s = as_stream(stream);
    const float2* st2 = reinterpret_cast<const float2*>(stats);
    const int k = (int)std::min<int64_t>(n, PT_SHIFT_ROWS);
    PT_DISPATCH(pt_launch_shift, x, weight, lin, st2, k, shift, index, src_rows, s);
    IPSX_TRY(launched(what));
    // (packed rows per launch: z below 2 GiB, and the plain call's x)
    const int64_t per = pt_rows_per_launch(f, d, esize, 64);
    for (int64_t i0 = 0; i0 < n; i0 += per) {
        const int64_t cnt = std::min(per, n - i0);
        PtFwdArgs a;
        a.x = index ? x : static_cast<const char*>(x) + (size_t)i0 * f * esize;
        a.wp = lin->w_packed; a.bias = lin->shift; a.stats = st2 + i0; a.shift = shift;
        a.z = z + (size_t)i0 * d;
        a.partial = partial + (size_t)(i0 / 64) * 2 * d;
        a.index = index ? index + i0 : nullptr;
        a.src_rows = index ? (unsigned)src_rows : 0u;
        a.n = (unsigned)cnt;
        a.x_bytes = (unsigned)((index ? src_rows : cnt) * f * esize);
        a.w_bytes = (unsigned)(cdiv(d, 32) * (int64_t)(f / 8) * 1024);
        a.c_in = f; a.c_out = d; a.kgs = f / 8;
        PT_DISPATCH(pt_launch_fwd, a, s);
        IPSX_TRY(launched(what));
    }
    return IPSX_OK;
}

IPSX_API int ipsx_projector_train_forward(const ipsx_conv* lin, const float* weight, const void* x, int dtype, int64_t n,
                                          const float* stats, float* z, float* shift, float* partial, void* stream) {
    return pt_forward("projector_train_forward", lin, weight, x, dtype, nullptr, 0, n, stats, z, shift, partial, stream);
}

IPSX_API int ipsx_projector_train_forward_indexed(const ipsx_conv* lin, const float* weight, const void* x, int dtype, const int32_t* index,
                                                  int64_t src_rows, int64_t n, const float* stats, float* z, float* shift, float* partial,
                                                  void* stream) {
    IPSX_REQUIRE(index, "projector_train_forward_indexed: bad arguments");
    return pt_forward("projector_train_forward_indexed", lin, weight, x, dtype, index, src_rows, n, stats, z, shift, partial, stream);
}

IPSX_API int64_t ipsx_projector_wgrad_chunk_rows(void) { return PW_CHUNK; }

IPSX_API int64_t ipsx_projector_wgrad_max_rows(int f, int d, int dtype) {
    if (!pt_shape(f, d) || dtype < 0 || dtype > 2) return 0;
    return pt_rows_per_launch(f, d, dtype == 0 ? 4 : 2, PW_CHUNK);
}

IPSX_API size_t ipsx_projector_wgrad_workspace_bytes(int64_t n, int f, int d) {
    if (n <= 0 || !pt_shape(f, d)) return 0;
    return (size_t)cdiv(n, PW_CHUNK) * ((size_t)d * f + d) * sizeof(float);
}

template <typename T, bool INDEXED>
static void pt_launch_wgrad(const PtWgArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    projector_wgrad_kernel<T, INDEXED><<<grid, block, 0, s>>>(a);
}

// the one host path of ipsx_projector_wgrad (index NULL) and ipsx_projector_wgrad_indexed
static int pt_wgrad(const char* what, const void* x, int dtype, const int32_t* index, int64_t src_rows, const float* dz, const float* stats,
                    int64_t n, int f, int d, float* dw, float* db, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(x && dz && stats && dw && db && n > 0, "%s: bad arguments", what);
    IPSX_REQUIRE(dtype >= 0 && dtype <= 2, "%s: dtype %d (0 float32, 1 bfloat16, 2 float16)", what, dtype);
    IPSX_REQUIRE(pt_shape(f, d), "%s: F = %d (a multiple of 32), D = %d (a power of two, 32 .. 1024)", what, f, d);
    IPSX_REQUIRE(n <= ipsx_projector_wgrad_max_rows(f, d, dtype),
                 "%s: %lld rows exceed one 2 GiB buffer - call per slice of whole chunks (ipsx_projector_wgrad_max_rows) with "
                 "accumulate = 1", what, (long long)n);
    const int esize = dtype == 0 ? 4 : 2;
    IPSX_REQUIRE(!index || pt_source_fits(src_rows, f, esize),
                 "%s: a source of %lld rows is not below 2 GiB (32-bit buffer offsets): gather the rows and take the plain call", what,
                 (long long)src_rows);
    const size_t need = ipsx_projector_wgrad_workspace_bytes(n, f, d);
    if (!workspace || workspace_bytes < need) return fail(IPSX_EWORKSPACE, "%s: workspace %zu B < %zu B", what, workspace_bytes, need);
    PtWgArgs a;
    a.x = x; a.dz = dz; a.stats = reinterpret_cast<const float2*>(stats); a.partial = static_cast<float*>(workspace);
    a.n = n; a.f = f; a.d = d;
    a.f_regions = (int)cdiv(f, PW_BF);
    a.regions = a.f_regions * (int)cdiv(d, PW_BO);
    a.index = index;
    a.src_rows = index ? (unsigned)src_rows : 0u;
    a.x_bytes = index ? (unsigned)(src_rows * f * esize) : 0u;
    const int chunks = (int)cdiv(n, PW_CHUNK);
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)(a.regions * chunks)), block(PW_WAVES * 64);
    PT_DISPATCH(pt_launch_wgrad, a, grid, block, s);
    IPSX_TRY(launched(what));
    const size_t dw_elems = (size_t)d * f, total = dw_elems + d;
    projector_wgrad_reduce_kernel<<<dim3((unsigned)cdiv((int64_t)total, 256)), dim3(256), 0, s>>>(a.partial, chunks, total, dw_elems, dw, db,
                                                                                                  accumulate ? 1 : 0);
    return launched(what);
}

IPSX_API int ipsx_projector_wgrad(const void* x, int dtype, const float* dz, const float* stats, int64_t n, int f, int d, float* dw,
                                  float* db, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    return pt_wgrad("projector_wgrad", x, dtype, nullptr, 0, dz, stats, n, f, d, dw, db, accumulate, workspace, workspace_bytes, stream);
}

IPSX_API int ipsx_projector_wgrad_indexed(const void* x, int dtype, const int32_t* index, int64_t src_rows, const float* dz,
                                          const float* stats, int64_t n, int f, int d, float* dw, float* db, int accumulate, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(index, "projector_wgrad_indexed: bad arguments");
    return pt_wgrad("projector_wgrad_indexed", x, dtype, index, src_rows, dz, stats, n, f, d, dw, db, accumulate, workspace, workspace_bytes,
                    stream);
}
