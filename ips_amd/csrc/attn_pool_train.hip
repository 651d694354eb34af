// attn_pool_train.hip - the cross-attention aggregator of the TRAINING step on folded queries (reference
// architecture/transformer.py:43-109 under autograd).  With the scaled query folded into k_w (A, R = H * n_token rows of D)
// and v_w applied AFTER the softmax-weighted sum, the only part of the node that touches the (B, M, D) embeddings is
//
//     L[b, m, r] = x[b, m, :] . A[r, :]      P[b, r, :] = softmax_m L[b, :, r]      P' = P * keep
//     Z[b, r, :] = sum_m P'[b, r, m] x[b, m, :]
//
// and its backward, with c[b, r] = dZ[b, r, :] . Z[b, r, :] ( = sum_m P' dP': the softmax-backward row constant needs no pass)
//
//     dP'[b, r, m] = dZ[b, r, :] . x[b, m, :]           dL = P * (keep * dP' - c)
//     dx[b, m, :]  = sum_r P'[b, r, m] dZ[b, r, :] + sum_r dL[b, m, r] A[r, :]
//     dA[r, :]     = sum_b sum_m dL[b, m, r] x[b, m, :]
//
// K and V (B x M x H x D_k each) never exist.  All contractions run on v_mfma_f32_32x32x2_f32 with R padded to the 32
// columns of a tile:
//   - over D (x . A, x . dZ): a wavefront takes 32 rows of x, a lane four consecutive d per 16-byte load, the two halves of
//     the wavefront the two k of an MFMA; the result has r on the lane and m in the registers;
//   - over M (P' . x, dL . x): the weights go through LDS as [m][r] (row pitch 33: conflict-free either way), the wavefront
//     owns 128 columns of D, a lane four consecutive d per load (output column i of MFMA j is d = base + 4 i + j);
//   - over r (dx, rank 2R): the same LDS image read along r, dZ[b] and A as the B operand.
// Forward: logits kernel (x read), one workgroup per (b, r) row for the softmax, pool kernel (x read again).  Backward: c,
// then ONE kernel per (b, 128 rows): x . dZ, then dA's block and dx from the same rows (the second and third walk hit the cache), dx
// written once.  Z and dA are sums over workgroups: every workgroup stores its block, attn_pool_sum_kernel adds the blocks
// in ascending (b, chunk) order - no float atomics, the same bits every run, and an image's Z / P / dx do not depend on
// what else is in the batch (the chunk is a constant: the tree of additions depends on M alone).
//
// COUNTED (the _counted exports, a zero-padded batch): image b's row bound is count[b] (device int32, clamped into 1 .. M)
// where it is M above; the row pitch stays M.  The mask is that bound and nothing else - no row at or beyond count[b] is
// read, so whatever the padding holds cannot reach an output - and since the trees depend on the row count alone, Z[b],
// P[b, :, :count[b]] and dx[b, :count[b]] have the bits of the unmasked kernels on x[b, :count[b]].  A workgroup whose
// chunk starts at or beyond count[b] does no arithmetic: it stores a zero block (attn_pool_sum_kernel is unchanged; a
// trailing +0.0 can only turn a -0.0 sum into +0.0) and, in the backward, zeros into its rows of dx.

#include "ipsx_common.h"
#include "ipsx_math.h"

namespace ipsx {

typedef float ap_f32x16 __attribute__((ext_vector_type(16)));
typedef float ap_f32x4 __attribute__((ext_vector_type(4)));

#define AP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int AP_CHUNK = 128;          // rows of x per workgroup: 4 wavefronts x 32
constexpr int AP_PITCH = 33;           // floats per [m] row of the LDS images
constexpr int AP_MAX_R = 32, AP_MAX_D = 1024;

// the row bound of image b
template <bool COUNTED>
__device__ __forceinline__ int ap_rows(const int32_t* __restrict__ count, int b, int M) {
    if constexpr (COUNTED) return min(max(count[b], 1), M);
    else return M;
}

// row of accumulator register q in lane half h (the 32x32 C/D map)
__device__ __forceinline__ int ap_row(int q, int half) { return (q & 3) + 8 * (q >> 2) + 4 * half; }

// acc[m][r] = sum_d x[m0 + m, d] * w[r, d] for the 32 rows from m0 (rows beyond `rows` repeat the last one: their results
// are not used), r < R (the others: zero operand).  xb: this image's rows; w: (R, D).
__device__ __forceinline__ ap_f32x16 ap_dot_tile(const float* __restrict__ xb, const float* __restrict__ w, int m0, int rows, int R,
                                                 int D, int lane) {
    const int half = lane >> 5, i = lane & 31;
    const float* xr = xb + (size_t)min(m0 + i, rows - 1) * D + 4 * half;
    const float* wr = w + (size_t)min(i, R - 1) * D + 4 * half;
    const bool wok = i < R;
    // eight chains - the 8-group u of a trip, the parity of j - added as a tree at the end: an eighth of the length per chain
    // (a single chain over D = 512 rounds 3 - 4 x worse than a blocked GEMM does), and no MFMA waits for the one before it
    ap_f32x16 acc[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[u][v][q] = 0.0f;
#pragma unroll 1
    for (int g0 = 0; g0 < D; g0 += 32) {           // (D is a multiple of 32: four loads of either operand in flight)
        ap_f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *reinterpret_cast<const ap_f32x4*>(xr + g0 + 8 * u);
            b[u] = *reinterpret_cast<const ap_f32x4*>(wr + g0 + 8 * u);
            if (!wok) b[u] = ap_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u][j & 1] = AP_MFMA(a[u][j], b[u][j], acc[u][j & 1]);
    }
    return ((acc[0][0] + acc[0][1]) + (acc[1][0] + acc[1][1])) + ((acc[2][0] + acc[2][1]) + (acc[3][0] + acc[3][1]));
}

// acc[g][j][r][i] += sum_m wl[m][r] * x[m0 + m, (wave + 4 g) * 128 + 4 i + j] over the chunk's rows: the wavefront's
// column groups.  wl: LDS image [m][AP_PITCH], zero for m beyond the chunk's rows and r >= R.
template <int GPW>
__device__ __forceinline__ void ap_pool_chunk(const float* __restrict__ xb, const float* wl, int m0, int nrows, int rows, int D, int wave,
                                              int lane, ap_f32x16 (&acc)[GPW][4]) {
    const int half = lane >> 5, i = lane & 31;
    int col[GPW];
    bool ok[GPW];
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
        col[g] = (wave + 4 * g) * 128 + 4 * i;
        ok[g] = col[g] < D;
    }
    // four row pairs per trip (the image's zero rows pad the last one; AP_CHUNK is a multiple of 8): their loads in flight
    const int steps = ((nrows + 7) >> 3) << 2;
    // two chains, alternate row pairs (a chain of 128 equal terms drifts past 1e-6 of the sum; half of it does not)
    ap_f32x16 odd[GPW][4];
#pragma unroll
    for (int g = 0; g < GPW; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) odd[g][j][q] = 0.0f;
#pragma unroll 1
    for (int k0 = 0; k0 < steps; k0 += 4) {
        float a[4];
        ap_f32x4 b[4][GPW];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ml = 2 * (k0 + u) + half;
            a[u] = wl[ml * AP_PITCH + i];
            const float* xr = xb + (size_t)min(m0 + ml, rows - 1) * D;
#pragma unroll
            for (int g = 0; g < GPW; ++g) {
                b[u][g] = ap_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (ok[g]) b[u][g] = *reinterpret_cast<const ap_f32x4*>(xr + col[g]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int g = 0; g < GPW; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (u & 1) odd[g][j] = AP_MFMA(a[u], b[u][g][j], odd[g][j]);
                    else acc[g][j] = AP_MFMA(a[u], b[u][g][j], acc[g][j]);
                }
    }
#pragma unroll
    for (int g = 0; g < GPW; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[g][j] = acc[g][j] + odd[g][j];
}

// the block of (R, D) a wavefront holds after ap_pool_chunk -> out[r][d]
template <int GPW>
__device__ __forceinline__ void ap_store_block(float* __restrict__ out, const ap_f32x16 (&acc)[GPW][4], int R, int D, int wave, int lane) {
    const int half = lane >> 5, i = lane & 31;
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
        const int col = (wave + 4 * g) * 128 + 4 * i;
        if (col >= D) continue;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = ap_row(q, half);
            if (r < R) *reinterpret_cast<ap_f32x4*>(out + (size_t)r * D + col) = ap_f32x4{acc[g][0][q], acc[g][1][q], acc[g][2][q], acc[g][3][q]};
        }
    }
}

// a block of zeros in its place: a workgroup whose chunk lies beyond the image's rows (COUNTED)
template <int GPW>
__device__ __forceinline__ void ap_store_zero_block(float* __restrict__ out, int R, int D, int wave, int lane) {
    ap_f32x16 acc[GPW][4];
#pragma unroll
    for (int g = 0; g < GPW; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[g][j][q] = 0.0f;
    ap_store_block<GPW>(out, acc, R, D, wave, lane);
}

// dx[ml, :] = 0 for the chunk's rows ml = from .. to - 1 (COUNTED: the rows beyond the image's count), the wavefront's columns
template <int GPW>
__device__ __forceinline__ void ap_zero_dx_rows(float* __restrict__ dxb, int from, int to, int D, int wave, int lane) {
    const int half = lane >> 5, i = lane & 31;
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
        const int col = (wave + 4 * g) * 128 + 4 * i;
        if (col >= D) continue;
        for (int ml = from + half; ml < to; ml += 2) *reinterpret_cast<ap_f32x4*>(dxb + (size_t)ml * D + col) = ap_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// ------------------------------------------------------------------ forward 1: raw logits into P
template <bool COUNTED>
__global__ __launch_bounds__(256) void attn_pool_logits_kernel(const float* __restrict__ x, const float* __restrict__ A, float* __restrict__ P,
                                                               const int32_t* __restrict__ count, int M, int R, int D) {
    const int lane = threadIdx.x & 63, half = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, m0 = blockIdx.x * AP_CHUNK + wave * 32;
    const int rows = ap_rows<COUNTED>(count, b, M);
    if (m0 >= rows) return;                                         // wave-uniform; no barrier below
    const float* xb = x + (size_t)b * M * D;
    const ap_f32x16 acc = ap_dot_tile(xb, A, m0, rows, R, D, lane);
    if (i >= R) return;
    float* pr = P + ((size_t)b * R + i) * M;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int m = m0 + ap_row(q, half);
        if (m < rows) pr[m] = acc[q];
    }
}

// ------------------------------------------------------------------ forward 2: P[b, r, :] = softmax of its logits, in place
// One workgroup per row; maximum and sum through a fixed tree (thread-strided chains, xor butterfly, the four wavefronts
// in order).  COUNTED: over the image's count[b] slots; the slots beyond (which the logits kernel left unwritten) get +0.0.
template <bool COUNTED>
__global__ __launch_bounds__(256) void attn_pool_softmax_kernel(float* __restrict__ P, const int32_t* __restrict__ count, int M, int R) {
    __shared__ float red[4];
    float* row = P + (size_t)blockIdx.x * M;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int rows = ap_rows<COUNTED>(count, (int)(blockIdx.x / (unsigned)R), M);
    float mx = -INFINITY;
    for (int m = t; m < rows; m += 256) mx = nanmax(mx, row[m]);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
    __syncthreads();
    float s = 0.0f;
    for (int m = t; m < rows; m += 256) {
        const float e = expf(row[m] - mx);
        row[m] = e;
        s = s + e;
    }
    s = s + lane_xor_f32<32>(s, lane); s = s + lane_xor_f32<16>(s, lane); s = s + lane_xor_f32<8>(s, lane);
    s = s + lane_xor_f32<4>(s, lane); s = s + lane_xor_f32<2>(s, lane); s = s + lane_xor_f32<1>(s, lane);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    for (int m = t; m < rows; m += 256) row[m] = row[m] / s;
    if constexpr (COUNTED)
        for (int m = rows + t; m < M; m += 256) row[m] = 0.0f;
}

// ------------------------------------------------------------------ forward 3: this chunk's block of Z
template <int GPW, bool COUNTED>
__global__ __launch_bounds__(256) void attn_pool_pool_kernel(const float* __restrict__ x, const float* __restrict__ P,
                                                             const float* __restrict__ keep, const int32_t* __restrict__ count,
                                                             float* __restrict__ part, int M, int R, int D, int chunks) {
    __shared__ float wl[AP_CHUNK * AP_PITCH];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, m0 = blockIdx.x * AP_CHUNK;
    const int rows = ap_rows<COUNTED>(count, b, M);
    const int nrows = min(AP_CHUNK, rows - m0);
    if constexpr (COUNTED) {
        if (nrows <= 0) {                                           // (the whole workgroup: no barrier is skipped by a part of it)
            if (wave * 128 < D) ap_store_zero_block<GPW>(part + ((size_t)b * chunks + blockIdx.x) * R * D, R, D, wave, lane);
            return;
        }
    }
    for (int e = threadIdx.x; e < AP_CHUNK * 32; e += 256) {        // e = r * 128 + m: a row of P per 128 threads' loads
        const int r = e >> 7, ml = e & (AP_CHUNK - 1);
        float v = 0.0f;
        if (r < R && ml < nrows) {
            const size_t at = ((size_t)b * R + r) * M + m0 + ml;
            v = P[at];
            if (keep) v = v * keep[at];
        }
        wl[ml * AP_PITCH + r] = v;
    }
    __syncthreads();
    if (wave * 128 >= D) return;                                    // (after the only barrier)
    ap_f32x16 acc[GPW][4];
#pragma unroll
    for (int g = 0; g < GPW; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[g][j][q] = 0.0f;
    ap_pool_chunk<GPW>(x + (size_t)b * M * D, wl, m0, nrows, rows, D, wave, lane, acc);
    ap_store_block<GPW>(part + ((size_t)b * chunks + blockIdx.x) * R * D, acc, R, D, wave, lane);
}

// out[y][e] = part[y][0][e] + part[y][1][e] + ... in ascending order (n blocks of `total` floats per y)
__global__ void attn_pool_sum_kernel(const float* __restrict__ part, int n, int total, float* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const float* p = part + (size_t)blockIdx.y * n * total + e;
    float s = p[0];
    int k = 1;
    for (; k + 8 <= n; k += 8) {                   // order kept; eight loads in flight
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(k + j) * total];
#pragma unroll
        for (int j = 0; j < 8; ++j) s = s + v[j];
    }
    for (; k < n; ++k) s = s + p[(size_t)k * total];
    out[(size_t)blockIdx.y * total + e] = s;
}

// ------------------------------------------------------------------ backward 1: c[b][r] = dZ[b, r, :] . Z[b, r, :]
// The diagonal of Z[b] . dZ[b]^T through the SAME chain as dP' (ap_dot_tile with the rows of Z in the place of x): where a
// row of Z is a row of x - one patch, or all weight on one - dP' - c cancels exactly, as it does in exact arithmetic.
__global__ __launch_bounds__(64) void attn_pool_rowdot_kernel(const float* __restrict__ Z, const float* __restrict__ dZ, float* __restrict__ c,
                                                              int R, int D) {
    const int lane = threadIdx.x, half = lane >> 5, i = lane & 31;
    const size_t at = (size_t)blockIdx.x * R * D;
    const ap_f32x16 acc = ap_dot_tile(Z + at, dZ + at, 0, R, R, D, lane);
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (ap_row(q, half) == i) c[(size_t)blockIdx.x * AP_MAX_R + i] = i < R ? acc[q] : 0.0f;
}

// ------------------------------------------------------------------ backward: dx of this chunk's rows, its block of dA
struct ApBwdArgs {
    const float *x, *A, *keep, *P, *dZ, *c;
    float *dx, *part;          // dx may be null
    int M, R, D, chunks;
    const int32_t* count;      // COUNTED only
};

template <int GPW, bool COUNTED>
__global__ __launch_bounds__(256) void attn_pool_bwd_kernel(ApBwdArgs a) {
    __shared__ float wp[AP_CHUNK * AP_PITCH];      // P'[m][r]
    __shared__ float wd[AP_CHUNK * AP_PITCH];      // dL[m][r]
    const int lane = threadIdx.x & 63, half = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, m0 = blockIdx.x * AP_CHUNK;
    const int M = a.M, R = a.R, D = a.D;
    const int rows = ap_rows<COUNTED>(a.count, b, M);
    const int nrows = min(AP_CHUNK, rows - m0);
    const float* xb = a.x + (size_t)b * M * D;
    const float* dzb = a.dZ + (size_t)b * R * D;
    if constexpr (COUNTED) {
        if (nrows <= 0) {                          // (the whole workgroup, in front of the barrier)
            if (wave * 128 >= D) return;
            ap_store_zero_block<GPW>(a.part + ((size_t)b * a.chunks + blockIdx.x) * R * D, R, D, wave, lane);
            if (a.dx) ap_zero_dx_rows<GPW>(a.dx + ((size_t)b * M + m0) * D, 0, min(AP_CHUNK, M - m0), D, wave, lane);
            return;
        }
    }
    {
        // dP' of this wavefront's 32 rows (a tile beyond M: zeros into the images, no arithmetic)
        const int t0 = wave * 32;
        ap_f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        if (t0 < nrows) acc = ap_dot_tile(xb, dzb, m0 + t0, rows, R, D, lane);
        const float c = a.c[(size_t)b * AP_MAX_R + i];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int ml = t0 + ap_row(q, half);
            float pk = 0.0f, dl = 0.0f;
            if (i < R && ml < nrows) {
                const size_t at = ((size_t)b * R + i) * M + m0 + ml;
                const float p = a.P[at], k = a.keep ? a.keep[at] : 1.0f;
                pk = p * k;
                dl = p * (k * acc[q] - c);
            }
            wp[ml * AP_PITCH + i] = pk;
            wd[ml * AP_PITCH + i] = dl;
        }
    }
    __syncthreads();
    if (wave * 128 >= D) return;                   // (after the last barrier)
    {
        ap_f32x16 acc[GPW][4];
#pragma unroll
        for (int g = 0; g < GPW; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[g][j][q] = 0.0f;
        ap_pool_chunk<GPW>(xb, wd, m0, nrows, rows, D, wave, lane, acc);
        ap_store_block<GPW>(a.part + ((size_t)b * a.chunks + blockIdx.x) * R * D, acc, R, D, wave, lane);
    }
    if (!a.dx) return;
    // dx[m, d] = sum_r P'[m, r] dZ[r, d] + dL[m, r] A[r, d]: 32 rows x 128 columns at a time, k = r in pairs
    const int ksteps = (R + 1) >> 1;
    float* dxb = a.dx + ((size_t)b * M + m0) * D;
    if constexpr (COUNTED) ap_zero_dx_rows<GPW>(dxb, nrows, min(AP_CHUNK, M - m0), D, wave, lane);          // (the chunk straddles count[b])
#pragma unroll 1
    for (int g = 0; g < GPW; ++g) {
        const int col = (wave + 4 * g) * 128 + 4 * i;
        const bool cok = col < D;
#pragma unroll 1
        for (int t0 = 0; t0 < nrows; t0 += 32) {
            ap_f32x16 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[j][q] = 0.0f;
#pragma unroll 1
            for (int kk = 0; kk < ksteps; ++kk) {
                const int r = 2 * kk + half;
                const float a1 = wp[(t0 + i) * AP_PITCH + r], a2 = wd[(t0 + i) * AP_PITCH + r];
                ap_f32x4 b1 = ap_f32x4{0.0f, 0.0f, 0.0f, 0.0f}, b2 = b1;
                if (cok && r < R) {
                    b1 = *reinterpret_cast<const ap_f32x4*>(dzb + (size_t)r * D + col);
                    b2 = *reinterpret_cast<const ap_f32x4*>(a.A + (size_t)r * D + col);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = AP_MFMA(a1, b1[j], acc[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = AP_MFMA(a2, b2[j], acc[j]);
            }
            if (!cok) continue;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int ml = t0 + ap_row(q, half);
                if (ml < nrows) *reinterpret_cast<ap_f32x4*>(dxb + (size_t)ml * D + col) = ap_f32x4{acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
            }
        }
    }
}

static bool ap_shape(int R, int D) { return R >= 1 && R <= AP_MAX_R && D >= 32 && D <= AP_MAX_D && D % 32 == 0; }

static bool ap_sizes(int64_t B, int64_t M) {
    // grid.y = B, grid.x = chunks; a row of P and a chunk index are ints
    return B >= 1 && B <= 65535 && M >= 1 && M <= ((int64_t)1 << 30);
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_attn_pool_supported(int R, int D) { return ap_shape(R, D) ? 1 : 0; }

IPSX_API size_t ipsx_attn_pool_workspace_bytes(int64_t B, int64_t M, int R, int D) {
    if (!ap_shape(R, D) || !ap_sizes(B, M)) return 0;
    // the workgroups' blocks of Z / dA, and the backward's c[b][32]
    return ((size_t)B * (size_t)cdiv(M, AP_CHUNK) * R * D + (size_t)B * AP_MAX_R) * sizeof(float);
}

// the forward and the backward behind their two exports each: count NULL = the unmasked kernels, as before
template <bool COUNTED>
static int ap_forward(const float* x, const float* A, const float* keep, const int32_t* count, int64_t B, int64_t M, int R, int D, float* Z,
                      float* P, void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(x && A && Z && P, "attn_pool_forward: bad arguments");
    IPSX_REQUIRE(ap_shape(R, D), "attn_pool_forward: R = %d (1 .. 32), D = %d (a multiple of 32, 32 .. 1024)", R, D);
    IPSX_REQUIRE(ap_sizes(B, M), "attn_pool_forward: B = %lld (1 .. 65535), M = %lld (1 .. 2^30)", (long long)B, (long long)M);
    const size_t need = ipsx_attn_pool_workspace_bytes(B, M, R, D);
    if (!workspace || workspace_bytes < need) return fail(IPSX_EWORKSPACE, "attn_pool_forward: workspace %zu B < %zu B", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const int chunks = (int)cdiv(M, AP_CHUNK);
    const dim3 grid((unsigned)chunks, (unsigned)B), block(256);
    float* part = static_cast<float*>(workspace);
    attn_pool_logits_kernel<COUNTED><<<grid, block, 0, s>>>(x, A, P, count, (int)M, R, D);
    IPSX_TRY(launched("attn_pool_forward (logits)"));
    attn_pool_softmax_kernel<COUNTED><<<dim3((unsigned)(B * R)), block, 0, s>>>(P, count, (int)M, R);
    IPSX_TRY(launched("attn_pool_forward (softmax)"));
    if (D <= 512) attn_pool_pool_kernel<1, COUNTED><<<grid, block, 0, s>>>(x, P, keep, count, part, (int)M, R, D, chunks);
    else attn_pool_pool_kernel<2, COUNTED><<<grid, block, 0, s>>>(x, P, keep, count, part, (int)M, R, D, chunks);
    IPSX_TRY(launched("attn_pool_forward (pool)"));
    const int total = R * D;
    attn_pool_sum_kernel<<<dim3((unsigned)cdiv(total, 256), (unsigned)B), block, 0, s>>>(part, chunks, total, Z);
    return launched("attn_pool_forward (sum)");
}

template <bool COUNTED>
static int ap_backward(const float* x, const float* A, const float* keep, const int32_t* count, const float* P, const float* Z,
                       const float* dZ, int64_t B, int64_t M, int R, int D, float* dx, float* dA, void* workspace, size_t workspace_bytes,
                       void* stream) {
    IPSX_REQUIRE(x && A && P && Z && dZ && dA, "attn_pool_backward: bad arguments");
    IPSX_REQUIRE(ap_shape(R, D), "attn_pool_backward: R = %d (1 .. 32), D = %d (a multiple of 32, 32 .. 1024)", R, D);
    IPSX_REQUIRE(ap_sizes(B, M), "attn_pool_backward: B = %lld (1 .. 65535), M = %lld (1 .. 2^30)", (long long)B, (long long)M);
    const size_t need = ipsx_attn_pool_workspace_bytes(B, M, R, D);
    if (!workspace || workspace_bytes < need) return fail(IPSX_EWORKSPACE, "attn_pool_backward: workspace %zu B < %zu B", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const int chunks = (int)cdiv(M, AP_CHUNK);
    ApBwdArgs a;
    a.x = x; a.A = A; a.keep = keep; a.P = P; a.dZ = dZ; a.count = count;
    a.dx = dx; a.part = static_cast<float*>(workspace);
    float* c = a.part + (size_t)B * chunks * R * D;
    a.c = c;
    attn_pool_rowdot_kernel<<<dim3((unsigned)B), dim3(64), 0, s>>>(Z, dZ, c, R, D);
    IPSX_TRY(launched("attn_pool_backward (row constants)"));
    a.M = (int)M; a.R = R; a.D = D; a.chunks = chunks;
    const dim3 grid((unsigned)chunks, (unsigned)B), block(256);
    if (D <= 512) attn_pool_bwd_kernel<1, COUNTED><<<grid, block, 0, s>>>(a);
    else attn_pool_bwd_kernel<2, COUNTED><<<grid, block, 0, s>>>(a);
    IPSX_TRY(launched("attn_pool_backward"));
    const int total = R * D;
    const int64_t n = B * chunks;
    IPSX_REQUIRE(n < ((int64_t)1 << 31), "attn_pool_backward: %lld partial blocks", (long long)n);
    attn_pool_sum_kernel<<<dim3((unsigned)cdiv(total, 256), 1), block, 0, s>>>(a.part, (int)n, total, dA);
    return launched("attn_pool_backward (sum)");
}

IPSX_API int ipsx_attn_pool_forward(const float* x, const float* A, const float* keep, int64_t B, int64_t M, int R, int D, float* Z,
                                    float* P, void* workspace, size_t workspace_bytes, void* stream) {
    return ap_forward<false>(x, A, keep, nullptr, B, M, R, D, Z, P, workspace, workspace_bytes, stream);
}

IPSX_API int ipsx_attn_pool_forward_counted(const float* x, const float* A, const float* keep, const int32_t* count, int64_t B, int64_t M,
                                            int R, int D, float* Z, float* P, void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(count, "attn_pool_forward_counted: count is null (ipsx_attn_pool_forward is the unmasked call)");
    return ap_forward<true>(x, A, keep, count, B, M, R, D, Z, P, workspace, workspace_bytes, stream);
}

IPSX_API int ipsx_attn_pool_backward(const float* x, const float* A, const float* keep, const float* P, const float* Z, const float* dZ,
                                     int64_t B, int64_t M, int R, int D, float* dx, float* dA, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return ap_backward<false>(x, A, keep, nullptr, P, Z, dZ, B, M, R, D, dx, dA, workspace, workspace_bytes, stream);
}

IPSX_API int ipsx_attn_pool_backward_counted(const float* x, const float* A, const float* keep, const int32_t* count, const float* P,
                                             const float* Z, const float* dZ, int64_t B, int64_t M, int R, int D, float* dx, float* dA,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(count, "attn_pool_backward_counted: count is null (ipsx_attn_pool_backward is the unmasked call)");
    return ap_backward<true>(x, A, keep, count, P, Z, dZ, B, M, R, D, dx, dA, workspace, workspace_bytes, stream);
}
