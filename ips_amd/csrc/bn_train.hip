// bn_train.hip - training-mode BatchNorm2d fused with the residual add and the ReLU of a ResNet BasicBlock, forward and
// backward, on channels-last activations (rows = patches x pixels, C contiguous).
//
// Reference: training/iterative.py:158-163 runs `net(mem_patch, mem_pos)` with autograd under net.train(), where
// architecture/ips_net.py:273 sends the M selected patches through the ResNet trunk with BatchNorm in batch-statistics
// mode (torchvision BasicBlock: conv - bn - relu - conv - bn - (+identity) - relu).  On stock ROCm ops every bn / add /
// relu is a kernel of its own in both directions (~25 % of the step's device time at the MNIST configuration, more than
// the convolutions); here a BatchNorm with its add and ReLU is two memory passes forward (batch moments; normalise +
// add + ReLU) and two backward (d_gamma / d_beta; dx and the residual's gradient).
//
// Numerics: fp32 like torch.nn.functional.batch_norm, deterministic (every sum in a fixed order).  Sums of d = x - k and
// d^2 in fp32 give var = E[d^2] - E[d]^2 to (1 + E[d]^2 / var) * 2^-24 per rounding: as good as the shift k is near the
// mean, and a shift SAMPLED from the data (row 0, as this file did until the conditioning tests) is 50 sigma off as soon
// as that row is an outlier - invstd came to 2e-4 where the stock kernel gives 1e-7.  What holds now
// (tests/test_bn_train_conditioning.py):
//  * bn_reduce_kernel<false>: every THREAD shifts by the first row it reads itself and hands on (k, sum d, sum d^2) of
//    its 4 .. rows / (512 row lanes) rows; from there on everything is fp64 (the row lanes of a slab, then the slabs, each
//    about the mean of what it combines).  A row that is an outlier spoils the share of the one thread that starts on
//    it: the variance loses at most (rows per thread) * 2^-24 of itself wherever the outliers lie, and what a stock
//    two-pass kernel loses on typical data.
//  * partial sums that come from a producer's epilogue (bn_train_forward_partials: the convolutions, the projector) are
//    around ONE shift per channel, which the producer had to choose before it saw the batch.  bn_finalize_kernel checks
//    it against the mean it finds and sums a channel again, in fp64 over the activation, when the shift was more than
//    BN_RECENTRE sigma^2 off or not finite.
// Results agree with the stock path to fp32 rounding (tests/test_hip_train.py), they are not bit-identical to it (a
// different summation order), which the training path never was across devices.

#include "ipsx_common.h"
#include "ipsx_math.h"

namespace ipsx {

constexpr int BN_MAX_SLABS = 512;

// bn_finalize_kernel<false>: a channel whose one-pass variance is below 1 / (1 + BN_RECENTRE) of its E[d^2] - the shift
// more than sqrt(BN_RECENTRE) = 2 sigma from the mean - is summed again.  (ipsx_rowstats.h draws that line at 4 sigma for
// the LayerNorm's rows, RM_RECENTRE = 17.  Here the sums are longer and the bound asked of invstd is 1e-6: at 4 sigma the
// one-pass form has lost 17 * 2^-24 = 1e-6 per rounding already, at 2 sigma 3e-7.  Every shift a producer passes in a
// running training loop - the previous step's batch mean, the mean of 8 rows of z - lies well inside 2 sigma.)
constexpr double BN_RECENTRE = 4.0;

struct BnShape {
    long long rows;
    int c, cg;           // cg = C / 4 float4 columns (a power of two <= 256)
    int slabs;
    long long slab;      // rows per slab
};

__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__device__ __forceinline__ float f4_at(const float4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

// Two per-channel numbers per slab of rows -> partial[slab][0|1][C].  Threads: (row lane, float4 column); the row lanes
// are combined through LDS in ascending order.
//   BWD = true : sum g, sum g * xhat                 with g = dy (masked by y > 0 under ReLU), xhat = (x - mean) * invstd
//   BWD = false: the slab's moments.  Row lane j sums d = x - k_j and d^2 over its rows j, j + nrl, .. with k_j the FIRST
//                of them; row lane 0 then combines the lanes in fp64: [0] = sum (x - K) over the slab, K = k_0 = the
//                slab's first row (which bn_finalize_slabs_kernel reads again), [1] = sum (x - slab mean)^2.
template <bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const float4* __restrict__ x, const float4* __restrict__ dy,
                                                        const float4* __restrict__ y, const float4* __restrict__ mean,
                                                        const float4* __restrict__ invstd, BnShape s, int relu,
                                                        float* __restrict__ partial) {
    __shared__ float4 red[BWD ? 2 : 3][256];
    __shared__ double wide[BWD ? 1 : 4][BWD ? 1 : 256], centre[BWD ? 1 : 4][BWD ? 1 : 256];    // (forward: the lanes' fp64 terms)
    const int tid = threadIdx.x, c4 = tid & (s.cg - 1), rl = tid / s.cg, nrl = 256 / s.cg;
    const long long r0 = (long long)blockIdx.x * s.slab, r1 = r0 + s.slab < s.rows ? r0 + s.slab : s.rows;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    const float4 k = BWD ? mean[c4] : x[(r0 + rl < r1 ? r0 + rl : r0) * s.cg + c4];      // (a lane without rows: sums of 0)
    const float4 is = BWD ? invstd[c4] : make_float4(1.f, 1.f, 1.f, 1.f);
    // four rows per trip, every load issued before the first add (the pass is latency-bound otherwise)
    for (long long r = r0 + rl; r < r1; r += 4ll * nrl) {
        float4 xv[4], gv[4], yv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long ru = r + (long long)u * nrl;
            const bool in = ru < r1;
            const long long i = (in ? ru : r) * s.cg + c4;
            xv[u] = x[i];
            if (BWD) {
                gv[u] = dy[i];
                if (relu) yv[u] = y[i];
                if (!in) gv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else if (!in) {
                xv[u] = k;                       // contributes (k - k) = 0
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 d = f4_sub(xv[u], k);
            if (!BWD) {
                a = f4_add(a, d);
                b = f4_add(b, f4_mul(d, d));
            } else {
                float4 g = gv[u];
                if (relu) {
                    g.x = yv[u].x > 0.f ? g.x : 0.f; g.y = yv[u].y > 0.f ? g.y : 0.f;
                    g.z = yv[u].z > 0.f ? g.z : 0.f; g.w = yv[u].w > 0.f ? g.w : 0.f;
                }
                a = f4_add(a, g);
                b = f4_add(b, f4_mul(g, f4_mul(d, is)));
            }
        }
    }
    red[0][tid] = a;
    red[1][tid] = b;
    if (!BWD) red[2][tid] = k;
    __syncthreads();
    if (!BWD) {
        // lane j holds nj rows; about K = k_0: sum (x - K) = sum_j a_j + nj (k_j - K), then about the slab's mean m:
        // sum (x - m)^2 = sum_j b_j + 2 (k_j - m) a_j + nj (k_j - m)^2 - in fp64, where a shift's square is exact.
        // Every lane forms its own term (one wavefront doing all of them took 6 us); row lane 0 adds them in lane order.
        const long long ng = r1 - r0;
        const int lanes = ng < nrl ? (int)ng : nrl;
        // rows j, j + nrl, ..: ng / nrl of them and one more below the remainder (nrl is a power of two)
        const double nj = rl < lanes ? (double)((ng >> __builtin_ctz(nrl)) + (rl < (int)(ng & (nrl - 1)) ? 1 : 0)) : 0.0;
        const float4 k0 = red[2][c4];
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0}, m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wide[q][tid] = (double)f4_at(a, q) + nj * ((double)f4_at(k, q) - (double)f4_at(k0, q));
        __syncthreads();
        if (rl == 0) {
            for (int j = 0; j < lanes; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) s1[q] += wide[q][j * s.cg + c4];
#pragma unroll
            for (int q = 0; q < 4; ++q) centre[q][c4] = (double)f4_at(k, q) + s1[q] / (double)ng;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            m[q] = centre[q][c4];
            const double e = (double)f4_at(k, q) - m[q];
            wide[q][tid] = (double)f4_at(b, q) + 2.0 * e * (double)f4_at(a, q) + nj * e * e;
        }
        __syncthreads();
        if (rl != 0) return;
        for (int j = 0; j < lanes; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) s2[q] += wide[q][j * s.cg + c4];
        float4* p = reinterpret_cast<float4*>(partial + (size_t)blockIdx.x * 2 * s.c);
        p[c4] = make_float4((float)s1[0], (float)s1[1], (float)s1[2], (float)s1[3]);
        p[s.cg + c4] = make_float4(s2[0] < 0.0 ? 0.f : (float)s2[0], s2[1] < 0.0 ? 0.f : (float)s2[1],
                                   s2[2] < 0.0 ? 0.f : (float)s2[2], s2[3] < 0.0 ? 0.f : (float)s2[3]);
        return;
    }
    if (rl == 0) {
        for (int j = 1; j < nrl; ++j) {
            a = f4_add(a, red[0][j * s.cg + c4]);
            b = f4_add(b, red[1][j * s.cg + c4]);
        }
        float4* p = reinterpret_cast<float4*>(partial + (size_t)blockIdx.x * 2 * s.c);
        p[c4] = a;
        p[s.cg + c4] = b;
    }
}

// mean, invstd and the running statistics (momentum update with the unbiased variance, as torch does) of one channel
__device__ __forceinline__ void bn_write_stats(int c, double mean, double var, double n, float eps, float momentum,
                                               float* running_mean, float* running_var, float* save_mean, float* save_invstd) {
    save_mean[c] = (float)mean;
    save_invstd[c] = 1.0f / __builtin_sqrtf((float)var + eps);
    if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
}

// bn_reduce_kernel<false>'s slabs -> mean, invstd, running statistics; one workgroup per 4 channels, fp64, ascending slab
// order inside 64 slab lanes, then the lanes in ascending order.  Slab g holds a_g = sum (x - K_g) around its first row
// K_g and q_g = sum (x - m_g)^2 around its own mean m_g = K_g + a_g / n_g: first the mean (about K_0), then
// sum_g q_g + n_g (m_g - mean)^2 - no term of which cancels.
__global__ __launch_bounds__(256) void bn_finalize_slabs_kernel(const float* __restrict__ partial, const float* __restrict__ x,
                                                                BnShape s, float eps, float momentum, float* running_mean,
                                                                float* running_var, float* __restrict__ save_mean,
                                                                float* __restrict__ save_invstd) {
    __shared__ double red[64][4];
    __shared__ double centre[4];
    const int cl = threadIdx.x & 3, gl = threadIdx.x >> 2, c = blockIdx.x * 4 + cl;
    const bool live = c < s.c;
    const double n = (double)s.rows, k0 = live ? (double)x[c] : 0.0;
    // a lane's slabs (at most BN_MAX_SLABS / 64 = 8) in registers, every load issued before the first add: both passes
    // below run off them
    constexpr int PER = BN_MAX_SLABS / 64;
    double ng[PER], kg[PER], ag[PER], qg[PER], mg[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int g = gl + 64 * t;
        const bool ok = live && g < s.slabs;
        const long long r0 = ok ? (long long)g * s.slab : 0;
        const size_t p = ok ? (size_t)g * 2 * s.c + c : 0;
        ng[t] = ok ? (double)(r0 + s.slab < s.rows ? s.slab : s.rows - r0) : 0.0;
        kg[t] = ok ? (double)x[(size_t)r0 * s.c + c] : 0.0;
        ag[t] = ok ? (double)partial[p] : 0.0;
        qg[t] = ok ? (double)partial[p + s.c] : 0.0;
        mg[t] = ok ? kg[t] + ag[t] / ng[t] : 0.0;                 // the slab's mean (the divisions ahead of the barrier)
    }
    double a = 0.0;
#pragma unroll
    for (int t = 0; t < PER; ++t)
        if (ng[t] > 0.0) a += ag[t] + ng[t] * (kg[t] - k0);
    red[gl][cl] = a;
    __syncthreads();
    if (gl == 0) {
        for (int j = 1; j < 64; ++j) a += red[j][cl];
        centre[cl] = k0 + a / n;
    }
    __syncthreads();
    const double mean = centre[cl];
    double b = 0.0;
#pragma unroll
    for (int t = 0; t < PER; ++t)
        if (ng[t] > 0.0) {
            const double e = mg[t] - mean;
            b += qg[t] + ng[t] * e * e;
        }
    red[gl][cl] = b;                                  // (centre[] was written after every lane 0 had read red[])
    __syncthreads();
    if (gl != 0 || !live) return;
    for (int j = 1; j < 64; ++j) b += red[j][cl];
    bn_write_stats(c, mean, b / n, n, eps, momentum, running_mean, running_var, save_mean, save_invstd);
}

// Combine a producer's slabs of [0] = sum d, [1] = sum d^2, d = x - shift (fp64, ascending slab order inside 64 slab
// lanes, then the lanes in ascending order); one workgroup per 4 channels.
//   BWD = false: mean, invstd (+ running statistics)
//   BWD = true : d_beta = sum g, d_gamma = sum g * xhat
// (shift: what the producer's epilogue subtracted, per channel - chosen before it saw the batch; it may alias running_mean:
//  no __restrict__ on the two, the read precedes the update)
//
// var = E[d^2] - E[d]^2 of fp32 sums loses (E[d]^2 / var) * 2^-24 of itself per rounding.  A channel whose shift turns out
// more than 2 sigma off (E[d]^2 > BN_RECENTRE * var), or whose sums are not finite (a stale NaN shift: d = x - NaN; a
// finite one so far out that d^2 overflows fp32), is therefore taken AGAIN here, over the activation `act` itself, by this
// workgroup's 64 row lanes in fp64 around row 0 of the channel - a fixed order too, so still deterministic.  (Row 0, not
// the mean just found: behind a wild shift that mean is rounding debris of the shift's size.  A row of the data is at most
// sqrt(n) sigma from its mean, which costs fp64 n * 2^-53 of the variance.)  Slow (4 channels per workgroup) and rare: a
// layer's first step, a jump of the data between two steps, the step after a non-finite one.  Channels whose shift was
// typical never take that pass and keep their bits.
template <bool BWD>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, const float* shift,
                                                          const float* __restrict__ act, BnShape s, float eps,
                                                          float momentum, float* running_mean,
                                                          float* __restrict__ running_var, float* __restrict__ out0,
                                                          float* __restrict__ out1) {
    __shared__ double red[2][64][4];
    __shared__ int again[4];
    const int cl = threadIdx.x & 3, gl = threadIdx.x >> 2, c = blockIdx.x * 4 + cl;
    double a = 0.0, b = 0.0;
    if (c < s.c)
        for (int g = gl; g < s.slabs; g += 64) {
            a += (double)partial[(size_t)g * 2 * s.c + c];
            b += (double)partial[(size_t)g * 2 * s.c + s.c + c];
        }
    red[0][gl][cl] = a;
    red[1][gl][cl] = b;
    __syncthreads();
    if (BWD) {
        if (gl != 0 || c >= s.c) return;
        for (int j = 1; j < 64; ++j) { a += red[0][j][cl]; b += red[1][j][cl]; }
        out0[c] = (float)b;          // d_gamma
        out1[c] = (float)a;          // d_beta
        return;
    }
    const double n = (double)s.rows;
    double mean = 0.0, var = 0.0;
    if (gl == 0) {
        for (int j = 1; j < 64; ++j) { a += red[0][j][cl]; b += red[1][j][cl]; }
        const double m1 = a / n;
        mean = (shift && c < s.c ? (double)shift[c] : 0.0) + m1;
        var = b / n - m1 * m1;
        var = var > 0.0 ? var : 0.0;
        // (written so that a NaN on either side asks for the second pass, and so does a sum of squares that overflowed:
        //  var = inf would pass the comparison and come out as invstd = 0)
        const bool redo = act && c < s.c && !(m1 * m1 <= BN_RECENTRE * var && var < __builtin_inf());
        again[cl] = redo ? 1 : 0;
    }
    __syncthreads();      // (orders the write of again[], and every lane 0's reads of red[][1..63] before the writes below)
    if ((again[0] | again[1] | again[2] | again[3]) != 0) {               // rare: uniform over the workgroup
        a = 0.0; b = 0.0;
        const double k = again[cl] ? (double)act[c] : 0.0;
        if (again[cl])
            for (long long r = gl; r < s.rows; r += 64) {
                const double d = (double)act[(size_t)r * s.c + c] - k;
                a += d;
                b += d * d;
            }
        red[0][gl][cl] = a;
        red[1][gl][cl] = b;
        __syncthreads();
        if (gl == 0 && again[cl]) {
            for (int j = 1; j < 64; ++j) { a += red[0][j][cl]; b += red[1][j][cl]; }
            const double m1 = a / n;
            mean = k + m1;
            var = b / n - m1 * m1;
            var = var > 0.0 ? var : 0.0;
        }
    }
    if (gl != 0 || c >= s.c) return;
    bn_write_stats(c, mean, var, n, eps, momentum, running_mean, running_var, out0, out1);
}

// y = [relu]( (x - mean) * invstd * gamma + beta [+ residual] )
__global__ __launch_bounds__(256) void bn_apply_kernel(const float4* __restrict__ x, const float4* __restrict__ res,
                                                       const float4* __restrict__ mean, const float4* __restrict__ invstd,
                                                       const float4* __restrict__ gamma, const float4* __restrict__ beta,
                                                       long long total4, int cg, int relu, float4* __restrict__ y) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c4 = (int)(i & (cg - 1));
    const float4 xv = x[i], m = mean[c4], is = invstd[c4], g = gamma[c4], b = beta[c4];
    float4 v = f4_add(f4_mul(f4_mul(f4_sub(xv, m), is), g), b);
    if (res) v = f4_add(v, res[i]);
    if (relu) {
        v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
        v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
    }
    y[i] = v;
}

// dx = gamma * invstd * (g - d_beta / n - xhat * d_gamma / n);  d_residual = g
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float4* __restrict__ dy, const float4* __restrict__ y,
                                                           const float4* __restrict__ x, const float4* __restrict__ mean,
                                                           const float4* __restrict__ invstd, const float4* __restrict__ gamma,
                                                           const float4* __restrict__ dgamma, const float4* __restrict__ dbeta,
                                                           long long total4, int cg, int relu, float inv_n,
                                                           float4* __restrict__ dx, float4* __restrict__ dres) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c4 = (int)(i & (cg - 1));
    float4 g = dy[i];
    if (relu) {
        const float4 yv = y[i];
        g.x = yv.x > 0.f ? g.x : 0.f; g.y = yv.y > 0.f ? g.y : 0.f;
        g.z = yv.z > 0.f ? g.z : 0.f; g.w = yv.w > 0.f ? g.w : 0.f;
    }
    if (dres) dres[i] = g;
    const float4 is = invstd[c4];
    const float4 xh = f4_mul(f4_sub(x[i], mean[c4]), is);
    const float4 sc = f4_mul(gamma[c4], is);
    const float4 dg = dgamma[c4], db = dbeta[c4];
    float4 v;
    v.x = sc.x * (g.x - db.x * inv_n - xh.x * (dg.x * inv_n));
    v.y = sc.y * (g.y - db.y * inv_n - xh.y * (dg.y * inv_n));
    v.z = sc.z * (g.z - db.z * inv_n - xh.z * (dg.z * inv_n));
    v.w = sc.w * (g.w - db.w * inv_n - xh.w * (dg.w * inv_n));
    dx[i] = v;
}

static bool bn_shape(int64_t rows, int c, BnShape* s) {
    if (rows <= 0 || c < 4 || c % 4 != 0) return false;
    const int cg = c / 4;
    if (cg > 256 || (cg & (cg - 1)) != 0) return false;
    s->rows = rows; s->c = c; s->cg = cg;
    // slabs of at least one sweep of the workgroup's row lanes x 4, at most BN_MAX_SLABS of them
    const int64_t sweep = (int64_t)(256 / cg) * 4;
    int64_t slabs = cdiv(rows, sweep);
    if (slabs > BN_MAX_SLABS) slabs = BN_MAX_SLABS;
    s->slab = cdiv(rows, slabs);
    s->slabs = (int)cdiv(rows, s->slab);
    return true;
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_bn_train_supported(int64_t rows, int c) {
    BnShape s;
    return bn_shape(rows, c, &s) ? 1 : 0;
}

IPSX_API size_t ipsx_bn_train_workspace_floats(int64_t rows, int c) {
    BnShape s;
    if (!bn_shape(rows, c, &s)) return 0;
    return (size_t)s.slabs * 2 * c;
}

IPSX_API int ipsx_bn_train_forward(const float* x, const float* residual, int64_t rows, int c, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean,
                                   float* running_var, int relu, float* y, float* save_mean, float* save_invstd,
                                   float* workspace, void* stream) {
    BnShape s;
    IPSX_REQUIRE(bn_shape(rows, c, &s), "bn_train_forward: rows = %lld, C = %d (C / 4 must be a power of two <= 256)",
                 (long long)rows, c);
    IPSX_REQUIRE(x && gamma && beta && y && save_mean && save_invstd && workspace, "bn_train_forward: bad arguments");
    hipStream_t st = as_stream(stream);
    bn_reduce_kernel<false><<<dim3(s.slabs), dim3(256), 0, st>>>(reinterpret_cast<const float4*>(x), nullptr, nullptr,
                                                                 nullptr, nullptr, s, 0, workspace);
    bn_finalize_slabs_kernel<<<dim3((unsigned)cdiv(c, 4)), dim3(256), 0, st>>>(workspace, x, s, eps, momentum, running_mean,
                                                                                 running_var, save_mean, save_invstd);
    const long long total4 = (long long)rows * s.cg;
    bn_apply_kernel<<<dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, st>>>(
        reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(residual),
        reinterpret_cast<const float4*>(save_mean), reinterpret_cast<const float4*>(save_invstd),
        reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(beta), total4, s.cg, relu,
        reinterpret_cast<float4*>(y));
    return launched("bn_train_forward");
}

IPSX_API int ipsx_bn_train_forward_partials(const float* x, const float* residual, int64_t rows, int c, const float* gamma,
                                            const float* beta, float eps, float momentum, float* running_mean,
                                            float* running_var, int relu, float* y, float* save_mean, float* save_invstd,
                                            const float* partial, int64_t slabs, const float* shift, void* stream) {
    BnShape s;
    IPSX_REQUIRE(bn_shape(rows, c, &s), "bn_train_forward_partials: rows = %lld, C = %d (C / 4 must be a power of two <= 256)",
                 (long long)rows, c);
    IPSX_REQUIRE(x && gamma && beta && y && save_mean && save_invstd && partial && slabs > 0 && slabs < (1 << 30),
                 "bn_train_forward_partials: bad arguments");
    hipStream_t st = as_stream(stream);
    s.slabs = (int)slabs;                                   // the producer's slabs (bn_finalize_kernel only counts them)
    bn_finalize_kernel<false><<<dim3((unsigned)cdiv(c, 4)), dim3(256), 0, st>>>(partial, shift, x, s, eps, momentum,
                                                                                  running_mean, running_var, save_mean,
                                                                                  save_invstd);
    const long long total4 = (long long)rows * s.cg;
    bn_apply_kernel<<<dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, st>>>(
        reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(residual),
        reinterpret_cast<const float4*>(save_mean), reinterpret_cast<const float4*>(save_invstd),
        reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(beta), total4, s.cg, relu,
        reinterpret_cast<float4*>(y));
    return launched("bn_train_forward_partials");
}

IPSX_API int ipsx_bn_train_backward(const float* dy, const float* y, const float* x, int64_t rows, int c,
                                    const float* gamma, const float* save_mean, const float* save_invstd, int relu,
                                    float* dx, float* dresidual, float* dgamma, float* dbeta, float* workspace,
                                    void* stream) {
    BnShape s;
    IPSX_REQUIRE(bn_shape(rows, c, &s), "bn_train_backward: rows = %lld, C = %d (C / 4 must be a power of two <= 256)",
                 (long long)rows, c);
    IPSX_REQUIRE(dy && x && gamma && save_mean && save_invstd && dx && dgamma && dbeta && workspace && (y || !relu),
                 "bn_train_backward: bad arguments");
    hipStream_t st = as_stream(stream);
    bn_reduce_kernel<true><<<dim3(s.slabs), dim3(256), 0, st>>>(
        reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(y),
        reinterpret_cast<const float4*>(save_mean), reinterpret_cast<const float4*>(save_invstd), s, relu, workspace);
    bn_finalize_kernel<true><<<dim3((unsigned)cdiv(c, 4)), dim3(256), 0, st>>>(workspace, nullptr, nullptr, s, 0.f, 0.f,
                                                                                 nullptr, nullptr, dgamma, dbeta);
    const long long total4 = (long long)rows * s.cg;
    bn_bwd_apply_kernel<<<dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, st>>>(
        reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(y), reinterpret_cast<const float4*>(x),
        reinterpret_cast<const float4*>(save_mean), reinterpret_cast<const float4*>(save_invstd),
        reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(dgamma),
        reinterpret_cast<const float4*>(dbeta), total4, s.cg, relu, 1.0f / (float)rows, reinterpret_cast<float4*>(dx),
        reinterpret_cast<float4*>(dresidual));
    return launched("bn_train_backward");
}
