// logits_wave.h - the attention logits of ONE wavefront's 32 patches (logits.hip's kernels), as a device function the
// selection loop that computes its own image's logits in a prologue shares (scan_mnist.hip).  A patch's logits depend on that
// patch alone - and a row of a 32x32x2 MFMA on that row of A alone -, so which tile a patch falls into, and which wavefront
// takes the tile, does not touch a bit of them.
#pragma once

#include "scan_common.h"

namespace ipsx {

struct LogitsArgs {
    const float* emb; long long emb_bs;
    const float* pos; long long pos_bs;
    const float* vp;             // folded query, packed (fold_query_kernel)
    long long n;
    int d, R, kgs;
    float* out; long long out_bs;
};

// One wavefront = 32 patches x all H*T logits (NT tiles of 32 columns); WAVES wavefronts per workgroup (logits_kernel: 4), and
// workgroup bx of image bi takes rows [bx * WAVES * 32, (bx + 1) * WAVES * 32).
// U: k-groups per trip of the pipelined loop (d % 8 == 0).  It only sets how far the operand loads run ahead of the MFMAs -
// 8: logits_kernel, a wave per SIMD with 512 registers a lane; 4: a kernel held to 128 (scan_mnist.hip) - the MFMA sequence
// of every accumulator, k ascending, is the same for every U.
// POS: 0 - whether there are positional rows is asked of the pointer, lane by lane, in front of every load of one (a branch
// the compiler cannot move: each k-group's emb + pos is a round trip of its own); 1 / -1 - the caller knows (there are / are
// none): the loads of a trip are issued together and the additions follow.  The same additions either way.
template <int NT, int U = 8, int WAVES = 4, int POS = 0>
__device__ __forceinline__ void logits_wave(const LogitsArgs& a, unsigned bx, int bi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const long long r0 = ((long long)bx * WAVES + wave) * 32;
    if (r0 >= a.n) return;                                           // wave-uniform
    const long long row = r0 + (lane & 31);
    const bool rv = row < a.n;
    const float* e = a.emb + (size_t)bi * a.emb_bs + (size_t)(rv ? row : 0) * a.d + 4 * half;
    const float* p = a.pos ? a.pos + (size_t)bi * a.pos_bs + (size_t)(rv ? row : 0) * a.d + 4 * half : nullptr;

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    const float4* vq = reinterpret_cast<const float4*>(a.vp) + lane;
    const bool vec = (a.d & 7) == 0;                 // rows are 16-byte aligned and every k-group is complete
    int kg0 = 0;
    if (vec) {
        // U (eight) k-groups per trip, every operand load of the trip in flight before its first MFMA: with one wave per SIMD
        // (a part of a slide is ~100 workgroups) nothing else hides the load latency - 64 dependent trips of ~0.5 us
        // were the whole 35 us of the kernel.  The MFMA sequence of every accumulator is unchanged.
        // (two register sets: the loads of the next trip are issued before this trip's MFMAs)
        float4 ev[2][U], bv[2][NT][U];
        auto fetch = [&](int k0, int set) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ev[set][u] = *reinterpret_cast<const float4*>(e + (k0 + u) * 8);
                if (POS == 0 ? p != nullptr : POS > 0) {
                    const float4 pv = *reinterpret_cast<const float4*>(p + (k0 + u) * 8);
                    ev[set][u].x = ev[set][u].x + pv.x; ev[set][u].y = ev[set][u].y + pv.y;
                    ev[set][u].z = ev[set][u].z + pv.z; ev[set][u].w = ev[set][u].w + pv.w;
                }
#pragma unroll
                for (int i = 0; i < NT; ++i) bv[set][i][u] = vq[((size_t)i * a.kgs + k0 + u) * 64];
            }
        };
        auto mma = [&](int set) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float a0 = rv ? ev[set][u].x : 0.0f, a1 = rv ? ev[set][u].y : 0.0f;
                const float a2 = rv ? ev[set][u].z : 0.0f, a3 = rv ? ev[set][u].w : 0.0f;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[set][i][u].x, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[set][i][u].y, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, bv[set][i][u].z, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, bv[set][i][u].w, acc[i], 0, 0, 0);
                }
            }
        };
        if (a.kgs >= U) {
            fetch(0, 0);
            for (; kg0 + 2 * U <= a.kgs; kg0 += 2 * U) {
                fetch(kg0 + U, 1);
                mma(0);
                if (kg0 + 3 * U <= a.kgs) fetch(kg0 + 2 * U, 0);
                mma(1);
            }
            if (kg0 + U <= a.kgs) { mma(0); kg0 += U; }
        }
    }
    for (int kg = kg0; kg < a.kgs; ++kg) {
        float av[4];
        if (vec) {                                   // one 16-byte load per operand row per k-group
            const float4 ev = *reinterpret_cast<const float4*>(e + kg * 8);
            av[0] = ev.x; av[1] = ev.y; av[2] = ev.z; av[3] = ev.w;
            if (p) {
                const float4 pv = *reinterpret_cast<const float4*>(p + kg * 8);
                av[0] = av[0] + pv.x; av[1] = av[1] + pv.y; av[2] = av[2] + pv.z; av[3] = av[3] + pv.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) av[j] = rv ? av[j] : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = kg * 8 + j;              // + 4*half is in the base pointers
                float v = (c + 4 * half < a.d) ? e[c] : 0.0f;
                if (p) v = v + ((c + 4 * half < a.d) ? p[c] : 0.0f);
                av[j] = rv ? v : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const float4 b = vq[((size_t)i * a.kgs + kg) * 64];
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], b.x, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], b.y, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], b.z, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], b.w, acc[i], 0, 0, 0);
        }
    }
    // C layout: lane = column (logit index), registers = rows (patches)
    float* out = a.out + (size_t)bi * a.out_bs;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int o = i * 32 + (lane & 31);
        if (o < a.R) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long rr = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (rr < a.n) out[(size_t)rr * a.R + o] = acc[i][r];
            }
        }
    }
}

}  // namespace ipsx
