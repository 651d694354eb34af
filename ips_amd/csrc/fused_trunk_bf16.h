// fused_trunk_bf16.h - the bf16 fused trunk, precision 1 "bf16" (BASELINE configs[4]): fused_trunk_bf16_kernel (included by
// fused_trunk.hip behind fused_trunk_split.h, whose stem (stem_pool<1>, transpose_stem), packed-weight layout, LDS image
// layout (XL<1>, epilogue_l1s<1, 2>, store_planes4<1>) it shares).
//
// One workgroup = 4 wavefronts = EIGHT patches, 76 KB of LDS, two workgroups per compute unit.
//   stem + 8x8 stage   two quads of four patches go through stem + layer1 one after the other, each on its own four slabs,
//             the images IN PLACE (convolution reads, barrier, epilogue overwrites, barrier); the first quad's final images
//             rest while the second quad works.  Stem: wave = patch.  Its fp32 result is the residual identity; layer1 runs
//             wave = (ROW TILE of 32 output channels, PAIR of patches), so the half of a patch's identity that the pair's
//             other wave carries reaches it through the (dead) input slab.  A K-step of conv_l1_bf16 is 4 MFMAs - the pair's
//             128 pixels are 4 column tiles - on 1 KB of weights, one 16-byte register quad per lane: the weight ring holds
//             EIGHT K-steps (requested seven ahead: ~900 pipe cycles of cover for an L2 round trip of 500+), activations
//             4 ds_read_b128 per K-step, two steps ahead.
//   4x4 stage  ONCE over all eight patches: wave = 32 output channels x 128 pixels = FOUR column tiles per weight operand,
//             so a K-step is again 4 MFMAs on 1 KB of weights (fetched once per workgroup), ring of six.  The 4x4 images
//             ping-pong between two sets of eight (2 x 38 KB) laid over the 8x8 slabs: ONE barrier per layer.
//   avgpool   sequential 16-term sums of fp32 images [pix][PS2], one per patch slab.
// Arithmetic: operands (input pixels, weights, every activation a convolution reads) rounded to bf16, nearest even; ONE
// bf16 product per term on v_mfma_f32_32x32x16_bf16, fp32 accumulation in K order (tap-major, 16 channels per K-step);
// BatchNorm as one fma, identity and residual sum in fp32 registers, ReLU; the reference has no reduced-precision path:
// tolerance-tested against the fp32 kernel and a float64 emulation that rounds at the same places, and held bit for bit
// to a recorded result (tests/golden/bf16_trunk.npz, tests/test_hip_kernels.py::
// test_bf16_trunk_matches_recorded_first_build) - ragged ends, index lists and half-stored patches included.
// How the kernel came to this shape: docs/rounds.md.

// A patch's slab: its 8x8 image (65 pixel rows of 144 B = 9,360 B) rounded up to a multiple of 256 B.  The 4x4 stage reads
// TWO patches per ds_read_b128 (lanes 0-15 | 16-31); the LDS serves such a read in groups of 16 lanes that mix the two
// patches, conflict-free only when the second patch's rows fall on the bank slots the first one leaves free - which they do
// when the patches lie a multiple of 256 B apart.  (At the unrounded 9,360 B 7 of 16 lanes of every group fall on a taken
// slot: the 4x4 stage then runs at 1.8-2.1 x its matrix-pipe time even with the unit to itself, 2.8 beside a second wave -
// LDS-bound.)  The 4x4 images (17 rows of 272 B) get a stride of their own, BF16_S2, for the same reason.
constexpr int BF16_SLAB = (XL<1>::SLAB + 255) & ~255;      // 9,472 B
constexpr int BF16_S2 = ((XZ2 + 1) * XP2 + 255) & ~255;   // 4,864 B: a patch's 4x4 image (16 pixel rows + the zero row)
constexpr int BF16_LDS = 16 * BF16_S2;                  // 77,824 B: two sets of eight 4x4 images; the eight 8x8 slabs need 75,776
// (a slab also holds a patch's fp32 [16][PS2] image for the average pool)
static_assert(8 * BF16_SLAB <= BF16_LDS && BF16_LDS <= 80 * 1024 && BF16_SLAB >= 16 * PS2 * 4, "two workgroups per unit");

#define BF16_SG_MFMA(n) __builtin_amdgcn_sched_group_barrier(0x008, n, 0)
#define BF16_SG_LDS(n) __builtin_amdgcn_sched_group_barrier(0x100, n, 0)
#define BF16_SG_VMEM(n) __builtin_amdgcn_sched_group_barrier(0x020, n, 0)

// byte offset (within a patch slab) of the pixel row a lane reads for tap `tap` of output pixel 32 h + i: the source pixel,
// or the zero row for a halo tap; + 16 * half: this lane half's 8 channels of a K-step
__device__ __forceinline__ unsigned bf16_tap_off(int tap, int h, int i, int half) {
    const int t3 = tap / 3;
    const int dy = t3 - 1, dx = tap - 3 * t3 - 1;
    const int x = i & 7, y = (i >> 3) + 4 * h;
    const bool ok = (unsigned)(x + dx) < 8u && (unsigned)(y + dy) < 8u;
    return (unsigned)((ok ? 32 * h + i + dy * 8 + dx : XZ1) * XP1 + 16 * half);
}

// acc[2 q + h] = output channels 32 rt .. 32 rt + 31 (rows) x pixels 32 h .. 32 h + 31 of patch q of the pair (columns) of
// conv3x3(images at P0, P0 + BF16_SLAB) over K = 9 * 64.  wp: the layer's packed weights, wave-uniform; rt: wave-uniform.
__device__ __forceinline__ void conv_l1_bf16(const void* __restrict__ wp, const char* P0, int rt, f32x16 (&acc)[4], int lane) {
    constexpr int WR = 8, XR = 3, G = 36;          // weight ring (7 K-steps ahead), activation ring (2 ahead), K-steps
    const int i = lane & 31, half = lane >> 5;
    const char* wb = reinterpret_cast<const char*>(wp) + (size_t)rt * G * 1024;      // wave-uniform: scalar base ...
    const unsigned lo = lane * 16;                                                  // ... + the only vector part
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) zero(acc[ct]);
    uint4 wr[WR], xr[XR][4];
#define BF16_LOADW(g) wr[(g) % WR] = *reinterpret_cast<const uint4*>(wb + (size_t)((g) < G ? (g) : G - 1) * 1024 + lo)
#define BF16_LOADX(g)                                                                                              \
    do {                                                                                                         \
        const int g_ = (g) < G ? (g) : G - 1;                                                                    \
        const char* p0_ = P0 + bf16_tap_off(g_ >> 2, 0, i, half) + (g_ & 3) * 32;                                  \
        const char* p1_ = P0 + bf16_tap_off(g_ >> 2, 1, i, half) + (g_ & 3) * 32;                                  \
        xr[(g) % XR][0] = *reinterpret_cast<const uint4*>(p0_);                                                  \
        xr[(g) % XR][1] = *reinterpret_cast<const uint4*>(p1_);                                                  \
        xr[(g) % XR][2] = *reinterpret_cast<const uint4*>(p0_ + BF16_SLAB);                                        \
        xr[(g) % XR][3] = *reinterpret_cast<const uint4*>(p1_ + BF16_SLAB);                                        \
    } while (0)
#pragma unroll
    for (int g = 0; g < WR - 1; ++g) BF16_LOADW(g);
    BF16_LOADX(0);
    BF16_LOADX(1);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        BF16_LOADX(g + 2);
        BF16_LOADW(g + WR - 1);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = MFMA16(wr[g % WR], xr[g % XR][ct], acc[ct]);
        BF16_SG_MFMA(1); BF16_SG_LDS(2); BF16_SG_MFMA(1); BF16_SG_VMEM(1); BF16_SG_MFMA(1); BF16_SG_LDS(2); BF16_SG_MFMA(1);
        SB();
    }
#undef BF16_LOADW
#undef BF16_LOADX
}

// BatchNorm (+ identity) + ReLU on the wave's tiles, then the bf16 image the next layer reads: channels 32 rt .. of both
// patches of the pair at Q0, Q0 + BF16_SLAB.  MODE 0: BN + ReLU; 1: BN + identity + ReLU, identity updated
template <int MODE>
__device__ __forceinline__ void epilogue_l1_bf16(char* Q0, const float* __restrict__ al, const float* __restrict__ sh, int rt,
                                              const f32x16 (&acc)[4], f32x16 (&idn)[4], int lane) {
    const int i = lane & 31, half = lane >> 5;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int ch = rt * 32 + 8 * g + 4 * half;
        const float4 A = *reinterpret_cast<const float4*>(al + ch), B = *reinterpret_cast<const float4*>(sh + ch);
        const float Aa[4] = {A.x, A.y, A.z, A.w}, Bb[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = __builtin_fmaf(acc[ct][4 * g + j], Aa[j], Bb[j]);
                if (MODE == 1) x = x + idn[ct][4 * g + j];
                x = x > 0.0f ? x : 0.0f;
                if (MODE == 1) idn[ct][4 * g + j] = x;
                v[j] = x;
            }
            store_planes4<1>(Q0 + (ct >> 1) * BF16_SLAB + ((ct & 1) * 32 + i) * XP1 + 2 * ch, XP1, v);
        }
    }
}

// input pixels of one patch, 16 per lane: float32 or half-precision storage (2 KiB per patch, 8 bytes per lane and load)
__device__ __forceinline__ void bf16_fetch(const FusedArgs& a, long long pi, int lane, float4 (&px)[4]) {
    if (a.in_dtype == 0) {
        const float4* src = reinterpret_cast<const float4*>(a.patches + (size_t)pi * 1024);
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = src[k * 64 + lane];
    } else {
        const uint2* src = reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(a.patches) + (size_t)pi * 1024);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint2 h = src[k * 64 + lane];
            const unsigned short hs[4] = {(unsigned short)(h.x & 0xFFFFu), (unsigned short)(h.x >> 16),
                                          (unsigned short)(h.y & 0xFFFFu), (unsigned short)(h.y >> 16)};
            float f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                f[j] = a.in_dtype == 1 ? __uint_as_float((unsigned)hs[j] << 16)
                                       : (float)__builtin_bit_cast(_Float16, hs[j]);
            px[k] = make_float4(f[0], f[1], f[2], f[3]);
        }
    }
}

// 4x4 stage over EIGHT patches: wave = 32 output channels x 128 pixels - column tile ct = patches 2 ct, 2 ct + 1 (column
// i -> patch 2 ct + (i >> 4), pixel i & 15).  A K-step = 4 MFMAs - 128 pipe cycles - on 1 KB of weights; passes of 3 taps (12 or 24 K-steps; 1x1: all 4)
// close both rings.
template <int CIN, int WIN, int RB, int ZR, int STRIDE, int KS, int PSTR>
__device__ __forceinline__ void conv_l2_bf16(const void* __restrict__ wp, const char* lds, f32x16 (&acc)[4], int lane, int wave) {
    constexpr int TAPS = KS * KS, SPT = CIN / 16, G = TAPS * SPT;          // K-steps per tap, K-steps
    constexpr int TPP = TAPS < 3 ? TAPS : 3, PASS = TPP * SPT;             // a pass = 3 taps (12 or 24 K-steps; 1x1: all 4)
    constexpr int WR = 6, XR = 3, XA = 2;                                  // a K-step is 128 pipe cycles here: 5 ahead = 640
    constexpr int PAD = KS / 2;
    static_assert(G % PASS == 0 && (G == PASS || (PASS % XR == 0 && PASS % WR == 0)) && XA < SPT, "passes close the rings");
    const int i = lane & 31, half = lane >> 5;
    const int pix = i & 15, oy = pix >> 2, ox = pix & 3;
    const char* wb = reinterpret_cast<const char*>(wp) + (size_t)wave * G * 1024;    // wave-uniform
    const unsigned lo = lane * 16;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) zero(acc[ct]);
    uint4 wr[WR], xr[XR][4];
    auto tap_row = [&](int tap) -> unsigned {
        tap = tap < TAPS ? tap : TAPS - 1;
        const int ky = tap / KS, kx = tap - ky * KS;
        const int iy = oy * STRIDE + ky - PAD, ix = ox * STRIDE + kx - PAD;
        const bool ok = (unsigned)iy < (unsigned)WIN && (unsigned)ix < (unsigned)WIN;
        return (unsigned)((i >> 4) * PSTR + 16 * half + (ok ? iy * WIN + ix : ZR) * RB);
    };
#pragma unroll
    for (int g = 0; g < WR - 1; ++g) wr[g] = *reinterpret_cast<const uint4*>(wb + (size_t)(g < G ? g : G - 1) * 1024 + lo);
    unsigned rows[TPP + 1];
#pragma unroll
    for (int t = 0; t <= TPP; ++t) rows[t] = tap_row(t);
#pragma unroll
    for (int g = 0; g < XA; ++g)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) xr[g][ct] = *reinterpret_cast<const uint4*>(lds + rows[0] + g * 32 + ct * 2 * PSTR);
#pragma unroll 1
    for (int g0 = 0; g0 < G; g0 += PASS) {
#pragma unroll
        for (int u = 0; u < PASS; ++u) {
            const int g = g0 + u;
            {
                const unsigned p = rows[(u + XA) / SPT] + ((u + XA) % SPT) * 32;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) xr[(u + XA) % XR][ct] = *reinterpret_cast<const uint4*>(lds + p + ct * 2 * PSTR);
            }
            wr[(u + WR - 1) % WR] = *reinterpret_cast<const uint4*>(wb + (size_t)(g + WR - 1 < G ? g + WR - 1 : G - 1) * 1024 + lo);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct] = MFMA16(wr[u % WR], xr[u % XR][ct], acc[ct]);
            BF16_SG_MFMA(1); BF16_SG_LDS(2); BF16_SG_MFMA(1); BF16_SG_VMEM(1); BF16_SG_MFMA(1); BF16_SG_LDS(2); BF16_SG_MFMA(1);
            SB();
        }
        if (G > PASS) {
            const int t0 = (g0 + PASS) / SPT;
#pragma unroll
            for (int t = 0; t <= TPP; ++t) rows[t] = tap_row(t0 + t);
        }
    }
}

// epilogue of the 4x4 stage over eight patches: v[ct][r] = channel 32 wave + (r&3) + 8(r>>2) + 4 half of patch 2 ct + (i>>4),
// pixel i & 15.  MODE 0: BN + ReLU -> bf16 image (patches BF16_S2 apart);  1: BN + identity + ReLU -> image, identity updated;
// 2: like 1, stored as fp32 [pix][PS2] (patches BF16_SLAB apart) for the average pool
template <int MODE>
__device__ __forceinline__ void epilogue_l2_bf16(char* lds, const float* __restrict__ al, const float* __restrict__ sh,
                                              const f32x16 (&acc)[4], f32x16 (&id2)[4], int lane, int wave) {
    const int i = lane & 31, half = lane >> 5;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int ch = 32 * wave + 8 * g + 4 * half;
        const float4 A = *reinterpret_cast<const float4*>(al + ch), B = *reinterpret_cast<const float4*>(sh + ch);
        const float Aa[4] = {A.x, A.y, A.z, A.w}, Bb[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = __builtin_fmaf(acc[ct][4 * g + j], Aa[j], Bb[j]);
                if (MODE != 0) x = x + id2[ct][4 * g + j];
                x = x > 0.0f ? x : 0.0f;
                if (MODE != 0) id2[ct][4 * g + j] = x;
                v[j] = x;
            }
            if (MODE == 2)
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(lds + (2 * ct + (i >> 4)) * BF16_SLAB) + (i & 15) * PS2 + ch) =
                    make_float4(v[0], v[1], v[2], v[3]);
            else
                store_planes4<1>(lds + (2 * ct + (i >> 4)) * BF16_S2 + (i & 15) * XP2 + 2 * ch, XP2, v);
        }
    }
}

// STAMP: the diagnostic instantiation (tools/fused_stamps.py): the phase boundaries of quad q on row 8 * workgroup + 4 q +
// wave; the 4x4 stage's (stamps 11 .. 15) on both quads' rows - the SECOND quad's rows (4 .. 7 of every 8) read like those of
// a four-patch workgroup
template <bool STAMP>
__global__ __launch_bounds__(256, 2) void fused_trunk_bf16_kernel(FusedArgs a, unsigned long long* stamps) {
    extern __shared__ __attribute__((aligned(16))) char ldsx[];
#undef IPSX_STAMP
#define IPSX_STAMP(k)                                                                      \
    do {                                                                                   \
        if (STAMP) {                                                                       \
            __builtin_amdgcn_sched_barrier(0);                                             \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                    \
            if (lane == 0) stamps[((size_t)blockIdx.x * 8 + 4 * q + wave) * 16 + (k)] = t_; \
            __builtin_amdgcn_sched_barrier(0);                                             \
        }                                                                                  \
    } while (0)
#define IPSX_STAMP2(k)                                                                     \
    do {                                                                                   \
        if (STAMP) {                                                                       \
            __builtin_amdgcn_sched_barrier(0);                                             \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();                    \
            if (lane == 0) {                                                               \
                stamps[((size_t)blockIdx.x * 8 + wave) * 16 + (k)] = t_;                   \
                stamps[((size_t)blockIdx.x * 8 + 4 + wave) * 16 + (k)] = t_;               \
            }                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                             \
        }                                                                                  \
    } while (0)
    constexpr int R1 = XL<1>::R1, R2 = XL<1>::R2;
    const int lane0 = threadIdx.x & 63, wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long n_valid = a.count ? (long long)*a.count : a.n;
    const long long p_first = (long long)blockIdx.x * 8;
    if (p_first >= n_valid) return;                      // workgroup-uniform

    // ---- two quads through stem + layer1, one after the other; the 8x8 images in place
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        // (lane and wave through an opaque copy per quad: what is derived from them - tap offsets, slab addresses - is formed
        //  where it is used instead of being carried round the loop in registers the 8x8 stage does not have)
        int lane = lane0, wave = wave0;
        asm volatile("" : "+v"(lane));
        asm volatile("" : "+s"(wave));
        const int rt = wave & 1, pp = wave >> 1;
        char* const base = ldsx + 4 * q * BF16_SLAB;       // this quad's four slabs
        char* const Sb = base + wave * BF16_SLAB;          // this wave's own patch: input image, transposition scratch, hand-over
        float* const S = reinterpret_cast<float*>(Sb);
        long long pi = p_first + 4 * q + wave;
        if (pi >= n_valid) pi = n_valid - 1;             // tail: recompute a valid patch, store nothing
        if (a.index) pi = a.index[pi];
        IPSX_STAMP(0);
        {
            float4 px[4];
            bf16_fetch(a, pi, lane, px);
            for (int z = lane; z < SPLANE / 16; z += 64) reinterpret_cast<uint4*>(Sb)[z] = make_uint4(0u, 0u, 0u, 0u);
            wave_fence();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = (k * 64 + lane) * 4, y = e >> 5, x = e & 31;
                const unsigned short b0 = bf16_bits(px[k].x), b1 = bf16_bits(px[k].y), b2 = bf16_bits(px[k].z), b3 = bf16_bits(px[k].w);
                char* d = Sb + ((y + 3) * SPW + x + 3) * 2;
                *reinterpret_cast<unsigned short*>(d) = b0;
                *reinterpret_cast<unsigned*>(d + 2) = (unsigned)b1 | ((unsigned)b2 << 16);
                *reinterpret_cast<unsigned short*>(d + 6) = b3;
            }
        }
        wave_fence();
        f32x16 idn[4], acc[4];
        IPSX_STAMP(1);
        {
            f32x16 st[2][2], tr[2][2];
            stem_pool<1>(a, Sb, st, lane);
            wave_fence();                                // the input image is dead
            transpose_stem(S, st, tr, lane);
            // the other channel tile of this patch's fp32 stem output: to the pair's other wave through this slab
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[(h * 16 + r) * 64 + lane] = rt ? tr[0][h][r] : tr[1][h][r];
            __syncthreads();
            {
                const float* O = reinterpret_cast<const float*>(base + (wave ^ 1) * BF16_SLAB);
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float o = O[(h * 16 + r) * 64 + lane];
                        const float own = rt ? tr[1][h][r] : tr[0][h][r];
                        idn[h][r] = rt ? o : own;
                        idn[2 + h][r] = rt ? own : o;
                    }
            }
            __syncthreads();                             // both hand-overs are read: the slabs become images
            epilogue_l1s<1, 2>(Sb, nullptr, nullptr, tr, tr, lane);      // the patch's image, all 64 channels, in its own slab
            for (int z = lane; z < R1 / 4; z += 64) reinterpret_cast<unsigned*>(Sb + XZ1 * R1)[z] = 0u;
        }
        __syncthreads();
        IPSX_STAMP(2);
        char* const P = base + 2 * pp * BF16_SLAB;         // the pair's two slabs
#pragma unroll 1
        for (int blk = 0; blk < 2; ++blk) {
            conv_l1_bf16(a.wh[2 * blk], P, rt, acc, lane);
            IPSX_STAMP(3 + 4 * blk);
            __syncthreads();                             // every wave has read the images: overwrite them
            epilogue_l1_bf16<0>(P, a.al[2 * blk], a.sh[2 * blk], rt, acc, idn, lane);
            __syncthreads();
            IPSX_STAMP(4 + 4 * blk);
            conv_l1_bf16(a.wh[2 * blk + 1], P, rt, acc, lane);
            IPSX_STAMP(5 + 4 * blk);
            __syncthreads();
            epilogue_l1_bf16<1>(P, a.al[2 * blk + 1], a.sh[2 * blk + 1], rt, acc, idn, lane);
            __syncthreads();
            IPSX_STAMP(6 + 4 * blk);
        }
    }

    // ---- layer2 over the eight patches: wave = 32 output channels x 128 pixels
    int lane = lane0, wave = wave0;
    asm volatile("" : "+v"(lane));
    asm volatile("" : "+s"(wave));
    char* const setX = ldsx;
    char* const setY = ldsx + 8 * BF16_S2;
    f32x16 t2[4], id2[4];
    conv_l2_bf16<64, 8, R1, XZ1, 2, 3, BF16_SLAB>(a.wh[4], ldsx, t2, lane, wave);
    conv_l2_bf16<64, 8, R1, XZ1, 2, 1, BF16_SLAB>(a.wh_down, ldsx, id2, lane, wave);
    {   // projection shortcut: BatchNorm only, kept in fp32 registers
        const int half = lane >> 5;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = 32 * wave + 8 * g + 4 * half;
            const float4 A = *reinterpret_cast<const float4*>(a.a_down + ch), B = *reinterpret_cast<const float4*>(a.s_down + ch);
            const float Aa[4] = {A.x, A.y, A.z, A.w}, Bb[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int j = 0; j < 4; ++j) id2[ct][4 * g + j] = __builtin_fmaf(id2[ct][4 * g + j], Aa[j], Bb[j]);
        }
    }
    IPSX_STAMP2(11);
    __syncthreads();                                     // every wave is done with the 8x8 images: their space is the 4x4 stage's
    epilogue_l2_bf16<0>(setX, a.al[4], a.sh[4], t2, id2, lane, wave);
    for (int p = wave; p < 8; p += 4)                    // the zero (halo) rows of both sets' 4x4 images
        for (int z = lane; z < R2 / 4; z += 64) {
            reinterpret_cast<unsigned*>(setX + p * BF16_S2 + XZ2 * R2)[z] = 0u;
            reinterpret_cast<unsigned*>(setY + p * BF16_S2 + XZ2 * R2)[z] = 0u;
        }
    __syncthreads();
    conv_l2_bf16<128, 4, R2, XZ2, 1, 3, BF16_S2>(a.wh[5], setX, t2, lane, wave);
    epilogue_l2_bf16<1>(setY, a.al[5], a.sh[5], t2, id2, lane, wave);
    __syncthreads();
    IPSX_STAMP2(12);
    conv_l2_bf16<128, 4, R2, XZ2, 1, 3, BF16_S2>(a.wh[6], setY, t2, lane, wave);
    epilogue_l2_bf16<0>(setX, a.al[6], a.sh[6], t2, id2, lane, wave);
    __syncthreads();
    IPSX_STAMP2(13);
    conv_l2_bf16<128, 4, R2, XZ2, 1, 3, BF16_S2>(a.wh[7], setX, t2, lane, wave);
    __syncthreads();                                     // the fp32 images of the average pool take the whole space
    epilogue_l2_bf16<2>(ldsx, a.al[7], a.sh[7], t2, id2, lane, wave);
    __syncthreads();
    IPSX_STAMP2(14);
    for (int o = threadIdx.x; o < 8 * 128; o += 256) {
        const int pl = o >> 7, n = o & 127;
        const float* sp = reinterpret_cast<const float*>(ldsx + pl * BF16_SLAB) + n;
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum = sum + sp[k * PS2];
        if (p_first + pl < n_valid) a.emb[(size_t)(p_first + pl) * 128 + n] = sum / 16.0f;
    }
    IPSX_STAMP2(15);
}
