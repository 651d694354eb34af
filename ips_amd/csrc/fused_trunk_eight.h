// fused_trunk_eight.h - fused_trunk_kernel, the exact fp32 trunk's kernel for whole rounds: EIGHT patches per workgroup.
// Included by fused_trunk.hip, whose stem (trunk_front) and 32-row stage pieces (L2Tap, L2Stage, l2_loadb, l2_mma) it uses.
//
//   conv_l8                 the stride-2 3x3 convolution and the 1x1/2 projection from the 8x8 image, tiled by output row
//   the position-tiled      ONE 3x3 / stride 1 stage over a geometry trait: conv_p1 (layer1, 8x8 map, Geo8) and conv_t16
//   stage (pt_*)            (the three 128 -> 128 convolutions at 4x4, Geo4), with their epilogue loops layer1_p1, layer2_t16
//   fused_trunk_body        the kernel, and its nine __global__ entry points (storage kinds x the parts' count, and the
//                           counted launch behind the blank scan)
#pragma once

// ------------------------------------------------------------------ fused_trunk_kernel: eight patches per workgroup
// One workgroup = 8 wavefronts = 8 patches, one workgroup per compute unit: still 2 wavefronts per SIMD of 256 registers
// and 8 patches per unit per round, as two workgroups of four were.  The stem is trunk_front (wave = patch, its own
// slab); layer1 is tiled by position (conv_p1, below).  The 4x4 stage is tiled by POSITION across the eight patches: row i of an M-tile = patch i >> 2, output
// column i & 3 of ONE output row oy, so a tile is one output row of all eight patches; N = 4 tiles of 32 channels.
// Wave w owns channels 32 (w & 3) .. 32 (w & 3) + 31 and two tiles: waves 0-3 the top row (oy 0) and oy 1, waves 4-7 the
// bottom row (oy 3) and oy 2; waves w and w + 4 share a SIMD, so every SIMD issues the same MFMAs.
// For the top-row tile of the 3x3 convolution the tap row ky = 0 reads the zero padding in all 32 rows, and those taps'
// MFMAs and A-operand loads are left out: in code (a loop of its own over those taps), not by a branch.  That changes no
// bit (an accumulation chain that starts at +0 is not changed by adding fma(0, w, .) for a finite w).
// Of the 4x4 stage only the stride-2 convolution and the projection, which read the 8x8 image, run so (conv_l8); the three
// 128 -> 128 convolutions run on 16-row tiles (conv_t16, below), which leave out more.
constexpr int SLAB8 = SLAB + 12;      // floats per slab here: 4432 = 16 (mod 64 banks), so the 4 patches x 4 columns of the 16
                                      // lanes of one ds_read_b128 pass fall on 16 different 4-bank groups (SLAB: 1 - 4-way)

template <int WIN, int PS, int ZP, int STRIDE, int KS>
__device__ __forceinline__ L2Tap l8_tap(int tap, const float* S0, int oy0, int oy1, int ox) {
    constexpr int PAD = KS / 2;
    const int ky = tap / KS, kx = tap - ky * KS;
    const int ix = ox * STRIDE + kx - PAD, iy0 = oy0 * STRIDE + ky - PAD, iy1 = oy1 * STRIDE + ky - PAD;
    const bool okx = (unsigned)ix < (unsigned)WIN;
    L2Tap d;
    d.s0 = S0 + (okx && (unsigned)iy0 < (unsigned)WIN ? iy0 * WIN + ix : ZP) * PS;
    d.s1 = S0 + (okx && (unsigned)iy1 < (unsigned)WIN ? iy1 * WIN + ix : ZP) * PS;
    return d;
}

// SK0: tile 0 reads only padding at this tap - its loads and MFMAs are left out
template <int C2, bool SK0>
__device__ __forceinline__ void l8_load(L2Stage& st, const L2Tap& d) {
    if (!SK0) {
        st.a[0][0] = *reinterpret_cast<const float4*>(d.s0 + C2 * 16);
        st.a[0][1] = *reinterpret_cast<const float4*>(d.s0 + C2 * 16 + 8);
    }
    st.a[1][0] = *reinterpret_cast<const float4*>(d.s1 + C2 * 16);
    st.a[1][1] = *reinterpret_cast<const float4*>(d.s1 + C2 * 16 + 8);
}

template <bool SK0>
__device__ __forceinline__ void l8_mma(const L2Stage& st, const float4 (&b)[2], f32x16 (&acc)[2]) {
    if (!SK0) {
        l2_mma(st, b, acc);
        return;
    }
    const float a1[8] = {st.a[1][0].x, st.a[1][0].y, st.a[1][0].z, st.a[1][0].w,
                         st.a[1][1].x, st.a[1][1].y, st.a[1][1].z, st.a[1][1].w};
    const float bb[8] = {b[0].x, b[0].y, b[0].z, b[0].w, b[1].x, b[1].y, b[1].z, b[1].w};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[1] = MFMA(a1[j], bb[j], acc[1]);
}

// a stage's interleave of NM MFMAs with its NL LDS reads and 2 weight loads: L2_POST's spacing when both tiles are live;
// with tile 0 out, 8 MFMAs (the stage's own) and 2 LDS reads (the next stage's tile 1 only) - 4 in front of the first tap
// that has both tiles
template <int NM, int NL>
__device__ __forceinline__ void l8_post() {
    static_assert((NM == 16 && NL == 4) || NM == 8, "tile 0 comes in at a tap boundary and stays");
#if IPSX_SPREAD
    if constexpr (NM == 16) {
        L2_POST();
    } else if constexpr (NL == 4) {
        SG_MFMA(1); SG_LDS(1); SG_MFMA(1); SG_LDS(1); SG_MFMA(1); SG_VMEM(1); SG_MFMA(1); SG_LDS(1); SG_MFMA(1); SG_LDS(1);
        SG_MFMA(1); SG_VMEM(1); SG_MFMA(2); SB();
    } else {
        SG_MFMA(1); SG_LDS(1); SG_MFMA(2); SG_VMEM(1); SG_MFMA(1); SG_LDS(1); SG_MFMA(2); SG_VMEM(1); SG_MFMA(1); SB();
    }
#else
    SB();
#endif
}

// one tap of conv_l8 (64 input channels: 4 stages): conv_l2's stages and weight ring; SK: tile 0 is out at this tap, SKN: at
// the next one
template <int G2, bool SK, bool SKN>
__device__ __forceinline__ void l8_tap_stages(const L2Tap& cur, const L2Tap& nxt, L2Stage& sa, L2Stage& sb, float4 (&b0)[2],
                                              float4 (&b1)[2], float4 (&b2)[2], float4 (&b3)[2], const char* w, unsigned lo,
                                              int g, f32x16 (&acc)[2]) {
    constexpr int NM = SK ? 8 : 16, NL = SK ? 2 : 4, NLN = SKN ? 2 : 4;
    l8_load<1, SK>(sb, cur); l2_loadb<G2>(b2, w, lo, g + 2); L2_PRE(); l8_mma<SK>(sa, b0, acc); l8_post<NM, NL>();
    l8_load<2, SK>(sa, cur); l2_loadb<G2>(b3, w, lo, g + 3); L2_PRE(); l8_mma<SK>(sb, b1, acc); l8_post<NM, NL>();
    l8_load<3, SK>(sb, cur); l2_loadb<G2>(b0, w, lo, g + 4); L2_PRE(); l8_mma<SK>(sa, b2, acc); l8_post<NM, NL>();
    l8_load<0, SKN>(sa, nxt); l2_loadb<G2>(b1, w, lo, g + 5); L2_PRE(); l8_mma<SK>(sb, b3, acc); l8_post<NM, NLN>();
}

// conv_l2 over the eight patches of fused_trunk_kernel: acc[0] = output row OY0 (0 top, 3 bottom), acc[1] = the row next to it
// (1, 2), channels 32 nw .. 32 nw + 31.  The same k order and weight stream as conv_l2; the taps whose every row of tile 0 is
// padding - for the top row the first row of taps - run without tile 0.
template <int CIN, int WIN, int PS, int ZP, int STRIDE, int KS, int OY0>
__device__ __forceinline__ void conv_l8(const float* __restrict__ wp, const float* lds, f32x16 (&acc)[2], int lane, int nw) {
    constexpr int KGS = KS * KS * CIN / 8, G2 = KGS / 2, PER_TAP = CIN / 16, TAPS = KS * KS, PAD = KS / 2;
    static_assert(OY0 == 0 || OY0 == 3, "tile 0 is the top or the bottom output row");
    static_assert(PER_TAP == 4 && OY0 * STRIDE + KS - 1 - PAD < WIN,
                  "conv_l8 is the two convolutions that read the 8x8 image (64 channels, stride 2): no tap row lies below the map");
    constexpr int OY1 = OY0 == 0 ? 1 : 2;
    constexpr bool SKIP_FIRST = OY0 * STRIDE - PAD < 0;                    // tap row ky = 0 above the map for all of tile 0
    const int i = lane & 31, half = lane >> 5;
    const int ox = i & 3;
    const float* S0 = lds + (i >> 2) * SLAB8 + 4 * half;
    const char* w = reinterpret_cast<const char*>(wp) + (size_t)__builtin_amdgcn_readfirstlane(nw) * KGS * 1024;
    const unsigned lo = lane * 16;
    zero(acc[0]); zero(acc[1]);
    L2Tap cur = l8_tap<WIN, PS, ZP, STRIDE, KS>(0, S0, OY0, OY1, ox);
    L2Stage sa, sb;
    float4 b0[2], b1[2], b2[2], b3[2];
    l2_loadb<G2>(b0, w, lo, 0);
    l2_loadb<G2>(b1, w, lo, 1);
    l8_load<0, SKIP_FIRST>(sa, cur);
    auto tap_at = [&](int t) { return l8_tap<WIN, PS, ZP, STRIDE, KS>(t < TAPS - 1 ? t + 1 : TAPS - 1, S0, OY0, OY1, ox); };
    int tap = 0;
    if constexpr (SKIP_FIRST) {
#pragma unroll 1
        for (; tap < KS - 1; ++tap) {
            const L2Tap nxt = tap_at(tap);
            l8_tap_stages<G2, true, true>(cur, nxt, sa, sb, b0, b1, b2, b3, w, lo, tap * PER_TAP, acc);
            cur = nxt;
        }
        const L2Tap nxt = tap_at(tap);
        l8_tap_stages<G2, true, false>(cur, nxt, sa, sb, b0, b1, b2, b3, w, lo, tap * PER_TAP, acc);
        cur = nxt;
        ++tap;
    }
#pragma unroll 1
    for (; tap < TAPS; ++tap) {                                             // the taps with both tiles
        const L2Tap nxt = tap_at(tap);
        l8_tap_stages<G2, false, false>(cur, nxt, sa, sb, b0, b1, b2, b3, w, lo, tap * PER_TAP, acc);
        cur = nxt;
    }
}

// the wave's edge-row or inner-row tiles, by a wave-uniform branch
template <int CIN, int WIN, int PS, int ZP, int STRIDE, int KS>
__device__ __forceinline__ void conv_l8_rows(const float* __restrict__ wp, const float* lds, f32x16 (&acc)[2], int lane, int nw,
                                             bool bottom) {
    if (bottom) conv_l8<CIN, WIN, PS, ZP, STRIDE, KS, 3>(wp, lds, acc, lane, nw);
    else conv_l8<CIN, WIN, PS, ZP, STRIDE, KS, 0>(wp, lds, acc, lane, nw);
}

// ------------------------------------------------------------------ the position-tiled 3x3 stage: conv_p1 and conv_t16
// layer1's four convolutions (64 -> 64 at 8x8) and the three 128 -> 128 convolutions at 4x4 - all 3x3, stride 1, pad 1 - run
// over the workgroup's eight slabs tiled by POSITION: row m of an M-tile = one patch and one position slot, so a tile is a
// few pixel positions of ALL eight patches, and a wave computes the four tiles of one SET for its output channels.  A tile
// whose positions all read the zero padding at a tap leaves that tap out - in code, by a row loop whose bodies know the live
// tiles of each tap at compile time; that changes no bit.  The stage is written once (pt_*) over a geometry trait
// that holds what differs between the two maps: Geo8 (layer1) and Geo4 (the 4x4 stage), below.
enum : int { PT_ALL, PT_KY0, PT_KY2, PT_KX0, PT_KX2 };
struct PosTile {
    int pix0, s1, s2, skip;   // slot s -> pixel pix0 + (s & 1) s1 + (s >> 1) s2; the tap row or column the tile leaves out
    bool x0, xl;              // a slot sits in the first / last column and reads the zero row at kx = 0 / 2
};

// Geo8 - layer1 on v_mfma_f32_32x32x2_f32: row m of an M-tile = patch m >> 2, position slot m & 3, so a tile is four pixel
// positions of all eight patches.  The 64 positions make 16 tiles:
//   T0 T1   row 0, columns 0-3 / 4-7          leave out ky = 0 (taps 0 1 2): those rows read only the zero padding
//   B0 B1   row 7, columns 0-3 / 4-7          leave out ky = 2 (taps 6 7 8)
//   L       column 0, rows 1-4                leave out kx = 0 (taps 0 3 6)
//   R       column 7, rows 1-4                leave out kx = 2 (taps 2 5 8)
//   M50 M54 M60 M64   rows 5 and 6, columns 0-3 / 4-7     every tap (one column of lanes reads the padding at kx 0 or 2)
//   I1-I4   rows 1-4, columns 1-4;  J1 J2  rows 1-2 / 3-4, columns 5-6   interior: no tap leaves the map
// Wave w computes the 32 channels of N-tile w >> 2 for the four M-tiles of set (w + 2 (w >> 2)) & 3: T {T0 T1 I1 I2},
// B {B0 B1 I3 I4}, L {L M50 M54 J1}, R {R M60 M64 J2}.  Waves w and w + 4 share a SIMD and hold T + L, B + R, L + T or
// R + B: 960 + 1,056 MFMAs per convolution on every SIMD, 1,008 per patch where wave = patch needed 1,152.  LDS banks
// (ds_read_b128 takes 16 lanes = 4 patches x 4 slots at a time, and the patches lie 16 banks apart): the row tiles' four
// columns fall on four different 4-bank groups, J1 J2 two ways, L and R (one column) four ways - one of the wave's four
// operand reads per stage, prefetched a stage ahead.  Same k order and weight stream as conv_l1 (packed: 2 n-tiles x 72
// k-groups of 1 KiB); a stage is one k-group.
struct Geo8 {
    typedef f32x16 acc_t;
    static constexpr int W = 8, PS = PS1, ZP = ZP1, SETS = 4;
    static constexpr int ROW_BITS = 5, SLOT_BITS = 2;     // lane -> tile row lane & 31 (patch row >> 2, slot row & 3), k half lane >> 5
    static constexpr int NT = 1, REGS = 16;               // N-tiles per wave, C registers per tile
    static constexpr int KF = 8, WB = 1024;               // floats of the A operand and bytes of the weights per stage
    static constexpr bool PIN_STORE = true;               // pt_store computes its addresses per call, as pt_conv does
    __host__ __device__ static constexpr PosTile tile(int set, int t) {
        constexpr PosTile tiles[4][4] = {
            {{0, 1, 2, PT_KY0, true, false}, {4, 1, 2, PT_KY0, false, true}, {9, 1, 2, PT_ALL, false, false}, {17, 1, 2, PT_ALL, false, false}},
            {{56, 1, 2, PT_KY2, true, false}, {60, 1, 2, PT_KY2, false, true}, {25, 1, 2, PT_ALL, false, false}, {33, 1, 2, PT_ALL, false, false}},
            {{8, 8, 16, PT_KX0, true, false}, {40, 1, 2, PT_ALL, true, false}, {44, 1, 2, PT_ALL, false, true}, {13, 1, 8, PT_ALL, false, false}},
            {{15, 8, 16, PT_KX2, false, true}, {48, 1, 2, PT_ALL, true, false}, {52, 1, 2, PT_ALL, false, true}, {29, 1, 8, PT_ALL, false, false}}};
        return tiles[set][t];
    }
    __host__ __device__ static constexpr int set_of_wave(int w) { return (w + 2 * (w >> 2)) & 3; }
    __device__ __forceinline__ static acc_t mma(float a, float b, acc_t c) { return MFMA(a, b, c); }
    // C layout: reg r is tile row (r & 3) + 4 half + 8 (r >> 2), i.e. patch 2 (r >> 2) + half, slot r & 3; channel 32 n + lane & 31
    __device__ __forceinline__ static int c_patch0(int lane) { return lane >> 5; }
    __device__ __forceinline__ static int c_chan(int lane) { return lane & 31; }
    __host__ __device__ static constexpr int c_patch(int r) { return 2 * (r >> 2); }
    __host__ __device__ static constexpr int c_slot(int r) { return r & 3; }
    // a stage's interleave of NM MFMAs with its NL LDS reads and 1 weight load: the loads 2 MFMAs apart (1 when there are
    // more loads than that leaves room for), the weight load in the middle, 4 or more MFMAs at the end
    template <int G, int K, int NL>
    __device__ __forceinline__ static void groups() {
#if IPSX_SPREAD
        if constexpr (K <= NL) {
            SG_MFMA(G);
            if constexpr (K == NL / 2) SG_VMEM(1);
            else SG_LDS(1);
            groups<G, K + 1, NL>();
        }
#endif
    }
    template <int NM, int NL>
    __device__ __forceinline__ static void post() {
#if IPSX_SPREAD
        constexpr int G = (NM - 4) / (NL + 1) > 0 ? (NM - 4) / (NL + 1) : 1;
        groups<G, 0, NL>();
        SG_MFMA(NM - G * (NL + 1));
#endif
        SB();
    }
};

// Geo4 - the 4x4 stage on v_mfma_f32_16x16x4_f32: row m of an M-tile = patch m >> 1, position slot m & 1, so a tile is TWO
// pixel positions of all eight patches and the 16 positions make eight tiles:
//   TL TR   row 0, columns 0-1 / 2-3          leave out ky = 0          BL BR   row 3, columns 0-1 / 2-3    leave out ky = 2
//   LC      column 0, rows 1-2                leave out kx = 0          RC      column 3, rows 1-2          leave out kx = 2
//   I1 I2   rows 1 / 2, columns 1-2           every tap
// Wave w computes channels 32 (w & 3) .. + 31 as two 16-channel N-tiles, for set w >> 2: {TL TR LC I1} or {BL BR RC I2} -
// 27 of 36 tile-taps each, 54 of 72 in all where one output row per tile ran 30 of 36 (960 -> 864 MFMA equivalents per
// convolution and patch).  The instruction accumulates its four k slots as one fma chain in slot order (lane group
// g = lane >> 4 is slot g; ipsx_dbg_mfma16_chain, tests/test_mfma16_chain.py), so the two instructions of an aligned 8-group
// take k (0,4,1,5) and (2,6,3,7): the contract's order.  For a lane group's four k of two 8-groups to lie side by side - ONE
// ds_read_b128 per tile and 16 k, one 16-byte weight load per N-tile and 16 k - the stage's LDS images keep their channels
// permuted inside every aligned block of 16 (position t16_pos(c)); store_l8t, pt_store / pt_load and the average pool write
// and read it so, and ipsx_pack_conv_weight_tile16 packs the weights to match: per wave 72 blocks of 16 k x 2 N-tiles of
// 1 KiB; a stage is one block.
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// where channel c (mod 16) lies inside its block of 16: lane group g = (k >> 2) + 2 (k & 1) of k = c & 7 holds it, as
// component 2 (c >> 3) + ((k >> 1) & 1) of the group's float4 - [0 2 8 10 | 4 6 12 14 | 1 3 9 11 | 5 7 13 15]
__host__ __device__ constexpr int t16_pos(int c) {
    return 4 * (((c & 7) >> 2) + 2 * (c & 1)) + 2 * ((c >> 3) & 1) + ((c >> 1) & 1);
}
__host__ __device__ constexpr int t16_col(int n) { return (n & ~15) + t16_pos(n & 15); }

constexpr int T16_ID = (ZP2 + 1) * PS2;     // floats into a slab: a second 4x4 image behind the stage's own (the identity's hand-over)
static_assert(T16_ID + 16 * PS2 <= SLAB8, "the hand-over image fits the slab");

struct Geo4 {
    typedef f32x4 acc_t;
    static constexpr int W = 4, PS = PS2, ZP = ZP2, SETS = 2;
    static constexpr int ROW_BITS = 4, SLOT_BITS = 1;     // lane -> tile row lane & 15 (patch row >> 1, slot row & 1), k group lane >> 4
    static constexpr int NT = 2, REGS = 4;
    static constexpr int KF = 16, WB = 2048;
    static constexpr bool PIN_STORE = false;
    __host__ __device__ static constexpr PosTile tile(int set, int t) {
        constexpr PosTile tiles[2][4] = {
            {{0, 1, 0, PT_KY0, true, false}, {2, 1, 0, PT_KY0, false, true}, {4, 4, 0, PT_KX0, true, false}, {5, 1, 0, PT_ALL, false, false}},
            {{12, 1, 0, PT_KY2, true, false}, {14, 1, 0, PT_KY2, false, true}, {7, 4, 0, PT_KX2, false, true}, {9, 1, 0, PT_ALL, false, false}}};
        return tiles[set][t];
    }
    __host__ __device__ static constexpr int set_of_wave(int w) { return w >> 2; }
    __device__ __forceinline__ static acc_t mma(float a, float b, acc_t c) { return MFMA4(a, b, c); }
    // C layout: reg r is tile row 4 (lane >> 4) + r, i.e. patch 2 (lane >> 4) + (r >> 1), slot r & 1; channel 32 n + 16 h +
    // lane & 15 of N-tile h, at its permuted position
    __device__ __forceinline__ static int c_patch0(int lane) { return 2 * (lane >> 4); }
    __device__ __forceinline__ static int c_chan(int lane) { return t16_pos(lane & 15); }
    __host__ __device__ static constexpr int c_patch(int r) { return r >> 1; }
    __host__ __device__ static constexpr int c_slot(int r) { return r & 1; }
    // a stage's interleave of NM MFMAs with its NL LDS reads and 2 weight loads: G MFMAs in front of every load, the weight
    // loads second and fourth (second and third when there are three loads), the rest of the MFMAs at the end
    template <int G, int K, int NL>
    __device__ __forceinline__ static void groups() {
#if IPSX_SPREAD
        if constexpr (K < NL + 2) {
            SG_MFMA(G);
            if constexpr (K == 1 || K == (NL + 1 < 3 ? NL + 1 : 3)) SG_VMEM(1);
            else SG_LDS(1);
            groups<G, K + 1, NL>();
        }
#endif
    }
    template <int NM, int NL>
    __device__ __forceinline__ static void post() {
#if IPSX_SPREAD
        constexpr int G = (NM - 4) / (NL + 3) > 0 ? (NM - 4) / (NL + 3) : 1;
        groups<G, 0, NL>();
        SG_MFMA(NM - G * (NL + 2));
#endif
        SB();
    }
};

template <class G>
__host__ __device__ constexpr int pt_pix(int set, int t, int slot) {
    return G::tile(set, t).pix0 + (slot & 1) * G::tile(set, t).s1 + (slot >> 1) * G::tile(set, t).s2;
}

// the set's live tiles at tap (ky, kx) (bit t)
template <class G>
__host__ __device__ constexpr int pt_live(int set, int ky, int kx) {
    int m = 0;
    for (int t = 0; t < 4; ++t) {
        const int k = G::tile(set, t).skip;
        const bool out = (k == PT_KY0 && ky == 0) || (k == PT_KY2 && ky == 2) || (k == PT_KX0 && kx == 0) || (k == PT_KX2 && kx == 2);
        if (!out) m |= 1 << t;
    }
    return m;
}

__host__ __device__ constexpr int pt_count(int m) { return (m & 1) + (m >> 1 & 1) + (m >> 2 & 1) + (m >> 3 & 1); }

// the operand pointers of one tap row ky: p = pixel (y + ky - 1, x) for tiles with a first-column slot, else (y + ky - 1, x - 1),
// so that the other taps of the row are p plus an immediate; e = the one tap whose column leaves the map for some lanes
// (kx = 0 for first-column tiles, 2 for last-column tiles), the zero row for those lanes
struct PtRow {
    const float* p[4];
    const float* e[4];
};

template <class G, int SET>
__device__ __forceinline__ PtRow pt_row(const float* const (&P)[4], const float* Z, const bool (&ok)[4], int ky) {
    PtRow r;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const PosTile d = G::tile(SET, t);
        const float* c = P[t] + (ky - 1) * G::W * G::PS;
        r.p[t] = d.x0 ? c : c - G::PS;
        r.e[t] = d.x0 ? (ok[t] ? c - G::PS : Z) : (d.xl ? (ok[t] ? c + G::PS : Z) : c);
    }
    return r;
}

template <class G, int SET>
__device__ __forceinline__ const float* pt_src(const PtRow& r, int t, int kx) {
    const PosTile d = G::tile(SET, t);
    if (d.x0) return kx == 0 ? r.e[t] : r.p[t] + (kx - 1) * G::PS;
    if (d.xl && kx == 2) return r.e[t];
    return r.p[t] + kx * G::PS;
}

template <class G>
struct PtState {
    typename G::acc_t acc[4][G::NT];    // [tile][N-tile]
    float4 a[2][4];                     // [stage & 1][tile]: the lane's four k of the stage's KF
    float4 b[4][G::NT];                 // weight ring: slot = stage & 3, refilled 2 stages ahead; [N-tile]
};

// a stage's weights at p: one 16-byte load per N-tile, 1 KiB apart (H: a constant, so every offset is an immediate)
template <class G, int H = 0>
__device__ __forceinline__ void pt_loadb(float4 (&b)[G::NT], const char* p, unsigned lo) {
    if constexpr (H < G::NT) {
        b[H] = *reinterpret_cast<const float4*>(p + H * 1024 + lo);
        pt_loadb<G, H + 1>(b, p, lo);
    }
}

// stage ST (= 8 kx + the stage inside the tap) of a tap row like ky = KY: prefetch the next stage's operands of its live
// tiles (the next row's first when ST = 23: a row like KYN) and the weights two stages on, then this stage's MFMAs - per
// (tile, N-tile) the four instructions of its k in the contract's order, the chains interleaved
template <class G, int SET, int KY, int KYN, int ST>
__device__ __forceinline__ void pt_stages(PtState<G>& s, const PtRow& cur, const PtRow& nxt, const char* w, unsigned lo, int g0) {
    if constexpr (ST < 24) {
        constexpr int KX = ST >> 3, LIVE = pt_live<G>(SET, KY, KX);
        constexpr bool LAST = ST == 23;
        constexpr int NKX = LAST ? 0 : (ST + 1) >> 3, NCG = LAST ? 0 : (ST + 1) & 7;
        constexpr int LIVEN = LAST ? pt_live<G>(SET, KYN, 0) : pt_live<G>(SET, KY, NKX);
        constexpr int NB = (ST + 1) & 1;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (LIVEN >> t & 1)
                s.a[NB][t] = *reinterpret_cast<const float4*>(pt_src<G, SET>(LAST ? nxt : cur, t, NKX) + NCG * G::KF);
        {
            int g = g0 + ST + 2;
            g = g < 72 ? g : 71;                                            // the tail prefetches re-read the last stage's
            pt_loadb<G>(s.b[(ST + 2) & 3], w + (size_t)g * G::WB, lo);
        }
        L1_PRE();
        {
            float bb[G::NT][4];
#pragma unroll
            for (int h = 0; h < G::NT; ++h) {
                const float4& bq = s.b[ST & 3][h];
                bb[h][0] = bq.x; bb[h][1] = bq.y; bb[h][2] = bq.z; bb[h][3] = bq.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (LIVE >> t & 1) {
                        const float4& aq = s.a[ST & 1][t];
                        const float av[4] = {aq.x, aq.y, aq.z, aq.w};
#pragma unroll
                        for (int h = 0; h < G::NT; ++h) s.acc[t][h] = G::mma(av[j], bb[h][j], s.acc[t][h]);
                    }
        }
        G::template post<4 * G::NT * pt_count(LIVE), pt_count(LIVEN)>();
        pt_stages<G, SET, KY, KYN, ST + 1>(s, cur, nxt, w, lo, g0);
    }
}

// one tap row: its three taps x 8 stages; leaves cur = the next row's pointers (ky + 1, clamped: the last row's tail prefetch
// re-reads its own first operands, as conv_l1's does)
template <class G, int SET, int KY, int KYN>
__device__ __forceinline__ void pt_tap_row(PtState<G>& s, PtRow& cur, const float* const (&P)[4], const float* Z,
                                           const bool (&ok)[4], const char* w, unsigned lo, int ky) {
    const PtRow nxt = pt_row<G, SET>(P, Z, ok, ky < 2 ? ky + 1 : 2);
    pt_stages<G, SET, KY, KYN, 0>(s, cur, nxt, w, lo, ky * 24);
    cur = nxt;
}

// conv3x3 (stride 1, pad 1) of the stage over the workgroup's eight slabs: acc[t][h] = tile t of set SET, N-tile h of the
// wave's channels 32 n .. 32 n + 31.  wp: the stage's weight stream, per 32 channels 72 stages of WB bytes.
template <class G, int SET>
__device__ __forceinline__ void pt_conv(const float* __restrict__ wp, const float* lds, typename G::acc_t (&acc)[4][G::NT], int lane,
                                        int n) {
    int m = lane & ((1 << G::ROW_BITS) - 1);
    asm volatile("" : "+v"(m));            // the addresses below are computed per call, not kept live across the stage
    const int slot = m & ((1 << G::SLOT_BITS) - 1);
    const float* S0 = lds + (m >> G::SLOT_BITS) * SLAB8 + 4 * (lane >> G::ROW_BITS);
    const float* Z = S0 + G::ZP * G::PS;
    const float* P[4];
    bool ok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const PosTile d = G::tile(SET, t);
        const int pix = d.pix0 + (slot & 1) * d.s1 + (slot >> 1) * d.s2;
        P[t] = S0 + pix * G::PS;
        ok[t] = d.x0 ? (pix & (G::W - 1)) != 0 : (pix & (G::W - 1)) != G::W - 1;
    }
    const char* w = reinterpret_cast<const char*>(wp) + (size_t)__builtin_amdgcn_readfirstlane(n) * 72 * G::WB;
    const unsigned lo = lane * 16;
    PtState<G> s;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < G::NT; ++h)
#pragma unroll
            for (int r = 0; r < G::REGS; ++r) s.acc[t][h][r] = 0.0f;
    pt_loadb<G>(s.b[0], w, lo);
    pt_loadb<G>(s.b[1], w + G::WB, lo);
    PtRow cur = pt_row<G, SET>(P, Z, ok, 0);
    constexpr int LIVE0 = pt_live<G>(SET, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (LIVE0 >> t & 1) s.a[0][t] = *reinterpret_cast<const float4*>(pt_src<G, SET>(cur, t, 0));
    // the three tap rows; rows with the same live tiles share a body
    if constexpr (SET == 0) {                                               // row ky = 0 without the top tiles, rows 1 and 2 alike
        pt_tap_row<G, SET, 0, 1>(s, cur, P, Z, ok, w, lo, 0);
#pragma unroll 1
        for (int ky = 1; ky < 3; ++ky) pt_tap_row<G, SET, 1, 1>(s, cur, P, Z, ok, w, lo, ky);
    } else if constexpr (SET == 1 && G::SETS == 4) {                        // layer1's B: row ky = 2 without B0 B1
        pt_tap_row<G, SET, 0, 1>(s, cur, P, Z, ok, w, lo, 0);
        pt_tap_row<G, SET, 1, 2>(s, cur, P, Z, ok, w, lo, 1);
        pt_tap_row<G, SET, 2, 2>(s, cur, P, Z, ok, w, lo, 2);
    } else if constexpr (SET == 1) {  // the 4x4 stage's: rows 0 and 1 alike - row 1's tail prefetches BL BR for row 2 too, unused (inside the slab)
#pragma unroll 1
        for (int ky = 0; ky < 2; ++ky) pt_tap_row<G, SET, 0, 0>(s, cur, P, Z, ok, w, lo, ky);
        pt_tap_row<G, SET, 2, 2>(s, cur, P, Z, ok, w, lo, 2);
    } else {                                                                // layer1's L, R: a column of taps out in every row
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) pt_tap_row<G, SET, 1, 1>(s, cur, P, Z, ok, w, lo, ky);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < G::NT; ++h) acc[t][h] = s.acc[t][h];
}

// layer1: 64 -> 64 at 8x8, acc[t][0] = tile t, channels 32 nt .. + 31; the 4x4 stage: 128 -> 128, acc[t][h] = tile t, channels
// 32 nw + 16 h .. + 15
template <int SET>
__device__ __forceinline__ void conv_p1(const float* __restrict__ wp, const float* lds, f32x16 (&acc)[4][1], int lane, int nt) {
    pt_conv<Geo8, SET>(wp, lds, acc, lane, nt);
}
template <int SET>
__device__ __forceinline__ void conv_t16(const float* __restrict__ wp, const float* lds, f32x4 (&acc)[4][2], int lane, int nw) {
    pt_conv<Geo4, SET>(wp, lds, acc, lane, nw);
}

// the wave's four tiles <-> an image of the stage at `lds` (the slabs' [pix][c] layout; lds + T16_ID: the 4x4 stage's
// hand-over image), by the trait's C layout
template <class G, int SET>
__device__ __forceinline__ void pt_store(float* lds, const typename G::acc_t (&v)[4][G::NT], int lane, int n) {
    int o = G::c_patch0(lane) * SLAB8 + 32 * n + G::c_chan(lane);
    if constexpr (G::PIN_STORE) asm volatile("" : "+v"(o));
    float* base = lds + o;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < G::NT; ++h)
#pragma unroll
            for (int r = 0; r < G::REGS; ++r)
                base[G::c_patch(r) * SLAB8 + pt_pix<G>(SET, t, G::c_slot(r)) * G::PS + 16 * h] = v[t][h][r];
}

template <class G, int SET>
__device__ __forceinline__ void pt_load(const float* lds, typename G::acc_t (&v)[4][G::NT], int lane, int n) {
    const float* base = lds + G::c_patch0(lane) * SLAB8 + 32 * n + G::c_chan(lane);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < G::NT; ++h)
#pragma unroll
            for (int r = 0; r < G::REGS; ++r)
                v[t][h][r] = base[G::c_patch(r) * SLAB8 + pt_pix<G>(SET, t, G::c_slot(r)) * G::PS + 16 * h];
}

// write conv_l8's 2 tiles as a 4x4 image of the 16-row stage (channels permuted), at `lds` or at lds + T16_ID: C reg r is
// tile row (r & 3) + 4 half + 8 (r >> 2), i.e. patch 2 (r >> 2) + half, column r & 3
__device__ __forceinline__ void store_l8t(float* lds, const f32x16 (&v)[2], int lane, int nw, int oy0, int oy1) {
    const int i = lane & 31, half = lane >> 5;
    const int n = t16_col(32 * nw + i);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pl = 2 * (r >> 2) + half, pix = (mt ? oy1 : oy0) * 4 + (r & 3);
            lds[pl * SLAB8 + pix * PS2 + n] = v[mt][r];
        }
}

// The two epilogue loops stay two functions over the shared stage: they differ in the weights' field, the channels a lane
// holds, the stamps and which convolutions add the identity, and sharing even the BatchNorm arithmetic between them makes the
// compiler emit another kernel (its branches merge differently).
//
// block 0's second convolution and block 1 of layer2 for the wave's set: the slabs hold conv1's output (permuted) and the
// projected identity at T16_ID on entry, layer2's output (permuted) on return
template <bool STAMP, int SET>
__device__ __forceinline__ void layer2_t16(const FusedArgs& a, float* lds, int lane, int wave, unsigned long long* stamps) {
    constexpr int WPB = 8;
    const int nw = wave & 3;
    const int n0 = 32 * nw + (lane & 15);
    f32x4 idn[4][2], acc[4][2];
    pt_load<Geo4, SET>(lds + T16_ID, idn, lane, nw);
#pragma unroll 1
    for (int cv = 5; cv < 8; ++cv) {
        conv_t16<SET>(static_cast<const float*>(a.wh[cv]), lds, acc, lane, nw);
        const float A[2] = {a.al[cv][n0], a.al[cv][n0 + 16]}, B[2] = {a.sh[cv][n0], a.sh[cv][n0 + 16]};
        if (cv == 6) {                                                      // block 1 conv1: BN + ReLU only
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = __builtin_fmaf(acc[t][h][r], A[h], B[h]);
                        acc[t][h][r] = v > 0.0f ? v : 0.0f;
                    }
        } else {                                                            // conv2 -> BN -> += identity -> ReLU
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = __builtin_fmaf(acc[t][h][r], A[h], B[h]);
                        v = v + idn[t][h][r];
                        idn[t][h][r] = v > 0.0f ? v : 0.0f;
                    }
        }
        __syncthreads();                                                    // every wave has read this convolution's input
        if (cv == 6) pt_store<Geo4, SET>(lds, acc, lane, nw);
        else pt_store<Geo4, SET>(lds, idn, lane, nw);
        __syncthreads();
        IPSX_STAMP(7 + cv);
    }
}

// layer1 of fused_trunk_kernel (two BasicBlocks at 8x8) for the wave's set; the slabs hold the stem's output on entry and
// layer1's on return.  Every convolution reads all eight slabs, so its epilogue writes in place between two barriers.
template <bool STAMP, int SET>
__device__ __forceinline__ void layer1_p1(const FusedArgs& a, float* lds, int lane, int wave, unsigned long long* stamps) {
    constexpr int WPB = 8;                                                  // stamp rows: fused_trunk_kernel's eight waves
    const int nt = wave >> 2, n = 32 * nt + (lane & 31);
    f32x16 idn[4][1], acc[4][1];
    pt_load<Geo8, SET>(lds, idn, lane, nt);                                     // identity of block 1
#pragma unroll 1
    for (int cv = 0; cv < 4; ++cv) {
        conv_p1<SET>(a.w[cv], lds, acc, lane, nt);
        IPSX_STAMP(3 + 2 * cv);
        const float A = a.al[cv][n], B = a.sh[cv][n];
        if ((cv & 1) == 0) {                                                // conv1 -> BN -> ReLU
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = __builtin_fmaf(acc[t][0][r], A, B);
                    acc[t][0][r] = v > 0.0f ? v : 0.0f;
                }
        } else {                                                            // conv2 -> BN -> += identity -> ReLU
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = __builtin_fmaf(acc[t][0][r], A, B);
                    v = v + idn[t][0][r];
                    idn[t][0][r] = v > 0.0f ? v : 0.0f;
                }
        }
        __syncthreads();                                                    // every wave has read this convolution's input
        if (cv & 1) pt_store<Geo8, SET>(lds, idn, lane, nt);
        else pt_store<Geo8, SET>(lds, acc, lane, nt);
        __syncthreads();
        IPSX_STAMP(4 + 2 * cv);
    }
}

// PARTS (ipsx_trunk_encode_parts; PartsArgs: ipsx_internal.h).
// Entries [lo, hi) of the list are stored by this workgroup: make them visible, then count them into their parts.
// The hand-over: every storing wavefront drains its stores, the workgroup meets, ONE thread releases at agent scope (the
// write-back of this XCD's L2 - per-XCD L2s are not coherent) and only then adds, relaxed, at agent scope.  The explicit
// waits are inline assembly on purpose: the compiler may drop the wait behind the write-back when it believes the
// wavefront's memory counter empty, and the add must not overtake it.
__device__ __forceinline__ void parts_count(const PartsArgs& pa, int lo, int hi) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int begin = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {                                    // (constant indices: part_end stays in the kernel arguments)
            if (k < pa.parts) {
                const int end = pa.part_end[k];
                const int c = (hi < end ? hi : end) - (lo > begin ? lo : begin);
                if (c > 0) __hip_atomic_fetch_add(pa.done + k, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                begin = end;
            }
        }
    }
}

// The same hand-over behind the blank scan (COMPACT): this workgroup stored the rows of the list entries js[0 .. 7] - increasing,
// anywhere in the list, -1: none - and counts each into the part its ORIGINAL position lies in.  (E = 2: the pair workgroups of
// fused_trunk_pair_parts_dedup_kernel, their two rows.)
template <int E = 8>
__device__ __forceinline__ void parts_count_compact(const PartsArgs& pa, const int* js) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int j[E];
#pragma unroll
        for (int e = 0; e < E; ++e) j[e] = js[e];
        int begin = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {                                    // (constant indices: part_end stays in the kernel arguments)
            if (k < pa.parts) {
                const int end = pa.part_end[k];
                int c = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) c += j[e] >= begin && j[e] < end;
                if (c > 0) __hip_atomic_fetch_add(pa.done + k, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                begin = end;
            }
        }
    }
}

__device__ __forceinline__ int* compact_rows() {
    __shared__ int js[8];
    return js;
}

// COMPACT (fused_trunk_parts_dedup_kernel only): workgroup b takes the entries clist[8 b .. 8 b + 7] below *a.count of the
// call's list.  clist[p] = (j, a.index[j]): patch .y -> emb row j = .x.  The rows are kept in LDS (32 bytes beside the slabs)
// for the store and the count at the end, so that nothing there waits for memory again.  Only the first n8 entries are this
// launch's (trunk_split_n8 of the count, ipsx_internal.h: whole rounds, or all of them); the pair launch behind takes the rest.
// VA: as in trunk_front
template <bool STAMP, bool U8, bool PARTS = false, bool VIEW = false, bool COMPACT = false, class VA = ViewArgs>
__device__ __forceinline__ void fused_trunk_body(const FusedArgs& a, unsigned long long* stamps, const float* table,
                                                 const PartsArgs* pa = nullptr, const typename as_given<VA>::type* va = nullptr,
                                                 const int2* __restrict__ clist = nullptr, int cus = 0, int pair_mode = 0) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // 8 slabs of SLAB8
    constexpr int WPB = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31;
    const long long p_first = (long long)blockIdx.x * 8;
    const long long n_valid = a.count ? (long long)*a.count : a.n;        // compacted launches read their length on device
    if constexpr (COMPACT) {
        if (p_first >= trunk_split_n8(n_valid, cus, pair_mode)) return;   // workgroup-uniform
    } else if (p_first >= n_valid) return;                                // workgroup-uniform
    long long pi = p_first + wave;
    if (pi >= n_valid) pi = n_valid - 1;                                  // tail: recompute a valid patch, store nothing
    int* js = nullptr;                                                    // COMPACT: the eight rows this workgroup stores
    if constexpr (COMPACT) {
        js = compact_rows();
        const int2 e = clist[pi];
        if (lane == 0) js[wave] = p_first + wave < n_valid ? e.x : -1;    // (read behind layer1's barriers)
        pi = e.y;
    } else if (a.index) pi = a.index[pi];
    else if constexpr (VIEW) pi += va->first;
    trunk_front<STAMP, WPB, U8, VIEW, VA>(a, pi, lds + wave * SLAB8, lane, wave, stamps, table, va);
    switch (__builtin_amdgcn_readfirstlane(Geo8::set_of_wave(wave))) {   // the wave's layer1 tile set, see Geo8
        case 0: layer1_p1<STAMP, 0>(a, lds, lane, wave, stamps); break;
        case 1: layer1_p1<STAMP, 1>(a, lds, lane, wave, stamps); break;
        case 2: layer1_p1<STAMP, 2>(a, lds, lane, wave, stamps); break;
        default: layer1_p1<STAMP, 3>(a, lds, lane, wave, stamps); break;
    }

    // ---- layer2 block 0: conv3x3/2 (64->128) and the 1x1/2 projection read the 8x8 stage
    const int nw = wave & 3;
    const bool bottom = __builtin_amdgcn_readfirstlane(wave) >= 4;        // wave-uniform: tiles oy 3 + 2, else 0 + 1
    const int oy0 = bottom ? 3 : 0, oy1 = bottom ? 2 : 1;
    const int n2 = 32 * nw + i;
    f32x16 t2[2], id2[2];
    conv_l8_rows<64, 8, PS1, ZP1, 2, 3>(a.w[4], lds, t2, lane, nw, bottom);
    conv_l8_rows<64, 8, PS1, ZP1, 2, 1>(a.w_down, lds, id2, lane, nw, bottom);
    IPSX_STAMP(11);
    {
        const float A = a.al[4][n2], B = a.sh[4][n2], Ad = a.a_down[n2], Bd = a.s_down[n2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = __builtin_fmaf(t2[mt][r], A, B);
                t2[mt][r] = v > 0.0f ? v : 0.0f;
                id2[mt][r] = __builtin_fmaf(id2[mt][r], Ad, Bd);
            }
    }
    __syncthreads();
    store_l8t(lds, t2, lane, nw, oy0, oy1);
    store_l8t(lds + T16_ID, id2, lane, nw, oy0, oy1);                     // the identity, into the 16-row tiles' registers below
    for (int z = lane; z < PS2; z += 64) lds[wave * SLAB8 + ZP2 * PS2 + z] = 0.0f;  // zero pixel row of the 4x4 stage
    __syncthreads();
    // conv2 of block 0, then block 1 (conv1, conv2), all 128->128 at 4x4, on 16-row tiles
    if (bottom) layer2_t16<STAMP, 1>(a, lds, lane, wave, stamps);
    else layer2_t16<STAMP, 0>(a, lds, lane, wave, stamps);

    // ---- global average pool over the 16 pixels, sequential order
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int o = threadIdx.x + 512 * h;
        const int pl = o >> 7, n = o & 127;
        const float* s = lds + pl * SLAB8 + t16_col(n);                   // the stage's channel permutation, undone
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum = sum + s[k * PS2];
        if constexpr (COMPACT) {
            if (p_first + pl < n_valid) a.emb[(size_t)js[pl] * 128 + n] = sum / 16.0f;
        } else {
            if (p_first + pl < n_valid) a.emb[(size_t)(p_first + pl) * 128 + n] = sum / 16.0f;
        }
    }
    IPSX_STAMP(15);
    if constexpr (PARTS) {
        const long long p_end = p_first + 8 < n_valid ? p_first + 8 : n_valid;
        if constexpr (COMPACT) parts_count_compact(*pa, js);
        else parts_count(*pa, (int)p_first, (int)p_end);
    }
}

template <bool STAMP>
__global__ __launch_bounds__(512, 1) void fused_trunk_kernel(FusedArgs a, unsigned long long* stamps) {
    fused_trunk_body<STAMP, false>(a, stamps, nullptr);
}

// the same, counting its patches into the parts of the call (PartsArgs)
__global__ __launch_bounds__(512, 1) void fused_trunk_parts_kernel(FusedArgs a, PartsArgs pa) {
    fused_trunk_body<false, false, true>(a, nullptr, nullptr, &pa);
}

// the same on uint8 patches (a.patches: bytes; table: 256 floats) - only the input load differs (trunk_front)
__global__ __launch_bounds__(512, 1) void fused_trunk_u8_kernel(FusedArgs a, const float* table) {
    fused_trunk_body<false, true>(a, nullptr, table);
}

// the same reading its patches through a patch-grid view (a.patches: whole images) - only the input load differs (trunk_front)
__global__ __launch_bounds__(512, 1) void fused_trunk_view_kernel(FusedArgs a, ViewArgs va) {
    fused_trunk_body<false, false, false, true>(a, nullptr, nullptr, nullptr, &va);
}

// ... through a view of whole uint8 images (a.patches: bytes; table: 256 floats)
__global__ __launch_bounds__(512, 1) void fused_trunk_view_u8_kernel(FusedArgs a, const float* table, ViewArgs va) {
    fused_trunk_body<false, true, false, true>(a, nullptr, table, nullptr, &va);
}

// ... through a ragged view (a.patches: the packed buffer of images of different sizes; the list travels in rv.index, a.index
// and a.count are NULL): the wavefront (= patch) resolves its patch - the body's own number, tail included - on scalar
// registers, the body stages it as the view kernel does
__global__ __launch_bounds__(512, 1) void fused_trunk_ragged_view_kernel(FusedArgs a, RaggedViewArgs rv) {
    long long j = (long long)blockIdx.x * 8 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= a.n) j = a.n - 1;
    const RaggedAt at = ragged_at(rv, j);
    fused_trunk_body<false, false, false, true, false, RaggedAt>(a, nullptr, nullptr, nullptr, &at);
}

// ... behind the blank scan of a ragged view (ipsx_trunk_encode_ragged_view_dedup, dedup.hip): rv.index is the compacted list,
// of which only the first *a.count entries are written - a workgroup beyond the count returns BEFORE it resolves a patch, so
// nothing reads the list's tail; the body reads the same count for its own tail rule
__global__ __launch_bounds__(512, 1) void fused_trunk_ragged_view_counted_kernel(FusedArgs a, RaggedViewArgs rv) {
    const long long n_valid = *a.count;
    if ((long long)blockIdx.x * 8 >= n_valid) return;                     // workgroup-uniform
    long long j = (long long)blockIdx.x * 8 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= n_valid) j = n_valid - 1;
    const RaggedAt at = ragged_at(rv, j);
    fused_trunk_body<false, false, false, true, false, RaggedAt>(a, nullptr, nullptr, nullptr, &at);
}

// ... through a ragged view of whole uint8 images (a.patches: the packed bytes; table: 256 floats): the patch resolved as in
// fused_trunk_ragged_view_kernel, staged as in fused_trunk_view_u8_kernel (rv.wide: 16, 4 or 1 bytes per load)
__global__ __launch_bounds__(512, 1) void fused_trunk_ragged_view_u8_kernel(FusedArgs a, const float* table, RaggedViewArgs rv) {
    long long j = (long long)blockIdx.x * 8 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= a.n) j = a.n - 1;
    const RaggedAt at = ragged_at(rv, j);
    fused_trunk_body<false, true, false, true, false, RaggedAt>(a, nullptr, table, nullptr, &at);
}

// ... behind the blank scan of a ragged view of uint8 images (ipsx_trunk_encode_ragged_view_dedup_u8), as
// fused_trunk_ragged_view_counted_kernel: nothing reads the list beyond *a.count
__global__ __launch_bounds__(512, 1) void fused_trunk_ragged_view_counted_u8_kernel(FusedArgs a, const float* table,
                                                                                   RaggedViewArgs rv) {
    const long long n_valid = *a.count;
    if ((long long)blockIdx.x * 8 >= n_valid) return;                     // workgroup-uniform
    long long j = (long long)blockIdx.x * 8 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= n_valid) j = n_valid - 1;
    const RaggedAt at = ragged_at(rv, j);
    fused_trunk_body<false, true, false, true, false, RaggedAt>(a, nullptr, table, nullptr, &at);
}

__global__ __launch_bounds__(512, 1) void fused_trunk_parts_view_kernel(FusedArgs a, PartsArgs pa, ViewArgs va) {
    fused_trunk_body<false, false, true, true>(a, nullptr, nullptr, &pa, &va);
}

// the counted launch on uint8 patches and on whole uint8 images: the uint8 kernels' staging, the parts' count at the end
__global__ __launch_bounds__(512, 1) void fused_trunk_parts_u8_kernel(FusedArgs a, PartsArgs pa, const float* table) {
    fused_trunk_body<false, true, true>(a, nullptr, table, &pa);
}

__global__ __launch_bounds__(512, 1) void fused_trunk_parts_view_u8_kernel(FusedArgs a, PartsArgs pa, const float* table,
                                                                          ViewArgs va) {
    fused_trunk_body<false, true, true, true>(a, nullptr, table, &pa, &va);
}

// the counted launch behind the blank scan (dedup.hip): the entries clist[0 .. n8) of the list only, n8 <= *a.count
__global__ __launch_bounds__(512, 1) void fused_trunk_parts_dedup_kernel(FusedArgs a, PartsArgs pa, const int2* clist, int cus,
                                                                        int pair_mode) {
    fused_trunk_body<false, false, true, false, true>(a, nullptr, nullptr, &pa, nullptr, clist, cus, pair_mode);
}

// ... on uint8 patches, on a view of float32 images and on a view of uint8 images: clist[p].y is the patch - or GRID patch -
// number as it stands (the COMPACT arm of fused_trunk_body never adds va->first), the input load is the kind's (trunk_front)
__global__ __launch_bounds__(512, 1) void fused_trunk_parts_dedup_u8_kernel(FusedArgs a, PartsArgs pa, const int2* clist, int cus,
                                                                           int pair_mode, const float* table) {
    fused_trunk_body<false, true, true, false, true>(a, nullptr, table, &pa, nullptr, clist, cus, pair_mode);
}

__global__ __launch_bounds__(512, 1) void fused_trunk_parts_dedup_view_kernel(FusedArgs a, PartsArgs pa, const int2* clist, int cus,
                                                                             int pair_mode, ViewArgs va) {
    fused_trunk_body<false, false, true, true, true>(a, nullptr, nullptr, &pa, &va, clist, cus, pair_mode);
}

__global__ __launch_bounds__(512, 1) void fused_trunk_parts_dedup_view_u8_kernel(FusedArgs a, PartsArgs pa, const int2* clist,
                                                                                int cus, int pair_mode, const float* table,
                                                                                ViewArgs va) {
    fused_trunk_body<false, true, true, true, true>(a, nullptr, table, &pa, &va, clist, cus, pair_mode);
}
