// dedup.hip - exact blank-patch deduplication in front of the encoder (SURVEY.md section 8 f, N-c).
//
// About 93 % of the 32-px patches of a Megapixel-MNIST image are all-zero
// (reference data/megapixel_mnist/make_mnist.py).  In eval / no-grad mode the encoder is a pure
// function of the patch (reference architecture/ips_net.py:191-193), so all blank patches share ONE
// embedding: encode the non-blank patches and a single blank one, then copy.  The result is
// bit-identical to encoding every patch (same kernel, same inputs) - this is not an approximation.
// Two routes.  Inside the one counted launch of an image batch (ipsx_trunk_encode_parts_dedup, the default there: the second
// half of this file).  And the explicit one for any call (ipsx_trunk_encode_dedup, IPSX_DEDUP_BLANK=1); everything stays on the
// device, no host synchronisation:
//   blank_flags_kernel   one wavefront per patch: is any element non-zero?        (HBM-bound, reads all patches once)
//   compact_kernel       one workgroup: ordered list of the patches to encode (non-blank ones + the first
//                        blank), its length, and for every patch the slot of its representative
//   fused trunk          launched for the worst case, workgroups beyond the device-side count exit at once
//   scatter_rows_kernel  emb[j] = emb_unique[slot[j]]
// The explicit route's shape also runs on a ragged view - whole images of different sizes, the grid patches read where they
// lie (ipsx_trunk_encode_ragged_view_dedup, the default of IPSNet.ips_image_ragged on the fused trunk): its scan and its
// many-workgroup compaction stand behind the counted launch's kernels below.

#include "ipsx_internal.h"

namespace ipsx {

__global__ __launch_bounds__(256) void blank_flags_kernel(const float* __restrict__ x, long long n, int elems4,
                                                          int* __restrict__ nonblank) {
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const uint4* p = reinterpret_cast<const uint4*>(x) + (size_t)j * elems4;
    unsigned any = 0;
    for (int i = lane; i < elems4; i += 64) {
        const uint4 v = p[i];
        any |= (v.x | v.y | v.z | v.w) & 0x7FFFFFFFu;        // -0.0 is zero too
    }
    const unsigned long long b = __ballot(any != 0);
    if (lane == 0) nonblank[j] = b != 0ull;
}

// single workgroup, ordered compaction (patch order is preserved, so results do not depend on timing)
__global__ __launch_bounds__(1024) void compact_kernel(const int* __restrict__ nonblank, int n, int* __restrict__ index,
                                                       int* __restrict__ slot, int* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int base, first_blank;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { base = 0; first_blank = 0x7FFFFFFF; }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int j = c0 + tid;
        const int f = (j < n) ? nonblank[j] : 0;
        const unsigned long long m = __ballot(f != 0);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        if (j < n && !f) atomicMin(&first_blank, j);   // value = smallest blank index, whatever the arrival order
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (f) { index[off + before] = j; slot[j] = off + before; }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; base += t; }
        __syncthreads();
    }
    // one representative for all blank patches, after the non-blank ones
    const int nb = base, fb = first_blank == 0x7FFFFFFF ? -1 : first_blank;
    if (tid == 0) {
        if (fb >= 0) index[nb] = fb;
        *count = nb + (fb >= 0 ? 1 : 0);
    }
    for (int j = tid; j < n; j += 1024)
        if (!nonblank[j]) slot[j] = nb;
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const float4* __restrict__ src, const int* __restrict__ slot,
                                                           float4* __restrict__ dst, long long n, int row4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * row4) return;
    const long long j = i / row4;
    const int c = (int)(i - j * row4);
    dst[i] = src[(size_t)slot[j] * row4 + c];
}

// ---- the same dedup inside the one counted launch (ipsx_trunk_encode_parts_dedup): no workspace of embeddings, no scatter
//   blank_scan_parts_kernel     64 list entries per workgroup: blank or not (with an early exit), the blank entries' rows
//                               written and counted into their parts, a mask and a count of the others
//   blank_scan_parts_{u8,view,view_u8}_kernel   the same scan of uint8 patches (blank: every byte 0), of grid patches of
//                               float32 images and of grid patches of uint8 images
//   blank_compact_kernel        many workgroups: the ordered list of the entries to encode, and its length
//   fused_trunk_parts_dedup_kernel (fused_trunk_eight.h)   encodes those, each to its own row, and counts them: the whole
//                               rounds of the list, or all of it (trunk_split_n8 of the length, ipsx_internal.h)
//   fused_trunk_pair_parts_dedup_kernel (fused_trunk_pair.h)   the same for the remainder of up to half a round
constexpr int SCAN_ENT = 64;          // list entries per scan workgroup: 16 wavefronts x 4
constexpr int PATCH_U4 = 256;         // a 1x32x32 float32 patch in 16-byte loads: 4 per lane

__device__ __forceinline__ unsigned nonzero_bits(const uint4& v) { return (v.x | v.y | v.z | v.w) & 0x7FFFFFFFu; }   // -0.0 is zero
__device__ __forceinline__ uint4 float4_bits(const float4& f) {
    return uint4{__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)};
}
__device__ __forceinline__ unsigned long long low_bits(int b) { return b >= 64 ? ~0ull : (1ull << b) - 1ull; }

// Does the 1x32x32 float32 window at p (its image's row pitch w floats) hold a non-zero bit?  A wavefront's question: v0 is
// the lane's share of the first KiB (patch rows 0 - 7, view_load_32 unit 0), loaded by the caller - so that several windows'
// first reads can be in flight together -, the other three are read only where that is all zero; -0.0 is zero.
__device__ __forceinline__ bool window_nonzero(const float* p, int w, int wide, int lane, const float4& v0) {
    unsigned any = nonzero_bits(float4_bits(v0));
    if (__ballot(any != 0) == 0ull) {
        float4 r[3];
        view_load_32<3>(p, w, wide, lane, 1, r);
        any = nonzero_bits(float4_bits(r[0])) | nonzero_bits(float4_bits(r[1])) | nonzero_bits(float4_bits(r[2]));
    }
    return __ballot(any != 0) != 0ull;
}
// ... of uint8 pixels: blank means every byte 0.  A lane's 16 bytes are half a patch row, contiguous in the image
// (view_load_u8: 16, 4 or 1 bytes per load by `wide`) - the whole KiB in one read per lane, nothing to exit early from
__device__ __forceinline__ void window_load_u8(const unsigned char* p, int w, int wide, unsigned (&d)[4]) {
    const int lane = threadIdx.x & 63;
    view_load_u8<4>(p + (long long)(lane >> 1) * w + 16 * (lane & 1), wide, d);
}
__device__ __forceinline__ bool window_nonzero_u8(const unsigned (&d)[4]) { return __ballot((d[0] | d[1] | d[2] | d[3]) != 0u) != 0ull; }

// List entry j is patch index[j].  A wavefront takes four entries: the first KiB of each (one 16-byte load per lane, the four
// in flight together) and, only where that is all zero, the other three.  On data without blank patches a KiB per patch is
// read.  Blank entry j: emb row j = blank_emb.  The hand-over of those rows is parts_count's (fused_trunk_eight.h): every
// storing wavefront drained, the workgroup's barrier, one lane's agent-scope release, waited for, then relaxed agent-scope adds.
__global__ __launch_bounds__(1024) void blank_scan_parts_kernel(const float* __restrict__ x, const int* __restrict__ index, int n,
                                                                const float* __restrict__ blank_emb, float* __restrict__ emb,
                                                                PartsArgs pa, unsigned long long* __restrict__ mask,
                                                                int* __restrict__ cnt) {
    __shared__ unsigned wbits[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo = blockIdx.x * SCAN_ENT, j0 = lo + wave * 4;
    const uint4* p[4];
    uint4 v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[e] = reinterpret_cast<const uint4*>(x) + (size_t)(j0 + e < n ? index[j0 + e] : 0) * PATCH_U4 + lane;
        v[e] = j0 + e < n ? p[e][0] : uint4{0u, 0u, 0u, 0u};
    }
    const float2 be = reinterpret_cast<const float2*>(blank_emb)[lane];
    unsigned bits = 0;                                                    // the wavefront's non-blank entries
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (j0 + e >= n) break;                                           // wavefront-uniform
        unsigned any = nonzero_bits(v[e]);
        if (__ballot(any != 0) == 0ull) {
            const uint4 a = p[e][64], b = p[e][128], c = p[e][192];
            any = nonzero_bits(a) | nonzero_bits(b) | nonzero_bits(c);
        }
        if (__ballot(any != 0) != 0ull) bits |= 1u << e;
        else reinterpret_cast<float2*>(emb + (size_t)(j0 + e) * 128)[lane] = be;
    }
    if (lane == 0) wbits[wave] = bits;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) m |= (unsigned long long)wbits[w] << (4 * w);
        mask[blockIdx.x] = m;
        cnt[blockIdx.x] = __popcll(m);
        const unsigned long long blank = ~m & low_bits(n - lo);
        if (blank) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int begin = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {                                // (constant indices: part_end stays in the kernel arguments)
                if (k < pa.parts) {
                    const int end = pa.part_end[k];
                    const int b0 = begin - lo, b1 = end - lo;             // the part's entries in this workgroup: bits b0 .. b1 - 1
                    const int c = b1 <= 0 || b0 >= SCAN_ENT ? 0 : __popcll(blank & low_bits(b1) & ~low_bits(b0 > 0 ? b0 : 0));
                    if (c > 0) __hip_atomic_fetch_add(pa.done + k, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    begin = end;
                }
            }
        }
    }
}

// What the three scans below do with a wavefront's answer, step for step blank_scan_parts_kernel's (which keeps its own text:
// its instruction stream is pinned): the rows of the blank ones among the wavefront's `valid` entries j0 .. (bit e of `bits`
// clear) = blank_emb, then the workgroup's mask and count and the blank entries counted into their parts, by the same
// hand-over.
__device__ __forceinline__ void scan_hand_over(unsigned bits, int valid, int j0, int lo, int n, const float* __restrict__ blank_emb,
                                               float* __restrict__ emb, const PartsArgs& pa,
                                               unsigned long long* __restrict__ mask, int* __restrict__ cnt) {
    __shared__ unsigned wbits[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2 be = reinterpret_cast<const float2*>(blank_emb)[lane];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < valid && !(bits >> e & 1u)) reinterpret_cast<float2*>(emb + (size_t)(j0 + e) * 128)[lane] = be;   // wavefront-uniform
    if (lane == 0) wbits[wave] = bits;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) m |= (unsigned long long)wbits[w] << (4 * w);
        mask[blockIdx.x] = m;
        cnt[blockIdx.x] = __popcll(m);
        const unsigned long long blank = ~m & low_bits(n - lo);
        if (blank) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int begin = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {                                // (constant indices: part_end stays in the kernel arguments)
                if (k < pa.parts) {
                    const int end = pa.part_end[k];
                    const int b0 = begin - lo, b1 = end - lo;             // the part's entries in this workgroup: bits b0 .. b1 - 1
                    const int c = b1 <= 0 || b0 >= SCAN_ENT ? 0 : __popcll(blank & low_bits(b1) & ~low_bits(b0 > 0 ? b0 : 0));
                    if (c > 0) __hip_atomic_fetch_add(pa.done + k, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    begin = end;
                }
            }
        }
    }
}

// uint8 patches (table[c][byte] is their value): an entry is blank when every BYTE is 0 - its embedding is that of a patch of
// table[c][0], the caller's blank_emb, whatever that float is.  A patch is 1,024 bytes: one 16-byte load per lane, the four
// entries of a wavefront in flight together, nothing to exit early from.
__global__ __launch_bounds__(1024) void blank_scan_parts_u8_kernel(const unsigned char* __restrict__ x, const int* __restrict__ index,
                                                                   int n, const float* __restrict__ blank_emb,
                                                                   float* __restrict__ emb, PartsArgs pa,
                                                                   unsigned long long* __restrict__ mask, int* __restrict__ cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo = blockIdx.x * SCAN_ENT, j0 = lo + wave * 4;
    uint4 v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        v[e] = j0 + e < n ? reinterpret_cast<const uint4*>(x + (size_t)index[j0 + e] * 1024)[lane] : uint4{0u, 0u, 0u, 0u};
    unsigned bits = 0;                                                    // the wavefront's non-blank entries
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (__ballot((v[e].x | v[e].y | v[e].z | v[e].w) != 0u) != 0ull) bits |= 1u << e;
    const int valid = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
    scan_hand_over(bits, valid, j0, lo, n, blank_emb, emb, pa, mask, cnt);   // (an entry beyond n: no bit, masked out there)
}

// A view of float32 images: list entry j is GRID patch index[j], its rows at pitch w in the image (view_base, view_load_32:
// 16-byte loads where va.wide allows, dwords otherwise).  The float32 scan's order: the first KiB of the four entries in
// flight together, then window_nonzero.
__global__ __launch_bounds__(1024) void blank_scan_parts_view_kernel(const float* __restrict__ x, ViewArgs va,
                                                                     const int* __restrict__ index, int n,
                                                                     const float* __restrict__ blank_emb, float* __restrict__ emb,
                                                                     PartsArgs pa, unsigned long long* __restrict__ mask,
                                                                     int* __restrict__ cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo = blockIdx.x * SCAN_ENT, j0 = lo + wave * 4;
    const int valid = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
    const float* p[4];
    float4 v[4][1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[e] = x + view_base(va, e < valid ? index[j0 + e] : 0);
        if (e < valid) view_load_32<1>(p[e], va.v.w, va.wide, lane, 0, v[e]);
        else v[e][0] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    unsigned bits = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e >= valid) break;                                            // wavefront-uniform
        if (window_nonzero(p[e], va.v.w, va.wide, lane, v[e][0])) bits |= 1u << e;
    }
    scan_hand_over(bits, valid, j0, lo, n, blank_emb, emb, pa, mask, cnt);
}

// A view of uint8 images: one window_load_u8 per entry, the four of a wavefront in flight together.
__global__ __launch_bounds__(1024) void blank_scan_parts_view_u8_kernel(const unsigned char* __restrict__ x, ViewArgs va,
                                                                        const int* __restrict__ index, int n,
                                                                        const float* __restrict__ blank_emb, float* __restrict__ emb,
                                                                        PartsArgs pa, unsigned long long* __restrict__ mask,
                                                                        int* __restrict__ cnt) {
    const int wave = threadIdx.x >> 6;
    const int lo = blockIdx.x * SCAN_ENT, j0 = lo + wave * 4;
    const int valid = n - j0 < 4 ? (n - j0 > 0 ? n - j0 : 0) : 4;
    unsigned w[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < valid) window_load_u8(x + view_base(va, index[j0 + e]), va.v.w, va.wide, w[e]);
        else w[e][0] = w[e][1] = w[e][2] = w[e][3] = 0u;
    }
    unsigned bits = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (window_nonzero_u8(w[e])) bits |= 1u << e;
    scan_hand_over(bits, valid, j0, lo, n, blank_emb, emb, pa, mask, cnt);
}

// Ordered compaction with many workgroups: a workgroup takes four scan workgroups' masks (256 entries), sums the counts of the
// scan workgroups in front of it and writes clist[p] = (j, index[j]) in list order - the trunk then has its patch number with
// one load; the one that holds the last mask writes the length.
// Sums of integers: the list depends on the data only, never on timing.
__global__ __launch_bounds__(256) void blank_compact_kernel(const unsigned long long* __restrict__ mask,
                                                            const int* __restrict__ cnt, int n_mask,
                                                            const int* __restrict__ index, int2* __restrict__ clist,
                                                            int* __restrict__ count, int* __restrict__ n_encoded) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int first = blockIdx.x * 4;
    int sum = 0;
    for (int i = threadIdx.x; i < first; i += 256) sum += cnt[i];
#pragma unroll
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    const int s = first + wave;
    if (s >= n_mask) return;
    int base = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    for (int w = 0; w < wave; ++w) base += cnt[first + w];
    const unsigned long long m = mask[s];
    if (m >> lane & 1ull) {
        const int j = s * SCAN_ENT + lane;
        clist[base + __popcll(m & ((1ull << lane) - 1ull))] = int2{j, index[j]};
    }
    if (s == n_mask - 1 && lane == 0) {
        *count = base + __popcll(m);
        if (n_encoded) *n_encoded = base + __popcll(m);
    }
}

// ---- the explicit route on a ragged view (ipsx_trunk_encode_ragged_view_dedup): images of different sizes, DESIGN 2.8
//   blank_flags_ragged_view_kernel   one wavefront per list entry: its patch resolved as the ragged stems resolve it, read
//                                    where it lies in its image
//   ragged_compact_kernel            many workgroups: the ordered list of the entries to encode as PACKED PATCH NUMBERS (the
//                                    non-blank ones, then the first blank one), its length, every entry's slot
//   fused_trunk_ragged_view_counted_kernel (fused_trunk_eight.h) over that list, then scatter_rows_kernel
// One wavefront per list entry j (wave-uniform: readfirstlane), the bisection, the table entry and the offset on scalar
// registers (ragged_at); an entry that is no packed patch is packed patch 0, as in the encoder.  The 1x32x32 window at its
// image's row pitch, asked as the counted launch's view scans ask it (window_nonzero; U8: whole uint8 images,
// window_nonzero_u8) - nothing outside the window is read.
template <bool U8>
__global__ __launch_bounds__(256) void blank_flags_ragged_view_kernel(const void* __restrict__ x, RaggedViewArgs rv, long long n,
                                                                      int* __restrict__ nonblank) {
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= n) return;                                                   // wavefront-uniform
    const RaggedAt at = ragged_at(rv, j);
    bool any;
    if constexpr (U8) {
        unsigned w[4];
        window_load_u8(static_cast<const unsigned char*>(x) + at.off, at.v.w, at.wide, w);
        any = window_nonzero_u8(w);
    } else {
        const float* p = static_cast<const float*>(x) + at.off;
        float4 v[1];
        view_load_32<1>(p, at.v.w, at.wide, lane, 0, v);
        any = window_nonzero(p, at.v.w, at.wide, lane, v[0]);
    }
    if (lane == 0) nonblank[j] = any;
}

// Ordered compaction with many workgroups: a workgroup takes 1,024 entries.  It counts the non-blank entries in front of its
// own and in the whole list and finds the first blank one by reading ALL flags (n / 1,024 workgroups x n flags out of the L2:
// 35 us at 118 k entries, profiles/ips_image_ragged_dedup_trace.txt - 0.8 % of encoding a seventh of them), then writes list[slot] = the packed patch
// number of its non-blank entries - index[j], or first + j - and slot[j] of every entry; the blank entries' slot is the one
// behind the non-blank ones, where workgroup 0 puts the first blank entry, and the length.  Sums and a minimum of integers:
// the list depends on the data only, never on timing.
__global__ __launch_bounds__(1024) void ragged_compact_kernel(const int* __restrict__ nonblank, int n, const int* __restrict__ index,
                                                              long long first, int* __restrict__ list, int* __restrict__ slot,
                                                              int* __restrict__ count) {
    __shared__ int s_before[16], s_total[16], s_blank[16], s_own[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned lo = blockIdx.x * 1024u;
    int before = 0, total = 0, blank = 0x7FFFFFFF;
    for (unsigned i = tid; i < (unsigned)n; i += 1024u) {
        const int f = nonblank[i] != 0;
        total += f;
        before += f & (i < lo);
        if (!f && blank == 0x7FFFFFFF) blank = (int)i;                    // (i grows: the thread's first blank entry)
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        before += __shfl_xor(before, o);
        total += __shfl_xor(total, o);
        const int other = __shfl_xor(blank, o);
        blank = other < blank ? other : blank;
    }
    const unsigned j = lo + tid;
    const int f = j < (unsigned)n ? nonblank[j] != 0 : 0;
    const unsigned long long m = __ballot(f != 0);
    if (lane == 0) { s_before[wave] = before; s_total[wave] = total; s_blank[wave] = blank; s_own[wave] = __popcll(m); }
    __syncthreads();
    int pos = 0, nb = 0, fb = 0x7FFFFFFF;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        pos += s_before[w] + (w < wave ? s_own[w] : 0);
        nb += s_total[w];
        fb = s_blank[w] < fb ? s_blank[w] : fb;
    }
    pos += __popcll(m & ((1ull << lane) - 1ull));
    if (j < (unsigned)n) {
        if (f) list[pos] = index ? index[j] : (int)(first + j);
        slot[j] = f ? pos : nb;
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (fb != 0x7FFFFFFF) list[nb] = index ? index[fb] : (int)(first + fb);
        *count = nb + (fb != 0x7FFFFFFF ? 1 : 0);
    }
}

// ---- the host side.  The ipsx_trunk_encode* exports themselves stand in trunk.hip, each a call of one of these.

// The workspace of the two explicit routes, in ONE place: flags, list and slots (n ints each) and the length, then - at the
// next 256-byte boundary - the n + 1 compacted rows of 128 floats.  -> the bytes the workspace exports report (they cover it:
// the rows start at most 259 bytes behind the ints, 512 are allowed for)
struct DedupWork {
    int *flags, *list, *slot, *count;
    float* rows;
};
static size_t dedup_layout(int64_t n, void* workspace, DedupWork* w) {
    if (w) {
        w->flags = static_cast<int*>(workspace); w->list = w->flags + n; w->slot = w->list + n; w->count = w->slot + n;
        w->rows = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + (((size_t)n * 12 + 4 + 255) & ~(size_t)255));
    }
    return (size_t)n * 12 + 256 + (size_t)(n + 1) * 128 * sizeof(float) + 256;
}

// The explicit route behind its entry's refusals: the flags (flags(w): made into w.flags, or the caller's own), the route's
// compaction (compact(w): list, slots and length), the trunk over the list - patch numbers of `src`, read as an index list of
// up to n entries, *count of them written -, the scatter and the copy of the length.
template <class Flags, class Compact>
static int dedup_explicit(const ipsx_trunk* t, PatchSrc src, int64_t n, float* emb, void* workspace, int32_t* n_encoded, hipStream_t s,
                          const char* what, Flags flags, Compact compact) {
    DedupWork w;
    dedup_layout(n, workspace, &w);
    IPSX_TRY(flags(w));
    IPSX_TRY(compact(w));
    src.index = w.list; src.first = 0;
    IPSX_TRY(fused_launch(t, src, n, w.rows, s, w.count));
    scatter_rows_kernel<<<dim3((unsigned)cdiv(n * 32, 256)), dim3(256), 0, s>>>(
        reinterpret_cast<const float4*>(w.rows), w.slot, reinterpret_cast<float4*>(emb), n, 32);
    IPSX_TRY(launched("scatter_rows"));
    if (n_encoded && hipMemcpyAsync(n_encoded, w.count, sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(IPSX_EHIP, "%s: count copy failed", what);
    return IPSX_OK;
}

// ipsx_trunk_encode_dedup (flags: NULL) and _flagged (flagged: the caller's flags, which must be there)
int encode_dedup(const ipsx_trunk* t, const PatchSrc& src, int64_t n_patch, const int32_t* flags, bool flagged, float* emb,
                 void* workspace, size_t workspace_bytes, int32_t* n_encoded, void* stream) {
    IPSX_REQUIRE(!flagged || flags, "trunk_encode_dedup_flagged: no flags");
    IPSX_REQUIRE(t && t->patch_dtype == 0, "trunk_encode_dedup: blank-patch detection reads float32 patches");
    IPSX_REQUIRE(t && src.base && emb && n_patch >= 0, "trunk_encode_dedup: bad arguments");
    IPSX_REQUIRE(fused_trunk_supported(t), "trunk_encode_dedup: only the fused 1x32x32 trunk is supported");
    IPSX_REQUIRE(n_patch < ((int64_t)1 << 31), "trunk_encode_dedup: too many patches");
    IPSX_TRY(patch_src_check(t, src, n_patch, true, "trunk_encode_dedup"));
    if (n_patch == 0) return IPSX_OK;
    const size_t need = ipsx_trunk_dedup_workspace_bytes(t, n_patch);
    if (!workspace || workspace_bytes < need)
        return fail(IPSX_EWORKSPACE, "trunk_encode_dedup: workspace %zu B < %zu B", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    return dedup_explicit(t, src, n_patch, emb, workspace, n_encoded, s, "trunk_encode_dedup",
        [&](const DedupWork& w) {
            if (flags) return (int)IPSX_OK;
            blank_flags_kernel<<<dim3((unsigned)cdiv(n_patch, 4)), dim3(256), 0, s>>>(static_cast<const float*>(src.base), n_patch,
                                                                                      t->c_in * t->h * t->w / 4, w.flags);
            return launched("blank_flags");
        },
        [&](const DedupWork& w) {
            compact_kernel<<<dim3(1), dim3(1024), 0, s>>>(flags ? reinterpret_cast<const int*>(flags) : w.flags, (int)n_patch, w.list,
                                                          w.slot, w.count);
            return launched("compact");
        });
}

// ---- exact blank-patch dedup inside the one counted launch
static size_t parts_dedup_masks(int64_t n_index) { return (size_t)cdiv(n_index, (int64_t)SCAN_ENT); }

// The four entries are one function of the source's kind.  Every refusal - the arguments, the trunk, the source (a byte
// source without a table, misaligned bytes, a view the trunk does not read), the parts, the workspace - comes in front of the
// scan: a refused call has written no row and no counter.
int encode_parts_dedup(const ipsx_trunk* t, const PatchSrc& src, bool u8, bool view, int64_t n_index, float* emb,
                       const int64_t* part_end, int n_parts, int32_t* done, const float* blank_emb, void* workspace,
                       size_t workspace_bytes, int32_t* n_encoded, void* stream, const char* what) {
    IPSX_REQUIRE(t && src.base && src.index && emb && part_end && done && blank_emb && (!u8 || src.table) && (!view || src.view),
                 "%s: null pointer", what);
    IPSX_REQUIRE(fused_trunk_supported(t), "%s: only the fused 1x32x32 trunk is supported", what);
    IPSX_REQUIRE(t->precision == 0 && t->patch_dtype == 0 && t->c_in * t->h * t->w == PATCH_U4 * 4,
                 "%s: blank-patch detection reads float32 or uint8 patches, on the exact fp32 trunk", what);
    PartsArgs pa;
    IPSX_TRY(parts_args(pa, n_index, part_end, n_parts, done, what));
    IPSX_TRY(parts_trunk_check(t, what));                                 // everything the trunk launch refuses: before the scan
    if (u8 || view) IPSX_TRY(patch_src_check(t, src, n_index, true, what));
    const size_t need = ipsx_trunk_parts_dedup_workspace_bytes(t, n_index);
    if (!workspace || workspace_bytes < need || !at_multiple(workspace, 8))
        return fail(IPSX_EWORKSPACE, "%s: workspace %zu B < %zu B", what, workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const int n_mask = (int)parts_dedup_masks(n_index), n = (int)n_index;
    unsigned long long* mask = static_cast<unsigned long long*>(workspace);
    int* cnt = reinterpret_cast<int*>(mask + n_mask);
    int* count = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) + (((size_t)n_mask * 12 + 255) & ~(size_t)255));
    int2* clist = reinterpret_cast<int2*>(count + 64);
    const dim3 grid((unsigned)n_mask), block(1024);
    const unsigned char* bytes = static_cast<const unsigned char*>(src.base);
    const float* floats = static_cast<const float*>(src.base);
    // the scans' load widths are the eight-patch trunk kernel's: 16-byte loads or dwords (float32 images), 16 / 4 / 1 bytes
    if (u8 && view)
        blank_scan_parts_view_u8_kernel<<<grid, block, 0, s>>>(bytes, view_args(src, {16, 4, 1}), src.index, n, blank_emb, emb, pa,
                                                               mask, cnt);
    else if (u8) blank_scan_parts_u8_kernel<<<grid, block, 0, s>>>(bytes, src.index, n, blank_emb, emb, pa, mask, cnt);
    else if (view)
        blank_scan_parts_view_kernel<<<grid, block, 0, s>>>(floats, view_args(src, {16}), src.index, n, blank_emb, emb, pa, mask, cnt);
    else blank_scan_parts_kernel<<<grid, block, 0, s>>>(floats, src.index, n, blank_emb, emb, pa, mask, cnt);
    IPSX_TRY(launched("blank_scan_parts"));
    blank_compact_kernel<<<dim3((unsigned)cdiv(n_mask, 4)), dim3(256), 0, s>>>(mask, cnt, n_mask, src.index, clist, count, n_encoded);
    IPSX_TRY(launched("blank_compact"));
    return fused_trunk_encode_parts_compact(t, src, n_index, emb, part_end, n_parts, done, clist, count, s);
}

// ---- exact blank-patch dedup on a ragged view: the explicit route's shape on plain launches
// what every entry asks of the view and the list: a valid host table (checked again), a device table, 1x32x32 windows on
// float32 pixels - or bytes (u8) -, the entries inside the packed patches (an index list: any int32 number, resolved to
// packed patch 0)
static int ragged_dedup_list_check(const void* pixels, bool u8, const ipsx_ragged_view* view, const int32_t* index, int64_t first,
                                   int64_t n, const char* what) {
    IPSX_REQUIRE(pixels && view && n >= 0 && first >= 0, "%s: bad arguments", what);
    IPSX_REQUIRE(n < ((int64_t)1 << 31), "%s: too many entries", what);
    const int64_t total = ragged_view_total(view, what);
    if (total < 0) return IPSX_EINVAL;
    IPSX_REQUIRE(view->images, "%s: no device table", what);
    IPSX_REQUIRE(view->c == 1 && view->ph == 32 && view->pw == 32, "%s: blank-patch detection reads the 1x32x32 patches of the "
                 "fused trunk, the view's are %dx%dx%d", what, view->c, view->ph, view->pw);
    IPSX_REQUIRE(u8 || at_multiple(pixels, 4), "%s: images must lie at a 4-byte address", what);
    IPSX_REQUIRE(index ? n <= 0x7FFFFFF0ll : first + n <= total, "%s: packed patches %lld .. %lld of %lld", what,
                 (long long)first, (long long)(first + n), (long long)total);
    return IPSX_OK;
}

// (u8: src.base holds bytes - the scan needs no table, so src.table does not say it)
static int ragged_blank_flags(const PatchSrc& src, bool u8, int64_t n, int32_t* nonblank, hipStream_t s) {
    RaggedViewArgs rv = ragged_view_args(src, 16);
    if (u8) rv.wide = ragged_view_load_width(src.base, *src.ragged, 1, {16, 4, 1});
    const dim3 grid((unsigned)cdiv(n, 4)), block(256);
    if (u8) blank_flags_ragged_view_kernel<true><<<grid, block, 0, s>>>(src.base, rv, n, nonblank);
    else blank_flags_ragged_view_kernel<false><<<grid, block, 0, s>>>(src.base, rv, n, nonblank);
    return launched(u8 ? "blank_flags_ragged_view_u8" : "blank_flags_ragged_view");
}

// ipsx_ragged_view_blank_flags and _u8
static int ragged_view_blank_flags(const void* pixels, bool u8, const ipsx_ragged_view* view, const int32_t* index, int64_t first,
                                   int64_t n, int32_t* nonblank, void* stream, const char* what) {
    IPSX_TRY(ragged_dedup_list_check(pixels, u8, view, index, first, n, what));
    IPSX_REQUIRE(nonblank || n == 0, "%s: no flags", what);
    if (n == 0) return IPSX_OK;
    return ragged_blank_flags(PatchSrc{pixels, nullptr, nullptr, index, index ? 0 : first, view}, u8, n, nonblank, as_stream(stream));
}

// ipsx_trunk_encode_ragged_view_dedup and _u8 (u8: the pixels are bytes and the table must be there.  The ONE blank entry is
// encoded from its image like any other - every pixel table[0] -, so no blank embedding comes in from outside)
int encode_ragged_view_dedup(const ipsx_trunk* t, const void* pixels, const float* table, bool u8, const ipsx_ragged_view* view,
                             const int32_t* index, int64_t first, int64_t n, float* emb, void* workspace, size_t workspace_bytes,
                             int32_t* n_encoded, void* stream, const char* what) {
    IPSX_REQUIRE(!u8 || table, "%s: no table", what);
    IPSX_REQUIRE(t && emb, "%s: null pointer", what);
    IPSX_TRY(ragged_dedup_list_check(pixels, u8, view, index, first, n, what));
    IPSX_REQUIRE(fused_trunk_supported(t) && t->precision == 0 && t->patch_dtype == 0 && t->c_in * t->h * t->w == PATCH_U4 * 4,
                 "%s: the exact fp32 fused 1x32x32 trunk only", what);
    const PatchSrc src{pixels, table, nullptr, index, index ? 0 : first, view};
    IPSX_TRY(patch_src_check(t, src, n, true, what));
    IPSX_TRY(parts_trunk_check(t, what));                                 // what the trunk launch refuses: before the scan
    if (n == 0) return IPSX_OK;
    const size_t need = ipsx_trunk_ragged_view_dedup_workspace_bytes(t, n);
    if (!workspace || workspace_bytes < need || !at_multiple(workspace, 16))
        return fail(IPSX_EWORKSPACE, "%s: workspace %zu B < %zu B (at a 16-byte address)", what, workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    return dedup_explicit(t, src, n, emb, workspace, n_encoded, s, what,
        [&](const DedupWork& w) { return ragged_blank_flags(src, u8, n, w.flags, s); },
        [&](const DedupWork& w) {
            ragged_compact_kernel<<<dim3((unsigned)cdiv(n, 1024)), dim3(1024), 0, s>>>(w.flags, (int)n, src.index, src.first, w.list,
                                                                                       w.slot, w.count);
            return launched("ragged_compact");
        });
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API size_t ipsx_trunk_dedup_workspace_bytes(const ipsx_trunk* t, int64_t n_patch) {
    return t && n_patch > 0 ? dedup_layout(n_patch, nullptr, nullptr) : 0;
}

IPSX_API size_t ipsx_trunk_ragged_view_dedup_workspace_bytes(const ipsx_trunk* t, int64_t n) {
    return ipsx_trunk_dedup_workspace_bytes(t, n);     // the same route, the same parts
}

IPSX_API size_t ipsx_trunk_parts_dedup_workspace_bytes(const ipsx_trunk* t, int64_t n_index) {
    if (!t || n_index <= 0) return 0;
    // the scan workgroups' masks (8 B) and counts, the length, the list of the entries to encode (8 B each)
    return parts_dedup_masks(n_index) * 12 + 256 + (size_t)n_index * 8 + 256;
}

IPSX_API int ipsx_ragged_view_blank_flags(const float* pixels, const ipsx_ragged_view* view, const int32_t* index,
                                          int64_t first, int64_t n, int32_t* nonblank, void* stream) {
    return ragged_view_blank_flags(pixels, false, view, index, first, n, nonblank, stream, "ragged_view_blank_flags");
}

IPSX_API int ipsx_ragged_view_blank_flags_u8(const uint8_t* pixels, const ipsx_ragged_view* view, const int32_t* index,
                                             int64_t first, int64_t n, int32_t* nonblank, void* stream) {
    return ragged_view_blank_flags(pixels, true, view, index, first, n, nonblank, stream, "ragged_view_blank_flags_u8");
}
