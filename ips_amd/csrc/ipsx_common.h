// ipsx_common.h - host-side helpers shared by the translation units of libipsx.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ipsx.h"

#define IPSX_API extern "C" __attribute__((visibility("default")))

namespace ipsx {

// thread-local message of the last failing call (ipsx_last_error)
char* err_buf();
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// after a kernel launch: report a launch error without synchronising
static inline int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IPSX_EHIP, "%s: %s", what, hipGetErrorString(e));
    return IPSX_OK;
}

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// (a padded map smaller than the kernel has NO output: C's division rounds (in + 2p - k) / s towards zero, which made it 1
//  under stride >= 2 - a window hanging over the far edge, accepted by every "empty output" gate)
static inline int conv_out(int in, int k, int s, int p) { return in + 2 * p < k ? 0 : (in + 2 * p - k) / s + 1; }

// ---- patch-grid view (ipsx_patch_view): the stems read their patches straight from the (b, c, h, w) images
// Element offset of patch p's (channel 0, row 0, column 0) inside the images; -1 for a geometry that has no patches, more than
// 2^31 - 1 of them, or a p outside [0, b * ny * nx).  ONE definition for the host export ipsx_patch_view_offset and the
// kernels' address arithmetic.  Element (ch, y, x) of the patch lies at offset + (ch * h + y) * w + x.
__host__ __device__ inline long long patch_view_offset(const ipsx_patch_view& v, long long p) {
    if (v.b <= 0 || v.c <= 0 || v.ph <= 0 || v.pw <= 0 || v.sh <= 0 || v.sw <= 0 || v.ph > v.h || v.pw > v.w) return -1;
    const unsigned ny = (unsigned)((v.h - v.ph) / v.sh + 1), nx = (unsigned)((v.w - v.pw) / v.sw + 1);
    const unsigned long long total = (unsigned long long)v.b * ny * nx;
    if (total > 0x7FFFFFFFull || p < 0 || (unsigned long long)p >= total) return -1;
    const unsigned up = (unsigned)p, r = up / nx, px = up - r * nx, bi = r / ny, py = r - bi * ny;
    return (((long long)bi * v.c) * v.h + (long long)py * v.sh) * v.w + (long long)px * v.sw;
}

// what a view kernel gets beside its usual arguments: patch j of the launch is grid patch index[j] (index: device int32) or
// first + j; wide: the launch's load width in bytes, picked by the host (view_args, ipsx_internal.h) - 0 where no width of
// the kernel's list fits (the float kernels' dword loads)
struct ViewArgs {
    ipsx_patch_view v;
    const int* index;
    long long first;
    int wide;
};

// a patch number that is no patch of the grid (a bad index list) reads patch 0: never outside the images
__device__ __forceinline__ long long view_base(const ViewArgs& va, long long p) {
    const long long off = patch_view_offset(va.v, p);
    return off < 0 ? 0 : off;
}

// ---- ragged patch-grid view (ipsx_ragged_view): images of DIFFERENT sizes in one packed buffer, one table entry each
// The image of packed patch p - the largest bi with images[bi].first <= p - by bisection, as patchify_sparse_kernel finds
// the image of a non-zero.  0 <= p is the caller's; a p behind the last grid lands in the last image and fails its range test.
__host__ __device__ inline int ragged_view_image(const ipsx_image_entry* im, int b, long long p) {
    int lo = 0, hi = b;                               // im[lo].first <= p < im[hi].first
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (im[mid].first <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// Element offset of packed patch p's (channel 0, row 0, column 0) inside the packed buffer, with the row pitch *w and the
// image height *h of ITS image (channel pitch h * w); -1 - and nothing written - for a p outside [0, total).  ONE definition
// for the host export ipsx_ragged_view_offset and the kernels' address arithmetic: elem_off of the image plus what
// patch_view_offset gives for the image's own one-image view.
__host__ __device__ inline long long ragged_view_offset(const ipsx_image_entry* im, int b, int sh, int sw, long long p, int* w, int* h) {
    if (b <= 0 || p < 0) return -1;
    const ipsx_image_entry e = im[ragged_view_image(im, b, p)];
    const long long local = p - e.first;
    if (local < 0 || e.nx <= 0 || local >= (long long)e.ny * e.nx) return -1;
    const unsigned ul = (unsigned)local, py = ul / (unsigned)e.nx, px = ul - py * (unsigned)e.nx;
    *w = e.w; *h = e.h;
    return e.elem_off + ((long long)py * sh) * e.w + (long long)px * sw;
}

// what a ragged view kernel gets beside its usual arguments: the device table, and patch j of the launch is packed patch
// index[j] (device int32) or first + j; wide as in ViewArgs, picked by the host that filled the table
struct RaggedViewArgs {
    const ipsx_image_entry* images;
    int b, sh, sw;
    const int* index;
    long long first;
    int wide;
};

// ... resolved for ONE patch: what the stems' staging code reads of a ViewArgs - the patch's first pixel in place of its
// number (view_base below), the pitches of its image in v.w / v.h.  The bodies are templated on the type.
struct RaggedAt {
    struct { int h, w; } v;
    const int* index;
    long long first;
    int wide;
    long long off;
};
__device__ __forceinline__ long long view_base(const RaggedAt& at, long long) { return at.off; }

// in a template's parameter list: the argument is not deduced from (the bodies' `va` defaults to nullptr)
template <class T> struct as_given { using type = T; };

#ifdef __HIPCC__
// launch patch j (wave-uniform; the caller hands the same j to every lane) of a ragged view, on scalar registers: the packed
// number is made uniform for the compiler, the bisection and the entry are scalar loads.  A number that is no packed patch
// (a bad index list) reads packed patch 0: never outside the buffer.
__device__ __forceinline__ RaggedAt ragged_at(const RaggedViewArgs& rv, long long j) {
    const long long q = rv.index ? (long long)rv.index[j] : rv.first + j;
    const long long p = (long long)__builtin_amdgcn_readfirstlane((int)q);       // (the host keeps first + n below 2^31)
    RaggedAt at;
    int w = rv.images[0].w, h = rv.images[0].h;
    const long long off = ragged_view_offset(rv.images, rv.b, rv.sh, rv.sw, p, &w, &h);
    at.off = off < 0 ? rv.images[0].elem_off : off;
    at.v.w = w; at.v.h = h;
    at.index = nullptr; at.first = 0; at.wide = rv.wide;
    return at;
}

// uint8 pixels as float32 through their table, for the copies that hand patches back (gather.hip, patchify.hip): the VW (1
// or 4) bytes at q - 4: one naturally aligned dword load - are tc[byte], tc = table + 256 * channel
template <int VW> struct TableFloats { typedef float type; };
template <> struct TableFloats<4> { typedef float4 type; };
template <int VW>
__device__ __forceinline__ typename TableFloats<VW>::type table_floats(const float* tc, const unsigned char* q) {
    if constexpr (VW == 4) {
        const unsigned v = *reinterpret_cast<const unsigned*>(q);
        return make_float4(tc[v & 0xFFu], tc[(v >> 8) & 0xFFu], tc[(v >> 16) & 0xFFu], tc[v >> 24]);
    } else {
        return tc[q[0]];
    }
}

// uint8 images: the 4 NW consecutive bytes at q (inside one image row) as NW little-endian dwords, by loads of `width` bytes
// (launch-uniform, every load naturally aligned): ONE load of 4 NW bytes, NW dwords, or 4 NW single bytes put together -
// the same registers whatever the width, so a kernel's staging code has one form
template <int NW>
__device__ __forceinline__ void view_load_u8(const unsigned char* q, int width, unsigned (&w)[NW]) {
    if (NW == 4 && width == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(q);
        w[0] = v.x; w[1 % NW] = v.y; w[2 % NW] = v.z; w[3 % NW] = v.w;
    } else if (NW == 2 && width == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(q);
        w[0] = v.x; w[1 % NW] = v.y;
    } else if (width >= 4) {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = reinterpret_cast<const unsigned*>(q)[k];
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k)
            w[k] = (unsigned)q[4 * k] | ((unsigned)q[4 * k + 1] << 8) | ((unsigned)q[4 * k + 2] << 16) | ((unsigned)q[4 * k + 3] << 24);
    }
}

// float32 images: the NK float4 units k0 .. k0 + NK - 1 (unit k: pixels 4 (64 k + lane) .. + 3 of the 1x32x32 patch) that
// this lane stages, read from the image rows at `src` (the patch's first pixel; row pitch w floats).  wide (launch-uniform):
// 16-byte loads - src and every row start are 16-byte aligned - else four dword loads.
template <int NK>
__device__ __forceinline__ void view_load_32(const float* src, int w, int wide, int lane, int k0, float4 (&px)[NK]) {
    if (wide) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int e = ((k0 + k) * 64 + lane) * 4;
            px[k] = *reinterpret_cast<const float4*>(src + (long long)(e >> 5) * w + (e & 31));
        }
    } else {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int e = ((k0 + k) * 64 + lane) * 4;
            const float* q = src + (long long)(e >> 5) * w + (e & 31);
            px[k] = make_float4(q[0], q[1], q[2], q[3]);
        }
    }
}
#endif

}  // namespace ipsx

#define IPSX_REQUIRE(cond, ...)                                  \
    do {                                                          \
        if (!(cond)) return ipsx::fail(IPSX_EINVAL, __VA_ARGS__); \
    } while (0)

#define IPSX_TRY(expr)            \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != IPSX_OK) return rc_; \
    } while (0)
