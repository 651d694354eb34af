// quant.hip - uint8 patches back to float32 through their table (ipsx_dequant_patches).
//
// uint8 patch storage (ipsx_trunk_encode_u8) keeps a pixel as the byte the dataset read from disk; its float32 value is
// table[channel][byte], a 256-entry row per channel the host fills with the dataset's own tensor ops.  The encoders' stems
// look bytes up as they stage a patch; this kernel does the same for the M patches a selection keeps, which go on to
// forward() / the training step as float32 - so what leaves ips() is bit for bit what it returns for the expanded tensor.

#include "ipsx_common.h"

namespace ipsx {

// q (n, c, hw) bytes -> out (n, c, hw) floats; thread = 4 consecutive elements (one dword load where q is 4-byte
// aligned, one 16-byte store where out is 16-byte aligned and the four lie inside the tensor), the last thread the tail
__global__ __launch_bounds__(256) void dequant_patches_kernel(const unsigned char* __restrict__ q, const float* __restrict__ table,
                                                              float* __restrict__ out, long long total, int c, int hw, int aligned) {
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    if (aligned && e0 + 4 <= total) {
        const unsigned w = *reinterpret_cast<const unsigned*>(q + e0);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = (int)(((e0 + j) / hw) % c);
            v[j] = table[ch * 256 + ((w >> (8 * j)) & 0xFFu)];
        }
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (long long e = e0; e < e0 + 4 && e < total; ++e) {
        const int ch = (int)((e / hw) % c);
        out[e] = table[ch * 256 + q[e]];
    }
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_dequant_patches(const uint8_t* q, const float* table, float* out, int64_t n_patch, int c, int hw, void* stream) {
    IPSX_REQUIRE(q && table && out && n_patch >= 0 && c > 0 && hw > 0, "dequant_patches: bad arguments");
    const int64_t total = n_patch * c * hw;
    if (total == 0) return IPSX_OK;
    const int aligned = reinterpret_cast<uintptr_t>(q) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int64_t blocks = cdiv(cdiv(total, 4), 256);
    IPSX_REQUIRE(blocks < ((int64_t)1 << 31), "dequant_patches: %lld elements in one call", (long long)total);
    dequant_patches_kernel<<<dim3((unsigned)blocks), dim3(256), 0, as_stream(stream)>>>(q, table, out, total, c, hw, aligned);
    return launched("dequant_patches");
}
