// gather.hip - row gathers that assemble the output of IPSNet.ips:
// mem_patch = gather(patches, mem_idx), mem_pos = gather(pos_enc, mem_idx)
// (reference architecture/ips_net.py:245-250).  Pure HBM-bound copy: one workgroup
// per selected row, 16 bytes per lane when the row allows it.

#include "ipsx_internal.h"

namespace ipsx {

template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(const V* __restrict__ src,
                                                          const long long* __restrict__ idx,
                                                          V* __restrict__ dst, long long n_rows, int m,
                                                          long long row_units, long long src_bstride_rows) {
    const int j = blockIdx.x, b = blockIdx.y;
    long long r = idx[(size_t)b * m + j];
    r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);          // never read out of bounds
    const V* s = src + ((size_t)b * src_bstride_rows + (size_t)r) * row_units;
    V* d = dst + ((size_t)b * m + j) * row_units;
    for (long long i = threadIdx.x; i < row_units; i += 256) d[i] = s[i];
}

// The end of an ips() call whose selection ran as a resident loop, in ONE launch (round 5; it was four: a copy of the
// loop's index buffer, the gather of the patches, the gather of the positional encodings and the copy of the loop's
// status word to the host): workgroup (j, b) copies patch row and positional row of selection j of image b (16 bytes per
// lane) and the index itself; the first thread of the launch also hands the loop's status word to its pinned host mirror.
struct FinishArgs {
    const uint4* patches; long long patch_units, patch_bstride_rows, n_rows;
    const uint4* pos; long long pos_units, pos_bstride_rows;
    const long long* idx; long long* idx_out;
    uint4* out_patch; uint4* out_pos;
    const int* status; int* status_host;
    int m;
    const long long* order; long long order_bstride;      // ORDER kernels: patch row r of image b is source row order[b][r]
};

// ORDER: the selection ran on a permuted NUMBERING of the patches (a shuffle applied as an index, not as a copy): the patch
// row comes from the unshuffled tensor through the permutation; the positional rows (shuffled by copy) and the returned
// indices stay in the loop's numbering.
template <bool ORDER>
__global__ __launch_bounds__(256) void ips_finish_kernel(FinishArgs a) {
    const int j = blockIdx.x, b = blockIdx.y;
    const long long raw = a.idx[(size_t)b * a.m + j];
    const long long r = raw < 0 ? 0 : (raw >= a.n_rows ? a.n_rows - 1 : raw);         // never read out of bounds
    long long rs = r;
    if (ORDER) {
        rs = a.order[(size_t)b * a.order_bstride + r];
        rs = rs < 0 ? 0 : (rs >= a.n_rows ? a.n_rows - 1 : rs);
    }
    const uint4* s = a.patches + ((size_t)b * a.patch_bstride_rows + (size_t)rs) * a.patch_units;
    uint4* d = a.out_patch + ((size_t)b * a.m + j) * a.patch_units;
    for (long long i = threadIdx.x; i < a.patch_units; i += 256) d[i] = s[i];
    if (a.pos) {
        const uint4* sp = a.pos + ((size_t)b * a.pos_bstride_rows + (size_t)r) * a.pos_units;
        uint4* dp = a.out_pos + ((size_t)b * a.m + j) * a.pos_units;
        for (long long i = threadIdx.x; i < a.pos_units; i += 256) dp[i] = sp[i];
    }
    if (threadIdx.x == 0) {
        a.idx_out[(size_t)b * a.m + j] = raw;
        if (a.status_host && j == 0 && b == 0)
            __hip_atomic_store(a.status_host, __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The end of a PADDED ragged call (IPSNet.ips_ragged(pad=True), IPSNet.ips_image_ragged) in ONE launch: workgroup
// (j, b) fills slot j of slide - or image - b: patch row, positional row, local index and global packed row.  The slot rule
// is ragged_finish_slot below, written ONCE for the three sources (packed rows, a float32 ragged view, a uint8 one); a source
// supplies what differs:
//   guard(b, lo, hi, &n)   are the two row offsets this slide's, and its length n
//   dst(slot)              where slot's row of mem_patch lies
//   zero(d)                the padding of mem_patch
//   copy(d, ps)            packed row / packed patch ps into mem_patch
// The argument structs share the names the rule reads (row_off, idx, flat, total, pos, pos_units, out_pos, idx_out, rows_out, m).
struct RaggedFinishArgs {
    const uint4* rows; long long row_units, total;
    const long long* row_off; const long long* idx; const int* flat;
    const uint4* pos; long long pos_units;
    uint4* out_patch; uint4* out_pos; long long* idx_out; long long* rows_out;
    int m;
};

// ... of whole images: the source row is a grid patch copied out of its image
struct RaggedFinishViewArgs {
    const float* pixels; const ipsx_image_entry* images; int b, c, ph, pw, sh, sw; long long total;
    const long long* row_off; const long long* idx; const int* flat;
    const uint4* pos; long long pos_units;
    float* out_patch; uint4* out_pos; long long* idx_out; long long* rows_out;
    int m;
};

// The slide's length comes from the two row offsets (workgroup-uniform, kept scalar as ragged_slide does).  A LONG slide (more
// than m rows) takes the loop's selection idx[b][j], clamped into its own slide; a SHORT one is its rows in the order given -
// idx is not read for it, the loop left that row unwritten - and zeros behind them: the padding is WRITTEN here (index and
// row -1), the output buffers need no memset.  Packed row g is source row flat[g] when a shuffle was applied as an index (the
// positional rows are in packed numbering).  No read leaves [0, total); a slide the source's guard refuses is left untouched.
template <class S>
__device__ __forceinline__ void ragged_finish_slot(const S& src) {
    const auto& a = src.a;
    const int j = blockIdx.x, b = blockIdx.y;
    const long long r0 = a.row_off[b], r1 = a.row_off[b + 1];
    const long long lo = ((long long)__builtin_amdgcn_readfirstlane((int)(r0 >> 32)) << 32) |
                         (unsigned int)__builtin_amdgcn_readfirstlane((int)r0);
    const long long hi = ((long long)__builtin_amdgcn_readfirstlane((int)(r1 >> 32)) << 32) |
                         (unsigned int)__builtin_amdgcn_readfirstlane((int)r1);
    long long n;
    if (!src.guard(b, lo, hi, &n)) return;
    const size_t slot = (size_t)b * a.m + j;
    const auto d = src.dst(slot);
    uint4* dp = a.pos ? a.out_pos + slot * a.pos_units : nullptr;
    long long r;
    if (n > a.m) {
        if (!a.idx) return;                                     // (a batch of short slides only has no selection)
        r = a.idx[slot];
        r = r < 0 ? 0 : (r >= n ? n - 1 : r);                   // inside its OWN slide
    } else if (j < n) {
        r = j;
    } else {                                                    // the padding of a short slide
        src.zero(d);
        if (dp)
            for (long long i = threadIdx.x; i < a.pos_units; i += 256) dp[i] = make_uint4(0u, 0u, 0u, 0u);
        if (threadIdx.x == 0) {
            a.idx_out[slot] = -1;
            a.rows_out[slot] = -1;
        }
        return;
    }
    const long long g = lo + r;                                 // in [lo, hi): inside the table
    long long ps = g;
    if (a.flat) {
        ps = a.flat[g];
        ps = ps < 0 ? 0 : (ps >= a.total ? a.total - 1 : ps);
    }
    src.copy(d, ps);
    if (dp) {
        const uint4* sp = a.pos + (size_t)g * a.pos_units;
        for (long long i = threadIdx.x; i < a.pos_units; i += 256) dp[i] = sp[i];
    }
    if (threadIdx.x == 0) {
        a.idx_out[slot] = r;
        a.rows_out[slot] = g;
    }
}

// packed rows of 16-byte units: offsets that leave the table are refused
struct FinishRows {
    const RaggedFinishArgs& a;
    __device__ __forceinline__ bool guard(int, long long lo, long long hi, long long* n) const {
        if (!(lo >= 0 && hi >= lo && hi <= a.total)) return false;
        *n = hi - lo;
        return true;
    }
    __device__ __forceinline__ uint4* dst(size_t slot) const { return a.out_patch + slot * a.row_units; }
    __device__ __forceinline__ void zero(uint4* d) const {
        for (long long i = threadIdx.x; i < a.row_units; i += 256) d[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __device__ __forceinline__ void copy(uint4* d, long long rs) const {
        const uint4* s = a.rows + (size_t)rs * a.row_units;
        for (long long i = threadIdx.x; i < a.row_units; i += 256) d[i] = s[i];
    }
};

// A ragged view: the image's table entry is workgroup-uniform and kept scalar; an image whose offsets are not its entry's
// (first, first + ny * nx) is refused.  The patch copied is packed patch ps, resolved through the table by the function the
// stems use (ragged_view_offset) - a number that is no packed patch reads packed patch 0, so no read leaves the packed buffer.
// VW: pixels per thread and step (4: 16-byte stores, and 16-byte or - bytes - dword loads: pw, every w, sw and the addresses
// allow them, the host's decision - or 1).  U8: a.pixels holds bytes and mem_patch is float32 table[channel][byte] - what
// ipsx_dequant_patches makes of the copied bytes -, the padding float +0.0, not table[channel][0]; the table (c x 256 floats)
// is read where it lies: L2-resident, and the launch is the call's last one, not its hot one.
template <int VW, bool U8>
struct FinishView {
    typedef typename TableFloats<VW>::type V;
    const RaggedFinishViewArgs& a;
    const float* __restrict__ table;
    struct Dst { V* d; int rowv, units; };                           // the slot's row in units of V, rowv to a patch row
    __device__ __forceinline__ Dst dst(size_t slot) const {
        const int rowv = a.pw / VW;
        return Dst{reinterpret_cast<V*>(a.out_patch + slot * ((size_t)a.c * a.ph * a.pw)), rowv, a.c * a.ph * rowv};
    }
    __device__ __forceinline__ bool guard(int k, long long lo, long long hi, long long* n) const {
        const ipsx_image_entry e = a.images[k];
        const long long len = (long long)e.ny * e.nx;
        if (!(lo >= 0 && lo == e.first && hi - lo == len && hi <= a.total)) return false;
        *n = len;
        return true;
    }
    __device__ __forceinline__ void zero(const Dst& t) const {
        V zero;
        if constexpr (VW == 4) zero = make_float4(0.f, 0.f, 0.f, 0.f); else zero = 0.f;
        for (int i = threadIdx.x; i < t.units; i += 256) t.d[i] = zero;
    }
    __device__ __forceinline__ void copy(const Dst& t, long long ps) const {
        ps = (long long)__builtin_amdgcn_readfirstlane((int)ps);    // (total < 2^31; workgroup-uniform: the table is read scalar)
        int w = a.images[0].w, h = a.images[0].h;
        long long off = ragged_view_offset(a.images, a.b, a.sh, a.sw, ps, &w, &h);
        if (off < 0) off = a.images[0].elem_off;
        for (int i = threadIdx.x; i < t.units; i += 256) {
            const int xv = i % t.rowv, u = i / t.rowv, y = u % a.ph, ch = u / a.ph;
            const long long at = off + ((long long)ch * h + y) * w + xv * VW;
            if constexpr (U8) t.d[i] = table_floats<VW>(table + 256 * ch, reinterpret_cast<const unsigned char*>(a.pixels) + at);
            else t.d[i] = *reinterpret_cast<const V*>(a.pixels + at);
        }
    }
};

__global__ __launch_bounds__(256) void ragged_finish_kernel(RaggedFinishArgs a) { ragged_finish_slot(FinishRows{a}); }

template <int VW, bool U8>
__global__ __launch_bounds__(256) void ragged_finish_view_kernel(RaggedFinishViewArgs a, const float* __restrict__ table) {
    ragged_finish_slot(FinishView<VW, U8>{a, table});
}

}  // namespace ipsx

using namespace ipsx;

static int ips_finish_impl(const void* patches, int64_t patch_row_bytes, int64_t patch_bstride_rows, int64_t n_rows,
                           const void* pos, int64_t pos_row_bytes, int64_t pos_bstride_rows, const int64_t* mem_idx, int b, int m,
                           void* mem_patch, void* mem_pos, int64_t* mem_idx_out, const int32_t* status, int32_t* status_host,
                           const int64_t* order, int64_t order_bstride, void* stream) {
    IPSX_REQUIRE(patches && mem_idx && mem_patch && mem_idx_out && b > 0 && m > 0 && n_rows > 0, "ips_finish: bad arguments");
    IPSX_REQUIRE(patch_row_bytes > 0 && patch_row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(patches) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(mem_patch) & 15) == 0, "ips_finish: patch rows of 16-byte units at 16-byte addresses");
    IPSX_REQUIRE(!pos || (mem_pos && pos_row_bytes > 0 && pos_row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(pos) & 15) == 0 &&
                          (reinterpret_cast<uintptr_t>(mem_pos) & 15) == 0), "ips_finish: positional rows of 16-byte units");
    IPSX_REQUIRE(!status_host || status, "ips_finish: a host mirror needs the status word");
    FinishArgs a;
    a.patches = static_cast<const uint4*>(patches); a.patch_units = patch_row_bytes / 16; a.patch_bstride_rows = patch_bstride_rows;
    a.n_rows = n_rows;
    a.pos = static_cast<const uint4*>(pos); a.pos_units = pos ? pos_row_bytes / 16 : 0; a.pos_bstride_rows = pos_bstride_rows;
    a.idx = reinterpret_cast<const long long*>(mem_idx); a.idx_out = reinterpret_cast<long long*>(mem_idx_out);
    a.out_patch = static_cast<uint4*>(mem_patch); a.out_pos = static_cast<uint4*>(mem_pos);
    a.status = status; a.status_host = status_host; a.m = m;
    a.order = reinterpret_cast<const long long*>(order); a.order_bstride = order_bstride;
    if (order) ips_finish_kernel<true><<<dim3((unsigned)m, (unsigned)b), dim3(256), 0, as_stream(stream)>>>(a);
    else ips_finish_kernel<false><<<dim3((unsigned)m, (unsigned)b), dim3(256), 0, as_stream(stream)>>>(a);
    return launched("ips_finish");
}

IPSX_API int ipsx_ips_finish(const void* patches, int64_t patch_row_bytes, int64_t patch_bstride_rows, int64_t n_rows,
                             const void* pos, int64_t pos_row_bytes, int64_t pos_bstride_rows, const int64_t* mem_idx, int b, int m,
                             void* mem_patch, void* mem_pos, int64_t* mem_idx_out, const int32_t* status, int32_t* status_host,
                             void* stream) {
    return ips_finish_impl(patches, patch_row_bytes, patch_bstride_rows, n_rows, pos, pos_row_bytes, pos_bstride_rows, mem_idx, b, m,
                           mem_patch, mem_pos, mem_idx_out, status, status_host, nullptr, 0, stream);
}

// ipsx_ips_finish after a selection on shuffled NUMBERING: mem_patch[b][j] = patches[b][order[b][mem_idx[b][j]]] from the
// UNSHUFFLED tensor (order: (b or 1, n_rows) int64, order_bstride = n_rows or 0 for one permutation shared by every image);
// mem_pos and mem_idx_out as in ipsx_ips_finish.
IPSX_API int ipsx_ips_finish_indexed(const void* patches, int64_t patch_row_bytes, int64_t patch_bstride_rows, int64_t n_rows,
                                     const void* pos, int64_t pos_row_bytes, int64_t pos_bstride_rows, const int64_t* mem_idx,
                                     const int64_t* order, int64_t order_bstride, int b, int m, void* mem_patch, void* mem_pos,
                                     int64_t* mem_idx_out, const int32_t* status, int32_t* status_host, void* stream) {
    IPSX_REQUIRE(order && (order_bstride == 0 || order_bstride == n_rows), "ips_finish_indexed: order is (b or 1, n_rows)");
    return ips_finish_impl(patches, patch_row_bytes, patch_bstride_rows, n_rows, pos, pos_row_bytes, pos_bstride_rows, mem_idx, b, m,
                           mem_patch, mem_pos, mem_idx_out, status, status_host, order, order_bstride, stream);
}

// The end of IPSNet.ips_ragged(pad=True) in ONE launch (ragged_finish_kernel above): rows (total, row_bytes) the packed
// rows, row_offsets (b + 1) int64 on the device, mem_idx (b, m) slide-local (rows of slides with at most m rows are never
// read; NULL when no slide is longer), flat (total) int32 or NULL, pos (total, pos_row_bytes) or NULL.
IPSX_API int ipsx_ragged_finish(const void* rows, int64_t row_bytes, int64_t total, const int64_t* row_offsets,
                                const int64_t* mem_idx, const int32_t* flat, const void* pos, int64_t pos_row_bytes, int b, int m,
                                void* mem_patch, void* mem_pos, int64_t* mem_idx_out, int64_t* rows_out, void* stream) {
    IPSX_REQUIRE(rows && row_offsets && mem_patch && mem_idx_out && rows_out && b > 0 && b <= 65535 && m > 0 && total > 0,
                 "ragged_finish: bad arguments");
    IPSX_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(mem_patch) & 15) == 0, "ragged_finish: rows of 16-byte units at 16-byte addresses");
    IPSX_REQUIRE(!pos || (mem_pos && pos_row_bytes > 0 && pos_row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(pos) & 15) == 0 &&
                          (reinterpret_cast<uintptr_t>(mem_pos) & 15) == 0), "ragged_finish: positional rows of 16-byte units");
    RaggedFinishArgs a;
    a.rows = static_cast<const uint4*>(rows); a.row_units = row_bytes / 16; a.total = total;
    a.row_off = reinterpret_cast<const long long*>(row_offsets); a.idx = reinterpret_cast<const long long*>(mem_idx); a.flat = flat;
    a.pos = static_cast<const uint4*>(pos); a.pos_units = pos ? pos_row_bytes / 16 : 0;
    a.out_patch = static_cast<uint4*>(mem_patch); a.out_pos = static_cast<uint4*>(mem_pos);
    a.idx_out = reinterpret_cast<long long*>(mem_idx_out); a.rows_out = reinterpret_cast<long long*>(rows_out); a.m = m;
    ragged_finish_kernel<<<dim3((unsigned)m, (unsigned)b), dim3(256), 0, as_stream(stream)>>>(a);
    return launched("ragged_finish");
}

// The end of IPSNet.ips_image_ragged in ONE launch (ragged_finish_view_kernel above): ipsx_ragged_finish on the patches of
// images of different sizes, copied out of the packed buffer.  The view's host table is checked here, before the launch.
// (table: the pixels are bytes, mem_patch their float32 values - ipsx_ragged_finish_view_u8)
static int ragged_finish_view_impl(const void* pixels, const float* table, const ipsx_ragged_view* view, const int64_t* row_offsets,
                                   const int64_t* mem_idx, int m, const int32_t* flat, const void* pos, int64_t pos_row_bytes,
                                   void* mem_patch, void* mem_pos, int64_t* mem_idx_out, int64_t* rows_out, void* stream) {
    IPSX_REQUIRE(pixels && view && row_offsets && mem_patch && mem_idx_out && rows_out && m > 0, "ragged_finish_view: bad arguments");
    const int64_t total = ragged_view_total(view, "ragged_finish_view");
    if (total < 0) return IPSX_EINVAL;
    IPSX_REQUIRE(view->images && view->b <= 65535 && total > 0, "ragged_finish_view: a device table of at most 65535 images");
    IPSX_REQUIRE((table || at_multiple(pixels, 4)) && at_multiple(mem_patch, 4), "ragged_finish_view: pixels and mem_patch at 4-byte addresses");
    IPSX_REQUIRE(!pos || (mem_pos && pos_row_bytes > 0 && pos_row_bytes % 16 == 0 && at_multiple(pos, 16) && at_multiple(mem_pos, 16)),
                 "ragged_finish_view: positional rows of 16-byte units");
    RaggedFinishViewArgs a;
    a.pixels = static_cast<const float*>(pixels); a.images = view->images; a.b = view->b; a.c = view->c; a.ph = view->ph; a.pw = view->pw;
    a.sh = view->sh; a.sw = view->sw; a.total = total;
    a.row_off = reinterpret_cast<const long long*>(row_offsets); a.idx = reinterpret_cast<const long long*>(mem_idx); a.flat = flat;
    a.pos = static_cast<const uint4*>(pos); a.pos_units = pos ? pos_row_bytes / 16 : 0;
    a.out_patch = static_cast<float*>(mem_patch); a.out_pos = static_cast<uint4*>(mem_pos);
    a.idx_out = reinterpret_cast<long long*>(mem_idx_out); a.rows_out = reinterpret_cast<long long*>(rows_out); a.m = m;
    const dim3 grid((unsigned)m, (unsigned)view->b);
    if (table) {                                           // bytes: dword loads where the view allows them, else single bytes
        if (view->pw % 4 == 0 && at_multiple(mem_patch, 16) && ragged_view_at_multiple(pixels, *view, 4, 1))
            ragged_finish_view_kernel<4, true><<<grid, dim3(256), 0, as_stream(stream)>>>(a, table);
        else
            ragged_finish_view_kernel<1, true><<<grid, dim3(256), 0, as_stream(stream)>>>(a, table);
        return launched("ragged_finish_view_u8");
    }
    if (view->pw % 4 == 0 && at_multiple(mem_patch, 16) && ragged_view_at_multiple(pixels, *view, 16))
        ragged_finish_view_kernel<4, false><<<grid, dim3(256), 0, as_stream(stream)>>>(a, nullptr);
    else
        ragged_finish_view_kernel<1, false><<<grid, dim3(256), 0, as_stream(stream)>>>(a, nullptr);
    return launched("ragged_finish_view");
}

IPSX_API int ipsx_ragged_finish_view(const float* pixels, const ipsx_ragged_view* view, const int64_t* row_offsets,
                                     const int64_t* mem_idx, int m, const int32_t* flat, const void* pos, int64_t pos_row_bytes,
                                     void* mem_patch, void* mem_pos, int64_t* mem_idx_out, int64_t* rows_out, void* stream) {
    return ragged_finish_view_impl(pixels, nullptr, view, row_offsets, mem_idx, m, flat, pos, pos_row_bytes, mem_patch, mem_pos,
                                   mem_idx_out, rows_out, stream);
}

// ... on whole uint8 images: mem_patch (b, m, c, ph, pw) float32 = table[channel][byte], the padding float +0.0
IPSX_API int ipsx_ragged_finish_view_u8(const uint8_t* pixels, const float* table, const ipsx_ragged_view* view,
                                        const int64_t* row_offsets, const int64_t* mem_idx, int m, const int32_t* flat,
                                        const void* pos, int64_t pos_row_bytes, void* mem_patch, void* mem_pos,
                                        int64_t* mem_idx_out, int64_t* rows_out, void* stream) {
    IPSX_REQUIRE(table, "ragged_finish_view_u8: no table");
    return ragged_finish_view_impl(pixels, table, view, row_offsets, mem_idx, m, flat, pos, pos_row_bytes, mem_patch, mem_pos,
                                   mem_idx_out, rows_out, stream);
}

IPSX_API int ipsx_gather_rows(const void* src, const int64_t* idx, void* dst, int b, int64_t n_rows, int m,
                              int64_t row_bytes, int64_t src_bstride_rows, void* stream) {
    IPSX_REQUIRE(src && idx && dst && b > 0 && n_rows > 0 && m > 0, "gather_rows: bad arguments");
    IPSX_REQUIRE(row_bytes > 0, "gather_rows: row of %lld bytes", (long long)row_bytes);
    dim3 grid((unsigned)m, (unsigned)b);
    const bool a16 = row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    if (a16)
        gather_rows_kernel<uint4><<<grid, dim3(256), 0, as_stream(stream)>>>(
            static_cast<const uint4*>(src), reinterpret_cast<const long long*>(idx), static_cast<uint4*>(dst),
            n_rows, m, row_bytes / 16, src_bstride_rows);
    else if (row_bytes % 4 != 0 || (reinterpret_cast<uintptr_t>(src) & 3) != 0 || (reinterpret_cast<uintptr_t>(dst) & 3) != 0)
        // rows of any size, byte by byte: uint8 patches whose C * h * w is no multiple of 4 (3 x 37 x 45)
        gather_rows_kernel<unsigned char><<<grid, dim3(256), 0, as_stream(stream)>>>(
            static_cast<const unsigned char*>(src), reinterpret_cast<const long long*>(idx),
            static_cast<unsigned char*>(dst), n_rows, m, row_bytes, src_bstride_rows);
    else
        gather_rows_kernel<uint32_t><<<grid, dim3(256), 0, as_stream(stream)>>>(
            static_cast<const uint32_t*>(src), reinterpret_cast<const long long*>(idx),
            static_cast<uint32_t*>(dst), n_rows, m, row_bytes / 4, src_bstride_rows);
    return launched("gather_rows");
}
