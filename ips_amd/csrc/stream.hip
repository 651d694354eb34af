// stream.hip - the state update of IPSNet.ips_stream (ips_amd/stream.py): after the iterations a feed has
// completed, the M winners and the not yet scored tail move to the front of the other buffer set - for up to four tables
// (patch rows, embeddings, logits, global ids) in ONE launch.  The candidates of a table are two segments that are never
// joined: the rows the stream holds, then the caller's piece (its own base address and batch stride - a slice of a larger
// tensor is read where it lies).  Pure HBM-bound copy like gather.hip: one workgroup per (row, image, table), 16 / 4 / 1
// bytes per lane as row size and addresses allow, source rows clamped into the candidates.

#include "ipsx_common.h"

namespace ipsx {

constexpr int COMMIT_MAX_TABLES = 4;

struct CommitTable {
    const unsigned char* held; long long held_rows, held_bs;     // (held_bs: bytes between the images)
    const unsigned char* piece; long long piece_bs;
    unsigned char* dst; long long dst_bs;
    long long row_bytes;
    int unit;                                                     // 16, 4 or 1 bytes per lane
};

struct CommitArgs {
    CommitTable t[COMMIT_MAX_TABLES];
    const long long* sel;      // (b, m) candidate rows of the new memory, or nullptr: append the piece behind the held rows
    int m;
    long long n_cand, tail_first;
};

template <typename V>
__device__ __forceinline__ void copy_units(const unsigned char* s, unsigned char* d, long long units) {
    const V* sv = reinterpret_cast<const V*>(s);
    V* dv = reinterpret_cast<V*>(d);
    for (long long i = threadIdx.x; i < units; i += 256) dv[i] = sv[i];
}

__global__ __launch_bounds__(256) void stream_commit_kernel(CommitArgs a) {
    const CommitTable& t = a.t[blockIdx.z];
    const long long j = blockIdx.x;
    const int b = blockIdx.y;
    long long r, out;                                             // candidate row read, row of dst written (workgroup-uniform)
    if (a.sel) {
        if (j < a.m) {
            r = a.sel[(size_t)b * a.m + j];
            r = r < 0 ? 0 : (r >= a.n_cand ? a.n_cand - 1 : r);   // never read out of bounds
        } else {
            r = a.tail_first + (j - a.m);
        }
        out = j;
    } else {
        r = t.held_rows + j;                                      // append: the piece's rows go behind the held ones, in place
        if (r >= a.n_cand) return;
        out = r;
    }
    const unsigned char* s = r < t.held_rows ? t.held + (size_t)b * t.held_bs + (size_t)r * t.row_bytes
                                             : t.piece + (size_t)b * t.piece_bs + (size_t)(r - t.held_rows) * t.row_bytes;
    unsigned char* d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
    if (t.unit == 16) copy_units<uint4>(s, d, t.row_bytes / 16);
    else if (t.unit == 4) copy_units<uint32_t>(s, d, t.row_bytes / 4);
    else copy_units<unsigned char>(s, d, t.row_bytes);
}

}  // namespace ipsx

using namespace ipsx;

static bool overlaps(const void* p, long long p_bytes, const void* q, long long q_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q);
    return a < c + (uintptr_t)q_bytes && c < a + (uintptr_t)p_bytes;
}

static bool multiple_of(const void* p, long long unit) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(unit - 1)) == 0; }

IPSX_API int ipsx_stream_commit(const ipsx_stream_table* tables, int n_tables, const int64_t* sel, int b, int m, int64_t n_cand,
                                int64_t tail_first, void* stream) {
    IPSX_REQUIRE(tables, "stream_commit: null tables");
    IPSX_REQUIRE(n_tables > 0 && n_tables <= COMMIT_MAX_TABLES, "stream_commit: %d tables (1 .. %d in one launch)", n_tables,
                 COMMIT_MAX_TABLES);
    IPSX_REQUIRE(b > 0 && m > 0 && n_cand > 0, "stream_commit: bad sizes (b = %d, m = %d, %lld candidates)", b, m, (long long)n_cand);
    IPSX_REQUIRE(!sel || (tail_first >= 0 && tail_first <= n_cand), "stream_commit: the tail starts at candidate %lld of %lld",
                 (long long)tail_first, (long long)n_cand);
    CommitArgs a;
    a.sel = reinterpret_cast<const long long*>(sel); a.m = m; a.n_cand = n_cand; a.tail_first = tail_first;
    long long rows = sel ? m + (n_cand - tail_first) : 0;         // workgroups per image and table
    for (int k = 0; k < n_tables; ++k) {
        const ipsx_stream_table& s = tables[k];
        IPSX_REQUIRE(s.dst && s.row_bytes > 0, "stream_commit: table %d has no destination or no row size", k);
        IPSX_REQUIRE(s.held_rows >= 0 && s.held_rows <= n_cand, "stream_commit: table %d holds %lld of %lld candidates", k,
                     (long long)s.held_rows, (long long)n_cand);
        IPSX_REQUIRE(s.held_rows == n_cand || s.piece, "stream_commit: table %d has candidates behind its held rows but no piece", k);
        IPSX_REQUIRE(!sel || s.held_rows == 0 || (s.held && s.held_bstride_rows >= s.held_rows),
                     "stream_commit: table %d: the held rows are missing or overlap the next image's", k);
        const long long written = sel ? rows : n_cand;            // rows of dst this call may touch: [0, written)
        if (sel) {      // workgroups read candidates while others write dst: the bytes written lie apart from every byte read
            const long long dst_span = ((long long)(b - 1) * s.dst_bstride_rows + written) * s.row_bytes;
            IPSX_REQUIRE(s.held_rows == 0 || !overlaps(s.dst, dst_span, s.held, ((long long)(b - 1) * s.held_bstride_rows + s.held_rows) * s.row_bytes),
                         "stream_commit: table %d is moved in place (a selection goes to the other buffer set)", k);
            IPSX_REQUIRE(s.held_rows == n_cand || !overlaps(s.dst, dst_span, s.piece, (long long)(b - 1) * s.piece_bstride_bytes +
                                                                                       (n_cand - s.held_rows) * s.row_bytes),
                         "stream_commit: table %d: the destination overlaps the piece", k);
        }
        IPSX_REQUIRE(s.dst_rows >= written && (b == 1 || s.dst_bstride_rows >= written),
                     "stream_commit: table %d: %lld rows do not fit the destination (%lld rows, %lld between the images)", k, written,
                     (long long)s.dst_rows, (long long)s.dst_bstride_rows);
        IPSX_REQUIRE(s.piece_bstride_bytes >= 0, "stream_commit: table %d: negative batch stride of the piece", k);
        CommitTable& t = a.t[k];
        t.held = static_cast<const unsigned char*>(s.held); t.held_rows = s.held_rows; t.held_bs = s.held_bstride_rows * s.row_bytes;
        t.piece = static_cast<const unsigned char*>(s.piece); t.piece_bs = s.piece_bstride_bytes;
        t.dst = static_cast<unsigned char*>(s.dst); t.dst_bs = s.dst_bstride_rows * s.row_bytes;
        t.row_bytes = s.row_bytes;
        t.unit = 1;
        for (long long u : {16ll, 4ll})
            if (s.row_bytes % u == 0 && multiple_of(s.dst, u) && (!s.held || multiple_of(s.held, u)) &&
                (!s.piece || (multiple_of(s.piece, u) && s.piece_bstride_bytes % u == 0))) {
                t.unit = (int)u;
                break;
            }
        if (!sel) rows = std::max<long long>(rows, n_cand - s.held_rows);
    }
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.t[k] = a.t[0];
    if (rows <= 0) return IPSX_OK;                                // nothing to append
    IPSX_REQUIRE(rows < ((int64_t)1 << 31) && b < 65536, "stream_commit: %lld rows x %d images in one launch", rows, b);
    stream_commit_kernel<<<dim3((unsigned)rows, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched("stream_commit");
}
