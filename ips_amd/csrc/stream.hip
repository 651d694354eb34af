// stream.hip - the state update of IPSNet.ips_stream (ips_amd/stream.py): after the iterations a feed has
// completed, the M winners and the not yet scored tail move to the front of the other buffer set - for up to four tables
// (patch rows, embeddings, logits, global ids) in ONE launch.  The candidates of a table are two segments that are never
// joined: the rows the stream holds, then the caller's piece (its own base address and batch stride - a slice of a larger
// tensor is read where it lies).  Pure HBM-bound copy like gather.hip: one workgroup per (row, image, table), 16 / 4 / 1
// bytes per lane as row size and addresses allow, source rows clamped into the candidates.
//
// stream_commit_view_kernel (IPSStream.feed_rows) is the same update when the piece of the PATCH table is no
// tensor at all: the candidates behind the held rows are patches of a (b, c, h, w) window of whole images, read through its
// ipsx_patch_view - c * ph segments of pw elements each, copied raw (bytes stay bytes).  The other tables of the launch keep
// their contiguous pieces.  stream_commit_ragged_view_kernel (RaggedIPSStream.feed_rows) is that for slides with
// their own numbers: the patches are those of a ragged view over windows of different sizes.

#include "ipsx_internal.h"

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

// the patch table of a row stream: table 0's piece is (images, view) - candidate held_rows + r of image b is grid patch
// b * per_image + r.  unit: bytes per lane of THAT segment, uniform over the launch (host: images, w, sw, pw, dst, held).
struct CommitViewArgs {
    CommitArgs c;
    const unsigned char* images;
    ipsx_patch_view v;
    int elem, unit;                                               // bytes per pixel (4 | 1); 16, 4 or 1 bytes per lane
    long long per_image;                                          // ny * nx
};

// one patch out of the image grid: c * ph segments of seg_units lanes; no load leaves its patch row
template <typename V>
__device__ __forceinline__ void copy_patch_units(const unsigned char* s, unsigned char* d, const ipsx_patch_view& v, int elem) {
    const unsigned seg_units = (unsigned)(v.pw * elem) / (unsigned)sizeof(V), total = (unsigned)(v.c * v.ph) * seg_units;
    const long long pitch = (long long)v.w * elem;                // bytes between two rows of an image
    V* dv = reinterpret_cast<V*>(d);
    for (unsigned i = threadIdx.x; i < total; i += 256) {
        const unsigned seg = i / seg_units, u = i - seg * seg_units, ch = seg / (unsigned)v.ph, y = seg - ch * (unsigned)v.ph;
        dv[i] = *reinterpret_cast<const V*>(s + ((long long)ch * v.h + y) * pitch + (size_t)u * sizeof(V));
    }
}

__global__ __launch_bounds__(256) void stream_commit_view_kernel(CommitViewArgs a) {
    const CommitTable& t = a.c.t[blockIdx.z];
    const long long j = blockIdx.x;
    const int b = blockIdx.y;
    long long r, out;                                             // as stream_commit_kernel
    if (a.c.sel) {
        if (j < a.c.m) {
            r = a.c.sel[(size_t)b * a.c.m + j];
            r = r < 0 ? 0 : (r >= a.c.n_cand ? a.c.n_cand - 1 : r);
        } else {
            r = a.c.tail_first + (j - a.c.m);
        }
        out = j;
    } else {
        r = t.held_rows + j;
        if (r >= a.c.n_cand) return;
        out = r;
    }
    unsigned char* d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
    if (blockIdx.z == 0 && r >= t.held_rows) {                    // a patch of the window (r - held_rows < per_image: host)
        long long off = patch_view_offset(a.v, (long long)b * a.per_image + (r - t.held_rows));
        if (off < 0) off = 0;
        const unsigned char* s = a.images + off * a.elem;
        if (a.unit == 16) copy_patch_units<uint4>(s, d, a.v, a.elem);
        else if (a.unit == 4) copy_patch_units<uint32_t>(s, d, a.v, a.elem);
        else copy_patch_units<unsigned char>(s, d, a.v, a.elem);
        return;
    }
    const unsigned char* s = r < t.held_rows ? t.held + (size_t)b * t.held_bs + (size_t)r * t.row_bytes
                                             : t.piece + (size_t)b * t.piece_bs + (size_t)(r - t.held_rows) * t.row_bytes;
    if (t.unit == 16) copy_units<uint4>(s, d, t.row_bytes / 16);
    else if (t.unit == 4) copy_units<uint32_t>(s, d, t.row_bytes / 4);
    else copy_units<unsigned char>(s, d, t.row_bytes);
}

// stream_commit_ragged_kernel (IPSNet.ips_ragged_stream): the update for slides that each have their own numbers.
// Per slide six int64 words on the device - held rows, candidates, tail_first, the slide's first row in the packed piece,
// the mode, one reserved - where stream_commit_kernel reads one n_cand and one tail_first for all images; the piece of a
// table is ONE packed (piece_rows, row_bytes) tensor for all slides.  A table without a piece holds all of a slide's
// candidates itself (the logits table behind the loop).
constexpr long long COMMIT_APPEND = 1, COMMIT_SELECT = 2, COMMIT_MOVE = 3;      // (0, and anything else: idle)

struct RaggedCommitTable {
    const unsigned char* held; long long held_rows, held_bs;     // held_rows: rows per slide that may be read; held_bs: bytes between the slides
    const unsigned char* piece;                                   // packed for all slides, or nullptr
    unsigned char* dst; long long dst_rows, dst_bs;
    long long row_bytes;
    int unit;                                                     // 16, 4 or 1 bytes per lane
    int in_place;                                                 // dst is the buffer `held` points into: append only
};

struct RaggedCommitArgs {
    RaggedCommitTable t[COMMIT_MAX_TABLES];
    const long long* sel;      // (b, m) candidate rows of the slides that select, or nullptr
    const long long* slides;   // (b, 6)
    int m, n_tables;
    long long piece_rows;      // rows of the packed pieces
};

__device__ __forceinline__ long long uniform_ll(long long v) {
    return ((long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)v);
}

__global__ __launch_bounds__(256) void stream_commit_ragged_kernel(RaggedCommitArgs a) {
    const long long j = blockIdx.x;
    const int b = blockIdx.y;
    const long long* w = a.slides + (size_t)b * 6;
    const long long held = uniform_ll(w[0]), cand = uniform_ll(w[1]), tail_first = uniform_ll(w[2]), first = uniform_ll(w[3]),
                    mode = uniform_ll(w[4]);
    if (mode != COMMIT_APPEND && mode != COMMIT_SELECT && mode != COMMIT_MOVE) return;      // idle (and anything unknown)
    // the slide's numbers against every table of the launch: one contradiction and the slide is not touched in any of them
    const long long lim = 1ll << 40;                              // (sums below cannot overflow)
    if (!(held >= 0 && cand >= held && cand > 0 && cand < lim && first >= 0 && first < lim)) return;
    if (mode == COMMIT_SELECT && !(a.sel && tail_first >= 0 && tail_first <= cand)) return;
    const long long rows = mode == COMMIT_APPEND ? cand - held : (mode == COMMIT_SELECT ? a.m + (cand - tail_first) : cand);
    const long long last = mode == COMMIT_APPEND ? cand : rows;  // dst rows [.., last) are written
    for (int k = 0; k < a.n_tables; ++k) {
        const RaggedCommitTable& c = a.t[k];
        const long long in_held = c.piece ? held : cand;          // candidates of this table that lie in its held rows
        if (in_held > c.held_rows || last > c.dst_rows) return;
        if (c.piece && first + (cand - held) > a.piece_rows) return;
        if (c.in_place && mode != COMMIT_APPEND) return;
    }
    if (j >= rows) return;
    const RaggedCommitTable& t = a.t[blockIdx.z];
    long long r, out;                                             // candidate row read, row of dst written (workgroup-uniform)
    if (mode == COMMIT_APPEND) {
        if (!t.piece) return;                                     // (a table that holds its candidates has nothing to append)
        r = held + j;
        out = r;
    } else if (mode == COMMIT_SELECT) {
        if (j < a.m) {
            r = a.sel[(size_t)b * a.m + j];
            r = r < 0 ? 0 : (r >= cand ? cand - 1 : r);           // never read out of bounds
        } else {
            r = tail_first + (j - a.m);
        }
        out = j;
    } else {
        r = out = j;
    }
    const long long in_held = t.piece ? held : cand;
    const unsigned char* s = r < in_held ? t.held + (size_t)b * t.held_bs + (size_t)r * t.row_bytes
                                         : t.piece + (size_t)(first + (r - in_held)) * t.row_bytes;
    unsigned char* d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
    if (t.unit == 16) copy_units<uint4>(s, d, t.row_bytes / 16);
    else if (t.unit == 4) copy_units<uint32_t>(s, d, t.row_bytes / 4);
    else copy_units<unsigned char>(s, d, t.row_bytes);
}

// stream_commit_ragged_view_kernel (RaggedIPSStream.feed_rows): stream_commit_ragged_kernel when the piece of
// the PATCH table (table 0) is no tensor: candidate held + r of slide k is packed patch first_k + r of a ragged view over the
// feed's packed pixel windows - word 3 of the slide's row means in the view what it means in the packed pieces of tables
// 1 .. - copied raw, c * ph segments of pw elements with the pitches of ITS image.  The image is found by the stems'
// bisection, on scalar registers: the patch number is workgroup-uniform, the lanes only copy.
struct RaggedCommitViewArgs {
    RaggedCommitArgs c;
    const unsigned char* pixels;
    const ipsx_image_entry* images;                               // the view's DEVICE table, vb entries
    int vb, vc, ph, pw, sh, sw;
    int elem, unit;                                               // bytes per pixel (4 | 1); 16, 4 or 1 bytes per lane (host)
    long long view_total, pixel_elems;                            // packed patches of the view; elements of the pixel buffer (host table)
};

// one patch of an image of height h and row pitch w: c * ph segments of seg_units lanes; no load leaves its patch row
template <typename V>
__device__ __forceinline__ void copy_ragged_patch_units(const unsigned char* s, unsigned char* d, int c, int ph, int pw, int h, int w,
                                                        int elem) {
    const unsigned seg_units = (unsigned)(pw * elem) / (unsigned)sizeof(V), total = (unsigned)(c * ph) * seg_units;
    const long long pitch = (long long)w * elem;                  // bytes between two rows of the image
    V* dv = reinterpret_cast<V*>(d);
    for (unsigned i = threadIdx.x; i < total; i += 256) {
        const unsigned seg = i / seg_units, u = i - seg * seg_units, ch = seg / (unsigned)ph, y = seg - ch * (unsigned)ph;
        dv[i] = *reinterpret_cast<const V*>(s + ((long long)ch * h + y) * pitch + (size_t)u * sizeof(V));
    }
}

__global__ __launch_bounds__(256) void stream_commit_ragged_view_kernel(RaggedCommitViewArgs a) {
    const long long j = blockIdx.x;
    const int b = blockIdx.y;
    const long long* w = a.c.slides + (size_t)b * 6;
    const long long held = uniform_ll(w[0]), cand = uniform_ll(w[1]), tail_first = uniform_ll(w[2]), first = uniform_ll(w[3]),
                    mode = uniform_ll(w[4]);
    if (mode != COMMIT_APPEND && mode != COMMIT_SELECT && mode != COMMIT_MOVE) return;      // idle (and anything unknown)
    // as stream_commit_ragged_kernel: one contradiction with any table - the view is table 0's piece - and the slide is not touched
    const long long lim = 1ll << 40;
    if (!(held >= 0 && cand >= held && cand > 0 && cand < lim && first >= 0 && first < lim)) return;
    if (mode == COMMIT_SELECT && !(a.c.sel && tail_first >= 0 && tail_first <= cand)) return;
    const long long rows = mode == COMMIT_APPEND ? cand - held : (mode == COMMIT_SELECT ? a.c.m + (cand - tail_first) : cand);
    const long long last = mode == COMMIT_APPEND ? cand : rows;
    if (first + (cand - held) > a.view_total) return;
    for (int k = 0; k < a.c.n_tables; ++k) {
        const RaggedCommitTable& c = a.c.t[k];
        const long long in_held = (k == 0 || c.piece) ? held : cand;
        if (in_held > c.held_rows || last > c.dst_rows) return;
        if (k && c.piece && first + (cand - held) > a.c.piece_rows) return;
        if (c.in_place && mode != COMMIT_APPEND) return;
    }
    if (j >= rows) return;
    const bool patches = blockIdx.z == 0;
    const RaggedCommitTable& t = a.c.t[blockIdx.z];
    long long r, out;                                             // candidate row read, row of dst written (workgroup-uniform)
    if (mode == COMMIT_APPEND) {
        if (!patches && !t.piece) return;
        r = held + j;
        out = r;
    } else if (mode == COMMIT_SELECT) {
        if (j < a.c.m) {
            r = a.c.sel[(size_t)b * a.c.m + j];
            r = r < 0 ? 0 : (r >= cand ? cand - 1 : r);           // never read out of bounds
        } else {
            r = tail_first + (j - a.c.m);
        }
        out = j;
    } else {
        r = out = j;
    }
    const long long in_held = (patches || t.piece) ? held : cand;
    unsigned char* d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
    if (patches && r >= in_held) {                                // a patch of the view: first + (r - held) < view_total (above)
        const long long p = uniform_ll(first + (r - in_held));
        int iw = 0, ih = 0;
        const long long off = uniform_ll(ragged_view_offset(a.images, a.vb, a.sh, a.sw, p, &iw, &ih));
        iw = __builtin_amdgcn_readfirstlane(iw); ih = __builtin_amdgcn_readfirstlane(ih);
        // the entry against the buffer the host measured: a device table that says otherwise is not followed out of it
        if (off < 0 || off >= a.pixel_elems || ih < a.ph || iw < a.pw || (long long)ih * iw > a.pixel_elems) return;
        if (off +((long long)(a.vc - 1) * ih + (a.ph - 1)) * iw + a.pw > a.pixel_elems) return;
        const unsigned char* s = a.pixels + off * a.elem;
        if (a.unit == 16) copy_ragged_patch_units<uint4>(s, d, a.vc, a.ph, a.pw, ih, iw, a.elem);
        else if (a.unit == 4) copy_ragged_patch_units<uint32_t>(s, d, a.vc, a.ph, a.pw, ih, iw, a.elem);
        else copy_ragged_patch_units<unsigned char>(s, d, a.vc, a.ph, a.pw, ih, iw, a.elem);
        return;
    }
    const unsigned char* s = r < in_held ? t.held + (size_t)b * t.held_bs + (size_t)r * t.row_bytes
                                         : t.piece + (size_t)(first + (r - in_held)) * t.row_bytes;
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

// one table of a commit, checked and translated for the kernels.  rows: workgroups per image of a selection (m + tail).
// view_piece: the candidates behind the held rows are no tensor (stream_commit_view's patch table) - `piece` stays null and
// the caller picks the lane width.
static int commit_table(const char* what, const ipsx_stream_table& s, int k, bool sel, int b, long long n_cand, long long rows,
                        bool view_piece, CommitTable& t) {
    IPSX_REQUIRE(s.dst && s.row_bytes > 0, "%s: table %d has no destination or no row size", what, k);
    IPSX_REQUIRE(s.held_rows >= 0 && s.held_rows <= n_cand, "%s: table %d holds %lld of %lld candidates", what, k,
                 (long long)s.held_rows, (long long)n_cand);
    IPSX_REQUIRE(!view_piece || !s.piece, "%s: table %d: its piece is the patch view (no piece pointer)", what, k);
    IPSX_REQUIRE(view_piece || s.held_rows == n_cand || s.piece, "%s: table %d has candidates behind its held rows but no piece", what, k);
    IPSX_REQUIRE(!sel || s.held_rows == 0 || (s.held && s.held_bstride_rows >= s.held_rows),
                 "%s: table %d: the held rows are missing or overlap the next image's", what, k);
    const long long written = sel ? rows : n_cand;                // rows of dst this call may touch: [0, written)
    if (sel) {          // workgroups read candidates while others write dst: the bytes written lie apart from every byte read
        const long long dst_span = ((long long)(b - 1) * s.dst_bstride_rows + written) * s.row_bytes;
        IPSX_REQUIRE(s.held_rows == 0 || !overlaps(s.dst, dst_span, s.held, ((long long)(b - 1) * s.held_bstride_rows + s.held_rows) * s.row_bytes),
                     "%s: table %d is moved in place (a selection goes to the other buffer set)", what, k);
        IPSX_REQUIRE(view_piece || s.held_rows == n_cand ||
                         !overlaps(s.dst, dst_span, s.piece, (long long)(b - 1) * s.piece_bstride_bytes + (n_cand - s.held_rows) * s.row_bytes),
                     "%s: table %d: the destination overlaps the piece", what, k);
    }
    IPSX_REQUIRE(s.dst_rows >= written && (b == 1 || s.dst_bstride_rows >= written),
                 "%s: table %d: %lld rows do not fit the destination (%lld rows, %lld between the images)", what, k, written,
                 (long long)s.dst_rows, (long long)s.dst_bstride_rows);
    IPSX_REQUIRE(s.piece_bstride_bytes >= 0, "%s: table %d: negative batch stride of the piece", what, k);
    t.held = static_cast<const unsigned char*>(s.held); t.held_rows = s.held_rows; t.held_bs = s.held_bstride_rows * s.row_bytes;
    t.piece = static_cast<const unsigned char*>(s.piece); t.piece_bs = s.piece_bstride_bytes;
    t.dst = static_cast<unsigned char*>(s.dst); t.dst_bs = s.dst_bstride_rows * s.row_bytes;
    t.row_bytes = s.row_bytes;
    t.unit = 1;
    if (view_piece) return IPSX_OK;
    for (long long u : {16ll, 4ll})
        if (s.row_bytes % u == 0 && multiple_of(s.dst, u) && (!s.held || multiple_of(s.held, u)) &&
            (!s.piece || (multiple_of(s.piece, u) && s.piece_bstride_bytes % u == 0))) {
            t.unit = (int)u;
            break;
        }
    return IPSX_OK;
}

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
        IPSX_TRY(commit_table("stream_commit", tables[k], k, sel != nullptr, b, n_cand, rows, false, a.t[k]));
        if (!sel) rows = std::max<long long>(rows, n_cand - tables[k].held_rows);
    }
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.t[k] = a.t[0];
    if (rows <= 0) return IPSX_OK;                                // nothing to append
    IPSX_REQUIRE(rows < ((int64_t)1 << 31) && b < 65536, "stream_commit: %lld rows x %d images in one launch", rows, b);
    stream_commit_kernel<<<dim3((unsigned)rows, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched("stream_commit");
}

IPSX_API int ipsx_stream_commit_view(const ipsx_stream_table* tables, int n_tables, const void* images, const ipsx_patch_view* v,
                                     int elem_size, const int64_t* sel, int b, int m, int64_t n_cand, int64_t tail_first,
                                     int* unit, void* stream) {
    const char* what = "stream_commit_view";
    IPSX_REQUIRE(tables, "%s: null tables", what);
    IPSX_REQUIRE(images && v, "%s: null images or view", what);
    IPSX_REQUIRE(elem_size == 4 || elem_size == 1, "%s: an element of %d bytes (float32: 4, uint8: 1)", what, elem_size);
    IPSX_REQUIRE(n_tables > 0 && n_tables <= COMMIT_MAX_TABLES, "%s: %d tables (1 .. %d in one launch)", what, n_tables, COMMIT_MAX_TABLES);
    IPSX_REQUIRE(b > 0 && m > 0 && n_cand > 0, "%s: bad sizes (b = %d, m = %d, %lld candidates)", what, b, m, (long long)n_cand);
    IPSX_REQUIRE(!sel || (tail_first >= 0 && tail_first <= n_cand), "%s: the tail starts at candidate %lld of %lld", what,
                 (long long)tail_first, (long long)n_cand);
    IPSX_REQUIRE(patch_view_offset(*v, 0) >= 0, "%s: the view does not fit its images (%dx%dx%dx%d, patch %dx%d, stride %dx%d)", what,
                 v->b, v->c, v->h, v->w, v->ph, v->pw, v->sh, v->sw);
    IPSX_REQUIRE(v->b == b, "%s: a view of %d images in a call of %d", what, v->b, b);
    CommitViewArgs a;
    a.c.sel = reinterpret_cast<const long long*>(sel); a.c.m = m; a.c.n_cand = n_cand; a.c.tail_first = tail_first;
    a.images = static_cast<const unsigned char*>(images); a.v = *v; a.elem = elem_size;
    a.per_image = (long long)((v->h - v->ph) / v->sh + 1) * ((v->w - v->pw) / v->sw + 1);
    long long rows = sel ? m + (n_cand - tail_first) : 0;
    for (int k = 0; k < n_tables; ++k) {
        const ipsx_stream_table& s = tables[k];
        IPSX_TRY(commit_table(what, s, k, sel != nullptr, b, n_cand, rows, k == 0, a.c.t[k]));
        if (!sel) rows = std::max<long long>(rows, n_cand - s.held_rows);
        if (k) continue;
        // table 0: the patch table.  Its rows are whole patches of the view, its piece at most the view's patches per image,
        // and nothing it writes lies inside the images (in EITHER mode: the images are read while dst is written)
        const long long eb = elem_size, seg = (long long)v->pw * eb;
        IPSX_REQUIRE(s.row_bytes == (long long)v->c * v->ph * seg, "%s: rows of %lld bytes, a %dx%dx%d patch of %d-byte elements has %lld",
                     what, (long long)s.row_bytes, v->c, v->ph, v->pw, elem_size, (long long)v->c * v->ph * seg);
        IPSX_REQUIRE(n_cand - s.held_rows <= a.per_image, "%s: %lld candidates behind the held rows, the view has %lld patches per image", what,
                     (long long)(n_cand - s.held_rows), a.per_image);
        const long long written = sel ? rows : n_cand;
        IPSX_REQUIRE(!overlaps(s.dst, ((long long)(b - 1) * s.dst_bstride_rows + written) * s.row_bytes, images,
                               (long long)v->b * v->c * v->h * v->w * eb),
                     "%s: the destination overlaps the images", what);
        a.unit = 1;
        for (long long u : {16ll, 4ll})
            if (seg % u == 0 && ((long long)v->w * eb) % u == 0 && ((long long)v->sw * eb) % u == 0 && multiple_of(images, u) &&
                multiple_of(s.dst, u) && (!s.held || multiple_of(s.held, u))) {
                a.unit = (int)u;
                break;
            }
        a.c.t[0].unit = a.unit;                                   // (row_bytes is a multiple of seg: the held rows go the same width)
    }
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.c.t[k] = a.c.t[0];
    if (unit) *unit = a.unit;
    if (rows <= 0) return IPSX_OK;
    IPSX_REQUIRE(rows < ((int64_t)1 << 31) && b < 65536, "%s: %lld rows x %d images in one launch", what, rows, b);
    stream_commit_view_kernel<<<dim3((unsigned)rows, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched(what);
}

// one table of a ragged commit, checked and translated for the kernels.  view_piece: the candidates behind the held rows are
// patches of a ragged view (stream_commit_ragged_view's patch table) - `piece` stays null and the caller picks the lane width.
static int ragged_commit_table(const char* what, const ipsx_stream_table& s, int k, int b, long long piece_rows_total, bool view_piece,
                               RaggedCommitTable& t) {
    IPSX_REQUIRE(s.dst && s.row_bytes > 0, "%s: table %d has no destination or no row size", what, k);
    IPSX_REQUIRE(s.held_rows >= 0 && (s.held_rows == 0 || (s.held && (b == 1 || s.held_bstride_rows >= s.held_rows))),
                 "%s: table %d: the held rows are missing or overlap the next slide's", what, k);
    IPSX_REQUIRE(!view_piece || !s.piece, "%s: table %d: its piece is the ragged view (no piece pointer)", what, k);
    IPSX_REQUIRE(view_piece || s.piece || s.held_rows > 0, "%s: table %d has neither held rows nor a piece", what, k);
    IPSX_REQUIRE(!s.piece || piece_rows_total > 0, "%s: table %d: a piece of no rows", what, k);
    IPSX_REQUIRE(s.piece_bstride_bytes == 0, "%s: table %d: the piece is one packed tensor (batch stride 0)", what, k);
    IPSX_REQUIRE(s.dst_rows > 0 && (b == 1 || s.dst_bstride_rows >= s.dst_rows),
                 "%s: table %d: a destination of %lld rows, %lld between the slides", what, k, (long long)s.dst_rows,
                 (long long)s.dst_bstride_rows);
    const long long dst_span = ((long long)(b - 1) * s.dst_bstride_rows + s.dst_rows) * s.row_bytes;
    t.in_place = 0;
    if (s.held_rows > 0) {
        // in place (append only: the kernel leaves a slide that selects or moves there untouched), or apart
        if (s.held == s.dst && (b == 1 || s.held_bstride_rows == s.dst_bstride_rows)) t.in_place = 1;
        else
            IPSX_REQUIRE(!overlaps(s.dst, dst_span, s.held, ((long long)(b - 1) * s.held_bstride_rows + s.held_rows) * s.row_bytes),
                         "%s: table %d: the destination overlaps the held rows (in place only from the same address)", what, k);
    }
    IPSX_REQUIRE(!s.piece || !overlaps(s.dst, dst_span, s.piece, piece_rows_total * s.row_bytes),
                 "%s: table %d: the destination overlaps the piece", what, k);
    t.held = static_cast<const unsigned char*>(s.held); t.held_rows = s.held_rows; t.held_bs = s.held_bstride_rows * s.row_bytes;
    t.piece = static_cast<const unsigned char*>(s.piece);
    t.dst = static_cast<unsigned char*>(s.dst); t.dst_rows = s.dst_rows; t.dst_bs = s.dst_bstride_rows * s.row_bytes;
    t.row_bytes = s.row_bytes;
    t.unit = 1;
    if (view_piece) return IPSX_OK;
    for (long long u : {16ll, 4ll})
        if (s.row_bytes % u == 0 && multiple_of(s.dst, u) && (!s.held || multiple_of(s.held, u)) && (!s.piece || multiple_of(s.piece, u))) {
            t.unit = (int)u;
            break;
        }
    return IPSX_OK;
}

// The state update of a ragged stream (IPSNet.ips_ragged_stream) as ONE launch: see stream_commit_ragged_kernel.  What the host
// can know is refused here; what only the device table says is checked per slide in the kernel.
IPSX_API int ipsx_stream_commit_ragged(const ipsx_stream_table* tables, int n_tables, const int64_t* sel, const int64_t* slides,
                                       int b, int m, int64_t rows_max, int64_t piece_rows_total, void* stream) {
    const char* what = "stream_commit_ragged";
    IPSX_REQUIRE(tables, "%s: null tables", what);
    IPSX_REQUIRE(n_tables > 0 && n_tables <= COMMIT_MAX_TABLES, "%s: %d tables (1 .. %d in one launch)", what, n_tables, COMMIT_MAX_TABLES);
    IPSX_REQUIRE(b > 0 && m > 0 && rows_max >= 0 && piece_rows_total >= 0, "%s: bad sizes (b = %d, m = %d, %lld rows, a piece of %lld)",
                 what, b, m, (long long)rows_max, (long long)piece_rows_total);
    IPSX_REQUIRE(slides, "%s: null slide table", what);
    RaggedCommitArgs a;
    a.sel = reinterpret_cast<const long long*>(sel); a.slides = reinterpret_cast<const long long*>(slides);
    a.m = m; a.n_tables = n_tables; a.piece_rows = piece_rows_total;
    for (int k = 0; k < n_tables; ++k) IPSX_TRY(ragged_commit_table(what, tables[k], k, b, piece_rows_total, false, a.t[k]));
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.t[k] = a.t[0];
    if (rows_max == 0) return IPSX_OK;
    IPSX_REQUIRE(rows_max < ((int64_t)1 << 31) && b < 65536, "%s: %lld rows x %d slides in one launch", what, (long long)rows_max, b);
    stream_commit_ragged_kernel<<<dim3((unsigned)rows_max, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched(what);
}

// ... for a ragged stream fed pixel-row bands (RaggedIPSStream.feed_rows): table 0's piece is (pixels, view).  The view's HOST
// table is checked again and gives the patch count, the extent of the pixel buffer and the launch's load width.
IPSX_API int ipsx_stream_commit_ragged_view(const ipsx_stream_table* tables, int n_tables, const void* pixels,
                                            const ipsx_ragged_view* view, int elem_size, const int64_t* sel, const int64_t* slides,
                                            int b, int m, int64_t rows_max, int64_t piece_rows_total, int* unit, void* stream) {
    const char* what = "stream_commit_ragged_view";
    IPSX_REQUIRE(tables, "%s: null tables", what);
    IPSX_REQUIRE(pixels && view, "%s: null pixels or view", what);
    IPSX_REQUIRE(elem_size == 4 || elem_size == 1, "%s: an element of %d bytes (float32: 4, uint8: 1)", what, elem_size);
    IPSX_REQUIRE(n_tables > 0 && n_tables <= COMMIT_MAX_TABLES, "%s: %d tables (1 .. %d in one launch)", what, n_tables, COMMIT_MAX_TABLES);
    IPSX_REQUIRE(b > 0 && m > 0 && rows_max >= 0 && piece_rows_total >= 0, "%s: bad sizes (b = %d, m = %d, %lld rows, a piece of %lld)",
                 what, b, m, (long long)rows_max, (long long)piece_rows_total);
    IPSX_REQUIRE(slides, "%s: null slide table", what);
    const int64_t total = ragged_view_total(view, what);
    if (total < 0) return IPSX_EINVAL;
    IPSX_REQUIRE(view->images, "%s: no device table", what);
    const ipsx_image_entry& back = view->host[view->b - 1];
    const long long eb = elem_size, seg = (long long)view->pw * eb;
    RaggedCommitViewArgs a;
    a.c.sel = reinterpret_cast<const long long*>(sel); a.c.slides = reinterpret_cast<const long long*>(slides);
    a.c.m = m; a.c.n_tables = n_tables; a.c.piece_rows = piece_rows_total;
    a.pixels = static_cast<const unsigned char*>(pixels); a.images = view->images;
    a.vb = view->b; a.vc = view->c; a.ph = view->ph; a.pw = view->pw; a.sh = view->sh; a.sw = view->sw;
    a.elem = elem_size; a.view_total = total;
    a.pixel_elems = back.elem_off + (long long)view->c * back.h * back.w;
    for (int k = 0; k < n_tables; ++k) {
        const ipsx_stream_table& s = tables[k];
        IPSX_TRY(ragged_commit_table(what, s, k, b, piece_rows_total, k == 0, a.c.t[k]));
        if (k) continue;
        // table 0: the patch table.  Its rows are whole patches of the view and nothing it writes lies inside the pixels
        IPSX_REQUIRE(s.row_bytes == (long long)view->c * view->ph * seg, "%s: rows of %lld bytes, a %dx%dx%d patch of %d-byte elements has %lld",
                     what, (long long)s.row_bytes, view->c, view->ph, view->pw, elem_size, (long long)view->c * view->ph * seg);
        IPSX_REQUIRE(!overlaps(s.dst, ((long long)(b - 1) * s.dst_bstride_rows + s.dst_rows) * s.row_bytes, pixels, a.pixel_elems * eb),
                     "%s: the destination overlaps the pixels", what);
        a.unit = 1;
        for (long long u : {16ll, 4ll})
            if (seg % u == 0 && multiple_of(s.dst, u) && (!s.held || multiple_of(s.held, u)) &&
                ragged_view_at_multiple(pixels, *view, (int)u, (size_t)elem_size)) {
                a.unit = (int)u;
                break;
            }
        a.c.t[0].unit = a.unit;                                   // (row_bytes is a multiple of seg: the held rows go the same width)
    }
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.c.t[k] = a.c.t[0];
    if (unit) *unit = a.unit;
    if (rows_max == 0) return IPSX_OK;
    IPSX_REQUIRE(rows_max < ((int64_t)1 << 31) && b < 65536, "%s: %lld rows x %d slides in one launch", what, (long long)rows_max, b);
    stream_commit_ragged_view_kernel<<<dim3((unsigned)rows_max, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched(what);
}
