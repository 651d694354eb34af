// stream.hip - the state update of the four stream routes (ips_amd/stream.py, ips_amd/ragged_stream.py; DESIGN 2.4, 2.5,
// 2.7, 2.10): after the iterations a feed has completed, the M winners and the not yet scored tail move to the front of the
// other buffer set - for up to four tables (patch rows, embeddings, logits, global ids) in ONE launch.  The candidates of a
// table are two segments that are never joined: the rows the stream holds, then the feed's piece.  Pure HBM-bound copy like
// gather.hip: one workgroup per (row, image, table), 16 / 4 / 1 bytes per lane as row size and addresses allow, source rows
// clamped into the candidates.
//
// One body, two axes.
//   Whose numbers: stream_commit_kernel has ONE n_cand and ONE tail_first for all images, and a table's piece has its own
//   base address and batch stride (a slice of a larger tensor is read where it lies).  stream_commit_ragged_kernel reads six
//   int64 words per slide from the device and the piece of a table is ONE packed tensor for all slides; what only the device
//   table says is checked per slide in the kernel (slide_numbers, table_takes_slide); a slide that contradicts the launch is not touched.
//   What the piece is: a tensor (A::VIEW false), or - for the PATCH table, table 0, of a stream fed pixel-row bands - no tensor
//   at all (A::VIEW true): the candidates behind the held rows are patches of whole images, read through an ipsx_patch_view
//   (uniform) or a ragged view over windows of different sizes (ragged) as c * ph segments of pw elements each, copied raw
//   (bytes stay bytes).  The other tables of such a launch keep their contiguous pieces.
// The view instantiations extend the argument struct of their sibling; the others neither carry nor read a view field.

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
    static constexpr bool VIEW = false;
    CommitTable t[COMMIT_MAX_TABLES];
    const long long* sel;      // (b, m) candidate rows of the new memory, or nullptr: append the piece behind the held rows
    int m;
    long long n_cand, tail_first;
};

// the patch table of a row stream: table 0's piece is (images, view) - candidate held_rows + r of image b is grid patch
// b * per_image + r.  unit: bytes per lane of THAT segment, uniform over the launch (host: images, w, sw, pw, dst, held).
struct CommitViewArgs : CommitArgs {
    static constexpr bool VIEW = true;
    const unsigned char* images;
    ipsx_patch_view v;
    int elem, unit;                                               // bytes per pixel (4 | 1); 16, 4 or 1 bytes per lane
    long long per_image;                                          // ny * nx
};

template <typename V>
__device__ __forceinline__ void copy_units(const unsigned char* s, unsigned char* d, long long units) {
    const V* sv = reinterpret_cast<const V*>(s);
    V* dv = reinterpret_cast<V*>(d);
    for (long long i = threadIdx.x; i < units; i += 256) dv[i] = sv[i];
}

__device__ __forceinline__ void copy_row(const unsigned char* s, unsigned char* d, long long row_bytes, int unit) {
    if (unit == 16) copy_units<uint4>(s, d, row_bytes / 16);
    else if (unit == 4) copy_units<uint32_t>(s, d, row_bytes / 4);
    else copy_units<unsigned char>(s, d, row_bytes);
}

// one patch out of its image - v: that image's c, h, w and the patch's ph, pw; the uniform kernel passes its view, the ragged
// one the entry it resolved - as c * ph segments of seg_units lanes; no load leaves its patch row
template <typename V>
__device__ __forceinline__ void copy_patch_units(const unsigned char* s, unsigned char* d, const ipsx_patch_view& v, int elem) {
    const unsigned seg_units = (unsigned)(v.pw * elem) / (unsigned)sizeof(V), total = (unsigned)(v.c * v.ph) * seg_units;
    const long long pitch = (long long)v.w * elem;                // bytes between two rows of the image
    V* dv = reinterpret_cast<V*>(d);
    for (unsigned i = threadIdx.x; i < total; i += 256) {
        const unsigned seg = i / seg_units, u = i - seg * seg_units, ch = seg / (unsigned)v.ph, y = seg - ch * (unsigned)v.ph;
        dv[i] = *reinterpret_cast<const V*>(s + ((long long)ch * v.h + y) * pitch + (size_t)u * sizeof(V));
    }
}

// The helpers below take what lies in the kernel arguments through pointers: a field is loaded on the path that needs it, not
// at the call ("One body, two axes").

// workgroup j of image b while a selection is committed -> the candidate row it reads: a winner, clamped into the n_cand
// candidates (never read out of bounds), or a row of the tail
__device__ __forceinline__ long long selected_row(const long long* sel, int b, const int* m, const long long* n_cand,
                                                   const long long* tail_first, long long j) {
    long long r;
    if (j < *m) {
        r = sel[(size_t)b * *m + j];
        r = r < 0 ? 0 : (r >= *n_cand ? *n_cand - 1 : r);
    } else {
        r = *tail_first + (j - *m);
    }
    return r;
}

// the row resolution of the uniform kernels -> does workgroup j have a row; r: candidate row read, out: row of dst written
// (workgroup-uniform).  No sel: append - the piece's rows go behind the held ones, in place.
__device__ __forceinline__ bool commit_row(const CommitArgs* a, const CommitTable* t, int b, long long j, long long& r, long long& out) {
    if (a->sel) {
        r = selected_row(a->sel, b, &a->m, &a->n_cand, &a->tail_first, j);
        out = j;
    } else {
        r = t->held_rows + j;
        if (r >= a->n_cand) return false;
        out = r;
    }
    return true;
}

template <typename A>
__global__ __launch_bounds__(256) void stream_commit_kernel(A a) {
    const CommitTable& t = a.t[blockIdx.z];
    const long long j = blockIdx.x;
    const int b = blockIdx.y;
    long long out, r;                                             // row of dst written, candidate row read (workgroup-uniform)
    if (!commit_row(&a, &t, b, j, r, out)) return;
    unsigned char* d;                                             // (formed in front of the patch branch, or behind s: DESIGN 2.4 says why)
    if constexpr (A::VIEW) {
        d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
        if (blockIdx.z == 0 && r >= t.held_rows) {                // a patch of the window (r - held_rows < per_image: host)
            long long off = patch_view_offset(a.v, (long long)b * a.per_image + (r - t.held_rows));
            if (off < 0) off = 0;
            const unsigned char* s = a.images + off * a.elem;
            if (a.unit == 16) copy_patch_units<uint4>(s, d, a.v, a.elem);
            else if (a.unit == 4) copy_patch_units<uint32_t>(s, d, a.v, a.elem);
            else copy_patch_units<unsigned char>(s, d, a.v, a.elem);
            return;
        }
    }
    const unsigned char* s = r < t.held_rows ? t.held + (size_t)b * t.held_bs + (size_t)r * t.row_bytes
                                             : t.piece + (size_t)b * t.piece_bs + (size_t)(r - t.held_rows) * t.row_bytes;
    if constexpr (!A::VIEW) d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
    copy_row(s, d, t.row_bytes, t.unit);
}

// ---- slides that each have their own numbers.  A table without a piece holds all of a slide's candidates itself (the
// logits table behind the loop).
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
    static constexpr bool VIEW = false;
    RaggedCommitTable t[COMMIT_MAX_TABLES];
    const long long* sel;      // (b, m) candidate rows of the slides that select, or nullptr
    const long long* slides;   // (b, 6): held rows, candidates, tail_first, the slide's first row in the packed piece, the mode, one reserved
    int m, n_tables;
    long long piece_rows;      // rows of the packed pieces
};

// the patch table of a ragged row stream: candidate held + r of slide k is packed patch first_k + r of a ragged view over the
// feed's packed pixel windows - word 3 of the slide's row means in the view what it means in the packed pieces of tables
// 1 .. - with the pitches of ITS image.  The image is found by the stems' bisection, on scalar registers: the patch number
// is workgroup-uniform, the lanes only copy.
struct RaggedCommitViewArgs : RaggedCommitArgs {
    static constexpr bool VIEW = true;
    const unsigned char* pixels;
    const ipsx_image_entry* images;                               // the view's DEVICE table, vb entries
    int vb, vc, ph, pw, sh, sw;
    int elem, unit;                                               // bytes per pixel (4 | 1); 16, 4 or 1 bytes per lane (host)
    long long view_total, pixel_elems;                            // packed patches of the view; elements of the pixel buffer (host table)
};

__device__ __forceinline__ long long uniform_ll(long long v) {
    return ((long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)v);
}

struct SlideNumbers {
    long long held, cand, tail_first, first;
    bool append, select;       // the mode (neither: move)
    long long rows, last;      // workgroups with a row; dst rows [.., last) are written
    long long piece_end;       // first + (cand - held): the slide's end in the packed pieces, or in the view
};

// The device-side guards, in two steps that every workgroup of a slide takes before it touches anything: one contradiction
// and the slide is left as it is in EVERY table of the launch.  With a view table 0's piece is the view: the table counts as
// having a piece, and the slide's rows behind its held ones are measured against the view's patch count, not the packed pieces.

// slide b's six words, read once onto scalar registers, against each other and the launch -> false: idle, an unknown mode, or
// numbers that contradict themselves
template <typename A>
__device__ __forceinline__ bool slide_numbers(const A* a, int b, SlideNumbers& n) {
    const long long* w = a->slides + (size_t)b * 6;
    const long long held = uniform_ll(w[0]), cand = uniform_ll(w[1]), tail_first = uniform_ll(w[2]), first = uniform_ll(w[3]),
                    mode = uniform_ll(w[4]);
    if (mode != COMMIT_APPEND && mode != COMMIT_SELECT && mode != COMMIT_MOVE) return false;
    const long long lim = 1ll << 40;                              // (sums below cannot overflow)
    if (!(held >= 0 && cand >= held && cand > 0 && cand < lim && first >= 0 && first < lim)) return false;
    if (mode == COMMIT_SELECT && !(a->sel && tail_first >= 0 && tail_first <= cand)) return false;
    const long long rows = mode == COMMIT_APPEND ? cand - held : (mode == COMMIT_SELECT ? a->m + (cand - tail_first) : cand);
    const long long last = mode == COMMIT_APPEND ? cand : rows;  // dst rows [.., last) are written
    const long long piece_end = first + (cand - held);
    if constexpr (A::VIEW)
        if (piece_end > a->view_total) return false;
    n.held = held; n.cand = cand; n.tail_first = tail_first; n.first = first; n.append = mode == COMMIT_APPEND; n.select = mode == COMMIT_SELECT;
    n.rows = rows; n.last = last; n.piece_end = piece_end;
    return true;
}

// ... and against table k of the launch: nothing is read outside its held rows or the packed pieces, nothing written outside dst_rows
template <bool view>
__device__ __forceinline__ bool table_takes_slide(const RaggedCommitArgs* a, int k, const SlideNumbers& n) {
    const RaggedCommitTable& c = a->t[k];
    const long long in_held = ((view && k == 0) || c.piece) ? n.held : n.cand;      // candidates of this table that lie in its held rows
    if (in_held > c.held_rows || n.last > c.dst_rows) return false;
    // (n.piece_end either way; without a view the sum is formed here, for the compiler to hoist out of the kernel's loop: DESIGN 2.4)
    const long long piece_end = view ? n.piece_end : n.first + (n.cand - n.held);
    if (!(view && k == 0) && c.piece && piece_end > a->piece_rows) return false;
    if (c.in_place && !n.append) return false;
    return true;
}

template <typename A>
__global__ __launch_bounds__(256) void stream_commit_ragged_kernel(A a) {
    const long long j = blockIdx.x;
    const int b = blockIdx.y;
    SlideNumbers n;
    if (!slide_numbers(&a, b, n)) return;
    for (int k = 0; k < a.n_tables; ++k)
        if (!table_takes_slide<A::VIEW>(&a, k, n)) return;
    if (j >= n.rows) return;
    const bool patches = A::VIEW && blockIdx.z == 0;
    const RaggedCommitTable& t = a.t[blockIdx.z];
    long long r, out;                                             // candidate row read, row of dst written (workgroup-uniform)
    if (n.append) {
        if (!patches && !t.piece) return;                         // (a table that holds its candidates has nothing to append)
        r = out = n.held + j;
    } else if (n.select) {
        r = selected_row(a.sel, b, &a.m, &n.cand, &n.tail_first, j);
        out = j;
    } else {
        r = out = j;
    }
    const long long in_held = (patches || t.piece) ? n.held : n.cand;
    unsigned char* d;                                             // (where it is formed: as in stream_commit_kernel)
    if constexpr (A::VIEW) {
        d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
        if (patches && r >= in_held) {                            // a patch of the view: first + (r - held) < view_total (slide_numbers)
            const long long p = uniform_ll(n.first + (r - in_held));
            int iw = 0, ih = 0;
            const long long off = uniform_ll(ragged_view_offset(a.images, a.vb, a.sh, a.sw, p, &iw, &ih));
            iw = __builtin_amdgcn_readfirstlane(iw); ih = __builtin_amdgcn_readfirstlane(ih);
            // the entry against the buffer the host measured: a device table that says otherwise is not followed out of it
            if (off < 0 || off >= a.pixel_elems || ih < a.ph || iw < a.pw || (long long)ih * iw > a.pixel_elems) return;
            if (off +((long long)(a.vc - 1) * ih + (a.ph - 1)) * iw + a.pw > a.pixel_elems) return;
            const unsigned char* s = a.pixels + off * a.elem;
            ipsx_patch_view v;                                    // the patch's image alone
            v.b = 1; v.c = a.vc; v.h = ih; v.w = iw; v.ph = a.ph; v.pw = a.pw; v.sh = a.sh; v.sw = a.sw;
            if (a.unit == 16) copy_patch_units<uint4>(s, d, v, a.elem);
            else if (a.unit == 4) copy_patch_units<uint32_t>(s, d, v, a.elem);
            else copy_patch_units<unsigned char>(s, d, v, a.elem);
            return;
        }
    }
    const unsigned char* s = r < in_held ? t.held + (size_t)b * t.held_bs + (size_t)r * t.row_bytes
                                         : t.piece + (size_t)(n.first + (r - in_held)) * t.row_bytes;
    if constexpr (!A::VIEW) d = t.dst + (size_t)b * t.dst_bs + (size_t)out * t.row_bytes;
    copy_row(s, d, t.row_bytes, t.unit);
}

}  // namespace ipsx

using namespace ipsx;

static bool overlaps(const void* p, long long p_bytes, const void* q, long long q_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q);
    return a < c + (uintptr_t)q_bytes && c < a + (uintptr_t)p_bytes;
}

// the widest of 16 / 4 / 1 bytes per lane that divides `bytes` and every stride and at which every pointer lies (null: not read)
static int lane_unit(long long bytes, std::initializer_list<const void*> ptrs, std::initializer_list<long long> strides = {}) {
    for (const long long u : {16ll, 4ll}) {
        bool fits = bytes % u == 0;
        for (const void* p : ptrs) fits = fits && (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(u - 1)) == 0;
        for (const long long s : strides) fits = fits && s % u == 0;
        if (fits) return (int)u;
    }
    return 1;
}

// what the four exports check first.  pixels_name: what a view flavour calls its pixel buffer (null: no view)
static int commit_head(const char* what, const ipsx_stream_table* tables, int n_tables, const char* pixels_name, const void* pixels,
                       const void* view, int elem_size) {
    IPSX_REQUIRE(tables, "%s: null tables", what);
    if (pixels_name) {
        IPSX_REQUIRE(pixels && view, "%s: null %s or view", what, pixels_name);
        IPSX_REQUIRE(elem_size == 4 || elem_size == 1, "%s: an element of %d bytes (float32: 4, uint8: 1)", what, elem_size);
    }
    IPSX_REQUIRE(n_tables > 0 && n_tables <= COMMIT_MAX_TABLES, "%s: %d tables (1 .. %d in one launch)", what, n_tables, COMMIT_MAX_TABLES);
    return IPSX_OK;
}

// table 0 of a view launch, the patch table: its rows are whole c x ph x pw patches of the view ...
static int view_patch_rows(const char* what, const ipsx_stream_table& s, int c, int ph, int pw, int elem_size) {
    const long long bytes = (long long)c * ph * pw * elem_size;
    IPSX_REQUIRE(s.row_bytes == bytes, "%s: rows of %lld bytes, a %dx%dx%d patch of %d-byte elements has %lld", what,
                 (long long)s.row_bytes, c, ph, pw, elem_size, bytes);
    return IPSX_OK;
}

// ... and none of the `written` rows per image it may write lies inside the pixels (in EVERY mode: they are read while dst is
// written) -> unit: the lanes of the launch's patch copies, no wider than view_unit, the widest load the view allows
// (row_bytes is a multiple of a segment: the held rows go the same width)
static int view_patch_unit(const char* what, const ipsx_stream_table& s, int b, long long written, int pw, int elem_size,
                           const char* pixels_name, const void* pixels, long long pixel_elems, int view_unit, int& unit) {
    IPSX_REQUIRE(!overlaps(s.dst, ((long long)(b - 1) * s.dst_bstride_rows + written) * s.row_bytes, pixels, pixel_elems * elem_size),
                 "%s: the destination overlaps the %s", what, pixels_name);
    unit = std::min(lane_unit((long long)pw * elem_size, {s.dst, s.held}), view_unit);
    return IPSX_OK;
}

// one table of a commit, checked and translated for the kernels.  rows: workgroups per image of a selection (m + tail).
// view_piece: the candidates behind the held rows are no tensor (the patch table of a view launch) - `piece` stays null and
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
    t.unit = view_piece ? 1 : lane_unit(s.row_bytes, {s.dst, s.held, s.piece}, {s.piece ? (long long)s.piece_bstride_bytes : 0});
    return IPSX_OK;
}

// The state update of a stream as ONE launch.  A: CommitArgs (images, v, unit: unused), or CommitViewArgs - table 0's piece
// is (images, view).  Everything is checked before the launch.
template <typename A>
static int stream_commit(const char* what, const ipsx_stream_table* tables, int n_tables, const void* images, const ipsx_patch_view* v,
                         int elem_size, const int64_t* sel, int b, int m, int64_t n_cand, int64_t tail_first, int* unit, void* stream) {
    IPSX_TRY(commit_head(what, tables, n_tables, A::VIEW ? "images" : nullptr, images, v, elem_size));
    IPSX_REQUIRE(b > 0 && m > 0 && n_cand > 0, "%s: bad sizes (b = %d, m = %d, %lld candidates)", what, b, m, (long long)n_cand);
    IPSX_REQUIRE(!sel || (tail_first >= 0 && tail_first <= n_cand), "%s: the tail starts at candidate %lld of %lld", what,
                 (long long)tail_first, (long long)n_cand);
    A a;
    if constexpr (A::VIEW) {
        IPSX_REQUIRE(patch_view_offset(*v, 0) >= 0, "%s: the view does not fit its images (%dx%dx%dx%d, patch %dx%d, stride %dx%d)", what,
                     v->b, v->c, v->h, v->w, v->ph, v->pw, v->sh, v->sw);
        IPSX_REQUIRE(v->b == b, "%s: a view of %d images in a call of %d", what, v->b, b);
        a.images = static_cast<const unsigned char*>(images); a.v = *v; a.elem = elem_size;
        a.per_image = (long long)((v->h - v->ph) / v->sh + 1) * ((v->w - v->pw) / v->sw + 1);
    }
    a.sel = reinterpret_cast<const long long*>(sel); a.m = m; a.n_cand = n_cand; a.tail_first = tail_first;
    long long rows = sel ? m + (n_cand - tail_first) : 0;         // workgroups per image and table
    for (int k = 0; k < n_tables; ++k) {
        const ipsx_stream_table& s = tables[k];
        IPSX_TRY(commit_table(what, s, k, sel != nullptr, b, n_cand, rows, A::VIEW && k == 0, a.t[k]));
        if (!sel) rows = std::max<long long>(rows, n_cand - s.held_rows);
        if constexpr (A::VIEW) {
            if (k) continue;
            IPSX_TRY(view_patch_rows(what, s, v->c, v->ph, v->pw, elem_size));
            // (the kernel numbers the patches of an image from 0: its piece is at most the view's patches per image)
            IPSX_REQUIRE(n_cand - s.held_rows <= a.per_image, "%s: %lld candidates behind the held rows, the view has %lld patches per image", what,
                         (long long)(n_cand - s.held_rows), a.per_image);
            IPSX_TRY(view_patch_unit(what, s, b, sel ? rows : n_cand, v->pw, elem_size, "images", images, (long long)v->b * v->c * v->h * v->w,
                                     view_load_width(images, *v, (size_t)elem_size, {16, 4, 1}), a.unit));
            a.t[0].unit = a.unit;
        }
    }
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.t[k] = a.t[0];
    if constexpr (A::VIEW)
        if (unit) *unit = a.unit;
    if (rows <= 0) return IPSX_OK;                                // nothing to append
    IPSX_REQUIRE(rows < ((int64_t)1 << 31) && b < 65536, "%s: %lld rows x %d images in one launch", what, rows, b);
    stream_commit_kernel<A><<<dim3((unsigned)rows, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched(what);
}

IPSX_API int ipsx_stream_commit(const ipsx_stream_table* tables, int n_tables, const int64_t* sel, int b, int m, int64_t n_cand,
                                int64_t tail_first, void* stream) {
    return stream_commit<CommitArgs>("stream_commit", tables, n_tables, nullptr, nullptr, 0, sel, b, m, n_cand, tail_first, nullptr, stream);
}

IPSX_API int ipsx_stream_commit_view(const ipsx_stream_table* tables, int n_tables, const void* images, const ipsx_patch_view* v,
                                     int elem_size, const int64_t* sel, int b, int m, int64_t n_cand, int64_t tail_first,
                                     int* unit, void* stream) {
    return stream_commit<CommitViewArgs>("stream_commit_view", tables, n_tables, images, v, elem_size, sel, b, m, n_cand, tail_first, unit,
                                         stream);
}

// one table of a ragged commit, checked and translated for the kernels.  view_piece: the candidates behind the held rows are
// patches of a ragged view (the patch table of a view launch) - `piece` stays null and the caller picks the lane width.
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
    t.unit = view_piece ? 1 : lane_unit(s.row_bytes, {s.dst, s.held, s.piece});
    return IPSX_OK;
}

// The state update of a ragged stream as ONE launch.  What the host can know is refused here; what only the device table
// says is checked per slide in the kernel.  A: RaggedCommitArgs (pixels, view, unit: unused), or RaggedCommitViewArgs - table
// 0's piece is (pixels, view); the view's HOST table is checked again and gives the patch count, the extent of the pixel
// buffer and the launch's load width.
template <typename A>
static int stream_commit_ragged(const char* what, const ipsx_stream_table* tables, int n_tables, const void* pixels,
                                const ipsx_ragged_view* view, int elem_size, const int64_t* sel, const int64_t* slides, int b, int m,
                                int64_t rows_max, int64_t piece_rows_total, int* unit, void* stream) {
    IPSX_TRY(commit_head(what, tables, n_tables, A::VIEW ? "pixels" : nullptr, pixels, view, elem_size));
    IPSX_REQUIRE(b > 0 && m > 0 && rows_max >= 0 && piece_rows_total >= 0, "%s: bad sizes (b = %d, m = %d, %lld rows, a piece of %lld)",
                 what, b, m, (long long)rows_max, (long long)piece_rows_total);
    IPSX_REQUIRE(slides, "%s: null slide table", what);
    A a;
    if constexpr (A::VIEW) {
        const int64_t total = ragged_view_total(view, what);
        if (total < 0) return IPSX_EINVAL;
        IPSX_REQUIRE(view->images, "%s: no device table", what);
        const ipsx_image_entry& back = view->host[view->b - 1];
        a.pixels = static_cast<const unsigned char*>(pixels); a.images = view->images;
        a.vb = view->b; a.vc = view->c; a.ph = view->ph; a.pw = view->pw; a.sh = view->sh; a.sw = view->sw;
        a.elem = elem_size; a.view_total = total;
        a.pixel_elems = back.elem_off + (long long)view->c * back.h * back.w;
    }
    a.sel = reinterpret_cast<const long long*>(sel); a.slides = reinterpret_cast<const long long*>(slides);
    a.m = m; a.n_tables = n_tables; a.piece_rows = piece_rows_total;
    for (int k = 0; k < n_tables; ++k) {
        const ipsx_stream_table& s = tables[k];
        IPSX_TRY(ragged_commit_table(what, s, k, b, piece_rows_total, A::VIEW && k == 0, a.t[k]));
        if constexpr (A::VIEW) {
            if (k) continue;
            IPSX_TRY(view_patch_rows(what, s, view->c, view->ph, view->pw, elem_size));
            IPSX_TRY(view_patch_unit(what, s, b, s.dst_rows, view->pw, elem_size, "pixels", pixels, a.pixel_elems,
                                     ragged_view_load_width(pixels, *view, (size_t)elem_size, {16, 4, 1}), a.unit));
            a.t[0].unit = a.unit;
        }
    }
    for (int k = n_tables; k < COMMIT_MAX_TABLES; ++k) a.t[k] = a.t[0];
    if constexpr (A::VIEW)
        if (unit) *unit = a.unit;
    if (rows_max == 0) return IPSX_OK;
    IPSX_REQUIRE(rows_max < ((int64_t)1 << 31) && b < 65536, "%s: %lld rows x %d slides in one launch", what, (long long)rows_max, b);
    stream_commit_ragged_kernel<A><<<dim3((unsigned)rows_max, (unsigned)b, (unsigned)n_tables), dim3(256), 0, as_stream(stream)>>>(a);
    return launched(what);
}

IPSX_API int ipsx_stream_commit_ragged(const ipsx_stream_table* tables, int n_tables, const int64_t* sel, const int64_t* slides,
                                       int b, int m, int64_t rows_max, int64_t piece_rows_total, void* stream) {
    return stream_commit_ragged<RaggedCommitArgs>("stream_commit_ragged", tables, n_tables, nullptr, nullptr, 0, sel, slides, b, m, rows_max,
                                                  piece_rows_total, nullptr, stream);
}

IPSX_API int ipsx_stream_commit_ragged_view(const ipsx_stream_table* tables, int n_tables, const void* pixels,
                                            const ipsx_ragged_view* view, int elem_size, const int64_t* sel, const int64_t* slides,
                                            int b, int m, int64_t rows_max, int64_t piece_rows_total, int* unit, void* stream) {
    return stream_commit_ragged<RaggedCommitViewArgs>("stream_commit_ragged_view", tables, n_tables, pixels, view, elem_size, sel, slides, b, m,
                                                      rows_max, piece_rows_total, unit, stream);
}
