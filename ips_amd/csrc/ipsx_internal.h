// ipsx_internal.h - what the translation units of libipsx call in each other (none of it is part of include/ipsx.h), and
// PatchSrc: the ONE description of where the patches of an image-encoder launch lie.
#pragma once

#include <initializer_list>

#include "ipsx_common.h"

namespace ipsx {

// ---- where the patches of a launch lie.  Patch j of the launch is patch index[j], or first + j, of
//   the patch tensor at `base`: float32, t->patch_dtype (fused split trunks) or - with `table` - uint8 whose values are
//   table[channel][byte]; or
//   the grid of `view` over the whole images at `base`: float32, or - with `table` - uint8 through the table.
//   the grids of `ragged` over images of different sizes packed into the buffer at `base`: float32, or - with
//   `table` - uint8 through the table; index and first count packed patches.
// A tensor that is read from patch k on has its base moved (`first` stays 0); only a view counts in `first`.
struct PatchSrc {
    const void* base;
    const float* table = nullptr;
    const ipsx_patch_view* view = nullptr;
    const int* index = nullptr;
    long long first = 0;
    const ipsx_ragged_view* ragged = nullptr;
};

// the source of patches k .. of this source - the remainder of a launch, a chunk, the second half of a call
static inline PatchSrc patch_src_from(const ipsx_trunk* t, PatchSrc s, int64_t k) {
    if (s.index) s.index += k;
    else if (s.view || s.ragged) s.first += k;
    else s.base = static_cast<const unsigned char*>(s.base) +
                  (size_t)k * t->c_in * t->h * t->w * (s.table ? 1 : (t->patch_dtype ? 2 : sizeof(float)));
    return s;
}

// the widest of `widths` (bytes per load, widest first) at which every patch row of the view starts: the images, their row
// pitch and the patches' column stride are all multiples of it; 0 when none is.  elem: bytes per pixel (4, or 1 with a table)
static inline int view_load_width(const void* base, const ipsx_patch_view& v, size_t elem, std::initializer_list<int> widths) {
    for (const int wd : widths)
        if (reinterpret_cast<uintptr_t>(base) % wd == 0 && (v.w * elem) % wd == 0 && (v.sw * elem) % wd == 0) return wd;
    return 0;
}

// what a view kernel gets beside its usual arguments, made by the launcher that knows its kernel's load widths (bytes, widest
// first).  float32 images: the one wide load, else 0 = dwords; uint8 images: a list that ends on 1, which always fits
static inline ViewArgs view_args(const PatchSrc& s, std::initializer_list<int> widths) {
    ViewArgs va;
    va.v = *s.view; va.index = s.index; va.first = s.first;
    va.wide = view_load_width(s.base, *s.view, s.table ? 1 : sizeof(float), widths);
    return va;
}

// ---- the ragged view (trunk.hip).  The checked HOST table of a view -> its total patch count, or -1 with the message set
// (`what`: the entry's name): what ipsx_ragged_view_fill accepts, asked again by every entry that is handed a view
int64_t ragged_view_total(const ipsx_ragged_view* rv, const char* what);
// can every patch row of the view be read by loads of `wd` bytes: the buffer, every image's offset and row pitch and the
// patches' column stride are multiples of it (the host knows the table it uploaded).  elem: bytes per pixel (4, or 1 for
// uint8 images - elem_off counts pixels, so a byte image's offset is its byte offset)
static inline bool ragged_view_at_multiple(const void* base, const ipsx_ragged_view& rv, int wd, size_t elem = sizeof(float)) {
    if (reinterpret_cast<uintptr_t>(base) % wd != 0 || (rv.sw * elem) % wd != 0) return false;
    for (int k = 0; k < rv.b; ++k)
        if ((rv.host[k].elem_off * (long long)elem) % wd != 0 || (rv.host[k].w * elem) % wd != 0) return false;
    return true;
}
// the widest of `widths` (bytes per load, widest first) at which every patch row of the ragged view starts; 0 when none does
static inline int ragged_view_load_width(const void* base, const ipsx_ragged_view& rv, size_t elem, std::initializer_list<int> widths) {
    for (const int wd : widths)
        if (ragged_view_at_multiple(base, rv, wd, elem)) return wd;
    return 0;
}
// what a ragged view kernel gets beside its usual arguments, made by the launcher that knows its kernel's load widths (bytes,
// widest first), as view_args: float32 images the one wide load, else 0 = dwords; uint8 images (s.table) a list that ends on
// 1, which always fits
static inline RaggedViewArgs ragged_view_args(const PatchSrc& s, std::initializer_list<int> widths) {
    RaggedViewArgs rv;
    rv.images = s.ragged->images; rv.b = s.ragged->b; rv.sh = s.ragged->sh; rv.sw = s.ragged->sw;
    rv.index = s.index; rv.first = s.first;
    rv.wide = ragged_view_load_width(s.base, *s.ragged, s.table ? 1 : sizeof(float), widths);
    return rv;
}
static inline RaggedViewArgs ragged_view_args(const PatchSrc& s, int widest) { return ragged_view_args(s, {widest}); }

// PARTS (ipsx_trunk_encode_parts): ONE launch encodes the index lists of every part of a call, one after the other, and says
// how far each part has come - done[k] counts the patches of part k whose embeddings are written AND visible to the whole
// device, so that a one-wave wait kernel on another stream (part_wait_kernel, scorer.hip) can let the part's logits and loop
// iterations go while later parts are still being encoded.  A launch boundary per part drains the chip.
struct PartsArgs {
    int* done;               // [parts] device counters, zeroed by the caller in front of the launch
    int parts;
    int part_end[16];        // exclusive prefix ends of the parts, in list entries
};
// fused_trunk.hip: the checked PartsArgs of a list of n entries (`what`: the entry's name in the messages)
int parts_args(PartsArgs& pa, int64_t n, const int64_t* part_end, int parts, int* done, const char* what);
// ... and what a counted launch asks of its trunk: precision 0, patch_dtype 0, the tile16 packing of the 128 -> 128 convolutions
int parts_trunk_check(const ipsx_trunk* t, const char* what);

// ---- the two exact fp32 trunk kernels share a list (fused_trunk.hip).  `count` entries on `cus` compute units: the first n8
// go through eight-patch workgroups (one per unit and round: a started round costs a whole one, 0.45 ms), the other count - n8
// through pair workgroups (fused_trunk_pair.h: a quarter round per unit each, 0.15 ms the layer).  n8 is the whole rounds when
// the remainder r = count % (8 cus) is at most PAIR_REST_NUM / PAIR_REST_DEN of a round, and the whole list otherwise.
// Measured (profiles/dedup_rounds_pair_table.txt): alone, the pair kernel is the faster one up to three quarters of a round
// (0.42 against 0.45 ms); inside a call its third layer of workgroups slows the selection loop that runs beside it by more
// than that, and only a remainder of up to half a round gains.  A pure function of the count: host (fused_launch) and device
// (the launches behind the blank scan, which alone know the count) agree, and both kernels give the same bits.
// mode (ipsx_dbg_fused_trunk_pair): 0 this rule, 1 n8 = count, 2 n8 = 0.
constexpr int PAIR_REST_NUM = 1, PAIR_REST_DEN = 2;
__host__ __device__ static inline long long trunk_pair_rest_max(int cus) { return 8ll * cus * PAIR_REST_NUM / PAIR_REST_DEN; }
__host__ __device__ static inline long long trunk_split_n8(long long count, int cus, int mode) {
    if (count <= 0 || mode == 2) return 0;
    if (mode == 1 || count > 0x7FFFFFFFll) return count;
    const unsigned r = (unsigned)count % (8u * (unsigned)cus);            // (32-bit: once per workgroup on the device)
    return (long long)r <= trunk_pair_rest_max(cus) ? count - r : count;
}
// ... and the pair workgroups a launch needs for a list of at most n entries whose length only the device knows
static inline long long trunk_split_pair_grid(long long n, int cus, int mode) {
    if (n <= 0 || mode == 1) return 0;
    const long long most = mode == 2 ? n : (n < trunk_pair_rest_max(cus) ? n : trunk_pair_rest_max(cus));
    return (most + 1) / 2;
}

static inline bool at_multiple(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// conv.hip (table: x holds uint8 elements)
int conv2d_affine_impl(const ipsx_conv* cv, const float* x, const float* residual, float* y, int64_t n, int h,
                       int w, int relu, int out_nhwc, void* stream, const float* table = nullptr);
// conv_nhwc.hip
int conv_nhwc_impl(const ipsx_conv* cv, const float* x, const float* residual, const float* row_stats, float* y,
                   int64_t n, int h, int w, int relu, void* stream, int* ready = nullptr, int ready_value = 0,
                   const int32_t* index = nullptr, int64_t src_rows = 0);
// conv_nhwc_bf16.hip: the pooled fp32 map rounded once to bf16 (count % 8 == 0)
int round_to_bf16(const float* x, void* y, size_t count, hipStream_t s);
// fused_stage.hip: the leading 64 -> 64 BasicBlocks on a small map, LDS-resident (50-px patches: 13x13)
int fused_stage64_blocks(const ipsx_block* blocks, int n_block, int h, int w);
int fused_stage64(const ipsx_block* blocks, int n_block, const float* x, float* y, int64_t n, int h, int w, hipStream_t s);
// ... and stem + max-pool of 1x50x50 / 3x100x100 patches -> (n, 13, 13, 64) / (n, 25, 25, 64) channels-last:
// 1 = ran, 0 = the trunk is another shape, -1 = failed
int fused_stem_pool50(const ipsx_trunk* t, const PatchSrc& src, float* y, int64_t n, hipStream_t s);
bool fused_stem_pool50_covers(const ipsx_trunk* t);
bool fused_stem_pool100x3_covers(const ipsx_trunk* t);
// fused_trunk.hip; count: a device-side number of patches (blank-patch dedup), stamps: diagnostic clocks per patch
bool fused_trunk_supported(const ipsx_trunk* t);
int fused_launch(const ipsx_trunk* t, const PatchSrc& src, int64_t n, float* emb, hipStream_t s, const int* count = nullptr,
                 unsigned long long* stamps = nullptr);
int fused_trunk_encode_parts(const ipsx_trunk* t, const PatchSrc& src, int64_t n, float* emb, const int64_t* part_end, int parts,
                             int* done, hipStream_t s);
// ... behind the blank scan (dedup.hip): only the list entries clist[0 .. *count) are encoded, clist[p] = (j, src.index[j]):
// that patch to emb row j, counted into the part j lies in; the other rows, and their share of done[], are the scan's
int fused_trunk_encode_parts_compact(const ipsx_trunk* t, const PatchSrc& src, int64_t n, float* emb, const int64_t* part_end,
                                     int parts, int* done, const int2* clist, const int* count, hipStream_t s);
int fused_trunk_stream(const ipsx_trunk* t, const float* patches, int64_t n, float* emb, const float* pos, const float* v_packed,
                       int r, float* logits, int32_t* ctl, int32_t* ready, int workgroups, int quad_pulls, hipStream_t s,
                       const int32_t* index = nullptr);
// dedup.hip: what stands behind the dedup exports among the ipsx_trunk_encode* family (trunk.hip); `what`: the entry's name
int encode_dedup(const ipsx_trunk* t, const PatchSrc& src, int64_t n_patch, const int32_t* flags, bool flagged, float* emb,
                 void* workspace, size_t workspace_bytes, int32_t* n_encoded, void* stream);
int encode_parts_dedup(const ipsx_trunk* t, const PatchSrc& src, bool u8, bool view, int64_t n_index, float* emb,
                       const int64_t* part_end, int n_parts, int32_t* done, const float* blank_emb, void* workspace,
                       size_t workspace_bytes, int32_t* n_encoded, void* stream, const char* what);
int encode_ragged_view_dedup(const ipsx_trunk* t, const void* pixels, const float* table, bool u8, const ipsx_ragged_view* view,
                             const int32_t* index, int64_t first, int64_t n, float* emb, void* workspace, size_t workspace_bytes,
                             int32_t* n_encoded, void* stream, const char* what);
// trunk.hip: a source of `n` patches against a trunk, once per entry (`what`: the entry's name in the message; `fused`:
// fused_trunk_supported(t))
int patch_src_check(const ipsx_trunk* t, const PatchSrc& src, int64_t n, bool fused, const char* what);

}  // namespace ipsx
