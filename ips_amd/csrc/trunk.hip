// trunk.hip - walks the nn.Sequential of IPSNet.get_conv_patch_enc (reference
// architecture/ips_net.py:35-50) over a batch of patches: stem conv 7x7/2 + BN +
// ReLU, max-pool 3x3/2, residual blocks, global average pool.
//
// Host-side runtime only: it sequences the kernels of conv.hip (or the fused
// LDS-resident kernel of fused_trunk.hip when the trunk matches it) on the
// caller's stream, in chunks of patches so the activation workspace stays bounded.
// At precision 1 (bf16) a layer-by-layer trunk keeps its fp32 stem and max-pool, rounds the pooled map once to bf16 and
// runs every convolution behind it through conv_nhwc_bf16.hip ("bf16 layered trunk").

#include <algorithm>
#include <cstdlib>

#include "ipsx_internal.h"

namespace ipsx {

struct TrunkGeom {
    size_t max_elems;   // largest per-patch activation (floats) of any layer
    int d_out;
};

static int trunk_geom(const ipsx_trunk* t, TrunkGeom* g) {
    IPSX_REQUIRE(t && t->n_block >= 0 && (t->n_block == 0 || t->blocks), "trunk: missing blocks");
    IPSX_REQUIRE(t->c_in > 0 && t->h > 0 && t->w > 0, "trunk: bad patch shape %dx%dx%d", t->c_in, t->h, t->w);
    IPSX_REQUIRE(t->stem.c_in == t->c_in, "trunk: stem expects %d channels, patches have %d", t->stem.c_in, t->c_in);
    int h = conv_out(t->h, t->stem.kh, t->stem.stride, t->stem.pad);
    int w = conv_out(t->w, t->stem.kw, t->stem.stride, t->stem.pad);
    IPSX_REQUIRE(h > 0 && w > 0, "trunk: patch too small");
    int c = t->stem.c_out;
    size_t mx = (size_t)c * h * w;
    h = conv_out(h, 3, 2, 1); w = conv_out(w, 3, 2, 1);
    for (int b = 0; b < t->n_block; ++b) {
        const ipsx_block& B = t->blocks[b];
        IPSX_REQUIRE(B.n_conv == 2 || B.n_conv == 3, "trunk: block %d has %d convs", b, B.n_conv);
        int ch = h, cw = w, cc = c;
        for (int j = 0; j < B.n_conv; ++j) {
            const ipsx_conv& cv = B.conv[j];
            IPSX_REQUIRE(cv.c_in == cc, "trunk: block %d conv %d expects %d channels, gets %d", b, j, cv.c_in, cc);
            IPSX_REQUIRE(cv.c_in % 32 == 0, "trunk: block %d conv %d has %d input channels (need a multiple of 32)", b, j, cv.c_in);
            ch = conv_out(ch, cv.kh, cv.stride, cv.pad); cw = conv_out(cw, cv.kw, cv.stride, cv.pad);
            IPSX_REQUIRE(ch > 0 && cw > 0, "trunk: feature map vanished in block %d", b);
            cc = cv.c_out;
            mx = std::max(mx, (size_t)cc * ch * cw);
        }
        if (B.has_down) {
            IPSX_REQUIRE(B.down.c_in == c && B.down.c_out == cc, "trunk: block %d shortcut shape", b);
            IPSX_REQUIRE(conv_out(h, B.down.kh, B.down.stride, B.down.pad) == ch, "trunk: block %d shortcut size", b);
        } else {
            IPSX_REQUIRE(cc == c && ch == h && cw == w, "trunk: block %d needs a projection shortcut", b);
        }
        h = ch; w = cw; c = cc;
    }
    g->max_elems = mx;
    g->d_out = c;
    return IPSX_OK;
}

// patches per chunk: 4 activation buffers of chunk*max_elems floats, <= 24 GiB in all.  Sized for 288 GB of HBM: the
// deep layers of a trunk have few output pixels per patch, and a chunk has to be large for THEM to fill 256 CUs
// (traffic signs, 512 channels at 4x4: 768 patches are 384 workgroups - fewer than the GPU runs at once)
// The budget is the smallest of: IPSX_TRUNK_WORKSPACE_MB (default 24576), 40 % of the device memory that is free right
// now (other processes / the training step's activations live there too).  ipsx_trunk_encode itself sizes its chunks
// from the workspace it is GIVEN, so a caller may hand over less than ipsx_trunk_workspace_bytes proposes.
static size_t trunk_budget() {
    size_t budget = (size_t)24 << 30;
    if (const char* e = getenv("IPSX_TRUNK_WORKSPACE_MB")) {
        const long long mb = atoll(e);
        if (mb > 0) budget = (size_t)mb << 20;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) budget = std::min(budget, free_b / 10 * 4);
    else (void)hipGetLastError();
    return budget;
}

static int64_t chunk_for(const TrunkGeom& g, int64_t n, size_t bytes) {
    int64_t cap = (int64_t)(bytes / (4 * g.max_elems * sizeof(float)));
    return std::min<int64_t>(n, cap);
}

static int64_t trunk_chunk(const TrunkGeom& g, int64_t n) {
    return std::max<int64_t>(chunk_for(g, n, trunk_budget()), 1);
}

// precision 1 on a layer-by-layer trunk: every convolution behind the stem runs conv_nhwc_bf16_kernel
static int layered_bf16_check(const ipsx_trunk* t) {
    IPSX_REQUIRE(t->stem.c_out % 8 == 0, "trunk (bf16): the stem has %d output channels (need a multiple of 8)", t->stem.c_out);
    for (int b = 0; b < t->n_block; ++b) {
        const ipsx_block& B = t->blocks[b];
        for (int j = 0; j < B.n_conv + (B.has_down ? 1 : 0); ++j) {
            const ipsx_conv& cv = j < B.n_conv ? B.conv[j] : B.down;
            const char* what = j < B.n_conv ? "conv" : "shortcut";
            IPSX_REQUIRE(cv.w_packed_bf16, "trunk (bf16): block %d %s %d has no w_packed_bf16 (ipsx_pack_conv_weight_bf16)", b, what, j);
            IPSX_REQUIRE(ipsx_conv2d_affine_nhwc_bf16_supported(&cv), "trunk (bf16): block %d %s %d, %d -> %d channels: the bf16 "
                         "convolution needs C_in %% 16 == 0 and C_out %% 8 == 0", b, what, j, cv.c_in, cv.c_out);
        }
    }
    return IPSX_OK;
}

static int64_t view_patches(const ipsx_patch_view& v) {
    return (int64_t)v.b * ((v.h - v.ph) / v.sh + 1) * ((v.w - v.pw) / v.sw + 1);
}

// Is `src` a source this trunk can encode `n` patches from?  Asked ONCE, by every entry, before its first launch.
int patch_src_check(const ipsx_trunk* t, const PatchSrc& src, int64_t n, bool fused, const char* what) {
    IPSX_REQUIRE(t->precision >= 0 && t->precision <= 2, "%s: precision %d", what, t->precision);
    IPSX_REQUIRE(t->patch_dtype >= 0 && t->patch_dtype <= 2, "%s: patch_dtype %d", what, t->patch_dtype);
    IPSX_REQUIRE(t->precision != 2 || fused, "%s: fp32x3 exists for the fused 1x32x32 trunk only", what);
    IPSX_REQUIRE(t->patch_dtype == 0 || (fused && t->precision != 0), "%s: the stem kernels of the layer-by-layer trunk "
                 "(stem_pool50_kernel, stem_pool100x3_kernel, conv_any_kernel) read float32 patches; half-precision patch storage "
                 "exists for the fused 1x32x32 trunk at precision 1 (bf16) / 2 (fp32x3) only", what);
    if (src.table && (src.view || src.ragged)) {
        // whole uint8 images: the byte tier of the view kernels takes any image address (view_args, ragged_view_args), the table
        // copy is 16-byte loads
        IPSX_REQUIRE(t->precision == 0 && t->patch_dtype == 0, "%s: uint8 images go with the exact fp32 trunk only (precision 0, "
                     "patch_dtype 0), got precision %d, patch_dtype %d", what, t->precision, t->patch_dtype);
        IPSX_REQUIRE(at_multiple(src.table, 16), "%s: the table of uint8 images must lie at a 16-byte address", what);
    } else if (src.table) {
        IPSX_REQUIRE(t->precision == 0 && t->patch_dtype == 0, "%s: uint8 patches go with the exact fp32 trunk only (precision 0, "
                     "patch_dtype 0), got precision %d, patch_dtype %d", what, t->precision, t->patch_dtype);
        // what each stem's byte loads need (the generic stem gathers byte by byte); the layered stems' codes are those
        // their launcher used to hand up
        if (fused)
            IPSX_REQUIRE(at_multiple(src.base, 16) && at_multiple(src.table, 16),
                         "fused trunk: uint8 patches and their table must lie at 16-byte addresses");
        else if (fused_stem_pool100x3_covers(t) && !(at_multiple(src.base, 16) && at_multiple(src.table, 16)))
            return fail(IPSX_EHIP, "stem_pool100x3: uint8 patches and their table must lie at 16-byte addresses");
        else if (fused_stem_pool50_covers(t) && !(at_multiple(src.base, 4) && at_multiple(src.table, 16)))
            return fail(IPSX_EHIP, "stem_pool50: uint8 patches must lie at a 4-byte address, their table at a 16-byte address");
    }
    if (src.view) {
        IPSX_REQUIRE(src.table || at_multiple(src.base, 4), "%s: images must lie at a 4-byte address", what);
        IPSX_REQUIRE(ipsx_trunk_view_supported(t, src.view), "%s: the exact fp32 trunks whose stem stages its patch into LDS "
                     "(1x32x32 fused, 1x50x50, 3x100x100) on a valid view of their patch shape (ipsx_trunk_view_supported)", what);
        IPSX_REQUIRE(src.index || src.first + n <= view_patches(*src.view), "%s: patches %lld .. %lld of a grid of %lld", what,
                     src.first, (long long)(src.first + n), (long long)view_patches(*src.view));
    }
    if (src.ragged) {
        IPSX_REQUIRE(!src.view, "%s: a ragged view is no ipsx_patch_view", what);
        IPSX_REQUIRE(src.table || at_multiple(src.base, 4), "%s: images must lie at a 4-byte address", what);
        const int64_t total = ragged_view_total(src.ragged, what);
        if (total < 0) return IPSX_EINVAL;
        IPSX_REQUIRE(src.ragged->images, "%s: no device table", what);
        IPSX_REQUIRE(ipsx_trunk_ragged_view_supported(t, src.ragged), "%s: the exact fp32 trunks whose stem stages its patch into "
                     "LDS (1x32x32 fused, 1x50x50, 3x100x100) on a ragged view of their patch shape "
                     "(ipsx_trunk_ragged_view_supported)", what);
        IPSX_REQUIRE(src.index ? n <= 0x7FFFFFF0ll : src.first + n <= total, "%s: packed patches %lld .. %lld of %lld", what,
                     src.first, (long long)(src.first + n), (long long)total);
    }
    return IPSX_OK;
}

// The checked host table of a ragged view -> the total patch count, or -1
int64_t ragged_view_total(const ipsx_ragged_view* rv, const char* what) {
    if (!rv || !rv->host || rv->b <= 0 || rv->c <= 0 || rv->ph <= 0 || rv->pw <= 0 || rv->sh <= 0 || rv->sw <= 0) {
        fail(IPSX_EINVAL, "%s: a ragged view needs a host table and positive b, c, patch and stride", what);
        return -1;
    }
    int64_t total = 0, end = 0;                            // packed patches so far; the element behind the last image
    for (int k = 0; k < rv->b; ++k) {
        const ipsx_image_entry& e = rv->host[k];
        if (e.h <= 0 || e.w <= 0 || rv->ph > e.h || rv->pw > e.w) {
            fail(IPSX_EINVAL, "%s: image %d is %dx%d, the patch %dx%d", what, k, e.h, e.w, rv->ph, rv->pw);
            return -1;
        }
        if (e.ny != (e.h - rv->ph) / rv->sh + 1 || e.nx != (e.w - rv->pw) / rv->sw + 1 || e.first != total) {
            fail(IPSX_EINVAL, "%s: image %d: the entry's grid %dx%d from patch %lld is not the geometry's", what, k, e.ny, e.nx,
                 (long long)e.first);
            return -1;
        }
        if (e.elem_off < end) {
            fail(IPSX_EINVAL, "%s: image %d at element %lld lies inside or in front of the image before it (ends at %lld)", what, k,
                 (long long)e.elem_off, (long long)end);
            return -1;
        }
        end = e.elem_off + (int64_t)rv->c * e.h * e.w;
        total += (int64_t)e.ny * e.nx;
        if (total > 0x7FFFFFFFll) {
            fail(IPSX_EINVAL, "%s: more than 2^31 - 1 patches", what);
            return -1;
        }
    }
    return total;
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API size_t ipsx_trunk_workspace_bytes(const ipsx_trunk* t, int64_t n_patch) {
    TrunkGeom g;
    if (trunk_geom(t, &g) != IPSX_OK || n_patch <= 0) return 0;
    if (fused_trunk_supported(t)) return 0;
    return (size_t)trunk_chunk(g, n_patch) * g.max_elems * sizeof(float) * 4;
}

IPSX_API const char* ipsx_trunk_kernel(const ipsx_trunk* t) {
    if (t && fused_trunk_supported(t))
        return t->precision == 2 ? "fused_trunk_x3_kernel" : (t->precision == 1 ? "fused_trunk_bf16_kernel" : "fused_trunk_kernel");
    if (t && t->n_block >= 2 && fused_stem_pool50_covers(t) &&
        fused_stage64_blocks(t->blocks, t->n_block, 13, 13) > 0)          // the reference's shipped 50-px Megapixel-MNIST trunk
        return t->precision == 1 ? "stem_pool50_kernel + conv_nhwc_bf16_kernel (layer by layer, bf16)"
                                 : "stem_pool50_kernel + fused_stage64_kernel (layer1, LDS-resident) + conv_nhwc_kernel (layer2, layer by layer)";
    if (t && t->precision == 1 && fused_stem_pool50_covers(t))
        return "stem_pool50_kernel + conv_nhwc_bf16_kernel (layer by layer, bf16)";
    if (t && fused_stem_pool100x3_covers(t))                               // the traffic-sign trunk: fused stem + pool, then layer by layer
        return t->precision == 1 ? "stem_pool100x3_kernel + conv_nhwc_bf16_kernel (layer by layer, bf16)"
                                 : "stem_pool100x3_kernel + conv_nhwc_kernel (layer by layer)";
    if (t && t->precision == 1) return "conv_any_kernel (stem) + conv_nhwc_bf16_kernel (layer by layer, bf16)";
    return "conv_nhwc_kernel (layer by layer)";
}

// an export's own first refusal, where it has one: "<its name>: <text>" unless ok
struct Need {
    bool ok = true;
    const char* text = "";
};

// The one path behind ipsx_trunk_encode, _view, _ragged_view and their _u8 twins: `n_patch` patches of `src` -> emb; only the
// stem's load differs
static int trunk_encode(const ipsx_trunk* t, const PatchSrc& src, int64_t n_patch, float* emb, void* workspace,
                        size_t workspace_bytes, void* stream, const char* what, Need need = Need()) {
    IPSX_REQUIRE(need.ok, "%s: %s", what, need.text);
    TrunkGeom g;
    IPSX_TRY(trunk_geom(t, &g));
    IPSX_REQUIRE(src.base && emb && n_patch >= 0, "%s: bad arguments", what);
    const bool fused = fused_trunk_supported(t);
    IPSX_TRY(patch_src_check(t, src, n_patch, fused, what));
    const bool bf16 = t->precision == 1 && !fused;       // ("bf16 layered trunk")
    if (bf16) IPSX_TRY(layered_bf16_check(t));
    if (n_patch == 0) return IPSX_OK;
    if (fused) return fused_launch(t, src, n_patch, emb, as_stream(stream));

    const int64_t chunk = workspace ? chunk_for(g, n_patch, workspace_bytes) : 0;      // chunks fit what the caller gave
    if (chunk < 1)
        return fail(IPSX_EWORKSPACE, "trunk_encode: workspace %zu B < %zu B (one patch)", workspace_bytes,
                    g.max_elems * sizeof(float) * 4);
    const size_t buf_elems = (size_t)chunk * g.max_elems;
    float* buf[4];
    for (int i = 0; i < 4; ++i) buf[i] = static_cast<float*>(workspace) + i * buf_elems;
    // bf16: the same workspace and the same chunks - four bf16 activation buffers in its first half, the fp32 stem output
    // and pooled map in its second (2 + 2 + 4 + 4 bytes x chunk x max_elems of the 16 it has)
    unsigned short* hb[4];
    for (int i = 0; i < 4; ++i) hb[i] = static_cast<unsigned short*>(workspace) + i * buf_elems;
    if (bf16) { buf[0] = static_cast<float*>(workspace) + 2 * buf_elems; buf[1] = buf[0] + buf_elems; }

    for (int64_t p0 = 0; p0 < n_patch; p0 += chunk) {
        const int64_t n = std::min(chunk, n_patch - p0);
        int h = conv_out(t->h, t->stem.kh, t->stem.stride, t->stem.pad);
        int w = conv_out(t->w, t->stem.kw, t->stem.stride, t->stem.pad);
        int c = t->stem.c_out;
        // stem reads the NCHW patches (the chunk's: the source from patch p0 on) and writes channels-last; everything after
        // it is channels-last
        const PatchSrc chunk_src = patch_src_from(t, src, p0);
        const int fused_stem = fused_stem_pool50(t, chunk_src, buf[1], n, as_stream(stream));
        if (fused_stem < 0) return IPSX_EHIP;
        if (!fused_stem) {
            IPSX_TRY(conv2d_affine_impl(&t->stem, static_cast<const float*>(chunk_src.base), nullptr, buf[0], n, t->h, t->w, 1, 1,
                                        stream, src.table));
            IPSX_TRY(ipsx_maxpool_3x3s2_nhwc(buf[0], buf[1], n, c, h, w, stream));
        }
        h = conv_out(h, 3, 2, 1); w = conv_out(w, 3, 2, 1);
        if (bf16) {
            // the pooled map (the fp32 kernels' bits) rounded ONCE to bf16; from here on activations are bf16 in HBM
            IPSX_TRY(round_to_bf16(buf[1], hb[1], (size_t)n * h * w * c, as_stream(stream)));
            int cur = 1;
            for (int b = 0; b < t->n_block; ++b) {
                const ipsx_block& B = t->blocks[b];
                int fr[3], k = 0;
                for (int i = 0; i < 4; ++i) if (i != cur) fr[k++] = i;
                const unsigned short* src = hb[cur];
                int ch = h, cw = w, si = -1;
                for (int j = 0; j < B.n_conv - 1; ++j) {   // conv -> BN -> ReLU
                    const ipsx_conv& cv = B.conv[j];
                    const int di = (si == fr[0]) ? fr[1] : fr[0];
                    IPSX_TRY(ipsx_conv2d_affine_nhwc_bf16(&cv, src, nullptr, hb[di], n, ch, cw, 1, stream));
                    ch = conv_out(ch, cv.kh, cv.stride, cv.pad); cw = conv_out(cw, cv.kw, cv.stride, cv.pad);
                    src = hb[di]; si = di;
                }
                const ipsx_conv& last = B.conv[B.n_conv - 1];
                const unsigned short* shortcut = hb[cur];  // the STORED bf16 block input (or projection output)
                if (B.has_down) {
                    IPSX_TRY(ipsx_conv2d_affine_nhwc_bf16(&B.down, hb[cur], nullptr, hb[fr[2]], n, h, w, 0, stream));
                    shortcut = hb[fr[2]];
                }
                const int oi = (si == fr[0]) ? fr[1] : fr[0];
                IPSX_TRY(ipsx_conv2d_affine_nhwc_bf16(&last, src, shortcut, hb[oi], n, ch, cw, 1, stream));
                h = conv_out(ch, last.kh, last.stride, last.pad); w = conv_out(cw, last.kw, last.stride, last.pad);
                c = last.c_out;
                cur = oi;
            }
            IPSX_TRY(ipsx_avgpool_nhwc_bf16(hb[cur], emb + (size_t)p0 * g.d_out, n, c, h * w, stream));
            continue;
        }
        int cur = 1;                                   // buf[cur] holds the block input
        int b_first = 0;
        if (c == 64) {                                 // layer1 on a small map: all of its convolutions in one LDS-resident kernel
            const int nf = fused_stage64_blocks(t->blocks, t->n_block, h, w);
            if (nf > 0) {
                IPSX_TRY(fused_stage64(t->blocks, nf, buf[1], buf[0], n, h, w, as_stream(stream)));
                cur = 0;
                b_first = nf;
            }
        }
        for (int b = b_first; b < t->n_block; ++b) {
            const ipsx_block& B = t->blocks[b];
            // free buffers: the three that are not `cur`
            int fr[3], k = 0;
            for (int i = 0; i < 4; ++i) if (i != cur) fr[k++] = i;
            const float* src = buf[cur];
            int ch = h, cw = w, si = -1;
            for (int j = 0; j < B.n_conv - 1; ++j) {   // conv -> BN -> ReLU
                const ipsx_conv& cv = B.conv[j];
                const int di = (si == fr[0]) ? fr[1] : fr[0];
                IPSX_TRY(ipsx_conv2d_affine_nhwc(&cv, src, nullptr, buf[di], n, ch, cw, 1, stream));
                ch = conv_out(ch, cv.kh, cv.stride, cv.pad); cw = conv_out(cw, cv.kw, cv.stride, cv.pad);
                src = buf[di]; si = di;
            }
            const ipsx_conv& last = B.conv[B.n_conv - 1];
            const float* shortcut = buf[cur];
            if (B.has_down) {                          // 1x1 strided conv + BN on the identity path
                IPSX_TRY(ipsx_conv2d_affine_nhwc(&B.down, buf[cur], nullptr, buf[fr[2]], n, h, w, 0, stream));
                shortcut = buf[fr[2]];
            }
            const int oi = (si == fr[0]) ? fr[1] : fr[0];
            // last conv -> BN -> += identity -> ReLU
            IPSX_TRY(ipsx_conv2d_affine_nhwc(&last, src, shortcut, buf[oi], n, ch, cw, 1, stream));
            h = conv_out(ch, last.kh, last.stride, last.pad); w = conv_out(cw, last.kw, last.stride, last.pad);
            c = last.c_out;
            cur = oi;
        }
        IPSX_TRY(ipsx_avgpool_nhwc(buf[cur], emb + (size_t)p0 * g.d_out, n, c, h * w, stream));
    }
    return IPSX_OK;
}

// An index list into a patch tensor, one launch of the fused trunk (ipsx_trunk_encode_indexed, _u8: the table must be there)
static int trunk_encode_indexed(const ipsx_trunk* t, const PatchSrc& src, bool u8, int64_t n_index, float* emb, void* stream,
                                const char* what) {
    IPSX_REQUIRE(t && src.base && (!u8 || src.table) && src.index && emb && n_index >= 0, "%s: bad arguments", what);
    IPSX_REQUIRE(fused_trunk_supported(t), "%s: only the fused 1x32x32 trunk is supported", what);
    IPSX_TRY(patch_src_check(t, src, n_index, true, what));
    if (n_index == 0) return IPSX_OK;
    return fused_launch(t, src, n_index, emb, as_stream(stream));
}

// The counted launch (ipsx_trunk_encode_parts and its _u8 / _view / _view_u8 twins), shaped like encode_parts_dedup.  Float32
// patches are checked by the launch alone; the view entries say more of a trunk that is not the fused one.
static int trunk_encode_parts(const ipsx_trunk* t, const PatchSrc& src, bool u8, bool view, int64_t n_index, float* emb,
                              const int64_t* part_end, int n_parts, int32_t* done, void* stream, const char* what) {
    IPSX_REQUIRE(t && src.base && (!u8 || src.table) && (!view || src.view) && src.index && emb && part_end && done,
                 "%s: null pointer", what);
    IPSX_REQUIRE(fused_trunk_supported(t), view ? "%s: the fused fp32 1x32x32 trunk on a valid view of 1x32x32 patches only"
                                                : "%s: only the fused 1x32x32 trunk is supported", what);
    if (u8 || view) IPSX_TRY(patch_src_check(t, src, n_index, true, what));
    return fused_trunk_encode_parts(t, src, n_index, emb, part_end, n_parts, done, as_stream(stream));
}

// ---- the ipsx_trunk_encode* exports, all twenty: a source and one call each.  Behind them stand trunk_encode,
// trunk_encode_indexed and trunk_encode_parts above and, in dedup.hip, encode_parts_dedup, encode_dedup and
// encode_ragged_view_dedup.  A view's `first` counts only without an index list.
IPSX_API int ipsx_trunk_encode(const ipsx_trunk* t, const float* patches, int64_t n_patch, float* emb,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return trunk_encode(t, PatchSrc{patches}, n_patch, emb, workspace, workspace_bytes, stream, "trunk_encode");
}

IPSX_API int ipsx_trunk_encode_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, int64_t n_patch, float* emb,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    return trunk_encode(t, PatchSrc{patches, table}, n_patch, emb, workspace, workspace_bytes, stream, "trunk_encode_u8",
                        Need{table != nullptr, "no table"});
}

IPSX_API int ipsx_trunk_encode_view(const ipsx_trunk* t, const float* images, const ipsx_patch_view* v, const int32_t* index,
                                    int64_t first, int64_t n, float* emb, void* workspace, size_t workspace_bytes, void* stream) {
    return trunk_encode(t, PatchSrc{images, nullptr, v, index, index ? 0 : first}, n, emb, workspace, workspace_bytes, stream,
                        "trunk_encode_view", Need{t && images && v && emb && n >= 0 && first >= 0, "bad arguments"});
}

IPSX_API int ipsx_trunk_encode_view_u8(const ipsx_trunk* t, const uint8_t* images, const float* table, const ipsx_patch_view* v,
                                       const int32_t* index, int64_t first, int64_t n, float* emb, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return trunk_encode(t, PatchSrc{images, table, v, index, index ? 0 : first}, n, emb, workspace, workspace_bytes, stream,
                        "trunk_encode_view_u8", Need{t && images && table && v && emb && n >= 0 && first >= 0, "bad arguments"});
}

IPSX_API int ipsx_trunk_encode_ragged_view(const ipsx_trunk* t, const float* pixels, const ipsx_ragged_view* view,
                                           const int32_t* index, int64_t first, int64_t n, float* emb, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    return trunk_encode(t, PatchSrc{pixels, nullptr, nullptr, index, index ? 0 : first, view}, n, emb, workspace, workspace_bytes,
                        stream, "trunk_encode_ragged_view", Need{t && pixels && view && emb && n >= 0 && first >= 0, "bad arguments"});
}

IPSX_API int ipsx_trunk_encode_ragged_view_u8(const ipsx_trunk* t, const uint8_t* pixels, const float* table,
                                              const ipsx_ragged_view* view, const int32_t* index, int64_t first, int64_t n,
                                              float* emb, void* workspace, size_t workspace_bytes, void* stream) {
    return trunk_encode(t, PatchSrc{pixels, table, nullptr, index, index ? 0 : first, view}, n, emb, workspace, workspace_bytes,
                        stream, "trunk_encode_ragged_view_u8",
                        Need{t && pixels && table && view && emb && n >= 0 && first >= 0, "bad arguments"});
}

IPSX_API int ipsx_trunk_encode_indexed(const ipsx_trunk* t, const float* patches, const int32_t* index,
                                       int64_t n_index, float* emb, void* stream) {
    return trunk_encode_indexed(t, PatchSrc{patches, nullptr, nullptr, index}, false, n_index, emb, stream, "trunk_encode_indexed");
}

IPSX_API int ipsx_trunk_encode_indexed_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, const int32_t* index,
                                          int64_t n_index, float* emb, void* stream) {
    return trunk_encode_indexed(t, PatchSrc{patches, table, nullptr, index}, true, n_index, emb, stream, "trunk_encode_indexed_u8");
}

IPSX_API int ipsx_trunk_encode_parts(const ipsx_trunk* t, const float* patches, const int32_t* index, int64_t n_index,
                                     float* emb, const int64_t* part_end, int n_parts, int32_t* done, void* stream) {
    return trunk_encode_parts(t, PatchSrc{patches, nullptr, nullptr, index}, false, false, n_index, emb, part_end, n_parts, done,
                              stream, "trunk_encode_parts");
}

IPSX_API int ipsx_trunk_encode_parts_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, const int32_t* index,
                                        int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                        void* stream) {
    return trunk_encode_parts(t, PatchSrc{patches, table, nullptr, index}, true, false, n_index, emb, part_end, n_parts, done, stream,
                              "trunk_encode_parts_u8");
}

IPSX_API int ipsx_trunk_encode_parts_view(const ipsx_trunk* t, const float* images, const ipsx_patch_view* v, const int32_t* index,
                                          int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                          void* stream) {
    return trunk_encode_parts(t, PatchSrc{images, nullptr, v, index}, false, true, n_index, emb, part_end, n_parts, done, stream,
                              "trunk_encode_parts_view");
}

IPSX_API int ipsx_trunk_encode_parts_view_u8(const ipsx_trunk* t, const uint8_t* images, const float* table,
                                             const ipsx_patch_view* v, const int32_t* index, int64_t n_index, float* emb,
                                             const int64_t* part_end, int n_parts, int32_t* done, void* stream) {
    return trunk_encode_parts(t, PatchSrc{images, table, v, index}, true, true, n_index, emb, part_end, n_parts, done, stream,
                              "trunk_encode_parts_view_u8");
}

IPSX_API int ipsx_trunk_encode_parts_dedup(const ipsx_trunk* t, const float* patches, const int32_t* index, int64_t n_index,
                                           float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                           const float* blank_emb, void* workspace, size_t workspace_bytes, int32_t* n_encoded,
                                           void* stream) {
    return encode_parts_dedup(t, PatchSrc{patches, nullptr, nullptr, index}, false, false, n_index, emb, part_end, n_parts, done,
                              blank_emb, workspace, workspace_bytes, n_encoded, stream, "trunk_encode_parts_dedup");
}

IPSX_API int ipsx_trunk_encode_parts_dedup_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, const int32_t* index,
                                              int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                              const float* blank_emb, void* workspace, size_t workspace_bytes,
                                              int32_t* n_encoded, void* stream) {
    return encode_parts_dedup(t, PatchSrc{patches, table, nullptr, index}, true, false, n_index, emb, part_end, n_parts, done,
                              blank_emb, workspace, workspace_bytes, n_encoded, stream, "trunk_encode_parts_dedup_u8");
}

IPSX_API int ipsx_trunk_encode_parts_dedup_view(const ipsx_trunk* t, const float* images, const ipsx_patch_view* v,
                                                const int32_t* index, int64_t n_index, float* emb, const int64_t* part_end,
                                                int n_parts, int32_t* done, const float* blank_emb, void* workspace,
                                                size_t workspace_bytes, int32_t* n_encoded, void* stream) {
    return encode_parts_dedup(t, PatchSrc{images, nullptr, v, index}, false, true, n_index, emb, part_end, n_parts, done,
                              blank_emb, workspace, workspace_bytes, n_encoded, stream, "trunk_encode_parts_dedup_view");
}

IPSX_API int ipsx_trunk_encode_parts_dedup_view_u8(const ipsx_trunk* t, const uint8_t* images, const float* table,
                                                   const ipsx_patch_view* v, const int32_t* index, int64_t n_index, float* emb,
                                                   const int64_t* part_end, int n_parts, int32_t* done, const float* blank_emb,
                                                   void* workspace, size_t workspace_bytes, int32_t* n_encoded, void* stream) {
    return encode_parts_dedup(t, PatchSrc{images, table, v, index}, true, true, n_index, emb, part_end, n_parts, done,
                              blank_emb, workspace, workspace_bytes, n_encoded, stream, "trunk_encode_parts_dedup_view_u8");
}

IPSX_API int ipsx_trunk_encode_dedup(const ipsx_trunk* t, const float* patches, int64_t n_patch, float* emb,
                                     void* workspace, size_t workspace_bytes, int32_t* n_encoded, void* stream) {
    return encode_dedup(t, PatchSrc{patches}, n_patch, nullptr, false, emb, workspace, workspace_bytes, n_encoded, stream);
}

IPSX_API int ipsx_trunk_encode_dedup_flagged(const ipsx_trunk* t, const float* patches, int64_t n_patch,
                                             const int32_t* nonblank, float* emb, void* workspace,
                                             size_t workspace_bytes, int32_t* n_encoded, void* stream) {
    return encode_dedup(t, PatchSrc{patches}, n_patch, nonblank, true, emb, workspace, workspace_bytes, n_encoded, stream);
}

IPSX_API int ipsx_trunk_encode_ragged_view_dedup(const ipsx_trunk* t, const float* pixels, const ipsx_ragged_view* view,
                                                 const int32_t* index, int64_t first, int64_t n, float* emb, void* workspace,
                                                 size_t workspace_bytes, int32_t* n_encoded, void* stream) {
    return encode_ragged_view_dedup(t, pixels, nullptr, false, view, index, first, n, emb, workspace, workspace_bytes, n_encoded,
                                    stream, "trunk_encode_ragged_view_dedup");
}

IPSX_API int ipsx_trunk_encode_ragged_view_dedup_u8(const ipsx_trunk* t, const uint8_t* pixels, const float* table,
                                                    const ipsx_ragged_view* view, const int32_t* index, int64_t first, int64_t n,
                                                    float* emb, void* workspace, size_t workspace_bytes, int32_t* n_encoded,
                                                    void* stream) {
    return encode_ragged_view_dedup(t, pixels, table, true, view, index, first, n, emb, workspace, workspace_bytes, n_encoded, stream,
                                    "trunk_encode_ragged_view_dedup_u8");
}

// ---- the patch-grid view (3.06): whole images in place of the patch tensor
IPSX_API int64_t ipsx_patch_view_offset(const ipsx_patch_view* v, int64_t p) { return v ? patch_view_offset(*v, p) : -1; }

IPSX_API int ipsx_trunk_view_supported(const ipsx_trunk* t, const ipsx_patch_view* v) {
    if (!t || !v || patch_view_offset(*v, 0) < 0) return 0;
    if (t->precision != 0 || t->patch_dtype != 0) return 0;
    if (v->c != t->c_in || v->ph != t->h || v->pw != t->w) return 0;
    return fused_trunk_supported(t) || fused_stem_pool50_covers(t) || fused_stem_pool100x3_covers(t) ? 1 : 0;
}

// ---- the ragged patch-grid view: whole images of different sizes, packed
IPSX_API int64_t ipsx_ragged_view_fill(ipsx_image_entry* table, int b, int c, int ph, int pw, int sh, int sw, const int32_t* h,
                                       const int32_t* w, const int64_t* elem_off) {
    if (!table || !h || !w || !elem_off || b <= 0 || c <= 0 || ph <= 0 || pw <= 0 || sh <= 0 || sw <= 0) {
        fail(IPSX_EINVAL, "ragged_view_fill: bad arguments");
        return -1;
    }
    int64_t first = 0;
    for (int k = 0; k < b; ++k) {
        if (h[k] <= 0 || w[k] <= 0 || ph > h[k] || pw > w[k]) {
            fail(IPSX_EINVAL, "ragged_view_fill: image %d is %dx%d, the patch %dx%d", k, h[k], w[k], ph, pw);
            return -1;
        }
        ipsx_image_entry& e = table[k];
        e.elem_off = elem_off[k]; e.first = first; e.h = h[k]; e.w = w[k];
        e.ny = (h[k] - ph) / sh + 1; e.nx = (w[k] - pw) / sw + 1;
        first += (int64_t)e.ny * e.nx;
        if (first > 0x7FFFFFFFll) {
            fail(IPSX_EINVAL, "ragged_view_fill: more than 2^31 - 1 patches");
            return -1;
        }
    }
    const ipsx_ragged_view rv{b, c, ph, pw, sh, sw, nullptr, table};
    return ragged_view_total(&rv, "ragged_view_fill");
}

IPSX_API int64_t ipsx_ragged_view_offset(const ipsx_image_entry* table, int b, const ipsx_ragged_view* geometry, int64_t p,
                                         int64_t* pitch, int64_t* chan_pitch) {
    if (!table || !geometry || b != geometry->b) return -1;
    const ipsx_ragged_view rv{b, geometry->c, geometry->ph, geometry->pw, geometry->sh, geometry->sw, nullptr, table};
    if (ragged_view_total(&rv, "ragged_view_offset") < 0) return -1;
    int w = 0, h = 0;
    const long long off = ragged_view_offset(table, b, rv.sh, rv.sw, p, &w, &h);
    if (off < 0) return -1;
    if (pitch) *pitch = w;
    if (chan_pitch) *chan_pitch = (int64_t)h * w;
    return off;
}

IPSX_API int ipsx_trunk_ragged_view_supported(const ipsx_trunk* t, const ipsx_ragged_view* view) {
    if (!t || !view || ragged_view_total(view, "trunk_ragged_view_supported") < 0) return 0;
    if (t->precision != 0 || t->patch_dtype != 0) return 0;
    if (view->c != t->c_in || view->ph != t->h || view->pw != t->w) return 0;
    return fused_trunk_supported(t) || fused_stem_pool50_covers(t) || fused_stem_pool100x3_covers(t) ? 1 : 0;
}

// One image: trunk AND logits of its patches as ONE persistent launch that feeds ipsx_scan_persistent patch by patch
// (fused_trunk_stream_kernel).  ctl: ipsx_trunk_stream_ctl_words(n) int32 words ZEROED by the caller before every call.
IPSX_API size_t ipsx_trunk_stream_ctl_words(int64_t n_patch) { return n_patch > 0 ? (size_t)ipsx::cdiv(n_patch, 2) + 3 : 0; }   // (+ the exit counter)

IPSX_API int ipsx_trunk_stream_supported(const ipsx_trunk* t, int d, int r) {
    return t && ipsx::fused_trunk_supported(t) && t->precision == 0 && t->patch_dtype == 0 && d == 128 && r >= 1 && r <= 32 ? 1 : 0;
}

IPSX_API int ipsx_trunk_stream(const ipsx_trunk* t, const float* patches, int64_t n_patch, float* emb, const float* pos,
                               const float* v_packed, int r, float* logits, int32_t* ctl, int32_t* ready, int workgroups,
                               int quad_pulls, void* stream) {
    IPSX_REQUIRE(t && patches && emb && v_packed && logits && ctl && ready && n_patch > 0, "trunk_stream: bad arguments");
    IPSX_REQUIRE(ipsx_trunk_stream_supported(t, 128, r), "trunk_stream: the fused fp32 1x32x32 trunk with 128 features and at most 32 logits per patch");
    return ipsx::fused_trunk_stream(t, patches, n_patch, emb, pos, v_packed, r, logits, ctl, ready, workgroups, quad_pulls,
                                    ipsx::as_stream(stream));
}

// 3.06: the stream reading patch index[j] of `patches` (src_patches of them) where it reads patch j.  The tiles read the
// index as it is: whoever composes it keeps it inside [0, src_patches) (ipsx_order_index clamps).
IPSX_API int ipsx_trunk_stream_indexed(const ipsx_trunk* t, const float* patches, const int32_t* index, int64_t src_patches,
                                       int64_t n_patch, float* emb, const float* pos, const float* v_packed, int r, float* logits,
                                       int32_t* ctl, int32_t* ready, int workgroups, int quad_pulls, void* stream) {
    IPSX_REQUIRE(t && patches && emb && v_packed && logits && ctl && ready && n_patch > 0, "trunk_stream_indexed: bad arguments");
    IPSX_REQUIRE(src_patches >= 1, "trunk_stream_indexed: a source of %lld patches", (long long)src_patches);
    IPSX_REQUIRE(!index || n_patch <= 0x7FFFFFF0ll, "trunk_stream_indexed: %lld patches through an int32 index", (long long)n_patch);
    IPSX_REQUIRE(ipsx_trunk_stream_supported(t, 128, r), "trunk_stream_indexed: the fused fp32 1x32x32 trunk with 128 features and at most 32 logits per patch");
    return ipsx::fused_trunk_stream(t, patches, n_patch, emb, pos, v_packed, r, logits, ctl, ready, workgroups, quad_pulls,
                                    ipsx::as_stream(stream), index);
}
