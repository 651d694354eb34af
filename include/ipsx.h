/*
 * ipsx.h - C ABI of libipsx.so: the MI355X (gfx950) implementation of the
 * Iterative-Patch-Selection no-grad hot path of benbergner/ips.
 *
 * Everything here is plain C: device pointers, sizes, an opaque stream handle
 * (a hipStream_t passed as void*; NULL = the null stream).  No torch types.  All
 * functions enqueue asynchronously on `stream`, never synchronise, never allocate
 * device memory (workspaces are caller-owned) and return 0 on success or a
 * negative IPSX_E* code; ipsx_last_error() gives the message for the calling
 * thread.  Buffers are contiguous fp32 (int64 for indices) unless stated.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the reference repo benbergner/ips).
 *
 * Arithmetic contract (restated on the CPU in oracle/ips_oracle.cpp):
 *   - every contraction (convolution taps x channels, Linear rows, q.k, attn.v)
 *     is ONE fp32 fused-multiply-add chain, which is what
 *     v_mfma_f32_32x32x2_f32 computes bit for bit;
 *   - convolution K index is tap-major: k = (ky*KW + kx)*C_in + c;
 *   - chains that run on the matrix cores (convolutions, projector Linear, K and V
 *     projections) visit every aligned group of 8 k in the order 0,4,1,5,2,6,3,7
 *     (the MFMA consumes k in (lane-half 0, lane-half 1) pairs and a lane half
 *     fetches 4 consecutive k with one 16-byte load); all others ascend;
 *   - eval BatchNorm is the affine y = fma(acc, alpha, shift) with
 *     alpha = gamma * (1/sqrt(var+eps)), shift = beta - mean*alpha;
 *   - exp() is ipsx's own fma polynomial (identical bits on host and device); softmax weights are
 *     e * (1 / den): ONE IEEE division per (head, token) row, a multiplication per candidate (round 5);
 *   - row sums (softmax denominators, the transformer's LayerNorm moments) are 64 strided
 *     partial sums combined by an xor butterfly (the wavefront reduction order);
 *   - the projector (ipsx_projector*) evaluates Linear(LayerNorm(x)) with the LayerNorm FOLDED
 *     into the epilogue: acc = the fma chain of the RAW row, t = fma(-mean, colsum[o], acc),
 *     u = t * rstd, y = relu(fma(u, alpha, shift')); the row's moments are eight chains - chain
 *     (h, j) over x[8g + 4h + j], g ascending: exactly what lane (row, half h) of the GEMM's
 *     operand stream holds - folded ((c0+c1)+(c2+c3)) per half, half 0 + half 1;
 *     mean = sum / F, var = fma(-mean, mean, sumsq / F) clamped at 0, rstd = 1 / sqrt(var + eps).
 *     Round 6: a row with var * 17 < sumsq / F (mean^2 / var > 16 - both forms above cancel there) is CENTRED, as
 *     nn.LayerNorm itself does: over d = x - mean the same eight chains sum d and d * d, mean' = mean + E[d],
 *     var = fma(-E[d], E[d], E[d^2]) clamped at 0; acc = the chain over (x - mean') * w, t = acc.  Its statistics read
 *     (mean', -rstd): the SIGN of rstd marks the row.  Well-conditioned rows never take this path (bits unchanged).
 */
#ifndef IPSX_H
#define IPSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version = 100 * major + minor.  The MAJOR number changes whenever the signature or meaning of an exported
 * function changes incompatibly or an export is removed (a caller built against another major must refuse to run:
 * `ipsx_version() / 100 != IPSX_VERSION / 100`); the minor number counts compatible additions.
 *   1.xx  rounds 1-2
 *   2.00  round 3: ipsx_scan / ipsx_scan_range / ipsx_topm take (workspace, workspace_bytes) in front of `stream`,
 *         ipsx_scan_persistent takes ready_per_image, ipsx_projector_stats_publish removed
 *   2.01  round 4 (additions only): ipsx_aggregate_packed, ipsx_set_persistent_wait_ms, ipsx_conv2d_wgrad_nhwc*,
 *         ipsx_pack_conv_weight_strided, ipsx_conv2d_affine_to_nhwc, ipsx_conv2d_lds_nhwc*;
 *         ipsx_projector_stream accepts
 *         short_first <= -3 (guided tile sizes)
 *   2.02  round 4: ipsx_scan_persistent_on, ipsx_scan_persistent_groupable
 *   2.03  round 4: ipsx_scan_persistent_ws, ipsx_scan_range_if_ws (persistent loops for candidate sets beyond the LDS)
 *   3.00  round 5: struct ipsx_conv grew by `colsum` (every struct that embeds it moved) and the projector's arithmetic
 *         contract changed (LayerNorm folded into the epilogue: ipsx_projector* need lin->colsum, ipsx_projector_stats
 *         returns the moments in the operand-stream order); ipsx_weight_colsum added; the two stream kernels publish their
 *         last rows themselves (one more control word each: ipsx_*_stream_ctl_words), ipsx_ips_finish, ipsx_ips_call_run /
 *         ipsx_ips_call_elapsed added
 *   3.01  round 5 (additions only): ipsx_pack_conv_weights_batch, ipsx_conv2d_lds_nhwc_stats (+ _slabs),
 *         ipsx_bn_train_forward_partials, ipsx_stem7x7s2_nhwc (+ _supported), ipsx_conv2d_dgrad_s2_lds_nhwc (+ _supported),
 *         ipsx_maxpool_3x3s2_bwd_nhwc (+ _supported)
 *   3.02  round 6 (additions): ipsx_projector_stream_ctl_zero_words (the stream's control words were re-ordered: what must be
 *         zero comes first); ipsx_scan_workgroups_per_image - candidate sets beyond the LDS with 8 heads and one token run
 *         as a team of workgroups per image; ipsx_scan_workspace_bytes grew for those shapes
 *   3.03  (additions only): ipsx_projector_stats_typed, ipsx_projector_apply_bf16, ipsx_projector_bf16_supported - the
 *         feature projector on the bf16 matrix pipe, rows stored as float32 / bfloat16 / float16;
 *         ipsx_conv2d_affine_nhwc_bf16 (+ _supported), ipsx_avgpool_nhwc_bf16 - the layer-by-layer trunk at precision 1:
 *         ipsx_trunk_encode no longer refuses precision 1 on a trunk the fused kernel does not take
 *   3.04  (additions only): ipsx_projector_train_forward (+ _supported, _slabs), ipsx_projector_wgrad (+ _chunk_rows,
 *         _max_rows, _workspace_bytes) - the feature projector of the training step, forward and weight gradient
 *   3.05  (additions only): ipsx_attn_pool_forward, ipsx_attn_pool_backward (+ _supported, _workspace_bytes) - the
 *         cross-attention aggregator of the training step on folded queries
 *   3.06  (additions only): ipsx_projector_stats_indexed, ipsx_projector_apply_indexed, ipsx_projector_apply_bf16_indexed,
 *         ipsx_projector_stream_indexed, ipsx_ips_finish_indexed - the feature projector reading its rows through an index
 *         (a shuffle applied as addressing, not as a copy of the patch tensor) and the end of such a call;
 *         ipsx_trunk_encode_u8, ipsx_trunk_encode_indexed_u8, ipsx_dequant_patches - uint8 patch storage: the stems of the
 *         exact fp32 trunks read bytes and look their float32 values up in a per-channel table;
 *         ipsx_trunk_encode_parts, ipsx_part_wait, ipsx_logits_if - every part of a call through the fused fp32 trunk as
 *         ONE launch that counts each part's finished patches, the one-wave kernel that holds another stream until a part
 *         is complete, and the conditional logits of its recovery;
 *         ipsx_patch_view (struct), ipsx_patch_view_offset, ipsx_trunk_view_supported, ipsx_trunk_encode_view,
 *         ipsx_trunk_encode_parts_view, ipsx_gather_patches_view - the patch-grid view: the LDS-staging stems of the exact
 *         fp32 trunks read their patches straight from the (b, c, h, w) images, no (b, n, c, ph, pw) tensor exists;
 *         ipsx_trunk_encode_view_u8, ipsx_gather_patches_view_u8 - the view over whole uint8 images: the same stems stage
 *         table[c][byte] off the image grid, neither float32 images nor a patch tensor exist;
 *         ipsx_scan_range_strided, ipsx_stream_commit (+ struct ipsx_stream_table) - IPS over patches fed in pieces: the
 *         loop on logits that sit in a candidate table of fixed capacity, and the launch that carries a stream's state
 *         (the m winners in rank order, then the not yet scored tail) forward without joining or copying the piece;
 *         ipsx_stream_commit_view - that launch for a stream fed pixel-row bands of whole images: the piece of the patch
 *         table is read out of the images through an ipsx_patch_view, no patch tensor exists;
 *         ipsx_order_index, ipsx_trunk_stream_indexed, ipsx_ips_call_run_ordered (+ struct ipsx_call_order) - a shuffle
 *         index on the one-call route: the launch that composes a permutation into flat int32 row numbers, the one-image
 *         trunk stream reading its patches through such an index, and ipsx_ips_call_run with both inside it;
 *         ipsx_trunk_encode_parts_u8, ipsx_trunk_encode_parts_view_u8 - the counted one-launch route on uint8 patches and on
 *         whole uint8 images: ipsx_trunk_encode_parts / _parts_view with the bytes' staging (the minor number stays: it and
 *         this block are pinned by the tests of the earlier 3.06 additions);
 *         ipsx_pack_conv_weight_tile16 (+ ipsx_packed_conv_weight_tile16_elems) - the fused 1x32x32 trunk at precision 0 runs
 *         its three 128 -> 128 convolutions on 16-row tiles and reads their weights in this packing from
 *         ipsx_conv.w_packed_bf16, which precision 0 did not read before: a caller that left it NULL there is refused;
 *         ipsx_trunk_encode_parts_dedup (+ ipsx_trunk_parts_dedup_workspace_bytes) - ipsx_trunk_encode_parts with exact
 *         blank-patch dedup inside the counted launch (the minor number stays, as above: the tests of the earlier 3.06
 *         additions pin it);
 *         ipsx_trunk_encode_parts_dedup_u8, ipsx_trunk_encode_parts_dedup_view, ipsx_trunk_encode_parts_dedup_view_u8 - that
 *         dedup on the other three sources of the counted launch: uint8 patches, float32 images and uint8 images through a
 *         patch view (additions only, the minor number stays for the same reason);
 *         ipsx_scan_ragged - the selection loop over slides of different lengths packed into one logits table, one launch
 *         (an addition, the minor number stays for the same reason);
 *         ipsx_ragged_finish - the end of a padded ragged call in one launch: selected rows of long slides, the rows of
 *         short slides in the order given, zero padding, indices and global rows (an addition, the minor number stays);
 *         ipsx_scan_ragged_spans, ipsx_stream_commit_ragged - slides of different lengths fed in pieces
 *         (IPSNet.ips_ragged_stream): ipsx_scan_ragged on slides that lie anywhere in one logits table, and ipsx_stream_commit
 *         with per-slide numbers read from a device table (additions, the minor number stays);
 *         ipsx_image_entry, ipsx_ragged_view (structs), ipsx_ragged_view_fill, ipsx_ragged_view_offset,
 *         ipsx_trunk_ragged_view_supported, ipsx_trunk_encode_ragged_view, ipsx_ragged_finish_view - whole images of
 *         different sizes in one call (IPSNet.ips_image_ragged): the patch-grid view with where a patch lies and its
 *         pitches read per patch from a table, and the end of such a call in one launch (additions, the minor number stays);
 *         ipsx_ragged_view_blank_flags, ipsx_trunk_encode_ragged_view_dedup (+ ipsx_trunk_ragged_view_dedup_workspace_bytes) -
 *         exact blank-patch dedup on the ragged view: ipsx_trunk_encode_ragged_view encoding every non-blank entry and one
 *         blank one (additions, the minor number stays);
 *         ipsx_trunk_encode_ragged_view_u8, ipsx_ragged_finish_view_u8, ipsx_ragged_view_blank_flags_u8,
 *         ipsx_trunk_encode_ragged_view_dedup_u8 - the ragged view over whole uint8 images with their table: the four ragged
 *         entries with the bytes' staging of ipsx_trunk_encode_view_u8 (additions, the minor number stays);
 *         ipsx_stream_commit_ragged_view - row bands of whole images of different sizes (IPSNet.ips_ragged_stream with a
 *         patch size): ipsx_stream_commit_ragged whose patch table reads its piece out of the packed pixel windows of a feed
 *         through an ipsx_ragged_view, no patch tensor exists (an addition, the minor number stays);
 *         ipsx_scan_range_logits, ipsx_scan_logits_check (+ struct ipsx_logits_part) - a range of the selection loop whose
 *         launch computes its own logits in a prologue (8 heads x 4 tokens, m = i = 64), and the conditional redo of a counted
 *         call inside its last part's launch (additions, the minor number stays);
 *         ipsx_scan_range_logits_gate - ipsx_scan_range_logits handed over on the device between two streams: a word per
 *         image published at a launch's end and waited for behind the next launch's prologue, the result in a buffer of its
 *         own (an addition, the minor number stays);
 *         ipsx_aggregate_counted, ipsx_attn_pool_forward_counted, ipsx_attn_pool_backward_counted - the masked aggregator:
 *         image b of a zero-padded batch (IPSNet.ips_ragged(pad=True)) attends to its first count[b] slots only, in the
 *         eval aggregation and in the training step's attention pool (additions, the minor number stays);
 *         ipsx_projector_train_forward_indexed, ipsx_projector_wgrad_indexed - the masked encoder pass: the training step's
 *         projector reads the filled rows of a zero-padded batch where they lie, through a row index, every intermediate
 *         packed (additions, the minor number stays) */
#define IPSX_VERSION 306

#define IPSX_OK            0
#define IPSX_EINVAL       -1      /* bad argument / unsupported shape */
#define IPSX_EHIP         -2      /* HIP runtime error (launch failed ...) */
#define IPSX_EWORKSPACE   -3      /* workspace too small */

int ipsx_version(void);
const char* ipsx_last_error(void);
/* number of GPUs visible, and whether device `dev` is a gfx950 part (1/0) */
int ipsx_device_count(void);
int ipsx_device_is_gfx950(int dev);

/* ------------------------------------------------------------------ encoder
 * Replaces IPSNet.encoder as built by get_conv_patch_enc
 * (architecture/ips_net.py:17-52; called at :209, :227, :273).            */

/* elements of the packed form of an OIHW weight (C_out padded to 32, K to 8) */
size_t ipsx_packed_conv_weight_elems(int c_out, int c_in, int kh, int kw);

/* OIHW fp32 -> MFMA B-operand stream [C_out/32][K/8][64 lanes][4], tap-major K;
 * element j of lane l holds k = 8*group + 4*(l>>5) + j, output channel 32*tile + (l&31) */
int ipsx_pack_conv_weight(const float* w_oihw, int c_out, int c_in, int kh, int kw,
                          float* packed, void* stream);
/* The same from a strided view: element (n, c, ky, kx) of the convolution's weight is w[base + n*s_out + c*s_in + ky*s_ky +
 * kx*s_kx] (element strides, any sign) - a channels-last tensor as it lies, or, with base at the last tap, negated tap
 * strides and swapped channel strides, the weights rotated by 180 degrees and transposed that make ipsx_conv2d_affine_nhwc
 * on dy the data gradient of the convolution. */
int ipsx_pack_conv_weight_strided(const float* w, int64_t base, int c_out, int c_in, int kh, int kw, int64_t s_out,
                                  int64_t s_in, int64_t s_ky, int64_t s_kx, float* packed, void* stream);
/* Up to 32 of those as ONE launch (the training step re-packs every convolution's weights, in forward and in data-gradient
 * form, after each optimizer step: training/iterative.py:155-163).  Same bits as the single calls. */
typedef struct ipsx_pack_job {
    const float* w; int64_t base; int c_out, c_in, kh, kw; int64_t s_out, s_in, s_ky, s_kx; float* packed;
} ipsx_pack_job;
int ipsx_pack_conv_weights_batch(const ipsx_pack_job* jobs, int n_jobs, void* stream);

/* bf16 variant for the reduced-precision trunk: [C_out/32][K/16][64 lanes][8 bf16], round to nearest even */
size_t ipsx_packed_conv_weight_bf16_bytes(int c_out, int c_in, int kh, int kw);
int ipsx_pack_conv_weight_bf16(const float* w_oihw, int c_out, int c_in, int kh, int kw,
                               void* packed, void* stream);

/* fp32 B-operand stream of the fused 1x32x32 trunk's 16-row tiles (v_mfma_f32_16x16x4_f32), for its three 3x3 convolutions
 * 128 -> 128 at precision 0: [C_out/32][K/16][2][64 lanes][4], tap-major K; component j of lane l holds output channel
 * 32*tile + 16*half + (l&15) and, of the block's 16 k, the one at position 4*(l>>4) + j of the order
 * 0 2 8 10 | 4 6 12 14 | 1 3 9 11 | 5 7 13 15.  C_out % 32 == 0 and C_in % 16 == 0 (elems: 0 otherwise).  Goes into
 * ipsx_conv.w_packed_bf16 beside the ipsx_pack_conv_weight stream in w_packed, which every other kernel keeps reading. */
size_t ipsx_packed_conv_weight_tile16_elems(int c_out, int c_in, int kh, int kw);
int ipsx_pack_conv_weight_tile16(const float* w_oihw, int c_out, int c_in, int kh, int kw,
                                 float* packed, void* stream);

/* eval-mode BatchNorm (nn.BatchNorm2d/1d with running stats) -> per-channel affine.
 * lin_bias (or NULL): bias of a Linear feeding the BatchNorm, folded in as
 * shift = fma(lin_bias, alpha, shift)                                        */
int ipsx_bn_affine(const float* gamma, const float* beta, const float* mean,
                   const float* var, const float* lin_bias, float eps, int c,
                   float* alpha, float* shift, void* stream);

/* split variant for precision 2 ("fp32x3"): every weight as three bf16 terms hi + mid + lo (exact),
 * [C_out/32][K/16][plane][64 lanes][8 bf16]; three times the bf16 stream                            */
size_t ipsx_packed_conv_weight_x3_bytes(int c_out, int c_in, int kh, int kw);
int ipsx_pack_conv_weight_x3(const float* w_oihw, int c_out, int c_in, int kh, int kw,
                             void* packed, void* stream);

/* stem of the split trunks (precision 1: planes = 1, precision 2: planes = 3): the (c_out, 1, 7, 7) weights as the
 * B-operand stream of a contraction whose K is laid out as k = 8 ky + kx (zero weights for ky = 7 and kx = 7),
 * [C_out/32][4][plane][64 lanes][8 bf16]; goes into the stem's ipsx_conv.w_packed_bf16                       */
size_t ipsx_packed_stem_weight_split_bytes(int c_out, int planes);
int ipsx_pack_stem_weight_split(const float* w_oihw, int c_out, int planes, void* packed, void* stream);

typedef struct ipsx_conv {
    int c_in, c_out, kh, kw, stride, pad;
    const float* w_packed;        /* ipsx_pack_conv_weight output            */
    const float* alpha;           /* c_out, BatchNorm scale (or NULL = 1)    */
    const float* shift;           /* c_out, BatchNorm shift / bias (or NULL) */
    const void* w_packed_bf16;    /* bf16 operand stream for ipsx_trunk.precision: ipsx_pack_conv_weight_bf16
                                     (precision 1) or ipsx_pack_conv_weight_x3 (precision 2); NULL = fp32 only.
                                     At precision 0, on a 3x3 convolution 128 -> 128 of stride 1:
                                     ipsx_pack_conv_weight_tile16 (float32), read by the fused 1x32x32 trunk */
    const float* colsum;          /* c_out, sum over c_in of the weights (ipsx_weight_colsum): the projector's Linear
                                     only (ipsx_projector*: the folded LayerNorm's mean term); NULL elsewhere      */
} ipsx_conv;

/* one residual block: BasicBlock (n_conv = 2) or Bottleneck (n_conv = 3)     */
typedef struct ipsx_block {
    int n_conv;
    ipsx_conv conv[3];
    int has_down;                 /* 1x1 strided projection on the shortcut  */
    ipsx_conv down;
} ipsx_block;

/* the nn.Sequential of ips_net.py:35-50: stem conv 7x7/2 + BN + ReLU,
 * max-pool 3x3/2, residual blocks, global average pool                      */
typedef struct ipsx_trunk {
    int c_in, h, w;               /* patch shape (C, h, w)                    */
    ipsx_conv stem;
    int n_block;
    const ipsx_block* blocks;     /* HOST array of n_block descriptors        */
    int precision;                /* 0 = fp32 (exact, default); 1 = bf16 operands / fp32 accumulate in the
                                     residual stages; 2 = "fp32x3": every fp32 operand split exactly into three
                                     bf16 terms, the six significant products on the bf16 matrix pipe, fp32
                                     accumulate - fp32-grade accuracy, not bit-identical to precision 0.
                                     1 and 2 need w_packed_bf16.  2: fused 1x32x32 trunk only.  1 on any other
                                     trunk: stem + max-pool in fp32, the pooled map rounded once to bf16, every
                                     convolution behind it ipsx_conv2d_affine_nhwc_bf16 on bf16 activations   */
    int patch_dtype;              /* storage type of the `patches` argument of the encode calls: 0 = float32
                                     (default), 1 = bfloat16, 2 = float16 (BASELINE configs[4]: half-precision patch
                                     storage; fused 1x32x32 trunk at precision 1 or 2 only - the exact path and
                                     the stems of the layer-by-layer trunks read float32)                   */
} ipsx_trunk;

/* y = act(affine(conv(x)) [+ residual]); x (n,c_in,h,w), y (n,c_out,ho,wo) NCHW */
int ipsx_conv2d_affine(const ipsx_conv* cv, const float* x, const float* residual,
                       float* y, int64_t n, int h, int w, int relu, void* stream);
/* x NCHW as above, residual / y channels-last (n,ho,wo,c_out): the stems (1 or 3 input channels) in front of the
 * channels-last layers */
int ipsx_conv2d_affine_to_nhwc(const ipsx_conv* cv, const float* x, const float* residual,
                               float* y, int64_t n, int h, int w, int relu, void* stream);
/* the same on channels-last activations: x (n,h,w,c_in), residual / y (n,ho,wo,c_out); C_in % 32 == 0.
 * This is the fast layer-by-layer path (16-byte operand loads); a Linear over rows is h = w = 1.
 * Alignment: x, residual, y and w_packed at 16-byte addresses (no scalar route; not tested here - the caller's duty). */
int ipsx_conv2d_affine_nhwc(const ipsx_conv* cv, const float* x, const float* residual,
                            float* y, int64_t n, int h, int w, int relu, void* stream);
/* The same on the bf16 matrix pipe (3.03; the layer-by-layer trunk at precision 1): x, residual and y are bfloat16,
 * channels-last, at 16-byte addresses; B operand cv->w_packed_bf16 (ipsx_pack_conv_weight_bf16), fp32 accumulation in one
 * fixed k order per output, then in fp32 fma(acc, alpha, shift) [+ residual widened exactly] [ReLU] and ONE rounding to
 * bfloat16 (nearest even).  Any kernel size, stride and padding; C_in % 16 == 0, C_out % 8 == 0 (_supported). */
int ipsx_conv2d_affine_nhwc_bf16_supported(const ipsx_conv* cv);
int ipsx_conv2d_affine_nhwc_bf16(const ipsx_conv* cv, const void* x, const void* residual, void* y, int64_t n, int h,
                                 int w, int relu, void* stream);
/* The fused trunk's stages as stand-alone plain convolutions of channels-last maps (training step: forward and data
 * gradient on the maps of 32-px patches, each layer's input read once and LDS-resident for all taps): 64 -> 64 3x3 on 8x8,
 * 128 -> 128 3x3 on 4x4, 64 -> 128 3x3 / 2 and 1x1 / 2 from 8x8 (ipsx_conv2d_lds_nhwc_supported).  cv: kernel, stride, pad and
 * w_packed (ipsx_pack_conv_weight[_strided]); alpha / shift are ignored. */
int ipsx_conv2d_lds_nhwc_supported(int c_in, int c_out, int k, int stride, int pad, int h, int w);
int ipsx_conv2d_lds_nhwc(const ipsx_conv* cv, const float* x, float* y, int64_t n, int h, int w, void* stream);
/* The same with the BatchNorm BATCH STATISTICS of the output taken off the accumulators (training step: conv -> bn of a
 * torchvision BasicBlock, architecture/ips_net.py:273 under net.train()): partial[slab][0 | 1][C_out] = sum (y - shift[c]),
 * sum (y - shift[c])^2 over the slab's output rows, slab = 4 patches, ipsx_conv2d_lds_nhwc_stats_slabs(n) of them; shift: a
 * per-channel constant near the mean (the BatchNorm's running mean; NULL = 0).  ipsx_bn_train_forward_partials combines them
 * (fp64, slab order: deterministic) and applies the BatchNorm - the reduction pass over y is gone.  partial NULL: plain. */
/* The 1 -> 64 channel 7x7 / 2 stem on 32 x 32 patches as a stand-alone layer, channels-last output (n, 16, 16, 64): the
 * training step's first convolution (ips_net.py:29-31 under net.train()) on the matrix cores - the fused trunk's stem
 * without its BatchNorm / ReLU / max-pool epilogue; same bits as ipsx_conv2d_affine_to_nhwc without affine. */
int ipsx_stem7x7s2_nhwc_supported(int c_in, int c_out, int kh, int kw, int stride, int pad, int h, int w);
int ipsx_stem7x7s2_nhwc(const ipsx_conv* conv, const float* x, float* y, int64_t n, const float* shift, float* partial,
                        void* stream);          /* shift / partial: as ipsx_conv2d_lds_nhwc_stats (slabs of 4 patches); NULL: none */
/* The data gradient of the 32-px trunk's strided convolution (64 -> 128 channels, 3x3 / 2, 8x8 -> 4x4 maps; the arguments of
 * _supported describe that FORWARD convolution): dy (n, 4, 4, 128) -> dx (n, 8, 8, 64), channels-last, taken by parity class
 * of the input pixel - nine taps instead of the thirty-six of a stride-1 convolution over dy spread on a zero map.
 * w_packed_dgrad: ipsx_pack_conv_weight_strided of the weights rotated by 180 degrees and transposed (128 -> 64, 3x3).
 * Alignment: w_packed_dgrad, dy and dx at 16-byte addresses (float4 loads and stores, no scalar route). */
int ipsx_conv2d_dgrad_s2_lds_nhwc_supported(int c_in, int c_out, int k, int stride, int pad, int h, int w);
int ipsx_conv2d_dgrad_s2_lds_nhwc(const float* w_packed_dgrad, int k, const float* dy, float* dx, int64_t n, void* stream);
                                  /* k = 3 (pad 1), or k = 1: the 1x1 / 2 projection beside it (pad 0; three of four input pixels
                                   * receive zeros) */
int64_t ipsx_conv2d_lds_nhwc_stats_slabs(int64_t n);
int ipsx_conv2d_lds_nhwc_stats(const ipsx_conv* conv, const float* x, float* y, int64_t n, int h, int w, const float* shift,
                               float* partial, void* stream);
/* Weight gradient of that convolution for the training step (reference: loss.backward() of training/iterative.py:157-163
 * through the BasicBlocks of architecture/ips_net.py:264-283):
 *   dw[co][ky][kx][ci] = sum over (img, oy, ox) of dy[img,oy,ox,co] * x[img, stride*oy + ky - pad, stride*ox + kx - pad, ci]
 * x (n,h,w,c_in) and dy (n,ho,wo,c_out) channels-last, dw in the memory order of a channels-last weight tensor
 * ((c_out, c_in, kh, kw) with strides (kh*kw*c_in, 1, kw*c_in, c_in)).  fp32 MFMA, reduction over the pixels split across
 * workgroups and added in a fixed order (deterministic).  c_out a multiple of 64, c_in a multiple of 64 or 1 (the 7x7 stem)
 * (ipsx_conv2d_wgrad_nhwc_supported).
 * The data gradient is ipsx_conv2d_affine_nhwc itself: on dy with the weights rotated by 180 degrees and transposed. */
int ipsx_conv2d_wgrad_nhwc_supported(int c_in, int c_out, int kh, int kw, int stride, int pad);
size_t ipsx_conv2d_wgrad_nhwc_workspace_bytes(int64_t n, int c_in, int c_out, int kh, int kw);
int ipsx_conv2d_wgrad_nhwc(const float* x, const float* dy, int64_t n, int h, int w, int c_in, int c_out, int kh, int kw,
                           int stride, int pad, float* dw, void* workspace, size_t workspace_bytes, void* stream);
/* (x and y at 16-byte addresses, c % 4 == 0: float4 along the channels, no scalar route; the same holds for x, dy and dx of
 * the backward pass below) */
int ipsx_maxpool_3x3s2_nhwc(const float* x, float* y, int64_t n, int c, int h, int w, void* stream);
/* Its backward pass for the training step (16 x 16 maps, C % 32 == 0): dx (n, 16, 16, C) from x and dy (n, 8, 8, C), the
 * gradient of a window to its first maximum in row-major order - ATen's max_pool2d_with_indices_backward bit for bit, without
 * an index tensor. */
int ipsx_maxpool_3x3s2_bwd_nhwc_supported(int c, int h, int w);
int ipsx_maxpool_3x3s2_bwd_nhwc(const float* x, const float* dy, float* dx, int64_t n, int c, int h, int w, void* stream);
/* (n,hw,c) -> (n,c) */
int ipsx_avgpool_nhwc(const float* x, float* y, int64_t n, int c, int hw, void* stream);
/* the same over a bfloat16 map: fp32 sum in the same order, same division, float32 out (3.03) */
int ipsx_avgpool_nhwc_bf16(const void* x, float* y, int64_t n, int c, int hw, void* stream);
/* nn.MaxPool2d(3, 2, 1) */
int ipsx_maxpool_3x3s2(const float* x, float* y, int64_t n, int c, int h, int w, void* stream);
/* nn.AdaptiveAvgPool2d(1): (n,c,hw) -> (n,c) */
int ipsx_avgpool(const float* x, float* y, int64_t n, int c, int hw, void* stream);

size_t ipsx_trunk_workspace_bytes(const ipsx_trunk* t, int64_t n_patch);
/* name of the kernel family ipsx_trunk_encode will use for this trunk (static string) */
const char* ipsx_trunk_kernel(const ipsx_trunk* t);
/* patches (n_patch, c_in, h, w) -> emb (n_patch, D); picks the fused LDS-resident
 * kernel when the trunk matches it, the layer-by-layer kernels otherwise       */
int ipsx_trunk_encode(const ipsx_trunk* t, const float* patches, int64_t n_patch,
                      float* emb, void* workspace, size_t workspace_bytes, void* stream);

/* Encode the patches patches[index[0..n_index)] (int32 indices, device) -> emb (n_index, D): lets a caller
 * encode a strided subset (e.g. columns lo..hi of a (B, N, ...) tensor) without copying it.  Fused trunk only. */
int ipsx_trunk_encode_indexed(const ipsx_trunk* t, const float* patches, const int32_t* index,
                              int64_t n_index, float* emb, void* stream);

/* 3.06: uint8 patch storage.  `patches` holds the pixels as bytes, `table` (c_in x 256 floats, device) the float32 value of
 * every byte per channel - e.g. byte / 255, or (byte / 255 - mean[c]) / std[c], filled by the host with the very tensor ops
 * the dataset would have run.  The stem looks each pixel up while it stages the patch (the zero padding stays 0.0f) and
 * everything behind that load is the float32 code: emb is bit for bit ipsx_trunk_encode of the expanded tensor
 * x[p][c][..] = table[c][patches[p][c][..]].  The exact path only (precision 0, patch_dtype 0; anything else: IPSX_EINVAL);
 * ipsx_trunk_kernel and ipsx_trunk_workspace_bytes serve both.  Addresses: table 16-byte aligned; patches 16-byte aligned
 * for the fused 1x32x32 and the 3x100x100 stem, 4-byte aligned for the 1x50x50 stem, any for other shapes.
 * ipsx_dequant_patches: q (n_patch, c, hw) bytes -> out (n_patch, c, hw) floats, out = table[c][q] - for the M patches a
 * selection keeps. */
int ipsx_trunk_encode_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, int64_t n_patch,
                         float* emb, void* workspace, size_t workspace_bytes, void* stream);
int ipsx_trunk_encode_indexed_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, const int32_t* index,
                                 int64_t n_index, float* emb, void* stream);
int ipsx_dequant_patches(const uint8_t* q, const float* table, float* out, int64_t n_patch, int c, int hw, void* stream);

/* 3.06: the parts of a call in ONE launch.  index (n_index int32, device): the parts' index lists one after the other; emb row
 * j belongs to list entry j, so a part's embeddings are one contiguous block, bit for bit ipsx_trunk_encode_indexed of its
 * list.  part_end (n_parts values on the HOST): the exclusive prefix ends of the parts in list entries, increasing, the last
 * one n_index.  done (n_parts int32, device, ZEROED by the caller on the same stream in front of the call): done[k] counts
 * the patches of part k whose embeddings are written and visible device-wide; it ends on the part's size.  The exact fp32
 * fused 1x32x32 trunk on float32 patches only (precision 0, patch_dtype 0) and n_parts <= 16; anything else: IPSX_EINVAL,
 * nothing launched.
 * ipsx_part_wait: a one-wavefront kernel that holds `stream` until *done >= want, so that kernels behind it in that stream
 * may read the part's embeddings while the trunk launch is still running on another stream.  It gives up after
 * ipsx_set_persistent_wait_ms WITHOUT PROGRESS of the counter (never unbounded) and then ORs `bit` into *status (device
 * int32, zeroed by the caller): what followed it has to be redone (ipsx_logits_if, ipsx_scan_range_if on that word).
 * Enqueue the trunk launch BEFORE the waits. */
int ipsx_trunk_encode_parts(const ipsx_trunk* t, const float* patches, const int32_t* index, int64_t n_index,
                            float* emb, const int64_t* part_end, int n_parts, int32_t* done, void* stream);
int ipsx_part_wait(const int32_t* done, int32_t want, int32_t* status, int32_t bit, void* stream);

/* 3.06: the patch-grid view.  The patches of a batch of whole images, addressed where they lie: no patch tensor.
 * images: float32 (b, c, h, w), contiguous; patch p = (bi * ny + py) * nx + px, ny = (h - ph) / sh + 1, nx = (w - pw) / sw + 1
 * (the order of the reference's unfold, data/megapixel_mnist/mnist_dataset.py:44-51, image-major: the numbering of
 * ipsx_patchify's output), starts at element ((bi * c) * h + py * sh) * w + px * sw; its row pitch is w, its channel pitch
 * h * w.  A geometry is valid when every field is positive, ph <= h, pw <= w and b * ny * nx < 2^31. */
typedef struct ipsx_patch_view {   /* images (b, c, h, w), contiguous;         patches numbered (bi*ny + py)*nx + px, */
    int b, c, h, w;                /* ny = (h-ph)/sh + 1, nx = (w-pw)/sw + 1: the order of the reference's unfold       */
    int ph, pw, sh, sw;
} ipsx_patch_view;

/* host: element offset of patch p's (0,0,0) inside the images; -1 for an invalid geometry or a p outside the grid */
int64_t ipsx_patch_view_offset(const ipsx_patch_view* v, int64_t p);
/* 1 when ipsx_trunk_encode_view takes this trunk and view: the exact path (precision 0, patch_dtype 0), a valid geometry
 * whose (c, ph, pw) is the trunk's patch shape, and a stem that stages its patch into LDS - the fused 1x32x32 trunk,
 * stem_pool50_kernel (1x50x50) or stem_pool100x3_kernel (3x100x100).  0 otherwise (the generic stem, bf16 / fp32x3). */
int ipsx_trunk_view_supported(const ipsx_trunk* t, const ipsx_patch_view* v);
/* emb row j (j < n) = the embedding of grid patch index[j] (device int32), or of patch first + j when index is NULL: bit for
 * bit ipsx_trunk_encode of those patches copied out of the images (ipsx_patchify) - only the stem's input load differs.  A
 * list entry outside the grid reads patch 0.  The load width is picked per launch: 16-byte loads (8-byte for the 50-px
 * stem) when `images` lies at a multiple of the width and w and sw are multiples of 4 (2) floats, dword loads otherwise.
 * workspace: as ipsx_trunk_encode (ipsx_trunk_workspace_bytes; none for the fused trunk). */
int ipsx_trunk_encode_view(const ipsx_trunk* t, const float* images, const ipsx_patch_view* v,
                           const int32_t* index /* NULL: patches first .. first+n-1 */, int64_t first, int64_t n,
                           float* emb, void* workspace, size_t workspace_bytes, void* stream);
/* ipsx_trunk_encode_parts (below) with (images, view) in place of patches: index holds grid patch numbers */
int ipsx_trunk_encode_parts_view(const ipsx_trunk* t, const float* images, const ipsx_patch_view* v, const int32_t* index,
                                 int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                 void* stream);
/* out[bi][j] = patch idx[bi][j] of image bi (idx: (b, m) int64 on the device, patch numbers INSIDE an image, py * nx + px;
 * a number outside [0, ny * nx) reads patch 0), out (b, m, c, ph, pw): the M patches a selection keeps, copied out of the
 * images (ips_net.py:245-247 on a tensor that does not exist).  One thread per output float, or per 16 bytes when the
 * addresses allow. */
int ipsx_gather_patches_view(const float* images, const ipsx_patch_view* v, const int64_t* idx /* (b, m), per image */,
                             int m, float* out /* (b, m, c, ph, pw) */, void* stream);

/* 3.06: the patch-grid view over uint8 images.  `images` holds the pixels of the (b, c, h, w) images as bytes, `table` (c x 256
 * floats, device, 16-byte aligned) their float32 values per channel as for ipsx_trunk_encode_u8; ipsx_patch_view keeps its
 * layout and its offsets are the same in bytes, an element being one byte.  emb is bit for bit ipsx_trunk_encode_view of the
 * expanded images x[b][c][y][x] = table[c][images[b][c][y][x]]: a stem stages table[c][byte] where its float32 twin stages the
 * float it loaded, and the padding stays 0.0f.  The same trunks as ipsx_trunk_view_supported.  `images` may lie at ANY
 * address: the load width is picked per launch as the widest of the kernel's list at which images, w and sw are all multiples
 * of it - fused 1x32x32 trunk 16 / 4 / 1 bytes (its pair kernel 8 / 4 / 1), 1x50x50 stem 2 / 1, 3x100x100 stem 4 / 1.
 * ipsx_gather_patches_view_u8: ipsx_gather_patches_view out of such images, out (float32) = table[c][byte]. */
int ipsx_trunk_encode_view_u8(const ipsx_trunk* t, const uint8_t* images, const float* table, const ipsx_patch_view* v,
                              const int32_t* index /* NULL: patches first .. first+n-1 */, int64_t first, int64_t n,
                              float* emb, void* workspace, size_t workspace_bytes, void* stream);
int ipsx_gather_patches_view_u8(const uint8_t* images, const float* table, const ipsx_patch_view* v,
                                const int64_t* idx /* (b, m), per image */, int m, float* out /* (b, m, c, ph, pw) */,
                                void* stream);

/* 3.06: the parts of a call in ONE launch (ipsx_trunk_encode_parts, ipsx_trunk_encode_parts_view) on uint8 patches and on whole
 * uint8 images: index, emb, part_end, n_parts and done mean what they mean there, patches / images / table / view what they mean
 * for ipsx_trunk_encode_indexed_u8 and ipsx_trunk_encode_view_u8, and emb is bit for bit theirs on every part's list.  The exact
 * fp32 fused 1x32x32 trunk only (precision 0, patch_dtype 0), n_parts <= 16, table and - for patches - `patches` 16-byte
 * aligned (images: any address, the load width 16 / 4 / 1 bytes is picked per launch); anything else: IPSX_EINVAL, nothing
 * launched. */
int ipsx_trunk_encode_parts_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, const int32_t* index,
                               int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done, void* stream);
int ipsx_trunk_encode_parts_view_u8(const ipsx_trunk* t, const uint8_t* images, const float* table, const ipsx_patch_view* v,
                                    const int32_t* index, int64_t n_index, float* emb, const int64_t* part_end, int n_parts,
                                    int32_t* done, void* stream);

/* Same result as ipsx_trunk_encode, with exact blank-patch deduplication (all-zero patches share one
 * embedding in eval mode; ~93 % of Megapixel-MNIST patches): only the non-blank patches and one blank
 * are encoded, everything on the device.  Fused 1x32x32 trunk only.  n_encoded (device int32, or NULL)
 * receives the number of patches actually encoded.                                              */
size_t ipsx_trunk_dedup_workspace_bytes(const ipsx_trunk* t, int64_t n_patch);
int ipsx_trunk_encode_dedup(const ipsx_trunk* t, const float* patches, int64_t n_patch, float* emb,
                            void* workspace, size_t workspace_bytes, int32_t* n_encoded, void* stream);
/* Same, with the per-patch flags (1 = has a non-zero element) already known, e.g. from
 * ipsx_patchify_sparse: the pass that reads every patch to find the blank ones is skipped.        */
int ipsx_trunk_encode_dedup_flagged(const ipsx_trunk* t, const float* patches, int64_t n_patch,
                                    const int32_t* nonblank, float* emb, void* workspace,
                                    size_t workspace_bytes, int32_t* n_encoded, void* stream);

/* ipsx_trunk_encode_parts with exact blank-patch dedup inside the one counted launch: emb, done[] and every argument they
 * share mean what they mean there, and emb is bit for bit what that call writes WHEN blank_emb (128 floats on the device) is
 * the embedding this trunk gives an all-zero patch - the caller computes it once per weight state, with
 * ipsx_trunk_encode_parts on one zero patch.  A scan finds the all-zero list entries (-0.0 counts as zero; it stops reading a
 * patch at the first KiB that holds a non-zero bit), writes blank_emb to their rows and counts them into done[]; an ordered
 * compaction lists the others, and the trunk launch encodes only those, each to its own row, and counts them.  No copy of the
 * embeddings, no host synchronisation.  n_encoded (device int32, or NULL) receives the number of entries encoded, the
 * non-blank ones.  float32 patches, the exact fp32 fused 1x32x32 trunk (precision 0, patch_dtype 0), n_parts <= 16; anything
 * else: IPSX_EINVAL, nothing launched.  workspace: ipsx_trunk_parts_dedup_workspace_bytes(t, n_index) bytes, 8-byte aligned. */
size_t ipsx_trunk_parts_dedup_workspace_bytes(const ipsx_trunk* t, int64_t n_index);
int ipsx_trunk_encode_parts_dedup(const ipsx_trunk* t, const float* patches, const int32_t* index, int64_t n_index, float* emb,
                                  const int64_t* part_end, int n_parts, int32_t* done, const float* blank_emb, void* workspace,
                                  size_t workspace_bytes, int32_t* n_encoded, void* stream);

/* ipsx_trunk_encode_parts_dedup on the other three sources of the counted launch.  patches / images / table / v mean what they
 * mean for ipsx_trunk_encode_parts_u8, ipsx_trunk_encode_parts_view and ipsx_trunk_encode_parts_view_u8 (index: patch numbers,
 * or grid patch numbers of the view), everything from blank_emb on what it means for ipsx_trunk_encode_parts_dedup, and emb is
 * bit for bit what the entry without `_dedup` writes.  float32 images: a grid patch is blank when all its pixels are zero
 * (-0.0 counts), blank_emb as above.  BYTES: an entry is blank when every byte of the patch is 0, and blank_emb is the
 * embedding of such a patch - of a patch whose every pixel is table[c][0], which need NOT be 0.0f (a normalising table): the
 * caller computes it with ipsx_trunk_encode_parts_u8 on one patch of zero bytes, once per weight state AND per table.  A patch
 * of another byte whose table entry happens to be 0.0f is not blank by this rule; it is encoded, to the same bits.  The same
 * trunk, alignments and limits as the entries without `_dedup`; anything else, a missing table or view among it: IPSX_EINVAL
 * (workspace: IPSX_EWORKSPACE), nothing launched, no row and no counter written.  workspace:
 * ipsx_trunk_parts_dedup_workspace_bytes(t, n_index) bytes, 8-byte aligned, for all four. */
int ipsx_trunk_encode_parts_dedup_u8(const ipsx_trunk* t, const uint8_t* patches, const float* table, const int32_t* index,
                                     int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                     const float* blank_emb, void* workspace, size_t workspace_bytes, int32_t* n_encoded,
                                     void* stream);
int ipsx_trunk_encode_parts_dedup_view(const ipsx_trunk* t, const float* images, const ipsx_patch_view* v, const int32_t* index,
                                       int64_t n_index, float* emb, const int64_t* part_end, int n_parts, int32_t* done,
                                       const float* blank_emb, void* workspace, size_t workspace_bytes, int32_t* n_encoded,
                                       void* stream);
int ipsx_trunk_encode_parts_dedup_view_u8(const ipsx_trunk* t, const uint8_t* images, const float* table, const ipsx_patch_view* v,
                                          const int32_t* index, int64_t n_index, float* emb, const int64_t* part_end, int n_parts,
                                          int32_t* done, const float* blank_emb, void* workspace, size_t workspace_bytes,
                                          int32_t* n_encoded, void* stream);

/* ---------------------------------------------------------- image -> patches
 * The step that feeds ips(): replaces, for a whole batch on the device,
 *   img.unfold(1, ph, sh).unfold(2, pw, sw).permute(1, 2, 0, 3, 4).reshape(-1, C, ph, pw)
 * of data/megapixel_mnist/mnist_dataset.py:44-51 and data/traffic/traffic_dataset.py:336-343.
 * img (b,c,h,w) -> patches (b, ny*nx, c, ph, pw), ny = (h-ph)/sh+1, nx = (w-pw)/sw+1, patch order
 * row-major over (py, px).  ipsx_patchify_count returns ny*nx (0 for an invalid geometry).         */
int64_t ipsx_patchify_count(int h, int w, int ph, int pw, int sh, int sw);
int ipsx_patchify(const float* img, int b, int c, int h, int w, int ph, int pw, int sh, int sw,
                  float* patches, void* stream);
/* Megapixel-MNIST's on-disk form straight to patches (mnist_dataset.py:34-51): image i owns the
 * non-zeros [offsets[i], offsets[i+1]) of (index, value); index is the flat position in an (h, w, c)
 * canvas (the reference's _img_shape), value its pixel.  patches is zeroed and filled; nonblank
 * (b*ny*nx int32, or NULL) is set to 1 for every patch that received a non-zero value.  Indices
 * outside the canvas are skipped (the host validates them before upload; numpy would raise).
 * offsets, index and value are device pointers; nnz = offsets[b] - and no entry at or past nnz is read, whatever
 * offsets[b] holds: nnz is what index and value are known to hold.  Element-sized loads only (any aligned int64 / float). */
int ipsx_patchify_sparse(const int64_t* index, const float* value, const int64_t* offsets, int64_t nnz,
                         int b, int c, int h, int w, int ph, int pw, int sh, int sw,
                         float* patches, int32_t* nonblank, void* stream);

/* Replaces IPSNet.encoder as built by get_projector (ips_net.py:54-60):
 * ReLU(BN1d(Linear(LayerNorm_noaffine(x)))); x (n,f) -> out (n,d).
 * `lin` is the Linear packed as a 1x1 conv (c_in=f, c_out=d; f % 32 == 0) whose alpha/shift
 * hold the BatchNorm affine with the Linear bias folded into shift
 * (shift' = fma(bias, alpha, shift)) and whose colsum holds ipsx_weight_colsum of the weights.
 * The LayerNorm is folded into the GEMM's epilogue (see "Arithmetic contract") from a (mean, rstd)
 * pass; workspace: ipsx_projector_workspace_bytes(n).                                              */
/* cs[o] = sum over c of w[o][c] of a Linear's (c_out, c_in) fp32 weights: ascending in float64, rounded once */
int ipsx_weight_colsum(const float* w, int c_out, int c_in, float* colsum, void* stream);
int ipsx_projector(const ipsx_conv* lin, const float* x, int64_t n, float ln_eps,
                   float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t ipsx_projector_workspace_bytes(int64_t n);      /* 8 bytes per row: (mean, rstd); rstd < 0: a centred row (above) */
/* the two halves of ipsx_projector, for callers that compute the row statistics (n x 2 floats: mean, rstd) ahead of
 * the GEMM - e.g. on another stream, beside the GEMM of an earlier slab (the pass is HBM-bound, the GEMM MFMA-bound) */
int ipsx_projector_stats(const float* x, int64_t n, int f, float ln_eps, float* stats, void* stream);
int ipsx_projector_apply(const ipsx_conv* lin, const float* x, int64_t n, const float* stats, float* out, void* stream);
/* ipsx_projector_apply that also does what ipsx_publish_rows(ready, value) does, at its start: the launches enqueued before
 * it (the logits of the previous slab) have completed, which is all a publication says - one launch less per slab in a
 * pipeline that feeds ipsx_scan_persistent. */
int ipsx_projector_apply_publish(const ipsx_conv* lin, const float* x, int64_t n, const float* stats, float* out,
                                 int32_t* ready, int32_t value, void* stream);

/* The projector on the bf16 matrix pipe (3.03; IPSX_PRECISION=bf16 for feature nets): rows stored as
 * dtype 0 = float32, 1 = bfloat16, 2 = float16.  ipsx_projector_stats_typed: the fp32 moments of the stored values widened
 * exactly - dtype 0 is ipsx_projector_stats, a half-stored row gets the bits of the same values passed as float32.
 * ipsx_projector_apply_bf16: out = ReLU(alpha * (|rstd| * sum_k bf16(x - mean) * bf16(W)) + shift), centred in fp32 and
 * rounded to bf16 in the operand load, fp32 accumulation in one fixed k order; lin->w_packed_bf16 =
 * ipsx_pack_conv_weight_bf16 of the (d, f) weights as a 1x1 convolution (lin->colsum is not read).  Needs f % 16 == 0,
 * d % 32 == 0 (ipsx_projector_bf16_supported) and rows at 16-byte addresses.  ready (or NULL): what
 * ipsx_projector_apply_publish does with it. */
int ipsx_projector_stats_typed(const void* x, int dtype, int64_t n, int f, float ln_eps, float* stats, void* stream);
int ipsx_projector_bf16_supported(const ipsx_conv* lin);
int ipsx_projector_apply_bf16(const ipsx_conv* lin, const void* x, int dtype, int64_t n, const float* stats, float* out,
                              int32_t* ready, int32_t ready_value, void* stream);

/* ONE image's patches through the fused 1x32x32 trunk AND their logits as ONE persistent launch that feeds
 * ipsx_scan_persistent patch by patch (reference: self.encoder(...) chunk by chunk in IPSNet.ips, architecture/ips_net.py:
 * 213-241, and transformer.py:71-83 for the logits of emb + pos): resident workgroups pull two patches at a time, encode
 * them (out: emb (n_patch, 128)), compute their logits against the folded query v_packed from emb + pos (pos: (n_patch,
 * 128) or NULL; out: logits (n_patch, r)) and advance *ready past every completed pair in order.  Bit-identical to
 * ipsx_trunk_encode + ipsx_logits.  ctl: ipsx_trunk_stream_ctl_words(n_patch) int32 words ZEROED before every call.
 * workgroups <= 0: a few more than compute units (one that finds no unit at once starts late or finds nothing left);
 * quad_pulls: a workgroup's first quad_pulls pulls are four patches (the trunk's full rate), the rest two (the finer
 * deal); < 0: as many as leave a round of two-patch pulls.                                                              */
size_t ipsx_trunk_stream_ctl_words(int64_t n_patch);
int ipsx_trunk_stream_supported(const ipsx_trunk* t, int d, int r);
int ipsx_trunk_stream(const ipsx_trunk* t, const float* patches, int64_t n_patch, float* emb, const float* pos,
                      const float* v_packed, int r, float* logits, int32_t* ctl, int32_t* ready, int workgroups,
                      int quad_pulls, void* stream);
/* 3.06: ipsx_trunk_stream reading patch index[j] of `patches` (src_patches of them, float32) where it reads patch j;
 * everything else (emb, pos, logits, ctl, ready: in OUTPUT numbering) as there - the bits of ipsx_trunk_stream on the
 * gathered tensor patches[index].  index == NULL is ipsx_trunk_stream.  The tiles read index[j] as it is: every entry must
 * lie in [0, src_patches) (ipsx_order_index composes such an index from any permutation).  Refused before the launch: what
 * ipsx_trunk_stream refuses, src_patches < 1, an index with n_patch > 0x7FFFFFF0. */
int ipsx_trunk_stream_indexed(const ipsx_trunk* t, const float* patches, const int32_t* index, int64_t src_patches,
                              int64_t n_patch, float* emb, const float* pos, const float* v_packed, int r,
                              float* logits, int32_t* ctl, int32_t* ready, int workgroups, int quad_pulls, void* stream);

/* The projector AND the logits of one slide as ONE persistent launch that feeds ipsx_scan_persistent row by row
 * (reference: the projector of architecture/ips_net.py:60-66 applied chunk by chunk in IPSNet.ips :213-241, and
 * transformer.py:71-83 for the logits).  Resident workgroups pull 64-row tiles off a counter; a tile's Linear (its rows'
 * LayerNorm moments come off the GEMM's own operand registers: every row is read once) + folded LayerNorm + BatchNorm +
 * ReLU (out: emb, (n, 512)), and logits against the folded query v_packed
 * (ipsx_fold_query; r = h * n_token <= 32; out: logits (n, r)) are computed in place, and `*ready` - the progress word
 * of the selection loop - is advanced past every completed 32-row unit in order.  Several slides: x holds them one
 * after the other (n rows in all, slide_rows each, a multiple of 32), ready[s] is slide s's word, and the stream of
 * tiles runs across the slides' ends.  Bit-identical to ipsx_projector_stats + ipsx_projector_apply + ipsx_logits.  ctl: ipsx_projector_stream_ctl_words(n) int32 words, the first ipsx_projector_stream_ctl_zero_words(n) of them ZEROED before every call (3.02; the rest are hand-over accumulators, written before they are read).
 * workgroups <= 0: 7 of every 8 compute units (the loop's unit stays free); short_first >= 0: that many workgroups
 * start with a 32-row tile, -1: half of them (completions then do not come in bursts), -2: every tile is 32 rows (a
 * steady supply at 12 % less throughput), -3 - (head + 8 tail), head < 8: every workgroup's first `head` pulls and the
 * last `tail` x workgroups units are 32-row tiles (early first rows, an even end; head = 0: half the workgroups start
 * short as with -1), and the few units left over when every workgroup has had its whole share go out as four column
 * quarters each (the logits' accumulators pass from quarter to quarter: the same bits).  ipsx_projector_stream_supported: 1x1 Linear with
 * 512 outputs and its column sums (lin->colsum), c_in % 32 == 0, 64 <= n < 2^31.                    */
size_t ipsx_projector_stream_ctl_words(int64_t n);
size_t ipsx_projector_stream_ctl_zero_words(int64_t n);
int ipsx_projector_stream_supported(const ipsx_conv* lin, int64_t n, int r);
/* 3.06: the row-indexed feature producers.  Output row j (stats, out, emb, logits, the 32-row units and the `ready`
 * progress, all in output order) is computed from source row index[j] of the (src_rows, F) tensor x: index is a flat
 * int32 row number, the row base is computed in 64 bits (x may be many GB), a number outside [0, src_rows) is clamped
 * into it.  Per-row arithmetic and k-order are those of the plain entry points - the results are the bits of the plain
 * kernel run on the gathered tensor x[index] - and every other argument means what it means there (ready may be NULL
 * in the two apply forms).  A feature row is 4-8 KB of contiguous memory: a gathered row costs no coalescing. */
int ipsx_projector_stats_indexed(const void* x, int dtype, const int32_t* index, int64_t src_rows, int64_t n, int f,
                                 float ln_eps, float* stats, void* stream);
int ipsx_projector_apply_indexed(const ipsx_conv* lin, const float* x, const int32_t* index, int64_t src_rows, int64_t n,
                                 const float* stats, float* out, int32_t* ready, int32_t value, void* stream);
int ipsx_projector_apply_bf16_indexed(const ipsx_conv* lin, const void* x, int dtype, const int32_t* index, int64_t src_rows,
                                      int64_t n, const float* stats, float* out, int32_t* ready, int32_t ready_value,
                                      void* stream);
int ipsx_projector_stream_indexed(const ipsx_conv* lin, const float* x, const int32_t* index, int64_t src_rows, int64_t n,
                                  int64_t slide_rows, float ln_eps, float* emb, const float* v_packed, int r, float* logits,
                                  int32_t* ctl, int32_t* ready, int workgroups, int short_first, void* stream);
int ipsx_projector_stream(const ipsx_conv* lin, const float* x, int64_t n, int64_t slide_rows, float ln_eps, float* emb,
                          const float* v_packed, int r, float* logits, int32_t* ctl, int32_t* ready,
                          int workgroups, int short_first, void* stream);

/* ------------------------------------------------------------------- scorer
 * Replaces MultiHeadCrossAttention.get_attn + ScaledDotProductAttention.
 * compute_attn + Transformer.get_scores (architecture/transformer.py:29-34,
 * 71-83, 143-148) and IPSNet.score_and_select (ips_net.py:136-155).          */

/* qs[t][o] = (sum_c q[t][c]*wq[o][c]) / temperature; q (T,D), wq (H*Dk,D)
 * (transformer.py:76 and the division of :31)                               */
int ipsx_query_proj(const float* q, const float* wq, float temperature,
                    int n_token, int d, int hdk, float* qs, void* stream);

/* Attention logits before the softmax (transformer.py:77,31: matmul(q / temperature, k_w(x)^T)):
 *   logit[n][h*T + t] = sum_j qs[t][h,j] * sum_c W_k[h*dk + j][c] * x[n][c],   x = emb (+ pos)
 * evaluated with the query folded into the key weights (the two sums commute; this order is the arithmetic
 * contract, restated by the oracle):  v = ipsx_fold_query(qs, wk_packed)  once per call, then
 * logit[n][r] = sum_c x[n][c] * v[r][c]  on the matrix cores - H*T*D multiply-adds per patch instead of
 * H*Dk*D, so the kernel is bound by reading the embeddings.
 * emb (b,n,d) with batch stride emb_bstride (floats); pos (b|1,n,d) or NULL, pos_bstride = 0 broadcasts one
 * (n,d) table over the batch; wk_packed = ipsx_pack_conv_weight of k_w.weight viewed as (H*Dk, D, 1, 1);
 * v_packed: ipsx_folded_query_elems(h, n_token, d) floats; r = h * n_token; logits (b,n,r).
 * Alignment: v_packed at a 16-byte address, always; with d % 8 == 0 the rows of emb and pos are read with 16-byte loads
 * and there is no scalar route - emb, pos at 16-byte addresses, emb_bstride and pos_bstride multiples of 4 floats (d % 8 != 0
 * takes 4-byte loads).  logits is written with 4-byte stores: any row range of a longer table.  The same holds for
 * ipsx_logits_if, ipsx_logits_stats (stats_out: 8-byte stores), x of ipsx_scores and x of ipsx_aggregate*.  None of this is
 * tested by the entry points: ips_amd/hip.py copies a read-only view that misses it. */
size_t ipsx_folded_query_elems(int h, int n_token, int d);
int ipsx_fold_query(const float* qs, const float* wk_packed, int h, int dk, int n_token, int d,
                    float* v_packed, void* stream);
int ipsx_logits(const float* emb, int64_t emb_bstride,
                const float* pos, int64_t pos_bstride,
                const float* v_packed,
                int b, int64_t n, int d, int r,
                float* logits, int64_t logits_bstride, void* stream);

/* 3.06: ipsx_logits as a conditional launch - every workgroup returns at once unless (*cond & cond_mask) != 0 (device int32) */
int ipsx_logits_if(const float* emb, int64_t emb_bstride, const float* pos, int64_t pos_bstride,
                   const float* v_packed, int b, int64_t n, int d, int r,
                   float* logits, int64_t logits_bstride, const int32_t* cond, int32_t cond_mask, void* stream);

/* BASELINE configs[4]: the same logits on the bf16 matrix pipe - x = emb (+ pos) rounded to bfloat16, the folded query
 * rounded to bfloat16 (ipsx_fold_query_bf16: ipsx_folded_query_bf16_bytes(h, n_token, d) bytes, from the float32 folded
 * query's inputs), float32 accumulation.  No reference behaviour to match: tolerance-tested against ipsx_logits.   */
size_t ipsx_folded_query_bf16_bytes(int h, int n_token, int d);
int ipsx_fold_query_bf16(const float* qs, const float* wk_packed, int h, int dk, int n_token, int d,
                         void* v_packed_bf16, void* stream);
int ipsx_logits_bf16(const float* emb, int64_t emb_bstride, const float* pos, int64_t pos_bstride,
                     const void* v_packed_bf16, int b, int64_t n, int d, int r,
                     float* logits, int64_t logits_bstride, void* stream);

/* Order of equal scores in the top-M steps of ipsx_scan / ipsx_scan_range / ipsx_topm (process-wide).
 * 1 (default) = the reference's: torch.topk on CPU returns what libstdc++'s nth_element + sort (or
 * partial_sort when 64*M <= L) leave behind (ATen/native/TopKImpl.h:45-68, reference call site
 * ips_net.py:148); those routines are replayed on the device - by ipsx_topm whenever two of the first M+1
 * ranked scores are equal; by the selection loops (ipsx_scan*, round 5) when two NEIGHBOURS among the first
 * M+1 canonical ranks have equal scores AND bit-identical logit rows (duplicated patches: they tie in the
 * reference's arithmetic as well, so its order there is torch's) - two different rows whose scores collide in
 * the last bit of THIS arithmetic keep the canonical order (in the reference's arithmetic they are an ulp apart).
 * 2 = the loops replay on every tie too (rounds 1-4).
 * 0 = canonical: score descending, earlier candidate position first (no sequential step).
 * Returns the previous mode; any other argument only queries.                                       */
int ipsx_set_tie_order(int mode);

/* The chunk loop of IPSNet.ips (ips_net.py:213-241) on cached logits
 * (b, n, h*T): memory = first m patches; for every chunk of `i` further
 * patches: candidates = memory ++ chunk, per-(h,t) softmax over candidates,
 * mean over h then t, keep top m (score descending, ties: earlier candidate
 * position first).  One workgroup per image, one launch for the whole loop.
 * mem_idx (b,m) int64 = selected patch indices in final score order;
 * mem_score (b,m) or NULL; tie_flag (b) int32 or NULL: set when two candidates
 * straddling a top-m boundary had bit-equal scores (the reference's own order is
 * then implementation-defined, ips_net.py:199).
 * Alignment (every ipsx_scan* entry point): logits at a 16-byte address - the loops
 * for candidate sets beyond the LDS and the 8-row shapes load rows as float4 and
 * have no scalar route; mem_idx 8, mem_score / tie_flag / the int32 words 4.     */
int ipsx_scan(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
              int64_t* mem_idx, float* mem_score, int32_t* tie_flag,
              void* workspace, size_t workspace_bytes, void* stream);

/* Candidate sets that do not fit one compute unit's LDS - m + i above ~4,000, up to 16,384; the reference's shipped
 * CAMELYON configuration is m = i = 5000 (config/camelyon_config.yml:35-36, torch.topk over 10,000 candidates,
 * ips_net.py:148) - keep only the ranking in LDS and need a caller-owned device workspace of this many bytes (0 = none
 * needed, workspace may be NULL).  ipsx_scan / ipsx_scan_range return IPSX_EWORKSPACE when it is missing or too small. */
size_t ipsx_scan_workspace_bytes(int b, int m, int i, int h, int n_token);
/* Workgroups (= compute units) the loop of ONE image occupies for a call of b images: 1 for every LDS-resident shape; the
 * shapes above with 8 heads and one token - the shipped CAMELYON configuration - run as a TEAM of up to 8 workgroups per
 * image that share the element-wise passes and pre-sort their shares of the ranking (csrc/scan_large_team.h; same results).
 * A caller that launches a persistent producer beside persistent loops leaves b x this many units free (3.02). */
int ipsx_scan_workgroups_per_image(int b, int m, int i, int h, int n_token);

/* Iterations [it_begin, it_end) of the same loop.  it_begin = 0 starts from the first m patches, it_begin > 0
 * resumes from the state a previous call left in mem_idx; only logits rows below m + it_end*i are read, so a
 * range can run (on another stream) while later patches are still being encoded.  tie_flag is only ever SET.  */
int ipsx_scan_range(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                    int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                    int32_t* tie_flag, void* workspace, size_t workspace_bytes, void* stream);
/* 3.06: ipsx_scan_range on logits that sit in a table of fixed capacity - image k's rows start k * logits_bstride_rows rows
 * behind image 0's (>= n), the first n of them are the candidates.  ipsx_scan_range is this call with
 * logits_bstride_rows = n: same kernels, same launch shapes, same results.  A stream's candidate table (IPSNet.ips_stream:
 * the memory's m rows in rank order, then the carried rows, then the fed piece's) is scanned this way from it_begin = 0:
 * mem_idx then holds row numbers of that table. */
int ipsx_scan_range_strided(const float* logits, int64_t logits_bstride_rows, int b, int64_t n, int m, int i, int h,
                            int n_token, int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                            int32_t* tie_flag, void* workspace, size_t workspace_bytes, void* stream);
/* 3.06: ipsx_scan on b slides of DIFFERENT lengths in one launch.  The slides' logits lie one after the other in one packed
 * (total, h * n_token) table; row_offsets (device, b + 1 int64, ascending from 0 to total) says where each starts.  Slide k is
 * scanned as ipsx_scan scans a contiguous copy of its rows alone - its own n = row_offsets[k + 1] - row_offsets[k], its own
 * ceil((n - m) / i) iterations and ragged last chunk - by one workgroup (plain launches only; never a team of workgroups):
 * mem_idx (b, m) holds slide-LOCAL row numbers, mem_score and tie_flag are per slide as ipsx_scan leaves them.  No row at or
 * behind row_offsets[k + 1] is read for slide k.  n_max (the longest slide) and total are the caller's host-side knowledge
 * (dispatch, the < 2^31 checks); the caller guarantees that EVERY slide has more than m rows - a slide that has not, or
 * whose offsets leave the table, is left untouched.  workspace: b times ipsx_scan_workspace_bytes(1, m, i, h, n_token). */
int ipsx_scan_ragged(const float* logits, const int64_t* row_offsets, int b, int64_t n_max, int64_t total, int m, int i,
                     int h, int n_token, int64_t* mem_idx, float* mem_score, int32_t* tie_flag, void* workspace,
                     size_t workspace_bytes, void* stream);
/* 3.06: ipsx_scan_ragged on slides that lie ANYWHERE in one (rows_total, h * n_token) table.  spans (device, (b, 2) int64):
 * the first row and the row count of slide k's candidates; the spans need not touch each other nor ascend.  Slide k is scanned
 * as ipsx_scan_ragged scans a slide of that many rows - its own ceil((count - m) / i) iterations and ragged last chunk - by one
 * workgroup (a plain launch; never a team, never the kernel specialised for 8 heads x 4 tokens): mem_idx holds row numbers
 * inside the span.  A slide whose count is not above m, or whose span leaves [0, rows_total), is left untouched in all three
 * outputs - tie_flag is only ever SET here, the caller clears it.  No row outside a span is read.  n_max: the caller's
 * host-side bound on the counts (dispatch, the < 2^31 checks).  workspace: b times ipsx_scan_workspace_bytes(1, m, i, h,
 * n_token). */
int ipsx_scan_ragged_spans(const float* logits, const int64_t* spans, int b, int64_t n_max, int64_t rows_total, int m, int i,
                           int h, int n_token, int64_t* mem_idx, float* mem_score, int32_t* tie_flag, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The whole loop as ONE launch that may start before any logits exist (overlap with the encoder without re-launching
 * per part): the kernel waits until *ready (device int32, written with ipsx_publish_rows on another stream after the
 * kernels that produced the rows) says the rows it is about to read are in memory.  The wait is bounded: 50 ms (see
 * ipsx_set_persistent_wait_ms) WITHOUT PROGRESS of any of the call's progress words; on a timeout, or when *ready is set
 * negative, the kernel ends and sets bit 0 of *status (results are then invalid - ipsx_scan_range_if behind it redoes the
 * loop in the same call; bit 1 = the kernel is resident).  ready_per_image != 0: `ready` is an array of b words and image k follows ready[k] - a
 * producer that works through the images one after the other publishes each image's rows as it goes, and image k's loop
 * runs beside the production of image k + 1.
 * Shapes: ipsx_scan_persistent_supported() != 0.     */
int ipsx_scan_persistent_supported(int m, int i, int h, int n_token);
int ipsx_scan_persistent(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                         int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const int32_t* ready,
                         int32_t ready_per_image, int32_t* status, void* stream);
/* ipsx_scan_persistent with FEWER resident workgroups than images (0 < workgroups < b; otherwise one per image):
 * workgroup w runs the loops of images w, w + workgroups, ... one after the other - for a producer that works through
 * the images in order and needs longer for an image than its loop does (the projector of 16 CAMELYON slides: two
 * resident loops keep up, and 14 more compute units stay the projector's).  Shapes: ipsx_scan_persistent_groupable(). */
int ipsx_scan_persistent_groupable(int m, int i, int h, int n_token);
int ipsx_scan_persistent_on(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                            int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const int32_t* ready,
                            int32_t ready_per_image, int32_t* status, int workgroups, void* stream);
/* The persistent loop and its conditional recovery launch for EVERY shape ipsx_scan covers: candidate sets beyond the LDS
 * (ipsx_scan_workspace_bytes() > 0: the reference's shipped CAMELYON M = I = 5000) take the workspace of ipsx_scan; for
 * the other shapes these are ipsx_scan_persistent_on / ipsx_scan_range_if and the workspace is ignored (2.03). */
int ipsx_scan_persistent_ws(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                            int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const int32_t* ready,
                            int32_t ready_per_image, int32_t* status, int workgroups, void* workspace,
                            size_t workspace_bytes, void* stream);
int ipsx_scan_range_if_ws(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                          int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                          int32_t* tie_flag, const int32_t* cond, int32_t cond_mask, void* workspace,
                          size_t workspace_bytes, void* stream);
int ipsx_publish_rows(int32_t* ready, int32_t value, void* stream);
/* longest wait of a persistent loop (and of ipsx_scan_gate) without progress, in milliseconds (1 .. 20000; default 50);
 * returns the previous value, ms <= 0 only queries */
int ipsx_set_persistent_wait_ms(int ms);
/* ipsx_scan_range that runs only when (*cond & cond_mask) != 0, tested ON THE DEVICE by every workgroup as it starts (no
 * host synchronisation): enqueued behind ipsx_scan_persistent with cond = its status word and mask 1, it redoes the loop
 * with plain launches in the very call whose persistent loop gave up waiting, and costs one empty launch otherwise.
 * Shapes of the LDS-resident loops (ipsx_scan_workspace_bytes() == 0). */
int ipsx_scan_range_if(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                       int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                       int32_t* tie_flag, const int32_t* cond, int32_t cond_mask, void* stream);
/* A range of the loop whose launch computes its own logits: ipsx_logits of the parts [part_begin, part_end) and ipsx_scan_range
 * of the iterations [it_begin, it_end) in ONE launch, bit for bit.  Workgroup k of the loop reads image k's logits alone, and
 * a patch's logits depend on that patch alone, so in front of its first iteration it writes image k's rows of those parts
 * into `logits` (b, n, r) itself - no logits launch, no dependency between workgroups.  The embeddings of a call lie
 * part-major: parts[j] = {emb: (b, rows, d) float32 at a 16-byte address, rows per image, first row of the part in an
 * image}, n_parts <= 16, in order and tiling [0, n); pos (b | 1, n, d) of whole images or NULL, pos_bstride 0 broadcasts.
 * The rows the iterations read end inside part part_end - 1 at the latest; those in front of part_begin are in `logits`
 * (part_begin == part_end: all of them - the launch computes no rows unless it redoes the call).
 * redo (device int32, or NULL with mask 0): with (*redo & redo_mask) != 0 - a part wait of the call gave up (ipsx_part_wait)
 * - the launch computes ALL parts and runs the iterations [0, it_end): the conditional redo of ipsx_logits_if /
 * ipsx_scan_range_if, in the launch of the call's last part.
 * Shape: 8 heads x 4 tokens, m = i = 64 (r = 32), d % 8 == 0; anything else: IPSX_EINVAL, nothing launched.
 * ipsx_scan_logits_check: the arithmetic of the part table and the two ranges alone, on the host (no device needed). */
typedef struct ipsx_logits_part {
    const float* emb;
    int64_t rows;
    int64_t first;
} ipsx_logits_part;
int ipsx_scan_logits_check(const ipsx_logits_part* parts, int n_parts, int part_begin, int part_end, int64_t n, int m, int i,
                           int64_t it_begin, int64_t it_end);
int ipsx_scan_range_logits(float* logits, int b, int64_t n, int m, int i, int h, int n_token, int64_t it_begin, int64_t it_end,
                           int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const ipsx_logits_part* parts, int n_parts,
                           int part_begin, int part_end, int d, const float* pos, int64_t pos_bstride, const float* v_packed,
                           const int32_t* redo, int32_t redo_mask, void* stream);
/* ipsx_scan_range_logits between two launches on DIFFERENT streams with no stream wait between them: the same arguments, and
 *   gate_publish (b int32, or NULL): at its very end workgroup k stores it_end to gate_publish[k], behind its stores of
 *            mem_idx / mem_score / tie_flag (an agent-scope release in front of the word);
 *   gate, gate_target (b int32 zeroed by the caller before either launch, or NULL and 0): behind its prologue - the rows of its
 *            parts, which need nothing of the other stream - workgroup k waits until gate[k] >= gate_target (it_begin or later),
 *            then runs its iterations.  A wait that sees no progress of its word for ipsx_set_persistent_wait_ms sets status_bit
 *            in *status and does in its workgroup what redo does: every part's rows, the iterations [0, it_end).  With redo set
 *            on entry the (bounded) wait comes first;
 *   mem_out  (b, m) int64 other than mem_idx, or NULL: the final indices go there and mem_idx is only read - a launch that
 *            gave up may have a late launch of the other stream writing mem_idx behind it.
 * A gate without its target, or without status and status_bit: IPSX_EINVAL.  Always the one launch (ipsx_dbg_scan_logits is
 * not consulted). */
int ipsx_scan_range_logits_gate(float* logits, int b, int64_t n, int m, int i, int h, int n_token, int64_t it_begin, int64_t it_end,
                                int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const ipsx_logits_part* parts, int n_parts,
                                int part_begin, int part_end, int d, const float* pos, int64_t pos_bstride, const float* v_packed,
                                const int32_t* redo, int32_t redo_mask, const int32_t* gate, int32_t gate_target,
                                int32_t* gate_publish, int32_t* status, int32_t status_bit, int64_t* mem_out, void* stream);
/* ipsx_logits for rows [0, n) and, in the SAME launch, the LayerNorm row moments (ipsx_projector_stats) of stats_n rows
 * of stats_x - the next slab the projector is about to take: two short latency-bound launches of a slab-by-slab producer
 * of ipsx_scan_persistent as one. */
int ipsx_logits_stats(const float* emb, int64_t emb_bstride, const float* pos, int64_t pos_bstride,
                      const float* v_packed, int b, int64_t n, int d, int r, float* logits, int64_t logits_bstride,
                      const float* stats_x, int64_t stats_n, int stats_f, float ln_eps, float* stats_out, void* stream);
/* holds `stream` (one waiting thread, bounded) until the persistent scan that owns `status` is resident: enqueue it on
 * the producing stream right after launching the scan, so that the producers do not take the compute units first */
int ipsx_scan_gate(const int32_t* status, void* stream);

/* Transformer.get_scores on arbitrary embeddings x (b,l,d) -> scores (b,l);
 * attn (b,h,T,l) optionally written too (get_attn).                          */
int ipsx_scores(const float* x, const float* wk_packed, const float* qs,
                int b, int l, int d, int h, int dk, int n_token,
                float* scores, float* attn, void* workspace, size_t workspace_bytes,
                void* stream);
size_t ipsx_scores_workspace_bytes(int b, int l, int d, int h, int n_token);

/* torch.topk(scores, m, dim=-1)[1] (ips_net.py:148): (b,l) -> (b,m) int64, l <= 16,384.  Rows beyond the LDS
 * (l above ~8,000) need ipsx_topm_workspace_bytes(b, l, m) bytes of device workspace (0 = none, NULL allowed). */
int ipsx_topm(const float* scores, int b, int l, int m, int64_t* top_idx,
              int32_t* tie_flag, void* workspace, size_t workspace_bytes, void* stream);
size_t ipsx_topm_workspace_bytes(int b, int l, int m);

/* ------------------------------------------------------------------- gather
 * Replaces the torch.gather calls of ips_net.py:245-250: dst[b][j] = src[b][idx[b][j]]
 * for rows of row_bytes bytes (16 / 4 per lane where size and addresses allow, else by bytes).  src_bstride_rows = rows between
 * batches of src (0 = one table shared by all batches).                       */
int ipsx_gather_rows(const void* src, const int64_t* idx, void* dst,
                     int b, int64_t n_rows, int m, int64_t row_bytes,
                     int64_t src_bstride_rows, void* stream);

/* The end of IPSNet.ips (architecture/ips_net.py:243-250: mem_patch = patches[mem_idx], mem_pos = pos_enc[mem_idx]) in ONE
 * launch for calls whose selection ran as a resident loop: both gathers (rows of 16-byte units; pos may be NULL;
 * *_bstride_rows = rows per image, 0 = one table for every image), a fresh copy of the loop's (b, m) index buffer, and -
 * status_host != NULL - the loop's status word stored to its pinned host mirror (read by the caller one call later). */
int ipsx_ips_finish(const void* patches, int64_t patch_row_bytes, int64_t patch_bstride_rows, int64_t n_rows,
                    const void* pos, int64_t pos_row_bytes, int64_t pos_bstride_rows, const int64_t* mem_idx, int b, int m,
                    void* mem_patch, void* mem_pos, int64_t* mem_idx_out, const int32_t* status, int32_t* status_host,
                    void* stream);
/* 3.06: ipsx_ips_finish after a selection that ran on a permuted NUMBERING of the patches (row-indexed producers below):
 * mem_patch[b][j] = patches[b][order[b][mem_idx[b][j]]], read from the UNSHUFFLED tensor.  order: (b or 1, n_rows) int64,
 * order_bstride = n_rows, or 0 for one permutation shared by every image.  pos (already in the loop's numbering), mem_pos
 * and mem_idx_out: as in ipsx_ips_finish. */
int ipsx_ips_finish_indexed(const void* patches, int64_t patch_row_bytes, int64_t patch_bstride_rows, int64_t n_rows,
                            const void* pos, int64_t pos_row_bytes, int64_t pos_bstride_rows, const int64_t* mem_idx,
                            const int64_t* order, int64_t order_bstride, int b, int m, void* mem_patch, void* mem_pos,
                            int64_t* mem_idx_out, const int32_t* status, int32_t* status_host, void* stream);

/* 3.06: the end of a PADDED ragged call (IPSNet.ips_ragged(pad=True)) in ONE launch, grid (m, b).  rows: the packed rows of
 * all slides, (total, row_bytes); row_offsets: (b + 1) int64 on the device; mem_idx: (b, m) slide-local, as ipsx_scan_ragged
 * leaves it (the rows of slides with no more than m rows are never read; NULL when no slide is longer); flat: (total) int32
 * or NULL - packed row g is source row flat[g] of `rows` (a shuffle applied as an index); pos: the packed positional rows
 * (total, pos_row_bytes) in packed numbering, or NULL.  Slide k has n = row_offsets[k + 1] - row_offsets[k] rows.
 *   n > m:   slot j takes local row r = clamp(mem_idx[k][j], 0, n - 1);
 *   n <= m:  slot j < n takes r = j; slots j >= n are WRITTEN as zeros (patch and positional row), index and row -1.
 * mem_patch[k][j] = rows[flat ? clamp(flat[g], 0, total - 1) : g], mem_pos[k][j] = pos[g], mem_idx_out[k][j] = r,
 * rows_out[k][j] = g = row_offsets[k] + r.  Nothing is read outside [0, total); a slide whose offsets leave the table is
 * left untouched.  Rows are whole 16-byte units at 16-byte addresses, as ipsx_ips_finish asks. */
int ipsx_ragged_finish(const void* rows, int64_t row_bytes, int64_t total, const int64_t* row_offsets,
                       const int64_t* mem_idx, const int32_t* flat, const void* pos, int64_t pos_row_bytes, int b, int m,
                       void* mem_patch, void* mem_pos, int64_t* mem_idx_out, int64_t* rows_out, void* stream);

/* 3.06: the RAGGED patch-grid view (IPSNet.ips_image_ragged).  Whole images of DIFFERENT sizes, (c, h_k, w_k) each - float32,
 * or uint8 with their table through the _u8 entries at the end of this group, where an element is a byte -, packed into ONE
 * buffer; the patches of all of them numbered one image after the other ("packed patches"), each image's
 * grid in the order of ipsx_patch_view.  One table entry per image: elem_off its first element inside the buffer, first its
 * first packed patch number, ny = (h - ph) / sh + 1, nx = (w - pw) / sw + 1.  Packed patch p belongs to the image k with the
 * largest first <= p and is grid patch p - first of it: it starts at element elem_off + (py * sh) * w + px * sw, its row
 * pitch is w, its channel pitch h * w. */
typedef struct ipsx_image_entry {
    int64_t elem_off;
    int64_t first;
    int32_t h, w, ny, nx;
} ipsx_image_entry;

typedef struct ipsx_ragged_view {
    int b, c, ph, pw, sh, sw;
    const ipsx_image_entry* images;      /* DEVICE: the table of b entries the kernels read */
    const ipsx_image_entry* host;        /* HOST: the same table, as ipsx_ragged_view_fill left it - every entry point checks
                                          * it again and takes the patch count and the launch's load width from it */
} ipsx_ragged_view;

/* host: fills table[0 .. b) from the images' (h[k], w[k], elem_off[k]) and checks it - every field positive (elem_off[0] >=
 * 0), ph <= h, pw <= w, offsets increasing, no image reaching into the next (elem_off[k] + c * h * w <= elem_off[k + 1]),
 * fewer than 2^31 patches in all.  Returns the total patch count, or -1 (ipsx_last_error says why; the table is then not to
 * be used). */
int64_t ipsx_ragged_view_fill(ipsx_image_entry* table, int b, int c, int ph, int pw, int sh, int sw, const int32_t* h,
                              const int32_t* w, const int64_t* elem_off);
/* host: element offset of packed patch p's (0, 0, 0) inside the packed buffer, its row pitch in *pitch and its channel pitch
 * in *chan_pitch (either may be NULL); -1 for a p outside [0, total) or an invalid table.  `geometry`: the view (b, c, patch,
 * stride; its table pointers are not read - `table` is).  The kernels compute their addresses by the same function. */
int64_t ipsx_ragged_view_offset(const ipsx_image_entry* table, int b, const ipsx_ragged_view* geometry, int64_t p,
                                int64_t* pitch, int64_t* chan_pitch);
/* 1 when ipsx_trunk_encode_ragged_view takes this trunk and view: what ipsx_trunk_view_supported asks of the trunk and the
 * patch shape, and a valid host table */
int ipsx_trunk_ragged_view_supported(const ipsx_trunk* t, const ipsx_ragged_view* view);
/* emb row j (j < n) = the embedding of packed patch index[j] (device int32), or of packed patch first + j when index is NULL:
 * bit for bit ipsx_trunk_encode of those patches copied out of their images - the stems' staging code is the view's, only
 * where a patch's first pixel lies and its two pitches are per patch.  A list entry that is no packed patch reads packed
 * patch 0, never outside the buffer.  The load width is picked per launch from the HOST table: the kernel's wide load when
 * `pixels`, every elem_off, every w and sw are multiples of it, dword loads otherwise.  Plain launches only (no counted
 * launch; uint8 images: ipsx_trunk_encode_ragged_view_u8, blank-patch dedup: ipsx_trunk_encode_ragged_view_dedup, both below).
 * workspace: as ipsx_trunk_encode. */
int ipsx_trunk_encode_ragged_view(const ipsx_trunk* t, const float* pixels, const ipsx_ragged_view* view,
                                  const int32_t* index /* NULL: packed patches first .. first+n-1 */, int64_t first, int64_t n,
                                  float* emb, void* workspace, size_t workspace_bytes, void* stream);
/* ipsx_ragged_finish with the source row replaced by a grid patch copied out of its image, grid (m, b).  row_offsets: (b + 1)
 * int64 on the device, the packed patch numbers (entry k = images[k].first, entry b the total); mem_idx, flat, pos and the
 * four outputs as there, mem_patch (b, m, c, ph, pw) float32.  Image k with n = ny * nx patches:
 *   n > m:   slot j takes local patch r = clamp(mem_idx[k][j], 0, n - 1);
 *   n <= m:  slot j < n takes r = j; slots j >= n are WRITTEN as zeros (patch and positional row), index and row -1.
 * The patch copied is grid patch (flat ? flat[g] : g) - a packed number, clamped into [0, total) - with g = first + r;
 * mem_pos[k][j] = pos[g], mem_idx_out[k][j] = r, rows_out[k][j] = g.  16-byte copies where pw, every w, sw and the addresses
 * allow (the host table decides), dwords otherwise.  No read leaves the packed buffer. */
int ipsx_ragged_finish_view(const float* pixels, const ipsx_ragged_view* view, const int64_t* row_offsets, const int64_t* mem_idx,
                            int m, const int32_t* flat, const void* pos, int64_t pos_row_bytes, void* mem_patch, void* mem_pos,
                            int64_t* mem_idx_out, int64_t* rows_out, void* stream);

/* 3.06: exact blank-patch dedup on the ragged view (ipsx_trunk_encode_dedup for images of different sizes).  The fused
 * 1x32x32 trunk at precision 0 on float32 images (uint8 images: the _u8 twins below); every entry checks the view's HOST table again before it launches.
 * nonblank[j] (device int32, n entries) = 1 when entry j's patch - packed patch index[j], or first + j when index is NULL -
 * has a non-zero element (-0.0 is zero, a denormal is not), 0 otherwise.  An entry that is no packed patch is flagged as
 * packed patch 0, the patch the encoder reads for it.  Nothing outside the patch windows is read. */
int ipsx_ragged_view_blank_flags(const float* pixels, const ipsx_ragged_view* view, const int32_t* index,
                                 int64_t first, int64_t n, int32_t* nonblank, void* stream);
/* bytes of device workspace ipsx_trunk_encode_ragged_view_dedup needs for n entries (0 for n <= 0): the flags, the list, the
 * slots (n int32 each), the list's length and the compacted embeddings (n + 1 rows of 128 floats) */
size_t ipsx_trunk_ragged_view_dedup_workspace_bytes(const ipsx_trunk* t, int64_t n);
/* ipsx_trunk_encode_ragged_view, bit for bit, encoding every non-blank entry and ONE blank one.  On one stream, no host
 * synchronisation: the flags (above); the ordered list of the entries to encode - the non-blank ones in list order, then the
 * FIRST blank one - as packed patch numbers, its length and every entry's slot in it, all on the device (sums of integers:
 * the list depends on the data only); the trunk launched for n entries, its workgroups beyond the device-side length
 * returning before they read the list; emb[j] = the row of entry j's slot.  *n_encoded (device int32, may be NULL) = the
 * list's length: the non-blank entries, plus 1 if any entry is blank.  workspace: device memory at a 16-byte address,
 * ipsx_trunk_ragged_view_dedup_workspace_bytes(t, n) bytes (IPSX_EWORKSPACE otherwise).  n = 0 returns IPSX_OK; n >= 2^31, a
 * null pointer and any other trunk are refused (IPSX_EINVAL) before the first launch. */
int ipsx_trunk_encode_ragged_view_dedup(const ipsx_trunk* t, const float* pixels, const ipsx_ragged_view* view,
                                        const int32_t* index /* NULL: packed patches first .. first+n-1 */, int64_t first,
                                        int64_t n, float* emb, void* workspace, size_t workspace_bytes, int32_t* n_encoded,
                                        void* stream);

/* 3.06: the ragged view over whole uint8 images.  `pixels` holds the packed images as bytes, `table` (c x 256 floats, device,
 * at a 16-byte address) the float32 value of every byte per channel, as in ipsx_trunk_encode_view_u8; ipsx_image_entry.elem_off
 * stays an element offset - for bytes an element is a byte - and ipsx_trunk_ragged_view_supported answers for bytes as for
 * floats.  Every entry is, bit for bit, its float32 twin on the expanded buffer table[channel][byte] (which is never made);
 * the exact fp32 trunks only (precision 0, patch_dtype 0).  The load width is picked per launch from the HOST table, the widest
 * of the kernel's own list at which `pixels`, every image's byte offset, every w and sw are multiples: 1x32x32 fused 16 / 4 /
 * 1 bytes (its pair kernel 8 / 4 / 1), 1x50x50 2 / 1, 3x100x100 4 / 1 - single bytes always fit, so any address is taken. */
int ipsx_trunk_encode_ragged_view_u8(const ipsx_trunk* t, const uint8_t* pixels, const float* table, const ipsx_ragged_view* view,
                                     const int32_t* index /* NULL: packed patches first .. first+n-1 */, int64_t first, int64_t n,
                                     float* emb, void* workspace, size_t workspace_bytes, void* stream);
/* ipsx_ragged_finish_view on bytes: mem_patch (b, m, c, ph, pw) is FLOAT32 table[channel][byte] of the copied patch; the
 * padding slots of a short image are written as float +0.0 (not table[channel][0]).  Everything else as there. */
int ipsx_ragged_finish_view_u8(const uint8_t* pixels, const float* table, const ipsx_ragged_view* view, const int64_t* row_offsets,
                               const int64_t* mem_idx, int m, const int32_t* flat, const void* pos, int64_t pos_row_bytes,
                               void* mem_patch, void* mem_pos, int64_t* mem_idx_out, int64_t* rows_out, void* stream);
/* ipsx_ragged_view_blank_flags on bytes: blank means every byte of the 1x32x32 window is 0 (whatever the table makes of 0) */
int ipsx_ragged_view_blank_flags_u8(const uint8_t* pixels, const ipsx_ragged_view* view, const int32_t* index, int64_t first,
                                    int64_t n, int32_t* nonblank, void* stream);
/* ipsx_trunk_encode_ragged_view_u8, bit for bit, by the four steps and the workspace of ipsx_trunk_encode_ragged_view_dedup
 * (ipsx_trunk_ragged_view_dedup_workspace_bytes).  The ONE blank entry is encoded from its image like any other - every pixel
 * table[0] -, so no blank embedding is handed in. */
int ipsx_trunk_encode_ragged_view_dedup_u8(const ipsx_trunk* t, const uint8_t* pixels, const float* table,
                                           const ipsx_ragged_view* view, const int32_t* index, int64_t first, int64_t n, float* emb,
                                           void* workspace, size_t workspace_bytes, int32_t* n_encoded, void* stream);

/* 3.06: the state update of a stream (IPSNet.ips_stream) as ONE launch, for up to four tables at once (patch rows,
 * embeddings, logits, global ids).  The n_cand candidates of a table are two segments that are never joined: its first
 * held_rows rows lie in `held` ((b, held_bstride_rows, row_bytes)), the rest in `piece` - the caller's tensor, which may be
 * a slice: image k's rows start piece_bstride_bytes * k bytes behind `piece` (0: one piece shared by every image).
 *   sel != NULL ((b, m) candidate rows, e.g. what ipsx_scan_range_strided left in mem_idx; clamped into the candidates):
 *       dst[k][j] = cand[k][sel[k][j]] for j < m, dst[k][m + r] = cand[k][tail_first + r] for the n_cand - tail_first
 *       candidates no iteration has consumed; dst is another buffer than held.
 *   sel == NULL (the memory is unchanged - a feed that completes no chunk): dst[k][held_rows + r] = piece[k][r], the rows
 *       in front of them are not touched (dst is normally the buffer `held` points into; tail_first is ignored).
 * Rows are copied 16 / 4 / 1 bytes per lane, chosen per table from row size, addresses and the piece's batch stride.
 * dst_rows: rows per image dst has room for - a call that would write more is refused. */
typedef struct ipsx_stream_table {
    const void* held;
    int64_t held_rows, held_bstride_rows;
    const void* piece;
    int64_t piece_bstride_bytes;
    void* dst;
    int64_t dst_rows, dst_bstride_rows;
    int64_t row_bytes;
} ipsx_stream_table;
int ipsx_stream_commit(const ipsx_stream_table* tables, int n_tables, const int64_t* sel, int b, int m, int64_t n_cand,
                       int64_t tail_first, void* stream);
/* 3.06: ipsx_stream_commit for a stream fed pixel-row bands (IPSStream.feed_rows).  tables[0] is the patch table and has no
 * `piece` pointer: its candidates behind the held rows are patches of `images` ((b, c, h, w), contiguous, elem_size 4: float32
 * | 1: uint8) read through `v` - candidate held_rows + r of image k is grid patch k * ny * nx + r, i.e. c * ph segments of pw
 * elements from element ipsx_patch_view_offset(v, .) + (ch * h + y) * w on, copied raw (bytes stay bytes); its row_bytes is
 * c * ph * pw * elem_size and at most ny * nx candidates lie behind its held rows.  tables[1 ..] keep their contiguous
 * pieces.  Both modes as above.  The patch table is copied 16 / 4 / 1 bytes per lane, ONE width for the launch: the widest of
 * which images, dst, held and w, sw, pw in bytes are all multiples (*unit, when given, says which); no load touches a byte
 * outside a patch row.  Refused before the launch: what ipsx_stream_commit refuses, a view that does not fit its images or
 * has another b, another elem_size, a destination that overlaps the images. */
int ipsx_stream_commit_view(const ipsx_stream_table* tables, int n_tables, const void* images, const ipsx_patch_view* v,
                            int elem_size, const int64_t* sel, int b, int m, int64_t n_cand, int64_t tail_first, int* unit,
                            void* stream);
/* 3.06: ipsx_stream_commit for slides that each have their own numbers (IPSNet.ips_ragged_stream), ONE launch, grid
 * (rows_max, b, n_tables).  tables: as above with these differences - `piece` is ONE packed (piece_rows_total, row_bytes)
 * tensor for all slides (piece_bstride_bytes 0), a table without a piece holds ALL of a slide's candidates in `held`, and
 * held_rows is the number of rows per slide that may be READ from `held` (its capacity).  slides (device, (b, 6) int64), per
 * slide: held rows, candidates, tail_first, the slide's first row in the packed piece, the mode, one reserved word.
 *   mode 0 (idle):   nothing is read or written.
 *   mode 1 (append): dst[k][held + r] = piece[first + r]; the rows in front stay as they are (tables without a piece: nothing).
 *   mode 2 (select): dst[k][j] = cand[k][clamp(sel[k][j])] for j < m, dst[k][m + r] = cand[k][tail_first + r] behind them.
 *   mode 3 (move):   dst[k][j] = cand[k][j] for every candidate.
 * A workgroup beyond its slide's rows returns at once.  Whatever the device table says, nothing is read outside a table's
 * held_rows or the packed piece and nothing is written outside dst_rows: a slide whose numbers contradict the capacities of
 * ANY table of the launch (or that selects without sel, or selects / moves in a table whose dst is its held buffer) is left
 * untouched in all of them.  Refused before the launch: what ipsx_stream_commit refuses that the host can know - a
 * destination that overlaps the piece, or the held rows other than in place from the same address. */
int ipsx_stream_commit_ragged(const ipsx_stream_table* tables, int n_tables, const int64_t* sel, const int64_t* slides, int b,
                              int m, int64_t rows_max, int64_t piece_rows_total, void* stream);
/* 3.06: ipsx_stream_commit_ragged for a ragged stream fed pixel-row bands (RaggedIPSStream.feed_rows).  tables[0] is the patch
 * table and has no `piece` pointer: candidate held + r of slide k is packed patch first_k + r of `view` over `pixels` (the
 * packed 1-d buffer of the feed's windows, elem_size 4: float32 | 1: uint8) - word 3 of the slide's row counts packed patches
 * of the view as it counts rows of the packed pieces of tables[1 ..], which keep them.  The patch's image is resolved by the
 * bisection of the ragged stems, once per workgroup; the patch is copied raw, c * ph segments of pw elements with row pitch w
 * and channel pitch h * w of ITS image (bytes stay bytes); row_bytes of table 0 is c * ph * pw * elem_size.  The view may
 * have fewer entries than the launch has slides.  Table 0 is copied 16 / 4 / 1 bytes per lane, ONE width for the launch: the
 * widest of which pixels, every entry's byte offset, every w, sw and pw in bytes, dst and held are all multiples - decided
 * from the view's HOST table (*unit, when given, says which); no load touches a byte outside a patch row.  Whatever the
 * device tables say, nothing is read outside the pixel buffer (its extent is the host table's) or a table's held_rows and
 * nothing is written outside dst_rows; a slide whose numbers contradict any table of the launch - first + (cand - held)
 * beyond the view's patch count included - is left untouched in all of them.  Refused before the launch: what
 * ipsx_stream_commit_ragged refuses, a view whose host table is invalid or that has no device table, table 0 with a piece
 * pointer or another row_bytes, another elem_size, a destination of table 0 that overlaps the pixels. */
int ipsx_stream_commit_ragged_view(const ipsx_stream_table* tables, int n_tables, const void* pixels, const ipsx_ragged_view* view,
                                   int elem_size, const int64_t* sel, const int64_t* slides, int b, int m, int64_t rows_max,
                                   int64_t piece_rows_total, int* unit, void* stream);

/* ONE IPSNet.ips call whose selection loop is resident (architecture/ips_net.py:169-262 for one image on the fused trunk,
 * or for feature slides through the projector), enqueued by ONE library call: fill of the control words, the loop on
 * `side_stream` (ipsx_scan_persistent_ws), the gate, the producer on `stream` (ipsx_trunk_stream when `trunk` is set -
 * b == 1 -, ipsx_projector_stream when `lin` is set), the conditional recovery launch (ipsx_scan_range_if_ws) and the end
 * of the call (ipsx_ips_finish), with the two cross-stream hand-overs between them.  Same kernels, same results as the
 * entry points called one by one; the host's share of a call drops from ~12 calls to one, and nothing of the caller's
 * runtime (an interpreter's collector or allocator) sits between the launch of the loop and the launch of the producer it
 * waits for - a host thread the OS deschedules there still can: the loop's wait is bounded and the call then redoes it.
 *   words: words_total int32 = tie flags [b] | progress words [b] | status | the producer's control words
 *          (ipsx_trunk_stream_ctl_words / ipsx_projector_stream_ctl_words); zeroed by the call (what has to be: see ipsx_projector_stream_ctl_zero_words).
 *   timing_slot in [0, 64): the producer's launch is bracketed by a library-owned HIP event pair; ipsx_ips_call_elapsed
 *          (slot, &ms) reads it once the stream has been synchronised.  -1: no events.
 * The two hand-over events are the library's, one pair per device; the call enqueues under a per-device lock, so calls
 * from several threads (on streams of their own) do not mix their hand-overs.                                          */
typedef struct ipsx_ips_call {
    int b; int64_t n; int m, i, h, n_token;
    float* logits; int64_t* mem_idx; int32_t* words; int64_t words_total;
    int loops; void* scan_workspace; size_t scan_workspace_bytes;
    const ipsx_trunk* trunk; const float* pos; int quad_pulls;
    const ipsx_conv* lin; float ln_eps; int short_first;
    const void* x; float* emb; const float* v_packed; int r; int workgroups;
    const void* src; int64_t src_row_bytes, src_bstride_rows;
    const void* pos_table; int64_t pos_row_bytes, pos_bstride_rows;
    void* mem_patch; void* mem_pos; int64_t* mem_idx_out; int32_t* status_host;
    int timing_slot;
    void* stream; void* side_stream;
} ipsx_ips_call;
int ipsx_ips_call_run(const ipsx_ips_call* c);
int ipsx_ips_call_elapsed(int slot, float* ms);

/* 3.06: a permutation as the flat row index the row-indexed producers read through, ONE launch:
 * index[bi * n + j] = bi * n + clamp(order[bi * order_bstride + j], 0, n - 1);  order: (b or 1, n) int64 on the device,
 * order_bstride = n, or 0 for one permutation shared by every image; b * n <= 0x7FFFFFF0.  The clamp keeps whatever reads
 * through the index inside image bi's rows, whatever the caller handed in. */
int ipsx_order_index(const int64_t* order, int64_t order_bstride, int b, int64_t n, int32_t* index, void* stream);

/* 3.06: ipsx_ips_call_run for a selection on a permuted NUMBERING of the patches (a shuffle applied as addressing).
 * c->x and c->src are the UNSHUFFLED tensor; c->pos, c->pos_table, c->logits, c->emb, c->mem_idx are in shuffled
 * numbering.  The call enqueues what ipsx_ips_call_run enqueues, with ipsx_order_index behind the fill of the control
 * words - in front of the loop's launch: nothing sits between that and its producer's -, the producer reading through the
 * index (ipsx_trunk_stream_indexed | ipsx_projector_stream_indexed) and ipsx_ips_finish_indexed as the end of the call.
 * Refused before any launch: what ipsx_ips_call_run refuses, a null o, o->order or o->index, an order_bstride that is
 * neither 0 nor c->n. */
typedef struct ipsx_call_order {
    const int64_t* order; int64_t order_bstride;   /* (b or 1, n) int64 on the device, as ipsx_ips_finish_indexed takes it */
    int32_t* index;                                /* workspace, b * n int32 on the device: filled by the call */
} ipsx_call_order;
int ipsx_ips_call_run_ordered(const ipsx_ips_call* c, const ipsx_call_order* o);

/* --------------------------------------------------------------- aggregation
 * Replaces Transformer.forward (transformer.py:85-109,122-132,150-152) and the
 * task heads (ips_net.py:72-81,157-166) in eval / no-grad mode.               */
typedef struct ipsx_transf {
    int n_token, h, d, dk, dv, d_inner;
    const float *q, *wq, *wk, *wv, *fc;          /* (T,D) (HDk,D) (HDk,D) (HDv,D) (D,HDv) */
    const float *ln1_g, *ln1_b;                  /* LayerNorm after attention, eps 1e-6   */
    const float *w1, *b1, *w2, *b2;              /* (Dinner,D) (Dinner) (D,Dinner) (D)    */
    const float *ln2_g, *ln2_b;
    float temperature, ln_eps;
} ipsx_transf;

size_t ipsx_aggregate_workspace_bytes(const ipsx_transf* t, int b, int m);
/* x (b,m,d) -> out (b,T,d) */
int ipsx_aggregate(const ipsx_transf* t, const float* x, int b, int m, float* out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The same with operands the caller keeps between calls (they depend on the parameters only): vq_packed = ipsx_fold_query
 * of (q, wq, wk), wv_packed = ipsx_pack_conv_weight(wv, h*dv, d, 1, 1); either may be NULL (then it is made here, in the
 * workspace, as ipsx_aggregate does).  Saves four small launches per call in an evaluation loop. */
int ipsx_aggregate_packed(const ipsx_transf* t, const float* vq_packed, const float* wv_packed, const float* x, int b,
                          int m, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* 3.06: ipsx_aggregate_packed on a zero-padded batch.  count (b int32, device): image k attends to its slots 0 .. count[k] - 1
 * only - the softmax of every head and token runs over those slots, the others have probability +0.0 and add nothing to the
 * context, and what they hold cannot reach `out`.  The values are read on the device and clamped into 1 .. m there (the
 * host cannot see them); count NULL is refused with IPSX_EINVAL.  The same launches over the same rows, the same refusals
 * and the same workspace (ipsx_aggregate_workspace_bytes) as ipsx_aggregate_packed; out[k] has the bits of
 * ipsx_aggregate_packed on the first count[k] rows of image k alone. */
int ipsx_aggregate_counted(const ipsx_transf* t, const float* vq_packed, const float* wv_packed, const float* x,
                           const int32_t* count, int b, int m, float* out, void* workspace, size_t workspace_bytes,
                           void* stream);
/* out[b][c] = act(w[c,:] . emb[b][token,:] + bias[c]); act 0 = softmax, 1 = sigmoid */
int ipsx_head(const float* emb, int b, int n_token, int d, int token,
              const float* w, const float* bias, int n_class, int act,
              float* out, void* stream);

/* ------------------------------------------------------- training step (with-grad forward, SURVEY 8 f N-b)
 * Training-mode BatchNorm2d of the ResNet trunk with its residual add and ReLU, forward and backward, on channels-last
 * activations x (rows, c), rows = patches * pixels.  Replaces, under net.train() with autograd
 * (training/iterative.py:158-163 -> ips_net.py:273), the bn / += identity / relu kernels of a torchvision BasicBlock:
 *   forward : y = [relu]( (x - mean_batch) * invstd_batch * gamma + beta [+ residual] ); running_mean / running_var are
 *             updated in place with `momentum` (unbiased variance), save_mean / save_invstd (c floats) go to backward;
 *   backward: g = dy masked by y > 0 (when relu); dbeta = sum g; dgamma = sum g * xhat;
 *             dx = gamma * invstd * (g - dbeta / rows - xhat * dgamma / rows); dresidual = g (when not NULL).
 * c / 4 must be a power of two <= 256 (ipsx_bn_train_supported); workspace: ipsx_bn_train_workspace_floats floats.
 * fp32 results to rounding of torch.nn.functional.batch_norm (another summation order), deterministic.
 * Alignment: x, residual, y, dy, dx, dresidual, gamma, beta, save_mean, save_invstd, dgamma, dbeta, partial and the workspace
 * at 16-byte addresses (whole float4, no scalar route; c % 4 == 0 keeps the rows there); running_mean, running_var and
 * shift are read and written one float per channel: any float address, e.g. a slice of a longer buffer.        */
int ipsx_bn_train_supported(int64_t rows, int c);
size_t ipsx_bn_train_workspace_floats(int64_t rows, int c);
int ipsx_bn_train_forward(const float* x, const float* residual, int64_t rows, int c, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                          int relu, float* y, float* save_mean, float* save_invstd, float* workspace, void* stream);
/* ipsx_bn_train_forward without its reduction pass: the per-slab partial sums come from the convolution that produced x
 * (ipsx_conv2d_lds_nhwc_stats), taken around `shift` (may alias running_mean: it is read before the update).  A channel
 * whose shift proves more than 2 standard deviations from the batch mean, or not finite, is summed again over x on the
 * device (fp64, deterministic): any shift gives statistics to float32 rounding, a near one gives them without that pass. */
int ipsx_bn_train_forward_partials(const float* x, const float* residual, int64_t rows, int c, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                   int relu, float* y, float* save_mean, float* save_invstd, const float* partial,
                                   int64_t slabs, const float* shift, void* stream);
int ipsx_bn_train_backward(const float* dy, const float* y, const float* x, int64_t rows, int c, const float* gamma,
                           const float* save_mean, const float* save_invstd, int relu, float* dx, float* dresidual,
                           float* dgamma, float* dbeta, float* workspace, void* stream);

/* The feature projector of the training step (architecture/ips_net.py:54-60 under net.train() with autograd: LayerNorm
 * without affine -> Linear -> BatchNorm1d -> ReLU; the features need no gradient).  x: (n, F) rows stored as dtype 0 =
 * float32, 1 = bfloat16, 2 = float16 (widened exactly in the operand load: the bits of the same values passed as float32);
 * stats: ipsx_projector_stats_typed of those rows (only |rstd| is used).  Both GEMMs run the RAW rows through the fp32
 * matrix cores, centred in registers: the normalised rows never exist.  F a multiple of 32, D a power of two 32 .. 1024
 * (ipsx_projector_train_supported).
 * ipsx_projector_train_forward: z (n, D) = |rstd| * ((x - mean) W^T) + b - lin: the 1x1 Linear (w_packed:
 * ipsx_pack_conv_weight, shift: its bias, alpha NULL), weight: the same (D, F) weights unpacked - and, off the accumulators,
 * partial[slab][0 | 1][D] = sum (z - shift), sum (z - shift)^2 per slab of 64 rows (ipsx_projector_train_slabs(n) of them),
 * shift (D floats, written by the call) = the column mean of the first min(n, 8) rows of z: what
 * ipsx_bn_train_forward_partials takes.
 * ipsx_projector_wgrad: dw (D, F) [+]= sum_r (dz[r, :] |rstd_r|)^T (x[r, :] - mean_r), db (D) [+]= sum_r dz[r, :]; the rows
 * are cut into chunks of ipsx_projector_wgrad_chunk_rows() rows whose partial blocks are added in chunk order - on top of
 * what dw / db hold when accumulate != 0.  One call takes at most ipsx_projector_wgrad_max_rows rows (activations below
 * 2 GiB; a multiple of the chunk): more rows go slice by slice with accumulate = 1 from the second on, which gives the bits
 * of one call whatever the slice (a multiple of the chunk).  workspace: ipsx_projector_wgrad_workspace_bytes(n, F, D). */
int ipsx_projector_train_supported(int f, int d);
int64_t ipsx_projector_train_slabs(int64_t n);
int ipsx_projector_train_forward(const ipsx_conv* lin, const float* weight, const void* x, int dtype, int64_t n,
                                 const float* stats, float* z, float* shift, float* partial, void* stream);
int64_t ipsx_projector_wgrad_chunk_rows(void);
int64_t ipsx_projector_wgrad_max_rows(int f, int d, int dtype);
size_t ipsx_projector_wgrad_workspace_bytes(int64_t n, int f, int d);
int ipsx_projector_wgrad(const void* x, int dtype, const float* dz, const float* stats, int64_t n, int f, int d, float* dw,
                         float* db, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The row-indexed forms (the masked encoder pass): packed row j of stats / z / partial / dz is computed from source row
 * index[j] of the (src_rows, F) tensor x; index holds n flat int32 row numbers, one outside [0, src_rows) is clamped into it
 * (the rule of ipsx_projector_stats_indexed, whose statistics these calls take).  Slabs (64 packed rows), chunks, k order and
 * every tree of additions are those of the packed rows: z, shift, partial, dw and db are the bits of the plain calls on the
 * gathered tensor x[index], and no source row outside index is read.  A weight-gradient slice takes the matching n entries
 * of index with the WHOLE source.  The kernels address the source with 32-bit buffer offsets: src_rows * F * element size
 * must stay below 2 GiB - 64 KiB, a larger source is refused (IPSX_EINVAL) - gather the rows and take the plain calls. */
int ipsx_projector_train_forward_indexed(const ipsx_conv* lin, const float* weight, const void* x, int dtype, const int32_t* index,
                                         int64_t src_rows, int64_t n, const float* stats, float* z, float* shift, float* partial,
                                         void* stream);
int ipsx_projector_wgrad_indexed(const void* x, int dtype, const int32_t* index, int64_t src_rows, const float* dz,
                                 const float* stats, int64_t n, int f, int d, float* dw, float* db, int accumulate, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* The cross-attention aggregator of the training step on folded queries (architecture/transformer.py:43-109 under
 * autograd).  x: (B, M, D) float32 embeddings; A: (R, D) the scaled query folded into k_w, R = H * n_token rows in the order
 * r = h * n_token + t (ipsx_fold_query's); keep: (B, R, M) attention-dropout factors (0 or 1 / (1 - p)) or NULL = ones.
 *   forward   L[b, m, r] = x[b, m, :] . A[r, :],  P[b, r, :] = softmax_m L (max-subtracted),  P' = P * keep,
 *             Z[b, r, :] = sum_m P'[b, r, m] x[b, m, :]                      -> Z (B, R, D), P (B, R, M)
 *   backward  dP' = dZ . x,  dL = P * (keep * dP' - dZ[b, r, :] . Z[b, r, :]),
 *             dx[b, m, :] = sum_r P' dZ[b, r, :] + dL A[r, :]  (dx NULL: not computed),  dA[r, :] = sum_b sum_m dL x[b, m, :]
 * All contractions run on the fp32 matrix cores; no tensor of B x M x H x D_k elements exists.  Sums over workgroups (Z, dA)
 * go through per-workgroup blocks in the workspace, added in ascending (b, row) order: the same bits every call, and an
 * image's Z, P and dx do not depend on the rest of the batch.  R 1 .. 32, D a multiple of 32 up to 1024
 * (ipsx_attn_pool_supported), any M >= 1, B <= 65535.  workspace: ipsx_attn_pool_workspace_bytes(B, M, R, D), either
 * direction.  No allocation, no host synchronisation (graph-capturable).  Alignment: x, A, dZ, Z, dx and dA at 16-byte
 * addresses (rows of D % 32 == 0 floats read and written as float4, no scalar route). */
int ipsx_attn_pool_supported(int R, int D);
size_t ipsx_attn_pool_workspace_bytes(int64_t B, int64_t M, int R, int D);
int ipsx_attn_pool_forward(const float* x, const float* A, const float* keep, int64_t B, int64_t M, int R, int D, float* Z,
                           float* P, void* workspace, size_t workspace_bytes, void* stream);
int ipsx_attn_pool_backward(const float* x, const float* A, const float* keep, const float* P, const float* Z, const float* dZ,
                            int64_t B, int64_t M, int R, int D, float* dx, float* dA, void* workspace, size_t workspace_bytes,
                            void* stream);
/* 3.06: the two calls above on a zero-padded batch.  count (B int32, device; clamped into 1 .. M on the device; NULL is
 * refused): the rows of image b are 0 .. count[b] - 1 where they are 0 .. M - 1 above, the row pitch of x, keep, P and dx
 * stays M.  P[b, r, m >= count[b]] is written +0.0 and dx[b, m >= count[b], :] is written 0; the rows of x beyond count[b]
 * are never read, so nothing they hold reaches Z, P, dx or dA.  Z[b], P[b, :, :count[b]] and dx[b, :count[b]] have the bits
 * of the unmasked calls on x[b, :count[b]] alone (up to the sign of a zero).  The same number of launches, the same
 * workspace and the same refusals as the unmasked calls. */
int ipsx_attn_pool_forward_counted(const float* x, const float* A, const float* keep, const int32_t* count, int64_t B, int64_t M,
                                   int R, int D, float* Z, float* P, void* workspace, size_t workspace_bytes, void* stream);
int ipsx_attn_pool_backward_counted(const float* x, const float* A, const float* keep, const int32_t* count, const float* P,
                                    const float* Z, const float* dZ, int64_t B, int64_t M, int R, int D, float* dx, float* dA,
                                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IPSX_H */
