/*
 * diffews_hip.h -- C ABI of libdiffews_hip.so, the MI355X (gfx950) kernel library behind the
 * DiffewS hot path.
 *
 * The reference (ga1i13o/DiffewS) has no native code: every op below replaces a PyTorch /
 * diffusers-0.25 / xformers library call made from the reference's Python hot path.  Each entry
 * point cites the reference call site(s) it stands in for (paths relative to the reference root;
 * U = diffews/models/unet_2d_condition.py, A = diffews/models/attention_processor.py,
 * P = diffews/marigold_pipeline_rgb_latent_noise.py).
 *
 * Conventions:
 *   - the caller owns every buffer; kernels never allocate, free or synchronise;
 *   - pointers are raw device pointers; activations are NHWC / [rows][channels] row-major with an
 *     explicit element stride per row, images and latents at the pipeline boundary are NCHW fp32;
 *   - launches are asynchronous on the hipStream_t passed in (graph-capturable);
 *   - return value: 0 on success, a negative DFW_E* code for a rejected argument, or a positive
 *     hipError_t from the launch; no C++ exception crosses the boundary;
 *   - no global mutable state and nothing read from the environment, with ONE explicit exception: the process-wide
 *     tuning record of dfw_configure() below (defaults = the measured-best plans; meant for sweeps and A/B runs).
 */
#ifndef DIFFEWS_HIP_H
#define DIFFEWS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dfw_stream_t; /* hipStream_t */

enum { DFW_BF16 = 0, DFW_F16 = 1 };                       /* storage dtype of activations/weights */
enum { DFW_OUT_T = 0, DFW_OUT_F32 = 1, DFW_OUT_NCHW_F32 = 2 };
enum { DFW_ACT_NONE = 0, DFW_ACT_SILU = 1, DFW_ACT_CLAMP1 = 2 /* clamp to [-1, 1]: decode_seg, P:903 */ };
enum {
  DFW_EINVAL = -1,   /* null pointer / non-positive size */
  DFW_ESHAPE = -2,   /* shape not supported by the kernel (alignment / multiple-of constraints) */
  DFW_ERANGE = -3,   /* tensor exceeds the 2 GiB buffer-descriptor range */
  DFW_EWORKSPACE = -4
};

int dfw_version(void);
const char* dfw_error_string(int code);

/* Process-wide kernel-plan switches.  Every field's 0 value is NOT special: pass a record obtained from
 * dfw_get_config() with the fields of interest changed.  dfw_configure(NULL) restores the defaults.  Call it before the
 * launches it should affect; it is not synchronised against concurrent launches from other threads. */
typedef struct {
  int32_t conv_patch;        /* conv_patch_kernel: 0 off, 1 the N = 128 conv3x3 layers only, 2 also the N % 256 == 0 ones; 3: conv_patch8_kernel
                                (64-channel K-tiles on the eight-phase schedule) for the N % 256 == 0 layers, 4: also its 256 x 128 tile for
                                the other N % 64 == 0 layers */
  int32_t big_kernels;       /* 1 (default) gemm_big_kernel where eligible; 0: gemm_kernel tiles only */
  int32_t big_bm, big_bn, big_bk;   /* != 0: force this gemm_big configuration where it fits (sweeps), e.g. 256, 128, 64 */
  int32_t gemm_bm, gemm_bn;  /* != 0: force this gemm_kernel tile (128x128, 128x64, 64x64) instead of the cost model */
  int32_t fsa_key_split;     /* 1 (default) split the bank readers' key range when a workspace is passed; 0 never */
  int32_t fsa_force_splits;  /* != 0: this split count for eligible launches (forward and dQ) */
  int32_t big_min_tiles;     /* gemm_big_kernel only for launches with at least this many tiles (default 192 of the 256 CUs) */
  int32_t k8;                /* gemm8_kernel (64-deep K-tiles, half-tile staging): 0 never; 1 where gemm_big's 256 x 256 tile was planned;
                                2 also its 256 x 128 tiles; 3 also 256 x 128 in place of gemm_big's 512 x 128 tile */
} dfw_config;
int dfw_configure(const dfw_config* cfg);
void dfw_get_config(dfw_config* out);

/* HOST function: number of memset nodes in a captured hipGraph_t (child graphs included), or a negative DFW_E* code;
 * *n_nodes (optional) receives the node count.  The pipeline-owned step graph (pipeline.run_episodes(captured=True))
 * must contain none: on ROCm 7.2 a small memset node replayed next to plain launches on the same stream was observed to
 * receive the next launch's kernel arguments, so the library zeroes scratch with kernels and the host asserts that no
 * torch.zeros / fill_ slipped into the captured step. */
int dfw_graph_memset_nodes(void* hip_graph, int32_t* n_nodes);

/*
 * Implicit-GEMM on MFMA:  C[m][n] = epi( sum_k A(m,k) * W[n][k] ).
 *   taps == 1: A is [M][lda] (a Linear layer / 1x1 conv on NHWC tokens):
 *              to_q/to_k/to_v/to_out (A:237-245, A:276), proj_in/proj_out, GEGLU proj, FF out,
 *              time_embedding / time_emb_proj (U:1015), conv_shortcut, VAE attention projections.
 *   taps == 9: A is the im2col view of an NHWC image [B][Hi][Wi][lda>=Cin], k = (ky*3+kx)*Cin + c:
 *              every conv3x3 of ResnetBlock2D / Downsample2D / Upsample2D / conv_out
 *              (U:1161-1171, U:1191, U:1226-1243, U:1249; VAE encoder/decoder P:852, P:902).
 *              `ups` fuses the nearest-2x upsample of Upsample2D into the load indexing.
 *   W is [N][K] row-major (K = taps*Cin), i.e. nn.Linear.weight, or conv weight permuted to
 *   [Cout][ky][kx][Cin].
 *   epi: + bias[n] + rowbias[m / rows_per_img][n] + residual[m][n], * out_scale, optional SiLU;
 *        geglu != 0: W rows are interleaved in 64-row groups (32 value rows, 32 gate rows) and
 *        C[m][j] = (a + bias_a) * gelu(g + bias_g)  (diffusers GEGLU), C has N/2 columns.
 *   batch > 1: independent GEMMs at strideA/strideW/strideC elements (VAE attention QK^T, PV).
 *   splitk > 1: K is split over `splitk` workgroups per tile; `workspace` must hold
 *               splitk*M*N floats (dfw_gemm_workspace_bytes).
 */
typedef struct {
  const void* A; const void* W; void* C;
  const float* bias; const float* rowbias; const void* residual;
  void* workspace; size_t workspace_bytes;
  int64_t a_elems, w_elems;           /* extent of A / W in elements (for bounds-checked loads) */
  int32_t M, N, K;
  int32_t lda, ldc, ldr;
  int32_t ld_rowbias;                 /* row stride of rowbias in floats (0 => N) */
  int32_t taps, Cin, Hi, Wi, Ho, Wo, stride, pad, ups;
  int32_t rows_per_img;
  float out_scale;
  int32_t act, geglu, out_mode, splitk;
  int32_t batch; int64_t strideA, strideW, strideC;
  int32_t dtype;
  /* Optional fused GroupNorm statistics of the OUTPUT (the next op's GroupNorm input): when
   * gn_partial != NULL the epilogue also writes per-(image, chunk, group) (sum, sum of squares)
   * of the stored values, gn_partial[img][chunk][group][2] floats, chunk < dfw_gemm_gn_chunks().
   * Only kernels/shapes for which dfw_gemm_gn_chunks() returns > 0 support it. */
  float* gn_partial; int32_t gn_groups;
  /* Optional: output columns n < colscale_n (a multiple of 64) are multiplied by `colscale` instead of
   * out_scale, in fp32 before the single rounding to the storage dtype.  The fused [Wq;Wk;Wv] projection
   * (A:237-245) uses it to hand the attention kernel q * (scale * log2 e): the softmax then needs no
   * multiply per score (dfw_fsa_args.q_prescaled). */
  float colscale; int32_t colscale_n;
  /* != 0: `residual` is fp32 [M][ldr floats] instead of the storage dtype.  With out_mode DFW_OUT_F32 this is
   * the fp32 residual stream (residual_dtype=torch.float32 of the Python engines): x + branch(x) of
   * ResnetBlock2D / BasicTransformerBlock / Transformer2DModel is summed and stored in fp32, so the stream
   * is never rounded to 16 bits; only MFMA operands are.  Needs N % 4 == 0 and ldr % 4 == 0. */
  int32_t residual_f32;
  /* Optional second copy of a conv3x3 weight in the BLOCKED layout [tap][Cin / 32][N][32] (element
   * ((tap * Cin/32 + c) * N + n) * 32 + k holds W[n][tap * Cin + 32 c + k]): one (tap, 32-channel chunk) W stage of the
   * patch conv kernel is then ONE contiguous N x 64-byte block, so every LDS-DMA wave-instruction fetches eight whole
   * 128-byte lines instead of sixteen half lines at a row stride of K elements.  Used by the kernels that stage W per
   * (tap, chunk) -- conv_patch_kernel; ignored by the others, which read `W`.  NULL: everything reads `W`. */
  const void* W_blocked;
} dfw_gemm_args;

int dfw_gemm(const dfw_gemm_args* a, dfw_stream_t stream);
size_t dfw_gemm_workspace_bytes(const dfw_gemm_args* a);
/* Which kernel instantiation dfw_gemm would launch for these arguments, e.g.
 * "gemm_kernel<bf16,128,128,conv>" (used by bench.py to attribute time per kernel). */
int dfw_gemm_kernel_name(const dfw_gemm_args* a, char* buf, size_t n);
/* Chunks per image of the fused GroupNorm partial sums this call would emit for gn_groups groups
 * (0: unsupported for this shape / kernel; run dfw_groupnorm's own statistics pass instead). */
int32_t dfw_gemm_gn_chunks(const dfw_gemm_args* a);

/*
 * Upsample2D's nearest-2x + conv3x3 (U:1243; VAE decoder P:902) as four 2x2 convs on the LOW-resolution input
 * (version >= 111).  Under a 3x3 window an upsampled pixel has only four distinct source pixels, so for output parity
 * (py, px) = (Y & 1, X & 1) the nine taps fold onto a 2x2 window: tap (ty, tx) in {0,1}^2 reads source pixel
 * (y + ty - 1 + py, x + tx - 1 + px) with the SUM of the 3x3 weights that land there, ky in S(py, ty), kx in S(px, tx),
 * S(0,0) = {0}, S(0,1) = {1,2}, S(1,0) = {0,1}, S(1,1) = {2}.  The upsampled image's zero padding is the source image's
 * bounds check.  4 taps instead of 9: the same output on 2.25x fewer multiply-adds.
 *   x [B][Hi][Wi][ldx >= Cin] NHWC -> y [B][2 Hi][2 Wi][ldy >= Cout] NHWC, both the storage dtype; y = fold + bias.
 *   W is the folded pack [Cout][16 Cin], k = (((py*2 + px)*2 + ty)*2 + tx)*Cin + c, summed in fp32 and rounded once at
 *   load time (packing.fold_up2x).
 * Supported: Hi % 16 == 0, Wi % 16 == 0, Cin % 64 == 0, Cout % 64 == 0 (256-wide tiles when Cout % 256 == 0, else
 * 128-wide), ldx % 8 == 0, ldy % 8 == 0, x / W / y 16-byte aligned; anything else is DFW_ESHAPE and belongs on
 * dfw_gemm with ups = 1.  Null pointers, non-positive sizes, extents smaller than the shape: DFW_EINVAL.
 * gn_partial / gn_groups: as dfw_gemm_args, [B][chunks][gn_groups][2] floats with chunks from the query below; passing
 * gn_partial for a group count the query answers 0 for is DFW_ESHAPE.
 */
typedef struct {
  const void* x; const void* W; void* y; const float* bias;
  int64_t x_elems, w_elems;           /* extent of x / W in elements (for bounds-checked loads) */
  int32_t B, Hi, Wi, Cin, Cout;
  int32_t ldx, ldy;
  int32_t dtype;
  float* gn_partial; int32_t gn_groups;
} dfw_conv_up2x_args;

int dfw_conv_up2x(const dfw_conv_up2x_args* a, dfw_stream_t stream);
/* HOST-only plan queries, the same validation as the launch.  The name is e.g. "gemm8_kernel<bf16,256,256,64,up2x>";
 * for arguments the launch would reject the query returns that DFW_E* code and leaves the empty string in buf.  The chunk
 * count is 4 * (Hi/16) * (Wi/16) * wave rows of the tile (0: rejected arguments, or a group count whose groups do not
 * tile 64 channels -- run dfw_groupnorm's own statistics pass); gn_partial itself is not read by the query. */
int dfw_conv_up2x_kernel_name(const dfw_conv_up2x_args* a, char* buf, size_t n);
int32_t dfw_conv_up2x_gn_chunks(const dfw_conv_up2x_args* a);

/*
 * KV-fusion self-attention (the DiffewS-specific op): out = softmax(q [k_own ; k_bank]^T * scale) [v_own ; v_bank]
 * Replaces xformers.ops.memory_efficient_attention + the bank concat of MyXFormersAttnProcessor
 * (A:247-271).  q/k/v/out are [batch][tokens][heads*64] views with element row strides; the bank
 * holds `nshot` reference images per episode, ref image index = episode*nshot + shot (A:256-257,
 * evaluation_util/main_oss.py:103), each with n_bank tokens; keys are visited in the reference
 * order [own ; shot0 ; shot1 ; ...] without materialising the concat.  nshot == 0: plain
 * self-attention (bank-fill pass, A:251-252).  head_dim must be 64.
 * bank_shared: one support set for the whole batch -- the bank holds exactly nshot images and every
 * entry walks [own ; bank image 0 ; ... ; bank image nshot-1] (ref image index = shot).
 */
typedef struct {
  const void* q; const void* k; const void* v;
  const void* k_bank; const void* v_bank; void* out;
  int32_t batch, heads, n_q, n_kv, n_bank, nshot;
  int32_t ldq, ldk, ldv, ldkb, ldvb, ldo;      /* element strides between tokens */
  int64_t q_bs, k_bs, v_bs, kb_bs, vb_bs, o_bs; /* element strides between batch items */
  float scale;
  int32_t dtype;
  /* Lock-step launch over [support images ; query images] (one trunk pass for both UNet passes): the
   * first n_plain batch entries attend over their own keys only (the bank-fill pass, A:251-252); entry
   * b >= n_plain is episode b - n_plain and reads bank images (b - n_plain)*nshot + shot.  0 = every
   * entry reads the bank (the two-pass form). */
  int32_t n_plain;
  /* != 0: q already carries the factor scale * log2(e) (dfw_gemm_args.colscale on the projection that
   * produced it); `scale` is then ignored and the kernel exponentiates with exp2(q.k - m) directly. */
  int32_t q_prescaled;
  /* Optional (training): lse[batch][heads][n_q] fp32 = log2 of the row's sum of exp2(scaled score), so that
   * exp2(scaled score - lse) is the attention probability -- what dfw_fsa_attention_bwd recomputes P from. */
  float* lse;
  /* Optional scratch of dfw_fsa_workspace_bytes() (16-byte aligned): with it, a lock-step launch whose bank-reading images
   * walk many more keys than the plain ones (nshot >= 2) splits those images' key range over several workgroups and merges
   * the partial softmax results (same mathematics, fp32 partials, fixed order); without it the launch is unsplit. */
  void* workspace; size_t workspace_bytes;
  /* 0: the bank holds (batch - n_plain) * nshot images, entry b reads its own nshot of them (above).
   * 1: the bank holds nshot images and EVERY entry reads them (one prepared support set, many queries); the bank's
   *    extent is then nshot images.  Needs nshot > 0 and n_plain == 0; any other value is DFW_EINVAL. */
  int32_t bank_shared;
} dfw_fsa_args;

int dfw_fsa_attention(const dfw_fsa_args* a, dfw_stream_t stream);
size_t dfw_fsa_workspace_bytes(const dfw_fsa_args* a);
/* Which kernel dfw_fsa_attention would launch for these arguments (host-only plan query, like dfw_gemm_tn_kernel_name),
 * e.g. "fsa_ring_kernel<bf16,8,1,pre>+xcd+split3" ("scale": q not pre-scaled; +xcd: the grid is re-mapped onto the XCDs;
 * +splitS: S key splits of the bank-reading images merged by fsa_combine_kernel, only with the workspace passed;
 * +shared, always last: bank_shared launch). */
int dfw_fsa_kernel_name(const dfw_fsa_args* a, char* buf, size_t n);
/* Bank SETS: entries [j*group, (j+1)*group) read bank images j*nshot .. j*nshot+nshot-1 (key order [own ; shot 0 ; ...] as
 * ever) -- a class-major batch of N-way queries, `group` queries per class, against N prepared support sets stacked in one
 * bank.  Needs nshot > 0, n_plain == 0, bank_shared == 0, group >= 1, batch % group == 0 (else DFW_EINVAL, from both
 * functions, before any launch); the bank holds (batch/group)*nshot images and its descriptor extent is exactly that.
 * Same kernels, key-split plan and workspace as dfw_fsa_attention with the same fields; group == 1 is that launch.
 * The name is the unshared name + "+sets". */
int dfw_fsa_attention_sets(const dfw_fsa_args* a, int32_t group, dfw_stream_t stream);
int dfw_fsa_sets_kernel_name(const dfw_fsa_args* a, int32_t group, char* buf, size_t n);
/* RAGGED bank sets: a sets launch whose sets hold different numbers of images.  `shots` is a HOST array of nsets counts;
 * the stack holds the sets packed set-major, set j at images first[j] = shots[0] + ... + shots[j-1], and entries
 * [j*group, (j+1)*group) walk [own ; image first[j] ; ... ; image first[j]+shots[j]-1].  The (first, shots) table travels by
 * value in the kernel arguments: no device allocation, no copy, safe under stream capture (the graph keeps the values).
 * Needs what dfw_fsa_attention_sets needs, and shots != NULL, 1 <= nsets <= 64, nsets == batch / group, every count >= 1,
 * a->nshot == max(shots) (else DFW_EINVAL, from all three functions -- 0 bytes from the workspace query -- before any
 * launch); the bank's descriptor extent is exactly sum(shots) images.  Both the pre-scaled and the scaling form exist.
 * Key split: dfw_fsa_attention's rule on the longest set with the launch's summed work, clamped to 1 + min(shots) so
 * that every split instance owns a key segment; with all counts equal it is dfw_fsa_attention_sets' plan, kernel
 * arithmetic and result.  The workspace is a->workspace as ever, sized by dfw_fsa_ragged_workspace_bytes.
 * The name is the sets name with "+ragged" in place of "+sets". */
int dfw_fsa_attention_ragged(const dfw_fsa_args* a, const int32_t* shots, int32_t nsets, int32_t group, dfw_stream_t stream);
int dfw_fsa_ragged_kernel_name(const dfw_fsa_args* a, const int32_t* shots, int32_t nsets, int32_t group, char* buf, size_t n);
size_t dfw_fsa_ragged_workspace_bytes(const dfw_fsa_args* a, const int32_t* shots, int32_t nsets, int32_t group);
/* ROUTED queries (version >= 109): a query-only launch in which every entry reads a support set of its own choice out of
 * a stack of `nbank` bank images.  `table` is a DEVICE array int32 [batch][2], row e = (first_e, shots_e): entry e walks
 * [own ; image first_e ; ... ; image first_e + shots_e - 1].  The kernel reads its row when it RUNS, so a captured launch
 * follows whatever the table holds at each replay; `table_host` is a host mirror of the rows at the time of the call.
 * The plan (waves, grid, key split, workspace) is a function of a, nbank and min_shots only, never of the rows:
 * a->nshot is the LARGEST count a row may hold, min_shots the smallest; the key split is dfw_fsa_attention's rule on
 * batch * (1 + a->nshot) segments, clamped to 1 + min_shots so that no split instance is ever empty.
 * Needs n_plain == 0, bank_shared == 0, nshot > 0, nbank >= 1, 1 <= min_shots <= nshot (else DFW_EINVAL from all three
 * functions, 0 bytes from the workspace query); the launch also needs table and table_host non-NULL and every mirrored
 * row with first >= 0, min_shots <= shots <= nshot, first + shots <= nbank -- all checked before any launch.  Rows written
 * later (a replayed graph) are the caller's to keep inside those rules.  The bank descriptors claim exactly nbank
 * images and every bank read goes through them: a bad row gives wrong numbers, never a read outside the stack.
 * Per entry the arithmetic, key order and tile sequence of dfw_fsa_attention on that set with bank_shared = 1.
 * The name is the unshared name + "+routed". */
int dfw_fsa_attention_routed(const dfw_fsa_args* a, const int32_t* table, const int32_t* table_host, int32_t nbank,
                             int32_t min_shots, dfw_stream_t stream);
int dfw_fsa_routed_kernel_name(const dfw_fsa_args* a, int32_t nbank, int32_t min_shots, char* buf, size_t n);
size_t dfw_fsa_routed_workspace_bytes(const dfw_fsa_args* a, int32_t nbank, int32_t min_shots);

/*
 * Cross-attention over a short context (attn2 of BasicTransformerBlock; L = 2 prompt tokens at
 * inference P:591-600, 77 in training).  q/out [batch][n_q][heads*64]; k/v [batch][L][heads*64].
 */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  int32_t batch, heads, n_q, L;
  int32_t ldq, ldk, ldv, ldo;
  int64_t q_bs, k_bs, v_bs, o_bs;
  float scale;
  int32_t dtype;
} dfw_xattn_args;

int dfw_cross_attention(const dfw_xattn_args* a, dfw_stream_t stream);

/*
 * GroupNorm (+ optional SiLU) on NHWC: torch.nn.GroupNorm of ResnetBlock2D.norm1/norm2,
 * Transformer2DModel.norm, conv_norm_out (U:1247-1248), VAE attention group_norm.
 * Two launches: statistics (deterministic two-level reduction, fp32 partials, fp64 combine)
 * then apply.  `stats_ws` must hold dfw_groupnorm_workspace_bytes().
 */
typedef struct {
  const void* x; void* y; const float* gamma; const float* beta;
  void* stats_ws; size_t stats_ws_bytes;
  int32_t B, HW, C, groups, ldx, ldy;
  float eps;
  int32_t silu;
  int32_t dtype;
  /* Optional: partial sums already produced by the conv that wrote x (dfw_gemm_args.gn_partial),
   * [B][pre_chunks][groups][2] floats; the statistics pass over x is then skipped. */
  const float* pre_partial; int32_t pre_chunks;
  /* != 0: x is fp32 [B][HW][ldx floats] (the fp32 residual stream); y stays the storage dtype. */
  int32_t x_f32;
} dfw_groupnorm_args;

int dfw_groupnorm(const dfw_groupnorm_args* a, dfw_stream_t stream);
size_t dfw_groupnorm_workspace_bytes(const dfw_groupnorm_args* a);

/* LayerNorm over the last dim of [rows][C] (BasicTransformerBlock.norm1/2/3). */
typedef struct {
  const void* x; void* y; const float* gamma; const float* beta;
  int32_t rows, C, ldx, ldy;
  float eps;
  int32_t dtype;
  int32_t x_f32;   /* != 0: x is fp32 [rows][ldx floats] (fp32 residual stream); y stays the storage dtype */
} dfw_layernorm_args;

int dfw_layernorm(const dfw_layernorm_args* a, dfw_stream_t stream);

/*
 * Direct convolution for tiny channel counts on the pipeline boundary (NCHW fp32 in):
 * conv_in / conv_in_ref (U:1119-1121), VAE encoder.conv_in, decoder.conv_in, quant_conv,
 * post_quant_conv (P:853, P:901).  Cin <= 8.  W is [Cout][taps][Cin] fp32.
 * out_mode DFW_OUT_T: NHWC storage dtype (Cout % 8 == 0); DFW_OUT_F32: NHWC fp32 (Cout % 8 == 0; the fp32
 * residual stream starts at conv_in); DFW_OUT_NCHW_F32: NCHW fp32.
 * y = (conv(x * in_scale) + bias) * out_scale.
 */
typedef struct {
  const float* x; const float* W; const float* bias; void* y;
  int32_t B, Cin, H, Wd, Cout, taps, ldy;
  float in_scale, out_scale;
  int32_t out_mode;
  int32_t dtype;
  /* Optional fused GroupNorm statistics of the NHWC output (the first resnet's norm1 reads them through
   * dfw_groupnorm_args.pre_partial): gn_partial[B][chunks][gn_groups][2], chunks from
   * dfw_conv_small_gn_chunks() (0: not supported for this shape -- leave gn_partial NULL). */
  float* gn_partial; int32_t gn_groups;
  /* DFW_OUT_NCHW_F32 only: element stride between the images of y (0 => Cout*H*Wd).  Lets the conv write
   * its Cout channels into a channel slice of a wider NCHW tensor, e.g. the latent mean of the support
   * image and of its mask straight into the two halves of `cat([rgb_latent, mask_latent], dim=1)` (P:674). */
  int64_t y_bstride;
  /* Optional: the input batch spread over up to three buffers (each NCHW fp32, contiguous, 16-byte aligned):
   * images [0, b0) from x, [b0, b1) from x1, [b1, B) from x2.  x1 == NULL: all B images from x.  One launch
   * then covers the support images, the support masks and the query images of an episode batch
   * (P:649-651 encodes them in three calls) without first concatenating them. */
  const float* x1; const float* x2; int32_t b0, b1;
} dfw_conv_small_args;

int dfw_conv_small(const dfw_conv_small_args* a, dfw_stream_t stream);
int32_t dfw_conv_small_gn_chunks(const dfw_conv_small_args* a);
/* Which kernel dfw_conv_small would launch for these arguments (host-only plan query, like dfw_gemm_kernel_name; of x
 * only the alignment is read), with its grid: "conv_small8w_kernel<9> iters=4 grid=512x1" (8 pixels x 8 channels per
 * thread, iters pixel groups per thread), "conv_small4_kernel grid=3x40" or "conv_small_kernel grid=2x1". */
int dfw_conv_small_kernel_name(const dfw_conv_small_args* a, char* buf, size_t n);

/* Row softmax of fp32 scores -> storage dtype probabilities (VAE mid-block attention, 1 head of
 * dim 512: diffusers Attention.get_attention_scores with upcast_softmax).  y = softmax(x*scale). */
int dfw_softmax_rows(const float* x, void* y, int64_t rows, int32_t L, float scale, int32_t dtype,
                     dfw_stream_t stream);

/* Batched 2-D transpose of storage-dtype matrices: y[b][c][r] = x[b][r][c]. */
/* Softmax over L consecutive fp32 scores per (row, group): y[r][g*L + l] = softmax_l(x[r][g*L + l]),
 * g < groups; the remaining columns of the ld-wide row are zeroed.  The folded attn2 (prompt tokens are
 * constants of a checkpoint, P:585-601): scores = LN(x) G, probabilities here, out = P U + residual. */
int dfw_softmax_groups(const float* x, void* y, int64_t rows, int32_t ld, int32_t groups, int32_t L,
                       int32_t dtype, dfw_stream_t stream);
int dfw_transpose(const void* x, void* y, int32_t batch, int32_t R, int32_t C, int32_t dtype,
                  dfw_stream_t stream);

/* Channel concat of two NHWC tensors (torch.cat([h, skip], dim=1) in the up blocks, U:1226). */
int dfw_concat_channels(const void* a, const void* b, void* y, int64_t rows, int32_t Ca, int32_t Cb,
                        int32_t dtype, dfw_stream_t stream);

/* y[i] = (storage dtype) x[i], n % 8 == 0, 16-byte aligned: the 16-bit MFMA-operand copy of an fp32 residual-stream
 * tensor where a conv / Linear consumes the stream itself (conv_shortcut, Downsample2D / Upsample2D convs). */
int dfw_convert_f32(const float* x, void* y, int64_t n, int32_t dtype, dfw_stream_t stream);

/* Zero `bytes` bytes at p (both multiples of 16) with a kernel: buffers zeroed inside a captured step (gradient seeds of
 * the training step, T:1381: the support rows' zero gradient) must not become memset nodes -- see dfw_graph_memset_nodes. */
int dfw_zero(void* p, int64_t bytes, dfw_stream_t stream);

/* hi[i] = (storage dtype) x[i], lo[i] = (storage dtype)(x[i] - hi[i]): the two-operand form of an fp32 tensor (hi + lo = x
 * to ~2^-22 relative in fp16).  Where the fp32 residual stream itself is a conv / Linear operand (ResnetBlock2D.conv_shortcut,
 * Downsample2D / Upsample2D), the GEMM runs on hi, then on lo with the first result as its fp32 residual. */
int dfw_split_f32(const float* x, void* hi, void* lo, int64_t n, int32_t dtype, dfw_stream_t stream);

/* Sinusoidal timestep embedding, flip_sin_to_cos, fp32 math (diffusers Timesteps, U:1008);
 * out [B][dim] in storage dtype. */
int dfw_timestep_embedding(const float* timesteps, void* out, int32_t B, int32_t dim,
                           int32_t flip_sin_to_cos, float freq_shift, int32_t dtype,
                           dfw_stream_t stream);

/*
 * Segmentation post-processing on device (P:790-795, P:534; evaluation_util/main_oss.py:128-137;
 * evaluation_util/common/evaluation.py:24-38): from decoder output x [B][3][H][W] fp32 (already
 * clipped to [-1,1]) produce seg_u8 = uint8(clip((x*0.5+0.5)*255, 0, 255)) [B][3][H][W],
 * and when `gt` is non-null the per-episode 2x2 intersection/union pixel counts of
 * pred = (mean_c(u8/255) > r_threshold * max(u8/255)) against gt [B][H][W] (uint8 0/1, 255 = ignore)
 * into counts [B][4] int64 = {inter0, inter1, union0, union1}.
 * scratch: B uint32 words (per-image max), zeroed by this call.
 */
int dfw_seg_postprocess(const float* x, uint8_t* seg_u8, const uint8_t* gt, int64_t* counts,
                        uint32_t* scratch, int32_t B, int32_t H, int32_t Wd, float r_threshold,
                        dfw_stream_t stream);
/* Same with the launcher's other two choices (evaluation_util/main_oss.py:128-135):
 *   r_threshold > 0: dynamic threshold r_threshold * max; batch_max == 0 takes the max per image (what the
 *     reference computes at --bsz 1, the only batch size its E:128 `to_tensor` accepts; results do not
 *     depend on how episodes are batched), batch_max != 0 takes it over the whole [B,3,H,W] tensor, as
 *     `pred_mask.max()` literally reads for B > 1;
 *   r_threshold <= 0: fixed `--threshold`: pred = mean_c(u8/255) > threshold (> 0 required with gt). */
int dfw_seg_postprocess_ex(const float* x, uint8_t* seg_u8, const uint8_t* gt, int64_t* counts,
                           uint32_t* scratch, int32_t B, int32_t H, int32_t Wd, float r_threshold,
                           float threshold, int32_t batch_max, dfw_stream_t stream);

/* N-way label fusion: seg_u8 [N][B][3][H][W] (N calls' worth of dfw_seg_postprocess_ex output, class-major) and the
 * per-image maxima mx [N][B] those calls left in their scratch -> labels uint8 [B][H][W].  Per pixel and class c,
 * score_c = ((u0/255.0f + u1/255.0f) + u2/255.0f) / 3.0f (the fp32 expressions of the binary prediction) and c is
 * foreground when score_c > thr_c, thr_c = (m/255.0f) * r_threshold when r_threshold > 0 (m: the maximum of class c,
 * image b, or over the B images of class c when batch_max), else the fixed `threshold`.  label = 0 when no class is
 * foreground, else 1 + c of the foreground class with the largest score (lowest c on a tie).
 * gt (optional; then counts is required): uint8 [B][H][W], 0..N, 255 = ignore, values in (N, 255) dropped as well ->
 * counts int64 [B][2][N+1], zeroed by this call: row 0 intersections (label == gt == l), row 1 unions
 * (pred_l + gt_l - inter_l).  With N == 1, counts[b] is dfw_seg_postprocess_ex's {inter0, inter1, union0, union1}.
 * 1 <= N <= 254, else DFW_EINVAL; mx may be NULL with the fixed threshold. */
int dfw_seg_labels(const uint8_t* seg_u8, const uint32_t* mx, const uint8_t* gt, uint8_t* labels, int64_t* counts,
                   int32_t N, int32_t B, int32_t H, int32_t Wd, float r_threshold, float threshold,
                   int32_t batch_max, dfw_stream_t stream);

/* Label fusion over CANDIDATE classes per query (version >= 110): dfw_seg_labels' rule per ENTRY instead of per class.
 * seg_u8 [E_cap][3][H][W] is entry-major: entry e is one (query, candidate class) pair, the entries of one query are
 * adjacent; mx [E_cap] are the per-entry maxima a gt-less dfw_seg_postprocess_ex leaves (NULL allowed with the fixed
 * threshold).  `tab` is a DEVICE array int32 [B + 1 + E_cap]: offsets off[0 .. B] (non-decreasing, off[0] = 0,
 * off[B] = E <= E_cap; query q owns entries [off[q], off[q+1]), an empty range gives labels 0), then lab[e], the label
 * byte written where entry e wins, 1..nlabels for e < E; entries e >= E are padding and never read.  The kernel reads
 * `tab` when it RUNS, so a captured launch follows whatever the table holds at each replay; `tab_host` is its host mirror
 * at the time of the call and is what the call validates.  What the kernel reads it clamps (0 <= lo <= hi <= E_cap,
 * hi - lo <= 254): a bad table written later gives wrong numbers, never a read outside seg_u8 / mx / tab.
 *   score_e = ((u0/255.0f + u1/255.0f) + u2/255.0f) / 3.0f; e is foreground when score_e > thr_e,
 *   thr_e = (mx[e]/255.0f) * r_threshold when r_threshold > 0, else the fixed `threshold` (there is no batch_max form);
 *   label = 0 with no foreground entry, else lab[e] of the foreground entry with the largest score, earliest e on a tie.
 * labels uint8 [B][H][W].  counts (optional; then gt is required) int64 [B][2][nlabels+1]: row 0 label == gt == l, row 1
 * pred_l + gt_l - inter_l, gt uint8 [B][H][W] as dfw_seg_labels takes it (0..nlabels, 255 = ignore, values in
 * (nlabels, 255) dropped); a gt label that is not among the query's candidates counts in that label's union, as a miss.
 * area (optional) int64 [E_cap][2]: per entry, pixels where e is foreground on its own and pixels where e won the label;
 * ignore pixels included, independent of gt, rows e >= E left 0.  counts and area are zeroed by this call (a library
 * kernel).  With off = (0, N, 2N, ...), lab[qN + c] = 1 + c and seg_u8 / mx permuted from class-major to query-major,
 * labels and counts are those of dfw_seg_labels(..., batch_max = 0), bit for bit.
 * DFW_EINVAL, all on the host before any launch: NULL seg_u8 / tab / tab_host / labels; B, H, Wd or E_cap < 1; nlabels
 * outside 1..254; counts without gt; r_threshold > 0 without mx; neither threshold > 0; offsets not starting at 0,
 * decreasing or ending above E_cap; a query with more than 254 entries; a lab[e] outside 1..nlabels for e < E.
 * DFW_ERANGE: B above 65535 (also E_cap above 2^24 or H * Wd above 2^30). */
int dfw_seg_labels_cand(const uint8_t* seg_u8, const uint32_t* mx, const int32_t* tab, const int32_t* tab_host,
                        const uint8_t* gt, uint8_t* labels, int64_t* counts, int64_t* area,
                        int32_t B, int32_t E_cap, int32_t nlabels, int32_t H, int32_t Wd,
                        float r_threshold, float threshold, dfw_stream_t stream);

/* AverageMeter.update on device (evaluation_util/common/logger.py:35-37): for every episode b,
 * inter_buf[k][class_id[b]] += counts[b][k], union_buf[k][class_id[b]] += counts[b][2+k], k = 0, 1.
 * Buffers are int64 [2][nclass] (exact, order-independent sums); class ids outside [0, nclass) are skipped. */
int dfw_meter_update(const int64_t* counts, const int64_t* class_id, int64_t* inter_buf, int64_t* union_buf,
                     int32_t B, int32_t nclass, dfw_stream_t stream);

/*
 * Episode input transform (evaluation_util/data/dataset.py:36-40: Resize((S,S)) on the PIL image,
 * ToTensor, Normalize([0.5],[0.5]); coco.py:36-46: nearest resize of the class mask;
 * main_oss.py:100: mask -> 3 channels, {0,1} -> {-1,+1}).  Bit-exact with Pillow's ImagingResample
 * (BILINEAR, 8 bits per channel: horizontal then vertical pass, uint8 intermediate, 22-bit fixed-point
 * weights) and ATen's `nearest`.  JPEG/PNG decoding stays with the caller.
 *
 * dfw_resample_ksize / dfw_resample_coeffs are HOST functions: Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc for one axis; bounds [out_size][2] = (first input index, tap count),
 * coeffs [out_size][ksize].  The caller copies them to the device next to the image bytes.
 *
 * dfw_image_to_tensor / dfw_mask_to_tensor are the ONE-ITEM forms: pointers as arguments, two launches per image, one per
 * mask.  dfw_inputs_to_tensor below runs the same stage bodies (one copy of the arithmetic, csrc/inputs.hip) over a whole
 * ragged batch in three launches; the Python package calls only that one.
 */
int32_t dfw_resample_ksize(int32_t in_size, int32_t out_size);
int dfw_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs);

typedef struct {
  const uint8_t* src;                 /* device, [H][W][3] RGB bytes */
  int32_t H, W, out_h, out_w;
  const int32_t* xbounds; const int32_t* xcoef; int32_t xk;   /* device, from dfw_resample_coeffs(W, out_w) */
  const int32_t* ybounds; const int32_t* ycoef; int32_t yk;   /* device, from dfw_resample_coeffs(H, out_h) */
  uint8_t* tmp;                       /* device scratch, [H][out_w][3] */
  float* dst;                         /* device, [3][out_h][out_w] fp32 */
  const float* lut;                   /* device, 256 floats: byte v after ToTensor + Normalize */
} dfw_image_args;

int dfw_image_to_tensor(const dfw_image_args* a, dfw_stream_t stream);
/* mask: device [H][W] class ids (elem_bytes 1 = uint8 PNG, 4 = int32); on = (id == class_value);
 * dst_pm1 [3][out_h][out_w] fp32 in (-1,+1) and/or dst_bin [out_h][out_w] uint8 in (0,1). */
int dfw_mask_to_tensor(const void* mask, int32_t elem_bytes, int32_t H, int32_t W, int32_t class_value,
                       int32_t out_h, int32_t out_w, float* dst_pm1, uint8_t* dst_bin, dfw_stream_t stream);

/*
 * Native-size masks and scores (the launcher's --use_original_imgsize, main_oss.py:128-155): the output-side counterpart
 * of the input transform.  The quantised prediction seg_u8 [B][3][Hs][Ws] is resized back to every query's own h x w as
 * `Image.fromarray(hwc).resize((w, h))` does (marigold_pipeline_rgb_latent_noise.py:539: Pillow's default filter,
 * BICUBIC, a = -0.5, support 2; bit-exact, planar = three single-channel resizes), thresholded with the maximum of the
 * RESIZED image (bicubic overshoots) and counted against a ground truth read in place at native size.
 *
 * dfw_resample_ksize_ex / dfw_resample_coeffs_ex: the HOST functions above for either filter; with DFW_FILTER_BILINEAR
 * they return exactly what dfw_resample_ksize / dfw_resample_coeffs return.  Unknown filter: 0 / DFW_EINVAL.
 */
enum { DFW_FILTER_BILINEAR = 0, DFW_FILTER_BICUBIC = 1 };
int32_t dfw_resample_ksize_ex(int32_t in_size, int32_t out_size, int32_t filter);
int dfw_resample_coeffs_ex(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, int32_t* coeffs);

/* One image of a ragged batch.  Every offset is in BYTES from the base pointer named; bounds / coefficients need 4-byte
 * alignment, an int32 ground truth too. */
typedef struct {
  int32_t h, w;                        /* native size */
  int32_t xk, yk;                      /* dfw_resample_ksize_ex(Ws, w, BICUBIC), (Hs, h, BICUBIC) */
  int64_t xb_off, xc_off;              /* from `weights`: x bounds [w][2], x coefficients [w][xk] (int32) */
  int64_t yb_off, yc_off;              /* from `weights`: y bounds [h][2], y coefficients [h][yk] (int32) */
  int64_t tmp_off;                     /* from `tmp`: horizontal intermediate [3][Hs][w] bytes */
  int64_t u8_off;                      /* from `out_u8` (or tmp + tmp_res_off without it): resized [3][h][w] bytes */
  int64_t pred_off;                    /* from `pred`: [h][w] bytes */
  int64_t gt_off;                      /* from `gt`: [h][w] elements of gt_elem bytes */
  int32_t gt_elem;                     /* 1 (uint8) or 4 (int32) */
  int32_t class_value;                 /* foreground where id == class_value (1 for a 0/1 mask) */
  int32_t ignore_value;                /* pixel dropped where id == ignore_value; -1: none (255: PASCAL's boundary) */
  int32_t reserved;
} dfw_native_item;

typedef struct {
  const uint8_t* seg_u8;               /* device, planar [B][3][Hs][Ws] */
  int32_t B, Hs, Ws;
  const void* items;                   /* device, dfw_native_item [B]: what the kernels read */
  const void* items_host;              /* host mirror of the same table: what this call validates */
  const uint8_t* weights; size_t weights_bytes;   /* device base of the bounds / coefficient offsets */
  const uint8_t* gt; size_t gt_bytes;             /* device base of the ground-truth offsets; required with counts */
  uint8_t* tmp; size_t tmp_bytes;                 /* device scratch */
  size_t tmp_res_off;                  /* without out_u8 the resized bytes are staged at tmp + tmp_res_off + u8_off */
  uint8_t* out_u8; size_t out_u8_bytes;           /* optional: packed planar [3][h_i][w_i] per image */
  uint8_t* pred; size_t pred_bytes;               /* optional: packed [h_i][w_i] bytes 0/1 */
  uint32_t* mx;                        /* optional, [B]: maximum of each resized image; required with pred / counts and
                                          r_threshold > 0.  Zeroed by this call. */
  int64_t* counts;                     /* optional, [B][4] = inter0, inter1, union0, union1 as dfw_seg_postprocess;
                                          zeroed by this call */
  float r_threshold, threshold;        /* as dfw_seg_postprocess_ex; m is the RESIZED image's maximum */
  int32_t batch_max;
} dfw_seg_native_args;

/* Launches, whatever B: zero (mx / counts, a library kernel), horizontal pass, vertical pass + maximum, and -- with pred
 * or counts -- threshold + count.  Grid z runs over images, x / y are sized for the largest image of the batch.
 * Validated on the host mirror before the first launch: null pointers / non-positive sizes / nothing to produce /
 * gt_elem not 1 or 4 -> DFW_EINVAL; a ksize that disagrees with dfw_resample_ksize_ex or a misaligned offset ->
 * DFW_ESHAPE; h, w, Hs, Ws or B above 65535 -> DFW_ERANGE; an offset whose extent leaves its buffer -> DFW_EWORKSPACE. */
int dfw_seg_native(const dfw_seg_native_args* a, dfw_stream_t stream);

/* N-way labels and counts at native size (version >= 106): dfw_seg_native's resize for the N classes of
 * pipeline.segment_classes, then dfw_seg_labels' rule on the RESIZED bytes.  The ragged batch is the same
 * dfw_native_item [B] table and weights; class c of image i uses item i, its horizontal intermediates at
 * tmp + c * tmp_cls_stride + tmp_off and its resized bytes at out_u8 (or tmp + tmp_res_off) + c * u8_cls_stride + u8_off.
 * The item's class_value is not read.
 *   score_c = ((u0/255.0f + u1/255.0f) + u2/255.0f) / 3.0f from the resized bytes; c is foreground when score_c > thr_c,
 *   thr_c = (m/255.0f) * r_threshold with m = mx[c][i] (batch_max: the maximum over class c's B images) when
 *   r_threshold > 0, else the fixed `threshold`; label = 0 when no class is foreground, else 1 + c of the foreground
 *   class with the largest score, lowest c on a tie.
 * Ground truth (with counts): read in place at native size from the item's gt_off, gt_elem 1 or 4.  A pixel whose id
 * equals the item's ignore_value (when >= 0) is dropped.  Without class_ids the id is the label and ids outside 0..N are
 * dropped (dfw_seg_labels' rule); with class_ids the label is 1 + the lowest c with class_ids[c] == id and every other id
 * is background 0.  counts [B][2][N+1]: row 0 label == gt == l, row 1 pred_l + gt_l - inter_l.
 *
 * Workspace: tmp_cls_stride >= max_i(tmp_off_i + 3 * Hs * w_i), u8_cls_stride >= max_i(u8_off_i + 3 * h_i * w_i);
 * with out_u8:    tmp_bytes >= (N - 1) * tmp_cls_stride + max_i(tmp_off_i + 3 * Hs * w_i),
 *                 out_u8_bytes >= (N - 1) * u8_cls_stride + max_i(u8_off_i + 3 * h_i * w_i);
 * without out_u8: the same with tmp_res_off in place of tmp_bytes and tmp_bytes - tmp_res_off in place of out_u8_bytes,
 *                 i.e. tmp_bytes = N * tmp_cls_stride + N * u8_cls_stride with tmp_res_off = N * tmp_cls_stride always fits.
 * The resized bytes of all classes are materialised either way: a plane's maximum is known only once it is complete. */
typedef struct {
  const uint8_t* seg_u8;               /* device, planar [N][B][3][Hs][Ws], class-major */
  int32_t N, B, Hs, Ws;
  const void* items;                   /* device, dfw_native_item [B]: what the kernels read */
  const void* items_host;              /* host mirror of the same table: what this call validates */
  const uint8_t* weights; size_t weights_bytes;   /* device base of the bounds / coefficient offsets */
  const uint8_t* gt; size_t gt_bytes;             /* device base of the ground-truth offsets; required with counts */
  uint8_t* tmp; size_t tmp_bytes;                 /* device scratch */
  size_t tmp_res_off;                  /* without out_u8 the resized bytes are staged from tmp + tmp_res_off */
  size_t tmp_cls_stride;               /* bytes between two classes' horizontal intermediates */
  size_t u8_cls_stride;                /* bytes between two classes' resized bytes */
  uint8_t* out_u8; size_t out_u8_bytes;           /* optional: per class, packed planar [3][h_i][w_i] per image */
  uint8_t* labels; size_t labels_bytes;           /* packed [h_i][w_i] bytes 0..N, at the items' pred_off */
  uint32_t* mx;                        /* optional, [N][B]: maximum of each resized (class, image); required with
                                          r_threshold > 0.  Zeroed by this call. */
  int64_t* counts;                     /* optional, [B][2][N+1]; zeroed by this call */
  const int32_t* class_ids;            /* optional, device int32 [N]: ground-truth id of class c */
  float r_threshold, threshold;        /* as dfw_seg_labels; m is the RESIZED plane's maximum */
  int32_t batch_max;
} dfw_seg_labels_native_args;

/* Four launches whatever N and B: zero (mx / counts, a library kernel), horizontal pass and vertical pass + maximum over
 * N * B planes-of-3 (grid z), label + count over B images.  Validated on the host mirror before the first launch, as
 * dfw_seg_native: null pointers / non-positive sizes / N outside 1..254 / counts without gt / r_threshold > 0 without mx /
 * neither threshold > 0 / gt_elem not 1 or 4 -> DFW_EINVAL; ksize mismatch or a misaligned offset -> DFW_ESHAPE; h, w,
 * Hs, Ws, B or N * B above 65535 -> DFW_ERANGE; an extent that leaves its buffer, or a class stride smaller than one
 * class plane's extent -> DFW_EWORKSPACE. */
int dfw_seg_labels_native(const dfw_seg_labels_native_args* a, dfw_stream_t stream);

/* Candidate classes per query at native size (version >= 112): dfw_seg_labels_native's resize for the ENTRIES of
 * dfw_seg_labels_cand, then dfw_seg_labels_cand's rule on the RESIZED bytes.  seg_u8 [E_cap][3][Hs][Ws] is entry-major
 * and `tab` / `tab_host` are the same int32 [B + 1 + E_cap] table and host mirror as dfw_seg_labels_cand takes: offsets
 * off[0 .. B], then lab[e]; entries e >= E = off[B] are padding and never read.  The ragged batch is the same
 * dfw_native_item [B] table, weights and in-place ground truth as dfw_seg_labels_native: entry e of query q uses item q
 * (its class_value is not read).  Position k = e - off[q] in the query's list plays the part class c plays there: the
 * horizontal intermediates of entry e lie at tmp + k * tmp_cls_stride + tmp_off and its resized bytes at out_u8 (or
 * tmp + tmp_res_off) + k * u8_cls_stride + u8_off, so the workspace is K strides with K the LONGEST list, not E_cap:
 *   tmp_cls_stride >= max_i(tmp_off_i + 3 * Hs * w_i), u8_cls_stride >= max_i(u8_off_i + 3 * h_i * w_i), and
 *   (K - 1) * stride + that extent inside tmp (tmp_res_off without out_u8) / inside out_u8 (tmp_bytes - tmp_res_off).
 *   score_e = ((u0/255.0f + u1/255.0f) + u2/255.0f) / 3.0f from the resized bytes; e is foreground when score_e > thr_e,
 *   thr_e = (mx[e]/255.0f) * r_threshold when r_threshold > 0, else the fixed `threshold` (there is no batch_max form);
 *   label = 0 with no foreground entry, else lab[e] of the foreground entry with the largest score, earliest e on a tie;
 *   a query with no entries gets labels 0.
 * Ground truth (with counts): read in place at native size, gt_elem 1 or 4; a pixel equal to the item's ignore_value (when
 * >= 0) is dropped.  The id of every other pixel becomes a label in one of three ways:
 *   neither table   the id is the label; ids outside 0..nlabels are dropped;
 *   class_ids       device int32 [nlabels] (labels are 1 + set index): 1 + the lowest c with class_ids[c] == id, every
 *                   other id background -- a class that is not among the query's candidates still counts in its own
 *                   label's union, as a miss, as in dfw_seg_labels_cand;
 *   entry_ids       device int32 [E_cap] (labels are local to the query): lab[e] of the earliest entry e OF THIS QUERY with
 *                   entry_ids[e] == id, every other id background -- local labels have no bin for a class the query did
 *                   not name, so such a pixel is background (a false positive where it is labelled, never a miss).
 * counts [B][2][nlabels+1]: row 0 label == gt == l, row 1 pred_l + gt_l - inter_l.  area [E_cap][2]: per entry, pixels of
 * the RESIZED image where e is foreground on its own and where e won the label; ignore pixels included, rows e >= E 0.
 * The kernels read `tab` when they run and clamp what they read (0 <= lo <= hi <= E_cap, hi - lo <= min(254, K), the
 * query of an entry inside 0 .. B-1, its position inside 0 .. K-1 with K from the host mirror): a table rewritten after
 * the call gives wrong numbers, never an access outside the buffers. */
typedef struct {
  const uint8_t* seg_u8;               /* device, planar [E_cap][3][Hs][Ws], entry-major */
  int32_t B, E_cap, nlabels, Hs, Ws;
  const int32_t* tab;                  /* device, int32 [B + 1 + E_cap]: what the kernels read */
  const int32_t* tab_host;             /* host mirror of the same table: what this call validates */
  const void* items;                   /* device, dfw_native_item [B]: what the kernels read */
  const void* items_host;              /* host mirror of the same table: what this call validates */
  const uint8_t* weights; size_t weights_bytes;   /* device base of the bounds / coefficient offsets */
  const uint8_t* gt; size_t gt_bytes;             /* device base of the ground-truth offsets; required with counts */
  uint8_t* tmp; size_t tmp_bytes;                 /* device scratch */
  size_t tmp_res_off;                  /* without out_u8 the resized bytes are staged from tmp + tmp_res_off */
  size_t tmp_cls_stride;               /* bytes between two list positions' horizontal intermediates */
  size_t u8_cls_stride;                /* bytes between two list positions' resized bytes */
  uint8_t* out_u8; size_t out_u8_bytes;           /* optional: per list position, packed planar [3][h_i][w_i] per query */
  uint8_t* labels; size_t labels_bytes;           /* packed [h_i][w_i] label bytes, at the items' pred_off */
  uint32_t* mx;                        /* optional, [E_cap]: maximum of each entry's resized planes; required with
                                          r_threshold > 0.  Zeroed by this call. */
  int64_t* counts;                     /* optional, [B][2][nlabels+1]; zeroed by this call */
  int64_t* area;                       /* optional, [E_cap][2]; zeroed by this call */
  const int32_t* class_ids;            /* optional, device int32 [nlabels]: ground-truth id of label 1 + c */
  const int32_t* entry_ids;            /* optional, device int32 [E_cap]: ground-truth id of entry e's class */
  float r_threshold, threshold;        /* as dfw_seg_labels_cand; the maximum is the RESIZED planes' */
} dfw_seg_labels_cand_native_args;

/* Four launches whatever B and E: zero (mx / counts / area, a library kernel), horizontal pass and vertical pass + maximum
 * over the E planes-of-3 (grid z = E from the host mirror), label + count + area over the B queries.  Everything is
 * validated on the host before the first launch, with dfw_seg_labels_native's and dfw_seg_labels_cand's codes: null
 * pointers / sizes < 1 / nlabels outside 1..254 / counts without gt / class_ids together with entry_ids / r_threshold > 0
 * without mx / neither threshold > 0 / a bad table (offsets not from 0, decreasing, above E_cap, more than 254 entries a
 * query, lab[e] outside 1..nlabels for e < E) / h or w < 1 / gt_elem not 1 or 4 -> DFW_EINVAL; ksize mismatch or a
 * misaligned offset -> DFW_ESHAPE; h, w, Hs, Ws or B above 65535, E_cap above 2^24, E above 65535 -> DFW_ERANGE; an extent
 * that leaves its buffer, a stride smaller than one position's extent, or (K - 1) * stride + extent outside its buffer ->
 * DFW_EWORKSPACE. */
int dfw_seg_labels_cand_native(const dfw_seg_labels_cand_native_args* a, dfw_stream_t stream);

/*
 * Input transform of a whole ragged batch (version >= 107): dfw_image_to_tensor for n_img RGB images and
 * dfw_mask_to_tensor for n_mask class-id maps of assorted sizes, all going to one out_h x out_w, driven by two
 * device-resident tables.  The same device code computes both: Pillow's 8-bit two-pass BILINEAR resize (uint8 intermediate
 * [H][out_w][3], weights from dfw_resample_coeffs, the caller's 256-entry lut) and ATen's nearest rule
 * (on = id == class_value, index min((int)floorf((float)o * scale), size - 1), scale = (float)in / out in float).
 * Every offset is in BYTES from the base pointer named; bounds, coefficients, int32 masks and float destinations need
 * 4-byte alignment.
 */
typedef struct {
  int32_t H, W;                        /* size of the image */
  int32_t xk, yk;                      /* dfw_resample_ksize(W, out_w), (H, out_h) */
  int64_t src_off;                     /* from `staged`: [H][W][3] RGB bytes */
  int64_t xb_off, xc_off;              /* from `staged`: x bounds [out_w][2], x coefficients [out_w][xk] (int32) */
  int64_t yb_off, yc_off;              /* from `staged`: y bounds [out_h][2], y coefficients [out_h][yk] (int32) */
  int64_t tmp_off;                     /* from `tmp`: horizontal intermediate [H][out_w][3] bytes */
  int64_t dst_off;                     /* from `dst`: planar fp32 [3][out_h][out_w] */
} dfw_input_image_item;

typedef struct {
  int32_t H, W;                        /* size of the class-id map */
  int32_t elem;                        /* bytes per id: 1 (uint8) or 4 (int32) */
  int32_t class_value;                 /* on where id == class_value */
  int64_t src_off;                     /* from `staged`: [H][W] ids */
  int64_t pm1_off;                     /* from `pm1`: fp32 [3][out_h][out_w] in (-1, +1); -1 = none */
  int64_t bin_off;                     /* from `bin`: uint8 [out_h][out_w] in (0, 1); -1 = none */
} dfw_input_mask_item;

typedef struct {
  const void* image_items;             /* device, dfw_input_image_item [n_img]: what the kernels read */
  const void* image_items_host;        /* host mirror of the same table: what this call validates */
  int32_t n_img;
  const void* mask_items;              /* device, dfw_input_mask_item [n_mask] */
  const void* mask_items_host;         /* host mirror */
  int32_t n_mask;
  int32_t out_h, out_w;
  const uint8_t* staged; size_t staged_bytes;     /* device base of image bytes, weights and mask ids */
  uint8_t* tmp; size_t tmp_bytes;                 /* device scratch of the horizontal intermediates (images only) */
  float* dst; size_t dst_bytes;                   /* device base of the image outputs */
  float* pm1; size_t pm1_bytes;                   /* device base of the +-1 mask outputs; may be null when no item uses it */
  uint8_t* bin; size_t bin_bytes;                 /* device base of the 0/1 mask outputs; may be null when no item uses it */
  const float* lut;                    /* device, 256 floats: byte v after ToTensor + Normalize (images only) */
} dfw_inputs_args;

/* Three launches whatever the batch: horizontal pass and vertical pass + table lookup over all images (grid z = image,
 * x / y sized for the largest one; skipped when n_img == 0), one over all masks (grid z = mask; skipped when
 * n_mask == 0).  No memset node.  Validated on the host mirrors before the first launch: null pointers / non-positive
 * sizes / nothing to do / elem not 1 or 4 / a mask with neither destination -> DFW_EINVAL; a ksize that disagrees with
 * dfw_resample_ksize or a misaligned offset -> DFW_ESHAPE; H, out_h, n_img or n_mask above 65535 -> DFW_ERANGE; an
 * extent that leaves its buffer -> DFW_EWORKSPACE.  Regions of different items must not overlap (not checked). */
int dfw_inputs_to_tensor(const dfw_inputs_args* a, dfw_stream_t stream);

/*
 * Tiled segmentation (version >= 108): an image larger than the processing size is covered with overlapping
 * tile_h x tile_w windows, each window is one query of the existing routes, and the windows' quantised masks are blended
 * back into one image that is thresholded ONCE (its maximum is the merged image's, not a window's).
 *
 * The window plan is a plain struct the host fills; both entry points read it from HOST memory, validate it and hand it
 * BY VALUE to their kernels (no device allocation, no copy; a capture keeps the values).  Per axis: n origins in
 * 1..DFW_TILE_MAX_ORIGINS, strictly ascending, the first 0, the last = image - tile, neighbours at most a tile apart (no
 * pixel uncovered, no padding).  Windows are numbered row-major, t = iy * nx + ix, T = ny * nx.  The blend weight of pixel
 * (dy, dx) of a window is min(dy + 1, tile_h - dy, ramp) * min(dx + 1, tile_w - dx, ramp), 1 <= ramp <=
 * max(1, min(tile_h, tile_w) / 2); ramp = 1 is the plain mean.
 */
enum { DFW_TILE_MAX_ORIGINS = 64 };
typedef struct {
  int32_t img_h, img_w;                /* size of the image */
  int32_t tile_h, tile_w;              /* size of a window: the processing size */
  int32_t ny, nx;                      /* windows per axis */
  int32_t ramp;
  int32_t ys[64], xs[64];              /* first row / column of the windows of each axis; entries beyond ny / nx unused */
} dfw_tile_plan;

/* Windows first .. first + count - 1 of the staged image img (device, uint8 [img_h][img_w][3]) -> out (device, planar fp32
 * [count][3][tile_h][tile_w]) through lut (device, 256 floats: byte v after ToTensor + Normalize, as dfw_inputs_args.lut).
 * One launch.  A window is bit for bit what the input transform returns for the same crop at the same size. */
int dfw_tiles_cut(const dfw_tile_plan* plan, const uint8_t* img, const float* lut, float* out, int32_t first,
                  int32_t count, dfw_stream_t stream);

/* win (device, uint8 [N][T][3][tile_h][tile_w]: the seg_u8 of every window and class) -> out (device, uint8
 * [N][3][img_h][img_w]) and mx (device, [N]: the maximum byte of each class' merged image).  Per output byte, over the
 * windows that cover it, A = sum w * u and W = sum w in integers and the byte is (2 A + W) / (2 W) (round half up); a
 * gather without float operations or atomics on the image, so the result depends on no order; one window is the
 * identity.  Two launches: mx zeroed by a library kernel (no memset node), then the merge with one atomicMax per
 * workgroup.  out viewed as [N][1][3][img_h][img_w] and mx are what dfw_seg_labels takes with B = 1.
 *
 * Both validate on the host before the first launch: a null pointer, a plan that breaks a rule above, first / count
 * outside 0..T, N outside 1..254 -> DFW_EINVAL; img_h above 65535 (merge), or a plan whose sums are not proven to fit 32
 * bits, 511 * (most windows over a row) * (most windows over a column) * ramp^2 >= 2^32 (merge) -> DFW_ERANGE. */
int dfw_tiles_merge(const dfw_tile_plan* plan, const uint8_t* win, int32_t N, uint8_t* out, uint32_t* mx,
                    dfw_stream_t stream);

/* Candidate classes per WINDOW, merged sparsely (version >= 113): dfw_tiles_merge + dfw_seg_labels(B = 1, batch_max = 0)
 * on a window buffer [N][T][3][tile_h][tile_w] in which only the listed (window, class) pairs hold a mask and every other
 * pair is zero -- bit for bit, without that buffer and without the merged [N][3][img_h][img_w] image.
 *
 *   ent       device, uint8 [E_cap][3][tile_h][tile_w]: entry-major, the entries of one window adjacent, in ascending class;
 *             may be null only when the table lists no entry
 *   tab       device, int32 [T + 1 + E_cap]: offsets off[0..T] (window t owns entries [off[t], off[t + 1]), off[0] = 0,
 *             off[T] = E <= E_cap, E = 0 allowed, E_cap >= 1), then the class cls[e] in 0..N-1 of every entry, strictly
 *             ascending within a window.  The kernels read it when they RUN and clamp what they read (offsets into
 *             0..E_cap, classes into 0..N-1): a table overwritten later gives wrong numbers, never a read outside ent / tab
 *             or a bin outside a histogram
 *   tab_host  its host mirror: what this call validates
 *   gt        optional, device uint8 [img_h][img_w] as dfw_seg_labels takes it (0..N; 255 and anything above N ignored)
 *   labels    device, uint8 [img_h][img_w]: 0, or 1 + the foreground class of the largest score, lowest class on a tie
 *   mx        device, [N]: the maximum byte of each class' (virtual) merged image over its 3 channels; 0 for a class no
 *             window lists, which is therefore never foreground
 *   counts    optional (needs gt), device int64 [2][N+1]: dfw_seg_labels' counts for B = 1
 *   area      optional, device int64 [N][2]: (pixels where the class is foreground on its own, pixels where it won the
 *             label), ignore pixels included
 *
 * Per pixel, channel and class c: A = sum w * u over the covering windows that list c, W = sum w over ALL covering windows
 * (dfw_tiles_merge's weights), byte = (2 A + W) / (2 W) in 32-bit integers -- a class ramps down to 0 toward a
 * neighbouring window that does not list it.  Score, threshold (r_threshold > 0: mx[c] / 255 * r_threshold, else the
 * fixed `threshold`) and tie rule are dfw_seg_labels' fp32 expressions on those bytes.  No float operation and no atomic
 * on the image: the result depends on no order.  Launches: one library kernel that zeroes mx / counts / area (no memset
 * node), the maximum pass (only with r_threshold > 0 and E > 0), the label pass.
 *
 * Validated on the host before the first launch: a null plan / tab / tab_host / labels / mx, ent null with E > 0, a plan
 * that breaks a rule above, N outside 1..254, E_cap < 1, counts without gt, neither threshold > 0, offsets that do not
 * start at 0, decrease or end above E_cap, a class outside 0..N-1, classes not strictly ascending within a window ->
 * DFW_EINVAL; dfw_tiles_merge's img_h limit and its 32-bit proof -> DFW_ERANGE. */
int dfw_tiles_labels_cand(const dfw_tile_plan* plan, const uint8_t* ent, const int32_t* tab, const int32_t* tab_host,
                          const uint8_t* gt, uint8_t* labels, uint32_t* mx, int64_t* counts, int64_t* area, int32_t E_cap,
                          int32_t N, float r_threshold, float threshold, dfw_stream_t stream);

/*
 * The buffers of the object stages -- dfw_seg_components, dfw_seg_holes, dfw_seg_rle, dfw_seg_match, dfw_seg_scores,
 * dfw_seg_boundary, dfw_seg_boundary_counts and dfw_seg_contours, everything from here to the end of dfw_seg_contours --
 * are judged by one rule (one piece of code, csrc/seg_args.h; version >= 122).  Every stage validates on the host before
 * its first launch, in this order: null pointers and scalars (DFW_EINVAL), sizes (DFW_EINVAL before DFW_ERANGE), the
 * workspace (DFW_EWORKSPACE: ws_bytes below the stage's query), then the buffers:
 *   overlap    DFW_EINVAL when a buffer the call WRITES -- every output, and the workspace, taken as the bytes the query
 *              returns and not as ws_bytes -- shares a byte with any other device buffer of the call.  Extents are the
 *              shapes documented at the struct, half-open: buffers that touch end to start are fine, so outputs and
 *              workspace may be carved back to back out of one allocation.  Two INPUTS may alias each other (gt ==
 *              labels, pids == gids, pred == gt).  An optional buffer takes part only when the call uses it
 *   alignment  only then DFW_ESHAPE when a buffer is off its alignment: 4 bytes for int32 tables and maps and for the
 *              workspace, 8 for int64 tables, none for byte maps, unless the stage says otherwise
 * An extent is only known to be the caller's once sizes and workspace have passed, hence the order.  Up to version 121
 * dfw_seg_components compared only filtered == labels, dfw_seg_rle only ids against its outputs and dfw_seg_match only
 * inputs against outputs; a call with two outputs on each other, or with the workspace on anything, was launched there
 * and returned garbage.  From 122 on all three refuse it like the other five, which refuse exactly what they did.
 */

/*
 * Connected components of a label map (version >= 114): the last stage behind every route that ends in `labels`.  Two
 * pixels belong to one component when they carry the same NON-ZERO byte and a 4- or 8-connected path of that byte joins
 * them; different bytes never merge.  A component whose area is below min_area is removed (0 and 1 keep everything).  The
 * kept components of an image are numbered 1..n_b in row-major order of their FIRST pixel, the smallest y * W + x;
 * numbering restarts for every image.  All integers: the result depends on no order of execution.
 *
 *   ids       0 for background and for removed components, else the component's number
 *   filtered  the label bytes with the removed components set to 0 (labels itself with min_area <= 1)
 *   n         per image (components kept, components before the filter)
 *   stats     row id - 1 of an image = {label byte, area, y0, x0, y1, x1 (the box, half-open), first pixel y * W + x, 0};
 *             rows from min(n_b, cap) on are zero.  ONLY stats truncates -- ids, filtered, n and counts are complete
 *             whatever cap is -- and the caller sees it as n[b][0] > cap
 *   counts    dfw_seg_labels' counting rule applied to the FILTERED byte: row 0 filtered == gt == l, row 1 pred_l + gt_l -
 *             inter_l; gt 0..nlabels, 255 and anything above nlabels dropped; a filtered byte above nlabels has no bin.
 *             With min_area <= 1 on labels that dfw_seg_labels made, these are that call's counts bit for bit
 *   ws        dfw_seg_components_workspace_bytes(B, H, W) bytes: 8 per pixel plus 8 per dfw_seg_components_tile() pixels of
 *             an image, rounded up.  The call writes every word it reads: the caller initialises nothing
 *
 * A fixed number of launches (8, or 7 for an image of one tile), chosen by the arguments and never by the image; no host
 * readback, no loop until convergence, no memset node (stats and counts are zeroed by a library kernel), no thread that
 * waits for another: the call can be captured and is correct at any residency.  Union-find with parent[i] <= i: tiles in
 * LDS, borders by global atomicMin, then a flatten pass after which a component's root is its first pixel.  Area and box
 * reach global memory as one atomic per (tile, tile-local component) and field, never one per pixel.
 *
 * Validated on the host before the first launch.  DFW_EINVAL: null labels / ids / n / ws; B, H or W < 1; connectivity not 4
 * or 8; min_area < 0; stats with cap < 1; counts without gt; gt with nlabels outside 1..254.  DFW_ERANGE: H or W above
 * 65535, H * W above 2^30, B above 65535 (also B * cap * 8 above 2^31 - 1 with stats).  Then the workspace and the buffers,
 * by the rule above: filtered on labels is one such overlap; gt counts only with counts.
 *
 * Components of equal (byte, key) (version >= 125): keys, appended to the struct.  With keys null the call is the one
 * above, launch for launch and byte for byte.  With keys, int32 [B][H][W], two neighbouring pixels join when their label
 * bytes are equal and non-zero AND their keys are equal.  Keys are compared for equality only: 0 and negative values are
 * keys like any other, and a pixel is an object pixel by its byte alone.  Numbering by first pixel, min_area, filtered,
 * stats (the label column is still the byte), n, counts, the number of launches and the workspace query are unchanged;
 * launches 1 and 2 (the tile pass, which keeps the keys of its pixels in 8 KB more of LDS, and the border merge) compare
 * pairs, everything behind them never looks at a label.  With keys all equal the outputs are those of the keyless call.
 * This is also how an int32 map is labelled at all: labels = (map != 0), keys = map.  keys is an input of the buffer rule,
 * aligned to 4: it may alias nothing the call writes.
 *
 * The nearest seed inside the object (version >= 125): map, seeds, nearest, dist, reach and passes, appended to the struct.
 * With all of them zero the call is the one above, launch for launch and byte for byte.  With seeds (int32 [B][H][W], any
 * non-zero value is a seed) the call is ANOTHER STAGE on the same entry point: it reads map (int32 [B][H][W], values
 * compared for equality only, 0 = background) and seeds, writes nearest, dist and the workspace, and looks at no other
 * field than B, H, W, ws, ws_bytes, reach (1..254) and passes (1..8) -- labels, ids, n and keys may be null, and none of
 * the launches above runs.  It stands here and not on dfw_seg_boundary, whose row and column passes it shares (the code is
 * in csrc/seg_boundary.hip), because that struct's last fields are pinned by its tests and a new launching entry point
 * needs a case in every launch-guard table.  objects.split_objects runs it and then this call with keys = nearest.  With
 * R = reach:
 *
 *   A CANDIDATE of a pixel p = (y, x) with v = map[p] != 0 is a position q = (y + dy, x + dx) with seeds[q] != 0, dy^2 +
 *   dx^2 <= R^2 and an L path from p to q that stays on v, the column first and then the row: map[y + t][x] == v for every
 *   t between 0 and dy, and map[y + dy][x + s] == v for every s between 0 and dx.
 *   One pass: nearest[p] = seeds[q] of the candidate with the smallest (dy^2 + dx^2, seeds[q]) -- the nearer one, and among
 *   equally near ones the smaller value as a signed int -- and 0 without a candidate.  dist[p] (uint16) = 0 on a seed
 *   pixel, else the winner's dy^2 + dx^2, and (R + 1)^2 without a candidate.  Background has nearest 0 and dist 0.
 *   passes = k repeats the pass k - 1 times with seeds := nearest, in place: a pixel that holds a value keeps it and its
 *   dist, and its walk is skipped, so every pass carries each label round one more bend and a label never changes.
 *
 * map [[5,5,5,5],[5,0,0,5]], seeds [[0,0,0,0],[9,0,0,3]], R = 3.  One pass: nearest [[9,0,0,3],[9,0,0,3]], dist
 * [[1,16,16,1],[0,0,0,0]] -- (0, 0) goes down one row to the 9; (0, 1) has no seed in its row and its column leaves the
 * value at once, so it has no candidate.  passes = 2: the second pass's seeds are that result, (0, 1) finds the 9 one to
 * its left and (0, 2) the 3 one to its right: nearest [[9,9,3,3],[9,0,0,3]], dist [[1,1,1,1],[0,0,0,0]].
 *
 * The two-pass form.  The row pass writes, per pixel, h = the distance along the row to the nearest seed inside the
 * pixel's run of equal value (0 on a seed, R + 1 for none within R) and lab = that seed's value, the smaller of the two
 * when left and right are equally near.  The column pass starts from (h(y, x)^2, lab(y, x)) and offers, for dy = 1, 2,
 * ... up and down while the rows exist and map[y + dy][x] == v, the pair (dy^2 + h(y + dy, x)^2, lab(y + dy, x)) when it
 * is within R^2; the smallest pair wins.  Sketch of the proof: every pair the walk offers belongs to a real candidate --
 * the walk has stayed on v down column x to row y + dy, and h, lab describe a seed of that row inside the run of (y + dy,
 * x), which is the row part of an L path.  And no candidate beats it: a candidate (dy, dx) lies in row y + dy, which the
 * walk reaches because the column holds v that far, inside the run of (y + dy, x); the row pass's seed of that run
 * position is no farther along than |dx|, and at the same |dx| no larger in value, so it dominates the candidate in both
 * parts of the key -- a farther seed of the same row only has a larger distance.  A row with dy^2 above the best so far
 * cannot win; one with dy^2 EQUAL to it still can, by a smaller value straight above or below, so the walk goes on while
 * dy^2 <= the best so far, at most R steps, with dy^2 + h^2 <= 2 * 254^2.
 *
 * Launches: 2 * passes, fixed by the argument -- a row pass of its own (the same window of positions with halo, the breaks'
 * scans and the same scans over seed positions; dfw_seg_boundary's, see there) and a column pass on the tile and the
 * four-pixels-a-thread rule of the Euclidean one (W % 4 == 0, map, nearest and ws aligned to 16, dist to 8).  The column pass reads labels from the
 * workspace only, never from nearest, which it writes: the row pass of pass k + 1 reads nearest after the column pass of
 * pass k has finished it, which is what makes the repeat in place safe.  No atomics, no memset node, no host readback,
 * no thread that waits for another; a lexicographic minimum depends on no order of execution.  Nothing is written outside
 * nearest, dist and ws.  The workspace is dfw_seg_nearest_workspace_bytes(B, H, W), 5 bytes a pixel; the other query and
 * its value do not change.
 *
 * Refusals of the stage, in the house order.  DFW_EINVAL: null map / nearest / dist / ws, reach outside 1..254, passes
 * outside 1..8, B, H or W < 1; DFW_ERANGE: the sizes, as above; DFW_EWORKSPACE against dfw_seg_nearest_workspace_bytes; then
 * the buffers: map and seeds are inputs aligned to 4, dist an output aligned to 2, nearest an output aligned to 4 that may
 * share no byte with map, seeds, dist or ws.  Without seeds, a non-null nearest is DFW_EINVAL (behind nlabels' rule, before
 * the sizes); map, dist, reach and passes are not looked at.
 */
typedef struct {
  const uint8_t* labels;   /* [B][H][W] contiguous; 0 = background, any other byte is a class; equal bytes connect */
  int32_t* ids;            /* out [B][H][W]: 0 = background or removed, else 1..n_b */
  uint8_t* filtered;       /* out, optional [B][H][W]: labels with removed components set to 0; must not alias labels */
  int32_t* n;              /* out [B][2]: (components kept, components before the filter) */
  int32_t* stats;          /* out, optional [B][cap][8]: label, area, y0, x0, y1, x1 (half-open), first pixel y*W+x, 0 */
  const uint8_t* gt;       /* optional [B][H][W], as dfw_seg_labels takes it */
  int64_t* counts;         /* optional [B][2][nlabels+1], needs gt: intersections / unions of the FILTERED labels */
  void* ws;
  size_t ws_bytes;
  int32_t B, H, W, connectivity, min_area, cap, nlabels;   /* connectivity 4 | 8; min_area >= 0 */
  const int32_t* keys;     /* optional [B][H][W] (version >= 125): neighbours join only when their keys are equal too */
  const int32_t* map;      /* the nearest-seed stage (seeds non-null): [B][H][W], read only */
  const int32_t* seeds;    /* [B][H][W] or null; non-null: the call is the nearest-seed stage, see above */
  int32_t* nearest;        /* out [B][H][W], with seeds only */
  void* dist;              /* out uint16 [B][H][W], with seeds only */
  int32_t reach, passes;   /* 1..254 and 1..8, with seeds only */
} dfw_seg_components_args;
int dfw_seg_components(const dfw_seg_components_args* a, dfw_stream_t stream);
size_t dfw_seg_components_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* the workspace of the nearest-seed stage (seeds non-null): 5 bytes a pixel -- the row pass's value (int32 [B * H * W],
 * rounded up to 16 bytes) and its distance (one byte a pixel, rounded up to 16) -- and 0 for sizes the call refuses;
 * monotone otherwise */
size_t dfw_seg_nearest_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* the tile of the LDS pass (rows, columns): the shapes at which the kernels change path, for tests and docs */
int dfw_seg_components_tile(int32_t* tile_h, int32_t* tile_w);
/* How often each loop of dfw_seg_components that carries a value from one round to the next would run for these
 * arguments (version >= 117; host only, launches nothing, like dfw_gemm_kernel_name): computed by the expressions the
 * launcher sizes its grids with, for tests and docs.  ws is only looked at for its alignment, which chooses the flatten
 * path.  Errors as dfw_seg_components gives them for the same B, H, W and ws. */
typedef struct {
  int32_t blocks;           /* scan blocks of dfw_seg_components_tile() pixels per image */
  int32_t merge;            /* grid-stride trips of the border-union kernel (0: one tile, no launch) */
  int32_t flatten;          /* grid-stride trips of the flatten kernel on the path it takes */
  int32_t flatten_vector;   /* 1: four pixels a thread (H * W a multiple of 4 and a 16-byte aligned area plane), else 0 */
  int32_t scan;             /* rounds of 256 block sums of the one-workgroup scan */
} dfw_seg_components_rounds_out;
int dfw_seg_components_rounds(int32_t B, int32_t H, int32_t W, const void* ws, dfw_seg_components_rounds_out* out);

/*
 * Filling the holes of labelled objects (version >= 120): the partner of min_area.  labels and ids are normally the
 * `filtered` and `ids` outputs of dfw_seg_components (any pair of maps is accepted).  All integers: the result is exact and
 * depends on no order of execution.
 *
 *   background     a pixel whose labels byte is 0; every other byte, 255 included, is not
 *   region         a connected component of background pixels under the DUAL connectivity hc: 4 when `connectivity` (that
 *                  of the objects, as dfw_seg_components takes it) is 8, and 8 when it is 4
 *   enclosed       no pixel of the region lies on the first or last row or on the first or last column; a map with H < 3
 *                  or W < 3 therefore has no enclosed region
 *   owner          the ids value of the pixel to the LEFT of the region's first pixel, the smallest y * W + x; for an
 *                  enclosed region that pixel exists and is not background
 *   border pixels  the non-background pixels in the hc-neighbourhood of any pixel of the region
 *   filled         enclosed, owner >= 1, every border pixel has ids == owner, and area <= max_area (>= 0; 0 fills nothing)
 *
 * NOT filled, on purpose: a region bordered by two objects, whether or not the two share a class (two 4-connected objects
 * of one class that touch diagonally included), and a hole with an island of another object inside it.  min_area removes
 * such islands first, so a second rule is not needed.
 *
 *   ids_out, labels_out  the inputs, except that every pixel of a filled region takes the owner's id and the owner's label
 *                  byte, the labels byte of the pixel to the left of the region's first pixel
 *   holes          per image (regions filled, regions enclosed)
 *   stats_out      optional, needs stats and cap >= 1: stats, except that in the rows of ids <= cap column 1 (area) grows
 *                  by the object's filled pixels and column 7 (0 so far) holds that number.  Label, box and first pixel
 *                  do not change: a hole lies inside its owner's box and behind its first pixel
 *   counts         optional, needs gt and nlabels: dfw_seg_components' counting rule applied to labels_out
 *   ws             dfw_seg_holes_workspace_bytes(B, H, W) bytes, 8 per pixel.  The call writes every word it reads: the
 *                  caller initialises nothing
 *
 * A fixed number of launches (6, or 5 for an image of one tile), chosen by the arguments and never by the image: the three
 * union-find passes of dfw_seg_components on the zero bytes (their grids are that call's, so dfw_seg_components_rounds
 * describes their trips), one pass over the frame pixels that also zeroes holes and counts and copies stats, one pass that
 * decides per region, one that writes the outputs.  No host readback, no memset or copy node, no thread that waits for
 * another: the call can be captured.  The filled pixels reach stats_out as one atomic per (tile, tile-local region) and
 * field, holes as one per tile and field, never one per pixel.
 *
 * Validated on the host before the first launch, in this order.  DFW_EINVAL: null args / labels / ids / ids_out /
 * labels_out / holes / ws; B, H or W < 1; connectivity not 4 or 8; max_area < 0; stats_out without stats or with cap < 1;
 * counts without gt; gt with nlabels outside 1..254.  DFW_ERANGE: H or W above 65535, H * W above 2^30, B above 65535 (also
 * B * cap * 8 above 2^31 - 1 with stats_out).  Then the workspace and the buffers, by the rule above: stats only counts
 * with stats_out.
 */
typedef struct {
  const uint8_t* labels;   /* [B][H][W] contiguous; 0 = background */
  const int32_t* ids;      /* [B][H][W] the object of every pixel, 0 = none */
  const int32_t* stats;    /* optional [B][cap][8], dfw_seg_components' stats: read only with stats_out */
  const uint8_t* gt;       /* optional [B][H][W], as dfw_seg_labels takes it */
  int32_t* ids_out;        /* out [B][H][W] */
  uint8_t* labels_out;     /* out [B][H][W] */
  int32_t* holes;          /* out [B][2]: (regions filled, regions enclosed) */
  int32_t* stats_out;      /* out, optional [B][cap][8], needs stats and cap >= 1 */
  int64_t* counts;         /* out, optional [B][2][nlabels+1], needs gt: intersections / unions of labels_out */
  void* ws;
  size_t ws_bytes;
  int32_t B, H, W, connectivity, max_area, cap, nlabels;   /* connectivity 4 | 8: the OBJECTS'; max_area >= 0 */
} dfw_seg_holes_args;
int dfw_seg_holes(const dfw_seg_holes_args* a, dfw_stream_t stream);
/* 0 for sizes dfw_seg_holes refuses (B, H or W < 1 or above 65535, H * W above 2^30) */
size_t dfw_seg_holes_workspace_bytes(int32_t B, int32_t H, int32_t W);

/*
 * Run-length encoding of labelled objects (version >= 115): the shape of every object of an id map, normally the one
 * dfw_seg_components wrote (any int32 map is accepted).  A pixel's position is q = y * W + x with order = 0 (rows) or
 * q = x * H + y with order = 1 (columns, COCO's order); its value v(q) is its id when 1 <= id <= cap and 0 otherwise (ids
 * above cap are not encoded, as stats does not list them; negative ids count as 0).  A run is a maximal interval
 * [s, s + l) of positions with one equal non-zero value.  Runs do NOT stop at the end of a row or column: this flattened
 * order is COCO's, so order = 1 maps onto an uncompressed COCO RLE one-to-one.  `found` is the number of runs of an image;
 * the first kept = min(found, max_runs) runs IN ASCENDING s are encoded, the rest dropped: found > kept tells the caller
 * that the encoding is incomplete.  All integers: the result depends on no order of execution.
 *
 *   runs      the encoded runs as (s, l), grouped by id ascending and ascending in s within an id; rows from kept on are
 *             not written
 *   run_off   object k's runs are rows run_off[k-1] .. run_off[k]; run_off[0] = 0, run_off[cap] = kept
 *   nruns     per image (kept, found)
 *   ws        dfw_seg_rle_workspace_bytes(..) bytes.  The call writes every word it reads: the caller initialises nothing
 *
 * Ids [[1,1,0],[2,1,1]], cap = 2: rows give runs (0,2) (4,2) | (3,1), run_off = [0,2,3]; columns read the values as
 * 1,2,1,1,0,1 and give (0,1) (2,2) (5,1) | (1,1), run_off = [0,3,4] -- object 1's COCO counts are [0,1,1,2,1,1].
 *
 * A fixed number of launches, 5 + order + 3 * (the bytes cap needs: 1 below 256, 2 below 65536, ..), chosen by the
 * arguments and never by the image; no host readback, no memset node (run_off is zeroed by a library kernel), no thread
 * that waits for another: every cross-workgroup prefix is a scan in a launch of its own, so the call can be captured and
 * is correct at any residency.  Starts are counted per block of positions, scanned, and compacted into (id, s, end)
 * records; a stable LSD radix sort on the id, one byte a pass, groups them, its in-chunk ranks taken in a fixed order (no
 * atomic decides a position).  Nothing is written outside runs[.., :kept], run_off, nruns and ws; ids is read only.
 *
 * Validated on the host before the first launch.  DFW_EINVAL: null args / ids / runs / run_off / nruns / ws; B, H, W, cap
 * or max_runs < 1; order not 0 or 1.  DFW_ERANGE: H or W above 65535, H * W above 2^30, B above 65535, B * max_runs * 2
 * or B * (cap + 1) above 2^31 - 1.  Then the workspace and the buffers, by the rule above; runs, rows of two int32, needs
 * 4-byte alignment only.
 */
typedef struct {
  const int32_t* ids;      /* [B][H][W] contiguous, read only */
  int32_t* runs;           /* out [B][max_runs][2]: (s, l); rows [kept, max_runs) are left as they were */
  int32_t* run_off;        /* out [B][cap + 1] */
  int32_t* nruns;          /* out [B][2]: (kept, found) */
  void* ws;
  size_t ws_bytes;
  int32_t B, H, W, cap, max_runs, order;   /* order 0 = rows, 1 = columns */
} dfw_seg_rle_args;
int dfw_seg_rle(const dfw_seg_rle_args* a, dfw_stream_t stream);
/* 0 for arguments dfw_seg_rle answers DFW_EINVAL for; monotone in every argument */
size_t dfw_seg_rle_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_runs, int32_t order);
/* positions one scan block covers, run records one sort chunk covers: the sizes at which the kernels change path, for
 * tests and docs */
int dfw_seg_rle_block(int32_t* pixels, int32_t* records);
/* How often each one-workgroup scan of dfw_seg_rle / dfw_seg_match would go round, 1024 words a round with the sum
 * carried into the next (version >= 117; host only, launches nothing): computed by the expressions the launchers use,
 * for tests and docs.  Errors: DFW_EINVAL for a null out, then the size errors of dfw_seg_rle / dfw_seg_match
 * themselves, in their order (DFW_EINVAL before DFW_ERANGE); pointers, workspace and overlap are not part of it. */
typedef struct {
  int32_t blocks;         /* scan blocks of `pixels` positions per image, position H * W included */
  int32_t block_scan;     /* the scan of the block sums: (kept, found) */
  int32_t passes;         /* digit passes of the sort, each with one table scan */
  int32_t table_scan;     /* the scan of the digit table, 256 words per chunk of `records` */
  int32_t offsets_scan;   /* the scan of run_off (cap + 1 words) or pair_off (capP + 2 words) */
  int32_t heads_scan;     /* dfw_seg_match only: the scan of the heads and lengths per chunk; 0 for dfw_seg_rle */
} dfw_seg_sort_rounds;
int dfw_seg_rle_rounds(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_runs, int32_t order,
                       dfw_seg_sort_rounds* out);

/*
 * Matching of predicted objects to ground-truth objects (version >= 116): the object-level score behind two id maps,
 * normally dfw_seg_components' ids of the prediction and of the ground truth (any int32 maps are accepted).  All integers:
 * the result depends on no order of execution.
 *
 *   p(q) = pid when 1 <= pid <= capP, else 0; g(q) likewise with capG.
 *   A pixel has w(q) = (p, g) unless it is skipped (skip[q] == 255); a skipped pixel has w(q) = (0, 0).
 *   Position is q = y * W + x.
 *   A RECORD is a maximal interval of positions with one equal w != (0, 0).  As in dfw_seg_rle, it does not stop at a
 *   row's end.
 *   key = p * (capG + 1) + g.
 *   A PAIR is a distinct key over the kept records; inter is the sum of the record lengths of that key.
 *   Pairs with g = 0 or p = 0 are kept.  Row sums are therefore areaP[p], the counted pixels of p; column sums are
 *   areaG[g].  Neither depends on stats, and both respect skip.
 *   union = areaP[p] + areaG[g] - inter.
 *   p and g (both > 0) MATCH when their classes are equal, the class is in 1..nlabels, and inter * den > num * union in
 *   64-bit integers.  The threshold is num / den with 1 <= num <= den <= 65535 and 2 * num >= den; the comparison is
 *   strictly greater.  Because ids partition the pixels, each object has at most one partner at any threshold >= 1/2, so
 *   no assignment problem arises.  An object's class is column 0 of its row of pstats / gstats (as dfw_seg_components
 *   writes them; nothing else is read), and 1 for every object of a side without a table.
 *   An object with area == 0 (all its pixels skipped, or its id above cap) is absent: neither FP nor FN.
 *
 *   pairs     (p, g, inter), ascending in (p, g); rows from `kept` on are not written
 *   pair_off  the rows of p are pair_off[p] .. pair_off[p + 1], for p = 0..capP; the last entry is the number of pairs kept
 *   area      areaP[0..capP], then areaG[0..capG]
 *   match     row p - 1 = (g, inter, union) of object p's partner; zeros without one
 *   gmatch    entry g - 1 = the partner p, or 0
 *   pq        per class (TP, FP, FN, S), S = the sum over the TPs of floor(inter * 2^32 / union) (inter <= 2^30: the
 *             product fits; the sum is an integer atomic, so it is order-free); row 0 stays zero
 *   n         per image (pairs kept, pairs found, records kept, records found)
 *   ws        dfw_seg_match_workspace_bytes(..) bytes.  The call writes every word it reads: the caller initialises nothing
 *
 * Truncation is deterministic and visible: of the records the first max_records in ascending start are kept, of the pairs
 * the first max_pairs in ascending key; every output is what the definition gives on the kept records and pairs, and the
 * caller sees n[0] < n[1] or n[2] < n[3] and knows the result is incomplete.
 *
 * pids = [[1,1,0],[2,1,1]], gids = [[1,1,1],[0,2,2]], caps 2 and 2, threshold 1/2: records (1,1)x2, (0,1)x1, (2,0)x1,
 * (1,2)x2; pairs (0,1,1), (1,1,2), (1,2,2), (2,0,1); pair_off = [0,1,3,4]; areaP = [1,4,1], areaG = [1,3,2]; IoU(1,1) =
 * 2/5 and IoU(1,2) = 2/4, which is not above 1/2: no match, pq[1] = (0, 2, 2, 0).
 *
 * A fixed number of launches, 14 + 3 * (the bytes (capP + 1) * (capG + 1) - 1 needs, 1..4), chosen by the arguments and
 * never by the image; no host readback, no memset node (the tables are zeroed by a library kernel), no thread that waits
 * for another: every cross-workgroup prefix is a scan in a launch of its own, so the call can be captured and is correct
 * at any residency.  Record starts are counted per block of positions, scanned and compacted into (key, start, end); a
 * stable LSD radix sort on the key, one byte a pass, groups them (the in-chunk ranking is dfw_seg_rle's: no atomic decides
 * a position); the heads of the sorted records are counted, scanned and compacted into the pair rows.  Atomics only add
 * counts and sums.  Nothing is written outside pairs[.., :kept], the other outputs and ws; the inputs are read only.
 *
 * Validated on the host before the first launch.  DFW_EINVAL: null args / pids / gids / an output / ws; B, H, W, capP, capG,
 * max_records or max_pairs < 1; a threshold that breaks the rule above; nlabels outside 1..254 (with or without stats: pq
 * has nlabels + 1 rows).  DFW_ERANGE: H or W above 65535, H * W above 2^30, B above 65535, a highest key (capP + 1) *
 * (capG + 1) - 1 above 2^31 - 1, word counts of an output or of a workspace array beyond an int.  Then the workspace and
 * the buffers, by the rule above.
 */
typedef struct {
  const int32_t* pids;     /* [B][H][W] contiguous, read only: the prediction's ids */
  const int32_t* gids;     /* [B][H][W] contiguous, read only: the ground truth's ids */
  const int32_t* pstats;   /* optional [B][capP][8]: column 0 is the class of object row + 1 */
  const int32_t* gstats;   /* optional [B][capG][8] */
  const uint8_t* skip;     /* optional [B][H][W]: a pixel whose byte is 255 is not counted */
  int32_t* pairs;          /* out [B][max_pairs][3]: (p, g, inter); rows [kept, max_pairs) are left as they were */
  int32_t* pair_off;       /* out [B][capP + 2] */
  int32_t* area;           /* out [B][capP + capG + 2] */
  int32_t* match;          /* out [B][capP][3]: (g, inter, union) */
  int32_t* gmatch;         /* out [B][capG] */
  int64_t* pq;             /* out [B][nlabels + 1][4]: (TP, FP, FN, S) */
  int32_t* n;              /* out [B][4]: (pairs kept, pairs found, records kept, records found) */
  void* ws;
  size_t ws_bytes;
  int32_t B, H, W, capP, capG, nlabels, max_records, max_pairs, num, den;   /* the IoU threshold is num / den */
} dfw_seg_match_args;
int dfw_seg_match(const dfw_seg_match_args* a, dfw_stream_t stream);
/* 0 for sizes dfw_seg_match refuses (DFW_EINVAL or DFW_ERANGE); monotone in every argument over the sizes it accepts */
size_t dfw_seg_match_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t capP, int32_t capG, int32_t max_records,
                                     int32_t max_pairs);
/* positions one scan block covers, records one sort chunk covers: the sizes at which the kernels change path, for tests
 * and docs */
int dfw_seg_match_block(int32_t* pixels, int32_t* records);
/* dfw_seg_rle_rounds for dfw_seg_match (version >= 117) */
int dfw_seg_match_rounds(int32_t B, int32_t H, int32_t W, int32_t capP, int32_t capG, int32_t max_records, int32_t max_pairs,
                         dfw_seg_sort_rounds* out);

/*
 * Per-object confidence (version >= 118): how sure the decoder is of every object of an id map -- the uint8 mask planes
 * the label rule was computed from, reduced over the ids.  A segmented reduction, per object and exact.  All integers:
 * the result depends on no order of execution.
 *
 *   Position is q = y * W + x.
 *   A pixel is COUNTED when 1 <= id <= cap, l = labels[q] lies in 1..nlabels and g = planes[b][l] lies in 0..P-1.
 *   A counted pixel's value is s = u0 + u1 + u2, the three bytes of plane group g at q: 0..765, the numerator of
 *   dfw_seg_labels' score_c.
 *   Row id - 1 of scores[b] is (sum of s, counted pixels, min s, max s) over the object's counted pixels; a row without a
 *   counted pixel is (0, 0, 0, 0).  Every row 0..cap-1 is written.  Ids above cap are not scored, as stats does not list
 *   them; negative ids count as 0.
 *
 *   ids          normally dfw_seg_components' ids (any int32 map is accepted)
 *   labels       normally dfw_seg_components' filtered map: the class byte of every pixel
 *   seg_u8       P plane groups of three channels, each [H][W].  Which group a class of an image reads is the table's
 *                business, so one layout serves every route: N-way class-major planes [N][B] give planes[b][l] =
 *                (l - 1) * B + b, the binary routes planes[b][1] = b, entry-major candidate planes planes[b][lab[e]] = e
 *   planes       device, [B][nlabels + 1]: the plane group of label l of image b, -1 for none; entry 0 is never read.  The
 *                kernel reads it when it RUNS and clamps what it reads: an entry outside 0..P-1 means "not counted", so a
 *                table overwritten later gives other numbers, never a read outside seg_u8
 *   planes_host  its host mirror: what this call validates
 *   ws           dfw_seg_scores_workspace_bytes(B, cap) bytes.  The call writes every word it reads: the caller
 *                initialises nothing
 *
 * ids [[1,1,2]], labels [[2,2,1]], cap = 2, nlabels = 2, planes = [[*, -1, 0]], group 0 = channels [[10,20,9]],
 * [[1,2,9]], [[0,3,9]]: the two pixels of object 1 carry label 2 -> group 0 and s = 11 and 25, so row 0 = (36, 2, 11, 25);
 * object 2's pixel carries label 1, which has no plane: row 1 = (0, 0, 0, 0).
 *
 * Three launches whatever the image holds: a library kernel zeroes the accumulators (no memset node), the reduction, and
 * a finish kernel that writes every row.  No host readback, no thread that waits for another: the call can be captured
 * and is correct at any residency.  The reduction never issues an atomic per pixel: a workgroup covers a block of
 * dfw_seg_scores_block() consecutive positions, each thread folds its equal neighbouring ids, a segmented scan folds the
 * runs across the lanes of a wave and LDS across the waves, and every maximal piece of one id inside the block issues ONE
 * set of integer atomics (64-bit add of the sum, 32-bit add / max / max of the rest; the minimum is kept as the maximum
 * of 765 - s, so zero is every field's identity).  Nothing is written outside scores and ws; the inputs are read only.
 *
 * Validated on the host before the first launch, in this order.  DFW_EINVAL: null args / ids / labels / seg_u8 / planes /
 * planes_host / scores / ws; B, H, W, cap or P < 1; nlabels outside 1..254.  DFW_ERANGE: H or W above 65535, H * W above
 * 2^30, B above 65535; P * 3 * H * W above 2^63 - 1 (seg_u8 is addressed in size_t, so no int32 arguments reach this);
 * B * cap * 5 above 2^31 - 1 (the accumulators' words and the rows of scores are counted in an int; the B * cap * 4 words
 * of scores are addressed in size_t).  DFW_EINVAL: a planes_host entry 1..nlabels above P - 1 or below -1.
 * Then the workspace and the buffers, by the rule above: sizes are judged before the table, the table before the
 * workspace.  planes_host is host memory and no part of the overlap rule.
 */
typedef struct {
  const int32_t* ids;           /* [B][H][W] contiguous, read only */
  const uint8_t* labels;        /* [B][H][W] contiguous, read only */
  const uint8_t* seg_u8;        /* [P][3][H][W] contiguous, read only */
  const int32_t* planes;        /* device [B][nlabels + 1]: plane group per label, -1 for none; entry 0 unused */
  const int32_t* planes_host;   /* host mirror of planes */
  int64_t* scores;              /* out [B][cap][4]: (sum, counted pixels, min, max) */
  void* ws;
  size_t ws_bytes;
  int32_t B, H, W, cap, nlabels, P;
} dfw_seg_scores_args;
int dfw_seg_scores(const dfw_seg_scores_args* a, dfw_stream_t stream);
/* 0 for sizes dfw_seg_scores refuses (B or cap < 1, B above 65535, B * cap * 5 above 2^31 - 1); monotone otherwise */
size_t dfw_seg_scores_workspace_bytes(int32_t B, int32_t cap);
/* positions one workgroup covers: the size at which the kernel changes path, for tests and docs */
int dfw_seg_scores_block(int32_t* pixels);

/* Boundary bands (objects.boundary_bands, Boundary IoU of Cheng et al., CVPR 2021): the capped chessboard distance of
 * every pixel of a label map or an id map to its own contour.  All integers: the result depends on no order of execution.
 *
 *   map is [B][H][W] of uint8 (elem = 1) or int32 (elem = 4).  Values are compared for equality only; 0 is background and
 *   every other value -- 255, values above 255 and negative ints included -- is an object value.
 *   For a pixel q = (y, x) with v = map[q] != 0, D(q) is the smallest max(|dy|, |dx|) to a position that lies outside the
 *   image or holds a value != v: D >= 1, and a pixel on the image's edge or next to another value has D = 1.  Images of a
 *   batch never see each other.
 *   dist[q] = 0 where map[q] == 0, else min(D(q), dmax + 1): dmax + 1 means "deeper than dmax", so one dist answers every
 *   band width d <= dmax.
 *   band (optional, the type of map) holds map[q] where 1 <= dist[q] <= d and 0 elsewhere.  For the binary mask map == v
 *   this is mask - eroded of the published mask_to_boundary (zero padding, d iterations of a 3 x 3 erosion).
 *
 * map [[7,7,7,7,7],[7,7,7,7,7],[7,7,7,7,7]] with dmax = 2: dist [[1,1,1,1,1],[1,2,2,2,1],[1,1,1,1,1]], and with d = 1 band
 * is the map with its three middle pixels of the middle row set to 0.
 *
 * Two launches whatever the image holds (a row pass into ws, one byte a pixel, and a column pass that writes dist and
 * band), no memset node, no host readback, no atomics and no thread that waits for another: the call can be captured and
 * is correct at any residency.  The column pass takes four pixels a thread when W % 4 == 0 and map, band and dist are
 * aligned to four elements; one pixel a thread otherwise.  Nothing is written outside dist, band and ws; map is read only.
 *
 * Validated on the host before the first launch, in this order.  DFW_EINVAL: null args / map / dist / ws; elem not 1 or
 * 4; dmax outside 1..254; d outside 1..dmax when band is given; B, H or W < 1.  DFW_ERANGE: H, W or B above 65535, H * W
 * above 2^30.  Then the workspace and the buffers, by the rule above: map and band are aligned to their element, dist
 * needs no alignment.
 *
 * The Euclidean metric and inscribed circles (version >= 124): metric, peaks and cap, appended to the struct.  With all
 * three zero the call is the one above, launch for launch and byte for byte.  With metric = 1:
 *
 *   D2(q), for v = map[q] != 0, is the smallest (y - y')^2 + (x - x')^2 over the integer positions (y', x') that lie
 *   outside the image or hold a value != v.
 *   dist is uint16 [B][H][W] (2 * B * H * W bytes, aligned to 2): 0 where map[q] == 0, else min(D2(q), (dmax + 1)^2), at
 *   most 255^2 = 65 025; the cap means "at least dmax + 1 away".
 *   band holds map[q] where 1 <= dist[q] <= d^2 and 0 elsewhere.
 *   peaks (optional; int32 id maps only) is int64 [B][cap]: row k - 1 = the maximum over the pixels q = (y, x) with map[q]
 *   == k of (dist[q] << 32) | (0xFFFFFFFF - (y * W + x)) -- the largest squared distance of object k, i.e. the squared
 *   radius of its largest inscribed circle, capped like dist, and among equals the smallest position, its centre -- and 0
 *   when no pixel holds k.  Values outside 1..cap are not counted.
 *
 * map [[7,7,7],[7,7,7],[7,7,7]] with metric = 1, dmax = 2: dist [[1,1,1],[1,4,1],[1,1,1]]; as ids with cap = 7, row 6 of
 * peaks is (4 << 32) | (0xFFFFFFFF - 4) and the other rows are 0.
 *
 * The two-pass form.  h(y, x), which the row pass writes to ws capped at dmax + 1, is the distance along the row to the
 * nearest position that is outside the row or holds another value.  Then
 *   D2(y, x) = min(min(y + 1, H - y)^2, min over dy of c(dy)),  c(0) = h(y, x)^2,
 *   c(dy) = dy^2 + h(y + dy, x)^2 while map[y + dy][x] == v, and c(dy) = dy^2 at the first row where it differs;
 * nothing beyond that row, or beyond dy^2 >= the best so far, can be smaller.  Sketch of the proof: every candidate is the
 * squared distance to a real differing position, so the minimum is not below D2; and for a nearest differing position
 * (y', x') either column x holds v from y to y', and then h(y', x) reaches a differing position of row y' no farther along
 * than x', or the column differs earlier, at a row that is nearer.  Capping h changes no capped D2: a candidate with h >
 * dmax + 1 is above (dmax + 1)^2 already.  The workspace is the same one byte a pixel; its query does not change.
 *
 * Launches: the row pass and a column pass of its own (the same tile and the same four-pixels-a-thread rule, dist aligned
 * to four of its elements; every product stays below 2 * 255^2, the walk ends after at most dmax steps), two without
 * peaks; with peaks a library kernel zeroes the table first (no memset node) and the column pass reduces it, three.  The
 * reduction issues no atomic per pixel: a thread folds its pixels of equal id, a wave its lanes' maximal pieces of equal
 * id, and one 64-bit atomic maximum goes out per piece unless the row already holds as much.  A maximum is order-free:
 * the table depends on no order of execution and on no residency.
 *
 * Further refusals, each behind the existing ones of its kind: DFW_EINVAL for metric not 0 or 1, and for peaks with
 * metric = 0, elem != 4 or cap < 1 (after d); DFW_ERANGE for B * cap above 2^31 - 1 with peaks (after the sizes, before
 * the workspace).  peaks is an output of the buffer rule, aligned to 8; cap is not looked at without peaks.
 */
typedef struct {
  const void* map;              /* [B][H][W] of uint8 or int32, contiguous, read only */
  void* dist;                   /* out [B][H][W] of uint8, or of uint16 when metric = 1 */
  void* band;                   /* out [B][H][W] of map's type, or null */
  void* ws;
  size_t ws_bytes;
  int32_t elem, B, H, W, dmax, d;
  int32_t metric;               /* 0 chessboard, 1 Euclidean (squared) */
  void* peaks;                  /* out int64 [B][cap], or null; metric = 1 and elem = 4 only */
  int32_t cap;
} dfw_seg_boundary_args;
int dfw_seg_boundary(const dfw_seg_boundary_args* a, dfw_stream_t stream);
/* 0 for sizes dfw_seg_boundary refuses (B, H or W < 1 or above 65535, H * W above 2^30, elem not 1 or 4) */
size_t dfw_seg_boundary_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t elem);
/* the tile of the column pass (rows x cols) and the positions a workgroup of the row pass covers, for tests and docs */
int dfw_seg_boundary_block(int32_t* rows, int32_t* cols, int32_t* positions);

/* Per-class counts of two boundary bands, in dfw_seg_labels' counts layout.  Per pixel: dropped when gt > nlabels (255
 * included); else l = pred if 1 <= pdist <= d, else 0, and g = gt if 1 <= gdist <= d, else 0; predicted[l]++ when l <=
 * nlabels, truth[g]++, intersection[l]++ when l == g.  counts [B][2][nlabels + 1] = (intersections, unions = predicted +
 * truth - intersection) per image; bin 0 holds the pixels in neither band.  gdist is the distance of gt as given: 255 is a
 * value like any other there, so a class pixel beside an ignore region lies in the band.  Counts for several d come from
 * one pair of dist maps by calling again.  Two launches: a library kernel zeroes counts (no memset node), then LDS
 * histograms per workgroup flushed with 64-bit integer atomics; capturable, order-free.
 *
 * Validated in this order.  DFW_EINVAL: null args / pred / pdist / gt / gdist / counts; d outside 1..254; nlabels outside
 * 1..254; B, H or W < 1.  DFW_ERANGE: as dfw_seg_boundary.  Then the buffers, by the rule above; there is no workspace.
 *
 * dist_elem (version >= 124, appended): 0 and 1 mean uint8 dist maps as above, byte for byte; 2 means the uint16 squared
 * maps of metric = 1, both of them, aligned to 2, with the band rule 1 <= dist <= d * d.  Any other value is DFW_EINVAL,
 * behind nlabels.
 */
typedef struct {
  const uint8_t* pred;          /* [B][H][W] label bytes, read only */
  const void* pdist;            /* [B][H][W] dfw_seg_boundary's dist of pred, uint8 or uint16 (dist_elem) */
  const uint8_t* gt;            /* [B][H][W] */
  const void* gdist;            /* [B][H][W] dist of gt, of the same kind */
  int64_t* counts;              /* out [B][2][nlabels + 1] */
  int32_t B, H, W, d, nlabels;
  int32_t dist_elem;            /* 0 | 1: uint8 distances; 2: uint16 squared distances */
} dfw_seg_boundary_counts_args;
int dfw_seg_boundary_counts(const dfw_seg_boundary_counts_args* a, dfw_stream_t stream);

/*
 * Outlines of labelled objects (version >= 121): every object of an id map, normally the one dfw_seg_components or
 * dfw_seg_holes wrote (any int32 map is accepted), as rings of corner points -- what GeoJSON polygons, COCO polygon
 * segmentations and GIS tools take.  All integers: the result depends on no order of execution.
 *
 *   v(y, x)    the id when 1 <= id <= cap, else 0; outside the image v is 0
 *   pixel      (x, y) is the unit square with the corners (x, y) and (x + 1, y + 1); vertices are the lattice points
 *              0 <= X <= W, 0 <= Y <= H
 *   edge       a side of a pixel p with v(p) != 0 whose pixel across that side has a different v.  Edges are directed
 *              clockwise on screen (y down), the object on the right: side 0 is the top, heading east; 1 the right, heading
 *              south; 2 the bottom, heading west; 3 the left, heading north.  Its key is 4 * (y * W + x) + side.  Between two
 *              different objects both pixels own an edge
 *   successor  of edge e of pixel p, side s, id i; it depends on `connectivity`, which must be the one the ids were made
 *              with.  A is the pixel ahead of p in the heading, L the pixel to the left of A relative to the heading.  A
 *              left turn goes to side (s + 3) % 4 of L, straight to side s of A, a right turn to side (s + 1) % 4 of p.
 *              Connectivity 8: left if v(L) == i, else straight if v(A) == i, else right.  Connectivity 4: right if
 *              v(A) != i, else left if v(L) == i, else straight.  The map is a bijection on the edges, also for ids that do
 *              not match the connectivity
 *   ring       a cycle of the successor; it belongs to one id.  Its leader is its smallest key, the rank of an edge the
 *              number of successor steps from the leader, its area the sum of X over its south edges minus the sum of X over
 *              its north edges, X the edge's column: the integral of x dy, positive for an outer ring, negative for a hole
 *   corners    of a ring: the start vertices of the edges whose predecessor has another heading, in ascending rank.  The
 *              leader's own start need not be one (a hole two pixels wide).  With connectivity 8 a ring may visit a vertex
 *              twice, where two pixels touch diagonally; it never crosses itself
 *
 *   n          per image (edges found, corners, rings, complete); complete = 1 when edges found <= max_edges.  Otherwise
 *              n = (edges found, 0, 0, 0), ring_off is all zero and no row of rings or verts is written: there are no
 *              partial results, a cut ring is not a ring.  The caller sizes max_edges from n[0] and calls again
 *   rings      (id, first, count, area), sorted by id ascending, then by leader ascending; first is the row of the ring's
 *              first corner in verts
 *   ring_off   object k's rings are rows ring_off[k-1] .. ring_off[k]; ring_off[0] = 0
 *   verts      (X, Y); each ring's corners are contiguous and in rank order, the rings in the order of `rings`
 *   ws         dfw_seg_contours_workspace_bytes(..) bytes, 4 per pixel and 64 per edge of max_edges and a little more.  The
 *              call writes every word it reads: the caller initialises nothing
 * Rows behind the kept ones are left as they were; nothing is written outside the four outputs and ws; ids is read only.
 *
 * When the ids come from dfw_seg_components with the same connectivity, the first ring of an object is its only outer
 * ring and its leader has side 0, every later ring is a hole ring (negative area, a leader of another side), and the areas
 * of an object's rings sum to its pixel count.
 *
 * Connectivity 8, cap = 1.  [[1,1,1,1],[1,0,0,1],[1,1,1,1]] has 20 edges and two rings: (1, 0, 4, 12) with the corners
 * (0,0) (4,0) (4,3) (0,3) and (1, 4, 4, -2) with the corners (1,1) (1,2) (3,2) (3,1).  The diamond [[0,1,0],[1,0,1],[0,1,0]]
 * has 16 edges: the outer ring has 12 corners, starts at (1,0) and has area 5, the hole ring has the corners (2,1) (1,1)
 * (1,2) (2,2) and area -1.  Under connectivity 4 with the ids 1..4 the same diamond gives four unit squares.
 *
 * A fixed number of launches, 14 + 2 * R + 3 * passes with R = ceil(log2(max_edges)) and passes = the bytes cap needs (1
 * below 256, 2 below 65536, ..), chosen by the arguments and never by the image; no host readback, no memset node
 * (ring_off is zeroed by a library kernel), no thread that waits for another: every cross-workgroup prefix is a scan in a
 * launch of its own, the cycles are followed by pointer doubling between two buffers in turn (R rounds to find every
 * ring's leader, R to sum corners and area to the ring's end), and the ring table is sorted by dfw_seg_rle's stable radix
 * sort -- no atomic decides a position.  The call can be captured and is correct at any residency.
 *
 * Validated on the host before the first launch, in this order.  DFW_EINVAL: null args / ids / verts / rings / ring_off /
 * n / ws; connectivity not 4 or 8; B, H, W or cap < 1; max_edges < 4 or not a multiple of 4.  DFW_ERANGE: H, W or B above
 * 65535, 4 * H * W above 2^31 - 1 (the keys), B * max_edges * 2 or B * (cap + 1) above 2^31 - 1.  Then the workspace and
 * the buffers, by the rule above, with alignments of its own: verts 8 bytes, rings, n and ws 16 (rows and records of 16).
 *
 * SIMPLIFIED RINGS (version >= 123), an optional last stage of the same call, as approxPolyDP stands behind findContours:
 * Douglas-Peucker with a tolerance of tol4 quarter pixels on every ring, in integers only, so the result is exact and
 * depends on no order of execution.  With simp_verts, simp_rings and simp_n null and tol4 = 0 the call is what it was,
 * launch for launch.  A ring is the count >= 4 corners P[0..c) of one row of rings, in rank order and closed (P[c] means
 * P[0]).
 *   1  anchors: f is the corner with the largest squared distance from P[0], the lowest rank on ties.  Corners 0 and f
 *      are kept; the chains are (0, f) and (f, c)
 *   2  a chain (a, b) with b - a >= 2: the measure m(i) of an interior corner is, in line mode (P[a] != P[b]),
 *      |(bx-ax)(py-ay) - (by-ay)(px-ax)| with L = (bx-ax)^2 + (by-ay)^2, and in point mode (P[a] == P[b]: an 8-connected
 *      ring may visit a vertex twice) its squared distance to P[a].  The winner w has the largest m; on ties the rank
 *      nearest the middle, the smallest |2i - (a+b)|, then the lower rank.  w is kept iff 16 m^2 > tol4^2 L (line mode) or
 *      16 m > tol4^2 (point mode), strictly.  If w is kept the chains (a, w) and (w, b) follow, else every interior corner
 *      is dropped.  The distance is the one to the infinite line through the anchors, as in the original algorithm
 *   3  if only the two anchors survive, the corner with the largest line-mode measure against P[0]P[f] is kept too, the
 *      lowest rank on ties: a ring encloses area, so that measure is above zero, every ring keeps at least 3 corners and
 *      no ring disappears
 * The middle rule keeps the rounds few: a perfect 45 degree staircase at half a pixel splits in the middle every round
 * where "lowest rank" would peel one corner a round.  At tol4 = 0 every corner is kept.  Example: [[1,0],[0,1]] with
 * connectivity 8 is one ring of 8 corners, (0,0) (1,0) (1,1) (2,1) (2,2) (1,2) (1,1) (0,1); at tol4 = 4 the anchors are
 * ranks 0 and 4, every other corner lies within one pixel of the diagonal, and rule 3 keeps rank 1: ranks 0, 1, 4.
 * Bounds: 4 H W <= 2^31 - 1 gives |cross| <= 2 H W < 2^30, so 16 m^2 < 2^64; a point-mode m is at most 2 * 65535^2 <
 * 2^33; tol4 <= 32768 (8192 pixels) and L < 2^33 give tol4^2 L < 2^63: everything fits 64 unsigned bits.  A winner is
 * one order-free 64-bit maximum of the packed key m << 31 | (2^31 - 1 - (2 |2i - (a+b)| + (2i > a+b))), 33 bits above 31.
 *   simp_rings  row r = (id, first', count', area) in the rows and the order of rings; area is the ORIGINAL ring's exact
 *               area, whose sign still tells outer from hole: the simplified polygon's area is not computed
 *   simp_verts  the kept corners, contiguous per ring in rank order; a ring's first corner is still P[0]
 *   simp_n      (corners in, corners kept, rings, complete): dfw_seg_contours' readers of columns 1 to 3 take it as it is.
 *               An image that is not complete gets (0, 0, 0, 0) and no row
 *   ring_off    is shared with the unsimplified result
 * Rows behind the kept ones are left as they were.  Douglas-Peucker preserves no topology: a simplified ring may touch or
 * cross itself or a neighbour, and two objects' shared border is simplified twice, independently.
 * Three more launches (dfw_seg_contours_trips.simplify_launches), whatever the image: one workgroup of 256 per ring row
 * runs the level-synchronous form in a bounded loop -- every round each live chain finishes or keeps one more corner, at
 * most count - 2 rounds, the exit test uniform over the workgroup -- with the state of a ring of at most
 * dfw_seg_contours_simplify_block() corners in LDS and of a longer one in the workspace; a scan of the corners kept per
 * ring gives first'; one workgroup per ring row writes.  No memset node, no readback, no atomic decides a position, no
 * thread waits for another workgroup.  The workspace does not grow: the state lives where the pointer doubling's buffers
 * lay.  Validated with the null pointers and scalars (DFW_EINVAL, before the sizes): some but not all of the three
 * pointers; tol4 outside 0..32768; tol4 != 0 with the stage off.  The three outputs are written buffers of the table
 * above, also against verts, rings and n, which the stage reads.
 */
typedef struct {
  const int32_t* ids;      /* [B][H][W] contiguous, read only */
  int32_t* verts;          /* out [B][max_edges][2]: (X, Y); rows behind the corners are left as they were */
  int32_t* rings;          /* out [B][max_edges / 4][4]: (id, first, count, area); rows behind the rings are left */
  int32_t* ring_off;       /* out [B][cap + 1] */
  int32_t* n;              /* out [B][4]: (edges found, corners, rings, complete) */
  void* ws;
  size_t ws_bytes;
  int32_t B, H, W, cap, max_edges, connectivity;   /* connectivity 4 | 8: the one the ids were made with */
  /* the simplified rings (version >= 123, below): all three null and tol4 = 0 -- the stage is off -- or all three given */
  int32_t* simp_verts;     /* out [B][max_edges][2], 8-byte aligned: the kept corners; rows behind them are left */
  int32_t* simp_rings;     /* out [B][max_edges / 4][4], 16-byte aligned: (id, first', count', area of the original ring) */
  int32_t* simp_n;         /* out [B][4], 16-byte aligned: (corners in, corners kept, rings, complete) */
  int32_t tol4;            /* the tolerance in quarter pixels, 0..32768 */
} dfw_seg_contours_args;
int dfw_seg_contours(const dfw_seg_contours_args* a, dfw_stream_t stream);
/* 0 for arguments dfw_seg_contours answers DFW_EINVAL for; monotone in every argument */
size_t dfw_seg_contours_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_edges);
/* pixels one scan block covers, edges one block of the ring count covers: the sizes at which the kernels change path, for
 * tests and docs */
int dfw_seg_contours_block(int32_t* pixels, int32_t* edges);
/* The trip counts of dfw_seg_contours (host only, launches nothing), computed by the expressions the launcher uses, for
 * tests and docs.  Errors: DFW_EINVAL for a null out, then the size errors of dfw_seg_contours in its order; pointers,
 * connectivity, workspace and overlap are not part of it. */
typedef struct {
  int32_t blocks;         /* scan blocks of `pixels` positions per image */
  int32_t block_scan;     /* trips of the scan of the block sums, 1024 words a trip: edges found */
  int32_t doubling;       /* R: the rounds of each of the two pointer-doubling loops */
  int32_t ring_blocks;    /* blocks of `edges` edges per image */
  int32_t ring_scan;      /* trips of the scan of the leaders per block: rings */
  int32_t passes;         /* digit passes of the sort, each with one table scan */
  int32_t table_scan;     /* trips of the scan of the digit table, 256 words per chunk of ring rows */
  int32_t offsets_scan;   /* trips of the scan of ring_off (cap + 1 words) */
  int32_t corners_scan;   /* trips of the scan of the corners per ring (max_edges / 4 words) */
  int32_t launches;       /* 14 + 2 * doubling + 3 * passes */
  int32_t simplify_launches;   /* 3: the launches behind them when the simplified rings are asked for */
} dfw_seg_contours_trips;
int dfw_seg_contours_rounds(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_edges, dfw_seg_contours_trips* out);
/* the ring length up to which the simplification keeps a ring's state in LDS; longer rings keep it in the workspace.
 * Host only, launches nothing.  DFW_EINVAL for a null pointer */
int dfw_seg_contours_simplify_block(int32_t* lds_corners);

/* ======================================================================================================
 * Training step (BASELINE configs[4]; train_tools/train_icl_multitask_nocrop_nearest_nshot_v3.py:1374-1396 =
 * T): backward of the UNet's ops.  Data gradients of Linear / conv3x3 are dfw_gemm calls with transposed /
 * tap-mirrored weights; everything else is below.  All reductions are deterministic (fp32 slabs folded in a
 * fixed order).  `accumulate` != 0 adds into the output gradient (gradient accumulation, T:1323), else
 * overwrites; `scale` / `grad_scale` multiply parameter gradients (1 / loss scale of fp16 training).
 * ====================================================================================================== */

/* Weight gradient on MFMA: out[b][n][tap][k] (+)= scale * sum_m A[m][n] * B[row(m, tap)][k]
 *   taps == 1: dW = dY^T X for nn.Linear (A = dY [M][lda], B = X [M][ldb]; torch autograd of A:237-245, A:276);
 *   taps == 9: dW[Cout][ky][kx][Cin] of a conv3x3 (A = dY NHWC rows, B = the conv's NHWC input gathered with the
 *              forward's stride / pad / fused nearest-2x upsample), the packed layout dfw_gemm consumes.
 * batch / batch2: independent problems at element strides strideA/strideB (and strideA2/strideB2).
 * out strides in floats: ldo_n (0 => taps*Kc), ldo_t (0 => Kc), ldo_b (0 => N*taps*Kc).
 * workspace: dfw_gemm_tn_workspace_bytes() (split-M slabs). N, Kc, lda, ldb multiples of 8. */
typedef struct {
  const void* A; const void* B; float* out;
  void* workspace; size_t workspace_bytes;
  int64_t a_elems, b_elems;
  int32_t M, N, Kc, lda, ldb;
  int32_t taps, Hi, Wi, Ho, Wo, stride, pad, ups;
  int32_t batch, batch2; int64_t strideA, strideB, strideA2, strideB2;
  int64_t ldo_n, ldo_t, ldo_b;
  float scale; int32_t accumulate;
  int32_t dtype;
} dfw_gemm_tn_args;

int dfw_gemm_tn(const dfw_gemm_tn_args* a, dfw_stream_t stream);
size_t dfw_gemm_tn_workspace_bytes(const dfw_gemm_tn_args* a);
/* Which kernel dfw_gemm_tn would launch for these arguments (host-only plan query, like dfw_gemm_kernel_name), e.g.
 * "gemm_tn_ring_kernel<bf16,2,1,conv>+split6" or "gemm_tn_kernel<f16>+split2" (+splitS: S split-M slabs folded by
 * tn_reduce_kernel; no suffix: one split, written directly). */
int dfw_gemm_tn_kernel_name(const dfw_gemm_tn_args* a, char* buf, size_t n);

/* Column sums: out[seg * ldo + n] (+)= scale * sum_{r < rows_per_seg} x[(seg * rows_per_seg + r) * ldx + n].
 * Bias gradients (segs = 1) and the gradient of the per-image time-embedding projection added in
 * ResnetBlock2D (segment = image).  workspace: dfw_colsum_workspace_bytes(). */
int dfw_colsum(const void* x, float* out, void* workspace, size_t workspace_bytes, int64_t rows_per_seg, int32_t segs,
               int32_t N, int32_t ldx, int64_t ldo, float scale, int32_t accumulate, int32_t dtype, dfw_stream_t stream);
size_t dfw_colsum_workspace_bytes(int64_t rows_per_seg, int32_t segs, int32_t N);

/* Every column sum of a backward walk in two launches.  items: DEVICE array of n_items records of sixteen int64_t
 * { x, out, rows_per_seg, segs, N, ldx, ldo, scale (float bits), accumulate, chunks, rpc, part_off, block_begin1, block_begin2,
 *   0, 0 }: the dfw_colsum arguments of the item (x / out as addresses), its plan from dfw_colsum_plan(), the offset in floats
 * of its segs * chunks * N partial sums in `workspace`, and its first block in the two flattened grids:
 *   block_begin1[i+1] = block_begin1[i] + ceil(N / 256) * chunks * segs,  block_begin2[i+1] = block_begin2[i] + ceil(N / 16) * segs;
 * total_blocks1 / 2 = the sums.  All items share `dtype`; N % 8 == 0, ldx % 8 == 0 (caller-checked).  Deterministic. */
int dfw_colsum_plan(int64_t rows_per_seg, int32_t* chunks, int32_t* rpc);
/* Write n_records (<= 24) records of sixteen int64_t from HOST memory `records` into the DEVICE table at record index
 * first_record.  The records travel as kernel arguments: no pinned memory, no memcpy node -- capture-safe. */
int dfw_table_write(void* table, int64_t first_record, const int64_t* records, int32_t n_records, dfw_stream_t stream);
int dfw_colsum_batch(const void* items, int32_t n_items, int64_t total_blocks1, int64_t total_blocks2, void* workspace,
                     int32_t dtype, dfw_stream_t stream);

/* GroupNorm(+SiLU) backward (torch.nn.GroupNorm + F.silu under autograd; ResnetBlock2D.norm1/norm2,
 * Transformer2DModel.norm, conv_norm_out).  mean_rstd [B][groups][2] are the forward's statistics
 * (the tail of dfw_groupnorm's stats_ws).  dgamma / dbeta may be NULL.
 * dx_add (optional, laid out like dx): a gradient x has already received from another consumer (the residual add that
 * follows the block: pre-norm blocks reach their input's gradient through a norm backward LAST); dx = computed + dx_add,
 * summed in fp32 and rounded once -- the separate add pass over the activation is gone. */
typedef struct {
  const void* x; const void* dy; void* dx; const float* gamma; const float* beta; const float* mean_rstd;
  float* dgamma; float* dbeta;
  void* workspace; size_t workspace_bytes;
  int32_t B, HW, C, groups, ldx, lddy, lddx;
  int32_t silu, accumulate;
  float grad_scale;
  int32_t dtype;
  const void* dx_add;
} dfw_groupnorm_bwd_args;

int dfw_groupnorm_bwd(const dfw_groupnorm_bwd_args* a, dfw_stream_t stream);
size_t dfw_groupnorm_bwd_workspace_bytes(const dfw_groupnorm_bwd_args* a);

/* LayerNorm backward (BasicTransformerBlock.norm1/2/3); statistics are recomputed from x.  dx_add: as above (rows at
 * stride lddx). */
typedef struct {
  const void* x; const void* dy; void* dx; const float* gamma; float* dgamma; float* dbeta;
  void* workspace; size_t workspace_bytes;
  int32_t rows, C, ldx, lddy, lddx;
  float eps;
  int32_t accumulate;
  float grad_scale;
  int32_t dtype;
  const void* dx_add;
} dfw_layernorm_bwd_args;

int dfw_layernorm_bwd(const dfw_layernorm_bwd_args* a, dfw_stream_t stream);
size_t dfw_layernorm_bwd_workspace_bytes(int32_t rows, int32_t C);

/* GEGLU on the packed column order (see dfw_gemm_args.geglu): pre [rows][2H].
 * dout == NULL: forward, out [rows][H] = value * gelu(gate); else backward, out = d(pre) [rows][2H]. */
int dfw_geglu(const void* pre, const void* dout, void* out, int64_t rows, int32_t H, int32_t dtype, dfw_stream_t stream);

/* Data movement of the backward graph, C % 8 == 0:
 *   mode 0  y = a + b                                  [rows][C]    (a tensor consumed twice: residual, skip)
 *   mode 1  y = a[:, c0 : c0 + C], a has lda columns     (backward of torch.cat([h, skip], 1), U:1226)
 *   mode 2  y[B][2H][2W][C]: y[2i][2j] = a[i][j], else 0  (rows = B*2H*2W; stride-2 conv data gradient)
 *   mode 3  y[B][H][W][C] = 2x2 block sums of a[B][2H][2W][C]  (rows = B*H*W; fused nearest-2x upsample) */
int dfw_elementwise(int32_t mode, const void* a, const void* b, void* y, int64_t rows, int32_t C, int32_t lda,
                    int32_t c0, int32_t H, int32_t W, int32_t dtype, dfw_stream_t stream);

/* NCHW fp32 [B][C][HW] -> NHWC storage dtype [B][HW][Cp], channels zero-padded to Cp, times scale
 * (the UNet's latent inputs as the B operand of the conv_in weight gradient). */
int dfw_nchw_to_nhwc(const float* x, void* y, int32_t B, int32_t C, int32_t HW, int32_t Cp, float scale, int32_t dtype,
                     dfw_stream_t stream);

/* loss = mean((pred - target)^2) (F.mse_loss, T:1384; pred/target NCHW fp32 [B][C][HW], C <= 8) and
 * dpred = 2 (pred - target) / numel * loss_scale as NHWC storage dtype [B][HW][8] (zero-initialised by the
 * caller: channels C..7 are not written); dpred_nchw (optional): the same rounded values as NCHW fp32 [B][C][HW], the
 * input of conv_out's data-gradient conv.  workspace: 256 floats. */
int dfw_mse_loss(const float* pred, const float* target, void* dpred, float* dpred_nchw, float* loss, float* workspace,
                 int32_t B, int32_t C, int32_t HW, float loss_scale, int32_t dtype, dfw_stream_t stream);

/* The UNet's backward seeded by an EXTERNAL loss gradient g = d loss / d pred (NCHW fp32 [B][C][HW], C <= 8), e.g. from
 * torch autograd of the launcher's own loss expression (T:1381-1391): dpred / dpred_nchw as dfw_mse_loss writes them,
 * (storage dtype)(g * scale) with scale = the loss scale. */
int dfw_loss_grad(const float* g, void* dpred, float* dpred_nchw, int32_t B, int32_t C, int32_t HW, float scale,
                  int32_t dtype, dfw_stream_t stream);

/* y[i] = (float)x[i] * scale, x in the storage dtype, n % 8 == 0, 16-byte aligned (with dfw_convert_f32: the 16-bit wire
 * format of the gradient all-reduce, T:1226-1228 with grad_comm_dtype=bf16; scale = 1 / world size). */
int dfw_convert_to_f32(const void* x, float* y, int64_t n, float scale, int32_t dtype, dfw_stream_t stream);

/* KV-fusion attention backward for the lock-step batch (dfw_fsa_args.n_plain form; nshot == 0: plain
 * self-attention).  qkv [batch][n][ld >= 3C]: the fused projection output with q PRE-SCALED
 * (dfw_gemm_args.colscale); out / dout [batch][n][ldo]; lse from the forward; delta is scratch of
 * 2 * batch * heads * n floats (the kernels keep -rowsum(dO o O) in the first half and -lse in the second so the dK/dV
 * kernel fetches both row constants of a query tile with one LDS-DMA descriptor).  dqkv [batch][n][ldd >= 3C] receives (dq, dk, dv) with dq taken with respect to the UNSCALED
 * projection output, so it is the dY of the QKV Linear as is.  scale = attn.scale (A:269-271). */
typedef struct {
  const void* qkv; const void* out; const void* dout; const float* lse; float* delta; void* dqkv;
  int32_t batch, heads, n, nshot, n_plain;
  int32_t ld, ldo, ldd;
  float scale;
  int32_t dtype;
  /* Optional scratch of dfw_fsa_attention_bwd_workspace_bytes() (16-byte aligned): the dQ kernel then splits the key range
   * of the bank-reading images over several workgroups (partial dQ in fp32, summed in order), as the forward does. */
  void* workspace; size_t workspace_bytes;
  /* Bytes behind `delta` (version >= 103): must be >= 2 * batch * heads * n * sizeof(float), else DFW_EWORKSPACE -- the
   * scratch doubled in version 102, and a caller still sized for the single array must get an error, not a device write
   * past its buffer. */
  size_t delta_bytes;
} dfw_fsa_bwd_args;

int dfw_fsa_attention_bwd(const dfw_fsa_bwd_args* a, dfw_stream_t stream);
size_t dfw_fsa_attention_bwd_workspace_bytes(const dfw_fsa_bwd_args* a);

/* The same backward with queries and keys / values in their own tensors (attn2 of the training step, T:1368-1375, on
 * the MFMA path: forward = dfw_fsa_attention with n_kv = 77 prompt tokens and lse requested).  q [batch][n_q][heads*64]
 * PRE-SCALED as above; k / v [batch][n_kv][heads*64] column slices of ONE buffer (v >= k, same strides); out / dout share
 * strides; lse fp32 [batch][heads][n_q]; delta: scratch of 2 * batch * heads * n_q floats, as above.  dq with respect to the unscaled projection output;
 * dk / dv share strides.  Strides in elements.  Deterministic: no cross-workgroup sums. */
typedef struct {
  const void* q; const void* k; const void* v; const void* out; const void* dout; const float* lse; float* delta;
  void* dq; void* dk; void* dv;
  int32_t batch, heads, n_q, n_kv;
  int32_t ldq, ldkv, ldo, lddq, lddkv;
  int64_t q_bs, kv_bs, o_bs, dq_bs, dkv_bs;
  float scale;
  int32_t dtype;
  /* Optional scratch of dfw_attention_bwd_workspace_bytes() (16-byte aligned; 0 bytes when the launch fills the chip by
   * itself): with a short key axis (77 prompt tokens = one key block per image and head) the dK/dV kernel then splits the
   * query rows over several workgroups per key block (fp32 partials, summed in order: still deterministic). */
  void* workspace; size_t workspace_bytes;
  size_t delta_bytes;   /* bytes behind `delta`: >= 2 * batch * heads * n_q * sizeof(float), else DFW_EWORKSPACE (version >= 103) */
} dfw_attn_bwd_args;

int dfw_attention_bwd(const dfw_attn_bwd_args* a, dfw_stream_t stream);
size_t dfw_attention_bwd_workspace_bytes(const dfw_attn_bwd_args* a);

/* Cross-attention (attn2) backward over a short context; same tensor conventions as dfw_cross_attention.
 * dq [batch][n_q][heads*64] (strides lddq / dq_bs); dk / dv [batch][L][heads*64] at row stride lddkv, image stride
 * dkv_bs (column slices of the fused prompt K/V gradient buffer).  workspace: dfw_cross_attention_bwd_workspace_bytes. */
typedef struct {
  const void* q; const void* k; const void* v; const void* dout; void* dq; void* dk; void* dv;
  void* workspace; size_t workspace_bytes;
  int32_t batch, heads, n_q, L;
  int32_t ldq, ldk, ldv, ldo, lddq, lddkv;
  int64_t q_bs, k_bs, v_bs, o_bs, dq_bs, dkv_bs;
  float scale;
  int32_t dtype;
} dfw_xattn_bwd_args;

int dfw_cross_attention_bwd(const dfw_xattn_bwd_args* a, dfw_stream_t stream);
size_t dfw_cross_attention_bwd_workspace_bytes(int32_t batch, int32_t heads, int32_t n_q, int32_t L);

/* y = silu(a) (dy == NULL) or y = dy * silu'(a), n storage-dtype elements (the timestep-embedding MLP). */
int dfw_silu(const void* a, const void* dy, void* y, int64_t n, int32_t dtype, dfw_stream_t stream);

/* Memory-efficient attention of the VAE mid-block (diffusers AutoencoderKL `Attention`: ONE head of dim 512 over N = h * w
 * tokens; the reference routes it through xformers memory_efficient_attention, evaluation_util/main_oss.py:374-376, so the
 * N x N scores are never materialised): out[b][i] = softmax_j(q[b][i] . k[b][j]) v[b][j], flash-style, fp32 statistics.
 * q / k / v / out: [batch][n][ld* >= 512] views (16-byte aligned, ld % 8 == 0; column slices of one fused QKV buffer are
 * fine), batch strides in elements.  q must arrive multiplied by head_dim^-0.5 * log2(e) (dfw_gemm_args.colscale of the
 * projection that produced it): q_prescaled != 0 is required, head_dim must be 512.  Any n (keys beyond n are masked). */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  int32_t batch, n, head_dim, q_prescaled;
  int32_t ldq, ldk, ldv, ldo;
  int64_t q_bs, k_bs, v_bs, o_bs;
  int32_t dtype;
} dfw_vattn_args;
int dfw_vae_attention(const dfw_vattn_args* a, dfw_stream_t stream);

/* Sum of squares of an fp32 vector (the global gradient norm of clip_grad_norm_, T:1393); workspace: 1024 floats. */
int dfw_sumsq(const float* x, float* out, float* workspace, int64_t n, dfw_stream_t stream);

/* AdamW step on flat fp32 tensors (torch.optim.AdamW, T:1186-1194), with the clip factor
 * min(1, max_grad_norm / (sqrt(*grad_sumsq) + 1e-6)) applied to the gradient when grad_sumsq != NULL. */
typedef struct {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq; const float* grad_sumsq;
  int64_t n;
  float lr, beta1, beta2, eps, weight_decay, max_grad_norm;
  int32_t step;
  /* Optional: storage-dtype copy of the updated parameters (what the MFMA kernels read), written in the same pass. */
  void* shadow; int32_t shadow_dtype;
  /* Overflow guard: when grad_sumsq != NULL and *grad_sumsq is inf / NaN (one non-finite gradient), the step is SKIPPED --
   * param, both moments and the shadow are left untouched.  *found_inf (optional, device int32) is written by every call
   * that has grad_sumsq: 1 when the step was skipped, else 0.  The
   * behaviour of torch.cuda.amp.GradScaler.step under accelerate mixed_precision='fp16' (T:1017, T:1239, T:1394); the
   * host halves its loss scale on the flag (diffews_amd.train.UNetTrainer.optimizer_step). */
  int32_t* found_inf;
} dfw_adamw_args;

int dfw_adamw(const dfw_adamw_args* a, dfw_stream_t stream);

/* 16-bit weight re-layout for the data-gradient GEMMs: y[(flip ? nb-1-b : b)][c][r] = x[b][r][c], matrices of R x C
 * elements with row strides ldx / ldy and matrix strides x_bs / y_bs (all multiples of 8 elements).
 *   Linear:  nb = 1            -> W^T ([K][N] read by dfw_gemm as the weight of dX = dY W)
 *   conv3x3: nb = 9, flip != 0 -> W'[Cin][8 - tap][Cout] = W[Cout][tap][Cin] (x_bs = Cin, ldx = 9*Cin, y_bs = Cout, ldy = 9*Cout) */
int dfw_weight_relayout(const void* x, void* y, int32_t R, int32_t C, int64_t ldx, int64_t ldy, int32_t nb, int64_t x_bs,
                        int64_t y_bs, int32_t flip, dfw_stream_t stream);

/* Every re-layout of a training step in one launch.  items: DEVICE array of n_items records of twelve int64_t
 * { x, y, R, C, ldx, ldy, x_bs, y_bs, nb, flip, block_begin, 0 } -- the dfw_weight_relayout arguments of the item (x / y
 * as addresses) and the index of its first block in the flattened grid: block_begin[0] = 0, block_begin[i+1] =
 * block_begin[i] + ceil(C/64) * ceil(R/64) * nb; total_blocks = the sum.  Same alignment rules as above (caller-checked). */
int dfw_weight_relayout_batch(const void* items, int32_t n_items, int64_t total_blocks, dfw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFEWS_HIP_H */
