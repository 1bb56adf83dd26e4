/* libotrans_hip.so -- C ABI of the MI355X (gfx950) hot path for ZhengkunTian/OpenTransformer.
 *
 * The reference has no FFI (it is pure PyTorch); every entry below names the reference code it
 * replaces (paths relative to the reference root).  The reference-side binding a maintainer would
 * add is the ctypes stub shown in INTEGRATION.md (opentransformer_amd/_lib.py is that stub).
 *
 * Conventions:
 *  - plain pointers + sizes; the CALLER owns every buffer (inputs, outputs, saved-for-backward,
 *    workspace).  The library never allocates or frees device memory and keeps no pointer after
 *    a call returns.
 *  - every launch is asynchronous on the hipStream_t passed in (as void*); no hidden syncs, so all
 *    entries are legal inside hipGraph stream capture.
 *  - return 0 = OK, negative = bad argument (nothing launched), positive = hipError_t.
 *    otr_last_error_string() describes the last failure on the calling thread.
 *  - dtype codes: OTR_F32 = 0, OTR_BF16 = 1 (raw bf16 bits), OTR_F16 = 2 (IEEE binary16 bits).  The library is built
 *    twice from one source: libotrans_hip.so has bf16 as its 16-bit storage / MFMA-input type and accepts OTR_BF16,
 *    libotrans_hip_f16.so has fp16 and accepts OTR_F16 (otr_half_type() says which; the other code is rejected).
 *    Below, "bf16" in a parameter name or comment means "the 16-bit type of the build".  fp16 carries 3 more mantissa
 *    bits (logits 5e-4 from the fp32 reference instead of 3.9e-3, tools/precision_study.py) at the same MFMA rate;
 *    its gradients need loss scaling (see otr_optimizer_step).  `compute` selects the MFMA type: the 16-bit code ->
 *    v_mfma_f32_{16x16x32,32x32x16}_{bf16,f16} (fp32 accumulate), OTR_F32 -> v_mfma_f32_16x16x4_f32 (exact fp32,
 *    the parity mode).
 */
#ifndef OTRANS_HIP_H
#define OTRANS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OTR_F32 0
#define OTR_BF16 1
#define OTR_F16 2
#define OTR_ACT_NONE 0
#define OTR_ACT_RELU 1

/* ABI version of THIS header: bumped whenever a signature, a descriptor struct or the meaning of an argument changes (600: round 6;
 * 300 was rounds 3-5, during which otr_optimizer_step, otr_ln_desc_t, otr_wgrad_item_t and otr_beam_prune_cached changed without a
 * bump; 602: the rescoring entries, additions only; 603: otr_ctc_align, additions only; 604: otr_ngram_lookup and otr_ctc_beam_search_lm, additions only; 605:
 * otr_edit_distance, additions only; 606: otr_ngram_score_cands, otr_ngram_score_seqs and otr_rescore_select_add, additions only; 607: otr_ngram_count, otr_ngram_stats and otr_ngram_estimate, additions only;
 * 608: otr_mwer_workspace_floats and otr_mwer_loss, additions only; still 608: otr_feature_prepare_workspace_bytes, otr_feature_prepare and
 * otr_cmvn_accumulate, after them otr_ctc_segment_workspace_bytes and otr_ctc_segment, and after those otr_distill_workspace_floats and otr_distill_loss (additions only), after those otr_bias_score_cands and otr_bias_score_seqs (additions only), and otr_ctc_beam_search_bias (an addition only), after them otr_edit_align and otr_nbest_consensus (additions only), after them otr_mixspeech_mix and otr_ctc_loss_pair (additions only), after them otr_ctc_mwer_workspace_floats and otr_ctc_mwer_loss (additions only), after them the otr_rnnt_* entries, and last otr_rnnt_beam_joint, otr_rnnt_beam_select and otr_rnnt_beam_gather (additions only), were added without a bump -- no existing signature, structure or meaning changed, and a binding that needs them
 * fails on the missing symbol of an older library when it loads it).  A binding compares otr_version() with the OTR_ABI_VERSION it was written against BEFORE its first call and refuses a
 * library that answers anything else: descriptors are passed by pointer and read at the library's idea of their size. */
#define OTR_ABI_VERSION 608
int32_t otr_version(void);
/* OTR_BF16 or OTR_F16: the 16-bit type this library was built for */
int32_t otr_half_type(void);
/* tuning hook for benchmarks and tests' reference paths: key 0 = force GEMM tile (0 auto / 64 / 128), key 1 = force split-K (0 auto),
 * key 6 = 0/1: 256-wide weight-gradient launch off / on (-1: environment OTR_WGRAD256), key 7 = its workgroup count (0 = one per CU),
 * key 11 = bound of every in-kernel turnstile / arrival spin (<= 0: the default 2^22; tests force a give-up with 1), key 12 = 1: the
 * split FFN kernels exchange their partial sums with write-through stores / memory-served loads only (the path a row block split across
 * XCDs takes), key 13 = 1: attention backward as two launches (dQ, then dK/dV) instead of one, key 15 = workgroup mapping of the split
 * FFN kernels (1, the default: an XCD owns one weight slice; 0: the four slices of a row block share an XCD), key 16 = workgroup mapping
 * of the attention launches (1, the default: the blocks of one (head, utterance) on one XCD; 0: the plain 3-D grid), key 21 = 0: the
 * streamed attention backward instead of csrc/encattn.hip, key 22 = conv2 forward on the weight-stationary kernel (1) or the implicit
 * GEMM (0), key 23 = utterances per workgroup of the fused decoder launches (0 = the library's choice), key 24 / 25 = forms of the cached
 * decode self-attention / the beam top-k (25 = 2: the arg-max rounds), key 29 = 0: conv2's weight gradient of a 256-channel frontend on
 * the transposing GEMM instead of the gathered-row form of wgrad256.hip, key 30 = 0: no sliced parity-class input gradient for 256
 * output channels, key 31 = 0: otr_conv2_dgrad_wide answers "not served", key 33 = 0: the streamed dQ + dK/dV pair instead of
 * csrc/encattn96.hip.  Any other key is refused (returns -1). */
int32_t otr_debug_set(int32_t key, int32_t value);
/* Register the caller-owned, zero-initialised DEVICE word that spin-bounded kernels (the turnstile of the 256-wide
 * weight-gradient launch; NULL = none) add 1 to whenever a wait gives up -- the results of such a launch may be wrong sums.
 * otr_optimizer_step reads and clears it: a non-zero count skips the update exactly like a non-finite gradient norm and is
 * accumulated in state[10].  Process-wide like the compute type; the pointer is baked into captured graphs, so register it
 * before capturing and keep the word alive.  Replaces nothing in the reference (train/trainer.py:229 only guards NaNs). */
int32_t otr_set_fault_counter(void* device_word);
/* hardware probe used by the tests of the 256-wide weight-gradient kernel: one wave copies image[2048] (16-bit words)
 * to LDS and issues ONE ds_read_b64_tr_b16 with lane l at byte address addr[l]; out[l*4 + j] = element j lane l got. */
int32_t otr_debug_trread(const void* image, const int32_t* addr, void* out, void* stream);
/* tuning hook: when buf != NULL every GEMM workgroup writes 4 shader-clock timestamps (start, operands staged,
 * k-loop done, stores issued) to buf[(blockIdx.y*gridDim.x + blockIdx.x)*4 ..]; otr_conv2_dgrad writes, per workgroup, the 100 MHz
 * real time at start / operand fragments built / end and its parity class; NULL disables.  Not for production. */
int32_t otr_debug_trace(void* buf);
const char* otr_last_error_string(void);

/* ---- nn.Linear and its gradients (module/attention.py:43,68,128-129; module/ffn.py:39-41;
 *      frontend/conv.py:146; decoder/transformer.py:181; model/ctc.py:47).
 * All matrices row-major with leading dimensions in elements.  `accumulate` != 0 adds into out.
 * workspace (fp32, caller owned, may be NULL): enables split-K for contraction-heavy / output-small
 * shapes; partial [M,N] slabs are reduced in a FIXED order by a second kernel, so results stay
 * deterministic.  64 MiB covers every shape of the AISHELL configs. */
typedef struct {
  int32_t M, N, K;              /* y[M,N] = x[M,K] * w[N,K]^T */
  int32_t x_dtype, w_dtype, y_dtype, compute;
  int64_t ldx, ldw, ldy;
  int32_t act;                  /* OTR_ACT_* applied after bias (forward only) */
  int32_t accumulate;
} otr_linear_desc_t;
/* y = act(x w^T + bias); bias f32[N] or NULL */
int32_t otr_linear_fwd(const otr_linear_desc_t* d, const void* x, const void* w, const float* bias, void* y,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* dx[M,K] (dtype x_dtype, ld ldx) = dy[M,N] (dtype y_dtype, ld ldy) * w[N,K] */
/* otr_linear_fwd_batched: nbatch products of ONE shape in one launch, y_b = x_b w_b^T with x_b = x + b*bsx, w_b = w + b*bsw,
 * y_b = y + b*bsy (ELEMENT strides): the per-head products of module/attention.py:217-253 (MultiHeadedSelfAttentionWithRelPos:
 * (q+v) p^T per head, and its input gradient).  No bias, activation, accumulation or split-K.  Returns 1 WITHOUT launching when
 * the operands do not qualify (fp32 compute, unaligned rows / strides, operand types other than 16-bit x 16-bit -> f32 and
 * f32 x 16-bit -> 16-bit): the caller then loops over otr_linear_fwd. */
int32_t otr_linear_fwd_batched(const otr_linear_desc_t* d, const void* x, const void* w, void* y, int32_t nbatch, int64_t bsx, int64_t bsw,
                               int64_t bsy, void* stream);
int32_t otr_linear_dgrad(const otr_linear_desc_t* d, const void* dy, const void* w, void* dx, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* dw[N,K] (dtype w_dtype, ld ldw) = dy[M,N]^T * x[M,K] */
int32_t otr_linear_wgrad(const otr_linear_desc_t* d, const void* dy, const void* x, void* dw, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* out[N] (f32) (+)= sum over M rows of a[M,N]  (bias gradients) */
int32_t otr_colsum(const void* a, int32_t dtype, int64_t M, int64_t N, int64_t lda, float* out, int32_t accumulate,
                   void* stream);

/* ---- FFN forward through w_1 and the GLU in ONE launch (module/ffn.py:38-40): t[M,2F] = x[M,d] . w1[2F,d]^T + b1,
 *      u[M,F] = t[:, :F] * sigmoid(t[:, F:]); h[M,2F] = (t[:, :F] | sigmoid(t[:, F:])) is kept for backward (the
 *      sigmoid is computed once; otr_ffn_glu_bwd / otr_glu_bwd take it with h_has_sigmoid = 1).  Each GEMM tile holds 64 value columns and their 64 gate
 *      columns, so the GLU runs in the epilogue on data that is already on chip.  bf16 operands and outputs.
 *      Returns 1 without launching anything when the operands do not qualify; use otr_linear_fwd + otr_glu_fwd then. */
int32_t otr_ffn_glu_fwd(const void* x, int64_t ldx, const void* w1, int64_t ldw, const float* b1, void* h, void* u, int32_t M,
                        int32_t F, int32_t d_model, void* stream);
/* ---- FFN backward through w_2 and the GLU in ONE launch (module/ffn.py:38-41 backward): du = dy[M,d] . w2 (w2t = the
 *      [F,d] transposed bf16 shadow of w_2; du is never stored), dh[M,2F] = GLU'(h) * du with h[M,2F] the saved GLU
 *      input (h_has_sigmoid != 0: its second half already holds sigmoid(gate), as otr_ffn_glu_fwd writes it), and
 *      dbias_partial[rows, 2F] = column sums of dh per row tile (column-sum them for the w_1 bias gradient;
 *      *partial_rows receives the number of rows written, <= partial_rows_cap, size it ceil(M/64)).  bf16 operands.
 *      Returns 1 without launching anything when the operands do not qualify (alignment); use otr_linear_dgrad +
 *      otr_glu_bwd then. */
int32_t otr_ffn_glu_bwd(const void* dy, int32_t dy_dtype, int64_t ldy, const void* w2t, int64_t ldw, const void* h,
                        int32_t h_has_sigmoid, void* dh, float* dbias_partial, int32_t partial_rows_cap,
                        int32_t* partial_rows, int32_t M, int32_t F, int32_t d_model, void* stream);

/* ---- row-block fused FFN sub-layer of the post-norm layers (encoder/transformer.py:58-63, decoder/transformer.py:82-86,
 *      module/ffn.py:38-41 with activation 'glu'; SURVEY.md K7 + K8), d_model = 256, d_ff % 256 == 0, 16-bit operands.
 *      A workgroup owns 32 rows and streams the PACKED weights (otr_pack_frags) from L2 into registers; the d_ff-wide
 *      hidden lives in MFMA accumulators only.
 * otr_pack_frags: fragment-major copies of 16-bit matrices, many per launch.  table: DEVICE int64 [n_items][8] rows of
 *   {src element offset, row stride, col stride, rows (%32), cols (%16), perm, dst element offset, first block}; item i
 *   views src+offset as A[r][c] = src[r*rs + c*cs] (r = output index, c = contraction index) and writes one 1 KiB MFMA
 *   A-operand per (32 rows, 16 contraction indices) in (row tile, k-step) order; perm = 1 orders the contraction
 *   indices the way an accumulator tile presents them when it is fed back as an operand.  A block packs 4 fragments;
 *   total_blocks = sum of ceil(rows/32 * cols/16 / 4).
 * otr_ffn_ln_fwd:  y = LayerNorm(x + dropout(w_2(glu(w_1 x + b_1)) + b_2)) in ONE launch.  x f32 [M,256] and its 16-bit
 *   twin x16; w1_pack = pack(w_1 [2F,256] as A[f][k], perm 0); w2_pack = pack(w_2 [256,F] as A[n][f], perm 1).
 *   Outputs as otr_add_layernorm_fwd: y, y16 (may be NULL), z = x + dropout(branch) (may be NULL), mean, rstd; the
 *   dropout mask is the one otr_add_layernorm_bwd regenerates from (seed, rng_offset).
 * otr_ffn_bwd:  recomputes the pre-activations from x16, then dh[M,2F] = GLU'(.) * (dy16 . w_2), u[M,F] = glu(.)
 *   (row-major, the operands of the two weight gradients) and dx[M,256] f32 = skip + dh . w_1 in ONE launch.
 *   w2t_pack = pack(w_2 as A[f][n], perm 0); w1t_pack = pack(w_1 as A[k][f'], perm 1); skip may be NULL or alias dx.
 *   db1_part f32 [ceil(M/32)][2F]: column sums of dh per 32-row block (column-sum them for the w_1 bias gradient; the
 *   reduction over each block's rows happens on the accumulator registers, dh is not read again). */
int32_t otr_pack_frags(const void* src, void* dst, const int64_t* table, int32_t n_items, int64_t total_blocks,
                       void* stream);
int32_t otr_ffn_ln_fwd(const float* x, const void* x16, const void* w1_pack, const float* b1, const void* w2_pack,
                       const float* b2, const float* gamma, const float* beta, const uint64_t* seed, float p_drop,
                       uint64_t rng_offset, float eps, float* y, void* y16, float* z, float* mean, float* rstd, int64_t M,
                       int32_t F, int32_t d_model, void* stream);
int32_t otr_ffn_bwd(const void* x16, const void* dy16, const void* w1_pack, const float* b1, const void* w2t_pack,
                    const void* w1t_pack, void* dh, void* u, float* db1_part, const float* skip, float* dx, int64_t M,
                    int32_t F, int32_t d_model, void* stream);

/* ---- row-block projections of the attention sub-layers (module/attention.py:62-75 qvk_proj / output_proj, :120-140 q_proj /
 *      output_proj with the residual + LayerNorm of encoder/transformer.py:47-56, decoder/transformer.py:58-80), d_model = 256,
 *      16-bit operands.  Same structure as the fused FFN: 32 rows per workgroup, packed weights (otr_pack_frags, perm 0)
 *      streamed from L2, whole-row epilogues.
 * otr_rb_linear:  out[M,N] = x16[M,K] . W^T (+ bias) (+ skip), (N,K) in {(256,256), (768,256), (256,768)}; w_pack =
 *   pack(W as A[n][k]); for an input gradient pass dy16 as x16 and pack(W as A[k][n]) (rows = K inputs).  out f32 or 16-bit.
 * otr_proj_ln_fwd:  y = LayerNorm(x + dropout(c16 . W^T + bias)); outputs as otr_add_layernorm_fwd (y16, z may be NULL).
 * otr_ln_bwd_proj:  the LayerNorm backward of that sub-layer -- dx[M,256] f32 (may be NULL), da16 = dropout-masked gradient
 *   of the projection output (16-bit, the weight-gradient operand; may be NULL), partial f32
 *   [otr_ln_bwd_proj_partial_rows(M)][3][256] = per-workgroup sums of dgamma | dbeta | da (may be NULL) -- followed in
 *   the same launch by dc16 = da . W (16-bit, row stride ldc).  wt_pack = pack(W as A[k][n]). */
int32_t otr_rb_linear(const void* x16, int64_t ldx, const void* w_pack, const float* bias, const float* skip, int64_t lds,
                      void* out, int32_t out_dtype, int64_t ldo, int64_t M, int32_t N, int32_t K, void* stream);
int32_t otr_proj_ln_fwd(const float* x, const void* c16, int64_t ldc, const void* w_pack, const float* bias, const float* gamma,
                        const float* beta, const uint64_t* seed, float* y, void* y16, float* z, float* mean, float* rstd,
                        int64_t M, int32_t d_model, float eps, float p_drop, uint64_t rng_offset, void* stream);
int64_t otr_ln_bwd_proj_partial_rows(int64_t M);
/* otr_rb_linear_ln_bwd:  the input gradient of a projection whose INPUT is the output of a LayerNorm y = LN(z), z = x + dropout(a)
 *   (layer l's q|k|v projection reads layer l-1's FFN sub-layer: encoder/transformer.py:47-63), followed in the same launch by
 *   that LayerNorm's backward: dy = skip + g16[M,K] . W stays on chip; dx = d z f32 [M,256], da16 = dropout-masked branch
 *   gradient, partial as otr_ln_bwd_proj ([otr_ln_bwd_proj_partial_rows(M)][3][256]).  wt_pack = pack(W as A[k][n]); N = 256,
 *   K in {256, 768}. */
int32_t otr_rb_linear_ln_bwd(const void* g16, int64_t ldg, const void* wt_pack, const float* skip, int64_t lds, const float* z,
                             const float* mean, const float* rstd, const float* gamma, const uint64_t* seed, float p_drop,
                             uint64_t rng_offset, float* dx, void* da16, float* partial, int64_t M, int32_t N, int32_t K,
                             void* stream);
/* The same with a PREFETCH range: while the epilogue runs every workgroup touches its share of [prefetch, prefetch + prefetch_bytes)
 * (one dword per 64 bytes, no consumer) so that the NEXT launch finds those lines in the memory-side cache -- used for the two
 * input-gradient packs of the split FFN's backward launch that follows this one in the backward pass (3 MB it would otherwise
 * fetch from HBM in scattered 1 KiB pieces).  prefetch may be NULL (then exactly otr_rb_linear_ln_bwd). */
/* Ranges the NEXT otr_ln_bwd_proj / otr_ln_bwd_proj_slabs call of the calling thread has its kernel touch the same way (then the hint
 * is forgotten): the saved q|k|v and context the attention backward launch that follows it would otherwise fetch cold. */
/* Read [p, p + bytes) once and consume nothing: the lines are then in the memory-side cache for the launches that follow (the fused
 * decoder's packed weights, touched once before the stack's forward pass). */
int32_t otr_touch(const void* p, int64_t bytes, void* stream);
/* The start of a training step in one launch: buf[0..n) = 0 (the flat gradient buffer; f32, 16-byte aligned) and, when counter is not
 * NULL, counter[0] += inc (the device-resident dropout seed, advanced once per step so that forward and backward of one step draw
 * the same masks).  Replaces a fill launch + an 8-byte add launch (train/trainer.py:206-208 optimizer.zero_grad()). */
int32_t otr_zero_tick(float* buf, int64_t n, int64_t* counter, int64_t inc, void* stream);
int32_t otr_touch_hint(const void* p0, int64_t bytes0, const void* p1, int64_t bytes1);
int32_t otr_rb_linear_ln_bwd_pf(const void* g16, int64_t ldg, const void* wt_pack, const float* skip, int64_t lds, const float* z,
                                const float* mean, const float* rstd, const float* gamma, const uint64_t* seed, float p_drop,
                                uint64_t rng_offset, float* dx, void* da16, float* partial, int64_t M, int32_t N, int32_t K,
                                const void* prefetch, int64_t prefetch_bytes, void* stream);
int32_t otr_ln_bwd_proj(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma,
                        const uint64_t* seed, const void* wt_pack, float* dx, void* da16, void* dc16, int64_t ldc,
                        float* partial, int64_t M, int32_t d_model, float p_drop, uint64_t rng_offset, void* stream);

/* ---- the same sub-layer on 128-row workgroups (csrc/ffn3.hip): a workgroup owns 128 rows x 1/4 of the hidden units, the
 *      packed weights reach it ONCE through an LDS-DMA ring shared by its four waves (64 rows per wave, activations in the
 *      accumulator half of the register file), and the four workgroups of a row block exchange their fp32 partial sums
 *      through `scratch` (write-through stores, one arrival counter per row block in `sync`) and finish a quarter of the rows
 *      each.  d_ff % 256 == 0, d_model 256.
 *      scratch: >= otr_ffn_split_scratch_bytes(M) bytes, contents don't care; sync: >= otr_ffn_split_sync_ints(M) ints, ZERO
 *      before the first call and owned by these kernels afterwards (monotonic arrival counters: launches on one buffer must
 *      be stream-ordered).  The arrival wait is bounded (otr_debug_set(11, v)); a
 *      give-up is reported through otr_set_fault_counter and leaves wrong rows behind.  Needs the four workgroups of a row
 *      block co-resident: any grid on an otherwise idle GPU (they sit next to each other in dispatch order).
 * otr_ffn_ln_fwd_split: y = LayerNorm(x + dropout(w_2 glu(w_1 x + b_1) + b_2)), outputs as otr_ffn_ln_fwd.  With hsave / usave
 *      (both or neither) the pass also leaves what otr_ffn_bwd_split needs instead of recomputing it: hsave
 *      [otr_ffn_split_hsave_bytes(M, F) bytes] = (value + bias, sigmoid(gate)) of every hidden unit, 16-bit, in accumulator-tile
 *      order (opaque); usave [otr_ffn_split_padded_rows(M), F] 16-bit row-major = the glu output (operand of the w_2 weight
 *      gradient; rows past M are scratch).
 * otr_ffn_bwd_split: dh [otr_ffn_split_padded_rows(M), 2F] 16-bit row-major = GLU'(saved tiles, dy . w_2) (operand of the w_1
 *      weight gradient; its column sums are the w_1 bias gradient); dx = skip (or 0) + dh . w_1, f32 [M, 256], may alias skip. */
int64_t otr_ffn_split_scratch_bytes(int64_t M);
int64_t otr_ffn_split_sync_ints(int64_t M);
int64_t otr_ffn_split_hsave_bytes(int64_t M, int32_t F);
int64_t otr_ffn_split_padded_rows(int64_t M);
int32_t otr_ffn_ln_fwd_split(const float* x, const void* x16, const void* w1_pack, const float* b1, const void* w2_pack,
                             const float* b2, const float* gamma, const float* beta, const uint64_t* seed, float p_drop,
                             uint64_t rng_offset, float eps, float* y, void* y16, float* z, float* mean, float* rstd,
                             void* hsave, void* usave, void* scratch, int64_t scratch_bytes, int32_t* sync, int64_t sync_ints,
                             int64_t M, int32_t F, int32_t d_model, void* stream);
int32_t otr_ffn_bwd_split(const void* dy16, const void* hsave, const void* w2t_pack, const void* w1t_pack, void* dh,
                          const float* skip, float* dx, void* scratch, int64_t scratch_bytes, int32_t* sync, int64_t sync_ints,
                          int64_t M, int32_t F, int32_t d_model, void* stream);
/* ---- the same split FFN kernels in SLAB mode: no partial-sum exchange, no LayerNorm inside the launch.  The four hidden slices of
 *      a row block leave their shares as 16-bit slabs [4][M][256] and the launch that reads the sub-layer's output finishes
 *      y = LayerNorm(x + dropout(sum of slabs + b_2))  in its prologue (the in-launch exchange is a chain of far round trips: a third
 *      of the forward kernel's cycles; a launch boundary is cheaper).
 * otr_ffn_fwd_split_slab:  slabs = w_2[:, slice] glu(w_1[slice] x + b_1[slice]); hsave / usave as otr_ffn_ln_fwd_split.
 * otr_rb_linear_ln:        the q|k|v projection of the NEXT layer with that LayerNorm in its prologue: out[M,768] = y16 . W^T + bias,
 *      y and the LayerNorm's saved z / mean / rstd written on the way (otr_dec_ln_t, nslab <= 4).
 * otr_dec_ln (declared with the fused decoder below) is the LayerNorm alone, for an output nobody projects (the last encoder layer).
 * otr_ffn_bwd_split_slab:  dh as otr_ffn_bwd_split; slabs = the slices' shares dh[slice] . w_1[slice] of the input gradient.
 * otr_ln_bwd_proj_slabs:   otr_ln_bwd_proj with the LayerNorm's output gradient given as dskip f32 [M,256] + nslab (<= 4) such slabs. */
int32_t otr_ffn_fwd_split_slab(const void* x16, const void* w1_pack, const float* b1, const void* w2_pack, void* hsave, void* usave,
                               void* slabs, int64_t M, int32_t F, int32_t d_model, void* stream);
int32_t otr_ffn_bwd_split_slab(const void* dy16, const void* hsave, const void* w2t_pack, const void* w1t_pack, void* dh, void* slabs,
                               int64_t M, int32_t F, int32_t d_model, void* stream);
int32_t otr_ln_bwd_proj_slabs(const float* dskip, const void* slabs, int32_t nslab, const float* z, const float* mean, const float* rstd,
                              const float* gamma, const uint64_t* seed, const void* wt_pack, float* dx, void* da16, void* dc16, int64_t ldc,
                              float* partial, int64_t M, int32_t d_model, float p_drop, uint64_t rng_offset, void* stream);
/* ---- grouped weight / bias gradients: every dw_i[N,K] += dy_i[M,N]^T x_i[M,K] of a backward pass in a few launches
 *      (one per operand-type group), likewise every bias gradient out_i[N] += column sums of a_i[M,N].  The per-layer
 *      launches they replace are latency bound (a 4-k-step GEMM workgroup lives ~10 us, every launch costs 2-3 us);
 *      grouped, the long-contraction tiles of all layers fill the chip at once, so no split-K, no workspace, no
 *      reduce kernels.  Items that miss the alignment rules of the fast loaders run through otr_linear_wgrad
 *      (accumulate) with the workspace given here.  Results are always ACCUMULATED. */
typedef struct {
  const void* dy;
  const void* x;
  float* dw;
  int32_t M, N, K;
  int64_t ldy, ldx, ldw;
  int32_t dy_dtype, x_dtype;
  float* dbias;          /* NULL, or [N]: dbias += column sums of dy (the bias gradient of the same Linear), folded into the
                          * 256-wide launch -- allowed only on items for which otr_wgrad256_takes() returns 1 */
  int32_t overwrite;     /* != 0: the caller guarantees that dw holds ZEROS which nothing else has written in this backward pass (a
                          * gradient buffer cleared at the start of the step, this item its only writer): the 256-wide launch then
                          * STORES the first partial sum of every tile instead of reading the zeros back (7 % of that launch's
                          * bytes).  The result is the same sum; other paths ignore the flag and accumulate. */
} otr_wgrad_item_t;
/* 1 when otr_linear_wgrad_grouped would run this item on the 256-wide kernel (csrc/wgrad256.hip), else 0 */
int32_t otr_wgrad256_takes(const otr_wgrad_item_t* item, int32_t compute);
/* the schedule the 256-wide launch would use for these items (host only; tests replay the kernel's work decoding on it):
 * out[0..7] = {mode (1 rounds / 0 stream-K), grid, chunk, full rounds, tiles left, row ranges per left tile, total slabs, n},
 * out[8 + i] = first slab of problem i; grid_cap as otr_debug_set(7, v) */
/* host-only views of two launch geometries, for tests (no device work): the (row block, slice) of every workgroup of the split FFN
 * kernels under mapping `map` (otr_debug_set(15, .)) -- out[2 b], out[2 b + 1], returns the grid size (out may be NULL) -- and the
 * (block, head, utterance) of every workgroup of the XCD-aware attention grid (-1 for padding workgroups), out[3 i ..] */
int32_t otr_debug_ffn_split_map(int64_t M, int32_t map, int32_t* out, int32_t cap);
int32_t otr_debug_attention_grid(int32_t nx, int32_t H, int32_t B, int32_t* out, int32_t cap);
int32_t otr_debug_wgrad256_plan(const otr_wgrad_item_t* items, int32_t n, int32_t grid_cap, int32_t* out);
/* number of pieces of the last 256-wide launch on `workspace` that gave up waiting for their turn (bounded spin; 0 in any
 * healthy run; < 0 on error).  Synchronises the device. */
int32_t otr_debug_wgrad256_errors(const void* workspace);
int32_t otr_linear_wgrad_grouped(const otr_wgrad_item_t* items, int32_t n, int32_t compute, void* workspace,
                                 int64_t workspace_bytes, void* stream);
typedef struct {
  const void* a;
  float* out;
  int64_t M, N, lda;
  int32_t dtype;
} otr_colsum_item_t;
int32_t otr_colsum_grouped(const otr_colsum_item_t* items, int32_t n, void* stream);

/* ---- scaled-dot-product attention, flash style: scores are never materialised
 *      (module/attention.py:23-46 compute_context, :76-82 self, :137-143 cross).
 * q/k/v/o are [B, T, H*dk] slices addressed by (batch stride, time stride) in elements; head h
 * occupies columns [h*dk, (h+1)*dk).  key_mask: uint8 [B, Tk] (1 = valid) or NULL; causal != 0
 * additionally masks key > query (decoder/utils.py:7-11).  lse: f32 [B,H,Tq] (saved for bwd), the natural-log sum of exp(S) over
 * the keys a query may see.
 * A query row that may see NO key (every key of its utterance masked; torch's softmax gives NaN there): o = 0 and lse = -inf, and in
 * the backward pass the row contributes nothing -- its dq row is 0, delta is 0, and it adds nothing to dk, dv or dbias.  A masked key
 * gets dk = dv = 0 and every masked in-range (query, key) pair dbias = 0, written, not skipped.  Operands need no alignment: base
 * pointers off a 16-byte boundary or strides that are no multiple of 16 bytes take scalar loads and stores.  Batch strides may exceed
 * T * (time stride); nothing outside the [B, T, H*dk] elements of o / dq / dk / dv is written. */
typedef struct {
  int32_t B, H, Tq, Tk, dk;
  int32_t dtype;                /* element type of q,k,v,o and their grads; also the MFMA type */
  int64_t q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts;
  int32_t causal;
  float scale;                  /* 1/sqrt(dk) */
} otr_attn_desc_t;
int32_t otr_attention_fwd(const otr_attn_desc_t* d, const void* q, const void* k, const void* v,
                          const uint8_t* key_mask, void* o, float* lse, void* stream);
/* do_/dq/dk/dv use the strides of o/q/k/v.  delta: f32 [B,H,Tq] workspace: the streamed kernels leave rowsum(dO * O) in all of it.
 * The whole-utterance kernels keep that sum in LDS and need not write the workspace; a caller must not read it after a launch they
 * may have served: 16-bit operands on 16-byte boundaries, Tq == Tk <= 512 and no causal mask, at head dim 64 without a bias
 * (csrc/encattn.hip; otr_debug_set(21, 0) turns it off) and, in otr_attention_bias_bwd, at head dim 96 with rel_shift and bias rows long
 * enough for 16-byte loads (csrc/encattn96.hip; otr_debug_set(33, 0)).  Every other launch writes all of delta. */
int32_t otr_attention_bwd(const otr_attn_desc_t* d, const void* q, const void* k, const void* v,
                          const uint8_t* key_mask, const void* o, const void* do_, const float* lse,
                          float* delta, void* dq, void* dk, void* dv, void* stream);

/* Variant with an additive fp32 score bias, S = (q.k + bias[b,h,i,col]) * scale, addressed as
 * bias[b*bias_bs + h*bias_hs + i*bias_rs + col], col = j, or col = j - i + Tq - 1 when rel_shift != 0: the
 * Transformer-XL relative-position term of MultiHeadedSelfAttentionWithRelPos (module/attention.py:196-253; the
 * reference materialises [B,h,T,2T-1] and gathers it at :209-215).  dbias (same addressing, caller pre-zeroed when
 * rel_shift) receives d loss / d bias, in f32 or (r06, dbias_dtype) in the library's 16-bit type: the band tensor of one Conformer block is
 * 64 MB in f32, written once and read by two GEMMs. */
int32_t otr_attention_bias_fwd(const otr_attn_desc_t* d, const void* q, const void* k, const void* v,
                               const uint8_t* key_mask, const float* bias, int64_t bias_bs, int64_t bias_hs,
                               int64_t bias_rs, int32_t rel_shift, void* o, float* lse, void* stream);
int32_t otr_attention_bias_bwd(const otr_attn_desc_t* d, const void* q, const void* k, const void* v,
                               const uint8_t* key_mask, const float* bias, void* dbias, int32_t dbias_dtype, int64_t bias_bs,
                               int64_t bias_hs, int64_t bias_rs, int32_t rel_shift, const void* o, const void* do_,
                               const float* lse, float* delta, void* dq, void* dk, void* dv, void* stream);

/* ---- y = LayerNorm(x + dropout(a)) (encoder/transformer.py:54-56,61-63; decoder/transformer.py:
 *      66-68,76-78,84-86).  x f32 [M,d]; a [M,d] of a_dtype or NULL; z (= x+drop(a), f32) and
 *      mean/rstd (f32 [M]) are saved for backward.  Dropout masks come from a counter RNG keyed by
 *      (*seed, rng_offset + element index) and are regenerated, never stored. */
typedef struct {
  int64_t M;
  int32_t d;
  int32_t a_dtype;
  float eps, p_drop;            /* p_drop = 0 -> no dropout */
  uint64_t rng_offset;
  float a_scale;                /* r05: y = LN(x + a_scale * dropout(a)), da = a_scale * dropout'(dz); 0 means 1 (older callers) */
  const uint8_t* a_row_mask;    /* r05: [M] or NULL; rows with 0 take no branch: a row := 0 forward, da row := 0 backward (the
                                 * masked_fill of module/conformer.py:109 folded into the residual add that consumes the branch).
                                 * A fill, not a multiply: `a` of a masked row is not read, whatever it holds (NaN, Inf) stays out
                                 * of z, y and the statistics, and da of a masked row or a dropped element is exactly 0 */
  int32_t dy_dtype;             /* r06, backward entries: OTR_F32 (0) or the library's 16-bit type -- the LayerNorm's output fed a 16-bit
                                 * reader only (a Linear), whose input gradient then comes back in that type (half the bytes of the
                                 * input-gradient GEMM's output); forward entries may pass y = NULL then and write the 16-bit twin alone */
} otr_ln_desc_t;
/* y_bf16 (may be NULL): bf16 copy of y, the GEMM-operand form of the residual stream */
int32_t otr_add_layernorm_fwd(const otr_ln_desc_t* d, const float* x, const void* a, const float* gamma,
                              const float* beta, const uint64_t* seed, float* y, void* y_bf16, float* z, float* mean,
                              float* rstd, void* stream);
/* dx f32 [M,d] (residual grad), da [M,d] a_dtype (branch grad, may be NULL), dgamma/dbeta f32[d] +=.
 * da_colsum (f32[d] +=, may be NULL): column sums of da, i.e. the bias gradient of the Linear that produced the
 * branch (module/attention.py:43 output_proj, module/ffn.py:41 w_2) without a separate reduction launch. */
int32_t otr_add_layernorm_bwd(const otr_ln_desc_t* d, const float* dy, const float* z, const float* mean,
                              const float* rstd, const float* gamma, const uint64_t* seed, float* dx, void* da,
                              float* dgamma, float* dbeta, float* da_colsum, float* partial, void* stream);
/* partial (may be NULL): f32 [otr_add_layernorm_bwd_partial_rows(M), 3, d].  When given, NOTHING is added to dgamma / dbeta /
 * da_colsum (they may be NULL); each workgroup writes its own sums (dgamma | dbeta | da column sums) to its row and the
 * caller column-sums the rows (otr_colsum / otr_colsum_grouped): no atomics, deterministic.  With da == NULL there are no da column
 * sums: segment 2 ([.., 2, d], and columns [2d, 3d) of the 5 d / 7 d forms below) is NOT written and keeps what it held -- do not sum it. */
int64_t otr_add_layernorm_bwd_partial_rows(int64_t M);
/* the same with dx = skip + (gradient w.r.t. the LayerNorm input), skip f32 [M,d] or NULL: a pre-norm residual
 * x + f(LN(x)) (encoder/conformer.py:50-73; normalize_before layers) hands x two gradients, and this saves the elementwise
 * add autograd would launch to join them.  skip may alias dx.  With a branch (da != NULL) the skip gradient is part of the
 * gradient of the sum x + a_scale * dropout(a): da = a_scale * dropout'(skip + LayerNorm input gradient) (r05, ops.ResidualLnFn). */
int32_t otr_add_layernorm_bwd_skip(const otr_ln_desc_t* d, const float* dy, const float* z, const float* mean,
                                   const float* rstd, const float* gamma, const uint64_t* seed, const float* skip, float* dx,
                                   void* da, float* dgamma, float* dbeta, float* da_colsum, float* partial, void* stream);

/* Two LayerNorms back to back, y2 = LN2(LN1(x + a_scale * dropout(a))) -- encoder/conformer.py:87-89 (post_ffn_norm, then final_norm, on
 * the result of the convolution branch's residual add) -- in one launch each way (r05).  Forward writes y2 (+ 16-bit twin), the pre-norm
 * sum z and both LayerNorms' row statistics; backward takes d y2, recomputes y1 = LN1(z) from z / mean / rstd, and leaves
 * partial f32 [otr_add_layernorm_bwd_partial_rows(M)][5 d] = per-workgroup sums of dgamma | dbeta | da | dgamma2 | dbeta2 (the
 * caller column-sums them).  skip / dx / da as otr_add_layernorm_bwd_skip.  d y2 is f32: otr_add_layernorm2_bwd and
 * otr_add_layernorm3_bwd refuse a descriptor whose dy_dtype is not OTR_F32 (only d y3 may be 16-bit, by dy3_dtype). */
int32_t otr_add_layernorm2_fwd(const otr_ln_desc_t* d, const float* x, const void* a, const float* gamma, const float* beta,
                               const float* gamma2, const float* beta2, const uint64_t* seed, float* y2, void* y2_bf16, float* z,
                               float* mean, float* rstd, float* mean2, float* rstd2, void* stream);
int32_t otr_add_layernorm2_bwd(const otr_ln_desc_t* d, const float* dy2, const float* z, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, const float* mean2, const float* rstd2, const float* gamma2,
                               const uint64_t* seed, const float* skip, float* dx, void* da, float* partial, void* stream);
/* Three LayerNorms back to back (r06): y2 = LN2(LN1(x + a_scale * dropout(a))) as above AND y3 = LN3(y2) -- final_norm of a Conformer block
 * is followed by the NEXT block's macaron_ffn_norm (encoder/conformer.py:89, :50), whose output only feeds a Linear: y3 (NULL: not written)
 * and its 16-bit twin.  Backward takes d y2 AND d y3 (autograd hands the node both; d y3 in f32 or in the library's 16-bit type, dy3_dtype:
 * a 16-bit consumer's input gradient comes back in that type), recomputes y1 and y2 from z and the saved statistics,
 * and leaves partial f32 [rows][7 d] = dgamma | dbeta | da | dgamma2 | dbeta2 | dgamma3 | dbeta3. */
int32_t otr_add_layernorm3_fwd(const otr_ln_desc_t* d, const float* x, const void* a, const float* gamma, const float* beta,
                               const float* gamma2, const float* beta2, const float* gamma3, const float* beta3, const uint64_t* seed,
                               float* y2, float* y3, void* y3_bf16, float* z, float* mean, float* rstd, float* mean2, float* rstd2,
                               float* mean3, float* rstd3, void* stream);
int32_t otr_add_layernorm3_bwd(const otr_ln_desc_t* d, const float* dy2, const void* dy3, int32_t dy3_dtype, const float* z, const float* mean,
                               const float* rstd, const float* gamma, const float* beta, const float* mean2, const float* rstd2,
                               const float* gamma2, const float* beta2, const float* mean3, const float* rstd3, const float* gamma3,
                               const uint64_t* seed, const float* skip, float* dx, void* da, float* partial, void* stream);

/* ---- F.glu / F.relu on the FFN hidden (module/ffn.py:15-21,40): u[M,F] = h[:, :F]*sigmoid(h[:, F:]) */
/* row_mask (uint8 [M], may be NULL): rows with mask 0 produce u = 0 / dh = 0 (module/conformer.py:46) */
int32_t otr_glu_fwd(const void* h, void* u, int32_t dtype, int64_t M, int64_t F, const uint8_t* row_mask, void* stream);
/* dh[M,2F] from du[M,F]; if dbias_partial != NULL it receives per-row-block partial column sums of dh,
 * f32 [ceil(M/32), 2F] (deterministic; column-sum them with otr_colsum to get the w_1 bias gradient) */
int32_t otr_glu_bwd(const void* h, const void* du, void* dh, float* dbias, int32_t dtype, int64_t M, int64_t F,
                    const uint8_t* row_mask, int32_t h_has_sigmoid, void* stream);

/* ---- PositionalEncoding (module/pos.py:30-57): y = x*scale + PE[t], t = row % T.
 *      x may alias y. */
int32_t otr_posenc_fwd(const float* x, float* y, void* y_bf16, int64_t rows, int32_t T, int32_t d, float scale,
                       void* stream);
/* the same launch also casts the encoder's key mask: mask_out[r] (uint8 [rows]) = mask_in[(r / T) * mask_bs + (r % T) * mask_ts] != 0,
 * mask_in = the bytes of a bool / uint8 mask read through its strides (the frame mask behind the two stride-2 convolutions is a
 * strided view, frontend/conv.py:78-83); both NULL = otr_posenc_fwd.  d % 4 == 0, x / y 16-byte aligned. */
int32_t otr_posenc_mask_fwd(const float* x, float* y, void* y_bf16, int64_t rows, int32_t T, int32_t d, float scale,
                            const uint8_t* mask_in, int64_t mask_bs, int64_t mask_ts, uint8_t* mask_out, void* stream);
/* decoder embedding + posenc (decoder/transformer.py:163-169): y[r,:] = E[tok[r],:]*scale + PE[r % L] */
int32_t otr_embed_posenc_fwd(const int64_t* tok, const float* E, float* y, void* y_bf16, int64_t rows, int32_t L,
                             int32_t d, int32_t vocab, float scale, void* stream);
/* dE[tok[r],:] += scale * dy[r,:]  (atomic f32) */
int32_t otr_embed_bwd(const int64_t* tok, const float* dy, float* dE, int64_t rows, int32_t d, int32_t vocab,
                      float scale, void* stream);
/* The two above on a token VIEW: tok is addressed as tok[(r / L) * ld_tok + r % L] (`truth[:, :-1]` of the [B, L + 1] target matrix,
 * model/speech2text.py:53: no copy).  otr_embed_bwd_ld also takes the gradient as partial sums: dE[tok[r],:] += scale * (dy[r,:] +
 * sum_s slabs[s][r,:]) with dy f32 [rows, d] or NULL and slabs 16-bit [nslab][rows][d] or NULL (what otr_dec_self_bwd leaves). */
int32_t otr_embed_posenc_fwd_ld(const int64_t* tok, int64_t ld_tok, const float* E, float* y, void* y_bf16, int64_t rows, int32_t L,
                                int32_t d, int32_t vocab, float scale, void* stream);
int32_t otr_embed_bwd_ld(const int64_t* tok, int64_t ld_tok, int32_t L, const float* dy, const void* slabs, int32_t nslab, float* dE,
                         int64_t rows, int32_t d, int32_t vocab, float scale, void* stream);
/* dst (bf16) = src (f32), n elements: bf16 shadows of weights / activations */
int32_t otr_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* y = x * (*s_dev) * s_host, elementwise f32 (n elements); x may alias y; s_dev may be NULL */
int32_t otr_scale(const float* x, float* y, int64_t n, const float* s_dev, float s_host, void* stream);
/* y16 (the library's 16-bit type) = x * s, n elements; x 16-byte, y16 8-byte aligned.  The positional encoding's backward
 * (module/pos.py:44-57) when its gradient goes on as a GEMM operand. */
int32_t otr_scale_cast(const float* x, void* y16, int64_t n, float s, void* stream);

/* ---- Conv2d-subsampling frontend (frontend/conv.py:50-83 Conv2dLayer, :131-153 ConvFrontEnd).
 *      Activations are channel-last: act1 [B,T1,F1,C1], act2 [B,T2,F2,C2] == [B*T2, F2*C2] rows
 *      (the flatten of conv.py:145 becomes a column permutation of output_layer.weight). */
typedef struct {
  int32_t B, T, F;              /* input fbank [B,T,F] f32 */
  int32_t C1, C2;               /* mid / out channels */
  int32_t T1, F1, T2, F2;       /* derived: T1=(T-3)/2+1, F1=(F-1)/2+1, ... */
  int32_t act_dtype, compute;
  int32_t w_dtype;              /* dtype of w2r as passed (f32 master or its bf16 shadow) */
} otr_conv_desc_t;
/* conv1: 1->C1, 3x3, stride 2, pad (0,1), +bias, ReLU.  w1 f32 [C1,1,3,3] */
int32_t otr_conv1_fwd(const otr_conv_desc_t* d, const float* x, const float* w1, const float* b1, void* act1,
                      void* stream);
/* dw1 [C1,9] f32 +=, db1 [C1] f32 += ; dact1 already masked by ReLU.  partial (may be NULL): f32
 * [otr_conv1_wgrad_partial_rows()][10*C1]; when given NOTHING is added to dw1 / db1 (they may be NULL): every workgroup
 * writes its own sums (9*C1 weight-gradient values in dw1's layout, then C1 bias-gradient values) and the caller
 * column-sums the rows (otr_colsum / otr_colsum_grouped): no atomics, deterministic, 4x the workgroups. */
int32_t otr_conv1_wgrad(const otr_conv_desc_t* d, const float* x, const void* dact1, float* dw1, float* db1,
                        float* partial, void* stream);
int32_t otr_conv1_wgrad_partial_rows(void);
/* conv2 as implicit GEMM on MFMA: w2r = w2 permuted to [C2,3,3,C1] (f32). +bias, ReLU */
int32_t otr_conv2_fwd(const otr_conv_desc_t* d, const void* act1, const void* w2r, const float* b2, void* act2,
                      void* stream);
/* Both Conv2dLayers of frontend/conv.py:141-142 in ONE launch (csrc/conv2fwd.hip): conv2 on a weight-stationary kernel whose input
 * rows are computed from the filterbank frames in place (conv1's arithmetic, bit for bit); act1 is written for the backward pass.
 * 16-bit activations and w2r, (C1, C2) = (64, 128), F1 = 40 or 20.  Returns 1 without launching anything when the operands do not
 * qualify: call otr_conv1_fwd + otr_conv2_fwd then.  otr_debug_set(22, 0 | 1 | 2): 0 = the generic paths, 2 = conv2 alone on the new kernel. */
int32_t otr_conv12_fwd(const otr_conv_desc_t* d, const float* x, const float* w1, const float* b1, void* act1, const void* w2r,
                       const float* b2, void* act2, void* stream);
/* dcol[B*T2*F2, 9*C1] (act dtype) = dact2 * w2r  (dact2 already masked by ReLU) */
int32_t otr_conv2_dgrad_cols(const otr_conv_desc_t* d, const void* dact2, const void* w2r, void* dcol,
                             void* stream);
/* dact1 = col2im(dcol) * (act1 > 0) */
int32_t otr_conv2_col2im(const otr_conv_desc_t* d, const void* dcol, const void* act1, void* dact1, void* stream);
/* The two above in ONE launch, implicitly (no column matrix): dact1 = [act1 > 0] * conv2's input gradient of dact2.  The
 * stride-2 output pixels fall into four parity classes with 4 / 2 / 2 / 1 taps; each is a GEMM whose B operand is read
 * straight from dact2's channel rows (csrc/conv.hip).  16-bit operands, (C1, C2) = (64, 128) or (32, 64).
 * Returns 1 without launching anything when the operands do not qualify: use otr_conv2_dgrad_cols + otr_conv2_col2im then. */
int32_t otr_conv2_dgrad(const otr_conv_desc_t* d, const void* dact2, const void* w2r, const void* act1, void* dact1,
                        void* stream);
/* r06 (ABI 601) -- the input gradient of a WIDE frontend, C1 == C2 == 256 (conformer_baseline.yaml; frontend/conv.py:50-83): the parity
 * classes as an implicit GEMM whose weights stream through LDS in MFMA-fragment order, all 256 channels of a pixel per workgroup
 * (csrc/conv2wide.hip); the ReLU mask of act1 is fused.  `scratch` (>= otr_conv2_wide_scratch_bytes(), 16-byte aligned) receives the
 * re-ordered weights on the launch's stream.  16-bit activations and weights.
 * Returns 1 without launching anything when the operands do not qualify: use otr_conv2_dgrad (or its column-matrix form). */
int64_t otr_conv2_wide_scratch_bytes(void);
int32_t otr_conv2_dgrad_wide(const otr_conv_desc_t* d, const void* dact2, const void* w2r, const void* act1, void* dact1, void* scratch,
                             int64_t scratch_bytes, void* stream);
/* host-side plan of that launch, no device work (tests): out[10] = {served 0/1, first workgroup of the parity classes
 * c = 2*(t1&1) + (f1&1) and the total (5 values), 256-pixel tiles per class (4 values)} */
int32_t otr_debug_conv2_dgrad_plan(const otr_conv_desc_t* d, int32_t* out);
/* dw2r [C2, 9*C1] f32 = dact2^T * im2col(act1) */
int32_t otr_conv2_wgrad(const otr_conv_desc_t* d, const void* dact2, const void* act1, float* dw2r, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* g = g * (y > 0) elementwise (ReLU backward through a stored post-ReLU activation); g may alias out */
int32_t otr_relu_bwd(const void* y, const void* g, void* out, int32_t dtype, int64_t n, void* stream);
/* The same over a [rows, cols] matrix plus the bias gradient of the layer that produced y (column sums of out) in one pass:
 * partial [otr_relu_bwd_colsum_partial_rows(rows, cols, dtype)][cols] f32 receives per-workgroup sums (no atomics) for the
 * caller's column sum.  The second Conv2dLayer of frontend/conv.py:63-66 (relu then bias, C2 channels) is the user.
 * partial_rows returns 0 when the shape is not served (cols must be a multiple of the 16-byte vector, cols / vector dividing 256). */
int32_t otr_relu_bwd_colsum_partial_rows(int64_t rows, int32_t cols, int32_t dtype);
int32_t otr_relu_bwd_colsum(const void* y, const void* g, void* out, float* partial, int32_t dtype, int64_t rows, int32_t cols,
                            void* stream);

/* The other FFN activations of module/ffn.py:15-21 (relu runs in the GEMM epilogue, glu has otr_glu_* / otr_ffn_glu_*):
 * kind 1 = gelu (erf form, F.gelu's default), 2 = tanh, 3 = swish (x * sigmoid(x)).  y = act(x);  dx = dy * act'(x) from
 * the saved pre-activation x.  f32 or bf16, n elements, 16-byte aligned buffers; dx may alias dy. */
int32_t otr_act_fwd(const void* x, void* y, int32_t dtype, int64_t n, int32_t kind, void* stream);
int32_t otr_act_bwd(const void* x, const void* dy, void* dx, int32_t dtype, int64_t n, int32_t kind, void* stream);

/* ---- LabelSmoothingLoss (module/loss.py:21-48): logits f32 [R,V], target int64 [R].
 *      loss (f32 scalar) = sum_nonpad KL(conf || softmax) / #nonpad ; dlogits = d loss / d logits.
 *      scratch: f32[R+2] workspace (per-row losses are reduced in a fixed order: deterministic). */
int32_t otr_label_smoothing_loss(const float* logits, const int64_t* target, int64_t R, int32_t V, float smoothing,
                                 int32_t pad_idx, float* loss, float* dlogits, float* scratch, void* stream);
/* The same on rows longer than V (leading dimensions ld_logits, ld_dlogits >= V, in elements): the logits of an output layer
 * whose width is not a multiple of 8 (decoder/transformer.py:153, 4234 tokens) arrive as the head of a [R, V8] product and the
 * gradient leaves the same way, its columns V .. ld_dlogits-1 written as zeros, so that the layer's backward GEMMs read aligned
 * rows at the padded width. */
int32_t otr_label_smoothing_loss_ld(const float* logits, int64_t ld_logits, const int64_t* target, int64_t R, int32_t V,
                                    float smoothing, int32_t pad_idx, float* loss, float* dlogits, int64_t ld_dlogits,
                                    float* scratch, void* stream);

/* The whole loss in ONE launch, for the training step (module/loss.py:21-48 + the two scalar multiplications around it): every row
 * is read once (16-byte loads: logits and dlogits rows 16-byte aligned, ld % 4 == 0, V <= 8192, R <= 8192), the block that finishes
 * last adds up the row losses in the fixed order of otr_label_smoothing_loss (deterministic), and dlogits leaves already multiplied
 * by the device scalar *grad_scale (NULL = 1: the factor the caller's backward pass will be seeded with, e.g. the dynamic loss
 * scale of otr_optimizer_step's state block).  target: int64, addressed as target[(r / L) * ld_target + r % L] for r in [0, R): a
 * [B, L] view with row stride ld_target (model/speech2text.py:57 `truth[:, 1:]`) needs no copy; R % L == 0.
 * dlogits_dtype OTR_F32, or OTR_H16: the gradient in the library's 16-bit type (ld_dlogits % 8 == 0) -- the operand type of the output
 * layer's three backward GEMMs.  scratch: f32[R+2]; ticket: one uint32 the caller zero-initialises ONCE (the launch leaves it at
 * zero again). */
int32_t otr_label_smoothing_loss_fused(const float* logits, int64_t ld_logits, const int64_t* target, int64_t ld_target, int32_t L,
                                       int64_t R, int32_t V, float smoothing, int32_t pad_idx, const float* grad_scale, float* loss,
                                       void* dlogits, int32_t dlogits_dtype, int64_t ld_dlogits, float* scratch, uint32_t* ticket,
                                       void* stream);

/* ---- log_softmax over the last dim, f32 [R,V] (model/ctc.py:51,66; decoder/transformer.py:206) */
int32_t otr_log_softmax(const float* x, float* y, int64_t R, int32_t V, void* stream);

/* ---- Conformer encoder pieces (BASELINE configs[3]; encoder/conformer.py:20-114, module/conformer.py:12-57,
 *      module/attention.py:176-253).  All [M = B*T, C] row-major, C % 4 == 0. */
/* y = x + scale * dropout(a)  (pre-norm residual branches, ffn_scale 0.5 for the macaron FFN) and its branch grad */
int32_t otr_residual_add_fwd(const float* x, const void* a, int32_t a_dtype, float* y, int64_t n, float scale,
                             float p_drop, const uint64_t* seed, uint64_t rng_offset, void* stream);
int32_t otr_residual_add_bwd(const float* dy, void* da, int32_t a_dtype, int64_t n, float scale, float p_drop,
                             const uint64_t* seed, uint64_t rng_offset, void* stream);
/* y = dropout(x): x * mask / (1 - p), mask from the counter RNG keyed by (*seed, rng_offset + element index); applied to dy
 * with the same (seed, offset) it is the backward pass.  nn.Dropout of module/attention.py:46 (projected context),
 * module/ffn.py:40 (hidden), frontend/conv.py:66, module/conformer.py (end of the convolution module).  n % 4 == 0. */
int32_t otr_dropout(const void* x, void* y, int32_t dtype, int64_t n, float p_drop, const uint64_t* seed,
                    uint64_t rng_offset, void* stream);
/* out[M, 2d] = [q + u | q + v] (pos_bias_u / pos_bias_v flattened to [d]); q has leading dimension ldq */
int32_t otr_head_bias_add(const void* q, int64_t ldq, const float* u, const float* v, void* out, int32_t dtype,
                          int64_t M, int32_t d, void* stream);
/* dst[r, c, f] += src[r, f, c] (fp32; dst [rows, C, F], src [rows, F, C], both dense); clear_src != 0 leaves src ZERO.  Regroups a
 * weight gradient produced in a kernel's column order into the parameter's layout in one launch: the frontend Linear's staging image
 * (frontend/conv.py:145-146: flatten c*F+f, kernel order f*C+c) and conv2's channel-last taps (frontend/conv.py:56).  Replaces
 * torch's strided add (AccumulateGrad / add_) in the step. */
int32_t otr_regroup_add(float* dst, float* src, int64_t rows, int32_t C, int32_t F, int32_t clear_src, void* stream);
/* out[r, :cols] = a[r, :cols] + b[r, :cols] with independent leading dimensions */
int32_t otr_add2_strided(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int32_t dtype,
                         int64_t M, int32_t cols, void* stream);
/* r06: the same sum with the column sums of a and of b left as per-workgroup partials, partial [otr_add2_colsum_partial_rows(M)][2 cols] f32
 * (a's sums, then b's): d(q+u) + d(q+v) -> the packed qkv gradient, and the gradients of pos_bias_u / pos_bias_v (module/attention.py:241-245)
 * without a second pass over the two operands. */
int64_t otr_add2_colsum_partial_rows(int64_t M);
int32_t otr_add2_strided_colsum(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int32_t dtype, int64_t M,
                                int32_t cols, float* partial, void* stream);
/* out = x where mask[row] else 0 (f32) */
int32_t otr_row_mask(const float* x, const uint8_t* mask, float* out, int64_t M, int32_t C, void* stream);
/* the same with a type change on the way (OTR_F32 / OTR_H16 either side): the Conformer convolution module hands its
 * branch to the residual add, and takes the gradient back, in the activation type (module/conformer.py:56) */
int32_t otr_row_mask_cast(const void* x, int32_t x_dtype, const uint8_t* mask, void* out, int32_t out_dtype, int64_t M,
                          int32_t C, void* stream);
/* depthwise Conv1d over time, channel-last, per utterance, zero padded:
 *   y[b,t,c] = bias[c] + sum_{j<k} w[c,j] * g[b, t + j - pad, c]          k <= 7, 0 <= pad < k
 * pad = (k-1)/2 is the Conformer's 'same' convolution (module/conformer.py:26-28); pad = 0 with k = lookahead_steps + 1 is
 * the CTC head's look-ahead convolution (model/ctc.py:17-24,35-39: right-padded, no bias).  y f32 [B,T,C]; stats f32 [2C]
 * (may be NULL) receives per-channel sum / sum of squares of y over all B*T rows (BatchNorm batch statistics) */
int32_t otr_dwconv_fwd(const void* g, int32_t dtype, const float* w, const float* bias, float* y, float* stats,
                       int32_t B, int32_t T, int32_t C, int32_t k, int32_t pad, void* stream);
/* dg (dtype), dw f32 [C,k] +=, db f32 [C] += (may be NULL) */
int32_t otr_dwconv_bwd(const float* dy, const void* g, int32_t dtype, const float* w, void* dg, float* dw, float* db,
                       int32_t B, int32_t T, int32_t C, int32_t k, int32_t pad, void* stream);
/* otr_dwconv_bwd_part: the same with the weight / bias gradient sums left PER WORKGROUP in part [otr_dwconv_bwd_partial_rows(B*T)][C*k + C]
 * (columns: dw as [C][k], then db) instead of atomic adds on dw / db: the caller column-sums them (otr_colsum_grouped at the end of the
 * backward pass): 249 workgroups x 2304 atomics on 2304 addresses were half of the launch at the bench batch. */
int64_t otr_dwconv_bwd_partial_rows(int64_t M);
int32_t otr_dwconv_bwd_part(const float* dy, const void* g, int32_t dtype, const float* w, void* dg, float* part, int32_t B, int32_t T,
                            int32_t C, int32_t k, int32_t pad, void* stream);
/* BatchNorm1d (training: batch statistics from `stats`, running stats updated in place; eval: running stats) fused
 * with swish; saved f32 [2C] = mean | rstd for backward */
int32_t otr_bn_swish_fwd(const float* y, const float* stats, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* saved, void* out, int32_t out_dtype, int64_t M, int32_t C, float eps,
                         float momentum, int32_t training, void* stream);
/* r05: the BatchNorm batch statistics without a zeroing launch and without atomics: otr_dwconv_fwd_part leaves the depthwise
 * convolution's per-workgroup sums in spart [otr_dwconv_fwd_partial_rows(B*T)][sum y (C) | sum y^2 (C)], otr_bn_swish_fwd_part adds
 * them up in its statistics launch (training mode; module/conformer.py:40-46,103-110). */
int64_t otr_dwconv_fwd_partial_rows(int64_t M);
int32_t otr_dwconv_fwd_part(const void* g, int32_t dtype, const float* w, const float* bias, float* y, float* spart, int32_t B, int32_t T,
                            int32_t C, int32_t k, int32_t pad, void* stream);
int32_t otr_bn_swish_fwd_part(const float* y, const float* spart, int32_t nblk, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float* saved, void* out, int32_t out_dtype, int64_t M, int32_t C, float eps,
                              float momentum, void* stream);
/* red f32 [2C]: on return d beta | d gamma of THIS call; dy f32 [M,C] = gradient w.r.t. the BatchNorm input.
 * partial: f32 scratch [otr_bn_swish_bwd_partial_rows(M)][2C] (per-strip sums: no atomics, deterministic).
 * dgamma_acc / dbeta_acc (f32 [C], may be NULL): the parameter gradients, += the same sums in the reduction launch. */
int32_t otr_bn_swish_bwd_partial_rows(int64_t M);
int32_t otr_bn_swish_bwd(const float* y, const void* ds, int32_t ds_dtype, const float* saved, const float* gamma,
                         const float* beta, float* red, float* partial, float* dgamma_acc, float* dbeta_acc, float* dy,
                         int64_t M, int32_t C, int32_t training, void* stream);
/* r06 (ABI 601): the middle of ConformerConvolutionModule's backward (module/conformer.py:36-57) as two steps instead of five launches.
 * otr_bn_swish_bwd_sums = the first two launches of otr_bn_swish_bwd (per-strip sums, their reduction into red [2C] and, when given, into
 * the BatchNorm parameter gradients); otr_conformer_conv_bwd_mid then does BatchNorm's apply step, the depthwise convolution's backward and
 * the GLU's backward in ONE launch: dh [M, 2C] from y, ds, red, g (the GLU output) and h (the GLU input).  The [M, C] fp32 dy and the
 * [M, C] dg tensors of the stand-alone chain are never written.  part [otr_dwconv_bwd_partial_rows(M)][C*k + C] and gpart [same rows][2C]
 * receive per-workgroup sums (no atomics): the depthwise conv's dw | db and the columns of dh (pointwise_conv1's bias gradient). */
int32_t otr_bn_swish_bwd_sums(const float* y, const void* ds, int32_t ds_dtype, const float* saved, const float* gamma, const float* beta,
                              float* red, float* partial, float* dgamma_acc, float* dbeta_acc, int64_t M, int32_t C, void* stream);
int32_t otr_conformer_conv_bwd_mid(const float* y, const void* ds, const float* saved, const float* gamma, const float* beta,
                                   const float* red, const void* g, const float* w, const void* h, const uint8_t* row_mask, void* dh,
                                   float* part, float* gpart, int32_t dtype, int32_t training, int32_t B, int32_t T, int32_t C, int32_t k,
                                   int32_t pad, void* stream);

/* ---- CTC loss with gradient w.r.t. the logits (nn.CTCLoss(blank, zero_infinity=True), reduction
 *      'mean', as built at model/ctc.py:30 and called at :50-53).  log_probs f32 [B,T,V] (already
 *      log-softmaxed), targets int64 [B, ldt], in_len/tgt_len int32 [B], max_tgt >= max(tgt_len) (<=127).
 *      alpha_ws: f32 [B, T, 2*max_tgt+1] workspace; nll: f32 [B] (0 where infeasible);
 *      loss: f32 scalar; dlogits f32 [B,T,V] or NULL. */
int32_t otr_ctc_loss(const float* log_probs, const int64_t* targets, int64_t ldt, const int32_t* in_len,
                     const int32_t* tgt_len, int32_t B, int32_t T, int32_t V, int32_t max_tgt, int32_t blank,
                     float* alpha_ws, float* nll, float* loss, float* dlogits, void* stream);

/* ---- MixSpeech on the device (otrans/train/trainer.py:155-201, Trainer(mixspeech=True)); csrc/mixspeech.hip and csrc/ctc.hip.
 * otr_mixspeech_mix: utterances 2p and 2p + 1 of a padded batch mixed frame by frame, P = B / 2 pairs (integer division: an odd last
 *   utterance takes no part, trainer.py:160).  x f32 [B, T, F], utterance b at x + b * pitch (pitch >= T * F floats); lengths int32 [B],
 *   clamped to [0, T]; lam a DEVICE f32 scalar, read by the kernel, never by the host.
 *   out f32 [P, T, F] (contiguous): out[p, t, :] = lam * x[2p, t, :] + (1 - lam) * x[2p + 1, t, :], where a frame t >= lengths[b] of an
 *   input utterance counts as 0.0f and is NOT read (the reference mixes the collate's zero padding: the same result, and padding that is
 *   not zero cannot leak in).  1 - lam is rounded to f32 once, each product is rounded, then the sum: bit for bit the float32 numpy /
 *   torch composition of trainer.py:172-173 (no fused multiply-add).
 *   out_lengths int32 [P] = max(lengths[2p], lengths[2p + 1]) after the clamp; out_mask uint8 [P, T] = 1 where t < out_lengths[p], the
 *   form otr_feature_prepare writes; frames at or past out_lengths[p] are written as exactly 0.0f.  EVERY cell of the three outputs is
 *   written (they may be uninitialised).
 *   One launch.  Loads and stores are 16 bytes wide where an utterance's base is 16-byte aligned (x[2p], x[2p + 1] and out[p] judged
 *   separately), scalar otherwise and in the tail of a live span.  Refused before the launch (< 0, outputs untouched): a NULL pointer;
 *   B < 2, B / 2 > 65535, T < 1, F < 1, T * F >= 2^31; pitch < T * F.  No allocation or host synchronisation: capturable.
 * otr_ctc_loss_pair: the CTC term of MixSpeech in one call.  log_probs f32 [P, T, V] and in_len int32 [P] are scored against two label
 *   sets: a = (targets_a int64 rows of stride ldt_a, tgt_len_a int32 [P]) with weight lam, b likewise with weight 1 - lam (lam a DEVICE
 *   f32 scalar).  The two sets may be the even and the odd rows of one [B, W] matrix (ldt = 2W): nothing is copied.  max_tgt, blank and
 *   the guards on in_len and tgt_len are those of otr_ctc_loss; in addition a label outside [0, V) makes its (utterance, set) infeasible.
 *   nll f32 [2, P]: row k what otr_ctc_loss writes for set k alone (0 where infeasible or guarded).
 *   loss3 f32 [3] = {lam * loss_a + (1 - lam) * loss_b, loss_a, loss_b}, loss_k = sum_p nll[k, p] / (P * max(L_kp, 1)): otr_ctc_loss's
 *   value for set k, here added in utterance order (no atomics).
 *   dlogits f32 [P, T, V] (NULL: losses only) = lam * g_a + (1 - lam) * g_b with g_k what otr_ctc_loss writes for set k alone.  An
 *   infeasible or guarded (utterance, set) adds nothing and leaves the other set's share of the slab intact; where both are, the slab
 *   is exactly zero, as are the frames at or past in_len.  A set whose weight is exactly 0 adds nothing whatever its labels are.
 *   alpha_ws: f32 [2, P, T, 2 * max_tgt + 1] workspace.  Launches: the two sets' alpha sweeps side by side; one dense pass over [P, T, V]
 *   (coefficient lam * ok_a * coef_a + (1 - lam) * ok_b * coef_b, known only after both sweeps; it also forms loss3); the two beta sweeps,
 *   whose occupancies are added onto the slab with fp32 atomics (as in otr_ctc_loss, their order is free).  With the caller's
 *   log-softmax that is ONE log-softmax and ONE dense pass where two otr_ctc_loss calls make two of each.
 *   Refused before any launch (< 0, outputs untouched): a NULL pointer other than dlogits; P outside [1, 65535], T < 1, V < 2; max_tgt
 *   outside [0, 127]; ldt_a or ldt_b below max_tgt; blank outside [0, V).  Capturable. */
int32_t otr_mixspeech_mix(const float* x, int64_t pitch, const int32_t* lengths, const float* lam, int32_t B, int32_t T, int32_t F,
                          float* out, int32_t* out_lengths, uint8_t* out_mask, void* stream);
int32_t otr_ctc_loss_pair(const float* log_probs, const int64_t* targets_a, int64_t ldt_a, const int32_t* tgt_len_a,
                          const int64_t* targets_b, int64_t ldt_b, const int32_t* tgt_len_b, const int32_t* in_len, const float* lam,
                          int32_t P, int32_t T, int32_t V, int32_t max_tgt, int32_t blank, float* alpha_ws, float* nll, float* loss3,
                          float* dlogits, void* stream);

/* ---- minimum word error rate training of the CTC model (sequence-discriminative training on the n-best of the CTC prefix beam
 *      search), csrc/ctc.hip: otr_ctc_loss_pair generalised to N hypotheses per utterance plus, optionally, the reference, with a
 *      posterior step between the sweeps.  f32 in every build.  B utterances with N hypothesis slots each, slot (b, n).
 *   log_probs f32 [B, T, V] (already log-softmaxed); in_len int32 [B], clamped to [0, T] as in otr_ctc_loss; hyps int64 tokens, row
 *   (b, n) at hyps + (b*N + n)*ldh; hyp_len int32 [B, N]; errors int32 [B, N] (otr_edit_distance's dist; < 0: invalid).  ref int64 rows
 *   of stride ldr with ref_len int32 [B]: the reference labels of the interpolated CTC term, or all three NULL / 0: no CTC term.
 *   ctc_weight >= 0 and scale > 0 are host floats; gscale a DEVICE f32 scalar (NULL: 1) that rides in the written gradient, as
 *   otr_mwer_loss's grad_scale does; max_tgt <= 127 bounds hyp_len and ref_len as in otr_ctc_loss; blank is the blank index.
 *   ll_n = the CTC log-likelihood of hypothesis n, what -otr_ctc_loss's nll is for those labels.
 *   Slot (b, n) is LIVE iff errors >= 0, hyp_len lies in [0, max_tgt], every label inside hyp_len lies in [0, V) and an alignment
 *   exists (ll_n > -inf: in_len[b] > 0 and the labels, with a blank between equal neighbours, fit into the frames).  A hypothesis of
 *   length 0 is valid (one state, all blank).  Nothing behind hyp_len is read, nothing at all of a slot with errors < 0.
 *   Per utterance: P_n = softmax over the live n of scale * ll_n (max-subtracted), E_b = sum_n P_n W_n with W = errors.
 *   mwer = (1 / B_live) sum_b E_b, B_live = the number of utterances with at least one live slot; B_live = 0: mwer 0.
 *   ctc = otr_ctc_loss's value for (ref, ref_len): sum_b nll_ref[b] * coef_b, coef_b = 1 / (B * max(ref_len[b], 1)); 0 without ref.
 *   c_n = scale * P_n (W_n - E_b).  d E_b / d logits[t, v] = sum_n c_n (gamma_n[t, v] - softmax[t, v]) with gamma_n the occupancy of
 *   (t, v) under hypothesis n; sum_n c_n is identically zero, so the dense softmax term of the hypotheses cancels and the MWER gradient
 *   touches only the columns of the hypotheses' labels and of the blank.  A dense term survives only for the reference.
 * Outputs: loss3 f32 [3] = {mwer + ctc_weight * ctc, mwer, ctc}; seq_logp f32 [B, N] = ll_n, -inf where the slot is not live; post f32
 *   [B, N] = P, 0 where not live; utt_err f32 [B] = E_b (0 without a live slot); nll_ref f32 [B]: what otr_ctc_loss writes for the
 *   reference (0 where infeasible or guarded, and 0 throughout without ref).  The sums over the utterances go through one fixed tree,
 *   no atomics: these outputs have the same bits on every run.
 *   dlogits f32 [B, T, V] (NULL: forward only) = g * [ctc_weight * ok_ref * coef_b * (softmax - gamma_ref) + sum over the live n of
 *   (c_n / B_live) * gamma_n], g = *gscale.  EVERY cell is written by the call, no memset is needed: the dense pass writes
 *   g * ctc_weight * ok_ref * coef_b * exp(lp) on the frames below in_len and exact 0 elsewhere -- it does not read lp where that
 *   coefficient is 0 -- and the beta sweeps then add -wc * gamma onto the slab, wc = g * ctc_weight * coef_b for the reference and
 *   -g * c_n / B_live for a live slot.  A slot whose wc is exactly 0 returns before it touches anything: every slot at N = 1, where
 *   the loss is W and the gradient of the MWER term exactly zero.  The occupancies go on with fp32 atomics in free order, as in
 *   otr_ctc_loss: the gradient is not bit-reproducible.
 *   workspace: at least otr_ctc_mwer_workspace_floats(B, N, T, max_tgt) floats = the alpha tables [N + 1, B, T, 2*max_tgt + 1] and the
 *   weights wc [B, N + 1]; that entry runs on the host and answers -1 for a shape otr_ctc_mwer_loss refuses.
 * Launches: the alpha sweeps on a grid (B, N + 1) (N without ref), which leave ll; one workgroup over the B * N scalars (post, utt_err,
 *   loss3, wc); the dense or zero pass, in the chunks of otr_ctc_loss_pair's, 16 bytes per access where an utterance's base is 16-byte
 *   aligned (log_probs and dlogits judged separately) and scalar otherwise; the beta sweeps on the same grid.  Forward only: the first two.
 * Refused before any launch (< 0, outputs untouched): a NULL pointer other than ref / ref_len / gscale / dlogits; only some of ref,
 *   ldr (non-zero) and ref_len given; B outside [1, 65535], N outside [1, 32], T < 1, V < 2; max_tgt outside [0, 127]; ldh or (with
 *   ref) ldr below max_tgt; blank outside [0, V); ctc_weight < 0 or scale <= 0 or either not finite; a workspace smaller than
 *   otr_ctc_mwer_workspace_floats answers.  No allocation or host synchronisation: capturable. */
int64_t otr_ctc_mwer_workspace_floats(int32_t B, int32_t N, int32_t T, int32_t max_tgt);
int32_t otr_ctc_mwer_loss(const float* log_probs, const int32_t* in_len, const int64_t* hyps, int64_t ldh, const int32_t* hyp_len,
                          const int32_t* errors, const int64_t* ref, int64_t ldr, const int32_t* ref_len, float ctc_weight, float scale,
                          const float* gscale, int32_t B, int32_t N, int32_t T, int32_t V, int32_t max_tgt, int32_t blank, float* loss3,
                          float* seq_logp, float* post, float* utt_err, float* nll_ref, float* dlogits, float* workspace,
                          int64_t workspace_floats, void* stream);

/* ---- one optimizer update over a replica's FLAT buffers (train/trainer.py:221-234 clip_grad_norm_(5) + gradient noise +
 *      NaN guard + scheduler.step + optimizer.step; train/scheduler.py:129-138 Noam lr; torch Adam with
 *      L2 weight decay, train/scheduler.py:10-13).  grad_scale (1/world_size after the all-reduce-sum)
 *      is folded into clip + update.  state: f32[OTR_OPT_STATE_FLOATS = 528] device block, zero-initialised by the caller once;
 *      [16..527] is scratch (per-workgroup partial sums of the gradient norm, added up in a fixed order: the clip factor is
 *      bit-reproducible, so data-parallel replicas that hold identical all-reduced gradients stay identical):
 *        [0] step  [1] lr  [2] bc1  [3] bc2  [4] sqnorm  [5] skipped  [6] loss_scale  [7] good_steps  [8] unscale
 *        [9] growth_interval  [10] faults (give-ups reported through otr_set_fault_counter; each skipped its update)
 *        [11..15] reserved.
 *      Loss scaling (fp16 builds): when state[6] > 0 the gradients in `grad` are state[6] times too large (the caller
 *      seeded its backward pass with that device scalar); the update divides it out, HALVES it and skips the update when
 *      the gradient norm is not finite, and doubles it after state[9] consecutive finite updates (0 = never) -- all on
 *      the device, so the step stays hipGraph-replayable.  grad_noise_std > 0 adds N(0, std) to every gradient element
 *      after clipping (trainer.py:223-227; pass train.grad_noise / accum_steps) -- except where gradient AND parameter are
 *      exactly zero (padding cells of the flat buffers stay zero).  noam_warmup <= 0 selects base_lr.  All arguments are
 *      checked before the first launch: a refused call leaves the device state untouched. */
#define OTR_OPT_STATE_FLOATS 528
int32_t otr_optimizer_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                           float* state, int32_t state_floats /* floats the caller allocated for `state`: refused below OTR_OPT_STATE_FLOATS */,
                           void* param_bf16 /* NULL or 16-bit shadow[n] refreshed in the same pass */,
                           float base_lr, float beta1, float beta2, float eps, float weight_decay,
                           float grad_scale, float clip_norm, float noam_model_size, float noam_warmup,
                           float noam_factor, float noam_step_offset, float grad_noise_std, void* stream);

/* ---- gradient all-reduce over RCCL / xGMI (replaces nn.DataParallel's per-step scatter / replicate / gather /
 *      reduce-add, train/trainer.py:56-66).  One in-place sum over the replica's flat gradient buffer,
 *      issued on the stream passed in (the compute stream: nothing to synchronise before the optimizer).  librccl is
 *      opened lazily (dlopen); the communicator is the one object the library owns.
 *      Rendezvous: rank 0 calls otr_allreduce_unique_id, the HOST ships the 128 bytes to every rank, every rank (having
 *      selected its GPU with hipSetDevice) calls otr_allreduce_init; dtype is OTR_F32 / OTR_BF16 / OTR_F16 of `buf`. */
int32_t otr_allreduce_unique_id(void* id128);
int32_t otr_allreduce_init(void** handle, const void* id128, int32_t rank, int32_t world);
int32_t otr_allreduce_run(void* handle, void* buf, int64_t count, int32_t dtype, void* stream);
int32_t otr_allreduce_destroy(void* handle);

/* ---- batch beam search step (recognize/speech2text.py:95-192).
 * beam_topk: rows = batch*beam hypotheses; logits f32 [rows, V] (row stride ld) are the decoder logits of
 *   the last position; optional LM logits are fused as log_softmax(dec) + lm_weight*log_softmax(lm)
 *   (speech2text.py:102-105); writes the k best (score, token) per row, descending (:112).
 * beam_prune: finished-beam masking (:156-192), score update, top-k over beam^2 candidates, prefix
 *   gather + token append (:118-146).  preds_* int64 [batch*beam, ldp] hold t tokens on entry, t+1 on
 *   exit; n_finished (int32 device scalar) = number of hypotheses ending in EOS after the step. */
int32_t otr_beam_topk(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm, float lm_weight,
                      int64_t rows, int32_t V, int32_t k, float* out_score, int64_t* out_idx, void* stream);
int32_t otr_beam_prune(const float* k_score, const int64_t* k_idx, const float* scores_in, const uint8_t* flag_in,
                       const int64_t* preds_in, int64_t ldp, int32_t batch, int32_t beam, int32_t t, int32_t eos,
                       float* scores_out, uint8_t* flag_out, int64_t* preds_out, int32_t* n_finished, void* stream);

/* ---- CTC prefix beam search (CTCRecognizer mode='beam'; recognize/ctc.py:60-67 hands it to ctcdecode), csrc/ctcbeam.hip.  f32.
 * log_probs f32 [B, T, V]: frame (b, t) at log_probs + (b*T + t)*ld; lengths int32 [B] on the device, clamped to [0, T]; frames
 * t >= lengths[b] are not read.  Standard prefix beam search in log space: every prefix carries pb (paths ending in blank) and pnb
 * (ending in a non-blank); the empty prefix starts with pb = 0, pnb = -inf.  At frame t the candidates are the K tokens of highest
 * log-prob (ties -> lower token); blank takes part only if it is among them.  For prefix s with last token l and candidate c, log-prob p:
 *   c == blank:  pb'(s) += (pb(s) + pnb(s)) * p          (in log space: + is log-add-exp, * is +)
 *   c == l:      pnb'(s) += pnb(s) * p,  pnb'(s+c) += pb(s) * p
 *   other c:     pnb'(s+c) += (pb(s) + pnb(s)) * p
 * Equal strings reached from different parents merge.  The new beam is the W entries of highest pb' + pnb' (log-add-exp) that are
 * above -inf; ties go to the lower (parent slot, token), a prefix carried over from slot i counting as (i, -1).  After the last
 * frame the beam is in descending score order.  The score-threshold pruning of ctcdecode ("min_cutoff") is NOT applied.
 * Prefix identity inside the beam is (length, 64-bit hash): a false merge needs a hash collision between two of the <= W*(W+1)
 * pairs compared per frame, probability <= T*W*(W+1) / 2^64 per utterance.
 * otr_ctc_topk:        top_lp f32 / top_tok int32 [B*T, K] (rows of frames past lengths[b] are left untouched); V <= 8192,
 *   K <= min(128, V) (ctcdecode's cutoff_top_n is 40; 128 lets K = V for the vocabularies up to 128).
 * otr_ctc_beam_search: one launch, one workgroup per utterance; W <= 32.  workspace: otr_ctc_beam_workspace_bytes(B, T, W) bytes,
 *   8-byte aligned (the back-pointer trie, int32 {parent node, token} per (b, t, slot)); tokens int64 [B, W, T] padded with -1,
 *   out_len int32 [B, W], scores f32 [B, W] = log-probability of the prefix; slots past the live beam get score -inf, length 0.
 * otr_ctc_beam_workspace_bytes: pure host function, -1 for a bad shape. */
int64_t otr_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t W);
int32_t otr_ctc_topk(const float* log_probs, int64_t ld, const int32_t* lengths, int32_t B, int32_t T, int32_t V, int32_t K,
                     float* top_lp, int32_t* top_tok, void* stream);
int32_t otr_ctc_beam_search(const float* top_lp, const int32_t* top_tok, const int32_t* lengths, int32_t B, int32_t T, int32_t V,
                            int32_t K, int32_t blank, int32_t W, void* workspace, int64_t ws_bytes, int64_t* tokens,
                            int32_t* out_len, float* scores, void* stream);

/* ---- n-gram LM fusion for the CTC prefix beam search (the ngram_lm / alpha / beta that recognize/ctc.py:22-25 hands to
 *      ctcdecode.CTCBeamDecoder; character based, ctcdecode's is_character_based case), csrc/ngram.hip + csrc/ctcbeam.hip.  f32.
 * The model: a backoff n-gram of order N <= 5 over the acoustic model's units.  Ids [0, V) are the units, id V is <s>; V <= 8192, so
 * an id fits 16 bits.  Log-probs and backoff weights are natural logs in f32 (ARPA's log10 values converted once at load).
 * The table: `capacity` entries of 32 bytes, capacity a power of two, the base 32-byte aligned; open addressing with linear probing
 * from hash(key) & (capacity - 1), load <= 0.5, nothing ever deleted.  Entry = { u64 lo, u64 hi, f32 log-prob, f32 backoff, 8 bytes
 * of padding }.  The key of the n-gram w_0 .. w_{m-1} is exact, not a fingerprint: id w_{m-1-j} sits at bits [16j, 16j+16) of an
 * 80-bit value, lo = its bits 0-63, hi = its bits 64-79 | m << 16; hi == 0 marks an empty entry.  hash = the splitmix64 finaliser of
 * lo ^ (hi * 0x9e3779b97f4a7c15) (csrc/ngram.h ng_hash).  A lookup walks from the home entry until it meets the key, an empty entry,
 * or has read max_probe entries: max_probe is the longest chain of the build (opentransformer_amd/ngram.py records it).
 * Context: the context of a prefix s is <s> followed by s, cut to its last N-1 ids (ctcdecode's make_ngram: one <s>, no padding).
 * ln P(c | h), h of length L <= N-1: for k = L down to 0: if the n-gram (last k ids of h, c) is stored, the result is the backoffs
 *   accumulated so far plus its log-prob; otherwise the backoff of (last k ids of h) is added if that n-gram is stored (0 if not, and
 *   for k = 0) and the context is shortened.  The sum runs in f32, longest context first.  If c or any id of h has no unigram entry
 *   the result is oov_score (ctcdecode's OOV_SCORE is -1000.0), before alpha is applied.
 * otr_ngram_lookup: out f32 [n] = ln P(tok[q] | ctx row q).  ctx int32 [n, N-1]: row q holds its ctx_len[q] ids oldest first, left
 *   aligned (ctx_len clamped to [0, N-1]; ctx and ctx_len may be NULL when N = 1); tok int32 [n].  An id outside [0, V] gives
 *   oov_score.  One thread per query; every probe it can need is issued before any result is consumed.  n = 0: nothing to do.
 * Fusion (otr_ctc_beam_search_lm): every contribution to pnb'(s+c) in the recursion of otr_ctc_beam_search gains the addend
 *   a(s+c) = alpha * ln P(c | context(s)) + beta.  It depends on the new string only, so the extension from the parent and the merge
 *   of that extension into a string already in the beam add the same value.  Blank and repeat stays gain nothing.  With nothing
 *   pruned, score(s) = ln P_ctc(s) + alpha * ln P_LM(s) + beta * |s|.  Candidates, ranking, tie order, the per-slot cut and the
 *   outputs are those of otr_ctc_beam_search, whose arguments keep their meaning; the addend enters an extension's score before it
 *   is ranked.  New output lm_scores f32 [B, W]: the sum of the addends of the hypothesis (0 for the empty one and for slots past
 *   the live beam), so scores - lm_scores is the acoustic part.  alpha = beta = 0 gives otr_ctc_beam_search's outputs bit for bit.
 *   One launch, no allocation, no host synchronisation. */
int32_t otr_ngram_lookup(const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V, const int32_t* ctx,
                         const int32_t* ctx_len, const int32_t* tok, int64_t n, float oov_score, float* out, void* stream);
int32_t otr_ctc_beam_search_lm(const float* top_lp, const int32_t* top_tok, const int32_t* lengths, int32_t B, int32_t T, int32_t V,
                               int32_t K, int32_t blank, int32_t W, void* workspace, int64_t ws_bytes, int64_t* tokens,
                               int32_t* out_len, float* scores, const void* table, int64_t capacity, int32_t max_probe,
                               int32_t order, float alpha, float beta, float oov_score, float* lm_scores, void* stream);

/* ---- phrase biasing (hotwords) fused into the CTC prefix beam search (CTCRecognizer bias=..., and the first pass of
 *      SpeechToTextRecognizer rescore=True, bias_first_pass=True), csrc/ctcbeam.hip + csrc/bias.h.  f32 and integers only.
 * The phrase table, state, psi_minus, psi and the 16-token window are those of the phrase-biasing section below (otr_bias_score_cands);
 *   there is no EOS inside the search.  bias_table / bias_capacity / bias_max_probe / bias_max_len are checked as that section's
 *   entries check them (16-byte aligned, a power of two, max_probe in [1, capacity], max_len in [1, 16]).
 * otr_ctc_beam_search_bias: otr_ctc_beam_search (ngram_table == NULL: capacity .. oov_score are not looked at and lm_scores must be
 *   NULL) or otr_ctc_beam_search_lm (ngram_table given, its arguments checked as there, lm_scores required), and in either case every
 *   contribution to pnb'(s+c) gains the phrase addend a(s, c) = psi_minus(state(s c)) - psi(state(s)), ONE f32 subtraction, whether
 *   the extension creates s+c or merges into an s+c already in the beam.  Order of the f32 additions of an extension:
 *   ((acoustic + n-gram addend) + phrase addend); the merge adds (n-gram addend + phrase addend), formed once when the slot was made,
 *   to its acoustic term.  Blank and repeat stays gain nothing.  The blank is never emitted and never enters a state; a unit that is
 *   in no phrase leads to the root and refunds the open match (a negative addend).  Candidates, ranking, tie order and the per-slot
 *   cut are the plain search's; the addends enter an extension's score before it is ranked.
 *   After the last frame every live slot r loses psi(state(h_r)) -- an utterance that ends inside a phrase keeps no credit for it --
 *   from scores and from bias_scores, and the live slots are ranked again by the refunded score (descending, ties -> the earlier
 *   slot); tokens, out_len, scores, lm_scores and bias_scores are written in that order.  Hence bias_scores f32 [B, W] = the summed
 *   addends of h_r + EOS, the quantity otr_bias_score_seqs computes, whatever path the search took: bit for bit where the weights
 *   are dyadic (every sum exact), else within (len + 1) * 2^-24 * sum |a|.  0 for slots past the live beam.  scores - lm_scores -
 *   bias_scores is the acoustic part.  All weights 0 gives the outputs of otr_ctc_beam_search / otr_ctc_beam_search_lm bit for bit.
 *   The workspace is otr_ctc_beam_workspace_bytes, unchanged.  One launch, no allocation, no host synchronisation. */
int32_t otr_ctc_beam_search_bias(const float* top_lp, const int32_t* top_tok, const int32_t* lengths, int32_t B, int32_t T, int32_t V,
                                 int32_t K, int32_t blank, int32_t W, void* workspace, int64_t ws_bytes, int64_t* tokens,
                                 int32_t* out_len, float* scores, const void* ngram_table /* NULL = no n-gram */, int64_t capacity,
                                 int32_t max_probe, int32_t order, float alpha, float beta, float oov_score,
                                 float* lm_scores /* NULL iff no n-gram */, const void* bias_table, int64_t bias_capacity,
                                 int32_t bias_max_probe, int32_t bias_max_len, float* bias_scores, void* stream);

/* ---- CTC forced alignment (token time stamps from the CTC head: what ctcdecode's `timesteps`, dropped at recognize/ctc.py:64, gives
 *      for the decoded string), csrc/ctcalign.hip.  The most probable CTC path of a KNOWN label sequence.  f32 in both builds.
 * log_probs f32 [B, T, V]: frame (b, t) at log_probs + (b*T + t)*ld; in_len int32 [B] on the device, clamped to [0, T] (= T_b); frames
 * t >= T_b are not read.  targets int64 [B, ldt], tgt_len int32 [B]: L = tgt_len[b], 0 <= L <= max_tgt <= 127 (the limit of
 * otr_ctc_loss).  An utterance whose tgt_len is negative or above max_tgt, or one of whose L labels lies outside [0, V), is infeasible:
 * nothing of it is computed.
 * Extended states s = 0 .. 2L as in the loss: even s is blank, odd s is label s>>1 (= ext(s)).  With x_t(c) the log-prob of token c:
 *   v_0(0) = x_0(blank), v_0(1) = x_0(label 0), v_0(s) = -inf otherwise;
 *   v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if allowed) + x_t(ext(s)),  one f32 add after an exact max;
 *   the step from s-2 is allowed exactly as in the loss: ext(s) is a label and differs from ext(s-2).
 * Ties: among equal predecessors the smallest step wins (stay, then s-1, then s-2); at the end v_{T_b-1}(2L) wins a tie against
 * v_{T_b-1}(2L-1).  The path is the one these choices trace back from the end.
 * Outputs: score f32 [B] = the path's log-probability; frame_token int32 [B, T] = the token of the path's state at each frame (blank on
 * blank frames, -1 for t >= T_b); spans int32 [B, max_tgt, 2] = first frame and one-past-last frame at which label j's state is
 * occupied (-1, -1 for j >= L); label_logp f32 [B, max_tgt] = sum of x_t(label j) over that span, added in ascending t (0 for j >= L).
 * Infeasible (score -inf: T_b = 0 with L > 0, fewer frames than labels plus adjacent repeats, log-probs of -inf on every path, a bad
 * length or label): score = -inf, frame_token and spans all -1, label_logp all 0.  T_b = 0 with L = 0: score 0, the empty path.
 * One launch, one workgroup per utterance.  The 2-bit back-pointers (64 B per frame) stay in LDS while T <= 960 and go to `workspace`
 * above that: otr_ctc_align_workspace_bytes(B, T, max_tgt) bytes (8 where T <= 960, B*T*64 above), 8-byte aligned, never NULL.
 * Every argument is checked before the launch (null pointers, V <= 1, blank outside [0, V), ld < V, ldt < max_tgt, max_tgt > 127, the
 * workspace's size and alignment): a refused call leaves the outputs untouched.
 * otr_ctc_align_workspace_bytes: pure host function, -1 for a bad shape (B < 1, T < 1, max_tgt outside [0, 127]). */
int64_t otr_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t max_tgt);
int32_t otr_ctc_align(const float* log_probs, int64_t ld, const int64_t* targets, int64_t ldt, const int32_t* in_len,
                      const int32_t* tgt_len, int32_t B, int32_t T, int32_t V, int32_t max_tgt, int32_t blank, void* workspace,
                      int64_t ws_bytes, int32_t* frame_token, int32_t* spans, float* label_logp, float* score, void* stream);

/* ---- CTC segmentation of long recordings (Kuerzinger et al. 2020, the ctc-segmentation tool): where in minutes of audio a transcript
 *      of many utterances lies, csrc/ctcseg.hip.  otr_ctc_align's recursion for up to 4095 labels, with a path that need not cover the
 *      whole recording.  f32 in both builds.
 * log_probs, ld, in_len (T_b = clamp(in_len[b], 0, T); frames t >= T_b are not read), targets, ldt, tgt_len, the extended states
 * s = 0 .. 2L, ext(s) and x_t(c) as in otr_ctc_align, with 1 <= L = tgt_len[b] <= max_tgt <= 4095 and 1 <= T <= 2^20 (float(t) exact).
 * free_start, free_end: 0 or 1.  skip_logp: f32, finite and <= 0, charged once for every frame the path does not cover.
 *   Start: v_0(0) = x_0(blank), v_0(1) = x_0(l_0), -inf elsewhere; both carry back-pointer code 3, "the path starts here".
 *   t >= 1: the candidates, in tie order, are stay v_{t-1}(s); v_{t-1}(s-1); v_{t-1}(s-2) where otr_ctc_align allows it (ext(s) is a
 *   label and differs from ext(s-2)); for s in {0, 1} and only if free_start the virtual start float(t) * skip_logp (one f32 multiply
 *   of the exactly converted t), code 3.  A later candidate wins only if it is strictly greater.  v_t(s) = max + x_t(ext(s)): one f32
 *   add after an exact max.
 *   End: with free_end every frame t is a candidate, for s = 2L and then 2L-1: e = v_t(s) + tail, tail = float(T_b-1-t) * skip_logp for
 *   t < T_b-1 and exactly 0 at the last frame; otherwise only t = T_b-1 is.  The largest e wins; on ties the earliest t, then 2L
 *   before 2L-1.  The trace follows the codes back from there until it meets a code 3.
 * Outputs: score f32 [B] = the winning e; bounds int32 [B, 2] = the first covered frame and one past the last covered frame;
 * frame_token int32 [B, T] = the path's token on covered frames (blank on blank frames), -1 on skipped frames and for t >= T_b; spans
 * int32 [B, max_tgt, 2] and label_logp f32 [B, max_tgt] as in otr_ctc_align (sums in ascending t; rows j >= L hold -1 and 0).
 * Infeasible -- L < 1 or L > max_tgt (L = 0 too, unlike otr_ctc_align), a label outside [0, V), T_b = 0, no path of finite score --:
 * nothing is computed, score = -inf, bounds, frame_token and spans all -1, label_logp all 0; other recordings are unaffected.
 * With free_start = free_end = 0 and L <= 127 the outputs equal otr_ctc_align's and bounds = (0, T_b).
 * Why skip_logp: with skip_logp = 0 leaving a frame out costs nothing while covering it costs its log-prob, so the path shrinks its
 * first and last labels to one frame each.  With ln p(token) > skip_logp > ln p(blank on noise), e.g. ln 0.5, covering a frame the
 * label explains is cheaper than skipping it and skipping a frame of noise is cheaper than calling it blank.
 * One launch, one workgroup per recording (no waiting between workgroups), no allocation, no host synchronisation, legal under stream
 * capture.  workspace: otr_ctc_segment_workspace_bytes(B, T, max_tgt) bytes of 2-bit back-pointers, 8-byte aligned, never NULL; it need
 * not be zeroed.  Every argument is checked before the launch (null pointers; B < 1, T outside [1, 2^20], V <= 1, max_tgt outside
 * [1, 4095]; ld < V, ldt < max_tgt; blank outside [0, V); a flag other than 0 or 1; skip_logp positive, NaN or infinite; the
 * workspace's size and alignment): a refused call leaves every output untouched.
 * otr_ctc_segment_workspace_bytes: pure host function, -1 for a bad shape (B < 1, T outside [1, 2^20], max_tgt outside [1, 4095]). */
int64_t otr_ctc_segment_workspace_bytes(int32_t B, int32_t T, int32_t max_tgt);
int32_t otr_ctc_segment(const float* log_probs, int64_t ld, const int64_t* targets, int64_t ldt, const int32_t* in_len,
                        const int32_t* tgt_len, int32_t B, int32_t T, int32_t V, int32_t max_tgt, int32_t blank, int32_t free_start,
                        int32_t free_end, float skip_logp, void* workspace, int64_t ws_bytes, int32_t* frame_token, int32_t* spans,
                        float* label_logp, float* score, int32_t* bounds, void* stream);

/* ---- WER / CER scoring: batched edit distance with corpus totals (the editdistance.eval calls of eval.py:160-178 and
 *      tools/computer_wer.py), csrc/editdist.hip.  Integer only, identical in both builds.
 * Pair (b, n) scores hypothesis n of utterance b against reference b.  ref int64 [B, Lr], row b at ref + b*ref_bs, ref_len int32 [B];
 * hyp int64 [B, N, Lh], hypothesis (b, n) at hyp + b*hyp_bs + n*hyp_ns, hyp_len int32 [B, N] (contiguous); all on the device.
 * eos >= 0: a hypothesis ends before its first token equal to eos among its first hyp_len tokens; eos = -1: none.
 * Tokens are compared as integers.  Nothing at or beyond a length is ever read: the padding may hold anything.
 * D[i][j] is the textbook Levenshtein table with unit costs, i over the R reference tokens and j over the H hypothesis tokens:
 *   D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (ref[i-1] != hyp[j-1]), D[i-1][j] + 1, D[i][j-1] + 1);  dist = D[R][H].
 * counts = (substitutions, deletions, insertions) of ONE canonical alignment, defined recursively: cell (i, j) takes, among the
 *   predecessors that achieve D[i][j], the diagonal first (a match, or one substitution more), then the cell above (i-1, j) (one
 *   deletion more), then the cell to the left (i, j-1) (one insertion more); row 0 is all insertions, column 0 all deletions.
 *   S + D + I == dist always.
 * A ref_len outside [0, Lr] makes every pair of the utterance invalid, a hyp_len outside [0, Lh] that pair: dist = -1, counts = -1.
 * Outputs: dist int32 [B, N], counts int32 [B, N, 3], and totals int64 [8], ACCUMULATED into (the caller zeroes it once):
 *   {utterances, ref_tokens, errors_1best, S_1best, D_1best, I_1best, errors_oracle, bad}.  1-best is n = 0; oracle is the least dist
 *   over the valid n of the utterance.  An utterance enters the first seven only if its reference and its hypothesis 0 are valid,
 *   otherwise it adds 1 to `bad` and nothing else; invalid hypotheses n > 0 are left out of the oracle.
 * Limits, checked before the launch (a refused call returns < 0, launches nothing and leaves the outputs untouched): 1 <= N <= 32,
 *   0 <= Lr, Lh <= 2048, B >= 0 (B = 0 returns 0 without a launch), eos >= -1, strides >= 0, totals 8-byte aligned.
 * One launch (one workgroup per utterance, one wave per pair), no workspace, no allocation, no host synchronisation; capturable. */
int32_t otr_edit_distance(const int64_t* ref, int64_t ref_bs, const int32_t* ref_len, const int64_t* hyp, int64_t hyp_bs,
                          int64_t hyp_ns, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Lr, int32_t Lh, int32_t eos,
                          int32_t* dist, int32_t* counts, int64_t* totals, void* stream);

/* ---- per-token edit alignment, and the consensus of an n-best: token confidences and minimum Bayes risk (MBR) selection,
 *      csrc/nbest.hip.  Integer alignment, f32 sums in a fixed order, no 16-bit operand: identical in both builds and on every run.
 * otr_edit_align: the arguments, the eos cut and the validity rules of otr_edit_distance, widths 0 <= Lr, Lh <= OTR_NBEST_MAX_LEN.  The
 *   alignment is the canonical one of otr_edit_distance, walked back from (R, H): at (i, j) the diagonal if D[i-1][j-1] + (ref[i-1] !=
 *   hyp[j-1]) == D[i][j], else the cell above if D[i-1][j] + 1 == D[i][j] (a deletion), else the cell to the left (an insertion);
 *   row 0 is all insertions, column 0 all deletions.  Outputs: dist int32 [B, N] = D[R][H]; code int8 [B, N, Lh]: 0 a match, 1 a
 *   substitution, 2 an insertion for each of the H hypothesis tokens, -1 from H on; ref_pos int32 [B, N, Lh]: the index i-1 of the
 *   reference token a match or substitution is aligned to, -1 on insertions and from H on.  The codes' counts of 1s and 2s are
 *   otr_edit_distance's S and I, and D = R - (matches + substitutions).  An invalid pair gives dist -1 and -1 in all of code and
 *   ref_pos.  Every element of the three outputs is written.  One launch, one wave per pair, the 2-bit back-pointers of a pair (16 KB
 *   at 256 x 256) in LDS: no workspace.
 * otr_nbest_consensus: tokens int64 [B, N, L], hypothesis (b, n) at tokens + b*tok_bs + n*tok_ns; lengths int32 [B, N], scores f32
 *   [B, N] (both contiguous); eos as above; scale finite.  Slot (b, n) is LIVE if its score is finite and 0 <= lengths <= L.
 *   post f32 [B, N] = softmax over the live slots of scale * score (formed as exp(scale * (score - pivot)), the pivot the live slot of
 *     largest scale * score, summed with n ascending), 0 on dead slots;
 *   risk f32 [B, N]: risk[b,i] = sum over the live j, ascending, of post[b,j] * dist(hypothesis i against hypothesis j as the
 *     reference): the expected edit distance of i under the posterior; +inf on dead slots;
 *   conf f32 [B, N, L]: conf[b,i,k] = sum over the live j, ascending, of post[b,j] * [otr_edit_align's code of token k of i against
 *     j is 0]; j = i adds post[b,i].  0 from the hypothesis's end on and on dead slots;
 *   best int32 [B]: the live slot of least risk, ties to the higher score, then the lower index; -1 without a live slot.
 *   Every element of the four outputs is written.  Two launches (one workgroup per (b, i), one wave per pair, then the arg-min), no
 *   atomics, no workspace.
 * Both: checked before the launch (a refused call returns < 0, launches nothing, leaves the outputs untouched): 1 <= N <= 32, the
 *   widths, 0 <= B <= 2^20 (B = 0 returns 0 without a launch), eos >= -1, strides >= 0.  No allocation, no host synchronisation;
 *   capturable.  OTR_NBEST_MAX_LEN is what the back-pointers of one pair may take of a workgroup's 64 KB of LDS. */
#define OTR_NBEST_MAX_LEN 256
int32_t otr_edit_align(const int64_t* ref, int64_t ref_bs, const int32_t* ref_len, const int64_t* hyp, int64_t hyp_bs, int64_t hyp_ns,
                       const int32_t* hyp_len, int32_t B, int32_t N, int32_t Lr, int32_t Lh, int32_t eos, int32_t* dist, int8_t* code,
                       int32_t* ref_pos, void* stream);
int32_t otr_nbest_consensus(const int64_t* tokens, int64_t tok_bs, int64_t tok_ns, const int32_t* lengths, const float* scores,
                            float scale, int32_t B, int32_t N, int32_t L, int32_t eos, float* post, float* risk, int32_t* best,
                            float* conf, void* stream);

/* ---- joint CTC/attention beam search (SpeechToTextRecognizer joint_ctc=True; Watanabe et al. 2017, Algorithm 2; ESPnet's
 *      CTCPrefixScore), csrc/ctcscore.hip.  f32 in every build.  lambda = ctc_weight in [0, 1]; x_t(c) = log_probs of token c at frame
 *      t of the utterance, T_b = lengths[b] clamped to [1, T']; "+" of probabilities is log-add-exp, "*" is +.  BOS = EOS.
 * Prefix state: every hypothesis g carries r^n_t(g), r^b_t(g) for t < T_b and its prefix score psi(g).  The start prefix (BOS only):
 *   r^n = -inf, r^b_t = sum_{tau <= t} x_tau(blank), psi = 0; it has no last token.
 * Pre-beam (otr_joint_prebeam): per hypothesis the K' tokens of highest att_weight * log_softmax(att) + lm_weight * log_softmax(lm)
 *   (att_weight = 1 - lambda; lm_logits NULL: no LM term), descending, ties -> lower token.  The log-softmaxes are formed exactly as
 *   otr_beam_topk forms them.  cand_score f32 / cand_idx int32 [rows, K'].  V <= 8192, K' <= min(32, V).
 * Prefix score of h = g.c (otr_ctc_prefix_score), per candidate of an unfinished hypothesis:
 *   c == blank: psi(h) = -inf.   c == eos: psi(h) = r^n_{T_b-1}(g) + r^b_{T_b-1}(g).
 *   otherwise: phi_t = r^b_t(g) + (c == last(g) ? -inf : r^n_t(g));  r^n_0(h) = x_0(c) if g is the start prefix else -inf,
 *   r^b_0(h) = -inf;  for t = 1 .. T_b-1: r^n_t(h) = (r^n_{t-1}(h) + phi_{t-1}) * x_t(c), r^b_t(h) = (r^b_{t-1}(h) + r^n_{t-1}(h)) * x_t(blank);
 *   psi(h) = r^n_0(h) + sum_{t=1}^{T_b-1} phi_{t-1} * x_t(c).  Frames t >= T_b are never read.
 * Joint score (cand_score given): j = cand_score + lambda * (psi(h) - psi(g)); at lambda = 0 exactly cand_score (no CTC term, even where
 *   psi is -inf); for lambda > 0, -inf where psi(h) or psi(g) is -inf (never NaN).  Each hypothesis keeps the `beam` best of its K'
 *   candidates, descending, ties -> lower token, written in the layout otr_beam_prune reads: k_score f32 / k_idx int64 [rows, beam], plus
 *   k_src int32 [rows, beam] = row * K' + candidate (the candidate's state slot).  A finished hypothesis (flags[row] != 0) does not
 *   consult the CTC head: its k_score = -inf, k_idx = eos, k_src = -1 (the prune masks them).
 * Prefix of row r: preds int64 [rows, ldp], BOS at column 0; the prefix has t columns (t = *pos + 1 where pos is given, the cached
 *   search's device scalar; else the host t), last(g) = preds[r, t-1] when t > 1.  Hypothesis row r belongs to utterance
 *   r / rows_per_utt.  log_probs f32 [B, T', V], frame (b, t) at log_probs + (b*T' + t)*ld; lengths int32 [B] on the device.
 * State: slot s of a state buffer holds r^n / r^b f32 [slots, T'] (row s at s*T') and psi f32 [slots].  For t > 1 row r's parent state
 *   is slot jsrc[r] of (rn_in, rb_in, psi_in); the launch writes every candidate's state to slot r*K' + k of (rn_out, rb_out, psi_out)
 *   (rn_out / rb_out may both be NULL: psi only; frames t >= T_b are not written).  In and out buffers must differ (double-buffer them
 *   per ping-pong phase like preds).  Limits: T' <= 2048, K' <= min(32, V), beam <= min(16, K').
 * otr_beam_prune_joint / otr_beam_prune_cached_joint: otr_beam_prune / otr_beam_prune_cached plus jsrc_out[r'] = ksrc_in[the entry
 *   r' came from] (-1 where its parent was finished): the state slot each survivor inherits, for the next step's jsrc. */
int32_t otr_joint_prebeam(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm, float att_weight, float lm_weight,
                          int64_t rows, int32_t V, int32_t K, float* cand_score, int32_t* cand_idx, void* stream);
int32_t otr_ctc_prefix_score(const float* log_probs, int64_t ld, const int32_t* lengths, int32_t B, int32_t T, int32_t V, int32_t blank,
                             int32_t eos, int64_t rows, int32_t rows_per_utt, int32_t K, const int32_t* cand_idx, const float* cand_score,
                             const uint8_t* flags, const int64_t* preds, int64_t ldp, int32_t t, const int32_t* pos, const int32_t* jsrc,
                             const float* rn_in, const float* rb_in, const float* psi_in, float ctc_weight, float* rn_out, float* rb_out,
                             float* psi_out, int32_t beam, float* k_score, int64_t* k_idx, int32_t* k_src, void* stream);
int32_t otr_beam_prune_joint(const float* k_score, const int64_t* k_idx, const float* scores_in, const uint8_t* flag_in,
                             const int64_t* preds_in, int64_t ldp, int32_t batch, int32_t beam, int32_t t, int32_t eos, float* scores_out,
                             uint8_t* flag_out, int64_t* preds_out, int32_t* n_finished, const int32_t* ksrc_in, int32_t* jsrc_out,
                             void* stream);
int32_t otr_beam_prune_cached_joint(const float* k_score, const int64_t* k_idx, const float* scores_in, const uint8_t* flag_in,
                                    const int64_t* preds_in, int64_t ldp, int32_t batch, int32_t beam, int32_t eos, const int32_t* pos_in,
                                    int32_t* pos_out, const int32_t* anc_in, int32_t* anc_out, int32_t ld_anc, float* scores_out,
                                    uint8_t* flag_out, int64_t* preds_out, int32_t* n_finished, const int32_t* ksrc_in, int32_t* jsrc_out,
                                    void* stream);

/* ---- attention rescoring of the CTC n-best (SpeechToTextRecognizer rescore=True: two-pass decoding), csrc/rescore.hip.  f32 in every
 *      build.  The first pass is otr_ctc_topk + otr_ctc_beam_search: per utterance b the W hypotheses h of the CTC beam, tokens int64
 *      [B, W, T] padded with -1, out_len int32 [B, W], scores f32 [B, W] in descending order.  lambda = ctc_weight in [0, 1],
 *      mu = lm_weight (0 without an LM).  BOS = EOS.  A hypothesis is RESCORABLE when its score is above -inf and len(h) + 1 <= max_len.
 *   att(h) = sum over l = 0 .. len(h) of log_softmax(decoder([BOS] + h, memory_b, mask_b))[l, (h + [EOS])[l]]   (teacher-forced, one pass)
 *   lm(h)  = the same sum over the language model's logits on [BOS] + h
 *   ctc(h) = the beam's own score of h: log(pb + pnb) at the last frame, the beam's approximation of log P_ctc(h | x), taken as is
 *   total(h) = (1 - lambda) att(h) + lambda ctc(h) + mu lm(h), the combination of the joint search above; with penalty != 0 divided by
 *     ((lamda + len(h)) / (lamda + 1)) ** penalty, as the beam search's n-best selection does (recognize/speech2text.py:76-79).
 *   Slots that are not rescorable (and NaN totals) get total = -inf.  Order: total descending, ties -> the lower CTC rank; -inf entries
 *   come last in CTC order, so an utterance without a rescorable hypothesis returns its CTC order with scores -inf.  The empty
 *   hypothesis is an ordinary one: input [BOS], target [EOS].
 * otr_rescore_pack: for each of the n_hyp = B * W hypotheses: ys_in int64 [n_hyp, max_len] = BOS, the tokens, then EOS as filler (any
 *   valid id would do: the causal mask keeps the tail from mattering; tokens are clamped into [0, V)); ys_out int64 [n_hyp, max_len] =
 *   the tokens, EOS, then -1; n_rows int32 [n_hyp] = len + 1, or 0 where the slot is not rescorable (then ys_in = BOS, EOS ..., ys_out
 *   = -1).  V <= 8192.
 * otr_rescore_score: logits f32 [n_hyp * max_len, ld >= V], row (h, l) at logits + (h*max_len + l)*ld.  att_score[h] = sum over
 *   l < n_rows[h] of logits[h, l, ys_out[h, l]] - logsumexp(logits[h, l, :V]); -inf where n_rows[h] == 0.  Rows l >= n_rows[h] are not
 *   read; a row is read once, with 16-byte loads when logits % 16 == 0 and ld % 4 == 0; no [rows, V] log-softmax is written; the sum
 *   runs in a fixed order (the same bits on every run).  lm_logits (may be NULL; row stride ld_lm) is scored the same way into lm_score
 *   by the same launch.
 * otr_rescore_select: one workgroup per utterance: forms total [B, W] (CTC order), ranks by counting, writes perm int32 [B, W] (rank ->
 *   CTC slot) and the nbest best: nbest_tokens int64 [B, nbest, T] (the search's rows, -1 padded), nbest_len int32 [B, nbest],
 *   nbest_score f32 [B, nbest].  lm_score may be NULL.  W <= 32, 1 <= nbest <= W, 0 <= ctc_weight <= 1.
 * Three launches, no allocation, memset or host synchronisation: capturable into a graph behind the search. */
int32_t otr_rescore_pack(const int64_t* tokens, const int32_t* out_len, const float* scores, int64_t n_hyp, int32_t T, int32_t max_len,
                         int32_t V, int32_t bos, int32_t eos, int64_t* ys_in, int64_t* ys_out, int32_t* n_rows, void* stream);
int32_t otr_rescore_score(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm, const int64_t* ys_out, int64_t ld_ys,
                          const int32_t* n_rows, int64_t n_hyp, int32_t max_len, int32_t V, float* att_score, float* lm_score, void* stream);
int32_t otr_rescore_select(const int64_t* tokens, const int32_t* out_len, const float* ctc_score, const int32_t* n_rows,
                           const float* att_score, const float* lm_score, int32_t B, int32_t W, int32_t T, int32_t nbest, float ctc_weight,
                           float lm_weight, float penalty, float lamda, float* total, int32_t* perm, int64_t* nbest_tokens,
                           int32_t* nbest_len, float* nbest_score, void* stream);

/* ---- n-gram LM fusion for the attention, joint and two-pass decoders (SpeechToTextRecognizer ngram_lm=...; ESPnet's partial
 *      scorers: the n-gram sees the pre-beam candidates, not all V tokens), csrc/ngramattn.hip + csrc/rescore.hip.  f32 in every build.
 * The table, its arguments (checked as otr_ngram_lookup checks them) and ln P are those of the n-gram section above; N = order <= 5,
 * <s> = id V, </s> = the EOS unit.  BOS == EOS here, so column 0 of a preds row is <s> by POSITION, never by value.
 * Context of a hypothesis g = preds[r, 0:t]: <s> followed by preds[r, 1:t], cut to its last N-1 ids (the rule of the section above).
 * Addend of extending g by candidate c:  a(g, c) = alpha * ln P(c | context(g)) + (c == eos ? 0 : beta), formed in f32 as alpha * lnP
 *   (one rounding), then + beta (one rounding).  ln P includes oov_score (a candidate or context id without a unigram, or outside
 *   [0, V]), applied before alpha.  EOS is scored as </s> and earns no length bonus.
 * Candidate stage: per unfinished hypothesis the K' candidates come from otr_joint_prebeam, unchanged; a(g, c) is added to their
 *   cand_score.  With nothing pruned (K' = V, beam >= the number of strings) a hypothesis that ended in EOS scores
 *   (1 - lambda) ln P_att + lambda ln P_ctc + mu ln P_lm + alpha * ln P_ng(h </s>) + beta * |h|   (plain mode: lambda = 0).
 * otr_ngram_score_cands: preds int64 [rows, ldp]; the prefix has t columns (t = *pos + 1 where pos, a device scalar, is given; else
 *   the host t, 1 <= t <= ldp), exactly as otr_ctc_prefix_score takes them; flags u8 [rows] (may be NULL); cand_idx int32 / cand_score
 *   f32 [rows, K'], K' <= 32.  cand_out f32 [rows, K'] = cand_score + a (may alias cand_score); rows with flags != 0 are copied
 *   unchanged; a -inf score stays -inf, never NaN.  cand_add f32 [rows, K'] (may be NULL) = the addend alone, 0 on finished rows.
 *   beam > 0 (select mode, beam <= min(16, K')): also the `beam` best of the K' totals in the layout otr_beam_prune /
 *   otr_beam_prune_cached read: k_score f32 / k_idx int64 [rows, beam], descending, ties -> lower token (NaN ranks as -inf); finished
 *   rows get k_score = -inf, k_idx = eos (the prune masks them).  beam = 0: k_score / k_idx are not touched (may be NULL).
 *   One thread per (row, candidate); a row's context-suffix backoffs and context unigrams are probed once per row and shared by
 *   shuffle; every probe of a thread is issued before any is consumed.  One launch, no allocation, memset or host synchronisation.
 * otr_ngram_score_seqs: tokens int64 [n_hyp, T] (negative = padding), out_len int32 [n_hyp].  out f32 [n_hyp] =
 *   ng(h) = alpha * (sum_l ln P(h_l | context(h_{<l})) + ln P(</s> | context(h))) + beta * |h|  for every slot with 0 <= out_len <= T
 *   (0 otherwise); the empty hypothesis gives alpha * ln P(</s> | <s>).  A token outside [0, V] inside the length scores oov_score.
 *   logp f32 [n_hyp] (may be NULL) = the bare sum of ln P.  One wave per hypothesis, one lane per position 0 .. len (the last is </s>),
 *   summed in a fixed order: the same bits on every run.
 * otr_rescore_select_add: otr_rescore_select plus add_score f32 [B, W] (may be NULL), added to total before the division by the length
 *   penalty.  otr_rescore_select is this entry with add_score = NULL: one kernel body, its outputs bit for bit what they were.
 *   In SpeechToTextRecognizer(rescore=True, ngram_lm=...) the first pass is otr_ctc_beam_search_lm, ctc(h) = scores - lm_scores of
 *   that search, and add_score = ng(h) from otr_ngram_score_seqs, computed afresh (it carries the </s> term and does not inherit the
 *   search's rounding): total(h) = (1 - lambda) att + lambda ctc + mu lm + ng, then the penalty. */
int32_t otr_ngram_score_cands(const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V, const int64_t* preds,
                              int64_t ldp, int32_t t, const int32_t* pos, const uint8_t* flags, const int32_t* cand_idx,
                              const float* cand_score, int64_t rows, int32_t K, float alpha, float beta, float oov_score, int32_t eos,
                              float* cand_out, float* cand_add, int32_t beam, float* k_score, int64_t* k_idx, void* stream);
int32_t otr_ngram_score_seqs(const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V, const int64_t* tokens,
                             const int32_t* out_len, int64_t n_hyp, int32_t T, float alpha, float beta, float oov_score, int32_t eos,
                             float* out, float* logp, void* stream);
int32_t otr_rescore_select_add(const int64_t* tokens, const int32_t* out_len, const float* ctc_score, const int32_t* n_rows,
                               const float* att_score, const float* lm_score, const float* add_score, int32_t B, int32_t W, int32_t T,
                               int32_t nbest, float ctc_weight, float lm_weight, float penalty, float lamda, float* total, int32_t* perm,
                               int64_t* nbest_tokens, int32_t* nbest_len, float* nbest_score, void* stream);

/* ---- phrase biasing (hotwords) for the attention, joint and two-pass decoders (SpeechToTextRecognizer bias=...; opentransformer_amd/
 *      bias.py PhraseBias builds the table), csrc/bias.hip.  f32 and integers only: the same code in every build.
 * Phrase set: n sequences of unit ids, each of 1 .. BIAS_MAX_LEN = 16 ids in [0, V), none of them EOS, V <= 8192; phrase i has a
 *   weight w_i >= 0, finite, earned per token.
 * Trie: one node per distinct phrase prefix, the root = the empty prefix = node 0.  Per node u:
 *   tok(u)       = the maximum of w_i over the phrases that pass through the edge into u;
 *   end(u)       = some phrase ends at u;
 *   psi_minus(u) = the sum of tok along root -> u, counted from just behind the last end node strictly above u (from the root where
 *                  there is none), added in f32 from the root towards the leaf;
 *   psi(u)       = end(u) ? 0 : psi_minus(u);  the root has psi_minus = psi = 0.
 * state(x) of a token string x = the longest suffix of x that is a node (the root where none is).  Its depth is at most 16, so the
 *   last 16 tokens of x decide it.  An id outside [0, V) is a token in no phrase.
 * Addend of extending hypothesis g by candidate c:  a(g, c) = psi_minus(state(g c)) - psi(state(g)), ONE f32 subtraction.  EOS is in
 *   no phrase, so state(g EOS) is the root and a = -psi(state(g)): a partial match is refunded.  Hence the addends of a string x sum to
 *   (the psi_minus(v) of every step that landed on an end node v) + psi(state(x)), and with the EOS step to the first term alone: a
 *   finished hypothesis carries its completed phrases, >= 0, however the search reached it.
 *   No output links: a phrase that ends strictly inside a longer partial match of another phrase is credited only if the state itself
 *   is its end node.  That is the rule, not an omission to repair with a second rule.
 *   Column 0 of a prefix row is BOS by POSITION and is not a token (BOS == EOS here), as in otr_ngram_score_cands.
 * Table: `capacity` entries of 16 bytes (capacity a power of two >= 2, the base 16-byte aligned), one per edge (u, token) -> child:
 *   u32 u + 1 (0 = an empty entry), u32 token | end(child) << 31, u32 child, f32 psi_minus(child).  Open addressing, linear probing
 *   from hash(u << 16 | token) & (capacity - 1) (the 64-bit mix of csrc/bias.hip bs_hash); a chain ends at the edge, at an empty entry
 *   or after max_probe entries (the longest chain of the build).  n_nodes = the nodes incl. the root (n_nodes - 1 edges are stored);
 *   max_len = the longest phrase.  A node number is only ever compared, never used as an index.
 * otr_bias_score_cands: the twin of otr_ngram_score_cands -- preds, ldp, t / pos, flags, cand_idx, cand_score, rows, K', cand_out,
 *   cand_add, beam, k_score, k_idx as there, with the same rules: a row with flags != 0 is copied unchanged, its addend 0, its select
 *   -inf / eos; a -inf score stays -inf; NaN ranks as -inf; ties -> the lower token, then the lower slot; cand_out = cand_score + a
 *   is one f32 addition and may alias cand_score.  K' <= 32, beam <= min(16, K').  A row owns 32 lanes, 8 rows per workgroup: lane
 *   j <= 16 walks the last j tokens from the root, the lanes that arrive are the suffix chain of state(g); each candidate lane then
 *   asks for child(n_j, c) from the deepest j down.  One launch, no allocation, memset, atomics, LDS or host synchronisation.
 * otr_bias_score_seqs: the twin of otr_ngram_score_seqs -- tokens int64 [n_hyp, T] (an id < 0 or >= V inside the length is a token in
 *   no phrase; whatever lies behind the length is not read), out_len int32 [n_hyp].  out f32 [n_hyp] = the summed addends of h EOS for
 *   every slot with 0 <= out_len <= T (0 otherwise).  Summation order: one wave per hypothesis; lane i adds the addends of the
 *   positions l = i, i + 64, .. (position out_len is EOS) in ascending l, starting from 0; then the 64 lane sums are combined by the
 *   butterfly v_i += v_(i xor o) for o = 32, 16, 8, 4, 2, 1.  The same bits on every run.
 * Both refuse (< 0, otr_last_error_string() names the argument) before the launch: a null pointer, K', beam, t / ldp, eos and V outside
 *   their limits, a capacity that is no power of two, a table that is not 16-byte aligned, max_probe outside [1, capacity], n_nodes
 *   outside [2, capacity + 1], max_len outside [1, 16].  rows == 0 / n_hyp == 0 returns 0 without a launch. */
#define OTR_BIAS_MAX_LEN 16
int32_t otr_bias_score_cands(const void* table, int64_t capacity, int32_t max_probe, int32_t n_nodes, int32_t max_len, int32_t V,
                             const int64_t* preds, int64_t ldp, int32_t t, const int32_t* pos, const uint8_t* flags,
                             const int32_t* cand_idx, const float* cand_score, int64_t rows, int32_t K, int32_t eos, float* cand_out,
                             float* cand_add, int32_t beam, float* k_score, int64_t* k_idx, void* stream);
int32_t otr_bias_score_seqs(const void* table, int64_t capacity, int32_t max_probe, int32_t n_nodes, int32_t max_len, int32_t V,
                            const int64_t* tokens, const int32_t* out_len, int64_t n_hyp, int32_t T, int32_t eos, float* out,
                            void* stream);

/* ---- n-gram LM estimation (NGramLM.train: interpolated modified Kneser-Ney from unit-id sentences, the ARPA file the entries above
 *      start from), csrc/ngramtrain.hip.  Integers, f32 and f64 only: the same code in every build.  Order N in [1, 4], V in [1, 8192].
 * Corpus: tokens int64 [n_sent, ld] (row b at tokens + b * ld), lengths int32 [n_sent] with 0 <= lengths[b] <= max_len <= ld; columns
 *   at or past lengths[b] are never read.  Every id inside a length lies in [1, V) and differs from eos (1 <= eos < V).  Sentence b is
 *   read as x = <s> w_1 .. w_n </s> with <s> = V and </s> = eos.
 * Count table: `capacity` entries of 32 bytes (capacity a power of two >= 2, the base 8-byte aligned), all zero before otr_ngram_count:
 *   { u64 key, u32 raw, u32 cont, u32 sum, u32 n1, u32 n2, u32 n3p }.  key: the gram's ids, 16 bits each, newest id in bits 0-15 (the
 *   `lo` word of the scoring table's key; ids are >= 1, so key != 0, 0 marks an empty entry, and the gram's order m is the number of
 *   non-zero fields).  Open addressing with linear probing from ng_hash(key, m << 16) & (capacity - 1): the scoring table's hash of the
 *   same gram.  raw = c(g); cont = the number of distinct (m+1)-grams of the corpus that end in g; sum / n1 / n2 / n3p = the context
 *   statistics of g below.  Counters are 32-bit: a corpus holds fewer than 2^32 tokens.
 * Estimator.  Raw counts: for every end position i of x and every m in 1 .. min(N, i+1) the m-gram x[i-m+1 .. i] is counted.
 *   Adjusted count a(g) = c(g) if |g| == N or g starts with <s>, else cont(g) (Kneser-Ney continuation counts, KenLM's <s> rule).  The
 *   unigram <s> takes part in no statistic.  Context h (the empty one included), over all grams h.w of order |h|+1: sum(h) = the sum
 *   of a, n1 / n2 / n3p(h) = the number of them with a = 1, a = 2, a >= 3.  nn[m][k], k = 1 .. 4 = the number of order-m grams with
 *   a = k.  Discounts of order m (Chen & Goodman): Y = nn1 / (nn1 + 2 nn2), D_k = k - (k+1) Y nn_{k+1} / nn_k for k = 1, 2, 3; the
 *   order falls back to (0.5, 1, 1.5) if one of nn1 .. nn4 is 0 or a D_k leaves [0, k].  (The discounts are formed by the caller from
 *   otr_ngram_stats' integers and handed to otr_ngram_estimate.)  With U the predictable units (|U| = n_units; </s> is one of them):
 *     p_m(w | h) = (a(hw) - D_m[min(a, 3)]) / sum(h) + gamma(h) p_{m-1}(w | h'),   h' = h without its oldest id,
 *     gamma(h)   = (D_m[1] n1(h) + D_m[2] n2(h) + D_m[3] n3p(h)) / sum(h),          p_0 = 1 / n_units,
 *   in f64 from the integers.  Entry of a gram g: log-prob = ln p (the unigram <s>: -99 ln 10), backoff = ln gamma(g) with the
 *   discounts of order |g|+1 if sum(g) > 0, else 0; both rounded to f32 once.
 * err int32 [1] on the device, zero before the first pass; the passes OR bits into it and leave the rest to the caller, who reads it
 *   after a pass: 1 = the count table is full (a probe loop ran `capacity` entries), 2 = an id inside a length is outside [1, V) or
 *   equals eos, 4 = a length outside [0, max_len], 8 = a gram's context or suffix is missing from the table (a table that
 *   otr_ngram_count did not fill).  A sentence with a bad length and an end position whose window holds a bad id count nothing.
 * No pass takes a lock or waits for another thread: an insertion is one 64-bit compare-and-swap on the key followed by integer
 *   atomic adds, and every probe loop is bounded by `capacity`.  Every statistic is an integer sum, so the results do not depend on the
 *   order of threads, entries or sentences.
 * otr_ngram_count: one thread per (sentence, end position of x).  Inserts the m = 1 .. N grams in that order and adds 1 to raw; the
 *   thread whose compare-and-swap created an (m+1)-gram adds 1 to cont of its m-gram suffix (which it inserted one step earlier).
 *   n_sent = 0: nothing to do.
 * otr_ngram_stats: one thread per entry; fills sum / n1 / n2 / n3p of every context and glob u64 [20] on the device (zero before):
 *   glob[0..3] = sum, n1, n2, n3p of the empty context, glob[4 + 4 (m-1) + (k-1)] = nn[m][k].  The additions to glob are summed per
 *   workgroup first.
 * otr_ngram_estimate: one launch per order m = 1 .. N, one thread per entry; order m reads prob of its suffix.  discounts f64 [N, 3]
 *   on the HOST (row m-1 = D_m[1..3], each in [0, k]); glob as otr_ngram_stats left it.  Outputs per entry of the count table:
 *   prob f64 = p, logp f32, backoff f32 (entries with key == 0 are not written). */
int32_t otr_ngram_count(const int64_t* tokens, int64_t ld, const int32_t* lengths, int64_t n_sent, int32_t max_len, int32_t order,
                        int32_t V, int32_t eos, void* table, int64_t capacity, int32_t* err, void* stream);
int32_t otr_ngram_stats(void* table, int64_t capacity, int32_t order, int32_t V, uint64_t* glob, int32_t* err, void* stream);
int32_t otr_ngram_estimate(const void* table, int64_t capacity, int32_t order, int32_t V, int32_t n_units, const double* discounts,
                           const uint64_t* glob, double* prob, float* logp, float* backoff, int32_t* err, void* stream);

/* ---- minimum word error rate (MWER) training: the N-best approximation of the expected number of errors (Prabhavalkar et al. 2018)
 *      with its gradient into the decoder's logits, csrc/mwer.hip.  f32 in every build.  B utterances with N hypothesis slots each,
 *      n_hyp = B * N, slot h = b * N + n.  The inputs are what otr_rescore_pack and otr_edit_distance produce:
 *   logits f32, row (h, l) at logits + (h*max_len + l)*ld, ld >= V (the teacher-forced decoder output on otr_rescore_pack's ys_in);
 *   ys_out int64 [n_hyp, ld_ys] (the tokens, EOS, then -1); n_rows int32 [n_hyp] (len + 1, or 0 for a dead slot; a value above max_len
 *   counts as max_len); errors int32 [B, N] (otr_edit_distance's dist; < 0: invalid).
 *   s_h = sum over l < n_rows[h] of x[h, l, ys_out[h, l]] - logsumexp(x[h, l, :V])     (otr_rescore_score's att_score)
 *   Slot h is LIVE iff n_rows[h] > 0, errors[h] >= 0 and every target inside n_rows lies in [0, V); a target outside that range makes
 *   the slot dead (nothing is read out of bounds).  Rows of a slot with n_rows[h] <= 0 or errors[h] < 0 are not read at all.
 *   Per utterance: P_n = softmax over the live n of s (max-subtracted), E_b = sum_n P_n W_n with W = errors.
 *   loss = (1 / B_live) sum_b E_b, B_live = the number of utterances with at least one live slot; B_live = 0: loss 0, gradient all zero.
 *   c_h = P_n (W_n - E_b) / B_live   (sum_n P_n (W_n - E_b) is identically zero: the value is E_b, the centring appears in the gradient only)
 *   dlogits[h, l, v] = g c_h (1[v == ys_out[h, l]] - softmax(x[h, l, :V])_v) for l < n_rows[h] on live slots, g = *grad_scale (a device
 *   scalar; NULL: 1).  EVERY other element of dlogits [n_hyp * max_len, ld_dlogits] is written as zero -- rows at or past n_rows, dead
 *   slots, columns V .. ld_dlogits - 1 -- so the launch needs no memset (a live slot whose g c_h is exactly 0 gets zeros unread).
 * Outputs: loss f32 [1]; seq_logp f32 [n_hyp] = s_h, -inf where the slot is not live; post f32 [B, N] = P, 0 where not live; utt_err f32
 *   [B] = E_b (0 without a live slot); dlogits (NULL: forward only, two launches).  workspace: at least
 *   otr_mwer_workspace_floats(B, N, max_len) floats (the rows' logsumexps and g c_h); that entry runs on the host and answers -1 for a
 *   shape otr_mwer_loss refuses.
 * Launches (at most three): a row pass as otr_rescore_score's -- one workgroup per slot, one wave per row, the row read once into an
 *   online max / sum; wave w adds rows w, w + 4, ... in order and thread 0 adds the four partials in order; one workgroup that forms P,
 *   E_b, c_h and the loss over the B * N scalars in a fixed order; a gradient pass, one wave per row, that reads each live row once
 *   more.  No floating-point atomics: the same bits on every run.  Loads and stores are 16 bytes wide where the base is 16-byte aligned
 *   and the row stride a multiple of 4 floats (logits and dlogits judged separately), scalar otherwise.
 * Refused before any launch (< 0, outputs untouched): a null pointer (grad_scale and dlogits may be NULL), N outside [1, 32], V outside
 *   [1, 8192], ld < V, ld_dlogits < V (with dlogits), ld_ys < max_len, max_len < 1, B < 0, B * N * max_len >= 2^30, a NULL or too small
 *   workspace.  B = 0 returns 0 without a launch.  Caller-owned buffers, no allocation, memset or host synchronisation: capturable. */
int64_t otr_mwer_workspace_floats(int32_t B, int32_t N, int32_t max_len);
int32_t otr_mwer_loss(const float* logits, int64_t ld, const int64_t* ys_out, int64_t ld_ys, const int32_t* n_rows, const int32_t* errors,
                      int32_t B, int32_t N, int32_t max_len, int32_t V, const float* grad_scale, float* loss, float* seq_logp,
                      float* post, float* utt_err, float* dlogits, int64_t ld_dlogits, float* workspace, int64_t workspace_floats,
                      void* stream);

/* ---- knowledge distillation (Hinton et al. 2015): the temperature-scaled KL divergence of a student's logits from a teacher's, per
 *      frame, with its gradient into the student's logits, csrc/distill.hip.  f32 in every build.  Rows are [B, T]: row r = b * T + i
 *      at student + r * ld_s (and teacher + r * ld_t, top_val / top_idx + r * K, dlogits + r * ld_d).
 *   Row (b, i) is LIVE iff i < min(max(lengths[b], 0), T), lengths int32 [B] on the device -- and, in the sparse form, it lists at least
 *   one entry; in the dense form, its teacher row holds at least one element above -inf (a teacher row of -inf throughout has no
 *   distribution to distil).  Rows that are dead by lengths are never read; finding the other two kinds takes a read of the row's teacher.
 *   n_live = the number of live rows, formed on the device.
 *   With tau = temperature: p = softmax(student[r, :V] / tau).
 *   Dense teacher (teacher != NULL):  q = softmax(teacher[r, :V] / tau); a teacher element of -inf gives q_v = 0 and a term of 0.
 *   Sparse teacher (top_val f32, top_idx int32, both [B*T, K]): the LISTED entries of row r are the k with 0 <= top_idx[r, k] < V; q over
 *   them is softmax(top_val[r, k] / tau) -- the top-K mass is renormalised, and the values may be logits or log-probs, the softmax being
 *   shift-invariant -- and 0 elsewhere.  An index outside [0, V) drops its entry and is never used as an address.  Indices within a row
 *   must be distinct (the caller's contract; otr_ctc_topk keeps it).  An entry of -inf is listed with q = 0.
 *   kl_r = sum_v q_v (ln q_v - ln p_v)
 *   loss = tau^2 / n_live * sum over the live rows of kl_r      (Hinton's scaling: the gradient's magnitude does not depend on tau)
 *   dlogits[r, v] = g * tau / n_live * (p_v - q_v) on live rows for v < V, g = *grad_scale (a device scalar; NULL: 1).  EVERY other
 *   element of dlogits [B*T, ld_d] is written as zero -- dead rows, columns V .. ld_d - 1 -- so the launch needs no memset.
 *   n_live = 0: loss 0, gradient all zero.
 * Outputs: loss f32 [1]; row_kl f32 [B*T] = kl_r, 0 on dead rows; dlogits (NULL: forward only, two launches).  workspace: at least
 *   otr_distill_workspace_floats(B, T) floats (every row's maxima and reciprocal sums, and g tau / n_live); that entry runs on the host
 *   and answers -1 for a shape otr_distill_loss refuses.
 * Launches (at most three): a row pass, one wave per row, that reads the row ONCE -- student and teacher together -- into online
 *   maxima / sums; the cross term sum_v e^{t_v/tau - m} (t_v - s_v) / tau is rescaled whenever the teacher's maximum moves, so kl_r needs
 *   no second read (the sparse form gathers student[r, top_idx] after the row pass instead); one workgroup that adds row_kl up in a fixed
 *   order; a gradient pass, one wave per row, that reads each live row once more.  No floating-point atomics: the same bits on every run.
 *   Loads and stores are 16 bytes wide where the base is 16-byte aligned and the row stride a multiple of 4 floats (student, teacher and
 *   dlogits judged separately), scalar otherwise.
 * Refused before any launch (< 0, outputs untouched): both teacher forms or neither (the sparse form counts as given when top_val,
 *   top_idx or K is non-zero); a NULL student, lengths, loss, row_kl, or one of top_val / top_idx in the sparse form; V outside
 *   [1, 8192]; K outside [1, 128] in the sparse form; ld_s, ld_t (dense) or ld_d (with dlogits) below V; T < 1, B < 0, B * T >= 2^30;
 *   temperature not finite or <= 0; a NULL, too small or not 16-byte aligned workspace.  B = 0 returns 0 without a launch.  Caller-owned buffers, no
 *   allocation, memset or host synchronisation: capturable. */
int64_t otr_distill_workspace_floats(int32_t B, int32_t T);
int32_t otr_distill_loss(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t, const float* top_val,
                         const int32_t* top_idx, int32_t K, const int32_t* lengths, int32_t B, int32_t T, int32_t V, float temperature,
                         const float* grad_scale, float* loss, float* row_kl, float* dlogits, int64_t ld_d, float* workspace,
                         int64_t workspace_floats, void* stream);

/* ---- transposed copies of many matrices in ONE launch (the W^T bf16 shadows that turn dx = dy.W into a
 *      forward-type GEMM; refreshed after every optimizer step).  table: DEVICE int64 [n_mats,4] rows of
 *      {element offset, rows, cols, first tile}; matrix i is src+offset [rows,cols] row-major and is written to
 *      dst+offset as [cols,rows]; tiles are 64x64, total_tiles = sum of ceil(rows/64)*ceil(cols/64). */
int32_t otr_transpose_batched(const void* src, void* dst, const int64_t* table, int32_t n_mats, int64_t total_tiles,
                              int32_t elem_bytes, void* stream);

/* ---- SpecAugment on the device (data/augment.py:9-41): zero x[b,t,f] (f32 [B,T,F]) inside NR
 *      rectangles per utterance, ranges int32 [B,NR,4] = {t0,t1,f0,f1} half-open.  The rectangles are drawn on the host
 *      with the reference's own random calls (opentransformer_amd/data.py), so the masks are bit-identical. */
int32_t otr_spec_mask(float* x, const int32_t* ranges, int32_t B, int32_t NR, int32_t T, int32_t F, void* stream);

/* ---- feature preparation for device batch assembly (otrans/data/audio.py:125-136: normalisation -> gaussian noise -> SpecAugment, run
 *      per utterance after the fbank) while a packed ragged upload is spread into the padded batch, and the sums of a global CMVN;
 *      csrc/featprep.hip.  fp32 / fp64 in every build.
 * otr_feature_prepare: utterance b is the contiguous span of lengths[b] * F floats at src + row_off[b] * F (row_off int64 [B] in FRAMES,
 *   lengths int32 [B], both on the device; lengths[b] is clamped to [0, Tmax]): one [sum T, F] buffer.  src == dst with row_off[b] ==
 *   b * Tmax is the in-place padded form; every other overlap of src and dst is undefined.
 *   dst f32 [B, Tmax, F]: EVERY cell is written (it may be uninitialised).  Rows t >= lengths[b] are exactly 0.0f.  A live cell is
 *   y = norm(x) + noise[b, f] (noise f32 [B, F] or NULL: one vector per utterance added to every frame, the reference's quirk), then
 *   exactly 0.0f inside any of the NR rectangles of utterance b, ranges int32 [B, NR, 4] = {t0, t1, f0, f1} half-open as otr_spec_mask
 *   takes them (NULL: none; NR <= 64; an empty rectangle changes nothing).
 *   norm_mode 0: norm(x) = x.  1: (x - mean_b) / std_b with the utterance's scalar mean and UNBIASED std over its lengths[b] * F values,
 *   both rounded to fp32 before use as torch.std_mean gives them (audio.py:22-24); a zero std or fewer than two values gives what IEEE
 *   gives, there is no epsilon.  2: (x - gmean[f]) / gstd[f], f32 [F] each.
 *   mask uint8 [B, Tmax] (or NULL) = 1 where t < lengths[b]; stats f32 [B, 2] (or NULL) = the mean and std used in mode 1 (untouched in
 *   the other modes).  An utterance of length 0 gives zero rows and a zero mask; its row_off is not read from and its stats are
 *   unspecified.
 *   Launches: one (modes 0 and 2) or two (mode 1: fp64 sums of d = x - x[0] and d * d per chunk of 4096 elements into the workspace; then
 *   every workgroup of the second launch adds the utterance's partials in index order).  No floating-point atomics: the same call gives
 *   the same bits.  Loads and stores are 16 bytes wide where the utterance's base allows (src span and dst row judged separately; a dst
 *   row is aligned when dst is and Tmax * F is a multiple of 4 or b = 0), scalar otherwise.
 *   workspace: at least otr_feature_prepare_workspace_bytes(B, Tmax, F) bytes, 8-byte aligned, in every mode; that entry runs on the host
 *   and answers -1 for a shape otr_feature_prepare refuses.
 *   Refused before any launch (< 0, outputs untouched): a NULL src, row_off, lengths or dst; B outside [0, 65535], Tmax <= 0, F <= 0,
 *   Tmax * F >= 2^31; NR outside [0, 64]; NR > 0 with NULL ranges; norm_mode outside 0 .. 2; mode 2 with a NULL gmean or gstd; a
 *   workspace that is too small.  B = 0 returns 0 without a launch.  Caller-owned buffers, no allocation or host synchronisation: capturable.
 * otr_cmvn_accumulate: adds into acc f64 [2F + 1] the per-dimension sums [F], the per-dimension sums of squares [F] and the frame count
 *   over all live frames (lengths[b] <= 0: none) of the call, src / row_off / lengths as above.  One launch; a workgroup owns 16
 *   dimensions and is the only writer of their entries, and adds in a fixed order: a given sequence of calls on one stream gives the
 *   same bits.  Mean and std are formed on the host from acc. */
int64_t otr_feature_prepare_workspace_bytes(int32_t B, int32_t Tmax, int32_t F);
int32_t otr_feature_prepare(const float* src, const int64_t* row_off, const int32_t* lengths, int32_t B, int32_t Tmax, int32_t F,
                            int32_t norm_mode, const float* gmean, const float* gstd, const float* noise, const int32_t* ranges, int32_t NR,
                            float* dst, uint8_t* mask, float* stats, void* workspace, int64_t workspace_bytes, void* stream);
int32_t otr_cmvn_accumulate(const float* src, const int64_t* row_off, const int32_t* lengths, int32_t B, int32_t F, double* acc,
                            void* stream);

/* ---- incremental (KV-cached) decoding, SURVEY.md 8f rank 1.  The reference threads a `cache` argument through
 *      decoder.inference / attention.inference but never fills it (decoder/transformer.py:185-208,
 *      module/attention.py:86-104, README.md:13 TODO) and re-runs the decoder over the whole prefix each step.
 *      Here one token per hypothesis is fed per step; every step-dependent scalar is read from DEVICE memory
 *      (pos = index of the token being fed) so one captured hipGraph serves all steps.
 * decode_embed: y[r,:] = E[preds[r, *pos], :]*scale + PE[*pos]  (decoder/transformer.py:163-169, model/lm.py:143-150)
 * decode_self_attention: qkv [rows, 3*H*dk] (q|k|v of the new position); kcache/vcache [rows, maxlen, H*dk] are
 *   write-once: the new k,v are stored at [r, *pos]; anc int32 [rows, maxlen]: anc[r,j] = cache row that holds
 *   position j < *pos of hypothesis r (hypotheses form a tree under beam pruning, so caches are never gathered);
 *   out [rows, H*dk] = softmax(q.k/sqrt(dk)) v over positions 0..*pos.
 * beam_prune_cached: otr_beam_prune with t = *pos_in + 1, plus anc_out[r'] = anc_in[parent(r')] ++ parent(r') and
 *   *pos_out = *pos_in + 1 (in/out buffers must be distinct). */
int32_t otr_decode_embed(const int64_t* preds, int64_t ldp, const int32_t* pos, const float* E, float* y, void* y_bf16,
                         int64_t rows, int32_t d, int32_t vocab, float scale, void* stream);
/* ---- the recurrent language model of the shallow fusion (model/lm.py:33-91: nn.Embedding -> nn.LSTM -> Linear; reached through
 *      recognize/base.py:26-37, which feeds it the LAST token of every hypothesis).
 * otr_decode_lookup: y[r,:] = E[preds[r, *pos],:] (f32 + optional 16-bit twin), pos a device scalar or NULL (= column 0).
 * otr_lstm_cell:     one cell update in torch.nn.LSTM's gate order i | f | g | o: gates = gates_a [rows,4H] + gates_b [rows,4H] (NULL)
 *                    + bias_b [4H] (NULL);  c = sigmoid(f) c_prev + sigmoid(i) tanh(g) (c_prev NULL = zeros);  h = sigmoid(o) tanh(c).
 *                    The two GEMMs (W_ih x + b_ih, W_hh h + b_hh) are otr_linear_fwd calls. */
int32_t otr_decode_lookup(const int64_t* preds, int64_t ldp, const int32_t* pos, const float* E, float* y, void* y_bf16, int64_t rows,
                          int32_t d, int32_t vocab, void* stream);
int32_t otr_lstm_cell(const float* gates_a, const float* gates_b, const float* bias_b, const float* c_prev, float* h, void* h_bf16,
                      float* c, int64_t rows, int32_t hidden, void* stream);
/* ---- training the recurrent LM: nn.LSTM forward with saved activations, and backpropagation through time (csrc/lstm.hip).
 * Per layer the caller computes gx = X W_ih^T + b_ih for all T steps at once (otr_linear_fwd), stored TIME-MAJOR [T, B, 4H], then
 * runs one step launch per t; the weight gradients are GEMMs over the saved dG [T, B, 4H] afterwards (dW_hh = sum_t dG_t^T h_{t-1},
 * dW_ih = dG^T X, db_ih = db_hh = column sums of dG, dX = dG W_ih).  Gate order i | f | g | o; act holds the activations
 * (sigmoid(i), sigmoid(f), tanh(g), sigmoid(o)) [B, 4H] f32; h, c [B, H] f32.
 *  dtype: OTR_F32 (f32 operands, exact-f32 MFMA) or this build's 16-bit code (16-bit operands, f32 accumulate).  "CT" below is that
 *  type: h_prev, dg_next and dg are CT; in f32 mode h_prev is the previous step's f32 h and h_bf16 is NULL.
 * Limits of the fused step kernels (otr_lstm_step_supported says whether a shape is inside): 1 <= rows (the batch) <=
 * OTR_LSTM_MAX_ROWS, hidden a multiple of OTR_LSTM_HIDDEN_MULT and <= OTR_LSTM_MAX_HIDDEN; h_prev, dg_next and the packs 16-byte
 * aligned.  Other shapes take the unfused route: the recurrent products as otr_linear_fwd / otr_linear_dgrad calls per step and the
 * elementwise otr_lstm_cell_fwd / otr_lstm_cell_bwd, which have no shape limit.
 * otr_lstm_pack_whh: W_hh [4H, H] f32 -> fwd_pack and/or bwd_pack (either may be NULL), 4H*H elements of CT each, in the MFMA
 *   fragment order the step kernels read (per block of 16 hidden units: its four gate rows / its 16 columns).  A pack is a copy:
 *   make it again after every change of W_hh.
 * otr_lstm_fwd_step:  z = gx_t [B,4H] + bias [4H] (NULL: none; pass b_hh) + h_prev W_hh^T (h_prev NULL = zero state, no product);
 *   act = activations of z; c = act_f c_prev + act_i act_g (c_prev NULL = zeros); h = act_o tanh(c), h_bf16 its 16-bit twin (NULL: none).
 * otr_lstm_bwd_step:  dh = dy [B,H] + dg_next W_hh (dg_next NULL: the last step, no product); dc = dh act_o (1 - tanh^2 c) + dc_in
 *   (dc_in NULL = zeros); dg = (dc act_g act_i(1-act_i), dc c_prev act_f(1-act_f), dc act_i (1-act_g^2), dh tanh(c) act_o(1-act_o));
 *   dc_out = dc act_f.  dc_in and dc_out may be the same buffer.
 * otr_lstm_cell_fwd / otr_lstm_cell_bwd: the same cell maths on `rows` rows, with the recurrent product given as gh [rows,4H] /
 *   dh_rec [rows,H] (NULL: none). */
#define OTR_LSTM_MAX_ROWS 64
#define OTR_LSTM_HIDDEN_MULT 64
#define OTR_LSTM_MAX_HIDDEN 2048
int32_t otr_lstm_step_supported(int64_t rows, int32_t hidden);
int32_t otr_lstm_pack_whh(const float* w_hh, void* fwd_pack, void* bwd_pack, int32_t dtype, int32_t hidden, void* stream);
int32_t otr_lstm_fwd_step(const float* gx, const float* bias, const void* h_prev, const float* c_prev, const void* fwd_pack, float* h,
                          void* h_bf16, float* c, float* act, int32_t dtype, int64_t rows, int32_t hidden, void* stream);
int32_t otr_lstm_bwd_step(const float* dy, const void* dg_next, const void* bwd_pack, const float* act, const float* c,
                          const float* c_prev, const float* dc_in, float* dc_out, void* dg, int32_t dtype, int64_t rows, int32_t hidden,
                          void* stream);
int32_t otr_lstm_cell_fwd(const float* gx, const float* gh, const float* bias, const float* c_prev, float* h, void* h_bf16, float* c,
                          float* act, int64_t rows, int32_t hidden, void* stream);
int32_t otr_lstm_cell_bwd(const float* dy, const float* dh_rec, const float* act, const float* c, const float* c_prev,
                          const float* dc_in, float* dc_out, void* dg, int32_t dtype, int64_t rows, int32_t hidden, void* stream);
int32_t otr_decode_self_attention(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const int32_t* pos,
                                  void* out, int32_t dtype, int64_t rows, int32_t H, int32_t dk, int32_t maxlen,
                                  float scale, void* stream);
/* otr_beam_prune_cached: n_finished is int32[2] here -- [0] receives the number of finished hypotheses, [1] is the kernel's arrival
 * word: zero it once when the buffer is made, the launch leaves it zero (no zeroing launch per step, r05).  batch * beam < 65536. */
int32_t otr_beam_prune_cached(const float* k_score, const int64_t* k_idx, const float* scores_in, const uint8_t* flag_in,
                              const int64_t* preds_in, int64_t ldp, int32_t batch, int32_t beam, int32_t eos,
                              const int32_t* pos_in, int32_t* pos_out, const int32_t* anc_in, int32_t* anc_out,
                              int32_t ld_anc, float* scores_out, uint8_t* flag_out, int64_t* preds_out,
                              int32_t* n_finished, void* stream);

/* ---- fused decoder layer for few rows (decoder/transformer.py:47-90 TransformerDecoderLayer.forward, post-norm, and :161-183
 *      the stack around it; module/attention.py:60-84,120-145; module/ffn.py:38-41 'glu'), csrc/declayer.hip.  d_model 256, 4 heads
 *      of 64, 16-bit operands, L <= 32 decoder rows per utterance.  Three launches per layer, cut along (utterance group, head) /
 *      (32-row block, hidden slice); a sub-layer leaves PARTIAL sums of its branch in `slabs` 16-BIT [n][R][256] (R = B * L rows) and the
 *      next launch finishes  y = LayerNorm(xres + dropout(sum_n slabs[n] + bias))  in its prologue -- described by otr_dec_ln_t --
 *      writing y / y16 / z / mean / rstd (each may be NULL) once per row.  nslab == 0: nothing to finish, the rows are taken from x16.
 *      Weight packs are otr_pack_frags packs with perm 0, rows = outputs (the forward packs of otr_rb_linear / otr_ffn_ln_fwd).
 * otr_dec_self_fwd:  q|k|v of every head (qkv16 [R,768], columns q | k | v), causal self-attention inside each utterance (ctx16 [R,256],
 *      lse f32 [B,4,L]), slabs [4][R][256] = per-head shares of ctx . W_o^T (no bias), 16-bit.
 * otr_dec_cross_fwd: q (q16 [R,256]) against the utterance's encoder keys / values, element (b, t, c) at kv[b*kv_bs + t*kv_ts + c], keys
 *      from column koff, values from voff (head h adds 64 h); key_mask uint8 [B,Tk] or NULL; ctx16, lse, slabs as above.
 * otr_dec_ffn_fwd:   slabs [S][R][256] = w_2 glu(w_1 y + b_1) over 1/S of the hidden units each (no b_2); F % (128 S) == 0.  hsave
 *      (may be NULL; otr_dec_ffn_hsave_bytes(R, F) bytes, opaque) receives (value + bias, sigmoid(gate)) of every hidden unit for
 *      otr_dec_ffn_bwd.  Every slab is 16-bit (the shares are rounded once and added up in fp32 by the consumer): the prologues are
 *      bound by what a CU can ingest, and the slabs were most of it.
 * otr_dec_ln:        the LayerNorm alone (closes the last layer). */
typedef struct {
  const float* xres; const void* x16; const void* slabs; int32_t nslab;
  const float* bias; const float* gamma; const float* beta; const uint64_t* seed;
  float p_drop, eps; uint64_t rng_offset;
  float* y; void* y16; float* z; float* mean; float* rstd;
} otr_dec_ln_t;
int32_t otr_rb_linear_ln(const otr_dec_ln_t* ln, const void* w_pack, const float* bias, void* out, int32_t out_dtype, int64_t ldo, int64_t M,
                         int32_t N, int32_t K, void* stream);
/* utterances per (group, head) workgroup of the four attention launches for a batch of B utterances x L decoder rows (host only): the
 * per-group partial buffers of otr_dec_cross_bwd / otr_dec_self_bwd have ceil(B / this) rows.  0 for shapes the launches refuse. */
int32_t otr_dec_group_size(int32_t B, int32_t L);
int32_t otr_dec_self_fwd(const otr_dec_ln_t* ln, int32_t B, int32_t L, const void* wqkv_pack, const float* bqkv, const void* wo_pack,
                         void* qkv16, void* ctx16, float* lse, void* slabs, void* stream);
/* otr_dec_self_step: the self-attention sub-layer of ONE cached beam-search step (recognize/speech2text.py:95-146 with the KV cache the
 *      reference leaves as a TODO, README.md:13): R hypothesis rows, one new position *pos each.  Finishes `ln` (the layer below), projects
 *      q | k | v, appends k, v to kcache / vcache [R, maxlen, 256] at position *pos, attends over positions 0..*pos of the row's ancestors
 *      (anc int32 [R, maxlen]: anc[r][j] = the row whose cache holds position j of r's prefix; as otr_decode_self_attention), and leaves
 *      slabs [4][R][256] = per-head shares of ctx . W_o^T for the next launch's prologue.  Replaces otr_dec_ln + otr_linear_fwd +
 *      otr_decode_self_attention + otr_proj_ln_fwd of the step. */
int32_t otr_dec_self_step(const otr_dec_ln_t* ln, int64_t R, const void* wqkv_pack, const float* bqkv, const void* wo_pack, void* kcache,
                          void* vcache, const int32_t* anc, const int32_t* pos, int32_t maxlen, void* slabs, void* stream);
int32_t otr_dec_cross_fwd(const otr_dec_ln_t* ln, int32_t B, int32_t L, const void* wq_pack, const float* bq, const void* wo_pack,
                          const void* kv, int64_t kv_bs, int64_t kv_ts, int32_t koff, int32_t voff, const uint8_t* key_mask, int32_t Tk,
                          void* q16, void* ctx16, float* lse, void* slabs, void* stream);
/* otr_dec_cross_fwd_shared: otr_dec_cross_fwd for B sequences of which every `share` consecutive ones attend to the SAME encoder memory
 *      (the W hypotheses of an utterance in attention rescoring): sequence s reads kv[(s / share)*kv_bs + t*kv_ts + c] and key_mask row
 *      s / share; kv and key_mask hold B / share memories, B % share == 0.  Everything else, and the result for share == 1, as
 *      otr_dec_cross_fwd.  Forward only. */
int32_t otr_dec_cross_fwd_shared(const otr_dec_ln_t* ln, int32_t B, int32_t L, const void* wq_pack, const float* bq, const void* wo_pack,
                                 const void* kv, int64_t kv_bs, int64_t kv_ts, int32_t koff, int32_t voff, const uint8_t* key_mask,
                                 int32_t Tk, int32_t share, void* q16, void* ctx16, float* lse, void* slabs, void* stream);
int64_t otr_dec_ffn_hsave_bytes(int64_t R, int32_t F);
int32_t otr_dec_ffn_fwd(const otr_dec_ln_t* ln, int64_t R, const void* w1_pack, const float* b1, const void* w2_pack, int32_t F, int32_t S,
                        void* slabs, void* hsave, void* stream);
int32_t otr_dec_ln(const otr_dec_ln_t* ln, int64_t R, void* stream);
/* PAIR launches (r06): two independent problems of the same launch in ONE grid -- the decoder's and the language model's layer of a
 * beam-search step (recognize/speech2text.py:100-113 runs them one after the other; they only meet in the top-k).  Block ids
 * 0 .. n_a - 1 work on problem a, the rest on b; each descriptor holds exactly the arguments of the single entry.  The LM chain then
 * rides in the decoder's launches: no second stream, no branch in the captured step. */
typedef struct {
  otr_dec_ln_t ln; int64_t R; const void* wqkv_pack; const float* bqkv; const void* wo_pack; void* kcache; void* vcache;
  const int32_t* anc; const int32_t* pos; int32_t maxlen; void* slabs;
} otr_dec_self_step_t;
typedef struct {
  otr_dec_ln_t ln; int64_t R; const void* w1_pack; const float* b1; const void* w2_pack; int32_t F, S; void* slabs; void* hsave;
} otr_dec_ffn_fwd_t;
int32_t otr_dec_self_step_pair(const otr_dec_self_step_t* a, const otr_dec_self_step_t* b, void* stream);
int32_t otr_dec_ffn_fwd_pair(const otr_dec_ffn_fwd_t* a, const otr_dec_ffn_fwd_t* b, void* stream);
int32_t otr_dec_ln_pair(const otr_dec_ln_t* a, int64_t Ra, const otr_dec_ln_t* b, int64_t Rb, void* stream);
/* Backward, the same cut mirrored (csrc/declayer.hip).  The gradient of a sub-layer's LayerNorm output arrives as dskip f32 [R,256]
 * (may be NULL) plus nslab partial slabs; every launch finishes it and runs that LayerNorm's backward in its prologue
 * (otr_dec_lnb_t; z / mean / rstd as saved by the forward prologue), writing -- once per row -- dz (the gradient of the residual input =
 * the skip part for the launch below), da16 (the dropout-masked branch gradient: weight-gradient operand of output_proj / w_2) and
 * partial f32 [row blocks][3][256] = per-block sums of dgamma | dbeta | d branch-bias (column-sum them; a row block is a group for the
 * attention launches (ceil(B / (32 / L)) of them), 32 rows for the FFN launch).
 * otr_dec_ffn_bwd:   the hidden comes from hsave (otr_dec_ffn_fwd); dh [R,2F], u [R,F] (weight-gradient operands), db1_part
 *      [ceil(R/32)][2F] (column-sum for the w_1 bias gradient), slabs 16-BIT [S][R][256] = shares of dh . w_1.  Packs as otr_ffn_bwd.
 *      (all slabs 16-bit, as in the forward launches)
 * otr_dec_cross_bwd: wo / wq input-gradient packs (otr_pack_frags of W as A[k][n]); q16, ctx16, lse as the forward left them; dkv has kv's
 *      geometry and receives d keys / d values of this layer's columns (every (utterance, key) once); dq16 [R,256]; slabs [4][R][256] =
 *      per-head shares of dq . W_q.
 * otr_dec_self_bwd:  dqkv16 [R,768]; slabs [4][R][256] = per-head shares of dqkv . W_qkv.
 * otr_dec_sum:       out = skip + sum of slabs (the gradient that leaves the stack). */
typedef struct {
  const float* dskip; const void* slabs; int32_t nslab;
  const float* z; const float* mean; const float* rstd; const float* gamma; const uint64_t* seed;
  float p_drop; uint64_t rng_offset;
  float* dz; void* da16; float* partial;
} otr_dec_lnb_t;
int32_t otr_dec_ffn_bwd(const otr_dec_lnb_t* ln, int64_t R, const void* hsave, const void* w2t_pack, const void* w1t_pack, int32_t F,
                        int32_t S, void* dh, void* u, float* db1_part, void* slabs, void* stream);
int32_t otr_dec_cross_bwd(const otr_dec_lnb_t* ln, int32_t B, int32_t L, const void* wo_dgrad_pack, const void* wq_dgrad_pack, const void* q16,
                          const void* ctx16, const float* lse, const void* kv, void* dkv, int64_t kv_bs, int64_t kv_ts, int32_t koff,
                          int32_t voff, const uint8_t* key_mask, int32_t Tk, void* dq16, void* slabs, void* stream);
int32_t otr_dec_self_bwd(const otr_dec_lnb_t* ln, int32_t B, int32_t L, const void* wo_dgrad_pack, const void* wqkv_dgrad_pack,
                         const void* qkv16, const void* ctx16, const float* lse, void* dqkv16, void* slabs, void* stream);
int32_t otr_dec_sum(const float* skip, const void* slabs, int32_t nslab, int64_t R, float* out, void* stream);

/* ---- the transducer (RNN-T): joint, lattice loss, greedy decoding (csrc/rnnt.hip).  f32 in both builds; blank is an index of the
 *      vocabulary (the models use 0).  U1 = U + 1 lattice columns, at most OTR_RNNT_MAX_TGT + 1 = 256 (one thread per column, four
 *      wavefronts); B, T <= 65535 and B * T * U1 < 2^31 rows; every element offset is 64-bit (rows * V passes 2^32 bytes early).
 *      enc_len / tgt_len int32 [B]: T_b frames and U_b labels of utterance b.
 * otr_rnnt_joint_fwd: z[b,t,u,:] = tanh(pe[b,t,:] + pg[b,u,:]) for t < T_b, u <= U_b (lengths clamped to [0, T] / [0, U1]) and exact
 *      zeros elsewhere, where pe / pg are not read.  pe f32 [B,T,J], pg f32 [B,U1,J], z f32 [B,T,U1,J], z16 its 16-bit twin (the
 *      build's type) or NULL; J a multiple of 4, the four buffers 16-byte aligned.
 * otr_rnnt_joint_bwd: dpe[b,t,:] = sum_u dz (1 - z^2), dpg[b,u,:] = sum_t dz (1 - z^2) over the same live positions; dz outside them
 *      is not read (NaN there is harmless), dpe / dpg rows outside the lengths are zeros.  Two launches, each reads dz and z once,
 *      16 bytes per lane along J; the partial sums meet in a fixed order: the same bits on every run.
 * otr_rnnt_loss: logits f32, row (b,t,u) at logits + ((b*T + t)*U1 + u) * ld, ld >= V, RAW (one log-softmax is taken here): lp.
 *      labels int64, y_1..y_U of utterance b at labels + b*ldl (ldl >= U1 - 1; a strided view is read in place).
 *        alpha(0,0) = 0; alpha(t,u) = logaddexp(alpha(t-1,u) + lp[t-1,u,blank], alpha(t,u-1) + lp[t,u-1,y_u]);
 *        beta(T_b-1,U_b) = lp[T_b-1,U_b,blank]; beta(t,u) = logaddexp(beta(t+1,u) + lp[t,u,blank], beta(t,u+1) + lp[t,u,y_{u+1}]);
 *        nll[b] = -(alpha(T_b-1,U_b) + lp[T_b-1,U_b,blank]); loss = (1/B) sum_b nll[b].
 *      An utterance is GUARDED (nll 0, valid 0, zero gradient, still counted in 1/B) when T_b <= 0, T_b > T, U_b < 0, U_b >= U1,
 *      U_b > OTR_RNNT_MAX_TGT, or a label inside U_b lies outside [0, V) or equals blank; the guard is taken on the device and no
 *      label is an index before it was range-checked.  Labels are read only where the lengths are in range.
 *      dlogits (NULL: forward only), row stride ldd >= V, EVERY cell written: with p = softmax and s = *grad_scale / B (NULL: 1 / B)
 *        s * [ p_v exp(alpha + beta - lnP) - [v == blank] exp(alpha + lp_blank + beta(t+1,u) - lnP)
 *                                          - [v == y_{u+1}] exp(alpha + lp_label + beta(t,u+1) - lnP) ]   (beta(T_b,U_b) := 0)
 *      on live rows of valid utterances, exact zeros on every other row and behind column V; rows that are not live are not read.
 *      workspace: otr_rnnt_workspace_floats(B, T, U1) = 5 * B*T*U1 + 2 * B floats (lse, lp_blank, lp_label, alpha, beta; per utterance
 *      the shifted ln P and the shift c), -1 for a refused shape.  The sweeps run on lp + c, c = minus the mean of lp_blank over up to
 *      256 evenly spaced live cells: alpha + (t + u) c and beta + (T_b + U_b - t - u) c stay small numbers where the plain ones grow
 *      like (t + u) |lp|, whose float32 ulp would otherwise sit in every exponent of the gradient; nll is shifted back.
 *      Launches: a wave per live row (logsumexp, 16-byte loads behind the row's own alignment peel); 2B workgroups (alpha and beta of
 *      every utterance, a barrier per anti-diagonal); one workgroup for the mean; a wave per row of dlogits.  No atomics: the same
 *      bits on every run.  No allocation or host synchronisation: capturable.  Refused before any launch: a shape outside the limits
 *      above, V < 2, ld or ldd < V, ldl < U1 - 1, blank outside [0, V), a NULL pointer other than grad_scale / dlogits (labels
 *      may be NULL at U1 = 1), a workspace that is too small.
 * otr_rnnt_greedy_joint: one decode step's joint input z[b,:] = tanh(pe[b, t[b], :] + pg_cur[b,:]) with its 16-bit twin; a row that is
 *      done (t[b] >= T_b or n[b] >= max_len) gets zeros.
 * otr_rnnt_greedy_advance: one decode step's tail on logits [B, V] (row stride ld).  A row that is done is left alone (emit 0).
 *      Otherwise k = arg-max (lowest index on ties), lp = log-softmax of the row.  If k != blank and count[b] < max_symbols the row
 *      EMITS: tokens[b, n[b]] = k, frames[b, n[b]] = t[b], score[b] += lp[k], n[b]++, count[b]++, emit[b] = 1, step_tok[b] = k.  Else
 *      t[b]++, count[b] = 0, score[b] += lp[blank], emit[b] = 0, step_tok[b] = blank.  *remaining loses 1 when the row becomes done
 *      (t[b] == T_b or n[b] == max_len): initialise it with the number of rows that start not done.  tokens int64 / frames int32
 *      are [B, max_len].
 * otr_rnnt_greedy_commit: for every item k < n_items (at most 16) and every row b with emit[b] != 0, copy row b (row_bytes[k] bytes,
 *      a multiple of 4) of src[k] over row b of dst[k]: the candidate predictor state becomes the committed one.  src / dst /
 *      row_bytes are HOST arrays of device pointers / sizes. */
#define OTR_RNNT_MAX_TGT 255
int32_t otr_rnnt_joint_fwd(const float* pe, const float* pg, const int32_t* enc_len, const int32_t* tgt_len, int32_t B, int32_t T, int32_t U1,
                           int32_t J, float* z, void* z16, void* stream);
int32_t otr_rnnt_joint_bwd(const float* dz, const float* z, const int32_t* enc_len, const int32_t* tgt_len, int32_t B, int32_t T, int32_t U1,
                           int32_t J, float* dpe, float* dpg, void* stream);
int64_t otr_rnnt_workspace_floats(int32_t B, int32_t T, int32_t U1);
int32_t otr_rnnt_loss(const float* logits, int64_t ld, const int64_t* labels, int64_t ldl, const int32_t* enc_len, const int32_t* tgt_len,
                      int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, const float* grad_scale, float* loss, float* nll,
                      int32_t* valid, float* dlogits, int64_t ldd, float* workspace, int64_t workspace_floats, void* stream);
int32_t otr_rnnt_greedy_joint(const float* pe, const float* pg_cur, const int32_t* t, const int32_t* n, const int32_t* enc_len, int32_t B,
                              int32_t T, int32_t J, int32_t max_len, float* z, void* z16, void* stream);
int32_t otr_rnnt_greedy_advance(const float* logits, int64_t ld, const int32_t* enc_len, int32_t B, int32_t T, int32_t V, int32_t blank,
                                int32_t max_symbols, int32_t max_len, int32_t* t, int32_t* n, int32_t* count, int64_t* tokens,
                                int32_t* frames, float* score, int32_t* emit, int64_t* step_tok, int32_t* remaining, void* stream);
int32_t otr_rnnt_greedy_commit(const int32_t* emit, const void* const* src, void* const* dst, const int32_t* row_bytes, int32_t n_items,
                               int32_t B, void* stream);

/* ---- the transducer's beam search (csrc/rnntbeam.hip): frame-synchronous, at most one symbol per frame, identical hypotheses merged
 *      before pruning ("modified beam search").  f32 in both builds.  Rows are R = B * W, slot r belongs to utterance r / W; W <=
 *      OTR_RNNT_BEAM_MAX, 1 <= max_len <= OTR_RNNT_BEAM_MAX_LEN, R <= 65535.  The beam of an utterance is score f32 [R] (-inf: a dead
 *      slot), n int32 [R], tokens int64 [R, max_len], frames int32 [R, max_len], held twice: a frame reads one half and writes the other.
 *      A search starts from slot 0 of every utterance at score 0 and length 0, the others dead.
 *   One frame t of utterance b, for t < T_b = enc_len[b] clamped to [0, T]: with lp_i = log-softmax of row i of the logits, every live
 *      slot i (tokens y_i, score s_i) offers its STAY (y_i, s_i + lp_i[blank]) and, if n_i < max_len, for every k != blank the EXTENSION
 *      (y_i + [k], s_i + lp_i[k]) whose new token carries frame t.  Candidates that name the same sequence are merged before pruning,
 *      scores combined with logaddexp: live hypotheses are distinct, so only the stay of i and the extension (j, k) with y_i == y_j +
 *      [k] can meet, one j per i at most; the merged candidate keeps i's frames and predictor state (it is i's stay).  The new beam is
 *      the W candidates of highest score, best first; equal scores: a stay before an extension, then the lower parent slot, then the
 *      lower token.  (Two extensions of one slot tie by their LOGITS: two different logits whose f32 scores happen to round to the
 *      same number keep the order of the logits.)  Slots that no candidate fills are dead (score -inf, n 0).  Nothing is written
 *      behind a length.
 * otr_rnnt_beam_joint: z[r,:] = tanh(pe[r / W, t, :] + pg[r,:]) with its 16-bit twin (z16 may be NULL); exact zeros for a slot that is
 *      dead (score[r] == -inf) or whose utterance has ended (t >= T_b), where pe / pg are not read.  pe f32 [B, T, J], pg f32 [R, J];
 *      J a multiple of 4; pe, pg, z 16-byte aligned.
 * otr_rnnt_beam_select: the whole frame above on logits [R, V] (row stride ld >= V, RAW; nothing behind column V is read): one
 *      workgroup per utterance, one wavefront per slot.  Per new slot, in rank order: parent[r] (the slot of the same utterance, 0 ..
 *      W - 1, the candidate came from), step_tok[r] (the new token; blank for a stay), emit[r] (1 for an extension), and score, n, tokens,
 *      frames in the OUT half: the parent's history copied, the new token appended.  A dead output slot gets score -inf, n 0, parent
 *      = itself, step_tok blank, emit 0.  An utterance with t >= T_b is carried over unchanged into the out half (parent = itself,
 *      step_tok blank, emit 0).  The partner's score s_j + lp_j[k] of a merge is read from row j of the logits whether or not k is
 *      among j's W best; if it is, that candidate is removed.  Token histories are compared directly.
 * otr_rnnt_beam_gather: for every item k < n_items (at most 16) and EVERY row r, dst[k][r] = src[k][(r / W) * W + parent[r]] (rows of
 *      row_bytes[k] bytes, a multiple of 4): the committed predictor state re-seated onto the new slots.  src / dst / row_bytes are
 *      HOST arrays as otr_rnnt_greedy_commit takes them; src[k] != dst[k] (the state is double-buffered).
 *   No atomics: the same bits on every run.  No allocation or host synchronisation.  Refused before any launch: W outside [1,
 *      OTR_RNNT_BEAM_MAX], R > 65535, max_len outside [1, OTR_RNNT_BEAM_MAX_LEN], J % 4 != 0, V < 2, ld < V, blank outside [0, V),
 *      t outside [0, T), a NULL pointer other than z16, an in half that is its out half. */
#define OTR_RNNT_BEAM_MAX 16
#define OTR_RNNT_BEAM_MAX_LEN 256
int32_t otr_rnnt_beam_joint(const float* pe, const float* pg, const float* score, const int32_t* enc_len, int32_t B, int32_t W, int32_t T,
                            int32_t t, int32_t J, float* z, void* z16, void* stream);
int32_t otr_rnnt_beam_select(const float* logits, int64_t ld, const int32_t* enc_len, int32_t B, int32_t W, int32_t T, int32_t t, int32_t V,
                             int32_t blank, int32_t max_len, const float* score_in, const int32_t* n_in, const int64_t* tokens_in,
                             const int32_t* frames_in, float* score_out, int32_t* n_out, int64_t* tokens_out, int32_t* frames_out,
                             int32_t* parent, int64_t* step_tok, int32_t* emit, void* stream);
int32_t otr_rnnt_beam_gather(const int32_t* parent, const void* const* src, void* const* dst, const int32_t* row_bytes, int32_t n_items,
                             int32_t B, int32_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OTRANS_HIP_H */
