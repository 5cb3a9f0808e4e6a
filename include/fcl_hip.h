/* fcl_hip.h — C ABI of libfcl_hip.so: the MI355X (gfx950) FCL-taco2 mel-synthesis hot path.
 *
 * The reference (Wendison/FCL-taco2) has no FFI: its plug-in point is the Python class path
 * `--model-module pkg.mod:Class` (tts_train.py:103-109).  This header is the boundary this build puts
 * UNDER that class: every entry point replaces a block of stock torch ops inside the reference's
 * nets/ modules (cited per function; paths relative to the reference root).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless the name ends in `_host`;
 *   - all activations are fp32, row-major, "channels-last": a sequence tensor is [rows, C] with
 *     rows = (utterance, time) flattened;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return 0 on success, a negative FCL_ERR_* otherwise; fcl_last_error() gives the message for the
 *     calling thread.  Nothing throws across the boundary.  Calls are re-entrant; the only global
 *     state is the thread-local error string.  The caller owns every buffer, workspaces included.
 */
#ifndef FCL_HIP_H_
#define FCL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fcl_stream_t;

enum { FCL_OK = 0, FCL_ERR_INVALID = -1, FCL_ERR_SHAPE = -2, FCL_ERR_ALIGN = -3, FCL_ERR_HIP = -4, FCL_ERR_WORKSPACE = -5 };
enum { FCL_ACT_NONE = 0, FCL_ACT_RELU = 1, FCL_ACT_TANH = 2, FCL_ACT_SIGMOID = 3 };
enum { FCL_DROP_NONE = 0, FCL_DROP_MASK = 1, FCL_DROP_RNG = 2 };
/* Bits of a DEVICE status word (uint32, caller-owned, zeroed by the caller): failures a kernel can only detect while it runs are OR-ed into
 * it instead of being lost.  fcl_adam_step refuses to update the parameters while the word is non-zero; the host reads it back next to the
 * losses (one 4-byte copy) and raises. */
enum {
    FCL_STATUS_GROUP_TIMEOUT = 1, /* a cooperating-workgroup BiLSTM kernel gave up waiting for a group member: its outputs are partial */
    /* device-built row maps (fcl_row_maps_build) and the decoder loop driven by them: */
    FCL_STATUS_ZERO_DURATION = 2, /* a non-padded phoneme has duration 0: the reference's `assert ds_nonzeros.shape[0] == hs.shape[0]`
                                   * (decoder_sa_kd.py:739) — the pass produced nothing valid */
    FCL_STATUS_LMAX_CAP = 4,      /* max duration > lmax_cap: the loop would have needed more steps than were launched (nothing was decoded) */
    FCL_STATUS_FRAMES_CAP = 8,    /* sum of durations > frames_cap: the frame-major buffers are too small (nothing was decoded) */
    FCL_STATUS_ROWS_CAP = 16,     /* live rows of a decoder step > the host's bound for that step (rows beyond the bound were not computed) */
    FCL_STATUS_VOCODER_CAP = 32,  /* fcl_pwg_maps_build: the batch has more frames than the vocoder's frames_cap, or the status word was already set when
                                   * the vocoder's maps were built: nothing is live, no waveform was generated */
    FCL_STATUS_PCM_NONFINITE = 64 /* fcl_pcm16_fwd met a NaN / Inf sample (written as 0) */
};

/* Arithmetic of the MFMA contractions (Linear / Conv1d / LSTM-step GEMMs and the weight-gradient GEMM) launched by the CALLING THREAD:
 *   FCL_GEMM_F32  (default) fp32-equivalent: both operands split into bf16 hi + lo, three MFMAs per product (or exact fp32 MFMAs under FCL_PRECISION=0);
 *   FCL_GEMM_BF16 the autocast form of mixed-precision training (the reference trains under apex AMP O1, tts.py:414-416; bf16 replaces its fp16 and
 *                 needs no loss scaling): both operands ROUNDED to bf16 (round to nearest even = the hi plane), one MFMA per product, fp32
 *                 accumulation, fp32 outputs.  Everything that is not a big-tile contraction keeps fp32: norms, activations, losses, the
 *                 optimizer, and the latency-bound small-row kernels (BiLSTM recurrences, decoder steps with few live rows).
 * The mode is thread-local, like torch.autocast.  Returns FCL_ERR_INVALID for an unknown mode, or for FCL_GEMM_BF16 under FCL_PRECISION=0. */
enum { FCL_GEMM_F32 = 0, FCL_GEMM_BF16 = 1 };

const char* fcl_last_error(void);
/* ABI revision of this header: bumped whenever a struct layout or a signature changes (100 = round 1; 200 = round 2: fcl_gemm_term_t.a_chunk_stride,
 * fcl_pwg_layer_t, the round-2 entry points).  A binding compares it with fcl_version() of the library it loaded before passing any struct. */
#define FCL_ABI_VERSION 423
int fcl_version(void);
void* fcl_debug_ptr(void); /* developer aid: device buffer of the last instrumented launch (FCL_PWG_TS), NULL otherwise */
int fcl_set_gemm_mode(int mode);
int fcl_get_gemm_mode(void);

/* ---- plan-time weight packing (run once per checkpoint) ------------------------------------------ */

/* torch Conv1d weight [Cout, Cin, k] -> tap-major [k, Cout, Cin], each output channel optionally
 * multiplied by scale[Cout] (eval BatchNorm folded into the conv; encoder_sa.py:61-78,
 * decoder_sa.py:199-263). */
int fcl_pack_conv1d_weight(const float* w, const float* scale, float* out, int cout, int cin, int k, fcl_stream_t stream);

/* Eval BatchNorm1d -> per-channel scale = gamma/sqrt(var+eps), shift = beta - mean*scale. */
int fcl_fold_batchnorm(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                       float* scale, float* shift, int c, fcl_stream_t stream);

/* dst[r, 0:cols] = src[r, 0:cols] (strided 2-D copy; splits LSTMCell.weight_ih / feat_out.weight into
 * their att_c / prenet / position column blocks, decoder_sa.py:357-369,397-398). */
int fcl_copy2d(float* dst, int ld_dst, const float* src, int ld_src, int rows, int cols, fcl_stream_t stream);

/* *p += v on the stream (a graph-capturable way to advance the dropout seed word). */
int fcl_u32_add(uint32_t* p, uint32_t v, fcl_stream_t stream);

/* bf16x3 operand planes of a weight matrix w [rows, cols] in MFMA-FRAGMENT-MAJOR order: hi = bf16_rn(x), lo = bf16_rn(x - hi),
 * stored as blocks (tile = row/16, step = col/32) of 64 lanes x 8 bf16, lane (r = lane&15, q = lane>>4) holding
 * w[tile*16 + r][step*32 + q*8 .. +7] (zero past rows/cols): element index ((tile*nsteps + step)*64 + lane)*8, nsteps =
 * ceil(cols/32).  One wave-wide 16-byte load then reads 1 KB contiguous = exactly one v_mfma_f32_16x16x32_bf16 B operand.
 * fcl_frag_bf16_elems() gives the plane length in uint16 elements.  Optional plan-time step for the decoder's small tiles. */
size_t fcl_frag_bf16_elems(int rows, int cols);
int fcl_pack_frag_bf16(const float* w, int rows, int cols, uint16_t* hi, uint16_t* lo, fcl_stream_t stream);
/* the same fragment order in fp32 (fcl_frag_bf16_elems(rows, cols) floats): lane (r16, kq) of (16-row tile, 32-k step) holds W[row][32 st + 4 kq + 0..3]
 * and W[row][32 st + 16 + 4 kq + 0..3] -- the operand form of the exact-fp32 (FCL_PRECISION=0) feat/prenet kernel (v_mfma_f32_16x16x4_f32) */
int fcl_pack_frag_f32(const float* w, int rows, int cols, float* out, fcl_stream_t stream);

/* ---- bf16x3 operand planes ("P32" layout) -----------------------------------------------------------------------------------------
 * The default arithmetic computes a.b as a_lo.b_hi + a_hi.b_lo + a_hi.b_hi on the bf16 MFMA pipe with fp32 accumulation, hi = bf16_rn(x),
 * lo = bf16_rn(x - hi).  Operands that are consumed by a GEMM are therefore kept ALREADY SPLIT next to (or instead of) their fp32 form:
 *     P32 planes of X [R, K]: uint16 [R][ld][2][32] — per row and per block of 32 columns one 128-byte line = 32 hi | 32 lo, zeros past K;
 *     ld >= ceil(K / 32) lines per row; the buffer must be 128-byte aligned.
 * Weights are packed once at plan time (fcl_pack_planes); activations are written in this form by the kernel that produces them (the `*_p`
 * outputs below), so the GEMM main loops move whole lines global -> LDS by LDS-DMA with no register staging and no conversion work. */
size_t fcl_planes_elems(int rows, int cols); /* uint16 elements of a dense plane buffer: rows * ceil(cols / 32) * 64 */
int fcl_pack_planes(const float* x, int ld, int rows, int cols, uint16_t* out, fcl_stream_t stream);

/* out = a + b (bias_ih + bias_hh). */
int fcl_add_vec(const float* a, const float* b, float* out, int n, fcl_stream_t stream);

/* ---- H1: Encoder.embed (encoder_sa.py:58,134) ------------------------------------------------------ */
/* out[m, :] = table[ids[m], :]; ids outside [0, V) produce a zero row.  out_p (optional): the same rows as P32 planes (ceil(e/32) lines per
 * row) for the convolution that consumes them; out may then be NULL. */
int fcl_embedding_fwd(const int64_t* ids, const float* table, float* out, uint16_t* out_p, int m, int v, int e, fcl_stream_t stream);

/* H1 + the first encoder Conv1d (+ folded BatchNorm) in one launch, for CONSTANT weights (synthesis): the convolution's input rows are rows of the
 * embedding table, so with tables[tap][id][co] = sum_ci W[co, ci, tap] * E[id, ci] (built once, in float64, rounded once; [k, V, Cout] fp32)
 *   y[r, :] = act(bias + sum over tap = 0 .. k-1, in that order, of tables[tap][ids[r + tap - k/2]] where seg_lo[r] <= r + tap - k/2 < seg_hi[r])
 *             (+ residual_table[ids[r]] when residual_table != NULL: the embedding table itself, `use_residual`, V x Cout).
 * k fp32 additions of correctly rounded entries replace the k * Cin products of fcl_embedding_fwd + fcl_conv1d_planes_fwd.  An id outside [0, V)
 * contributes nothing, as the zero row fcl_embedding_fwd gives it.  y (fp32) and / or y_p (P32 planes, Cout % 32 == 0); Cout % 4 == 0.  m_dev
 * (optional DEVICE row count): rows at or beyond min(m, *m_dev) are not written. */
int fcl_embed_conv_table_fwd(const int64_t* ids, const float* tables, const float* bias, const int32_t* seg_lo, const int32_t* seg_hi,
                             const float* residual_table, float* y, uint16_t* y_p, int m, int v, int cout, int k, int act, const int32_t* m_dev,
                             fcl_stream_t stream);

/* ---- H6/H8 + every nn.Linear: y = act(x . w^T + bias) --------------------------------------------- */
/* x [M, K] (lda), w [N, K] (torch layout, ldw), y [M, N] (ldy).  K, lda, ldw multiples of 4. */
int fcl_linear_fwd(const float* x, int lda, const float* w, int ldw, const float* bias, float* y, int ldy,
                   int m, int n, int k, int act, fcl_stream_t stream);

/* ---- H2/H4/H5/H11: Conv1d over channels-last rows (encoder_sa.py:136-140, decoder_sa.py:284-286,
 *      variance_predictor.py:86-88) ------------------------------------------------------------------ */
/* y[m, :] = act( sum_j x[m + j - (k-1)/2, :] . wp[j]^T + bias ) (+ residual), with rows outside
 * [seg_lo[m], seg_hi[m]) contributing zero (zero padding at utterance edges).  wp is the packed
 * [k, Cout, Cin] weight.  residual (optional, [M, Cout]) is added after the activation. */
int fcl_conv1d_fwd(const float* x, const float* wp, const float* bias, const int32_t* seg_lo, const int32_t* seg_hi,
                   const float* residual, float* y, int m, int cin, int cout, int k, int act, fcl_stream_t stream);

/* The same two on pre-split operands: xp = P32 planes of x (ldxp lines per row), wpp = P32 planes of the weight (Linear: [N, K]; Conv1d: the
 * packed taps as one [k*Cout, Cin] matrix, i.e. fcl_pack_planes of fcl_pack_conv1d_weight's output).  y (fp32) and / or yp (P32 planes, dense:
 * ceil(N/32) lines per row, zero past N) receive the result; residual / bias as above. */
int fcl_linear_planes_fwd(const uint16_t* xp, int ldxp, const uint16_t* wpp, const float* bias, float* y, int ldy, uint16_t* yp,
                          int m, int n, int k, int act, fcl_stream_t stream);
/* round 6 (421): fcl_linear_planes_fwd + masked MSE against `target` + its gradient in ONE launch (the GEMM's epilogue) -- one KD term of the student's update
 * (e2e_tts_tacotron2_sa_kd_student.py:134-179: MSE(proj(student tap), teacher tap) over the valid rows).  With d = x . W^T - target on the rows where row_valid is
 * set (all rows when NULL): grad [m, n] (ldg) / grad_p (P32 planes) = 2 d / count, 0 on the other rows; sums[0 .. 2] += sum |d|, sum d^2, element count (fp64
 * atomics: the three slots fcl_loss_terms_batch fills for a term).  The projection itself is never stored (8 bytes per element of HBM traffic less than
 * projection + fcl_loss_terms_batch).  n % 4 == 0, target 16-byte aligned with ld_t % 4 == 0; planes kernels only (FCL_ERR_INVALID under FCL_PLANES=0 /
 * FCL_PRECISION=0). */
int fcl_linear_planes_mse_fwd(const uint16_t* xp, int ldxp, const uint16_t* wpp, const float* target, int ld_t, const uint8_t* row_valid, double count,
                              float* grad, int ldg, uint16_t* grad_p, double* sums, int m, int n, int k, fcl_stream_t stream);
int fcl_conv1d_planes_fwd(const uint16_t* xp, int ldxp, const uint16_t* wpp, const float* bias, const int32_t* seg_lo, const int32_t* seg_hi,
                          const float* residual, float* y, uint16_t* yp, int m, int cin, int cout, int k, int act, fcl_stream_t stream);
/* fcl_conv1d_planes_fwd with a DEVICE row count (round 5): m is then the capacity of the buffers and tiles at or beyond *m_dev are not computed
 * (their output rows are left untouched).  The postnet of a capacity graph: the frame buffers carry slack (decode driver: x 1.3) and the batch's real
 * frame total lives in HBM (fcl_row_maps_t.totals[0]); nothing reads the rows beyond it (/root/reference/nets/modules/decoder_sa.py:199-263). */
int fcl_conv1d_planes_rows_fwd(const uint16_t* xp, int ldxp, const uint16_t* wpp, const float* bias, const int32_t* seg_lo, const int32_t* seg_hi,
                               const float* residual, float* y, uint16_t* yp, int m, int cin, int cout, int k, int act, const int32_t* m_dev,
                               fcl_stream_t stream);

/* G independent Conv1d's of the SAME shape in one launch (the duration / pitch / energy predictors' layers, variance_predictor.py:48-66): group g
 * reads planes xp + g * x_group_stride (uint16 elements; 0 = all groups read the same input), weights wpp [G][k * Cout][Cin planes] (each group
 * packed as for fcl_conv1d_planes_fwd), bias [G][Cout], and writes y / yp GROUP-MAJOR: [G][M][Cout].  Cin <= 384, Cout % 32 == 0, k >= 3. */
/* round 6 (422): Conv1d (no bias) on pre-split operands + the train-mode BatchNorm statistics of its output from the GEMM's epilogue (encoder / postnet blocks of the
 * training forward, encoder_sa.py:61-78, decoder_sa.py:199-263): z [m, cout] as fcl_conv1d_planes_fwd; mean, invstd and the running statistics exactly as
 * fcl_bn_stats_ws_fwd(z, ...) leaves them (fp64 column sums, the last row tile of a column tile finalises; `zero_workspace` = 2 cout doubles + ceil(cout / 64) tickets,
 * zero on entry and on exit) -- one launch and one pass over z less.  Planes kernels only (FCL_ERR_INVALID under FCL_PLANES=0 / FCL_PRECISION=0). */
int fcl_conv1d_planes_bn_fwd(const uint16_t* xp, int ldxp, const uint16_t* wpp, const int32_t* seg_lo, const int32_t* seg_hi, float* z, int m, int cin, int cout, int k,
                             float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var, double* zero_workspace,
                             fcl_stream_t stream);
int fcl_conv1d_planes_group_fwd(const uint16_t* xp, int ldxp, int64_t x_group_stride, const uint16_t* wpp, const float* bias, const int32_t* seg_lo,
                                const int32_t* seg_hi, float* y, uint16_t* yp, int m, int cin, int cout, int k, int act, int groups,
                                fcl_stream_t stream);

/* ---- H4/H5: channel LayerNorm (+ the predictor's Linear(C->1) and masked_fill) ---------------------- */
/* y[m,:] = LN(x[m,:]) * gamma + beta (y may be NULL).  If lin_w != NULL:
 * scalar[m] = pad_mask[m] ? 0 : (y[m,:] . lin_w + lin_b[0])   (variance_predictor.py:90-93).
 * keep != NULL (training): the Dropout after the LayerNorm, y *= keep[m,c] * keep_scale before it is stored / fed to the head. */
int fcl_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, uint16_t* yp /* optional P32 planes of y */,
                      const float* lin_w, const float* lin_b, const uint8_t* pad_mask, const uint8_t* keep, float keep_scale,
                      float* scalar, int m, int c, fcl_stream_t stream);
/* G independent LayerNorms of the same shape in one launch: row mi of group g is read at x + g * x_group_stride + mi * ldx (so both a
 * [M][G * C] matrix -- ldx = G * C, stride C: the output of a Conv1d whose output channels are G predictors' stacked -- and a group-major
 * [G][M][C] one -- ldx = C, stride M * C -- work); gamma / beta / lin_w are [G][C], lin_b [G], pad_mask [M] (shared); y / yp / scalar are written
 * group-major ([G][M][C], [G][M]). */
int fcl_layernorm_group_fwd(const float* x, int ldx, int64_t x_group_stride, const float* gamma, const float* beta, float eps, float* y, uint16_t* yp,
                            const float* lin_w, const float* lin_b, const uint8_t* pad_mask, float* scalar, int m, int c, int groups,
                            fcl_stream_t stream);

/* ---- H4: DurationPredictor.inference rounding (ESPnet; call site ..._kd_student.py:825) ------------- */
/* out = pad_mask ? 0 : (int64) max(rint(linear_domain ? x : exp(x) - offset), 0); rint = half-to-even. */
int fcl_duration_round_fwd(const float* x, int64_t* out, int n, int linear_domain, float offset,
                           const uint8_t* pad_mask, fcl_stream_t stream);

/* ---- H5: pitch_embed + energy_embed + the decoder's `hs + p_embs + e_embs`
 *      (..._kd_student.py:837-838, decoder_sa_kd.py:734) ---------------------------------------------- */
/* out[m,c] = hs[m,c] + bp[c] + sum_j wp[c,j]*p[m+j-k/2] + be[c] + sum_j we[c,j]*e[m+j-k/2]; p_emb/e_emb
 * (optional) receive the two embeddings separately. */
int fcl_variance_embed_add_fwd(const float* hs, const float* p, const float* e, const float* wp, const float* bp,
                               const float* we, const float* be, const int32_t* seg_lo, const int32_t* seg_hi,
                               float* out, float* p_emb, float* e_emb, int m, int c, int k, fcl_stream_t stream);

/* ---- prosody control: the two entries above with per-row controls (speaking rate, pitch, energy) applied to the predictions ------------
 * The controls of padded row i are the five floats at ctl + (i / ctl_row_div) * ctl_ld:
 *   [0] duration scale a, [1] pitch scale, [2] pitch shift, [3] energy scale, [4] energy shift;  identity (1, 1, 0, 1, 0).
 * ctl_row_div = t_max: one control per utterance of the padded [B, t_max] layout; 1: one per row.  ctl == NULL: exactly the entries above.
 * Duration: d = max(rint(linear_domain ? x : exp(x) - offset), 0); if a != 1 and d >= 1: d = max(rint((float)d * a), 1) (a scaled duration is
 * never 0; a predicted 0 stays 0); then the pad mask.  ctl_ld >= 5 and ctl_row_div >= 1 when ctl != NULL. */
int fcl_duration_round_ctl_fwd(const float* x, int64_t* out, int n, int linear_domain, float offset, const uint8_t* pad_mask, const float* ctl,
                               int ctl_ld, int ctl_row_div, fcl_stream_t stream);
/* Pitch / energy: p' = fmaf(p, pitch scale, pitch shift) where (scale, shift) != (1, 0), else p unchanged (e likewise).  p_out / e_out
 * (optional, must not alias p / e) receive p' / e'; the embed stencil reads the same p' / e'.  out, p_emb, e_emb may all be NULL (no weights or
 * segments are read then): a launch that only writes the controlled scalars. */
int fcl_variance_embed_add_ctl_fwd(const float* hs, const float* p, const float* e, const float* wp, const float* bp, const float* we,
                                   const float* be, const int32_t* seg_lo, const int32_t* seg_hi, const float* ctl, int ctl_ld, int ctl_row_div,
                                   float* out, float* p_emb, float* e_emb, float* p_out, float* e_out, int m, int c, int k, fcl_stream_t stream);
/* The entry above followed by fcl_gather_rows_fwd(out, src_rows, NULL, out_p, n, c) in ONE launch, bit for bit: out_p row i (P32 planes, c % 32 == 0,
 * c / 32 lines per row) is row r = src_rows[i] of (hs + p_emb) + e_emb; r outside [0, m) gives a zero row.  The fp32 [m, c] sum is never written and only
 * the n gathered rows are computed.  wp_t / we_t are the embedding weights TAP-MAJOR ([k][c]: the transpose of wp / we [c][k]), a constant of the plan;
 * k odd, <= 31.
 * ctl == NULL: no controls.  p_out / e_out (optional, [m], must not alias p / e): the controlled scalars of all m padded rows, from the same launch.
 * n == 0 writes only p_out / e_out (src_rows and out_p may then be NULL). */
int fcl_variance_embed_rows_fwd(const float* hs, const float* p, const float* e, const float* wp_t, const float* bp, const float* we_t, const float* be,
                                const int32_t* seg_lo, const int32_t* seg_hi, const int32_t* src_rows, const float* ctl, int ctl_ld, int ctl_row_div,
                                uint16_t* out_p, float* p_out, float* e_out, int m, int n, int c, int k, fcl_stream_t stream);

/* ---- speaker embedding (..._sa.py:555-557 forward, :636-638 inference; `--spk-embed-dim`): out [M, C + S] = cat[hs, F.normalize(spemb)] over the
 *      padded [B, T] row layout (row m belongs to utterance m / t; spk [B, S]; F.normalize: x / max(||x||_2, 1e-12)).  out_p (optional, (C + S) % 32
 *      == 0): the same rows as P32 planes; out may then be NULL. */
int fcl_concat_spk_fwd(const float* hs, int ldh, const float* spk, float* out, uint16_t* out_p, int m, int c, int s, int t, fcl_stream_t stream);

/* ---- H10: position table (..._kd_student.py:845-851): pos[n, t] = t < dur[n] ? (float)t/(float)dur[n] : 0 */
int fcl_position_table_fwd(const int32_t* dur, float* pos, int n, int lmax, fcl_stream_t stream);

/* ---- H9: row gather (decoder_sa.py:467: hs[non_zero_lens_mask.eq(1)], plus the duration sort) -------- */
/* dst_p (optional): the gathered rows as P32 planes (ceil(c/32) lines per row); dst may then be NULL. */
int fcl_gather_rows_fwd(const float* src, const int32_t* idx, float* dst, uint16_t* dst_p, int n, int c, fcl_stream_t stream);

/* ---- H3: Encoder.blstm over packed sequences (encoder_sa.py:98-100,143-146) -------------------------- */
/* x [B*T, C]; lens [B] int32 (device); w_ih_* [4H, C], w_hh_* [4H, H], b_* [4H] (= bias_ih + bias_hh);
 * out [B*T, 2H] = fwd | bwd, zero past each length.  algo: 0 auto, 1 per-step launches, 2 persistent
 * register-resident recurrence (H in {8,16,32,64,128}), 3 (H = 256) four cooperating workgroups per (utterance, direction)
 * exchanging h through global memory — fastest on an idle GPU, not the default when other streams are in flight.
 * algo 3 is SINGLE-STREAM ONLY (two such kernels in flight can starve each other's groups) and needs `status`, a device status word
 * (FCL_STATUS_*): a group that times out reports there and its outputs are partial.  It is refused (per-step launches instead) when
 * 8*B workgroups do not fit the device one per CU.  status may be NULL for the other algorithms.
 * Optional P32 planes: out_p receives out as planes (for the predictor convolutions); x_p / w_ih_f_p / w_ih_r_p (all or none) are the
 * pre-split operands of the input projection, in which case x may be NULL.
 * row_maps (optional; fcl_row_maps_t is declared with fcl_row_maps_build below): also build the batch's row / frame maps, exactly as
 * fcl_row_maps_build(row_maps, stream) would.  Forced durations are known before the encoder runs, so with the persistent recurrence at H = 128
 * (the shipped encoders) the map build is one more workgroup of the recurrence's launch and leaves the pass's dependent chain; every other path
 * issues fcl_row_maps_build's launches after the recurrence.  Same contract and status bits either way. */
struct fcl_row_maps;
size_t fcl_bilstm_workspace_bytes(int b, int t, int h);
int fcl_bilstm_fwd(const float* x, const int32_t* lens, const float* w_ih_f, const float* w_hh_f, const float* b_f,
                   const float* w_ih_r, const float* w_hh_r, const float* b_r, float* out, uint16_t* out_p, const uint16_t* x_p,
                   const uint16_t* w_ih_f_p, const uint16_t* w_ih_r_p, int b, int t, int c, int h,
                   int algo, void* workspace, size_t workspace_bytes, uint32_t* status, const struct fcl_row_maps* row_maps, fcl_stream_t stream);
/* The same layer over COMPACT rows (capacity passes of synthesis: engine.Caps.rows): utterance b owns rows [utt_row0[b], utt_row0[b] + lens[b]) of
 * x [n_rows, C] and out [n_rows, 2H]; utt_row0 [B + 1] int32 (device), utt_row0[B] = the batch's row total <= n_rows.  The input projections run with
 * M = n_rows; every recurrence workgroup reads its row base once in place of b * T; rows [utt_row0[B], n_rows) of out / out_p are zeroed (they take
 * the place of the padded tails).  A row range that would pass n_rows is cut there.  H = 128 only, fp32 or pre-split operands as above; other H,
 * stacked layers and training keep the padded entry.  row_maps: the same compact universe (n = n_rows, utt_row0, row_src == NULL); built by one more
 * workgroup of the recurrence's launch when the counting-sort form applies, by fcl_row_maps_build's launches otherwise. */
size_t fcl_bilstm_rows_workspace_bytes(int n_rows, int h);
int fcl_bilstm_rows_fwd(const float* x, const int32_t* lens, const int32_t* utt_row0, const float* w_ih_f, const float* w_hh_f, const float* b_f,
                        const float* w_ih_r, const float* w_hh_r, const float* b_r, float* out, uint16_t* out_p, const uint16_t* x_p,
                        const uint16_t* w_ih_f_p, const uint16_t* w_ih_r_p, int b, int n_rows, int c, int h, void* workspace, size_t workspace_bytes,
                        const struct fcl_row_maps* row_maps, fcl_stream_t stream);

/* ---- H7 as a single step: one LSTMCell (+ zoneout) update of M rows — the building block of the decoder loop, of the per-step
 *      BiLSTM, and of the TRAINING forward, which also saves what the backward pass needs (decoder_sa.py:63-96, 500-504) ------ */
typedef struct {
    const float* A;  /* [M, K] activations (lda) */
    const float* W;  /* [4U (or N), K] weights, torch layout (ldw) */
    int lda, ldw, K; /* multiples of 4 */
    int shift;       /* conv tap row shift (GEMM terms only; 0 here) */
    const uint16_t* Whi; /* optional fragment-major bf16x3 planes of W (fcl_pack_frag_bf16) */
    const uint16_t* Wlo;
    const uint16_t* Ap;  /* optional P32 planes of A and of W (fcl_pack_planes layout; see "bf16x3 operand planes" above): when EVERY term of a */
    const uint16_t* Wp;  /* call carries both, the contraction runs on the LDS-DMA kernels of gemm_planes.hip and A / W may be NULL */
    int lda_p, ldw_p;    /* row strides of the planes in 128-byte lines (>= ceil(K / 32)) */
    int64_t a_chunk_stride; /* 0: Ap is row-major as above.  != 0: CHUNK-MAJOR planes of A -- line (row m, 32-column chunk c) at byte offset
                             * c * a_chunk_stride + m * 128 (lda_p unused): a tile's rows of one chunk are one contiguous stream, which is what
                             * the vocoder's sample-major activations use (DRAM-friendly: [chunk][row] instead of [row][chunk]) */
    const float* Wff;       /* optional (round 4, exact-fp32 mode): fcl_pack_frag_f32 of W -- small LSTM steps (K = 256 per term) keep it in registers */
} fcl_gemm_term_t;

typedef struct {
    fcl_gemm_term_t term[3]; /* gates[m, g*U+u] = sum_t A_t[m,:] . W_t[g*U+u,:] + ... */
    int nterms;
    int M, U;
    const float* G;          /* optional pre-activation init [*, 4U]; row = m*g_row_mul + g_row_add */
    long long g_row_mul, g_row_add;
    const float* bias;       /* optional [4U] */
    const float* rank1_w;    /* optional [4U]: + (step / dur[m]) * rank1_w  (the decoder's position input) */
    const int32_t* dur;
    int step;
    const float* h_in;       /* [M, U] previous hidden state.  NULL = the ZERO-STATE form: the previous hidden AND cell state are zero; neither h_in nor c
                              * is read, c is write-only, and the caller passes only the terms whose A operand is non-zero (no h_in . W_hh^T term).
                              * Bit for bit the result of zero-filled h_in / c and a zero A of the dropped term (a decoder's step 0) */
    float* h_out;            /* [M, U], must not alias h_in */
    float* c;                /* [M, U] cell state, in place (write-only in the zero-state form) */
    float zoneout;           /* expectation-form rate (0 = plain LSTMCell) */
    const uint8_t* zone_keep_h; /* optional sampled zoneout masks [M, U] (1 keeps the OLD state), in pairs */
    const uint8_t* zone_keep_c;
    const int32_t* row_len;  /* optional: row live iff step < row_len[m] (packed-sequence semantics) */
    float* out2;             /* optional copy of h: row = (out2_row_base ? out2_row_base[m] : m*out2_row_mul) + out2_row_add */
    const int32_t* out2_row_base;
    long long out2_row_mul, out2_row_add;
    int ld2, out2_col_off;
    uint16_t* h_out_p;       /* optional P32 planes of h_out (ld_hp lines per row): the next step's GEMM operand, written by the same epilogue */
    int ld_hp;
    float* save_gates;       /* optional, training: activated gates i,f,g,o [M, 4U] */
    float* save_c_new;       /* optional: raw new cell (before zoneout) [M, U] */
    float* save_c_old;       /* optional: incoming cell / hidden state [M, U] */
    float* save_h_old;
    const int32_t* m_dev;    /* optional DEVICE word: rows live in this step; the kernel processes min(M, *m_dev) rows (M then bounds the grid).
                              * Lets a decoder loop whose durations were computed on the device run without a host round trip (fcl_decoder_io_t.live_rows) */
} fcl_lstm_step_t;

int fcl_lstm_step_fwd(const fcl_lstm_step_t* args, fcl_stream_t stream);

/* ---- H6-H8 (+H9/H10 scatter): the per-phoneme-parallel decoder loop
 *      (Decoder.inference decoder_sa_kd.py:742-790; Decoder.forward :572-655) ------------------------- */
typedef struct {
    int c;     /* att_c width (= eunits) */
    int p;     /* prenet units */
    int u;     /* dunits */
    int odim;  /* mel bins */
    const float* prenet_w0; /* [P, odim] */
    const float* prenet_b0; /* [P] */
    const float* prenet_w1; /* [P, P] */
    const float* prenet_b1; /* [P] */
    const float* w0_att;    /* [4U, C]  lstm.0.cell.weight_ih[:, :C]      */
    const float* w0_pre;    /* [4U, P]  lstm.0.cell.weight_ih[:, C:C+P]   */
    const float* w0_pos;    /* [4U]     lstm.0.cell.weight_ih[:, C+P]     */
    const float* w0_hh;     /* [4U, U] */
    const float* b0;        /* [4U]     bias_ih + bias_hh */
    const float* w1_ih;     /* [4U, U] */
    const float* w1_hh;     /* [4U, U] */
    const float* b1;        /* [4U] */
    const float* wf_h;      /* [odim, U] feat_out.weight[:, :U] */
    const float* wf_att;    /* [odim, C] feat_out.weight[:, U:] */
    float zoneout_rate;     /* eval-form zoneout (decoder_sa.py:96) */
    float prenet_dropout;   /* always-on prenet dropout rate (decoder_sa.py:156-158) */
    /* optional fragment-major bf16x3 planes (fcl_pack_frag_bf16) of the matrices above; all NULL = exact-fp32 small tiles */
    const uint16_t *prenet_w0_hi, *prenet_w0_lo, *prenet_w1_hi, *prenet_w1_lo;
    const uint16_t *w0_pre_hi, *w0_pre_lo, *w0_hh_hi, *w0_hh_lo, *w1_ih_hi, *w1_ih_lo, *w1_hh_hi, *w1_hh_lo;
    const uint16_t *wf_h_hi, *wf_h_lo;
    /* optional P32 planes (fcl_pack_planes) of the GEMM-sized matrices: with all six set (and C, P, U multiples of 32) the hoists and the
     * LSTM steps with more than ~1000 live rows run on the LDS-DMA kernels, states and prenet outputs travelling between them pre-split */
    const uint16_t *w0_att_p, *wf_att_p, *w0_pre_p, *w0_hh_p, *w1_ih_p, *w1_hh_p;
    int out_act;            /* FCL_ACT_*: `output_activation_fn` on the frame fed back to the prenet in the free-running loop
                             * (decoder_sa.py:614-617; `before` keeps the raw feat_out values, the caller activates the final output :635-636) */
    const float *wf_h_ff, *prenet_w0_ff, *prenet_w1_ff; /* optional (round 4, exact-fp32 mode): fcl_pack_frag_f32 of wf_h / prenet_w0 / prenet_w1: with all
                             * three (and U = P = 256, 64 < odim <= 96) the fused feat/prenet launch keeps its weights in registers as the bf16x3 one does */
    const float *w0_pre_ff, *w0_hh_ff, *w1_ih_ff, *w1_hh_ff; /* ... and of the four LSTM matrices: the small steps' register-resident operands in that mode */
    const uint16_t* stream; /* optional (round 4): the step's weights in the consumption order of the persistent row-tile kernel
                             * (fcl_decoder_stream_pack; fcl_decoder_stream_bytes() bytes, 0 = shape not covered).  With it, the P32 planes above and
                             * a free-running loop of >= FCL_DEC_TILE_MIN_ROWS rows (no teacher forcing, taps or injected masks), fcl_decoder_loop_fwd
                             * runs the whole loop as ONE launch: 32 rows per workgroup, states resident in LDS / registers for all their steps */
    /* ---- structure options beyond the shipped recipes (round 5; /root/reference/nets/modules/decoder_sa.py:119-158, 357-369, 500-504) ----
     * prenet_layers: 0 or 2 = the two blocks above; 1 = prenet_w0 / prenet_b0 alone; 3 = a third block prenet_w2 [P, P] / prenet_b2 [P].
     * dlayers: 0 or 2 = the two cells above; 1 = cell 0 alone (w1_* / b1 unused, feat_out reads cell 0); 3 = a third cell w2_ih [4U, U],
     * w2_hh [4U, U], b2 [4U] on cell 1's new state (feat_out reads it).  Anything but (2, 2) runs the loop launch by launch on the fp32
     * operands (one GEMM per prenet block, one LSTM-step launch per cell, feat_out as a GEMM): host row counts only (fcl_decoder_io_t.live_rows
     * and tail_from are refused), prenet_keep is then [Lmax, prenet_layers, N, P], tap_lstm1 the LAST cell's state. */
    int prenet_layers;
    int dlayers;
    const float *prenet_w2, *prenet_b2, *w2_ih, *w2_hh, *b2;
    /* reduction_factor r (0 / 1 = one frame per step; decoder_sa.py:397-398, 512-516, 611-627): a step emits r frames.  wf_h / wf_att are then
     * [r * odim, .] with the rows PERMUTED to frame-major order (row j * odim + o = feat_out.weight row o * r + j), so a step's output is r
     * consecutive rows of the frame-major `before`; the last of them is the next step's prenet input.  `dur` / live rows count STEPS, frame_off
     * and the frame buffers count FRAMES (r per step).  Runs on the launch-by-launch loop (see dlayers). */
    int reduction_factor;
} fcl_decoder_weights_t;

typedef struct {
    int n;                      /* phoneme rows, SORTED by duration descending */
    int lmax;                   /* = dur[0] */
    const float* att_c;         /* [N, C]: hs + p_embs + e_embs, compacted + sorted rows */
    const int32_t* dur;         /* [N] device, > 0 */
    const int32_t* live_rows_host; /* [Lmax] HOST: rows with dur > t (non-increasing).  Exact when live_rows is NULL; otherwise an UPPER BOUND per step,
                                    * used for grid sizes and kernel selection only (never for correctness: see live_rows / status) */
    const int32_t* frame_off;   /* [N] device: output frame index of (row, t = 0) */
    const float* teacher_ys;    /* NULL = free running; else [N, Lmax, odim] teacher-forced inputs */
    int dropout_mode;           /* FCL_DROP_* for the prenet */
    const uint8_t* prenet_keep; /* FCL_DROP_MASK: [Lmax, 2, N, P] keep masks (sorted row order) */
    uint32_t seed;              /* FCL_DROP_RNG */
    const uint32_t* seed_dev;   /* optional device word added to `seed` at run time (lets a captured hipGraph
                                   draw fresh dropout masks on every replay; bump it with fcl_u32_add) */
    float* before;              /* [F, odim] frame-major decoder output (pre-postnet), F = sum(dur) */
    float* tap_prenet;          /* optional [F, P]  (KD taps, decoder_sa_kd.py:627-637) */
    float* tap_lstm0;           /* optional [F, U] */
    float* tap_lstm1;           /* optional [F, U] */
    void* workspace;
    size_t workspace_bytes;
    const uint16_t* att_c_p;    /* optional P32 planes of att_c (C/32 lines per row; fcl_gather_rows_fwd writes them); att_c may then be NULL */
    uint16_t* before_p;         /* optional out: P32 planes of `before` (ceil(odim/32) lines per row), the postnet's pre-split operand */
    const int32_t* live_rows;   /* optional [Lmax + 1] DEVICE: rows with dur > t as fcl_row_maps_build wrote them (entry Lmax and beyond: 0).  With it the
                                 * loop needs nothing from the host about the durations: every step kernel processes min(live_rows_host[t], live_rows[t])
                                 * rows, `lmax` is the number of steps LAUNCHED (>= the true maximum, else FCL_STATUS_LMAX_CAP was raised by the map
                                 * builder), and a step with more live rows than its bound raises FCL_STATUS_ROWS_CAP in `status`.  NULL: host counts are exact */
    uint32_t* status;           /* device status word (FCL_STATUS_*); required with live_rows */
    int tail_from;              /* 0 = off.  Steps tail_from .. lmax - 1 (0 < tail_from < lmax) of the rows still live then run as ONE launch of the persistent
                                 * row-tile kernel (csrc/decoder_tile.hip; needs fcl_decoder_weights_t.stream and a free-running loop without taps / injected
                                 * masks, ignored otherwise), continuing from the loop's own states: in a capacity graph (lmax = a bound with slack) the steps
                                 * beyond the durations actually seen cost one launch in all instead of three each; rows that do reach them pay ~2x per step */
} fcl_decoder_io_t;

size_t fcl_decoder_loop_workspace_bytes(const fcl_decoder_weights_t* w, int n);
/* the weight stream of the persistent row-tile decoder kernel (csrc/decoder_tile.hip): bytes (0: this U / P / odim is not covered: U = P = 256,
 * odim <= 128) and the packing of the fp32 matrices of `w` (hi | lo bf16 lines, tile-major in consumption order, swizzled for the fragment reads) */
size_t fcl_decoder_stream_bytes(const fcl_decoder_weights_t* w);
int fcl_decoder_stream_pack(const fcl_decoder_weights_t* w, void* out, size_t out_bytes, fcl_stream_t stream);
int fcl_decoder_loop_fwd(const fcl_decoder_weights_t* w, const fcl_decoder_io_t* io, fcl_stream_t stream);

/* ---- H10 on the device: the integer row / frame maps of a batch from durations that live in HBM (predicted by fcl_duration_round_fwd, or
 *      forced and uploaded), with no host round trip.  Replaces the reference's host bookkeeping — `ds_nonzeros` filter + assert
 *      (decoder_sa_kd.py:736-739), the per-phoneme position / trim / concat loops (..._kd_student.py:845-851, decoder_sa_kd.py:781-791) — and this
 *      build's own numpy version (engine.build_row_maps), to which it is bit-identical (tests/test_gpu_rowmaps.py).
 *      Rows are the non-padded (utterance, phoneme) pairs in row-major order (N = sum of phoneme counts, known to the host), or the whole padded
 *      [B, t_max] layout (row_src == NULL).
 *        dur_sorted[r], src_rows[r], frame_off[r] : rows STABLY sorted by duration descending; padded row index b*T + t; first output frame
 *                                                   (exclusive cumsum of the durations in compact order = utterance base + offset inside it)
 *        live_rows[t], t = 0 .. lmax_cap          : rows with duration > t
 *        utt_frame0[b], b = 0 .. B                : first frame of utterance b; [B] = total frames
 *        frame_lo / frame_hi [frames_cap]         : utterance frame range of every frame row (0, 0 beyond the total): the postnet's segment bounds
 *        totals[0] = total frames, totals[1] = max duration, totals[2] = zero-duration rows
 *      Violations are reported in *status (FCL_STATUS_ZERO_DURATION / LMAX_CAP / FRAMES_CAP) and live_rows is then zeroed, so a decoder loop
 *      driven by these maps does nothing instead of writing out of bounds.  Two launches (none of its own through fcl_bilstm_fwd's row_maps). */
typedef struct fcl_row_maps {
    int b, n;                   /* utterances; rows of the row universe (see row_src) */
    int lmax_cap, frames_cap;
    int t_max;                  /* with utt_row0 == NULL: utterance b owns rows [b * t_max, (b + 1) * t_max) */
    const int32_t* row_src;     /* [N] device: padded row index b*T + t of compact row i (a function of the phoneme counts alone), or NULL: the row
                                 * universe IS the padded [B, t_max] layout (n = B * t_max); padding rows carry duration 0, sort behind every real
                                 * row and add nothing to the prefix sums, so the real rows get exactly the maps of the compact form -- this is the
                                 * form whose every size is a capacity, i.e. the one a captured hipGraph can replay for any batch that fits */
    const int32_t* utt_row0;    /* [B + 1] device: row range of every utterance, or NULL (t_max) */
    const uint8_t* pad;         /* optional [N]: 1 = padding row (a duration of 0 there is not an error) */
    const int64_t* dur_i64;     /* durations as int64 (fcl_duration_round_fwd's output), row i at dur[row_src ? row_src[i] : i]; or NULL */
    const int32_t* dur_i32;     /* durations as int32 per ROW OF THE UNIVERSE (forced durations); exactly one of the two is set */
    int32_t* src_rows;          /* [N] */
    int32_t* dur_sorted;        /* [N] */
    int32_t* frame_off;         /* [N] */
    int32_t* order;             /* optional [N]: compact index of sorted row r (mask re-ordering, tests) */
    int32_t* live_rows;         /* [lmax_cap + 1] */
    int32_t* utt_frame0;        /* [B + 1] */
    int32_t* frame_lo;          /* [frames_cap] */
    int32_t* frame_hi;          /* [frames_cap] */
    int32_t* totals;            /* [4] */
    uint32_t* status;           /* device status word, OR-ed */
    int32_t* scratch;           /* optional [2 N] workspace: with it and lmax_cap <= 254 the maps are built by a one-workgroup COUNTING sort (O(N):
                                 * wave-ballot ranks per duration value, block scans), a few microseconds; without it by the O(N^2 / threads) form */
} fcl_row_maps_t;
int fcl_row_maps_build(const fcl_row_maps_t* maps, fcl_stream_t stream);

/* ---- H12: masked L1 / MSE loss sums (Tacotron2Loss ..._sa.py:26-82, Knowledge_loss ..._kd_student.py:134-179,
 *      DurationPredictorLoss) ------------------------------------------------------------------------ */
/* Over the rows with row_valid[m] != 0 (NULL = every row) and all c columns:
 *   out[0] += sum |a - b'|, out[1] += sum (a - b')^2, out[2] += number of elements,
 * with b' = b, or log(b + b_log_offset) when b_log != 0 (the duration target).  out: 3 doubles in device memory,
 * accumulated with atomics (the caller zeroes them); the masked means are out[0]/out[2] and out[1]/out[2]. */
int fcl_masked_l1_mse_fwd(const float* a, int lda, const float* b, int ldb, const uint8_t* row_valid, int m, int c,
                          int b_log, float b_log_offset, double* out, fcl_stream_t stream);

/* ---- H13: gradient primitives of the teacher-forced training step (tts.py:137-179; losses ..._sa.py:601-613).
 *      dX of every Linear / Conv1d is the forward GEMM on transposed weights (fcl_transpose2d + fcl_linear_fwd / fcl_conv1d_fwd
 *      with the taps reversed); the entries below are what the backward pass needs beyond that. ------------------------------- */
/* dW: c[n, k] += sum_m a[m, n] * b[m + shift, k]  (rows of b outside [seg_lo[m], seg_hi[m]) — or outside [0, M) when the
 * bounds are NULL — contribute zero).  Linear: shift 0; Conv1d tap j: shift = j - (k-1)/2, c = packed dW[j] ([Cout, Cin]).
 * Accumulates with fp32 atomics (the caller zeroes c once per step: gradient accumulation is the natural mode).
 * Arithmetic follows FCL_PRECISION like the forward GEMMs: bf16x3-split operands with fp32 accumulation (default) or exact fp32 MFMA (0). */
int fcl_gemm_tn_fwd(const float* a, int lda, const float* b, int ldb, float* c, int ldc, int m, int n, int k, int shift,
                    const int32_t* seg_lo, const int32_t* seg_hi, fcl_stream_t stream);
/* The same for NTAPS consecutive shifts in one launch: c + j*c_tap_stride gets shift0 + j (all taps of a Conv1d weight gradient, tap-major). */
int fcl_gemm_tn_taps_fwd(const float* a, int lda, const float* b, int ldb, float* c, int ldc, int m, int n, int k, int shift0, int ntaps,
                         size_t c_tap_stride, const int32_t* seg_lo, const int32_t* seg_hi, fcl_stream_t stream);
/* The same contraction on pre-split operands: the LDS-DMA GEMM kernels (fcl_linear_planes_fwd's) with the roles of rows and columns exchanged.
 * fcl_pack_planes_t writes TRANSPOSED planes (P32T) of x [rows, cols]: one plane row per column, ceil(rows/32) lines of 32 consecutive rows
 * (hi | lo, zero past `rows`); with ntaps > 1 plane row t*cols + c holds column c read at row m + shift0 + t (zero outside
 * [seg_lo[m], seg_hi[m]), or outside [0, rows) when the bounds are NULL): the shifted inputs of all taps of a Conv1d weight gradient.
 * out: ntaps * cols * ceil(rows/32) * 64 uint16, 128-byte aligned.
 * fcl_gemm_tn_planes: c[n_, k_] += sum_m a[m, n_] * b[m, k_] with ap_t = P32T of a [m, n] and bp_t = P32T of b [m, k] (k = ntaps * cols for
 * a tap-stacked b).  The contraction is split over workgroup slices and accumulated with fp32 atomics (the caller zeroes c once per update).
 * nblk > 0: output column k_ lands at c + (k_ / nblk) * blk_stride + n_ * ldc + k_ % nblk (nblk = Cin, blk_stride = Cout * Cin: tap-major
 * [ntaps, Cout, Cin] like fcl_gemm_tn_taps_fwd); nblk = 0: plain [n, k] with row stride ldc.  Honours fcl_set_gemm_mode. */
int fcl_pack_planes_t(const float* x, int ld, int rows, int cols, int ntaps, int shift0, const int32_t* seg_lo, const int32_t* seg_hi, uint16_t* out,
                      fcl_stream_t stream);
int fcl_gemm_tn_planes(const uint16_t* ap_t, const uint16_t* bp_t, float* c, int ldc, int m, int n, int k, int nblk, size_t blk_stride,
                       fcl_stream_t stream);
/* out[c] += sum_m x[m,c] (mode 0) | x*y (mode 1) | x*(y - b[c])/g[c] (mode 2: gamma gradient of a folded eval BatchNorm)
 * | x*(y - b[c])*g[c] (mode 3: b = batch mean, g = invstd: gamma gradient of a train-mode BatchNorm). */
int fcl_colsum_fwd(const float* x, const float* y, const float* g, const float* b, float* out, int m, int c, int mode, fcl_stream_t stream);
/* the same pass with a second output: out_x[c] += sum_m x[m,c] (optional) -- train-mode BatchNorm's dbeta beside its dgamma (mode 3), dy read once */
int fcl_colsum2_fwd(const float* x, const float* y, const float* g, const float* b, float* out, float* out_x, int m, int c, int mode, fcl_stream_t stream);
/* Weight / bias gradients of a Conv1d with ONE input channel and odd k <= 16 (the pitch / energy embeddings, ..._sa.py:435-443,
 * ..._kd_student.py:570-596): dw[c, j] += sum_m dy[m, c] * x[m + j - (k-1)/2] over the positions inside row m's utterance [seg_lo[m], seg_hi[m])
 * (null: [0, m)), db[c] += sum_m dy[m, c] (db may be null).  dw is the [C, 1, k] weight gradient, contiguous. */
int fcl_conv1d_in1_dw(const float* dy, int ldy, const float* x, const int32_t* seg_lo, const int32_t* seg_hi, float* dw, float* db, int m, int c, int k,
                      fcl_stream_t stream);
/* dst[r, 0:cols] += alpha * src[r, 0:cols] on rows with row_valid[r] != 0 (null: every row).  Strided on both sides: accumulates a
 * gradient block into a column range of weight_ih / feat_out.weight, adds residual-path gradients, masks padded rows. */
int fcl_add2d(float* dst, int ld_dst, const float* src, int ld_src, int rows, int cols, float alpha, const uint8_t* row_valid, fcl_stream_t stream);
/* y = act(x) [* keep * keep_scale]   (elementwise; the training forward keeps pre-activations for the BatchNorm gradients).
 * yp (optional): the result as P32 planes of the [n / cols, cols] matrix (cols % 32 == 0); y may then be NULL. */
int fcl_act_fwd(const float* x, const uint8_t* keep, float keep_scale, float* y, uint16_t* yp, int cols, size_t n, int act, fcl_stream_t stream);
/* dw[co, ci, j] += dwp[j, co, ci] * (scale ? scale[co] : 1): packed tap-major conv gradient back to the torch Conv1d layout. */
int fcl_unpack_conv1d_grad(const float* dwp, const float* scale, float* dw, int cout, int cin, int k, fcl_stream_t stream);
/* dz = dy * act'(y) [* keep * keep_scale]   (y = the activation's OUTPUT before dropout; act = FCL_ACT_*). */
int fcl_act_bwd(const float* dy, const float* y, const uint8_t* keep, float keep_scale, float* dz, uint16_t* dzp /* optional P32 planes of dz */,
                int cols /* row width for the planes, % 32 == 0 */, size_t n, int act, fcl_stream_t stream);
/* da (+)= (w_l1 * sign(a - b') + 2 * w_mse * (a - b')) / count on the valid rows, 0 elsewhere  (b' as in fcl_masked_l1_mse_fwd). */
int fcl_l1_mse_grad(const float* a, const float* b, const uint8_t* row_valid, int m, int c, int b_log, float b_log_offset, float w_l1,
                    float w_mse, double count, float* da, int accumulate, fcl_stream_t stream);
/* fcl_masked_l1_mse_fwd (sums[0:3] += sum|d|, sum d^2, count) and fcl_l1_mse_grad in ONE pass over a and b (C % 4 == 0).  da_planes (optional,
 * C % 32 == 0): the gradient also as P32 planes [m][C/32][2][32] for the input-gradient GEMM that consumes it (the KD projections). */
int fcl_l1_mse_loss_grad(const float* a, const float* b, const uint8_t* row_valid, int m, int c, int b_log, float b_log_offset, float w_l1,
                         float w_mse, double count, float* da, int accumulate, double* sums, uint16_t* da_planes, fcl_stream_t stream);
/* ---- round 6: the small-launch tail of the training update (csrc/fused_small.hip) ------------------------------------------------------------------
 * Every ELEMENT-WISE loss term of a step in one launch (..._kd_student.py:759-802, ..._sa.py:60-70,122-126): term k computes, over the rows of a [m, c]
 * with valid[r] != 0 (all rows when NULL),
 *     sums[0:3]  += sum |a - b'|, sum (a - b')^2, count          b' = b_log ? log(b + b_log_offset) : b          (fcl_masked_l1_mse_fwd)
 *     da          = (w_l1 sign(a - b') + 2 w_mse (a - b')) / count                                                (fcl_l1_mse_grad)
 * and, when b2 is given (the teacher's output for the same tensor: the output-KD and prosody-KD terms), the same against b2 with valid2 / w_*_2 /
 * count2 into sums2, its gradient ADDED to da -- what a second, accumulating fcl_l1_mse_loss_grad launch did.  da is written (never accumulated
 * into); da_planes (optional, c % 32 == 0): the gradient as P32 planes too.  `terms` is a HOST array (passed to the kernel by value). */
#define FCL_LOSS_MAX_TERMS 12
typedef struct {
    const float* a;
    const float* b;
    const float* b2;         /* optional second target */
    const uint8_t* valid;    /* [m] or NULL */
    const uint8_t* valid2;   /* [m] or NULL (second target) */
    float* da;               /* [m, c] */
    uint16_t* da_planes;     /* optional */
    double* sums;            /* [3] */
    double* sums2;           /* [3], required with b2 */
    int32_t m, c;
    int32_t b_log;
    float b_log_offset;
    float w_l1, w_mse;
    double count;
    float w_l1_2, w_mse_2;
    double count2;
} fcl_loss_term_t;
int fcl_loss_terms_batch(const fcl_loss_term_t* terms, int n_terms, fcl_stream_t stream);
/* dst[r, :] = row_valid[r] ? srcs[0][r, :] + ... + srcs[n_src - 1][r, :] : 0 over dense [rows, cols] matrices (cols % 4 == 0); dst_p (optional, cols % 32
 * == 0): the result as P32 planes; dst may be NULL then, and may alias a source.  `srcs` is a HOST array of n_src <= FCL_SUM_ROWS_MAX device pointers.
 * Replaces the chains of fcl_add2d that assemble a gradient from its sources (pad_packed_sequence's zero rows: row_valid). */
#define FCL_SUM_ROWS_MAX 6
int fcl_sum_rows(const float* const* srcs, int n_src, const uint8_t* row_valid, float* dst, uint16_t* dst_p, int rows, int cols, fcl_stream_t stream);
/* Train-mode BatchNorm backward, first pass, with the activation / dropout backward as its prologue: dz = (dy [+ dy2]) [* keep * keep_scale] * act'(y_act)
 * is written, and dbeta[c] += sum_m dz, dgamma[c] += sum_m dz * (z - mean[c]) * invstd[c] (fp64 accumulation) -- fcl_act_bwd + fcl_colsum2_fwd(mode 3)
 * in one pass; fcl_bn_bwd consumes dz and the two sums. */
int fcl_bn_bwd_sums(const float* dy, const float* dy2, const float* y_act, const uint8_t* keep, float keep_scale, int act, const float* z, const float* mean,
                    const float* invstd, float* dz, float* dgamma, float* dbeta, int m, int c, fcl_stream_t stream);
/* fcl_act_bwd of dy + dy2 (a gradient that arrives from two consumers); dz may be NULL when only the planes are wanted. */
int fcl_act_bwd_sum(const float* dy, const float* dy2, const float* y, const uint8_t* keep, float keep_scale, float* dz, uint16_t* dzp, int cols, size_t n, int act,
                    fcl_stream_t stream);
/* fcl_gather_rows_fwd of src + src2 + src3 (src2 / src3 optional; c % 4 == 0): dst[i, :] = sum_k src_k[idx[i], :], zero rows for idx[i] < 0. */
int fcl_gather_rows_sum_fwd(const float* src, const float* src2, const float* src3, const int32_t* idx, float* dst, uint16_t* dst_p, int n, int c,
                            fcl_stream_t stream);
/* y = act(x . w^T [+ x2 . w2^T] + bias) [+ residual]: nn.Linear on fp32 operands with an optional second (x2 [M, k2], w2 [N, k2]) pair contracted into the
 * same output and an optional residual [M, N] (row stride ldr) -- the input gradients that reach one tensor through two weights, and a gradient
 * injected at the GEMM's output, without a separate addition pass. */
int fcl_linear2_fwd(const float* x, int lda, const float* w, int ldw, int k, const float* x2, int lda2, const float* w2, int ldw2, int k2, const float* bias,
                    const float* residual, int ldr, float* y, int ldy, int m, int n, int act, fcl_stream_t stream);

/* Channel LayerNorm backward (+ the predictor's scalar head: ds = gradient of scalar[m]).  dgamma/dbeta/dlin_w/dlin_b accumulate. */
int fcl_layernorm_bwd(const float* x, const float* gamma, const float* beta, float eps, const float* dy, const float* lin_w, const float* ds,
                      const uint8_t* pad_mask, const uint8_t* keep, float keep_scale, float* dx, float* dgamma, float* dbeta, float* dlin_w,
                      float* dlin_b, int m, int c, fcl_stream_t stream);
/* Train-mode BatchNorm1d over the rows of z [M, C] (encoder_sa.py:61-78, decoder_sa.py:199-263 under model.train(): statistics over every
 * position of the padded batch).  stats: mean / 1/sqrt(biased var + eps) accumulated in fp64, running statistics updated as torch (momentum 0.1,
 * unbiased variance) when given; ONE kernel (the last workgroup of a column group to finish finalises it).  workspace: 2*C + (C+63)/64 doubles;
 * fcl_bn_stats_fwd clears it first (any content on entry), fcl_bn_stats_ws_fwd requires it ZERO on entry and leaves it zero on return (a
 * workspace allocated once per stream serves every call: no clearing launch).  act: y_act = act(gamma*zhat + beta), y_drop = y_act*keep*keep_scale.
 * bwd: dz = gamma*invstd*(dy - dbeta/M - zhat*dgamma/M) with THIS batch's dbeta = sum dy, dgamma = sum dy*zhat (fcl_colsum_fwd modes 0 / 3). */
int fcl_bn_stats_fwd(const float* z, int m, int c, float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                     double* workspace, fcl_stream_t stream);
int fcl_bn_stats_ws_fwd(const float* z, int m, int c, float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                     double* zero_workspace, fcl_stream_t stream);
/* (round 6) y_act may be NULL when y_drop / yp receive the result (a forward that keeps nothing for a backward). */
int fcl_bn_act_fwd(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta, const uint8_t* keep, float keep_scale,
                   float* y_act, float* y_drop, uint16_t* yp /* optional P32 planes of the block output (after dropout), C % 32 == 0 */, int m, int c, int act,
                   fcl_stream_t stream);
int fcl_bn_bwd(const float* dy, const float* z, const float* mean, const float* invstd, const float* gamma, const float* dbeta, const float* dgamma,
               float* dz, uint16_t* dzp /* optional P32 planes of dz, C % 32 == 0 */, int m, int c,
               float* acc_dbeta, float* acc_dgamma /* optional pair: acc += this batch's dbeta / dgamma (the parameters' gradient accumulators) */,
               fcl_stream_t stream);
/* ---- the training step's time loops, enqueued by ONE call each (H13; decoder_sa.py:472-515, encoder_sa.py:143-146) ----------------------------
 * Cells are step-major: rows sorted by duration descending, cell (t, m) at offset(t) + m with offset(t) = sum_{t' < t} live_rows[t'].
 * s0 / s1 (decoder layers) and s (BiLSTM direction) are the saved tensors {gates [.,4U], c_new, c_old, h_old [.,U]} fcl_lstm_cell_bwd needs.
 * fcl_decoder_train_fwd (round 6): s0 and s1 may ALL be NULL -- a forward that keeps nothing for a backward (the frozen KD teacher) then skips those stores. */
typedef struct {
    int n, lmax, u, p;              /* sorted rows, steps, dunits, prenet units */
    const int32_t* live_rows_host;  /* [lmax] HOST */
    const float* p1d;               /* [F, P] prenet output per cell (after dropout) */
    const float* g0;                /* [N, 4U] att_c . W0_att^T + b0 (hoisted out of the loop) */
    const float *w0_pre, *w0_hh, *w0_pos;
    const int32_t* dur;             /* [N] device */
    const float *w1_ih, *w1_hh, *b1;
    float zoneout;
    const uint8_t *zk_h0, *zk_c0, *zk_h1, *zk_c1; /* optional sampled zoneout masks [F, U] (1 keeps the old state), all or none */
    float* s0[4];
    float* s1[4];
    float *h0_all, *h1_all;         /* [F, U] zoneout-ed outputs of both layers */
    void* workspace;
    size_t workspace_bytes;         /* fcl_decoder_train_workspace_bytes(n, u) */
    /* optional P32 planes (all five or none; P and U multiples of 32): the prenet output per cell [F, P/32 lines] and the four weight matrices;
     * the steps with more than ~1000 live rows (~250 at U >= 512) then run on the LDS-DMA kernels, the states travelling pre-split */
    const uint16_t *p1d_p, *w0_pre_p, *w0_hh_p, *w1_ih_p, *w1_hh_p;
} fcl_decoder_train_t;
typedef struct {
    int n, lmax, u;
    const int32_t* live_rows_host;
    const float* s0[3];             /* gates, c_new, c_old of layer 0 (as saved by the forward) */
    const float* s1[3];
    float zoneout;
    const uint8_t *zk_h0, *zk_c0, *zk_h1, *zk_c1;
    const float* dh1_all;           /* [F, U] gradient w.r.t. layer-1 outputs (feat_out path + KD tap) */
    const float* dh0_all;           /* optional [F, U] extra gradient w.r.t. layer-0 outputs (KD tap) */
    const float *w1_ih_t, *w1_hh_t, *w0_hh_t; /* transposed weights [U, 4U] */
    float *dg0_all, *dg1_all;       /* out [F, 4U]: gate pre-activation gradients of every cell */
    void* workspace;
    size_t workspace_bytes;
    /* optional P32 planes (all five or none; U % 8 == 0): the transposed weights, and out: the gate gradients of every cell as planes
     * [F, 4U/32 lines].  The recurrence's three GEMMs per step then run on the pre-split-operand kernels for steps with enough live rows. */
    const uint16_t *w1_ih_t_p, *w1_hh_t_p, *w0_hh_t_p;
    uint16_t *dg0_all_p, *dg1_all_p;
    /* optional: [W1_hh^T ; W1_ih^T] as one [2U, 4U] matrix (and its planes when the five above are given): the two GEMMs that leave layer 1's gate
     * gradients are then ONE launch per step (four dependent launches per step instead of five) */
    const float* w1_cat_t;
    const uint16_t* w1_cat_t_p;
} fcl_decoder_bptt_t;
typedef struct {
    int b, t, h;
    const int32_t* lens;            /* [B] device */
    const float* gx[2];             /* per direction (0 forward, 1 reverse): x . W_ih^T + bias_ih + bias_hh, [B*T, 4H], rows (b, t) */
    const float* w_hh[2];           /* [4H, H] */
    float* out;                     /* [B*T, 2H]: direction d writes columns [d*H, d*H + H), zeros past each length */
    float* s[2][4];                 /* saved, t-major: gates [T, B, 4H], c_new, c_old, h_old [T, B, H]; only live cells are written */
    void* workspace;                /* fcl_bilstm_train_workspace_bytes(b, h): used by the per-step fallback (H not in {8,16,32,64,128}) */
    size_t workspace_bytes;
    uint32_t* status;               /* device status word (FCL_STATUS_*); NULL = never use the cooperating-workgroup kernel (H = 256) */
} fcl_bilstm_train_t;
typedef struct {
    int b, t, h;
    const int32_t* lens;
    const float* s[2][3];           /* gates, c_new, c_old of each direction */
    const float* d_out;             /* [B*T, ld_dout] gradient w.r.t. the layer output, ZERO on padded rows; direction d in columns [d*H, d*H + H) */
    int ld_dout;
    const float* w_hh_t[2];         /* [H, 4H] */
    float* dg[2];                   /* out, t-major [T, B, 4H]; dead cells are written as 0 */
    void* workspace;
    size_t workspace_bytes;
    uint32_t* status;               /* as in fcl_bilstm_train_t */
} fcl_bilstm_bptt_t;
size_t fcl_decoder_train_workspace_bytes(int n, int u);
int fcl_decoder_train_fwd(const fcl_decoder_train_t* args, fcl_stream_t stream);
int fcl_decoder_bptt(const fcl_decoder_bptt_t* args, fcl_stream_t stream);
size_t fcl_bilstm_train_workspace_bytes(int b, int h);
int fcl_bilstm_train_fwd(const fcl_bilstm_train_t* args, fcl_stream_t stream);
int fcl_bilstm_bptt(const fcl_bilstm_bptt_t* args, fcl_stream_t stream);
/* x *= alpha (gradient averaging after a SUM all-reduce on backends without AVG). */
int fcl_scale(float* x, size_t n, float alpha, fcl_stream_t stream);
/* out[i] = 1 with probability p_one: counter hash of (seed + *seed_dev, i).  The training path's source of dropout keep masks
 * (p_one = 1 - p) and zoneout keep-old masks (p_one = zoneout rate); not bit-compatible with torch's Philox stream by design. */
int fcl_bernoulli_u8(uint8_t* out, size_t n, float p_one, uint32_t seed, const uint32_t* seed_dev, fcl_stream_t stream);
/* Up to FCL_BERNOULLI_MAX_SITES masks in ONE launch (a training forward draws ~22 of them: one launch per site was ~10 % of its launches):
 * site k gets exactly the bytes fcl_bernoulli_u8(out, n, p_one, seed, NULL) would write.  `sites` is a HOST array (passed to the kernel by value). */
#define FCL_BERNOULLI_MAX_SITES 16
typedef struct {
    uint8_t* out;
    int64_t n;
    float p_one;
    uint32_t seed;
} fcl_bernoulli_site_t;
int fcl_bernoulli_batch(const fcl_bernoulli_site_t* sites, int n_sites, fcl_stream_t stream);
/* LSTMCell + zoneout backward of one step from the forward's saved gate activations [M,4U] (i,f,g,o), c_old and c_new (raw):
 * dgates [M,4U] (pre-activation), dh_old (zoneout keep path), dc_old.  The caller adds dgates . W_hh to dh_old.
 * dh_out2 (optional, row stride ld_dh2) is added to dh_out: the per-step output gradient next to the recurrent carry. */
int fcl_lstm_cell_bwd(const float* gates, const float* c_old, const float* c_new, const float* dh_out, const float* dh_out2, int ld_dh2,
                      const float* dc_out, float zoneout,
                      const uint8_t* zone_keep_h, const uint8_t* zone_keep_c, const int32_t* row_len, int step, float* dgates, float* dh_old,
                      float* dc_old, uint16_t* dgates_p /* optional P32 planes of dgates (4U/32 lines per row) */, int m, int u, fcl_stream_t stream);
/* dst[idx[m], :] += src[m, :]  (embedding gradient; idx == skip rows are dropped: padding_idx). */
int fcl_scatter_add_rows(const float* src, const int64_t* idx, float* dst, int m, int c, int64_t skip, fcl_stream_t stream);
int fcl_transpose2d(const float* src, float* dst, int rows, int cols, fcl_stream_t stream);
/* Batched operand forms of the parameters, one launch for any number of matrices (a training step re-derives every packed / transposed /
 * pre-split weight once per optimizer update; the frozen KD teacher once).  Descriptor i produces the [a*b, c] matrix
 *     out[(ia*b + ib), ic] = src[ia*sa + ib*sb + ic*sc]  (+ src2[same offset] when src2 != NULL)        (strides in floats, may be negative)
 * as fp32 (dst, dense, row stride c; optional) and / or as P32 planes (dst_p, ceil(c/32) lines per row, zero past c, 128-byte aligned;
 * optional).  Examples: transpose of W[r, c]: a=1, b=c, c=r, sb=1, sc=c; columns [c0, c0+n) of W: src=W+c0, b=r, c=n, sb=ld, sc=1; Conv1d taps
 * [Cout, Cin, k] -> [k, Cout, Cin]: a=k, b=Cout, c=Cin, sa=1, sb=Cin*k, sc=k; the backward's reversed, transposed taps [k, Cin, Cout]:
 * src=W+k-1, a=k, b=Cin, c=Cout, sa=-1, sb=k, sc=Cin*k; bias_ih + bias_hh: src2.
 * The table lives in DEVICE memory (the caller uploads it once and replays it); first_block = sum of fcl_derive_blocks(a, b, c) of the
 * descriptors before it, total_blocks = the sum over all.  Pointers inside the table cannot be checked here. */
typedef struct {
    const float* src;
    const float* src2;
    float* dst;
    uint16_t* dst_p;
    int32_t a, b, c;
    int32_t sa, sb, sc;
    int32_t first_block;
    int32_t reserved;
} fcl_derive_t;
int fcl_derive_blocks(int a, int b, int c);
int fcl_derive_batch(const fcl_derive_t* descs_dev, int n, int total_blocks, fcl_stream_t stream);
/* Optimizer (tts.py:173-182): *out += sum x^2 ; Adam step with clip_grad_norm_(max_norm) and the NaN guard taken from the
 * device-resident squared gradient norm, so the whole step stays on the stream.
 * step_dev: device int32 = number of updates APPLIED so far (torch's per-parameter `step`); the bias corrections use *step_dev + 1 and the
 * counter advances only when the update is applied, exactly like the reference, which does not call optimizer.step() on a NaN norm
 * (tts.py:173-179).  Deliberate deviation: an INFINITE norm is skipped as well — the reference would scale the gradients by 0, turn the
 * overflowed entries into NaN (inf * 0) and write them into the parameters.  status (optional): the update is also skipped while the device
 * status word is non-zero (a kernel of this step reported partial outputs). */
int fcl_sumsq_accum(const float* x, size_t n, double* out, fcl_stream_t stream);
int fcl_adam_step(float* p, const float* g, float* m, float* v, size_t n, const double* gradnorm_sq, float max_norm, float lr, float beta1,
                  float beta2, float eps, int32_t* step_dev, const uint32_t* status, fcl_stream_t stream);
/* fcl_adam_step with torch.optim.Adam's weight_decay (`--weight-decay`, /root/reference/tts.py:397-399, tts_distill.py:418-420): the L2 term
 * weight_decay * p is added to the clipped gradient inside the step, before the moment updates (torch's non-decoupled form). */
int fcl_adam_step_wd(float* p, const float* g, float* m, float* v, size_t n, const double* gradnorm_sq, float max_norm, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int32_t* step_dev, const uint32_t* status, fcl_stream_t stream);

/* ---- measurement hook (bench.py's live roofline figures) ------------------------------- */
/* While enabled, every GEMM / LSTM-step / BiLSTM launch is bracketed by HIP events on the stream it is
 * launched on.  fcl_prof_collect synchronises those events and returns one entry per kernel instantiation:
 * launches, summed duration, summed executed FLOPs (2*M*N*sum(K); no credit for hoisted or padded work) and
 * summed rows.  Off by default; never enabled inside a timed region. */
typedef struct {
    char name[56];
    int launches;
    double ms;
    double flops;
    double rows;
    double fill_bytes; /* round 6: bytes the launch's workgroups move global -> LDS through the CU's vector-memory path (LDS-DMA lines of the tiled GEMM /
                        * Conv1d / LSTM-step kernels: workgroups x k-chunks x (A lines + W lines) x 128 B); 0 for kernels that do not report it.  Against the
                        * measured per-CU delivery ceiling (tools/stream_probe.hip) this is the BINDING resource of those loops */
} fcl_prof_entry_t;
int fcl_prof_enable(int on);
int fcl_prof_collect(fcl_prof_entry_t* out, int max_entries);

/* ---- §8f N4 / BASELINE configs[4]: Parallel WaveGAN generator (mel -> waveform), the stage the reference delegates to the external
 *      `parallel-wavegan-decode` (inference_student.sh:20-23).  No source in the reference: the architecture is the published
 *      kan-bayashi/ParallelWaveGAN generator (v1, LJSpeech: 80 mels, hop 256 = 4*4*4*4, 30 layers / 3 stacks, 64 residual + skip channels,
 *      128 gate channels, kernel 3), restated in oracle/pwg_oracle.py (parity unpinned).  Rows are SAMPLES, time-major, utterances concatenated;
 *      seg_lo / seg_hi [M] give every row the sample range of its utterance (zero padding at utterance edges).  Needs the pre-split operand
 *      path (refused under FCL_PRECISION=0 / FCL_PLANES=0).  That tool selects its generator class by `generator_type`: the HiFi-GAN generator
 *      is the section after this one. ---------------------------------------------------------------------------------------------------- */
/* One stage of the upsampling network: nearest-neighbour stretch by `scale` + the 1 x (2*scale+1) smoothing convolution w (no bias), per channel.
 * in [frames * rate_in, c] -> out [frames * rate_in * scale, c] fp32 and / or out_p (P32 planes, ceil(c/32) lines per row, zero past c).
 * frame_utt [frames]: utterance of each mel frame; utt_off [n_utt + 1]: first frame of each utterance.  c % 4 == 0; in / out 16-byte aligned. */
int fcl_pwg_upsample_stage(const float* in, const int32_t* frame_utt, const int32_t* utt_off, int64_t frames, int rate_in, int scale, const float* w,
                           float* out, uint16_t* out_p, int c, int chunk_major /* out_p as [chunk][row] lines (fcl_gemm_term_t.a_chunk_stride) */,
                           fcl_stream_t stream);
/* Coefficient lines of the frame-rate auxiliary term (fcl_pwg_layer_t.kp).  kc [m, 8]: the upsampling network's response to the colour basis
 * e[g][c] = (g mod 5 == c) over the batch's frames (columns 5..7 unused), i.e. kc[m][g mod 5] is the weight of frame g in sample m for the five
 * frames g = f-2 .. f+2 around the sample's own frame f = m / hop.  Line of sample m: that weight at column g - w0(f), zero elsewhere, where the
 * window is w0 = 32 (f >> 5) (read from pt_a) when 2 <= f mod 32 <= 29 and w0 = 32 ((f + 16) >> 5) - 16 (read from pt_b) otherwise. */
int fcl_pwg_aux_coeff(const float* kc, int64_t m, int hop, int64_t frames, uint16_t* kp, fcl_stream_t stream);
/* The generator's input noise z ~ N(0, 1) (ParallelWaveGANGenerator.inference draws torch.randn): counter-based, reproducible per (seed, index). */
int fcl_pwg_noise(float* z, int64_t n, uint32_t seed, fcl_stream_t stream);
/* first_conv (Conv1d1x1 1 -> r): x[m, ch] = w[ch] * z[m] + b[ch], written as fp32 (optional) and as planes (row-major or chunk-major). */
int fcl_pwg_first_conv(const float* z, const float* w, const float* b, float* x, uint16_t* xp, int64_t m, int r, int chunk_major, fcl_stream_t stream);
/* One residual block (ResidualBlock.forward): dilated Conv1d(r -> 2r, ksize, dilation) + conv1x1_aux(aux -> 2r) as ONE GEMM of ksize + 1 K-terms,
 * tanh * sigmoid gate, conv1x1_out / conv1x1_skip as one GEMM, x = (out + x) * sqrt(0.5), skips += skip (= skip when first_layer). */
typedef struct {
    int64_t m;                 /* samples (rows) */
    int32_t r, aux;            /* residual (= skip = gate/2) channels, multiple of 32; auxiliary channels */
    int32_t ksize, dilation;
    int32_t first_layer;       /* != 0: skips is written, not accumulated */
    const int32_t* seg_lo;     /* [m] */
    const int32_t* seg_hi;
    float* x;                  /* [m, r] fp32, in / out */
    uint16_t* xp;              /* its planes (r/32 lines per row), in / out */
    const uint16_t* cp;        /* planes of the upsampled features [m, aux] (ceil(aux/32) lines per row) */
    const uint16_t* w_conv_p;  /* planes of the taps, tap-major [ksize * 2r, r] (fcl_pack_conv1d_weight + fcl_pack_planes) */
    const float* b_conv;       /* [2r] */
    const uint16_t* w_aux_p;   /* planes of conv1x1_aux [2r, aux] */
    const uint16_t* w_os_p;    /* planes of [conv1x1_out ; conv1x1_skip] stacked [2r, r] */
    const float* b_os;         /* [2r] = [b_out ; b_skip] */
    float* skips;              /* [m, r] */
    float* z;                  /* workspaces of the unfused path: [m, 2r] fp32 */
    uint16_t* gp;              /*             planes [m, r] */
    float* o;                  /*             [m, 2r] fp32 */
    uint16_t* xp_out;          /* != NULL: the block runs as ONE launch (r = 64, ksize = 3, aux <= 96 only) that reads x from xp and writes the new
                                * planes to xp_out (a different buffer: neighbouring tiles still read xp for their taps); x, z, gp, o are unused.
                                * In this form xp, xp_out and cp are CHUNK-MAJOR planes (line (chunk c, row m) at c * m_total * 128 + m * 128 bytes) */
    /* one-launch form only, optional (kp != NULL; cp / w_aux_p are then unused): the auxiliary term evaluated at FRAME rate.  The upsampling network
     * is linear and a sample of frame f sees frames f-2 .. f+2 only, so conv1x1_aux(upsample(c))[m] = sum_g k[m][g] * (W_aux c_in[g]): one K-chunk of 32
     * (coefficient line of the sample x the frame window of the projected features) replaces the ceil(aux/32) chunks of upsampled features. */
    const uint16_t* kp;        /* [m] coefficient lines (fcl_pwg_aux_coeff) */
    const uint16_t* pt_a;      /* planes of (W_aux c_in^T) [2r, frames]: line q of a row = frames [32q, 32q + 32) */
    const uint16_t* pt_b;      /* the same shifted by 16 frames: line q = frames [32q - 16, 32q + 16), zero where there is no frame */
    int32_t ld_pt;             /* lines per row of pt_a / pt_b (>= (frames + 16 + 31) / 32) */
    int32_t hop;               /* samples per frame: a multiple of 128 (a 128-sample tile lies inside one frame); with kp, seg_lo / seg_hi may change
                                * only at multiples of hop (utterances are whole frames): the kernel reads one pair of bounds per tile */
} fcl_pwg_layer_t;
int fcl_pwg_layer_fwd(const fcl_pwg_layer_t* a, fcl_stream_t stream);
/* last_conv_layers: wav[m] = relu(relu(skips * scale) W1^T + b1) . w2 + b2.  yp: workspace planes [m, s_ch]; h: workspace fp32 [m, s_ch]
 * (both unused, may be NULL, for s_ch = 64: one launch that reads skips once). */
int fcl_pwg_last_fwd(const float* skips, float scale, const uint16_t* w1p, const float* b1, const float* w2, float b2, uint16_t* yp, float* h, float* wav,
                     int64_t m, int s_ch, fcl_stream_t stream);

/* ---- capacity form of the vocoder: the same generator with every buffer, map and grid sized by a CAPACITY (frames_cap mel frames,
 * frames_cap * hop samples) and the live extent read from the device, so that the synthesis pass's predicted durations never have to reach the
 * host and the whole chain text -> waveform is capturable.  Restricted to the one-launch block (r = 64, ksize = 3, aux <= 96) and a hop that is a
 * multiple of 128.  No entry allocates, synchronises or copies; fcl_pwg_layer_cap_fwd opts its kernel into its dynamic LDS on first use, so
 * call it once outside a capture.
 * fcl_pwg_maps_build: ONE launch that builds every index map of a batch from the synthesis pass's frame starts utt_frame0 [batch + 1] (device):
 *      utt_off [batch + 2], frame_utt / keep [frames_cap], pad_idx / lo / hi [frames_cap + 2 * ctx * (batch + 1)], seg_lo / seg_hi
 *      [frames_cap * hop] and live [4] = {live frames, live samples, live padded rows, utterances with frames}.  On the live extent they are what
 *      the host builds for the utterances that have frames (an utterance without frames contributes nothing); frames [live, frames_cap) form one
 *      pseudo-utterance (index `batch`) that owns the rest of every buffer, so every index lies inside its target and dead rows only see dead rows.
 *      *status != 0 on entry, frame starts that do not ascend from 0, or more than frames_cap frames: live = {0, 0, 0, 0}, FCL_STATUS_VOCODER_CAP is
 *      OR-ed into *status, the whole capacity becomes the pseudo-utterance.
 * fcl_pwg_gather_pad: out [pad_cap, c] = mel[pad_idx[j]] for the live padded rows, ZERO for the rest (the synthesis buffer's rows past its total
 *      are not valid and must not enter: 0 x NaN is NaN in the frame windows next to the live / dead boundary).
 * fcl_pwg_noise_cap / fcl_pwg_first_conv_cap / fcl_pwg_layer_cap_fwd / fcl_pwg_last_cap_fwd: the exact-size entries' arithmetic on samples
 *      [0, live[1]) only (a->m / m_cap / n_cap are capacities: buffer strides and grids); the noise seed is seed + *seed_dev (seed_dev may be NULL);
 *      first_conv writes chunk-major planes.
 * fcl_pcm16_fwd: pcm[i] = clip(rint((double)wav[i] * 32767), -32768, 32767), ties to even, for i < live[1] (live NULL: i < n_cap); a non-finite
 *      sample becomes 0 and sets FCL_STATUS_PCM_NONFINITE in *status. */
int fcl_pwg_maps_build(const int32_t* utt_frame0, uint32_t* status, int batch, int64_t frames_cap, int ctx, int hop, int32_t* pad_idx, int32_t* lo, int32_t* hi,
                       int32_t* keep, int32_t* frame_utt, int32_t* utt_off, int32_t* seg_lo, int32_t* seg_hi, int32_t* live, fcl_stream_t stream);
int fcl_pwg_gather_pad(const float* mel, int64_t mel_rows, const int32_t* pad_idx, const int32_t* live, int64_t pad_cap, int c, float* out, fcl_stream_t stream);
int fcl_pwg_noise_cap(float* z, int64_t n_cap, uint32_t seed, const uint32_t* seed_dev, const int32_t* live, fcl_stream_t stream);
int fcl_pwg_first_conv_cap(const float* z, const float* w, const float* b, uint16_t* xp, int64_t m_cap, int r, const int32_t* live, fcl_stream_t stream);
int fcl_pwg_layer_cap_fwd(const fcl_pwg_layer_t* a, const int32_t* live, fcl_stream_t stream);
int fcl_pwg_last_cap_fwd(const float* skips, float scale, const uint16_t* w1p, const float* b1, const float* w2, float b2, float* wav, int64_t m_cap, int s_ch,
                         const int32_t* live, fcl_stream_t stream);
int fcl_pcm16_fwd(const float* wav, int16_t* pcm, int64_t n_cap, const int32_t* live, uint32_t* status, fcl_stream_t stream);

/* ---- HiFi-GAN generator (mel -> waveform): the second generator family `parallel-wavegan-decode` (inference_student.sh:20-23) selects by
 *      `generator_type`.  Published architecture (kan-bayashi/ParallelWaveGAN HiFiGANGenerator, v1 / LJSpeech: 80 mels, 512 channels halved per stage,
 *      transposed convolutions 8 x 8 x 2 x 2 with kernels 16 / 16 / 4 / 4, residual blocks of kernel 3 / 7 / 11 x dilations 1 / 3 / 5), restated in
 *      tests/hifigan_ref.py (parity unpinned).  Rows are SAMPLES at the stage's rate, time-major, utterances concatenated, channels contiguous.
 *      frame_utt [frames] / utt_off [n_utt + 1] (as fcl_pwg_upsample_stage) with `rate` rows per frame give every row its utterance: every
 *      convolution sees zeros outside it.  P32 convention: a producer writes the fp32 value where a residual needs it and the planes of
 *      LeakyReLU(value, slope), the next consumer's operand.  bf16x3 on the bf16 MFMA; FCL_GEMM_BF16 = hi planes only.  Refused under
 *      FCL_PRECISION=0 / FCL_PLANES=0.  No entry allocates, synchronises or copies. ---------------------------------------------------------- */
/* One Conv1d (input_conv; the building block of residual units wider than 128 channels): v = conv(xp) + bias (+ resid), 'same' zero padding
 * inside the utterance; y = v (optional), yp = planes of LeakyReLU(v, slope) (optional).  ksize odd <= 11, dilation 1..5, cout % 32 == 0. */
typedef struct {
    int64_t m;                  /* rows */
    int32_t cin, cout;          /* xp / wp carry ceil(cin / 32) lines per row */
    int32_t ksize, dilation;
    int32_t rate;               /* rows per frame */
    float slope;
    const uint16_t* xp;         /* operand planes [m, cin] */
    const uint16_t* wp;         /* planes of the taps, tap-major [ksize * cout, cin] (fcl_pack_conv1d_weight + fcl_pack_planes) */
    const float* bias;          /* [cout] */
    const int32_t* frame_utt;
    const int32_t* utt_off;
    const float* resid;         /* optional [m, cout] */
    float* y;                   /* optional [m, cout] */
    uint16_t* yp;               /* optional planes [m, cout] */
} fcl_hfg_conv_t;
int fcl_hfg_conv_fwd(const fcl_hfg_conv_t* a, fcl_stream_t stream);
/* One upsampling stage in one launch: ConvTranspose1d(cin -> cout, ksize, stride, padding, output_padding = stride % 2) on xp = planes of
 * LeakyReLU(c) [m_in, cin], computed polyphase: output row n = stride * q + p takes the ksize / stride taps of phase p from the input rows around q
 * (utterance bounds at the INPUT rate).  Writes y [m_in * stride, cout] and / or yp = planes of LeakyReLU(y, slope).  ksize must be a multiple of
 * stride and ksize - 2 * padding + stride % 2 == stride (stride x as many rows out as in); other geometries are refused (FCL_ERR_SHAPE).
 * The tap count ksize / stride (<= 8) is deliberately general: the package's padding rule (stride / 2 + stride % 2) admits ksize = 2 * stride only,
 * which is what fcl_taco2_amd/hifigan.py accepts, but the entry takes any padding that keeps the length. */
typedef struct {
    int64_t m_in;               /* input rows */
    int32_t cin, cout;          /* multiples of 32 */
    int32_t stride, ksize, padding;
    int32_t rate_in;            /* input rows per frame */
    float slope;
    int32_t reserved;
    const uint16_t* xp;
    const uint16_t* wp;         /* planes of the taps, tap-major [ksize * cout, cin]: the (cin, cout, ksize) weight with its first two dimensions swapped,
                                 * through fcl_pack_conv1d_weight + fcl_pack_planes */
    const float* bias;          /* [cout] */
    const int32_t* frame_utt;
    const int32_t* utt_off;
    float* y;
    uint16_t* yp;
} fcl_hfg_tconv_t;
int fcl_hfg_tconv_fwd(const fcl_hfg_tconv_t* a, fcl_stream_t stream);
/* One residual unit: xt = conv1(LeakyReLU(x), ksize, dilation); x' = conv2(LeakyReLU(xt), ksize, 1) + x.  ONE launch for c = 32 / 64 / 128 (xt and
 * its (ksize - 1) / 2-row halo stay in LDS); other multiples of 32 run as one launch per convolution through the workspace tp.  ksize 3 / 5 / 7 / 11,
 * dilation 1..5.  Writes x_out = x' (optional; may be x) and xp_out = planes of LeakyReLU(x', slope) (optional; NOT xp).  last != 0 (the last unit of
 * a block): cs = first ? x' * cs_scale : cs + x' * cs_scale, and csp (optional) = planes of LeakyReLU(new cs, csp_slope), the next stage's operand. */
typedef struct {
    int64_t m;
    int32_t c, ksize, dilation;
    int32_t rate;               /* rows per frame */
    int32_t first, last;
    float slope, cs_scale, csp_slope;
    int32_t reserved;
    const uint16_t* xp;         /* planes of LeakyReLU(x) */
    const float* x;             /* [m, c] */
    const uint16_t* w1p;        /* planes of the taps [ksize * c, c] */
    const float* b1;
    const uint16_t* w2p;
    const float* b2;
    const int32_t* frame_utt;
    const int32_t* utt_off;
    float* x_out;
    uint16_t* xp_out;
    float* cs;                  /* [m, c] */
    uint16_t* csp;
    uint16_t* tp;               /* workspace planes [m, c] (c > 128 only) */
} fcl_hfg_unit_t;
int fcl_hfg_unit_fwd(const fcl_hfg_unit_t* a, fcl_stream_t stream);
/* output_conv + tanh: wav [m, cout] = tanh(conv(cp, w, ksize) + b); cp = planes of LeakyReLU(c) [m, c]; w [ksize][cout][c] fp32
 * (fcl_pack_conv1d_weight); 1 <= cout <= 4. */
int fcl_hfg_out_fwd(const uint16_t* cp, const float* w, const float* b, const int32_t* frame_utt, const int32_t* utt_off, int rate, float* wav, int64_t m, int c,
                    int cout, int ksize, fcl_stream_t stream);

/* ---- capacity form of the HiFi-GAN generator: the same kernels with every buffer and grid sized by a CAPACITY (frames_cap mel frames) and the live
 * extent read from the device, so that the chain text -> waveform is capturable with this generator too (fcl_taco2_amd/hifigan.py CapacitySynth).
 * No entry allocates, synchronises or copies; each cap entry opts its kernel into its dynamic LDS on first use, so call it once outside a capture.
 * fcl_hfg_maps_build: ONE launch that builds frame_utt [frames_cap], utt_off [batch + 2] and live [4] = {live frames, live samples (frames x hop), 0,
 *      utterances with frames} (the words fcl_pcm16_fwd reads) from the synthesis pass's frame starts utt_frame0 [batch + 1] (device).  A slot without
 *      frames (utt_frame0[u] == utt_frame0[u + 1]) owns no frame; frames [live, frames_cap) belong to pseudo-utterance `batch` with
 *      utt_off[batch] = live, utt_off[batch + 1] = frames_cap, so every index lies inside its buffer.  *status != 0 on entry, frame starts that do
 *      not ascend from 0, or more than frames_cap frames: live = {0, 0, 0, 0} and the whole capacity is the pseudo-utterance; the last two also OR
 *      FCL_STATUS_VOCODER_CAP into *status, an incoming status is left as it is.  Any hop >= 1; 1 <= batch <= 1024; frames_cap * hop < 2^31.
 * fcl_hfg_conv_cap_fwd / fcl_hfg_tconv_cap_fwd / fcl_hfg_unit_cap_fwd / fcl_hfg_out_cap_fwd: the exact entries' arguments, checks and arithmetic with
 *      m / m_in read as the CAPACITY (grid and buffer extent); the rows worked on are live[0] x rate (rate_in), read by every workgroup from the
 *      device.  A live row is computed exactly as the exact entry computes it at m = live rows on the same buffers; rows at and beyond the live rows
 *      are neither read nor written in any buffer. */
int fcl_hfg_maps_build(const int32_t* utt_frame0, uint32_t* status, int batch, int64_t frames_cap, int hop, int32_t* frame_utt, int32_t* utt_off, int32_t* live,
                       fcl_stream_t stream);
int fcl_hfg_conv_cap_fwd(const fcl_hfg_conv_t* a, const int32_t* live, fcl_stream_t stream);
int fcl_hfg_tconv_cap_fwd(const fcl_hfg_tconv_t* a, const int32_t* live, fcl_stream_t stream);
int fcl_hfg_unit_cap_fwd(const fcl_hfg_unit_t* a, const int32_t* live, fcl_stream_t stream);
int fcl_hfg_out_cap_fwd(const uint16_t* cp, const float* w, const float* b, const int32_t* frame_utt, const int32_t* utt_off, int rate, float* wav, int64_t m, int c,
                        int cout, int ksize, const int32_t* live, fcl_stream_t stream);

/* ---- Griffin-Lim vocoder: mel -> waveform without a trained generator (fcl_taco2_amd/griffinlim.py; restated in float64 numpy in
 *      tests/griffinlim_ref.py).  The library links no FFT: csrc/griffinlim.hip holds an LDS-resident real FFT (complex FFT of n_fft / 2 points + split).
 * Inputs: packed mel rows [frames, n_mels] (normalised log10 mel, utterances concatenated), frames per utterance T_u, optional mel_stats [2, n_mels]
 *      (mean, std), and fs, n_fft, hop, win_length, fmin, fmax, n_iter, momentum, seed.  F = n_fft / 2 + 1 bins.
 * Mel to linear:  lm = mel * (std + 1e-8) + mean (identity without stats);  m = 10^lm;  S = max(1e-10, m @ pinv(B)^T) [frames, F].  B is the Slaney-style
 *      mel filterbank (triangles on the Slaney mel scale, area normalisation 2 / (f_hi - f_lo)); the package builds B and pinv(B) in float64 numpy and
 *      uploads pinv(B)^T [n_mels, F] as float32.
 * Window: periodic Hann of win_length, zero-padded centred to n_fft.
 * STFT per utterance: reflect-pad n_fft / 2 on both sides; frame t starts at t * hop of the padded signal; times the window; real FFT.  A signal of
 *      hop (T - 1) samples gives T frames.
 * ISTFT: per frame the inverse real FFT (imaginary parts of the DC and Nyquist bins ignored) times the window, overlap-added into n_fft + hop (T - 1)
 *      samples, divided by the window-sum-square where that exceeds FLT_MIN (left undivided elsewhere), n_fft / 2 samples dropped at both ends:
 *      hop (T - 1) samples, NOT T * hop.
 * Iteration: P = exp(2 pi i u), C_prev = 0; n_iter times { y = istft(S P); C = stft(y); A = C - momentum / (1 + momentum) C_prev; P = A / (|A| + 1e-16);
 *      C_prev = C }; the result is istft(S P).  momentum 0 is the classic form (no C_prev).
 * Initial phase: u [T, F] of utterance i from counter hashes, h(x) = the library's hash_u32 (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *      x *= 0x846ca68b; x ^= x >> 16, uint32):  u = (h(h(utt_seed[i] ^ h(t + 0x9E3779B9)) ^ (k * 0x85EBCA6B)) >> 8) * 2^-24 for local frame t and bin k
 *      (numpy twin: griffinlim.phase_uniforms).  utt_seed is a device array, so a batch equals its per-utterance runs with the same seeds.
 * Supported: n_fft 512 / 1024 / 2048, 1 <= hop <= n_fft / 2, win_length <= n_fft, and (refused by the package, by utterance, before any device call)
 *      T_u >= n_fft / (2 hop) + 2, so that the reflection is a single one; the kernels clamp and stay inside their buffers for any T_u >= 1.
 * Buffers of a batch: s [frames, F] float, p / c_prev / c_out [frames, F] complex (float pairs), fr [frames, n_fft] float, y [hop (frames - n_utt)] float:
 *      utterance i (frames utt_off[i] .. utt_off[i + 1]) owns the samples from hop (utt_off[i] - i).  frame_utt [frames] / utt_off [n_utt + 1] as
 *      fcl_hfg_*.  window [n_fft]; twiddle [n_fft] complex, W^k = exp(-2 pi i k / n_fft), computed in double.  No entry allocates, synchronises or copies.
 * fcl_gl_mel2lin_fwd: the mel-to-linear step (mel_stats optional; n_mels <= 256).
 * fcl_gl_phase_init:  p = exp(2 pi i u) from utt_seed; u_out (optional, [frames, F] float) receives u itself.
 * fcl_gl_synth_fwd:   fr = irfft(s p) x window.        fcl_gl_ola_fwd: y from fr (a gather in fixed frame order, no atomics).
 * fcl_gl_analysis_fwd: C = stft(y); the phase update into p (and c_prev, which momentum != 0 requires); c_out (optional) receives C. */
typedef struct {
    int64_t frames;
    int32_t n_fft, hop, n_utt;
    float momentum;
    const float* window;
    const float* twiddle;
    const int32_t* frame_utt;
    const int32_t* utt_off;
    const uint32_t* utt_seed;
    const float* s;
    float* p;
    float* fr;
    float* y;
    float* c_prev;
    float* c_out;
    float* u_out;
} fcl_gl_t;
int fcl_gl_mel2lin_fwd(const float* mel, const float* mel_stats, const float* pinv_t, float* s, int64_t frames, int n_mels, int bins, fcl_stream_t stream);
int fcl_gl_phase_init(const fcl_gl_t* a, fcl_stream_t stream);
int fcl_gl_synth_fwd(const fcl_gl_t* a, fcl_stream_t stream);
int fcl_gl_ola_fwd(const fcl_gl_t* a, fcl_stream_t stream);
int fcl_gl_analysis_fwd(const fcl_gl_t* a, fcl_stream_t stream);

/* ---- Feature extraction: waveform -> log-mel rows, frame energy and phoneme-level means (fcl_taco2_amd/features.py; restated in float64
 *      numpy in tests/features_ref.py).  The forward half of the Griffin-Lim block above, on the same LDS-resident FFT (csrc/gl_fft.h), same window,
 *      twiddle table and filterbank B.
 * Inputs: x, the utterances' float samples back to back; utterance u owns the samples smp_off[u] .. smp_off[u + 1] (L_u of them, any length that is
 *      at least n_fft / 2 + 1, so that the reflection at either end is a single one) and the T_u = L_u / hop + 1 (integer division) frames
 *      utt_off[u] .. utt_off[u + 1]; frame_utt [frames] / utt_off [n_utt + 1] as fcl_gl_*.
 * Frame t of an utterance: samples q = t * hop + n - n_fft / 2, n < n_fft, with q < 0 -> -q and q >= L -> 2 (L - 1) - q (reflect padding); times the
 *      window; real FFT X[k], k <= n_fft / 2 (imaginary parts of the DC and Nyquist bins zero).
 * S[k] = |X[k]|  (to mag_out [frames, n_fft / 2 + 1] when that pointer is given: tests and diagnostics; otherwise the magnitudes stay in LDS).
 * energy[f] = sqrt(sum_k S[k]^2), summed in a fixed order (no atomics).
 * mel[f, c] = log10(max(1e-10, sum_k S[k] B[c, k])); with mel_stats ([2, n_mels]: mean, std) then (v - mean[c]) / (std[c] + 1e-8).  B arrives in banded
 *      form: row c is zero outside the bins fb_lo[c] .. fb_lo[c] + (fb_off[c + 1] - fb_off[c]) and holds fb_w[fb_off[c] .. fb_off[c + 1]) there
 *      (fb_lo [n_mels], fb_off [n_mels + 1], fb_w [nnz]); the sum runs in ascending k.  n_mels <= 256.
 * A batch is bit for bit its per-utterance runs.  Supported: n_fft 512 / 1024 / 2048, 1 <= hop <= n_fft / 2; window and twiddle 8-byte aligned;
 *      frames x max(n_fft / 2 + 1, n_mels) and samples (the length of x) below 2^31.  Shorter utterances are refused by the package, by id, before any
 *      device call; the kernel clamps and stays inside x for any L_u >= 1.  No entry allocates, synchronises or copies.
 * fcl_fx_segment_mean_fwd: out[p] = the mean of v over the frames of phoneme p in ascending frame order, 0 for an empty set.  Phoneme p of utterance
 *      u = ph_utt[p] (phonemes ph_off[u] .. ph_off[u + 1]) owns the frames [a, a + dur[p]), a = utt_off[u] + the sum of dur over the utterance's
 *      earlier phonemes, cut at utt_off[u + 1].  nonzero_only != 0: only frames with mask[frame] != 0 count (phoneme-level log F0 over voiced frames). */
typedef struct {
    int64_t frames, samples;
    int32_t n_fft, hop, n_utt, n_mels, nnz, reserved;
    const float* x;
    const int32_t* smp_off;
    const int32_t* frame_utt;
    const int32_t* utt_off;
    const float* window;
    const float* twiddle;
    const int32_t* fb_lo;
    const int32_t* fb_off;
    const float* fb_w;
    const float* mel_stats;
    float* mel;
    float* energy;
    float* mag_out;
} fcl_fx_t;
int fcl_fx_logmel_fwd(const fcl_fx_t* a, fcl_stream_t stream);
int fcl_fx_segment_mean_fwd(const float* v, const float* mask, const int32_t* dur, const int32_t* ph_utt, const int32_t* ph_off, const int32_t* utt_off,
                            float* out, int64_t n_ph, int n_utt, int64_t frames, int nonzero_only, fcl_stream_t stream);

/* ---- F0 tracking: waveform -> frame-level F0 in Hz, 0 = unvoiced (fcl_taco2_amd/pitch.py; restated in float64 numpy in
 *      tests/pitch_ref.py).  YIN (de Cheveigne & Kawahara 2002) steps 1 - 5 on the frame grid of the feature extraction above, so that a track has
 *      exactly the T frames of the utterance's mel rows.
 * Inputs: x / smp_off / frame_utt / utt_off as fcl_fx_*; utterance u has L_u samples and T_u = L_u / hop + 1 frames and needs L_u >= n / 2 + 1.
 * Frame t: samples q = t * hop + j - n / 2, j < n, with q < 0 -> -q and q >= L -> 2 (L - 1) - q; NO window.  n (512 or 1024) is the pitch frame
 *      length, W = n / 2 the integration length.
 * Difference function, 0 <= tau <= tau_max + 1:  d(tau) = sum_{j < W} (x[j] - x[j + tau])^2  (= e(0) + e(tau) - 2 c(tau), e(tau) = sum_{j < W}
 *      x[j + tau]^2, c(tau) = sum_{j < W} x[j] x[j + tau]).  tau_min = floor(fs / f0_ceil), tau_max = ceil(fs / f0_floor); 2 <= tau_min < tau_max <= n / 2 - 1.
 *      The kernel sums the squared differences directly, in a fixed order, so that the error of d(tau) is relative to d(tau) itself.
 * Cumulative-mean normalisation:  d'(0) = 1;  d'(tau) = d(tau) tau / sum_{j = 1 .. tau} d(j), and 1 where that sum is 0 (digital silence).  The sum
 *      runs over ascending j in a fixed order (blocks of 8 lags in ascending j, the block totals in ascending block order); no atomics.
 * Pick: the smallest tau in [tau_min, tau_max] with d'(tau) < threshold (a float; the package's default 0.1); from there tau + 1 while tau < tau_max and
 *      d'(tau + 1) < d'(tau).  No such tau: the frame is unvoiced, F0 = 0 (tau_out 0).
 * Parabola: a, b, c = d'(tau - 1), d'(tau), d'(tau + 1); delta = (a - c) / (2 (a - 2 b + c)) clamped to [-1/2, 1/2], 0 when the denominator is <= 0;
 *      F0 = fs / (tau + delta).
 * cmnd_out (optional, [frames, tau_max + 2] float: d'(0 .. tau_max + 1)) and tau_out (optional, [frames] int32: the picked integer lag) reach memory
 *      only when given: tests and diagnostics.
 * fcl_px_short_run_fwd: f0_out[f] = f0_in[f], but 0 where f lies in a run of non-zero frames shorter than min_voiced (>= 1; 1 keeps everything); a run
 *      ends at its utterance's first and last frame, so runs never join across utterances.  f0_out must not be f0_in.
 * A batch is bit for bit its per-utterance runs.  frames x (tau_max + 2) and samples below 2^31.  Shorter utterances and a tau range outside the
 *      frame are refused by the package before any device call; the kernels clamp every index read from a device table and stay inside their
 *      buffers for any L_u >= 1.  No entry allocates, synchronises or copies. */
typedef struct {
    int64_t frames, samples;
    int32_t n, hop, n_utt, tau_min, tau_max, reserved;
    float fs, threshold;
    const float* x;
    const int32_t* smp_off;
    const int32_t* frame_utt;
    const int32_t* utt_off;
    float* f0;
    float* cmnd_out;
    int32_t* tau_out;
} fcl_px_t;
int fcl_px_yin_fwd(const fcl_px_t* a, fcl_stream_t stream);
int fcl_px_short_run_fwd(const float* f0_in, const int32_t* frame_utt, const int32_t* utt_off, float* f0_out, int64_t frames, int n_utt, int min_voiced,
                         fcl_stream_t stream);

/* Probabilistic YIN (csrc/pyin.hip; Mauch & Dixon 2014; restated in numpy, float64 and float32, in tests/pyin_ref.py): the d' rows above
 *      (cmnd_out of fcl_px_yin_fwd) -> a track chosen over the whole utterance.  Two launches between fcl_px_yin_fwd and fcl_px_short_run_fwd.
 * Tables (device, float; the package builds them in float64): thr[i - 1] = i / 100, i = 1 .. 100; cw[0 .. 100], cw[i] = sum_{j <= i} w_j with
 *      w_i = F(i / 100) - F((i - 1) / 100), F(x) = 1 - (1 - x)^18 (1 + 18 x) the Beta(2, 18) cdf; nb pitch bins, B per semitone, with centres
 *      f_bin[b] = f0_floor 2^(b / (12 B)) and descending period edges edge[j] = fs / (f0_floor 2^((j + 1/2) / (12 B))), j < nb - 1; the band's half
 *      width W bins with tri[k] = ln((W + 1 - |k - W|) / (W + 1)^2), k <= 2 W; la[v1][v2] = ln 0.99 (v1 == v2) or ln 0.01.  PA = 0.01f, FLOOR = 1e-30f.
 *      Every comparison and operation below is ONE float32 operation (no contraction), in the order written.
 * fcl_px_pyin_obs_fwd, per frame.  Candidates: rec = +inf, rec_i = 100, t = tau_min; while t <= tau_max: if d'(t) < rec { m = t; while m < tau_max and
 *      d'(m + 1) < d'(m): m += 1; lo_i = #{i : thr[i - 1] <= d'(m)}; candidate m with mass = cw[rec_i] - cw[lo_i]; rec = d'(m), rec_i = lo_i,
 *      t = m + 1 } else t += 1.  The last candidate (the global record) gets mass += PA * cw[lo_i] (product and sum rounded).  This is the pick of
 *      fcl_px_yin_fwd run once per threshold.  A row whose comparisons are all false has no candidate.
 *      Period: a, b, c = d'(m - 1), d'(m), d'(m + 1); D = (a - (b + b)) + c; delta = clamp((0.5f (a - c)) / D, -1/2, 1/2) if D > 0, else 0;
 *      p = (float)m + delta; f = fs / p.  Bin: b = #{j : edge[j] >= p}.
 *      In candidate order: ov[b] += mass; a mass strictly greater than the bin's largest so far (0 at first) sets bf0[b] = f.  pv = sum_b ov[b] over
 *      ascending b.  lv[f][b] = logf(max(ov[b], FLOOR)), lu[f] = logf(max((1 - pv) / nb, FLOOR)), bf0[f][b] (0 where no candidate with mass fell);
 *      ov_out [frames, nb] optional.  cmnd has row pitch n_lag >= tau_max + 2 (n_lag <= 520, tau_max <= 511).
 * fcl_px_pyin_viterbi_fwd, per utterance u (frames utt_off[u] .. utt_off[u + 1], T of them).  State (v, b), v = 0 voiced, index v nb + b.
 *      V0[0][b] = lv[0][b], V0[1][b] = lu[0].  Step: M[v1][b] = max_k (V[v1][b + k - W] + tri[k]) over ascending k, predecessors outside [0, nb) left
 *      out, a later k winning only when strictly greater; c0 = M[0][b] + la[0][v2], c1 = M[1][b] + la[1][v2];
 *      V'[v2][b] = (c1 > c0 ? c1 : c0) + (v2 == 0 ? lv[t][b] : lu[t]).  End: the largest V, the lowest index among equals; score[u] is that V.
 *      state [frames] int32; f0 [frames]: a voiced state gets bf0[t][b] if > 0, else f_bin[b]; an unvoiced one 0.  The backtrack runs in the same
 *      launch from one back-pointer byte per (frame, state) in the caller's workspace (frames x 2 nb bytes at least), stays inside [0, nb) and ends
 *      after T steps whatever the workspace holds.  utt_off is clamped to [0, frames]; an empty or descending slice writes score -inf only.
 * 1 <= nb <= 512, 1 <= W <= 63, n_utt <= 65535, frames x 2 nb and frames x n_lag below 2^31: otherwise FCL_ERR_SHAPE; a null pointer
 *      FCL_ERR_INVALID; a short workspace FCL_ERR_WORKSPACE; an empty batch: nothing is launched -- all before any HIP call.  No atomics; a batch is
 *      bit for bit its per-utterance runs.  No entry allocates, synchronises or copies. */
typedef struct {
    int64_t frames;
    int32_t n_utt, n_lag, tau_min, tau_max, nb, w;
    float fs;
    int32_t reserved;
    const float* cmnd;
    const float* thr;
    const float* cw;
    const float* edge;
    const float* f_bin;
    const float* tri;
    const float* la;
    const int32_t* utt_off;
    float* lv;
    float* lu;
    float* bf0;
    float* ov_out;
    void* workspace;
    size_t workspace_bytes;
    int32_t* state;
    float* f0;
    float* score;
} fcl_pyin_t;
int fcl_px_pyin_obs_fwd(const fcl_pyin_t* a, fcl_stream_t stream);
int fcl_px_pyin_viterbi_fwd(const fcl_pyin_t* a, fcl_stream_t stream);

/* ---- Resampling: waveform at fs_in -> waveform at fs_out, band-limited (fcl_taco2_amd/resample.py; restated in float64 numpy in
 *      tests/resample_ref.py).  A Kaiser-windowed sinc evaluated exactly at the L phases of the rational ratio, in front of the two blocks above.
 * fs_out / fs_in = L / M in lowest terms, s = min(1, L / M).  Z = 64 zero crossings, rho = 0.9475937167399596, beta = 14.769656459379492.
 * h(tau) = s rho sinc(s rho tau) I0(beta sqrt(1 - u^2)) / I0(beta), u = s tau / Z; h = 0 for |u| >= 1; sinc(v) = sin(pi v) / (pi v).
 * Utterance u owns the input samples smp_off_in[u] .. smp_off_in[u + 1] of x (n_in of them) and the output samples smp_off_out[u] ..
 *      smp_off_out[u + 1] of y; the package sizes the latter as n_out = (n_in L) / M (integer division).
 * Output t of an utterance: n = (t M) / L, p = (t M) mod L (64-bit integers), y[t] = sum_{j = -K .. K} c[p][j] x[n - j], c[p][j] = h(j + p / L),
 *      K = ceil(Z / s); samples outside [0, n_in) count as zero.  The sum is one float32 fma chain in ascending j; no atomics and no order that
 *      depends on the batch: a batch is bit for bit its per-utterance runs.
 * table: the coefficients, built in float64 on the host and rounded to float32, TRANSPOSED: table[(j + K) L + p] = c[p][j]  ([2 K + 1][L] floats).
 * One launch: a workgroup owns a tile of consecutive outputs of one utterance (grid: tiles of the longest utterance x n_utt), stages the input span
 *      of the tile (zero-filled past either end of the utterance) in LDS once and reads every product's sample from there.  Where a tile holds whole
 *      periods of L outputs its threads take them in the order of their phase p, so that a wave reads consecutive floats of a table row.
 * max_out: the largest n_out of the batch (it sizes the grid; an utterance whose table entry says more is cut there).
 * Supported: L, M >= 1 and coprime, K >= 1, n_utt <= 65535, samples_in and samples_out below 2^31, and an input span of 64 outputs that fits the
 *      48 KB of LDS the kernel stages in: 64 M / L + 2 K + 2 <= 12288 (ratios down to 1 / 64).  The package refuses L > 1024 and tables above 4 MB
 *      before any device call.  The kernel clamps every offset it reads from a device table and stays inside x and y for any table.
 *      n_utt == 0 or max_out == 0: nothing is launched.  No entry allocates, synchronises or copies. */
typedef struct {
    int64_t samples_in, samples_out;
    int32_t l, m, k, n_utt, max_out, reserved;
    const float* x;
    const int32_t* smp_off_in;
    const int32_t* smp_off_out;
    const float* table;
    float* y;
} fcl_rs_t;
int fcl_rs_resample_fwd(const fcl_rs_t* a, fcl_stream_t stream);

/* ---- Evaluation: mel-cepstral distortion and F0 error over a dynamic-time-warping path (fcl_taco2_amd/metrics.py, evaluate.py; restated
 *      in float64 numpy in tests/evaluate_ref.py).  Two utterances of Ta and Tb frames are compared on the frame grid of the blocks above.
 * Cepstra (fcl_ev_cepstra_fwd): for a frame's log10-mel vector L[0 .. N), N = n_mels:  c_k = ln10 sqrt(2 / N) sum_m L[m] cos(pi k (m + 1/2) / N),
 *      k = 1 .. D; c_0 is left out; 1 <= D <= min(N - 1, 40), N <= 256.  table [D][N] and bias [D] are built in float64 on the host and uploaded as
 *      float32: row k - 1 of table is ln10 sqrt(2 / N) cos(pi k (m + 1/2) / N), times (std[m] + 1e-8) where the rows are normalised mels; bias is then
 *      sum_m table_raw[k][m] mean[m], and zero for raw rows.  x [frames][N] -> c [frames][D]:  c = (sum_m table[k][m] x[m]) + bias[k], the sum ONE
 *      float32 fma chain in ascending m from 0, the bias added last.  The table is staged in LDS.
 * Local distance:  d(i, j) = sqrt(sum_k (a_i[k] - b_j[k])^2), from the differences, one float32 fma chain in ascending k.
 * DTW (fcl_ev_dtw_fwd), symmetric steps, unit weights:  C(0, 0) = d(0, 0);  C(i, j) = d(i, j) + min(C(i - 1, j - 1), C(i - 1, j), C(i, j - 1)),
 *      predecessors outside the matrix do not count.  Ties: the diagonal wins; (i - 1, j) replaces it only when strictly smaller; (i, j - 1)
 *      replaces the winner only when strictly smaller.  The path is backtracked from (Ta - 1, Tb - 1) to (0, 0) and written in forward order as
 *      (i, j) pairs; its length n satisfies max(Ta, Tb) <= n <= Ta + Tb - 1.  cost = C(Ta - 1, Tb - 1);  MCD_dB = (10 sqrt 2 / ln 10) cost / n (host).
 * Pitch (fcl_ev_path_pitch_fwd): pitch_a [frames_a] / pitch_b [frames_b] hold cents above 1 Hz, p = 1200 log2 f0, 0 (or anything not > 0) for an
 *      unvoiced frame.  Over the path cells: n_vv counts both voiced, n_vuv exactly one voiced, S = sum_vv (p_a - p_b)^2, each thread over the
 *      cells t, t + 256, ... in ascending order, then a fixed tree.  counts [n_pairs][2] = (n_vv, n_vuv), sums [n_pairs] = S.
 *      F0_RMSE_cents = sqrt(S / n_vv) (NaN for n_vv = 0) and VUV_error = n_vuv / n are formed on the host.
 * A batch of pairs is packed: pair p owns the rows a_off[p] .. a_off[p + 1] of a (Ta of them; pitch_a likewise), b_off likewise of b, the
 *      back-pointer cells cell_off[p] .. cell_off[p + 1] (cumulative Ta Tb, int64) of the workspace and the rows path_off[p] .. path_off[p + 1]
 *      (cumulative Ta + Tb - 1) of path [path_rows][2]; rows of a pair's path slice past its length are set to -1.  frames_a, frames_b, cells and
 *      path_rows are the totals the tables end at.  One workgroup per pair, no atomics and no reduction whose order depends on the batch: a batch
 *      is bit for bit its per-pair runs (path, path_len, cost, counts, sums).
 * Workspace: fcl_ev_dtw_workspace_bytes(total_cells, n_pairs) bytes; its layout is the library's own (one back-pointer per cell).
 * Supported: 1 <= Ta, Tb <= 4096 (max_ta, max_tb: the batch's largest), n_pairs <= 65535, 1 <= D <= 40.  The kernels clamp every offset they read
 *      from a device table and every index they read from the workspace or the path; a pair whose slices are smaller than its lengths need is
 *      skipped (path_len 0, cost NaN).  Whatever the inputs hold, non-finite values included, the path written is a valid warping path and every
 *      store stays inside the pair's slices.  Each entry validates before any HIP call: a null pointer FCL_ERR_INVALID; D, a length or a count out of
 *      range FCL_ERR_SHAPE; a workspace that is too small FCL_ERR_WORKSPACE; n_pairs == 0 (frames == 0): nothing is launched.  No entry allocates,
 *      synchronises or copies. */
typedef struct {
    int64_t frames_a, frames_b, cells, path_rows;
    int32_t n_pairs, d, max_ta, max_tb;
    const float* a;
    const float* b;
    const int32_t* a_off;
    const int32_t* b_off;
    const int64_t* cell_off;
    const int32_t* path_off;
    void* workspace;
    size_t workspace_bytes;
    int32_t* path;
    int32_t* path_len;
    float* cost;
    const float* pitch_a;
    const float* pitch_b;
    int32_t* counts;
    float* sums;
} fcl_ev_t;
size_t fcl_ev_dtw_workspace_bytes(int64_t total_cells, int n_pairs);
int fcl_ev_cepstra_fwd(const float* x, const float* table, const float* bias, float* c, int64_t frames, int n_mels, int d, fcl_stream_t stream);
int fcl_ev_dtw_fwd(const fcl_ev_t* a, fcl_stream_t stream);
int fcl_ev_path_pitch_fwd(const fcl_ev_t* a, fcl_stream_t stream);

/* ---- Forced alignment: flat-start Viterbi training of single-Gaussian monophone models (fcl_taco2_amd/alignment.py, align.py; restated
 *      in float64 numpy in tests/align_ref.py).  Features x [frames][D] on the frame grid of the blocks above.
 * Model: every phoneme of the inventory has K states, 1 <= K <= 3; model state m = phoneme * K + k; M states in all.  mean [M][D], ivar [M][D]
 *      (inverse variances) and gconst [M], gconst[m] = -0.5 (D ln 2pi + sum_d ln var[m][d]), are built in float64 on the host and uploaded as
 *      float32.  There are no transition probabilities: every allowed move costs 0.  1 <= M <= 1024, 1 <= D <= 40.
 * Log-likelihood (fcl_al_loglik_fwd): ll [frames][M],  ll[t][m] = fma(-0.5, q, gconst[m]),  q = sum_d (x_d - mean_d)^2 ivar_d formed from the
 *      differences as ONE float32 fma chain in ascending d from 0:  df = x_d - mean_d;  q = fma(df * df, ivar_d, q)  (df * df rounded once).  D is
 *      padded to a multiple of 4 with zero x, mean and ivar, which adds exactly 0.  The model is staged in LDS in tiles of 64 states.
 * Utterance graph: utterance u owns S_u rows; row_state [rows] is each row's model state; row_skip [rows] is 0, or j >= 2: "this row may also be
 *      entered from row r - j".  An optional phoneme on the rows [a, a + K) is expressed by row_skip[a + K] = K + 1.  max_skip is 0 or the largest
 *      row_skip of the batch (2 .. 4); a row_skip outside 2 .. max_skip, or one that points before row 0, counts as 0.
 * Viterbi (fcl_al_viterbi_fwd) over an utterance of T frames and S rows, in float32:  V(0, 0) = ll(0, row_state[0]),  V(r, 0) = -inf for r > 0;
 *      V(r, t) = ll(t, row_state[r]) + max(stay V(r, t - 1), advance V(r - 1, t - 1), skip V(r - row_skip[r], t - 1)), predecessors that do not
 *      exist do not count.  Ties: stay wins; advance replaces it only when strictly greater; skip replaces the winner only when strictly greater.
 *      The backtrack runs from (S - 1, T - 1) in the same launch.  Outputs: frame_row [frames], the row within the utterance, non-decreasing;
 *      row_begin / row_frames [rows], each row's first GLOBAL frame and its count (a skipped row: 0 frames, beginning where the next row with frames
 *      begins); score [n_utt] = V(S - 1, T - 1); ok [n_utt].  An utterance gets ok 0, score -inf, frame_row -1 and row_frames 0 (row_begin: its first
 *      frame) when it has too few frames for its mandatory rows, when its backtrack does not arrive at row 0 in frame 0 (non-finite inputs, a
 *      foreign workspace), or when its slices are too small for its lengths (or longer than max_t / max_s); the rest of the batch is unaffected.
 * A batch is packed: utterance u owns the frames frame_off[u] .. frame_off[u + 1] of ll and frame_row, the rows row_off[u] .. row_off[u + 1] of
 *      row_state / row_skip / row_begin / row_frames and the back-pointer cells cell_off[u] .. cell_off[u + 1] (cumulative S T, int64) of the
 *      workspace.  frames, rows and cells are the totals the tables end at.  One workgroup per utterance, no atomics: a batch is bit for bit its
 *      per-utterance runs.
 * Statistics (fcl_al_stats_fwd): state_off [M + 1] / state_rows [rows] list the batch's rows grouped by model state, ascending row index inside a
 *      group.  The kernel ADDS to acc_n [M] (int64: frames), acc_s [M][D] and acc_q [M][D] (float64: sum x, sum x^2), so that batches chain in
 *      stream order.  The summation order is part of the contract: one float64 chain per (state, coefficient), rows in list order, frames
 *      ascending, x and x * x (exact in double) widened before the add; the chain starts at 0 and its total is added to the accumulator.
 * Workspace: fcl_al_workspace_bytes(total_cells, n_utt) bytes; its layout is the library's own (one back-pointer byte per cell).
 * Supported: 1 <= T <= 4096 (max_t: the batch's largest), 1 <= S <= 1024 (max_s), n_utt <= 65535.  The kernels clamp every offset they read from a
 *      device table, check every move of the backtrack against [0, S), and keep every store inside the utterance's slices whatever the inputs
 *      hold.  Each entry validates before any HIP call: a null pointer FCL_ERR_INVALID; a count, a length, D, M or max_skip out of range
 *      FCL_ERR_SHAPE; a workspace that is too small FCL_ERR_WORKSPACE; an empty batch: nothing is launched.  No entry allocates, synchronises or
 *      copies. */
typedef struct {
    int64_t frames, rows, cells;
    int32_t n_utt, n_states, max_t, max_s, max_skip, reserved;
    const float* ll;
    const int32_t* frame_off;
    const int32_t* row_off;
    const int64_t* cell_off;
    const int32_t* row_state;
    const int32_t* row_skip;
    void* workspace;
    size_t workspace_bytes;
    int32_t* frame_row;
    int32_t* row_begin;
    int32_t* row_frames;
    float* score;
    int32_t* ok;
} fcl_al_t;
size_t fcl_al_workspace_bytes(int64_t total_cells, int n_utt);
int fcl_al_loglik_fwd(const float* x, const float* mean, const float* ivar, const float* gconst, float* ll, int64_t frames, int d, int n_states,
                      fcl_stream_t stream);
int fcl_al_viterbi_fwd(const fcl_al_t* a, fcl_stream_t stream);
int fcl_al_stats_fwd(const float* x, const int32_t* row_begin, const int32_t* row_frames, const int32_t* state_off, const int32_t* state_rows,
                     int64_t* acc_n, double* acc_s, double* acc_q, int64_t frames, int64_t rows, int d, int n_states, fcl_stream_t stream);
/* Forced alignment, lattice graphs (csrc/align_lattice.hip; restated in numpy in tests/align_lattice_ref.py).  fcl_al_lattice_viterbi_fwd is
 *      fcl_al_viterbi_fwd over a graph whose rows name their predecessors: the words of a transcript with all their pronunciations side by side and
 *      an optional silence between them.  The packing is that of fcl_al_t -- ll [frames][M], frame_off, row_off, cell_off, row_state and the
 *      one-byte-per-cell workspace of fcl_al_workspace_bytes -- and two tables replace row_skip / max_skip:
 *      row_pred [rows][8] int32: a slot value j >= 1 means "this row may also be entered from row r - j of the same utterance"; a slot with j <= 0
 *           or r - j < 0 does not count; the eight slots are judged independently.  Predecessors have lower indices: the rows are in topological
 *           order by construction.
 *      row_flags [rows] int32: bit 0 (FCL_AL_START) the row may hold frame 0, bit 1 (FCL_AL_FINAL) the row may hold the last frame; the other bits
 *           are ignored.
 * Recurrence, in float32:  V(r, 0) = ll(0, row_state[r]) on a START row, -inf elsewhere;  V(r, t) = ll(t, row_state[r]) + best for t > 0, where best
 *      starts as stay, V(r, t - 1); the usable slots are then visited in slot order 0 .. 7 and a slot replaces the winner only when strictly greater.
 *      The back-pointer byte is 0 for stay and 1 + slot otherwise.
 * End and backtrack: the end row r* is the FINAL row with the largest finite V(r, T - 1), the lowest row index on ties, whatever the order of the
 *      workgroup's reduction; without a FINAL row that holds a finite value the utterance fails.  The backtrack runs from (r*, T - 1) in the same
 *      launch; it is valid only if it arrives at a START row in frame 0, and every move is checked against [0, S) and against the row's own slots.
 * Outputs: frame_row [frames] (non-decreasing); row_begin / row_frames [rows], each row's first GLOBAL frame and its count -- a row off the path has
 *      0 frames and row_begin = the utterance's first global frame --; score [n_utt] = V(r*, T - 1); ok [n_utt].  A failed utterance has the form of
 *      fcl_al_viterbi_fwd: ok 0, score -inf, frame_row -1, row_frames 0 (row_begin: its first frame); the rest of the batch is unaffected.
 * Contract: a chain written as a lattice -- slot 0 = 1 on every row r > 0, slot 1 = row_skip[r] where usable, START on row 0 alone, FINAL on row
 *      S - 1 alone -- gives frame_row, row_frames, score and ok bit for bit equal to fcl_al_viterbi_fwd on finite ll, and an equal row_begin on every
 *      row with frames.
 * Supported: 1 <= T <= 4096, 1 <= S <= 1024, n_utt <= 65535, 1 <= M <= 1024.  The kernel clamps every offset, state, slot and flag it reads from
 *      device memory and keeps every store inside the utterance's slices whatever the tables hold.  One workgroup per utterance, no atomics: a batch
 *      is bit for bit its single launches.  Validation before any HIP call as in fcl_al_viterbi_fwd: a null pointer FCL_ERR_INVALID; a count, a
 *      length or M out of range FCL_ERR_SHAPE; a workspace that is too small FCL_ERR_WORKSPACE; an empty batch: nothing is launched.  The entry
 *      does not allocate, synchronise or copy. */
#define FCL_AL_START 1
#define FCL_AL_FINAL 2
typedef struct {
    int64_t frames, rows, cells;
    int32_t n_utt, n_states, max_t, max_s;
    const float* ll;
    const int32_t* frame_off;
    const int32_t* row_off;
    const int64_t* cell_off;
    const int32_t* row_state;
    const int32_t* row_pred;
    const int32_t* row_flags;
    void* workspace;
    size_t workspace_bytes;
    int32_t* frame_row;
    int32_t* row_begin;
    int32_t* row_frames;
    float* score;
    int32_t* ok;
} fcl_al_lattice_t;
int fcl_al_lattice_viterbi_fwd(const fcl_al_lattice_t* a, fcl_stream_t stream);
/* Forced alignment, Gaussian-mixture states (csrc/align_gmm.hip; restated in float64 numpy in tests/align_gmm_ref.py).  The graph, the Viterbi
 *      entry and everything above are unchanged; these three entries replace the log-likelihood and the statistics when a state has several components.
 * Model: model state m owns the components comp_off[m] .. comp_off[m + 1] (comp_off [M + 1] int32 on the device), between 1 and max_comp <= 8 of
 *      them, G <= 8192 in all (M <= G <= M max_comp).  Per component mean [G][D], ivar [G][D] and cconst [G] = ln w + gconst(var), w the component's
 *      weight inside its state; formed in float64 on the host and uploaded as float32.
 * fcl_al_gmm_loglik_fwd: ll [frames][M].  Per component l_c = fma(-0.5, q_c, cconst_c) with q_c by the chain of fcl_al_loglik_fwd (ONE float32 fma
 *      chain in ascending d from 0, D padded to a multiple of 4 by zeros).  mx = max_c l_c (a NaN wins);  ll = mx + logf(sum_c expf(l_c - mx)), the sum
 *      in float32 over the components in ascending order from 0.  A state with one component gets ll = l_0, no exp or log.  When mx is not finite,
 *      ll = mx: -inf stays -inf, NaN stays NaN, and the Viterbi entry's failure path handles the utterance.  Consequences that are part of the
 *      contract: with one component everywhere and cconst = gconst the output is bit for bit fcl_al_loglik_fwd's; a component whose l_c - mx
 *      underflows expf leaves ll bit for bit the dominant component's value.
 * fcl_al_gmm_post_fwd: gamma [frames][8] float32 from frame_state [frames] int32, the model state the alignment gave each frame (-1: a frame of an
 *      utterance without an alignment).  gamma[f][c] = expf(l_c - mx) / sum (a correctly rounded division) over the components of that state, the
 *      l_c recomputed by the same chain, the sum as above; exactly 1 for a one-component state; 0 for c beyond the state's count and for a negative
 *      frame_state.
 * fcl_al_gmm_stats_fwd ADDS to acc_w [G], acc_s [G][D], acc_q [G][D] (float64) over row_begin / row_frames and the state-grouped row lists of
 *      fcl_al_stats_fwd.  Per (component, coefficient) one float64 chain from 0, rows in list order, frames ascending; a step is
 *      g = (double)gamma, v = (double)x, p = g v (exact), w += g, s += p, q += p v, each product and each sum rounded on its own (never fused); the
 *      chain's total is then added to the accumulator.  No atomics: a batch is bit for bit its per-utterance runs, batches chain in stream order.
 * Each entry validates before any HIP call: a null pointer FCL_ERR_INVALID; D, M, G, max_comp or a count out of range FCL_ERR_SHAPE; an empty
 *      batch returns 0 and launches nothing; none allocates, synchronises or copies.  Device tables are clamped: a state's components are
 *      g0 = clamp(comp_off[m], 0, G - 1) and count = clamp(comp_off[m + 1] - g0, 1, min(max_comp, G - g0)); frame_state above M - 1 counts as M - 1;
 *      the row lists as in fcl_al_stats_fwd.  The kernels stay inside their buffers whatever the tables hold. */
int fcl_al_gmm_loglik_fwd(const float* x, const float* mean, const float* ivar, const float* cconst, const int32_t* comp_off, float* ll, int64_t frames,
                          int d, int n_states, int n_comp, int max_comp, fcl_stream_t stream);
int fcl_al_gmm_post_fwd(const float* x, const float* mean, const float* ivar, const float* cconst, const int32_t* comp_off, const int32_t* frame_state,
                        float* gamma, int64_t frames, int d, int n_states, int n_comp, int max_comp, fcl_stream_t stream);
int fcl_al_gmm_stats_fwd(const float* x, const float* gamma, const int32_t* row_begin, const int32_t* row_frames, const int32_t* state_off,
                         const int32_t* state_rows, const int32_t* comp_off, double* acc_w, double* acc_s, double* acc_q, int64_t frames, int64_t rows, int d,
                         int n_states, int n_comp, int max_comp, fcl_stream_t stream);

/* ---- Multi-resolution STFT loss: spectral convergence and log-magnitude distance of a generated waveform x against a target y, and the gradient
 *      with respect to x (fcl_taco2_amd/stft_loss.py; restated in float64 numpy in tests/stft_loss_ref.py).  One resolution (n_fft, hop,
 *      window) per call, on the LDS-resident FFT and the frame grid of the feature extraction above.
 * Inputs: x and y, the utterances' float samples back to back; utterance u owns the samples smp_off[u] .. smp_off[u + 1] of both (L_u >= n_fft / 2 + 1)
 *      and the T_u = L_u / hop + 1 frames utt_off[u] .. utt_off[u + 1]; frame_utt / utt_off / window / twiddle as fcl_fx_*.
 * Frame t: samples q = t * hop + n - n_fft / 2, n < n_fft, reflected once at either end; times the window; X[k] = rfft, k <= n_fft / 2, for x and y alike.
 *      p = re^2 + im^2, m = sqrt(max(p, 1e-7)).
 * fcl_stl_sums_fwd: frame_sums [frames, 3] float = per frame (sum_k (m_y - m_x)^2, sum_k m_y^2, sum_k |log m_y - log m_x|) over a fixed partition of the
 *      bins; utt_sums [n_utt, 3] double = each utterance's frames added in ascending order in float64 (64 contiguous chunks, then the chunk totals).
 *      The caller forms sc = sqrt(A / B) and mag = C / (frames x bins) over one utterance or the batch.
 * fcl_stl_grad_bwd: coef [n_utt, 2] float = per utterance (-g_sc / sqrt(A B), g_mag / n), the reduction folded in by the caller.
 *      dm = coef0 (m_y - m_x) - coef1 sign(log m_y - log m_x) / m_x;  G[k] = (dm / m_x) X[k] where p_x > 1e-7, else 0 (the clamp passes no gradient);
 *      fr [frames, n_fft] = w N irfft(Yh), Yh[0] = Re G[0], Yh[N / 2] = Re G[N / 2], Yh[k] = G[k] / 2 between (each one-sided bin counts once);
 *      gx[j] = the sum of fr over the frames that cover the padded position j + N / 2, then its left mirror N / 2 - j (1 <= j <= N / 2), then its right
 *      mirror N / 2 + 2 (L - 1) - j (L - 1 - N / 2 <= j <= L - 2), each in ascending frame order; accumulate != 0 adds that to gx instead of storing it.
 *      Both transforms are recomputed: nothing of size frames x bins is kept between the two entries or reaches memory.
 * No atomics: a batch is bit for bit its per-utterance runs.  Supported: n_fft 512 / 1024 / 2048, 1 <= hop <= n_fft / 2; window, twiddle, fr and utt_sums
 *      8-byte aligned; frames x n_fft and samples below 2^31.  Shorter utterances are refused by the package, by id, before any device call; the kernels
 *      clamp every index read from a device table.  No entry allocates, synchronises or copies. */
typedef struct {
    int64_t frames, samples;
    int32_t n_fft, hop, n_utt, accumulate;
    const float* x;
    const float* y;
    const int32_t* smp_off;
    const int32_t* frame_utt;
    const int32_t* utt_off;
    const float* window;
    const float* twiddle;
    float* frame_sums;
    double* utt_sums;
    const float* coef;
    float* fr;
    float* gx;
} fcl_stl_t;
int fcl_stl_sums_fwd(const fcl_stl_t* a, fcl_stream_t stream);
int fcl_stl_grad_bwd(const fcl_stl_t* a, fcl_stream_t stream);

/* ---- Mel-spectrogram loss: the L1 distance of the log10 mel spectrograms of a generated waveform x and a target y, and the gradient with respect
 *      to x (fcl_taco2_amd/mel_loss.py; restated in float64 numpy in tests/mel_loss_ref.py).  HiFi-GAN's reconstruction term.  One
 *      resolution per call: n_fft N, hop, window, and a mel matrix B [n_mels, N / 2 + 1] of contiguous bands (fb_lo / fb_off / fb_w as fcl_fx_*).
 * Inputs, utterances, frames, the reflection, the window and X = rfft(frame w) exactly as in the STFT loss above (L_u >= n_fft / 2 + 1).
 *      p = re^2 + im^2;  m = sqrt(max(p, 1e-10)) for x and for y (this floor is the mel loss's own: neither the STFT loss's 1e-7 nor
 *      fcl_fx_logmel_fwd's unclamped magnitude);  M_c = max(sum_k m_k B[c, k], 1e-10), summed in ascending k;  l_c = log10 M_c.
 * fcl_msl_sums_fwd: frame_sums [frames] float = per frame sum_c |l_x,c - l_y,c| (a fixed-order tree); utt_sums [n_utt] double = each utterance's
 *      frames added in ascending order in float64 (64 contiguous chunks that depend on the utterance's own frame count only, then the chunk totals).
 *      The caller forms D / (frames x n_mels) over one utterance or the batch.
 * fcl_msl_grad_bwd: coef [n_utt] float = per utterance kappa = g / (ln 10 n), the reduction folded in by the caller.
 *      dl_c = kappa sign(l_x,c - l_y,c) / M_x,c where sum_k m_x,k B[c, k] > 1e-10, else 0;  dm_k = sum_c B[c, k] dl_c over the channels that cover
 *      bin k in ascending c: the bin-major transpose of B, bt_off [bins + 1], bt_ch [nnz], bt_w [nnz], a list because the channels covering a bin
 *      need not be contiguous;  G[k] = (dm_k / m_x,k) X[k] where p_x > 1e-10, else 0 (neither floor passes a gradient);  from G on as
 *      fcl_stl_grad_bwd: fr [frames, n_fft] = w N irfft(Yh) with each one-sided bin counted once, then the gather over a sample's own position
 *      and its two mirrors; accumulate != 0 adds to gx.  Both transforms and the mels are recomputed: nothing of size frames x bins or
 *      frames x n_mels is kept between the two entries or reaches memory.
 * No atomics: a batch is bit for bit its per-utterance runs.  Supported: n_fft 512 / 1024 / 2048, 1 <= hop <= n_fft / 2, 1 <= n_mels <= 256,
 *      nnz >= 1; window, twiddle, fr and utt_sums 8-byte aligned; frames x n_fft and samples below 2^31.  The kernels clamp every index read from a
 *      device table.  No entry allocates, synchronises or copies. */
typedef struct {
    int64_t frames, samples;
    int32_t n_fft, hop, n_utt, accumulate, n_mels, nnz;
    const float* x;
    const float* y;
    const int32_t* smp_off;
    const int32_t* frame_utt;
    const int32_t* utt_off;
    const float* window;
    const float* twiddle;
    const int32_t* fb_lo;
    const int32_t* fb_off;
    const float* fb_w;
    const int32_t* bt_off;
    const int32_t* bt_ch;
    const float* bt_w;
    float* frame_sums;
    double* utt_sums;
    const float* coef;
    float* fr;
    float* gx;
} fcl_msl_t;
int fcl_msl_sums_fwd(const fcl_msl_t* a, fcl_stream_t stream);
int fcl_msl_grad_bwd(const fcl_msl_t* a, fcl_stream_t stream);

/* ---- Parallel WaveGAN discriminator: a stack of dilated Conv1d + LeakyReLU on the waveform, one layer per call, forward and backward
 *      (fcl_taco2_amd/pwg_discriminator.py; restated in float64 numpy in tests/pwgd_ref.py).
 * Layout: activations and gradients float32, channel-last [samples, C]; the batch packed, one row per sample, the utterances back to back.  Row t's
 *      utterance is [seg_lo[t], seg_hi[t]) (as fcl_conv1d_fwd; the kernels clamp both to [0, samples]): a tap that falls outside it reads zero.
 * A layer is 1 -> C (the first), C -> C or C -> 1 (the last), C a multiple of 16 from 16 to 128, ksize k 3 or 5, tap j at offset (j - (k - 1) / 2) d,
 *      d = dilation >= 1 (no upper limit).  Weights are tap-major: wf [k][cin][cout], wf[j][ci][co] = W[co][ci][j] of torch's Conv1d.
 * fcl_pwd_layer_fwd: y[t, co] = act(bias[co] + sum_j sum_ci x[t + (j - (k - 1) / 2) d, ci] wf[j][ci][co]); act is LeakyReLU(slope) except for the last
 *      layer (cout 1), which has none.  w = wf; bias optional; x [samples, cin], y [samples, cout].
 * fcl_pwd_layer_dx: y[t, ci] = m(h[t, ci]) sum_j sum_co g[t + (j - (k - 1) / 2) d, co] wb[j][co][ci], the gradient of the PRE-activation of the layer
 *      below: g [samples, cout] is the gradient of this layer's pre-activation, w = wb [k][cout][cin] with wb[j][co][ci] = W[co][ci][k - 1 - j] (taps
 *      reversed, transposed), h [samples, cin] the stored post-activation of this layer's input, m = 1 where h > 0, else slope (h == 0 takes the slope,
 *      as torch does).  The first layer (cin 1) has no mask: h must be null, y [samples] is the waveform gradient.
 * fcl_pwd_layer_dw: dw [k][cin][cout] (the layout of wf) = sum_t x[t + (j - (k - 1) / 2) d, ci] g[t, co]; db [cout] = sum_t g[t, co] (optional).  x is the
 *      layer's input.  Each chunk of 1024 samples leaves a partial in the workspace (fcl_pwd_dw_workspace_bytes); a second launch adds them in
 *      ascending order.  No atomics anywhere: two runs give the same bits, and a batch's activations and input gradients are bit for bit those of its
 *      per-utterance runs.
 * One arithmetic mode, exact fp32: the C -> C contractions run on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain), the rest on fmaf.  Every entry
 *      validates before any HIP call: a null pointer or a slope outside [0, 1) FCL_ERR_INVALID; channels, ksize, dilation or samples (1 .. 2^31 - 1)
 *      out of range FCL_ERR_SHAPE; x, g, w, h, y not 16-byte aligned FCL_ERR_ALIGN; a workspace that is too small FCL_ERR_WORKSPACE.  No entry
 *      allocates, synchronises or copies. */
typedef struct {
    int64_t samples;
    int32_t cin, cout, ksize, dilation;
    float slope;
    int32_t reserved;
    const float* x;
    const float* w;
    const float* bias;
    const float* h;
    const float* g;
    const int32_t* seg_lo;
    const int32_t* seg_hi;
    float* y;
    float* dw;
    float* db;
    float* workspace;
    size_t workspace_bytes;
} fcl_pwd_t;
size_t fcl_pwd_dw_workspace_bytes(int64_t samples, int cin, int cout, int ksize);
int fcl_pwd_layer_fwd(const fcl_pwd_t* a, fcl_stream_t stream);
int fcl_pwd_layer_dx(const fcl_pwd_t* a, fcl_stream_t stream);
int fcl_pwd_layer_dw(const fcl_pwd_t* a, fcl_stream_t stream);

/* ---- Parallel WaveGAN generator, training form: one residual block per call, forward (activations kept) and backward
 *      (fcl_taco2_amd/pwg_generator.py; restated in float64 numpy in tests/pwgt_ref.py).
 * Layout: as the discriminator above -- float32, channel-last, packed [samples, C], row t's utterance [seg_lo[t], seg_hi[t]), a tap outside it reads zero, no
 *      dilation limit.  R = residual = skip channels (a multiple of 16 from 16 to 64), the gate has 2 R channels, A = aux channels (a multiple of 16 from 16 to
 *      128), ksize k 3 or 5, tap j at offset (j - (k - 1) / 2) d, d = dilation >= 1.
 * Weights: w_gate [k R + A][2 R], rows j R + ci = Wconv[:, ci, j] and rows k R + ai = Waux[:, ai, 0] of torch's Conv1d; b_gate [2 R] (conv.bias; the aux
 *      convolution has none); w_out [R][2 R], columns [0, R) = Wout^T, [R, 2 R) = Wskip^T; b_out [2 R] = (b_out | b_skip).  The backward forms are
 *      permutations of them: w_dz [2 R][R] = (Wout ; Wskip) (rows: output channel, columns: gate channel), w_dx [k][2 R][R] with w_dx[j][co][ci] =
 *      Wconv[co][ci][k - 1 - j] (taps reversed), w_dc [2 R][A] = Waux.
 * fcl_pwt_block_fwd (launches pwt_gate_kernel, pwt_out_kernel):
 *      z = b_gate + sum_j x[t + (j - (k - 1) / 2) d] Wconv_j + c[t] Waux;  ab = (tanh(z[:, :R]) | sigmoid(z[:, R:])) [samples, 2 R], KEPT for the backward pass
 *      (tanhf, and 1 / (1 + expf(-z)) with a true division: the backward pass takes 1 - a^2 and b (1 - b), differences near saturation);  g = a * b;
 *      x_out = (g Wout + b_out + x) sqrt(.5);  skips = g Wskip + b_skip (first != 0) or skips + that (first == 0).  z_out (optional, for tests): z.
 * fcl_pwt_block_dx (pwt_dz_kernel, then pwt_dx_kernel when dx is given, pwt_dc_kernel when dc is given): dxo [samples, R] is the gradient of x_out and must
 *      be null exactly when last != 0 (the last block's x_out is read by nobody); ds [samples, R] the gradient of the skip sum.
 *      dg = sqrt(.5) dxo Wout^T + ds Wskip^T;  dz = (dg b (1 - a^2) | dg a b (1 - b)) [samples, 2 R], written for fcl_pwt_block_dw;
 *      dx = sum_j dz[t - (j - (k - 1) / 2) d] Wconv_j^T + sqrt(.5) dxo;  dc = dz Waux^T (last != 0) or dc + that (last == 0).
 * fcl_pwt_block_dw (pwt_dw_kernel<gate>, pwt_dw_kernel<out>, each followed by pwt_dw_reduce_kernel), after fcl_pwt_block_dx of the same block:
 *      dw_gate [k R + A][2 R] = (sum_t x[t + shift_j]^T dz[t] ; sum_t c^T dz), db_gate [2 R] = sum_t dz;  dw_out [R][2 R] = sum_t g^T (sqrt(.5) dxo | ds),
 *      db_out [2 R] = sum_t (sqrt(.5) dxo | ds); with last != 0 the Wout halves are exactly zero.  Each chunk of 1024 samples leaves a partial in the
 *      workspace (fcl_pwt_dw_workspace_bytes); a second launch adds them in ascending order.  No atomics anywhere.
 * One arithmetic mode, exact fp32: every contraction runs on v_mfma_f32_16x16x4_f32.  Every entry validates before any HIP call: a null pointer (or a dxo
 *      that contradicts last) FCL_ERR_INVALID; channels, ksize, dilation or samples (1 .. 2^31 - 1) out of range FCL_ERR_SHAPE; an activation, gradient or
 *      weight pointer not 16-byte aligned FCL_ERR_ALIGN; a workspace that is too small FCL_ERR_WORKSPACE.  No entry allocates, synchronises or copies. */
typedef struct {
    int64_t samples;
    int32_t residual, aux, ksize, dilation;
    int32_t first, last;
    const int32_t* seg_lo;
    const int32_t* seg_hi;
    const float* x;        /* [samples, R] the block's input */
    const float* c;        /* [samples, A] the conditioning */
    const float* w_gate;
    const float* b_gate;
    const float* w_out;
    const float* b_out;
    float* ab;             /* [samples, 2 R] written by fwd, read by dx and dw */
    float* x_out;          /* [samples, R] */
    float* skips;          /* [samples, R] */
    float* z_out;          /* [samples, 2 R] or null */
    const float* dxo;      /* [samples, R] or null (last) */
    const float* ds;       /* [samples, R] */
    const float* w_dz;
    const float* w_dx;
    const float* w_dc;
    float* dz;             /* [samples, 2 R] written by dx, read by dw */
    float* dx;             /* [samples, R] or null: not computed */
    float* dc;             /* [samples, A] or null: not computed */
    float* dw_gate;
    float* db_gate;
    float* dw_out;
    float* db_out;
    float* workspace;
    size_t workspace_bytes;
} fcl_pwt_t;
size_t fcl_pwt_dw_workspace_bytes(int64_t samples, int residual, int aux, int ksize);
int fcl_pwt_block_fwd(const fcl_pwt_t* a, fcl_stream_t stream);
int fcl_pwt_block_dx(const fcl_pwt_t* a, fcl_stream_t stream);
int fcl_pwt_block_dw(const fcl_pwt_t* a, fcl_stream_t stream);

/* ---- HiFi-GAN generator, training form: the upsampling stages' launches, forward (pre-activations kept) and backward
 *      (csrc/hifigan_train.hip; fcl_taco2_amd/hifigan_generator.py; restated in float64 numpy in tests/hfgt_ref.py).
 * Layout: as the Parallel WaveGAN training entries -- float32, channel-last, packed [rows, C], utterances back to back, row t's utterance is
 *      [seg_lo[t], seg_hi[t]) and a tap outside it contributes zero.  LeakyReLU: l(v) = v > 0 ? v : slope v, formed on load; its backward mask
 *      m(v) = v > 0 ? 1 : slope is read from the stored pre-activation (v == 0 takes the slope).
 *
 * fcl_hft_conv_t, one convolution of cin -> cout channels, k in (1, 3, 5, 7, 11) taps at `dilation`, tap j at row t + (j - (k - 1) / 2) dilation;
 *      w [k][cin][cout] tap-major (row j cin + ci = W[:, ci, j] of torch's Conv1d for fwd; for dx the taps reversed and W transposed):
 *   fcl_hft_conv_fwd (hft_conv_kernel):  y = bias + sum_j op(x)[row_j] w_j (+ res when res is given), op = l when lrelu, else the identity;
 *   fcl_hft_conv_dx (hft_conv_dx_kernel): y = m(pre) * sum_j x[row_j] w_j + res; x is the OUTPUT gradient [rows, cin], the operand is taken as stored;
 *      pre null: no mask; res null: no carry.  res may be y itself.
 *   fcl_hft_conv_dw (hft_dw_kernel, hft_dw_reduce_kernel): dw [k][cin][cout] = sum_t op(x)[row_j]^T g[t] in the forward weights' layout and
 *      db [cout] = sum_t g[t], as per-chunk partials of 1 024 rows in the workspace added in ascending chunk order by the second launch.
 * fcl_hft_tconv_t, the transposed convolution of stride s, kernel 2 s, padding s / 2 + s % 2, output padding s % 2; rows and the tables are at the INPUT
 *      rate, u and du have rows x s rows.  Output row s q + p reads, with ph = (p + padding) % s and q1 = q + (p + padding) / s, l(c)[q1] W[:, :, ph] and
 *      l(c)[q1 - 1] W[:, :, ph + s]:
 *   fcl_hft_tconv_fwd (hft_tconv_kernel): w [s][2][cin][cout], phase ph holds (W[:, :, ph + s] ; W[:, :, ph]);
 *   fcl_hft_tconv_dx (hft_tconv_dx_kernel): dc[q] = m(c[q]) * sum_j du[s q + j - padding] w_j, w [2 s][cout][cin] = W[:, :, j]^T (gather form);
 *   fcl_hft_tconv_dw (hft_tconv_dw_kernel, hft_dw_reduce_kernel): dw [2 s][cin][cout], db [cout]; partials of 1 024 / s input rows (a multiple of 32).
 * fcl_hft_sum (hft_sum_kernel): out = scale (terms[0] + terms[1] + ..) in ascending order, 1 to 4 terms of `elems` floats (a multiple of 4); `terms` is
 *      a host array of device pointers.  The stage's output (1 / nk) sum x_last, the backward seed dc / nk and du = the sum of the blocks' dx.
 * fcl_hft_workspace_bytes(rows, cin, cout, taps, stride): stride 1 for a convolution of `taps`, s (with taps = 2 s) for the transposed convolution.
 *
 * Exact fp32 on v_mfma_f32_16x16x4_f32; no atomics; two passes give the same bits; a batch's activations and input gradients are bit for bit those of
 *      its utterances alone.  Every entry validates before any HIP call: a null pointer or a slope outside [0, 1) FCL_ERR_INVALID; channels (multiples of
 *      16 from 16 to 512), kernel size, stride (2 .. 16), dilation or rows (rows x stride below 2^31) out of range FCL_ERR_SHAPE; an activation,
 *      gradient, weight or workspace pointer not 16-byte aligned FCL_ERR_ALIGN; a workspace that is too small FCL_ERR_WORKSPACE.  No entry allocates,
 *      synchronises or copies. */
typedef struct {
    int64_t rows;
    int32_t cin, cout, ksize, dilation;
    int32_t lrelu;         /* fwd, dw: 1 = the operand is l(x) */
    float slope;
    const int32_t* seg_lo;
    const int32_t* seg_hi;
    const float* x;        /* [rows, cin] */
    const float* w;        /* [ksize][cin][cout] */
    const float* bias;     /* [cout] (fwd) */
    const float* res;      /* [rows, cout] or null */
    const float* pre;      /* [rows, cout] or null (dx) */
    float* y;              /* [rows, cout] */
    const float* g;        /* [rows, cout] (dw) */
    float* dw;
    float* db;
    float* workspace;
    size_t workspace_bytes;
} fcl_hft_conv_t;
typedef struct {
    int64_t rows;          /* input rows */
    int32_t cin, cout, stride;
    float slope;
    const int32_t* seg_lo; /* [rows] */
    const int32_t* seg_hi;
    const float* c;        /* [rows, cin] the stage's input, a pre-activation */
    const float* w;
    const float* bias;     /* [cout] (fwd) */
    float* u;              /* [rows stride, cout] (fwd) */
    const float* du;       /* [rows stride, cout] (dx, dw) */
    float* dc;             /* [rows, cin] (dx) */
    float* dw;
    float* db;
    float* workspace;
    size_t workspace_bytes;
} fcl_hft_tconv_t;
size_t fcl_hft_workspace_bytes(int64_t rows, int cin, int cout, int taps, int stride);
int fcl_hft_conv_fwd(const fcl_hft_conv_t* a, fcl_stream_t stream);
int fcl_hft_conv_dx(const fcl_hft_conv_t* a, fcl_stream_t stream);
int fcl_hft_conv_dw(const fcl_hft_conv_t* a, fcl_stream_t stream);
int fcl_hft_tconv_fwd(const fcl_hft_tconv_t* a, fcl_stream_t stream);
int fcl_hft_tconv_dx(const fcl_hft_tconv_t* a, fcl_stream_t stream);
int fcl_hft_tconv_dw(const fcl_hft_tconv_t* a, fcl_stream_t stream);
int fcl_hft_sum(float* out, const float* const* terms, int count, float scale, int64_t elems, fcl_stream_t stream);

/* ---- HiFi-GAN generator, output end: LeakyReLU at the end's own slope, output_conv and tanh on the last stage's packed rows, forward and backward
 *      (csrc/hifigan_end.hip; fcl_taco2_amd/hifigan_generator.py; restated in float64 numpy in tests/hfge_ref.py).
 * Layout: as the training form above -- float32, channel-last, packed [rows, C], row t's utterance is [seg_lo[t], seg_hi[t]) and a tap outside it
 *      contributes zero; l and m as there, at `slope`.  w [k][cout][cin]: row j cout + o = W[o, :, j] of torch's Conv1d, the same matrix for all three
 *      entries; h = (k - 1) / 2.
 *   fcl_hfe_fwd (hfe_fwd_kernel): wav[t, o] = tanh(bias[o] + sum_j sum_ch l(x)[t + j - h, ch] w[j][o][ch]); only wav [rows, cout] is written.
 *   fcl_hfe_dx (hfe_dx_kernel): with dpre[t, o] = dwav[t, o] (1 - wav[t, o]^2), formed on load and never stored,
 *      dx[t, ch] = m(x[t, ch]) sum_j sum_o dpre[t - (j - h), o] w[j][o][ch].
 *   fcl_hfe_dw (hfe_dw_kernel, hfe_dw_reduce_kernel): dw [k][cout][cin] = sum_t dpre[t, o] l(x)[t + j - h, ch] in the weights' layout and
 *      db [cout] = sum_t dpre[t, o], as per-chunk partials of 1 024 rows in the workspace added in ascending chunk order by the second launch.
 * fcl_hfe_workspace_bytes(rows, cin, cout, ksize): what fcl_hfe_dw asks of the workspace.
 *
 * Plain fp32 FMAs (at most four output columns: no MFMA), the device library's tanhf; no atomics; two passes give the same bits; a batch's wav and dx
 *      are bit for bit those of its utterances alone.  Every entry validates before any HIP call: a null pointer or a slope outside [0, 1)
 *      FCL_ERR_INVALID; cin (a multiple of 16 from 16 to 256), cout (1 .. 4), ksize (3, 5, 7, 11) or rows (1 .. 2^31 - 2) out of range FCL_ERR_SHAPE;
 *      x, w, dx or the workspace not 16-byte aligned FCL_ERR_ALIGN; a workspace that is too small FCL_ERR_WORKSPACE.  No entry allocates, synchronises
 *      or copies. */
typedef struct {
    int64_t rows;
    int32_t cin, cout, ksize;
    float slope;
    const int32_t* seg_lo;
    const int32_t* seg_hi;
    const float* x;        /* [rows, cin] the last stage's output, a pre-activation */
    const float* w;        /* [ksize][cout][cin] */
    const float* bias;     /* [cout] (fwd) */
    float* wav;            /* [rows, cout]: written by fwd, read by dx and dw */
    const float* dwav;     /* [rows, cout] (dx, dw) */
    float* dx;             /* [rows, cin] (dx) */
    float* dw;             /* [ksize][cout][cin] (dw) */
    float* db;             /* [cout] (dw) */
    float* workspace;
    size_t workspace_bytes;
} fcl_hfe_t;
size_t fcl_hfe_workspace_bytes(int64_t rows, int cin, int cout, int ksize);
int fcl_hfe_fwd(const fcl_hfe_t* a, fcl_stream_t stream);
int fcl_hfe_dx(const fcl_hfe_t* a, fcl_stream_t stream);
int fcl_hfe_dw(const fcl_hfe_t* a, fcl_stream_t stream);

/* ---- HiFi-GAN period discriminator: a stack of strided (k, 1) Conv2d + LeakyReLU on the waveform folded by its period, one layer per call, forward and
 *      backward (csrc/hifigan_disc.hip; fcl_taco2_amd/hifigan_discriminator.py; restated in float64 numpy in tests/hfgd_ref.py).
 * Layout: float32, channel-last, packed [rows, C].  For period p an utterance becomes p segments (segment q holds the samples h p + q), the segments lie
 *      back to back, and the (k, 1) convolution is a 1-D convolution along each segment.  Every level has its own row count; the geometry comes from
 *      three int32 tables at the rate of the layer's OUTPUT rows: src[t] = the input row under the kernel's centre (the segment's first input row +
 *      stride x the row's index in its segment), [in_lo[t], in_hi[t]) the input segment (clamped to [0, rows_in] by the kernels).  Tap j of output row t
 *      reads input row src[t] + j - pad; outside the segment it reads zero.  The output segment of row t follows from the tables: it starts
 *      (src[t] - in_lo[t]) / stride rows before t and holds (in_hi[t] - in_lo[t] + 2 pad - ksize) / stride + 1 rows.
 * A layer is 1 -> C (the first), C -> C' or C -> 1 (the score layer), C, C' multiples of 16 from 16 to 1024.  The first and the C -> C' layers have
 *      ksize 3 or 5, pad (ksize - 1) / 2, stride 1 to 4, and LeakyReLU(slope); the score layer has ksize 2 or 3, pad 1, stride 1 and no activation (with
 *      2 taps a segment of H rows gives H + 1 scores).  Weights are tap-major: wf [ksize][cin][cout], wf[j][ci][co] = W[co][ci][j][0] of torch's Conv2d.
 * fcl_hpd_layer_fwd: y[t, co] = act(bias[co] + sum_j sum_ci x[src[t] + j - pad, ci] wf[j][ci][co]); w = wf, bias optional, x [rows_in, cin], y [rows_out, cout].
 * fcl_hpd_layer_dx: y[h, ci] = m(hin[h, ci]) (sum over the taps j and output rows o of h's segment with stride o + j - pad == h of
 *      g[o, co] W[co][ci][j] + extra[h, ci]): the gradient of the PRE-activation of the layer below.  g [rows_out, cout] is the gradient of this layer's
 *      pre-activation; h = hin [rows_in, cin] the stored post-activation of this layer's input, m = 1 where hin > 0, else slope (0 takes the slope, as
 *      torch does); extra [rows_in, cin] (optional) the gradient that reaches that feature map directly.  Every row of y is written.  w: for C -> C' the
 *      per-phase form wb [stride][ceil(ksize / stride)][cout][cin], wb[ph][i][co][ci] = W[co][ci][(ph + pad) % stride + stride i] (zero where that is
 *      no tap); for the first and the score layer w = wf.  The first layer (cin 1) has no mask: h and extra must be null, y [rows_in] is the
 *      waveform gradient.
 * fcl_hpd_layer_dw: dw [ksize][cin][cout] (the layout of wf) = sum_t x[src[t] + j - pad, ci] g[t, co]; db [cout] = sum_t g[t, co] (optional).  Each chunk of
 *      1024 output rows leaves a partial in the workspace (fcl_hpd_dw_workspace_bytes); a second launch adds them in ascending order.  No atomics
 *      anywhere: two runs give the same bits, and a batch's maps and input gradients are bit for bit those of its per-utterance runs.
 * One arithmetic mode, exact fp32: the C -> C' contractions run on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain), the rest on fmaf.  Every entry
 *      validates before any HIP call: a null pointer or a slope outside [0, 1) FCL_ERR_INVALID; channels, ksize, stride, pad or rows (1 .. 2^31 - 1)
 *      out of range FCL_ERR_SHAPE; x, g, w, h, extra, y not 16-byte aligned FCL_ERR_ALIGN; a workspace that is too small FCL_ERR_WORKSPACE.  No entry
 *      allocates, synchronises or copies. */
typedef struct {
    int64_t rows_in, rows_out;
    int32_t cin, cout, ksize, stride, pad;
    float slope;
    const int32_t* src;
    const int32_t* in_lo;
    const int32_t* in_hi;
    const float* x;
    const float* w;
    const float* bias;
    const float* h;
    const float* g;
    const float* extra;
    float* y;
    float* dw;
    float* db;
    float* workspace;
    size_t workspace_bytes;
} fcl_hpd_t;
size_t fcl_hpd_dw_workspace_bytes(int64_t rows_out, int cin, int cout, int ksize);
int fcl_hpd_layer_fwd(const fcl_hpd_t* a, fcl_stream_t stream);
int fcl_hpd_layer_dx(const fcl_hpd_t* a, fcl_stream_t stream);
int fcl_hpd_layer_dw(const fcl_hpd_t* a, fcl_stream_t stream);

/* ---- HiFi-GAN scale discriminator: grouped, strided 1-D convolutions + LeakyReLU on the waveform pooled 0, 1, 2, .. times, one layer per call, forward and
 *      backward, and the pooling with its adjoint (csrc/hifigan_sdisc.hip; fcl_taco2_amd/hifigan_scale_discriminator.py; restated in float64
 *      numpy in tests/hfgs_ref.py).
 * Layout and geometry as the period discriminator's above: float32, channel-last, packed [rows, C], the three int32 tables at the rate of the layer's
 *      OUTPUT rows; a segment is an utterance here.  Tap j of output row t reads input row src[t] + j - pad; outside the utterance it reads zero.
 * A layer is either the first (cin 1, groups 1, cout a multiple of 16 up to 1024, ksize odd from 3 to 15) or grouped (cin, cout multiples of 16 up to 1024,
 *      groups >= 1 dividing both, cout / groups a multiple of 16, cin / groups a multiple of 8, ksize odd from 3 to 41); pad (ksize - 1) / 2, stride 1 to 4,
 *      LeakyReLU(slope).  Output channel co belongs to group co / (cout / groups) and reads the input channels [g cin / groups, (g + 1) cin / groups).  The
 *      dense ksize 3 or 5 layer and the score layer (C -> 1) of a scale discriminator are fcl_hpd_* layers.
 *      Weights are tap-major: wf [ksize][cin / groups][cout], wf[j][c][co] = W[co][c][j] of torch's Conv1d(groups=).
 * fcl_hsd_layer_fwd: y[t, co] = lrelu(bias[co] + sum_j sum_c x[src[t] + j - pad, g(co) cin / groups + c] wf[j][c][co]); bias optional.
 * fcl_hsd_layer_dx: as fcl_hpd_layer_dx, y = m(hin) (adjoint + extra); w for a grouped layer is the per-phase form
 *      wb [stride][ceil(ksize / stride)][cout / groups][cin], wb[ph][i][o][ci] = W[g(ci) cout / groups + o][ci mod (cin / groups)][(ph + pad) % stride + stride i]
 *      (zero where that is no tap); for the first layer w = wf, h and extra must be null and y [rows_in] is the waveform gradient.  Every row is written once.
 * fcl_hsd_layer_dw: dw [ksize][cin / groups][cout] (the layout of wf), db [cout] (optional); chunked partials over 1024 output rows in the workspace
 *      (fcl_hsd_dw_workspace_bytes: chunks x (ksize cin / groups + 1) x cout floats), added in ascending order by a second launch.
 * fcl_hsd_pool_fwd: AvgPool1d(4, 2, padding 2) per utterance: y[n] = (x[2n - 2] + x[2n - 1] + x[2n] + x[2n + 1]) / 4 for n = 0 .. T / 2 (T / 2 + 1 outputs), zeros
 *      outside the utterance, the pad counted in the divisor.  in_off / out_off [n_utt + 1] int32: the utterances' first rows in x and y, the last entry
 *      rows_in / rows_out.  fcl_hsd_pool_dx: the adjoint in gather form, dx[m] = (g[m / 2] + g[m / 2 + 1]) / 4, the second term where m / 2 + 1 <= T / 2.
 * Exact fp32, no atomics, error classes as above (a null pointer or a bad slope FCL_ERR_INVALID; channels, groups, ksize, stride, pad, rows or n_utt out of
 *      range FCL_ERR_SHAPE; misaligned x, g, w, h, extra, y FCL_ERR_ALIGN; a small workspace FCL_ERR_WORKSPACE), checked before any HIP call. */
typedef struct {
    int64_t rows_in, rows_out;
    int32_t cin, cout, groups, ksize, stride, pad;
    float slope;
    const int32_t* src;
    const int32_t* in_lo;
    const int32_t* in_hi;
    const float* x;
    const float* w;
    const float* bias;
    const float* h;
    const float* g;
    const float* extra;
    float* y;
    float* dw;
    float* db;
    float* workspace;
    size_t workspace_bytes;
} fcl_hsd_t;
size_t fcl_hsd_dw_workspace_bytes(int64_t rows_out, int cin, int cout, int groups, int ksize);
int fcl_hsd_layer_fwd(const fcl_hsd_t* a, fcl_stream_t stream);
int fcl_hsd_layer_dx(const fcl_hsd_t* a, fcl_stream_t stream);
int fcl_hsd_layer_dw(const fcl_hsd_t* a, fcl_stream_t stream);
int fcl_hsd_pool_fwd(const float* x, float* y, const int32_t* in_off, const int32_t* out_off, int n_utt, int64_t rows_in, int64_t rows_out, fcl_stream_t stream);
int fcl_hsd_pool_dx(const float* g, float* dx, const int32_t* in_off, const int32_t* out_off, int n_utt, int64_t rows_in, int64_t rows_out, fcl_stream_t stream);

/* ---- Parallel WaveGAN generator, the ends: what stands in front of the residual stack and behind it, forward and backward
 *      (csrc/pwg_ends.hip; fcl_taco2_amd/pwg_generator.py; restated in float64 numpy in tests/pwge_ref.py).
 * Layout: as above -- float32, channel-last, packed rows, utterances back to back.  Utterance b has F_b frames (frame_off [n_utt + 1], frame_off[0] = 0,
 *      frames = frame_off[n_utt]) and F_b hop samples, hop = the product of scales[0 .. n_scales); seg_lo / seg_hi [samples] as above.  Its conditioning
 *      c_b has F_b + 2 ctx rows, so c is [frames + 2 ctx n_utt, A].  R and A as above; ctx 0 .. 8; 1 .. 6 scales of 2 .. 16.
 * Weights: w_in [(2 ctx + 1) A][A], row j A + ai = Win[:, ai, j] of torch's Conv1d (no bias); h[i] [2 s_i + 1] the stage's filter; w0, b0 [R] first_conv;
 *      w1 [R][R] = W1^T (row: input channel), w1t [R][R] = W1 (row: output channel), b1 [R]; w3 [R], b3 [1] the last layer.
 * fcl_pwe_in_fwd (pwe_convin_kernel, pwe_stage_kernel once per scale, pwe_first_kernel):
 *      u[0][f, :] = sum_j c_b[f + j, :] Win_j  [frames, A];
 *      u[i + 1][t, a] = sum_{j = 0 .. 2 s} h[i][j] u[i][(t + j - s) div s, a] over 0 <= t + j - s < s n_i of the utterance's own rows (s = scales[i]);
 *      the last stage writes cu [samples, A], the rows the stack reads; u[0 .. n_scales) are KEPT for the backward pass.  x0[t, :] = z[t] w0 + b0.
 * fcl_pwe_in_bwd: from dcu [samples, A] and dx0 [samples, R].  With dw_in (then dw0, db0 and every dh[i] too; all or none): dw0 = sum_t z[t] dx0[t, :],
 *      db0 = sum_t dx0 (pwe_outer_kernel), dh[i][j] = sum_{t, a} u[i][(t + j - s) div s, a] du_{i + 1}[t, a] (pwe_dh_kernel), dw_in = sum_f c_run(f)^T du0[f]
 *      (pwe_dwin_kernel), each as per-chunk partials that pwe_reduce_kernel adds in ascending chunk order.  With dz: dz[t] = dx0[t, :] . w0
 *      (pwe_first_dz_kernel).  With dc: dc = the transposed conv_in of du0 (pwe_dc_kernel).  The gradients of the stage inputs (pwe_stage_bwd_kernel, the
 *      transposed stretch and filter) are computed when weight gradients or dc are asked for and live in the workspace.
 * fcl_pwe_out_fwd (pwe_out_kernel): y1 = relu(relu(sigma skips) W1 + b1) [samples, R], KEPT; wav[t] = y1[t, :] . w3 + b3.
 * fcl_pwe_out_bwd (pwe_dy1_kernel, pwe_ds_kernel): dy1 = (dwav x w3) [y1 > 0] [samples, R]; ds = sigma (dy1 W1^T) [sigma skips > 0].  With dw1 (then db1,
 *      dw3, db3 too; all or none): dw1 [R][R] = sum_t relu(sigma skips)^T dy1 (row: input channel), db1 = sum_t dy1 (pwe_dw_kernel<last>), dw3 = sum_t
 *      dwav[t] y1[t, :], db3 = sum_t dwav (pwe_outer_kernel), reduced as above.
 * Exact fp32, no atomics, two runs give the same bits.  Every entry validates before any HIP call (FCL_ERR_INVALID / _SHAPE / _ALIGN / _WORKSPACE as
 *      above); none allocates, synchronises or copies.  fcl_pwe_workspace_bytes: what the backward entries ask for at the struct's sizes. */
typedef struct {
    int64_t samples;
    int32_t frames, n_utt;
    int32_t residual, aux, ctx, n_scales;
    int32_t scales[6];
    float sigma;           /* sqrt(1 / layers): the output side */
    int32_t reserved;
    const int32_t* seg_lo;
    const int32_t* seg_hi;
    const int32_t* frame_off;
    const float* c;
    const float* z;        /* [samples] */
    const float* w_in;
    const float* h[6];
    const float* w0;
    const float* b0;
    float* u[6];           /* u[i] [frames s_0 .. s_{i-1}, A]: written by in_fwd, read by in_bwd */
    float* cu;             /* [samples, A] */
    float* x0;             /* [samples, R] */
    const float* dcu;      /* [samples, A] */
    const float* dx0;      /* [samples, R] */
    float* dh[6];          /* or null: no weight gradient of the input side */
    float* dw_in;
    float* dw0;
    float* db0;
    float* dc;             /* [frames + 2 ctx n_utt, A] or null: not computed */
    float* dz;             /* [samples] or null: not computed */
    const float* skips;    /* [samples, R] the stack's un-scaled skip sum */
    const float* w1;
    const float* w1t;
    const float* b1;
    const float* w3;
    const float* b3;
    float* y1;             /* [samples, R] written by out_fwd, read by out_bwd */
    float* wav;            /* [samples] */
    const float* dwav;     /* [samples] */
    float* dy1;            /* [samples, R] written by out_bwd */
    float* ds;             /* [samples, R] */
    float* dw1;            /* or null: no weight gradient of the output side */
    float* db1;
    float* dw3;
    float* db3;
    float* workspace;
    size_t workspace_bytes;
} fcl_pwe_t;
size_t fcl_pwe_workspace_bytes(const fcl_pwe_t* a);
int fcl_pwe_in_fwd(const fcl_pwe_t* a, fcl_stream_t stream);
int fcl_pwe_in_bwd(const fcl_pwe_t* a, fcl_stream_t stream);
int fcl_pwe_out_fwd(const fcl_pwe_t* a, fcl_stream_t stream);
int fcl_pwe_out_bwd(const fcl_pwe_t* a, fcl_stream_t stream);

/* ---- the input feed of a capacity graph (..._kd_student.py:821-843: what inference() receives per call) -------------------------------------
 * fcl_feed_copy: ONE kernel that copies `bytes` (a multiple of 16) from pinned, mapped host memory (`src`: the DEVICE view of the block,
 * fcl_host_device_ptr) to `dst`, then increments *seq_dev, stores the new value to *seq_host (device view of a pinned word) and, when given,
 * adds 1 to *bump (the pass's RNG seed word).  Captured as the first node of a pass's hipGraph it replaces the hipMemcpyAsync in front of every
 * launch (~80 us of host time per pass); the host may repack the block once *seq_host equals the number of launches it has made. */
/* ---- streams restricted to a share of the compute units (round 6) --------------------------------------------------------------------------------
 * The KD update (tts_distill.py:143-182) runs the frozen teacher's forward one batch ahead on its own stream beside the student's update.  Both
 * are chains of dependent launches; the teacher's LSTM-step workgroups (72 - 96 KB of LDS, ~30 us each) fill every CU, so each of the student's
 * ~260 dependent launches first waits for one of them to retire (kernel trace: median 8.8 us between two launches of the student's stream, 0.1 us
 * on the teacher's).  A stream created here only dispatches to `n_cus` compute units, spread evenly over the XCDs (the queue's CU mask is
 * interleaved across XCCs by the driver: bit i -> XCD i % 8), which leaves the other CUs to the unrestricted streams.  n_cus <= 0 or >= the
 * device's CU count: an ordinary non-blocking stream. */
int fcl_stream_create_cus(int n_cus, fcl_stream_t* out);
int fcl_stream_destroy(fcl_stream_t stream);
/* Compute pipes (round 6).  The queue behind a HIP stream sits on one of MI355X's four compute pipes (queue index mod 4, in creation order within the process) and
 * a pipe advances one of its queues at a time: two chains of dependent launches take 1.0x the time of one when their streams are on different pipes, 1.43x on
 * the same pipe, 2.0x on the same hardware queue (more streams than GPU_MAX_HW_QUEUES).  HIP does not report the pipe; these two entries measure it (two chains
 * of 16 dependent ~20 us launches, alone and together, ~2 ms per pair; the streams must be idle).
 *   fcl_streams_share_pipe: *shared = 1 when a and b contend; *ratio (optional) = pair time / alone.
 *   fcl_stream_create_apart: a new stream apart from every others[k] (<= 24 candidates; n <= 3 can be met on four pipes; FCL_ERR_HIP when none fits, e.g. in a process holding dozens of streams); *tried (optional) = candidates created. */
int fcl_streams_share_pipe(fcl_stream_t a, fcl_stream_t b, int* shared, double* ratio);
int fcl_stream_create_apart(const fcl_stream_t* others, int n, fcl_stream_t* out, int* tried);
void* fcl_host_device_ptr(void* pinned_host);
int fcl_feed_copy(void* dst, const void* src, size_t bytes, uint32_t* seq_dev, uint32_t* seq_host, uint32_t* bump, fcl_stream_t stream);

/* ---- N3: the wire format handed to the vocoder (tts.py:652,674: kaldiio.WriteHelper("ark,scp:..."); inference_student.sh:20-23) --------------
 * HOST function (no device work): appends n Kaldi binary FloatMatrix records -- <key> ' ' "\0BFM " '\4' <int32 rows> '\4' <int32 cols> <float32 data>
 * -- to the open file descriptor `fd` with writev, straight from `data` (the utterances' matrices back to back, rows[i] x cols each; e.g. the
 * pinned landing buffer of a decoded batch).  file_pos: the file offset the first byte lands at; offsets[i] receives the offset of utterance i's
 * "\0B" marker (what its scp line points at).  Returns the new file offset (>= file_pos), or a negative FCL_ERR_* (fcl_last_error()). */
long long fcl_kaldi_ark_append(int fd, long long file_pos, int n, const char* const* keys, const float* data, const int* rows, int cols,
                               long long* offsets);

/* ---- H13 as ONE native routine: the teacher-forced training step orchestrated in C++ (round 4) -------------------------------------------------
 * Replaces, per update, the reference's `[teacher_knowledge = teacher(**x)]; loss = model(**x); loss.backward()` (tts_distill.py:143-182,
 * tts.py:137-179; forward()s: ..._kd_teacher.py:521-603, ..._kd_student.py:673-802, ..._sa.py:520-622) with a handful of host calls: the ~530
 * kernel launches of a KD update were issued one by one through Python / ctypes (16 us each: 8.7 ms of host time per 11 ms update);
 * here the same launches -- the very entry points above, in the same order, on the same three streams -- are issued from C++.
 * An engine (fcl_te_t) is bound to the flat parameter / gradient buffers of ONE model; it owns the operand forms of the parameters (packed taps,
 * transposes, column blocks, P32 planes: fcl_derive_batch, refreshed after every fcl_te_params_changed), a work arena and a zero arena in device
 * memory (sized by a dry run of the step before anything is launched; grown between steps), its weight-gradient stream and its events.
 * Scope: model.train() form (batch-statistics BatchNorm, sampled dropout / zoneout drawn on the device with the seeds the Python engine uses,
 * so both engines produce the same masks), the shipped-recipe structure (use_batch_norm, use_concate, no speaker embedding, no residual encoder,
 * no output activation), channel widths that are multiples of 32 (odim: of 4).  Everything else stays on fcl_taco2_amd.training.TrainEngine's
 * per-launch path, which is also the reference implementation this routine is tested against (equal losses / gradients on the same batch). */
typedef struct fcl_te fcl_te_t;
enum { FCL_TE_TEACHER = 0, FCL_TE_KD_TEACHER = 1, FCL_TE_STUDENT = 2 };
enum { FCL_TE_MAX_SITES = 48, FCL_TE_MAX_LOSSES = 48 };
typedef struct {
    int32_t role;                 /* FCL_TE_* */
    int32_t idim, odim, embed_dim, econv_layers, econv_chans, econv_filts, eunits, dunits, prenet_units, postnet_layers, postnet_chans, postnet_filts;
    int32_t dp_layers, dp_chans, dp_kernel;   /* duration predictor (ESPnet DurationPredictor) */
    int32_t vp_layers, vp_chans, vp_kernel;   /* pitch / energy predictors (variance_predictor.py) */
    int32_t ve_kernel;                         /* pitch / energy embedding Conv1d(1 -> C, k) */
    float dropout_rate, zoneout_rate, dp_dropout, vp_dropout, ve_dropout;
    int32_t use_masking;
    /* student: the teacher's widths (targets of the KD projections) and the distillation switches (..._kd_student.py:438-456) */
    int32_t t_embed_dim, t_econv_chans, t_eunits, t_prenet_units, t_dunits, t_postnet_chans;
    int32_t share_proj, distill_output, distill_encoder, distill_decoder, distill_prosody;
    int32_t accum_grad;
    uint32_t seed;                /* the engine's RNG seed (TrainEngine.seed) */
    uint32_t site_tag[FCL_TE_MAX_SITES]; /* per mask site: crc32(repr(site name)) & 0x7fffffff, order of fcl_te_site_name() */
    int32_t dw_planes_min;        /* weight gradients with at least this many outputs run on transposed planes */
    int32_t pred_stream;          /* predictors' forward / backward beside the decoder's on the weight-gradient stream (FCL_PRED_STREAM) */
    int32_t late_losses;          /* late KD terms on the weight-gradient stream (FCL_KD_LATE_LOSSES) */
} fcl_te_config_t;
/* one batch in the converter's layout (tts.py:215-306) with the integer maps of fcl_taco2_amd.training.build_maps_host, all in DEVICE memory
 * except live_rows_host */
typedef struct {
    int32_t B, T, L, N, F, lmax;
    const int64_t* xs;            /* [B*T] phoneme ids, 0 = padding */
    const float* ys;              /* [B*L, odim] target mels, zero padded */
    const float *f0, *energy, *ds;/* [B*T] ground-truth pitch / energy, durations as floats */
    const int32_t *lens, *e_lo, *e_hi, *f_lo, *f_hi, *src_sorted, *row_of_enc, *cell_frame, *frame_cell, *prev_frame, *cell_row, *dur, *perm_tb;
    const int64_t* cell_row_i64;
    const uint8_t *enc_pad, *enc_valid, *frame_valid, *cell_valid;
    const float* pos4;            /* [F, 4]: t / d in column 0 */
    const int32_t* live_rows_host;/* [lmax] HOST */
    double n_enc, n_frames;       /* valid phoneme positions / valid frames */
} fcl_te_batch_t;
/* the KD teacher's knowledge (..._kd_teacher.py:597-603) as device pointers.  dec[0..2] (prenet, LSTM-0, LSTM-1 taps): CELL-major [F, .] when
 * dec_cell_major != 0 (the native hand-over between two engines that share the batch's maps: no frame round trip), else frame-major [B*L, .] like
 * the reference's tuple. */
typedef struct {
    const float *after, *before;  /* [B*L, odim] */
    const float* enc[5];          /* embed, conv x3, blstm: [B*T, C_t] */
    const float* dec[8];          /* prenet, lstm0, lstm1 taps; postnet layer outputs x5 */
    const float* pro[5];          /* d_outs, p_outs, e_outs [B*T]; p_embs, e_embs [B*T, C_t] */
    int32_t dec_cell_major;
} fcl_te_knowledge_t;
int fcl_te_create(const fcl_te_config_t* cfg, fcl_te_t** out);
void fcl_te_destroy(fcl_te_t* te);
/* names of the mask sites (for site_tag) and of the loss slots (rows of the [FCL_TE_MAX_LOSSES][3] sums), NULL past the end */
const char* fcl_te_site_name(int i);
const char* fcl_te_loss_name(int i);
/* bind a parameter (value + gradient accumulator inside the caller's flat buffers) or a buffer (BatchNorm running statistics) by its state_dict
 * name; fcl_te_finalize checks that everything the configuration needs is bound */
int fcl_te_bind_param(fcl_te_t* te, const char* name, float* value, float* grad, int64_t numel);
int fcl_te_bind_buffer(fcl_te_t* te, const char* name, float* value);
int fcl_te_finalize(fcl_te_t* te, uint32_t* status_word);
/* the parameters were written (optimizer step, load_state_dict): operand forms are re-derived before the next forward */
int fcl_te_params_changed(fcl_te_t* te);
/* the engine's weight-gradient stream (created by the engine): the caller issues bucketed all-reduces from it between backward stages */
fcl_stream_t fcl_te_side_stream(fcl_te_t* te);
/* before the first pass (round 6): should the weight-gradient stream share a compute pipe with `main_stream` (measured, see fcl_streams_share_pipe), it is
 * replaced by a stream that does not; *moved (optional) = 1 then (a handle obtained from fcl_te_side_stream before the call is invalid), -1 when it contends but
 * no replacement could be placed (the stream is kept), 0 when it was fine */
int fcl_te_place_streams(fcl_te_t* te, fcl_stream_t main_stream, int* moved);
/* forward only (frozen KD teacher, train-mode statistics): *know points into one of the engine's two alternating arenas: valid until the
 * second next fcl_te_knowledge call on this engine */
int fcl_te_knowledge(fcl_te_t* te, const fcl_te_batch_t* batch, uint32_t draw, fcl_te_knowledge_t* know, fcl_stream_t stream);
/* forward + losses + backward stage 0 (postnet; gradient bucket 0 is final when it returns, in stream order); then fcl_te_backward_stage 1 (decoder:
 * bucket 1), 2 (predictors / embeddings: bucket 2), 3 (encoder: bucket 3 + the join of the weight-gradient stream).  know: required for the student.
 * loss_sums_host: pinned [FCL_TE_MAX_LOSSES][3] doubles receiving (sum |d|, sum d^2, count) per loss slot, status_host: pinned uint32, both copied
 * asynchronously on `stream` at the end of stage 0.  draw: the forward's ordinal (seeds the masks with cfg.seed and the site tags). */
int fcl_te_forward_backward(fcl_te_t* te, const fcl_te_batch_t* batch, const fcl_te_knowledge_t* know, uint32_t draw, double* loss_sums_host,
                            uint32_t* status_host, fcl_stream_t stream);
int fcl_te_backward_stage(fcl_te_t* te, int stage, fcl_stream_t stream);
/* the end-of-backward join: `stream` waits for everything on the weight-gradient stream (after the caller issued its last bucket's collective there) */
int fcl_te_join(fcl_te_t* te, fcl_stream_t stream);
/* diagnostics: launches issued by the last forward_backward (all stages) / knowledge call, and the arena bytes it used */
int64_t fcl_te_last_launches(fcl_te_t* te);
/* developer aid (FCL_TE_STAMPS=1): ms from the start of the last fcl_te_forward_backward to its phase boundaries on the main stream: [0] start,
 * [1] encoder, [2] prenet + hoists, [3] decoder cells, [4] forward end, [5] losses, [6..9] backward stages 0..3, [10] join; -1 = not recorded */
int fcl_te_phase_ms(fcl_te_t* te, float* out12);
int64_t fcl_te_arena_bytes(fcl_te_t* te);

#ifdef __cplusplus
}
#endif
#endif /* FCL_HIP_H_ */
