/* mmt_hip.h — C ABI of libmmt_hip.so, the MI355X (gfx950) implementation of the attention hot path
 * of frankaging/Multimodal-Transformer.
 *
 * The reference has no FFI: its boundary for this path is the Python class surface of
 * transformer/{SFT,MFT,B2-Trans}/multiTransformer.py.  Each entry point below replaces
 * the forward (or the autograd backward) of one of those classes and is what a binding for the
 * reference would call (ctypes stub: INTEGRATION.md).  Conventions:
 *   - every pointer is a DEVICE pointer unless named host_*; tensors are contiguous fp32 in the
 *     reference's own layouts: activations (B,T,d) row-major, mask (B,T,1) float {0,1} (a window is
 *     blanked where mask == 0, multiTransformer.py:30), nn.Linear weights (out,in);
 *   - the pointer contract.  Every tensor argument is CONTIGUOUS in the layout its entry names, of the element type its
 *     declaration names (float = fp32, int32_t, double, uint64_t; a stream state and a workspace are bytes), and aligned to
 *     that element type.  Nothing is read through a stride: a caller with a strided, transposed, expanded or non-fp32 tensor
 *     makes a contiguous fp32 copy first (the Python binding's _f32c does).  Beyond that an argument is in one of three
 *     classes:
 *       (a) scalar access: any address aligned to the element type.  Every argument not listed under (b) or (c): masks,
 *           row scales, key lengths, positions, weights and biases that are converted into a workspace (mmt_linear_* Wt / b,
 *           every scan's W_rec / P / W_hh / W1 / Wm / W2, the conv weight and bias, the parameters given to a
 *           *_stream_prepare), seed words, and every argument of mmt_sdpa_*, mmt_key_lengths, mmt_ar_combine_*,
 *           mmt_lstm_stack_scan_*, mmt_lstm_fb_scan_*, mmt_softmax_mul_*, mmt_colsum, mmt_highway_*, mmt_adam_step,
 *           mmt_ccc_forward, and x_t / e_t / mask_t / y_t / params of the stream steps;
 *       (b) alignment selects the instantiation: a 16-byte aligned address (with leading dimensions and widths that are
 *           multiples of 4) runs a kernel that moves four floats per lane, any other address the scalar one, which gives the
 *           same values: every pointer of an mmt_copy2d segment, h / ctx / dctx / dh of mmt_local_attn_*, q / k of
 *           mmt_attn_probs_forward*;
 *       (c) 16-byte alignment is REQUIRED: a kernel of the entry moves 16 bytes per lane through the pointer.  The entry
 *           returns MMT_EINVAL before any launch, and mmt_last_error() names the argument:
 *             mmt_encoder_forward*: x, params, y;  mmt_encoder_backward*: dy, x, params, dx;
 *             mmt_layernorm_forward: x, a_2, b_2, y;  mmt_layernorm_backward: dy, x, a_2, dx;
 *             mmt_linear_forward / mmt_linear_dropout_forward: x, y;  mmt_linear_backward / mmt_linear_dropout_backward: dx;
 *             mmt_linear_prepare: prepared;  mmt_linear_forward_prepared: x, prepared, y;
 *             mmt_lstm_scan_forward: gx, h0, c0, h_all, c_all, acts;
 *             mmt_lstm_scan_backward: dh_all, dc_all, c0, c_all, acts, dgx, dh0, dc0;
 *             mmt_mfn_mem_scan_forward*: apre, chat, b2, mem_all, u_all, g_all;
 *             mmt_mfn_mem_scan_backward: dmem_all, chat, mem_all, u_all, g_all, dchat, dapre, dz_all;
 *             mmt_convpool_* and mmt_convpool_k_*: x;  mmt_mse_sum_forward: pred, target, dpred;
 *             the `state` of every mmt_*_stream_prepare / _step / _step_slots (its pieces are laid out from its base and
 *             a step reads the prepared weights and the K/V cache eight bf16 per lane).
 *       An optional argument that is absent (a null pointer) passes.  A workspace is carved into 256-byte aligned pieces
 *       from its base and is accessed 16 bytes wide: pass the base of an allocation (hipMalloc gives 256-byte alignment);
 *   - the library allocates nothing: the caller passes a workspace of *_workspace_bytes() bytes, under
 *     one of two contracts, named at each entry's workspace query:
 *       "zero once": the workspace MUST be zero-filled when first created and may then be reused, without
 *         clearing, by any later call of the same entry family and the same shape arguments, whatever
 *         else differs (inputs, a NaN among them, mask, key lengths, plain / _keys / _causal / _band form,
 *         dropout probability, seed by value or device-resident).  Pad regions are never written, so
 *         they stay zero; every other word a call reads it has written itself (or, in a backward, its
 *         forward has: saved-for-backward tensors live in the workspace between the two).  This is the
 *         contract of every entry that says nothing else;
 *       "any contents": every word used is written first by a kernel of the same call, so the memory
 *         may come uninitialised: mmt_lstm_scan_*, mmt_mfn_mem_scan_*, mmt_convpool_*,
 *         mmt_convpool_k_* and mmt_local_attn_backward.
 *     tests/test_gpu_workspace_state.py holds both, bit for bit;
 *   - all work is enqueued on `stream` (a hipStream_t); nothing synchronises, so calls are capturable
 *     into a hipGraph;
 *   - return 0 on success, non-zero MMT_E* on error with a message in mmt_last_error() (thread local).
 *     Asynchronous HIP faults surface at the caller's next synchronisation, as in PyTorch.
 */
#ifndef MMT_HIP_H
#define MMT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMT_OK 0
#define MMT_EINVAL 1      /* bad shape / null pointer */
#define MMT_EUNSUPPORTED 2 /* e.g. d_k > 64, d_model > 512, d % 4 != 0 */
#define MMT_EWORKSPACE 3  /* workspace too small */
#define MMT_EHIP 4        /* a HIP runtime call failed */

typedef void* mmt_stream_t; /* hipStream_t */

int mmt_abi_version(void);
const char* mmt_last_error(void);

/* ---- Per-launch-site timing with HIP events on the caller's stream (eager mode only: do not enable
 * while capturing a hipGraph).  Used by bench.py for the roofline of the dominant kernel. */
int mmt_profile_enable(int on);
int mmt_profile_reset(void);
int mmt_profile_num_sites(void);
const char* mmt_profile_site_name(int site);
/* waits for the recorded events; total_ms[num_sites], launches[num_sites] */
int mmt_profile_collect(float* total_ms, int* launches);

/* ---- Encoder stack: N x (pre-norm self-attention sublayer + pre-norm FFN sublayer) + final LayerNorm.
 * Replaces Encoder.forward(x, mask)                       transformer/MFT/multiTransformer.py:73-76
 *   with EncoderLayer.forward / SublayerConnection.forward                              :103-104,114-116
 *        MultiHeadedAttention.forward + attention()                                      :22-34,47-65
 *        PositionwiseFeedForward.forward                                                 :19-20
 *        LayerNorm.forward (unbiased std, eps added to std)                              :88-91
 * `params`: one flat fp32 buffer, per layer in the reference's registration order
 *   self_attn.linears.{0,1,2,3}.{weight(d,d),bias(d)}, feed_forward.w_1.{weight(f,d),bias(f)},
 *   feed_forward.w_2.{weight(d,f),bias(d)}, sublayer.0.norm.{a_2,b_2}, sublayer.1.norm.{a_2,b_2},
 * followed by the stack's norm.{a_2,b_2}.  mmt_encoder_param_count() gives its length.
 * Eval-mode (dropout = identity) when dropout_p == 0; see mmt_encoder_forward's `dropout_p`, `seed`. */
size_t mmt_encoder_param_count(int d, int f, int n_layers);
/* workspace: zero once; reusable for the same (B, T, d, h, f, n_layers) and the same kind (train / eval, below) by every form of the
 * entry (plain, _keys, _causal, _band, _devseed). */
size_t mmt_encoder_workspace_bytes(int B, int T, int d, int h, int f, int n_layers);
/* ... for calls with dropout_p == 0 only (eval mode): without the attention-dropout bit masks (2 x n_layers x B*h x Tp^2/4 bytes, the
 * last region of the full workspace: an eval workspace is a prefix of a train one).  A forward and its backward take the same kind. */
size_t mmt_encoder_workspace_bytes_eval(int B, int T, int d, int h, int f, int n_layers);

int mmt_encoder_forward(const float* x, const float* mask, const float* params, float* y,
                        void* workspace, size_t workspace_bytes,
                        int B, int T, int d, int h, int f, int n_layers, float eps,
                        float dropout_p, uint64_t seed, mmt_stream_t stream);

/* Backward of the above (what torch autograd derives for the reference).  Must follow a forward on the
 * same workspace.  dx: (B,T,d); dparams: flat, same layout as params (fully overwritten). */
int mmt_encoder_backward(const float* dy, const float* x, const float* mask, const float* params,
                         float* dx, float* dparams,
                         void* workspace, size_t workspace_bytes,
                         int B, int T, int d, int h, int f, int n_layers, float eps,
                         float dropout_p, uint64_t seed, mmt_stream_t stream);

/* Device-resident dropout seed: the same pair for a step that is captured into a hipGraph and replayed, where a seed passed by value
 * would be frozen at capture (the reference's nn.Dropout draws fresh masks every step: transformer/MFT/multiTransformer.py:17,45,101,
 * torch keeps its generator state on the device under graph capture for the same reason).  `seed_state`: one uint64 in device memory,
 * owned by the caller.  The forward's first kernel copies it into the workspace (the seed of THIS forward and of its backward) and
 * advances it (splitmix64), so every replay draws new masks; the masks of a step are those mmt_debug_dropout_mask gives for the value
 * seed_state held before that step.  The backward takes no seed: it reads the workspace. */
int mmt_encoder_forward_devseed(const float* x, const float* mask, const float* params, float* y,
                                void* workspace, size_t workspace_bytes,
                                int B, int T, int d, int h, int f, int n_layers, float eps,
                                float dropout_p, uint64_t* seed_state, mmt_stream_t stream);
int mmt_encoder_backward_devseed(const float* dy, const float* x, const float* mask, const float* params,
                                 float* dx, float* dparams,
                                 void* workspace, size_t workspace_bytes,
                                 int B, int T, int d, int h, int f, int n_layers, float eps,
                                 float dropout_p, mmt_stream_t stream);

/* ---- LayerNorm alone.  Replaces LayerNorm.forward            transformer/MFT/multiTransformer.py:88-91
 * stats: (M,2) fp32 scratch kept for the backward (mean, 1/(std+eps)).
 * colpart: scratch of mmt_layernorm_scratch_floats(M,d) floats. */
size_t mmt_layernorm_scratch_floats(int M, int d);
int mmt_layernorm_forward(const float* x, const float* a_2, const float* b_2, float* y, float* stats,
                          int M, int d, float eps, mmt_stream_t stream);
int mmt_layernorm_backward(const float* dy, const float* x, const float* a_2, const float* stats,
                           float* dx, float* da_2, float* db_2, float* scratch,
                           int M, int d, float eps, mmt_stream_t stream);

/* ---- Scaled dot-product attention core on already-projected q, k, v.
 * Replaces attention(query, key, value, mask)                 transformer/MFT/multiTransformer.py:22-34
 * q,k,v,ctx: (B,T,d) fp32 with head `i` in columns [i*d/h,(i+1)*d/h) (the layout before the reference's
 * .view(B,-1,h,d_k).transpose(1,2)); mask (B,T,1) blanks QUERY rows; may be NULL.
 * dropout_p, seed: the reference's nn.Dropout on p_attn (:32-33) in train mode (0 = eval / dropout=None); the decisions are
 * drawn by the forward into the workspace and re-read by the backward (same dropout_p and seed must be passed); they are
 * dropout stream 0 of mmt_debug_dropout_mask. */
/* workspace: zero once; reusable for the same (B, T, d, h) and the same kind (train / eval) by the plain, _keys, _causal and _band forms. */
size_t mmt_sdpa_workspace_bytes(int B, int T, int d, int h);
size_t mmt_sdpa_workspace_bytes_eval(int B, int T, int d, int h);      /* dropout_p == 0 calls: without the dropout bit masks */
int mmt_sdpa_forward(const float* q, const float* k, const float* v, const float* mask, float* ctx,
                     void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                     float dropout_p, uint64_t seed, mmt_stream_t stream);
int mmt_sdpa_backward(const float* dctx, const float* mask, float* dq, float* dk, float* dv,
                      void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                      float dropout_p, uint64_t seed, mmt_stream_t stream);

/* ---- The attention probabilities, materialised on request.
 * Replaces p_attn, the second return value of attention(), which MultiHeadedAttention keeps as self.attn
 *                                                              transformer/MFT/multiTransformer.py:22-34,59
 * q,k: (B,T,d) fp32 as for mmt_sdpa_forward; mask (B,T,1) blanks QUERY rows (such a row is exactly 1/T); may be NULL.
 * probs: (B,h,T,T) fp32, [b][head][query][key]: the post-dropout probabilities mmt_sdpa_forward uses for the same q, k, mask,
 * dropout_p and seed (same operand rounding; in train mode the same keep decisions, dropped = 0, kept = P/(1-p)).
 * d_k <= 64 and T <= 4096.  No workspace; one launch. */
int mmt_attn_probs_forward(const float* q, const float* k, const float* mask, float* probs,
                           int B, int T, int d, int h, float dropout_p, uint64_t seed, mmt_stream_t stream);

/* ---- Key lengths: a padding mask that masks KEYS (opt-in; no counterpart in the reference, whose attention() blanks query rows
 * only and lets every window attend the padded windows behind its sequence: transformer/MFT/multiTransformer.py:29-31).
 * key_lengths: int32 (B,) in device memory.  Sequence b attends keys 0 .. key_lengths[b]-1: later keys score -inf, their probabilities
 * are exactly 0, their dK and dV exactly 0.  The query-row mask keeps its meaning (a blanked row is uniform over the visible keys and
 * passes no gradient to q).  The kernels clamp every length they read into [1, T].  Each `_keys` entry is the plain entry of the same
 * name plus the trailing `key_lengths` (NULL: MMT_EINVAL), with the plain entry's workspace; with every length equal to T it computes
 * what the plain entry computes.  The backward always runs as two kernels (dK/dV, dQ).
 * mmt_key_lengths: len[b] = 1 + index of the last non-zero entry of row b of mask (B,T) fp32, 1 for an all-zero row — holes inside
 * the prefix stay attended.  One launch, capture-safe. */
int mmt_key_lengths(const float* mask, int32_t* key_lengths, int B, int T, mmt_stream_t stream);
/* mmt_sdpa_forward / mmt_sdpa_backward with key lengths                       (attention(), :22-34) */
int mmt_sdpa_forward_keys(const float* q, const float* k, const float* v, const float* mask, float* ctx,
                          void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                          float dropout_p, uint64_t seed, mmt_stream_t stream, const int32_t* key_lengths);
int mmt_sdpa_backward_keys(const float* dctx, const float* mask, float* dq, float* dk, float* dv,
                           void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                           float dropout_p, uint64_t seed, mmt_stream_t stream, const int32_t* key_lengths);
/* mmt_attn_probs_forward with key lengths: columns >= key_lengths[b] are exact zeros, a blanked query row is 1/key_lengths[b]
 * on the visible columns                                                      (p_attn, :22-34,59) */
int mmt_attn_probs_forward_keys(const float* q, const float* k, const float* mask, float* probs,
                                int B, int T, int d, int h, float dropout_p, uint64_t seed, mmt_stream_t stream,
                                const int32_t* key_lengths);
/* mmt_encoder_forward / mmt_encoder_backward and their device-seeded twins with key lengths: every layer's attention uses them
 *                                                                             (Encoder.forward, :72-83) */
int mmt_encoder_forward_keys(const float* x, const float* mask, const float* params, float* y,
                             void* workspace, size_t workspace_bytes,
                             int B, int T, int d, int h, int f, int n_layers, float eps,
                             float dropout_p, uint64_t seed, mmt_stream_t stream, const int32_t* key_lengths);
int mmt_encoder_backward_keys(const float* dy, const float* x, const float* mask, const float* params,
                              float* dx, float* dparams,
                              void* workspace, size_t workspace_bytes,
                              int B, int T, int d, int h, int f, int n_layers, float eps,
                              float dropout_p, uint64_t seed, mmt_stream_t stream, const int32_t* key_lengths);
int mmt_encoder_forward_keys_devseed(const float* x, const float* mask, const float* params, float* y,
                                     void* workspace, size_t workspace_bytes,
                                     int B, int T, int d, int h, int f, int n_layers, float eps,
                                     float dropout_p, uint64_t* seed_state, mmt_stream_t stream, const int32_t* key_lengths);
int mmt_encoder_backward_keys_devseed(const float* dy, const float* x, const float* mask, const float* params,
                                      float* dx, float* dparams,
                                      void* workspace, size_t workspace_bytes,
                                      int B, int T, int d, int h, int f, int n_layers, float eps,
                                      float dropout_p, mmt_stream_t stream, const int32_t* key_lengths);

/* ---- Causal self-attention (opt-in; no counterpart in the reference, whose attention() lets window t attend every window of the
 * batch row, later ones included: scores.masked_fill(mask == 0, -1e9) blanks query rows only, transformer/MFT/multiTransformer.py:29-31).
 * Query t of a sequence sees keys 0 .. t of that sequence: later keys score -inf, their probability is exactly 0 and they get no dK or
 * dV from that query.  The query-row mask keeps its meaning (a blanked row t is uniform over its t + 1 visible keys and passes no
 * gradient to q); row 0 attends one key, so in eval mode its context is bf16(v[b, 0]).  Dropout bits are drawn as for the plain entry,
 * per position for the whole T x T block; bits above the diagonal are never read.  Each `_causal` entry has the plain entry's exact
 * signature and workspace.  The backward always runs as two kernels (dK/dV, dQ).  There is no form with key lengths: a valid window
 * t < len of a prefix-masked batch sees keys <= t < len only, so causal attention already keeps it from the padding behind its sequence. */
/* mmt_sdpa_forward / mmt_sdpa_backward, causal                                (attention(), :22-34; departs from :27-31) */
int mmt_sdpa_forward_causal(const float* q, const float* k, const float* v, const float* mask, float* ctx,
                            void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                            float dropout_p, uint64_t seed, mmt_stream_t stream);
int mmt_sdpa_backward_causal(const float* dctx, const float* mask, float* dq, float* dk, float* dv,
                             void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                             float dropout_p, uint64_t seed, mmt_stream_t stream);
/* mmt_attn_probs_forward, causal: entries above the diagonal are exact zeros, a blanked query row t is 1/(t+1) on columns 0 .. t
 *                                                                             (p_attn, :22-34,59; departs from :27-31) */
int mmt_attn_probs_forward_causal(const float* q, const float* k, const float* mask, float* probs,
                                  int B, int T, int d, int h, float dropout_p, uint64_t seed, mmt_stream_t stream);
/* mmt_encoder_forward / mmt_encoder_backward and their device-seeded twins, causal: every layer's self-attention is causal
 *                                                                             (Encoder.forward, :72-83; departs from :27-31) */
int mmt_encoder_forward_causal(const float* x, const float* mask, const float* params, float* y,
                               void* workspace, size_t workspace_bytes,
                               int B, int T, int d, int h, int f, int n_layers, float eps,
                               float dropout_p, uint64_t seed, mmt_stream_t stream);
int mmt_encoder_backward_causal(const float* dy, const float* x, const float* mask, const float* params,
                                float* dx, float* dparams,
                                void* workspace, size_t workspace_bytes,
                                int B, int T, int d, int h, int f, int n_layers, float eps,
                                float dropout_p, uint64_t seed, mmt_stream_t stream);
int mmt_encoder_forward_causal_devseed(const float* x, const float* mask, const float* params, float* y,
                                       void* workspace, size_t workspace_bytes,
                                       int B, int T, int d, int h, int f, int n_layers, float eps,
                                       float dropout_p, uint64_t* seed_state, mmt_stream_t stream);
int mmt_encoder_backward_causal_devseed(const float* dy, const float* x, const float* mask, const float* params,
                                        float* dx, float* dparams,
                                        void* workspace, size_t workspace_bytes,
                                        int B, int T, int d, int h, int f, int n_layers, float eps,
                                        float dropout_p, mmt_stream_t stream);

/* ---- Banded causal self-attention (opt-in; sliding-window / local causal attention; departs from :27-31 as the causal entries do).
 * Query t of a sequence sees keys max(0, t - span + 1) .. t of that sequence, span >= 1 windows, its own included: every other key scores
 * -inf, its probability is exactly 0 and it gets no dK or dV from that query.  span = 1: a query sees itself only, in eval mode
 * ctx[b, t] == bf16(v[b, t]).  span >= T is causal attention as a function, computed by the band kernels (agreement with the _causal
 * entries is within tolerance, not bit for bit: the forward sweeps its key tiles downwards from the diagonal).  The query-row mask keeps
 * its meaning: a blanked row t is uniform over its min(t + 1, span) visible keys and passes no gradient to q.  Dropout bits are drawn as
 * for the plain entry, per position for the whole T x T block; bits outside the band are never read.  Each `_band` entry has the plain
 * entry's signature with `int span` in front of the stream, and the plain entry's workspace (zero once, reusable for the same shape
 * and kind by every form); span < 1 returns MMT_EINVAL.  The backward always runs as two kernels (dK/dV, dQ).  There is no form with
 * key lengths, for the reason given for causal. */
/* mmt_sdpa_forward / mmt_sdpa_backward, band                                  (attention(), :22-34; departs from :27-31) */
int mmt_sdpa_forward_band(const float* q, const float* k, const float* v, const float* mask, float* ctx,
                          void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                          float dropout_p, uint64_t seed, int span, mmt_stream_t stream);
int mmt_sdpa_backward_band(const float* dctx, const float* mask, float* dq, float* dk, float* dv,
                           void* workspace, size_t workspace_bytes, int B, int T, int d, int h,
                           float dropout_p, uint64_t seed, int span, mmt_stream_t stream);
/* mmt_attn_probs_forward, band: entries outside columns max(0, t - span + 1) .. t of row t are exact zeros, a blanked query row t is
 * 1/min(t + 1, span) on those columns                                         (p_attn, :22-34,59; departs from :27-31) */
int mmt_attn_probs_forward_band(const float* q, const float* k, const float* mask, float* probs,
                                int B, int T, int d, int h, float dropout_p, uint64_t seed, int span, mmt_stream_t stream);
/* mmt_encoder_forward / mmt_encoder_backward and their device-seeded twins, band: every layer's self-attention has the same span
 *                                                                             (Encoder.forward, :72-83; departs from :27-31) */
int mmt_encoder_forward_band(const float* x, const float* mask, const float* params, float* y,
                             void* workspace, size_t workspace_bytes,
                             int B, int T, int d, int h, int f, int n_layers, float eps,
                             float dropout_p, uint64_t seed, int span, mmt_stream_t stream);
int mmt_encoder_backward_band(const float* dy, const float* x, const float* mask, const float* params,
                              float* dx, float* dparams,
                              void* workspace, size_t workspace_bytes,
                              int B, int T, int d, int h, int f, int n_layers, float eps,
                              float dropout_p, uint64_t seed, int span, mmt_stream_t stream);
int mmt_encoder_forward_band_devseed(const float* x, const float* mask, const float* params, float* y,
                                     void* workspace, size_t workspace_bytes,
                                     int B, int T, int d, int h, int f, int n_layers, float eps,
                                     float dropout_p, uint64_t* seed_state, int span, mmt_stream_t stream);
int mmt_encoder_backward_band_devseed(const float* dy, const float* x, const float* mask, const float* params,
                                      float* dx, float* dparams,
                                      void* workspace, size_t workspace_bytes,
                                      int B, int T, int d, int h, int f, int n_layers, float eps,
                                      float dropout_p, int span, mmt_stream_t stream);

/* ---- A causal encoder stack, one window at a time (opt-in; eval mode, forward only).
 * Replaces Encoder.forward(x, mask)[:, t] with causal attention on               transformer/MFT/multiTransformer.py:73-76
 *                                                                             (departs from :27-31 as the causal entries above do)
 * for t = 0, 1, 2, ... of one recording per batch row, without recomputing the prefix: the state keeps, per layer, the bf16 K and V of
 * the windows seen so far (exactly the operands the batch kernels consume).  One step is ONE launch for the whole stack and the final
 * LayerNorm, one workgroup per sequence, no communication between workgroups: a sequence's result does not depend on its batch.
 * Numerics: the batch path's rounding sites (bf16 operands of every product, fp32 sums, biases, residuals, LayerNorm) with one
 * difference, the softmax reference point: the row's own exact maximum, where the batch kernel keeps a lazily moved maximum per
 * 32-query tile (csrc/encoder_step.h).  Two equally faithful roundings: rows agree to about 1.5e-3 rel-L2.
 * `state`: mmt_encoder_stream_bytes() bytes, ANY CONTENTS: every word a step reads was written by mmt_encoder_stream_prepare or by an
 * earlier step of this recording.  A new recording starts by passing t = 0 again; nothing needs clearing.
 * Limits: d % h == 0, d % 4 == 0, f % 4 == 0, d_k <= 64, d <= 512, f <= 2048, 1 <= n_layers <= 16, 1 <= capacity <= 4096,
 * h * (d_k rounded up to 8) <= 2048: anything else is MMT_EUNSUPPORTED with the limit named in mmt_last_error(), at the size query
 * (which then returns 0); non-positive sizes and null pointers: MMT_EINVAL. */
/* (Encoder.forward, :73-76; departs from :27-31) */
size_t mmt_encoder_stream_bytes(int B, int capacity, int d, int h, int f, int n_layers);
/* One launch: the weight matrices of `params` (mmt_encoder_param_count() floats, the layout above) to bf16 in the step kernel's layout,
 * at the front of the state.  Does not touch the cache.  Call it again after the parameters change.
 * (Encoder.forward, :73-76; departs from :27-31) */
int mmt_encoder_stream_prepare(const float* params, void* state, size_t state_bytes,
                               int B, int capacity, int d, int h, int f, int n_layers, mmt_stream_t stream);
/* x_t (B,d) -> y_t (B,d) at position t; mask_t (B) float {0,1} or NULL: a blanked window is uniform over its t + 1 keys, and its K_t
 * and V_t are appended like any other.  `params`: the same buffer prepare saw (biases and LayerNorm weights are read from it in fp32).
 * t is passed by value; t < 0 or t >= capacity returns MMT_EINVAL before any launch.  Steps of one recording must be enqueued in
 * order t = 0, 1, ... on one stream.                                           (Encoder.forward, :73-76; departs from :27-31) */
int mmt_encoder_stream_step(const float* x_t, const float* mask_t, const float* params, float* y_t,
                            void* state, size_t state_bytes, int t, int B, int capacity, int d, int h, int f, int n_layers,
                            float eps, mmt_stream_t stream);
/* The step of a stack with a span (mmt_encoder_forward_band: window t attends t - span + 1 .. t), against a RING cache: the state is
 * the one above with capacity := span (mmt_encoder_stream_bytes(B, span, ...), mmt_encoder_stream_prepare(..., B, span, ...)), position
 * j lives in cache row j mod span, and a recording has no last window.  y_t is the row mmt_encoder_forward_band gives at [:, t];
 * while t < span it is the row of mmt_encoder_stream_step, bit for bit.  span < 1, t < 0 or t == INT_MAX returns MMT_EINVAL with a
 * message before anything else is looked at; span > 4096 is refused as a capacity > 4096 is. */
int mmt_encoder_stream_step_ring(const float* x_t, const float* mask_t, const float* params, float* y_t,
                                 void* state, size_t state_bytes, int t, int B, int span, int d, int h, int f, int n_layers,
                                 float eps, mmt_stream_t stream);

/* ---- The MFN gate, one window at a time (opt-in; eval mode, forward only).
 * Replaces one iteration t of MFN.forward's loop                               transformer/MFT/multiTransformer.py:200-247
 * (per-modality LSTMCell, cStar, the attention over the cell states, the memory candidate, both gates, the memory update and the
 * read-out MLP) for t = 0, 1, 2, ... of one recording per batch row: the state carries (h_m, c_m, mem) between the calls.  One step
 * is ONE launch, one workgroup per sequence, no communication between workgroups: a sequence's result does not depend on its batch.
 * Numerics: the batch path's rounding sites exactly (the left operand of every product and every weight bf16; sums, biases,
 * activations, softmax, the carried state and everything stored fp32); no site depends on a tile (csrc/mfn_step.h).
 * nmods modalities (1..4) with input widths in_dims[m] (multiples of 4, <= 512) and LSTM hidden sizes hidden[m] (multiples of 4,
 * their sum <= 256), both HOST arrays of nmods ints; the gate's other sizes are fixed: mem_dim 128, gamma hidden 64, att1 hidden 128,
 * att2 hidden 256, read-out hidden 64; 1 <= output_dim <= 256.  Anything else is MMT_EUNSUPPORTED with the limit named in
 * mmt_last_error(), at the size query (which then returns 0); non-positive sizes, null pointers and t < 0: MMT_EINVAL, before any launch.
 * `state`: mmt_mfn_stream_bytes() bytes, ANY CONTENTS: every word a step reads was written by mmt_mfn_stream_prepare or by the step
 * before it in this recording.  A new recording starts by passing t = 0 again; nothing needs clearing. */
/* (MFN.forward, :200-247) */
size_t mmt_mfn_stream_bytes(int B, int nmods, const int* in_dims, const int* hidden, int output_dim);
/* One launch: every parameter into the state, weights to bf16 in the step kernel's layout, biases in fp32 (b_ih + b_hh summed).
 * lstm_params: a HOST array of 4 * nmods device pointers, per modality weight_ih (4H,D), weight_hh (4H,H), bias_ih, bias_hh of its
 * nn.LSTMCell; gate_params: a HOST array of 20 device pointers, weight then bias of att1_fc1, att1_fc2, att2_fc1, att2_fc2, gamma1_fc1,
 * gamma1_fc2, gamma2_fc1, gamma2_fc2, out_fc1, out_fc2.  Does not touch the carried state.  Call it again after a parameter changes:
 * a step reads the biases from the state too.                                  (MFN.__init__ / forward, :118-180, :200-247) */
int mmt_mfn_stream_prepare(const float* const* lstm_params, const float* const* gate_params, void* state, size_t state_bytes,
                           int B, int nmods, const int* in_dims, const int* hidden, int output_dim, mmt_stream_t stream);
/* x_t: a HOST array of nmods device pointers, x_t[m] (B, in_dims[m]) -> y_t (B, output_dim) at position t; mask_t (B) float or NULL
 * multiplies the output row (MultiTransformer.forward's `* mask`, :310); the state advances under a blanked window as it does in
 * the batch path.  t is passed by value; step t reads copy t & 1 of the carried state and writes the other, so steps of one
 * recording must be enqueued in order t = 0, 1, ... on one stream.              (MFN.forward, :200-247; :310) */
int mmt_mfn_stream_step(const float* const* x_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                        int t, int B, int nmods, const int* in_dims, const int* hidden, int output_dim, mmt_stream_t stream);

/* ---- Slots: the positioned forms of both steps (opt-in).  The position of every sequence lives in DEVICE memory, `pos` (B ints), and
 * the kernel reads it, runs that window and advances it itself, so a step carries no host-side position: it can be captured into a
 * hipGraph and replayed, and the sequences of a batch may start and end at different calls.  Per sequence b (csrc/step_slots.h):
 *   pos[b] < 0                  idle: y_t[b] is written as zeros; nothing else is written, pos[b] stays
 *   0 <= pos[b] < limit         the step above at t = pos[b], bit for bit; then, if advance != 0, pos[b] = pos[b] + 1
 *   pos[b] >= limit, INT_MAX    full: as idle, and pos[b] stays, so the host can see it
 * A slot is seated by storing 0 to pos[b] and released by storing a negative value, between launches on the step's stream; at
 * position 0 no carried state and no cache row is read, so nothing else is needed.  No host-side check of the positions: the check is
 * the kernel's.  Plans, state layout, *_bytes and *_prepare are those above, and one state serves both forms.  A null `pos` is
 * MMT_EINVAL before any launch; every refusal of the step above passes through. */
/* The encoder step at t = pos[b]; the limit is `capacity`.                    (Encoder.forward, :73-76; departs from :27-31) */
int mmt_encoder_stream_step_slots(const float* x_t, const float* mask_t, const float* params, float* y_t,
                                  void* state, size_t state_bytes, int* pos, int advance,
                                  int B, int capacity, int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);
/* mmt_encoder_stream_step_ring at t = pos[b].  There is no limit: only idle slots and INT_MAX are skipped, and the position stored
 * after the step, pos[b] + 1, reaches INT_MAX at most, the value that never runs. */
int mmt_encoder_stream_step_ring_slots(const float* x_t, const float* mask_t, const float* params, float* y_t,
                                       void* state, size_t state_bytes, int* pos, int advance,
                                       int B, int span, int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);
/* The MFN gate step at t = pos[b]: copy pos[b] & 1 of the carried state is read and the other written, per sequence.  limit <= 0: no
 * limit (a gate has no cache); a gate behind encoders passes their capacity.   (MFN.forward, :200-247; :310) */
int mmt_mfn_stream_step_slots(const float* const* x_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                              int* pos, int limit, int advance,
                              int B, int nmods, const int* in_dims, const int* hidden, int output_dim, mmt_stream_t stream);

/* ---- The LSTM decoder and the read-out, one window at a time (opt-in; eval mode, forward only).
 * Replaces one iteration t of the decoder loop and the read-out MLP            transformer/SFT/multiTransformer.py:463-483
 * (nn.LSTM(2d, d, n_layers) fed [o_{t-1} ; enc_t] with o the top layer's output, o_{-1} = 0 and (dec_h0, dec_c0) the initial state;
 * then Linear(d, h_dim) -> ReLU -> Linear(h_dim, 1) -> * mask) for t = 0, 1, 2, ... of one recording per batch row: the state carries
 * (h, c) of every layer between the calls.  n_layers == 0: the read-out alone (transformer/B2-Trans/multiTransformer.py:400-402).
 * One step is ONE launch, one workgroup per sequence, no communication between workgroups: a sequence's result does not depend on its
 * batch.  Numerics: the batch path's rounding sites exactly (the left operand of every product and every weight bf16; sums, biases,
 * activations, the carried state and everything stored fp32); no site depends on a tile (csrc/decoder_step.h).
 * Limits: d % 4 == 0, 4 <= d <= 512, 1 <= h_dim <= 512, 0 <= n_layers <= 4, B >= 1: anything else is MMT_EUNSUPPORTED with the limit
 * named in mmt_last_error(), at the size query (which then returns 0); non-positive sizes, null pointers, t < 0 and a state of fewer
 * than mmt_decoder_stream_bytes() bytes: MMT_EINVAL, before any launch.
 * `state`: mmt_decoder_stream_bytes() bytes, ANY CONTENTS: every word a step reads was written by mmt_decoder_stream_prepare or by the
 * step before it in this recording.  A new recording starts by passing t = 0 again; nothing needs clearing. */
/* (_decode, :463-483) */
size_t mmt_decoder_stream_bytes(int B, int d, int h_dim, int n_layers);
/* One launch: every parameter into the state, weights to bf16 in the step kernel's layout (n_layers == 1: W_ih[:, :d] + W_hh summed
 * in fp32 and rounded once), vectors in fp32 (b_ih + b_hh summed).  lstm_params: a HOST array of 4 * n_layers device pointers, per
 * layer weight_ih (4d, 2d for layer 0, else d), weight_hh (4d, d), bias_ih, bias_hh; dec_h0, dec_c0 (n_layers, d); all three may be
 * NULL when n_layers == 0.  W1 (h_dim, d), b1, W2 (1, h_dim), b2: the read-out.  Does not touch the carried state.  Call it again
 * after a parameter changes.                                                   (__init__ / _decode, :444-452, :463-483) */
int mmt_decoder_stream_prepare(const float* const* lstm_params, const float* dec_h0, const float* dec_c0,
                               const float* W1, const float* b1, const float* W2, const float* b2, void* state, size_t state_bytes,
                               int B, int d, int h_dim, int n_layers, mmt_stream_t stream);
/* e_t (B, d), the encoder's row of this window -> y_t (B, 1) at position t; mask_t (B) float or NULL multiplies the output row; the
 * state advances under a blanked window as it does in the batch path.  t is passed by value; step t reads copy t & 1 of the carried
 * state and writes the other, so steps of one recording must be enqueued in order t = 0, 1, ... on one stream.   (_decode, :463-483) */
int mmt_decoder_stream_step(const float* e_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                            int t, int B, int d, int h_dim, int n_layers, mmt_stream_t stream);
/* The positioned form (the slots contract above): the step at t = pos[b]; copy pos[b] & 1 of the carried state is read and the other
 * written, per sequence.  limit <= 0: no limit; behind an encoder step its capacity.                            (_decode, :463-483) */
int mmt_decoder_stream_step_slots(const float* e_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                                  int* pos, int limit, int advance, int B, int d, int h_dim, int n_layers, mmt_stream_t stream);

/* ---- Prefill: open a recording from its history in ONE batch forward (opt-in; eval mode, forward only; csrc/step_prefill.h, the index
 * rule in csrc/step_prefill_plan.h).  This project's own addition.  Each entry is one launch that reads what a finished batch call left
 * behind and writes a stream state; no step kernel, no forward kernel and no state layout changes.
 * (dst, len): sequence b < B_src of the batch has len[b] windows, 1 <= len[b] <= P, and goes to sequence dst[b] < B_state of the
 * state.  Both null: dst[b] = b and len[b] = P, by value (a host stream, which then continues at t = P).  Both given: two int arrays
 * (B_src) in DEVICE memory (a slots stream); the kernel checks each pair against the launch arguments and skips one outside them.
 * pos: the stream's positions (B_state ints, device) or null; where given, pos[dst[b]] = len[b] is stored.  Distinct dst[b].
 * Nothing else of the state is written: no other sequence, no row >= len[b], no prepared weight.
 * MMT_EINVAL / MMT_EUNSUPPORTED before any launch, the limit named: null pointers, dst without len, B_src > B_state, P > capacity
 * (plain form), a workspace or a state smaller than its size query or not 16-byte aligned, and every refusal of the size queries. */
/* Replaces P calls of mmt_encoder_stream_step (ring != 0: mmt_encoder_stream_step_ring) at t = 0 .. P - 1.  `workspace`: that of a
 * finished mmt_encoder_forward_causal (ring: mmt_encoder_forward_band with the same span) of dims (B_src, P, d, h, f, n_layers) on
 * this stream, at least mmt_encoder_workspace_bytes_eval() bytes; it is only read.  `state`: mmt_encoder_stream_bytes(B_state, rows,
 * d, h, f, n_layers) bytes, rows = the capacity, or the span with ring != 0.  Per layer, K | V, sequence and head, the bf16 rows of
 * positions < len[b] (ring: the last min(len[b], span)) go to cache row pos (ring: pos mod span), the pad columns as zeros. */
int mmt_encoder_stream_prefill(const void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                               const int* dst, const int* len, int* pos, int B_src, int P, int B_state, int rows, int ring,
                               int d, int h, int f, int n_layers, mmt_stream_t stream);
/* Replaces P calls of mmt_decoder_stream_step at t = 0 .. P - 1 for n_layers == 1.  h_all, c_all: (P, B_src, d) fp32, what
 * mmt_lstm_scan_forward returned for the decoder's scan over the history: row len[b] - 1 of sequence b goes to copy len[b] & 1 of the
 * carried state of sequence dst[b], the copy step len[b] reads.  n_layers == 0 has no carried state: the positions alone (pos must be
 * given).  n_layers > 1: MMT_EUNSUPPORTED (the stacked scan returns the top layer only).  limit: the encoder's capacity, <= 0: none. */
int mmt_decoder_stream_prefill(const float* h_all, const float* c_all, void* state, size_t state_bytes,
                               const int* dst, const int* len, int* pos, int B_src, int P, int B_state, int limit,
                               int d, int h_dim, int n_layers, mmt_stream_t stream);

/* ---- Extend: move an encoder stream forward by C windows from ANY position (opt-in; eval mode, forward only; csrc/encoder_extend.h,
 * the index rule in csrc/encoder_extend_plan.h).  This project's own addition.  The state is the step's, untouched in layout
 * (mmt_encoder_stream_bytes / _prepare; the ring forms with capacity := span), so step, prefill and extend mix freely on one stream.
 * x (rows, C, d), mask (rows, C) float or NULL, y (rows, C, d): row i is what mmt_encoder_stream_step (ring: _step_ring) gives for
 * window t + i after windows t .. t + i - 1, to fp32 summation order: the same rounding sites, every product on the matrix cores.
 * A call runs as ceil(C / 16) launches in order on `stream`, each ONE kernel launch and nothing else; one workgroup per sequence and
 * no communication between workgroups, so a sequence's rows do not depend on its batch.  The plain forms write cache rows
 * t .. t + C - 1; the ring forms, of the c <= 16 rows of each launch, the last min(c, span) positions, position pos to row pos mod span.
 * MMT_EINVAL / MMT_EUNSUPPORTED before any launch, the limit named: null pointers, C < 1, t < 0, t + C > capacity (plain form; ring:
 * t + C reaching INT_MAX), a state smaller than its size query or not 16-byte aligned, every refusal of mmt_encoder_stream_bytes, and
 * a shape whose 16-row working set exceeds 160 KB of LDS (d = 512 with f = 2048: step through it). */
/* The host's form: all B sequences stand at t, passed by value, and get C windows; the stream then stands at t + C. */
int mmt_encoder_stream_extend(const float* x, const float* mask, const float* params, float* y, void* state, size_t state_bytes,
                              int t, int C, int B, int capacity, int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);
int mmt_encoder_stream_extend_ring(const float* x, const float* mask, const float* params, float* y, void* state, size_t state_bytes,
                                   int t, int C, int B, int span, int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);
/* The positioned forms (the slots contract above).  (dst, len): two int arrays (k) in DEVICE memory; row b < k of x goes to sequence
 * dst[b] < B_state with its first len[b] windows, 1 <= len[b] <= C, from position pos[dst[b]].  Distinct dst[b].  All or nothing, and
 * the same decision in every launch of the call: a pair outside its ranges, an idle slot, and a slot whose position plus len[b]
 * exceeds the capacity (ring: reaches INT_MAX) is skipped WHOLE: its rows of y are zeros, and no byte of its cache and no position
 * changes.  A slot that runs has rows >= len[b] of y as zeros and, with advance != 0, pos[dst[b]] += len[b], stored by the call's last
 * launch (the earlier ones read the position the call started on).  A sequence no dst names is not touched by a byte. */
int mmt_encoder_stream_extend_slots(const float* x, const float* mask, const float* params, float* y, void* state, size_t state_bytes,
                                    int* pos, const int* dst, const int* len, int advance, int C, int k, int B_state, int capacity,
                                    int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);
int mmt_encoder_stream_extend_ring_slots(const float* x, const float* mask, const float* params, float* y, void* state, size_t state_bytes,
                                         int* pos, const int* dst, const int* len, int advance, int C, int k, int B_state, int span,
                                         int d, int h, int f, int n_layers, float eps, mmt_stream_t stream);

/* ---- The LSTM baseline, ONE WINDOW PER CALL (csrc/lstm_step.h): embed, attention MLP, the n_layers LSTM cells from zero states, the
 * local attention over the last attn_len outputs with the softmax over the TAPS (mmt_local_attn_forward_taps) and the read-out MLP,
 * eval mode.  This project's own addition; it steps models._LocalAttnLSTM with attend_over_taps on (MultiLSTM, MultiLSTMB1).
 * One step is ONE launch, one workgroup per sequence, no communication between workgroups: a sequence's result does not depend on its
 * batch.  Numerics: the batch path's rounding sites exactly (the left operand of every product and every weight bf16; sums, biases,
 * activations, the softmax, the context, the carried state and everything stored fp32).
 * Dimensions (B, in, E, H, n_layers, attn_len): input width 1..2048, embed_dim 1..512, h_dim 1..512, n_layers 1..4, attn_len 1..16,
 * B >= 1: anything above a limit is MMT_EUNSUPPORTED with the limit named in mmt_last_error(), at the size query (which then returns
 * 0); non-positive sizes, null pointers, t < 0 and a state of fewer than mmt_lstm_stream_bytes() bytes: MMT_EINVAL, before any launch.
 * `state`: mmt_lstm_stream_bytes() bytes, ANY CONTENTS: every word a step reads was written by mmt_lstm_stream_prepare or by an earlier
 * step of this recording (two copies of (h, c) of every layer and a ring of attn_len rows of m_t * h_top per sequence).  A new
 * recording starts by passing t = 0 again; nothing needs clearing. */
size_t mmt_lstm_stream_bytes(int B, int in, int E, int H, int n_layers, int attn_len);
/* One launch: every parameter into the state, weights to bf16 in the step kernel's layout, vectors in fp32 (b_ih + b_hh summed).
 * params: a HOST array of 10 + 4 * n_layers device pointers: embed (W (E, in), b), attn[0] (W (E, E), b), attn[2] (W (attn_len, E), b),
 * per layer weight_ih (4H, E for layer 0, else H), weight_hh (4H, H), bias_ih, bias_hh, then the read-out (W (E, H), b, W (1, E), b).
 * Does not touch the carried state or the ring.  Call it again after a parameter changes. */
int mmt_lstm_stream_prepare(const float* const* params, void* state, size_t state_bytes,
                            int B, int in, int E, int H, int n_layers, int attn_len, mmt_stream_t stream);
/* x_t (B, in) -> y_t (B, 1) at position t; mask_t (B) float or NULL multiplies the top layer's output that enters the attention (now
 * and as a later tap) and the output row; (h, c) advance under a blanked window as they do in the batch path.  t is passed by value;
 * steps of one recording must be enqueued in order t = 0, 1, ... on one stream. */
int mmt_lstm_stream_step(const float* x_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                         int t, int B, int in, int E, int H, int n_layers, int attn_len, mmt_stream_t stream);
/* The positioned form (the slots contract above): the step at t = pos[b], per sequence.  limit <= 0: no limit. */
int mmt_lstm_stream_step_slots(const float* x_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                               int* pos, int limit, int advance, int B, int in, int E, int H, int n_layers, int attn_len,
                               mmt_stream_t stream);

/* ---- The LSTM baselines whose read-out feeds its own prediction back, ONE WINDOW PER CALL (csrc/lstm_step.h, the same body with a
 * tail; layout: csrc/lstm_feedback_step_plan.h), eval mode, free-running (the teacher-forced branch reads the current target, so it is
 * no online predictor).  This project's own addition; with attend_over_taps on it steps
 *   tail = 1: models.MultiEDLSTM, the decoder LSTM with the read-out MLP in its recurrence     (transformer/MFT/models.py:268-308),
 *   tail = 2: models.MultiARLSTM, the autoregressive read-out of order ar_order                 (transformer/MFT/models.py:354-400).
 * One step is ONE launch, one workgroup per sequence, no communication between workgroups.  Numerics: the rounding sites of the
 * batch path (mmt_lstm_fb_scan_forward, mmt_ar_combine_forward); tail 1 sums the read-out's last layer in another, fixed, order.
 * p_init stands in for the predictions before step 0 (the models' tgt_init); the UNMASKED prediction is what is fed back.
 * Dimensions: those of mmt_lstm_stream_* with, for tail 1, n_layers == 1 (ar_order is ignored) and, for tail 2, ar_order 1..16.
 * Anything above a limit is MMT_EUNSUPPORTED with the limit named in mmt_last_error(), at the size query (which then returns 0); an
 * unknown tail, non-positive sizes, null pointers, t < 0, a p_init that is not finite and a state of fewer than
 * mmt_lstm_feedback_stream_bytes() bytes: MMT_EINVAL, before any launch.
 * `state`: ANY CONTENTS; every word a step reads was written by the prepare entry or by an earlier step of this recording.  It holds
 * the state of mmt_lstm_stream_* and, behind it, tail 1: the decoder's weights, the four initial rows and two copies of (hd, cd, q)
 * per sequence; tail 2: autoreg's weights and a ring of ar_order + 1 predictions per sequence (step t writes slot t % (ar_order + 1)
 * and reads the ar_order slots below it, never the one it writes). */
size_t mmt_lstm_feedback_stream_bytes(int tail, int ar_order, int B, int in, int E, int H, int n_layers, int attn_len);
/* One launch: every parameter into the state; does not touch a carried block or a ring.  params: a HOST array of device pointers, first
 * the 10 + 4 * n_layers of mmt_lstm_stream_prepare (the LSTM being the one that reads the embedding: `encoder` for tail 1; the
 * read-out being out.0, out.2 for tail 1 and decoder.0, decoder.2 for tail 2), then
 *   tail 1 (9): decoder.weight_ih_l0 (4H, 1 + H), its column 0 as a contiguous (4H) vector, decoder.weight_hh_l0 (4H, H),
 *               decoder.bias_ih_l0, decoder.bias_hh_l0 (4H), enc_h0, enc_c0, dec_h0, dec_c0 (H each);
 *   tail 2 (2): autoreg.weight (ar_order, H), autoreg.bias (ar_order).                  (__init__, :233-266 and :322-352) */
int mmt_lstm_feedback_stream_prepare(const float* const* params, void* state, size_t state_bytes, int tail, int ar_order,
                                     int B, int in, int E, int H, int n_layers, int attn_len, mmt_stream_t stream);
/* x_t (B, in) -> y_t (B, 1) at position t = the row the model's eval forward(target=None, tgt_init=p_init) gives at [:, t]; mask_t as
 * in mmt_lstm_stream_step.  t is passed by value; steps of one recording must be enqueued in order t = 0, 1, ... on one stream.
 *                                                                                                        (forward, :268-308, :354-400) */
int mmt_lstm_feedback_stream_step(const float* x_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                                  int t, float p_init, int tail, int ar_order, int B, int in, int E, int H, int n_layers, int attn_len,
                                  mmt_stream_t stream);
/* The positioned form (the slots contract above): the step at t = pos[b], per sequence.  limit <= 0: no limit.  With advance == 0 the
 * call is repeatable: no word it reads is one it writes.                                              (forward, :268-308, :354-400) */
int mmt_lstm_feedback_stream_step_slots(const float* x_t, const float* mask_t, float* y_t, void* state, size_t state_bytes,
                                        int* pos, int limit, int advance, float p_init, int tail, int ar_order,
                                        int B, int in, int E, int H, int n_layers, int attn_len, mmt_stream_t stream);

/* ---- Fused affine map  y = act(x W^T + b) [* rowscale] on bf16 MFMA.
 * Replaces nn.Linear (+ F.relu) call sites of the path: PositionwiseFeedForward (:15-20), the four
 * attention projections (:43,55,65), embeds and read-out MLPs (:270,296,340-342,400-402).
 * x (M,K), W (N,K), b (N) or NULL, y (M,N), all fp32; act: 0 none, 1 ReLU, 2 tanh, 3 sigmoid; rowscale (M) or NULL. */
/* workspace: zero once; reusable for the same (M, K, N), with or without dropout, rowscale and bias, for any act. */
size_t mmt_linear_workspace_bytes(int M, int K, int N);
int mmt_linear_forward(const float* x, const float* W, const float* b, const float* rowscale, float* y,
                       void* workspace, size_t workspace_bytes, int M, int K, int N, int act, mmt_stream_t stream);
/* dx (M,K) or NULL; dW (N,K), db (N) or NULL.  `y` is the forward output (activation-derivative source when act != 0). */
int mmt_linear_backward(const float* dy, const float* x, const float* W, const float* y, const float* rowscale,
                        float* dx, float* dW, float* db,
                        void* workspace, size_t workspace_bytes, int M, int K, int N, int act, mmt_stream_t stream);

/* ... with W and b prepared once (forward only; a stream's embed, whose weights do not change between steps): `prepared`,
 * mmt_linear_prepared_bytes(K, N) bytes, any contents, receives from mmt_linear_prepare (two launches) what mmt_linear_forward lays into
 * its workspace at every call, the padded bf16 W and the padded fp32 bias (b may be NULL: zeros).  mmt_linear_forward_prepared is then
 * ONE launch, the row GEMM alone on the same operands: the same bits as mmt_linear_forward.  Prepare again after W or b changed. */
size_t mmt_linear_prepared_bytes(int K, int N);
int mmt_linear_prepare(const float* W, const float* b, void* prepared, size_t prepared_bytes, int K, int N, mmt_stream_t stream);
int mmt_linear_forward_prepared(const float* x, const void* prepared, size_t prepared_bytes, const float* rowscale, float* y,
                                int M, int K, int N, int act, mmt_stream_t stream);

/* ... with train-mode dropout fused in: on the INPUT (x -> drop(x) while the A tile is staged: the `Dropout(0.1) -> Linear -> ReLU` embed of
 * NLPTransformer, transformer/SFT/multiTransformer.py:431-433,461) and / or behind the ReLU (act must be 1: MFN's out_dropout on
 * relu(out_fc1), transformer/MFT/multiTransformer.py:244-245).  Streams 2000 (input, index m*KP + k, KP = K rounded up to 64) and 2001
 * (output, index m*NP + n) of mmt_debug_dropout_mask.  seed_state: NULL (seed by value) or a device-resident seed as in
 * mmt_encoder_forward_devseed; the backward then passes device_seeded = 1 (the seed sits in the workspace) and any seed. */
int mmt_linear_dropout_forward(const float* x, const float* W, const float* b, const float* rowscale, float* y,
                               void* workspace, size_t workspace_bytes, int M, int K, int N, int act,
                               float in_dropout_p, float out_dropout_p, uint64_t seed, uint64_t* seed_state, mmt_stream_t stream);
int mmt_linear_dropout_backward(const float* dy, const float* x, const float* W, const float* y, const float* rowscale,
                                float* dx, float* dW, float* db,
                                void* workspace, size_t workspace_bytes, int M, int K, int N, int act,
                                float in_dropout_p, float out_dropout_p, uint64_t seed, int device_seeded, mmt_stream_t stream);

/* ---- Data movement between the kernels of a sequence model, so that its forward and backward run no library kernel: up to any number of
 * strided 2-D fp32 copies per call (24 per launch).  Replaces the torch.cat / stack / permute / slicing / broadcasting glue of
 * MFN.forward (cStar = [c_{t-1}; c_t] :212-217, [h; mem] :241-243), MultiTransformer.forward (permute :300, `* mask` :310) and of the SFT decoder
 * (transformer/SFT/multiTransformer.py:463-483) and their autograd twins.
 * dst[perm(r)][c] (+)= rowscale[.] * (src[r][c] + src2[r][c]) for r < rows, c < cols.  src NULL: zeros; src2 optional; a stride of 0
 * broadcasts one row; perm 1: source rows are batch-major (b*T+t), destination rows time-major (t*B+b); perm 2: the reverse; rowscale is
 * indexed by the batch-major row under a permutation.  Segments of one call must not overlap in their destinations. */
typedef struct {
    const float* src; const float* src2; float* dst; const float* rowscale;
    int rows, cols, src_ld, src2_ld, dst_ld, perm, pB, pT, accumulate;
} mmt_copy_seg;
int mmt_copy2d(const mmt_copy_seg* host_segs, int nsegs, mmt_stream_t stream);

/* attended = softmax(logits, over the N features) * v, att kept for the backward.   Replaces transformer/MFT/multiTransformer.py:218-219
 * backward: dlogits = att * (dout * v - sum_n dout v att), dv = dout * att. */
int mmt_softmax_mul_forward(const float* logits, const float* v, float* att, float* out, int M, int N, mmt_stream_t stream);
int mmt_softmax_mul_backward(const float* dout, const float* att, const float* v, float* dlogits, float* dv, int M, int N, mmt_stream_t stream);
/* out[c] = sum over `rows` rows of x (row stride ld): gradient of a row that the forward broadcast over the batch. */
int mmt_colsum(const float* x, float* out, int rows, int cols, int ld, mmt_stream_t stream);

/* Highway combine of the window encoder with the Dropout(0.3) the front-end applies to it.
 * Replaces `x_gate * x_proj + (1 - x_gate) * x_conv_out` (transformer/SFT/models.py:47-55; MFT / B2-Trans twins) and `self.dropout(...)`
 * (transformer/SFT/models.py:132-134): out = drop(gate * proj + (1 - gate) * x) over n elements; proj / gate are the outputs of the two
 * Linear layers (mmt_linear_forward, act 0 / 3).  Dropout stream 3000 of mmt_debug_dropout_mask, index = element.
 * seed_state: NULL (seed by value) or a device-resident seed as in mmt_encoder_forward_devseed; then `seedblock` (2 uint64 of device
 * memory) receives the seed of this call and its stream keys, and the backward takes the same block instead of a seed.
 * backward: g = drop'(dout); dx = g (1 - gate) [the direct path only: add the two Linear layers' input gradients], dproj = g gate,
 * dgate = g (proj - x) [w.r.t. the gate's OUTPUT: the sigmoid's derivative is mmt_linear_backward's, act 3]. */
int mmt_highway_forward(const float* x, const float* proj, const float* gate, float* out, size_t n,
                        float dropout_p, uint64_t seed, uint64_t* seed_state, uint64_t* seedblock, mmt_stream_t stream);
int mmt_highway_backward(const float* dout, const float* x, const float* proj, const float* gate, float* dx, float* dproj, float* dgate,
                         size_t n, float dropout_p, uint64_t seed, const uint64_t* seedblock, mmt_stream_t stream);

/* accum[0] |= word[0] on the device, in stream order: keeps a kernel's device error word (mmt_lstm_scan_*: first word of the workspace)
 * beyond the life of its workspace, also inside a captured hipGraph.  Both pointers are device memory. */
int mmt_error_accumulate(const uint32_t* word, uint32_t* accum, mmt_stream_t stream);

/* ---- LSTM recurrence over T steps with the input projection already applied.
 * Replaces the per-step nn.LSTMCell loop of MFN.forward       transformer/MFT/multiTransformer.py:200-208
 * and the per-step nn.LSTM call of the SFT decoder            transformer/SFT/multiTransformer.py:471-476.
 * gx (T,B,4H) = x_t W_ih^T + b_ih + b_hh (gate order i,f,g,o); W_rec (4H,H) multiplies h_{t-1};
 * h0,c0 (B,H) or NULL (zeros).  Outputs h_all, c_all (T,B,H) and the gate activations acts (T,B,4H)
 * kept for the backward.  H % 4 == 0, H <= 256.
 * Device error word: the first uint32 of `workspace` is zeroed by every call and is non-zero once the kernels have run
 * if a scan for H > 128 (four workgroups per sequence exchanging h through memory) timed out waiting for a partner
 * workgroup — e.g. another process held the CUs.  The outputs are then INVALID.  Nothing synchronises here: read the word
 * after the stream has drained (the Python wrapper does, functional.check_device_errors()). */
/* workspace: any contents (every word used is written first; the error block and the exchange granules are cleared by a kernel of
 * the call). */
size_t mmt_lstm_scan_workspace_bytes(int H);
int mmt_lstm_scan_forward(const float* gx, const float* W_rec, const float* h0, const float* c0,
                          float* h_all, float* c_all, float* acts, void* workspace, size_t workspace_bytes,
                          int T, int B, int H, mmt_stream_t stream);
/* dh_all, dc_all: gradients on the (T,B,H) outputs (either may be NULL).  dgx (T,B,4H) is the gradient of gx
 * (also the operand of the batched dW_ih / dW_rec products); dh0, dc0 (B,H) or NULL. */
int mmt_lstm_scan_backward(const float* dh_all, const float* dc_all, const float* W_rec, const float* c0,
                           const float* c_all, const float* acts, float* dgx, float* dh0, float* dc0,
                           void* workspace, size_t workspace_bytes, int T, int B, int H, mmt_stream_t stream);

/* ---- Stacked LSTM scan: the autoregressive decoder with n_layers = L > 1.
 * Replaces the per-step call of a multi-layer nn.LSTM on [o_{t-1} ; enc_t]   transformer/SFT/multiTransformer.py:444-446,463-483
 *                                                                           transformer/MFT/multiTransformer.py:335-337,357-376
 * With d = H and gate order i,f,g,o:  o_{-1} = 0 (zeros, not h0[L-1]);  h^l_{-1} = h0[l], c^l_{-1} = c0[l];
 *   g^0_t = gx0_t + [o_{t-1} ; h^0_{t-1}] P_0^T          gx0 (T,B,4H) = enc_t W_ih_l0[:, d:]^T + b_ih_l0 + b_hh_l0, computed by the caller
 *   g^l_t = bias_{l-1} + [h^{l-1}_t ; h^l_{t-1}] P_l^T   l = 1 .. L-1;    o_t = h^{L-1}_t
 * P (L,4H,2H) fp32 packed weights: P_0 = [W_ih_l0[:, :d] | W_hh_l0], P_l = [W_ih_l | W_hh_l]; bias (L-1,4H) = b_ih_l + b_hh_l of
 * layers >= 1; h0, c0 (L,B,H) or NULL (zeros).  Outputs h_all, c_all (L,T,B,H) and the gate activations acts (L,T,B,4H) kept for the
 * backward.  With the first H columns of P_0 zero this is a plain stacked LSTM.
 * Limits: 2 <= L <= 4, H % 4 == 0, H <= 128, B <= 512; anything else returns MMT_EINVAL (the workspace query returns 0) with the limit
 * named in mmt_last_error().  One workgroup scans its sequences alone: no device error word.  bf16 MFMA operands, fp32 accumulation
 * and cell state, as mmt_lstm_scan_*. */
/* workspace: zero once; reusable for the same (H, L) with any T and B, by the forward and the backward (each prepares its own weight
 * fragments; nothing is kept in it between the two). */
size_t mmt_lstm_stack_workspace_bytes(int H, int L);
int mmt_lstm_stack_scan_forward(const float* gx0, const float* P, const float* bias, const float* h0, const float* c0,
                                float* h_all, float* c_all, float* acts, void* workspace, size_t workspace_bytes,
                                int T, int B, int H, int L, mmt_stream_t stream);
/* dh_top (T,B,H): the gradient on the TOP layer's outputs h_all[L-1] (or NULL); c0, c_all, acts as the forward had them.
 * dG (L,T,B,4H): the gate pre-activation gradients — dG[0] is the gradient of gx0, dG[l] the operand of dP_l = dG[l]^T [x_a ; x_b] and
 * of the bias gradients (column sums), which the caller forms in batched GEMMs.  dh0, dc0 (L,B,H) or NULL. */
int mmt_lstm_stack_scan_backward(const float* dh_top, const float* P, const float* c0, const float* c_all, const float* acts,
                                 float* dG, float* dh0, float* dc0, void* workspace, size_t workspace_bytes,
                                 int T, int B, int H, int L, mmt_stream_t stream);

/* ---- LSTM scan with the read-out MLP inside its recurrence: the decoder loop of the encoder-decoder LSTM, nn.LSTM(1 + H, H) called one
 * step at a time on [p_{t-1} ; ctx_t] with p_t = out(h_t)                          transformer/MFT/models.py:290-305
 *   gates_t = gxc_t + p_{t-1} w_p + h_{t-1} W_hh^T,  (h_t, c_t) = cell(gates_t, c_{t-1}),  p_{-1} = p_init, h_{-1} = h0, c_{-1} = c0
 *   u_t = ReLU(W1 h_t + b1),  p_t = w2 . u_t + b2
 * gxc (T,B,4H) = ctx W_ih[:, 1:]^T + b_ih + b_hh (one batched GEMM before the scan); w_p (4H) = W_ih[:, 0]; W_hh (4H,H); W1 (E,H),
 * b1 (E) = out.0; w2 (E), b2 (1) = out.2; h0, c0 (B,H) or NULL (zeros).  Outputs p_all (T+1,B): row 0 holds p_init and row t + 1
 * holds p_t (rows 0 .. T-1 are the p_{t-1} operand of dw_p); h_all, c_all (T,B,H), acts (T,B,4H), u_all (T,B,E) kept for the backward.
 * Limits: H % 4 == 0, 4 <= H <= 128, E % 4 == 0, 4 <= E <= 128, B <= 512: MMT_EUNSUPPORTED with the limit named in mmt_last_error()
 * (the workspace query returns 0); T or B < 1, null pointers: MMT_EINVAL.  One workgroup scans its sequences alone: no device error
 * word.  bf16 MFMA operands (h, W_hh, W1; backward: dG, du), everything else and every sum fp32. */
/* workspace: zero once; reusable for the same (H, E) with any T and B, by the forward and the backward (as the stacked scan's). */
size_t mmt_lstm_fb_scan_workspace_bytes(int H, int E);
int mmt_lstm_fb_scan_forward(const float* gxc, const float* w_p, const float* W_hh, const float* W1, const float* b1,
                             const float* w2, const float* b2, const float* h0, const float* c0, float p_init,
                             float* h_all, float* c_all, float* acts, float* u_all, float* p_all,
                             void* workspace, size_t workspace_bytes, int T, int B, int H, int E, mmt_stream_t stream);
/* The backward of the loop above (transformer/MFT/models.py:290-305), t = T-1 .. 0.  dp_ext (T,B): the gradient on p_all.
 * dG (T,B,4H): the gate pre-activation gradients — the gradient of gxc, and the operand of dW_hh = dG^T h_prev and dw_p = sum p_prev dG;
 * du (T,B,E): the gradient of the MLP's pre-activations (dW1 = du^T h, db1 = its column sums); dp (T,B): the full gradient of p_t
 * (dw2 = sum dp u, db2 = sum dp).  The caller forms those in batched GEMMs.  dh0, dc0 (B,H) or NULL. */
int mmt_lstm_fb_scan_backward(const float* dp_ext, const float* w_p, const float* W_hh, const float* W1, const float* w2,
                              const float* c0, const float* c_all, const float* acts, const float* u_all,
                              float* dG, float* du, float* dp, float* dh0, float* dc0,
                              void* workspace, size_t workspace_bytes, int T, int B, int H, int E, mmt_stream_t stream);

/* ---- Local attention of the LSTM baselines: the softmax of the attention MLP's logits and the convolution of the LSTM outputs
 * with them.  Replaces `attn = self.attn(embed)`'s nn.Softmax(dim=1), pad_packed_sequence's zeroing and convolve / pad_shift
 *                                                             transformer/B1-LSTM/models.py:10-25,186-207
 *                                                             (the shared MultiLSTM copy: transformer/SFT/models.py:10-25,195-216)
 * z (B,T,L) logits; h (T,B,H) the LSTM outputs, time-major as mmt_lstm_scan_forward writes them; valid (B,T) the prefix mask {0,1}.
 * Outputs ctx (B,T,H) = sum_{i<L, t-i>=0} a[b,t,i] valid[b,t-i] h[t-i,b,:] and attn = a (B,T,L), kept for the backward, where
 * a[b,t,i] = softmax over t of z[b,:,i]: the reference's dim=1 is the TIME axis of the 3-D logits, so each of the L columns is
 * normalised over all T steps of the padded batch, padded steps included.  1 <= L <= 16; any B >= 1, T >= 1 (taps before step 0
 * are zero), H >= 1 (four-float accesses when H % 4 == 0 and h / ctx are 16-byte aligned).  No workspace. */
int mmt_local_attn_forward(const float* z, const float* h, const float* valid, float* ctx, float* attn,
                           int B, int T, int H, int L, mmt_stream_t stream);
/* dctx (B,T,H) -> dz (B,T,L), dh (T,B,H) (zero at steps where valid == 0).  Two launches; deterministic (no atomics).
 * workspace: mmt_local_attn_workspace_bytes(B,T,H,L) bytes, any contents (every word used is written first); 0 = bad arguments. */
size_t mmt_local_attn_workspace_bytes(int B, int T, int H, int L);
int mmt_local_attn_backward(const float* dctx, const float* attn, const float* h, const float* valid, float* dz, float* dh,
                            void* workspace, size_t workspace_bytes, int B, int T, int H, int L, mmt_stream_t stream);
/* The second mode (models.attend_over_taps): a[b,t,:] = softmax over the L TAPS of row (b,t), all L of them (taps that reach before
 * step 0 or onto a masked step take part and bring zero rows), so that ctx[b,t] depends on steps <= t alone.  Same arguments, layouts,
 * limits, launches and workspace (mmt_local_attn_workspace_bytes) as the two entries above; dz = a (da - sum_i a da) per row. */
int mmt_local_attn_forward_taps(const float* z, const float* h, const float* valid, float* ctx, float* attn,
                                int B, int T, int H, int L, mmt_stream_t stream);
int mmt_local_attn_backward_taps(const float* dctx, const float* attn, const float* h, const float* valid, float* dz, float* dh,
                                 void* workspace, size_t workspace_bytes, int B, int T, int H, int L, mmt_stream_t stream);

/* ---- Autoregressive read-out of the LSTM baseline MultiARLSTM: the teacher-forced sum and the free-running step loop
 *                                                             transformer/MFT/models.py:381-386 (teacher-forced), :388-397 (free-running),
 *                                                             :399 (mask); the same lines in SFT, B2-Trans, B3-MFN, Performance-Eval
 *                                                             and B1-LSTM
 * in_part (B,T) = decoder(context); w (B,T,K) = autoreg(context), K = ar_order; mask (B,T) {0,1}; target (B,T) or NULL.
 *   target given:  p[b,t] = in_part[b,t] + sum_{i<K} w[b,t,i] target[b,t-i],  target[b,s<0] = 0 (not p_init); tap 0 reads the current target
 *   target NULL:   p[b,t] = in_part[b,t] + sum_{k<K} w[b,t,k] p[b,t-K+k],     p[b,s<0] = p_init; tap K-1 reads the newest prediction
 * Outputs p (B,T), kept for the backward, and out (B,T) = p * mask.  The free-running loop is ONE launch (a wave per sequence).
 * 1 <= K <= 16: anything else MMT_EUNSUPPORTED with the limit named in mmt_last_error(), before any launch; B or T < 1, null pointers:
 * MMT_EINVAL.  T < K, T = 1 and B = 1 are legal.  fp32, no atomics, no workspace. */
int mmt_ar_combine_forward(const float* in_part, const float* w, const float* mask, const float* target, float p_init,
                           float* p, float* out, int B, int T, int K, mmt_stream_t stream);
/* dout (B,T) on out -> din_part (B,T) = dout * mask and dw (B,T,K) = din_part[b,t] * hist, one element-wise launch.  The reference
 * detaches the fed-back predictions (:392), so nothing flows through the history.  hist (B,T): the target (teacher_forced != 0: tap k
 * reads target[b,t-k], zero before step 0) or the forward's p (teacher_forced == 0: tap k reads p[b,t-K+k], p_init before step 0). */
int mmt_ar_combine_backward(const float* dout, const float* mask, const float* hist, int teacher_forced, float p_init,
                            float* din_part, float* dw, int B, int T, int K, mmt_stream_t stream);

/* ---- MFN delta-memory recurrence.  Replaces the memory update inside MFN.forward's time loop
 *                                                             transformer/MFT/multiTransformer.py:221-224
 * apre (T,B,128): gamma{1,2}_fc1 applied to the `attended` part of `both` (+bias), rows [gamma1(64); gamma2(64)];
 * Wm (128,128): the memory columns of gamma{1,2}_fc1.weight stacked the same way; W2 (2,128,64), b2 (2,128):
 * gamma{1,2}_fc2; chat (T,B,128) = cHat.  Outputs mem_all (T,B,128) and u_all (T,B,128), g_all (T,B,256) kept
 * for the backward.  mem_dim must be 128 and h_gamma 64 (the reference's constants, :133,140-141).
 * dropout_p / seed: gamma{1,2}_dropout on relu(fc1) in train mode (0 = eval). */
/* workspace: any contents (every word used is written first). */
size_t mmt_mfn_mem_scan_workspace_bytes(void);
int mmt_mfn_mem_scan_forward(const float* apre, const float* chat, const float* Wm, const float* W2, const float* b2,
                             float* mem_all, float* u_all, float* g_all, void* workspace, size_t workspace_bytes,
                             int T, int B, int mem_dim, int h_gamma, float dropout_p, uint64_t seed, mmt_stream_t stream);
/* the same with a device-resident seed (see mmt_encoder_forward_devseed); the backward needs none (u_all keeps the dropped values) */
int mmt_mfn_mem_scan_forward_devseed(const float* apre, const float* chat, const float* Wm, const float* W2, const float* b2,
                                     float* mem_all, float* u_all, float* g_all, void* workspace, size_t workspace_bytes,
                                     int T, int B, int mem_dim, int h_gamma, float dropout_p, uint64_t* seed_state, mmt_stream_t stream);
/* dmem_all (T,B,128) or NULL -> dchat (T,B,128), dapre (T,B,128), dz_all (T,B,256) (pre-sigmoid gate gradients). */
int mmt_mfn_mem_scan_backward(const float* dmem_all, const float* chat, const float* mem_all, const float* u_all,
                              const float* g_all, const float* Wm, const float* W2,
                              float* dchat, float* dapre, float* dz_all, void* workspace, size_t workspace_bytes,
                              int T, int B, int mem_dim, int h_gamma, float dropout_p, mmt_stream_t stream);

/* ---- Window encoder: Conv1d(D -> F, kernel 2, bias) over the W positions (tokens / frames) of each window followed by
 *      the global max-pool over the W-1 conv positions.  Replaces CNN.forward
 *                                                             transformer/SFT/models.py:57-79 (call site :118-127;
 *                                                             same class in MFT/models.py:57-79, B2-Trans/models.py:57-79)
 * x fp32 (N, W, D) contiguous: N = B*T windows (the reference loops over the batch; windows are independent), D % 4 == 0,
 * W >= 2.  weight fp32 (F, D, 2) in nn.Conv1d's layout, bias (F).  out fp32 (N, F); argmax int32 (N, F): the conv position
 * of the maximum (first one on ties), saved for the backward.  Kernel size 2 (the reference's constant, :82); other sizes: mmt_convpool_k_*. */
/* workspace: any contents (every word used is written first: the padded weights by the forward's first kernel, the backward's
 * partial sums by its first). */
size_t mmt_convpool_workspace_bytes(int N, int W, int D, int F);
int mmt_convpool_forward(const float* x, const float* weight, const float* bias, float* out, int32_t* argmax,
                         void* workspace, size_t workspace_bytes, int N, int W, int D, int F, mmt_stream_t stream);
/* dout (N, F) -> dweight (F, D, 2), dbias (F).  There is no dx: the windows are input data (the reference never
 * differentiates them either). */
int mmt_convpool_backward(const float* x, const float* dout, const int32_t* argmax, float* dweight, float* dbias,
                          void* workspace, size_t workspace_bytes, int N, int W, int D, int F, mmt_stream_t stream);

/* ---- Window encoder with K taps: Conv1d(D -> F, kernel K, bias) followed by the global max-pool over the W-K+1 conv
 *      positions, for 1 <= K <= 5.  The reference passes its k argument straight to nn.Conv1d
 *                                                             transformer/SFT/models.py:57-79 (CNN), :82-93 (k reaches every CNN)
 * Arguments as mmt_convpool_*, with weight / dweight fp32 (F, D, K) in nn.Conv1d's layout, W >= K, argmax in [0, W-K] (first
 * maximum on ties).  K outside 1..5: MMT_EUNSUPPORTED ("kernel size"); W < K, non-positive sizes, null pointers: MMT_EINVAL;
 * D % 4 != 0: MMT_EUNSUPPORTED.  The workspace query returns 0 for a refused shape, with mmt_last_error() set.  Same numerics
 * as the 2-tap entries (bf16 operands, fp32 accumulation, bias after the pool, no atomics); K = 2 is accepted but runs other
 * kernels than mmt_convpool_* (the Python layer keeps k = 2 on those). */
/* workspace: any contents (every word used is written first), as mmt_convpool_*. */
size_t mmt_convpool_k_workspace_bytes(int N, int W, int D, int F, int K);
int mmt_convpool_k_forward(const float* x, const float* weight, const float* bias, float* out, int32_t* argmax,
                           void* workspace, size_t workspace_bytes, int N, int W, int D, int F, int K, mmt_stream_t stream);
/* dout (N, F) -> dweight (F, D, K), dbias (F).  There is no dx. */
int mmt_convpool_k_backward(const float* x, const float* dout, const int32_t* argmax, float* dweight, float* dbias,
                            void* workspace, size_t workspace_bytes, int N, int W, int D, int F, int K, mmt_stream_t stream);

/* ---- Training loss and its gradient in one pass.
 * Replaces criterion(output, target) / sum(lengths) and its autograd backward   transformer/SFT/train.py:133-139 (criterion :538)
 * loss[0] = sum((pred - target)^2) * inv_denom (fp64 accumulation, deterministic);  dpred = 2 (pred - target) * inv_denom.
 * pred, target, dpred: n fp32 (16-byte aligned); scratch: mmt_mse_sum_scratch_doubles(n) doubles; all on the device. */
size_t mmt_mse_sum_scratch_doubles(size_t n);
int mmt_mse_sum_forward(const float* pred, const float* target, float inv_denom, float* loss, float* dpred, double* scratch,
                        size_t n, mmt_stream_t stream);

/* ---- Optimiser step.
 * Replaces optimizer.step() of torch.optim.Adam(lr, weight_decay) (L2 form, not AdamW)   transformer/SFT/train.py:621, called at :141
 * on `nchunks` contiguous fp32 ranges (parameter, gradient, first and second moment of chunk c: counts[c] elements each) in one
 * launch per 48 chunks.  `step` = 1, 2, ... (bias corrections 1 - beta^step are taken on the host).  The pointer arrays are HOST arrays
 * of device pointers. */
int mmt_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const size_t* counts, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int step, mmt_stream_t stream);

/* ---- Concordance correlation coefficient per sequence, on the device.
 * Replaces eval_ccc + the per-sequence host loop of evaluate()     transformer/SFT/train.py:42-50, :236-238
 * pred, target: (B, T) fp32 row-major (the (B,T,1) valence tensors); lengths: B int32 on the device; sequence b uses its first
 * lengths[b] windows.  ccc: B float64 on the device: 2 cov / (var_t + var_p + (mean_p - mean_t)^2) with population moments
 * (np.var, np.cov(bias=True)), accumulated in fp64; NaN for a sequence with fewer than 2 windows or zero spread in both. */
int mmt_ccc_forward(const float* pred, const float* target, const int32_t* lengths, double* ccc, int B, int T, mmt_stream_t stream);

/* ---- Test hook: the keep-mask (1 = kept) of dropout stream `stream_id` for indices [0,n) under (p, seed), and the
 * scale applied to kept values (host pointer, may be NULL).  Streams used by the encoder stack for layer l:
 * 4l+0 attention probabilities, index ((b*h+head)*Tp + q)*Tp + key (Tp = T rounded up to 32; pass attn_Tp = Tp and
 *      n = B*h*Tp*Tp; 0 for every other stream).  These are stored bit masks drawn once per forward (csrc/attn_mask.h);
 * 4l+1 / 4l+3 sublayer outputs and 4l+2 FFN hidden, index m*NP + n (NP = width rounded up to 64);
 * 1000: MFN gamma hidden, index (t*B+b)*128 + j. */
int mmt_debug_dropout_mask(float p, uint64_t seed, uint32_t stream_id, uint64_t n, uint32_t attn_Tp, uint8_t* keep,
                           float* host_scale_out, mmt_stream_t stream);

/* ---- Test hook: the attention-dropout generator's stored words of one layer (nbh * nt * nt blocks of 32x32 decisions, 64 uint16 per
 * block and array), as the kernels read them: lq in the 16-bit lane-word form (lanes = 0) or the 64-bit lane-mask form (lanes = 1), lk
 * always in the lane-word form.  The decisions are those of mmt_debug_dropout_mask(p, seed, stream_id, ..., attn_Tp = 32 nt). */
int mmt_debug_attn_mask_words(float p, uint64_t seed, uint32_t stream_id, int nbh, int nt, int lanes,
                              uint16_t* lq, uint16_t* lk, mmt_stream_t stream);

/* ---- Test hook: fill every LDS word of every CU, and the vector registers of every SIMD, with `pattern` (e.g. 0x7FC00000, a NaN).
 * Kernels must not depend on LDS or registers they did not write; tests run a workload, poison, run it again and require identical results.  `sink4`: any 4 writable device bytes. */
int mmt_debug_poison_lds(uint32_t pattern, void* sink4, mmt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMT_HIP_H */
