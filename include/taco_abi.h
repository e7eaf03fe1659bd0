/* taco_abi.h -- C ABI of libtaco_hip.so, the MI355X (gfx950) Tacotron hot path.
 *
 * The reference (GSByeon/multi-speaker-tacotron-tensorflow) has no FFI/plugin interface: its hot
 * path is the TF1 graph built by Tacotron.initialize() (models/tacotron.py:21-271) and executed by
 * sess.run from Synthesizer.synthesize (synthesizer.py:166-167) and train() (train.py:217-219).
 * This header is the boundary a maintainer would bind instead of sess.run (see INTEGRATION.md for
 * the ctypes stub).  Each entry point cites the reference lines it replaces.
 *
 * Conventions: extern "C"; plain pointers and sizes; fp32 row-major [batch, time, channels];
 * all `d_*` pointers are DEVICE pointers owned by the caller; the library owns only the weight
 * pack inside taco_model.  Every call is asynchronous on `hip_stream` (a hipStream_t passed as
 * void*), performs no allocation and no host<->device synchronisation, and is hipGraph-capturable.
 * Return value 0 = OK; negative = error class below, text in taco_last_error().
 */
#ifndef TACO_ABI_H
#define TACO_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TACO_ABI_VERSION 1

#define TACO_OK 0
#define TACO_ERR_ARG (-1)         /* null pointer, bad size, unknown name */
#define TACO_ERR_SHAPE (-2)       /* weight/activation shape mismatch (tacotron.py:192-194) */
#define TACO_ERR_UNSUPPORTED (-3) /* unknown model_type / attention_type (tacotron.py:88,152) */
#define TACO_ERR_HIP (-4)         /* HIP runtime error */
#define TACO_ERR_STATE (-5)       /* model not finalized / missing weights / workspace too small */

typedef struct taco_model taco_model; /* opaque: hparams + device weight pack */
typedef struct taco_plan taco_plan;   /* opaque: an instantiated hipGraph of one forward */

/* Mirrors the model keys of hparams.py:33-69 and max_iters (hparams.py:141). */
typedef struct {
  int32_t num_symbols;             /* len(symbols), text/symbols.py:13 (80) */
  int32_t num_mels, num_freq;      /* hparams.py:16-17 */
  int32_t num_speakers;            /* train.py:301 / synthesizer.py:28 */
  int32_t model_type;              /* 0 single, 1 simple, 2 deepvoice      tacotron.py:51-94 */
  int32_t speaker_embedding_size;  /* hparams.py:35 */
  int32_t embedding_size;          /* hparams.py:37 */
  int32_t enc_prenet_n, enc_prenet[4];                                     /* hparams.py:40 */
  int32_t enc_bank_size, enc_bank_channels, enc_maxpool, enc_highway_depth, enc_rnn_size;
  int32_t enc_proj_n, enc_proj[4], enc_proj_width;                         /* hparams.py:41-47 */
  int32_t attention_type;          /* 0 bah, 1 bah_norm, 2 bah_mon         tacotron.py:132-146 */
  int32_t attention_size, attention_state_size;                            /* hparams.py:51-52 */
  int32_t dec_layer_num, dec_rnn_size;                                     /* hparams.py:55-56 */
  int32_t dec_prenet_n, dec_prenet[4];                                     /* hparams.py:59 */
  int32_t post_bank_size, post_bank_channels, post_maxpool, post_highway_depth, post_rnn_size;
  int32_t post_proj_n, post_proj[4], post_proj_width;                      /* hparams.py:60-66 */
  int32_t reduction_factor;        /* hparams.py:68 */
  int32_t max_iters;               /* hparams.py:141 */
} taco_hparams;

int taco_abi_version(void);
const char* taco_last_error(void); /* thread-local; valid until the next call on this thread */

/* ---- model life cycle: replaces create_model + tf.train.Saver.restore (models/__init__.py:6-7,
 *      synthesizer.py:46-67).  Weight names are the canonical names listed in DESIGN.md
 *      (one per TF variable of SURVEY App. B); tensors are HOST fp32 arrays in TF layout
 *      (dense kernel [in,out]; conv1d kernel [k,in,out]; GRU gates [in+n,2n] r|u, candidate [in+n,n]). */
int taco_model_create(const taco_hparams* hp, int device, taco_model** out);
int taco_model_set_weight(taco_model* m, const char* name, const float* host, const int64_t* shape, int ndim);
int taco_model_num_weights(const taco_model* m);                 /* how many tensors the hparams require */
int taco_model_weight_name(const taco_model* m, int i, char* buf, int buflen, int64_t* shape4, int* ndim);
int taco_model_finalize(taco_model* m); /* repack: MFMA fragment layouts, BN -> scale/shift, GRU [x;h] split */
void taco_model_destroy(taco_model* m);

/* ---- whole forward: replaces sess.run([linear_outputs, alignments]) at synthesizer.py:166-167
 *      over the graph of models/tacotron.py:29-239 (inference, is_training False).
 * Any B: more rows than one pass holds (64; 32 for an inference model with attention_size 512) run as passes of equal size over ONE
 * pass's workspace, with the passes' stop words carved behind it -- taco_workspace_bytes counts both.  The arguments are validated once,
 * before the batch is split: a null model or buffer, a bad shape, a missing speaker_id, a model not finalized and a workspace too small
 * get the same code and message at every B (a call of more than 64 rows with such an argument used to be answered "batch ... > 64 rows
 * per device is not supported" or "bad time ... / steps ..."). */
size_t taco_workspace_bytes(const taco_model* m, int B, int T_in, int n_steps);

int taco_forward_infer(taco_model* m, void* hip_stream,
                       const int32_t* d_inputs,          /* [B,T_in] ids, PAD=0 EOS=1   tacotron.py:38 */
                       const int32_t* d_input_lengths,   /* [B]                          synthesizer.py:120 */
                       const int32_t* d_speaker_id,      /* [B] or NULL (zeros)          synthesizer.py:43-44 */
                       int B, int T_in, int n_steps,     /* n_steps = max_iters          tacotron.py:210 */
                       const float* d_manual_alignments, /* NULL, or [B,n_steps,T_in]    rnn_wrappers.py:313-317 */
                       float* d_mel,                     /* [B,n_steps*r,num_mels]       tacotron.py:213-214 */
                       float* d_linear,                  /* [B,n_steps*r,num_freq]       tacotron.py:235 */
                       float* d_alignments,              /* [B,T_in,n_steps]             tacotron.py:238-239 */
                       int32_t* d_stop_step,             /* [1]: decoder steps the reference's stop rule
                                                            (helpers.py:29 + dynamic_decode) would have run;
                                                            == n_steps unless every row emitted an all-zero step.
                                                            NEGATIVE = -(device error word): a persistent kernel of
                                                            this forward (or of an earlier one whose error was never
                                                            acknowledged with taco_model_device_errors) gave up and
                                                            the outputs are invalid */
                       void* d_workspace, size_t workspace_bytes);

/* The same forward captured once into a hipGraph (all pointers baked in) and replayed. */
int taco_plan_create(taco_model* m, const int32_t* d_inputs, const int32_t* d_input_lengths,
                     const int32_t* d_speaker_id, int B, int T_in, int n_steps,
                     const float* d_manual_alignments, float* d_mel, float* d_linear,
                     float* d_alignments, int32_t* d_stop_step, void* d_workspace, size_t workspace_bytes,
                     taco_plan** out);
int taco_plan_launch(taco_plan* p, void* hip_stream);
int taco_plan_num_nodes(const taco_plan* p);
/* 1 if the plan contains a whole-chip persistent kernel (the decoder loop or a post-net scan on the persistent engine).  Such kernels need
 * every compute unit of the device at once; the library puts them -- eager launches and plan replays alike, from any stream or thread of
 * the process -- in a total order per device (a launch that follows one on another stream waits for an event recorded on that stream), so that
 * two of them never wait for each other's compute units.
 * Everything else of a forward still overlaps across streams.  Other processes on the same device are outside its reach. */
int taco_plan_whole_chip(const taco_plan* p);
void taco_plan_destroy(taco_plan* p);

/* ---- speaker mixtures: blending trained speakers at inference ----
 * The reference's Synthesizer.synthesize takes `speaker_ids` as a dict {speaker_id: weight} and forms weight * speaker_embed_table[
 * speaker_id] (synthesizer.py:153-164); that branch never ran there (an undefined `sess`, an argument-less np.tile()), but its intent
 * is plain and linear: the speaker vector of a row is a weighted sum of table rows.  The *_mix entry points are their namesakes with
 * `const float* d_speaker_weights` where `const int32_t* d_speaker_id` stands; every other argument, output and rule is the namesake's.
 * d_speaker_weights is float32 [B, num_speakers], row-major, on the device.  For row b, every table lookup the model would do with
 * speaker_id[b] (tacotron.py:41-94) is replaced by sum_s weights[b,s] * table[s,:]:
 *   speaker_embedding_size != 1       the one table `speaker_embedding` is mixed; 'deepvoice' feeds the mixed row to its five dense +
 *                                     softsign layers (tacotron.py:67-86), 'simple' concatenates it at the three places it goes today
 *                                     (rnn_wrappers.py:372-376,408-413; tacotron.py:226-233).
 *   'deepvoice', size == 1            (the get_embed tables, tacotron.py:52-66) each of the 3 + dec_layer_num tables `spk/<name>/table`
 *                                     is mixed with the same weights.
 * Weights are used as given: not normalised and not required to sum to 1 (the reference multiplies raw weights).  The sum is taken
 * in ascending s with one fmaf per term, starting from +0 (k_mix_rows): deterministic, and a one-hot row reproduces the looked-up row
 * -- and with it the whole forward -- exactly for finite tables (a table entry of -0 comes out as +0).  The added work is
 * B * D * num_speakers multiply-adds per table of width D, one small launch each; nothing else of the forward changes.
 * The buffer is read only by kernels: no host read, synchronisation or allocation, so the calls stay capturable.  A plan made by
 * taco_plan_create_mix reads its weights buffer on every replay: the caller changes voices between replays by writing the buffer.
 * More than 64 rows run as passes (as the namesakes do); the weights of the pass that starts at row b0 start at b0 * num_speakers.
 * TACO_ERR_ARG with a message, before any launch: null weights on a multi-speaker model; non-null weights on a single-speaker model
 * (they are not ignored).  taco_postnet_forward_mix reads the weights only for model_type 'simple', like its namesake its ids.
 * Training with mixtures is not offered: taco_train_* take ids. */
int taco_forward_infer_mix(taco_model* m, void* hip_stream, const int32_t* d_inputs, const int32_t* d_input_lengths,
                           const float* d_speaker_weights /* [B,num_speakers] */, int B, int T_in, int n_steps,
                           const float* d_manual_alignments, float* d_mel, float* d_linear, float* d_alignments,
                           int32_t* d_stop_step, void* d_workspace, size_t workspace_bytes);
int taco_plan_create_mix(taco_model* m, const int32_t* d_inputs, const int32_t* d_input_lengths,
                         const float* d_speaker_weights, int B, int T_in, int n_steps,
                         const float* d_manual_alignments, float* d_mel, float* d_linear,
                         float* d_alignments, int32_t* d_stop_step, void* d_workspace, size_t workspace_bytes,
                         taco_plan** out);
int taco_encoder_forward_mix(taco_model* m, void* hip_stream, const int32_t* d_inputs,
                             const int32_t* d_input_lengths, const float* d_speaker_weights, int B, int T_in,
                             float* d_encoder_out, void* d_workspace, size_t workspace_bytes);
int taco_decoder_forward_mix(taco_model* m, void* hip_stream, const float* d_encoder_out,
                             const float* d_speaker_weights, int B, int T_in, int n_steps,
                             const float* d_manual_alignments, const float* d_teacher_frames,
                             float* d_mel, float* d_alignments, int32_t* d_stop_step, float* d_dbg_states,
                             void* d_workspace, size_t workspace_bytes);
int taco_postnet_forward_mix(taco_model* m, void* hip_stream, const float* d_mel, const float* d_speaker_weights, int B, int T_mel,
                             float* d_linear, float* d_post_out, void* d_workspace, size_t workspace_bytes);

/* ---- stage-level entry points (parity tests, profiling) ----
 * Any B, validated once and served as passes like the whole forward (above); taco_decoder_forward combines the passes' stop words, and
 * refuses d_dbg_states with more than 64 rows (the dump is laid out [step][row]: one pass).  taco_stage_workspace_bytes(m, B, T) is
 * enough for each of the three at (B, T) -- the decoder with T_in = n_steps = T, with or without d_dbg_states, stop words included. */
/* embedding -> prenet -> encoder CBHG (tacotron.py:34-112).  d_encoder_out [B,T_in,2*enc_rnn_size]. */
int taco_encoder_forward(taco_model* m, void* hip_stream, const int32_t* d_inputs,
                         const int32_t* d_input_lengths, const int32_t* d_speaker_id, int B, int T_in,
                         float* d_encoder_out, void* d_workspace, size_t workspace_bytes);
/* attention memory + decoder loop (tacotron.py:120-214; rnn_wrappers.py:218-341,367-415; helpers.py).
 * d_teacher_frames NULL, or [B,n_steps,num_mels]: frame fed at step t>=1 is teacher[:,t-1]
 * (TacoTrainingHelper rule, helpers.py:44,66).  d_dbg_states NULL, or
 * [n_steps,B,attention_state_size + 2*enc_rnn_size + dec_layer_num*dec_rnn_size]: (h_att, ctx, h_1..h_L) after each step. */
int taco_decoder_forward(taco_model* m, void* hip_stream, const float* d_encoder_out,
                         const int32_t* d_speaker_id, int B, int T_in, int n_steps,
                         const float* d_manual_alignments, const float* d_teacher_frames,
                         float* d_mel, float* d_alignments, int32_t* d_stop_step, float* d_dbg_states,
                         void* d_workspace, size_t workspace_bytes);
/* post-net CBHG + linear head (tacotron.py:219-235).  d_mel [B,T_mel,num_mels] -> d_linear [B,T_mel,num_freq];
 * d_post_out optional [B,T_mel,2*post_rnn_size]; d_speaker_id is read only by model_type 'simple' (:226-233). */
int taco_postnet_forward(taco_model* m, void* hip_stream, const float* d_mel, const int32_t* d_speaker_id, int B, int T_mel,
                         float* d_linear, float* d_post_out, void* d_workspace, size_t workspace_bytes);
size_t taco_stage_workspace_bytes(const taco_model* m, int B, int T);

/* ---- op-level entry points, addressed by layer name inside the model ---- */
/* modules.py:123-131 conv1d -> act -> batch_norm (inference).  act: 0 none, 1 relu.
 * maxpool_width > 1 applies max_pooling1d(width, stride 1, 'same') (modules.py:47-51) to x first. */
int taco_conv1d_bn_f32(taco_model* m, void* hip_stream, const char* layer, const float* d_x, int B, int T,
                       int act, int maxpool_width, float* d_out);
/* tf.layers.dense on [rows, in] (A.1).  act: 0 none, 1 relu, 2 sigmoid, 3 tanh. */
int taco_dense_f32(taco_model* m, void* hip_stream, const char* layer, const float* d_x, int rows, int act,
                   float* d_out);
/* modules.py:105-120 on [rows, D]. */
int taco_highway_f32(taco_model* m, void* hip_stream, const char* layer, const float* d_x, int rows,
                     float* d_out);
/* modules.py:82-96 BiGRU; scope "encoder_cbhg" or "post_cbhg".  d_lengths / d_init_state ([B,2H]) nullable. */
int taco_bigru_f32(taco_model* m, void* hip_stream, const char* scope, const float* d_x,
                   const int32_t* d_lengths, const float* d_init_state, int B, int T, float* d_out,
                   void* d_workspace, size_t workspace_bytes);
/* one attention evaluation (rnn_wrappers.py:304-341 + TF-sem score/normaliser):
 * query = d_cell_output . W_q; alignments from keys/prev; context = alignments . values. */
int taco_attention_step_f32(taco_model* m, void* hip_stream, const float* d_cell_output, const float* d_keys,
                            const float* d_values, const float* d_prev_alignments, int B, int T_in,
                            float* d_alignments, float* d_context, void* d_workspace, size_t workspace_bytes);

/* one tf.contrib.rnn.GRUCell step (A.6) of a decoder GRU by name ("decoder/attention_gru",
 * "decoder/gru_1", ...; tacotron.py:127-130,171-172).  d_h [R,H] is updated in place; d_out_res
 * (nullable) = h' + x (ResidualWrapper).  Workspace: 3*R*H floats. */
int taco_gru_cell_f32(taco_model* m, void* hip_stream, const char* name, const float* d_x, float* d_h, int R,
                      float* d_out_res, void* d_workspace, size_t workspace_bytes);

/* attention-based end-of-speech trimming (synthesizer.py:242-262, attention_trim && end_of_sentence): per batch row the number of
 * spectrogram frames to keep, reduction_factor * j + 3, from the argmax walk over d_alignments [B, T_in, n_steps];
 * d_seq_len[b] = len(sequence) of the row (tokens incl. EOS and padding, as the reference passes it).  d_spec_end [B]. */
int taco_attention_trim(void* hip_stream, const float* d_alignments, const int32_t* d_seq_len, int B, int T_in, int n_steps,
                        int reduction_factor, int32_t* d_spec_end);
/* the alignments of the second pass of the reference's two-pass synthesis (synthesizer.py:171-205, manual_attention_mode 1 and 3), built
 * from the first pass's d_alignments [B, T_in, n_steps] as the forward writes them into d_manual [B, n_steps, T_in], the layout the
 * forward's d_manual_alignments takes.  Per batch row and ENCODER position e, d* = argmax over the DECODER steps of d_alignments[b, e, :]
 * (the reference's axis: alignments[idx].argmax(1)): the first index of the maximum wins, a NaN counts as the maximum and the first NaN
 * wins (NumPy's rule), +0 and -0 compare equal.  d_manual[b, d, e] = 1 where d == d*; elsewhere +0 (mode 1, "argmax one hot") or the
 * bits of d_alignments[b, e, d] (mode 3, "prunning").  Padding positions e >= input_length get their one too, as in the reference; a
 * decoder step may end up with no one or with several.  One launch that writes every element of d_manual exactly once: no memset,
 * no atomics, deterministic; n_steps and T_in are not bounded by the kernel.
 * Checked before any HIP call: a null pointer, B, T_in or n_steps < 1, overlapping byte ranges of the two buffers, a mode other than
 * 1, 2, 3 -> TACO_ERR_ARG; mode 2 -> TACO_ERR_UNSUPPORTED: the reference calls np.pow there, which does not exist (synthesizer.py:181-188),
 * so mode 2 is refused rather than guessed at. */
int taco_manual_alignments(void* hip_stream, const float* d_alignments, int B, int T_in, int n_steps, int mode, float* d_manual);
/* ---- rate, per-token duration and pitch control on the spectrogram, between the attention trim and a vocoder.  NOT in the reference: its
 * synthesizer says a sentence at the speed and pitch the model chose.  The forward produces a MAGNITUDE spectrogram and Griffin-Lim
 * invents the phase afterwards, so speed is a resampling of the frame axis and pitch a resampling of the bin axis; the alignments
 * attribute every decoder step to an input token, so the stretch can differ per token.  tests/warp_reference.py restates both calls in
 * NumPy, the map in int64 exactly as below. ----
 * taco_spec_warp_map: the integer time map of every batch row, one launch (k_warp_map, csrc/taco_warp.h).  Inputs: d_alignments
 * [B, T_in, n_steps] (nullable); d_frames [B] (nullable: T) -- taco_attention_trim's d_spec_end as it stands; d_row_stretch [B] fp32
 * (nullable: 1); d_token_stretch [B, T_in] fp32 (nullable: 1; needs d_alignments); T = n_steps * reduction_factor source frames; T_out
 * = the capacity of the outputs.  For row b:
 *   f = clamp(d_frames[b], 1, T).
 *   tok(s) = argmax over e in [0, T_in) of d_alignments[b, e, s] for decoder step s: the first maximum wins, a NaN counts as the maximum
 *   and the first NaN wins (the rule of taco_manual_alignments, on the other axis).  Source frame t < f belongs to step t / r.
 *   Its duration is an integer in units of 2^-16 output frame:
 *     d_t = clamp(lrint(fp32(row_stretch[b] * token_stretch[b, tok(t / r)]) * 65536), 2^12, 2^20)
 *   -- one correctly rounded fp32 product, then an exact scaling; a NaN or a non-positive product gives 2^12.
 *   C_t = the inclusive prefix sum of d_t in int64, C_-1 = 0 (integer sums are associative: any scan shape gives the same bits).
 *   d_out_frames[b] = clamp((C_{f-1} + 2^15) >> 16, 1, T_out).
 *   For output frame j < d_out_frames[b], tau = j << 16: d_src[b, j] = the t with C_{t-1} <= tau < C_t (tau < C_{f-1} always holds there),
 *   d_frac[b, j] = ((tau - C_{src-1}) << 16) / d_src, an integer division, in [0, 65536).  For j >= d_out_frames[b]: src = f - 1, frac = 0.
 *   d_token_frames [B, T_in] int32 (nullable; needs d_alignments): the number of source frames t < f attributed to each token -- the
 *   model's own durations, which a caller needs before asking for different ones.  Every element is written exactly once per call.
 * d_src, d_frac [B, T_out] int32, d_out_frames [B].  d_workspace: taco_spec_warp_workspace_bytes(B, T), 8-byte aligned; it holds C, so T
 * is not bounded by the kernel.
 * taco_spec_warp: the gather and the interpolation, one launch (k_spec_warp): d_spec [B, T, W] fp32 with any W >= 1 (num_freq for the
 * linear outputs, num_mels for the mel outputs), the map above, d_frames, d_freq_scale [B] fp32 (nullable) -> d_out [B, T_out, W].  Per
 * output element, THE TIME INTERPOLATION FIRST, THEN THE FREQUENCY INTERPOLATION, every operation an fp32 operation rounded on its own:
 *   t0 = src, t1 = min(t0 + 1, f - 1), w_t = frac * 2^-16 (exact in fp32);
 *   v(k) = x[t0, k] when frac == 0 (the bits are copied; a NaN next door never leaks), else x[t0, k] + w_t * (x[t1, k] - x[t0, k]);
 *   v(k) = +0 for k >= W: normalised 0 is the floor level, and content scaled past Nyquist is gone.
 *   Without a frequency scale out[j, k] = v(k).  With c = d_freq_scale[b]: q = fp32(k * c), k0 = (int)q, w_f = q - k0; out = v(k0) if
 *   w_f == 0, otherwise v(k0) + w_f * (v(k0 + 1) - v(k0)).  (c = 2^(-p / 12) raises the pitch by p semitones.  A q outside [0, W) --
 *   a NaN or a negative c among them -- gives +0.)
 *   Rows j >= d_out_frames[b] are written as +0.  Every element of d_out is written exactly once; nothing at frames >= f of the input is
 *   ever read (src is clamped to [0, f - 1] and frac to [0, 65535] on the device: a garbage map gives a wrong picture, nothing worse).
 * The bin-axis scale moves the formants with the pitch, as a resampling-based shift does; taco_spec_warp_formant below moves the two apart.
 * NOT reproduced / out of scope: waveform-domain stretching of recordings.
 * Both calls launch on hip_stream only: no read-back, allocation, memset or synchronisation; safe under stream capture; no atomics, two
 * calls give the same bits.  Checked before any HIP call: a null required pointer (d_src, d_frac, d_out_frames, d_workspace; d_spec,
 * d_out); B, T, T_out, reduction_factor or W < 1, and T_in or n_steps < 1 when d_alignments is given; T != n_steps * reduction_factor
 * when d_alignments is given; d_token_stretch or d_token_frames without d_alignments; a misaligned workspace; an output that shares a byte
 * with an input, the workspace or another output -> TACO_ERR_ARG; a workspace that is too small -> TACO_ERR_STATE; W >= 2^24 ->
 * TACO_ERR_UNSUPPORTED. */
size_t taco_spec_warp_workspace_bytes(int B, int T);
int taco_spec_warp_map(void* hip_stream, const float* d_alignments, const int32_t* d_frames, const float* d_row_stretch,
                       const float* d_token_stretch, int B, int T_in, int n_steps, int reduction_factor, int T, int T_out,
                       int32_t* d_src, int32_t* d_frac, int32_t* d_out_frames, int32_t* d_token_frames,
                       void* d_workspace, size_t workspace_bytes);
int taco_spec_warp(void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src, const int32_t* d_frac,
                   const int32_t* d_out_frames, const float* d_freq_scale, int B, int T, int W, int T_out, float* d_out);
/* ---- the spectral envelope of a frame, and pitch and formant shifted apart (k_spec_envelope, k_spec_warp_formant, csrc/taco_envelope.h).
 * NOT in the reference.  The linear output is normalised dB, affine in log|D|, so the real cepstrum of a frame is a cosine transform of the
 * frame itself and its low-quefrency part is the envelope -- the vocal tract, the formants -- while the rest, the excitation, carries the
 * harmonics.  Scaling the two along the bin axis by different factors changes the pitch and keeps the voice, or the other way round.
 * tests/envelope_reference.py restates everything below in NumPy, in float64 and in fp32. ----
 * Let W >= 3 be the bins of a frame, M = W - 1, and Q the number of cepstral coefficients kept, 1 <= Q <= min(W - 1, 128).
 * taco_envelope_create: host_basis [Q, W] doubles, basis[n, k] = cos(pi * n * k / M), and host_lifter [Q] doubles (NULL: all ones), both from
 * the caller: no libm call of this library decides a bit (as in taco_resample_create, taco_gl_set_mel_basis).  The library forms two fp32
 * tables on the host in double, in exactly this order, and rounds once:
 *   A[n, k] = fp32((w_k * basis[n, k]) / M),  w_0 = w_M = 0.5 and every other w_k = 1;
 *   S[n, k] = fp32((a_n * l[n]) * basis[n, k]),  a_0 = 1 and every other a_n = 2
 * -- the DCT-I pair of the even extension of length 2 M: c below is the real cepstrum of the frame, and with Q = W and the last a halved S
 * would give the frame back.  taco_envelope_tables copies both out, [Q, W] each; taco_envelope_width / _order return W / Q (0 for NULL).
 * For a frame v[0 .. W):  c_n = sum over k of A[n, k] * v_k;  env_k = sum over n of S[n, k] * c_n  -- fp32 products and fp32 sums, the order
 * of a sum is the kernel's;  e_k = v_k - env_k, one fp32 subtraction.
 * taco_spec_envelope: d_spec [B, T, W] -> d_env [B, T, W] and, when d_cep is given, d_cep [B, T, Q], for every frame t < f_b =
 * clamp(d_frames[b], 1, T) (d_frames NULL: T).  Frames t >= f_b are written as +0 in both and are never read.
 * taco_spec_warp_formant: the inputs of taco_spec_warp with d_pitch_scale [B] and d_formant_scale [B] (both nullable) in place of
 * d_freq_scale -> d_out [B, T_out, W].  For output frame j < d_out_frames[b]:
 *   1. v(k) is the time interpolation of taco_spec_warp, to the bit, the frac == 0 copy included;
 *   2. c, env and e are formed from v as above;
 *   3. out[j, k] = G(env, formant_scale[b])[k] + G(e, pitch_scale[b])[k], one fp32 addition, where G(y, s) is the frequency gather of
 *      taco_spec_warp applied to y: q = fp32(k * s), k0 = (int)q, w_f = q - k0; y(k0) when w_f == 0, otherwise y(k0) + w_f * (y(k0 + 1) - y(k0));
 *      y(k >= W) = +0; a q outside [0, W) gives +0.  A NULL scale means y[k] itself.
 *   Rows j >= d_out_frames[b] are +0.  Every element of d_out is written exactly once; nothing at frames >= f of the input is read.
 * A NaN in a source frame makes the cepstrum of every output frame that reads it NaN, and with it every bin G reads there; no other
 * output frame is affected.  Equal scales give taco_spec_warp(freq_scale) up to rounding (G is linear); a lifter of zeros gives env = +0
 * and taco_spec_warp on the bits for inputs without -0 and without values that are not finite.
 * taco_envelope_create needs no device: the first taco_spec_envelope / taco_spec_warp_formant on the handle uploads the tables.  That
 * call allocates, so it must be made outside stream capture.  After it both calls are one launch on hip_stream: no workspace, read-back,
 * memset, atomics or synchronisation; capturable; two calls give the same bits.  The handle's `device` is made current.
 * Checked before any HIP call, TACO_ERR_ARG: a null required pointer (host_basis, out; e, d_spec, d_env; d_src, d_frac, d_out_frames,
 * d_out); W < 3, Q < 1 or Q > W - 1; a basis or lifter entry that is not finite, a basis entry above 1 in magnitude; B, T or T_out < 1; an
 * output that shares a byte with an input or with the other output.  TACO_ERR_UNSUPPORTED: Q > 128, or W > 2304 -- one workgroup keeps v
 * and env of its frames in LDS, 16 frames up to W = 1152 and 8 beyond. */
typedef struct taco_envelope taco_envelope;
int taco_envelope_create(int W, int Q, const double* host_basis /* [Q, W] */, const double* host_lifter /* [Q], nullable */, int device,
                         taco_envelope** out);
void taco_envelope_destroy(taco_envelope* e);
int taco_envelope_width(const taco_envelope* e);
int taco_envelope_order(const taco_envelope* e);
int taco_envelope_tables(const taco_envelope* e, float* host_A /* [Q, W] */, float* host_S /* [Q, W] */);
int taco_spec_envelope(taco_envelope* e, void* hip_stream, const float* d_spec, const int32_t* d_frames /* nullable */, int B, int T,
                       float* d_env, float* d_cep /* nullable */);
int taco_spec_warp_formant(taco_envelope* e, void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src,
                           const int32_t* d_frac, const int32_t* d_out_frames, const float* d_pitch_scale, const float* d_formant_scale,
                           int B, int T, int T_out, float* d_out);
/* The stop rule (helpers.py:29 + dynamic_decode: the loop ends after the first step at which every row has emitted an all-zero
 * step) evaluated on a finished mel buffer d_mel [B, n_steps, width = r*num_mels] per group of rows_per_group consecutive rows:
 * d_stop[B / rows_per_group].  For requests that were served together through one plan (PlanPool coalesce > 1), whose plan-wide
 * stop step covers all of them; with rows_per_group = B it equals the stop step the forward itself reports. */
int taco_stop_steps(void* hip_stream, const float* d_mel, int B, int n_steps, int width, int rows_per_group, int32_t* d_stop);

/* ---- spectrogram -> waveform (audio/__init__.py:54-56,76-96,118-122,149-165; synthesizer.py:264) ---- */
typedef struct {
  int32_t num_freq, sample_rate, griffin_lim_iters;
  float frame_length_ms, frame_shift_ms, preemphasis, min_level_db, ref_level_db, power;
} taco_audio_hparams;                       /* hparams.py:16-23,144-145 */
typedef struct taco_gl taco_gl;
int taco_gl_create(const taco_audio_hparams* hp, int device, taco_gl** out);
void taco_gl_destroy(taco_gl* g);
int taco_gl_num_samples(const taco_gl* g, int T);            /* hop_length * (T - 1), librosa istft with center=True */
size_t taco_gl_workspace_bytes(const taco_gl* g, int B, int T);
/* inv_spectrogram of B utterances: d_spec [B, T, num_freq] in the model's linear_outputs layout (the reference transposes to
 * [num_freq, T] first).  d_init_uniform [B, T, num_freq] in [0,1) plays np.random.rand of _griffin_lim (NULL: counter-based
 * hash of `seed`).  iters < 0: griffin_lim_iters.  d_wav [B, taco_gl_num_samples(T)].  Needs hop*(T-1) > n_fft/2. */
int taco_gl_inv_spectrogram(taco_gl* g, void* hip_stream, const float* d_spec, const float* d_init_uniform,
                            unsigned long long seed, int B, int T, int iters, float* d_wav, void* d_workspace, size_t workspace_bytes);
/* The same per utterance length, as synthesizer.py:242-264 does it (`wav = wav[:spec_end_idx]; inv_spectrogram(wav.T)`): row b of d_wav
 * [B, taco_gl_num_samples(T)] holds inv_spectrogram(spec[b, :f_b]) in its first hop*(f_b-1) samples and exact zeros after; frames
 * t >= f_b have magnitude 0, take no part in the row's window sum-square, and every iteration's reflect padding is taken at the
 * row's own ends.  d_frames [B] is device memory (NULL: every row keeps T) -- taco_attention_trim's d_spec_end as it stands -- and
 * is only read on the device: no read-back, synchronisation or allocation, capturable.  Each value is clamped on the device to
 * [taco_gl_min_frames, T], and d_num_samples [B] (nullable) receives hop*(f_b-1) for the clamped value.  NOT reproduced: the
 * reference's trim can return 3 frames, which librosa serves by reflecting more than once; such a row is synthesised from
 * taco_gl_min_frames frames here.  d_init_uniform[b, t, :] is used for t < f_b; with NULL the hash is indexed as in
 * taco_gl_inv_spectrogram, so a row that keeps T frames gets that entry point's phases (and its output, bit for bit).
 * T < taco_gl_min_frames: TACO_ERR_SHAPE.  Workspace: taco_gl_rows_workspace_bytes. */
int taco_gl_min_frames(const taco_gl* g);                    /* smallest T with hop*(T-1) > n_fft/2: n_fft/2/hop + 2 */
size_t taco_gl_rows_workspace_bytes(const taco_gl* g, int B, int T);
int taco_gl_inv_spectrogram_rows(taco_gl* g, void* hip_stream, const float* d_spec, const int32_t* d_frames, const float* d_init_uniform,
                                 unsigned long long seed, int B, int T, int iters, float* d_wav, int32_t* d_num_samples, void* d_workspace,
                                 size_t workspace_bytes);
/* save_audio's scaling to 16-bit PCM (audio/__init__.py:23-24) per row of d_wav [B, L]: peak = max|x| over the first d_num_samples[b]
 * samples (NULL: L), pcm = (int16) trunc(x * (32767 / max(0.01, peak))), zeros past them.  d_pcm [B, L].  One launch. */
int taco_wav_to_pcm16(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, int16_t* d_pcm);

/* ---- the reference's two other vocoders ---- */
/* inv_spectrogram_tensorflow (audio/__init__.py:59-61,87-96,109-116,152-153,167-168), the Griffin-Lim the reference builds into its
 * inference graph as Synthesizer.wav_output (synthesizer.py:53-54).  UNPINNED on TensorFlow: the reference runs tf.contrib.signal.stft /
 * inverse_stft of TF 1.x, this project does not depend on TensorFlow, and what follows restates their documented algorithm; it could
 * not be checked against TensorFlow's source or output.  With N = n_fft, W = win_length, h = hop and w[n] = 0.5 - 0.5 cos(2 pi n / W):
 *   stft(y), pad_end=False   frame t = y[t*h .. t*h + W) for t = 0 .. (len - W) / h, times w, zero-padded AT THE END to N, rfft:
 *                            X_k = sum_n y[t*h + n] w[n] e^{-2 pi i k n / N} -- the window is left-aligned, where librosa centres it
 *   inverse_stft(X)          irfft(X, N)[:W] * w, overlap-added at stride h: no window sum-square division (tf's default
 *                            window_fn is used as the reference passes none other), no reflect padding; h*(T-1) + W samples
 *   inv_spectrogram_tensorflow(spec)   S = (10^((clip(spec,0,1) * -min_db + min_db + ref_db) / 20))^power; y = inverse_stft(S + 0i)
 *                            (zero phase, not np.random.rand); griffin_lim_iters times est = stft(y), y = inverse_stft(S * est /
 *                            max(1e-8, |est|)) -- a bin whose estimate is 0 gives 0; no inverse pre-emphasis.
 * Deterministic: the same spectrogram gives the same samples, bit for bit.  A handle of taco_gl_create_tf carries this flavour's two
 * DFT packs and serves taco_gl_inv_spectrogram_tf (and taco_gl_set_inv_mel_basis / taco_gl_mel_to_linear, taco_wav_*) only: the
 * librosa-flavour entry points (taco_gl_inv_spectrogram*, taco_gl_inv_melspectrogram_rows, taco_spec_targets) return TACO_ERR_STATE
 * on it, and taco_gl_inv_spectrogram_tf returns TACO_ERR_STATE on a handle of taco_gl_create.
 * d_spec [B, T, num_freq], T >= 1.  d_frames [B] device memory (NULL: every row keeps T), clamped on the device to [1, T] and never
 * read on the host; row b of d_wav [B, taco_gl_tf_num_samples(T)] is the vocoding of spec[b, :f_b] -- frames t < f_b touch only
 * samples those frames produce -- in its first h*(f_b-1) + W samples and exact zeros after; d_num_samples [B] (nullable) receives
 * that count.  iters < 0: griffin_lim_iters.  No read-back, synchronisation or allocation: capturable. */
int taco_gl_create_tf(const taco_audio_hparams* hp, int device, taco_gl** out);
int taco_gl_tf_num_samples(const taco_gl* g, int T);         /* hop_length * (T - 1) + win_length */
size_t taco_gl_tf_workspace_bytes(const taco_gl* g, int B, int T);
int taco_gl_inv_spectrogram_tf(taco_gl* g, void* hip_stream, const float* d_spec, const int32_t* d_frames, int B, int T, int iters,
                               float* d_wav, int32_t* d_num_samples, void* d_workspace, size_t workspace_bytes);
/* inv_melspectrogram (audio/__init__.py:70-72,136-140): S = max(1e-10, inv_mel_basis . 10^((clip(mel,0,1) * -min_db + min_db) / 20))
 * (no ref_level_db: melspectrogram never subtracts it), then ^power, Griffin-Lim and inverse pre-emphasis as inv_spectrogram.
 * host_inv [num_freq, num_mels] is the pseudo-inverse of the filter bank, computed on the host (np.linalg.pinv in float64,
 * audio.inv_mel_basis; fp32 here) -- UNPINNED on librosa as far as the filter bank is (taco_gl_set_mel_basis).  Works on a handle of
 * either flavour.  The product is a fixed-order fp32 sum over the mels, m = 0 .. num_mels-1 with fmaf (k_gl_mel_magnitude), not the
 * split-bf16 product: the pseudo-inverse has entries of both signs and the sum cancels.
 * taco_gl_mel_to_linear: d_mel [B, T, num_mels] -> d_out [B, T, num_freq] = _mel_to_linear(_db_to_amp(_denormalize(mel))), before ^power.
 * taco_gl_inv_melspectrogram_rows: taco_gl_inv_spectrogram_rows with those magnitudes^power in place of the linear ones; every other
 * argument, the clamp of d_frames, the outputs and the workspace (taco_gl_rows_workspace_bytes) are that entry point's.
 * Both return TACO_ERR_STATE until taco_gl_set_inv_mel_basis was called. */
int taco_gl_set_inv_mel_basis(taco_gl* g, const float* host_inv, int num_mels);
int taco_gl_mel_to_linear(taco_gl* g, void* hip_stream, const float* d_mel, int B, int T, float* d_out);
int taco_gl_inv_melspectrogram_rows(taco_gl* g, void* hip_stream, const float* d_mel, const int32_t* d_frames, const float* d_init_uniform,
                                    unsigned long long seed, int B, int T, int iters, float* d_wav, int32_t* d_num_samples,
                                    void* d_workspace, size_t workspace_bytes);

/* ---- Fast Griffin-Lim (Perraudin, Balazs, Sondergaard 2013): momentum in the loop of all three vocoders ----
 * With momentum a and c = a / (1 + a) every iteration projects z = t - c * t_prev in place of t = stft(y), t_prev the estimate of the
 * iteration before (the first iteration: z = t): librosa.griffinlim's loop (0.7 and later) with the reference's own normalisation --
 * S * exp(i angle(z)), angle(0) = 0, for inv_spectrogram and inv_melspectrogram, S * z / max(1e-8, |z|) for inv_spectrogram_tensorflow --
 * in place of librosa's z / (|z| + 1e-16).  Not in the reference: momentum 0, the default, is the reference's loop, bit for bit and
 * launch for launch.  The momentum is host state of the handle, read when a call is issued: a captured graph keeps the value it was
 * captured with.  A non-zero momentum adds one [rows, 2*num_freq] estimate buffer to the loop's workspace, so taco_gl_workspace_bytes,
 * taco_gl_rows_workspace_bytes and taco_gl_tf_workspace_bytes READ THE HANDLE: query them again after taco_gl_set_momentum.
 * taco_gl_set_momentum: finite and 0 <= momentum <= 1, else TACO_ERR_ARG.  taco_gl_momentum: the value in use, 0 for NULL. */
int taco_gl_set_momentum(taco_gl* g, float momentum);
float taco_gl_momentum(const taco_gl* g);
/* Spectral convergence sc[b] = || |stft(y_b)| - S_b || / || S_b || of B waveforms against the magnitudes they were synthesised
 * from, over utterance b's own frames t < f_b and all num_freq bins; 0 where S_b is all zero.  d_wav [B, taco_gl_num_samples(T)] is
 * the output rectangle of taco_gl_inv_spectrogram(_rows) / taco_gl_inv_melspectrogram_rows at any momentum and iteration count:
 * the analysis is that of taco_spec_targets (pre-emphasis, which undoes the vocoder's inverse pre-emphasis; reflect padding at each
 * row's own ends; row b has hop*(f_b - 1) samples), followed by a two-stage sum in one fixed order, without atomics: two calls and a
 * captured replay give the same bits.  d_frames [B] is device memory (NULL: every row keeps T), clamped on the device to
 * [taco_gl_min_frames, T] as the vocoder clamps it.  The target is formed on the fly from d_target [B, T, num_freq]:
 *   target_kind 0   a normalised linear spectrogram, as the vocoder takes it: S = (10^((clip(x,0,1) * -min_db + min_db + ref_db) / 20))^power
 *                   by the very function the vocoder fills its own target with
 *   target_kind 1   the magnitudes themselves (for the mel vocoder: taco_gl_mel_to_linear's output raised to `power`)
 * librosa-flavour handles only (a handle of taco_gl_create_tf: TACO_ERR_STATE).  NULL pointers, B outside [1, 65535], T < 2, another
 * target_kind -> TACO_ERR_ARG; T < taco_gl_min_frames -> TACO_ERR_SHAPE; a workspace below taco_gl_convergence_workspace_bytes ->
 * TACO_ERR_STATE; all of them before any HIP call.  No allocation, no synchronisation: capturable. */
size_t taco_gl_convergence_workspace_bytes(const taco_gl* g, int B, int T);
int taco_gl_convergence(taco_gl* g, void* hip_stream, const float* d_target, int target_kind, const int32_t* d_frames, const float* d_wav,
                        int B, int T, float* d_sc, void* d_workspace, size_t workspace_bytes);

/* Silence trimming of a synthesised waveform: the `librosa.effects.trim(audio_out, frame_length=5120, hop_length=256, top_db=50)` of
 * synthesizer.py:266-269 (`audio_out = audio_out[:index[-1]]`), per row of d_wav [B, L].  UNPINNED on librosa: the reference pins
 * librosa==0.5.1, this project does not depend on librosa, and what follows restates the documented algorithm; it could not be
 * checked against librosa's source or output.  With N = frame_length, frame t of a row of n samples is N samples of
 * np.pad(y, N/2, mode="reflect") from t*hop_length (a row shorter than N/2 is reflected more than once, as np.pad does: every
 * n >= 2 is reproduced); the row has 1 + n / hop_length frames.  Two conventions for a frame's energy:
 *   TACO_TRIM_SPECTRAL  librosa 0.5.x, the reference's pin: rmse goes through the magnitude spectrogram, mse = mean over the N/2 + 1
 *                       one-sided bins of |rfft(hann_periodic * frame)|^2 (DC and Nyquist at full weight; NOT the time-domain mean
 *                       square).  Computed without a transform as (N sum xw^2 + (sum xw)^2 + (sum (-1)^i xw)^2) / 2 / (N/2 + 1).
 *   TACO_TRIM_TIME      librosa >= 0.6: mse = mean of the squares of the unwindowed frame.
 * Then db = 10 log10(max(1e-10, mse)) - 10 log10(max(1e-10, max_t mse)), a frame is non-silent where db > -top_db, and
 * d_index[b] = {start, end} = {first*hop_length, min(n, (last + 1)*hop_length)}, {0, 0} when no frame is non-silent.  The reference
 * cuts the tail only (`[:end]`); start is reported, not applied.  d_num_samples [B] is device memory, only read on the device
 * (NULL: every row has L samples); each count is clamped to [0, L] and nothing at or past it is read; a row with n < 2 returns
 * {0, n}.  d_frame_db [B, 1 + L/hop_length] (nullable; for diagnostics and tests) receives db for the row's own frames and exact
 * zeros after.  Asynchronous on the stream, two launches; no allocation, read-back or synchronisation: capturable.  Two calls on the
 * same input return the same bits.  TACO_ERR_ARG (before any device call): hop_length < 1, frame_length < 2, unknown energy, a null
 * pointer, workspace below taco_wav_trim_workspace_bytes.  TACO_ERR_UNSUPPORTED: an odd frame_length, or one whose frame (and
 * window) does not fit 64 KB of LDS (8192 spectral, 16384 time-domain). */
#define TACO_TRIM_SPECTRAL 0   /* librosa 0.5.x: one-sided mean of |stft|^2, Hann window (the reference's pin) */
#define TACO_TRIM_TIME     1   /* librosa >= 0.6: mean square of the unwindowed frame */
size_t taco_wav_trim_workspace_bytes(int B, int L, int frame_length, int hop_length);
int taco_wav_trim(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, float top_db, int frame_length,
                  int hop_length, int energy, int32_t* d_index, float* d_frame_db, void* d_workspace, size_t workspace_bytes);

/* Splitting a recording on silence: the `librosa.effects.split(audio, top_db=40, frame_length=1024, hop_length=256)` of
 * audio/silence.py:44-45,53-54 and the `remove_breath` of audio/silence.py:21-31 (a second split at frame_length=128, hop_length=32
 * and a mute of the quiet sub-intervals).  UNPINNED on librosa, exactly as the trim above: what follows restates the documented
 * algorithm and could not be checked against librosa's source or output.
 * taco_wav_split, per row of d_wav [B, L]: frames, energies (both conventions), db and `non_silent = db > -top_db` are the trim's,
 * computed by the same first launch.  Then, as librosa.effects.split does: edges = flatnonzero(diff(non_silent)) + 1, a 0 prepended if
 * frame 0 is non-silent, len(non_silent) appended if the last frame is, frames_to_samples (times hop_length), minimum(edges, n),
 * reshape(-1, 2) -- the maximal runs of non-silent frames in order, run r = {s*hop_length, min(n, e*hop_length)} with s its first
 * frame and e one past its last.  d_counts[b] always receives the true number of runs; d_intervals [B, max_intervals, 2] receives the
 * first max_intervals of them and exact zeros in every other word ((Fmax + 1) / 2 runs is the most Fmax = 1 + L/hop_length frames
 * can hold).  A row with n < 2 has no frames: count 0.  An interval may be empty, {n, n}, when n % hop_length == 0 and only the last
 * frame is non-silent; it is reported like any other.  The identity that ties the split to the trim: on the same input and
 * parameters, intervals[b, 0, 0] and intervals[b, count - 1, 1] equal the trim's d_index[b] for every row with n >= 2 (and count 0
 * where the trim returns {0, 0}).  d_num_samples, d_frame_db, the energy conventions, their LDS limits and TACO_ERR_UNSUPPORTED
 * cases are the trim's.  Asynchronous on the stream, two launches; no allocation, read-back or synchronisation: capturable.  The order
 * of the runs comes from a prefix count, not from atomics: two calls on the same input return the same bits.
 * taco_wav_breath_mute, per row of d_wav [S, L] with that row's interval table and count (a split of the same rectangle): interval k
 * is muted iff abs_mean(audio[start:end]) < abs_mean(audio) - threshold (0.05 in the reference), abs_mean = mean |x|, and because
 * the reference mutes in place, abs_mean(audio) is re-evaluated after every mute.  Restated: total = sum |x| over the row's n
 * samples; walking the intervals in order, k is muted iff len_k > 0 and sum_k/len_k < total/n - threshold, and a muted interval's sum
 * is then subtracted from total.  An empty interval is never muted (NumPy's mean of nothing is NaN; the comparison is false).  d_out
 * [S, L] receives the row with the muted intervals as exact zeros, every other sample bit for bit, zeros at and past n; it may be
 * d_wav itself.  Nothing at or past n is read.  Of a row whose count exceeds max_intervals only the first max_intervals intervals
 * are considered.  d_muted [S, max_intervals] (nullable) receives the flags; d_abs_mean [S, 1 + max_intervals] (nullable) total/n
 * before any mute (0 for an empty row), then every interval's mean (NaN for an empty one); entries past a row's count are zero.
 * One launch, capturable; every sum has one order, two calls return the same bits.
 * TACO_ERR_ARG (before any device call): a null required pointer, B, S or L < 1, hop_length < 1, frame_length < 2, max_intervals < 1,
 * unknown energy, workspace below taco_wav_split_workspace_bytes. */
size_t taco_wav_split_workspace_bytes(int B, int L, int frame_length, int hop_length);
int taco_wav_split(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, float top_db,
                   int frame_length, int hop_length, int energy, int max_intervals,
                   int32_t* d_intervals /* [B, max_intervals, 2] */, int32_t* d_counts /* [B] */,
                   float* d_frame_db /* nullable */, void* d_workspace, size_t workspace_bytes);
int taco_wav_breath_mute(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int S, int L,
                         const int32_t* d_intervals, const int32_t* d_counts, int max_intervals, float threshold,
                         float* d_out, int32_t* d_muted /* nullable */, float* d_abs_mean /* nullable */);

/* Splitting and levelling 16-bit PCM on silence, the pydub way: `pydub.silence.detect_nonsilent` as split_on_silence_with_pydub
 * (audio/silence.py:81-117, the method the reference's README and scripts/prepare_*.sh run: min_silence_len=100, silence_thresh=-40)
 * and amplify (app.py:27-53: silence_thresh=-50, min_silence_len=300, every non-silent stretch brought to -20 dBFS) call it.
 * UNPINNED on pydub: the reference pins pydub==0.20.0, this project does not depend on pydub, and what follows restates pydub's
 * published silence.py with seek_step = 1; it could not be checked against pydub's source or output, only against the standard
 * library's audioop, which pydub calls (tests/pydub_reference.py).  Where the 0.20.0 pin may differ, the rule taken: (1) a window is
 * silent when rms <= thresh, not <: the two part only for an integral threshold; (2) two runs of silent windows whose starts lie no
 * more than min_silence_len apart are reported as ONE silent range (detect_silence's `silence_has_gap`); an older detect_silence that
 * closes a range at every break would report two.
 * Input: d_pcm [B, L, channels] int16, interleaved, as pydub's AudioSegment holds PCM and audioop sees every channel of a frame; row b
 * has n_b = d_num_frames[b] frames (device memory, only read on the device, clamped to [0, L]; NULL: L) at sample_rate (sr).
 * The millisecond grid.  p(j) = floor(j*sr/1000) in 64-bit integers is the frame at which millisecond j starts -- pydub evaluates
 * int(j * (sr/1000.0)) in double, and the two are equal at every j whenever fl(sr/1000.0) >= sr/1000 (every multiple of 1000 Hz,
 * 11025, 22050, 44100, 88200, 176400 Hz; the product can then not fall below an integral j*sr/1000, and stays within 1/1000 of any
 * other).  A rate whose quotient rounds DOWN (1001 Hz: they part at j = 1000; 11024 Hz) is TACO_ERR_UNSUPPORTED;
 * taco_pcm_rate_supported answers 1 / 0 for a rate on the host, without a device.  A row is M = round_half_even(
 * 1000.0 * (n / (double)sr)) milliseconds long, Python's round of pydub's expression.  A frame index at or past n reads as a zero frame
 * but still counts as a frame (pydub pads a slice's missing frames with silence; it happens only where M was rounded up).
 * Windows.  W = min_silence_len.  Window i, 0 <= i <= M - W, covers the frames [p(i), p(i + W)) over all channels; S_i is the sum of
 * the squares of its samples and c_i their number, frames x channels.  audioop.rms returns (unsigned)sqrt(S/c) in double (0 for an
 * empty fragment) and pydub calls the window silent when rms <= thresh = 10^(dB/20) * 32768.  With k = floor(thresh), formed by the
 * CALLER in double (the device evaluates no pow or log): silent iff c_i == 0 or S_i < (k + 1)^2 * c_i, an integer comparison, equal to
 * the double one while c_i * (k + 1)^2 < 2^52 -- beyond that TACO_ERR_UNSUPPORTED.  No rms passes 32768, so taco_pcm_nonsilent takes a k
 * above 32768 as 32768 (before that limit is checked).
 * detect_silence.  M < W: no silent range.  Otherwise the maximal runs [a..b] of consecutive silent starts give the ranges [a, b + W];
 * a run opens a new range only if a > b_prev + W and otherwise extends the one before it.
 * detect_nonsilent.  No silent range: [[0, M]].  One silent range [0, M]: [].  Otherwise the gaps [prev_end, start] with prev_end = 0
 * at first, [prev_end, M] added if the last silent range does not end at M, a leading [0, 0] removed.  Milliseconds, in order.
 * taco_pcm_nonsilent writes, per row, the true number of non-silent ranges to d_counts[b], the first max_ranges of them to d_ranges
 * [B, max_ranges, 2] and exact zeros to every other word of the table; M to d_len_ms[b] (nullable); S_i of the row's own windows and
 * zeros in every other word to d_window_sumsq [B, Mmax] (nullable, uint64; for tests and diagnostics), Mmax = the M of a row of L
 * frames.  Three launches: (1) E[b, j], uint64, the sum of squares of millisecond j's frames [p(j), p(j + 1)) -- the only pass over
 * the samples, 16-byte loads, a tile's span staged in LDS, nothing at or past n_b read; (2) the flags: a tile of window starts takes its
 * tile + W energies into LDS and forms their prefix sums there (windows sit on the millisecond grid: no scan across tiles);
 * TACO_ERR_UNSUPPORTED when 256 + W energies exceed 64 KB (W above 7904), or when one millisecond of samples exceeds 48 KB; (3) one
 * workgroup per row orders the ranges with a prefix count, as taco_wav_split does, without atomics.  The workspace BEGINS with E
 * [B, Mmax] uint64: pass it to taco_pcm_range_sumsq as d_energy.
 * taco_pcm_range_sumsq: for a table of ranges [B, max_ranges, 2] in milliseconds, each clamped to 0 <= s <= e <= M, the exact
 * d_sumsq[b, k] = E[s] + ... + E[e - 1] (the frames [p(s), p(e)), zero frames past n) and d_samples[b, k] = (p(e) - p(s)) * channels;
 * zeros at and past d_counts[b].  d_energy holds only the entries j < M_b the taco_pcm_nonsilent call wrote: B, L, sample_rate and
 * d_num_frames must be the ones given to that call (another d_num_frames would read words that were never written).  The caller forms rms_k = (unsigned)sqrt(S_k/c_k) and amplify's factor_k = 10^((target - 20
 * log10(rms_k/32768))/20) from them on the host in double, where the reference forms them: a device log or pow could part by an ulp
 * and flip a floor.
 * taco_pcm_apply_gains: audioop.mul per range and amplify's cut.  Row b of d_out [B, L_out, channels] receives the frames
 * [p(s_0), p(M)) of the row (s_0 the start of its first range: what precedes it is dropped, as the reference drops it; zero frames
 * at or past n), a sample x inside range k as clip(floor((double)x * d_gains[b, k]), -32768, 32767), a sample between ranges
 * unchanged; zeros after; d_out_frames[b] (nullable) = p(M) - p(s_0), 0 for a row without a range.  Only the first min(count,
 * max_ranges) ranges of a row exist for it, and they must be in order, as taco_pcm_nonsilent writes them.  A DEPARTURE: a range whose
 * S_k is 0 would be multiplied by infinity in the reference; the Python caller gives it the gain 1.0, a copy.
 * All three: asynchronous on the stream; no allocation, read-back or synchronisation: capturable; integer sums and one double product
 * per sample: two calls return the same bits.  TACO_ERR_ARG (before any device call): a null required pointer, B, L, channels,
 * sample_rate, min_silence_len, max_ranges or L_out < 1, B > 65535, k < 0, a misaligned pointer, workspace below
 * taco_pcm_nonsilent_workspace_bytes.  TACO_ERR_SHAPE: more milliseconds than int32 holds. */
int taco_pcm_rate_supported(int sample_rate);
size_t taco_pcm_nonsilent_workspace_bytes(int B, int L, int sample_rate);
int taco_pcm_nonsilent(void* hip_stream, const int16_t* d_pcm, const int32_t* d_num_frames /* nullable */, int B, int L, int channels,
                       int sample_rate, int min_silence_len, int k, int max_ranges, int32_t* d_ranges /* [B, max_ranges, 2] */,
                       int32_t* d_counts /* [B] */, int32_t* d_len_ms /* nullable */, uint64_t* d_window_sumsq /* nullable */,
                       void* d_workspace, size_t workspace_bytes);
int taco_pcm_range_sumsq(void* hip_stream, const uint64_t* d_energy /* [B, Mmax] */, const int32_t* d_num_frames, int B, int L, int channels,
                         int sample_rate, const int32_t* d_ranges, const int32_t* d_counts, int max_ranges,
                         uint64_t* d_sumsq /* [B, max_ranges] */, int64_t* d_samples /* [B, max_ranges] */);
int taco_pcm_apply_gains(void* hip_stream, const int16_t* d_pcm, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate,
                         const int32_t* d_ranges, const int32_t* d_counts, int max_ranges, const double* d_gains /* [B, max_ranges] */,
                         int16_t* d_out /* [B, L_out, channels] */, int L_out, int32_t* d_out_frames /* nullable */);

/* ---- recordings to the model's sample rate: librosa.core.load(path, sr=hparams.sample_rate) after decoding, and resample_audio
 * (audio/__init__.py:12-20,30-32; recognition/google.py:48: 24 kHz -> 16 kHz) -- resampy.resample's band-limited sinc interpolation
 * (filter 'kaiser_best') and librosa.core.resample's fix_length, restated ----
 * UNPINNED on resampy and librosa (the reference pins resampy 0.2.0 and librosa 0.5.1; neither is a dependency and no test runs
 * them): a restatement of the documented algorithm, held by tests/resample_reference.py, not by either library.
 * The filter.  The caller supplies the half window of resampy's sinc_window(num_zeros, precision, kaiser(beta), rolloff): with
 * num_table = 2^precision and n = num_table*num_zeros, half[i] = rolloff * sinc(rolloff * i/num_table) * kaiser(2n + 1, beta)[n + i],
 * i = 0..n (n_window = n + 1 entries; the Python package builds it in float64, audio.kaiser_window -- the precedent is
 * taco_gl_set_mel_basis).  With ratio = (double)target_sr/orig_sr: win = half*ratio if ratio < 1 else half; delta[i] = win[i+1] - win[i],
 * delta[last] = 0; scale = min(1, ratio); step = (int)(scale*num_table).  An output at input position tau = n + rem (n integer) is
 *   left wing:  frac = scale*rem, f = frac*num_table, off = (int)f, eta = f - off;
 *               sum over i < (n_window - off)/step of (win[off + i*step] + eta*delta[off + i*step]) * x[n - i]
 *   right wing: the same with frac = scale - scale*rem, over k < (n_window - off)/step, on x[n + k + 1]
 * and a tap outside [0, n_samples) contributes nothing (the bounds of resampy's loops).  No rescaling (librosa's scale=False).
 * EXACT POSITIONS -- where this departs from the pin.  resampy 0.2.0 advances tau by `time_register += 1/ratio`, a serial float64 sum
 * whose rounding depends on every output before it; no parallel kernel reproduces it.  Here tau = t*orig_sr/target_sr exactly: with
 * g = gcd(orig_sr, target_sr), P = target_sr/g, Q = orig_sr/g, output t has n = (t*Q) div P and r = (t*Q) mod P in 64-bit integers and
 * rem = (double)r/P.  The weights of an output then depend on r alone: the filter is a POLYPHASE BANK of P rows, built once by
 * taco_resample_create on the host in double with exactly the operations above in that order (no fused multiply-add), rounded to
 * fp32.  Against the accumulated register (checked in float64 for 44100, 48000, 22050, 16000, 32000, 11025 -> 24000 and 24000 -> 16000
 * over 2e6 outputs each): int(t*(1/ratio)) is the exact n everywhere, and the accumulated register lands on a different integer only
 * at outputs with r == 0 (a rounding to one side of an integer position or the other; 18 286 of 2e6 outputs at 44100 -> 24000,
 * 419 430 of 2e6 at 16000 -> 24000).  When up-sampling, step == num_table and the two evaluations are continuous across that
 * boundary: the values agree to ~1e-10.  When down-sampling, step is truncated and they differ: up to 8e-4 on a row of 3000
 * unit-scale samples at 44100 -> 24000 (2.4e-3 with kaiser_best and 1.8e-2 with a 4-zero filter in tests/test_resample_host.py), at
 * those outputs only.  At every other output the two share n and differ by the register's own rounding (~1e-12 of the position)
 * times the filter's slope.  This is inherent, not an error bound of the kernel.
 * The bank.  Row r has LW + RW = taco_resample_taps entries, LW = taco_resample_left_taps the most left-wing taps any phase has and
 * RW the most right-wing taps; entry j weighs x[n - (LW - 1) + j]: the left wing runs backwards from j = LW - 1 (x[n]) to j = 0, the
 * right wing forwards from j = LW (x[n + 1]); a phase with fewer taps in a wing has exact zeros at that end.  taco_resample_bank copies
 * the fp32 bank to host memory as [P, taps] in this order (for tests and native callers).
 * taco_resample_create needs no device: the bank is uploaded by the first taco_wav_resample on the handle (that first call allocates
 * and copies: make it outside stream capture).  TACO_ERR_ARG with a message: a null pointer, a rate <= 0, num_table < 1, n_window < 2,
 * (int)(scale*num_table) == 0, a filter without taps, a bank of more than 2^22 entries (16 MB; every pair among 8000, 11025, 16000,
 * 22050, 24000, 32000, 44100, 48000 Hz with kaiser_best fits: the largest are 32000 -> 11025, 441 x 372, and 11025 -> 32000, 1280 x
 * 128).  TACO_ERR_UNSUPPORTED: a ratio so small that the inputs of one tile of outputs (taco_resample_tile = 1024 consecutive outputs
 * of a row) and the filter's reach exceed 64 KB of LDS (orig_sr/target_sr above ~14 with kaiser_best).
 * Lengths, the float64 expressions of the reference: taco_resample_computed_len = (int)(n*ratio), what resampy computes;
 * taco_resample_out_len = (int)ceil(n*ratio), what librosa.core.resample returns after fix_length (at most one trailing zero). */
typedef struct taco_resample taco_resample;
int taco_resample_create(int orig_sr, int target_sr, const double* host_half_window, int n_window, int num_table, int device,
                         taco_resample** out);
void taco_resample_destroy(taco_resample* r);
int taco_resample_out_len(const taco_resample* r, int n);
int taco_resample_computed_len(const taco_resample* r, int n);
int taco_resample_phases(const taco_resample* r);            /* P */
int taco_resample_taps(const taco_resample* r);              /* LW + RW: the length of a bank row */
int taco_resample_left_taps(const taco_resample* r);         /* LW: entry LW - 1 of a row weighs x[n] */
int taco_resample_tile(const taco_resample* r);              /* consecutive outputs of a row one workgroup computes */
int taco_resample_bank(const taco_resample* r, float* host_out /* [P, taps] */);
/* B rows at once.  d_in [B, L, channels], interleaved, of in_format TACO_WAV_F32 (float) or TACO_WAV_PCM16 (int16_t, converted as
 * s * (1/32768): audioread's buf_to_float); channels > 1 takes the mean over channels (librosa.to_mono) while the inputs are staged --
 * the sum in double, rounded to fp32 once; no mono copy reaches memory.  d_num_samples [B] device int32 (NULL: every row has L),
 * clamped to [0, L] and only read on the device.  Row b of d_out [B, L_out]: outputs [0, computed_len(n_b)) are computed, exact zeros
 * follow up to L_out, and d_out_samples[b] (nullable) = out_len(n_b) -- both lengths formed on the device in double from the
 * expressions above.  L_out >= taco_resample_out_len(r, L).  fp32 products and sums, taps in the order j = 0, 1, ... by fused
 * multiply-add: an output's bits depend on its row's samples alone, not on the batch, the tile or the call.  One launch, no workspace,
 * no read-back or synchronisation: capturable (after the handle's first call).  TACO_ERR_ARG (before any device call): a null
 * required pointer, B < 1 or > 65535, L < 1, an unknown in_format, channels < 1, L_out below taco_resample_out_len(r, L). */
#define TACO_WAV_F32 0
#define TACO_WAV_PCM16 1
int taco_wav_resample(taco_resample* r, void* hip_stream, const void* d_in, int in_format, int channels,
                      const int32_t* d_num_samples, int B, int L, float* d_out, int L_out, int32_t* d_out_samples);

/* ---- waveform -> linear and mel training targets (audio/__init__.py:48-51,64-67,142-147,155-156,161-162; datasets/generate_data.py:151-158),
 * on the taco_gl handle: the same windowed-DFT pack, slots and frame rows as the Griffin-Lim loop ---- */
/* The mel filter bank, host memory [num_mels, num_freq] row-major (librosa.filters.mel of the reference's _build_mel_basis; the Python
 * package restates it, audio.mel_basis).  Each filter is kept as the band from its first to its last non-zero bin plus that band's
 * weights, so a dense basis works too (full bands).  Calling it again replaces the basis (it waits for launches that read the old one).
 * Allocates device memory: call it at set-up time, not under stream capture. */
int taco_gl_set_mel_basis(taco_gl* g, const float* host_basis, int num_mels);
int taco_spec_num_mels(const taco_gl* g);                    /* filters of the basis in use; 0 = none set */
/* 1 + n_samples / hop_length (librosa stft with center=True), hop_length as taco_gl_create derives it.  Host arithmetic only:
 * takes the parameters, not a handle, so it also answers where there is no device. */
int taco_spec_num_frames(const taco_audio_hparams* hp, int n_samples);
size_t taco_spec_workspace_bytes(const taco_gl* g, int B, int Lmax);
/* spectrogram(y) and melspectrogram(y) of B utterances: d_wav [B, Lmax] float32, d_num_samples [B] device memory (NULL: every row has
 * Lmax samples), only read on the device.  With Tmax = 1 + Lmax / hop_length: d_linear [B, Tmax, num_freq] and d_mel
 * [B, Tmax, num_mels] (NULL: no mel output; otherwise TACO_ERR_STATE until taco_gl_set_mel_basis was called) in the model's layout
 * (generate_data.py stores the reference functions' outputs transposed the same way); row b holds its own T_b = 1 + n_b / hop frames
 * and exact zeros after (the value _pad_target pads with, datafeeder.py:322-323); d_num_frames [B] (nullable) receives T_b.
 * Per row: pre-emphasis y[i] - preemphasis*y[i-1], |stft| with the reflect padding taken at the row's OWN ends, then
 * linear = clip((20 log10(max(1e-5, D)) - ref_level_db - min_level_db) / -min_level_db, 0, 1) and
 * mel = clip((20 log10(max(1e-5, basis . D)) - min_level_db) / -min_level_db, 0, 1) (no ref_level_db on the mel side, as in the reference).
 * Reflect padding needs n_b > n_fft/2: Lmax <= n_fft/2 is TACO_ERR_SHAPE, and each count is clamped on the device to
 * [n_fft/2 + 1, Lmax] (d_num_frames reports the clamped row).  NOT reproduced: librosa serves a shorter recording by reflecting more
 * than once; such a row is analysed as its first n_fft/2 + 1 samples of d_wav here (what lies past its count in d_wav is then read).
 * Asynchronous on the stream; no allocation, read-back or synchronisation: capturable.  Two calls on the same input return the same bits. */
int taco_spec_targets(taco_gl* g, void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int Lmax, float* d_linear,
                      float* d_mel, int32_t* d_num_frames, void* d_workspace, size_t workspace_bytes);

/* ---- a training batch gathered out of a device-resident corpus (the batching of datasets/datafeeder.py:289-328, _prepare_batch /
 * _prepare_inputs / _pad_target, with the data already on the device) ----
 * A STREAM is one field of a batch: a pack of items laid end to end in device memory, tables saying where item i starts and how many
 * rows it has, and the padded rectangle the batch rows go to.  For every stream and batch row b, with i = d_index[b] and
 * c = min(rows[i], rows_out): out[b] receives the first c * width words of item i and exact zeros in every word after them (the value
 * _pad_target and _prepare_inputs pad with), and counts[b] = c.  An index outside [0, N) gives an all-zero row and count 0 and causes
 * no read; no word outside an item's c * width words is read (neither the pack's slack nor a neighbouring item).  Words are copied as
 * bits: float and int32 streams alike.
 * One launch serves all streams of a batch (tokens, mel, linear or samples, loss_coeff, speaker_id); the descriptors travel by value
 * in the kernel arguments.  Asynchronous on the stream; no allocation, read-back or synchronisation: capturable, and since d_index is
 * device memory a replayed graph collates a different batch each time.  Offsets are 64-bit.  pack and out must be 4-byte aligned;
 * any alignment of item starts and batch rows beyond that is served.
 * TACO_ERR_ARG (before any device call): null streams / d_index / pack / out, n_streams outside [1, TACO_COLLATE_MAX_STREAMS],
 * width < 1, rows_out < 1, B < 1, N < 1, or start == NULL together with rows != NULL. */
#define TACO_COLLATE_MAX_STREAMS 8
typedef struct {
  const void*      pack;      /* device, 4-byte words (float or int32: bits are copied, never converted) */
  const long long* start;     /* device [N]: word offset of item i in pack; NULL: item i starts at i * rows_out * width */
  const int32_t*   rows;      /* device [N]: rows of item i (a row is `width` words); NULL: every item has rows_out rows */
  int32_t          width;     /* words per row: 1 (tokens, samples, per-item scalars), num_mels, num_freq */
  int32_t          rows_out;  /* rows per batch row of the output */
  void*            out;       /* device [B, rows_out, width] */
  int32_t*         counts;    /* device [B], nullable: rows copied for batch row b */
} taco_collate_stream;
int taco_collate(void* hip_stream, const taco_collate_stream* streams, int n_streams, const int32_t* d_index, int B, int N);

/* ---- training-side entry points on flat buffers (loss, schedule, clip + Adam); forward/backward: taco_train_* below ---- */
/* add_loss (tacotron.py:274-302).  d_mel_* [B,T,num_mels], d_lin_* [B,T,num_freq], d_loss_coeff [B] (nullable = 1).
 * d_losses[4] = loss, mel_loss, linear_loss, loss_without_coeff.  Workspace >= 64 KiB.
 * prioritize_loss: the band is bins [int(165 / (sample_rate / 2) * num_freq), int(5000 / (sample_rate / 2) * num_freq)) clamped to num_freq, as the
 * reference's slice linear_loss[:, :, lower:upper] clamps it (sample rates below 10000 Hz put the 5 kHz bin past the last one); its mean is over the
 * bins that exist.  The training step's gradient counts the band the same way. */
int taco_loss_f32(void* hip_stream, const float* d_mel_out, const float* d_mel_tgt, const float* d_lin_out,
                  const float* d_lin_tgt, const float* d_loss_coeff, int B, int T, int num_mels, int num_freq,
                  int prioritize_loss, int sample_rate, float* d_losses, void* d_workspace, size_t workspace_bytes);
/* learning-rate schedule of add_optimizer (tacotron.py:313-325); global_step = completed updates. */
float taco_learning_rate(long long global_step, float initial_learning_rate, int decay_learning_rate_mode,
                         int is_randomly_initialized);
/* clip_by_global_norm + tf.train.AdamOptimizer update (tacotron.py:327-336, TF form of Adam) on flat fp32 buffers.
 * Workspace >= 8 KiB.  d_gnorm_out nullable.  A non-finite global norm (NaN / inf: a step poisoned after a device fault, or a genuine
 * overflow) leaves parameters and moments untouched -- where tf.clip_by_global_norm would turn every parameter into NaN. */
int taco_adam_step_f32(void* hip_stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n,
                       long long global_step, float learning_rate, float beta1, float beta2, float epsilon, float clip_norm,
                       float* d_gnorm_out, void* d_workspace, size_t workspace_bytes);
/* Segmented norms over a flat fp32 buffer: the gradient scalars of the reference's summaries (add_stats, train.py:50-77; fetched at
 * train.py:232-240), whose scope 'train' adds max_gradient_norm = reduce_max([tf.norm(g) for g in model.gradients if g is not None]).
 * Caveat: train.py:156 calls add_stats(model, scope_name='stats'), so in the reference as run the 'train' branch never executes; the
 * function is reproduced as it stands, and 'train' is the useful scope.  model.gradients are the UNCLIPPED gradients
 * (tacotron.py:328-330: self.gradients is taken before clip_by_global_norm), so these are norms of the unclipped gradients too.
 * A plan holds the work table of `n_seg` segments [h_offsets[s], h_offsets[s + 1]) (element indices, ascending, a segment may be empty,
 * no alignment asked of any offset), built on the host once: pieces of at most taco_segnorm_piece_floats() floats, none across a
 * segment boundary, ascending.  A call reads the buffer ONCE (16-byte loads in the aligned interior of a piece, scalar loads at its
 * ragged ends) and writes
 *   d_norms[s]  = sqrt(sum of x[i]^2 over segment s), 0 for an empty segment; beyond the fp32 range: +inf;
 *   d_stats[0]  = the largest norm, *d_argmax = its segment: ties go to the first index; if any counted norm is NaN the maximum is NaN
 *                 and the index is that of the first NaN segment (a step that taco_train_forward_backward poisoned after a device
 *                 fault -- NaN in d_grads[0] -- stays visible; tf.reduce_max's treatment of NaN is not imitated);
 *   d_stats[1]  = the norm over all counted segments together (the global norm that clip_by_global_norm divides by).
 * skip (h_skip[s] != 0): the segment is not read at all, its norm is written as 0, and it takes no part in the maximum, its index
 * or the global norm; with no counted segment at all: 0, 0 and index -1.
 * Squares and sums are accumulated in double (an fp32 product is exact in double) in an order fixed by the table -- no
 * floating-point atomics: the same input gives the same bits on every call, from any stream and in a replayed graph.
 * Three launches; no allocation, no host synchronisation, no copy and no memset: capturable.  All state is in the plan, so calls on ONE
 * plan must be ordered among themselves (one stream, or events between streams).
 * TACO_ERR_ARG, before any HIP call: a null pointer (d_argmax may be null), n_seg < 1, descending offsets, h_offsets[n_seg] > n, an
 * input that is not 4-byte aligned, d_norms / d_stats / d_argmax overlapping the n floats of the input. */
typedef struct taco_segnorm_plan taco_segnorm_plan;
int taco_segment_norms(const taco_segnorm_plan* plan, void* hip_stream, const float* d_flat, size_t n,
                       float* d_norms /* [n_seg] */, float* d_stats /* [2]: max norm, norm over all counted segments */,
                       int32_t* d_argmax /* [1] or null */);
/* P, the largest piece of the work table of taco_segment_norms (train.py:50-77) in floats */
int taco_segnorm_piece_floats(void);
/* the plan of taco_segment_norms (train.py:50-77; rules and errors there).  Allocates and copies on `device`: make it outside stream capture. */
int taco_segnorm_plan_create(const uint64_t* h_offsets /* [n_seg+1], host */, int n_seg,
                             const uint8_t* h_skip /* [n_seg] or null */, int device, taco_segnorm_plan** out);
/* frees a plan of taco_segment_norms (train.py:50-77) and its device buffers; null is allowed */
void taco_segnorm_plan_destroy(taco_segnorm_plan* plan);

/* ---- training path (config C4): teacher-forced forward with batch-statistics BatchNorm
 * (tacotron.py:26,199-202; modules.py:131; helpers.py:35-67), add_loss and its full backward pass (tf.gradients of
 * tacotron.py:274-336).  All parameters live in ONE flat fp32 device buffer owned by the caller (layout: the tensors of
 * taco_model_weight_name() in order, TF layout, no padding) and all gradients in a second buffer of the same layout --
 * the single all-reduce bucket of the data-parallel step.  A taco_train owns only index maps and weight packs that it
 * regenerates from the flat parameters (taco_train_refresh) after every optimizer step.
 * modules.py:24 calls tf.layers.dropout without training=True, so the reference applies no prenet dropout even when
 * training; neither does this path.  Supported: single-speaker and multi-speaker ('simple', 'deepvoice') models, all three attention types. ---- */
typedef struct taco_train taco_train;
int taco_train_create(const taco_hparams* hp, int device, taco_train** out);
void taco_train_destroy(taco_train* t);
/* the model handle whose taco_model_num_weights / taco_model_weight_name give the flat parameter order and shapes */
taco_model* taco_train_model(taco_train* t);
/* Deterministic reductions: on = 1 makes every sum over rows that normally leaves its workgroup through fp32 atomics (weight
 * gradients, bias and BatchNorm sums, embedding gradients, d attention_v) a two-stage sum in a fixed order, so that a step is
 * run-to-run reproducible TO THE BIT, as the reference's single-device step is (train.py:215-219).  Costs 192 MB of workspace
 * (taco_train_workspace_bytes reflects it: query it again) and 6.6 % of the step (15.85 instead of 14.87 ms at the C4 shard, round 4: the small
 * problems stay in their group launches, their per-slice partials are added up by two more group launches).  Default 1 since round 4
 * (rounds 1-3: 0); on = 0 selects the atomics. */
int taco_train_set_deterministic(taco_train* t, int on);
/* Weight gradients: on = 0 (default) computes dW = X^T . dY on the bf16 matrix cores with operands split three ways (24 bits) and
 * six products per tile, fp32 accumulation (k_wgrad_bf3: fp32-grade, ~2^-24 per product); on = 1 keeps them on the
 * exact-fp32 MFMA (k_wgrad, round 1).  Per trainer (as every taco_train_set_* switch): A/B and test hook. */
int taco_train_set_exact_wgrad(taco_train* t, int on);
/* Split-bf16 weight gradients from PRE-SPLIT operands (csrc/taco_wgrad_planes.h): mode 1 (default) converts the operands of the large
 * problems -- a whole conv bank, proj_1, the linear head -- once into bf16 planes and multiplies them with a kernel that converts
 * nothing; mode 2 sends every eligible problem that way (test hook); mode 0 keeps all of them on k_wgrad_bf3.  Same six products, same
 * fixed summation order per slice.  Changing 0 <-> non-zero changes taco_train_workspace_bytes. */
int taco_train_set_wgrad_planes(taco_train* t, int mode);
/* How many weight gradients of the last taco_train_forward_backward were computed from pre-split planes (a conv bank counts once). */
int taco_train_planes_problems(const taco_train* t);
/* Feed-forward GEMMs of the training step (both CBHGs' conv banks / projections / highways / GRU input projections, encoder prenet,
 * linear head) and their data gradients.  k_gemm = exact-fp32 MFMA; k_gemm_bf3 = the inference kernels: bf16 matrix cores, both
 * operands split in two, three products per tile (~2^-17 per product, fp32 accumulation), weight planes re-split on the device from
 * the live parameters by taco_train_refresh (k_bf3_gather).
 *   on = 3 (the default of rounds 2-3): forward on k_gemm, data gradients on k_gemm_bf3.  The forward -- and with it every ReLU / max-pool decision and
 *          every BatchNorm statistic -- is exact; a data gradient is linear in dY, and the split costs 4e-6 of the gradient norm
 *          against the all-exact step (measured; tensor by tensor <= 4e-5 of the tensor's scale).  9 % off the C4-shard step.
 *   on = 1: everything on k_gemm (rounds 1-2).
 *   on = 0: everything on k_gemm_bf3: 16 % off the step; the forward's ~1e-5 relative product error is amplified by the BatchNorm
 *          backward's cancellations to ~1e-3 of the gradient norm and resolves near-ties differently.
 *   on = 2: forward k_gemm_bf3, data gradients k_gemm (A/B hook).
 *   on = 4 (default since round 4): forward on the SIX-product instantiation of k_gemm_bf3 (every operand split three ways, hi + lo + l3 = 24 mantissa bits;
 *          l3*hi, hi*l3, lo*lo, lo*hi, hi*lo, hi*hi accumulated in fp32: 2^-24 per product, fp32-grade, as k_wgrad_bf3), data
 *          gradients as in mode 3: the forward leaves the fp32-input MFMA (1/16 of the bf16 rate) without touching its decisions.
 * Call taco_train_refresh after switching (the planes are generated only while an engine that needs them is selected). */
int taco_train_set_exact_gemm(taco_train* t, int on);
/* Back-propagation through the decoder loop (tf.gradients of rnn_wrappers.py:218-341 under train.py:215-219): persistent = 1 (default)
 * runs all T_out/r steps as ONE whole-chip launch (k_decoder_bwd_xcd, csrc/taco_decoder_bwd_xcd.h) when the forward ran on the persistent
 * decoder (reference widths, every model type, <= 64 rows, a whole MI355X); 0 keeps the chain of per-stage launches. */
int taco_train_set_bptt_engine(taco_train* t, int persistent);
size_t taco_train_num_params(const taco_train* t);
int taco_train_param_offset(const taco_train* t, const char* name, size_t* offset);
/* regenerate every weight pack from the flat parameter buffer (call after loading parameters and after every update) */
int taco_train_refresh(taco_train* t, void* hip_stream, const float* d_params);
size_t taco_train_workspace_bytes(const taco_train* t, int B, int T_in, int T_out);
/* Synchronised BatchNorm for the data-parallel step: with a callback set, every BatchNorm layer's batch
 * statistics (forward: sum, centred sum of squares; backward: sum dy, sum dy*xhat) are handed to `fn` as a device vector that
 * the host must replace, in place and ordered on the stream of the running taco_train_forward_backward call, by its sum over
 * all `world_size` ranks (RCCL all-reduce).  Mean, variance, moving averages and the input gradient are then those of the
 * global batch, i.e. of the reference's single-device step over the whole batch (modules.py:131, train.py:145-166); the
 * gamma/beta gradients stay per-rank sums and are averaged by the flat gradient all-reduce like every other parameter.
 * fn == NULL (default): statistics of this rank's rows only.  40 calls per step at the reference architecture (12 forward,
 * 28 backward), 80 to 4096 floats each.  Not capturable into a hipGraph. */
typedef void (*taco_sync_sum_fn)(void* user, float* d_vec, int n);
int taco_train_set_sync_bn(taco_train* t, taco_sync_sum_fn fn, void* user, int world_size);
/* One training forward (+ backward when d_grads != NULL).  d_params is in/out: a forward+backward pass updates the BatchNorm
 * moving averages in place (UPDATE_OPS run only as a dependency of `optimize`, tacotron.py:334); a forward-only pass
 * (d_grads == NULL: loss fetches, the test model) leaves them untouched, as the reference does.  d_mel_targets [B,T_out,num_mels], d_linear_targets [B,T_out,num_freq],
 * T_out a multiple of r, T_out/r <= max_iters (helpers.py:44-48).  d_losses[4] = loss, mel_loss, linear_loss,
 * loss_without_coeff (nullable).  d_mel_out / d_linear_out / d_alignments ([B,T_in,T_out/r]) nullable.
 * d_grads (flat, overwritten) = d loss / d parameter; moving statistics get zero.
 * rnn_decoder_test_mode bit 0 (helpers.py:63-64, the test model of train.py:158-166): the decoder is fed its own previous
 * output instead of the target frame; forward/loss only (d_grads must be NULL).  Bit 1: freeze the moving averages even though
 * d_grads is given (a warm-up pass whose update is discarded, e.g. before capturing the step into a graph).
 * Device faults: if a persistent whole-chip kernel of the step gave up (its bounded spin expired; taco_model_device_errors on
 * taco_train_model(t) reports and clears the sticky word), d_losses[0..3] and d_grads[0] are set to NaN on the stream: the fault is
 * visible in the step's own outputs, survives the data-parallel all-reduce, and makes taco_adam_step_f32 skip the update (the
 * BatchNorm moving averages, which the pass writes itself, may have absorbed that pass's statistics with weight 0.01). */
int taco_train_forward_backward(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const int32_t* d_inputs,
                                const int32_t* d_input_lengths, const int32_t* d_speaker_id /* nullable: single speaker */,
                                const float* d_mel_targets, const float* d_linear_targets,
                                const float* d_loss_coeff, int B, int T_in, int T_out, int prioritize_loss, int sample_rate,
                                float* d_losses, float* d_mel_out, float* d_linear_out, float* d_alignments,
                                int rnn_decoder_test_mode, void* d_workspace, size_t workspace_bytes);
/* The per-variable gradient norms of add_stats' scope 'train' (train.py:50-77; in the reference as run, train.py:156 passes scope
 * 'stats' and that branch never executes): taco_segment_norms over d_grads (the flat gradients of taco_train_forward_backward, UNCLIPPED as
 * model.gradients is, tacotron.py:328-330) with one segment per tensor of taco_model_weight_name, in that order.  The BatchNorm moving
 * statistics (".../moving_mean", ".../moving_variance") are no trainable variables and have no entry in model.gradients: they are
 * skipped -- norm 0, outside the maximum, its index and the global norm.  d_stats[0] is the reference's max_gradient_norm, d_stats[1]
 * the global norm that taco_adam_step_f32 computes again for its clip (both accumulated in double, in different orders).  Double accumulation,
 * determinism, the NaN, tie and skip rules and the argument errors are those of taco_segment_norms.  After a data-parallel all-reduce the
 * norms are those of the averaged gradient, bit-equal on every rank.  The plan is built from the trainer's layout on the first call
 * (which allocates: make it outside stream capture) and freed by taco_train_destroy; later calls are capturable. */
int taco_train_grad_norms(taco_train* t, void* hip_stream, const float* d_grads,
                          float* d_norms /* [taco_model_num_weights] in taco_model_weight_name order */,
                          float* d_stats, int32_t* d_argmax);

/* Persistent (multi-workgroup, in-kernel synchronised) kernels bound every spin; if one ever expires it sets a
 * device-side error word and all workgroups leave.  This call synchronises, returns the word in *out and clears it;
 * non-zero means the outputs of the affected forward are invalid. */
int taco_model_device_errors(taco_model* m, int* out);
/* Which engine a forward of this shape WOULD run on -- and, when it is not the persistent whole-chip one, why not (widths, rows, LDS,
 * compute units of the device, debug switches).  Nothing is launched.  `out` receives a NUL-terminated line (out_len >= 64; truncated
 * if shorter than the text).  The run-time facts (exchange protocol the census chose) are in taco_debug_decoder_info afterwards.
 * flags: bit 0 = manual alignments; for a taco_decoder_forward call, bit 1 = teacher frames, bit 2 = the per-step state dump (which keeps
 * up to 64 rows in one pass).  For a training shadow model (taco_train_model) the line describes a training step, backward loops included. */
int taco_model_engine_plan(taco_model* m, int B, int T_in, int T_mel, int flags, char* out, int out_len);
/* Batch-position bit-invariance for serving setups that need it (a request's outputs must not depend on which rows it was batched or
 * sharded with).  on = 1: every row tile of the fused point-wise kernel walks a layer's contraction from step 0, so a row's fp32
 * accumulation order is the same wherever the row lands: outputs are bitwise equal under batch permutation / re-sharding at any
 * size.  on = 0 (default): the workgroups of an XCD start their K loops at different steps (faster weight stream out of the L2);
 * results are reproducible run to run and equal under permutation to fp32 rounding (bitwise only while a layer has fewer than 8
 * row tiles of 64 rows).  Takes effect for calls and plans made afterwards. */
int taco_model_set_batch_invariant(taco_model* m, int on);

/* ---- matching recognised text to script lines (recognition/alignment.py:21-26,107-113) ----
 * Text is a pool of Unicode code points, d_chars [n_chars] int32, and d_offsets [n_texts + 1]: text t is d_chars[d_offsets[t] ..
 * d_offsets[t+1]).  The caller strips what the reference's plain_text strips before it packs the pool.
 *
 * taco_text_matches: d_matches[p] = M of difflib.SequenceMatcher(None, a, b), a = text d_pairs[2p], b = text d_pairs[2p+1]; the
 * reference's similarity() is ratio() = 2.0 * M / (len(a) + len(b)), and 1.0 when both are empty, which the caller forms in double.
 * M is the total length of difflib's matching blocks: the longest common block of a and b, then the same left of it in both strings and
 * right of it in both.  The tie rule: among the longest blocks the one that starts earliest in a wins, among those the one that starts
 * earliest in b; M depends on it and the kernel follows it.  Exact equality with difflib holds for len(b) <= 199: from len(b) = 200 on
 * difflib's autojunk drops the characters of b that occur more than 1 + len(b)/100 times from its index and finds other blocks, so such
 * a pair is REFUSED, not approximated.  len(a) has no cap.
 * The -1 convention: a refused pair gets d_matches[p] = -1 and nothing else changes; the stream stays sound.  Refused are: len(b) >= 200;
 * a text index outside [0, n_texts); offsets of either text that decrease or run outside [0, n_chars].  Score those on the host.
 *
 * taco_text_best_two: the decision of :107-113 per group g, the pairs [d_group_offsets[g], d_group_offsets[g+1]) of one utterance
 * (increasing offsets into the pairs; they are trusted, the pair count is not an argument).  d_best[g] = {the pair of the largest ratio
 * -- the first such pair on equal ratios --, its M, its T = len(a) + len(b), flag}.  flag = 1 when every other pair of the group has a
 * strictly smaller ratio (the reference's first[1] > second[1]; a group of one pair has flag 1).  Ratios are compared as M1*T2 against
 * M2*T1 in 64-bit integers, T == 0 counting as ratio 1; that is the order of the doubles 2.0*M/T wherever T1*T2 < 2^52 (beyond, two
 * different fractions may round to one double).  Refused pairs (-1) are skipped and set the group's flag to 0, so the caller knows to
 * redo that group on the host.  An empty group, or one whose pairs are all refused, writes {-1, 0, 0, 0}.
 *
 * Both calls launch on hip_stream only: no allocation, no synchronisation, no workspace, plain stores, every output element written
 * exactly once; safe under stream capture.  Checked before any HIP call (TACO_ERR_ARG): a null pointer (d_chars may be null when
 * n_chars is 0), a negative count, an output that overlaps an input (for taco_text_best_two's d_matches and d_pairs, whose length it
 * does not know: their first element).  n_pairs or n_groups of 0 is a no-op.  Byte counts are formed in 128 bits. */
int taco_text_matches(void* hip_stream, const int32_t* d_chars, long long n_chars, const int32_t* d_offsets /* [n_texts + 1] */, int n_texts,
                      const int32_t* d_pairs /* [n_pairs, 2]: text index of a, of b */, int n_pairs, int32_t* d_matches /* [n_pairs] */);
int taco_text_best_two(void* hip_stream, const int32_t* d_matches, const int32_t* d_pairs, const int32_t* d_offsets, int n_texts,
                       const int32_t* d_group_offsets /* [n_groups + 1] into the pairs */, int n_groups, int32_t* d_best /* [n_groups, 4] */);

/* ---- dynamic time warping of two feature sequences (not in the reference: the distance of a free-running decoder's mel frames from
 * their targets with the drift in time taken out, where tacotron.py:274-302 compares frame t with frame t) ----
 * Pair p warps d_a[p, :n, :] onto d_b[p, :m, :] (fp32 rectangles [B, Ta, D] and [B, Tb, D]); n = d_len_a[p] clamped to [1, Ta] and
 * m = d_len_b[p] clamped to [1, Tb] on the device, a NULL length array meaning full rows.  Nothing past the lengths is read: slack may
 * hold anything, NaN included.
 * Frame cost c(i, j), summed over d ascending in fp32: cost_kind 0 = (1/D) * sum_d |a_id - b_jd| (the per-frame term of the mel L1 of
 * tacotron.py:278), cost_kind 1 = sqrt(sum_d (a_id - b_jd)^2).
 * Recurrence (symmetric steps, diagonal weight 2, so the normaliser does not depend on the path):
 *   G(0,0) = 2 c(0,0);  G(i,0) = G(i-1,0) + c(i,0);  G(0,j) = G(0,j-1) + c(0,j);
 *   G(i,j) = min(G(i-1,j-1) + 2 c(i,j), G(i-1,j) + c(i,j), G(i,j-1) + c(i,j));   d_total[p] = G(n-1,m-1);  d_dist[p] = total / (n + m).
 * For n == m, dist <= the mean of c(i,i).  d_dir [B, Ta, Tb] (nullable) receives for every cell with i < n and j < m where its value
 * came from: 0 = (i-1,j-1), 1 = (i-1,j), 2 = (i,j-1); border cells their only predecessor, cell (0,0) 0; on ties the diagonal is
 * tried first, then (i-1,j), then (i,j-1), a later candidate winning under strict '<' only.  Cells outside are left untouched.
 * If any used element of a pair is NaN or infinite, that pair's total and dist are NaN (a flag carries it, not the minimum); other
 * pairs are not affected and the call ends normally.
 * No Ta x Tb memory exists unless d_dir is given: costs are formed on the fly, G lives in registers (csrc/taco_dtw.h).  One fixed
 * summation order and no atomics: two calls give the same bits.  The call launches on hip_stream only: no allocation, no
 * synchronisation, no read-back; safe under stream capture.  Ta, Tb and B have no cap; D above 128 is refused (TACO_ERR_UNSUPPORTED:
 * a column's features are registers).  d_workspace: taco_dtw_workspace_bytes(B, Ta, Tb, D) bytes, which is 0 (and the pointer may
 * then be NULL) while Tb fits one strip of columns.
 * Checked before any HIP call: a null d_a, d_b or d_dist, or a null workspace where the query is not 0, B, Ta, Tb or D < 1, an unknown
 * cost_kind, an output (d_dist, d_total, d_dir, the workspace) that shares a byte with an input or another output -> TACO_ERR_ARG;
 * D > 128 -> TACO_ERR_UNSUPPORTED; a workspace below the query -> TACO_ERR_STATE.  Byte counts are formed in 128 bits.
 *
 * taco_dtw_path: the warping path of every pair from d_dir, ascending from (0,0) to (n-1,m-1): d_path [B, Ta+Tb-1, 2] int32 rows
 * (i, j), entries from d_path_len[p] on set to -1.  Whatever bytes d_dir holds, the walk ends within n + m - 1 entries inside the
 * rectangle: a byte above 2 counts as 0, in row 0 the move is to (0,j-1), in column 0 to (i-1,0); garbage gives a wrong path, nothing
 * worse.  Same stream rules; TACO_ERR_ARG for a null d_dir, d_path or d_path_len, B, Ta or Tb < 1, or an output overlapping an input or
 * the other output. */
size_t taco_dtw_workspace_bytes(int B, int Ta, int Tb, int D);
int taco_dtw(void* hip_stream, const float* d_a, const int32_t* d_len_a, const float* d_b, const int32_t* d_len_b,
             int B, int Ta, int Tb, int D, int cost_kind,
             float* d_dist /* [B] */, float* d_total /* [B], nullable */, uint8_t* d_dir /* [B,Ta,Tb], nullable */,
             void* d_workspace, size_t workspace_bytes);
int taco_dtw_path(void* hip_stream, const uint8_t* d_dir, const int32_t* d_len_a, const int32_t* d_len_b,
                  int B, int Ta, int Tb, int32_t* d_path /* [B,Ta+Tb-1,2] */, int32_t* d_path_len /* [B] */);

/* ---- pitch tracking: YIN F0 tracks, and F0 error statistics along a warping path (not in the reference, which is judged by ear; with
 * the cepstral distortion above these are the objective numbers of a synthesiser: envelope, intonation, voicing) ----
 * taco_f0_yin: the YIN estimator (de Cheveigne and Kawahara 2002, steps 2 to 5) per row of d_wav [B, L] (fp32) with that row's own sample
 * count n = d_num_samples[b] clamped to [0, L] on the device, a NULL array meaning L.  This project's own definition, UNPINNED on any
 * pitch-tracking package; tests/yin_reference.py restates it in NumPy.
 *   tau_min = floor(sample_rate / fmax), tau_max = ceil(sample_rate / fmin) (formed in double from the fp32 arguments), W = window,
 *   F = 1 + L / hop columns; row b owns the frames t < 1 + n / hop -- the grid of taco_spec_num_frames, so a path found on mel frames
 *   indexes the F0 track directly.  For frame t:
 *   1. samples: x~[k] for k = s0 .. s0 + W + tau_max, s0 = t * hop - (W + tau_max) / 2 (integer division); x~[k] = x[k] inside [0, n)
 *      and 0 outside.  Nothing at or past n is read: the slack may hold anything, NaN included.
 *   2. d(tau) = sum_{j < W} (x~[s0+j] - x~[s0+j+tau])^2 for tau = 0 .. tau_max + 1, in fp32: each difference rounded, its square added to
 *      the running sum by one fmaf; the sum is formed directly (not as energies minus a correlation, which cancels), in one fixed order
 *      of the kernel's own (csrc/taco_f0.h: blocks of j, then the blocks' sums).
 *   3. S(tau) = sum_{k = 1 .. tau} d(k) (fp32, one fixed order); d'(0) = 1; d'(tau) = (d(tau) * tau) / S(tau), the product and the quotient
 *      two separately rounded fp32 operations; d'(tau) = 1 where S(tau) == 0.
 *   4. the lag: the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; from there tau -> tau + 1 while tau + 1 <= tau_max and
 *      d'(tau + 1) < d'(tau).  That is tau*, and the frame is voiced.  If no tau is below the threshold the frame is unvoiced and tau* is
 *      the first argmin of d' over the range.
 *   5. y0, y1, y2 = d'(tau* - 1), d'(tau*), d'(tau* + 1); q = (y0 - 2 * y1) + y2; delta = q > 0 ? clamp((0.5 * (y0 - y2)) / q, -0.5, 0.5)
 *      : 0, every operation rounded on its own (nothing contracted); f0 = sample_rate / (tau* + delta) when voiced, exactly 0 when not.
 *   Outputs: d_f0 [B, F]; d_aper [B, F] (nullable) = d'(tau*), voiced or not; d_lag [B, F] (nullable) = tau*, int32.  Columns past a
 *   row's own frames receive exact zeros.  A frame that reads a NaN or an infinity gives NaN in d_f0 and d_aper and -1 in d_lag; other
 *   frames are not affected.  (Silence: S == 0 everywhere, d' = 1, unvoiced, tau* = tau_min.)
 * No atomics and one fixed summation order: two calls and a captured replay give the same bits.  Where every d, S and d * tau is an
 * integer below 2^24 (integer samples in [-8, 8], window <= 256, tau_max <= 255) the sums are exact in any order and the outputs are
 * bit-equal to the restatement's.
 *
 * taco_f0_path_stats: per pair p, over the entries k < d_path_len[p] (clamped to [0, path_cap]) of d_path [B, path_cap, 2] as
 * taco_dtw_path writes it, with fa = d_f0_a[p, i] ([B, Fa]) and fb = d_f0_b[p, j] ([B, Fb]); a track value is voiced when it is > 0.
 * Both voiced: c = 1200 * log2(fa / fb) (fp32), c^2 and a count are accumulated; exactly one voiced: a V/UV error is counted; an entry
 * whose i or j lies outside [0, Fa) x [0, Fb) is skipped (-1 fill included); a NaN track value at a used entry makes that pair's sum
 * NaN (the entry still counts as used).  d_stats [B, 4] fp32 = {sum c^2, entries voiced on both sides, V/UV errors, entries used}.
 * One workgroup per pair, strided partial sums and one fixed tree: bit-reproducible.
 *
 * Both calls launch on hip_stream only: no allocation, no workspace, no synchronisation, no read-back; safe under stream capture.  The
 * stream's device must be the current one (a plan above 64 KB of LDS -- a long frame or a long hop -- sets a kernel attribute there).
 * Checked before any HIP call: a null required pointer; B, L, hop, window, Fa, Fb or path_cap < 1; sample_rate < 1; fmin <= 0 or
 * fmax <= fmin; tau_min < 2; a threshold outside (0, 1]; an output that shares a byte with an input or another output -> TACO_ERR_ARG;
 * a frame of window + tau_max + 2 floats above 8192 -> TACO_ERR_UNSUPPORTED (k_yin keeps a frame, its lag sums and their parts in the
 * 144 KB of LDS it is built for; 24 kHz / 50 ms / 60 Hz needs 1602).  Byte counts are formed in 128 bits. */
int taco_f0_yin(void* hip_stream, const float* d_wav, const int32_t* d_num_samples /* nullable */, int B, int L,
                int sample_rate, int hop, int window, float fmin, float fmax, float threshold,
                float* d_f0, float* d_aper /* nullable */, int32_t* d_lag /* nullable */);
int taco_f0_path_stats(void* hip_stream, const float* d_f0_a, int Fa, const float* d_f0_b, int Fb,
                       const int32_t* d_path, const int32_t* d_path_len, int B, int path_cap, float* d_stats);

#ifdef __cplusplus
}
#endif
#endif /* TACO_ABI_H */
