/* taco_debug.h -- test hooks, A/B switches and timing / tracing hooks of libtaco_hip.so.
 *
 * NOT part of the drop-in boundary: a reference-side binding needs include/taco_abi.h only.  What is
 * declared here exists for this repository's own tests (tests/), benchmarks (bench.py companions and stage timing) and tools/;
 * the functions may change between builds without a change of TACO_ABI_VERSION.  The library exports them unconditionally. */
#ifndef TACO_DEBUG_H
#define TACO_DEBUG_H

#include "taco_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test hook: which BiGRU scan runs (tests / A-B timing).  Any other value is refused with TACO_ERR_ARG and changes nothing.
 *    0 = two launches per step
 *    1 = (default) the fastest kernel that fits: k_bigru_oct (H = 256, 9 to 32 rows) or k_bigru_duo (up to 64 rows) on a whole MI355X,
 *        else k_bigru_resw (H = 256), k_bigru_quad (H = 128), k_bigru_rows (other widths)
 *    2 = k_bigru_rows (weights streamed every step)
 *    3 = k_bigru_res (one unit per thread, libm transcendentals; H = 256 / 128)
 *    7 = k_bigru_resw (H = 256: one CU per direction and row)
 *   10 = k_bigru_oct wherever it fits (also below 9 rows), else k_bigru_duo
 *   11 = k_bigru_duo, never k_bigru_oct
 * A forced kernel that does not fit the width or the device falls back to k_bigru_rows. */
int taco_debug_set_persistent(taco_model* m, int on);

/* test hook: on = 1 (default) runs the feed-forward GEMMs of inference on the bf16 matrix cores with 3-term split
 * operands (fp32-grade accuracy, ~1e-5); 0 = exact-fp32 MFMA everywhere.  tile_n: 0 auto, 4 = 64x64, 5 = 64x64 with four wave groups
 * splitting K inside the workgroup, 7 = 64x256 by 1x8 waves, 9 = 64x128 by 1x4 waves, 10 = tile 7 with two wave groups splitting K (auto
 * picks among these five).  Any other tile_n -- the retired tiles 1, 2, 3 and 11 included -- is TACO_ERR_ARG and changes nothing, `on` included.
 * A forced tile that a launch has no instantiation for is answered by gemm_plan (csrc/taco_lib.hip): tile 10 exists at three products for
 * one weight matrix only, so a highway layer or a six-product launch under it runs tile 7; a six-product highway layer under tile 5 runs tile 4.
 * on bit 2 (on = 5): the point-wise tail of a CBHG ([dense ->] highway x depth -> BiGRU input projection; modules.py:72-96) runs as
 * one launch per layer instead of ONE launch with the activations resident on the CU (csrc/taco_chain.h, the default with on = 1).  The
 * encoder prenet then runs as one GEMM launch per layer too, and the forward's zero fills -- riders of its chain launch otherwise -- as
 * one launch of k_zero_fill in front.
 * on bit 3 (on = 9): conv bank and proj_1 of a CBHG as two launches instead of the fused front (csrc/taco_front.h).
 * on bit 4 (on = 17): with the fused front, proj_1's epilogue (k_front_combine) and proj_2 as launches of their own instead of the fused
 * entry of the point-wise chain (csrc/taco_chain.h).
 * on bit 5 (on = 33): the linear head on k_gemm_bf3's tiles instead of the row sweep k_head_sweep (csrc/taco_head.h).
 * on bit 6 (on = 65): every feed-forward layer on the six-product instantiation k_gemm_bf3<..., X6> (operands split three ways: fp32-grade
 * products on the bf16 pipe), one launch per layer: the fused kernels (front, chain, head sweep) are three-product kernels and stay out.
 * Ignored on a training shadow model (taco_train_set_exact_gemm picks its level).
 * A forced tile, a forced k_gemm config (taco_debug_force_gemm_config) and on = 0 switch all fused kernels off too.  Which kernels a call
 * then gets: ff_plan, prenet_chain_why, head_sweep_why and gemm_plan (csrc/taco_lib.hip), told by taco_model_engine_plan. */
int taco_debug_set_bf3(taco_model* m, int on, int tile_n);

/* retired: the chunked post-net overlap (feed-forward stages on a second stream behind a launch-per-stage decoder loop; it measured slower,
 * profiles/README.md).  on = 0 returns 0; any other value is TACO_ERR_ARG and changes nothing.  Kept because bench.py --overlap calls it. */
int taco_debug_set_overlap(taco_model* m, int on);
/* debug/test: 0 = run decoder prenet layer 1 as its own launch every step (default 1: folded into the previous step's
 * frame-projection launch through composite weights; same function, rounding differs at the 1e-7 level) */
int taco_debug_set_fuse_prenet(taco_model* m, int on);
/* debug/test: 0 = run the concat projection (rnn_wrappers.py:405-415 + OutputProjectionWrapper, tacotron.py:166-170) as its own
 * launch every step (default 1: folded into the gates launch of the first decoder GRU through composite weights Wc . Wg_x; the
 * same launch emits the projection output for the residual connection; rounding differs at the 1e-7 level) */
int taco_debug_set_fuse_concat(taco_model* m, int on);
/* debug/test: attention launch shape.  -1 (default): one workgroup per batch row, or -- few rows, long inputs (B <= 16, T_in >= 256) --
 * two launches with 4 slices per row; 0: always one workgroup per row; n > 1: always n slices per row */
int taco_debug_set_att_split(taco_model* m, int slices);

/* Decoder loop engine (reference: rnn_wrappers.py:218-341,367-415; helpers.py:9-32).  mode 1 (default): the whole loop runs as ONE
 * persistent, weight-stationary launch (csrc/taco_decoder_xcd.h) whenever the configuration fits it -- reference widths (256-wide
 * cells, prenet 256/128, two decoder GRUs), model_type single or deepvoice, no manual alignments, no teacher forcing, the
 * attention memory slice of a member fits its LDS; every other call uses the launch-per-stage loop.  mode 0: always launch per
 * stage.  mode 2: persistent with write-through (placement-independent) exchanges even when the census finds one group per XCD.
 * rows_per_group: 0 = smallest of 1/2/4/8 that covers the batch with 8 groups; 1, 2, 4 or 8 packs the batch onto fewer XCDs (any other
 * value: TACO_ERR_ARG, nothing changes).  A value that does not fit a call -- fewer than B rows on 8 groups, or below 4 outside the
 * reference widths -- is ignored for that call.  Which kernel a call then gets: decoder_plan (csrc/taco_lib.hip), told by taco_model_engine_plan. */
int taco_debug_set_decoder_persist(taco_model* m, int mode, int rows_per_group);
/* test hook: set the sticky device error word (as a persistent kernel does when its bounded spin expires) to `value` */
int taco_debug_raise_device_error(taco_model* m, int value);
/* after a forward: out16[0] = exchange protocol the last persistent decoder launch used (0 none ran, 1 XCD-local plain stores,
 * 2 write-through), out16[1..8] = workgroups the census saw per XCD, out16[9] = protocol of the persistent BPTT launch when the
 * last decoder backward (training shadow model) used it, else 0, out16[14] = compute units of the device (the whole-chip
 * persistent kernels are used only when there are 256: an unpartitioned MI355X; a CPX / DPX partition runs the launch-per-stage
 * engine), out16[15] = 1 when the model has a persistent-decoder pack */
int taco_debug_decoder_info(taco_model* m, int* out16);
/* phase timeline of group 0 / member 0 for the first 8 decoder steps (scan: steps 8-15): enable bit 0 = launches enqueued from now
 * on write their stamps (the buffer is allocated on first use and lives as long as the model, because captured plans keep its
 * address; drop plans captured under the other setting); out (nullable) receives [8][16] shader-clock stamps of the decoder, or,
 * with enable bit 1, of the post-net scan (its own third of the buffer), or, with bit 2, of the persistent BPTT of a training
 * shadow model (k_decoder_bwd_xcd, steps 8-15 of its launch) */
int taco_debug_decoder_trace(taco_model* m, int enable, long long* out);

/* timing hook: on = 1 leaves the recurrent scan launches of both CBHGs out of every forward / stage call enqueued from now on
 * (their outputs are then meaningless), so that the feed-forward part of a stage can be timed alone (bench.py roofline.stages) */
int taco_debug_set_skip_scans(taco_model* m, int on);

/* A/B hook: on = 0 switches off the per-device ordering of whole-chip kernels across the streams of this process (taco_plan_whole_chip in
 * taco_abi.h); two persistent forwards on different streams then starve each other until their bounded spins report a device fault */
int taco_debug_set_chip_turns(int on);

/* test hook: force the exact-fp32 k_gemm and its tile configuration (1: 64x64, 2: 32x64 split-K; -1: the model's level, automatic choice).
 * Any other value -- the retired configs 0 and 3 included -- is TACO_ERR_ARG and changes nothing. */
int taco_debug_force_gemm_config(taco_model* m, int cfg);

/* tuning hook of k_cbhg_front (csrc/taco_front.h: conv bank -> max-pool -> proj_1 as one launch): the second K half of every workgroup
 * starts `delay_clocks` shader clocks late and runs at s_setprio level `prio` (0..3).  Defaults 0 / 1 (tools/time_front.py).
 * taco_debug_set_bf3 bit 3 (on = 9) switches the fused front off (bank and proj_1 as two k_gemm_bf3 launches). */
int taco_debug_set_front(taco_model* m, int delay_clocks, int prio);

/* Test hook: the post-net BiGRU scan alone -- forward with the gate tape, then backward -- on caller data, ragged lengths and
 * initial states included.  persistent = 1: the whole-chip kernels k_bigru_duo<RG, true> + k_bigru_duo_bwd; 0: k_bigru_res + k_bigru_rows_bwd.
 * d_xproj [B*T, 6H] (hoisted input projection, backward direction time-reversed per row), d_lengths [B] / NULL, d_h0 [B, 2H] / NULL,
 * d_dout [B*T, 2H] -> d_out [B*T, 2H], d_gsave / d_dg [B*T, 6H], d_rh [B*T, 2H], d_dh0 [B, 2H] / NULL; scratch >= 1 MB. */
int taco_train_debug_bigru(taco_train* t, void* hip_stream, const float* d_xproj, const int32_t* d_lengths, const float* d_h0,
                           const float* d_dout, int B, int T, int persistent, float* d_out, float* d_gsave, float* d_dg, float* d_rh,
                           float* d_dh0, void* d_scratch, size_t scratch_bytes);

/* Test hook: ONE CBHG of a trainer alone -- the training forward with its tape (cbhg_forward_train), then its backward (cbhg_backward) -- on caller
 * data, exactly as the step calls them: the step's context and state objects, the tape layout of the step, the trainer's current switches
 * (taco_train_set_exact_gemm, _set_exact_wgrad, _set_wgrad_planes, _set_deterministic, _set_bptt_engine) and the batching region for small weight
 * gradients that the backward opens.  BatchNorm uses batch statistics; the moving statistics in d_params are not touched.
 * which: 0 = encoder CBHG (in_dim = last encoder prenet width, rnn = enc_rnn_size), 1 = post CBHG (in_dim = num_mels, rnn = post_rnn_size).
 * d_in [B*T, in_dim], d_dout [B*T, 2*rnn] -> d_out [B*T, 2*rnn], d_din [B*T, in_dim].  Nullable: d_lengths [B]; d_h0 [B, 2*rnn] (initial states)
 * with d_dh0; d_before [B, in_dim] (the vector added before the highway layers) with d_dbefore; a gradient output without its input is TACO_ERR_ARG.
 * d_params: the trainer's flat parameters, as of the last taco_train_refresh.  The parameter gradients of the scope are ADDED into d_grads at their
 * taco_train_param_offset -- zero-fill the scope first, as the step zero-fills the whole buffer; no other element of d_grads is written.
 * d_ws: at least taco_train_debug_cbhg_workspace_bytes(t, which, B, T) bytes (ask again after a switch that changes the step's workspace),
 * 16-byte aligned; else TACO_ERR_STATE / TACO_ERR_ARG, as the step answers.
 * paths (nullable) receives which branch each dispatch of THIS call took, OR-ed in at the dispatch site where the kernel is launched:
 *   bit  0 / 1   conv bank forward: BatchNorm + max-pool fused (k_bn_pool_bank_v4) / k_bn_apply per width + k_maxpool_fwd
 *   bit  2 / 3   max-pool backward: BatchNorm-fused (k_maxpool_bwd_bn_v4) / k_maxpool_bwd
 *   bit  4 / 5   BatchNorm apply of a projection: k_bn_apply_v4 / k_bn_apply
 *   bit  6 / 7   BatchNorm backward of one layer: k_bn_bwd_v4 / k_bn_bwd (projections; bank widths too when bit 9 is set)
 *   bit  8 / 9   dz of the conv bank: all widths in one launch (k_bn_bwd_bank_v4) / one BatchNorm backward per width
 *   bit 10 / 11  kernel gradients of the conv bank: one product from pre-split planes / one weight gradient per width
 *   bit 12 / 13  highway backward: k_highway_bwd_v4 / k_highway_bwd
 *   bits 16-19   forward scan launched: 1 k_bigru_rows, 2 k_bigru_res, 3 k_bigru_quad, 5 k_bigru_duo, 6 k_bigru_oct (TAPE instantiations)
 *   bits 20-23   backward scan launched: 1 k_bigru_rows_bwd, 2 k_bigru_resb, 3 k_bigru_duo_bwd, 4 k_bigru_oct_bwd
 * Both bits of a pair are set when layers of one call went different ways (e.g. 18- and 16-wide projections).  Bit 13 cannot be reached through a
 * trainer: taco_train_create accepts only rnn sizes that are multiples of 4, and the tape is carved in 256-byte steps. */
size_t taco_train_debug_cbhg_workspace_bytes(const taco_train* t, int which, int B, int T);
int taco_train_debug_cbhg(taco_train* t, void* hip_stream, int which, float* d_params, float* d_grads, const float* d_in, const int32_t* d_lengths,
                          const float* d_h0, const float* d_before, const float* d_dout, int B, int T, float* d_out, float* d_din, float* d_dh0,
                          float* d_dbefore, void* d_ws, size_t ws_bytes, uint32_t* paths);

/* Test hook: the DECODER of a trainer alone -- the teacher-forced training forward with its tape (decoder_forward_train, feed_back = false), then its backward
 * (decoder_backward: the persistent BPTT or the per-stage chain, the hoisted weight gradients, the attention-memory gradients) -- on caller data, exactly as
 * the step calls them: the step's context and state objects, the tape layout of the step (carve_dec_tape), the trainer's current switches
 * (taco_train_set_exact_gemm, _set_exact_wgrad, _set_wgrad_planes, _set_deterministic, _set_bptt_engine; taco_debug_set_decoder_persist on taco_train_model).
 * Inputs: d_enc_out [B*T_in, D] (D = 2 * enc_rnn_size), d_teacher [B, n, num_mels] (the frame fed to step t + 1 is row t), d_dmel [B, n, r*num_mels] (the
 * upstream gradient of d_mel).  Nullable: d_att_init [B, attention_state_size] and d_dec_init (dec_layer_num pointers to [B, dec_rnn_size], each nullable) --
 * model type deepvoice only; d_spk_emb [B, S], the speaker rows -- required by model type 'simple' and refused elsewhere.
 * Outputs: d_mel [B, n, r*num_mels], d_alignments [B, T_in, n], d_denc [B*T_in, D], and the nullable gradient twins d_datt_init, d_ddec_init (an array as
 * d_dec_init), d_dspk_emb [B, S] (required with d_spk_emb; overwritten).  A gradient output without its input is TACO_ERR_ARG.
 * d_params: the trainer's flat parameters, as of the last taco_train_refresh.  The parameter gradients of everything decoder_backward writes (decoder/...,
 * attention/...) are ADDED into d_grads at their taco_train_param_offset -- zero-fill them first, as the step zero-fills the whole buffer; no other element of
 * d_grads is written.
 * d_ws: at least taco_train_debug_decoder_workspace_bytes(t, B, T_in, n) bytes (ask again after a switch that changes the step's workspace), 16-byte aligned.
 * Errors, as the step's and all returned before the first HIP call: misaligned workspace TACO_ERR_ARG, stale split-bf16 planes (a switch without a
 * taco_train_refresh) TACO_ERR_STATE, T_in > 2048 (ATT_MAXT) and attention sizes the training kernels do not serve TACO_ERR_UNSUPPORTED, too small a workspace
 * TACO_ERR_STATE; a host-only trainer (taco_debug_train_create_host) that passes them all TACO_ERR_STATE.
 * paths (nullable) receives which engine each of the two loops ran on, OR-ed in where it is launched:
 *   bit  0 / 1   forward: ONE persistent launch (k_decoder_xcd<RG, true>) / one launch per stage
 *   bit  2 / 3   BPTT: ONE persistent launch (k_decoder_bwd_xcd<RG>) / one launch per stage
 *   bits 4-7     rows per group (1, 2, 4 or 8) of the persistent forward, 0 when it did not run
 *   bits 8-11    rows per group of the persistent BPTT, 0 when it did not run
 *   bit 12 / 13  exchange protocol of each persistent launch of the call: XCD-local plain stores / write-through -- what the census of the launch found
 *                (taco_debug_decoder_info out16[0] and [9]).  To read them the hook waits for the stream when `paths` is given and a persistent launch ran. */
size_t taco_train_debug_decoder_workspace_bytes(const taco_train* t, int B, int T_in, int n);
int taco_train_debug_decoder(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const float* d_enc_out, const float* d_teacher,
                             const float* d_dmel, const float* d_att_init, const float* const* d_dec_init, const float* d_spk_emb, int B, int T_in, int n,
                             float* d_mel, float* d_alignments, float* d_denc, float* d_datt_init, float* const* d_ddec_init, float* d_dspk_emb,
                             void* d_ws, size_t ws_bytes, uint32_t* paths);

/* Test hook: the INPUT END of a trainer's step alone -- embedding gather, encoder prenet and speaker conditioning forward (front_forward_train), then their
 * backward (speaker_rows_backward for model type 'simple', front_backward: the deepvoice speaker layers, the prenet, the embedding's gradient) -- on caller
 * data, exactly as the step calls them: the step's context and state objects, buffers carved as the step carves them, the trainer's current switches
 * (taco_train_set_exact_gemm, _set_exact_wgrad, _set_wgrad_planes, _set_deterministic).
 * Inputs: d_ids [B, T_in] (every id below num_symbols; nothing is masked by a length, as the reference masks nothing in the prenet), d_dpre [B*T_in, P] (P = last
 * encoder prenet width), the upstream gradient of d_pre.  Multi-speaker models: d_speaker_id [B]; deepvoice: d_dvec, 3 + dec_layer_num pointers to the upstream
 * gradients of before_highway [B, P], encoder_rnn_init [B, 2*enc_rnn_size], attention_rnn_init [B, attention_state_size], decoder_rnn_init_i [B, dec_rnn_size];
 * simple: d_dspk_emb [B, S], what the decoder and the linear head hand back for the speaker rows.
 * Outputs: d_pre [B*T_in, P]; deepvoice: d_vec, pointers as d_dvec, the speaker vectors; d_spk_emb [B, S], the gathered speaker rows (required by simple,
 * nullable for deepvoice with S > 1, refused elsewhere).
 * d_params: the trainer's flat parameters, as of the last taco_train_refresh.  The gradients of embedding, prenet/dense_*, speaker_embedding and spk/... are ADDED
 * into d_grads at their taco_train_param_offset -- zero-fill them first, as the step zero-fills the whole buffer; no other element of d_grads is written.
 * d_ws: at least taco_train_debug_front_workspace_bytes(t, B, T_in) bytes (ask again after a switch that changes the step's workspace), 16-byte aligned.
 * Errors, all returned before the first HIP call: a null required argument, speaker_id missing on a multi-speaker model, speaker inputs or outputs on a
 * single-speaker model (or of the other model type), a gradient without its forward output, a misaligned workspace: TACO_ERR_ARG; stale split-bf16 planes (a switch
 * without a taco_train_refresh) and too small a workspace: TACO_ERR_STATE; more than 64 rows: TACO_ERR_UNSUPPORTED; a host-only trainer
 * (taco_debug_train_create_host) that passes them all: TACO_ERR_STATE.
 * paths (nullable) receives which branch each dispatch of THIS call took, OR-ed in where the kernel is launched:
 *   bit 0 / 1   embedding-style gradients (embedding, speaker_embedding, spk tables): k_embed_bwd_det (ordered) / k_embed_bwd (atomics)
 *   bit 2 / 3   deepvoice speaker backward: tables (speaker_embedding_size = 1) / softsign + dense layers into speaker_embedding */
size_t taco_train_debug_front_workspace_bytes(const taco_train* t, int B, int T_in);
int taco_train_debug_front(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const int32_t* d_ids, const int32_t* d_speaker_id,
                           const float* d_dpre, const float* const* d_dvec, const float* d_dspk_emb, int B, int T_in, float* d_pre, float* const* d_vec,
                           float* d_spk_emb, void* d_ws, size_t ws_bytes, uint32_t* paths);

/* Test hook: the OUTPUT END of a trainer's step alone -- the teacher-frame gather (teacher_frames), the linear head and add_loss (head_forward_train:
 * taco_loss_f32), then the two L1 gradients, the head's weight, bias and data gradients (head_backward) and dmel += dmel_post (head_backward_join) -- on caller
 * data, exactly as the step calls them: the step's context and state objects, the trainer's current switches.
 * Inputs: d_post_out [B*T_out, 2*post_rnn_size] (the post CBHG's output), d_mel [B*T_out, num_mels] (the decoder's frames), d_mel_tgt [B, T_out, num_mels],
 * d_lin_tgt [B, T_out, num_freq], prioritize_loss, sample_rate.  Nullable: d_loss_coeff [B]; d_dmel_post [B*T_out, num_mels], what the post CBHG's backward hands
 * back, added to d_dmel as the step adds it; d_spk_emb [B, S], the speaker rows -- required by model type 'simple' and refused elsewhere.
 * Outputs: d_teacher [B, T_out/r, num_mels] (target frame t*r + r-1 of every row), d_lin [B*T_out, num_freq], d_losses[4] (loss, mel_loss, linear_loss,
 * loss_without_coeff), d_dmel [B*T_out, num_mels], d_dpost [B*T_out, 2*post_rnn_size], d_dspk_emb [B, S] (required with d_spk_emb; overwritten: the head's share
 * of the gradient of the speaker rows alone).  A gradient output without its input is TACO_ERR_ARG.
 * The gradients of linear/kernel and linear/bias are ADDED into d_grads at their taco_train_param_offset -- zero-fill them first; no other element is written.
 * d_ws: at least taco_train_debug_head_workspace_bytes(t, B, T_out) bytes, 16-byte aligned.
 * Errors, all returned before the first HIP call: null argument, bad shape, misaligned workspace TACO_ERR_ARG; T_out no multiple of the reduction factor or
 * T_out/r above max_iters TACO_ERR_SHAPE; more than 64 rows TACO_ERR_UNSUPPORTED; stale split-bf16 planes and too small a workspace TACO_ERR_STATE; a host-only
 * trainer that passes them all TACO_ERR_STATE. */
size_t taco_train_debug_head_workspace_bytes(const taco_train* t, int B, int T_out);
int taco_train_debug_head(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const float* d_post_out, const float* d_mel, const float* d_mel_tgt,
                          const float* d_lin_tgt, const float* d_loss_coeff, const float* d_dmel_post, const float* d_spk_emb, int B, int T_out,
                          int prioritize_loss, int sample_rate, float* d_teacher, float* d_lin, float* d_losses, float* d_dmel, float* d_dpost,
                          float* d_dspk_emb, void* d_ws, size_t ws_bytes);

/* Test hook: a trainer that stays on the host -- its shadow model is packed and never uploaded, no device is touched.  It serves the argument and state
 * checks of taco_train_debug_decoder, taco_train_debug_front and taco_train_debug_head, which come before its first HIP call, on a machine without a GPU; nothing may be launched on it (its split-bf16
 * planes count as stale until taco_train_set_exact_gemm with on = 1 selects the engines that need none).  Freed by taco_train_destroy. */
int taco_debug_train_create_host(const taco_hparams* hp, taco_train** out);

/* Test hook: which kernel the training step gives a weight gradient, and how it slices the rows -- wgrad_plan / wgrad_bank_plan of
 * csrc/taco_train.h, pure host functions: no handle, no device.  Inputs: the trainer's switches (wgrad_bf3: 0 = exact-fp32 weight
 * gradients are on; wgrad_planes: the mode of taco_train_set_wgrad_planes), whether the deterministic scratch exists and its floats, the
 * plane scratch in 16-byte units (0: none), whether a batching region is open, and the problem: dW [kw][K][N] summed over M rows (T per
 * batch row, 0: no time axis), left padding padl, whether x / dy rows are gathered.  nw > 0 asks for a whole conv bank instead: widths
 * 1 .. nw of N channels each over a K-wide input (kw, padl, ygather unused).
 * out8: [0] engine (0 cannot run / bank not eligible, 1 pre-split planes, 2 k_wgrad_bf3<4>, 3 k_wgrad_bf3<1> alone, 4 k_wgrad_bf3<1> in the
 * group launch, 5 k_wgrad), [1] rows per slice, [2] slices, [3] planes: x carries the tap copies, [4] planes: padded rows, [5] [6] planes:
 * 16-byte units of the x / dy plane sets, [7] 1 = cannot run (the step fails with TACO_ERR_STATE). */
int taco_debug_wgrad_plan(int wgrad_bf3, int wgrad_planes, int deterministic, long long det_floats, long long planes_uint4, int region_open,
                          int M, int T, int K, int N, int kw, int padl, int gather, int ygather, int nw, int* out8);

/* Test hook: k_spec_targets (the fused back end of taco_spec_targets: magnitude -> dB -> normalise, mel projection) alone on a
 * caller-supplied d_est [R, 2*num_freq] (Re | Im of R frames) -> d_linear [R, num_freq], d_mel [R, num_mels] (nullable).  Lets the
 * dB / normalise arithmetic be held against the reference's own recorded outputs, and the kernel be timed alone. */
int taco_debug_spec_epilogue(taco_gl* g, void* hip_stream, const float* d_est, int R, float* d_linear, float* d_mel);

/* Timing hook: k_pcm_energy, the first launch of taco_pcm_nonsilent and its only pass over the samples, alone: d_energy [B, Mmax]
 * uint64 receives E[b, j] for every j < M_b (include/taco_abi.h).  Arguments and errors as taco_pcm_nonsilent's. */
int taco_debug_pcm_energy(void* hip_stream, const int16_t* d_pcm, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate,
                          uint64_t* d_energy);

/* Test hook: a taco_gl handle of either flavour (tf_flavor != 0: taco_gl_create_tf's) whose packs are built on the host and never
 * uploaded -- no device is touched.  It serves the argument and state checks of the taco_gl_* entry points, which come before their
 * first device call, on a machine without a GPU; nothing may be launched on it.  Freed by taco_gl_destroy. */
int taco_debug_gl_create_host(const taco_audio_hparams* hp, int tf_flavor, taco_gl** out);

/* Test and timing hook: the projection kernel of one Griffin-Lim iteration alone, in the handle's flavour, on caller-supplied
 * d_est, d_prev [R, 2*num_freq] (Re | Im), d_S [R, num_freq] -> d_X [R, 2*num_freq].  d_prev NULL: the plain loop's k_gl_project /
 * k_gl_project_tf (c is not used); else k_gl_project_fast on z = est - c * prev. */
int taco_debug_gl_project(taco_gl* g, void* hip_stream, const float* d_est, const float* d_prev, const float* d_S, float* d_X, float c, int R);

/* Test hooks: the stages of the librosa-flavour Griffin-Lim path alone, on caller data (tests/test_gpu_gl_stages.py against tests/gl_reference.py).
 * Each one launches the kernels the product path launches (gl_vocode_rows, taco_gl_inv_spectrogram_tf, gl_iterate), with its launch shapes.
 * Every argument error is returned before the first HIP call; a host-only handle (taco_debug_gl_create_host) that passes them all is
 * TACO_ERR_STATE.
 *
 * taco_debug_gl_info: the slot geometry of a call with T frames, host only.  The first n (at most 8) values are written: out[0] = Tr, frame
 * rows per utterance slot, [1] = slot, samples per utterance slot, [2] = half = n_fft / 2, [3] = lpad, [4] = floats behind the last slot that
 * the product path clears with the slots (2 * n_fft + win), [5] = floats of the window-sum table (hop * (T - 1) + n_fft), [6] = the fewest
 * frames a row keeps (taco_gl_min_frames; 1 on a taco_gl_create_tf handle), [7] = samples of a row of T frames in the handle's flavour.  A null
 * pointer, n < 0 or T < 1 is TACO_ERR_ARG. */
int taco_debug_gl_info(const taco_gl* g, int T, int* out, int n);
/* k_gl_magnitude, then k_gl_init_phase: d_spec [B, T, num_freq], d_frames [B] / NULL, d_init_uniform [B, T, num_freq] / NULL (then the counter
 * hash of seed) -> d_S [B, Tr, num_freq], d_X [B, Tr, 2 * num_freq].  Frames are clamped as the handle's flavour clamps them (out[6] above). */
int taco_debug_gl_prologue(taco_gl* g, void* hip_stream, const float* d_spec, const int32_t* d_frames, const float* d_init_uniform,
                           unsigned long long seed, int B, int T, float* d_S, float* d_X);
/* The synthesis half of an iteration behind the inverse product: d_ypad [B * slot + out[4]] is cleared as the product path clears it, then
 * k_gl_wss fills d_wss [out[5]] and k_gl_overlap_add turns the frames d_Y [B, Tr, win] into the padded rows; on a taco_gl_create_tf handle
 * k_gl_overlap_add_tf runs instead and d_wss is not used (nullable).  d_frames [B] / NULL.  TACO_ERR_SHAPE where the vocoder answers it
 * (hop * (T - 1) <= n_fft / 2 on a librosa handle). */
int taco_debug_gl_overlap_add(taco_gl* g, void* hip_stream, const float* d_Y, const int32_t* d_frames, int B, int T, float* d_ypad, float* d_wss);
/* k_inv_preemphasis as the vocoder launches it, on rows that start at their slot (slot = L = hop * (T - 1), half = 0) and with the
 * coefficient a passed in: d_x [B, L], d_frames [B] / NULL clamped to [fmin, T] -> d_wav [B, L], d_num_samples [B] / NULL.  No handle: hop = 1
 * gives every L.  1 <= fmin <= T, T >= 2, hop >= 1, hop * (T - 1) within an int, a finite; else TACO_ERR_ARG. */
int taco_debug_gl_inv_preemphasis(void* hip_stream, const float* d_x, const int32_t* d_frames, int fmin, int T, int hop, int B, float a,
                                  float* d_wav, int32_t* d_num_samples);
/* One run_gemm on a pack of the handle, as gl_iterate calls it: which = 0 the forward pack (K = win, N = 2 * num_freq), 1 the inverse pack
 * (K = 2 * num_freq, N = win); exact = 0 the split-bf16 planes the product path uses, 1 the exact-fp32 pack.  Row i of the M rows is
 * d_rows[i * ld .. i * ld + K), so ld < K is the overlapping stride of the loop's forward product; rows_floats is what d_rows holds, and
 * (M - 1) * ld + K beyond it is TACO_ERR_ARG.  d_out [M, N]. */
int taco_debug_gl_dft(taco_gl* g, void* hip_stream, int which, int exact, const float* d_rows, size_t rows_floats, int M, int ld, float* d_out);

/* Test hook: the host half of taco_model_finalize alone -- model_pack_host (csrc/taco_pack.h): every weight pack, the GemmVar table and, on a
 * shadow model, the index lists and backward packs -- with no handle and no device.  shadow = 0: flat_weights holds every tensor of the spec in
 * spec order, TF layout, no padding (the flat layout of taco_train_create); another n_floats is TACO_ERR_SHAPE.  shadow = 1: flat_weights must
 * be NULL; the index-valued weights of a trainer's shadow model are filled in exactly as taco_train_create does, with a TrainPacks attached.
 * out[0] = arena length in floats, out[1] = FNV-1a-64 of the arena bytes, out[2] = FNV-1a-64 of the GemmVar table before pointer resolution
 * (arena offsets + 1 in the pointer fields), out[3] = FNV-1a-64 of bf3_idx followed by bf3_segs (0: both empty), out[4] = which optional packs
 * were built: bit 0 dx_pack, 1 dx_p1o_raw, 2 dx_spkw, 3-6 dx_qpack[0..3], 7 dbx_pack, 8 / 9 gd and go packs of the encoder / post CBHG,
 * 10 / 11 gb and gob packs, 12 / 13 fused-front packs, 14 a wtail, 15 spk_table, 16 spk_dense, 17 att_b, 18 att_sb, 19 gru1_fold,
 * 20 res_g2p packs of either CBHG.  Everything is freed before it returns. */
int taco_debug_pack_host(const taco_hparams* hp, int shadow, const float* flat_weights, size_t n_floats, uint64_t out[5]);

/* Test hook: the work table of taco_segment_norms as its host-only builder makes it (csrc/taco_segnorm.h) -- no handle, no device.  Piece i covers
 * elements [out_begin[i], out_begin[i] + out_len[i]) of segment out_seg[i]; *n_pieces receives their number.  Arguments and errors as
 * taco_segnorm_plan_create's; more than `cap` pieces is TACO_ERR_ARG too (*n_pieces is still set, nothing is written past cap). */
int taco_debug_segnorm_pieces(const uint64_t* h_offsets, int n_seg, const uint8_t* h_skip, uint64_t* out_begin, int32_t* out_len,
                              int32_t* out_seg, int cap, int* n_pieces);
/* Test hook: a taco_segnorm_plan that stays on the host -- no device is touched.  It serves the argument checks of taco_segment_norms,
 * which come before its first device call, on a machine without a GPU; a call that passes them returns TACO_ERR_STATE.  Freed by
 * taco_segnorm_plan_destroy. */
int taco_debug_segnorm_plan_create_host(const uint64_t* h_offsets, int n_seg, const uint8_t* h_skip, taco_segnorm_plan** out);

/* Timing hook: k_sumsq_partial alone, launched exactly as taco_adam_step_f32 launches it (same grid, same workspace of at least 8 KiB): the
 * yardstick that tools/bench_train.py --grad-stats holds taco_train_grad_norms against -- both read the same bytes once. */
int taco_debug_sumsq_partial(void* hip_stream, const float* d_grads, size_t n, void* d_workspace, size_t workspace_bytes);

/* Timing hook: taco_text_matches with the kernel instantiation chosen by the caller.  cols = 0: as taco_text_matches does, one column per lane for
 * len(b) <= 64 and four above; cols = 4: the four-column kernel for every length -- what tools/bench_align.py holds the one-column form against.
 * Arguments, results and errors are taco_text_matches's; another cols is TACO_ERR_ARG. */
int taco_debug_text_matches_cols(void* hip_stream, const int32_t* d_chars, long long n_chars, const int32_t* d_offsets, int n_texts,
                                 const int32_t* d_pairs, int n_pairs, int32_t* d_matches, int cols);

/* Test hook: the sizes at which k_dtw (csrc/taco_dtw.h) changes path, so that tests/test_gpu_dtw.py can sit on either side of each.  The first n (at most 6)
 * values are written, so a caller's buffer sets what it gets: out[0] =
 * columns of a strip (Tb beyond it runs as further strips through the workspace), [1] = rows of A staged at a time, [2] = the largest D,
 * [3] = the step D is rounded up to, [4] = columns of one wave (its last lane hands over through LDS), [5] = rows of the LDS ring (where a
 * row's slot wraps).  Host only; a null pointer or n < 0 is TACO_ERR_ARG. */
int taco_debug_dtw_info(int* out, int n);

/* Test and timing hook: taco_f0_yin with the difference function formed the plain way, one lag per thread walking j over LDS (k_yin<true>,
 * csrc/taco_f0.h), in place of the register-blocked form.  Arguments, results and errors are taco_f0_yin's; on inputs whose sums are exact
 * (include/taco_abi.h) the bits are equal.  Used by tools/bench_f0.py and by one equality test only. */
int taco_debug_f0_yin_plain(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, int sample_rate, int hop, int window,
                            float fmin, float fmax, float threshold, float* d_f0, float* d_aper, int32_t* d_lag);
/* Test hook: the widths at which k_yin changes path, so that tests/test_gpu_f0.py can sit on either side of each.  The first n (at most 7) values
 * are written: out[0] = lanes of a wave (the lags of the finishing pass are dealt over them), [1] = lags of a thread's block, [2] = values of
 * j per register block, [3] = frames of one workgroup (they share one staged span), [4] = threads of a workgroup (lag blocks beyond them are
 * further rounds; below them the j range is cut into parts), [5] = the largest frame (window + tau_max + 2) in floats, [6] = floats of
 * LDS a workgroup may use.  Host only; a null pointer or n < 0 is TACO_ERR_ARG. */
int taco_debug_f0_info(int* out, int n);
/* Test hook: the layout k_yin would run (window, tau_max, hop) with: out[0..4] = lag blocks, parts of the j range, values of j per part,
 * frames per workgroup (fewer than taco_debug_f0_info's [3] where that many frames' span does not fit the LDS), floats of LDS.  Host only;
 * TACO_ERR_ARG for a null pointer, window or hop < 1, tau_max < 2 or a frame above the largest. */
int taco_debug_f0_plan(int window, int tau_max, int hop, int* out);
/* Test hook: the sizes at which k_warp_map and k_spec_warp (csrc/taco_warp.h) change path, so that tests/test_gpu_warp.py can sit on either
 * side of each.  The first n (at most 4) values are written: out[0] = frames of one scan chunk (a row beyond it runs as further chunks with a
 * carry), [1] = lanes of a wave (the shuffle scan inside a chunk; the waves' totals go through LDS), [2] = output rows of one workgroup of
 * k_spec_warp, [3] = the widest row (W) whose frequency gather is staged in LDS; wider rows read the source rows from the cache.  Host
 * only; a null pointer or n < 0 is TACO_ERR_ARG. */
int taco_debug_warp_info(int* out, int n);
/* Test and timing hook: taco_spec_warp with the frequency gather reading the source rows straight from the cache at every width, the form
 * rows wider than taco_debug_warp_info's [3] always take, in place of the row staged in LDS.  Arguments, results and errors are
 * taco_spec_warp's, and so are the bits of d_out. */
int taco_debug_spec_warp_direct(void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src, const int32_t* d_frac,
                                const int32_t* d_out_frames, const float* d_freq_scale, int B, int T, int W, int T_out, float* d_out);
/* Test hook: the tile constants of k_spec_envelope and k_spec_warp_formant (csrc/taco_envelope.h), so that tests/test_gpu_envelope.py can
 * sit on either side of each.  The first n (at most 8) values are written: out[0] = frames of one workgroup, [1] = lanes of a wave, [2] = the
 * edge of the matrix tile (v_mfma_f32_16x16x4_f32: 16 frames by 16 coefficients or bins; W and Q are rounded up to it), [3] = terms of the
 * sum one matrix instruction takes, [4] = the widest frame (W) the kernels serve, [5] = the widest frame a workgroup takes out[0] of --
 * wider ones get [6] frames a workgroup --, [7] = the largest Q.  Host only; a null pointer or n < 0 is TACO_ERR_ARG. */
int taco_debug_envelope_info(int* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* TACO_DEBUG_H */
