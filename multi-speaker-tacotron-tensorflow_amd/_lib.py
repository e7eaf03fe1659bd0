"""ctypes binding of libtaco_hip.so (include/taco_abi.h; the test / timing hooks of include/taco_debug.h).  There is NO fallback: if the HIP library
is missing or fails to load, importing the compute path raises."""
import ctypes as C
import os

from .hparams import MODEL_TYPES, ATTENTION_TYPES, NUM_SYMBOLS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libtaco_hip.so")

TACO_ERR_ARG, TACO_ERR_SHAPE, TACO_ERR_UNSUPPORTED, TACO_ERR_HIP, TACO_ERR_STATE = -1, -2, -3, -4, -5
TACO_TRIM_SPECTRAL, TACO_TRIM_TIME = 0, 1      # taco_wav_trim's `energy`
TACO_WAV_F32, TACO_WAV_PCM16 = 0, 1            # taco_wav_resample's `in_format`


class TacoHParams(C.Structure):
    _fields_ = [
        ("num_symbols", C.c_int32), ("num_mels", C.c_int32), ("num_freq", C.c_int32),
        ("num_speakers", C.c_int32), ("model_type", C.c_int32), ("speaker_embedding_size", C.c_int32),
        ("embedding_size", C.c_int32),
        ("enc_prenet_n", C.c_int32), ("enc_prenet", C.c_int32 * 4),
        ("enc_bank_size", C.c_int32), ("enc_bank_channels", C.c_int32), ("enc_maxpool", C.c_int32),
        ("enc_highway_depth", C.c_int32), ("enc_rnn_size", C.c_int32),
        ("enc_proj_n", C.c_int32), ("enc_proj", C.c_int32 * 4), ("enc_proj_width", C.c_int32),
        ("attention_type", C.c_int32), ("attention_size", C.c_int32), ("attention_state_size", C.c_int32),
        ("dec_layer_num", C.c_int32), ("dec_rnn_size", C.c_int32),
        ("dec_prenet_n", C.c_int32), ("dec_prenet", C.c_int32 * 4),
        ("post_bank_size", C.c_int32), ("post_bank_channels", C.c_int32), ("post_maxpool", C.c_int32),
        ("post_highway_depth", C.c_int32), ("post_rnn_size", C.c_int32),
        ("post_proj_n", C.c_int32), ("post_proj", C.c_int32 * 4), ("post_proj_width", C.c_int32),
        ("reduction_factor", C.c_int32), ("max_iters", C.c_int32),
    ]


class TacoAudioHParams(C.Structure):
    _fields_ = [("num_freq", C.c_int32), ("sample_rate", C.c_int32), ("griffin_lim_iters", C.c_int32),
                ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float), ("preemphasis", C.c_float),
                ("min_level_db", C.c_float), ("ref_level_db", C.c_float), ("power", C.c_float)]


class TacoCollateStream(C.Structure):
    """taco_collate_stream (include/taco_abi.h): one field of a batch, gathered out of a device pack."""
    _fields_ = [("pack", C.c_void_p), ("start", C.c_void_p), ("rows", C.c_void_p), ("width", C.c_int32), ("rows_out", C.c_int32),
                ("out", C.c_void_p), ("counts", C.c_void_p)]


TACO_COLLATE_MAX_STREAMS = 8


class TacoError(Exception):
    """Raised for every non-zero return of the C ABI.  The reference raises bare `Exception`
    for unknown model/attention types and shape mismatches (tacotron.py:88,152,192-194)."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _list4(vals, what):
    vals = list(vals)
    if not 1 <= len(vals) <= 4:
        raise TacoError(TACO_ERR_ARG, "%s must have 1..4 entries, got %d" % (what, len(vals)))
    arr = (C.c_int32 * 4)(*(vals + [0] * (4 - len(vals))))
    return len(vals), arr


def to_c_hparams(hp, num_speakers):
    """HParams (reference key names) -> taco_hparams POD."""
    if hp.model_type not in MODEL_TYPES:
        raise Exception(" [!] Unkown multi-speaker model type: {}".format(hp.model_type))   # tacotron.py:88
    if hp.attention_type not in ATTENTION_TYPES:
        raise Exception(" [!] Unkown attention type: {}".format(hp.attention_type))         # tacotron.py:152
    c = TacoHParams()
    c.num_symbols = getattr(hp, "num_symbols", NUM_SYMBOLS)
    c.num_mels, c.num_freq = hp.num_mels, hp.num_freq
    c.num_speakers = int(num_speakers)
    c.model_type = MODEL_TYPES[hp.model_type]
    c.speaker_embedding_size = hp.speaker_embedding_size
    c.embedding_size = hp.embedding_size
    c.enc_prenet_n, c.enc_prenet = _list4(hp.enc_prenet_sizes, "enc_prenet_sizes")
    c.enc_bank_size, c.enc_bank_channels = hp.enc_bank_size, hp.enc_bank_channel_size
    c.enc_maxpool, c.enc_highway_depth, c.enc_rnn_size = hp.enc_maxpool_width, hp.enc_highway_depth, hp.enc_rnn_size
    c.enc_proj_n, c.enc_proj = _list4(hp.enc_proj_sizes, "enc_proj_sizes")
    c.enc_proj_width = hp.enc_proj_width
    c.attention_type = ATTENTION_TYPES[hp.attention_type]
    c.attention_size, c.attention_state_size = hp.attention_size, hp.attention_state_size
    c.dec_layer_num, c.dec_rnn_size = hp.dec_layer_num, hp.dec_rnn_size
    c.dec_prenet_n, c.dec_prenet = _list4(hp.dec_prenet_sizes, "dec_prenet_sizes")
    c.post_bank_size, c.post_bank_channels = hp.post_bank_size, hp.post_bank_channel_size
    c.post_maxpool, c.post_highway_depth, c.post_rnn_size = hp.post_maxpool_width, hp.post_highway_depth, hp.post_rnn_size
    c.post_proj_n, c.post_proj = _list4(hp.post_proj_sizes, "post_proj_sizes")
    c.post_proj_width = hp.post_proj_width
    c.reduction_factor, c.max_iters = hp.reduction_factor, hp.max_iters
    return c


_P = C.c_void_p
_I = C.c_int
_S = C.c_size_t
# taco_sync_sum_fn (include/taco_abi.h): void (*)(void* user, float* d_vec, int n)
SYNC_SUM_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)

# name -> (restype, argtypes); every symbol declared in include/taco_abi.h
PROTOTYPES = {
    "taco_abi_version": (_I, []),
    "taco_last_error": (C.c_char_p, []),
    "taco_model_create": (_I, [C.POINTER(TacoHParams), _I, C.POINTER(_P)]),
    "taco_model_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "taco_model_num_weights": (_I, [_P]),
    "taco_model_weight_name": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_int64), C.POINTER(_I)]),
    "taco_model_finalize": (_I, [_P]),
    "taco_model_destroy": (None, [_P]),
    "taco_workspace_bytes": (_S, [_P, _I, _I, _I]),
    "taco_stage_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_forward_infer": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _S]),
    "taco_forward_infer_mix": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _S]),
    "taco_plan_create": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _S, C.POINTER(_P)]),
    "taco_plan_create_mix": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _S, C.POINTER(_P)]),
    "taco_plan_launch": (_I, [_P, _P]),
    "taco_plan_num_nodes": (_I, [_P]),
    "taco_plan_whole_chip": (_I, [_P]),
    "taco_plan_destroy": (None, [_P]),
    "taco_encoder_forward": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _S]),
    "taco_encoder_forward_mix": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _S]),
    "taco_decoder_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _S]),
    "taco_decoder_forward_mix": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _S]),
    "taco_postnet_forward": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _S]),
    "taco_postnet_forward_mix": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _S]),
    "taco_conv1d_bn_f32": (_I, [_P, _P, C.c_char_p, _P, _I, _I, _I, _I, _P]),
    "taco_dense_f32": (_I, [_P, _P, C.c_char_p, _P, _I, _I, _P]),
    "taco_highway_f32": (_I, [_P, _P, C.c_char_p, _P, _I, _P]),
    "taco_bigru_f32": (_I, [_P, _P, C.c_char_p, _P, _P, _P, _I, _I, _P, _P, _S]),
    "taco_attention_step_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _S]),
    "taco_gru_cell_f32": (_I, [_P, _P, C.c_char_p, _P, _P, _I, _P, _P, _S]),
    "taco_gl_create": (_I, [C.POINTER(TacoAudioHParams), _I, C.POINTER(_P)]),
    "taco_gl_destroy": (None, [_P]),
    "taco_gl_num_samples": (_I, [_P, _I]),
    "taco_gl_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_gl_inv_spectrogram": (_I, [_P, _P, _P, _P, C.c_ulonglong, _I, _I, _I, _P, _P, _S]),
    "taco_gl_min_frames": (_I, [_P]),
    "taco_gl_rows_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_gl_inv_spectrogram_rows": (_I, [_P, _P, _P, _P, _P, C.c_ulonglong, _I, _I, _I, _P, _P, _P, _S]),
    "taco_wav_to_pcm16": (_I, [_P, _P, _P, _I, _I, _P]),
    "taco_gl_create_tf": (_I, [C.POINTER(TacoAudioHParams), _I, C.POINTER(_P)]),
    "taco_gl_tf_num_samples": (_I, [_P, _I]),
    "taco_gl_tf_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_gl_inv_spectrogram_tf": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _S]),
    "taco_gl_set_inv_mel_basis": (_I, [_P, _P, _I]),
    "taco_gl_mel_to_linear": (_I, [_P, _P, _P, _I, _I, _P]),
    "taco_gl_inv_melspectrogram_rows": (_I, [_P, _P, _P, _P, _P, C.c_ulonglong, _I, _I, _I, _P, _P, _P, _S]),
    "taco_debug_gl_create_host": (_I, [C.POINTER(TacoAudioHParams), _I, C.POINTER(_P)]),
    "taco_gl_set_momentum": (_I, [_P, C.c_float]),
    "taco_gl_momentum": (C.c_float, [_P]),
    "taco_gl_convergence_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_gl_convergence": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _S]),
    "taco_debug_gl_project": (_I, [_P, _P, _P, _P, _P, _P, C.c_float, _I]),
    "taco_debug_gl_info": (_I, [_P, _I, C.POINTER(_I), _I]),
    "taco_debug_gl_prologue": (_I, [_P, _P, _P, _P, _P, C.c_ulonglong, _I, _I, _P, _P]),
    "taco_debug_gl_overlap_add": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "taco_debug_gl_inv_preemphasis": (_I, [_P, _P, _P, _I, _I, _I, _I, C.c_float, _P, _P]),
    "taco_debug_gl_dft": (_I, [_P, _P, _I, _I, _P, _S, _I, _I, _P]),
    "taco_wav_trim_workspace_bytes": (_S, [_I, _I, _I, _I]),
    "taco_wav_trim": (_I, [_P, _P, _P, _I, _I, C.c_float, _I, _I, _I, _P, _P, _P, _S]),
    "taco_wav_split_workspace_bytes": (_S, [_I, _I, _I, _I]),
    "taco_wav_split": (_I, [_P, _P, _P, _I, _I, C.c_float, _I, _I, _I, _I, _P, _P, _P, _P, _S]),
    "taco_wav_breath_mute": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, C.c_float, _P, _P, _P]),
    "taco_pcm_rate_supported": (_I, [_I]),
    "taco_pcm_nonsilent_workspace_bytes": (_S, [_I, _I, _I]),
    "taco_pcm_nonsilent": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _S]),
    "taco_pcm_range_sumsq": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P]),
    "taco_pcm_apply_gains": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P]),
    "taco_resample_create": (_I, [_I, _I, _P, _I, _I, _I, C.POINTER(_P)]),
    "taco_resample_destroy": (None, [_P]),
    "taco_resample_out_len": (_I, [_P, _I]),
    "taco_resample_computed_len": (_I, [_P, _I]),
    "taco_resample_phases": (_I, [_P]),
    "taco_resample_taps": (_I, [_P]),
    "taco_resample_left_taps": (_I, [_P]),
    "taco_resample_tile": (_I, [_P]),
    "taco_resample_bank": (_I, [_P, _P]),
    "taco_wav_resample": (_I, [_P, _P, _P, _I, _I, _P, _I, _I, _P, _I, _P]),
    "taco_gl_set_mel_basis": (_I, [_P, _P, _I]),
    "taco_spec_num_mels": (_I, [_P]),
    "taco_spec_num_frames": (_I, [C.POINTER(TacoAudioHParams), _I]),
    "taco_spec_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_spec_targets": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _S]),
    "taco_collate": (_I, [_P, C.POINTER(TacoCollateStream), _I, _P, _I, _I]),
    "taco_debug_pcm_energy": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "taco_debug_spec_epilogue": (_I, [_P, _P, _P, _I, _P, _P]),
    "taco_attention_trim": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "taco_manual_alignments": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "taco_loss_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _S]),
    "taco_learning_rate": (C.c_float, [C.c_longlong, C.c_float, _I, _I]),
    "taco_adam_step_f32": (_I, [_P, _P, _P, _P, _P, _S, C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _S]),
    "taco_segment_norms": (_I, [_P, _P, _P, _S, _P, _P, _P]),
    "taco_segnorm_piece_floats": (_I, []),
    "taco_segnorm_plan_create": (_I, [C.POINTER(C.c_uint64), _I, C.POINTER(C.c_uint8), _I, C.POINTER(_P)]),
    "taco_segnorm_plan_destroy": (None, [_P]),
    "taco_train_grad_norms": (_I, [_P, _P, _P, _P, _P, _P]),
    "taco_debug_segnorm_pieces": (_I, [C.POINTER(C.c_uint64), _I, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), _I, C.POINTER(_I)]),
    "taco_debug_segnorm_plan_create_host": (_I, [C.POINTER(C.c_uint64), _I, C.POINTER(C.c_uint8), C.POINTER(_P)]),
    "taco_debug_sumsq_partial": (_I, [_P, _P, _S, _P, _S]),
    "taco_train_create": (_I, [C.POINTER(TacoHParams), _I, C.POINTER(_P)]),
    "taco_train_destroy": (None, [_P]),
    "taco_train_model": (_P, [_P]),
    "taco_train_num_params": (_S, [_P]),
    "taco_train_param_offset": (_I, [_P, C.c_char_p, C.POINTER(_S)]),
    "taco_train_refresh": (_I, [_P, _P, _P]),
    "taco_train_set_sync_bn": (_I, [_P, _P, _P, _I]),
    "taco_train_set_deterministic": (_I, [_P, _I]),
    "taco_train_set_exact_wgrad": (_I, [_P, _I]),
    "taco_train_set_wgrad_planes": (_I, [_P, _I]),
    "taco_train_planes_problems": (_I, [_P]),
    "taco_train_set_bptt_engine": (_I, [_P, _I]),
    "taco_train_set_exact_gemm": (_I, [_P, _I]),
    "taco_debug_wgrad_plan": (_I, [_I, _I, _I, C.c_longlong, C.c_longlong, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "taco_debug_pack_host": (_I, [C.POINTER(TacoHParams), _I, _P, _S, C.POINTER(C.c_uint64)]),
    "taco_train_debug_bigru": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _S]),
    "taco_train_debug_cbhg_workspace_bytes": (_S, [_P, _I, _I, _I]),
    "taco_train_debug_cbhg": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _S, _P]),
    "taco_train_debug_decoder_workspace_bytes": (_S, [_P, _I, _I, _I]),
    "taco_train_debug_decoder": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _S, _P]),
    "taco_train_debug_front_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_train_debug_front": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _S, _P]),
    "taco_train_debug_head_workspace_bytes": (_S, [_P, _I, _I]),
    "taco_train_debug_head": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _S]),
    "taco_debug_train_create_host": (_I, [C.POINTER(TacoHParams), C.POINTER(_P)]),
    "taco_train_workspace_bytes": (_S, [_P, _I, _I, _I]),
    "taco_train_forward_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _S]),
    "taco_debug_force_gemm_config": (_I, [_P, _I]),
    "taco_debug_set_skip_scans": (_I, [_P, _I]),
    "taco_debug_set_chip_turns": (_I, [_I]),
    "taco_debug_set_front": (_I, [_P, _I, _I]),
    "taco_debug_set_persistent": (_I, [_P, _I]),
    "taco_debug_set_overlap": (_I, [_P, _I]),
    "taco_stop_steps": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "taco_debug_set_fuse_prenet": (_I, [_P, _I]),
    "taco_debug_set_fuse_concat": (_I, [_P, _I]),
    "taco_debug_set_att_split": (_I, [_P, _I]),
    "taco_debug_set_bf3": (_I, [_P, _I, _I]),
    "taco_model_device_errors": (_I, [_P, C.POINTER(_I)]),
    "taco_debug_raise_device_error": (_I, [_P, _I]),
    "taco_debug_set_decoder_persist": (_I, [_P, _I, _I]),
    "taco_debug_decoder_info": (_I, [_P, C.POINTER(_I)]),
    "taco_model_engine_plan": (_I, [_P, _I, _I, _I, _I, C.c_char_p, _I]),
    "taco_model_set_batch_invariant": (_I, [_P, _I]),
    "taco_debug_decoder_trace": (_I, [_P, _I, C.POINTER(C.c_longlong)]),
    "taco_text_matches": (_I, [_P, _P, C.c_longlong, _P, _I, _P, _I, _P]),
    "taco_text_best_two": (_I, [_P, _P, _P, _P, _I, _P, _I, _P]),
    "taco_debug_text_matches_cols": (_I, [_P, _P, C.c_longlong, _P, _I, _P, _I, _P, _I]),
    "taco_dtw_workspace_bytes": (_S, [_I, _I, _I, _I]),
    "taco_dtw": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _S]),
    "taco_dtw_path": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "taco_debug_dtw_info": (_I, [C.POINTER(_I), _I]),
    "taco_f0_yin": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
    "taco_f0_path_stats": (_I, [_P, _P, _I, _P, _I, _P, _P, _I, _I, _P]),
    "taco_debug_f0_yin_plain": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
    "taco_debug_f0_info": (_I, [C.POINTER(_I), _I]),
    "taco_debug_f0_plan": (_I, [_I, _I, _I, C.POINTER(_I)]),
    "taco_spec_warp_workspace_bytes": (_S, [_I, _I]),
    "taco_spec_warp_map": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _S]),
    "taco_spec_warp": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "taco_debug_warp_info": (_I, [C.POINTER(_I), _I]),
    "taco_debug_spec_warp_direct": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "taco_envelope_create": (_I, [_I, _I, _P, _P, _I, C.POINTER(_P)]),
    "taco_envelope_destroy": (None, [_P]),
    "taco_envelope_width": (_I, [_P]),
    "taco_envelope_order": (_I, [_P]),
    "taco_envelope_tables": (_I, [_P, _P, _P]),
    "taco_spec_envelope": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "taco_spec_warp_formant": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "taco_debug_envelope_info": (_I, [C.POINTER(_I), _I]),
}

_lib = None


def load_library(path=None):
    """Load libtaco_hip.so and bind every symbol of the header.  Raises if anything is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("TACO_LIB") or LIB_PATH      # TACO_LIB: an instrumented build (tools/trace_*.py, -DTACO_TRACE)
    if path is None and os.environ.get("TACO_LIB") and os.path.abspath(p) != os.path.abspath(LIB_PATH):
        import warnings
        warnings.warn("TACO_LIB overrides the library: loading %s instead of %s" % (p, LIB_PATH), RuntimeWarning, stacklevel=2)
    if not os.path.exists(p):
        raise ImportError(
            "libtaco_hip.so not found at %s -- build it first (python -c 'import __graft_entry__ as g; g.build()' "
            "or multi-speaker-tacotron-tensorflow_amd/csrc/build.sh).  There is no CPU fallback." % p)
    lib = C.CDLL(p)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.taco_abi_version() != 1:
        raise ImportError("libtaco_hip.so ABI version %d, expected 1" % lib.taco_abi_version())
    if path is None:
        _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load_library().taco_last_error().decode("utf-8", "replace")
        if rc == TACO_ERR_UNSUPPORTED and msg.startswith(" [!]"):
            raise Exception(msg)     # same text and type as the reference (tacotron.py:88,152)
        raise TacoError(rc, "libtaco_hip error %d: %s" % (rc, msg))
