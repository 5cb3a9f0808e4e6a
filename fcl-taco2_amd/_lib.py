"""ctypes binding of libfcl_hip.so (include/fcl_hip.h).  Fails loudly when the library is missing.

This is the only place the package touches the shared library.  There is no CPU fallback: if the HIP
extension cannot be loaded, importing any compute entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FCL_LIB") or os.path.join(_HERE, "libfcl_hip.so")  # (FCL_LIB: developer A/B builds of the same ABI)

# name -> (restype, argtypes); mirrors include/fcl_hip.h one to one
_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_Z = C.c_size_t


class DecoderWeights(C.Structure):
    _fields_ = [("c", _I), ("p", _I), ("u", _I), ("odim", _I)] + [
        (n, _P) for n in ("prenet_w0", "prenet_b0", "prenet_w1", "prenet_b1", "w0_att", "w0_pre", "w0_pos", "w0_hh", "b0",
                          "w1_ih", "w1_hh", "b1", "wf_h", "wf_att")
    ] + [("zoneout_rate", _F), ("prenet_dropout", _F)] + [
        (n + sfx, _P) for n in ("prenet_w0", "prenet_w1", "w0_pre", "w0_hh", "w1_ih", "w1_hh", "wf_h") for sfx in ("_hi", "_lo")] + [
        (n + "_p", _P) for n in ("w0_att", "wf_att", "w0_pre", "w0_hh", "w1_ih", "w1_hh")] + [("out_act", _I), ("wf_h_ff", _P), ("prenet_w0_ff", _P), ("prenet_w1_ff", _P),
                                                                                           ("w0_pre_ff", _P), ("w0_hh_ff", _P), ("w1_ih_ff", _P), ("w1_hh_ff", _P), ("stream", _P),
                                                                                           ("prenet_layers", _I), ("dlayers", _I), ("prenet_w2", _P), ("prenet_b2", _P), ("w2_ih", _P),
                                                                                           ("w2_hh", _P), ("b2", _P), ("reduction_factor", _I)]


class DecoderIO(C.Structure):
    _fields_ = [("n", _I), ("lmax", _I), ("att_c", _P), ("dur", _P), ("live_rows_host", _P), ("frame_off", _P),
                ("teacher_ys", _P), ("dropout_mode", _I), ("prenet_keep", _P), ("seed", C.c_uint32), ("seed_dev", _P), ("before", _P),
                ("tap_prenet", _P), ("tap_lstm0", _P), ("tap_lstm1", _P), ("workspace", _P), ("workspace_bytes", _Z), ("att_c_p", _P), ("before_p", _P),
                ("live_rows", _P), ("status", _P), ("tail_from", _I)]


class RowMaps(C.Structure):  # fcl_row_maps_t
    _fields_ = [("b", _I), ("n", _I), ("lmax_cap", _I), ("frames_cap", _I), ("t_max", _I)] + [
        (n, _P) for n in ("row_src", "utt_row0", "pad", "dur_i64", "dur_i32", "src_rows", "dur_sorted", "frame_off", "order", "live_rows", "utt_frame0",
                          "frame_lo", "frame_hi", "totals", "status", "scratch")]


class GemmTerm(C.Structure):
    _fields_ = [("A", _P), ("W", _P), ("lda", _I), ("ldw", _I), ("K", _I), ("shift", _I), ("Whi", _P), ("Wlo", _P), ("Ap", _P), ("Wp", _P),
                ("lda_p", _I), ("ldw_p", _I), ("a_chunk_stride", C.c_int64), ("Wff", _P)]


class LstmStep(C.Structure):
    _fields_ = [("term", GemmTerm * 3), ("nterms", _I), ("M", _I), ("U", _I), ("G", _P), ("g_row_mul", C.c_longlong), ("g_row_add", C.c_longlong),
                ("bias", _P), ("rank1_w", _P), ("dur", _P), ("step", _I), ("h_in", _P), ("h_out", _P), ("c", _P), ("zoneout", _F),
                ("zone_keep_h", _P), ("zone_keep_c", _P), ("row_len", _P), ("out2", _P), ("out2_row_base", _P), ("out2_row_mul", C.c_longlong),
                ("out2_row_add", C.c_longlong), ("ld2", _I), ("out2_col_off", _I), ("h_out_p", _P), ("ld_hp", _I), ("save_gates", _P), ("save_c_new", _P), ("save_c_old", _P),
                ("save_h_old", _P), ("m_dev", _P)]


class DecoderTrain(C.Structure):  # fcl_decoder_train_t
    _fields_ = [("n", _I), ("lmax", _I), ("u", _I), ("p", _I), ("live_rows_host", _P), ("p1d", _P), ("g0", _P), ("w0_pre", _P), ("w0_hh", _P),
                ("w0_pos", _P), ("dur", _P), ("w1_ih", _P), ("w1_hh", _P), ("b1", _P), ("zoneout", _F), ("zk_h0", _P), ("zk_c0", _P), ("zk_h1", _P),
                ("zk_c1", _P), ("s0", _P * 4), ("s1", _P * 4), ("h0_all", _P), ("h1_all", _P), ("workspace", _P), ("workspace_bytes", _Z),
                ("p1d_p", _P), ("w0_pre_p", _P), ("w0_hh_p", _P), ("w1_ih_p", _P), ("w1_hh_p", _P)]


class DecoderBptt(C.Structure):  # fcl_decoder_bptt_t
    _fields_ = [("n", _I), ("lmax", _I), ("u", _I), ("live_rows_host", _P), ("s0", _P * 3), ("s1", _P * 3), ("zoneout", _F), ("zk_h0", _P),
                ("zk_c0", _P), ("zk_h1", _P), ("zk_c1", _P), ("dh1_all", _P), ("dh0_all", _P), ("w1_ih_t", _P), ("w1_hh_t", _P), ("w0_hh_t", _P),
                ("dg0_all", _P), ("dg1_all", _P), ("workspace", _P), ("workspace_bytes", _Z), ("w1_ih_t_p", _P), ("w1_hh_t_p", _P), ("w0_hh_t_p", _P),
                ("dg0_all_p", _P), ("dg1_all_p", _P), ("w1_cat_t", _P), ("w1_cat_t_p", _P)]


class BilstmTrain(C.Structure):  # fcl_bilstm_train_t
    _fields_ = [("b", _I), ("t", _I), ("h", _I), ("lens", _P), ("gx", _P * 2), ("w_hh", _P * 2), ("out", _P), ("s", (_P * 4) * 2), ("workspace", _P),
                ("workspace_bytes", _Z), ("status", _P)]


class BilstmBptt(C.Structure):  # fcl_bilstm_bptt_t
    _fields_ = [("b", _I), ("t", _I), ("h", _I), ("lens", _P), ("s", (_P * 3) * 2), ("d_out", _P), ("ld_dout", _I), ("w_hh_t", _P * 2), ("dg", _P * 2),
                ("workspace", _P), ("workspace_bytes", _Z), ("status", _P)]


GEMM_F32, GEMM_BF16 = 0, 1


class Derive(C.Structure):  # fcl_derive_t
    _fields_ = [("src", _P), ("src2", _P), ("dst", _P), ("dst_p", _P), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("sa", C.c_int32),
                ("sb", C.c_int32), ("sc", C.c_int32), ("first_block", C.c_int32), ("reserved", C.c_int32)]


ABI_VERSION = 423  # FCL_ABI_VERSION of include/fcl_hip.h


class PwgLayer(C.Structure):  # fcl_pwg_layer_t
    _fields_ = [("m", C.c_int64), ("r", C.c_int32), ("aux", C.c_int32), ("ksize", C.c_int32), ("dilation", C.c_int32), ("first_layer", C.c_int32)] + [
        (n, _P) for n in ("seg_lo", "seg_hi", "x", "xp", "cp", "w_conv_p", "b_conv", "w_aux_p", "w_os_p", "b_os", "skips", "z", "gp", "o", "xp_out",
                          "kp", "pt_a", "pt_b")] + [("ld_pt", C.c_int32), ("hop", C.c_int32)]


class HfgConv(C.Structure):  # fcl_hfg_conv_t
    _fields_ = [("m", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "ksize", "dilation", "rate")] + [("slope", _F)] + [
        (n, _P) for n in ("xp", "wp", "bias", "frame_utt", "utt_off", "resid", "y", "yp")]


class HfgTconv(C.Structure):  # fcl_hfg_tconv_t
    _fields_ = [("m_in", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "stride", "ksize", "padding", "rate_in")] + [
        ("slope", _F), ("reserved", C.c_int32)] + [(n, _P) for n in ("xp", "wp", "bias", "frame_utt", "utt_off", "y", "yp")]


class HfgUnit(C.Structure):  # fcl_hfg_unit_t
    _fields_ = [("m", C.c_int64)] + [(n, C.c_int32) for n in ("c", "ksize", "dilation", "rate", "first", "last")] + [
        ("slope", _F), ("cs_scale", _F), ("csp_slope", _F), ("reserved", C.c_int32)] + [
        (n, _P) for n in ("xp", "x", "w1p", "b1", "w2p", "b2", "frame_utt", "utt_off", "x_out", "xp_out", "cs", "csp", "tp")]


class GriffinLim(C.Structure):  # fcl_gl_t
    _fields_ = [("frames", C.c_int64), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_utt", C.c_int32), ("momentum", _F)] + [
        (n, _P) for n in ("window", "twiddle", "frame_utt", "utt_off", "utt_seed", "s", "p", "fr", "y", "c_prev", "c_out", "u_out")]


class Features(C.Structure):  # fcl_fx_t
    _fields_ = [("frames", C.c_int64), ("samples", C.c_int64)] + [(n, C.c_int32) for n in ("n_fft", "hop", "n_utt", "n_mels", "nnz", "reserved")] + [
        (n, _P) for n in ("x", "smp_off", "frame_utt", "utt_off", "window", "twiddle", "fb_lo", "fb_off", "fb_w", "mel_stats", "mel", "energy", "mag_out")]


class Pitch(C.Structure):  # fcl_px_t
    _fields_ = [("frames", C.c_int64), ("samples", C.c_int64)] + [(n, C.c_int32) for n in ("n", "hop", "n_utt", "tau_min", "tau_max", "reserved")] + [
        ("fs", _F), ("threshold", _F)] + [(n, _P) for n in ("x", "smp_off", "frame_utt", "utt_off", "f0", "cmnd_out", "tau_out")]


class Pyin(C.Structure):  # fcl_pyin_t
    _fields_ = [("frames", C.c_int64)] + [(n, C.c_int32) for n in ("n_utt", "n_lag", "tau_min", "tau_max", "nb", "w")] + [("fs", _F), ("reserved", C.c_int32)] + [
        (n, _P) for n in ("cmnd", "thr", "cw", "edge", "f_bin", "tri", "la", "utt_off", "lv", "lu", "bf0", "ov_out", "workspace")] + [("workspace_bytes", _Z)] + [
        (n, _P) for n in ("state", "f0", "score")]


class Resample(C.Structure):  # fcl_rs_t
    _fields_ = [("samples_in", C.c_int64), ("samples_out", C.c_int64)] + [(n, C.c_int32) for n in ("l", "m", "k", "n_utt", "max_out", "reserved")] + [
        (n, _P) for n in ("x", "smp_off_in", "smp_off_out", "table", "y")]


class Evaluate(C.Structure):  # fcl_ev_t
    _fields_ = [(n, C.c_int64) for n in ("frames_a", "frames_b", "cells", "path_rows")] + [(n, C.c_int32) for n in ("n_pairs", "d", "max_ta", "max_tb")] + [
        (n, _P) for n in ("a", "b", "a_off", "b_off", "cell_off", "path_off", "workspace")] + [("workspace_bytes", _Z)] + [
        (n, _P) for n in ("path", "path_len", "cost", "pitch_a", "pitch_b", "counts", "sums")]


class Align(C.Structure):  # fcl_al_t
    _fields_ = [(n, C.c_int64) for n in ("frames", "rows", "cells")] + [(n, C.c_int32) for n in ("n_utt", "n_states", "max_t", "max_s", "max_skip", "reserved")] + [
        (n, _P) for n in ("ll", "frame_off", "row_off", "cell_off", "row_state", "row_skip", "workspace")] + [("workspace_bytes", _Z)] + [
        (n, _P) for n in ("frame_row", "row_begin", "row_frames", "score", "ok")]


class AlignLattice(C.Structure):  # fcl_al_lattice_t
    _fields_ = [(n, C.c_int64) for n in ("frames", "rows", "cells")] + [(n, C.c_int32) for n in ("n_utt", "n_states", "max_t", "max_s")] + [
        (n, _P) for n in ("ll", "frame_off", "row_off", "cell_off", "row_state", "row_pred", "row_flags", "workspace")] + [("workspace_bytes", _Z)] + [
        (n, _P) for n in ("frame_row", "row_begin", "row_frames", "score", "ok")]


class StftLoss(C.Structure):  # fcl_stl_t
    _fields_ = [("frames", C.c_int64), ("samples", C.c_int64)] + [(n, C.c_int32) for n in ("n_fft", "hop", "n_utt", "accumulate")] + [
        (n, _P) for n in ("x", "y", "smp_off", "frame_utt", "utt_off", "window", "twiddle", "frame_sums", "utt_sums", "coef", "fr", "gx")]


class MelLoss(C.Structure):  # fcl_msl_t
    _fields_ = [("frames", C.c_int64), ("samples", C.c_int64)] + [(n, C.c_int32) for n in ("n_fft", "hop", "n_utt", "accumulate", "n_mels", "nnz")] + [
        (n, _P) for n in ("x", "y", "smp_off", "frame_utt", "utt_off", "window", "twiddle", "fb_lo", "fb_off", "fb_w", "bt_off", "bt_ch", "bt_w",
                          "frame_sums", "utt_sums", "coef", "fr", "gx")]


class PwdLayer(C.Structure):  # fcl_pwd_t
    _fields_ = [("samples", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "ksize", "dilation")] + [("slope", _F), ("reserved", C.c_int32)] + [
        (n, _P) for n in ("x", "w", "bias", "h", "g", "seg_lo", "seg_hi", "y", "dw", "db", "workspace")] + [("workspace_bytes", _Z)]


class PwtBlock(C.Structure):  # fcl_pwt_t
    _fields_ = [("samples", C.c_int64)] + [(n, C.c_int32) for n in ("residual", "aux", "ksize", "dilation", "first", "last")] + [
        (n, _P) for n in ("seg_lo", "seg_hi", "x", "c", "w_gate", "b_gate", "w_out", "b_out", "ab", "x_out", "skips", "z_out", "dxo", "ds", "w_dz", "w_dx",
                          "w_dc", "dz", "dx", "dc", "dw_gate", "db_gate", "dw_out", "db_out", "workspace")] + [("workspace_bytes", _Z)]


class HftConv(C.Structure):  # fcl_hft_conv_t
    _fields_ = [("rows", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "ksize", "dilation", "lrelu")] + [("slope", _F)] + [
        (n, _P) for n in ("seg_lo", "seg_hi", "x", "w", "bias", "res", "pre", "y", "g", "dw", "db", "workspace")] + [("workspace_bytes", _Z)]


class HftTconv(C.Structure):  # fcl_hft_tconv_t
    _fields_ = [("rows", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "stride")] + [("slope", _F)] + [
        (n, _P) for n in ("seg_lo", "seg_hi", "c", "w", "bias", "u", "du", "dc", "dw", "db", "workspace")] + [("workspace_bytes", _Z)]


class HfeEnd(C.Structure):  # fcl_hfe_t
    _fields_ = [("rows", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "ksize")] + [("slope", _F)] + [
        (n, _P) for n in ("seg_lo", "seg_hi", "x", "w", "bias", "wav", "dwav", "dx", "dw", "db", "workspace")] + [("workspace_bytes", _Z)]


class HpdLayer(C.Structure):  # fcl_hpd_t
    _fields_ = [("rows_in", C.c_int64), ("rows_out", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "ksize", "stride", "pad")] + [("slope", _F)] + [
        (n, _P) for n in ("src", "in_lo", "in_hi", "x", "w", "bias", "h", "g", "extra", "y", "dw", "db", "workspace")] + [("workspace_bytes", _Z)]


class HsdLayer(C.Structure):  # fcl_hsd_t
    _fields_ = [("rows_in", C.c_int64), ("rows_out", C.c_int64)] + [(n, C.c_int32) for n in ("cin", "cout", "groups", "ksize", "stride", "pad")] + [
        ("slope", _F)] + [(n, _P) for n in ("src", "in_lo", "in_hi", "x", "w", "bias", "h", "g", "extra", "y", "dw", "db", "workspace")] + [
        ("workspace_bytes", _Z)]


class PweEnds(C.Structure):  # fcl_pwe_t
    _fields_ = [("samples", C.c_int64)] + [(n, C.c_int32) for n in ("frames", "n_utt", "residual", "aux", "ctx", "n_scales")] + [
        ("scales", C.c_int32 * 6), ("sigma", _F), ("reserved", C.c_int32)] + [(n, _P) for n in ("seg_lo", "seg_hi", "frame_off", "c", "z", "w_in")] + [
        ("h", _P * 6), ("w0", _P), ("b0", _P), ("u", _P * 6)] + [(n, _P) for n in ("cu", "x0", "dcu", "dx0")] + [("dh", _P * 6)] + [
        (n, _P) for n in ("dw_in", "dw0", "db0", "dc", "dz", "skips", "w1", "w1t", "b1", "w3", "b3", "y1", "wav", "dwav", "dy1", "ds", "dw1", "db1", "dw3",
                          "db3", "workspace")] + [("workspace_bytes", _Z)]


class BernoulliSite(C.Structure):  # fcl_bernoulli_site_t
    _fields_ = [("out", _P), ("n", C.c_int64), ("p_one", _F), ("seed", C.c_uint32)]


BERNOULLI_MAX_SITES = 16


class LossTerm(C.Structure):  # fcl_loss_term_t
    _fields_ = [(n, _P) for n in ("a", "b", "b2", "valid", "valid2", "da", "da_planes", "sums", "sums2")] + [
        ("m", C.c_int32), ("c", C.c_int32), ("b_log", C.c_int32), ("b_log_offset", _F), ("w_l1", _F), ("w_mse", _F), ("count", C.c_double),
        ("w_l1_2", _F), ("w_mse_2", _F), ("count2", C.c_double)]


LOSS_MAX_TERMS, SUM_ROWS_MAX = 12, 6


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 56), ("launches", _I), ("ms", C.c_double), ("flops", C.c_double), ("rows", C.c_double), ("fill_bytes", C.c_double)]


TE_MAX_SITES, TE_MAX_LOSSES = 48, 48
TE_TEACHER, TE_KD_TEACHER, TE_STUDENT = 0, 1, 2


class TeConfig(C.Structure):  # fcl_te_config_t
    _fields_ = ([(n, C.c_int32) for n in ("role", "idim", "odim", "embed_dim", "econv_layers", "econv_chans", "econv_filts", "eunits", "dunits", "prenet_units",
                                          "postnet_layers", "postnet_chans", "postnet_filts", "dp_layers", "dp_chans", "dp_kernel", "vp_layers", "vp_chans",
                                          "vp_kernel", "ve_kernel")]
                + [(n, _F) for n in ("dropout_rate", "zoneout_rate", "dp_dropout", "vp_dropout", "ve_dropout")]
                + [(n, C.c_int32) for n in ("use_masking", "t_embed_dim", "t_econv_chans", "t_eunits", "t_prenet_units", "t_dunits", "t_postnet_chans", "share_proj",
                                            "distill_output", "distill_encoder", "distill_decoder", "distill_prosody", "accum_grad")]
                + [("seed", C.c_uint32), ("site_tag", C.c_uint32 * TE_MAX_SITES), ("dw_planes_min", C.c_int32), ("pred_stream", C.c_int32),
                   ("late_losses", C.c_int32)])


class TeBatch(C.Structure):  # fcl_te_batch_t
    _fields_ = ([(n, C.c_int32) for n in ("B", "T", "L", "N", "F", "lmax")]
                + [(n, _P) for n in ("xs", "ys", "f0", "energy", "ds", "lens", "e_lo", "e_hi", "f_lo", "f_hi", "src_sorted", "row_of_enc", "cell_frame", "frame_cell",
                                     "prev_frame", "cell_row", "dur", "perm_tb", "cell_row_i64", "enc_pad", "enc_valid", "frame_valid", "cell_valid", "pos4",
                                     "live_rows_host")]
                + [("n_enc", C.c_double), ("n_frames", C.c_double)])


class TeKnowledge(C.Structure):  # fcl_te_knowledge_t
    _fields_ = [("after", _P), ("before", _P), ("enc", _P * 5), ("dec", _P * 8), ("pro", _P * 5), ("dec_cell_major", C.c_int32)]


SIGNATURES = {
    "fcl_te_create": (_I, [C.POINTER(TeConfig), C.POINTER(_P)]),
    "fcl_te_destroy": (None, [_P]),
    "fcl_te_site_name": (C.c_char_p, [_I]),
    "fcl_te_loss_name": (C.c_char_p, [_I]),
    "fcl_te_bind_param": (_I, [_P, C.c_char_p, _P, _P, C.c_int64]),
    "fcl_te_bind_buffer": (_I, [_P, C.c_char_p, _P]),
    "fcl_te_finalize": (_I, [_P, _P]),
    "fcl_te_params_changed": (_I, [_P]),
    "fcl_te_side_stream": (_P, [_P]),
    "fcl_te_place_streams": (_I, [_P, _P, C.POINTER(C.c_int)]),
    "fcl_te_knowledge": (_I, [_P, C.POINTER(TeBatch), C.c_uint32, C.POINTER(TeKnowledge), _P]),
    "fcl_te_forward_backward": (_I, [_P, C.POINTER(TeBatch), C.POINTER(TeKnowledge), C.c_uint32, _P, _P, _P]),
    "fcl_te_backward_stage": (_I, [_P, _I, _P]),
    "fcl_te_join": (_I, [_P, _P]),
    "fcl_te_last_launches": (C.c_int64, [_P]),
    "fcl_te_phase_ms": (_I, [_P, _P]),
    "fcl_te_arena_bytes": (C.c_int64, [_P]),
    "fcl_last_error": (C.c_char_p, []),
    "fcl_version": (_I, []),
    "fcl_debug_ptr": (_P, []),
    "fcl_set_gemm_mode": (_I, [_I]),
    "fcl_get_gemm_mode": (_I, []),
    "fcl_pack_conv1d_weight": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "fcl_fold_batchnorm": (_I, [_P, _P, _P, _P, _F, _P, _P, _I, _P]),
    "fcl_copy2d": (_I, [_P, _I, _P, _I, _I, _I, _P]),
    "fcl_add2d": (_I, [_P, _I, _P, _I, _I, _I, _F, _P, _P]),
    "fcl_frag_bf16_elems": (_Z, [_I, _I]),
    "fcl_pack_frag_bf16": (_I, [_P, _I, _I, _P, _P, _P]),
    "fcl_pack_frag_f32": (_I, [_P, _I, _I, _P, _P]),
    "fcl_add_vec": (_I, [_P, _P, _P, _I, _P]),
    "fcl_u32_add": (_I, [_P, C.c_uint32, _P]),
    "fcl_planes_elems": (_Z, [_I, _I]),
    "fcl_pack_planes": (_I, [_P, _I, _I, _I, _P, _P]),
    "fcl_linear_planes_fwd": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "fcl_linear_planes_mse_fwd": (_I, [_P, _I, _P, _P, _I, _P, C.c_double, _P, _I, _P, _P, _I, _I, _I, _P]),
    "fcl_conv1d_planes_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fcl_conv1d_planes_rows_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "fcl_embedding_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "fcl_embed_conv_table_fwd": (_I, [_P] * 8 + [_I, _I, _I, _I, _I, _P, _P]),
    "fcl_linear_fwd": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fcl_conv1d_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fcl_layernorm_fwd": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _P]),
    "fcl_layernorm_group_fwd": (_I, [_P, _I, C.c_int64, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fcl_conv1d_planes_bn_fwd": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P]),
    "fcl_conv1d_planes_group_fwd": (_I, [_P, _I, C.c_int64, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fcl_duration_round_fwd": (_I, [_P, _P, _I, _I, _F, _P, _P]),
    "fcl_variance_embed_add_fwd": (_I, [_P] * 12 + [_I, _I, _I, _P]),
    "fcl_duration_round_ctl_fwd": (_I, [_P, _P, _I, _I, _F, _P, _P, _I, _I, _P]),
    "fcl_variance_embed_add_ctl_fwd": (_I, [_P] * 10 + [_I, _I] + [_P] * 5 + [_I, _I, _I, _P]),
    "fcl_variance_embed_rows_fwd": (_I, [_P] * 11 + [_I, _I] + [_P] * 3 + [_I, _I, _I, _I, _P]),
    "fcl_position_table_fwd": (_I, [_P, _P, _I, _I, _P]),
    "fcl_concat_spk_fwd": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "fcl_kaldi_ark_append": (C.c_longlong, [_I, C.c_longlong, _I, _P, _P, _P, _I, _P]),
    "fcl_host_device_ptr": (_P, [_P]),
    "fcl_feed_copy": (_I, [_P, _P, _Z, _P, _P, _P, _P]),
    "fcl_row_maps_build": (_I, [C.POINTER(RowMaps), _P]),
    "fcl_gather_rows_fwd": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "fcl_bilstm_workspace_bytes": (_Z, [_I, _I, _I]),
    "fcl_bilstm_fwd": (_I, [_P] * 13 + [_I, _I, _I, _I, _I, _P, _Z, _P, _P, _P]),
    "fcl_bilstm_rows_workspace_bytes": (_Z, [_I, _I]),
    "fcl_bilstm_rows_fwd": (_I, [_P] * 14 + [_I, _I, _I, _I, _P, _Z, _P, _P]),
    "fcl_decoder_loop_workspace_bytes": (_Z, [C.POINTER(DecoderWeights), _I]),
    "fcl_decoder_stream_bytes": (_Z, [C.POINTER(DecoderWeights)]),
    "fcl_decoder_stream_pack": (_I, [C.POINTER(DecoderWeights), _P, _Z, _P]),
    "fcl_decoder_loop_fwd": (_I, [C.POINTER(DecoderWeights), C.POINTER(DecoderIO), _P]),
    "fcl_masked_l1_mse_fwd": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _F, _P, _P]),
    "fcl_gemm_tn_fwd": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "fcl_gemm_tn_taps_fwd": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _Z, _P, _P, _P]),
    "fcl_colsum_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fcl_colsum2_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fcl_conv1d_in1_dw": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fcl_act_fwd": (_I, [_P, _P, _F, _P, _P, _I, _Z, _I, _P]),
    "fcl_unpack_conv1d_grad": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "fcl_act_bwd": (_I, [_P, _P, _P, _F, _P, _P, _I, _Z, _I, _P]),
    "fcl_l1_mse_grad": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, C.c_double, _P, _I, _P]),
    "fcl_l1_mse_loss_grad": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, C.c_double, _P, _I, _P, _P, _P]),
    "fcl_layernorm_bwd": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _P]),
    "fcl_bn_stats_fwd": (_I, [_P, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P]),
    "fcl_bn_stats_ws_fwd": (_I, [_P, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P]),
    "fcl_bn_act_fwd": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _P]),
    "fcl_bn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "fcl_scale": (_I, [_P, _Z, _F, _P]),
    "fcl_bernoulli_u8": (_I, [_P, _Z, _F, C.c_uint32, _P, _P]),
    "fcl_bernoulli_batch": (_I, [C.POINTER(BernoulliSite), _I, _P]),
    "fcl_lstm_cell_bwd": (_I, [_P, _P, _P, _P, _P, _I, _P, _F, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _P]),
    "fcl_scatter_add_rows": (_I, [_P, _P, _P, _I, _I, C.c_int64, _P]),
    "fcl_transpose2d": (_I, [_P, _P, _I, _I, _P]),
    "fcl_pack_planes_t": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "fcl_gemm_tn_planes": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _Z, _P]),
    "fcl_pwg_upsample_stage": (_I, [_P, _P, _P, C.c_int64, _I, _I, _P, _P, _P, _I, _I, _P]),
    "fcl_pwg_noise": (_I, [_P, C.c_int64, C.c_uint32, _P]),
    "fcl_pwg_aux_coeff": (_I, [_P, C.c_int64, _I, C.c_int64, _P, _P]),
    "fcl_pwg_first_conv": (_I, [_P, _P, _P, _P, _P, C.c_int64, _I, _I, _P]),
    "fcl_pwg_layer_fwd": (_I, [_P, _P]),
    "fcl_pwg_last_fwd": (_I, [_P, _F, _P, _P, _P, _F, _P, _P, _P, C.c_int64, _I, _P]),
    "fcl_pwg_maps_build": (_I, [_P, _P, _I, C.c_int64, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fcl_pwg_gather_pad": (_I, [_P, C.c_int64, _P, _P, C.c_int64, _I, _P, _P]),
    "fcl_pwg_noise_cap": (_I, [_P, C.c_int64, C.c_uint32, _P, _P, _P]),
    "fcl_pwg_first_conv_cap": (_I, [_P, _P, _P, _P, C.c_int64, _I, _P, _P]),
    "fcl_pwg_layer_cap_fwd": (_I, [_P, _P, _P]),
    "fcl_pwg_last_cap_fwd": (_I, [_P, _F, _P, _P, _P, _F, _P, C.c_int64, _I, _P, _P]),
    "fcl_pcm16_fwd": (_I, [_P, _P, C.c_int64, _P, _P, _P]),
    "fcl_hfg_conv_fwd": (_I, [C.POINTER(HfgConv), _P]),
    "fcl_hfg_tconv_fwd": (_I, [C.POINTER(HfgTconv), _P]),
    "fcl_hfg_unit_fwd": (_I, [C.POINTER(HfgUnit), _P]),
    "fcl_hfg_out_fwd": (_I, [_P, _P, _P, _P, _P, _I, _P, C.c_int64, _I, _I, _I, _P]),
    "fcl_hfg_maps_build": (_I, [_P, _P, _I, C.c_int64, _I, _P, _P, _P, _P]),
    "fcl_hfg_conv_cap_fwd": (_I, [C.POINTER(HfgConv), _P, _P]),
    "fcl_hfg_tconv_cap_fwd": (_I, [C.POINTER(HfgTconv), _P, _P]),
    "fcl_hfg_unit_cap_fwd": (_I, [C.POINTER(HfgUnit), _P, _P]),
    "fcl_hfg_out_cap_fwd": (_I, [_P, _P, _P, _P, _P, _I, _P, C.c_int64, _I, _I, _I, _P, _P]),
    "fcl_gl_mel2lin_fwd": (_I, [_P, _P, _P, _P, C.c_int64, _I, _I, _P]),
    "fcl_gl_phase_init": (_I, [C.POINTER(GriffinLim), _P]),
    "fcl_gl_synth_fwd": (_I, [C.POINTER(GriffinLim), _P]),
    "fcl_gl_ola_fwd": (_I, [C.POINTER(GriffinLim), _P]),
    "fcl_gl_analysis_fwd": (_I, [C.POINTER(GriffinLim), _P]),
    "fcl_fx_logmel_fwd": (_I, [C.POINTER(Features), _P]),
    "fcl_fx_segment_mean_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, _I, C.c_int64, _I, _P]),
    "fcl_px_yin_fwd": (_I, [C.POINTER(Pitch), _P]),
    "fcl_px_short_run_fwd": (_I, [_P, _P, _P, _P, C.c_int64, _I, _I, _P]),
    "fcl_px_pyin_obs_fwd": (_I, [C.POINTER(Pyin), _P]),
    "fcl_px_pyin_viterbi_fwd": (_I, [C.POINTER(Pyin), _P]),
    "fcl_rs_resample_fwd": (_I, [C.POINTER(Resample), _P]),
    "fcl_ev_dtw_workspace_bytes": (_Z, [C.c_int64, _I]),
    "fcl_ev_cepstra_fwd": (_I, [_P, _P, _P, _P, C.c_int64, _I, _I, _P]),
    "fcl_ev_dtw_fwd": (_I, [C.POINTER(Evaluate), _P]),
    "fcl_ev_path_pitch_fwd": (_I, [C.POINTER(Evaluate), _P]),
    "fcl_al_workspace_bytes": (_Z, [C.c_int64, _I]),
    "fcl_al_loglik_fwd": (_I, [_P, _P, _P, _P, _P, C.c_int64, _I, _I, _P]),
    "fcl_al_viterbi_fwd": (_I, [C.POINTER(Align), _P]),
    "fcl_al_stats_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, _I, _I, _P]),
    "fcl_al_lattice_viterbi_fwd": (_I, [C.POINTER(AlignLattice), _P]),
    "fcl_al_gmm_loglik_fwd": (_I, [_P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _I, _P]),
    "fcl_al_gmm_post_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _I, _P]),
    "fcl_al_gmm_stats_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, _I, _I, _I, _I, _P]),
    "fcl_stl_sums_fwd": (_I, [C.POINTER(StftLoss), _P]),
    "fcl_stl_grad_bwd": (_I, [C.POINTER(StftLoss), _P]),
    "fcl_msl_sums_fwd": (_I, [C.POINTER(MelLoss), _P]),
    "fcl_msl_grad_bwd": (_I, [C.POINTER(MelLoss), _P]),
    "fcl_pwd_dw_workspace_bytes": (_Z, [C.c_int64, _I, _I, _I]),
    "fcl_pwd_layer_fwd": (_I, [C.POINTER(PwdLayer), _P]),
    "fcl_pwd_layer_dx": (_I, [C.POINTER(PwdLayer), _P]),
    "fcl_pwd_layer_dw": (_I, [C.POINTER(PwdLayer), _P]),
    "fcl_pwt_dw_workspace_bytes": (_Z, [C.c_int64, _I, _I, _I]),
    "fcl_pwt_block_fwd": (_I, [C.POINTER(PwtBlock), _P]),
    "fcl_pwt_block_dx": (_I, [C.POINTER(PwtBlock), _P]),
    "fcl_pwt_block_dw": (_I, [C.POINTER(PwtBlock), _P]),
    "fcl_hft_workspace_bytes": (_Z, [C.c_int64, _I, _I, _I, _I]),
    "fcl_hft_conv_fwd": (_I, [C.POINTER(HftConv), _P]),
    "fcl_hft_conv_dx": (_I, [C.POINTER(HftConv), _P]),
    "fcl_hft_conv_dw": (_I, [C.POINTER(HftConv), _P]),
    "fcl_hft_tconv_fwd": (_I, [C.POINTER(HftTconv), _P]),
    "fcl_hft_tconv_dx": (_I, [C.POINTER(HftTconv), _P]),
    "fcl_hft_tconv_dw": (_I, [C.POINTER(HftTconv), _P]),
    "fcl_hft_sum": (_I, [_P, C.POINTER(_P), _I, _F, C.c_int64, _P]),
    "fcl_hfe_workspace_bytes": (_Z, [C.c_int64, _I, _I, _I]),
    "fcl_hfe_fwd": (_I, [C.POINTER(HfeEnd), _P]),
    "fcl_hfe_dx": (_I, [C.POINTER(HfeEnd), _P]),
    "fcl_hfe_dw": (_I, [C.POINTER(HfeEnd), _P]),
    "fcl_hpd_dw_workspace_bytes": (_Z, [C.c_int64, _I, _I, _I]),
    "fcl_hpd_layer_fwd": (_I, [C.POINTER(HpdLayer), _P]),
    "fcl_hpd_layer_dx": (_I, [C.POINTER(HpdLayer), _P]),
    "fcl_hpd_layer_dw": (_I, [C.POINTER(HpdLayer), _P]),
    "fcl_hsd_dw_workspace_bytes": (_Z, [C.c_int64, _I, _I, _I, _I]),
    "fcl_hsd_layer_fwd": (_I, [C.POINTER(HsdLayer), _P]),
    "fcl_hsd_layer_dx": (_I, [C.POINTER(HsdLayer), _P]),
    "fcl_hsd_layer_dw": (_I, [C.POINTER(HsdLayer), _P]),
    "fcl_hsd_pool_fwd": (_I, [_P, _P, _P, _P, _I, C.c_int64, C.c_int64, _P]),
    "fcl_hsd_pool_dx": (_I, [_P, _P, _P, _P, _I, C.c_int64, C.c_int64, _P]),
    "fcl_pwe_workspace_bytes": (_Z, [C.POINTER(PweEnds)]),
    "fcl_pwe_in_fwd": (_I, [C.POINTER(PweEnds), _P]),
    "fcl_pwe_in_bwd": (_I, [C.POINTER(PweEnds), _P]),
    "fcl_pwe_out_fwd": (_I, [C.POINTER(PweEnds), _P]),
    "fcl_pwe_out_bwd": (_I, [C.POINTER(PweEnds), _P]),
    "fcl_derive_blocks": (_I, [_I, _I, _I]),
    "fcl_derive_batch": (_I, [_P, _I, _I, _P]),
    "fcl_sumsq_accum": (_I, [_P, _Z, _P, _P]),
    "fcl_adam_step": (_I, [_P, _P, _P, _P, _Z, _P, _F, _F, _F, _F, _F, _P, _P, _P]),
    "fcl_adam_step_wd": (_I, [_P, _P, _P, _P, _Z, _P, _F, _F, _F, _F, _F, _F, _P, _P, _P]),
    "fcl_lstm_step_fwd": (_I, [C.POINTER(LstmStep), _P]),
    "fcl_decoder_train_workspace_bytes": (_Z, [_I, _I]),
    "fcl_decoder_train_fwd": (_I, [C.POINTER(DecoderTrain), _P]),
    "fcl_decoder_bptt": (_I, [C.POINTER(DecoderBptt), _P]),
    "fcl_bilstm_train_workspace_bytes": (_Z, [_I, _I]),
    "fcl_bilstm_train_fwd": (_I, [C.POINTER(BilstmTrain), _P]),
    "fcl_bilstm_bptt": (_I, [C.POINTER(BilstmBptt), _P]),
    "fcl_loss_terms_batch": (_I, [C.POINTER(LossTerm), _I, _P]),
    "fcl_sum_rows": (_I, [C.POINTER(C.c_void_p), _I, _P, _P, _P, _I, _I, _P]),
    "fcl_bn_bwd_sums": (_I, [_P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "fcl_act_bwd_sum": (_I, [_P, _P, _P, _P, _F, _P, _P, _I, _Z, _I, _P]),
    "fcl_gather_rows_sum_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "fcl_linear2_fwd": (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _I, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "fcl_stream_create_cus": (_I, [_I, C.POINTER(C.c_void_p)]),
    "fcl_stream_destroy": (_I, [_P]),
    "fcl_streams_share_pipe": (_I, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "fcl_stream_create_apart": (_I, [C.POINTER(C.c_void_p), _I, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "fcl_prof_enable": (_I, [_I]),
    "fcl_prof_collect": (_I, [C.POINTER(ProfEntry), _I]),
}

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
DROP_NONE, DROP_MASK, DROP_RNG = 0, 1, 2
STATUS_GROUP_TIMEOUT, STATUS_ZERO_DURATION, STATUS_LMAX_CAP, STATUS_FRAMES_CAP, STATUS_ROWS_CAP = 1, 2, 4, 8, 16  # FCL_STATUS_* bits of a device status word
STATUS_VOCODER_CAP, STATUS_PCM_NONFINITE = 32, 64  # the vocoder stage of a text -> waveform pass

_lib = None


class FclError(RuntimeError):
    pass


def load():
    """Load libfcl_hip.so and bind every symbol of include/fcl_hip.h.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FclError(
            "fcl-taco2_amd: %s not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C fcl-taco2_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    # torch first: device memory and streams come from torch, so libfcl_hip.so must bind to the HIP runtime torch has loaded.  Loading the .so
    # before torch pulls in /opt/rocm's libamdhip64 and torch then finds "no ROCm-capable device" in the same process (seen with build(); smoke()).
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.fcl_version() != ABI_VERSION:  # a stale in-tree build: the struct layouts mirrored here would not match
        raise FclError("fcl-taco2_amd: %s has ABI revision %d, this package mirrors %d — rebuild it (`make -C fcl-taco2_amd/csrc`)"
                       % (LIB_PATH, lib.fcl_version(), ABI_VERSION))
    _lib = lib
    return lib


def prof_enable(on):
    check(load().fcl_prof_enable(int(on)))


def prof_collect():
    """{kernel name: dict(launches, ms, flops, rows)} for the launches since prof_enable(True)."""
    buf = (ProfEntry * 256)()
    n = load().fcl_prof_collect(buf, 256)
    if n < 0:
        check(n)
    return {buf[i].name.decode(): dict(launches=buf[i].launches, ms=buf[i].ms, flops=buf[i].flops, rows=buf[i].rows, fill_bytes=buf[i].fill_bytes) for i in range(n)}


def check(rc):
    if rc != 0:
        msg = load().fcl_last_error()
        raise FclError("libfcl_hip error %d: %s" % (rc, msg.decode("utf-8", "replace") if msg else "?"))
