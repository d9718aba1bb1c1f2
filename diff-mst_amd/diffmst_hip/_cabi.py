"""ctypes binding of the C ABI declared in ``include/diffmst_hip.h``.

``bind(lib)`` only attaches argument / return types to an already opened shared
library; which library gets opened is decided elsewhere (``mst._hip`` opens the
gfx950 build and nothing else).
"""
from __future__ import annotations

import ctypes as C

NUM_TRACK_PARAMS = 27
NUM_FX_PARAMS = 25
NUM_MASTER_PARAMS = 26

USE_TRACK_INPUT_FADER = 0x01
USE_TRACK_EQ = 0x02
USE_TRACK_COMPRESSOR = 0x04
USE_TRACK_PANNER = 0x08
USE_FX_BUS = 0x10
USE_MASTER_BUS = 0x20
USE_OUTPUT_FADER = 0x40
SAVE_FOR_BACKWARD = 0x100
DEV_MULTIPASS_EQ = 0x200
NO_RANGE_CHECK = 0x400
BWD_PREPARED = 0x800
SPLIT_BATCH = 0x1000

ABI_VERSION = 13


class ConsoleDesc(C.Structure):
    _fields_ = [
        ("bs", C.c_int32),
        ("n_tracks", C.c_int32),
        ("n_samples", C.c_int64),
        ("track_row_stride", C.c_int64),
        ("sample_rate", C.c_float),
        ("flags", C.c_uint32),
        ("track_lookahead", C.c_int32),
        ("master_lookahead", C.c_int32),
        ("track_lo", C.c_float * NUM_TRACK_PARAMS),
        ("track_hi", C.c_float * NUM_TRACK_PARAMS),
        ("master_lo", C.c_float * NUM_MASTER_PARAMS),
        ("master_hi", C.c_float * NUM_MASTER_PARAMS),
        ("fx_lo", C.c_float * NUM_FX_PARAMS),
        ("fx_hi", C.c_float * NUM_FX_PARAMS),
        ("fx_ir_samples", C.c_int32),
        ("fx_bandpass_taps", C.c_int32),
    ]


class ConsoleFx(C.Structure):  # mirrors mst_console_fx
    _fields_ = [("noise", C.c_void_p), ("filters", C.c_void_p), ("tables", C.c_void_p)]


class ConsoleOverlap(C.Structure):  # mirrors mst_console_overlap: the side stream and the two events a split call borrows
    _fields_ = [("side_stream", C.c_void_p), ("fork_event", C.c_void_p), ("join_event", C.c_void_p)]


MAX_RESOLUTIONS = 8


class MrstftDesc(C.Structure):
    _fields_ = [
        ("rows", C.c_int32),
        ("n_samples", C.c_int64),
        ("n_res", C.c_int32),
        ("fft_size", C.c_int32 * MAX_RESOLUTIONS),
        ("hop_size", C.c_int32 * MAX_RESOLUTIONS),
        ("win_length", C.c_int32 * MAX_RESOLUTIONS),
        ("w_sc", C.c_float),
        ("w_log_mag", C.c_float),
        ("w_lin_mag", C.c_float),
        ("sc_per_example", C.c_int32),
        ("eps", C.c_float),
    ]


class Cnn14Desc(C.Structure):  # mirrors mst_cnn14_desc
    _fields_ = [("n", C.c_int32), ("frames", C.c_int32), ("bins", C.c_int32), ("embed_dim", C.c_int32), ("precision", C.c_int32),
                ("training", C.c_int32), ("bn_eps", C.c_float), ("world", C.c_int32)]


SYNC_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)  # mst_sync_fn(user, sums, n_doubles, stream)


CNN14_CONVS = 12


class Cnn14Params(C.Structure):  # mirrors mst_cnn14_params
    _fields_ = [("conv_w", C.c_void_p * CNN14_CONVS), ("bn_gamma", C.c_void_p * CNN14_CONVS), ("bn_beta", C.c_void_p * CNN14_CONVS),
                ("bn_mean", C.c_void_p * CNN14_CONVS), ("bn_var", C.c_void_p * CNN14_CONVS), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


class Cnn14Grads(C.Structure):  # mirrors mst_cnn14_grads
    _fields_ = [("conv_w", C.c_void_p * CNN14_CONVS), ("bn_gamma", C.c_void_p * CNN14_CONVS), ("bn_beta", C.c_void_p * CNN14_CONVS),
                ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


CTRL_FIELDS = ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "linear1_weight", "linear1_bias",
               "linear2_weight", "linear2_bias", "norm1_weight", "norm1_bias", "norm2_weight", "norm2_bias")


class CtrlDesc(C.Structure):  # mirrors mst_ctrl_desc
    _fields_ = [("bs", C.c_int32), ("seq", C.c_int32), ("d_model", C.c_int32), ("nhead", C.c_int32), ("d_ff", C.c_int32),
                ("n_layers", C.c_int32), ("ln_eps", C.c_float)]


CTRL_IO_FIELDS = ("track_embedding", "mix_embedding", "fx_bus_embedding", "master_bus_embedding", "track_w", "track_b", "fx_w", "fx_b",
                  "master_w", "master_b")


class CtrlIO(C.Structure):  # mirrors mst_ctrl_io and mst_ctrl_io_grads (same ten pointers)
    _fields_ = [(name, C.c_void_p) for name in CTRL_IO_FIELDS]


class CtrlLayer(C.Structure):  # mirrors mst_ctrl_layer and mst_ctrl_layer_grads (same twelve pointers)
    _fields_ = [(name, C.c_void_p) for name in CTRL_FIELDS]


OPT_MAX_TERMS = 8  # MST_OPT_MAX_TERMS
OPT_MAX_ITEMS = 1024  # items of mst_logit_adam_step_batch
OPT_MAX_SECTIONS = 64  # MST_OPT_MAX_SECTIONS: sections of mst_logit_adam_step_sections, and of mst_pick_sections
OPT_MAX_LINK_ROWS = 256  # MST_OPT_MAX_LINK_ROWS: rows of the tied segment of mst_logit_adam_step_linked
OPT_HEADER_WORDS = 16  # int32 words in front of an item's moments
OPT_BEST_HEADER_WORDS = 16  # int32 words in front of an item's best logits (mst_logit_adam_step_best)
AF_PROFILE_DOUBLES = 54  # MST_AF_PROFILE_DOUBLES
LOUDNESS_MAX_BLOCKS = 4092  # MST_LOUDNESS_MAX_BLOCKS: gating blocks of a signal, windows of mst_pick_sections
PICK_MAX_TRACKS = 256  # MST_PICK_MAX_TRACKS
TRUE_PEAK_TILE = 2048  # MST_TRUE_PEAK_TILE: positions one workgroup of k_true_peak covers


class LogitAdamSegment(C.Structure):  # mirrors mst_logit_adam_segment
    _fields_ = [("theta", C.c_void_p), ("p", C.c_void_p), ("grad_p", C.c_void_p), ("count", C.c_int64)]


class LogitAdamLinks(C.Structure):  # mirrors mst_logit_adam_links
    _fields_ = [("segment", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("mirror_col", C.c_int32),
                ("leader", C.c_uint8 * OPT_MAX_LINK_ROWS)]


def ptr(t):
    """Address of a tensor (device memory, or host memory in the simulator tests) as a ``c_void_p``; NULL for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


class DevPtr:
    """Argument type of a buffer pointer: ``ptr()`` applied by ``ctypes`` at the call.  A tensor is passed as it is and goes in as
    its ``data_ptr()``, ``None`` as NULL; an int or a ``c_void_p`` passes as ``c_void_p`` takes it and anything else is a
    ``ctypes.ArgumentError`` - ``str`` and ``bytes`` too, which ``c_void_p`` itself would pass as the address of their characters.
    Dtype, contiguity and device are the caller's to check (``_hip.require_cuda``, ``.float().contiguous()``)."""

    @classmethod
    def from_param(cls, obj):
        if obj is None or hasattr(obj, "data_ptr"):
            return ptr(obj)
        if isinstance(obj, (str, bytes)):
            raise TypeError("a buffer argument is a tensor, None, an address or a c_void_p")
        return C.c_void_p.from_param(obj)


class STATUS:
    """Return-type marker of the entries that report a ``hipError_t``-like int (0 = ok): the launchers and the ``*_init_tables``
    functions.  ``bind()`` makes a non-zero value of these an ``AbiError``; the sizes and counts (``c_int32`` is ``c_int`` here, so the
    type cannot tell them apart) and ``mst_abi_version`` come back as numbers."""


class AbiError(RuntimeError):
    """A ``STATUS`` entry returned non-zero: ``name`` is the exported symbol that was called, ``code`` what it returned."""

    def __init__(self, name, code):
        super().__init__(f"{name} failed with hipError {code}")
        self.name, self.code = name, code


_P = DevPtr      # buffers
_S = C.c_void_p  # streams, events and the sync hook's `user` pointer: raw handles


SIGNATURES = {
    "mst_abi_version": (C.c_int, []),
    "mst_console_workspace_bytes": (C.c_size_t, [C.POINTER(ConsoleDesc)]),
    "mst_console_fx_tables_bytes": (C.c_size_t, []),
    "mst_console_fx_init_tables": (STATUS, [_P, _S]),
    "mst_console_forward": (STATUS, [C.POINTER(ConsoleDesc), _P, _P, _P, _P, C.POINTER(ConsoleFx), _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_console_forward_mirrored": (STATUS, [C.POINTER(ConsoleDesc), _P, _P, _P, _P, C.POINTER(ConsoleFx), _P, _P, _P, _P, C.c_size_t, _S, _P, _S]),
    "mst_console_backward": (STATUS, [C.POINTER(ConsoleDesc), _P, _P, _P, _P, C.POINTER(ConsoleFx), _P, _P, _P, _P, _P, _P, _P, _P,
                                     C.c_size_t, _S]),
    "mst_console_backward_prepare": (STATUS, [C.POINTER(ConsoleDesc), _P, C.c_size_t, _S]),
    "mst_console_forward_overlapped": (STATUS, [C.POINTER(ConsoleDesc), _P, _P, _P, _P, C.POINTER(ConsoleFx), _P, _P, _P, _P, C.c_size_t, _S,
                                               C.POINTER(ConsoleOverlap)]),
    "mst_console_backward_overlapped": (STATUS, [C.POINTER(ConsoleDesc), _P, _P, _P, _P, C.POINTER(ConsoleFx), _P, _P, _P, _P, _P, _P, _P, _P,
                                                C.c_size_t, _S, C.POINTER(ConsoleOverlap)]),
    "mst_mrstft_tables_bytes": (C.c_size_t, [C.POINTER(MrstftDesc)]),
    "mst_mrstft_init_tables": (STATUS, [C.POINTER(MrstftDesc), _P, _S]),
    "mst_mrstft_workspace_bytes": (C.c_size_t, [C.POINTER(MrstftDesc)]),
    "mst_mrstft_forward": (STATUS, [C.POINTER(MrstftDesc), _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_forward_eval": (STATUS, [C.POINTER(MrstftDesc), _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_forward_partial": (STATUS, [C.POINTER(MrstftDesc), _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_forward_finish": (STATUS, [C.POINTER(MrstftDesc), _P, C.c_int32, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_backward": (STATUS, [C.POINTER(MrstftDesc), _P, _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_forward_items": (STATUS, [C.POINTER(MrstftDesc), C.c_int32, _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_forward_items_eval": (STATUS, [C.POINTER(MrstftDesc), C.c_int32, _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_mrstft_backward_items": (STATUS, [C.POINTER(MrstftDesc), C.c_int32, _P, _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_peak_normalize_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "mst_peak_normalize_forward": (STATUS, [_P, _P, C.c_int32, C.c_int64, _P, C.c_size_t, _S]),
    "mst_peak_normalize_backward": (STATUS, [_P, _P, _P, C.c_int32, C.c_int64, _P, C.c_size_t, _S]),
    "mst_loudness_tables_bytes": (C.c_size_t, [C.c_int32]),
    "mst_loudness_init_tables": (STATUS, [C.c_int32, _P, _S]),
    "mst_loudness_num_blocks": (C.c_int32, [C.c_int64, C.c_int32]),
    "mst_loudness_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "mst_loudness_integrated": (STATUS, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P,
                                        C.c_size_t, _S]),
    "mst_loudness_normalize": (STATUS, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float,
                                       _P, _S]),
    "mst_loudness_num_windows": (STATUS, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "mst_loudness_windows_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "mst_loudness_windows": (STATUS, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _P, C.c_int32, C.c_int32, _P,
                                     _P, _P, C.c_size_t, _S]),
    "mst_true_peak_factor": (STATUS, [C.c_int32, C.POINTER(C.c_int32)]),
    "mst_true_peak_coefficients": (STATUS, [C.c_int32, C.POINTER(C.c_float)]),
    "mst_true_peak_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "mst_true_peak": (STATUS, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, C.c_size_t, _S]),
    "mst_true_peak_sample": (STATUS, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, C.c_size_t,
                                     _S]),
    "mst_loudness_num_short_term": (STATUS, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "mst_loudness_range_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "mst_loudness_range": (STATUS, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, _P, _P,
                                   _P, _P, C.c_size_t, _S]),
    "mst_loudness_normalize_limited": (STATUS, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_float,
                                               C.c_float, C.c_float, _P, _P, _S]),
    "mst_pick_sections": (STATUS, [_P, _P, _P, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _S]),
    "mst_resample_tables_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "mst_resample_init_tables": (STATUS, [C.c_int32, C.c_int32, _P, _S]),
    "mst_resample_out_samples": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "mst_resample_forward": (STATUS, [_P, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, _S]),
    "mst_resample_backward": (STATUS, [_P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _S]),
    "mst_logit_adam_state_bytes": (C.c_size_t, [C.c_int64]),
    "mst_logit_adam_init": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, _P, _S]),
    "mst_logit_adam_step": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.POINTER(C.c_void_p), C.c_int32, _P, C.c_double, C.c_double,
                                     C.c_double, C.c_double, _P, _S]),
    "mst_logit_adam_batch_state_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "mst_logit_adam_init_batch": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, _P, _S]),
    "mst_logit_adam_step_batch": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double, C.c_double,
                                           C.c_double, C.c_double, _P, _S]),
    "mst_logit_adam_best_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "mst_logit_adam_step_best": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.POINTER(C.c_void_p), C.c_int32, _P, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _S]),
    "mst_logit_adam_step_best_batch": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double,
                                                C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _S]),
    "mst_logit_adam_init_sections": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, _P, _S]),
    "mst_logit_adam_step_sections": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, _P,
                                              C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _S]),
    "mst_logit_adam_init_sections_batch": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, C.c_int32, _P, _S]),
    "mst_logit_adam_step_sections_batch": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P,
                                                    C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _S]),
    "mst_logit_adam_init_linked": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, C.c_int32, C.POINTER(LogitAdamLinks), _P,
                                            _S]),
    "mst_logit_adam_step_linked": (STATUS, [C.POINTER(LogitAdamSegment), C.c_int32, C.c_int32, C.c_int32, C.POINTER(LogitAdamLinks), _P,
                                            C.c_int32, _P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P,
                                            _S]),
    "mst_afloss_tables_bytes": (C.c_size_t, []),
    "mst_afloss_init_tables": (STATUS, [_P, _S]),
    "mst_afloss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "mst_afloss_forward": (STATUS, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_spectrogram_tables_bytes": (C.c_size_t, []),
    "mst_spectrogram_init_tables": (STATUS, [_P, _S]),
    "mst_spectrogram_forward": (STATUS, [_P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _S]),
    "mst_cnn14_workspace_bytes": (C.c_size_t, [C.POINTER(Cnn14Desc)]),
    "mst_cnn14_forward": (STATUS, [C.POINTER(Cnn14Desc), _P, C.POINTER(Cnn14Params), _P, _P, _P, C.c_size_t, _S]),
    "mst_cnn14_backward": (STATUS, [C.POINTER(Cnn14Desc), _P, C.POINTER(Cnn14Params), _P, C.POINTER(Cnn14Grads), _P, C.c_size_t, _S]),
    "mst_cnn14_forward_sync": (STATUS, [C.POINTER(Cnn14Desc), _P, C.POINTER(Cnn14Params), _P, _P, _P, C.c_size_t, _S, SYNC_FN, _S]),
    "mst_cnn14_backward_sync": (STATUS, [C.POINTER(Cnn14Desc), _P, C.POINTER(Cnn14Params), _P, C.POINTER(Cnn14Grads), _P, C.c_size_t, _S,
                                        SYNC_FN, _S]),
    "mst_conv3x3_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "mst_conv3x3_splitk_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mst_conv3x3_part_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mst_conv3x3": (STATUS, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                             C.c_int32, _P, C.c_size_t, _P, C.c_size_t, _S]),
    "mst_conv_wgrad_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mst_conv_wgrad": (STATUS, [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32), _S]),
    "mst_afloss_backward": (STATUS, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_af_profile_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "mst_af_profile": (STATUS, [_P, C.c_int32, C.c_int64, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_afloss_profile_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "mst_afloss_forward_profile": (STATUS, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_afloss_backward_profile": (STATUS, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_afloss_forward_profile_items": (STATUS, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_afloss_backward_profile_items": (STATUS, [_P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, _P, C.c_size_t,
                                                   _S]),
    "mst_af_profile_pooled": (STATUS, [_P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, _P, C.c_size_t, _S]),
    "mst_afloss_forward_profile_pooled": (STATUS, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P,
                                                   C.c_size_t, _S]),
    "mst_afloss_backward_profile_pooled": (STATUS, [_P, _P, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P, _P, _P, _P, _P,
                                                    C.c_size_t, _S]),
    "mst_ctrl_workspace_bytes": (C.c_size_t, [C.POINTER(CtrlDesc)]),
    "mst_ctrl_forward": (STATUS, [C.POINTER(CtrlDesc), _P, _P, C.POINTER(CtrlLayer), _P, _P, C.c_size_t, _S]),
    "mst_ctrl_backward": (STATUS, [C.POINTER(CtrlDesc), _P, C.POINTER(CtrlLayer), _P, C.POINTER(CtrlLayer), _P, _P, C.c_size_t, _S]),
    "mst_ctrl_tokens_forward": (STATUS, [C.POINTER(CtrlDesc), C.c_int32, _P, _P, _P, C.POINTER(CtrlIO), _P, _P, _S]),
    "mst_ctrl_heads_forward": (STATUS, [C.POINTER(CtrlDesc), C.c_int32, _P, C.POINTER(CtrlIO), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _S]),
    "mst_ctrl_heads_scratch_bytes": (C.c_size_t, [C.POINTER(CtrlDesc), C.c_int32]),
    "mst_ctrl_heads_backward": (STATUS, [C.POINTER(CtrlDesc), C.c_int32, _P, C.POINTER(CtrlIO), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P,
                                        C.POINTER(CtrlIO), _P, _P, _S]),
    "mst_ctrl_tokens_backward": (STATUS, [C.POINTER(CtrlDesc), C.c_int32, _P, C.POINTER(CtrlIO), _S]),
}


def _raise_on_status(code, fn, _args):
    if code:
        raise AbiError(fn.__name__, code)
    return code


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.argtypes = args
        if res is STATUS:
            fn.restype, fn.errcheck = C.c_int, _raise_on_status
        else:
            fn.restype = res
    if lib.mst_abi_version() != ABI_VERSION:
        raise RuntimeError(f"diffmst ABI mismatch: library {lib.mst_abi_version()} != binding {ABI_VERSION}")
    return lib
