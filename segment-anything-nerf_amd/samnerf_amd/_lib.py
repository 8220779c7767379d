"""ctypes binding of libsamnerf_hip.so (include/samnerf_hip.h).

The product path has no fallback: if the HIP library is missing or cannot be
loaded, every op raises SamnerfUnavailable with the build command.
"""
import contextlib
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAMNERF_LIB: another build of the same library (A/B timing of two builds in
# one GPU session); the in-tree build otherwise.
LIB_PATH = os.environ.get("SAMNERF_LIB") or os.path.join(_HERE, "libsamnerf_hip.so")

_u32 = ctypes.c_uint32
_f32 = ctypes.c_float
_f64 = ctypes.c_double
_int = ctypes.c_int
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_u64 = ctypes.c_uint64


class SamnerfUnavailable(RuntimeError):
    pass


class SamnerfGrid(ctypes.Structure):
    _fields_ = [("embeddings", _vp), ("offsets_host", ctypes.POINTER(ctypes.c_int32)),
                ("num_levels", _u32), ("level_dim", _u32), ("S", _f32),
                ("base_resolution", _u32)]


class SamnerfModel(ctypes.Structure):
    _fields_ = [("grid", SamnerfGrid), ("s_grid", SamnerfGrid), ("prop", SamnerfGrid * 2),
                ("grid_mlp", _vp * 3), ("view_mlp", _vp * 3), ("prop_mlp", (_vp * 2) * 2),
                ("sam_w", _vp * 5), ("sam_b", _vp * 5), ("ln_w", _vp), ("ln_b", _vp),
                ("with_sam", _int), ("aabb", _f32 * 6), ("grid_bound", _f32),
                ("min_near", _f32), ("num_steps", _u32 * 3), ("head_mode", _int),
                ("t_thresh", _f32), ("view_width", _u32),
                ("with_mask", _int), ("mask_kind", _int), ("m_grid", SamnerfGrid), ("mask_w", _vp * 8),
                ("mask_out", _u32),
                ("sum_after_mlp", _int), ("perturb", _vp * 3), ("reuse_packed", _int),
                ("perturb_device", _int), ("perturb_seed", _u64), ("perturb_offset", _u64)]


class SamnerfBackground(ctypes.Structure):
    """samnerf_background (include/samnerf_hip.h): samnerf_set_background's argument."""
    _fields_ = [("background", _int), ("bg_rgb", _vp), ("n_bg", _u32)]


class SamnerfMaskLossArgs(ctypes.Structure):
    """samnerf_mask_loss_args (include/samnerf_hip.h)."""
    _fields_ = [("N", _u32), ("K", _u32), ("n", _u32), ("L", _u32), ("Q", _u32), ("S", _u32), ("P", _u32),
                ("redundant", ctypes.c_int32), ("use_pred_logistics", ctypes.c_int32),
                ("incoherent_weight", _f32), ("label_reg_weight", _f32), ("rgb_weight", _f32),
                ("rgb_threshold", _f32), ("rgb_exp_weight", _f32), ("epsilon", _f64), ("map_cells", _u64),
                ("labels", _vp), ("incoherent", _vp), ("error_map", _vp), ("error_cells", _vp),
                ("depth", _vp), ("image", _vp), ("sample_index", _vp)]


class SamnerfBatchSource(ctypes.Structure):
    """samnerf_batch_source (include/samnerf_hip.h)."""
    _fields_ = [("poses", _vp), ("intrinsics", _vp), ("n_img", _u32), ("n_intr", _u32), ("H", _u32), ("W", _u32),
                ("images", _vp), ("C", _u32), ("images_float", ctypes.c_int32), ("masks", _vp),
                ("incoherent_masks", _vp), ("incoherent_bytes", _u32), ("incoherent_size", _u32),
                ("error_map", _vp), ("error_size", _u32), ("cam_near_far", _vp)]


class SamnerfBatchOut(ctypes.Structure):
    """samnerf_batch_out (include/samnerf_hip.h)."""
    _fields_ = [(k, _vp) for k in ("rays_o", "rays_d", "i", "j", "inds_coarse", "images", "masks",
                                   "incoherent_masks", "error_maps", "cam_near_far")]


class SamnerfBatchDrawArgs(ctypes.Structure):
    """samnerf_batch_draw_args (include/samnerf_hip.h)."""
    _fields_ = [("mode", ctypes.c_int32), ("seeded", ctypes.c_int32), ("seed", _u64), ("offset", _u64),
                ("n_img", _u32), ("H", _u32), ("W", _u32), ("n", _u32), ("patch", _u32), ("M", _u32),
                ("weights", _vp), ("weight_bytes", _u32), ("rows", _vp), ("int0", _vp), ("int1", _vp),
                ("keys", _vp), ("u0", _vp), ("u1", _vp), ("index", _vp), ("pixels", _vp), ("cells", _vp)]


class SamnerfPresentArgs(ctypes.Structure):
    """samnerf_present_args (include/samnerf_hip.h)."""
    _fields_ = [("rH", _u32), ("rW", _u32), ("H", _u32), ("W", _u32), ("K", _u32), ("n_inst", _u32),
                ("n_colors", _u32), ("n_points", _u32), ("spp", _u32), ("mask_type", ctypes.c_int32),
                ("instance_id", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("image", _vp), ("depth", _vp), ("logits", _vp), ("color_map", _vp), ("sam_mask", _vp),
                ("points", _vp), ("buffer", _vp), ("probs", _vp), ("ids", _vp), ("depth_out", _vp)]


class SamnerfEvalArgs(ctypes.Structure):
    """samnerf_eval_args (include/samnerf_hip.h)."""
    _fields_ = [("H", _u32), ("W", _u32), ("C", _u32), ("ssim", _u32), ("K", _u32), ("n_inst", _u32),
                ("n_classes", _u32), ("h", _u32), ("w", _u32), ("bg_color", _f32), ("epsilon", _f64),
                ("pred_rgb", _vp), ("truth", _vp), ("logits", _vp), ("labels", _vp), ("pred_feat", _vp),
                ("gt_feat", _vp), ("pred_u8", _vp), ("truth_u8", _vp), ("error_u8", _vp), ("truth_out", _vp),
                ("probs", _vp), ("ids", _vp), ("stats", _vp), ("workspace", _vp), ("workspace_bytes", _sz)]


class SamnerfIncoherentIdsArgs(ctypes.Structure):
    """samnerf_incoherent_ids_args (include/samnerf_hip.h)."""
    _fields_ = [("N", _u32), ("K", _u32), ("n_inst", _u32), ("logits", _vp), ("ids", _vp), ("pred_mask", _vp)]


class SamnerfIncoherentMasksArgs(ctypes.Structure):
    """samnerf_incoherent_masks_args (include/samnerf_hip.h)."""
    _fields_ = [("n", _u32), ("H", _u32), ("W", _u32), ("sfact", _u32), ("keep_size", ctypes.c_int32),
                ("input_type", ctypes.c_int32), ("masks", _vp), ("table", _vp), ("uncertain", _vp)]


_SIGS = {
    "samnerf_diag_variants": ([], _int),
    "samnerf_version": ([], ctypes.c_char_p),
    "samnerf_last_error": ([], ctypes.c_char_p),
    "samnerf_grid_encode_forward": ([_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _f32, _u32,
                                     _vp, _u32, _int, _u32, _vp], _int),
    "samnerf_grid_encode_backward": ([_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _f32,
                                      _u32, _vp, _vp, _u32, _int, _u32, _vp], _int),
    "samnerf_grad_total_variation": ([_vp, _vp, _vp, _vp, _f32, _u32, _u32, _u32, _u32, _f32, _u32,
                                      _u32, _int, _vp], _int),
    "samnerf_grad_weight_decay": ([_vp, _vp, _vp, _f32, _u32, _u32, _u32, _vp], _int),
    "samnerf_sh_encode_forward": ([_vp, _vp, _u32, _u32, _u32, _vp, _vp], _int),
    "samnerf_sh_encode_backward": ([_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp], _int),
    "samnerf_freq_encode_forward": ([_vp, _u32, _u32, _u32, _u32, _vp, _vp], _int),
    "samnerf_freq_encode_backward": ([_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp], _int),
    "samnerf_get_rays": ([ctypes.POINTER(_f32), _f32, _f32, _f32, _f32, _u32, _u32, _u32, _u32,
                          _vp, _vp, _vp], _int),
    "samnerf_near_far": ([_vp, _vp, _u32, ctypes.POINTER(_f32), _f32, _vp, _vp, _vp], _int),
    "samnerf_contract": ([_vp, _vp, _u32, _vp], _int),
    "samnerf_sample_pdf": ([_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp], _int),
    "samnerf_composite_weights": ([_vp, _vp, _u32, _u32, _vp, _vp], _int),
    "samnerf_linspace_host": ([_f32, _f32, _u32, ctypes.POINTER(_f32)], None),
    "samnerf_perturb_host": ([_u64, _u64, ctypes.POINTER(_u32), _u32, _u32, ctypes.POINTER(_f32)], _int),
    "samnerf_perturb_fill": ([_u64, _u64, _u32, ctypes.POINTER(_u32), _vp, _vp, _vp, _vp], _int),
    "samnerf_set_background": ([ctypes.POINTER(SamnerfBackground)], _int),
    "samnerf_render_workspace_size": ([ctypes.POINTER(SamnerfModel), _u32], _sz),
    "samnerf_render_forward": ([ctypes.POINTER(SamnerfModel), _vp, _vp, _u32, _vp, _u32, _f32,
                                _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp], _int),
    "samnerf_render_forward_tile": ([ctypes.POINTER(SamnerfModel), _vp, _vp, _u32, _vp, _u32, _f32,
                                     _vp, _u32, _int, _vp, _vp, _sz, _vp], _int),
    "samnerf_sgrid_backward": ([ctypes.POINTER(SamnerfModel), _vp, _u32, _vp, _vp, _sz, _vp],
                               _int),
    "samnerf_sgrid_accum_size": ([ctypes.POINTER(SamnerfModel)], _sz),
    "samnerf_sgrid_backward_det": ([ctypes.POINTER(SamnerfModel), _vp, _u32, _vp, _vp, _sz, _vp, _sz, _vp],
                                   _int),
    "samnerf_mask_forward": ([ctypes.POINTER(SamnerfModel), _u32, _vp, _vp, _sz, _vp], _int),
    "samnerf_tile_words": ([], _u32),
    "samnerf_tile_encode": ([_vp, _vp, _vp, _vp, _u32, _vp, _vp], _int),
    "samnerf_tile_decode": ([_vp, _u32, _vp, _vp, _vp, _vp, _vp], _int),
    "samnerf_set_stage_events": ([ctypes.POINTER(_vp), _u32], _int),
    "samnerf_set_taps": ([ctypes.c_void_p, _u32], _int),
    "samnerf_last_forms": ([ctypes.c_void_p, _u32], _int),
    "samnerf_clock_stamp": ([_vp, _vp], _int),
    "samnerf_adam_step": ([ctypes.c_void_p, _u32, _f64, _f64, _f64, _f64, _f64, _u32, _vp], _int),
    "samnerf_rgb_train_workspace_size": ([ctypes.POINTER(SamnerfModel), _u32], _sz),
    "samnerf_rgb_train_step": ([ctypes.POINTER(SamnerfModel), _vp, _vp, _u32, _vp, _u32, _vp,
                                ctypes.c_void_p, _vp, _vp, _vp, _vp, ctypes.c_void_p, _vp, _sz, _vp], _int),
    "samnerf_rgb_train_forward": ([ctypes.POINTER(SamnerfModel), _vp, _vp, _u32, _vp, _u32, _f32, _int,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp], _int),
    "samnerf_rgb_train_backward": ([ctypes.POINTER(SamnerfModel), _vp, _vp, _u32, _f32, _int, _vp, _vp,
                                    _vp, _vp, _vp, ctypes.c_void_p, _vp, _sz, _vp], _int),
    "samnerf_sam_head_workspace_size": ([], _sz),
    "samnerf_sam_head_forward": ([ctypes.POINTER(SamnerfModel), _vp, _u32, _vp, _vp, _sz, _vp], _int),
    "samnerf_head_train_workspace_size": ([_u32], _sz),
    "samnerf_head_train_forward": ([ctypes.POINTER(SamnerfModel), _vp, _u32, _vp, _vp, _sz, _vp], _int),
    "samnerf_head_train_backward": ([ctypes.POINTER(SamnerfModel), _vp, _vp, _u32, _vp,
                                     ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp, _sz,
                                     _vp], _int),
    "samnerf_mask_train_workspace_size": ([_u32], _sz),
    "samnerf_mask_train_workspace_size_model": ([ctypes.POINTER(SamnerfModel), _u32], _sz),
    "samnerf_mask_train_forward": ([ctypes.POINTER(SamnerfModel), _u32, _vp, _vp, _sz, _vp, _sz, _vp], _int),
    "samnerf_mask_train_backward": ([ctypes.POINTER(SamnerfModel), _u32, _vp, ctypes.POINTER(_vp), _vp, _vp,
                                     _sz, _vp, _sz, _vp], _int),
    "samnerf_mask_loss_workspace_size": ([ctypes.POINTER(SamnerfMaskLossArgs)], _sz),
    "samnerf_mask_loss": ([ctypes.POINTER(SamnerfMaskLossArgs), _vp, _vp, _vp, _vp, _vp, _sz, _vp], _int),
    "samnerf_batch_gather": ([ctypes.POINTER(SamnerfBatchSource), _vp, _u32, _vp, _u32, _u32, _u32, _u32,
                              ctypes.POINTER(SamnerfBatchOut), _vp], _int),
    "samnerf_batch_draw": ([ctypes.POINTER(SamnerfBatchDrawArgs), _vp], _int),
    "samnerf_batch_draw_fill": ([_u64, _u64, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32,
                                 _u32, _vp, _vp], _int),
    "samnerf_batch_draw_host": ([_u64, _u64, _u32, _u32, _u32, ctypes.POINTER(ctypes.c_int64),
                                 ctypes.POINTER(_f32)], _int),
    "samnerf_present_workspace_size": ([ctypes.POINTER(SamnerfPresentArgs)], _sz),
    "samnerf_present_frame": ([ctypes.POINTER(SamnerfPresentArgs), _vp, _sz, _vp], _int),
    "samnerf_eval_workspace_size": ([ctypes.POINTER(SamnerfEvalArgs), ctypes.POINTER(_sz)], _int),
    "samnerf_eval_frame": ([ctypes.POINTER(SamnerfEvalArgs), _vp], _int),
    "samnerf_eval_confusion": ([_vp, _vp, _u32, _u32, _vp, _vp], _int),
    "samnerf_incoherent_ids": ([ctypes.POINTER(SamnerfIncoherentIdsArgs), _vp], _int),
    "samnerf_incoherent_masks": ([ctypes.POINTER(SamnerfIncoherentMasksArgs), _vp], _int),
    "samnerf_feat_loss_workspace_size": ([_u32, _u32, _u32, _u32], _sz),
    "samnerf_feat_loss_forward": ([_vp, _u32, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _sz, _vp], _int),
    "samnerf_feat_loss_backward": ([_vp, _u32, _u32, _u32, _u32, _vp, _vp, _sz, _vp], _int),
    "samnerf_bilinear_taps_host": ([_u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                    ctypes.POINTER(_f32)], _int),
    "samnerf_teacher_image_shape": ([_u32, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32)], _int),
    "samnerf_teacher_image_workspace_size": ([_u32, _u32, _u32, _u32], _sz),
    "samnerf_teacher_image": ([_vp, _u32, _u32, _u32, _u32, _u32, ctypes.POINTER(_f32), ctypes.POINTER(_f32),
                               _vp, _vp, _vp, _sz, _vp], _int),
    "samnerf_sam_decoder_raw_count": ([], _sz),
    "samnerf_sam_decoder_pack_size": ([_u32], _sz),
    "samnerf_sam_decoder_pack": ([_vp, _sz, _u32, _vp, _sz, _vp], _int),
    "samnerf_sam_decoder_workspace_size": ([_u32], _sz),
    "samnerf_sam_decoder": ([_vp, _sz, _u32, _vp, _u32, _u32, ctypes.POINTER(ctypes.c_int32),
                             ctypes.POINTER(ctypes.c_int32), _u32, _vp, _vp, _vp, _sz, _vp], _int),
    "samnerf_sam_decoder_launches": ([], _int),
    "samnerf_sam_masks": ([_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp], _int),
    "samnerf_sam_decoder_batch_workspace_size": ([_u32, _u32], _sz),
    "samnerf_sam_decoder_batch": ([_vp, _sz, _u32, _vp, _u32, _u32, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _sz, _vp],
                                  _int),
    "samnerf_sam_masks_select": ([_vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _f32, _vp, _vp, _vp],
                                 _int),
    "samnerf_sam_mask_stats": ([_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _f32, _f32, _f32, _f32, _vp, _vp],
                               _int),
    "samnerf_sam_nms": ([_vp, _u32, _f32, _vp, _vp, _vp], _int),
}


class SamnerfAdamTensor(ctypes.Structure):
    """samnerf_adam_tensor (include/samnerf_hip.h)."""
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp),
                ("n", ctypes.c_uint64)]


class SamnerfTaps(ctypes.Structure):
    """samnerf_taps (include/samnerf_hip.h): parity-test taps of the render."""
    _fields_ = [("ds0", _vp), ("ds1", _vp), ("w0", _vp), ("w1", _vp), ("bins1", _vp),
                ("bins2", _vp), ("inds1", _vp), ("inds2", _vp), ("sigma2", _vp), ("w2", _vp),
                ("u2", _vp), ("row_stride", _u32), ("rows2", _vp), ("srows", _vp)]


class SamnerfRgbTrainOpts(ctypes.Structure):
    """samnerf_rgb_train_opts (include/samnerf_hip.h)."""
    _fields_ = [("lambda_proposal", _f32), ("lambda_distort", _f32), ("lambda_entropy", _f32),
                ("update_proposal", _int), ("bg_color", _f32)]


class SamnerfRgbGrads(ctypes.Structure):
    """samnerf_rgb_grads (include/samnerf_hip.h)."""
    _fields_ = [("grid", _vp), ("grid_mlp", _vp * 3), ("view_mlp", _vp * 3), ("prop", _vp * 2),
                ("prop_mlp", (_vp * 2) * 2)]


EXPORTED = tuple(_SIGS)
_lib = None


def _load(path, lenient=False):
    if not os.path.exists(path):
        raise SamnerfUnavailable(
            f"{path} is not built; run `python segment-anything-nerf_amd/build.py` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    try:
        L = ctypes.CDLL(path)
    except OSError as e:
        raise SamnerfUnavailable(f"cannot load {path}: {e}") from e
    for name, (args, res) in _SIGS.items():
        if lenient and not hasattr(L, name):
            continue                  # an older diagnostic build (tools/diag) lacks newer entry points
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    return L


def lib():
    """Load the HIP library (once).  Raises SamnerfUnavailable if absent."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, lenient=bool(os.environ.get("SAMNERF_LIB")))
    return _lib


DIAG_LIB_PATH = os.path.join(_HERE, "libsamnerf_hip_diag.so")
_diag = None


@contextlib.contextmanager
def diag_library():
    """Tests and tools only: while the context is active, EVERY call of the
    process (all threads: the swap is of the module-global library handle)
    goes through the diagnostic build (libsamnerf_hip_diag.so), whose kernels
    read the A/B variant switches (SAMNERF_LOOKUP, SAMNERF_FINAL_S, ...) from
    the environment -- the product library has one path per configuration.
    Not for use while product renders run on other threads."""
    global _lib, _diag
    if _diag is None:
        _diag = _load(DIAG_LIB_PATH)
        assert _diag.samnerf_diag_variants() == 1
    prev = lib()
    _lib = _diag
    try:
        yield _diag
    finally:
        _lib = prev


def check(rc, what):
    if rc != 0:
        msg = lib().samnerf_last_error().decode(errors="replace")
        raise RuntimeError(f"{what}: {msg} (code {rc})")


def last_error():
    return lib().samnerf_last_error().decode(errors="replace")
