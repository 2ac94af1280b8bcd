"""ctypes binding of ``libffcv_hip.so`` (include/ffcv_hip.h).

Replaces the reference's ``ffcv/libffcv.py`` (CDLL of ``ffcv._libffcv``,
ffcv/libffcv.py:8-55).  The reference binds one-sample CPU functions
(``resize``, ``imdecode``, ``my_memcpy``) called from numba ``prange``
workers.  This binding exposes the batch/device ABI: every call enqueues HIP
work on the caller's stream (``torch.cuda.current_stream().cuda_stream`` is a
``hipStream_t`` on ROCm) and takes device pointers (``tensor.data_ptr()``).

The library is built in-tree (``python -m ffcv_amd._build``).  There is no CPU
fallback for any compute entry point: if the shared object is missing this
module raises at import of the compute functions.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libffcv_hip.so')

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_int32 = ctypes.c_int32
c_uint32 = ctypes.c_uint32
c_uint64 = ctypes.c_uint64
c_int64 = ctypes.c_int64
c_double = ctypes.c_double
c_float = ctypes.c_float

# per-sample device status codes (FFCV_SAMPLE_*)
SAMPLE_STATUS = {0: 'ok', 1: 'bad marker', 2: 'unsupported JPEG feature',
                 3: 'image larger than decoder context', 4: 'corrupt entropy stream',
                 5: 'geometry mismatch', 6: 'rng stream exhausted', 7: 'label outside [0, num_classes)',
                 8: 'sample index or row outside the dataset bytes'}


class FFCVError(RuntimeError):
    pass


class Sample(ctypes.Structure):
    """ffcv_sample (32 bytes)."""
    _fields_ = [('offset', c_uint64), ('size', c_uint64), ('height', c_uint32),
                ('width', c_uint32), ('mode', c_uint32), ('reserved', c_uint32)]


SAMPLE_DTYPE = np.dtype([('offset', '<u8'), ('size', '<u8'), ('height', '<u4'),
                         ('width', '<u4'), ('mode', '<u4'), ('reserved', '<u4')])
assert SAMPLE_DTYPE.itemsize == ctypes.sizeof(Sample) == 32


class RRCParams(ctypes.Structure):
    _fields_ = [('out_h', c_int32), ('out_w', c_int32), ('cutout_size', c_int32),
                ('cutout_fill', ctypes.c_uint8 * 4), ('lut', c_void_p),
                ('out_stride', c_uint64)]


class DrawParams(ctypes.Structure):
    _fields_ = [('crop_kind', c_int32), ('out_h', c_int32), ('out_w', c_int32),
                ('cutout_size', c_int32), ('scale', ctypes.c_double * 2),
                ('ratio', ctypes.c_double * 2), ('center_ratio', ctypes.c_double),
                ('loader_seed', c_uint64), ('epoch', c_uint64),
                ('flip_prob', ctypes.c_double)]


# ffcv_simple_aug_params steps (FFCV_AUG_*)
AUG_FLIP, AUG_TRANSLATE, AUG_CUTOUT = 1, 2, 3


class SimpleAugParams(ctypes.Structure):
    _fields_ = [('n_steps', c_int32), ('steps', ctypes.c_uint8 * 4), ('padding', c_int32),
                ('cutout_size', c_int32), ('translate_fill', ctypes.c_uint8 * 4),
                ('cutout_fill', ctypes.c_uint8 * 4)]


class ColorJitterParams(ctypes.Structure):
    """ffcv_color_jitter_params: FFCV_CJ_* kinds in pipeline order."""
    _fields_ = [('n_steps', c_int32), ('steps', ctypes.c_uint8 * 4)]


class ToneParams(ctypes.Structure):
    """ffcv_tone_params: FFCV_TONE_* kinds in pipeline order, posterize's bits."""
    _fields_ = [('n_steps', c_int32), ('steps', ctypes.c_uint8 * 4), ('bits', c_int32)]


_lib = None

_SIGS = {
    'ffcv_abi_version': (c_int, []),
    'ffcv_last_error': (ctypes.c_char_p, []),
    'ffcv_device_count': (c_int, [c_void_p]),
    'ffcv_set_device': (c_int, [c_int]),
    'ffcv_stream_synchronize': (c_int, [c_void_p]),
    'ffcv_malloc': (c_int, [c_void_p, c_uint64]),
    'ffcv_free': (c_int, [c_void_p]),
    'ffcv_memcpy_h2d_async': (c_int, [c_void_p, c_void_p, c_uint64, c_void_p]),
    'ffcv_memcpy_d2h_async': (c_int, [c_void_p, c_void_p, c_uint64, c_void_p]),
    'my_memcpy': (None, [c_void_p, c_void_p, c_uint64]),
    'my_fread': (None, [ctypes.c_int64, ctypes.c_int64, c_void_p, ctypes.c_int64]),
    'resize': (None, [ctypes.c_int64] * 11),
    'imdecode': (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32,
                         c_uint32, c_uint32, c_uint32, c_uint32, ctypes.c_bool, ctypes.c_bool]),
    'ffcv_cpu_decode_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                      c_int, c_void_p, c_uint64, c_int, c_void_p]),
    'ffcv_imdecode_device': (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32,
                                     c_uint32, c_uint32, c_uint32, c_uint32, ctypes.c_bool, ctypes.c_bool]),
    'ffcv_host_gather': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int]),
    'ffcv_draw_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    'ffcv_draw_batch_host': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    'ffcv_rrc_raw_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    'ffcv_rrc_raw_batch_ws': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_uint64]),
    'ffcv_rrc_raw_workspace_bytes': (c_uint64, [c_int, c_int, c_int]),
    'ffcv_gather_samples': (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_void_p]),
    'ffcv_gather_raw_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_uint64]),
    'ffcv_gather_rows': (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_int, c_uint64,
                                 c_void_p, c_uint64, c_void_p]),
    'ffcv_gather_rows_cutover': (c_uint64, []),
    'ffcv_gather_rows_subwave': (c_uint64, []),
    'ffcv_jpeg_scan_stats': (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    'ffcv_jpeg_create': (c_int, [c_void_p, c_int, c_uint32, c_uint32, c_uint64]),
    'ffcv_jpeg_destroy': (c_int, [c_void_p]),
    'ffcv_jpeg_create_arena': (c_int, [c_void_p, c_int, c_uint32, c_uint32, c_uint64, c_uint64]),
    'ffcv_jpeg_scratch_bound': (c_uint64, [c_uint32, c_uint32, c_uint64]),
    'ffcv_jpeg_set_diag': (c_int, [c_void_p, c_int, c_int]),
    'ffcv_jpeg_arena_used': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    'ffcv_jpeg_set_entropy_index': (c_int, [c_void_p, c_void_p, c_uint64]),
    'ffcv_jpeg_set_timing': (c_int, [c_void_p, c_int]),
    'ffcv_jpeg_timing_read': (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    'ffcv_jpeg_rrc_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ffcv_jpeg_rrc_fused': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p,
                                    c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    'ffcv_jpeg_decode_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                       c_uint64, c_void_p]),
    'ffcv_jpeg_coefficients_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                             c_void_p, c_uint64, c_void_p]),
    'ffcv_cutout_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int,
                                  c_void_p]),
    'ffcv_normalize_batch': (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
    'ffcv_lut_batch': (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_void_p]),
    'ffcv_flip_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                c_void_p]),
    'ffcv_translate_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_int, c_void_p,
                                          c_void_p]),
    'ffcv_translate_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_int, c_void_p]),
    'ffcv_translate_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int,
                                     c_void_p]),
    'ffcv_crop_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_uint64, c_uint64,
                                     c_void_p, c_void_p]),
    'ffcv_crop_draw_batch_host': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_uint64, c_uint64,
                                          c_void_p, c_void_p]),
    'ffcv_rrc_images_batch': (c_int, [c_void_p, c_void_p, c_uint64, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64]),
    'ffcv_rrc_images_workspace_bytes': (c_uint64, [c_int, c_int, c_int, c_int, c_int]),
    'ffcv_rrc_images_lds_bytes': (c_uint64, []),
    'ffcv_rrc_images_batch_host': (c_int, [c_void_p, c_uint64, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                           c_void_p, c_uint64, c_void_p, c_int]),
    'ffcv_simple_aug_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_uint64]),
    'ffcv_color_jitter_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_int, c_double,
                                             c_double, c_void_p, c_void_p, c_void_p]),
    'ffcv_color_jitter_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_int, c_double, c_double,
                                                  c_void_p, c_void_p]),
    'ffcv_color_jitter_workspace_bytes': (c_uint64, [c_int]),
    'ffcv_color_jitter_lds_bytes': (c_uint64, []),
    'ffcv_color_jitter_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_uint64]),
    'ffcv_color_jitter_batch_host': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'ffcv_uniform_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_int, c_double, c_double,
                                        c_double, c_void_p, c_void_p, c_void_p]),
    'ffcv_uniform_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_int, c_double, c_double, c_double,
                                             c_void_p, c_void_p]),
    'ffcv_blur_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_double, c_double, c_double,
                                     c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'ffcv_blur_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_double, c_double, c_double, c_int,
                                          c_void_p, c_void_p, c_void_p]),
    'ffcv_gaussian_blur_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                         c_void_p, c_uint64]),
    'ffcv_gaussian_blur_batch_host': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                              c_uint64, c_int]),
    'ffcv_gaussian_blur_lds_bytes': (c_uint64, []),
    'ffcv_gaussian_blur_band_rows': (c_uint64, []),
    'ffcv_gaussian_blur_strip_cols': (c_uint64, [c_int, c_int, c_int]),
    'ffcv_sharpness_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_double, c_double,
                                          c_void_p, c_void_p, c_void_p]),
    'ffcv_sharpness_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_double, c_double, c_void_p,
                                               c_void_p]),
    'ffcv_sharpness_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_uint64]),
    'ffcv_sharpness_batch_host': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_uint64,
                                          c_int]),
    'ffcv_tone_batch_bits': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_uint64,
                                     c_void_p]),
    'ffcv_tone_batch_bits_host': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'ffcv_policy_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_int, c_void_p, c_int, c_int] +
                               [c_void_p] * 10),
    'ffcv_policy_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_int, c_void_p, c_int, c_int] +
                                    [c_void_p] * 9),
    'ffcv_sharpness_lds_bytes': (c_uint64, []),
    'ffcv_sharpness_band_rows': (c_uint64, []),
    'ffcv_sharpness_strip_cols': (c_uint64, [c_int, c_int]),
    'ffcv_hue_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_double, c_double, c_void_p,
                                    c_void_p, c_void_p]),
    'ffcv_hue_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_double, c_double, c_void_p,
                                         c_void_p]),
    'ffcv_color_jitter_joint_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_double, c_void_p,
                                                   c_void_p, c_void_p, c_void_p]),
    'ffcv_color_jitter_joint_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_double, c_void_p,
                                                        c_void_p, c_void_p]),
    'ffcv_hue_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'ffcv_hue_batch_host': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'ffcv_tone_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    'ffcv_tone_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_void_p]),
    'ffcv_tone_workspace_bytes': (c_uint64, [c_int]),
    'ffcv_tone_lds_bytes': (c_uint64, []),
    'ffcv_tone_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_uint64]),
    'ffcv_tone_batch_host': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'ffcv_tone_tables_host': (c_int, [c_int, c_int, c_void_p, c_void_p, c_int]),
    'ffcv_affine_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_double, c_void_p, c_int,
                                       c_int, c_void_p, c_void_p, c_void_p]),
    'ffcv_affine_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_double, c_void_p, c_int, c_int,
                                            c_void_p, c_void_p]),
    'ffcv_affine_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p, c_uint64]),
    'ffcv_affine_batch_host': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_uint64, c_int]),
    'ffcv_affine_whole_bytes': (c_uint64, []),
    'ffcv_affine_tile_rows': (c_uint64, []),
    'ffcv_affine_tile_cols': (c_uint64, []),
    'ffcv_affine_tile_lds': (c_uint64, []),
    'ffcv_affine_tile_bytes': (c_uint64, [c_int, c_int, c_int, c_void_p, c_int, c_int]),
    'ffcv_mixup_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p, c_int]),
    'ffcv_mixup_batch_host': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p, c_int,
                                      c_int]),
    'ffcv_mixup_onehot_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    'ffcv_poison_batch': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_float, c_float]),
    'ffcv_poison_batch_host': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_float, c_float, c_int]),
    'ffcv_replace_label_batch': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                         c_int64]),
    'ffcv_cutmix_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int64,
                                  c_void_p, c_int]),
    'ffcv_cutmix_batch_host': (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int64,
                                       c_void_p, c_int, c_int]),
    'ffcv_erase_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_double, c_void_p, c_void_p,
                                      c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'ffcv_erase_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_double, c_void_p, c_void_p, c_int,
                                           c_int, c_void_p, c_void_p]),
    'ffcv_erase_batch': (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int,
                                 c_int32, c_void_p, c_void_p]),
    'ffcv_erase_batch_host': (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int, c_int32,
                                      c_void_p, c_void_p, c_int]),
    'ffcv_randaugment_draw_batch': (c_int, [c_void_p, c_void_p, c_int, c_uint64, c_uint64, c_int, c_int, c_int,
                                            c_void_p, c_int, c_int] + [c_void_p] * 10),
    'ffcv_randaugment_draw_batch_host': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_int, c_int, c_int, c_void_p,
                                                 c_int, c_int] + [c_void_p] * 9),
    'ffcv_randaugment_lds_bytes': (c_uint64, []),
    'ffcv_randaugment_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p] +
                               [c_void_p] * 9),
}

EXPORTED_SYMBOLS = tuple(_SIGS)


def lib():
    """Load libffcv_hip.so (raises if it was not built -- no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FFCVError(f'{LIB_PATH} is missing: build it with `python -m ffcv_amd._build` '
                            '(there is no CPU fallback for the decode path)')
        # Load torch's HIP runtime first: libffcv_hip.so's NEEDED
        # libamdhip64.so.7 then binds to the runtime torch already uses
        # (same soname), so tensors and our kernels share one HIP runtime.
        # Loading ours first would pull /opt/rocm's copy and give the process
        # two runtimes ("no ROCm-capable device" in the second).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        if l.ffcv_abi_version() != 1:
            raise FFCVError('libffcv_hip.so ABI version mismatch')
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = lib().ffcv_last_error().decode(errors='replace')
        raise FFCVError(f'{what} failed ({rc}): {msg}')


def _p(x):
    """Device/host pointer of a torch tensor, numpy array, int or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return c_void_p(x)
    if hasattr(x, 'data_ptr'):
        return c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        return c_void_p(x.ctypes.data)
    raise TypeError(type(x))


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return c_void_p(stream.cuda_stream if hasattr(stream, 'cuda_stream') else int(stream))


# ----------------------------------------------------------------- wrappers
def memcpy_h2d_async(dst, src, nbytes: int, stream):
    """hipMemcpyAsync host -> device on ``stream`` (pinned ``src``): one
    library call instead of a torch copy dispatch inside a stream context."""
    _check(lib().ffcv_memcpy_h2d_async(_p(dst), _p(src), int(nbytes), _stream(stream)), 'ffcv_memcpy_h2d_async')


def memcpy_d2h_async(dst, src, nbytes: int, stream):
    """hipMemcpyAsync device -> host on ``stream`` (pinned ``dst``)."""
    _check(lib().ffcv_memcpy_d2h_async(_p(dst), _p(src), int(nbytes), _stream(stream)), 'ffcv_memcpy_d2h_async')


def memcpy(source: np.ndarray, dest: np.ndarray):
    """ffcv/libffcv.py:51-55 memcpy (host plumbing)."""
    lib().my_memcpy(source.ctypes.data, dest.ctypes.data, source.size * source.itemsize)


# --------------------------------------- reference one-sample host API --
# ffcv/libffcv.py:11-48: read (libc pread), resize_crop, imdecode, same
# names and argument meaning, for Operations written against the reference.
_libc = None


def read(fileno: int, destination: np.ndarray, offset: int):
    """pread(fileno, destination, destination.size, offset) (libffcv.py:11-19)."""
    global _libc
    if _libc is None:
        _libc = ctypes.CDLL('libc.so.6', use_errno=True)
        _libc.pread.restype = ctypes.c_ssize_t
        _libc.pread.argtypes = [c_int, c_void_p, ctypes.c_size_t, ctypes.c_int64]
    return _libc.pread(int(fileno), destination.ctypes.data, destination.size, int(offset))


def resize_crop(source, start_row, end_row, start_col, end_col, destination):
    """INTER_AREA resize of source[start_row:end_row, start_col:end_col]
    (HWC uint8) into destination (its shape is the target), libffcv.py:22-31."""
    source = np.asarray(source)
    if source.dtype != np.uint8 or destination.dtype != np.uint8 or not source.flags.c_contiguous \
            or not destination.flags.c_contiguous:
        raise ValueError('resize_crop: source and destination must be C-contiguous uint8 HWC arrays')
    lib().resize(0, source.ctypes.data, source.shape[0], source.shape[1], int(start_row), int(end_row),
                 int(start_col), int(end_col), destination.ctypes.data, destination.shape[0],
                 destination.shape[1])


def imdecode(source: np.ndarray, dst: np.ndarray, source_height: int, source_width: int,
             crop_height=None, crop_width=None, offset_x=0, offset_y=0, scale_factor_num=1,
             scale_factor_denom=1, enable_crop=False, do_flip=False):
    """Decode one JPEG (host bytes) into dst (host HWC uint8), libffcv.py:34-48,
    on the CPU like the reference.  Returns 0 or -1 like tjDecompress2."""
    return _imdecode(lib().imdecode, source, dst, source_height, source_width, crop_height, crop_width,
                     offset_x, offset_y, scale_factor_num, scale_factor_denom, enable_crop, do_flip)


def imdecode_device(source: np.ndarray, dst: np.ndarray, source_height: int, source_width: int,
                    crop_height=None, crop_width=None, offset_x=0, offset_y=0, scale_factor_num=1,
                    scale_factor_denom=1, enable_crop=False, do_flip=False):
    """imdecode executed by the gfx950 JPEG kernels (host buffers in and out)."""
    return _imdecode(lib().ffcv_imdecode_device, source, dst, source_height, source_width, crop_height,
                     crop_width, offset_x, offset_y, scale_factor_num, scale_factor_denom, enable_crop, do_flip)


def _imdecode(fn, source, dst, source_height, source_width, crop_height, crop_width, offset_x, offset_y,
              scale_factor_num, scale_factor_denom, enable_crop, do_flip):
    if crop_height is None:
        crop_height = source_height
    if crop_width is None:
        crop_width = source_width
    return fn(source.ctypes.data, source.size, int(source_height), int(source_width),
              dst.ctypes.data, int(crop_height), int(crop_width), int(offset_x), int(offset_y),
              int(scale_factor_num), int(scale_factor_denom), bool(enable_crop), bool(do_flip))


def jpeg_scan_stats(images):
    """(symbols, blocks, entropy-coded bytes) per JPEG, uint64 (n, 3), from the
    CPU decoder's Huffman loop (ffcv_jpeg_scan_stats); rows of images that
    do not parse are zero."""
    images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    n = len(images)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    sizes = np.array([im.size for im in images], dtype=np.uint64)
    stats = np.zeros((max(n, 1), 3), dtype=np.uint64)
    rc = lib().ffcv_jpeg_scan_stats(ptrs.ctypes.data, sizes.ctypes.data, n, stats.ctypes.data)
    if rc not in (0, -1):
        raise RuntimeError('ffcv_jpeg_scan_stats: ' + lib().ffcv_last_error().decode(errors='replace'))
    return stats[:n]


def cpu_jpeg_coefficients(image):
    """int16 (blocks, 64): every coded block of one JPEG in scan order, natural
    order with the absolute DC, from the CPU decoder (a test helper; bound on
    first use, so that a library of an earlier revision still loads)."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    fn = lib().ffcv_cpu_jpeg_coefficients
    fn.restype = ctypes.c_int
    fn.argtypes = [c_void_p, c_uint64, c_void_p, c_uint64, c_void_p]
    n = ctypes.c_uint64()
    out = np.zeros((1, 64), np.int16)
    for cap in (0, None):  # count the blocks, then read them
        cap = n.value if cap is None else cap
        out = np.zeros((max(cap, 1), 64), np.int16)
        if fn(image.ctypes.data, image.size, out.ctypes.data, cap, ctypes.byref(n)):
            raise RuntimeError(lib().ffcv_last_error().decode(errors='replace'))
    return out[:n.value]


def cpu_decode_batch(images, heights, widths, modes, out: np.ndarray, crops=None, nthreads=1):
    """The reference's per-sample CPU decode loop as one native call
    (ffcv_cpu_decode_batch): images[k] are host uint8 arrays (JPEG bytes or
    raw HWC pixels), out is [B, ...] C-contiguous uint8 (the sample's whole
    image, or its crops[k] resized to out.shape[1:3]).  Returns the status
    array (0 / -1 per sample)."""
    B = len(images)
    ptrs = np.array([im.ctypes.data if im is not None else 0 for im in images], np.uint64)
    sizes = np.array([im.size if im is not None else 0 for im in images], np.uint64)
    hs = np.ascontiguousarray(heights, np.uint32)
    ws = np.ascontiguousarray(widths, np.uint32)
    ms = np.ascontiguousarray(modes, np.uint32)
    status = np.zeros(B, np.int32)
    if not out.flags['C_CONTIGUOUS'] or out.dtype != np.uint8:
        raise ValueError('cpu_decode_batch: out must be C-contiguous uint8')
    stride = out[0].nbytes if B else 0
    cr = None
    oh = ow = 0
    if crops is not None:
        cr = np.ascontiguousarray(crops, np.int32)
        oh, ow = int(out.shape[1]), int(out.shape[2])
    rc = lib().ffcv_cpu_decode_batch(ptrs.ctypes.data, sizes.ctypes.data, hs.ctypes.data, ws.ctypes.data,
                                     ms.ctypes.data, B, cr.ctypes.data if cr is not None else None, oh, ow,
                                     out.ctypes.data, stride, int(max(1, nthreads)), status.ctypes.data)
    if rc != 0:
        raise RuntimeError('ffcv_cpu_decode_batch: ' + lib().ffcv_last_error().decode(errors='replace'))
    return status


def host_gather(src: np.ndarray, src_off: np.ndarray, sizes: np.ndarray, dst_off: np.ndarray, dst,
                nthreads=8):
    """Gather byte ranges of a host buffer (e.g. the mmap) into dst (numpy / pinned tensor)."""
    so = np.ascontiguousarray(src_off, dtype=np.uint64)
    sz = np.ascontiguousarray(sizes, dtype=np.uint64)
    do = np.ascontiguousarray(dst_off, dtype=np.uint64)
    _check(lib().ffcv_host_gather(_p(src), _p(so), _p(sz), _p(do), int(len(sz)), _p(dst), int(nthreads)),
           'ffcv_host_gather')


def draw_batch(ids, samples, params: DrawParams, crops=None, cutout_yx=None, flips=None,
               status=None, stream=None):
    _check(lib().ffcv_draw_batch(_stream(stream), _p(ids), _p(samples), int(ids.shape[0]),
                                 ctypes.byref(params), _p(crops), _p(cutout_yx), _p(flips),
                                 _p(status)), 'ffcv_draw_batch')


def draw_batch_host(ids, heights, widths, params: DrawParams, crops=None, cutout_yx=None, flips=None):
    """ffcv_draw_batch on host arrays (the CPU-device decoders' draws)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    hs = np.ascontiguousarray(heights, dtype=np.uint32) if heights is not None else None
    ws = np.ascontiguousarray(widths, dtype=np.uint32) if widths is not None else None
    _check(lib().ffcv_draw_batch_host(_p(ids), _p(hs), _p(ws), int(ids.size), ctypes.byref(params), _p(crops),
                                      _p(cutout_yx), _p(flips)), 'ffcv_draw_batch_host')


def gather_samples(table, ids, out, stream=None):
    _check(lib().ffcv_gather_samples(_stream(stream), _p(table), int(table.shape[0]), _p(ids),
                                     int(ids.shape[0]), _p(out)), 'ffcv_gather_samples')


def rrc_raw_workspace_bytes(batch, out_h, out_w):
    """Device bytes rrc_raw_batch's workspace needs (per-image plan + taps)."""
    return int(lib().ffcv_rrc_raw_workspace_bytes(int(batch), int(out_h), int(out_w)))


def rrc_raw_batch(base, samples, batch, crops, cutout_yx, flips, params: RRCParams, out,
                  stream=None, workspace=None):
    """Raw-mode RRC (+ cutout / flip / LUT).  With a device uint8 `workspace`
    of rrc_raw_workspace_bytes() the per-image plans and tap tables are
    computed once per image (ffcv_rrc_raw_batch_ws); output is identical."""
    if workspace is not None:
        _check(lib().ffcv_rrc_raw_batch_ws(_stream(stream), _p(base), _p(samples), int(batch),
                                           _p(crops), _p(cutout_yx), _p(flips), ctypes.byref(params),
                                           _p(out), _p(workspace), int(workspace.numel())),
               'ffcv_rrc_raw_batch_ws')
        return
    _check(lib().ffcv_rrc_raw_batch(_stream(stream), _p(base), _p(samples), int(batch),
                                    _p(crops), _p(cutout_yx), _p(flips), ctypes.byref(params),
                                    _p(out)), 'ffcv_rrc_raw_batch')


def gather_raw_batch(base, samples, batch, out, out_stride, stream=None):
    _check(lib().ffcv_gather_raw_batch(_stream(stream), _p(base), _p(samples), int(batch),
                                       _p(out), int(out_stride)), 'ffcv_gather_raw_batch')


def gather_rows_cutover():
    """Row size in bytes from which ffcv_gather_rows runs its 2-D grid."""
    return int(lib().ffcv_gather_rows_cutover())


def gather_rows_subwave():
    """Largest row size in bytes that ffcv_gather_rows gives 16 lanes (above: a wave)."""
    return int(lib().ffcv_gather_rows_subwave())


def gather_rows(base, base_bytes, row_off, ids, row_bytes, out, out_stride, status, stream=None, shape=None):
    """``out[k * out_stride : + row_bytes] = base[row_off[ids[k]] : + row_bytes]``
    in one launch (ffcv_gather_rows).  base: device uint8, 16-byte aligned,
    allocated up to the next multiple of 16 past base_bytes; row_off: device
    uint64 (or int64) per sample; ids: device int64 / uint64 [B]; status:
    device int32[B] (0, or 8 with a zero-filled row for an id or a row out of
    range).  ``shape``: diagnostics only, the dispatch shape (1: 16 lanes per
    row, 2: a wave per row, 3: the 2-D grid)."""
    args = (_stream(stream), _p(base), int(base_bytes), _p(row_off), int(row_off.shape[0]), _p(ids),
            int(ids.shape[0]), int(row_bytes), _p(out), int(out_stride), _p(status))
    if shape is None:
        _check(lib().ffcv_gather_rows(*args), 'ffcv_gather_rows')
        return
    fn = lib().ffcv_gather_rows_shape   # not in ffcv_hip.h: bound on first use
    fn.restype = c_int
    fn.argtypes = _SIGS['ffcv_gather_rows'][1] + [c_int]
    _check(fn(*args, int(shape)), 'ffcv_gather_rows_shape')


def _dense_device(who, *tensors, what='tensor'):
    """Every tensor is contiguous, and every one is in device memory (what the
    standalone kernels index); the layout is checked first."""
    for t in tensors:
        if isinstance(t, np.ndarray) or not hasattr(t, 'data_ptr') or not t.is_contiguous():
            raise TypeError(f'{who}: a contiguous device {what} is required')
    for t in tensors:
        if not t.is_cuda:
            raise TypeError(f'{who}: the {what} must be in device memory, got one on {t.device}')


def _u8_device_dims(images, who):
    """_u8_batch_dims of a tensor that is in device memory."""
    dims = _u8_batch_dims(images, who)
    _dense_device(who, images)
    return dims


def cutout_batch(images, yx, crop_size, fill, stream=None):
    """cutout.py:36-47 in place on a contiguous device uint8 (B, H, W, 3) batch;
    yx device int32 (B, 2), every origin >= 0."""
    B, H, W = _u8_device_dims(images, 'cutout_batch')
    f = (ctypes.c_uint8 * 3)(*[int(x) for x in fill])
    _check(lib().ffcv_cutout_batch(_stream(stream), _p(images), B, H, W, _p(yx), int(crop_size),
                                   f), 'ffcv_cutout_batch')


def normalize_batch(inp, lut, out, stream=None):
    _check(lib().ffcv_normalize_batch(_stream(stream), _p(inp), int(inp.numel()), _p(lut),
                                      _p(out)), 'ffcv_normalize_batch')


def lut_batch(inp, lut, out, stream=None):
    """out[i] = lut[inp[i]*3 + i%3] for a [256,3] device table of any dtype
    (element size 1/2/4/8); inp: contiguous device uint8 whose last dimension
    is the channel, out: contiguous, of the table's element size."""
    _dense_device('lut_batch', inp, lut, out)
    if inp.element_size() != 1 or int(lut.numel()) != 768 or out.element_size() != lut.element_size() or \
            out.numel() < inp.numel():
        raise TypeError('lut_batch: a uint8 input, a (256, 3) table and an output of the table\'s element size '
                        'with room for every input element are required')
    _check(lib().ffcv_lut_batch(_stream(stream), _p(inp), int(inp.numel()), _p(lut),
                                int(lut.element_size()), _p(out)), 'ffcv_lut_batch')


def flip_batch(inp, out, flips, stream=None):
    """flip.py:35-40 of a contiguous device (B, H, W, ...) batch of any element
    size into ``out`` (same shape and element size, not ``inp``)."""
    _dense_device('flip_batch', inp, out, what='(B, H, W, ...) tensor')
    if inp.dim() < 3 or tuple(out.shape) != tuple(inp.shape) or out.element_size() != inp.element_size():
        raise TypeError('flip_batch: contiguous device (B, H, W, ...) tensors of one shape and element size are '
                        f'required, got {tuple(inp.shape)} and {tuple(out.shape)}')
    B, H, W = int(inp.shape[0]), int(inp.shape[1]), int(inp.shape[2])
    cb = int(np.prod([int(x) for x in inp.shape[3:]], dtype=np.int64)) * int(inp.element_size())
    _check(lib().ffcv_flip_batch(_stream(stream), _p(inp), _p(out), B, H, W, cb, _p(flips)),
           'ffcv_flip_batch')


def _seed64(loader_seed):
    """The loader's seed as the uint64 the C ABI takes."""
    return int(loader_seed) & 0xFFFFFFFFFFFFFFFF


def fill_u8(fill):
    """A fill colour (a number, or one or three of them) as a fresh (3,) uint8 array."""
    return np.broadcast_to(np.asarray(fill).astype(np.uint8).reshape(-1), (3,)).copy()


def _u8_batch_dims(images, who):
    """(B, H, W) of a contiguous uint8 (B, H, W, 3) batch: a numpy array for a
    ``*_host`` entry, else a tensor."""
    if who.endswith('_host'):
        ok = isinstance(images, np.ndarray) and images.dtype == np.uint8 and images.flags.c_contiguous
        what = 'C-contiguous uint8 (B, H, W, 3) array'
    else:
        ok = not isinstance(images, np.ndarray) and images.element_size() == 1 and images.is_contiguous()
        what = 'contiguous uint8 (B, H, W, 3) tensor'
    if not ok or len(images.shape) != 4 or int(images.shape[3]) != 3:
        raise TypeError(f'{who}: a {what} is required')
    return int(images.shape[0]), int(images.shape[1]), int(images.shape[2])


def _u8_out_of_place_dims(src, dst, who):
    """_u8_batch_dims of the ``src`` of an out-of-place ``*_host`` entry, whose
    ``dst`` is such an array too, of the same image shape, with room for B."""
    dims = _u8_batch_dims(src, who)
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and
            dst.shape[1:] == src.shape[1:] and dst.shape[0] >= src.shape[0]):
        raise TypeError(f'{who}: C-contiguous uint8 (B, H, W, 3) arrays of one image shape are required')
    return dims


def _per_image(who, name, a, dtype, *shape):
    """``a`` as a C-contiguous per-image array of ``dtype`` and ``shape`` (B, ...); (B,): of B values."""
    a = np.ascontiguousarray(a, dtype)
    a = a.reshape(-1) if len(shape) == 1 else a
    if a.shape != shape:
        raise TypeError(f'{who}: {name} {shape} is required, got {a.shape}')
    return a


def translate_draw_batch(ids, loader_seed, epoch, padding, yx, status=None, stream=None):
    """RandomTranslate windows (y, x) of the batch on the device (op id 4)."""
    _check(lib().ffcv_translate_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                           _seed64(loader_seed), int(epoch), int(padding),
                                           _p(yx), _p(status)), 'ffcv_translate_draw_batch')


def translate_draw_batch_host(ids, loader_seed, epoch, padding):
    """The same draws on the host: int32 (B, 2) of (y, x)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    yx = np.empty((ids.size, 2), np.int32)
    _check(lib().ffcv_translate_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed),
                                                int(epoch), int(padding), _p(yx)),
           'ffcv_translate_draw_batch_host')
    return yx


def translate_batch(inp, out, yx, padding, fill, stream=None):
    """translate.py:35-44 of a contiguous device uint8 (B, H, W, 3) batch into
    ``out`` (same shape, not ``inp``); yx device int32 (B, 2)."""
    B, H, W = _u8_batch_dims(inp, 'translate_batch')
    if _u8_batch_dims(out, 'translate_batch') != (B, H, W):
        raise TypeError(f'translate_batch: out must have the input\'s shape {tuple(inp.shape)}, got '
                        f'{tuple(out.shape)}')
    _dense_device('translate_batch', inp, out)
    f = (ctypes.c_uint8 * 3)(*[int(x) for x in fill])
    _check(lib().ffcv_translate_batch(_stream(stream), _p(inp), _p(out), B, H, W, _p(yx), int(padding), f),
           'ffcv_translate_batch')


def _ranges(scale, ratio):
    return (c_double * 2)(float(scale[0]), float(scale[1])), (c_double * 2)(float(ratio[0]), float(ratio[1]))


def crop_draw_batch(ids, height, width, scale, ratio, loader_seed, epoch, crops, status=None, stream=None):
    """RandomResizedCrop (transform) windows (i, j, h, w) of the batch on the
    device (op id 8): ids device int64 / uint64 [B], crops device int32 (B, 4)."""
    sc, ra = _ranges(scale, ratio)
    _check(lib().ffcv_crop_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]), int(height), int(width), sc, ra,
                                      _seed64(loader_seed), int(epoch), _p(crops), _p(status)),
           'ffcv_crop_draw_batch')


def crop_draw_batch_host(ids, height, width, scale, ratio, loader_seed, epoch, status=None):
    """The same draws on the host: int32 (B, 4) of (i, j, h, w)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    crops = np.empty((ids.size, 4), np.int32)
    sc, ra = _ranges(scale, ratio)
    _check(lib().ffcv_crop_draw_batch_host(_p(ids), int(ids.size), int(height), int(width), sc, ra,
                                           _seed64(loader_seed), int(epoch), _p(crops), _p(status)),
           'ffcv_crop_draw_batch_host')
    return crops


def rrc_images_lds_bytes():
    """The largest staged source one workgroup of ffcv_rrc_images_batch keeps in LDS."""
    return int(lib().ffcv_rrc_images_lds_bytes())


def rrc_images_workspace_bytes(batch, height, width, out_h, out_w):
    """Device bytes rrc_images_batch's workspace needs (0 in the LDS regime)."""
    return int(lib().ffcv_rrc_images_workspace_bytes(int(batch), int(height), int(width), int(out_h), int(out_w)))


def rrc_images_band_workspace_bytes(batch, out_h, out_w):
    """The workspace of a band-regime launch (rrc_images_batch's ``regime=2``)."""
    a256 = lambda x: (x + 255) & ~255  # noqa: E731
    return a256(int(batch) * 32) + a256(int(batch) * 16) + rrc_raw_workspace_bytes(batch, out_h, out_w)


def rrc_images_batch(inp, in_stride, batch, height, width, crops, cutout_yx, flips, params: RRCParams, out,
                     status=None, workspace=None, stream=None, regime=None):
    """Crop + INTER_AREA resize (+ flip / cutout / fp16 LUT through ``params``)
    of a dense device uint8 batch of height x width x 3 images, image k at
    ``inp + k * in_stride`` (ffcv_rrc_images_batch); ``workspace``: a device
    uint8 tensor of rrc_images_workspace_bytes(), None where that is 0.
    ``regime``: diagnostics only (1: the LDS kernel, 2: the band kernel with
    a workspace of rrc_images_band_workspace_bytes())."""
    wb = int(workspace.numel() * workspace.element_size()) if workspace is not None else 0
    args = (_stream(stream), _p(inp), int(in_stride), int(batch), int(height), int(width), _p(crops), _p(cutout_yx),
            _p(flips), ctypes.byref(params), _p(out), _p(status), _p(workspace), wb)
    if regime is None:
        _check(lib().ffcv_rrc_images_batch(*args), 'ffcv_rrc_images_batch')
        return
    fn = lib().ffcv_rrc_images_batch_regime   # not in ffcv_hip.h: bound on first use
    fn.restype = c_int
    fn.argtypes = _SIGS['ffcv_rrc_images_batch'][1] + [c_int]
    _check(fn(*args, int(regime)), 'ffcv_rrc_images_batch_regime')


def rrc_images_batch_host(inp: np.ndarray, crops, out: np.ndarray, status=None, nthreads=1):
    """The resize on C-contiguous numpy uint8 arrays: inp (B, H, W, 3), crops
    int32 (B, 4), out (B, out_h, out_w, 3); an invalid crop gives a zero image
    and status 8 (status: int32 (B,) or None)."""
    if not (isinstance(inp, np.ndarray) and isinstance(out, np.ndarray) and inp.dtype == np.uint8 and
            out.dtype == np.uint8 and inp.ndim == 4 and out.ndim == 4 and inp.shape[3] == 3 and out.shape[3] == 3
            and inp.flags.c_contiguous and out.flags.c_contiguous and out.shape[0] >= inp.shape[0]):
        raise TypeError('rrc_images_batch_host: C-contiguous uint8 (B, H, W, 3) arrays are required')
    crops = np.ascontiguousarray(crops, np.int32)
    B, H, W = (int(x) for x in inp.shape[:3])
    if crops.shape != (B, 4):
        raise TypeError(f'rrc_images_batch_host: crops must be int32 ({B}, 4), got {crops.shape}')
    _check(lib().ffcv_rrc_images_batch_host(_p(inp), H * W * 3, B, H, W, _p(crops), int(out.shape[1]),
                                            int(out.shape[2]), _p(out), int(out[0].nbytes) if B else 0, _p(status),
                                            int(max(1, nthreads))), 'ffcv_rrc_images_batch_host')
    return out[:B]


def simple_aug_batch(base, samples, batch, height, width, params: SimpleAugParams, flips, cutout_yx,
                     translate_yx, lut, out, out_stride=0, stream=None):
    """Raw constant-size samples -> flip / translate / cutout in the program's
    order (+ fp16 LUT) in one launch (ffcv_simple_aug_batch)."""
    _check(lib().ffcv_simple_aug_batch(_stream(stream), _p(base), _p(samples), int(batch), int(height),
                                       int(width), ctypes.byref(params), _p(flips), _p(cutout_yx),
                                       _p(translate_yx), _p(lut), _p(out), int(out_stride)),
           'ffcv_simple_aug_batch')


CJ_BRIGHTNESS, CJ_CONTRAST, CJ_SATURATION, CJ_GRAYSCALE, CJ_SOLARIZE = 1, 2, 3, 4, 5


def color_jitter_params(steps) -> ColorJitterParams:
    """The program of FFCV_CJ_* kinds in pipeline order."""
    p = ColorJitterParams()
    p.n_steps = len(steps)
    for i, st in enumerate(list(steps)[:4]):
        p.steps[i] = int(st)
    return p


def color_jitter_draw_batch(ids, loader_seed, epoch, op_id, p, magnitude, apply, ratio, status=None, stream=None):
    """Colour-jitter decisions of the batch on the device: apply uint8[B],
    ratio float64[B] (op id 5 brightness, 6 contrast, 7 saturation)."""
    _check(lib().ffcv_color_jitter_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                              _seed64(loader_seed), int(epoch), int(op_id),
                                              float(p), float(magnitude), _p(apply), _p(ratio), _p(status)),
           'ffcv_color_jitter_draw_batch')


def color_jitter_draw_batch_host(ids, loader_seed, epoch, op_id, p, magnitude):
    """The same draws on the host: (apply uint8 (B,), ratio float64 (B,))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    apply = np.empty(ids.size, np.uint8)
    ratio = np.empty(ids.size, np.float64)
    _check(lib().ffcv_color_jitter_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed),
                                                   int(epoch), int(op_id), float(p), float(magnitude), _p(apply),
                                                   _p(ratio)), 'ffcv_color_jitter_draw_batch_host')
    return apply, ratio


def color_jitter_workspace_bytes(batch):
    return int(lib().ffcv_color_jitter_workspace_bytes(int(batch)))


def color_jitter_lds_bytes():
    return int(lib().ffcv_color_jitter_lds_bytes())


def color_jitter_batch(images, steps, apply, ratio, workspace=None, stream=None):
    """The program ``steps`` in place on a device uint8 (B, H, W, 3) batch
    (apply uint8 (n, B), ratio float64 (n, B)); one launch while an image fits
    color_jitter_lds_bytes(), else one without and two with a contrast step."""
    B, H, W = _u8_batch_dims(images, 'color_jitter_batch')
    params = steps if isinstance(steps, ColorJitterParams) else color_jitter_params(steps)
    wb = int(workspace.numel() * workspace.element_size()) if workspace is not None else 0
    _check(lib().ffcv_color_jitter_batch(_stream(stream), _p(images), B, H, W, ctypes.byref(params), _p(apply),
                                         _p(ratio), _p(workspace), wb), 'ffcv_color_jitter_batch')


def color_jitter_batch_host(images, steps, apply, ratio):
    """The same program in place on a C-contiguous numpy uint8 (B, H, W, 3)."""
    B, H, W = _u8_batch_dims(images, 'color_jitter_batch_host')
    params = steps if isinstance(steps, ColorJitterParams) else color_jitter_params(steps)
    apply = np.ascontiguousarray(apply, np.uint8).reshape(params.n_steps, B)
    ratio = np.ascontiguousarray(ratio, np.float64).reshape(params.n_steps, B)
    _check(lib().ffcv_color_jitter_batch_host(_p(images), B, H, W, ctypes.byref(params), _p(apply), _p(ratio)),
           'ffcv_color_jitter_batch_host')
    return images


def uniform_draw_batch(ids, loader_seed, epoch, op_id, p, lo, hi, apply, value, status=None, stream=None):
    """``rand() < p`` then ``uniform(lo, hi)`` of the batch on the device (op id
    9 grayscale, 10 solarization, 11 blur): apply uint8[B], value float64[B]."""
    _check(lib().ffcv_uniform_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                         _seed64(loader_seed), int(epoch), int(op_id), float(p),
                                         float(lo), float(hi), _p(apply), _p(value), _p(status)),
           'ffcv_uniform_draw_batch')


def uniform_draw_batch_host(ids, loader_seed, epoch, op_id, p, lo, hi):
    """The same draws on the host: (apply uint8 (B,), value float64 (B,))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    apply = np.empty(ids.size, np.uint8)
    value = np.empty(ids.size, np.float64)
    _check(lib().ffcv_uniform_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed),
                                              int(epoch), int(op_id), float(p), float(lo), float(hi), _p(apply),
                                              _p(value)), 'ffcv_uniform_draw_batch_host')
    return apply, value


BLUR_WROW = 32  # floats per sample in a blur weights array


def blur_draw_batch(ids, loader_seed, epoch, p, sigma_lo, sigma_hi, ksize, apply, sigma, weights, status=None,
                    stream=None):
    """GaussianBlur's draws of the batch on the device (op id 11): apply
    uint8[B], sigma float64[B], weights float32 (B, 32)."""
    _check(lib().ffcv_blur_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                      _seed64(loader_seed), int(epoch), float(p), float(sigma_lo),
                                      float(sigma_hi), int(ksize), _p(apply), _p(sigma), _p(weights), _p(status)),
           'ffcv_blur_draw_batch')


def blur_draw_batch_host(ids, loader_seed, epoch, p, sigma_lo, sigma_hi, ksize):
    """The same draws on the host: (apply uint8 (B,), sigma float64 (B,),
    weights float32 (B, 32))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    apply = np.empty(ids.size, np.uint8)
    sigma = np.empty(ids.size, np.float64)
    weights = np.empty((ids.size, BLUR_WROW), np.float32)
    _check(lib().ffcv_blur_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch),
                                           float(p), float(sigma_lo), float(sigma_hi), int(ksize), _p(apply),
                                           _p(sigma), _p(weights)), 'ffcv_blur_draw_batch_host')
    return apply, sigma, weights


def gaussian_blur_lds_bytes():
    """15 * H * W of the largest image one workgroup of gaussian_blur_batch blurs whole."""
    return int(lib().ffcv_gaussian_blur_lds_bytes())


def gaussian_blur_band_rows():
    """Output rows per workgroup beyond the whole-image regime."""
    return int(lib().ffcv_gaussian_blur_band_rows())


def gaussian_blur_strip_cols(height, width, ksize):
    """Output columns per workgroup (== width while one strip serves a band)."""
    return int(lib().ffcv_gaussian_blur_strip_cols(int(height), int(width), int(ksize)))


def gaussian_blur_batch(src, dst, ksize, apply, weights, dst_stride=0, stream=None):
    """Blur (apply[k] != 0) or copy each image of a dense device uint8
    (B, H, W, 3) batch into ``dst`` (ffcv_gaussian_blur_batch): one launch, out
    of place; apply device uint8 (B,), weights device float32 (B, 32)."""
    B, H, W = _u8_batch_dims(src, 'gaussian_blur_batch')
    _check(lib().ffcv_gaussian_blur_batch(_stream(stream), _p(src), _p(dst), B, H, W, int(ksize), _p(apply),
                                          _p(weights), int(dst_stride)), 'ffcv_gaussian_blur_batch')
    return dst


def gaussian_blur_batch_host(src: np.ndarray, dst: np.ndarray, ksize, apply, weights, nthreads=1):
    """The same on C-contiguous numpy uint8 (B, H, W, 3) arrays."""
    B, H, W = _u8_out_of_place_dims(src, dst, 'gaussian_blur_batch_host')
    apply = _per_image('gaussian_blur_batch_host', 'apply', apply, np.uint8, B)
    weights = _per_image('gaussian_blur_batch_host', 'weights', weights, np.float32, B, BLUR_WROW)
    _check(lib().ffcv_gaussian_blur_batch_host(_p(src), _p(dst), B, H, W, int(ksize), _p(apply), _p(weights), 0,
                                               int(max(1, nthreads))), 'ffcv_gaussian_blur_batch_host')
    return dst[:B]


def sharpness_draw_batch(ids, loader_seed, epoch, p, factor, apply, factor_out, status=None, stream=None):
    """RandomAdjustSharpness's draws of the batch on the device (op id 19):
    apply uint8[B] = rand() < p, factor_out float32[B] = the constant."""
    _check(lib().ffcv_sharpness_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]), _seed64(loader_seed),
                                           int(epoch), float(p), float(factor), _p(apply), _p(factor_out),
                                           _p(status)), 'ffcv_sharpness_draw_batch')


def sharpness_draw_batch_host(ids, loader_seed, epoch, p, factor):
    """The same draws on the host: (apply uint8 (B,), factor float32 (B,))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    apply = np.empty(ids.size, np.uint8)
    factor_out = np.empty(ids.size, np.float32)
    _check(lib().ffcv_sharpness_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch), float(p),
                                                float(factor), _p(apply), _p(factor_out)),
           'ffcv_sharpness_draw_batch_host')
    return apply, factor_out


def sharpness_lds_bytes():
    """6 * H * W of the largest image one workgroup of sharpness_batch takes whole."""
    return int(lib().ffcv_sharpness_lds_bytes())


def sharpness_band_rows():
    """Output rows per workgroup beyond the whole-image regime."""
    return int(lib().ffcv_sharpness_band_rows())


def sharpness_strip_cols(height, width):
    """Output columns per workgroup (== width while one strip serves a band)."""
    return int(lib().ffcv_sharpness_strip_cols(int(height), int(width)))


def sharpness_batch(src, dst, apply, factor, dst_stride=0, stream=None):
    """Per image of a dense device uint8 (B, H, W, 3) batch: copy (apply[k] ==
    0), sharpen with factor[k] (1) or leave ``dst`` alone (2)
    (ffcv_sharpness_batch): one launch, out of place; apply device uint8 (B,),
    factor device float32 (B,)."""
    B, H, W = _u8_batch_dims(src, 'sharpness_batch')
    _check(lib().ffcv_sharpness_batch(_stream(stream), _p(src), _p(dst), B, H, W, _p(apply), _p(factor),
                                      int(dst_stride)), 'ffcv_sharpness_batch')
    return dst


def sharpness_batch_host(src: np.ndarray, dst: np.ndarray, apply, factor, nthreads=1):
    """The same on C-contiguous numpy uint8 (B, H, W, 3) arrays."""
    B, H, W = _u8_out_of_place_dims(src, dst, 'sharpness_batch_host')
    apply = _per_image('sharpness_batch_host', 'apply', apply, np.uint8, B)
    factor = _per_image('sharpness_batch_host', 'factor', factor, np.float32, B)
    _check(lib().ffcv_sharpness_batch_host(_p(src), _p(dst), B, H, W, _p(apply), _p(factor), 0,
                                           int(max(1, nthreads))), 'ffcv_sharpness_batch_host')
    return dst[:B]


def hue_draw_batch(ids, loader_seed, epoch, p, magnitude, apply, shift, status=None, stream=None):
    """RandomHue's decisions of the batch on the device (op id 12): apply
    uint8[B], shift float64[B] = uniform(-magnitude, magnitude)."""
    _check(lib().ffcv_hue_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                     _seed64(loader_seed), int(epoch), float(p), float(magnitude),
                                     _p(apply), _p(shift), _p(status)), 'ffcv_hue_draw_batch')


def hue_draw_batch_host(ids, loader_seed, epoch, p, magnitude):
    """The same draws on the host: (apply uint8 (B,), shift float64 (B,))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    apply = np.empty(ids.size, np.uint8)
    shift = np.empty(ids.size, np.float64)
    _check(lib().ffcv_hue_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch),
                                          float(p), float(magnitude), _p(apply), _p(shift)),
           'ffcv_hue_draw_batch_host')
    return apply, shift


def _magnitude4(magnitude):
    m = np.ascontiguousarray([float(x) for x in magnitude], dtype=np.float64)
    if m.shape != (4,):
        raise TypeError('four magnitudes (brightness, contrast, saturation, hue) are required')
    return m


def color_jitter_joint_rows(magnitude):
    """Rows the joint draw writes: the components with a non-zero magnitude."""
    return sum(1 for x in magnitude if float(x) != 0.0)


def color_jitter_joint_draw_batch(ids, loader_seed, epoch, p, magnitude, apply, ratio, status=None, stream=None):
    """RandomColorJitter's five draws of the batch on the device (op id 13):
    one row of apply uint8 (rows, B) / ratio float64 (rows, B) per component of
    (brightness, contrast, saturation, hue) with a non-zero magnitude."""
    m = _magnitude4(magnitude)
    _check(lib().ffcv_color_jitter_joint_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                                    _seed64(loader_seed), int(epoch), float(p),
                                                    _p(m), _p(apply), _p(ratio), _p(status)),
           'ffcv_color_jitter_joint_draw_batch')


def color_jitter_joint_draw_batch_host(ids, loader_seed, epoch, p, magnitude):
    """The same draws on the host: (apply uint8 (rows, B), ratio float64 (rows, B))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    m = _magnitude4(magnitude)
    rows = color_jitter_joint_rows(m)
    apply = np.empty((max(rows, 1), ids.size), np.uint8)
    ratio = np.empty((max(rows, 1), ids.size), np.float64)
    _check(lib().ffcv_color_jitter_joint_draw_batch_host(_p(ids), int(ids.size),
                                                         _seed64(loader_seed), int(epoch), float(p),
                                                         _p(m), _p(apply), _p(ratio)),
           'ffcv_color_jitter_joint_draw_batch_host')
    return apply[:rows], ratio[:rows]


def hue_batch(images, apply, shift, stream=None):
    """The hue shift in place on a device uint8 (B, H, W, 3) batch, one launch:
    image k turns by shift[k] where apply[k] != 0 (apply uint8 (B,), shift
    float64 (B,), both on the device)."""
    B, H, W = _u8_batch_dims(images, 'hue_batch')
    _check(lib().ffcv_hue_batch(_stream(stream), _p(images), B, H, W, _p(apply), _p(shift)), 'ffcv_hue_batch')
    return images


def hue_batch_host(images, apply, shift):
    """The same in place on a C-contiguous numpy uint8 (B, H, W, 3)."""
    B, H, W = _u8_batch_dims(images, 'hue_batch_host')
    apply = np.ascontiguousarray(apply, np.uint8).reshape(-1)
    shift = np.ascontiguousarray(shift, np.float64).reshape(-1)
    if apply.size != B or shift.size != B:
        raise TypeError(f'hue_batch_host: apply ({B},) and shift ({B},) are required, got {apply.shape} and '
                        f'{shift.shape}')
    _check(lib().ffcv_hue_batch_host(_p(images), B, H, W, _p(apply), _p(shift)), 'ffcv_hue_batch_host')
    return images


TONE_POSTERIZE, TONE_AUTOCONTRAST, TONE_EQUALIZE, TONE_INVERT = 1, 2, 3, 4  # FFCV_TONE_*


def tone_params(steps, bits=8) -> ToneParams:
    """The program of FFCV_TONE_* kinds in pipeline order (and posterize's bits)."""
    p = ToneParams()
    p.n_steps = len(steps)
    for i, st in enumerate(list(steps)[:4]):
        p.steps[i] = int(st)
    p.bits = int(bits)
    return p


def _tone_pairs(op_ids, ps):
    ops = np.ascontiguousarray([int(o) for o in op_ids], dtype=np.int32)
    ps = np.ascontiguousarray([float(x) for x in ps], dtype=np.float64)
    if ops.size != ps.size:
        raise TypeError(f'as many probabilities as op ids are required, got {ops.size} and {ps.size}')
    return ops, ps


def tone_draw_batch(ids, loader_seed, epoch, op_ids, ps, apply, status=None, stream=None):
    """The decisions of up to four table operations (op id 15 posterize, 16
    autocontrast, 17 equalize, 18 invert) of the batch in one launch:
    apply uint8 (n, B), row i ``rand() < ps[i]`` from the stream of op_ids[i]."""
    ops, ps = _tone_pairs(op_ids, ps)
    _check(lib().ffcv_tone_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                      _seed64(loader_seed), int(epoch), int(ops.size), _p(ops),
                                      _p(ps), _p(apply), _p(status)), 'ffcv_tone_draw_batch')


def tone_draw_batch_host(ids, loader_seed, epoch, op_ids, ps):
    """The same draws on the host: apply uint8 (n, B)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    ops, ps = _tone_pairs(op_ids, ps)
    apply = np.empty((max(int(ops.size), 1), ids.size), np.uint8)
    _check(lib().ffcv_tone_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch),
                                           int(ops.size), _p(ops), _p(ps), _p(apply)), 'ffcv_tone_draw_batch_host')
    return apply


def tone_workspace_bytes(batch):
    return int(lib().ffcv_tone_workspace_bytes(int(batch)))


def tone_lds_bytes():
    return int(lib().ffcv_tone_lds_bytes())


def tone_batch(images, steps, bits, apply, workspace=None, stream=None):
    """The program ``steps`` in place on a device uint8 (B, H, W, 3) batch
    (apply uint8 (n, B)); one launch while an image fits tone_lds_bytes(), else
    one without and two with an autocontrast or equalize step."""
    B, H, W = _u8_batch_dims(images, 'tone_batch')
    params = steps if isinstance(steps, ToneParams) else tone_params(steps, bits)
    wb = int(workspace.numel() * workspace.element_size()) if workspace is not None else 0
    _check(lib().ffcv_tone_batch(_stream(stream), _p(images), B, H, W, ctypes.byref(params), _p(apply),
                                 _p(workspace), wb), 'ffcv_tone_batch')


def tone_batch_host(images, steps, bits, apply):
    """The same program in place on a C-contiguous numpy uint8 (B, H, W, 3)."""
    B, H, W = _u8_batch_dims(images, 'tone_batch_host')
    params = steps if isinstance(steps, ToneParams) else tone_params(steps, bits)
    apply = np.ascontiguousarray(apply, np.uint8).reshape(max(params.n_steps, 1), B)
    _check(lib().ffcv_tone_batch_host(_p(images), B, H, W, ctypes.byref(params), _p(apply)), 'ffcv_tone_batch_host')
    return images


def tone_batch_bits(images, steps, apply, bits, workspace=None, stream=None):
    """tone_batch with posterize's bits per image: bits device uint8 (B,)
    (ffcv_tone_batch_bits)."""
    B, H, W = _u8_batch_dims(images, 'tone_batch_bits')
    params = steps if isinstance(steps, ToneParams) else tone_params(steps, 8)
    wb = int(workspace.numel() * workspace.element_size()) if workspace is not None else 0
    _check(lib().ffcv_tone_batch_bits(_stream(stream), _p(images), B, H, W, ctypes.byref(params), _p(apply),
                                      _p(workspace), wb, _p(bits)), 'ffcv_tone_batch_bits')


def tone_batch_bits_host(images, steps, apply, bits):
    """The same in place on a C-contiguous numpy uint8 (B, H, W, 3); bits uint8 (B,)."""
    B, H, W = _u8_batch_dims(images, 'tone_batch_bits_host')
    params = steps if isinstance(steps, ToneParams) else tone_params(steps, 8)
    apply = np.ascontiguousarray(apply, np.uint8).reshape(max(params.n_steps, 1), B)
    bits = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    if bits.size != B:
        raise TypeError(f'tone_batch_bits_host: bits ({B},) is required, got {bits.shape}')
    _check(lib().ffcv_tone_batch_bits_host(_p(images), B, H, W, ctypes.byref(params), _p(apply), _p(bits)),
           'ffcv_tone_batch_bits_host')
    return images


POLICY_NOPS = 14  # operations of the TrivialAugmentWide policy, rows of its value table
# the arrays ffcv_policy_draw_batch fills, in argument order: (name, dtype, shape per batch size B)
POLICY_ARRAYS = (('op', np.uint8, lambda B: (B,)), ('cj_apply', np.uint8, lambda B: (4, B)),
                 ('cj_ratio', np.float64, lambda B: (4, B)), ('tone_apply', np.uint8, lambda B: (3, B)),
                 ('tone_bits', np.uint8, lambda B: (B,)), ('aff_apply', np.uint8, lambda B: (B,)),
                 ('aff_coef', np.int64, lambda B: (B, 6)), ('sharp_apply', np.uint8, lambda B: (B,)),
                 ('sharp_factor', np.float32, lambda B: (B,)))


def policy_draw_batch(ids, loader_seed, epoch, nbins, table, height, width, out, status=None, stream=None):
    """TrivialAugmentWide's draws of the batch on the device (op id 20) into
    the device tensors ``out[name]`` of POLICY_ARRAYS; table: device float64
    (14, nbins)."""
    if table.numel() != POLICY_NOPS * int(nbins) or table.element_size() != 8 or not table.is_contiguous():
        raise TypeError(f'policy_draw_batch: a contiguous float64 ({POLICY_NOPS}, {nbins}) table is required')
    _check(lib().ffcv_policy_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]), _seed64(loader_seed), int(epoch),
                                        int(nbins), _p(table), int(height), int(width),
                                        *[_p(out[name]) for name, _, _ in POLICY_ARRAYS], _p(status)),
           'ffcv_policy_draw_batch')


def policy_draw_batch_host(ids, loader_seed, epoch, nbins, table, height, width):
    """The same draws on the host: a dict of the POLICY_ARRAYS."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.shape != (POLICY_NOPS, int(nbins)):
        raise TypeError(f'policy_draw_batch_host: a float64 ({POLICY_NOPS}, {nbins}) table is required')
    out = {name: np.empty(shape(ids.size), dt) for name, dt, shape in POLICY_ARRAYS}
    _check(lib().ffcv_policy_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch), int(nbins),
                                             _p(table), int(height), int(width),
                                             *[_p(out[name]) for name, _, _ in POLICY_ARRAYS]),
           'ffcv_policy_draw_batch_host')
    return out


RANDAUGMENT_MAX_OPS = 8  # slots per sample, at most


def randaugment_arrays(num_ops):
    """The arrays ffcv_randaugment_draw_batch fills, in argument order: those
    of POLICY_ARRAYS, each with a leading slot dimension."""
    return tuple((name, dt, lambda B, shape=shape: (int(num_ops),) + shape(B)) for name, dt, shape in POLICY_ARRAYS)


def randaugment_slot(d, s):
    """Slot s's slices of the draw's arrays: the arguments of the pixel
    entries of TrivialAugmentWide for that slot."""
    return {name: d[name][s] for name, _, _ in POLICY_ARRAYS}


def randaugment_draw_batch(ids, loader_seed, epoch, num_ops, nbins, magnitude, table, height, width, out, status=None,
                           stream=None):
    """RandAugment's draws of the batch on the device (op id 23) into the
    device tensors ``out[name]`` of randaugment_arrays(num_ops); table: device
    float64 (14, nbins)."""
    if table.numel() != POLICY_NOPS * int(nbins) or table.element_size() != 8 or not table.is_contiguous():
        raise TypeError(f'randaugment_draw_batch: a contiguous float64 ({POLICY_NOPS}, {nbins}) table is required')
    _check(lib().ffcv_randaugment_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]), _seed64(loader_seed),
                                             int(epoch), int(num_ops), int(nbins), int(magnitude), _p(table),
                                             int(height), int(width),
                                             *[_p(out[name]) for name, _, _ in POLICY_ARRAYS], _p(status)),
           'ffcv_randaugment_draw_batch')


def randaugment_draw_batch_host(ids, loader_seed, epoch, num_ops, nbins, magnitude, table, height, width):
    """The same draws on the host: a dict of the randaugment_arrays(num_ops)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.shape != (POLICY_NOPS, int(nbins)):
        raise TypeError(f'randaugment_draw_batch_host: a float64 ({POLICY_NOPS}, {nbins}) table is required')
    if not 1 <= int(num_ops) <= RANDAUGMENT_MAX_OPS:
        raise FFCVError(f'randaugment_draw_batch_host: {num_ops} operations per sample, outside 1 to '
                        f'{RANDAUGMENT_MAX_OPS}')
    out = {name: np.empty(shape(ids.size), dt) for name, dt, shape in randaugment_arrays(num_ops)}
    _check(lib().ffcv_randaugment_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch),
                                                  int(num_ops), int(nbins), int(magnitude), _p(table), int(height),
                                                  int(width), *[_p(out[name]) for name, _, _ in POLICY_ARRAYS]),
           'ffcv_randaugment_draw_batch_host')
    return out


def randaugment_lds_bytes():
    """6 * H * W of the largest image randaugment_batch takes: the bound of the
    fused regime, for the dispatch and the tests alike."""
    return int(lib().ffcv_randaugment_lds_bytes())


def randaugment_batch(src, dst, num_ops, mode, fill, d, stream=None):
    """Every slot of every sample of a dense device uint8 (B, H, W, 3) batch in
    ONE launch, into ``dst`` (ffcv_randaugment_batch; images up to
    randaugment_lds_bytes()); d: the device arrays of randaugment_draw_batch."""
    B, H, W = _u8_batch_dims(src, 'randaugment_batch')
    if tuple(dst.shape) != tuple(src.shape) or not dst.is_contiguous():
        raise TypeError(f'randaugment_batch: a contiguous dst of shape {tuple(src.shape)} is required')
    for name, dt, shape in randaugment_arrays(num_ops):
        a = d[name]
        if tuple(a.shape) != shape(B) or a.element_size() != np.dtype(dt).itemsize or not a.is_contiguous():
            raise TypeError(f'randaugment_batch: {name} must be a contiguous {np.dtype(dt).name} {shape(B)}')
    f = fill_u8(fill)
    _check(lib().ffcv_randaugment_batch(_stream(stream), _p(src), _p(dst), B, H, W, int(num_ops), int(mode), _p(f),
                                        *[_p(d[name]) for name, _, _ in POLICY_ARRAYS]), 'ffcv_randaugment_batch')
    return dst


def tone_tables_host(kind, bits, hists):
    """The host twin's table builder: uint8 (n, 256) tables of step ``kind``
    for channels with the uint32 (n, 256) histograms ``hists``."""
    hists = np.ascontiguousarray(hists, dtype=np.uint32).reshape(-1, 256)
    tables = np.empty(hists.shape, np.uint8)
    _check(lib().ffcv_tone_tables_host(int(kind), int(bits), _p(hists), _p(tables), int(hists.shape[0])),
           'ffcv_tone_tables_host')
    return tables


AFFINE_BILINEAR, AFFINE_NEAREST = 0, 1  # FFCV_AFFINE_*
AFFINE_NOT_STAGEABLE = (1 << 64) - 1    # ffcv_affine_tile_bytes: relative coordinates leave 32 bits


def _ranges12(ranges):
    r = np.ascontiguousarray([float(x) for x in ranges], dtype=np.float64)
    if r.shape != (12,):
        raise TypeError('six (low, high) pairs (angle, tx, ty, scale, shear x, shear y) are required')
    return r


def affine_draw_batch(ids, loader_seed, epoch, p, ranges, height, width, apply, coef, status=None, stream=None):
    """RandomAffine's seven draws of the batch and their Q16 coefficients on
    the device (op id 14): apply uint8[B], coef int64 (B, 6)."""
    r = _ranges12(ranges)
    _check(lib().ffcv_affine_draw_batch(_stream(stream), _p(ids), int(ids.shape[0]),
                                        _seed64(loader_seed), int(epoch), float(p), _p(r),
                                        int(height), int(width), _p(apply), _p(coef), _p(status)),
           'ffcv_affine_draw_batch')


def affine_draw_batch_host(ids, loader_seed, epoch, p, ranges, height, width):
    """The same draws on the host: (apply uint8 (B,), coef int64 (B, 6))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    r = _ranges12(ranges)
    apply = np.empty(ids.size, np.uint8)
    coef = np.empty((ids.size, 6), np.int64)
    _check(lib().ffcv_affine_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed),
                                             int(epoch), float(p), _p(r), int(height), int(width), _p(apply),
                                             _p(coef)), 'ffcv_affine_draw_batch_host')
    return apply, coef


def affine_whole_bytes():
    """3 * H * W of the largest image one workgroup of affine_batch warps whole."""
    return int(lib().ffcv_affine_whole_bytes())


def affine_tile_shape():
    """(rows, columns) of an output tile beyond the whole-image regime."""
    return int(lib().ffcv_affine_tile_rows()), int(lib().ffcv_affine_tile_cols())


def affine_tile_lds():
    """Bytes of staged source beyond which a tile reads global memory directly."""
    return int(lib().ffcv_affine_tile_lds())


def affine_tile_bytes(height, width, mode, coef, tile_row, tile_col):
    """Bytes the kernel stages for one tile (0: it reads nothing;
    AFFINE_NOT_STAGEABLE: its coordinates leave 32 bits)."""
    q = np.ascontiguousarray(coef, dtype=np.int64).reshape(-1)
    if q.shape != (6,):
        raise TypeError('six coefficients are required')
    return int(lib().ffcv_affine_tile_bytes(int(height), int(width), int(mode), _p(q), int(tile_row), int(tile_col)))


def affine_batch(src, dst, mode, fill, apply, coef, dst_stride=0, stream=None):
    """Warp (apply[k] != 0) or copy each image of a dense device uint8
    (B, H, W, 3) batch into ``dst`` (ffcv_affine_batch): one launch, out of
    place; apply device uint8 (B,), coef device int64 (B, 6)."""
    B, H, W = _u8_batch_dims(src, 'affine_batch')
    f = fill_u8(fill)
    _check(lib().ffcv_affine_batch(_stream(stream), _p(src), _p(dst), B, H, W, int(mode), _p(f), _p(apply), _p(coef),
                                   int(dst_stride)), 'ffcv_affine_batch')
    return dst


def affine_batch_host(src: np.ndarray, dst: np.ndarray, mode, fill, apply, coef, nthreads=1):
    """The same on C-contiguous numpy uint8 (B, H, W, 3) arrays."""
    B, H, W = _u8_out_of_place_dims(src, dst, 'affine_batch_host')
    f = fill_u8(fill)
    apply = _per_image('affine_batch_host', 'apply', apply, np.uint8, B)
    coef = _per_image('affine_batch_host', 'coef', coef, np.int64, B, 6)
    _check(lib().ffcv_affine_batch_host(_p(src), _p(dst), B, H, W, int(mode), _p(f), _p(apply), _p(coef), 0,
                                        int(max(1, nthreads))), 'ffcv_affine_batch_host')
    return dst[:B]


MIXUP_U8, MIXUP_F32 = 1, 2  # FFCV_MIXUP_*


def _dense_like(a, b):
    """True when tensors a and b have the same shape and strides and cover
    their storage without gaps (contiguous in some permutation of the axes)."""
    if tuple(a.shape) != tuple(b.shape) or tuple(a.stride()) != tuple(b.stride()):
        return False
    expect = 1
    for size, stride in sorted(((int(n), int(st)) for n, st in zip(a.shape, a.stride()) if n != 1),
                               key=lambda x: x[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def mixup_batch(inp, out, lam, batch_size, same_lambda, stream=None, run=None):
    """ImageMixup on a device uint8 or float32 batch (ffcv_mixup_batch):
    ``out[i] = cast(l * inp[i] + (1 - l) * inp[neighbour])`` in float64, the
    neighbour being sample i - 1, or the last sample of i's own batch of
    ``batch_size`` when i is its first.  ``lam``: device float64, one per
    sample or, with ``same_lambda``, one per batch.  ``inp`` and ``out`` are
    dense, laid out alike, with the samples outermost in memory (a
    channels_last view of a dense buffer is fine), and must not overlap.
    ``run``: diagnostics only, the kernel's run length (1, 2, 4 or 8)."""
    import torch
    dt = {torch.uint8: MIXUP_U8, torch.float32: MIXUP_F32}.get(inp.dtype)
    if dt is None or out.dtype != inp.dtype:
        raise TypeError(f'mixup_batch: uint8 or float32 tensors of one dtype are required, got {inp.dtype} '
                        f'and {out.dtype}')
    n = int(inp.shape[0]) if inp.dim() else 0
    if inp.dim() < 1 or n < 1 or inp.numel() < 1 or not _dense_like(inp, out) or \
            int(inp.stride(0)) * n != inp.numel():
        raise TypeError('mixup_batch: inp and out must be dense tensors of the same shape and strides with the '
                        f'samples outermost in memory, got shapes {tuple(inp.shape)}, {tuple(out.shape)} and '
                        f'strides {tuple(inp.stride())}, {tuple(out.stride())}')
    nb = -(-n // int(batch_size)) if int(batch_size) > 0 else 0
    if lam.dtype != torch.float64 or not lam.is_contiguous() or lam.numel() < (nb if same_lambda else n):
        raise TypeError('mixup_batch: lam must be a contiguous float64 tensor with one value per '
                        + ('batch' if same_lambda else 'sample'))
    args = (_stream(stream), _p(inp), _p(out), n, inp.numel() // n, dt, int(batch_size), _p(lam),
            int(bool(same_lambda)))
    if run is None:
        _check(lib().ffcv_mixup_batch(*args), 'ffcv_mixup_batch')
        return out
    fn = lib().ffcv_mixup_batch_run   # not in ffcv_hip.h: bound on first use
    fn.restype = c_int
    fn.argtypes = _SIGS['ffcv_mixup_batch'][1] + [c_int]
    _check(fn(*args, int(run)), 'ffcv_mixup_batch_run')
    return out


def mixup_batch_host(inp: np.ndarray, out: np.ndarray, lam, batch_size, same_lambda, nthreads=1):
    """The same on C-contiguous numpy uint8 or float32 arrays (samples along
    axis 0), compiled from the kernel's pixel function."""
    dt = {np.dtype(np.uint8): MIXUP_U8, np.dtype(np.float32): MIXUP_F32}.get(inp.dtype)
    if dt is None or out.dtype != inp.dtype or inp.shape != out.shape or inp.ndim < 1 or inp.size < 1 or \
            not inp.flags.c_contiguous or not out.flags.c_contiguous:
        raise TypeError('mixup_batch_host: C-contiguous uint8 or float32 arrays of one shape are required')
    n = int(inp.shape[0])
    lam = np.ascontiguousarray(lam, np.float64).reshape(-1)
    nb = -(-n // int(batch_size)) if int(batch_size) > 0 else 0
    if lam.size < (nb if same_lambda else n):
        raise TypeError('mixup_batch_host: lam needs one value per ' + ('batch' if same_lambda else 'sample'))
    _check(lib().ffcv_mixup_batch_host(_p(inp), _p(out), n, inp.size // n, dt, int(batch_size), _p(lam),
                                       int(bool(same_lambda)), int(max(1, nthreads))), 'ffcv_mixup_batch_host')
    return out


def mixup_onehot_batch(labels3, out, status, stream=None):
    """MixupToOneHot in one launch (ffcv_mixup_onehot_batch): labels3 device
    float32 (n, 3) of (a, b, lam); out device float32 (n, num_classes);
    status device int32 (n,), nonzero where a label is out of range (that
    row stays zero)."""
    import torch
    n = int(labels3.shape[0]) if labels3.dim() == 2 else -1
    if labels3.dtype != torch.float32 or out.dtype != torch.float32 or status.dtype != torch.int32 or \
            labels3.dim() != 2 or int(labels3.shape[1]) != 3 or out.dim() != 2 or int(out.shape[0]) != n or \
            status.numel() != n or not (labels3.is_contiguous() and out.is_contiguous() and status.is_contiguous()):
        raise TypeError('mixup_onehot_batch: contiguous float32 (n, 3) labels, float32 (n, num_classes) out and '
                        'int32 (n,) status are required')
    _check(lib().ffcv_mixup_onehot_batch(_stream(stream), _p(labels3), _p(out), n, int(out.shape[1]), _p(status)),
           'ffcv_mixup_onehot_batch')
    return out


CUTMIX_LAYOUTS = ('auto', 'hwc', 'chw')


def cutmix_geometry(who, x, layout='auto'):
    """(planes, height, width, pixel_bytes) of a batch of images, a torch
    tensor or a numpy array with the samples along axis 0, as
    ffcv_cutmix_batch takes it.  ``'auto'``: a 4-D tensor with
    channels-last strides that is not contiguous is the NCHW view of NHWC
    storage (``H, W = shape[2:]``, one plane); anything contiguous is
    ``(B, H, W, C...)``.  ``'hwc'`` requires the second reading, ``'chw'`` a
    contiguous ``(B, C, H, W)`` (C planes)."""
    if layout not in CUTMIX_LAYOUTS:
        raise ValueError(f'{who}: layout must be one of {CUTMIX_LAYOUTS}, got {layout!r}')
    is_np = isinstance(x, np.ndarray)
    itemsize = int(x.itemsize if is_np else x.element_size())
    ndim = x.ndim if is_np else x.dim()
    shape = tuple(int(v) for v in x.shape)
    if ndim < 3 or min(shape) < 1:
        raise TypeError(f'{who}: a non-empty batch of images (B, H, W, ...) is required, got shape {shape}')
    contiguous = bool(x.flags.c_contiguous) if is_np else x.is_contiguous()
    if layout == 'auto' and not is_np and ndim == 4 and not contiguous:
        import torch
        if x.is_contiguous(memory_format=torch.channels_last):
            return 1, shape[2], shape[3], shape[1] * itemsize
    if not contiguous:
        raise TypeError(f'{who}: the images must be contiguous, or with layout=\'auto\' the NCHW view of channels-last '
                        f'storage, got shape {shape} and strides '
                        f'{tuple(x.strides) if is_np else tuple(x.stride())}')
    if layout == 'chw':
        if ndim != 4:
            raise TypeError(f'{who}: layout=\'chw\' takes (B, C, H, W), got shape {shape}')
        return shape[1], shape[2], shape[3], itemsize
    pixel = itemsize
    for v in shape[3:]:
        pixel *= v
    return 1, shape[1], shape[2], pixel


def _cutmix_boxes_ok(n_boxes, n, batch_size, same_box):
    nb = -(-n // int(batch_size)) if int(batch_size) > 0 else 0
    return n_boxes >= 4 * (nb if same_box else n)


def cutmix_batch(inp, out, boxes, batch_size, same_box, layout='auto', stream=None):
    """ImageCutMix on a device batch of any dtype of 1, 2, 4 or 8 bytes
    (ffcv_cutmix_batch): ``out[i] = inp[i]`` with the box ``[y1:y2, x1:x2]``
    taken from the neighbour, which is sample i - 1, or the last sample of i's
    own batch of ``batch_size`` when i is its first.  ``boxes``: device
    int32 rows of ``(y1, x1, y2, x2)``, one per sample or, with ``same_box``,
    one per batch; they are clamped to the image on the device.  ``inp`` and
    ``out`` are dense, laid out alike, with the samples outermost in memory,
    and must not overlap; ``layout`` as in :func:`cutmix_geometry`."""
    import torch
    if out.dtype != inp.dtype:
        raise TypeError(f'cutmix_batch: tensors of one dtype are required, got {inp.dtype} and {out.dtype}')
    n = int(inp.shape[0]) if inp.dim() else 0
    if inp.dim() < 1 or n < 1 or inp.numel() < 1 or not _dense_like(inp, out) or \
            int(inp.stride(0)) * n != inp.numel():
        raise TypeError('cutmix_batch: inp and out must be dense tensors of the same shape and strides with the '
                        f'samples outermost in memory, got shapes {tuple(inp.shape)}, {tuple(out.shape)} and '
                        f'strides {tuple(inp.stride())}, {tuple(out.stride())}')
    planes, h, w, pb = cutmix_geometry('cutmix_batch', inp, layout)
    if boxes.dtype != torch.int32 or not boxes.is_contiguous() or \
            not _cutmix_boxes_ok(boxes.numel(), n, batch_size, same_box):
        raise TypeError('cutmix_batch: boxes must be a contiguous int32 tensor with one (y1, x1, y2, x2) per '
                        + ('batch' if same_box else 'sample'))
    _check(lib().ffcv_cutmix_batch(_stream(stream), _p(inp), _p(out), n, planes, h, w, pb, int(batch_size), _p(boxes),
                                   int(bool(same_box))), 'ffcv_cutmix_batch')
    return out


def cutmix_batch_host(inp: np.ndarray, out: np.ndarray, boxes, batch_size, same_box, layout='auto', nthreads=1):
    """The same on C-contiguous numpy arrays of any dtype (samples along
    axis 0), with memcpy of row segments."""
    if out.dtype != inp.dtype or inp.shape != out.shape or inp.ndim < 1 or inp.size < 1 or \
            not inp.flags.c_contiguous or not out.flags.c_contiguous:
        raise TypeError('cutmix_batch_host: C-contiguous arrays of one dtype and shape are required')
    planes, h, w, pb = cutmix_geometry('cutmix_batch_host', inp, layout)
    n = int(inp.shape[0])
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1)
    if not _cutmix_boxes_ok(boxes.size, n, batch_size, same_box):
        raise TypeError('cutmix_batch_host: boxes needs one (y1, x1, y2, x2) per ' + ('batch' if same_box else 'sample'))
    _check(lib().ffcv_cutmix_batch_host(_p(inp), _p(out), n, planes, h, w, pb, int(batch_size), _p(boxes),
                                        int(bool(same_box)), int(max(1, nthreads))), 'ffcv_cutmix_batch_host')
    return out


ERASE_CONSTANT, ERASE_NOISE = 0, 1  # FFCV_ERASE_*
ERASE_TABLE = 4096                  # entries of the noise table


def _pair(who, name, v):
    r = np.ascontiguousarray([float(x) for x in v], dtype=np.float64)
    if r.shape != (2,):
        raise TypeError(f'{who}: {name} must be two numbers')
    return r


def erase_draw_batch(ids, loader_seed, epoch, p, scale, ratio, height, width, boxes, keys=None, status=None,
                     stream=None):
    """RandomErasing's draws of the batch on the device (op id 21): boxes
    device int32 (B, 4) of ``(y, x, h, w)``, ``h = w = 0`` where nothing is
    erased; keys device 8-byte integers (B,), the noise keys (op id 22), or
    None."""
    B = int(ids.shape[0])
    if boxes.element_size() != 4 or boxes.numel() < 4 * B or not boxes.is_contiguous() or \
            (keys is not None and (keys.element_size() != 8 or keys.numel() < B or not keys.is_contiguous())):
        raise TypeError('erase_draw_batch: boxes must be a contiguous int32 (B, 4) tensor and keys a contiguous '
                        '8-byte integer (B,) tensor')
    s, r = _pair('erase_draw_batch', 'scale', scale), _pair('erase_draw_batch', 'ratio', ratio)
    _check(lib().ffcv_erase_draw_batch(_stream(stream), _p(ids), B, _seed64(loader_seed), int(epoch), float(p), _p(s),
                                       _p(r), int(height), int(width), _p(boxes), _p(keys), _p(status)),
           'ffcv_erase_draw_batch')


def erase_draw_batch_host(ids, loader_seed, epoch, p, scale, ratio, height, width):
    """The same draws on the host: (boxes int32 (B, 4), keys uint64 (B,))."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
    s, r = _pair('erase_draw_batch_host', 'scale', scale), _pair('erase_draw_batch_host', 'ratio', ratio)
    boxes = np.zeros((ids.size, 4), np.int32)
    keys = np.zeros(ids.size, np.uint64)
    _check(lib().ffcv_erase_draw_batch_host(_p(ids), int(ids.size), _seed64(loader_seed), int(epoch), float(p), _p(s),
                                            _p(r), int(height), int(width), _p(boxes), _p(keys)),
           'ffcv_erase_draw_batch_host')
    return boxes, keys


def _erase_fill_ok(fill, keys, planes, pb, itemsize):
    """The mode of a fill: a pattern of planes x pixel_bytes bytes without keys,
    a table of ERASE_TABLE entries of the images' itemsize with them."""
    is_np = isinstance(fill, np.ndarray)
    size = int(fill.size if is_np else fill.numel())
    isz = int(fill.itemsize if is_np else fill.element_size())
    contiguous = bool(fill.flags.c_contiguous) if is_np else fill.is_contiguous()
    if keys is None:
        return ERASE_CONSTANT if contiguous and size * isz == planes * pb else None
    return ERASE_NOISE if contiguous and size == ERASE_TABLE and isz == itemsize and itemsize in (1, 2, 4) else None


def erase_batch(images, boxes, fill, keys=None, layout='auto', stream=None, form=None):
    """RandomErasing's fill in place on a device batch (ffcv_erase_batch): the
    box ``(y, x, h, w)`` of each sample (device int32 rows, clamped to the
    image on the device; ``h <= 0`` or ``w <= 0``: nothing) is filled in every
    channel.  Without ``keys`` ``fill`` is one pixel of every plane, planes x
    pixel_bytes bytes already in the images' dtype; with ``keys`` (device
    8-byte integers, one per sample) it is the noise table of 4096 entries of
    the images' dtype (itemsize 1, 2 or 4) and every element gets the entry
    its index in the sample selects.  ``images`` is dense with the samples
    outermost in memory; ``layout`` as in :func:`cutmix_geometry`.  ``form``:
    diagnostics only, (workgroups per sample and plane, table staged in LDS)."""
    import torch
    n = int(images.shape[0]) if images.dim() else 0
    if images.dim() < 1 or n < 1 or images.numel() < 1 or images.device.type != 'cuda' or \
            not _dense_like(images, images) or int(images.stride(0)) * n != images.numel():
        raise TypeError('erase_batch: a dense device tensor with the samples outermost in memory is required, got '
                        f'shape {tuple(images.shape)} and strides {tuple(images.stride())}')
    planes, h, w, pb = cutmix_geometry('erase_batch', images, layout)
    if boxes.dtype != torch.int32 or not boxes.is_contiguous() or boxes.numel() < 4 * n:
        raise TypeError('erase_batch: boxes must be a contiguous int32 tensor with one (y, x, h, w) per sample')
    if keys is not None and (keys.element_size() != 8 or not keys.is_contiguous() or keys.numel() < n):
        raise TypeError('erase_batch: keys must be a contiguous tensor of one 8-byte integer per sample')
    itemsize = int(images.element_size())
    mode = _erase_fill_ok(fill, keys, planes, pb, itemsize)
    if mode is None or isinstance(fill, np.ndarray) or fill.device != images.device:
        raise TypeError(f'erase_batch: fill must be a contiguous device tensor of {planes} x {pb} bytes (one pixel of '
                        f'every plane), or with keys a table of {ERASE_TABLE} entries of the images\' dtype')
    args = (_stream(stream), _p(images), n, planes, h, w, pb, _p(boxes), mode, itemsize, _p(fill), _p(keys))
    if form is None:
        _check(lib().ffcv_erase_batch(*args), 'ffcv_erase_batch')
        return images
    fn = lib().ffcv_erase_batch_form   # not in ffcv_hip.h: bound on first use
    fn.restype = c_int
    fn.argtypes = _SIGS['ffcv_erase_batch'][1] + [c_int, c_int]
    _check(fn(*args, int(form[0]), int(bool(form[1]))), 'ffcv_erase_batch_form')
    return images


def erase_batch_host(images: np.ndarray, boxes, fill, keys=None, layout='auto', nthreads=1):
    """The same in place on a writeable C-contiguous numpy array (samples
    along axis 0); ``fill``: the pattern's bytes, or with ``keys`` the table,
    an array of the images' itemsize."""
    if not isinstance(images, np.ndarray) or images.ndim < 1 or images.size < 1 or not images.flags.c_contiguous or \
            not images.flags.writeable:
        raise TypeError('erase_batch_host: a writeable C-contiguous array is required')
    planes, h, w, pb = cutmix_geometry('erase_batch_host', images, layout)
    n = int(images.shape[0])
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1)
    if boxes.size < 4 * n:
        raise TypeError('erase_batch_host: boxes needs one (y, x, h, w) per sample')
    if keys is not None:
        keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
        if keys.size < n:
            raise TypeError('erase_batch_host: keys needs one per sample')
    fill = np.ascontiguousarray(fill)
    mode = _erase_fill_ok(fill, keys, planes, pb, int(images.itemsize))
    if mode is None:
        raise TypeError(f'erase_batch_host: fill must hold {planes} x {pb} bytes (one pixel of every plane), or with '
                        f'keys be a table of {ERASE_TABLE} entries of the images\' itemsize')
    _check(lib().ffcv_erase_batch_host(_p(images), n, planes, h, w, pb, _p(boxes), mode, int(images.itemsize),
                                       _p(fill), _p(keys), int(max(1, nthreads))), 'ffcv_erase_batch_host')
    return images


def _device_ids(who, sample_ids, poison_ids, n, device):
    import torch
    if sample_ids.dtype != torch.int64 or poison_ids.dtype != torch.int64 or sample_ids.numel() != n or \
            poison_ids.dim() != 1 or not (sample_ids.is_contiguous() and poison_ids.is_contiguous()) or \
            sample_ids.device != device or poison_ids.device != device:
        raise TypeError(f'{who}: sample_ids must be a contiguous int64 tensor with one id per sample and poison_ids '
                        'a contiguous 1-D int64 tensor of sorted unique non-negative ids, both on the data\'s device')


def poison_batch(images, sample_ids, poison_ids, keep, add, clamp=(0, 255), stream=None, form=None):
    """Poison in place on a device uint8 batch (ffcv_poison_batch): every
    sample whose id in ``sample_ids`` is one of the sorted ``poison_ids``
    becomes ``uint8(clip(float32(float32(v * keep) + add), *clamp))``.
    ``images`` is C-contiguous with the samples along axis 0 (``keep`` and
    ``add``, device float64, follow a sample's element order); the ids are
    device int64.  ``form``: diagnostics only, the kernel's (bytes per thread,
    run length, workgroups ordered by table chunk)."""
    import torch
    n = int(images.shape[0]) if images.dim() else 0
    if images.dtype != torch.uint8 or images.device.type != 'cuda' or n < 1 or images.numel() < 1 or \
            not images.is_contiguous():
        raise TypeError('poison_batch: a C-contiguous uint8 device tensor with the samples along axis 0 is required, '
                        f'got {images.dtype} {tuple(images.shape)} with strides {tuple(images.stride())}')
    elems = images.numel() // n
    _device_ids('poison_batch', sample_ids, poison_ids, n, images.device)
    for t in (keep, add):
        if t.dtype != torch.float64 or t.numel() != elems or not t.is_contiguous() or t.device != images.device:
            raise TypeError('poison_batch: keep and add must be contiguous float64 device tensors of one sample\'s '
                            f'{elems} elements')
    args = (_stream(stream), _p(images), n, elems, _p(sample_ids), _p(poison_ids), int(poison_ids.numel()), _p(keep),
            _p(add), float(np.float32(clamp[0])), float(np.float32(clamp[1])))
    if form is None:
        _check(lib().ffcv_poison_batch(*args), 'ffcv_poison_batch')
        return images
    fn = lib().ffcv_poison_batch_form   # not in ffcv_hip.h: bound on first use
    fn.restype = c_int
    fn.argtypes = _SIGS['ffcv_poison_batch'][1] + [c_int, c_int, c_int]
    _check(fn(*args, int(form[0]), int(form[1]), int(bool(form[2]))), 'ffcv_poison_batch_form')
    return images


def poison_batch_host(images: np.ndarray, sample_ids, poison_ids, keep, add, clamp=(0, 255), nthreads=1):
    """The same in place on a C-contiguous numpy uint8 array (samples along
    axis 0), compiled from the kernel's membership and pixel functions.
    ``poison_ids``: sorted unique ids (uint64)."""
    if not isinstance(images, np.ndarray) or images.dtype != np.uint8 or images.ndim < 1 or images.size < 1 or \
            not images.flags.c_contiguous or not images.flags.writeable:
        raise TypeError('poison_batch_host: a writeable C-contiguous uint8 array is required')
    n = int(images.shape[0])
    elems = images.size // n
    sample_ids = np.ascontiguousarray(sample_ids).astype(np.int64, copy=False).reshape(-1)
    poison_ids = np.ascontiguousarray(poison_ids, np.uint64).reshape(-1)
    keep = np.ascontiguousarray(keep, np.float64).reshape(-1)
    add = np.ascontiguousarray(add, np.float64).reshape(-1)
    if sample_ids.size != n or keep.size != elems or add.size != elems:
        raise TypeError(f'poison_batch_host: {n} sample ids and keep / add tables of {elems} values are required, '
                        f'got {sample_ids.size}, {keep.size} and {add.size}')
    _check(lib().ffcv_poison_batch_host(_p(images), n, elems, _p(sample_ids), _p(poison_ids), int(poison_ids.size),
                                        _p(keep), _p(add), float(np.float32(clamp[0])), float(np.float32(clamp[1])),
                                        int(max(1, nthreads))), 'ffcv_poison_batch_host')
    return images


def replace_label_batch(labels, sample_ids, poison_ids, new_label, stream=None):
    """ReplaceLabel in place on a contiguous device int64 tensor with one row
    per sample (ffcv_replace_label_batch); ids as for poison_batch."""
    import torch
    n = int(labels.shape[0]) if labels.dim() else 0
    if labels.dtype != torch.int64 or labels.device.type != 'cuda' or n < 1 or labels.numel() < 1 or \
            not labels.is_contiguous():
        raise TypeError(f'replace_label_batch: a contiguous int64 device tensor is required, got {labels.dtype} '
                        f'{tuple(labels.shape)}')
    _device_ids('replace_label_batch', sample_ids, poison_ids, n, labels.device)
    _check(lib().ffcv_replace_label_batch(_stream(stream), _p(labels), n, labels.numel() // n, _p(sample_ids),
                                          _p(poison_ids), int(poison_ids.numel()), int(new_label)),
           'ffcv_replace_label_batch')
    return labels


def scratch_bound(heights, widths, nbytes):
    """ffcv_jpeg_scratch_bound over arrays (numpy restatement of the C
    formula, checked against it in tests/test_abi.py): the most arena bytes
    one image can take, whatever its crop."""
    h = np.asarray(heights, dtype=np.uint64)
    w = np.asarray(widths, dtype=np.uint64)
    n = np.asarray(nbytes, dtype=np.uint64)

    def a256(x):
        return (x + np.uint64(255)) // np.uint64(256) * np.uint64(256)
    blocks = np.uint64(3) * ((w + np.uint64(7)) // np.uint64(8) + np.uint64(4)) * \
        ((h + np.uint64(7)) // np.uint64(8) + np.uint64(4))
    return (a256(n + np.uint64(64)) + a256(blocks * np.uint64(128)) + a256(blocks * np.uint64(2)) +
            a256(blocks * np.uint64(64)) + a256(h * w * np.uint64(3)))


def arena_for(heights, widths, nbytes, max_batch):
    """Arena bytes that no launch of max_batch images of this dataset can
    exhaust: the sum of the max_batch largest per-image bounds."""
    b = scratch_bound(heights, widths, nbytes)
    if max_batch <= 0:
        return 4096
    if b.size > max_batch:
        b = np.partition(b, b.size - max_batch)[b.size - max_batch:]
    # fewer images than a launch (repeated samples: a small dataset, padded
    # distributed orders, replicated benchmark encodings): each extra slot
    # may hold the largest image again
    extra = max(0, max_batch - b.size) * (int(b.max()) if b.size else 0)
    return int(b.sum()) + extra + 4096


EIDX_LANES, EIDX_WORDS = 64, 3  # entropy index record: words per lane range


class JpegDecoder:
    """Owns an ffcv_jpeg_ctx: launch scratch for up to max_batch images in
    one arena of arena_bytes (default: max_batch images of the maximum size)."""

    def __init__(self, max_batch, max_height, max_width, max_bytes, arena_bytes=0):
        self.handle = c_void_p()
        self.max_batch = int(max_batch)
        self.max_height, self.max_width = int(max_height), int(max_width)
        self.max_bytes = int(max_bytes)
        self.arena_bytes = int(arena_bytes)
        _check(lib().ffcv_jpeg_create_arena(ctypes.byref(self.handle), self.max_batch,
                                            self.max_height, self.max_width, self.max_bytes,
                                            self.arena_bytes), 'ffcv_jpeg_create')

    def rrc(self, base, samples, batch, crops, cutout_yx, flips, params: RRCParams, out,
            status, stream=None):
        _check(lib().ffcv_jpeg_rrc_batch(self.handle, _stream(stream), _p(base), _p(samples),
                                         int(batch), _p(crops), _p(cutout_yx), _p(flips),
                                         ctypes.byref(params), _p(out), _p(status)),
               'ffcv_jpeg_rrc_batch')

    def rrc_fused(self, base, table, ids, draw: DrawParams, crops, cutout_yx, flips,
                  params: RRCParams, out, status, samples_out=None, stream=None):
        """gather + draws + decode/crop/resize/epilogue (ffcv_jpeg_rrc_fused)."""
        _check(lib().ffcv_jpeg_rrc_fused(self.handle, _stream(stream), _p(base), _p(table),
                                         table.numel() // 32, _p(ids), int(ids.shape[0]),
                                         ctypes.byref(draw), _p(crops), _p(cutout_yx), _p(flips),
                                         _p(samples_out), ctypes.byref(params), _p(out),
                                         _p(status)), 'ffcv_jpeg_rrc_fused')

    def decode(self, base, samples, batch, out, out_stride, status, stream=None):
        _check(lib().ffcv_jpeg_decode_batch(self.handle, _stream(stream), _p(base), _p(samples),
                                            int(batch), _p(out), int(out_stride), _p(status)),
               'ffcv_jpeg_decode_batch')

    def set_diag(self, only=7):
        """Diagnostics: kernels a launch runs (bit 0 K1, bit 1 the IDCT
        kernel, bit 2 K2), fixed on this context (never read per launch).  The
        C entry point's third argument (the K2 timing-only flags of rounds
        1-4) must be 0 and is always passed as 0 here."""
        _check(lib().ffcv_jpeg_set_diag(self.handle, int(only), 0), 'ffcv_jpeg_set_diag')

    def arena_used(self, stream=None):
        """(bytes the last entropy launch allocated, arena capacity)."""
        used, cap = c_uint64(), c_uint64()
        _check(lib().ffcv_jpeg_arena_used(self.handle, _stream(stream), ctypes.byref(used), ctypes.byref(cap)),
               'ffcv_jpeg_arena_used')
        return used.value, cap.value

    def set_entropy_index(self, index):
        """Attach (or, with None, detach) an entropy index: a zeroed uint32
        device tensor of shape (n_samples, 64, 3) that fused launches fill
        and then use to skip the Huffman sync of samples decoded before."""
        if index is None:
            _check(lib().ffcv_jpeg_set_entropy_index(self.handle, None, 0), 'ffcv_jpeg_set_entropy_index')
            self._eidx = None
            return
        if index.dim() != 3 or tuple(index.shape[1:]) != (EIDX_LANES, EIDX_WORDS) or \
                index.element_size() != 4 or not index.is_contiguous() or not index.is_cuda:
            raise ValueError('entropy index must be a contiguous 4-byte device tensor of shape '
                             f'(n, {EIDX_LANES}, {EIDX_WORDS})')
        _check(lib().ffcv_jpeg_set_entropy_index(self.handle, _p(index), int(index.shape[0])),
               'ffcv_jpeg_set_entropy_index')
        self._eidx = index  # keep it alive while attached

    def set_timing(self, max_launches):
        """Record HIP events around each kernel of the next max_launches RRC
        launches (0: off); timing_read() returns their durations."""
        self._tcap = int(max_launches)
        _check(lib().ffcv_jpeg_set_timing(self.handle, self._tcap), 'ffcv_jpeg_set_timing')

    def timing_read(self):
        """ms[launch, kernel] (kernel 0 entropy, 1 IDCT, 2 colour/resize) of
        the launches recorded since set_timing / the last read."""
        cap = getattr(self, '_tcap', 0)
        ms = np.zeros((max(1, cap), 3), np.float32)
        n = c_int()
        _check(lib().ffcv_jpeg_timing_read(self.handle, _p(ms), cap, ctypes.byref(n)), 'ffcv_jpeg_timing_read')
        return ms[:n.value]

    def coefficients(self, base, samples, batch, out, max_blocks, status, stream=None):
        _check(lib().ffcv_jpeg_coefficients_batch(self.handle, _stream(stream), _p(base),
                                                  _p(samples), int(batch), _p(out),
                                                  int(max_blocks), _p(status)),
               'ffcv_jpeg_coefficients_batch')

    def close(self):
        if self.handle:
            lib().ffcv_jpeg_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
