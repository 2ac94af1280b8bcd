"""RandomResizedCrop (ffcv/transforms/random_resized_crop.py:14-57).

Each uint8 (H, W, 3) image of the batch is cut to a random window and the
window resized to ``size x size``: the window is ``get_random_crop(H, W,
scale, ratio)`` (fast_crop.py; torchvision's rule) drawn from the sample's own
MT19937 under the seeding contract (op id 8, not the crop
decoder's id 1), the resize is ``cv::resize(INTER_AREA)`` (resize_crop).

The reference recommends the decoder form for variable-size JPEG datasets.
This transform is for fixed-size datasets read by SimpleRGBImageDecoder, where
the crop follows another operation (Poison, colour jitter, RandomTranslate) or
replaces pad-and-crop.

On device tensors it is the draws plus ONE launch (ffcv_rrc_images_batch: a
workgroup per image that stages the crop in LDS; larger images run the raw
decoder's band kernel).  The graph lowering absorbs a following Cutout /
RandomHorizontalFlip / NormalizeImage(float16) into that launch
(``_lower_rrc_transform``).  On host arrays it is the host draws plus
``resize()`` per image over the Loader's threads.
"""
import numbers
from dataclasses import replace
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.epilogue import FusesEpilogue
from ..pipeline.operation import Operation
from ..pipeline.state import State
from ..pipeline import runtime
from .u8_image import check_u8_images


class RandomResizedCrop(FusesEpilogue, Operation):
    """Crop a random portion of image with random aspect ratio and resize it to
    a given size.

    Parameters
    ----------
    scale : Tuple[float, float]
        Lower and upper bounds for the ratio of random area of the crop.
    ratio : Tuple[float, float]
        Lower and upper bounds for random aspect ratio of the crop.
    size : int
        Side length of the output.
    """
    device_aware = True
    per_sample = True

    def __init__(self, scale: Tuple[float, float], ratio: Tuple[float, float], size: int):
        super().__init__()
        if isinstance(size, bool) or not isinstance(size, numbers.Integral) or size <= 0:
            raise ValueError(f'RandomResizedCrop: size must be an int > 0, got {size!r}')
        self.scale = scale
        self.ratio = ratio
        self.size = int(size)
        # graph lowering hook (fuse): the Cutout / RandomHorizontalFlip / fp16
        # NormalizeImage behind this transform that its launch applies
        self.fuse()

    @property
    def fused(self):
        return bool(self._epilogue)

    def _ranges(self):
        scale = tuple(float(x) for x in np.asarray(self.scale, np.float64).reshape(-1))
        ratio = tuple(float(x) for x in np.asarray(self.ratio, np.float64).reshape(-1))
        if len(scale) != 2 or len(ratio) != 2:
            raise ValueError(f'RandomResizedCrop: scale and ratio are (low, high) pairs, got {self.scale!r}, '
                             f'{self.ratio!r}')
        return scale, ratio

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        scale, ratio = self._ranges()
        size = self.size
        ep = self._epilogue
        cut, flip, norm = ep.cutout, ep.flip, ep.normalize
        rp = ep.fill_rrc_params(L.RRCParams())
        rp.out_h = rp.out_w = size
        key = ('rrc_transform', id(self))

        def random_resized_crop(images, storage, indices):
            dst, crops = storage
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                if not images.is_contiguous():
                    raise TypeError('RandomResizedCrop: a contiguous (B, H, W, 3) batch is required')
                B, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
                stream = ctx.stream
                L.crop_draw_batch(ctx.batch_ids, H, W, scale, ratio, ctx.loader_seed, ctx.epoch, crops, None, stream)
                cyx = flips = None
                if cut is not None or flip is not None:
                    dp = ep.draw_params(ctx.loader_seed, ctx.epoch, size, size)
                    if cut is not None:
                        cyx = ctx.device_buffer(key + ('cut',), 2 * ctx.batch_size, ch.int32)
                    if flip is not None:
                        flips = ctx.device_buffer(key + ('flip',), ctx.batch_size, ch.uint8)
                    L.draw_batch(ctx.batch_ids, None, dp, None, cyx, flips, None, stream)
                ws = None
                nws = L.rrc_images_workspace_bytes(ctx.batch_size, H, W, size, size)
                if nws:
                    ws = ctx.device_buffer(key + ('ws', H, W), nws, ch.uint8)
                out = dst[:B]
                if norm is not None:
                    rp.lut = norm.device_lut(out.device).data_ptr()
                rp.out_stride = out[0].numel() * out.element_size()
                L.rrc_images_batch(images, H * W * 3, B, H, W, crops, cyx, flips, rp, out, None, ws, stream)
                return out
            if cut is not None or flip is not None or norm is not None:
                raise RuntimeError('RandomResizedCrop: operations were fused into its device launch, but it '
                                   'received host data')
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            src = images.numpy() if isinstance(images, ch.Tensor) else images
            src = np.ascontiguousarray(src)
            B = len(indices)
            out = dst[:B]
            out_np = out.numpy() if isinstance(out, ch.Tensor) else out
            from ..pipeline.compiler import Compiler
            cr = L.crop_draw_batch_host(np.asarray(indices, np.uint64), src.shape[1], src.shape[2], scale, ratio,
                                        seed, epoch)
            crops_np = crops.numpy() if isinstance(crops, ch.Tensor) else crops
            crops_np[:B] = cr
            L.rrc_images_batch_host(src[:B], cr, out_np, None, nthreads=max(1, int(Compiler.num_threads)))
            return out
        random_resized_crop.is_parallel = True
        random_resized_crop.with_indices = True
        return random_resized_crop

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        dt, _ = check_u8_images('RandomResizedCrop', previous_state)
        self._ranges()
        out_shape = (self.size, self.size, 3)
        on_dev = previous_state.device.type == 'cuda'
        if on_dev:
            out_dt = self._epilogue.output_dtype(dt)
            return (replace(previous_state, jit_mode=False, shape=out_shape, dtype=out_dt),
                    (AllocationQuery(out_shape, out_dt, previous_state.device),
                     AllocationQuery((4,), ch.int32, previous_state.device)))   # crop window
        return (replace(previous_state, jit_mode=not isinstance(dt, ch.dtype), shape=out_shape),
                (AllocationQuery(out_shape, dt),
                 AllocationQuery((4,), ch.int32 if isinstance(dt, ch.dtype) else np.dtype('<i4'))))
