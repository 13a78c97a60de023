"""``Collage``: the reference's image-logging callback (utils/collage.py:29-121) without Lightning, torchvision or PIL.  Methods of the
module decorated with ``Collage.log_method`` return lists of image batches; the callback lays their first ``num_samples`` samples out
side by side (``functional.collage``: one kernel, no concatenated temporary) and hands the grid to the logger.  Loggers are duck-typed:
``logger.log_image(key, [collage], step=)`` (the W&B form) when present, else ``logger.experiment.add_image(key, collage, global_step=)``
(the TensorBoard form); without a logger the collage is written to ``collages/{step:04d}_{func}.png``."""
import os
import struct
import warnings
import zlib
from typing import Any, List, Optional

from torch import Tensor

from .. import functional as HF

__all__ = ["Collage", "write_png"]


def write_png(path: str, image) -> None:
    """8-bit RGB PNG of a uint8 [H, W, 3] array (numpy array or CPU tensor): signature, IHDR, one IDAT of filter-0 scanlines, IEND."""
    import numpy as np
    arr = np.ascontiguousarray(image.numpy() if isinstance(image, Tensor) else image)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"write_png takes a uint8 [H, W, 3] image, got {arr.dtype} {arr.shape}")
    h, w = arr.shape[:2]

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    rows = np.concatenate([np.zeros((h, 1), np.uint8), arr.reshape(h, w * 3)], axis=1)   # filter type 0 in front of every scanline
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


class Collage:
    def __init__(self, log_interval: int = 100, num_samples: int = 8) -> None:
        """:param log_interval: number of steps between logging.  :param num_samples: number of images displayed in the grid."""
        self.log_interval = log_interval
        self.num_samples = num_samples

    @staticmethod
    def log_method(method):
        """Decorates a method to mark it as a method which outputs a list of images to log"""
        method.is_collage = True
        return method

    @staticmethod
    def list_to_collage(images: List[Tensor], num_samples: int, as_uint8: bool = False) -> Optional[Tensor]:
        if len(images) == 0:
            return None
        return HF.collage(images, num_samples, as_uint8=as_uint8)

    def log_images(self, trainer, pl_module, batch: Any, mode: str = "val") -> None:
        found = False
        for func in dir(pl_module):
            try:
                method = getattr(pl_module, func)
            except Exception:   # a property that cannot be evaluated now is no method
                continue
            if not (callable(method) and getattr(method, "is_collage", False) is True):
                continue
            found = True
            images = method(pl_module.batch_preprocess(batch))
            if len(images) == 0:
                continue
            logger = getattr(trainer, "logger", None)
            step = getattr(trainer, "global_step", 0)
            key = f"{mode}/collage/{func}"
            if logger is None:
                warnings.warn("No logger found. Logging locally.")
                os.makedirs("collages", exist_ok=True)
                write_png(f"collages/{str(step).zfill(4)}_{func}.png", self.list_to_collage(images, self.num_samples, as_uint8=True).cpu())
            elif hasattr(logger, "log_image"):
                logger.log_image(key, [self.list_to_collage(images, self.num_samples)], step=step)
            elif hasattr(getattr(logger, "experiment", None), "add_image"):
                logger.experiment.add_image(key, self.list_to_collage(images, self.num_samples), global_step=step)
            else:
                raise NotImplementedError(f"Image logging for class {type(logger)} not supported")
        if not found:
            warnings.warn("`Collage` didn't find any method of the module which is marked as a collage method and should have its "
                          "outputs logged. Use the @Collage.log_method decorator in order to have a method affected by the callback.")

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch: Any, batch_idx: int, dataloader_idx: int = 0) -> None:
        if batch_idx == 0 and getattr(trainer, "is_global_zero", True):
            self.log_images(trainer, pl_module, batch, "val")

    def on_test_batch_end(self, trainer, pl_module, outputs, batch: Any, batch_idx: int, unused: Optional[int] = 0) -> None:
        if batch_idx == 0 and getattr(trainer, "is_global_zero", True):
            self.log_images(trainer, pl_module, batch, "test")
