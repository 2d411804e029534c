"""Decoded images kept on the device: each file is decoded once per process, later reads are a dictionary lookup.

The value is what `DecodeAhead.planar` and `datasets.read_image` hand to the mapper -- a uint8 (3, H, W) tensor on the device --
and an insert keeps the very tensor the loader produced anyway (the output of the one unpack launch, or the serial path's
host -> device copy): no copy and no launch of its own.  A hit launches nothing.

Insert-only: nothing is ever evicted; an image that does not fit into what is left of `budget_bytes` is not cached and is
decoded again next time.  The key is (realpath, st_size, st_mtime_ns, bgr), so a rewritten file is a different entry (the stale
one stays and keeps its bytes: no eviction).  `bytes_used` counts 3 * H * W per image; the device allocator rounds every
tensor up to its block size (512 bytes), which matters only for thumbnails.

Cached tensors are shared with every later reader and are therefore never written to: the mapper, the augmentations and the
test records all produce new tensors (data/build.py clones the one case that would hand the source itself on).

Only the consuming thread of a loader touches the cache; the decode workers never do.  Under DDP each rank owns its cache."""
import os
from typing import Dict, Iterator, Optional, Tuple

import torch

Key = Tuple[str, int, int, bool]


class DeviceImageCache:
    def __init__(self, budget_bytes: int, device):
        if isinstance(budget_bytes, bool) or not isinstance(budget_bytes, int) or budget_bytes < 0:
            raise ValueError(f"DeviceImageCache: budget_bytes must be a non-negative integer, got {budget_bytes!r}")
        self.budget_bytes = budget_bytes
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:       # tensors report their index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.bytes_used = 0
        self.hits = 0              # lookups answered from the cache
        self.misses = 0            # lookups that were not (the image was then decoded)
        self._images: Dict[Key, torch.Tensor] = {}

    @staticmethod
    def key(file_name: str, bgr: bool) -> Optional[Key]:
        """the key of the file as it is now; None when it cannot be stat'ed (the decode then reports what is wrong with it)"""
        try:
            path = os.path.realpath(file_name)
            st = os.stat(path)
        except OSError:
            return None
        return path, st.st_size, st.st_mtime_ns, bool(bgr)

    def lookup(self, file_name: str, bgr: bool) -> Tuple[Optional[Key], Optional[torch.Tensor]]:
        """(key, cached image or None); counts a hit or a miss.  The key goes back into `insert` once the image is decoded."""
        key = self.key(file_name, bgr)
        img = self._images.get(key) if key is not None else None
        if img is None:
            self.misses += 1
        else:
            self.hits += 1
        return key, img

    def insert(self, key: Optional[Key], image: torch.Tensor) -> bool:
        """Keep `image` (not a copy of it) under `key` if it fits; True when it is cached now.  The caller no longer writes
        to a tensor it has inserted."""
        if key is None:
            return False
        if key in self._images:                    # decoded twice within one look-ahead window: the first one stays
            return True
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[0] != 3 or image.device != self.device:
            raise ValueError(f"DeviceImageCache: expected a uint8 (3, H, W) tensor on {self.device}, got {image.dtype} "
                             f"{tuple(image.shape)} on {image.device}")
        size = image.numel()
        if self.bytes_used + size > self.budget_bytes:
            return False
        self._images[key] = image
        self.bytes_used += size
        return True

    def __len__(self) -> int:
        return len(self._images)

    def items(self) -> Iterator[Tuple[Key, torch.Tensor]]:
        return iter(self._images.items())

    def __repr__(self) -> str:
        return (f"DeviceImageCache({len(self)} images, {self.bytes_used} of {self.budget_bytes} bytes on {self.device}, "
                f"{self.hits} hits, {self.misses} misses)")
