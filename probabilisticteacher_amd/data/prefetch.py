"""Decode-ahead for the loaders: cfg.DATALOADER.NUM_WORKERS threads run the host half of `datasets.read_image` (Pillow decode
-> packed RGB bytes) ahead of the training thread, into pinned host slabs; the consuming thread copies a chunk's slabs to the
device asynchronously and turns them into the planar records with one `unpack_hwc_batch` launch.

Threads, not processes: Pillow's decoders release the GIL, and a worker process would have to stay clear of the GPU that its
parent holds (the reference's DataLoader workers are processes because its mapper runs PIL / torchvision Python code per image;
here that work is on the device).  All randomness and every device call stay on the consuming thread, so the record stream
does not depend on the number of workers.

Bounds: at most LOOKAHEAD_STEPS steps' worth of images (`max_in_flight`) are submitted and not yet handed back, and the ring
holds at most that many pinned slabs, each as large as the largest image it has carried.

With a `DeviceImageCache` (data/cache.py) a file that is already resident is not decoded at all: its ticket is done when it is
submitted, takes no slab and no worker, and planar() hands out the cached tensor.  The misses are decoded, copied and unpacked
as without a cache, and the tensors that one unpack launch wrote are what the cache keeps.  Only the consuming thread looks
into the cache or inserts."""
import collections
import queue
import threading
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import datasets

LOOKAHEAD_STEPS = 2                # how many steps' images may be decoded ahead of the consumer
THREAD_NAME = "ptmi-decode"        # worker threads are named THREAD_NAME-<k>


def max_in_flight(images_per_step: int) -> int:
    """the look-ahead bound: decodes submitted and not yet released, and the number of pinned slabs"""
    return LOOKAHEAD_STEPS * int(images_per_step)


def num_workers(cfg) -> int:
    """cfg.DATALOADER.NUM_WORKERS, checked: 0 = decode on the consuming thread (the serial path), n > 0 = n decode threads"""
    n = cfg.DATALOADER.NUM_WORKERS
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"DATALOADER.NUM_WORKERS must be a non-negative integer, got {n!r}")
    return n


class _Slab:
    """one pinned staging buffer of the ring; `event` is recorded behind the last host -> device copy that read it"""
    __slots__ = ("buf", "event")

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.event = None


class _Ticket:
    __slots__ = ("item", "file_name", "slab", "array", "error", "done", "key", "image")

    def __init__(self, item, file_name: str, slab: Optional[_Slab]):
        self.item, self.file_name, self.slab = item, file_name, slab
        self.array: Optional[np.ndarray] = None      # (H, W, 3) uint8: a view of the slab, or the decoder's own array
        self.key = None                              # with an image cache: the file's key there
        self.image: Optional[torch.Tensor] = None    # a cache hit: the resident (3, H, W) tensor, and nothing to decode
        self.error: Optional[BaseException] = None
        self.done = threading.Event()


def _decode(ticket: _Ticket) -> None:
    try:
        arr = datasets.read_image_hwc(ticket.file_name)           # looked up per call: tests substitute it
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError(f"decoded image is {arr.dtype} {arr.shape}, expected uint8 (H, W, 3)")
        slab = ticket.slab
        if slab is not None:
            if slab.buf is None or slab.buf.numel() < arr.size:    # grows to the largest image seen
                slab.buf = torch.empty(arr.size, dtype=torch.uint8, pin_memory=True)
            view = slab.buf[:arr.size].numpy().reshape(arr.shape)
            np.copyto(view, arr)
            arr = view
        ticket.array = arr
    except Exception as e:                                         # handed to the consumer at this sample's position
        ticket.error = e
    finally:
        ticket.done.set()


def _worker(tasks: "queue.SimpleQueue", stop: threading.Event) -> None:
    while True:
        ticket = tasks.get()
        if ticket is None:
            return
        if stop.is_set():
            ticket.error = RuntimeError("decode pool closed")
            ticket.done.set()
            continue
        _decode(ticket)


class DecodeAhead:
    """Ordered decode-ahead over `items` (any iterable, also an endless one); `file_of(item)` names the image file.

    take(n) hands out the next up to n items with their decoded images, in the order of `items`; planar() turns what was taken
    into (3, H, W) tensors on `device`; release() gives the slabs back.  Everything but the decode itself runs on the calling
    thread.  The worker threads are daemons and hold no reference to this object: close(), or dropping the object, stops them.

    cache: a DeviceImageCache on `device`; `bgr` is then the channel order planar() will be asked for (it is part of the key,
    and a hit is decided at submission)."""

    def __init__(self, items: Iterable, file_of: Callable[[object], str], workers: int, in_flight: int, device,
                 cache=None, bgr: Optional[bool] = None):
        assert workers > 0 and in_flight > 0
        assert cache is None or bgr is not None, "with a cache the channel order is fixed when the object is made"
        self._cache, self._bgr = cache, bgr
        self._items = iter(items)
        self._file_of = file_of
        self._bound = in_flight
        self.device = torch.device(device)
        self._pinned = self.device.type == "cuda"
        self._pending = collections.deque()         # submitted, not yet taken
        self._held = 0                              # taken, not yet released
        self._free = collections.deque()            # released slabs, oldest first
        self._slabs = 0
        self._exhausted = False
        self._tasks: "queue.SimpleQueue" = queue.SimpleQueue()
        self._stop = threading.Event()
        self._workers = workers
        self._threads: List[threading.Thread] = []  # started with the first submission

    def _slab(self) -> Optional[_Slab]:
        if not self._pinned:
            return None
        if self._free:
            slab = self._free.popleft()
            if slab.event is not None:
                slab.event.synchronize()            # the copy that read it has completed: the slab may be overwritten
                slab.event = None
            return slab
        assert self._slabs < self._bound
        self._slabs += 1
        return _Slab()

    def _top_up(self) -> None:
        if not self._threads and not self._stop.is_set():
            self._threads = [threading.Thread(target=_worker, args=(self._tasks, self._stop), name=f"{THREAD_NAME}-{k}", daemon=True)
                             for k in range(self._workers)]
            for t in self._threads:
                t.start()
        while not self._exhausted and not self._stop.is_set() and len(self._pending) + self._held < self._bound:
            try:
                item = next(self._items)
            except StopIteration:
                self._exhausted = True
                return
            file_name = self._file_of(item)
            key, image = self._cache.lookup(file_name, self._bgr) if self._cache is not None else (None, None)
            ticket = _Ticket(item, file_name, self._slab() if image is None else None)
            ticket.key, ticket.image = key, image
            self._pending.append(ticket)
            if image is None:
                self._tasks.put(ticket)
            else:                                   # resident: done as submitted, no slab, no task; it keeps its place in line
                ticket.done.set()

    def take(self, n: int, multiple: int = 1) -> List[_Ticket]:
        """The next up to n tickets (fewer at the end of `items`), a multiple of `multiple` of them.  A failed decode raises
        when its sample (its group of `multiple`) is the next one to hand out: the samples in front of it come out first."""
        assert self._held == 0, "release() what was taken first"
        self._top_up()
        out: List[_Ticket] = []
        while len(out) < n and len(out) < len(self._pending):
            t = self._pending[len(out)]
            t.done.wait()
            if t.error is not None:
                break
            out.append(t)
        out = out[:len(out) - len(out) % multiple]
        if not out:
            for t in list(self._pending)[:multiple]:
                t.done.wait()
                if t.error is not None:
                    self.close()
                    raise RuntimeError(f"decoding {t.file_name} failed: {type(t.error).__name__}: {t.error}") from t.error
            return out                              # `items` is exhausted
        for _ in out:
            self._pending.popleft()
        self._held = len(out)
        return out

    def planar(self, tickets: List[_Ticket], bgr: bool) -> List[torch.Tensor]:
        """what `datasets.read_image` returns for the taken images, on the device: one async copy per image and one unpack
        launch for all of them ("cpu": the reorder of read_image itself).  With a cache only the misses are copied and
        unpacked, the cache keeps what the launch wrote, and hits and misses come back in ticket order."""
        if self._cache is None:
            return self._unpack(tickets, bgr)
        assert bool(bgr) == bool(self._bgr), "the cache was keyed for the other channel order"
        misses = [t for t in tickets if t.image is None]
        for t, img in zip(misses, self._unpack(misses, bgr) if misses else ()):
            t.image = img
            self._cache.insert(t.key, img)
        return [t.image for t in tickets]

    def _unpack(self, tickets: List[_Ticket], bgr: bool) -> List[torch.Tensor]:
        if not self._pinned:
            return [torch.from_numpy(np.ascontiguousarray((t.array[:, :, ::-1] if bgr else t.array).transpose(2, 0, 1)))
                    for t in tickets]
        from .augment import unpack_hwc_batch
        srcs = []
        for t in tickets:
            h, w, _ = t.array.shape
            d = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
            d.view(-1).copy_(t.slab.buf[:d.numel()], non_blocking=True)
            srcs.append(d)
        event = torch.cuda.Event()
        event.record()                              # on the current stream, behind the copies
        for t in tickets:
            t.slab.event = event
        return unpack_hwc_batch(srcs, bgr)

    def release(self, tickets: List[_Ticket]) -> None:
        for t in tickets:
            if t.slab is not None:
                self._free.append(t.slab)
            t.array = t.slab = t.image = None
        self._held -= len(tickets)
        self._top_up()

    def take_planar(self, n: int, bgr: bool, multiple: int = 1) -> List[Tuple[object, torch.Tensor]]:
        """take + planar + release: [(item, uint8 (3, H, W) tensor on the device)]"""
        tickets = self.take(n, multiple)
        imgs = self.planar(tickets, bgr)
        items = [t.item for t in tickets]
        self.release(tickets)
        return list(zip(items, imgs))

    def close(self) -> None:
        if self._stop.is_set():
            return
        self._stop.set()
        for _ in self._threads:
            self._tasks.put(None)
        for t in self._threads:
            if t is not threading.current_thread():
                t.join(timeout=30.0)
        self._pending.clear()
        self._free.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
