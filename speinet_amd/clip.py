"""The clip as a source, for the clip loop (speinet_amd.video), the labelling pass (speinet_amd.detector), the loaders (speinet_amd.data),
blur synthesis (speinet_amd.blurset) and the harness (speinet_amd.inference).  `frames_of` validates a clip in any form the clip API takes
and returns it as `Frames`: frame i on the host or on the device, a rectangle of every frame (`view`), a subset of the frames (`sample`),
one field of every interlaced frame (`woven`, `field`);
a clip of unknown length (a `y4m.Y4MStream`, an iterator of frames) as `StreamFrames`, the same interface over a bounded ring of frames
that one reader thread fills (`FrameRing`).
Frames cross PCIe as uint8 (a deep clip's as its bytes) from page-locked staging buffers (`FrameCache`) and are decoded, for image paths, on
worker threads a few windows ahead; finished frames land in page-locked memory for worker threads (`HostRing`).  `imread` / `imwrite`: the
image codec of every tool.  `mattes_of` does for the mattes of a clip (`deblur_clip(..., matte=)`) what `frames_of` does for its frames:
`Mattes`, matte i on the host or the device, whether it is empty, and the bounding box of them all."""
from __future__ import annotations

import collections
import copy
import os
from concurrent.futures import Future, ThreadPoolExecutor
from typing import Optional

import numpy as np
import torch

from . import ops, y4m

MIN_SIZE = 20
IMAGE_EXTS = (".png", ".jpg", ".jpeg", ".bmp")

padded_size = ops.padded_size


def imread(path: str) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def imwrite(path: str, img: np.ndarray) -> None:
    """Lossless PNG at zlib level 1: the reference writes with cv2.imwrite's default, OpenCV's "best speed" PNG setting
    (inference_SPEINet.py:415-417); PIL's own default (level 6) costs twice the encode time for 10 % smaller files."""
    from PIL import Image
    Image.fromarray(img).save(path, compress_level=1)


class FrameCache:
    """Decode-once, upload-once cache of frames: `load(key)` decodes one (host uint8 [H,W,3]).  `request(keys)` schedules decodes on
    the thread pool; `get_dev(key)` returns the frame on the device, uploaded once however many windows share it (a frame is a
    neighbour twice, a middle frame once and often a reference).  Uploads go through a small ring of page-locked staging buffers
    allocated once: a copy from pageable memory makes the host wait for everything queued on the stream before it (one full GPU drain
    per window), and allocating page-locked memory per frame synchronises the device.  Bounded LRUs (a 720p RGB frame is 2.8 MB)."""
    RING = 8

    def __init__(self, pool: ThreadPoolExecutor, load, device, capacity: int = 16, convert=None):
        self.pool, self.load, self.device, self.capacity = pool, load, device, capacity
        self.convert = convert           # uploaded bytes -> the frame that is kept (planar YUV -> packed RGB, on the device)
        self.items: "collections.OrderedDict[object, Future]" = collections.OrderedDict()
        self.dev: "collections.OrderedDict[object, torch.Tensor]" = collections.OrderedDict()
        self._ring, self._events, self._n = [], [], 0

    def request(self, keys) -> None:
        for p in keys:
            if p in self.items:
                self.items.move_to_end(p)
            elif p not in self.dev:
                self.items[p] = self.pool.submit(self.load, p)
        while len(self.items) > self.capacity:
            self.items.popitem(last=False)

    def _upload(self, arr: np.ndarray) -> torch.Tensor:
        n = arr.nbytes
        if not self._ring or self._ring[0].numel() < n:
            self._ring = [torch.empty(n, dtype=torch.uint8, pin_memory=True) for _ in range(self.RING)]
            self._events = [None] * self.RING
        i = self._n % self.RING
        self._n += 1
        if self._events[i] is not None:
            self._events[i].synchronize()                 # the copy issued RING uploads ago: long finished
        stage = self._ring[i][:n]
        if arr.dtype == np.uint16:                        # a deep frame crosses as its bytes
            stage = stage.view(torch.uint16)
        stage = stage.view(arr.shape)
        stage.numpy()[...] = arr
        t = stage.to(self.device, non_blocking=True)
        self._events[i] = torch.cuda.Event()
        self._events[i].record()
        return t

    def get_dev(self, key) -> torch.Tensor:
        t = self.dev.get(key)
        if t is None:
            self.request([key])
            t = self._upload(self.items.pop(key).result())
            t = self.dev[key] = t if self.convert is None else self.convert(t)
            while len(self.dev) > self.capacity:
                self.dev.popitem(last=False)
        else:
            self.dev.move_to_end(key)
        return t


class HostRing:
    """Finished frames landed in page-locked memory for worker threads: `land(fn, *tensors)` queues the device->host copies of the
    tensors on the current stream, behind whatever produced them, and returns the future of `fn(*host_tensors)`, which runs on the
    pool once those copies are done.  A worker waits on its own copies only: a `.cpu()` from a worker thread is a synchronous copy on
    the stream and would wait for every window queued after its own as well.  `n` slots in turn, a slot reused once its last worker
    has finished; the buffers are allocated once per set of shapes (allocating page-locked memory synchronises the device)."""

    def __init__(self, pool: ThreadPoolExecutor, n: int = 8):
        self.pool, self.n, self.k = pool, n, 0
        self.bufs, self.futs = [], [None] * n

    def land(self, fn, *tensors) -> Future:
        if not self.bufs or [(b.shape, b.dtype) for b in self.bufs[0]] != [(t.shape, t.dtype) for t in tensors]:
            self.drain()
            self.bufs = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors] for _ in range(self.n)]
        i = self.k % self.n
        self.k += 1
        if self.futs[i] is not None:
            self.futs[i].result()
        for b, t in zip(self.bufs[i], tensors):
            b.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.futs[i] = self.pool.submit(self._work, fn, ev, self.bufs[i])
        return self.futs[i]

    @staticmethod
    def _work(fn, ev, bufs):
        ev.synchronize()
        return fn(*bufs)

    def drain(self) -> None:
        for f in self.futs:
            if f is not None:
                f.result()


class RecordQueue:
    """Host records handed to a pool of one thread, which writes them in the order queued: `put(fn, record)` copies the record (the
    caller's buffer may be a view of a ring that moves on) and queues `fn(copy)`.  At most `n` writes are in flight: with `n` queued
    `put` first waits for the oldest, as `HostRing.land` waits for the slot it used `n` frames earlier, so a producer that outruns the
    sink holds `n` records, not the clip.  An error in a write is raised by the `put` or the `drain` that waits for it."""

    def __init__(self, pool: ThreadPoolExecutor, n: int = 8):
        self.pool, self.n, self.futs = pool, n, collections.deque()

    @property
    def in_flight(self) -> int:
        """Writes queued and not yet waited for: an upper bound of those not yet done."""
        return len(self.futs)

    def put(self, fn, record: np.ndarray) -> None:
        while len(self.futs) >= self.n:
            self.futs.popleft().result()
        self.futs.append(self.pool.submit(fn, np.array(record)))

    def drain(self) -> None:
        while self.futs:
            self.futs.popleft().result()


def reflect_index(n: int, n_pad: Optional[int] = None) -> np.ndarray:
    """Source row (or column) of each of the n_pad padded rows of a dimension of n: i < n reads i, n + j reads n - 2 - j (torch F.pad
    mode "reflect"; what spei_frames_u8_in computes in its pad band)."""
    n_pad = padded_size(n) if n_pad is None else n_pad
    if not n_pad - n < n:
        raise ValueError(f"reflect padding of {n} to {n_pad} needs a pad smaller than {n}")
    i = np.arange(n_pad)
    return np.where(i < n, i, 2 * n - 2 - i)


class Frames:
    """The clip behind one interface: frame i as a host uint8 [H,W,3] array (`host`) or a device tensor (`device`), cropped at the
    bottom and right to H x W (`crop`: the source size rounded down to multiples of 20; otherwise the source size).  A y4m clip
    (`yuv`: its (layout, matrix, range); `items` the `Y4MReader`) is the exception: `host` returns the frame's planar bytes as they
    are in the file, and `rgb` turns uploaded planar frames into the cropped RGB frames on the device.  `depth`: 8 (uint8 frames), or
    10 / 12 (uint16 frames: `dtype`; the planar bytes of a deep y4m clip are still uint8, two per sample).  `view` is the same clip
    seen through a rectangle (the region of interest: the analysis pass is handed that view), `sample` a subset of its frames.
    `woven` is the same clip read as interlaced frames, two woven fields each (`interlaced`: the `rgb` of a y4m clip then goes through
    the field-aware conversion), and `field(p)` its clip of the fields of parity p, frame rows p::2: a view with a row step of 2."""

    def __init__(self, items, T: int, H: int, W: int, paths: bool, crop: bool = False, yuv=None, depth: int = 8):
        self.items, self.T, self.paths, self.src, self.yuv, self.depth = items, T, paths, (H, W), yuv, depth
        self.dtype = torch.uint8 if depth == 8 else torch.uint16
        self.H, self.W = (H - H % 20, W - W % 20) if crop else (H, W)
        self.y0 = self.x0 = 0            # the origin of the H x W view in the source frames (`view`: a rectangle)
        self.index = None                # the source frame of each of the T frames (`sample`: a subset); None: all, in order
        self.ystep = 1                   # the rows of the view are the source rows y0, y0 + ystep, ... (`field`: 2)
        self.interlaced = False          # the frames are two woven fields each (`woven`, `field`)

    def view(self, rect) -> "Frames":
        """The same clip seen through the rectangle (y0, x0, h, w) of this view: `device`, `host` and `rgb` hand out the cropped
        frames, H and W are the rectangle's.  Nothing is copied."""
        y0, x0, h, w = rect
        assert 0 <= y0 and 0 <= x0 and y0 + h <= self.H and x0 + w <= self.W
        v = copy.copy(self)
        v.y0, v.x0, v.H, v.W = self.y0 + y0, self.x0 + x0, h, w
        return v

    def woven(self) -> "Frames":
        """The same clip with its frames read as two woven fields each (field p: rows p::2).  H and W are still the frame's; what
        changes is `rgb`: the planar frames of a y4m clip go through `ops.yuv_to_rgb_u8(..., fields=True)` (or `_u16`), in which no
        chroma row of one field reaches the other.  Nothing is copied."""
        v = copy.copy(self)
        v.interlaced = True
        return v

    def field(self, p: int) -> "Frames":
        """The clip of the fields of parity p (0 = top, 1 = bottom) of this clip's frames: `device`, `host` and `rgb` hand out the
        rows p::2, H is half the frame's (which must be even).  A strided view: nothing is copied on the host."""
        assert p in (0, 1) and self.ystep == 1 and self.H % 2 == 0
        v = self.woven()
        v.y0, v.ystep, v.H = self.y0 + p, 2, self.H // 2
        return v

    def sample(self, index) -> "Frames":
        """The clip of the frames `index` (indices into this one) of this clip.  Nothing is copied."""
        v = copy.copy(self)
        v.index = [self._at(int(i)) for i in index]
        v.T = len(v.index)
        return v

    def _at(self, i: int) -> int:
        return i if self.index is None else self.index[i]

    def _crop(self, f):
        return f[..., self.y0:self.y0 + self.H * self.ystep:self.ystep, self.x0:self.x0 + self.W, :]

    def upto(self, i: int) -> int:
        """How many of the first i frames exist: min(i, T).  A stream (`StreamFrames`) waits for frame i - 1 or its end."""
        return min(i, self.T)

    def release(self, lo: int) -> None:
        """No frame below `lo` will be asked for again: a stream gives up their buffers."""

    def on_device(self, i: int) -> bool:
        if self.yuv is not None:
            return False
        f = self.items[self._at(i)]
        return torch.is_tensor(f) and f.is_cuda

    def rgb(self, planar: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Planar frames [N, frame_bytes] (uint8: the file's bytes) of a y4m clip on the device -> uint8 [N,H,W,3] there
        (`ops.yuv_to_rgb_u8`), or uint16 for a deep clip (`ops.yuv_to_rgb_u16` on the bytes viewed as words); cropped after the
        conversion, into the contiguous `out` if given.  An interlaced 4:2:0 clip (`woven`, `field`) goes through the field-aware
        conversion; the other layouts convert row by row, so their progressive launch is the field-aware one."""
        fields = self.interlaced and self.yuv[0] in (y4m.CENTER, y4m.LEFT)
        if self.depth == 8:
            def convert(p, h, w, *how, out=None):
                return ops.yuv_to_rgb_u8(p, h, w, *how, out=out, fields=fields)
        else:
            planar = planar.view(torch.uint16)

            def convert(p, h, w, *how, out=None):
                return ops.yuv_to_rgb_u16(p, h, w, *how, self.depth, out=out, fields=fields)
        if (self.H, self.W) == self.src:
            return convert(planar, self.H, self.W, *self.yuv, out=out)
        full = self._crop(convert(planar, *self.src, *self.yuv))
        return full.contiguous() if out is None else out.copy_(full)

    def device(self, i: int) -> torch.Tensor:
        return self._crop(self.items[self._at(i)])

    def host(self, i: int) -> np.ndarray:
        if self.yuv is not None:
            return self.items.raw(self._at(i))
        f = self.items[self._at(i)]
        if self.paths:
            img = imread(f)
            if img.shape[:2] != self.src:
                raise ValueError(f"frame {i} ({f}) is {img.shape[1]}x{img.shape[0]}, the clip is {self.src[1]}x{self.src[0]}")
        else:
            img = f.numpy() if torch.is_tensor(f) else np.asarray(f)
        return self._crop(img)


class FrameRing:
    """A bounded window on a stream of frames: one reader thread calls `fill(slot) -> bool` (False: the stream has ended) for frame
    0, 1, 2, ... in turn, each into slot i % capacity of `capacity` buffers of one shape, page-locked where a GPU is present.  The
    thread blocks while frame `lo + capacity` would overwrite a frame that has not been released; `release(lo)` frees every frame
    below `lo`.  `upto(i)` blocks until frame i - 1 has been read or the stream has ended and returns min(i, frames read);
    `get(i)` is frame i's buffer (a view, valid until the frame is released), and an IndexError for a frame that was released or
    has not been read yet: either is a bug of the caller's.  `T` is None until the stream has ended, then its length.  An error in
    the reader thread (a frame cut short) is raised from `upto`."""

    def __init__(self, fill, shape, dtype, capacity: int):
        import threading
        if capacity < 1:
            raise ValueError(f"a frame ring needs at least one slot, got {capacity}")
        pin = torch.cuda.is_available()
        self.slots = [torch.empty(shape, dtype=dtype, pin_memory=pin).numpy() for _ in range(capacity)]
        self.capacity, self.fill = capacity, fill
        self.lo, self.read, self.T, self.error, self.closed = 0, 0, None, None, False
        self.cv = threading.Condition()
        self.thread = threading.Thread(target=self._work, name="speinet-frame-ring", daemon=True)
        self.thread.start()                          # `fill` must not need this object: it is not its owner's yet

    def _work(self) -> None:
        try:
            while True:
                with self.cv:
                    self.cv.wait_for(lambda: self.closed or self.read < self.lo + self.capacity)
                    if self.closed:
                        return
                    slot = self.slots[self.read % self.capacity]
                more = self.fill(slot)               # blocks on the source, outside the lock
                with self.cv:
                    if more:
                        self.read += 1
                    else:
                        self.T = self.read
                    self.cv.notify_all()
                if not more:
                    return
        except BaseException as e:                   # handed to the consumer: `upto` raises it
            with self.cv:
                self.error, self.T = e, self.read
                self.cv.notify_all()

    def upto(self, i: int) -> int:
        with self.cv:
            if self.T is None and i > self.lo + self.capacity:
                raise IndexError(f"frame {i - 1} cannot be waited for: the ring holds {self.capacity} frames from {self.lo} on")
            self.cv.wait_for(lambda: self.read >= i or self.T is not None)
            if self.error is not None and self.read < i:
                raise self.error
            return min(i, self.read)

    def ready(self, i: int) -> int:
        """min(i, frames read so far), without waiting."""
        with self.cv:
            return min(i, self.read)

    def get(self, i: int) -> np.ndarray:
        with self.cv:
            if not self.lo <= i < self.read:
                raise IndexError(f"frame {i} was released already (the ring starts at {self.lo})" if i < self.lo else
                                 f"frame {i} has not been read yet ({self.read} so far)")
            return self.slots[i % self.capacity]

    def release(self, lo: int) -> None:
        with self.cv:
            if lo > self.lo:
                self.lo = min(lo, self.read)
                self.cv.notify_all()

    def close(self) -> None:
        """Stop the reader thread at its next frame (one blocked on its source ends with the process: it is a daemon)."""
        with self.cv:
            self.closed = True
            self.cv.notify_all()


class StreamFrames(Frames):
    """A clip whose length is not known before its last frame: `Frames` over a `FrameRing`.  `T` is None until the stream has ended.
    `source`: a `y4m.Y4MStream` (`host(i)` is then the frame's planar bytes and `yuv` its (layout, matrix, range), as for a reader),
    or an iterator of uint8 [H,W,3] frames (uint16 with `depth`: arrays or host tensors), whose first frame `frames_of` has taken
    already (`first`).  `host`, `rgb`, `view`, `woven`, `field`, `depth`, `dtype` and `yuv` are `Frames`'; `upto(i)` waits for frame i - 1 (or the
    end), `release(lo)` gives up every frame below `lo`, `ready(i)` does not wait.  `capacity`: the ring's slots; the clip loop sets
    it from its look-ahead (`reserve`) before the first frame is asked for, which is when the reader thread starts."""

    def __init__(self, source, H: int, W: int, crop: bool = False, yuv=None, depth: int = 8, first=None, capacity: int = 64):
        Frames.__init__(self, source, None, H, W, paths=False, crop=crop, yuv=yuv, depth=depth)
        self._shared = {"ring": None, "capacity": capacity, "first": first}

    T = property(lambda self: None if self._shared["ring"] is None else self._shared["ring"].T, lambda self, value: None)

    def reserve(self, capacity: int) -> None:
        if self._shared["ring"] is not None:
            raise RuntimeError("the frame ring is running already")
        self._shared["capacity"] = capacity

    @property
    def ring(self) -> FrameRing:
        sh = self._shared
        if sh["ring"] is None:
            if self.yuv is not None:
                sh["ring"] = FrameRing(self.items.read_into, (self.items.frame_bytes,), torch.uint8, sh["capacity"])
            else:
                sh["ring"] = FrameRing(self._next, (*self.src, 3), self.dtype, sh["capacity"])
        return sh["ring"]

    def _next(self, slot: np.ndarray) -> bool:
        """The iterator's next frame into `slot` (the reader thread)."""
        sh = self._shared
        f, sh["first"] = sh["first"], None
        if f is None:
            f = next(self.items, None)
            if f is None:
                return False
        n = sh["taken"] = sh.get("taken", -1) + 1
        if not isinstance(f, (np.ndarray, torch.Tensor)) or (torch.is_tensor(f) and f.is_cuda):
            raise ValueError(f"frame {n} of the stream is a {type(f).__name__}, not a host array or tensor")
        a = f.numpy() if torch.is_tensor(f) else f
        if a.shape != slot.shape or a.dtype != slot.dtype:
            raise ValueError(f"mixed frames: frame 0 is {self.src[1]}x{self.src[0]} {slot.dtype}, frame {n} has shape {tuple(a.shape)} "
                             f"and is {a.dtype}")
        slot[...] = a
        return True

    def upto(self, i: int) -> int:
        return self.ring.upto(i)

    def ready(self, i: int) -> int:
        return self.ring.ready(i)

    def release(self, lo: int) -> None:
        self.ring.release(lo)

    def close(self) -> None:
        if self._shared["ring"] is not None:
            self._shared["ring"].close()

    def sample(self, index):
        raise ValueError("a stream cannot be sampled: its frames are read once, in order")

    def on_device(self, i: int) -> bool:
        return False

    def device(self, i: int):
        raise ValueError("a stream's frames are on the host")

    def host(self, i: int) -> np.ndarray:
        f = self.ring.get(i)
        return f if self.yuv is not None else self._crop(f)


def _check_frame(i, shape, dtype, depth=None) -> None:
    if dtype in (np.uint16, torch.uint16):
        if depth is None:
            raise ValueError(f"uint16 frames need depth=10 or depth=12 (bits per sample); frame {i} is {dtype}")
    elif depth is not None:
        raise ValueError(f"depth= applies to uint16 frames only; frame {i} is {dtype}")
    elif dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"frames must be uint8, or uint16 with depth=; frame {i} is {dtype}")
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"frames must be 3-channel HWC arrays [H,W,3]; frame {i} has shape {tuple(shape)}")
    if shape[0] < MIN_SIZE or shape[1] < MIN_SIZE:
        raise ValueError(f"frames must be at least {MIN_SIZE}x{MIN_SIZE}; frame {i} is {shape[1]}x{shape[0]}")


def frames_of(frames, crop: bool = False, yuv: Optional[dict] = None, depth: Optional[int] = None) -> Frames:
    """Validate a clip: a uint8 [T,H,W,3] array or tensor (host or device), a list of uint8 [H,W,3] arrays / tensors, a list of
    image paths (only their headers are read here), or a `y4m.Y4MReader` (`yuv`: optional `matrix` / `range` in place of the
    reader's; a reader opened with `depths=(8, 10, 12)` may hold a deep clip).  uint16 arrays, tensors or lists of them are deep
    frames and need `depth` = 10 or 12 (bits per sample; a word above 2^depth - 1 reads as that); `depth` with anything else is an
    error.  A `y4m.Y4MStream`, or an iterator of host frames ([H,W,3] uint8, or uint16 with `depth`), is a clip of unknown length
    and comes back as `StreamFrames` (the iterator's first frame is taken here).  Raises ValueError with the reason."""
    if depth is not None and (isinstance(depth, bool) or depth not in (10, 12)):
        raise ValueError(f"depth must be 10 or 12, got {depth!r}")
    if isinstance(frames, y4m.Y4MReader):
        if depth is not None:
            raise ValueError("depth= applies to uint16 frames only: a y4m clip carries its own")
        if set(yuv or {}) - {"matrix", "range"}:
            raise ValueError(f"yuv holds {sorted(set(yuv) - {'matrix', 'range'})}: it takes matrix and range")
        if len(frames) < 2:
            raise ValueError(f"a clip needs at least 2 frames (its 3-frame windows reflect at the ends); got {len(frames)}")
        _check_frame(0, (frames.height, frames.width, 3), np.uint8)
        how = (frames.layout, y4m.matrix_of((yuv or {}).get("matrix", frames.matrix)), y4m.range_of((yuv or {}).get("range", frames.range)))
        return Frames(frames, len(frames), frames.height, frames.width, paths=False, crop=crop, yuv=how, depth=frames.depth)
    if isinstance(frames, y4m.Y4MStream):              # a stream: its length is not known here (`StreamFrames`)
        if depth is not None:
            raise ValueError("depth= applies to uint16 frames only: a y4m clip carries its own")
        if set(yuv or {}) - {"matrix", "range"}:
            raise ValueError(f"yuv holds {sorted(set(yuv) - {'matrix', 'range'})}: it takes matrix and range")
        _check_frame(0, (frames.height, frames.width, 3), np.uint8)
        how = (frames.layout, y4m.matrix_of((yuv or {}).get("matrix", frames.matrix)), y4m.range_of((yuv or {}).get("range", frames.range)))
        return StreamFrames(frames, frames.height, frames.width, crop=crop, yuv=how, depth=frames.depth)
    if yuv is not None:
        raise ValueError("yuv= applies to y4m clips only")
    if hasattr(frames, "__next__"):                    # an iterator of frames: the first one says what the others must be
        first = next(frames, None)
        if first is None:
            raise ValueError("a clip needs at least 2 frames (its 3-frame windows reflect at the ends); got 0")
        if not isinstance(first, (np.ndarray, torch.Tensor)) or (torch.is_tensor(first) and first.is_cuda):
            raise ValueError(f"frame 0 of the stream is a {type(first).__name__}, not a host array or tensor")
        _check_frame(0, tuple(first.shape), first.dtype, depth)
        return StreamFrames(frames, int(first.shape[0]), int(first.shape[1]), crop=crop, depth=depth or 8, first=first)
    if isinstance(frames, (str, bytes)) or not hasattr(frames, "__len__") or not hasattr(frames, "__getitem__"):
        raise ValueError(f"frames must be an indexable sequence of frames, got {type(frames).__name__}")
    T = len(frames)
    if T < 2:
        raise ValueError(f"a clip needs at least 2 frames (its 3-frame windows reflect at the ends); got {T}")
    if isinstance(frames, (np.ndarray, torch.Tensor)):
        if frames.ndim != 4:
            raise ValueError(f"a frame array must be [T,H,W,3]; got shape {tuple(frames.shape)}")
        _check_frame(0, tuple(frames.shape[1:]), frames.dtype, depth)
        return Frames(frames, T, int(frames.shape[1]), int(frames.shape[2]), paths=False, crop=crop, depth=depth or 8)
    items = list(frames)
    is_path = [isinstance(f, (str, os.PathLike)) for f in items]
    if any(is_path) and not all(is_path):
        raise ValueError("frames mixes image paths and arrays")
    if all(is_path):
        if depth is not None:
            raise ValueError("depth= applies to uint16 frames only: image files are read as 8-bit")
        from PIL import Image
        sizes = []
        for p in items:
            with Image.open(p) as im:           # the header only: decoding happens later, on worker threads
                sizes.append((im.size[1], im.size[0]))
        for i, (h, w) in enumerate(sizes):
            _check_frame(i, (h, w, 3), np.uint8)
            if (h, w) != sizes[0]:
                raise ValueError(f"mixed frame sizes: frame 0 is {sizes[0][1]}x{sizes[0][0]}, frame {i} ({items[i]}) is {w}x{h}")
        return Frames([os.fspath(p) for p in items], T, sizes[0][0], sizes[0][1], paths=True, crop=crop)
    for i, f in enumerate(items):
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            raise ValueError(f"frame {i} is a {type(f).__name__}, not an array, tensor or image path")
        _check_frame(i, tuple(f.shape), f.dtype, depth)
        if tuple(f.shape) != tuple(items[0].shape):
            raise ValueError(f"mixed frame sizes: frame 0 is {items[0].shape[1]}x{items[0].shape[0]}, frame {i} is {f.shape[1]}x{f.shape[0]}")
    return Frames(items, T, int(items[0].shape[0]), int(items[0].shape[1]), paths=False, crop=crop, depth=depth or 8)



# ---- mattes ---------------------------------------------------------------------------------------------------------------------------
MATTE_GROW = 20                          # pixels the matte's bounding box is grown by on every side: the clip API's `shave` default
MATTE_MEMO = 32                          # decoded mattes held on the host at most (more than a window's look-ahead)


def _matte_plane(a, what: str) -> np.ndarray:
    """A host matte as uint8 (a bool matte is 0 / 255); ValueError for any other dtype."""
    if a.dtype == np.bool_:
        return a.astype(np.uint8) * np.uint8(255)
    if a.dtype != np.uint8:
        raise ValueError(f"a matte is uint8 or bool; {what} is {a.dtype}")
    return a


def grow_box(box, H: int, W: int, grow: int = MATTE_GROW, least: int = MIN_SIZE):
    """The rectangle (y0, x0, h, w) of a bounding box (ya, yb, xa, xb) (half open) in an H x W frame: grown by `grow` pixels on every
    side, then symmetrically to at least `least` per axis (an odd pixel goes to the far side), then clamped to the frame; an axis that
    the clamp left shorter than `least` is extended back into the frame from the edge it lies on.  None for None (nothing to box)."""
    if box is None:
        return None

    def axis(a: int, b: int, n: int):
        a, b = a - grow, b + grow
        if b - a < least:
            d = least - (b - a)
            a, b = a - d // 2, b + d - d // 2
        a, b = max(a, 0), min(b, n)
        if b - a < least:
            a, b = (0, min(n, least)) if a == 0 else (max(0, b - least), b)
        return a, b - a

    (y0, h), (x0, w) = axis(box[0], box[1], H), axis(box[2], box[3], W)
    return y0, x0, h, w


class Mattes:
    """The mattes of a clip behind one interface: matte i as a contiguous host uint8 [H,W] array (`host`) or a device tensor
    (`device`, where `on_device`), cropped at the bottom and right as the frames are under `crop`.  `static`: one matte for every
    frame (`T` is then None, and every index reads it).  The bytes are handed out as given; `invert` is applied by whoever reads them
    (`ops.frame_matte(..., invert=)`), and by `empty` and `bbox`, which speak of the matte in effect, 255 - m under `invert`:
    `empty(i)`, is it 0 everywhere; `bbox()`, the rectangle (y0, x0, h, w) around the non-zero samples of every matte, grown and
    clamped by `grow_box`, or None when every matte is empty.  Host mattes are decided on the host (each decoded once while it is in
    the memo; `prefetch` decodes ahead on a thread pool); device mattes with one reduction and one sync, on first use."""

    def __init__(self, items, kind: str, T: Optional[int], H: int, W: int, crop: bool = False, invert: bool = False):
        import threading
        self.items, self.kind, self.T, self.src, self.invert = items, kind, T, (H, W), bool(invert)
        self.static = T is None
        self.H, self.W = (H - H % 20, W - W % 20) if crop else (H, W)
        self._memo: "collections.OrderedDict[int, object]" = collections.OrderedDict()
        self._empty, self._lock = {}, threading.Lock()

    def describe(self) -> str:
        return ("static" if self.static else f"per frame, {self.T} frames") + f", {self.W}x{self.H}" + (", inverted" if self.invert else "")

    def key(self, i: int) -> int:
        """What identifies matte i: 0 for a static matte."""
        if self.static:
            return 0
        if not 0 <= i < self.T:
            raise IndexError(f"matte {i} of {self.T}")
        return i

    def _item(self, k: int):
        return self.items if self.static and self.kind != "paths" else self.items[k]

    def on_device(self, i: int) -> bool:
        return self.kind == "device" or (self.kind == "list" and torch.is_tensor(self._item(self.key(i))) and self._item(self.key(i)).is_cuda)

    def device(self, i: int) -> torch.Tensor:
        m = self._item(self.key(i))[:self.H, :self.W]
        return (m.to(torch.uint8) * 255 if m.dtype == torch.bool else m).contiguous()

    def _load(self, k: int) -> np.ndarray:
        if self.kind == "y4m":
            a = self.items.raw(k).reshape(self.src)
        elif self.kind == "paths":
            from PIL import Image
            with Image.open(self.items[k]) as im:
                a = np.asarray(im.convert("L"))
            if a.shape != self.src:
                raise ValueError(f"matte {k} ({self.items[k]}) is {a.shape[1]}x{a.shape[0]}, the frames are {self.src[1]}x{self.src[0]}")
        else:
            m = self._item(k)
            a = _matte_plane(m.numpy() if torch.is_tensor(m) else np.asarray(m), f"matte {k}")
        return np.ascontiguousarray(a[:self.H, :self.W])

    def prefetch(self, pool: ThreadPoolExecutor, indices) -> None:
        """Decode the host mattes `indices` on the pool, for the `host` and `empty` calls to come."""
        with self._lock:
            for i in indices:
                k = self.key(i)
                if k not in self._memo and not self.on_device(i):
                    self._memo[k] = pool.submit(self._load, k)
            while len(self._memo) > MATTE_MEMO:
                self._memo.popitem(last=False)

    def host(self, i: int) -> np.ndarray:
        k = self.key(i)
        with self._lock:
            a = self._memo.get(k)
        if a is None:                                      # not asked for ahead (or given up since): decoded by the caller
            a = self._load(k)
            with self._lock:
                self._memo[k] = a
                while len(self._memo) > MATTE_MEMO:
                    self._memo.popitem(last=False)
        return a.result() if isinstance(a, Future) else a

    def _device_stack(self) -> Optional[torch.Tensor]:
        return self.items[None] if self.static else self.items

    def empty(self, i: int) -> bool:
        k = self.key(i)
        if k not in self._empty:
            blank = 255 if self.invert else 0
            if self.kind == "device":                      # one reduction over every matte, one sync
                lit = (self._device_stack()[:, :self.H, :self.W] != (self.invert if self.items.dtype == torch.bool else blank))
                for j, v in enumerate(lit.flatten(1).any(1).cpu().tolist()):
                    self._empty[j] = not v
            elif self.on_device(i):
                self._empty[k] = not bool((self.device(i) != blank).any().item())
            else:
                self._empty[k] = not bool((self.host(i) != blank).any())
        return self._empty[k]

    def bbox(self, grow: int = MATTE_GROW):
        """One pass over every matte (a static one: over it); host mattes on the host, device mattes with two reductions and one sync."""
        blank = 255 if self.invert else 0
        n = 1 if self.static else self.T
        if self.kind == "device":
            lit = (self._device_stack()[:, :self.H, :self.W] != (self.invert if self.items.dtype == torch.bool else blank)).any(0)
            rows, cols = lit.any(1).cpu().numpy(), lit.any(0).cpu().numpy()
        else:
            rows, cols = np.zeros(self.H, bool), np.zeros(self.W, bool)
            for i in range(n):
                lit = (self.device(i).cpu().numpy() if self.on_device(i) else self.host(i)) != blank
                rows |= lit.any(1)
                cols |= lit.any(0)
        ys, xs = np.flatnonzero(rows), np.flatnonzero(cols)
        if not ys.size:
            return None
        return grow_box((int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1), self.H, self.W, grow)


def _matte_shape(i, shape, dtype, H: int, W: int) -> None:
    if dtype not in (np.uint8, np.bool_, torch.uint8, torch.bool):
        raise ValueError(f"a matte is uint8 or bool; {'the matte' if i is None else f'matte {i}'} is {dtype}")
    if tuple(shape) != (H, W):
        raise ValueError(f"{'the matte' if i is None else f'matte {i}'} has shape {tuple(shape)}, the frames are {W}x{H}: a matte is [H,W] = "
                         f"[{H},{W}], one byte per pixel")


def mattes_of(matte, T: Optional[int], H: int, W: int, crop: bool = False, invert: bool = False) -> Mattes:
    """Validate the mattes of a clip of T frames of H x W (T None: a stream, its length is not known; `crop`: the frames are cropped to
    multiples of 20 as they are loaded, and so is the matte) and return them as `Mattes`.  Static: a uint8 or bool [H,W] numpy array or
    torch tensor (host or device), or the path of an image file (decoded to one 8-bit channel, PIL `convert("L")`).  Per frame: a
    [T,H,W] array or tensor, a list of [H,W] arrays / tensors or of image paths (only their headers are read here), a directory of
    images (in file-name order), or an 8-bit `Cmono` y4m clip (a path ending in .y4m, or a `y4m.Y4MReader` opened with
    `layouts=y4m.LAYOUTS`), whose luma bytes are the matte as stored: m = 255 needs full-range grey.  Raises ValueError naming what is
    wrong: a size, a dtype, a length other than T, a y4m clip that is not `Cmono`."""
    def length(n: int, what: str) -> None:
        if T is not None and n != T:
            raise ValueError(f"{what} holds {n} mattes for a clip of {T} frames: a per-frame matte has one per frame")

    if isinstance(matte, (str, os.PathLike)):
        path = os.fspath(matte)
        if path.lower().endswith(".y4m"):
            matte = y4m.Y4MReader(path, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS, interlace=y4m.INTERLACE)
        elif os.path.isdir(path):
            matte = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(IMAGE_EXTS))
            if not matte:
                raise ValueError(f"the matte directory {path} holds no image file ({', '.join(IMAGE_EXTS)})")
        else:
            from PIL import Image
            with Image.open(path) as im:
                if (im.size[1], im.size[0]) != (H, W):
                    raise ValueError(f"the matte {path} is {im.size[0]}x{im.size[1]}, the frames are {W}x{H}")
            return Mattes([path], "paths", None, H, W, crop, invert)
    if isinstance(matte, y4m.Y4MReader):
        if matte.layout != y4m.MONO or matte.depth != 8:
            raise ValueError(f"a y4m matte is an 8-bit Cmono clip (its luma bytes are the matte); {matte.name} is C{matte.chroma}")
        _matte_shape(None, (matte.height, matte.width), np.uint8, H, W)
        length(len(matte), f"the y4m matte {matte.name}")
        return Mattes(matte, "y4m", len(matte), H, W, crop, invert)
    if isinstance(matte, (np.ndarray, torch.Tensor)):
        device = torch.is_tensor(matte) and matte.is_cuda
        if matte.ndim == 2:
            _matte_shape(None, matte.shape, matte.dtype, H, W)
            return Mattes(matte, "device" if device else "array", None, H, W, crop, invert)
        if matte.ndim != 3:
            raise ValueError(f"a matte array is [H,W] (static) or [T,H,W] (per frame); got shape {tuple(matte.shape)}")
        _matte_shape(None, matte.shape[1:], matte.dtype, H, W)
        length(int(matte.shape[0]), "the matte array")
        return Mattes(matte, "device" if device else "array", int(matte.shape[0]), H, W, crop, invert)
    if isinstance(matte, (bytes, bytearray)) or not hasattr(matte, "__len__") or not hasattr(matte, "__getitem__"):
        raise ValueError(f"matte must be an [H,W] or [T,H,W] array or tensor, an image path, a list of either, a directory or a Cmono y4m "
                         f"clip, got {type(matte).__name__} (an iterator of mattes is not built)")
    items = list(matte)
    length(len(items), "the matte list")
    if not items:
        raise ValueError("the matte list is empty")
    is_path = [isinstance(m, (str, os.PathLike)) for m in items]
    if any(is_path) and not all(is_path):
        raise ValueError("matte mixes image paths and arrays")
    if all(is_path):
        from PIL import Image
        for i, p in enumerate(items):
            with Image.open(p) as im:                      # the header only: decoding happens later, on worker threads
                if (im.size[1], im.size[0]) != (H, W):
                    raise ValueError(f"matte {i} ({os.fspath(p)}) is {im.size[0]}x{im.size[1]}, the frames are {W}x{H}")
        return Mattes([os.fspath(p) for p in items], "paths", len(items), H, W, crop, invert)
    for i, m in enumerate(items):
        if not isinstance(m, (np.ndarray, torch.Tensor)):
            raise ValueError(f"matte {i} is a {type(m).__name__}, not an array, tensor or image path")
        _matte_shape(i, m.shape, m.dtype, H, W)
    return Mattes(items, "list", len(items), H, W, crop, invert)
