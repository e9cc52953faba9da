"""YUV4MPEG2 ("y4m") streams: decoded video as `ffmpeg -f yuv4mpegpipe` writes and reads it, a text header line and then one
`FRAME` line plus raw planar bytes per frame.  Host side only (numpy, no torch): the planar bytes go to the device as they are and
become packed RGB there (csrc/yuv_io.hip, `ops.yuv_to_rgb_u8`), and come back the same way (`ops.rgb_u8_to_yuv`).

Supported: progressive 8-bit 4:2:0 (`C420jpeg`, bare `C420`, `C420mpeg2`) and 4:4:4 (`C444`), and, for a reader opened with
`depths=(8, 10, 12)`, 10- and 12-bit 4:2:0 and 4:4:4 (`C420p10`, `C420p12`, `C444p10`, `C444p12`: little-endian 16-bit samples, which
`ops.yuv_to_rgb_u16` / `ops.rgb_u16_to_yuv` convert).  For a reader opened with `layouts=LAYOUTS`, also 4:2:2 (`C422`, `C422p10`,
`C422p12`: chroma planes [H][ceil(W/2)], co-sited with the even column) and mono (`Cmono`, `Cmono10`, `Cmono12`: the Y plane alone) at
the depths it was given; the same four `ops` functions convert them.  `Y4MReader` indexes a file; `Y4MStream` reads a pipe in order, with the same header
parsing and error texts.

Interlaced streams (`It`: top field first, `Ib`: bottom field first) are an opt-in as well: a reader opened with
`interlace=("p", "t", "b")` accepts them and says which it met in `.interlace`; a record is then a WOVEN frame of `frame_bytes` bytes
whose rows p::2 are field p, and for 4:2:0 chroma-plane row j belongs to field j & 1 (`ops.yuv_to_rgb_u8(..., fields=True)`; the clip
API's `fields="split"`).  `Y4MWriter(..., interlace="t")` writes the tag.  The two tags differ in nothing but the tag.

Not supported: mixed-mode streams (`Im`), interlaced streams without the opt-in, other depths (9, 14, 16 bits), 4:1:1, 4:4:0,
`C420paldv`."""
from __future__ import annotations

import os
import re
import threading

import numpy as np

CENTER, LEFT, P444 = 0, 1, 2           # SPEI_YUV_420_CENTER, SPEI_YUV_420_LEFT, SPEI_YUV_444 (include/speinet_hip.h)
P422, MONO = 3, 4                      # SPEI_YUV_422, SPEI_YUV_MONO
LAYOUTS = (CENTER, LEFT, P444, P422, MONO)
BT601, BT709 = 0, 1                    # SPEI_YUV_BT601, SPEI_YUV_BT709
FULL, LIMITED = 0, 1                   # SPEI_YUV_FULL, SPEI_YUV_LIMITED

MAGIC = b"YUV4MPEG2"
# a reader takes a tag only if its layout is among the reader's `layouts` (P422 and MONO are an opt-in)
LAYOUT_OF_TAG = {"420jpeg": CENTER, "420": CENTER, "420mpeg2": LEFT, "444": P444, "422": P422, "mono": MONO}
DEEP_TAGS = {"420p10": (LEFT, 10), "420p12": (LEFT, 12), "444p10": (P444, 10), "444p12": (P444, 12),     # tag -> (layout, depth)
             "422p10": (P422, 10), "422p12": (P422, 12), "mono10": (MONO, 10), "mono12": (MONO, 12)}
DEPTHS = (8, 10, 12)
TAG_OF_LAYOUT = {CENTER: "420jpeg", LEFT: "420mpeg2", P444: "444", P422: "422", MONO: "mono"}
MATRIX_NAMES = {"bt601": BT601, "bt709": BT709}
RANGE_NAMES = {"full": FULL, "limited": LIMITED}
HINT = "convert it with `ffmpeg -i <in> -pix_fmt yuv420p -f yuv4mpegpipe <out.y4m>`"
MAX_HEADER = 4096
INTERLACE = ("p", "t", "b")            # the I tags a reader can take: progressive, top field first, bottom field first ("p" always)


def _named(value, names: dict, what: str) -> int:
    if isinstance(value, str) and value.lower() in names:
        return names[value.lower()]
    if not isinstance(value, (str, bool)) and value in names.values():
        return int(value)
    raise ValueError(f"{what} must be one of {sorted(names)}, got {value!r}")


def matrix_of(value) -> int:
    """BT601 / BT709 from the constant or from "bt601" / "bt709"."""
    return _named(value, MATRIX_NAMES, "matrix")


def range_of(value) -> int:
    """FULL / LIMITED from the constant or from "full" / "limited"."""
    return _named(value, RANGE_NAMES, "range")


def layout_of(value) -> int:
    """CENTER / LEFT / P444 / P422 / MONO from the constant or from a y4m chroma tag ("420jpeg", "420", "420mpeg2", "444", "422",
    "mono")."""
    return _named(value, LAYOUT_OF_TAG, "chroma layout")


def depth_of(depth) -> int:
    """8, 10 or 12 bits per sample."""
    if isinstance(depth, bool) or depth not in DEPTHS:
        raise ValueError(f"depth must be one of {DEPTHS}, got {depth!r}")
    return int(depth)


def interlace_of(interlace) -> tuple:
    """The I tags a reader takes, from a sequence of "p", "t", "b": "p" is always among them."""
    tags = (interlace,) if isinstance(interlace, str) else tuple(interlace)
    if any(not isinstance(t, str) or t not in INTERLACE for t in tags):
        raise ValueError(f"interlace must hold \"p\", \"t\" or \"b\", got {interlace!r}")
    return tuple(t for t in INTERLACE if t == "p" or t in tags)


def frame_bytes(h: int, w: int, layout: int, depth: int = 8) -> int:
    """Bytes of one planar frame: Y [h][w], then U and V, [ceil(h/2)][ceil(w/2)] each for 4:2:0, [h][ceil(w/2)] each for 4:2:2 and
    [h][w] each for 4:4:4 (mono: the Y plane alone); one byte per sample at `depth` 8, two (a little-endian word) at 10 and 12."""
    if layout not in TAG_OF_LAYOUT:
        raise ValueError(f"unknown chroma layout {layout!r}")
    chroma = {P444: h * w, P422: h * ((w + 1) // 2), MONO: 0}.get(layout, ((h + 1) // 2) * ((w + 1) // 2))
    samples = h * w + 2 * chroma
    return samples * (1 if depth_of(depth) == 8 else 2)


def chroma_tag(layout: int, depth: int = 8) -> str:
    """The C tag's text of a layout at a depth: "420jpeg", "420mpeg2", "444", "422", "mono"; "420p10", "444p12", "422p10", "mono12"
    and the like for deep streams (which carry no siting)."""
    if depth_of(depth) == 8:
        return TAG_OF_LAYOUT[layout]
    return {P444: "444p", P422: "422p", MONO: "mono"}.get(layout, "420p") + str(depth)


def _ratio(tag: str, text: str):
    try:
        a, b = text.split(":")
        return int(a), int(b)
    except ValueError:
        raise ValueError(f"y4m header: tag {tag}{text} is not <int>:<int>") from None


class _Header:
    """What `Y4MReader` and `Y4MStream` share: the header line's tags, their validation and the error texts."""

    def _open(self, path_or_file, depths, layouts, interlace=("p",), mode: str = "rb") -> None:
        self.depths = tuple(depth_of(d) for d in depths)
        self.layouts = tuple(layout_of(v) for v in layouts)
        self.interlaces = interlace_of(interlace)
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike))
        self._f = open(path_or_file, mode) if self._own else path_or_file
        self.name = os.fspath(path_or_file) if self._own else getattr(path_or_file, "name", "<file>")

    def _fail(self, text: str):
        raise ValueError(f"{self.name}: {text}; {HINT}")

    def _header(self, head: bytes) -> int:
        """Parse the header line at the start of `head` into the attributes; returns the offset of its newline."""
        end = head.find(b"\n")
        if not head.startswith(MAGIC) or end < 0:
            raise ValueError(f"{self.name}: not a YUV4MPEG2 stream (no '{MAGIC.decode()} ...' header line)")
        tags = head[len(MAGIC):end].decode("ascii", "replace").split()
        self.width = self.height = None
        self.fps, self.aspect, self.chroma, self.range, self.interlace = (25, 1), None, "420jpeg", LIMITED, "p"
        for t in tags:
            key, val = t[0], t[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                self.fps = _ratio(key, val)
            elif key == "A":
                self.aspect = _ratio(key, val)
            elif key == "I":
                if val == "m":
                    self._fail("tag Im: mixed-mode streams (every frame with an interlacing flag of its own) are not supported")
                if val in ("t", "b") and val in self.interlaces:
                    self.interlace = val
                elif val not in ("p", "?"):
                    self._fail(f"tag I{val}: interlaced streams are not supported (progressive Ip only)")
            elif key == "C":
                self.chroma = val
            elif key == "X" and val.upper().startswith("COLORRANGE="):
                name = val.split("=", 1)[1].lower()
                if name not in RANGE_NAMES:
                    self._fail(f"tag X{val}: the colour range must be FULL or LIMITED")
                self.range = RANGE_NAMES[name]
        for key, val in (("W", self.width), ("H", self.height)):
            if val is None:
                self._fail(f"the header has no {key} tag")
            if val < 1:
                self._fail(f"tag {key}{val}: the size must be positive")
        c = self.chroma
        # the tags of the layouts this reader takes: a tag of another layout is as unknown to it as C411
        flat = {t: lay for t, lay in LAYOUT_OF_TAG.items() if lay in self.layouts}
        deep_tags = {t: v for t, v in DEEP_TAGS.items() if v[0] in self.layouts}
        if c in deep_tags and deep_tags[c][1] in self.depths:
            self.layout, self.depth = deep_tags[c]
        elif c in flat and 8 in self.depths:
            self.layout, self.depth = flat[c], 8
        else:
            deep = re.fullmatch(r"(?:(?:420|422|444)p|mono)(\d+)", c)
            wide = P422 in self.layouts or MONO in self.layouts
            if c in flat:
                why = f"8 bits per sample ({', '.join(map(str, self.depths))} only)"
            elif deep and self.depths != (8,) and int(deep.group(1)) in self.depths:     # C422p10, Cmono12: not the depth's fault
                why = "only 4:2:0 and 4:4:4 are supported"
            elif deep:
                why = f"{deep.group(1)} bits per sample ({', '.join(map(str, self.depths))} only)"
            elif c.startswith(("422", "411", "mono")) or c == "420paldv":
                why = ("only 4:2:0 (C420jpeg, C420, C420mpeg2), 4:2:2 (C422), 4:4:4 (C444) and mono (Cmono) are supported" if wide else
                       "only 4:2:0 (C420jpeg, C420, C420mpeg2) and 4:4:4 (C444) are supported")
            else:
                why = "unknown chroma format"
            self._fail(f"tag C{c}: {why}")
        self.matrix = BT709 if self.height >= 720 else BT601
        self.frame_bytes = frame_bytes(self.height, self.width, self.layout, self.depth)
        return end

    @staticmethod
    def _is_frame_line(line: bytes) -> bool:
        return line[:5] == b"FRAME" and line[5:6] in (b" ", b"\n") and line.find(b"\n") == len(line) - 1

    def _bad_line(self, i: int, n: int, first: bytes):
        raise ValueError(f"{self.name}: frame {i} does not start with a FRAME line of {n} bytes like the first frame's "
                         f"({bytes(first)!r}): FRAME lines of different lengths are not supported")

    def close(self) -> None:
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

class Y4MReader(_Header):
    """A y4m file as an indexable sequence of frames: `len(r)`, and `r.raw(i)` = the `frame_bytes` planar bytes of frame i as a uint8
    numpy array, read at its offset with `readinto` (callable from several threads).  `path_or_file`: a path, or a seekable binary
    file object (a pipe has no length: the command line spools it to a file first).

    Only the header line and the first `FRAME` line are scanned.  `FRAME` lines may carry parameters, but every one must be as long
    as the first: T is then the payload size divided by the record size, and a later line that differs raises ValueError when its
    frame is read.  A file that ends inside a frame raises ValueError here.

    `depths`: the sample depths the caller can take.  The default, (8,), refuses deep streams, as every caller that indexes the
    payload as bytes needs; with (8, 10, 12) the reader also accepts `C420p10`, `C420p12`, `C444p10` and `C444p12`.  `raw(i)` still
    returns the payload's bytes as uint8 (`frame_bytes` of them, two per sample, little-endian).  A deep 4:2:0 tag carries no
    siting: `layout` is then LEFT, the MPEG-2 siting of the codecs such streams come from; it is a plain attribute that the caller
    may set to CENTER before the clip is used.

    `layouts`: the chroma layouts the caller can take, an opt-in like `depths`.  The default, (CENTER, LEFT, P444), refuses `C422*`
    and `Cmono*`, whatever `depths` says; with `layouts=LAYOUTS` the reader also accepts `C422` and `Cmono` and, at the depths it
    was given, `C422p10`, `C422p12`, `Cmono10` and `Cmono12` (`layout` is then P422 or MONO).

    `interlace`: the I tags the caller can take, the third opt-in.  The default, ("p",), refuses `It` and `Ib`; with
    `interlace=INTERLACE` (("p", "t", "b")) the reader accepts them and `interlace` is then "t" or "b" ("p" for `Ip`, `I?` and a
    missing tag).  `frame_bytes` and `raw(i)` are unchanged: an interlaced record is a woven frame, rows p::2 its field p.  `Im`
    (mixed mode) is refused either way.

    Attributes: `width`, `height`, `fps` and `aspect` ((num, den); 25:1 and None when absent), `layout` (CENTER / LEFT / P444; P422 /
    MONO for a reader that takes them),
    `depth` (8, 10 or 12), `chroma` (the C tag's text), `range` (from XCOLORRANGE=FULL|LIMITED; LIMITED when absent), `matrix`, `frame_bytes`.  y4m carries
    no matrix tag: `matrix` is BT709 when height >= 720 and BT601 otherwise, which is ffmpeg's usual guess for untagged video;
    assign `matrix` / `range`, or pass `yuv=dict(matrix=..., range=...)` to `deblur_clip`, to override.

    Interlaced streams without the opt-in, depths outside `depths` (9, 14 and 16 bits always), layouts outside `layouts` (C422 and Cmono at any depth
    by default), C420paldv, C411 and C440 are rejected with a ValueError that names the tag."""

    def __init__(self, path_or_file, depths=(8,), layouts=(CENTER, LEFT, P444), interlace=("p",)):
        self._open(path_or_file, depths, layouts, interlace)
        self._lock = threading.Lock()
        try:
            self._parse()
        except Exception:
            self.close()
            raise

    def _parse(self) -> None:
        f = self._f
        f.seek(0)
        end = self._header(f.read(MAX_HEADER))
        c = self.chroma
        self._data = end + 1
        size = f.seek(0, os.SEEK_END)
        if size == self._data:
            self._line, self._T = b"FRAME\n", 0
            return
        f.seek(self._data)
        first = f.read(MAX_HEADER)
        end = first.find(b"\n")
        self._line = first[:end + 1]
        if end < 0 or not self._is_frame_line(self._line):
            raise ValueError(f"{self.name}: no FRAME line after the header")
        record = len(self._line) + self.frame_bytes
        self._T, rest = divmod(size - self._data, record)
        if rest:
            raise ValueError(f"{self.name}: truncated: {size - self._data} bytes after the header are {self._T} frames of "
                             f"{record} bytes ({len(self._line)} of FRAME line, {self.frame_bytes} of {self.width}x{self.height} "
                             f"C{c}) and {rest} bytes more (a cut last frame, or FRAME lines of different lengths)")

    def __len__(self) -> int:
        return self._T

    def raw(self, i: int) -> np.ndarray:
        """The planar bytes of frame i: a fresh uint8 array of `frame_bytes`."""
        if not 0 <= i < self._T:
            raise IndexError(f"frame {i} of a y4m clip of {self._T} frames")
        n = len(self._line)
        line, buf = bytearray(n), np.empty(self.frame_bytes, dtype=np.uint8)
        with self._lock:
            self._f.seek(self._data + i * (n + self.frame_bytes))
            got = self._f.readinto(line), self._f.readinto(memoryview(buf))
        if got != (n, self.frame_bytes):
            raise ValueError(f"{self.name}: frame {i} is cut short")
        if not self._is_frame_line(bytes(line)):
            self._bad_line(i, n, self._line)
        return buf

    def __getitem__(self, i: int) -> np.ndarray:
        return self.raw(i + self._T if isinstance(i, int) and i < 0 else i)


class Y4MStream(_Header):
    """A y4m stream read in order from a binary file object that need not seek (a pipe, a socket's file, stdin), or from a path: what
    `Y4MReader` is for a file, without a length.  The header line is read here, with `Y4MReader`'s tags, `depths=` / `layouts=` / `interlace=`
    opt-ins, attributes and error texts (the two share the code); then `read_into(buf)` fills `buf` (`frame_bytes` bytes: a uint8
    numpy array or any writable buffer) with the next frame's planar bytes and returns True, or returns False at a clean end of the
    stream (the end in front of a FRAME line).  Short reads are put together.  ValueError: a stream that ends inside a FRAME line or
    a frame, or a FRAME line that is not one of the first frame's length.  `frames` counts the frames read so far.  One reader at
    a time: the object keeps the bytes it read past a line."""

    def __init__(self, path_or_file, depths=(8,), layouts=(CENTER, LEFT, P444), interlace=("p",)):
        self._open(path_or_file, depths, layouts, interlace)
        self._rest, self._line, self.frames = b"", None, 0
        try:
            head = b""
            while b"\n" not in head and len(head) < MAX_HEADER:
                more = getattr(self._f, "read1", self._f.read)(MAX_HEADER - len(head))       # what the pipe holds, not all 4096
                if not more:
                    break
                head += more
            end = self._header(head)
            self._rest = head[end + 1:]
        except Exception:
            self.close()
            raise

    def _fill(self, view: memoryview) -> int:
        """Fill `view` from the bytes kept and then the file; returns the bytes got (fewer than asked: the stream has ended)."""
        got = min(len(self._rest), len(view))
        if got:
            view[:got] = self._rest[:got]
            self._rest = self._rest[got:]
        while got < len(view):
            n = self._f.readinto(view[got:])
            if not n:
                break
            got += n
        return got

    def _frame_line(self) -> bool:
        i = self.frames
        if self._line is None:               # the first frame's line: up to its newline, byte by byte from what a pipe holds
            line = bytearray()
            while not line.endswith(b"\n") and len(line) < MAX_HEADER:
                one = bytearray(1)
                if not self._fill(memoryview(one)):
                    break
                line += one
            if not line:
                return False
            if not self._is_frame_line(bytes(line)):
                raise ValueError(f"{self.name}: no FRAME line after the header")
            self._line = bytes(line)
            return True
        n = len(self._line)
        line = bytearray(n)
        got = self._fill(memoryview(line))
        if got == 0:
            return False
        if got != n:
            raise ValueError(f"{self.name}: frame {i} is cut short")
        if not self._is_frame_line(bytes(line)):
            self._bad_line(i, n, self._line)
        return True

    def read_into(self, buf) -> bool:
        view = memoryview(buf).cast("B")
        if view.nbytes != self.frame_bytes:
            raise ValueError(f"y4m: a {self.width}x{self.height} C{self.chroma} frame is {self.frame_bytes} bytes, the buffer holds {view.nbytes}")
        if not self._frame_line():
            return False
        if self._fill(view) != self.frame_bytes:
            raise ValueError(f"{self.name}: frame {self.frames} is cut short")
        self.frames += 1
        return True


class Y4MWriter:
    """Write a y4m stream, progressive unless `interlace` is "t" or "b" (the header then says `It` / `Ib`, top / bottom field first; a
    frame is a woven frame of the same `frame_bytes`): the header once, then `write(planar bytes)` per frame (`frame_bytes` bytes: a bytes-like
    object or a contiguous numpy array, uint8, or uint16 for a deep stream).  `path_or_file`: a path, or a binary file object (a pipe
    will do), which `close` flushes and leaves open.  `depth` 10 or 12 writes `C420p10`, `C444p12`, `C422p10`, `Cmono12` and the like
    (little-endian words; the tag carries no siting, whatever `layout` says) and adds `XYSCSS=420P10`, `XYSCSS=422P12` and the like,
    as ffmpeg does (none for mono).  `layout` P422 / MONO writes `C422` / `Cmono` frames: Y, then U and V of [h][ceil(w/2)]; Y alone."""

    def __init__(self, path_or_file, w: int, h: int, fps=(25, 1), layout: int = CENTER, range: int = LIMITED, aspect=None,
                 depth: int = 8, interlace: str = "p"):
        if not isinstance(interlace, str) or interlace not in INTERLACE:
            raise ValueError(f"y4m: interlace must be \"p\", \"t\" or \"b\", got {interlace!r}")
        self.interlace = interlace
        self.width, self.height, self.fps, self.aspect = int(w), int(h), (int(fps[0]), int(fps[1])), aspect
        self.layout, self.range, self.depth = layout_of(layout), range_of(range), depth_of(depth)
        self.chroma = chroma_tag(self.layout, self.depth)
        self.frame_bytes = frame_bytes(self.height, self.width, self.layout, self.depth)
        if self.width < 1 or self.height < 1 or self.fps[0] < 1 or self.fps[1] < 1:
            raise ValueError(f"y4m: bad size {w}x{h} or frame rate {fps}")
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike))
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        tags = [f"W{self.width}", f"H{self.height}", f"F{self.fps[0]}:{self.fps[1]}", "I" + interlace]
        if aspect is not None:
            tags.append(f"A{int(aspect[0])}:{int(aspect[1])}")
        tags += [f"C{self.chroma}"] + ([] if self.depth == 8 or self.layout == MONO else [f"XYSCSS={self.chroma.upper()}"])
        tags += ["XCOLORRANGE=" + ("FULL" if self.range == FULL else "LIMITED")]
        self._f.write(MAGIC + b" " + " ".join(tags).encode("ascii") + b"\n")
        self.frames = 0

    def write(self, planar) -> None:
        data = memoryview(planar).cast("B")
        if data.nbytes != self.frame_bytes:
            raise ValueError(f"y4m: a {self.width}x{self.height} C{self.chroma} frame is {self.frame_bytes} bytes, "
                             f"got {data.nbytes}")
        self._f.write(b"FRAME\n")
        self._f.write(data)
        self.frames += 1

    def close(self) -> None:
        if self._own:
            self._f.close()
        else:
            self._f.flush()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
