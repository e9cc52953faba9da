"""The light a run of sharp frames is averaged in (blurset.py, data.SharpTrainLoader; csrc/light.h).

The reference's data-set scripts average code values: the gamma-encoded bytes.  That is the light `code`, the default, and it selects
the kernels that sum bytes.  A sensor integrates LIGHT and applies its transfer curve afterwards, so an exposure over a black / white
edge is far brighter than mid-gray; the GoPro set's `blur_gamma` variant is made that way, through an inverse gamma 2.2 curve (Nah et
al., CVPR 2017).  A light other than `code` does the same in integer arithmetic, defined bit for bit:

    spec      "code" | "srgb" | "gamma:<g>"
    f         the forward transfer, code value in [0, 1] -> linear light in [0, 1]:
              srgb      IEC 61966-2-1: c / 12.92 for c <= 0.04045, else ((c + 0.055) / 1.055) ** 2.4
              gamma:g   c ** g
    S         2 ** 24 - 1
    lin[c]    rint(S * f(c / 255)), c = 0..255              the linear value of code c
    thr[c]    rint(S * f((c - 0.5) / 255)), c = 1..255      the linear value of the boundary between codes c - 1 and c; thr[0] = 0

both tables built here, once, in float64.  Per byte position of a run of n frames (1..15):

    L    = floor(sum of lin[byte] over the run / n)
    blur = #{c in 1..255 : thr[c] <= L}                      the largest code whose lower boundary is at or below L

A pair of tables is VALID iff lin[0] == 0, lin[255] <= S and lin[c - 1] < thr[c] <= lin[c] for c = 1..255.  Then both increase
strictly and encode(lin[c]) == c: a run of length 1, or of identical frames, returns its bytes, which the ground-truth records rely
on.  No range of gamma is written down anywhere: the tables are validated (`gamma:2.8` fails, its thr[1] rounds to 0), here and again
by the C entry points on the host copy they are handed.

`srgb` and `gamma:2.2` are the conventional approximations of a camera curve that is not known; no model has been trained here on
either.
"""
from __future__ import annotations

import math
import threading
from typing import Optional, Tuple

import numpy as np

S = 2 ** 24 - 1
CODE = "code"

_cache = {}
_cache_lock = threading.Lock()


def parse(spec) -> Tuple[str, Optional[float]]:
    """`spec` -> ("code", None), ("srgb", None) or ("gamma", g); None is "code".  Anything else raises ValueError.  Whether a gamma
    makes usable tables is `tables`' question, not asked here."""
    if spec is None or spec == CODE:
        return CODE, None
    if spec == "srgb":
        return "srgb", None
    if isinstance(spec, str) and spec.startswith("gamma:"):
        try:
            g = float(spec[len("gamma:"):])
        except ValueError:
            g = math.nan
        if math.isfinite(g):
            return "gamma", g
    raise ValueError(f"light {spec!r}: expected 'code', 'srgb' or 'gamma:<number>'")


def name(spec) -> str:
    """The canonical spelling of a spec: "code", "srgb" or "gamma:<repr of the float>"."""
    kind, g = parse(spec)
    return kind if g is None else f"gamma:{g!r}"


def is_code(spec) -> bool:
    return parse(spec)[0] == CODE


def first_invalid(lin, thr) -> Optional[int]:
    """The first code at which the pair fails the validity conditions (0 for lin[0] != 0, 255 for lin[255] > S), or None."""
    lin, thr = np.asarray(lin).astype(np.int64).reshape(-1), np.asarray(thr).astype(np.int64).reshape(-1)
    if lin.size != 256 or thr.size != 256:
        raise ValueError(f"light tables hold 256 words each; got {lin.size} and {thr.size}")
    if lin[0] != 0:
        return 0
    bad = np.flatnonzero(~((lin[:-1] < thr[1:]) & (thr[1:] <= lin[1:])))
    if bad.size:
        return int(bad[0]) + 1
    return 255 if lin[255] > S else None


def check(lin, thr) -> bool:
    """Is (lin, thr) a valid pair?"""
    return first_invalid(lin, thr) is None


def tables(spec) -> Tuple[np.ndarray, np.ndarray]:
    """(lin, thr) of a light as uint32 [256] each; ValueError for `code` (no light at all) and for a pair that is not valid."""
    kind, g = parse(spec)
    if kind == CODE:
        raise ValueError("light 'code' averages code values: it has no tables")
    c = np.arange(256, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "srgb":
            def f(v):
                return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
        else:
            def f(v):
                return v ** g
        lin = np.rint(S * f(c / 255.0))
        thr = np.rint(S * f(np.maximum(c - 0.5, 0.0) / 255.0))
    thr[0] = 0.0
    both = np.concatenate([lin, thr])
    if not np.all(np.isfinite(both)) or both.min() < 0 or both.max() >= 2.0 ** 32:
        code = int(np.flatnonzero(~((both >= 0) & (both < 2.0 ** 32)))[0]) % 256
        raise ValueError(f"light {name(spec)}: the tables are not valid at code {code}: its transfer is not a 32-bit value there")
    bad = first_invalid(lin, thr)
    if bad is not None:
        raise ValueError(f"light {name(spec)}: the tables are not valid at code {bad} (lin[{max(bad - 1, 0)}] = {int(lin[max(bad - 1, 0)])}, "
                         f"thr[{bad}] = {int(thr[bad])}, lin[{bad}] = {int(lin[bad])}; need lin[0] == 0, lin[255] <= {S} and "
                         f"lin[c-1] < thr[c] <= lin[c])")
    return lin.astype(np.uint32), thr.astype(np.uint32)


def device_tables(spec, device):
    """(device, host) int32 tensors of the 512 words lin[256], thr[256] (all below 2^24) for the C entry points, made once per light and
    device and kept; the upload has completed when this returns, so any stream may read them."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("light tables live on an MI355X (HIP kernels); there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (name(spec), dev.index)
    with _cache_lock:
        if key not in _cache:
            lin, thr = tables(spec)
            host = torch.from_numpy(np.concatenate([lin, thr]).astype(np.int32))
            on = host.to(dev)
            torch.cuda.current_stream(dev).synchronize()
            _cache[key] = (on, host)
        return _cache[key]
