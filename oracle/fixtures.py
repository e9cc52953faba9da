"""Packed form of the training-step fixtures (tests/golden/make_golden_train.py).

A fixture holds a few arrays per parameter (`norm/<name>`, `sub/<name>`, ...).  Stored one zip entry each, ~3 400 entries cost
~1 MB of archive headers alone; the packed form stores each family as ONE array: the parameter names, the scalars per name, and
the per-name arrays concatenated with their lengths.  `load_train_fixture` returns either form with the per-name keys, so a
check reads `d["sub/<name>"]` and `d.files` whichever form the file has."""
from __future__ import annotations

import numpy as np

_SCALAR = ("norm", "norm64")             # one number per parameter
_ARRAY = ("sub", "sub64", "adam", "bn")  # one array per parameter (or buffer)


def pack_train_fixture(res: dict) -> dict:
    """{"norm/<k>": float, "sub/<k>": array, ...} -> the packed arrays (other keys pass through)."""
    out = {k: v for k, v in res.items() if "/" not in k}
    for fam in _SCALAR + _ARRAY:
        keys = [k[len(fam) + 1:] for k in res if k.startswith(fam + "/")]
        if not keys:
            continue
        out[f"{fam}@names"] = np.asarray(keys)
        if fam in _SCALAR:
            out[f"{fam}@values"] = np.asarray([float(res[f"{fam}/{k}"]) for k in keys], dtype=np.float64)
        else:
            parts = [np.asarray(res[f"{fam}/{k}"]).reshape(-1) for k in keys]
            dtype = np.float64 if fam == "bn" else np.float32          # bn: running buffers and the integer batch counters
            out[f"{fam}@values"] = np.concatenate(parts).astype(dtype)
            out[f"{fam}@len"] = np.asarray([p.size for p in parts], dtype=np.int64)
    return out


class _Fixture(dict):
    @property
    def files(self):
        return list(self.keys())


def load_train_fixture(path: str) -> _Fixture:
    """The fixture at `path` with per-name keys (`norm/<k>`, `sub/<k>`, ...), packed or not."""
    d = np.load(path)
    out = _Fixture()
    for f in d.files:
        if "@" not in f:
            out[f] = d[f]
    for fam in _SCALAR + _ARRAY:
        if f"{fam}@names" not in d.files:
            continue
        names, values = d[f"{fam}@names"], d[f"{fam}@values"]
        if fam in _SCALAR:
            for k, v in zip(names, values):
                out[f"{fam}/{k}"] = np.float64(v)
        else:
            ends = np.cumsum(d[f"{fam}@len"])
            for k, a, e in zip(names, np.concatenate(([0], ends[:-1])), ends):
                out[f"{fam}/{k}"] = values[a:e]
    return out
