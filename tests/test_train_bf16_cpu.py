"""CPU side of `train_precision = "bf16"` (speinet_amd/train.py): the mode is accepted on both drop-in models, directly and through
SPEINET_TRAIN_PRECISION, unknown modes still raise, and every C-ABI entry the mode adds is declared and exported."""
import ctypes
import os

import pytest

from speinet_amd import _lib

NEW_ENTRIES = ("spei_conv_wgrad_bf16_batched", "spei_conv_s2_adjoint_slab16", "spei_window_attention16_train",
               "spei_window_attention16_bwd")


def _models():
    from speinet_amd.speinet import SPEINet as Full, default_args
    from speinet_amd.swint import SPEINet as Swint
    args = default_args()
    args.n_sequence = 3
    return Swint(n_sequence=3, args=args), Full(args=args)


def test_bf16_is_accepted_on_both_models():
    from speinet_amd import train as T
    for net in _models():
        net.train_precision = "bf16"
        assert T._train_precision(net) == "bf16"


def test_bf16_through_the_environment(monkeypatch):
    from speinet_amd import train as T
    monkeypatch.setenv("SPEINET_TRAIN_PRECISION", "bf16")
    for net in _models():
        assert net.train_precision == "bf16" and T._train_precision(net) == "bf16"


def test_unknown_precision_still_raises():
    from speinet_amd import train as T
    for net in _models():
        for bad in ("f16", "bf16x2", "tf32"):
            net.train_precision = bad
            with pytest.raises(ValueError):
                T._train_precision(net)


def test_new_entries_declared_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        from speinet_amd.build import build_lib
        build_lib(verbose=False)
    h = ctypes.CDLL(_lib.LIB_PATH)
    declared = _lib.header_symbols()
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} missing from include/speinet_hip.h"
        assert name in _lib.SIGNATURES, f"{name} missing from the ctypes table"
        assert hasattr(h, name), f"{name} not exported by the library"
