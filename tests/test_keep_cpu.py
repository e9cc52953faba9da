"""`deblur_clip(..., sharp=)` without a GPU: the argument check in the whole-clip and the stream mode, with the model None (every refusal
comes before the model is looked at, as in tests/test_clip_checks_cpu.py), the command line's refusal before the model loads, the
entry point in the C-ABI header, and the bound on the input records that wait to be written (`clip.RecordQueue`)."""
import numpy as np
import pytest

from speinet_amd import _lib, video

T, H, W = 8, 20, 24
FRAMES = np.zeros((T, H, W, 3), np.uint8)
TEXT = r"sharp must be \"deblur\" or \"keep\", got "


@pytest.mark.parametrize("mode", ["whole", "stream"])
@pytest.mark.parametrize("value", ["maybe", True, None, 1, "KEEP"], ids=repr)
def test_sharp_is_refused(value, mode):
    frames, kw = (FRAMES, {}) if mode == "whole" else (iter(list(FRAMES)), {"stream": True})
    with pytest.raises(ValueError, match=TEXT + ("'" + value + "'" if isinstance(value, str) else repr(value))):
        video.deblur_clip(None, frames, sharp=value, **kw)


@pytest.mark.parametrize("mode", ["whole", "stream"])
def test_sharp_speaks_among_the_argument_checks(mode):
    """Behind the ensemble check, in front of the checks that look at the frames."""
    frames, kw = (FRAMES, {}) if mode == "whole" else (iter(list(FRAMES)), {"stream": True})
    with pytest.raises(ValueError, match="ensemble must be"):
        video.deblur_clip(None, frames, sharp="maybe", ensemble=3, **kw)
    frames = FRAMES if mode == "whole" else iter(list(FRAMES))
    with pytest.raises(ValueError, match=TEXT):
        video.deblur_clip(None, frames, sharp="maybe", roi=(0, 0, 30, 30), out_depth=9, **kw)


@pytest.mark.parametrize("value", ["deblur", "keep"])
def test_the_two_values_pass_the_check(value):
    """With a model of None the call then fails where `ClipRun` looks at the model, not in the argument checks."""
    with pytest.raises(AttributeError, match="parameters"):
        video.deblur_clip(None, FRAMES, sharp=value)


def test_cli_refuses_sharp_before_the_model_loads(monkeypatch, tmp_path, capsys):
    def boom(*a, **k):
        raise AssertionError("the model was loaded")
    monkeypatch.setattr(video, "load_model", boom)
    with pytest.raises(SystemExit) as e:
        video.main(["--input", str(tmp_path), "--output", str(tmp_path / "out"), "--model_path", "synthetic", "--sharp", "x"])
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "--sharp" in err and "deblur" in err and "keep" in err


def test_header_declares_frame_requant():
    assert "spei_frame_requant" in _lib.header_symbols()
    res, args = _lib.SIGNATURES["spei_frame_requant"]
    assert res is _lib.C.c_int and len(args) == 7
    assert args == [_lib.C.c_void_p, _lib.C.c_int, _lib.C.c_void_p, _lib.C.c_int, _lib.C.c_int, _lib.C.c_int, _lib.C.c_void_p]


def test_record_queue_bounds_the_writes_in_flight():
    """A sink slower than the producer: write i does not end before the producer has come to queue record i + n.  With at most n writes
    in flight that `put` waits for write i, so every write sees at most n records handed over and not yet written; a queue without
    the bound would have let the producer run on.  The records are copies: the producer reuses its buffer."""
    import threading
    from concurrent.futures import ThreadPoolExecutor

    from speinet_amd.clip import RecordQueue
    n, total = 4, 24
    reached = [threading.Event() for _ in range(total)]
    handed, written, pending = [0], [], []

    def write(rec):
        i = int(rec[0])
        assert reached[min(i + n, total - 1)].wait(60)
        pending.append(handed[0] - len(written))
        written.append(i)

    with ThreadPoolExecutor(max_workers=1) as pool:
        q = RecordQueue(pool, n)
        buf = np.zeros(3, np.uint8)
        for i in range(total):
            buf[0] = i
            reached[i].set()
            q.put(write, buf)
            handed[0] += 1
            assert q.in_flight <= n
        q.drain()
    assert written == list(range(total)) and q.in_flight == 0
    assert max(pending) <= n and pending[0] == n           # the bound held, and the producer did run up against it


def test_record_queue_raises_a_failed_write():
    from concurrent.futures import ThreadPoolExecutor

    from speinet_amd.clip import RecordQueue

    def write(rec):
        raise OSError("the sink is gone")
    with ThreadPoolExecutor(max_workers=1) as pool:
        q = RecordQueue(pool, 2)
        with pytest.raises(OSError, match="the sink is gone"):
            for _ in range(3):
                q.put(write, np.zeros(1, np.uint8))
        q.put(write, np.zeros(1, np.uint8))
        with pytest.raises(OSError):
            q.drain()
