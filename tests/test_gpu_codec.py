"""Codec artefacts of blur synthesis on the device: spei_codec_u8 and spei_train_batch_codec_f32 (csrc/codec.hip) bit for bit against the
numpy restatement tests/codec_ref.py, blurset.synthesize across chunk sizes, data.SharpTrainLoader and one training step with a codec,
and the checks that refuse a launch.  Equality throughout: the arithmetic is integer."""
import ctypes as C
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import codec_ref  # noqa: E402
from sharpset_ref import moving_clip, write_sharp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QUALITIES = (10, 50, 90, 100)
OFFSETS = (0, 7, 15)
# one MCU; smaller than a block; 20 x 28: partial MCUs both ways; 33 x 47: odd, rows of 141 bytes (not dword-aligned), three MCUs each way
SIZES = [(16, 16), (5, 3), (20, 28), (33, 47)]


def _qtabs():
    from speinet_amd import codec
    return np.stack([codec.quant_tables(q) for q in QUALITIES])


def _content(kind, H, W):
    rs = np.random.RandomState(H * 100 + W)
    if kind == "random":
        return rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        one = np.stack([3 * x + 2 * y, 255 - 4 * x, 40 + 5 * y], axis=-1)
        return np.stack([np.clip(one + 20 * n, 0, 255) for n in range(3)]).astype(np.uint8)
    flat = np.empty((3, H, W, 3), np.uint8)
    flat[...] = np.array([[200, 30, 90], [0, 0, 0], [255, 255, 254]], np.uint8)[:, None, None, :]
    return flat


@pytest.mark.parametrize("H,W", SIZES)
def test_codec_u8_against_the_numpy_restatement(H, W):
    """Three frames a launch with three different records, the middle one SKIP, a frame stride of one frame plus 7 bytes; every pair of
    grid offsets from {0, 7, 15}, the four qualities in turn, random bytes, a ramp and flat frames: the coded frames bit for bit, the
    skipped frame and its gray plane untouched, the gray planes of the coded frames those of `frames_u8_in` on the new bytes."""
    from speinet_amd import codec, ops
    qtabs = _qtabs()
    stride = H * W * 3 + 7
    k = 0
    for kind in ("random", "ramp", "flat"):
        src = _content(kind, H, W)
        for oy, ox in itertools.product(OFFSETS, OFFSETS):
            buf = torch.full((3 * stride,), 201, dtype=torch.uint8, device=DEV)
            frames = buf.as_strided((3, H, W, 3), (stride, W * 3, 3, 1))
            frames.copy_(torch.from_numpy(src))
            gray = torch.full((3, H, W), -1.0, device=DEV)
            rec = codec.records(3, qtab=[k % 4, 2, (k + 1) % 4], oy=[oy, 3, ox], ox=[ox, 4, oy], flags=[0, codec.SKIP, 0])
            assert ops.codec_u8(frames, rec, qtabs, gray=gray) is frames
            torch.cuda.synchronize()
            got = frames.cpu().numpy()
            assert np.array_equal(got[0], codec_ref.round_trip(src[0], qtabs[k % 4], oy, ox)), (kind, oy, ox, QUALITIES[k % 4])
            assert np.array_equal(got[2], codec_ref.round_trip(src[2], qtabs[(k + 1) % 4], ox, oy)), (kind, ox, oy, QUALITIES[(k + 1) % 4])
            assert np.array_equal(got[1], src[1]) and bool((gray[1] == -1.0).all())
            assert bool((buf.view(3, stride)[:, H * W * 3:] == 201).all())            # the bytes between the frames
            if min(H, W) > 16:
                _, want_gray = ops.frames_u8_in(frames, gray=True, planes=False)
            else:                       # frames_u8_in reflect-pads and refuses a 5 x 3 frame: the window mean's gray plane is the same one
                _, _, want_gray = ops.window_mean_u8(frames, np.arange(3), np.ones(3, np.int64), gray=True)
            assert torch.equal(gray[0], want_gray[0]) and torch.equal(gray[2], want_gray[2])
            if kind == "flat":
                assert (got[0] == got[0][0, 0]).all() and (got[2] == got[2][0, 0]).all()
            k += 1
    # without a gray plane, and contiguous frames: the same bytes
    src = _content("random", H, W)
    frames = torch.from_numpy(src).to(DEV)
    ops.codec_u8(frames, codec.records(3, qtab=1, oy=7, ox=15), qtabs)
    assert np.array_equal(frames.cpu().numpy(), np.stack([codec_ref.round_trip(f, qtabs[1], 7, 15) for f in src]))


def _synthesised(P, y0, x0, rgb_range):
    """One launch of train_batch_runs with light and shake on a 70 x 150 clip: nine input records at (y0, x0) — the eight flag
    combinations and a zero record, runs of 1, 2 and 15 frames, every other one shaken -> (input on the device, its records' flags,
    the full synthesised frame of every record as uint8)."""
    from speinet_amd import ops, shake
    from speinet_amd.data import RUN_RECORD
    H, W, T = 70, 150, 17
    frames = np.random.RandomState(5).randint(0, 256, (T, H, W, 3)).astype(np.uint8)
    src = torch.from_numpy(frames).to(DEV)
    w, radius, q16 = shake.psf("4..12", 5, 1, 2)
    table = w[None].astype(np.uint32)
    runs = [(0, 1), (1, 2), (2, 15)]
    rows, srec, flags = [], [], []
    for k in range(9):
        s, n = runs[k % 3]
        f = (8 | 5) if k == 8 else k
        rows.append((src.data_ptr() + s * H * W * 3, H * W * 3, W * 3, y0, x0, f, H, W, n, T - s))
        srec.append((0, radius, q16, 0) if k % 2 else (0, 0, 65536, 0))
        flags.append(f)
    rec = np.array(rows, dtype=RUN_RECORD)
    srec = np.array(srec, dtype=shake.SHAKE_RECORD)
    host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    shost = torch.from_numpy(srec.view(np.uint8).reshape(-1).copy())
    inp = torch.full((9, 3, P, P), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch_runs(host.to(DEV), host, 9, 0, inp, torch.empty(0, device=DEV), P, rgb_range, light="srgb",
                                             shake=(shost.to(DEV), shost, shake.device_psfs(table, DEV)))
    full = [ops.window_mean_u8(src, [runs[k % 3][0]], [runs[k % 3][1]], light="srgb", shake=(srec[k:k + 1], table))[0] for k in range(9)]
    torch.cuda.synchronize()
    return inp, np.array(flags), torch.cat(full)


@pytest.mark.parametrize("rgb_range", [1.0, 255.0])
@pytest.mark.parametrize("P,y0,x0", [(20, 23, 29), (32, 16, 48), (40, 23, 29)])
def test_train_batch_codec(P, y0, x0, rgb_range):
    """In place on the real output of train_batch_runs (light srgb, shake), all eight flag combinations and a zero record, the four
    qualities in turn: the whole tensor is the restatement's — border ring included — and, un-augmented, every MCU wholly inside the
    crop equals spei_codec_u8 on the whole synthesised frame.  (7, 13) are the offsets of the crop at (23, 29); a 20 x 20 crop there
    holds no whole MCU, the 40 x 40 one holds two, the 32 x 32 one at a multiple of 16 is four whole MCUs."""
    from speinet_amd import codec, ops
    qtabs = _qtabs()
    inp, flags, full = _synthesised(P, y0, x0, rgb_range)
    before = inp.cpu().numpy()
    assert (before[8] == 0).all() and before[:8].max() > 0
    rec = codec.records(9, qtab=np.arange(9) % 4, oy=y0 % 16, ox=x0 % 16, flags=flags)
    assert (y0 % 16, x0 % 16) in ((7, 13), (0, 0))
    rhost = torch.from_numpy(rec.view(np.uint8).copy())
    with torch.cuda.device(DEV):
        ops.Ctx(device=DEV).train_batch_codec(inp, 9, P, rgb_range, rhost.to(DEV), rhost, codec.device_qtabs(qtabs, DEV))
    torch.cuda.synchronize()
    got = inp.cpu().numpy()
    want = codec_ref.train_batch_codec(before, rgb_range, rec, qtabs)
    for k in range(9):
        assert np.array_equal(got[k], want[k]), (k, int(flags[k]))
    assert (got[8] == 0).all() and not np.array_equal(got[:8], before[:8])
    # the whole-frame pass on the synthesised frames, on the frame's own grid
    ops.codec_u8(full, codec.records(9, qtab=np.arange(9) % 4), qtabs)
    full = full.cpu().numpy()
    s = np.float32(rgb_range / 255.0)
    whole = 0
    for k in range(8):
        mine = codec_ref.unaugment(got[k].transpose(1, 2, 0), int(flags[k]))
        for my in range(-(-y0 // 16) * 16, y0 + P - 15, 16):
            for mx in range(-(-x0 // 16) * 16, x0 + P - 15, 16):
                a = mine[my - y0:my - y0 + 16, mx - x0:mx - x0 + 16]
                assert np.array_equal(a, full[k][my:my + 16, mx:mx + 16].astype(np.float32) * s), (k, my, mx)
                whole += 1
    assert whole == 8 * {20: 0, 32: 4, 40: 2}[P]


def test_train_batch_codec_refuses_an_inexact_rgb_range():
    """(float)u * (float)(rgb_range / 255) must give u back by (int)(v * (float)(255 / rgb_range) + 0.5f) for all 256 codes: a range so
    small that its scale underflows does not, and nothing is launched."""
    from speinet_amd import codec, ops
    qtabs = _qtabs()
    inp = torch.full((1, 3, 16, 16), 0.5, device=DEV)
    rec = codec.records(1)
    rhost = torch.from_numpy(rec.view(np.uint8).copy())
    with torch.cuda.device(DEV):
        with pytest.raises(RuntimeError, match="spei_train_batch_codec_f32: rgb_range"):
            ops.Ctx(device=DEV).train_batch_codec(inp, 1, 16, 1e-43, rhost.to(DEV), rhost, codec.device_qtabs(qtabs, DEV))
    torch.cuda.synchronize()
    assert bool((inp == 0.5).all())


def test_synthesize_with_a_codec_does_not_depend_on_the_chunk():
    """blurset.synthesize(codec=) on a 6-frame 20 x 28 clip with chunk_frames 2 and 64, and — a chunk holds at least 15 frames — on a
    34-frame clip with chunks of 15 and of 64: identical bytes and gray planes, gt untouched, blur the restatement of the frames made
    without a codec at the clip's quality, the gray planes those of the coded bytes; `codec=None` is the plain call."""
    from speinet_amd import blurset, codec, ops
    H, W = 20, 28
    for n, chunks in ((6, (2, 64)), (34, (15, 64))):
        frames = moving_clip(4, n, H, W)
        runs = blurset.plan_runs(n, 0.5, rng=random.Random(1)) if n > 6 else (np.arange(6), np.ones(6, np.int64), np.array([0, 1, 0, 1, 1, 0]))
        assert n == 6 or len(list(blurset._chunks(runs[0], runs[1], 15))) > 1
        cc = codec.ClipCodec("30..90", 21, 2)
        q = codec.quality("30..90", 21, 2)
        outs = [blurset.synthesize(frames, runs, DEV, gray=True, chunk_frames=c, light="srgb", codec=cc) for c in chunks]
        assert all(torch.equal(a, b) for a, b in zip(*outs))
        plain = blurset.synthesize(frames, runs, DEV, gray=True, chunk_frames=64, light="srgb")
        again = blurset.synthesize(frames, runs, DEV, gray=True, chunk_frames=64, light="srgb", codec=None)
        assert all(torch.equal(a, b) for a, b in zip(plain, again))
        assert torch.equal(outs[0][1], plain[1])                                  # gt is never coded
        want = np.stack([codec_ref.round_trip(f, codec.quant_tables(q)) for f in plain[0].cpu().numpy()])
        assert np.array_equal(outs[0][0].cpu().numpy(), want) and not np.array_equal(want, plain[0].cpu().numpy())
        _, gray = ops.frames_u8_in(outs[0][0], gray=True, planes=False)
        assert torch.equal(outs[0][2], gray)
    # the light `code` takes a codec too
    coded = blurset.synthesize(frames, runs, DEV, codec=cc)[0].cpu().numpy()
    base = blurset.synthesize(frames, runs, DEV)[0].cpu().numpy()
    assert np.array_equal(coded, np.stack([codec_ref.round_trip(f, codec.quant_tables(q)) for f in base]))


def test_loader_and_one_training_step(tmp_path):
    """One batch of SharpTrainLoader at batch size 2 and patch 20 with a codec equals the restatement applied to the batch made without
    it (ground truth identical); one training step on such batches runs and its loss is finite."""
    from speinet_amd import data
    from speinet_amd.fit import Fit, build_model
    from speinet_amd.loss import Loss
    src = write_sharp(str(tmp_path / "sharp"), {f"clip{c}": moving_clip(30 + c, 30, 40, 48) for c in range(2)})

    def first_batch(codec_spec):
        cs = data.SharpClipSet(src, ratios=(0.5,), seed=2, patch=20, light="srgb", codec=codec_spec)
        store = data.SharpStore(cs, device=DEV, log=None)
        loader = data.SharpTrainLoader(cs, store, 2, 20, seed=3, rank=0, world=1)
        inp, gt = [(i.clone(), g.clone()) for i, g in loader][0]
        return cs, store, inp, gt

    _, _, plain_in, plain_gt = first_batch(None)
    cs, store, coded_in, coded_gt = first_batch("30..90")
    torch.cuda.synchronize()
    assert torch.equal(plain_gt, coded_gt) and coded_in.shape == (2, 5, 3, 20, 20)
    items = data.SharpSampler(cs, 2, 20, seed=3, rank=0, world=1).epoch()[0]
    rec = data.run_codec_records(cs, items, data.run_records(cs, store, items))
    from speinet_amd import codec
    want = codec_ref.train_batch_codec(plain_in.cpu().numpy().reshape(10, 3, 20, 20), 1.0, rec, codec.all_tables())
    assert np.array_equal(coded_in.cpu().numpy().reshape(10, 3, 20, 20), want) and not torch.equal(coded_in, plain_in)

    net = build_model("swint", DEV, train_precision="f32", synthetic_seed=0)
    cs = data.SharpClipSet(src, ratios=(0.5,), seed=2, references=False, patch=40, codec="30..90")
    loader = data.SharpTrainLoader(cs, data.SharpStore(cs, device=DEV, log=None), batch=2, patch=40, seed=1)
    lines = []
    fit = Fit(net, Loss("1*L1+2*HEM", device=DEV), loader, None, save=str(tmp_path / "exp"), lr=1e-4, lr_decay=3, epochs=1, print_every=1000,
              resume=False, seed=1, log=lines.append)
    fit.run()
    assert "codec 30..90" in "\n".join(lines) and len(fit.loss_log) == 1 and np.isfinite(fit.loss_log[0])


def test_invalid_records_launch_nothing():
    """Each bad record or table, second of two records, handed straight to either entry point: non-zero, the text names the entry
    point and the record (or the table), and the frames, pre-filled with a sentinel, are untouched."""
    from speinet_amd import _lib, codec
    lib = _lib.lib()
    H, W, P = 16, 32, 16
    good = _qtabs()[:2]
    flat = np.full((H, W, 3), 77, np.uint8)
    zero_entry = good.copy()
    zero_entry[1, 1, 5] = 0
    big_entry = good.copy()
    big_entry[0, 0, 63] = 256
    cases = [("qtab out of range", good, (2, 0, 0, 0), "codec record 1: table 2 of 2 tables"),
             ("a table entry of 0", zero_entry, (0, 0, 0, 0), "quantisation table 1: entry 5 of its chrominance table is 0"),
             ("a table entry of 256", big_entry, (0, 0, 0, 0), "quantisation table 0: entry 63 of its luminance table is 256"),
             ("oy = 16", good, (0, 16, 0, 0), "codec record 1: grid offset (oy 16, ox 0)"),
             ("ox = 16", good, (0, 0, 16, 0), "codec record 1: grid offset (oy 0, ox 16)"),
             ("an unknown flag bit", good, (0, 0, 0, 32), "codec record 1 has unknown flag bits 0x20"),
             ("valid", good, (1, 15, 15, 0), None)]
    for what, tables, fields, text in cases:
        q_dev, q_host = codec.device_qtabs(tables, DEV)
        rec = codec.records(2)
        rec[1] = fields
        r_host = torch.from_numpy(rec.view(np.uint8).copy())
        r_dev = r_host.to(DEV)
        frames = torch.full((2, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        inp = torch.full((2, 3, P, P), 77.0, device=DEV)
        with torch.cuda.device(DEV):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc_u = lib.spei_codec_u8(C.c_void_p(frames.data_ptr()), H * W * 3, 2, H, W, C.c_void_p(r_dev.data_ptr()), C.c_void_p(r_host.data_ptr()),
                                     C.c_void_p(q_dev.data_ptr()), C.c_void_p(q_host.data_ptr()), 2, C.c_void_p(0), st)
            msg_u = lib.spei_last_error().decode()
            rc_f = lib.spei_train_batch_codec_f32(C.c_void_p(inp.data_ptr()), 2, P, 255.0, C.c_void_p(r_dev.data_ptr()),
                                                  C.c_void_p(r_host.data_ptr()), C.c_void_p(q_dev.data_ptr()), C.c_void_p(q_host.data_ptr()), 2, st)
            msg_f = lib.spei_last_error().decode()
        torch.cuda.synchronize()
        if text is None:
            assert rc_u == 0 and rc_f == 0, (msg_u, msg_f)
            want = [codec_ref.round_trip(flat, good[0]), codec_ref.round_trip(flat, good[1], 15, 15)]
            assert np.array_equal(frames.cpu().numpy(), np.stack(want)) and not (want[0] == 77).all()
            assert np.array_equal(inp.cpu().numpy(), codec_ref.train_batch_codec(np.full((2, 3, P, P), 77.0, np.float32), 255.0, rec, good))
            continue
        assert rc_u != 0 and msg_u.startswith("spei_codec_u8: ") and text in msg_u, (what, rc_u, msg_u)
        assert rc_f != 0 and msg_f.startswith("spei_train_batch_codec_f32: ") and text in msg_f, (what, rc_f, msg_f)
        assert bool((frames == 77).all()) and bool((inp == 77.0).all()), what
    # the geometry flags belong to the training entry alone
    rec = codec.records(2, flags=[0, 1])
    r_host = torch.from_numpy(rec.view(np.uint8).copy())
    r_dev = r_host.to(DEV)
    q_dev, q_host = codec.device_qtabs(good, DEV)
    frames = torch.full((2, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.spei_codec_u8(C.c_void_p(frames.data_ptr()), H * W * 3, 2, H, W, C.c_void_p(r_dev.data_ptr()), C.c_void_p(r_host.data_ptr()),
                               C.c_void_p(q_dev.data_ptr()), C.c_void_p(q_host.data_ptr()), 2, C.c_void_p(0), st)
        assert rc != 0 and "codec record 1 has unknown flag bits 0x1" in lib.spei_last_error().decode()
