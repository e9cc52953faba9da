"""SHA-256 digests of what blur synthesis computes under six recipes, through the public keyword spelling alone (blurset.synthesize,
data.SharpClipSet, data.SharpTrainLoader), so the same code runs on any commit: tests/golden/make_golden_recipe.py records them at one
commit, tests/test_gpu_recipe.py requires them of the checkout.  The kernels are integer and counter-based: equality is exact.

Content: two clips of sharpset_ref.moving_clip (seeded numpy) — 20 frames of 48 x 64 (W % 4 == 0 and H W % 16 == 0: the vector and
wide paths) and 23 frames of 41 x 47 (the pixel paths)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sharpset_ref import moving_clip, write_sharp      # noqa: E402

NOISE, SHAKE, CODEC = "0.001..0.01:0.002", "4..12", "30..90"
RECIPES = {"reference": {},
           "srgb": {"light": "srgb"},
           "srgb_noise": {"light": "srgb", "noise": NOISE},
           "gamma_shake": {"light": "gamma:2.2", "shake": SHAKE},
           "all": {"light": "srgb", "noise": NOISE, "shake": SHAKE, "codec": CODEC},
           "all_single": {"light": "srgb", "noise": NOISE, "shake": SHAKE, "codec": CODEC, "frames": "single"}}
SEED, RATIO, CHUNKS, BATCH, PATCH = 1, 0.7, (15, 64), 2, 32


def clips() -> dict:
    return {"clip0": moving_clip(26, 20, 48, 64), "clip1": moving_clip(27, 23, 41, 47)}


def _sha(t) -> str:
    a = np.ascontiguousarray(t.cpu().numpy())
    return hashlib.sha256(f"{a.dtype} {a.shape} ".encode() + a.tobytes()).hexdigest()


def digests(tmp_dir: str, device: str = "cuda:0") -> dict:
    """name -> digest: `synthesize`'s blur, gt and gray of each clip at both chunk sizes, and the input and gt tensors of the first two
    batches of epochs 0 and 1 of SharpTrainLoader (batch 2, patch 32, augmentation on, references on and off), per recipe."""
    import torch
    from speinet_amd import blurset, codec, data, light, shake
    content = clips()
    src = write_sharp(os.path.join(tmp_dir, "sharp"), content)
    out = {}
    for name, kw in RECIPES.items():
        plans = blurset.plan_dataset([f.shape[0] for f in content.values()], [RATIO], SEED, frames=kw.get("frames", "runs"))
        for k, (frames, (_ratio, runs)) in enumerate(zip(content.values(), plans)):
            stages = {"light": kw.get("light", "code"),
                      "noise": light.ClipNoise(kw["noise"], SEED, k) if "noise" in kw else None,
                      "shake": shake.ClipShake(kw["shake"], SEED, k) if "shake" in kw else None,
                      "codec": codec.ClipCodec(kw["codec"], SEED, k) if "codec" in kw else None}
            for chunk in CHUNKS:
                parts = blurset.synthesize(frames, runs, device, gray=True, chunk_frames=chunk, **stages)
                for what, t in zip(("blur", "gt", "gray"), parts):
                    out[f"{name}/synthesize/clip{k}/chunk{chunk}/{what}"] = _sha(t)
        for refs in (True, False):
            cs = data.SharpClipSet(src, ratios=(RATIO,), seed=SEED, references=refs, patch=PATCH, **kw)
            loader = data.SharpTrainLoader(cs, data.SharpStore(cs, device=device, log=None), BATCH, PATCH, seed=3, rank=0, world=1)
            for epoch in (0, 1):
                for b, (inp, gt) in enumerate(loader):
                    if b == 2:
                        break
                    out[f"{name}/loader/refs{int(refs)}/epoch{epoch}/batch{b}/input"] = _sha(inp)
                    out[f"{name}/loader/refs{int(refs)}/epoch{epoch}/batch{b}/gt"] = _sha(gt)
                assert cs.epoch == epoch
            torch.cuda.synchronize()
    return out
