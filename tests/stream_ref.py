"""Reference side of the streaming tests (tests/test_stream_cpu.py, tests/test_gpu_stream.py): the two situations in which the
incremental plan (`speinet_amd.plan.StreamPlan`) may commit an entry under its assumption, stated from the reference's selection
rule and NOT from the planner's code, the generator of the randomised plan cases, and y4m streams as bytes.

The two situations, for entry j of a scene (j counted from the scene's start; its last window frame is f = j + 1, the frame the
reference measures its later reference frame from), at a look-ahead of `horizon` frames:
  1. "after the last sharp frame": the scene's first j + horizon + 1 frames hold two or more sharp frames (so the nearest-sharp rule
     holds whatever follows), f is blurry, a sharp frame lies fewer than 7 frames before f, and none within the 7 frames after
     it.  `blurry_indices` then takes that sharp frame as the later reference if it is the scene's last one, and a far index (zeroed
     by the 7-frame rule) if any sharp frame follows, however late.
  2. "one sharp frame": the scene's first j + horizon + 1 frames hold exactly one sharp frame in padded terms (frame 1 counts twice:
     the reflect pad repeats it in front of frame 0), at frame s.  One sharp frame is planned by the neighbour rule (the reference is
     the frame next to the window's first / last frame, if that is the sharp one), two or more by the nearest-sharp rule (the sharp
     frame within 7).  For the earlier reference (looked up from frame j - 1) the two rules differ for j - 1 - s in -6..5 except 1,
     for the later one (from frame j + 1) for s - (j + 1) in 0..6 except 1: together j - s in -7..6 except 2.
Neither can arise when the scene ends within the horizon: it is then planned on its true labels."""
import random

import numpy as np

DENSITIES = (0.0, 0.05, 0.1, 0.3, 0.6)


def scenes(T, cuts):
    edges = [0] + list(cuts or []) + [T]
    return list(zip(edges[:-1], edges[1:]))


def quirk(scene_labels, j, horizon):
    """1, 2 (the situations above) or None for entry j of a scene with these (true, whole) labels."""
    lab = [int(v) for v in scene_labels]
    n, f = len(lab), j + 1
    if j + horizon >= n:
        return None
    known = lab[:j + horizon + 1]
    sharp = [i for i, v in enumerate(known) if v]
    count = len(sharp) + known[1]                            # in padded terms
    if count >= 2 and not lab[f] and any(lab[max(0, f - 6):f]) and not any(lab[f + 1:f + 8]):
        return 1
    if count == 1 and -7 <= j - sharp[0] <= 6 and j - sharp[0] != 2:
        return 2
    return None


def may_assume(labels, cuts, horizon):
    """The frames of a clip in either situation: the only ones the incremental plan may commit under its assumption."""
    return [a + j for a, b in scenes(len(labels), cuts) for j in range(b - a) if quirk(labels[a:b], j, horizon) is not None]


def plan_case(seed):
    """(labels, cuts, horizon, batch sizes) of randomised case `seed`: 2..200 frames at one of the five sharp densities, up to four
    cuts with one-frame scenes among them, feed batches of 1..40 frames."""
    r = random.Random(seed)
    T, density = r.randint(2, 200), r.choice(DENSITIES)
    labels = [1 if r.random() < density else 0 for _ in range(T)]
    cuts = set(r.sample(range(1, T), min(T - 1, r.choice([0, 0, 1, 2, 3]))))
    if cuts and r.random() < 0.5:
        cuts.add(min(T - 1, min(cuts) + 1))                  # a one-frame scene
    batches, left = [], T
    while left:
        batches.append(min(left, r.randint(1, 40)))
        left -= batches[-1]
    return labels, sorted(cuts), r.choice([24, 48]), batches


# every chroma tag the readers take with depths=(8, 10, 12) and every layout: tag -> (bytes per sample, chroma samples of an h x w frame)
def _c420(h, w):
    return 2 * ((h + 1) // 2) * ((w + 1) // 2)


def _c422(h, w):
    return 2 * h * ((w + 1) // 2)


TAGS = {"420jpeg": (1, _c420), "420": (1, _c420), "420mpeg2": (1, _c420), "444": (1, lambda h, w: 2 * h * w), "422": (1, _c422),
        "mono": (1, lambda h, w: 0)}
for _d in (10, 12):
    TAGS.update({f"420p{_d}": (2, _c420), f"444p{_d}": (2, lambda h, w: 2 * h * w), f"422p{_d}": (2, _c422), f"mono{_d}": (2, lambda h, w: 0)})


def y4m_bytes(tag, h, w, T, seed=0, frame_line=b"FRAME\n", extra="F30000:1001 Ip A1:1 XCOLORRANGE=FULL"):
    """(the stream's bytes, its T frames' payloads) for chroma tag `tag`: random samples within the tag's depth."""
    size, chroma = TAGS[tag]
    n = h * w + chroma(h, w)
    rng = np.random.default_rng(seed)
    top = 256 if size == 1 else 1 << int(tag[-2:])
    frames = [rng.integers(0, top, n).astype("u1" if size == 1 else "<u2").tobytes() for _ in range(T)]
    head = f"YUV4MPEG2 W{w} H{h} {extra} C{tag}\n".encode()
    return head + b"".join(frame_line + f for f in frames), frames
