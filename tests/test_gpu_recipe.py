"""Blur synthesis computes, byte for byte, what it computed before it was restated over speinet_amd.recipe: the digests of
tests/recipe_digests.py — blurset.synthesize at two chunk sizes and the first batches of two epochs of data.SharpTrainLoader, under six
recipes from the reference's path to every stage at once — against tests/golden/g26_recipe_parent.json, recorded by
tests/golden/make_golden_recipe.py at the commit named in that file.  The kernels are integer and counter-based: no tolerance."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import recipe_digests      # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_digest_is_the_parent_commits(tmp_path):
    with open(os.path.join(HERE, "golden", "g26_recipe_parent.json")) as f:
        golden = json.load(f)
    want = golden["digests"]
    # 6 recipes x (2 clips x 2 chunk sizes x (blur, gt, gray) + references on / off x 2 epochs x 2 batches x (input, gt))
    assert len(want) == len(recipe_digests.RECIPES) * (2 * 2 * 3 + 2 * 2 * 2 * 2) == 168
    got = recipe_digests.digests(str(tmp_path))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"{len(differ)} of {len(want)} digests differ from commit {golden['commit']}: {differ[:8]}"
    # the recipes are not each other: every stage changes the bytes it is meant to change, and none touches the ground truth
    blur = {name: got[f"{name}/synthesize/clip1/chunk15/blur"] for name in recipe_digests.RECIPES}
    assert len(set(blur.values())) == len(blur)
    assert len({got[f"{name}/synthesize/clip1/chunk15/gt"] for name in recipe_digests.RECIPES if name != "all_single"}) == 1
    assert all(got[k] == got[k.replace("chunk15", "chunk64")] for k in got if "chunk15" in k)
