#!/usr/bin/env python3
"""g26_recipe_parent.json — the digests of tests/recipe_digests.py as computed by one commit on an MI355X, with that commit's id:

    python tests/golden/make_golden_recipe.py <commit id> [<output json>]

Run at the commit BEFORE blur synthesis was restated over speinet_amd.recipe (its parent); tests/test_gpu_recipe.py holds every later
commit to these bytes.  Nothing but the checkout is read: the content is seeded numpy."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main(argv) -> None:
    from recipe_digests import digests
    commit = argv[0]
    out = argv[1] if len(argv) > 1 else os.path.join(HERE, "g26_recipe_parent.json")
    with tempfile.TemporaryDirectory() as tmp:
        found = digests(tmp)
    with open(out, "w") as f:
        json.dump({"commit": commit, "digests": found}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(found)} digests at {commit}")


if __name__ == "__main__":
    main(sys.argv[1:])
