"""Fixture generator, run once by hand on a GPU at the commit whose index layouts are to be pinned
(`python tests/golden/make_index_layout_fixture.py <full commit hash>`, after building that commit's library):
-> tests/golden/index_layout.npz, what tests/test_index_layout_gpu.py compares the mesh indexes with.

The cases and what is recorded of each are that test module's (``record()``): the generator adds the provenance.  It refuses to run
unless the hash given is the work tree's HEAD and no tracked source of the library differs from it, and it stores the hash under
``commit``.  tests/golden/index_layout.md names the commit the committed file came from.
Data fixture (numbers only)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "index_layout.npz")


def git(*args):
    return subprocess.run(["git", "-C", ROOT] + list(args), check=True, capture_output=True, text=True).stdout.strip()


def main():
    if len(sys.argv) != 2 or len(sys.argv[1]) != 40:
        raise SystemExit(__doc__)
    commit = sys.argv[1].lower()
    head = git("rev-parse", "HEAD")
    if head != commit:
        raise SystemExit(f"HEAD is {head}, not {commit}: check that commit out, build it, and run again")
    dirty = git("status", "--porcelain", "--untracked-files=no", "--", "nicer_slam_amd", "include")
    if dirty:
        raise SystemExit("the library's sources differ from HEAD:\n" + dirty)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_index_layout_gpu as T
    out = T.record()
    out["commit"] = np.array(commit)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays, commit", commit)


if __name__ == "__main__":
    main()
