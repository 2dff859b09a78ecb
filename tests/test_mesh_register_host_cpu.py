"""The bodies the registration kernels call (csrc/register_passes.hpp: moving a point, a face's normal, a row's terms and weight, the
rows a lane adds and the tree over the lanes), compiled by the host compiler with -ffp-contract=off into
tests/register_host_check.cpp and held to tests/register_ref.py bit for bit; once plain and once under the address and
undefined-behaviour sanitizers where the host compiler has them."""
import numpy as np
import pytest

import eval_ref as E
import host_program
from host_program import bits32, bits64, words
import register_ref as R

KERNELS = ("l2", ("huber", R.K_EXACT), ("tukey", R.K_EXACT))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("register_host_check.cpp", tmp_path_factory.mktemp("register_host"), sanitize, flags=("-ffp-contract=off",))

    def call(path, args, kernel, T):
        name, k = R.parse_kernel(kernel)
        cur = args["cur"]
        surface = "face_idx" in args
        m, V, F = (0, len(args["verts"]), len(args["faces"])) if surface else (len(args["targets"]), 0, 0)
        lines = [words([len(cur), int(surface), R.KERNELS.index(name), int(np.array([k], np.float64).view(np.uint64)[0]), m, V, F]),
                 bits64(T), bits64(cur)]
        if surface:
            lines += [words(args["face_idx"]), bits64(args["d2"]), bits32(args["closest"]), bits32(args["verts"]), words(args["faces"])]
        else:
            lines += [words(args["idx"]), bits32(args["dist"]), bits32(args["targets"]), bits32(args["normals"])]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        out = host_program.run(exe, [str(path)], 120, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
        rows = out.stdout.split("\n")
        return dict(sums=np.array(rows[0].split(), np.uint64), counts=[int(x) for x in rows[1].split()],
                    moved=np.array(rows[2].split(), np.uint64).reshape(-1, 3), moved32=np.array(rows[3].split(), np.uint32).reshape(-1, 3))
    return call


def _compare(got, args, kernel, T):
    ref = R.plane_system(kernel=kernel, **args)
    assert got["counts"] == [ref["k_corr"], ref["k_used"]]
    assert (got["sums"] == ref["sums"].view(np.uint64)).all(), np.nonzero(got["sums"] != ref["sums"].view(np.uint64))[0]
    moved = E.transform(args["cur"], T)
    assert (got["moved"] == moved.view(np.uint64)).all()
    assert (got["moved32"] == moved.astype(np.float32).view(np.uint32)).all()


@pytest.mark.parametrize("n", [1, 255, 257, 4097])
@pytest.mark.parametrize("mode", ["cloud", "surface"])
def test_bodies_equal_the_reference_bit_for_bit(run, tmp_path, mode, n):
    """every third row without a correspondence, zero and NaN normals, a face without area, and rows with |r| exactly k"""
    args = (R.synthetic_cloud if mode == "cloud" else R.synthetic_surface)(n, seed=n)
    T = E.rigid([0.3, -1.0, 0.5], 7.0, [0.1, -0.2, 0.05])
    for kernel in KERNELS:
        _compare(run(tmp_path / "case.txt", args, kernel, T), args, kernel, T)


def test_no_correspondence_and_the_large_coordinate_rows(run, tmp_path):
    T = E.rigid([1.0, 0.2, 0.1], 1.0, [3.0, -2.0, 1.0])
    none = R.synthetic_cloud(300, drop="all")
    got = run(tmp_path / "case.txt", none, "l2", T)
    assert got["counts"] == [0, 0] and not got["sums"].any()                       # thirty times +0.0
    _compare(got, none, "l2", T)
    big = R.large_coordinate_cloud(4097)
    _compare(run(tmp_path / "case.txt", big, "l2", T), big, "l2", T)
