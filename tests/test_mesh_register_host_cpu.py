"""The bodies the registration kernels call (csrc/register_passes.hpp: moving a point, a face's normal, a row's terms and weight, the
rows a lane adds and the tree over the lanes), compiled by the host compiler with -ffp-contract=off into
tests/register_host_check.cpp and held to tests/register_ref.py bit for bit; once plain and once under the address and
undefined-behaviour sanitizers where the host compiler has them."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import eval_ref as E
import register_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = "-fsanitize=address,undefined"
KERNELS = ("l2", ("huber", R.K_EXACT), ("tukey", R.K_EXACT))


@functools.lru_cache(maxsize=None)
def _program(tmp, sanitize):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    assert cxx, "no host C++ compiler (the oracle's Makefile needs one as well)"
    exe = os.path.join(tmp, "register_host_check" + ("_san" if sanitize else ""))
    cmd = [cxx, "-O1" if sanitize else "-O2", "-g", "-std=c++17", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "register_host_check.cpp"), "-o", exe]
    if sanitize:
        if subprocess.run(cmd + [SANITIZE, "-fno-sanitize-recover=all"], capture_output=True, text=True).returncode != 0:
            pytest.skip("host compiler without " + SANITIZE)
    else:
        subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    exe = _program(str(tmp_path_factory.mktemp("register_host")), request.param)

    def call(path, args, kernel, T):
        name, k = R.parse_kernel(kernel)
        words = lambda a: " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))
        bits64 = lambda a: words(np.ascontiguousarray(a, np.float64).view(np.uint64))
        bits32 = lambda a: words(np.ascontiguousarray(a, np.float32).view(np.uint32))
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
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
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
