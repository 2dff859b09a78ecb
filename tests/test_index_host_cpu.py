"""The host-compilable parts of the shared index builds (csrc/octree_build.hpp: level_of, max_nodes, the Morton code;
csrc/bulk_grid.hpp: the resolution solve, lower_bound, the 256-byte round-up) -- the functions the kernels call, compiled by the host
compiler into tests/index_host_check.cpp and held to the numpy oracles; once plain and once under the address and
undefined-behaviour sanitizers where the host compiler has them."""
import bisect

import numpy as np
import pytest

import host_program
import raycast_ref as R


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("index_host_check.cpp", tmp_path_factory.mktemp("index_host"), sanitize)

    def call(*args):
        out = host_program.run(exe, [str(a) for a in args], 120, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
        return [line.split() for line in out.stdout.strip().splitlines()]
    return call


def test_level_and_node_bound(run):
    sizes = [1, 8, 9, 64, 65, 38012, 2 ** 31 - 1]
    got = [[int(x) for x in row] for row in run("level", *sizes)]
    assert got == [[F, R.level_of(F), R.max_nodes(F)] for F in sizes]
    assert [row[1] for row in got] == [0, 0, 1, 2, 2, 7, 10]            # 8 * 4^L >= F, at most 10


def test_morton_code(run):
    rng = np.random.default_rng(5)
    cells = np.concatenate([[[0, 0, 0], [1023, 1023, 1023], [1023, 0, 0], [0, 1023, 0], [0, 0, 1023], [1, 2, 4], [682, 341, 1023]],
                            rng.integers(0, 1024, (50, 3))]).astype(np.int64)
    got = [int(row[0]) for row in run("morton", *cells.reshape(-1).tolist())]
    assert got == R._morton(cells, 10).tolist()
    small = rng.integers(0, 8, (20, 3)).astype(np.int64)                 # L = 3: the low 9 bits
    assert [int(row[0]) for row in run("morton", *small.reshape(-1).tolist())] == R._morton(small, 3).tolist()
    assert got[2] == 0x24924924 and got[4] == 0x09249249                # x is the highest bit of each triple


def test_resolution_solve_on_the_two_layouts_derived_by_hand(run):
    """tests/test_mesh_closest_gpu.py: the 3 x 3 x 2 box (span (3, 3, 2), 24 cells allowed: 3 x 3 x 2 cells of size 1) and the
    2 x 1 x 0.5 box (5 x 2 x 1 cells).  Cell counts only: the host's cbrt need not round as the device's, and both cases sit far
    from a boundary of the floor (3.3, 3.3, 2.2 and 5.8, 2.9, 1.4)."""
    assert [int(x) for x in run("solve", -1.5, -1.5, -1.0, 1.5, 1.5, 1.0, 12, 24)[0][:4]] == [3, 3, 2, 18]
    assert [int(x) for x in run("solve", -1.0, -0.5, -0.25, 1.0, 0.5, 0.25, 12, 24)[0][:4]] == [5, 2, 1, 10]
    # nothing to index, and a bulk of one point: one unit cell
    assert run("solve", 0, 0, 0, 0, 0, 0, 0, 2)[0] == ["1", "1", "1", "1", "1", "1", "1"]
    assert run("solve", 3, 4, 5, 3, 4, 5, 7, 14)[0] == ["1", "1", "1", "1", "1", "1", "1"]
    # a planar bulk: the thin axis is taken as 2^-10 of the longest, and gets one cell of that size
    row = run("solve", 0, 0, 1, 4, 4, 1, 100, 200)[0]
    Rx, Ry, Rz, ncells = (int(x) for x in row[:4])
    assert Rz == 1 and Rx == Ry and ncells == Rx * Ry <= 200 and float(row[6]) == np.float32(4.0 * 2.0 ** -10)
    # the per-axis cap
    row = run("solve", 0, 0, 0, 1e6, 1.0, 1.0, 1 << 21, 1 << 22)[0]
    assert int(row[0]) == 1024 and int(row[3]) <= 1 << 22


def test_lower_bound_and_round_up(run):
    v = [0, 0, 3, 3, 3, 7, 9, 9]
    for x in (0, 1, 3, 4, 9, 10):
        assert [int(y) for y in run("search", x, *v)[0]] == [bisect.bisect_left(v, x), -(-x // 256) * 256]
    assert [int(y) for y in run("search", 5)[0]] == [0, 256]              # an empty array
