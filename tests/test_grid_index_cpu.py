"""The pure index arithmetic of csrc/grid_common.hpp -- make_grid_geom, level_row, generic_corner_terms / generic_corner_row (the index
part of gather_corners_generic) and corner_offsets, the functions the kernels call -- compiled by the host compiler into
tests/grid_index_host_check.cpp and swept over every level of the shipped geometries and of the tiny tables of
tests/test_grid_float64_gpu.py: once plain, once under the address and undefined-behaviour sanitizers where the host compiler has them.
  * cells inside a level and on its upper face: the three paths give the row of the reference's rule (stride loop with wrap, hash,
    modulo), below the level's row count;
  * cells far outside (what the device's saturating conversion makes of unit coordinates up to 1e6, negative ones and NaN; their results
    are discarded, but the fused kernels form the read): corner_offsets never leaves the TABLE (it may land in another level); level_row
    and the generic gather stay inside the level on every hashed or power-of-two level -- and do NOT on a dense level whose row count is
    no power of two (LV_SUBONCE: one conditional subtract is a modulo only for cell + 1 <= res).  That last finding is asserted as found
    (DESIGN.md section 7): a guard of the gather has to turn it into zero, and this assertion with it."""
import numpy as np
import pytest

import grid_ref64 as G
import host_program

LV_HASHED, LV_POW2, LV_SUBONCE = 1, 2, 4
SHIPPED = {"coarse": (4, 8, 32, 32, 19), "fine": (8, 4, 32, 128, 19), "colour": (16, 2, 16, 2048, 24)}


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def sweep(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("grid_index_host_check.cpp", tmp_path_factory.mktemp("grid_index_host"), sanitize)

    def call(geometry):
        from oracle import render_ref as R
        spec = R.make_grid_spec(*geometry)
        args = [spec.level_dim, repr(float(np.float32(np.log2(spec.per_level_scale)))), spec.base_resolution] + [int(o) for o in spec.offsets]
        out = host_program.run(exe, [str(a) for a in args], 120, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
        keys = "level flags rows res n_in in_disagree n_far generic_over generic_max offsets_over level_row_over offsets_out_of_table".split()
        rows = [dict(zip(keys, (int(x) for x in line.split()))) for line in out.stdout.strip().splitlines()]
        assert len(rows) == spec.num_levels
        for r, lv in zip(rows, G.levels(spec)):          # the kernel's classification against the restatement's geometry
            assert (r["rows"], r["res"], bool(r["flags"] & LV_HASHED)) == (lv.rows, lv.res, lv.hashed), (r, lv)
        return rows
    return call


@pytest.mark.parametrize("name", list(SHIPPED) + ["colour_small"] + list(G.TINY))
def test_in_range_cells_every_path_gives_the_reference_row(sweep, name):
    for r in sweep({**SHIPPED, **G.GEOMS, **G.TINY}[name]):
        assert r["n_in"] == 8 ** 3 * 8 and r["in_disagree"] == 0, r


@pytest.mark.parametrize("name", list(SHIPPED) + ["colour_small"] + list(G.TINY))
def test_far_outside_cells(sweep, name):
    rows = sweep({**SHIPPED, **G.GEOMS, **G.TINY}[name])
    for r in rows:
        assert r["n_far"] > 40000, r
        assert r["offsets_out_of_table"] == 0, f"corner_offsets addresses outside the table: {r}"
        if r["flags"] & LV_SUBONCE:
            # found by this sweep, as read from the code: one conditional subtract does not bring a far cell's dense index below rows
            assert r["generic_over"] > 0 and r["level_row_over"] > 0 and r["generic_max"] >= r["rows"], r
        else:
            assert r["flags"] & LV_POW2 and r["generic_over"] == 0 and r["level_row_over"] == 0, r
    if name == "fine":
        assert [bool(r["flags"] & LV_SUBONCE) for r in rows] == [False, True, True, True, True, False, False, False]
        assert rows[4]["rows"] == 357911 and rows[4]["res"] == 71
