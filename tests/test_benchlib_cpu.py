"""tools/benchlib.py and the command lines of the benchmark tools built on it, without a GPU: every tool imports whatever
the process's command line holds, no tool imports another tool, every parse_args keeps the positions and defaults the tools had
before they shared a library, the results writer, and the two statistics."""
import glob
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

NAMES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "bench_*.py"))) + ["trace_mesh_fill_area", "benchlib"]
MESH4 = dict(reps=5, resolution=512, voxels=256, frames=100)
# parse_args([]) of every tool: the positions (in this order) and defaults of the tools before they had a shared library
DEFAULTS = {
    "bench_mesh": dict(resolution=512, reps=5, ply=None),
    "bench_mesh_clean": MESH4, "bench_mesh_topology": MESH4, "bench_mesh_orient": MESH4, "bench_mesh_decimate": MESH4,
    "bench_mesh_simplify": MESH4, "bench_mesh_repair": MESH4,
    "bench_mesh_smooth": dict(MESH4, lattice=3000),
    "bench_mesh_fill": dict(MESH4, method="polar"),
    "bench_intersect": dict(reps=20, resolution=128, voxels=256, frames=100, brute_faces=8192),
    "bench_raycast": dict(reps=20, resolution=128, out=None),
    "bench_mesh_closest": dict(reps=5, resolution=512, out=None, legs="all"),
    "bench_mesh_eval": dict(reps=5, resolution=512),
    "bench_mesh_register": dict(reps=7, rows=[200000, 2000000]),
    "bench_cloud_normals": dict(reps=7, points=200000),
    "bench_flow_cues": dict(reps=7, out=None),
    "bench_patch_ssim": dict(reps=7),
    "bench_render_eval": dict(reps=5),
    "bench_hashenc": dict(B=8192 * 98),
    "bench_tsdf": dict(voxels=512, frames=1000, batch_frames=256, repeat=2, out=None, no_child=False),
    "bench_mesh_render": dict(model_res=512, room_voxels=256, views=32, visible_views=1000, reps=5, json=None),
    "trace_mesh_fill_area": dict(MESH4, summarise=None),
}
# a full positional command line of every tool that takes positionals, and what it must parse to
FULL = {
    "bench_mesh": (["64", "3", "m.ply"], dict(resolution=64, reps=3, ply="m.ply")),
    "bench_mesh_smooth": (["2", "64", "32", "8", "50"], dict(reps=2, resolution=64, voxels=32, frames=8, lattice=50)),
    "bench_mesh_fill": (["2", "64", "32", "8"], dict(reps=2, resolution=64, voxels=32, frames=8, method="polar")),
    "bench_intersect": (["4", "48", "32", "8", "512"], dict(reps=4, resolution=48, voxels=32, frames=8, brute_faces=512)),
    "bench_raycast": (["4", "48", "r.json"], dict(reps=4, resolution=48, out="r.json")),
    "bench_mesh_closest": (["2", "64", "c.json", "winding"], dict(reps=2, resolution=64, out="c.json", legs="winding")),
    "bench_mesh_eval": (["2", "64"], dict(reps=2, resolution=64)),
    "bench_mesh_register": (["3", "1000,20000"], dict(reps=3, rows=[1000, 20000])),
    "bench_cloud_normals": (["3", "5000"], dict(reps=3, points=5000)),
    "bench_flow_cues": (["3", "f.json"], dict(reps=3, out="f.json")),
    "bench_patch_ssim": (["3"], dict(reps=3)),
    "bench_render_eval": (["3"], dict(reps=3)),
    "bench_hashenc": (["9800"], dict(B=9800)),
    "trace_mesh_fill_area": (["2", "64", "32", "8"], dict(reps=2, resolution=64, voxels=32, frames=8, summarise=None)),
}
for _name in ("clean", "topology", "orient", "decimate", "simplify", "repair"):
    FULL["bench_mesh_" + _name] = (["2", "64", "32", "8"], dict(reps=2, resolution=64, voxels=32, frames=8))


@pytest.fixture(scope="module")
def tools():
    """every tool imported afresh under a command line none of them can parse"""
    argv, sys.argv = sys.argv, ["x", "not-a-number", "--bogus"]
    try:
        for name in NAMES:
            sys.modules.pop(name, None)
        return {name: importlib.import_module(name) for name in NAMES}
    finally:
        sys.argv = argv


def test_every_tool_is_covered(tools):
    assert set(DEFAULTS) == set(NAMES) - {"benchlib"}
    assert set(FULL) == set(DEFAULTS) - {"bench_tsdf", "bench_mesh_render"}            # (those two keep their argparse options)


def test_import_under_a_hostile_command_line(tools):
    for name, module in tools.items():
        assert module.__name__ == name
        if name != "benchlib":
            assert callable(module.parse_args) and callable(module.main), name


def test_no_tool_imports_another_tool():
    for name in NAMES:
        with open(os.path.join(TOOLS, name + ".py")) as fh:
            text = fh.read()
        assert not re.search(r"\b(import|from)\s+(bench_|trace_mesh_fill_area)", text), name
        assert not re.search(r"^(REPS|RES|TSDF_N|TSDF_FRAMES)\s*=", text, re.M), name
        for line in text.splitlines():                                        # the command line is read in main(), nowhere else
            if "sys.argv" in line:
                assert "sys.argv[1:] if argv is None else argv" in line, (name, line)


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_defaults(tools, name):
    got = vars(tools[name].parse_args([]))
    assert got == DEFAULTS[name]
    if name not in ("bench_tsdf", "bench_mesh_render", "trace_mesh_fill_area", "bench_mesh_fill"):
        assert list(got) == list(DEFAULTS[name]), "the order of the positionals"


@pytest.mark.parametrize("name", sorted(FULL))
def test_full_positional_list(tools, name):
    argv, want = FULL[name]
    assert vars(tools[name].parse_args(argv)) == want
    assert vars(tools[name].parse_args(argv + ["one", "more"])) == want, "what follows the last positional is ignored"
    for n in range(len(argv)):                                                # every prefix: the rest take their defaults
        got = vars(tools[name].parse_args(argv[:n]))
        assert got == {**DEFAULTS[name], **{k: want[k] for k in list(want)[:n]}}, n


def test_the_two_orders_of_resolution_and_reps_are_both_kept(tools):
    a, b = tools["bench_mesh"].parse_args(["64", "3"]), tools["bench_mesh_clean"].parse_args(["64", "3"])
    assert (a.resolution, a.reps) == (64, 3) and (b.reps, b.resolution) == (64, 3)


def test_options_of_the_argparse_tools(tools):
    a = tools["bench_tsdf"].parse_args(["--voxels", "64", "--frames", "16", "--batch-frames", "8", "--repeat", "1", "--out", "t.json", "--no-child"])
    assert vars(a) == dict(voxels=64, frames=16, batch_frames=8, repeat=1, out="t.json", no_child=True)
    a = tools["bench_mesh_render"].parse_args(["--model-res", "64", "--room-voxels", "0", "--views", "4", "--visible-views", "8", "--reps", "1",
                                              "--json", "r.json"])
    assert vars(a) == dict(model_res=64, room_voxels=0, views=4, visible_views=8, reps=1, json="r.json")
    assert vars(tools["trace_mesh_fill_area"].parse_args(["--summarise", "DIR"])) == dict(summarise="DIR")


def test_fill_takes_its_method_anywhere(tools):
    parse = tools["bench_mesh_fill"].parse_args
    want = dict(reps=2, resolution=64, voxels=32, frames=8, method="min_area")
    for at in range(5):
        argv = ["2", "64", "32", "8"]
        argv[at:at] = ["--method", "min_area"]
        assert vars(parse(argv)) == want, argv
    assert vars(parse(["--method", "auto", "3"])) == dict(MESH4, reps=3, method="auto")
    with pytest.raises(SystemExit):
        parse(["--method", "nonsense"])


def test_positionals_helper(tools):
    B = tools["benchlib"]
    a = B.positionals(["7", "x"], n=(int, 1), s=(str, "d"), f=(float, 0.5))
    assert vars(a) == dict(n=7, s="x", f=0.5) and list(vars(a)) == ["n", "s", "f"]
    with pytest.raises(ValueError):
        B.positionals(["not-a-number"], n=(int, 1))
    assert vars(B.mesh_positionals([], reps=20, resolution=128, extra=(int, 9))) == dict(reps=20, resolution=128, voxels=256, frames=100, extra=9)


def test_writer(tools, tmp_path, capsys, monkeypatch):
    B = tools["benchlib"]
    res = {"device": "d", "rows": {"a ms": 1.5, "n": [1, 2]}, "ok": True}
    want = json.dumps(res, indent=1)
    assert os.path.samefile(B.ROOT, ROOT)
    monkeypatch.setattr(B, "ROOT", str(tmp_path))                             # the default path is <root>/profiles/<name>
    path = tmp_path / "profiles" / "x_bench.json"
    assert B.write_results(res, "x_bench.json") == str(path)
    assert capsys.readouterr().out == want + "\n"
    assert path.read_text() == want + "\n" and json.loads(path.read_text()) == res
    explicit = tmp_path / "a" / "b" / "out.json"                              # an explicit path wins, and its directory is made
    B.write_results(res, "y_bench.json", str(explicit))
    assert explicit.read_text() == want + "\n" and not (tmp_path / "profiles" / "y_bench.json").exists()
    assert capsys.readouterr().out == want + "\n"
    B.write_results(res, path=str(tmp_path / "quiet.json"), echo=False)       # written, not printed
    assert capsys.readouterr().out == "" and (tmp_path / "quiet.json").read_text() == want + "\n"
    before = sorted(p.name for p in tmp_path.rglob("*"))
    B.write_results(res)                                                      # neither a name nor a path: only printed
    assert capsys.readouterr().out == want + "\n" and sorted(p.name for p in tmp_path.rglob("*")) == before
    monkeypatch.chdir(tmp_path)
    B.write_results(res, path="bare.json", echo=False)                        # a bare file name has no directory to make
    assert (tmp_path / "bare.json").read_text() == want + "\n"


def test_summaries(tools):
    B = tools["benchlib"]
    odd, even = [5.0, 1.0, 3.0], [4.0, 1.0, 3.0, 10.0]
    assert B.median(odd) == 3.0 and B.median(even) == 3.5                     # np.median: the mean of the two middle samples
    assert type(B.median(np.float32([1, 2]))) is float
    for ms in (odd, even, [2.0]):
        assert B.median(ms) == float(np.median(ms))
        assert B.median_min_max(ms) == (float(np.median(ms)), min(ms), max(ms))
    assert all(type(x) is float for x in B.median_min_max(np.float32(even)))
    assert sorted(odd)[len(odd) // 2] == B.median(odd)                        # the upper middle sample is the median of an odd count
