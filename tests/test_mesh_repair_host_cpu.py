"""The pass bodies the fan-split kernels run (csrc/manifold_passes.hpp on uf_passes.hpp), compiled as host C++ into a stand-alone
program (tests/manifold_host_check.cpp) and run by 8 threads on host-built edge tables: every output array and total equals the
sequential oracle tests/manifold_ref.py element for element.  Once plain, once under the address and undefined-behaviour sanitizers
and once under the thread sanitizer, where the host compiler has them.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import manifold_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("manifold") / "cases.txt")
    row = lambda a: " ".join(str(int(x)) for x in np.asarray(a).reshape(-1)) + "\n"
    with open(path, "w") as fh:
        for name, f, V, kw in M.kernel_cases():
            r = M.split_fans(f, V, **kw)
            fh.write(f"{name.replace(' ', '_')} {V} {len(f)} {int(kw.get('cut_inconsistent', False))} {int('labels' in kw)} "
                     f"{int('face_mask' in kw)}\n")
            fh.write(row(f) + row(kw.get("labels", [])) + row(kw.get("face_mask", [])))
            fh.write(row(r["corner_fan"]) + row(r["vertex_fans"]) + row(r["faces"]) + f"{r['n_new']}\n" + row(r["new_source"]))
            fh.write(row(M.totals_of(r)))
    return path


@pytest.mark.parametrize("sanitize", [None, "address,undefined", "thread"])
def test_fan_split_passes_on_host_threads(tmp_path, cases_file, sanitize):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    assert cxx, "no host C++ compiler (the oracle's Makefile needs one as well)"
    exe = str(tmp_path / "manifold_host_check")
    cmd = [cxx, "-O1" if sanitize else "-O2", "-g", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "manifold_host_check.cpp"),
           "-o", exe]
    if sanitize:
        probe = subprocess.run(cmd + [f"-fsanitize={sanitize}", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip(f"host compiler without -fsanitize={sanitize}")
    else:
        subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="exitcode=67", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, cases_file, "8"], capture_output=True, text=True, env=env, timeout=600)
    if sanitize and ("FATAL: ThreadSanitizer" in run.stderr and "data race" not in run.stderr
                     or "ReserveShadowMemoryRange failed" in run.stderr or "Shadow memory range interleaves" in run.stderr):
        pytest.skip("the sanitizer cannot start here: " + run.stderr.strip().splitlines()[-1])
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    assert f"{len(M.kernel_cases())} cases" in run.stdout
