"""The pass bodies the fan-split kernels run (csrc/manifold_passes.hpp on uf_passes.hpp), compiled as host C++ into a stand-alone
program (tests/manifold_host_check.cpp) and run by 8 threads on host-built edge tables: every output array and total equals the
sequential oracle tests/manifold_ref.py element for element.  Once plain, once under the address and undefined-behaviour sanitizers
and once under the thread sanitizer, where the host compiler has them.  No GPU."""
import numpy as np
import pytest

import host_program
import manifold_ref as M


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
    exe = host_program.build("manifold_host_check.cpp", tmp_path, sanitize, flags=("-pthread",))
    run = host_program.run(exe, [cases_file, "8"], 600, sanitize)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    assert f"{len(M.kernel_cases())} cases" in run.stdout
