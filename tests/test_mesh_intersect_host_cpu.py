"""The bodies the self-intersection kernels call (csrc/intersect_passes.hpp), compiled by the host compiler with -ffp-contract=off into
tests/intersect_host_check.cpp: the 256-bit integer against Python's, products compared bit for bit at every limb boundary; the
fp32 -> integer conversion; the stage-1 / stage-2 decisions against tests/intersect_ref.py on the known pairs and the lattice soup.
Once plain and once under the address and undefined-behaviour sanitizers where the host compiler has them."""
import functools
import random

import numpy as np
import pytest

import host_program
import intersect_ref as R

M = 1 << 256


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("intersect_host_check.cpp", tmp_path_factory.mktemp("intersect_host"), sanitize, flags=("-ffp-contract=off",))

    def call(path, lines):
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        out = host_program.run(exe, [str(path)], 300, sanitize)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
        got = out.stdout.split("\n")[:-1]
        assert len(got) == len(lines)
        return got
    return call


def _signed(x):
    return 0 if x == 0 else (-1 if x >> 255 else 1)


def test_wide_integer_equals_python(run, tmp_path):
    rnd = random.Random(11)
    widths = [w + d for w in range(0, 257, 32) for d in (-1, 0, 1) if 0 < w + d <= 256]
    lines, want = [], []
    for na in widths:
        for nb in widths:
            for sa, sb in ((1, 1), (-1, 1), (-1, -1)):
                a, b = sa * (rnd.getrandbits(na) | 1 << (na - 1)) % M, sb * (rnd.getrandbits(nb) | 1 << (nb - 1)) % M
                for op, r in (("add", a + b), ("sub", a - b), ("mul", a * b)):
                    lines.append(f"w {op} {a:064x} {b:064x}")
                    want.append(f"{r % M:064x} {_signed(r % M)}")
    for a, b in ((0, 0), (M - 1, M - 1), (M - 1, 1), (1 << 255, 1), ((1 << 128) - 1, (1 << 128) - 1), ((1 << 32) - 1, (1 << 32) - 1)):
        for op, r in (("add", a + b), ("sub", a - b), ("mul", a * b)):
            lines.append(f"w {op} {a:064x} {b:064x}")
            want.append(f"{r % M:064x} {_signed(r % M)}")
    assert run(tmp_path / "wide.txt", lines) == want


def test_coordinates_become_integers(run, tmp_path):
    xs = np.array([1.0, -1.0, 0.0, -0.0, 1.5, 2.0 ** -149, -2.0 ** -126, 3.0 * 2.0 ** -140, 2.0 ** 23 + 1, -16777215.0, 0.1, 2.0 ** 60],
                  np.float32)
    lines, want = [], []
    for x in xs:
        num, den = float(x).as_integer_ratio()
        e = -149 if x == 0 else min(e for e in range(-149, 128) if (num * 2 ** -e if e < 0 else num) % (den * (2 ** e if e > 0 else 1)) == 0
                                    and abs(num) * 2 ** 149 // den >> (e + 149) < 1 << 24)
        for E in (e, e - 1, e - 31, e - 32, e - 59, e - 102):
            lines.append(f"c {int(np.array([x]).view(np.uint32)[0])} {E}")
            want.append(f"{int(float(x) * 2.0 ** -E) % M if abs(E) < 900 else 0:064x}")
    assert run(tmp_path / "coord.txt", lines) == want


def _pair_line(a, b):
    return "p " + " ".join(str(int(x)) for x in np.concatenate([a.reshape(-1), b.reshape(-1)]).view(np.uint32))


def test_known_pairs(run, tmp_path):
    cases = R.known_answers()
    names = sorted(cases)
    got = run(tmp_path / "pairs.txt", [_pair_line(*cases[n][:2]) for n in names] + [_pair_line(*R.unresolved_case()[:2])])
    for n, g in zip(names, got):
        a, b, kind, coplanar, s = cases[n]
        want = R.code_of(kind, coplanar, s) if kind else 0
        code, s_got, stage, exact = (int(x) for x in g.split())
        assert (code, s_got, exact) == (want, s, want) and stage in (1, 2), (n, g)
    code, s_got, stage, exact = (int(x) for x in got[-1].split())
    assert (code & 3, stage, exact & 3) == (R.UNRESOLVED, 3, R.UNRESOLVED)


@functools.lru_cache(maxsize=None)
def _soups():
    out = []
    for mesh in (R.lattice_soup(), R.lattice_soup(40, 5, (3.25, -1.5, 100.0)), R.random_soup(150, 7)):
        v, f = mesh["verts"], mesh["faces"]
        cand = R.candidates(v, f)
        out.append((v, f, cand, [R.pair(v[f[i]], v[f[j]]) for i, j in cand]))
    return out


def test_soups_filter_is_sound_and_exact_stage_is_complete(run, tmp_path):
    n_filter = n_exact = 0
    for v, f, cand, want in _soups():
        got = run(tmp_path / "soup.txt", [_pair_line(v[f[i]], v[f[j]]) for i, j in cand])
        for g, w, (i, j) in zip(got, want, cand):
            code, s, stage, exact = (int(x) for x in g.split())
            assert code == w and exact == w and s == R.shared_positions(v[f[i]], v[f[j]]) and stage in (1, 2), (i, j, g, w)
            n_filter += stage == 1
            n_exact += stage == 2
    assert n_filter > 200 and n_exact > 200                                # both stages did decide pairs


def test_collinear_faces(run, tmp_path):
    faces = [np.array([(0, 0, 0), (1, 2, 3), (3, 6, 9)], np.float32), R.collinear_case(),
             np.array([(0, 0, 0), (1, 2, 3), (3, 6, np.nextafter(np.float32(9), np.float32(10)))], np.float32),
             np.array([(2.0 ** -120, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)]
    got = run(tmp_path / "faces.txt", ["f " + " ".join(str(int(x)) for x in t.reshape(-1).view(np.uint32)) for t in faces])
    assert got == ["1", "1", "0", "-1"]
