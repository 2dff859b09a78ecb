"""tests/host_program.py on two ten-line programs (host only, no GPU): a clean one builds and runs in every mode; one that reads an
element past a heap array passes plain and is caught under the address sanitizer -- the proof that the sanitized mode of the
*_host_cpu tests is instrumented; and a sanitizer that cannot start is a skip only if it reports no finding."""
import os
import stat

import pytest

import host_program as H

CLEAN = """\
#include <cstdio>
#include <thread>
#include <vector>
int main() {
    std::vector<int> a(8, 1), sum(2, 0);
    std::thread t([&] { for (int i = 0; i < 4; ++i) sum[0] += a[i]; });
    for (int i = 4; i < 8; ++i) sum[1] += a[i];
    t.join();
    std::printf("%d ok\\n", sum[0] + sum[1]);
    return 0;
}
"""
PAST_THE_END = """\
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    int n = argc > 1 ? std::atoi(argv[1]) : 8;
    int* volatile a = new int[8]();                              // (volatile: the allocation and its reads stay)
    int sum = 0;
    for (int i = 0; i <= n; ++i) sum += a[i < 8 ? i : 8];       // n = 8: one read of a[8]
    delete[] a;
    std::printf("%d ok\\n", sum == 0x7eadbeef);
    return 0;
}
"""


def _source(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


@pytest.mark.parametrize("sanitize", [None, "address,undefined", "thread"])
def test_a_clean_program_builds_and_runs(tmp_path, sanitize):
    exe = H.build(_source(tmp_path, "clean.cpp", CLEAN), tmp_path, sanitize, flags=("-pthread",))
    assert H.build(_source(tmp_path, "clean.cpp", CLEAN), tmp_path, sanitize, flags=("-pthread",)) is exe      # built once
    out = H.run(exe, [], 60, sanitize)
    assert out.returncode == 0 and out.stdout == "8 ok\n" and not out.stderr, out.stdout + out.stderr


def test_a_read_past_a_heap_array_passes_plain_and_is_caught_when_sanitized(tmp_path):
    src = _source(tmp_path, "past_the_end.cpp", PAST_THE_END)
    plain, san = H.build(src, tmp_path), H.build(src, tmp_path, "address,undefined")
    assert plain != san
    for n, caught in ((7, False), (8, True)):
        out = H.run(plain, [n], 60)
        assert out.returncode == 0 and out.stdout == "0 ok\n" and not out.stderr, out.stdout + out.stderr
        out = H.run(san, [n], 60, "address,undefined")
        if caught:
            assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and "ok" not in out.stdout, out.stdout + out.stderr
        else:
            assert out.returncode == 0 and out.stdout == "0 ok\n" and not out.stderr, out.stdout + out.stderr


STARTUPS = ["FATAL: ThreadSanitizer: unexpected memory mapping 0x5c9bd4d2b000-0x5c9bd4d4b000",
            "==7==ReserveShadowMemoryRange failed while trying to map 0xdfff0001000 bytes. Perhaps you're using ulimit -v",
            "==7==Shadow memory range interleaves with an existing memory mapping. ASan cannot proceed correctly. ABORTING."]
FINDINGS = ["WARNING: ThreadSanitizer: data race (pid=7)", "==7==ERROR: AddressSanitizer: heap-buffer-overflow on address 0x602000000030",
            "check.cpp:9:31: runtime error: signed integer overflow: 2147483647 + 1 cannot be represented in type 'int'"]


def _says(tmp_path, stderr, code):
    """a stand-in for a sanitized program: writes ``stderr`` and exits with ``code``"""
    (tmp_path / "stderr.txt").write_text(stderr)
    exe = tmp_path / "says.sh"
    exe.write_text(f"#!/bin/sh\ncat '{tmp_path}/stderr.txt' >&2\nexit {code}\n")
    os.chmod(exe, os.stat(exe).st_mode | stat.S_IXUSR)
    return str(exe)


@pytest.mark.parametrize("startup", STARTUPS, ids=["thread", "address-reserve", "address-interleave"])
def test_a_sanitizer_that_cannot_start_is_a_skip_unless_it_reports_a_finding(tmp_path, startup):
    assert H.startup_failure(startup + "\n") == startup
    with pytest.raises(pytest.skip.Exception, match="cannot start here"):
        H.run(_says(tmp_path, startup + "\n", 66), [], 60, "thread")
    assert H.run(_says(tmp_path, startup + "\n", 66), [], 60).returncode == 66          # (a plain run never skips)
    for finding in FINDINGS:
        for text in (finding + "\n" + startup + "\n", startup + "\n" + finding + "\n", finding + "\n"):
            assert H.startup_failure(text) is None
            out = H.run(_says(tmp_path, text, 66), [], 60, "thread")
            assert out.returncode == 66 and out.stderr == text
