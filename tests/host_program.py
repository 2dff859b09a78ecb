"""Compile a tests/*_host_check.cpp with the host compiler and run it (test infrastructure): the kernels' *_passes.hpp bodies and index
arithmetic as stand-alone host programs, plain or under a sanitizer ("address,undefined" or "thread"), held to the Python references
by the test modules that call this.  tests/test_host_program_cpu.py proves that the sanitized mode is really instrumented."""
import functools
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = ("address,undefined", "thread")
# what a sanitizer says when it cannot lay out its shadow memory in this address space (before main()), and what it says when it
# has found something in the program: only the first without the second is a reason to skip
STARTUP = ("FATAL: ThreadSanitizer", "ReserveShadowMemoryRange failed", "Shadow memory range interleaves")
FINDINGS = ("data race", "WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")
_built = {}

words = lambda a: " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))
bits32 = lambda a: words(np.ascontiguousarray(a, np.float32).view(np.uint32))
bits64 = lambda a: words(np.ascontiguousarray(a, np.float64).view(np.uint64))


def build(source_name, tmp, sanitize=None, flags=()):
    """tests/<source_name> (or an absolute path) -> executable under ``tmp``, built once per (source, tmp, sanitize): -O2 -g plain,
    -O1 -g -fsanitize=<sanitize> -fno-sanitize-recover=all otherwise; a compiler without that sanitizer skips the test"""
    assert sanitize is None or sanitize in SANITIZERS, sanitize
    key = (source_name, str(tmp), sanitize)
    if key not in _built:
        cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
        assert cxx, "no host C++ compiler (the oracle's Makefile needs one as well)"
        stem = os.path.splitext(os.path.basename(source_name))[0]
        exe = os.path.join(str(tmp), stem + ("_" + sanitize.replace(",", "_") if sanitize else ""))
        cmd = [cxx, "-O1" if sanitize else "-O2", "-g", "-std=c++17", *flags, os.path.join(ROOT, "tests", source_name), "-o", exe]
        if sanitize:
            if subprocess.run(cmd + [f"-fsanitize={sanitize}", "-fno-sanitize-recover=all"], capture_output=True, text=True).returncode != 0:
                pytest.skip(f"host compiler without -fsanitize={sanitize}")
        else:
            subprocess.run(cmd, check=True)
        _built[key] = exe
    return _built[key]


@functools.lru_cache(maxsize=None)
def _no_randomisation():
    """the prefix that starts a program with address randomisation off, [] where that cannot be done"""
    setarch = shutil.which("setarch")
    prefix = [setarch, platform.machine(), "-R"] if setarch else []
    if prefix and subprocess.run(prefix + ["true"], capture_output=True).returncode != 0:
        return []
    return prefix


def startup_failure(stderr):
    """-> the sanitizer's own message if it could not start (and reports no finding), else None"""
    if any(s in stderr for s in STARTUP) and not any(f in stderr for f in FINDINGS):
        return stderr.strip().splitlines()[-1]
    return None


def run(exe, args, timeout, sanitize=None, env=None):
    """-> the completed process (stdout, stderr as text); the caller states what success is.  A sanitized program starts with
    address randomisation off: the sanitizer's shadow memory needs the address space laid out its way, and with many bits of
    randomisation its start-up can die before main() (a FATAL line, or a bare SIGSEGV).  If it still cannot start, and only then,
    the test is skipped with the sanitizer's message."""
    env = dict(os.environ if env is None else env)
    prefix = []
    if sanitize:
        env.update(TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="exitcode=67", UBSAN_OPTIONS="halt_on_error=1")
        prefix = _no_randomisation()
    out = subprocess.run(prefix + [exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=timeout)
    if sanitize:
        why = startup_failure(out.stderr)
        if why:
            pytest.skip("the sanitizer cannot start here: " + why)
    return out
