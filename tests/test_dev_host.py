"""The owners of device memory and timing events in the library's host code (csrc/avsim_dev.h: DevBuf, DevArena, EventTimer) and the staging ring built
on them (csrc/avsim_stage.h) against a counting stand-in for the HIP runtime, as a program of its own (tests/hostshim_io/dev_main.cpp) built with
AddressSanitizer, LeakSanitizer and UBSan: a buffer grows only for a larger size and then to exactly that size, a failed allocation leaves it empty and
usable, a set-up whose n-th allocation fails stops there and frees exactly what it got, the timer keeps at most EV_RING event pairs however long the run
and counts only complete pairs, and nothing leaks on any of these paths."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
STATIC = ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it runs the same whatever else a machine loads into every process


def _build(out, flags):
    shim = os.path.join(ROOT, "tests", "hostshim_io")
    cmd = ["g++", "-std=c++17", "-pthread", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + shim, "-I" + os.path.join(ROOT, "av_aloha_amd", "csrc"),
           os.path.join(shim, "dev_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_device_owners_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dev_main")
    built = _build(exe, SAN + STATIC)
    if built.returncode != 0:
        built = _build(exe, SAN)
    sanitized = built.returncode == 0
    if not sanitized:
        # only a missing sanitizer runtime excuses the flags; anything else the plain build below reports as well
        assert "asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr, built.stderr
        plain = _build(exe, [])
        assert plain.returncode == 0, plain.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("dev ok")
    if not sanitized:
        pytest.xfail("the sanitizer runtimes are missing here: dev_main passed, but built WITHOUT -fsanitize=address,undefined:\n" + built.stderr[-400:])
