"""CPU: the host-side launch rules of the per-ray kernels (mipnerf_pl_amd/csrc/lane_buckets.hpp -- the very header every launcher of a
kernel templated on K includes) compiled with g++ into a stand-alone program: the samples-per-lane bucket of every sample count, the
dispatcher's compile-time constant, the sampler's draw step and the grid size."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostmath", "lane_buckets_host.cpp")
DRAWS = (2, 65, 129, 1025)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def lines(request, tmp_path_factory):
    """output lines of the program; `sanitized`: the same program built with AddressSanitizer and UBSan (host code only, its own main)"""
    exe = str(tmp_path_factory.mktemp("lane_buckets") / request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall"] + flags + [SRC, "-o", exe])
    out = subprocess.run([exe] + [str(n) for n in DRAWS], check=True, capture_output=True, text=True)
    assert out.stderr == ""
    return [l.split() for l in out.stdout.splitlines()]


def test_bucket_and_dispatch_for_every_sample_count(lines):
    rows = [tuple(map(int, l[1:])) for l in lines if l[0] == "B"]
    assert [r[0] for r in rows] == list(range(-1, 1031))
    for N, bucket, got, ok in rows:
        if 1 <= N <= 1024:
            want = min(k for k in (1, 2, 4, 8, 16) if k >= -(-N // 64))              # the smallest bucket >= ceil(N / 64)
            assert 64 * want >= N and (want == 1 or 64 * (want // 2) < N)
        else:
            want = 0                                                                   # none: nothing is launched
        assert bucket == want, N
        assert got == want and ok == (want != 0), N                                    # the callable saw exactly that constant, or was not called


def test_draw_step_is_the_double_arithmetic_rounded_once(lines):
    rows = {int(l[1]): (int(l[2]), int(l[3])) for l in lines if l[0] == "D"}
    assert sorted(rows) == sorted(DRAWS)
    eps32 = np.float64(np.float32(1.1920928955078125e-07))
    assert eps32 == np.finfo(np.float32).eps
    for n in DRAWS:
        s = np.float64(1.0) / np.float64(n)
        want = (np.float32(s), np.float32(s - eps32))
        assert rows[n] == tuple(int(w.view(np.uint32)) for w in want), n


def test_grid_covers_the_items(lines):
    (row,) = [l for l in lines if l[0] == "G"]
    assert [int(x) for x in row[1:]] == [0, 1, 1, 2, (2 ** 33 + 1 + 255) // 256]
