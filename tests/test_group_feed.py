"""CPU: the group feed of the ELAS engine's batch entries (stereo-vision_amd/csrc/group_feed.h): which group a worker of
a batch call gets next, in fixed round-robin shares or on demand from one atomic counter.  The header holds no HIP
call; tests/cxx/group_feed_check.cpp is built over it by g++ alone and lets K threads with random short sleeps draw
the groups of a call.

What is asserted is what the engine relies on, in both modes: every index in [0, ngroups) is handed out exactly once,
none lies outside, every worker's indices ascend, an exhausted feed stays exhausted; in fixed-share mode worker w gets
exactly w, w + K, w + 2 K, ...; on demand every worker's first group is its own index, so that none is left without
one while there are at least K groups.  The same program, built as a stand-alone executable under ThreadSanitizer,
runs the same cases without a report."""
import os
import subprocess

import pytest

import helpers as H

CHECK = os.path.join(H.ROOT, "tests", "cxx", "group_feed_check.cpp")
LANES = [1, 2, 3, 6, 16]


def cases():
    out = []
    for fixed in (0, 1):
        for k in LANES:
            for n in sorted({0, 1, max(k - 1, 0), k, k + 1, 2 * k + 1, 1000}):
                out.append((fixed, k, n, 17 * k + n))
    return out


def build(tmp_path_factory, flags):
    exe = str(tmp_path_factory.mktemp("group_feed") / "group_feed_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, CHECK, "-lpthread"])
    return exe


def run(exe, cs, env=None):
    text = "".join("%d %d %d %d\n" % c for c in cs)
    r = subprocess.run([exe], input=text.encode(), capture_output=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cs)
    res = []
    for line in lines:
        fields = line.split()
        assert fields[-1].startswith("end:")
        per = []
        for f in fields[:-1]:
            w, _, idx = f.partition(":")
            assert int(w) == len(per)
            per.append([int(x) for x in idx.split(",")] if idx else [])
        res.append((per, int(fields[-1][4:])))
    return res, r.stderr.decode()


def check(cs, res):
    for (fixed, k, n, _), (per, ends) in zip(cs, res):
        what = (fixed, k, n)
        assert len(per) == k, what
        assert ends == 3 * k, (what, "every worker saw the end three times, and no group after it", ends)
        flat = [i for w in per for i in w]
        assert all(0 <= i < n for i in flat), (what, "index out of range")
        assert sorted(flat) == list(range(n)), (what, "every group exactly once")
        for w, idx in enumerate(per):
            assert idx == sorted(idx) and len(set(idx)) == len(idx), (what, w, "ascending")
            if fixed:
                assert idx == list(range(w, n, k)), (what, w, "fixed shares: w + i * lanes")
            elif w < n:
                assert idx[0] == w, (what, w, "the first group of a worker is its own")
            else:
                assert idx == [], (what, w)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory, ["-fsanitize=undefined", "-fno-sanitize-recover=all"])


def test_the_sizes_the_engine_meets(exe):
    cs = cases()
    assert {c[2] for c in cs if c[1] == 6} >= {0, 1, 5, 7, 1000}        # 0, 1, lanes - 1, lanes + 1, 1000
    res, _ = run(exe, cs)
    check(cs, res)


def test_on_demand_follows_the_quicker_worker(exe):
    """what the mode is for: with sleeps between the draws the shares differ from the fixed ones (over 1000 groups and
    six threads equal shares by chance are out of the question), while the whole is still each group once"""
    cs = [(0, 6, 1000, s) for s in (1, 2, 3)]
    res, _ = run(exe, cs)
    check(cs, res)
    assert any([len(w) for w in per] != [len(range(k, 1000, 6)) for k in range(6)] for per, _ in res)


def test_under_thread_sanitizer(tmp_path_factory):
    """the same program as a stand-alone executable with -fsanitize=thread: no report, same properties"""
    tsan = build(tmp_path_factory, ["-fsanitize=thread"])
    cs = cases()
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    res, err = run(tsan, cs, env)
    assert "ThreadSanitizer" not in err, err[-3000:]
    check(cs, res)
