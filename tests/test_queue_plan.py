"""CPU: the queue plan of the ELAS engine (stereo-vision_amd/csrc/queue_plan.h): which streams a lane owns, their
priority classes, and the stream every phase runs on.  The header holds no HIP call; tests/cxx/queue_plan_check.cpp is
built over it by g++ alone (undefined-behaviour checks armed) and prints the table for caps 1, 4, 8, 20, unset, for
priority ranges of one, two and three levels, for every plan and for the automatic choice.

What is asserted is what the engine relies on: at most three streams per lane and three classes per process, never
more than 12 hardware queues where a plan other than 0 is in effect, the one-stream layout for plan 0 and for a
one-level range, the same layout for every worker (it depends on the lane's parity only, and under plans 1 and 3 not
even on that), phases of one class on one stream, and the priority values of the classes inside the device's range."""
import os
import subprocess

import pytest

import helpers as H

CHECK = os.path.join(H.ROOT, "tests", "cxx", "queue_plan_check.cpp")
NORMAL, HIGH, LOW = 0, 1, 2
A, S, B = 0, 1, 2
RANGES = {1: (0, 0), 2: (0, -1), 3: (1, -1)}          # levels -> (least, greatest); HIP: numerically lower = higher priority
CAPS = ["1", "4", "8", "20", "-"]                     # "-": GPU_MAX_HW_QUEUES unset (= 4)
WORKERS = [1, 3, 6, 8]
BUDGET = 12


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("queue_plan") / "queue_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined",
                           "-fno-sanitize-recover=all", "-o", exe, CHECK])

    def run(cases):
        """cases: (least, greatest, cap text, workers, requested) -> list of dicts"""
        text = "".join("%d %d %s %d %d\n" % c for c in cases)
        out = subprocess.run([exe], input=text.encode(), check=True, capture_output=True).stdout.decode().splitlines()
        assert len(out) == len(cases)
        res = []
        for line in out:
            v = [int(x) for x in line.split()]
            q = dict(plan=v[0], streams=v[1], classes=v[2], queues=v[3], lane=[])
            for p in range(2):
                w = v[4 + 10 * p:14 + 10 * p]
                q["lane"].append(dict(n=w[0], cls=w[1:4], phase=w[4:7], prio=w[7:10]))
            res.append(q)
        return res
    return run


def all_cases():
    return [(RANGES[lv][0], RANGES[lv][1], cap, w, req)
            for lv in (1, 2, 3) for cap in CAPS for w in WORKERS for req in (-1, 0, 1, 2, 3, 4)]


def cap_of(text):
    return 4 if text == "-" else int(text)


def test_invariants_over_the_whole_table(table):
    cases = all_cases()
    for c, q in zip(cases, table(cases)):
        least, greatest, cap, workers, req = c
        assert 0 <= q["plan"] <= 4 and 1 <= q["streams"] <= 3 and 1 <= q["classes"] <= 3, (c, q)
        seen = set()
        for lane in q["lane"]:
            assert 1 <= lane["n"] <= 3 and lane["n"] <= q["streams"], (c, q)
            used = lane["cls"][:lane["n"]]
            assert len(set(used)) == lane["n"] and all(k in (NORMAL, HIGH, LOW) for k in used), (c, "one stream per class")
            assert lane["cls"][lane["n"]:] == [-1] * (3 - lane["n"])
            assert lane["phase"][A] == 0 and all(0 <= s < lane["n"] for s in lane["phase"]), (c, q)
            assert set(lane["phase"]) == set(range(lane["n"])), (c, "no stream without a phase")
            assert all(greatest <= p <= least for p in lane["prio"]), (c, q)
            for ph in (A, S, B):
                k = used[lane["phase"][ph]]
                want = greatest if k == HIGH else least if k == LOW else 0
                assert lane["prio"][ph] == want, (c, q)
            seen |= set(used)
        assert q["classes"] == len(seen), (c, q)
        if q["plan"] != 0:
            assert q["queues"] <= BUDGET, (c, q)
        # queues: per class min(cap, streams of that class over 2 x workers lanes)
        per = {}
        for lane in q["lane"]:
            for k in lane["cls"][:lane["n"]]:
                per[k] = per.get(k, 0) + workers
        assert q["queues"] == sum(min(cap_of(cap), n) for n in per.values()), (c, q)


def test_plan_0_and_a_one_level_range_are_one_normal_stream(table):
    cases = [c for c in all_cases() if c[4] == 0 or (c[0], c[1]) == RANGES[1]]
    assert len(cases) > 100
    for c, q in zip(cases, table(cases)):
        assert q["plan"] == 0 and q["streams"] == 1 and q["classes"] == 1, (c, q)
        for lane in q["lane"]:
            assert lane == dict(n=1, cls=[NORMAL, -1, -1], phase=[0, 0, 0], prio=[0, 0, 0]), (c, q)


def test_layout_does_not_depend_on_the_worker(table):
    """the layout is a function of the lane's parity alone: batch_impl hands groups out in static round-robin shares,
    so no worker may sit in a lower class than another.  Plans 1 and 3 do not even depend on the parity."""
    for lv in (2, 3):
        for cap in ("1", "4", "-"):
            for req in (1, 2, 3, 4):
                qs = table([(RANGES[lv][0], RANGES[lv][1], cap, w, req) for w in (1, 2, 3)])
                assert all(q["lane"] == qs[0]["lane"] and q["plan"] == qs[0]["plan"] for q in qs), (lv, cap, req)
                if req in (1, 3):
                    assert qs[0]["lane"][0] == qs[0]["lane"][1]


def test_the_three_layouts_at_three_levels_and_a_cap_of_4(table):
    least, greatest = RANGES[3]
    q1, q2, q3 = table([(least, greatest, "4", 6, r) for r in (1, 2, 3)])
    stage_high = dict(n=2, cls=[NORMAL, HIGH, -1], phase=[0, 1, 0], prio=[0, -1, 0])
    assert (q1["plan"], q1["streams"], q1["classes"], q1["queues"]) == (1, 2, 2, 8)
    assert q1["lane"] == [stage_high, stage_high]
    assert (q2["plan"], q2["streams"], q2["classes"], q2["queues"]) == (2, 2, 3, 12)
    assert q2["lane"] == [stage_high, dict(n=2, cls=[LOW, HIGH, -1], phase=[0, 1, 0], prio=[1, -1, 1])]
    by_phase = dict(n=3, cls=[NORMAL, HIGH, LOW], phase=[0, 1, 2], prio=[0, -1, 1])
    assert (q3["plan"], q3["streams"], q3["classes"], q3["queues"]) == (3, 3, 3, 12)
    assert q3["lane"] == [by_phase, by_phase]
    # the layout that keeps a group on one stream: second lanes low
    q4 = table([(least, greatest, "4", 6, 4)])[0]
    one = dict(n=1, cls=[NORMAL, -1, -1], phase=[0, 0, 0], prio=[0, 0, 0])
    assert (q4["plan"], q4["streams"], q4["classes"], q4["queues"]) == (4, 1, 2, 8)
    assert q4["lane"] == [one, dict(n=1, cls=[LOW, -1, -1], phase=[0, 0, 0], prio=[1, 1, 1])]


def test_two_levels_fold_the_missing_class_into_normal(table):
    # (0, -1): normal and high exist, low folds.  (1, 0): normal and low exist, high folds.
    q1, q2, q3 = table([(0, -1, "4", 6, r) for r in (1, 2, 3)])
    stage_high = dict(n=2, cls=[NORMAL, HIGH, -1], phase=[0, 1, 0], prio=[0, -1, 0])
    assert q1["lane"] == q2["lane"] == q3["lane"] == [stage_high, stage_high]        # phases A and B share the normal stream
    assert [q["classes"] for q in (q1, q2, q3)] == [2, 2, 2]
    p1, p2, p3 = table([(1, 0, "4", 6, r) for r in (1, 2, 3)])
    one = dict(n=1, cls=[NORMAL, -1, -1], phase=[0, 0, 0], prio=[0, 0, 0])
    assert p1["plan"] == 0 and p1["lane"] == [one, one]                               # nothing left of plan 1
    # (the second lane's main stream is low; its stage chain, with no high class to go to, is normal)
    assert p2["lane"] == [one, dict(n=2, cls=[LOW, NORMAL, -1], phase=[0, 1, 0], prio=[1, 0, 1])] and p2["classes"] == 2
    post_low = dict(n=2, cls=[NORMAL, LOW, -1], phase=[0, 0, 1], prio=[0, 0, 1])
    assert p3["lane"] == [post_low, post_low]


def test_the_queue_budget_turns_a_plan_into_plan_0(table):
    least, greatest = RANGES[3]
    # six workers: 12 lane streams.  cap 8: plan 1 would hold 8 + 8, plans 2 and 3 more; cap 20: 12 per class
    for cap in ("8", "20"):
        for q in table([(least, greatest, cap, 6, r) for r in (1, 2, 3)]):
            assert q["plan"] == 0 and q["streams"] == 1 and q["classes"] == 1, (cap, q)
        q = table([(least, greatest, cap, 6, 4)])[0]         # (six normal + six low lane streams: a queue each)
        assert q["plan"] == 4 and q["queues"] == 12
    # three workers at a cap of 8: 6 + 6 fits
    q = table([(least, greatest, "8", 3, 1)])[0]
    assert q["plan"] == 1 and q["queues"] == 12
    # a cap of 1: one queue per class
    assert [q["queues"] for q in table([(least, greatest, "1", 6, r) for r in (0, 1, 2, 3, 4)])] == [1, 2, 3, 3, 2]


def test_automatic_choice(table):
    least, greatest = RANGES[3]
    # a queue per lane stream (2 x workers) or more: today's layout
    for cap, workers in (("20", 6), ("8", 4), ("4", 2), ("-", 2), ("12", 6)):
        assert table([(least, greatest, cap, workers, -1)])[0]["plan"] == 0, (cap, workers)
    # fewer: the plan the A/B kept, which is the same plan for every such cap and worker count -- and, whichever it
    # is, within the invariants above (a request out of range is the automatic choice)
    short = table([(least, greatest, cap, 6, req) for cap in ("1", "4", "-", "8") for req in (-1, -7, 5)])
    kept = {q["plan"] for q in short[:9]}                    # caps 1, 4 and unset
    assert len(kept) == 1 and kept <= {0, 1, 2, 3, 4}
    assert all(q["plan"] in kept | {0} for q in short[9:])   # cap 8 with six workers: the kept plan if it fits the budget


def test_cap_text_as_the_runtime_reads_it(table):
    least, greatest = RANGES[3]
    got = [q["queues"] for q in table([(least, greatest, t, 6, 0) for t in ("-", "0", "-3", "abc", "4", "7", "20", "99999")])]
    assert got == [4, 4, 4, 4, 4, 7, 12, 12]
